"""Restatement of csrc_recon/meshdecim.hip (test oracle) and the scenes of tests/test_mesh_decimate_{cpu,gpu}.py, written from the statements
of include/v3d_recon.h "Mesh decimation".  Plain Python over numpy scalars: fp64 by default; `dtype=np.float32` runs the same statements, in
the same order, in single precision (what that run loses against the fp64 one is the cost of the number format).  Every sum over a vertex's
list adds the entries in list order (ascending corner 3 f + k).  A mesh in flight is a list of faces, None for a dead one."""
from __future__ import annotations

import functools
import math

import numpy as np
import torch

import mesh_clean_ref as C
import mesh_render_ref as M
import recon_geom_ref as R

NO_KEY = 2 ** 64 - 1
DEFAULT_MAX_VALENCE = 24


# ---- numbers --------------------------------------------------------------------------------------------------------------------------------
def _scalar(dtype):
    return float if np.dtype(dtype) == np.float64 else np.float32


def _positions(verts, dtype):
    """[V] tuples of scalars of `dtype` (float32 positions are exact in either)"""
    T = _scalar(dtype)
    return [tuple(T(x) for x in row) for row in np.asarray(verts, dtype=np.float32).tolist()]


def _sqrt(x):
    return math.sqrt(x) if isinstance(x, float) else np.sqrt(x)


def face_cross(p0, p1, p2):
    """(p1 - p0) x (p2 - p0)"""
    ux, uy, uz = p1[0] - p0[0], p1[1] - p0[1], p1[2] - p0[2]
    wx, wy, wz = p2[0] - p0[0], p2[1] - p0[1], p2[2] - p0[2]
    return uy * wz - uz * wy, uz * wx - ux * wz, ux * wy - uy * wx


def cost_bits(cost) -> int:
    """The fp32 bits of a cost, clamped at 0"""
    c = np.float32(cost)
    if c < 0:
        c = np.float32(0.0)
    return int(np.asarray(c, dtype=np.float32).view(np.uint32))


def bits_cost(bits: int) -> float:
    return float(np.asarray(bits, dtype=np.uint32).view(np.float32))


# ---- lists ----------------------------------------------------------------------------------------------------------------------------------
def face_list(faces):
    """list of (i0, i1, i2) of python ints from a [F, 3] array"""
    return [tuple(int(i) for i in row) for row in np.asarray(faces).reshape(-1, 3).tolist()]


def stars(faces, V):
    """star[v]: the entries (f, k, next, prev) of v's list, in list order; dead faces (None) are absent"""
    out = [[] for _ in range(V)]
    for f, tri in enumerate(faces):
        if tri is None:
            continue
        for k in range(3):
            out[tri[k]].append((f, k, tri[(k + 1) % 3], tri[(k + 2) % 3]))
    return out


def neighbours(star):
    """per vertex the set of its neighbours"""
    return [{x for _, _, a, b in s for x in (a, b)} for s in star]


# ---- quadrics -------------------------------------------------------------------------------------------------------------------------------
def face_quadric(P, tri, T):
    p0 = P[tri[0]]
    nx, ny, nz = face_cross(p0, P[tri[1]], P[tri[2]])
    len2 = nx * nx + ny * ny + nz * nz
    if not len2 > 0:
        return None
    ln = _sqrt(len2)
    a, b, c = nx / ln, ny / ln, nz / ln
    d = -(a * p0[0] + b * p0[1] + c * p0[2])
    w = T(0.5) * ln
    return [w * (a * a), w * (a * b), w * (a * c), w * (a * d), w * (b * b), w * (b * c), w * (b * d), w * (c * c), w * (c * d), w * (d * d)]


def vertex_quadrics(verts, faces, dtype=np.float64):
    """Q [V, 10] of `dtype`: the sum in list order of the area-weighted plane quadrics of every vertex's faces"""
    T = _scalar(dtype)
    P = _positions(verts, dtype)
    faces = face_list(faces) if not isinstance(faces, list) else faces
    fq = [face_quadric(P, tri, T) if tri is not None else None for tri in faces]
    Q = [[T(0.0)] * 10 for _ in P]
    for v, s in enumerate(stars(faces, len(P))):
        for f, _, _, _ in s:
            if fq[f] is not None:
                Q[v] = [x + y for x, y in zip(Q[v], fq[f])]
    return np.asarray(Q, dtype=dtype).reshape(len(P), 10)


def collapse_cost(P, Qv, Qu, u):
    """(Q_v + Q_u)(p_u), in the scalars of P and the rows"""
    q = [a + b for a, b in zip(Qv, Qu)]
    x, y, z = P[u]
    return (x * (q[0] * x + q[1] * y + q[2] * z + q[3]) + y * (q[1] * x + q[4] * y + q[5] * z + q[6]) +
            z * (q[2] * x + q[5] * y + q[7] * z + q[8]) + (q[3] * x + q[6] * y + q[8] * z + q[9]))


# ---- propose --------------------------------------------------------------------------------------------------------------------------------
def removable(v, s, max_valence):
    """v's star is one closed fan of 3 .. max_valence faces"""
    n = len(s)
    if n < 3 or n > max_valence:
        return False
    step = {}
    for _, _, a, b in s:
        if a == v or b == v or a == b or a in step:
            return False
        step[a] = b
    if len(set(step.values())) != n or set(step.values()) != set(step):
        return False
    first = s[0][2]
    x, steps = step[first], 1
    while x != first and steps <= n:
        x, steps = step[x], steps + 1
    return steps == n


def analyse(verts, faces, Q, max_valence=DEFAULT_MAX_VALENCE, dtype=np.float64, only=None):
    """Per vertex None (not removable) or {u: {"why": the set of rules v -> u breaks ("link", "valence", "flip", "duplicate"), "cost": in
    `dtype`, "dots": n_before . n_after of every surviving face}} over its neighbours in list order.  Q rows are used in `dtype`."""
    T = _scalar(dtype)
    P = _positions(verts, dtype)
    V = len(P)
    star = stars(faces, V)
    nbr = neighbours(star)
    Qr = [[T(x) for x in row] for row in np.asarray(Q).tolist()]
    out = [None] * V
    for v in (range(V) if only is None else only):
        s = star[v]
        if not removable(v, s, max_valence):
            continue
        info = {}
        for _, _, u, a1 in s:                                   # the face (v, u, a1); the face (v, a2, u)
            a2 = next(a for _, _, a, b in s if b == u)
            why = set()
            if a1 == a2 or (nbr[v] & nbr[u]) - {u} != {a1, a2}:
                why.add("link")
            if len(star[u]) + len(s) - 4 > max_valence:
                why.add("valence")
            at_u = {frozenset((a, b)) for _, _, a, b in star[u]}
            dots = []
            for f, k, a, b in s:
                if a == u or b == u:
                    continue
                tri = faces[f]
                pts = [P[i] for i in tri]
                before = face_cross(*pts)
                pts[k] = P[u]
                after = face_cross(*pts)
                dots.append(before[0] * after[0] + before[1] * after[1] + before[2] * after[2])
                if not dots[-1] > 0:
                    why.add("flip")
                if frozenset((a, b)) in at_u:
                    why.add("duplicate")
            cost = collapse_cost(P, Qr[v], Qr[u], u)
            if not cost == cost:
                why.add("nan")
            info[u] = {"why": why, "cost": cost, "dots": dots}
        out[v] = info
    return out


def clear_of_the_flip_threshold(i64, i32):
    """Per vertex, from the analyses of both precisions: every n_before . n_after of every one of its collapses lies further from 0 than the
    float32 run is off (where it does not, float32 may decide a flip the other way), or is exactly 0 in both (the flat grid, where every
    product is exact in either precision: both refuse the face without area)"""
    out = []
    for c64, c32 in zip(i64, i32):
        out.append(c64 is None or all(abs(d) > abs(float(e) - d) or d == 0.0 == float(e) for u in c64 for d, e in zip(c64[u]["dots"], c32[u]["dots"])))
    return out


def propose(verts, faces, Q, max_valence=DEFAULT_MAX_VALENCE, dtype=np.float64, info=None):
    """(keys [V] python ints, targets [V]): the cheapest valid neighbour by fp32 cost bits, the smaller index among equals"""
    info = analyse(verts, faces, Q, max_valence, dtype) if info is None else info
    keys, targets = [], []
    for v, cand in enumerate(info):
        best = None
        for u, c in (cand or {}).items():
            if not c["why"]:
                k = (cost_bits(c["cost"]), u)
                best = k if best is None or k < best else best
        keys.append(NO_KEY if best is None else (best[0] << 32) | v)
        targets.append(-1 if best is None else best[1])
    return keys, targets


# ---- select, cut, apply ---------------------------------------------------------------------------------------------------------------------
def min_round(faces, keys):
    out = list(keys)
    for tri in faces:
        if tri is not None:
            m = min(keys[tri[0]], keys[tri[1]], keys[tri[2]])
            for i in tri:
                out[i] = min(out[i], m)
    return out


def select(faces, keys, max_bits=None):
    """accept [V] of 0 / 1: the key is not all ones, the smallest within graph distance 2, and its cost bits are at most max_bits"""
    m2 = min_round(faces, min_round(faces, keys))
    return [int(k != NO_KEY and m == k and (max_bits is None or (k >> 32) <= max_bits)) for k, m in zip(keys, m2)]


def cut(keys, accept, live, target):
    quota = max(0, (live - target + 1) // 2)
    order = sorted(v for v, a in enumerate(accept) if a)
    order.sort(key=lambda v: keys[v])
    out = [0] * len(accept)
    for v in order[:quota]:
        out[v] = 1
    return out


def apply(faces, accept, targets, Q):
    """(faces with None for the dead, Q after Q_u += Q_v); Q is a [V, 10] array and is copied"""
    out = []
    for tri in faces:
        if tri is not None:
            hit = [k for k in range(3) if accept[tri[k]]]
            if hit:
                k = hit[0]
                u = targets[tri[k]]
                tri = None if u in tri else tuple(u if j == k else tri[j] for j in range(3))
        out.append(tri)
    Q = np.array(Q, copy=True)
    for v, a in enumerate(accept):
        if a:
            Q[targets[v]] = Q[targets[v]] + Q[v]
    return out, Q


# ---- the loop -------------------------------------------------------------------------------------------------------------------------------
def decimate(verts, faces, target, max_valence=DEFAULT_MAX_VALENCE, max_bits=None, dtype=np.float64, incremental=True):
    """(kept [Vo] old vertex indices ascending, faces [Fo, 3] in the new indices, stats): rounds of propose, select, cut and apply until the
    target is reached or a round accepts nothing.  Only the vertices whose proposal can have changed are looked at again: those within
    distance 2 of a vertex whose star or quadric the round changed (a proposal reads the stars of v and of its neighbours); incremental=False
    looks at every vertex in every round."""
    faces = face_list(faces)
    V = np.asarray(verts).shape[0]
    Q = vertex_quadrics(verts, faces, dtype)
    live = len(faces)
    removed = [False] * V
    stats = {"rounds": 0, "accepted": [], "reached": live <= target, "max_cost": 0.0, "faces_before": live}
    info, dirty = [None] * V, range(V)
    while live > target:
        fresh = analyse(verts, faces, Q, max_valence, dtype, only=dirty)
        for v in dirty:
            info[v] = fresh[v]
        keys, targets = propose(verts, faces, Q, max_valence, dtype, info=info)
        accept = cut(keys, select(faces, keys, max_bits), live, target)
        n = sum(accept)
        if n == 0:
            break
        nbr = neighbours(stars(faces, V))
        touched = set()
        for v, a in enumerate(accept):
            if a:
                removed[v] = True
                touched |= {v, targets[v]} | nbr[v]
                stats["max_cost"] = max(stats["max_cost"], bits_cost(keys[v] >> 32))
        faces, Q = apply(faces, accept, targets, Q)
        nbr = neighbours(stars(faces, V))
        ring1 = set(touched)
        for v in touched:
            ring1 |= nbr[v]
        dirty = set(ring1)
        for v in ring1:
            dirty |= nbr[v]
        dirty = sorted(dirty) if incremental else range(V)
        live -= 2 * n
        stats["rounds"] += 1
        stats["accepted"].append(n)
    keep = np.array([not r for r in removed])
    new = np.cumsum(keep) - 1
    out = np.array([[new[i] for i in tri] for tri in faces if tri is not None], dtype=np.int64).reshape(-1, 3)
    stats.update(faces_after=int(out.shape[0]), reached=out.shape[0] <= target)
    return np.nonzero(keep)[0], out, stats


# ---- measures -------------------------------------------------------------------------------------------------------------------------------
def manifold_report(faces, num_verts):
    """What the tests ask of a closed result: {"edges_twice_opposite", "euler", "duplicates", "degenerate", "used_vertices"}"""
    f = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    und, cnt, direction = R.undirected_counts(f)
    used = np.unique(f)
    key = np.sort(f, axis=1)
    return {"edges_twice_opposite": bool((cnt == 2).all() and (direction == 0).all()), "euler": int(used.shape[0] - und.shape[0] + f.shape[0]),
            "duplicates": int(f.shape[0] - np.unique(key, axis=0).shape[0]),
            "degenerate": int(((f[:, 0] == f[:, 1]) | (f[:, 1] == f[:, 2]) | (f[:, 0] == f[:, 2])).sum()), "used_vertices": int(used.shape[0])}


def sphere_measures(verts, faces, before_verts, before_faces, radius=0.5):
    """{"radial": the largest | |p| - radius | over the vertices, the edge midpoints and the face centroids, "volume_ratio": against the mesh
    before}: how far the result leaves the sphere both meshes approximate"""
    p = np.asarray(verts, dtype=np.float64)
    f = np.asarray(faces, dtype=np.int64)
    tri = p[f]
    pts = np.concatenate([p[np.unique(f)], tri.mean(1), 0.5 * (tri[:, 0] + tri[:, 1]), 0.5 * (tri[:, 1] + tri[:, 2]), 0.5 * (tri[:, 2] + tri[:, 0])])
    return {"radial": float(np.abs(np.linalg.norm(pts, axis=1) - radius).max()),
            "volume_ratio": R.signed_volume(p, f) / R.signed_volume(np.asarray(before_verts, dtype=np.float64), np.asarray(before_faces))}


# ---- scenes ---------------------------------------------------------------------------------------------------------------------------------
LOOP_CASES = {"net": 400, "ico3": 200}          # name -> target faces of the end-to-end runs


@functools.lru_cache(maxsize=None)
def scene(name):
    """(verts float32 [V, 3], faces int64 [F, 3], colors float32 [V, 3]) torch tensors, built once (nothing writes into them)"""
    if name == "net":
        return C.sphere_mesh()
    if name == "noisy":
        return C.noisy_sphere(0)
    if name in ("ico2", "ico3"):
        v, f = M.icosphere(int(name[3]), 0.5, (0.0, 0.0, 0.0), seed=2)
        return v, f, M.position_colors(v)
    if name == "unreferenced":
        return C.insert_unreferenced(*scene("ico2"))[:3]
    v, f = {"tetrahedron": tetrahedron, "octahedron": octahedron, "grid": wavy_grid, "flat": flat_grid, "bipyramid": bipyramid, "dart": dart}[name]()
    return v, f, M.position_colors(v)


def tetrahedron():
    v = torch.tensor([[0.0, 0.0, 0.5], [0.45, 0.0, -0.2], [-0.25, 0.4, -0.2], [-0.25, -0.4, -0.25]])
    return v, torch.tensor([[0, 1, 2], [0, 2, 3], [0, 3, 1], [1, 3, 2]])


def octahedron():
    v = torch.tensor([[0.5, 0.0, 0.0], [-0.45, 0.0, 0.0], [0.0, 0.4, 0.0], [0.0, -0.5, 0.0], [0.0, 0.0, 0.55], [0.0, 0.0, -0.35]])
    return v, torch.tensor([[0, 2, 4], [2, 1, 4], [1, 3, 4], [3, 0, 4], [2, 0, 5], [1, 2, 5], [3, 1, 5], [0, 3, 5]])


def _grid(nx, ny, height):
    x, y = torch.meshgrid(torch.arange(nx, dtype=torch.float32), torch.arange(ny, dtype=torch.float32), indexing="xy")
    x, y = x.reshape(-1), y.reshape(-1)
    dx, dy = (7 * x + 3 * y) % 5 - 2, (3 * x + 5 * y) % 7 - 3          # no three neighbours in a line: no collapse leaves a face without area
    v = torch.stack([(16 * x + 2 * dx) / 256.0 - 0.5, (16 * y + dy) / 256.0 - 0.5, torch.zeros(nx * ny)], 1)
    v[:, 2] = height(v)
    faces = []
    for j in range(ny - 1):
        for i in range(nx - 1):
            a, b, c, d = j * nx + i, j * nx + i + 1, (j + 1) * nx + i + 1, (j + 1) * nx + i
            faces += [(a, b, c), (a, c, d)] if (i + j) % 2 == 0 else [(a, b, d), (b, c, d)]
    return v, torch.tensor(faces)


GRID = (19, 17)                                  # more than one block of vertices: 323


def wavy_grid():
    """An open quad grid (cells of 1/16, every vertex moved by a few 1/256 in x and y) with alternating diagonals over a smooth height field"""
    return _grid(*GRID, lambda v: 0.05 * torch.sin(7 * v[:, 0]) * torch.cos(5 * v[:, 1]))


def flat_grid():
    """The same grid in the plane z = 0.25 (x and y on multiples of 1/256): every quadric form is exactly 0 at every vertex"""
    return _grid(*GRID, lambda v: torch.full((v.shape[0],), 0.25))


def grid_rim(nx=GRID[0], ny=GRID[1]):
    i = torch.arange(nx * ny)
    return (i % nx == 0) | (i % nx == nx - 1) | (i // nx == 0) | (i // nx == ny - 1)


FAN = 700


def bipyramid(n=FAN // 2):
    """Two closed fans of n faces each over one wavy rim of n vertices (vertex 0 the upper apex, 1 the lower): FAN faces, closed, the
    apexes far above any valence cap, the rim vertices of valence 4"""
    t = torch.arange(n, dtype=torch.float64) * (2 * np.pi / n)
    ring = torch.stack([0.5 * torch.cos(t), 0.5 * torch.sin(t), 0.03 * torch.sin(5 * t)], 1)
    v = torch.cat([torch.tensor([[0.0, 0.0, 0.4], [0.0, 0.0, -0.3]], dtype=torch.float64), ring]).float()
    i = torch.arange(n)
    a, b = 2 + i, 2 + (i + 1) % n
    return v, torch.cat([torch.stack([torch.zeros(n, dtype=torch.long), a, b], 1), torch.stack([torch.ones(n, dtype=torch.long), b, a], 1)])


DART = dict(centre=0, top=1, left=2, notch=3, right=4)


def dart():
    """A dart (a concave quadrilateral) fanned around an interior vertex: moving the centre onto the left or the right tip folds the face
    between the notch and the other tip over (n_before . n_after = 0.3 x -1.4 = -0.42 in the plane, far from 0); onto the top or the notch
    nothing flips.  The centre is the one removable vertex: the other four lie on the open edge."""
    v = torch.tensor([[0.0, 0.0, 0.125], [0.0, 1.0, 0.0], [-1.0, -1.0, 0.0], [0.0, -0.3, 0.0], [1.0, -1.0, 0.0]])
    return v, torch.tensor([[0, 1, 2], [0, 2, 3], [0, 3, 4], [0, 4, 1]])
