"""Restatement of the mesh check (include/v3d_recon.h "Mesh check", csrc_recon/meshcheck.hip, v3d_amd/recon/mesh_check.py) in torch and plain
python, and the scenes of tests/test_mesh_check_cpu.py and tests/test_mesh_check_gpu.py.

THE PAIR RULE is restated as a brute force over all pairs of faces, statement by statement, in float64 (the oracle) and in float32 (every
product rounded on its own, as the kernel rounds it).  A second formulation (Moeller-Trumbore with the edge as a ray, det == 0 a miss) only
cross-checks the oracle where its determinant is not small.  THE CENSUS is restated with dicts over directed edges.

Every pair of faces that reaches rule (d) reports a MARGIN, per edge test that the rule runs: the smaller |signed distance| of the edge's two
endpoints from the triangle's plane over the diagonal of the mesh's bounding box, and, for an edge whose endpoints lie strictly on opposite
sides, the smallest |barycentric| of the crossing point.  A scene whose smallest margin is far above the float32 error of these figures
(about 1e-7) is decided alike in float32 and float64: tests/test_mesh_check_cpu.py holds every scene to SCENE_MARGIN."""
import collections
import functools
import math

import numpy as np
import torch

import mesh_render_ref as M

F64, F32 = torch.float64, torch.float32
SCENE_MARGIN = 5e-5
DET_FLOOR = 1e-6                   # the cross-check speaks only where |det| / (|e1| |e2| |d|) is at least this
SEEDS = (1, 2, 3)
# the prototype's census of the scenes for seeds 1, 2, 3: pairs, and pairs that share a vertex
PINNED = {"sphere": ((0, 0, 0), (0, 0, 0)), "pair": ((76, 77, 77), (0, 0, 0)), "fold": ((69, 68, 71), (2, 2, 2))}
OPEN, NON_MANIFOLD, WINDING, PINCHED = 1, 2, 4, 8


# ---- THE PAIR RULE --------------------------------------------------------------------------------------------------------------------------
def _dot(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def _cross(u, w):
    return torch.stack([u[..., 1] * w[..., 2] - u[..., 2] * w[..., 1], u[..., 2] * w[..., 0] - u[..., 0] * w[..., 2],
                        u[..., 0] * w[..., 1] - u[..., 1] * w[..., 0]], -1)


def _no_area(e1, e2):
    return ((e1[..., 1] * e2[..., 2] == e1[..., 2] * e2[..., 1]) & (e1[..., 2] * e2[..., 0] == e1[..., 0] * e2[..., 2])
            & (e1[..., 0] * e2[..., 1] == e1[..., 1] * e2[..., 0]))


def edge_test(p, q, a, b, c):
    """(d) on rows: (holds, dp, dq, |n|, crosses the plane, ta, tb, tc, d . n)"""
    n = _cross(b - a, c - a)
    dp, dq = _dot(n, p - a), _dot(n, q - a)
    opposite = ((dp > 0) & (dq < 0)) | ((dp < 0) & (dq > 0))
    d = q - p
    ta, tb, tc = _dot(d, _cross(b - p, c - p)), _dot(d, _cross(c - p, a - p)), _dot(d, _cross(a - p, b - p))
    inside = torch.where(dp > 0, (ta <= 0) & (tb <= 0) & (tc <= 0), (ta >= 0) & (tb >= 0) & (tc >= 0))
    return opposite & inside, dp, dq, _dot(n, n).sqrt(), opposite, ta, tb, tc, _dot(d, n)


def moller_trumbore(p, q, a, b, c):
    """The second formulation: the edge as the ray p + t (q - p), 0 < t < 1.  (hit, |det| / (|e1| |e2| |d|))"""
    d, e1, e2 = q - p, b - a, c - a
    pv = torch.linalg.cross(d, e2)
    det = (e1 * pv).sum(-1)
    ok = det != 0
    inv = torch.where(ok, 1.0 / torch.where(ok, det, torch.ones_like(det)), torch.zeros_like(det))
    s = p - a
    u = (s * pv).sum(-1) * inv
    qv = torch.linalg.cross(s, e1)
    v = (d * qv).sum(-1) * inv
    t = (e2 * qv).sum(-1) * inv
    rel = det.abs() / (e1.norm(dim=-1) * e2.norm(dim=-1) * d.norm(dim=-1)).clamp_min(1e-300)
    return ok & (u >= 0) & (v >= 0) & (u + v <= 1) & (t > 0) & (t < 1), rel


def candidates(verts, faces, dtype=F64):
    """(a), (b), (c) over all pairs f < g: (f [n], g [n], s [n], ka [n], kb [n]) of the pairs that reach (d); ka, kb: the shared vertex's
    corner where s == 1.  Also the number of faces that pass (a)."""
    v = verts.to(dtype)
    f = faces.long()
    V, F = v.shape[0], f.shape[0]
    present = ((f >= 0) & (f < V)).all(1)
    fc = f.clamp(0, max(V - 1, 0))
    a, b, c = v[fc[:, 0]], v[fc[:, 1]], v[fc[:, 2]]
    ok = present & ~_no_area(b - a, c - a)
    lo, hi = torch.minimum(a, torch.minimum(b, c)), torch.maximum(a, torch.maximum(b, c))
    meet = ((lo[:, None] <= hi[None]) & (lo[None] <= hi[:, None])).all(-1) & ok[:, None] & ok[None]
    meet &= torch.ones(F, F, dtype=torch.bool).triu(1)
    fi, gi = torch.nonzero(meet, as_tuple=True)
    eq = f[fi][:, :, None] == f[gi][:, None, :]                 # [n, corner of A, corner of B]
    s = eq.sum((1, 2))
    keep = s < 2
    fi, gi, s, eq = fi[keep], gi[keep], s[keep], eq[keep]
    return fi, gi, s, eq.any(2).int().argmax(1), eq.any(1).int().argmax(1), int(ok.sum())


def pair_rule(verts, faces, dtype=F64, cross_check=False):
    """The brute force.  {"pairs": sorted [(f, g)], f < g; "shared": how many of them share a vertex; "reached": pairs that reached (d);
    "margin": the smallest over every test run (inf when none); "plane", "bary": the plane distances (over |n|) and barycentrics of every test
    run, for the float32 run's error against float64; with cross_check "disagree": tests whose two formulations differ at a relative
    |det| >= DET_FLOOR, and "min_det": the smallest relative |det| seen}"""
    v = verts.to(dtype)
    f = faces.long()
    fi, gi, s, ka, kb, _ = candidates(verts, faces, dtype)
    n = fi.shape[0]
    diag = float((verts.double().max(0).values - verts.double().min(0).values).norm())
    A = [v[f[fi][:, k]] for k in range(3)] if n else [v[:0]] * 3
    B = [v[f[gi][:, k]] for k in range(3)] if n else [v[:0]] * 3
    rows = torch.arange(n)

    def corner(T, k):                                           # corner k [n] of the triangles T
        return torch.stack(T, 1)[rows, k % 3]

    # the tests in the rule's order: (runs [n], p, q, a, b, c)
    tests = []
    one, none = s == 1, s == 0
    tests.append((one, corner(A, ka + 1), corner(A, ka + 2), *B))
    tests.append((one, corner(B, kb + 1), corner(B, kb + 2), *A))
    for k in range(3):
        tests.append((none, A[k], A[(k + 1) % 3], *B))
    for k in range(3):
        tests.append((none, B[k], B[(k + 1) % 3], *A))
    hit = torch.zeros(n, dtype=torch.bool)
    margin, plane, bary, disagree, min_det = math.inf, [], [], 0, math.inf
    for runs, p, q, a, b, c in tests:
        if not bool(runs.any()):
            continue
        p, q, a, b, c = (x[runs] for x in (p, q, a, b, c))
        holds, dp, dq, nlen, opp, ta, tb, tc, dn = edge_test(p, q, a, b, c)
        hit[runs] |= holds
        sd = torch.stack([dp, dq], 1) / nlen[:, None]
        bc = torch.stack([ta, tb, tc], 1) / torch.where(opp, dn, torch.ones_like(dn))[:, None]
        plane.append(sd)
        bary.append(torch.where(opp[:, None], bc, torch.zeros_like(bc)))
        margin = min(margin, float(sd.abs().min()) / diag)
        if bool(opp.any()):
            margin = min(margin, float(bc[opp].abs().min()))
        if cross_check:
            mt, rel = moller_trumbore(p, q, a, b, c)
            said = rel >= DET_FLOOR
            disagree += int((mt[said] != holds[said]).sum())
            min_det = min(min_det, float(rel.min()))
    pairs = sorted(zip(fi[hit].tolist(), gi[hit].tolist()))
    out = {"pairs": pairs, "shared": int((s[hit] == 1).sum()), "reached": n, "margin": margin,
           "plane": torch.cat(plane) if plane else torch.zeros(0, 2, dtype=dtype), "bary": torch.cat(bary) if bary else torch.zeros(0, 3, dtype=dtype)}
    if cross_check:
        out.update(disagree=disagree, min_det=min_det)
    return out


def degrees(pairs, F):
    d = [0] * F
    for f, g in pairs:
        d[f] += 1
        d[g] += 1
    return d


# ---- THE CENSUS -----------------------------------------------------------------------------------------------------------------------------
def _face_rows(faces):
    return [tuple(int(x) for x in row) for row in np.asarray(faces).reshape(-1, 3)]


def census(faces, V):
    """(same [3F], opposite [3F], flags [V]) as lists, with dicts over directed edges"""
    rows = _face_rows(faces)
    present = [all(0 <= i < V for i in r) for r in rows]
    counted = [ok and len(set(r)) == 3 for ok, r in zip(present, rows)]
    directed = collections.Counter()
    for r, ok in zip(rows, counted):
        if ok:
            for k in range(3):
                directed[(r[k], r[(k + 1) % 3])] += 1
    same, opposite = [], []
    for r, ok in zip(rows, counted):
        for k in range(3):
            u, w = r[k], r[(k + 1) % 3]
            same.append(directed[(u, w)] if ok else -1)
            opposite.append(directed[(w, u)] if ok else -1)
    flags = [0] * V
    for (u, w), out in list(directed.items()):
        back = directed.get((w, u), 0)
        bits = (OPEN if out + back == 1 else 0) | (NON_MANIFOLD if out + back >= 3 else 0)
        bits |= WINDING if (out == 2 and back == 0) or (back == 2 and out == 0) else 0
        flags[u] |= bits
        flags[w] |= bits
    star = collections.defaultdict(list)                        # v -> [(next, previous)] over the present faces
    for r, ok in zip(rows, present):
        if ok:
            for k in range(3):
                star[r[k]].append((r[(k + 1) % 3], r[(k + 2) % 3]))
    for v, entries in star.items():
        if flags[v] == 0 and not one_closed_fan(v, entries):
            flags[v] = PINCHED
    return same, opposite, flags


def one_closed_fan(v, entries):
    """next -> previous over v's entries is one cycle through every neighbour"""
    if any(a == v or b == v or a == b for a, b in entries):
        return False
    step = dict(entries)
    if len(step) != len(entries) or sorted(step) != sorted(b for _, b in entries):
        return False
    x, n = entries[0][1], 1
    while x != entries[0][0] and n <= len(entries):
        x, n = step[x], n + 1
    return n == len(entries)


def components(faces, V):
    """the connected components that have a face (two vertices are joined when a present face uses both)"""
    parent = list(range(V))

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x

    roots = []
    for r in _face_rows(faces):
        if all(0 <= i < V for i in r):
            for i in r[1:]:
                parent[find(i)] = find(r[0])
            roots.append(r[0])
    return len({find(x) for x in roots})


def report(verts, faces):
    """check_mesh restated: every key but "seconds" """
    v32 = verts.float()
    v = v32.double()
    rows = _face_rows(faces)
    V, F = v.shape[0], len(rows)
    same, opposite, flags = census(faces, V)
    present = [r for r in rows if all(0 <= i < V for i in r)]
    counted = [r for r in present if len(set(r)) == 3]
    edges = collections.Counter()
    for r in counted:
        for k in range(3):
            edges[frozenset((r[k], r[(k + 1) % 3]))] += 1
    by_mult = collections.Counter(edges.values())
    directed = collections.Counter((r[k], r[(k + 1) % 3]) for r in counted for k in range(3))
    inconsistent = sum(1 for e, m in edges.items() if m == 2 and 2 in (directed[tuple(e)], directed[tuple(e)[::-1]]))
    E, Fc, Vu = len(edges), len(counted), len({i for r in counted for i in r})
    boundary, non_manifold = by_mult.get(1, 0), sum(n for m, n in by_mult.items() if m >= 3)
    pinched = sum(1 for b in flags if b & PINCHED)
    closed, manifold, oriented = Fc > 0 and boundary == 0, non_manifold == 0 and pinched == 0, inconsistent == 0
    comp = components(faces, V)
    euler = Vu - E + Fc
    fp = torch.tensor(present, dtype=torch.long).reshape(-1, 3)
    a, b, c = v[fp[:, 0]], v[fp[:, 1]], v[fp[:, 2]]
    e1, e2 = v32[fp[:, 1]] - v32[fp[:, 0]], v32[fp[:, 2]] - v32[fp[:, 0]]
    sound = closed and manifold and oriented
    hits = pair_rule(verts, faces)
    return {"vertices": V, "vertices_used": Vu, "faces": F, "absent_faces": F - len(present), "repeated_index_faces": len(present) - Fc,
            "zero_area_faces": int(_no_area(e1, e2).sum()), "edges": E, "edges_by_multiplicity": {str(m): n for m, n in sorted(by_mult.items())},
            "boundary_edges": boundary, "non_manifold_edges": non_manifold, "inconsistent_edges": inconsistent, "pinched_vertices": pinched,
            "components": comp, "euler": euler, "closed": closed, "manifold": manifold, "oriented": oriented,
            "genus": (2 * comp - euler) // 2 if sound and (2 * comp - euler) % 2 == 0 else None,
            "area": 0.5 * float(torch.linalg.cross(b - a, c - a).norm(dim=1).sum()),
            "volume": float((a * torch.linalg.cross(b, c)).sum()) / 6.0 if closed and oriented else None,
            "self_intersections": len(hits["pairs"]), "intersecting_faces": sum(1 for d in degrees(hits["pairs"], F) if d),
            "watertight": sound and not hits["pairs"]}


def same_report(got, want, rel=1e-12):
    """every key of `want` in `got`: integers, booleans and None exactly, area and volume within `rel`"""
    for k, x in want.items():
        y = got[k]
        if isinstance(x, float):
            assert isinstance(y, float) and abs(y - x) <= rel * abs(x), (k, y, x)
        else:
            assert y == x and type(y) is type(x), (k, y, x)
    return True


# ---- the scenes -----------------------------------------------------------------------------------------------------------------------------
FOLD_CENTRE = (0.02, -0.01, 0.03)
FOLD_MOVES = ((0, (0.031, -0.017, 0.023)), (7, (-0.027, 0.013, 0.019)), (19, (0.011, 0.029, -0.021)))


def fold(seed):
    """The 320-face icosphere with three vertices pushed through to the far side, each a little off the antipode (at the exact antipode the
    margin falls to 1e-8)"""
    v, f = M.icosphere(2, 0.5, FOLD_CENTRE, seed)
    c = torch.tensor(FOLD_CENTRE, dtype=F64)
    v = v.double()
    for i, off in FOLD_MOVES:
        v[i] = c - 1.3 * (v[i] - c) + torch.tensor(off, dtype=F64)
    return v.float(), f


def pair3(seed=1):
    """The two spheres of "pair" at subdivision 3 without the last 7 faces: F = 2553, not a multiple of 64, open, a deeper tree.  The second
    sphere stands 0.041 higher than in "pair": at 0.1 the smallest margin of the 12 000 pairs that reach (d) was 1.6e-5, here it is 6.7e-5."""
    v1, f1 = M.icosphere(3, 0.4, (-0.12, 0.1, 0.0), seed)
    v2, f2 = M.icosphere(3, 0.33, (0.2, -0.12, 0.141), seed + 1)
    return torch.cat([v1, v2]), torch.cat([f1, f2 + v1.shape[0]])[:-7]


CASES_VERTS = (
    (0.0, 0.0, 0.0), (2.0, 0.0, 0.0), (0.0, 2.0, 0.0), (0.5, 0.5, -1.0), (0.7, 0.6, 1.0),           # 0-4: one shared vertex, B's far edge pierces A
    (4.0, 0.0, 0.0), (6.0, 0.0, 0.0), (4.0, 2.0, 0.0), (4.5, 0.5, 0.3), (4.7, 0.6, 1.0),            # 5-9: the same, B stays above A
    (8.0, 0.0, 0.0), (10.0, 0.0, 0.0), (9.0, 2.0, 0.0), (9.0, 1.9, 0.05),                           # 10-13: a common edge, folded sharply
    (0.0, 4.0, 0.0), (2.0, 4.0, 0.0), (0.0, 6.0, 0.0),                                              # 14-16: the duplicated face
    (4.0, 4.0, 0.0), (4.25, 4.25, 0.25), (4.5, 4.5, 0.5),                                           # 17-19: three points on a line
    (8.0, 8.0, 8.0), (9.0, 8.0, 8.0), (8.0, 9.0, 8.0),                                              # 20-22: the far triangle
    (0.0, 8.0, 0.0), (2.0, 8.0, 0.0), (0.0, 10.0, 0.0), (0.5, 8.5, -1.0), (0.7, 8.6, 1.0), (0.4, 8.9, 1.0),      # 23-28: no shared vertex, crossing
)
CASES_FACES = (
    (0, 1, 2), (0, 3, 4),                  # 0, 1: a pair
    (5, 6, 7), (5, 8, 9),                  # 2, 3: not a pair
    (10, 11, 12), (11, 10, 13),            # 4, 5: a common edge: never reported
    (14, 15, 16), (14, 15, 16),            # 6, 7: the same three vertices: never reported
    (20, 21, 29),                          # 8: an index outside the vertices
    (17, 17, 19),                          # 9: a repeated index
    (17, 18, 19),                          # 10: no area, three indices
    (20, 21, 22),                          # 11: alone
    (23, 24, 25), (26, 27, 28),            # 12, 13: a pair
)
CASES_PAIRS = [(0, 1), (12, 13)]


def cases():
    return torch.tensor(CASES_VERTS, dtype=F32), torch.tensor(CASES_FACES, dtype=torch.long)


def single(F):
    """F = 1: one triangle;  F = 2: two that cross"""
    v, f = cases()
    return (v[20:23].clone(), torch.tensor([[0, 1, 2]])) if F == 1 else (v[23:29].clone(), torch.tensor([[0, 1, 2], [3, 4, 5]]))


@functools.lru_cache(maxsize=None)
def scene(name):
    """(verts float32, faces int64) of "sphere-1", "pair-2", "fold-3", "pair3", "cases", "single-1", "single-2" """
    kind, _, arg = name.partition("-")
    if kind in ("sphere", "pair"):
        return M.mesh_scene(kind, int(arg))[:2]
    if kind == "fold":
        return fold(int(arg))
    if kind == "single":
        return single(int(arg))
    return {"pair3": pair3, "cases": cases}[kind]()


PAIR_SCENES = tuple(f"{k}-{s}" for k in ("sphere", "pair", "fold") for s in SEEDS) + ("cases", "pair3", "single-1", "single-2")


@functools.lru_cache(maxsize=None)
def oracle(name):
    """the float64 rule on a scene, with the cross-check; computed once"""
    return pair_rule(*scene(name), dtype=F64, cross_check=True)


@functools.lru_cache(maxsize=None)
def oracle32(name):
    return pair_rule(*scene(name), dtype=F32)


# ---- the census meshes ----------------------------------------------------------------------------------------------------------------------
TORUS = (6, 5)
GRID = (5, 3)


def torus(n=TORUS[0], m=TORUS[1], R=1.0, r=0.4):
    """n x m quads around both circles, two faces each: V = n m, E = 3 n m, F = 2 n m, genus 1"""
    v, f = [], []
    for i in range(n):
        for j in range(m):
            a, b = 2 * math.pi * i / n, 2 * math.pi * j / m
            v.append(((R + r * math.cos(b)) * math.cos(a), (R + r * math.cos(b)) * math.sin(a), r * math.sin(b)))
            p00, p10, p01, p11 = i * m + j, ((i + 1) % n) * m + j, i * m + (j + 1) % m, ((i + 1) % n) * m + (j + 1) % m
            f += [(p00, p10, p11), (p00, p11, p01)]
    return torch.tensor(v, dtype=F32), torch.tensor(f, dtype=torch.long)


def open_grid(nx=GRID[0], ny=GRID[1]):
    """nx x ny cells, two faces each: 2 (nx + ny) open edges"""
    v = [(float(x), float(y), 0.1 * math.sin(x + 2 * y)) for y in range(ny + 1) for x in range(nx + 1)]
    f = []
    for y in range(ny):
        for x in range(nx):
            p = y * (nx + 1) + x
            f += [(p, p + 1, p + nx + 2), (p, p + nx + 2, p + nx + 1)]
    return torch.tensor(v, dtype=F32), torch.tensor(f, dtype=torch.long)


def fin():
    """three faces on the edge 0 1, two of them running the same way"""
    v = [(0.0, 0.0, 0.0), (1.0, 0.0, 0.0), (0.5, 1.0, 0.0), (0.5, -1.0, 0.2), (0.5, 0.1, 1.0)]
    return torch.tensor(v, dtype=F32), torch.tensor([(0, 1, 2), (1, 0, 3), (0, 1, 4)], dtype=torch.long)


def _tetrahedron(apex, base, offset):
    x, y, z = apex
    v = [apex, (x + base, y + 0.1, z + offset), (x - 0.3 * base, y + base, z + offset), (x - 0.4 * base, y - base, z + offset)]
    f = [(0, 1, 2), (0, 2, 3), (0, 3, 1), (1, 3, 2)] if offset < 0 else [(0, 2, 1), (0, 3, 2), (0, 1, 3), (1, 2, 3)]
    return v, f


def bow_tie():
    """two tetrahedra that share vertex 0 and nothing else: closed, every edge has two faces, one pinched vertex"""
    v1, f1 = _tetrahedron((0.0, 0.0, 0.0), 0.5, 1.0)
    v2, f2 = _tetrahedron((0.0, 0.0, 0.0), 0.5, -1.0)
    remap = {0: 0, 1: 4, 2: 5, 3: 6}
    return torch.tensor(v1 + v2[1:], dtype=F32), torch.tensor(f1 + [tuple(remap[i] for i in t) for t in f2], dtype=torch.long)


def flipped(face=37):
    v, f = M.icosphere(2, 0.5, (0.0, 0.0, 0.0), 1)
    f = f.clone()
    f[face] = f[face][[0, 2, 1]]
    return v, f


@functools.lru_cache(maxsize=None)
def census_mesh(name):
    if name == "icosphere":
        return M.icosphere(2, 0.5, (0.03, -0.02, 0.04), 1)
    if name == "two":
        return M.mesh_scene("pair", 1)[:2]
    return {"torus": torus, "open_grid": open_grid, "fin": fin, "bow_tie": bow_tie, "flipped": flipped, "cases": cases}[name]()


CENSUS_MESHES = ("icosphere", "torus", "open_grid", "fin", "bow_tie", "flipped", "two", "cases")
# what is known of each without running anything
CENSUS_FACTS = {
    "icosphere": {"vertices_used": 162, "edges": 480, "faces": 320, "euler": 2, "genus": 0, "boundary_edges": 0, "non_manifold_edges": 0,
                  "inconsistent_edges": 0, "pinched_vertices": 0, "components": 1, "closed": True, "manifold": True, "oriented": True,
                  "edges_by_multiplicity": {"2": 480}},
    "torus": {"vertices_used": TORUS[0] * TORUS[1], "edges": 3 * TORUS[0] * TORUS[1], "faces": 2 * TORUS[0] * TORUS[1], "euler": 0, "genus": 1,
              "closed": True, "manifold": True, "oriented": True, "components": 1},
    "open_grid": {"boundary_edges": 2 * (GRID[0] + GRID[1]), "edges": GRID[0] * (GRID[1] + 1) + GRID[1] * (GRID[0] + 1) + GRID[0] * GRID[1],
                  "closed": False, "manifold": True, "oriented": True, "genus": None, "euler": 1, "volume": None},
    "fin": {"non_manifold_edges": 1, "boundary_edges": 6, "edges_by_multiplicity": {"1": 6, "3": 1}, "manifold": False, "closed": False, "genus": None},
    "bow_tie": {"pinched_vertices": 1, "boundary_edges": 0, "non_manifold_edges": 0, "closed": True, "manifold": False, "oriented": True,
                "components": 1, "genus": None, "euler": 3},
    "flipped": {"inconsistent_edges": 3, "oriented": False, "closed": True, "manifold": True, "genus": None, "volume": None, "euler": 2},
    "two": {"components": 2, "euler": 4, "genus": 0, "closed": True, "manifold": True, "oriented": True, "watertight": False, "self_intersections": 76},
    "cases": {"absent_faces": 1, "repeated_index_faces": 1, "zero_area_faces": 2, "faces": len(CASES_FACES), "self_intersections": 2,
              "intersecting_faces": 4, "watertight": False},
}
