"""Restatement of csrc_recon/meshremesh.hip (test oracle) and the scenes of tests/test_mesh_remesh_{cpu,gpu}.py, written from the statements
of include/v3d_recon.h "Mesh remeshing".  Plain Python over scalars: fp64 by default; `dtype=np.float32` runs every length, the relaxation
and the reprojection in single precision, statement for statement as the kernels do (the normal tests are fp64 in both, as in the kernels:
the float32 run IS the kernel's arithmetic).  The rounds are the kernels' rounds: every vertex proposes on the state of the round's start,
mesh_decimate_ref.select accepts, the accepted operations are applied.  A mesh in flight is a State: rows up to a capacity, None for a dead
or unborn face."""
from __future__ import annotations

import functools
import math

import numpy as np
import torch

import mesh_clean_ref as C
import mesh_decimate_ref as Dm
import mesh_query_ref as Q

NO_KEY = Dm.NO_KEY
KEY_HASH = 0x9E3779B1
DEFAULT_MAX_VALENCE = 24
NEAR = 1e-6                         # a decision whose fp64 value lies within this, relative, of its threshold is left out of a comparison
EXCLUDE_MAX = 0.02                  # at most this share of a case's decisions may be left out
NORMAL_EPS = 1e-20
INF = float("inf")


# ---- numbers --------------------------------------------------------------------------------------------------------------------------------
def _scalar(dtype):
    return float if np.dtype(dtype) == np.float64 else np.float32


def _sqrt(x):
    return math.sqrt(x) if isinstance(x, float) else np.sqrt(x)


def bits(x) -> int:
    return int(np.asarray(np.float32(x), dtype=np.float32).view(np.uint32))


def make_key(priority, v: int) -> int:
    return (bits(priority) << 32) | ((v * KEY_HASH) & 0xFFFFFFFF)


def thresholds(L, T):
    """(L^2, lo^2, hi^2) as the entries compute them from the float32 target_edge"""
    e = T(np.float32(L))
    L2 = e * e
    return L2, (T(16.0) / T(25.0)) * L2, (T(16.0) / T(9.0)) * L2


def dist2(P, i, j):
    dx, dy, dz = P[i][0] - P[j][0], P[i][1] - P[j][1], P[i][2] - P[j][2]
    return (dx * dx + dy * dy) + dz * dz


def _f64(p):
    return (float(p[0]), float(p[1]), float(p[2]))


def _dot(a, b):
    return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]


def _rel(x, t):
    """how far x lies from the threshold t, relative to t"""
    x, t = float(x), float(t)
    return abs(x - t) / t if t > 0 else INF


def _sign_margin(d, n1, n2):
    """how far the product n1 . n2 = d lies from 0, relative to |n1| |n2|"""
    s = math.sqrt(_dot(n1, n1)) * math.sqrt(_dot(n2, n2))
    return abs(d) / s if s > 0 else INF


# ---- the state ------------------------------------------------------------------------------------------------------------------------------
class State:
    def __init__(self, verts, faces, colors, spare_verts=None, dtype=np.float64):
        T = self.T = _scalar(dtype)
        v = np.asarray(verts, dtype=np.float32)
        c = np.asarray(colors, dtype=np.float32) if colors is not None else np.zeros_like(v)
        f = Dm.face_list(faces)
        spare = len(f) // 2 + 64 if spare_verts is None else spare_verts
        self.V_live, self.F_live = v.shape[0], len(f)
        self.Vcap, self.Fcap = self.V_live + spare, self.F_live + 2 * spare
        zero = (T(0.0),) * 3
        self.P = [tuple(T(x) for x in row) for row in v.tolist()] + [zero] * spare
        self.C = [tuple(T(x) for x in row) for row in c.tolist()] + [zero] * spare
        self.faces = [tri if all(0 <= i < self.Vcap for i in tri) else None for tri in f] + [None] * (2 * spare)          # (the entries' rule)
        self.removed = [False] * self.Vcap
        self.flag = False

    def stars(self):
        return Dm.stars(self.faces, self.Vcap)

    def grow(self, spare):
        zero = (self.T(0.0),) * 3
        self.P += [zero] * spare
        self.C += [zero] * spare
        self.removed += [False] * spare
        self.faces += [None] * (2 * spare)
        self.Vcap += spare
        self.Fcap += 2 * spare

    def result(self):
        """(verts [Vo, 3] float64 array, faces [Fo, 3] int64, colors [Vo, 3]): the live faces and the born vertices no collapse removed"""
        keep = np.array([i < self.V_live and not self.removed[i] for i in range(self.Vcap)])
        new = np.cumsum(keep) - 1
        f = np.array([[new[i] for i in tri] for tri in self.faces if tri is not None], dtype=np.int64).reshape(-1, 3)
        return (np.array([self.P[i] for i in np.nonzero(keep)[0]], dtype=np.float64).reshape(-1, 3), f,
                np.array([self.C[i] for i in np.nonzero(keep)[0]], dtype=np.float64).reshape(-1, 3))


def editable(s, a, b):
    """(fc, kc, c, fd, kd, d) of THE EDGE (a, b) IS EDITABLE from a's star s, or None"""
    ab = [(f, k, y) for f, k, x, y in s if x == b]
    ba = [(f, k, x) for f, k, x, y in s if y == b]
    if len(ab) != 1 or len(ba) != 1:
        return None
    (fc, kc, c), (fd, kd, d) = ab[0], ba[0]
    if len({a, b, c, d}) != 4:
        return None
    return fc, kc, c, fd, kd, d


def boundary_flags(star):
    out = []
    for v, s in enumerate(star):
        nb = {x for _, _, a, b in s for x in (a, b) if x != v}
        out.append(int(any(sum(1 for _, _, a, b in s if a == u or b == u) == 1 for u in nb)))
    return out


# ---- split ----------------------------------------------------------------------------------------------------------------------------------
def split_propose(st, L, cap=DEFAULT_MAX_VALENCE, star=None):
    """(keys, targets, margin): margin[v] = how near v's nearest length decision came to hi^2, relative"""
    L2, _, hi2 = thresholds(L, st.T)
    star = st.stars() if star is None else star
    keys, targets, margin = [], [], []
    for a, s in enumerate(star):
        best, near = None, INF
        if 1 <= len(s) <= cap:
            for _, _, b, _ in s:
                if b == a:
                    continue
                len2 = dist2(st.P, a, b)
                if editable(s, a, b) is not None:
                    near = min(near, _rel(len2, hi2))
                if not len2 > hi2 or editable(s, a, b) is None:
                    continue
                if best is None or len2 > best[0] or (len2 == best[0] and b < best[1]):
                    best = (len2, b)
        keys.append(NO_KEY if best is None else make_key(L2 / best[0], a))
        targets.append(-1 if best is None else best[1])
        margin.append(near)
    return keys, targets, margin


def split_apply(st, accept, targets, star=None):
    """Applies the accepted splits by rank; {a: (faces written, vertices touched)}.  st.flag is set when some were dropped."""
    star = st.stars() if star is None else star
    total = sum(1 for a in accept if a)
    done = max(0, min(total, st.Vcap - st.V_live, (st.Fcap - st.F_live) // 2))
    if total > done:
        st.flag = True
    touched, r = {}, 0
    T = st.T
    for a, on in enumerate(accept):
        if not on:
            continue
        rank, r = r, r + 1
        b = targets[a]
        if rank >= done or not 0 <= b < st.Vcap:
            continue
        e = editable(star[a], a, b)
        if e is None:
            continue
        fc, kc, c, fd, kd, d = e
        m, f0 = st.V_live + rank, st.F_live + 2 * rank
        st.P[m] = tuple(T(0.5) * (x + y) for x, y in zip(st.P[a], st.P[b]))
        st.C[m] = tuple(T(0.5) * (x + y) for x, y in zip(st.C[a], st.C[b]))
        tri = list(st.faces[fc])
        tri[(kc + 1) % 3] = m
        st.faces[fc] = tuple(tri)
        st.faces[f0] = (m, b, c)
        tri = list(st.faces[fd])
        tri[kd] = m
        st.faces[fd] = tuple(tri)
        st.faces[f0 + 1] = (m, a, d)
        touched[a] = ({fc, fd, f0, f0 + 1}, {a, b, c, d, m})
    st.V_live += done
    st.F_live += 2 * done
    return touched


# ---- collapse -------------------------------------------------------------------------------------------------------------------------------
def collapse_analyse(st, L, cap=DEFAULT_MAX_VALENCE, star=None):
    """Per vertex None (not removable) or {u: {"why": the rules v -> u breaks, "len2", "margin"}} in list order"""
    _, lo2, hi2 = thresholds(L, st.T)
    star = st.stars() if star is None else star
    nbr = Dm.neighbours(star)
    out = [None] * st.Vcap
    for v, s in enumerate(star):
        if not Dm.removable(v, s, cap):
            continue
        info = {}
        for _, _, u, a1 in s:
            a2 = next(a for _, _, a, b in s if b == u)
            why, near = set(), INF
            len2 = dist2(st.P, v, u)
            near = min(near, _rel(len2, lo2))
            if not len2 < lo2:
                why.add("long")
            if a1 == a2 or (nbr[v] & nbr[u]) - {u} != {a1, a2}:
                why.add("link")
            if len(star[u]) + len(s) - 4 > cap:
                why.add("valence")
            for _, _, w, _ in s:
                if w != u:
                    d2 = dist2(st.P, u, w)
                    near = min(near, _rel(d2, hi2))
                    if d2 > hi2:
                        why.add("stretch")
            at_u = {frozenset((a, b)) for _, _, a, b in star[u]}
            for f, k, a, b in s:
                if a == u or b == u:
                    continue
                pts = [_f64(st.P[i]) for i in st.faces[f]]
                before = Dm.face_cross(*pts)
                pts[k] = _f64(st.P[u])
                after = Dm.face_cross(*pts)
                d = _dot(before, after)
                near = min(near, _sign_margin(d, before, after))
                if not d > 0:
                    why.add("flip")
                if frozenset((a, b)) in at_u:
                    why.add("duplicate")
            info[u] = {"why": why, "len2": len2, "margin": near}
        out[v] = info
    return out


def collapse_propose(st, L, cap=DEFAULT_MAX_VALENCE, star=None, info=None):
    info = collapse_analyse(st, L, cap, star) if info is None else info
    keys, targets, margin = [], [], []
    for v, cand in enumerate(info):
        best = None
        for u, c in (cand or {}).items():
            if not c["why"]:
                k = (bits(c["len2"]), u)
                best = k if best is None or k < best else best
        keys.append(NO_KEY if best is None else (best[0] << 32) | ((v * KEY_HASH) & 0xFFFFFFFF))
        targets.append(-1 if best is None else best[1])
        margin.append(min([c["margin"] for c in (cand or {}).values()], default=INF))
    return keys, targets, margin


def collapse_apply(st, accept, targets, star=None):
    star = st.stars() if star is None else star
    touched = {}
    for v, on in enumerate(accept):
        u = targets[v]
        if not on or not 0 <= u < st.Vcap or u == v:
            continue
        written, ring = set(), {v}
        for f, k, a, b in star[v]:
            ring |= {a, b}
            written.add(f)
            st.faces[f] = None if u in (a, b) else tuple(u if j == k else st.faces[f][j] for j in range(3))
        st.removed[v] = True
        touched[v] = (written, ring)
    return touched


# ---- flip -----------------------------------------------------------------------------------------------------------------------------------
def _dev(val, t):
    return abs(val - t)


def flip_propose(st, cap=DEFAULT_MAX_VALENCE, star=None, boundary=None):
    star = st.stars() if star is None else star
    boundary = boundary_flags(star) if boundary is None else boundary
    tgt = [4 if b else 6 for b in boundary]
    val = [len(s) for s in star]
    keys, targets, margin = [], [], []
    for a, s in enumerate(star):
        best, near = None, INF
        if 3 < val[a] <= cap:
            for _, _, b, _ in s:
                e = editable(s, a, b)
                if e is None:
                    continue
                _, _, c, _, _, d = e
                if not (3 < val[b] <= cap and val[c] < cap and val[d] < cap):
                    continue
                gain = (_dev(val[a], tgt[a]) + _dev(val[b], tgt[b]) + _dev(val[c], tgt[c]) + _dev(val[d], tgt[d])) - \
                       (_dev(val[a] - 1, tgt[a]) + _dev(val[b] - 1, tgt[b]) + _dev(val[c] + 1, tgt[c]) + _dev(val[d] + 1, tgt[d]))
                if gain <= 0 or any(x == d or y == d for _, _, x, y in star[c]):
                    continue
                pa, pb, pc, pd = (_f64(st.P[i]) for i in (a, b, c, d))
                n1, n2 = Dm.face_cross(pa, pb, pc), Dm.face_cross(pb, pa, pd)
                m1, m2 = Dm.face_cross(pa, pd, pc), Dm.face_cross(pd, pb, pc)
                ok = True
                for m in (m1, m2):
                    for n in (n1, n2):
                        dd = _dot(m, n)
                        near = min(near, _sign_margin(dd, m, n))
                        ok = ok and dd > 0
                if ok and (best is None or gain > best[0] or (gain == best[0] and b < best[1])):
                    best = (gain, b)
        keys.append(NO_KEY if best is None else make_key(np.float32(8 - best[0]), a))
        targets.append(-1 if best is None else best[1])
        margin.append(near)
    return keys, targets, margin


def flip_apply(st, accept, targets, star=None):
    star = st.stars() if star is None else star
    touched = {}
    for a, on in enumerate(accept):
        b = targets[a]
        if not on or not 0 <= b < st.Vcap:
            continue
        e = editable(star[a], a, b)
        if e is None:
            continue
        fc, kc, c, fd, kd, d = e
        tri = list(st.faces[fc])
        tri[(kc + 1) % 3] = d
        st.faces[fc] = tuple(tri)
        tri = list(st.faces[fd])
        tri[kd] = c
        st.faces[fd] = tuple(tri)
        touched[a] = ({fc, fd}, {a, b, c, d})
    return touched


def potential(st):
    """the summed deviation from the target valences: every flip lowers it"""
    star = st.stars()
    return sum(abs(len(s) - (4 if b else 6)) for s, b in zip(star, boundary_flags(star)) if s)


# ---- relax, reproject -----------------------------------------------------------------------------------------------------------------------
def relax(st, lam, pinned=None, star=None, boundary=None, tangential=True, pin_boundary=True):
    """The new positions [Vcap] (st.P is left alone)"""
    T = st.T
    star = st.stars() if star is None else star
    boundary = boundary_flags(star) if boundary is None else boundary
    lam = T(np.float32(lam))
    out = []
    for v, s in enumerate(star):
        p = st.P[v]
        if (pin_boundary and boundary[v]) or (pinned is not None and pinned[v]) or not s:
            out.append(p)
            continue
        sx = sy = sz = nx = ny = nz = T(0.0)
        for f, _, a, b in s:
            pa, pb = st.P[a], st.P[b]
            sx, sy, sz = sx + T(0.5) * (pa[0] + pb[0]), sy + T(0.5) * (pa[1] + pb[1]), sz + T(0.5) * (pa[2] + pb[2])
            p0, p1, p2 = (st.P[i] for i in st.faces[f])
            ux, uy, uz = p1[0] - p0[0], p1[1] - p0[1], p1[2] - p0[2]
            wx, wy, wz = p2[0] - p0[0], p2[1] - p0[1], p2[2] - p0[2]
            nx, ny, nz = nx + (uy * wz - uz * wy), ny + (uz * wx - ux * wz), nz + (ux * wy - uy * wx)
        len2 = nx * nx + ny * ny + nz * nz
        if not len2 > T(NORMAL_EPS):
            out.append(p)
            continue
        ln, n = _sqrt(len2), T(len(s))
        nx, ny, nz = nx / ln, ny / ln, nz / ln
        dx, dy, dz = sx / n - p[0], sy / n - p[1], sz / n - p[2]
        nd = (nx * dx + ny * dy) + nz * dz if tangential else T(0.0)
        out.append((p[0] + lam * (dx - nx * nd), p[1] + lam * (dy - ny * nd), p[2] + lam * (dz - nz * nd)))
    return out


def on_triangle(a, b, c, u, v):
    q = a + u * (b - a) + v * (c - a)
    if u == 1:
        q = b
    if v == 1:
        q = c
    return q


def project_rows(P, C, face, uv, src_verts, src_colors, src_faces, T):
    """(positions, colours) after v3d_recon_remesh_project on given (face, uv) answers"""
    sv = [tuple(T(x) for x in row) for row in np.asarray(src_verts, dtype=np.float32).tolist()]
    sc = [tuple(T(x) for x in row) for row in np.asarray(src_colors, dtype=np.float32).tolist()]
    sf = Dm.face_list(src_faces)
    outP, outC = list(P), list(C)
    for i, f in enumerate(face):
        if not 0 <= f < len(sf) or not all(0 <= j < len(sv) for j in sf[f]):
            continue
        u, v = T(uv[i][0]), T(uv[i][1])
        if not (0 <= u <= 1 and 0 <= v <= 1):
            continue
        i0, i1, i2 = sf[f]
        outP[i] = tuple(on_triangle(sv[i0][j], sv[i1][j], sv[i2][j], u, v) for j in range(3))
        outC[i] = tuple(on_triangle(sc[i0][j], sc[i1][j], sc[i2][j], u, v) for j in range(3))
    return outP, outC


def project(st, src_verts, src_colors, src_faces):
    """Reprojects the state's rows onto the input mesh by mesh_query_ref.closest_point in the state's precision"""
    td = torch.float64 if st.T is float else torch.float32
    pts = torch.tensor(np.array(st.P, dtype=np.float64), dtype=td)
    got = Q.closest_point(torch.as_tensor(src_verts).float(), torch.as_tensor(src_faces), pts, dtype=td)
    st.P, st.C = project_rows(st.P, st.C, got["face"].tolist(), got["uv"].tolist(), src_verts, src_colors, src_faces, st.T)


# ---- the loop -------------------------------------------------------------------------------------------------------------------------------
def default_edge(verts, faces, target_faces=None):
    """L = sqrt(4 A / (sqrt(3) F)): the edge of the equilateral triangle that F of cover the mesh's area A"""
    p = np.asarray(verts, dtype=np.float64)
    f = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    area = 0.5 * np.linalg.norm(np.cross(p[f[:, 1]] - p[f[:, 0]], p[f[:, 2]] - p[f[:, 0]]), axis=1).sum()
    return math.sqrt(4.0 * area / (math.sqrt(3.0) * (target_faces or f.shape[0])))


def one_round(st, op, L, cap, check=None):
    """One round of `op` ("split", "collapse", "flip"); how many operations it accepted.  check(touched) sees the round's touched sets."""
    star = st.stars()
    if op == "split":
        keys, targets, _ = split_propose(st, L, cap, star)
    elif op == "collapse":
        keys, targets, _ = collapse_propose(st, L, cap, star)
    else:
        keys, targets, _ = flip_propose(st, cap, star)
    accept = Dm.select(st.faces, keys)
    if not any(accept):
        return 0
    touched = {"split": split_apply, "collapse": collapse_apply, "flip": flip_apply}[op](st, accept, targets, star)
    if check is not None:
        check(op, touched)
    return sum(accept)


def live_edges(st):
    return 3 * sum(1 for t in st.faces if t is not None) // 2


def remesh(verts, faces, colors, L=None, target_faces=None, iterations=3, lam=0.5, reproject=True, cap=DEFAULT_MAX_VALENCE,
           dtype=np.float64, spare=None, check=None):
    """(verts, faces, colors, stats): `iterations` of split rounds, collapse rounds, flip rounds, relax, reproject.  A pass ends at the
    first round that accepts nothing; RuntimeError at E + 8 rounds (4 E + 8 for flip).  When the capacity runs out the state grows and the
    pass goes on (stats["reallocations"])."""
    L = default_edge(verts, faces, target_faces) if L is None else L
    st = State(verts, faces, colors, spare, dtype)
    stats = {"target_edge": float(np.float32(L)), "ops": {"split": [], "collapse": [], "flip": []}, "rounds": {"split": [], "collapse": [], "flip": []},
             "reallocations": 0}
    for _ in range(iterations):
        for op in ("split", "collapse", "flip"):
            limit = (4 if op == "flip" else 1) * live_edges(st) + 8
            rounds = ops = 0
            while True:
                if rounds >= limit:
                    raise RuntimeError(f"remesh: the {op} pass did not end within {limit} rounds")
                before = st.V_live
                n = one_round(st, op, L, cap, check)
                if st.flag:
                    st.flag = False
                    st.grow(max(64, st.Vcap // 2))
                    stats["reallocations"] += 1
                    ops += st.V_live - before
                    rounds += 1
                    continue
                if n == 0:
                    break
                ops, rounds = ops + n, rounds + 1
            stats["ops"][op].append(ops)
            stats["rounds"][op].append(rounds)
        if lam > 0:
            st.P = relax(st, lam)
        if reproject:
            project(st, verts, colors if colors is not None else np.zeros_like(np.asarray(verts)), faces)
    v, f, c = st.result()
    return v, f, c, stats


# ---- measures -------------------------------------------------------------------------------------------------------------------------------
MEASURES = {"edges_in_range": +1, "area_cov": -1, "area_ratio": -1, "mean_min_angle": +1, "valence6": +1}          # name -> the better direction


def measures(verts, faces):
    """The five measures of a mesh's evenness.  L: the edge of the equilateral triangle with the mean face area.  "edges_in_range": the share
    of the undirected edges within [4/5 L, 4/3 L]; "area_cov": std / mean of the face areas; "area_ratio": largest / smallest; "mean_min_angle":
    the mean over the faces of the smallest angle, degrees; "valence6": the share of the vertices with faces that have 6."""
    p = np.asarray(verts, dtype=np.float64)
    f = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    if f.shape[0] == 0:
        return {k: float("nan") for k in MEASURES}
    a, b, c = p[f[:, 0]], p[f[:, 1]], p[f[:, 2]]
    area = 0.5 * np.linalg.norm(np.cross(b - a, c - a), axis=1)
    L = math.sqrt(4.0 * area.mean() / math.sqrt(3.0))
    e = np.sort(np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]]), axis=1)
    e = np.unique(e, axis=0)
    ln = np.linalg.norm(p[e[:, 0]] - p[e[:, 1]], axis=1)
    la, lb, lc = np.linalg.norm(c - b, axis=1), np.linalg.norm(a - c, axis=1), np.linalg.norm(b - a, axis=1)
    with np.errstate(invalid="ignore", divide="ignore"):
        cos = np.stack([(lb ** 2 + lc ** 2 - la ** 2) / (2 * lb * lc), (la ** 2 + lc ** 2 - lb ** 2) / (2 * la * lc),
                        (la ** 2 + lb ** 2 - lc ** 2) / (2 * la * lb)], 1)
    ang = np.degrees(np.arccos(np.clip(np.nan_to_num(cos, nan=1.0), -1.0, 1.0)))
    val = np.bincount(f.reshape(-1))
    val = val[val > 0]
    return {"edges_in_range": float(((ln >= 0.8 * L) & (ln <= 4.0 / 3.0 * L)).mean()), "area_cov": float(area.std() / area.mean()),
            "area_ratio": float(area.max() / area.min()) if area.min() > 0 else INF, "mean_min_angle": float(ang.min(1).mean()),
            "valence6": float((val == 6).mean())}


def improved(before, after):
    """per measure: did it move in its better direction"""
    return {k: (after[k] - before[k]) * s > 0 for k, s in MEASURES.items()}


# ---- scenes ---------------------------------------------------------------------------------------------------------------------------------
LOOP_CASES = Dm.LOOP_CASES          # name -> the face count of the decimation the end-to-end runs start from


@functools.lru_cache(maxsize=None)
def decimated(name):
    """(verts float32 [V, 3], faces int64 [F, 3], colors float32 [V, 3]) numpy: the scene after mesh_decimate_ref.decimate to LOOP_CASES[name]"""
    v, f, c = Dm.scene(name)
    keep, faces, _ = Dm.decimate(v, f, LOOP_CASES[name])
    return v.numpy()[keep].astype(np.float32), faces, c.numpy()[keep].astype(np.float32)


@functools.lru_cache(maxsize=None)
def loop_run(name, dtype_name="float64"):
    """The restatement's own 3 iterations on a decimated scene, computed once: (verts, faces, colors, stats)"""
    v, f, c = decimated(name)
    return remesh(v, f, c, iterations=3, dtype=np.dtype(dtype_name))


INT32_MAX = 2 ** 31 - 1
# name -> (scene, target edge as a factor of the mesh's own default_edge): the states the per-operation GPU tests run every entry on.  On the
# decimated meshes the own edge leaves long and short edges both; a factor below 1 asks for splits, one above 1 for collapses.
CASES = {"net400": ("net", 1.0), "ico3_200": ("ico3", 1.0), "net": ("net", 1.25), "ico2": ("ico2", 0.7), "ico3": ("ico3", 1.0), "noisy": ("noisy", 1.0),
         "grid": ("grid", 0.7), "flat": ("flat", 1.3), "tetrahedron": ("tetrahedron", 0.5), "octahedron": ("octahedron", 0.6),
         "bipyramid": ("bipyramid", 1.0), "dart": ("dart", 0.5), "unreferenced": ("unreferenced", 0.8), "degenerate": ("ico2", 0.7),
         "bad_indices": ("ico2", 0.7), "single": ("tetrahedron", 0.5)}
SPARE = 300                         # spare vertex rows of every case's state: Vcap = V + SPARE, the index the "bad_indices" case plants


@functools.lru_cache(maxsize=None)
def case(name):
    """(verts float32 [V, 3], faces int64 [F, 3], colors float32 [V, 3], L) numpy, built once"""
    scene, factor = CASES[name]
    if name in ("net400", "ico3_200"):
        v, f, c = decimated(scene)
        v, f, c = torch.from_numpy(v), torch.from_numpy(f), torch.from_numpy(c)
    else:
        v, f, c = Dm.scene(scene)
    L = factor * default_edge(v.numpy(), f.numpy())
    if name == "degenerate":
        v, f, c = C.add_degenerate(v, f, c)
    if name == "bad_indices":
        f = f.clone()
        f[3, 1], f[40, 0], f[77, 2], f[100] = -1, v.shape[0] + SPARE, INT32_MAX, torch.tensor([INT32_MAX, -1, -7])
    if name == "single":
        f = f[:1]
    return v.numpy().astype(np.float32), f.numpy().astype(np.int64), c.numpy().astype(np.float32), float(np.float32(L))


def proposals(name, op, dtype=np.float64, cap=DEFAULT_MAX_VALENCE):
    """(state, keys, targets, margin) of one propose entry on a case's first state"""
    v, f, c, L = case(name)
    st = State(v, f, c, SPARE, dtype)
    star = st.stars()
    if op == "split":
        return (st,) + split_propose(st, L, cap, star)
    if op == "collapse":
        return (st,) + collapse_propose(st, L, cap, star)
    return (st,) + flip_propose(st, cap, star)


def excluded(margin):
    """the vertices whose decisions the comparison leaves out"""
    return [m <= NEAR for m in margin]


# ---- against decimation ---------------------------------------------------------------------------------------------------------------------
# The planted scenes of decimation whose normal tests all lie clear of 0 (tests/test_mesh_decimate_cpu.py), and a target edge that opens the
# two length rules of the remeshing collapse wide: on these unit-scale scenes every edge is below 4/5 of it and none can come out above 4/3 of
# it.  What is left of the remeshing rule is decimation's, so the two proposers must name the same proposing vertices.
PLANTED = ("tetrahedron", "octahedron", "bipyramid", "dart", "grid")
OPEN_WIDE = 1e3


@functools.lru_cache(maxsize=None)
def decimation_verdict(name, cap=DEFAULT_MAX_VALENCE):
    """(keys, analysis) of mesh_decimate_ref on a planted scene, computed once"""
    v, f, _ = Dm.scene(name)
    faces = Dm.face_list(f)
    Qv = Dm.vertex_quadrics(v, faces)
    info = Dm.analyse(v, faces, Qv, cap)
    return Dm.propose(v, faces, Qv, cap, info=info)[0], info


def assert_collapse_proposers_agree(name, decim_keys, remesh_keys, remesh_targets, cap=DEFAULT_MAX_VALENCE):
    """The same vertices propose in both, and every remeshing target is a collapse the decimation restatement calls valid"""
    _, info = decimation_verdict(name, cap)
    assert len(decim_keys) == len(remesh_keys) == len(remesh_targets) == len(info), name
    assert [k != NO_KEY for k in remesh_keys] == [k != NO_KEY for k in decim_keys], name
    for v, u in enumerate(remesh_targets):
        assert (u == -1) == (remesh_keys[v] == NO_KEY), (name, v)
        if u >= 0:
            assert info[v] is not None and u in info[v] and not info[v][u]["why"], (name, v, u)
