"""Pure-torch restatement of csrc_recon/meshsolid.hip and of v3d_amd/recon/mesh_solid.py (test oracle), fp64 by default; with
dtype=torch.float32 what that run loses against the fp64 one is the cost of the number format (the bar idiom of tests/mesh_bake_ref.py).

Written from the statements of include/v3d_recon.h "Mesh solid".  exact_winding is a brute force over the triangles;  moments takes every
node's row from the SET of leaves below it (not from its children's rows);  tree_sum walks a given tree (left, right, order, lo, hi) with
given moments, all queries at once: the nodes are taken in pre-order, left before right, which is the order of the device's walk, and a
query visits a node when it opened every ancestor.  build_tree is a median split, a valid tree of THE NODES that need not equal the
device's;  the GPU tests walk the device's own tree and moments."""
from __future__ import annotations

import functools
import math

import numpy as np
import torch

import mesh_bake_ref as B
import mesh_query_ref as Q
import mesh_render_ref as M
import recon_geom_ref as R

F64, F32 = torch.float64, torch.float32
INF = float("inf")
GAP = 1e-5                           # a query is compared only when no far decision it took was closer than this (relative)
EXCLUDE_MAX = M.EXCLUDE_MAX          # at most 2 % of a case may be left out
SURFACE_MARGIN = 1e-3                # x the diagonal: every compared query keeps this far from the surface
_dot, _cross = B._dot, B._cross


# ---- the exact winding number -----------------------------------------------------------------------------------------------------------------
def solid_angles(verts, faces, points, dtype=F64):
    """Omega [N, F] of THE WINDING NUMBER; 0 for a face with an index outside the vertices and where num == 0"""
    f = faces.long()
    ok = ((f >= 0) & (f < verts.shape[0])).all(1)
    fz = torch.where(ok[:, None], f, torch.zeros_like(f))
    v = verts.to(dtype)
    q = points.to(dtype)[:, None, :]
    a, b, c = v[fz[:, 0]][None] - q, v[fz[:, 1]][None] - q, v[fz[:, 2]][None] - q
    num = _dot(a, _cross(b, c))
    la, lb, lc = torch.sqrt(_dot(a, a)), torch.sqrt(_dot(b, b)), torch.sqrt(_dot(c, c))
    den = la * lb * lc + _dot(a, b) * lc + _dot(b, c) * la + _dot(c, a) * lb
    om = 2.0 * torch.atan2(num, den)
    return torch.where(ok[None] & (num != 0), om, torch.zeros_like(om))


@torch.no_grad()
def exact_winding(verts, faces, points, dtype=F64, chunk=2048):
    """w [N]: the sum over every triangle, accumulated in double, over 4 pi; NaN for a query that is not finite"""
    out = []
    for s in range(0, points.shape[0], chunk):
        p = points[s:s + chunk]
        w = solid_angles(verts, faces, p, dtype).double().sum(1) / (4.0 * math.pi)
        out.append(torch.where(torch.isfinite(p).all(1), w, torch.full_like(w, float("nan"))))
    return torch.cat(out).to(dtype) if out else torch.zeros(0, dtype=dtype)


# ---- a tree of its own ------------------------------------------------------------------------------------------------------------------------
def build_tree(verts, faces):
    """dict(left, right [max(F-1, 1)] int64, order [F] int64, lo, hi [2F-1, 3] float32) in the layout of THE NODES: internal nodes 0 .. F-2
    in pre-order, leaf k = node F - 1 + k.  Median split of the box centres along the longest axis of their spread."""
    F = faces.shape[0]
    flo, fhi = B.face_boxes(verts, faces)
    ctr = np.nan_to_num(np.asarray(0.5 * (flo + fhi), dtype=np.float64), nan=0.0, posinf=0.0, neginf=0.0)
    left, right = np.full(max(F - 1, 1), -1, dtype=np.int64), np.full(max(F - 1, 1), -1, dtype=np.int64)
    order, counter = [], [0]

    def rec(ids):
        if len(ids) == 1:
            order.append(int(ids[0]))
            return F - 1 + len(order) - 1
        me = counter[0]
        counter[0] += 1
        c = ctr[ids]
        axis = int(np.argmax(c.max(0) - c.min(0)))
        ids = ids[np.argsort(c[:, axis], kind="stable")]
        half = len(ids) // 2
        left[me] = rec(ids[:half])
        right[me] = rec(ids[half:])
        return me

    rec(np.arange(F))
    order_t = torch.tensor(order, dtype=torch.long)
    lo = torch.full((2 * F - 1, 3), INF, dtype=F32)
    hi = torch.full((2 * F - 1, 3), -INF, dtype=F32)
    lo[F - 1:], hi[F - 1:] = flo[order_t], fhi[order_t]
    for n in range(F - 2, -1, -1):                       # pre-order numbering: children have larger indices than their parent
        lo[n] = torch.minimum(lo[left[n]], lo[right[n]])
        hi[n] = torch.maximum(hi[left[n]], hi[right[n]])
    return dict(left=torch.from_numpy(left), right=torch.from_numpy(right), order=order_t, lo=lo, hi=hi)


def host_tree(bvh):
    """The device's tree (mesh_bake.MeshBVH) as the dict of build_tree"""
    return dict(left=bvh.left.cpu().long(), right=bvh.right.cpu().long(), order=bvh.order.cpu().long(), lo=bvh.lo.cpu(), hi=bvh.hi.cpu())


def preorder(tree, F):
    """[(node, parent)] from the root, left before right"""
    out, stack = [], [(0, -1)]
    left, right = tree["left"].tolist(), tree["right"].tolist()
    while stack:
        n, p = stack.pop()
        out.append((n, p))
        if n < F - 1:
            stack.append((right[n], n))
            stack.append((left[n], n))
    assert len(out) == 2 * F - 1 and len({n for n, _ in out}) == 2 * F - 1, "not a tree of 2F - 1 nodes"
    return out


# ---- the moments ------------------------------------------------------------------------------------------------------------------------------
@torch.no_grad()
def moments(tree, verts, faces, dtype=F64):
    """mom [2F-1, 8] of THE MOMENTS, every node from the set of leaves below it"""
    F = faces.shape[0]
    ok, v0, e1, e2 = Q._triangles(verts, faces, dtype)
    n_f = 0.5 * _cross(e1, e2)
    a_f = torch.sqrt(_dot(n_f, n_f))
    fz = torch.where(ok[:, None], faces.long(), torch.zeros_like(faces.long()))
    v = verts.to(dtype)
    c_f = ((v[fz[:, 0]] + v[fz[:, 1]]) + v[fz[:, 2]]) / 3.0
    zero = torch.zeros((), dtype=dtype)
    n_f, a_f, c_f = torch.where(ok[:, None], n_f, zero), torch.where(ok, a_f, zero), torch.where(ok[:, None], c_f, zero)
    order = tree["order"]
    leaves = {}
    for n, _ in reversed(preorder(tree, F)):             # children before their parent
        leaves[n] = [int(order[n - (F - 1)])] if n >= F - 1 else leaves[int(tree["left"][n])] + leaves[int(tree["right"][n])]
    lo, hi = tree["lo"].to(dtype), tree["hi"].to(dtype)
    mom = torch.zeros(2 * F - 1, 8, dtype=dtype)
    for n in range(2 * F - 1):
        ids = torch.tensor(leaves[n])
        area = a_f[ids].sum()
        empty = bool((lo[n] > hi[n]).any())
        if n >= F - 1:
            c = c_f[ids[0]]
        elif float(area) > 0:
            c = (a_f[ids, None] * c_f[ids]).sum(0) / area
        else:
            c = torch.zeros(3, dtype=dtype) if empty else 0.5 * (lo[n] + hi[n])
        m = torch.maximum((c - lo[n]) ** 2, (hi[n] - c) ** 2)
        r2 = zero if empty else (m[0] + m[1]) + m[2]
        mom[n] = torch.cat([n_f[ids].sum(0), r2.reshape(1), c, area.reshape(1)])
    return mom


# ---- THE SUM ----------------------------------------------------------------------------------------------------------------------------------
@torch.no_grad()
def tree_sum(tree, mom, verts, faces, points, beta, dtype=F64):
    """(w [N], gap [N], visited [N]): THE SUM on the given tree and moments;  gap: the smallest |d2 - beta^2 r2| / (beta^2 r2) among the far
    decisions the query took (inf when it took none);  visited: nodes the query looked at"""
    F, N = faces.shape[0], points.shape[0]
    q = points.to(dtype)
    m = mom.to(dtype)
    b2 = torch.tensor(float(beta), dtype=dtype) ** 2
    total = torch.zeros(N, dtype=F64)
    gap = torch.full((N,), INF, dtype=F64)
    count = torch.zeros(N, dtype=torch.long)
    opened = {-1: torch.arange(N)}                       # per node: the queries that opened it
    none = torch.zeros(0, dtype=torch.long)
    order = tree["order"]
    for n, p in preorder(tree, F):
        idx = opened[p]
        opened[n] = none
        if idx.numel() == 0:
            continue
        count[idx] += 1
        if float(m[n, 7]) == 0:
            continue
        d = m[n, 4:7][None] - q[idx]
        d2 = _dot(d, d)
        far = torch.zeros(idx.numel(), dtype=torch.bool)
        if float(b2) > 0:
            lim = b2 * m[n, 3]
            far = d2 > lim
            if float(lim) > 0:
                gap[idx] = torch.minimum(gap[idx], (d2.double() - float(lim)).abs() / float(lim))
        if bool(far.any()):
            df, d2f = d[far], d2[far]
            total[idx[far]] += (_dot(m[n, 0:3][None].expand(df.shape[0], 3), df) / (d2f * torch.sqrt(d2f))).double()
        near = idx[~far]
        if n >= F - 1:
            f = int(order[n - (F - 1)])
            if near.numel():
                total[near] += solid_angles(verts, faces[f:f + 1], points[near], dtype)[:, 0].double()
        else:
            opened[n] = near
    w = (total / (4.0 * math.pi)).to(dtype)
    w = torch.where(torch.isfinite(points).all(1), w, torch.full_like(w, float("nan")))
    return w, gap, count


# ---- the volume -------------------------------------------------------------------------------------------------------------------------------
@torch.no_grad()
def sdf_volume(tree, mom, verts, faces, colors, N, bound, trunc, beta, dtype=F64, points=None):
    """The rule of v3d_recon_sdf_grid on Q.closest_point and tree_sum: dict(N, bound, trunc, tsdf_sum, weight [N^3], rgb_sum [3, N^3],
    rgb_weight [N^3]: a volume R.extract takes;  w, dist, gap [N^3]).  points: the voxel centres to use (default: formed in float32 as the
    kernel forms them)."""
    p = voxel_centres32(N, bound) if points is None else points
    cp = Q.closest_point(verts, faces, p, max_dist=trunc, dtype=dtype)
    w, gap, _ = tree_sum(tree, mom, verts, faces, p, beta, dtype)
    s = torch.where(w >= 0.5, -torch.ones_like(w), torch.ones_like(w))
    found = cp["face"] >= 0
    dist = torch.where(found, cp["dist"], torch.full_like(cp["dist"], INF))
    t = torch.tensor(trunc, dtype=dtype)
    tsdf = torch.where(found, s * torch.minimum(dist / t, torch.ones_like(dist)), s)
    rgb = torch.zeros(3, N ** 3, dtype=dtype)
    if colors is not None:
        f = faces.long()[cp["face"].clamp_min(0)]
        c = colors.to(dtype)
        u, v = cp["uv"][:, 0:1], cp["uv"][:, 1:2]
        mix = (1 - u - v) * c[f[:, 0]] + u * c[f[:, 1]] + v * c[f[:, 2]]
        rgb = torch.where(found[None], mix.t(), torch.zeros_like(mix.t())).contiguous()
    rw = (found if colors is not None else torch.zeros_like(found)).to(dtype)
    return dict(N=N, bound=float(bound), trunc=float(trunc), tsdf_sum=tsdf, weight=torch.ones(N ** 3, dtype=dtype), rgb_sum=rgb, rgb_weight=rw, w=w,
                dist=dist, gap=gap, face=cp["face"])


def voxel_centres32(N, bound):
    """[N^3, 3] float32: fmaf(i + 0.5, voxel, -bound) with voxel = 2 bound / N in float, as the kernel forms them: exact in double, rounded
    to float once"""
    b = torch.tensor(float(bound), dtype=F32)
    voxel = 2.0 * b / torch.tensor(float(N), dtype=F32)
    c = ((torch.arange(N, dtype=F64) + 0.5) * voxel.double() - b.double()).float()
    zz, yy, xx = torch.meshgrid(c, c, c, indexing="ij")
    return torch.stack([xx, yy, zz], -1).reshape(-1, 3)


# ---- scenes -----------------------------------------------------------------------------------------------------------------------------------
RADIUS = 0.5
CAP = 0.8                            # the open sphere: faces whose centroid lies above CAP x the radius (along z) are removed
COUNTS = B.RAY_COUNTS                # 1, 63, 64, 65, 1100 queries


@functools.lru_cache(maxsize=None)
def mesh(kind):
    """(verts, faces): "closed" the icosphere of 1280 faces, r = 0.5;  "open" the same without its cap;  "nested" the closed one around one of
    320 faces and r = 0.2;  "nested-reversed" with the inner one wound inward;  "reversed" the closed one wound inward;  "small" 320 faces"""
    v, f = M.icosphere(3, RADIUS)
    if kind == "small":
        return M.icosphere(2, RADIUS)
    if kind == "closed":
        return v, f
    if kind == "reversed":
        return v, f[:, [0, 2, 1]]
    if kind == "open":
        cz = v[f].mean(1)[:, 2]
        return v, f[cz <= CAP * RADIUS]
    v2, f2 = M.icosphere(2, 0.2, seed=4)
    if kind == "nested-reversed":
        f2 = f2[:, [0, 2, 1]]
    assert kind in ("nested", "nested-reversed"), kind
    return torch.cat([v, v2]), torch.cat([f, f2 + v.shape[0]])


def half_octahedron():
    """(verts, faces): the four upper faces of the unit octahedron, wound outward, the base open.  Seen from the origin each face is
    exactly one octant: num = 1, den = 1, Omega = 2 atan2(1, 1), so w(0) = 0.5 - in float exactly 0.5 too (8 float(pi / 4) is 2 pi
    (1 + 2.8e-8), and 0.5 (1 + 2.8e-8) rounds to 0.5): the one query that tells `w >= 0.5` from `w > 0.5`"""
    v = torch.tensor([[0.0, 0, 1], [1, 0, 0], [0, 1, 0], [-1, 0, 0], [0, -1, 0]])
    return v, torch.tensor([[0, 1, 2], [0, 2, 3], [0, 3, 4], [0, 4, 1]])


HALF_GRID = dict(N=3, bound=1.5)     # voxel (1, 1, 1) is the origin exactly: 1.5 x 1 - 1.5


def diagonal(verts):
    return float((verts.max(0).values - verts.min(0).values).double().norm())


def mesh_area(verts, faces):
    v = verts.double()
    f = faces.long()
    return float(0.5 * torch.linalg.cross(v[f[:, 1]] - v[f[:, 0]], v[f[:, 2]] - v[f[:, 0]]).norm(dim=1).sum())


@functools.lru_cache(maxsize=None)
def queries(seed=7):
    """[1100, 3] float32: 500 in the ball of radius 0.45 below z = 0.25 (inside), 400 in the shell 0.55 .. 0.8 (outside, in the root box's corners and
    beyond its faces), 200 beyond the root box on every side (a coordinate of +-0.9 .. 1.5);  shuffled, so a prefix holds every kind"""
    g = torch.Generator().manual_seed(seed)
    rnd = lambda *s: torch.rand(*s, generator=g, dtype=F64)  # noqa: E731
    sph = lambda n: torch.nn.functional.normalize(torch.randn(n, 3, generator=g, dtype=F64), dim=1)  # noqa: E731
    inside = sph(500) * 0.45 * rnd(500, 1) ** (1 / 3)
    inside[:, 2] = torch.where(inside[:, 2] > 0.25, -inside[:, 2], inside[:, 2])          # clear of the open sphere's hole, where w passes 0.5
    shell = sph(400) * (0.55 + 0.25 * rnd(400, 1))
    far = (rnd(200, 3) * 2 - 1) * 0.6
    rows = torch.arange(200)
    far[rows, rows % 3] = torch.where(rows % 2 == 0, 1.0, -1.0).to(F64) * (0.9 + 0.6 * rnd(200))
    perm = torch.randperm(1100, generator=g)
    return torch.cat([inside, shell, far])[perm].float()


@functools.lru_cache(maxsize=None)
def surface_distance(kind):
    """the fp64 distance of every query from the mesh"""
    v, f = mesh(kind)
    return Q.closest_point(v, f, queries())["dist"]


def float_bar(ref64, ref32):
    """4x the largest error of the float32 restatement against the fp64 one over the whole case (the project's standing bar)"""
    return 4.0 * float((ref32.double() - ref64.double()).abs().max())


def excluded_share(mask):
    return 1.0 - float(mask.double().mean()) if mask.numel() else 0.0


# the volumes of the GPU test: (mesh, N, bound, with colours)
# (the bounds are the first of 0.70, 0.71, .. at which every voxel centre keeps SURFACE_MARGIN x the diagonal from the surface)
GRID_CASES = (("open", 8, 0.71, True), ("open", 18, 0.71, True), ("open", 22, 0.71, True), ("closed", 24, 0.8, True), ("closed", 24, 0.8, False))
BETAS = (2.0, 3.0)
GRID_BETA = 2.0


@functools.lru_cache(maxsize=None)
def cpu_case(kind):
    """(verts, faces, tree, mom64, mom32) on the median-split tree: computed once and shared"""
    v, f = mesh(kind)
    tree = build_tree(v, f)
    return v, f, tree, moments(tree, v, f), moments(tree, v, f, F32)


@functools.lru_cache(maxsize=None)
def cpu_winding(kind, beta):
    """(w64, gap, w32) of all 1100 queries on the median-split tree"""
    v, f, tree, m64, m32 = cpu_case(kind)
    w, gap, _ = tree_sum(tree, m64, v, f, queries(), beta)
    return w, gap, tree_sum(tree, m32, v, f, queries(), beta, F32)[0]


@functools.lru_cache(maxsize=None)
def cpu_volume(case):
    kind, N, bound, rgb = case
    v, f, tree, m64, m32 = cpu_case(kind)
    c = M.position_colors(v) if rgb else None
    t = grid_trunc(N, bound)
    return sdf_volume(tree, m64, v, f, c, N, bound, t, GRID_BETA), sdf_volume(tree, m32, v, f, c, N, bound, t, GRID_BETA, F32)
E2E = dict(N=24, bound=0.7, radius=RADIUS)


def grid_case_id(case):
    return f"{case[0]}-n{case[1]}-{'rgb' if case[3] else 'plain'}"


def grid_trunc(N, bound):
    return 4.0 * 2.0 * bound / N


def volume_mask(ref64, ref32, trunc):
    """Which voxels of a volume are compared: the decision gap at least GAP, the fp64 |w - 0.5| at least the bar on w, the fp64 distance
    further than that bar from trunc"""
    bar_w = float_bar(ref64["w"], ref32["w"])
    d = ref64["dist"]
    near_trunc = torch.isfinite(d) & ((d - trunc).abs() < bar_w)
    return (ref64["gap"] >= GAP) & ((ref64["w"] - 0.5).abs() >= bar_w) & ~near_trunc


def cap_vertices(out_verts, in_verts, in_faces, voxel):
    """the vertices of a result farther than two voxels from every input face"""
    d = Q.closest_point(in_verts, in_faces, torch.as_tensor(out_verts).float())["dist"]
    return d > 2.0 * voxel


def rim_heights(kind="open"):
    """(lowest, highest) z of the vertices on the open sphere's boundary edges"""
    v, f = mesh(kind)
    und, cnt, _ = R.undirected_counts(f.numpy())
    rim = np.unique(und[cnt == 1])
    z = v[torch.from_numpy(rim)][:, 2]
    return float(z.min()), float(z.max())
