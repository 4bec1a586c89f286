"""Pure-torch restatement of csrc_recon/meshtopo.hip (test oracle) and the scenes of tests/test_mesh_clean_{cpu,gpu}.py, written from the
statements of include/v3d_recon.h "Mesh topology".  fp64 by default; `dtype=torch.float32` runs the same statements, in the same order, in
single precision (what that run loses against the fp64 one is the cost of the number format).  Every sum over a vertex's list adds the
entries in list order: entry j of every vertex is added in step j."""
from __future__ import annotations

import numpy as np
import torch

import mesh_render_ref as M
import recon_geom_ref as R

NORMAL_EPS = 1e-20          # the squared length at or below which a normal sum counts as none
NORMAL_MARGIN = 1e-18       # every scene keeps every squared normal sum exactly 0 or above this: fp32 and fp64 decide alike


# ---- the lists ----------------------------------------------------------------------------------------------------------------------------
def corner_lists(faces, V):
    """(ranges [V, 2], corners [3F]) int64: the stable sort of the corners 3 f + k on their vertex"""
    flat = faces.long().reshape(-1)
    corners = torch.argsort(flat, stable=True)
    length = torch.bincount(flat, minlength=V)
    end = torch.cumsum(length, 0)
    ranges = torch.stack([end - length, end], 1)
    ranges[length == 0] = 0
    return ranges, corners


def list_table(faces, V):
    """(table [V, L] int64 of corners, -1 beyond a list's end; length [V])"""
    ranges, corners = corner_lists(faces, V)
    length = ranges[:, 1] - ranges[:, 0]
    L = int(length.max()) if V else 0
    table = torch.full((V, max(L, 1)), -1, dtype=torch.long)
    for j in range(L):
        has = length > j
        table[has, j] = corners[ranges[has, 0] + j]
    return table, length


def _entries(faces, table, j):
    """Of step j: which vertices have an entry, its three vertices (i0, i1, i2) and the two neighbours (a, b) of the entry's corner"""
    has = table[:, j] >= 0
    c = table[has, j]
    f, k = torch.div(c, 3, rounding_mode="floor"), c % 3
    tri = faces.long()[f]
    a, b = tri.gather(1, ((k + 1) % 3)[:, None])[:, 0], tri.gather(1, ((k + 2) % 3)[:, None])[:, 0]
    return has, tri, a, b


# ---- normals ------------------------------------------------------------------------------------------------------------------------------
@torch.no_grad()
def normal_sums(verts, faces, dtype=torch.float64):
    """[V, 3]: the sum in list order of (v1 - v0) x (v2 - v0) over every vertex's faces"""
    p = verts.to(dtype)
    V = p.shape[0]
    table, _ = list_table(faces, V)
    s = torch.zeros(V, 3, dtype=dtype)
    for j in range(table.shape[1]):
        has, tri, _, _ = _entries(faces, table, j)
        if not bool(has.any()):
            break
        a = p[tri[:, 0]]
        u, w = p[tri[:, 1]] - a, p[tri[:, 2]] - a
        cr = torch.stack([u[:, 1] * w[:, 2] - u[:, 2] * w[:, 1], u[:, 2] * w[:, 0] - u[:, 0] * w[:, 2], u[:, 0] * w[:, 1] - u[:, 1] * w[:, 0]], 1)
        s[has] = s[has] + cr
    return s


def _has_normal(s):
    len2 = s[:, 0] * s[:, 0] + s[:, 1] * s[:, 1] + s[:, 2] * s[:, 2]
    return len2, len2 > torch.tensor(NORMAL_EPS, dtype=torch.float32).to(s.dtype)


def has_normal(verts, faces, dtype=torch.float64):
    """[V] bool: the vertices whose normal sum is long enough to be normalised (the others get 0 0 1)"""
    return _has_normal(normal_sums(verts, faces, dtype))[1]


@torch.no_grad()
def normals(verts, faces, dtype=torch.float64):
    s = normal_sums(verts, faces, dtype)
    len2, ok = _has_normal(s)
    n = s / torch.sqrt(torch.where(ok, len2, torch.ones_like(len2)))[:, None]
    return torch.where(ok[:, None], n, torch.tensor([0.0, 0.0, 1.0], dtype=dtype)[None])


def normal_len2(verts, faces):
    s = normal_sums(verts, faces)
    return (s * s).sum(1)


# ---- components -----------------------------------------------------------------------------------------------------------------------------
def label_round(faces, labels, jump=True):
    f = faces.long()
    fmin = labels[f].min(1).values                                     # the smallest label on every face
    m = labels.clone()
    m.scatter_reduce_(0, f.reshape(-1), fmin.repeat_interleave(3), "amin")
    return labels[m] if jump else m


def components(faces, V, jump=True):
    """(labels [V] int64, rounds): the rule of v3d_recon_mesh_label_round from labels = 0 .. V-1; rounds counts up to and including the first
    round that changes nothing"""
    labels = torch.arange(V)
    if faces.shape[0] == 0:
        return labels, 0
    for r in range(1, V + 9):
        new = label_round(faces, labels, jump)
        if torch.equal(new, labels):
            return labels, r
        labels = new
    raise AssertionError("no fixed point")


def component_table(faces, V, labels):
    """[{"root", "faces", "vertices"}] of the components with a face, by ascending root"""
    f = faces.long()
    nf = torch.bincount(labels[f[:, 0]], minlength=V)
    nv = torch.bincount(labels, minlength=V)
    return [{"root": r, "faces": int(nf[r]), "vertices": int(nv[r])} for r in torch.nonzero(nf > 0).reshape(-1).tolist()]


def kept_roots(table, min_faces, keep_largest):
    rows = [r for r in table if r["faces"] >= min_faces]
    if keep_largest > 0:
        rows.sort(key=lambda r: r["root"])
        rows.sort(key=lambda r: r["faces"], reverse=True)              # (stable: the smaller root first among equals)
        rows = rows[:keep_largest]
    return sorted(r["root"] for r in rows)


def filter_components(verts, faces, colors, min_faces=64, keep_largest=0):
    """(verts, faces, colors, keep_face [F] bool, keep_vert [V] bool, table)"""
    V = verts.shape[0]
    f = faces.long()
    labels, _ = components(f, V)
    table = component_table(f, V, labels)
    keep_root = torch.zeros(V, dtype=torch.bool)
    keep_root[kept_roots(table, min_faces, keep_largest)] = True
    used = torch.zeros(V, dtype=torch.bool)
    used[f.reshape(-1)] = True
    keep_vert, keep_face = keep_root[labels] & used, keep_root[labels[f[:, 0]]]
    new = torch.cumsum(keep_vert.long(), 0) - keep_vert.long()
    return verts[keep_vert], new[f[keep_face]], colors[keep_vert], keep_face, keep_vert, table


# ---- boundary -------------------------------------------------------------------------------------------------------------------------------
def boundary_flags(faces, V):
    """[V] int64: 1 where some neighbour other than the vertex itself is a neighbour in exactly one entry of the vertex's list"""
    entries = [[] for _ in range(V)]
    for tri in faces.tolist():
        for k in range(3):
            entries[tri[k]].append((tri[(k + 1) % 3], tri[(k + 2) % 3]))
    flags = torch.zeros(V, dtype=torch.long)
    for v, ent in enumerate(entries):
        for u in {x for pair in ent for x in pair if x != v}:
            if sum(1 for a, b in ent if a == u or b == u) == 1:
                flags[v] = 1
                break
    return flags


# ---- smoothing ------------------------------------------------------------------------------------------------------------------------------
@torch.no_grad()
def smooth_pass(p, faces, table, length, factor, pinned=None):
    """out = in + factor (mean - in) in p's dtype, the mean over the list in list order of (a + b) / 2"""
    s = torch.zeros_like(p)
    for j in range(table.shape[1]):
        has, _, a, b = _entries(faces, table, j)
        if not bool(has.any()):
            break
        s[has] = s[has] + 0.5 * (p[a] + p[b])
    move = length > 0
    if pinned is not None:
        move = move & (pinned == 0)
    n = length.clamp_min(1).to(p.dtype)[:, None]
    out = p + torch.tensor(factor, dtype=torch.float32).to(p.dtype) * (s / n - p)
    return torch.where(move[:, None], out, p)


@torch.no_grad()
def taubin(verts, faces, iterations=10, lam=0.5, mu=-0.53, fix_boundary=False, dtype=torch.float64):
    p = verts.to(dtype)
    V = p.shape[0]
    table, length = list_table(faces, V)
    pinned = boundary_flags(faces, V) if fix_boundary else None
    for _ in range(iterations):
        for factor in (lam, mu):
            p = smooth_pass(p, faces, table, length, factor, pinned)
    return p


# ---- the float bar --------------------------------------------------------------------------------------------------------------------------
def float_bar(out, ref64, ref32):
    """(error of `out`, error of the float32 restatement, bound): the kernel may be off from the fp64 restatement by 4 x what the float32 run
    of the restatement is off, or by 2^-23 x the largest magnitude in the array when that is larger (a scene where float32 happens to be
    exact)."""
    err = float((out.double() - ref64).abs().max())
    err32 = float((ref32.double() - ref64).abs().max())
    return err, err32, max(4.0 * err32, 2.0 ** -23 * float(ref64.abs().max()))


# ---- scenes ---------------------------------------------------------------------------------------------------------------------------------
SPHERE = dict(N=24, bound=1.0, radius=0.5)
NOISE_VOXELS = 0.25


def sphere_mesh(N=SPHERE["N"]):
    """(verts float32, faces int64, colors float32) of the restatement's surface nets on the sphere volume, vertices in raster order"""
    v, f, c, _, _ = R.extract(R.sphere_volume(N, SPHERE["bound"], SPHERE["radius"]))
    return v.float(), f, c.float()


def noisy_sphere(seed, N=SPHERE["N"]):
    """sphere_mesh with every vertex moved along its radius by Gaussian noise of NOISE_VOXELS voxels"""
    v, f, c = sphere_mesh(N)
    g = torch.Generator().manual_seed(seed)
    step = NOISE_VOXELS * (2.0 * SPHERE["bound"] / N) * torch.randn(v.shape[0], generator=g, dtype=torch.float64)
    vd = v.double()
    return (vd + step[:, None] * vd / vd.norm(dim=1, keepdim=True)).float(), f, c


FAN = 700


def fan(n=FAN):
    """A closed fan of n triangles around vertex 0 (a shallow cone): its list is longer than a block"""
    t = torch.arange(n, dtype=torch.float64) * (2 * np.pi / n)
    ring = torch.stack([torch.cos(t), torch.sin(t), 0.1 * torch.sin(3 * t)], 1)
    v = torch.cat([torch.tensor([[0.0, 0.0, 0.4]], dtype=torch.float64), ring]).float()
    i = torch.arange(n)
    return v, torch.stack([torch.zeros(n, dtype=torch.long), 1 + i, 1 + (i + 1) % n], 1), M.position_colors(v)


def triangle():
    v = torch.tensor([[0.0, 0.0, 0.0], [1.0, 0.0, 0.0], [0.0, 1.0, 0.25]])
    return v, torch.tensor([[0, 1, 2]]), M.position_colors(v)


def insert_unreferenced(v, f, c, at=(0, 5, 5, 17), seed=3):
    """The mesh with one more vertex, used by no face, in front of every old index of `at` (and one at the very end)"""
    g = torch.Generator().manual_seed(seed)
    V = v.shape[0]
    shift = torch.zeros(V + 1, dtype=torch.long)
    for i in at:
        shift[min(i, V):] += 1
    n = V + len(at) + 1
    nv, nc = torch.rand(n, 3, generator=g) - 0.5, torch.rand(n, 3, generator=g)
    new = torch.arange(V) + shift[:V]
    nv[new], nc[new] = v, c
    return nv, new[f], nc, new


def add_degenerate(v, f, c):
    """Two more faces on six more vertices: three vertices at one point, and three on one line at exactly representable steps: both cross
    products are exactly 0 in either precision, so their vertices get the default normal"""
    p = torch.tensor([[0.75, -0.5, 0.25]]).expand(3, 3)
    d = torch.tensor([0.25, 0.5, 0.125])
    q = torch.stack([torch.ones(3), torch.ones(3) + d, torch.ones(3) + 2 * d])
    V = v.shape[0]
    extra = torch.cat([p, q])
    return torch.cat([v, extra]), torch.cat([f, torch.tensor([[V, V + 1, V + 2], [V + 3, V + 4, V + 5]])]), torch.cat([c, M.position_colors(extra)])


def permute_vertices(v, f, c, seed):
    """The same mesh under a seeded permutation of the vertex indices: old vertex i is new vertex perm[i]"""
    perm = torch.randperm(v.shape[0], generator=torch.Generator().manual_seed(seed))
    nv, nc = torch.empty_like(v), torch.empty_like(c)
    nv[perm], nc[perm] = v, c
    return nv, perm[f], nc, perm


def floater_scene(seed=11, permute=True):
    """mesh_scene("pair") (two icospheres of 320 faces) + two single triangles + a tetrahedron + three vertices that no face uses, all under a
    seeded permutation of the vertex indices.  (verts, faces, colors, perm or None)"""
    v, f, c = M.mesh_scene("pair", M.SEEDS["pair"])
    V = v.shape[0]
    t1 = torch.tensor([[0.8, 0.8, 0.8], [0.85, 0.8, 0.8], [0.8, 0.85, 0.82]])
    t2 = -t1
    tet = torch.tensor([[0.7, -0.7, 0.0], [0.75, -0.7, 0.0], [0.7, -0.65, 0.0], [0.72, -0.68, 0.05]])
    loose = torch.tensor([[0.9, 0.0, 0.0], [0.0, 0.9, 0.0], [0.0, 0.0, 0.9]])
    extra = torch.cat([t1, t2, tet, loose])
    ef = torch.tensor([[0, 1, 2], [3, 4, 5], [6, 8, 7], [6, 7, 9], [7, 8, 9], [8, 6, 9]]) + V
    v, f, c = torch.cat([v, extra]), torch.cat([f, ef]), torch.cat([c, M.position_colors(extra)])
    if not permute:
        return v, f, c, None
    return permute_vertices(v, f, c, seed)


def quad_strip(n=500, seed=None):
    """n quads in a row (2 n triangles on 2 (n + 1) vertices, numbered along the strip), optionally under a seeded permutation"""
    i = torch.arange(n + 1, dtype=torch.float32)
    v = torch.stack([torch.stack([i, torch.zeros_like(i), torch.zeros_like(i)], 1), torch.stack([i, torch.ones_like(i), torch.zeros_like(i)], 1)], 1).reshape(-1, 3)
    q = torch.arange(n)
    a, b, c, d = 2 * q, 2 * q + 2, 2 * q + 3, 2 * q + 1
    f = torch.stack([torch.stack([a, b, c], 1), torch.stack([a, c, d], 1)], 1).reshape(-1, 3)
    col = M.position_colors(v / n)
    if seed is None:
        return v, f, col, None
    return permute_vertices(v, f, col, seed)


def open_grid():
    """The pixel-aligned quad grid of mesh_render_ref as a flat world-space mesh with a boundary (alternating diagonals)"""
    q, f, _ = M.quad_grid(split=2)
    v = torch.cat([q.float() / (256.0 * 16.0) - 0.5, torch.zeros(q.shape[0], 1)], 1)
    v[:, 2] = 0.05 * torch.sin(7 * v[:, 0]) * torch.cos(5 * v[:, 1])
    return v, f, M.position_colors(v)

