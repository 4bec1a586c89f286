"""Pure-torch restatement of csrc_recon/meshquery.hip and of v3d_amd/recon/mesh_query.py (test oracle), fp64 by default; with
dtype=torch.float32 what that run loses against the fp64 one is the cost of the number format (the bar idiom of tests/mesh_bake_ref.py).

Written from the statements of include/v3d_recon.h "Mesh queries".  Every query is a brute force over the triangles: the tree does not enter.
occlusion() may leave out, per block of points, the triangles no ray of the block can reach (further from every origin than the rays are
long): a conservative saving that `cull=False` turns off, and tests/test_mesh_query_cpu.py holds the two to the same counts."""
from __future__ import annotations

import functools
import math

import numpy as np
import torch

import mesh_bake_ref as B
import mesh_render_ref as M
import mesh_texture_ref as TX

F64, F32 = torch.float64, torch.float32
INF = float("inf")
BARY_MARGIN, T_MARGIN = B.BARY_MARGIN, B.T_MARGIN
MARGINAL_MAX = M.EXCLUDE_MAX         # at most 2 % of a case's rays may be marginal
FACE_GAP = 1e-5                      # `face` is compared where the runner-up is further than this
THIRD, TWO_THIRDS = float(np.float32(1.0 / 3.0)), float(np.float32(2.0 / 3.0))
_dot, _cross = B._dot, B._cross


def _triangles(verts, faces, dtype):
    """(ok [F], a, e1, e2 [F, 3]) with the faces whose indices are not vertices zeroed"""
    V = verts.shape[0]
    f = faces.long()
    ok = ((f >= 0) & (f < V)).all(1)
    fz = torch.where(ok[:, None], f, torch.zeros_like(f))
    v = verts.to(dtype)
    a = v[fz[:, 0]]
    return ok, a, v[fz[:, 1]] - a, v[fz[:, 2]] - a


# ---- the closest point ------------------------------------------------------------------------------------------------------------------------
def triangle_regions(p, a, e1, e2):
    """(u, v, region) of THE CLOSEST POINT OF A TRIANGLE, broadcast; region: 0 vertex a, 1 vertex b, 2 edge ab, 3 vertex c, 4 edge ac,
    5 edge bc, 6 inside"""
    b, c = a + e1, a + e2
    d1, d2 = _dot(e1, p - a), _dot(e2, p - a)
    d3, d4 = _dot(e1, p - b), _dot(e2, p - b)
    d5, d6 = _dot(e1, p - c), _dot(e2, p - c)
    vc, vb, va = d1 * d4 - d3 * d2, d5 * d2 - d1 * d6, d3 * d6 - d5 * d4
    m, n = d4 - d3, d5 - d6
    conds = [(d1 <= 0) & (d2 <= 0), (d3 >= 0) & (d4 <= d3), (vc <= 0) & (d1 >= 0) & (d3 <= 0), (d6 >= 0) & (d5 <= d6),
             (vb <= 0) & (d2 >= 0) & (d6 <= 0), (va <= 0) & (m >= 0) & (n >= 0)]
    one, zero = torch.ones_like(d1), torch.zeros_like(d1)
    safe = lambda x: torch.where(x != 0, x, one)  # noqa: E731   (only ever used where the region's condition makes it nonzero, or discarded)
    w = m / safe(m + n)
    s = safe(va + vb + vc)
    us = [zero, one, d1 / safe(d1 - d3), zero, zero, 1 - w, vb / s]
    vs = [zero, zero, zero, one, d2 / safe(d2 - d6), w, vc / s]
    u, v, region = us[6], vs[6], torch.full(d1.shape, 6, dtype=torch.long)
    for k in range(5, -1, -1):
        u, v = torch.where(conds[k], us[k], u), torch.where(conds[k], vs[k], v)
        region = torch.where(conds[k], torch.full_like(region, k), region)
    return u, v, region


@torch.no_grad()
def closest_point(verts, faces, points, max_dist=INF, dtype=F64, chunk=2048):
    """dict(dist [N], face [N] int64 (-1: a miss), uv [N, 2], region [N], runner [N]: the distance of the nearest OTHER face, max_dist or not).
    Every point against every triangle; the smallest d2 within max_dist^2 (closed), the smaller face on equal d2."""
    ok, a, e1, e2 = _triangles(verts, faces, dtype)
    ng = _cross(e1, e2)
    fz = torch.where(ok[:, None], faces.long(), torch.zeros_like(faces.long()))
    v_all, fb, fc = verts.to(dtype), fz[:, 1], fz[:, 2]
    ok = ok & (ng != 0).any(1)
    p_all = points.to(dtype)
    N = p_all.shape[0]
    md = torch.tensor(max_dist, dtype=dtype)
    max_d2 = md * md
    out = dict(dist=torch.full((N,), INF, dtype=dtype), face=torch.full((N,), -1, dtype=torch.long), uv=torch.zeros(N, 2, dtype=dtype),
               region=torch.full((N,), -1, dtype=torch.long), runner=torch.full((N,), INF, dtype=dtype))
    for s in range(0, N, chunk):
        p = p_all[s:s + chunk, None, :]
        n = p.shape[0]
        u, v, region = triangle_regions(p, a[None], e1[None], e2[None])
        q = a[None] + u[..., None] * e1[None] + v[..., None] * e2[None]
        q = torch.where((u == 1)[..., None], (v_all[fb])[None], q)
        q = torch.where((v == 1)[..., None], (v_all[fc])[None], q)
        r = p - q
        d2 = _dot(r, r)
        finite = torch.isfinite(p).all(-1)
        d2 = torch.where(ok[None] & finite, d2, torch.full_like(d2, INF))
        live = (d2 <= max_d2) & torch.isfinite(d2)          # (a d2 that is not finite is skipped, max_dist = inf or not)
        dd = torch.where(live, d2, torch.full_like(d2, INF))
        best = dd.min(1).values
        first = ((dd == best[:, None]) & live).to(torch.int8).argmax(1)
        found = live.any(1)
        rows = torch.arange(n)
        out["dist"][s:s + n] = torch.where(found, torch.sqrt(best), torch.full_like(best, INF))
        out["face"][s:s + n] = torch.where(found, first, torch.full_like(first, -1))
        out["uv"][s:s + n] = torch.where(found[:, None], torch.stack([u[rows, first], v[rows, first]], -1), torch.zeros(n, 2, dtype=dtype))
        out["region"][s:s + n] = torch.where(found, region[rows, first], torch.full_like(first, -1))
        other = d2.clone()
        other[rows, first] = INF
        out["runner"][s:s + n] = torch.sqrt(other.min(1).values)
    return out


def rebuilt_distance(verts, faces, points, face, uv):
    """|p - (a + u e1 + v e2)| in fp64 from a (face, uv) answer; inf where face < 0"""
    v, f = verts.double(), faces.long()[face.long().clamp_min(0)]
    a = v[f[:, 0]]
    q = a + uv[:, 0:1].double() * (v[f[:, 1]] - a) + uv[:, 1:2].double() * (v[f[:, 2]] - a)
    d = (points.double() - q).norm(dim=1)
    return torch.where(face >= 0, d, torch.full_like(d, INF))


# ---- the samples ------------------------------------------------------------------------------------------------------------------------------
def sample_order(n):
    """[(i, j, t)] of k = 0 .. n^2 - 1: the upright sub-triangles row by row, then the inverted ones"""
    up = [(i, j, THIRD) for j in range(n) for i in range(n - j)]
    return up + [(i, j, TWO_THIRDS) for j in range(n - 1) for i in range(n - 1 - j)]


@torch.no_grad()
def face_samples(verts, faces, n, dtype=F64):
    """(points [F n^2, 3], weights [F n^2], b [n^2, 2]: the barycentrics b1, b2 of every k)"""
    ok, a, e1, e2 = _triangles(verts, faces, dtype)
    ijt = torch.tensor(sample_order(n), dtype=dtype)
    nn = torch.tensor(float(n), dtype=dtype)
    b1, b2 = (ijt[:, 0] + ijt[:, 2]) / nn, (ijt[:, 1] + ijt[:, 2]) / nn
    pts = a[:, None, :] + b1[None, :, None] * e1[:, None, :] + b2[None, :, None] * e2[:, None, :]
    ng = _cross(e1, e2)
    w = 0.5 * torch.sqrt(_dot(ng, ng)) / torch.tensor(float(n * n), dtype=dtype)
    pts = torch.where(ok[:, None, None], pts, torch.zeros_like(pts))
    w = torch.where(ok, w, torch.zeros_like(w))
    return pts.reshape(-1, 3), w[:, None].expand(-1, n * n).reshape(-1), torch.stack([b1, b2], 1)


# ---- the directions ---------------------------------------------------------------------------------------------------------------------------
def point_hash(index, seed):
    """h of DIRECTION k OF POINT i, numpy uint64 arithmetic masked to 32 bits"""
    m = np.uint64(0xFFFFFFFF)
    h = ((np.asarray(index, dtype=np.uint64) + np.uint64(1)) * np.uint64(0x9E3779B9) & m) ^ np.uint64(seed)
    h ^= h >> np.uint64(16)
    h = h * np.uint64(0x85EBCA6B) & m
    h ^= h >> np.uint64(13)
    h = h * np.uint64(0xC2B2AE35) & m
    h ^= h >> np.uint64(16)
    return h


def valid_points(points, normals):
    len2 = (normals.float() * normals.float()).sum(1)
    return torch.isfinite(points).all(1) & (len2 > 1e-20) & torch.isfinite(len2)


@torch.no_grad()
def sample_directions(normals, K, seed=0, dtype=F64, index=None):
    """(d [N, K, 3], n [N, 3] the unit normals, z [K]) for points index[i] (default 0 .. N-1).  Rows of normals without length are garbage."""
    N = normals.shape[0]
    index = np.arange(N) if index is None else np.asarray(index)
    h = point_hash(index, seed)
    x = (np.arange(K, dtype=np.uint64)[None, :] * np.uint64(2654435769) + h[:, None]) & np.uint64(0xFFFFFFFF)
    if dtype == F32:
        frac = torch.from_numpy(x.astype(np.float32)) * torch.tensor(2.0 ** -32, dtype=F32)
        ang = (2.0 * frac).double() * math.pi                                   # sincospif: the sine and cosine of pi x, rounded once
        cs, sn = torch.cos(ang).to(F32), torch.sin(ang).to(F32)
    else:
        ang = torch.from_numpy(x.astype(np.float64)) * (2.0 * math.pi / 2.0 ** 32)
        cs, sn = torch.cos(ang), torch.sin(ang)
    k = torch.arange(K, dtype=dtype)
    u = (k + 0.5) / torch.tensor(float(K), dtype=dtype)
    r, z = torch.sqrt(u), torch.sqrt(1 - u)
    nn = normals.to(dtype)
    n = nn / torch.sqrt(_dot(nn, nn))[:, None]
    s = torch.where(torch.signbit(n[:, 2]), -torch.ones_like(n[:, 2]), torch.ones_like(n[:, 2]))
    a = -1.0 / (s + n[:, 2])
    b = n[:, 0] * n[:, 1] * a
    t1 = torch.stack([1 + s * n[:, 0] * n[:, 0] * a, s * b, -s * n[:, 0]], 1)
    t2 = torch.stack([b, s + n[:, 1] * n[:, 1] * a, -n[:, 1]], 1)
    d = (r[None, :] * cs)[..., None] * t1[:, None, :] + (r[None, :] * sn)[..., None] * t2[:, None, :] + z[None, :, None] * n[:, None, :]
    return d, n, z


# ---- occlusion --------------------------------------------------------------------------------------------------------------------------------
@torch.no_grad()
def occlusion(verts, faces, points, normals, K, radius, bias, seed=0, dtype=F64, index=None, cull=True, block=64):
    """dict(valid [N] bool, sure [N], marginal [N] int64, hits [N]: the count by the header's test itself).  sure: rays with a triangle hit
    clear of the margins (u, v, 1 - u - v >= BARY_MARGIN, T_MARGIN <= t <= radius - T_MARGIN);  marginal: rays with no such hit but a triangle
    not clearly missed (u, v, 1 - u - v >= -BARY_MARGIN, -T_MARGIN <= t <= radius + T_MARGIN).  -1 everywhere on points that are not valid."""
    ok, a, e1, e2 = _triangles(verts, faces, dtype)
    N = points.shape[0]
    index = np.arange(N) if index is None else np.asarray(index)
    valid = valid_points(points, normals)
    out = {k: torch.full((N,), -1, dtype=torch.long) for k in ("sure", "marginal", "hits")}
    out["valid"] = valid
    rows_all = torch.nonzero(valid).reshape(-1)
    centre = a + (e1 + e2) / 3
    reach = torch.stack([(a - centre).norm(dim=1), (a + e1 - centre).norm(dim=1), (a + e2 - centre).norm(dim=1)]).max(0).values
    for s in range(0, rows_all.numel(), block):
        rows = rows_all[s:s + block]
        d, n, _ = sample_directions(normals[rows], K, seed, dtype, index[rows.numpy()])
        o = points[rows].to(dtype) + torch.tensor(bias, dtype=dtype) * n
        sel = ok.clone()
        if cull:                    # a triangle further from every origin of the block than radius (+ the margin, + 1e-6 for the rounding)
            near = ((o[:, None, :] - centre[None]).norm(dim=2) <= reach[None] + radius + T_MARGIN + 1e-6).any(0)
            sel &= near
        ia = torch.nonzero(sel).reshape(-1)
        A, E1, E2 = a[ia][None, None], e1[ia][None, None], e2[ia][None, None]                    # [1, 1, T, 3]
        D, O = d[:, :, None, :], o[:, None, None, :]
        p = _cross(D, E2)
        det = _dot(E1, p)
        live = det != 0
        inv = 1.0 / torch.where(live, det, torch.ones_like(det))
        sv = O - A
        u = _dot(sv, p) * inv
        q = _cross(sv, E1)
        v = _dot(D, q) * inv
        t = _dot(E2, q) * inv
        w = 1 - u - v
        hit = live & (u >= 0) & (v >= 0) & (u + v <= 1) & (t >= 0) & (t <= radius)
        clear = live & (u >= BARY_MARGIN) & (v >= BARY_MARGIN) & (w >= BARY_MARGIN) & (t >= T_MARGIN) & (t <= radius - T_MARGIN)
        wide = live & (u >= -BARY_MARGIN) & (v >= -BARY_MARGIN) & (w >= -BARY_MARGIN) & (t >= -T_MARGIN) & (t <= radius + T_MARGIN)
        sure = clear.any(2)
        out["sure"][rows] = sure.sum(1)
        out["marginal"][rows] = (~sure & wide.any(2)).sum(1)
        out["hits"][rows] = hit.any(2).sum(1)
    return out


# ---- the distance -----------------------------------------------------------------------------------------------------------------------------
def _one_way(v, f, n, tv, tf, dtype):
    pts, w, _ = face_samples(v, f, n, dtype)
    r = closest_point(tv, tf, torch.cat([pts, v.to(dtype)]), INF, dtype)
    d, w = r["dist"].double(), w.double()
    ds = d[:pts.shape[0]]
    return {"mean": float((ds * w).sum() / w.sum()), "rms": math.sqrt(float((ds * ds * w).sum() / w.sum())), "max": float(d.max()),
            "vertex_max": float(d[pts.shape[0]:].max()), "dists": d}


@torch.no_grad()
def mesh_distance(a_verts, a_faces, b_verts, b_faces, n=2, dtype=F64):
    """The dict of v3d_amd.recon.mesh_query.mesh_distance without its timings (and per direction "vertex_max" and "dists", every queried
    point's distance, samples first)"""
    ab, ba = _one_way(a_verts, a_faces, n, b_verts, b_faces, dtype), _one_way(b_verts, b_faces, n, a_verts, a_faces, dtype)
    diag = float((b_verts.double().max(0).values - b_verts.double().min(0).values).norm())
    return {"a_to_b": ab, "b_to_a": ba, "hausdorff": max(ab["max"], ba["max"]), "chamfer": 0.5 * (ab["mean"] + ba["mean"]), "diagonal": diag}


def distance_figures(d):
    """the seven absolute figures of a mesh_distance dict, in one order"""
    return [d["a_to_b"]["mean"], d["a_to_b"]["rms"], d["a_to_b"]["max"], d["b_to_a"]["mean"], d["b_to_a"]["rms"], d["b_to_a"]["max"], d["hausdorff"],
            d["chamfer"]]


# ---- the AO bake ------------------------------------------------------------------------------------------------------------------------------
@torch.no_grad()
def texel_frames(low_verts, low_faces, low_normals, R, dtype=F64):
    """(owner [R*R], cast [R*R] bool, P [R*R, 3], n [R*R, 3]): mesh_bake_ref.bake's texel rule up to the casts (NaN and (0, 0, 1) off the casts)"""
    Fl, Vl = low_faces.shape[0], low_verts.shape[0]
    S, _ = TX.layout(Fl, R)
    owner, i, j = TX.texel_cells(Fl, R)
    tri = low_faces.long()[owner.clamp_min(0)]
    cast = (owner >= 0) & ((tri >= 0) & (tri < Vl)).all(1)
    tri = torch.where(cast[:, None], tri, torch.zeros_like(tri))
    L = torch.tensor(float(S - 3), dtype=dtype)
    b1 = (i.to(dtype) / L).clamp(0, 1)
    b2 = torch.minimum((j.to(dtype) / L).clamp_min(0), 1 - b1)
    b0 = 1 - b1 - b2
    mix = lambda a: b0[:, None] * a[tri[:, 0]] + b1[:, None] * a[tri[:, 1]] + b2[:, None] * a[tri[:, 2]]  # noqa: E731
    P, n = mix(low_verts.to(dtype)), B.unit(mix(low_normals.to(dtype)))
    z = torch.zeros_like(n)
    z[:, 2] = 1
    return owner, cast, torch.where(cast[:, None], P, torch.full_like(P, float("nan"))), torch.where(cast[:, None], n, z)


@torch.no_grad()
def bake_ao(low_verts, low_faces, low_normals, high_verts, high_faces, high_normals, R, max_dist, K, radius, bias, seed=0, dtype=F64):
    """dict(owner, cast, keep (mesh_bake_ref.bake's: the texels whose normal-bake decisions hold its margins), sure, marginal, hits [R*R]
    (-1 where nothing is cast), points, normals [R*R, 3]: where every texel's hemisphere stands)"""
    b = B.bake(low_verts, low_faces, low_normals, high_verts, high_faces, high_normals, R, max_dist, dtype)
    owner, cast, P, n = texel_frames(low_verts, low_faces, low_normals, R, dtype)
    hit = ~torch.isnan(b["dist"])
    pts = torch.where(hit[:, None], P + torch.where(hit, b["dist"], torch.zeros_like(b["dist"]))[:, None] * n, P)
    nrm = torch.where(hit[:, None], b["normal"], n)
    o = occlusion(high_verts, high_faces, pts.float() if dtype == F32 else pts, nrm, K, radius, bias, seed, dtype)
    return dict(owner=owner, cast=cast, keep=b["keep"], sure=o["sure"], marginal=o["marginal"], hits=o["hits"], points=pts, normals=nrm, dist=b["dist"])


# ---- scenes -----------------------------------------------------------------------------------------------------------------------------------
AO_AMPLITUDE = 0.1                   # mesh_bake_ref.bake_scene's 0.03 occludes 0.26 % of the rays: too shallow to test AO
AO_BIAS = 1e-3
POINT_COUNTS = (1, 63, 64, 65, 1100)
OCC_COUNTS = (1, 63, 65, 700)
OCC_CASES = (("pair", 64, 0.5), ("pair", 65, 0.1), ("pair", 1, 0.5), ("pair", 16, 0.5), ("pair", 200, 0.3), ("bumped", 64, 0.25))
OCC_SMALL = 130                      # points of every case but the first, which runs OCC_COUNTS


def occ_mesh(name):
    if name == "bumped":
        v, f = M.icosphere(3, 0.5, (0.0, 0.0, 0.0), seed=1)
        return B.bumped(v, amplitude=AO_AMPLITUDE), f
    return M.mesh_scene(name, 1)[:2]


def face_normals(verts, faces):
    v, f = verts.double(), faces.long()
    return B.unit(_cross(v[f[:, 1]] - v[f[:, 0]], v[f[:, 2]] - v[f[:, 0]])).float()


@functools.lru_cache(maxsize=None)
def occ_points(name):
    """(points, normals) float32: the samples of the scene's own faces (face_samples at n = 2) with their face normals, shuffled once"""
    v, f = occ_mesh(name)
    pts, _, _ = face_samples(v, f, 2)
    perm = torch.randperm(4 * f.shape[0], generator=torch.Generator().manual_seed(11))
    return pts.float()[perm].contiguous(), face_normals(v, f).repeat_interleave(4, 0)[perm].contiguous()


@functools.lru_cache(maxsize=None)
def occ_case(name, K, radius, count):
    """The restatement of the first `count` points of a case, computed once"""
    v, f = occ_mesh(name)
    p, n = occ_points(name)
    return occlusion(v, f, p[:count], n[:count], K, radius, AO_BIAS)


EXTRA_OCC_CASES = ("seed", "invalid", "bias0")
EXTRA_SEED = 12345


def extra_occ_inputs(name):
    """(points, normals, K, radius, bias, seed) of the further occlusion runs on the pair: another seed on the first 65 points; 70 points of
    which five are not valid (a NaN and an infinite coordinate, a zero, a tiny and an infinite normal) and one has a long normal; the valid
    ones of those lifted 0.01 off the surface, with bias 0"""
    p, n = occ_points("pair")
    if name == "seed":
        return p[:65], n[:65], 64, 0.5, AO_BIAS, EXTRA_SEED
    p, n = p[:70].clone(), n[:70].clone()
    p[3, 1] = float("nan")
    p[10, 0] = INF
    n[20] = 0.0
    n[30] = torch.tensor([1e-11, 0.0, 0.0])
    n[40] = torch.tensor([INF, 0.0, 0.0])
    n[50] *= 7.5                                       # a normal is used by its direction
    if name == "invalid":
        return p, n, 64, 0.5, AO_BIAS, 0
    ok = valid_points(p, n)
    return (p + 0.01 * torch.nn.functional.normalize(n.nan_to_num(0.0, 0.0, 0.0), dim=1))[ok], n[ok], 64, 0.5, 0.0, 0


@functools.lru_cache(maxsize=None)
def extra_occ_case(name):
    """(the restatement, K) of a further occlusion run, computed once"""
    p, n, K, radius, bias, seed = extra_occ_inputs(name)
    return occlusion(*occ_mesh("pair"), p, n, K, radius, bias, seed), K


@functools.lru_cache(maxsize=None)
def queries(kind, seed=4):
    """[1100, 3] float32 query points for the sphere and pair scenes (inside the ball of radius 0.6): 500 in the ball of radius 0.45 (inside
    the meshes), 400 in the shell 0.55 .. 0.9 (outside), 100 far away, beyond the root box on every side (|x|, |y|, |z| all > 5), and 100 exactly at
    vertices; shuffled, so a prefix holds every kind"""
    v, _ = M.mesh_scene(kind, 1)[:2]
    g = torch.Generator().manual_seed(seed)
    sph = lambda n: torch.nn.functional.normalize(torch.randn(n, 3, generator=g, dtype=F64), dim=1)  # noqa: E731
    rnd = lambda *s: torch.rand(*s, generator=g, dtype=F64)  # noqa: E731
    inside = sph(500) * 0.45 * rnd(500, 1) ** (1 / 3)
    outside = sph(400) * (0.55 + 0.35 * rnd(400, 1))
    far = (5.0 + 5.0 * rnd(100, 3)) * torch.where(rnd(100, 3) < 0.5, -1.0, 1.0)
    at = v[torch.randint(v.shape[0], (100,), generator=g)].double()
    perm = torch.randperm(1100, generator=g)
    return torch.cat([inside, outside, far, at])[perm].float().contiguous()


@functools.lru_cache(maxsize=None)
def point_case(kind):
    """(verts, faces, points, fp64 restatement, fp32 restatement) of all 1100 queries, computed once"""
    v, f = M.mesh_scene(kind, 1)[:2]
    p = queries(kind)
    return v, f, p, closest_point(v, f, p), closest_point(v, f, p, dtype=F32)


def exact_triangle():
    """A triangle and seven queries on small power-of-two coordinates: every operation of the region method is exact in float32, and the
    queries take regions 0 .. 6 in this order.  (verts, faces, points, distances)"""
    v = torch.tensor([[0.0, 0.0, 0.0], [4.0, 0.0, 0.0], [0.0, 4.0, 0.0]])
    p = torch.tensor([[-1.0, -1.0, 0.0], [6.0, -1.0, 0.0], [2.0, -2.0, 0.0], [-1.0, 6.0, 0.0], [-2.0, 2.0, 0.0], [4.0, 4.0, 0.0], [1.0, 1.0, 2.0]])
    d = torch.tensor([math.sqrt(2.0), math.sqrt(5.0), 2.0, math.sqrt(5.0), 2.0, math.sqrt(8.0), 2.0], dtype=F64)
    return v, torch.tensor([[0, 1, 2]]), p, d


@functools.lru_cache(maxsize=None)
def ao_scene():
    """mesh_bake_ref.bake_scene("nested") with the bump at AO_AMPLITUDE: (low_verts, low_faces, high_verts, high_faces, max_dist, radius)"""
    lv, lf = M.icosphere(2, 0.5, (0.0, 0.0, 0.0), seed=2)
    hv, hf = M.icosphere(3, 0.5, (0.0, 0.0, 0.0), seed=1)
    return lv, lf, B.bumped(hv, amplitude=AO_AMPLITUDE), hf, 0.3, 0.25


def bump_sign(points, amplitude=AO_AMPLITUDE, seed=5):
    """the radial term of mesh_bake_ref.bumped at the directions of `points`: negative in a dimple, positive on a bump"""
    u = torch.nn.functional.normalize(points.double(), dim=1)
    return torch.sin(7.0 * u[:, 0] + seed) * torch.sin(5.0 * u[:, 1]) + 0.6 * torch.sin(9.0 * u[:, 2])


def distance_pair():
    """the 320-face icosphere against the bumped 1280-face one, rotated differently (seeds 2 and 1)"""
    lv, lf, hv, hf, _ = B.bake_scene("nested")
    return lv, lf, hv, hf


def quad(size, z=0.0):
    """a square of side 2 size in the plane at height z, two triangles"""
    v = torch.tensor([[-size, -size, z], [size, -size, z], [size, size, z], [-size, size, z]])
    return v, torch.tensor([[0, 1, 2], [0, 2, 3]])


def cube(side=1.0):
    """a closed cube around the origin, 12 triangles"""
    h = side / 2
    v = torch.tensor([[x, y, z] for x in (-h, h) for y in (-h, h) for z in (-h, h)])
    f = torch.tensor([[0, 1, 3], [0, 3, 2], [4, 6, 7], [4, 7, 5], [0, 4, 5], [0, 5, 1], [2, 3, 7], [2, 7, 6], [0, 2, 6], [0, 6, 4], [1, 5, 7], [1, 7, 3]])
    return v, f
