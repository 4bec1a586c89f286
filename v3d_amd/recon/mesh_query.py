"""Queries on the BVH of mesh_bake.py, on the gfx950 kernels of libv3d_recon.so (csrc_recon/meshquery.hip, include/v3d_recon.h "Mesh
queries"): the closest point of a mesh, with it a two-sided distance between two meshes, and ambient occlusion baked onto the atlas of
mesh_texture.py.

    bvh = mesh_bake.build_bvh(verts, faces)
    dist, face, uv = closest_points(bvh, points, max_dist=inf)
    points, weights = face_samples(verts, faces, subdivide=2)
    d = mesh_distance(a_verts, a_faces, b_verts, b_faces)         # mean, rms, max both ways, hausdorff, chamfer, the same over B's diagonal
    hits = occlusion(bvh, points, normals, samples=64, radius=0.1, bias=1e-4)
    ao_map, stats = bake_ambient_occlusion(low_verts, low_faces, high_verts, high_faces, tex_size=1024, samples=64)
    save_textured_obj("mesh.obj", low_verts, low_faces, vt, texture, ao_map=ao_map)                # + mesh_ao.png, `map_Ka` in the MTL

No atomics anywhere: two calls with the same arguments return bit-equal results.  Everything runs under no_grad.  There is no fallback:
without the libraries this raises."""
from __future__ import annotations

import math
import operator
import time
from typing import Optional

import numpy as np
import torch

from .geometry import _check, _stream, load_library
from .mesh_bake import MeshBVH, _tex_arg, _vertex_normals, bake_texels, build_bvh, default_max_dist
from .mesh_clean import _mesh_arg
from .mesh_render import _dev
from .mesh_texture import atlas_layout

MAX_SUBDIVIDE = 16
MAX_SAMPLES = 1024
DEFAULT_AO_RADIUS = 0.1            # x the diagonal of the high mesh's bounding box: a choice, not a measurement
DEFAULT_AO_BIAS = 1e-4             # x the same diagonal: a choice, not a measurement


def _points_arg(points, dev, who: str, name: str = "points"):
    p = _dev(points, torch.float32, dev)
    if p.dim() != 2 or p.shape[1] != 3:
        raise ValueError(f"{who}: {name} must be [N, 3], got {tuple(p.shape)}")
    if p.shape[0] > 2 ** 31 - 1:
        raise ValueError(f"{who}: {p.shape[0]} {name} do not fit int32")
    return p


def _int_arg(value, lo: int, hi: int, who: str, name: str) -> int:
    try:
        i = None if isinstance(value, (bool, np.bool_)) else operator.index(value)         # Python and numpy integers; not 2.5, not True
    except TypeError:
        i = None
    if i is None or not lo <= i <= hi:
        raise ValueError(f"{who}: {name} {value!r} is not an integer in {lo} .. {hi}")
    return i


@torch.no_grad()
def closest_points(bvh: MeshBVH, points, max_dist: float = math.inf):
    """(dist [N] float32, face [N] int32, uv [N, 2] float32) of the point of the tree's mesh closest to every points[i], no further than
    max_dist (closed; +inf allowed), on the tree's device: verts[f0] + u (verts[f1] - verts[f0]) + v (verts[f2] - verts[f0]).  On equal
    distances the smaller face.  A miss, also a point with a coordinate that is not finite: +inf, -1, 0 0."""
    md = float(max_dist)
    if math.isnan(md) or md < 0:
        raise ValueError(f"closest_points: max_dist {max_dist} must not be negative or NaN")
    dev = bvh.verts.device
    p = _points_arg(points, dev, "closest_points")
    N = p.shape[0]
    dist = torch.empty(N, dtype=torch.float32, device=dev)
    face = torch.empty(N, dtype=torch.int32, device=dev)
    uv = torch.empty(N, 2, dtype=torch.float32, device=dev)
    if N == 0:
        return dist, face, uv
    lib = load_library()
    _check(lib, lib.v3d_recon_bvh_closest_point(p.data_ptr(), N, md, *bvh._args(), dist.data_ptr(), face.data_ptr(), uv.data_ptr(), _stream()),
           "v3d_recon_bvh_closest_point")
    return dist, face, uv


@torch.no_grad()
def _face_samples(v: torch.Tensor, f: torch.Tensor, n: int):
    """on validated device tensors (V >= 1, F >= 1)"""
    lib = load_library()
    F = f.shape[0]
    pts = torch.empty(F * n * n, 3, dtype=torch.float32, device=v.device)
    w = torch.empty(F * n * n, dtype=torch.float32, device=v.device)
    _check(lib, lib.v3d_recon_mesh_face_samples(v.data_ptr(), v.shape[0], f.data_ptr(), F, n, pts.data_ptr(), w.data_ptr(), _stream()),
           "v3d_recon_mesh_face_samples")
    return pts, w


@torch.no_grad()
def face_samples(verts, faces, subdivide: int = 2, device="cuda"):
    """(points [F n^2, 3], weights [F n^2]) float32: the centroids and areas of the n^2 congruent sub-triangles of every face, n = subdivide in
    1 .. 16, in the order of include/v3d_recon.h.  The weights sum to the mesh's area.  No faces: empty tensors without a launch."""
    n = _int_arg(subdivide, 1, MAX_SUBDIVIDE, "face_samples", "subdivide")
    v, f, _ = _mesh_arg(verts, faces, None, device, "face_samples")
    if f.shape[0] * n * n > 2 ** 31 - 1:
        raise ValueError(f"face_samples: {f.shape[0]} faces x {n * n} samples do not fit int32")
    if f.shape[0] == 0 or v.shape[0] == 0:
        return torch.empty(0, 3, dtype=torch.float32, device=device), torch.empty(0, dtype=torch.float32, device=device)
    return _face_samples(v, f, n)


def _one_way(v, f, n: int, bvh: MeshBVH) -> dict:
    """The samples of (v, f) and its vertices (weight 0: they count for the maximum only) against the tree"""
    pts, w = _face_samples(v, f, n)
    dist, _, _ = closest_points(bvh, torch.cat([pts, v]))
    d, w64 = dist.double(), w.double()
    ds = d[:pts.shape[0]]
    area = float(w64.sum())
    mean = float((ds * w64).sum()) / area if area > 0 else float("nan")
    rms = math.sqrt(float((ds * ds * w64).sum()) / area) if area > 0 else float("nan")
    return {"mean": mean, "rms": rms, "max": float(dist.max()), "area": area, "samples": int(dist.shape[0])}


@torch.no_grad()
def mesh_distance(a_verts, a_faces, b_verts, b_faces, subdivide: int = 2, device="cuda") -> dict:
    """How far mesh A is from mesh B and B from A.  Per direction ("a_to_b": the samples of A, face_samples at `subdivide`, and A's vertices
    against the closest point of B) "mean" and "rms", area-weighted and summed in float64, and "max";  "hausdorff": the larger maximum;
    "chamfer": the mean of the two means;  "diagonal": of B's bounding box, and every figure again divided by it under "relative";
    "samples": points queried both ways;  "seconds".  A mesh without faces on either side raises ValueError."""
    n = _int_arg(subdivide, 1, MAX_SUBDIVIDE, "mesh_distance", "subdivide")
    av, af, _ = _mesh_arg(a_verts, a_faces, None, device, "mesh_distance")
    bv, bf, _ = _mesh_arg(b_verts, b_faces, None, device, "mesh_distance")
    for name, v, f in (("the mesh", av, af), ("the reference", bv, bf)):
        if v.shape[0] == 0 or f.shape[0] == 0:
            raise ValueError(f"mesh_distance: {name} has {v.shape[0]} vertices and {f.shape[0]} faces: nothing to measure")
        if f.shape[0] * n * n > 2 ** 31 - 1:
            raise ValueError(f"mesh_distance: {f.shape[0]} faces x {n * n} samples do not fit int32")
    t0 = time.perf_counter()
    ab = _one_way(av, af, n, build_bvh(bv, bf, device))
    ba = _one_way(bv, bf, n, build_bvh(av, af, device))
    diag = float((bv.max(0).values - bv.min(0).values).double().norm())
    out = {"a_to_b": {k: ab[k] for k in ("mean", "rms", "max")}, "b_to_a": {k: ba[k] for k in ("mean", "rms", "max")},
           "hausdorff": max(ab["max"], ba["max"]), "chamfer": 0.5 * (ab["mean"] + ba["mean"]), "diagonal": diag, "subdivide": n,
           "samples": ab["samples"] + ba["samples"], "area_a": ab["area"], "area_b": ba["area"]}
    rel = (lambda x: x / diag) if diag > 0 else (lambda x: float("nan"))
    out["relative"] = {"a_to_b": {k: rel(x) for k, x in out["a_to_b"].items()}, "b_to_a": {k: rel(x) for k, x in out["b_to_a"].items()},
                       "hausdorff": rel(out["hausdorff"]), "chamfer": rel(out["chamfer"])}
    if device != "cpu" and torch.cuda.is_available():
        torch.cuda.synchronize()
    out["seconds"] = time.perf_counter() - t0
    return out


def _ao_args(samples, radius, bias, seed, who: str):
    K = _int_arg(samples, 1, MAX_SAMPLES, who, "samples")
    r, b = float(radius), float(bias)
    if not (math.isfinite(r) and r > 0):
        raise ValueError(f"{who}: radius {radius} must be finite and positive")
    if not (math.isfinite(b) and b >= 0):
        raise ValueError(f"{who}: bias {bias} must be finite and not negative")
    s = _int_arg(seed, 0, 2 ** 32 - 1, who, "seed")
    return K, r, b, s


@torch.no_grad()
def occlusion(bvh: MeshBVH, points, normals, samples: int = 64, radius: float = 0.1, bias: float = 1e-4, seed: int = 0):
    """hits [N] int32 on the tree's device: of `samples` (1 .. 1024) cosine-weighted directions over the hemisphere of normals[i], how many
    meet the tree's mesh between points[i] + bias n and `radius` further on; the occlusion is hits / samples.  -1 for a point that is not
    finite or a normal without length.  The directions depend on i, samples and seed only (include/v3d_recon.h)."""
    K, r, b, s = _ao_args(samples, radius, bias, seed, "occlusion")
    dev = bvh.verts.device
    p, n = _points_arg(points, dev, "occlusion"), _points_arg(normals, dev, "occlusion", "normals")
    if p.shape != n.shape:
        raise ValueError(f"occlusion: {p.shape[0]} points, {n.shape[0]} normals")
    N = p.shape[0]
    hits = torch.empty(N, dtype=torch.int32, device=dev)
    if N == 0:
        return hits
    lib = load_library()
    _check(lib, lib.v3d_recon_bvh_occlusion(p.data_ptr(), n.data_ptr(), N, K, r, b, s, *bvh._args(), hits.data_ptr(), _stream()), "v3d_recon_bvh_occlusion")
    return hits


@torch.no_grad()
def texel_frames(verts, faces, normals, tex_size: int):
    """The kernel's three outputs on validated device tensors (V, F >= 1): owner [R*R] int32, P [R*R, 3] (NaN where the texel has no face),
    n [R*R, 3]: the position and unit normal every texel of the atlas stands for"""
    lib = load_library()
    R, dev = int(tex_size), verts.device
    owner = torch.empty(R * R, dtype=torch.int32, device=dev)
    P = torch.empty(R * R, 3, dtype=torch.float32, device=dev)
    n = torch.empty(R * R, 3, dtype=torch.float32, device=dev)
    _check(lib, lib.v3d_recon_tex_texel_frames(verts.data_ptr(), verts.shape[0], faces.data_ptr(), faces.shape[0], normals.data_ptr(), R, owner.data_ptr(),
                                               P.data_ptr(), n.data_ptr(), _stream()), "v3d_recon_tex_texel_frames")
    return owner, P, n


def ao_points(P, n, dist, nmap):
    """Where a texel's hemisphere stands: on the high mesh, P + dist n with the baked normal, where the normal bake hit; else P with n"""
    hit = ~torch.isnan(dist)
    pts = torch.where(hit[:, None], P + torch.where(hit, dist, torch.zeros_like(dist))[:, None] * n, P)
    return pts, torch.where(hit[:, None], nmap, n)


@torch.no_grad()
def bake_ambient_occlusion(low_verts, low_faces, high_verts, high_faces, tex_size: int = 1024, samples: int = 64, radius: Optional[float] = None,
                           bias: Optional[float] = None, max_dist: Optional[float] = None, seed: int = 0, device="cuda"):
    """(ao_map [R*R] float32 on `device`, stats).  Every owned texel of the low mesh's atlas finds its point of the high mesh as
    bake_normal_map does (max_dist as there), and casts `samples` cosine-weighted rays of length `radius` (default 0.1 x the diagonal of the
    high mesh's bounding box) from there, lifted by `bias` (default 1e-4 x the diagonal), against the high mesh: ao = 1 - hits / samples,
    1.0 on unowned texels.  stats: "owned", "mean_ao", "min_ao" (over the owned texels), "fully_open" (owned texels with ao 1), "samples",
    "radius", "bias", "max_dist", "rays", "bvh_rounds", "tex_size", "seconds".  A low mesh with V = 0 or F = 0 gives an all-1 map without a
    launch."""
    R = _tex_arg(tex_size, "bake_ambient_occlusion")
    lv, lf, _ = _mesh_arg(low_verts, low_faces, None, device, "bake_ambient_occlusion")
    hv, hf, _ = _mesh_arg(high_verts, high_faces, None, device, "bake_ambient_occlusion")
    diag = float((hv.max(0).values - hv.min(0).values).norm()) if hv.shape[0] else 0.0
    md = default_max_dist(hv) if max_dist is None else float(max_dist)
    if not (math.isfinite(md) and md >= 0):
        raise ValueError(f"bake_ambient_occlusion: max_dist {max_dist} must be finite and not negative")
    empty = lv.shape[0] == 0 or lf.shape[0] == 0
    if not empty and (hv.shape[0] == 0 or hf.shape[0] == 0):
        raise ValueError("bake_ambient_occlusion: the high mesh has no faces to hit")
    if empty and radius is None:                   # (nothing is cast; the high mesh may be empty too and have no diagonal)
        radius = 1.0
    K, r, b, s = _ao_args(samples, DEFAULT_AO_RADIUS * diag if radius is None else radius, DEFAULT_AO_BIAS * diag if bias is None else bias, seed,
                          "bake_ambient_occlusion")
    stats = {"owned": 0, "mean_ao": float("nan"), "min_ao": float("nan"), "fully_open": 0, "samples": K, "radius": r, "bias": b, "max_dist": md, "rays": 0,
             "bvh_rounds": 0, "tex_size": R, "seconds": 0.0}
    if empty:
        return torch.ones(R * R, dtype=torch.float32, device=device), stats
    atlas_layout(lf.shape[0], R)
    t0 = time.perf_counter()
    bvh = build_bvh(hv, hf, device)
    ln = _vertex_normals(lv, lf)
    owner, P, n = texel_frames(lv, lf, ln, R)
    _, nmap, dist, _ = bake_texels(lv, lf, ln, bvh, _vertex_normals(hv, hf), R, md)
    pts, nrm = ao_points(P, n, dist, nmap)
    hits = occlusion(bvh, pts, nrm, K, r, b, s)
    cast = hits >= 0
    ao = torch.where(cast, 1.0 - hits.float() / float(K), torch.ones_like(dist))
    owned = owner >= 0
    stats.update(owned=int(owned.sum()), rays=K * int(cast.sum()), bvh_rounds=bvh.rounds)
    if stats["owned"]:
        a = ao[owned]
        stats.update(mean_ao=float(a.double().mean()), min_ao=float(a.min()), fully_open=int((a == 1.0).sum()))
    if device != "cpu" and torch.cuda.is_available():
        torch.cuda.synchronize()
    stats["seconds"] = time.perf_counter() - t0
    return ao, stats


# ---- looking at it --------------------------------------------------------------------------------------------------------------------------
@torch.no_grad()
def render_ao_orbit(verts, faces, ao_map, n: int, radius: float, elevation: float, fov: float, reso: int, white_background: bool = True,
                    cull: bool = True, device="cuda"):
    """n turntable frames of the low mesh with its AO map as a grey texture (prepare_texture_view, texture_shade_forward), uint8
    [n, reso, reso, 3] on the host"""
    from .cameras import orbit_cameras
    from .mesh_render import _bg, _check_view
    from .mesh_texture import prepare_texture_view, texture_shade_forward
    cams, _ = orbit_cameras(n, radius, elevation, fov, reso)
    _check_view(int(reso), int(reso), 8)
    v, f, _ = _mesh_arg(verts, faces, None, device, "render_ao_orbit")
    m = _dev(ao_map, torch.float32, device).reshape(-1)
    R = math.isqrt(m.shape[0])
    if R * R != m.shape[0] or R == 0:
        raise ValueError(f"render_ao_orbit: {m.shape[0]} texels are not a square")
    grey = m[:, None].expand(-1, 3).contiguous()
    out = []
    for cam in cams:
        view = prepare_texture_view(cam, v, f, R, _bg(white_background), cull=cull, lists=False, device=device)
        img = texture_shade_forward(view, grey).reshape(3, view.height, view.width)
        out.append((img.clamp(0, 1) * 255).to(torch.uint8).permute(1, 2, 0).cpu())
    return torch.stack(out).numpy() if out else np.zeros((0, int(reso), int(reso), 3), dtype=np.uint8)
