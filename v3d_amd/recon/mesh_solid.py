"""Inside and outside of a mesh, open or closed, on the gfx950 kernels of libv3d_recon.so (csrc_recon/meshsolid.hip, include/v3d_recon.h
"Mesh solid"): the generalized winding number on the BVH of mesh_bake.py, with it a signed distance, a TSDF volume filled from a mesh, and
through the surface nets of geometry.extract_mesh a closed mesh from an open one.

    bvh = mesh_bake.build_bvh(verts, faces)
    mom = node_moments(bvh)                                       # [2F-1, 8]: one dipole per node
    w = winding_numbers(bvh, points, beta=2.0, moments=mom)       # 1 inside, 0 outside, in between near a hole;  beta=0: the exact sum
    sd = signed_distances(bvh, points)                            # dist (negative inside), face, uv, w
    vol = mesh_to_volume(verts, faces, colors, resolution=256)    # a geometry.TsdfVolume
    v, f, c, stats = solidify_mesh(verts, faces, colors, resolution=256, smooth=0)

ORIENTATION MATTERS.  A triangle must be wound so that (v1 - v0) x (v2 - v0) points outward, as extract_mesh winds its own: then w = 1
inside.  A mesh wound inward has w = -1 inside, no voxel counts as inside and it solidifies to NOTHING (an empty mesh);  `flip=True`
reverses every face first.  No atomics anywhere: two calls with the same arguments return bit-equal results.  Everything runs under
no_grad.  There is no fallback: without the libraries this raises."""
from __future__ import annotations

import math
import time
from typing import Optional

import numpy as np
import torch

from .geometry import MAX_RESOLUTION  # noqa: F401  (the limit of `resolution`, for callers)
from .geometry import TsdfVolume, _check, _check_resolution, _stream, extract_mesh, load_library
from .mesh_bake import ROUND_GROUP, MeshBVH, _high_mesh, build_bvh, height_bound
from .mesh_clean import _count_arg, _mesh_arg, _rows_arg, boundary_vertices, taubin_smooth
from .mesh_query import _points_arg, closest_points, mesh_distance

DEFAULT_BETA = 2.0                 # a node is a dipole from beta x its radius on: a choice (DESIGN 3.18 has the measured error at 2 and 3)
DEFAULT_TRUNC_VOXELS = 4.0         # as geometry.new_volume


def _beta_arg(beta, who: str) -> float:
    b = float(beta)
    if not (math.isfinite(b) and b >= 0):
        raise ValueError(f"{who}: beta {beta} must be finite and not negative")
    return b


def _moments(bvh: MeshBVH):
    """(mom [2F-1, 8], rounds): the rounds of v3d_recon_bvh_moment_round, in groups with a flag word each as mesh_bake._fit runs the fit;
    rounds counts up to and including the first that changed nothing (1 when F = 1: the lone leaf, nothing further)"""
    lib = load_library()
    F, dev = bvh.num_faces, bvh.verts.device
    mom = torch.zeros(2 * F - 1, 8, dtype=torch.float32, device=dev)
    cur = torch.zeros(2 * F - 1, dtype=torch.int32, device=dev)
    nxt = torch.empty_like(cur)
    flags = torch.empty(ROUND_GROUP, dtype=torch.int32, device=dev)

    def one(j):
        nonlocal cur, nxt
        _check(lib, lib.v3d_recon_bvh_moment_round(*bvh._args(), cur.data_ptr(), nxt.data_ptr(), mom.data_ptr(), flags.data_ptr() + 4 * j, _stream()),
               "v3d_recon_bvh_moment_round")
        cur, nxt = nxt, cur

    if F == 1:
        one(0)
        return mom, 1
    done, limit = 0, height_bound(F) + 8
    while done < limit:
        group = min(ROUND_GROUP, limit - done)
        flags.zero_()
        for j in range(group):
            one(j)
        changed = flags.cpu().tolist()[:group]
        if 0 in changed:
            if not bool(cur.all()):
                raise RuntimeError(f"node_moments: the rounds stopped with nodes left open on {F} faces: the tree is broken")
            return mom, done + changed.index(0) + 1
        done += group
    raise RuntimeError(f"node_moments: no fixed point after {limit} rounds on {F} faces: the tree is broken")


@torch.no_grad()
def node_moments(bvh: MeshBVH) -> torch.Tensor:
    """mom [2F-1, 8] float32 on the tree's device: (nx, ny, nz, r2, cx, cy, cz, area) per node, THE MOMENTS of include/v3d_recon.h"""
    return _moments(bvh)[0]


def _moments_arg(bvh: MeshBVH, moments, who: str) -> torch.Tensor:
    if moments is None:
        return _moments(bvh)[0]
    m = moments
    if not torch.is_tensor(m) or m.dtype != torch.float32 or tuple(m.shape) != (2 * bvh.num_faces - 1, 8) or m.device != bvh.verts.device:
        raise ValueError(f"{who}: moments must be the float32 [{2 * bvh.num_faces - 1}, 8] tensor of node_moments on the tree's device")
    return m.contiguous()


@torch.no_grad()
def winding_numbers(bvh: MeshBVH, points, beta: float = DEFAULT_BETA, moments: Optional[torch.Tensor] = None) -> torch.Tensor:
    """w [N] float32 on the tree's device: the generalized winding number of the tree's mesh at every points[i].  beta = 0 sums every
    triangle's solid angle;  beta > 0 takes a node further away than beta x its radius as one dipole (THE SUM).  NaN for a point with a
    coordinate that is not finite.  moments: node_moments(bvh), computed here when None."""
    b = _beta_arg(beta, "winding_numbers")
    dev = bvh.verts.device
    p = _points_arg(points, dev, "winding_numbers")
    N = p.shape[0]
    w = torch.empty(N, dtype=torch.float32, device=dev)
    if N == 0:
        return w
    mom = _moments_arg(bvh, moments, "winding_numbers")
    lib = load_library()
    _check(lib, lib.v3d_recon_bvh_winding(p.data_ptr(), N, b, *bvh._args(), mom.data_ptr(), w.data_ptr(), _stream()), "v3d_recon_bvh_winding")
    return w


@torch.no_grad()
def signed_distances(bvh: MeshBVH, points, beta: float = DEFAULT_BETA, max_dist: float = math.inf, moments: Optional[torch.Tensor] = None) -> dict:
    """{"dist", "face", "uv": mesh_query.closest_points with `dist` negated where w >= 0.5 (a miss: -inf inside, +inf outside), "w":
    winding_numbers}"""
    b = _beta_arg(beta, "signed_distances")
    dist, face, uv = closest_points(bvh, points, max_dist)
    w = winding_numbers(bvh, points, b, moments)
    return {"dist": torch.where(w >= 0.5, -dist, dist), "face": face, "uv": uv, "w": w}


def voxel_axis(resolution: int, bound: float, device="cuda") -> torch.Tensor:
    """[N] float32: the voxel centres along one axis, the very floats v3d_recon_sdf_grid forms, fmaf(i + 0.5, voxel, -bound) with
    voxel = 2 bound / N in float.  Formed in double, where the product and the sum are exact, and rounded to float once."""
    N = int(resolution)
    b = torch.tensor(float(bound), dtype=torch.float32)
    voxel = 2.0 * b / torch.tensor(float(N), dtype=torch.float32)
    return ((torch.arange(N, dtype=torch.float64) + 0.5) * voxel.double() - b.double()).float().to(device)


def voxel_centres(resolution: int, bound: float, device="cuda", layers=None) -> torch.Tensor:
    """[N^3, 3] float32 in linear voxel order (iz N + iy) N + ix, every coordinate from voxel_axis.  layers = (z0, z1): only the voxels of
    the z layers z0 .. z1-1, [(z1 - z0) N^2, 3], the same floats in the same order."""
    c = voxel_axis(resolution, bound, device)
    zz, yy, xx = torch.meshgrid(c if layers is None else c[layers[0]:layers[1]], c, c, indexing="ij")
    return torch.stack([xx, yy, zz], -1).reshape(-1, 3).contiguous()


def default_volume(verts, resolution: int, bound: Optional[float] = None, trunc: Optional[float] = None):
    """(bound, trunc).  trunc None: 4 voxels, as geometry.new_volume.  bound None: 1.1 x the largest |coordinate| plus trunc, so that the
    band around the surface lies inside the volume (with trunc None too: plus 4 voxels of the volume of half-extent 1.1 x).  Choices, like
    mesh_bake.DEFAULT_MAX_DIST."""
    N = int(resolution)
    if bound is None:
        m = 1.1 * float(verts.abs().max()) if verts.numel() else 1.0
        m = m if m > 0 else 1.0
        bound = m + (DEFAULT_TRUNC_VOXELS * 2.0 * m / N if trunc is None else float(trunc))
    bound = float(bound)
    trunc = DEFAULT_TRUNC_VOXELS * 2.0 * bound / N if trunc is None else float(trunc)
    return bound, trunc


def _volume_args(resolution, bound, trunc, beta, who: str):
    _check_resolution(resolution)
    for name, x in (("bound", bound), ("trunc", trunc)):
        if x is not None and not (math.isfinite(float(x)) and float(x) > 0):
            raise ValueError(f"{who}: {name} {x} must be finite and positive")
    return int(resolution), _beta_arg(beta, who)


def _fill(bvh: MeshBVH, mom, colors, N: int, bound: float, trunc: float, beta: float) -> TsdfVolume:
    lib = load_library()
    dev = bvh.verts.device
    e = lambda *s: torch.empty(*s, dtype=torch.float32, device=dev)  # noqa: E731
    vol = TsdfVolume(N, bound, trunc, e(N, N, N), e(N, N, N), e(3, N, N, N), e(N, N, N))
    _check(lib, lib.v3d_recon_sdf_grid(*bvh._args(), mom.data_ptr(), colors.data_ptr() if colors is not None else None, N, bound, trunc, beta,
                                       vol.tsdf_sum.data_ptr(), vol.weight.data_ptr(), vol.rgb_sum.data_ptr(), vol.rgb_weight.data_ptr(), _stream()),
           "v3d_recon_sdf_grid")
    return vol


def _mesh_to_volume(verts, faces, colors, resolution, bound, trunc, beta, device, who: str):
    """(volume, bvh, moment rounds)"""
    N, b = _volume_args(resolution, bound, trunc, beta, who)
    v, f = _high_mesh(verts, faces, device, who)
    c = None
    if colors is not None:
        c = _rows_arg(colors, device, who, "colors")
        if c.shape != v.shape:
            raise ValueError(f"{who}: {v.shape[0]} vertices, {c.shape[0]} colours")
    bound, trunc = default_volume(v, N, bound, trunc)
    bvh = build_bvh(v, f, device)
    mom, rounds = _moments(bvh)
    return _fill(bvh, mom, c, N, bound, trunc, b), bvh, rounds


@torch.no_grad()
def mesh_to_volume(verts, faces, colors=None, resolution: int = 256, bound: Optional[float] = None, trunc: Optional[float] = None,
                   beta: float = DEFAULT_BETA, device="cuda") -> TsdfVolume:
    """A geometry.TsdfVolume filled from a mesh in one launch: per voxel the distance to the closest point over trunc, capped at 1, negative
    where the winding number is at least 0.5;  weight 1 everywhere (every voxel is observed: extract_mesh leaves nothing open);  the closest
    face's interpolated vertex colours where the surface is within trunc.  bound, trunc: default_volume.  The faces must be wound outward
    (the module's head).  A mesh with no faces raises ValueError before any launch."""
    return _mesh_to_volume(verts, faces, colors, resolution, bound, trunc, beta, device, "mesh_to_volume")[0]


def edge_counts(faces: torch.Tensor, num_verts: int):
    """(undirected edges, of them used by exactly one face) of faces [F, 3], counted in torch"""
    if faces.shape[0] == 0:
        return 0, 0
    f = faces.long()
    e = torch.cat([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]])
    key = e.min(1).values * int(num_verts) + e.max(1).values
    _, n = torch.unique(key, return_counts=True)
    return int(n.numel()), int((n == 1).sum())


def signed_volume(verts: torch.Tensor, faces: torch.Tensor) -> float:
    """sum of v0 . (v1 x v2) / 6 in float64: the enclosed volume of a closed mesh wound outward"""
    if faces.shape[0] == 0:
        return 0.0
    v, f = verts.double(), faces.long()
    return float((v[f[:, 0]] * torch.linalg.cross(v[f[:, 1]], v[f[:, 2]])).sum() / 6.0)


@torch.no_grad()
def solidify_mesh(verts, faces, colors, resolution: int = 256, bound: Optional[float] = None, trunc: Optional[float] = None,
                  beta: float = DEFAULT_BETA, smooth: int = 0, flip: bool = False, device="cuda"):
    """(verts, faces, colors, stats) of the closed mesh around the solid that (verts, faces) bounds: mesh_to_volume, then
    geometry.extract_mesh, then `smooth` iterations of mesh_clean.taubin_smooth (0: none).  A hole is closed where the winding number
    crosses 0.5, to a voxel: for a flat hole, about the flat disc on its rim.  ORIENTATION MATTERS: the faces must be wound outward;  a mesh
    wound inward solidifies to an empty mesh, and flip=True reverses every face first.  stats: "boundary_edges_before", "boundary_edges_after",
    "boundary_vertices_before", "boundary_vertices_after", "vertices", "faces", "edges", "euler" (V - E + F of the result), "volume"
    (signed_volume), "resolution", "bound", "trunc", "beta", "smooth_iterations", "flipped", "bvh_rounds", "moment_rounds",
    "mesh_distance" (mesh_query.mesh_distance from the input to the result and back, its "relative" part: over the result's diagonal;
    None for an empty result), "seconds"."""
    who = "solidify_mesh"
    smooth = _count_arg(smooth, who, "smooth")
    _volume_args(resolution, bound, trunc, beta, who)
    v, f, c = _mesh_arg(verts, faces, colors, device, who)
    if v.shape[0] == 0 or f.shape[0] == 0:
        raise ValueError(f"{who}: a mesh of {v.shape[0]} vertices and {f.shape[0]} faces bounds nothing")
    if flip:
        f = f[:, [0, 2, 1]].contiguous()
    t0 = time.perf_counter()
    _, open_before = edge_counts(f, v.shape[0])
    bv_before = int(boundary_vertices(f, v.shape[0], device).sum())
    vol, bvh, mrounds = _mesh_to_volume(v, f, c, resolution, bound, trunc, beta, device, who)
    vo, fo, co = extract_mesh(vol)
    if smooth and fo.shape[0]:
        vo = taubin_smooth(vo, fo, iterations=smooth, device=device)
    E, open_after = edge_counts(fo, vo.shape[0])
    stats = {"boundary_edges_before": open_before, "boundary_edges_after": open_after, "boundary_vertices_before": bv_before,
             "boundary_vertices_after": int(boundary_vertices(fo, vo.shape[0], device).sum()) if fo.shape[0] else 0, "vertices": int(vo.shape[0]),
             "faces": int(fo.shape[0]), "edges": E, "euler": int(vo.shape[0]) - E + int(fo.shape[0]), "volume": signed_volume(vo, fo),
             "resolution": vol.resolution, "bound": vol.bound, "trunc": vol.trunc, "beta": float(beta), "smooth_iterations": smooth,
             "flipped": bool(flip), "bvh_rounds": bvh.rounds, "moment_rounds": mrounds, "mesh_distance": None}
    if fo.shape[0]:
        stats["mesh_distance"] = mesh_distance(v, f, vo, fo, device=device)["relative"]
    if device != "cpu" and torch.cuda.is_available():
        torch.cuda.synchronize()
    stats["seconds"] = time.perf_counter() - t0
    return vo, fo, co, stats


# ---- looking at it --------------------------------------------------------------------------------------------------------------------------
def render_solid_orbit(verts, faces, colors, n: int, radius: float, elevation: float, fov: float, reso: int, white_background: bool = True,
                       device="cuda") -> np.ndarray:
    """n turntable frames of the mesh through the mesh rasterizer (mesh_render.render_mesh_orbit), uint8 [n, reso, reso, 3] on the host"""
    from .mesh_render import render_mesh_orbit
    return render_mesh_orbit(verts, faces, colors, n, radius, elevation, fov, reso, white_background, device=device)
