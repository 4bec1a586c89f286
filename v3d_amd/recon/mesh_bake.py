"""Bake a normal map of the full mesh onto the decimated one, on the gfx950 kernels of libv3d_recon.so (csrc_recon/meshbvh.hip,
include/v3d_recon.h "Mesh BVH and normal bake"): a linear BVH built on the device, a closest-hit query, and the bake over the per-face atlas
of mesh_texture.py.

    bvh = build_bvh(high_verts, high_faces)                       # MeshBVH: order, left, right, parent, lo, hi, rounds
    t, face, uv = cast_rays(bvh, origins, directions, tmin=0.0, tmax=inf, cull=0)
    normal_map, stats = bake_normal_map(low_verts, low_faces, high_verts, high_faces, tex_size=1024)
    fid = normal_map_fidelity(low_verts, low_faces, normal_map, high_verts, high_faces, cameras)
    save_textured_obj("mesh.obj", low_verts, low_faces, vt, texture, normal_map=normal_map)     # + mesh_normal.png, `norm` in the MTL

The map is in object space.  No atomics anywhere: two calls with the same arguments return bit-equal trees and maps.  Everything runs under
no_grad.  There is no fallback: without the libraries this raises."""
from __future__ import annotations

import dataclasses
import math
import time
from typing import Optional, Sequence

import numpy as np
import torch

from ..ops import get_ops
from .cameras import Camera, orbit_cameras
from .geometry import _check, _stream, load_library
from .mesh_clean import DEFAULT_NORMAL, _corner_lists, _mesh_arg, _normals, normal_colors, render_mesh_normals
from .mesh_render import _bg, _check_view, _dev
from .mesh_texture import MAX_TEX_SIZE, atlas_layout, prepare_texture_view, texture_shade_forward

MAX_FACES = 2 ** 30                # 2 F - 1 fits int32
ROUND_GROUP = 8                    # fit rounds between two reads of the flag words
KEY_BITS = 30
DEFAULT_MAX_DIST = 0.05            # x the diagonal of the high mesh's bounding box: a choice, not a measurement


@dataclasses.dataclass
class MeshBVH:
    """The tree of include/v3d_recon.h "THE NODES" over faces [F, 3] (int32) of verts [V, 3]: order [F] (int32: the face of every leaf),
    left, right [max(F - 1, 1)] (int32; -1 -1 when F = 1), parent [2F - 1], lo, hi [2F - 1, 3]; rounds: the fit rounds run up to and including
    the first that changed nothing (0 when F = 1)."""
    verts: torch.Tensor
    faces: torch.Tensor
    order: torch.Tensor
    left: torch.Tensor
    right: torch.Tensor
    parent: torch.Tensor
    lo: torch.Tensor
    hi: torch.Tensor
    rounds: int

    @property
    def num_faces(self) -> int:
        return self.faces.shape[0]

    def _args(self):
        return (self.left.data_ptr(), self.right.data_ptr(), self.order.data_ptr(), self.lo.data_ptr(), self.hi.data_ptr(), self.verts.data_ptr(),
                self.verts.shape[0], self.faces.data_ptr(), self.faces.shape[0])


def height_bound(num_faces: int) -> int:
    """30 levels of code prefix, then the tie-break on the sorted position"""
    return KEY_BITS + max(int(num_faces) - 1, 0).bit_length()


def _high_mesh(verts, faces, device, who: str):
    """verts [V, 3] float32, faces [F, 3] int32 on the device.  Unlike the other stages' meshes this one may hold faces with an index outside
    the vertices: they get an empty box and are never hit."""
    v = _dev(verts, torch.float32, device)
    f = faces if torch.is_tensor(faces) else torch.from_numpy(np.ascontiguousarray(faces))
    if v.dim() != 2 or v.shape[1] != 3:
        raise ValueError(f"{who}: verts must be [V, 3], got {tuple(v.shape)}")
    if f.is_floating_point() or f.dtype == torch.bool or f.dim() != 2 or f.shape[1] != 3:
        raise ValueError(f"{who}: faces must be integers [F, 3], got {f.dtype} {tuple(f.shape)}")
    if f.shape[0] == 0 or v.shape[0] == 0:
        raise ValueError(f"{who}: a mesh of {v.shape[0]} vertices and {f.shape[0]} faces has nothing to hit")
    if f.shape[0] > MAX_FACES:
        raise ValueError(f"{who}: {f.shape[0]} faces: 2 F - 1 must fit int32")
    if not bool(torch.isfinite(v).all()):
        raise ValueError(f"{who}: a vertex is not finite")
    f = f.detach().clamp(-1, 2 ** 31 - 1).to(device=device, dtype=torch.int32).contiguous()
    return v, f


@torch.no_grad()
def build_bvh(verts, faces, device="cuda") -> MeshBVH:
    """The BVH of a mesh (tensors or numpy arrays; at least one vertex and one face, else ValueError before any launch)."""
    v, f = _high_mesh(verts, faces, device, "build_bvh")
    lib, ops = load_library(), get_ops()
    V, F = v.shape[0], f.shape[0]
    box = torch.stack([v.min(0).values, v.max(0).values]).cpu().tolist()
    keys = torch.empty(F, dtype=torch.int64, device=device)
    vals = torch.empty(F, dtype=torch.int32, device=device)
    face_lo = torch.empty(F, 3, dtype=torch.float32, device=device)
    face_hi = torch.empty(F, 3, dtype=torch.float32, device=device)
    _check(lib, lib.v3d_recon_bvh_face_keys(v.data_ptr(), V, f.data_ptr(), F, *box[0], *box[1], keys.data_ptr(), vals.data_ptr(), face_lo.data_ptr(),
                                            face_hi.data_ptr(), _stream()), "v3d_recon_bvh_face_keys")
    keys_s, order = ops.gs_radix_sort_pairs(keys, vals, KEY_BITS)
    n = max(F - 1, 1)
    left = torch.full((n,), -1, dtype=torch.int32, device=device)
    right = torch.full((n,), -1, dtype=torch.int32, device=device)
    parent = torch.empty(2 * F - 1, dtype=torch.int32, device=device)
    lo = torch.full((2 * F - 1, 3), float("inf"), dtype=torch.float32, device=device)
    hi = torch.full((2 * F - 1, 3), float("-inf"), dtype=torch.float32, device=device)
    _check(lib, lib.v3d_recon_bvh_build_nodes(keys_s.data_ptr(), order.data_ptr(), face_lo.data_ptr(), face_hi.data_ptr(), F, left.data_ptr(),
                                              right.data_ptr(), parent.data_ptr(), lo.data_ptr(), hi.data_ptr(), _stream()), "v3d_recon_bvh_build_nodes")
    rounds = _fit(lib, left, right, F, lo, hi) if F > 1 else 0
    return MeshBVH(v, f, order, left, right, parent, lo, hi, rounds)


def _fit(lib, left, right, F: int, lo, hi) -> int:
    """The fit rounds, in groups of ROUND_GROUP with a flag word each, read once per group (as mesh_clean._labels)"""
    cur = torch.zeros(F - 1, dtype=torch.int32, device=left.device)
    nxt = torch.empty_like(cur)
    flags = torch.empty(ROUND_GROUP, dtype=torch.int32, device=left.device)
    done, limit = 0, height_bound(F) + 8
    while done < limit:
        group = min(ROUND_GROUP, limit - done)
        flags.zero_()
        for j in range(group):
            _check(lib, lib.v3d_recon_bvh_fit_round(left.data_ptr(), right.data_ptr(), F, cur.data_ptr(), nxt.data_ptr(), lo.data_ptr(), hi.data_ptr(),
                                                    flags.data_ptr() + 4 * j, _stream()), "v3d_recon_bvh_fit_round")
            cur, nxt = nxt, cur
        changed = flags.cpu().tolist()[:group]
        if 0 in changed:
            if not bool(cur.all()):
                raise RuntimeError(f"build_bvh: the fit stopped with nodes left open on {F} faces: the tree is broken")
            return done + changed.index(0) + 1
        done += group
    raise RuntimeError(f"build_bvh: no fixed point after {limit} fit rounds on {F} faces: the tree is broken")


def _cull_arg(cull, who: str) -> int:
    if isinstance(cull, bool) or cull not in (0, 1, 2):
        raise ValueError(f"{who}: cull {cull!r} is not 0 (every triangle), 1 (Ng . d < 0) or 2 (Ng . d > 0)")
    return int(cull)


@torch.no_grad()
def cast_rays(bvh: MeshBVH, origins, directions, tmin: float = 0.0, tmax: float = math.inf, cull: int = 0):
    """(t [N] float32, face [N] int32, uv [N, 2] float32) of the closest hit of every ray origins[i] + t directions[i], tmin <= t <= tmax, on
    the tree's device.  Directions are used as given.  A miss: +inf, -1, 0 0."""
    cull = _cull_arg(cull, "cast_rays")
    tmin, tmax = float(tmin), float(tmax)
    if math.isnan(tmin) or math.isnan(tmax):
        raise ValueError("cast_rays: tmin or tmax is NaN")
    dev = bvh.verts.device
    o, d = _dev(origins, torch.float32, dev), _dev(directions, torch.float32, dev)
    if o.dim() != 2 or o.shape[1] != 3 or o.shape != d.shape:
        raise ValueError(f"cast_rays: origins {tuple(o.shape)} and directions {tuple(d.shape)} must both be [N, 3]")
    N = o.shape[0]
    if N > 2 ** 31 - 1:
        raise ValueError(f"cast_rays: {N} rays do not fit int32")
    t = torch.empty(N, dtype=torch.float32, device=dev)
    face = torch.empty(N, dtype=torch.int32, device=dev)
    uv = torch.empty(N, 2, dtype=torch.float32, device=dev)
    if N == 0:
        return t, face, uv
    lib = load_library()
    _check(lib, lib.v3d_recon_bvh_closest_hit(o.data_ptr(), d.data_ptr(), tmin, tmax, N, cull, *bvh._args(), t.data_ptr(), face.data_ptr(), uv.data_ptr(),
                                              _stream()), "v3d_recon_bvh_closest_hit")
    return t, face, uv


def default_max_dist(high_verts) -> float:
    v = high_verts if torch.is_tensor(high_verts) else torch.from_numpy(np.ascontiguousarray(high_verts))
    v = v.detach().float().reshape(-1, 3)
    return DEFAULT_MAX_DIST * float((v.max(0).values - v.min(0).values).norm()) if v.shape[0] else 0.0


def _tex_arg(tex_size, who: str) -> int:
    R = int(tex_size)
    if not 1 <= R <= MAX_TEX_SIZE:
        raise ValueError(f"{who}: tex_size {R} outside 1 .. {MAX_TEX_SIZE}")
    return R


@torch.no_grad()
def bake_texels(low_verts, low_faces, low_normals, bvh: MeshBVH, high_normals, tex_size: int, max_dist: float):
    """The kernel's four outputs on validated device tensors (low mesh V, F >= 1): owner [R*R] int32, normal_map [R*R, 3], dist [R*R] (signed,
    NaN without a hit), hit_face [R*R] int32"""
    lib = load_library()
    R, dev = int(tex_size), bvh.verts.device
    owner = torch.empty(R * R, dtype=torch.int32, device=dev)
    nmap = torch.empty(R * R, 3, dtype=torch.float32, device=dev)
    dist = torch.empty(R * R, dtype=torch.float32, device=dev)
    hit = torch.empty(R * R, dtype=torch.int32, device=dev)
    _check(lib, lib.v3d_recon_tex_bake_normals(low_verts.data_ptr(), low_verts.shape[0], low_faces.data_ptr(), low_faces.shape[0], low_normals.data_ptr(), R,
                                               float(max_dist), *bvh._args(), high_normals.data_ptr(), owner.data_ptr(), nmap.data_ptr(), dist.data_ptr(),
                                               hit.data_ptr(), _stream()), "v3d_recon_tex_bake_normals")
    return owner, nmap, dist, hit


def _vertex_normals(v, f):
    return _normals(v, f, *_corner_lists(f, v.shape[0]))


@torch.no_grad()
def bake_normal_map(low_verts, low_faces, high_verts, high_faces, tex_size: int = 1024, max_dist: Optional[float] = None, device="cuda"):
    """(normal_map [R*R, 3] float32 on `device`, stats).  Every texel of the low mesh's atlas casts along its interpolated vertex normal, both
    ways, against the high mesh (at most max_dist away; default 0.05 x the diagonal of the high mesh's bounding box) and takes the high mesh's
    interpolated vertex normal at the nearer hit; a texel without a hit keeps the low mesh's own normal; unowned texels hold (0, 0, 1).
    stats: "hit_plus", "hit_minus", "missed", "owned", "displacement_mean", "displacement_max" (|signed distance| over the owned texels that
    hit: the geometric error of the decimation sampled along the normals), "max_dist", "bvh_rounds", "tex_size", "cell", "seconds".  A low
    mesh with V = 0 or F = 0 gives an all-(0, 0, 1) map without a launch."""
    R = _tex_arg(tex_size, "bake_normal_map")
    lv, lf, _ = _mesh_arg(low_verts, low_faces, None, device, "bake_normal_map")
    hv, hf, _ = _mesh_arg(high_verts, high_faces, None, device, "bake_normal_map")
    md = default_max_dist(hv) if max_dist is None else float(max_dist)
    if not (math.isfinite(md) and md >= 0):
        raise ValueError(f"bake_normal_map: max_dist {max_dist} must be finite and not negative")
    stats = {"hit_plus": 0, "hit_minus": 0, "missed": 0, "owned": 0, "displacement_mean": float("nan"), "displacement_max": float("nan"), "max_dist": md,
             "bvh_rounds": 0, "tex_size": R, "cell": 0, "seconds": 0.0}
    if lv.shape[0] == 0 or lf.shape[0] == 0:
        return torch.tensor(DEFAULT_NORMAL, dtype=torch.float32, device=device).expand(R * R, 3).contiguous(), stats
    stats["cell"] = atlas_layout(lf.shape[0], R)[0]
    if hv.shape[0] == 0 or hf.shape[0] == 0:
        raise ValueError("bake_normal_map: the high mesh has no faces to hit")
    t0 = time.perf_counter()
    bvh = build_bvh(hv, hf, device)
    owner, nmap, dist, _ = bake_texels(lv, lf, _vertex_normals(lv, lf), bvh, _vertex_normals(hv, hf), R, md)
    owned, hit = owner >= 0, ~torch.isnan(dist)
    plus = hit & ~torch.signbit(dist)
    stats.update(owned=int(owned.sum()), hit_plus=int(plus.sum()), hit_minus=int((hit & ~plus).sum()), bvh_rounds=bvh.rounds)
    stats["missed"] = stats["owned"] - stats["hit_plus"] - stats["hit_minus"]
    if bool(hit.any()):
        d = dist[hit].abs()
        stats["displacement_mean"], stats["displacement_max"] = float(d.double().mean()), float(d.max())
    if device != "cpu" and torch.cuda.is_available():
        torch.cuda.synchronize()
    stats["seconds"] = time.perf_counter() - t0
    return nmap, stats


# ---- looking at it --------------------------------------------------------------------------------------------------------------------------
def _camera_normals(camera: Camera, image: torch.Tensor) -> torch.Tensor:
    """[3, H, W] unit normals in the camera's frame from an image of normal_colors"""
    n = image * 2.0 - 1.0
    return n / n.norm(dim=0, keepdim=True).clamp_min(1e-12)


def _map_square(normal_map, device):
    m = _dev(normal_map, torch.float32, device).reshape(-1, 3)
    R = math.isqrt(m.shape[0])
    if R * R != m.shape[0] or R == 0:
        raise ValueError(f"normal map: {m.shape[0]} texels are not a square")
    return m, R


def sample_normal_map(camera: Camera, verts, faces, normal_map, R: int, cull: bool = True, device="cuda"):
    """(normals [3, H, W] in the camera's frame as normal_colors orients them, of length 1; alpha [H, W]): the map sampled as a texture
    (prepare_texture_view, texture_shade_forward), rotated into the camera and renormalised per pixel"""
    view = prepare_texture_view(camera, verts, faces, R, [0.0, 0.0, 0.0], cull=cull, lists=False, device=device)
    img = texture_shade_forward(view, normal_map)                                      # object-space vectors, 0 where nothing covers
    H, W = view.height, view.width
    n = normal_colors(camera, img.reshape(3, H * W).t()) * 2.0 - 1.0                    # [HW, 3]: the rotation and the flip of normal_colors
    n = n / n.norm(dim=1, keepdim=True).clamp_min(1e-12)
    return n.t().reshape(3, H, W), view.alpha


def _mean_angle(a: torch.Tensor, b: torch.Tensor, both: torch.Tensor) -> float:
    if not bool(both.any()):
        return float("nan")
    cos = (a * b).sum(0)[both].double().clamp(-1, 1)
    return float(torch.rad2deg(torch.acos(cos)).mean())


@torch.no_grad()
def normal_map_fidelity(low_verts, low_faces, normal_map, high_verts, high_faces, cameras: Sequence[Camera], device="cuda") -> dict:
    """How close the low mesh's shading normals come to the high mesh's: per view the mean angle in degrees, over the pixels both meshes
    cover, between the high mesh's rendered vertex normals (render_mesh_normals) and the low mesh's (a) rendered vertex normals, "before",
    (b) normal map sampled per pixel, "after".  {"angle_before", "angle_after": per view, "angle_before_mean", "angle_after_mean",
    "pixels": per view}."""
    lv, lf, _ = _mesh_arg(low_verts, low_faces, None, device, "normal_map_fidelity")
    hv, hf, _ = _mesh_arg(high_verts, high_faces, None, device, "normal_map_fidelity")
    m, R = _map_square(normal_map, device)
    before, after, pixels = [], [], []
    for cam in cameras:
        _check_view(int(cam.width), int(cam.height), 8)
        high = render_mesh_normals(cam, hv, hf, device=device)
        low = render_mesh_normals(cam, lv, lf, device=device)
        mapped, alpha = sample_normal_map(cam, lv, lf, m, R, device=device)
        both = (high["alpha"] > 0) & (low["alpha"] > 0) & (alpha > 0)
        nh = _camera_normals(cam, high["render"])
        before.append(_mean_angle(_camera_normals(cam, low["render"]), nh, both))
        after.append(_mean_angle(mapped, nh, both))
        pixels.append(int(both.sum()))
    mean = lambda xs: float(np.nanmean(xs)) if len(xs) and not all(math.isnan(x) for x in xs) else float("nan")  # noqa: E731
    return {"angle_before": before, "angle_after": after, "angle_before_mean": mean(before), "angle_after_mean": mean(after), "pixels": pixels}


@torch.no_grad()
def render_normal_mapped_orbit(verts, faces, normal_map, n: int, radius: float, elevation: float, fov: float, reso: int, white_background: bool = True,
                               cull: bool = True, device="cuda") -> np.ndarray:
    """n turntable frames of the low mesh shaded with its normal map as normal_colors draws normals, uint8 [n, reso, reso, 3] on the host"""
    cams, _ = orbit_cameras(n, radius, elevation, fov, reso)
    _check_view(int(reso), int(reso), 8)
    v, f, _ = _mesh_arg(verts, faces, None, device, "render_normal_mapped_orbit")
    m, R = _map_square(normal_map, device)
    bg = torch.tensor(_bg(white_background), dtype=torch.float32, device=device).view(3, 1, 1)
    out = []
    for cam in cams:
        nrm, alpha = sample_normal_map(cam, v, f, m, R, cull, device)
        img = torch.where(alpha[None] > 0, (nrm + 1.0) * 0.5, bg)
        out.append((img.clamp(0, 1) * 255).to(torch.uint8).permute(1, 2, 0).cpu())
    return torch.stack(out).numpy() if out else np.zeros((0, int(reso), int(reso), 3), dtype=np.uint8)
