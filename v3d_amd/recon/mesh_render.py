"""Render the extracted triangle mesh on the gfx950 rasterizer of libv3d_recon.so (csrc_recon/meshrast.hip, include/v3d_recon.h "Mesh
rasterizer"): previews of the mesh, and how well it reproduces the orbit it was built from.

    out = render_mesh(cam, verts, faces, colors, bg)          # {"render", "depth", "alpha", "face_id"}
    frames = render_mesh_orbit(verts, faces, colors, 36, 2.0, 0.0, 60.0, 512, True)
    fid = mesh_fidelity(verts, faces, colors, cameras, images, bg)

One view: project -> face_setup -> scan -> duplicate_keys -> sort -> tile_ranges -> render; the scan and the sort are the splat rasterizer's
(v3d_gs_scan, v3d_gs_radix_sort_pairs).  Forward only, no atomics: two runs are bit-equal.  There is no fallback: without the libraries this
raises."""
from __future__ import annotations

import ctypes as C
from typing import Sequence

import numpy as np
import torch

from ..ops import get_ops
from .cameras import Camera, orbit_cameras
from .geometry import _check, _stream, load_library
from .rasterize import gs_camera

MAX_IMAGE = 4096
MAX_SUBPIXEL_BITS = 8
INT32_MAX = 2 ** 31 - 1


def _dev(a, dtype, device) -> torch.Tensor:
    t = a if torch.is_tensor(a) else torch.from_numpy(np.ascontiguousarray(a))
    return t.detach().to(device=device, dtype=dtype).contiguous()


def _mesh_on_device(verts, faces, colors, device):
    v = _dev(verts, torch.float32, device).reshape(-1, 3)
    c = _dev(colors, torch.float32, device).reshape(-1, 3)
    f = faces if torch.is_tensor(faces) else torch.from_numpy(np.ascontiguousarray(faces))
    if f.is_floating_point() or f.dtype == torch.bool:
        raise ValueError(f"render_mesh: faces must be integers, got {f.dtype}")
    f = f.detach().reshape(-1, 3)
    if c.shape != v.shape:
        raise ValueError(f"render_mesh: {v.shape[0]} vertices, {c.shape[0]} colours")
    if f.numel() and (int(f.min()) < 0 or int(f.max()) >= v.shape[0]):
        raise ValueError("render_mesh: face index outside the vertex array")
    return v, f.to(device=device, dtype=torch.int32).contiguous(), c


def _check_view(W: int, H: int, subpixel_bits: int):
    if not (0 < W <= MAX_IMAGE and 0 < H <= MAX_IMAGE):
        raise ValueError(f"render_mesh: image {W} x {H} outside 1 .. {MAX_IMAGE} on a side")
    if not 0 <= int(subpixel_bits) <= MAX_SUBPIXEL_BITS:
        raise ValueError(f"render_mesh: subpixel_bits {subpixel_bits} outside 0 .. {MAX_SUBPIXEL_BITS}")


def project_vertices(gc, verts: torch.Tensor, subpixel_bits: int = 8):
    """(zv [V], pix_f [V, 2] float32, pix_q [V, 2] int32) of device vertices [V, 3] through the camera struct `gc` (rasterize.gs_camera)."""
    lib = load_library()
    V = verts.shape[0]
    zv = torch.empty(V, dtype=torch.float32, device=verts.device)
    pix_f = torch.empty(V, 2, dtype=torch.float32, device=verts.device)
    pix_q = torch.empty(V, 2, dtype=torch.int32, device=verts.device)
    _check(lib, lib.v3d_recon_mesh_project(verts.data_ptr(), V, C.byref(gc), int(subpixel_bits), zv.data_ptr(), pix_f.data_ptr(), pix_q.data_ptr(),
                                           _stream()), "v3d_recon_mesh_project")
    return zv, pix_f, pix_q


def rasterize_projected(gc, faces: torch.Tensor, pix_q: torch.Tensor, zv: torch.Tensor, colors: torch.Tensor, cull: bool = True,
                        count_hits: bool = False, subpixel_bits: int = 8) -> dict:
    """Everything after the projection, on device tensors: faces [F, 3] int32 (F >= 1), the projection's pix_q and zv, colors [V, 3].  Also
    returns the binning's intermediates ("tiles_touched", "zmin", "ranges", "n_inst")."""
    lib, ops = load_library(), get_ops()
    dev = faces.device
    W, H = int(gc.width), int(gc.height)
    _check_view(W, H, subpixel_bits)
    F, V, bits = faces.shape[0], zv.shape[0], int(subpixel_bits)
    tiles = torch.empty(F, dtype=torch.int32, device=dev)
    zmin = torch.empty(F, dtype=torch.float32, device=dev)
    _check(lib, lib.v3d_recon_mesh_face_setup(faces.data_ptr(), F, pix_q.data_ptr(), zv.data_ptr(), V, W, H, bits, int(bool(cull)), tiles.data_ptr(),
                                              zmin.data_ptr(), _stream()), "v3d_recon_mesh_face_setup")
    total = int(tiles.sum(dtype=torch.int64).item())       # (the int32 scan below would wrap silently)
    if total > INT32_MAX:
        raise RuntimeError(f"render_mesh: {total} face-tile pairs exceed {INT32_MAX}; render at a lower resolution or split the mesh")
    offsets = ops.gs_scan(tiles)
    n_inst = int(offsets[-1].item())
    ntiles = ((W + 15) // 16) * ((H + 15) // 16)
    ranges = torch.empty(ntiles, 2, dtype=torch.int32, device=dev)
    vals_s = None
    if n_inst:
        keys = torch.empty(n_inst, dtype=torch.int64, device=dev)
        vals = torch.empty(n_inst, dtype=torch.int32, device=dev)
        _check(lib, lib.v3d_recon_mesh_duplicate_keys(faces.data_ptr(), F, pix_q.data_ptr(), V, tiles.data_ptr(), offsets.data_ptr(), zmin.data_ptr(),
                                                      W, H, bits, keys.data_ptr(), vals.data_ptr(), _stream()), "v3d_recon_mesh_duplicate_keys")
        keys_s, vals_s = ops.gs_radix_sort_pairs(keys, vals, 32 + max(1, (ntiles - 1).bit_length()))
        _check(lib, lib.v3d_recon_mesh_tile_ranges(keys_s.data_ptr(), n_inst, W, H, ranges.data_ptr(), _stream()), "v3d_recon_mesh_tile_ranges")
    else:
        _check(lib, lib.v3d_recon_mesh_tile_ranges(None, 0, W, H, ranges.data_ptr(), _stream()), "v3d_recon_mesh_tile_ranges")
    image = torch.empty(3, H, W, dtype=torch.float32, device=dev)
    depth = torch.empty(H, W, dtype=torch.float32, device=dev)
    alpha = torch.empty(H, W, dtype=torch.float32, device=dev)
    face_id = torch.empty(H, W, dtype=torch.int32, device=dev)
    n_hit = torch.empty(H, W, dtype=torch.int32, device=dev) if count_hits else None
    _check(lib, lib.v3d_recon_mesh_render(ranges.data_ptr(), vals_s.data_ptr() if vals_s is not None else None, faces.data_ptr(), F, pix_q.data_ptr(),
                                          zv.data_ptr(), zmin.data_ptr(), colors.data_ptr(), C.byref(gc), bits, image.data_ptr(), depth.data_ptr(),
                                          alpha.data_ptr(), face_id.data_ptr(), n_hit.data_ptr() if count_hits else None, _stream()),
           "v3d_recon_mesh_render")
    out = {"render": image, "depth": depth, "alpha": alpha, "face_id": face_id, "tiles_touched": tiles, "zmin": zmin, "ranges": ranges, "n_inst": n_inst}
    if count_hits:
        out["n_hit"] = n_hit
    return out


@torch.no_grad()
def render_mesh(camera: Camera, verts, faces, colors, bg, cull: bool = True, count_hits: bool = False, subpixel_bits: int = 8, device="cuda") -> dict:
    """{"render": image [3, H, W], "depth": view z [H, W] (0 where nothing covers), "alpha": 0 or 1 [H, W], "face_id": int32 [H, W] (-1 where
    nothing covers)} and, with count_hits, "n_hit": int32 [H, W], the number of drawn faces over every pixel centre (even everywhere for a
    closed mesh with cull=False).  verts [V, 3], faces [F, 3] (integers), colors [V, 3] in 0 .. 1: tensors or numpy arrays, moved to `device`.
    cull=True drops the faces that look away from the camera (outward normals, the winding extract_mesh writes).  A face with a vertex at
    view z <= 0.2 is dropped whole: there is no near-plane clipping."""
    _check_view(int(camera.width), int(camera.height), subpixel_bits)
    v, f, c = _mesh_on_device(verts, faces, colors, device)
    return _render_views(camera, v, f, c, bg, ((cull, count_hits),), subpixel_bits)[0]


_OUTPUTS = ("render", "depth", "alpha", "face_id", "n_hit")


def _render_views(camera: Camera, v, f, c, bg, modes, subpixel_bits: int = 8):
    """One dict per (cull, count_hits) of `modes` from ONE projection of a mesh that _mesh_on_device has already validated and moved"""
    H, W = int(camera.height), int(camera.width)
    device = v.device
    if f.shape[0] == 0 or v.shape[0] == 0:          # nothing to draw: the background, without a launch (the kernels take V, F >= 1)
        outs = []
        for _, count_hits in modes:
            bgt = torch.as_tensor(bg, dtype=torch.float32).to(device)
            out = {"render": bgt.view(3, 1, 1).expand(3, H, W).contiguous(), "depth": torch.zeros(H, W, device=device),
                   "alpha": torch.zeros(H, W, device=device), "face_id": torch.full((H, W), -1, dtype=torch.int32, device=device)}
            if count_hits:
                out["n_hit"] = torch.zeros(H, W, dtype=torch.int32, device=device)
            outs.append(out)
        return outs
    gc = gs_camera(camera, bg)
    zv, _, pix_q = project_vertices(gc, v, subpixel_bits)
    outs = []
    for cull, count_hits in modes:
        full = rasterize_projected(gc, f, pix_q, zv, c, cull, count_hits, subpixel_bits)
        outs.append({k: full[k] for k in _OUTPUTS if k in full})
    return outs


def _bg(white_background: bool):
    return [1.0, 1.0, 1.0] if white_background else [0.0, 0.0, 0.0]


@torch.no_grad()
def render_mesh_orbit(verts, faces, colors, n: int, radius: float, elevation: float, fov: float, reso: int, white_background: bool = True,
                      cull: bool = True, device="cuda") -> np.ndarray:
    """n turntable frames of the mesh from the cameras of orbit_cameras, uint8 [n, reso, reso, 3] on the host (as train.render_orbit)."""
    cams, _ = orbit_cameras(n, radius, elevation, fov, reso)
    _check_view(int(reso), int(reso), 8)
    v, f, c = _mesh_on_device(verts, faces, colors, device)          # validated and moved once, not per view
    out = []
    for cam in cams:
        img = _render_views(cam, v, f, c, _bg(white_background), ((cull, False),))[0]["render"]
        out.append((img.clamp(0, 1) * 255).to(torch.uint8).permute(1, 2, 0).cpu())
    return torch.stack(out).numpy()


def _frames(images, device) -> torch.Tensor:
    """float32 [T, 3, H, W] in 0 .. 1 of uint8 frames [T, H, W, 3] or of float images [T, 3, H, W]"""
    t = images if torch.is_tensor(images) else (torch.from_numpy(np.ascontiguousarray(images)) if isinstance(images, np.ndarray)
                                                else torch.stack([torch.as_tensor(i) for i in images]))
    if t.dtype == torch.uint8:
        return t.to(device).permute(0, 3, 1, 2).float() / 255.0
    return t.to(device).float().clamp(0, 1)


@torch.no_grad()
def mesh_fidelity(verts, faces, colors, cameras: Sequence[Camera], images, bg, device="cuda") -> dict:
    """How well the mesh reproduces `images` (uint8 [T, H, W, 3] or float [T, 3, H, W], one per camera): {"psnr": per-view PSNR of the mesh
    render (culling on, clamped to 0 .. 1) against the frame, "psnr_mean", "coverage": share of covered pixels per view, "odd_hit_pixels":
    per view, pixels with an odd number of faces over them with culling off (0 everywhere for a closed mesh)}."""
    from .train import psnr
    gt = _frames(images, device)
    if gt.shape[0] != len(cameras):
        raise ValueError(f"mesh_fidelity: {gt.shape[0]} images for {len(cameras)} cameras")
    v, f, c = _mesh_on_device(verts, faces, colors, device)
    ps, cov, odd = [], [], []
    for cam, frame in zip(cameras, gt):
        if tuple(frame.shape) != (3, int(cam.height), int(cam.width)):
            raise ValueError(f"mesh_fidelity: frame {tuple(frame.shape)} does not match the {cam.width} x {cam.height} camera")
        _check_view(int(cam.width), int(cam.height), 8)
        out, counted = _render_views(cam, v, f, c, bg, ((True, False), (False, True)))
        hits = counted["n_hit"]
        ps.append(psnr(out["render"].clamp(0, 1), frame))
        cov.append(float(out["alpha"].mean()))
        odd.append(int((hits % 2 == 1).sum()))
    return {"psnr": ps, "psnr_mean": float(np.mean(ps)) if ps else float("nan"), "coverage": cov, "odd_hit_pixels": odd}
