"""Fit the mesh's vertices to the orbit's silhouettes on the gfx950 kernels of libv3d_recon.so (csrc_recon/meshdeform.hip, include/v3d_recon.h
"Mesh vertex fit"): the counterpart of the reference's recon/convert_nerf_mesh.py::fit_mesh, the one stage that moves the geometry.

    alpha = antialiased_alpha(cam, verts, faces)               # [H, W], differentiable in verts [V, 3]
    targets = silhouette_targets(gaussians, cameras, bg)       # the alpha of the splats, one map per camera
    verts, stats = fit_vertices(verts, faces, cameras, targets)

Coverage is the integer rasterizer's (mesh_render.py); at the border between the object and the background it is antialiased from the
unsnapped float positions, and that is where the gradient to the vertices comes from.  Visibility changes with every step, so every
iteration rasterizes anew.  The gradient is reduced without atomics (count -> v3d_gs_scan -> emit -> v3d_gs_radix_sort_pairs -> ranges -> one
wave per vertex): two calls with the same arguments return bit-equal vertices.  There is no fallback: without the libraries this raises."""
from __future__ import annotations

import ctypes as C
import time
from typing import Sequence

import numpy as np
import torch

from ..ops import get_ops
from .cameras import Camera
from .geometry import _check, _stream, load_library
from .mesh_clean import _corner_lists
from .mesh_refine import optimisation_views, view_schedule
from .mesh_render import _check_view, _dev, _mesh_on_device, project_vertices, rasterize_projected
from .rasterize import gs_camera

LR, LAMBDA_OFFSET, ITERATIONS = 1e-4, 0.1, 2048          # the reference's fit_mesh
LAMBDA_SMOOTH = 10.0                                    # no counterpart there: DESIGN.md 3.14 has the sweep
BG = (0.0, 0.0, 0.0)


# ---- the kernels, on device tensors (V >= 1, F >= 1) ----------------------------------------------------------------------------------------
def aa_forward(face_id: torch.Tensor, faces: torch.Tensor, pix_f: torch.Tensor, pix_q: torch.Tensor):
    """(alpha_aa [H, W], alpha_raw [H, W]: the sum before the clamp) of a face_id map [H, W] int32 and the faces [F, 3] int32, unsnapped
    pix_f [V, 2] and snapped pix_q [V, 2] it was rendered from (v3d_recon_mesh_aa_alpha)"""
    lib = load_library()
    H, W = face_id.shape
    alpha = torch.empty(H, W, dtype=torch.float32, device=face_id.device)
    raw = torch.empty(H, W, dtype=torch.float32, device=face_id.device)
    _check(lib, lib.v3d_recon_mesh_aa_alpha(face_id.data_ptr(), faces.data_ptr(), faces.shape[0], pix_f.data_ptr(), pix_q.data_ptr(), pix_f.shape[0],
                                            W, H, alpha.data_ptr(), raw.data_ptr(), _stream()), "v3d_recon_mesh_aa_alpha")
    return alpha, raw


def aa_pairs(face_id: torch.Tensor, faces: torch.Tensor, pix_f: torch.Tensor, pix_q: torch.Tensor, debug: bool = False):
    """(counts [H W] int32: records per pixel, pair_info [H, W, 4] int32 or None) of v3d_recon_mesh_aa_count.  pair_info: per neighbour
    (right, left, down, up) -1 no pair, -2 a pair without a candidate, else the chosen edge k, + 4 when the neighbour receives."""
    lib = load_library()
    H, W = face_id.shape
    counts = torch.empty(H * W, dtype=torch.int32, device=face_id.device)
    info = torch.empty(H, W, 4, dtype=torch.int32, device=face_id.device) if debug else None
    _check(lib, lib.v3d_recon_mesh_aa_count(face_id.data_ptr(), faces.data_ptr(), faces.shape[0], pix_f.data_ptr(), pix_q.data_ptr(), pix_f.shape[0],
                                            W, H, counts.data_ptr(), info.data_ptr() if debug else None, _stream()), "v3d_recon_mesh_aa_count")
    return counts, info


def aa_reduce(ranges: torch.Tensor, vals_sorted, payload, num_verts: int) -> torch.Tensor:
    """dL_dpix [V, 2]: every vertex's payload rows summed by one wave in list order (v3d_recon_mesh_aa_reduce)"""
    lib = load_library()
    n = 0 if vals_sorted is None else vals_sorted.numel()
    out = torch.empty(num_verts, 2, dtype=torch.float32, device=ranges.device)
    _check(lib, lib.v3d_recon_mesh_aa_reduce(ranges.data_ptr(), vals_sorted.data_ptr() if n else None, payload.data_ptr() if n else None, n, num_verts,
                                             out.data_ptr(), _stream()), "v3d_recon_mesh_aa_reduce")
    return out


def aa_backward(face_id, faces, pix_f, pix_q, alpha_raw, dL_dalpha, debug: bool = False) -> dict:
    """{"dL_dpix" [V, 2], "records": n, "ranges" [V, 2]} (+ "pair_info", "keys", "payload" with debug) of dL_dalpha [H, W]"""
    lib, ops = load_library(), get_ops()
    H, W = face_id.shape
    V, dev = pix_f.shape[0], face_id.device
    g = dL_dalpha.detach().to(device=dev, dtype=torch.float32).contiguous()
    counts, info = aa_pairs(face_id, faces, pix_f, pix_q, debug)
    offsets = ops.gs_scan(counts)
    n = int(offsets[-1].item())          # (at most 8 x 4096^2: fits int32)
    ranges = torch.empty(V, 2, dtype=torch.int32, device=dev)
    out = {"records": n, "ranges": ranges}
    if n == 0:
        _check(lib, lib.v3d_recon_mesh_vertex_ranges(None, 0, V, ranges.data_ptr(), _stream()), "v3d_recon_mesh_vertex_ranges")
        out["dL_dpix"] = aa_reduce(ranges, None, None, V)
    else:
        keys = torch.empty(n, dtype=torch.int64, device=dev)
        vals = torch.empty(n, dtype=torch.int32, device=dev)
        payload = torch.empty(n, 2, dtype=torch.float32, device=dev)
        _check(lib, lib.v3d_recon_mesh_aa_emit(face_id.data_ptr(), faces.data_ptr(), faces.shape[0], pix_f.data_ptr(), pix_q.data_ptr(), V, W, H,
                                               alpha_raw.data_ptr(), g.data_ptr(), offsets.data_ptr(), n, keys.data_ptr(), vals.data_ptr(),
                                               payload.data_ptr(), _stream()), "v3d_recon_mesh_aa_emit")
        keys_s, vals_s = ops.gs_radix_sort_pairs(keys, vals, max(1, (V - 1).bit_length()))
        _check(lib, lib.v3d_recon_mesh_vertex_ranges(keys_s.data_ptr(), n, V, ranges.data_ptr(), _stream()), "v3d_recon_mesh_vertex_ranges")
        out["dL_dpix"] = aa_reduce(ranges, vals_s, payload, V)
        if debug:
            out.update(keys=keys, payload=payload, vals_sorted=vals_s)
    if debug:
        out["pair_info"] = info
    return out


def project_backward(gc, verts: torch.Tensor, pix_q: torch.Tensor, dL_dpix: torch.Tensor) -> torch.Tensor:
    """dL_dverts [V, 3] of dL_dpix [V, 2] through the projection of the camera struct `gc` (v3d_recon_mesh_project_bwd)"""
    lib = load_library()
    V = verts.shape[0]
    out = torch.empty(V, 3, dtype=torch.float32, device=verts.device)
    _check(lib, lib.v3d_recon_mesh_project_bwd(verts.data_ptr(), V, C.byref(gc), pix_q.data_ptr(), dL_dpix.data_ptr(), out.data_ptr(), _stream()),
           "v3d_recon_mesh_project_bwd")
    return out


def smooth_gradient(offsets: torch.Tensor, faces: torch.Tensor, ranges: torch.Tensor, corners: torch.Tensor) -> torch.Tensor:
    """The gradient [V, 3] of smooth_energy with respect to offsets [V, 3], over the corner lists (v3d_recon_mesh_smooth_grad)"""
    lib = load_library()
    V, F = offsets.shape[0], faces.shape[0]
    out = torch.empty(V, 3, dtype=torch.float32, device=offsets.device)
    _check(lib, lib.v3d_recon_mesh_smooth_grad(offsets.data_ptr(), V, faces.data_ptr(), F, ranges.data_ptr(), corners.data_ptr(), 2.0 / (3.0 * F),
                                               out.data_ptr(), _stream()), "v3d_recon_mesh_smooth_grad")
    return out


def smooth_energy_value(offsets: torch.Tensor, faces: torch.Tensor) -> torch.Tensor:
    """sum over faces and their 3 edges of |d_a - d_b|^2 / (3 F): on the deformation field, so it does not shrink the mesh"""
    d = offsets[faces.long()]                                                   # [F, 3, 3]
    e = d - d.roll(-1, 1)
    return (e * e).sum() / (3.0 * faces.shape[0])


class _Smooth(torch.autograd.Function):
    @staticmethod
    def forward(ctx, offsets, faces, ranges, corners):
        ctx.lists = (faces, ranges, corners)
        ctx.save_for_backward(offsets)
        return smooth_energy_value(offsets.detach(), faces)

    @staticmethod
    def backward(ctx, grad):
        (offsets,) = ctx.saved_tensors
        return grad * smooth_gradient(offsets.detach().contiguous(), *ctx.lists), None, None, None


def corner_lists(faces: torch.Tensor, num_verts: int):
    """(ranges [V, 2], corners [3F]) of faces [F, 3] int32 on the device: built once, the topology is fixed"""
    return _corner_lists(faces, int(num_verts))


def smooth_energy(offsets: torch.Tensor, faces: torch.Tensor, lists=None) -> torch.Tensor:
    """The edge energy of the deformation field offsets [V, 3] (float32, on the faces' device), differentiable in `offsets`"""
    ranges, corners = lists if lists is not None else corner_lists(faces, offsets.shape[0])
    return _Smooth.apply(offsets, faces, ranges, corners)


# ---- one view ---------------------------------------------------------------------------------------------------------------------------------
@torch.no_grad()
def alpha_forward(gc, verts: torch.Tensor, faces: torch.Tensor, subpixel_bits: int = 8) -> dict:
    """The forward of one view on device tensors (verts [V, 3] float32, faces [F, 3] int32, V, F >= 1): {"alpha_aa", "alpha_raw", "face_id",
    "pix_f", "pix_q", "zv"}.  Culling is on.  Without a covered pixel the antialiasing pass is not launched."""
    V = verts.shape[0]
    zv, pix_f, pix_q = project_vertices(gc, verts, subpixel_bits)
    out = rasterize_projected(gc, faces, pix_q, zv, torch.zeros(V, 3, dtype=torch.float32, device=verts.device), True, False, subpixel_bits)
    face_id = out["face_id"]
    if out["n_inst"] == 0:
        alpha, raw = torch.zeros_like(out["alpha"]), torch.zeros_like(out["alpha"])
    else:
        alpha, raw = aa_forward(face_id, faces, pix_f, pix_q)
    return {"alpha_aa": alpha, "alpha_raw": raw, "face_id": face_id, "pix_f": pix_f, "pix_q": pix_q, "zv": zv, "drawn": out["n_inst"] > 0}


@torch.no_grad()
def alpha_backward(gc, verts: torch.Tensor, faces: torch.Tensor, fwd: dict, dL_dalpha: torch.Tensor, debug: bool = False) -> dict:
    """{"dL_dverts" [V, 3], "dL_dpix" [V, 2], "records", "ranges"} of dL_dalpha [H, W] for the forward `fwd` of alpha_forward"""
    V = verts.shape[0]
    if tuple(dL_dalpha.shape) != tuple(fwd["face_id"].shape):
        raise ValueError(f"antialiased_alpha: gradient {tuple(dL_dalpha.shape)} for a view of {tuple(fwd['face_id'].shape)}")
    if not fwd["drawn"]:
        z = torch.zeros(V, 2, dtype=torch.float32, device=verts.device)
        return {"dL_dverts": torch.zeros(V, 3, dtype=torch.float32, device=verts.device), "dL_dpix": z, "records": 0,
                "ranges": torch.zeros(V, 2, dtype=torch.int32, device=verts.device)}
    out = aa_backward(fwd["face_id"], faces, fwd["pix_f"], fwd["pix_q"], fwd["alpha_raw"], dL_dalpha, debug)
    out["dL_dverts"] = project_backward(gc, verts, fwd["pix_q"], out["dL_dpix"])
    return out


class _Alpha(torch.autograd.Function):
    @staticmethod
    def forward(ctx, verts, faces, gc, bits, keep):
        v = verts.detach().contiguous()
        fwd = alpha_forward(gc, v, faces, bits)
        ctx.state = (v, faces, gc, fwd, keep)
        keep.update(face_id=fwd["face_id"], alpha_raw=fwd["alpha_raw"])
        return fwd["alpha_aa"]

    @staticmethod
    def backward(ctx, grad):
        v, faces, gc, fwd, keep = ctx.state
        out = alpha_backward(gc, v, faces, fwd, grad)
        keep.update(pairs=out["records"] // 2, ranges=out["ranges"])
        return out["dL_dverts"], None, None, None, None


class AlphaView:
    """What antialiased_alpha keeps for inspection: face_id [H, W] and alpha_raw [H, W] after the forward; pairs (the number of pairs with a
    candidate) and ranges [V, 2] (every vertex's records) after the backward."""

    def __init__(self):
        self.face_id = self.alpha_raw = self.pairs = self.ranges = None

    def update(self, **kw):
        self.__dict__.update(kw)


def antialiased_alpha(camera: Camera, verts: torch.Tensor, faces, bg=BG, subpixel_bits: int = 8, keep: AlphaView | None = None) -> torch.Tensor:
    """alpha_aa [H, W] of the mesh seen from `camera`, differentiable in verts [V, 3] (float32, on the device the faces go to).  Culling is
    on.  `keep` (an AlphaView) receives face_id and, after the backward, the pair count.  V = 0 or F = 0: zeros, without a launch."""
    H, W = int(camera.height), int(camera.width)
    _check_view(W, H, subpixel_bits)
    if not torch.is_tensor(verts) or verts.dim() != 2 or verts.shape[1] != 3 or verts.dtype != torch.float32:
        raise ValueError("antialiased_alpha: verts must be a float32 tensor [V, 3]")
    _, f, _ = _mesh_on_device(verts, faces, verts, verts.device)
    keep = keep if keep is not None else AlphaView()
    if verts.shape[0] == 0 or f.shape[0] == 0:
        keep.update(face_id=torch.full((H, W), -1, dtype=torch.int32, device=verts.device), pairs=0)
        return torch.zeros(H, W, dtype=torch.float32, device=verts.device) + 0.0 * verts.sum()
    return _Alpha.apply(verts, f, gs_camera(camera, list(bg)), int(subpixel_bits), keep)


# ---- targets ----------------------------------------------------------------------------------------------------------------------------------
@torch.no_grad()
def silhouette_targets(gaussians, cameras: Sequence[Camera], bg=BG) -> torch.Tensor:
    """[T, H, W]: the accumulated alpha of the splats from every camera (geometry.render_geometry)"""
    from .geometry import render_geometry
    bgt = torch.as_tensor(list(bg), dtype=torch.float32, device=gaussians.xyz.device)
    return torch.stack([render_geometry(cam, gaussians, bgt)["alpha"] for cam in cameras])


def alpha_from_frames(frames, white_background: bool = True, threshold: float = 0.05) -> torch.Tensor:
    """[T, H, W] float32 coverage (0 or 1) of frames (uint8 [T, H, W, 3] or float [T, 3, H, W]) when only the video is at hand: 1 where a
    pixel's largest channel distance from the background exceeds `threshold`.  Host torch code."""
    if not 0.0 <= float(threshold) < 1.0:
        raise ValueError(f"alpha_from_frames: threshold {threshold} outside 0 .. 1")
    t = frames if torch.is_tensor(frames) else torch.from_numpy(np.ascontiguousarray(frames))
    if t.dim() != 4:
        raise ValueError(f"alpha_from_frames: frames must be [T, H, W, 3] uint8 or [T, 3, H, W] float, got {tuple(t.shape)}")
    t = t.permute(0, 3, 1, 2).float() / 255.0 if t.dtype == torch.uint8 else t.float().clamp(0, 1)
    return ((t - (1.0 if white_background else 0.0)).abs().amax(1) > float(threshold)).float()


# ---- the fit ----------------------------------------------------------------------------------------------------------------------------------
@torch.no_grad()
def _silhouette_stats(v, f, gcs, alphas, bits=8):
    """(mean alpha MSE, mean IoU of face_id >= 0 against target >= 0.5) over all cameras"""
    mse, iou = [], []
    for gc, tgt in zip(gcs, alphas):
        fwd = alpha_forward(gc, v, f, bits)
        mse.append(float(((fwd["alpha_aa"] - tgt) ** 2).mean()))
        a, b = fwd["face_id"] >= 0, tgt >= 0.5
        union = int((a | b).sum())
        iou.append(int((a & b).sum()) / union if union else 1.0)
    return float(np.mean(mse)), float(np.mean(iou))


def fit_vertices(verts, faces, cameras: Sequence[Camera], alphas, *, iterations: int = ITERATIONS, lr: float = LR,
                 lambda_offset: float = LAMBDA_OFFSET, lambda_smooth: float = LAMBDA_SMOOTH, num_opt: int = 0, seed: int = 0, device="cuda"):
    """(verts' [V, 3] float32 on `device`, stats).  Per-vertex offsets d, fitted by `iterations` steps of torch.optim.Adam, one view per step
    (mesh_refine.view_schedule over mesh_refine.optimisation_views), on
        mean((alpha_aa - target)^2) + lambda_offset mean_i |d_i|^2 + lambda_smooth sum over faces and edges |d_a - d_b|^2 / (3 F).
    alphas [T, H, W]: one target per camera (silhouette_targets or alpha_from_frames).  stats: "mse_before" / "mse_after" and "iou_before" /
    "iou_after" over ALL cameras, "opt_views", "iterations", "loss_first", "loss_last", "seconds", "max_offset", "vertices_moved" (vertices
    that ever received a silhouette gradient), "pairs" (per optimisation view, at its last visit)."""
    if len(cameras) == 0:
        raise ValueError("fit_vertices: no cameras")
    tg = alphas if torch.is_tensor(alphas) else torch.from_numpy(np.ascontiguousarray(alphas))
    if tg.dim() != 3 or tg.shape[0] != len(cameras):
        raise ValueError(f"fit_vertices: {tuple(tg.shape)} alphas for {len(cameras)} cameras")
    for cam, a in zip(cameras, tg):
        if tuple(a.shape) != (int(cam.height), int(cam.width)):
            raise ValueError(f"fit_vertices: alpha {tuple(a.shape)} does not match the {cam.width} x {cam.height} camera")
        _check_view(int(cam.width), int(cam.height), 8)
    if int(iterations) != iterations or iterations < 0:
        raise ValueError(f"iterations {iterations} must not be negative")
    if not (lr >= 0 and lambda_offset >= 0 and lambda_smooth >= 0):                # (false on NaN)
        raise ValueError(f"fit_vertices: lr {lr}, lambda_offset {lambda_offset} and lambda_smooth {lambda_smooth} must not be negative")
    opt_views = optimisation_views(len(cameras), num_opt)
    v0 = _dev(verts, torch.float32, device).reshape(-1, 3)
    _, f, _ = _mesh_on_device(v0, faces, v0, device)
    V, F = v0.shape[0], f.shape[0]
    stats = {"opt_views": opt_views, "iterations": int(iterations), "loss_first": None, "loss_last": None, "max_offset": 0.0, "vertices_moved": 0,
             "pairs": [], "seconds": 0.0, "mse_before": None, "mse_after": None, "iou_before": None, "iou_after": None}
    if V == 0 or F == 0:
        return v0, stats
    tg = tg.to(device=device, dtype=torch.float32).contiguous()
    gcs = [gs_camera(cam, list(BG)) for cam in cameras]
    stats["mse_before"], stats["iou_before"] = _silhouette_stats(v0, f, gcs, tg)
    t0 = time.perf_counter()
    d = torch.zeros_like(v0, requires_grad=True)
    moved = torch.zeros(V, dtype=torch.bool, device=v0.device)
    pairs = {}
    if iterations:
        lists = corner_lists(f, V)
        opt = torch.optim.Adam([d], lr=float(lr))
        with torch.enable_grad():                  # (a caller may have switched autograd off)
            for it, j in enumerate(view_schedule(len(opt_views), iterations, seed)):
                i = opt_views[j]
                keep = AlphaView()
                opt.zero_grad(set_to_none=True)
                alpha = _Alpha.apply(v0 + d, f, gcs[i], 8, keep)
                diff = alpha - tg[i]
                loss = (diff * diff).mean() + float(lambda_offset) * (d * d).sum(1).mean() + float(lambda_smooth) * smooth_energy(d, f, lists)
                loss.backward()
                opt.step()
                moved |= keep.ranges[:, 1] > keep.ranges[:, 0]
                pairs[i] = keep.pairs
                if it == 0:
                    first = loss.detach()
                last = loss.detach()
        stats["loss_first"], stats["loss_last"] = float(first), float(last)
    out = (v0 + d.detach()).contiguous()
    if v0.device.type == "cuda":
        torch.cuda.synchronize()
    stats["seconds"] = time.perf_counter() - t0
    stats["max_offset"] = float(d.detach().norm(dim=1).max())
    stats["vertices_moved"] = int(moved.sum())
    stats["pairs"] = [int(pairs.get(i, 0)) for i in opt_views]
    stats["mse_after"], stats["iou_after"] = _silhouette_stats(out, f, gcs, tg)
    return out, stats
