"""Refine the vertex colours of the extracted mesh against the orbit it was built from, on the gfx950 kernels of libv3d_recon.so
(csrc_recon/meshshade.hip, include/v3d_recon.h "Mesh colour refinement"): the last step of the reference's pipeline (mesh_recon/refine.py).

    view = prepare_view(cam, verts, faces, bg)                 # rasterize once, freeze what the camera sees
    image = shade(view, colors)                                # [3, H, W], differentiable in colors [V, 3]
    colors, stats = refine_vertex_colors(verts, faces, colors, cameras, images)

The geometry is fixed, so visibility per camera never changes: every optimisation view is rasterized once by mesh_render.py's forward and
frozen into three vertex indices and three weights per pixel.  The image is then a sparse linear map of the colours (a gather per pixel)
and its gradient the transpose (a gather per vertex over lists built once with v3d_gs_scan and v3d_gs_radix_sort_pairs).  No atomics: two
calls with the same arguments return bit-equal colours.  There is no fallback: without the libraries this raises."""
from __future__ import annotations

import dataclasses
import time
from typing import Sequence

import numpy as np
import torch

from ..ops import get_ops
from .cameras import Camera
from .geometry import _check, _stream, load_library
from .mesh_render import _bg, _check_view, _dev, _frames, _mesh_on_device, mesh_fidelity, project_vertices, rasterize_projected
from .rasterize import gs_camera

COLOR_CLAMP = 0.5 / 255.0          # the PLY stores 8 bits: half a step keeps the logits of 0 and 255 finite
BETAS, EPS = (0.9, 0.999), 1e-8    # torch.optim.Adam's defaults, as the reference uses them


@dataclasses.dataclass
class MeshView:
    """What one camera sees of a fixed mesh.  depth, alpha [H, W] and face_id [H, W] (int32) are the forward's; pix_vert [H, W, 3] (int32, -1
    where nothing covers) and pix_w [H, W, 3] its winner's vertices and b_k / zv_k; ranges [V, 2] (int32) every vertex's [start, end) in
    ent_pix [n] (int32 pixel) / ent_w [n] (depth x weight), ascending in the pixel; bg [3].  `launch` is False for a mesh with V = 0 or F = 0."""
    width: int
    height: int
    num_verts: int
    depth: torch.Tensor
    alpha: torch.Tensor
    face_id: torch.Tensor
    pix_vert: torch.Tensor
    pix_w: torch.Tensor
    ranges: torch.Tensor
    ent_pix: torch.Tensor
    ent_w: torch.Tensor
    bg: torch.Tensor
    bg_values: tuple = (0.0, 0.0, 0.0)      # bg on the host (a launch argument: no read-back per shade)
    launch: bool = True


def pixel_weights(face_id: torch.Tensor, faces: torch.Tensor, pix_q: torch.Tensor, zv: torch.Tensor, subpixel_bits: int = 8):
    """(pix_vert [H, W, 3] int32, pix_w [H, W, 3]) of a face_id map [H, W] and the faces, snapped positions and view z it was rendered from"""
    lib = load_library()
    H, W = face_id.shape
    pix_vert = torch.empty(H, W, 3, dtype=torch.int32, device=face_id.device)
    pix_w = torch.empty(H, W, 3, dtype=torch.float32, device=face_id.device)
    _check(lib, lib.v3d_recon_mesh_pixel_weights(face_id.data_ptr(), faces.data_ptr(), faces.shape[0], pix_q.data_ptr(), zv.data_ptr(), zv.shape[0],
                                                 W, H, int(subpixel_bits), pix_vert.data_ptr(), pix_w.data_ptr(), _stream()),
           "v3d_recon_mesh_pixel_weights")
    return pix_vert, pix_w


def vertex_lists(pix_vert: torch.Tensor, pix_w: torch.Tensor, depth: torch.Tensor, num_verts: int):
    """(ranges [V, 2], ent_pix [n], ent_w [n]): the transpose of the per-pixel records, every vertex's entries in ascending pixel order"""
    lib, ops = load_library(), get_ops()
    dev = pix_vert.device
    H, W = depth.shape
    V = int(num_verts)
    covered = (pix_vert[:, :, 0] >= 0).reshape(-1).to(torch.int32).contiguous()
    offsets = ops.gs_scan(covered)
    n = 3 * int(offsets[-1].item())          # (at most 3 x 4096^2: fits int32)
    ranges = torch.empty(V, 2, dtype=torch.int32, device=dev)
    if n == 0:
        _check(lib, lib.v3d_recon_mesh_vertex_ranges(None, 0, V, ranges.data_ptr(), _stream()), "v3d_recon_mesh_vertex_ranges")
        return ranges, torch.zeros(0, dtype=torch.int32, device=dev), torch.zeros(0, dtype=torch.float32, device=dev)
    keys = torch.empty(n, dtype=torch.int64, device=dev)
    vals = torch.empty(n, dtype=torch.int32, device=dev)
    _check(lib, lib.v3d_recon_mesh_vertex_records(pix_vert.data_ptr(), offsets.data_ptr(), W, H, n, keys.data_ptr(), vals.data_ptr(), _stream()),
           "v3d_recon_mesh_vertex_records")
    keys_s, vals_s = ops.gs_radix_sort_pairs(keys, vals, max(1, (V - 1).bit_length()))
    _check(lib, lib.v3d_recon_mesh_vertex_ranges(keys_s.data_ptr(), n, V, ranges.data_ptr(), _stream()), "v3d_recon_mesh_vertex_ranges")
    rec = vals_s.long()
    ent_pix = torch.div(rec, 3, rounding_mode="floor")
    ent_w = (depth.reshape(-1)[ent_pix] * pix_w.reshape(-1)[rec]).contiguous()
    return ranges, ent_pix.to(torch.int32).contiguous(), ent_w


def _host_bg(bg, device):
    bgh = torch.as_tensor(bg, dtype=torch.float32).reshape(3).cpu()
    return bgh.to(device), tuple(bgh.tolist())


@torch.no_grad()
def freeze_projected(gc, faces: torch.Tensor, pix_q: torch.Tensor, zv: torch.Tensor, bg, cull: bool = True, subpixel_bits: int = 8) -> MeshView:
    """The view of already projected vertices (project_vertices: pix_q [V, 2], zv [V]; faces [F, 3] int32, F >= 1; all on the device):
    rasterize once, then the per-pixel record and the per-vertex lists"""
    V = zv.shape[0]
    out = rasterize_projected(gc, faces, pix_q, zv, torch.zeros(V, 3, dtype=torch.float32, device=zv.device), cull, False, subpixel_bits)
    pix_vert, pix_w = pixel_weights(out["face_id"], faces, pix_q, zv, subpixel_bits)       # (the colours above do not matter: only the maps are kept)
    ranges, ent_pix, ent_w = vertex_lists(pix_vert, pix_w, out["depth"], V)
    bgt, bgv = _host_bg(bg, zv.device)
    return MeshView(int(gc.width), int(gc.height), V, out["depth"], out["alpha"], out["face_id"], pix_vert, pix_w, ranges, ent_pix, ent_w, bgt, bgv)


@torch.no_grad()
def prepare_view(camera: Camera, verts, faces, bg, cull: bool = True, subpixel_bits: int = 8, device="cuda") -> MeshView:
    """Rasterize the mesh once from `camera` and freeze the result.  verts [V, 3], faces [F, 3] (integers): tensors or numpy arrays."""
    H, W = int(camera.height), int(camera.width)
    _check_view(W, H, subpixel_bits)
    v = _dev(verts, torch.float32, device).reshape(-1, 3)
    _, f, _ = _mesh_on_device(v, faces, v, device)
    V = v.shape[0]
    if V == 0 or f.shape[0] == 0:          # nothing to draw: the background, without a launch (the kernels take V, F >= 1)
        z = lambda *s, dt=torch.float32: torch.zeros(*s, dtype=dt, device=device)  # noqa: E731
        return MeshView(W, H, V, z(H, W), z(H, W), torch.full((H, W), -1, dtype=torch.int32, device=device),
                        torch.full((H, W, 3), -1, dtype=torch.int32, device=device), z(H, W, 3), z(V, 2, dt=torch.int32), z(0, dt=torch.int32), z(0),
                        *_host_bg(bg, device), launch=False)
    gc = gs_camera(camera, bg)
    zv, _, pix_q = project_vertices(gc, v, subpixel_bits)
    return freeze_projected(gc, f, pix_q, zv, bg, cull, subpixel_bits)


def _colors_ok(view: MeshView, colors: torch.Tensor) -> torch.Tensor:
    if tuple(colors.shape) != (view.num_verts, 3):
        raise ValueError(f"shade: colours {tuple(colors.shape)} for a view of {view.num_verts} vertices")
    if colors.dtype != torch.float32 or colors.device != view.depth.device:
        raise ValueError(f"shade: expected float32 colours on {view.depth.device}, got {colors.dtype} on {colors.device}")
    return colors.contiguous()


def shade_forward(view: MeshView, colors: torch.Tensor) -> torch.Tensor:
    """image [3, H, W] of colors [V, 3] (v3d_recon_mesh_shade), outside autograd"""
    H, W = view.height, view.width
    if not view.launch:
        return view.bg.view(3, 1, 1).expand(3, H, W).contiguous()
    c = _colors_ok(view, colors.detach())
    lib = load_library()
    image = torch.empty(3, H, W, dtype=torch.float32, device=c.device)
    bg = view.bg_values
    _check(lib, lib.v3d_recon_mesh_shade(view.pix_vert.data_ptr(), view.pix_w.data_ptr(), view.depth.data_ptr(), c.data_ptr(), view.num_verts, W, H,
                                         bg[0], bg[1], bg[2], image.data_ptr(), _stream()), "v3d_recon_mesh_shade")
    return image


def shade_backward(view: MeshView, dL_dimage: torch.Tensor) -> torch.Tensor:
    """dL_dcolors [V, 3] of dL_dimage [3, H, W] (v3d_recon_mesh_shade_bwd), outside autograd"""
    H, W, V = view.height, view.width, view.num_verts
    dev = view.depth.device
    if tuple(dL_dimage.shape) != (3, H, W):
        raise ValueError(f"shade: gradient {tuple(dL_dimage.shape)} for a {W} x {H} view")
    if not view.launch or V == 0:
        return torch.zeros(V, 3, dtype=torch.float32, device=dev)
    g = dL_dimage.detach().to(device=dev, dtype=torch.float32).contiguous()
    lib = load_library()
    out = torch.empty(V, 3, dtype=torch.float32, device=dev)
    n = view.ent_pix.numel()
    _check(lib, lib.v3d_recon_mesh_shade_bwd(view.ranges.data_ptr(), view.ent_pix.data_ptr() if n else None, view.ent_w.data_ptr() if n else None, n,
                                             g.data_ptr(), W, H, V, out.data_ptr(), _stream()), "v3d_recon_mesh_shade_bwd")
    return out


class _Shade(torch.autograd.Function):
    @staticmethod
    def forward(ctx, colors, view):
        ctx.view = view
        return shade_forward(view, colors)

    @staticmethod
    def backward(ctx, grad):
        return shade_backward(ctx.view, grad), None


def shade(view: MeshView, colors: torch.Tensor) -> torch.Tensor:
    """The image [3, H, W] the view's camera sees of the mesh with colors [V, 3] (float32, on the view's device); differentiable in `colors`."""
    if view.launch:
        _colors_ok(view, colors)
    return _Shade.apply(colors, view)


def color_adam(logit: torch.Tensor, m: torch.Tensor, v: torch.Tensor, grad: torch.Tensor, colors: torch.Tensor, step: int, lr: float,
               betas=BETAS, eps: float = EPS):
    """One torch.optim.Adam step on logit [V, 3] (in place, with its moments m, v) from grad = dL/dcolors, colors = sigmoid(logit) written anew"""
    lib = load_library()
    for t in (logit, m, v, grad, colors):
        if t.shape != logit.shape or t.dtype != torch.float32 or not t.is_contiguous() or t.device != logit.device:
            raise ValueError("color_adam: logit, m, v, grad and colors must be contiguous float32 tensors of one shape on one device")
    if logit.dim() != 2 or logit.shape[1] != 3 or logit.shape[0] == 0:
        raise ValueError(f"color_adam: expected [V, 3] with V >= 1, got {tuple(logit.shape)}")
    _check(lib, lib.v3d_recon_mesh_color_adam(logit.data_ptr(), m.data_ptr(), v.data_ptr(), grad.data_ptr(), logit.shape[0], float(lr), float(betas[0]),
                                              float(betas[1]), float(eps), int(step), colors.data_ptr(), _stream()), "v3d_recon_mesh_color_adam")


def optimisation_views(num_views: int, num_opt: int) -> list:
    """The reference's choice: num_opt evenly spaced views, linspace(0, T, num_opt + 1)[:num_opt] as integers; num_opt = 0 means every view."""
    if num_opt < 0:
        raise ValueError(f"num_opt {num_opt} must not be negative")
    if num_opt == 0:
        return list(range(num_views))
    return [int(i) for i in np.linspace(0, num_views, num_opt + 1)[:num_opt].astype(int)]


def view_schedule(num_opt_views: int, iterations: int, seed: int) -> list:
    """Which optimisation view (a position in optimisation_views) every iteration uses: drawn once from a generator seeded with `seed`"""
    g = torch.Generator().manual_seed(int(seed))
    return torch.randint(num_opt_views, (int(iterations),), generator=g).tolist() if iterations > 0 else []


def initial_logits(colors: torch.Tensor) -> torch.Tensor:
    c = colors.clamp(COLOR_CLAMP, 1.0 - COLOR_CLAMP)
    return torch.log(c / (1.0 - c))


@torch.no_grad()
def refine_vertex_colors(verts, faces, colors, cameras: Sequence[Camera], images, *, iterations: int = 2000, lr: float = 1e-3, num_opt: int = 4,
                         white_background: bool = True, seed: int = 0, device="cuda"):
    """(colors [V, 3] float32 on `device`, stats).  The vertex colours that best reproduce `images` (uint8 [T, H, W, 3] or float [T, 3, H, W],
    one per camera) from num_opt evenly spaced cameras, by `iterations` Adam steps on the colours' logits, one view per step, mean squared
    error over the whole image.  A vertex that no optimisation view sees keeps its colour.  stats: "psnr_before" / "psnr_after" (mesh_fidelity's
    psnr_mean over ALL cameras), "opt_views", "loss_first", "loss_last", "seconds", "iterations", "vertices_seen"."""
    gt = _frames(images, device)
    if gt.shape[0] != len(cameras):
        raise ValueError(f"refine_vertex_colors: {gt.shape[0]} images for {len(cameras)} cameras")
    for cam, frame in zip(cameras, gt):
        if tuple(frame.shape) != (3, int(cam.height), int(cam.width)):
            raise ValueError(f"refine_vertex_colors: frame {tuple(frame.shape)} does not match the {cam.width} x {cam.height} camera")
        _check_view(int(cam.width), int(cam.height), 8)
    if iterations < 0:
        raise ValueError(f"iterations {iterations} must not be negative")
    v, f, c0 = _mesh_on_device(verts, faces, colors, device)
    bg = _bg(white_background)
    opt = optimisation_views(len(cameras), num_opt)
    V = v.shape[0]
    stats = {"opt_views": opt, "iterations": int(iterations), "loss_first": None, "loss_last": None}
    stats["psnr_before"] = mesh_fidelity(v, f, c0, cameras, gt, bg, device)["psnr_mean"]
    t0 = time.perf_counter()
    out, seen = c0.clone(), torch.zeros(V, dtype=torch.bool, device=device)
    if V and f.shape[0] and opt and iterations:
        views = [prepare_view(cameras[i], v, f, bg, True, 8, device) for i in opt]
        targets = [gt[i].contiguous() for i in opt]
        for view in views:
            seen |= view.ranges[:, 1] > view.ranges[:, 0]
        logit = initial_logits(c0).contiguous()
        cur = torch.sigmoid(logit)
        m, s, first, last = torch.zeros_like(logit), torch.zeros_like(logit), None, None
        for it, j in enumerate(view_schedule(len(opt), iterations, seed)):
            diff = shade_forward(views[j], cur) - targets[j]
            if it == 0:
                first = (diff * diff).mean()
            if it == iterations - 1:
                last = (diff * diff).mean()
            grad = shade_backward(views[j], diff * (2.0 / diff.numel()))
            color_adam(logit, m, s, grad, cur, it + 1, lr)
        out = torch.where(seen[:, None], cur, c0)
        stats["loss_first"], stats["loss_last"] = float(first), float(last)
    if device != "cpu" and torch.cuda.is_available():
        torch.cuda.synchronize()
    stats["seconds"] = time.perf_counter() - t0
    stats["vertices_seen"] = int(seen.sum())
    stats["psnr_after"] = mesh_fidelity(v, f, out, cameras, gt, bg, device)["psnr_mean"]
    return out, stats
