"""Texture the decimated mesh against the orbit it was built from, on the gfx950 kernels of libv3d_recon.so (csrc_recon/meshtex.hip,
include/v3d_recon.h "Mesh texture"): what the reference's fit_mesh_uv / export_mesh do after decimation, with a closed-form atlas.

    vt = face_uvs(F, R)                                           # [F, 3, 2] texel coordinates, by the face index alone
    owner, texture = bake_vertex_colors(faces, colors, R)         # the initial albedo [R*R, 3]
    view = prepare_texture_view(cam, verts, faces, R, bg)         # rasterize once, freeze four texels and weights per pixel
    image = texture_shade(view, texture)                          # [3, H, W], differentiable in texture
    texture, stats = fit_texture(verts, faces, colors, cameras, images, tex_size=1024)
    save_textured_obj("mesh.obj", verts, faces, vt, texture)      # + mesh.mtl, mesh.png

The method of mesh_refine.py with texels in the place of vertices: the geometry is fixed, so every view is rasterized once, the image is a
gather per pixel and its gradient the transposed gather per texel over lists built once.  No atomics: two calls with the same arguments
return bit-equal textures.  There is no fallback: without the libraries this raises."""
from __future__ import annotations

import dataclasses
import math
import os
import time
from typing import Sequence

import numpy as np
import torch

from ..ops import get_ops
from .cameras import Camera, orbit_cameras
from .geometry import _check, _stream, load_library
from .mesh_refine import COLOR_CLAMP, _host_bg, color_adam, initial_logits, optimisation_views, pixel_weights, view_schedule  # noqa: F401
from .mesh_render import _bg, _check_view, _dev, _frames, _mesh_on_device, mesh_fidelity, project_vertices, rasterize_projected
from .rasterize import gs_camera

MAX_TEX_SIZE = 4096
MIN_CELL = 4
FILL = 0.5          # unowned texels, and the faces whose indices are not vertices


def atlas_layout(num_faces: int, tex_size: int):
    """(S, g): cell size and cells per row of the per-face atlas of F faces in an R x R texture.  g = ceil(sqrt(ceil(F / 2))), S = R // g."""
    F, R = int(num_faces), int(tex_size)
    if F < 1:
        raise ValueError(f"atlas_layout: {F} faces")
    if not 1 <= R <= MAX_TEX_SIZE:
        raise ValueError(f"atlas_layout: tex_size {R} outside 1 .. {MAX_TEX_SIZE}")
    cells = (F + 1) // 2
    g = math.isqrt(cells - 1) + 1 if cells > 1 else 1          # the smallest g with g g >= cells
    S = R // g
    if S < MIN_CELL:
        raise ValueError(f"texture too small for {F} faces: {R} x {R} leaves cells of {S} texels, below {MIN_CELL}")
    return S, g


@torch.no_grad()
def face_uvs(num_faces: int, tex_size: int, device="cuda") -> torch.Tensor:
    """vt [F, 3, 2] float32: the UV corners of every face in texels (v3d_recon_tex_face_uvs)"""
    F, R = int(num_faces), int(tex_size)
    if F == 0:
        return torch.zeros(0, 3, 2, dtype=torch.float32, device=device)
    atlas_layout(F, R)
    lib = load_library()
    vt = torch.empty(F, 3, 2, dtype=torch.float32, device=device)
    _check(lib, lib.v3d_recon_tex_face_uvs(F, R, vt.data_ptr(), _stream()), "v3d_recon_tex_face_uvs")
    return vt


@torch.no_grad()
def bake_vertex_colors(faces, colors, tex_size: int, device="cuda"):
    """(owner [R*R] int32, texture [R*R, 3] float32): every texel's face (-1: unowned) and the vertex colours interpolated over the charts"""
    R = int(tex_size)
    if not 1 <= R <= MAX_TEX_SIZE:
        raise ValueError(f"bake_vertex_colors: tex_size {R} outside 1 .. {MAX_TEX_SIZE}")
    c = _dev(colors, torch.float32, device).reshape(-1, 3)
    f = _dev(faces, torch.int32, device).reshape(-1, 3)
    F, V = f.shape[0], c.shape[0]
    if F == 0 or V == 0:
        return torch.full((R * R,), -1, dtype=torch.int32, device=device), torch.full((R * R, 3), FILL, dtype=torch.float32, device=device)
    atlas_layout(F, R)
    lib = load_library()
    owner = torch.empty(R * R, dtype=torch.int32, device=device)
    texture = torch.empty(R * R, 3, dtype=torch.float32, device=device)
    _check(lib, lib.v3d_recon_tex_bake_vertex_colors(f.data_ptr(), F, c.data_ptr(), V, R, FILL, owner.data_ptr(), texture.data_ptr(), _stream()),
           "v3d_recon_tex_bake_vertex_colors")
    return owner, texture


@dataclasses.dataclass
class TextureView:
    """What one camera sees of a fixed mesh through its atlas.  face_id, alpha [H, W] are the forward's; pix_tex [H, W, 4] (int32 texel
    indices, -1 where nothing covers) and pix_tw [H, W, 4] the bilinear taps of every pixel; ranges [R*R, 2] (int32) every texel's
    [start, end) in ent_pix [n] (int32 pixel) / ent_w [n], ascending in 4 pixel + tap (None when the view was prepared without lists);
    bg [3].  `launch` is False for a mesh with V = 0 or F = 0."""
    width: int
    height: int
    tex_size: int
    num_faces: int
    face_id: torch.Tensor
    alpha: torch.Tensor
    pix_tex: torch.Tensor
    pix_tw: torch.Tensor
    ranges: torch.Tensor
    ent_pix: torch.Tensor
    ent_w: torch.Tensor
    bg: torch.Tensor
    bg_values: tuple = (0.0, 0.0, 0.0)
    launch: bool = True


def pixel_texels(face_id: torch.Tensor, pix_w: torch.Tensor, num_faces: int, tex_size: int):
    """(pix_tex [H, W, 4] int32, pix_tw [H, W, 4]) of a face_id map [H, W] and the pix_w [H, W, 3] of pixel_weights of the same view"""
    lib = load_library()
    H, W = face_id.shape
    pix_tex = torch.empty(H, W, 4, dtype=torch.int32, device=face_id.device)
    pix_tw = torch.empty(H, W, 4, dtype=torch.float32, device=face_id.device)
    _check(lib, lib.v3d_recon_tex_pixel_texels(face_id.data_ptr(), pix_w.data_ptr(), int(num_faces), int(tex_size), W, H, pix_tex.data_ptr(),
                                               pix_tw.data_ptr(), _stream()), "v3d_recon_tex_pixel_texels")
    return pix_tex, pix_tw


def texel_lists(pix_tex: torch.Tensor, pix_tw: torch.Tensor, tex_size: int):
    """(ranges [R*R, 2], ent_pix [n], ent_w [n]): the transpose of the per-pixel taps, every texel's entries in ascending 4 pixel + tap"""
    lib, ops = load_library(), get_ops()
    dev = pix_tex.device
    H, W = pix_tex.shape[:2]
    T = int(tex_size) ** 2
    covered = (pix_tex[:, :, 0] >= 0).reshape(-1).to(torch.int32).contiguous()
    offsets = ops.gs_scan(covered)
    n = 4 * int(offsets[-1].item())          # (at most 4 x 4096^2: fits int32)
    ranges = torch.empty(T, 2, dtype=torch.int32, device=dev)
    if n == 0:
        _check(lib, lib.v3d_recon_mesh_vertex_ranges(None, 0, T, ranges.data_ptr(), _stream()), "v3d_recon_mesh_vertex_ranges")
        return ranges, torch.zeros(0, dtype=torch.int32, device=dev), torch.zeros(0, dtype=torch.float32, device=dev)
    keys = torch.empty(n, dtype=torch.int64, device=dev)
    vals = torch.empty(n, dtype=torch.int32, device=dev)
    _check(lib, lib.v3d_recon_tex_texel_records(pix_tex.data_ptr(), offsets.data_ptr(), W, H, n, keys.data_ptr(), vals.data_ptr(), _stream()),
           "v3d_recon_tex_texel_records")
    keys_s, vals_s = ops.gs_radix_sort_pairs(keys, vals, max(1, (T - 1).bit_length()))
    _check(lib, lib.v3d_recon_mesh_vertex_ranges(keys_s.data_ptr(), n, T, ranges.data_ptr(), _stream()), "v3d_recon_mesh_vertex_ranges")
    rec = vals_s.long()
    ent_pix = torch.div(rec, 4, rounding_mode="floor").to(torch.int32).contiguous()
    return ranges, ent_pix, pix_tw.reshape(-1)[rec].contiguous()


@torch.no_grad()
def prepare_texture_view(camera: Camera, verts, faces, tex_size: int, bg, cull: bool = True, subpixel_bits: int = 8, lists: bool = True,
                         device="cuda") -> TextureView:
    """Rasterize the mesh once from `camera` and freeze every pixel's four texels and weights; with `lists` also the per-texel lists the
    gradient needs.  verts [V, 3], faces [F, 3] (integers): tensors or numpy arrays."""
    H, W, R = int(camera.height), int(camera.width), int(tex_size)
    _check_view(W, H, subpixel_bits)
    if not 1 <= R <= MAX_TEX_SIZE:
        raise ValueError(f"prepare_texture_view: tex_size {R} outside 1 .. {MAX_TEX_SIZE}")
    v = _dev(verts, torch.float32, device).reshape(-1, 3)
    _, f, _ = _mesh_on_device(v, faces, v, device)
    V, F = v.shape[0], f.shape[0]
    bgt, bgv = _host_bg(bg, device)
    if V == 0 or F == 0:          # nothing to draw: the background, without a launch (the kernels take V, F >= 1)
        z = lambda *s, dt=torch.float32: torch.zeros(*s, dtype=dt, device=device)  # noqa: E731
        return TextureView(W, H, R, F, torch.full((H, W), -1, dtype=torch.int32, device=device), z(H, W),
                           torch.full((H, W, 4), -1, dtype=torch.int32, device=device), z(H, W, 4), z(R * R, 2, dt=torch.int32), z(0, dt=torch.int32),
                           z(0), bgt, bgv, launch=False)
    atlas_layout(F, R)
    gc = gs_camera(camera, bg)
    zv, _, pix_q = project_vertices(gc, v, subpixel_bits)
    out = rasterize_projected(gc, f, pix_q, zv, torch.zeros(V, 3, dtype=torch.float32, device=device), cull, False, subpixel_bits)
    _, pix_w = pixel_weights(out["face_id"], f, pix_q, zv, subpixel_bits)
    pix_tex, pix_tw = pixel_texels(out["face_id"], pix_w, F, R)
    ranges, ent_pix, ent_w = texel_lists(pix_tex, pix_tw, R) if lists else (None, None, None)
    return TextureView(W, H, R, F, out["face_id"], out["alpha"], pix_tex, pix_tw, ranges, ent_pix, ent_w, bgt, bgv)


def _texture_ok(view: TextureView, texture: torch.Tensor) -> torch.Tensor:
    T = view.tex_size ** 2
    if tuple(texture.shape) != (T, 3):
        raise ValueError(f"texture_shade: texture {tuple(texture.shape)} for a view of {view.tex_size} x {view.tex_size} texels")
    if texture.dtype != torch.float32 or texture.device != view.pix_tex.device:
        raise ValueError(f"texture_shade: expected a float32 texture on {view.pix_tex.device}, got {texture.dtype} on {texture.device}")
    return texture.contiguous()


def texture_shade_forward(view: TextureView, texture: torch.Tensor) -> torch.Tensor:
    """image [3, H, W] of texture [R*R, 3] (v3d_recon_tex_shade), outside autograd"""
    H, W = view.height, view.width
    if not view.launch:
        return view.bg.view(3, 1, 1).expand(3, H, W).contiguous()
    t = _texture_ok(view, texture.detach())
    lib = load_library()
    image = torch.empty(3, H, W, dtype=torch.float32, device=t.device)
    bg = view.bg_values
    _check(lib, lib.v3d_recon_tex_shade(view.pix_tex.data_ptr(), view.pix_tw.data_ptr(), t.data_ptr(), view.tex_size, W, H, bg[0], bg[1], bg[2],
                                        image.data_ptr(), _stream()), "v3d_recon_tex_shade")
    return image


def _list_sum(lib, ranges, ent_pix, ent_w, n, grad, W, H, T, out):
    """The one place that decides the order a texel's list is added in: front to back by v3d_recon_tex_shade_bwd (a thread per texel)."""
    return lib.v3d_recon_tex_shade_bwd(ranges, ent_pix, ent_w, n, grad, W, H, T, out, _stream())


def texture_shade_backward(view: TextureView, dL_dimage: torch.Tensor) -> torch.Tensor:
    """dL_dtexture [R*R, 3] of dL_dimage [3, H, W] (v3d_recon_tex_shade_bwd), outside autograd"""
    H, W, T = view.height, view.width, view.tex_size ** 2
    dev = view.pix_tex.device
    if tuple(dL_dimage.shape) != (3, H, W):
        raise ValueError(f"texture_shade: gradient {tuple(dL_dimage.shape)} for a {W} x {H} view")
    if not view.launch:
        return torch.zeros(T, 3, dtype=torch.float32, device=dev)
    if view.ranges is None:
        raise ValueError("texture_shade: the view was prepared without lists (prepare_texture_view(..., lists=False))")
    g = dL_dimage.detach().to(device=dev, dtype=torch.float32).contiguous()
    lib = load_library()
    out = torch.empty(T, 3, dtype=torch.float32, device=dev)
    n = view.ent_pix.numel()
    _check(lib, _list_sum(lib, view.ranges.data_ptr(), view.ent_pix.data_ptr() if n else None, view.ent_w.data_ptr() if n else None, n, g.data_ptr(),
                          W, H, T, out.data_ptr()), "v3d_recon_tex_shade_bwd")
    return out


class _TextureShade(torch.autograd.Function):
    @staticmethod
    def forward(ctx, texture, view):
        ctx.view = view
        return texture_shade_forward(view, texture)

    @staticmethod
    def backward(ctx, grad):
        return texture_shade_backward(ctx.view, grad), None


def texture_shade(view: TextureView, texture: torch.Tensor) -> torch.Tensor:
    """The image [3, H, W] the view's camera sees of the mesh with texture [R*R, 3] (float32, on the view's device); differentiable in it."""
    _texture_ok(view, texture)
    return _TextureShade.apply(texture, view)


def _psnr_views(views, texture, gt) -> float:
    from .train import psnr
    ps = [psnr(texture_shade_forward(vw, texture).clamp(0, 1), frame) for vw, frame in zip(views, gt)]
    return float(np.mean(ps)) if ps else float("nan")


@torch.no_grad()
def textured_fidelity(verts, faces, texture, cameras: Sequence[Camera], images, bg, device="cuda") -> dict:
    """{"psnr": per view, "psnr_mean"} of the textured mesh (culling on, clamped to 0 .. 1) against `images`, as mesh_fidelity reports"""
    from .train import psnr
    gt = _frames(images, device)
    if gt.shape[0] != len(cameras):
        raise ValueError(f"textured_fidelity: {gt.shape[0]} images for {len(cameras)} cameras")
    tex = _dev(texture, torch.float32, device).reshape(-1, 3)
    R = math.isqrt(tex.shape[0])
    if R * R != tex.shape[0]:
        raise ValueError(f"textured_fidelity: {tex.shape[0]} texels are not a square")
    ps = [psnr(texture_shade_forward(prepare_texture_view(cam, verts, faces, R, bg, lists=False, device=device), tex).clamp(0, 1), frame)
          for cam, frame in zip(cameras, gt)]
    return {"psnr": ps, "psnr_mean": float(np.mean(ps)) if ps else float("nan")}


@torch.no_grad()
def render_textured_orbit(verts, faces, texture, n: int, radius: float, elevation: float, fov: float, reso: int, white_background: bool = True,
                          cull: bool = True, device="cuda") -> np.ndarray:
    """n turntable frames of the textured mesh, uint8 [n, reso, reso, 3] on the host (as mesh_render.render_mesh_orbit)"""
    cams, _ = orbit_cameras(n, radius, elevation, fov, reso)
    tex = _dev(texture, torch.float32, device).reshape(-1, 3)
    R = math.isqrt(tex.shape[0])
    out = []
    for cam in cams:
        img = texture_shade_forward(prepare_texture_view(cam, verts, faces, R, _bg(white_background), cull, lists=False, device=device), tex)
        out.append((img.clamp(0, 1) * 255).to(torch.uint8).permute(1, 2, 0).cpu())
    return torch.stack(out).numpy()


def list_statistics(views: Sequence[TextureView]) -> dict:
    """Over the views' non-empty texel lists: median and longest length, and the share of texels that any list holds"""
    lens, seen = [], None
    for vw in views:
        n = (vw.ranges[:, 1] - vw.ranges[:, 0]).long()
        lens.append(n[n > 0])
        seen = (n > 0) if seen is None else seen | (n > 0)
    lens = torch.cat(lens) if lens else torch.zeros(0, dtype=torch.long)
    if lens.numel() == 0:
        return {"list_median": 0, "list_longest": 0, "texels_seen_share": 0.0}
    return {"list_median": int(lens.median()), "list_longest": int(lens.max()), "texels_seen_share": float(seen.float().mean())}


@torch.no_grad()
def fit_texture(verts, faces, colors, cameras: Sequence[Camera], images, *, tex_size: int = 1024, iterations: int = 2000, lr: float = 1e-3,
                num_opt: int = 0, white_background: bool = True, seed: int = 0, device="cuda"):
    """(texture [R*R, 3] float32 on `device`, stats).  The texture of the per-face atlas that best reproduces `images` (uint8 [T, H, W, 3] or
    float [T, 3, H, W], one per camera): baked from the vertex colours, then `iterations` Adam steps on the texels' logits, one view per
    step, mean squared error over the whole image, against num_opt evenly spaced cameras (0, the default: all of them).  A texel that no
    optimisation view samples keeps its baked value bit for bit.  stats: "psnr_vertex" (mesh_fidelity of the vertex colours), "psnr_baked",
    "psnr_fitted" (all means over ALL cameras), "opt_views", "texels_seen", "loss_first", "loss_last", "seconds", "iterations", "tex_size",
    "cell"."""
    gt = _frames(images, device)
    if gt.shape[0] != len(cameras):
        raise ValueError(f"fit_texture: {gt.shape[0]} images for {len(cameras)} cameras")
    for cam, frame in zip(cameras, gt):
        if tuple(frame.shape) != (3, int(cam.height), int(cam.width)):
            raise ValueError(f"fit_texture: frame {tuple(frame.shape)} does not match the {cam.width} x {cam.height} camera")
        _check_view(int(cam.width), int(cam.height), 8)
    if iterations < 0:
        raise ValueError(f"iterations {iterations} must not be negative")
    R = int(tex_size)
    if not 1 <= R <= MAX_TEX_SIZE:
        raise ValueError(f"fit_texture: tex_size {R} outside 1 .. {MAX_TEX_SIZE}")
    v, f, c0 = _mesh_on_device(verts, faces, colors, device)
    V, F = v.shape[0], f.shape[0]
    cell = atlas_layout(F, R)[0] if F else 0
    bg = _bg(white_background)
    opt = optimisation_views(len(cameras), num_opt)
    stats = {"opt_views": opt, "iterations": int(iterations), "loss_first": None, "loss_last": None, "tex_size": R, "cell": cell}
    stats["psnr_vertex"] = mesh_fidelity(v, f, c0, cameras, gt, bg, device)["psnr_mean"]
    _, baked = bake_vertex_colors(f, c0, R, device)
    t0 = time.perf_counter()
    views = [prepare_texture_view(cam, v, f, R, bg, True, 8, lists=i in opt, device=device) for i, cam in enumerate(cameras)]
    stats["psnr_baked"] = _psnr_views(views, baked, gt)
    out, seen = baked, torch.zeros(R * R, dtype=torch.bool, device=device)
    if V and F and opt and iterations:
        ov = [views[i] for i in opt]
        targets = [gt[i].contiguous() for i in opt]
        for view in ov:
            seen |= view.ranges[:, 1] > view.ranges[:, 0]
        logit = initial_logits(baked).contiguous()
        cur = torch.sigmoid(logit)
        m, s, first, last = torch.zeros_like(logit), torch.zeros_like(logit), None, None
        for it, j in enumerate(view_schedule(len(opt), iterations, seed)):
            diff = texture_shade_forward(ov[j], cur) - targets[j]
            if it == 0:
                first = (diff * diff).mean()
            if it == iterations - 1:
                last = (diff * diff).mean()
            grad = texture_shade_backward(ov[j], diff * (2.0 / diff.numel()))
            color_adam(logit, m, s, grad, cur, it + 1, lr)
        out = torch.where(seen[:, None], cur, baked)
        stats["loss_first"], stats["loss_last"] = float(first), float(last)
    if device != "cpu" and torch.cuda.is_available():
        torch.cuda.synchronize()
    stats["seconds"] = time.perf_counter() - t0
    stats["texels_seen"] = int(seen.sum())
    stats["psnr_fitted"] = _psnr_views(views, out, gt)
    return out, stats


# ---- OBJ + MTL + PNG ----------------------------------------------------------------------------------------------------------------------
def _host(a, dtype):
    return (a.detach().cpu().numpy() if torch.is_tensor(a) else np.asarray(a)).astype(dtype)


def save_textured_obj(path: str, verts, faces, vt, texture, normal_map=None, ao_map=None):
    """Write <path> (.obj: v, vt, f a/ta b/tb c/tc, mtllib, usemtl), <stem>.mtl (map_Kd) and <stem>.png (8 bits).  vt [F, 3, 2] in texels
    (face_uvs); texture [R*R, 3] in 0 .. 1.  The file's vt is ((x + 0.5) / R, 1 - (y + 0.5) / R): v runs upwards in an OBJ.  With normal_map
    [R*R, 3] (object-space unit vectors on the same atlas: mesh_bake.bake_normal_map) also <stem>_normal.png, 0.5 n + 0.5 in 8 bits, and a
    `norm` line in the MTL; without it the three files are what they were before the argument existed.  With ao_map [R*R] (0 .. 1 on the same
    atlas: mesh_query.bake_ambient_occlusion) also <stem>_ao.png, 8-bit greyscale, and a `map_Ka` line after the others; the same holds."""
    from PIL import Image
    v, f = _host(verts, np.float32).reshape(-1, 3), _host(faces, np.int64).reshape(-1, 3)
    uv, tex = _host(vt, np.float64).reshape(-1, 2), _host(texture, np.float32).reshape(-1, 3)
    R = math.isqrt(tex.shape[0])
    if R * R != tex.shape[0] or R == 0:
        raise ValueError(f"save_textured_obj: {tex.shape[0]} texels are not a square")
    if uv.shape[0] != 3 * f.shape[0]:
        raise ValueError(f"save_textured_obj: {uv.shape[0]} texture coordinates for {f.shape[0]} faces")
    if f.size and (f.min() < 0 or f.max() >= v.shape[0]):
        raise ValueError("save_textured_obj: face index outside the vertex array")
    nm = None
    if normal_map is not None:
        nm = _host(normal_map, np.float32).reshape(-1, 3)
        if nm.shape[0] != tex.shape[0]:
            raise ValueError(f"save_textured_obj: a normal map of {nm.shape[0]} texels beside a texture of {tex.shape[0]}")
    ao = None
    if ao_map is not None:
        ao = _host(ao_map, np.float32).reshape(-1)
        if ao.shape[0] != tex.shape[0]:
            raise ValueError(f"save_textured_obj: an occlusion map of {ao.shape[0]} texels beside a texture of {tex.shape[0]}")
    stem = os.path.splitext(path)[0]
    name = os.path.basename(stem)
    Image.fromarray(np.floor(np.clip(tex, 0.0, 1.0) * 255.0 + 0.5).astype(np.uint8).reshape(R, R, 3)).save(stem + ".png")
    with open(stem + ".mtl", "w") as fh:
        fh.write(f"newmtl {name}\nKa 1 1 1\nKd 1 1 1\nKs 0 0 0\nillum 1\nmap_Kd {name}.png\n")
        if nm is not None:
            fh.write(f"norm {name}_normal.png\n")
        if ao is not None:
            fh.write(f"map_Ka {name}_ao.png\n")
    if ao is not None:
        Image.fromarray(np.floor(np.clip(ao, 0.0, 1.0) * 255.0 + 0.5).astype(np.uint8).reshape(R, R), mode="L").save(stem + "_ao.png")
    if nm is not None:
        Image.fromarray(np.floor(np.clip(0.5 * nm + 0.5, 0.0, 1.0) * 255.0 + 0.5).astype(np.uint8).reshape(R, R, 3)).save(stem + "_normal.png")
    lines = [f"mtllib {name}.mtl", f"usemtl {name}"]
    lines += [f"v {float(x)!r} {float(y)!r} {float(z)!r}" for x, y, z in v]
    lines += [f"vt {float((x + 0.5) / R)!r} {float(1.0 - (y + 0.5) / R)!r}" for x, y in uv]
    lines += [f"f {a + 1}/{3 * i + 1} {b + 1}/{3 * i + 2} {c + 1}/{3 * i + 3}" for i, (a, b, c) in enumerate(f.tolist())]
    with open(path, "w") as fh:
        fh.write("\n".join(lines) + "\n")


def read_textured_obj(path: str):
    """(verts [V, 3] float32, faces [F, 3] int32, vt [F, 3, 2] float32 in texels, texture [R*R, 3] float32) of what save_textured_obj wrote"""
    from PIL import Image
    vs, vts, fs, fts, mtl = [], [], [], [], None
    with open(path) as fh:
        for line in fh:
            p = line.split()
            if not p:
                continue
            if p[0] == "v":
                vs.append([float(x) for x in p[1:4]])
            elif p[0] == "vt":
                vts.append([float(x) for x in p[1:3]])
            elif p[0] == "f":
                if len(p) != 4:
                    raise ValueError(f"{path}: only triangles are read, got a face of {len(p) - 1} corners")
                ab = [q.split("/") for q in p[1:4]]
                if any(len(q) < 2 or not q[1] for q in ab):
                    raise ValueError(f"{path}: a face without texture coordinates")
                fs.append([int(q[0]) - 1 for q in ab])
                fts.append([int(q[1]) - 1 for q in ab])
            elif p[0] == "mtllib":
                mtl = p[1]
    if mtl is None:
        raise ValueError(f"{path}: no mtllib")
    png = None
    with open(os.path.join(os.path.dirname(path), mtl)) as fh:
        for line in fh:
            p = line.split()
            if p and p[0] == "map_Kd":
                png = p[1]
    if png is None:
        raise ValueError(f"{path}: {mtl} names no map_Kd")
    img = np.asarray(Image.open(os.path.join(os.path.dirname(path), png)).convert("RGB"))
    if img.shape[0] != img.shape[1]:
        raise ValueError(f"{png}: the texture must be square, got {img.shape[1]} x {img.shape[0]}")
    R = img.shape[0]
    uv = np.asarray(vts, dtype=np.float64).reshape(-1, 2)[np.asarray(fts, dtype=np.int64).reshape(-1, 3)]        # [F, 3, 2]
    vt = np.stack([uv[..., 0] * R - 0.5, (1.0 - uv[..., 1]) * R - 0.5], -1)
    vt = (np.round(vt * 65536.0) / 65536.0).astype(np.float32)          # to 2^-16 texel: the writer's integers come back as integers
    return (np.asarray(vs, dtype=np.float32).reshape(-1, 3), np.asarray(fs, dtype=np.int32).reshape(-1, 3), vt,
            (img.reshape(R * R, 3).astype(np.float32) / 255.0))
