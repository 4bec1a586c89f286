"""Export the baked asset as one self-contained GLB (glTF 2.0 binary), on the gfx950 kernels of libv3d_recon.so (csrc_recon/meshtangent.hip,
include/v3d_recon.h "Tangent space and GLB"): per-corner NORMAL / TANGENT frames of the per-face atlas, the object-space normal map of
mesh_bake.py re-expressed in those frames (glTF's normalTexture is in tangent space) and back, and a lit shade from exactly the data the file
carries.

    cn, ct = corner_frames(verts, faces)                              # [3F, 3], [3F, 4] (xyz, w)
    tmap = to_tangent_space(verts, faces, normal_map, tex_size)       # [R*R, 3] float unit vectors
    omap = to_object_space(moved_verts, faces, tmap, tex_size)        # the object-space map of the mesh after it moved
    lit = prepare_lit_view(cam, verts, faces, tex_size, bg)
    image, normals = shade_lit(lit, texture, tmap, ao_map)            # [3, H, W] each; normals in world space
    frames = render_lit_orbit(verts, faces, texture, tmap, ao_map, 36, 2.0, 0.0, 60.0, 512)
    fid = tangent_map_fidelity(verts, faces, tmap, high_verts, high_faces, cameras)
    save_glb("mesh.glb", verts, faces, texture, tangent_map=tmap, ao_map=ao_map, tex_size=R)
    asset = read_glb("mesh.glb")

save_glb and read_glb are numpy + PIL + json + struct, written from the glTF 2.0 specification: they take numpy arrays (tensors are moved to
the host) and need neither a GPU nor the library; without corner frames they compute them with the numpy restatement below.  Everything
else runs under no_grad on the device.  No atomics: two calls with the same arguments return bit-equal results.  There is no fallback:
without the libraries the device functions raise."""
from __future__ import annotations

import dataclasses
import io
import json
import math
import os
import struct
from typing import Optional, Sequence

import numpy as np
import torch

from .cameras import Camera, orbit_cameras
from .geometry import _check, _stream, load_library
from .mesh_render import _bg, _check_view, _dev

MAX_TEX_SIZE = 4096
MAX_LIGHTS = 4
LEN2_EPS = 1e-20
# The default rig of render_lit_orbit: a key light from the upper left behind the camera, a fill light from the right, both fixed to the
# camera, plus ambient.  Directions point TOWARDS the light, in the camera's frame (x right, y DOWN, z forward).  The numbers are a choice,
# not a measurement: they add up to 1.4 where a surface faces the key light, so a frame is clamped only on its brightest patches.
KEY_LIGHT = ((-0.5, -0.7, -1.0), 0.85)
FILL_LIGHT = ((0.8, -0.1, -0.6), 0.30)
AMBIENT = 0.25
# glTF constants
_FLOAT, _ARRAY_BUFFER, _LINEAR, _CLAMP, _TRIANGLES = 5126, 34962, 9729, 33071, 4
Y_UP_ROTATION = [-math.sqrt(0.5), 0.0, 0.0, math.sqrt(0.5)]            # (x, y, z) -> (x, z, -y): the project's +z up to glTF's +y up


# ---- the frames and the two conversions, on the device ----------------------------------------------------------------------------------------
def _low_mesh(verts, faces, normals, device, who: str):
    from .mesh_clean import _corner_lists, _mesh_arg, _normals, _rows_arg
    v, f, _ = _mesh_arg(verts, faces, None, device, who)
    n = None
    if normals is not None:
        n = _rows_arg(normals, device, who, "normals")
        if n.shape != v.shape:
            raise ValueError(f"{who}: {v.shape[0]} vertices, {n.shape[0]} normals")
    elif v.shape[0] and f.shape[0]:
        n = _normals(v, f, *_corner_lists(f, v.shape[0]))
    return v, f, n


def _tex_arg(tex_size, who: str) -> int:
    R = int(tex_size)
    if not 1 <= R <= MAX_TEX_SIZE:
        raise ValueError(f"{who}: tex_size {R} outside 1 .. {MAX_TEX_SIZE}")
    return R


def frames_on_device(v: torch.Tensor, f: torch.Tensor, n: torch.Tensor):
    """(corner_normals [3F, 3], corner_tangents [3F, 4]) of validated device tensors (V >= 1, F >= 1): v3d_recon_tex_corner_frames"""
    lib = load_library()
    F = f.shape[0]
    cn = torch.empty(3 * F, 3, dtype=torch.float32, device=v.device)
    ct = torch.empty(3 * F, 4, dtype=torch.float32, device=v.device)
    _check(lib, lib.v3d_recon_tex_corner_frames(v.data_ptr(), v.shape[0], f.data_ptr(), F, n.data_ptr(), cn.data_ptr(), ct.data_ptr(), _stream()),
           "v3d_recon_tex_corner_frames")
    return cn, ct


@torch.no_grad()
def corner_frames(verts, faces, normals=None, device="cuda"):
    """(corner_normals [3F, 3], corner_tangents [3F, 4] = xyz, w) float32 on `device`: glTF's NORMAL and TANGENT of corner 3 f + k, place k of
    face f, by THE TANGENT FRAME of include/v3d_recon.h.  normals [V, 3]: the vertex normals to use (default: mesh_clean.vertex_normals).  A
    mesh with V = 0 or F = 0 gives empty arrays without a launch."""
    v, f, n = _low_mesh(verts, faces, normals, device, "corner_frames")
    if v.shape[0] == 0 or f.shape[0] == 0:
        return torch.zeros(0, 3, dtype=torch.float32, device=device), torch.zeros(0, 4, dtype=torch.float32, device=device)
    return frames_on_device(v, f, n)


def convert_texels(f: torch.Tensor, num_verts: int, cn: torch.Tensor, ct: torch.Tensor, source: torch.Tensor, tex_size: int, encode: bool):
    """(owner [R*R] int32, map [R*R, 3]) of validated device tensors: v3d_recon_tex_encode_tangent (encode) or v3d_recon_tex_decode_tangent"""
    lib = load_library()
    R = int(tex_size)
    owner = torch.empty(R * R, dtype=torch.int32, device=f.device)
    out = torch.empty(R * R, 3, dtype=torch.float32, device=f.device)
    fn, name = (lib.v3d_recon_tex_encode_tangent, "v3d_recon_tex_encode_tangent") if encode else (lib.v3d_recon_tex_decode_tangent,
                                                                                                 "v3d_recon_tex_decode_tangent")
    _check(lib, fn(f.data_ptr(), f.shape[0], int(num_verts), cn.data_ptr(), ct.data_ptr(), source.data_ptr(), R, owner.data_ptr(), out.data_ptr(),
                   _stream()), name)
    return owner, out


def _convert(verts, faces, source, tex_size, normals, device, encode: bool, who: str):
    from .mesh_texture import atlas_layout
    R = _tex_arg(tex_size, who)
    m = _dev(source, torch.float32, device).reshape(-1, 3)
    if m.shape[0] != R * R:
        raise ValueError(f"{who}: a map of {m.shape[0]} texels for a texture of {R} x {R}")
    v, f, n = _low_mesh(verts, faces, normals, device, who)
    if v.shape[0] == 0 or f.shape[0] == 0:
        return torch.tensor((0.0, 0.0, 1.0), dtype=torch.float32, device=device).expand(R * R, 3).contiguous()
    atlas_layout(f.shape[0], R)
    cn, ct = frames_on_device(v, f, n)
    return convert_texels(f, v.shape[0], cn, ct, m, R, encode)[1]


@torch.no_grad()
def to_tangent_space(verts, faces, object_map, tex_size: int, normals=None, device="cuda") -> torch.Tensor:
    """tangent_map [R*R, 3] float32 on `device`: the object-space map [R*R, 3] (mesh_bake.bake_normal_map) in the mesh's tangent frames, unit
    vectors (not yet 0.5 c + 0.5); (0, 0, 1) on unowned texels.  A mesh with V = 0 or F = 0 gives an all-(0, 0, 1) map without a launch."""
    return _convert(verts, faces, object_map, tex_size, normals, device, True, "to_tangent_space")


@torch.no_grad()
def to_object_space(verts, faces, tangent_map, tex_size: int, normals=None, device="cuda") -> torch.Tensor:
    """object_map [R*R, 3]: the inverse.  With the vertices of a mesh that moved since the bake, the tangent map gives the new object-space
    map: a rigid motion of the mesh rotates every decoded normal with it."""
    return _convert(verts, faces, tangent_map, tex_size, normals, device, False, "to_object_space")


# ---- the lit view -----------------------------------------------------------------------------------------------------------------------------
@dataclasses.dataclass
class LitView:
    """A mesh_texture.TextureView (prepared without lists) with what it does not keep: pix_w [H, W, 3], the perspective-correct weights of
    v3d_recon_mesh_pixel_weights, and the mesh's corner frames [3F, 3], [3F, 4]; `camera` is the view's."""
    view: object
    pix_w: torch.Tensor
    corner_normals: torch.Tensor
    corner_tangents: torch.Tensor
    camera: Camera


@torch.no_grad()
def prepare_lit_view(camera: Camera, verts, faces, tex_size: int, bg, cull: bool = True, subpixel_bits: int = 8, normals=None, frames=None,
                     device="cuda") -> LitView:
    """Rasterize the mesh once from `camera` as mesh_texture.prepare_texture_view does (the same kernels in the same order, so face_id,
    pix_tex and pix_tw are bit-equal to its), and keep pix_w and the corner frames (`frames`: a pair already computed for this mesh)."""
    from .mesh_refine import _host_bg, pixel_weights
    from .mesh_render import project_vertices, rasterize_projected
    from .mesh_texture import TextureView, atlas_layout, pixel_texels
    from .rasterize import gs_camera
    H, W = int(camera.height), int(camera.width)
    _check_view(W, H, subpixel_bits)
    R = _tex_arg(tex_size, "prepare_lit_view")
    v, f, n = _low_mesh(verts, faces, normals, device, "prepare_lit_view")
    V, F = v.shape[0], f.shape[0]
    bgt, bgv = _host_bg(bg, device)
    if V == 0 or F == 0:
        z = lambda *s, dt=torch.float32: torch.zeros(*s, dtype=dt, device=device)  # noqa: E731
        view = TextureView(W, H, R, F, torch.full((H, W), -1, dtype=torch.int32, device=device), z(H, W),
                           torch.full((H, W, 4), -1, dtype=torch.int32, device=device), z(H, W, 4), None, None, None, bgt, bgv, launch=False)
        return LitView(view, z(H, W, 3), z(0, 3), z(0, 4), camera)
    atlas_layout(F, R)
    gc = gs_camera(camera, bg)
    zv, _, pix_q = project_vertices(gc, v, subpixel_bits)
    out = rasterize_projected(gc, f, pix_q, zv, torch.zeros(V, 3, dtype=torch.float32, device=device), cull, False, subpixel_bits)
    _, pix_w = pixel_weights(out["face_id"], f, pix_q, zv, subpixel_bits)
    pix_tex, pix_tw = pixel_texels(out["face_id"], pix_w, F, R)
    cn, ct = frames if frames is not None else frames_on_device(v, f, n)
    view = TextureView(W, H, R, F, out["face_id"], out["alpha"], pix_tex, pix_tw, None, None, None, bgt, bgv)
    return LitView(view, pix_w, cn, ct, camera)


def _lights_arg(lights, who: str):
    """(K, dirs float32 [K, 3] normalised, intensity float32 [K]) of [((x, y, z), intensity), ...] in world space"""
    lights = list(lights)
    if len(lights) > MAX_LIGHTS:
        raise ValueError(f"{who}: {len(lights)} lights, at most {MAX_LIGHTS}")
    dirs = np.zeros((len(lights), 3), dtype=np.float64)
    inten = np.zeros(len(lights), dtype=np.float32)
    for k, (d, i) in enumerate(lights):
        d = np.asarray(d, dtype=np.float64).reshape(3)
        length = float(np.linalg.norm(d))
        if not (math.isfinite(length) and length > 0) or not math.isfinite(float(i)):
            raise ValueError(f"{who}: light {k} has no direction or no finite intensity")
        dirs[k], inten[k] = d / length, i
    return len(lights), np.ascontiguousarray(dirs, dtype=np.float32), inten


def camera_lights(camera: Camera, rig=(KEY_LIGHT, FILL_LIGHT)):
    """The rig's directions (camera frame: x right, y down, z forward) in world space: [((x, y, z), intensity), ...].  world_view is for row
    vectors, view = world @ R, so world = view @ R^T."""
    Rm = camera.world_view[:3, :3].detach().cpu().double().numpy()
    return [(tuple((np.asarray(d, dtype=np.float64) @ Rm.T).tolist()), float(i)) for d, i in rig]


def _map_arg(a, rows: int, cols: int, device, who: str, what: str):
    if a is None:
        return None
    t = _dev(a, torch.float32, device).reshape(-1, cols) if cols > 1 else _dev(a, torch.float32, device).reshape(-1)
    if t.shape[0] != rows:
        raise ValueError(f"{who}: {what} of {t.shape[0]} texels for a texture of {rows}")
    return t


@torch.no_grad()
def shade_lit(lit: LitView, albedo, tangent_map=None, ao_map=None, lights=None, ambient: float = AMBIENT):
    """(image [3, H, W], normals [3, H, W]) float32 on the view's device (v3d_recon_tex_shade_lit): per pixel the normal decoded from the
    tangent map in the interpolated corner frames (the interpolated vertex normal, normalised, when tangent_map is None), in world space, 0
    where nothing covers; and albedo x (ambient x ao + sum_k I_k max(0, n . d_k)), not clamped, the background where nothing covers.
    albedo [R*R, 3], ao_map [R*R] or None (1).  lights: [((x, y, z), intensity), ...] in world space, up to 4, directions towards the
    light (normalised here); default: the camera-fixed rig KEY_LIGHT, FILL_LIGHT of this module."""
    view = lit.view
    H, W, R = view.height, view.width, view.tex_size
    dev = view.pix_tex.device
    K, dirs, inten = _lights_arg(camera_lights(lit.camera) if lights is None else lights, "shade_lit")
    ambient = float(ambient)
    if not math.isfinite(ambient):
        raise ValueError(f"shade_lit: ambient {ambient} is not finite")
    alb = _map_arg(albedo, R * R, 3, dev, "shade_lit", "an albedo")
    tm = _map_arg(tangent_map, R * R, 3, dev, "shade_lit", "a tangent map")
    ao = _map_arg(ao_map, R * R, 1, dev, "shade_lit", "an occlusion map")
    if not view.launch:
        return view.bg.view(3, 1, 1).expand(3, H, W).contiguous(), torch.zeros(3, H, W, dtype=torch.float32, device=dev)
    lib = load_library()
    image = torch.empty(3, H, W, dtype=torch.float32, device=dev)
    normals = torch.empty(3, H, W, dtype=torch.float32, device=dev)
    bg = view.bg_values
    _check(lib, lib.v3d_recon_tex_shade_lit(view.face_id.data_ptr(), lit.pix_w.data_ptr(), view.pix_tex.data_ptr(), view.pix_tw.data_ptr(), view.num_faces,
                                            lit.corner_normals.data_ptr(), lit.corner_tangents.data_ptr(), tm.data_ptr() if tm is not None else None,
                                            alb.data_ptr(), ao.data_ptr() if ao is not None else None, R, W, H, K, dirs.ctypes.data if K else None,
                                            inten.ctypes.data if K else None, ambient, bg[0], bg[1], bg[2], image.data_ptr(), normals.data_ptr(),
                                            _stream()), "v3d_recon_tex_shade_lit")
    return image, normals


@torch.no_grad()
def render_lit_orbit(verts, faces, texture, tangent_map, ao_map, n: int, radius: float, elevation: float, fov: float, reso: int,
                     white_background: bool = True, cull: bool = True, lights=None, ambient: float = AMBIENT, device="cuda") -> np.ndarray:
    """n turntable frames of the mesh lit from exactly what the GLB carries (albedo, tangent-space normal map, occlusion; either map may be
    None), uint8 [n, reso, reso, 3] on the host.  lights None: the rig of this module, fixed to the camera, so the light turns with it;
    a list of world-space lights stays put while the camera turns.  No shadows."""
    cams, _ = orbit_cameras(n, radius, elevation, fov, reso)
    _check_view(int(reso), int(reso), 8)
    tex = _dev(texture, torch.float32, device).reshape(-1, 3)
    R = math.isqrt(tex.shape[0])
    if R * R != tex.shape[0] or R == 0:
        raise ValueError(f"render_lit_orbit: {tex.shape[0]} texels are not a square")
    v, f, nrm = _low_mesh(verts, faces, None, device, "render_lit_orbit")
    frames = frames_on_device(v, f, nrm) if v.shape[0] and f.shape[0] else None
    out = []
    for cam in cams:
        lit = prepare_lit_view(cam, v, f, R, _bg(white_background), cull, normals=nrm, frames=frames, device=device)
        img, _ = shade_lit(lit, tex, tangent_map, ao_map, lights, ambient)
        out.append((img.clamp(0, 1) * 255).to(torch.uint8).permute(1, 2, 0).cpu())
    return torch.stack(out).numpy() if out else np.zeros((0, int(reso), int(reso), 3), dtype=np.uint8)


@torch.no_grad()
def tangent_map_fidelity(low_verts, low_faces, tangent_map, high_verts, high_faces, cameras: Sequence[Camera], device="cuda") -> dict:
    """mesh_bake.normal_map_fidelity for the tangent-space map: per view the mean angle in degrees, over the pixels both meshes cover, between
    the high mesh's rendered vertex normals (render_mesh_normals) and the low mesh's (a) rendered vertex normals, "before", (b) `normals` output
    of shade_lit, "after".  tangent_map None: the interpolated corner normals.  The same keys."""
    from .mesh_bake import _camera_normals, _mean_angle
    from .mesh_clean import _mesh_arg, render_mesh_normals
    lv, lf, ln = _low_mesh(low_verts, low_faces, None, device, "tangent_map_fidelity")
    hv, hf, _ = _mesh_arg(high_verts, high_faces, None, device, "tangent_map_fidelity")
    R = None
    if tangent_map is not None:
        tm = _dev(tangent_map, torch.float32, device).reshape(-1, 3)
        R = math.isqrt(tm.shape[0])
        if R * R != tm.shape[0] or R == 0:
            raise ValueError(f"tangent map: {tm.shape[0]} texels are not a square")
    frames = frames_on_device(lv, lf, ln) if lv.shape[0] and lf.shape[0] else None
    before, after, pixels = [], [], []
    flip = torch.tensor([1.0, -1.0, -1.0], dtype=torch.float32, device=device)
    for cam in cameras:
        _check_view(int(cam.width), int(cam.height), 8)
        high = render_mesh_normals(cam, hv, hf, device=device)
        low = render_mesh_normals(cam, lv, lf, device=device)
        H, W = int(cam.height), int(cam.width)
        if R is None:
            from .mesh_texture import MIN_CELL
            g = math.isqrt(max((lf.shape[0] + 1) // 2 - 1, 0)) + 1
            size = min(MAX_TEX_SIZE, MIN_CELL * g)
            lit = prepare_lit_view(cam, lv, lf, size, [0.0, 0.0, 0.0], normals=ln, frames=frames, device=device)
            _, nrm = shade_lit(lit, torch.zeros(size * size, 3, device=device), None, None, [], 0.0)
        else:
            lit = prepare_lit_view(cam, lv, lf, R, [0.0, 0.0, 0.0], normals=ln, frames=frames, device=device)
            _, nrm = shade_lit(lit, torch.zeros(R * R, 3, device=device), tm, None, [], 0.0)
        Rm = cam.world_view[:3, :3].to(device=device, dtype=torch.float32)
        mapped = ((nrm.reshape(3, H * W).t() @ Rm) * flip).t().reshape(3, H, W)            # the rotation and the flip of normal_colors
        both = (high["alpha"] > 0) & (low["alpha"] > 0) & (lit.view.alpha > 0)
        nh = _camera_normals(cam, high["render"])
        before.append(_mean_angle(_camera_normals(cam, low["render"]), nh, both))
        after.append(_mean_angle(mapped, nh, both))
        pixels.append(int(both.sum()))
    mean = lambda xs: float(np.nanmean(xs)) if len(xs) and not all(math.isnan(x) for x in xs) else float("nan")  # noqa: E731
    return {"angle_before": before, "angle_after": after, "angle_before_mean": mean(before), "angle_after_mean": mean(after), "pixels": pixels}


# ---- numpy restatement of the frames (for save_glb without a device) ----------------------------------------------------------------------------
def _host(a, dtype):
    return np.ascontiguousarray(a.detach().cpu().numpy() if torch.is_tensor(a) else np.asarray(a)).astype(dtype)


def _np_unit(x):
    """rows of x divided by their length; (0, 0, 1) where the squared length is not above 1e-20; also which rows had a direction"""
    len2 = (x[:, 0] * x[:, 0] + x[:, 1] * x[:, 1]) + x[:, 2] * x[:, 2]
    ok = len2 > LEN2_EPS
    out = x / np.sqrt(np.where(ok, len2, 1.0))[:, None]
    out[~ok] = (0.0, 0.0, 1.0)
    return out, ok


def vertex_normals_host(verts, faces) -> np.ndarray:
    """[V, 3] float64: the area-weighted mean of the incident faces' normals, of length 1, (0, 0, 1) where there is none (what
    mesh_clean.vertex_normals computes, in numpy; faces with an index outside the vertices add nothing)"""
    v, f = _host(verts, np.float64).reshape(-1, 3), _host(faces, np.int64).reshape(-1, 3)
    s = np.zeros_like(v)
    if f.shape[0] and v.shape[0]:
        ok = ((f >= 0) & (f < v.shape[0])).all(1)
        f = f[ok]
        fn = np.cross(v[f[:, 1]] - v[f[:, 0]], v[f[:, 2]] - v[f[:, 0]])
        for k in range(3):
            np.add.at(s, f[:, k], fn)
    return _np_unit(s)[0] if v.shape[0] else s


def corner_frames_host(verts, faces, normals=None):
    """(corner_normals [3F, 3], corner_tangents [3F, 4]) float32: THE TANGENT FRAME of include/v3d_recon.h in numpy (fp64, rounded at the end)"""
    v, f = _host(verts, np.float64).reshape(-1, 3), _host(faces, np.int64).reshape(-1, 3)
    F, V = f.shape[0], v.shape[0]
    n = vertex_normals_host(v, f) if normals is None else _host(normals, np.float64).reshape(-1, 3)
    if n.shape != v.shape:
        raise ValueError(f"corner_frames_host: {V} vertices, {n.shape[0]} normals")
    cn = np.tile(np.array([0.0, 0.0, 1.0]), (3 * F, 1))
    ct = np.tile(np.array([1.0, 0.0, 0.0, -1.0]), (3 * F, 1))
    if F == 0 or V == 0:
        return cn.astype(np.float32), ct.astype(np.float32)
    ok = ((f >= 0) & (f < V)).all(1)
    fz = np.where(ok[:, None], f, 0)
    s = np.where(np.arange(F) & 1, -1.0, 1.0)
    se1 = np.repeat(s[:, None] * (v[fz[:, 1]] - v[fz[:, 0]]), 3, 0)                          # [3F, 3]
    N, _ = _np_unit(n[fz.reshape(-1)])
    d = (N[:, 0] * se1[:, 0] + N[:, 1] * se1[:, 1]) + N[:, 2] * se1[:, 2]
    T, has = _np_unit(se1 - N * d[:, None])
    q = np.copysign(1.0, N[:, 2])
    a = -1.0 / (q + N[:, 2])
    b = N[:, 0] * N[:, 1] * a
    t1 = np.stack([1.0 + q * N[:, 0] * N[:, 0] * a, q * b, -q * N[:, 0]], 1)
    T = np.where(has[:, None], T, t1)
    rows = np.repeat(ok, 3)
    cn[rows], ct[rows, :3] = N[rows], T[rows]
    return cn.astype(np.float32), ct.astype(np.float32)


# ---- the GLB ----------------------------------------------------------------------------------------------------------------------------------
def quantise(x) -> np.ndarray:
    """the project's 8-bit rule: floor(clip(x, 0, 1) * 255 + 0.5)"""
    return np.floor(np.clip(np.asarray(x, dtype=np.float32), 0.0, 1.0) * np.float32(255.0) + np.float32(0.5)).astype(np.uint8)


def _png(pixels: np.ndarray) -> bytes:
    from PIL import Image
    buf = io.BytesIO()
    Image.fromarray(pixels).save(buf, format="PNG")
    return buf.getvalue()


def face_uvs_host(num_faces: int, tex_size: int) -> np.ndarray:
    """vt [F, 3, 2] float64 in texels: THE ATLAS of include/v3d_recon.h (what mesh_texture.face_uvs returns), by the face index alone"""
    from .mesh_texture import atlas_layout
    F = int(num_faces)
    if F == 0:
        return np.zeros((0, 3, 2))
    S, g = atlas_layout(F, int(tex_size))
    L = S - 3
    fi = np.arange(F)
    c, half = fi >> 1, fi & 1
    x0, y0 = (c % g) * S, (c // g) * S
    d = np.array([[0, 0], [L, 0], [0, L]])
    u = np.where(half[:, None] == 0, x0[:, None] + d[None, :, 0], x0[:, None] + S - 1 - d[None, :, 0])
    w = np.where(half[:, None] == 0, y0[:, None] + d[None, :, 1], y0[:, None] + S - 1 - d[None, :, 1])
    return np.stack([u, w], -1).astype(np.float64)


def save_glb(path: str, verts, faces, texture, tangent_map=None, ao_map=None, tex_size: Optional[int] = None, corner_normals=None,
             corner_tangents=None, normals=None) -> int:
    """Write one self-contained GLB and return its size in bytes.  verts [V, 3], faces [F, 3] (the mesh of the per-face atlas), texture
    [R*R, 3] the albedo in 0 .. 1, tangent_map [R*R, 3] float unit vectors (to_tangent_space) or None, ao_map [R*R] in 0 .. 1 or None;
    tex_size R (default: the square root of the texture's length).  corner_normals [3F, 3] and corner_tangents [3F, 4]: those of corner_frames
    (the frames the tangent map was encoded in); without them corner_frames_host computes them (from `normals` [V, 3] when given).

    The file: one scene, one node, one mesh, one non-indexed TRIANGLES primitive of 3F vertices (corners of different faces share a
    position but not a UV or a tangent, so nothing is welded) with POSITION (min / max), NORMAL, TANGENT (VEC4) and TEXCOORD_0 =
    ((x + 0.5) / R, (y + 0.5) / R) of the atlas coordinates, no flip; the mesh data stays in the project's +z-up object space and the NODE
    carries the rotation to glTF's +y up.  One material: baseColorTexture, metallicFactor 0, roughnessFactor 1, normalTexture when a
    tangent map is given (0.5 c + 0.5), occlusionTexture when an occlusion map is given (a grey RGB PNG: glTF reads the R channel).  One
    sampler, LINEAR / CLAMP_TO_EDGE, no mipmaps (the atlas's gutters are one to two texels).  The images are PNG bytes in buffer views,
    quantised by floor(clip(x) 255 + 0.5).  A mesh with F = 0 gives a file with the node alone."""
    v, f = _host(verts, np.float32).reshape(-1, 3), _host(faces, np.int64).reshape(-1, 3)
    tex = _host(texture, np.float32).reshape(-1, 3)
    R = math.isqrt(tex.shape[0]) if tex_size is None else int(tex_size)
    if R < 1 or R * R != tex.shape[0]:
        raise ValueError(f"save_glb: a texture of {tex.shape[0]} texels is not {R} x {R}")
    if f.size and (f.min() < 0 or f.max() >= v.shape[0]):
        raise ValueError("save_glb: face index outside the vertex array")
    tm = ao = None
    if tangent_map is not None:
        tm = _host(tangent_map, np.float32).reshape(-1, 3)
        if tm.shape[0] != R * R:
            raise ValueError(f"save_glb: a tangent map of {tm.shape[0]} texels beside a texture of {R * R}")
    if ao_map is not None:
        ao = _host(ao_map, np.float32).reshape(-1)
        if ao.shape[0] != R * R:
            raise ValueError(f"save_glb: an occlusion map of {ao.shape[0]} texels beside a texture of {R * R}")
    if (corner_normals is None) != (corner_tangents is None):
        raise ValueError("save_glb: corner_normals and corner_tangents come together")
    F = f.shape[0]
    gltf = {"asset": {"version": "2.0", "generator": "v3d_amd.recon.mesh_gltf"}, "scene": 0, "scenes": [{"nodes": [0]}],
            "nodes": [{"name": "mesh", "rotation": list(Y_UP_ROTATION)}]}
    blob = bytearray()
    views = []

    def add_view(data: bytes, target=None) -> int:
        while len(blob) % 4:
            blob.append(0)
        view = {"buffer": 0, "byteOffset": len(blob), "byteLength": len(data)}
        if target is not None:
            view["target"] = target
        blob.extend(data)
        views.append(view)
        return len(views) - 1

    if F:
        if corner_normals is None:
            cn, ct = corner_frames_host(v, f, normals)
        else:
            cn, ct = _host(corner_normals, np.float32).reshape(-1, 3), _host(corner_tangents, np.float32).reshape(-1, 4)
        if cn.shape[0] != 3 * F or ct.shape[0] != 3 * F:
            raise ValueError(f"save_glb: {cn.shape[0]} corner normals and {ct.shape[0]} corner tangents for {F} faces")
        pos = np.ascontiguousarray(v[f.reshape(-1)], dtype="<f4")
        uv = np.ascontiguousarray((face_uvs_host(F, R).reshape(-1, 2) + 0.5) / R, dtype="<f4")
        accessors = []
        for data, kind in ((pos, "VEC3"), (np.ascontiguousarray(cn, dtype="<f4"), "VEC3"), (np.ascontiguousarray(ct, dtype="<f4"), "VEC4"), (uv, "VEC2")):
            accessors.append({"bufferView": add_view(data.tobytes(), _ARRAY_BUFFER), "componentType": _FLOAT, "count": 3 * F, "type": kind})
        accessors[0]["min"], accessors[0]["max"] = [float(x) for x in pos.min(0)], [float(x) for x in pos.max(0)]
        images = [_png(quantise(tex).reshape(R, R, 3))]
        material = {"name": "baked", "pbrMetallicRoughness": {"baseColorTexture": {"index": 0}, "metallicFactor": 0.0, "roughnessFactor": 1.0},
                    "doubleSided": False}
        if tm is not None:
            material["normalTexture"] = {"index": len(images)}
            images.append(_png(quantise(np.float32(0.5) * tm + np.float32(0.5)).reshape(R, R, 3)))
        if ao is not None:
            material["occlusionTexture"] = {"index": len(images)}
            images.append(_png(np.repeat(quantise(ao).reshape(R, R, 1), 3, 2)))
        gltf["nodes"][0]["mesh"] = 0
        gltf["meshes"] = [{"primitives": [{"attributes": {"POSITION": 0, "NORMAL": 1, "TANGENT": 2, "TEXCOORD_0": 3}, "material": 0,
                                           "mode": _TRIANGLES}]}]
        gltf["materials"] = [material]
        gltf["samplers"] = [{"magFilter": _LINEAR, "minFilter": _LINEAR, "wrapS": _CLAMP, "wrapT": _CLAMP}]
        gltf["textures"] = [{"sampler": 0, "source": i} for i in range(len(images))]
        gltf["images"] = [{"bufferView": add_view(png), "mimeType": "image/png"} for png in images]
        gltf["accessors"] = accessors
        while len(blob) % 4:
            blob.append(0)
        gltf["bufferViews"] = views
        gltf["buffers"] = [{"byteLength": len(blob)}]
    js = json.dumps(gltf, separators=(",", ":"), allow_nan=False).encode("utf-8")
    js += b" " * (-len(js) % 4)
    total = 12 + 8 + len(js) + ((8 + len(blob)) if blob else 0)
    d = os.path.dirname(path)
    if d:
        os.makedirs(d, exist_ok=True)
    with open(path, "wb") as fh:
        fh.write(struct.pack("<4sII", b"glTF", 2, total))
        fh.write(struct.pack("<II", len(js), 0x4E4F534A))
        fh.write(js)
        if blob:
            fh.write(struct.pack("<II", len(blob), 0x004E4942))
            fh.write(bytes(blob))
    return total


def read_glb(path: str) -> dict:
    """What save_glb wrote, as float arrays: {"verts" [3F, 3], "faces" [F, 3] = arange(3F), "uv" [3F, 2], "normals" [3F, 3], "tangents" [3F, 4],
    "texture" [R*R, 3] in 0 .. 1, "tangent_map" [R*R, 3] = 2 x - 1 of the 8-bit image (not renormalised) or None, "ao_map" [R*R] (the R
    channel) or None, "tex_size" R (0 without a texture), "rotation": the node's quaternion, "json": the parsed JSON chunk}"""
    from PIL import Image
    with open(path, "rb") as fh:
        raw = fh.read()
    if len(raw) < 20 or raw[:4] != b"glTF":
        raise ValueError(f"{path}: not a GLB file")
    version, total = struct.unpack_from("<II", raw, 4)
    if version != 2 or total != len(raw):
        raise ValueError(f"{path}: version {version}, length {total} in a file of {len(raw)} bytes")
    n, kind = struct.unpack_from("<II", raw, 12)
    if kind != 0x4E4F534A:
        raise ValueError(f"{path}: the first chunk is not JSON")
    gltf = json.loads(raw[20:20 + n].decode("utf-8"))
    at, blob = 20 + n, b""
    if at < len(raw):
        m, kind = struct.unpack_from("<II", raw, at)
        if kind != 0x004E4942:
            raise ValueError(f"{path}: the second chunk is not BIN")
        blob = raw[at + 8:at + 8 + m]
    node = gltf["nodes"][gltf["scenes"][gltf.get("scene", 0)]["nodes"][0]]
    out = {"verts": np.zeros((0, 3), np.float32), "faces": np.zeros((0, 3), np.int32), "uv": np.zeros((0, 2), np.float32),
           "normals": np.zeros((0, 3), np.float32), "tangents": np.zeros((0, 4), np.float32), "texture": None, "tangent_map": None, "ao_map": None,
           "tex_size": 0, "rotation": node.get("rotation"), "json": gltf}
    if "mesh" not in node:
        return out
    prim = gltf["meshes"][node["mesh"]]["primitives"][0]
    if prim.get("mode", 4) != 4 or "indices" in prim:
        raise ValueError(f"{path}: not the non-indexed triangle list save_glb writes")
    width = {"VEC2": 2, "VEC3": 3, "VEC4": 4}

    def accessor(i):
        a = gltf["accessors"][i]
        bv = gltf["bufferViews"][a["bufferView"]]
        if a["componentType"] != _FLOAT or "byteStride" in bv:
            raise ValueError(f"{path}: accessor {i} is not tightly packed float")
        start = bv.get("byteOffset", 0) + a.get("byteOffset", 0)
        return np.frombuffer(blob, dtype="<f4", count=a["count"] * width[a["type"]], offset=start).reshape(a["count"], width[a["type"]]).copy()

    def image(tex_ref):
        bv = gltf["bufferViews"][gltf["images"][gltf["textures"][tex_ref["index"]]["source"]]["bufferView"]]
        start = bv.get("byteOffset", 0)
        return np.asarray(Image.open(io.BytesIO(blob[start:start + bv["byteLength"]])).convert("RGB"))

    att = prim["attributes"]
    out["verts"], out["normals"], out["tangents"], out["uv"] = (accessor(att[k]) for k in ("POSITION", "NORMAL", "TANGENT", "TEXCOORD_0"))
    out["faces"] = np.arange(out["verts"].shape[0], dtype=np.int32).reshape(-1, 3)
    mat = gltf["materials"][prim["material"]]
    img = image(mat["pbrMetallicRoughness"]["baseColorTexture"])
    if img.shape[0] != img.shape[1]:
        raise ValueError(f"{path}: the texture must be square, got {img.shape[1]} x {img.shape[0]}")
    R = img.shape[0]
    out["tex_size"], out["texture"] = R, img.reshape(R * R, 3).astype(np.float32) / 255.0
    if "normalTexture" in mat:
        out["tangent_map"] = image(mat["normalTexture"]).reshape(-1, 3).astype(np.float32) / 255.0 * 2.0 - 1.0
    if "occlusionTexture" in mat:
        out["ao_map"] = image(mat["occlusionTexture"]).reshape(-1, 3)[:, 0].astype(np.float32) / 255.0
    return out
