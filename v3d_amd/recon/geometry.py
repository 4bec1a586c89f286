"""Geometry from the reconstructed splats on the gfx950 kernels of libv3d_recon.so (csrc_recon/geom.hip, include/v3d_recon.h): depth and
alpha maps beside the colour image (what the reference's render() returns as `depth` and `alpha`), TSDF fusion of orbit views, and a
triangle mesh by naive surface nets.

    out = render_geometry(cam, gaussians, bg)            # {"render", "depth", "alpha", "radii"}
    vol = fuse_tsdf(gaussians, cameras, resolution=256)
    verts, faces, colors = extract_mesh(vol)
    save_mesh_ply("mesh.ply", verts, faces, colors)

Forward only (everything runs under no_grad); training and the colour rasterizer are untouched: the depth pass reads the intermediates that
rasterize.forward_pass already produces.  There is no fallback: without the library this raises."""
from __future__ import annotations

import ctypes as C
import dataclasses
import os
from typing import Optional, Sequence

import numpy as np
import torch

from ..hip import GsCamera
from ..ops import get_ops
from .cameras import Camera
from .rasterize import forward_pass, gs_camera

LIB_PATH = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "lib", "libv3d_recon.so")
ABI_VERSION = 1
MAX_RESOLUTION = 512

c_i32, c_f32, c_f64, c_vp = C.c_int32, C.c_float, C.c_double, C.c_void_p
_CAM = C.POINTER(GsCamera)

# name -> (restype, argtypes); must list every symbol declared in include/v3d_recon.h (tests/test_recon_geom_cpu.py)
SIGNATURES = {
    "v3d_recon_abi_version": (c_i32, []),
    "v3d_recon_last_error": (C.c_char_p, []),
    "v3d_recon_depth_alpha": (c_i32, [c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_i32, c_i32, c_vp, c_vp, c_vp]),
    "v3d_recon_tsdf_integrate": (c_i32, [c_vp, c_vp, c_vp, _CAM, c_i32, c_f32, c_f32, c_f32, c_vp, c_vp, c_vp, c_vp, c_vp]),
    "v3d_recon_cells_flag": (c_i32, [c_vp, c_vp, c_i32, c_vp, c_vp]),
    "v3d_recon_cells_vertices": (c_i32, [c_vp, c_vp, c_vp, c_vp, c_i32, c_f32, c_vp, c_vp, c_vp, c_vp, c_vp]),
    "v3d_recon_edges_flag": (c_i32, [c_vp, c_vp, c_i32, c_vp, c_vp, c_vp]),
    "v3d_recon_edges_faces": (c_i32, [c_vp, c_vp, c_i32, c_vp, c_vp, c_vp, c_vp, c_vp]),
    # mesh rasterizer (csrc_recon/meshrast.hip, v3d_amd/recon/mesh_render.py)
    "v3d_recon_mesh_project": (c_i32, [c_vp, c_i32, _CAM, c_i32, c_vp, c_vp, c_vp, c_vp]),
    "v3d_recon_mesh_face_setup": (c_i32, [c_vp, c_i32, c_vp, c_vp, c_i32, c_i32, c_i32, c_i32, c_i32, c_vp, c_vp, c_vp]),
    "v3d_recon_mesh_duplicate_keys": (c_i32, [c_vp, c_i32, c_vp, c_i32, c_vp, c_vp, c_vp, c_i32, c_i32, c_i32, c_vp, c_vp, c_vp]),
    "v3d_recon_mesh_tile_ranges": (c_i32, [c_vp, c_i32, c_i32, c_i32, c_vp, c_vp]),
    "v3d_recon_mesh_render": (c_i32, [c_vp, c_vp, c_vp, c_i32, c_vp, c_vp, c_vp, c_vp, _CAM, c_i32, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp]),
    # mesh colour refinement (csrc_recon/meshshade.hip, v3d_amd/recon/mesh_refine.py)
    "v3d_recon_mesh_pixel_weights": (c_i32, [c_vp, c_vp, c_i32, c_vp, c_vp, c_i32, c_i32, c_i32, c_i32, c_vp, c_vp, c_vp]),
    "v3d_recon_mesh_shade": (c_i32, [c_vp, c_vp, c_vp, c_vp, c_i32, c_i32, c_i32, c_f32, c_f32, c_f32, c_vp, c_vp]),
    "v3d_recon_mesh_vertex_records": (c_i32, [c_vp, c_vp, c_i32, c_i32, c_i32, c_vp, c_vp, c_vp]),
    "v3d_recon_mesh_vertex_ranges": (c_i32, [c_vp, c_i32, c_i32, c_vp, c_vp]),
    "v3d_recon_mesh_shade_bwd": (c_i32, [c_vp, c_vp, c_vp, c_i32, c_vp, c_i32, c_i32, c_i32, c_vp, c_vp]),
    "v3d_recon_mesh_color_adam": (c_i32, [c_vp, c_vp, c_vp, c_vp, c_i32, c_f64, c_f64, c_f64, c_f64, c_i32, c_vp, c_vp]),
    # mesh topology (csrc_recon/meshtopo.hip, v3d_amd/recon/mesh_clean.py)
    "v3d_recon_mesh_corner_records": (c_i32, [c_vp, c_i32, c_i32, c_vp, c_vp, c_vp]),
    "v3d_recon_mesh_vertex_normals": (c_i32, [c_vp, c_i32, c_vp, c_i32, c_vp, c_vp, c_vp, c_vp]),
    "v3d_recon_mesh_label_round": (c_i32, [c_vp, c_i32, c_vp, c_vp, c_i32, c_vp, c_vp, c_vp, c_vp]),
    "v3d_recon_mesh_face_labels": (c_i32, [c_vp, c_i32, c_vp, c_i32, c_vp, c_vp, c_vp]),
    "v3d_recon_mesh_keep_flags": (c_i32, [c_vp, c_i32, c_vp, c_vp, c_i32, c_vp, c_vp, c_vp, c_vp, c_vp]),
    "v3d_recon_mesh_compact_faces": (c_i32, [c_vp, c_i32, c_i32, c_vp, c_vp, c_vp, c_vp, c_i32, c_i32, c_vp, c_vp]),
    "v3d_recon_mesh_boundary_flags": (c_i32, [c_vp, c_i32, c_vp, c_vp, c_i32, c_vp, c_vp]),
    "v3d_recon_mesh_smooth_pass": (c_i32, [c_vp, c_i32, c_vp, c_i32, c_vp, c_vp, c_vp, c_f32, c_vp, c_vp]),
    "v3d_recon_mesh_vertex_quadrics": (c_i32, [c_vp, c_i32, c_vp, c_i32, c_vp, c_vp, c_vp, c_vp]),
    "v3d_recon_mesh_decim_propose": (c_i32, [c_vp, c_i32, c_vp, c_i32, c_vp, c_vp, c_vp, c_i32, c_vp, c_vp, c_vp]),
    "v3d_recon_mesh_decim_min_round": (c_i32, [c_vp, c_i32, c_vp, c_vp, c_i32, c_vp, c_vp, c_vp]),
    "v3d_recon_mesh_decim_accept": (c_i32, [c_vp, c_vp, c_i32, c_f32, c_vp, c_vp, c_vp, c_vp, c_vp]),
    "v3d_recon_mesh_decim_cut": (c_i32, [c_vp, c_vp, c_i32, c_vp, c_i32, c_vp, c_vp]),
    "v3d_recon_mesh_decim_apply": (c_i32, [c_vp, c_i32, c_i32, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp]),
    # mesh texture (csrc_recon/meshtex.hip, v3d_amd/recon/mesh_texture.py)
    "v3d_recon_tex_face_uvs": (c_i32, [c_i32, c_i32, c_vp, c_vp]),
    "v3d_recon_tex_bake_vertex_colors": (c_i32, [c_vp, c_i32, c_vp, c_i32, c_i32, c_f32, c_vp, c_vp, c_vp]),
    "v3d_recon_tex_pixel_texels": (c_i32, [c_vp, c_vp, c_i32, c_i32, c_i32, c_i32, c_vp, c_vp, c_vp]),
    "v3d_recon_tex_shade": (c_i32, [c_vp, c_vp, c_vp, c_i32, c_i32, c_i32, c_f32, c_f32, c_f32, c_vp, c_vp]),
    "v3d_recon_tex_texel_records": (c_i32, [c_vp, c_vp, c_i32, c_i32, c_i32, c_vp, c_vp, c_vp]),
    "v3d_recon_tex_shade_bwd": (c_i32, [c_vp, c_vp, c_vp, c_i32, c_vp, c_i32, c_i32, c_i32, c_vp, c_vp]),
    # mesh vertex fit (csrc_recon/meshdeform.hip, v3d_amd/recon/mesh_deform.py)
    "v3d_recon_mesh_aa_alpha": (c_i32, [c_vp, c_vp, c_i32, c_vp, c_vp, c_i32, c_i32, c_i32, c_vp, c_vp, c_vp]),
    "v3d_recon_mesh_aa_count": (c_i32, [c_vp, c_vp, c_i32, c_vp, c_vp, c_i32, c_i32, c_i32, c_vp, c_vp, c_vp]),
    "v3d_recon_mesh_aa_emit": (c_i32, [c_vp, c_vp, c_i32, c_vp, c_vp, c_i32, c_i32, c_i32, c_vp, c_vp, c_vp, c_i32, c_vp, c_vp, c_vp, c_vp]),
    "v3d_recon_mesh_aa_reduce": (c_i32, [c_vp, c_vp, c_vp, c_i32, c_i32, c_vp, c_vp]),
    "v3d_recon_mesh_project_bwd": (c_i32, [c_vp, c_i32, _CAM, c_vp, c_vp, c_vp, c_vp]),
    "v3d_recon_mesh_smooth_grad": (c_i32, [c_vp, c_i32, c_vp, c_i32, c_vp, c_vp, c_f32, c_vp, c_vp]),
    # mesh BVH and normal bake (csrc_recon/meshbvh.hip, v3d_amd/recon/mesh_bake.py)
    "v3d_recon_bvh_face_keys": (c_i32, [c_vp, c_i32, c_vp, c_i32, c_f32, c_f32, c_f32, c_f32, c_f32, c_f32, c_vp, c_vp, c_vp, c_vp, c_vp]),
    "v3d_recon_bvh_build_nodes": (c_i32, [c_vp, c_vp, c_vp, c_vp, c_i32, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp]),
    "v3d_recon_bvh_fit_round": (c_i32, [c_vp, c_vp, c_i32, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp]),
    "v3d_recon_bvh_closest_hit": (c_i32, [c_vp, c_vp, c_f32, c_f32, c_i32, c_i32, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_i32, c_vp, c_i32, c_vp, c_vp,
                                          c_vp, c_vp]),
    "v3d_recon_tex_bake_normals": (c_i32, [c_vp, c_i32, c_vp, c_i32, c_vp, c_i32, c_f32, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_i32, c_vp, c_i32, c_vp,
                                           c_vp, c_vp, c_vp, c_vp, c_vp]),
    # mesh queries (csrc_recon/meshquery.hip, v3d_amd/recon/mesh_query.py)
    "v3d_recon_bvh_closest_point": (c_i32, [c_vp, c_i32, c_f32, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_i32, c_vp, c_i32, c_vp, c_vp, c_vp, c_vp]),
    "v3d_recon_mesh_face_samples": (c_i32, [c_vp, c_i32, c_vp, c_i32, c_i32, c_vp, c_vp, c_vp]),
    "v3d_recon_bvh_occlusion": (c_i32, [c_vp, c_vp, c_i32, c_i32, c_f32, c_f32, C.c_uint32, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_i32, c_vp, c_i32, c_vp,
                                        c_vp]),
    "v3d_recon_tex_texel_frames": (c_i32, [c_vp, c_i32, c_vp, c_i32, c_vp, c_i32, c_vp, c_vp, c_vp, c_vp]),
    # mesh solid (csrc_recon/meshsolid.hip, v3d_amd/recon/mesh_solid.py)
    "v3d_recon_bvh_moment_round": (c_i32, [c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_i32, c_vp, c_i32, c_vp, c_vp, c_vp, c_vp, c_vp]),
    "v3d_recon_bvh_winding": (c_i32, [c_vp, c_i32, c_f32, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_i32, c_vp, c_i32, c_vp, c_vp, c_vp]),
    "v3d_recon_sdf_grid": (c_i32, [c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_i32, c_vp, c_i32, c_vp, c_vp, c_i32, c_f32, c_f32, c_f32, c_vp, c_vp, c_vp, c_vp,
                                   c_vp]),
    # tangent space and GLB (csrc_recon/meshtangent.hip, v3d_amd/recon/mesh_gltf.py)
    "v3d_recon_tex_corner_frames": (c_i32, [c_vp, c_i32, c_vp, c_i32, c_vp, c_vp, c_vp, c_vp]),
    "v3d_recon_tex_encode_tangent": (c_i32, [c_vp, c_i32, c_i32, c_vp, c_vp, c_vp, c_i32, c_vp, c_vp, c_vp]),
    "v3d_recon_tex_decode_tangent": (c_i32, [c_vp, c_i32, c_i32, c_vp, c_vp, c_vp, c_i32, c_vp, c_vp, c_vp]),
    "v3d_recon_tex_shade_lit": (c_i32, [c_vp, c_vp, c_vp, c_vp, c_i32, c_vp, c_vp, c_vp, c_vp, c_vp, c_i32, c_i32, c_i32, c_i32, c_vp, c_vp, c_f32, c_f32,
                                        c_f32, c_f32, c_vp, c_vp, c_vp]),
    # mesh remeshing (csrc_recon/meshremesh.hip, v3d_amd/recon/mesh_remesh.py)
    "v3d_recon_remesh_split_propose": (c_i32, [c_vp, c_i32, c_vp, c_i32, c_vp, c_vp, c_f32, c_i32, c_vp, c_vp, c_vp]),
    "v3d_recon_remesh_split_apply": (c_i32, [c_vp, c_vp, c_i32, c_vp, c_i32, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp]),
    "v3d_recon_remesh_collapse_propose": (c_i32, [c_vp, c_i32, c_vp, c_i32, c_vp, c_vp, c_f32, c_i32, c_vp, c_vp, c_vp]),
    "v3d_recon_remesh_collapse_apply": (c_i32, [c_vp, c_i32, c_i32, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp]),
    "v3d_recon_remesh_flip_propose": (c_i32, [c_vp, c_i32, c_vp, c_i32, c_vp, c_vp, c_vp, c_i32, c_vp, c_vp, c_vp]),
    "v3d_recon_remesh_flip_apply": (c_i32, [c_vp, c_i32, c_i32, c_vp, c_vp, c_vp, c_vp, c_vp]),
    "v3d_recon_remesh_relax": (c_i32, [c_vp, c_i32, c_vp, c_i32, c_vp, c_vp, c_vp, c_vp, c_f32, c_vp, c_vp]),
    "v3d_recon_remesh_project": (c_i32, [c_vp, c_vp, c_vp, c_vp, c_i32, c_vp, c_i32, c_vp, c_vp, c_i32, c_vp]),
    # mesh check (csrc_recon/meshcheck.hip, v3d_amd/recon/mesh_check.py)
    "v3d_recon_bvh_self_count": (c_i32, [c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_i32, c_vp, c_i32, c_vp, c_vp, c_vp]),
    "v3d_recon_bvh_self_emit": (c_i32, [c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_i32, c_vp, c_i32, c_vp, c_i32, c_vp, c_vp]),
    "v3d_recon_mesh_edge_census": (c_i32, [c_vp, c_i32, c_vp, c_vp, c_i32, c_vp, c_vp, c_vp]),
    "v3d_recon_mesh_vertex_census": (c_i32, [c_vp, c_i32, c_vp, c_vp, c_i32, c_vp, c_vp]),
    # mesh repair (csrc_recon/meshrepair.hip, v3d_amd/recon/mesh_repair.py)
    "v3d_recon_repair_weld_keys": (c_i32, [c_vp, c_i32, c_vp, c_vp, c_vp, c_vp]),
    "v3d_recon_repair_weld_heads": (c_i32, [c_vp, c_i32, c_vp, c_vp, c_vp]),
    "v3d_recon_repair_weld_first": (c_i32, [c_vp, c_vp, c_vp, c_i32, c_vp, c_vp]),
    "v3d_recon_repair_weld_remap": (c_i32, [c_vp, c_vp, c_vp, c_i32, c_vp, c_vp]),
    "v3d_recon_repair_remap_faces": (c_i32, [c_vp, c_i32, c_i32, c_vp, c_vp, c_vp]),
    "v3d_recon_repair_drop_flags": (c_i32, [c_vp, c_i32, c_vp, c_i32, c_vp, c_vp, c_vp, c_vp]),
    "v3d_recon_repair_orient_round": (c_i32, [c_vp, c_i32, c_vp, c_vp, c_i32, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp]),
    "v3d_recon_repair_orient_conflicts": (c_i32, [c_vp, c_i32, c_vp, c_vp, c_i32, c_vp, c_vp, c_vp, c_vp, c_vp]),
    "v3d_recon_repair_orient_apply": (c_i32, [c_vp, c_i32, c_vp, c_vp, c_vp, c_vp, c_vp]),
    "v3d_recon_repair_vertex_open": (c_i32, [c_vp, c_i32, c_vp, c_vp, c_i32, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp]),
    "v3d_recon_repair_trouble": (c_i32, [c_vp, c_i32, c_i32, c_vp, c_vp, c_vp, c_vp]),
    "v3d_recon_repair_grow": (c_i32, [c_vp, c_i32, c_vp, c_vp, c_i32, c_vp, c_vp, c_vp]),
    "v3d_recon_repair_loop_round": (c_i32, [c_i32, c_vp, c_vp, c_vp, c_vp, c_vp]),
    "v3d_recon_repair_loop_flags": (c_i32, [c_i32, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_i32, c_vp, c_vp, c_vp]),
    "v3d_recon_repair_fill_emit": (c_i32, [c_vp, c_vp, c_i32, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_i32, c_i32, c_vp, c_vp, c_vp, c_vp]),
    # mesh alignment (csrc_recon/meshalign.hip, v3d_amd/recon/mesh_align.py)
    "v3d_recon_align_correspond": (c_i32, [c_vp, c_vp, c_i32, c_vp, c_f32, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_i32, c_vp, c_i32, c_vp, c_vp, c_vp, c_vp,
                                           c_vp, c_vp, c_vp]),
    "v3d_recon_align_reduce": (c_i32, [c_vp, c_i32, c_vp, c_vp]),
}

_lib = None


def load_library(path: Optional[str] = None) -> C.CDLL:
    """dlopen libv3d_recon.so and bind every declared symbol (no GPU needed for this step)."""
    global _lib
    if path is None and _lib is not None:
        return _lib
    p = path or LIB_PATH
    if not os.path.exists(p):
        raise RuntimeError(f"{p} not found: the geometry library is not built. Run `python -m v3d_amd.build`. There is no fallback.")
    lib = C.CDLL(p)
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = res, args
    v = lib.v3d_recon_abi_version()
    if v != ABI_VERSION:
        raise RuntimeError(f"libv3d_recon.so ABI version {v} != expected {ABI_VERSION}; rebuild")
    if path is None:
        _lib = lib
    return lib


def _check(lib, rc: int, what: str):
    if rc != 0:
        msg = lib.v3d_recon_last_error()
        raise RuntimeError(f"{what} failed (rc={rc}): {msg.decode() if msg else ''}")


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _f32(t: torch.Tensor, what: str) -> torch.Tensor:
    if t.device.type != "cuda" or t.dtype != torch.float32:
        raise RuntimeError(f"{what}: expected a float32 tensor in device memory, got {t.dtype} on {t.device}")
    return t.contiguous()


# ---- depth / alpha ------------------------------------------------------------------------------------------------------------------
def depth_alpha(st: dict, width: int, height: int):
    """(depth [H, W], alpha [H, W]) of the view whose forward intermediates `st` are (rasterize.forward_pass)."""
    lib = load_library()
    dev = st["means2d"].device
    depth = torch.zeros(height, width, dtype=torch.float32, device=dev)
    alpha = torch.zeros(height, width, dtype=torch.float32, device=dev)
    vals = st["vals_s"]
    _check(lib, lib.v3d_recon_depth_alpha(st["ranges"].data_ptr(), vals.data_ptr() if vals.numel() else None, st["means2d"].data_ptr(),
                                          st["conic_opacity"].data_ptr(), st["depth"].data_ptr(), st["n_contrib"].data_ptr(), width, height,
                                          depth.data_ptr(), alpha.data_ptr(), _stream()), "v3d_recon_depth_alpha")
    return depth, alpha


@torch.no_grad()
def render_geometry(camera: Camera, gaussians, bg):
    """{"render": image [3, H, W], "depth": sum alpha_i T_i z_i [H, W] (not divided by alpha, as the reference's rasterizer returns it),
    "alpha": 1 - T [H, W], "radii" [P]} of one view.  The maps end at the colour image's last contributor of every pixel."""
    xyz = gaussians.xyz.detach()
    dev = xyz.device
    H, W = int(camera.height), int(camera.width)
    if xyz.shape[0] == 0:       # every Gaussian pruned: background, nothing in front of it (the kernels take P >= 1)
        bgt = torch.as_tensor(bg, dtype=torch.float32, device=dev)
        return {"render": bgt.view(3, 1, 1).expand(3, H, W).contiguous(), "depth": torch.zeros(H, W, device=dev),
                "alpha": torch.zeros(H, W, device=dev), "radii": torch.zeros(0, dtype=torch.int32, device=dev)}
    gc = gs_camera(camera, bg)
    img, st = forward_pass(get_ops(), xyz.contiguous(), gaussians.scaling.detach().contiguous(), gaussians.rotation.detach().contiguous(),
                           gaussians.opacity.detach().contiguous(), gaussians.features_dc.detach().contiguous(), gc)
    depth, alpha = depth_alpha(st, W, H)
    return {"render": img, "depth": depth, "alpha": alpha, "radii": st["radii"]}


def normalised_depth(depth: torch.Tensor, alpha: torch.Tensor, alpha_min: float = 0.5) -> torch.Tensor:
    """Expected depth depth / alpha where alpha >= alpha_min, mapped to [0, 1] over its own range (near = 1), 0 elsewhere."""
    hit = alpha >= alpha_min
    out = torch.zeros_like(depth)
    if bool(hit.any()):
        d = depth[hit] / alpha[hit]
        lo, hi = d.min(), d.max()
        out[hit] = 1.0 - (d - lo) / (hi - lo).clamp_min(1e-12)
    return out


# ---- TSDF ---------------------------------------------------------------------------------------------------------------------------
@dataclasses.dataclass
class TsdfVolume:
    """N^3 voxels, axis-aligned, centred at the origin, half-extent `bound`; voxel (ix, iy, iz) is element [iz, iy, ix]."""
    resolution: int
    bound: float
    trunc: float
    tsdf_sum: torch.Tensor      # [N, N, N]
    weight: torch.Tensor        # [N, N, N]
    rgb_sum: torch.Tensor       # [3, N, N, N]
    rgb_weight: torch.Tensor    # [N, N, N]

    @property
    def voxel(self) -> float:
        return 2.0 * self.bound / self.resolution


def _check_resolution(resolution: int):
    if not 2 <= int(resolution) <= MAX_RESOLUTION:
        raise ValueError(f"resolution {resolution} outside 2 .. {MAX_RESOLUTION} (voxel indices are int32)")


def new_volume(resolution: int, bound: float, trunc: Optional[float] = None, device="cuda") -> TsdfVolume:
    _check_resolution(resolution)
    N = int(resolution)
    if not bound > 0:
        raise ValueError(f"bound {bound} must be positive")
    trunc = 4.0 * 2.0 * bound / N if trunc is None else float(trunc)
    z = lambda *s: torch.zeros(*s, dtype=torch.float32, device=device)  # noqa: E731
    return TsdfVolume(N, float(bound), trunc, z(N, N, N), z(N, N, N), z(3, N, N, N), z(N, N, N))


def integrate_view(vol: TsdfVolume, depth: torch.Tensor, alpha: torch.Tensor, image: torch.Tensor, camera: Camera, alpha_min: float = 0.5):
    """One view (depth [H, W] un-normalised, alpha [H, W], image [3, H, W]) into the volume, in place."""
    lib = load_library()
    H, W = int(camera.height), int(camera.width)
    depth, alpha, image = _f32(depth, "depth"), _f32(alpha, "alpha"), _f32(image, "image")
    if tuple(depth.shape) != (H, W) or tuple(alpha.shape) != (H, W) or tuple(image.shape) != (3, H, W):
        raise ValueError(f"integrate_view: maps {tuple(depth.shape)}, {tuple(alpha.shape)}, {tuple(image.shape)} do not match the {W} x {H} camera")
    gc = gs_camera(camera, [0.0, 0.0, 0.0])
    _check(lib, lib.v3d_recon_tsdf_integrate(depth.data_ptr(), alpha.data_ptr(), image.data_ptr(), C.byref(gc), vol.resolution, vol.bound, vol.trunc,
                                             float(alpha_min), vol.tsdf_sum.data_ptr(), vol.weight.data_ptr(), vol.rgb_sum.data_ptr(),
                                             vol.rgb_weight.data_ptr(), _stream()), "v3d_recon_tsdf_integrate")


def default_bound(gaussians) -> float:
    """1.1 x the largest |coordinate| over the Gaussians with opacity >= 0.5 (over all of them when none is that opaque)."""
    xyz = gaussians.xyz.detach()
    if xyz.shape[0] == 0:
        return 1.0
    solid = torch.sigmoid(gaussians.opacity.detach()).reshape(-1) >= 0.5
    pts = xyz[solid] if bool(solid.any()) else xyz
    return 1.1 * float(pts.abs().max())


@torch.no_grad()
def fuse_tsdf(gaussians, cameras: Sequence[Camera], resolution: int = 256, bound: Optional[float] = None, trunc: Optional[float] = None,
              alpha_min: float = 0.5, bg=(1.0, 1.0, 1.0)) -> TsdfVolume:
    """Render depth, alpha and colour of every camera and integrate them, in camera order, into a fresh volume."""
    _check_resolution(resolution)
    dev = gaussians.xyz.device
    vol = new_volume(resolution, default_bound(gaussians) if bound is None else bound, trunc, dev)
    bgt = torch.as_tensor(bg, dtype=torch.float32, device=dev)
    for cam in cameras:
        out = render_geometry(cam, gaussians, bgt)
        integrate_view(vol, out["depth"], out["alpha"], out["render"], cam, alpha_min)
    return vol


# ---- surface nets -------------------------------------------------------------------------------------------------------------------
@torch.no_grad()
def extract_mesh(vol: TsdfVolume):
    """(verts [V, 3] float32, faces [F, 3] int32, colors [V, 3] float32 in 0 .. 1) on the volume's device.  One vertex per cell whose 8 corners
    were all observed and whose mean TSDF changes sign, in linear cell order; two triangles per sign-changing interior grid edge whose 4
    cells all have a vertex, in linear edge order, normals pointing from inside (negative) to outside."""
    lib, ops = load_library(), get_ops()
    N = vol.resolution
    _check_resolution(N)
    dev = vol.tsdf_sum.device
    ts, w, rs, rw = (_f32(t, n) for t, n in ((vol.tsdf_sum, "tsdf_sum"), (vol.weight, "weight"), (vol.rgb_sum, "rgb_sum"), (vol.rgb_weight, "rgb_weight")))
    empty = (torch.zeros(0, 3, dtype=torch.float32, device=dev), torch.zeros(0, 3, dtype=torch.int32, device=dev),
             torch.zeros(0, 3, dtype=torch.float32, device=dev))
    cflags = torch.empty((N - 1) ** 3, dtype=torch.int32, device=dev)
    _check(lib, lib.v3d_recon_cells_flag(ts.data_ptr(), w.data_ptr(), N, cflags.data_ptr(), _stream()), "v3d_recon_cells_flag")
    coffs = ops.gs_scan(cflags)
    nv = int(coffs[-1].item())
    if nv == 0:
        return empty
    verts = torch.empty(nv, 3, dtype=torch.float32, device=dev)
    colors = torch.empty(nv, 3, dtype=torch.float32, device=dev)
    _check(lib, lib.v3d_recon_cells_vertices(ts.data_ptr(), w.data_ptr(), rs.data_ptr(), rw.data_ptr(), N, vol.bound, cflags.data_ptr(),
                                             coffs.data_ptr(), verts.data_ptr(), colors.data_ptr(), _stream()), "v3d_recon_cells_vertices")
    eflags = torch.empty(3 * N ** 3, dtype=torch.int32, device=dev)
    _check(lib, lib.v3d_recon_edges_flag(ts.data_ptr(), w.data_ptr(), N, cflags.data_ptr(), eflags.data_ptr(), _stream()), "v3d_recon_edges_flag")
    eoffs = ops.gs_scan(eflags)
    ne = int(eoffs[-1].item())
    if ne == 0:
        return verts, empty[1], colors
    faces = torch.empty(2 * ne, 3, dtype=torch.int32, device=dev)
    _check(lib, lib.v3d_recon_edges_faces(ts.data_ptr(), w.data_ptr(), N, coffs.data_ptr(), eflags.data_ptr(), eoffs.data_ptr(), faces.data_ptr(),
                                          _stream()), "v3d_recon_edges_faces")
    return verts, faces, colors


# ---- mesh PLY -----------------------------------------------------------------------------------------------------------------------
_VERT = np.dtype([("x", "<f4"), ("y", "<f4"), ("z", "<f4"), ("red", "u1"), ("green", "u1"), ("blue", "u1")])
_FACE = np.dtype([("n", "u1"), ("v", "<i4", (3,))])
_HEAD = ["property float x", "property float y", "property float z", "property uchar red", "property uchar green", "property uchar blue"]


def _np(a, dtype):
    return np.ascontiguousarray(a.detach().cpu().numpy() if torch.is_tensor(a) else a, dtype=dtype)


def save_mesh_ply(path: str, verts, faces, colors):
    """Binary little-endian PLY: vertices x y z (float) red green blue (uchar, colours in 0 .. 1 rounded to 0 .. 255), faces as
    `list uchar int vertex_indices`."""
    v, f, c = _np(verts, np.float32).reshape(-1, 3), _np(faces, np.int32).reshape(-1, 3), _np(colors, np.float32).reshape(-1, 3)
    if c.shape != v.shape:
        raise ValueError(f"save_mesh_ply: {v.shape[0]} vertices, {c.shape[0]} colours")
    if f.size and (f.min() < 0 or f.max() >= v.shape[0]):
        raise ValueError("save_mesh_ply: face index outside the vertex array")
    d = os.path.dirname(path)
    if d:
        os.makedirs(d, exist_ok=True)
    vr = np.empty(v.shape[0], dtype=_VERT)
    vr["x"], vr["y"], vr["z"] = v[:, 0], v[:, 1], v[:, 2]
    c8 = np.rint(np.clip(c, 0.0, 1.0) * 255.0).astype(np.uint8)
    vr["red"], vr["green"], vr["blue"] = c8[:, 0], c8[:, 1], c8[:, 2]
    fr = np.empty(f.shape[0], dtype=_FACE)
    fr["n"], fr["v"] = 3, f
    head = ["ply", "format binary_little_endian 1.0", f"element vertex {v.shape[0]}", *_HEAD, f"element face {f.shape[0]}",
            "property list uchar int vertex_indices", "end_header"]
    with open(path, "wb") as fh:
        fh.write(("\n".join(head) + "\n").encode("ascii"))
        fh.write(vr.tobytes())
        fh.write(fr.tobytes())


def read_mesh_ply(path: str):
    """(verts [V, 3] float32, faces [F, 3] int32, colors [V, 3] uint8) of a file save_mesh_ply wrote."""
    with open(path, "rb") as fh:
        raw = fh.read()
    end = raw.find(b"end_header\n")
    if not raw.startswith(b"ply\n") or end < 0:
        raise ValueError(f"{path}: not a PLY file")
    lines = raw[:end].decode("ascii").splitlines()
    if "format binary_little_endian 1.0" not in lines:
        raise ValueError(f"{path}: only binary little-endian PLY is supported")
    counts = {ln.split()[1]: int(ln.split()[2]) for ln in lines if ln.startswith("element ")}
    props = [ln for ln in lines if ln.startswith("property ")]
    if list(counts) != ["vertex", "face"] or props != _HEAD + ["property list uchar int vertex_indices"]:
        raise ValueError(f"{path}: not the vertex / face layout save_mesh_ply writes")
    body = raw[end + len(b"end_header\n"):]
    nv, nf = counts["vertex"], counts["face"]
    if len(body) != nv * _VERT.itemsize + nf * _FACE.itemsize:
        raise ValueError(f"{path}: body of {len(body)} bytes does not hold {nv} vertices and {nf} triangles")
    vr = np.frombuffer(body, dtype=_VERT, count=nv)
    fr = np.frombuffer(body, dtype=_FACE, count=nf, offset=nv * _VERT.itemsize)
    if nf and not (fr["n"] == 3).all():
        raise ValueError(f"{path}: a face is not a triangle")
    verts = np.stack([vr["x"], vr["y"], vr["z"]], 1).astype(np.float32)
    colors = np.stack([vr["red"], vr["green"], vr["blue"]], 1).astype(np.uint8)
    return verts, fr["v"].astype(np.int32).reshape(-1, 3), colors


# ---- orbit helpers of scripts/pub/recon_from_vid.py -----------------------------------------------------------------------------------
@torch.no_grad()
def render_depth_orbit(gaussians, n: int, radius: float, elevation: float, fov: float, reso: int, white_background: bool = True) -> np.ndarray:
    """n turntable frames of normalised depth (normalised_depth), float32 [n, reso, reso] on the host."""
    from .cameras import orbit_cameras
    cams, _ = orbit_cameras(n, radius, elevation, fov, reso)
    bg = [1.0, 1.0, 1.0] if white_background else [0.0, 0.0, 0.0]
    frames = []
    for c in cams:
        out = render_geometry(c, gaussians, bg)
        frames.append(normalised_depth(out["depth"], out["alpha"]).cpu())
    return torch.stack(frames).numpy().astype(np.float32)
