#!/usr/bin/env python
"""Export the baked mesh as one self-contained GLB (glTF 2.0 binary) that any glTF loader opens (v3d_amd/recon/mesh_gltf.py): the albedo,
the normal map converted on the GPU from the project's object space to glTF's tangent space, with per-corner NORMAL and TANGENT frames, and
the ambient-occlusion map, all on the per-face atlas.

    python scripts/pub/export_glb.py --mesh out/gs/mesh_50k_ao.obj -o out/gs/mesh_50k.glb [--high out/gs/mesh_clean.ply] [--render_orbit 36]

--mesh is an OBJ of texture_mesh.py, bake_normals.py or bake_ao.py: its texture and resolution are kept, the 8-bit object-space normal map
its MTL names on a `norm` line is decoded and converted, and the occlusion map of a `map_Ka` line goes in as it is.  An OBJ without a normal
map, or a PLY (its vertex colours baked as the albedo at --texture_resolution, as texture_mesh.py bakes them), still exports, without a
normalTexture.  With --high (the mesh before decimation, a PLY) the normal map is baked again in float (mesh_bake.bake_normal_map) before it
is converted, instead of starting from the 8-bit PNG (--max_dist as bake_normals.py), and the mean angle to the high mesh's normals over
--views orbit views is reported for the object-space map and for the tangent-space map.  Prints one line with the face count, the file's
size and the maps that went in; --json writes the figures.  --render_orbit N also writes N lit turntable frames, shaded from exactly what
the GLB carries (one key and one fill light fixed to the camera, plus ambient; --reso, --radius, --elevation, --fov), to
<out without .glb>_lit_orbit/."""
from __future__ import annotations

import argparse
import json
import math
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
for _p in (ROOT, os.path.dirname(os.path.abspath(__file__))):
    if _p not in sys.path:
        sys.path.insert(0, _p)

MAX_TEXTURE = 4096


def build_parser() -> argparse.ArgumentParser:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--mesh", required=True, help="the baked mesh: an OBJ of texture_mesh.py, bake_normals.py or bake_ao.py, or a PLY")
    ap.add_argument("-o", "--out", default=None, help="the GLB (default: <mesh without its suffix>.glb)")
    ap.add_argument("--high", default=None, help="the mesh before decimation, a PLY: bake the normal map again in float and report the angles")
    ap.add_argument("-w", "--white_background", action="store_true")
    ap.add_argument("--texture_resolution", type=int, default=1024, help=f"texels on a side for a PLY input, up to {MAX_TEXTURE}")
    ap.add_argument("--max_dist", type=float, default=None, help="with --high: how far a texel looks (default: 0.05 x the high mesh's diagonal)")
    ap.add_argument("--views", type=int, default=8, help="with --high: orbit views the angles are measured over (0: none)")
    ap.add_argument("--reso", type=int, default=512)
    ap.add_argument("--radius", type=float, default=2.0)
    ap.add_argument("--elevation", type=float, default=0.0)
    ap.add_argument("--fov", type=float, default=60.0)
    ap.add_argument("--render_orbit", type=int, default=0, help="write N lit turntable frames of the mesh")
    ap.add_argument("--json", default=None, help="write the figures here")
    return ap


def check_args(ap: argparse.ArgumentParser, a):
    if a.render_orbit < 0:
        ap.error("--render_orbit must not be negative")
    if a.views < 0:
        ap.error("--views must not be negative")
    if not 1 <= a.texture_resolution <= MAX_TEXTURE:
        ap.error(f"--texture_resolution {a.texture_resolution} outside 1 .. {MAX_TEXTURE}")
    if not 1 <= a.reso <= 4096:
        ap.error(f"--reso {a.reso} outside 1 .. 4096")
    if a.max_dist is not None and not (a.max_dist >= 0 and math.isfinite(a.max_dist)):
        ap.error(f"--max_dist {a.max_dist} must be finite and not negative")
    if a.out is not None and not a.out.lower().endswith(".glb"):
        ap.error(f"-o {a.out}: the output is a GLB")
    if a.json is not None and not a.json.lower().endswith(".json"):
        ap.error(f"--json {a.json}: a .json file")
    if not a.mesh.lower().endswith((".obj", ".ply")):
        ap.error(f"--mesh {a.mesh}: an OBJ or a PLY")
    if a.high is not None and not a.high.lower().endswith(".ply"):
        ap.error(f"--high {a.high}: a PLY")


def map_of(obj_path: str, key: str):
    """the path of the image the OBJ's MTL names on a `key` line (`norm`, `map_Ka`), or None: bake_ao.normal_map_of for any key"""
    from bake_ao import _rest
    mtl = None
    with open(obj_path) as fh:
        for line in fh:
            mtl = _rest(line, "mtllib")
            if mtl is not None:
                break
    if mtl is None:
        return None
    with open(os.path.join(os.path.dirname(obj_path), mtl)) as fh:
        for line in fh:
            png = _rest(line, key)
            if png is not None:
                return os.path.join(os.path.dirname(obj_path), png)
    return None


def decode_normal_png(path: str, R: int) -> np.ndarray:
    """[R*R, 3] float32 unit vectors of an 8-bit 0.5 n + 0.5 image; (0, 0, 1) where nothing is left"""
    from PIL import Image
    img = np.asarray(Image.open(path).convert("RGB"))
    if img.shape[:2] != (R, R):
        raise SystemExit(f"{path}: {img.shape[1]} x {img.shape[0]} beside a texture of {R} x {R}")
    n = img.reshape(-1, 3).astype(np.float64) / 255.0 * 2.0 - 1.0
    length = np.linalg.norm(n, axis=1, keepdims=True)
    return np.where(length > 1e-10, n / np.maximum(length, 1e-10), np.array([0.0, 0.0, 1.0])).astype(np.float32)


def main(argv=None):
    ap = build_parser()
    a = ap.parse_args(argv)
    check_args(ap, a)
    from recon_from_vid import save_frames
    from render_mesh import strict_json
    from v3d_amd.recon import geometry, mesh_bake, mesh_gltf, mesh_texture
    norm_png = ao_png = None
    if a.mesh.lower().endswith(".obj"):
        verts, faces, _, texture = mesh_texture.read_textured_obj(a.mesh)
        R = int(round(texture.shape[0] ** 0.5))
        norm_png, ao_png = map_of(a.mesh, "norm"), map_of(a.mesh, "map_Ka")
        for png in (norm_png, ao_png):
            if png is not None and not os.path.isfile(png):             # before anything is converted or written
                raise SystemExit(f"{a.mesh}: its MTL names {png}, which is not there")
    else:
        verts, faces, colors8 = geometry.read_mesh_ply(a.mesh)
        R = a.texture_resolution
        texture = None
    out = a.out or os.path.splitext(a.mesh)[0] + ".glb"
    stem = os.path.splitext(out)[0]
    F = faces.shape[0]
    if F:
        try:
            mesh_texture.atlas_layout(F, R)
        except ValueError as e:
            raise SystemExit(f"{a.mesh}: {e}; decimate the mesh or raise --texture_resolution")
    stats = {"faces": int(F), "vertices": int(verts.shape[0]), "tex_size": int(R), "normal_source": None}
    if texture is None:
        _, texture = mesh_texture.bake_vertex_colors(faces, colors8.astype(np.float32) / 255.0, R)
    object_map = None
    if a.high is not None and F:
        hverts, hfaces, _ = geometry.read_mesh_ply(a.high)
        if hfaces.shape[0] == 0:
            raise SystemExit(f"{a.high}: no faces to bake from")
        object_map, bake = mesh_bake.bake_normal_map(verts, faces, hverts, hfaces, tex_size=R, max_dist=a.max_dist)
        stats.update(normal_source="float bake", missed=bake["missed"], owned=bake["owned"])
    elif norm_png is not None:
        object_map = decode_normal_png(norm_png, R)
        stats["normal_source"] = "8-bit map"
    cn, ct = mesh_gltf.corner_frames(verts, faces)
    tangent_map = mesh_gltf.to_tangent_space(verts, faces, object_map, R) if object_map is not None and F else None
    ao_map = None
    if ao_png is not None:
        from PIL import Image
        ao_img = np.asarray(Image.open(ao_png).convert("L"))
        if ao_img.shape != (R, R):
            raise SystemExit(f"{ao_png}: {ao_img.shape[1]} x {ao_img.shape[0]} beside a texture of {R} x {R}")
        ao_map = ao_img.reshape(-1).astype(np.float32) / 255.0
    size = mesh_gltf.save_glb(out, verts, faces, texture, tangent_map=tangent_map, ao_map=ao_map, tex_size=R, corner_normals=cn, corner_tangents=ct)
    maps = ["albedo"] + (["normal (tangent space)"] if tangent_map is not None else []) + (["occlusion"] if ao_map is not None else [])
    stats.update(bytes=int(size), maps=maps)
    print(f"[glb] {a.mesh}: {F} triangles as {3 * F} vertices, maps {R} x {R}: {', '.join(maps)}; {size} bytes -> {out}")
    if a.high is not None and F and a.views:
        from v3d_amd.recon.cameras import orbit_cameras
        cams, _ = orbit_cameras(a.views, a.radius, a.elevation, a.fov, a.reso)
        obj = mesh_bake.normal_map_fidelity(verts, faces, object_map, hverts, hfaces, cams)
        tan = mesh_gltf.tangent_map_fidelity(verts, faces, tangent_map, hverts, hfaces, cams)
        stats.update(angle_vertex=obj["angle_before_mean"], angle_object=obj["angle_after_mean"], angle_tangent=tan["angle_after_mean"])
        print(f"[glb] mean angle to the high mesh's normals over {a.views} views: vertex normals {stats['angle_vertex']:.3f}, object-space map "
              f"{stats['angle_object']:.3f}, tangent-space map {stats['angle_tangent']:.3f} degrees")
    if a.json:
        with open(a.json, "w") as fh:
            json.dump(strict_json(stats), fh, indent=1, allow_nan=False)
            fh.write("\n")
    if a.render_orbit:
        orbit = mesh_gltf.render_lit_orbit(verts, faces, texture, tangent_map, ao_map, a.render_orbit, a.radius, a.elevation, a.fov, a.reso,
                                           a.white_background)
        save_frames(orbit, stem + "_lit_orbit")
        print(f"[glb] {a.render_orbit} lit turntable frames at {a.reso} x {a.reso} -> {stem}_lit_orbit")


if __name__ == "__main__":
    main()
