#!/usr/bin/env python
"""Bake an ambient-occlusion map of the full mesh onto the decimated one (v3d_amd/recon/mesh_query.py): a BVH of the high mesh built on the
GPU, every texel of the low mesh's per-face atlas finds its point of the high mesh as bake_normals.py does and casts a cosine-weighted
hemisphere of rays from there; the share that gets away is the texel's value.  Written as OBJ + MTL + PNG with <out>_ao.png (8-bit grey)
beside the albedo and a `map_Ka` line in the MTL.

    python scripts/pub/bake_ao.py --mesh out/gs/mesh_50k_nm.obj --high out/gs/mesh_clean.ply -o out/gs/mesh_50k_ao.obj [--samples 64] [--render_orbit 36]

--mesh is the low mesh: an OBJ of texture_mesh.py or bake_normals.py keeps its texture and its resolution (--texture_resolution is then
ignored), and a normal map its MTL names is kept too: the PNG is copied under the new name and the `norm` line written; a PLY gets its
vertex colours baked as the albedo at --texture_resolution (1024).  --high is the mesh before decimation.  --samples rays per texel
(1 .. 1024) of length --ao_radius (default: 0.1 x the diagonal of the high mesh's bounding box), starting --ao_bias above the surface
(default: 1e-4 x the diagonal); --max_dist is how far a texel looks for the high surface (default: 0.05 x the diagonal).  Prints one line
with the map's statistics and writes them as <out without .obj>_ao.json.  --render_orbit N also writes N turntable frames of the mesh with
the map as a grey texture (--reso, --radius, --elevation, --fov) to <out without .obj>_ao_orbit/."""
from __future__ import annotations

import argparse
import json
import math
import os
import shutil
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
for _p in (ROOT, os.path.dirname(os.path.abspath(__file__))):
    if _p not in sys.path:
        sys.path.insert(0, _p)

MAX_TEXTURE = 4096
MAX_SAMPLES = 1024


def build_parser() -> argparse.ArgumentParser:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--mesh", required=True, help="the low mesh: an OBJ of texture_mesh.py or bake_normals.py, or a PLY (decimate_mesh.py's output)")
    ap.add_argument("--high", required=True, help="the high mesh, a PLY (the mesh before decimation)")
    ap.add_argument("-o", "--out", default=None, help="the OBJ (default: <mesh without its suffix>_ao.obj); .mtl and the .png files go beside it")
    ap.add_argument("-w", "--white_background", action="store_true")
    ap.add_argument("--texture_resolution", type=int, default=1024, help=f"texels on a side for a PLY input, up to {MAX_TEXTURE}")
    ap.add_argument("--samples", type=int, default=64, help=f"rays per texel, 1 .. {MAX_SAMPLES}")
    ap.add_argument("--ao_radius", type=float, default=None, help="how long a ray is (default: 0.1 x the high mesh's diagonal)")
    ap.add_argument("--ao_bias", type=float, default=None, help="how far above the surface a ray starts (default: 1e-4 x the high mesh's diagonal)")
    ap.add_argument("--max_dist", type=float, default=None, help="how far a texel looks for the high surface (default: 0.05 x the high mesh's diagonal)")
    ap.add_argument("--reso", type=int, default=512)
    ap.add_argument("--radius", type=float, default=2.0)
    ap.add_argument("--elevation", type=float, default=0.0)
    ap.add_argument("--fov", type=float, default=60.0)
    ap.add_argument("--render_orbit", type=int, default=0, help="write N turntable frames of the mesh with the map as a grey texture")
    return ap


def check_args(ap: argparse.ArgumentParser, a):
    if a.render_orbit < 0:
        ap.error("--render_orbit must not be negative")
    if not 1 <= a.texture_resolution <= MAX_TEXTURE:
        ap.error(f"--texture_resolution {a.texture_resolution} outside 1 .. {MAX_TEXTURE}")
    if not 1 <= a.samples <= MAX_SAMPLES:
        ap.error(f"--samples {a.samples} outside 1 .. {MAX_SAMPLES}")
    if not 1 <= a.reso <= 4096:
        ap.error(f"--reso {a.reso} outside 1 .. 4096")
    if a.ao_radius is not None and not (a.ao_radius > 0 and math.isfinite(a.ao_radius)):
        ap.error(f"--ao_radius {a.ao_radius} must be finite and positive")
    if a.ao_bias is not None and not (a.ao_bias >= 0 and math.isfinite(a.ao_bias)):
        ap.error(f"--ao_bias {a.ao_bias} must be finite and not negative")
    if a.max_dist is not None and not (a.max_dist >= 0 and math.isfinite(a.max_dist)):
        ap.error(f"--max_dist {a.max_dist} must be finite and not negative")
    if a.out is not None and not a.out.lower().endswith(".obj"):
        ap.error(f"-o {a.out}: the output is an OBJ")
    if not a.mesh.lower().endswith((".obj", ".ply")):
        ap.error(f"--mesh {a.mesh}: an OBJ or a PLY")


def _rest(line: str, key: str):
    """what follows `key` on a line of an OBJ or MTL, spaces in a file name included; None on any other line"""
    p = line.split(None, 1)
    return p[1].strip() if len(p) == 2 and p[0] == key and p[1].strip() else None


def normal_map_of(obj_path: str):
    """the path of the PNG the OBJ's MTL names on a `norm` line, or None"""
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
            png = _rest(line, "norm")
            if png is not None:
                return os.path.join(os.path.dirname(obj_path), png)
    return None


def keep_normal_map(src_png: str, stem: str):
    """The input's normal map under the output's name, byte for byte, and its `norm` line between map_Kd and map_Ka (where
    save_textured_obj puts it)"""
    dst = stem + "_normal.png"
    if os.path.abspath(src_png) != os.path.abspath(dst):
        shutil.copyfile(src_png, dst)
    name = os.path.basename(stem)
    with open(stem + ".mtl") as fh:
        lines = fh.read().splitlines()
    at = next((k for k, line in enumerate(lines) if line.startswith("map_Ka ")), len(lines))
    lines.insert(at, f"norm {name}_normal.png")
    with open(stem + ".mtl", "w") as fh:
        fh.write("\n".join(lines) + "\n")


def main(argv=None):
    ap = build_parser()
    a = ap.parse_args(argv)
    check_args(ap, a)
    from recon_from_vid import save_frames
    from render_mesh import strict_json
    from v3d_amd.recon import geometry, mesh_query, mesh_texture
    norm_png = None
    if a.mesh.lower().endswith(".obj"):
        verts, faces, vt, texture = mesh_texture.read_textured_obj(a.mesh)
        R = int(round(texture.shape[0] ** 0.5))
        norm_png = normal_map_of(a.mesh)
        if norm_png is not None and not os.path.isfile(norm_png):           # before anything is baked or written
            raise SystemExit(f"{a.mesh}: its MTL names the normal map {norm_png}, which is not there")
    else:
        verts, faces, colors8 = geometry.read_mesh_ply(a.mesh)
        R = a.texture_resolution
        vt = texture = None
    hverts, hfaces, _ = geometry.read_mesh_ply(a.high)
    out = a.out or os.path.splitext(a.mesh)[0] + "_ao.obj"
    stem = os.path.splitext(out)[0]
    if faces.shape[0]:
        try:
            mesh_texture.atlas_layout(faces.shape[0], R)
        except ValueError as e:
            raise SystemExit(f"{a.mesh}: {e}; decimate the mesh or raise --texture_resolution")
    if hfaces.shape[0] == 0:
        raise SystemExit(f"{a.high}: no faces to bake from")
    print(f"[ao] {a.mesh}: {verts.shape[0]} vertices, {faces.shape[0]} triangles; {a.high}: {hverts.shape[0]} vertices, {hfaces.shape[0]} triangles; "
          f"map {R} x {R}, {a.samples} rays per texel")
    if texture is None:
        _, texture = mesh_texture.bake_vertex_colors(faces, colors8.astype(np.float32) / 255.0, R)
        vt = mesh_texture.face_uvs(faces.shape[0], R)
    ao_map, stats = mesh_query.bake_ambient_occlusion(verts, faces, hverts, hfaces, tex_size=R, samples=a.samples, radius=a.ao_radius, bias=a.ao_bias,
                                                      max_dist=a.max_dist)
    mesh_texture.save_textured_obj(out, verts, faces, vt, texture, ao_map=ao_map)
    if norm_png is not None:
        keep_normal_map(norm_png, stem)
    stats["normal_map_kept"] = norm_png is not None
    print(f"[ao] mean {stats['mean_ao']:.4f}, darkest {stats['min_ao']:.4f}, {stats['fully_open']} of {stats['owned']} owned texels fully open; "
          f"{stats['rays']} rays of length {stats['radius']:.4g} (bias {stats['bias']:.3g}); {stats['bvh_rounds']} fit rounds, {stats['seconds']:.3f} s -> {out}")
    with open(stem + "_ao.json", "w") as fh:
        json.dump(strict_json(stats), fh, indent=1, allow_nan=False)
        fh.write("\n")
    print(f"[ao] -> {stem}.mtl, {stem}.png, {stem}_ao.png, {stem}_ao.json" + (f", {stem}_normal.png" if norm_png else ""))
    if a.render_orbit:
        orbit = mesh_query.render_ao_orbit(verts, faces, ao_map, a.render_orbit, a.radius, a.elevation, a.fov, a.reso, a.white_background)
        save_frames(orbit, stem + "_ao_orbit")
        print(f"[ao] {a.render_orbit} turntable frames at {a.reso} x {a.reso} -> {stem}_ao_orbit")


if __name__ == "__main__":
    main()
