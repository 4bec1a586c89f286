#!/usr/bin/env python
"""Bake a normal map of the full mesh onto the decimated one (v3d_amd/recon/mesh_bake.py): a BVH of the high mesh built on the GPU, two rays
per texel of the low mesh's per-face atlas along its interpolated normal, the high mesh's normal at the nearer hit.  Written as OBJ + MTL +
PNG with <out>_normal.png beside the albedo and a `norm` line in the MTL.  The map is in object space.

    python scripts/pub/bake_normals.py --mesh out/gs/mesh_50k.obj --high out/gs/mesh_clean.ply -o out/gs/mesh_50k_nm.obj [--render_orbit 36]

--mesh is the low mesh: an OBJ of texture_mesh.py keeps its texture and its resolution (--texture_resolution is then ignored); a PLY gets
its vertex colours baked as the albedo at --texture_resolution (1024).  --high is the mesh before decimation (clean_mesh.py's output).
--max_dist is how far a texel looks for the high surface, both ways (default: 0.05 x the diagonal of the high mesh's bounding box).  Prints
one line with the mean angle to the high mesh's normals over --views orbit views (--reso, --radius, --elevation, --fov) before (vertex
normals) and after (the map), and the hit counts; writes the statistics as <out without .obj>_normal.json.  --render_orbit N also writes N
turntable frames of the normal-mapped mesh to <out without .obj>_normal_orbit/."""
from __future__ import annotations

import argparse
import json
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
    ap.add_argument("--mesh", required=True, help="the low mesh: an OBJ of texture_mesh.py, or a PLY (decimate_mesh.py's output)")
    ap.add_argument("--high", required=True, help="the high mesh, a PLY (the mesh before decimation)")
    ap.add_argument("-o", "--out", default=None, help="the OBJ (default: <mesh without its suffix>_nm.obj); .mtl and the .png files go beside it")
    ap.add_argument("-w", "--white_background", action="store_true")
    ap.add_argument("--texture_resolution", type=int, default=1024, help=f"texels on a side for a PLY input, up to {MAX_TEXTURE}")
    ap.add_argument("--max_dist", type=float, default=None, help="how far a texel looks for the high surface (default: 0.05 x the high mesh's diagonal)")
    ap.add_argument("--views", type=int, default=18, help="orbit views the two angles are measured over (0: none)")
    ap.add_argument("--reso", type=int, default=512)
    ap.add_argument("--radius", type=float, default=2.0)
    ap.add_argument("--elevation", type=float, default=0.0)
    ap.add_argument("--fov", type=float, default=60.0)
    ap.add_argument("--render_orbit", type=int, default=0, help="write N turntable frames of the normal-mapped mesh")
    return ap


def check_args(ap: argparse.ArgumentParser, a):
    if a.views < 0 or a.render_orbit < 0:
        ap.error("--views and --render_orbit must not be negative")
    if not 1 <= a.texture_resolution <= MAX_TEXTURE:
        ap.error(f"--texture_resolution {a.texture_resolution} outside 1 .. {MAX_TEXTURE}")
    if not 1 <= a.reso <= 4096:
        ap.error(f"--reso {a.reso} outside 1 .. 4096")
    if a.max_dist is not None and not (a.max_dist >= 0 and a.max_dist != float("inf")):
        ap.error(f"--max_dist {a.max_dist} must be finite and not negative")
    if a.out is not None and not a.out.lower().endswith(".obj"):
        ap.error(f"-o {a.out}: the output is an OBJ")
    if not a.mesh.lower().endswith((".obj", ".ply")):
        ap.error(f"--mesh {a.mesh}: an OBJ or a PLY")


def main(argv=None):
    ap = build_parser()
    a = ap.parse_args(argv)
    check_args(ap, a)
    from recon_from_vid import save_frames
    from render_mesh import strict_json
    from v3d_amd.recon import geometry, mesh_bake, mesh_texture
    from v3d_amd.recon.cameras import orbit_cameras
    if a.mesh.lower().endswith(".obj"):
        verts, faces, vt, texture = mesh_texture.read_textured_obj(a.mesh)
        R = int(round(texture.shape[0] ** 0.5))
    else:
        verts, faces, colors8 = geometry.read_mesh_ply(a.mesh)
        R = a.texture_resolution
        vt = texture = None
    hverts, hfaces, _ = geometry.read_mesh_ply(a.high)
    out = a.out or os.path.splitext(a.mesh)[0] + "_nm.obj"
    stem = os.path.splitext(out)[0]
    if faces.shape[0]:
        try:
            mesh_texture.atlas_layout(faces.shape[0], R)
        except ValueError as e:
            raise SystemExit(f"{a.mesh}: {e}; decimate the mesh or raise --texture_resolution")
    if hfaces.shape[0] == 0:
        raise SystemExit(f"{a.high}: no faces to bake from")
    print(f"[bake] {a.mesh}: {verts.shape[0]} vertices, {faces.shape[0]} triangles; {a.high}: {hverts.shape[0]} vertices, {hfaces.shape[0]} triangles; "
          f"map {R} x {R}")
    if texture is None:
        _, texture = mesh_texture.bake_vertex_colors(faces, colors8.astype(np.float32) / 255.0, R)
        vt = mesh_texture.face_uvs(faces.shape[0], R)
    normal_map, stats = mesh_bake.bake_normal_map(verts, faces, hverts, hfaces, tex_size=R, max_dist=a.max_dist)
    mesh_texture.save_textured_obj(out, verts, faces, vt, texture, normal_map=normal_map)
    if a.views:
        cams, _ = orbit_cameras(a.views, a.radius, a.elevation, a.fov, a.reso)
        fid = mesh_bake.normal_map_fidelity(verts, faces, normal_map, hverts, hfaces, cams)
        stats.update(angle_before=fid["angle_before_mean"], angle_after=fid["angle_after_mean"], views=a.views)
    else:
        stats.update(angle_before=float("nan"), angle_after=float("nan"), views=0)
    print(f"[bake] mean angle to the high mesh's normals over {a.views} views: vertex normals {stats['angle_before']:.3f}, normal map "
          f"{stats['angle_after']:.3f} degrees; texels: {stats['hit_plus']} hit outwards, {stats['hit_minus']} inwards, {stats['missed']} missed of "
          f"{stats['owned']} owned; displacement mean {stats['displacement_mean']:.3e}, largest {stats['displacement_max']:.3e}; "
          f"{stats['bvh_rounds']} fit rounds, {stats['seconds']:.3f} s -> {out}")
    with open(stem + "_normal.json", "w") as fh:
        json.dump(strict_json(stats), fh, indent=1, allow_nan=False)
        fh.write("\n")
    print(f"[bake] -> {stem}.mtl, {stem}.png, {stem}_normal.png, {stem}_normal.json")
    if a.render_orbit:
        orbit = mesh_bake.render_normal_mapped_orbit(verts, faces, normal_map, a.render_orbit, a.radius, a.elevation, a.fov, a.reso, a.white_background)
        save_frames(orbit, stem + "_normal_orbit")
        print(f"[bake] {a.render_orbit} turntable frames at {a.reso} x {a.reso} -> {stem}_normal_orbit")


if __name__ == "__main__":
    main()
