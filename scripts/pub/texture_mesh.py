#!/usr/bin/env python
"""Texture the (decimated) mesh against the orbit it was built from (v3d_amd/recon/mesh_texture.py): what the reference's fit_mesh_uv and
export_mesh do after decimation, with a closed-form per-face atlas, written as OBJ + MTL + PNG.

    python scripts/pub/texture_mesh.py --mesh out/gs/mesh_decimated.ply --video outputs/V3D_512/000000.npy -o out/gs/mesh.obj -w [--render_orbit 36]

The texture (--texture_resolution 1024, a square) starts from the PLY's vertex colours; Adam on the texels' logits (--lr 1e-3, --iters 2000),
mean squared error against --num_opt evenly spaced frames of the video (0, the default: all of them), one frame per iteration drawn with
--seed.  Prints one line with the mean PSNR over ALL frames of the vertex-coloured mesh, of the baked texture and of the fitted one, and
writes the statistics next to the output as <output without .obj>.json (strict JSON).  --radius, --elevation and --fov must be those of the
reconstruction.  --render_orbit N also writes N turntable frames of the textured mesh to <output without .obj>_orbit/.  A mesh with more
faces than the texture has room for (cells below 4 texels) is refused: decimate first (scripts/pub/decimate_mesh.py) or raise the resolution."""
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
    ap.add_argument("--mesh", required=True, help="the PLY to texture (decimate_mesh.py's output on the documented path)")
    ap.add_argument("--video", required=True, help="the orbit the mesh was built from (what recon_from_vid.py --video takes)")
    ap.add_argument("-o", "--out", default=None, help="the OBJ (default: <mesh without .ply>_textured.obj); .mtl and .png go beside it")
    ap.add_argument("-w", "--white_background", action="store_true")
    ap.add_argument("--texture_resolution", type=int, default=1024, help=f"texels on a side, up to {MAX_TEXTURE}")
    ap.add_argument("--iters", type=int, default=2000)
    ap.add_argument("--num_opt", type=int, default=0, help="evenly spaced frames to optimise against (0: all)")
    ap.add_argument("--lr", type=float, default=1e-3)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--num_frames", type=int, default=None)
    ap.add_argument("--radius", type=float, default=2.0)
    ap.add_argument("--elevation", type=float, default=0.0)
    ap.add_argument("--fov", type=float, default=60.0)
    ap.add_argument("--render_orbit", type=int, default=0, help="write N turntable frames of the textured mesh")
    return ap


def check_args(ap: argparse.ArgumentParser, a):
    if a.iters < 0 or a.num_opt < 0 or a.render_orbit < 0:
        ap.error("--iters, --num_opt and --render_orbit must not be negative")
    if not 1 <= a.texture_resolution <= MAX_TEXTURE:
        ap.error(f"--texture_resolution {a.texture_resolution} outside 1 .. {MAX_TEXTURE}")
    if not a.lr >= 0:
        ap.error(f"--lr {a.lr} must not be negative")
    if a.out is not None and not a.out.lower().endswith(".obj"):
        ap.error(f"-o {a.out}: the output is an OBJ")


def main(argv=None):
    ap = build_parser()
    a = ap.parse_args(argv)
    check_args(ap, a)
    from recon_from_vid import load_video, save_frames
    from render_mesh import strict_json
    from v3d_amd.recon import geometry, mesh_texture
    from v3d_amd.recon.cameras import orbit_cameras
    verts, faces, colors8 = geometry.read_mesh_ply(a.mesh)
    frames = load_video(a.video, a.num_frames)
    if frames.shape[1] != frames.shape[2]:
        raise SystemExit(f"{a.video}: frames must be square, got {frames.shape[2]} x {frames.shape[1]}")
    out = a.out or os.path.splitext(a.mesh)[0] + "_textured.obj"
    stem = os.path.splitext(out)[0]
    R = a.texture_resolution
    if faces.shape[0]:
        try:
            cell, _ = mesh_texture.atlas_layout(faces.shape[0], R)
        except ValueError as e:
            raise SystemExit(f"{a.mesh}: {e}; decimate the mesh or raise --texture_resolution")
    else:
        cell = 0
    print(f"[texture] {a.mesh}: {verts.shape[0]} vertices, {faces.shape[0]} triangles; {frames.shape[0]} frames of {frames.shape[2]} x {frames.shape[1]}; "
          f"texture {R} x {R}, {cell} texels to a face's cell")
    cams, _ = orbit_cameras(int(frames.shape[0]), a.radius, a.elevation, a.fov, int(frames.shape[1]))
    texture, stats = mesh_texture.fit_texture(verts, faces, colors8.astype(np.float32) / 255.0, cams, frames, tex_size=R, iterations=a.iters, lr=a.lr,
                                              num_opt=a.num_opt, white_background=a.white_background, seed=a.seed)
    mesh_texture.save_textured_obj(out, verts, faces, mesh_texture.face_uvs(faces.shape[0], R), texture)
    print(f"[texture] {len(stats['opt_views'])} views, {a.iters} iterations in {stats['seconds']:.2f} s: PSNR mean over all frames: vertex colours "
          f"{stats['psnr_vertex']:.2f}, baked texture {stats['psnr_baked']:.2f}, fitted texture {stats['psnr_fitted']:.2f} dB; "
          f"{stats['texels_seen']} of {R * R} texels seen -> {out}")
    with open(stem + ".json", "w") as fh:
        json.dump(strict_json(stats), fh, indent=1, allow_nan=False)
        fh.write("\n")
    print(f"[texture] -> {stem}.json, {stem}.mtl, {stem}.png")
    if a.render_orbit:
        reso = int(frames.shape[1])
        orbit = mesh_texture.render_textured_orbit(verts, faces, texture, a.render_orbit, a.radius, a.elevation, a.fov, reso, a.white_background)
        save_frames(orbit, stem + "_orbit")
        print(f"[texture] {a.render_orbit} turntable frames at {reso} x {reso} -> {stem}_orbit")


if __name__ == "__main__":
    main()
