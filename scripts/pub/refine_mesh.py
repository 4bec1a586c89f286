#!/usr/bin/env python
"""Refine the vertex colours of the mesh that recon_from_vid.py --save_mesh wrote against the orbit it was built from
(v3d_amd/recon/mesh_refine.py): the last step of the reference's pipeline (mesh_recon/refine.py), with the geometry held fixed.

    python scripts/pub/refine_mesh.py --mesh out/gs/mesh.ply --video outputs/V3D_512/000000.npy -o out/gs/mesh_refined.ply -w [--render_orbit 36]

Adam on the colours' logits (--lr 1e-3, --iters 2000), mean squared error against --num_opt evenly spaced frames of the video (0: all of
them), one frame per iteration drawn with --seed.  Prints one line with the mean PSNR of the mesh over ALL frames before and after and
writes the statistics next to the output as <output without .ply>.json (strict JSON).  --radius, --elevation and --fov must be those of the
reconstruction.  --render_orbit N also writes N turntable frames of the refined mesh to <output without .ply>_orbit/.  The reference's
perceptual term has no counterpart here: --lpips takes 0 only."""
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


def build_parser() -> argparse.ArgumentParser:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--mesh", required=True, help="the PLY recon_from_vid.py --save_mesh wrote")
    ap.add_argument("--video", required=True, help="the orbit the mesh was built from (what recon_from_vid.py --video takes)")
    ap.add_argument("-o", "--out", default=None, help="the refined PLY (default: <mesh without .ply>_refined.ply)")
    ap.add_argument("-w", "--white_background", action="store_true")
    ap.add_argument("--iters", type=int, default=2000)
    ap.add_argument("--num_opt", type=int, default=4, help="evenly spaced frames to optimise against (0: all)")
    ap.add_argument("--lr", type=float, default=1e-3)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--lpips", type=float, default=0.0, help="0 only")
    ap.add_argument("--num_frames", type=int, default=None)
    ap.add_argument("--radius", type=float, default=2.0)
    ap.add_argument("--elevation", type=float, default=0.0)
    ap.add_argument("--fov", type=float, default=60.0)
    ap.add_argument("--render_orbit", type=int, default=0, help="write N turntable frames of the refined mesh")
    return ap


def check_lpips(lpips: float):
    """what v3d_amd.recon.train.check_options says of --lambda_lpips"""
    if lpips > 0:
        raise NotImplementedError(f"--lpips {lpips}: LPIPS needs VGG weights that this build does not ship; pass --lpips 0")
    if lpips < 0:
        raise ValueError(f"--lpips {lpips} must not be negative")


def main(argv=None):
    ap = build_parser()
    a = ap.parse_args(argv)
    check_lpips(a.lpips)
    if a.iters < 0 or a.num_opt < 0:
        ap.error("--iters and --num_opt must not be negative")
    from recon_from_vid import load_video, save_frames
    from render_mesh import strict_json
    from v3d_amd.recon import geometry, mesh_refine, mesh_render
    from v3d_amd.recon.cameras import orbit_cameras
    verts, faces, colors8 = geometry.read_mesh_ply(a.mesh)
    frames = load_video(a.video, a.num_frames)
    if frames.shape[1] != frames.shape[2]:
        raise SystemExit(f"{a.video}: frames must be square, got {frames.shape[2]} x {frames.shape[1]}")
    out = a.out or os.path.splitext(a.mesh)[0] + "_refined.ply"
    stem = os.path.splitext(out)[0]
    print(f"[refine] {a.mesh}: {verts.shape[0]} vertices, {faces.shape[0]} triangles; {frames.shape[0]} frames of {frames.shape[2]} x {frames.shape[1]}")
    cams, _ = orbit_cameras(int(frames.shape[0]), a.radius, a.elevation, a.fov, int(frames.shape[1]))
    colors, stats = mesh_refine.refine_vertex_colors(verts, faces, colors8.astype(np.float32) / 255.0, cams, frames, iterations=a.iters, lr=a.lr,
                                                     num_opt=a.num_opt, white_background=a.white_background, seed=a.seed)
    geometry.save_mesh_ply(out, verts, faces, colors)
    print(f"[refine] views {stats['opt_views']}, {a.iters} iterations in {stats['seconds']:.2f} s: PSNR mean over all frames "
          f"{stats['psnr_before']:.2f} -> {stats['psnr_after']:.2f} dB; {stats['vertices_seen']} of {verts.shape[0]} vertices seen -> {out}")
    with open(stem + ".json", "w") as fh:
        json.dump(strict_json(stats), fh, indent=1, allow_nan=False)
        fh.write("\n")
    print(f"[refine] -> {stem}.json")
    if a.render_orbit:
        reso = int(frames.shape[1])
        orbit = mesh_render.render_mesh_orbit(verts, faces, colors, a.render_orbit, a.radius, a.elevation, a.fov, reso, a.white_background)
        save_frames(orbit, stem + "_orbit")
        print(f"[refine] {a.render_orbit} turntable frames at {reso} x {reso} -> {stem}_orbit")


if __name__ == "__main__":
    main()
