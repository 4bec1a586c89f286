#!/usr/bin/env python
"""Fit the vertices of a mesh to the silhouettes of the splats it was built from (v3d_amd/recon/mesh_deform.py): the counterpart of the
reference's recon/convert_nerf_mesh.py::fit_mesh, the one stage that moves the geometry.

    python scripts/pub/fit_mesh.py --mesh out/gs/mesh_50k.ply --gaussians out/gs/point_cloud/iteration_4000/point_cloud.ply \
        -o out/gs/mesh_50k_fit.ply -w [--video outputs/V3D_512/000000.npy] [--render_orbit 36]

The targets are the accumulated alpha of the splats from --views orbit cameras at --reso; the mesh's antialiased coverage is fitted to them
by Adam on per-vertex offsets (--lr 1e-4, --iters 2048, one view per iteration drawn with --seed), with an offset penalty (--lambda_offset)
and a smoothness term on the deformation field (--lambda_smooth).  Colours are carried over unchanged: refine_mesh.py / texture_mesh.py take
the output.  Prints the alpha MSE and the silhouette IoU over all views before and after and writes the statistics next to the output as
<output without .ply>.json (strict JSON).  --video (what recon_from_vid.py --video takes) only adds the PSNR of the mesh render against the
orbit before and after.  --radius, --elevation and --fov must be those of the reconstruction.  --render_orbit N also writes N turntable
frames of the fitted mesh to <output without .ply>_orbit/."""
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
    ap.add_argument("--mesh", required=True, help="the PLY of recon_from_vid.py --save_mesh, clean_mesh.py or decimate_mesh.py")
    ap.add_argument("--gaussians", required=True, help="the splats' PLY: <model>/point_cloud/iteration_N/point_cloud.ply")
    ap.add_argument("-o", "--out", default=None, help="the fitted PLY (default: <mesh without .ply>_fit.ply)")
    ap.add_argument("-w", "--white_background", action="store_true")
    ap.add_argument("--iters", type=int, default=2048)
    ap.add_argument("--lr", type=float, default=1e-4)
    ap.add_argument("--lambda_offset", type=float, default=0.1)
    ap.add_argument("--lambda_smooth", type=float, default=10.0)
    ap.add_argument("--views", type=int, default=36, help="orbit cameras to take silhouettes from")
    ap.add_argument("--num_opt", type=int, default=0, help="evenly spaced views to optimise against (0: all)")
    ap.add_argument("--reso", type=int, default=512, help="size of the silhouettes")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--video", default=None, help="the orbit the mesh was built from: adds the mesh render's PSNR before and after")
    ap.add_argument("--num_frames", type=int, default=None)
    ap.add_argument("--radius", type=float, default=2.0)
    ap.add_argument("--elevation", type=float, default=0.0)
    ap.add_argument("--fov", type=float, default=60.0)
    ap.add_argument("--render_orbit", type=int, default=0, help="write N turntable frames of the fitted mesh")
    return ap


def main(argv=None):
    ap = build_parser()
    a = ap.parse_args(argv)
    if a.iters < 0 or a.num_opt < 0:
        ap.error("--iters and --num_opt must not be negative")
    if a.views < 1 or not 0 < a.reso <= 4096:
        ap.error("--views must be positive and --reso lie in 1 .. 4096")
    if a.lr < 0 or a.lambda_offset < 0 or a.lambda_smooth < 0:
        ap.error("--lr, --lambda_offset and --lambda_smooth must not be negative")
    from recon_from_vid import load_video, save_frames
    from render_mesh import strict_json
    from v3d_amd.recon import geometry, mesh_deform, mesh_render
    from v3d_amd.recon.cameras import orbit_cameras
    from v3d_amd.recon.gaussians import GaussianModel
    verts, faces, colors8 = geometry.read_mesh_ply(a.mesh)
    colors = colors8.astype(np.float32) / 255.0
    gaussians = GaussianModel(0)
    gaussians.load_ply(a.gaussians, device="cuda")
    out = a.out or os.path.splitext(a.mesh)[0] + "_fit.ply"
    stem = os.path.splitext(out)[0]
    bg = [1.0, 1.0, 1.0] if a.white_background else [0.0, 0.0, 0.0]
    print(f"[fit] {a.mesh}: {verts.shape[0]} vertices, {faces.shape[0]} triangles; {gaussians.xyz.shape[0]} splats; {a.views} views of {a.reso} x {a.reso}")
    cams, _ = orbit_cameras(a.views, a.radius, a.elevation, a.fov, a.reso)
    targets = mesh_deform.silhouette_targets(gaussians, cams, bg)
    fitted, stats = mesh_deform.fit_vertices(verts, faces, cams, targets, iterations=a.iters, lr=a.lr, lambda_offset=a.lambda_offset,
                                             lambda_smooth=a.lambda_smooth, num_opt=a.num_opt, seed=a.seed)
    if a.video is not None:
        frames = load_video(a.video, a.num_frames)
        if frames.shape[1] != frames.shape[2]:
            raise SystemExit(f"{a.video}: frames must be square, got {frames.shape[2]} x {frames.shape[1]}")
        vcams, _ = orbit_cameras(int(frames.shape[0]), a.radius, a.elevation, a.fov, int(frames.shape[1]))
        stats["psnr_before"] = mesh_render.mesh_fidelity(verts, faces, colors, vcams, frames, bg)["psnr_mean"]
        stats["psnr_after"] = mesh_render.mesh_fidelity(fitted, faces, colors, vcams, frames, bg)["psnr_mean"]
    geometry.save_mesh_ply(out, fitted, faces, colors)
    print(f"[fit] {a.iters} iterations in {stats['seconds']:.2f} s: alpha MSE over all views {stats['mse_before']:.3e} -> {stats['mse_after']:.3e}, "
          f"silhouette IoU {stats['iou_before']:.4f} -> {stats['iou_after']:.4f}; largest offset {stats['max_offset']:.4f}; "
          f"{stats['vertices_moved']} of {verts.shape[0]} vertices moved -> {out}")
    if a.video is not None:
        print(f"[fit] against {a.video}: PSNR mean over all frames {stats['psnr_before']:.2f} -> {stats['psnr_after']:.2f} dB")
    with open(stem + ".json", "w") as fh:
        json.dump(strict_json(stats), fh, indent=1, allow_nan=False)
        fh.write("\n")
    print(f"[fit] -> {stem}.json")
    if a.render_orbit:
        orbit = mesh_render.render_mesh_orbit(fitted, faces, colors, a.render_orbit, a.radius, a.elevation, a.fov, a.reso, a.white_background)
        save_frames(orbit, stem + "_orbit")
        print(f"[fit] {a.render_orbit} turntable frames at {a.reso} x {a.reso} -> {stem}_orbit")


if __name__ == "__main__":
    main()
