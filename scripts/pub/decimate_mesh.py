#!/usr/bin/env python
"""Decimate the mesh that recon_from_vid.py --save_mesh wrote (v3d_amd/recon/mesh_decimate.py): quadric-error edge collapse down to a target
number of triangles, what the reference's mesh stage does first (fit_mesh, decimate_target = 5e4) before it unwraps and textures.

    python scripts/pub/decimate_mesh.py --mesh out/gs/mesh.ply -o out/gs/mesh_50k.ply --target_faces 50000 [--max_error E]
                                        [--render_orbit 36 -w --video outputs/V3D_512/000000.npy]

A collapse moves one end of an edge onto the other, so the output's vertices are a subset of the input's with their positions and colours
unchanged; vertices on open edges stay.  --max_error E stops before the target when the cheapest remaining collapse costs more than E (the
area-weighted sum of squared plane distances); --max_valence caps the number of triangles around a vertex.  The output has the layout of the
input, so render_mesh.py, refine_mesh.py and clean_mesh.py take it unchanged.  Prints one line of statistics and writes them next to the
output as <output without .ply>.json (strict JSON).  --video (what recon_from_vid.py --video takes) compares the mesh before and after with
the orbit it was built from, over the video's own cameras: PSNR, share of covered pixels, and pixels with an odd number of faces over them
(0 for a closed mesh).  --render_orbit N also writes N turntable frames of the decimated mesh to <output without .ply>_orbit/, at the
video's size or --reso.  --radius, --elevation and --fov must be those of the reconstruction."""
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
    ap.add_argument("-o", "--out", required=True, help="the decimated PLY")
    ap.add_argument("--target_faces", type=int, default=50000, help="triangles to keep at most")
    ap.add_argument("--max_error", type=float, default=None, help="stop when the cheapest collapse costs more")
    ap.add_argument("--max_valence", type=int, default=24, help="triangles around a vertex at most")
    ap.add_argument("-w", "--white_background", action="store_true")
    ap.add_argument("--render_orbit", type=int, default=0, help="write N turntable frames of the decimated mesh")
    ap.add_argument("--video", default=None, help="the orbit the mesh was built from: report the fidelity before and after")
    ap.add_argument("--num_frames", type=int, default=None)
    ap.add_argument("--reso", type=int, default=None, help="frame size of --render_orbit (default: the video's, or 512)")
    ap.add_argument("--radius", type=float, default=2.0)
    ap.add_argument("--elevation", type=float, default=0.0)
    ap.add_argument("--fov", type=float, default=60.0)
    return ap


def fidelity_line(fid: dict) -> str:
    return (f"PSNR mean {fid['psnr_mean']:.2f} dB, worst view {min(fid['psnr']):.2f} dB; coverage {100 * float(np.mean(fid['coverage'])):.1f} %; "
            f"pixels with an odd number of faces over them: {sum(fid['odd_hit_pixels'])}")


def main(argv=None, device="cuda"):
    ap = build_parser()
    a = ap.parse_args(argv)
    if a.target_faces < 0 or a.render_orbit < 0:
        ap.error("--target_faces and --render_orbit must not be negative")
    if a.max_error is not None and not a.max_error >= 0:
        ap.error("--max_error must be a number that is not negative")
    if not 3 <= a.max_valence <= 1024:
        ap.error("--max_valence must lie in 3 .. 1024")
    if a.reso is not None and not 0 < a.reso <= 4096:
        ap.error("--reso must lie in 1 .. 4096")
    from recon_from_vid import load_video, save_frames
    from render_mesh import strict_json
    from v3d_amd.recon import geometry, mesh_decimate, mesh_render
    from v3d_amd.recon.cameras import orbit_cameras
    verts, faces, colors8 = geometry.read_mesh_ply(a.mesh)
    colors = colors8.astype(np.float32) / 255.0
    stem = os.path.splitext(a.out)[0]
    print(f"[decimate] {a.mesh}: {verts.shape[0]} vertices, {faces.shape[0]} triangles")
    frames = load_video(a.video, a.num_frames) if a.video is not None else None
    cams, bg = None, [1.0, 1.0, 1.0] if a.white_background else [0.0, 0.0, 0.0]
    if frames is not None:
        if frames.shape[1] != frames.shape[2]:
            raise SystemExit(f"{a.video}: frames must be square, got {frames.shape[2]} x {frames.shape[1]}")
        cams, _ = orbit_cameras(int(frames.shape[0]), a.radius, a.elevation, a.fov, int(frames.shape[1]))
    v, f, c, stats = mesh_decimate.decimate_mesh(verts, faces, colors, a.target_faces, max_error=a.max_error, max_valence=a.max_valence, device=device)
    geometry.save_mesh_ply(a.out, v, f, c)
    print(f"[decimate] {stats['rounds']} rounds, {sum(stats['accepted'])} collapses, largest cost {stats['max_cost']:.3e}; stopped by: "
          f"{stats['stopped']}{'' if stats['reached'] else ' (target not reached)'}; vertices on open edges {stats['boundary_vertices_before']} -> "
          f"{stats['boundary_vertices_after']}; {stats['vertices_after']} vertices, {stats['faces_after']} triangles -> {a.out}")
    if frames is not None:
        stats["fidelity_before"] = mesh_render.mesh_fidelity(verts, faces, colors, cams, frames, bg, device=device)
        stats["fidelity_after"] = mesh_render.mesh_fidelity(v, f, c, cams, frames, bg, device=device)
        print(f"[decimate] against {a.video}, before: {fidelity_line(stats['fidelity_before'])}")
        print(f"[decimate] against {a.video}, after:  {fidelity_line(stats['fidelity_after'])}")
    with open(stem + ".json", "w") as fh:
        json.dump(strict_json(stats), fh, indent=1, allow_nan=False)
        fh.write("\n")
    print(f"[decimate] -> {stem}.json")
    if a.render_orbit:
        reso = a.reso or (int(frames.shape[1]) if frames is not None else 512)
        orbit = mesh_render.render_mesh_orbit(v, f, c, a.render_orbit, a.radius, a.elevation, a.fov, reso, a.white_background, device=device)
        save_frames(orbit, stem + "_orbit")
        print(f"[decimate] {a.render_orbit} turntable frames at {reso} x {reso} -> {stem}_orbit")


if __name__ == "__main__":
    main()
