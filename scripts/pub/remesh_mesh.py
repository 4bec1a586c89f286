#!/usr/bin/env python
"""Remesh the mesh that recon_from_vid.py --save_mesh (or decimate_mesh.py) wrote into even triangles (v3d_amd/recon/mesh_remesh.py):
isotropic remeshing to one edge length, what the reference's mesh stage does with clean_mesh(..., remesh=True) around its decimation.

    python scripts/pub/remesh_mesh.py --mesh out/gs/mesh_50k.ply -o out/gs/mesh_even.ply [--target_edge L | --target_faces N]
                                      [--iterations 3] [--relax 0.5] [--no_reproject] [--json F]
                                      [--render_orbit 36 -w --video outputs/V3D_512/000000.npy]

Edges longer than 4/3 L are split, edges shorter than 4/5 L collapsed, edges flipped towards six triangles around every vertex; then the
vertices slide in their tangent planes and are put back on the input surface, whose colours they take.  --target_faces N picks the L at which
N equilateral triangles cover the mesh's area (the result has about N triangles); with neither option L keeps the input's triangle count.
Open edges and the vertices on them stay as they are.  The output has the layout of the input, so fit_mesh.py, texture_mesh.py,
render_mesh.py and decimate_mesh.py take it unchanged: run it after decimate_mesh.py and before fit_mesh.py / texture_mesh.py.  Prints one
line of statistics and writes them as strict JSON to --json (default: <output without .ply>.json).  --video compares the mesh before and
after with the orbit it was built from; --render_orbit N also writes N turntable frames of the result to <output without .ply>_orbit/.
--radius, --elevation and --fov must be those of the reconstruction."""
from __future__ import annotations

import argparse
import json
import math
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
for _p in (ROOT, os.path.dirname(os.path.abspath(__file__))):
    if _p not in sys.path:
        sys.path.insert(0, _p)


def build_parser() -> argparse.ArgumentParser:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--mesh", required=True, help="the PLY recon_from_vid.py --save_mesh or decimate_mesh.py wrote")
    ap.add_argument("-o", "--out", required=True, help="the remeshed PLY")
    ap.add_argument("--target_edge", type=float, default=None, help="the edge length to aim at")
    ap.add_argument("--target_faces", type=int, default=None, help="aim at the edge length of this many even triangles")
    ap.add_argument("--iterations", type=int, default=3)
    ap.add_argument("--relax", type=float, default=0.5, help="factor of the tangential smoothing step, 0 .. 1 (0: none)")
    ap.add_argument("--no_reproject", action="store_true", help="leave the vertices where the relaxation put them")
    ap.add_argument("--max_valence", type=int, default=24, help="triangles around a vertex at most")
    ap.add_argument("--json", default=None, help="where the statistics go (default: next to the output)")
    ap.add_argument("-w", "--white_background", action="store_true")
    ap.add_argument("--render_orbit", type=int, default=0, help="write N turntable frames of the remeshed mesh")
    ap.add_argument("--video", default=None, help="the orbit the mesh was built from: report the fidelity before and after")
    ap.add_argument("--num_frames", type=int, default=None)
    ap.add_argument("--reso", type=int, default=None, help="frame size of --render_orbit (default: the video's, or 512)")
    ap.add_argument("--radius", type=float, default=2.0)
    ap.add_argument("--elevation", type=float, default=0.0)
    ap.add_argument("--fov", type=float, default=60.0)
    return ap


def parse(argv=None):
    """The options, checked: every bad one ends in SystemExit here, before anything touches a GPU"""
    ap = build_parser()
    a = ap.parse_args(argv)
    if a.target_edge is not None and a.target_faces is not None:
        ap.error("give --target_edge or --target_faces, not both")
    if a.target_edge is not None and not (a.target_edge > 0 and math.isfinite(a.target_edge)):
        ap.error("--target_edge must be positive and finite")
    if a.target_faces is not None and a.target_faces <= 0:
        ap.error("--target_faces must be positive")
    if a.iterations < 0 or a.render_orbit < 0:
        ap.error("--iterations and --render_orbit must not be negative")
    if not 0 <= a.relax <= 1:
        ap.error("--relax must lie in 0 .. 1")
    if not 3 <= a.max_valence <= 1024:
        ap.error("--max_valence must lie in 3 .. 1024")
    if a.reso is not None and not 0 < a.reso <= 4096:
        ap.error("--reso must lie in 1 .. 4096")
    return a


def main(argv=None, device="cuda"):
    a = parse(argv)
    import numpy as np
    from decimate_mesh import fidelity_line
    from recon_from_vid import load_video, save_frames
    from render_mesh import strict_json
    from v3d_amd.recon import geometry, mesh_remesh, mesh_render
    from v3d_amd.recon.cameras import orbit_cameras
    verts, faces, colors8 = geometry.read_mesh_ply(a.mesh)
    colors = colors8.astype(np.float32) / 255.0
    stem = os.path.splitext(a.out)[0]
    print(f"[remesh] {a.mesh}: {verts.shape[0]} vertices, {faces.shape[0]} triangles")
    frames = load_video(a.video, a.num_frames) if a.video is not None else None
    cams, bg = None, [1.0, 1.0, 1.0] if a.white_background else [0.0, 0.0, 0.0]
    if frames is not None:
        if frames.shape[1] != frames.shape[2]:
            raise SystemExit(f"{a.video}: frames must be square, got {frames.shape[2]} x {frames.shape[1]}")
        cams, _ = orbit_cameras(int(frames.shape[0]), a.radius, a.elevation, a.fov, int(frames.shape[1]))
    v, f, c, stats = mesh_remesh.remesh_mesh(verts, faces, colors, target_edge=a.target_edge, target_faces=a.target_faces, iterations=a.iterations,
                                             relax=a.relax, reproject=not a.no_reproject, max_valence=a.max_valence, device=device)
    geometry.save_mesh_ply(a.out, v, f, c)
    ops = {k: sum(n) for k, n in stats["operations"].items()}
    line = f"[remesh] edge {stats['target_edge']:.4g}: {ops['split']} splits, {ops['collapse']} collapses, {ops['flip']} flips in " \
           f"{sum(sum(n) for n in stats['rounds'].values())} rounds"
    if stats["before"] is not None:
        b, s = stats["before"], stats["after"]
        line += f"; edges in range {100 * b['edges_in_range']:.1f} -> {100 * s['edges_in_range']:.1f} %, area CoV {b['area_cov']:.3f} -> " \
                f"{s['area_cov']:.3f}, smallest angle {b['mean_min_angle']:.1f} -> {s['mean_min_angle']:.1f} deg"
    if stats["distance"] is not None:
        line += f"; {100 * stats['distance']['hausdorff']:.2f} % of the diagonal from the input at most"
    print(f"{line}; {stats['vertices_after']} vertices, {stats['faces_after']} triangles -> {a.out}")
    if frames is not None:
        stats["fidelity_before"] = mesh_render.mesh_fidelity(verts, faces, colors, cams, frames, bg, device=device)
        stats["fidelity_after"] = mesh_render.mesh_fidelity(v, f, c, cams, frames, bg, device=device)
        print(f"[remesh] against {a.video}, before: {fidelity_line(stats['fidelity_before'])}")
        print(f"[remesh] against {a.video}, after:  {fidelity_line(stats['fidelity_after'])}")
    out_json = a.json or stem + ".json"
    with open(out_json, "w") as fh:
        json.dump(strict_json(stats), fh, indent=1, allow_nan=False)
        fh.write("\n")
    print(f"[remesh] -> {out_json}")
    if a.render_orbit:
        reso = a.reso or (int(frames.shape[1]) if frames is not None else 512)
        orbit = mesh_render.render_mesh_orbit(v, f, c, a.render_orbit, a.radius, a.elevation, a.fov, reso, a.white_background, device=device)
        save_frames(orbit, stem + "_orbit")
        print(f"[remesh] {a.render_orbit} turntable frames at {reso} x {reso} -> {stem}_orbit")


if __name__ == "__main__":
    main()
