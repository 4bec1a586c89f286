#!/usr/bin/env python
"""Clean the mesh that recon_from_vid.py --save_mesh wrote (v3d_amd/recon/mesh_clean.py): drop the small connected components (floaters) and
the vertices that no face uses, smooth the voxel-scale noise away, and look at the geometry alone through its normals - what the reference's
mesh stage does in Mesh.load(clean=.., renormal=True) and render_normal.

    python scripts/pub/clean_mesh.py --mesh out/gs/mesh.ply -o out/gs/mesh_clean.ply --min_faces 64 --smooth 10 --render_normals 36 -w

--min_faces N drops every component of fewer than N faces, --keep_largest K all but the K components of the most faces (0: off); with both 0
the filter is left out.  --smooth N runs N Taubin iterations (--lam, then --mu; --fix_boundary keeps the vertices on open edges in place),
0 leaves the smoothing out.  The output has the layout of the input, so render_mesh.py and refine_mesh.py take it unchanged; the colours ride
along.  Prints one line of statistics and writes them next to the output as <output without .ply>.json (strict JSON).  --render_normals N
also writes N turntable frames of the cleaned mesh's camera-space normals ((n + 1) / 2 with x right, y up, z towards the camera) to
<output without .ply>_normals/ (000.png .. and orbit.npy), at --reso, from the orbit of --radius, --elevation and --fov."""
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


def build_parser() -> argparse.ArgumentParser:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--mesh", required=True, help="the PLY recon_from_vid.py --save_mesh wrote")
    ap.add_argument("-o", "--out", required=True, help="the cleaned PLY")
    ap.add_argument("-w", "--white_background", action="store_true")
    ap.add_argument("--min_faces", type=int, default=64, help="drop the components of fewer faces")
    ap.add_argument("--keep_largest", type=int, default=0, help="keep only the K components of the most faces (0: off)")
    ap.add_argument("--smooth", type=int, default=10, help="Taubin iterations (0: none)")
    ap.add_argument("--lam", type=float, default=0.5)
    ap.add_argument("--mu", type=float, default=-0.53)
    ap.add_argument("--fix_boundary", action="store_true", help="keep the vertices on open edges where they are")
    ap.add_argument("--render_normals", type=int, default=0, help="write N turntable frames of the normals")
    ap.add_argument("--reso", type=int, default=512)
    ap.add_argument("--radius", type=float, default=2.0)
    ap.add_argument("--elevation", type=float, default=0.0)
    ap.add_argument("--fov", type=float, default=60.0)
    return ap


def main(argv=None, device="cuda"):
    ap = build_parser()
    a = ap.parse_args(argv)
    if a.min_faces < 0 or a.keep_largest < 0 or a.smooth < 0 or a.render_normals < 0:
        ap.error("--min_faces, --keep_largest, --smooth and --render_normals must not be negative")
    if not (math.isfinite(a.lam) and math.isfinite(a.mu)):
        ap.error("--lam and --mu must be finite")
    if not 0 < a.reso <= 4096:
        ap.error("--reso must lie in 1 .. 4096")
    from recon_from_vid import save_frames
    from render_mesh import strict_json
    from v3d_amd.recon import geometry, mesh_clean
    verts, faces, colors8 = geometry.read_mesh_ply(a.mesh)
    stem = os.path.splitext(a.out)[0]
    print(f"[clean] {a.mesh}: {verts.shape[0]} vertices, {faces.shape[0]} triangles")
    v, f, c, stats = mesh_clean.clean_mesh(verts, faces, colors8.astype(np.float32) / 255.0, min_faces=a.min_faces, keep_largest=a.keep_largest,
                                           iterations=a.smooth, lam=a.lam, mu=a.mu, fix_boundary=a.fix_boundary, device=device)
    geometry.save_mesh_ply(a.out, v, f, c)
    print(f"[clean] components {len(stats['components_before'])} -> {len(stats['components_after'])} ({stats['rounds']} labelling rounds); removed "
          f"{stats['removed_faces']} triangles and {stats['removed_vertices']} vertices ({stats['unreferenced_vertices']} of them used by no face); "
          f"vertices on open edges {stats['boundary_vertices_before']} -> {stats['boundary_vertices_after']}; {stats['smooth_iterations']} smoothing "
          f"iterations; {stats['vertices']} vertices, {stats['faces']} triangles -> {a.out}")
    with open(stem + ".json", "w") as fh:
        json.dump(strict_json(stats), fh, indent=1, allow_nan=False)
        fh.write("\n")
    print(f"[clean] -> {stem}.json")
    if a.render_normals:
        frames = mesh_clean.render_normal_orbit(v, f, a.render_normals, a.radius, a.elevation, a.fov, a.reso, a.white_background, device=device)
        save_frames(frames, stem + "_normals")
        print(f"[clean] {a.render_normals} normal frames at {a.reso} x {a.reso} -> {stem}_normals")


if __name__ == "__main__":
    main()
