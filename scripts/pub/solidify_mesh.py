#!/usr/bin/env python
"""Close a mesh (v3d_amd/recon/mesh_solid.py): every mesh of this pipeline is open where the orbit never looked - the underside of the
object.  This fills a volume with the signed distance to the mesh, the sign from the generalized winding number (inside where it is at
least 0.5), and extracts the closed surface again with the surface nets of recon_from_vid.py --save_mesh.  The hole is capped where the
winding number crosses 0.5, to a voxel: for a flat hole about the flat disc on its rim.

    python scripts/pub/solidify_mesh.py --mesh out/gs/mesh_clean.ply -o out/gs/mesh_solid.ply --resolution 256 --render_orbit 36 -w

The faces must be wound outward, as every mesh of this pipeline is; a mesh wound the other way solidifies to NOTHING, and --flip reverses
every face first.  --beta B: a tree node further away than B x its radius counts as one dipole (2: a winding number within about 0.03 of
the exact one; 0: the exact sum, slow).  --smooth K runs K Taubin iterations on the result (0: none).  --bound and --trunc set the volume's
half-extent and the truncation distance (default: 1.1 x the largest |coordinate| plus the truncation; 4 voxels).  The output has the layout
of the input, so every later script takes it.  Prints one line of statistics and writes them to --json F (default: <output without
.ply>.json, strict JSON).  --render_orbit N also writes N turntable frames of the result through the mesh rasterizer to <output without
.ply>_orbit/ (000.png .. and orbit.npy), at --reso, from the orbit of --radius, --elevation and --fov."""
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

MAX_RESOLUTION = 512               # geometry.MAX_RESOLUTION, V3D_RECON_MAX_N


def build_parser() -> argparse.ArgumentParser:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--mesh", required=True, help="a PLY of recon_from_vid.py --save_mesh or of a later script")
    ap.add_argument("-o", "--out", required=True, help="the closed PLY")
    ap.add_argument("-w", "--white_background", action="store_true")
    ap.add_argument("--resolution", type=int, default=256, help="voxels on a side")
    ap.add_argument("--beta", type=float, default=2.0, help="a node is a dipole from beta x its radius on (0: the exact sum)")
    ap.add_argument("--bound", type=float, default=None, help="half-extent of the volume")
    ap.add_argument("--trunc", type=float, default=None, help="truncation distance")
    ap.add_argument("--smooth", type=int, default=0, help="Taubin iterations on the result (0: none)")
    ap.add_argument("--flip", action="store_true", help="reverse every face first (a mesh wound inward)")
    ap.add_argument("--json", default=None, help="where the statistics go")
    ap.add_argument("--render_orbit", type=int, default=0, help="write N turntable frames of the result")
    ap.add_argument("--reso", type=int, default=512)
    ap.add_argument("--radius", type=float, default=2.0)
    ap.add_argument("--elevation", type=float, default=0.0)
    ap.add_argument("--fov", type=float, default=60.0)
    return ap


def main(argv=None, device="cuda"):
    ap = build_parser()
    a = ap.parse_args(argv)
    if not 2 <= a.resolution <= MAX_RESOLUTION:
        ap.error(f"--resolution must lie in 2 .. {MAX_RESOLUTION}")
    if not (math.isfinite(a.beta) and a.beta >= 0):
        ap.error("--beta must be finite and not negative")
    for name in ("bound", "trunc"):
        x = getattr(a, name)
        if x is not None and not (math.isfinite(x) and x > 0):
            ap.error(f"--{name} must be finite and positive")
    if a.smooth < 0 or a.render_orbit < 0:
        ap.error("--smooth and --render_orbit must not be negative")
    if not 0 < a.reso <= 4096:
        ap.error("--reso must lie in 1 .. 4096")
    from recon_from_vid import save_frames
    from render_mesh import strict_json
    from v3d_amd.recon import geometry, mesh_solid
    assert geometry.MAX_RESOLUTION == MAX_RESOLUTION
    verts, faces, colors8 = geometry.read_mesh_ply(a.mesh)
    stem = os.path.splitext(a.out)[0]
    print(f"[solid] {a.mesh}: {verts.shape[0]} vertices, {faces.shape[0]} triangles")
    v, f, c, stats = mesh_solid.solidify_mesh(verts, faces, colors8.astype(np.float32) / 255.0, resolution=a.resolution, bound=a.bound, trunc=a.trunc,
                                              beta=a.beta, smooth=a.smooth, flip=a.flip, device=device)
    geometry.save_mesh_ply(a.out, v, f, c)
    if stats["faces"] == 0:
        print("[solid] the result is EMPTY: nothing counts as inside.  Is the mesh wound inward?  Try --flip.")
    print(f"[solid] open edges {stats['boundary_edges_before']} -> {stats['boundary_edges_after']}; V - E + F = {stats['euler']}; volume "
          f"{stats['volume']:.6g}; {stats['resolution']}^3 voxels, bound {stats['bound']:.4g}, trunc {stats['trunc']:.4g}, beta {stats['beta']:g}; "
          f"{stats['bvh_rounds']} fit and {stats['moment_rounds']} moment rounds; {stats['vertices']} vertices, {stats['faces']} triangles in "
          f"{stats['seconds']:.2f} s -> {a.out}")
    path = a.json or stem + ".json"
    with open(path, "w") as fh:
        json.dump(strict_json(stats), fh, indent=1, allow_nan=False)
        fh.write("\n")
    print(f"[solid] -> {path}")
    if a.render_orbit and stats["faces"]:
        frames = mesh_solid.render_solid_orbit(v, f, c, a.render_orbit, a.radius, a.elevation, a.fov, a.reso, a.white_background, device=device)
        save_frames(frames, stem + "_orbit")
        print(f"[solid] {a.render_orbit} frames at {a.reso} x {a.reso} -> {stem}_orbit")


if __name__ == "__main__":
    main()
