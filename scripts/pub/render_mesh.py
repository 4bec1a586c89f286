#!/usr/bin/env python
"""Render the mesh that recon_from_vid.py --save_mesh wrote, on the gfx950 triangle rasterizer (v3d_amd/recon/mesh_render.py), the way the
reference's recon/render*.py scripts look at every product of the reconstruction.

    python scripts/pub/render_mesh.py --mesh out/gs/mesh.ply -o out/gs/mesh_orbit --render_orbit 36 -w [--video outputs/V3D_512/000000.npy]

--render_orbit N writes N turntable frames (000.png .. and orbit.npy, the layout of recon_from_vid.py --render_orbit) to the output folder.
--video (what recon_from_vid.py --video takes) compares the mesh with the orbit it was built from, over the video's own cameras: one line
with the mean and the worst-view PSNR of the mesh render, the share of covered pixels and the number of pixels with an odd number of faces
over them (0 for a mesh that is closed as seen from every camera), also written to <out>/fidelity.json (strict JSON: a PSNR that is not
finite, as of a view the mesh reproduces exactly, is written as the string "inf", which float() reads back).  --radius, --elevation and --fov must be
those of the reconstruction.  Without --reso the frames have the size of the video's, or 512."""
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
    ap.add_argument("-o", "--out", default=None, help="output folder (default: <folder of --mesh>/mesh_orbit)")
    ap.add_argument("-w", "--white_background", action="store_true")
    ap.add_argument("--render_orbit", type=int, default=0, help="write N turntable frames of the mesh")
    ap.add_argument("--video", default=None, help="the orbit the mesh was built from: report how well the mesh reproduces it")
    ap.add_argument("--num_frames", type=int, default=None)
    ap.add_argument("--radius", type=float, default=2.0)
    ap.add_argument("--elevation", type=float, default=0.0)
    ap.add_argument("--fov", type=float, default=60.0)
    ap.add_argument("--reso", type=int, default=None, help="frame size of --render_orbit (default: the video's, or 512)")
    ap.add_argument("--no_cull", action="store_true", help="also draw the faces that look away from the camera")
    return ap


def strict_json(obj):
    """`obj` with every float that is not finite replaced by its str() ("inf", "-inf", "nan"): json.dump would write bare tokens no strict
    parser accepts"""
    if isinstance(obj, dict):
        return {k: strict_json(v) for k, v in obj.items()}
    if isinstance(obj, (list, tuple)):
        return [strict_json(v) for v in obj]
    if isinstance(obj, float) and not math.isfinite(obj):
        return str(obj)
    return obj


def main(argv=None):
    ap = build_parser()
    a = ap.parse_args(argv)
    if not a.render_orbit and a.video is None:
        ap.error("nothing to do: give --render_orbit N and / or --video")
    if a.reso is not None and not 0 < a.reso <= 4096:
        ap.error("--reso must lie in 1 .. 4096")
    from recon_from_vid import load_video, save_frames
    from v3d_amd.recon import geometry, mesh_render
    from v3d_amd.recon.cameras import orbit_cameras
    verts, faces, colors8 = geometry.read_mesh_ply(a.mesh)
    colors = colors8.astype(np.float32) / 255.0
    out = a.out or os.path.join(os.path.dirname(os.path.abspath(a.mesh)), "mesh_orbit")
    os.makedirs(out, exist_ok=True)
    frames = load_video(a.video, a.num_frames) if a.video is not None else None
    print(f"[mesh] {a.mesh}: {verts.shape[0]} vertices, {faces.shape[0]} triangles")
    if a.render_orbit:
        reso = a.reso or (int(frames.shape[1]) if frames is not None else 512)
        orbit = mesh_render.render_mesh_orbit(verts, faces, colors, a.render_orbit, a.radius, a.elevation, a.fov, reso, a.white_background,
                                              cull=not a.no_cull)
        save_frames(orbit, out)
        print(f"[mesh] {a.render_orbit} turntable frames at {reso} x {reso} -> {out}")
    if frames is not None:
        if frames.shape[1] != frames.shape[2]:
            raise SystemExit(f"{a.video}: frames must be square, got {frames.shape[2]} x {frames.shape[1]}")
        cams, _ = orbit_cameras(int(frames.shape[0]), a.radius, a.elevation, a.fov, int(frames.shape[1]))
        fid = mesh_render.mesh_fidelity(verts, faces, colors, cams, frames, [1.0, 1.0, 1.0] if a.white_background else [0.0, 0.0, 0.0])
        print(f"[mesh] against {a.video}: PSNR mean {fid['psnr_mean']:.2f} dB, worst view {min(fid['psnr']):.2f} dB; coverage "
              f"{100 * float(np.mean(fid['coverage'])):.1f} %; pixels with an odd number of faces over them: {sum(fid['odd_hit_pixels'])}")
        path = os.path.join(out, "fidelity.json")
        with open(path, "w") as fh:
            json.dump(strict_json(fid), fh, indent=1, allow_nan=False)
            fh.write("\n")
        print(f"[mesh] -> {path}")


if __name__ == "__main__":
    main()
