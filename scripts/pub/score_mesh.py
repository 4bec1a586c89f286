#!/usr/bin/env python
"""Align a mesh to a reference and score it (v3d_amd/recon/mesh_align.py): a point-to-surface ICP on the reference's BVH, then Chamfer
distance, F-scores, normal consistency and volume IoU of the moved mesh against the reference, all on the GPU.

    python scripts/pub/score_mesh.py --mesh out/gs/mesh_50k.ply --reference gt.ply [--align similarity] [--starts 24] [--json out/gs/score.json] [-o out/gs/aligned.ply]

--mesh is an OBJ of texture_mesh.py or a PLY; --reference is a PLY.  --align none scores the pair as it stands, rigid keeps the scale at 1,
similarity (the default) solves for it too.  --starts 24 tries the 24 rotations of the cube first (for a mesh that may stand on its head).
--trim 0.9 lets the furthest 10 % of the mesh's area go without a correspondence (floaters).  --threshold: the F-score distances, relative
to the diagonal of the reference's bounding box.  --iou_resolution 0 skips the volume IoU (which needs both meshes wound outward).  Prints
one line; --json writes the whole dict with the 4 x 4 matrix; -o writes the moved mesh with its colours as a PLY."""
from __future__ import annotations

import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
for _p in (ROOT, os.path.dirname(os.path.abspath(__file__))):
    if _p not in sys.path:
        sys.path.insert(0, _p)

MAX_SUBDIVIDE = 16
MAX_IOU_RESOLUTION = 1024


def build_parser() -> argparse.ArgumentParser:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--mesh", required=True, help="the mesh to score: an OBJ of texture_mesh.py, or a PLY")
    ap.add_argument("--reference", required=True, help="the mesh to score against, a PLY")
    ap.add_argument("--align", choices=("none", "rigid", "similarity"), default="similarity", help="what the registration may change")
    ap.add_argument("--starts", type=int, default=1, help="1: from the bounding boxes as they stand; 24: from every rotation of the cube")
    ap.add_argument("--iterations", type=int, default=200, help="ICP iterations at the most (it stops early on a relative RMS change below 1e-5)")
    ap.add_argument("--trim", type=float, default=1.0, help="the share of the mesh's area that takes part, in (0, 1]")
    ap.add_argument("--threshold", type=float, nargs="+", default=[0.01, 0.02, 0.05], help="F-score distances over the reference's diagonal")
    ap.add_argument("--iou_resolution", type=int, default=128, help=f"voxels on a side for the volume IoU, 0 .. {MAX_IOU_RESOLUTION}; 0 skips it")
    ap.add_argument("--subdivide", type=int, default=2, help=f"sub-triangles along a face's edge, 1 .. {MAX_SUBDIVIDE}")
    ap.add_argument("--json", default=None, help="write the figures and the matrix here")
    ap.add_argument("-o", "--out", default=None, help="write the moved mesh here, a PLY")
    return ap


def check_args(ap: argparse.ArgumentParser, a):
    if a.starts not in (1, 24):
        ap.error(f"--starts {a.starts}: 1 or 24")
    if a.iterations < 0:
        ap.error(f"--iterations {a.iterations} must not be negative")
    if not 0 < a.trim <= 1:
        ap.error(f"--trim {a.trim} outside (0, 1]")
    if any(not 0 < t < float("inf") for t in a.threshold):
        ap.error(f"--threshold {a.threshold}: finite and positive")
    if not 0 <= a.iou_resolution <= MAX_IOU_RESOLUTION:
        ap.error(f"--iou_resolution {a.iou_resolution} outside 0 .. {MAX_IOU_RESOLUTION}")
    if not 1 <= a.subdivide <= MAX_SUBDIVIDE:
        ap.error(f"--subdivide {a.subdivide} outside 1 .. {MAX_SUBDIVIDE}")
    if not a.mesh.lower().endswith((".obj", ".ply")):
        ap.error(f"--mesh {a.mesh}: an OBJ or a PLY")
    if not a.reference.lower().endswith(".ply"):
        ap.error(f"--reference {a.reference}: a PLY")
    if a.json is not None and not a.json.lower().endswith(".json"):
        ap.error(f"--json {a.json}: a .json file")
    if a.out is not None:
        if not a.out.lower().endswith(".ply"):
            ap.error(f"-o {a.out}: a PLY")
        if os.path.abspath(a.out) in (os.path.abspath(a.mesh), os.path.abspath(a.reference)):
            ap.error(f"-o {a.out} would overwrite an input")


def line(mesh: str, reference: str, st: dict, sc: dict) -> str:
    """the one line printed"""
    rel, nc, iou = sc["relative"], sc["normal_consistency"], sc["volume_iou"]
    fs = ", ".join(f"F@{100 * f['threshold']:g}% {f['fscore']:.4f}" for f in sc["fscore"])
    return (f"[score] {mesh} -> {reference}: align {st['mode']} (start {st['start']}, {st['iterations_run']} iterations, scale {st['scale']:.5f}, "
            f"rotation {st['rotation_angle']:.3f} deg, rms {st['rms']:.3e}); chamfer {sc['chamfer']:.3e} ({100 * rel['chamfer']:.4f} % of the diagonal "
            f"{sc['diagonal']:.4f}); {fs}; normal consistency {nc['mean']:.4f}; IoU {'skipped' if iou is None else format(iou['iou'], '.4f')}; "
            f"{st['seconds'] + sc['seconds']:.3f} s")


def main(argv=None):
    ap = build_parser()
    a = ap.parse_args(argv)
    check_args(ap, a)
    from render_mesh import strict_json
    from v3d_amd.recon import geometry, mesh_align, mesh_texture
    import numpy as np
    if a.mesh.lower().endswith(".obj"):
        verts, faces, _, _ = mesh_texture.read_textured_obj(a.mesh)
        colors = np.full((verts.shape[0], 3), 0.5, dtype=np.float32)
    else:
        verts, faces, c8 = geometry.read_mesh_ply(a.mesh)
        colors = np.asarray(c8, dtype=np.float32) / 255.0
    rverts, rfaces, _ = geometry.read_mesh_ply(a.reference)
    for path, f in ((a.mesh, faces), (a.reference, rfaces)):
        if f.shape[0] == 0:
            raise SystemExit(f"{path}: no faces to score")
    matrix, st = mesh_align.align_mesh(verts, faces, rverts, rfaces, mode=a.align, starts=a.starts, iterations=a.iterations, trim=a.trim,
                                       subdivide=a.subdivide)
    moved = mesh_align.transform_vertices(verts, matrix)
    sc = mesh_align.score_meshes(moved, faces, rverts, rfaces, thresholds=a.threshold, iou_resolution=a.iou_resolution, subdivide=a.subdivide)
    print(line(a.mesh, a.reference, st, sc))
    if a.out:
        geometry.save_mesh_ply(a.out, moved, faces, colors)
        print(f"[score] -> {a.out}")
    if a.json:
        d = dict(sc, mesh=a.mesh, reference=a.reference, mesh_faces=int(faces.shape[0]), reference_faces=int(rfaces.shape[0]),
                 matrix=[[float(x) for x in row] for row in matrix], alignment=st)
        with open(a.json, "w") as fh:
            json.dump(strict_json(d), fh, indent=1, allow_nan=False)
            fh.write("\n")
        print(f"[score] -> {a.json}")


if __name__ == "__main__":
    main()
