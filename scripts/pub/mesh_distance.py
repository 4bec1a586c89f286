#!/usr/bin/env python
"""How far one mesh is from another (v3d_amd/recon/mesh_query.py): BVHs of both meshes built on the GPU, the midpoint samples and the
vertices of each queried for their closest point on the other.

    python scripts/pub/mesh_distance.py --mesh out/gs/mesh_50k.ply --reference out/gs/mesh_clean.ply [--subdivide 2] [--json out/gs/mesh_50k_distance.json]

--mesh is an OBJ of texture_mesh.py or a PLY; --reference is a PLY (the mesh before decimation).  --subdivide n splits every face into n^2
sub-triangles (1 .. 16) whose centroids are the samples.  Prints one line with both directions (mean, RMS, largest) and the Hausdorff
distance, absolute and relative to the diagonal of the reference's bounding box; --json writes the whole dict."""
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


def build_parser() -> argparse.ArgumentParser:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--mesh", required=True, help="the mesh to measure: an OBJ of texture_mesh.py, or a PLY")
    ap.add_argument("--reference", required=True, help="the mesh to measure against, a PLY")
    ap.add_argument("--subdivide", type=int, default=2, help=f"sub-triangles along a face's edge, 1 .. {MAX_SUBDIVIDE}")
    ap.add_argument("--json", default=None, help="write the figures here")
    return ap


def check_args(ap: argparse.ArgumentParser, a):
    if not 1 <= a.subdivide <= MAX_SUBDIVIDE:
        ap.error(f"--subdivide {a.subdivide} outside 1 .. {MAX_SUBDIVIDE}")
    if not a.mesh.lower().endswith((".obj", ".ply")):
        ap.error(f"--mesh {a.mesh}: an OBJ or a PLY")
    if not a.reference.lower().endswith(".ply"):
        ap.error(f"--reference {a.reference}: a PLY")
    if a.json is not None and not a.json.lower().endswith(".json"):
        ap.error(f"--json {a.json}: a .json file")


def main(argv=None):
    ap = build_parser()
    a = ap.parse_args(argv)
    check_args(ap, a)
    from render_mesh import strict_json
    from v3d_amd.recon import geometry, mesh_query, mesh_texture
    if a.mesh.lower().endswith(".obj"):
        verts, faces, _, _ = mesh_texture.read_textured_obj(a.mesh)
    else:
        verts, faces, _ = geometry.read_mesh_ply(a.mesh)
    rverts, rfaces, _ = geometry.read_mesh_ply(a.reference)
    for path, f in ((a.mesh, faces), (a.reference, rfaces)):
        if f.shape[0] == 0:
            raise SystemExit(f"{path}: no faces to measure")
    d = mesh_query.mesh_distance(verts, faces, rverts, rfaces, subdivide=a.subdivide)
    d.update(mesh=a.mesh, reference=a.reference, mesh_faces=int(faces.shape[0]), reference_faces=int(rfaces.shape[0]))
    ab, ba, rel = d["a_to_b"], d["b_to_a"], d["relative"]
    print(f"[distance] {a.mesh} ({faces.shape[0]} triangles) -> {a.reference} ({rfaces.shape[0]}): mean {ab['mean']:.3e}, rms {ab['rms']:.3e}, "
          f"largest {ab['max']:.3e}; back: mean {ba['mean']:.3e}, rms {ba['rms']:.3e}, largest {ba['max']:.3e}; Hausdorff {d['hausdorff']:.3e} "
          f"({100 * rel['hausdorff']:.4f} % of the diagonal {d['diagonal']:.4f}), chamfer {d['chamfer']:.3e} ({100 * rel['chamfer']:.4f} %); "
          f"{d['samples']} points, {d['seconds']:.3f} s")
    if a.json:
        with open(a.json, "w") as fh:
            json.dump(strict_json(d), fh, indent=1, allow_nan=False)
            fh.write("\n")
        print(f"[distance] -> {a.json}")


if __name__ == "__main__":
    main()
