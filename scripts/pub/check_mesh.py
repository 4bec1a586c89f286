#!/usr/bin/env python
"""Is this mesh sound (v3d_amd/recon/mesh_check.py): closed, manifold, consistently wound, and free of faces that pass through each other.
The BVH of the mesh is built on the GPU and walked with the mesh's own faces; the faces at every edge are counted on the corner lists.

    python scripts/pub/check_mesh.py --mesh out/gs/mesh_50k.ply [--json out/gs/mesh_50k_check.json] [--paint out/gs/mesh_50k_check.ply] [--strict]

--mesh is an OBJ of texture_mesh.py or a PLY.  Prints one line; --json writes the whole report.  --paint writes the mesh as a PLY, grey, with
the vertices of intersecting faces red, of non-manifold edges yellow and of open edges blue (in that order of precedence), for
render_mesh.py to show where the trouble is.  A plain run always exits 0; --strict exits 1 when the mesh is not watertight (closed, manifold,
oriented, no intersecting pair)."""
from __future__ import annotations

import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
for _p in (ROOT, os.path.dirname(os.path.abspath(__file__))):
    if _p not in sys.path:
        sys.path.insert(0, _p)

MAX_PAIRS = 2 ** 31 - 1
GREY, INTERSECTING, NON_MANIFOLD, BOUNDARY = (0.6, 0.6, 0.6),(1.0, 0.0, 0.0), (1.0, 1.0, 0.0), (0.0, 0.0, 1.0)


def build_parser() -> argparse.ArgumentParser:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--mesh", required=True, help="the mesh to check: an OBJ of texture_mesh.py, or a PLY")
    ap.add_argument("--json", default=None, help="write the report here")
    ap.add_argument("--paint", default=None, help="write the mesh here as a PLY with the trouble marked in colour")
    ap.add_argument("--max_pairs", type=int, default=1 << 24, help="list at most this many intersecting pairs (they are counted regardless)")
    ap.add_argument("--strict", action="store_true", help="exit with status 1 when the mesh is not watertight")
    return ap


def check_args(ap: argparse.ArgumentParser, a):
    if not a.mesh.lower().endswith((".obj", ".ply")):
        ap.error(f"--mesh {a.mesh}: an OBJ or a PLY")
    if a.json is not None and not a.json.lower().endswith(".json"):
        ap.error(f"--json {a.json}: a .json file")
    if a.paint is not None and not a.paint.lower().endswith(".ply"):
        ap.error(f"--paint {a.paint}: a .ply file")
    if a.paint is not None and os.path.abspath(a.paint) == os.path.abspath(a.mesh):
        ap.error(f"--paint {a.paint}: would overwrite --mesh")
    if not 1 <= a.max_pairs <= MAX_PAIRS:
        ap.error(f"--max_pairs {a.max_pairs} outside 1 .. {MAX_PAIRS}")


def paint_colors(num_verts: int, faces, per_face, flags):
    """[V, 3] float32: grey, then blue on open edges, yellow on non-manifold edges, red on the vertices of intersecting faces"""
    import numpy as np
    from v3d_amd.recon import mesh_check
    colors = np.tile(np.asarray(GREY, dtype=np.float32), (num_verts, 1))
    flags = np.asarray(flags)
    colors[(flags & mesh_check.OPEN) != 0] = BOUNDARY
    colors[(flags & mesh_check.NON_MANIFOLD) != 0] = NON_MANIFOLD
    hit = np.asarray(faces)[np.asarray(per_face) > 0].reshape(-1)
    colors[hit[(hit >= 0) & (hit < num_verts)]] = INTERSECTING
    return colors


def main(argv=None):
    ap = build_parser()
    a = ap.parse_args(argv)
    check_args(ap, a)
    import numpy as np
    from render_mesh import strict_json
    from v3d_amd.recon import geometry, mesh_check, mesh_texture
    if a.mesh.lower().endswith(".obj"):
        verts, faces, _, _ = mesh_texture.read_textured_obj(a.mesh)
    else:
        verts, faces, _ = geometry.read_mesh_ply(a.mesh)
    if faces.shape[0] == 0:
        raise SystemExit(f"{a.mesh}: no faces to check")
    r, d = mesh_check.check_mesh(verts, faces, max_pairs=a.max_pairs, details=True)
    r["mesh"] = a.mesh
    genus = "" if r["genus"] is None else f", genus {r['genus']}"
    volume = "" if r["volume"] is None else f", volume {r['volume']:.6g}"
    print(f"[check] {a.mesh} ({r['faces']} triangles, {r['vertices_used']} of {r['vertices']} vertices in use, {r['components']} components): "
          f"{'watertight' if r['watertight'] else 'NOT watertight'}; closed {r['closed']} ({r['boundary_edges']} open edges), manifold {r['manifold']} "
          f"({r['non_manifold_edges']} non-manifold edges, {r['pinched_vertices']} pinched vertices), oriented {r['oriented']} "
          f"({r['inconsistent_edges']} edges whose two faces run the same way); {r['self_intersections']} intersecting pairs on {r['intersecting_faces']} faces; "
          f"{r['absent_faces']} absent and {r['zero_area_faces']} zero-area faces; V - E + F = {r['euler']}{genus}; area {r['area']:.6g}{volume}; "
          f"{r['seconds']:.3f} s")
    if a.json:
        with open(a.json, "w") as fh:
            json.dump(strict_json(r), fh, indent=1, allow_nan=False)
            fh.write("\n")
        print(f"[check] -> {a.json}")
    if a.paint:
        f = np.asarray(faces).reshape(-1, 3)
        present = ((f >= 0) & (f < verts.shape[0])).all(1)
        geometry.save_mesh_ply(a.paint, verts, f[present], paint_colors(verts.shape[0], f, d["per_face"].cpu().numpy(), d["flags"].cpu().numpy()))
        print(f"[check] -> {a.paint}")
    if a.strict and not r["watertight"]:
        raise SystemExit(1)


if __name__ == "__main__":
    main()
