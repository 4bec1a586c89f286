#!/usr/bin/env python
"""Repair what check_mesh.py reports (v3d_amd/recon/mesh_repair.py) and keep the triangles: weld the vertices that coincide, drop the faces
that are none, give the patches one winding, cut out the faces that pass through each other or hang on a non-manifold vertex, and fan the
open loops shut.

    python scripts/pub/repair_mesh.py --mesh out/gs/mesh_50k.ply -o out/gs/mesh_50k_repaired.ply [--grow 1] [--max_rounds 8]
        [--max_hole_edges N] [--no_orient] [--no_weld] [--json report.json] [--strict]

--mesh is an OBJ of texture_mesh.py (written back grey: an OBJ carries no vertex colours) or a PLY, whose colours are carried over.  Prints
one line before and one after.  A plain run exits 0 whatever is left; --strict exits 1 when the result is not watertight."""
from __future__ import annotations

import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
for _p in (ROOT, os.path.dirname(os.path.abspath(__file__))):
    if _p not in sys.path:
        sys.path.insert(0, _p)

MAX_EDGES = 2 ** 31 - 1
GREY = (0.6, 0.6, 0.6)


def build_parser() -> argparse.ArgumentParser:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--mesh", required=True, help="the mesh to repair: an OBJ of texture_mesh.py, or a PLY")
    ap.add_argument("-o", "--out", required=True, help="the repaired mesh, a PLY")
    ap.add_argument("--grow", type=int, default=1, help="grow the set of faces to cut this many times over shared vertices")
    ap.add_argument("--max_rounds", type=int, default=8, help="rounds of check, cut, fill at the most")
    ap.add_argument("--max_hole_edges", type=int, default=None, help="leave open loops longer than this alone (default: fill every loop)")
    ap.add_argument("--no_orient", action="store_true", help="leave the winding as it is")
    ap.add_argument("--no_weld", action="store_true", help="leave coinciding vertices apart")
    ap.add_argument("--json", default=None, help="write both reports and the history here")
    ap.add_argument("--strict", action="store_true", help="exit with status 1 when the result is not watertight")
    return ap


def check_args(ap: argparse.ArgumentParser, a):
    if not a.mesh.lower().endswith((".obj", ".ply")):
        ap.error(f"--mesh {a.mesh}: an OBJ or a PLY")
    if not a.out.lower().endswith(".ply"):
        ap.error(f"--out {a.out}: a .ply file")
    if os.path.abspath(a.out) == os.path.abspath(a.mesh):
        ap.error(f"--out {a.out}: would overwrite --mesh")
    if a.json is not None and not a.json.lower().endswith(".json"):
        ap.error(f"--json {a.json}: a .json file")
    if not 0 <= a.grow <= 64:
        ap.error(f"--grow {a.grow} outside 0 .. 64")
    if not 0 <= a.max_rounds <= 1024:
        ap.error(f"--max_rounds {a.max_rounds} outside 0 .. 1024")
    if a.max_hole_edges is not None and not 3 <= a.max_hole_edges <= MAX_EDGES:
        ap.error(f"--max_hole_edges {a.max_hole_edges} outside 3 .. {MAX_EDGES}")


def line(tag: str, path: str, r: dict) -> str:
    return (f"[repair] {tag} {path}: {'watertight' if r['watertight'] else 'NOT watertight'}; {r['faces']} triangles, {r['boundary_edges']} open and "
            f"{r['non_manifold_edges']} non-manifold edges, {r['self_intersections']} intersecting pairs, {r['components']} components")


def main(argv=None):
    ap = build_parser()
    a = ap.parse_args(argv)
    check_args(ap, a)
    import numpy as np
    from render_mesh import strict_json
    from v3d_amd.recon import geometry, mesh_repair, mesh_texture
    if a.mesh.lower().endswith(".obj"):
        verts, faces, _, _ = mesh_texture.read_textured_obj(a.mesh)
        colors = np.tile(np.asarray(GREY, dtype=np.float32), (verts.shape[0], 1))
    else:
        verts, faces, colors8 = geometry.read_mesh_ply(a.mesh)
        colors = colors8.astype(np.float32) / 255.0
    if faces.shape[0] == 0:
        raise SystemExit(f"{a.mesh}: no faces to repair")
    try:
        v, f, c, info = mesh_repair.repair_mesh(verts, faces, colors, grow=a.grow, max_rounds=a.max_rounds, max_hole_edges=a.max_hole_edges,
                                                orient=not a.no_orient, weld=not a.no_weld)
    except ValueError as e:
        raise SystemExit(f"{a.mesh}: {e}; nothing written")
    if f.shape[0] == 0:
        raise SystemExit(f"{a.mesh}: the repaired mesh would be empty; nothing written")
    print(line("before", a.mesh, info["before"]))
    geometry.save_mesh_ply(a.out, v.cpu(), f.cpu(), c.cpu())
    print(line("after ", a.out, info["after"]) + f"; {len(info['history'])} rounds ({info['stopped']})")
    if a.json:
        with open(a.json, "w") as fh:
            json.dump(strict_json({"mesh": a.mesh, "out": a.out, **info}), fh, indent=1, allow_nan=False)
            fh.write("\n")
        print(f"[repair] -> {a.json}")
    if a.strict and not info["after"]["watertight"]:
        raise SystemExit(1)


if __name__ == "__main__":
    main()
