"""Timing of the isotropic remeshing (v3d_amd/recon/mesh_remesh.py) on the bench mesh of tools/mesh_decimate_bench.py: the bumpy sphere at
N^3 through extract_mesh, decimated to --target_faces, then 3 iterations at the default edge length.  Prints one JSON line (and writes it
to --out): the whole of remesh_mesh in ms (second of two passes), operations, rounds and ms per pass and iteration, one round's steps on the
decimated mesh (lists, the three propose entries, select, the three apply entries, relax, closest point + project), the five measures of
evenness before and after, and the spread of texels per unit area under the per-face atlas of mesh_texture.py (every face gets the same
number of texels, so the density is 1 / area: its coefficient of variation and its largest / smallest).  Nothing is promised from it.

    python tools/mesh_remesh_bench.py [--resolution 256] [--target_faces 50000] [--iterations 3] [--out FILE]
"""
from __future__ import annotations

import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.dirname(os.path.abspath(__file__))):
    if _p not in sys.path:
        sys.path.insert(0, _p)


def texel_density(verts, faces) -> dict:
    p, f = verts.detach().cpu().double().numpy(), faces.detach().cpu().long().numpy()
    area = 0.5 * np.linalg.norm(np.cross(p[f[:, 1]] - p[f[:, 0]], p[f[:, 2]] - p[f[:, 0]]), axis=1)
    d = 1.0 / area[area > 0]
    return {"cov": float(d.std() / d.mean()), "largest_over_smallest": float(d.max() / d.min()), "faces_without_area": int((area <= 0).sum())}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--resolution", type=int, default=256)
    ap.add_argument("--target_faces", type=int, default=50000)
    ap.add_argument("--iterations", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from mesh_refine_bench import bumpy_sphere_volume, timed
    from v3d_amd.recon import geometry as G
    from v3d_amd.recon import mesh_decimate as MD
    from v3d_amd.recon import mesh_remesh as MR
    from v3d_amd.recon.mesh_bake import build_bvh
    v0, f0, c0 = G.extract_mesh(bumpy_sphere_volume(a.resolution))
    v, f, c, _ = MD.decimate_mesh(v0, f0, c0, a.target_faces)
    V, F = v.shape[0], f.shape[0]
    t, res = {}, []
    for _ in range(2):                  # (second of two passes: the first loads the libraries and sizes the allocator)
        res.clear()
        t["remesh_mesh_ms"] = timed(lambda: res.extend(MR.remesh_mesh(v, f, c, iterations=a.iterations)))
        L = res[3]["target_edge"]
        st = MR.RemeshState(v, f, c, max(MR.MIN_SPARE, F // 2))
        t["lists_ms"] = timed(lambda: (st.touched(), st.lists()))
        flags = MR.boundary(st)
        out = {}
        t["split_propose_ms"] = timed(lambda: out.update(split=MR.split_propose(st, L)))
        t["collapse_propose_ms"] = timed(lambda: out.update(collapse=MR.collapse_propose(st, L)))
        t["flip_propose_ms"] = timed(lambda: out.update(flip=MR.flip_propose(st, flags=flags)))
        t["select_ms"] = timed(lambda: out.update(accept=MR.select(st, out["split"][0])[0]))
        bvh = build_bvh(v, f)
        t["relax_ms"] = timed(lambda: MR.relax_vertices(st, 0.5, flags=flags))
        t["closest_point_and_project_ms"] = timed(lambda: MR.project_vertices(st, bvh, c))
        for op, apply in (("split", MR.split_apply), ("collapse", MR.collapse_apply), ("flip", MR.flip_apply)):
            one = MR.RemeshState(v, f, c, max(MR.MIN_SPARE, F // 2))
            one.lists()
            accept = MR.select(one, out[op][0])[0]
            t[f"{op}_apply_ms"] = timed(lambda: apply(one, accept, out[op][1]))
    ov, of, oc, stats = res
    line = {"resolution": a.resolution, "vertices": V, "triangles": F, "iterations": a.iterations, "target_edge": stats["target_edge"],
            "vertices_after": int(ov.shape[0]), "triangles_after": int(of.shape[0]), "operations": stats["operations"], "rounds": stats["rounds"],
            "pass_ms": {k: [round(x, 3) for x in ms] for k, ms in stats["milliseconds"].items()}, "reallocations": stats["reallocations"],
            **{k: round(x, 4) for k, x in t.items()}, "before": stats["before"], "after": stats["after"], "distance": stats["distance"],
            "texel_density_before": texel_density(v, f), "texel_density_after": texel_density(ov, of), "device": torch.cuda.get_device_name(0)}
    text = json.dumps(line)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
