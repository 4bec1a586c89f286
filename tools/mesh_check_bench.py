"""Timing of the mesh check (v3d_amd/recon/mesh_check.py) on the scene of tools/mesh_query_bench.py: the bumpy sphere at N^3 through
extract_mesh, decimated to --target_faces, as it is and after every vertex has been moved by a random offset of --offset mean edge lengths
(what a vertex fit with only a smoothness term can do to a mesh).  Prints one JSON line per mesh (and writes them to --out): the time of
every pass (tree, count, scan, emit, sort, census), each the second of two passes, the whole of check_mesh, and what the check found.
Nothing is promised from it and nothing is compared against a threshold.

    python tools/mesh_check_bench.py [--resolution 256] [--target_faces 50000] [--offset 0.5] [--seed 0] [--out FILE]
"""
from __future__ import annotations

import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.dirname(os.path.abspath(__file__))):
    if _p not in sys.path:
        sys.path.insert(0, _p)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--resolution", type=int, default=256)
    ap.add_argument("--target_faces", type=int, default=50000)
    ap.add_argument("--offset", type=float, default=0.5)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from mesh_refine_bench import bumpy_sphere_volume, timed
    from v3d_amd.recon import geometry as G
    from v3d_amd.recon import mesh_bake as MB
    from v3d_amd.recon import mesh_check as MK
    from v3d_amd.recon import mesh_decimate as MD
    vf, ff, _ = G.extract_mesh(bumpy_sphere_volume(a.resolution))
    vd, fd, _, _ = MD.decimate_mesh(vf, ff, None, a.target_faces)
    fl = fd.long()
    edge = float(torch.cat([(vd[fl[:, k]] - vd[fl[:, (k + 1) % 3]]).norm(dim=1) for k in range(3)]).mean())
    g = torch.Generator(device="cpu").manual_seed(a.seed)
    moved = vd + (a.offset * edge * torch.randn(vd.shape, generator=g)).to(vd.device)
    base = {"resolution": a.resolution, "triangles_full": int(ff.shape[0]), "triangles": int(fd.shape[0]), "mean_edge": edge,
            "device": torch.cuda.get_device_name(0)}
    lines = []
    for name, v in (("decimated", vd), ("offset", moved)):
        ms, report = {}, {}
        for _ in range(2):                      # (second of two passes: the first loads the libraries and sizes the allocator)
            bvh = None

            def tree():
                nonlocal bvh
                bvh = MB.build_bvh(v, fd)

            ms["tree"] = timed(tree)
            t = {}
            MK.self_intersections(bvh, timings=t)
            ms.update({k: 1000.0 * x for k, x in t.items()})
            ms["census"] = timed(lambda: MK._census(fd, v.shape[0]))
            report = MK.check_mesh(v, fd)
        lines.append({**base, "mesh": name, "offset_edge_lengths": 0.0 if name == "decimated" else a.offset,
                      "ms": {k: round(x, 3) for k, x in ms.items()}, "check_mesh_seconds": round(report["seconds"], 4),
                      "faces_per_second_of_count": round(int(fd.shape[0]) / (ms["count"] * 1e-3)),
                      "report": {k: x for k, x in report.items() if k != "seconds"}})
        print(json.dumps(lines[-1]), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write("\n".join(json.dumps(x) for x in lines) + "\n")


if __name__ == "__main__":
    main()
