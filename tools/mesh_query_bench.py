"""Timing of the mesh queries (v3d_amd/recon/mesh_query.py) on the scene of tools/mesh_bake_bench.py: the bumpy sphere at N^3 through
extract_mesh against its decimation to --target_faces.  Prints one JSON line per measurement (and writes them to --out): mesh_distance at
every --subdivide, with its figures, and bake_ambient_occlusion at --tex with every --samples, with its statistics and the occlusion
launch alone; each the second of two passes.  Nothing is promised from it and nothing is compared against a threshold.

    python tools/mesh_query_bench.py [--resolution 256] [--target_faces 50000] [--subdivide 1 2] [--tex 1024] [--samples 16 64] [--out FILE]
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
    ap.add_argument("--subdivide", type=int, nargs="+", default=[1, 2])
    ap.add_argument("--tex", type=int, default=1024)
    ap.add_argument("--samples", type=int, nargs="+", default=[16, 64])
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from mesh_refine_bench import bumpy_sphere_volume, timed
    from v3d_amd.recon import geometry as G
    from v3d_amd.recon import mesh_bake as MB
    from v3d_amd.recon import mesh_decimate as MD
    from v3d_amd.recon import mesh_query as MQ
    vf, ff, _ = G.extract_mesh(bumpy_sphere_volume(a.resolution))
    vd, fd, _, _ = MD.decimate_mesh(vf, ff, None, a.target_faces)
    base = {"resolution": a.resolution, "triangles_full": int(ff.shape[0]), "triangles": int(fd.shape[0]), "device": torch.cuda.get_device_name(0)}
    lines = []
    for n in a.subdivide:
        d = {}
        for _ in range(2):                      # (second of two passes: the first loads the libraries and sizes the allocator)
            d = MQ.mesh_distance(vd, fd, vf, ff, subdivide=n)
        lines.append({**base, "stage": "mesh_distance", "subdivide": n, "samples": d["samples"], "seconds": round(d["seconds"], 4),
                      "points_per_second": round(d["samples"] / d["seconds"]), "a_to_b": d["a_to_b"], "b_to_a": d["b_to_a"], "hausdorff": d["hausdorff"],
                      "chamfer": d["chamfer"], "diagonal": d["diagonal"], "hausdorff_relative": d["relative"]["hausdorff"]})
        print(json.dumps(lines[-1]), flush=True)
    bvh = MB.build_bvh(vf, ff)
    ln, hn = MB._vertex_normals(vd, fd), MB._vertex_normals(vf, ff)
    md = MB.default_max_dist(vf)
    owner, P, nrm = MQ.texel_frames(vd, fd, ln, a.tex)
    _, nmap, dist, _ = MB.bake_texels(vd, fd, ln, bvh, hn, a.tex, md)
    pts, normals = MQ.ao_points(P, nrm, dist, nmap)
    for K in a.samples:
        st, ms = {}, 0.0
        for _ in range(2):
            _, st = MQ.bake_ambient_occlusion(vd, fd, vf, ff, tex_size=a.tex, samples=K)
            ms = timed(lambda: MQ.occlusion(bvh, pts, normals, K, st["radius"], st["bias"]))
        lines.append({**base, "stage": "bake_ambient_occlusion", "tex_size": a.tex, "samples": K, "seconds": round(st["seconds"], 4),
                      "occlusion_ms": round(ms, 3), "rays": st["rays"], "rays_per_second": round(st["rays"] / (ms * 1e-3)), "owned": st["owned"],
                      "mean_ao": st["mean_ao"], "min_ao": st["min_ao"], "fully_open": st["fully_open"], "radius": st["radius"], "bias": st["bias"]})
        print(json.dumps(lines[-1]), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write("\n".join(json.dumps(x) for x in lines) + "\n")


if __name__ == "__main__":
    main()
