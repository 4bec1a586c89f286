"""Timing of the mesh cleaning (v3d_amd/recon/mesh_clean.py) on a mesh of the size the reconstruction produces: a bumpy sphere at N^3 through
extract_mesh with a few thousand planted floaters (single triangles) and loose vertices.  Prints one JSON line (and writes it to --out): ms
for the corner lists, the normals, the labelling (with its number of rounds), the boundary flags, one smoothing pass, and the whole of
clean_mesh (filter + 10 Taubin iterations), second of two passes each.  Nothing is promised from it.

    python tools/mesh_clean_bench.py [--resolution 256] [--floaters 2000] [--out FILE]
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
    ap.add_argument("--floaters", type=int, default=2000)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from mesh_refine_bench import bumpy_sphere_volume, timed
    from v3d_amd.recon import geometry as G
    from v3d_amd.recon import mesh_clean as MC
    verts, faces, colors = G.extract_mesh(bumpy_sphere_volume(a.resolution))
    V0 = verts.shape[0]
    g = torch.Generator().manual_seed(0)
    centre = 0.9 * (2 * torch.rand(a.floaters, 1, 3, generator=g) - 1)
    tri = (centre + 0.01 * torch.randn(a.floaters, 3, 3, generator=g)).reshape(-1, 3).cuda()
    loose = (2 * torch.rand(a.floaters, 3, generator=g) - 1).cuda()
    v = torch.cat([verts, tri, loose]).contiguous()
    f = torch.cat([faces, (V0 + torch.arange(3 * a.floaters, dtype=torch.int32, device="cuda")).reshape(-1, 3)]).contiguous()
    c = torch.cat([colors, torch.full((4 * a.floaters, 3), 0.5, device="cuda")]).contiguous()
    V = v.shape[0]
    t, rounds, stats = {}, 0, {}
    for _ in range(2):                  # (second of two passes: the first loads the libraries and sizes the allocator)
        lists = []
        t["lists_ms"] = timed(lambda: lists.extend(MC._corner_lists(f, V)))
        ranges, corners = lists
        t["normals_ms"] = timed(lambda: MC._normals(v, f, ranges, corners))
        out = []
        t["labels_ms"] = timed(lambda: out.extend(MC._labels(f, V, ranges, corners)))
        rounds = out[1]
        t["boundary_ms"] = timed(lambda: MC._boundary(f, V, ranges, corners))
        t["smooth_pass_ms"] = timed(lambda: MC._smooth(v, f, ranges, corners, None, 10, 0.5, -0.53)) / 20
        res = []
        t["clean_mesh_ms"] = timed(lambda: res.extend(MC.clean_mesh(v, f, c)))
        stats = res[3]
    line = {"resolution": a.resolution, "vertices": V, "triangles": int(f.shape[0]), "floaters": a.floaters, "rounds": rounds,
            "longest_list": int((ranges[:, 1] - ranges[:, 0]).max()), **{k: round(x, 4) for k, x in t.items()},
            "vertices_after": stats["vertices"], "triangles_after": stats["faces"], "components_before": len(stats["components_before"]),
            "components_after": len(stats["components_after"]), "device": torch.cuda.get_device_name(0)}
    text = json.dumps(line)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
