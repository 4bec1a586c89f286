"""Timing of the winding number and the mesh-to-volume stage (v3d_amd/recon/mesh_solid.py) on the mesh of tools/mesh_bake_bench.py: the
bumpy sphere at N^3 through extract_mesh.  Prints one JSON line per measurement (and writes them to --out): the moments, winding_numbers
on --points random points of the mesh's box at every --beta (0 is the exact sum: the comparison to report is the tree walk against it, on
the same box), and the sdf_grid launch at every --grid.  Each is the mean of --repeat calls between device events, second of two passes.
Nothing is promised from it and nothing is compared against a threshold.

    python tools/mesh_solid_bench.py [--resolution 256] [--points 1000000] [--beta 0 2 3] [--grid 128 256] [--exact_points 20000] [--out FILE]
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
    ap.add_argument("--points", type=int, default=1000000)
    ap.add_argument("--exact_points", type=int, default=20000, help="points of the exact sum (beta 0 visits every triangle: scaled to --points in the report)")
    ap.add_argument("--beta", type=float, nargs="+", default=[0.0, 2.0, 3.0])
    ap.add_argument("--grid", type=int, nargs="+", default=[128, 256])
    ap.add_argument("--repeat", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from mesh_refine_bench import bumpy_sphere_volume, timed
    from v3d_amd.recon import geometry as G
    from v3d_amd.recon import mesh_bake as MB
    from v3d_amd.recon import mesh_solid as MS
    v, f, c = G.extract_mesh(bumpy_sphere_volume(a.resolution))
    bvh = MB.build_bvh(v, f)
    base = {"resolution": a.resolution, "triangles": int(f.shape[0]), "device": torch.cuda.get_device_name(0)}
    lines = []

    def mean_ms(fn):
        ms = 0.0
        for _ in range(2):                          # (second of two passes)
            ms = sum(timed(fn) for _ in range(a.repeat)) / a.repeat
        return ms

    mom, rounds = MS._moments(bvh)
    lines.append({**base, "stage": "node_moments", "rounds": rounds, "ms": round(mean_ms(lambda: MS._moments(bvh)), 3)})
    print(json.dumps(lines[-1]), flush=True)
    g = torch.Generator(device="cuda").manual_seed(0)
    lo, hi = v.min(0).values, v.max(0).values
    pts = lo + (hi - lo) * torch.rand(a.points, 3, generator=g, device="cuda")
    exact = None
    for beta in a.beta:
        p = pts[:a.exact_points] if beta == 0 else pts
        ms = mean_ms(lambda: MS.winding_numbers(bvh, p, beta, mom))
        w = MS.winding_numbers(bvh, pts[:a.exact_points], beta, mom)
        if beta == 0:
            exact = w
        row = {**base, "stage": "winding_numbers", "beta": beta, "points": int(p.shape[0]), "ms": round(ms, 3),
               "points_per_second": round(p.shape[0] / (ms * 1e-3)), "inside_share": float((w >= 0.5).float().mean())}
        if exact is not None and beta != 0:
            row.update(max_abs_from_exact=float((w - exact).abs().max()), mean_abs_from_exact=float((w - exact).abs().mean()),
                       changed_side=int(((w >= 0.5) != (exact >= 0.5)).sum()), compared=int(w.shape[0]))
        lines.append(row)
        print(json.dumps(row), flush=True)
    for N in a.grid:
        bound, trunc = MS.default_volume(v, N)
        ms = mean_ms(lambda: MS._fill(bvh, mom, c, N, bound, trunc, MS.DEFAULT_BETA))
        lines.append({**base, "stage": "sdf_grid", "grid": N, "beta": MS.DEFAULT_BETA, "bound": bound, "trunc": trunc, "ms": round(ms, 3),
                      "voxels_per_second": round(N ** 3 / (ms * 1e-3))})
        print(json.dumps(lines[-1]), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write("\n".join(json.dumps(x) for x in lines) + "\n")


if __name__ == "__main__":
    main()
