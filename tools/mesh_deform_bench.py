"""Timing of the silhouette fit (v3d_amd/recon/mesh_deform.py) on a mesh of the size the reconstruction produces: a bumpy sphere at N^3 through
extract_mesh, decimated to --faces triangles, 18 orbit cameras at 512 x 512, targets the antialiased alpha of the mesh itself before it is
shrunk by 3 %.  Prints one JSON line (and writes it to --out): ms per iteration of fit_vertices' loop (second of two passes) and its split
into rasterize (project + binning + render), alpha (the antialiasing pass), backward (count, scan, emit, sort, ranges, reduce, projection)
and Adam (loss, regularisers and torch.optim.Adam), each timed alone on one view; and what `--iterations` steps reach.

    python tools/mesh_deform_bench.py [--resolution 256] [--faces 50000] [--reso 512] [--iterations 200] [--out FILE]
"""
from __future__ import annotations

import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")):
    if _p not in sys.path:
        sys.path.insert(0, _p)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--resolution", type=int, default=256)
    ap.add_argument("--faces", type=int, default=50000)
    ap.add_argument("--reso", type=int, default=512)
    ap.add_argument("--views", type=int, default=18)
    ap.add_argument("--iterations", type=int, default=200)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from mesh_refine_bench import bumpy_sphere_volume, timed
    from v3d_amd.recon import geometry as G
    from v3d_amd.recon import mesh_deform as MD
    from v3d_amd.recon import mesh_render as MR
    from v3d_amd.recon.cameras import orbit_cameras
    from v3d_amd.recon.mesh_decimate import decimate_mesh
    from v3d_amd.recon.rasterize import gs_camera
    verts, faces, _ = G.extract_mesh(bumpy_sphere_volume(a.resolution))
    verts, faces, _, _ = decimate_mesh(verts, faces, None, a.faces)
    cams, _ = orbit_cameras(a.views, 2.0, 0.0, 60.0, a.reso)
    v, f, _ = MR._mesh_on_device(verts, faces, verts, "cuda")
    V = v.shape[0]
    targets = torch.stack([MD.antialiased_alpha(c, v, f).detach() for c in cams])
    start = (0.97 * v).contiguous()
    gc = gs_camera(cams[0], [0.0, 0.0, 0.0])
    lists = MD.corner_lists(f, V)
    d = torch.zeros_like(start, requires_grad=True)
    opt = torch.optim.Adam([d], lr=1e-4)
    zeros = torch.zeros(V, 3, device="cuda")
    fwd = MD.alpha_forward(gc, start, f)
    dL = (fwd["alpha_aa"] - targets[0]) * (2.0 / targets[0].numel())
    step = [0]

    def iteration():
        i = step[0] % len(cams)
        step[0] += 1
        keep = MD.AlphaView()
        opt.zero_grad(set_to_none=True)
        with torch.enable_grad():
            diff = MD._Alpha.apply(start + d, f, gs_camera(cams[i], [0.0, 0.0, 0.0]), 8, keep) - targets[i]
            ((diff * diff).mean() + MD.LAMBDA_OFFSET * (d * d).sum(1).mean() + MD.LAMBDA_SMOOTH * MD.smooth_energy(d, f, lists)).backward()
        opt.step()

    def rasterize():
        zv, _, pix_q = MR.project_vertices(gc, start, 8)
        MR.rasterize_projected(gc, f, pix_q, zv, zeros, True, False, 8)

    def regularisers_and_adam():
        opt.zero_grad(set_to_none=True)
        with torch.enable_grad():
            (MD.LAMBDA_OFFSET * (d * d).sum(1).mean() + MD.LAMBDA_SMOOTH * MD.smooth_energy(d, f, lists)).backward()
        opt.step()

    per_iter, parts = 0.0, {}
    for _ in range(2):                  # (second of two passes: the first loads the libraries and sizes the allocator)
        per_iter = timed(iteration, 50)
        parts = {"rasterize_ms": timed(rasterize, 50),
                 "alpha_ms": timed(lambda: MD.aa_forward(fwd["face_id"], f, fwd["pix_f"], fwd["pix_q"]), 50),
                 "backward_ms": timed(lambda: MD.alpha_backward(gc, start, f, fwd, dL), 50),
                 "adam_ms": timed(regularisers_and_adam, 50)}
    _, st = MD.fit_vertices(start, f, cams, targets, iterations=a.iterations)
    line = {"resolution": a.resolution, "reso": a.reso, "views": a.views, "vertices": int(V), "triangles": int(f.shape[0]),
            "pairs_per_view": st["pairs"], "iteration_ms": round(per_iter, 4), **{k: round(x, 4) for k, x in parts.items()},
            "fit_iterations": a.iterations, "fit_seconds": round(st["seconds"], 3), "mse_before": st["mse_before"], "mse_after": st["mse_after"],
            "iou_before": st["iou_before"], "iou_after": st["iou_after"], "max_offset": st["max_offset"], "vertices_moved": st["vertices_moved"],
            "device": torch.cuda.get_device_name(0)}
    text = json.dumps(line)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
