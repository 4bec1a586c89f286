"""Timing of the vertex-colour refinement (v3d_amd/recon/mesh_refine.py) on a mesh of the size the reconstruction produces: a bumpy sphere
at N^3 through extract_mesh, 18 orbit cameras at 512 x 512, frames rendered from the mesh itself with position colours, refinement from grey.
Prints one JSON line (and writes it to --out): per-view set-up (rasterize once + per-pixel record + per-vertex lists), ms per iteration
(shade + loss gradient + transpose + Adam, second of two passes), one full _render_views of the same mesh in the same run - what an
iteration's forward alone would cost without frozen visibility - and the PSNR over all 18 frames before and after `--iterations` steps.

    python tools/mesh_refine_bench.py [--resolution 256] [--reso 512] [--iterations 2000] [--out FILE]
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "tests")):
    if _p not in sys.path:
        sys.path.insert(0, _p)


def bumpy_sphere_volume(N: int, bound: float = 1.0, device="cuda"):
    """A TsdfVolume whose zero level is a sphere of radius 0.5 with bumps of a few percent; every voxel observed, colour varying over space"""
    from v3d_amd.recon import geometry as G
    c = (torch.arange(N, dtype=torch.float32, device=device) + 0.5) * (2.0 * bound / N) - bound
    z, y, x = torch.meshgrid(c, c, c, indexing="ij")
    d = torch.sqrt(x * x + y * y + z * z).clamp_min(1e-6)
    rad = 0.5 * (1.0 + 0.06 * torch.sin(7.0 * x / d) * torch.sin(5.0 * y / d) + 0.04 * torch.sin(9.0 * z / d))
    trunc = 4.0 * 2.0 * bound / N
    one = torch.ones(N, N, N, device=device)
    rgb = torch.stack([(0.5 + 0.5 * t / bound).clamp(0, 1) for t in (x, y, z)]).contiguous()
    return G.TsdfVolume(N, bound, trunc, ((d - rad) / trunc).clamp(-1, 1).contiguous(), one, rgb, one.clone())


def timed(fn, reps=1):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return 1000.0 * (time.perf_counter() - t0) / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--resolution", type=int, default=256)
    ap.add_argument("--reso", type=int, default=512)
    ap.add_argument("--views", type=int, default=18)
    ap.add_argument("--iterations", type=int, default=2000)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import mesh_render_ref as M
    from v3d_amd.recon import geometry as G
    from v3d_amd.recon import mesh_refine as RFN
    from v3d_amd.recon import mesh_render as MR
    from v3d_amd.recon.cameras import orbit_cameras
    verts, faces, _ = G.extract_mesh(bumpy_sphere_volume(a.resolution))
    target = M.position_colors(verts.cpu(), (0.9, 0.7, 0.5)).cuda()
    cams, _ = orbit_cameras(a.views, 2.0, 0.0, 60.0, a.reso)
    bg = [1.0, 1.0, 1.0]
    frames = torch.stack([MR.render_mesh(c, verts, faces, target, bg)["render"] for c in cams])
    opt = RFN.optimisation_views(len(cams), 4)
    v, f, c0 = MR._mesh_on_device(verts, faces, torch.full_like(verts, 0.5), "cuda")
    setup = render = 0.0
    for _ in range(2):                  # (second of two passes: the first loads the libraries and sizes the allocator)
        views = []
        setup = timed(lambda: views.extend(RFN.prepare_view(cams[i], v, f, bg) for i in opt)) / len(opt)
        render = timed(lambda: [MR._render_views(cams[i], v, f, c0, bg, ((True, False),)) for i in opt]) / len(opt)
    logit = RFN.initial_logits(c0).contiguous()
    cur, m, s = torch.sigmoid(logit), torch.zeros_like(logit), torch.zeros_like(logit)
    step = [0]

    def iteration():
        j = step[0] % len(opt)
        diff = RFN.shade_forward(views[j], cur) - frames[opt[j]]
        grad = RFN.shade_backward(views[j], diff * (2.0 / diff.numel()))
        step[0] += 1
        RFN.color_adam(logit, m, s, grad, cur, step[0], 1e-3)

    parts = {}
    for _ in range(2):
        per_iter = timed(iteration, 200)
        parts = {"shade_ms": timed(lambda: RFN.shade_forward(views[0], cur), 200),
                 "transpose_ms": timed(lambda: RFN.shade_backward(views[0], frames[0]), 200)}
    _, st = RFN.refine_vertex_colors(verts, faces, c0, cams, frames, iterations=a.iterations)
    line = {"resolution": a.resolution, "reso": a.reso, "views": a.views, "vertices": int(verts.shape[0]), "triangles": int(faces.shape[0]),
            "entries_per_view": [int(vw.ent_pix.numel()) for vw in views], "longest_list": max(int((vw.ranges[:, 1] - vw.ranges[:, 0]).max()) for vw in views),
            "setup_ms_per_view": round(setup, 3), "render_views_ms_per_view": round(render, 3), "iteration_ms": round(per_iter, 4),
            **{k: round(x, 4) for k, x in parts.items()}, "refine_iterations": a.iterations, "refine_seconds": round(st["seconds"], 3),
            "refine_ms_per_iter_with_setup": round(1000 * st["seconds"] / max(a.iterations, 1), 4), "psnr_before": round(st["psnr_before"], 2),
            "psnr_after": round(st["psnr_after"], 2), "loss_first": st["loss_first"], "loss_last": st["loss_last"],
            "vertices_seen": st["vertices_seen"], "device": torch.cuda.get_device_name(0)}
    text = json.dumps(line)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
