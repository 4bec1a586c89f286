"""Timing of the mesh texture (v3d_amd/recon/mesh_texture.py) on a mesh of the size the reconstruction produces: the bumpy sphere of
tools/mesh_refine_bench.py at N^3 through extract_mesh, decimated to --target_faces as tools/mesh_decimate_bench.py does, 18 orbit cameras
at 512 x 512, frames rendered from the UNDECIMATED mesh with its colours times a stripe finer than the decimated vertex spacing.  Prints one
JSON line per texture size (and writes them to --out): per-view set-up, ms per iteration split into shade, transpose and Adam (second of
two passes), the transpose by the wave-per-row entry v3d_recon_mesh_shade_bwd on the same lists, median and longest list, the share of
texels in any list, and the three PSNRs of fit_texture beside refine_vertex_colors at equal iterations.  Nothing is promised from it.

    python tools/mesh_texture_bench.py [--resolution 256] [--target_faces 50000] [--tex 1024 2048] [--iterations 2000] [--out FILE]
"""
from __future__ import annotations

import argparse
import json
import math
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.dirname(os.path.abspath(__file__))):
    if _p not in sys.path:
        sys.path.insert(0, _p)

STRIPE_PERIOD = 0.03


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--resolution", type=int, default=256)
    ap.add_argument("--target_faces", type=int, default=50000)
    ap.add_argument("--reso", type=int, default=512)
    ap.add_argument("--views", type=int, default=18)
    ap.add_argument("--tex", type=int, nargs="+", default=[1024, 2048])
    ap.add_argument("--iterations", type=int, default=2000)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from mesh_refine_bench import bumpy_sphere_volume, timed
    from v3d_amd.recon import geometry as G
    from v3d_amd.recon import mesh_decimate as MD
    from v3d_amd.recon import mesh_refine as RFN
    from v3d_amd.recon import mesh_render as MR
    from v3d_amd.recon import mesh_texture as MT
    from v3d_amd.recon.cameras import orbit_cameras
    stripe = lambda v: 1.0 - 0.5 * (torch.sin(v[:, 0:1] * (2 * math.pi / STRIPE_PERIOD)) > 0).float()  # noqa: E731
    vf, ff, cf = G.extract_mesh(bumpy_sphere_volume(a.resolution))
    vd, fd, cd, _ = MD.decimate_mesh(vf, ff, cf, a.target_faces)
    cf, cd = cf * stripe(vf), cd * stripe(vd)
    cams, _ = orbit_cameras(a.views, 2.0, 0.0, 60.0, a.reso)
    bg = [1.0, 1.0, 1.0]
    frames = torch.stack([MR.render_mesh(c, vf, ff, cf, bg)["render"] for c in cams])
    v, f, c0 = MR._mesh_on_device(vd, fd, cd, "cuda")
    lib = G.load_library()
    _, rst = RFN.refine_vertex_colors(v, f, c0, cams, frames, iterations=a.iterations, num_opt=0)
    lines = []
    for R in a.tex:
        T = R * R
        setup, views = 0.0, []
        for _ in range(2):                  # (second of two passes: the first loads the libraries and sizes the allocator)
            views.clear()
            setup = timed(lambda: views.extend(MT.prepare_texture_view(cam, v, f, R, bg) for cam in cams)) / len(cams)
        _, baked = MT.bake_vertex_colors(f, c0, R)
        logit = MT.initial_logits(baked).contiguous()
        cur, m, s = torch.sigmoid(logit), torch.zeros_like(logit), torch.zeros_like(logit)
        step = [0]

        def iteration():
            j = step[0] % len(views)
            diff = MT.texture_shade_forward(views[j], cur) - frames[j]
            grad = MT.texture_shade_backward(views[j], diff * (2.0 / diff.numel()))
            step[0] += 1
            MT.color_adam(logit, m, s, grad, cur, step[0], 1e-3)

        vw, grad, out = views[0], torch.zeros(T, 3, device="cuda"), torch.empty(T, 3, device="cuda")
        n = vw.ent_pix.numel()
        wave = lambda: G._check(lib, lib.v3d_recon_mesh_shade_bwd(vw.ranges.data_ptr(), vw.ent_pix.data_ptr(), vw.ent_w.data_ptr(), n,  # noqa: E731
                                                                  frames[0].data_ptr(), a.reso, a.reso, T, out.data_ptr(), G._stream()), "wave")
        parts = {}
        for _ in range(2):
            per_iter = timed(iteration, 200)
            parts = {"shade_ms": timed(lambda: MT.texture_shade_forward(vw, cur), 200),
                     "transpose_ms": timed(lambda: MT.texture_shade_backward(vw, frames[0]), 200),
                     "transpose_wave_per_row_ms": timed(wave, 200),
                     "adam_ms": timed(lambda: MT.color_adam(logit, m, s, grad, cur, 1, 0.0), 200)}
        same = float((out - MT.texture_shade_backward(vw, frames[0])).abs().max())
        ls = MT.list_statistics(views)
        del views, logit, cur, m, s, grad, out
        _, st = MT.fit_texture(v, f, c0, cams, frames, tex_size=R, iterations=a.iterations)
        line = {"resolution": a.resolution, "reso": a.reso, "views": a.views, "triangles_full": int(ff.shape[0]), "triangles": int(f.shape[0]),
                "vertices": int(v.shape[0]), "tex_size": R, "cell": st["cell"], "entries_view0": n, "setup_ms_per_view": round(setup, 3),
                "iteration_ms": round(per_iter, 4), **{k: round(x, 4) for k, x in parts.items()}, "transposes_max_abs_diff": same, **ls,
                "iterations": a.iterations, "fit_seconds": round(st["seconds"], 3), "psnr_vertex": round(st["psnr_vertex"], 2),
                "psnr_baked": round(st["psnr_baked"], 2), "psnr_fitted": round(st["psnr_fitted"], 2), "texels_seen": st["texels_seen"],
                "refine_vertex_colors_psnr_after": round(rst["psnr_after"], 2), "refine_vertex_colors_seconds": round(rst["seconds"], 3),
                "loss_first": st["loss_first"], "loss_last": st["loss_last"], "device": torch.cuda.get_device_name(0)}
        print(json.dumps(line), flush=True)
        lines.append(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write("\n".join(json.dumps(x) for x in lines) + "\n")


if __name__ == "__main__":
    main()
