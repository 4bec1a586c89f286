"""Timing of the reconstruction step (v3d_amd/recon/) at the documented settings: 18-view 512 x 512 orbit, --sh_degree 0 --lambda_dssim 1.0
--lambda_lpips 0 --num_pts 100000 -w, 4000 iterations.  The orbit is a seeded 3000-Gaussian scene rendered by the HIP forward (no
checkpoints needed).  Prints one JSON line: total seconds, ms per iteration, Gaussian count after densification, final training-view PSNR.

    python tools/recon_bench.py [--iterations 4000] [--reso 512] [--mesh 256 [--refine 2000]]
--mesh N adds the time of the mesh stage on the result (v3d_amd/recon/geometry.py: depth / alpha maps and TSDF fusion of the training views at
N^3, surface nets, the PLY), second of two runs, then renders that mesh (v3d_amd/recon/mesh_render.py): rasterization ms per view at 512 x 512 over
the orbit cameras, and how well the mesh reproduces the training frames (PSNR, coverage, pixels with an odd number of faces over them).
--refine ITERS (with --mesh) then refines the mesh's vertex colours against the training frames (v3d_amd/recon/mesh_refine.py, the defaults of
scripts/pub/refine_mesh.py): ms per iteration, set-up of the optimisation views included, and the mean PSNR over all frames before and after.
    rocprofv3 --kernel-trace --stats -d /tmp/rp -o rp -- python tools/recon_bench.py --iterations 300     # per-kernel split
"""
from __future__ import annotations

import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "tests")):
    if _p not in sys.path:
        sys.path.insert(0, _p)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iterations", type=int, default=4000)
    ap.add_argument("--reso", type=int, default=512)
    ap.add_argument("--views", type=int, default=18)
    ap.add_argument("--num_pts", type=int, default=100_000)
    ap.add_argument("--mesh", type=int, default=0, metavar="N", help="also time fuse_tsdf + extract_mesh + save_mesh_ply at N^3")
    ap.add_argument("--refine", type=int, default=0, metavar="ITERS", help="with --mesh: also refine the mesh's vertex colours for ITERS iterations")
    a = ap.parse_args()
    if a.refine and not a.mesh:
        ap.error("--refine needs --mesh N")
    import gs_dense_ref as D
    from v3d_amd.recon import rasterize as RZ
    from v3d_amd.recon import train as TR
    from v3d_amd.recon.cameras import orbit_cameras
    scene = [t.cuda() for t in D.random_scene(3000, 11, spread=0.3)]
    cams, _ = orbit_cameras(a.views, 2.0, 0.0, 60.0, a.reso)
    with torch.no_grad():
        frames = torch.stack([(RZ.rasterize(*scene, c, [1, 1, 1])[0].clamp(0, 1) * 255).round().to(torch.uint8).permute(1, 2, 0) for c in cams])
    TR.reconstruct(frames[:, :64, :64].contiguous(), iterations=20, num_pts=1000, white_background=True)      # warm-up (library load, allocator)
    g, cams, st = TR.reconstruct(frames, iterations=a.iterations, lambda_dssim=1.0, lambda_lpips=0.0, num_pts=a.num_pts, white_background=True,
                                 seed=0)
    gt = frames.permute(0, 3, 1, 2).float() / 255.0
    bg = torch.ones(3, device="cuda")
    with torch.no_grad():
        ps = [TR.psnr(RZ.render(c, g, bg)["render"].clamp(0, 1), gt[i]) for i, c in enumerate(cams)]
    mesh = {}
    if a.mesh:
        import tempfile
        import time

        from v3d_amd.recon import geometry as GE
        for _ in range(2):      # (the first run loads the library and sizes the allocator)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            vol = GE.fuse_tsdf(g, cams, resolution=a.mesh)
            torch.cuda.synchronize()
            t1 = time.perf_counter()
            verts, faces, colors = GE.extract_mesh(vol)
            torch.cuda.synchronize()
            t2 = time.perf_counter()
            with tempfile.TemporaryDirectory() as d:
                GE.save_mesh_ply(os.path.join(d, "mesh.ply"), verts, faces, colors)
            t3 = time.perf_counter()
        mesh = {"mesh_resolution": a.mesh, "mesh_fuse_ms": round(1000 * (t1 - t0), 2), "mesh_extract_ms": round(1000 * (t2 - t1), 2),
                "mesh_ply_ms": round(1000 * (t3 - t2), 2), "mesh_vertices": int(verts.shape[0]), "mesh_triangles": int(faces.shape[0])}
        from v3d_amd.recon import mesh_render as MR
        if faces.shape[0]:
            rcams, _ = orbit_cameras(a.views, 2.0, 0.0, 60.0, 512)
            mv, mf, mc = MR._mesh_on_device(verts, faces, colors, "cuda")          # validated once, outside the timed loop
            for rep in range(2):      # (second of two runs, as above)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for c in rcams:
                    MR._render_views(c, mv, mf, mc, [1.0, 1.0, 1.0], ((True, False),))
                torch.cuda.synchronize()
                t1 = time.perf_counter()
            fid = MR.mesh_fidelity(verts, faces, colors, cams, frames, [1.0, 1.0, 1.0])
            mesh.update({"mesh_render_ms_per_view_512": round(1000 * (t1 - t0) / len(rcams), 3), "mesh_psnr_mean": round(fid["psnr_mean"], 2),
                         "mesh_psnr_worst": round(min(fid["psnr"]), 2), "mesh_coverage": round(float(np.mean(fid["coverage"])), 4),
                         "mesh_odd_hit_pixels": int(sum(fid["odd_hit_pixels"]))})
            if a.refine:
                from v3d_amd.recon import mesh_refine as RFN
                _, rst = RFN.refine_vertex_colors(verts, faces, colors, cams, frames, iterations=a.refine)
                mesh.update({"refine_iterations": a.refine, "refine_opt_views": rst["opt_views"],
                             "refine_ms_per_iter": round(1000 * rst["seconds"] / a.refine, 4), "refine_psnr_before": round(rst["psnr_before"], 2),
                             "refine_psnr_after": round(rst["psnr_after"], 2)})
    print(json.dumps({**mesh, "iterations": a.iterations, "reso": a.reso, "views": a.views, "num_pts": a.num_pts, "seconds": round(st["seconds"], 2),
                      "ms_per_iter": round(1000 * st["seconds"] / a.iterations, 3), "num_gaussians": st["num_gaussians"],
                      "psnr_mean": round(float(np.mean(ps)), 2), "device": torch.cuda.get_device_name(0)}))


if __name__ == "__main__":
    main()
