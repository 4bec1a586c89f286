"""Timing of the mesh alignment (v3d_amd/recon/mesh_align.py) on a mesh of the size the reconstruction produces: the bumpy sphere of
tools/mesh_refine_bench.py at N^3 through extract_mesh, decimated to --target_faces as tools/mesh_decimate_bench.py does and moved by a known
similarity, against the undecimated mesh, at `subdivide` 2.  Prints one JSON line (and writes it to --out): ms per ICP iteration split into
the correspond launch, the reduce launch and the host's share (read-back and solve);  the same iteration built from the entries that were
there before (a torch transform, closest_points, the closest points and the float64 moments in torch), on the same run;  seconds for 24
starts of 10 iterations;  seconds and iterations of a whole align_mesh;  seconds for score_meshes at --iou_resolution.  Nothing is promised
from it.

    python tools/mesh_align_bench.py [--resolution 256] [--target_faces 50000] [--subdivide 2] [--iou_resolution 128] [--out FILE]
"""
from __future__ import annotations

import argparse
import json
import math
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.dirname(os.path.abspath(__file__))):
    if _p not in sys.path:
        sys.path.insert(0, _p)


def known_motion():
    """12 degrees about (1, 2, 3), scale 1.08, shift (0.05, -0.03, 0.04)"""
    k = np.array([1.0, 2.0, 3.0]) / math.sqrt(14.0)
    K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    a = math.radians(12.0)
    T = np.eye(4)
    T[:3, :3] = 1.08 * (np.eye(3) + math.sin(a) * K + (1 - math.cos(a)) * (K @ K))
    T[:3, 3] = (0.05, -0.03, 0.04)
    return T


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--resolution", type=int, default=256)
    ap.add_argument("--target_faces", type=int, default=50000)
    ap.add_argument("--subdivide", type=int, default=2)
    ap.add_argument("--iou_resolution", type=int, default=128)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from mesh_refine_bench import bumpy_sphere_volume, timed
    from v3d_amd.recon import geometry as G
    from v3d_amd.recon import mesh_align as MA
    from v3d_amd.recon import mesh_bake as MB
    from v3d_amd.recon import mesh_decimate as MD
    from v3d_amd.recon import mesh_query as MQ
    vf, ff, cf = G.extract_mesh(bumpy_sphere_volume(a.resolution))
    vd, fd, _, _ = MD.decimate_mesh(vf, ff, cf, a.target_faces)
    T0 = known_motion()
    vm = MA.transform_vertices(vd, T0).cuda().contiguous()
    fd = fd.cuda().to(torch.int32).contiguous()
    pts, w = MQ.face_samples(vm, fd, a.subdivide)
    bvh = MB.build_bvh(vf, ff)
    T = MA.start_transform(0, vm.double().cpu().numpy(), vf.double().cpu().numpy(), "similarity")
    lib = G.load_library()
    N = pts.shape[0]
    rows = (N + 63) // 64
    r = MA.correspond(bvh, pts, w, T)                   # (loads the library, sizes the allocator, and gives the buffers for the raw calls)
    xf = np.ascontiguousarray(T[:3].astype(np.float32))
    sums = torch.empty(20, dtype=torch.float64, device="cuda")
    launch = lambda: G._check(lib, lib.v3d_recon_align_correspond(pts.data_ptr(), w.data_ptr(), N, xf.ctypes.data, math.inf, *bvh._args(),  # noqa: E731
                                                                  r["moved"].data_ptr(), r["closest"].data_ptr(), r["dist"].data_ptr(), r["face"].data_ptr(),
                                                                  r["uv"].data_ptr(), r["partials"].data_ptr(), G._stream()), "correspond")
    reduce = lambda: G._check(lib, lib.v3d_recon_align_reduce(r["partials"].data_ptr(), rows, sums.data_ptr(), G._stream()), "reduce")  # noqa: E731
    iteration = lambda: MA.solve_similarity(MA.correspond(bvh, pts, w, T)["sums"], "similarity")  # noqa: E731

    Rt = torch.as_tensor(T[:3, :3].T, dtype=torch.float32, device="cuda")
    tt = torch.as_tensor(T[:3, 3], dtype=torch.float32, device="cuda")
    fl = bvh.faces.long()

    def torch_iteration():
        """the same step from the entries of mesh_query alone: 20 sums in float64 on the device, one read-back"""
        p = pts @ Rt + tt
        dist, face, uv = MQ.closest_points(bvh, p)
        tri = fl[face.long().clamp_min(0)]
        va, vb, vc = bvh.verts[tri[:, 0]], bvh.verts[tri[:, 1]], bvh.verts[tri[:, 2]]
        q = va + uv[:, 0:1] * (vb - va) + uv[:, 1:2] * (vc - va)
        ok = (face >= 0) & torch.isfinite(w) & (w >= 0)
        w64 = torch.where(ok, w, torch.zeros_like(w)).double()
        p64, q64 = p.double(), torch.where(ok[:, None], q, torch.zeros_like(q)).double()
        s = torch.cat([w64.sum()[None], (w64[:, None] * p64).sum(0), (w64[:, None] * q64).sum(0),
                       ((w64[:, None] * q64)[:, :, None] * p64[:, None, :]).sum(0).reshape(9), (w64 * (p64 * p64).sum(1))[None].sum(1),
                       (w64 * dist.double().nan_to_num(0.0, 0.0, 0.0) ** 2).sum()[None], ok.sum().double()[None], w64.sum()[None]])
        return MA.solve_similarity(s.cpu(), "similarity")

    out = {}
    for _ in range(2):                                  # (second of two passes)
        out = {"correspond_ms": timed(launch, a.reps), "reduce_ms": timed(reduce, a.reps), "iteration_ms": timed(iteration, a.reps),
               "torch_iteration_ms": timed(torch_iteration, a.reps), "closest_points_ms": timed(lambda: MQ.closest_points(bvh, r["moved"]), a.reps)}
    out["host_ms"] = out["iteration_ms"] - out["correspond_ms"] - out["reduce_ms"]
    same = float(np.abs(iteration() - torch_iteration()).max())
    _, st24 = MA.align_mesh(vm, fd, vf, ff, starts=24, iterations=10, start_iterations=10, tol=0.0, subdivide=a.subdivide)
    M, st = MA.align_mesh(vm, fd, vf, ff, subdivide=a.subdivide)
    res = MA.decompose(M @ T0)
    sc = MA.score_meshes(MA.transform_vertices(vm, M), fd, vf, ff, iou_resolution=a.iou_resolution, subdivide=a.subdivide)
    line = {"resolution": a.resolution, "triangles_full": int(ff.shape[0]), "triangles": int(fd.shape[0]), "subdivide": a.subdivide, "samples": N,
            **{k: round(x, 4) for k, x in out.items()}, "both_paths_max_abs_diff": same, "starts24_seconds": round(st24["seconds"], 3),
            "starts24_chosen": st24["start"], "align_seconds": round(st["seconds"], 3), "align_iterations": st["iterations_run"], "align_rms": st["rms"],
            "residual_degrees": res["rotation_angle"], "residual_scale": res["scale"], "score_seconds": round(sc["seconds"], 3),
            "iou_resolution": a.iou_resolution, "chamfer_relative": sc["relative"]["chamfer"], "fscore": [f["fscore"] for f in sc["fscore"]],
            "normal_consistency": sc["normal_consistency"]["mean"], "iou": sc["volume_iou"]["iou"] if sc["volume_iou"] else None,
            "device": torch.cuda.get_device_name(0)}
    print(json.dumps(line), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
