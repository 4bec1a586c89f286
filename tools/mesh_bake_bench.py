"""Timing of the normal bake (v3d_amd/recon/mesh_bake.py) on a mesh of the size the reconstruction produces: the bumpy sphere of
tools/mesh_refine_bench.py at N^3 through extract_mesh, decimated to --target_faces, baked from the undecimated mesh.  Prints one JSON line
per texture size (and writes them to --out): the BVH build split into keys, sort, nodes and fit rounds (and their count), the bake, both the
second of two passes, the bake's statistics, and the mean angle to the high mesh's normals over 18 views at 512 x 512 before (vertex
normals) and after (the map).  Nothing is promised from it.

    python tools/mesh_bake_bench.py [--resolution 256] [--target_faces 50000] [--tex 1024 2048] [--out FILE]
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


def build_parts(v, f):
    """ms of every step of build_bvh on device tensors, and the fit's round count: the statements of mesh_bake.build_bvh, timed apart"""
    from mesh_refine_bench import timed
    from v3d_amd.ops import get_ops
    from v3d_amd.recon import geometry as G
    from v3d_amd.recon import mesh_bake as MB
    lib, ops = G.load_library(), get_ops()
    V, F = v.shape[0], f.shape[0]
    box = torch.stack([v.min(0).values, v.max(0).values]).cpu().tolist()
    keys, vals = torch.empty(F, dtype=torch.int64, device="cuda"), torch.empty(F, dtype=torch.int32, device="cuda")
    flo, fhi = torch.empty(F, 3, device="cuda"), torch.empty(F, 3, device="cuda")
    left, right = torch.empty(F - 1, dtype=torch.int32, device="cuda"), torch.empty(F - 1, dtype=torch.int32, device="cuda")
    parent = torch.empty(2 * F - 1, dtype=torch.int32, device="cuda")
    lo, hi = torch.empty(2 * F - 1, 3, device="cuda"), torch.empty(2 * F - 1, 3, device="cuda")
    st = {}
    out = {"keys_ms": timed(lambda: G._check(lib, lib.v3d_recon_bvh_face_keys(v.data_ptr(), V, f.data_ptr(), F, *box[0], *box[1], keys.data_ptr(),
                                                                              vals.data_ptr(), flo.data_ptr(), fhi.data_ptr(), G._stream()), "keys")),
           "sort_ms": timed(lambda: st.update(s=ops.gs_radix_sort_pairs(keys, vals, MB.KEY_BITS)))}
    keys_s, order = st["s"]
    out["nodes_ms"] = timed(lambda: G._check(lib, lib.v3d_recon_bvh_build_nodes(keys_s.data_ptr(), order.data_ptr(), flo.data_ptr(), fhi.data_ptr(), F,
                                                                                left.data_ptr(), right.data_ptr(), parent.data_ptr(), lo.data_ptr(),
                                                                                hi.data_ptr(), G._stream()), "nodes"))
    out["fit_ms"] = timed(lambda: st.update(rounds=MB._fit(lib, left, right, F, lo, hi)))
    out["fit_rounds"] = st["rounds"]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--resolution", type=int, default=256)
    ap.add_argument("--target_faces", type=int, default=50000)
    ap.add_argument("--reso", type=int, default=512)
    ap.add_argument("--views", type=int, default=18)
    ap.add_argument("--tex", type=int, nargs="+", default=[1024, 2048])
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from mesh_refine_bench import bumpy_sphere_volume, timed
    from v3d_amd.recon import geometry as G
    from v3d_amd.recon import mesh_bake as MB
    from v3d_amd.recon import mesh_decimate as MD
    from v3d_amd.recon.cameras import orbit_cameras
    vf, ff, _ = G.extract_mesh(bumpy_sphere_volume(a.resolution))
    vd, fd, _, _ = MD.decimate_mesh(vf, ff, None, a.target_faces)
    cams, _ = orbit_cameras(a.views, 2.0, 0.0, 60.0, a.reso)
    parts = {}
    for _ in range(2):                      # (second of two passes: the first loads the libraries and sizes the allocator)
        parts = build_parts(vf, ff)
        parts["build_ms"] = timed(lambda: MB.build_bvh(vf, ff))
    bvh = MB.build_bvh(vf, ff)
    ln, hn = MB._vertex_normals(vd, fd), MB._vertex_normals(vf, ff)
    md = MB.default_max_dist(vf)
    lines = []
    for R in a.tex:
        bake = 0.0
        for _ in range(2):
            bake = timed(lambda: MB.bake_texels(vd, fd, ln, bvh, hn, R, md))
        nm, st = MB.bake_normal_map(vd, fd, vf, ff, tex_size=R)
        fid = MB.normal_map_fidelity(vd, fd, nm, vf, ff, cams)
        line = {"resolution": a.resolution, "reso": a.reso, "views": a.views, "triangles_full": int(ff.shape[0]), "triangles": int(fd.shape[0]),
                "tex_size": R, "cell": st["cell"], **{k: (round(x, 4) if isinstance(x, float) else x) for k, x in parts.items()},
                "bake_ms": round(bake, 3), "bake_normal_map_seconds": round(st["seconds"], 4), "max_dist": st["max_dist"], "owned": st["owned"],
                "hit_plus": st["hit_plus"], "hit_minus": st["hit_minus"], "missed": st["missed"], "displacement_mean": st["displacement_mean"],
                "displacement_max": st["displacement_max"], "angle_before": round(fid["angle_before_mean"], 4),
                "angle_after": round(fid["angle_after_mean"], 4), "device": torch.cuda.get_device_name(0)}
        print(json.dumps(line), flush=True)
        lines.append(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write("\n".join(json.dumps(x) for x in lines) + "\n")


if __name__ == "__main__":
    main()
