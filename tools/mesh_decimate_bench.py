"""Timing of the mesh decimation (v3d_amd/recon/mesh_decimate.py) on a mesh of the size the reconstruction produces: the bumpy sphere of
tools/mesh_clean_bench.py at N^3 through extract_mesh, down to --target_faces.  Prints one JSON line (and writes it to --out): the whole of
decimate_mesh in ms (second of two passes), its rounds and ms per round, the collapses per round, one round's steps on the full mesh
(lists, propose, select, cut, apply), and how far the result is from the input (mesh_fidelity of the result against renders of the input
from 4 cameras).  Nothing is promised from it.

    python tools/mesh_decimate_bench.py [--resolution 256] [--target_faces 50000] [--out FILE]
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
    ap.add_argument("--reso", type=int, default=512)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from mesh_refine_bench import bumpy_sphere_volume, timed
    from v3d_amd.recon import geometry as G
    from v3d_amd.recon import mesh_decimate as MD
    from v3d_amd.recon import mesh_render as MR
    from v3d_amd.recon.cameras import orbit_cameras
    v, f, c = G.extract_mesh(bumpy_sphere_volume(a.resolution))
    V, F = v.shape[0], f.shape[0]
    t, res = {}, []
    for _ in range(2):                  # (second of two passes: the first loads the libraries and sizes the allocator)
        res.clear()
        t["decimate_mesh_ms"] = timed(lambda: res.extend(MD.decimate_mesh(v, f, c, a.target_faces)))
        lists, out = [], []
        t["lists_ms"] = timed(lambda: lists.extend(MD._live_lists(f, V)))
        ranges, corners = lists
        t["quadrics_ms"] = timed(lambda: out.append(MD._quadrics(v, f, ranges, corners)))
        Q = out.pop()
        t["propose_ms"] = timed(lambda: out.extend(MD._propose(v, f, ranges, corners, Q, MD.DEFAULT_MAX_VALENCE)))
        keys, targets = out
        flags = torch.zeros(2, dtype=torch.int32, device=f.device)
        sel = []
        t["select_ms"] = timed(lambda: sel.extend(MD._select(f, V, ranges, corners, keys, float("inf"), flags)))
        live = torch.tensor([F], dtype=torch.int32, device=f.device)
        t["cut_ms"] = timed(lambda: MD._cut(sel[0], sel[1], sel[2], live, a.target_faces))
        t["apply_ms"] = timed(lambda: MD._apply(f, V, sel[0], targets, Q.clone(), torch.zeros(V, dtype=torch.int32, device=f.device)))
    ov, of, oc, stats = res
    cams, _ = orbit_cameras(4, 2.0, 15.0, 60.0, a.reso)
    bg = [1.0, 1.0, 1.0]
    frames = torch.stack([MR.render_mesh(cam, v, f, c, bg)["render"] for cam in cams])
    fid = MR.mesh_fidelity(ov, of, oc, cams, frames, bg)
    rounds = max(1, stats["rounds"])
    line = {"resolution": a.resolution, "vertices": V, "triangles": F, "target_faces": a.target_faces, "vertices_after": int(ov.shape[0]),
            "triangles_after": int(of.shape[0]), "reached": stats["reached"], "stopped": stats["stopped"], "rounds": stats["rounds"],
            "ms_per_round": round(t["decimate_mesh_ms"] / rounds, 4), **{k: round(x, 4) for k, x in t.items()}, "max_cost": stats["max_cost"],
            "accepted_first_rounds": stats["accepted"][:8], "accepted_last_rounds": stats["accepted"][-4:], "psnr_mean_against_input": fid["psnr_mean"],
            "coverage": fid["coverage"], "odd_hit_pixels": fid["odd_hit_pixels"], "device": torch.cuda.get_device_name(0)}
    text = json.dumps(line)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
