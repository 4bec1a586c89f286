"""Timing of the tangent-space kernels (v3d_amd/recon/mesh_gltf.py) on the scene of tools/mesh_bake_bench.py: the bumpy sphere at N^3 through
extract_mesh against its decimation to --target_faces.  Prints one JSON line per measurement (and writes them to --out): the corner frames,
encode and decode at every --tex, the lit shade of one --reso view, each as the mean of --reps launches between device events in the second
of two passes, with the bytes the kernel has to move (computed from the shapes, below) and the rate that gives; then the size of the GLB
with the albedo and the normal map.  Nothing is promised from it and nothing is compared against a threshold.

    python tools/mesh_tangent_bench.py [--resolution 256] [--target_faces 50000] [--tex 1024 2048] [--reso 512] [--reps 20] [--out FILE]
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import tempfile
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.dirname(os.path.abspath(__file__))):
    if _p not in sys.path:
        sys.path.insert(0, _p)

HBM_COPY_RATE = 6.29e12          # bytes/s: the chip's measured float4 copy rate, the yardstick for a streaming kernel


def event_ms(fn, reps):
    """mean milliseconds of `reps` back-to-back launches between two device events"""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--resolution", type=int, default=256)
    ap.add_argument("--target_faces", type=int, default=50000)
    ap.add_argument("--tex", type=int, nargs="+", default=[1024, 2048])
    ap.add_argument("--reso", type=int, default=512)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from mesh_refine_bench import bumpy_sphere_volume
    from v3d_amd.recon import geometry as G
    from v3d_amd.recon import mesh_bake as MB
    from v3d_amd.recon import mesh_decimate as MD
    from v3d_amd.recon import mesh_gltf as MG
    from v3d_amd.recon import mesh_texture as MT
    from v3d_amd.recon.cameras import orbit_cameras
    vf, ff, _ = G.extract_mesh(bumpy_sphere_volume(a.resolution))
    vd, fd, _, _ = MD.decimate_mesh(vf, ff, None, a.target_faces)
    V, F = int(vd.shape[0]), int(fd.shape[0])
    base = {"resolution": a.resolution, "triangles_full": int(ff.shape[0]), "triangles": F, "device": torch.cuda.get_device_name(0), "reps": a.reps}
    ln = MB._vertex_normals(vd, fd)
    lines = []

    def report(stage, ms, nbytes, **more):
        lines.append({**base, "stage": stage, "ms": round(ms, 4), "bytes": int(nbytes), "GB_per_s": round(nbytes / (ms * 1e-3) / 1e9, 1),
                      "share_of_copy_rate": round(nbytes / (ms * 1e-3) / HBM_COPY_RATE, 4), **more})
        print(json.dumps(lines[-1]), flush=True)

    # frames: faces 12 F, the vertices and normals once each (24 V), out 36 F + 48 F
    frame_bytes = 12 * F + 24 * V + 84 * F
    ms = 0.0
    for _ in range(2):
        ms = event_ms(lambda: MG.frames_on_device(vd, fd, ln), a.reps)
    report("corner_frames", ms, frame_bytes)
    cn, ct = MG.frames_on_device(vd, fd, ln)
    cam = orbit_cameras(4, 2.0, 15.0, 60.0, a.reso)[0][0]
    for R in a.tex:
        nm, _ = MB.bake_normal_map(vd, fd, vf, ff, tex_size=R)
        # per texel: the map in (12), the map and the owner out (16); the frames (84 F) and the faces (12 F) once
        nbytes = 28 * R * R + 96 * F
        tm = None
        for enc, src in ((True, nm), (False, None)):
            src = src if enc else tm
            for _ in range(2):
                ms = event_ms(lambda: MG.convert_texels(fd, V, cn, ct, src, R, enc), a.reps)
            report("encode_tangent" if enc else "decode_tangent", ms, nbytes, tex_size=R)
            if enc:
                tm = MG.convert_texels(fd, V, cn, ct, nm, R, True)[1]
        _, albedo = MT.bake_vertex_colors(fd, (0.5 + 0.6 * vd).clamp(0, 1), R)
        lit = MG.prepare_lit_view(cam, vd, fd, R, [1.0, 1.0, 1.0], normals=ln, frames=(cn, ct))
        ao = torch.ones(R * R, device=vd.device)
        covered = int((lit.view.face_id >= 0).sum())
        # per pixel: face_id, pix_w, pix_tex, pix_tw in (48), image and normals out (24); per covered pixel four taps of three maps (112)
        # and the face's frames (84)
        nbytes = 72 * a.reso * a.reso + 196 * covered
        for _ in range(2):
            ms = event_ms(lambda: MG.shade_lit(lit, albedo, tm, ao), a.reps)
        report("shade_lit", ms, nbytes, tex_size=R, reso=a.reso, covered=covered)
        with tempfile.TemporaryDirectory() as d:
            t0 = time.perf_counter()
            size = MG.save_glb(os.path.join(d, "m.glb"), vd, fd, albedo, tangent_map=tm, tex_size=R, corner_normals=cn, corner_tangents=ct)
            lines.append({**base, "stage": "save_glb", "tex_size": R, "maps": ["albedo", "normal"], "bytes": int(size),
                          "seconds": round(time.perf_counter() - t0, 3)})
            print(json.dumps(lines[-1]), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write("\n".join(json.dumps(x) for x in lines) + "\n")


if __name__ == "__main__":
    main()
