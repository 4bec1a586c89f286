#!/usr/bin/env python
"""Generated orbit -> 3-D Gaussians on MI355X (the reference's recon/train_from_vid.py, step 4 of V3D), on the gfx950 splat kernels.

    python scripts/pub/recon_from_vid.py -w --sh_degree 0 --iterations 4000 --lambda_dssim 1.0 --lambda_lpips 0 \\
           --save_iterations 4000 --num_pts 100000 --video outputs/V3D_512/000000.npy -m out/gs --render_orbit 36
    python scripts/pub/recon_from_vid.py -w --input_path assets/img.png --synthetic --iterations 500 -m out/gs2

--video takes the .npy that V3D_512.py --save writes without mediapy, a folder of PNG frames (sorted by name), or an .mp4 when mediapy is
installed.  --input_path generates the orbit in-process (scripts/pub/V3D_512.py sample_one) and hands model.last_frames_u8 over on the device.
Writes <model_path>/point_cloud/iteration_<n>/point_cloud.ply (the reference's layout and attributes).  SH degree 0 only; LPIPS is not
available (pass --lambda_lpips 0).  --save_mesh fuses depth maps of the training views into a TSDF and writes a coloured triangle mesh
(v3d_amd/recon/geometry.py); --render_depth N writes N turntable frames of normalised depth."""
from __future__ import annotations

import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def load_video(path: str, num_frames=None) -> np.ndarray:
    """uint8 frames [T, H, W, 3] from an .npy, a folder of PNGs or an .mp4 (mediapy)."""
    if os.path.isdir(path):
        from PIL import Image
        names = sorted(f for f in os.listdir(path) if f.lower().endswith(".png"))
        if not names:
            raise SystemExit(f"{path}: no .png frames")
        frames = np.stack([np.asarray(Image.open(os.path.join(path, f)).convert("RGB")) for f in names])
    elif path.endswith(".npy"):
        frames = np.load(path)
    elif path.endswith(".mp4"):
        try:
            import mediapy
        except ImportError:
            raise SystemExit(f"{path}: reading .mp4 needs mediapy, which is not installed; pass the .npy V3D_512.py --save writes or a PNG folder")
        frames = np.asarray(mediapy.read_video(path))
    else:
        raise SystemExit(f"{path}: --video must be an .npy, a folder of PNGs or an .mp4")
    if frames.dtype != np.uint8 or frames.ndim != 4 or frames.shape[-1] not in (3, 4):
        raise SystemExit(f"{path}: expected uint8 frames [T, H, W, 3], got {frames.dtype} {frames.shape}")
    frames = frames[..., :3]
    if num_frames is not None and num_frames != frames.shape[0]:
        raise SystemExit(f"{path}: {frames.shape[0]} frames, --num_frames says {num_frames}")
    return frames


def save_frames(frames: np.ndarray, folder: str):
    from PIL import Image
    os.makedirs(folder, exist_ok=True)
    np.save(os.path.join(folder, "orbit.npy"), frames)
    for i, f in enumerate(frames):
        Image.fromarray(f).save(os.path.join(folder, f"{i:03d}.png"))


def build_parser() -> argparse.ArgumentParser:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("-w", "--white_background", action="store_true")
    ap.add_argument("--sh_degree", type=int, default=0)
    ap.add_argument("--iterations", type=int, default=4000)
    ap.add_argument("--lambda_dssim", type=float, default=0.2)
    ap.add_argument("--lambda_lpips", type=float, default=0.0)
    ap.add_argument("--save_iterations", type=int, nargs="+", default=None, help="default: the last iteration")
    ap.add_argument("--num_pts", type=int, default=100_000)
    ap.add_argument("--num_frames", type=int, default=None, help="frames of the orbit (default: all frames of --video, 18 with --input_path)")
    ap.add_argument("--radius", type=float, default=2.0)
    ap.add_argument("--elevation", type=float, default=0.0)
    ap.add_argument("--fov", type=float, default=60.0)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("-m", "--model_path", default="outputs/recon")
    ap.add_argument("--video", default=None)
    ap.add_argument("--input_path", default=None, help="generate the orbit from this image in-process (V3D_512.py sample_one)")
    ap.add_argument("--synthetic", action="store_true", help="with --input_path: random-init weights (no checkpoints)")
    ap.add_argument("--checkpoint_path", default=None)
    ap.add_argument("--num_steps", type=int, default=None)
    ap.add_argument("--render_orbit", type=int, default=0, help="write N turntable frames of the result to <model_path>/orbit/")
    ap.add_argument("--save_mesh", nargs="?", const="", default=None, metavar="PATH",
                    help="fuse the orbit views' depth into a TSDF and write a coloured triangle mesh (default PATH: <model_path>/mesh.ply)")
    ap.add_argument("--mesh_resolution", type=int, default=256, help="voxels per axis of the TSDF volume of --save_mesh (at most 512)")
    ap.add_argument("--render_depth", type=int, default=0, help="write N turntable frames of normalised depth to <model_path>/depth.npy (float32)")
    return ap


def main(argv=None):
    ap = build_parser()
    a = ap.parse_args(argv)
    if a.save_mesh is not None and not 2 <= a.mesh_resolution <= 512:
        ap.error("--mesh_resolution must lie in 2 .. 512")
    from v3d_amd.recon import train
    try:
        train.check_options(a.sh_degree, a.lambda_lpips)
    except NotImplementedError as e:
        ap.error(str(e))
    if (a.video is None) == (a.input_path is None):
        ap.error("give exactly one of --video and --input_path")
    if a.video is not None:
        frames = load_video(a.video, a.num_frames)
    else:
        import torch
        sys.path.insert(0, os.path.join(ROOT, "scripts", "pub"))
        from V3D_512 import sample_one
        image = None
        if os.path.isfile(a.input_path):
            from PIL import Image
            im = Image.open(a.input_path).convert("RGB").resize((512, 512))
            image = torch.from_numpy(np.asarray(im).copy()).permute(2, 0, 1)[None].float() / 127.5 - 1.0
        elif not a.synthetic:
            raise SystemExit(f"input image {a.input_path} not found (pass --synthetic to run on synthetic conditioning)")
        _, model = sample_one(a.input_path, a.checkpoint_path, a.num_frames, a.num_steps, synthetic=a.synthetic, image=image)
        frames = model.last_frames_u8          # [T, H, W, 3] uint8, still on the device
    it = a.iterations
    saves = a.save_iterations or [it]
    g, _, st = train.reconstruct(frames, model_path=a.model_path, iterations=it, save_iterations=saves, sh_degree=a.sh_degree,
                                 lambda_dssim=a.lambda_dssim, lambda_lpips=a.lambda_lpips, num_pts=a.num_pts, radius=a.radius,
                                 elevation=a.elevation, fov=a.fov, white_background=a.white_background, seed=a.seed, log_every=500)
    print(f"[recon] {it} iterations in {st['seconds']:.1f} s ({1000 * st['seconds'] / it:.2f} ms/iter), {st['num_gaussians']} Gaussians; "
          f"PLY: {os.path.join(a.model_path, 'point_cloud', f'iteration_{saves[-1]}', 'point_cloud.ply')}")
    if a.render_orbit:
        reso = int(frames.shape[1])
        orbit = train.render_orbit(g, a.render_orbit, a.radius, a.elevation, a.fov, reso, a.white_background)
        save_frames(orbit, os.path.join(a.model_path, "orbit"))
        print(f"[recon] {a.render_orbit} turntable frames -> {os.path.join(a.model_path, 'orbit')}")
    if a.render_depth:
        from v3d_amd.recon import geometry
        path = os.path.join(a.model_path, "depth.npy")
        os.makedirs(a.model_path, exist_ok=True)
        np.save(path, geometry.render_depth_orbit(g, a.render_depth, a.radius, a.elevation, a.fov, int(frames.shape[1]), a.white_background))
        print(f"[recon] {a.render_depth} normalised depth frames -> {path}")
    if a.save_mesh is not None:
        from v3d_amd.recon import geometry
        from v3d_amd.recon.cameras import orbit_cameras
        path = a.save_mesh or os.path.join(a.model_path, "mesh.ply")
        cams, _ = orbit_cameras(int(frames.shape[0]), a.radius, a.elevation, a.fov, int(frames.shape[1]))
        vol = geometry.fuse_tsdf(g, cams, resolution=a.mesh_resolution, bg=[1.0, 1.0, 1.0] if a.white_background else [0.0, 0.0, 0.0])
        verts, faces, colors = geometry.extract_mesh(vol)
        geometry.save_mesh_ply(path, verts, faces, colors)
        print(f"[recon] mesh: {verts.shape[0]} vertices, {faces.shape[0]} triangles at {a.mesh_resolution}^3 -> {path}")


if __name__ == "__main__":
    main()
