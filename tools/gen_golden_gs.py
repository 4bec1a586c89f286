"""TEST INFRASTRUCTURE — generate tests/golden/v3d_gs.pt by running the REFERENCE's own reconstruction helpers (recon/utils/camera_utils.py,
graphics_utils.py, general_utils.py, loss_utils.py and recon/scene/dataset_readers.py constructVideoNVSInfo).

Run in the build container only (needs the reference checkout, see oracle/ref_import.py):   python tools/gen_golden_gs.py
Modules the reference imports at module level but these functions never touch (mediapy, lpipsPyTorch, plyfile, rembg, mcubes, trimesh,
simple_knn, the COLMAP loader) are stubbed in sys.modules.  Stored:
  cameras  for (T, radius, elevation, fov) = (18, 2, 0, 60), (5, 1.5, 15, 40), (24, 2, -10, 60): world_view / full_proj (the reference's
           Camera.world_view_transform / full_proj_transform), camera centres and cameras_extent (getNerfppNorm radius)
  lr       get_expon_lr_func samples over the xyz schedule of OptimizationParams (spatial_lr_scale = 2.2)
  ssim     ssim(img1, img2) and its autograd gradient w.r.t. img1 on two seeded 3 x 40 x 56 image pairs
"""
from __future__ import annotations

import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = os.environ.get("V3D_REFERENCE", "/root/reference")
OUT = os.path.join(ROOT, "tests", "golden", "v3d_gs.pt")


def _stub(name, **attrs):
    m = types.ModuleType(name)
    m.__dict__.update(attrs)
    sys.modules[name] = m


def load_reference():
    recon = os.path.join(REF, "recon")
    sys.path.insert(0, recon)
    _any = lambda *a, **k: None  # noqa: E731
    _stub("mediapy", read_video=_any, write_video=_any)
    _stub("lpipsPyTorch", lpips=_any)
    _stub("lpipsPyTorch.modules")
    _stub("lpipsPyTorch.modules.lpips", LPIPS=object)
    _stub("plyfile", PlyData=object, PlyElement=object)
    for n in ("rembg", "mcubes", "trimesh"):
        _stub(n)
    _stub("simple_knn")
    _stub("simple_knn._C", distCUDA2=_any)
    _stub("scene.colmap_loader", read_extrinsics_text=_any, read_intrinsics_text=_any, qvec2rotmat=_any, read_extrinsics_binary=_any,
          read_intrinsics_binary=_any, read_points3D_binary=_any, read_points3D_text=_any)
    import importlib
    mods = {}
    for n in ("scene.dataset_readers", "utils.graphics_utils", "utils.general_utils", "utils.loss_utils", "utils.camera_utils", "scene.cameras"):
        mods[n.split(".")[-1]] = importlib.import_module(n)
    return mods


def main():
    m = load_reference()
    cams_out = []
    for (T, radius, elevation, fov) in ((18, 2.0, 0.0, 60.0), (5, 1.5, 15.0, 40.0), (24, 2.0, -10.0, 60.0)):
        poses = m["camera_utils"].get_uniform_poses(T, radius, elevation)
        w2cs = np.linalg.inv(poses)
        gu = m["graphics_utils"]
        wv, fp, cc = [], [], []
        infos = []
        for pose in w2cs:
            R, t = np.transpose(pose[:3, :3]), pose[:3, 3]
            fovr = np.deg2rad(fov)
            w = torch.tensor(gu.getWorld2View2(R, t, np.array([0.0, 0.0, 0.0]), 1.0)).transpose(0, 1)
            p = gu.getProjectionMatrix(znear=0.01, zfar=100.0, fovX=fovr, fovY=fovr).transpose(0, 1)
            f = w.unsqueeze(0).bmm(p.unsqueeze(0)).squeeze(0)
            wv.append(w), fp.append(f), cc.append(w.inverse()[3, :3])
            infos.append(types.SimpleNamespace(R=R, T=t))
        extent = m["dataset_readers"].getNerfppNorm(infos)["radius"]
        cams_out.append({"T": T, "radius": radius, "elevation": elevation, "fov": fov, "world_view": torch.stack(wv), "full_proj": torch.stack(fp),
                         "center": torch.stack(cc), "extent": float(extent)})
    f = m["general_utils"].get_expon_lr_func(lr_init=0.00016 * 2.2, lr_final=0.0000016 * 2.2, lr_delay_mult=0.01, max_steps=30_000)
    steps = [0, 1, 2, 10, 100, 999, 1000, 4000, 15_000, 29_999, 30_000, 40_000]
    lr = {"steps": steps, "values": torch.tensor([float(f(s)) for s in steps], dtype=torch.float64), "lr_init": 0.00016 * 2.2,
          "lr_final": 0.0000016 * 2.2, "lr_delay_mult": 0.01, "max_steps": 30_000}
    ssim = []
    for seed in (0, 1):
        g = torch.Generator().manual_seed(seed)
        a = torch.rand(3, 40, 56, generator=g)
        b = (a + 0.2 * torch.randn(3, 40, 56, generator=g)).clamp(0, 1)
        ar = a.clone().requires_grad_(True)
        v = m["loss_utils"].ssim(ar, b)
        v.backward()
        ssim.append({"img1": a, "img2": b, "value": v.detach(), "grad": ar.grad.detach()})
    torch.save({"cameras": cams_out, "lr": lr, "ssim": ssim}, OUT)
    print(f"wrote {OUT} ({os.path.getsize(OUT)} bytes)")


if __name__ == "__main__":
    main()
