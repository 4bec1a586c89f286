"""Reconstruction loop (reference: recon/train_from_vid.py, recon/scene/__init__.py, recon/arguments/__init__.py OptimizationParams).

Per iteration: xyz learning rate from the exponential schedule; one view popped at random from a shuffled stack; render on the HIP
rasterizer; loss = (1 - lambda_dssim) L1 + lambda_dssim (1 - SSIM) + 0.1 mean(opacity); backward; densification statistics, densify / prune,
opacity reset; Adam.  One `seed` seeds python `random`, numpy and torch (the reference's safe_state) and the split sampler, so a run is
reproducible bit for bit."""
from __future__ import annotations

import dataclasses
import math
import os
import random
import time
from typing import Iterable, Optional

import numpy as np
import torch

from .cameras import orbit_cameras
from .gaussians import GaussianModel, sh_to_rgb
from .rasterize import render, ssim_l1_loss


@dataclasses.dataclass
class OptimizationParams:
    iterations: int = 30_000
    position_lr_init: float = 0.00016
    position_lr_final: float = 0.0000016
    position_lr_delay_mult: float = 0.01
    position_lr_max_steps: int = 30_000
    feature_lr: float = 0.0025
    opacity_lr: float = 0.05
    scaling_lr: float = 0.005
    rotation_lr: float = 0.001
    percent_dense: float = 0.01
    lambda_dssim: float = 0.2
    lambda_lpips: float = 0.0
    densification_interval: int = 100
    opacity_reset_interval: int = 3000
    densify_from_iter: int = 500
    densify_until_iter: int = 15_000
    densify_grad_threshold: float = 0.0002


def check_options(sh_degree: int = 0, lambda_lpips: float = 0.0):
    if sh_degree != 0:
        raise NotImplementedError(f"--sh_degree {sh_degree}: only SH degree 0 is implemented (V3D's documented command passes --sh_degree 0)")
    if lambda_lpips > 0:
        raise NotImplementedError(f"--lambda_lpips {lambda_lpips}: LPIPS needs VGG weights that this build does not ship; pass --lambda_lpips 0")


def seed_all(seed: int):
    random.seed(seed)
    np.random.seed(seed)
    torch.manual_seed(seed)


def frames_to_images(frames, device) -> torch.Tensor:
    """uint8 frames [T, H, W, 3] (numpy or tensor, host or device) -> fp32 [T, 3, H, W] in [0, 1] on `device`; frames must be square."""
    f = frames if torch.is_tensor(frames) else torch.from_numpy(np.ascontiguousarray(frames))
    if f.dim() != 4 or f.shape[-1] < 3:
        raise ValueError(f"frames must be [T, H, W, 3] uint8, got {tuple(f.shape)}")
    if f.shape[1] != f.shape[2]:
        raise ValueError(f"frames are {f.shape[2]} x {f.shape[1]}: the orbit cameras are square (width = height = reso), as in the reference")
    return (f[..., :3].to(device).permute(0, 3, 1, 2).float() / 255.0).contiguous()


def initial_points(num_pts: int, radius: float):
    """The reference's random initialisation: randn * radius / 16 (drawn twice, the first draw discarded, as constructVideoNVSInfo does) and
    SH colour 0.2 passed through its uint8 point-cloud file."""
    np.random.randn(num_pts, 3)
    xyz = np.random.randn(num_pts, 3) * radius / 16
    shs = np.ones((num_pts, 3)) * 0.2
    rgb = (sh_to_rgb(shs) * 255).astype(np.uint8).astype(np.float32) / 255.0
    return torch.tensor(xyz, dtype=torch.float32), torch.tensor(rgb, dtype=torch.float32)


@torch.enable_grad()
def reconstruct(frames, *, model_path: Optional[str] = None, iterations: int = 4000, save_iterations: Iterable[int] = (), sh_degree: int = 0,
                lambda_dssim: float = 0.2, lambda_lpips: float = 0.0, num_pts: int = 100_000, radius: float = 2.0, elevation: float = 0.0,
                fov: float = 60.0, white_background: bool = False, seed: int = 0, device="cuda", opt: Optional[OptimizationParams] = None,
                log_every: int = 0):
    """Fit 3-D Gaussians to an orbit video; returns (GaussianModel, cameras, stats).  PLYs of `save_iterations` go to
    <model_path>/point_cloud/iteration_<n>/point_cloud.ply."""
    check_options(sh_degree, lambda_lpips)
    opt = dataclasses.replace(opt or OptimizationParams(), iterations=iterations, lambda_dssim=lambda_dssim, lambda_lpips=lambda_lpips)
    seed_all(seed)
    images = frames_to_images(frames, device)
    T, _, reso, _ = images.shape
    cams, extent = orbit_cameras(T, radius, elevation, fov, reso, device="cpu")
    train = list(range(T))
    random.shuffle(train)       # the Scene's shuffle of its training cameras
    xyz, rgb = initial_points(num_pts, radius)
    g = GaussianModel(sh_degree)
    g.create_from_points(xyz.to(device), rgb.to(device), extent)
    g.training_setup(opt, seed=seed)
    bg = torch.tensor([1.0, 1.0, 1.0] if white_background else [0.0, 0.0, 0.0], device=device)
    save_iterations = set(save_iterations)
    stack = None
    t0 = time.perf_counter()
    stats = {"extent": extent, "num_initial": num_pts}
    for it in range(1, opt.iterations + 1):
        g.update_learning_rate(it)
        if not stack:
            stack = train.copy()
        view = stack.pop(random.randint(0, len(stack) - 1))
        pkg = render(cams[view], g, bg)
        loss, _ssim, _l1 = ssim_l1_loss(pkg["render"], images[view], opt.lambda_dssim)
        if g.xyz.shape[0]:
            loss = loss + torch.mean(g.get_opacity) * 0.1
        loss.backward()
        with torch.no_grad():
            if log_every and it % log_every == 0:
                print(f"[recon] iter {it}: loss {loss.item():.5f}, {g.xyz.shape[0]} Gaussians, {time.perf_counter() - t0:.1f} s")
            if it in save_iterations and model_path:
                g.save_ply(os.path.join(model_path, "point_cloud", f"iteration_{it}", "point_cloud.ply"))
            if it < opt.densify_until_iter:
                g.record_view(pkg["radii"], pkg["viewspace_points"].grad)
                if it > opt.densify_from_iter and it % opt.densification_interval == 0:
                    g.densify_and_prune(opt.densify_grad_threshold, 0.005, extent, 20 if it > opt.opacity_reset_interval else None)
                if it % opt.opacity_reset_interval == 0 or (white_background and it == opt.densify_from_iter):
                    g.reset_opacity()
            if it < opt.iterations:
                g.optimizer.step()
                g.optimizer.zero_grad(set_to_none=True)
    if torch.cuda.is_available() and str(device).startswith("cuda"):
        torch.cuda.synchronize()
    stats.update(seconds=time.perf_counter() - t0, num_gaussians=int(g.xyz.shape[0]))
    return g, cams, stats


def psnr(a: torch.Tensor, b: torch.Tensor) -> float:
    mse = torch.mean((a.float() - b.float()) ** 2).item()
    return float("inf") if mse == 0 else 10.0 * math.log10(1.0 / mse)


@torch.no_grad()
def render_orbit(g: GaussianModel, n: int, radius: float, elevation: float, fov: float, reso: int, white_background: bool, device="cuda"):
    """n turntable frames of the trained splats, uint8 [n, reso, reso, 3] on the host."""
    cams, _ = orbit_cameras(n, radius, elevation, fov, reso)
    bg = torch.tensor([1.0, 1.0, 1.0] if white_background else [0.0, 0.0, 0.0], device=device)
    out = []
    for c in cams:
        img = render(c, g, bg)["render"]
        out.append((img.clamp(0, 1) * 255).to(torch.uint8).permute(1, 2, 0).cpu())
    return torch.stack(out).numpy()
