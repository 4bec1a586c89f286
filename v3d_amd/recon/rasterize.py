"""Differentiable splat rasterizer over the gfx950 kernels (csrc/gs.hip), the counterpart of the reference's
recon/gaussian_renderer/__init__.py `render` + diff_gaussian_rasterization.

Forward of one view: preprocess_fwd -> scan(tiles touched) -> duplicate_keys -> radix_sort_pairs (32 + bits(tiles) key bits) -> tile_ranges
-> render_fwd.  Backward: render_bwd (per-instance gradient slots) -> reduce_instance_grads (fixed-order segmented sum) -> preprocess_bwd.
No step uses atomics, so images and gradients are bit-reproducible.  There is no fallback: without the HIP library this raises."""
from __future__ import annotations

import torch

from ..hip import GsCamera
from ..ops import get_ops
from .cameras import Camera


def gs_camera(cam: Camera, bg) -> GsCamera:
    c = GsCamera()
    wv = cam.world_view.detach().float().cpu().reshape(-1).tolist()
    fp = cam.full_proj.detach().float().cpu().reshape(-1).tolist()
    for k in range(16):
        c.view[k], c.proj[k] = wv[k], fp[k]
    c.tanfovx, c.tanfovy = cam.tanfovx, cam.tanfovy
    bgl = [float(v) for v in (bg.detach().cpu().tolist() if torch.is_tensor(bg) else bg)]
    for k in range(3):
        c.bg[k] = bgl[k]
    c.width, c.height = int(cam.width), int(cam.height)
    return c


def forward_pass(ops, xyz, scale_raw, rot_raw, opacity_raw, f_dc, gc: GsCamera):
    """All forward kernels of one view; returns the image and every intermediate the backward needs."""
    pre = ops.gs_preprocess_fwd(xyz, scale_raw, rot_raw, opacity_raw, f_dc, gc)
    offsets = ops.gs_scan(pre["tiles"])
    n_inst = int(offsets[-1].item())
    keys, vals = ops.gs_duplicate_keys(pre["means2d"], pre["radii"], pre["depth"], offsets, n_inst, gc.width, gc.height)
    ntiles = ((gc.width + 15) // 16) * ((gc.height + 15) // 16)
    nbits = 32 + max(1, (ntiles - 1).bit_length())
    keys_s, vals_s = ops.gs_radix_sort_pairs(keys, vals, nbits)
    ranges, inst_pos = ops.gs_tile_ranges(keys_s, vals_s, pre["means2d"], pre["radii"], offsets, gc.width, gc.height)
    img, final_T, n_contrib = ops.gs_render_fwd(ranges, vals_s, pre["means2d"], pre["conic_opacity"], pre["rgb"], gc)
    st = dict(pre, offsets=offsets, n_inst=n_inst, vals_s=vals_s, ranges=ranges, inst_pos=inst_pos, final_T=final_T, n_contrib=n_contrib)
    return img, st


def backward_pass(ops, xyz, scale_raw, rot_raw, opacity_raw, gc: GsCamera, st, dimg):
    inst = ops.gs_render_bwd(st["ranges"], st["vals_s"], st["means2d"], st["conic_opacity"], st["rgb"], gc, st["final_T"], st["n_contrib"],
                             dimg.contiguous())
    g9 = ops.gs_reduce_instance_grads(inst, st["offsets"], st["inst_pos"], xyz.shape[0])
    return ops.gs_preprocess_bwd(xyz, scale_raw, rot_raw, opacity_raw, gc, st["radii"], st["clamped"], g9)


class _Rasterize(torch.autograd.Function):
    @staticmethod
    def forward(ctx, xyz, scale_raw, rot_raw, opacity_raw, f_dc, means2d_holder, gc):
        ctx.empty = xyz.shape[0] == 0
        if ctx.empty:       # every Gaussian pruned: the view is the background (the kernels take P >= 1)
            ctx.save_for_backward(xyz, scale_raw, rot_raw, opacity_raw, f_dc, means2d_holder)
            img = torch.tensor(list(gc.bg), dtype=torch.float32, device=xyz.device).view(3, 1, 1).expand(3, gc.height, gc.width).contiguous()
            radii = torch.zeros(0, dtype=torch.int32, device=xyz.device)
            ctx.mark_non_differentiable(radii)
            return img, radii
        ops = get_ops()
        xyz, scale_raw, rot_raw = xyz.contiguous(), scale_raw.contiguous(), rot_raw.contiguous()
        opacity_raw, f_dc = opacity_raw.contiguous(), f_dc.contiguous()
        img, st = forward_pass(ops, xyz, scale_raw, rot_raw, opacity_raw, f_dc, gc)
        ctx.gc, ctx.st = gc, st
        ctx.fdc_shape, ctx.op_shape = f_dc.shape, opacity_raw.shape
        ctx.save_for_backward(xyz, scale_raw, rot_raw, opacity_raw)
        ctx.mark_non_differentiable(st["radii"])
        return img, st["radii"]

    @staticmethod
    def backward(ctx, dimg, _dradii):
        if ctx.empty:
            return tuple(torch.zeros_like(t) for t in ctx.saved_tensors) + (None,)
        xyz, scale_raw, rot_raw, opacity_raw = ctx.saved_tensors
        g = backward_pass(get_ops(), xyz, scale_raw, rot_raw, opacity_raw, ctx.gc, ctx.st, dimg)
        return (g["xyz"], g["scale"], g["rot"], g["opacity"].view(ctx.op_shape), g["f_dc"].view(ctx.fdc_shape), g["means2d"], None)


def rasterize(xyz, scale_raw, rot_raw, opacity_raw, f_dc, cam: Camera, bg, means2d_holder=None):
    """Image [3, H, W] and radii [P] of raw (pre-activation) parameters: xyz [P, 3], log scales [P, 3], quaternions [P, 4] (unnormalised),
    opacity logits [P, 1], SH degree-0 coefficients [P, 1, 3] (or [P, 3]).  means2d_holder [P, 2] receives dL/d(NDC mean) as its .grad."""
    if means2d_holder is None:
        means2d_holder = torch.zeros(xyz.shape[0], 2, device=xyz.device, requires_grad=True)
    return _Rasterize.apply(xyz, scale_raw, rot_raw, opacity_raw, f_dc, means2d_holder, gs_camera(cam, bg))


def render(camera: Camera, gaussians, bg):
    """The reference's render(): {"render": image, "viewspace_points": screen-space mean holder, "visibility_filter": radii > 0, "radii"}."""
    holder = torch.zeros(gaussians.xyz.shape[0], 2, device=gaussians.xyz.device, requires_grad=True)
    img, radii = rasterize(gaussians.xyz, gaussians.scaling, gaussians.rotation, gaussians.opacity, gaussians.features_dc, camera, bg, holder)
    return {"render": img, "viewspace_points": holder, "visibility_filter": radii > 0, "radii": radii}


class _SsimL1(torch.autograd.Function):
    @staticmethod
    def forward(ctx, img, gt, lambda_dssim):
        ops = get_ops()
        img, gt = img.contiguous(), gt.contiguous()
        out3, work = ops.gs_ssim_l1_fwd(img, gt, lambda_dssim)
        ctx.save_for_backward(img, gt, work)
        ctx.lam = lambda_dssim
        return out3[0], out3[1].detach(), out3[2].detach()

    @staticmethod
    def backward(ctx, dloss, _ds, _dl):
        img, gt, work = ctx.saved_tensors
        dl = dloss.reshape(1).float().contiguous()
        return get_ops().gs_ssim_l1_bwd(img, gt, ctx.lam, work, dl), None, None


def ssim_l1_loss(img, gt, lambda_dssim: float):
    """(loss, ssim, l1) with loss = (1 - lambda) L1 + lambda (1 - SSIM) on the fused HIP kernels; only loss carries a gradient."""
    return _SsimL1.apply(img, gt, float(lambda_dssim))
