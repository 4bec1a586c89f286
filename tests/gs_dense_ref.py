"""Dense fp64 restatement of the 3-D Gaussian splatting rasterizer (test oracle of csrc/gs.hip), written from the published math
(Kerbl et al. 2023): no tiles except the tile-rectangle membership rule; every pixel blends every member Gaussian in depth order with the
same thresholds; torch autograd gives the gradients.  `dtype=torch.float32` runs the same restatement in single precision: what it loses
against the fp64 run is the error the number format itself costs, the yardstick of the GPU bars.  Also the SSIM of the reference's loss
(F.conv2d, CPU) and scene helpers: random scenes, deep scenes (long tile lists, saturated pixels), cull scenes (every cull and clamp branch
of the preprocess) and a scene of equal depths."""
from __future__ import annotations

import math

import torch
import torch.nn.functional as F

SH_C0 = 0.28209479177387814
TILE = 16


def quat_to_rot(r):
    q = r / torch.sqrt((r * r).sum(1, keepdim=True))
    w, x, y, z = q.unbind(1)
    return torch.stack([1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y),
                        2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x),
                        2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)], 1).view(-1, 3, 3)


def project(xyz, scale_raw, rot_raw, opacity_raw, f_dc, world_view, full_proj, tanfovx, tanfovy, W, H, dtype=torch.float64):
    """Per-Gaussian screen quantities in `dtype` (differentiable): dict with pix [P, 2], conic [P, 3] (A, B, C), opacity, rgb, depth, radius,
    rect, and the cull inputs (txtz, tytz: view x / z and y / z, which the 1.3 tan(fov / 2) guard clamps)."""
    d = dtype
    xyz, V, Pm = xyz.to(d), world_view.to(d), full_proj.to(d)
    ph = torch.cat([xyz, torch.ones_like(xyz[:, :1])], 1)
    t = ph @ V
    hom = ph @ Pm
    pw = 1.0 / (hom[:, 3] + 1e-7)
    pix = torch.stack([((hom[:, 0] * pw + 1) * W - 1) * 0.5, ((hom[:, 1] * pw + 1) * H - 1) * 0.5], 1)
    s = torch.exp(scale_raw.to(d))
    R = quat_to_rot(rot_raw.to(d))
    Sig = R @ torch.diag_embed(s * s) @ R.transpose(1, 2)
    tx, ty, tz = t[:, 0], t[:, 1], t[:, 2]
    fx, fy = W / (2 * tanfovx), H / (2 * tanfovy)
    limx, limy = 1.3 * tanfovx, 1.3 * tanfovy
    # outside the guard the Jacobian uses the clamped position as a constant (the published backward passes no gradient through it)
    cx, cy = (tx / tz).abs() > limx, (ty / tz).abs() > limy
    txc = torch.where(cx, ((tx / tz).clamp(-limx, limx) * tz).detach(), tx)
    tyc = torch.where(cy, ((ty / tz).clamp(-limy, limy) * tz).detach(), ty)
    z0 = torch.zeros_like(tz)
    J = torch.stack([fx / tz, z0, -fx * txc / tz ** 2, z0, fy / tz, -fy * tyc / tz ** 2], 1).view(-1, 2, 3)
    Wm = V[:3, :3].transpose(0, 1)
    T = J @ Wm
    cov = T @ Sig @ T.transpose(1, 2)
    a, b, c = cov[:, 0, 0] + 0.3, cov[:, 0, 1], cov[:, 1, 1] + 0.3
    det = a * c - b * b
    conic = torch.stack([c / det, -b / det, a / det], 1)
    with torch.no_grad():
        mid = 0.5 * (a + c)
        disc = torch.sqrt(torch.clamp_min(mid * mid - det, 0.1))
        lmax = torch.maximum(mid + disc, mid - disc)
        rad = torch.ceil(3 * torch.sqrt(lmax))
        gx, gy = (W + TILE - 1) // TILE, (H + TILE - 1) // TILE
        trunc = lambda v: torch.trunc(v)  # noqa: E731  (C float -> int casts truncate toward zero)
        x0 = trunc((pix[:, 0] - rad) / TILE).clamp(0, gx)
        y0 = trunc((pix[:, 1] - rad) / TILE).clamp(0, gy)
        x1 = trunc((pix[:, 0] + rad + TILE - 1) / TILE).clamp(0, gx)
        y1 = trunc((pix[:, 1] + rad + TILE - 1) / TILE).clamp(0, gy)
        visible = (tz > 0.2) & (det != 0) & ((x1 - x0) * (y1 - y0) > 0)
    rgb_raw = 0.5 + SH_C0 * f_dc.reshape(-1, 3).to(d)
    return {"pix": pix, "conic": conic, "opacity": torch.sigmoid(opacity_raw.reshape(-1).to(d)), "rgb": torch.clamp_min(rgb_raw, 0.0),
            "depth": tz, "radius": rad, "rect": torch.stack([x0, y0, x1, y1], 1), "visible": visible, "lmax": lmax,
            "txtz": (tx / tz).detach(), "tytz": (ty / tz).detach(), "guarded": (cx | cy).detach(), "rgb_raw": rgb_raw.detach()}


def _alphas(pr, W, H):
    d = pr["pix"].dtype
    ys, xs = torch.meshgrid(torch.arange(H, dtype=d), torch.arange(W, dtype=d), indexing="ij")
    px, py = xs.reshape(-1, 1), ys.reshape(-1, 1)
    dx, dy = pr["pix"][None, :, 0] - px, pr["pix"][None, :, 1] - py
    A, B, C = pr["conic"][:, 0], pr["conic"][:, 1], pr["conic"][:, 2]
    power = -0.5 * (A * dx * dx + C * dy * dy) - B * dx * dy
    alpha = torch.clamp(pr["opacity"] * torch.exp(power), max=0.99)
    r = pr["rect"]
    tx, ty = (px // TILE), (py // TILE)
    member = pr["visible"][None] & (tx >= r[None, :, 0]) & (tx < r[None, :, 2]) & (ty >= r[None, :, 1]) & (ty < r[None, :, 3])
    valid = member & (power <= 0) & (alpha >= 1.0 / 255.0)
    return alpha, valid, member


def render(xyz, scale_raw, rot_raw, opacity_raw, f_dc, world_view, full_proj, tanfovx, tanfovy, W, H, bg, dtype=torch.float64):
    """Image [3, H, W] in `dtype` and the projection dict.  pr['pix'] carries the screen-space mean; pr['final_T'] [H, W] is every pixel's
    transmittance after its last blended Gaussian, pr['n_contrib'] [H, W] the 1-based position of that Gaussian in the depth-ordered list of
    the pixel's tile members (0: nothing blended; equal depths go by Gaussian index, what a stable sort of index-ordered input gives) and
    pr['color'] [H * W, 3] the blended colour without the background (image = color + final_T * bg)."""
    pr = project(xyz, scale_raw, rot_raw, opacity_raw, f_dc, world_view, full_proj, tanfovx, tanfovy, W, H, dtype)
    alpha, valid, member = _alphas(pr, W, H)
    order = torch.argsort(pr["depth"].detach(), stable=True)
    n = W * H
    T = torch.ones(n, dtype=dtype)
    Cacc = torch.zeros(n, 3, dtype=dtype)
    done = torch.zeros(n, dtype=torch.bool)
    pos = torch.zeros(n, dtype=torch.int32)
    last = torch.zeros(n, dtype=torch.int32)
    any_member = member.any(0)
    for k in order.tolist():
        if not bool(any_member[k]):
            continue
        pos = pos + member[:, k].to(torch.int32)
        v = valid[:, k] & ~done
        if not bool(v.any()):
            continue
        a = alpha[:, k]
        tT = T * (1 - a)
        stop = v & (tT < 1e-4)
        done = done | stop
        blend = v & ~stop
        Cacc = Cacc + torch.where(blend, a * T, torch.zeros_like(a))[:, None] * pr["rgb"][k][None]
        T = torch.where(blend, tT, T)
        last = torch.where(blend, pos, last)
    img = Cacc + T[:, None] * torch.as_tensor(bg, dtype=dtype)[None]
    pr.update(final_T=T.detach().reshape(H, W), n_contrib=last.reshape(H, W), color=Cacc.detach(), saturated=done.reshape(H, W),
              list_len=pos.reshape(H, W))
    return img.t().reshape(3, H, W), pr


@torch.no_grad()
def scene_margins(xyz, scale_raw, rot_raw, opacity_raw, f_dc, world_view, full_proj, tanfovx, tanfovy, W, H):
    """Smallest distance of the fp64 decisions of this view from their thresholds, by kind: fp32 decides the same where these are large.
    alpha: vs 1/255 and 0.99; transmittance: vs 1e-4 in log space (a relative distance); radius: 3-sigma radius vs the integer it is rounded
    up to; edges: tile-rectangle edges vs the grid line they are truncated to (pixels); depth: view z vs the 0.2 cull; guard: x / z and
    y / z vs 1.3 tan(fov / 2); colour: raw colour vs the clamp at 0; depth_gap: smallest difference of two unequal depths of visible
    Gaussians (their order in every tile list).  Culled Gaussians take part only in the decisions that culled them: depth for those at
    z <= 0.2, and for those whose rectangle is empty the radius and the edges against the grid lines that would let them in."""
    pr = project(xyz, scale_raw, rot_raw, opacity_raw, f_dc, world_view, full_proj, tanfovx, tanfovy, W, H)
    alpha, valid, member = _alphas(pr, W, H)
    m = {k: [1.0] for k in ("alpha", "transmittance", "radius", "edges", "depth", "guard", "colour", "depth_gap")}
    am = alpha[member]
    if am.numel():
        m["alpha"] += [float((am - 1 / 255).abs().min()), float((am - 0.99).abs().min())]
    m["depth"].append(float((pr["depth"] - 0.2).abs().min()))
    vis = pr["visible"]
    if vis.any():
        r3 = 3 * torch.sqrt(pr["lmax"][vis])
        m["radius"].append(float((r3 - torch.round(r3)).abs().min()))
        rad = pr["radius"][vis]
        for e in ((pr["pix"][vis, 0] - rad) / TILE, (pr["pix"][vis, 1] - rad) / TILE, (pr["pix"][vis, 0] + rad + TILE - 1) / TILE,
                  (pr["pix"][vis, 1] + rad + TILE - 1) / TILE):
            m["edges"].append(float((e - torch.round(e)).abs().min()) * TILE)
        m["guard"] += [float((pr["txtz"][vis].abs() - 1.3 * tanfovx).abs().min()), float((pr["tytz"][vis].abs() - 1.3 * tanfovy).abs().min())]
        m["colour"].append(float(pr["rgb_raw"][vis].abs().min()))
        gaps = torch.diff(torch.sort(pr["depth"][vis]).values)
        gaps = gaps[gaps > 0]        # (equal depths are equal in every precision only by construction: tie_scene; index order decides them)
        if gaps.numel():
            m["depth_gap"].append(float(gaps.min()))
    out = (pr["depth"] > 0.2) & ~vis        # in front of the camera, rectangle empty: it stays empty while no edge crosses a grid line 1 .. g
    if out.any():
        r3 = 3 * torch.sqrt(pr["lmax"][out])
        m["radius"].append(float((r3 - torch.round(r3)).abs().min()))
        rad = pr["radius"][out]
        gx, gy = (W + TILE - 1) // TILE, (H + TILE - 1) // TILE
        for e, g in (((pr["pix"][out, 0] - rad) / TILE, gx), ((pr["pix"][out, 1] - rad) / TILE, gy),
                     ((pr["pix"][out, 0] + rad + TILE - 1) / TILE, gx), ((pr["pix"][out, 1] + rad + TILE - 1) / TILE, gy)):
            lines = torch.arange(1, g + 1, dtype=e.dtype)
            m["edges"].append(float((e[:, None] - lines[None]).abs().min()) * TILE)
    order = torch.argsort(pr["depth"], stable=True)
    T = torch.ones(W * H, dtype=torch.float64)
    done = torch.zeros(W * H, dtype=torch.bool)
    for k in order.tolist():
        v = valid[:, k] & ~done
        if not bool(v.any()):
            continue
        tT = T * (1 - alpha[:, k])
        m["transmittance"].append(float((torch.log(tT[v]) - math.log(1e-4)).abs().min()))
        stop = v & (tT < 1e-4)
        done |= stop
        T = torch.where(v & ~stop, tT, T)
    return {k: min(v) for k, v in m.items()}


def scene_margin(*args):
    """Smallest of scene_margins() except the depth gap, which has a bar of its own (DEPTH_GAP_MARGIN)."""
    return min(v for k, v in scene_margins(*args).items() if k != "depth_gap")


def gaussian_window(size=11, sigma=1.5):
    """1-D window: Gaussian taps evaluated in float64, rounded to float32, normalised in float32 (the precision the published loss has)."""
    x = torch.arange(size, dtype=torch.float64) - (size - 1) / 2
    taps = torch.exp(-0.5 * (x / sigma) ** 2).float()
    return taps / taps.sum()


def ssim(img1, img2, size=11):
    """Mean SSIM of [C, H, W] images: local statistics are Gaussian-weighted means (separable 11-tap sigma-1.5 window, zero padding 5, each
    channel alone), SSIM = (2 m_a m_b + c1)(2 cov_ab + c2) / ((m_a^2 + m_b^2 + c1)(var_a + var_b + c2)), c1 = 0.01^2, c2 = 0.03^2."""
    g = gaussian_window(size).to(img1.dtype)
    k2 = torch.outer(g, g)
    chans = img1.shape[-3]
    weight = k2.expand(chans, 1, size, size)

    def local_mean(x):
        return F.conv2d(x, weight, padding=size // 2, groups=chans)

    ma, mb = local_mean(img1), local_mean(img2)
    var_a = local_mean(img1 * img1) - ma * ma
    var_b = local_mean(img2 * img2) - mb * mb
    cov = local_mean(img1 * img2) - ma * mb
    c1, c2 = 1e-4, 9e-4
    num = (2 * ma * mb + c1) * (2 * cov + c2)
    den = (ma * ma + mb * mb + c1) * (var_a + var_b + c2)
    return (num / den).mean()


# Forward-test scenes (tests/test_gs_gpu.py): seeds of random_scene(300, seed) whose fp64 decisions all lie at least SCENE_MARGIN from their
# thresholds over every view of FORWARD_VIEWS (tests/test_gs_cpu.py::test_forward_scenes_keep_their_margin holds that).
SCENE_SEEDS = (1116, 2270, 3301)
SCENE_MARGIN = 2e-7
# Two Gaussians keep their fp64 order in fp32 when their depths differ by more than both roundings: view z is a 4-term fp32 dot product of
# magnitude ~2 (ulp 2.4e-7); the float32 run of the oracle is off by at most 2.5e-7 on a visible Gaussian of the test scenes
# (tests/test_gs_cpu.py asserts it).  The bar is 4x that.
DEPTH_GAP_MARGIN = 1e-6
# A transmittance that is the product of hundreds of fp32 factors carries more than one rounding: on the edge scenes below the float32 run of
# the oracle is off by up to 7.0e-6 relative.  Their decisions against 1e-4 keep about 3x that.
DEEP_T_MARGIN = 2e-5
FORWARD_SIZES = ((64, 48), (80, 80))


def cams_for(W, H, n=4, elevation=15.0):
    """n orbit cameras at distance 2 with a 60-degree horizontal field of view on a W x H image."""
    from v3d_amd.recon.cameras import make_camera, orbit_positions
    fx = math.radians(60.0)
    fy = 2 * math.atan(math.tan(fx / 2) * H / W)
    return [make_camera(e, fx, fy, W, H) for e in orbit_positions(n, 2.0, elevation)]


def random_scene(n, seed, spread=0.35, device="cpu"):
    """Raw parameters of n Gaussians around the origin: opacities in [0.05, 0.9] (never near the 0.99 clamp), anisotropic scales."""
    g = torch.Generator().manual_seed(seed)
    xyz = torch.randn(n, 3, generator=g) * spread
    scale = torch.log(0.015 + 0.04 * torch.rand(n, 3, generator=g))
    rot = torch.randn(n, 4, generator=g)
    op = torch.logit(0.05 + 0.85 * torch.rand(n, 1, generator=g))
    fdc = torch.randn(n, 1, 3, generator=g) * 1.2
    return [t.float().to(device) for t in (xyz, scale, rot, op, fdc)]


# ---- scenes of tests/test_gs_edges_gpu.py; tests/test_gs_cpu.py holds their margins, their float32 cost and what they cover ------------
FORWARD_SIZES_RAGGED = ((56, 40), (72, 24))      # neither side a multiple of the 16-pixel tile


def deep_scene(n, seed, spread=0.15, core=48, device="cpu"):
    """A tight cloud of n opaque Gaussians (opacities in [0.3, 0.95], still away from the 0.99 clamp; scales in [0.02, 0.08]): tile lists of
    several forward batches and pixels that saturate.  The last `core` of them are large (scales in [0.35, 0.5]) and sit at the centre: every
    pixel of the tiles around the image centre saturates inside them, so the part of those tiles' lists that lies behind reaches no pixel."""
    g = torch.Generator().manual_seed(seed)
    xyz = torch.randn(n, 3, generator=g) * spread
    scale = torch.log(0.02 + 0.06 * torch.rand(n, 3, generator=g))
    rot = torch.randn(n, 4, generator=g)
    op = torch.logit(0.3 + 0.65 * torch.rand(n, 1, generator=g))
    fdc = torch.randn(n, 1, 3, generator=g) * 1.2
    if core:
        xyz[n - core:] *= 0.25
        scale[n - core:] = torch.log(0.35 + 0.15 * torch.rand(core, 3, generator=g))
        op[n - core:] = torch.logit(0.8 + 0.15 * torch.rand(core, 1, generator=g))
    return [t.float().to(device) for t in (xyz, scale, rot, op, fdc)]


CULL_GROUPS = ("base", "behind", "near", "far_out", "guard", "huge", "dark")


def cull_scene(n, seed, cam, device="cpu"):
    """A base cloud of n Gaussians plus groups placed in the view space of `cam` for one branch of the preprocess each: `behind` the camera
    and `near` (0 < z < 0.2) are culled by depth; `far_out` lies far outside the frustum with a rectangle that misses every tile; `guard`
    lies outside the frustum past the 1.3 tan(fov / 2) guard, large enough to reach the image (the clamped Jacobian, forward and backward);
    `huge` covers the image, its rectangle clamped on all four sides; `dark` has every colour channel clamped at 0.
    Returns (scene, groups: name -> index tensor)."""
    g = torch.Generator().manual_seed(seed)
    tx_, ty_ = cam.tanfovx, cam.tanfovy
    rand = lambda k, lo, hi: lo + (hi - lo) * torch.rand(k, generator=g, dtype=torch.float64)  # noqa: E731
    sign = lambda k: torch.where(torch.rand(k, generator=g) < 0.5, -1.0, 1.0).double()  # noqa: E731
    view, scales, ops, dcs, groups = [], [], [], [], {}

    def add(name, z, xz, yz, sc_lo, sc_hi, op_lo=0.05, op_hi=0.9, dc=None):
        k = z.numel()
        start = sum(v.shape[0] for v in view)
        view.append(torch.stack([xz * z, yz * z, z], 1))
        scales.append(torch.log(sc_lo + (sc_hi - sc_lo) * torch.rand(k, 3, generator=g, dtype=torch.float64)))
        ops.append(torch.logit(op_lo + (op_hi - op_lo) * torch.rand(k, 1, generator=g, dtype=torch.float64)))
        dcs.append(torch.randn(k, 1, 3, generator=g, dtype=torch.float64) * 1.2 if dc is None else dc)
        groups[name] = torch.arange(start, start + k)

    base = torch.randn(n, 3, generator=g, dtype=torch.float64) * 0.35
    add("base", 2.0 + base[:, 2], base[:, 0] / (2.0 + base[:, 2]), base[:, 1] / (2.0 + base[:, 2]), 0.015, 0.055)
    add("behind", -rand(12, 0.3, 3.0), rand(12, -0.3, 0.3), rand(12, -0.3, 0.3), 0.02, 0.06)
    add("near", rand(12, 0.02, 0.18), rand(12, -0.4, 0.4) * tx_, rand(12, -0.4, 0.4) * ty_, 0.005, 0.02)
    add("far_out", rand(12, 1.5, 2.5), sign(12) * rand(12, 3.0, 4.0) * tx_, sign(12) * rand(12, 3.0, 4.0) * ty_, 0.015, 0.04)
    # past the guard on x (first half) or on y (second half), inside the frustum on the other axis
    gx_ = torch.cat([sign(6) * rand(6, 1.32, 1.45) * tx_, rand(6, -0.6, 0.6) * tx_])
    gy_ = torch.cat([rand(6, -0.6, 0.6) * ty_, sign(6) * rand(6, 1.32, 1.45) * ty_])
    add("guard", rand(12, 1.8, 2.2), gx_, gy_, 0.2, 0.3, 0.3, 0.9)
    add("huge", rand(3, 1.9, 2.1), rand(3, -0.1, 0.1) * tx_, rand(3, -0.1, 0.1) * ty_, 0.8, 1.2, 0.05, 0.15)
    add("dark", rand(12, 1.7, 2.0), rand(12, -0.5, 0.5) * tx_, rand(12, -0.5, 0.5) * ty_, 0.03, 0.06, 0.3, 0.9,
        dc=-rand(36, 2.5, 4.0).view(12, 1, 3))
    pv = torch.cat(view)
    xyz = (torch.cat([pv, torch.ones_like(pv[:, :1])], 1) @ torch.linalg.inv(cam.world_view.double()))[:, :3]
    rot = torch.randn(xyz.shape[0], 4, generator=g)
    scene = [t.float().to(device) for t in (xyz, torch.cat(scales), rot, torch.cat(ops), torch.cat(dcs))]
    return scene, groups


def axis_camera(W, H):
    """A camera on the +x axis at distance 2 looking at the origin: its view matrix holds only 0, +-1 and 2, so view depth = 2 - x exactly
    and Gaussians that share x share their depth bit for bit in every precision."""
    import numpy as np

    from v3d_amd.recon.cameras import make_camera
    fx = math.radians(60.0)
    fy = 2 * math.atan(math.tan(fx / 2) * H / W)
    return make_camera(np.array([2.0, 0.0, 0.0]), fx, fy, W, H)


def tie_scene(device="cpu"):
    """Three groups of three overlapping, fairly opaque Gaussians with distinct saturated colours; the members of a group share their world x,
    hence their depth under axis_camera, so only the stable sort's index order decides which is in front.  Returns (scene, groups)."""
    xs = (0.25, 0.0, -0.375)
    centres = ((-0.45, 0.2), (0.0, 0.0), (0.45, -0.25))      # (world y, z): the groups overlap in part and together reach the image edges
    xyz, dc = [], []
    cols = ((3.0, -1.5, -1.5), (-1.5, 3.0, -1.5), (-1.5, -1.5, 3.0))
    for gi, (x, (cy, cz)) in enumerate(zip(xs, centres)):
        for k in range(3):
            xyz.append((x, cy + 0.08 * (k - 1), cz + 0.06 * (1 - k) * (-1) ** gi))
            dc.append(cols[(k + gi) % 3])
    n = len(xyz)
    xyz = torch.tensor(xyz)
    scale = torch.log(torch.tensor([[0.15, 0.27, 0.2], [0.24, 0.18, 0.3], [0.2, 0.3, 0.17]]).repeat(3, 1))
    rot = torch.tensor([[1.0, 0.1 * k, -0.05 * k, 0.02 * k] for k in range(n)])
    op = torch.logit(torch.tensor([0.8, 0.7, 0.9, 0.75, 0.85, 0.65, 0.9, 0.8, 0.7]).view(n, 1))
    fdc = torch.tensor(dc).view(n, 1, 3)
    groups = [torch.arange(3 * gi, 3 * gi + 3) for gi in range(3)]
    return [t.float().to(device) for t in (xyz, scale, rot, op, fdc)], groups


def swap_rows(scene, i, j):
    """The scene with Gaussians i and j exchanged (same set of Gaussians, different index order)."""
    perm = torch.arange(scene[0].shape[0])
    perm[i], perm[j] = j, i
    return [t[perm].clone() for t in scene]


# Seeds searched like SCENE_SEEDS: every fp64 decision of each case below lies at least SCENE_MARGIN from its threshold
# (tests/test_gs_cpu.py::test_edge_scenes_keep_their_margin).  (kind, seed, W, H, view of cams_for, white background in the backward)
DEEP_SEEDS = (73, 87, 262)
CULL_SEEDS = (3, 8, 11)
EDGE_CASES = (("deep", 73, 56, 40, 2, True), ("deep", 87, 72, 24, 1, False), ("deep", 262, 64, 48, 3, True),
              ("cull", 3, 56, 40, 0, False), ("cull", 8, 72, 24, 1, True), ("cull", 11, 64, 64, 2, False),
              ("tie", 0, 56, 40, 0, True), ("tie", 0, 72, 24, 0, False))
GRAD_NAMES = ("xyz", "scale", "rot", "opacity", "f_dc", "means2d")


def case_id(case):
    kind, seed, W, H, view, _ = case
    return f"{kind}{seed}-{W}x{H}-v{view}"


def edge_case(case):
    """(scene, camera, groups or None) of one entry of EDGE_CASES."""
    kind, seed, W, H, view, _ = case
    if kind == "deep":
        return deep_scene(1200, seed), cams_for(W, H)[view], None
    if kind == "cull":
        cam = cams_for(W, H)[view]
        scene, groups = cull_scene(300, seed, cam)
        return scene, cam, groups
    scene, groups = tie_scene()
    return scene, axis_camera(W, H), groups


def image_weight(case):
    """The random image weight of the backward tests: loss = sum(image * weight)."""
    _, seed, W, H, view, _ = case
    return torch.randn(3, H, W, generator=torch.Generator().manual_seed(1000 * seed + 10 * W + view + 1), dtype=torch.float64)


def oracle_run(scene, cam, W, H, bg, wgt, dtype=torch.float64):
    """One forward and backward of the dense oracle in `dtype`: (image, projection dict, gradients by GRAD_NAMES).  The screen-space mean
    gradient is dL/d(NDC mean) = dL/d(pixel mean) * (W / 2, H / 2), what the rasterizer hands to densification."""
    with torch.enable_grad():
        params = [t.detach().to(dtype).clone().requires_grad_(True) for t in scene]
        img, pr = render(*params, cam.world_view, cam.full_proj, cam.tanfovx, cam.tanfovy, W, H, bg, dtype)
        pr["pix"].retain_grad()
        (img * wgt.to(dtype)).sum().backward()
    grads = {n: p.grad.detach() for n, p in zip(GRAD_NAMES, params)}
    grads["means2d"] = pr["pix"].grad.detach() * torch.tensor([W / 2, H / 2], dtype=dtype)
    pr = {k: v.detach() for k, v in pr.items()}
    return img.detach(), pr, grads


class EdgeOracles:
    """case of EDGE_CASES -> the scene, its camera and one fp64 and one float32 run of the dense oracle (forward and backward), computed on
    first use and kept: a module-scoped fixture shares them between the forward and the backward tests."""

    def __init__(self):
        self.cache = {}

    def __call__(self, case):
        if case not in self.cache:
            _, _, W, H, _, white = case
            scene, cam, groups = edge_case(case)
            bg, wgt = ([1.0, 1.0, 1.0] if white else [0.0, 0.0, 0.0]), image_weight(case)
            self.cache[case] = dict(scene=scene, cam=cam, groups=groups, bg=bg, wgt=wgt, o64=oracle_run(scene, cam, W, H, bg, wgt),
                                    o32=oracle_run(scene, cam, W, H, bg, wgt, torch.float32))
        return self.cache[case]


def rel_l2(a, b):
    return ((a.double() - b.double()).norm() / b.double().norm().clamp_min(1e-30)).item()


def per_gaussian_error(got, ref, floor=1e-3):
    """Largest relative error of a single Gaussian's gradient row, |got_i - ref_i| / |ref_i|, over the Gaussians whose reference row is
    larger than `floor` times the largest row: a norm over all Gaussians hides a wrong gradient on a few small contributors."""
    got, ref = got.double().reshape(ref.shape[0], -1), ref.double().reshape(ref.shape[0], -1)
    rn = ref.norm(dim=1)
    sel = rn > floor * rn.max()
    return float(((got - ref).norm(dim=1)[sel] / rn[sel]).max()), int(sel.sum())
