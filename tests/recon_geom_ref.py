"""Pure-torch restatement of csrc_recon/geom.hip (test oracle): per-pixel expected depth and accumulated alpha on top of the dense splat
oracle (gs_dense_ref.project / _alphas), TSDF integration of one view, and naive surface nets.  fp64 by default; `dtype=torch.float32` runs
the same statements in single precision (what that run loses against the fp64 one is the cost of the number format).  Also the decision
margins of the TSDF pass, the analytic sphere views and the scenes of tests/test_recon_geom_{cpu,gpu}.py."""
from __future__ import annotations

import numpy as np
import torch

import gs_dense_ref as D

# ---- depth / alpha ------------------------------------------------------------------------------------------------------------------


@torch.no_grad()
def depth_alpha(scene, cam, W, H, dtype=torch.float64):
    """dict(depth [H, W] = sum alpha_i T_i z_i, alpha [H, W] = 1 - final T, final_T, n_contrib, color [H * W, 3] without background, zmax =
    largest view z of a Gaussian that contributes to a pixel).  Every pixel blends its tile members in depth order (stable, by index among
    equal depths) with the rasterizer's rules: power <= 0, alpha = min(0.99, o exp(power)) >= 1/255, stop before T would fall below 1e-4."""
    pr = D.project(*scene, cam.world_view, cam.full_proj, cam.tanfovx, cam.tanfovy, W, H, dtype)
    alpha, valid, member = D._alphas(pr, W, H)
    order = torch.argsort(pr["depth"], stable=True)
    a = torch.where(valid, alpha, torch.zeros_like(alpha))[:, order]
    valid, member = valid[:, order], member[:, order]
    z, rgb = pr["depth"][order], pr["rgb"][order]
    cp = torch.cumprod(1 - a, dim=1)                              # transmittance after each list entry, were nothing to stop the pixel
    done = torch.cumsum((valid & (cp < 1e-4)).to(torch.int32), dim=1) > 0
    blend = valid & ~done
    t_before = torch.cat([torch.ones_like(cp[:, :1]), cp[:, :-1]], dim=1)
    wgt = torch.where(blend, a * t_before, torch.zeros_like(a))
    final_T = torch.cumprod(torch.where(blend, 1 - a, torch.ones_like(a)), dim=1)[:, -1]
    pos = torch.cumsum(member.to(torch.int32), dim=1)
    n_contrib = torch.where(blend, pos, torch.zeros_like(pos)).max(dim=1).values
    used = blend.any(0)
    return dict(depth=(wgt * z[None]).sum(1).reshape(H, W), alpha=(1 - final_T).reshape(H, W), final_T=final_T.reshape(H, W),
                n_contrib=n_contrib.reshape(H, W), color=wgt @ rgb, zmax=float(z[used].max()) if bool(used.any()) else 0.0)


def image_of(da, bg, W, H):
    """[3, H, W] colour image of a depth_alpha() result over background bg"""
    img = da["color"] + da["final_T"].reshape(-1, 1) * torch.as_tensor(bg, dtype=da["color"].dtype)[None]
    return img.t().reshape(3, H, W)


# ---- TSDF ---------------------------------------------------------------------------------------------------------------------------
ALPHA_MIN = 0.5


def voxel_centres(N, bound, dtype=torch.float64):
    """[N^3, 3] centres in linear voxel order (iz N + iy) N + ix"""
    c = (torch.arange(N, dtype=dtype) + 0.5) * (2.0 * bound / N) - bound
    zz, yy, xx = torch.meshgrid(c, c, c, indexing="ij")
    return torch.stack([xx, yy, zz], -1).reshape(-1, 3)


def new_volume(N, bound, trunc=None, dtype=torch.float64):
    z = lambda *s: torch.zeros(*s, dtype=dtype)  # noqa: E731
    return dict(N=N, bound=float(bound), trunc=4.0 * 2.0 * bound / N if trunc is None else float(trunc), tsdf_sum=z(N ** 3), weight=z(N ** 3),
                rgb_sum=z(3, N ** 3), rgb_weight=z(N ** 3))


@torch.no_grad()
def tsdf_view(vol, depth, alpha, image, cam, alpha_min=ALPHA_MIN):
    """One view into `vol` in place, the statements of tsdf_integrate_kernel in the volume's dtype.  Returns the fp-sensitive quantities of
    this view for tsdf_margins(): seen, frac (distance of the continuous pixel coordinate from the nearest rounding boundary, pixels; the
    image border is one of them), alpha at the pixel, sdf."""
    d = vol["tsdf_sum"].dtype
    N, trunc = vol["N"], vol["trunc"]
    W, H = cam.width, cam.height
    p = voxel_centres(N, vol["bound"], d)
    ph = torch.cat([p, torch.ones_like(p[:, :1])], 1)
    zv = (ph @ cam.world_view.to(d))[:, 2]
    hom = ph @ cam.full_proj.to(d)
    pw = 1.0 / (hom[:, 3] + 1e-7)
    fx, fy = ((hom[:, 0] * pw + 1) * W - 1) * 0.5, ((hom[:, 1] * pw + 1) * H - 1) * 0.5
    rx, ry = torch.floor(fx + 0.5), torch.floor(fy + 0.5)
    seen = (zv > 0.2) & (rx >= 0) & (rx < W) & (ry >= 0) & (ry < H)
    pix = (ry.clamp(0, H - 1) * W + rx.clamp(0, W - 1)).long()
    a = alpha.to(d).reshape(-1)[pix]
    dm = depth.to(d).reshape(-1)[pix]
    empty = seen & ((a < alpha_min) | ~(a > 0))
    sdf = dm / a.clamp_min(1e-30) - zv
    surf = seen & ~empty & (sdf >= -trunc)
    one = torch.ones_like(zv)
    vol["tsdf_sum"] += torch.where(empty, one, torch.zeros_like(one)) + torch.where(surf, torch.clamp(sdf / trunc, max=1.0), torch.zeros_like(one))
    vol["weight"] += (empty | surf).to(d)
    col = surf & (sdf.abs() <= trunc)
    vol["rgb_sum"] += torch.where(col[None], image.to(d).reshape(3, -1)[:, pix], torch.zeros(3, 1, dtype=d))
    vol["rgb_weight"] += col.to(d)
    fxy = torch.stack([fx + 0.5, fy + 0.5], 1)
    frac = (fxy - torch.round(fxy)).abs().min(1).values
    return dict(front=zv > 0.2, zdist=(zv - 0.2).abs(), seen=seen, frac=frac, alpha=a, sdf=sdf, empty=empty)


# fp32 against fp64 in tsdf_integrate_kernel.  A voxel's continuous pixel coordinate is W / 2 times a quotient of two 4-term dot products of
# magnitude <= 4: each carries at most 4 roundings of 2^-24 relative to ~4, the quotient and the affine map three more; at W = 32 that is below
# 16 * 12 * 6e-8 * 4 = 5e-5 pixels.  PIXEL_MARGIN is 4x that (2x at W = 56, the widest of TSDF_CASES; tests/test_recon_geom_cpu.py holds
# that the float32 run decides every voxel outside the margins as the fp64 run does, case by case).  View z and depth / alpha (values ~2, ulp 2.4e-7) carry at most 6 roundings between
# them: 1.5e-6; SDF_MARGIN (on |sdf| against trunc and on z against 0.2) is ~7x that.  alpha is read, not computed: any distance from alpha_min
# that fp32 can represent decides the same, the margin only keeps the test scenes from sitting on the threshold.  A mean TSDF is a sum of at
# most 8 terms of size <= 1 divided by a small integer, each term off by SDF_MARGIN / trunc at most: SIGN_MARGIN bounds that for trunc >= 0.1.
PIXEL_MARGIN = 2e-4
SDF_MARGIN = 1e-5
ALPHA_MARGIN = 1e-6
SIGN_MARGIN = 1e-4
MAX_EXCLUDED = 0.01


def tsdf_margins(views, trunc, alpha_min=ALPHA_MIN):
    """Boolean [N^3]: voxels some view decides within a margin of a threshold (`views`: what tsdf_view returned, per view)."""
    near = torch.zeros_like(views[0]["seen"])
    for v in views:
        near |= v["zdist"] < SDF_MARGIN
        near |= v["front"] & (v["frac"] < PIXEL_MARGIN)
        s = v["seen"]
        near |= s & ((v["alpha"] - alpha_min).abs() < ALPHA_MARGIN)
        near |= s & ~v["empty"] & (((v["sdf"].abs() - trunc).abs() < SDF_MARGIN))
    return near


# ---- analytic sphere views ----------------------------------------------------------------------------------------------------------
def sphere_view(cam, radius, dist=2.0):
    """Closed-form float32 maps of a sphere of `radius` at the origin seen by an orbit camera at distance `dist`: alpha [H, W] falls smoothly
    from 0.95 at the centre of the disc to 0 at its rim, depth [H, W] = alpha * (view z of the ray's first hit), image [3, H, W] a smooth
    colour of the pixel position."""
    W, H = cam.width, cam.height
    ys, xs = torch.meshgrid(torch.arange(H, dtype=torch.float64), torch.arange(W, dtype=torch.float64), indexing="ij")
    dx, dy = ((2 * xs + 1) / W - 1) * cam.tanfovx, ((2 * ys + 1) / H - 1) * cam.tanfovy
    dd = dx * dx + dy * dy + 1
    disc = dist * dist - dd * (dist * dist - radius * radius)
    hit = disc > 0
    t = (dist - torch.sqrt(disc.clamp_min(0))) / dd
    rho2 = 1 - disc.clamp_min(0) / (radius * radius)              # 0 at the centre of the disc, 1 at its rim
    alpha = torch.where(hit, 0.95 * (1 - rho2 ** 4), torch.zeros_like(t))
    image = torch.stack([0.5 + 0.4 * torch.sin(xs / 5), 0.5 + 0.4 * torch.cos(ys / 7), 0.3 + 0.02 * (xs + ys) / 2])
    return (alpha * t).float(), alpha.float(), image.float()


# ---- surface nets -------------------------------------------------------------------------------------------------------------------
@torch.no_grad()
def extract(vol):
    """(verts [V, 3], faces [F, 3] int64, colors [V, 3], cell_flags [(N-1)^3] bool, mean [N^3]) by the statements of the extraction kernels:
    vertices in linear cell order, faces in linear edge order (axis N^3 + voxel)."""
    N, bound = vol["N"], vol["bound"]
    d = vol["tsdf_sum"].dtype
    M = N - 1
    w = vol["weight"].reshape(N, N, N)
    mean = torch.where(w > 0, vol["tsdf_sum"].reshape(N, N, N) / w.clamp_min(1e-30), torch.ones_like(w))
    neg = (w > 0) & (mean < 0)
    corner = lambda t, k: t[(k >> 2) & 1:M + ((k >> 2) & 1), (k >> 1) & 1:M + ((k >> 1) & 1), (k & 1):M + (k & 1)]  # noqa: E731  ([z, y, x])
    seen_all = torch.stack([corner(w, k) > 0 for k in range(8)]).all(0)
    nneg = torch.stack([corner(neg, k) for k in range(8)]).sum(0)
    flags = seen_all & (nneg > 0) & (nneg < 8)
    offs = torch.cumsum(flags.reshape(-1).long(), 0) - flags.reshape(-1).long()
    psum = torch.zeros(M, M, M, 3, dtype=d)
    ncross = torch.zeros(M, M, M, dtype=d)
    for axis in range(3):
        for k in range(8):
            if k & (1 << axis):
                continue
            m0, m1 = corner(mean, k), corner(mean, k | (1 << axis))
            cross = (m0 < 0) != (m1 < 0)
            s = m0 / torch.where(cross, m0 - m1, torch.ones_like(m0))
            pos = torch.stack([s if dd == axis else torch.full_like(s, float((k >> dd) & 1)) for dd in range(3)], -1)
            psum += torch.where(cross[..., None], pos, torch.zeros_like(pos))
            ncross += cross.to(d)
    voxel = 2.0 * bound / N
    c = (torch.arange(M, dtype=d) + 0.5) * voxel - bound
    zz, yy, xx = torch.meshgrid(c, c, c, indexing="ij")
    base = torch.stack([xx, yy, zz], -1)
    verts = (base + psum / ncross.clamp_min(1)[..., None] * voxel)[flags]
    rw = vol["rgb_weight"].reshape(N, N, N)
    rgb = vol["rgb_sum"].reshape(3, N, N, N) / rw.clamp_min(1e-30)[None]
    csum = torch.zeros(3, M, M, M, dtype=d)
    ncol = torch.zeros(M, M, M, dtype=d)
    for k in range(8):
        has = corner(rw, k) > 0
        csum += torch.where(has[None], torch.stack([corner(rgb[ch], k) for ch in range(3)]), torch.zeros(1, dtype=d))
        ncol += has.to(d)
    colors = torch.where(ncol[None] > 0, csum / ncol.clamp_min(1)[None], torch.full_like(csum, 0.5)).permute(1, 2, 3, 0)[flags]
    faces = []
    fl = flags.reshape(-1)
    idx = torch.arange(N, dtype=torch.long)
    iz, iy, ix = torch.meshgrid(idx, idx, idx, indexing="ij")
    ijk = [ix.reshape(-1), iy.reshape(-1), iz.reshape(-1)]
    negl = neg.reshape(-1)
    stride = (1, N, N * N)
    for axis in range(3):
        u, wax = (axis + 1) % 3, (axis + 2) % 3
        ok = (ijk[axis] < M) & (ijk[u] >= 1) & (ijk[u] < M) & (ijk[wax] >= 1) & (ijk[wax] < M)
        v = torch.nonzero(ok).reshape(-1)
        cells = []
        for du, dw in ((-1, -1), (0, -1), (0, 0), (-1, 0)):
            cc = [None, None, None]
            cc[axis], cc[u], cc[wax] = ijk[axis][v], ijk[u][v] + du, ijk[wax][v] + dw
            cells.append((cc[2] * M + cc[1]) * M + cc[0])
        act = fl[cells[0]] & fl[cells[1]] & fl[cells[2]] & fl[cells[3]] & (negl[v] != negl[v + stride[axis]])
        v, cells = v[act], [cq[act] for cq in cells]
        a, b, c4, d4 = (offs[cq] for cq in cells)
        up = negl[v]
        t1 = torch.stack([a, torch.where(up, b, c4), torch.where(up, c4, b)], 1)
        t2 = torch.stack([a, torch.where(up, c4, d4), torch.where(up, d4, c4)], 1)
        faces.append(torch.stack([t1, t2], 1).reshape(-1, 3))
    return verts, torch.cat(faces), colors, fl, mean.reshape(-1)


def sphere_volume(N, bound, radius, dtype=torch.float32):
    """A volume holding the exact signed distance to a sphere (in units of trunc, clamped at +-1; negative inside), weight 1 everywhere, and a
    colour that varies over space with colour weight 1."""
    vol = new_volume(N, bound, dtype=dtype)
    p = voxel_centres(N, bound)
    vol["tsdf_sum"] = ((p.norm(dim=1) - radius) / vol["trunc"]).clamp(-1, 1).to(dtype)
    vol["weight"] = torch.ones(N ** 3, dtype=dtype)
    vol["rgb_sum"] = (0.5 + 0.5 * p.t() / bound).clamp(0, 1).to(dtype).contiguous()
    vol["rgb_weight"] = torch.ones(N ** 3, dtype=dtype)
    return vol


def random_volume(N, seed, p_unseen=0.03, bound=1.0):
    """A float32 volume of independent voxels: weight an integer in 1 .. 4, 0 (unobserved) with probability p_unseen; mean TSDF uniform in
    -1 .. 1; colour weight an integer in 0 .. 2, 0 on the block [: N // 2, : N // 2, :]; mean colour uniform in 0 .. 1.  Its cells take
    nearly every configuration of corner signs, some have an unobserved corner, some no coloured corner."""
    g = torch.Generator().manual_seed(seed)
    vol = new_volume(N, bound, dtype=torch.float32)
    w = torch.randint(1, 5, (N ** 3,), generator=g).float()
    w[torch.rand(N ** 3, generator=g) < p_unseen] = 0
    vol["weight"] = w
    vol["tsdf_sum"] = (torch.rand(N ** 3, generator=g) * 2 - 1) * w
    rw = torch.randint(0, 3, (N, N, N), generator=g).float()
    rw[:N // 2, :N // 2, :] = 0
    vol["rgb_weight"] = rw.reshape(-1)
    vol["rgb_sum"] = torch.rand(3, N ** 3, generator=g) * vol["rgb_weight"]
    return vol


def plane_volume(N, normal, offset, bound=1.0):
    """A float32 volume holding the signed distance to the plane normal . p = offset (normal normalised; in units of trunc, clamped at +-1;
    negative below the plane), weight and colour weight 1 everywhere, coloured by position."""
    vol = new_volume(N, bound, dtype=torch.float32)
    p = voxel_centres(N, bound)
    n = torch.tensor(normal, dtype=torch.float64)
    vol["tsdf_sum"] = ((p @ (n / n.norm()) - offset) / vol["trunc"]).clamp(-1, 1).float()
    vol["weight"] = torch.ones(N ** 3)
    vol["rgb_sum"] = (0.5 + 0.5 * p.t() / bound).clamp(0, 1).float().contiguous()
    vol["rgb_weight"] = torch.ones(N ** 3)
    return vol


# The volumes of the surface-nets tests beside the sphere: name -> builder.  tests/test_recon_geom_cpu.py states what each one covers.
MESH_VOLUMES = {
    "random13": lambda: random_volume(13, 2),          # 13^3, 12^3 and 3 * 13^3 all end in a partial block of 256
    "random11": lambda: random_volume(11, 1),
    "random6": lambda: random_volume(6, 3),
    "random3": lambda: random_volume(3, 5),
    "random2": lambda: random_volume(2, 4),            # one cell
    "plane-oblique": lambda: plane_volume(13, (0.3, 0.5, 0.81), 0.05),
    "plane-x": lambda: plane_volume(12, (1, 0, 0), 0.0),
    "plane-z-zero": lambda: plane_volume(13, (0, 0, 1), 0.0),      # a layer of voxels whose mean is exactly 0, above the negative side
    "plane-z-zero-down": lambda: plane_volume(13, (0, 0, -1), 0.0),    # ... and below it
}


def promoted(vol):
    """The same volume with its tensors in fp64"""
    return {k: (v.double() if torch.is_tensor(v) else v) for k, v in vol.items()}


def cell_stats(vol):
    """Of a volume's (N-1)^3 cells: `configurations`, the distinct mixed corner-sign patterns (8 bits, neither 0 nor 255) among the cells with all
    corners observed, and `refused_unseen`, the number of cells with an unobserved corner whose observed corners change sign."""
    N = vol["N"]
    M = N - 1
    w = vol["weight"].reshape(N, N, N)
    neg = (w > 0) & (vol["tsdf_sum"].reshape(N, N, N) < 0)        # the sign of a mean is the sign of its numerator
    corner = lambda t, k: t[(k >> 2) & 1:M + ((k >> 2) & 1), (k >> 1) & 1:M + ((k >> 1) & 1), (k & 1):M + (k & 1)]  # noqa: E731
    seen = torch.stack([corner(w, k) > 0 for k in range(8)])
    negs = torch.stack([corner(neg, k) for k in range(8)])
    code = sum(negs[k].long() << k for k in range(8))
    mixed = seen.all(0) & (code > 0) & (code < 255)
    pos = (seen & ~negs).any(0)
    return dict(configurations=int(torch.unique(code[mixed]).numel()), refused_unseen=int((~seen.all(0) & negs.any(0) & pos).sum()))


# ---- mesh measures ------------------------------------------------------------------------------------------------------------------
def edge_table(faces):
    """directed edges [3F, 2] of a triangle list (numpy int64)"""
    f = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    return np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]])


def undirected_counts(faces):
    """(unique undirected edges [E, 2], number of triangles on each, sum of directions on each: 0 when the two triangles run it opposite ways)"""
    e = edge_table(faces)
    lo, hi = e.min(1), e.max(1)
    sign = np.where(e[:, 0] < e[:, 1], 1, -1)
    und, inv, cnt = np.unique(np.stack([lo, hi], 1), axis=0, return_inverse=True, return_counts=True)
    return und, cnt, np.bincount(inv.reshape(-1), weights=sign, minlength=und.shape[0])


def signed_volume(verts, faces):
    v, f = np.asarray(verts, dtype=np.float64), np.asarray(faces, dtype=np.int64)
    return float(np.einsum("ij,ij->i", v[f[:, 0]], np.cross(v[f[:, 1]], v[f[:, 2]])).sum() / 6.0)


def chamfer(a, b):
    """Symmetric Chamfer distance of two point sets: mean nearest-neighbour distance a -> b plus b -> a, halved."""
    a, b = torch.as_tensor(np.asarray(a), dtype=torch.float64), torch.as_tensor(np.asarray(b), dtype=torch.float64)
    dm = torch.cdist(a, b)
    return 0.5 * float(dm.min(1).values.mean() + dm.min(0).values.mean())


# Symmetric Chamfer distance between the vertex sets of the end-to-end scene below, float32 run of this restatement against its fp64 run,
# measured on the CPU (e2e_restatement(torch.float32) vs e2e_restatement()): 3.21e-8 at 2694 vertices each.  It is what the number format
# costs; the kernels are granted 4x that (tests/test_recon_geom_gpu.py).
E2E_CHAMFER_FP32 = 3.21e-8
# The same measure for the ragged end-to-end case E2E_RAGGED below (72 x 40 views, a 30^3 volume whose last block of voxels is partial), again
# from the restatement alone on the CPU, with tests/ and the repository root on sys.path:
#   python -c "import torch, recon_geom_ref as R; a = R.e2e_restatement(torch.float32, **R.E2E_RAGGED); b = R.e2e_restatement(**R.E2E_RAGGED);
#   print(a[0].shape, a[1].shape, b[0].shape, b[1].shape, R.chamfer(a[0], b[0]))"
# 2.21e-6 at 2293 vertices and 4472 triangles on both sides, the same faces.  (70x the square case's: the median vertex moves by 5e-8 as there,
# but 65 move by more than 1e-6, up to 5e-4: a few voxel-views that float32 decides the other way, without a change of sign.  N and the scene
# seed are the first ones tried.)
E2E_CHAMFER_FP32_RAGGED = 2.21e-6


# ---- the end-to-end scene -----------------------------------------------------------------------------------------------------------
E2E = dict(n=3000, radius=0.5, views=8, size=64, N=32, seed=5)


def shell_scene(n=E2E["n"], radius=E2E["radius"], seed=E2E["seed"]):
    """Raw parameters of n small, nearly opaque Gaussians on a sphere of `radius` (opacity 0.9 .. 0.97, scales 0.02 .. 0.03: they overlap, the shell is
    closed), coloured by position."""
    g = torch.Generator().manual_seed(seed)
    p = torch.randn(n, 3, generator=g, dtype=torch.float64)
    p = radius * p / p.norm(dim=1, keepdim=True)
    scale = torch.log(0.02 + 0.01 * torch.rand(n, 3, generator=g, dtype=torch.float64))
    rot = torch.randn(n, 4, generator=g)
    op = torch.logit(0.9 + 0.07 * torch.rand(n, 1, generator=g, dtype=torch.float64))
    fdc = ((0.5 + p / (2 * radius)) - 0.5) / D.SH_C0
    return [t.float() for t in (p, scale, rot, op, fdc.view(n, 1, 3))]


E2E_RAGGED = dict(W=72, H=40, N=30)      # 30^3 = 105 * 256 + 120


def e2e_cameras(W=None, H=None):
    return D.cams_for(E2E["size"] if W is None else W, E2E["size"] if H is None else H, n=E2E["views"], elevation=20.0)


E2E_BOUND = 0.75        # fixed for both sides of the comparison (fuse_tsdf's default would come from fp32 positions)


def cam_to(cam, device):
    import dataclasses
    return dataclasses.replace(cam, world_view=cam.world_view.to(device), full_proj=cam.full_proj.to(device), center=cam.center.to(device))


def e2e_restatement(dtype=torch.float64, bg=(1.0, 1.0, 1.0), device="cpu", W=None, H=None, N=None):
    """The end-to-end scene through the restatement alone, every step in `dtype`: vertices [V, 3], faces, colours (on the CPU).  `device`: where
    the torch statements run (the restatement creates its tensors on torch's default device, set here).  W x H views (E2E["size"] squared by
    default) into an N^3 volume (E2E["N"])."""
    W, H = E2E["size"] if W is None else W, E2E["size"] if H is None else H
    scene = [t.to(device) for t in shell_scene()]
    with torch.device(device):
        vol = new_volume(E2E["N"] if N is None else N, E2E_BOUND, dtype=dtype)
        for cam in e2e_cameras(W, H):
            cam = cam_to(cam, device)
            da = depth_alpha(scene, cam, W, H, dtype)
            tsdf_view(vol, da["depth"], da["alpha"], image_of(da, bg, W, H), cam)
        return tuple(t.cpu() for t in extract(vol)[:3])


def sphere_tsdf_case(N=24, size=32, views=4, radius=0.5, bound=1.0, W=None, H=None, elevation=15.0, trunc=None, alpha_min=ALPHA_MIN):
    """The TSDF test's inputs: cameras and closed-form float32 maps of `views` orbit views (W x H, `size` squared by default) of a sphere"""
    cams = D.cams_for(size if W is None else W, size if H is None else H, n=views, elevation=elevation)
    return dict(N=N, bound=bound, trunc=trunc, alpha_min=alpha_min, cams=cams, maps=[sphere_view(c, radius) for c in cams])


# The default case and four with a partial last block of voxels (N^3 mod 256 = 168, 168, 152, 200), landscape and portrait views, cameras
# inside the volume (bound 2.25 > their distance 2: voxels at view z <= 0.2 and behind the camera), explicit trunc and alpha_min.
# Even N only: with odd N the centre plane of voxels projects exactly onto pixel-rounding boundaries of an even-sized image, and 4-6 % of the
# volume lands inside PIXEL_MARGIN (checked at N = 25 and N = 17).
_RAGGED = dict(radius=0.9, bound=2.25, trunc=0.4)
TSDF_CASES = {
    "default": dict(),
    "n26-40x24": dict(N=26, W=40, H=24, views=5, elevation=15.0, alpha_min=0.5, **_RAGGED),
    "n26-24x40": dict(N=26, W=24, H=40, views=5, elevation=-20.0, alpha_min=0.3, **_RAGGED),
    "n22-24x40": dict(N=22, W=24, H=40, views=4, elevation=-20.0, alpha_min=0.3, **_RAGGED),
    "n18-56x40": dict(N=18, W=56, H=40, views=3, elevation=15.0, alpha_min=0.5, **_RAGGED),
}
TSDF_CANARY_CASE = "n26-24x40"      # (the first voxel past this volume lies inside one of its views: tsdf_phantom_voxel)


def sphere_tsdf_views(case, dtype=torch.float64):
    """(volume, what tsdf_view returned per view) of a sphere_tsdf_case"""
    vol = new_volume(case["N"], case["bound"], case["trunc"], dtype=dtype)
    return vol, [tsdf_view(vol, d, a, img, cam, case["alpha_min"]) for cam, (d, a, img) in zip(case["cams"], case["maps"])]


def sphere_tsdf_restatement(case, dtype=torch.float64):
    """(volume, margin voxels [N^3] bool) of sphere_tsdf_case through tsdf_view"""
    vol, views = sphere_tsdf_views(case, dtype)
    near = tsdf_margins(views, vol["trunc"], case["alpha_min"])
    near |= (vol["weight"] > 0) & ((vol["tsdf_sum"] / vol["weight"].clamp_min(1)).abs() < SIGN_MARGIN)     # sign of the mean TSDF
    return vol, near


def tsdf_branch_counts(vol, views):
    """How often the restatement leaves tsdf_integrate_kernel by each of its ways, summed over the views (voxel-views), and the number of
    voxels no view wrote."""
    trunc = vol["trunc"]
    n = lambda f: sum(int(f(v).sum()) for v in views)  # noqa: E731
    surf = lambda v: v["seen"] & ~v["empty"]  # noqa: E731
    return dict(near_plane=n(lambda v: ~v["front"]), off_image=n(lambda v: v["front"] & ~v["seen"]), empty=n(lambda v: v["empty"]),
                behind=n(lambda v: surf(v) & (v["sdf"] < -trunc)), clamped=n(lambda v: surf(v) & (v["sdf"] > trunc)),
                colour=n(lambda v: surf(v) & (v["sdf"].abs() <= trunc)), unseen=int((vol["weight"] == 0).sum()))


def tsdf_phantom_voxel(case):
    """What tsdf_integrate_kernel would do with linear index N^3, the first past the volume (ix = iy = 0, iz = N), were its bound check off by
    one: the number of views of `case` that write it (fp64 statements of tsdf_view).  tests/test_recon_geom_cpu.py holds this above 0 for the
    case whose accumulators the GPU test surrounds with guard elements."""
    N, bound = case["N"], case["bound"]
    trunc = 4.0 * 2.0 * bound / N if case["trunc"] is None else case["trunc"]
    c = lambda i: (i + 0.5) * (2.0 * bound / N) - bound  # noqa: E731
    ph = torch.tensor([c(0), c(0), c(N), 1.0], dtype=torch.float64)
    written = 0
    for cam, (depth, alpha, _) in zip(case["cams"], case["maps"]):
        W, H = cam.width, cam.height
        zv = float((ph @ cam.world_view.double())[2])
        hom = ph @ cam.full_proj.double()
        pw = 1.0 / (float(hom[3]) + 1e-7)
        rx = np.floor(((float(hom[0]) * pw + 1) * W - 1) * 0.5 + 0.5)
        ry = np.floor(((float(hom[1]) * pw + 1) * H - 1) * 0.5 + 0.5)
        if not (zv > 0.2 and 0 <= rx < W and 0 <= ry < H):
            continue
        a, dm = float(alpha[int(ry), int(rx)]), float(depth[int(ry), int(rx)])
        written += int(a < case["alpha_min"] or not a > 0 or dm / a - zv >= -trunc)
    return written


# ---- depth / alpha cases ------------------------------------------------------------------------------------------------------------
# (kind, seed, W, H, view of cams_for): random_scene(300, seed) of gs_dense_ref.SCENE_SEEDS at 64 x 48 and at the ragged 56 x 40, two views
# each, one deep_scene(1200) case of gs_dense_ref.EDGE_CASES (tile lists of several batches, saturated pixels, early stop), and portrait
# images: 40 x 56, 24 x 72 and 8 x 24, the last narrower than one 16-pixel tile (a single column of tiles).  Every fp64 decision of every
# case keeps gs_dense_ref.SCENE_MARGIN (tests/test_recon_geom_cpu.py); (seed, view) pairs that do not on a portrait image are left out.
DEPTH_CASES = tuple(("random", seed, W, H, view) for seed in D.SCENE_SEEDS for W, H in ((64, 48), (56, 40)) for view in (0, 2)) + \
    (("deep", 73, 56, 40, 2),) + \
    (("random", 1116, 40, 56, 1), ("random", 2270, 40, 56, 3), ("random", 1116, 24, 72, 1), ("random", 2270, 24, 72, 3), ("random", 1116, 8, 24, 1))


def depth_case(case):
    kind, seed, W, H, view = case
    scene = D.random_scene(300, seed) if kind == "random" else D.deep_scene(1200, seed)
    return scene, D.cams_for(W, H)[view]


def depth_case_id(case):
    return f"{case[0]}{case[1]}-{case[2]}x{case[3]}-v{case[4]}"
