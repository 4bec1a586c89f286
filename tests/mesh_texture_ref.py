"""Pure-torch restatement of csrc_recon/meshtex.hip and of v3d_amd/recon/mesh_texture.py's loop (test oracle), fp64 by default; with
dtype=torch.float32 what that run loses against the fp64 one is the cost of the number format (the bar idiom of tests/mesh_render_ref.py).

Written from the statements of include/v3d_recon.h "Mesh texture".  Everything starts from a GIVEN face_id map and the pix_w of
v3d_recon_mesh_pixel_weights (the kernel's own, or mesh_refine_ref.pixel_weights'): coverage is not decided again here."""
from __future__ import annotations

import functools
import math

import numpy as np
import torch

import mesh_refine_ref as RF
import mesh_render_ref as M

FILL = 0.5
MIN_CELL = 4


# ---- the atlas ----------------------------------------------------------------------------------------------------------------------------
def layout(F, R):
    """(S, g); ValueError where a cell would be smaller than 4 texels"""
    cells = (F + 1) // 2
    g = 1
    while g * g < cells:
        g += 1
    S = R // g
    if S < MIN_CELL:
        raise ValueError(f"texture too small for {F} faces")
    return S, g


def _charts(f, S, g):
    """(x0, y0, half) of face indices f (int64 tensor)"""
    c = f >> 1
    return (c % g) * S, torch.div(c, g, rounding_mode="floor") * S, f & 1


def face_uvs(F, R, dtype=torch.float64):
    """vt [F, 3, 2] in texels"""
    S, g = layout(F, R)
    L = S - 3
    x0, y0, half = _charts(torch.arange(F), S, g)
    d = torch.tensor([[0, 0], [L, 0], [0, L]])                                       # place -> offset from the right-angle corner
    u = torch.where(half[:, None] == 0, x0[:, None] + d[None, :, 0], x0[:, None] + S - 1 - d[None, :, 0])
    v = torch.where(half[:, None] == 0, y0[:, None] + d[None, :, 1], y0[:, None] + S - 1 - d[None, :, 1])
    return torch.stack([u, v], -1).to(dtype)


def texel_cells(F, R):
    """(owner [R*R] int64, -1 where unowned; i, j [R*R]: the texel's local coordinates, mirrored in half 1)"""
    S, g = layout(F, R)
    y, x = torch.meshgrid(torch.arange(R), torch.arange(R), indexing="ij")
    x, y = x.reshape(-1), y.reshape(-1)
    inside = (x < g * S) & (y < g * S)
    cx, cy = torch.div(x, S, rounding_mode="floor"), torch.div(y, S, rounding_mode="floor")
    i, j = x - cx * S, y - cy * S
    half = (i + j > S - 2).long()
    f = 2 * (cy * g + cx) + half
    owner = torch.where(inside & (f < F), f, torch.full_like(f, -1))
    return owner, torch.where(half == 1, S - 1 - i, i), torch.where(half == 1, S - 1 - j, j)


def bake(faces, colors, R, dtype=torch.float64, fill=FILL):
    """(owner [R*R], texture [R*R, 3]): b1 = clamp(i / L, 0, 1), b2 = clamp(j / L, 0, 1 - b1), b0 = 1 - b1 - b2 over the face's colours;
    `fill` on unowned texels and on faces with an index outside 0 .. V-1"""
    F, V = faces.shape[0], colors.shape[0]
    S, _ = layout(F, R)
    owner, i, j = texel_cells(F, R)
    tri = faces.long()[owner.clamp_min(0)]
    ok = (owner >= 0) & ((tri >= 0) & (tri < V)).all(1)
    tri = torch.where(ok[:, None], tri, torch.zeros_like(tri))
    L = torch.tensor(float(S - 3), dtype=dtype)
    b1 = (i.to(dtype) / L).clamp(0, 1)
    b2 = torch.minimum((j.to(dtype) / L).clamp_min(0), 1 - b1)
    b0 = 1 - b1 - b2
    c = colors.to(dtype)
    tex = b0[:, None] * c[tri[:, 0]] + b1[:, None] * c[tri[:, 1]] + b2[:, None] * c[tri[:, 2]]
    return owner, torch.where(ok[:, None], tex, torch.full_like(tex, fill))


# ---- pixel -> texels, shade ---------------------------------------------------------------------------------------------------------------
@torch.no_grad()
def pixel_texels(face_id, pix_w, F, R, dtype=torch.float64):
    """dict(pix_tex [H, W, 4] int64 (-1 where nothing covers), pix_tw [H, W, 4], u, v, fu, fv [H, W] (0 where nothing covers))"""
    S, g = layout(F, R)
    L = S - 3
    H, W = face_id.shape
    fid = face_id.long().reshape(-1)
    w = pix_w.to(dtype).reshape(-1, 3)
    s = w.sum(1) if dtype == torch.float64 else (w[:, 0] + w[:, 1]) + w[:, 2]
    hit = (fid >= 0) & (fid < F) & (s > 0)
    s = torch.where(hit, s, torch.ones_like(s))
    f = fid.clamp(0, F - 1)
    x0, y0, half = _charts(f, S, g)
    hi = torch.where(half == 0, L, S - 1)
    # (u, v) = corner_0 + beta_1 (corner_1 - corner_0) + beta_2 (corner_2 - corner_0), relative to the cell's origin
    Lf, far = torch.tensor(float(L), dtype=dtype), torch.tensor(float(S - 1), dtype=dtype)
    du = (w[:, 1] / s * Lf).clamp(0, float(L))
    dv = torch.minimum((w[:, 2] / s * Lf).clamp_min(0), Lf - du)                      # beta_1 + beta_2 <= 1: under the hypotenuse in every format
    u, v = torch.where(half == 1, far - du, du), torch.where(half == 1, far - dv, dv)
    i0 = torch.minimum(torch.floor(u).long(), hi - 1)
    j0 = torch.minimum(torch.floor(v).long(), hi - 1)
    fu, fv = u - i0.to(dtype), v - j0.to(dtype)
    t0 = (y0 + j0) * R + x0 + i0
    tex = torch.stack([t0, t0 + 1, t0 + R, t0 + R + 1], 1)
    tw = torch.stack([(1 - fu) * (1 - fv), fu * (1 - fv), (1 - fu) * fv, fu * fv], 1)
    z = lambda a: torch.where(hit, a, torch.zeros_like(a)).reshape(H, W)  # noqa: E731
    # a coordinate whose weight is exactly 0 (du = 0 L), or the only one that is not (du = 1 L): no rounding in any format
    zero = w == 0
    exact_u, exact_v = zero[:, 1] | (zero[:, 0] & zero[:, 2]), zero[:, 2] | (zero[:, 0] & zero[:, 1])
    return dict(pix_tex=torch.where(hit[:, None], tex, torch.full_like(tex, -1)).reshape(H, W, 4),
                pix_tw=torch.where(hit[:, None], tw, torch.zeros_like(tw)).reshape(H, W, 4), u=z(u), v=z(v), fu=z(fu), fv=z(fv),
                exact_u=(hit & exact_u).reshape(H, W), exact_v=(hit & exact_v).reshape(H, W))


def compared_taps(pt, margin=1e-4):
    """[H, W] bool: the covered pixels on which pix_tex is compared exactly, and the share of covered pixels that leaves out.  A coordinate
    is kept when its fp64 fraction lies further than `margin` from 0 and 1 (there a float32 floor cannot fall the other way), or when it is
    exact in every format: a pixel centre on a snapped vertex or edge has a weight of exactly 0, and 0 L and 1 L are not rounded.  (At 0
    sub-pixel bits every covered centre of a small face is such a point; leaving those out would leave nothing to compare.)"""
    hit = pt["pix_tex"][..., 0] >= 0
    clear = lambda a: (a > margin) & (a < 1 - margin)  # noqa: E731
    keep = hit & (clear(pt["fu"]) | pt["exact_u"]) & (clear(pt["fv"]) | pt["exact_v"])
    return keep, 1.0 - float(keep.sum()) / max(int(hit.sum()), 1)


def shade(pix_tex, pix_tw, texture, bg, dtype=torch.float64):
    """image [3, H, W]: the four taps' weighted sum on covered pixels, bg elsewhere.  Differentiable in `texture` (torch autograd)."""
    H, W = pix_tex.shape[:2]
    pt = pix_tex.reshape(-1, 4)
    hit = pt[:, 0] >= 0
    idx = pt.clamp_min(0)
    q, T = pix_tw.to(dtype).reshape(-1, 4), texture.to(dtype)
    img = ((q[:, 0:1] * T[idx[:, 0]] + q[:, 1:2] * T[idx[:, 1]]) + q[:, 2:3] * T[idx[:, 2]]) + q[:, 3:4] * T[idx[:, 3]]
    bgt = torch.as_tensor(bg, dtype=dtype).reshape(1, 3)
    return torch.where(hit[:, None], img, bgt.expand_as(img)).t().reshape(3, H, W)


def foreign_weight(pix_tex, pix_tw, face_id, owner):
    """[H, W]: per pixel the weight on texels that its face does not own"""
    t = pix_tex.clamp_min(0)
    mine = owner[t] == face_id.long()[..., None]
    return torch.where(mine | (pix_tex < 0), torch.zeros_like(pix_tw), pix_tw.abs()).sum(-1)


# ---- the transpose --------------------------------------------------------------------------------------------------------------------------
@torch.no_grad()
def texel_lists(pix_tex, T):
    """(table [T, L] int64 of record numbers 4 pixel + j in ascending order, padded with -1; length [T]): a stable sort of the records of
    the covered pixels on the texel, as the host builds them"""
    rec = torch.nonzero(pix_tex.reshape(-1) >= 0).reshape(-1)
    tex = pix_tex.reshape(-1)[rec]
    order = torch.sort(tex, stable=True).indices
    tex, rec = tex[order], rec[order]
    length = torch.bincount(tex, minlength=T)
    start = torch.cumsum(length, 0) - length
    L = int(length.max()) if rec.numel() else 0
    table = torch.full((T, max(L, 1)), -1, dtype=torch.long)
    table[tex, torch.arange(rec.numel()) - start[tex]] = rec
    return table, length


@torch.no_grad()
def list_sum(table, ent_w, ent_g, dtype=torch.float64):
    """rows [T, C]: for every texel the sum over its list of ent_w[e] ent_g[e, :], IN THE KERNEL'S ORDER: front to back, one running sum.
    The one place that states the order (mesh_refine_ref.list_sum is the other order, a wave per row).  -1 pads add an exact 0."""
    pad = table < 0
    t = table.clamp_min(0)
    term = ent_w.to(dtype)[t][..., None] * ent_g.to(dtype)[t]
    term = torch.where(pad[..., None], torch.zeros_like(term), term)
    acc = torch.zeros(table.shape[0], term.shape[-1], dtype=dtype)
    for k in range(table.shape[1]):
        acc = acc + term[:, k]
    return acc


@torch.no_grad()
def shade_transpose(pix_tex, pix_tw, dL_dimage, T, dtype=torch.float64, lists=None):
    """dL_dtexture [T, 3] as the explicit sum over the records (pixel p, tap j) of every texel, in ascending 4 p + j"""
    table, _ = lists if lists is not None else texel_lists(pix_tex, T)
    H, W = pix_tex.shape[:2]
    g = dL_dimage.to(dtype).reshape(3, H * W).t().repeat_interleave(4, 0)              # by record number
    return list_sum(table, pix_tw.to(dtype).reshape(-1), g, dtype)


def synthetic_transpose(ranges, ent_pix, ent_w, dL_dimage, dtype=torch.float64):
    T = ranges.shape[0]
    length = (ranges[:, 1] - ranges[:, 0]).long()
    table = torch.full((T, max(int(length.max()), 1)), -1, dtype=torch.long)
    for t in range(T):
        table[t, :int(length[t])] = torch.arange(int(ranges[t, 0]), int(ranges[t, 1]))
    return list_sum(table, ent_w, dL_dimage.reshape(3, -1).t()[ent_pix.long()], dtype)


LIST_LENGTHS = (0, 1, 2, 63, 64, 65, 700)


def synthetic_lists(W=64, H=48, seed=0):
    """One texel per length of LIST_LENGTHS (+ a trailing one without entries): mesh_refine_ref.synthetic_lists with these lengths"""
    g = torch.Generator().manual_seed(seed)
    lens = list(LIST_LENGTHS) + [0]
    ranges, pix, o = [], [], 0
    for n in lens:
        ranges.append((o, o + n) if n else (0, 0))
        pix.append(torch.sort(torch.randperm(W * H, generator=g)[:n]).values)
        o += n
    mag = lambda *s: (torch.randn(*s, generator=g) * torch.pow(10.0, 3 * (2 * torch.rand(*s, generator=g) - 1))).float()  # noqa: E731
    return (torch.tensor(ranges, dtype=torch.int32), torch.cat(pix).to(torch.int32), mag(o), mag(3, H, W))


# ---- the loop -------------------------------------------------------------------------------------------------------------------------------
@torch.no_grad()
def frozen_view(face_id, pix_w, F, R, dtype=torch.float64):
    pt = pixel_texels(face_id, pix_w, F, R, dtype)
    return dict(pix_tex=pt["pix_tex"], pix_tw=pt["pix_tw"], lists=texel_lists(pt["pix_tex"], R * R))


@torch.no_grad()
def fit(views, targets, baked, iterations, lr, seed, bg, dtype=torch.float64):
    """The loop of fit_texture on frozen views (one per optimisation view) and their targets [3, H, W], from the baked texture [T, 3]:
    dict(texture (unseen texels keep `baked`), seen [T], loss_first, loss_last, losses)"""
    T = baked.shape[0]
    logit = RF.initial_logits(baked, dtype)
    cur = RF.sigmoid(logit)
    m, s = torch.zeros_like(logit), torch.zeros_like(logit)
    tg = [t.to(dtype) for t in targets]
    losses = []
    for it, j in enumerate(RF.view_schedule(len(views), iterations, seed)):
        vw = views[j]
        diff = shade(vw["pix_tex"], vw["pix_tw"], cur, bg, dtype) - tg[j]
        losses.append(float((diff * diff).mean()))
        grad = shade_transpose(vw["pix_tex"], vw["pix_tw"], diff * (2.0 / diff.numel()), T, dtype, vw["lists"])
        cur = RF.adam_step(logit, m, s, grad, it + 1, lr)
    seen = torch.zeros(T, dtype=torch.bool)
    for vw in views:
        seen |= vw["lists"][1] > 0
    return dict(texture=torch.where(seen[:, None], cur, baked.to(dtype)), seen=seen, loss_first=losses[0] if losses else None,
                loss_last=losses[-1] if losses else None, losses=losses)


def psnr(a, b):
    return float(-10.0 * torch.log10(((a.double().clamp(0, 1) - b.double()) ** 2).mean()))


# ---- cases ----------------------------------------------------------------------------------------------------------------------------------
# (F, R) of the layout test; the sizes the header quotes
LAYOUT_F = (1, 2, 3, 319, 320, 50_000, 131_072)
LAYOUT_R = (64, 100, 128, 1024)
QUOTED = {(50_000, 1024): 6, (50_000, 2048): 12, (320, 64): 4, (320, 128): 9, (1344, 256): 9}
BAKE_R = (64, 128, 100)

# Pixel -> texels: R and the scene's seed per raster case.  pix_tex is compared where the fp64 fu and fv are further than 1e-4 from 0 and 1;
# the share of covered pixels that leaves out must stay within mesh_render_ref.EXCLUDE_MAX (2 %) ON THE RESTATEMENT ALONE
# (tests/test_mesh_texture_cpu.py::test_premises_of_the_gpu_cases).  R = 100 (ragged, S = 7 for the sphere) was the first choice for every
# case and held it; the scenes keep the seeds of mesh_render_ref, so nothing was searched.
TAP_MARGIN = 1e-4
CASE_R = 100
TEX_CASES = M.RASTER_CASES + M.REFINE_EDGE_CASES


def random_texture(R, seed=11):
    return torch.rand(R * R, 3, generator=torch.Generator().manual_seed(seed))


@functools.lru_cache(maxsize=None)
def case_restatement(case):
    """A raster case wholly on the restatements (float32 projection, fp64 raster, float32 pixel weights as the kernel stores them):
    (verts, faces, colors, face_id, pix_w float32)"""
    kind, seed, W, H, _, cull = case[:6]
    bits = M.case_bits(case)
    v, f, c = M.mesh_scene(kind, seed)
    pr = M.project(v, M.case_camera(case), bits, torch.float32)
    r = M.rasterize(pr["pix_q"], pr["zv"], f, c, W, H, RF.BG, bits=bits, cull=cull)
    _, pw = RF.pixel_weights(pr["pix_q"], pr["zv"], f, r["face_id"], bits, torch.float32)
    return v, f, c, r["face_id"], pw


# ---- the end-to-end scene ---------------------------------------------------------------------------------------------------------------
# The 24^3 sphere of the extraction tests (1344 faces), decimated to 400 faces (mesh_decimate_ref.LOOP_CASES["net"]); 8 orbit cameras at
# 64 x 64, all of them optimised against; R = 128.  The target is the UNDECIMATED mesh with tinted position_colors (mesh_refine_ref.E2E says
# why tinted) times a stripe along x of period STRIPE_PERIOD, finer than the decimated mesh's vertex spacing (about 0.1): vertex colours on
# 202 vertices cannot carry it, a texture of S = 8 texels to a cell can.  LR and ITERATIONS are mesh_refine_ref's.
E2E = dict(RF.E2E, num_opt=0, target_faces=400, tex_size=128)
STRIPE_PERIOD = 0.12
STRIPE_DEPTH = 0.5


def stripe_colors(verts):
    """tinted position colours times a stripe in x: [V, 3] float32"""
    s = 1.0 - STRIPE_DEPTH * (torch.sin(verts[:, 0].double() * (2 * math.pi / STRIPE_PERIOD)) > 0).double()
    return (M.position_colors(verts, E2E["tint"]).double() * s[:, None]).float()


@functools.lru_cache(maxsize=None)
def e2e_cpu():
    """The end-to-end scene wholly on the restatements: dict(full=(verts, faces, colours) of the 1344-face mesh with stripe_colors, mesh=
    (verts, faces, colors0) of its decimation to 400 faces with the stripe sampled at the vertices left, cams, targets [8, 3, S, S] float32,
    views=[(pix_q, zv, face_id, depth, pix_w float32)] of the decimated mesh)"""
    import mesh_decimate_ref as DM
    vf, ff, _ = DM.scene("net")
    kept, fd, _ = DM.decimate(vf.numpy(), ff.numpy(), E2E["target_faces"])
    vd, fd = vf[torch.from_numpy(kept)], torch.from_numpy(fd)
    cf, cd = stripe_colors(vf), stripe_colors(vd)
    cams, S = RF.e2e_cameras(), E2E["size"]
    targets, views = [], []
    for cam in cams:
        pr = M.project(vf, cam, 8, torch.float32)
        targets.append(M.rasterize(pr["pix_q"], pr["zv"], ff, cf, S, S, RF.BG, cull=True)["image"].float())
        pd = M.project(vd, cam, 8, torch.float32)
        r = M.rasterize(pd["pix_q"], pd["zv"], fd, cd, S, S, RF.BG, cull=True)
        _, pw = RF.pixel_weights(pd["pix_q"], pd["zv"], fd, r["face_id"], 8, torch.float32)
        views.append((pd["pix_q"], pd["zv"], r["face_id"], r["depth"], pw))
    return dict(full=(vf, ff, cf), mesh=(vd, fd, cd), cams=cams, targets=torch.stack(targets), views=views)


def e2e_restatement(mesh, targets, views, dtype=torch.float64):
    """Both loops on frozen views [(pix_q, zv, face_id, depth, pix_w float32)] of the decimated mesh, all views optimised, the schedule and
    step of mesh_refine_ref: dict(tex: fit()'s result, psnr_vertex, psnr_baked, psnr_fitted, psnr_refined (refine_vertex_colors' restatement
    from the same start), gain = psnr_fitted - psnr_refined); PSNRs are means over all views"""
    vd, fd, cd = mesh
    R, F, V = E2E["tex_size"], fd.shape[0], vd.shape[0]
    tv = [frozen_view(fid, pw, F, R, dtype) for _, _, fid, _, pw in views]
    _, baked = bake(fd, cd, R, torch.float32)
    baked = baked.float()
    tex = fit(tv, list(targets), baked, RF.ITERATIONS, RF.LR, E2E["seed"], RF.BG, dtype)
    mean = lambda imgs: float(np.mean([psnr(i, t) for i, t in zip(imgs, targets)]))  # noqa: E731
    rv = [RF.frozen_view(q, zv, fd, fid, depth, V, dtype) for q, zv, fid, depth, _ in views]
    ref = RF.refine(rv, list(targets), cd, RF.ITERATIONS, RF.LR, E2E["seed"], RF.BG, dtype)
    vshade = lambda c: [RF.shade(w["pix_vert"], w["pix_w"], w["depth"], c, RF.BG, dtype) for w in rv]  # noqa: E731
    tshade = lambda t: [shade(w["pix_tex"], w["pix_tw"], t, RF.BG, dtype) for w in tv]  # noqa: E731
    out = dict(tex=tex, psnr_vertex=mean(vshade(cd)), psnr_baked=mean(tshade(baked)), psnr_fitted=mean(tshade(tex["texture"])),
               psnr_refined=mean(vshade(ref["colors"])))
    out["gain"] = out["psnr_fitted"] - out["psnr_refined"]
    mse = lambda imgs: float(np.mean([float(((i.double() - t.double()) ** 2).mean()) for i, t in zip(imgs, targets)]))  # noqa: E731
    out["mse_baked"], out["mse_fitted"] = mse(tshade(baked)), mse(tshade(tex["texture"]))
    return out
