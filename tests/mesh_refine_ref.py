"""Pure-torch restatement of csrc_recon/meshshade.hip and of v3d_amd/recon/mesh_refine.py's loop (test oracle), fp64 by default; with
dtype=torch.float32 what that run loses against the fp64 one is the cost of the number format (the bar idiom of tests/mesh_render_ref.py).

Everything starts from GIVEN snapped positions pix_q, view z, a face_id map and a depth map (the kernel's own, or mesh_render_ref.rasterize's):
coverage is not decided again here.  The edge functions are int64 and exact; the quotients, the shade, the transpose and Adam are in `dtype`."""
from __future__ import annotations

import numpy as np
import torch

import gs_dense_ref as D
import mesh_render_ref as M
import recon_geom_ref as R

COLOR_CLAMP = 0.5 / 255.0
BETAS, EPS = (0.9, 0.999), 1e-8

# ---- the end-to-end scene of tests/test_mesh_refine_{cpu,gpu}.py ------------------------------------------------------------------------
# The 24^3 sphere of the extraction tests, 8 orbit cameras at 64 x 64, target colours position_colors, start from 0.5 grey, 4 optimisation
# views.  LR and ITERATIONS are INPUTS: chosen on the CPU so that the fp64 restatement below brings the mean squared error over the
# optimisation views to a tenth of its initial value at most (tests/test_mesh_refine_cpu.py::test_restatement_refinement_converges: 0.021
# of it with these).
# The target is tinted.  Untinted, position_colors equals the grey start EXACTLY on the planes through the sphere's centre, and the scene is
# mirror-symmetric about them: the gradient of a vertex there is a sum that cancels to rounding noise, 1e-17 in fp64 and 1e-11 in float32,
# and Adam's eps of 1e-8 turns the float32 noise into a drift of 1e-3 .. 1e-2 that the fp64 run does not have.  Two float32 runs that differ
# only in the order of one sum then differ from each other as much as from fp64, and a comparison of final colours says nothing.  With the
# tint no vertex starts at its target; the float32 run ends 1e-5 from the fp64 one.
E2E = dict(N=24, bound=1.0, radius=0.5, views=8, size=64, num_opt=4, seed=0, orbit=(2.0, 0.0, 60.0), tint=(0.9, 0.7, 0.5))
LR = 0.05
ITERATIONS = 60
BG = [1.0, 1.0, 1.0]


def e2e_cameras():
    from v3d_amd.recon.cameras import orbit_cameras
    return orbit_cameras(E2E["views"], *E2E["orbit"], E2E["size"])[0]


def e2e_mesh():
    """(verts float32, faces int64, target colours float32) of the restatement's surface nets on the sphere volume"""
    v, f, _, _, _ = R.extract(R.sphere_volume(E2E["N"], E2E["bound"], E2E["radius"]))
    v = v.float()
    return v, f, M.position_colors(v, E2E["tint"])


# ---- per-pixel vertices and weights -----------------------------------------------------------------------------------------------------
@torch.no_grad()
def pixel_weights(pix_q, zv, faces, face_id, bits=8, dtype=torch.float64):
    """(pix_vert [H, W, 3] int64, -1 where face_id < 0; pix_w [H, W, 3] = b_k / zv[i_k], 0 where nothing covers)"""
    H, W = face_id.shape
    fid = face_id.long().reshape(-1)
    hit = fid >= 0
    tri = faces.long()[fid.clamp_min(0)]                                      # [P, 3]
    q = pix_q.long()
    S = 1 << bits
    ys, xs = torch.meshgrid(torch.arange(H, dtype=torch.long), torch.arange(W, dtype=torch.long), indexing="ij")
    Px, Py = xs.reshape(-1) * S, ys.reshape(-1) * S
    ax, ay, bx, by, cx, cy = (q[tri[:, k], d] for k in range(3) for d in range(2))
    a2 = (bx - ax) * (cy - ay) - (by - ay) * (cx - ax)
    s = torch.where(a2 < 0, -1, 1)
    e0 = s * ((cx - bx) * (Py - by) - (cy - by) * (Px - bx))
    e1 = s * ((ax - cx) * (Py - cy) - (ay - cy) * (Px - cx))
    e2 = s * ((bx - ax) * (Py - ay) - (by - ay) * (Px - ax))
    fa = (e0 + e1 + e2).to(dtype)
    fa = torch.where(hit, fa, torch.ones_like(fa))
    z3 = zv.to(dtype)[tri]
    w = torch.stack([e0.to(dtype) / fa / z3[:, 0], e1.to(dtype) / fa / z3[:, 1], e2.to(dtype) / fa / z3[:, 2]], 1)
    pix_vert = torch.where(hit[:, None], tri, torch.full_like(tri, -1))
    return pix_vert.reshape(H, W, 3), torch.where(hit[:, None], w, torch.zeros_like(w)).reshape(H, W, 3)


# ---- shade and its transpose ------------------------------------------------------------------------------------------------------------
def shade(pix_vert, pix_w, depth, colors, bg, dtype=torch.float64):
    """image [3, H, W]: depth (w0 c[i0] + w1 c[i1] + w2 c[i2]) on covered pixels, bg elsewhere.  Differentiable in `colors` (torch autograd)."""
    H, W = depth.shape
    pv = pix_vert.reshape(-1, 3)
    hit = pv[:, 0] >= 0
    idx = pv.clamp_min(0)
    w, c = pix_w.to(dtype).reshape(-1, 3), colors.to(dtype)
    acc = w[:, 0:1] * c[idx[:, 0]] + w[:, 1:2] * c[idx[:, 1]] + w[:, 2:3] * c[idx[:, 2]]
    img = depth.to(dtype).reshape(-1, 1) * acc
    bgt = torch.as_tensor(bg, dtype=dtype).reshape(1, 3)
    return torch.where(hit[:, None], img, bgt.expand_as(img)).t().reshape(3, H, W)


@torch.no_grad()
def vertex_lists(pix_vert, V):
    """The transposed lists as a padded table: (table [V, L] int64 of record numbers 3 pixel + k in ascending order, padded with -1;
    length [V]).  Built by a stable sort of the records of the covered pixels on the vertex, as the host builds them."""
    rec = torch.nonzero(pix_vert.reshape(-1) >= 0).reshape(-1)                 # ascending 3 pixel + k
    vert = pix_vert.reshape(-1)[rec]
    order = torch.sort(vert, stable=True).indices
    vert, rec = vert[order], rec[order]
    length = torch.bincount(vert, minlength=V)
    start = torch.cumsum(length, 0) - length
    L = int(length.max()) if rec.numel() else 0
    table = torch.full((V, max(L, 1)), -1, dtype=torch.long)
    table[vert, torch.arange(rec.numel()) - start[vert]] = rec
    return table, length


WAVE = 64


@torch.no_grad()
def list_sum(table, ent_w, ent_g, dtype=torch.float64):
    """rows [V, C]: for every vertex the sum over its list of ent_w[e] ent_g[e, :], IN THE KERNEL'S ORDER: 64 partial sums, the l-th over
    entries l, l + 64, .. of the list in list order, which then meet in an xor butterfly (offsets 32, 16, .. 1).  In fp64 the order hardly
    matters; in float32 it decides which roundings a row with cancellation gets, and a restatement that added left to right would be off
    from fp64 by a different draw of the same size (a row of 29 entries whose terms are 28 x its sum: 2.9e-7 one way, 7.5e-7 the other).
    `table` [V, L] holds entry numbers, -1 pads (a pad adds an exact 0)."""
    V, L = table.shape
    Lp = (L + WAVE - 1) // WAVE * WAVE
    tab = torch.cat([table, torch.full((V, Lp - L), -1, dtype=table.dtype)], 1)
    pad = tab < 0
    t = tab.clamp_min(0)
    term = ent_w.to(dtype)[t][..., None] * ent_g.to(dtype)[t]
    term = torch.where(pad[..., None], torch.zeros_like(term), term).reshape(V, Lp // WAVE, WAVE, -1)
    lanes = term.cumsum(1)[:, -1]                                              # [V, 64, C]: each lane adds its entries in list order
    lane = torch.arange(WAVE)
    o = WAVE // 2
    while o:
        lanes = lanes + lanes[:, lane ^ o]
        o //= 2
    return lanes[:, 0]


@torch.no_grad()
def shade_transpose(pix_vert, pix_w, depth, dL_dimage, V, dtype=torch.float64, lists=None):
    """dL_dcolors [V, 3] as the explicit sum: over the records (pixel p, corner k) of vertex v, listed in ascending pixel order, of
    (depth[p] pix_w[p][k]) dL_dimage[:, p], added in the order of list_sum"""
    table, _ = lists if lists is not None else vertex_lists(pix_vert, V)
    H, W = depth.shape
    w = (depth.to(dtype).reshape(-1, 1) * pix_w.to(dtype).reshape(-1, 3)).reshape(-1)       # by record number 3 p + k
    g = dL_dimage.to(dtype).reshape(3, H * W).t().repeat_interleave(3, 0)                   # by record number
    return list_sum(table, w, g, dtype)


# ---- Adam on logits ---------------------------------------------------------------------------------------------------------------------
def sigmoid(x):
    return 1.0 / (1.0 + torch.exp(-x))


def initial_logits(colors, dtype=torch.float64):
    c = colors.float().clamp(COLOR_CLAMP, 1.0 - COLOR_CLAMP).to(dtype)         # (the clamp on the float32 colours, as the host does it)
    return torch.log(c / (1.0 - c))


@torch.no_grad()
def adam_step(logit, m, v, grad_colors, step, lr, betas=BETAS, eps=EPS):
    """One step of torch.optim.Adam on the logits, in place, from the gradient with respect to colors = sigmoid(logit); returns the new colours"""
    s = sigmoid(logit)
    g = grad_colors.to(logit.dtype) * s * (1.0 - s)
    m += (g - m) * (1.0 - betas[0])
    v.mul_(betas[1]).add_((1.0 - betas[1]) * g * g)
    bc1, bc2 = 1.0 - betas[0] ** step, 1.0 - betas[1] ** step
    denom = v.sqrt() / (bc2 ** 0.5) + eps
    logit -= (lr / bc1) * (m / denom)
    return sigmoid(logit)


# ---- the loop ---------------------------------------------------------------------------------------------------------------------------
def optimisation_views(num_views, num_opt):
    return list(range(num_views)) if num_opt == 0 else [int(i) for i in np.linspace(0, num_views, num_opt + 1)[:num_opt].astype(int)]


def view_schedule(num_opt_views, iterations, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(num_opt_views, (iterations,), generator=g).tolist()


@torch.no_grad()
def frozen_view(pix_q, zv, faces, face_id, depth, V, dtype=torch.float64, bits=8):
    pv, pw = pixel_weights(pix_q, zv, faces, face_id, bits=bits, dtype=dtype)
    return dict(pix_vert=pv, pix_w=pw, depth=depth.to(dtype), lists=vertex_lists(pv, V))


@torch.no_grad()
def refine(views, targets, colors0, iterations, lr, seed, bg, dtype=torch.float64):
    """The loop of refine_vertex_colors on frozen views (frozen_view, one per optimisation view) and their target images [3, H, W]:
    dict(colors [V, 3] (unseen vertices keep colors0), logit, seen [V] bool, loss_first, loss_last, mse_before, mse_after: mean squared
    error over the optimisation views with the initial / final colours)"""
    V = colors0.shape[0]
    logit = initial_logits(colors0, dtype)
    cur = sigmoid(logit)
    m, s = torch.zeros_like(logit), torch.zeros_like(logit)
    tg = [t.to(dtype) for t in targets]
    mse = lambda c: float(np.mean([float(((shade(vw["pix_vert"], vw["pix_w"], vw["depth"], c, bg, dtype) - t) ** 2).mean())  # noqa: E731
                                   for vw, t in zip(views, tg)]))
    before = mse(cur)
    first = last = None
    for it, j in enumerate(view_schedule(len(views), iterations, seed)):
        vw = views[j]
        diff = shade(vw["pix_vert"], vw["pix_w"], vw["depth"], cur, bg, dtype) - tg[j]
        loss = float((diff * diff).mean())
        first, last = (loss if it == 0 else first), loss
        grad = shade_transpose(vw["pix_vert"], vw["pix_w"], vw["depth"], diff * (2.0 / diff.numel()), V, dtype, vw["lists"])
        cur = adam_step(logit, m, s, grad, it + 1, lr)
    seen = torch.zeros(V, dtype=torch.bool)
    for vw in views:
        seen |= vw["lists"][1] > 0
    out = torch.where(seen[:, None], cur, colors0.to(dtype))
    return dict(colors=out, logit=logit, seen=seen, loss_first=first, loss_last=last, mse_before=before, mse_after=mse(cur))


# ---- synthetic lists for the transpose entry ----------------------------------------------------------------------------------------------
LIST_LENGTHS = (0, 1, 63, 64, 65, 128, 700)


def synthetic_lists(W=64, H=48, seed=0):
    """One vertex per length of LIST_LENGTHS (+ a trailing vertex without entries): (ranges [V, 2] int32, ent_pix [n] int32 ascending inside a
    list, ent_w [n] float32, dL_dimage [3, H, W] float32), weights and gradients of mixed sign and magnitude (1e-3 .. 1e3)"""
    g = torch.Generator().manual_seed(seed)
    lens = list(LIST_LENGTHS) + [0]
    ranges, pix, o = [], [], 0
    for n in lens:
        ranges.append((o, o + n) if n else (0, 0))
        pix.append(torch.sort(torch.randperm(W * H, generator=g)[:n]).values)
        o += n
    mag = lambda *s: (torch.randn(*s, generator=g) * torch.pow(10.0, 3 * (2 * torch.rand(*s, generator=g) - 1))).float()  # noqa: E731
    return (torch.tensor(ranges, dtype=torch.int32), torch.cat(pix).to(torch.int32), mag(o), mag(3, H, W))


def synthetic_transpose(ranges, ent_pix, ent_w, dL_dimage, dtype=torch.float64):
    V = ranges.shape[0]
    length = (ranges[:, 1] - ranges[:, 0]).long()
    table = torch.full((V, max(int(length.max()), 1)), -1, dtype=torch.long)
    for v in range(V):
        table[v, :int(length[v])] = torch.arange(int(ranges[v, 0]), int(ranges[v, 1]))
    g = dL_dimage.reshape(3, -1).t()[ent_pix.long()]
    return list_sum(table, ent_w, g, dtype)


def full_quad(W=64, H=48, bits=8):
    """Two front-facing triangles (negative doubled area) that cover the whole image, corners one pixel outside it: each of the two vertices
    on the diagonal owns one record of EVERY pixel.  (pix_q [4, 2] int64, zv [4], faces [2, 3], colors [4, 3])"""
    q = torch.tensor([[-1, -1], [W, -1], [W, H], [-1, H]], dtype=torch.long) << bits
    return q, torch.tensor([2.0, 2.2, 2.5, 1.9]), torch.tensor([[0, 2, 1], [0, 3, 2]]), torch.tensor([[1.0, 0.2, 0.1], [0.1, 0.9, 0.3], [0.2, 0.3, 1.0],
                                                                                                      [0.7, 0.7, 0.1]])


def row_errors(x, ref):
    """(relative L2 over all rows, largest per-row relative L2 over the rows whose norm is above 1e-3 of the largest row's) of x against ref"""
    x, ref = x.double(), ref.double()
    rn = ref.norm(dim=1)
    big = rn > 1e-3 * rn.max()
    per = ((x - ref).norm(dim=1) / rn.clamp_min(1e-300))[big]
    return float((x - ref).norm() / ref.norm().clamp_min(1e-300)), float(per.max()) if per.numel() else 0.0
