"""Pure-torch restatement of csrc_recon/meshdeform.hip and of v3d_amd/recon/mesh_deform.py's loop (test oracle), fp64 by default; with
dtype=torch.float32 what that run loses against the fp64 one is the cost of the number format (the bar idiom of tests/mesh_render_ref.py).

The pair rule starts from GIVEN unsnapped positions pix_f, snapped positions pix_q and a face_id map (the kernel's own, or
mesh_render_ref's): coverage is not decided again here.  The sign s is int64 and exact; the edge functions, t, the sums, the backward, the
projection's backward and the smoothness gradient are in `dtype`, every product and difference rounded on its own, as the kernel's."""
from __future__ import annotations

import torch

import gs_dense_ref as D
import mesh_refine_ref as RF
import mesh_render_ref as M

NEIGH = ((1, 0), (-1, 0), (0, 1), (0, -1))          # (dx, dy): right, left, down, up

# ---- decision margins -------------------------------------------------------------------------------------------------------------------
# The float32 run of the restatement is off from the fp64 one by 1.1e-7 .. 3.3e-7 in alpha_aa on the scenes below (AA_FP32_ERR holds it
# below 5e-7 on the CPU).  A float decision of the fp64 run keeps its outcome in float32 when it is further from its threshold than that
# rounding: the margins are 8 x AA_FP32_ERR (the idiom of mesh_render_ref.Z_GAP_MARGIN), far below what the scenes keep (|t - 0.5| >= 3.4e-4,
# the two smallest t_k >= 1.1e-3 apart, |E_k(q)| >= 3.3e-3, no sum within the margin of the clamps).
AA_FP32_ERR = 5e-7
T_HALF_MARGIN = 4e-6          # |t - 0.5|: which pixel receives
T_TIE_MARGIN = 4e-6           # the two smallest t_k: which edge is chosen
EQ_MARGIN = 4e-6              # |E_k(q)|: which edges are candidates
CLAMP_MARGIN = 4e-6           # the unclamped sum's distance from 0 and 1 on a receiver
EXCLUDE_MAX = 0.02            # of the pairs, should a later case need to leave some out (none of these does)

# the scenes: the six culling-on cases of mesh_render_ref.RASTER_CASES and the ragged sizes of REFINE_EDGE_CASES at 8 sub-pixel bits
DEFORM_CASES = tuple(c for c in M.RASTER_CASES if c[5]) + (("sphere", 1, 37, 21, 1, True), ("pair", 1, 13, 9, 3, True))

# ---- the end-to-end scene ---------------------------------------------------------------------------------------------------------------
E2E = dict(kind="sphere", seed=1, scale=0.85, centre=(0.03, -0.02, 0.04), size=48, steps=40, lr=5e-3, seed_views=0)
# what the fp64 restatement reaches at these settings with the regularisers at their defaults (alpha MSE summed over the four views),
# held by tests/test_mesh_deform_cpu.py::test_restatement_fit_reaches_its_recorded_figure
E2E_MSE_BEFORE = 0.145
E2E_MSE_AFTER = 0.01037
LAMBDA_OFFSET, LAMBDA_SMOOTH = 0.1, 10.0


def e2e_mesh():
    v, f, _ = M.mesh_scene(E2E["kind"], E2E["seed"])
    c = torch.tensor(E2E["centre"])
    return (c + E2E["scale"] * (v - c)).float().contiguous(), f, v


def e2e_cameras():
    return D.cams_for(E2E["size"], E2E["size"])


# ---- the pair rule ----------------------------------------------------------------------------------------------------------------------
def _grid(H, W):
    return torch.meshgrid(torch.arange(H, dtype=torch.long), torch.arange(W, dtype=torch.long), indexing="ij")


def _faces_at(pix_f, pix_q, faces, face_id, dtype):
    """per pixel: corners [H, W, 3, 2] in dtype of the pixel's face (face 0 where nothing covers), s [H, W], vertex indices [H, W, 3]"""
    fid = face_id.long()
    tri = faces.long()[fid.clamp_min(0)]
    q = pix_q.long()[tri]
    a2 = (q[..., 1, 0] - q[..., 0, 0]) * (q[..., 2, 1] - q[..., 0, 1]) - (q[..., 1, 1] - q[..., 0, 1]) * (q[..., 2, 0] - q[..., 0, 0])
    s = torch.where(a2 < 0, -1.0, 1.0).to(dtype)
    return pix_f.to(dtype)[tri], s, tri


def edge_functions(c, s, X, Y):
    """E_k [.., 3] = s cross(v - u, x - u) of the edges corner k -> corner k + 1 of corners c [.., 3, 2] at points X, Y [..]"""
    u, v = c, c.roll(-1, -2)
    dx, dy = v[..., 0] - u[..., 0], v[..., 1] - u[..., 1]
    rx, ry = X[..., None] - u[..., 0], Y[..., None] - u[..., 1]
    return s[..., None] * (dx * ry - dy * rx)


@torch.no_grad()
def pairs(pix_f, pix_q, faces, face_id, dtype=torch.float64, float_sign=False):
    """The pair rule on every (pixel, neighbour): dict of [H, W, 4] tensors.  pair: p covered, q inside and uncovered;  k: the chosen edge,
    -1 without a candidate (or without a pair);  t, ep (E_k(p) BEFORE the clamp), eq of the chosen edge;  recv_q: the neighbour receives
    (not t < 0.5);  second: the second smallest t_k (inf with one candidate);  eq_min: the smallest |E_k(q)| over the three edges;
    info: the kernel's pair_info.  Also tri [H, W, 3], s [H, W], covered [H, W]."""
    H, W = face_id.shape
    ys, xs = _grid(H, W)
    cov = face_id.long() >= 0
    c, s, tri = _faces_at(pix_f, pix_q, faces, face_id, dtype)
    if float_sign:          # (a fault for the sensitivity check: the sign from the float corners)
        a2 = (c[..., 1, 0] - c[..., 0, 0]) * (c[..., 2, 1] - c[..., 0, 1]) - (c[..., 1, 1] - c[..., 0, 1]) * (c[..., 2, 0] - c[..., 0, 0])
        s = torch.where(a2 < 0, -1.0, 1.0).to(dtype)
    Ep = edge_functions(c, s, xs.to(dtype), ys.to(dtype))
    inf = torch.tensor(float("inf"), dtype=dtype)
    out = {k: [] for k in ("pair", "k", "t", "ep", "eq", "second", "eq_min")}
    for dx, dy in NEIGH:
        nx, ny = xs + dx, ys + dy
        inside = (nx >= 0) & (nx < W) & (ny >= 0) & (ny < H)
        ncov = cov[ny.clamp(0, H - 1), nx.clamp(0, W - 1)]
        is_pair = cov & inside & ~ncov
        Eq = edge_functions(c, s, nx.to(dtype), ny.to(dtype))
        ep = Ep.clamp_min(0)
        tk = ep / (ep - Eq)
        bk = torch.full((H, W), -1, dtype=torch.long)
        bt, second = inf.expand(H, W).clone(), inf.expand(H, W).clone()
        be, bq = torch.zeros(H, W, dtype=dtype), torch.zeros(H, W, dtype=dtype)
        for k in range(3):
            cand = Eq[..., k] < 0
            better = cand & ((bk < 0) | (tk[..., k] < bt))
            second = torch.where(better, bt, torch.where(cand, torch.minimum(second, tk[..., k]), second))
            bk = torch.where(better, k, bk)
            bt = torch.where(better, tk[..., k], bt)
            be = torch.where(better, Ep[..., k], be)
            bq = torch.where(better, Eq[..., k], bq)
        bk = torch.where(is_pair, bk, -1)
        out["pair"].append(is_pair)
        out["k"].append(bk)
        out["t"].append(torch.where(bk >= 0, bt, torch.zeros_like(bt)))
        out["ep"].append(be)
        out["eq"].append(bq)
        out["second"].append(second)
        out["eq_min"].append(Eq.abs().min(-1).values)
    res = {k: torch.stack(v, -1) for k, v in out.items()}
    res["recv_q"] = (res["k"] >= 0) & ~(res["t"] < 0.5)
    res["info"] = torch.where(res["pair"], torch.where(res["k"] >= 0, res["k"] + 4 * res["recv_q"].long(), -2), -1)
    res.update(tri=tri, s=s, covered=cov)
    return res


def _to_neighbour(a, j):
    """b[q] = a[p] for q = p + NEIGH[j] (0 where no p maps; what leaves the image is dropped)"""
    dx, dy = NEIGH[j]
    H, W = a.shape
    b = torch.zeros_like(a)
    b[max(dy, 0):H + min(dy, 0), max(dx, 0):W + min(dx, 0)] = a[max(-dy, 0):H + min(-dy, 0), max(-dx, 0):W + min(-dx, 0)]
    return b


@torch.no_grad()
def alpha_aa(pr, dtype=torch.float64):
    """(alpha_aa [H, W], alpha_raw [H, W]) of the pairs `pr`: coverage plus what every pixel receives, added in the pixel's OWN neighbour
    order (a background pixel's neighbour j is the p of a pair that runs in direction j ^ 1), clamped to 0 .. 1"""
    has = pr["k"] >= 0
    contrib = torch.where(has, pr["t"].to(dtype) - 0.5, torch.zeros_like(pr["t"], dtype=dtype))
    raw = pr["covered"].to(dtype)
    for j in range(4):
        mine = torch.where(has[..., j] & ~pr["recv_q"][..., j], contrib[..., j], torch.zeros_like(raw))
        theirs = _to_neighbour(torch.where(pr["recv_q"][..., j ^ 1], contrib[..., j ^ 1], torch.zeros_like(raw)), j ^ 1)
        raw = raw + mine + theirs          # (one of the two is an exact 0: a pixel is covered or it is not)
    return raw.clamp(0, 1), raw


def alpha_autograd(pix_f, pr):
    """alpha_aa [H, W] as a differentiable function of pix_f [V, 2] with the decisions of `pr` FROZEN (which pairs, which edge, which
    receiver, which sums are clamped): what torch autograd differentiates on the CPU tests"""
    H, W = pr["covered"].shape
    idx = torch.nonzero(pr["k"] >= 0)                                            # [n, 3]: y, x, j in pixel-then-neighbour order
    y, x, j = idx[:, 0], idx[:, 1], idx[:, 2]
    k = pr["k"][y, x, j]
    tri = pr["tri"][y, x]
    u, v = pix_f[tri.gather(1, k[:, None])[:, 0]], pix_f[tri.gather(1, ((k + 1) % 3)[:, None])[:, 0]]
    s = pr["s"][y, x].to(pix_f.dtype)
    nd = torch.tensor(NEIGH)[j]
    px, py = x.to(pix_f.dtype), y.to(pix_f.dtype)
    qx, qy = (x + nd[:, 0]).to(pix_f.dtype), (y + nd[:, 1]).to(pix_f.dtype)
    E = lambda X, Y: s * ((v[:, 0] - u[:, 0]) * (Y - u[:, 1]) - (v[:, 1] - u[:, 1]) * (X - u[:, 0]))  # noqa: E731
    ep = E(px, py).clamp_min(0)
    t = ep / (ep - E(qx, qy))
    recv = torch.where(pr["recv_q"][y, x, j], (y + nd[:, 1]) * W + x + nd[:, 0], y * W + x)
    raw = pr["covered"].to(pix_f.dtype).reshape(-1).index_add(0, recv, t - 0.5).reshape(H, W)
    inside = (raw > 0) & (raw < 1)
    return torch.where(inside, raw, raw.detach().clamp(0, 1))


@torch.no_grad()
def records(pr, pix_f, alpha_raw, dL_dalpha, dtype=torch.float64, keep_clamp_gradient=False):
    """(keys [n] vertex, payload [n, 2]) of the emit pass: two records per pair with a candidate, in pixel-then-neighbour-then-corner order,
    by the closed form of the header"""
    H, W = pr["covered"].shape
    idx = torch.nonzero(pr["k"] >= 0)
    y, x, j = idx[:, 0], idx[:, 1], idx[:, 2]
    k = pr["k"][y, x, j]
    tri = pr["tri"][y, x]
    iu, iv = tri.gather(1, k[:, None])[:, 0], tri.gather(1, ((k + 1) % 3)[:, None])[:, 0]
    pf = pix_f.to(dtype)
    u, v = pf[iu], pf[iv]
    s = pr["s"][y, x].to(dtype)
    nd = torch.tensor(NEIGH)[j]
    px, py = x.to(dtype), y.to(dtype)
    qx, qy = (x + nd[:, 0]).to(dtype), (y + nd[:, 1]).to(dtype)
    recv = torch.where(pr["recv_q"][y, x, j], (y + nd[:, 1]) * W + x + nd[:, 0], y * W + x)
    raw = alpha_raw.to(dtype).reshape(-1)[recv]
    e, eq = pr["ep"][y, x, j].to(dtype), pr["eq"][y, x, j].to(dtype)
    live = (raw > 0) & (raw < 1) & ~(e < 0)
    if keep_clamp_gradient:          # (a fault for the sensitivity check)
        live = ~(e < 0)
    g = torch.where(live, dL_dalpha.to(dtype).reshape(-1)[recv], torch.zeros_like(raw))
    ep = e.clamp_min(0)
    den = ep - eq
    gp, gq = g * (-eq / (den * den)), g * (ep / (den * den))
    gu = torch.stack([s * (gp * (v[:, 1] - py) + gq * (v[:, 1] - qy)), s * (gp * (px - v[:, 0]) + gq * (qx - v[:, 0]))], 1)
    gv = torch.stack([s * (gp * (py - u[:, 1]) + gq * (qy - u[:, 1])), s * (gp * (u[:, 0] - px) + gq * (u[:, 0] - qx))], 1)
    return torch.stack([iu, iv], 1).reshape(-1), torch.stack([gu, gv], 1).reshape(-1, 2)


@torch.no_grad()
def reduce_records(keys, payload, V, dtype=torch.float64):
    """dL_dpix [V, 2]: the records of every vertex, in record order (the sort is stable), summed in the kernel's order (RF.list_sum)"""
    n = keys.numel()
    if n == 0:
        return torch.zeros(V, 2, dtype=dtype), torch.zeros(V, dtype=torch.long)
    order = torch.sort(keys, stable=True).indices
    length = torch.bincount(keys, minlength=V)
    start = torch.cumsum(length, 0) - length
    table = torch.full((V, max(int(length.max()), 1)), -1, dtype=torch.long)
    table[keys[order], torch.arange(n) - start[keys[order]]] = order
    return RF.list_sum(table, torch.ones(n, dtype=dtype), payload.to(dtype), dtype), length


def alpha_backward(pr, pix_f, alpha_raw, dL_dalpha, V, dtype=torch.float64, **kw):
    keys, payload = records(pr, pix_f, alpha_raw, dL_dalpha, dtype, **kw)
    return reduce_records(keys, payload, V, dtype)


# ---- projection -------------------------------------------------------------------------------------------------------------------------
def project_pix(verts, cam, dtype=torch.float64):
    """pix_f [V, 2]: the statements of mesh_render_ref.project, differentiable in `verts`"""
    p = verts.to(dtype)
    P = cam.full_proj.to(dtype)
    x, y, z = p[:, 0], p[:, 1], p[:, 2]
    hx = x * P[0, 0] + y * P[1, 0] + z * P[2, 0] + P[3, 0]
    hy = x * P[0, 1] + y * P[1, 1] + z * P[2, 1] + P[3, 1]
    hw = x * P[0, 3] + y * P[1, 3] + z * P[2, 3] + P[3, 3]
    pw = 1.0 / (hw + torch.tensor(1e-7, dtype=dtype))
    return torch.stack([((hx * pw + 1) * cam.width - 1) * 0.5, ((hy * pw + 1) * cam.height - 1) * 0.5], 1)


@torch.no_grad()
def project_bwd(verts, cam, marked, dL_dpix, dtype=torch.float64, eps=1e-7):
    """dL_dverts [V, 3] by the explicit chain of the kernel; exact zeros on marked vertices"""
    p, g = verts.to(dtype), dL_dpix.to(dtype)
    P = cam.full_proj.to(dtype)
    x, y, z = p[:, 0], p[:, 1], p[:, 2]
    hx = x * P[0, 0] + y * P[1, 0] + z * P[2, 0] + P[3, 0]
    hy = x * P[0, 1] + y * P[1, 1] + z * P[2, 1] + P[3, 1]
    hw = x * P[0, 3] + y * P[1, 3] + z * P[2, 3] + P[3, 3]
    pw = 1.0 / (hw + torch.tensor(eps, dtype=dtype))
    gx, gy = g[:, 0] * (0.5 * cam.width), g[:, 1] * (0.5 * cam.height)
    ghx, ghy = gx * pw, gy * pw
    ghw = -(gx * hx + gy * hy) * (pw * pw)
    out = torch.stack([ghx * P[r, 0] + ghy * P[r, 1] + ghw * P[r, 3] for r in range(3)], 1)
    return torch.where(marked[:, None], torch.zeros_like(out), out)


# ---- smoothness -------------------------------------------------------------------------------------------------------------------------
def smooth_energy(d, faces):
    """sum over faces and their 3 edges of |d_a - d_b|^2 / (3 F), differentiable in d"""
    t = d[faces.long()]
    e = t - t.roll(-1, 1)
    return (e * e).sum() / (3.0 * faces.shape[0])


@torch.no_grad()
def smooth_grad(d, faces, dtype=torch.float64):
    """(2 / (3F)) x the sum over every vertex's corners, in ascending corner order, of 2 d_i - d_j - d_k"""
    V, F = d.shape[0], faces.shape[0]
    dd, f = d.to(dtype), faces.long()
    corner_vert = f.reshape(-1)
    order = torch.sort(corner_vert, stable=True).indices                        # every vertex's corners, ascending
    length = torch.bincount(corner_vert, minlength=V)
    start = torch.cumsum(length, 0) - length
    L = max(int(length.max()), 1)
    term = 2.0 * dd[f] - dd[f].roll(-1, 1) - dd[f].roll(-2, 1)                  # [F, 3, 3] by corner: 2 d_i - d_j - d_k
    term = term.reshape(-1, 3)
    table = torch.full((V, L), -1, dtype=torch.long)
    table[corner_vert[order], torch.arange(3 * F) - start[corner_vert[order]]] = order
    acc = torch.zeros(V, 3, dtype=dtype)
    for i in range(L):                                                           # left to right, as one thread adds them
        col = table[:, i]
        acc = acc + torch.where((col >= 0)[:, None], term[col.clamp_min(0)], torch.zeros_like(acc))
    return torch.tensor(2.0 / (3.0 * F), dtype=dtype) * acc


# ---- one view and the loop --------------------------------------------------------------------------------------------------------------
@torch.no_grad()
def view_forward(verts, faces, cam, dtype=torch.float64, given=None, bits=8):
    """dict(alpha_aa, alpha_raw, face_id, pairs, pix_f, marked) of one view.  `given` = (pix_f, pix_q, face_id) feeds a kernel's own
    decisions; without it the projection is mesh_render_ref.project's in `dtype` and the coverage mesh_render_ref.rasterize's."""
    if given is None:
        pj = M.project(verts, cam, bits, dtype)
        r = M.rasterize(pj["pix_q"], pj["zv"], faces, torch.zeros(verts.shape[0], 3), cam.width, cam.height, [0.0, 0.0, 0.0], bits=bits, cull=True,
                        dtype=dtype)
        pix_f, pix_q, face_id = pj["pix_f"], pj["pix_q"], r["face_id"]
    else:
        pix_f, pix_q, face_id = given
    pr = pairs(pix_f, pix_q, faces, face_id, dtype)
    a, raw = alpha_aa(pr, dtype)
    return dict(alpha_aa=a, alpha_raw=raw, face_id=face_id, pairs=pr, pix_f=pix_f, marked=pix_q.long()[:, 0] == M.MARK)


@torch.no_grad()
def view_backward(verts, cam, fwd, dL_dalpha, dtype=torch.float64):
    g_pix, length = alpha_backward(fwd["pairs"], fwd["pix_f"], fwd["alpha_raw"], dL_dalpha, verts.shape[0], dtype)
    return project_bwd(verts, cam, fwd["marked"], g_pix, dtype), g_pix, length


def fit(verts, faces, cams, targets, iterations, lr, lambda_offset=LAMBDA_OFFSET, lambda_smooth=LAMBDA_SMOOTH, seed=0, dtype=torch.float64,
        given=None):
    """The loop of fit_vertices: dict(verts, d, loss_first, loss_last, mse_before, mse_after (summed over the views), iou_before, iou_after
    (mean), max_offset).  `given`: a function (step, view, verts) -> (pix_f, pix_q, face_id) that feeds a kernel's decisions."""
    v0 = verts.to(dtype)
    V, F = v0.shape[0], faces.shape[0]
    d = torch.zeros_like(v0, requires_grad=True)
    opt = torch.optim.Adam([d], lr=lr)
    tg = [t.to(dtype) for t in targets]

    def measure(v):
        mse, iou = 0.0, []
        for cam, t in zip(cams, tg):
            fw = view_forward(v, faces, cam, dtype)
            mse += float(((fw["alpha_aa"] - t) ** 2).mean())
            a, b = fw["face_id"] >= 0, t >= 0.5
            iou.append(float((a & b).sum()) / max(float((a | b).sum()), 1.0))
        return mse, sum(iou) / len(iou)

    before = measure(v0)
    first = last = None
    for it, j in enumerate(RF.view_schedule(len(cams), iterations, seed)):
        v = (v0 + d.detach()).to(dtype)
        fw = view_forward(v, faces, cams[j], dtype, None if given is None else given(it, j, v))
        diff = fw["alpha_aa"] - tg[j]
        dd = d.detach()
        loss = float((diff * diff).mean() + lambda_offset * (dd * dd).sum(1).mean() + lambda_smooth * smooth_energy(dd, faces))
        first, last = (loss if it == 0 else first), loss
        g_verts, _, _ = view_backward(v, cams[j], fw, diff * (2.0 / diff.numel()), dtype)
        d.grad = g_verts + lambda_offset * (2.0 / V) * dd + lambda_smooth * smooth_grad(dd, faces, dtype)
        opt.step()
    out = (v0 + d.detach())
    after = measure(out)
    return dict(verts=out, d=d.detach(), loss_first=first, loss_last=last, mse_before=before[0], mse_after=after[0], iou_before=before[1],
                iou_after=after[1], max_offset=float(d.detach().norm(dim=1).max()))


# ---- hand-placed scenes -----------------------------------------------------------------------------------------------------------------
def snap(pix_f, bits=8):
    return torch.round(pix_f.double() * (1 << bits)).long()


def _raster(pix_f, faces, W, H, pix_q=None):
    q = snap(pix_f) if pix_q is None else pix_q
    r = M.rasterize(q, torch.ones(pix_f.shape[0]), faces, torch.zeros(pix_f.shape[0], 3), W, H, [0.0, 0.0, 0.0], cull=True)
    return q, r["face_id"]


def needle(W=16, H=12):
    """A front face 0.6 px wide at its top and 8 px long over the pixel centres of column 5, rows 2 .. 9, background left and right.  A pair
    takes at most 0.5, so a pixel of the column with two background neighbours keeps a sum of 0.1 .. 0.55; the pixel at the tip, (5, 9), has
    three, loses 0.49 + 0.49 + 0.2, and its sum of -0.18 clamps to 0: its gradient must be exactly 0.
    (pix_f [3, 2] float32, pix_q, faces, face_id)"""
    pix_f = torch.tensor([[4.71, 1.4], [5.0, 9.3], [5.31, 1.4]])      # negative doubled area: a front face
    faces = torch.tensor([[0, 1, 2]])
    q, fid = _raster(pix_f, faces, W, H)
    return pix_f, q, faces, fid


def dot(W=12, H=10):
    """A front face over the one pixel centre (5, 4) that nearly reaches its four neighbours: the receivers are background pixels, sums < 1"""
    pix_f = torch.tensor([[3.9, 3.3], [5.05, 4.9], [6.1, 3.2]])
    faces = torch.tensor([[0, 1, 2]])
    q, fid = _raster(pix_f, faces, W, H)
    return pix_f, q, faces, fid


def no_candidate(W=8, H=6):
    """Two faces with hand-set positions and a hand-set face_id: pixel (2, 2) is given to face 0, whose float corners contain BOTH (2, 2)
    and its right neighbour (3, 2), which face_id leaves uncovered: every E_k(q) is positive, the pair has no candidate and contributes
    nothing.  Pixel (5, 3) belongs to face 1 with ordinary pairs."""
    pix_f = torch.tensor([[0.5, 0.5], [2.5, 4.5], [4.5, 0.5], [4.6, 2.4], [5.1, 3.9], [5.6, 2.5]])
    faces = torch.tensor([[0, 1, 2], [3, 4, 5]])
    fid = torch.full((H, W), -1, dtype=torch.long)
    fid[2, 2] = 0
    fid[3, 5] = 1
    return pix_f, snap(pix_f), faces, fid


def negative_ep(W=8, H=6):
    """Pixels (3, 1 .. 3) are given to a face whose float edge 0 leaves them 0.1 px OUTSIDE (E_0(p) < 0) although face_id says covered, as
    happens when snapping moves an edge across a centre: towards the left neighbour Ep clamps to 0, t = 0, the pixel loses 0.5 and no
    gradient flows from that pair.  Pixel (3, 2) has that pair alone: its sum is 0.5, inside (0, 1), so the zero is the clamp of Ep's."""
    pix_f = torch.tensor([[3.1, 0.5], [3.1, 4.5], [6.0, 2.0]])          # edge 0 runs down the line x = 3.1; the pixels of column 3 lie left of it
    faces = torch.tensor([[0, 1, 2]])
    fid = torch.full((H, W), -1, dtype=torch.long)
    fid[1:4, 3] = 0
    fid[2, 4] = 0
    return pix_f, snap(pix_f), faces, fid


def exact_half(W=8, H=6):
    """Dyadic coordinates: the vertical edge x = 3.5 lies exactly half way between p = (3, 2) and q = (4, 2): t = 0.5 in every format, and
    the receiver is q (the rule is t < 0.5 for p)."""
    pix_f = torch.tensor([[3.5, 0.0], [3.5, 4.0], [0.75, 2.25]])
    faces = torch.tensor([[0, 2, 1]])
    q, fid = _raster(pix_f, faces, W, H)
    return pix_f, q, faces, fid


def on_edge(W=8, H=6):
    """Dyadic coordinates: the face's right edge is the line x = 4, through the pixel centres of column 4, which the fill rule leaves
    uncovered (a right edge owns nothing).  For p = (3, 2) and q = (4, 2), E_2(q) is exactly 0 and q lies inside the two other edges: the
    candidate test is E_k(q) < 0, so this pair has no candidate and contributes nothing."""
    pix_f = torch.tensor([[4.0, 0.0], [4.0, 4.0], [0.75, 2.25]])
    faces = torch.tensor([[0, 2, 1]])
    q, fid = _raster(pix_f, faces, W, H)
    return pix_f, q, faces, fid


def edge_tie(W=8, H=6):
    """Dyadic coordinates: a front face with its apex at (3.25, 2), on the row of p = (3, 2), and its two slanted edges (k = 1 and k = 2)
    mirror images about that row: towards q = (4, 2) both are candidates with the same Ep and the same E(q), so the same t = 0.25 bit
    for bit, and the lower k wins."""
    pix_f = torch.tensor([[1.25, 0.0], [1.25, 4.0], [3.25, 2.0]])
    faces = torch.tensor([[0, 1, 2]])
    q, fid = _raster(pix_f, faces, W, H)
    return pix_f, q, faces, fid


def sliver(W=8, H=6):
    """A face whose float corners have a NEGATIVE doubled area (-2e-3) and whose hand-set snapped corners a positive one (+1280): s must
    come from the snapped corners (+1).  face_id gives it pixel (3, 2)."""
    pix_f = torch.tensor([[1.0, 2.001], [6.0, 2.001], [3.5, 2.0006]])
    pix_q = torch.tensor([[256, 512], [1536, 512], [896, 513]])
    faces = torch.tensor([[0, 1, 2]])
    fid = torch.full((H, W), -1, dtype=torch.long)
    fid[2, 3] = 0
    return pix_f, pix_q, faces, fid


HAND_SCENES = {"needle": needle, "dot": dot, "no_candidate": no_candidate, "negative_ep": negative_ep, "exact_half": exact_half,
               "on_edge": on_edge, "edge_tie": edge_tie, "sliver": sliver}
