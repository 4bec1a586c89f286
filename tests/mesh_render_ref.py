"""Pure-torch restatement of csrc_recon/meshrast.hip (test oracle) and the scenes of tests/test_mesh_render_{cpu,gpu}.py.  It evaluates
every drawn face on every pixel: no tiles, no lists, no early exit (tile_list restates one tile's list, for the premises of the scenes
that are about batches).

Projection: the statements of mesh_project_kernel in fp64 (default) or float32.  Rasterization: takes the SNAPPED integer positions and the
view z of the vertices; drawn / not drawn, coverage, the fill rule and n_hit come from int64 arithmetic alone and are exact, z and colour are
fp64 (or float32: what that run loses against the fp64 one is the cost of the number format)."""
from __future__ import annotations

import math

import numpy as np
import torch

import gs_dense_ref as D

MARK = -2 ** 31
Q_LIMIT = 2.0 ** 28
INT_FAR = 2 ** 62          # above every face index
ZNEAR = 0.2


# ---- projection -----------------------------------------------------------------------------------------------------------------------
@torch.no_grad()
def project(verts, cam, bits=8, dtype=torch.float64):
    """dict(zv [V], pix_f [V, 2], pix_q [V, 2] int64 (MARK on marked vertices), marked [V] bool) of vertices [V, 3] in `dtype`"""
    p = verts.to(dtype)
    V, P = cam.world_view.to(dtype), cam.full_proj.to(dtype)
    x, y, z = p[:, 0], p[:, 1], p[:, 2]
    zv = x * V[0, 2] + y * V[1, 2] + z * V[2, 2] + V[3, 2]
    hx = x * P[0, 0] + y * P[1, 0] + z * P[2, 0] + P[3, 0]
    hy = x * P[0, 1] + y * P[1, 1] + z * P[2, 1] + P[3, 1]
    hw = x * P[0, 3] + y * P[1, 3] + z * P[2, 3] + P[3, 3]
    pw = 1.0 / (hw + torch.tensor(1e-7, dtype=dtype))
    fx, fy = ((hx * pw + 1) * cam.width - 1) * 0.5, ((hy * pw + 1) * cam.height - 1) * 0.5
    S = float(1 << bits)
    sx, sy = torch.round(fx * S), torch.round(fy * S)                       # (round half to even, as rintf)
    ok = (zv > torch.tensor(ZNEAR, dtype=torch.float32).to(dtype)) & (sx.abs() < Q_LIMIT) & (sy.abs() < Q_LIMIT)        # (false on NaN and infinity)
    q = torch.stack([torch.where(ok, sx, torch.zeros_like(sx)), torch.where(ok, sy, torch.zeros_like(sy))], 1).long()
    q[~ok] = MARK
    return dict(zv=zv, pix_f=torch.stack([fx, fy], 1), pix_q=q, marked=~ok)


# ---- rasterization --------------------------------------------------------------------------------------------------------------------
def _floor_div(a, b):
    return torch.div(a, b, rounding_mode="floor")


def _rects(c, W, H, bits):
    """(x0, y0, x1, y1) [F] int64: the pixel centres inside the bounding box of corners c [F, 3, 2], clamped to the image (empty: x0 > x1 or y0 > y1)"""
    S = 1 << bits
    lo, hi = c.min(1).values, c.max(1).values
    x0, y0 = (-_floor_div(-lo[:, 0], S)).clamp_min(0), (-_floor_div(-lo[:, 1], S)).clamp_min(0)       # first pixel centre at or after the box
    x1, y1 = _floor_div(hi[:, 0], S).clamp_max(W - 1), _floor_div(hi[:, 1], S).clamp_max(H - 1)
    return x0, y0, x1, y1


@torch.no_grad()
def drawn_faces(pix_q, faces, W, H, bits, cull):
    """(drawn [F] bool, area2 [F] int64, corners [F, 3, 2] int64 with marked ones zeroed, tiles [F] int64: 16 x 16 tiles under the clamped box)"""
    q = pix_q.long()
    f = faces.long()
    marked = q[:, 0] == MARK
    usable = ~marked[f].any(1)
    c = torch.where(usable[:, None, None], q[f], torch.zeros(1, dtype=torch.long))
    a, b, cc = c[:, 0], c[:, 1], c[:, 2]
    area2 = (b[:, 0] - a[:, 0]) * (cc[:, 1] - a[:, 1]) - (b[:, 1] - a[:, 1]) * (cc[:, 0] - a[:, 0])
    x0, y0, x1, y1 = _rects(c, W, H, bits)
    box = (x0 <= x1) & (y0 <= y1)
    drawn = usable & (area2 != 0) & box
    if cull:
        drawn &= area2 < 0                                                                               # front faces: negative doubled area
    tiles = (_floor_div(x1, 16) - _floor_div(x0, 16) + 1) * (_floor_div(y1, 16) - _floor_div(y0, 16) + 1)
    return drawn, area2, c, torch.where(drawn, tiles, torch.zeros_like(tiles))


@torch.no_grad()
def tile_list(pix_q, zv, faces, W, H, bits=8, cull=False, tile=(0, 0)):
    """(face indices [n] int64, zmin [n] float32) of one 16 x 16 tile's list in the kernel's order: the drawn faces whose clamped box meets
    the tile, by the float32 zmin (the smallest corner depth), equal zmin in face order (the sort is stable)"""
    drawn, _, c, _ = drawn_faces(pix_q, faces, W, H, bits, cull)
    x0, y0, x1, y1 = _rects(c, W, H, bits)
    tx, ty = tile
    on = drawn & (_floor_div(x0, 16) <= tx) & (tx <= _floor_div(x1, 16)) & (_floor_div(y0, 16) <= ty) & (ty <= _floor_div(y1, 16))
    idx = torch.nonzero(on).reshape(-1)
    zmin = zv.float()[faces.long()[idx]].min(1).values
    order = torch.sort(zmin, stable=True).indices
    return idx[order], zmin[order]


def _owns(dx, dy):
    """the top-left rule on an edge of a face whose inside has positive edge functions (y down): left edges run towards smaller y, top edges
    are horizontal and run towards larger x"""
    return (dy < 0) | ((dy == 0) & (dx > 0))


@torch.no_grad()
def rasterize(pix_q, zv, faces, colors, W, H, bg, bits=8, cull=True, dtype=torch.float64):
    """dict(face_id [H, W] (-1: nothing), alpha, n_hit, depth, image [3, H, W], gap [H, W]: z of the second nearest hit minus z of the nearest
    (inf with fewer than two hits), drawn [F], tiles [F])"""
    drawn_all, area2, c, tiles = drawn_faces(pix_q, faces, W, H, bits, cull)
    # only the drawn faces are evaluated on the pixels (an undrawn face covers nothing): `keep` maps their rows back to face indices
    keep = torch.nonzero(drawn_all).reshape(-1)
    if keep.numel() == 0:                                              # (one row that covers nothing keeps the shapes below)
        keep = torch.zeros(1, dtype=torch.long)
    faces, area2, c, drawn = faces[keep], area2[keep], c[keep], drawn_all[keep]
    F = faces.shape[0]
    S = 1 << bits
    ys, xs = torch.meshgrid(torch.arange(H, dtype=torch.long), torch.arange(W, dtype=torch.long), indexing="ij")
    Px, Py = (xs.reshape(1, -1) * S), (ys.reshape(1, -1) * S)
    s = torch.where(area2 < 0, -1, 1)[:, None]
    ax, ay, bx, by, cx, cy = (c[:, k, d][:, None] for k in range(3) for d in range(2))

    def edge(ux, uy, vx, vy):         # edge function of u -> v at the pixel centres, oriented; and whether a zero on it counts
        e = s * ((vx - ux) * (Py - uy) - (vy - uy) * (Px - ux))
        return e, e >= torch.where(_owns(s * (vx - ux), s * (vy - uy)), 0, 1)

    e0, in0 = edge(bx, by, cx, cy)
    e1, in1 = edge(cx, cy, ax, ay)
    e2, in2 = edge(ax, ay, bx, by)
    cover = drawn[:, None] & in0 & in1 & in2
    n_hit = cover.sum(0)
    z3 = zv.to(dtype)[faces.long()]                                   # [F, 3]
    fa = (e0 + e1 + e2).to(dtype)
    fa = torch.where(fa == 0, torch.ones_like(fa), fa)
    b0, b1, b2 = e0.to(dtype) / fa, e1.to(dtype) / fa, e2.to(dtype) / fa
    z = 1.0 / (b0 / z3[:, 0:1] + b1 / z3[:, 1:2] + b2 / z3[:, 2:3])
    z = torch.minimum(torch.maximum(z, z3.min(1, keepdim=True).values), z3.max(1, keepdim=True).values)
    inf = torch.tensor(float("inf"), dtype=dtype)
    z = torch.where(cover, z, inf)
    best = z.min(0).values
    win = torch.where(cover & (z == best[None]), keep[:, None], INT_FAR).min(0).values         # nearest; on equal z the lower face index
    row = torch.where(cover & (z == best[None]) & (keep[:, None] == win[None]), torch.arange(F)[:, None], 0).sum(0)      # its row
    hit = n_hit > 0
    g = lambda t: t.gather(0, row[None])[0]  # noqa: E731
    wb = [g(b0), g(b1), g(b2)]
    wi = faces.long()[row]                                             # [P, 3]
    col = colors.to(dtype)
    zz = zv.to(dtype)
    acc = sum((wb[k] / zz[wi[:, k]])[:, None] * col[wi[:, k]] for k in range(3))
    bgt = torch.as_tensor(bg, dtype=dtype)
    image = torch.where(hit[:, None], torch.where(hit, best, torch.zeros_like(best))[:, None] * acc, bgt[None])
    two = torch.topk(z, min(2, F), dim=0, largest=False).values
    gap = (two[1] - two[0]) if F > 1 else torch.full_like(best, float("inf"))
    gap = torch.where(n_hit >= 2, gap, inf)
    return dict(face_id=torch.where(hit, win, -1).reshape(H, W), alpha=hit.to(dtype).reshape(H, W), n_hit=n_hit.reshape(H, W),
                depth=torch.where(hit, best, torch.zeros_like(best)).reshape(H, W), image=image.t().reshape(3, H, W), gap=gap.reshape(H, W),
                drawn=drawn_all, tiles=tiles)


# ---- meshes ---------------------------------------------------------------------------------------------------------------------------
def icosphere(subdiv=2, radius=0.5, centre=(0.0, 0.0, 0.0), seed=None):
    """(verts [V, 3] float32, faces [F, 3] int64 wound counter-clockwise seen from outside): 20 * 4^subdiv faces, randomly rotated by `seed`"""
    t = (1.0 + math.sqrt(5.0)) / 2.0
    v = [(-1, t, 0), (1, t, 0), (-1, -t, 0), (1, -t, 0), (0, -1, t), (0, 1, t), (0, -1, -t), (0, 1, -t), (t, 0, -1), (t, 0, 1), (-t, 0, -1), (-t, 0, 1)]
    f = [(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6), (7, 1, 8), (3, 9, 4), (3, 4, 2),
         (3, 2, 6), (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10), (8, 6, 7), (9, 8, 1)]
    v = [np.asarray(p, dtype=np.float64) / math.sqrt(1 + t * t) for p in v]
    for _ in range(subdiv):
        mid, nf = {}, []

        def m(i, j):
            key = (min(i, j), max(i, j))
            if key not in mid:
                p = v[i] + v[j]
                v.append(p / np.linalg.norm(p))
                mid[key] = len(v) - 1
            return mid[key]

        for a, b, c in f:
            ab, bc, ca = m(a, b), m(b, c), m(c, a)
            nf += [(a, ab, ca), (b, bc, ab), (c, ca, bc), (ab, bc, ca)]
        f = nf
    v = np.stack(v)
    if seed is not None:
        g = torch.Generator().manual_seed(seed)
        Q, _ = np.linalg.qr(torch.randn(3, 3, generator=g, dtype=torch.float64).numpy())
        if np.linalg.det(Q) < 0:
            Q[:, 0] = -Q[:, 0]
        v = v @ Q.T
    verts = torch.from_numpy(radius * v + np.asarray(centre, dtype=np.float64)[None]).float()
    return verts, torch.tensor(f, dtype=torch.long)


def position_colors(verts, tint=(1.0, 1.0, 1.0)):
    return ((0.5 + 0.6 * verts).clamp(0, 1) * torch.tensor(tint)).float()


def mesh_scene(kind, seed):
    """(verts, faces, colors): "sphere" = one icosphere of 320 faces; "pair" = two interpenetrating icospheres of different colour"""
    if kind == "sphere":
        v, f = icosphere(2, 0.5, (0.03, -0.02, 0.04), seed)
        return v, f, position_colors(v)
    v1, f1 = icosphere(2, 0.4, (-0.12, 0.1, 0.0), seed)
    v2, f2 = icosphere(2, 0.33, (0.2, -0.12, 0.1), seed + 1)
    return torch.cat([v1, v2]), torch.cat([f1, f2 + v1.shape[0]]), torch.cat([position_colors(v1, (1.0, 0.5, 0.3)), position_colors(v2, (0.3, 0.6, 1.0))])


SIZES = ((64, 48), (56, 40), (72, 24))
# (kind, seed, W, H, view of cams_for, cull).  Seeds: for each kind the first seed counted up from 1 for which every case below keeps
# Z_GAP_MARGIN on the restatement alone (tests/test_mesh_render_cpu.py::test_scenes_keep_their_depth_margin); SEEDS_TRIED says how many were
# tried (seed 1 held it for both kinds).
SEEDS = {"sphere": 1, "pair": 1}
SEEDS_TRIED = {"sphere": 1, "pair": 1}
RASTER_CASES = tuple((kind, SEEDS[kind], W, H, view, cull) for kind in ("sphere", "pair") for (W, H), view in zip(SIZES, (0, 1, 3))
                     for cull in (True, False))
# The two nearest hits of a pixel keep their fp64 order in fp32 when they differ by more than both roundings.  z is ~2.3 at most here (ulp
# 2.4e-7) and comes from three quotients of rounded int64 edge functions, three divisions, two additions and a reciprocal; the float32 run of
# the restatement is off by 2.1e-7 .. 2.6e-7 on these cases, and the CPU test holds it below Z_FP32_ERR (two ulp).  The margin is 8 x that,
# like the depth-order margin of the splat scenes (gs_dense_ref.DEPTH_GAP_MARGIN is 4 x).  The smallest gap of the chosen cases is 2.7e-3.
Z_FP32_ERR = 5e-7
Z_GAP_MARGIN = 4e-6


def case_id(case):
    return f"{case[0]}{case[1]}-{case[2]}x{case[3]}-v{case[4]}-{'cull' if case[5] else 'nocull'}"


def case_camera(case):
    return D.cams_for(case[2], case[3])[case[4]]


# ---- pixel-aligned quad grid (fill rule) ----------------------------------------------------------------------------------------------
def quad_grid(bits=8, x0=3, y0=2, step=(5, 3, 7, 4), rows=(4, 6, 3), split=0, flip=False):
    """Snapped positions [V, 2] int64 exactly on pixel centres, faces [F, 3], and the pixel rectangle (x0, y0, x1, y1) the grid spans: columns
    of widths `step` and rows of heights `rows` (pixels), each quad cut into two triangles along one diagonal (split 0 / 1, 2 = alternating),
    `flip` reverses every winding."""
    xs = np.concatenate([[x0], x0 + np.cumsum(step)])
    ys = np.concatenate([[y0], y0 + np.cumsum(rows)])
    nx = len(xs)
    q = torch.tensor([[x << bits, y << bits] for y in ys for x in xs], dtype=torch.long)
    faces = []
    for j in range(len(ys) - 1):
        for i in range(nx - 1):
            a, b, c, d = j * nx + i, j * nx + i + 1, (j + 1) * nx + i + 1, (j + 1) * nx + i
            cut = split if split < 2 else (i + j) % 2
            tris = [(a, b, c), (a, c, d)] if cut == 0 else [(a, b, d), (b, c, d)]
            faces += [t[::-1] for t in tris] if flip else tris
    return q, torch.tensor(faces, dtype=torch.long), (int(xs[0]), int(ys[0]), int(xs[-1]), int(ys[-1]))


# ---- stacked layers (long lists, early exit) ------------------------------------------------------------------------------------------
LAYERS = 700


def layer_stack(bits=8, n=LAYERS, seed=0):
    """n triangles that each cover the whole first tile (corners at pixels (-1, -1), (34, -1), (-1, 34)), stacked 1e-3 apart in view z in a
    shuffled order (the nearest is face n - 5) and tilted by less than 2e-4, so they never meet; one colour per layer.  (pix_q [3n, 2], zv [3n], faces [n, 3], colors)"""
    g = torch.Generator().manual_seed(seed)
    order = torch.randperm(n, generator=g)
    i = int(torch.nonzero(order == 0)[0])
    order[i], order[n - 5] = order[n - 5].clone(), order[i].clone()         # the nearest layer is face n - 5: in the last batch of face order
    corner = torch.tensor([[-1, -1], [34, -1], [-1, 34]], dtype=torch.long) << bits
    q = corner.repeat(n, 1)
    zv = (1.0 + 1e-3 * order.double())[:, None] + 2e-4 * torch.rand(n, 3, generator=g, dtype=torch.float64)
    colors = torch.rand(n, 1, 3, generator=g).expand(n, 3, 3)
    return q, zv.reshape(-1).float(), torch.arange(3 * n).reshape(n, 3), colors.reshape(-1, 3).contiguous().float()


# ---- bit-equal depths (the tie rule) --------------------------------------------------------------------------------------------------
def tie_pair(bits=8, swap=False):
    """Two faces over the same three snapped corners with the same three view depths (so every pixel they share gets bit-equal z from both),
    red and blue; `swap` gives them in the other order.  (pix_q [6, 2], zv [6], faces [2, 3], colors [6, 3])"""
    tri = torch.tensor([[5 << bits, (3 << bits) + 7], [(40 << bits) + 100, 9 << bits], [(12 << bits) + 33, (30 << bits) + 5]], dtype=torch.long)
    z = torch.tensor([1.7, 2.1, 1.9])
    red, blue = torch.tensor([[1.0, 0.1, 0.1]]).expand(3, 3), torch.tensor([[0.1, 0.1, 1.0]]).expand(3, 3)
    cols = torch.cat([blue, red] if swap else [red, blue])
    return tri.repeat(2, 1), z.repeat(2), torch.arange(6).reshape(2, 3), cols.contiguous()


# ---- faces that are not drawn ---------------------------------------------------------------------------------------------------------
def undrawn_mesh(cam):
    """A world-space mesh of faces none of which is drawn from `cam` (an orbit camera at distance 2 looking at the origin): one with a corner
    behind the z = 0.2 plane, one with a corner behind the camera, one wholly outside the image, one with a repeated vertex, one with three
    collinear corners that snap onto one line.  (verts, faces, colors, names)"""
    eye = cam.center.double()
    fwd = -eye / eye.norm()
    right = torch.linalg.cross(fwd, torch.tensor([0.0, 0.0, 1.0], dtype=torch.float64))
    right = right / right.norm()
    down = torch.linalg.cross(fwd, right)
    at = lambda x, y, z: eye + x * right + y * down + z * fwd  # noqa: E731  (view coordinates -> world)
    v = [at(-0.3, 0.1, 1.5), at(0.3, -0.1, 1.5), at(0.0, 0.02, 0.15),          # a corner at z = 0.15 <= 0.2
         at(-0.3, 0.1, 1.5), at(0.3, -0.1, 1.5), at(0.0, 0.1, -0.5),           # a corner behind the camera
         at(5.0, 0.0, 2.0), at(6.0, 0.1, 2.0), at(5.5, 1.0, 2.0),              # wholly to the right of the image
         at(-0.2, 0.0, 2.0), at(0.2, 0.2, 2.0),                                # + a repeated vertex
         at(0.0, 0.0, 2.0), at(0.0, 0.0, 1.0), at(0.0, 0.0, 3.0)]              # all three on the optical axis: one pixel position
    faces = torch.tensor([[0, 1, 2], [3, 4, 5], [6, 7, 8], [9, 10, 10], [11, 12, 13]], dtype=torch.long)
    verts = torch.stack(v).float()
    return verts, faces, position_colors(verts), ("near", "behind", "outside", "repeated", "collinear")


# ---- sub-pixel depths and ragged images -----------------------------------------------------------------------------------------------
# (kind, seed, W, H, view of cams_for, cull, subpixel_bits).  Sizes: odd, narrower or lower than one 16-pixel tile, and a single pixel.
# Seeds: per case the first seed counted up from 1 for which the restatement alone keeps Z_GAP_MARGIN on every pixel
# (tests/test_mesh_render_cpu.py::test_edge_scenes_keep_their_depth_margin also holds that every smaller seed breaks it); EDGE_SEEDS_TRIED
# says how many were tried.  At 0 and 1 bits vertices snap onto each other and faces near the silhouette fold over their neighbours: a pixel
# centre on the edge two such faces share gets the same depth from both up to rounding, and which wins is the number format's choice.
# With culling off no seed up to 20 avoids that at 37 x 21 and 0 bits (from none of the four views, for neither scene): that case is listed
# in EDGE_EXCLUDING, face_id, depth and colour are compared on the pixels that keep the margin, alpha and n_hit on all, and the pixels left
# out may be EXCLUDE_MAX of the covered ones at most; its seed is the first that stays within that (1 of 163 covered pixels is left out).
EDGE_SIZES = ((37, 21), (17, 50), (13, 9), (1, 1))
EDGE_BITS = (0, 1, 4, 7)
EDGE_CASES = (
    ("pair", 1, 37, 21, 0, False, 0), ("sphere", 1, 37, 21, 1, True, 0), ("pair", 1, 17, 50, 1, False, 0), ("sphere", 2, 13, 9, 0, False, 0),
    ("sphere", 1, 1, 1, 0, False, 0),
    ("sphere", 4, 37, 21, 0, False, 1), ("pair", 1, 17, 50, 3, False, 1), ("pair", 1, 13, 9, 2, True, 1), ("sphere", 1, 1, 1, 2, True, 1),
    ("pair", 2, 37, 21, 2, False, 4), ("sphere", 1, 17, 50, 2, False, 4), ("pair", 1, 13, 9, 3, True, 4), ("sphere", 1, 1, 1, 1, False, 4),
    ("pair", 1, 37, 21, 1, False, 7), ("sphere", 1, 13, 9, 0, True, 7), ("pair", 1, 17, 50, 2, False, 7), ("sphere", 1, 37, 21, 3, True, 7),
)
EXCLUDE_MAX = 0.02
SEED_LIMIT = 20


def edge_case_id(case):
    return f"{case_id(case[:6])}-b{case[6]}"


def any_case_id(case):
    return edge_case_id(case) if len(case) > 6 else case_id(case)


def case_bits(case):
    return case[6] if len(case) > 6 else 8


EDGE_EXCLUDING = ("pair1-37x21-v0-nocull-b0",)
EDGE_SEEDS_TRIED = {edge_case_id(case): (SEED_LIMIT if edge_case_id(case) in EDGE_EXCLUDING else case[1]) for case in EDGE_CASES}
# the single pixel: its centre is at (0, 0), and at 0 and 1 bits every vertex in view snaps onto it or next to it, so no face with an area
# covers it; at 4 bits the sphere does
EDGE_SINGLE_PIXEL_COVERED = {0: False, 1: False, 4: True}
# the cases the refinement's tests run as well (tests/test_mesh_refine_gpu.py): 0 and 4 bits on an odd size each, and 7
REFINE_EDGE_CASES = tuple(EDGE_CASES[i] for i in (1, 3, 9, 11, 16))


def compared_pixels(ref, case=None):
    """[H, W] bool: the pixels on which face_id, depth and colour are compared, and how many covered pixels that leaves out.  Every pixel,
    unless the case is one of EDGE_EXCLUDING: then those whose two nearest hits keep Z_GAP_MARGIN."""
    keep = torch.ones_like(ref["gap"], dtype=torch.bool)
    if case is not None and len(case) > 6 and edge_case_id(case) in EDGE_EXCLUDING:
        keep = ref["gap"] >= Z_GAP_MARGIN
    return keep, int((~keep).sum())


# ---- the early exit where it must not fire --------------------------------------------------------------------------------------------
STEEP_FILLERS = 520
STEEP_LAYERS = 6


def _fillers(n, g, bits, cx, cy, sum_max, zlo, zhi):
    """n small triangles: centres uniform in cx x cy pixels (with x + y <= sum_max), corners within 1.6 pixels of the centre, corner depths
    uniform in zlo .. zhi; candidates with no area or with no pixel centre inside their box are passed over, so each of the n is drawn and
    has its entry in the tile's list.  (pix_q [3n, 2] int64, zv [3n] float64)"""
    S = 1 << bits
    m = 4 * n
    u = torch.rand(m, 2, generator=g, dtype=torch.float64)
    ctr = torch.stack([cx[0] + (cx[1] - cx[0]) * u[:, 0], cy[0] + (cy[1] - cy[0]) * u[:, 1]], 1)
    off = 3.2 * torch.rand(m, 3, 2, generator=g, dtype=torch.float64) - 1.6
    q = torch.round((ctr[:, None, :] + off) * S).long()
    z = zlo + (zhi - zlo) * torch.rand(m, 3, generator=g, dtype=torch.float64)
    a, b, c = q[:, 0], q[:, 1], q[:, 2]
    area2 = (b[:, 0] - a[:, 0]) * (c[:, 1] - a[:, 1]) - (b[:, 1] - a[:, 1]) * (c[:, 0] - a[:, 0])
    x0, y0, x1, y1 = _rects(q, 1 << 20, 1 << 20, bits)
    ok = torch.nonzero((ctr.sum(1) <= sum_max) & (area2 != 0) & (x0 <= x1) & (y0 <= y1)).reshape(-1)[:n]
    assert ok.numel() == n
    return q[ok].reshape(-1, 2), z[ok].reshape(-1)


def steep_cover(bits=8, seed=1):
    """Face 0 covers the whole first tile, has the smallest zmin of the list (1.0, at the corner outside pixel (0, 0)) and rises to 7.0 at its
    two other corners: it is deeper than 2.0 on the 78 pixels of the tile with x + y >= 19.  STEEP_FILLERS small faces follow, zmin in
    1.05 .. 1.95, all inside the tile where x + y < 18; then STEEP_LAYERS faces that cover the tile at constant depths 2.0, 2.1, ..  In the
    tile's list the layers come after face 0 and the fillers: in the third batch of 256, with every pixel covered since the first entry.
    (pix_q, zv, faces, colors)"""
    g = torch.Generator().manual_seed(seed)
    corner = torch.tensor([[-1, -1], [34, -1], [-1, 34]], dtype=torch.long) << bits
    fq, fz = _fillers(STEEP_FILLERS, g, bits, (2.0, 12.0), (2.0, 12.0), 14.0, 1.05, 1.95)
    q = torch.cat([corner, fq, corner.repeat(STEEP_LAYERS, 1)])
    lz = (2.0 + 0.1 * torch.arange(STEEP_LAYERS, dtype=torch.float64)).repeat_interleave(3)
    zv = torch.cat([torch.tensor([1.0, 7.0, 7.0], dtype=torch.float64), fz, lz])
    n = q.shape[0] // 3
    colors = torch.rand(n, 1, 3, generator=g).expand(n, 3, 3).reshape(-1, 3).contiguous()
    return q, zv.float(), torch.arange(3 * n).reshape(n, 3), colors.float()


# ---- a bit-equal depth across a batch boundary ----------------------------------------------------------------------------------------
TIE_FILLERS = 511
TIE_PIXEL = (8, 0)          # (x, y)


def tie_across_batches(bits=8, seed=1):
    """Face 1 has corner depths (1.5, 2.0, 2.0); its 2.0 - 2.0 edge is a top edge along row 0 (it owns the centres on it) with TIE_PIXEL at
    its midpoint: there E0 = 0 and b1 = b2 = 0.5, so z = 2.0 exactly in float32 as in fp64.  Face 0 is a small triangle around that pixel
    centre with all corners at 2.0: the clamp makes it exactly 2.0.  Face 0 has the LARGER zmin, so in the first tile's list it comes after
    face 1 and after the TIE_FILLERS small faces (zmin in 1.55 .. 1.95, rows 1 and below) between them: at position 512, the first entry of
    the third batch, where the batch's first zmin EQUALS the depth the pixel holds.  (pix_q, zv, faces, colors)"""
    g = torch.Generator().manual_seed(seed)
    S = 1 << bits
    x, y = TIE_PIXEL
    small = torch.tensor([[x * S - S // 2, y * S - S // 2], [x * S + S // 2, y * S - S // 2], [x * S, y * S + S // 2]], dtype=torch.long)
    big = torch.tensor([[x, y + 60], [x - 28, y], [x + 28, y]], dtype=torch.long) << bits
    fq, fz = _fillers(TIE_FILLERS, g, bits, (2.0, 13.0), (3.0, 12.0), 99.0, 1.55, 1.95)
    q = torch.cat([small, big, fq])
    zv = torch.cat([torch.tensor([2.0, 2.0, 2.0, 1.5, 2.0, 2.0], dtype=torch.float64), fz])
    n = q.shape[0] // 3
    colors = torch.rand(n, 1, 3, generator=g).expand(n, 3, 3).reshape(-1, 3).contiguous()
    return q, zv.float(), torch.arange(3 * n).reshape(n, 3), colors.float()


SYNTH_SEEDS = {"steep_cover": 1, "tie_across_batches": 1}
SYNTH_SEEDS_TRIED = {"steep_cover": 1, "tie_across_batches": 1}


# ---- corners at the coordinate limit --------------------------------------------------------------------------------------------------
Q_EXTREME = 2 ** 28 - 3


def limit_triangle(bits=8):
    """Face 0 has its snapped corners just inside +-2^28 and contains the whole of a 56 x 40 image, corner depths 1.5, 2.5, 4.0; face 1 is an
    ordinary nearer triangle in front of part of it.  (pix_q, zv, faces, colors)"""
    L = Q_EXTREME
    q = torch.tensor([[-L, -L], [L, -L + 11], [-7, L], [5 << bits, 3 << bits], [(45 << bits) + 17, 10 << bits], [20 << bits, (35 << bits) + 99]],
                     dtype=torch.long)
    zv = torch.tensor([1.5, 2.5, 4.0, 1.2, 1.3, 1.25])
    colors = torch.tensor([[1.0, 0.2, 0.1], [0.1, 0.9, 0.3], [0.2, 0.3, 1.0], [0.7, 0.7, 0.1], [0.1, 0.6, 0.6], [0.9, 0.4, 0.8]])
    return q, zv, torch.arange(6).reshape(2, 3), colors


def edge_intermediates_max(pix_q, faces, W, H, bits):
    """The largest magnitude (a Python integer) among the differences, the two products and the value of every edge function and of the
    doubled area, and the sum of the three edge functions, over all faces and all pixel centres.  Each is linear or bilinear in the pixel,
    so the image's four corner pixels bound it."""
    S = 1 << bits
    q = [[int(a) for a in row] for row in pix_q.tolist()]
    top = 0
    for f in faces.tolist():
        c = [q[i] for i in f]
        for Px, Py in ((0, 0), ((W - 1) * S, 0), (0, (H - 1) * S), ((W - 1) * S, (H - 1) * S)):
            es = []
            for u, v in ((c[1], c[2]), (c[2], c[0]), (c[0], c[1])):
                t = [v[0] - u[0], v[1] - u[1], Px - u[0], Py - u[1]]
                p1, p2 = t[0] * t[3], t[1] * t[2]
                es.append(p1 - p2)
                top = max([top, abs(p1), abs(p2), abs(p1 - p2)] + [abs(x) for x in t])
            top = max(top, abs(sum(es)))
    return top


# ---- the image limit ------------------------------------------------------------------------------------------------------------------
LIMIT_SIZES = ((4096, 16), (16, 4096))
LIMIT_VIEW = 1
LIMIT_SEEDS = {(4096, 16): 1, (16, 4096): 1}          # counted up from 1 like the others
LIMIT_SEEDS_TRIED = {(4096, 16): 1, (16, 4096): 1}


def limit_extra(W, H, bits=8):
    """Three hand-placed triangles in snapped coordinates, wound as front faces: one over the image's last column (W > H) or last row and
    one over pixel (0, 0), both in front of everything (z 1.0 .. 1.2), and one behind everything (z 3.0 .. 3.2) that runs the whole length
    of the image, through every tile column (or row).  (pix_q [9, 2], zv [9], faces [3, 3] numbered from 0, colors [9, 3])"""
    n = max(W, H)
    along = [(n - 6, -2), (n + 4, 5), (n - 11, 19), (-3, -3), (9, 2), (2, 12), (-5, 2), (n + 5, 7), (n // 2, 14)]          # (long axis, short axis)
    pts = [(a, b) if W > H else (b, a) for a, b in along]
    q = torch.tensor([[(x << bits) + 37 * k, (y << bits) + 11 * k] for k, (x, y) in enumerate(pts)], dtype=torch.long)
    faces = torch.arange(9).reshape(3, 3)
    a, b, c = q[faces[:, 0]], q[faces[:, 1]], q[faces[:, 2]]
    area2 = (b[:, 0] - a[:, 0]) * (c[:, 1] - a[:, 1]) - (b[:, 1] - a[:, 1]) * (c[:, 0] - a[:, 0])
    faces = torch.where((area2 > 0)[:, None], faces.flip(1), faces)
    zv = torch.tensor([1.0, 1.1, 1.2, 1.05, 1.15, 1.1, 3.0, 3.2, 3.1])
    colors = torch.rand(9, 3, generator=torch.Generator().manual_seed(11))
    return q, zv, faces, colors


def with_extra(pix_q, zv, faces, colors, extra):
    """the projected mesh followed by the hand-placed faces of `extra` (limit_extra)"""
    eq, ez, ef, ec = extra
    V = zv.shape[0]
    return torch.cat([pix_q.long(), eq]), torch.cat([zv.float(), ez]), torch.cat([faces.long(), ef + V]), torch.cat([colors.float(), ec])
