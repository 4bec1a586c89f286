"""Pure-torch restatement of csrc_recon/meshbvh.hip and of v3d_amd/recon/mesh_bake.py (test oracle), fp64 by default; with
dtype=torch.float32 what that run loses against the fp64 one is the cost of the number format (the bar idiom of tests/mesh_render_ref.py).

Written from the statements of include/v3d_recon.h "Mesh BVH and normal bake".  The closest hit is a brute force over ALL triangles: the
tree enters only as invariants (check_tree), never as a shape to compare - a Morton code one quantisation step off gives a different,
equally valid tree."""
from __future__ import annotations

import functools
import math

import numpy as np
import torch

import mesh_clean_ref as C
import mesh_refine_ref as RF
import mesh_render_ref as M
import mesh_texture_ref as TX
import recon_geom_ref as R

F64, F32 = torch.float64, torch.float32
INF = float("inf")
BARY_MARGIN = 1e-4          # a ray is compared only when no barycentric of a triangle it could hit lies this close to 0 or 1
T_MARGIN = 1e-5             # ... and no t this close to tmin, tmax or the runner-up
EXCLUDE_MAX = M.EXCLUDE_MAX  # at most 2 % of a case's rays may be left out
NORMAL_EPS = 1e-20
KEY_BITS = 30


def height_bound(F):
    return KEY_BITS + max(F - 1, 0).bit_length()


# ---- closest hit, brute force ---------------------------------------------------------------------------------------------------------------
def _cross(a, b):
    return torch.stack([a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1], a[..., 2] * b[..., 0] - a[..., 0] * b[..., 2],
                        a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]], -1)


def _dot(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


@torch.no_grad()
def closest_hit(verts, faces, origins, directions, tmin=0.0, tmax=INF, cull=0, dtype=F64, open_min=False, chunk=1024):
    """dict(t [N], face [N] int64 (-1: a miss), uv [N, 2], keep [N] bool).  Every ray against every triangle by the header's Moeller-Trumbore;
    the smallest t, the smaller face on equal t.  keep: the ray's decisions hold the margins above - over the triangles that pass the tests
    widened by the margins and lie no further than T_MARGIN behind the best, no barycentric (u, v, 1 - u - v) within BARY_MARGIN of 0 or 1 and
    no t within T_MARGIN of tmin or tmax, and the second-best t is further than T_MARGIN from the best."""
    V = verts.shape[0]
    f = faces.long()
    ok = ((f >= 0) & (f < V)).all(1)
    fz = torch.where(ok[:, None], f, torch.zeros_like(f))
    v = verts.to(dtype)
    v0 = v[fz[:, 0]]
    e1, e2 = v[fz[:, 1]] - v0, v[fz[:, 2]] - v0
    ng = _cross(e1, e2)
    o_all, d_all = origins.to(dtype), directions.to(dtype)
    N = o_all.shape[0]
    out = dict(t=torch.full((N,), INF, dtype=dtype), face=torch.full((N,), -1, dtype=torch.long), uv=torch.zeros(N, 2, dtype=dtype),
               keep=torch.ones(N, dtype=torch.bool))
    for a in range(0, N, chunk):
        o, d = o_all[a:a + chunk, None, :], d_all[a:a + chunk, None, :]
        n = o.shape[0]
        nd = _dot(ng[None], d)
        facing = torch.ones_like(nd, dtype=torch.bool) if cull == 0 else (nd < 0 if cull == 1 else nd > 0)
        p = _cross(d, e2[None])
        det = _dot(e1[None], p)
        live = ok[None] & facing & (det != 0)
        inv = 1.0 / torch.where(det != 0, det, torch.ones_like(det))
        s = o - v0[None]
        u = _dot(s, p) * inv
        q = _cross(s, e1[None])
        vv = _dot(d, q) * inv
        t = _dot(e2[None], q) * inv
        hit = live & (u >= 0) & (vv >= 0) & (u + vv <= 1) & ((t > tmin) if open_min else (t >= tmin)) & (t <= tmax)
        tt = torch.where(hit, t, torch.full_like(t, INF))
        best = tt.min(1).values
        first = ((tt == best[:, None]) & hit).to(torch.int8).argmax(1)            # the first of the equal ones: the smaller face
        found = hit.any(1)
        rows = torch.arange(n)
        out["t"][a:a + n] = torch.where(found, best, torch.full_like(best, INF))
        out["face"][a:a + n] = torch.where(found, first, torch.full_like(first, -1))
        out["uv"][a:a + n] = torch.where(found[:, None], torch.stack([u[rows, first], vv[rows, first]], -1), torch.zeros(n, 2, dtype=dtype))
        # the margins
        w = 1 - u - vv
        wide = live & (u >= -BARY_MARGIN) & (vv >= -BARY_MARGIN) & (w >= -BARY_MARGIN) & (t >= tmin - T_MARGIN) & (t <= tmax + T_MARGIN)
        wide &= t <= best[:, None] + T_MARGIN
        close = lambda x, c: (x - c).abs() < BARY_MARGIN  # noqa: E731
        edge = close(u, 0) | close(u, 1) | close(vv, 0) | close(vv, 1) | close(w, 0) | close(w, 1)
        ends = ((t - tmin).abs() < T_MARGIN) | ((t - tmax).abs() < T_MARGIN)
        second = tt.clone()
        second[rows, first] = INF
        runner = found & (second.min(1).values - best < T_MARGIN)
        out["keep"][a:a + n] = ~((wide & (edge | ends)).any(1) | runner)
    return out


def unit(x):
    """x / |x| row by row, (0, 0, 1) where the squared length is not above 1e-20 (the rule of mesh_vertex_normals)"""
    len2 = _dot(x, x)
    good = len2 > NORMAL_EPS
    z = torch.zeros_like(x)
    z[..., 2] = 1
    return torch.where(good[..., None], x / torch.sqrt(torch.where(good, len2, torch.ones_like(len2)))[..., None], z)


# ---- the bake -------------------------------------------------------------------------------------------------------------------------------
@torch.no_grad()
def bake(low_verts, low_faces, low_normals, high_verts, high_faces, high_normals, R, max_dist, dtype=F64):
    """dict(owner [R*R] (-1: unowned), normal [R*R, 3], dist [R*R] (signed; NaN without a hit), hit_face [R*R], side [R*R] (+1, -1, 0 a miss
    or no cast), cast [R*R] bool (the texels that cast: owned by a face whose indices are vertices), keep [R*R] bool (cast texels whose
    decisions hold the margins of closest_hit on both casts, and whose two hits are further than T_MARGIN apart in t)).  The normals are
    GIVEN (the kernel's own vertex normals, or mesh_clean_ref.normals)."""
    Fl, Vl = low_faces.shape[0], low_verts.shape[0]
    S, _ = TX.layout(Fl, R)
    owner, i, j = TX.texel_cells(Fl, R)
    tri = low_faces.long()[owner.clamp_min(0)]
    cast = (owner >= 0) & ((tri >= 0) & (tri < Vl)).all(1)
    tri = torch.where(cast[:, None], tri, torch.zeros_like(tri))
    L = torch.tensor(float(S - 3), dtype=dtype)
    b1 = (i.to(dtype) / L).clamp(0, 1)
    b2 = torch.minimum((j.to(dtype) / L).clamp_min(0), 1 - b1)
    b0 = 1 - b1 - b2
    mix = lambda a: b0[:, None] * a[tri[:, 0]] + b1[:, None] * a[tri[:, 1]] + b2[:, None] * a[tri[:, 2]]  # noqa: E731
    P, n = mix(low_verts.to(dtype)), unit(mix(low_normals.to(dtype)))
    T = R * R
    normal = torch.zeros(T, 3, dtype=dtype)
    normal[:, 2] = 1
    dist = torch.full((T,), float("nan"), dtype=dtype)
    hit_face, side, keep = torch.full((T,), -1, dtype=torch.long), torch.zeros(T, dtype=torch.long), torch.zeros(T, dtype=torch.bool)
    idx = torch.nonzero(cast).reshape(-1)
    if idx.numel():
        Pc, nc = P[idx], n[idx]
        hp = closest_hit(high_verts, high_faces, Pc, nc, 0.0, max_dist, 2, dtype)
        hm = closest_hit(high_verts, high_faces, Pc, -nc, 0.0, max_dist, 1, dtype, open_min=True)
        hit_p, hit_m = hp["face"] >= 0, hm["face"] >= 0
        plus = hit_p & (~hit_m | (hp["t"] <= hm["t"]))
        any_hit = hit_p | hit_m
        face = torch.where(plus, hp["face"], hm["face"])
        t = torch.where(plus, hp["t"], hm["t"])
        uv = torch.where(plus[:, None], hp["uv"], hm["uv"])
        hf = high_faces.long()[face.clamp_min(0)]
        hn = high_normals.to(dtype)
        m = unit((1 - uv[:, 0] - uv[:, 1])[:, None] * hn[hf[:, 0]] + uv[:, 0:1] * hn[hf[:, 1]] + uv[:, 1:2] * hn[hf[:, 2]])
        normal[idx] = torch.where(any_hit[:, None], m, nc)
        dist[idx] = torch.where(any_hit, torch.where(plus, t, -t), torch.full_like(t, float("nan")))
        hit_face[idx] = torch.where(any_hit, face, torch.full_like(face, -1))
        side[idx] = torch.where(any_hit, torch.where(plus, 1, -1), 0)
        apart = ~(hit_p & hit_m) | ((hp["t"] - hm["t"]).abs() >= T_MARGIN)
        keep[idx] = hp["keep"] & hm["keep"] & apart
    return dict(owner=owner, normal=normal, dist=dist, hit_face=hit_face, side=side, cast=cast, keep=keep)


# ---- the tree, as invariants ------------------------------------------------------------------------------------------------------------------
def face_boxes(verts, faces):
    """(lo, hi) [F, 3] float32, exact; the empty box for a face with an index outside the vertices"""
    V = verts.shape[0]
    f = faces.long()
    ok = ((f >= 0) & (f < V)).all(1)
    tri = verts.float()[torch.where(ok[:, None], f, torch.zeros_like(f))]             # [F, 3 corners, 3]
    lo, hi = tri.min(1).values, tri.max(1).values
    return (torch.where(ok[:, None], lo, torch.full_like(lo, INF)), torch.where(ok[:, None], hi, torch.full_like(hi, -INF)))


def check_tree(order, left, right, parent, lo, hi, verts, faces):
    """Asserts the invariants of "THE NODES" on host tensors and returns the tree's height (edges from the root to the deepest leaf): every
    leaf is reached exactly once from the root, parent and children agree, every node's box is bit-equal to the union of its leaves' face
    boxes, the height is within 30 + bits(F - 1)."""
    F = faces.shape[0]
    order, left, right, parent = (np.asarray(t.cpu()).astype(np.int64) for t in (order, left, right, parent))
    lo, hi = np.asarray(lo.cpu()), np.asarray(hi.cpu())
    assert order.shape == (F,) and sorted(order.tolist()) == list(range(F)), "order is not a permutation of the faces"
    assert parent.shape == (2 * F - 1,) and lo.shape == hi.shape == (2 * F - 1, 3) and lo.dtype == np.float32
    assert parent[0] == -1
    flo, fhi = (np.asarray(t) for t in face_boxes(verts, faces))
    seen = np.zeros(2 * F - 1, dtype=np.int64)
    depth = np.zeros(2 * F - 1, dtype=np.int64)
    visit, stack = [], [0]
    while stack:                                    # pre-order; a cycle would revisit a node
        n = stack.pop()
        seen[n] += 1
        assert seen[n] == 1, f"node {n} is reached twice"
        visit.append(n)
        if n < F - 1:
            for c in (int(left[n]), int(right[n])):
                assert 0 <= c < 2 * F - 1 and c != 0 and parent[c] == n, f"node {n}: child {c} does not name it as its parent"
                depth[c] = depth[n] + 1
                stack.append(c)
    assert bool((seen == 1).all()), "a node is not reached from the root"
    blo, bhi = np.empty_like(lo), np.empty_like(hi)
    for n in reversed(visit):                       # children before their parent
        if n >= F - 1:
            blo[n], bhi[n] = flo[order[n - (F - 1)]], fhi[order[n - (F - 1)]]
        else:
            blo[n], bhi[n] = np.minimum(blo[left[n]], blo[right[n]]), np.maximum(bhi[left[n]], bhi[right[n]])
    assert np.array_equal(lo, blo) and np.array_equal(hi, bhi), "a box is not the union of its leaves' face boxes"
    height = int(depth.max())
    assert height <= height_bound(F), f"height {height} above {height_bound(F)}"
    return height


# ---- scenes -----------------------------------------------------------------------------------------------------------------------------------
N_RANDOM, N_AXIS = 1000, 100
RAY_COUNTS = (1, 63, 64, 65, 1100)


@functools.lru_cache(maxsize=None)
def rays(seed=3):
    """(origins, directions) [1100, 3] float32 for the sphere and pair scenes (both lie inside the ball of radius 0.6): 1000 rays from a
    shell of radius 1.2 .. 2 towards points of the ball of radius 0.7 (some pass the meshes by), directions NOT normalised (lengths
    0.5 .. 2), then 100 axis-parallel rays (one nonzero direction component) from a plane outside; shuffled, so a prefix holds both kinds."""
    g = torch.Generator().manual_seed(seed)
    rnd = lambda *s: torch.rand(*s, generator=g, dtype=F64)  # noqa: E731
    sph = lambda n: torch.nn.functional.normalize(torch.randn(n, 3, generator=g, dtype=F64), dim=1)  # noqa: E731
    o = sph(N_RANDOM) * (1.2 + 0.8 * rnd(N_RANDOM, 1))
    aim = sph(N_RANDOM) * 0.7 * rnd(N_RANDOM, 1) ** (1 / 3)
    d = torch.nn.functional.normalize(aim - o, dim=1) * (0.5 + 1.5 * rnd(N_RANDOM, 1))
    axis = torch.randint(3, (N_AXIS,), generator=g)
    sign = torch.where(rnd(N_AXIS) < 0.5, -1.0, 1.0).to(F64)
    oa = (rnd(N_AXIS, 3) * 2 - 1) * 0.6
    da = torch.zeros(N_AXIS, 3, dtype=F64)
    rows = torch.arange(N_AXIS)
    oa[rows, axis] = -1.5 * sign
    da[rows, axis] = sign * (0.5 + rnd(N_AXIS))
    perm = torch.randperm(N_RANDOM + N_AXIS, generator=g)
    return torch.cat([o, oa])[perm].float(), torch.cat([d, da])[perm].float()


@functools.lru_cache(maxsize=None)
def ray_case(kind, cull):
    """The scene and both restatements of all 1100 rays, computed once and shared (a ray's result does not depend on the other rays)"""
    v, f, _ = M.mesh_scene(kind, 1)
    o, d = rays()
    return v, f, o, d, closest_hit(v, f, o, d, 0.0, INF, cull), closest_hit(v, f, o, d, 0.0, INF, cull, F32)


def bumped(verts, amplitude=0.03, seed=5):
    """The vertices moved along their radius by a smooth function of the direction: detail for a normal map to carry"""
    v = verts.double()
    r = v.norm(dim=1, keepdim=True)
    u = v / r
    k = 1.0 + amplitude / 0.5 * (torch.sin(7.0 * u[:, 0:1] + seed) * torch.sin(5.0 * u[:, 1:2]) + 0.6 * torch.sin(9.0 * u[:, 2:3]))
    return (v * k).float()


BAKE_SIZES = (64, 100)               # S = 4 at 320 faces; ragged
BAKE_MAX_DIST = 0.2
BAKE_SHORT = 0.012                   # shorter than the bump: misses
BAKE_CASES = ("nested", "short", "offset")


@functools.lru_cache(maxsize=None)
def bake_scene(name):
    """(low_verts, low_faces, high_verts, high_faces, max_dist): an icosphere of 320 faces inside / around a bumped one of 1280 faces, rotated
    DIFFERENTLY (seeds 2 and 1: with the same rotation the low mesh's edges project exactly onto the high mesh's edges and most rays lie
    inside the margins).  "short": max_dist below the bump, so many texels miss.  "offset": the low mesh shifted so that part of it lies
    outside the high one and part inside (both signs)."""
    lv, lf = M.icosphere(2, 0.5, (0.0, 0.0, 0.0), seed=2)
    hv, hf = M.icosphere(3, 0.5, (0.0, 0.0, 0.0), seed=1)
    hv = bumped(hv)
    if name == "offset":
        lv = lv + torch.tensor([0.05, -0.03, 0.02])
    return lv, lf, hv, hf, (BAKE_SHORT if name == "short" else BAKE_MAX_DIST)


def same_centroid_faces(n=8):
    """n triangles, pairwise different, with ONE box (two corners on the unit cube's diagonal, the third inside it) and so one box centre:
    all Morton codes are equal and only the index tie-break separates them"""
    g = torch.Generator().manual_seed(8)
    v, f = [], []
    for k in range(n):
        v.append(torch.cat([torch.zeros(1, 3), torch.ones(1, 3), 0.1 + 0.8 * torch.rand(1, 3, generator=g)]))
        f.append([3 * k, 3 * k + 1, 3 * k + 2])
    return torch.cat(v).float(), torch.tensor(f)


def low_bit_strip(n=64):
    """A strip of n small triangles along x inside ONE quantisation cell pair of a wide mesh: two far vertices stretch the bounding box so
    that neighbouring triangles' codes differ in the low bits only, or not at all: a deep tree.  Faces n and n + 1 are the far anchors."""
    step = 1.0 / 1024 / 8
    v, f = [], []
    for k in range(n):
        x = k * step
        v += [[x, 0.0, 0.0], [x + step, 0.0, 0.0], [x, step, 0.0]]
        f.append([3 * k, 3 * k + 1, 3 * k + 2])
    base = len(v)
    v += [[1.0, 1.0, 1.0], [1.0, 0.99, 1.0], [0.99, 1.0, 1.0], [-1.0, -1.0, -1.0], [-1.0, -0.99, -1.0], [-0.99, -1.0, -1.0]]
    f += [[base, base + 1, base + 2], [base + 3, base + 4, base + 5]]
    return torch.tensor(v, dtype=torch.float32), torch.tensor(f)


def degenerate_mesh():
    """The 320-face sphere plus a zero-area face and a face with index V: neither is ever hit"""
    v, f, _ = M.mesh_scene("sphere", 1)
    V = v.shape[0]
    return v, torch.cat([f, torch.tensor([[0, 1, 1], [0, V, 2]])])


# ---- the end-to-end scene -------------------------------------------------------------------------------------------------------------------
# A bumpy sphere at 24^3 through surface nets (about 1350 faces), decimated to 300 faces; 4 orbit cameras at 64 x 64; R = 128.  The bump's
# amplitude (0.08 of the radius, period about 5 voxels) is what the grid resolves and 300 faces do not.
E2E = dict(N=24, bound=1.0, radius=0.5, bump=0.08, target_faces=300, views=4, size=64, orbit=(2.0, 15.0, 60.0), tex_size=128)


def bumpy_radius(p, radius, bump):
    d = p.norm(dim=1).clamp_min(1e-6)
    u = p / d[:, None]
    return d, radius * (1.0 + bump * torch.sin(7.0 * u[:, 0]) * torch.sin(5.0 * u[:, 1]) + 0.6 * bump * torch.sin(9.0 * u[:, 2]))


def bumpy_volume(N=E2E["N"], bound=E2E["bound"], radius=E2E["radius"], bump=E2E["bump"], dtype=torch.float32):
    """recon_geom_ref.sphere_volume with a bumpy zero level (tools/mesh_refine_bench.bumpy_sphere_volume's idea, small)"""
    vol = R.new_volume(N, bound, dtype=dtype)
    p = R.voxel_centres(N, bound)
    d, rad = bumpy_radius(p, radius, bump)
    vol["tsdf_sum"] = ((d - rad) / vol["trunc"]).clamp(-1, 1).to(dtype)
    vol["weight"] = torch.ones(N ** 3, dtype=dtype)
    vol["rgb_sum"] = (0.5 + 0.5 * p.t() / bound).clamp(0, 1).to(dtype).contiguous()
    vol["rgb_weight"] = torch.ones(N ** 3, dtype=dtype)
    return vol


def e2e_cameras():
    from v3d_amd.recon.cameras import orbit_cameras
    return orbit_cameras(E2E["views"], *E2E["orbit"], E2E["size"])[0]


def _unit_image(img):
    n = img * 2 - 1
    return n / n.norm(dim=0, keepdim=True).clamp_min(1e-12)


@torch.no_grad()
def fidelity(low_verts, low_faces, low_normals, normal_map, high_verts, high_faces, high_normals, cameras, dtype=F64):
    """(angle_before, angle_after): the mean over the views of the mean angle in degrees, over the pixels both meshes cover, between the high
    mesh's rasterized vertex normals and the low mesh's (a) rasterized vertex normals, (b) normal map sampled per pixel.  Everything on the
    restatements (mesh_render_ref, mesh_refine_ref, mesh_texture_ref); the angle does not depend on the frame, so normals stay in world space."""
    R_ = math.isqrt(normal_map.shape[0])
    bg = [0.5, 0.5, 0.5]
    before, after = [], []
    for cam in cameras:
        W, H = int(cam.width), int(cam.height)
        ph = M.project(high_verts, cam, 8, F32)
        rh = M.rasterize(ph["pix_q"], ph["zv"], high_faces, (high_normals.float() + 1) * 0.5, W, H, bg, cull=True)
        pl = M.project(low_verts, cam, 8, F32)
        rl = M.rasterize(pl["pix_q"], pl["zv"], low_faces, (low_normals.float() + 1) * 0.5, W, H, bg, cull=True)
        _, pw = RF.pixel_weights(pl["pix_q"], pl["zv"], low_faces, rl["face_id"], 8, F32)
        pt = TX.pixel_texels(rl["face_id"], pw, low_faces.shape[0], R_, dtype)
        mapped = TX.shade(pt["pix_tex"], pt["pix_tw"], normal_map, [0.0, 0.0, 0.0], dtype)
        mapped = mapped / mapped.norm(dim=0, keepdim=True).clamp_min(1e-12)
        both = (rh["face_id"] >= 0) & (rl["face_id"] >= 0)
        nh = _unit_image(rh["image"].to(dtype))
        ang = lambda a: float(torch.rad2deg(torch.acos((a * nh).sum(0)[both].double().clamp(-1, 1))).mean())  # noqa: E731
        before.append(ang(_unit_image(rl["image"].to(dtype))))
        after.append(ang(mapped))
    return float(np.mean(before)), float(np.mean(after))


@functools.lru_cache(maxsize=None)
def e2e_cpu():
    """The end-to-end scene wholly on the restatements: dict(high=(verts, faces, normals), low=(verts, faces, normals), cams, max_dist)"""
    import mesh_decimate_ref as DM
    vf, ff, _, _, _ = R.extract(bumpy_volume())
    vf = vf.float()
    kept, fd, _ = DM.decimate(vf.numpy(), ff.numpy(), E2E["target_faces"])
    vd, fd = vf[torch.from_numpy(kept)], torch.from_numpy(fd)
    diag = float((vf.max(0).values - vf.min(0).values).norm())
    return dict(high=(vf, ff, C.normals(vf, ff).float()), low=(vd, fd, C.normals(vd, fd).float()), cams=e2e_cameras(), max_dist=0.05 * diag)


def e2e_restatement(dtype=F64):
    """dict(before, after, reduction: degrees; bake: bake()'s result) of the end-to-end scene"""
    sc = e2e_cpu()
    (hv, hf, hn), (lv, lf, ln) = sc["high"], sc["low"]
    b = bake(lv, lf, ln, hv, hf, hn, E2E["tex_size"], sc["max_dist"], dtype)
    before, after = fidelity(lv, lf, ln, b["normal"], hv, hf, hn, sc["cams"], dtype)
    return dict(before=before, after=after, reduction=before - after, bake=b)
