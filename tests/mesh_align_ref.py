"""Pure-torch restatement of csrc_recon/meshalign.hip and of v3d_amd/recon/mesh_align.py (test oracle), fp64 by default; with
dtype=torch.float32 what that run loses against the fp64 one is the cost of the number format (the bar idiom of tests/mesh_bake_ref.py).

Written from the statements of include/v3d_recon.h "Mesh alignment".  The correspondences are mesh_query_ref.closest_point, a brute force
over the triangles: the tree does not enter.  The sums are formed in double from the values of `dtype`, as the kernel forms them from its
floats;  the solve is always float64.  It also holds the scenes of tests/test_mesh_align_cpu.py and tests/test_mesh_align_gpu.py."""
from __future__ import annotations

import functools
import itertools
import json
import math
import os

import numpy as np
import torch

import mesh_query_ref as Q
import mesh_render_ref as M
import mesh_solid_ref as S

F64, F32 = torch.float64, torch.float32
INF = float("inf")
COLUMNS = 20
IOU_BOUND = 1.05
IOU_MARGIN = 1e-3                    # a voxel whose fp64 winding number is this close to 0.5 for either mesh may fall either side
EXCLUDE_MAX = M.EXCLUDE_MAX          # at most 2 % of a case may be left out


# ---- one step ---------------------------------------------------------------------------------------------------------------------------------
def matrix32(T):
    """the upper 3 x 4 of a 4 x 4 float64 matrix as the float32 the kernel receives"""
    return torch.as_tensor(np.asarray(T, dtype=np.float64)[:3].astype(np.float32))


def transform(points, m, dtype=F64):
    """p'_r = ((M_r0 x + M_r1 y) + M_r2 z) + M_r3 in `dtype`, from the float32 matrix m [3, 4]"""
    p, m = points.to(dtype), m.to(dtype)
    return torch.stack([((m[r, 0] * p[:, 0] + m[r, 1] * p[:, 1]) + m[r, 2] * p[:, 2]) + m[r, 3] for r in range(3)], 1)


def rebuild(verts, faces, face, uv, dtype=F64):
    """q = a + u e1 + v e2 of (face, uv) in `dtype`, b itself where u == 1 and c itself where v == 1;  NaN where face < 0"""
    v, f = verts.to(dtype), faces.long()[face.long().clamp_min(0)]
    a, b, c = v[f[:, 0]], v[f[:, 1]], v[f[:, 2]]
    u, w = uv[:, 0:1].to(dtype), uv[:, 1:2].to(dtype)
    q = a + u * (b - a) + w * (c - a)
    q = torch.where(u == 1, b, q)
    q = torch.where(w == 1, c, q)
    return torch.where((face >= 0)[:, None], q, torch.full_like(q, float("nan")))


def pair_terms(moved, closest, dist, face, weights):
    """[N, 20] float64: the terms of every sample exactly as the kernel forms them (every operation rounded on its own, products from the
    left), exact zeros for a sample that does not count"""
    p, q, d, w = moved.double(), closest.double(), dist.double(), weights.double()
    valid = torch.isfinite(moved).all(1) & torch.isfinite(weights) & (weights >= 0)
    counts = valid & (face >= 0)
    t = torch.zeros(p.shape[0], COLUMNS, dtype=F64)
    t[:, 0] = w
    t[:, 1:4] = w[:, None] * p
    wq = w[:, None] * q
    t[:, 4:7] = wq
    t[:, 7:16] = (wq[:, :, None] * p[:, None, :]).reshape(-1, 9)
    t[:, 16] = w * ((p[:, 0] * p[:, 0] + p[:, 1] * p[:, 1]) + p[:, 2] * p[:, 2])
    t[:, 17] = w * (d * d)
    t[:, 18] = 1.0
    t = torch.where(counts[:, None], t, torch.zeros_like(t))
    t[:, 19] = torch.where(valid, w, torch.zeros_like(w))
    return t


@torch.no_grad()
def correspond(verts, faces, points, weights, T, max_dist=INF, dtype=F64):
    """The dict of mesh_align.correspond without "partials": moved, closest, dist, uv in `dtype`, face int64, sums [20] float64"""
    moved = transform(points, matrix32(T), dtype)
    r = Q.closest_point(verts, faces, moved, max_dist, dtype)
    closest = rebuild(verts, faces, r["face"], r["uv"], dtype)
    t = pair_terms(moved, closest, r["dist"], r["face"], weights.to(dtype))
    return {"moved": moved, "closest": closest, "dist": r["dist"], "face": r["face"], "uv": r["uv"], "sums": t.sum(0), "runner": r["runner"]}


def umeyama(sums, mode="similarity"):
    """4 x 4 float64 from the 20 sums (Umeyama 1991, eqs. 34 - 43, weighted), written in torch;  mesh_align.solve_similarity uses numpy"""
    s = torch.as_tensor(np.asarray(sums, dtype=np.float64))
    out = torch.eye(4, dtype=F64)
    W = s[0]
    if not bool(W > 0):
        return out.numpy()
    mp, mq = s[1:4] / W, s[4:7] / W
    var = s[16] / W - (mp * mp).sum()
    if not bool(var > 0):
        return out.numpy()
    C = s[7:16].reshape(3, 3) / W - mq[:, None] * mp[None, :]
    U, D, Vh = torch.linalg.svd(C)
    sg = torch.ones(3, dtype=F64)
    if float(torch.linalg.det(U) * torch.linalg.det(Vh)) < 0:
        sg[2] = -1.0
    R = U @ torch.diag(sg) @ Vh
    c = (D * sg).sum() / var if mode == "similarity" else torch.tensor(1.0, dtype=F64)
    out[:3, :3] = c * R
    out[:3, 3] = mq - c * (R @ mp)
    return out.numpy()


def cube_rotations():
    out = []
    for perm in itertools.permutations(range(3)):
        for signs in itertools.product((1, -1), repeat=3):
            R = np.zeros((3, 3))
            R[np.arange(3), list(perm)] = signs
            if np.linalg.det(R) > 0:
                out.append(R)
    return out


def start_transform(k, verts, ref_verts, mode):
    R = cube_rotations()[k]
    r = verts.double().numpy() @ R.T
    ref = ref_verts.double().numpy()
    d0, d1 = np.linalg.norm(r.max(0) - r.min(0)), np.linalg.norm(ref.max(0) - ref.min(0))
    s = d1 / d0 if mode == "similarity" else 1.0
    T = np.eye(4)
    T[:3, :3] = s * R
    T[:3, 3] = 0.5 * (ref.min(0) + ref.max(0)) - s * 0.5 * (r.min(0) + r.max(0))
    return T


def trim_distance(dist, weights, valid_weight, trim):
    ok = torch.isfinite(dist) & torch.isfinite(weights) & (weights >= 0)
    ds, order = torch.sort(dist[ok], stable=True)
    cum = torch.cumsum(weights[ok].double()[order], 0)
    hit = torch.nonzero(cum >= trim * valid_weight).reshape(-1)
    if hit.numel() == 0:
        return INF
    return float(np.nextafter(np.float32(float(ds[hit[0]])), np.float32(np.inf)))


def rms_of(sums):
    return math.sqrt(float(sums[17]) / float(sums[0])) if float(sums[0]) > 0 else float("nan")


def icp(verts, faces, pts, w, T, mode, iterations, tol, trim, dtype):
    hist, r = [], None
    for it in range(iterations + 1):
        md = INF
        if trim < 1.0:
            u = correspond(verts, faces, pts, w, T, INF, dtype)
            md = trim_distance(u["dist"].float(), w.float(), float(u["sums"][19]), trim)
        r = correspond(verts, faces, pts, w, T, md, dtype)
        hist.append(rms_of(r["sums"]))
        if it == iterations or (tol > 0 and it > 0 and abs(hist[-2] - hist[-1]) < tol * hist[-2]):
            break
        T = umeyama(r["sums"], mode) @ T
    return T, hist, r


@torch.no_grad()
def align(verts, faces, ref_verts, ref_faces, mode="similarity", starts=1, iterations=200, tol=1e-5, trim=1.0, subdivide=2, start_iterations=10,
          dtype=F64, only_start=None):
    """(matrix, stats) of mesh_align.align_mesh: rms_history, iterations_run, start, start_rms.  only_start: run that start alone."""
    pts, w, _ = Q.face_samples(verts, faces, subdivide, dtype)
    pts, w = pts.float(), w.float()                    # the samples reach the kernel as float32 whatever formed them
    if mode == "none":
        T, hist, _ = icp(ref_verts, ref_faces, pts, w, np.eye(4), "rigid", 0, 0.0, trim, dtype)
        return T, {"rms_history": hist, "iterations_run": 0, "start": 0, "start_rms": None}
    if starts == 1 or only_start is not None:
        k = only_start or 0
        T, hist, _ = icp(ref_verts, ref_faces, pts, w, start_transform(k, verts, ref_verts, mode), mode, iterations, tol, trim, dtype)
        return T, {"rms_history": hist, "iterations_run": len(hist) - 1, "start": k, "start_rms": None}
    head_n = min(start_iterations, iterations)
    runs = [icp(ref_verts, ref_faces, pts, w, start_transform(k, verts, ref_verts, mode), mode, head_n, 0.0, trim, dtype) for k in range(24)]
    start_rms = [h[-1] for _, h, _ in runs]
    start = min(range(24), key=lambda k: (not math.isfinite(start_rms[k]), start_rms[k], k))
    T, hist, _ = runs[start]
    if iterations > head_n:
        T, tail, _ = icp(ref_verts, ref_faces, pts, w, T, mode, iterations - head_n, tol, trim, dtype)
        hist = hist + tail[1:]
    return T, {"rms_history": hist, "iterations_run": len(hist) - 1, "start": start, "start_rms": start_rms}


def decompose(T):
    """(scale, rotation [3, 3], angle in degrees)"""
    A = np.asarray(T, dtype=np.float64)[:3, :3]
    s = np.cbrt(np.linalg.det(A))
    R = A / s
    return float(s), R, math.degrees(math.acos(min(1.0, max(-1.0, (np.trace(R) - 1.0) / 2.0))))


def residual(T, T0):
    """(residual rotation in degrees, s s0) of an estimate T against the motion T0 it should undo"""
    s, _, angle = decompose(np.asarray(T) @ np.asarray(T0))
    return angle, s


# ---- the scores -------------------------------------------------------------------------------------------------------------------------------
def unit_normals(verts, faces, dtype=F64):
    v, f = verts.to(dtype), faces.long()
    n = torch.linalg.cross(v[f[:, 1]] - v[f[:, 0]], v[f[:, 2]] - v[f[:, 0]])
    length = n.norm(dim=1, keepdim=True)
    return torch.where(length > 0, n / length.clamp_min(1e-300 if dtype == F64 else 1e-38), torch.zeros_like(n))


@torch.no_grad()
def one_way_scores(v, f, n, tv, tf, dtype=F64):
    """dict(dist [S] of every sample, weights [S], nc: the normal consistency, dots [S])"""
    pts, w, _ = Q.face_samples(v, f, n, dtype)
    r = Q.closest_point(tv, tf, pts, INF, dtype)
    mine = unit_normals(v, f, dtype).repeat_interleave(n * n, 0)
    other = unit_normals(tv, tf, dtype)[r["face"].clamp_min(0)]
    dots = torch.where(r["face"] >= 0, (mine * other).sum(1).abs(), torch.zeros_like(r["dist"]))
    w64 = w.double()
    return {"dist": r["dist"].double(), "weights": w64, "nc": float((dots.double() * w64).sum() / w64.sum()), "dots": dots.double(), "face": r["face"]}


NORMAL_FLOOR = 1e-9                  # 1/60 of half an ulp of a float32 near 1, and below the bar of every case here: it decides none of them


def normal_bar(r64, r32):
    """The project's standing bar on the normal consistency itself: 4 x what the float32 restatement's figure is off from the fp64 one's.
    Never below NORMAL_FLOOR, which only keeps the bar from being 0 should a float32 run land on the fp64 figure exactly."""
    return max(4.0 * abs(r32["nc"] - r64["nc"]), NORMAL_FLOOR)


def share_interval(dist64, weights, tau, err):
    """(lo, hi): the share of the weight surely within tau, and that plus the share whose fp64 distance lies within err of tau"""
    area = float(weights.sum())
    return float((weights * (dist64 <= tau - err)).sum()) / area, float((weights * (dist64 <= tau + err)).sum()) / area


@torch.no_grad()
def iou_windings(a_verts, a_faces, b_verts, b_faces, N, dtype=F64):
    """(wa, wb [N^3] of S.exact_winding at the voxel centres of the IoU grid, bound)"""
    bound = IOU_BOUND * max(float(a_verts.abs().max()), float(b_verts.abs().max()))
    from v3d_amd.recon.mesh_solid import voxel_centres
    c = voxel_centres(N, bound, "cpu")
    return S.exact_winding(a_verts, a_faces, c, dtype).double(), S.exact_winding(b_verts, b_faces, c, dtype).double(), bound


def iou_counts(wa, wb, keep=None):
    oa, ob = wa >= 0.5, wb >= 0.5
    if keep is not None:
        oa, ob = oa & keep, ob & keep
    return int(oa.sum()), int(ob.sum()), int((oa & ob).sum()), int((oa | ob).sum())


def iou_sure(wa, wb):
    """the voxels whose occupancy no float rounding can change: both winding numbers further than IOU_MARGIN from 0.5"""
    return ((wa - 0.5).abs() >= IOU_MARGIN) & ((wb - 0.5).abs() >= IOU_MARGIN)


# ---- scenes -----------------------------------------------------------------------------------------------------------------------------------
def deform(verts):
    """no symmetry left: scale by (1, 0.7, 0.5), x += 0.5 relu(x), y += 0.6 x^2, z += 0.3 x y, each on the result of the one before, in float64"""
    v = verts.double() * torch.tensor([1.0, 0.7, 0.5], dtype=F64)
    x = v[:, 0] + 0.5 * torch.relu(v[:, 0])
    y = v[:, 1] + 0.6 * x * x
    z = v[:, 2] + 0.3 * x * y
    return torch.stack([x, y, z], 1).float()


def similarity(angle_deg, axis, scale, shift):
    """4 x 4 float64: a rotation about `axis`, then the scale, then the shift"""
    k = np.asarray(axis, dtype=np.float64)
    k /= np.linalg.norm(k)
    K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    a = math.radians(angle_deg)
    R = np.eye(3) + math.sin(a) * K + (1 - math.cos(a)) * (K @ K)
    T = np.eye(4)
    T[:3, :3] = scale * R
    T[:3, 3] = shift
    return T


KNOWN = similarity(12.0, (1, 2, 3), 1.08, (0.05, -0.03, 0.04))
FAR = similarity(170.0, (1, 2, 3), 1.3, (0.2, -0.1, 0.1))
TARGET_DIAGONAL = 1.552


def move(verts, T):
    T = torch.as_tensor(T)
    return (verts.double() @ T[:3, :3].T + T[:3, 3]).float()


@functools.lru_cache(maxsize=None)
def target():
    v, f = M.icosphere(3, 0.5, (0.0, 0.0, 0.0), seed=1)
    return deform(v), f


@functools.lru_cache(maxsize=None)
def coarse():
    v, f = M.icosphere(2, 0.5, (0.0, 0.0, 0.0), seed=2)
    return deform(v), f


@functools.lru_cache(maxsize=None)
def coarse_with_floater():
    v, f = coarse()
    fv, ff = M.icosphere(1, 0.12, (0.9, 0.7, 0.3), seed=3)
    return torch.cat([v, fv]), torch.cat([f, ff + v.shape[0]])


EARLY_TOL = 0.09
# name -> (the moving mesh, the motion it was given, the arguments of align)
ALIGN_CASES = {
    "recovery": (target, KNOWN, dict(subdivide=1, iterations=60, tol=0.0)),
    "far": (coarse, FAR, dict(subdivide=2, starts=24, iterations=60, tol=0.0, start_iterations=10)),
    "floater": (coarse_with_floater, KNOWN, dict(subdivide=1, iterations=60, tol=0.0, trim=1.0)),
    # (the trimmed run is still converging after 60 iterations, 4.5 degrees off; it is 0.64 degrees off after 100)
    "floater_trim": (coarse_with_floater, KNOWN, dict(subdivide=1, iterations=100, tol=0.0, trim=0.9)),
    "rigid": (target, similarity(12.0, (1, 2, 3), 1.0, (0.05, -0.03, 0.04)), dict(subdivide=1, iterations=60, tol=0.0, mode="rigid")),
    # the early stop: the RMS of the recovery falls by 9.2 % in iteration 9 and by 8.6 % in iteration 10, so tol = 0.09 stops it there, and
    # no rounding of float32 (1e-7 of these figures) can move the stop
    "early": (target, KNOWN, dict(subdivide=1, iterations=60, tol=EARLY_TOL)),
}
EARLY_ITERATIONS = 10


def align_inputs(name):
    """(moving verts, faces, reference verts, faces, the motion, the arguments)"""
    mesh, T0, kw = ALIGN_CASES[name]
    v, f = mesh()
    rv, rf = target()
    return move(v, T0), f, rv, rf, T0, kw


@functools.lru_cache(maxsize=None)
def align_case(name, dtype=F64):
    """(matrix, stats) of the restatement, computed once"""
    v, f, rv, rf, _, kw = align_inputs(name)
    return align(v, f, rv, rf, dtype=dtype, **kw)


# ---- the recorded runs ------------------------------------------------------------------------------------------------------------------------
# The ICP runs above take some minutes on a CPU.  tests/golden/mesh_align_cases.json records them (`python tests/mesh_align_ref.py`
# writes it);  tests/test_mesh_align_cpu.py runs every one afresh, fp64 and float32, and holds the file to them, tests/test_mesh_align_gpu.py
# reads the file.
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "mesh_align_cases.json")


@functools.lru_cache(maxsize=None)
def recorded():
    return json.load(open(GOLDEN))


def recorded_case(name, dtype=F64):
    """(matrix [4, 4] float64, {"rms_history", "start", "start_rms"}) as recorded"""
    r = recorded()[name]["float64" if dtype == F64 else "float32"]
    return np.asarray(r["matrix"], dtype=np.float64), r


def history_bar(name):
    """4 x the largest difference between the float32 restatement's RMS history and the fp64 one's (the project's standing bar)"""
    h64, h32 = recorded_case(name)[1]["rms_history"], recorded_case(name, F32)[1]["rms_history"]
    assert len(h64) == len(h32)
    return 4.0 * max(abs(a - b) for a, b in zip(h64, h32))


def record_cases(names=None, path=GOLDEN):
    """run the named cases (default: all) in both formats and write them into the file, beside what it already holds"""
    out = json.load(open(path)) if os.path.exists(path) else {}
    for name in names or ALIGN_CASES:
        out[name] = {}
        for key, dtype in (("float64", F64), ("float32", F32)):
            T, st = align_case(name, dtype)
            out[name][key] = {"matrix": np.asarray(T).tolist(), "rms_history": st["rms_history"], "start": st["start"], "start_rms": st["start_rms"]}
            print(name, key, st["start"], st["rms_history"][0], st["rms_history"][-1], flush=True)
    with open(path, "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")


# ---- the pairs that are scored ------------------------------------------------------------------------------------------------------------------
SCORE_PAIRS = ("distance", "aligned")
IOU_RESOLUTIONS = (16, 17)
THRESHOLDS = (0.01, 0.02, 0.05)


@functools.lru_cache(maxsize=None)
def score_pair(name):
    """(a_verts, a_faces, b_verts, b_faces): mesh_query_ref.distance_pair(), or the coarse body under the far start moved back by the
    recorded fp64 matrix of that case, against the target"""
    if name == "distance":
        return Q.distance_pair()
    v, f, rv, rf, _, _ = align_inputs("far")
    return move(v, recorded_case("far")[0]), f, rv, rf


@functools.lru_cache(maxsize=None)
def iou_case(name, N):
    return iou_windings(*score_pair(name), N)


@functools.lru_cache(maxsize=None)
def score_case(name, n=2):
    """dict per direction and dtype of one_way_scores, computed once: [("a_to_b" | "b_to_a", F64 | F32)]"""
    av, af, bv, bf = score_pair(name)
    return {(d, t): one_way_scores(*(m + (n,) + o + (t,))) for d, m, o in (("a_to_b", (av, af), (bv, bf)), ("b_to_a", (bv, bf), (av, af)))
            for t in (F64, F32)}


def premises():
    """The figures of the fp64 restatement that tests/test_mesh_align_cpu.py asserts and DESIGN.md quotes: per case of the file the RMS
    before and after over the target's diagonal, the fall, the residual rotation and s s0, the start, the iterations, and what the float32
    record is off;  with them two runs of their own: start 0 alone from the far start, and the trimmed floater stopped after 60 iterations"""
    out = {}
    for name in ALIGN_CASES:
        T, rec = recorded_case(name)
        h, h32 = rec["rms_history"], recorded_case(name, F32)[1]["rms_history"]
        angle, ss0 = residual(T, ALIGN_CASES[name][1])
        out[name] = {"rms_first_over_diagonal": h[0] / TARGET_DIAGONAL, "rms_last_over_diagonal": h[-1] / TARGET_DIAGONAL, "fall": h[0] / h[-1],
                     "residual_degrees": angle, "scale_product": ss0, "start": rec["start"], "iterations": len(h) - 1,
                     "float32_history_max_abs": max(abs(a - b) for a, b in zip(h, h32))}
    v, f, rv, rf, T0, kw = align_inputs("far")
    T, st = align(v, f, rv, rf, only_start=0, **{k: x for k, x in kw.items() if k != "starts"})
    out["far"].update(start0_alone_rms_over_diagonal=st["rms_history"][-1] / TARGET_DIAGONAL, start0_alone_residual_degrees=residual(T, T0)[0])
    v, f, rv, rf, T0, kw = align_inputs("floater_trim")
    T, st = align(v, f, rv, rf, **dict(kw, iterations=60))
    out["floater_trim"].update(residual_degrees_after_60_iterations=residual(T, T0)[0], scale_product_after_60_iterations=residual(T, T0)[1])
    return out


if __name__ == "__main__":
    import sys
    if sys.argv[1:2] == ["--premises"]:                # python tests/mesh_align_ref.py --premises profiles/mesh_align_premises.json
        with open(sys.argv[2], "w") as fh:
            json.dump(premises(), fh, indent=1, sort_keys=True)
            fh.write("\n")
    else:                                              # python tests/mesh_align_ref.py [case ..]
        record_cases(sys.argv[1:] or None)
