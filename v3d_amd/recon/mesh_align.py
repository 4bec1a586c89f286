"""Align a mesh to a reference and score it, on the gfx950 kernels of libv3d_recon.so (csrc_recon/meshalign.hip, include/v3d_recon.h "Mesh
alignment"): a point-to-surface ICP over the BVH of mesh_bake.py whose hot step (move every sample, find its closest point, reduce the 20
weighted moments of the pairs) is two launches and one read-back of 160 bytes, and the metrics that need a common frame: Chamfer distance
(mesh_query.mesh_distance), precision / recall / F-score at thresholds, normal consistency and volume IoU (mesh_solid.winding_numbers).

    bvh = mesh_bake.build_bvh(ref_verts, ref_faces)
    r = correspond(bvh, points, weights, transform, max_dist=inf)       # moved, closest, dist, face, uv, partials, sums [20] float64 (host)
    inc = solve_similarity(r["sums"], "similarity")                     # 4 x 4 float64: the next increment (pure host, Umeyama)
    matrix, stats = align_mesh(verts, faces, ref_verts, ref_faces, mode="similarity", starts=24)
    moved = transform_vertices(verts, matrix)
    s = score_meshes(moved, faces, ref_verts, ref_faces)                # chamfer, fscore, normal_consistency, volume_iou, ...

Not done: no point-to-plane step, no coarse-to-fine sampling, no symmetric (two-way) correspondences.  The point-to-surface iteration
converges linearly, which is why the default is 200 iterations with an early stop.

No atomics anywhere: two calls with the same arguments return bit-equal results.  Everything runs under no_grad.  There is no fallback:
without the libraries this raises."""
from __future__ import annotations

import itertools
import math
import time
from typing import Sequence

import numpy as np
import torch

from .geometry import _check, _stream, load_library
from .mesh_bake import MeshBVH, build_bvh
from .mesh_clean import _mesh_arg
from .mesh_query import MAX_SUBDIVIDE, _face_samples, _int_arg, _points_arg, closest_points, mesh_distance
from .mesh_render import _dev
from .mesh_solid import voxel_centres, winding_numbers

COLUMNS = 20
MODES = ("none", "rigid", "similarity")
IOU_BOUND = 1.05                   # x the largest |coordinate| of either mesh: the half-extent of the IoU grid (a choice)
IOU_SLAB_POINTS = 1 << 21          # voxels per winding-number launch


def cube_rotations() -> np.ndarray:
    """[24, 3, 3] float64: the proper rotations of the cube, row i of a matrix being sign[i] x the unit vector of axis perm[i], over
    itertools.permutations(range(3)) x itertools.product((1, -1), repeat=3) with determinant +1.  The first is the identity."""
    out = []
    for perm in itertools.permutations(range(3)):
        for signs in itertools.product((1, -1), repeat=3):
            R = np.zeros((3, 3))
            for i in range(3):
                R[i, perm[i]] = signs[i]
            if np.linalg.det(R) > 0:
                out.append(R)
    return np.stack(out)


def _matrix_arg(transform, who: str) -> np.ndarray:
    """a 4 x 4 float64 matrix from a 3 x 4 or 4 x 4 one"""
    m = np.asarray(transform.detach().cpu().numpy() if torch.is_tensor(transform) else transform, dtype=np.float64)
    if m.shape not in ((3, 4), (4, 4)):
        raise ValueError(f"{who}: transform must be 3 x 4 or 4 x 4, got {m.shape}")
    out = np.eye(4)
    out[:3] = m[:3]
    return out


def _max_dist_arg(max_dist, who: str) -> float:
    md = float(max_dist)
    if math.isnan(md) or md < 0:
        raise ValueError(f"{who}: max_dist {max_dist} must not be negative or NaN")
    return md


@torch.no_grad()
def correspond(bvh: MeshBVH, points, weights, transform, max_dist: float = math.inf) -> dict:
    """One step of the registration on the tree's device.  p' = M p with M the upper 3 x 4 of `transform` rounded to float32;  the closest
    point of the tree's mesh to every p' within max_dist (closed; +inf allowed) by the rules of mesh_query.closest_points.  Returns
    "moved", "closest" [N, 3], "dist" [N], "face" [N] int32, "uv" [N, 2] (a miss: closest NaN, +inf, -1, 0 0), "partials" [ceil(N / 64), 20]
    float64 and "sums" [20]: a float64 HOST tensor, the one read-back.  The columns (include/v3d_recon.h): sum w, sum w p', sum w q,
    sum w q_i p'_j, sum w |p'|^2, sum w dist^2, the samples that count, sum w over all valid samples."""
    md = _max_dist_arg(max_dist, "correspond")
    dev = bvh.verts.device
    p = _points_arg(points, dev, "correspond")
    w = _dev(weights, torch.float32, dev)
    N = p.shape[0]
    if w.dim() != 1 or w.shape[0] != N:
        raise ValueError(f"correspond: {N} points, weights of shape {tuple(w.shape)}")
    xf = np.ascontiguousarray(_matrix_arg(transform, "correspond")[:3].astype(np.float32))
    e = lambda *s: torch.empty(*s, dtype=torch.float32, device=dev)  # noqa: E731
    rows = (N + 63) // 64
    out = {"moved": e(N, 3), "closest": e(N, 3), "dist": e(N), "face": torch.empty(N, dtype=torch.int32, device=dev), "uv": e(N, 2),
           "partials": torch.empty(rows, COLUMNS, dtype=torch.float64, device=dev)}
    if N == 0:
        out["sums"] = torch.zeros(COLUMNS, dtype=torch.float64)
        return out
    sums = torch.empty(COLUMNS, dtype=torch.float64, device=dev)
    lib = load_library()
    _check(lib, lib.v3d_recon_align_correspond(p.data_ptr(), w.data_ptr(), N, xf.ctypes.data, md, *bvh._args(), out["moved"].data_ptr(),
                                               out["closest"].data_ptr(), out["dist"].data_ptr(), out["face"].data_ptr(), out["uv"].data_ptr(),
                                               out["partials"].data_ptr(), _stream()), "v3d_recon_align_correspond")
    _check(lib, lib.v3d_recon_align_reduce(out["partials"].data_ptr(), rows, sums.data_ptr(), _stream()), "v3d_recon_align_reduce")
    out["sums"] = sums.cpu()
    return out


def solve_similarity(sums, mode: str = "similarity") -> np.ndarray:
    """The 4 x 4 float64 matrix [s R | t] that best maps the p' onto their q in the weighted least-squares sense, from the 20 sums of
    correspond alone (weighted Umeyama / Kabsch;  pure host, float64).  With W = column 0: the means mu_p, mu_q, the centred
    cross-covariance C = sum w q p'^T / W - mu_q mu_p^T = U D V^T, S = diag(1, 1, det(U) det(V)) so that R = U S V^T is never a reflection,
    s = tr(D S) / var(p') for "similarity" and 1 for "rigid", t = mu_q - s R mu_p.  The identity when W is 0 or var(p') is not above 0."""
    if mode not in ("rigid", "similarity"):
        raise ValueError(f"solve_similarity: mode {mode!r} is not 'rigid' or 'similarity'")
    s = np.asarray(sums.detach().cpu().numpy() if torch.is_tensor(sums) else sums, dtype=np.float64).reshape(-1)
    if s.shape[0] != COLUMNS:
        raise ValueError(f"solve_similarity: {s.shape[0]} sums, not {COLUMNS}")
    out = np.eye(4)
    W = s[0]
    if not W > 0:
        return out
    mu_p, mu_q = s[1:4] / W, s[4:7] / W
    var = s[16] / W - mu_p @ mu_p
    if not var > 0:
        return out
    C = s[7:16].reshape(3, 3) / W - np.outer(mu_q, mu_p)
    U, D, Vt = np.linalg.svd(C)
    S = np.array([1.0, 1.0, 1.0 if np.linalg.det(U) * np.linalg.det(Vt) >= 0 else -1.0])
    R = (U * S) @ Vt
    scale = float((D * S).sum() / var) if mode == "similarity" else 1.0
    out[:3, :3] = scale * R
    out[:3, 3] = mu_q - scale * (R @ mu_p)
    return out


def decompose(matrix) -> dict:
    """{"scale", "rotation" [3, 3], "rotation_angle" (degrees), "translation" [3]} of a 4 x 4 similarity"""
    m = _matrix_arg(matrix, "decompose")
    A = m[:3, :3]
    det = float(np.linalg.det(A))
    scale = math.copysign(abs(det) ** (1.0 / 3.0), det)
    R = A / scale if scale != 0 else np.eye(3)
    angle = math.degrees(math.acos(min(1.0, max(-1.0, (float(np.trace(R)) - 1.0) / 2.0))))
    return {"scale": scale, "rotation": R, "rotation_angle": angle, "translation": m[:3, 3].copy()}


def start_transform(k: int, verts64: np.ndarray, ref64: np.ndarray, mode: str) -> np.ndarray:
    """Start k, 4 x 4 float64: rotation k of cube_rotations, then ("similarity" only) the scale that makes the diagonals of the two bounding
    boxes equal, then the shift that brings the centres of the two bounding boxes together"""
    R = cube_rotations()[k]
    r = verts64 @ R.T
    lo, hi, rlo, rhi = r.min(0), r.max(0), ref64.min(0), ref64.max(0)
    d = float(np.linalg.norm(hi - lo))
    s = float(np.linalg.norm(rhi - rlo)) / d if mode == "similarity" and d > 0 else 1.0
    out = np.eye(4)
    out[:3, :3] = s * R
    out[:3, 3] = 0.5 * (rlo + rhi) - s * 0.5 * (lo + hi)
    return out


def trim_distance(dist: torch.Tensor, weights: torch.Tensor, valid_weight: float, trim: float) -> float:
    """The smallest distance d such that the samples within d carry at least trim x valid_weight: a stable sort of the finite distances of
    the samples with a finite weight >= 0, a float64 cumulative sum of their weights;  the float32 above the distance found, so that the
    kernel's closed bound on d^2 keeps the sample itself.  +inf when nothing reaches the share."""
    ok = torch.isfinite(dist) & torch.isfinite(weights) & (weights >= 0)
    d, w = dist[ok], weights[ok].double()
    if d.numel() == 0:
        return math.inf
    ds, order = torch.sort(d, stable=True)
    cum = torch.cumsum(w[order], 0)
    hit = torch.nonzero(cum >= trim * valid_weight).reshape(-1)
    if hit.numel() == 0:
        return math.inf
    return float(np.nextafter(np.float32(float(ds[hit[0]])), np.float32(np.inf)))


def _rms(sums) -> float:
    return math.sqrt(float(sums[17]) / float(sums[0])) if float(sums[0]) > 0 else math.nan


def _icp(bvh, pts, w, T, mode, iterations, tol, trim):
    """(T, history, last measurement): `iterations` times measure at T, stop when the RMS moved by less than tol relative, else solve and
    compose;  a last measurement at the T returned, so history[-1] belongs to it and history has one entry more than there were solves"""
    hist, r, md = [], None, math.inf
    for it in range(iterations + 1):
        if trim < 1.0:
            u = correspond(bvh, pts, w, T, math.inf)
            md = trim_distance(u["dist"], w, float(u["sums"][19]), trim)
        r = correspond(bvh, pts, w, T, md)
        r["max_dist"] = md
        hist.append(_rms(r["sums"]))
        if it == iterations:
            break
        if tol > 0 and it > 0 and abs(hist[-2] - hist[-1]) < tol * hist[-2]:
            break
        T = solve_similarity(r["sums"], mode) @ T
    return T, hist, r


@torch.no_grad()
def align_mesh(verts, faces, ref_verts, ref_faces, mode: str = "similarity", starts: int = 1, iterations: int = 200, tol: float = 1e-5,
               trim: float = 1.0, subdivide: int = 2, start_iterations: int = 10, device="cuda"):
    """(matrix [4, 4] float64 numpy, stats): the similarity ("rigid": s = 1;  "none": the identity, and the figures of the pair as it is)
    that moves (verts, faces) onto the reference by point-to-surface ICP.  The samples are mesh_query.face_samples of the moving mesh at
    `subdivide` with their areas as weights;  the tree is built once on the reference.  The total transform is kept in float64 on the host
    and every iteration applies it to the ORIGINAL samples, rounded to float32 once, so nothing drifts;  the increment solved from the 20
    sums (solve_similarity) is composed onto it.  Start k (start_transform): rotation k of the 24 of the cube, the scale of the bounding
    boxes' diagonals ("similarity"), the shift of their centres.  starts = 1: start 0, the identity rotation.  starts = 24: every start
    runs start_iterations iterations, the one with the smallest weighted RMS (the lowest index on a tie) continues.  The run ends after
    `iterations` iterations or when the weighted RMS changes by less than tol relative (tol = 0: never early).  trim < 1: every iteration
    bounds its correspondences by trim_distance, the distance within which trim of the valid weight lies;  that costs a SECOND, unbounded
    correspond per iteration.  stats: "rms_history" (the weighted RMS before every solve and of the matrix returned: one entry more than
    "iterations_run"), "rms", "iterations_run", "start", "start_rms" (per start; None with starts = 1), "scale", "rotation_angle"
    (degrees), "translation", "counted_share" (column 0 over column 19 of the last measurement), "max_dist" (of the last measurement),
    "samples", "mode", "seconds".  A mesh without faces on either side raises ValueError."""
    who = "align_mesh"
    if mode not in MODES:
        raise ValueError(f"{who}: mode {mode!r} is not one of {MODES}")
    if starts not in (1, 24) or isinstance(starts, bool):
        raise ValueError(f"{who}: starts {starts!r} is not 1 or 24")
    iterations = _int_arg(iterations, 0, 1 << 20, who, "iterations")
    start_iterations = _int_arg(start_iterations, 0, 1 << 20, who, "start_iterations")
    n = _int_arg(subdivide, 1, MAX_SUBDIVIDE, who, "subdivide")
    tol, trim = float(tol), float(trim)
    if not (math.isfinite(tol) and tol >= 0):
        raise ValueError(f"{who}: tol {tol} must be finite and not negative")
    if not 0 < trim <= 1:
        raise ValueError(f"{who}: trim {trim} outside (0, 1]")
    v, f, _ = _mesh_arg(verts, faces, None, device, who)
    rv, rf, _ = _mesh_arg(ref_verts, ref_faces, None, device, who)
    for name, a, b in (("the mesh", v, f), ("the reference", rv, rf)):
        if a.shape[0] == 0 or b.shape[0] == 0:
            raise ValueError(f"{who}: {name} has {a.shape[0]} vertices and {b.shape[0]} faces: nothing to align")
    if f.shape[0] * n * n > 2 ** 31 - 1:
        raise ValueError(f"{who}: {f.shape[0]} faces x {n * n} samples do not fit int32")
    t0 = time.perf_counter()
    pts, w = _face_samples(v, f, n)
    bvh = build_bvh(rv, rf, device)
    v64, r64 = v.double().cpu().numpy(), rv.double().cpu().numpy()
    start, start_rms = 0, None
    if mode == "none":
        T, hist, last = _icp(bvh, pts, w, np.eye(4), "rigid", 0, 0.0, trim)
    elif starts == 1:
        T, hist, last = _icp(bvh, pts, w, start_transform(0, v64, r64, mode), mode, iterations, tol, trim)
    else:
        runs = [_icp(bvh, pts, w, start_transform(k, v64, r64, mode), mode, min(start_iterations, iterations), 0.0, trim) for k in range(24)]
        start_rms = [h[-1] for _, h, _ in runs]
        start = min(range(24), key=lambda k: (not math.isfinite(start_rms[k]), start_rms[k], k))
        T, head, last = runs[start]
        more = iterations - min(start_iterations, iterations)
        if more > 0:
            T, tail, last = _icp(bvh, pts, w, T, mode, more, tol, trim)
            hist = head + tail[1:]                     # (the tail's first measurement is the head's last over again)
        else:
            hist = head
    d = decompose(T)
    s19 = float(last["sums"][19])
    stats = {"rms_history": hist, "rms": hist[-1], "iterations_run": len(hist) - 1, "start": start, "start_rms": start_rms, "scale": d["scale"],
             "rotation_angle": d["rotation_angle"], "translation": d["translation"].tolist(),
             "counted_share": float(last["sums"][0]) / s19 if s19 > 0 else math.nan, "max_dist": last["max_dist"], "samples": int(pts.shape[0]),
             "mode": mode}
    if device != "cpu" and torch.cuda.is_available():
        torch.cuda.synchronize()
    stats["seconds"] = time.perf_counter() - t0
    return T, stats


def transform_vertices(verts, matrix) -> torch.Tensor:
    """verts [V, 3] moved by a 3 x 4 or 4 x 4 matrix: formed in float64, returned in the dtype and on the device of verts (float32 for an
    array that is not floating point)"""
    m = torch.from_numpy(_matrix_arg(matrix, "transform_vertices"))
    t = verts if torch.is_tensor(verts) else torch.from_numpy(np.ascontiguousarray(verts))
    if t.dim() != 2 or t.shape[1] != 3:
        raise ValueError(f"transform_vertices: verts must be [V, 3], got {tuple(t.shape)}")
    dtype = t.dtype if t.is_floating_point() else torch.float32
    m = m.to(t.device)
    return (t.double() @ m[:3, :3].T + m[:3, 3]).to(dtype)


# ---- the scores -----------------------------------------------------------------------------------------------------------------------------
def _unit_face_normals(v: torch.Tensor, f: torch.Tensor) -> torch.Tensor:
    """[F, 3] float32;  0 0 0 for a face without area"""
    fl = f.long()
    n = torch.linalg.cross(v[fl[:, 1]] - v[fl[:, 0]], v[fl[:, 2]] - v[fl[:, 0]])
    length = n.norm(dim=1, keepdim=True)
    return torch.where(length > 0, n / length.clamp_min(1e-38), torch.zeros_like(n))


def _one_way_scores(v, f, n: int, bvh: MeshBVH, taus: Sequence[float]):
    """(the share of (v, f)'s area within every tau of the tree's mesh, the normal consistency) over the samples of (v, f)"""
    pts, w = _face_samples(v, f, n)
    dist, face, _ = closest_points(bvh, pts)
    d, w64 = dist.double(), w.double()
    area = float(w64.sum())
    if not area > 0:
        return [math.nan] * len(taus), math.nan
    share = [float((w64 * (d <= tau)).sum()) / area for tau in taus]
    mine = _unit_face_normals(v, f).repeat_interleave(n * n, 0)
    other = _unit_face_normals(bvh.verts, bvh.faces)[face.long().clamp_min(0)]
    dot = torch.where(face >= 0, (mine * other).sum(1).abs(), torch.zeros_like(dist))
    return share, float((dot.double() * w64).sum()) / area


@torch.no_grad()
def volume_iou(a_bvh: MeshBVH, b_bvh: MeshBVH, resolution: int, bound: float) -> dict:
    """Occupancy winding_numbers >= 0.5 of both meshes at mesh_solid.voxel_centres(resolution, bound), in slabs of whole z layers:
    {"iou", "inside_a", "inside_b", "intersection", "union" (int64 counts), "volume_a", "volume_b", "resolution", "bound"}"""
    N = int(resolution)
    dev = a_bvh.verts.device
    layers = max(1, IOU_SLAB_POINTS // (N * N))
    ia = ib = both = 0
    for z in range(0, N, layers):                      # (the centres are formed slab by slab too: no N^3 tensor at all)
        p = voxel_centres(N, bound, dev, layers=(z, min(z + layers, N)))
        oa, ob = winding_numbers(a_bvh, p) >= 0.5, winding_numbers(b_bvh, p) >= 0.5
        ia += int(oa.sum(dtype=torch.int64))
        ib += int(ob.sum(dtype=torch.int64))
        both += int((oa & ob).sum(dtype=torch.int64))
    union = ia + ib - both
    cell = (2.0 * float(bound) / N) ** 3
    return {"iou": both / union if union else math.nan, "inside_a": ia, "inside_b": ib, "intersection": both, "union": union,
            "volume_a": ia * cell, "volume_b": ib * cell, "resolution": N, "bound": float(bound)}


@torch.no_grad()
def score_meshes(a_verts, a_faces, b_verts, b_faces, thresholds: Sequence[float] = (0.01, 0.02, 0.05), iou_resolution: int = 128,
                 subdivide: int = 2, device="cuda") -> dict:
    """How good mesh A is against the reference B, both in ONE frame (align_mesh first).  Everything mesh_query.mesh_distance returns
    (Chamfer among it), and
      "fscore": per threshold tau (x the diagonal of B's bounding box) {"threshold", "distance", "precision": the area-weighted share of A's
        samples within tau of B, "recall": the same from B to A, "fscore": 2 P R / (P + R), 0 when both are 0};
      "normal_consistency": {"a_to_b", "b_to_a", "mean"}: the area-weighted mean of |n of the sample's face . n of the closest face|, a face
        without area counting as 0, summed in float64;
      "volume_iou": volume_iou at `iou_resolution` voxels on a side of the cube of half-extent 1.05 x the largest |coordinate| of either
        mesh (None with iou_resolution = 0).  The faces must be wound outward (mesh_solid).
    The samples are queried once by mesh_distance and once more here: its dict keeps no per-sample distances."""
    who = "score_meshes"
    n = _int_arg(subdivide, 1, MAX_SUBDIVIDE, who, "subdivide")
    res = _int_arg(iou_resolution, 0, 1024, who, "iou_resolution")
    taus = [float(t) for t in thresholds]
    if any(not (math.isfinite(t) and t > 0) for t in taus):
        raise ValueError(f"{who}: thresholds {list(thresholds)} must be finite and positive")
    av, af, _ = _mesh_arg(a_verts, a_faces, None, device, who)
    bv, bf, _ = _mesh_arg(b_verts, b_faces, None, device, who)
    for name, v, f in (("the mesh", av, af), ("the reference", bv, bf)):
        if v.shape[0] == 0 or f.shape[0] == 0:
            raise ValueError(f"{who}: {name} has {v.shape[0]} vertices and {f.shape[0]} faces: nothing to score")
    t0 = time.perf_counter()
    out = mesh_distance(av, af, bv, bf, subdivide=n, device=device)
    diag = out["diagonal"]
    a_bvh, b_bvh = build_bvh(av, af, device), build_bvh(bv, bf, device)
    dists = [t * diag for t in taus]
    prec, nc_ab = _one_way_scores(av, af, n, b_bvh, dists)
    rec, nc_ba = _one_way_scores(bv, bf, n, a_bvh, dists)
    out["fscore"] = [{"threshold": t, "distance": d, "precision": p, "recall": r, "fscore": 2 * p * r / (p + r) if p + r > 0 else 0.0}
                     for t, d, p, r in zip(taus, dists, prec, rec)]
    out["normal_consistency"] = {"a_to_b": nc_ab, "b_to_a": nc_ba, "mean": 0.5 * (nc_ab + nc_ba)}
    out["volume_iou"] = None
    if res:
        bound = IOU_BOUND * max(float(av.abs().max()), float(bv.abs().max()))
        out["volume_iou"] = volume_iou(a_bvh, b_bvh, res, bound if bound > 0 else 1.0)
    if device != "cpu" and torch.cuda.is_available():
        torch.cuda.synchronize()
    out["seconds"] = time.perf_counter() - t0
    return out
