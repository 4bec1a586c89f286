"""The gfx950 mesh alignment (csrc_recon/meshalign.hip, v3d_amd/recon/mesh_align.py, scripts/pub/score_mesh.py) against the torch
restatement (tests/mesh_align_ref.py): one step of the registration on 1 .. 700 samples with misses, bad samples and a bad face, the rows of
sums against fp64 sums of the kernel's own outputs, the reduction bit for bit, guards around every output, the ICP on the three scenes whose
premises tests/test_mesh_align_cpu.py holds, the scores, and the script.

The bar for continuous outputs is that of tests/test_mesh_bake_gpu.py: the kernel may be off from the fp64 restatement by 4x what the
restatement's own float32 run is off, the float32 figure taken over the whole case, once.  The sums have a derived bound instead: two
summations of the same n terms in different orders differ by at most n 2^-52 sum |terms| (each is within (n - 1) 2^-53 sum |terms| of the
exact sum).  The ICP runs of the restatement are read from tests/golden/mesh_align_cases.json, which the CPU test holds to a fresh run."""
import functools
import importlib.util
import json
import math
import os

import numpy as np
import pytest
import torch

import mesh_align_ref as A
import mesh_query_ref as Q
import mesh_solid_ref as S
from conftest import record_parity
from v3d_amd.recon import geometry as G
from v3d_amd.recon import mesh_align as MA
from v3d_amd.recon import mesh_bake as MB
from v3d_amd.recon import mesh_query as MQ
from v3d_amd.recon import mesh_solid as MS

pytestmark = pytest.mark.gpu
DEV = "cuda"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F64, F32 = torch.float64, torch.float32
INF = float("inf")
GUARD = 4096
COUNTS = (1, 63, 64, 65, 700)
EPS52 = 2.0 ** -52


class Guarded:
    """An output of n rows with GUARD sentinel elements before and after it"""

    def __init__(self, n, width, dtype, sentinel):
        self.n, self.width, self.sentinel = n, width, sentinel
        self.buf = torch.full((2 * GUARD + n * width,), sentinel, dtype=dtype, device=DEV)

    @property
    def ptr(self):
        return self.buf.data_ptr() + GUARD * self.buf.element_size()

    def take(self):
        assert bool((self.buf[:GUARD] == self.sentinel).all()) and bool((self.buf[GUARD + self.n * self.width:] == self.sentinel).all()), "a guard was written"
        out = self.buf[GUARD:GUARD + self.n * self.width]
        return (out.reshape(self.n, self.width) if self.width > 1 else out).clone()


@functools.lru_cache(maxsize=None)
def target_bvh():
    return MB.build_bvh(*A.target())


@functools.lru_cache(maxsize=None)
def samples():
    """700 of the target's own n = 2 samples under the known motion, shuffled once: (points, weights) float32"""
    v, f = A.target()
    pts, w, _ = Q.face_samples(A.move(v, A.KNOWN), f, 2)
    perm = torch.randperm(pts.shape[0], generator=torch.Generator().manual_seed(21))[:700]
    return pts.float()[perm].contiguous(), w.float()[perm].contiguous()


BACK = np.linalg.inv(A.KNOWN) @ A.similarity(3.0, (3, 1, 2), 1.02, (0.01, 0.02, -0.01))       # nearly back: a few percent of the diagonal off


def same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.cpu().contiguous().view(torch.uint8), b.cpu().contiguous().view(torch.uint8))


def butterfly(rows):
    """THE BUTTERFLY of the header over [64, C] float64, in numpy: every lane's result (all equal)"""
    v = np.array(rows, dtype=np.float64)
    lane = np.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        v = v + v[lane ^ o]
    assert (v == v[0]).all()
    return v[0]


def check_step(bvh, verts, faces, p, w, T, max_dist, label):
    """One correspond against everything the header says of it; returns the dict on the host"""
    n = p.shape[0]
    r = {k: (x.cpu() if torch.is_tensor(x) else x) for k, x in MA.correspond(bvh, p, w, T, max_dist).items()}
    again = MA.correspond(bvh, p, w, T, max_dist)
    assert all(same_bits(r[k], again[k]) for k in r), "two runs differ"
    rows = (n + 63) // 64
    assert r["sums"].dtype == F64 and r["sums"].device.type == "cpu" and tuple(r["partials"].shape) == (rows, 20) and r["face"].dtype == torch.int32
    # dist, face, uv: the closest-point entry on the kernel's own moved, bit for bit
    dist, face, uv = [x.cpu() for x in MQ.closest_points(bvh, r["moved"], max_dist)]
    assert same_bits(r["dist"], dist) and same_bits(r["face"], face) and same_bits(r["uv"], uv)
    miss = r["face"] < 0
    assert bool(torch.isnan(r["closest"][miss]).all()) and bool((r["dist"][miss] == INF).all()) and not r["uv"][miss].any()
    # closest: rebuilt from (face, uv)
    q64, q32 = A.rebuild(verts, faces, r["face"], r["uv"], F64), A.rebuild(verts, faces, r["face"], r["uv"], F32)
    found = ~miss
    qbar = S.float_bar(q64[found], q32[found]) if bool(found.any()) else 0.0
    qerr = float((r["closest"].double() - q64)[found].abs().max()) if bool(found.any()) else 0.0
    fl = faces.long()[r["face"].long().clamp_min(0)]
    for col, k in ((0, 1), (1, 2)):                    # a vertex is itself
        at = found & (r["uv"][:, col] == 1)
        assert torch.equal(r["closest"][at], verts[fl[at, k]])
    # the rows and the sums: fp64 sums of the kernel's own per-sample outputs
    t = A.pair_terms(r["moved"], r["closest"], r["dist"], r["face"].long(), w)
    valid = torch.isfinite(r["moved"]).all(1) & torch.isfinite(w) & (w >= 0)
    worst = 0.0
    for b in range(rows):
        tb = t[64 * b:64 * b + 64]
        bound = tb.shape[0] * EPS52 * tb.abs().sum(0)
        diff = (r["partials"][b] - tb.sum(0)).abs()
        assert bool((diff <= bound).all()), (label, b, diff, bound)
        assert float(r["partials"][b, 18]) == float((valid & found)[64 * b:64 * b + 64].sum())
        lanes = np.zeros((64, 20))                     # and bit for bit: the header's terms (no contraction) through the header's butterfly
        lanes[:tb.shape[0]] = tb.numpy()
        assert same_bits(r["partials"][b], torch.from_numpy(butterfly(lanes))), (label, b)
        worst = max(worst, float((diff / bound.clamp_min(1e-300)).max()))
    diff, bound = (r["sums"] - t.sum(0)).abs(), n * EPS52 * t.abs().sum(0)
    assert bool((diff <= bound).all()), (label, diff, bound)
    lanes = np.zeros((64, 20))
    for b in range(rows):                              # the reduction's order replayed on the kernel's own rows
        lanes[b % 64] = lanes[b % 64] + r["partials"][b].numpy()
    assert same_bits(r["sums"], torch.from_numpy(butterfly(lanes))), label
    assert float(r["sums"][18]) == float((valid & found).sum())
    assert float(r["sums"][19]) >= float(r["sums"][0]) >= 0
    r["_figures"] = {"closest_max_abs": qerr, "closest_bar": qbar, "row_sum_error_over_bound": worst,
                     "sum_error_over_bound": float((diff / bound.clamp_min(1e-300)).max()), "counted": int((valid & found).sum()), "samples": n}
    assert qerr <= qbar, (label, qerr, qbar)
    return r


def guarded_step(bvh, p, w, T, max_dist, expect):
    """the two entries called by hand with guards around every output; the same bits as `expect`"""
    n = p.shape[0]
    rows = (n + 63) // 64
    pd, wd = p.to(DEV).contiguous(), w.to(DEV).contiguous()
    xf = np.ascontiguousarray(np.asarray(T, dtype=np.float64)[:3].astype(np.float32))
    outs = {"moved": Guarded(n, 3, F32, -7.0), "closest": Guarded(n, 3, F32, -7.0), "dist": Guarded(n, 1, F32, -7.0), "face": Guarded(n, 1, torch.int32, -7),
            "uv": Guarded(n, 2, F32, -7.0), "partials": Guarded(rows, 20, F64, -7.0)}
    sums = Guarded(1, 20, F64, -7.0)
    lib = G.load_library()
    G._check(lib, lib.v3d_recon_align_correspond(pd.data_ptr(), wd.data_ptr(), n, xf.ctypes.data, max_dist, *bvh._args(), *(outs[k].ptr for k in
                                                 ("moved", "closest", "dist", "face", "uv", "partials")), G._stream()), "align_correspond")
    G._check(lib, lib.v3d_recon_align_reduce(outs["partials"].ptr, rows, sums.ptr, G._stream()), "align_reduce")
    for k, g in outs.items():
        assert same_bits(g.take().reshape(expect[k].shape), expect[k]), k
    assert same_bits(sums.take().reshape(20), expect["sums"])


# ---- 1. one step ----------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def step_reference():
    """the restatement of all 700 samples under BACK, fp64 and float32, computed once"""
    v, f = A.target()
    p, w = samples()
    return A.correspond(v, f, p, w, BACK, INF, F64), A.correspond(v, f, p, w, BACK, INF, F32)


@pytest.mark.parametrize("n", COUNTS)
def test_correspond_matches_the_restatement(n):
    v, f = A.target()
    p, w = samples()
    r64, r32 = step_reference()
    mbar = S.float_bar(r64["moved"], r32["moved"])                                # over all 700 samples
    dbar = S.float_bar(r64["dist"], r32["dist"])
    r = check_step(target_bvh(), v, f, p[:n], w[:n], BACK, INF, f"plain-{n}")
    merr = float((r["moved"].double() - r64["moved"][:n]).abs().max())
    derr = float((r["dist"].double() - r64["dist"][:n]).abs().max())
    sure = r64["runner"][:n] - r64["dist"][:n] > Q.FACE_GAP
    assert torch.equal(r["face"].long()[sure], r64["face"][:n][sure])
    rms_err = abs(A.rms_of(r["sums"]) - A.rms_of(A.pair_terms(r64["moved"][:n], r64["closest"][:n], r64["dist"][:n], r64["face"][:n], w[:n].double()).sum(0)))
    record_parity(f"mesh_align_correspond[{n}]", dict(r["_figures"], moved_max_abs=merr, moved_bar=mbar, dist_max_abs=derr, dist_bar=dbar, rms_abs=rms_err))
    assert merr <= mbar and derr <= dbar and rms_err <= dbar
    if n in (65, 700):
        guarded_step(target_bvh(), p[:n], w[:n], BACK, INF, r)


@pytest.mark.parametrize("n", COUNTS)
def test_correspond_with_a_bound_and_samples_that_do_not_count(n):
    v, f = A.target()
    p, w = samples()
    p, w = p[:n].clone(), w[:n].clone()
    r64, _ = step_reference()
    md = float(r64["dist"].float().median())                                       # about half of the 700 miss
    bad = {}
    if n == 700:
        p[3, 1] = float("nan")
        p[10, 0] = INF
        w[20], w[30], w[40] = -1.0, float("nan"), 0.0
        bad = {"nan": 3, "inf": 10}
    r = check_step(target_bvh(), v, f, p, w, BACK, md, f"bound-{n}")
    for i in bad.values():
        assert not bool(torch.isfinite(r["moved"][i]).any()) and int(r["face"][i]) == -1 and float(r["dist"][i]) == INF
        assert bool(torch.isnan(r["closest"][i]).all()) and not r["uv"][i].any()
    if n == 700:
        assert bool(torch.isnan(r["moved"][3]).all())
        share = float((r["face"] < 0).float().mean())
        assert 0.3 < share < 0.7, share
        for i in (20, 30, 40):                         # the weight changes no per-sample output
            assert math.isfinite(float(r["moved"][i].sum()))
        valid = torch.isfinite(r["moved"]).all(1) & torch.isfinite(w) & (w >= 0)
        found = r["face"] >= 0
        w64 = w.double()
        assert float(r["sums"][19]) == pytest.approx(float(w64[valid].sum()), rel=1e-12)
        assert float(r["sums"][0]) == pytest.approx(float(w64[valid & found].sum()), rel=1e-12)
        assert float(r["sums"][19]) > float(r["sums"][0]) > 0                      # valid samples that missed count for column 19 alone
        assert int(r["sums"][18]) == int((valid & found).sum()) < int(found.sum()) + (0 if bool(found[[20, 30]].any()) else 1)
        guarded_step(target_bvh(), p, w, BACK, md, r)
    if n == 65:
        guarded_step(target_bvh(), p, w, BACK, md, r)
    record_parity(f"mesh_align_correspond_bound[{n}]", dict(r["_figures"], max_dist=md))


def test_identity_zero_scale_and_a_face_outside_the_vertices():
    v, f = A.target()
    p, w = samples()
    p, w = p[:130], w[:130]
    r = check_step(target_bvh(), v, f, p, w, np.eye(4), INF, "identity")
    assert same_bits(r["moved"], p)
    Z = np.zeros((4, 4))
    Z[:3, 3], Z[3, 3] = (0.3, -0.2, 0.1), 1.0
    r = check_step(target_bvh(), v, f, p, w, Z, INF, "zero-scale")
    assert torch.equal(r["moved"], torch.tensor([0.3, -0.2, 0.1]).expand(130, 3))
    assert len(set(r["dist"].tolist())) == 1 and len(set(r["face"].tolist())) == 1
    fb = f.clone()
    fb[5, 2], fb[77, 0], fb[900, 1] = v.shape[0] + 3, -1, 2 ** 31 - 1
    bvh = MB.build_bvh(v, fb)
    r64, r32 = A.correspond(v, fb, p, w, BACK, INF, F64), A.correspond(v, fb, p, w, BACK, INF, F32)
    r = check_step(bvh, v, fb, p, w, BACK, INF, "bad-face")
    assert not bool(torch.isin(r["face"], torch.tensor([5, 77, 900], dtype=torch.int32)).any())
    derr, dbar = float((r["dist"].double() - r64["dist"]).abs().max()), S.float_bar(r64["dist"], r32["dist"])
    record_parity("mesh_align_correspond_bad_face", dict(r["_figures"], dist_max_abs=derr, dist_bar=dbar))
    assert derr <= dbar


@pytest.mark.parametrize("rows", COUNTS)
def test_align_reduce_adds_the_rows_in_the_order_of_the_header(rows):
    g = torch.Generator().manual_seed(rows)
    part = (torch.randn(rows, 20, generator=g, dtype=F64) * torch.logspace(-6, 6, 20, dtype=F64)).contiguous()
    lanes = np.zeros((64, 20))
    for r in range(rows):                              # lane l adds rows l, l + 64, ... in increasing order
        lanes[r % 64] = lanes[r % 64] + part[r].numpy()
    expect = torch.from_numpy(butterfly(lanes))
    pd, sums = part.to(DEV), Guarded(1, 20, F64, -7.0)
    lib = G.load_library()
    for _ in range(2):
        G._check(lib, lib.v3d_recon_align_reduce(pd.data_ptr(), rows, sums.ptr, G._stream()), "align_reduce")
        assert same_bits(sums.take().reshape(20), expect)
    assert torch.equal(pd.cpu(), part)


# ---- 2. the ICP -----------------------------------------------------------------------------------------------------------------------------
def run_case(name):
    v, f, rv, rf, T0, kw = A.align_inputs(name)
    T, st = MA.align_mesh(v, f, rv, rf, **kw)
    T2, st2 = MA.align_mesh(v, f, rv, rf, **kw)
    assert T.dtype == np.float64 and T.shape == (4, 4) and T.tobytes() == T2.tobytes() and st["rms_history"] == st2["rms_history"], "two runs differ"
    _, rec = A.recorded_case(name)
    bar = A.history_bar(name)
    h = st["rms_history"]
    assert len(h) == len(rec["rms_history"]) == st["iterations_run"] + 1 and st["rms"] == h[-1]
    err = max(abs(a - b) for a, b in zip(h, rec["rms_history"]))
    angle, ss0 = A.residual(T, T0)
    print(f"{name}: history off by {err:.3e} (bar {bar:.3e}); rms {h[0]:.3e} -> {h[-1]:.3e}, {angle:.3f} deg, s s0 {ss0:.5f}, start {st['start']}")
    record_parity(f"mesh_align_icp[{name}]", {"history_max_abs": err, "history_bar": bar, "rms_first": h[0], "rms_last": h[-1], "residual_degrees": angle,
                                                "scale_product": ss0, "start": st["start"], "iterations_run": st["iterations_run"], "seconds": st["seconds"]})
    assert st["start"] == rec["start"]
    for key in ("scale", "rotation_angle", "translation", "counted_share", "seconds", "start_rms", "samples", "mode", "max_dist"):
        assert key in st
    return T, st, T0, err, bar, angle, ss0


def test_align_mesh_recovers_the_known_motion():
    T, st, T0, err, bar, angle, ss0 = run_case("recovery")
    h = st["rms_history"]
    assert h[0] / h[-1] >= 50 and angle <= 1.0 and abs(ss0 - 1) <= 1e-3
    assert err <= bar
    assert st["counted_share"] == 1.0 and st["samples"] == 1280 and st["start_rms"] is None


def test_align_mesh_stops_early_where_the_restatement_stops():
    T, st, T0, err, bar, angle, ss0 = run_case("early")
    assert st["iterations_run"] == A.EARLY_ITERATIONS == len(A.recorded_case("early")[1]["rms_history"]) - 1 < 60
    assert err <= bar
    v, f, rv, rf, _, _ = A.align_inputs("early")
    again = MA.correspond(target_bvh(), *MQ.face_samples(v, f, 1), T)              # the matrix returned is the one measured last
    assert A.rms_of(again["sums"]) == st["rms"]


def test_align_mesh_rigid_and_none():
    T, st, T0, err, bar, angle, ss0 = run_case("rigid")
    assert st["scale"] == pytest.approx(1.0, abs=1e-12) and angle <= 1.0 and st["rms_history"][0] / st["rms_history"][-1] >= 50
    assert err <= bar
    v, f, rv, rf, _, _ = A.align_inputs("recovery")
    I, sn = MA.align_mesh(v, f, rv, rf, mode="none", subdivide=1)
    assert np.array_equal(I, np.eye(4)) and sn["iterations_run"] == 0 and len(sn["rms_history"]) == 1
    ref = A.correspond(rv, rf, *[x.float() for x in Q.face_samples(v, f, 1)[:2]], np.eye(4))
    assert sn["rms"] == pytest.approx(A.rms_of(ref["sums"]), rel=1e-5)


def test_align_mesh_from_a_far_start_needs_the_24_starts():
    T, st, T0, err, bar, angle, ss0 = run_case("far")
    v, f, rv, rf, _, kw = A.align_inputs("far")
    _, alone = MA.align_mesh(v, f, rv, rf, **dict(kw, starts=1))
    assert alone["rms"] > 10 * st["rms"] and angle <= 1.0 and st["start"] != 0
    rec = A.recorded_case("far")[1]
    serr = max(abs(a - b) for a, b in zip(st["start_rms"], rec["start_rms"]))
    sbar = 4.0 * max(abs(a - b) for a, b in zip(A.recorded_case("far", F32)[1]["start_rms"], rec["start_rms"]))
    record_parity("mesh_align_icp[far-starts]", {"start_rms_max_abs": serr, "start_rms_bar": sbar, "alone_rms": alone["rms"]})
    assert serr <= sbar
    assert err <= bar


def test_align_mesh_trim_lets_a_floater_go():
    T1, st1, T0, err1, bar1, a1, s1 = run_case("floater")
    T9, st9, _, err9, bar9, a9, s9 = run_case("floater_trim")
    assert a1 > 5.0
    assert a9 <= 1.5 and abs(s9 - 1.0) <= 0.02
    assert 0.9 <= st9["counted_share"] < 0.93 and math.isfinite(st9["max_dist"]) and st1["max_dist"] == INF
    assert err1 <= bar1
    assert err9 <= bar9


# ---- 3. the scores --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pair", A.SCORE_PAIRS)
def test_score_meshes_against_the_restatement(pair):
    av, af, bv, bf = A.score_pair(pair)
    s = MA.score_meshes(av, af, bv, bf, thresholds=A.THRESHOLDS, iou_resolution=0)
    assert s["volume_iou"] is None
    d = MQ.mesh_distance(av, af, bv, bf)
    assert all(s[k] == d[k] for k in d if k != "seconds") and len(s["fscore"]) == 3
    ref = A.score_case(pair)
    diag = d["diagonal"]
    figures = {}
    for direction, key in (("a_to_b", "precision"), ("b_to_a", "recall")):
        r64, r32 = ref[(direction, F64)], ref[(direction, F32)]
        err = S.float_bar(r64["dist"], r32["dist"])    # a sample whose fp64 distance lies this near a threshold may fall either side
        werr = 4.0 * float((r32["weights"] - r64["weights"]).abs().sum() / r64["weights"].sum())
        for row in s["fscore"]:
            lo, hi = A.share_interval(r64["dist"], r64["weights"], row["threshold"] * diag, err)
            assert row["distance"] == row["threshold"] * diag
            assert lo - werr <= row[key] <= hi + werr, (pair, key, row, lo, hi)
            figures[f"{key}@{row['threshold']}"] = [lo, row[key], hi]
        nbar = A.normal_bar(r64, r32)
        nerr = abs(s["normal_consistency"][direction] - r64["nc"])
        figures[f"normal_consistency_{direction}"] = {"abs_error": nerr, "bar": nbar, "value": s["normal_consistency"][direction]}
        assert nerr <= nbar, (pair, direction, nerr, nbar)
    for row in s["fscore"]:
        p, r = row["precision"], row["recall"]
        assert row["fscore"] == (2 * p * r / (p + r) if p + r > 0 else 0.0)
    nc = s["normal_consistency"]
    assert nc["mean"] == 0.5 * (nc["a_to_b"] + nc["b_to_a"])
    record_parity(f"mesh_align_score[{pair}]", figures)


@pytest.mark.parametrize("pair", A.SCORE_PAIRS)
@pytest.mark.parametrize("N", A.IOU_RESOLUTIONS)
def test_volume_iou_counts_are_exact_off_the_cells_near_one_half(pair, N):
    av, af, bv, bf = A.score_pair(pair)
    wa, wb, bound = A.iou_case(pair, N)
    sure = A.iou_sure(wa, wb)
    assert 1.0 - float(sure.double().mean()) <= A.EXCLUDE_MAX
    iou = MA.score_meshes(av, af, bv, bf, iou_resolution=N)["volume_iou"]
    assert iou["resolution"] == N and iou["bound"] == pytest.approx(bound, rel=1e-6)
    c = MS.voxel_centres(N, iou["bound"])
    ga = (MS.winding_numbers(MB.build_bvh(av, af), c) >= 0.5).cpu()
    gb = (MS.winding_numbers(MB.build_bvh(bv, bf), c) >= 0.5).cpu()
    assert torch.equal(ga[sure], (wa >= 0.5)[sure]) and torch.equal(gb[sure], (wb >= 0.5)[sure])        # exact off the excluded cells
    counts = (int(ga.sum()), int(gb.sum()), int((ga & gb).sum()), int((ga | gb).sum()))
    assert (iou["inside_a"], iou["inside_b"], iou["intersection"], iou["union"]) == counts               # and the counts are those of the cells
    assert iou["iou"] == counts[2] / counts[3]
    cell = (2.0 * iou["bound"] / N) ** 3
    assert iou["volume_a"] == pytest.approx(counts[0] * cell) and iou["volume_b"] == pytest.approx(counts[1] * cell)
    ref = A.iou_counts(wa, wb)
    record_parity(f"mesh_align_iou[{pair}-{N}]", {"iou": iou["iou"], "iou_fp64": ref[2] / ref[3], "counts": list(counts), "counts_fp64": list(ref),
                                                  "left_out": 1.0 - float(sure.double().mean())})


# ---- 4. the script and the refusals -----------------------------------------------------------------------------------------------------------
def _entry(name):
    spec = importlib.util.spec_from_file_location("v3d_entry_" + name, os.path.join(ROOT, "scripts", "pub", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_score_mesh_script_end_to_end(tmp_path, capsys):
    v, f, rv, rf, T0, _ = A.align_inputs("recovery")
    colors = (rv - rv.min(0).values) / (rv.max(0).values - rv.min(0).values)
    mesh, gt, out, js = (str(tmp_path / n) for n in ("moved.ply", "gt.ply", "aligned.ply", "score.json"))
    G.save_mesh_ply(mesh, v, f, colors)
    G.save_mesh_ply(gt, rv, rf, colors)
    _entry("score_mesh").main(["--mesh", mesh, "--reference", gt, "--iterations", "60", "--subdivide", "1", "--iou_resolution", "16", "--json", js, "-o", out])
    printed = capsys.readouterr().out
    assert printed.count("[score] ") == 3 and "chamfer" in printed and "IoU 0." in printed
    text = open(js).read()
    assert "NaN" not in text and "Infinity" not in text
    d = json.loads(text)
    T = np.asarray(d["matrix"])
    assert T.shape == (4, 4) and d["alignment"]["mode"] == "similarity" and d["mesh_faces"] == d["reference_faces"] == 1280
    ov, of, oc = G.read_mesh_ply(out)
    assert np.array_equal(np.asarray(of), f.numpy()) and np.array_equal(np.asarray(oc), np.asarray(G.read_mesh_ply(mesh)[2]))
    ov = torch.as_tensor(np.asarray(ov))
    want64 = v.double() @ torch.as_tensor(T[:3, :3]).T + torch.as_tensor(T[:3, 3])
    want32 = (v @ torch.as_tensor(T[:3, :3]).float().T + torch.as_tensor(T[:3, 3]).float())
    bar = S.float_bar(want64, want32)
    err = float((ov.double() - want64).abs().max())
    # against the original: the residual of premise 1 (rotation <= 1 degree, scale within 1e-3) moves no vertex of a body of this diagonal
    # further than (1 degree in radians + 1e-3) x the diagonal
    off = float((ov.double() - rv.double()).norm(dim=1).max())
    record_parity("mesh_align_script", {"readback_max_abs": err, "readback_bar": bar, "largest_vertex_error": off, "fscore": d["fscore"], "iou": d["volume_iou"]["iou"]})
    assert err <= bar and off <= (math.radians(1.0) + 1e-3) * A.TARGET_DIAGONAL
    assert d["fscore"][2]["fscore"] > 0.99 and d["volume_iou"]["iou"] > 0.9


def test_empty_inputs_raise():
    v, f = A.coarse()
    for bad in ((v[:0], f[:0], v, f), (v, f[:0], v, f), (v, f, v, f[:0]), (v, f, v[:0], f[:0])):
        with pytest.raises(ValueError, match="align_mesh"):
            MA.align_mesh(*bad)
        with pytest.raises(ValueError, match="score_meshes"):
            MA.score_meshes(*bad)
    bvh = target_bvh()
    r = MA.correspond(bvh, torch.zeros(0, 3), torch.zeros(0), np.eye(4))           # no samples: no launch, zero sums
    assert r["moved"].shape == (0, 3) and r["partials"].shape == (0, 20) and not r["sums"].any()
    with pytest.raises(ValueError, match="correspond"):
        MA.correspond(bvh, torch.zeros(4, 3), torch.zeros(3), np.eye(4))
    with pytest.raises(ValueError, match="max_dist"):
        MA.correspond(bvh, torch.zeros(4, 3), torch.zeros(4), np.eye(4), max_dist=-1.0)
    with pytest.raises(ValueError, match="max_dist"):
        MA.correspond(bvh, torch.zeros(4, 3), torch.zeros(4), np.eye(4), max_dist=float("nan"))
