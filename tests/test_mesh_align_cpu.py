"""What holds of the mesh alignment without a GPU: the header, the entries and the ctypes table agree and every entry refuses bad arguments
before a launch;  solve_similarity against the restatement (tests/mesh_align_ref.py);  the 24 starts;  the script's options;  and the premises
of tests/test_mesh_align_gpu.py asserted on the fp64 restatement, so that a change of scene fails here and not as a flaky GPU test."""
import importlib.util
import json
import math
import os
import re
import sys

import numpy as np
import pytest
import torch

import mesh_align_ref as A
import mesh_query_ref as Q
from v3d_amd.recon import mesh_align as MA                                      # (without the feature: the import fails)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = {"v3d_recon_align_correspond", "v3d_recon_align_reduce"}
F64, F32 = torch.float64, torch.float32


@pytest.fixture(scope="module")
def lib():
    from v3d_amd.build import build_recon
    from v3d_amd.recon import geometry
    build_recon(verbose=False)
    return geometry.load_library()


# ---- the library ----------------------------------------------------------------------------------------------------------------------------
def test_header_declares_and_library_exports_the_entries(lib):
    from v3d_amd.recon import geometry
    hdr = open(os.path.join(ROOT, "include", "v3d_recon.h")).read()
    declared = set(re.findall(r"\b(v3d_recon_[a-z_0-9]+)\s*\(", hdr))
    assert ENTRIES <= declared and declared == set(geometry.SIGNATURES)
    for name in ENTRIES:
        assert hasattr(lib, name), f"{name} is not exported"
        proto = re.search(r"\bint " + name + r"\s*\(([^;]*)\);", hdr).group(1)
        assert len(proto.split(",")) == len(geometry.SIGNATURES[name][1]), f"{name}: the ctypes row and the prototype differ in length"
    assert lib.v3d_recon_abi_version() == geometry.ABI_VERSION == 1              # the new entries are additive
    assert int(re.search(r"#define V3D_RECON_ABI_VERSION (\d+)", hdr).group(1)) == 1
    assert int(re.search(r"#define V3D_RECON_ALIGN_COLUMNS (\d+)", hdr).group(1)) == MA.COLUMNS == A.COLUMNS == 20
    assert "Mesh alignment" in hdr and "THE BUTTERFLY" in hdr
    src = open(os.path.join(ROOT, "v3d_amd", "csrc_recon", "meshalign.hip")).read()
    assert "atomic" not in src.replace("No atomics", "")
    assert '#include "bvh_walk.h"' in src and "closest_point(tr," in src
    for reused in ("Near closest_point(", "void near_triangle(", "float box_d2("):  # reused, not rewritten
        assert reused not in src


def test_bad_arguments_are_refused_before_any_launch(lib):
    # (no GPU here: an entry that reached its launch would fail differently, or crash; `p` is never dereferenced by the device-less host code
    # but for xf, which the entry reads on the host: a real array)
    p = 0x1000
    xf = np.eye(4, dtype=np.float32)[:3].copy()
    x = xf.ctypes.data
    err = lambda: lib.v3d_recon_last_error().decode()  # noqa: E731
    tree = (p, p, p, p, p, p, 5, p, 4)

    def correspond(points=p, weights=p, n=3, m=x, md=1.0, tr=tree, outs=(p, p, p, p, p, p)):
        return lib.v3d_recon_align_correspond(points, weights, n, m, md, *tr, *outs, None)

    def refused(rc, name, word):
        assert rc == -1, name
        assert name in err() and word in err(), err()

    refused(correspond(points=None), "v3d_recon_align_correspond", "null")
    refused(correspond(weights=None), "v3d_recon_align_correspond", "null")
    refused(correspond(m=None), "v3d_recon_align_correspond", "null")
    for k in range(6):
        refused(correspond(outs=tuple(None if j == k else p for j in range(6))), "v3d_recon_align_correspond", "null")
    for k in (0, 1, 2, 3, 4, 5, 7):
        refused(correspond(tr=tuple(None if j == k else t for j, t in enumerate(tree))), "v3d_recon_align_correspond", "null")
    refused(correspond(tr=(p, p, p, p, p, p, 0, p, 4)), "v3d_recon_align_correspond", "num_verts")
    refused(correspond(tr=(p, p, p, p, p, p, 5, p, 0)), "v3d_recon_align_correspond", "num_faces")
    refused(correspond(tr=(p, p, p, p, p, p, 5, p, 2 ** 30 + 1)), "v3d_recon_align_correspond", "num_faces")
    refused(correspond(n=0), "v3d_recon_align_correspond", "num_points")
    refused(correspond(n=-1), "v3d_recon_align_correspond", "num_points")
    refused(correspond(md=-1.0), "v3d_recon_align_correspond", "max_dist")
    refused(correspond(md=float("nan")), "v3d_recon_align_correspond", "max_dist")
    refused(lib.v3d_recon_align_reduce(None, 3, p, None), "v3d_recon_align_reduce", "null")
    refused(lib.v3d_recon_align_reduce(p, 3, None, None), "v3d_recon_align_reduce", "null")
    refused(lib.v3d_recon_align_reduce(p, 0, p, None), "v3d_recon_align_reduce", "num_rows")
    refused(lib.v3d_recon_align_reduce(p, -4, p, None), "v3d_recon_align_reduce", "num_rows")


def test_host_api_refuses_bad_arguments_with_its_name():
    v, f = A.coarse()
    for kw in ({"mode": "affine"}, {"starts": 2}, {"starts": True}, {"iterations": -1}, {"iterations": 2.5}, {"tol": -1.0}, {"tol": float("nan")},
               {"trim": 0.0}, {"trim": 1.5}, {"subdivide": 0}, {"subdivide": 17}, {"start_iterations": -1}):
        with pytest.raises(ValueError, match="align_mesh"):
            MA.align_mesh(v, f, v, f, device="cpu", **kw)
    for bad in ((v[:0], f, v, f), (v, f[:0], v, f), (v, f, v[:0], f), (v, f, v, f[:0])):               # empty on either side, before any launch
        with pytest.raises(ValueError, match="align_mesh"):
            MA.align_mesh(*bad, device="cpu")
        with pytest.raises(ValueError, match="score_meshes"):
            MA.score_meshes(*bad, device="cpu")
    for kw in ({"thresholds": (0.01, 0.0)}, {"thresholds": (float("inf"),)}, {"iou_resolution": -1}, {"iou_resolution": 2.5}, {"subdivide": 0}):
        with pytest.raises(ValueError, match="score_meshes"):
            MA.score_meshes(v, f, v, f, device="cpu", **kw)
    with pytest.raises(ValueError, match="solve_similarity"):
        MA.solve_similarity(np.zeros(20), "none")
    with pytest.raises(ValueError, match="solve_similarity"):
        MA.solve_similarity(np.zeros(19), "rigid")
    with pytest.raises(ValueError, match="transform_vertices"):
        MA.transform_vertices(v[:, :2], np.eye(4))
    with pytest.raises(ValueError, match="transform"):
        MA.transform_vertices(v, np.eye(3))


# ---- the solve ------------------------------------------------------------------------------------------------------------------------------
def _moments(p, q, w):
    """the 20 sums of pairs (p, q) with weights w, by the restatement's terms"""
    return A.pair_terms(p, q, (p - q).norm(dim=1), torch.zeros(p.shape[0], dtype=torch.long), w).sum(0)


def test_solve_similarity_against_the_restatement_and_the_truth():
    g = torch.Generator().manual_seed(3)
    for trial in range(20):
        p = torch.randn(50, 3, generator=g, dtype=F64) * torch.tensor([1.0, 0.6, 0.3], dtype=F64) + torch.randn(3, generator=g, dtype=F64)
        w = torch.rand(50, generator=g, dtype=F64)
        T = A.similarity(float(torch.rand(1, generator=g)) * 179.0, torch.randn(3, generator=g).tolist(), 0.5 + float(torch.rand(1, generator=g)),
                         torch.randn(3, generator=g).tolist())
        q = p @ torch.as_tensor(T[:3, :3]).T + torch.as_tensor(T[:3, 3])
        s = _moments(p, q, w)
        got = MA.solve_similarity(s, "similarity")
        assert np.abs(got - A.umeyama(s, "similarity")).max() < 1e-10
        assert np.abs(got - T).max() < 1e-9                                      # exact pairs: the motion itself
        noisy = _moments(p, q + 0.05 * torch.randn(50, 3, generator=g, dtype=F64), w)
        for mode in ("rigid", "similarity"):
            got, ref = MA.solve_similarity(noisy, mode), A.umeyama(noisy, mode)
            assert np.abs(got - ref).max() < 1e-10
            scale, R, _ = A.decompose(got)
            assert np.abs(R @ R.T - np.eye(3)).max() < 1e-12 and np.linalg.det(R) > 0
            assert mode == "similarity" or abs(scale - 1.0) < 1e-12
        assert MA.solve_similarity(torch.as_tensor(noisy), "rigid").dtype == np.float64            # a tensor is taken too


def test_solve_similarity_never_returns_a_reflection_and_keeps_still_without_spread():
    g = torch.Generator().manual_seed(4)
    p = torch.randn(40, 3, generator=g, dtype=F64)
    w = torch.ones(40, dtype=F64)
    mirror = torch.tensor([1.0, 1.0, -1.0], dtype=F64)
    for mode in ("rigid", "similarity"):
        got = MA.solve_similarity(_moments(p, p * mirror, w), mode)                # a pure reflection: the determinant guard
        assert np.linalg.det(got[:3, :3]) > 0
        assert np.abs(got - A.umeyama(_moments(p, p * mirror, w), mode)).max() < 1e-10
        one = MA.solve_similarity(_moments(p[:1], p[:1] + 1.0, w[:1]), mode)       # one point: no variance
        assert np.array_equal(one, np.eye(4)) and np.array_equal(A.umeyama(_moments(p[:1], p[:1] + 1.0, w[:1]), mode), np.eye(4))
        zero = MA.solve_similarity(_moments(p, p + 1.0, 0.0 * w), mode)            # no weight
        assert np.array_equal(zero, np.eye(4))
        assert np.array_equal(MA.solve_similarity(np.zeros(20), mode), np.eye(4))


def test_the_24_starts_are_the_proper_rotations_of_the_cube():
    R = MA.cube_rotations()
    assert R.shape == (24, 3, 3) and np.array_equal(R[0], np.eye(3))
    assert all(np.array_equal(a, b) for a, b in zip(R, A.cube_rotations()))
    for k in range(24):
        assert np.array_equal(R[k] @ R[k].T, np.eye(3)) and np.linalg.det(R[k]) == pytest.approx(1.0)
        assert set(np.unique(R[k])) <= {-1.0, 0.0, 1.0}
    assert len({R[k].tobytes() for k in range(24)}) == 24
    v, _ = A.coarse()
    rv, _ = A.target()
    for mode in ("rigid", "similarity"):
        for k in (0, 6, 23):
            T = MA.start_transform(k, v.double().numpy(), rv.double().numpy(), mode)
            assert np.abs(T - A.start_transform(k, v, rv, mode)).max() < 1e-14
            moved = MA.transform_vertices(v.double(), T).numpy()
            assert np.abs(0.5 * (moved.min(0) + moved.max(0)) - 0.5 * (rv.double().numpy().min(0) + rv.double().numpy().max(0))).max() < 1e-12
            ratio = np.linalg.norm(moved.max(0) - moved.min(0)) / np.linalg.norm(rv.double().numpy().max(0) - rv.double().numpy().min(0))
            assert mode == "rigid" or abs(ratio - 1.0) < 1e-12


def test_trim_distance_decompose_and_transform_vertices():
    d = torch.tensor([0.4, 0.1, float("inf"), 0.3, 0.2, 0.25])
    w = torch.tensor([1.0, 1.0, 1.0, 1.0, 1.0, float("nan")])
    up = lambda x: float(np.nextafter(np.float32(x), np.float32(np.inf)))  # noqa: E731
    assert MA.trim_distance(d, w, 5.0, 0.4) == up(0.2) == A.trim_distance(d, w, 5.0, 0.4)             # 2 of 5 within 0.2
    assert MA.trim_distance(d, w, 5.0, 0.41) == up(0.3)
    assert MA.trim_distance(d, w, 5.0, 0.8) == up(0.4)
    assert MA.trim_distance(d, w, 5.0, 0.81) == math.inf == A.trim_distance(d, w, 5.0, 0.81)          # the miss never comes within reach
    assert MA.trim_distance(d[:0], w[:0], 0.0, 0.5) == math.inf
    from v3d_amd.recon.mesh_solid import voxel_centres
    whole = voxel_centres(7, 0.9, "cpu")                                         # the slabs of volume_iou are pieces of the whole, bit for bit
    assert torch.equal(torch.cat([voxel_centres(7, 0.9, "cpu", layers=(z, min(z + 3, 7))) for z in range(0, 7, 3)]), whole)
    dec = MA.decompose(A.KNOWN)
    assert dec["scale"] == pytest.approx(1.08, abs=1e-12) and dec["rotation_angle"] == pytest.approx(12.0, abs=1e-9)
    assert np.allclose(dec["translation"], [0.05, -0.03, 0.04])
    v, _ = A.coarse()
    assert torch.equal(MA.transform_vertices(v, A.KNOWN), A.move(v, A.KNOWN)) and MA.transform_vertices(v.numpy(), A.KNOWN[:3]).dtype == F32


# ---- the script -----------------------------------------------------------------------------------------------------------------------------
def _entry(name):
    spec = importlib.util.spec_from_file_location("v3d_entry_" + name, os.path.join(ROOT, "scripts", "pub", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_score_mesh_options_parse_and_are_checked_before_the_library_is_imported(monkeypatch):
    mod = _entry("score_mesh")
    ap = mod.build_parser()
    a = vars(ap.parse_args(["--mesh", "m.ply", "--reference", "gt.ply"]))
    assert a == {"mesh": "m.ply", "reference": "gt.ply", "align": "similarity", "starts": 1, "iterations": 200, "trim": 1.0,
                 "threshold": [0.01, 0.02, 0.05], "iou_resolution": 128, "subdivide": 2, "json": None, "out": None}
    b = vars(ap.parse_args(["--mesh", "m.obj", "--reference", "gt.ply", "--align", "rigid", "--starts", "24", "--iterations", "50", "--trim", "0.9",
                            "--threshold", "0.1", "0.2", "--iou_resolution", "0", "--subdivide", "3", "--json", "s.json", "-o", "moved.ply"]))
    assert (b["align"], b["starts"], b["iterations"], b["trim"], b["threshold"], b["iou_resolution"], b["subdivide"], b["json"], b["out"]) == \
        ("rigid", 24, 50, 0.9, [0.1, 0.2], 0, 3, "s.json", "moved.ply")
    for missing in ([], ["--mesh", "m.ply"], ["--reference", "gt.ply"], ["--mesh", "m.ply", "--reference", "gt.ply", "--align", "affine"]):
        with pytest.raises(SystemExit):
            ap.parse_args(missing)
    monkeypatch.setitem(sys.modules, "render_mesh", None)
    base = ["--mesh", "does/not/exist.ply", "--reference", "does/not/gt.ply"]
    for bad in (["--starts", "2"], ["--iterations", "-1"], ["--trim", "0"], ["--trim", "1.1"], ["--threshold", "0"], ["--threshold", "0.1", "inf"],
                ["--iou_resolution", "-1"], ["--iou_resolution", "1025"], ["--subdivide", "0"], ["--subdivide", "17"], ["--json", "out.txt"],
                ["-o", "out.obj"], ["-o", "does/not/exist.ply"], ["-o", "does/not/../not/gt.ply"], ["--mesh", "does/not/exist.glb"],
                ["--reference", "does/not/gt.obj"]):
        with pytest.raises(SystemExit):
            mod.main(base + bad)
    with pytest.raises(ImportError):                       # good arguments do reach the import
        mod.main(base)
    st = {"mode": "similarity", "start": 6, "iterations_run": 40, "scale": 0.77, "rotation_angle": 170.0, "rms": 1.25e-3, "seconds": 0.25}
    sc = {"relative": {"chamfer": 0.001}, "chamfer": 1.5e-3, "diagonal": 1.5, "normal_consistency": {"mean": 0.98}, "volume_iou": None,
          "fscore": [{"threshold": 0.01, "fscore": 0.9}], "seconds": 0.5}
    assert mod.line("m.ply", "gt.ply", st, sc) == ("[score] m.ply -> gt.ply: align similarity (start 6, 40 iterations, scale 0.77000, rotation 170.000 deg, "
                                                   "rms 1.250e-03); chamfer 1.500e-03 (0.1000 % of the diagonal 1.5000); F@1% 0.9000; normal consistency "
                                                   "0.9800; IoU skipped; 0.750 s")


# ---- the premises of the GPU cases, on the fp64 restatement ---------------------------------------------------------------------------------
def test_the_scenes_are_what_the_issue_says():
    rv, rf = A.target()
    cv, cf = A.coarse()
    fv, ff = A.coarse_with_floater()
    assert rf.shape[0] == 1280 and cf.shape[0] == 320 and ff.shape[0] == 400
    assert float((rv.max(0).values - rv.min(0).values).double().norm()) == pytest.approx(A.TARGET_DIAGONAL, abs=5e-4)
    _, w, _ = Q.face_samples(fv, ff, 1)
    assert float(w[320:].sum() / w.sum()) == pytest.approx(0.077, abs=1e-3)        # the floater's share of the area
    for T, angle, scale in ((A.KNOWN, 12.0, 1.08), (A.FAR, 170.0, 1.3)):
        s, R, a = A.decompose(T)
        axis = np.array([R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]])
        assert s == pytest.approx(scale) and a == pytest.approx(angle) and np.allclose(axis / np.linalg.norm(axis), np.array([1, 2, 3]) / math.sqrt(14))


def _golden():
    return json.load(open(os.path.join(ROOT, "tests", "golden", "mesh_align_cases.json")))


def _same_as_recorded(name, dtype, st, T):
    """tests/golden/mesh_align_cases.json is what tests/test_mesh_align_gpu.py reads in the restatement's place: it must be this very run"""
    rec = _golden()[name]["float64" if dtype == F64 else "float32"]
    assert rec["start"] == st["start"] and len(rec["rms_history"]) == len(st["rms_history"])
    assert np.allclose(rec["rms_history"], st["rms_history"], rtol=1e-6, atol=1e-9) and np.allclose(rec["matrix"], T, rtol=0, atol=1e-7)


def test_premise_1_recovery():
    T, st = A.align_case("recovery")
    h = st["rms_history"]
    angle, ss0 = A.residual(T, A.KNOWN)
    print(f"recovery: rms {h[0] / A.TARGET_DIAGONAL:.3e} -> {h[-1] / A.TARGET_DIAGONAL:.3e} of the diagonal ({h[0] / h[-1]:.0f} x), {angle:.3f} deg, "
          f"|s s0 - 1| {abs(ss0 - 1):.1e}")
    assert len(h) == 61 and h[0] / h[-1] >= 50 and angle <= 1.0 and abs(ss0 - 1) <= 1e-3
    _same_as_recorded("recovery", F64, st, T)


def test_premise_2_far_start():
    v, f, rv, rf, T0, kw = A.align_inputs("far")
    T, st = A.align_case("far")
    alone_T, alone = A.align(v, f, rv, rf, only_start=0, **{k: x for k, x in kw.items() if k != "starts"})
    angle, _ = A.residual(T, T0)
    print(f"far start: start {st['start']} chosen, final rms {st['rms_history'][-1] / A.TARGET_DIAGONAL:.3e} of the diagonal, {angle:.3f} deg;  start 0 alone "
          f"{alone['rms_history'][-1] / A.TARGET_DIAGONAL:.3e}, {A.residual(alone_T, T0)[0]:.1f} deg")
    assert alone["rms_history"][-1] > 10 * st["rms_history"][-1]
    assert angle <= 1.0 and st["start"] != 0
    order = sorted(st["start_rms"])
    assert order[1] > 1.1 * order[0]                   # the choice of the start is no close call: a float32 run cannot choose another
    _same_as_recorded("far", F64, st, T)


def test_premise_3_floater():
    T1, st1 = A.align_case("floater")
    T9, st9 = A.align_case("floater_trim")
    a1, s1 = A.residual(T1, A.KNOWN)
    a9, s9 = A.residual(T9, A.KNOWN)
    print(f"floater: trim 1.0 {a1:.2f} deg, scale {s1:.4f};  trim 0.9 {a9:.2f} deg, scale {s9:.4f}")
    assert a1 > 5.0
    assert a9 <= 1.5 and abs(s9 - 1.0) <= 0.02
    _same_as_recorded("floater", F64, st1, T1)
    _same_as_recorded("floater_trim", F64, st9, T9)


def test_the_early_stop_fires_where_the_history_says():
    T, st = A.align_case("early")
    full = A.recorded_case("recovery")[1]["rms_history"]
    h = st["rms_history"]
    change = [abs(full[i - 1] - full[i]) / full[i - 1] for i in range(1, len(full))]
    first = next(i for i, c in enumerate(change, 1) if i > 0 and c < A.EARLY_TOL)
    assert first == A.EARLY_ITERATIONS == st["iterations_run"] == len(h) - 1
    assert min(abs(c - A.EARLY_TOL) for c in change[:first]) > 1e-3              # the stop is no close call
    assert np.allclose(h, full[:len(h)], rtol=1e-9)                              # the same run up to there; the matrix is the one measured last
    assert abs(A.rms_of(A.correspond(*A.target(), *[x.float() for x in Q.face_samples(*A.align_inputs("early")[:2], 1)[:2]], T)["sums"]) - h[-1]) < 1e-12
    _same_as_recorded("early", F64, st, T)


@pytest.mark.parametrize("name,dtype", [("rigid", F64)] + [(n, F32) for n in A.ALIGN_CASES])
def test_every_other_record_is_this_restatement(name, dtype):
    """the fp64 records of the premises are held above; here the rest, so that both sides of every history bar of the GPU test are held"""
    T, st = A.align_case(name, dtype)
    _same_as_recorded(name, dtype, st, T)


@pytest.mark.parametrize("pair", A.SCORE_PAIRS)
@pytest.mark.parametrize("N", A.IOU_RESOLUTIONS)
def test_premise_4_iou_grids_keep_clear_of_one_half(pair, N):
    wa, wb, _ = A.iou_case(pair, N)
    left_out = 1.0 - float(A.iou_sure(wa, wb).double().mean())
    print(f"IoU {pair} N {N}: {left_out:.4f} of the cells within {A.IOU_MARGIN} of 0.5;  counts {A.iou_counts(wa, wb)}")
    assert left_out <= A.EXCLUDE_MAX
    ia, ib, both, union = A.iou_counts(wa, wb)
    assert 0 < both <= min(ia, ib) and union == ia + ib - both
