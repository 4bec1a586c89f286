"""The gfx950 silhouette fit (csrc_recon/meshdeform.hip, v3d_amd/recon/mesh_deform.py, scripts/pub/fit_mesh.py) against the torch restatement
(tests/mesh_deform_ref.py): the antialiased alpha, the receivers and chosen edges pair for pair, the gradient to pix_f and to the vertices,
the reduce on synthetic lists, guard sentinels around every output, the smoothness gradient, one step of the fit, the fit end to end and the
entry point.  The restatement is fed the KERNEL'S OWN pix_f, pix_q and face_id, as tests/test_mesh_refine_gpu.py does: coverage decisions
are shared and only the new arithmetic is compared.

The bar everywhere is that file's: the kernel may be off from the fp64 restatement by 4x what the restatement's own float32 run is off.
For the gradients "off" is measured two ways (mesh_refine_ref.row_errors): relative L2 over all rows, and the largest relative L2 of a
single row among the rows whose norm is above 1e-3 of the largest row's."""
import ctypes as C
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import gs_dense_ref as D
import mesh_deform_ref as DF
import mesh_refine_ref as RF
import mesh_render_ref as M
from conftest import record_parity
from v3d_amd.recon import geometry as G
from v3d_amd.recon import mesh_deform as MD
from v3d_amd.recon import mesh_render as MR
from v3d_amd.recon.rasterize import gs_camera

pytestmark = pytest.mark.gpu
DEV = "cuda"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BG = [0.0, 0.0, 0.0]
F64, F32 = torch.float64, torch.float32


def dev_i32(t):
    return t.to(DEV, torch.int32).contiguous()


@functools.lru_cache(maxsize=None)
def frozen(case):
    """The kernel's forward of a scene of DEFORM_CASES and both restatements of it on the kernel's own decisions, computed once and shared
    (nothing below writes into them)"""
    kind, seed, W, H, _, _ = case
    cam = M.case_camera(case)
    v, f, _ = M.mesh_scene(kind, seed)
    gc = gs_camera(cam, BG)
    vd, fd = v.to(DEV), dev_i32(f)
    fwd = MD.alpha_forward(gc, vd, fd)
    host = {k: fwd[k].cpu() for k in ("alpha_aa", "alpha_raw", "face_id", "pix_f", "pix_q", "zv")}
    ref = {dt: DF.view_forward(v, f, cam, dt, given=(host["pix_f"], host["pix_q"], host["face_id"])) for dt in (F64, F32)}
    return cam, gc, v, f, vd, fd, fwd, host, ref


@functools.lru_cache(maxsize=None)
def hand(name):
    pix_f, q, faces, fid = DF.HAND_SCENES[name]()
    dv = (dev_i32(fid), dev_i32(faces), pix_f.to(DEV).contiguous(), dev_i32(q))
    alpha, raw = MD.aa_forward(*dv)
    ref = {}
    for dt in (F64, F32):
        pr = DF.pairs(pix_f, q, faces, fid, dt)
        ref[dt] = (pr,) + DF.alpha_aa(pr, dt)
    return pix_f, q, faces, fid, dv, alpha, raw, ref


# ---- 1. the antialiased alpha -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", DF.DEFORM_CASES, ids=M.case_id)
def test_alpha_matches_the_restatement(case):
    cam, gc, v, f, vd, fd, fwd, host, ref = frozen(case)
    a64, a32 = ref[F64]["alpha_aa"], ref[F32]["alpha_aa"]
    err, err32 = float((host["alpha_aa"].double() - a64).abs().max()), float((a32.double() - a64).abs().max())
    rerr = float((host["alpha_raw"].double() - ref[F64]["alpha_raw"]).abs().max())
    rerr32 = float((ref[F32]["alpha_raw"].double() - ref[F64]["alpha_raw"]).abs().max())
    cov = host["face_id"] >= 0
    touched = int(((host["alpha_aa"] > 0) & (host["alpha_aa"] < 1)).sum())
    print(f"alpha_aa {err:.3e} (float32 restatement {err32:.3e})  alpha_raw {rerr:.3e} ({rerr32:.3e})  {touched} antialiased pixels")
    record_parity(f"mesh_deform_alpha[{M.case_id(case)}]", {"alpha_max_abs": err, "alpha_float32_restatement": err32, "raw_max_abs": rerr,
                                                            "raw_float32_restatement": rerr32, "antialiased_pixels": touched,
                                                            "pairs": int(ref[F64]["pairs"]["pair"].sum())})
    assert torch.equal(MR.render_mesh(cam, v, f, torch.zeros_like(v), BG)["face_id"].cpu(), host["face_id"])          # the same forward
    assert 0.05 < float(cov.double().mean()) < 0.6 and touched > 5
    assert torch.equal(host["alpha_aa"], host["alpha_raw"].clamp(0, 1))
    assert err <= 4 * err32 and rerr <= 4 * rerr32


@pytest.mark.parametrize("name", sorted(DF.HAND_SCENES))
def test_alpha_on_hand_placed_scenes(name):
    pix_f, q, faces, fid, dv, alpha, raw, ref = hand(name)
    r64, r32 = ref[F64][2], ref[F32][2]
    err, err32 = float((raw.cpu().double() - r64).abs().max()), float((r32.double() - r64).abs().max())
    print(f"{name}: alpha_raw {err:.3e} (float32 restatement {err32:.3e})")
    record_parity(f"mesh_deform_alpha[{name}]", {"raw_max_abs": err, "raw_float32_restatement": err32})
    assert torch.equal(alpha.cpu(), raw.cpu().clamp(0, 1))
    assert err <= 4 * err32
    if name == "needle":
        assert float(raw[9, 5]) < -0.1 and float(alpha[9, 5]) == 0.0
    if name == "no_candidate":
        assert float(raw[2, 2]) == 1.0 and float(raw[2, 3]) == 0.0
    if name == "negative_ep":
        assert float(raw[2, 3]) == 0.5
    if name == "exact_half":
        assert float(raw[2, 3]) == 1.0 and float(raw[2, 4]) == 0.0                 # t = 0.5 exactly: the neighbour receives 0
    if name == "on_edge":
        assert float(raw[2, 3]) == 1.0 and float(raw[2, 4]) == 0.0                 # E_k(q) = 0 exactly: no candidate, nothing added
    if name in ("exact_half", "edge_tie", "on_edge"):
        assert torch.equal(raw.cpu(), r32)                                         # dyadic: every step is exact


# ---- 2. receivers and chosen edges, pair for pair -------------------------------------------------------------------------------------------
def test_receivers_and_edges_are_the_restatements_pair_for_pair():
    to_p = to_q = 0
    for case in DF.DEFORM_CASES:
        cam, gc, v, f, vd, fd, fwd, host, ref = frozen(case)
        counts, info = MD.aa_pairs(fwd["face_id"], fd, fwd["pix_f"], fwd["pix_q"], debug=True)
        pr = ref[F64]["pairs"]
        assert torch.equal(info.cpu().long(), pr["info"]), M.case_id(case)
        assert torch.equal(counts.cpu().long().reshape(pr["k"].shape[:2]), 2 * (pr["k"] >= 0).sum(-1))
        to_q, to_p = to_q + int((info >= 4).sum()), to_p + int(((info >= 0) & (info < 4)).sum())
    assert to_p > 100 and to_q > 50                                            # both kinds of receiver (538 and 116 on the restatement)
    for name in sorted(DF.HAND_SCENES):
        pix_f, q, faces, fid, dv, alpha, raw, ref = hand(name)
        counts, info = MD.aa_pairs(*dv, debug=True)
        assert torch.equal(info.cpu().long(), ref[F64][0]["info"]), name
        assert torch.equal(counts.cpu().long().reshape(fid.shape), 2 * (ref[F64][0]["k"] >= 0).sum(-1)), name
    assert hand("edge_tie")[7][F64][0]["info"][2, 3, 0] == 1 and hand("exact_half")[7][F64][0]["info"][2, 3, 0] == 6
    assert hand("no_candidate")[7][F64][0]["info"][2, 2].tolist() == [-2, 4, -2, -2]


# ---- 3. the gradient ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", DF.DEFORM_CASES, ids=M.case_id)
def test_gradient_matches_the_restatement(case):
    cam, gc, v, f, vd, fd, fwd, host, ref = frozen(case)
    _, _, W, H, _, _ = case
    V = v.shape[0]
    dL = torch.randn(H, W, generator=torch.Generator().manual_seed(7))
    assert bool((dL[host["face_id"] < 0] != 0).all())                          # gradients on background pixels too
    out = MD.alpha_backward(gc, vd, fd, fwd, dL.to(DEV), debug=True)
    again = MD.alpha_backward(gc, vd, fd, fwd, dL.to(DEV))
    assert torch.equal(out["dL_dpix"], again["dL_dpix"]) and torch.equal(out["dL_dverts"], again["dL_dverts"]), "two runs differ"
    res = {}
    for dt in (F64, F32):
        g_verts, g_pix, length = DF.view_backward(v, cam, ref[dt], dL, dt)
        res[dt] = (g_pix, g_verts, length)
    length = res[F64][2]
    # the records: vertex and order as the restatement lists them
    keys, _ = DF.records(ref[F64]["pairs"], host["pix_f"], ref[F64]["alpha_raw"], dL)
    assert out["records"] == keys.numel() == 2 * int((ref[F64]["pairs"]["k"] >= 0).sum())
    assert torch.equal(out["keys"].cpu(), keys)
    r = out["ranges"].cpu().long()
    assert torch.equal(r[:, 1] - r[:, 0], length) and bool((r[length == 0] == 0).all())
    gp, gv = out["dL_dpix"].cpu(), out["dL_dverts"].cpu()
    (rel, row), (rel32, row32) = RF.row_errors(gp, res[F64][0]), RF.row_errors(res[F32][0], res[F64][0])
    (vrel, vrow), (vrel32, vrow32) = RF.row_errors(gv, res[F64][1]), RF.row_errors(res[F32][1], res[F64][1])
    print(f"dL_dpix rel L2 {rel:.3e} (float32 restatement {rel32:.3e}) worst row {row:.3e} ({row32:.3e});  dL_dverts {vrel:.3e} ({vrel32:.3e}) "
          f"worst row {vrow:.3e} ({vrow32:.3e});  {int((length == 0).sum())} of {V} rows empty, longest list {int(length.max())}")
    record_parity(f"mesh_deform_gradient[{M.case_id(case)}]", {"pix_rel_l2": rel, "pix_rel_l2_float32_restatement": rel32, "pix_worst_row": row,
                                                               "pix_worst_row_float32_restatement": row32, "verts_rel_l2": vrel,
                                                               "verts_rel_l2_float32_restatement": vrel32, "verts_worst_row": vrow,
                                                               "verts_worst_row_float32_restatement": vrow32, "records": out["records"]})
    assert 0 < int((length == 0).sum()) < V and not gp[length == 0].any() and not gv[length == 0].any()          # exact zeros without records
    assert rel <= 4 * rel32 and row <= 4 * row32 and vrel <= 4 * vrel32 and vrow <= 4 * vrow32
    # through autograd, the public way
    x = vd.clone().requires_grad_(True)
    keep = MD.AlphaView()
    with torch.enable_grad():                              # (a module of the suite may have switched autograd off for the process)
        a = MD.antialiased_alpha(cam, x, f, keep=keep)
        (a * dL.to(DEV)).sum().backward()
    assert torch.equal(a.detach(), fwd["alpha_aa"]) and torch.equal(x.grad, out["dL_dverts"]) and keep.pairs == out["records"] // 2
    assert torch.equal(keep.face_id, fwd["face_id"])


def test_gradient_on_hand_placed_scenes_and_marked_vertices():
    for name in sorted(DF.HAND_SCENES):
        pix_f, q, faces, fid, dv, alpha, raw, ref = hand(name)
        V = pix_f.shape[0]
        dL = torch.randn(fid.shape, generator=torch.Generator().manual_seed(11))
        out = MD.aa_backward(*dv, raw, dL.to(DEV), debug=True)
        g = {dt: DF.alpha_backward(ref[dt][0], pix_f, ref[dt][2], dL, V, dt)[0] for dt in (F64, F32)}
        (rel, row), (rel32, row32) = RF.row_errors(out["dL_dpix"].cpu(), g[F64]), RF.row_errors(g[F32], g[F64])
        print(f"{name}: dL_dpix rel L2 {rel:.3e} (float32 restatement {rel32:.3e}) worst row {row:.3e} ({row32:.3e})")
        record_parity(f"mesh_deform_gradient[{name}]", {"pix_rel_l2": rel, "pix_rel_l2_float32_restatement": rel32})
        assert rel <= 4 * rel32 + 1e-12 and row <= 4 * row32 + 1e-12, name
        if name == "negative_ep":
            assert out["records"] == 10 and not out["payload"].any() and not out["dL_dpix"].any()          # every Ep is clamped: zeros, emitted
        if name == "needle":
            pay = out["payload"].cpu()
            idx = torch.nonzero(ref[F64][0]["k"] >= 0)
            tip = (idx[:, 0] == 9).repeat_interleave(2)
            assert int(tip.sum()) == 6 and not pay[tip].any() and bool(pay[~tip].any(1).all())             # the clamped pixel: exactly 0
    # marked vertices get exact zeros from the projection's backward
    cam, gc, v, f, vd, fd, fwd, host, ref = frozen(DF.DEFORM_CASES[0])
    V = v.shape[0]
    g_pix = torch.randn(V, 2, generator=torch.Generator().manual_seed(2))
    pix_q = host["pix_q"].clone()
    marked = torch.zeros(V, dtype=torch.bool)
    marked[::5] = True
    pix_q[marked] = M.MARK
    out = MD.project_backward(gc, vd, dev_i32(pix_q), g_pix.to(DEV)).cpu()
    r64, r32 = DF.project_bwd(v, cam, marked, g_pix), DF.project_bwd(v, cam, marked, g_pix, F32)
    (rel, row), (rel32, row32) = RF.row_errors(out, r64), RF.row_errors(r32, r64)
    print(f"project_bwd rel L2 {rel:.3e} (float32 restatement {rel32:.3e}) worst row {row:.3e} ({row32:.3e})")
    record_parity("mesh_deform_project_bwd", {"rel_l2": rel, "rel_l2_float32_restatement": rel32, "worst_row": row, "worst_row_float32_restatement": row32})
    assert not out[marked].any() and bool(out[~marked].any(1).all())
    assert rel <= 4 * rel32 and row <= 4 * row32


# ---- 4. the reduce on synthetic lists ---------------------------------------------------------------------------------------------------------
def test_reduce_on_synthetic_lists_of_every_length():
    g = torch.Generator().manual_seed(0)
    lens = list(RF.LIST_LENGTHS) + [0]
    assert lens == [0, 1, 63, 64, 65, 128, 700, 0]
    n, V = sum(lens), len(lens)
    ranges, o = [], 0
    for m in lens:
        ranges.append((o, o + m) if m else (0, 0))
        o += m
    ranges = torch.tensor(ranges, dtype=torch.int32)
    vals = torch.randperm(n, generator=g).to(torch.int32)
    payload = (torch.randn(n, 2, generator=g) * torch.pow(10.0, 3 * (2 * torch.rand(n, 2, generator=g) - 1))).float()
    out = torch.full((V, 2), float("nan"), device=DEV)          # every row is written: nothing of this survives
    lib = G.load_library()
    dvals, dpay, drng = vals.to(DEV), payload.to(DEV), ranges.to(DEV)
    assert lib.v3d_recon_mesh_aa_reduce(drng.data_ptr(), dvals.data_ptr(), dpay.data_ptr(), n, V, out.data_ptr(), None) == 0
    torch.cuda.synchronize()
    out = out.cpu()
    assert torch.equal(out, MD.aa_reduce(drng, dvals, dpay, V).cpu())
    table = torch.full((V, max(lens)), -1, dtype=torch.long)
    for v in range(V):
        table[v, :lens[v]] = vals[int(ranges[v, 0]):int(ranges[v, 1])].long()
    ref, ref32 = (RF.list_sum(table, torch.ones(n, dtype=dt), payload.to(dt), dt) for dt in (F64, F32))
    assert bool(torch.isfinite(out).all()) and not out[0].any() and not out[-1].any()
    assert torch.equal(out[1], payload[vals[0].long()])                        # one entry: itself
    per = lambda x: ((x.double() - ref).norm(dim=1) / ref.norm(dim=1).clamp_min(1e-300))[1:-1]  # noqa: E731
    (rel, row), (rel32, row32) = RF.row_errors(out, ref), RF.row_errors(ref32, ref)
    print(f"rows {per(out).tolist()}\nfloat32 restatement {per(ref32).tolist()}\nrel L2 {rel:.3e} ({rel32:.3e})")
    record_parity("mesh_deform_reduce_synthetic", {"rel_l2": rel, "rel_l2_float32_restatement": rel32, "rows_rel": per(out).tolist(),
                                                   "rows_rel_float32_restatement": per(ref32).tolist()})
    assert rel <= 4 * rel32 and float(per(out).max()) <= 4 * float(per(ref32).max())
    # no record at all: zeros, with null lists
    z = torch.full((V, 2), float("nan"), device=DEV)
    zr = torch.zeros(V, 2, dtype=torch.int32, device=DEV)
    assert lib.v3d_recon_mesh_aa_reduce(zr.data_ptr(), None, None, 0, V, z.data_ptr(), None) == 0
    assert not z.cpu().any()


# ---- 5. guard sentinels ---------------------------------------------------------------------------------------------------------------------
GUARD = 64


def guarded(n, dtype, fill):
    buf = torch.full((n + 2 * GUARD,), fill, dtype=dtype, device=DEV)
    return buf, buf[GUARD:GUARD + n]


def intact(buf, n, fill):
    edge = torch.cat([buf[:GUARD], buf[GUARD + n:]]).cpu()
    return bool(torch.isnan(edge).all()) if isinstance(fill, float) else bool((edge == fill).all())


@pytest.mark.parametrize("case", DF.DEFORM_CASES[6:], ids=M.case_id)
def test_no_entry_writes_outside_its_outputs(case):
    cam, gc, v, f, vd, fd, fwd, host, ref = frozen(case)
    _, _, W, H, _, _ = case
    V, F, HW = v.shape[0], f.shape[0], W * H
    lib, nan, tag = G.load_library(), float("nan"), -7777
    fid, pf, pq = fwd["face_id"], fwd["pix_f"], fwd["pix_q"]
    view = (fid.data_ptr(), fd.data_ptr(), F, pf.data_ptr(), pq.data_ptr(), V, W, H)
    ab, a = guarded(HW, F32, nan)
    rb, r = guarded(HW, F32, nan)
    assert lib.v3d_recon_mesh_aa_alpha(*view, a.data_ptr(), r.data_ptr(), None) == 0
    cb, c = guarded(HW, torch.int32, tag)
    ib, i = guarded(4 * HW, torch.int32, tag)
    assert lib.v3d_recon_mesh_aa_count(*view, c.data_ptr(), i.data_ptr(), None) == 0
    torch.cuda.synchronize()
    assert intact(ab, HW, nan) and intact(rb, HW, nan) and intact(cb, HW, tag) and intact(ib, 4 * HW, tag)
    assert torch.equal(a.reshape(H, W), fwd["alpha_aa"]) and torch.equal(r.reshape(H, W), fwd["alpha_raw"]) and bool(torch.isfinite(a).all())
    assert bool((c >= 0).all()) and bool((i >= -2).all())
    from v3d_amd.ops import get_ops
    off = get_ops().gs_scan(c.contiguous())
    n = int(off[-1])
    assert n > 0
    dL = torch.randn(H, W, generator=torch.Generator().manual_seed(3)).to(DEV)
    kb, k = guarded(n, torch.int64, tag)
    vb, vals = guarded(n, torch.int32, tag)
    pb, pay = guarded(2 * n, F32, nan)
    assert lib.v3d_recon_mesh_aa_emit(*view, r.data_ptr(), dL.data_ptr(), off.data_ptr(), n, k.data_ptr(), vals.data_ptr(), pay.data_ptr(), None) == 0
    torch.cuda.synchronize()
    assert intact(kb, n, tag) and intact(vb, n, tag) and intact(pb, 2 * n, nan)
    assert bool(((k >= 0) & (k < V)).all()) and torch.equal(vals.long(), torch.arange(n, device=DEV)) and bool(torch.isfinite(pay).all())
    out = MD.alpha_backward(gc, vd, fd, fwd, dL, debug=True)
    assert torch.equal(k, out["keys"]) and torch.equal(pay.reshape(n, 2), out["payload"])
    gb, g = guarded(2 * V, F32, nan)
    assert lib.v3d_recon_mesh_aa_reduce(out["ranges"].data_ptr(), out["vals_sorted"].data_ptr(), out["payload"].data_ptr(), n, V, g.data_ptr(), None) == 0
    db, d = guarded(3 * V, F32, nan)
    assert lib.v3d_recon_mesh_project_bwd(vd.data_ptr(), V, C.byref(gc), pq.data_ptr(), out["dL_dpix"].data_ptr(), d.data_ptr(), None) == 0
    ranges, corners = MD.corner_lists(fd, V)
    sb, s = guarded(3 * V, F32, nan)
    assert lib.v3d_recon_mesh_smooth_grad(vd.data_ptr(), V, fd.data_ptr(), F, ranges.data_ptr(), corners.data_ptr(), 0.5, s.data_ptr(), None) == 0
    torch.cuda.synchronize()
    assert intact(gb, 2 * V, nan) and intact(db, 3 * V, nan) and intact(sb, 3 * V, nan)
    assert torch.equal(g.reshape(V, 2), out["dL_dpix"]) and torch.equal(d.reshape(V, 3), out["dL_dverts"]) and bool(torch.isfinite(s).all())


# ---- 6. the smoothness gradient -------------------------------------------------------------------------------------------------------------
def test_smoothness_gradient_on_the_sphere_and_on_an_isolated_vertex():
    v, f, _ = M.mesh_scene("sphere", 1)
    v = torch.cat([v, torch.zeros(1, 3)])                                      # + an isolated vertex
    V = v.shape[0]
    d = (0.05 * torch.randn(V, 3, generator=torch.Generator().manual_seed(3))).float()
    fd = dev_i32(f)
    lists = MD.corner_lists(fd, V)
    x = d.to(DEV).requires_grad_(True)
    with torch.enable_grad():
        e = MD.smooth_energy(x, fd, lists)
        e.backward()
    e, g = e.detach(), x.grad.cpu()
    assert torch.equal(g, MD.smooth_gradient(d.to(DEV), fd, *lists).cpu())
    r64, r32 = DF.smooth_grad(d, f), DF.smooth_grad(d, f, F32)
    (rel, row), (rel32, row32) = RF.row_errors(g, r64), RF.row_errors(r32, r64)
    eerr = abs(float(e.detach()) - float(DF.smooth_energy(d.double(), f)))
    print(f"smooth_grad rel L2 {rel:.3e} (float32 restatement {rel32:.3e}) worst row {row:.3e} ({row32:.3e}); energy {float(e):.4e} off by {eerr:.1e}")
    record_parity("mesh_deform_smooth_grad", {"rel_l2": rel, "rel_l2_float32_restatement": rel32, "worst_row": row, "worst_row_float32_restatement": row32})
    assert not g[-1].any() and bool(g[:-1].any(1).all())
    assert rel <= 4 * rel32 and row <= 4 * row32 and eerr <= 1e-5 * float(e)


# ---- 7. one step, and the fit end to end ------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def e2e():
    v, f, full = DF.e2e_mesh()
    cams = DF.e2e_cameras()
    targets = torch.stack([MD.antialiased_alpha(cam, full.to(DEV), f).detach() for cam in cams])
    return v, f, cams, targets


def test_one_step_of_the_fit_is_the_restatements(e2e):
    v, f, cams, targets = e2e
    lr = DF.E2E["lr"]
    out, stats = MD.fit_vertices(v, f, cams, targets, iterations=1, lr=lr, seed=DF.E2E["seed_views"])
    j = RF.view_schedule(len(cams), 1, DF.E2E["seed_views"])[0]
    fwd = MD.alpha_forward(gs_camera(cams[j], BG), v.to(DEV), dev_i32(f))
    given = lambda it, jj, vv: (fwd["pix_f"].cpu(), fwd["pix_q"].cpu(), fwd["face_id"].cpu())  # noqa: E731
    r = {dt: DF.fit(v, f, cams, list(targets.cpu()), 1, lr, seed=DF.E2E["seed_views"], dtype=dt, given=given) for dt in (F64, F32)}
    err = float((out.cpu().double() - r[F64]["verts"]).abs().max())
    err32 = float((r[F32]["verts"].double() - r[F64]["verts"]).abs().max())
    direct = float((out.cpu() - r[F32]["verts"]).abs().max())
    moved = (out.cpu() != v).any(1)
    print(f"one step: vertices {err:.3e} from fp64 (float32 restatement {err32:.3e}; kernel against float32 restatement {direct:.3e}); "
          f"{int(moved.sum())} of {v.shape[0]} vertices moved; loss {stats['loss_first']:.6e} (restatement {r[F64]['loss_first']:.6e})")
    record_parity("mesh_deform_one_step", {"verts_max_abs": err, "verts_float32_restatement": err32, "against_float32_restatement": direct,
                                           "moved": int(moved.sum()), "loss_first": stats["loss_first"]})
    assert stats["opt_views"] == [0, 1, 2, 3] and stats["pairs"][j] > 40 and stats["vertices_moved"] >= int(moved.sum()) > 20
    assert abs(stats["loss_first"] - r[F64]["loss_first"]) <= 1e-5 * r[F64]["loss_first"]
    assert int((r[F64]["d"] != 0).any(1).sum()) <= stats["vertices_moved"]      # only vertices with records move on the first step
    assert 0.5 * lr < float((out.cpu() - v).abs().max()) <= 1.01 * lr           # Adam's first step: lr g / (|g| + eps)
    assert err <= 4 * err32


def test_fit_end_to_end(e2e):
    v, f, cams, targets = e2e
    kw = dict(iterations=DF.E2E["steps"], lr=DF.E2E["lr"], seed=DF.E2E["seed_views"])
    out, stats = MD.fit_vertices(v, f, cams, targets, **kw)
    again, _ = MD.fit_vertices(v, f, cams, targets, **kw)
    assert torch.equal(out, again), "two calls with the same arguments differ"
    before, after = len(cams) * stats["mse_before"], len(cams) * stats["mse_after"]          # summed over the views, as the restatement's figure
    want = DF.E2E_MSE_BEFORE - DF.E2E_MSE_AFTER
    print(f"alpha MSE summed over the views {before:.5f} -> {after:.5f} (fp64 restatement {DF.E2E_MSE_BEFORE} -> {DF.E2E_MSE_AFTER}); IoU "
          f"{stats['iou_before']:.4f} -> {stats['iou_after']:.4f}; largest offset {stats['max_offset']:.4f}; {stats['vertices_moved']} of {v.shape[0]} "
          f"vertices moved; pairs {stats['pairs']}; {stats['seconds']:.2f} s")
    record_parity("mesh_deform_e2e", {"mse_before": before, "mse_after": after, "restatement_mse_before": DF.E2E_MSE_BEFORE,
                                      "restatement_mse_after": DF.E2E_MSE_AFTER, "iou_before": stats["iou_before"], "iou_after": stats["iou_after"],
                                      "max_offset": stats["max_offset"], "vertices_moved": stats["vertices_moved"], "seconds": stats["seconds"]})
    assert abs(before - DF.E2E_MSE_BEFORE) <= 2e-3
    assert before - after >= 0.5 * want
    assert stats["iou_after"] > stats["iou_before"] and stats["loss_last"] < stats["loss_first"]
    assert 0.02 < stats["max_offset"] < 0.3 and stats["vertices_moved"] > v.shape[0] // 2 and all(p > 40 for p in stats["pairs"])


def test_fit_mesh_script_end_to_end(tmp_path):
    from v3d_amd.recon.gaussians import GaussianModel
    v, f, full = DF.e2e_mesh()
    c = M.position_colors(v)
    g = torch.Generator().manual_seed(4)
    p = torch.randn(6000, 3, generator=g)
    p = p / p.norm(dim=1, keepdim=True) * 0.5 * torch.rand(6000, 1, generator=g).pow(1.0 / 3.0) + torch.tensor(DF.E2E["centre"])       # the ball of the full sphere
    gm = GaussianModel(0)
    gm.set_params(p, torch.zeros(6000, 1, 3), torch.full((6000, 3), float(np.log(0.03))), torch.tensor([[1.0, 0.0, 0.0, 0.0]]).repeat(6000, 1),
                  torch.full((6000, 1), 3.0))
    ply, splats, video, out = str(tmp_path / "mesh.ply"), str(tmp_path / "point_cloud.ply"), str(tmp_path / "video.npy"), str(tmp_path / "fit.ply")
    G.save_mesh_ply(ply, v, f, c)
    gm.save_ply(splats)
    np.save(video, MR.render_mesh_orbit(full, f, M.position_colors(full), 4, 2.0, 0.0, 60.0, 48, True))
    r = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "pub", "fit_mesh.py"), "--mesh", ply, "--gaussians", splats, "-o", out, "-w",
                        "--views", "4", "--reso", "48", "--iters", "30", "--lr", "5e-3", "--video", video, "--render_orbit", "2"],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "silhouette IoU" in r.stdout and "PSNR mean over all frames" in r.stdout
    assert sorted(os.listdir(tmp_path)) == ["fit.json", "fit.ply", "fit_orbit", "mesh.ply", "point_cloud.ply", "video.npy"]
    assert sorted(os.listdir(tmp_path / "fit_orbit")) == ["000.png", "001.png", "orbit.npy"]
    stats = json.load(open(tmp_path / "fit.json"))
    assert {"mse_before", "mse_after", "iou_before", "iou_after", "loss_first", "loss_last", "seconds", "max_offset", "vertices_moved", "pairs",
            "psnr_before", "psnr_after", "opt_views", "iterations"} <= set(stats)
    assert stats["iou_after"] > stats["iou_before"] and stats["mse_after"] < stats["mse_before"] and stats["iterations"] == 30
    rv, rf, rc = G.read_mesh_ply(out)
    _, _, c0 = G.read_mesh_ply(ply)
    assert np.array_equal(rf, f.numpy()) and np.array_equal(rc, c0)            # topology and colours are carried over
    moved = (rv != v.numpy()).any(1)
    # (the smoothness term moves the neighbours of the vertices on the silhouette too)
    assert int(moved.sum()) >= stats["vertices_moved"] > 20 and float(np.abs(rv - v.numpy()).max()) <= stats["max_offset"] + 1e-6


# ---- 8. empty cases -------------------------------------------------------------------------------------------------------------------------
def test_a_mesh_with_nothing_drawn_comes_back_as_it_is():
    W, H = 56, 40
    cam = D.cams_for(W, H)[1]
    uv, uf, _, _ = M.undrawn_mesh(cam)                                         # V, F > 0 and nothing drawn
    x = uv.to(DEV).requires_grad_(True)
    keep = MD.AlphaView()
    with torch.enable_grad():
        a = MD.antialiased_alpha(cam, x, uf, keep=keep)
        (a * torch.randn(H, W, device=DEV)).sum().backward()
    assert not a.any() and not x.grad.any() and keep.pairs == 0 and bool((keep.face_id == -1).all())
    out, stats = MD.fit_vertices(uv, uf, [cam] * 3, torch.zeros(3, H, W), iterations=3, lr=0.1)
    assert torch.equal(out.cpu(), uv) and stats["vertices_moved"] == 0 and stats["max_offset"] == 0.0 and stats["mse_after"] == 0.0
