"""The gfx950 vertex-colour refinement (csrc_recon/meshshade.hip, v3d_amd/recon/mesh_refine.py, scripts/pub/refine_mesh.py) against the torch
restatement (tests/mesh_refine_ref.py): per-pixel vertices and weights, the shade, its transpose on real views, on synthetic lists and on a
full-image quad, Adam on logits against torch.optim.Adam, the whole refinement on the project's own extracted sphere, the entry point, and
the empty cases.  The weights, the shade and the transpose also run at 0, 4 and 7 sub-pixel bits on odd images and on one below a tile
(mesh_render_ref.REFINE_EDGE_CASES).  The restatement is fed the KERNEL'S OWN snapped positions, view z, face_id and depth, as
tests/test_mesh_render_gpu.py does.

The bar everywhere is that file's: the kernel may be off from the fp64 restatement by 4x what the restatement's own float32 run is off.
For the transposes "off" is measured two ways (mesh_refine_ref.row_errors): relative L2 over all rows, and the largest relative L2 of a
single row among the rows whose norm is above 1e-3 of the largest row's; each figure of the kernel is held to 4x the same figure of the
float32 restatement, which adds every list in the kernel's order (64 strided partial sums, then the butterfly: mesh_refine_ref.list_sum
says why)."""
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import gs_dense_ref as D
import mesh_refine_ref as RF
import mesh_render_ref as M
import recon_geom_ref as R
from conftest import record_parity
from v3d_amd.recon import geometry as G
from v3d_amd.recon import mesh_refine as RFN
from v3d_amd.recon import mesh_render as MR
from v3d_amd.recon.rasterize import gs_camera

pytestmark = pytest.mark.gpu
DEV = "cuda"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BG = [0.25, 0.5, 1.0]


@functools.lru_cache(maxsize=None)
def frozen(case):
    """The kernel's view of a raster case (of RASTER_CASES at 8 sub-pixel bits, or of EDGE_CASES at its own) and both restatements of it,
    computed once and shared (nothing below writes into them)"""
    kind, seed, W, H, _, cull = case[:6]
    bits = M.case_bits(case)
    cam = M.case_camera(case)
    v, f, c = M.mesh_scene(kind, seed)
    gc = gs_camera(cam, BG)
    zv, _, pix_q = MR.project_vertices(gc, v.to(DEV), bits)
    view = RFN.prepare_view(cam, v, f, BG, cull=cull, subpixel_bits=bits)
    host = dict(zv=zv.cpu(), pix_q=pix_q.cpu(), face_id=view.face_id.cpu(), depth=view.depth.cpu())
    fz = {dt: RF.frozen_view(host["pix_q"], host["zv"], f, host["face_id"], host["depth"], v.shape[0], dt, bits) for dt in (torch.float64, torch.float32)}
    return cam, v, f, c, view, host, fz


# every case of 8 sub-pixel bits, and 0, 4 and 7 bits on odd images and on one below a tile (mesh_render_ref.REFINE_EDGE_CASES)
REFINE_CASES = M.RASTER_CASES + M.REFINE_EDGE_CASES


def lists_of(view):
    """(vertex [n], pixel [n]) of the kernel's lists, entry by entry, from its ranges"""
    r = view.ranges.cpu().long()
    n = view.ent_pix.numel()
    owner = torch.full((n,), -1, dtype=torch.long)
    for vtx in torch.nonzero(r[:, 1] > r[:, 0]).reshape(-1).tolist():
        owner[r[vtx, 0]:r[vtx, 1]] = vtx
    return owner, view.ent_pix.cpu().long()


# ---- 1. weights and shade ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", REFINE_CASES, ids=M.any_case_id)
def test_weights_and_shade_match_the_restatement(case):
    cam, v, f, c, view, host, fz = frozen(case)
    _, _, W, H, _, cull = case[:6]
    bits = M.case_bits(case)
    fid = host["face_id"].long()
    hit = fid >= 0
    assert 0.1 < float(hit.double().mean()) < 0.6
    pv = view.pix_vert.cpu().long()
    assert view.pix_vert.dtype == torch.int32 and tuple(pv.shape) == (H, W, 3)
    assert torch.equal(pv[hit], f[fid[hit]]) and bool((pv[~hit] == -1).all())
    assert torch.equal(pv, fz[torch.float64]["pix_vert"])
    pw = view.pix_w.cpu()
    assert not pw[~hit].any()
    werr = float((pw.double() - fz[torch.float64]["pix_w"]).abs().max())
    werr32 = float((fz[torch.float32]["pix_w"].double() - fz[torch.float64]["pix_w"]).abs().max())
    img = RFN.shade(view, c.to(DEV)).cpu()
    ref = RF.shade(fz[torch.float64]["pix_vert"], fz[torch.float64]["pix_w"], fz[torch.float64]["depth"], c, BG)
    ref32 = RF.shade(fz[torch.float32]["pix_vert"], fz[torch.float32]["pix_w"], fz[torch.float32]["depth"], c, BG, torch.float32)
    ierr, ierr32 = float((img.double() - ref).abs().max()), float((ref32.double() - ref).abs().max())
    full = MR.render_mesh(cam, v, f, c, BG, cull=cull, subpixel_bits=bits)
    same = bool(torch.equal(full["render"].cpu(), img))
    print(f"pix_w {werr:.3e} (float32 restatement {werr32:.3e})  image {ierr:.3e} ({ierr32:.3e})  bit-equal to render_mesh: {same}")
    record_parity(f"mesh_refine_shade[{M.any_case_id(case)}]", {"pix_w_max_abs": werr, "pix_w_float32_restatement": werr32, "image_max_abs": ierr,
                                                            "image_float32_restatement": ierr32, "bit_equal_to_render_mesh": same})
    assert torch.equal(full["face_id"].cpu(), host["face_id"]) and torch.equal(full["depth"].cpu(), host["depth"])      # the same forward
    assert torch.equal(img[:, ~hit], torch.tensor(BG).view(3, 1).expand(3, int((~hit).sum())))
    assert werr <= 4 * werr32 and ierr <= 4 * ierr32


# ---- 2. the transpose on real views -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", REFINE_CASES, ids=M.any_case_id)
def test_transpose_matches_the_restatement_on_real_views(case):
    cam, v, f, c, view, host, fz = frozen(case)
    _, _, W, H, _, _ = case[:6]
    V = v.shape[0]
    g = torch.Generator().manual_seed(7)
    dL = torch.randn(3, H, W, generator=g)
    assert bool((dL[:, host["face_id"] < 0] != 0).all())                      # gradients on background pixels too
    # the lists: every vertex's entries are the restatement's, in ascending pixel order (the sort is stable)
    table, length = fz[torch.float64]["lists"]
    owner, pix = lists_of(view)
    assert pix.numel() == int(length.sum()) == 3 * int((host["face_id"] >= 0).sum()) and bool((owner >= 0).all())
    r = view.ranges.cpu().long()
    assert torch.equal(r[:, 1] - r[:, 0], length) and bool((r[length == 0] == 0).all())
    flat = table[table >= 0]                                                  # row-major: vertex by vertex, list order
    want_owner = torch.repeat_interleave(torch.arange(V), length)
    order = torch.argsort(r[:, 0][length > 0])                                # vertices in the order their ranges lie in the kernel's list
    assert torch.equal(order, torch.arange(order.numel()))                    # sorted by vertex
    assert torch.equal(owner, want_owner) and torch.equal(pix, torch.div(flat, 3, rounding_mode="floor"))
    depth_w = (fz[torch.float32]["depth"].reshape(-1, 1) * view.pix_w.cpu().reshape(-1, 3)).reshape(-1)
    assert torch.equal(view.ent_w.cpu(), depth_w[flat])
    # the gradient, through autograd
    cc = c.to(DEV).requires_grad_(True)
    with torch.enable_grad():                              # (a module of the suite may have switched autograd off for the process)
        (RFN.shade(view, cc) * dL.to(DEV)).sum().backward()
    out = cc.grad.cpu()
    again = RFN.shade_backward(view, dL.to(DEV)).cpu()
    assert torch.equal(out, again), "two runs of the transpose differ"
    ref = RF.shade_transpose(fz[torch.float64]["pix_vert"], fz[torch.float64]["pix_w"], fz[torch.float64]["depth"], dL, V, torch.float64,
                             fz[torch.float64]["lists"])
    ref32 = RF.shade_transpose(fz[torch.float32]["pix_vert"], fz[torch.float32]["pix_w"], fz[torch.float32]["depth"], dL, V, torch.float32,
                               fz[torch.float32]["lists"])
    (rel, row), (rel32, row32) = RF.row_errors(out, ref), RF.row_errors(ref32, ref)
    print(f"dL_dcolors rel L2 {rel:.3e} (float32 restatement {rel32:.3e})  worst row {row:.3e} ({row32:.3e})  {int((length == 0).sum())} of {V} rows empty")
    record_parity(f"mesh_refine_transpose[{M.any_case_id(case)}]", {"rel_l2": rel, "rel_l2_float32_restatement": rel32, "worst_row_rel": row,
                                                                "worst_row_rel_float32_restatement": row32, "longest_list": int(length.max())})
    assert 0 < int((length == 0).sum()) < V and not out[length == 0].any()
    assert rel <= 4 * rel32 and row <= 4 * row32


# ---- 3. the transpose on synthetic lists and on a full-image quad ---------------------------------------------------------------------------
def test_transpose_on_synthetic_lists_of_every_length():
    W, H = 64, 48
    ranges, ent_pix, ent_w, dL = RF.synthetic_lists(W, H)
    V = ranges.shape[0]
    assert (ranges[:, 1] - ranges[:, 0]).tolist() == [0, 1, 63, 64, 65, 128, 700, 0]
    z = torch.zeros(H, W, device=DEV)
    view = RFN.MeshView(W, H, V, z, z, torch.full((H, W), -1, dtype=torch.int32, device=DEV), torch.full((H, W, 3), -1, dtype=torch.int32, device=DEV),
                        torch.zeros(H, W, 3, device=DEV), ranges.to(DEV), ent_pix.to(DEV), ent_w.to(DEV), torch.zeros(3, device=DEV))
    out = torch.full((V, 3), float("nan"), device=DEV)          # every row is written: nothing of this survives
    lib = G.load_library()
    assert lib.v3d_recon_mesh_shade_bwd(view.ranges.data_ptr(), view.ent_pix.data_ptr(), view.ent_w.data_ptr(), ent_pix.numel(), dL.to(DEV).data_ptr(),
                                        W, H, V, out.data_ptr(), None) == 0
    torch.cuda.synchronize()
    out = out.cpu()
    assert torch.equal(out, RFN.shade_backward(view, dL.to(DEV)).cpu())
    ref, ref32 = RF.synthetic_transpose(ranges, ent_pix, ent_w, dL), RF.synthetic_transpose(ranges, ent_pix, ent_w, dL, torch.float32)
    assert bool(torch.isfinite(out).all()) and not out[0].any() and not out[-1].any()
    assert torch.equal(out[1], ref32[1])                                      # one entry: one product
    per = lambda x: ((x.double() - ref).norm(dim=1) / ref.norm(dim=1).clamp_min(1e-300))[1:-1]  # noqa: E731
    (rel, row), (rel32, row32) = RF.row_errors(out, ref), RF.row_errors(ref32, ref)
    print(f"rows {per(out).tolist()}\nfloat32 restatement {per(ref32).tolist()}\nrel L2 {rel:.3e} ({rel32:.3e})  worst row {row:.3e} ({row32:.3e})")
    record_parity("mesh_refine_transpose_synthetic", {"rel_l2": rel, "rel_l2_float32_restatement": rel32, "worst_row_rel": row,
                                                      "worst_row_rel_float32_restatement": row32, "rows_rel": per(out).tolist(),
                                                      "rows_rel_float32_restatement": per(ref32).tolist()})
    assert rel <= 4 * rel32 and float(per(out).max()) <= 4 * float(per(ref32).max())


def test_full_image_quad_has_lists_of_thousands():
    W, H = 64, 48
    q, zv, faces, colors = RF.full_quad(W, H)
    gc = gs_camera(D.cams_for(W, H)[0], BG)
    view = RFN.freeze_projected(gc, faces.to(DEV, torch.int32).contiguous(), q.to(DEV, torch.int32).contiguous(), zv.to(DEV), BG, cull=True)
    assert bool((view.alpha == 1).all()) and set(view.face_id.unique().tolist()) == {0, 1}
    r = view.ranges.cpu().long()
    length = r[:, 1] - r[:, 0]
    assert length[0] == length[2] == W * H and int(length[1] + length[3]) == W * H and min(length.tolist()) > 1000
    fz = {dt: RF.frozen_view(q, zv, faces, view.face_id.cpu(), view.depth.cpu(), 4, dt) for dt in (torch.float64, torch.float32)}
    owner, pix = lists_of(view)
    table, _ = fz[torch.float64]["lists"]
    assert torch.equal(pix, torch.div(table[table >= 0], 3, rounding_mode="floor")) and torch.equal(owner, torch.repeat_interleave(torch.arange(4), length))
    img = RFN.shade(view, colors.to(DEV)).cpu()
    ref = RF.shade(fz[torch.float64]["pix_vert"], fz[torch.float64]["pix_w"], fz[torch.float64]["depth"], colors, BG)
    ref32 = RF.shade(fz[torch.float32]["pix_vert"], fz[torch.float32]["pix_w"], fz[torch.float32]["depth"], colors, BG, torch.float32)
    ierr, ierr32 = float((img.double() - ref).abs().max()), float((ref32.double() - ref).abs().max())
    dL = torch.randn(3, H, W, generator=torch.Generator().manual_seed(9))
    out = RFN.shade_backward(view, dL.to(DEV)).cpu()
    assert torch.equal(out, RFN.shade_backward(view, dL.to(DEV)).cpu())
    t64 = RF.shade_transpose(fz[torch.float64]["pix_vert"], fz[torch.float64]["pix_w"], fz[torch.float64]["depth"], dL, 4, torch.float64)
    t32 = RF.shade_transpose(fz[torch.float32]["pix_vert"], fz[torch.float32]["pix_w"], fz[torch.float32]["depth"], dL, 4, torch.float32)
    (rel, row), (rel32, row32) = RF.row_errors(out, t64), RF.row_errors(t32, t64)
    print(f"image {ierr:.3e} ({ierr32:.3e})  dL_dcolors rel L2 {rel:.3e} (float32 restatement {rel32:.3e})  worst row {row:.3e} ({row32:.3e})")
    record_parity("mesh_refine_quad", {"image_max_abs": ierr, "image_float32_restatement": ierr32, "rel_l2": rel, "rel_l2_float32_restatement": rel32,
                                       "worst_row_rel": row, "worst_row_rel_float32_restatement": row32, "list_lengths": length.tolist()})
    assert ierr <= 4 * ierr32 and rel <= 4 * rel32 and row <= 4 * row32


# ---- 4. Adam ------------------------------------------------------------------------------------------------------------------------------
def test_adam_on_logits_is_torch_adam():
    V, lr, steps = 257, 0.05, 5
    g = torch.Generator().manual_seed(3)
    logit0 = 2.0 * torch.randn(V, 3, generator=g)
    target = torch.rand(V, 3, generator=g)
    mask = (torch.rand(V, 1, generator=g) > 0.25).float() * torch.pow(10.0, 2 * torch.rand(V, 1, generator=g) - 2)        # all-zero rows; 1e-2 .. 1
    zero = mask[:, 0] == 0
    assert 20 < int(zero.sum()) < 120

    def torch_adam(dtype):
        p = logit0.to(dtype).clone().requires_grad_(True)
        opt = torch.optim.Adam([p], lr=lr)
        for _ in range(steps):
            opt.zero_grad()
            with torch.enable_grad():
                (0.5 * mask.to(dtype) * (torch.sigmoid(p) - target.to(dtype)) ** 2).sum().backward()    # dL/dcolors = mask (colors - target)
            opt.step()
        return p.detach(), torch.sigmoid(p.detach())

    (l64, c64), (l32, c32) = torch_adam(torch.float64), torch_adam(torch.float32)
    logit = logit0.to(DEV).contiguous()
    m, s = torch.zeros_like(logit), torch.zeros_like(logit)
    colors = torch.sigmoid(logit)
    for step in range(1, steps + 1):
        grad = (mask.to(DEV) * (colors - target.to(DEV))).contiguous()
        RFN.color_adam(logit, m, s, grad, colors, step, lr)
    lerr, cerr = float((logit.cpu().double() - l64).abs().max()), float((colors.cpu().double() - c64).abs().max())
    lerr32, cerr32 = float((l32.double() - l64).abs().max()), float((c32.double() - c64).abs().max())
    print(f"logits {lerr:.3e} (float32 torch.optim.Adam {lerr32:.3e})  colours {cerr:.3e} ({cerr32:.3e})")
    record_parity("mesh_refine_adam", {"logit_max_abs": lerr, "logit_float32_torch": lerr32, "color_max_abs": cerr, "color_float32_torch": cerr32})
    assert torch.equal(logit.cpu()[zero], logit0[zero]) and not m.cpu()[zero].any() and not s.cpu()[zero].any()
    assert float((l64 - logit0.double()).abs()[~zero].median()) > 0.1                                   # the other rows moved: about lr a step
    assert lerr <= 4 * lerr32 and cerr <= 4 * cerr32


# ---- 5. end to end ------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def sphere():
    N, S = RF.E2E["N"], RF.E2E["size"]
    ref = R.sphere_volume(N, RF.E2E["bound"], RF.E2E["radius"])
    f32 = lambda t, *s: t.float().reshape(*s).contiguous().to(DEV)  # noqa: E731
    vol = G.TsdfVolume(N, ref["bound"], ref["trunc"], f32(ref["tsdf_sum"], N, N, N), f32(ref["weight"], N, N, N), f32(ref["rgb_sum"], 3, N, N, N),
                       f32(ref["rgb_weight"], N, N, N))
    verts, faces, _ = G.extract_mesh(vol)
    target = M.position_colors(verts.cpu(), RF.E2E["tint"]).to(DEV)
    cams = RF.e2e_cameras()
    frames = torch.stack([MR.render_mesh(cam, verts, faces, target, RF.BG)["render"] for cam in cams])
    return verts, faces, target, cams, frames


def test_refinement_end_to_end(sphere):
    verts, faces, target, cams, frames = sphere
    V, S = verts.shape[0], RF.E2E["size"]
    assert V > 500 and tuple(frames.shape) == (8, 3, S, S)
    grey = torch.full((V, 3), 0.5, device=DEV)
    kw = dict(iterations=RF.ITERATIONS, lr=RF.LR, num_opt=RF.E2E["num_opt"], white_background=True, seed=RF.E2E["seed"])
    out, stats = RFN.refine_vertex_colors(verts, faces, grey, cams, frames, **kw)
    again, _ = RFN.refine_vertex_colors(verts, faces, grey, cams, frames, **kw)
    assert torch.equal(out, again), "two calls with the same arguments differ"
    assert stats["opt_views"] == [0, 2, 4, 6] and stats["iterations"] == RF.ITERATIONS
    # the restatement, on the kernel's own views
    views = [RFN.prepare_view(cams[i], verts, faces, RF.BG) for i in stats["opt_views"]]
    gt = frames.clamp(0, 1)
    mse = lambda c: float(np.mean([float(((RFN.shade_forward(vw, c) - gt[i]) ** 2).mean()) for vw, i in zip(views, stats["opt_views"])]))  # noqa: E731
    before, after = mse(grey), mse(out)
    res = {}
    for dt in (torch.float64, torch.float32):
        fz = []
        for vw, i in zip(views, stats["opt_views"]):
            zv, _, pix_q = MR.project_vertices(gs_camera(cams[i], RF.BG), verts)
            fz.append(RF.frozen_view(pix_q.cpu(), zv.cpu(), faces.cpu().long(), vw.face_id.cpu(), vw.depth.cpu(), V, dt))
        res[dt] = RF.refine(fz, [gt[i].cpu() for i in stats["opt_views"]], grey.cpu(), RF.ITERATIONS, RF.LR, RF.E2E["seed"], RF.BG, dt)
    r64, r32 = res[torch.float64], res[torch.float32]
    cerr = float((out.cpu().double() - r64["colors"]).abs().max())
    cerr32 = float((r32["colors"].double() - r64["colors"]).abs().max())
    seen = r64["seen"]
    print(f"mse {before:.4e} -> {after:.4e} (restatement {r64['mse_before']:.4e} -> {r64['mse_after']:.4e}); colours {cerr:.3e} from fp64 (float32 "
          f"restatement {cerr32:.3e}); PSNR {stats['psnr_before']:.2f} -> {stats['psnr_after']:.2f} dB; {int(seen.sum())} of {V} vertices seen")
    record_parity("mesh_refine_e2e", {"mse_before": before, "mse_after": after, "restatement_mse_after": r64["mse_after"], "colors_max_abs": cerr,
                                      "colors_float32_restatement": cerr32, "psnr_before": stats["psnr_before"], "psnr_after": stats["psnr_after"],
                                      "loss_first": stats["loss_first"], "loss_last": stats["loss_last"], "vertices": V, "vertices_seen": int(seen.sum()),
                                      "lr": RF.LR, "iterations": RF.ITERATIONS})
    assert stats["vertices_seen"] == int(seen.sum()) and 0 < int((~seen).sum()) < V // 2
    assert torch.equal(out.cpu()[~seen], grey.cpu()[~seen])                    # unseen: bit-unchanged
    assert float((out.cpu()[seen] != 0.5).any(1).float().mean()) > 0.9        # seen: moved (a vertex that a view barely sees may not)
    assert abs(stats["loss_first"] - r64["loss_first"]) <= 1e-6 * r64["loss_first"]
    assert after <= 0.1 * before
    assert cerr <= 4 * cerr32
    assert stats["psnr_after"] > stats["psnr_before"]


def test_refine_mesh_script_end_to_end(sphere, tmp_path):
    verts, faces, target, cams, _ = sphere
    V = verts.shape[0]
    ply, video, out = str(tmp_path / "mesh.ply"), str(tmp_path / "video.npy"), str(tmp_path / "refined.ply")
    G.save_mesh_ply(ply, verts, faces, torch.full((V, 3), 0.5))
    np.save(video, MR.render_mesh_orbit(verts, faces, target, 8, *RF.E2E["orbit"], RF.E2E["size"], True))
    r = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "pub", "refine_mesh.py"), "--mesh", ply, "--video", video, "-o", out, "-w",
                        "--iters", str(RF.ITERATIONS), "--lr", str(RF.LR), "--render_orbit", "2"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "PSNR mean over all frames" in r.stdout and "views [0, 2, 4, 6]" in r.stdout
    assert sorted(os.listdir(tmp_path)) == ["mesh.ply", "refined.json", "refined.ply", "refined_orbit", "video.npy"]
    assert sorted(os.listdir(tmp_path / "refined_orbit")) == ["000.png", "001.png", "orbit.npy"]
    stats = json.load(open(tmp_path / "refined.json"))
    assert {"psnr_before", "psnr_after", "opt_views", "loss_first", "loss_last", "seconds", "iterations", "vertices_seen"} <= set(stats)
    assert stats["psnr_after"] > stats["psnr_before"] and stats["opt_views"] == [0, 2, 4, 6] and stats["iterations"] == RF.ITERATIONS
    rv, rf, rc = G.read_mesh_ply(out)
    assert np.array_equal(rv, verts.cpu().numpy()) and np.array_equal(rf, faces.cpu().numpy())             # the geometry is held fixed
    moved = (rc != 128).any(1)
    assert 0.9 * stats["vertices_seen"] < int(moved.sum()) <= stats["vertices_seen"] < V           # unseen vertices keep their 8-bit grey


# ---- 6. empty cases -----------------------------------------------------------------------------------------------------------------------
def test_empty_views_shade_to_the_background_and_give_zero_gradients():
    W, H = 56, 40
    cam = D.cams_for(W, H)[1]
    bgt = torch.tensor(BG).view(3, 1, 1).expand(3, H, W)
    dL = torch.randn(3, H, W, generator=torch.Generator().manual_seed(1)).to(DEV)
    uv, uf, uc, _ = M.undrawn_mesh(cam)                                        # V, F > 0 and nothing drawn: the kernels run on empty lists
    meshes = [(uv, uf, True), (torch.zeros(0, 3), torch.zeros(0, 3, dtype=torch.int64), False), (uv, torch.zeros(0, 3, dtype=torch.int64), False)]
    for vv, ff, launch in meshes:
        view = RFN.prepare_view(cam, vv, ff, BG)
        assert view.launch == launch and view.ent_pix.numel() == 0 and not view.ranges.any() and bool((view.pix_vert == -1).all())
        cc = torch.rand(vv.shape[0], 3).to(DEV).requires_grad_(True)
        with torch.enable_grad():
            img = RFN.shade(view, cc)
            (img * dL).sum().backward()
        assert torch.equal(img.cpu(), bgt)
        assert tuple(cc.grad.shape) == (vv.shape[0], 3) and not cc.grad.any()
        out, stats = RFN.refine_vertex_colors(vv, ff, cc.detach(), [cam] * 4, torch.ones(4, 3, H, W), iterations=3, num_opt=2, lr=0.1)   # (undrawn from `cam`; white frames)
        assert torch.equal(out, cc.detach()) and stats["vertices_seen"] == 0 and stats["psnr_after"] == stats["psnr_before"] == float("inf")
