"""The vertex-colour refinement of libv3d_recon.so (csrc_recon/meshshade.hip, v3d_amd/recon/mesh_refine.py, scripts/pub/refine_mesh.py)
without a GPU: header, ctypes table and exports agree, bad arguments are refused before any launch, the script's options parse, and the
torch restatement (tests/mesh_refine_ref.py) is honest: its transpose is autograd's, its Adam is torch.optim.Adam's, and its refinement
loop converges on the end-to-end scene of tests/test_mesh_refine_gpu.py, whose views keep mesh_render_ref's depth margins."""
import ctypes as C
import importlib.util
import os
import re

import numpy as np
import pytest
import torch

import gs_dense_ref as D
import mesh_refine_ref as RF
import mesh_render_ref as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REFINE_ENTRIES = {"v3d_recon_mesh_pixel_weights", "v3d_recon_mesh_shade", "v3d_recon_mesh_vertex_records", "v3d_recon_mesh_vertex_ranges",
                  "v3d_recon_mesh_shade_bwd", "v3d_recon_mesh_color_adam"}


@pytest.fixture(scope="module")
def lib():
    from v3d_amd.build import build_recon
    from v3d_amd.recon import geometry
    build_recon(verbose=False)
    return geometry.load_library()


def test_header_signatures_and_exports_agree(lib):
    from v3d_amd.recon import geometry
    hdr = open(os.path.join(ROOT, "include", "v3d_recon.h")).read()
    declared = set(re.findall(r"\b(v3d_recon_[a-z_0-9]+)\s*\(", hdr))
    assert REFINE_ENTRIES <= declared and REFINE_ENTRIES <= set(geometry.SIGNATURES)
    for name in REFINE_ENTRIES:
        assert hasattr(lib, name), f"{name} is not exported"
        proto = re.search(r"\bint " + name + r"\s*\(([^;]*)\);", hdr).group(1)
        assert len(proto.split(",")) == len(geometry.SIGNATURES[name][1]), f"{name}: the ctypes row and the prototype differ in length"
    assert lib.v3d_recon_abi_version() == geometry.ABI_VERSION == 1          # the new entries are additive
    assert os.path.exists(os.path.join(ROOT, "v3d_amd", "csrc_recon", "meshshade.hip"))


def test_bad_arguments_are_refused_before_any_launch(lib):
    # (no GPU here: an entry that reached its launch would fail differently, or crash; `p` is never dereferenced by the host code)
    p = 0x1000
    err = lambda: lib.v3d_recon_last_error().decode()  # noqa: E731

    def calls(fn, order, **defaults):
        return lambda **kw: fn(*[kw.get(k, defaults[k]) for k in order])

    # pixel_weights
    pw = calls(lib.v3d_recon_mesh_pixel_weights, ("face_id", "faces", "F", "pix_q", "zv", "V", "W", "H", "bits", "pix_vert", "pix_w", "stream"),
               face_id=p, faces=p, F=4, pix_q=p, zv=p, V=8, W=32, H=32, bits=8, pix_vert=p, pix_w=p, stream=None)
    for k in ("face_id", "faces", "pix_q", "zv", "pix_vert", "pix_w"):
        assert pw(**{k: None}) == -1 and "v3d_recon_mesh_pixel_weights" in err() and "null" in err(), k
    assert pw(F=0) == -1 and "positive" in err()
    assert pw(V=0) == -1 and "positive" in err()
    assert pw(bits=9) == -1 and "subpixel_bits 9" in err()
    assert pw(bits=-1) == -1 and "subpixel_bits" in err()
    assert pw(W=4097) == -1 and "4097" in err() and "4096" in err()
    assert pw(H=0) == -1 and "4096" in err()
    # shade
    sh = calls(lib.v3d_recon_mesh_shade, ("pix_vert", "pix_w", "depth", "colors", "V", "W", "H", "b0", "b1", "b2", "image", "stream"),
               pix_vert=p, pix_w=p, depth=p, colors=p, V=8, W=32, H=32, b0=1.0, b1=1.0, b2=1.0, image=p, stream=None)
    for k in ("pix_vert", "pix_w", "depth", "colors", "image"):
        assert sh(**{k: None}) == -1 and "v3d_recon_mesh_shade:" in err() and "null" in err(), k
    assert sh(V=0) == -1 and "positive" in err()
    assert sh(W=-3) == -1 and "4096" in err()
    assert sh(H=4097) == -1 and "4097" in err()
    # vertex_records
    vr = calls(lib.v3d_recon_mesh_vertex_records, ("pix_vert", "offsets", "W", "H", "n", "keys", "vals", "stream"),
               pix_vert=p, offsets=p, W=32, H=32, n=30, keys=p, vals=p, stream=None)
    for k in ("pix_vert", "offsets", "keys", "vals"):
        assert vr(**{k: None}) == -1 and "v3d_recon_mesh_vertex_records" in err() and "null" in err(), k
    assert vr(n=0) == -1 and "num_records 0" in err()
    assert vr(n=31) == -1 and "multiple of 3" in err()
    assert vr(n=3 * 32 * 32 + 3) == -1 and "num_records" in err()
    assert vr(W=4097) == -1 and "4096" in err()
    # vertex_ranges (no record at all is legal, with a null list)
    assert lib.v3d_recon_mesh_vertex_ranges(p, 6, 8, None, None) == -1 and "v3d_recon_mesh_vertex_ranges" in err() and "null" in err()
    assert lib.v3d_recon_mesh_vertex_ranges(None, 6, 8, p, None) == -1 and "null" in err()
    assert lib.v3d_recon_mesh_vertex_ranges(p, -1, 8, p, None) == -1 and "negative" in err()
    assert lib.v3d_recon_mesh_vertex_ranges(p, 6, 0, p, None) == -1 and "positive" in err()
    # shade_bwd (no entry at all is legal, with null lists)
    bw = calls(lib.v3d_recon_mesh_shade_bwd, ("ranges", "ent_pix", "ent_w", "n", "dL", "W", "H", "V", "out", "stream"),
               ranges=p, ent_pix=p, ent_w=p, n=6, dL=p, W=32, H=32, V=8, out=p, stream=None)
    for k in ("ranges", "ent_pix", "ent_w", "dL", "out"):
        assert bw(**{k: None}) == -1 and "v3d_recon_mesh_shade_bwd" in err() and "null" in err(), k
    assert bw(n=-1) == -1 and "negative" in err()
    assert bw(V=0) == -1 and "positive" in err()
    assert bw(W=0) == -1 and "4096" in err()
    assert bw(H=5000) == -1 and "5000" in err()
    # color_adam
    ad = calls(lib.v3d_recon_mesh_color_adam, ("logit", "m", "v", "grad", "V", "lr", "b1", "b2", "eps", "step", "colors", "stream"),
               logit=p, m=p, v=p, grad=p, V=8, lr=1e-3, b1=0.9, b2=0.999, eps=1e-8, step=1, colors=p, stream=None)
    for k in ("logit", "m", "v", "grad", "colors"):
        assert ad(**{k: None}) == -1 and "v3d_recon_mesh_color_adam" in err() and "null" in err(), k
    assert ad(V=0) == -1 and "positive" in err()
    assert ad(step=0) == -1 and "step 0" in err()
    assert ad(lr=-1.0) == -1 and "lr" in err()
    assert ad(b1=1.0) == -1 and "beta" in err()
    assert ad(b2=-0.1) == -1 and "beta" in err()
    assert ad(eps=0.0) == -1 and "eps" in err()
    assert ad(lr=float("nan")) == -1 and "lr" in err()


def _entry(name):
    spec = importlib.util.spec_from_file_location("v3d_entry_" + name, os.path.join(ROOT, "scripts", "pub", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_script_options_parse_with_the_reconstructions_defaults():
    mod = _entry("refine_mesh")
    ap = mod.build_parser()
    a = vars(ap.parse_args(["--mesh", "out/gs/mesh.ply", "--video", "out/000000.npy", "-o", "out/gs/refined.ply", "-w"]))
    assert a == {"mesh": "out/gs/mesh.ply", "video": "out/000000.npy", "out": "out/gs/refined.ply", "white_background": True, "iters": 2000,
                 "num_opt": 4, "lr": 1e-3, "seed": 0, "lpips": 0.0, "num_frames": None, "radius": 2.0, "elevation": 0.0, "fov": 60.0,
                 "render_orbit": 0}
    recon = vars(_entry("recon_from_vid").build_parser().parse_args(["--video", "x.npy"]))
    for k in ("radius", "elevation", "fov", "seed", "num_frames", "white_background"):
        assert vars(ap.parse_args(["--mesh", "m.ply", "--video", "x.npy"]))[k] == recon[k], k
    with pytest.raises(SystemExit):
        ap.parse_args(["--video", "x.npy"])              # --mesh is required
    with pytest.raises(SystemExit):
        ap.parse_args(["--mesh", "m.ply"])               # --video is required
    # the reference's perceptual term: 0 is accepted, anything else refused before anything is read, in check_options' words
    from v3d_amd.recon.train import check_options
    with pytest.raises(NotImplementedError) as theirs:
        check_options(0, 1.0)
    with pytest.raises(NotImplementedError) as ours:
        mod.main(["--mesh", "does/not/exist.ply", "--video", "does/not/exist.npy", "--lpips", "1"])
    assert str(ours.value) == str(theirs.value).replace("--lambda_lpips", "--lpips")
    mod.check_lpips(0.0)


def test_host_api_refuses_what_does_not_fit_and_shades_the_empty_mesh():
    from v3d_amd.recon import mesh_refine as RFN
    cams = D.cams_for(32, 32)
    v, f = M.icosphere(0)
    c = M.position_colors(v)
    with pytest.raises(ValueError, match="does not match"):
        RFN.refine_vertex_colors(v, f, c, cams, torch.zeros(4, 3, 32, 40), device="cpu")
    with pytest.raises(ValueError, match="3 images for 4 cameras"):
        RFN.refine_vertex_colors(v, f, c, cams, torch.zeros(3, 3, 32, 32), device="cpu")
    with pytest.raises(ValueError, match="outside the vertex array"):
        RFN.prepare_view(cams[0], v, f + 1, [1, 1, 1], device="cpu")
    assert RFN.optimisation_views(18, 4) == [0, 4, 9, 13] == RF.optimisation_views(18, 4)          # the reference's linspace, truncated
    assert RFN.optimisation_views(8, 4) == [0, 2, 4, 6] and RFN.optimisation_views(5, 0) == [0, 1, 2, 3, 4] == RF.optimisation_views(5, 0)
    assert RFN.view_schedule(4, 50, 3) == RF.view_schedule(4, 50, 3) and set(RFN.view_schedule(4, 50, 3)) == {0, 1, 2, 3}
    assert RFN.view_schedule(4, 50, 3) != RFN.view_schedule(4, 50, 4)
    c8 = torch.tensor([[0.0, 1.0, 0.5]])
    assert torch.equal(RFN.initial_logits(c8), RF.initial_logits(c8, torch.float32)) and bool(torch.isfinite(RFN.initial_logits(c8)).all())
    # V = 0 / F = 0: the background, zero gradients, no launch (so it runs here)
    for vv, ff in ((torch.zeros(0, 3), torch.zeros(0, 3, dtype=torch.int64)), (v, torch.zeros(0, 3, dtype=torch.int64))):
        view = RFN.prepare_view(D.cams_for(56, 40)[0], vv, ff, [0.25, 0.5, 1.0], device="cpu")
        assert not view.launch and view.ent_pix.numel() == 0 and tuple(view.ranges.shape) == (vv.shape[0], 2)
        cc = torch.rand(vv.shape[0], 3, requires_grad=True)
        with torch.enable_grad():                          # (a module of the suite may have switched autograd off for the process)
            img = RFN.shade(view, cc)
            (img * torch.rand(3, 40, 56)).sum().backward()
        assert img.shape == (3, 40, 56) and torch.equal(img[:, 7, 9], torch.tensor([0.25, 0.5, 1.0]))
        assert cc.grad.shape == cc.shape and not cc.grad.any()
        out, stats = RFN.refine_vertex_colors(vv, ff, cc.detach(), D.cams_for(56, 40), torch.ones(4, 3, 40, 56), iterations=5, device="cpu")
        assert torch.equal(out, cc.detach()) and stats["vertices_seen"] == 0 and stats["loss_first"] is None


# ---- the restatement's own honesty ----------------------------------------------------------------------------------------------------
def _frozen(case, dtype=torch.float64):
    kind, seed, W, H, _, cull = case[:6]
    bits = M.case_bits(case)
    v, f, c = M.mesh_scene(kind, seed)
    pr = M.project(v, M.case_camera(case), bits, torch.float32)
    r = M.rasterize(pr["pix_q"], pr["zv"], f, c, W, H, RF.BG, bits=bits, cull=cull)
    return v, f, c, pr, r, RF.frozen_view(pr["pix_q"], pr["zv"], f, r["face_id"], r["depth"], v.shape[0], dtype, bits)


@pytest.mark.parametrize("case", (M.RASTER_CASES[0], M.RASTER_CASES[9]) + M.REFINE_EDGE_CASES, ids=M.any_case_id)
def test_restatement_shades_what_the_rasterizer_restatement_shades_and_its_transpose_is_autograd(case):
    v, f, c, pr, r, fz = _frozen(case)
    V = v.shape[0]
    assert torch.equal(fz["pix_vert"][r["face_id"] >= 0], f[r["face_id"][r["face_id"] >= 0]]) and bool((fz["pix_vert"][r["face_id"] < 0] == -1).all())
    assert not fz["pix_w"][r["face_id"] < 0].any()
    img = RF.shade(fz["pix_vert"], fz["pix_w"], fz["depth"], c, RF.BG)
    assert float((img - r["image"]).abs().max()) <= 1e-14                          # mesh_render_ref's image, from the frozen record
    g = torch.Generator().manual_seed(5)
    dL = torch.randn(3, case[3], case[2], generator=g, dtype=torch.float64)
    assert bool((dL[:, r["face_id"] < 0] != 0).all())                              # gradients on background pixels too
    cc = c.double().requires_grad_(True)
    with torch.enable_grad():                              # (a module of the suite may have switched autograd off for the process)
        (RF.shade(fz["pix_vert"], fz["pix_w"], fz["depth"], cc, RF.BG) * dL).sum().backward()
    mine = RF.shade_transpose(fz["pix_vert"], fz["pix_w"], fz["depth"], dL, V)
    assert float((mine - cc.grad).abs().max()) <= 1e-12 * float(cc.grad.abs().max())
    table, length = fz["lists"]
    assert int(length.sum()) == 3 * int((r["face_id"] >= 0).sum()) and 0 < int((length == 0).sum()) < V       # some vertices face away
    assert not mine[length == 0].any() and bool((cc.grad[length == 0] == 0).all())
    for row, n in zip(table.tolist(), length.tolist()):
        assert row[:n] == sorted(row[:n]) and all(x == -1 for x in row[n:])        # ascending pixel order


def test_restatement_adam_is_torch_adam():
    g = torch.Generator().manual_seed(2)
    logit0 = torch.randn(33, 3, generator=g, dtype=torch.float64)
    target, mask = torch.rand(33, 3, generator=g, dtype=torch.float64), (torch.rand(33, 1, generator=g) > 0.3).double()
    param = logit0.clone().requires_grad_(True)
    opt = torch.optim.Adam([param], lr=0.05)
    logit, m, v = logit0.clone(), torch.zeros_like(logit0), torch.zeros_like(logit0)
    for step in range(1, 6):
        opt.zero_grad()
        with torch.enable_grad():
            (0.5 * mask * (torch.sigmoid(param) - target) ** 2).sum().backward()
        opt.step()
        RF.adam_step(logit, m, v, mask * (RF.sigmoid(logit) - target), step, 0.05)
    assert float((logit - param.detach()).abs().max()) <= 1e-13
    assert torch.equal(logit[mask[:, 0] == 0], logit0[mask[:, 0] == 0]) and float((logit - logit0).abs().max()) > 0.1


@pytest.fixture(scope="module")
def e2e():
    v, f, target = RF.e2e_mesh()
    cams = RF.e2e_cameras()
    S = RF.E2E["size"]
    views = []
    for cam in cams:
        pr = M.project(v, cam, 8, torch.float32)
        assert not pr["marked"].any()
        views.append((pr, M.rasterize(pr["pix_q"], pr["zv"], f, target, S, S, RF.BG, cull=True)))
    return v, f, target, cams, views


def test_e2e_scene_keeps_the_depth_margin(e2e):
    v, f, target, cams, views = e2e
    assert v.shape[0] > 500 and f.shape[0] > 1000
    for pr, r in views:
        r32 = M.rasterize(pr["pix_q"], pr["zv"], f, target, RF.E2E["size"], RF.E2E["size"], RF.BG, cull=True, dtype=torch.float32)
        gap, err = float(r["gap"].min()), float((r32["depth"].double() - r["depth"]).abs().max())
        print(f"smallest gap {gap:.3e}, float32 restatement z error {err:.3e}")
        assert gap >= M.Z_GAP_MARGIN and err <= M.Z_FP32_ERR and torch.equal(r32["face_id"], r["face_id"])
        assert 0.1 < float(r["alpha"].mean()) < 0.6


def test_restatement_refinement_converges(e2e):
    """LR and ITERATIONS of mesh_refine_ref are inputs, fixed here: with them the fp64 restatement brings the mean squared error over the
    four optimisation views from grey to a tenth at most."""
    v, f, target, cams, views = e2e
    V = v.shape[0]
    assert RF.ITERATIONS <= 300
    opt = RF.optimisation_views(len(cams), RF.E2E["num_opt"])
    assert opt == [0, 2, 4, 6]
    fz = [RF.frozen_view(views[i][0]["pix_q"], views[i][0]["zv"], f, views[i][1]["face_id"], views[i][1]["depth"], V) for i in opt]
    grey = torch.full((V, 3), 0.5)
    res = RF.refine(fz, [views[i][1]["image"] for i in opt], grey, RF.ITERATIONS, RF.LR, RF.E2E["seed"], RF.BG)
    print(f"mse {res['mse_before']:.4e} -> {res['mse_after']:.4e}; loss {res['loss_first']:.4e} -> {res['loss_last']:.4e}; "
          f"{int(res['seen'].sum())} of {V} vertices seen")
    assert res["mse_after"] <= 0.1 * res["mse_before"]
    assert 0 < int((~res["seen"]).sum()) < V // 2                                  # the poles: no optimisation view sees them
    assert torch.equal(res["colors"][~res["seen"]], grey[~res["seen"]].double())
    again = RF.refine(fz, [views[i][1]["image"] for i in opt], grey, RF.ITERATIONS, RF.LR, RF.E2E["seed"], RF.BG)
    assert torch.equal(again["colors"], res["colors"])
