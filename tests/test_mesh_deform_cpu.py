"""The silhouette fit of libv3d_recon.so (csrc_recon/meshdeform.hip, v3d_amd/recon/mesh_deform.py, scripts/pub/fit_mesh.py) without a GPU:
header, ctypes table and exports agree, bad arguments are refused before any launch, the script's options parse, and the torch restatement
(tests/mesh_deform_ref.py) is honest: its explicit backward is autograd's of its forward with frozen decisions, its projection backward is
autograd's of mesh_render_ref.project's statements, its smoothness gradient is autograd's of the energy, its scenes keep their decision
margins, its hand-placed scenes are what they claim, and its loop reaches the figure recorded for the end-to-end scene."""
import ctypes as C
import importlib.util
import os
import re

import pytest
import torch

import gs_dense_ref as D
import mesh_deform_ref as DF
import mesh_render_ref as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEFORM_ENTRIES = {"v3d_recon_mesh_aa_alpha", "v3d_recon_mesh_aa_count", "v3d_recon_mesh_aa_emit", "v3d_recon_mesh_aa_reduce",
                  "v3d_recon_mesh_project_bwd", "v3d_recon_mesh_smooth_grad"}


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
    assert DEFORM_ENTRIES <= declared and DEFORM_ENTRIES <= set(geometry.SIGNATURES)
    for name in DEFORM_ENTRIES:
        assert hasattr(lib, name), f"{name} is not exported"
        proto = re.search(r"\bint " + name + r"\s*\(([^;]*)\);", hdr).group(1)
        assert len(proto.split(",")) == len(geometry.SIGNATURES[name][1]), f"{name}: the ctypes row and the prototype differ in length"
    assert lib.v3d_recon_abi_version() == geometry.ABI_VERSION == 1          # the new entries are additive
    src = open(os.path.join(ROOT, "v3d_amd", "csrc_recon", "meshdeform.hip")).read()
    assert "atomic" not in src.replace("No atomics", "")                      # no atomics of any kind, floating point or other


def test_bad_arguments_are_refused_before_any_launch(lib):
    # (no GPU here: an entry that reached its launch would fail differently, or crash; `p` is never dereferenced by the host code)
    p = 0x1000
    err = lambda: lib.v3d_recon_last_error().decode()  # noqa: E731

    def calls(fn, order, **defaults):
        return lambda **kw: fn(*[kw.get(k, defaults[k]) for k in order])

    from v3d_amd.recon.rasterize import gs_camera
    gc = gs_camera(D.cams_for(32, 32)[0], [0.0, 0.0, 0.0])
    view = ("face_id", "faces", "F", "pix_f", "pix_q", "V", "W", "H")
    base = dict(face_id=p, faces=p, F=4, pix_f=p, pix_q=p, V=8, W=32, H=32, stream=None)
    aa = calls(lib.v3d_recon_mesh_aa_alpha, view + ("alpha", "raw", "stream"), alpha=p, raw=p, **base)
    for k in ("face_id", "faces", "pix_f", "pix_q", "alpha", "raw"):
        assert aa(**{k: None}) == -1 and "v3d_recon_mesh_aa_alpha" in err() and "null" in err(), k
    assert aa(F=0) == -1 and "positive" in err()
    assert aa(V=-1) == -1 and "positive" in err()
    assert aa(W=4097) == -1 and "4097" in err() and "4096" in err()
    assert aa(H=0) == -1 and "4096" in err()
    cnt = calls(lib.v3d_recon_mesh_aa_count, view + ("counts", "info", "stream"), counts=p, info=None, **base)
    for k in ("face_id", "faces", "pix_f", "pix_q", "counts"):
        assert cnt(**{k: None}) == -1 and "v3d_recon_mesh_aa_count" in err() and "null" in err(), k
    assert cnt(F=0) == -1 and "positive" in err()
    assert cnt(V=0) == -1 and "positive" in err()
    assert cnt(W=0) == -1 and "4096" in err()
    em = calls(lib.v3d_recon_mesh_aa_emit, view + ("raw", "dL", "offsets", "n", "keys", "vals", "payload", "stream"), raw=p, dL=p, offsets=p, n=6,
               keys=p, vals=p, payload=p, **base)
    for k in ("face_id", "faces", "pix_f", "pix_q", "raw", "dL", "offsets", "keys", "vals", "payload"):
        assert em(**{k: None}) == -1 and "v3d_recon_mesh_aa_emit" in err() and "null" in err(), k
    assert em(n=0) == -1 and "num_records 0" in err()
    assert em(n=7) == -1 and "multiple of 2" in err()
    assert em(n=8 * 32 * 32 + 2) == -1 and "num_records" in err()
    assert em(F=0) == -1 and "positive" in err()
    assert em(H=5000) == -1 and "5000" in err()
    # reduce (no record at all is legal, with null lists)
    rd = calls(lib.v3d_recon_mesh_aa_reduce, ("ranges", "vals", "payload", "n", "V", "out", "stream"), ranges=p, vals=p, payload=p, n=6, V=8, out=p,
               stream=None)
    for k in ("ranges", "vals", "payload", "out"):
        assert rd(**{k: None}) == -1 and "v3d_recon_mesh_aa_reduce" in err() and "null" in err(), k
    assert rd(n=-2) == -1 and "negative" in err()
    assert rd(V=0) == -1 and "positive" in err()
    pb = calls(lib.v3d_recon_mesh_project_bwd, ("verts", "V", "cam", "pix_q", "dL", "out", "stream"), verts=p, V=8, cam=C.byref(gc), pix_q=p, dL=p, out=p,
               stream=None)
    for k in ("verts", "cam", "pix_q", "dL", "out"):
        assert pb(**{k: None}) == -1 and "v3d_recon_mesh_project_bwd" in err() and "null" in err(), k
    assert pb(V=0) == -1 and "positive" in err()
    gc.width = 5000
    assert pb() == -1 and "5000" in err()
    sg = calls(lib.v3d_recon_mesh_smooth_grad, ("d", "V", "faces", "F", "ranges", "corners", "scale", "grad", "stream"), d=p, V=8, faces=p, F=4, ranges=p,
               corners=p, scale=0.5, grad=p, stream=None)
    for k in ("d", "faces", "ranges", "corners", "grad"):
        assert sg(**{k: None}) == -1 and "v3d_recon_mesh_smooth_grad" in err() and "null" in err(), k
    assert sg(V=0) == -1 and "positive" in err()
    assert sg(F=0) == -1 and "positive" in err()
    assert sg(F=2 ** 31 - 1) == -1 and "INT32_MAX" in err()


def _entry(name):
    spec = importlib.util.spec_from_file_location("v3d_entry_" + name, os.path.join(ROOT, "scripts", "pub", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_script_options_parse_with_the_references_defaults():
    from v3d_amd.recon import mesh_deform as MD
    mod = _entry("fit_mesh")
    ap = mod.build_parser()
    a = vars(ap.parse_args(["--mesh", "out/gs/mesh_50k.ply", "--gaussians", "out/gs/point_cloud/iteration_4000/point_cloud.ply", "-o",
                            "out/gs/mesh_50k_fit.ply", "-w"]))
    assert a == {"mesh": "out/gs/mesh_50k.ply", "gaussians": "out/gs/point_cloud/iteration_4000/point_cloud.ply", "out": "out/gs/mesh_50k_fit.ply",
                 "white_background": True, "iters": 2048, "lr": 1e-4, "lambda_offset": 0.1, "lambda_smooth": 10.0, "views": 36, "num_opt": 0,
                 "reso": 512, "seed": 0, "video": None, "num_frames": None, "radius": 2.0, "elevation": 0.0, "fov": 60.0, "render_orbit": 0}
    assert (a["iters"], a["lr"], a["lambda_offset"], a["lambda_smooth"]) == (MD.ITERATIONS, MD.LR, MD.LAMBDA_OFFSET, MD.LAMBDA_SMOOTH)
    assert (MD.LAMBDA_OFFSET, MD.LAMBDA_SMOOTH) == (DF.LAMBDA_OFFSET, DF.LAMBDA_SMOOTH)
    recon = vars(_entry("recon_from_vid").build_parser().parse_args(["--video", "x.npy"]))
    for k in ("radius", "elevation", "fov", "seed", "num_frames", "white_background"):
        assert vars(ap.parse_args(["--mesh", "m.ply", "--gaussians", "g.ply"]))[k] == recon[k], k
    with pytest.raises(SystemExit):
        ap.parse_args(["--gaussians", "g.ply"])          # --mesh is required
    with pytest.raises(SystemExit):
        ap.parse_args(["--mesh", "m.ply"])               # --gaussians is required
    for bad in (["--iters", "-1"], ["--views", "0"], ["--reso", "5000"], ["--lambda_smooth", "-1"]):
        with pytest.raises(SystemExit):
            mod.main(["--mesh", "does/not/exist.ply", "--gaussians", "does/not/exist.ply"] + bad)


def test_host_api_refuses_what_does_not_fit_and_returns_the_empty_mesh():
    from v3d_amd.recon import mesh_deform as MD
    cams = D.cams_for(32, 32)
    v, f = M.icosphere(0)
    with pytest.raises(ValueError, match="alphas for 4 cameras"):
        MD.fit_vertices(v, f, cams, torch.zeros(3, 32, 32), device="cpu")
    with pytest.raises(ValueError, match="does not match"):
        MD.fit_vertices(v, f, cams, torch.zeros(4, 32, 40), device="cpu")
    with pytest.raises(ValueError, match="must not be negative"):
        MD.fit_vertices(v, f, cams, torch.zeros(4, 32, 32), iterations=-1, device="cpu")
    with pytest.raises(ValueError, match="must not be negative"):
        MD.fit_vertices(v, f, cams, torch.zeros(4, 32, 32), lambda_smooth=-1.0, device="cpu")
    with pytest.raises(ValueError, match="must not be negative"):
        MD.fit_vertices(v, f, cams, torch.zeros(4, 32, 32), num_opt=-2, device="cpu")
    with pytest.raises(ValueError, match="outside the vertex array"):
        MD.fit_vertices(v, f + 1, cams, torch.zeros(4, 32, 32), device="cpu")
    with pytest.raises(ValueError, match="no cameras"):
        MD.fit_vertices(v, f, [], torch.zeros(0, 32, 32), device="cpu")
    with pytest.raises(ValueError, match="float32"):
        MD.antialiased_alpha(cams[0], v.double(), f)
    with pytest.raises(ValueError, match="subpixel_bits"):
        MD.antialiased_alpha(cams[0], v, f, subpixel_bits=9)
    # V = 0 / F = 0: the input, zeros, no launch (so it runs here)
    for vv, ff in ((torch.zeros(0, 3), torch.zeros(0, 3, dtype=torch.int64)), (v, torch.zeros(0, 3, dtype=torch.int64))):
        out, stats = MD.fit_vertices(vv, ff, cams, torch.zeros(4, 32, 32), iterations=5, device="cpu")
        assert torch.equal(out, vv) and stats["loss_first"] is None and stats["vertices_moved"] == 0
        x = vv.clone().requires_grad_(True)
        keep = MD.AlphaView()
        with torch.enable_grad():
            a = MD.antialiased_alpha(cams[0], x, ff, keep=keep)
            (a * torch.rand(32, 32)).sum().backward()
        assert tuple(a.shape) == (32, 32) and not a.any() and not x.grad.any() and keep.pairs == 0 and bool((keep.face_id == -1).all())
    # targets from frames: host torch code
    fr = torch.full((2, 4, 5, 3), 255, dtype=torch.uint8)
    fr[0, 1, 2] = torch.tensor([255, 200, 255], dtype=torch.uint8)
    fr[1, 3, 4] = torch.tensor([250, 250, 250], dtype=torch.uint8)             # within the threshold of white
    a = MD.alpha_from_frames(fr, True, 0.05)
    assert tuple(a.shape) == (2, 4, 5) and a.dtype == torch.float32 and float(a.sum()) == 1.0 and a[0, 1, 2] == 1.0
    assert float(MD.alpha_from_frames(fr.permute(0, 3, 1, 2).float() / 255.0, False, 0.05).mean()) == 1.0
    with pytest.raises(ValueError, match="threshold"):
        MD.alpha_from_frames(fr, True, 1.5)
    d = torch.randn(v.shape[0], 3)
    assert float((MD.smooth_energy_value(d, f) - DF.smooth_energy(d.double(), f)).abs()) < 1e-5


# ---- the restatement's own honesty ------------------------------------------------------------------------------------------------------
def _scene(case, dtype=torch.float64):
    kind, seed, W, H, _, _ = case
    v, f, c = M.mesh_scene(kind, seed)
    cam = M.case_camera(case)
    pj = M.project(v, cam, 8, torch.float32)
    r = M.rasterize(pj["pix_q"], pj["zv"], f, c, W, H, [0.0, 0.0, 0.0], cull=True)
    return v, f, cam, pj, r["face_id"]


@pytest.mark.parametrize("case", DF.DEFORM_CASES, ids=M.case_id)
def test_scenes_keep_their_decision_margins(case):
    v, f, cam, pj, fid = _scene(case)
    res = {}
    for dt in (torch.float64, torch.float32):
        pr = DF.pairs(pj["pix_f"], pj["pix_q"], f, fid, dt)
        res[dt] = (pr,) + DF.alpha_aa(pr, dt)
    pr, a, raw = res[torch.float64]
    has = pr["k"] >= 0
    n = int(pr["pair"].sum())
    t = pr["t"][has]
    recv = torch.cat([raw[has.any(-1) & (raw < 1)], raw[(~pr["covered"]) & (raw > 0)]])          # every pixel that receives something
    err = float((res[torch.float32][1].double() - a).abs().max())
    print(f"{n} pairs; |t - 0.5| >= {float((t - 0.5).abs().min()):.2e}; t_k gap >= {float((pr['second'][has] - t).min()):.2e}; "
          f"|E_k(q)| >= {float(pr['eq_min'][pr['pair']].min()):.2e}; sums in {float(recv.min()):.3f} .. {float(recv.max()):.3f}; float32 {err:.2e}")
    assert 20 <= n <= 116 and torch.equal(pr["pair"], has)                     # pairs, and none without a candidate
    assert float((t - 0.5).abs().min()) >= DF.T_HALF_MARGIN
    assert float((pr["second"][has] - t).min()) >= DF.T_TIE_MARGIN
    assert float(pr["eq_min"][pr["pair"]].min()) >= DF.EQ_MARGIN
    assert float(recv.min()) >= DF.CLAMP_MARGIN and float(recv.max()) <= 1 - DF.CLAMP_MARGIN          # no clamped pixel
    assert not bool((pr["ep"][has] < 0).any())
    assert torch.equal(res[torch.float32][0]["info"], pr["info"])              # the float32 run takes the same decisions on every pair
    assert err <= DF.AA_FP32_ERR
    assert torch.equal((a > 0) | pr["covered"], (a > 0)) and float(a.max()) <= 1 and float(a.min()) >= 0


@pytest.mark.parametrize("case", (DF.DEFORM_CASES[0], DF.DEFORM_CASES[4], DF.DEFORM_CASES[7]), ids=M.case_id)
def test_explicit_backward_is_autograd_of_the_frozen_forward(case):
    v, f, cam, pj, fid = _scene(case)
    V = v.shape[0]
    pr = DF.pairs(pj["pix_f"], pj["pix_q"], f, fid)
    a, raw = DF.alpha_aa(pr)
    dL = torch.randn(fid.shape, generator=torch.Generator().manual_seed(5), dtype=torch.float64)
    assert bool((dL[fid < 0] != 0).all())
    x = pj["pix_f"].double().requires_grad_(True)
    with torch.enable_grad():
        out = DF.alpha_autograd(x, pr)
        (out * dL).sum().backward()
    assert float((out.detach() - a).abs().max()) <= 1e-14
    mine, length = DF.alpha_backward(pr, pj["pix_f"], raw, dL, V)
    assert float((mine - x.grad).abs().max()) <= 1e-10 * float(x.grad.abs().max())
    assert 0 < int((length == 0).sum()) < V and not mine[length == 0].any() and int(length.sum()) == 2 * int((pr["k"] >= 0).sum())
    # through the projection: autograd of mesh_render_ref.project's statements
    vv = v.double().requires_grad_(True)
    with torch.enable_grad():
        pix = DF.project_pix(vv, cam)
        (pix * mine).sum().backward()
    assert torch.equal(pix.detach(), M.project(v, cam, 8)["pix_f"])
    g = DF.project_bwd(v, cam, pj["marked"], mine)
    assert float((g - vv.grad).abs().max()) <= 1e-10 * float(vv.grad.abs().max())
    marked = torch.zeros(V, dtype=torch.bool)
    marked[::7] = True
    gm = DF.project_bwd(v, cam, marked, mine)
    assert not gm[marked].any() and torch.equal(gm[~marked], g[~marked])
    # the 1e-7 is part of the chain: without it the result is off by more than the check above allows
    assert float((DF.project_bwd(v, cam, pj["marked"], mine, eps=0.0) - vv.grad).abs().max()) > 1e-10 * float(vv.grad.abs().max())


def test_smoothness_gradient_is_autograd_of_the_energy():
    v, f, _ = M.mesh_scene("sphere", 1)
    v = torch.cat([v, torch.zeros(1, 3)])                                      # + an isolated vertex
    d = 0.05 * torch.randn(v.shape[0], 3, generator=torch.Generator().manual_seed(3), dtype=torch.float64)
    x = d.clone().requires_grad_(True)
    with torch.enable_grad():
        e = DF.smooth_energy(x, f)
        e.backward()
    g = DF.smooth_grad(d, f)
    assert float(e.detach()) > 0 and float((g - x.grad).abs().max()) <= 1e-10 * float(x.grad.abs().max()) and not g[-1].any()
    assert float(DF.smooth_energy(torch.ones_like(d) * 0.3, f)) == 0.0         # a translation costs nothing: the term does not shrink the mesh


def test_hand_placed_scenes_are_what_they_claim():
    g = lambda name: DF.HAND_SCENES[name]()  # noqa: E731
    both = {}
    for name in DF.HAND_SCENES:
        pix_f, q, faces, fid = g(name)
        assert pix_f.dtype == torch.float32
        pr = {dt: DF.pairs(pix_f, q, faces, fid, dt) for dt in (torch.float64, torch.float32)}
        assert torch.equal(pr[torch.float32]["info"], pr[torch.float64]["info"]), name
        both[name] = (pr[torch.float64],) + DF.alpha_aa(pr[torch.float64]) + (fid,)
    # needle: a column of covered pixels with background left and right; the tip clamps, and its gradient is exactly 0
    pr, a, raw, fid = both["needle"]
    cov = fid >= 0
    assert int(cov.sum()) == 8 and bool(cov[2:10, 5].all()) and bool((raw[cov] < 0.56).all())
    assert float(raw[9, 5]) < -0.1 and float(a[9, 5]) == 0.0 and int((raw < 0).sum()) == 1
    pix_f, q, faces, _ = g("needle")
    dL = torch.ones(fid.shape, dtype=torch.float64)
    keys, payload = DF.records(pr, pix_f, raw, dL)
    idx = torch.nonzero(pr["k"] >= 0)
    tip = (idx[:, 0] == 9).repeat_interleave(2)
    assert int(tip.sum()) == 6 and not payload[tip].any() and bool(payload[~tip].any(1).all())
    assert bool(DF.records(pr, pix_f, raw, dL, keep_clamp_gradient=True)[1][tip].any())          # the fault of the sensitivity list shows here
    # dot: one covered pixel, four background receivers, every sum below 1
    pr, a, raw, fid = both["dot"]
    assert int((fid >= 0).sum()) == 1 and fid[4, 5] == 0 and pr["info"][4, 5].tolist() == [5, 4, 4, 6]
    assert float(raw[4, 5]) == 1.0 and all(0.05 < float(raw[y, x]) < 0.5 for y, x in ((4, 6), (4, 4), (5, 5), (3, 5)))
    # a pair without a candidate contributes nothing
    pr, a, raw, fid = both["no_candidate"]
    assert pr["info"][2, 2].tolist() == [-2, 4, -2, -2] and float(raw[2, 2]) == 1.0 and float(raw[2, 3]) == 0.0 and float(raw[2, 1]) == 0.25
    assert int((pr["k"] >= 0).sum()) == 5
    # E_k(p) < 0: t = 0, the pixel loses 0.5, zero gradient although its sum lies inside (0, 1)
    pr, a, raw, fid = both["negative_ep"]
    assert pr["info"][2, 3].tolist() == [-1, 0, -1, -1] and float(pr["ep"][2, 3, 1]) < -0.3 and float(pr["t"][2, 3, 1]) == 0.0 and float(raw[2, 3]) == 0.5
    pix_f, q, faces, _ = g("negative_ep")
    keys, payload = DF.records(pr, pix_f, raw, torch.ones(fid.shape, dtype=torch.float64))
    assert payload.shape[0] == 2 * int((pr["k"] >= 0).sum()) and not payload.any()
    # t exactly 0.5: the neighbour receives
    pr, a, raw, fid = both["exact_half"]
    assert float(pr["t"][2, 3, 0]) == 0.5 and pr["info"][2, 3, 0] == 6 and float(raw[2, 3]) == 1.0 and float(raw[2, 4]) == 0.0
    # E_k(q) exactly 0 is no candidate
    pr, a, raw, fid = both["on_edge"]
    assert fid[2, 3] == 0 and fid[2, 4] == -1 and float(pr["eq_min"][2, 3, 0]) == 0.0 and pr["info"][2, 3].tolist() == [-2, -1, -1, -1]
    assert float(raw[2, 3]) == 1.0 and float(raw[2, 4]) == 0.0
    # equal t on two edges: the lower k
    pr, a, raw, fid = both["edge_tie"]
    assert float(pr["t"][2, 3, 0]) == 0.25 and float(pr["second"][2, 3, 0]) == 0.25 and pr["info"][2, 3, 0] == 1
    # the sign is the snapped corners'
    pix_f, q, faces, fid = g("sliver")
    c = pix_f.double()
    fa = (c[1, 0] - c[0, 0]) * (c[2, 1] - c[0, 1]) - (c[1, 1] - c[0, 1]) * (c[2, 0] - c[0, 0])
    qa = (q[1, 0] - q[0, 0]) * (q[2, 1] - q[0, 1]) - (q[1, 1] - q[0, 1]) * (q[2, 0] - q[0, 0])
    assert float(fa) < 0 < int(qa) and float(both["sliver"][0]["s"][2, 3]) == 1.0
    assert not torch.equal(DF.pairs(pix_f, q, faces, fid, float_sign=True)["info"], both["sliver"][0]["info"])


@pytest.fixture(scope="module")
def e2e():
    v, f, full = DF.e2e_mesh()
    cams = DF.e2e_cameras()
    return v, f, cams, [DF.view_forward(full, f, cam)["alpha_aa"] for cam in cams]


def test_restatement_fit_reaches_its_recorded_figure(e2e):
    """E2E_MSE_BEFORE / E2E_MSE_AFTER of mesh_deform_ref are what the fp64 restatement reaches on the end-to-end scene of
    tests/test_mesh_deform_gpu.py with the regularisers at their defaults: the GPU test asks the kernels for half of that reduction."""
    v, f, cams, targets = e2e
    r = DF.fit(v, f, cams, targets, DF.E2E["steps"], DF.E2E["lr"], seed=DF.E2E["seed_views"])
    print(f"mse {r['mse_before']:.5f} -> {r['mse_after']:.5f}; IoU {r['iou_before']:.4f} -> {r['iou_after']:.4f}; largest offset {r['max_offset']:.4f}; "
          f"loss {r['loss_first']:.5f} -> {r['loss_last']:.5f}")
    assert abs(r["mse_before"] - DF.E2E_MSE_BEFORE) <= 1e-3 and abs(r["mse_after"] - DF.E2E_MSE_AFTER) <= 1e-4
    assert r["mse_after"] <= 0.1 * r["mse_before"] and r["iou_after"] > r["iou_before"] + 0.1 and 0.05 < r["max_offset"] < 0.2
    again = DF.fit(v, f, cams, targets, DF.E2E["steps"], DF.E2E["lr"], seed=DF.E2E["seed_views"])
    assert torch.equal(again["verts"], r["verts"])
