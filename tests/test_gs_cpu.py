"""Gaussian-splat reconstruction without a GPU: orbit cameras and the xyz learning-rate schedule against the reference-generated fixture
(tests/golden/v3d_gs.pt), the dense rasterizer oracle (tests/gs_dense_ref.py) against the fixture's SSIM and a closed-form splat, option
checks, frame loaders, PLY I/O and densification bookkeeping (v3d_amd/recon/gaussians.py on CPU)."""
import importlib.util
import math
import os

import numpy as np
import pytest
import torch

import gs_dense_ref as D
from v3d_amd.recon import gaussians as GM
from v3d_amd.recon import train as TR
from v3d_amd.recon.cameras import orbit_cameras

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(autouse=True)
def _grad_enabled():
    # (other modules of the suite switch autograd off process-wide; these tests differentiate)
    with torch.enable_grad():
        yield


@pytest.fixture(scope="module")
def gs_golden():
    return torch.load(os.path.join(ROOT, "tests", "golden", "v3d_gs.pt"))


def _entry():
    spec = importlib.util.spec_from_file_location("v3d_recon_entry", os.path.join(ROOT, "scripts", "pub", "recon_from_vid.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def test_orbit_cameras_match_reference(gs_golden):
    for c in gs_golden["cameras"]:
        cams, extent = orbit_cameras(c["T"], c["radius"], c["elevation"], c["fov"])
        assert len(cams) == c["T"]
        torch.testing.assert_close(torch.stack([k.world_view for k in cams]), c["world_view"], rtol=0, atol=1e-6)
        torch.testing.assert_close(torch.stack([k.full_proj for k in cams]), c["full_proj"], rtol=0, atol=1e-6)
        torch.testing.assert_close(torch.stack([k.center for k in cams]), c["center"], rtol=0, atol=1e-6)
        assert abs(extent - c["extent"]) <= 1e-6
        assert all(abs(k.fovx - math.radians(c["fov"])) < 1e-12 and k.width == k.height == 512 for k in cams)


def test_xyz_lr_schedule_matches_reference(gs_golden):
    L = gs_golden["lr"]
    f = GM.ExponentialDecay(L["lr_init"], L["lr_final"], L["max_steps"])      # (the reference's xyz schedule has no warm-up steps)
    got = torch.tensor([float(f(s)) for s in L["steps"]], dtype=torch.float64)
    torch.testing.assert_close(got, L["values"], rtol=0, atol=1e-6)
    torch.testing.assert_close(got, L["values"], rtol=1e-9, atol=0)


def test_dense_ssim_matches_reference(gs_golden):
    for case in gs_golden["ssim"]:
        a = case["img1"].clone().requires_grad_(True)
        v = D.ssim(a, case["img2"])
        v.backward()
        assert abs(v.item() - case["value"].item()) <= 1e-6
        torch.testing.assert_close(a.grad, case["grad"], rtol=0, atol=1e-6)


def test_single_isotropic_gaussian_closed_form():
    # one isotropic Gaussian on the optical axis of a camera at distance 2 facing it: its screen footprint is an isotropic 2-D Gaussian of
    # variance (f s / z)^2 + 0.3 centred on the principal point ((W - 1) / 2, (H - 1) / 2)
    W = H = 64
    cams, _ = orbit_cameras(1, 2.0, 0.0, 60.0, reso=W)
    cam = cams[0]
    s, op, dc = 0.05, 0.6, 0.4
    xyz = torch.zeros(1, 3)
    params = (xyz, torch.full((1, 3), math.log(s)), torch.tensor([[1.0, 0, 0, 0]]), torch.logit(torch.tensor([[op]])), torch.full((1, 1, 3), dc))
    bg = [0.2, 0.3, 0.4]
    img, pr = D.render(*params, cam.world_view, cam.full_proj, cam.tanfovx, cam.tanfovy, W, H, bg)
    f = W / (2 * math.tan(math.radians(30)))
    var = (f * s / 2.0) ** 2 + 0.3
    ys, xs = torch.meshgrid(torch.arange(H, dtype=torch.float64), torch.arange(W, dtype=torch.float64), indexing="ij")
    c = (W - 1) / 2
    alpha = op * torch.exp(-((xs - c) ** 2 + (ys - c) ** 2) / (2 * var))
    r = math.ceil(3 * math.sqrt(var))
    inside = ((xs // 16) >= int((c - r) / 16)) & ((xs // 16) < int((c + r + 15) / 16)) & ((ys // 16) >= int((c - r) / 16)) & ((ys // 16) < int((c + r + 15) / 16))
    alpha = torch.where((alpha >= 1 / 255) & inside, alpha, torch.zeros_like(alpha))
    col = 0.5 + D.SH_C0 * dc
    for ch in range(3):
        exp = alpha * col + (1 - alpha) * bg[ch]
        torch.testing.assert_close(img[ch], exp, rtol=0, atol=1e-6)      # (fp32 camera matrices)
    assert int(pr["radius"][0]) == r


def test_options_refused():
    with pytest.raises(NotImplementedError, match="--lambda_lpips 0"):
        TR.check_options(0, 2.0)
    with pytest.raises(NotImplementedError, match="SH degree 0"):
        TR.check_options(3, 0.0)
    with pytest.raises(NotImplementedError):
        GM.GaussianModel(1)
    with pytest.raises(ValueError, match="square"):
        TR.frames_to_images(np.zeros((4, 48, 64, 3), np.uint8), "cpu")
    with pytest.raises(SystemExit):
        _entry().main(["--video", "x.npy", "--lambda_lpips", "2.0"])
    with pytest.raises(SystemExit):
        _entry().main(["--video", "x.npy", "--sh_degree", "3"])


def test_npy_and_png_folder_loaders_agree(tmp_path):
    from PIL import Image
    frames = np.random.default_rng(0).integers(0, 256, size=(5, 32, 32, 3), dtype=np.uint8)
    np.save(tmp_path / "v.npy", frames)
    (tmp_path / "png").mkdir()
    for i, f in enumerate(frames):
        Image.fromarray(f).save(tmp_path / "png" / f"{i:03d}.png")
    e = _entry()
    a, b = e.load_video(str(tmp_path / "v.npy")), e.load_video(str(tmp_path / "png"))
    np.testing.assert_array_equal(a, frames)
    np.testing.assert_array_equal(b, frames)
    imgs = TR.frames_to_images(a, "cpu")
    assert imgs.shape == (5, 3, 32, 32) and imgs.dtype == torch.float32 and float(imgs.max()) <= 1.0


def _model(n=6):
    g = GM.GaussianModel(0)
    gen = torch.Generator().manual_seed(0)
    g.set_params(torch.randn(n, 3, generator=gen), torch.randn(n, 3, generator=gen), torch.log(torch.full((n, 3), 0.05)),
                 torch.tensor([[1.0, 0, 0, 0]]).repeat(n, 1), torch.logit(torch.full((n, 1), 0.5)))
    return g


def test_ply_round_trip_and_reference_attributes(tmp_path):
    g = _model()
    names = g.attribute_names()
    assert names == ["x", "y", "z", "nx", "ny", "nz", "f_dc_0", "f_dc_1", "f_dc_2", "opacity", "scale_0", "scale_1", "scale_2",
                     "rot_0", "rot_1", "rot_2", "rot_3"]
    p = str(tmp_path / "point_cloud" / "iteration_7" / "point_cloud.ply")
    g.save_ply(p)
    raw = open(p, "rb").read()
    head = raw[:raw.index(b"end_header\n") + 11].decode()
    assert head.startswith("ply\nformat binary_little_endian 1.0\nelement vertex 6\nproperty float x\n")
    assert len(raw) - len(head) == 6 * 17 * 4
    h = GM.GaussianModel(0)
    h.load_ply(p)
    for k in ("xyz", "f_dc", "scaling", "rotation", "opacity"):
        assert torch.equal(g.params()[k].detach(), h.params()[k].detach()), k


def test_densify_clone_split_prune_bookkeeping():
    g = _model(6)
    opt = TR.OptimizationParams(percent_dense=0.01)
    g.spatial_lr_scale = 1.0
    g.training_setup(opt, seed=0)
    extent = 2.0                        # clone / split boundary: max scale 0.02
    with torch.no_grad():
        g.scaling[:] = torch.log(torch.tensor([[0.01] * 3, [0.01] * 3, [0.05] * 3, [0.05] * 3, [0.01] * 3, [0.05] * 3]))
        g.opacity[:] = torch.logit(torch.tensor([[0.5], [0.5], [0.5], [0.5], [0.001], [0.5]]))
    # give every row distinct Adam moments, so the carried-over rows can be identified
    for k, p in enumerate(g.optimizer.param_groups):
        par = p["params"][0]
        g.optimizer.state[par] = {"step": torch.tensor(3.0), "exp_avg": torch.arange(par.numel(), dtype=torch.float32).view(par.shape) + 100 * k,
                                  "exp_avg_sq": torch.ones_like(par) * (k + 1)}
    xyz0, sc0 = g.xyz.detach().clone(), g.scaling.detach().clone()
    ea0 = g.optimizer.state[g.xyz]["exp_avg"].clone()
    # gradient statistics: rows 0 (small) and 2 (large) exceed the threshold; 1, 3 do not; 4 is transparent; 5 large but quiet
    g.xyz_gradient_accum[:] = torch.tensor([[0.001], [0.0], [0.001], [0.0], [0.0], [0.00001]])
    g.denom[:] = 1.0
    g.densify_and_prune(0.0002, 0.005, extent, None)
    # survivors: originals 0, 1, 3, 5 (2 was split and removed, 4 pruned by opacity), then the clone of 0, then 2 split pieces of 2
    assert g.xyz.shape[0] == 4 + 1 + 2
    torch.testing.assert_close(g.xyz[:4].detach(), xyz0[[0, 1, 3, 5]])
    torch.testing.assert_close(g.xyz[4].detach(), xyz0[0])
    torch.testing.assert_close(g.get_scaling[5:].detach(), torch.exp(sc0[2]).repeat(2, 1) / (0.8 * 2))
    st = g.optimizer.state[g.xyz]
    torch.testing.assert_close(st["exp_avg"][:4], ea0[[0, 1, 3, 5]])
    assert torch.equal(st["exp_avg"][4:], torch.zeros(3, 3)) and torch.equal(st["exp_avg_sq"][4:], torch.zeros(3, 3))
    for p in g.optimizer.param_groups:
        par = p["params"][0]
        assert par.shape[0] == 7 and g.optimizer.state[par]["exp_avg"].shape == par.shape
        assert par is g.params()[p["name"]]
    assert g.xyz_gradient_accum.shape == (7, 1) and g.max_radii2D.shape == (7,)
    g.reset_opacity()
    assert float(g.get_opacity.max()) <= 0.01 + 1e-7
    assert torch.equal(g.optimizer.state[g.opacity]["exp_avg"], torch.zeros(7, 1))


def test_split_samples_are_seeded():
    runs = []
    for _ in range(2):
        g = _model(6)
        g.spatial_lr_scale = 1.0
        g.training_setup(TR.OptimizationParams(), seed=7)
        g.xyz_gradient_accum[:] = 0.001
        g.denom[:] = 1.0
        _, split = g.densify_and_prune(0.0002, 0.005, 2.0, None)
        assert int(split.sum()) == 6
        runs.append(g.xyz.detach().clone())
    assert runs[0].shape == (12, 3) and torch.equal(runs[0], runs[1])


def test_forward_scenes_keep_their_margin():
    # the GPU forward test holds fp32 to the fp64 oracle at 1e-4: that needs every alpha / transmittance / radius / tile-edge decision of its
    # scenes to fall the same way in both precisions, i.e. far from its threshold compared with fp32 error (~4e-8 on alpha near 1/255)
    for seed in D.SCENE_SEEDS:
        scene = D.random_scene(300, seed)
        for W, H in D.FORWARD_SIZES:
            for cam in D.cams_for(W, H):
                m = D.scene_margin(*scene, cam.world_view, cam.full_proj, cam.tanfovx, cam.tanfovy, W, H)
                assert m >= D.SCENE_MARGIN, (seed, W, H, m)


def test_rasterize_without_gaussians_gives_the_background():
    from v3d_amd.recon.rasterize import rasterize
    cam = D.cams_for(32, 32, n=1)[0]
    params = [torch.zeros(0, k, requires_grad=True) for k in (3, 3, 4, 1)] + [torch.zeros(0, 1, 3, requires_grad=True)]
    img, radii = rasterize(*params, cam, [0.25, 0.5, 1.0])
    assert img.shape == (3, 32, 32) and radii.numel() == 0
    assert torch.equal(img, torch.tensor([0.25, 0.5, 1.0]).view(3, 1, 1).expand(3, 32, 32))
    img.sum().backward()
    assert all(p.grad is not None and p.grad.numel() == 0 for p in params)


def test_screen_size_prune_after_reset_interval():
    g = _model(6)
    g.spatial_lr_scale = 1.0
    g.training_setup(TR.OptimizationParams(), seed=0)
    g.max_radii2D[:] = torch.tensor([5.0, 25.0, 5.0, 5.0, 5.0, 5.0])
    with torch.no_grad():
        g.scaling[3] = math.log(0.5)         # > 0.1 * extent
    g.densify_and_prune(0.0002, 0.005, 2.0, 20)
    # as in the reference, the clone / split steps reset max_radii2D before the screen-size test, so only the world-size rule removes a point
    assert g.xyz.shape[0] == 5
    assert not torch.isclose(g.scaling[:, 0], torch.tensor(math.log(0.5))).any()


# ---- the scenes of tests/test_gs_edges_gpu.py: what follows is the condition for those GPU tests meaning anything ------------------------
EDGE_IDS = [D.case_id(c) for c in D.EDGE_CASES]


@pytest.fixture(scope="module")
def edge_oracles():
    return D.EdgeOracles()


def _view(cam, W, H):
    return cam.world_view, cam.full_proj, cam.tanfovx, cam.tanfovy, W, H


@pytest.mark.parametrize("case", D.EDGE_CASES, ids=EDGE_IDS)
def test_edge_scenes_keep_their_margin(case):
    _, _, W, H, _, _ = case
    scene, cam, _ = D.edge_case(case)
    m = D.scene_margins(*scene, *_view(cam, W, H))
    assert min(v for k, v in m.items() if k != "depth_gap") >= D.SCENE_MARGIN, m
    assert m["depth_gap"] >= D.DEPTH_GAP_MARGIN, m
    assert m["transmittance"] >= D.DEEP_T_MARGIN, m


def test_edge_cases_use_the_listed_seeds_and_ragged_sizes():
    assert {c[1] for c in D.EDGE_CASES if c[0] == "deep"} == set(D.DEEP_SEEDS) and len(set(D.DEEP_SEEDS)) == 3
    assert {c[1] for c in D.EDGE_CASES if c[0] == "cull"} == set(D.CULL_SEEDS)
    for kind in ("deep", "cull", "tie"):
        sizes = {(c[2], c[3]) for c in D.EDGE_CASES if c[0] == kind}
        assert sizes & set(D.FORWARD_SIZES_RAGGED), kind
    assert all(W % 16 and H % 16 for W, H in D.FORWARD_SIZES_RAGGED)
    assert {(c[2], c[3]) for c in D.EDGE_CASES} >= set(D.FORWARD_SIZES_RAGGED)
    assert any(c[2] % 16 == 0 and c[3] % 16 == 0 for c in D.EDGE_CASES)
    assert all(c[2] * c[3] <= 64 * 64 for c in D.EDGE_CASES)


@pytest.mark.parametrize("case", D.EDGE_CASES, ids=EDGE_IDS)
def test_float32_oracle_agrees_with_float64_on_edge_scenes(edge_oracles, case):
    # the GPU bars are 1e-4 on the image and 1e-3 relative L2 on every gradient: the number format itself may cost a quarter of each at most
    c = edge_oracles(case)
    (i64, p64, g64), (i32, p32, g32) = c["o64"], c["o32"]
    assert (i32.double() - i64).abs().max().item() <= 2.5e-5
    for name in D.GRAD_NAMES:
        assert D.rel_l2(g32[name], g64[name]) <= 2.5e-4, name
    # every decision falls the same way in both precisions
    assert torch.equal(p32["visible"], p64["visible"]) and torch.equal(p32["n_contrib"], p64["n_contrib"])
    assert torch.equal(p32["saturated"], p64["saturated"]) and torch.equal(p32["guarded"], p64["guarded"])
    assert torch.equal(p32["radius"][p64["visible"]].double(), p64["radius"][p64["visible"]])
    vis = p64["visible"]
    assert (p32["depth"].double() - p64["depth"])[vis].abs().max().item() <= D.DEPTH_GAP_MARGIN / 4
    # the error the float32 run makes on one Gaussian is the yardstick of the per-Gaussian bound of the GPU test: it must be a number
    for name in ("xyz", "opacity"):
        e, rows = D.per_gaussian_error(g32[name], g64[name])
        assert 0 < e < 2.5e-4 and rows >= 9, (name, e, rows)


def _tiles(W, H):
    return [(ty, tx) for ty in range(0, H, D.TILE) for tx in range(0, W, D.TILE)]


@pytest.mark.parametrize("case", [c for c in D.EDGE_CASES if c[0] == "deep"], ids=[i for i in EDGE_IDS if i.startswith("deep")])
def test_deep_scenes_cover_long_lists_and_saturation(edge_oracles, case):
    _, _, W, H, _, _ = case
    _, pr, g64 = edge_oracles(case)["o64"]
    assert int(pr["list_len"].max()) > 512                      # three forward batches of 256 and more
    assert float(pr["saturated"].float().mean()) >= 0.05
    assert bool((pr["saturated"] & (pr["n_contrib"] > 256)).any())      # a pixel that stops in a later batch than the first
    # a tile whose last contributor lies more than one backward batch (64) before the end of its list: the backward zero-fills the rest
    gaps = [int(pr["list_len"][ty, tx]) - int(pr["n_contrib"][ty:ty + D.TILE, tx:tx + D.TILE].max()) for ty, tx in _tiles(W, H)]
    assert max(gaps) > 64, gaps
    # a tile all of whose pixels have stopped (the block-wide early exit), and one where some pixels go on after others have stopped
    sat = [bool(pr["saturated"][ty:ty + D.TILE, tx:tx + D.TILE].all()) for ty, tx in _tiles(W, H)]
    assert any(sat) and not all(sat)
    # Gaussians hidden behind saturation in every pixel: visible, yet their gradient is exactly zero
    hidden = pr["visible"] & (g64["opacity"].reshape(-1) == 0)
    assert int(hidden.sum()) >= 10


@pytest.mark.parametrize("case", [c for c in D.EDGE_CASES if c[0] == "cull"], ids=[i for i in EDGE_IDS if i.startswith("cull")])
def test_cull_groups_are_what_they_were_built_for(edge_oracles, case):
    _, _, W, H, _, _ = case
    c = edge_oracles(case)
    _, pr, g64 = c["o64"]
    gr, cam = c["groups"], c["cam"]
    assert set(gr) == set(D.CULL_GROUPS) and all(v.numel() > 0 for v in gr.values())
    gx, gy = (W + D.TILE - 1) // D.TILE, (H + D.TILE - 1) // D.TILE
    vis, depth, rect = pr["visible"], pr["depth"], pr["rect"]
    assert (depth[gr["behind"]] < 0).all() and not vis[gr["behind"]].any()
    assert ((depth[gr["near"]] > 0) & (depth[gr["near"]] < 0.2)).all() and not vis[gr["near"]].any()
    far = gr["far_out"]
    assert (depth[far] > 0.2).all() and not vis[far].any()
    assert (((rect[far, 2] - rect[far, 0]) * (rect[far, 3] - rect[far, 1])) == 0).all()
    gd = gr["guard"]
    outside = (pr["txtz"][gd].abs() > cam.tanfovx) | (pr["tytz"][gd].abs() > cam.tanfovy)
    assert vis[gd].all() and pr["guarded"][gd].all() and outside.all()
    assert (pr["txtz"][gd].abs() > 1.3 * cam.tanfovx).any() and (pr["tytz"][gd].abs() > 1.3 * cam.tanfovy).any()
    assert (g64["xyz"][gd].norm(dim=1) > 0).all()           # each reaches the image and takes a gradient through the clamped Jacobian
    assert not pr["guarded"][gr["huge"]].any() and not pr["guarded"][gr["dark"]].any()
    hg = gr["huge"]
    assert vis[hg].all() and (rect[hg] == torch.tensor([0, 0, gx, gy], dtype=rect.dtype)).all()
    full = torch.stack([(pr["pix"][hg, 0] - pr["radius"][hg]) / D.TILE, (pr["pix"][hg, 1] - pr["radius"][hg]) / D.TILE], 1)
    over = torch.stack([(pr["pix"][hg, 0] + pr["radius"][hg]) / D.TILE - gx, (pr["pix"][hg, 1] + pr["radius"][hg]) / D.TILE - gy], 1)
    assert (full < 0).all() and (over > 0).all()              # clamped on all four sides, not just touching
    dk = gr["dark"]
    assert vis[dk].all() and (pr["rgb_raw"][dk] < 0).all() and (pr["rgb"][dk] == 0).all()
    assert (g64["f_dc"][dk] == 0).all() and (g64["opacity"][dk].reshape(-1) != 0).all()
    for name in D.GRAD_NAMES:       # culled: exactly zero everywhere
        for k in ("behind", "near", "far_out"):
            assert (g64[name][gr[k]] == 0).all(), (name, k)


@pytest.mark.parametrize("case", [c for c in D.EDGE_CASES if c[2] % 16 or c[3] % 16], ids=[i for c, i in zip(D.EDGE_CASES, EDGE_IDS) if c[2] % 16 or c[3] % 16])
def test_ragged_sizes_have_lit_pixels_in_partial_tiles(edge_oracles, case):
    _, _, W, H, _, _ = case
    _, pr, _ = edge_oracles(case)["o64"]
    lit = pr["n_contrib"] > 0
    if W % 16:
        assert bool(lit[:, W - W % 16:].any())
    if H % 16:
        assert bool(lit[H - H % 16:, :].any())


def test_tie_scene_depths_are_equal_and_their_order_matters():
    scene, groups = D.tie_scene()
    for W, H in {(c[2], c[3]) for c in D.EDGE_CASES if c[0] == "tie"}:
        cam = D.axis_camera(W, H)
        wv = cam.world_view
        assert set(wv.flatten().tolist()) <= {0.0, 1.0, -1.0, 2.0} and wv[0, 2] == -1.0 and wv[3, 2] == 2.0      # view z = 2 - x, exactly
        for dt in (torch.float32, torch.float64):
            d = D.project(*scene, *_view(cam, W, H), dt)["depth"]
            for g in groups:
                assert (d[g] == d[g[0]]).all()
            assert len(set(d.tolist())) == len(groups)
        ref, pr = D.render(*scene, *_view(cam, W, H), [1.0, 1.0, 1.0])
        assert pr["visible"].all()
        for g in groups:      # the same Gaussians in another index order: a different image, by far more than the forward bar of 1e-4
            for a, b in ((0, 1), (1, 2), (0, 2)):
                swapped, _ = D.render(*D.swap_rows(scene, int(g[a]), int(g[b])), *_view(cam, W, H), [1.0, 1.0, 1.0])
                assert (swapped - ref).abs().max().item() >= 100 * 1e-4, (W, H, g, a, b)
