"""Gaussian-splat reconstruction on the gfx950 kernels (csrc/gs.hip, v3d_amd/recon/): sort / scan / tile ranges against numpy, the exact kNN,
the rasterizer forward and backward against the dense fp64 oracle (tests/gs_dense_ref.py), the fused loss against the reference-generated
fixture, bit-reproducibility, a fit of a known scene and the image -> orbit -> Gaussians pipeline end to end."""
import importlib.util
import os

import numpy as np
import pytest
import torch

import gs_dense_ref as D
from v3d_amd.recon import rasterize as RZ
from v3d_amd.recon import train as TR
from v3d_amd.recon.cameras import orbit_cameras
from v3d_amd.recon.gaussians import read_ply

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(autouse=True)
def _grad_enabled():
    # (other modules of the suite switch autograd off process-wide; these tests differentiate)
    with torch.enable_grad():
        yield
DEV = "cuda"
SCENE_SEEDS = D.SCENE_SEEDS       # (their threshold margins are checked on the CPU: tests/test_gs_cpu.py)
cams_for = D.cams_for


def to_dev(scene, grad=False):
    return [t.to(DEV).requires_grad_(grad) for t in scene]


@pytest.mark.parametrize("nbits", [10, 12, 42])
def test_radix_sort_pairs_is_a_stable_sort(hip_ops, nbits):
    rng = np.random.default_rng(nbits)
    n = 100_003
    pool = rng.integers(0, 1 << nbits, size=max(4, n // 16), dtype=np.int64)
    keys = pool[rng.integers(0, pool.size, size=n)]          # many ties
    vals = np.arange(n, dtype=np.int32)
    ks, vs = hip_ops.gs_radix_sort_pairs(torch.from_numpy(keys).to(DEV), torch.from_numpy(vals).to(DEV), nbits)
    order = np.argsort(keys, kind="stable")
    np.testing.assert_array_equal(ks.cpu().numpy(), keys[order])
    np.testing.assert_array_equal(vs.cpu().numpy(), vals[order])


@pytest.mark.parametrize("n", [1, 7, 4096, 50_001])
def test_scan(hip_ops, n):
    x = np.random.default_rng(n).integers(0, 20, size=n).astype(np.int32)
    out = hip_ops.gs_scan(torch.from_numpy(x).to(DEV)).cpu().numpy()
    np.testing.assert_array_equal(out, np.concatenate([[0], np.cumsum(x)]).astype(np.int32))


def test_duplicate_keys_and_tile_ranges(hip_ops):
    xyz, s, r, o, f = to_dev(D.random_scene(300, SCENE_SEEDS[0]))
    cam = cams_for(80, 80)[1]
    _, st = RZ.forward_pass(hip_ops, xyz, s, r, o, f.view(-1, 3).contiguous(), RZ.gs_camera(cam, [0, 0, 0]))
    offs = st["offsets"].cpu().numpy()
    tiles = st["tiles"].cpu().numpy()
    assert offs[-1] == tiles.sum() == st["n_inst"] > 0
    keys, vals = hip_ops.gs_duplicate_keys(st["means2d"], st["radii"], st["depth"], st["offsets"], st["n_inst"], 80, 80)
    keys, vals = keys.cpu().numpy(), vals.cpu().numpy()
    np.testing.assert_array_equal(vals, np.repeat(np.arange(300), tiles))
    order = np.argsort(keys, kind="stable")
    np.testing.assert_array_equal(st["vals_s"].cpu().numpy(), vals[order])
    # inst_pos is the inverse of the sort permutation
    inst_pos = st["inst_pos"].cpu().numpy()
    np.testing.assert_array_equal(order[inst_pos], np.arange(keys.size))
    ranges = st["ranges"].cpu().numpy()
    tile_s = keys[order] >> 32
    for t in range(ranges.shape[0]):
        idx = np.nonzero(tile_s == t)[0]
        exp = (idx[0], idx[-1] + 1) if idx.size else (0, 0)
        assert tuple(ranges[t]) == exp, t


def test_knn3_exact(hip_ops):
    pts = torch.randn(3000, 3, generator=torch.Generator().manual_seed(5)) * 0.3
    got = hip_ops.gs_knn3(pts.to(DEV)).cpu().double()
    p = pts.double()
    d2 = torch.cdist(p, p) ** 2
    d2.fill_diagonal_(float("inf"))
    ref = d2.topk(3, largest=False).values.mean(1)
    torch.testing.assert_close(got, ref, rtol=1e-6, atol=0)


@pytest.mark.parametrize("W,H", D.FORWARD_SIZES)
@pytest.mark.parametrize("seed", SCENE_SEEDS)
def test_render_forward_matches_dense_reference(W, H, seed):
    scene = D.random_scene(300, seed)
    dscene = to_dev(scene)
    for bg in ([0.0, 0.0, 0.0], [1.0, 1.0, 1.0]):
        for cam in cams_for(W, H):
            img, radii = RZ.rasterize(*dscene, cam, bg)
            ref, pr = D.render(*scene, cam.world_view, cam.full_proj, cam.tanfovx, cam.tanfovy, W, H, bg)
            err = (img.double().cpu() - ref).abs().max().item()
            assert err <= 1e-4, (seed, W, H, bg, err)
            vis = pr["visible"]
            np.testing.assert_array_equal(radii.cpu().numpy()[vis.numpy()], pr["radius"][vis].numpy().astype(np.int32))
            assert (radii.cpu()[~vis] == 0).all()


def _rel(a, b):
    return ((a.double() - b.double()).norm() / b.double().norm().clamp_min(1e-30)).item()


@pytest.mark.parametrize("W,H,seed,cam_i,white", [(64, 48, SCENE_SEEDS[0], 0, True), (64, 48, SCENE_SEEDS[1], 2, False),
                                                 (80, 80, SCENE_SEEDS[2], 1, True)])
def test_render_backward_matches_autograd(W, H, seed, cam_i, white):
    scene = D.random_scene(300, seed)
    cam = cams_for(W, H)[cam_i]
    bg = [1.0, 1.0, 1.0] if white else [0.0, 0.0, 0.0]
    wgt = torch.randn(3, H, W, generator=torch.Generator().manual_seed(seed + 1), dtype=torch.float64)
    dscene = to_dev(scene, grad=True)
    holder = torch.zeros(300, 2, device=DEV, requires_grad=True)
    img, _ = RZ.rasterize(*dscene, cam, bg, holder)
    (img * wgt.float().to(DEV)).sum().backward()
    cscene = [t.double().requires_grad_(True) for t in scene]
    ref, pr = D.render(*cscene, cam.world_view, cam.full_proj, cam.tanfovx, cam.tanfovy, W, H, bg)
    pr["pix"].retain_grad()
    (ref * wgt).sum().backward()
    for name, g, r in zip(("xyz", "scale", "rot", "opacity", "f_dc"), dscene, cscene):
        assert _rel(g.grad.cpu(), r.grad) <= 1e-3, (name, _rel(g.grad.cpu(), r.grad))
    # screen-space mean gradient = dL/d(NDC mean) = dL/d(pixel mean) * (W/2, H/2)
    ref_m2 = pr["pix"].grad * torch.tensor([W / 2, H / 2], dtype=torch.float64)
    assert _rel(holder.grad.cpu(), ref_m2) <= 1e-3


@pytest.fixture(scope="module")
def gs_golden():
    return torch.load(os.path.join(ROOT, "tests", "golden", "v3d_gs.pt"))


def test_fused_ssim_l1_matches_fixture_and_restatement(hip_ops, gs_golden):
    for case in gs_golden["ssim"]:
        a, b = case["img1"], case["img2"]
        out3, work = hip_ops.gs_ssim_l1_fwd(a.to(DEV), b.to(DEV), 1.0)
        assert abs(out3[1].item() - case["value"].item()) <= 1e-6
        grad = hip_ops.gs_ssim_l1_bwd(a.to(DEV), b.to(DEV), 1.0, work, torch.ones(1, device=DEV))
        assert _rel(-grad.cpu(), case["grad"]) <= 1e-4
        lam = 0.2
        ad = a.double().requires_grad_(True)
        loss = (1 - lam) * (ad - b.double()).abs().mean() + lam * (1 - D.ssim(ad, b.double()))
        loss.backward()
        out3, work = hip_ops.gs_ssim_l1_fwd(a.to(DEV), b.to(DEV), lam)
        assert abs(out3[0].item() - loss.item()) <= 1e-6
        grad = hip_ops.gs_ssim_l1_bwd(a.to(DEV), b.to(DEV), lam, work, torch.full((1,), 2.0, device=DEV))
        assert _rel(grad.cpu(), 2.0 * ad.grad) <= 1e-4


def test_forward_and_gradients_are_bit_identical():
    scene = D.random_scene(300, SCENE_SEEDS[1])
    cam = cams_for(80, 80)[3]
    wgt = torch.randn(3, 80, 80, generator=torch.Generator().manual_seed(3)).to(DEV)
    outs = []
    for _ in range(3):
        dscene = to_dev(scene, grad=True)
        holder = torch.zeros(300, 2, device=DEV, requires_grad=True)
        img, _ = RZ.rasterize(*dscene, cam, [1, 1, 1], holder)
        (img * wgt).sum().backward()
        outs.append([img.detach().cpu()] + [t.grad.cpu() for t in dscene] + [holder.grad.cpu()])
    for o in outs[1:]:
        for a, b in zip(outs[0], o):
            assert torch.equal(a, b)


def _target_frames(n_gauss, seed, n_views, reso, white=True):
    """uint8 orbit frames of a seeded scene, rendered by the HIP forward (pinned by the forward test above)."""
    xyz, s, r, o, f = D.random_scene(n_gauss, seed, spread=0.3)
    scene = to_dev([xyz, s, r, o, f])
    cams, _ = orbit_cameras(n_views, 2.0, 0.0, 60.0, reso)
    bg = [1.0, 1.0, 1.0] if white else [0.0, 0.0, 0.0]
    with torch.no_grad():
        imgs = [RZ.rasterize(*scene, c, bg)[0] for c in cams]
    return torch.stack([(i.clamp(0, 1) * 255).round().to(torch.uint8).permute(1, 2, 0) for i in imgs])


def _small_opt(iterations):
    return TR.OptimizationParams(densify_from_iter=50, densification_interval=25, opacity_reset_interval=100, densify_until_iter=iterations)


def test_training_run_is_bit_reproducible(tmp_path):
    frames = _target_frames(500, 7, 6, 64)
    runs = []
    for k in range(2):
        opt = _small_opt(150)
        g, _, st = TR.reconstruct(frames, model_path=str(tmp_path / f"r{k}"), iterations=150, save_iterations=[150], lambda_dssim=0.2,
                                  num_pts=2000, white_background=True, seed=3, opt=opt)
        runs.append((g, st))
    (g0, s0), (g1, s1) = runs
    assert s0["num_gaussians"] == s1["num_gaussians"]
    assert s0["num_gaussians"] != 2000        # densification and pruning ran
    for name, p in g0.params().items():
        assert torch.equal(p.detach().cpu(), g1.params()[name].detach().cpu()), name
    ply = "point_cloud/iteration_150/point_cloud.ply"
    assert open(tmp_path / "r0" / ply, "rb").read() == open(tmp_path / "r1" / ply, "rb").read()


# Fit bar: the first MI355X run measured 22.89 dB mean training-view PSNR after 600 iterations (2537 Gaussians); the bar keeps ~3 dB margin.
FIT_BAR_DB = 20.0


def test_fit_known_scene():
    frames = _target_frames(2000, 11, 18, 128)
    opt = TR.OptimizationParams(densify_from_iter=100, densification_interval=50, densify_until_iter=500, opacity_reset_interval=3000)
    g, cams, st = TR.reconstruct(frames, iterations=600, lambda_dssim=0.2, num_pts=5000, white_background=True, seed=0, opt=opt)
    gt = frames.permute(0, 3, 1, 2).float() / 255.0
    bg = torch.ones(3, device=DEV)
    with torch.no_grad():
        ps = [TR.psnr(RZ.render(c, g, bg)["render"].clamp(0, 1), gt[i]) for i, c in enumerate(cams)]
    mean = float(np.mean(ps))
    print(f"[fit] mean training-view PSNR {mean:.2f} dB, {st['num_gaussians']} Gaussians, {st['seconds']:.1f} s")
    assert mean >= FIT_BAR_DB


def test_image_to_orbit_to_gaussians_end_to_end(tmp_path):
    spec = importlib.util.spec_from_file_location("v3d_entry", os.path.join(ROOT, "scripts", "pub", "V3D_512.py"))
    entry = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(entry)
    _, model = entry.sample_one(synthetic=True, num_frames=6, num_steps=2, model_channels=64, vae_ch=32, height=128, width=128)
    frames = model.last_frames_u8
    assert frames.is_cuda and tuple(frames.shape) == (6, 128, 128, 3)
    g, _, st = TR.reconstruct(frames, model_path=str(tmp_path), iterations=50, save_iterations=[50], lambda_dssim=1.0, num_pts=3000,
                              white_background=True, seed=0)
    names, data = read_ply(str(tmp_path / "point_cloud" / "iteration_50" / "point_cloud.ply"))
    assert names == ["x", "y", "z", "nx", "ny", "nz", "f_dc_0", "f_dc_1", "f_dc_2", "opacity", "scale_0", "scale_1", "scale_2",
                     "rot_0", "rot_1", "rot_2", "rot_3"]
    assert data.shape == (st["num_gaussians"], 17) and np.isfinite(data).all()
