"""The splat rasterizer and its primitives (csrc/gs.hip) where the parity scenes of tests/test_gs_gpu.py do not reach: tile lists of several
forward batches, saturated pixels and blocks, list tails that reach no pixel, ragged edge tiles, every cull and clamp branch of the preprocess,
a view with every Gaussian culled, equal depths; the radix sort, the scan, the kNN and the fused loss at the edges of their chunking.
Oracles: the dense restatement of tests/gs_dense_ref.py in fp64 (and its float32 run, whose own error scales the per-Gaussian gradient
bound), numpy's stable argsort and cumsum, fp64 pairwise distances, fp64 autograd through D.ssim.  tests/test_gs_cpu.py keeps the scenes honest
(threshold margins, float32 cost, coverage) without a GPU."""
import numpy as np
import pytest
import torch

import gs_dense_ref as D
from conftest import record_parity
from v3d_amd.recon import rasterize as RZ

pytestmark = pytest.mark.gpu
DEV = "cuda"
RS_CHUNK = SCAN_CHUNK = 4096          # keys per radix block, values per scan block (csrc/gs.hip)
BLACK, WHITE = [0.0, 0.0, 0.0], [1.0, 1.0, 1.0]
CASE_IDS = [D.case_id(c) for c in D.EDGE_CASES]


@pytest.fixture(autouse=True)
def _grad_enabled():
    # (other modules of the suite switch autograd off process-wide; these tests differentiate)
    with torch.enable_grad():
        yield


@pytest.fixture(scope="module")
def oracles():
    return D.EdgeOracles()


def to_dev(scene, grad=False):
    return [t.to(DEV).requires_grad_(grad) for t in scene]


def gpu_backward(scene, cam, bg, wgt):
    dscene = to_dev(scene, grad=True)
    holder = torch.zeros(scene[0].shape[0], 2, device=DEV, requires_grad=True)
    img, radii = RZ.rasterize(*dscene, cam, bg, holder)
    (img * wgt.float().to(DEV)).sum().backward()
    grads = {n: t.grad.cpu() for n, t in zip(D.GRAD_NAMES, dscene)}
    grads["means2d"] = holder.grad.cpu()
    return img.detach().cpu(), radii.cpu(), grads


# ---- rasterizer ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", D.EDGE_CASES, ids=CASE_IDS)
def test_forward_matches_dense_reference_on_edge_scenes(hip_ops, oracles, case):
    _, _, W, H, _, _ = case
    c = oracles(case)
    _, pr, _ = c["o64"]
    xyz, s, r, o, f = to_dev(c["scene"])
    vis = pr["visible"].numpy()
    worst = {}
    for bg in (BLACK, WHITE):
        img, st = RZ.forward_pass(hip_ops, xyz, s, r, o, f.view(-1, 3).contiguous(), RZ.gs_camera(c["cam"], bg))
        ref = (pr["color"] + pr["final_T"].reshape(-1, 1) * torch.tensor(bg, dtype=torch.float64)).t().reshape(3, H, W)
        err = (img.double().cpu() - ref).abs().max().item()
        t_err = (st["final_T"].double().cpu() - pr["final_T"]).abs().max().item()
        n_bad = int((st["n_contrib"].cpu() != pr["n_contrib"]).sum())
        worst = {"image_max_abs": max(err, worst.get("image_max_abs", 0.0)), "final_T_max_abs": max(t_err, worst.get("final_T_max_abs", 0.0)),
                 "n_contrib_mismatches": max(n_bad, worst.get("n_contrib_mismatches", 0))}
        print(f"[edges fwd] {D.case_id(case)} bg {bg[0]:.0f}: image {err:.3e} final_T {t_err:.3e} n_contrib mismatches {n_bad}")
        assert err <= 1e-4, (D.case_id(case), bg, err)
        radii = st["radii"].cpu().numpy()
        np.testing.assert_array_equal(radii[vis], pr["radius"][pr["visible"]].numpy().astype(np.int32))
        assert (radii[~vis] == 0).all()
        assert n_bad == 0, (D.case_id(case), bg, n_bad)
        assert t_err <= 1e-6, (D.case_id(case), bg, t_err)
    record_parity(f"gs_edges_forward[{D.case_id(case)}]", worst)


@pytest.mark.parametrize("case", D.EDGE_CASES, ids=CASE_IDS)
def test_backward_matches_autograd_on_edge_scenes(oracles, case):
    c = oracles(case)
    _, _, g64 = c["o64"]
    _, _, g32 = c["o32"]
    _, _, got = gpu_backward(c["scene"], c["cam"], c["bg"], c["wgt"])
    rec = {}
    for name in D.GRAD_NAMES:
        rec[f"rel_l2_{name}"] = D.rel_l2(got[name], g64[name])
        rec[f"rel_l2_{name}_float32_oracle"] = D.rel_l2(g32[name], g64[name])
    for name in ("xyz", "opacity"):
        rec[f"per_gaussian_{name}"], rec[f"per_gaussian_{name}_rows"] = D.per_gaussian_error(got[name], g64[name])
        rec[f"per_gaussian_{name}_float32_oracle"], _ = D.per_gaussian_error(g32[name], g64[name])
    record_parity(f"gs_edges_backward[{D.case_id(case)}]", rec)
    for name in D.GRAD_NAMES:
        assert torch.isfinite(got[name]).all(), name
    for name in D.GRAD_NAMES:
        assert rec[f"rel_l2_{name}"] <= 1e-3, (name, rec[f"rel_l2_{name}"])
    # what the oracle leaves exactly zero (culled Gaussians, Gaussians behind saturation in every pixel, clamped colour channels) is exactly
    # zero here: element by element, so a clamped channel of an otherwise lit Gaussian counts
    for name in D.GRAD_NAMES:
        zero = g64[name].reshape(got[name].shape) == 0
        assert (got[name][zero] == 0).all(), (name, int((got[name][zero] != 0).sum()))
    # a norm over all Gaussians hides a wrong gradient on a few small contributors: every single Gaussian above 1e-3 of the largest is held
    # to 8x what the float32 run of the oracle itself loses on this scene
    for name in ("xyz", "opacity"):
        assert rec[f"per_gaussian_{name}"] <= 8 * rec[f"per_gaussian_{name}_float32_oracle"], (name, rec)


def test_all_gaussians_culled(hip_ops):
    W, H, P = 56, 40, 50
    cam = D.cams_for(W, H)[0]
    g = torch.Generator().manual_seed(4)
    view = torch.cat([torch.rand(P, 2, generator=g, dtype=torch.float64) - 0.5, -0.3 - 2 * torch.rand(P, 1, generator=g, dtype=torch.float64),
                      torch.ones(P, 1, dtype=torch.float64)], 1)
    xyz = (view @ torch.linalg.inv(cam.world_view.double()))[:, :3].float()
    scene = [xyz] + D.random_scene(P, 4)[1:]
    _, pr = D.render(*scene, cam.world_view, cam.full_proj, cam.tanfovx, cam.tanfovy, W, H, BLACK)
    assert float(pr["depth"].max()) < 0 and not pr["visible"].any()
    bg = [0.25, 0.5, 1.0]
    dscene = to_dev(scene, grad=True)
    holder = torch.zeros(P, 2, device=DEV, requires_grad=True)
    img, radii = RZ.rasterize(*dscene, cam, bg, holder)
    assert torch.equal(img.cpu(), torch.tensor(bg).view(3, 1, 1).expand(3, H, W))
    assert radii.shape == (P,) and (radii == 0).all()
    (img * torch.randn(3, H, W, generator=g).to(DEV)).sum().backward()
    for t in dscene + [holder]:
        assert t.grad is not None and t.grad.shape == t.shape and (t.grad == 0).all()
    # nothing is left pending: the next kernel launches, runs and synchronises cleanly
    out = hip_ops.gs_scan(torch.ones(10, dtype=torch.int32, device=DEV))
    torch.cuda.synchronize()
    assert out.cpu().tolist() == list(range(11))


def test_deep_ragged_case_is_bit_identical(oracles):
    case = next(c for c in D.EDGE_CASES if c[0] == "deep" and (c[2] % 16 or c[3] % 16))
    c = oracles(case)
    outs = []
    for _ in range(3):
        img, radii, grads = gpu_backward(c["scene"], c["cam"], c["bg"], c["wgt"])
        outs.append([img, radii] + [grads[n] for n in D.GRAD_NAMES])
    for o in outs[1:]:
        for a, b in zip(outs[0], o):
            assert torch.equal(a, b)


# ---- radix sort -----------------------------------------------------------------------------------------------------------------------------
def _check_sort(hip_ops, keys, nbits):
    """keys uint64 [n]: pairs come back in the stable order of the keys' low nbits, whole keys (the bits above too) travelling with them."""
    n = keys.size
    vals = np.arange(n, dtype=np.int32)[::-1].copy()      # (not the identity: a sort that returns positions instead of values fails)
    ks, vs = hip_ops.gs_radix_sort_pairs(torch.from_numpy(keys.view(np.int64)).to(DEV), torch.from_numpy(vals).to(DEV), nbits)
    masked = keys & np.uint64((1 << nbits) - 1)
    order = np.argsort(masked, kind="stable")
    np.testing.assert_array_equal(ks.cpu().numpy().view(np.uint64), keys[order])
    np.testing.assert_array_equal(vs.cpu().numpy(), vals[order])


def _random_keys(rng, n, nbits):
    """Many ties in the low nbits, random bits above them."""
    pool = rng.integers(0, 1 << 63, size=max(2, n // 8), dtype=np.uint64) * np.uint64(2) + rng.integers(0, 2, size=max(2, n // 8), dtype=np.uint64)
    return pool[rng.integers(0, pool.size, size=n)] if n > 1 else pool[:1].copy()


@pytest.mark.parametrize("n", [1, 255, 256, 257, RS_CHUNK - 1, RS_CHUNK, RS_CHUNK + 1, 300 * RS_CHUNK + 77])
def test_radix_sort_lengths(hip_ops, n):
    _check_sort(hip_ops, _random_keys(np.random.default_rng(n), n, 38), 38)


@pytest.mark.parametrize("nbits", [1, 8, 9, 33, 64])
def test_radix_sort_key_widths(hip_ops, nbits):
    _check_sort(hip_ops, _random_keys(np.random.default_rng(nbits), 3 * RS_CHUNK + 5, nbits), nbits)


@pytest.mark.parametrize("nbits", [1, 9, 33])
def test_radix_sort_ignores_bits_above_nbits(hip_ops, nbits):
    # keys equal in their low nbits and different above: the order of the input is the order of the output (the rasterizer passes
    # 32 + tile bits and relies on nothing above them taking part)
    rng = np.random.default_rng(100 + nbits)
    n = 2 * RS_CHUNK + 3
    low = np.uint64(rng.integers(0, 1 << nbits))
    high = rng.integers(1, 1 << (63 - nbits), size=n, dtype=np.uint64) << np.uint64(nbits)
    _check_sort(hip_ops, high | low, nbits)


@pytest.mark.parametrize("pattern", ["sorted", "reversed", "equal"])
def test_radix_sort_patterns(hip_ops, pattern):
    n = 3 * RS_CHUNK + 5
    keys = np.sort(_random_keys(np.random.default_rng(9), n, 64) >> np.uint64(30))
    keys = {"sorted": keys, "reversed": keys[::-1].copy(), "equal": np.full(n, keys[n // 2])}[pattern]
    _check_sort(hip_ops, keys, 34)


# ---- scan -----------------------------------------------------------------------------------------------------------------------------------
def _check_scan(hip_ops, x):
    out = hip_ops.gs_scan(torch.from_numpy(x).to(DEV)).cpu().numpy()
    exp = np.concatenate([[0], np.cumsum(x.astype(np.int64))])
    assert exp[-1] < 2 ** 31
    np.testing.assert_array_equal(out, exp.astype(np.int32))


# the block sums are scanned by one block in rounds of 256 with a carry: 256 blocks fill one round exactly, one more starts the second
@pytest.mark.parametrize("n", [SCAN_CHUNK - 1, SCAN_CHUNK, SCAN_CHUNK + 1, 256 * SCAN_CHUNK, 256 * SCAN_CHUNK + 1, 700 * SCAN_CHUNK + 13])
def test_scan_lengths(hip_ops, n):
    _check_scan(hip_ops, np.random.default_rng(n % 1000).integers(0, 20, size=n).astype(np.int32))


def test_scan_total_just_below_int32_limit(hip_ops):
    n = 2 * SCAN_CHUNK + 100
    x = np.full(n, (2 ** 31 - 1) // n, dtype=np.int32)
    x[-1] += (2 ** 31 - 1) - int(x.astype(np.int64).sum())
    assert int(x.astype(np.int64).sum()) == 2 ** 31 - 1
    _check_scan(hip_ops, x)


def test_scan_of_zeros(hip_ops):
    _check_scan(hip_ops, np.zeros(SCAN_CHUNK + 9, dtype=np.int32))


# ---- kNN ------------------------------------------------------------------------------------------------------------------------------------
def _knn_ref(pts):
    p = pts.double()
    d2 = ((p[:, None] - p[None]) ** 2).sum(-1)       # differences first: exact to fp64 rounding wherever the cloud sits
    d2.fill_diagonal_(float("inf"))
    return d2.topk(3, largest=False).values.mean(1)


@pytest.mark.parametrize("n", [4, 5, 257])
def test_knn3_small_clouds(hip_ops, n):
    pts = torch.randn(n, 3, generator=torch.Generator().manual_seed(n)) * 0.3
    torch.testing.assert_close(hip_ops.gs_knn3(pts.to(DEV)).cpu().double(), _knn_ref(pts), rtol=1e-6, atol=0)


def test_knn3_cloud_away_from_the_origin(hip_ops):
    # |a|^2 + |b|^2 - 2 a.b would lose these distances (~1e-3) under the rounding of |a|^2 = 300
    pts = torch.randn(1000, 3, generator=torch.Generator().manual_seed(8)) * 0.3 + 10.0
    torch.testing.assert_close(hip_ops.gs_knn3(pts.to(DEV)).cpu().double(), _knn_ref(pts), rtol=1e-6, atol=0)


def test_knn3_duplicate_points(hip_ops):
    g = torch.Generator().manual_seed(12)
    base = torch.randn(400, 3, generator=g) * 0.3
    pts = torch.cat([base, base[:150], base[:40]])[torch.randperm(590, generator=g)]     # pairs and triples of identical points
    ref = _knn_ref(pts)
    p = pts.double()
    d2 = ((p[:, None] - p[None]) ** 2).sum(-1)
    d2.fill_diagonal_(float("inf"))
    assert int((d2.min(1).values == 0).sum()) == 2 * 110 + 3 * 40       # the nearest distance of these is exactly 0
    torch.testing.assert_close(hip_ops.gs_knn3(pts.to(DEV)).cpu().double(), ref, rtol=1e-6, atol=1e-12)


# ---- fused D-SSIM + L1 ----------------------------------------------------------------------------------------------------------------------
def _loss_ref(a, b, lam):
    ad = a.double().requires_grad_(True)
    loss = (1 - lam) * (ad - b.double()).abs().mean() + lam * (1 - D.ssim(ad, b.double()))
    loss.backward()
    return loss.item(), ad.grad


@pytest.mark.parametrize("lam", [0.0, 0.2, 1.0])
@pytest.mark.parametrize("shape", [(3, 8, 8), (3, 11, 11), (3, 17, 33), (3, 128, 128), (1, 24, 40)], ids=lambda s: "x".join(map(str, s)))
def test_fused_ssim_l1_shapes_and_weights(hip_ops, shape, lam):
    g = torch.Generator().manual_seed(shape[1] * 1000 + shape[2])
    a = torch.rand(*shape, generator=g)
    b = (a + 0.2 * torch.randn(*shape, generator=g)).clamp(0, 1)
    ref, ref_grad = _loss_ref(a, b, lam)
    out3, work = hip_ops.gs_ssim_l1_fwd(a.to(DEV), b.to(DEV), lam)
    assert abs(out3[0].item() - ref) <= 1e-6, (out3[0].item(), ref)
    up = 0.7
    grad = hip_ops.gs_ssim_l1_bwd(a.to(DEV), b.to(DEV), lam, work, torch.full((1,), up, device=DEV))
    assert torch.isfinite(grad).all()
    assert D.rel_l2(grad.cpu(), up * ref_grad) <= 1e-4, D.rel_l2(grad.cpu(), up * ref_grad)


@pytest.mark.parametrize("lam", [0.2, 1.0])
def test_fused_ssim_l1_constant_images(hip_ops, lam):
    # E[x^2] - E[x]^2 cancels to ~0 inside the image (and not at the zero-padded border): what is left, c^2 S (1 - S) with S the window's
    # sum, is ~1e-8 beside c2 = 9e-4, so the value tells fp32 moments (off by up to 3e-5) and a window whose fp32 sum is rounded another way
    # (7e-6) from the real thing.  The gradient is not compared for this pair: it is the derivative of that cancellation
    a, b = torch.full((3, 32, 40), 0.3), torch.full((3, 32, 40), 0.6)
    ref, _ = _loss_ref(a, b, lam)
    out3, work = hip_ops.gs_ssim_l1_fwd(a.to(DEV), b.to(DEV), lam)
    assert torch.isfinite(out3).all()
    record_parity(f"gs_edges_ssim_constant[{lam}]", {"loss_abs_err": abs(out3[0].item() - ref)})
    assert abs(out3[0].item() - ref) <= 1e-6, (out3[0].item(), ref)
    assert torch.isfinite(hip_ops.gs_ssim_l1_bwd(a.to(DEV), b.to(DEV), lam, work, torch.ones(1, device=DEV))).all()
