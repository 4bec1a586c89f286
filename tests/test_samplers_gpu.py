"""-m gpu: the sampler-loop kernels of csrc/noise.hip (v3d_randn_add, v3d_lincomb_f32) and the ancestral / DPM++ / linear-multistep samplers
on the HIP kernels.  The noise is held to its numpy restatement (tests/philox_ref.py, pinned to the Random123 known answers): a counter
or key mistake gives O(1) errors, so 1e-5 pins the indexing; what is left is logf / sincospif rounding."""
import pytest
import torch

from conftest import record_parity, rel_cos
from sampler_emul import randn_ref
from test_samplers_emul import KINDS, make_sampler, run_tiny

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)


@pytest.mark.parametrize("seed,call", [(1234, 0), (1234, 5), (0, 1), ((0xDEADBEEF << 32) | 0x12345678, 0xFFFFFFFF)])
def test_randn_add_matches_restatement(hip_ops, seed, call):
    B, Tg, C, H, W = 2, 5, 4, 16, 16
    for t0, tl in ((0, Tg), (2, 2), (4, 1)):
        shape = (B * tl, C, H, W)
        ref = randn_ref(shape, seed, call, t0, tl, Tg)
        z = hip_ops.randn_add(None, 1.0, seed, call, t0=t0, T_local=tl, T_global=Tg, out=torch.empty(shape, device="cuda"))
        assert (z.cpu() - ref).abs().max().item() <= 1e-5, (t0, tl)
        x = torch.randn(shape, generator=torch.Generator().manual_seed(seed & 0xFFFF)).cuda()
        y = hip_ops.randn_add(x, 0.37, seed, call, t0=t0, T_local=tl, T_global=Tg)
        assert (y.cpu() - (x.cpu() + 0.37 * ref)).abs().max().item() <= 1e-5
        hip_ops.randn_add(x, 0.37, seed, call, t0=t0, T_local=tl, T_global=Tg, out=x)          # in place
        assert torch.equal(x, y)


def test_randn_add_shards_tile_the_full_tensor_bitwise(hip_ops):
    B, Tg, E = 3, 18, 4 * 64 * 64
    full = hip_ops.randn_add(None, 1.0, 99, 7, out=torch.empty(B * Tg, E, device="cuda"))
    parts = []
    for t0, tl in ((0, 3), (3, 3), (6, 2), (8, 2), (10, 2), (12, 2), (14, 2), (16, 2)):
        z = hip_ops.randn_add(None, 1.0, 99, 7, t0=t0, T_local=tl, T_global=Tg, out=torch.empty(B * tl, E, device="cuda"))
        parts.append(z.reshape(B, tl, E))
    assert torch.equal(torch.cat(parts, dim=1).reshape(B * Tg, E), full)


def test_randn_add_moments(hip_ops):
    """2^24 draws: mean, variance, every lane of the Box-Muller groups, and the correlation of consecutive draw indices (steps)."""
    rows = 1 << 22
    a = hip_ops.randn_add(None, 1.0, 2024, 0, out=torch.empty(rows, 4, device="cuda")).double()
    b = hip_ops.randn_add(None, 1.0, 2024, 1, out=torch.empty(rows, 4, device="cuda")).double()
    mean, var = a.mean().item(), a.var().item()
    corr = ((a - a.mean()) * (b - b.mean())).mean().item() / (a.std() * b.std()).item()
    lane_mean = a.mean(dim=0).abs().max().item()
    record_parity("randn_add_moments", {"mean": mean, "var": var, "corr_consecutive_calls": corr, "max_lane_mean": lane_mean})
    assert torch.isfinite(a).all()
    assert abs(mean) <= 1e-3 and abs(var - 1.0) <= 2e-3, (mean, var)
    assert abs(corr) <= 1e-3, corr
    assert lane_mean <= 2e-3, lane_mean


@pytest.mark.parametrize("nterms", [1, 2, 3, 6])
@pytest.mark.parametrize("n", [18 * 4 * 64 * 64, 1001])
def test_lincomb_matches_torch(hip_ops, nterms, n):
    g = torch.Generator().manual_seed(nterms * 7 + n)
    srcs = [torch.randn(n, generator=g).cuda() for _ in range(nterms)]
    coefs = [float(c) for c in torch.randn(nterms, generator=g)]
    want = sum(c * s.double() for c, s in zip(coefs, srcs))
    out = hip_ops.lincomb_f32(srcs, coefs)
    scale = want.abs().max().item()
    assert (out.double() - want).abs().max().item() <= 1e-6 * scale * nterms
    s0 = srcs[0].clone()
    hip_ops.lincomb_f32([s0] + srcs[1:], coefs, out=s0)                # out aliases the first source
    assert torch.equal(s0, out)
    if n % 4 == 0:                                                       # a misaligned view takes the scalar path
        off = [s[1:n - 3] for s in srcs]
        o2 = hip_ops.lincomb_f32(off, coefs)
        assert (o2.double() - want[1:n - 3]).abs().max().item() <= 1e-6 * scale * nterms


@pytest.fixture(scope="module")
def tiny_net():
    from tiny import build_unet
    return build_unet("cuda")


@pytest.mark.parametrize("kind", list(KINDS))
def test_sampler_on_hip_matches_reference_fixture(tiny_net, kind):
    import os

    from conftest import ROOT
    fx = torch.load(os.path.join(ROOT, "tests", "golden", "v3d_samplers.pt"))
    kw = {"noise_seed": fx["seed"]} if kind.endswith("ancestral") else {}
    z, calls = run_tiny(make_sampler(kind, fx["steps"], **kw), tiny_net, "cuda")
    rel, cos = rel_cos(z, fx["z"][kind])
    record_parity(f"sampler_{kind}_vs_reference", {"rel": rel, "cos": cos, "calls": calls, "steps": fx["steps"]})
    assert calls == fx["calls"][kind]
    assert torch.isfinite(z).all()
    assert cos >= 0.99 and rel <= 0.1, (kind, rel, cos)
    if kind.endswith("ancestral"):
        z2, _ = run_tiny(make_sampler(kind, fx["steps"], **kw), tiny_net, "cuda")
        assert torch.equal(z, z2), "same seed, same inputs: the run must repeat bit for bit"


def _local_denoiser(inp, sigma, cc):
    """Frame-local stand-in for the network (each output frame depends on its own input frame only), so a frame shard can be run alone."""
    return 0.5 * inp + 0.1 * torch.tanh(inp)


@pytest.mark.parametrize("kind", ["euler_ancestral", "dpmpp2s_ancestral"])
def test_frame_sharded_ancestral_equals_unsharded(hip_ops, kind):
    """Every rank of an 18-frame, 8-way frame shard (dist.local_sampler's noise map, SimFrameShard for the geometry) runs the sampler on its
    own frames; their concatenation is the unsharded run of the same seed, bit for bit (the updates are elementwise, the noise is a function
    of the global element index)."""
    from v3d_amd.dist import SimFrameShard, local_sampler
    T, B = 18, 1
    x = torch.randn(B * T, 4, 64, 64, generator=torch.Generator().manual_seed(5)).cuda()
    full = make_sampler(kind, 5, guided=False, noise_seed=77)
    z = full(_local_denoiser, x.clone(), cond={}, uc={})
    parts = []
    for rank in range(8):
        sh = SimFrameShard(T, 8, rank)
        s = local_sampler(make_sampler(kind, 5, guided=False, noise_seed=77), sh)
        parts.append(s(_local_denoiser, sh.take_frames(x, B), cond={}, uc={}))
    zs = torch.cat(parts, dim=0)
    assert torch.equal(zs, z)
    unmapped = make_sampler(kind, 5, guided=False, noise_seed=77)(_local_denoiser, x[6:8].clone(), cond={}, uc={})
    assert (unmapped - z[6:8]).abs().max().item() > 1e-2          # without the noise map a shard would draw other numbers
