"""-m gpu: images of any 64-px multiple.  v3d_attn_spatial_ld (spatial attention over a token count that is not a multiple of 8, V^T rows at a
padded stride) at the op level, and the product path end to end at latents whose U-Net levels hold such token counts: the tiny U-Net against the
device oracle and the reference fixture tests/golden/v3d_res.pt, one full-width evaluation at the 576 x 576 shape, the frame-sharded evaluation
and the entry script.  Bars are those of the same quantities at token counts that are multiples of 8 (test_ops_gpu.py, test_long_orbit_gpu.py,
test_headline_parity_gpu.py)."""
import importlib.util
import os

import pytest
import torch
import torch.nn.functional as F

import op_cases
from conftest import device_oracle, odev, rel_cos
from res_shapes import RES, res_inputs, stored_grid, unet_key
from tiny import TINY, build_denoiser, build_sampler, build_unet, to_dev

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)
DEV = "cuda"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BF = torch.bfloat16


@pytest.fixture(scope="module")
def golden_res():
    return torch.load(os.path.join(ROOT, "tests", "golden", "v3d_res.pt"))


def _inputs(n_img, S, heads, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    C = heads * 64
    qk = (torch.randn(n_img * S, 2 * C, generator=g) * scale).to(BF)
    v = torch.randn(n_img, C, S, generator=g).to(BF)              # V^T [n_img][C][S]
    return qk, v


def _attn(hip_ops, qk, v, n_img, S, heads, pad=float("nan"), ldv=None):
    """v3d_attn_spatial_ld through HipOps: V^T in a [n_img, C, ldv] buffer whose pad columns hold `pad`, passed as its [..., :S] view."""
    C = heads * 64
    ldv = ldv or -(-S // 8) * 8
    buf = torch.full((n_img, C, ldv), pad, dtype=BF, device=DEV)
    buf[..., :S] = v.to(DEV)
    qkd = qk.to(DEV)
    out = torch.zeros(n_img * S, C, dtype=BF, device=DEV)
    hip_ops.attn_spatial(qkd[:, :C], qkd[:, C:], buf[..., :S], out, n_img, S, heads, 0.125)
    torch.cuda.synchronize()
    return out.cpu()


def _sdpa(qk, v, n_img, S, heads, dtype=torch.float32, dev=None):
    C = heads * 64
    q = qk[:, :C].to(dev, dtype).reshape(n_img, S, heads, 64).permute(0, 2, 1, 3)
    k = qk[:, C:].to(dev, dtype).reshape(n_img, S, heads, 64).permute(0, 2, 1, 3)
    vv = v.to(dev, dtype).reshape(n_img, heads, 64, S).permute(0, 1, 3, 2)
    return F.scaled_dot_product_attention(q, k, vv, scale=0.125).permute(0, 2, 1, 3).reshape(n_img * S, C).cpu()


S_RAGGED = [1, 3, 4, 7, 9, 15, 25, 36, 49, 60, 81, 100, 121, 324, 1156, 1444]


@pytest.mark.parametrize("n_img", [1, 3])
@pytest.mark.parametrize("heads", [1, 5, 10])
@pytest.mark.parametrize("S", S_RAGGED)
def test_attn_spatial_ld_vs_sdpa(hip_ops, S, heads, n_img):
    qk, v = _inputs(n_img, S, heads, seed=S * 31 + heads * 7 + n_img)
    out = _attn(hip_ops, qk, v, n_img, S, heads)
    with device_oracle() as od:
        ref = _sdpa(qk, v, n_img, S, heads, dev=od)
    rel, cos = op_cases.compare(out, ref)
    assert rel <= op_cases.TOL_BF16 and cos >= 0.999, (rel, cos)


@pytest.mark.parametrize("S,ldv", [(3, 8), (81, 88), (81, 160), (324, 328), (1444, 1448), (64, 72), (1024, 1032)])
def test_pad_independence(hip_ops, S, ldv):
    """The result does not depend on what the pad columns S..ldv-1 hold: NaN, +1e4, -1e4 give bit-identical outputs (also with S % 8 == 0
    and a wider stride, which runs the ragged kernel too)."""
    n_img, heads = 3, 5
    qk, v = _inputs(n_img, S, heads, seed=5 + S)
    outs = [_attn(hip_ops, qk, v, n_img, S, heads, pad=p, ldv=ldv) for p in (float("nan"), 1e4, -1e4)]
    assert torch.isfinite(outs[0].float()).all()
    for o in outs[1:]:
        assert torch.equal(o.view(torch.int16), outs[0].view(torch.int16))
    with device_oracle() as od:
        rel, cos = op_cases.compare(outs[0], _sdpa(qk, v, n_img, S, heads, dev=od))
    assert rel <= op_cases.TOL_BF16 and cos >= 0.999, (rel, cos)


def _fp64_kernel_operands(qk, v, n_img, S, heads):
    """fp64 attention of the operands the kernel multiplies: q pre-scaled by scale * log2(e) and re-rounded to bf16 once (attn.hip
    attn_spatial_v2_kernel: 2^-9 relative per element), the softmax taken in the exp2 domain."""
    C = heads * 64
    sc2 = torch.tensor(0.125, dtype=torch.float32) * torch.tensor(1.4426950408889634, dtype=torch.float32)
    q = (qk[:, :C].float() * sc2).to(BF).double().reshape(n_img, S, heads, 64).permute(0, 2, 1, 3)
    k = qk[:, C:].double().reshape(n_img, S, heads, 64).permute(0, 2, 1, 3)
    vv = v.double().reshape(n_img, heads, 64, S).permute(0, 1, 3, 2)
    p = torch.softmax((q @ k.transpose(-1, -2)) * torch.log(torch.tensor(2.0, dtype=torch.float64)), dim=-1)
    return (p @ vv).permute(0, 2, 1, 3).reshape(n_img * S, C)


def test_large_logits_S81(hip_ops):
    """|s * scale| around 30 - 60 (q, k ~ N(0, 40)) at S = 81: the exponent range the streamed softmax carries into the masked last tile.
    Against fp64 of the operands the kernel multiplies at the op bars; against fp64 of the raw operands at the cosine bar (at these logits the
    2^-9 rounding of the pre-scaled q moves a weight by up to ~8 %, the same in the dense kernels)."""
    n_img, S, heads = 3, 81, 5
    qk, v = _inputs(n_img, S, heads, seed=47, scale=40.0 ** 0.5)
    C = heads * 64
    logits = (qk[:S, :64].double() @ qk[:S, C:C + 64].double().T) * 0.125
    assert 30.0 <= logits.abs().mean() <= 60.0, logits.abs().mean()
    out = _attn(hip_ops, qk, v, n_img, S, heads)
    assert torch.isfinite(out.float()).all()
    rel, cos = op_cases.compare(out, _fp64_kernel_operands(qk, v, n_img, S, heads))
    assert rel <= op_cases.TOL_BF16 and cos >= 0.999, (rel, cos)
    _, cos = op_cases.compare(out, _sdpa(qk, v, n_img, S, heads, dtype=torch.float64, dev="cpu"))
    assert cos >= 0.999, cos


def test_run_to_run_bit_identical_S324(hip_ops):
    qk, v = _inputs(4, 324, 10, seed=3)
    a, b = _attn(hip_ops, qk, v, 4, 324, 10), _attn(hip_ops, qk, v, 4, 324, 10)
    assert torch.equal(a.view(torch.int16), b.view(torch.int16))


def test_dense_calls_keep_the_abi7_entry(hip_ops):
    """S % 8 == 0 with ldv == S: v3d_attn_spatial_ld runs exactly v3d_attn_spatial (bit-identical), and a ragged S needs a padded stride."""
    n_img, S, heads = 2, 256, 5
    C = heads * 64
    qk, v = _inputs(n_img, S, heads, seed=9)
    qkd, vd = qk.to(DEV), v.to(DEV)
    outs = []
    for fn in ("v3d_attn_spatial", "v3d_attn_spatial_ld"):
        o = torch.zeros(n_img * S, C, dtype=BF, device=DEV)
        args = [qkd.data_ptr(), qkd.stride(0), qkd.data_ptr() + 2 * C, qkd.stride(0), vd.data_ptr()]
        args += [S] if fn.endswith("_ld") else []
        args += [o.data_ptr(), C, n_img, S, heads, 0.125, None]
        assert getattr(hip_ops.lib, fn)(*args) == 0, hip_ops.lib.v3d_last_error()
        torch.cuda.synchronize()
        outs.append(o.cpu())
    assert torch.equal(outs[0].view(torch.int16), outs[1].view(torch.int16))
    qk, v = _inputs(1, 81, 1, seed=1)
    with pytest.raises(RuntimeError, match="ldv must be"):
        _attn(hip_ops, qk, v, 1, 81, 1, ldv=81)


# ---- the U-Net at latents with ragged levels ----------------------------------------------------------------------------------------------
UNET_HW = [(8, 8), (16, 16), (24, 24), (40, 40), (24, 40), (56, 88), (72, 72)]     # deepest level 1, 4, 9, 25, 15, 77, 81 tokens


@pytest.mark.parametrize("H,W", UNET_HW, ids=[f"{h}x{w}" for h, w in UNET_HW])
def test_unet_vs_oracle(H, W):
    from oracle import sgm_oracle as O
    from v3d_amd import synth
    T = TINY["T"]
    g = torch.Generator().manual_seed(500 + H * W)
    n = 2 * T
    x8, ts = torch.randn(n, 8, H, W, generator=g), torch.randn(n, generator=g)
    ctx, y = torch.randn(n, 1, 1024, generator=g), torch.randn(n, 768, generator=g)
    ioi = torch.zeros(2, T)
    net = build_unet(DEV)
    out = net(x8.to(DEV), ts.to(DEV), context=ctx.to(DEV), y=y.to(DEV), num_video_frames=T, image_only_indicator=ioi.to(DEV))
    with device_oracle() as od:
        ref = O.unet_forward(odev(net.state_dict(), od), synth.unet_config(TINY["model_channels"]), *odev((x8, ts, ctx, y), od), T, ioi.to(od)).cpu()
    assert out.shape == (n, 4, H, W)
    rel, cos = rel_cos(out, ref)
    assert rel <= 4e-2 and cos >= 0.999, (rel, cos)


@pytest.mark.parametrize("H,W", RES["unet_hw"])
def test_unet_vs_reference_fixture(golden_res, H, W):
    T = RES["T"]
    _, _, _, x8, ts, ctx, y = res_inputs(H, W)
    net = build_unet(DEV)
    out = net(x8.to(DEV), ts.to(DEV), context=ctx.to(DEV), y=y.to(DEV), num_video_frames=T, image_only_indicator=torch.zeros(2, T, device=DEV))
    rel, cos = rel_cos(stored_grid(out), golden_res[unet_key(H, W)])
    assert rel <= 4e-2 and cos >= 0.999, (rel, cos)


def test_sampler_vs_reference_fixture(golden_res):
    from v3d_amd.sgm.modules.diffusionmodules.wrappers import OpenAIWrapper
    T = RES["T"]
    noise, c, uc, *_ = res_inputs(*RES["sample_hw"])
    net = build_unet(DEV)
    sampler, den, wr = build_sampler(T, steps=RES["steps"], device=DEV), build_denoiser(), OpenAIWrapper(net)
    extra = {"image_only_indicator": torch.zeros(2, T, device=DEV), "num_video_frames": T}
    z = sampler(lambda i, s, cc: den(wr, i, s, cc, **extra), noise.to(DEV), cond=to_dev(c, DEV), uc=to_dev(uc, DEV))
    rel, cos = rel_cos(stored_grid(z), golden_res["sample_z"])
    assert cos >= 0.99 and rel <= 0.1, (rel, cos)


def test_full_width_eval_576_vs_oracle(full_unet):
    """Width 320 (the V3D network), T = 4 frames of the guided batch (8 images) at 72 x 72 latents: 81 / 324 tokens at the two deepest levels."""
    from conftest import full_inputs
    from oracle import sgm_oracle as O
    from v3d_amd import synth
    T, H, W = 4, 72, 72
    x8, ts, ctx, y = full_inputs(2 * T, seed=576, H=H, W=W)
    ioi = torch.zeros(2, T)
    out = full_unet(x8.to(DEV), ts.to(DEV), context=ctx.to(DEV), y=y.to(DEV), num_video_frames=T, image_only_indicator=ioi.to(DEV)).float().cpu()
    assert torch.isfinite(out).all()
    with device_oracle() as od:
        ref = O.unet_forward(odev(full_unet.state_dict(), od), synth.unet_config(320), *odev((x8, ts, ctx, y), od), T, ioi.to(od)).cpu()
    rel, cos = rel_cos(out, ref)
    assert rel <= 4e-2 and cos >= 0.999, (rel, cos)


def test_two_ranks_on_one_gpu_24x40_sharded_equals_unsharded():
    """T = 4 split 2 + 2 over two processes on the one GPU at 24 x 40 latents (15 / 60 tokens at the two deepest levels).  The worker and the
    bars are those of test_dist_gpu.py::test_two_ranks_on_one_gpu_hip_sharded_equals_unsharded."""
    import torch.multiprocessing as mp
    from test_dist_gpu import _free_port, _worker
    T, H, W, steps, world = 4, 24, 40, 2, 2
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, world, port, q, T, H, W, steps, 1)) for r in range(world)]
    for pr in procs:
        pr.start()
    res = [q.get(timeout=900) for _ in range(world)]
    for pr in procs:
        pr.join(timeout=120)
    for r in res:
        assert r[1] >= 0, f"rank {r[0]} failed:\n{r[2]}"
    res.sort()
    assert [r[1] for r in res] == [2, 2]
    for rank, _, r_unet, r_dec, r_samp, sent in res:
        print(f"[sharded {H}x{W} rank {rank}] unet rel/cos {r_unet}  decode {r_dec}  sampler({steps} steps) {r_samp}  sent {sent / 1e6:.1f} MB")
        assert r_unet[0] <= 2e-2 and r_unet[1] >= 0.9998, f"rank {rank}: sharded U-Net vs unsharded HIP: {r_unet}"
        assert r_dec[0] <= 1.5e-2 and r_dec[1] >= 0.9999, f"rank {rank}: sharded decode vs unsharded HIP: {r_dec}"
        assert r_samp[1] >= 0.995, f"rank {rank}: sharded sampler loop vs unsharded HIP: {r_samp}"
        assert sent > 0


def test_entry_point_sample_one_576():
    spec = importlib.util.spec_from_file_location("v3d_entry", os.path.join(ROOT, "scripts", "pub", "V3D_512.py"))
    entry = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(entry)
    frames, _ = entry.sample_one(height=576, width=576, num_frames=4, num_steps=2, synthetic=True, model_channels=64, vae_ch=32)
    assert frames.shape == (4, 576, 576, 3) and frames.dtype.name == "uint8"
    assert int(frames.max()) > int(frames.min())
