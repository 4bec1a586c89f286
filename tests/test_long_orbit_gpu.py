"""-m gpu: orbits of more than 32 frames.  v3d_attn_temporal past its 32-frame tile (attn_temporal_long_kernel: 32-query tiles streaming 32-key
tiles with an online softmax) at the op level, and the product path end to end at T = 40 and 64: U-Net evaluation, sampler rollout, chunked
decode, the frame-sharded evaluation and the entry script.  Bars are those of the same quantities at <= 32 frames (test_ops_gpu.py,
test_engine_gpu.py, test_dist_gpu.py)."""
import importlib.util
import os

import pytest
import torch

import op_cases
from conftest import device_oracle, odev, rel_cos
from long_orbit import LONG, chunked_decode, long_decoder_latents, long_inputs, stored_grid
from tiny import TINY, build_decoder, build_denoiser, build_sampler, build_unet, to_dev

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)
DEV = "cuda"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TLONG_MAX = 1024                      # attn.hip TLONG_MAX: the largest Tq / Tk v3d_attn_temporal takes


@pytest.fixture(scope="module")
def emu():
    from oracle.ops_emul import EmulOps
    return EmulOps("cuda")


@pytest.fixture(scope="module")
def golden_long():
    return torch.load(os.path.join(ROOT, "tests", "golden", "v3d_long.pt"))


OP_SHAPES = [  # (B, Tq, Tk, S, heads)
    (2, 33, 33, 8, 2), (2, 40, 40, 8, 2), (1, 48, 48, 8, 3), (1, 64, 64, 8, 2), (1, 128, 128, 4, 2), (2, 1, 97, 8, 2),
    (2, 5, 40, 8, 2), (2, 20, 40, 8, 2),                          # frame-sharded: T_local queries over all 40 gathered keys
    (2, 40, 40, 4096, 5),                                         # the V3D 64 x 64 level (S = 4096, C = 320), cfg batch
    (1, TLONG_MAX, TLONG_MAX, 2, 1), (1, 7, TLONG_MAX, 2, 2),
]


@pytest.mark.parametrize("B,Tq,Tk,S,heads", OP_SHAPES, ids=[f"B{b}_Tq{tq}_Tk{tk}_S{s}_h{h}" for b, tq, tk, s, h in OP_SHAPES])
def test_attn_temporal_long_vs_sdpa(hip_ops, emu, B, Tq, Tk, S, heads):
    rel, cos = op_cases.case_attn_temporal(hip_ops, emu, DEV, B=B, Tq=Tq, Tk=Tk, S=S, heads=heads)
    assert rel <= op_cases.TOL_BF16 and cos >= 0.999, (rel, cos)


def test_attn_temporal_range_enforced(hip_ops):
    q = torch.zeros(1, TLONG_MAX + 1, 1, 64, dtype=torch.bfloat16, device=DEV)
    with pytest.raises(RuntimeError, match="Tq/Tk must be in"):
        hip_ops.attn_temporal(q, q, q, torch.empty_like(q), 1, 0.125)


def _fp64_attention(q, k, v, heads, scale):
    """Full-tensor host reference in fp64 of the bf16 inputs: q/out [B, Tq, S, C], k/v [B, Tk, S, C]."""
    B, Tq, S, C = q.shape
    Tk = k.shape[1]
    qf = q.double().cpu().reshape(B, Tq, S, heads, 64).permute(0, 2, 3, 1, 4)
    kf = k.double().cpu().reshape(B, Tk, S, heads, 64).permute(0, 2, 3, 1, 4)
    vf = v.double().cpu().reshape(B, Tk, S, heads, 64).permute(0, 2, 3, 1, 4)
    p = torch.softmax(qf @ kf.transpose(-1, -2) * scale, dim=-1)
    return (p @ vf).permute(0, 3, 1, 2, 4).reshape(B, Tq, S, C)


def _qkv(B, T, S, heads, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    C = heads * 64
    q = (torch.randn(B, T, S, C, generator=g) * scale).to(torch.bfloat16)
    k = (torch.randn(B, T, S, C, generator=g) * scale).to(torch.bfloat16)
    v = torch.randn(B, T, S, C, generator=g).to(torch.bfloat16)
    return q, k, v


def _run(hip_ops, q, k, v, heads):
    qd, kd, vd = q.to(DEV), k.to(DEV), v.to(DEV)
    out = torch.empty_like(qd)
    hip_ops.attn_temporal(qd, kd, vd, out, heads, 0.125)
    torch.cuda.synchronize()
    return out.cpu()


@pytest.mark.parametrize("T,late", [(40, 37), (128, 100)])
def test_online_softmax_running_max_jumps_at_a_late_tile(hip_ops, T, late):
    """cdna guide rule 26: one key row spiked against one query row, so that query's running max jumps at the key tile holding frame `late`
    (its earlier tiles' O and l are rescaled by ~2^-40); a second query is spiked at frame 2 (max set in the first tile, never grows after)."""
    B, S, heads = 2, 8, 2
    q, k, v = _qkv(B, T, S, heads, seed=31)
    b, s, h = 1, 5, 1
    qi, qj = T - 3, 4
    ch = slice(h * 64, h * 64 + 64)
    k[b, late, s, ch] = (q[b, qi, s, ch].float() * 6.0).to(torch.bfloat16)      # score ~ 6 |q|^2 / 8 ~ 48 above the rest
    k[b, 2, s, ch] = (q[b, qj, s, ch].float() * 6.0).to(torch.bfloat16)
    out = _run(hip_ops, q, k, v, heads)
    ref = _fp64_attention(q, k, v, heads, 0.125)
    rel, cos = rel_cos(out, ref)
    assert rel <= op_cases.TOL_BF16 and cos >= 0.999, (rel, cos)
    for qq, kk in ((qi, late), (qj, 2)):                         # the spiked rows: the attention is (almost) all on the spiked key
        row, want = out[b, qq, s, ch].double(), ref[b, qq, s, ch]
        assert (row - want).abs().max() <= 2e-2 * want.abs().max(), (qq, (row - want).abs().max())
        assert (want - v[b, kk, s, ch].double()).abs().max() < 1e-3


def test_online_softmax_large_logits(hip_ops):
    """|s * scale| around 30 - 60 everywhere (q, k ~ N(0, 40)): the exponent range the online softmax must carry across key tiles."""
    B, T, S, heads = 2, 72, 8, 2
    q, k, v = _qkv(B, T, S, heads, seed=47, scale=40.0 ** 0.5)
    ref = _fp64_attention(q, k, v, heads, 0.125)
    logits = (q.double().reshape(B, T, S, heads, 64)[:, :1] * k.double().reshape(B, T, S, heads, 64)).sum(-1) * 0.125
    assert 30.0 <= logits.abs().mean() <= 60.0, logits.abs().mean()
    out = _run(hip_ops, q, k, v, heads)
    assert torch.isfinite(out.float()).all()
    rel, cos = rel_cos(out, ref)
    assert rel <= op_cases.TOL_BF16 and cos >= 0.999, (rel, cos)


def test_run_to_run_bit_identical(hip_ops):
    q, k, v = _qkv(2, 48, 512, 5, seed=3)
    a, b = _run(hip_ops, q, k, v, 5), _run(hip_ops, q, k, v, 5)
    assert torch.equal(a.view(torch.int16), b.view(torch.int16))


def _oracle_unet(net, T, x8, ts, ctx, y, ioi):
    from oracle import sgm_oracle as O
    from v3d_amd import synth
    with device_oracle() as od:
        return O.unet_forward(odev(net.state_dict(), od), synth.unet_config(TINY["model_channels"]), *odev((x8, ts, ctx, y), od), T, ioi.to(od)).cpu()


@pytest.mark.parametrize("T,H,W", [(40, 16, 32), (64, 8, 64)])       # (latents whose deepest U-Net level has a multiple of 8 tokens: v3d_attn_spatial)
def test_unet_long_vs_oracle(T, H, W):
    g = torch.Generator().manual_seed(321 + T)
    n = 2 * T
    x8, ts = torch.randn(n, 8, H, W, generator=g), torch.randn(n, generator=g)
    ctx, y = torch.randn(n, 1, 1024, generator=g), torch.randn(n, 768, generator=g)
    ioi = torch.zeros(2, T)
    net = build_unet(DEV)
    ref = _oracle_unet(net, T, x8, ts, ctx, y, ioi)
    out = net(x8.to(DEV), ts.to(DEV), context=ctx.to(DEV), y=y.to(DEV), num_video_frames=T, image_only_indicator=ioi.to(DEV))
    rel, cos = rel_cos(out, ref)
    assert rel <= 4e-2 and cos >= 0.999, (rel, cos)


def test_unet_T40_vs_reference_fixture(golden_long):
    T = LONG["T"]
    _, _, _, x8, ts, ctx, y = long_inputs()
    net = build_unet(DEV)
    out = net(x8.to(DEV), ts.to(DEV), context=ctx.to(DEV), y=y.to(DEV), num_video_frames=T, image_only_indicator=torch.zeros(2, T, device=DEV))
    rel, cos = rel_cos(stored_grid(out), golden_long["unet_out"])
    assert rel <= 4e-2 and cos >= 0.999, (rel, cos)


def test_sampler_T40_vs_reference_fixture(golden_long):
    from v3d_amd.sgm.modules.diffusionmodules.wrappers import OpenAIWrapper
    T = LONG["T"]
    noise, c, uc, *_ = long_inputs()
    net = build_unet(DEV)
    sampler, den, wr = build_sampler(T, steps=LONG["steps"], device=DEV), build_denoiser(), OpenAIWrapper(net)
    extra = {"image_only_indicator": torch.zeros(2, T, device=DEV), "num_video_frames": T}
    z = sampler(lambda i, s, cc: den(wr, i, s, cc, **extra), noise.to(DEV), cond=to_dev(c, DEV), uc=to_dev(uc, DEV))
    rel, cos = rel_cos(stored_grid(z), golden_long["sample_z"])
    assert cos >= 0.99 and rel <= 0.1, (rel, cos)


def test_chunked_decode_T40_vs_reference_fixture(golden_long):
    dec = build_decoder(DEV)
    out = chunked_decode(dec, long_decoder_latents(DEV), LONG["decoding_t"])
    rel, cos = rel_cos(stored_grid(out), golden_long["dec_out"])
    assert rel <= 4e-2 and cos >= 0.999, (rel, cos)


def test_two_ranks_on_one_gpu_T40_sharded_equals_unsharded():
    """T = 40 split 20 + 20 over two processes on the one GPU: each rank's temporal attention is 20 queries x 40 gathered keys.  The worker
    and the bars are those of test_dist_gpu.py::test_two_ranks_on_one_gpu_hip_sharded_equals_unsharded."""
    import torch.multiprocessing as mp
    from test_dist_gpu import _free_port, _worker
    T, H, W, steps, world = 40, 16, 32, 2, 2
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
    assert [r[1] for r in res] == [20, 20]
    for rank, _, r_unet, r_dec, r_samp, sent in res:
        print(f"[sharded T={T} rank {rank}] unet rel/cos {r_unet}  decode {r_dec}  sampler({steps} steps) {r_samp}  sent {sent / 1e6:.1f} MB")
        assert r_unet[0] <= 2e-2 and r_unet[1] >= 0.9998, f"rank {rank}: sharded U-Net vs unsharded HIP: {r_unet}"
        assert r_dec[0] <= 1.5e-2 and r_dec[1] >= 0.9999, f"rank {rank}: sharded decode vs unsharded HIP: {r_dec}"
        assert r_samp[1] >= 0.995, f"rank {rank}: sharded sampler loop vs unsharded HIP: {r_samp}"
        assert sent > 0


def test_entry_point_sample_one_40_frames():
    spec = importlib.util.spec_from_file_location("v3d_entry", os.path.join(ROOT, "scripts", "pub", "V3D_512.py"))
    entry = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(entry)
    # (128 x 256: the 2 x 2 deepest level of a 128 x 128 image is below the 8-token granularity of v3d_attn_spatial, at any frame count)
    frames, _ = entry.sample_one(synthetic=True, num_frames=40, num_steps=2, model_channels=64, vae_ch=32, height=128, width=256)
    assert frames.shape == (40, 128, 256, 3) and frames.dtype.name == "uint8"
