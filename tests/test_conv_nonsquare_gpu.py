"""-m gpu: GroupNorm -> SiLU -> 3x3 convolution at non-square images, above the op level.

The library takes such a convolution on its LDS-haloed kernels by W, H and M (conv.hip v3d_conv_halo_variant; the rule is pinned on the CPU in
test_conv_halo_rule.py), the engine decides "this level rides the haloed kernel" from W alone (engine/blocks.py _halo_level / _small_norm) and
falls back to groupnorm(table=...) + conv3x3 when the library refuses.  Here both routes of `conv3x3_gn` run at an accepted and a refused shape
of each width, with the statistics computed by the call itself and handed over by the producing GEMM (what res_spatial does), against fp64
F.group_norm -> SiLU -> F.conv2d and with one image poisoned; and the full-width U-Net runs at three non-square latents whose width is 64 -
every ResBlock convolution of levels 0 - 2 haloed with stream-K tails, levels 0 - 1 haloed and level 2 refused, everything refused - against the
device oracle, with a census of the kernel family each convolution was given."""
import pytest
import torch

import op_cases
from conftest import device_oracle, full_inputs, odev, rel_cos
from v3d_amd.ops import GEMM_CONV3X3

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)
DEV = "cuda"
BF, F32 = torch.bfloat16, torch.float32

# (n, H, W), does the library take it on the haloed kernels
ENGINE_SHAPES = [((3, 4, 64), True), ((3, 3, 64), False), ((6, 7, 32), True), ((6, 6, 32), False), ((12, 13, 16), True), ((12, 12, 16), False),
                 ((8, 8, 64), False)]      # the last: H is fine, M % 192 is not


def _problem(n, H, W, C=320, N=320):
    g = torch.Generator().manual_seed(1000 * H + W + n)
    M = n * H * W
    r = lambda shape, dtype=BF, scale=1.0: op_cases._rand(g, shape, dtype, scale, DEV)
    off = ((torch.rand((C,), generator=g) * 2 - 1) * 0.5).to(DEV)
    return dict(x=(r((M, C), F32) + off).to(BF), x0=r((M, 64)), w0=r((C, 64), scale=0.125), b0=off.clone(),
                gamma=r((C,), F32, 0.3) + 1.0, beta=r((C,), F32, 0.3), w=r((9, N, C), scale=(9 * C) ** -0.5), bias=r((N,), F32, 0.5),
                add=r((n, N + 24), F32, 0.5), res=r((M, N)))


def _conv3x3_gn(ops, P, n, H, W, handed_over, poison=None):
    """engine.blocks.conv3x3_gn of the problem; handed_over: the input is produced by a GEMM whose epilogue gathers the GroupNorm statistics
    (blocks._gn_producer, the hand-over res_spatial makes).  poison = j: everything of image j is NaN before the call.
    Returns (input the convolution saw, output, kernel family of the convolution's launch)."""
    from v3d_amd.engine import blocks
    geo = blocks.Geo(n=n, B=1, T=n, H=H, W=W)
    S, C = H * W, P["x"].shape[1]
    ops.begin_evaluation(P["x"].device)
    st = None
    if handed_over:
        st, gkw = blocks._gn_producer(ops, n, S, C, P["x"].device, consumer_small=blocks._small_norm(ops, geo, C))
        assert st is not None, "the producer of a level the engine counts as haloed gathers the statistics"
        h = ops.linear(P["x0"], P["w0"], P["b0"], **gkw)
    else:
        h = P["x"]
    add, res = P["add"], P["res"]
    if poison is not None:
        h, add, res = h.clone(), add.clone(), res.clone()
        h[poison * S:(poison + 1) * S] = float("nan")
        res[poison * S:(poison + 1) * S] = float("nan")
        add[poison] = float("nan")
        if st is not None:
            st[poison] = float("nan")
    out = blocks.conv3x3_gn(ops, h, None, (P["gamma"], P["beta"], 1e-5), P["w"], P["bias"], geo, stats=st,
                            add=add, add_rpg=S, add_ld=add.stride(0), res1=res, c_acc=0.6, c_res1=0.75)
    family = ops.last_gemm_launch()["family"]
    torch.cuda.synchronize()
    return h, out.clone(), family


@pytest.mark.parametrize("handed_over", [False, True], ids=["own_stats", "producer_stats"])
@pytest.mark.parametrize("shape,accepted", ENGINE_SHAPES, ids=[f"{n}x{h}x{w}" for (n, h, w), _ in ENGINE_SHAPES])
def test_conv3x3_gn_both_routes(hip_ops, shape, accepted, handed_over):
    n, H, W = shape
    S = H * W
    P = _problem(n, H, W)
    N = P["w"].shape[1]
    h, out, family = _conv3x3_gn(hip_ops, P, n, H, W, handed_over)
    assert (family == 5) == accepted, f"kernel family {family}; the haloed kernels (5) are expected to {'take' if accepted else 'refuse'} this shape"
    kw = dict(bias=P["bias"], add=P["add"], res1=P["res"], c_acc=0.6, c_res1=0.75)
    ref = op_cases._conv_gn_ref64(h, None, P["gamma"], P["beta"], P["w"], kw, conv=shape, convt=None, silu=True, N=N)
    rel, cos = op_cases.compare(out, ref)
    print(f"[conv3x3_gn {shape} {'haloed' if accepted else 'fallback'} {'producer' if handed_over else 'own'} statistics] rel {rel:.3e} cos {cos:.6f}")
    assert rel <= op_cases.TOL_BF16 and cos >= 0.999, (rel, cos)
    for j in sorted({0, n // 2, n - 1}):
        _, out_p, fam_p = _conv3x3_gn(hip_ops, P, n, H, W, handed_over, poison=j)
        assert fam_p == family
        own = torch.zeros(n * S, dtype=torch.bool, device=DEV)
        own[j * S:(j + 1) * S] = True
        assert bool(torch.isnan(out_p[own].float()).all()), f"image {j} poisoned: some of its outputs are not NaN"
        diff = (out_p.view(torch.int16) != out.view(torch.int16)).any(dim=1) & ~own
        assert not bool(diff.any()), f"image {j} poisoned: {int(diff.sum())} rows of other images changed, first {diff.nonzero().flatten()[:8].tolist()}"
    hip_ops.check_health()


# ---- the full-width network --------------------------------------------------------------------------------------------------------------
# latents (H, W), T -> per level 0 / 1 / 2: None = the library refuses the level's GroupNorm -> conv (fallback), else (tiles, stream-K tail)
# of the launch with N = K = the level's width (test_conv_halo_rule.py holds the same rows without a GPU)
FULL = [
    ((72, 64), 4, [(192, True), (96, True), (48, True)]),
    ((24, 64), 3, [(48, False), (24, False), None]),
    ((8, 64), 4, [None, None, None]),
]


@pytest.mark.parametrize("hw,T,levels", FULL, ids=[f"{h}x{w}_T{t}" for (h, w), t, _ in FULL])
def test_full_width_nonsquare_vs_oracle(full_unet, monkeypatch, hw, T, levels):
    from oracle import sgm_oracle as O
    from v3d_amd import ops as ops_mod
    from v3d_amd import synth
    H, W = hw
    ops = ops_mod.get_ops()
    census = []
    inner = ops.gemm

    def counted(g):
        inner(g)
        if g.mode == GEMM_CONV3X3:
            rec = ops.last_gemm_launch()
            census.append((g.mode, g.Hout, g.Wout, g.N, g.gn_in is not None, rec["family"], g.K, g.stride, g.up, rec["tiles"], bool(rec["streamk_tail"])))

    monkeypatch.setattr(ops, "gemm", counted)
    x8, ts, ctx, y = full_inputs(2 * T, seed=H * 100 + W, H=H, W=W)
    ioi = torch.zeros(2, T)
    run = lambda: full_unet(x8.to(DEV), ts.to(DEV), context=ctx.to(DEV), y=y.to(DEV), num_video_frames=T, image_only_indicator=ioi.to(DEV)).float().cpu()
    out = run()
    first = list(census)
    again = run()
    monkeypatch.undo()
    assert torch.isfinite(out).all()
    ops.check_health()
    assert torch.equal(out, again), "two identical evaluations differ"
    assert census[len(first):] == first, "two identical evaluations launched different kernels"

    # the GroupNorm -> SiLU -> conv of the ResBlocks: 3 x 3, stride 1, no upsampling, whole 320-channel tiles, wide input
    for level, want in enumerate(levels):
        Hl, Wl, Cl = H >> level, W >> level, 320 << level
        here = [c for c in first if (c[1], c[2]) == (Hl, Wl) and c[7] == 1 and c[8] == 1 and c[3] % 320 == 0 and c[6] >= 320]
        assert here, f"level {level}: no ResBlock convolution seen at {Hl} x {Wl}"
        if want is None:
            assert not any(c[4] or c[5] == 5 for c in here), f"level {level} ({Hl} x {Wl}) is refused by the library, yet: {[c for c in here if c[4] or c[5] == 5]}"
        else:
            assert all(c[4] and c[5] == 5 for c in here), f"level {level} ({Hl} x {Wl}) rides the haloed kernels, yet: {[c for c in here if not (c[4] and c[5] == 5)]}"
            square = [c for c in here if c[3] == Cl and c[6] == Cl]
            assert square and all((c[9], c[10]) == want for c in square), f"level {level}: N = K = {Cl} launches {square}, the rule's table says {want}"
    assert not any(c[5] == 5 for c in first if c[2] not in (W, W >> 1, W >> 2)), "a haloed launch below level 2"

    with device_oracle() as od:
        ref = O.unet_forward(odev(full_unet.state_dict(), od), synth.unet_config(320), *odev((x8, ts, ctx, y), od), T, ioi.to(od)).cpu()
    rel, cos = rel_cos(out, ref)
    print(f"[full width {H} x {W}, T = {T}] rel {rel:.3e} cos {cos:.6f}; 3x3 launches {len(first)}, haloed {sum(c[5] == 5 for c in first)}")
    assert rel <= 4e-2 and cos >= 0.999, (rel, cos)
