"""Which GroupNorm -> SiLU -> 3x3 convolutions ride the LDS-haloed kernels (v3d_amd/csrc/conv.hip v3d_conv_halo_variant, gemm.hip plan_gemm), at
non-square images, read off the library's planner on the CPU.  The rule depends on the image's height as well as its width - M % 192 == 0 and
H >= 192 / W + 1 (a halo of tile rows + 2 lines touches at most two images) - while the engine (engine/blocks.py _halo_level) decides from W alone
and falls back to norm + convolution when the library refuses.  The tables below pin, per product resolution and U-Net level, where the fast path
ends: a planner change that moves a resolution off it (or onto it) shows here without a GPU.

The planner never dereferences a pointer: the arguments carry synthetic aligned addresses, as in tests/test_gemm_plan.py."""
import ctypes
import os

import pytest

from v3d_amd.hip import _GemmArgs
from v3d_amd.ops import GEMM_CONV3X3, OpsBase

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CUS = 256
DEFAULT_POLICY = (0, -1, 2, 1, 1)      # gemm.hip env_policy with no knob set: V3D_GEMM_IMPL, V3D_GEMM_SPLITK, V3D_GEMM_V3S, V3D_GEMM_V6, V3D_STREAMK
KNOBS = ("V3D_GEMM_IMPL", "V3D_GEMM_SPLITK", "V3D_GEMM_V3S", "V3D_GEMM_V6", "V3D_STREAMK")


@pytest.fixture(scope="module")
def lib():
    path = os.path.join(ROOT, "v3d_amd", "lib", "libv3d_hip.so")
    if not os.path.exists(path):
        import __graft_entry__
        __graft_entry__.build()
    lb = ctypes.CDLL(path)
    lb.v3d_debug_gemm_plan.restype = ctypes.c_int
    lb.v3d_debug_gemm_plan.argtypes = [ctypes.POINTER(_GemmArgs), ctypes.c_int, ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_longlong)]
    lb.v3d_gemm_gn_in_supported.restype = ctypes.c_int
    lb.v3d_gemm_gn_in_supported.argtypes = [ctypes.POINTER(_GemmArgs)]
    return lb


def conv_gn_args(n, H, W, N, K, *, stats=True, res=True):
    """The second convolution of a ResBlock half at n images of H x W: GroupNorm table in, per-image statistics out, residual."""
    a = _GemmArgs()
    S = H * W
    for i, name in enumerate(("A", "W", "out", "bias", "gn_in_table") + (("res1",) if res else ()) + (("gn_stats",) if stats else ())):
        setattr(a, name, (i + 1) << 32)
    a.M, a.N, a.K = n * S, N, K
    a.lda, a.ldw, a.ldo, a.ldr1 = K, K, N, N if res else 0
    a.a_rows = n * S
    a.c_acc, a.c_res1, a.c_res2 = 0.6, 0.75, 1.0
    a.mode, a.batch = GEMM_CONV3X3, 1
    a.Hin, a.Win, a.Hout, a.Wout, a.stride, a.up = H, W, H, W, 1, 1
    a.gn_in_rps, a.gn_in_rows, a.gn_in_silu = S, n, 1
    if stats:
        a.gn_rps, a.gn_cpg, a.gn_nslots = S, N // 32, OpsBase.gn_nslots(S)
    return a


def route(lib, a):
    """None = refused (the engine falls back to norm + convolution), else (tiles, stream-K tail planned) of the haloed launch."""
    out = (ctypes.c_longlong * 10)()
    rc = lib.v3d_debug_gemm_plan(ctypes.byref(a), CUS, (ctypes.c_int * 5)(*DEFAULT_POLICY), out)
    assert rc == 0, "the planner rejects the arguments themselves"
    kernel, family, bm, bn, tiles, grid, splitk, tail, gn_epi, _ = (int(v) for v in out)
    if not any(os.environ.get(k) for k in KNOBS):      # v3d_gemm_gn_in_supported reads the policy from the environment
        assert bool(lib.v3d_gemm_gn_in_supported(ctypes.byref(a))) == (kernel >= 0), "v3d_gemm_gn_in_supported and the planner disagree"
    if kernel < 0:
        return None
    assert (family, bm, bn) == (5, 192, 320), f"gn_in launch planned on family {family}, {bm} x {bn} tiles"
    assert splitk == 0 and grid == (CUS if tail else min(tiles, CUS))
    assert tiles == a.M // 192 * (a.N // 320)
    assert gn_epi == (1 if a.gn_stats else 0)
    return tiles, tail != 0


REFUSED = None
# latents H x W, images n -> levels 0 / 1 / 2 (H >> l x W >> l, N = K = 320 << l)
PRODUCT = [
    ((72, 64), 8, [(192, True), (96, True), (48, True)]),
    ((72, 64), 36, [(864, False), (432, True), (216, True)]),
    ((56, 64), 36, [(672, True), (336, True), (168, True)]),
    ((56, 64), 8, [REFUSED, REFUSED, REFUSED]),                        # M % 192
    ((24, 64), 6, [(48, False), (24, False), REFUSED]),                # level 2: H = 6 < 13
    ((8, 64), 36, [(96, False), REFUSED, REFUSED]),                    # level 1: H = 4 < 7
    ((8, 64), 8, [REFUSED, REFUSED, REFUSED]),
    ((64, 72), 36, [REFUSED, REFUSED, REFUSED]),                       # W
]


@pytest.mark.parametrize("hw,n,levels", PRODUCT, ids=[f"{h}x{w}_n{n}" for (h, w), n, _ in PRODUCT])
def test_product_resolutions(lib, hw, n, levels):
    for level, want in enumerate(levels):
        H, W, C = hw[0] >> level, hw[1] >> level, 320 << level
        got = route(lib, conv_gn_args(n, H, W, C, C))
        assert got == want, f"{hw[0]} x {hw[1]} latents, {n} images, level {level} ({H} x {W}, N = K = {C}): planned {got}, recorded {want}"


ACCEPTED = [(3, 4, 64), (3, 5, 64), (3, 7, 64), (6, 7, 32), (2, 9, 32), (1, 36, 32), (12, 13, 16), (6, 14, 16), (2, 18, 16)]
REFUSED_SHAPES = [(3, 3, 64), (6, 6, 32), (12, 12, 16), (1, 5, 64)]


@pytest.mark.parametrize("n,H,W", ACCEPTED)
def test_single_launch_accepted(lib, n, H, W):
    for stats in (False, True):
        got = route(lib, conv_gn_args(n, H, W, 320, 320, stats=stats, res=stats))
        assert got == (n * H * W // 192, False), got


@pytest.mark.parametrize("n,H,W", REFUSED_SHAPES)
def test_single_launch_refused(lib, n, H, W):
    for stats in (False, True):
        assert route(lib, conv_gn_args(n, H, W, 320, 320, stats=stats, res=stats)) is REFUSED


def test_nonsquare_streamk_tail(lib):
    """(36, 14, 16), N = 320, K = 1280: 42 tiles of 40 chunks on a 256-block grid."""
    assert route(lib, conv_gn_args(36, 14, 16, 320, 1280)) == (42, True)


@pytest.mark.parametrize("W,hmin", [(64, 4), (32, 7), (16, 13)])
def test_minimum_height(lib, W, hmin):
    """H >= 192 / W + 1, with M % 192 == 0 held on both sides of the boundary (n = 192 images)."""
    assert hmin == 192 // W + 1
    for N in (320, 640, 1280):
        for H in (hmin, hmin + 1):
            got = route(lib, conv_gn_args(192, H, W, N, 320))
            assert got is not REFUSED and got[0] == H * W * (N // 320), (H, W, N, got)
        assert route(lib, conv_gn_args(192, hmin - 1, W, N, 320)) is REFUSED
