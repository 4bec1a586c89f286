"""Images of any 64-px multiple, on the CPU: the oracle (oracle/sgm_oracle.py) and the product engine over the emulated C-ABI ops
(oracle/ops_emul.EmulOps, exact and bf16 modes) against tests/golden/v3d_res.pt, which the reference's own modules produced
(tools/gen_golden_res.py) at latents whose U-Net levels hold 15 / 60 and 81 / 324 tokens; and the size rule of the entry point's sample_one."""
import importlib.util
import os

import pytest
import torch

from conftest import rel_cos
from oracle import sgm_oracle as O
from oracle.ops_emul import EmulOps
from res_shapes import RES, res_inputs, stored_grid, unet_key
from tiny import TINY, build_denoiser, build_sampler, build_unet
from v3d_amd import synth
from v3d_amd.ops import use_backend
from v3d_amd.sgm.modules.diffusionmodules.video_model import VideoUNet
from v3d_amd.sgm.modules.diffusionmodules.wrappers import OpenAIWrapper

torch.set_grad_enabled(False)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = torch.load(os.path.join(ROOT, "tests", "golden", "v3d_res.pt"))
MODES = [(True, 5e-5, 0.999999), (False, 4e-2, 0.999)]          # the bars of test_engine_emul.py


def _close(a, b):
    assert a.shape == b.shape, (tuple(a.shape), tuple(b.shape))
    assert torch.allclose(a, b, rtol=1e-4, atol=1e-5), f"max abs diff {(a - b).abs().max().item():.3e}"


def test_fixture_params():
    assert GOLDEN["params"] == RES
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "v3d_res.pt")) < 250_000


@pytest.mark.parametrize("H,W", RES["unet_hw"])
def test_oracle_unet(H, W):
    p, T = TINY, RES["T"]
    cfg = synth.unet_config(p["model_channels"])
    sd = synth.seeded_state_dict(VideoUNet(**cfg), p["weight_seed"])
    _, _, _, x8, ts, ctx, y = res_inputs(H, W)
    _close(stored_grid(O.unet_forward(sd, cfg, x8, ts, ctx, y, T, torch.zeros(2, T))), GOLDEN[unet_key(H, W)])


def test_oracle_sampler():
    p, T = TINY, RES["T"]
    cfg = synth.unet_config(p["model_channels"])
    sd = synth.seeded_state_dict(VideoUNet(**cfg), p["weight_seed"])
    noise, c, uc, *_ = res_inputs(*RES["sample_hw"])
    ioi = torch.zeros(2, T)
    net = lambda x, t, ca, v: O.unet_forward(sd, cfg, x, t, ca, v, T, ioi)
    _close(stored_grid(O.sample_euler_edm(net, noise.clone(), c, uc, RES["steps"], T, p["min_scale"], p["max_scale"], p["sigma_max"])),
           GOLDEN["sample_z"])


@pytest.mark.parametrize("H,W", RES["unet_hw"])
@pytest.mark.parametrize("exact,tol,cosmin", MODES)
def test_engine_unet(H, W, exact, tol, cosmin):
    T = RES["T"]
    _, _, _, x8, ts, ctx, y = res_inputs(H, W)
    with use_backend(EmulOps("cpu", exact=exact)):
        out = build_unet()(x8, ts, context=ctx, y=y, num_video_frames=T, image_only_indicator=torch.zeros(2, T))
    rel, cos = rel_cos(stored_grid(out), GOLDEN[unet_key(H, W)])
    assert rel <= tol and cos >= cosmin, (rel, cos)


@pytest.mark.parametrize("exact,tol,cosmin", MODES)
def test_engine_sampler(exact, tol, cosmin):
    T = RES["T"]
    noise, c, uc, *_ = res_inputs(*RES["sample_hw"])
    with use_backend(EmulOps("cpu", exact=exact)):
        net = build_unet()
        sampler, den, wr = build_sampler(T, steps=RES["steps"]), build_denoiser(), OpenAIWrapper(net)
        extra = {"image_only_indicator": torch.zeros(2, T), "num_video_frames": T}
        z = sampler(lambda i, s, cc: den(wr, i, s, cc, **extra), noise.clone(), cond=c, uc=uc)
    rel, cos = rel_cos(stored_grid(z), GOLDEN["sample_z"])
    assert rel <= tol and cos >= cosmin, (rel, cos)


def _entry():
    spec = importlib.util.spec_from_file_location("v3d_entry", os.path.join(ROOT, "scripts", "pub", "V3D_512.py"))
    entry = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(entry)
    return entry


@pytest.mark.parametrize("height,width", [(520, 512), (512, 96), (0, 512), (512, -64), (512.0, 512)])
def test_sample_one_rejects_sizes_off_the_64_px_grid(height, width):
    """Checked before a model is built or a device is touched (device="cuda" on a machine without one)."""
    with pytest.raises(ValueError, match="multiple of 64"):
        _entry().sample_one(synthetic=True, height=height, width=width, device="cuda", num_frames=2, num_steps=1)


def test_entry_point_flags_check_the_size():
    import subprocess
    import sys
    r = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "pub", "V3D_512.py"), "--synthetic", "--height", "576", "--width", "600"],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 2 and "width must be a positive multiple of 64" in r.stderr, (r.returncode, r.stderr[-2000:])
