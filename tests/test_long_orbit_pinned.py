"""Pin the CPU oracle (oracle/sgm_oracle.py) to the reference at 40 frames: tests/golden/v3d_long.pt was produced by the reference's own modules
(tools/gen_golden_long.py).  fp32 restatement vs reference: rtol 1e-4 / atol 1e-5."""
import os

import torch

from long_orbit import LONG, long_decoder_latents, long_inputs, stored_grid
from oracle import sgm_oracle as O
from tiny import TINY
from v3d_amd import synth
from v3d_amd.sgm.modules.autoencoding.temporal_ae import VideoDecoder
from v3d_amd.sgm.modules.diffusionmodules.video_model import VideoUNet

torch.set_grad_enabled(False)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = torch.load(os.path.join(ROOT, "tests", "golden", "v3d_long.pt"))


def _close(a, b):
    assert a.shape == b.shape, (tuple(a.shape), tuple(b.shape))
    assert torch.allclose(a, b, rtol=1e-4, atol=1e-5), f"max abs diff {(a - b).abs().max().item():.3e}"


def test_fixture_params():
    assert GOLDEN["params"] == LONG and LONG["T"] > 32


def test_unet_eval_and_sampler_T40():
    p, T = TINY, LONG["T"]
    cfg = synth.unet_config(p["model_channels"])
    sd = synth.seeded_state_dict(VideoUNet(**cfg), p["weight_seed"])
    noise, c, uc, x8, ts, ctx, y = long_inputs()
    ioi = torch.zeros(2, T)
    _close(stored_grid(O.unet_forward(sd, cfg, x8, ts, ctx, y, T, ioi)), GOLDEN["unet_out"])
    net = lambda x, t, ca, v: O.unet_forward(sd, cfg, x, t, ca, v, T, ioi)
    _close(stored_grid(O.sample_euler_edm(net, noise.clone(), c, uc, LONG["steps"], T, p["min_scale"], p["max_scale"], p["sigma_max"])), GOLDEN["sample_z"])


def test_chunked_decode_T40():
    cfg = synth.decoder_config(TINY["vae_ch"])
    sd = synth.seeded_state_dict(VideoDecoder(**cfg), TINY["weight_seed"] + 1)
    _close(stored_grid(O.decode_first_stage(sd, cfg, long_decoder_latents(), 1.0, LONG["decoding_t"])), GOLDEN["dec_out"])
