"""TEST INFRASTRUCTURE — generate tests/golden/v3d_long.pt by running the REFERENCE's own modules at 40 frames (past the 32-frame tile).

Run in the build container only (needs the reference checkout, see oracle/ref_import.py):   python tools/gen_golden_long.py
Same tiny network, weights, seeds and CPU deviations as oracle/gen_golden.py, at T = 40 frames and 16 x 32 latents:
  unet_out   one VideoUNet evaluation of the guided batch [uc ; c] (80 images)
  sample_z   a 3-step EulerEDMSampler x LinearPredictionGuider(num_frames=40) rollout over the same network
  dec_out    a VideoDecoder decode of 40 latent frames (4 x 4) in chunks of decoding_t = 24 frames (24 + 16), the chunk loop of
             DiffusionEngine.decode_first_stage (video_diffusion.py) with en_and_decode_n_samples_a_time = decoding_t, scale factor 1
Only outputs are stored, on every second row and fourth column (long_orbit.stored_grid); inputs and weights are regenerated from seeds
(tests/long_orbit.py).
"""
from __future__ import annotations

import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "tests")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

from long_orbit import LONG, chunked_decode, long_decoder_latents, long_inputs, stored_grid  # noqa: E402
from oracle import ref_import  # noqa: E402
from oracle.gen_golden import TINY  # noqa: E402
from v3d_amd import synth  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "v3d_long.pt")


@torch.no_grad()
def main():
    torch.set_grad_enabled(False)
    m = ref_import.load()
    p = TINY
    T = LONG["T"]
    out = {"params": dict(LONG)}
    net = m["video_model"].VideoUNet(**synth.unet_config(p["model_channels"], attn_type="softmax")).eval()
    net.load_state_dict(synth.seeded_state_dict(net, p["weight_seed"]), strict=True)
    noise, c, uc, x8, timesteps, context, y = long_inputs()
    ioi = torch.zeros(2, T)
    out["unet_out"] = stored_grid(net(x8, timesteps, context=context, y=y, num_video_frames=T, image_only_indicator=ioi))

    sampler = m["sampling"].EulerEDMSampler(
        discretization_config={"target": "sgm.modules.diffusionmodules.discretizer.EDMDiscretization", "params": {"sigma_max": p["sigma_max"]}},
        num_steps=LONG["steps"],
        guider_config={"target": "sgm.modules.diffusionmodules.guiders.LinearPredictionGuider",
                       "params": {"max_scale": p["max_scale"], "min_scale": p["min_scale"], "num_frames": T}},
        device="cpu")
    denoiser = m["denoiser"].Denoiser({"target": "sgm.modules.diffusionmodules.denoiser_scaling.VScalingWithEDMcNoise"})
    wrapped = m["wrappers"].OpenAIWrapper(net)
    extra = {"image_only_indicator": ioi, "num_video_frames": T}
    out["sample_z"] = stored_grid(sampler(lambda inp, sigma, cc: denoiser(wrapped, inp, sigma, cc, **extra), noise.clone(), cond=c, uc=uc))

    dec = m["temporal_ae"].VideoDecoder(**synth.decoder_config(p["vae_ch"])).eval()
    dec.load_state_dict(synth.seeded_state_dict(dec, p["weight_seed"] + 1), strict=True)
    out["dec_out"] = stored_grid(chunked_decode(dec, long_decoder_latents(), LONG["decoding_t"]))

    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    torch.save(out, OUT)
    for k, v in out.items():
        if torch.is_tensor(v):
            print(f"{k:10s} {tuple(v.shape)} mean|x|={v.abs().mean():.4f} max|x|={v.abs().max():.4f}")
    print("wrote", OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
