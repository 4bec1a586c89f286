"""TEST INFRASTRUCTURE — generate tests/golden/v3d_res.pt by running the REFERENCE's own modules at latent sizes whose token counts are not
multiples of 8 (images of any 64-px multiple).

Run in the build container only (needs the reference checkout, see oracle/ref_import.py):   python tools/gen_golden_res.py
Same tiny network, weights, seeds and CPU deviations as oracle/gen_golden.py, at T = 3 frames:
  unet_out_24x40  one VideoUNet evaluation of the guided batch [uc ; c] at 24 x 40 latents (15 tokens at the deepest level, 60 at the next)
  unet_out_72x72  the same at 72 x 72 latents (81 / 324 tokens: the shape of a 576 x 576 image)
  sample_z        a 3-step EulerEDMSampler x LinearPredictionGuider rollout over the same network at 24 x 40 latents
Only outputs are stored, on every second row and fourth column (long_orbit.stored_grid); inputs and weights are regenerated from seeds
(tests/res_shapes.py).
"""
from __future__ import annotations

import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "tests")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

from oracle import ref_import  # noqa: E402
from oracle.gen_golden import TINY  # noqa: E402
from res_shapes import RES, res_inputs, stored_grid, unet_key  # noqa: E402
from v3d_amd import synth  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "v3d_res.pt")


@torch.no_grad()
def main():
    torch.set_grad_enabled(False)
    m = ref_import.load()
    p = TINY
    T = RES["T"]
    out = {"params": dict(RES)}
    net = m["video_model"].VideoUNet(**synth.unet_config(p["model_channels"], attn_type="softmax")).eval()
    net.load_state_dict(synth.seeded_state_dict(net, p["weight_seed"]), strict=True)
    ioi = torch.zeros(2, T)
    for H, W in RES["unet_hw"]:
        _, _, _, x8, timesteps, context, y = res_inputs(H, W)
        out[unet_key(H, W)] = stored_grid(net(x8, timesteps, context=context, y=y, num_video_frames=T, image_only_indicator=ioi))

    sampler = m["sampling"].EulerEDMSampler(
        discretization_config={"target": "sgm.modules.diffusionmodules.discretizer.EDMDiscretization", "params": {"sigma_max": p["sigma_max"]}},
        num_steps=RES["steps"],
        guider_config={"target": "sgm.modules.diffusionmodules.guiders.LinearPredictionGuider",
                       "params": {"max_scale": p["max_scale"], "min_scale": p["min_scale"], "num_frames": T}},
        device="cpu")
    denoiser = m["denoiser"].Denoiser({"target": "sgm.modules.diffusionmodules.denoiser_scaling.VScalingWithEDMcNoise"})
    wrapped = m["wrappers"].OpenAIWrapper(net)
    extra = {"image_only_indicator": ioi, "num_video_frames": T}
    noise, c, uc, *_ = res_inputs(*RES["sample_hw"])
    out["sample_z"] = stored_grid(sampler(lambda inp, sigma, cc: denoiser(wrapped, inp, sigma, cc, **extra), noise.clone(), cond=c, uc=uc))

    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    torch.save(out, OUT)
    for k, v in out.items():
        if torch.is_tensor(v):
            print(f"{k:15s} {tuple(v.shape)} mean|x|={v.abs().mean():.4f} max|x|={v.abs().max():.4f}")
    print("wrote", OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
