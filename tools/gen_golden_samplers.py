"""TEST INFRASTRUCTURE — generate tests/golden/v3d_samplers.pt by running the REFERENCE's own ancestral / DPM++ / linear-multistep samplers.

Run in the build container only (needs the reference checkout, see oracle/ref_import.py):   python tools/gen_golden_samplers.py
Same tiny network, weights, inputs, guider (LinearPredictionGuider) and CPU deviations as oracle/gen_golden.py, 6 steps.  The ancestral
samplers' `noise_sampler` (torch.randn_like in the reference) is replaced by the numpy restatement of the device noise (tests/philox_ref.py)
with a fixed seed and a draw counter that starts at 0 per run and counts its calls - one per step, so draw i is step i's, as in
v3d_amd's samplers.  Stored: the final latents and the denoiser call count of each sampler, the seed and the step count.
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
from oracle.gen_golden import TINY, tiny_unet_inputs  # noqa: E402
from philox_ref import randn_like  # noqa: E402
from v3d_amd import synth  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "v3d_samplers.pt")
SEED = 1234
STEPS = 6
SAMPLERS = {                       # fixture key -> (reference class, constructor keywords)
    "euler_ancestral": ("EulerAncestralSampler", {"eta": 1.0}),
    "dpmpp2s_ancestral": ("DPMPP2SAncestralSampler", {"eta": 1.0}),
    "dpmpp2m": ("DPMPP2MSampler", {}),
    "lms": ("LinearMultistepSampler", {"order": 4}),
}


class PhiloxNoise:
    """noise_sampler(x): the device generator's numbers for the whole (unsharded) tensor x, draw index = number of earlier calls."""

    def __init__(self, seed: int):
        self.seed, self.calls = seed, 0

    def __call__(self, x):
        z = torch.from_numpy(randn_like(tuple(x.shape), self.seed, self.calls)).to(x.dtype)
        self.calls += 1
        return z


@torch.no_grad()
def main():
    torch.set_grad_enabled(False)
    m = ref_import.load()
    p = TINY
    T, H, W = p["T"], p["H"], p["W"]
    net = m["video_model"].VideoUNet(**synth.unet_config(p["model_channels"], attn_type="softmax")).eval()
    net.load_state_dict(synth.seeded_state_dict(net, p["weight_seed"]), strict=True)
    noise, c, uc, *_ = tiny_unet_inputs(T, H, W, p["seed"])
    denoiser = m["denoiser"].Denoiser({"target": "sgm.modules.diffusionmodules.denoiser_scaling.VScalingWithEDMcNoise"})
    wrapped = m["wrappers"].OpenAIWrapper(net)
    extra = {"image_only_indicator": torch.zeros(2, T), "num_video_frames": T}
    calls = [0]

    def den(inp, sigma, cc):
        calls[0] += 1
        return denoiser(wrapped, inp, sigma, cc, **extra)

    disc = {"target": "sgm.modules.diffusionmodules.discretizer.EDMDiscretization", "params": {"sigma_max": p["sigma_max"]}}
    guider = {"target": "sgm.modules.diffusionmodules.guiders.LinearPredictionGuider",
              "params": {"max_scale": p["max_scale"], "min_scale": p["min_scale"], "num_frames": T}}
    out = {"seed": SEED, "steps": STEPS, "z": {}, "calls": {}}
    for key, (cls, kw) in SAMPLERS.items():
        sampler = getattr(m["sampling"], cls)(discretization_config=disc, num_steps=STEPS, guider_config=guider, device="cpu", **kw)
        if hasattr(sampler, "noise_sampler"):
            sampler.noise_sampler = PhiloxNoise(SEED)
        calls[0] = 0
        z = sampler(den, noise.clone(), cond=c, uc=uc).clone()
        out["z"][key], out["calls"][key] = z, calls[0]
        print(f"{key:18s} {tuple(z.shape)} calls={calls[0]} mean|z|={z.abs().mean():.5f} max|z|={z.abs().max():.5f}")
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    torch.save(out, OUT)
    print("wrote", OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
