"""Seeded inputs of the resolution fixture tests/golden/v3d_res.pt (tools/gen_golden_res.py): the tiny network of tests/golden/v3d_tiny.pt at
latent sizes whose U-Net levels hold token counts that are not multiples of 8.  24 x 40 latents (a 192 x 320 image) have 3 x 5 = 15 tokens at the
deepest level and 60 at the next; 72 x 72 (576 x 576) has 81 and 324."""
from __future__ import annotations

from long_orbit import stored_grid  # noqa: F401  (the same subsampled grid as the 40-frame fixture)
from oracle.gen_golden import TINY, tiny_unet_inputs

RES = dict(T=TINY["T"], unet_hw=((24, 40), (72, 72)), sample_hw=(24, 40), steps=3)


def unet_key(H, W):
    return f"unet_out_{H}x{W}"


def res_inputs(H, W):
    """(noise, c, uc, x8, timesteps, context, y) of the guided batch [uc ; c] at T = 3 frames, H x W latents."""
    return tiny_unet_inputs(RES["T"], H, W, TINY["seed"])
