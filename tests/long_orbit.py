"""Seeded inputs of the 40-frame fixture tests/golden/v3d_long.pt (tools/gen_golden_long.py): the tiny network of tests/golden/v3d_tiny.pt at
T = 40 frames, past the 32-frame tile of the short temporal-attention kernels.  Latents are 16 x 32, not 16 x 16: v3d_attn_spatial takes token
counts that are multiples of 8, and the U-Net's deepest level of a 16 x 16 latent is 2 x 2 (a limit of the spatial kernel at any frame count)."""
from __future__ import annotations

import math

import torch

from oracle.gen_golden import TINY, tiny_unet_inputs

LONG = dict(T=40, H=16, W=32, steps=3, decoding_t=24, dec_hw=4)


def stored_grid(x):
    """The pixels tests/golden/v3d_long.pt keeps of an output [N, C, H, W]: every second row, every fourth column (all images, frames and
    channels), an eighth of the bytes - the file stays small while every frame of the orbit is pinned."""
    return x[..., ::2, ::4].contiguous()


def long_inputs():
    """(noise, c, uc, x8, timesteps, context, y) of the guided batch [uc ; c] at T = 40, 16 x 32 latents."""
    return tiny_unet_inputs(LONG["T"], LONG["H"], LONG["W"], TINY["seed"])


def long_decoder_latents(device="cpu"):
    g = torch.Generator().manual_seed(TINY["seed"] + 6)
    return torch.randn(LONG["T"], 4, LONG["dec_hw"], LONG["dec_hw"], generator=g).to(device)


def chunked_decode(decoder, z, decoding_t):
    """DiffusionEngine.decode_first_stage's loop (en_and_decode_n_samples_a_time = decoding_t, scale factor 1): chunks of decoding_t frames,
    timesteps = the chunk's length."""
    outs = []
    for n in range(math.ceil(z.shape[0] / decoding_t)):
        zc = z[n * decoding_t:(n + 1) * decoding_t]
        outs.append(decoder(zc, timesteps=len(zc)))
    return torch.cat(outs, dim=0)
