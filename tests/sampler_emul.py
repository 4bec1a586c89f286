"""TEST INFRASTRUCTURE — the emulated backend (oracle/ops_emul.py) plus the two sampler-loop ops of csrc/noise.hip: v3d_randn_add from the numpy
restatement of its noise (tests/philox_ref.py), v3d_lincomb_f32 as fp32 torch."""
from __future__ import annotations

import torch

from oracle.ops_emul import EmulOps
from philox_ref import randn_like


def randn_ref(shape, seed, call, t0=0, T_local=None, T_global=None, device="cpu"):
    """The noise v3d_randn_add adds, as an fp32 tensor."""
    return torch.from_numpy(randn_like(tuple(shape), seed, call, t0, T_local, T_global)).float().to(device)


class SamplerEmulOps(EmulOps):
    def randn_add(self, x, scale, seed, call, *, t0=0, T_local=None, T_global=None, out=None):
        ref = x if x is not None else out
        r = float(scale) * randn_ref(ref.shape, seed, call, t0, T_local, T_global, ref.device)
        if x is not None:
            r = x.float() + r
        if out is not None:
            out.copy_(r)
            return out
        return r

    def lincomb_f32(self, srcs, coefs, out=None):
        acc = srcs[0].float() * float(coefs[0])
        for t, c in zip(srcs[1:], coefs[1:]):
            acc = acc + t.float() * float(c)
        if out is not None:
            out.copy_(acc)
            return out
        return acc
