"""Samplers (reference: sgm/modules/diffusionmodules/sampling.py; sampling_utils.py): EDM (Euler, Heun), ancestral (Euler, DPM++ 2S),
DPM++ 2M and linear multistep.

Sampler state `x` stays fp32 on the device; every elementwise update is a HIP kernel from libv3d_hip.so.  The
sigma schedule lives on the host, so the loop issues no device->host sync (the reference's `sigmas[i]` compares
and `torch.sum(next_sigma)` checks each force one).  Every update of the ancestral / DPM++ samplers is the reference's
`m1 x - m2 D` rearranged into the Euler kernel: m1 x - m2 D = x + (s' - s)(x - D)/s with m1 = s'/s, m2 = s'/s - 1.

The ancestral samplers draw their noise on the device from a counter-based generator (v3d_randn_add): the numbers are a pure
function of (seed, step, element index in the unsharded tensor), so a frame-sharded run adds exactly the noise of the unsharded
run of the same seed.
"""
from __future__ import annotations

import math
from typing import Dict, Optional, Union

import torch

from ....ops import get_ops
from ...util import default, instantiate_from_config
from .sampling_utils import get_ancestral_step, linear_multistep_coeff

DEFAULT_GUIDER = {"target": "v3d_amd.sgm.modules.diffusionmodules.guiders.IdentityGuider"}


class BaseDiffusionSampler:
    def __init__(self, discretization_config: Dict, num_steps: Union[int, None] = None,
                 guider_config: Union[Dict, None] = None, verbose: bool = False, device: str = "cuda"):
        self.num_steps = num_steps
        self.discretization = instantiate_from_config(discretization_config)
        self.guider = instantiate_from_config(default(guider_config, DEFAULT_GUIDER))
        self.verbose = verbose
        self.device = device

    def prepare_sampling_loop(self, x, cond, uc=None, num_steps=None):
        sigmas = self.discretization(self.num_steps if num_steps is None else num_steps, device="cpu").float()
        uc = default(uc, cond)
        # x *= sqrt(1 + sigma_0^2), in place on the caller's tensor like the reference (sampling.py:50)
        get_ops().axpb_f32(x, float(torch.sqrt(1.0 + sigmas[0] ** 2.0)), 0.0, out=x)
        num_sigmas = len(sigmas)
        s_in = x.new_ones([x.shape[0]])
        return x, s_in, sigmas, num_sigmas, cond, uc

    def denoise(self, x, denoiser, sigma, cond, uc):
        denoised = denoiser(*self.guider.prepare_inputs(x, sigma, cond, uc))
        return self.guider(denoised, sigma)

    def get_sigma_gen(self, num_sigmas):
        gen = range(num_sigmas - 1)
        if self.verbose:
            from tqdm import tqdm
            print("#" * 30, " Sampling setting ", "#" * 30)
            print(f"Sampler: {self.__class__.__name__}")
            print(f"Discretization: {self.discretization.__class__.__name__}")
            print(f"Guider: {self.guider.__class__.__name__}")
            gen = tqdm(gen, total=num_sigmas, desc=f"Sampling with {self.__class__.__name__} for {num_sigmas} steps")
        return gen


class SingleStepDiffusionSampler(BaseDiffusionSampler):
    def sampler_step(self, sigma, next_sigma, denoiser, x, cond, uc, *args, **kwargs):
        raise NotImplementedError


class EDMSampler(SingleStepDiffusionSampler):
    def __init__(self, s_churn=0.0, s_tmin=0.0, s_tmax=float("inf"), s_noise=1.0, *args, **kwargs):
        super().__init__(*args, **kwargs)
        self.s_churn = s_churn
        self.s_tmin = s_tmin
        self.s_tmax = s_tmax
        self.s_noise = s_noise

    def sampler_step(self, sigma, next_sigma, denoiser, x, cond, uc=None, gamma=0.0):
        ops = get_ops()
        sigma_hat = sigma if gamma == 0.0 else ops.axpb_f32(sigma, gamma + 1.0, 0.0)
        if gamma > 0:
            # churn: x += eps * s_noise * sqrt(sigma_hat^2 - sigma^2)   (sampling.py:98-100); V3D_512 uses s_churn = 0
            eps = torch.randn_like(x) * self.s_noise
            x = x + eps * ((sigma_hat ** 2 - sigma ** 2) ** 0.5).reshape((-1,) + (1,) * (x.dim() - 1))
        denoised = self.denoise(x, denoiser, sigma_hat, cond, uc)
        # d = (x - denoised) / sigma_hat ; euler: x + (next_sigma - sigma_hat) d   — one fused kernel
        x = x.contiguous()
        denoised = denoised.contiguous()
        euler = ops.euler_step(x, denoised, sigma_hat, next_sigma)
        # reference signature (euler_step, x, d, dt, next_sigma, ...).  d and dt are never materialised: a sampler that needs them
        # (Heun) gets the tensors they are made of in `_step_ctx` and fuses its update into one kernel
        self._step_ctx = (denoised, sigma_hat)
        out = self.possible_correction_step(euler, x, None, None, next_sigma, denoiser, cond, uc)
        self._step_ctx = None
        return out

    def __call__(self, denoiser, x, cond, uc=None, num_steps=None):
        ops = get_ops()
        x, s_in, sigmas, num_sigmas, cond, uc = self.prepare_sampling_loop(x, cond, uc, num_steps)
        sig = [float(s) for s in sigmas]
        for i in self.get_sigma_gen(num_sigmas):
            gamma = min(self.s_churn / (num_sigmas - 1), 2 ** 0.5 - 1) if self.s_tmin <= sig[i] <= self.s_tmax else 0.0
            self._next_sigma_is_zero = sig[i + 1] < 1e-14 / max(1, x.shape[0])   # host copy of `torch.sum(next_sigma) < 1e-14`
            x = self.sampler_step(ops.axpb_f32(s_in, sig[i], 0.0), ops.axpb_f32(s_in, sig[i + 1], 0.0),
                                  denoiser, x, cond, uc, gamma)
        return x


class EulerEDMSampler(EDMSampler):
    def possible_correction_step(self, euler_step, x, d, dt, next_sigma, denoiser, cond, uc):
        return euler_step


class HeunEDMSampler(EDMSampler):
    """2nd-order correction (sampling.py:221-237): one more guided evaluation at (euler_step, next_sigma), then
    x + dt (d + d_new) / 2 where next_sigma > 0.  The "all noise levels are 0 -> skip the evaluation" test of the reference
    (`torch.sum(next_sigma) < 1e-14`, a device sync there) is decided on the host copy of the sigma schedule."""

    def possible_correction_step(self, euler_step, x, d, dt, next_sigma, denoiser, cond, uc):
        if getattr(self, "_next_sigma_is_zero", False):
            return euler_step
        denoised, sigma_hat = self._step_ctx
        denoised2 = self.denoise(euler_step, denoiser, next_sigma, cond, uc)
        return get_ops().heun_step(x, denoised, euler_step, denoised2.contiguous(), sigma_hat, next_sigma)


def _full(ref: torch.Tensor, value: float) -> torch.Tensor:
    """Per-sample sigma tensor shaped like `ref` holding `value` (0 * ref + value on the device)."""
    return get_ops().axpb_f32(ref, 0.0, float(value))


def _host(sigma) -> float:
    """Host value of a per-sample sigma (only for direct sampler_step calls outside the samplers' own loops: one sync)."""
    return float(sigma.reshape(-1)[0]) if isinstance(sigma, torch.Tensor) else float(sigma)


def _all_zero(value: float, n: int) -> bool:
    """Host copy of the reference's `torch.sum(sigma) < 1e-14` over n equal per-sample sigmas."""
    return value * max(1, n) < 1e-14


class AncestralSampler(SingleStepDiffusionSampler):
    """Reference sampling.py:136-172.  `noise_sampler` is the reference's hook: None (default) draws the noise on the device from
    `noise_seed` (v3d_randn_add); a callable x -> noise tensor is used as the reference uses it.  `noise_seed=None` draws a seed from
    torch's default CPU generator at the start of every call, so `torch.manual_seed` reproduces a run.  Step i uses draw index i."""

    def __init__(self, eta=1.0, s_noise=1.0, *args, noise_seed: Optional[int] = None, **kwargs):
        super().__init__(*args, **kwargs)
        self.eta = eta
        self.s_noise = s_noise
        self.noise_seed = noise_seed
        self.noise_sampler = None
        # (t0, T_local, T_global): where this sampler's frames sit in the unsharded sample (set by dist.local_sampler); None: x is all of it
        self.noise_frames = None
        self._host_sig = None
        self._seed = None
        self._call = 0

    def _begin_noise(self):
        self._seed = self.noise_seed if self.noise_seed is not None else draw_noise_seed()
        self._call = 0

    def _host_sigmas(self, sigma, next_sigma):
        return self._host_sig if self._host_sig is not None else (_host(sigma), _host(next_sigma))

    def ancestral_euler_step(self, x, denoised, sigma, sigma_down):
        return get_ops().euler_step(x.contiguous(), denoised.contiguous(), sigma, sigma_down)

    def ancestral_step(self, x, sigma, next_sigma, sigma_up):
        """x + noise * s_noise * sigma_up where next_sigma > 0 (sigma_up: host float).  Draw index = the step's (one draw per step, the
        last step's unused, as in the reference)."""
        ops = get_ops()
        if self._seed is None:          # (sampler_step called outside __call__)
            self._begin_noise()
        call = self._call
        self._call += 1
        scale = float(self.s_noise) * float(sigma_up)
        nonzero = self._host_sig[1] > 0.0 if self._host_sig is not None else bool((next_sigma > 0).all())
        if self.noise_sampler is not None:
            noise = self.noise_sampler(x)
            if not nonzero:
                return x
            return ops.lincomb_f32([x.contiguous(), noise.float().contiguous()], [1.0, scale])
        if not nonzero or scale == 0.0:
            return x
        t0, tl, tg = self.noise_frames if self.noise_frames is not None else (0, None, None)
        return ops.randn_add(x.contiguous(), scale, self._seed, call, t0=t0, T_local=tl, T_global=tg)

    def __call__(self, denoiser, x, cond, uc=None, num_steps=None):
        ops = get_ops()
        x, s_in, sigmas, num_sigmas, cond, uc = self.prepare_sampling_loop(x, cond, uc, num_steps)
        sig = [float(s) for s in sigmas]
        self._begin_noise()
        try:
            for i in self.get_sigma_gen(num_sigmas):
                self._host_sig = (sig[i], sig[i + 1])
                self._call = i
                x = self.sampler_step(ops.axpb_f32(s_in, sig[i], 0.0), ops.axpb_f32(s_in, sig[i + 1], 0.0), denoiser, x, cond, uc)
        finally:
            self._host_sig = None
        return x


def draw_noise_seed() -> int:
    """A 63-bit noise seed from torch's default CPU generator."""
    return int(torch.randint(0, 2 ** 63 - 1, (), dtype=torch.int64).item())


class EulerAncestralSampler(AncestralSampler):
    """Reference sampling.py:240-248."""

    def sampler_step(self, sigma, next_sigma, denoiser, x, cond, uc):
        s, s_next = self._host_sigmas(sigma, next_sigma)
        sigma_down, sigma_up = get_ancestral_step(s, s_next, eta=self.eta)
        denoised = self.denoise(x, denoiser, sigma, cond, uc)
        x = self.ancestral_euler_step(x, denoised, sigma, _full(sigma, sigma_down))
        return self.ancestral_step(x, sigma, next_sigma, sigma_up)


class DPMPP2SAncestralSampler(AncestralSampler):
    """Reference sampling.py:251-290.  With t = -log sigma, h = t(sigma_down) - t, s = t + h/2: the midpoint is the Euler step to
    to_sigma(s) = sqrt(sigma sigma_down), the update the Euler step from x to sigma_down with the midpoint's denoised.  sigma_down = 0
    (the last step) is the plain Euler step and saves the second evaluation."""

    def sampler_step(self, sigma, next_sigma, denoiser, x, cond, uc=None, **kwargs):
        s, s_next = self._host_sigmas(sigma, next_sigma)
        sigma_down, sigma_up = get_ancestral_step(s, s_next, eta=self.eta)
        denoised = self.denoise(x, denoiser, sigma, cond, uc)
        if _all_zero(sigma_down, x.shape[0]):
            x = self.ancestral_euler_step(x, denoised, sigma, _full(sigma, sigma_down))
        else:
            t, t_next = -math.log(s), -math.log(sigma_down)
            sigma_s = _full(sigma, math.exp(-(t + 0.5 * (t_next - t))))
            x2 = self.ancestral_euler_step(x, denoised, sigma, sigma_s)
            denoised2 = self.denoise(x2, denoiser, sigma_s, cond, uc)
            x = self.ancestral_euler_step(x, denoised2, sigma, _full(sigma, sigma_down))
        return self.ancestral_step(x, sigma, next_sigma, sigma_up)


class DPMPP2MSampler(BaseDiffusionSampler):
    """Reference sampling.py:293-360.  x_standard = Euler step to next_sigma; from the second step on the denoised estimate is
    extrapolated, D_d = (1 + 1/(2r)) D - 1/(2r) D_old with r = h_last / h.  next_sigma = 0 (the last step) gives x = D, which is what
    the reference's -log(0) = inf arithmetic yields there (to_sigma(inf) = 0, expm1(-inf) = -1)."""

    _host_sig = None

    def sampler_step(self, old_denoised, previous_sigma, sigma, next_sigma, denoiser, x, cond, uc=None):
        ops = get_ops()
        if self._host_sig is not None:
            s_prev, s, s_next = self._host_sig
        else:
            s_prev = None if previous_sigma is None else _host(previous_sigma)
            s, s_next = _host(sigma), _host(next_sigma)
        denoised = self.denoise(x, denoiser, sigma, cond, uc).contiguous()
        if _all_zero(s_next, x.shape[0]):
            return denoised, denoised
        x = x.contiguous()
        if old_denoised is None:
            return ops.euler_step(x, denoised, sigma, next_sigma), denoised
        h, h_last = math.log(s / s_next), math.log(s_prev / s)
        r = h_last / h
        denoised_d = ops.lincomb_f32([denoised, old_denoised], [1.0 + 1.0 / (2.0 * r), -1.0 / (2.0 * r)])
        return ops.euler_step(x, denoised_d, sigma, next_sigma), denoised

    def __call__(self, denoiser, x, cond, uc=None, num_steps=None, **kwargs):
        ops = get_ops()
        x, s_in, sigmas, num_sigmas, cond, uc = self.prepare_sampling_loop(x, cond, uc, num_steps)
        sig = [float(s) for s in sigmas]
        old_denoised = None
        try:
            for i in self.get_sigma_gen(num_sigmas):
                self._host_sig = (None if i == 0 else sig[i - 1], sig[i], sig[i + 1])
                x, old_denoised = self.sampler_step(old_denoised, None if i == 0 else ops.axpb_f32(s_in, sig[i - 1], 0.0),
                                                    ops.axpb_f32(s_in, sig[i], 0.0), ops.axpb_f32(s_in, sig[i + 1], 0.0),
                                                    denoiser, x, cond, uc=uc)
        finally:
            self._host_sig = None
        return x


class LinearMultistepSampler(BaseDiffusionSampler):
    """Reference sampling.py:175-211.  d_i = (x - D)/sigma_i goes into a ring of the last `order` derivatives (no concatenation per
    step); x += sum_j c_j d_{i-j} with the coefficients integrated on the host (sampling_utils.linear_multistep_coeff)."""

    def __init__(self, order=4, *args, **kwargs):
        super().__init__(*args, **kwargs)
        self.order = order

    def __call__(self, denoiser, x, cond, uc=None, num_steps=None, **kwargs):
        ops = get_ops()
        x, s_in, sigmas, num_sigmas, cond, uc = self.prepare_sampling_loop(x, cond, uc, num_steps)
        sig = [float(s) for s in sigmas]
        x = x.contiguous()
        ring = None
        for i in self.get_sigma_gen(num_sigmas):
            sigma = ops.axpb_f32(s_in, sig[i], 0.0)
            denoised = denoiser(*self.guider.prepare_inputs(x, sigma, cond, uc), **kwargs)
            denoised = self.guider(denoised, sigma).contiguous()
            if ring is None:
                ring = torch.empty((self.order,) + tuple(x.shape), dtype=torch.float32, device=x.device)
            ops.lincomb_f32([x, denoised], [1.0 / sig[i], -1.0 / sig[i]], out=ring[i % self.order])
            cur_order = min(i + 1, self.order)
            terms = [(linear_multistep_coeff(cur_order, sig, i, j), ring[(i - j) % self.order]) for j in range(cur_order)]
            for k in range(0, len(terms), 5):
                chunk = terms[k:k + 5]
                # the first update writes a new tensor (x is the caller's noise tensor up to here), later ones update x in place
                x = ops.lincomb_f32([x] + [d for _, d in chunk], [1.0] + [c for c, _ in chunk], out=x if i > 0 or k > 0 else None)
        return x
