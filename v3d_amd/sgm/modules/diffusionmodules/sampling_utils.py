"""Host-side sigma arithmetic of the samplers (reference: sgm/modules/diffusionmodules/sampling_utils.py:7-31).

The reference evaluates these on device tensors (get_ancestral_step) or with scipy quadrature (linear_multistep_coeff); the schedule
is a host list here, so they take and return Python floats and the sampler loop never waits on the device.
"""
from __future__ import annotations

import math
from typing import Sequence, Tuple

import numpy as np


def linear_multistep_coeff(order: int, t: Sequence[float], i: int, j: int) -> float:
    """Integral over [t[i], t[i+1]] of the Lagrange basis polynomial j on the nodes t[i], t[i-1], ..., t[i-order+1].  The integrand has
    degree order - 1, so Gauss-Legendre with ceil(order / 2) points is exact (two points for the default order 4); the reference's
    integrate.quad(epsrel=1e-4) approximates the same number."""
    if order - 1 > i:
        raise ValueError(f"Order {order} too high for step {i}")
    a, b = float(t[i]), float(t[i + 1])
    nodes, weights = np.polynomial.legendre.leggauss(max(1, (order + 1) // 2))
    mid, half = 0.5 * (a + b), 0.5 * (b - a)
    total = 0.0
    for xn, w in zip(nodes.tolist(), weights.tolist()):
        tau = mid + half * xn
        prod = 1.0
        for k in range(order):
            if k != j:
                prod *= (tau - float(t[i - k])) / (float(t[i - j]) - float(t[i - k]))
        total += w * prod
    return total * half


def get_ancestral_step(sigma_from: float, sigma_to: float, eta: float = 1.0) -> Tuple[float, float]:
    """(sigma_down, sigma_up) of an ancestral step from sigma_from to sigma_to."""
    if not eta:
        return sigma_to, 0.0
    sigma_up = min(sigma_to, eta * math.sqrt(sigma_to ** 2 * (sigma_from ** 2 - sigma_to ** 2) / sigma_from ** 2))
    sigma_down = math.sqrt(max(sigma_to ** 2 - sigma_up ** 2, 0.0))
    return sigma_down, sigma_up
