"""TEST INFRASTRUCTURE — numpy restatement of the counter-based Gaussian noise of v3d_randn_add (spec: v3d_amd/csrc/noise.hip).

Vectorised over uint64 arrays.  Shared by tools/gen_golden_samplers.py (it replaces the reference samplers' `noise_sampler` with it) and
the tests (the emulated backend's randn_add, the GPU kernel's checker).  Pinned to the Random123 known-answer vectors in
tests/test_philox_ref.py.
"""
from __future__ import annotations

import numpy as np

M0, M1 = 0xD2511F53, 0xCD9E8D57
W0, W1 = 0x9E3779B9, 0xBB67AE85
_MASK = np.uint64(0xFFFFFFFF)


def philox4x32_10(c0, c1, c2, c3, k0, k1):
    """Philox4x32-10 of counters (c0, c1, c2, c3) under key (k0, k1); arrays / scalars of 32-bit values, returns four uint32 arrays."""
    c = [np.asarray(v, dtype=np.uint64) & _MASK for v in (c0, c1, c2, c3)]
    k0, k1 = np.uint64(int(k0) & 0xFFFFFFFF), np.uint64(int(k1) & 0xFFFFFFFF)
    for r in range(10):
        if r:
            k0, k1 = (k0 + np.uint64(W0)) & _MASK, (k1 + np.uint64(W1)) & _MASK
        p0 = c[0] * np.uint64(M0)           # < 2^64: exact in uint64
        p1 = c[2] * np.uint64(M1)
        hi0, lo0 = p0 >> np.uint64(32), p0 & _MASK
        hi1, lo1 = p1 >> np.uint64(32), p1 & _MASK
        c = [hi1 ^ c[1] ^ k0, lo1, hi0 ^ c[3] ^ k1, lo0]
    return tuple(v.astype(np.uint32) for v in c)


def _unit_open(r):
    """u(r) = ((r >> 8) + 0.5) * 2^-24 in fp32 arithmetic (the kernel's rounding of the + 0.5 above 2^23 included)."""
    return ((r >> np.uint32(8)).astype(np.float32) + np.float32(0.5)) * np.float32(2.0 ** -24)


def randn_flat(seed: int, call: int, g) -> np.ndarray:
    """N(seed, call, g) for an array of global flat element indices g (float64)."""
    g = np.asarray(g, dtype=np.uint64)
    q, lane = g >> np.uint64(2), g & np.uint64(3)
    r0, r1, r2, r3 = philox4x32_10(q & _MASK, q >> np.uint64(32), np.full_like(q, int(call) & 0xFFFFFFFF), np.zeros_like(q),
                                   int(seed) & 0xFFFFFFFF, (int(seed) >> 32) & 0xFFFFFFFF)
    lo = lane < 2
    a = np.where(lo, r0, r2)
    b = np.where(lo, r1, r3)
    rho = np.sqrt(-2.0 * np.log(_unit_open(a).astype(np.float64)))
    ang = 2.0 * np.pi * _unit_open(b).astype(np.float64)
    return rho * np.where(lane & np.uint64(1), np.sin(ang), np.cos(ang))


def global_index(rows: int, row_elems: int, t0: int = 0, T_local=None, T_global=None) -> np.ndarray:
    """Global flat indices of a local [(b T_local), row_elems] block placed at frame t0 of the unsharded [(b T_global), row_elems] tensor."""
    T_local = rows if T_local is None else T_local
    T_global = T_local if T_global is None else T_global
    r = np.arange(rows, dtype=np.int64)
    grow = (r // T_local) * T_global + t0 + r % T_local
    return (grow[:, None] * row_elems + np.arange(row_elems, dtype=np.int64)[None, :]).reshape(-1).astype(np.uint64)


def randn_like(shape, seed: int, call: int, t0: int = 0, T_local=None, T_global=None) -> np.ndarray:
    """Noise of a tensor of `shape` (rows = frames), float64."""
    rows = int(shape[0])
    row_elems = int(np.prod(shape[1:])) if len(shape) > 1 else 1
    return randn_flat(seed, call, global_index(rows, row_elems, t0, T_local, T_global)).reshape(shape)
