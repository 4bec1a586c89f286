"""The numpy restatement of the sampler noise (tests/philox_ref.py) against the published Philox4x32-10 known-answer vectors (Random123,
kat_vectors: philox4x32 10 rounds), and the shape of the Gaussian it makes.  No GPU."""
import numpy as np
import pytest

from philox_ref import global_index, philox4x32_10, randn_flat, randn_like

KAT = [
    ((0x00000000, 0x00000000, 0x00000000, 0x00000000), (0x00000000, 0x00000000), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
    ((0xffffffff, 0xffffffff, 0xffffffff, 0xffffffff), (0xffffffff, 0xffffffff), (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)),
]


@pytest.mark.parametrize("ctr,key,expect", KAT)
def test_philox4x32_10_known_answers(ctr, key, expect):
    out = philox4x32_10(*ctr, *key)
    assert tuple(int(v) for v in out) == expect


def test_vectorised_equals_scalar():
    ctr = np.array([0, 1, 0xffffffff, 12345], dtype=np.uint64)
    vec = philox4x32_10(ctr, ctr ^ 0x5a5a5a5a, ctr + 7, ctr * 3, 0xdeadbeef, 0x01234567)
    for i, c in enumerate(ctr.tolist()):
        one = philox4x32_10(c, c ^ 0x5a5a5a5a, (c + 7) & 0xffffffff, (c * 3) & 0xffffffff, 0xdeadbeef, 0x01234567)
        assert tuple(int(v) for v in one) == tuple(int(v[i]) for v in vec)


def test_lanes_follow_the_spec():
    """lanes 0..3 of group q are Box-Muller pairs of (r0, r1) and (r2, r3) of Philox(counter (q lo, q hi, call, 0), key (seed lo, seed hi))."""
    seed, call, q = (7 << 32) | 99, 5, (3 << 32) | 17
    r = philox4x32_10(q & 0xffffffff, q >> 32, call, 0, seed & 0xffffffff, seed >> 32)
    u = [((int(v) >> 8) + 0.5) * 2.0 ** -24 for v in r]
    z = randn_flat(seed, call, np.arange(4 * q, 4 * q + 4, dtype=np.uint64))
    rho0, rho2 = np.sqrt(-2 * np.log(u[0])), np.sqrt(-2 * np.log(u[2]))
    want = [rho0 * np.cos(2 * np.pi * u[1]), rho0 * np.sin(2 * np.pi * u[1]), rho2 * np.cos(2 * np.pi * u[3]), rho2 * np.sin(2 * np.pi * u[3])]
    np.testing.assert_allclose(z, want, rtol=0, atol=1e-6)


def test_shards_tile_the_unsharded_tensor():
    B, T, E = 2, 5, 12
    full = randn_like((B * T, E), seed=1234, call=3)
    parts = []
    for t0, tl in ((0, 2), (2, 2), (4, 1)):
        parts.append(randn_like((B * tl, E), seed=1234, call=3, t0=t0, T_local=tl, T_global=T).reshape(B, tl, E))
    np.testing.assert_array_equal(np.concatenate(parts, axis=1).reshape(B * T, E), full)
    assert global_index(B * 2, E, 2, 2, T)[0] == 2 * E


def test_gaussian_moments():
    z = randn_flat(42, 0, np.arange(1 << 20, dtype=np.uint64))
    assert abs(z.mean()) < 5e-3 and abs(z.var() - 1) < 5e-3
    assert abs(np.mean(z ** 4) - 3) < 3e-2
    z1 = randn_flat(42, 1, np.arange(1 << 20, dtype=np.uint64))
    assert abs(np.mean(z * z1)) < 5e-3                  # another call: independent numbers
    assert not np.array_equal(z, randn_flat(43, 0, np.arange(1 << 20, dtype=np.uint64)))
