"""Receiver noise on the host (no GPU): an independent Python restatement of Philox4x32-10 against the Random123 known answers,
rts_noise_eval against that restatement plus Box-Muller (include/rts_amd.h: rts_cube_add_noise), the statistics of the noise
over 10^6 samples, and argument validation."""
import ctypes as C
import math

import numpy as np
import pytest

M32 = 0xFFFFFFFF


def philox4x32_10(ctr, key):
    """Philox4x32-10 in Python integers: counter (c0, c1, c2, c3), key (k0, k1) -> (x0, x1, x2, x3)"""
    c0, c1, c2, c3 = ctr
    k0, k1 = key
    for r in range(10):
        if r:
            k0 = (k0 + 0x9E3779B9) & M32
            k1 = (k1 + 0xBB67AE85) & M32
        p0 = 0xD2511F53 * c0
        p1 = 0xCD9E8D57 * c2
        c0, c1, c2, c3 = (p1 >> 32) ^ c1 ^ k0, p1 & M32, (p0 >> 32) ^ c3 ^ k1, p0 & M32
    return c0, c1, c2, c3


def noise_ref(seed, i, noise_power):
    """the sample of flat index i: Philox counter (lo32(i), hi32(i), 0, 0), key (lo32(seed), hi32(seed)), then Box-Muller"""
    x0, x1, x2, x3 = philox4x32_10((i & M32, i >> 32, 0, 0), (seed & M32, seed >> 32))
    a = ((x0 << 32) | x1) >> 11
    b = ((x2 << 32) | x3) >> 11
    u1 = (a + 1) * 2.0 ** -53
    u2 = b * 2.0 ** -53
    r = math.sqrt(-2.0 * math.log(u1))
    s = math.sqrt(noise_power / 2.0)
    return complex(s * r * math.cos(2 * math.pi * u2), s * r * math.sin(2 * math.pi * u2))


@pytest.mark.parametrize("ctr,key,want", [
    ((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
    ((M32, M32, M32, M32), (M32, M32), (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)),
])
def test_philox_known_answers(ctr, key, want):
    assert philox4x32_10(ctr, key) == want


def test_eval_matches_the_restatement(rts):
    idx = [0, 1, 2, 12345, 2 ** 32 - 1, 2 ** 32, 2 ** 32 + 1, 2 ** 40 + 7, 2 ** 63, 2 ** 64 - 1]
    for seed in (0, 1, 0xDEADBEEF, 2 ** 32 + 5, 2 ** 64 - 1):
        for power in (1.0, 2.5e-3, 7.0e4):
            got = rts.noise_eval(seed, idx, power)
            want = np.array([noise_ref(seed, i, power) for i in idx])
            scale = math.sqrt(power)
            np.testing.assert_allclose(got.real, want.real, rtol=1e-13, atol=1e-13 * scale)
            np.testing.assert_allclose(got.imag, want.imag, rtol=1e-13, atol=1e-13 * scale)
    # a sample depends on its index and seed alone, not on the batch it is evaluated in
    a = rts.noise_eval(3, np.arange(100, dtype=np.uint64), 1.0)
    b = np.concatenate([rts.noise_eval(3, np.arange(0, 37, dtype=np.uint64), 1.0), rts.noise_eval(3, np.arange(37, 100, dtype=np.uint64), 1.0)])
    assert np.array_equal(a, b)
    assert not np.array_equal(a, rts.noise_eval(4, np.arange(100, dtype=np.uint64), 1.0))
    assert np.count_nonzero(rts.noise_eval(3, np.arange(100, dtype=np.uint64), 0.0)) == 0


def test_statistics_of_a_million_samples(rts):
    n, power = 1_000_000, 3.0
    z = rts.noise_eval(2024, np.arange(5_000_000, 5_000_000 + n, dtype=np.uint64), power)
    p = np.abs(z) ** 2
    # the mean of each component: standard error sqrt(power / 2 / n); five of them
    se = math.sqrt(power / 2 / n)
    assert abs(z.real.mean()) < 5 * se and abs(z.imag.mean()) < 5 * se
    # E|n|^2 = power: |n|^2 is exponential, standard deviation power, standard error power / sqrt(n)
    assert abs(p.mean() - power) < 5 * power / math.sqrt(n)
    # re and im uncorrelated: the sample correlation of independent samples has standard error 1 / sqrt(n)
    assert abs(np.corrcoef(z.real, z.imag)[0, 1]) < 5 / math.sqrt(n)
    # E|n|^4 / (E|n|^2)^2 = 2 for circular complex Gaussian noise (|n|^2 exponential: moments 1, 2, 6, 24 -> std of |n|^4 = sqrt(20))
    k = np.mean(p * p) / power ** 2
    assert abs(k - 2.0) < 5 * math.sqrt(20.0 / n)
    # Kolmogorov-Smirnov against 1 - exp(-x / power), at the 1 % bound 1.63 / sqrt(n)
    s = np.sort(p)
    cdf = -np.expm1(-s / power)
    i = np.arange(1, n + 1)
    d = max(np.max(i / n - cdf), np.max(cdf - (i - 1) / n))
    assert d < 1.63 / math.sqrt(n), d


def test_argument_validation(rts):
    from rts_amd import _lib as L
    lib = L.lib()
    idx = np.arange(4, dtype=np.uint64); out = np.zeros(8)
    for bad in (-1.0, math.nan, math.inf, -math.inf):
        assert lib.rts_noise_eval(1, idx.ctypes.data_as(C.c_void_p), 4, bad, out.ctypes.data_as(C.c_void_p)) == L.RTS_ERR_INVALID
        assert b"noise_power" in lib.rts_last_error()
    assert lib.rts_noise_eval(1, None, 4, 1.0, out.ctypes.data_as(C.c_void_p)) == L.RTS_ERR_INVALID
    assert lib.rts_noise_eval(1, idx.ctypes.data_as(C.c_void_p), 4, 1.0, None) == L.RTS_ERR_INVALID
    assert lib.rts_noise_eval(1, None, 0, 1.0, None) == L.RTS_OK
    with pytest.raises(L.RtsError):
        rts.noise_eval(1, [0, 1], -2.0)
