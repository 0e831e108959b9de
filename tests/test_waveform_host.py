"""Transmit waveform on the host (no GPU): rts_waveform_eval against an independent numpy restatement of the envelope defined in
include/rts_amd.h (RtsWaveform), and the validation of malformed descriptors."""
import ctypes as C
import math

import numpy as np
import pytest


def h_ref(u, L):
    """h_L(u), vectorised: sample-and-hold for L = 1, Blackman-windowed sinc on |u| < L/2 otherwise, h_L(0) = 1"""
    u = np.asarray(u, np.float64)
    if L == 1:
        return ((u > -1.0) & (u <= 0.0)).astype(np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        sinc = np.sin(np.pi * u) / (np.pi * u)
    w = 0.42 + 0.5 * np.cos(2 * np.pi * u / L) + 0.08 * np.cos(4 * np.pi * u / L)
    out = np.where(np.abs(u) < L / 2, sinc * w, 0.0)
    return np.where(u == 0.0, 1.0, out)


def envelope_ref(s, L, x):
    """s(x) = sum over ALL m of s[m] h_L(x - m)"""
    m = np.arange(len(s), dtype=np.float64)
    return (h_ref(np.asarray(x, np.float64)[:, None] - m[None, :], L) * np.asarray(s)[None, :]).sum(axis=1)


def random_waveform(rng, n):
    return rng.standard_normal(n) + 1j * rng.standard_normal(n)


@pytest.mark.parametrize("L", [1, 2, 8, 16, 64])
def test_eval_against_restatement(rts, L):
    rng = np.random.default_rng(100 + L)
    for n in (1, 5, 37, 300):
        s = random_waveform(rng, n)
        w = rts.Waveform(s, L)
        x = np.concatenate([rng.uniform(-L / 2 - 3, n + L / 2 + 3, 400),                  # negative ones and ones past the end
                            rng.uniform(-1.0, 1.0, 50), n - 1 + rng.uniform(0.0, 1.0, 20)])
        got = rts.waveform_eval(w, x)
        want = envelope_ref(s, L, x)
        np.testing.assert_allclose(got, want, rtol=1e-12, atol=1e-13 * np.abs(s).max())
        far = rts.waveform_eval(w, [-L / 2 - 1.0, -1e300, n + L / 2 + 0.5, 1e300, math.inf, -math.inf, math.nan])
        assert np.array_equal(far, np.zeros(7, np.complex128))


@pytest.mark.parametrize("L", [1, 2, 8, 16, 64])
def test_integer_positions_are_the_samples_bit_for_bit(rts, L):
    rng = np.random.default_rng(7 + L)
    s = random_waveform(rng, 64)
    got = rts.waveform_eval(rts.Waveform(s, L), np.arange(64, dtype=np.float64))
    assert np.array_equal(got.view(np.float64), s.view(np.float64))
    if L > 1:
        outside = rts.waveform_eval(rts.Waveform(s, L), np.array([-1.0, -2.0, 64.0, 65.0]))
        assert np.array_equal(outside, np.zeros(4, np.complex128))           # sinpi: every other integer offset weighs exactly 0


def test_sample_and_hold_picks_the_cube_bin(rts):
    """L = 1: s(x) = s[ceil(x)] -- output sample floor(d) + m of a start d reads sample m, the bin rts_cube_accumulate picks"""
    s = np.array([1 + 2j, 3 - 1j, -0.5 + 0.25j])
    got = rts.waveform_eval(rts.Waveform(s, 1), [-0.999, -0.5, 0.0, 0.25, 1.0, 1.75, 2.0, 2.001, -1.0])
    assert np.array_equal(got, [s[0], s[0], s[0], s[1], s[1], s[2], s[2], 0, 0])


def test_lfm_helper(rts):
    w = rts.Waveform.lfm(256, 0.5)
    assert w.taps == 16 and len(w.samples) == 256
    np.testing.assert_allclose(np.abs(w.samples), 1.0, rtol=1e-15)
    inst = np.diff(np.unwrap(np.angle(w.samples))) / (2 * np.pi)          # instantaneous frequency sweeps [-b/2, b/2] cycles per sample
    assert abs(inst[0] + 0.25) < 0.01 and abs(inst[-1] - 0.25) < 0.01


def test_malformed_descriptors_are_rejected(rts):
    from rts_amd import _lib as L
    lib = L.lib()
    ok = np.ascontiguousarray([1.0, 0.0, 0.5, -0.5])
    x = np.zeros(1); out = np.zeros(2)

    def desc(samples=ok, n=2, taps=1, reserved=(0, 0)):
        d = L.RtsWaveform()
        d.samples = samples.ctypes.data_as(C.c_void_p) if samples is not None else None
        d.n_samples, d.taps = n, taps
        d.reserved[0], d.reserved[1] = reserved
        return d

    assert lib.rts_waveform_eval(C.byref(desc()), x.ctypes.data_as(C.c_void_p), 1, out.ctypes.data_as(C.c_void_p)) == L.RTS_OK
    big = np.zeros(2 * 4097)
    cases = {
        "no samples": desc(n=0),
        "too many samples": desc(samples=big, n=4097),
        "null samples": desc(samples=None),
        "nan sample": desc(samples=np.ascontiguousarray([1.0, 0.0, math.nan, 0.0])),
        "inf sample": desc(samples=np.ascontiguousarray([1.0, -math.inf, 0.0, 0.0])),
        "taps 0": desc(taps=0),
        "taps 3": desc(taps=3),
        "taps 17": desc(taps=17),
        "taps 66": desc(taps=66),
        "reserved 0": desc(reserved=(1, 0)),
        "reserved 1": desc(reserved=(0, 5)),
    }
    for name, d in cases.items():
        rc = lib.rts_waveform_eval(C.byref(d), x.ctypes.data_as(C.c_void_p), 1, out.ctypes.data_as(C.c_void_p))
        assert rc == L.RTS_ERR_INVALID, name
        assert L.lib().rts_last_error(), name
    assert lib.rts_waveform_eval(None, x.ctypes.data_as(C.c_void_p), 1, out.ctypes.data_as(C.c_void_p)) == L.RTS_ERR_INVALID
    assert lib.rts_waveform_eval(C.byref(desc()), None, 1, None) == L.RTS_ERR_INVALID
    # the limits themselves are accepted
    full = np.zeros(2 * 4096); full[0] = 1.0
    for d in (desc(samples=full, n=4096, taps=64), desc(taps=2)):
        assert lib.rts_waveform_eval(C.byref(d), x.ctypes.data_as(C.c_void_p), 1, out.ctypes.data_as(C.c_void_p)) == L.RTS_OK
    with pytest.raises(L.RtsError):
        rts.waveform_eval(rts.Waveform([1.0], 5), [0.0])
