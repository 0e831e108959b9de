"""The reference helpers of tests/cube_ref.py (used by test_gpu_cube_edges.py) tied to independent ground, without a GPU: the
library's host export of the waveform envelope, the numpy restatement of test_gpu_render.py on that file's own inputs, numpy's
FFT and correlation, and the closed form of test_oracle_kat.py::test_cube_definition_closed_form."""
import math

import numpy as np
import pytest

import cube_ref as R


def one(a, tau, f=0.0, rx=0):
    return [(rx, R.CLD(a), tau, f)]


@pytest.mark.parametrize("L", [1, 2, 16, 64])
def test_single_contribution_is_the_host_envelope(rts, L):
    """one contribution's row = a s(n - d), s(.) from rts_waveform_eval, also for starts before the cube (d < 0), starts past its
    end (d > n_bins), on-grid starts and d in (-1, 0)"""
    rng = np.random.default_rng(40 + L)
    M, n_bins, t0, dt = 23, 50, 3.0, 0.25
    s = rng.standard_normal(M) + 1j * rng.standard_normal(M)
    w = rts.Waveform(s, L)
    a = 0.75 - 1.5j
    seen = set()
    for d_want in (-0.5, -0.0009765625, 0.0, 0.375, -7.0, -7.25, -(M + L), 11.625, n_bins - 1.0, n_bins - 0.5, n_bins + 0.0, n_bins + 2.5, -1.0):
        tau = t0 + d_want * dt                                   # (dt is a power of two and the d_want are dyadic: exact)
        d = R.start_of(tau, t0, dt)
        assert d == d_want
        cube = np.zeros((1, 1, n_bins), R.CLD)
        R.render_ref(cube, 0, one(a, tau), s, L, t0, dt, False)
        n = np.arange(n_bins, dtype=np.float64)
        want = a * rts.waveform_eval(w, n - d)
        np.testing.assert_allclose(R.to_double(cube[0, 0]), want, rtol=1e-13, atol=1e-14 * np.abs(s).max())
        assert np.array_equal(R.to_double(cube[0, 0]) != 0, want != 0)             # the same support, sample for sample
        seen.add(bool(np.any(want != 0)))
    assert seen == {True, False}                                  # rows that are hit and rows that stay zero


def test_sample_and_hold_takes_floor_not_truncation():
    """L = 1: sample m of a start d lands in floor(d) + m; for d in (-1, 0) that is m - 1 and sample 0 is lost"""
    s = np.array([1 + 1j, 2, 3, 4j])
    cube = np.zeros((1, 1, 6), R.CLD)
    R.render_ref(cube, 0, one(1.0, -0.25), s, 1, 0.0, 1.0, False)
    assert np.array_equal(R.to_double(cube[0, 0]), [2, 3, 4j, 0, 0, 0])
    imp = np.zeros((1, 1, 6), R.CLD)
    R.accumulate_ref(imp, 0, one(1.0, -0.25) + one(2.0, 0.0) + one(3.0, 5.999) + one(4.0, 6.0), 0.0, 1.0)
    assert np.array_equal(R.to_double(imp[0, 0]), [2, 0, 0, 0, 0, 3])


def test_agrees_with_the_restatement_of_test_gpu_render():
    """the same contributions, waveforms, T0 / DT / NB as test_gpu_render.py through both restatements, Doppler off and on"""
    import test_gpu_render as G
    rng = np.random.default_rng(5)
    waves = [(rng.standard_normal(24) + 1j * rng.standard_normal(24), 8), (np.exp(1j * np.pi * 0.6 * (np.arange(48) - 23.5) ** 2 / 48), 16),
             (np.full(40, 1.0 + 0.0j), 1)]
    cs, fc = 299792458.0, 1.0e9
    rec = np.zeros(30, [("rayLength", np.float64), ("power", np.float64), ("doppler", np.float64), ("received", np.int32)])
    rec["rayLength"] = cs * (G.T0 + G.DT * rng.uniform(-30.0, G.NB + 10.0, len(rec)))
    rec["power"] = rng.uniform(0.5, 4.0, len(rec)); rec["doppler"] = rng.uniform(-4e6, 4e6, len(rec)); rec["received"] = rng.integers(0, 3, len(rec))
    theirs, mine = G.contribs_rays(rec, cs, fc), R.contribs_rays(rec, cs, fc)
    for s, L in waves:
        for dop in (False, True):
            a = G.render_ref(np.zeros((2, 2, G.NB), np.complex128), 1, theirs, s, L, G.T0, G.DT, dop)
            b = R.render_ref(np.zeros((2, 2, G.NB), R.CLD), 1, mine, s, L, G.T0, G.DT, dop)
            assert np.count_nonzero(a) > 100
            assert np.array_equal(a != 0, R.to_double(b) != 0)
            # (the float64 restatement carries the rounding of tau 2 pi fc ~ 7e3 rad: 1e-12 of the amplitude)
            np.testing.assert_allclose(a, R.to_double(b), rtol=1e-10, atol=1e-11 * np.abs(a).max())
            assert np.count_nonzero(R.to_double(b)[:, 0]) == 0


def test_dft_is_numpy_fft():
    rng = np.random.default_rng(9)
    for n_p, n_fft, nb in ((1, 2, 3), (3, 4, 1), (17, 32, 7), (64, 64, 2), (100, 256, 3)):
        x = rng.standard_normal((2, n_p, nb)) + 1j * rng.standard_normal((2, n_p, nb))
        np.testing.assert_allclose(R.to_double(R.dft_ref(x, n_fft)), np.fft.fft(x, n=n_fft, axis=1), rtol=0, atol=1e-13 * math.sqrt(n_fft) * np.abs(x).max())


def test_correlate_is_numpy_correlate():
    rng = np.random.default_rng(10)
    for N, M in ((1, 1), (5, 1), (5, 9), (64, 2), (300, 77)):
        y = rng.standard_normal(N) + 1j * rng.standard_normal(N); s = rng.standard_normal(M) + 1j * rng.standard_normal(M)
        want = np.correlate(np.concatenate([y, np.zeros(M)]), s, "full")[M - 1:M - 1 + N]
        np.testing.assert_allclose(R.to_double(R.correlate_ref(y, s)), want, rtol=0, atol=1e-13 * M * np.abs(y).max() * np.abs(s).max())
    assert np.array_equal(R.to_double(R.correlate_ref([1, 2, 3 + 1j], [2j])), [-2j, -4j, 2 - 6j])


def test_accumulate_reproduces_the_closed_form():
    """the inputs and the closed form of test_oracle_kat.py::test_cube_definition_closed_form"""
    c, fc = 299792458.0, 1.0e9
    rec = np.zeros(4, [("rayLength", np.float64), ("power", np.float64), ("doppler", np.float64), ("received", np.int32)])
    rec["received"] = [0, 0, 1, 5]; rec["power"] = [4.0, 9.0, 16.0, 1.0]
    rec["rayLength"] = [c * 1.05e-6, c * 1.05e-6, c * 1.31e-6, c * 1.0e-6]
    cube = R.accumulate_ref(np.zeros((2, 3, 8), R.CLD), 1, R.contribs_rays(rec, c, fc), 1.0e-6, 0.1e-6)
    ph = lambda d: -math.fmod(d * 2 * math.pi * fc, 2 * math.pi)
    d0 = rec["rayLength"][0] / c; d2 = rec["rayLength"][2] / c
    want = np.zeros((2, 3, 8), np.complex128)
    want[0, 1, 0] = (2.0 + 3.0) * complex(math.cos(ph(d0)), math.sin(ph(d0)))
    want[1, 1, 3] = 4.0 * complex(math.cos(ph(d2)), math.sin(ph(d2)))
    got = R.to_double(cube)
    assert np.array_equal(got != 0, want != 0)
    np.testing.assert_allclose(got, want, rtol=1e-11, atol=0)      # (the closed form's float64 phase argument, 6.6e3 rad, is good to 1e-12)
    # per unique path: rays 0 and 1 form one group -> ONE term with the group's values
    grp = R.contribs_paths([0, 0, 1], [6.25, 6.25, 16.0], [0, 0, 0], [d0, d0, d2], [ph(d0), ph(d0), ph(d2)], [0, 0, 2])
    cube2 = R.to_double(R.accumulate_ref(np.zeros((2, 3, 8), R.CLD), 2, grp, 1.0e-6, 0.1e-6))
    assert np.count_nonzero(cube2) == 2 and abs(abs(cube2[0, 2, 0]) - 2.5) < 1e-15 and abs(abs(cube2[1, 2, 3]) - 4.0) < 1e-15
