"""Space-time adaptive processing on the host (no GPU): rts_st_covariance_eval, rts_st_apply_eval and rts_st_steering_make against the
plain-Python restatement of include/rts_amd.h's text (RtsStCovParams, RtsStApplyParams; tests/stap_ref.py) bit for bit and against
numpy within the project's bound for re-associated sums (rtol 1e-10, atol 1e-12 max|ref|, as tests/test_adapt_host.py); n_taps = 1
against rts_covariance_eval / rts_beamform_eval, bits; the steering's sign against numpy.fft; every refusal the header lists that
needs no device; rts_amd/csrc/rts_stap.h alone under AddressSanitizer + UndefinedBehaviorSanitizer (tests/stap/stap_main.cpp, a
stand-alone program; nothing is preloaded) with the filter's plan at its edges; and the host run of the whole chain on the clutter
scene, judged in the scene's TRUE covariance."""
import ctypes as C
import math
import os
import shutil
import subprocess

import numpy as np
import pytest

import adapt_ref as A
import beam_ref as B
import stap_ref as S

ROOT = S.ROOT
TILE, PARTS = S.TILE, S.MAX_PARTS


def bits(a):
    return np.ascontiguousarray(a).view(np.float64)


def close(got, want):
    np.testing.assert_allclose(got, want, rtol=1e-10, atol=1e-12 * np.abs(want).max())


# ----------------------------------------------------------------------------- 1. against the restatement and numpy
@pytest.mark.parametrize("N,M,K", [(1, 1, 5), (1, 2, TILE + 1), (3, 2, 1), (3, 2, TILE - 1), (3, 2, TILE), (3, 2, 2 * TILE + 3), (2, 16, 7), (8, 3, TILE + 2)])
def test_covariance_against_restatement(rts, N, M, K):
    rng = np.random.default_rng(1000 * N + 10 * M + K)
    srows, bins = A.shape_for(K)                                                   # snapshot rows x bins = K
    rows = srows + M - 1
    inp = B.random_complex(rng, (N, rows + 2, bins)); inp[:, 0] = np.nan; inp[:, -1] = np.nan       # rows outside the span: never read
    got = rts.st_covariance_eval(inp, M, first=1, count=rows)
    assert got.shape == (N * M, N * M) and np.all(np.isfinite(bits(got)))
    assert np.array_equal(bits(got), bits(S.st_cov_restated(inp, M, first=1, count=rows)))
    x = S.snapshots_numpy(inp, M, 1, rows).reshape(N * M, -1)
    close(got, x @ x.conj().T / K)


@pytest.mark.parametrize("K", [TILE * (PARTS - 1), TILE * PARTS, TILE * (PARTS + 1) - 7])
def test_covariance_at_the_parts_cap(rts, K):
    rng = np.random.default_rng(K)
    srows, bins = A.shape_for(K)
    inp = B.random_complex(rng, (1, srows + 1, bins))
    got = rts.st_covariance_eval(inp, 2)
    assert np.array_equal(bits(got), bits(S.st_cov_restated(inp, 2)))
    x = S.snapshots_numpy(inp, 2).reshape(2, -1)
    close(got, x @ x.conj().T / K)


@pytest.mark.parametrize("skip", [None, (2, 3), (13, 4), (3, 1), (2, 14), (3, 14)], ids=["none", "first", "last", "one", "leaves-last", "leaves-first"])
def test_covariance_skip_interval(rts, skip):
    """bins 2 .. 16 of 19, the span rows 1 .. 5 of 7 with 2 taps (4 snapshot rows)"""
    rng = np.random.default_rng(99)
    inp = B.random_complex(rng, (3, 7, 19)); inp[:, 0] = np.nan; inp[:, 6] = np.nan; inp[:, :, :2] = np.nan; inp[:, :, 17:] = np.nan
    if skip:
        inp[:, :, skip[0]:skip[0] + skip[1]] = np.nan                             # the skipped bins are never read
    train = dict(first=1, count=5, first_bin=2, n_bins=15, skip=skip)
    got = rts.st_covariance_eval(inp, 2, **train)
    assert np.all(np.isfinite(bits(got))) and np.array_equal(bits(got), bits(S.st_cov_restated(inp, 2, **train)))


@pytest.mark.parametrize("N,M,F,rows,bins", [(1, 1, 1, 1, 1), (2, 1, 3, 2, 5), (2, 3, 3, 3, 4), (2, 3, 3, 5, 4), (3, 2, 17, 4, 3), (2, 16, 2, 17, 2), (8, 8, 1, 9, 2)])
def test_apply_against_restatement(rts, N, M, F, rows, bins):
    rng = np.random.default_rng(N * 1000 + M * 100 + F)
    inp = B.random_complex(rng, (N, rows + 2, bins)); inp[:, 0] = np.nan; inp[:, -1] = np.nan
    w = B.random_complex(rng, (F, N * M))
    got = rts.st_apply_eval(inp, w, M, first=1, count=rows)
    assert got.shape == (F, rows - M + 1, bins) and np.all(np.isfinite(bits(got)))
    assert np.array_equal(bits(got), bits(S.st_apply_restated(inp, w, M, first=1, count=rows)))
    close(got, np.einsum("fd,dpb->fpb", w.conj(), S.snapshots_numpy(inp, M, 1, rows)))
    assert np.array_equal(rts.st_apply_eval(inp, w, M, first=1, count=rows, power=True), B.power_restated(got))


def test_one_tap_is_the_receivers_product(rts):
    rng = np.random.default_rng(5)
    inp = B.random_complex(rng, (5, 4, 70)); w = B.random_complex(rng, (3, 5))
    train = dict(first=1, count=2, first_bin=3, skip=(30, 5))
    assert np.array_equal(bits(rts.st_covariance_eval(inp, 1, **train)), bits(rts.covariance_eval(inp, **train)))
    assert np.array_equal(bits(rts.st_covariance_eval(inp, 1)), bits(rts.covariance_eval(inp)))
    assert np.array_equal(bits(rts.st_apply_eval(inp, w, 1, first=1, count=3)), bits(rts.beamform_eval(inp, w, first=1, count=3)))
    assert np.array_equal(rts.st_apply_eval(inp, w, 1, power=True), rts.beamform_eval(inp, w, power=True))


# ----------------------------------------------------------------------------- 2. the steering product
def test_steering_against_restatement(rts):
    rng = np.random.default_rng(8)
    spatial = B.random_complex(rng, (2, 3)); f = np.array([0.0, 0.25, -0.125, 0.3, 1.75, -2.6]); taper = np.array([1.0, 0.5, 0.25, 2.0])

    def cos_sin(fr):
        """the library's cosine and sine of 2 pi fr: rts_steering_make of one element at x = fr wavelengths along the direction"""
        w = rts.steering([[fr, 0.0, 0.0]], [[0.0, 0.0]], 1.0)[0, 0]
        return float(w.real), float(w.imag)
    for tp in (None, taper):
        got = rts.st_steering(spatial, f, 4, tp)
        assert got.shape == (12, 12) and np.array_equal(bits(got), bits(S.st_steering_restated(spatial, f, 4, tp, cos_sin)))
    t = np.exp(2j * np.pi * f[:, None] * np.arange(4)[None, :])
    want = np.einsum("km,br->bkmr", t, spatial).reshape(12, 12)
    # numpy's phase 2 pi f m is a product of rounded factors, off by up to 2 eps |2 pi f m| radians; 4 eps for the two products' roundings
    np.testing.assert_allclose(rts.st_steering(spatial, f, 4), want, rtol=0, atol=(4 * math.pi * np.abs(f).max() * 3 + 4) * A.EPS * np.abs(spatial).max())
    assert np.array_equal(bits(rts.st_steering(spatial, [0.3], 1)), bits(spatial))           # one tap: t_0 = 1 exactly


def test_steering_sign_against_fft(rts):
    """a scatterer at f = k / n cycles per pulse advances by e^{+2 pi j f} per pulse: numpy's forward transform (rts_cube_doppler's
    sign) peaks in bin k, and the filter steered at f -- not at -f -- takes it whole"""
    n, k = 16, 5
    x = np.exp(2j * np.pi * k / n * np.arange(n))
    assert np.argmax(np.abs(np.fft.fft(x))) == k
    s = rts.st_steering(np.ones((1, 1)), [k / n, -k / n], n)
    y = rts.st_apply_eval(x.reshape(1, n, 1), s, n)
    assert y.shape == (2, 1, 1) and abs(y[0, 0, 0] - n) < 1e-12 * n and abs(y[1, 0, 0]) < 1e-12 * n


# ----------------------------------------------------------------------------- 3. refusals
def setter(**kw):
    def f(p):
        for k, v in kw.items():
            setattr(p, k, v)
    return f


def reserved(i):
    def f(p):
        p.reserved[i] = 1
    return f


def test_st_covariance_eval_refusals(rts):
    from rts_amd import _lib as L
    lib = L.lib()

    def case():
        """3 receivers, 5 rows of 9 bins; 2 taps over rows 1 .. 3, bins 2 .. 7 without 4 .. 5"""
        q = L.RtsCubeParams(3, 5, 9, 0, 0.0, 1.0)
        p = L.RtsStCovParams()
        p.source, p.first_row, p.n_rows, p.first_bin, p.n_bins, p.skip_first_bin, p.skip_n_bins, p.n_taps = L.RTS_BEAM_FROM_CUBE, 1, 3, 2, 6, 4, 2, 2
        return q, np.ones((3, 5, 9, 2)), 5, p

    def call(q, inp, rows_in, p, out):
        return lib.rts_st_covariance_eval(C.byref(q) if q is not None else None, inp.ctypes.data if inp is not None else None, rows_in,
                                          C.byref(p) if p is not None else None, out.ctypes.data if out is not None else None)
    out = np.full(6 * 6 * 2 + 1, 7.25)
    q, inp, rows_in, p = case()
    assert call(q, inp, rows_in, p, out) == L.RTS_OK and not np.any(out[:-1] == 7.25) and out[-1] == 7.25
    bad = [("reserved 0", reserved(0), b"reserved"), ("reserved 1", reserved(1), b"reserved"), ("reserved0", setter(reserved0=1), b"reserved"),
           ("unknown source", setter(source=3), b"source"), ("n_rows_in with the cube", setter(n_rows_in=5), b"n_rows_in"),
           ("device_in with the cube", setter(device_in=inp.ctypes.data), b"device_in"), ("pointer without n_rows_in", setter(source=L.RTS_BEAM_FROM_POINTER), b"n_rows_in"),
           ("pointer with other rows", setter(source=L.RTS_BEAM_FROM_POINTER, n_rows_in=6), b"n_rows_in"),
           ("no taps", setter(n_taps=0), b"n_taps"), ("too many taps", setter(n_taps=17), b"n_taps"),
           ("rows below the taps", setter(n_rows=1), b"n_taps"), ("default rows below the taps", setter(first_row=4, n_rows=0), b"n_taps"),
           ("first_row beyond", setter(first_row=5, n_rows=0), b"first_row"), ("rows beyond", setter(first_row=3), b"n_rows"),
           ("first_bin beyond", setter(first_bin=9, n_bins=0, skip_n_bins=0, skip_first_bin=0), b"first_bin"), ("bins beyond", setter(first_bin=4), b"n_bins"),
           ("skip before the span", setter(skip_first_bin=1), b"skip_first_bin"), ("skip leaves nothing", setter(skip_first_bin=2, skip_n_bins=6), b"leaves no bin"),
           ("skip_first_bin without skip_n_bins", setter(skip_n_bins=0), b"skip_first_bin")]
    for name, mutate, word in bad:
        q, inp, rows_in, p = case()
        mutate(p)
        out[:] = 7.25
        assert call(q, inp, rows_in, p, out) == L.RTS_ERR_INVALID, name
        assert word in lib.rts_last_error(), (name, lib.rts_last_error())
        assert np.all(out == 7.25), name
    q, inp, rows_in, p = case()
    assert call(None, inp, rows_in, p, out) == L.RTS_ERR_INVALID and call(q, None, rows_in, p, out) == L.RTS_ERR_INVALID
    assert call(q, inp, rows_in, None, out) == L.RTS_ERR_INVALID and call(q, inp, rows_in, p, None) == L.RTS_ERR_INVALID
    assert call(q, inp, 0, p, out) == L.RTS_ERR_INVALID and b"n_rows_in" in lib.rts_last_error()
    assert call(L.RtsCubeParams(65, 5, 9, 0, 0.0, 1.0), inp, rows_in, p, out) == L.RTS_ERR_INVALID and b"n_rx" in lib.rts_last_error()
    p.n_taps = 13                                                                   # 13 taps of 5 receivers: 65 entries
    assert call(L.RtsCubeParams(5, 5, 9, 0, 0.0, 1.0), inp, rows_in, p, out) == L.RTS_ERR_INVALID and b"n_taps * n_rx" in lib.rts_last_error()
    assert np.all(out == 7.25)
    # accepted edges: as many rows as taps, the pointer source with its rows, the default rows, D = 64
    for kw in (dict(n_rows=2), dict(source=L.RTS_BEAM_FROM_POINTER, n_rows_in=5), dict(n_rows=0), dict(first_row=3, n_rows=0)):
        q, inp, rows_in, p = case()
        setter(**kw)(p)
        out[:] = 7.25
        assert call(q, inp, rows_in, p, out) == L.RTS_OK, kw
        assert not np.any(out[:-1] == 7.25) and out[-1] == 7.25, kw
    assert rts.st_covariance_eval(np.ones((4, 16, 2)), 16).shape == (64, 64)


def test_st_apply_eval_refusals(rts):
    from rts_amd import _lib as L
    lib = L.lib()

    def case():
        """3 receivers, 5 rows of 4 bins; 2 filters of 2 taps over rows 1 .. 3"""
        q = L.RtsCubeParams(3, 5, 4, 0, 0.0, 1.0)
        w = np.arange(1.0, 25.0).reshape(2, 6, 2) / 8.0
        p = L.RtsStApplyParams()
        p.n_filters, p.source, p.first_row, p.n_rows, p.n_taps, p.weights = 2, L.RTS_BEAM_FROM_CUBE, 1, 3, 2, w.ctypes.data
        return q, np.ones((3, 5, 4, 2)), 5, p, w

    def call(q, inp, rows_in, p, out):
        return lib.rts_st_apply_eval(C.byref(q) if q is not None else None, inp.ctypes.data if inp is not None else None, rows_in,
                                     C.byref(p) if p is not None else None, out.ctypes.data if out is not None else None)

    def poison(index, value):
        def f(p):
            C.cast(p.weights, C.POINTER(C.c_double))[index] = value
        return f
    out = np.full(2 * 2 * 4 * 2 + 1, 7.25)
    q, inp, rows_in, p, w = case()
    assert call(q, inp, rows_in, p, out) == L.RTS_OK and not np.any(out[:-1] == 7.25) and out[-1] == 7.25
    many = np.ones(2 * 1025 * 6)
    bad = [("reserved 0", reserved(0), b"reserved"), ("reserved 1", reserved(1), b"reserved"), ("reserved0", setter(reserved0=1), b"reserved"),
           ("unknown source", setter(source=3), b"source"), ("peak", setter(flags=L.RTS_BEAM_PEAK), b"flags"), ("unknown flag", setter(flags=4), b"flags"),
           ("no taps", setter(n_taps=0), b"n_taps"), ("too many taps", setter(n_taps=17), b"n_taps"),
           ("no filters", setter(n_filters=0), b"n_filters"), ("too many filters", setter(n_filters=1025, weights=many.ctypes.data), b"n_filters"),
           ("too many weights", setter(n_filters=683, weights=many.ctypes.data), b"n_filters * n_taps * n_rx"),
           ("null weights", setter(weights=None), b"weights"), ("weights nan", poison(5, math.nan), b"weights"), ("weights inf", poison(23, math.inf), b"weights"),
           ("n_rows_in with the cube", setter(n_rows_in=5), b"n_rows_in"), ("device_in with the cube", setter(device_in=inp.ctypes.data), b"device_in"),
           ("pointer without n_rows_in", setter(source=L.RTS_BEAM_FROM_POINTER), b"n_rows_in"), ("pointer with other rows", setter(source=L.RTS_BEAM_FROM_POINTER, n_rows_in=6), b"n_rows_in"),
           ("first_row beyond", setter(first_row=5, n_rows=0), b"first_row"), ("rows beyond", setter(first_row=3), b"n_rows"),
           ("rows below the taps", setter(n_rows=1), b"n_taps"), ("default rows below the taps", setter(first_row=4, n_rows=0), b"n_taps")]
    for name, mutate, word in bad:
        q, inp, rows_in, p, w = case()
        mutate(p)
        out[:] = 7.25
        assert call(q, inp, rows_in, p, out) == L.RTS_ERR_INVALID, name
        assert word in lib.rts_last_error(), (name, lib.rts_last_error())
        assert np.all(out == 7.25), name
    q, inp, rows_in, p, w = case()
    assert call(None, inp, rows_in, p, out) == L.RTS_ERR_INVALID and call(q, None, rows_in, p, out) == L.RTS_ERR_INVALID
    assert call(q, inp, rows_in, None, out) == L.RTS_ERR_INVALID and call(q, inp, rows_in, p, None) == L.RTS_ERR_INVALID
    assert call(q, inp, 0, p, out) == L.RTS_ERR_INVALID and b"n_rows_in" in lib.rts_last_error()
    p.n_taps = 13; p.weights = many.ctypes.data                                     # 13 taps of 5 receivers: 65 entries
    assert call(L.RtsCubeParams(5, 5, 4, 0, 0.0, 1.0), inp, rows_in, p, out) == L.RTS_ERR_INVALID and b"n_taps * n_rx" in lib.rts_last_error()
    assert np.all(out == 7.25)
    p.n_taps = 2
    p.n_filters = 682; p.weights = many.ctypes.data                                 # 682 * 6 = 4092 weights: accepted
    big = np.full(682 * 2 * 4 * 2, 7.25)
    assert call(q, inp, rows_in, p, big) == L.RTS_OK and not np.any(big == 7.25)
    with pytest.raises(ValueError):
        rts.st_apply_eval(np.ones((3, 5, 4)), np.ones((2, 5)), 2)
    # the steering's refusals
    sp = np.ones((2, 3, 2)); f = np.array([0.25]); o = np.full(2 * 6 * 2, 7.25)
    steer = lambda spatial, n_rx, n_beams, dop, n_dop, taps, taper, out_: lib.rts_st_steering_make(spatial, n_rx, n_beams, dop, n_dop, taps, taper, out_)
    assert steer(sp.ctypes.data, 3, 2, f.ctypes.data, 1, 2, None, o.ctypes.data) == L.RTS_OK and not np.any(o == 7.25)
    o[:] = 7.25
    nan = np.array([math.nan, 1.0])
    for args, word in (((None, 3, 2, f.ctypes.data, 1, 2, None, o.ctypes.data), b"null"), ((sp.ctypes.data, 3, 2, None, 1, 2, None, o.ctypes.data), b"null"),
                       ((sp.ctypes.data, 3, 2, f.ctypes.data, 1, 2, None, None), b"null"), ((sp.ctypes.data, 0, 2, f.ctypes.data, 1, 2, None, o.ctypes.data), b"n_rx"),
                       ((sp.ctypes.data, 3, 0, f.ctypes.data, 1, 2, None, o.ctypes.data), b"n_beams"), ((sp.ctypes.data, 3, 2, f.ctypes.data, 0, 2, None, o.ctypes.data), b"n_doppler"),
                       ((sp.ctypes.data, 3, 2, f.ctypes.data, 1, 0, None, o.ctypes.data), b"n_taps"), ((sp.ctypes.data, 3, 2, f.ctypes.data, 1, 17, None, o.ctypes.data), b"n_taps"),
                       ((sp.ctypes.data, 5, 1, f.ctypes.data, 1, 13, None, o.ctypes.data), b"n_taps * n_rx"), ((sp.ctypes.data, 3, 2, nan.ctypes.data, 1, 2, None, o.ctypes.data), b"doppler"),
                       ((sp.ctypes.data, 3, 2, f.ctypes.data, 1, 2, nan.ctypes.data, o.ctypes.data), b"tap_taper"),
                       ((np.full((2, 3, 2), math.inf).ctypes.data, 3, 2, f.ctypes.data, 1, 2, None, o.ctypes.data), b"spatial")):
        assert steer(*args) == L.RTS_ERR_INVALID, word
        assert word in lib.rts_last_error(), (word, lib.rts_last_error())
    assert np.all(o == 7.25)
    with pytest.raises(ValueError):
        rts.st_steering(np.ones((1, 2)), [0.1], 3, tap_taper=[1.0, 1.0])


# ----------------------------------------------------------------------------- 4. rts_stap.h alone, under the sanitizers
@pytest.fixture(scope="module")
def stap_main(tmp_path_factory):
    gxx = shutil.which("g++")
    if not gxx:
        pytest.skip("no g++")
    rt = subprocess.run([gxx, "-print-file-name=libasan.so"], capture_output=True, text=True).stdout.strip()
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"] if os.path.isabs(rt) and os.path.exists(rt) else []
    exe = str(tmp_path_factory.mktemp("stap") / "stap_main")
    subprocess.check_call([gxx, "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-ffp-contract=off"] + san + ["-I", os.path.join(ROOT, "rts_amd", "csrc"),
                           os.path.join(ROOT, "tests", "stap", "stap_main.cpp"), "-o", exe])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")

    def ask(cases, kind=float):
        text = "".join(" ".join(repr(x) if isinstance(x, float) else str(x) for x in c) + "\n" for c in cases)
        r = subprocess.run([exe], input=text, capture_output=True, text=True, env=env, timeout=120)
        assert r.returncode == 0, r.stderr[-3000:]
        out = [[kind(x) for x in line.split()] for line in r.stdout.splitlines()]
        assert len(out) == len(cases)
        return out
    return ask


def main_input(n_rx, rows, nb):
    """the input tests/stap/stap_main.cpp fills"""
    r = np.arange(n_rx)[:, None, None]; p = np.arange(rows)[None, :, None]; b = np.arange(nb)[None, None, :]
    return (((r * 131 + p * 17 + b * 7) % 23) - 11.0 + 0.25 * p) + 1j * (((r * 5 + p * 3 + b * 11) % 19) - 9.0 - 0.5 * b)


def main_weights(F, D):
    f = np.arange(F)[:, None]; d = np.arange(D)[None, :]
    return (((f * 7 + d * 3) % 11) - 5.0) / 8.0 + 1j * ((((f * 5 + d * 13) % 9) - 4.0) / 16.0 + 0.03125)


def test_header_alone_reads_only_what_it_is_given(stap_main):
    """every input element outside the training snapshots (the covariance) or outside the span's rows (the filter) is poisoned in the
    driver; outputs are heap arrays of exactly their sizes: a read or write beyond them ends the run.  The values: the restatement's"""
    cases = [("stcov", n_rx, taps, rows_in, nb, first, rows, fb, span, sf, sn)
             for (n_rx, taps) in ((1, 1), (1, 3), (3, 2), (4, 16))
             for (rows_in, first, rows) in ((taps, 0, taps), (taps + 3, 1, taps + 1), (taps + 3, 3, taps))
             for (nb, fb, span, sf, sn) in ((1, 0, 1, 0, 0), (9, 2, 6, 2, 2), (9, 2, 6, 6, 2), (9, 1, 8, 1, 7), (70, 3, 67, 10, 1))]
    for c, g in zip(cases, stap_main(cases)):
        _, n_rx, taps, rows_in, nb, first, rows, fb, span, sf, sn = c
        want = S.st_cov_restated(main_input(n_rx, rows_in, nb), taps, first=first, count=rows, first_bin=fb, n_bins=span, skip=(sf, sn) if sn else None)
        assert np.array_equal(np.array(g), bits(want).ravel()), c
    cases = [("stapply", n_rx, taps, rows_in, nb, first, rows, F, flags)
             for (n_rx, taps, F) in ((1, 1, 1), (2, 3, 3), (3, 2, 17), (4, 16, 2))
             for (rows_in, first, rows) in ((taps, 0, taps), (taps + 3, 1, taps + 1), (taps + 3, 3, taps))
             for nb in (1, 5) for flags in (0, 1)]
    for c, g in zip(cases, stap_main(cases)):
        _, n_rx, taps, rows_in, nb, first, rows, F, flags = c
        y = S.st_apply_restated(main_input(n_rx, rows_in, nb), main_weights(F, n_rx * taps), taps, first=first, count=rows)
        assert np.array_equal(np.array(g), (B.power_restated(y) if flags else bits(y)).ravel()), c


def test_apply_plan(stap_main):
    MT, T, STRIP, RXT, GRID, MAXRX, MAXB, MAXW, ATILE = stap_main([("consts",)], int)[0]
    assert (MT, T, STRIP, RXT) == (S.MAX_TAPS, S.THREADS, S.STRIP, S.RX_TILE) and T == 64 and GRID == 2 ** 31 - 1 and ATILE == TILE
    tiles = [stap_main([("tile", m)], int)[0][0] for m in range(1, MT + 1)]
    assert tiles == [S.filter_tile(m) for m in range(1, MT + 1)]
    assert all(m * t <= 32 for m, t in zip(range(1, MT + 1), tiles))                # the running sums of a thread: at most 128 VGPRs
    assert all(16 * t * min(MAXRX, MAXRX // m * m) <= 16 * 1024 for m, t in zip(range(1, MT + 1), tiles))      # a tile's weights in LDS
    plan = lambda *a: stap_main([("applyplan",) + a], int)[0]     # n_rx n_taps n_filters n_rows n_bins flags -> D out_rows tile tiles strips bin_groups groups out_cells lds out_doubles supported
    assert plan(1, 1, 1, 1, 1, 0) == [1, 1, 16, 1, 1, 1, 1, 1, 16 * 16, 2, 1]
    assert plan(8, 3, 16, 256, 4096, 0) == [24, 254, 8, 2, 16, 64, 2048, 254 * 4096, 16 * 8 * 24, 2 * 16 * 254 * 4096, 1]
    assert plan(8, 8, 16, 256, 4096, 1) == [64, 249, 4, 4, 16, 64, 4096, 249 * 4096, 16 * 4 * 64, 16 * 249 * 4096, 1]
    # the strips and the bin groups at their edges
    assert [plan(2, 3, 1, r + 2, 1, 0)[4] for r in (1, STRIP - 1, STRIP, STRIP + 1, 2 * STRIP + 1)] == [1, 1, 1, 2, 3]
    assert [plan(2, 3, 1, 3, b, 0)[5] for b in (1, T - 1, T, T + 1, 4 * T + 1)] == [1, 1, 1, 2, 5]
    assert [plan(2, 2, f, 2, 1, 0)[3] for f in (1, 15, 16, 17, 1024)] == [1, 1, 1, 2, 64]
    # the limits
    assert plan(2, 3, 1, 2, 1, 0)[-1] == 0 and plan(2, 0, 1, 2, 1, 0)[-1] == 0 and plan(2, 17, 1, 20, 1, 0)[-1] == 0 and plan(5, 13, 1, 20, 1, 0)[-1] == 0
    assert plan(4, 16, 64, 16, 1, 0)[-1] == 1 and plan(4, 16, 65, 16, 1, 0)[-1] == 0 and plan(2, 2, 1025, 2, 1, 0)[-1] == 0 and plan(2, 2, 1, 2, 0, 0)[-1] == 0
    assert plan(1, 1, 1, 2 ** 32 - 1, 64, 0)[-1] == 1 and plan(1, 1, 1, 2 ** 32 - 1, 1024, 0)[-1] == 0      # 2^28 strips x 16 bin groups: the grid


# ----------------------------------------------------------------------------- 5. the whole chain, on the host
def chain_figures(rts, taps):
    sc = S.SCENE
    cube, s, cov, w, y = S.scene_host(rts, taps)
    R = S.scene_true_covariance(taps)
    v = S.space_time_vector(sc["target_az"], sc["target_f"], taps)
    conv = s[0] / np.vdot(s[0], s[0]).real
    adaptive, conventional, optimum = S.sinr(w[0], v, R), S.sinr(conv, v, R), np.vdot(v, np.linalg.solve(R, v)).real
    amap = np.abs(S.doppler_map(y[0], sc["n_fft"])) ** 2
    cmap = np.abs(S.doppler_map(rts.st_apply_eval(cube, conv[None, :], taps)[0], sc["n_fft"])) ** 2
    return S.db(adaptive / conventional), S.db(optimum / adaptive), amap, cmap


def test_chain_on_the_host(rts):
    """clutter ridge + noise + a 0 dB target -> the stacked covariance without the target's bins -> weights -> the filter -> a 16-point
    Doppler transform.  With the scene's seed: SINR improvement over the conventional space-time beam 23.88 dB, loss against the
    clairvoyant optimum 0.19 dB, the target 12.87 dB over the strongest other cell of its Doppler row, the conventional map's peak
    at (1, 5); with one tap the improvement is 0.02 dB"""
    sc = S.SCENE
    improvement, loss, amap, cmap = chain_figures(rts, sc["taps"])
    target = (sc["doppler_row"], sc["target_bin"])
    row = amap[sc["doppler_row"]].copy(); row[sc["skip"][0]:sc["skip"][0] + sc["skip"][1]] = 0.0
    over = S.db(amap[target] / row.max())
    print("improvement %.2f dB, loss %.2f dB, target over its row %.2f dB, adaptive peak %s, conventional peak %s"
          % (improvement, loss, over, np.unravel_index(amap.argmax(), amap.shape), np.unravel_index(cmap.argmax(), cmap.shape)))
    assert improvement >= 20.0
    assert loss <= 1.0
    assert np.unravel_index(amap.argmax(), amap.shape) == target
    assert over >= 6.0
    assert np.unravel_index(cmap.argmax(), cmap.shape) != target
    one = chain_figures(rts, 1)[0]
    print("one tap: improvement %.3f dB" % one)
    assert abs(one) < 1.0
