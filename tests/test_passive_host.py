"""Passive radar on the host (no GPU): rts_cancel_eval and rts_xcorr_eval against the plain-Python restatement of the two trees in
include/rts_amd.h (RtsCancelParams, RtsXcorrParams; tests/passive_ref.py) bit for bit and against numpy within stated bounds, known
answers, the edge shapes, failed blocks, every numbered refusal, and rts_amd/csrc/rts_passive.h alone under AddressSanitizer +
UndefinedBehaviorSanitizer (tests/passive/passive_main.cpp) with the plans at their edges.

"Bit for bit" is meant literally: the trees hold + - * / and sqrt only, the library is built with -ffp-contract=off and Python floats
never contract.  Against numpy the sums have the project's bound for re-associated sums, rtol 1e-10 and atol 1e-12 max|ref|
(tests/test_adapt_host.py); the coefficients lie within K eps cond(G + loading I) of the longdouble solution of the normal equations,
relative to the largest |c| (the forward error of a Cholesky solve; cond computed here).  Measured: the evaluator's coefficients are
0.01 .. 0.26 of that bound away (conditions 1.2 .. 416; test_coefficients_against_longdouble prints each case)."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import passive_ref as P

ROOT = P.ROOT
bits = P.bits


def same(a, b):
    return np.array_equal(bits(a), bits(b), equal_nan=True)


# ----------------------------------------------------------------------------- 1. against the restatement, over the edge shapes
CANCEL, XCORR = P.cancel_cases(), P.xcorr_cases()


@pytest.mark.parametrize("case", CANCEL, ids=[c[0] for c in CANCEL])
def test_cancel_against_restatement(rts, case):
    name, n_rx, n_p, N, kw = case
    cube = P.cancel_input(name, n_rx, n_p, N, kw)                  # rows outside the span are NaN: never read, never written
    want_cube, want_c, want_info = P.cancel_restated(cube, **kw)
    got_cube, got_c, got_info = rts.cancel_eval(cube, **kw)
    assert got_info == want_info and want_info[1] == 0
    assert same(got_c, want_c) and same(got_cube, want_cube)
    first, count = kw.get("first", 0), kw.get("count", n_p - kw.get("first", 0))
    assert np.all(np.isfinite(bits(got_cube[:, first:first + count]))) and np.all(np.isfinite(bits(got_c)))
    assert same(got_cube[kw["ref_rx"]], cube[kw["ref_rx"]]) and not got_c[kw["ref_rx"]].any()      # the reference: never written, zeros in its slot


@pytest.mark.parametrize("case", XCORR, ids=[c[0] for c in XCORR])
def test_xcorr_against_restatement(rts, case):
    name, n_rx, n_p, N, kw = case
    cube = P.xcorr_input(name, n_rx, n_p, N, kw)
    got = rts.xcorr_eval(cube, **kw)
    assert same(got, P.xcorr_restated(cube, **kw)) and np.all(np.isfinite(bits(got)))
    first, count = kw.get("first", 0), kw.get("count", n_p - kw.get("first", 0))
    want = P.xcorr_numpy(cube[:, first:first + count], kw["ref_rx"], kw["n_lags"], kw.get("first_lag", 0))
    np.testing.assert_allclose(got, want, rtol=1e-10, atol=1e-12 * max(np.abs(want).max(), 1e-300))
    beyond = max(N - kw.get("first_lag", 0), 0)
    assert not bits(got[:, :, beyond:]).any()                         # lags at or beyond n_bins: exact zeros (+0.0)


@pytest.mark.parametrize("case", P.cancel_cases_evaluator_only(), ids=[c[0] for c in P.cancel_cases_evaluator_only()])
def test_cancel_many_tiles_per_part_against_numpy(rts, case):
    """64 taps, one part of several tiles per block: too many terms for the plain-Python tree, so the evaluator is held to numpy
    (G c = b with the loading, as test_gram_and_cross_sums_against_numpy; the cancelled rows are y - X c at the rows' own scale)"""
    name, n_rx, n_p, N, kw = case
    cube = P.cancel_input(name, n_rx, n_p, N, kw)
    got, c, info = rts.cancel_eval(cube, **kw)
    blks = P.blocks(n_p, kw["rows_per_block"])
    assert info == (len(blks), 0) and len(P.parts(blks[0][1], N, len(blks))) == 1
    K, ref = kw["n_taps"], kw["ref_rx"]
    for b, (r0, rb) in list(enumerate(blks))[::37]:
        X = P.lag_matrix(cube[ref, r0:r0 + rb], K)
        G = X.conj().T @ X + kw["loading"] * np.eye(K)
        for r in range(n_rx):
            if r == ref:
                continue
            y = cube[r, r0:r0 + rb].reshape(-1)
            np.testing.assert_allclose(G @ c[r, b], X.conj().T @ y, rtol=1e-10, atol=1e-12 * np.abs(G).max() * np.abs(c[r, b]).max() * K)
            np.testing.assert_allclose(got[r, r0:r0 + rb].reshape(-1), y - X @ c[r, b], rtol=1e-10, atol=1e-12 * np.abs(y).max() * K)


def test_partition_is_the_headers():
    """tiles of 256 bins, row-major; min(tiles, max(1, 512 / n_blocks)) parts"""
    assert (P.TILE, P.MAX_PARTS, P.MAX_TAPS, P.MAX_BLOCKS, P.MAX_LAGS) == (256, 512, 64, 4096, 16384)
    assert [len(P.parts(1, n, 128)) for n in (2 * 256 + 7, 3 * 256 + 7, 4 * 256 + 7)] == [3, 4, 4]
    assert len(P.parts(3, 700, 1)) == 9 and len(P.parts(200, 700, 1)) == 512 and len(P.parts(1, 5000, 4096)) == 1
    assert P.blocks(7, 3) == [(0, 3), (3, 3), (6, 1)] and P.blocks(5, 0) == [(0, 5)] == P.blocks(5, 6)


# ----------------------------------------------------------------------------- 2. against numpy
SUM_SHAPES = [(2, 3, 700, 5, 0), (3, 8, 300, 16, 4), (2, 40, 1100, 3, 1)]


@pytest.mark.parametrize("n_rx,n_p,N,K,R", SUM_SHAPES)
def test_gram_and_cross_sums_against_numpy(rts, n_rx, n_p, N, K, R):
    """INDIRECT: nothing hands out G or b (the evaluator returns the cancelled cube and the coefficients), so the sums are held to
    numpy's through the equation they determine with loading 0, G c = b, G and b formed by numpy from the stacked lag matrix of each
    block, at the project's bound for re-associated sums scaled by what the product sums (|G| |c| K).  A wrong term, lag, tile or
    part shows here; the shapes are well conditioned so that c does not hide it"""
    rng = np.random.default_rng(N + K)
    cube = P.random_complex(rng, (n_rx, n_p, N))
    _, c, (nblk, nfail) = rts.cancel_eval(cube, 0, K, R)
    assert nfail == 0
    for b, (r0, rb) in enumerate(P.blocks(n_p, R)):
        X = P.lag_matrix(cube[0, r0:r0 + rb], K)
        G = X.conj().T @ X
        for r in range(1, n_rx):
            rhs = X.conj().T @ cube[r, r0:r0 + rb].reshape(-1)
            np.testing.assert_allclose(G @ c[r, b], rhs, rtol=1e-10, atol=1e-12 * np.abs(G).max() * np.abs(c[r, b]).max() * K)


COEFF_CASES = [(4, 4, 300, 0.0, 1.0), (16, 8, 200, 0.0, 1.0), (64, 4, 400, 0.0, 1.0), (16, 8, 200, 1e-3, 1.0), (8, 2, 64, 0.0, 0.97), (8, 2, 64, 10.0, 0.97)]


@pytest.mark.parametrize("K,n_p,N,loading,rho", COEFF_CASES)
def test_coefficients_against_longdouble(rts, K, n_p, N, loading, rho):
    """rho < 1: a strongly coloured reference (a first-order recursion), an ill-conditioned G"""
    rng = np.random.default_rng(K * 1000 + N)
    cube = P.random_complex(rng, (3, n_p, N))
    if rho < 1.0:
        for n in range(1, N):
            cube[0, :, n] += rho * cube[0, :, n - 1]
    cube[1] += 30.0 * cube[0]; cube[2, :, 1:] += (2.0 + 1.0j) * cube[0, :, :-1]
    _, c, info = rts.cancel_eval(cube, 0, K, 0, loading=loading)
    assert info == (1, 0)
    for r in (1, 2):
        A, b = P.gram_longdouble(cube[0], cube[r], K, loading)
        want = P.solve_longdouble(A, b)
        err = float(np.abs(c[r, 0] - want).max() / np.abs(want).max())
        bound = P.solve_bound(A)
        print("K %d loading %g rho %g receiver %d: cond %.3g, error %.3g of bound %.3g (%.3g of it)" % (K, loading, rho, r, np.linalg.cond(A.astype(np.complex128)), err, bound, err / bound))
        assert err <= bound


def test_cancel_against_lstsq(rts):
    """the cancelled rows against np.linalg.lstsq on the stacked lag matrix: the residuals agree to the re-association bound of the
    rows' own scale (the subtraction forms 30 x the reference and takes it away again)"""
    rng = np.random.default_rng(8)
    cube = P.random_complex(rng, (3, 6, 90)); cube[1] += 30.0 * cube[0]; cube[2, :, 2:] += 7.0j * cube[0, :, :-2]
    got, c, _ = rts.cancel_eval(cube, 0, 4, 3)
    want, cn = P.cancel_numpy(cube, 0, 4, 3)
    np.testing.assert_allclose(c, cn, rtol=1e-10, atol=1e-12 * np.abs(cn).max())
    np.testing.assert_allclose(got, want, rtol=1e-10, atol=1e-12 * np.abs(cube).max() * 4)


# ----------------------------------------------------------------------------- 3. known answers
def test_a_row_in_the_span_cancels_to_the_bound(rts):
    """y = sum a_k x_k exactly representable terms aside: the coefficients are a_k and the residual is at K eps cond of the row"""
    rng = np.random.default_rng(21)
    K, N, n_p = 5, 120, 4
    cube = P.random_complex(rng, (2, n_p, N))
    a = np.array([3.0, -1.5 + 2.0j, 0.25j, 0.0, -4.0])
    X = P.lag_matrix(cube[0], K)
    cube[1] = (X @ a).reshape(n_p, N)
    got, c, info = rts.cancel_eval(cube, 0, K)
    bound = K * P.EPS * np.linalg.cond(X.conj().T @ X)
    print("coefficients off by %.3g, residual %.3g of the row (bound %.3g)" % (np.abs(c[1, 0] - a).max(), np.abs(got[1]).max() / np.abs(cube[1]).max(), bound))
    assert info == (1, 0) and np.abs(c[1, 0] - a).max() <= bound * np.abs(a).max()
    assert np.abs(got[1]).max() <= bound * K * np.abs(a).max() * np.abs(cube[0]).max()


def test_a_row_orthogonal_to_the_span_is_unchanged_within_the_bound(rts):
    rng = np.random.default_rng(22)
    K, N, n_p = 4, 80, 3
    cube = P.random_complex(rng, (2, n_p, N))
    X = P.lag_matrix(cube[0], K)
    y = cube[1].reshape(-1)
    y = y - X @ np.linalg.lstsq(X, y, rcond=None)[0]                  # orthogonal to every lagged copy, to rounding
    cube[1] = y.reshape(n_p, N)
    got, c, _ = rts.cancel_eval(cube, 0, K)
    bound = K * P.EPS * np.linalg.cond(X.conj().T @ X)
    # b = X^H y is rounding: N n_p eps |x| |y| per entry; c = G^-1 b is that over the smallest eigenvalue of G
    tiny = N * n_p * P.EPS * np.abs(cube[0]).max() * np.abs(y).max() * K / np.linalg.eigvalsh(X.conj().T @ X).min()
    assert np.abs(c[1, 0]).max() <= tiny + bound
    assert np.abs(got[1] - cube[1]).max() <= K * (tiny + bound) * np.abs(cube[0]).max()


def test_autocorrelation_known_answers(rts):
    rng = np.random.default_rng(23)
    x = np.round(P.random_complex(rng, (1, 2, 50)) * 8) / 8           # eighths: every product and sum below is exact
    z = rts.xcorr_eval(x, 0, 50)
    assert np.array_equal(z[0, :, 0], (np.abs(x[0]) ** 2).sum(axis=1)) and not z[0, :, 0].imag.any()
    # Hermitian symmetry: the lag -l of the autocorrelation is conj of lag l; with two receivers that are each other's reference
    two = np.concatenate([x, np.round(P.random_complex(rng, (1, 2, 50)) * 8) / 8])
    ab, ba = rts.xcorr_eval(two, 0, 50)[1], rts.xcorr_eval(two[::-1], 0, 50)[1]      # sum y[n + l] conj(x[n])  and  sum x[n + l] conj(y[n])
    assert np.array_equal(ab[:, 0], np.conj(ba[:, 0]))
    full = np.array([np.correlate(two[1, p], two[0, p], "full") for p in range(2)])   # index l + 49 holds sum y[n + l] conj(x[n])
    assert np.array_equal(ab, full[:, 49:]) and np.array_equal(np.conj(ba[:, ::-1]), full[:, :50])


def test_an_on_grid_echo_peaks_at_its_lag(rts):
    rng = np.random.default_rng(24)
    N, l0, a = 200, 37, 0.5 - 0.25j
    x = np.round(P.random_complex(rng, (3, N)) * 16) / 16
    cube = np.zeros((2, 3, N), np.complex128); cube[1] = x
    cube[0, :, l0:] = a * x[:, :N - l0]
    z = rts.xcorr_eval(cube, 1, 64)[0]
    assert np.all(np.argmax(np.abs(z), axis=1) == l0)
    assert np.array_equal(z[:, l0], a * (np.abs(x[:, :N - l0]) ** 2).sum(axis=1))


# ----------------------------------------------------------------------------- 4. masks, failed blocks
def test_mask_leaves_receivers_out(rts):
    name, n_rx, n_p, N, kw = [c for c in CANCEL if c[0] == "mask"][0]
    cube = P.cancel_input(name, n_rx, n_p, N, kw)
    got, c, _ = rts.cancel_eval(cube, **kw)
    assert same(got[1], cube[1]) and same(got[2], cube[2]) and not c[1].any() and not c[2].any()
    as_mask, c2, _ = rts.cancel_eval(cube, **dict(kw, rx=0b1001))
    assert same(as_mask, got) and same(c2, c)
    one, c1, _ = rts.cancel_eval(cube, **dict(kw, rx=[3]))            # a receiver's result does not depend on who else is cancelled
    assert same(one[3], got[3]) and same(one[0], cube[0]) and same(c1[3], c[3])


def test_one_receiver_is_a_no_op(rts):
    cube = P.random_complex(np.random.default_rng(3), (1, 3, 33))
    got, c, info = rts.cancel_eval(cube, 0, 3)
    assert same(got, cube) and not c.any() and info == (1, 0)
    z = rts.xcorr_eval(cube, 0, 33)
    assert z.shape == (1, 3, 33) and np.allclose(z[0, :, 0], (np.abs(cube[0]) ** 2).sum(axis=1))


@pytest.mark.parametrize("why", ["few_samples", "zero_reference", "nan_reference", "inf_reference"])
def test_failed_blocks(rts, why):
    """three blocks of two rows; the failing ones are untouched for every receiver, their coefficients 0, and counted -- in the
    restatement too"""
    rng = np.random.default_rng(5)
    K, N = (4, 1) if why == "few_samples" else (3, 20)
    cube = P.random_complex(rng, (3, 6, N))
    kw = dict(ref_rx=0, n_taps=K, rows_per_block=2)
    if why == "zero_reference":
        cube[0, 2:4] = 0.0
    if why == "nan_reference":
        cube[0, 3, 7] = np.nan
    if why == "inf_reference":
        cube[0, 2, 19] = np.inf
    got, c, info = rts.cancel_eval(cube, **kw)
    want, wc, winfo = P.cancel_restated(cube, **kw)
    assert info == winfo == ((3, 3) if why == "few_samples" else (3, 1))
    assert same(got, want) and same(c, wc)
    bad = slice(0, 6) if why == "few_samples" else slice(2, 4)
    assert same(got[:, bad], cube[:, bad]) and not c[:, 1].any()
    if why != "few_samples":
        assert not same(got[1, :2], cube[1, :2]) and c[1, 0].all() and c[2, 2].all()
    if why == "few_samples":                                          # a loading makes the same blocks solvable
        assert rts.cancel_eval(cube, loading=1e-6, **kw)[2] == (3, 0)


# ----------------------------------------------------------------------------- 5. every numbered refusal
def raw_cancel(rts, q, cube, p):
    L = rts.L
    rc = L.lib().rts_cancel_eval(C.byref(q) if q is not None else None, cube.ctypes.data_as(C.c_void_p) if cube is not None else None, C.byref(p) if p is not None else None, None, None, None)
    return rc, L.lib().rts_last_error().decode()


def raw_xcorr(rts, q, cube, p, out):
    L = rts.L
    rc = L.lib().rts_xcorr_eval(C.byref(q) if q is not None else None, cube.ctypes.data_as(C.c_void_p) if cube is not None else None, C.byref(p) if p is not None else None,
                                out.ctypes.data_as(C.c_void_p) if out is not None else None)
    return rc, L.lib().rts_last_error().decode()


def test_cancel_refusals(rts):
    L = rts.L
    cube = np.ones((3, 4, 8), np.complex128); before = cube.copy()
    q = L.RtsCubeParams(3, 4, 8, 0, 0.0, 1.0)

    def par(**kw):
        p = L.RtsCancelParams(); p.ref_rx, p.n_taps, p.first_pulse, p.n_pulses = 0, 2, 0, 4
        for k, v in kw.items():
            setattr(p, k, v)
        return p
    res = L.RtsCancelParams(); res.n_taps, res.n_pulses = 2, 4; res.reserved[1] = 1
    cases = [(par(reserved0=1), "reserved"), (res, "reserved"), (par(ref_rx=3), "ref_rx"), (par(n_taps=0), "n_taps"), (par(n_taps=P.MAX_TAPS + 1), "n_taps"),
             (par(n_pulses=0), "pulse"), (par(first_pulse=4, n_pulses=1), "pulse"), (par(first_pulse=2, n_pulses=3), "pulse"), (par(first_pulse=0xffffffff, n_pulses=2), "pulse"),
             (par(loading=-1e-300), "loading"), (par(loading=float("inf")), "loading"), (par(loading=float("nan")), "loading"),
             (par(rx_mask=0b011), "names ref_rx"), (par(rx_mask=0b1010), "beyond the cube"), (par(rx_mask=1 << 63), "beyond the cube")]
    for p, word in cases:
        rc, msg = raw_cancel(rts, q, cube, p)
        assert rc == L.RTS_ERR_INVALID and word in msg and msg.startswith("rts_cancel_eval"), (word, msg)
    assert raw_cancel(rts, q, cube, None)[0] == L.RTS_ERR_INVALID and raw_cancel(rts, q, None, par())[0] == L.RTS_ERR_INVALID
    assert raw_cancel(rts, None, cube, par())[0] == L.RTS_ERR_INVALID
    big = L.RtsCubeParams(65, 1, 1, 0, 0.0, 1.0)                      # rule 2: more receivers than rx_mask has bits
    rc, msg = raw_cancel(rts, big, np.ones((65, 1, 1), np.complex128), par(n_pulses=1))
    assert rc == L.RTS_ERR_INVALID and "RTS_PASSIVE_MAX_RX" in msg
    many = L.RtsCubeParams(1, P.MAX_BLOCKS + 1, 1, 0, 0.0, 1.0)      # rule 9: one block per row, one row too many
    tall = np.ones((1, P.MAX_BLOCKS + 1, 1), np.complex128)
    rc, msg = raw_cancel(rts, many, tall, par(n_pulses=P.MAX_BLOCKS + 1, rows_per_block=1))
    assert rc == L.RTS_ERR_INVALID and "RTS_PASSIVE_MAX_BLOCKS" in msg
    assert raw_cancel(rts, many, tall, par(n_pulses=P.MAX_BLOCKS, rows_per_block=1))[0] == L.RTS_OK
    assert same(cube, before)                                         # a refused call leaves the cube untouched
    assert raw_cancel(rts, q, cube, par(rx_mask=0b110))[0] == L.RTS_OK


def test_xcorr_refusals(rts):
    L = rts.L
    cube = np.ones((3, 4, 8), np.complex128); out = np.full((3, 4, 5), 7.0 + 0j)
    q = L.RtsCubeParams(3, 4, 8, 0, 0.0, 1.0)

    def par(**kw):
        p = L.RtsXcorrParams(); p.ref_rx, p.first_pulse, p.n_pulses, p.first_lag, p.n_lags = 0, 0, 4, 0, 5
        for k, v in kw.items():
            setattr(p, k, v)
        return p
    res = par(); res.reserved[0] = 1
    cases = [(par(reserved0=1), "reserved"), (res, "reserved"), (par(ref_rx=3), "ref_rx"), (par(n_pulses=0), "pulse"), (par(first_pulse=3, n_pulses=2), "pulse"),
             (par(n_lags=0), "n_lags"), (par(n_lags=P.MAX_LAGS + 1), "n_lags"), (par(first_lag=0x7fff0001), "first_lag")]
    for p, word in cases:
        rc, msg = raw_xcorr(rts, q, cube, p, out)
        assert rc == L.RTS_ERR_INVALID and word in msg and msg.startswith("rts_xcorr_eval"), (word, msg)
    wide = L.RtsCubeParams(1, 1, P.MAX_BINS + 1, 0, 0.0, 1.0)       # rule 6
    rc, msg = raw_xcorr(rts, wide, np.ones((1, 1, P.MAX_BINS + 1), np.complex128), par(n_pulses=1), out)
    assert rc == L.RTS_ERR_INVALID and "RTS_COMPRESS_MAX_BINS" in msg
    tall = L.RtsCubeParams(1, 65536, 1, 0, 0.0, 1.0)                 # rule 7
    rc, msg = raw_xcorr(rts, tall, np.ones((1, 65536, 1), np.complex128), par(n_pulses=65536), out)
    assert rc == L.RTS_ERR_INVALID and "launch grid" in msg
    for args in ((q, cube, None, out), (q, None, par(), out), (q, cube, par(), None), (None, cube, par(), out)):
        assert raw_xcorr(rts, *args)[0] == L.RTS_ERR_INVALID
    assert np.all(out == 7.0)                                         # a refused call leaves out untouched
    assert raw_xcorr(rts, q, cube, par(first_lag=0x7fff0000), out)[0] == L.RTS_OK and not out.any()


def test_abi_sizes(rts):
    L = rts.L
    assert C.sizeof(L.RtsCancelParams) == 56 and C.sizeof(L.RtsXcorrParams) == 40
    text = open(os.path.join(ROOT, "rts_amd", "csrc", "rts_internal.h")).read()
    assert "sizeof(RtsCancelParams) == 56 && sizeof(RtsXcorrParams) == 40" in text
    hdr = open(os.path.join(ROOT, "include", "rts_amd.h")).read()
    assert "} RtsCancelParams;                                            /* 56 bytes */" in hdr and "} RtsXcorrParams;                                             /* 40 bytes */" in hdr
    assert (L.RTS_PASSIVE_MAX_TAPS, L.RTS_PASSIVE_MAX_RX, L.RTS_PASSIVE_TILE, L.RTS_PASSIVE_MAX_PARTS, L.RTS_PASSIVE_MAX_BLOCKS, L.RTS_XCORR_MAX_LAGS) == (64, 64, P.TILE, P.MAX_PARTS, P.MAX_BLOCKS, P.MAX_LAGS)


# ----------------------------------------------------------------------------- 6. rts_passive.h alone, under the sanitizers
@pytest.fixture(scope="module")
def passive_main(tmp_path_factory):
    gxx = shutil.which("g++")
    if not gxx:
        pytest.skip("no g++")
    rt = subprocess.run([gxx, "-print-file-name=libasan.so"], capture_output=True, text=True).stdout.strip()
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"] if os.path.isabs(rt) and os.path.exists(rt) else []
    exe = str(tmp_path_factory.mktemp("passive") / "passive_main")
    subprocess.check_call([gxx, "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-ffp-contract=off"] + san + ["-I", os.path.join(ROOT, "rts_amd", "csrc"),
                           os.path.join(ROOT, "tests", "passive", "passive_main.cpp"), "-o", exe])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:verify_asan_link_order=0", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")

    def ask(lines):
        r = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True, env=env, timeout=120)
        assert r.returncode == 0, r.stderr[-3000:]
        out = r.stdout.splitlines()
        assert len(out) == len(lines)
        return [line.split() for line in out]
    return ask


def main_input(n_rx, n_p, N):
    """the driver's input: small dyadic values, so that it needs no file"""
    r, p, b = np.meshgrid(np.arange(n_rx), np.arange(n_p), np.arange(N), indexing="ij")
    re = ((r * 131 + p * 17 + b * 7) % 23 - 11.0) / 8.0 + 0.25 * p
    im = ((r * 5 + p * 3 + b * 11) % 19 - 9.0) / 16.0 - 0.03125 * b
    return re + 1j * im


def test_plans_at_their_edges(passive_main):
    """cancelplan n_rx n_bins n_rows rows_per_block K -> K R n_blocks tpr ppb tri stride gram_blocks gram_threads gram_lds solve_lds scratch sums coeff supported"""
    ask = [("cancelplan 4 4096 256 0 64", [64, 256, 1, 16, 512, 2080, 2336, 528, 576, 16 * 319, 16 * 64 * 64 + 16 * 64 * 64, 2 * 512 * 2336, 2 * 2336, 2 * 4 * 64, 1]),
           ("cancelplan 4 4096 256 1 64", [64, 1, 256, 16, 2, 2080, 2336, 528, 576, 16 * 319, 131072, 2 * 256 * 2 * 2336, 2 * 256 * 2336, 2 * 4 * 256 * 64, 1]),
           ("cancelplan 2 1 1 7 1", [1, 1, 1, 1, 512, 1, 3, 1, 64, 16 * 256, 16 + 1024, 2 * 512 * 3, 6, 4, 1]),
           ("cancelplan 1 256 4096 1 3", [3, 1, 4096, 1, 1, 6, 9, 3, 64, 16 * 258, 16 * 9 + 3072, 2 * 4096 * 9, 2 * 4096 * 9, 2 * 4096 * 3, 1]),
           ("cancelplan 1 257 4097 1 3", [3, 1, 4097, 2, 0, 6, 9, 3, 64, 16 * 258, 16 * 9 + 3072, 0, 2 * 4097 * 9, 2 * 4097 * 3, 0]),
           ("cancelplan 65 8 8 0 2", None), ("cancelplan 2 8 8 0 65", None), ("cancelplan 2 8 8 0 0", None)]
    got = passive_main([a for a, _ in ask])
    for (line, want), g in zip(ask, got):
        if want is None:
            assert g[-1] == "0", line
        else:
            assert [int(v) for v in g] == want, (line, g)
    x = passive_main(["xcorrplan 4 256 1024", "xcorrplan 1 1 1", "xcorrplan 1 1 16384", "xcorrplan 1 1 16385", "xcorrplan 65536 1 1", "xcorrplan 1 65536 1", "xcorrplan 1 1 257"])
    assert [[int(v) for v in g] for g in x] == [[4, 8192, 2 * 4 * 256 * 1024, 1], [1, 8192, 2, 1], [64, 8192, 32768, 1], [65, 8192, 32770, 0], [1, 8192, 131072, 0], [1, 8192, 131072, 0], [2, 8192, 514, 1]]


RULES = [("cancelrule 3 4 0 2 0 4 0 0 0 0", 0), ("cancelrule 3 4 0 2 0 4 0 1 0 0", 1), ("cancelrule 65 4 0 2 0 4 0 0 0 0", 2), ("cancelrule 3 4 3 2 0 4 0 0 0 0", 3),
         ("cancelrule 3 4 0 0 0 4 0 0 0 0", 4), ("cancelrule 3 4 0 65 0 4 0 0 0 0", 4), ("cancelrule 3 4 0 2 0 0 0 0 0 0", 5), ("cancelrule 3 4 0 2 4 1 0 0 0 0", 5),
         ("cancelrule 3 4 0 2 0 4 0 0 0 -1", 6), ("cancelrule 3 4 0 2 0 4 0 0 3 0", 7), ("cancelrule 3 4 0 2 0 4 0 0 8 0", 8), ("cancelrule 1 4097 0 2 0 4097 1 0 0 0", 9),
         ("cancelrule 1 4097 0 2 0 4097 2 0 0 0", 0), ("cancelrule 64 4 63 2 0 4 0 0 1 0", 0),
         ("xcorrrule 3 4 8 0 0 4 0 5 0", 0), ("xcorrrule 3 4 8 0 0 4 0 5 1", 1), ("xcorrrule 3 4 8 3 0 4 0 5 0", 2), ("xcorrrule 3 4 8 0 4 1 0 5 0", 3), ("xcorrrule 3 4 8 0 0 4 0 0 0", 4),
         ("xcorrrule 3 4 8 0 0 4 0 16385 0", 4), ("xcorrrule 3 4 8 0 0 4 2147418113 5 0", 5), ("xcorrrule 3 4 8193 0 0 4 0 5 0", 6), ("xcorrrule 65536 4 8 0 0 4 0 5 0", 7)]


def test_numbered_rules(passive_main):
    """cancelrule n_rx n_pulses ref_rx n_taps first n rows_per_block reserved rx_mask loading; xcorrrule n_rx n_pulses n_bins ref_rx first n first_lag n_lags reserved"""
    got = passive_main([a for a, _ in RULES])
    assert [int(g[0]) for g in got] == [w for _, w in RULES]


MAIN_CANCEL = [(2, 2, 1, dict(ref_rx=0, n_taps=1)), (3, 5, 7, dict(ref_rx=1, n_taps=8, rows_per_block=2, loading=0.5)), (3, 7, 300, dict(ref_rx=2, n_taps=3, rows_per_block=3, first=1, count=5)),
               (2, 3, 64, dict(ref_rx=0, n_taps=64, loading=1.0)), (4, 3, 30, dict(ref_rx=1, n_taps=2, rx=[0, 3])), (2, 2, 2, dict(ref_rx=0, n_taps=4))]


def test_header_alone_reads_and_writes_only_what_it_is_given(rts, passive_main):
    """cube, coefficients and work arrays are heap arrays of exactly their sizes in the driver and the rows outside the span are
    poisoned; the results equal the library's bit for bit (the last case: every block fails)"""
    lines = []
    for n_rx, n_p, N, kw in MAIN_CANCEL:
        first = kw.get("first", 0); count = kw.get("count", n_p - first)
        lines.append("cancel %d %d %d %d %d %d %d %d %d %s" % (n_rx, n_p, N, kw["ref_rx"], kw["n_taps"], first, count, kw.get("rows_per_block", 0), rts._rx_mask(kw.get("rx")),
                                                               float(kw.get("loading", 0.0)).hex()))
    got = passive_main(lines)
    for (n_rx, n_p, N, kw), g in zip(MAIN_CANCEL, got):
        first = kw.get("first", 0); count = kw.get("count", n_p - first)
        cube = main_input(n_rx, n_p, N)
        want_cube, want_c, info = rts.cancel_eval(cube, **kw)
        assert (int(g[0]), int(g[1])) == info
        vals = np.array([float.fromhex(v) for v in g[2:]])
        nc = want_c.size * 2
        assert same(vals[:nc], want_c.reshape(-1)) and same(vals[nc:], want_cube[:, first:first + count].reshape(-1))
    assert int(got[-1][1]) == 1
    xl = ["xcorr 2 3 40 1 0 3 0 45", "xcorr 3 4 300 2 1 2 7 260", "xcorr 1 1 1 0 0 1 0 1", "xcorr 2 2 9 0 0 2 9 3"]
    for line, g in zip(xl, passive_main(xl)):
        n_rx, n_p, N, ref, first, count, first_lag, n_lags = (int(v) for v in line.split()[1:])
        want = rts.xcorr_eval(main_input(n_rx, n_p, N), ref, n_lags, first_lag, first, count)
        assert same(np.array([float.fromhex(v) for v in g]), want.reshape(-1))
