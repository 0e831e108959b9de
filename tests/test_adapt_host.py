"""Adaptive (MVDR) beamforming on the host (no GPU): rts_covariance_eval and rts_mvdr_eval against the plain-Python restatement of
the two trees in include/rts_amd.h (RtsCovParams, RtsMvdrParams; tests/adapt_ref.py) bit for bit and against numpy within stated
bounds, known answers, the MVDR properties on a line array with a jammer, the failed solve, every refusal the header lists for the
two host calls, rts_amd/csrc/rts_adapt.h alone under AddressSanitizer + UndefinedBehaviorSanitizer (tests/adapt/adapt_main.cpp) with
the plans at their edges, and the host run of the whole chain that tests/test_gpu_adapt.py repeats on the device.

"Bit for bit" is meant literally: the trees hold + - * / and sqrt only, the library is built with -ffp-contract=off and Python floats
never contract.  Against numpy the covariance has the project's bound for re-associated sums, rtol 1e-10 and atol 1e-12 max|ref|;
the weights lie within n_rx eps cond(A) of each beam's largest |w| (the forward error of a Cholesky solve; cond computed here)."""
import ctypes as C
import math
import os
import shutil
import subprocess

import numpy as np
import pytest

import adapt_ref as A
import beam_ref as B

ROOT = A.ROOT
TILE, PARTS = A.TILE, A.MAX_PARTS


def bits(a):
    return np.ascontiguousarray(a).view(np.float64)


# ----------------------------------------------------------------------------- 1. against the restatement
# K around the tile (one part) with every n_rx; K around the parts cap with 2 receivers
SMALL_K = [1, TILE - 1, TILE, TILE + 1, 3 * TILE + 5]
CAP_K = [TILE * (PARTS - 1), TILE * PARTS, TILE * (PARTS + 1) - 7]


@pytest.mark.parametrize("K", SMALL_K)
@pytest.mark.parametrize("n_rx", [1, 2, 3, 8])
def test_covariance_against_restatement(rts, n_rx, K):
    rng = np.random.default_rng(1000 * n_rx + K)
    rows, bins = A.shape_for(K)
    inp = B.random_complex(rng, (n_rx, rows + 2, bins)); inp[:, 0] = np.nan; inp[:, -1] = np.nan      # rows outside the span: never read
    ref = A.cov_restated(inp, first=1, count=rows)
    got = rts.covariance_eval(inp, first=1, count=rows)
    assert got.shape == (n_rx, n_rx) and np.all(np.isfinite(bits(got)))
    assert np.array_equal(bits(got), bits(ref))
    z = inp[:, 1:1 + rows].reshape(n_rx, -1)
    want = z @ z.conj().T / K
    np.testing.assert_allclose(got, want, rtol=1e-10, atol=1e-12 * np.abs(want).max())


@pytest.mark.parametrize("K", CAP_K)
def test_covariance_at_the_parts_cap(rts, K):
    assert [len(A.partition(k)) for k in CAP_K] == [PARTS - 1, PARTS, PARTS]
    rng = np.random.default_rng(K)
    rows, bins = A.shape_for(K)
    inp = B.random_complex(rng, (2, rows, bins))
    got = rts.covariance_eval(inp)
    assert np.array_equal(bits(got), bits(A.cov_restated(inp)))
    z = inp.reshape(2, -1); want = z @ z.conj().T / K
    np.testing.assert_allclose(got, want, rtol=1e-10, atol=1e-12 * np.abs(want).max())


@pytest.mark.parametrize("skip", [None, (2, 3), (13, 4), (3, 1), (2, 14), (3, 14)], ids=["none", "first", "last", "one", "leaves-last", "leaves-first"])
def test_covariance_skip_interval(rts, skip):
    """bins 2 .. 16 of 19, rows 1 .. 5 of 7: the interval absent, at the first bin, at the last, one bin, and leaving one bin"""
    rng = np.random.default_rng(99)
    inp = B.random_complex(rng, (3, 7, 19)); inp[:, 0] = np.nan; inp[:, 6] = np.nan; inp[:, :, :2] = np.nan; inp[:, :, 17:] = np.nan
    if skip:
        inp[:, :, skip[0]:skip[0] + skip[1]] = np.nan                             # the skipped bins are never read
    train = dict(first=1, count=5, first_bin=2, n_bins=15, skip=skip)
    got = rts.covariance_eval(inp, **train)
    assert np.all(np.isfinite(bits(got))) and np.array_equal(bits(got), bits(A.cov_restated(inp, **train)))
    cells = A.training_cells(7, 19, **train)
    assert len(cells) == 5 * (15 - (skip[1] if skip else 0))
    z = np.array([[inp[r, row, b] for (row, b) in cells] for r in range(3)]); want = z @ z.conj().T / len(cells)
    np.testing.assert_allclose(got, want, rtol=1e-10, atol=1e-12 * np.abs(want).max())


@pytest.mark.parametrize("loading", [0.0, 0.5])
@pytest.mark.parametrize("n_rx", [1, 2, 3, 8])
def test_mvdr_against_restatement(rts, n_rx, loading):
    rng = np.random.default_rng(77 + n_rx)
    cov = A.hermitian_pd(rng, n_rx)
    s = B.random_complex(rng, (5, n_rx))
    got = rts.mvdr_eval(cov, s, loading)
    assert got.shape == (5, n_rx) and np.array_equal(bits(got), bits(A.mvdr_restated(cov, s, loading)))
    # only the lower triangle and the diagonal's real parts are read
    junk = cov.copy(); junk[np.triu_indices(n_rx, 1)] = np.nan; junk.imag[np.diag_indices(n_rx)] = np.nan
    assert np.array_equal(bits(rts.mvdr_eval(junk, s, loading)), bits(got))


# ----------------------------------------------------------------------------- 2. against numpy
def jammer_cov(rng, n_rx, K, jnr, wl=0.03):
    pos = B.line_array(n_rx, wl); fc = B.C0 / wl
    noise = B.random_complex(rng, (n_rx, 1, K)) / math.sqrt(2.0)
    jam = B.snapshot(pos, math.radians(-25.0), 0.0, fc)[:, None, None] * (math.sqrt(jnr / 2.0) * B.random_complex(rng, (1, 1, K)))
    return pos, noise + jam


@pytest.mark.parametrize("loading", [1.0, 1e-3, 0.0])
@pytest.mark.parametrize("n_rx,K,jnr", [(3, 5, 1e2), (8, 16, 1e4), (8, 128, 1e6), (64, 128, 1e4)])
def test_mvdr_against_numpy(rts, n_rx, K, jnr, loading):
    rng = np.random.default_rng(n_rx * 1000 + K)
    pos, z = jammer_cov(rng, n_rx, K, jnr)
    cov = rts.covariance_eval(z)
    s = rts.steering(pos, [[0.1, 0.0], [-0.4, 0.0], [0.7, 0.0]], 0.03)
    Am = A.loaded(cov, loading)
    bound = A.solve_bound(Am)
    got = rts.mvdr_eval(cov, s, loading)
    want = A.mvdr_numpy(cov, s, loading)
    err = np.abs(got - want).max(axis=1) / np.abs(want).max(axis=1)
    print("n_rx %d K %d jnr %g loading %g: cond %.3g, error %.3g of bound %.3g" % (n_rx, K, jnr, loading, np.linalg.cond(Am), err.max(), bound))
    assert np.all(err <= bound)


# ----------------------------------------------------------------------------- 3. known answers
def test_known_answers(rts):
    rng = np.random.default_rng(3)
    z1 = B.random_complex(rng, (1, 2, 9)); s1 = B.random_complex(rng, (4, 1))
    w = rts.mvdr_eval(rts.covariance_eval(z1), s1)
    np.testing.assert_allclose(w, 1.0 / np.conj(s1), rtol=16 * A.EPS, atol=0)           # one receiver: w = 1 / conj(s)
    s = B.random_complex(rng, (3, 6))
    w = rts.mvdr_eval(np.eye(6), s)
    np.testing.assert_allclose(w, s / np.sum(np.abs(s) ** 2, axis=1)[:, None], rtol=16 * A.EPS, atol=0)      # R = I: w = s / (s^H s)
    z = B.random_complex(rng, (5, 3, 40))
    R = rts.covariance_eval(z)
    assert np.array_equal(bits(R.diagonal().imag), np.zeros(5)) and not np.any(np.signbit(R.diagonal().imag))       # +0.0 exactly
    lo = np.tril_indices(5, -1)
    assert np.array_equal(bits(R[lo].real), bits(R.T[lo].real)) and np.array_equal(bits(R[lo].imag), bits(-R.T[lo].imag))
    assert np.array_equal(bits(rts.covariance_eval(2.0 * z)), bits(4.0 * R))             # scaling by 2 scales R by 4 exactly


# ----------------------------------------------------------------------------- 4. properties
def test_mvdr_properties(rts):
    cube, s, cov, w, beams = A.scene_host(rts)
    pos, directions, fc = A.scene_geometry()
    sj = rts.steering(pos, [[A.SCENE["jammer_az"], 0.0]], A.SCENE["wavelength"])[0]
    A.assert_mvdr_properties(w, s, cov, A.SCENE["noise_power"], sj, A.SCENE["jammer_beam"])


# ----------------------------------------------------------------------------- 5. the failed solve
def test_failed_solve(rts):
    from rts_amd import _lib as L
    lib = L.lib()
    cov = np.array([[1.0, 2.0], [2.0, 1.0]], np.complex128); s = np.ones((3, 2), np.complex128)
    out = np.full((3, 2, 2), 7.25)
    p = L.RtsMvdrParams(); p.n_beams, p.n_rx, p.loading, p.steering = 3, 2, 0.0, s.ctypes.data
    assert lib.rts_mvdr_eval(cov.ctypes.data, 2, C.byref(p), out.ctypes.data) == L.RTS_ERR_INVALID
    assert b"pivot 1" in lib.rts_last_error() and np.all(out == 7.25)
    with pytest.raises(A.SolveFailed) as e:
        A.mvdr_restated(cov, s)
    assert e.value.pivot == 1
    p.loading = 1.5                                                                      # loaded, it is positive definite
    assert lib.rts_mvdr_eval(cov.ctypes.data, 2, C.byref(p), out.ctypes.data) == L.RTS_OK and np.all(np.isfinite(out))
    for bad, pivot in ((np.array([[0.0]]), 0), (np.array([[math.nan]]), 0), (np.array([[math.inf]]), 0), (np.array([[1.0, 0], [math.nan, 1.0]]), 1)):
        n = len(bad); p.n_rx, p.loading = n, 0.0
        out[:] = 7.25
        assert lib.rts_mvdr_eval(bad.astype(np.complex128).ctypes.data, n, C.byref(p), out.ctypes.data) == L.RTS_ERR_INVALID
        assert b"pivot %d" % pivot in lib.rts_last_error() and np.all(out == 7.25)


# ----------------------------------------------------------------------------- 6. refusals
def setter(**kw):
    def f(p, keep):
        for k, v in kw.items():
            setattr(p, k, v)
    return f


def reserved(i):
    def f(p, keep):
        p.reserved[i] = 1
    return f


def test_covariance_eval_refusals(rts):
    from rts_amd import _lib as L
    lib = L.lib()

    def case():
        """3 receivers, 4 rows of 9 bins; rows 1 .. 2, bins 2 .. 7 without 4 .. 5"""
        q = L.RtsCubeParams(3, 4, 9, 0, 0.0, 1.0)
        p = L.RtsCovParams()
        p.source, p.first_row, p.n_rows, p.first_bin, p.n_bins, p.skip_first_bin, p.skip_n_bins = L.RTS_BEAM_FROM_CUBE, 1, 2, 2, 6, 4, 2
        return q, np.ones((3, 4, 9, 2)), 4, p

    def call(q, inp, rows_in, p, out):
        return lib.rts_covariance_eval(C.byref(q) if q is not None else None, inp.ctypes.data if inp is not None else None, rows_in,
                                       C.byref(p) if p is not None else None, out.ctypes.data if out is not None else None)
    out = np.full(3 * 3 * 2 + 1, 7.25)
    q, inp, rows_in, p = case()
    assert call(q, inp, rows_in, p, out) == L.RTS_OK and not np.any(out[:-1] == 7.25) and out[-1] == 7.25
    bad = [("reserved 0", reserved(0), b"reserved"), ("reserved 1", reserved(1), b"reserved"), ("unknown source", setter(source=3), b"source"),
           ("n_rows_in with the cube", setter(n_rows_in=4), b"n_rows_in"), ("n_rows_in with the map", setter(source=L.RTS_BEAM_FROM_MAP, n_rows_in=4), b"n_rows_in"),
           ("device_in with the cube", setter(device_in=inp.ctypes.data), b"device_in"),
           ("pointer without n_rows_in", setter(source=L.RTS_BEAM_FROM_POINTER), b"n_rows_in"),
           ("pointer with other rows", setter(source=L.RTS_BEAM_FROM_POINTER, n_rows_in=5), b"n_rows_in"),
           ("first_row beyond", setter(first_row=4, n_rows=0), b"first_row"), ("rows beyond", setter(first_row=3), b"n_rows"),
           ("wrapping rows", setter(first_row=2, n_rows=0xffffffff), b"n_rows"),
           ("first_bin beyond", setter(first_bin=9, n_bins=0, skip_n_bins=0, skip_first_bin=0), b"first_bin"), ("bins beyond", setter(first_bin=4), b"n_bins"),
           ("wrapping bins", setter(n_bins=0xffffffff), b"n_bins"),
           ("skip before the span", setter(skip_first_bin=1), b"skip_first_bin"), ("skip behind the span", setter(skip_first_bin=8, skip_n_bins=1), b"skip_first_bin"),
           ("skip past the span's end", setter(skip_first_bin=6, skip_n_bins=3), b"skip_n_bins"), ("wrapping skip", setter(skip_n_bins=0xffffffff), b"skip_n_bins"),
           ("skip leaves nothing", setter(skip_first_bin=2, skip_n_bins=6), b"leaves no bin"),
           ("skip_first_bin without skip_n_bins", setter(skip_n_bins=0), b"skip_first_bin")]
    for name, mutate, word in bad:
        q, inp, rows_in, p = case()
        mutate(p, None)
        out[:] = 7.25
        assert call(q, inp, rows_in, p, out) == L.RTS_ERR_INVALID, name
        assert word in lib.rts_last_error(), (name, lib.rts_last_error())
        assert np.all(out == 7.25), name
    q, inp, rows_in, p = case()
    assert call(None, inp, rows_in, p, out) == L.RTS_ERR_INVALID and call(q, None, rows_in, p, out) == L.RTS_ERR_INVALID
    assert call(q, inp, rows_in, None, out) == L.RTS_ERR_INVALID and call(q, inp, rows_in, p, None) == L.RTS_ERR_INVALID
    assert call(q, inp, 0, p, out) == L.RTS_ERR_INVALID and b"n_rows_in" in lib.rts_last_error()
    assert call(L.RtsCubeParams(0, 4, 9, 0, 0.0, 1.0), inp, rows_in, p, out) == L.RTS_ERR_INVALID
    assert call(L.RtsCubeParams(3, 4, 0, 0, 0.0, 1.0), inp, rows_in, p, out) == L.RTS_ERR_INVALID
    assert call(L.RtsCubeParams(65, 4, 9, 0, 0.0, 1.0), inp, rows_in, p, out) == L.RTS_ERR_INVALID and b"n_rx" in lib.rts_last_error()
    # more tiles than the plan takes: 2^32 - 1 rows of 2^32 - 1 bins, refused before a sample is read
    pg = L.RtsCovParams()
    assert call(L.RtsCubeParams(3, 4, 0xffffffff, 0, 0.0, 1.0), inp, 0xffffffff, pg, out) == L.RTS_ERR_INVALID and b"tiles" in lib.rts_last_error()
    assert np.all(out == 7.25)
    # accepted edges: the pointer source with its rows, the map source, zeros that mean "to the last", the last row and bin alone, a skip that leaves one bin
    for kw in (dict(source=L.RTS_BEAM_FROM_POINTER, n_rows_in=4), dict(source=L.RTS_BEAM_FROM_MAP), dict(n_rows=0), dict(n_bins=0, first_bin=3),
               dict(first_row=3, n_rows=1), dict(first_bin=8, n_bins=1, skip_first_bin=0, skip_n_bins=0), dict(skip_first_bin=2, skip_n_bins=5), dict(skip_first_bin=3, skip_n_bins=5)):
        q, inp, rows_in, p = case()
        setter(**kw)(p, None)
        out[:] = 7.25
        assert call(q, inp, rows_in, p, out) == L.RTS_OK, kw
        assert not np.any(out[:-1] == 7.25) and out[-1] == 7.25, kw


def test_mvdr_eval_refusals(rts):
    from rts_amd import _lib as L
    lib = L.lib()

    def case():
        cov = np.eye(3, dtype=np.complex128); s = np.arange(1.0, 13.0).reshape(2, 3, 2) / 8.0
        p = L.RtsMvdrParams(); p.n_beams, p.n_rx, p.loading, p.steering = 2, 3, 0.25, s.ctypes.data
        return cov, p, dict(s=s)

    def call(cov, n_rx, p, out):
        return lib.rts_mvdr_eval(cov.ctypes.data if cov is not None else None, n_rx, C.byref(p) if p is not None else None, out.ctypes.data if out is not None else None)

    def poison(index, value):
        def f(p, keep):
            keep["s"].reshape(-1)[index] = value
        return f
    out = np.full(2 * 3 * 2 + 1, 7.25)
    cov, p, keep = case()
    assert call(cov, 3, p, out) == L.RTS_OK and not np.any(out[:-1] == 7.25) and out[-1] == 7.25
    many = np.ones(2 * 1025 * 3)
    bad = [("reserved 0", reserved(0), b"reserved"), ("reserved 1", reserved(1), b"reserved"), ("no beams", setter(n_beams=0), b"n_beams"),
           ("too many beams", setter(n_beams=1025, steering=many.ctypes.data), b"n_beams"), ("other n_rx", setter(n_rx=2), b"n_rx"),
           ("loading < 0", setter(loading=-1e-300), b"loading"), ("loading nan", setter(loading=math.nan), b"loading"), ("loading inf", setter(loading=math.inf), b"loading"),
           ("null steering", setter(steering=None), b"steering"), ("steering nan", poison(5, math.nan), b"steering"), ("steering inf", poison(11, -math.inf), b"steering")]
    for name, mutate, word in bad:
        cov, p, keep = case()
        mutate(p, keep)
        out[:] = 7.25
        assert call(cov, 3, p, out) == L.RTS_ERR_INVALID, name
        assert word in lib.rts_last_error(), (name, lib.rts_last_error())
        assert np.all(out == 7.25), name
    cov, p, keep = case()
    assert call(None, 3, p, out) == L.RTS_ERR_INVALID and call(cov, 3, None, out) == L.RTS_ERR_INVALID and call(cov, 3, p, None) == L.RTS_ERR_INVALID
    p.n_rx = 0
    assert call(cov, 0, p, out) == L.RTS_ERR_INVALID and b"n_rx" in lib.rts_last_error()
    # the limits: 65 receivers; 64 receivers x 65 beams (a weight table of the beamformer)
    wide = np.ones(2 * 65 * 65); big = np.eye(65, dtype=np.complex128)
    p = L.RtsMvdrParams(); p.n_beams, p.n_rx, p.steering = 1, 65, wide.ctypes.data
    assert call(big, 65, p, out) == L.RTS_ERR_INVALID and b"n_rx" in lib.rts_last_error()
    p.n_beams, p.n_rx = 65, 64
    assert call(big, 64, p, out) == L.RTS_ERR_INVALID and b"n_beams * n_rx" in lib.rts_last_error()
    assert np.all(out == 7.25)
    with pytest.raises(ValueError):
        rts.mvdr_eval(np.eye(3), np.ones((2, 4)))
    with pytest.raises(ValueError):
        rts.mvdr_eval(np.ones((2, 3)), np.ones((2, 3)))


# ----------------------------------------------------------------------------- 7. rts_adapt.h alone, under the sanitizers
@pytest.fixture(scope="module")
def adapt_main(tmp_path_factory):
    gxx = shutil.which("g++")
    if not gxx:
        pytest.skip("no g++")
    rt = subprocess.run([gxx, "-print-file-name=libasan.so"], capture_output=True, text=True).stdout.strip()
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"] if os.path.isabs(rt) and os.path.exists(rt) else []
    exe = str(tmp_path_factory.mktemp("adapt") / "adapt_main")
    subprocess.check_call([gxx, "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-ffp-contract=off"] + san + ["-I", os.path.join(ROOT, "rts_amd", "csrc"),
                           os.path.join(ROOT, "tests", "adapt", "adapt_main.cpp"), "-o", exe])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:verify_asan_link_order=0", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")

    def ask(cases, kind=float):
        text = "".join(" ".join(repr(x) if isinstance(x, float) else str(x) for x in c) + "\n" for c in cases)
        r = subprocess.run([exe], input=text, capture_output=True, text=True, env=env, timeout=120)
        assert r.returncode == 0, r.stderr[-3000:]
        out = [[kind(x) for x in line.split()] for line in r.stdout.splitlines()]
        assert len(out) == len(cases)
        return out
    return ask


def main_input(n_rx, rows, nb):
    """the input tests/adapt/adapt_main.cpp fills"""
    r = np.arange(n_rx)[:, None, None]; p = np.arange(rows)[None, :, None]; b = np.arange(nb)[None, None, :]
    return (((r * 131 + p * 17 + b * 7) % 23) - 11.0 + 0.25 * p) + 1j * (((r * 5 + p * 3 + b * 11) % 19) - 9.0 - 0.5 * b)


def main_cov(n, scale=1.0):
    i = np.arange(n)[:, None]; j = np.arange(n)[None, :]
    re = np.where(i == j, (n + 0.25 * i) * scale, (((i * 7 + j * 3) % 5) - 2.0) / 8.0)
    return re + 1j * ((((i * 5 + j * 11) % 7) - 3.0) / 16.0)


def main_steering(n_beams, n):
    b = np.arange(n_beams)[:, None]; r = np.arange(n)[None, :]
    return (((b * 7 + r * 3) % 11) - 5.0) / 8.0 + 1j * ((((b * 5 + r * 13) % 9) - 4.0) / 16.0 + 0.03125)


def test_header_alone_reads_only_what_it_is_given(adapt_main):
    """every input element outside the training set, and the covariance's upper triangle and diagonal imaginary parts, are poisoned in
    the driver; outputs and work arrays are heap arrays of exactly their sizes: a read or write beyond them ends the run.  The
    values: the restatement's, bit for bit"""
    cases = [("cov", n_rx, rows_in, nb, first, rows, fb, span, sf, sn)
             for n_rx in (1, 3, 8)
             for (rows_in, first, rows) in ((1, 0, 1), (4, 1, 2), (4, 3, 1))
             for (nb, fb, span, sf, sn) in ((1, 0, 1, 0, 0), (9, 0, 9, 0, 0), (9, 2, 6, 2, 2), (9, 2, 6, 6, 2), (9, 1, 8, 1, 7), (70, 3, 67, 10, 1))]
    for c, g in zip(cases, adapt_main(cases)):
        _, n_rx, rows_in, nb, first, rows, fb, span, sf, sn = c
        want = A.cov_restated(main_input(n_rx, rows_in, nb), first=first, count=rows, first_bin=fb, n_bins=span, skip=(sf, sn) if sn else None)
        assert np.array_equal(np.array(g), bits(want).ravel()), c
    cases = [("mvdr", n, beams, loading, 1.0) for n in (1, 2, 5, 64) for beams in (1, 3) for loading in (0.0, 0.5)]
    for c, g in zip(cases, adapt_main(cases)):
        _, n, beams, loading, _ = c
        assert np.array_equal(np.array(g), bits(A.mvdr_restated(main_cov(n), main_steering(beams, n), loading)).ravel()), c
    # a failed pivot is reported, whatever the loading does not mend
    assert adapt_main([("mvdr", 3, 2, 0.0, -1.0), ("mvdr", 3, 2, 0.0, 0.0), ("mvdr", 3, 2, 0.03125, 0.0)], int) == [[0], [0], [1]]


def test_plans(adapt_main):
    T, P, BLK, WAVE, MAXT, RED, MT, MAXTILES = adapt_main([("consts",)], int)[0]
    assert (T, P, BLK, MT) == (A.TILE, A.MAX_PARTS, A.BLOCK, A.SOLVE_THREADS) and WAVE == 64 and MAXTILES == 2 ** 32 - 1
    assert T * 16 * 64 + 16 * 64 <= 160 * 1024 // 2 and P * 64 * 64 * 16 == 32 * 2 ** 20           # two workgroups' tiles in a CU's LDS; the scratch cap
    plan = lambda *a: adapt_main([("covplan",) + a], int)[0]      # n_rx n_rows kept -> K tiles parts block_rows blocks threads reduce_groups lds scratch out supported
    assert plan(1, 1, 1) == [1, 1, 1, 1, 1, 64, 1, 16 * (T + 1), 16, 2, 1]
    assert plan(64, 256, 4096) == [2 ** 20, 2 ** 20 // T, P, 32, 528, 576, 16, 64 * 16 * (T + 1), P * 64 * 64 * 16, 2 * 64 * 64, 1]
    assert plan(64, 1, 1)[5] == MAXT and plan(8, 256, 4096)[3:6] == [4, 10, 64]
    # tiles and parts at the tile and at the cap
    assert [plan(2, 1, k)[1:3] for k in (T - 1, T, T + 1, T * (P - 1), T * P, T * P + 1, T * (P + 1))] == [[1, 1], [1, 1], [2, 2], [P - 1, P - 1], [P, P], [P + 1, P], [P + 1, P]]
    # the block rows at B - 1, B, B + 1 and the workgroup at a wave's blocks
    assert [plan(n, 1, 1)[3:5] for n in (1, BLK - 1 or 1, BLK, BLK + 1, 2 * BLK, 2 * BLK + 1, 63, 64)] == [[1, 1], [1, 1], [1, 1], [2, 3], [2, 3], [3, 6], [32, 528], [32, 528]]
    # the workgroup: the blocks in whole waves, and at least a wave per 8 receivers to stage
    assert [plan(n, 1, 1)[5] for n in (8, 9, 16, 17, 56, 57, 62, 63, 64)] == [64, 128, 128, 192, 448, 512, 512, 576, 576]
    assert all(plan(n, 1, 1)[5] >= 64 * -(-n // 8) and plan(n, 1, 1)[5] >= plan(n, 1, 1)[4] and plan(n, 1, 1)[5] <= MAXT for n in range(1, 65))
    # the limits
    assert plan(65, 1, 1)[-1] == 0 and plan(0, 1, 1)[-1] == 0 and plan(1, 0, 5)[-1] == 0 and plan(1, 5, 0)[-1] == 0
    assert plan(1, 2 ** 32 - 1, T)[1::9] == [2 ** 32 - 1, 1] and plan(1, 2 ** 32 - 1, T + 1)[-1] == 0
    assert plan(1, 2 ** 32 - 1, 2 ** 32 - 1)[0] == (2 ** 32 - 1) ** 2
    # every part owns at least one tile, the parts tile the tiles in order
    for tiles, parts in ((1, 1), (P, P), (P + 1, P), (2 * P - 1, P), (1000003, P), (2 ** 32 - 1, P)):
        b = adapt_main([("parts", tiles, parts)], int)[0]
        assert b[0] == 0 and b[-1] == tiles and all(y > x for x, y in zip(b, b[1:])) and b == [p * tiles // parts for p in range(parts + 1)]
    # the blocks of the triangle, row-major
    want = [[i, j] for i in range(32) for j in range(i + 1)]
    assert adapt_main([("block", b) for b in range(528)], int) == want
    mplan = lambda *a: adapt_main([("mvdrplan",) + a], int)[0]    # n_rx n_beams -> passes lds out supported
    assert mplan(1, 1) == [1, 16 + 16 * MT, 2, 1] and mplan(64, 64) == [1, 16 * 64 * 64 + 16 * 64 * MT, 2 * 64 * 64, 1]
    assert mplan(64, 64)[1] <= 160 * 1024
    assert [mplan(4, n)[0] for n in (1, MT - 1, MT, MT + 1, 1024)] == [1, 1, 1, 2, 1024 // MT]
    assert mplan(65, 1)[-1] == 0 and mplan(64, 65)[-1] == 0 and mplan(4, 1025)[-1] == 0 and mplan(0, 1)[-1] == 0 and mplan(1, 0)[-1] == 0 and mplan(5, 819)[-1] == 1


# ----------------------------------------------------------------------------- 8. the whole chain, on the host
def test_chain_on_the_host(rts):
    """noise + jammer + one target bin -> the covariance without the target's bins -> weights -> rts_beamform_eval: the adaptive beam
    at the target holds the target at its power and the jammer far below the conventional beam's"""
    cube, s, cov, w, beams = A.scene_host(rts)
    sc = A.SCENE
    conv = rts.beamform_eval(cube, s / sc["n_rx"], power=True)
    power = np.abs(beams) ** 2
    tb, bin_ = sc["target_beam"], sc["target_bin"]
    others = np.delete(np.arange(sc["n_bins"]), np.arange(sc["skip"][0], sc["skip"][0] + sc["skip"][1]))
    print("target beam: target bin %.3g (conventional %.3g), elsewhere %.3g (conventional %.3g)"
          % (power[tb, :, bin_].mean(), conv[tb, :, bin_].mean(), power[tb][:, others].mean(), conv[tb][:, others].mean()))
    assert abs(power[tb, :, bin_].mean() / sc["target_power"] - 1.0) < 0.5             # distortionless: the target at its power (+ residue)
    assert power[tb][:, others].mean() < 0.05 * conv[tb][:, others].mean()             # the jammer: more than 13 dB further down
    assert power[tb][:, others].mean() < 0.1 * power[tb, :, bin_].mean()               # ... and the target stands out of it
