"""Direction finding on the host (no GPU): rts_eig_eval and rts_doa_scan_eval against the plain-Python restatement of
tests/doa_ref.py BIT FOR BIT, the eigensolver against numpy.linalg.eigh with bounds measured on this file's own matrices, known
answers, the status rules, the scan's identities (the beamformer's power, Bartlett's a^H R a, Capon's 1 / (a^H A^-1 a)), every refusal
of rts_doa_weights and rts_source_count, rts_amd/csrc/rts_doa.h alone under AddressSanitizer + UndefinedBehaviorSanitizer
(tests/doa/doa_main.cpp: the plans at their edges, the pairing for n = 1 .. 64, the sort, what the evaluators read), and the
two-source scenario: Bartlett sees one source, MUSIC and Capon two."""
import ctypes as C
import math
import os
import shutil
import subprocess

import numpy as np
import pytest

import beam_ref as B
import doa_ref as D

ROOT = D.ROOT
EPS = D.EPS


def bits(a):
    return np.ascontiguousarray(a).view(np.float64)


# ----------------------------------------------------------------------------- 1. against the restatement, bit for bit
@pytest.mark.parametrize("kind", ["full", "deficient", "identity", "diagonal"])
@pytest.mark.parametrize("n", [1, 2, 3, 4, 5, 8])
def test_eig_against_restatement(rts, n, kind):
    A = D.matrix(kind, n)
    values, vectors, sweeps = rts.eig_eval(A, sweeps=True)
    want_values, want_vectors, want_sweeps = D.eig_restated(A)
    assert sweeps == want_sweeps
    assert np.array_equal(bits(values), bits(want_values)) and np.array_equal(bits(vectors), bits(want_vectors)), (n, kind)


@pytest.mark.parametrize("inverse", [False, True])
@pytest.mark.parametrize("n,m", [(1, 1), (2, 1), (2, 2), (3, 2), (4, 4), (5, 3), (8, 6), (8, 8)])
def test_scan_against_restatement(rts, n, m, inverse):
    rng = np.random.default_rng(100 * n + m)
    v = B.random_complex(rng, (m, n)); g = rng.random(m) + 0.25; table = B.random_complex(rng, (7, n))
    got = rts.doa_scan_eval(v, g, table, inverse)
    assert np.array_equal(bits(got), bits(D.scan_restated(v, g, table, inverse))), (n, m, inverse)


def test_scan_inverse_of_zero_is_inf(rts):
    v = np.array([[1.0, -1.0]], np.complex128); table = np.array([[1.0, 1.0], [1.0, 0.0]], np.complex128)     # direction 0 is orthogonal to v
    got = rts.doa_scan_eval(v, [1.0], table, True)
    assert got[0] == math.inf and got[1] == 1.0
    assert np.array_equal(bits(got), bits(D.scan_restated(v, [1.0], table, True)))


# ----------------------------------------------------------------------------- 2. against numpy
NUMPY_N = [2, 3, 8, 21, 32, 33, 63, 64]
NUMPY_KINDS = ["full", "square", "deficient", "one", "identity", "diagonal"]
# the evaluator's own worst case over NUMPY_N x NUMPY_KINDS, measured on the CPU (test_eig_against_numpy prints every figure), and
# the bound the tests hold it to: 4 x that
WORST = dict(values=67.0, residual=68.9, orthogonality=95.8)
BOUND = {k: 4.0 * v for k, v in WORST.items()}
MOST_SWEEPS = 13


@pytest.fixture(scope="module")
def solved(rts):
    """every matrix of this section solved once: {(n, kind): (A, values, vectors, sweeps)}"""
    out = {}
    for n in NUMPY_N:
        for kind in NUMPY_KINDS:
            A = D.matrix(kind, n)
            out[n, kind] = (A,) + rts.eig_eval(A, sweeps=True)
    return out


@pytest.mark.parametrize("kind", NUMPY_KINDS)
@pytest.mark.parametrize("n", NUMPY_N)
def test_eig_against_numpy(solved, n, kind):
    """max |lambda - lambda_ref| / (eps |A|_2), |A V - V Lambda|_2 / (eps |A|_2) and |V^H V - I|_2 / eps against numpy.linalg.eigh.
    The constants cannot be derived and differ by tree; measured over this test's matrices the evaluator's worst case is 67.0 for
    the eigenvalues (n = 63, rank 21), 68.9 for the residual and 95.8 for the orthogonality (both n = 64 with K = 64 snapshots) --
    about n, as one-sided Jacobi should give; the bounds are 4 x those: 268, 275.6, 383.2.  The sweeps: at most 13 (n = 63 and 64
    with K = n) of RTS_EIG_MAX_SWEEPS = 30."""
    A, values, vectors, sweeps = solved[n, kind]
    ev, res, orth = D.accuracy(A, values, vectors)
    print("n = %2d %-9s sweeps %2d  values %6.1f  residual %6.1f  orthogonality %6.1f" % (n, kind, sweeps, ev, res, orth))
    assert np.all(values[:-1] >= values[1:])
    assert ev <= BOUND["values"] and res <= BOUND["residual"] and orth <= BOUND["orthogonality"], (ev, res, orth)
    assert sweeps <= MOST_SWEEPS < D.MAX_SWEEPS
    if kind in ("identity", "diagonal"):
        assert sweeps == 0


@pytest.mark.parametrize("n,kind,rank", [(8, "deficient", 2), (21, "deficient", 7), (63, "deficient", 21), (64, "deficient", 21), (33, "one", 1), (64, "one", 1)])
def test_degenerate_subspaces_as_projectors(solved, n, kind, rank):
    """the zero eigenvalue of a rank-deficient covariance is (n - rank)-fold: its vectors are any basis, so the subspaces are
    compared, never the vectors.  Davis and Kahan: |P - P_ref|_2 = |sin Theta| <= |residual|_2 / gap, the gap here the smallest
    nonzero eigenvalue; the residual is bounded by BOUND["residual"] eps |A|_2, twice for numpy's own"""
    A, values, vectors, _ = solved[n, kind]
    w, U = np.linalg.eigh(A)
    Us = U[:, ::-1][:, :rank]
    P_ref = Us @ Us.conj().T
    Vs = vectors[:rank].T
    P = Vs @ Vs.conj().T
    bound = 2.0 * BOUND["residual"] * EPS * w[-1] / w[::-1][rank - 1]
    err = np.linalg.norm(P - P_ref, 2)
    print("n = %d rank %d: |P - P_ref| = %.3g, bound %.3g" % (n, rank, err, bound))
    assert err <= bound
    assert np.max(np.abs(values[rank:])) <= BOUND["values"] * EPS * w[-1]


def test_diagonal_order_is_stable(rts):
    """a diagonal matrix takes no sweep: V stays I, the values are the diagonal in descending order, ties by ascending column"""
    d = [3.0, 0.0, 1.0, 3.0, 2.0, 0.0, 3.0]
    values, vectors, sweeps = rts.eig_eval(np.diag(d), sweeps=True)
    order = sorted(range(len(d)), key=lambda j: (-d[j], j))
    assert sweeps == 0 and list(values) == [d[j] for j in order]
    assert np.array_equal(vectors, np.eye(len(d))[order])


# ----------------------------------------------------------------------------- 3. known answers
def test_known_answers(rts):
    values, vectors = rts.eig_eval(np.array([[2.0, 1j], [-1j, 2.0]]))
    assert np.allclose(values, [3.0, 1.0], rtol=0, atol=4 * EPS)
    A = np.array([[2.0, 1j], [-1j, 2.0]])
    for k in range(2):
        assert np.allclose(A @ vectors[k], values[k] * vectors[k], rtol=0, atol=8 * EPS)
    rng = np.random.default_rng(5)
    a = B.random_complex(rng, 6)
    values, vectors = rts.eig_eval(D.hermitian(np.outer(a, a.conj())))
    n2 = float(np.vdot(a, a).real)
    assert abs(values[0] - n2) <= 16 * EPS * n2 and np.max(np.abs(values[1:])) <= 16 * EPS * n2
    assert abs(abs(np.vdot(vectors[0], a)) - math.sqrt(n2)) <= 16 * EPS * math.sqrt(n2)        # row 0 is parallel to a


# ----------------------------------------------------------------------------- 4. status
def test_status(rts):
    L = rts.L.lib()
    A = D.matrix("full", 4)
    up = A.copy(); up[0, 2] = np.nan; up[1, 3] = complex(0.0, np.inf)                        # the upper triangle is never read
    assert all(np.array_equal(bits(x), bits(y)) for x, y in zip(rts.eig_eval(up), rts.eig_eval(A)))
    im = A.copy(); im[2, 2] = complex(A[2, 2].real, np.nan)                                   # nor the diagonal's imaginary part
    assert all(np.array_equal(bits(x), bits(y)) for x, y in zip(rts.eig_eval(im), rts.eig_eval(A)))
    for i, j, bad in [(2, 1, np.nan), (3, 0, complex(0.0, np.nan)), (1, 1, np.inf), (3, 3, -np.inf)]:
        low = A.copy(); low[i, j] = bad
        values = np.full(4, 7.0); vectors = np.full((4, 4), 7.0 + 7.0j); sweeps = C.c_uint32(99)
        rc = L.rts_eig_eval(rts.ptr(low.view(np.float64)), 4, rts.ptr(values), rts.ptr(vectors.view(np.float64)), C.byref(sweeps))
        assert rc == rts.L.RTS_ERR_INVALID and b"status 2" in L.rts_last_error()
        assert np.all(values == 7.0) and np.all(vectors == 7.0 + 7.0j) and sweeps.value == 99  # the outputs are untouched
    for n in (0, D.MAX_N + 1):
        assert L.rts_eig_eval(rts.ptr(A.view(np.float64)), n, rts.ptr(np.zeros(4)), rts.ptr(np.zeros(32)), None) == rts.L.RTS_ERR_INVALID
    assert L.rts_eig_eval(None, 4, rts.ptr(np.zeros(4)), rts.ptr(np.zeros(32)), None) == rts.L.RTS_ERR_INVALID
    assert L.rts_eig_eval(rts.ptr(A.view(np.float64)), 4, None, rts.ptr(np.zeros(32)), None) == rts.L.RTS_ERR_INVALID


# ----------------------------------------------------------------------------- 5. the scan's identities
def test_scan_of_one_vector_is_the_beamformer(rts):
    rng = np.random.default_rng(11)
    for n in (1, 3, 8, 21):
        table = B.random_complex(rng, (37, n)); w = B.random_complex(rng, (1, n))
        cube = np.ascontiguousarray(table.T)[:, None, :]                                       # a cube of one row whose bins are the directions
        assert np.array_equal(bits(rts.doa_scan_eval(w, [1.0], table)), bits(rts.beamform_eval(cube, w, power=True)[0, 0]))


@pytest.mark.parametrize("n,K", [(8, 256), (21, 40), (64, 300), (33, 5)])
def test_bartlett_against_numpy(rts, n, K):
    rng = np.random.default_rng(n + K)
    R = D.sample_cov(rng, n, K); table = B.random_complex(rng, (50, n))
    values, vectors = rts.eig_eval(R)
    first, g, inverse = rts.doa_weights("bartlett", values)
    got = rts.doa_scan_eval(vectors[first:first + len(g)], g, table, inverse)
    want = np.einsum("di,ij,dj->d", table.conj(), R, table).real
    assert first == 0 and not inverse and np.allclose(got, want, rtol=1e-10, atol=1e-12 * want.max())


@pytest.mark.parametrize("n,K,loading", [(8, 256, 0.0), (21, 40, 0.0), (64, 300, 0.01), (33, 5, 0.5), (16, 16, 1e-3)])
def test_capon_against_numpy(rts, n, K, loading):
    """1 / Re(a^H A^-1 a), A = R + loading I, from numpy.linalg.solve.  The eigenpairs are those of A + E with |E|_2 <=
    BOUND["residual"] eps |A|_2 (section 2); the quadratic form of the inverse moves by at most cond(A) |E| / |A| of itself, and numpy's
    solve by its own n eps cond(A): the relative bound is (BOUND["residual"] + n) eps cond(A)"""
    rng = np.random.default_rng(7 * n + K)
    R = D.sample_cov(rng, n, K); table = B.random_complex(rng, (50, n))
    A = R + loading * np.eye(n)
    values, vectors = rts.eig_eval(R)
    first, g, inverse = rts.doa_weights("capon", values, loading=loading)
    got = rts.doa_scan_eval(vectors[first:first + len(g)], g, table, inverse)
    want = 1.0 / np.einsum("di,id->d", table.conj(), np.linalg.solve(A, table.T)).real
    bound = (BOUND["residual"] + n) * EPS * np.linalg.cond(A)
    err = np.max(np.abs(got / want - 1.0))
    print("n = %d K = %d: cond %.3g, error %.3g, bound %.3g" % (n, K, np.linalg.cond(A), err, bound))
    assert first == 0 and inverse and len(g) == n and err <= bound


def test_music_is_the_noise_projector(rts):
    rng = np.random.default_rng(3)
    n, K, ns = 8, 200, 3
    R = D.sample_cov(rng, n, K); table = B.random_complex(rng, (20, n))
    values, vectors = rts.eig_eval(R)
    first, g, inverse = rts.doa_weights("music", values, ns)
    assert first == ns and inverse and np.array_equal(g, np.ones(n - ns))
    got = rts.doa_scan_eval(vectors[first:], g, table, inverse)
    w, U = np.linalg.eigh(R)
    Un = U[:, :n - ns]
    want = 1.0 / np.sum(np.abs(table.conj() @ Un) ** 2, axis=1)
    assert np.allclose(got, want, rtol=2.0 * BOUND["residual"] * EPS * w[-1] / (w[n - ns] - w[n - ns - 1]) * 10.0, atol=0)


def test_scan_eval_refusals(rts):
    L = rts.L.lib()
    v = np.ones((2, 3), np.complex128); g = np.ones(2); a = np.ones((3, 5), np.complex128); out = np.full(5, 7.0)
    call = lambda vv=v, gg=g, n=3, m=2, aa=a, nd=5, fl=0, oo=out: L.rts_doa_scan_eval(rts.ptr(vv.view(np.float64)) if vv is not None else None, rts.ptr(gg) if gg is not None else None,
                                                                                    n, m, rts.ptr(aa.view(np.float64)) if aa is not None else None, nd, fl, rts.ptr(oo) if oo is not None else None)
    assert call() == rts.L.RTS_OK and np.all(out == 3.0 * 3.0 * 2.0)
    out[:] = 7.0
    for kw in (dict(n=0), dict(n=D.MAX_N + 1), dict(m=0), dict(m=4), dict(nd=0), dict(fl=2), dict(vv=None), dict(gg=None), dict(aa=None), dict(oo=None),
               dict(gg=np.array([1.0, np.nan])), dict(gg=np.array([np.inf, 1.0])), dict(nd=(2 ** 31 - 1) * 256 + 1)):
        assert call(**kw) == rts.L.RTS_ERR_INVALID, kw
    assert np.all(out == 7.0)


# ----------------------------------------------------------------------------- 6. rts_doa_weights, rts_source_count
def test_doa_weights(rts):
    lam = np.array([5.0, 2.0, 0.5, 0.25])
    first, g, inv = rts.doa_weights("bartlett", lam, n_sources=99, loading=3.0)               # neither is looked at
    assert (first, inv) == (0, False) and np.array_equal(g, lam)
    first, g, inv = rts.doa_weights("capon", lam, loading=0.5)
    assert (first, inv) == (0, True) and np.array_equal(g, [1.0 / (x + 0.5) for x in lam])
    first, g, inv = rts.doa_weights("music", lam, 0)
    assert (first, inv) == (0, True) and np.array_equal(g, np.ones(4))
    first, g, inv = rts.doa_weights("music", lam, 3)
    assert (first, inv) == (3, True) and np.array_equal(g, np.ones(1))
    first, g, inv = rts.doa_weights("capon", np.array([1.0, 0.0, -0.25]), loading=0.5)          # lambda + loading > 0 is what counts
    assert np.array_equal(g, [1.0 / 1.5, 2.0, 4.0])


def test_doa_weights_refusals(rts):
    lam = np.array([5.0, 2.0, 0.5, 0.25])
    bad = [dict(method=3), dict(method="music", n_sources=4), dict(method="music", n_sources=5), dict(method="capon", values=[1.0, 0.0]),
           dict(method="capon", values=[1.0, -0.5], loading=0.5), dict(method="capon", values=[1.0, -0.5], loading=0.25)]
    bad += [dict(method=m, loading=x) for m in ("bartlett", "capon", "music") for x in (-1e-300, -1.0, np.nan, np.inf)]
    bad += [dict(method=m, values=[1.0, x]) for m in ("bartlett", "capon", "music") for x in (np.nan, np.inf, -np.inf)]
    for kw in bad:
        with pytest.raises(rts.L.RtsError):
            rts.doa_weights(kw.get("method"), kw.get("values", lam), kw.get("n_sources", 1), kw.get("loading", 0.0))
    L = rts.L.lib()
    f, m, fl = C.c_uint32(7), C.c_uint32(7), C.c_uint32(7); g = np.full(4, 7.0)
    ok = lambda: (rts.L.RTS_DOA_MUSIC, rts.ptr(lam), 4, 1, 0.0, C.byref(f), C.byref(m), rts.ptr(g), C.byref(fl))
    for i in (1, 5, 6, 7, 8):                                                                  # each pointer NULL in turn
        args = list(ok()); args[i] = None
        assert L.rts_doa_weights(*args) == rts.L.RTS_ERR_INVALID
    for n in (0, D.MAX_N + 1):
        args = list(ok()); args[2] = n
        assert L.rts_doa_weights(*args) == rts.L.RTS_ERR_INVALID
    args = list(ok()); args[3] = 4
    assert L.rts_doa_weights(*args) == rts.L.RTS_ERR_INVALID
    assert (f.value, m.value, fl.value) == (7, 7, 7) and np.all(g == 7.0)                      # a refused call leaves the outputs untouched
    assert L.rts_doa_weights(*ok()) == rts.L.RTS_OK and (f.value, m.value, fl.value) == (1, 3, rts.L.RTS_DOA_INVERSE)


def source_count_restated(lam, K, criterion):
    n = len(lam); best = None
    for k in range(n):
        tail = [float(x) for x in lam[k:]]; cnt = n - k
        L = K * cnt * (math.log(sum(tail) / cnt) - sum(math.log(x) for x in tail) / cnt)
        pen = k * (2 * n - k)
        v = 2.0 * L + 2.0 * pen if criterion == "aic" else L + 0.5 * pen * math.log(K)
        if best is None or v < best[0]:
            best = (v, k)
    return best[1]


def test_source_count(rts):
    for lam, K in [([10.0, 8.0, 0.011, 0.01, 0.0101, 0.0098], 100), ([5.0, 1.0, 1.0, 1.0], 50), ([1.0, 1.0, 1.0], 1000), ([4.0], 10),
                   ([9.0, 3.0, 1.0, 0.3, 0.1], 20)]:
        lam = sorted(lam, reverse=True)
        for crit in ("aic", "mdl"):
            assert rts.source_count(lam, K, crit) == source_count_restated(lam, K, crit), (lam, K, crit)
    assert rts.source_count([10.0, 8.0, 0.0101, 0.01, 0.0099, 0.0098], 100, "mdl") == 2
    assert rts.source_count([1.0, 1.0, 1.0], 1000, "mdl") == 0


def test_source_count_refusals(rts):
    for lam, K, crit in [([2.0, 1.0, 0.0], 10, "mdl"), ([2.0, 1.0, -1.0], 10, "aic"), ([2.0, np.nan], 10, "mdl"), ([np.inf, 1.0], 10, "mdl"),
                         ([1.0, 2.0], 10, "mdl"), ([2.0, 1.0], 0, "mdl"), ([2.0, 1.0], 10, 2), ([], 10, "mdl"), ([1.0] * (D.MAX_N + 1), 10, "mdl")]:
        with pytest.raises(rts.L.RtsError):
            rts.source_count(lam, K, crit)
    L = rts.L.lib()
    k = C.c_uint32(7)
    assert L.rts_source_count(None, 2, 10, 0, C.byref(k)) == rts.L.RTS_ERR_INVALID
    assert L.rts_source_count(rts.ptr(np.array([2.0, 1.0])), 2, 10, 0, None) == rts.L.RTS_ERR_INVALID
    assert L.rts_source_count(rts.ptr(np.array([2.0, 0.0])), 2, 10, 0, C.byref(k)) == rts.L.RTS_ERR_INVALID and k.value == 7


# ----------------------------------------------------------------------------- 7. rts_doa.h alone, under the sanitizers
@pytest.fixture(scope="module")
def doa_main(tmp_path_factory):
    gxx = shutil.which("g++")
    if not gxx:
        pytest.skip("no g++")
    rt = subprocess.run([gxx, "-print-file-name=libasan.so"], capture_output=True, text=True).stdout.strip()
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"] if os.path.isabs(rt) and os.path.exists(rt) else []
    exe = str(tmp_path_factory.mktemp("doa") / "doa_main")
    subprocess.check_call([gxx, "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-ffp-contract=off"] + san + ["-I", os.path.join(ROOT, "rts_amd", "csrc"),
                           os.path.join(ROOT, "tests", "doa", "doa_main.cpp"), "-o", exe])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:verify_asan_link_order=0", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")

    def ask(cases, kind=float):
        text = "".join(" ".join(repr(x) if isinstance(x, float) else str(x) for x in c) + "\n" for c in cases)
        r = subprocess.run([exe], input=text, capture_output=True, text=True, env=env, timeout=120)
        assert r.returncode == 0, r.stderr[-3000:]
        out = [[kind(x) for x in line.split()] for line in r.stdout.splitlines()]
        assert len(out) == len(cases)
        return out
    return ask


def main_cov(n, scale=1.0):
    """the matrix tests/doa/doa_main.cpp fills"""
    i = np.arange(n)[:, None]; j = np.arange(n)[None, :]
    re = np.where(i == j, (n + 0.25 * i) * scale, (((i * 7 + j * 3) % 5) - 2.0) / 8.0)
    return re + 1j * ((((i * 5 + j * 11) % 7) - 3.0) / 16.0)


def main_vectors(rows, n):
    k = np.arange(rows)[:, None]; r = np.arange(n)[None, :]
    return (((k * 7 + r * 3) % 11) - 5.0) / 8.0 + 1j * ((((k * 5 + r * 13) % 9) - 4.0) / 16.0 + 0.03125)


def main_table(n, n_dirs):
    """[n_dirs][n]: the host layout of the driver's element-major table"""
    d = np.arange(n_dirs)[:, None]; r = np.arange(n)[None, :]
    return (((r * 3 + d * 5) % 13) - 6.0) / 4.0 + 1j * ((((r * 11 + d * 7) % 17) - 8.0) / 8.0)


def test_header_alone_reads_only_what_it_is_given(rts, doa_main):
    """the matrix's upper triangle and diagonal imaginary parts and the table's rows outside first .. first + m - 1 are poisoned in the
    driver; outputs and work arrays are heap arrays of exactly their sizes: a read or write beyond them ends the run.  The results
    equal the library's evaluators on the same inputs, bit for bit"""
    ns = [1, 2, 3, 5, 8, 21, 64]
    for n, got in zip(ns, doa_main([("eig", n, 1.0) for n in ns])):
        values, vectors, sweeps = rts.eig_eval(main_cov(n), sweeps=True)
        assert got[0] == 0 and got[1] == sweeps
        assert np.array_equal(bits(np.array(got[2:2 + n])), bits(values)) and np.array_equal(bits(np.array(got[2 + n:])), bits(vectors).ravel()), n
    cases = [(1, 1, 0, 1, 1, 0), (3, 3, 0, 3, 5, 1), (8, 8, 2, 6, 9, 1), (21, 21, 20, 1, 3, 0), (64, 64, 2, 62, 2, 1), (5, 5, 1, 3, 4, 0)]
    for (n, rows, first, m, nd, inv), got in zip(cases, doa_main([("scan",) + c for c in cases])):
        want = rts.doa_scan_eval(main_vectors(rows, n)[first:first + m], 0.5 + 0.25 * np.arange(m), main_table(n, nd), bool(inv))
        assert np.array_equal(bits(np.array(got)), bits(want)), (n, rows, first, m, nd, inv)
    assert doa_main([("eig", 3, float("nan")), ("eig", 3, float("inf"))], lambda x: int(float(x))) == [[2, 0], [2, 0]]


def test_plans(doa_main):
    SW, ET, ST, RXT, VT, GRID, MAXN = doa_main([("consts",)], int)[0]
    assert (SW, ET, ST, RXT, VT, MAXN) == (D.MAX_SWEEPS, D.EIG_THREADS, D.SCAN_THREADS, D.RX_TILE, D.VEC_TILE, D.MAX_N) and GRID == 2 ** 31 - 1
    eplan = lambda n: doa_main([("eigplan", n)], int)[0]          # n -> rounds slots lds values vectors supported
    assert eplan(0)[-1] == 0 and eplan(MAXN + 1)[-1] == 0
    for n in (1, 2, 3, 63, 64):
        M = n + n % 2
        assert eplan(n) == [M - 1, M // 2, 32 * n * n, n, 2 * n * n, 1]
    assert eplan(MAXN)[1] <= ET and eplan(MAXN)[2] == 128 * 1024          # a slot per thread; X and V fill 128 KiB of the CU's 160
    splan = lambda *a: doa_main([("scanplan",) + a], int)[0]      # n m n_dirs -> groups rx_tiles vec_tiles lds out supported
    assert splan(8, 6, 1) == [1, 1, 1, 16 * 48 + 48, 1, 1]
    assert splan(64, 62, 2 ** 20) == [4096, 8, 4, 16 * 62 * 64 + 8 * 62, 2 ** 20, 1]
    assert splan(64, 64, 1)[3] == 64 * 1024 + 512
    for nd, groups in [(ST - 1, 1), (ST, 1), (ST + 1, 2)]:
        assert splan(3, 2, nd)[0] == groups
    for n, tiles in [(RXT - 1, 1), (RXT, 1), (RXT + 1, 2)]:
        assert splan(n, 1, 5)[1] == tiles
    for m, tiles in [(VT - 1, 1), (VT, 1), (VT + 1, 2)]:
        assert splan(64, m, 5)[2] == tiles
    assert splan(0, 1, 5)[-1] == 0 and splan(MAXN + 1, 1, 5)[-1] == 0 and splan(4, 0, 5)[-1] == 0 and splan(4, MAXN + 1, 5)[-1] == 0 and splan(4, 4, 0)[-1] == 0
    # the grid's edge, and group counts that do not fit 32 bits: refused, never wrapped
    assert splan(4, 4, GRID * ST) == [GRID, 1, 1, 16 * 16 + 32, GRID * ST, 1]
    for nd in (GRID * ST + 1, 2 ** 32 * ST, 2 ** 32 * ST + 1, 2 ** 40 * ST + 3, 2 ** 64 - 1):
        assert splan(4, 4, nd)[0] == 0 and splan(4, 4, nd)[-1] == 0, nd


def test_pairing(doa_main):
    """for n = 1 .. 64: every pair exactly once per sweep, the pairs of a round disjoint, an odd n with one bye per round -- and the
    header's table is the restatement's"""
    ns = list(range(1, D.MAX_N + 1))
    for n, got in zip(ns, doa_main([("pairs", n) for n in ns], int)):
        M = n + n % 2
        assert got[:2] == [M - 1, M // 2]
        flat = list(zip(got[2::2], got[3::2]))
        assert len(flat) == (M - 1) * (M // 2)
        table = [flat[r * (M // 2):(r + 1) * (M // 2)] for r in range(M - 1)]
        for r, pairs in enumerate(table):
            live = [pq for pq in pairs if pq != (n, n)]
            assert len(pairs) - len(live) == n % 2                                              # the bye
            assert all(p < q < n for p, q in live)
            cols = [c for pq in live for c in pq]
            assert len(set(cols)) == len(cols)                                                  # disjoint within the round
            assert live == D.rounds(n)[r]
        everyone = [pq for pairs in table for pq in pairs if pq != (n, n)]
        assert sorted(everyone) == [(p, q) for p in range(n) for q in range(p + 1, n)]          # every pair exactly once


def test_sort(doa_main):
    cases = [[1.0], [1.0, 2.0], [2.0, 2.0, 2.0], [0.0, 3.0, 0.0, 3.0, 1.0], [-1.0, 0.0, -0.0, 5.0], [float(i % 7) for i in range(64)]]
    for lam, got in zip(cases, doa_main([("rank",) + tuple(c) for c in cases], int)):
        order = sorted(range(len(lam)), key=lambda j: (-lam[j], j))
        assert got == [order.index(j) for j in range(len(lam))]


def test_pure_functions_in_the_driver(doa_main):
    lam = (5.0, 2.0, 0.5, 0.25)
    got = doa_main([("weights", 0, 0, 0.0) + lam, ("weights", 1, 0, 0.5) + lam, ("weights", 2, 1, 0.0) + lam, ("weights", 2, 4, 0.0) + lam,
                    ("weights", 3, 0, 0.0) + lam, ("weights", 1, 0, -1.0) + lam, ("weights", 1, 0, 0.0, 1.0, 0.0), ("weights", 0, 0, 0.0, 1.0, float("nan"))])
    assert got[0] == [0, 0, 4, 0] + list(lam) and got[1] == [0, 0, 4, 1] + [1.0 / (x + 0.5) for x in lam] and got[2] == [0, 1, 3, 1, 1.0, 1.0, 1.0]
    assert [g[0] for g in got[3:]] == [4, 1, 2, 5, 3]
    assert doa_main([("count", 100, 1, 10.0, 8.0, 0.0101, 0.01, 0.0099, 0.0098), ("count", 100, 0, 10.0, 8.0, 0.0101, 0.01, 0.0099, 0.0098)], int) == [[2], [2]]


# ----------------------------------------------------------------------------- 8. the scenario
def test_two_sources_six_degrees_apart(rts):
    """8 elements at half a wavelength, sources at +-3 degrees, 20 dB SNR, 256 snapshots, a 0.25 degree grid: the conventional
    spectrum shows one peak, MUSIC and Capon two; AIC and MDL count two sources"""
    grid = np.degrees(D.SCENE["grid"])
    bartlett, values = D.scene_host(rts, "bartlett")
    assert len(D.peaks(bartlett)) == 1
    assert rts.source_count(values, D.SCENE["K"], "mdl") == 2 and rts.source_count(values, D.SCENE["K"], "aic") == 2
    music, _ = D.scene_host(rts, "music", 2)
    pk = D.peaks(music)
    print("MUSIC peaks at", grid[pk], "Bartlett's at", grid[D.peaks(bartlett)])
    assert len(pk) == 2 and abs(grid[pk[0]] + 3.0) <= 0.25 + 1e-9 and abs(grid[pk[1]] - 3.0) <= 0.25 + 1e-9
    assert np.array_equal(bits(D.scene_host(rts, "music")[0]), bits(music))                    # n_sources None: MDL's 2
    capon, _ = D.scene_host(rts, "capon")
    assert len(D.peaks(capon)) == 2
