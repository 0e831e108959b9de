"""Ordered-statistic CFAR on the host (no GPU): rts_cfar_os_alpha against the false-alarm law it inverts, rts_cfar_os_eval against an
independent numpy restatement of include/rts_amd.h (RtsCfarOsParams; tests/cfar_os_ref.py) on the shapes of the GPU test, the
masking that cell averaging suffers and OS does not, the false-alarm rate on Gaussian noise, the validation of malformed records,
and rts_amd/csrc/rts_cfar_os.h (with the rts_cfar.h every detector shares) alone under AddressSanitizer + UndefinedBehaviorSanitizer (tests/cfar_os/cfar_os_main.cpp).

An order statistic has no summation order: integer fields, power and noise are compared exactly, the threshold exactly when alpha
is given and to 1e-11 relative with pfa (the bound rts_cfar_os_alpha documents for the law at its alpha; the restatement's alpha is
its own bisection).  Case 7 of the shared shapes carries extra planted cells: see tests/cfar_os_ref.py."""
import ctypes as C
import math
import os
import shutil
import subprocess

import numpy as np
import pytest

import cfar_os_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T0, DT, PRI = 2.0e-6, 5.0e-9, 1.0e-3


# ----------------------------------------------------------------------------- alpha
@pytest.mark.parametrize("n,k,pfa", [(248, 186, 1e-2), (1, 1, 1e-3), (1088, 816, 1e-6), (17, 13, 0.5)])
def test_alpha_inverts_the_law(rts, n, k, pfa):
    a = rts.cfar_os_alpha(n, k, pfa)
    got = R.law(n, k, a)
    print("alpha(%d, %d, %g) = %.17g: law / pfa - 1 = %.3g" % (n, k, pfa, a, got / pfa - 1))
    assert a > 0 and abs(got - pfa) <= 1e-11 * pfa
    if (n, k) == (1, 1):
        assert abs(a - 999.0) <= 1e-12 * 999.0               # the closed form 1 / pfa - 1


def test_alpha_refusals(rts):
    from rts_amd import _lib as L
    lib = L.lib()
    a = C.c_double(7.25)
    for n, k, pfa, word in ((0, 1, 1e-3, b"n_train"), (8, 0, 1e-3, b"rank"), (8, 9, 1e-3, b"rank"), (8, 4, 0.0, b"pfa"), (8, 4, 1.0, b"pfa"),
                            (8, 4, -0.5, b"pfa"), (8, 4, math.nan, b"pfa")):
        assert lib.rts_cfar_os_alpha(n, k, pfa, C.byref(a)) == L.RTS_ERR_INVALID, (n, k, pfa)
        assert word in lib.rts_last_error(), (word, lib.rts_last_error())
        assert a.value == 7.25
    assert lib.rts_cfar_os_alpha(8, 4, 1e-3, None) == L.RTS_ERR_INVALID
    assert lib.rts_cfar_os_alpha(8, 8, 1e-3, C.byref(a)) == L.RTS_OK and a.value > 0


# ----------------------------------------------------------------------------- the evaluator against the restatement
@pytest.mark.parametrize("index", range(len(R.CASES)))
def test_eval_against_restatement(rts, index):
    guard, train, _, n_rx, nd, nb, pfa, alpha, local_max = R.CASES[index]
    z, P, want = R.case_expectation(index, T0, DT, PRI)        # (checks the margin and the 5 n_rx detections)
    got = rts.cfar_os_eval(z, guard, train, R.case_rank(R.CASES[index]), pfa=pfa, alpha=alpha, local_max=local_max, pri=PRI, t0=T0, dt=DT)
    R.assert_same_list(got, want, threshold_rtol=0.0 if alpha is not None else 1e-11)
    assert np.array_equal(got["threshold"] < got["power"], np.ones(len(got), bool))


# ----------------------------------------------------------------------------- masking
def test_masking(rts):
    """five 40 dB cells and a 16 dB cell four bins from one of them: OS at rank 186 of 248 reports all six, the weak one with noise
    1.3017 and threshold 8.94 against its power 39.8; cell averaging reports five and misses it with a threshold of 1 900"""
    z, strong, weak = R.masking_map()
    P = z.real * z.real + z.imag * z.imag
    got = rts.cfar_os_eval(z, (2, 2), (8, 4), 186, pfa=1e-4, local_max=False)
    cells = sorted(zip(got["doppler_bin"].tolist(), got["range_bin"].tolist()))
    assert cells == sorted(strong + [weak])
    w = got[(got["doppler_bin"] == weak[0]) & (got["range_bin"] == weak[1])][0]
    print("weak cell: power %.4g noise %.5g threshold %.4g" % (w["power"], w["noise"], w["threshold"]))
    assert abs(w["noise"] - 1.3017) < 1e-3 and abs(w["threshold"] - 8.94) < 1e-2
    noise, thr, n, det = R.os_ref(P, 2, 2, 8, 4, 186, 1e-4, None, False)
    assert sorted(zip(*(a.tolist() for a in np.nonzero(det)[1:]))) == sorted(strong + [weak])
    thr_ca, det_ca = R.ca_ref(P, 2, 2, 8, 4, 1e-4)
    assert sorted(zip(*(a.tolist() for a in np.nonzero(det_ca)[1:]))) == sorted(strong)
    print("CA threshold at the weak cell: %.4g" % thr_ca[0][weak])
    assert 1800 < thr_ca[0][weak] < 2000 and P[0][weak] < 40


# ----------------------------------------------------------------------------- false-alarm rate
def test_false_alarm_rate(rts):
    """rts_noise_eval's unit-power noise, 2 x 64 x 1 024, through an orthonormal DFT over the pulse axis: the count at pfa 1e-2 lies
    within 5 sd of the binomial mean, 1 310.72 +- 5 x 36.0, and the first and last ten range bins hold between 1 and 51 of them
    (mean 25.6, sd 5.03)"""
    n_rx, n_p, nb, pfa = 2, 64, 1024, 1e-2
    cube = rts.noise_eval(12345, np.arange(n_rx * n_p * nb, dtype=np.uint64), 1.0).reshape(n_rx, n_p, nb)
    z = np.fft.fft(cube, axis=1) / 8.0
    got = rts.cfar_os_eval(z, (2, 2), (8, 4), 186, pfa=pfa, local_max=False)
    cells = n_rx * n_p * nb
    mean, sd = cells * pfa, math.sqrt(cells * pfa * (1 - pfa))
    assert abs(mean - 1310.72) < 1e-9 and abs(sd - 36.0) < 0.03
    edge = int(np.count_nonzero((got["range_bin"] < 10) | (got["range_bin"] >= nb - 10)))
    print("false alarms: %d (%.2f sd from the mean), %d in the edge bins" % (len(got), (len(got) - mean) / sd, edge))
    assert abs(len(got) - mean) < 5 * sd, (len(got), mean, sd)
    assert 1 <= edge <= 51, edge
    assert np.all(got["power"] > got["threshold"])


# ----------------------------------------------------------------------------- validation
def raw_case(L, n_rx=2, nd=16, nb=64):
    q = L.RtsCubeParams(n_rx, 1, nb, 0, 0.0, 1.0)
    rng = np.random.default_rng(1)
    z = R.planted_map(rng, n_rx, nd, nb)
    p = L.RtsCfarOsParams()
    p.guard_range, p.guard_doppler, p.train_range, p.train_doppler, p.rank, p.flags = 1, 1, 4, 2, 30, 0
    p.pfa, p.alpha, p.pri, p.max_detections = 1e-3, 0.0, 0.0, 0
    return q, np.ascontiguousarray(z), nd, p


def bad_os_params():
    """(changes, word the message must hold): every refusal of the header on the record's fields"""
    return [
        (dict(flags=2), b"flags"), (dict(train_range=0, train_doppler=0), b"train"), (dict(guard_range=9, train_range=8), b"guard_range"),
        (dict(guard_doppler=10, train_doppler=7), b"guard_doppler"), (dict(guard_doppler=4, train_doppler=4), b"n_doppler"),
        (dict(guard_range=60, train_range=4), b"guard_range"), (dict(train_range=17), b"train_range"),
        (dict(pfa=1.0), b"pfa"), (dict(pfa=-0.1), b"pfa"), (dict(pfa=math.nan), b"pfa"), (dict(pfa=1e-3, alpha=2.0), b"pfa"),
        (dict(pfa=0.0, alpha=0.0), b"pfa"), (dict(pfa=0.0, alpha=-1.0), b"alpha"), (dict(pfa=0.0, alpha=math.inf), b"alpha"),
        (dict(pri=-1.0), b"pri"), (dict(pri=math.inf), b"pri"), (dict(pri=math.nan), b"pri"),
        (dict(rank=0), b"rank"), (dict(rank=69), b"rank"),                      # N0 = 11 x 7 - 3 x 3 = 68
        (dict(reserved0=1), b"reserved"),
    ]


def test_malformed_records_are_rejected(rts):
    from rts_amd import _lib as L
    lib = L.lib()
    q, z, nd, p = raw_case(L)
    n0 = R.n0_of((1, 1), (4, 2))
    assert n0 == 68
    out = np.zeros(4096, L.DETECTION_DTYPE)
    n = C.c_uint32(99)

    def run(q_, z_, nd_, p_, out_=out, cap=4096, n_=n):
        return lib.rts_cfar_os_eval(C.byref(q_) if q_ is not None else None, z_.ctypes.data if z_ is not None else None, nd_,
                                    C.byref(p_) if p_ is not None else None, out_.ctypes.data if out_ is not None else None, cap,
                                    C.byref(n_) if n_ is not None else None)
    assert run(q, z, nd, p) == L.RTS_OK and n.value >= 10
    full = out[:n.value].copy()
    for changes, word in bad_os_params():
        q, z, nd, p = raw_case(L)
        for k, v in changes.items():
            setattr(p, k, v)
        out[:] = np.zeros(1, L.DETECTION_DTYPE); out["power"] = 7.25; n.value = 99
        assert run(q, z, nd, p) == L.RTS_ERR_INVALID, changes
        assert word in lib.rts_last_error(), (changes, lib.rts_last_error())
        assert np.all(out["power"] == 7.25) and n.value == 99, changes
    q, z, nd, p = raw_case(L)
    p.reserved[1] = 1
    assert run(q, z, nd, p) == L.RTS_ERR_INVALID and b"reserved" in lib.rts_last_error()
    q, z, nd, p = raw_case(L)
    p.rank = n0                                               # the largest rank is accepted
    assert run(q, z, nd, p) == L.RTS_OK
    small = L.RtsCubeParams(1, 1, 16, 0, 0.0, 1.0)            # Gr + Tr >= n_bins
    p.rank, p.guard_range, p.train_range = 30, 4, 12
    assert run(small, z, nd, p) == L.RTS_ERR_INVALID and b"n_bins" in lib.rts_last_error()
    q, z, nd, p = raw_case(L)
    assert run(None, z, nd, p) == L.RTS_ERR_INVALID and run(q, None, nd, p) == L.RTS_ERR_INVALID and run(q, z, nd, None) == L.RTS_ERR_INVALID
    assert run(q, z, 0, p) == L.RTS_ERR_INVALID and b"n_doppler" in lib.rts_last_error()
    assert run(q, z, nd, p, n_=None) == L.RTS_ERR_INVALID and run(q, z, nd, p, out_=None) == L.RTS_ERR_INVALID
    # capacity below the total: RTS_ERR_CAPACITY, *n_out = the total, the first records in order
    out[:] = np.zeros(1, L.DETECTION_DTYPE); n.value = 0
    assert run(q, z, nd, p, cap=3) == L.RTS_ERR_CAPACITY and n.value == len(full)
    assert out[:3].tobytes() == full[:3].tobytes() and np.count_nonzero(out[3:]["power"]) == 0
    assert run(q, z, nd, p, out_=None, cap=0) == L.RTS_ERR_CAPACITY and n.value == len(full)


# ----------------------------------------------------------------------------- rts_cfar_os.h alone, under the sanitizers
@pytest.fixture(scope="module")
def os_main(tmp_path_factory):
    gxx = shutil.which("g++")
    if not gxx:
        pytest.skip("no g++")
    rt = subprocess.run([gxx, "-print-file-name=libasan.so"], capture_output=True, text=True).stdout.strip()
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"] if os.path.isabs(rt) and os.path.exists(rt) else []
    exe = str(tmp_path_factory.mktemp("cfar_os") / "cfar_os_main")
    subprocess.check_call([gxx, "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-ffp-contract=off"] + san + ["-I", os.path.join(ROOT, "rts_amd", "csrc"),
                           os.path.join(ROOT, "tests", "cfar_os", "cfar_os_main.cpp"), "-o", exe])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:verify_asan_link_order=0", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")

    def ask(cases, kind=float):
        text = "".join(" ".join(repr(x) if isinstance(x, float) else str(x) for x in c) + "\n" for c in cases)
        r = subprocess.run([exe], input=text, capture_output=True, text=True, env=env, timeout=120)
        assert r.returncode == 0, r.stderr[-3000:]
        out = [[kind(x) for x in line.split()] for line in r.stdout.splitlines()]
        assert len(out) == len(cases)
        return out
    return ask


WINDOWS = [((2, 2), (8, 4)), ((0, 0), (16, 16)), ((16, 0), (0, 1)), ((0, 2), (16, 0)), ((0, 0), (0, 16)), ((4, 0), (2, 1)), ((3, 1), (5, 6))]


def counts_ref(gr, gd, tr, td, nb):
    """the training cells of every range bin, counted one offset at a time"""
    r = np.arange(nb)
    n = np.zeros(nb, np.int64)
    for dk in range(-(gd + td), gd + td + 1):
        for dr in range(-(gr + tr), gr + tr + 1):
            if not (abs(dk) <= gd and abs(dr) <= gr):
                n += (r + dr >= 0) & (r + dr < nb)
    return n


def test_header_alone_window_and_rank(os_main):
    got = os_main([("n0", g[0], g[1], t[0], t[1]) for g, t in WINDOWS], int)
    assert [x[0] for x in got] == [R.n0_of(g, t) for g, t in WINDOWS]
    assert os_main([("n0", 0, 0, 16, 16)], int) == [[1088]]
    for (g, t) in WINDOWS:
        for nb in (g[0] + t[0] + 1, g[0] + t[0] + 2, 2 * (g[0] + t[0]) + 1, 70):
            assert os_main([("counts", g[0], g[1], t[0], t[1], nb)], int)[0] == counts_ref(g[0], g[1], t[0], t[1], nb).tolist(), (g, t, nb)
    for rank, n0 in ((1, 248), (186, 248), (248, 248), (816, 1088), (1, 1), (33, 66)):
        got = os_main([("ranks", rank, n0)], int)[0]
        assert got == [-(-rank * N // n0) for N in range(1, n0 + 1)]
        assert min(got) >= 1 and all(k <= N for k, N in zip(got, range(1, n0 + 1))) and got[-1] == rank


def test_header_alone_halves(os_main):
    """the training count's left and right halves (the mean-level kernel's GO / SO means divide by them) against a count one offset at
    a time, and, for every window of up to 16 cells per field and every pair of edge distances, the integers of the two texts the
    shared count replaced"""
    for (g, t) in WINDOWS:
        Or, Od = g[0] + t[0], g[1] + t[1]
        for nb in (Or + 1, Or + 2, 2 * Or + 1, 70):
            got = np.array(os_main([("halves", g[0], g[1], t[0], t[1], nb)], int)[0]).reshape(nb, 2)
            r = np.arange(nb)
            want = np.zeros((nb, 2), np.int64)
            for dk in range(-Od, Od + 1):
                for dr in range(-Or, Or + 1):
                    if dr != 0 and not (abs(dk) <= g[1] and abs(dr) <= g[0]):
                        want[:, 0 if dr < 0 else 1] += (r + dr >= 0) & (r + dr < nb)
            assert np.array_equal(got, want), (g, t, nb)
            assert (got.sum(axis=1) + 2 * t[1]).tolist() == counts_ref(g[0], g[1], t[0], t[1], nb).tolist()
    checked, bad = os_main([("halves", 16)], int)[0]
    assert checked == 17 * 17 * sum((gr + tr + 2) ** 2 for gr in range(17) for tr in range(17)) and bad == 0


def test_header_alone_alpha_and_table(os_main):
    for n, k, pfa in ((248, 186, 1e-2), (1, 1, 1e-3), (1088, 816, 1e-6), (17, 13, 0.5), (1088, 1088, 1e-9), (1088, 1, 0.999)):
        a = os_main([("alpha", n, k, pfa)])[0][0]
        assert abs(R.law(n, k, a) - pfa) <= 1e-11 * pfa, (n, k, pfa)
    for (g, t), rank, nb in ((((2, 2), (8, 4)), 186, 300), (((0, 0), (16, 1)), 72, 17), (((0, 0), (0, 16)), 24, 70)):
        n0 = R.n0_of(g, t)
        tab = os_main([("table", g[0], g[1], t[0], t[1], rank, 1e-3, nb)])[0]
        assert len(tab) == n0 + 1
        occurring = set(counts_ref(g[0], g[1], t[0], t[1], nb).tolist())
        for N, a in enumerate(tab):
            if N in occurring:
                k = -(-rank * N // n0)
                assert abs(R.law(N, k, a) - 1e-3) <= 1e-11 * 1e-3, (g, t, N)
            else:
                assert a == 0.0


def test_header_alone_selection(os_main):
    rng = np.random.default_rng(5)
    cases = []
    for n in (1, 2, 3, 7, 64, 248, 1088):
        x = rng.exponential(size=n)
        if n >= 7:
            x[:3] = x[3]                                      # ties
            x[-1] = math.inf; x[-2] = 0.0
        for k in sorted({1, 2, (n + 1) // 2, (3 * n) // 4, n - 1, n} & set(range(1, n + 1))):
            cases.append((k, x))
    got = os_main([("select", k) + tuple(float(v) for v in x) for k, x in cases])
    for (k, x), g in zip(cases, got):
        assert g[0] == np.sort(x)[k - 1], (k, len(x))


def main_map(n_rx, nd, nb):
    """the map tests/cfar_os/cfar_os_main.cpp fills"""
    rx = np.arange(n_rx)[:, None, None]; k = np.arange(nd)[None, :, None]; r = np.arange(nb)[None, None, :]
    re = ((rx * 131 + k * 17 + r * 7) % 23) - 11.0 + 0.25 * k
    im = ((rx * 5 + k * 3 + r * 11) % 19) - 9.0 - 0.5 * (r % 5)
    return re + 1j * im


def test_header_alone_evaluator(os_main):
    """the evaluator on heap arrays of exactly their sizes (the map, N0 keys, N0 + 1 alphas, `capacity` records): the integer
    fields, power and noise of every record against the restatement, on a map full of ties"""
    cases = []
    for (g, t), (n_rx, nd, nb) in zip(WINDOWS, ((2, 20, 70), (1, 33, 40), (1, 3, 64), (2, 5, 30), (2, 40, 5), (2, 12, 66), (1, 15, 17))):
        n0 = R.n0_of(g, t)
        for rank in (1, (3 * n0) // 4, n0):
            for flags in (0, 1):
                for pfa, alpha in ((0.0, 1.5), (0.2, 0.0)):
                    cases.append((n_rx, nd, nb, g[0], g[1], t[0], t[1], rank, flags, pfa, alpha, n_rx * nd * nb))
    cases.append((2, 20, 70, 2, 2, 8, 4, 100, 0, 0.0, 1.0, 3))          # capacity below the total
    got = os_main([("eval",) + c for c in cases])
    for c, g in zip(cases, got):
        n_rx, nd, nb, gr, gd, tr, td, rank, flags, pfa, alpha, cap = c
        z = main_map(n_rx, nd, nb)
        P = z.real * z.real + z.imag * z.imag
        noise, thr, n, det = R.os_ref(P, gr, gd, tr, td, rank, pfa or None, alpha or None, bool(flags))
        if pfa:                                               # the restatement's own alpha may differ in the last bits: cells on the threshold are not compared
            sure = np.abs(P - thr) > 1e-9 * np.abs(thr)
        else:
            sure = np.ones(P.shape, bool)
        total = int(g[0]); rec = np.array(g[1:]).reshape(-1, 6)
        assert len(rec) == min(total, cap)
        if not sure.all():
            continue
        want = np.argwhere(det)
        assert total == len(want), c
        for row, (rx, k, r) in zip(rec, want):
            assert (int(row[0]), int(row[1]), int(row[2]), int(row[3])) == (rx, k, r, int(n[rx, k, r])), c
            assert row[4] == P[rx, k, r] and row[5] == noise[rx, k, r], c
    assert int(got[-1][0]) > 3
