"""Autofocus on the host (no GPU): rts_align_eval, rts_pga_eval and rts_correct_eval against the numpy restatement of
tests/focus_ref.py, the edge and exactness cases, every refusal, the end-to-end scenes, and rts_amd/csrc/rts_focus.h alone under
AddressSanitizer + UndefinedBehaviorSanitizer (tests/focus/focus_main.cpp).

Bounds.  Alignment: IEEE basic operations in one order on both sides -- the integer shifts are compared with ==, the refined ones to
1e-12 bins.  Correction: rtol 1e-10, atol 1e-12 max|ref|, the image's bound, for the image's reason (the same interpolator against
the same restatement; one more rotation of a few ulp).  PGA: the evaluator runs the library's radix-2 tree, the restatement
numpy.fft; EVAL_VS_NUMPY is the largest |phase difference| in cycles measured over PGA_CASES (printed by
test_pga_eval_against_restatement and recorded in profiles/focus_bench.txt); the assertion bound is 100 times that and must stay
below 1e-9 cycles.  Every PGA comparison uses cubes in which each gate column's largest |X[k]|^2 exceeds its second largest by a
factor >= 1 + 1e-6 in every iteration (checked from the restatement): a flipped peak is no rounding error.

End to end (focus_ref.scene: shapes (64, 96) and (128, 256), seeds 0-4; autofocus(max_lag=8, align n_iters=4, taps=8, pga n_iters=6,
window_min=8)), measured on the restatement over all ten scenes before the bounds were fixed:
    largest shift error after removing its mean     0.202 .. 0.284 bin     asserted < 0.5 bin
    residual phase rms after constant and line      0.229 .. 0.398 rad     asserted < 0.6 rad
    contrast after / aligned-only cube's            2.149 .. 4.392         asserted >= 1.5
    contrast after / raw cube's                     3.892 .. 8.619         asserted >= 3
No scene comes within 20 % of a bound, so the bounds stand as the issue set them."""
import ctypes as C
import math
import os
import shutil
import subprocess

import numpy as np
import pytest

import focus_ref as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

EVAL_VS_NUMPY = 3.1e-15        # cycles: the largest |evaluator - numpy| phase over PGA_CASES as measured, 3.08e-15 (see the module's text)
PGA_BOUND = 100 * EVAL_VS_NUMPY
assert PGA_BOUND < 1e-9

# (N, gate length, n_iters, n_rx); the last: the one-column plan
PGA_CASES = [(N, G, it, n_rx) for N in (4, 8, 64, 512) for G in (1, 7, 8, 9, 17) for it, n_rx in ((1, 3), (4, 1))] + [(4096, 3, 4, 1)]


# ----------------------------------------------------------------------------- generators
def align_cube(seed, n_rx, rows, nb=140):
    """a random complex cube plus one walking scatterer (9 bins over the rows), so that the shifts are not all 0"""
    rng = np.random.default_rng(seed)
    cube = rng.standard_normal((n_rx, rows, nb)) + 1j * rng.standard_normal((n_rx, rows, nb))
    for p in range(rows):
        cube[:, p, 60 + (p * 9) // max(rows, 1)] += 30.0
    return cube


def pga_cube(seed, n_rx, N, G, first=1, first_bin=2):
    """rows first .. first + N - 1 and bins first_bin .. first_bin + G - 1 hold, per column, a dominant tone between two Doppler rows
    on a noise floor, under a common smooth-plus-random phase error of about a cycle: (cube [n_rx][N + 2][G + 4], the error in cycles)"""
    rng = np.random.default_rng(seed)
    cube = rng.standard_normal((n_rx, N + 2, G + 4)) + 1j * rng.standard_normal((n_rx, N + 2, G + 4))
    p = np.arange(N)
    t = (p - N / 2) / N
    err = 1.5 * t * t + np.cumsum(rng.normal(0.0, 0.02, N))
    fd = (rng.integers(0, N, (n_rx, G)) + 0.37) / N
    tone = np.exp(2j * np.pi * (fd[:, None, :] * p[None, :, None] + err[None, :, None]))
    cube[:, first:first + N, first_bin:first_bin + G] += 4.0 * math.sqrt(N) * tone
    return cube, err


def pga_distance(rts, cases=PGA_CASES):
    """the largest |evaluator - restatement| of the phase (cycles) and of the rms over the cases, and the least peak margin"""
    worst, worst_rms, margin = 0.0, 0.0, math.inf
    for i, (N, G, it, n_rx) in enumerate(cases):
        cube, _ = pga_cube(300 + i, n_rx, N, G)
        got, got_rms = rts.pga_eval(cube, first=1, count=N, gate=(2, G), n_iters=it)
        ref, ref_rms, m = F.pga_ref(cube, first=1, count=N, gate=(2, G), n_iters=it)
        assert m >= 1 + 1e-6, (N, G, it, n_rx, m)
        worst = max(worst, float(np.abs(got - ref).max())); worst_rms = max(worst_rms, float(np.abs(got_rms - ref_rms).max())); margin = min(margin, m)
    return worst, worst_rms, margin


# ----------------------------------------------------------------------------- against the restatement
@pytest.mark.parametrize("P", [1, 2, 63, 64, 65, 130])
def test_align_eval_against_restatement(rts, P):
    cube = align_cube(10 + P, 2, P + 4)
    for (fb, G), L, iters in (((0, 0), 9, 3), ((5, 64), 1, 1), ((140 - 65, 65), 64, 1), ((0, 1), 9, 3), ((10, 130), 0, 3), ((0, 63), 9, 1)):
        for integer in (True, False):
            got = rts.align_eval(cube, first=3, count=P, gate=(fb, G), max_lag=L, n_iters=iters, integer=integer)
            ref = F.align_ref(cube, first=3, count=P, gate=(fb, G), max_lag=L, n_iters=iters, integer=integer)
            assert got.shape == (2, P)
            if integer:
                assert np.array_equal(got, ref), (P, fb, G, L, iters)
                assert np.array_equal(got, np.round(got))
            else:
                assert np.abs(got - ref).max() <= 1e-12, (P, fb, G, L, iters, np.abs(got - ref).max())
            assert np.abs(got).max() <= L
    if P >= 63:
        full = rts.align_eval(cube, first=3, count=P, max_lag=9, n_iters=3)
        assert full.max() - full.min() > 5                     # the walking scatterer is followed


@pytest.mark.parametrize("taps", [1, 2, 8])
def test_correct_eval_against_restatement(rts, taps):
    rng = np.random.default_rng(77 + taps)
    cube = rng.standard_normal((2, 12, 48)) + 1j * rng.standard_normal((2, 12, 48))
    sh = rng.uniform(-3, 3, (2, 9))
    sh[0, :6] = (0.0, 2.0, -3.0, 0.5, -0.5, 60.0); sh[1, :3] = (-60.0, 47.5, -47.5)
    ph = rng.uniform(-3, 3, (2, 9)); ph[0, 0] = 0.0; ph[0, 1] = 1.0; ph[1, 0] = -0.25
    for s, p in ((sh, ph), (sh, None), (None, ph)):
        got = rts.correct_eval(cube, s, p, first=2, count=9, taps=taps)
        ref = F.correct_ref(cube, s, p, first=2, count=9, taps=taps)
        np.testing.assert_allclose(got, ref, rtol=1e-10, atol=1e-12 * np.abs(ref).max())
        assert np.array_equal(got[:, :2], cube[:, :2]) and np.array_equal(got[:, 11:], cube[:, 11:])       # rows outside the range
    got = rts.correct_eval(cube, sh, None, first=2, count=9, taps=taps)
    assert np.array_equal(got[0, 2], cube[0, 2])                                                           # S == 0: bit for bit
    assert np.array_equal(got[0, 3, :46], cube[0, 3, 2:]) and np.all(got[0, 3, 46:] == 0)                   # an integer shift: a copy, 0 beyond the row
    assert np.all(got[0, 7] == 0) and np.all(got[1, 2] == 0)                                               # reads off either end
    got = rts.correct_eval(cube, None, ph, first=2, count=9, taps=taps)
    assert np.array_equal(got[0, 2], cube[0, 2]) and np.array_equal(got[0, 3], cube[0, 3])                 # phi == 0 and phi == 1: bit for bit
    np.testing.assert_allclose(got[1, 2], cube[1, 2] * 1j, rtol=0, atol=1e-15 * np.abs(cube).max())


def test_pga_eval_against_restatement(rts):
    worst, worst_rms, margin = pga_distance(rts)
    print("evaluator vs numpy: largest |phase difference| %.3g cycles (rms record %.3g) over %d cases; least peak margin %.4g; recorded %.3g, bound %.3g"
          % (worst, worst_rms, len(PGA_CASES), margin, EVAL_VS_NUMPY, PGA_BOUND))
    assert worst <= PGA_BOUND and worst_rms <= PGA_BOUND


# ----------------------------------------------------------------------------- edge and exactness cases
def test_edge_cases(rts):
    cube = align_cube(3, 2, 20)
    # P == 1: the row is its own reference
    assert np.array_equal(rts.align_eval(cube, first=4, count=1, max_lag=9, integer=True), np.zeros((2, 1)))
    assert np.abs(rts.align_eval(cube, first=4, count=1, max_lag=9)).max() < 1e-9       # (C(-1) and C(+1) hold the same products in other blocks)
    # L == 0
    assert np.array_equal(rts.align_eval(cube, max_lag=0, n_iters=2), np.zeros((2, 20)))
    # a gate of one bin, gates touching either row end with lags that run off the row
    for gate in ((60, 1), (0, 3), (137, 3), (139, 1), (0, 0)):
        for integer in (True, False):
            got = rts.align_eval(cube, gate=gate, max_lag=64, n_iters=2, integer=integer)
            ref = F.align_ref(cube, gate=gate, max_lag=64, n_iters=2, integer=integer)
            assert np.array_equal(got, ref) if integer else np.abs(got - ref).max() <= 1e-12, gate
    # an all-zero row gives 0; a NaN never wins
    z = cube.copy(); z[:, 7] = 0
    assert np.all(rts.align_eval(z, max_lag=9)[:, 7] == 0)
    assert np.all(rts.align_eval(np.zeros((1, 5, 16), np.complex128), max_lag=4) == 0)
    # N == 4, window0 >= N (nothing is masked), an all-zero column
    c4, _ = pga_cube(8, 2, 4, 3)
    c4[:, :, 3] = 0
    for w0 in (0, 4, 1000):
        got, got_rms = rts.pga_eval(c4, first=1, count=4, gate=(2, 3), n_iters=2, window0=w0, window_min=1)
        ref, ref_rms, m = F.pga_ref(c4, first=1, count=4, gate=(2, 3), n_iters=2, window0=w0, window_min=1)
        assert m >= 1 + 1e-6
        assert np.abs(got - ref).max() <= PGA_BOUND and np.abs(got_rms - ref_rms).max() <= PGA_BOUND
    phase, rms = rts.pga_eval(np.zeros((1, 8, 4), np.complex128))
    assert np.all(phase == 0) and np.all(rms == 0)
    # a pure tone has no phase error: nothing to correct
    tone = np.exp(2j * np.pi * 0.125 * np.arange(16))[None, :, None] * np.ones((1, 16, 2))
    phase, rms = rts.pga_eval(tone, n_iters=2)
    assert np.abs(phase).max() < 1e-12
    # S == 0 and phi == 0 pass rows through bit for bit, whatever the taps
    for taps in (1, 2, 8, 64):
        out = rts.correct_eval(cube, np.zeros((2, 20)), np.zeros((2, 20)), taps=taps)
        assert np.array_equal(out, cube)


# ----------------------------------------------------------------------------- refusals
def raw_cube(L, n_rx=2, rows=12, nb=16):
    q = L.RtsCubeParams(n_rx, rows, nb, 0, 0.0, 1.0)
    return q, np.ones((n_rx, rows, nb, 2))


def setter(**kw):
    def f(p, keep):
        for k, v in kw.items():
            setattr(p, k, v)
    return f


def reserved(i):
    def f(p, keep):
        if i < 0:
            p.reserved0 = 1
        else:
            p.reserved[i] = 1
    return f


def poison(name, index, value):
    def f(p, keep):
        keep[name][index] = value
    return f


def test_malformed_align_is_rejected(rts):
    from rts_amd import _lib as L
    lib = L.lib()
    q, cube = raw_cube(L)

    def params():
        p = L.RtsAlignParams()
        p.first_pulse, p.n_pulses, p.first_bin, p.n_gate, p.max_lag, p.n_iters, p.flags = 1, 8, 2, 10, 3, 2, 0
        return p
    out = np.full((2, 8), 7.25)
    assert lib.rts_align_eval(C.byref(q), cube.ctypes.data, C.byref(params()), out.ctypes.data) == L.RTS_OK and not np.any(out == 7.25)
    bad = [("reserved0", reserved(-1), b"reserved"), ("reserved 0", reserved(0), b"reserved"), ("reserved 1", reserved(1), b"reserved"),
           ("unknown flag", setter(flags=2), b"flags"), ("no pulses", setter(n_pulses=0), b"n_pulses"), ("rows beyond", setter(first_pulse=5), b"n_pulses"),
           ("first beyond", setter(first_pulse=12), b"first_pulse"), ("wrapping rows", setter(first_pulse=0xffffffff), b"first_pulse"),
           ("first_bin beyond", setter(first_bin=16), b"first_bin"), ("gate beyond", setter(first_bin=7), b"n_gate"), ("wrapping gate", setter(n_gate=0xffffffff), b"n_gate"),
           ("max_lag", setter(max_lag=65), b"max_lag"), ("n_iters 0", setter(n_iters=0), b"n_iters"), ("n_iters 9", setter(n_iters=9), b"n_iters")]
    for name, mutate, word in bad:
        p = params(); mutate(p, None); out[:] = 7.25
        assert lib.rts_align_eval(C.byref(q), cube.ctypes.data, C.byref(p), out.ctypes.data) == L.RTS_ERR_INVALID, name
        assert word in lib.rts_last_error(), (name, lib.rts_last_error())
        assert np.all(out == 7.25), name
    p = params()
    big = L.RtsCubeParams(65536, 12, 16, 0, 0.0, 1.0)
    assert lib.rts_align_eval(C.byref(big), cube.ctypes.data, C.byref(p), out.ctypes.data) == L.RTS_ERR_INVALID and b"n_rx" in lib.rts_last_error()
    assert lib.rts_align_eval(None, cube.ctypes.data, C.byref(p), out.ctypes.data) == L.RTS_ERR_INVALID
    assert lib.rts_align_eval(C.byref(q), None, C.byref(p), out.ctypes.data) == L.RTS_ERR_INVALID
    assert lib.rts_align_eval(C.byref(q), cube.ctypes.data, None, out.ctypes.data) == L.RTS_ERR_INVALID
    assert lib.rts_align_eval(C.byref(q), cube.ctypes.data, C.byref(p), None) == L.RTS_ERR_INVALID
    assert np.all(out == 7.25)
    p.max_lag, p.n_iters, p.n_gate = 64, 8, 0                  # the limits themselves, and the gate to the row's end
    assert lib.rts_align_eval(C.byref(q), cube.ctypes.data, C.byref(p), out.ctypes.data) == L.RTS_OK


def test_malformed_pga_is_rejected(rts):
    from rts_amd import _lib as L
    lib = L.lib()
    q, cube = raw_cube(L)

    def params():
        p = L.RtsPgaParams()
        p.first_pulse, p.n_pulses, p.first_bin, p.n_gate, p.n_iters, p.window0, p.window_min = 1, 8, 2, 10, 2, 0, 0
        return p
    phase = np.full((2, 8), 7.25); rms = np.full((2, 2), 7.25)
    assert lib.rts_pga_eval(C.byref(q), cube.ctypes.data, C.byref(params()), phase.ctypes.data, rms.ctypes.data) == L.RTS_OK
    assert not np.any(phase == 7.25) and not np.any(rms == 7.25)
    bad = [("reserved0", reserved(-1), b"reserved"), ("reserved 0", reserved(0), b"reserved"), ("reserved 1", reserved(1), b"reserved"),
           ("N 0", setter(n_pulses=0), b"n_pulses"), ("N 2", setter(n_pulses=2), b"n_pulses"), ("N 6", setter(n_pulses=6), b"n_pulses"), ("N 8192", setter(n_pulses=8192), b"n_pulses"),
           ("rows beyond", setter(first_pulse=5), b"n_pulses"), ("first beyond", setter(first_pulse=12), b"first_pulse"),
           ("first_bin beyond", setter(first_bin=16), b"first_bin"), ("gate beyond", setter(first_bin=7), b"n_gate"), ("wrapping gate", setter(n_gate=0xffffffff), b"n_gate"),
           ("n_iters 0", setter(n_iters=0), b"n_iters"), ("n_iters 17", setter(n_iters=17), b"n_iters")]
    for name, mutate, word in bad:
        p = params(); mutate(p, None); phase[:] = 7.25; rms[:] = 7.25
        assert lib.rts_pga_eval(C.byref(q), cube.ctypes.data, C.byref(p), phase.ctypes.data, rms.ctypes.data) == L.RTS_ERR_INVALID, name
        assert word in lib.rts_last_error(), (name, lib.rts_last_error())
        assert np.all(phase == 7.25) and np.all(rms == 7.25), name
    p = params()
    big = L.RtsCubeParams(65536, 12, 16, 0, 0.0, 1.0)
    assert lib.rts_pga_eval(C.byref(big), cube.ctypes.data, C.byref(p), phase.ctypes.data, rms.ctypes.data) == L.RTS_ERR_INVALID and b"n_rx" in lib.rts_last_error()
    assert lib.rts_pga_eval(C.byref(q), None, C.byref(p), phase.ctypes.data, rms.ctypes.data) == L.RTS_ERR_INVALID
    assert lib.rts_pga_eval(C.byref(q), cube.ctypes.data, None, phase.ctypes.data, rms.ctypes.data) == L.RTS_ERR_INVALID
    assert lib.rts_pga_eval(C.byref(q), cube.ctypes.data, C.byref(p), None, rms.ctypes.data) == L.RTS_ERR_INVALID
    assert lib.rts_pga_eval(C.byref(q), cube.ctypes.data, C.byref(p), phase.ctypes.data, None) == L.RTS_ERR_INVALID
    assert np.all(phase == 7.25) and np.all(rms == 7.25)


def test_malformed_correct_is_rejected(rts):
    from rts_amd import _lib as L
    lib = L.lib()
    q, cube = raw_cube(L)

    def params():
        keep = dict(shifts=np.linspace(-1, 1, 16), phase=np.linspace(-2, 2, 16))
        p = L.RtsCorrectParams()
        p.first_pulse, p.n_pulses, p.taps, p.flags = 1, 8, 8, 0
        p.shifts = keep["shifts"].ctypes.data; p.phase = keep["phase"].ctypes.data
        return p, keep
    work = cube.copy()
    p, keep = params()
    assert lib.rts_correct_eval(C.byref(q), work.ctypes.data, C.byref(p)) == L.RTS_OK and not np.array_equal(work, cube)
    bad = [("reserved 0", reserved(0), b"reserved"), ("reserved 1", reserved(1), b"reserved"), ("unknown flag", setter(flags=4), b"flags"),
           ("use_align on the host", setter(flags=1, shifts=None), b"flags"), ("use_pga on the host", setter(flags=2, phase=None), b"flags"),
           ("no pulses", setter(n_pulses=0), b"n_pulses"), ("rows beyond", setter(first_pulse=5), b"n_pulses"), ("first beyond", setter(first_pulse=12), b"first_pulse"),
           ("taps 0", setter(taps=0), b"taps"), ("taps 3", setter(taps=3), b"taps"), ("taps 66", setter(taps=66), b"taps"),
           ("neither", setter(shifts=None, phase=None), b"neither"),
           ("shift nan", poison("shifts", 3, math.nan), b"shifts"), ("shift inf", poison("shifts", 15, math.inf), b"shifts"),
           ("phase nan", poison("phase", 0, math.nan), b"phase"), ("phase inf", poison("phase", 9, -math.inf), b"phase")]
    for name, mutate, word in bad:
        p, keep = params(); mutate(p, keep); work = cube.copy()
        assert lib.rts_correct_eval(C.byref(q), work.ctypes.data, C.byref(p)) == L.RTS_ERR_INVALID, name
        assert word in lib.rts_last_error(), (name, lib.rts_last_error())
        assert np.array_equal(work, cube), name
    p, keep = params()
    big = L.RtsCubeParams(65536, 12, 16, 0, 0.0, 1.0)
    assert lib.rts_correct_eval(C.byref(big), work.ctypes.data, C.byref(p)) == L.RTS_ERR_INVALID and b"n_rx" in lib.rts_last_error()
    assert lib.rts_correct_eval(C.byref(q), None, C.byref(p)) == L.RTS_ERR_INVALID
    assert lib.rts_correct_eval(C.byref(q), work.ctypes.data, None) == L.RTS_ERR_INVALID
    assert lib.rts_correct_eval(None, work.ctypes.data, C.byref(p)) == L.RTS_ERR_INVALID
    with pytest.raises(ValueError):
        rts.correct_eval(np.zeros((1, 8, 4)), shifts=np.zeros(7))


# ----------------------------------------------------------------------------- end to end, on the evaluators
def autofocus_eval(rts, raw):
    S = rts.align_eval(raw, max_lag=8, n_iters=4)
    aligned = rts.correct_eval(raw, shifts=S, taps=8)
    phase, rms = rts.pga_eval(aligned, n_iters=6, window_min=8)
    return S, phase, rms, aligned, rts.correct_eval(aligned, phase=phase, taps=8)


@pytest.mark.parametrize("shape,walk", F.SCENES)
def test_end_to_end(rts, shape, walk):
    for seed in range(5):
        sc = F.scene(shape, walk, seed)
        S, phase, rms, aligned, focused = autofocus_eval(rts, sc["raw"])
        es, pr, ca, cr = F.autofocus_metrics(sc, S, phase, focused, aligned)
        print("%s seed %d: shift error %.3f bin, residual phase %.3f rad rms, contrast x%.2f over aligned, x%.2f over raw; rms record %s"
              % (shape, seed, es, pr, ca, cr, np.array2string(rms[0], precision=4)))
        assert es < 0.5 and pr < 0.6 and ca >= 1.5 and cr >= 3.0, (shape, seed)


# ----------------------------------------------------------------------------- rts_focus.h alone, under the sanitizers
@pytest.fixture(scope="module")
def focus_main(tmp_path_factory):
    gxx = shutil.which("g++")
    if not gxx:
        pytest.skip("no g++")
    rt = subprocess.run([gxx, "-print-file-name=libasan.so"], capture_output=True, text=True).stdout.strip()
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"] if os.path.isabs(rt) and os.path.exists(rt) else []
    exe = str(tmp_path_factory.mktemp("focus") / "focus_main")
    subprocess.check_call([gxx, "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-ffp-contract=off"] + san + ["-I", os.path.join(ROOT, "rts_amd", "csrc"),
                           os.path.join(ROOT, "tests", "focus", "focus_main.cpp"), "-o", exe])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:verify_asan_link_order=0", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")

    def ask(cases, kind=float):
        text = "".join(" ".join(str(x) for x in c) + "\n" for c in cases)
        r = subprocess.run([exe], input=text, capture_output=True, text=True, env=env, timeout=120)
        assert r.returncode == 0, r.stderr[-3000:]
        out = [[kind(x) for x in line.split()] for line in r.stdout.splitlines()]
        assert len(out) == len(cases)
        return out
    return ask


def main_cube(n_rx, rows, nb, zero_row=-1):
    """the cube tests/focus/focus_main.cpp fills"""
    r = np.arange(n_rx)[:, None, None]; p = np.arange(rows)[None, :, None]; b = np.arange(nb)[None, None, :]
    re = ((r * 131 + p * 17 + b * 7) % 23) - 11.0 + 0.25 * p + 200.0 * (b == (nb // 2 + p // 8) % nb)
    im = ((r * 5 + p * 3 + b * 11) % 19) - 9.0 - 0.5 * b + 0.0 * p
    c = re + 1j * im
    if zero_row >= 0:
        c[:, zero_row] = 0
    return c


def test_header_alone_on_the_edge_shapes(rts, focus_main):
    """the three evaluators over the edge shapes, every sample outside what their definitions read poisoned: the driver's numbers are
    the library's (the alignment's to the bit)"""
    align = [(2, 70, 40, 3, 65, 0, 40, 9, 3, 0, -1), (2, 70, 40, 0, 1, 5, 1, 9, 2, 0, -1), (1, 70, 40, 5, 64, 0, 3, 64, 1, 1, -1), (2, 70, 40, 0, 70, 37, 3, 64, 2, 0, 9),
             (1, 70, 40, 2, 66, 4, 33, 0, 2, 0, -1), (1, 130, 40, 0, 130, 0, 40, 1, 1, 1, 129)]
    for c, g in zip(align, focus_main([("align",) + c for c in align])):
        n_rx, rows, nb, first, P, fb, G, L, iters, flags, zero = c
        ref = rts.align_eval(main_cube(n_rx, rows, nb, zero), first=first, count=P, gate=(fb, G), max_lag=L, n_iters=iters, integer=bool(flags))
        assert np.array_equal(np.array(g), ref.ravel()), c
    pga = [(2, 20, 12, 3, 16, 0, 12, 3, 0, 0), (1, 20, 12, 0, 4, 11, 1, 2, 4, 1), (1, 70, 12, 6, 64, 2, 9, 4, 1000, 2), (2, 20, 12, 12, 8, 0, 1, 1, 0, 0)]
    for c, g in zip(pga, focus_main([("pga",) + c for c in pga])):
        n_rx, rows, nb, first, N, fb, G, iters, w0, wmin = c
        phase, rms = rts.pga_eval(main_cube(n_rx, rows, nb), first=first, count=N, gate=(fb, G), n_iters=iters, window0=w0, window_min=wmin)
        np.testing.assert_allclose(np.array(g), np.concatenate([phase.ravel(), rms.ravel()]), rtol=0, atol=PGA_BOUND, err_msg=str(c))
    correct = [(2, 12, 40, 2, 9, 8, 3), (2, 12, 40, 0, 12, 1, 3), (1, 12, 40, 11, 1, 2, 1), (2, 12, 40, 3, 5, 64, 2)]
    for c, g in zip(correct, focus_main([("correct",) + c for c in correct])):
        n_rx, rows, nb, first, P, taps, mode = c
        i = np.arange(n_rx * P)
        sh = (((i * 3) % 11) - 5.0) * 0.5 if mode & 1 else None
        ph = ((i % 9) - 4.0) * 0.375 if mode & 2 else None
        ref = rts.correct_eval(main_cube(n_rx, rows, nb), sh, ph, first=first, count=P, taps=taps)
        got = np.array(g)
        got = (got[0::2] + 1j * got[1::2]).reshape(ref.shape)
        np.testing.assert_allclose(got, ref, rtol=1e-12, atol=1e-12 * np.abs(ref).max(), err_msg=str(c))


def test_launch_plans(focus_main):
    consts = focus_main([("consts",)], int)[0]
    assert consts == [64, 8, 64, 64, 2048, 4096, 16, 8, 160 * 1024, 65535]
    cases = [(n_rx, N, G) for n_rx in (1, 3) for N in (4 << e for e in range(11)) for G in (1, 7, 8, 9, 17, 4096)]
    for (n_rx, N, G), g in zip(cases, focus_main([("pgaplan",) + c for c in cases], int)):
        logN, BT, passes, tiles, lds, partial, out, w0, wmin, supported = g
        assert 1 << logN == N and BT in (1, 2, 4, 8) and passes * BT == 8 and tiles == -(-G // 8)
        assert lds == 2 * N * BT * 16 + N * 8 and lds <= 160 * 1024                     # two column sets and the twiddle table fit
        assert BT == 8 or 2 * N * (2 * BT) * 16 + N * 8 > 160 * 1024                    # ... and twice the columns would not
        assert 12 * min(256, N * BT) <= 16 * N * BT                                    # the peak search's candidates fit the idle column set
        assert partial == 2 * n_rx * tiles * N and out == n_rx * N + 3 * n_rx and (w0, wmin) == (N // 2, 8) and supported == 1
    assert [focus_main([("pgaplan", 1, n, 8)], int)[0][1] for n in (512, 1024, 2048, 4096)] == [8, 4, 2, 1]
    assert focus_main([("pgaplan", 65536, 8, 8)], int)[0][9] == 0
    for (n_rx, P, nb, G, L), g in zip([(2, 65, 140, 130, 9), (1, 1, 16, 1, 0), (1, 300, 5000, 5000, 64)],
                                      focus_main([("alignplan", 2, 65, 140, 130, 9), ("alignplan", 1, 1, 16, 1, 0), ("alignplan", 1, 300, 5000, 5000, 64)], int)):
        n_lags, n_blocks, bpp, env, ref, out, supported = g
        assert n_lags == 2 * L + 1 and n_blocks == -(-G // 64) and bpp == 2048 // n_lags and bpp * n_lags <= 2048 and bpp >= 1
        assert (env, ref, out, supported) == (n_rx * P * nb, n_rx * G, n_rx * P, 1)
