"""FMCW mode on the host (no GPU): rts_beat_eval against an independent numpy restatement of the definition in include/rts_amd.h
(RtsBeatParams: psi_k(n) written down directly, one np.exp per sample, no strips), known answers, rts_range_eval against
rts_stft_eval on the axis-swapped cube bit for bit, every refusal the header lists for the two evaluators, and rts_amd/csrc/rts_beat.h
alone under AddressSanitizer + UndefinedBehaviorSanitizer (tests/beat/beat_main.cpp) with the plans' documented values at their edges.

Tolerance of evaluator against restatement: the project's bound for a kernel against its evaluator, rtol 1e-10 and
atol 1e-12 max|ref| (tests/test_gpu_render.py).  The two sides differ in how psi is rounded (a few ulp of some hundred turns: below
1e-13 of a turn), in the strips' rotation (16 steps of about an ulp each) and in libm against numpy: all orders below the bound."""
import ctypes as C
import math
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T0, DT, NB = 1.1e-6, 5.0e-9, 200                 # the row spans 1.1 us .. 2.095 us; 200 is not a multiple of the strip (16)
SLOPE = 2.0e13                                   # |S tau| dt = 0.2 at tau = 2 us: below 1/2
T_CUT = 1.9e-6                                   # the oscillator stops inside the row, at sample 160


# ----------------------------------------------------------------------------- numpy restatement (from the header's text)
def beat_ref(cube, pulse, contribs, slope, duration, t0, dt, doppler):
    """cube[rx, pulse, n] += a e^{j 2 pi psi(n)}, psi(n) = (f - S tau) t_n + S tau^2 / 2 - f tau, where tau <= t_n and 0 <= t_n < T"""
    n_rx, _, nb = cube.shape
    t = t0 + np.arange(nb, dtype=np.float64) * dt
    for rx, a, tau, f in contribs:
        if rx < 0 or rx >= n_rx or not math.isfinite(tau):
            continue
        f = f if doppler else 0.0
        psi = (f - slope * tau) * t + slope * tau * tau / 2 - f * tau
        gate = (tau <= t) & (t >= 0) & (t < duration)
        cube[rx, pulse, gate] += a * np.exp(2j * np.pi * psi[gate])
    return cube


def random_contributions(seed, n=300, n_rx=3):
    """receivers -1 .. n_rx (both ends out of range), delays from before t0 to beyond the row's end, a fifth of them on the grid,
    some not finite"""
    rng = np.random.default_rng(seed)
    out = []
    for k in range(n):
        rx = int(rng.integers(-1, n_rx + 1))
        a = complex(rng.standard_normal(), rng.standard_normal())
        tau = float(rng.uniform(0.8e-6, 2.3e-6))
        if k % 5 == 0:
            tau = T0 + int(rng.integers(0, NB)) * DT                 # on the grid: the gate's tau <= t_n holds with equality
        if k % 29 == 3:
            tau = (math.nan, math.inf, -math.inf)[k % 3]
        out.append((rx, a, tau, float(rng.uniform(-2.0e6, 2.0e6))))
    return out


# ----------------------------------------------------------------------------- H1
@pytest.mark.parametrize("slope", [SLOPE, -SLOPE])
@pytest.mark.parametrize("doppler", [False, True])
def test_eval_against_restatement(rts, slope, doppler):
    contribs = random_contributions(11)
    assert sum(1 for c in contribs if c[2] < T0) > 20 and sum(1 for c in contribs if math.isfinite(c[2]) and c[2] > T0 + NB * DT) > 20
    assert sum(1 for c in contribs if not math.isfinite(c[2])) >= 6 and {c[0] for c in contribs} == {-1, 0, 1, 2, 3}
    ref = beat_ref(np.zeros((3, 2, NB), np.complex128), 1, contribs, slope, T_CUT, T0, DT, doppler)
    got = rts.beat_eval(np.zeros((3, 2, NB), np.complex128), 1, contribs, slope, T_CUT, T0, DT, doppler=doppler)
    assert np.count_nonzero(ref[:, 1]) > ref[:, 1].size // 2
    assert np.count_nonzero(ref[:, 0]) == 0 and np.count_nonzero(got[:, 0]) == 0
    assert np.all(ref[:, 1, 160:] == 0) and np.all(got[:, 1, 160:] == 0)            # t >= T: the oscillator has stopped
    print("slope %g doppler %s: max error %.3g of max |ref| %.3g" % (slope, doppler, np.abs(got - ref).max(), np.abs(ref).max()))
    np.testing.assert_allclose(got, ref, rtol=1e-10, atol=1e-12 * np.abs(ref).max())


def test_doppler_is_visible_and_slopes_differ(rts):
    contribs = random_contributions(11)
    z = lambda: np.zeros((3, 1, NB), np.complex128)
    a = rts.beat_eval(z(), 0, contribs, SLOPE, T_CUT, T0, DT, doppler=False)
    b = rts.beat_eval(z(), 0, contribs, SLOPE, T_CUT, T0, DT, doppler=True)
    c = rts.beat_eval(z(), 0, contribs, -SLOPE, T_CUT, T0, DT, doppler=False)
    assert not np.allclose(a, b, rtol=1e-6, atol=0) and not np.allclose(a, c, rtol=1e-6, atol=0)
    np.testing.assert_allclose(c, np.conj(rts.beat_eval(z(), 0, [(rx, np.conj(amp), tau, f) for rx, amp, tau, f in contribs], SLOPE, T_CUT, T0, DT,
                                                         doppler=False)), rtol=1e-10, atol=1e-12 * np.abs(c).max())


# ----------------------------------------------------------------------------- H2
@pytest.mark.parametrize("slope", [SLOPE, -SLOPE])
def test_known_answers(rts, slope):
    k0 = 40
    tau = T0 + k0 * DT                                   # on the grid: 1.3 us
    cube = rts.beat_eval(np.zeros((1, 1, NB), np.complex128), 0, [(0, 1.0 + 0.0j, tau, 0.0)], slope, 1.0, T0, DT)
    row = cube[0, 0]
    assert np.all(row[:k0] == 0) and np.count_nonzero(row[k0:]) == NB - k0           # exact zeros before the echo arrives
    np.testing.assert_allclose(np.abs(row[k0:]), 1.0, rtol=0, atol=1e-14)
    want = np.exp(-1j * math.pi * slope * tau * tau)                                  # psi(tau) = -S tau^2 + S tau^2 / 2
    assert abs(row[k0] - want) < 1e-11
    # the fast-time transform: the peak sits at |S| tau n_fft dt, reversed for an up-chirp, as it stands for a down-chirp
    n_fft = 256
    delays, reverse = rts.beat_axis(slope, n_fft, DT)
    assert reverse == (slope > 0) and delays.shape == (n_fft,) and delays[0] == 0.0
    np.testing.assert_allclose(delays[1], 1.0 / (abs(slope) * n_fft * DT), rtol=1e-15)
    z = rts.range_eval(cube, n_fft, reverse=reverse)
    peak = int(np.argmax(np.abs(z[0, 0])))
    assert peak == round(abs(slope) * tau * n_fft * DT) == 33
    assert abs(delays[peak] - tau) <= delays[1]
    wrong = rts.range_eval(cube, n_fft, reverse=not reverse)
    assert int(np.argmax(np.abs(wrong[0, 0]))) == n_fft - 33
    # the evaluator adds to what the row holds
    rng = np.random.default_rng(3)
    pre = rng.standard_normal((1, 1, NB)) + 1j * rng.standard_normal((1, 1, NB))
    got = rts.beat_eval(pre.copy(), 0, [(0, 1.0 + 0.0j, tau, 0.0)], slope, 1.0, T0, DT)
    assert np.array_equal(got, pre + cube)
    # a Doppler moves the beat frequency by f: the apparent delay by -f / S
    f = 3.0 / (n_fft * DT)                               # three bins
    zf = rts.range_eval(rts.beat_eval(np.zeros((1, 1, NB), np.complex128), 0, [(0, 1.0, tau, f)], slope, 1.0, T0, DT), n_fft, reverse=reverse)
    assert int(np.argmax(np.abs(zf[0, 0]))) == 33 - (3 if slope > 0 else -3)


# ----------------------------------------------------------------------------- H3
@pytest.fixture(scope="module")
def cube130():
    rng = np.random.default_rng(77)
    c = rng.standard_normal((2, 5, 130)) + 1j * rng.standard_normal((2, 5, 130))
    c.setflags(write=False)
    return c


@pytest.mark.parametrize("first_bin,n_samples,n_fft", [(0, 0, 256), (0, 130, 256), (3, 60, 64), (3, 64, 64), (7, 1, 2), (100, 0, 32)])
@pytest.mark.parametrize("tapered", [False, True])
def test_range_eval_equals_stft_eval_of_the_swapped_cube(rts, cube130, first_bin, n_samples, n_fft, tapered):
    cube = cube130
    ns = n_samples if n_samples else 130 - first_bin
    w = rts.window("hann", ns) + 0.125 if tapered else None
    first, count = 1, 3
    got = rts.range_eval(cube, n_fft, window=w, first=first, count=count, first_bin=first_bin, n_samples=n_samples)
    swapped = np.ascontiguousarray(cube.transpose(0, 2, 1))                      # [n_rx][bins as pulses][rows as bins]
    ref = rts.stft_eval(swapped, ns, 1, n_fft, window=w, first=first_bin, count=ns, first_bin=first, n_bins=count)
    assert ref.shape == (2, 1, n_fft, count)
    ref = np.ascontiguousarray(ref[:, 0].transpose(0, 2, 1))                     # [n_rx][rows][n_fft]
    assert got.shape == ref.shape and np.count_nonzero(ref) == ref.size
    assert np.array_equal(got.view(np.float64), ref.view(np.float64))
    # REVERSE is that result index-reversed, n_out truncates
    rev = rts.range_eval(cube, n_fft, window=w, first=first, count=count, first_bin=first_bin, n_samples=n_samples, reverse=True)
    idx = (n_fft - np.arange(n_fft)) % n_fft
    assert np.array_equal(rev.view(np.float64), np.ascontiguousarray(ref[:, :, idx]).view(np.float64))
    for n_out in (1, n_fft // 2, n_fft):
        for reverse, full in ((False, ref), (True, rev)):
            cut = rts.range_eval(cube, n_fft, window=w, first=first, count=count, first_bin=first_bin, n_samples=n_samples, n_out=n_out, reverse=reverse)
            assert cut.shape == (2, count, n_out) and np.array_equal(cut, full[:, :, :n_out])
    # against numpy's own transform, as a sanity check of the axis (tolerance: tests/test_stft_host.py's derivation)
    x = cube[:, first:first + count, first_bin:first_bin + ns] * (1.0 if w is None else w[None, None, :])
    atol = 64 * 2.0 ** -52 * math.log2(n_fft) * float(np.abs(x).sum(axis=-1).max())
    assert np.abs(got - np.fft.fft(x, n=n_fft, axis=-1)).max() <= atol


# ----------------------------------------------------------------------------- H4
def setter(**kw):
    def f(p, keep):
        for k, v in kw.items():
            setattr(p, k, v)
    return f


def reserved(i):
    def f(p, keep):
        p.reserved[i] = 1
    return f


def beat_case(L):
    """a valid raw descriptor and its arrays: (q, p, contributions, cube)"""
    q = L.RtsCubeParams(2, 3, 40, 0, T0, DT)
    p = L.RtsBeatParams()
    p.slope, p.duration, p.source, p.flags = SLOPE, 1.0, L.RTS_RENDER_RAYS, L.RTS_RENDER_DOPPLER
    c = np.zeros(4, L.BEAT_CONTRIBUTION_DTYPE)
    c["rx"] = [0, 1, 1, 0]; c["re"] = 1.0; c["delay"] = T0 + np.arange(4) * DT; c["doppler"] = 1.0e5
    return q, p, c, np.full((2, 3, 40, 2), 7.25)


def test_beat_eval_refusals(rts):
    from rts_amd import _lib as L
    lib = L.lib()

    def call(q, p, c, cube, pulse=1, n=None):
        return lib.rts_beat_eval(C.byref(q) if q is not None else None, C.byref(p) if p is not None else None, c.ctypes.data if c is not None else None,
                                 len(c) if n is None else n, pulse, cube.ctypes.data if cube is not None else None)
    q, p, c, cube = beat_case(L)
    assert call(q, p, c, cube) == L.RTS_OK
    assert np.all(cube[:, 0] == 7.25) and np.all(cube[:, 2] == 7.25) and np.count_nonzero(cube[:, 1] != 7.25) > 100
    bad = [("slope 0", setter(slope=0.0), b"slope"), ("slope nan", setter(slope=math.nan), b"slope"), ("slope inf", setter(slope=-math.inf), b"slope"),
           ("duration 0", setter(duration=0.0), b"duration"), ("duration < 0", setter(duration=-1.0), b"duration"),
           ("duration nan", setter(duration=math.nan), b"duration"), ("duration inf", setter(duration=math.inf), b"duration"),
           ("source", setter(source=2), b"source"), ("flags", setter(flags=2), b"flags"),
           ("reserved 0", reserved(0), b"reserved"), ("reserved 1", reserved(1), b"reserved")]
    for name, mutate, word in bad:
        q, p, c, cube = beat_case(L)
        mutate(p, None)
        assert call(q, p, c, cube) == L.RTS_ERR_INVALID, name
        assert word in lib.rts_last_error(), (name, lib.rts_last_error())
        assert np.all(cube == 7.25), name
    q, p, c, cube = beat_case(L)
    assert call(q, p, c, cube, pulse=3) == L.RTS_ERR_INVALID and b"pulse_index" in lib.rts_last_error()
    assert call(q, p, c, cube, pulse=0xffffffff) == L.RTS_ERR_INVALID
    assert call(q, None, c, cube) == L.RTS_ERR_INVALID and call(None, p, c, cube) == L.RTS_ERR_INVALID
    assert call(q, p, None, cube, n=4) == L.RTS_ERR_INVALID and call(q, p, c, None) == L.RTS_ERR_INVALID
    big = L.RtsCubeParams(65536, 3, 40, 0, T0, DT)
    assert call(big, p, c, cube) == L.RTS_ERR_INVALID and b"n_rx" in lib.rts_last_error()
    assert np.all(cube == 7.25)
    assert call(q, p, None, cube, n=0) == L.RTS_OK and np.all(cube == 7.25)           # no contributions: nothing to add
    with pytest.raises(L.RtsError):
        rts.beat_eval(np.zeros((1, 1, 8)), 0, [], 0.0, 1.0, T0, DT)


def range_case(L, n_rx=2, rows=6, nb=20):
    """a valid raw descriptor and its arrays: (q, cube, p, keep); the output is 2 x 4 rows x 8 bins complex"""
    q = L.RtsCubeParams(n_rx, rows, nb, 0, 0.0, 1.0)
    cube = np.ones((n_rx, rows, nb, 2))
    w = np.linspace(0.5, 1.5, 12)
    p = L.RtsRangeParams()
    p.first_pulse, p.n_pulses, p.first_bin, p.n_samples, p.n_fft, p.n_out, p.flags = 1, 4, 3, 12, 16, 8, L.RTS_RANGE_REVERSE
    p.window = w.ctypes.data
    return q, cube, p, dict(w=w)


def test_range_eval_refusals(rts):
    from rts_amd import _lib as L
    lib = L.lib()

    def poison(index, value):
        def f(p, keep):
            keep["w"][index] = value
        return f
    out = np.full((2, 4, 8, 2), 7.25)
    q, cube, p, keep = range_case(L)
    assert lib.rts_range_eval(C.byref(q), cube.ctypes.data, C.byref(p), out.ctypes.data) == L.RTS_OK and not np.any(out == 7.25)
    bad = [("reserved0", setter(reserved0=1), b"reserved"), ("reserved 0", reserved(0), b"reserved"), ("reserved 1", reserved(1), b"reserved"),
           ("unknown flag", setter(flags=2), b"flags"),
           ("n_fft 0", setter(n_fft=0), b"n_fft"), ("n_fft 1", setter(n_fft=1, n_samples=1, n_out=1), b"n_fft"), ("n_fft 12", setter(n_fft=12), b"n_fft"),
           ("n_fft 8192", setter(n_fft=8192), b"n_fft"),
           ("n_samples > n_fft", setter(n_fft=8), b"n_samples"), ("default n_samples > n_fft", setter(n_samples=0, window=None), b"n_samples"),
           ("first_bin beyond the row", setter(first_bin=20), b"first_bin"), ("gate beyond the row", setter(first_bin=9), b"n_samples"),
           ("wrapping gate", setter(n_samples=0xffffffff), b"n_samples"),
           ("n_out > n_fft", setter(n_out=17), b"n_out"),
           ("no pulses", setter(n_pulses=0), b"n_pulses"), ("pulses beyond the cube", setter(first_pulse=3), b"n_pulses"),
           ("first beyond the cube", setter(first_pulse=6), b"first_pulse"), ("wrapping pulse range", setter(first_pulse=0xffffffff), b"first_pulse"),
           ("window nan", poison(2, math.nan), b"window"), ("window inf", poison(11, math.inf), b"window")]
    for name, mutate, word in bad:
        q, cube, p, keep = range_case(L)
        mutate(p, keep)
        out[:] = 7.25
        assert lib.rts_range_eval(C.byref(q), cube.ctypes.data, C.byref(p), out.ctypes.data) == L.RTS_ERR_INVALID, name
        assert word in lib.rts_last_error(), (name, lib.rts_last_error())
        assert np.all(out == 7.25), name
    q, cube, p, keep = range_case(L)
    assert lib.rts_range_eval(C.byref(q), cube.ctypes.data, None, out.ctypes.data) == L.RTS_ERR_INVALID
    assert lib.rts_range_eval(None, cube.ctypes.data, C.byref(p), out.ctypes.data) == L.RTS_ERR_INVALID
    assert lib.rts_range_eval(C.byref(q), None, C.byref(p), out.ctypes.data) == L.RTS_ERR_INVALID
    assert lib.rts_range_eval(C.byref(q), cube.ctypes.data, C.byref(p), None) == L.RTS_ERR_INVALID
    # a shape the launch grid cannot take: 2^31 rows of 4096 points, one per workgroup (the check comes before any sample is read)
    big = L.RtsCubeParams(65536, 32768, 20, 0, 0.0, 1.0)
    q, cube, p, keep = range_case(L)
    p.first_pulse, p.n_pulses, p.n_fft = 0, 32768, 4096
    assert lib.rts_range_eval(C.byref(big), cube.ctypes.data, C.byref(p), out.ctypes.data) == L.RTS_ERR_INVALID and b"launch grid" in lib.rts_last_error()
    assert np.all(out == 7.25)
    # accepted edges: n_samples == n_fft, n_out 0 (all bins), a NULL window, n_fft 2 and 4096
    for kw, n_out in ((dict(n_samples=16, window=None), 8), (dict(n_out=0), 16), (dict(window=None), 8), (dict(n_fft=4096, n_out=0), 4096),
                      (dict(n_fft=2, n_samples=2, n_out=0, window=None), 2)):
        q, cube, p, keep = range_case(L)
        for k, v in kw.items():
            setattr(p, k, v)
        big_out = np.full(2 * 4 * n_out * 2 + 1, 7.25)
        assert lib.rts_range_eval(C.byref(q), cube.ctypes.data, C.byref(p), big_out.ctypes.data) == L.RTS_OK, kw
        assert not np.any(big_out[:-1] == 7.25) and big_out[-1] == 7.25, kw
    with pytest.raises(ValueError):
        rts.range_eval(np.zeros((1, 2, 8)), 8, window=np.ones(3))


# ----------------------------------------------------------------------------- rts_beat.h alone, under the sanitizers
@pytest.fixture(scope="module")
def beat_main(tmp_path_factory):
    gxx = shutil.which("g++")
    if not gxx:
        pytest.skip("no g++")
    rt = subprocess.run([gxx, "-print-file-name=libasan.so"], capture_output=True, text=True).stdout.strip()
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"] if os.path.isabs(rt) and os.path.exists(rt) else []
    exe = str(tmp_path_factory.mktemp("beat") / "beat_main")
    subprocess.check_call([gxx, "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-ffp-contract=off"] + san + ["-I", os.path.join(ROOT, "rts_amd", "csrc"),
                           os.path.join(ROOT, "tests", "beat", "beat_main.cpp"), "-o", exe])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:verify_asan_link_order=0", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")

    def ask(cases, kind=float):
        text = "".join(" ".join(repr(x) if isinstance(x, float) else str(x) for x in c) + "\n" for c in cases)
        r = subprocess.run([exe], input=text, capture_output=True, text=True, env=env, timeout=120)
        assert r.returncode == 0, r.stderr[-3000:]
        out = [[kind(x) for x in line.split()] for line in r.stdout.splitlines()]
        assert len(out) == len(cases)
        return out
    return ask


def main_contributions(n, n_rx, nb, t0, dt):
    """the contributions tests/beat/beat_main.cpp forms"""
    out = []
    for k in range(n):
        tau = t0 + dt * (((k * 37) % (nb + 40)) - 20.0 + 0.25 * (k % 4))
        if k % 13 == 5:
            tau = math.inf if k % 2 else (math.nan if k % 4 else -math.inf)
        out.append((k % (n_rx + 2) - 1, complex((((k * 7) % 11) - 5.0) / 4.0, (((k * 3) % 7) - 3.0) / 4.0), tau, ((k % 9) - 4.0) * 2.5e5))
    return out


def main_cube(n_rx, rows, nb):
    """the cube tests/beat/beat_main.cpp fills"""
    r = np.arange(n_rx)[:, None, None]; p = np.arange(rows)[None, :, None]; b = np.arange(nb)[None, None, :]
    re = ((r * 131 + p * 17 + b * 7) % 23) - 11.0 + 0.25 * p
    im = ((r * 5 + p * 3 + b * 11) % 19) - 9.0 - 0.5 * b
    return re + 1j * im


def test_header_alone_reads_only_what_it_is_given(beat_main):
    """the contributions, cube, work, window and output are heap arrays of exactly their sizes, and every cube sample outside the span's
    rows and the gate is poisoned in the driver: a read or write beyond them ends the run"""
    beat_cases = [("beat", n_rx, 3, nb, pulse, cnt, T0, DT, slope, dur, dop)
                  for (n_rx, nb, pulse, cnt) in ((3, 200, 1, 150), (1, 16, 0, 40), (2, 17, 2, 40), (2, 1, 0, 9), (1, 33, 1, 0))
                  for slope in (SLOPE, -SLOPE) for dur in (T0 + 0.6 * nb * DT, 1.0) for dop in (0, 1)]
    for c, g in zip(beat_cases, beat_main(beat_cases)):
        _, n_rx, rows, nb, pulse, cnt, t0, dt, slope, dur, dop = c
        ref = beat_ref(np.zeros((n_rx, rows, nb), np.complex128), pulse, main_contributions(cnt, n_rx, nb, t0, dt), slope, dur, t0, dt, bool(dop))
        got = np.array(g).reshape(n_rx, rows, nb, 2)
        got = got[..., 0] + 1j * got[..., 1]
        np.testing.assert_allclose(got, ref, rtol=1e-10, atol=1e-12 * max(np.abs(ref).max(), 1e-300), err_msg=str(c))
        assert cnt == 0 or nb < 16 or np.count_nonzero(ref) > 0
    range_cases = [("range", 2, 7, 21, first, count, first_bin, ns, n_fft, n_out, flags, tapered)
                   for (first, count) in ((0, 7), (2, 3), (6, 1)) for (first_bin, ns, n_fft) in ((0, 0, 32), (5, 16, 16), (20, 1, 2), (3, 7, 64), (0, 21, 4096))
                   for n_out in (0, 1, n_fft // 2) for flags in (0, 1) for tapered in (0, 1)
                   if n_fft < 4096 or (count == 1 and n_out == 1)]
    cube = main_cube(2, 7, 21)
    for c, g in zip(range_cases, beat_main(range_cases)):
        _, n_rx, rows, nb, first, count, first_bin, ns, n_fft, n_out, flags, tapered = c
        ns = ns if ns else nb - first_bin
        w = 0.5 + 0.25 * np.arange(ns) if tapered else np.ones(ns)
        x = cube[:, first:first + count, first_bin:first_bin + ns] * w[None, None, :]
        ref = np.fft.fft(x, n=n_fft, axis=-1)
        if flags & 1:
            ref = ref[:, :, (n_fft - np.arange(n_fft)) % n_fft]
        ref = ref[:, :, :n_out if n_out else n_fft]
        got = np.array(g); got = (got[0::2] + 1j * got[1::2]).reshape(ref.shape)
        atol = 64 * 2.0 ** -52 * math.log2(n_fft) * float(np.abs(x).sum(axis=-1).max())
        assert np.abs(got - ref).max() <= atol, c


def test_plans(beat_main):
    consts = beat_main([("consts",)], int)[0]
    assert consts == [16, 64, 64, 1024, 1024, 8, 64, 4096, 256, 16, 4096, 2 ** 31 - 1]
    plan = lambda *a: beat_main([("beatplan",) + a], int)[0]
    # one launch: a set of up to 64 records, whatever the cube; no scratch
    for R in (0, 1, 64):
        assert plan(R, 4, 4096, 0)[1:] == [1, max(R, 1), 0, 1]
    assert plan(64, 4, 4096, 0)[0] == 4 and plan(1, 1, 1, 0)[0] == 1 and plan(1, 1, 1025, 0)[0] == 2
    # above it: as many parts as fill 1024 workgroups, none shorter than 8 records, at most 64; no empty part
    assert plan(65, 1, 1024, 0) == [1, 8, 9, 2 * 8 * 1024, 1]                   # 65 // 8 = 8 parts of 9 (the last: 2)
    assert plan(230, 4, 4096, 0) == [4, 26, 9, 2 * 26 * 4 * 4096, 1]            # 28 parts of at least 8 wanted: 9 each make 26
    assert plan(230, 4, 1024, 0)[1] == 26
    assert plan(100000, 1, 1024, 0)[1:3] == [64, 1563]                           # RTS_BEAT_MAX_PARTS
    assert plan(100000, 4, 65536, 0)[:3] == [64, 4, 25000]                       # 256 workgroups per part: four parts fill the device
    assert plan(100000, 16, 2 ** 20, 0)[1] == 1                                  # the grid is full without parts
    assert plan(2 ** 32 - 1, 1, 1024, 0)[4] == 1 and plan(2 ** 32, 1, 1024, 0)[4] == 0
    assert plan(100, 65535, 16, 0)[4] == 1 and plan(100, 65536, 16, 0)[4] == 0
    # forced parts (the tests' switch): as far as the set has records
    assert plan(230, 4, 4096, 1)[1:4] == [1, 230, 0] and plan(230, 4, 4096, 64)[1:3] == [58, 4] and plan(30, 2, 200, 64)[1:3] == [30, 1]
    assert plan(30, 2, 200, 64)[3] == 2 * 30 * 2 * 200
    for R, force in ((230, 0), (230, 64), (1000, 7), (65, 0), (99999, 0)):
        _, P, part_len, _, _ = plan(R, 3, 200, force)
        assert (P - 1) * part_len < R <= P * part_len
    # the range transform: rows per workgroup and LDS at the edges
    rplan = lambda *a: beat_main([("rangeplan",) + a], int)[0]
    for n_fft in [2 << e for e in range(12)]:
        logN, RT, ns, n_out, groups, rows, lds, out_doubles, ok = rplan(3, 5, n_fft, n_fft, 0)
        assert 1 << logN == n_fft and RT == min(16, 4096 // n_fft) and lds == 16 * n_fft * RT + 8 * n_fft <= 160 * 1024
        assert RT * n_fft <= 16 * 256                                               # the kernel's elements per thread and pass
        assert (ns, n_out, rows, groups, out_doubles, ok) == (n_fft, n_fft, 15, -(-15 // RT), 2 * 15 * n_fft, 1)
    assert rplan(1, 1, 1, 2, 1)[:5] == [1, 16, 1, 1, 1] and rplan(1, 1, 1, 2, 1)[6] == 16 * 2 * 16 + 16
    assert rplan(1, 1, 4096, 4096, 0)[6] == 96 * 1024
    assert rplan(4, 17, 100, 128, 5)[3:6] == [5, 5, 68] and rplan(4, 17, 100, 128, 5)[7] == 2 * 68 * 5
    assert rplan(65536, 32768, 1, 4096, 1)[8] == 0 and rplan(65535, 32768, 1, 4096, 1)[8] == 1      # 2^31 workgroups, one fewer row set
    assert rplan(65536, 32768, 1, 2048, 1)[8] == 1                                                   # two rows per workgroup
