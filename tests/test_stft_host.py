"""The tapered slow-time spectrogram on the host (no GPU): rts_stft_eval against an independent numpy restatement of the definition
in include/rts_amd.h (RtsStftParams) -- np.fft.fft of the windowed, zero-padded segments --, known answers, the masking a taper
removes, a micro-Doppler ridge, rts_window_make against its formulas, the validation of malformed descriptors, and
rts_amd/csrc/rts_stft.h alone under AddressSanitizer + UndefinedBehaviorSanitizer (tests/stft/stft_main.cpp).

The tolerance of the comparison with the restatement is derived, not measured.  A radix-2 f64 FFT whose twiddles are good to a few
ulp has an error of at most about 5 2^-53 log2(n_fft) ||x||_2 per output, and numpy's own transform errs by the same order;
||x||_2 <= sum_i |x_i| <= B with B = sum_i |w_i| max|y|.  So  atol = 64 2^-52 log2(n_fft) B  (64: the two sides' ~5 2^-53 each with a
factor of about 12 to spare).  A power re^2 + im^2 of an output of magnitude at most B moves by at most 2 B times the output's
error, so the power forms use 2 B atol.  A wrong index, frame start or sign is an error of order B / window_len or more."""
import ctypes as C
import math
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CS = 299792458.0
EPS = 2.0 ** -52

CASES = [(1, 1, 2), (5, 3, 8), (16, 16, 16), (16, 40, 64), (64, 1, 64), (33, 7, 64)]      # (window_len, hop, n_fft)
GATES = [(0, 0), (5, 1), (0, 9), (31, 17)]                                                 # (first_bin, n_bins); (31, 17) ends on the last of 48 bins
FORMS = [dict(power=False, sum_bins=False), dict(power=True, sum_bins=False), dict(power=True, sum_bins=True)]


# ----------------------------------------------------------------------------- numpy restatement (from the header's text)
def stft_ref(cube, window_len, hop, n_fft, window=None, first=0, count=None, first_bin=0, n_bins=0):
    """complex [n_rx][n_frames][n_fft][n_gate]: the DFT of every whole frame's windowed, zero-padded samples"""
    n_rx, n_p, nb = cube.shape
    count = n_p - first if count is None else count
    G = n_bins if n_bins else nb - first_bin
    n_frames = 1 + (count - window_len) // hop
    w = np.ones(window_len) if window is None else np.asarray(window, np.float64)
    out = np.zeros((n_rx, n_frames, n_fft, G), np.complex128)
    for f in range(n_frames):
        p0 = first + f * hop
        seg = cube[:, p0:p0 + window_len, first_bin:first_bin + G] * w[None, :, None]
        out[:, f] = np.fft.fft(seg, n=n_fft, axis=1)
    return out


def as_form(z, power=False, sum_bins=False):
    if not power:
        return z
    p = z.real * z.real + z.imag * z.imag
    return p.sum(axis=-1) if sum_bins else p


def bound(n_fft, window_len, window, ymax, power=False):
    B = float(np.abs(window).sum() if window is not None else window_len) * ymax
    atol = 64 * EPS * math.log2(n_fft) * B
    return (2 * B * atol if power else atol), B


def random_cube(seed, n_rx=2, rows=130, nb=48):
    rng = np.random.default_rng(seed)
    return rng.standard_normal((n_rx, rows, nb)) + 1j * rng.standard_normal((n_rx, rows, nb))


@pytest.fixture(scope="module")
def cube130():
    c = random_cube(2024)
    c.setflags(write=False)
    return c


# ----------------------------------------------------------------------------- H1
@pytest.mark.parametrize("window_len,hop,n_fft", CASES)
def test_eval_against_restatement(rts, cube130, window_len, hop, n_fft):
    cube = cube130
    ymax = float(np.abs(cube).max())
    for first in (0, 3):
        count = 120                                          # leaves left-over pulses in every case, and rows of the cube beyond the span
        assert (count - window_len) % hop != 0 or hop == 1
        for window in (None, rts.window("hann", window_len)):
            for first_bin, n_bins in GATES:
                ref = stft_ref(cube, window_len, hop, n_fft, window, first, count, first_bin, n_bins)
                for form in FORMS:
                    got = rts.stft_eval(cube, window_len, hop, n_fft, window=window, first=first, count=count, first_bin=first_bin, n_bins=n_bins, **form)
                    want = as_form(ref, **form)
                    atol, B = bound(n_fft, window_len, window, ymax, form["power"])
                    assert got.shape == want.shape and got.dtype == want.dtype
                    err = float(np.abs(got - want).max())
                    if first == 0 and (first_bin, n_bins) == (0, 0):
                        print("(%d, %d, %d) window %s %s: max error %.3g, bound %.3g, B %.3g" % (window_len, hop, n_fft, window is not None, form, err, atol, B))
                    assert err <= atol, (first, window is not None, first_bin, n_bins, form, err, atol)
                    assert np.abs(want).max() > (B / window_len) ** (2 if form["power"] else 1) * 1e-3


# ----------------------------------------------------------------------------- H2
def test_known_answers(rts):
    N, k0 = 64, 11
    i = np.arange(N)
    cube = np.zeros((1, N, 3), np.complex128)
    cube[0, :, 1] = np.exp(2j * np.pi * k0 * i / N)          # an on-grid tone
    cube[0, 5, 2] = 0.75 - 0.5j                              # a single nonzero pulse
    z = rts.stft_eval(cube, N, 1, N)
    assert z.shape == (1, 1, N, 3)
    atol, _ = bound(N, N, None, 1.0)
    assert abs(abs(z[0, 0, k0, 1]) - N) <= atol
    others = np.delete(np.abs(z[0, 0, :, 1]), k0)
    assert others.max() < atol
    assert np.all(z[0, 0, :, 0] == 0)
    np.testing.assert_allclose(np.abs(z[0, 0, :, 2]), abs(0.75 - 0.5j), rtol=0, atol=atol)
    # window_len == 1: every row of a frame is the frame's one sample (times the window)
    rng = np.random.default_rng(4)
    c1 = rng.standard_normal((2, 7, 5)) + 1j * rng.standard_normal((2, 7, 5))
    z1 = rts.stft_eval(c1, 1, 2, 4, window=[1.5])
    assert z1.shape == (2, 4, 4, 5)
    for f in range(4):
        for k in range(4):
            assert np.array_equal(z1[:, f, k, :], 1.5 * c1[:, 2 * f, :])
    # Parseval: sum_k |X_k|^2 = n_fft sum_i |x_i|^2
    cube = random_cube(9, rows=40, nb=6)
    w = rts.window("hamming", 33)
    n_fft = 128
    p = rts.stft_eval(cube, 33, 7, n_fft, window=w, power=True)
    x = np.stack([cube[:, 7 * f:7 * f + 33, :] * w[None, :, None] for f in range(p.shape[1])], axis=1)
    atol, B = bound(n_fft, 33, w, float(np.abs(cube).max()), power=True)
    np.testing.assert_allclose(p.sum(axis=2), n_fft * (np.abs(x) ** 2).sum(axis=2), rtol=0, atol=n_fft * atol)


# ----------------------------------------------------------------------------- H3
def masking_cubes(n=64):
    i = np.arange(n)
    strong = np.exp(2j * np.pi * 20.5 * i / n).reshape(1, n, 1)
    weak = 1e-3 * np.exp(2j * np.pi * 29.0 * i / n).reshape(1, n, 1)
    return strong, weak


def test_masking(rts):
    """a unit tone between bins 20 and 21 against a -60 dB tone on bin 29, 64 pulses: under the rectangular window the strong tone's
    leak at row 29 is 1 487 times the weak tone's power there, under a Blackman taper 0.039 times (numpy)"""
    strong, weak = masking_cubes()
    ps = rts.stft_eval(strong, 64, 1, 64, power=True)[0, 0, :, 0]
    pw = rts.stft_eval(weak, 64, 1, 64, power=True)[0, 0, :, 0]
    print("rectangular: leak / weak at row 29 = %.4g" % (ps[29] / pw[29]))
    assert ps[29] > 100 * pw[29]
    w = rts.window("blackman", 64)
    ps = rts.stft_eval(strong, 64, 1, 64, window=w, power=True)[0, 0, :, 0]
    pw = rts.stft_eval(weak, 64, 1, 64, window=w, power=True)[0, 0, :, 0]
    print("blackman: leak / weak at row 29 = %.4g" % (ps[29] / pw[29]))
    assert ps[29] < 0.1 * pw[29]
    both = rts.stft_eval(strong + weak, 64, 1, 64, window=w, power=True)[0, 0, :, 0]
    assert both[29] > both[28] and both[29] > both[30]


# ----------------------------------------------------------------------------- H4
def micro_doppler_case():
    """one gate, 2 048 pulses at pri 1e-4 s of a scatterer at 1000 + 0.5 sin(2 pi 4 t) m, fc 10 GHz: (cube, pri, fc, dtau_dt(t))"""
    n, pri, fc = 2048, 1e-4, 10e9
    t = np.arange(n) * pri
    tau = 2 * (1000 + 0.5 * np.sin(2 * np.pi * 4 * t)) / CS
    ph = -np.fmod(2 * np.pi * fc * tau, 2 * np.pi)
    cube = np.exp(1j * ph).reshape(1, n, 1)
    return cube, pri, fc, lambda tt: 2 * 0.5 * 2 * np.pi * 4 * np.cos(2 * np.pi * 4 * tt) / CS


def test_micro_doppler_ridge(rts):
    """the ridge of a vibrating scatterer: in every frame the peak row lies within 1.5 rows of -fc dtau/dt pri n_fft at the frame's
    centre -- half a row of quantisation plus half of the 1.73 rows the ridge sweeps inside one window (numpy: worst frame 0.49; the
    excursion is +-10.7 rows, so a sign error misses by up to 21)"""
    cube, pri, fc, dtau_dt = micro_doppler_case()
    wl, hop, n_fft = 64, 32, 128
    p = rts.stft_eval(cube, wl, hop, n_fft, window=rts.window("hann", wl), power=True)[0, :, :, 0]
    assert p.shape == (63, n_fft)
    centres, doppler = rts.spectrogram_axes(wl, hop, n_fft, 2048, pri)
    np.testing.assert_array_equal(centres, np.arange(63) * 32 + 31.5)
    kk = np.arange(n_fft); kk = np.where(kk >= 64, kk - 128, kk)
    np.testing.assert_allclose(doppler, kk / (n_fft * pri), rtol=1e-15)
    assert doppler[0] == 0 and doppler[64] < 0 and doppler[63] > 0
    want_hz = -fc * dtau_dt(centres * pri)
    peak_hz = doppler[np.argmax(p, axis=1)]
    miss = np.abs(peak_hz - want_hz) * n_fft * pri
    print("ridge: worst frame misses by %.3g rows; excursion %.3g rows" % (miss.max(), np.abs(want_hz).max() * n_fft * pri))
    assert miss.max() <= 1.5
    assert np.abs(want_hz).max() * n_fft * pri > 10
    # the axes of a later span
    c3, _ = rts.spectrogram_axes(5, 3, 8, 12, pri, first=3)
    np.testing.assert_array_equal(c3, 3 + np.arange(3) * 3 + 2.0)


# ----------------------------------------------------------------------------- H5
COEFFS = {"rect": (1.0, 0.0, 0.0), "hann": (0.5, 0.5, 0.0), "hamming": (0.54, 0.46, 0.0), "blackman": (0.42, 0.5, 0.08)}


@pytest.mark.parametrize("n", [1, 2, 64, 65])
def test_window_make(rts, n):
    from rts_amd import _lib as L
    for kind, (a0, a1, a2) in COEFFS.items():
        w = rts.window(kind, n)
        assert w.shape == (n,)
        if n == 1:
            assert w[0] == 1.0
            continue
        i = np.arange(n)
        want = a0 - a1 * np.cos(2 * np.pi * i / (n - 1)) + a2 * np.cos(4 * np.pi * i / (n - 1))
        np.testing.assert_allclose(w, want, rtol=0, atol=4 * EPS)
        assert np.array_equal(w, w[::-1])
        if kind == "rect":
            assert np.all(w == 1.0)
        if kind == "hann":
            assert w[0] == 0.0 and w[-1] == 0.0
        if kind == "blackman":
            assert abs(w[0]) <= EPS and abs(w[-1]) <= EPS
        if n == 65:
            assert abs(w[32] - (a0 + a1 + a2)) <= 2 * EPS
    assert np.array_equal(rts.window(L.RTS_WINDOW_HANN, n), rts.window("hann", n))
    lib = L.lib()
    out = np.full(4, 7.25)
    assert lib.rts_window_make(0, 0, out.ctypes.data) == L.RTS_ERR_INVALID
    assert lib.rts_window_make(4, 4, out.ctypes.data) == L.RTS_ERR_INVALID and b"kind" in lib.rts_last_error()
    assert lib.rts_window_make(1, 4, None) == L.RTS_ERR_INVALID
    assert np.all(out == 7.25)


# ----------------------------------------------------------------------------- H6
def raw_case(L, n_rx=2, rows=12, nb=6):
    """a valid raw descriptor and its arrays: (q, cube, p, keep); the output is 2 x 3 frames x 8 rows x 4 bins complex"""
    q = L.RtsCubeParams(n_rx, rows, nb, 0, 0.0, 1.0)
    cube = np.ones((n_rx, rows, nb, 2))
    w = np.linspace(0.5, 1.5, 5)
    p = L.RtsStftParams()
    p.first_pulse, p.n_pulses, p.window_len, p.hop, p.n_fft, p.first_bin, p.n_bins, p.flags = 1, 11, 5, 3, 8, 1, 4, 0
    p.window = w.ctypes.data
    return q, cube, p, dict(w=w)


def bad_stft_params(L):
    """(name, mutate(p, keep), word the message must hold) for every refusal the header lists (bar the attached-cube test and the
    launch grid's limits)"""
    def setter(**kw):
        def f(p, keep):
            for k, v in kw.items():
                setattr(p, k, v)
        return f

    def poison(index, value):
        def f(p, keep):
            keep["w"][index] = value
        return f

    def reserved(i):
        def f(p, keep):
            p.reserved[i] = 1
        return f

    return [
        ("reserved 0", reserved(0), b"reserved"), ("reserved 1", reserved(1), b"reserved"),
        ("unknown flag", setter(flags=4), b"flags"), ("sum without power", setter(flags=L.RTS_STFT_SUM_BINS), b"RTS_STFT_POWER"),
        ("n_fft 0", setter(n_fft=0), b"n_fft"), ("n_fft 1", setter(n_fft=1, window_len=1), b"n_fft"), ("n_fft 12", setter(n_fft=12), b"n_fft"),
        ("n_fft 8192", setter(n_fft=8192), b"n_fft"),
        ("window_len 0", setter(window_len=0), b"window_len"), ("window_len > n_fft", setter(window_len=9), b"window_len"),
        ("window_len > n_pulses", setter(n_pulses=4), b"window_len"),
        ("hop 0", setter(hop=0), b"hop"),
        ("no pulses", setter(n_pulses=0), b"n_pulses"), ("pulses beyond the cube", setter(first_pulse=2), b"n_pulses"),
        ("first beyond the cube", setter(first_pulse=12), b"first_pulse"), ("wrapping pulse range", setter(first_pulse=0xffffffff), b"first_pulse"),
        ("first_bin beyond the cube", setter(first_bin=6), b"first_bin"), ("gate beyond the cube", setter(first_bin=3), b"n_bins"),
        ("wrapping gate", setter(n_bins=0xffffffff), b"n_bins"),
        ("window nan", poison(2, math.nan), b"window"), ("window inf", poison(4, math.inf), b"window"),
    ]


def test_malformed_descriptors_are_rejected(rts):
    from rts_amd import _lib as L
    lib = L.lib()
    out = np.full((2, 3, 8, 4, 2), 7.25)
    nf = C.c_uint32(99)
    q, cube, p, keep = raw_case(L)
    assert lib.rts_stft_eval(C.byref(q), cube.ctypes.data, C.byref(p), out.ctypes.data, C.byref(nf)) == L.RTS_OK
    assert nf.value == 3 and not np.any(out == 7.25)
    for name, mutate, word in bad_stft_params(L):
        q, cube, p, keep = raw_case(L)
        mutate(p, keep)
        out[:] = 7.25; nf.value = 99
        assert lib.rts_stft_eval(C.byref(q), cube.ctypes.data, C.byref(p), out.ctypes.data, C.byref(nf)) == L.RTS_ERR_INVALID, name
        assert word in lib.rts_last_error(), (name, lib.rts_last_error())
        assert np.all(out == 7.25) and nf.value == 99, name
    q, cube, p, keep = raw_case(L)
    assert lib.rts_stft_eval(C.byref(q), cube.ctypes.data, None, out.ctypes.data, None) == L.RTS_ERR_INVALID
    assert lib.rts_stft_eval(None, cube.ctypes.data, C.byref(p), out.ctypes.data, None) == L.RTS_ERR_INVALID
    assert lib.rts_stft_eval(C.byref(q), None, C.byref(p), out.ctypes.data, None) == L.RTS_ERR_INVALID
    assert lib.rts_stft_eval(C.byref(q), cube.ctypes.data, C.byref(p), None, None) == L.RTS_ERR_INVALID
    assert np.all(out == 7.25)
    # the launch grid: more receivers than it takes (the check comes before any sample is read)
    big = L.RtsCubeParams(65536, 12, 6, 0, 0.0, 1.0)
    assert lib.rts_stft_eval(C.byref(big), cube.ctypes.data, C.byref(p), out.ctypes.data, None) == L.RTS_ERR_INVALID and b"n_rx" in lib.rts_last_error()
    # accepted edge cases: window_len == n_pulses (one frame), hop > n_pulses (one frame), n_bins == 0 (to the last bin), a NULL window
    for kw, frames in ((dict(n_pulses=5), 1), (dict(hop=1000), 1), (dict(n_bins=0), 3), (dict(window=None), 3), (dict(n_fft=4096), 3)):
        q, cube, p, keep = raw_case(L)
        for k, v in kw.items():
            setattr(p, k, v)
        big_out = np.zeros(2 * 3 * p.n_fft * 5 * 2)
        assert lib.rts_stft_eval(C.byref(q), cube.ctypes.data, C.byref(p), big_out.ctypes.data, C.byref(nf)) == L.RTS_OK, kw
        assert nf.value == frames, kw
    with pytest.raises(ValueError):
        rts.stft_eval(np.zeros((1, 8, 4)), 4, 1, 4, window=np.ones(3))


# ----------------------------------------------------------------------------- rts_stft.h alone, under the sanitizers
@pytest.fixture(scope="module")
def stft_main(tmp_path_factory):
    gxx = shutil.which("g++")
    if not gxx:
        pytest.skip("no g++")
    rt = subprocess.run([gxx, "-print-file-name=libasan.so"], capture_output=True, text=True).stdout.strip()
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"] if os.path.isabs(rt) and os.path.exists(rt) else []
    exe = str(tmp_path_factory.mktemp("stft") / "stft_main")
    subprocess.check_call([gxx, "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-ffp-contract=off"] + san + ["-I", os.path.join(ROOT, "rts_amd", "csrc"),
                           os.path.join(ROOT, "tests", "stft", "stft_main.cpp"), "-o", exe])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:verify_asan_link_order=0", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")

    def ask(cases, kind=float):
        text = "".join(" ".join(str(x) for x in c) + "\n" for c in cases)
        r = subprocess.run([exe], input=text, capture_output=True, text=True, env=env, timeout=120)
        assert r.returncode == 0, r.stderr[-3000:]
        out = [[kind(x) for x in line.split()] for line in r.stdout.splitlines()]
        assert len(out) == len(cases)
        return out
    return ask


def main_cube(n_rx, rows, nb):
    """the cube tests/stft/stft_main.cpp fills"""
    r = np.arange(n_rx)[:, None, None]; p = np.arange(rows)[None, :, None]; b = np.arange(nb)[None, None, :]
    re = ((r * 131 + p * 17 + b * 7) % 23) - 11.0 + 0.25 * p
    im = ((r * 5 + p * 3 + b * 11) % 19) - 9.0 - 0.5 * b
    return re + 1j * im


def test_header_alone_reads_only_its_span_and_gate(stft_main):
    """every sample outside the whole frames of the span and outside the gate is poisoned in the driver: a read of one ends the run"""
    cases = []
    for window_len, hop, n_fft in CASES:
        for first, count in ((0, 40 if window_len < 64 else 70), (3, 67)):
            for first_bin, n_gate in ((0, 11), (5, 1), (2, 9)):
                for flags in (0, 1, 3):
                    for tapered in (0, 1):
                        cases.append(("eval", 2, 70, 11, first, count, window_len, hop, n_fft, first_bin, n_gate, flags, tapered))
    got = stft_main(cases)
    cube = main_cube(2, 70, 11)
    for c, g in zip(cases, got):
        _, n_rx, rows, nb, first, count, window_len, hop, n_fft, first_bin, n_gate, flags, tapered = c
        w = 0.5 + 0.25 * np.arange(window_len) if tapered else None
        ref = as_form(stft_ref(cube, window_len, hop, n_fft, w, first, count, first_bin, n_gate), power=bool(flags & 1), sum_bins=bool(flags & 2))
        assert int(g[0]) == ref.shape[1]
        vals = np.array(g[1:])
        vals = vals if flags & 1 else vals[0::2] + 1j * vals[1::2]
        atol, _ = bound(n_fft, window_len, w, float(np.abs(cube).max()), bool(flags & 1))
        assert vals.shape == (ref.size,) and np.abs(vals - ref.ravel()).max() <= atol, c


def test_launch_plan(stft_main):
    lds_max, threads, max_fft, tile, max_rx, max_x = stft_main([("consts",)], int)[0]
    assert (lds_max, threads, max_fft, tile, max_rx, max_x) == (160 * 1024, 256, 4096, 8, 65535, 2 ** 31 - 1)
    assert [r[0] for r in stft_main([("bitrev", p, 3) for p in range(8)], int)] == [0, 4, 2, 6, 1, 5, 3, 7]
    assert stft_main([("bitrev", 1, 12)], int) == [[2048]] and stft_main([("bitrev", 1, 1)], int) == [[1]]
    ffts = [2 << e for e in range(12)]
    cases = [(n_rx, n_p, wl, hop, n_fft, gate, flags) for n_fft in ffts for n_rx in (1, 4) for (n_p, wl, hop) in ((n_fft + 5, n_fft, 2), (7, 1, 3), (n_fft, n_fft, 9))
             for gate in (1, 7, 8, 9, 17, 4096) for flags in (0, 1, 3)]
    for (n_rx, n_p, wl, hop, n_fft, gate, flags), g in zip(cases, stft_main([("plan",) + c for c in cases], int)):
        logN, BT, passes, tiles, n_frames, lds, out_doubles, partial, supported = g
        assert 1 << logN == n_fft
        assert BT in (1, 2, 4, 8) and lds == n_fft * BT * 16 + n_fft * 8 and lds <= 160 * 1024          # the columns and the twiddle table fit
        assert BT == 8 or n_fft * (2 * BT) * 16 + n_fft * 8 > 160 * 1024                                  # ... and twice the columns would not
        assert n_fft * BT <= 32 * threads                                                                 # the kernel's elements per thread
        assert n_frames == 1 + (n_p - wl) // hop and supported == 1
        if flags & 2:
            assert passes * BT == 8 and tiles == -(-gate // 8)
            assert out_doubles == n_rx * n_frames * n_fft and partial == (out_doubles * tiles if tiles > 1 else 0)
        else:
            assert passes == 1 and tiles == -(-gate // BT) and partial == 0
            assert out_doubles == n_rx * n_frames * n_fft * gate * (1 if flags & 1 else 2)
    assert [stft_main([("plan", 1, n, n, 1, n, 8, 0)], int)[0][1] for n in (1024, 2048, 4096)] == [8, 4, 2]
    # the launch grid's limits: receivers, and frames x workgroups per frame
    assert stft_main([("plan", 65536, 8, 8, 1, 8, 8, 0)], int)[0][8] == 0
    assert stft_main([("plan", 65535, 8, 8, 1, 8, 8, 0)], int)[0][8] == 1
    n_p = 2 ** 31 // 4 + 1                                   # that many frames of one pulse, four workgroups each
    assert stft_main([("plan", 1, n_p, 1, 1, 2, 32, 0)], int)[0][8] == 0
    assert stft_main([("plan", 1, n_p - 2, 1, 1, 2, 32, 0)], int)[0][8] == 1
    assert stft_main([("plan", 1, n_p, 1, 1, 2, 16, 0)], int)[0][8] == 1                  # (two workgroups per frame)
