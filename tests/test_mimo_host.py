"""The MIMO matched-filter bank without a GPU (include/rts_amd.h: RtsBankParams): rts_bank_eval against the restated tree of
tests/mimo_ref.py bit for bit over the edge shapes the GPU tests share; its accuracy against a longdouble correlation; one waveform
and no code against tests/cube_ref.py's statement of the compression; linearity in the slow-time code on a cube rendered as two
transmitters; every refusal; the ABI sizes; Waveform.coded and virtual_positions; and rts_amd/csrc/rts_mimo.h alone under
AddressSanitizer + UndefinedBehaviorSanitizer (tests/mimo/mimo_main.cpp) with the plan at its edges."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import cube_ref as CR
import mimo_ref as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
same = M.same
CASES = M.cases()


def waves_of(rts, samples, taps=1):
    return [rts.Waveform(s, taps) for s in samples]


# ----------------------------------------------------------------------------- 1. bit identity
@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_bank_against_restatement(rts, case):
    name, n_rx, n_p, N, lengths, code, first, count = case
    cube, waves, table = M.case_input(*case)
    got = rts.bank_eval(cube, waves_of(rts, waves), table, first, count)
    want = M.bank_restated(cube, waves, table, first, count)
    assert got.shape == want.shape == (len(lengths) * n_rx, (n_p - first if count is None else count), N)
    assert not np.isnan(bits_of(got)).any()                          # the rows outside the span (NaN) were never read
    assert same(got, want)


def bits_of(a):
    return M.bits(a)


def test_a_zero_code_entry_gives_zeros_by_the_multiply(rts):
    """conj(0) z is (0 zr + 0 zi, 0 zi - 0 zr): zeros whose signs the multiply decides; a skip would leave +0.0 everywhere, and a
    non-finite z shows the difference outright: 0 * inf is NaN"""
    cube = np.ones((1, 2, 4), np.complex128); cube[0, 1, 2] = np.inf
    got = rts.bank_eval(cube, waves_of(rts, [np.array([1.0 + 0j])]), np.zeros((1, 2), np.complex128))
    assert not got[0, 0].any() and np.isnan(got[0, 1, 2]) and not got[0, 1, [0, 1, 3]].any()
    minus = np.full((1, 1, 2), -1.0 - 1.0j)
    neg = rts.bank_eval(minus, waves_of(rts, [np.array([1.0 + 0j])]), np.zeros((1, 1), np.complex128))
    assert same(neg, M.bank_restated(minus, [np.array([1.0 + 0j])], np.zeros((1, 1), np.complex128)))
    assert np.signbit(neg.real).all()                                # 0 * -1 + 0 * -1 = -0.0: formed, not skipped


# ----------------------------------------------------------------------------- 2. accuracy
@pytest.mark.parametrize("n_rx,n_p,N,lengths", [(2, 2, 300, [1, 7, 300]), (1, 1, 700, [512, 513]), (1, 1, 300, [4096]), (4, 3, 64, [16, 16])])
def test_accuracy_against_longdouble(rts, n_rx, n_p, N, lengths):
    """per component |z - longdouble z| <= M eps sum_m |y[n + m]| |s[m]|: each term's two products and one sum cost at most
    2 u (|yr sr| + |yi si|) <= 2 u |y| |s| (u = eps / 2), the M sums of the chain at most (M - m) u each on what is below them --
    (M + 1) u in all, under M eps.  The measured share of the bound is printed, not fixed."""
    rng = np.random.default_rng(N + len(lengths))
    cube = M.random_complex(rng, (n_rx, n_p, N))
    waves = [M.random_complex(rng, m) for m in lengths]
    got = rts.bank_eval(cube, waves_of(rts, waves))
    ref = M.bank_longdouble(cube, waves)
    mag = M.term_magnitudes(cube, waves)
    err = got.astype(CR.CLD) - ref
    share = 0.0
    for t, m in enumerate(lengths):
        sl = slice(t * n_rx, (t + 1) * n_rx)
        bound = min(m, N) * M.EPS * mag[sl]
        assert np.all(np.abs(err[sl].real) <= bound) and np.all(np.abs(err[sl].imag) <= bound)
        share = max(share, float(np.max(np.maximum(np.abs(err[sl].real), np.abs(err[sl].imag)) / bound)))
    print("bank accuracy: lengths %s, %d bins: the largest error is %.4f of M eps sum |y||s|" % (lengths, N, share))


# ----------------------------------------------------------------------------- 3. against the compression
def test_one_waveform_no_code_is_the_compression(rts):
    """tests/cube_ref.py states the compression in longdouble.  On small dyadic inputs every product and every sum of either
    statement is exact, so the two agree BIT FOR BIT (the order of the sum is then the only thing that could differ, and it cannot
    show); on random inputs they agree within the bound of the accuracy test"""
    rng = np.random.default_rng(9)
    for N, m in ((1, 1), (40, 7), (40, 40), (40, 45), (600, 513)):
        y = (rng.integers(-8, 9, (2, 3, N)) + 1j * rng.integers(-8, 9, (2, 3, N))) / 4.0
        s = (rng.integers(-8, 9, m) + 1j * rng.integers(-8, 9, m)) / 8.0
        got = rts.bank_eval(y, waves_of(rts, [s]))
        want = np.array([[CR.to_double(CR.correlate_ref(y[r, p], s)) for p in range(3)] for r in range(2)])
        assert same(got + 0.0, want + 0.0)                           # (+ 0.0: the sign of an exact zero is not the statement's subject)
        assert np.array_equal(got, want)
    y = M.random_complex(rng, (1, 1, 200)); s = M.random_complex(rng, 33)
    got = rts.bank_eval(y, waves_of(rts, [s]))[0, 0]
    ref = CR.correlate_ref(y[0, 0], s)
    bound = 33 * M.EPS * M.term_magnitudes(y, [s])[0, 0]
    assert np.all(np.abs((got.astype(CR.CLD) - ref).real) <= bound) and np.all(np.abs((got.astype(CR.CLD) - ref).imag) <= bound)


# ----------------------------------------------------------------------------- 4. linearity in the code
def test_two_coded_transmitters_come_apart(rts):
    """a cube 'rendered' as two transmitters: transmitter t's on-grid echo at bin n0 of row p is code[t][p] a_t s_t.  The waveforms are
    rows of a Hadamard matrix: orthogonal at zero lag.  At n0 the bank returns each transmitter's own compression (the bank of the
    cube that holds that transmitter alone) plus the other's leak, which is conj(c_t) c_u a_u <s_u, s_t> with the inner product
    computed here by numpy -- exactly 0 for these rows, so the two agree within the rounding of the sum alone"""
    n_rx, n_p, N, n0, m = 3, 4, 48, 11, 16
    h = np.array([[1.0]])
    while h.shape[0] < m:
        h = np.block([[h, h], [h, -h]])
    s = [h[5] * 1j, -h[10]]                                           # (exact phases: the inner product below is exactly 0)
    assert abs(np.vdot(s[0], s[1])) == 0.0
    rng = np.random.default_rng(4)
    amp = M.random_complex(rng, (2, n_rx))
    code = np.exp(2j * np.pi * np.outer([0, 1], np.arange(n_p)) / n_p) * np.exp(0.7j)      # DDMA: a ramp per transmitter
    alone = []
    for t in range(2):
        c = np.zeros((n_rx, n_p, N), np.complex128)
        c[:, :, n0:n0 + m] = amp[t][:, None, None] * code[t][None, :, None] * s[t][None, None, :]
        alone.append(c)
    both = rts.bank_eval(alone[0] + alone[1], waves_of(rts, s), code)
    for t in range(2):
        u = 1 - t
        own = rts.bank_eval(alone[t], waves_of(rts, [s[t]]), code[t:t + 1])[:, :, n0]
        cross = np.conj(code[t])[None, :] * code[u][None, :] * amp[u][:, None] * np.vdot(s[t], s[u])      # sum_m s_u[m] conj(s_t[m])
        got = both[t * n_rx:(t + 1) * n_rx, :, n0]
        scale = m * (np.abs(amp[0]) + np.abs(amp[1]))[:, None]                                            # sum_m |y[n0 + m]| |s_t[m]| at most
        assert np.all(np.abs(got - (own + cross)) <= 4 * m * M.EPS * scale)
        energy = amp[t][:, None] * m * np.abs(code[t][None, :]) ** 2
        assert np.all(np.abs(got - energy) <= 8 * m * M.EPS * scale)                                     # and that compression is a_t sum |s_t|^2
    # a waveform pair that is NOT orthogonal leaks by its inner product
    s2 = [s[0], s[0] * 0.5 + s[1]]
    x = np.vdot(s2[0], s2[1])
    c = np.zeros((1, 1, N), np.complex128); c[0, 0, n0:n0 + m] = s2[1]
    leak = rts.bank_eval(c, waves_of(rts, s2))[0, 0, n0]
    assert abs(leak - x) <= 4 * m * M.EPS * m and abs(x) == pytest.approx(0.5 * m)


# ----------------------------------------------------------------------------- 5. refusals
def raw_bank(rts, q, cube, p, out):
    L = rts.L
    rc = L.lib().rts_bank_eval(C.byref(q) if q is not None else None, cube.ctypes.data_as(C.c_void_p) if cube is not None else None, C.byref(p) if p is not None else None,
                               out.ctypes.data_as(C.c_void_p) if out is not None else None)
    return rc, L.lib().rts_last_error().decode()


def _wave(rts, samples=None, n=None, taps=1, reserved=0, null=False):
    s = np.ascontiguousarray(np.ones((4, 2)) if samples is None else samples)
    w = rts.L.RtsWaveform()
    w.samples = None if null else s.ctypes.data_as(C.c_void_p)
    w.n_samples, w.taps = (len(s) if n is None else n), taps
    w.reserved[1] = reserved
    return w, s


def _par(rts, waves, n_waves=None, first=0, n=4, code=None, reserved=0, null_waves=False):
    L = rts.L
    arr = (L.RtsWaveform * max(len(waves), 1))(*[w for w, _ in waves])
    p = L.RtsBankParams()
    p.n_waves, p.first_pulse, p.n_pulses = (len(waves) if n_waves is None else n_waves), first, n
    if not null_waves:
        p.waves = arr
    if code is not None:
        p.code = code.ctypes.data_as(C.c_void_p)
    p.reserved[0] = reserved
    return p, (arr, waves, code)


def _bad_samples(v):
    s = np.ones((4, 2)); s[2, 1] = v
    return s


REFUSALS = [
    ("reserved", lambda r: _par(r, [_wave(r)], reserved=1), "reserved"),
    ("no_waves", lambda r: _par(r, [_wave(r)], n_waves=0), "n_waves"),
    ("too_many_waves", lambda r: _par(r, [_wave(r)] * 17), "n_waves"),
    ("null_waves", lambda r: _par(r, [_wave(r)], null_waves=True), "null waves"),
    ("wave_reserved", lambda r: _par(r, [_wave(r), _wave(r, reserved=1)]), "waves[1]: reserved"),
    ("wave_no_samples", lambda r: _par(r, [_wave(r, n=0)]), "waves[0]: 0 samples"),
    ("wave_too_long", lambda r: _par(r, [_wave(r, np.ones((M.MAX_SAMPLES + 1, 2)))]), "samples (1 .. %d)" % M.MAX_SAMPLES),
    ("wave_odd_taps", lambda r: _par(r, [_wave(r, taps=3)]), "taps"),
    ("wave_null_samples", lambda r: _par(r, [_wave(r, null=True)]), "null sample array"),
    ("wave_nan_sample", lambda r: _par(r, [_wave(r), _wave(r), _wave(r, _bad_samples(np.nan))]), "waves[2]: sample 2 is not finite"),
    ("wave_inf_sample", lambda r: _par(r, [_wave(r, _bad_samples(-np.inf))]), "not finite"),
    ("span_empty", lambda r: _par(r, [_wave(r)], n=0), "pulse"),
    ("span_starts_outside", lambda r: _par(r, [_wave(r)], first=4, n=1), "pulse"),
    ("span_ends_outside", lambda r: _par(r, [_wave(r)], first=2, n=3), "pulse"),
    ("span_wraps", lambda r: _par(r, [_wave(r)], first=0xffffffff, n=2), "pulse"),
    ("code_nan", lambda r: _par(r, [_wave(r), _wave(r)], code=np.array([[1, 1, 1, 1], [1, 1, np.nan, 1]], np.complex128)), "code[1][2]"),
    ("code_inf", lambda r: _par(r, [_wave(r)], code=np.array([[1, 1, 1, 1j * np.inf]], np.complex128)), "code[0][3]"),
]


@pytest.mark.parametrize("name,make,word", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_refusal(rts, name, make, word):
    L = rts.L
    cube = np.ones((3, 4, 8), np.complex128); out = np.full((3 * 17, 4, 8), 7.0 + 0j)
    q = L.RtsCubeParams(3, 4, 8, 0, 0.0, 1.0)
    p, keep = make(rts)
    rc, msg = raw_bank(rts, q, cube, p, out)
    assert rc == L.RTS_ERR_INVALID and word in msg and msg.startswith("rts_bank_eval"), msg
    assert np.all(out == 7.0)                                         # a refused call leaves out untouched
    del keep


@pytest.mark.parametrize("shape,ok", [((1 << 20, 1 << 10, 1 << 10), False), ((0xffffffff, 0xffffffff, 0xffffffff), False), ((1 << 19, 1 << 10, 1 << 10), True)])
def test_the_outputs_size_is_formed_without_overflow(rts, shape, ok):
    """2^39 cells are the most: 2^20 x 2^10 x 2^10 with one waveform is one factor of two beyond, 2^32 - 1 in every dimension would
    wrap a 64-bit product.  (Refused before anything is read: the arrays are one cell; the last shape is accepted by the rule and
    turned away only for its null output.)"""
    L = rts.L
    q = L.RtsCubeParams(shape[0], shape[1], shape[2], 0, 0.0, 1.0)
    p, keep = _par(rts, [_wave(rts)], n=shape[1])
    rc, msg = raw_bank(rts, q, np.ones(1, np.complex128), p, None)
    assert rc == L.RTS_ERR_INVALID and (("RTS_BANK_MAX_CELLS" in msg) != ok) and (("null cube or output" in msg) == ok), msg


def test_null_arguments_and_a_good_call(rts):
    L = rts.L
    cube = np.ones((3, 4, 8), np.complex128); out = np.full((3, 4, 8), 7.0 + 0j)
    q = L.RtsCubeParams(3, 4, 8, 0, 0.0, 1.0)
    p, keep = _par(rts, [_wave(rts)])
    for args in ((q, cube, None, out), (q, None, p, out), (q, cube, p, None), (None, cube, p, out)):
        assert raw_bank(rts, *args)[0] == L.RTS_ERR_INVALID
    assert np.all(out == 7.0)
    assert raw_bank(rts, q, cube, p, out)[0] == L.RTS_OK and out[0, 0, 0] == 4.0 - 4.0j and out[2, 3, 7] == 1.0 - 1.0j      # (1 + 0j) conj(1 + 1j), four terms / one


def test_abi_sizes(rts):
    L = rts.L
    assert C.sizeof(L.RtsBankParams) == 48
    assert "sizeof(RtsBankParams) == 48" in open(os.path.join(ROOT, "rts_amd", "csrc", "rts_internal.h")).read()
    assert "} RtsBankParams;                                              /* 48 bytes */" in open(os.path.join(ROOT, "include", "rts_amd.h")).read()
    assert (L.RTS_BANK_MAX_WAVES, L.RTS_BANK_TILE) == (M.MAX_WAVES, M.TILE) and L.RTS_BANK_MAX_CELLS == 549755813888


# ----------------------------------------------------------------------------- 6. the Python helpers
def test_coded_waveform_and_virtual_positions(rts):
    w = rts.Waveform.coded([1, -1, 1j], samples_per_chip=3, taps=2)
    assert np.array_equal(w.samples, np.array([1, 1, 1, -1, -1, -1, 1j, 1j, 1j])) and w.taps == 2 and w.desc().n_samples == 9
    assert np.array_equal(rts.Waveform.coded([1, -1]).samples, np.array([1, -1], np.complex128))
    with pytest.raises(ValueError):
        rts.Waveform.coded([1], 0)
    tx = np.array([[0, 0, 0], [4.0, 0, 0]]); rx = np.array([[0, 0, 0], [1.0, 0, 0], [2.0, 0.5, 0]])
    v = rts.virtual_positions(tx, rx)
    assert v.shape == (6, 3) and np.array_equal(v[:3], rx) and np.array_equal(v[3:], rx + tx[1])
    with pytest.raises(ValueError):
        rts.bank_eval(np.ones((1, 2, 3)), [rts.Waveform([1.0])], code=np.ones((1, 3)))


# ----------------------------------------------------------------------------- 7. rts_mimo.h alone, under the sanitizers
@pytest.fixture(scope="module")
def mimo_main(tmp_path_factory):
    gxx = shutil.which("g++")
    if not gxx:
        pytest.skip("no g++")
    rt = subprocess.run([gxx, "-print-file-name=libasan.so"], capture_output=True, text=True).stdout.strip()
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"] if os.path.isabs(rt) and os.path.exists(rt) else []
    exe = str(tmp_path_factory.mktemp("mimo") / "mimo_main")
    subprocess.check_call([gxx, "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-ffp-contract=off"] + san + ["-I", os.path.join(ROOT, "rts_amd", "csrc"),
                           os.path.join(ROOT, "tests", "mimo", "mimo_main.cpp"), "-o", exe])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:verify_asan_link_order=0", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")

    def ask(lines):
        r = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True, env=env, timeout=120)
        assert r.returncode == 0, r.stderr[-3000:]
        out = r.stdout.splitlines()
        assert len(out) == len(lines)
        return [line.split() for line in out]
    return ask


def plan_line(n_rx, n_rows, N, lengths, code):
    return "plan %d %d %d %d %d %s" % (n_rx, n_rows, N, len(lengths), 1 if code else 0, " ".join(str(m) for m in lengths))


def test_plan_at_its_edges(mimo_main):
    """plan n_rx n_rows n_bins n_waves code M... -> tiles group groups max_M Q S blocks lds out_doubles tab_doubles code_off off[last] supported"""
    T = M.TILE
    ask = [(plan_line(4, 256, 4096, [256] * 8, False), [8, 4, 2, 256, 64, 196, 8 * 256 * 4 * 2, 16 * 4 * 196, 2 * 32 * 256 * 4096, 2 * 8 * 256, 2 * 8 * 256, 2 * 7 * 256, 1]),
           (plan_line(4, 16, 512, [1024] * 2, True), [1, 1, 2, 1024, 256, 388, 128, 16 * 4 * 388, 2 * 8 * 16 * 512, 4096 + 2 * 2 * 16, 4096, 2048, 1]),
           (plan_line(1, 1, 1, [1], False), [1, 1, 1, 1, 1, 148, 1, 16 * 4 * 148, 2, 2, 2, 0, 1]),
           (plan_line(1, 1, 300, [4096], False), [1, 1, 1, 4096, 1024, 1156, 1, 73984, 600, 8192, 8192, 0, 1]),
           (plan_line(1, 1, T + 1, [1, 7, 300], True), [2, 1, 3, 300, 75, 212, 6, 16 * 4 * 212, 2 * 3 * (T + 1), 2 * 308 + 6, 616, 16, 1]),
           (plan_line(1 << 20, 1 << 10, 1 << 10, [1], False), None), (plan_line(1 << 19, 1 << 10, 1 << 10, [1], False), "ok"),
           (plan_line(1, 1 << 30, 1, [1] * 16, False), None), (plan_line(1, 1 << 30, 1, [1], False), "ok"), (plan_line(0xffffffff, 0xffffffff, 0xffffffff, [1] * 16, True), None)]
    got = mimo_main([a for a, _ in ask])
    for (line, want), g in zip(ask, got):
        if want is None:
            assert g[-1] == "0", line
        elif want == "ok":
            assert g[-1] == "1", line
        else:
            assert [int(v) for v in g] == want, (line, g)
    # the group a thread holds in the cases the GPU tests run for it
    for name, group in M.GROUPS.items():
        _, n_rx, n_p, N, lengths, code, first, count = [c for c in CASES if c[0] == name][0]
        (g,) = mimo_main([plan_line(n_rx, n_p - first if count is None else count, N, lengths, code)])
        assert int(g[1]) == group, (name, g)


RULES = [("rule 4 2 0 4 0 0", 0), ("rule 4 2 0 4 1 0", 1), ("rule 4 0 0 4 0 0", 2), ("rule 4 17 0 4 0 0", 2), ("rule 4 16 0 4 0 0", 0), ("rule 4 2 0 4 0 1", 3),
         ("rule 4 2 0 0 0 0", 4), ("rule 4 2 4 1 0 0", 4), ("rule 4 2 3 2 0 0", 4), ("rule 4 2 3 1 0 0", 0), ("rule 4 2 4294967295 2 0 0", 4)]


def test_numbered_rules(mimo_main):
    """rule n_pulses n_waves first n reserved null_waves"""
    got = mimo_main([a for a, _ in RULES])
    assert [int(g[0]) for g in got] == [w for _, w in RULES]


def main_input(n_rx, n_p, N):
    """the driver's input: small dyadic values, so that it needs no file"""
    r, p, b = np.meshgrid(np.arange(n_rx), np.arange(n_p), np.arange(N), indexing="ij")
    return ((r * 131 + p * 17 + b * 7) % 23 - 11.0) / 8.0 + 0.25 * p + 1j * (((r * 5 + p * 3 + b * 11) % 19 - 9.0) / 16.0 - 0.03125 * b)


def main_wave(t, m):
    k = np.arange(m)
    return ((t * 37 + k * 13) % 17 - 8.0) / 4.0 + 1j * (((t * 11 + k * 5) % 13 - 6.0) / 8.0)


def main_code(nw, count):
    t, p = np.meshgrid(np.arange(nw), np.arange(count), indexing="ij")
    return ((t * 3 + p * 7) % 5 - 2.0) / 2.0 + 1j * (((t * 5 + p * 2) % 7 - 3.0) / 4.0)


MAIN_BANK = [(1, 1, 1, 0, 1, [1], False), (2, 3, 40, 0, 3, [7, 45], True), (3, 5, 30, 1, 2, [1, 30, 31], True), (2, 4, 9, 3, 1, [4] * 16, False), (1, 2, 600, 1, 1, [513], True)]


def test_header_alone_reads_and_writes_only_what_it_is_given(rts, mimo_main):
    """cube, waveforms, code table and output are heap arrays of exactly their sizes in the driver and the rows outside the span are
    poisoned; the results equal the library's bit for bit"""
    lines = ["bank %d %d %d %d %d %d %d %s" % (n_rx, n_p, N, first, count, len(lengths), 1 if code else 0, " ".join(str(m) for m in lengths))
             for n_rx, n_p, N, first, count, lengths, code in MAIN_BANK]
    for (n_rx, n_p, N, first, count, lengths, code), g in zip(MAIN_BANK, mimo_main(lines)):
        waves = [main_wave(t, m) for t, m in enumerate(lengths)]
        want = rts.bank_eval(main_input(n_rx, n_p, N), waves_of(rts, waves), main_code(len(lengths), count) if code else None, first, count)
        assert same(np.array([float.fromhex(v) for v in g]), want.reshape(-1))
