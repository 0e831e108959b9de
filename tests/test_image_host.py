"""Backprojection imaging on the host (no GPU): rts_backproject_eval against an independent numpy restatement of the definition in
include/rts_amd.h (RtsImageParams), known answers, linearity, the validation of malformed descriptors, the ISAR change of frame,
and rts_amd/csrc/rts_image.h alone under AddressSanitizer + UndefinedBehaviorSanitizer (tests/image/image_main.cpp).

The tolerance of the comparison with the restatement is derived, not measured.  The two sides may differ by a few roundings in tau
(two square roots, a sum, a division: at most ~8 roundings of 2^-53 relative), which the carrier multiplies into a phase error of
2 pi carrier tau 8 2^-53; every term is at most |w_j| H max|y| in magnitude, H the largest sum of |h_L| over the taps of one
sample.  So  atol = 64 2^-52 max(1, carrier tau_max) 2 pi B,  B = sum_j |w_j| H max|y|  (64: the ~8 roundings with a factor 8 to
spare; the interpolation weights' own rounding, ~1e-15 B, disappears in it).  With carrier tau_max near 1e4 that is below
1e-9 B, while a wrong index, sign or tap is an error of order B / P or more."""
import ctypes as C
import math
import os
import shutil
import subprocess

import numpy as np
import pytest

from test_waveform_host import h_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CS = 299792458.0
EPS = 2.0 ** -52


# ----------------------------------------------------------------------------- numpy restatement (from the header's text)
def interp_ref(row, d, taps):
    """the row interpolated at every d: taps == 1 the nearest sample, else sum_m row[m] h_L(d - m); 0 outside the row"""
    nb = len(row)
    if taps == 1:
        n = np.floor(d + 0.5).astype(np.int64)
        return np.where((n >= 0) & (n < nb), row[np.clip(n, 0, nb - 1)], 0.0)
    hl = taps // 2
    m = np.floor(d)[..., None].astype(np.int64) + np.arange(-hl - 1, hl + 2)
    ok = (m >= 0) & (m < nb)
    h = h_ref(d[..., None] - m, taps) * ok
    return (h * row[np.clip(m, 0, nb - 1)]).sum(axis=-1)


def pixels(g):
    ix = np.arange(g["n_x"], dtype=np.float64)[None, :, None]; iy = np.arange(g["n_y"], dtype=np.float64)[:, None, None]
    return np.asarray(g["origin"], np.float64) + ix * np.asarray(g["step_x"], np.float64) + iy * np.asarray(g["step_y"], np.float64)


def delays(g, r, j):
    x = pixels(g)
    return (np.linalg.norm(x - g["tx"][j], axis=-1) + np.linalg.norm(x - g["rx"][r][j], axis=-1)) / g["c"]


def backproject_ref(cube, g, taps, first, weights=None):
    n_rx = cube.shape[0]; P = len(g["tx"])
    w = np.ones(P) if weights is None else np.asarray(weights, np.float64)
    img = np.zeros((n_rx, g["n_y"], g["n_x"]), np.complex128)
    for r in range(n_rx):
        for j in range(P):
            tau = delays(g, r, j)
            v = interp_ref(cube[r, first + j], (tau - g["t0"]) / g["dt"], taps)
            img[r] += w[j] * v * np.exp(2j * np.pi * g["fc"] * tau)
    return img


def tap_sum_bound(taps):
    """H: the largest sum of |h_L(q - phi)| over the taps of one sample, on a fine grid of phi"""
    if taps == 1:
        return 1.0
    phi = np.linspace(0.0, 1.0, 2001)[:, None]
    q = np.arange(-taps // 2 - 1, taps // 2 + 2)[None, :]
    return float(np.abs(h_ref(q - phi, taps)).sum(axis=1).max())


def bound(g, taps, weights, ymax, factor=64.0):
    P = len(g["tx"])
    w = np.ones(P) if weights is None else np.abs(np.asarray(weights, np.float64))
    B = float(w.sum()) * tap_sum_bound(taps) * ymax
    tau_max = max(float(delays(g, r, j).max()) for r in range(len(g["rx"])) for j in range(P))
    return factor * EPS * max(1.0, g["fc"] * tau_max) * 2 * math.pi * B, B


def geometry(P, n_x=7, n_y=5, n_rx=2, nb=48, fc=1.5e9):
    """a side-looking track about 1 km from a 7 x 5 grid whose delays run from before bin 0 to beyond the last of nb bins;
    receiver 0 rides with the transmitter, receiver 1 is bistatic; carrier * tau is near 1e4"""
    j = np.arange(P, dtype=np.float64)
    tx = np.stack([np.full(P, -1000.0), -30.0 + 0.9 * j, np.full(P, 40.0)], axis=1)
    rx1 = np.stack([np.full(P, -990.0), 20.0 + 0.5 * j, np.full(P, 35.0)], axis=1)
    g = dict(n_x=n_x, n_y=n_y, origin=(-8.3, -2.0, 0.0), step_x=(2.6, 0.0, 0.0), step_y=(0.07, 1.0, 0.0), tx=tx, rx=np.stack([tx, rx1][:n_rx]), c=CS, fc=fc,
             dt=2.0e-9, t0=0.0)
    centre = dict(g, n_x=1, n_y=1, origin=(0.0, 0.0, 0.0))
    g["t0"] = float(delays(centre, 0, P // 2)[0, 0]) - (nb / 2) * g["dt"]
    return g


def call_eval(rts, cube, g, taps, first, weights=None, out=None):
    return rts.backproject_eval(cube, g["t0"], g["dt"], g["origin"], g["step_x"], g["step_y"], g["n_x"], g["n_y"], g["tx"], g["rx"], g["c"], g["fc"],
                                taps=taps, first=first, weights=weights, out=out)


def random_cube(seed, n_rx=2, rows=70, nb=48):
    rng = np.random.default_rng(seed)
    return rng.standard_normal((n_rx, rows, nb)) + 1j * rng.standard_normal((n_rx, rows, nb))


def hann(P):
    return 0.5 - 0.5 * np.cos(2 * np.pi * (np.arange(P) + 0.5) / P)


# ----------------------------------------------------------------------------- H1
@pytest.mark.parametrize("taps", [1, 2, 8])
@pytest.mark.parametrize("P", [1, 5, 65])
def test_eval_against_restatement(rts, P, taps):
    g = geometry(P)
    cube = random_cube(10 * P + taps)
    d = np.concatenate([((delays(g, r, j) - g["t0"]) / g["dt"]).ravel() for r in range(2) for j in range(P)])
    # the grid's delays leave the row on both sides and come within taps / 2 (of the 8-tap case) of either end
    assert d.min() < -1.0 and d.max() > 48.0 and np.any((d > -4.0) & (d < 4.0)) and np.any((d > 43.0) & (d < 51.0))
    assert 5e3 < g["fc"] * (d.max() * g["dt"] + g["t0"]) < 2e4
    for weights in (None, hann(P)):
        got = call_eval(rts, cube, g, taps, 3, weights)
        want = backproject_ref(cube, g, taps, 3, weights)
        atol, B = bound(g, taps, weights, float(np.abs(cube).max()))
        assert atol < 1e-9 * B
        err = float(np.abs(got - want).max())
        print("P %d taps %d weights %s: max error %.3g, bound %.3g, B %.3g, max |image| %.3g" % (P, taps, weights is not None, err, atol, B, np.abs(want).max()))
        assert np.abs(want).max() > 1e-3 * B / max(P, 1)
        assert err <= atol


# ----------------------------------------------------------------------------- H2
def arc_case(P=24, nb=48, n0=20, fc=1.5e9):
    """one scatterer at the origin, the radar on an arc of +-5 degrees of a circle of 1 km around it (receiver 0 with the transmitter,
    receiver 1 on the same circle 2 degrees on): every two-way delay is 2 R / c, on bin n0; pixel (1, 0) is the scatterer, pixels (0, 0)
    and (2, 0) lie one range cell (c dt / 2) nearer to and farther from the arc's middle"""
    R = 1000.0
    th = np.deg2rad(np.linspace(-5.0, 5.0, P))
    tx = np.stack([-R * np.cos(th), R * np.sin(th), np.zeros(P)], axis=1)
    th1 = th + np.deg2rad(2.0)
    rx1 = np.stack([-R * np.cos(th1), R * np.sin(th1), np.zeros(P)], axis=1)
    dt = 2.0e-9
    cell = CS * dt / 2
    g = dict(n_x=3, n_y=1, origin=(-cell, 0.0, 0.0), step_x=(cell, 0.0, 0.0), step_y=(0.0, 1.0, 0.0), tx=tx, rx=np.stack([tx, rx1]), c=CS, fc=fc, dt=dt,
             t0=2 * R / CS - n0 * dt)
    a = 0.75 - 0.5j
    cube = np.zeros((2, P, nb), np.complex128)
    s = np.zeros(3)
    for r in range(2):
        for j in range(P):
            tau = (np.linalg.norm(s - tx[j]) + np.linalg.norm(s - g["rx"][r][j])) / CS
            ph = -math.fmod(2 * math.pi * fc * tau, 2 * math.pi)
            cube[r, j, n0] = a * complex(math.cos(ph), math.sin(ph))
    return g, cube, a


@pytest.mark.parametrize("taps", [1, 8])
def test_known_answers(rts, taps):
    g, cube, a = arc_case()
    P = len(g["tx"])
    img = call_eval(rts, cube, g, taps, 0)
    atol, B = bound(g, taps, None, abs(a))
    for r in range(2):
        assert abs(img[r, 0, 1] - P * a) <= atol, (r, img[r, 0, 1], P * a)
        for ix in (0, 2):
            assert abs(img[r, 0, ix]) < 0.1 * abs(P * a)
            if taps == 1:
                assert img[r, 0, ix] == 0
    # carrier 0: the plain interpolated sum of the rows (no phase term at all)
    g0 = dict(g, fc=0.0)
    rng = np.random.default_rng(3)
    dense = rng.standard_normal(cube.shape) + 1j * rng.standard_normal(cube.shape)
    got = call_eval(rts, dense, g0, taps, 0)
    want = np.zeros_like(got)
    for r in range(2):
        for j in range(P):
            want[r] += interp_ref(dense[r, j], (delays(g0, r, j) - g0["t0"]) / g0["dt"], taps)
    atol0, _ = bound(g0, taps, None, float(np.abs(dense).max()))
    assert np.abs(got - want).max() <= atol0


# ----------------------------------------------------------------------------- H3
@pytest.mark.parametrize("taps", [1, 8])
def test_linearity(rts, taps):
    P = 65
    g = geometry(P)
    cube = random_cube(77, rows=P)
    w = hann(P)
    whole = call_eval(rts, cube, g, taps, 0, w)
    acc = None
    for lo, hi in ((0, 20), (20, 65)):
        part = dict(g, tx=g["tx"][lo:hi], rx=g["rx"][:, lo:hi])
        acc = call_eval(rts, cube, part, taps, lo, w[lo:hi], out=acc)
    _, B = bound(g, taps, w, float(np.abs(cube).max()))
    assert np.abs(acc - whole).max() <= 16 * EPS * B
    assert np.abs(whole).max() > 0
    assert np.array_equal(call_eval(rts, cube, g, taps, 0, 2 * w), 2 * whole)
    # accumulate adds to what the output holds
    base = np.full(whole.shape, 1.5 - 2j)
    np.testing.assert_allclose(call_eval(rts, cube, g, taps, 0, w, out=base), base + whole, rtol=0, atol=4 * EPS * (B + 3))


# ----------------------------------------------------------------------------- H4
def raw_case(L, n_rx=2, rows=6, nb=16, P=4):
    """a valid raw descriptor and its arrays: (q, cube, p, keep)"""
    q = L.RtsCubeParams(n_rx, rows, nb, 0, 1.0e-6, 2.0e-9)
    cube = np.ones((n_rx, rows, nb, 2))
    tx = np.zeros((P, 3)); tx[:, 0] = -150.0
    rx = np.zeros((n_rx, P, 3)); rx[:, :, 0] = -150.0
    w = np.ones(P)
    p = L.RtsImageParams()
    p.n_x, p.n_y, p.taps, p.flags, p.first_pulse, p.n_pulses = 3, 2, 8, 0, 1, P
    for k in range(3):
        p.origin[k], p.step_x[k], p.step_y[k] = 0.0, (0.3, 0.0, 0.0)[k], (0.0, 0.3, 0.0)[k]
    p.cspeed, p.carrier = CS, 1.0e9
    p.tx_position, p.rx_position, p.pulse_weight = tx.ctypes.data, rx.ctypes.data, w.ctypes.data
    return q, cube, p, dict(tx=tx, rx=rx, w=w)


def bad_image_params(L):
    """(name, mutate(p, keep), word the message must hold) for every refusal the header lists (bar the attached-cube test)"""
    def setter(**kw):
        def f(p, keep):
            for k, v in kw.items():
                setattr(p, k, v)
        return f

    def arr(field, index, value):
        def f(p, keep):
            getattr(p, field)[index] = value
        return f

    def poison(name, index, value):
        def f(p, keep):
            keep[name].reshape(-1)[index] = value
        return f

    def reserved(i):
        def f(p, keep):
            p.reserved[i] = 1
        return f

    return [
        ("n_x zero", setter(n_x=0), b"n_x"), ("n_y zero", setter(n_y=0), b"n_y"),
        ("too many pixels", setter(n_x=4097, n_y=4096), b"n_x"),
        ("taps 0", setter(taps=0), b"taps"), ("taps 3", setter(taps=3), b"taps"), ("taps 66", setter(taps=66), b"taps"),
        ("unknown flag", setter(flags=2), b"flags"),
        ("reserved 0", reserved(0), b"reserved"), ("reserved 1", reserved(1), b"reserved"),
        ("no pulses", setter(n_pulses=0), b"n_pulses"), ("pulses beyond the cube", setter(first_pulse=3), b"n_pulses"),
        ("first beyond the cube", setter(first_pulse=6), b"first_pulse"), ("wrapping pulse range", setter(first_pulse=0xffffffff), b"first_pulse"),
        ("cspeed 0", setter(cspeed=0.0), b"cspeed"), ("cspeed negative", setter(cspeed=-1.0), b"cspeed"), ("cspeed inf", setter(cspeed=math.inf), b"cspeed"),
        ("cspeed nan", setter(cspeed=math.nan), b"cspeed"),
        ("carrier negative", setter(carrier=-1.0), b"carrier"), ("carrier inf", setter(carrier=math.inf), b"carrier"), ("carrier nan", setter(carrier=math.nan), b"carrier"),
        ("origin nan", arr("origin", 1, math.nan), b"origin"), ("step_x inf", arr("step_x", 0, math.inf), b"step_x"), ("step_y nan", arr("step_y", 2, math.nan), b"step_y"),
        ("tx nan", poison("tx", 4, math.nan), b"tx_position"), ("rx inf", poison("rx", 17, -math.inf), b"rx_position"),
        ("weight nan", poison("w", 3, math.nan), b"pulse_weight"),
        ("null tx", setter(tx_position=None), b"tx_position"), ("null rx", setter(rx_position=None), b"rx_position"),
    ]


def test_malformed_descriptors_are_rejected(rts):
    from rts_amd import _lib as L
    lib = L.lib()
    out = np.full((2, 2, 3, 2), 7.25)
    q, cube, p, keep = raw_case(L)
    assert lib.rts_backproject_eval(C.byref(q), cube.ctypes.data, C.byref(p), out.ctypes.data) == L.RTS_OK
    assert not np.any(out == 7.25)
    p.pulse_weight = None
    assert lib.rts_backproject_eval(C.byref(q), cube.ctypes.data, C.byref(p), out.ctypes.data) == L.RTS_OK       # weights are optional
    for name, mutate, word in bad_image_params(L):
        q, cube, p, keep = raw_case(L)
        mutate(p, keep)
        out[:] = 7.25
        assert lib.rts_backproject_eval(C.byref(q), cube.ctypes.data, C.byref(p), out.ctypes.data) == L.RTS_ERR_INVALID, name
        assert word in lib.rts_last_error(), (name, lib.rts_last_error())
        assert np.all(out == 7.25), name
    q, cube, p, keep = raw_case(L)
    assert lib.rts_backproject_eval(C.byref(q), cube.ctypes.data, None, out.ctypes.data) == L.RTS_ERR_INVALID
    assert lib.rts_backproject_eval(None, cube.ctypes.data, C.byref(p), out.ctypes.data) == L.RTS_ERR_INVALID
    assert lib.rts_backproject_eval(C.byref(q), None, C.byref(p), out.ctypes.data) == L.RTS_ERR_INVALID
    assert lib.rts_backproject_eval(C.byref(q), cube.ctypes.data, C.byref(p), None) == L.RTS_ERR_INVALID
    # the limits themselves are accepted: 64 taps, the whole cube, carrier 0
    p.taps, p.first_pulse, p.n_pulses, p.carrier = 64, 2, 4, 0.0
    assert lib.rts_backproject_eval(C.byref(q), cube.ctypes.data, C.byref(p), out.ctypes.data) == L.RTS_OK
    with pytest.raises(ValueError):
        rts.backproject_eval(np.zeros((1, 2, 4)), 0.0, 1.0, (0, 0, 0), (1, 0, 0), (0, 1, 0), 2, 2, np.zeros((3, 3)), np.zeros((1, 2, 3)), CS, 0.0)


# ----------------------------------------------------------------------------- H5
def test_image_frame_keeps_distances(rts):
    """a target rotating about z and translating: a point fixed ON the target is as far from the radar in the target's frame (the
    point at rest, the radar moved by image_frame) as in the world frame (the point carried along), pulse by pulse"""
    P = 9
    rng = np.random.default_rng(8)
    body = np.array([3.0, -1.5, 0.7])
    radar = np.stack([np.array([-400.0, 20.0 * j, 60.0]) for j in range(P)])
    two = np.stack([radar, radar + rng.standard_normal((P, 3))])
    motions, world = [], []
    for j in range(P):
        a = 0.11 * j
        R = np.array([[math.cos(a), -math.sin(a), 0.0], [math.sin(a), math.cos(a), 0.0], [0.0, 0.0, 1.0]])
        pos = np.array([5.0 + 0.8 * j, -2.0 + 0.3 * j, 1.0])
        motions.append(dict(position=pos, rotation=R.ravel()))
        world.append(R @ body + pos)
    moved = rts.image_frame(two, motions)
    assert moved.shape == two.shape
    for k in range(2):
        for j in range(P):
            np.testing.assert_allclose(np.linalg.norm(moved[k, j] - body), np.linalg.norm(two[k, j] - world[j]), rtol=1e-13)
    assert not np.allclose(moved, two)
    # without a rotation: a plain shift; the ctypes record is taken too
    from rts_amd import _lib as L
    m = L.RtsTargetMotion(); m.position[:] = [1.0, 2.0, 3.0]; m.has_rotation = 0
    np.testing.assert_array_equal(rts.image_frame(np.array([[4.0, 4.0, 4.0]]), [m]), [[3.0, 2.0, 1.0]])
    np.testing.assert_array_equal(rts.image_frame(np.array([[4.0, 4.0, 4.0]]), [dict(position=(1.0, 2.0, 3.0))]), [[3.0, 2.0, 1.0]])


# ----------------------------------------------------------------------------- rts_image.h alone, under the sanitizers
@pytest.fixture(scope="module")
def image_main(tmp_path_factory):
    gxx = shutil.which("g++")
    if not gxx:
        pytest.skip("no g++")
    rt = subprocess.run([gxx, "-print-file-name=libasan.so"], capture_output=True, text=True).stdout.strip()
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"] if os.path.isabs(rt) and os.path.exists(rt) else []
    exe = str(tmp_path_factory.mktemp("image") / "image_main")
    subprocess.check_call([gxx, "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-ffp-contract=off"] + san + ["-I", os.path.join(ROOT, "rts_amd", "csrc"),
                           os.path.join(ROOT, "tests", "image", "image_main.cpp"), "-o", exe])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:verify_asan_link_order=0", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")

    def ask(cases, kind=float):
        text = "".join(" ".join(repr(x) if isinstance(x, float) else str(x) for x in c) + "\n" for c in cases)
        r = subprocess.run([exe], input=text, capture_output=True, text=True, env=env, timeout=120)
        assert r.returncode == 0, r.stderr[-3000:]
        out = [[kind(x) for x in line.split()] for line in r.stdout.splitlines()]
        assert len(out) == len(cases)
        return out
    return ask


def test_header_alone_reads_no_sample_outside_the_row(image_main):
    cases = []
    for taps in (1, 2, 8, 64):
        for nb in sorted({1, 2, max(taps - 1, 1), taps + 3, 100}):
            ds = [-float(taps), -0.5, 0.0, nb - 1.0, nb - 0.5, float(nb + taps), -0.25, 0.25, nb - 1.25, nb / 2 + 0.375, -taps / 2 + 0.01, nb + taps / 2 - 0.99,
                  math.inf, -math.inf, math.nan, 1e300, -1e300, 4294967296.5, -4294967296.5]
            cases += [("sample", nb, taps, float(d)) for d in ds]
    got = image_main(cases)
    for (_, nb, taps, d), (re, im) in zip(cases, got):
        row = (np.arange(nb) + 1.0) + 1j * (0.5 - np.arange(nb))
        want = complex(interp_ref(row, np.array([d]), taps)[0]) if math.isfinite(d) and abs(d) < 1e9 else 0.0
        assert abs(complex(re, im) - want) <= 1e-12 * tap_sum_bound(taps) * np.abs(row).max(), (nb, taps, d, re, im, want)
    # on a sample: the sample itself, bit for bit
    on = image_main([("sample", 9, taps, float(n)) for taps in (2, 8, 64) for n in range(9)])
    assert [tuple(x) for x in on] == [(n + 1.0, 0.5 - n) for taps in (2, 8, 64) for n in range(9)]


def test_launch_plan(image_main):
    assert image_main([("consts",)], int) == [[256, 64, 16777216, 65535]]
    shapes = [(1, 1), (17, 3), (16, 16), (33, 1), (1, 33), (15, 300), (300, 15), (512, 512), (128, 128), (4096, 4096), (1, 16777216), (16777216, 1), (3, 5)]
    cases = [(nx, ny, n_rx, P, below) for nx, ny in shapes for n_rx in (1, 4) for P in (1, 64, 65, 1024) for below in (0, 1024, 65536)]
    for (nx, ny, n_rx, P, below), g in zip(cases, image_main([("plan",) + c for c in cases], int)):
        twl, thl, tiles_x, tiles_y, n_chunks, split, supported, scratch = g
        assert twl + thl == 8                                                          # 256 pixels per tile
        assert tiles_x == -(-nx // (1 << twl)) and tiles_y == -(-ny // (1 << thl))      # the tiles cover the image, none is empty
        assert (1 << twl) < 2 * max(nx, 1) or twl == 0 or nx >= 16      # a narrow image's tile is no wider than its next power of two
        if nx >= 16 and ny >= 16:
            assert (twl, thl) == (4, 4)
        assert n_chunks == -(-P // 64) and supported == 1
        assert split == (1 if n_chunks > 1 and tiles_x * tiles_y * n_rx < below else 0)
        assert scratch == (n_chunks * n_rx * nx * ny if split else 0)
    # the launch grid's limits
    assert image_main([("plan", 4, 4, 65536, 1, 0)], int)[0][6] == 0
    assert image_main([("plan", 4, 4, 1, 64 * 65535 + 1, 0)], int)[0][6] == 0
    assert image_main([("plan", 4, 4, 65535, 64 * 65535, 0)], int)[0][6] == 1
