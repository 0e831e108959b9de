"""Receive-array beamforming on the host (no GPU): rts_beamform_eval against a plain-Python restatement of the tree in
include/rts_amd.h (RtsBeamParams; tests/beam_ref.py) bit for bit and against numpy.einsum within the project's bound, known answers,
the streaming peak (ties, edges, a known vertex, the detection records' refinement bit for bit), rts_steering_make on plane waves,
every refusal the header lists for the two host calls, rts_amd/csrc/rts_beam.h alone under AddressSanitizer +
UndefinedBehaviorSanitizer (tests/beam/beam_main.cpp) with the plan's values at its edges, and the host run of the whole chain that
fixed the scenario tests/test_gpu_beam.py repeats on the device.

"Bit for bit" is meant literally: the tree holds IEEE basic operations only, the library is built with -ffp-contract=off and Python
floats never contract.  The einsum bound is the project's for a kernel against its evaluator, rtol 1e-10 and atol 1e-12 max|ref|:
einsum associates and may fuse differently, a few ulp of a sum of at most eight terms of order one."""
import ctypes as C
import math
import os
import shutil
import subprocess

import numpy as np
import pytest

import beam_ref as B

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def bits(a):
    return np.ascontiguousarray(a).view(np.float64)


# ----------------------------------------------------------------------------- 1. against the restatement
@pytest.mark.parametrize("n_bins", [1, 7])
@pytest.mark.parametrize("n_beams", [1, 2, 5])
@pytest.mark.parametrize("n_rx", [1, 2, 3, 8])
def test_eval_against_restatement(rts, n_rx, n_beams, n_bins):
    rng = np.random.default_rng(1000 * n_rx + 10 * n_beams + n_bins)
    inp = B.random_complex(rng, (n_rx, 3, n_bins)); inp[:, 0] = np.nan                 # row 0 is outside the span: never read
    w = B.random_complex(rng, (n_beams, n_rx))
    ref = B.beam_restated(inp, w, 1, 2)
    got = rts.beamform_eval(inp, w, first=1, count=2)
    assert got.shape == (n_beams, 2, n_bins) and np.all(np.isfinite(bits(got)))
    assert np.array_equal(bits(got), bits(ref))
    assert np.array_equal(bits(rts.beamform_eval(inp, w, first=1)), bits(ref))          # count None: to the last row
    es = np.einsum("br,rjn->bjn", np.conj(w), inp[:, 1:3])
    np.testing.assert_allclose(got, es, rtol=1e-10, atol=1e-12 * np.abs(es).max())
    power = rts.beamform_eval(inp, w, first=1, count=2, power=True)
    assert power.dtype == np.float64 and np.array_equal(power, B.power_restated(ref))
    peak = rts.beamform_eval(inp, w, first=1, count=2, peak=True)
    want = B.peak_restated(B.power_restated(ref))
    assert peak.shape == (2, n_bins, 2) and np.array_equal(peak[..., 0], want[..., 0])
    assert np.array_equal(np.rint(peak[..., 1]), np.rint(want[..., 1]))
    np.testing.assert_allclose(peak[..., 1], want[..., 1], rtol=1e-12, atol=0)


# ----------------------------------------------------------------------------- 2. known answers
def test_known_answers(rts):
    rng = np.random.default_rng(7)
    z = B.random_complex(rng, (1, 2, 9))
    assert np.array_equal(bits(rts.beamform_eval(z, [[1.0]])), bits(z))                  # w = 1: the input
    got = rts.beamform_eval(z, [[1j]])                                                    # w = j: conj(j) z = (zi, -zr)
    assert np.array_equal(got.real, z.imag) and np.array_equal(got.imag, -z.real)
    inp = B.random_complex(rng, (4, 3, 11)); w = B.random_complex(rng, (6, 4))
    y = rts.beamform_eval(inp, w)
    p = rts.beamform_eval(inp, w, power=True)
    assert np.array_equal(p, B.power_restated(y))                                        # POWER: re re + im im of the complex output
    assert np.array_equal(p, y.real * y.real + y.imag * y.imag)
    both = rts.beamform_eval(inp, np.concatenate([w, w]))                                 # beams do not see each other
    assert np.array_equal(bits(both[:6]), bits(y)) and np.array_equal(bits(both[6:]), bits(y))


# ----------------------------------------------------------------------------- 3. the peak
def peak_of_amplitudes(rts, amps):
    """one receiver, z = 1, real weights a_b: the beam powers are a_b a_b exactly"""
    out = rts.beamform_eval(np.ones((1, 1, 1)), np.array(amps, np.float64).reshape(-1, 1), peak=True)
    return float(out[0, 0, 0]), float(out[0, 0, 1])


def test_peak_ties_and_edges(rts):
    # the LOWEST beam of a plateau: beam 1, which its equal right neighbour pulls to + 1/2 exactly (0.5 (0 - ln 4) / (-ln 4))
    assert peak_of_amplitudes(rts, [1.0, 2.0, 2.0, 1.0]) == (4.0, 1.5)
    assert peak_of_amplitudes(rts, [1.0, 2.0, 2.0, 2.0, 0.5]) == (4.0, 1.5)
    assert peak_of_amplitudes(rts, [2.0, 1.0, 2.0, 1.0, 2.0]) == (4.0, 0.0)
    assert peak_of_amplitudes(rts, [3.0, 3.0, 3.0]) == (9.0, 0.0)                        # all equal: the first beam, no offset at the edge
    assert peak_of_amplitudes(rts, [3.0, 2.0, 1.0]) == (9.0, 0.0)                        # the first beam
    assert peak_of_amplitudes(rts, [1.0, 2.0, 3.0]) == (9.0, 2.0)                        # the last beam: the axis does not wrap
    assert peak_of_amplitudes(rts, [5.0]) == (25.0, 0.0)                                 # one beam is both
    assert peak_of_amplitudes(rts, [1.0, 5.0]) == (25.0, 1.0)
    assert peak_of_amplitudes(rts, [0.0, 0.0, 0.0]) == (0.0, 0.0)
    assert peak_of_amplitudes(rts, [1.0, 3.0, 0.0, 2.0]) == (9.0, 1.0)                   # a zero neighbour: no refinement


def test_peak_gaussian_vertex(rts):
    """ln P a parabola through three beams: the log-parabola returns its vertex"""
    for v, s in ((1.3, 1.0), (0.75, 0.8), (1.0, 2.0), (1.49, 1.5)):
        amps = [math.sqrt(math.exp(-(b - v) ** 2 / (2 * s * s))) for b in range(3)]
        P, c = peak_of_amplitudes(rts, amps)
        print("vertex %.2f: coordinate %.17g, error %.3g" % (v, c, c - v))
        assert abs(c - v) <= 1e-12 and abs(P - max(a * a for a in amps)) == 0.0


def test_peak_coordinate_is_the_detection_records_refinement(rts):
    """coordinate = b* + rts_cfar_delta(P[b* - 1], P[b*], P[b* + 1]) evaluated by rts_cfar_os_eval (its range_offset on a map whose range
    axis carries the beams of one cell), bit for bit; P* is that record's power bit for bit"""
    rng = np.random.default_rng(33)
    inp = B.random_complex(rng, (3, 2, 5)); w = B.random_complex(rng, (7, 3))
    y = rts.beamform_eval(inp, w)
    peak = rts.beamform_eval(inp, w, peak=True)
    interior = 0
    for j in range(2):
        for n in range(5):
            det = rts.cfar_os_eval(y[:, j, n].reshape(1, 1, 7), (0, 0), (1, 0), 1, alpha=1e-300, local_max=False)
            assert len(det) == 7
            b = int(np.argmax(det["power"]))
            want = float(b) + (float(det["range_offset"][b]) if 0 < b < 6 else 0.0)
            assert peak[j, n, 0] == det["power"][b] and peak[j, n, 1] == want, (j, n, peak[j, n], det[b])
            interior += 0 < b < 6 and det["range_offset"][b] != 0.0
    assert interior >= 3


# ----------------------------------------------------------------------------- 4. steering
@pytest.mark.parametrize("array", ["line", "planar"])
def test_steering_on_a_plane_wave(rts, array):
    wl = 0.03; fc = B.C0 / wl
    pos = B.line_array(8, wl) if array == "line" else B.planar_array(wl)
    el0 = 0.0 if array == "line" else 0.35
    fan = np.linspace(-math.pi / 3, math.pi / 3, 17)
    k0 = 12                                                                              # the beam at u0; its mirror image is beam 4
    amp = 0.7 - 0.4j
    z = B.snapshot(pos, float(fan[k0]), el0, fc, amp)
    directions = np.stack([fan, np.full(17, el0)], axis=1)
    w = rts.steering(pos, directions, wl)
    assert w.shape == (17, len(pos))
    np.testing.assert_allclose(np.abs(w), 1.0, rtol=1e-15, atol=0)
    p = rts.beamform_eval(z.reshape(len(pos), 1, 1), w, power=True)[:, 0, 0]
    want = abs(amp) ** 2 * len(pos) ** 2
    print(array, "power at u0 %.17g, want %.17g; the fan:" % (p[k0], want), np.round(p / want, 4))
    assert abs(p[k0] - want) <= 1e-9 * want
    assert np.argmax(p) == k0 and np.all(np.delete(p, k0) < p[k0])                       # the strict maximum of the fan
    assert p[16 - k0] < 0.5 * p[k0]                                                      # the mirrored direction is not: the sign
    peak = rts.beamform_eval(z.reshape(len(pos), 1, 1), w, peak=True)[0, 0]
    assert peak[0] == p[k0] and abs(peak[1] - k0) <= 0.5
    az = rts.beam_angles(peak[1], fan)
    assert abs(az - fan[k0]) <= 0.5 * (fan[1] - fan[0])
    both = rts.beam_angles(np.array([0.0, 3.5, 16.0]), directions)
    assert both.shape == (3, 2) and both[1, 0] == 0.5 * (fan[3] + fan[4]) and both[2, 0] == fan[16] and np.all(both[:, 1] == el0)
    # a taper scales the weights exactly
    t = np.linspace(0.25, 1.75, len(pos))
    wt = rts.steering(pos, directions, wl, taper=t)
    assert np.array_equal(wt.real, t[None, :] * w.real) and np.array_equal(wt.imag, t[None, :] * w.imag)
    with pytest.raises(ValueError):
        rts.steering(pos, directions, wl, taper=t[:-1])


def test_steering_definition(rts):
    """w = cos 2 pi f + j sin 2 pi f, f = x - floor(x), x = ((ux px + uy py) + uz pz) / wavelength: against numpy, and exact where f is a
    multiple of a quarter turn"""
    rng = np.random.default_rng(5)
    pos = rng.uniform(-2.0, 2.0, (6, 3)); d = np.stack([rng.uniform(-math.pi, math.pi, 9), rng.uniform(-1.5, 1.5, 9)], axis=1)
    w = rts.steering(pos, d, 0.1)
    u = np.stack([np.cos(d[:, 1]) * np.cos(d[:, 0]), np.cos(d[:, 1]) * np.sin(d[:, 0]), np.sin(d[:, 1])], axis=1)
    np.testing.assert_allclose(w, np.exp(2j * np.pi * (u @ pos.T) / 0.1), rtol=0, atol=1e-12)      # (x is tens of turns: 1e-14 of a turn of rounding)
    quarter = rts.steering([[1.0, 0, 0], [1.25, 0, 0], [1.5, 0, 0], [-0.25, 0, 0], [0.0, 0, 0]], [[0.0, 0.0]], 1.0)[0]
    assert np.array_equal(quarter, np.array([1.0, 1j, -1.0, -1j, 1.0]))


# ----------------------------------------------------------------------------- 5. refusals
def eval_case(L):
    """a valid raw call: (q, inp, n_rows_in, p, keep); 3 receivers, 4 rows of 5 bins, rows 1 .. 2, 2 beams"""
    q = L.RtsCubeParams(3, 4, 5, 0, 0.0, 1.0)
    inp = np.ones((3, 4, 5, 2))
    w = np.arange(12, dtype=np.float64).reshape(2, 3, 2) / 8.0
    p = L.RtsBeamParams()
    p.n_beams, p.source, p.first_row, p.n_rows, p.n_rows_in, p.flags = 2, L.RTS_BEAM_FROM_CUBE, 1, 2, 0, 0
    p.weights = w.ctypes.data
    return q, inp, 4, p, dict(w=w)


def setter(**kw):
    def f(p, keep):
        for k, v in kw.items():
            setattr(p, k, v)
    return f


def test_beamform_eval_refusals(rts):
    from rts_amd import _lib as L
    lib = L.lib()

    def call(q, inp, rows_in, p, out):
        return lib.rts_beamform_eval(C.byref(q) if q is not None else None, inp.ctypes.data if inp is not None else None, rows_in,
                                     C.byref(p) if p is not None else None, out.ctypes.data if out is not None else None)

    def poison(index, value):
        def f(p, keep):
            keep["w"].reshape(-1)[index] = value
        return f

    def reserved(i):
        def f(p, keep):
            p.reserved[i] = 1
        return f
    out = np.full((2, 2, 5, 2), 7.25)
    q, inp, rows_in, p, keep = eval_case(L)
    assert call(q, inp, rows_in, p, out) == L.RTS_OK and not np.any(out == 7.25)
    big_w = np.ones(2 * 4097 + 2 * 1025 * 3)
    bad = [("reserved 0", reserved(0), b"reserved"), ("reserved 1", reserved(1), b"reserved"),
           ("unknown source", setter(source=3), b"source"), ("unknown flags", setter(flags=4), b"flags"),
           ("peak and power", setter(flags=L.RTS_BEAM_PEAK | L.RTS_BEAM_POWER), b"RTS_BEAM_PEAK"),
           ("no beams", setter(n_beams=0), b"n_beams"), ("too many beams", setter(n_beams=1025, weights=big_w.ctypes.data), b"n_beams"),
           ("null weights", setter(weights=None), b"weights"),
           ("weight nan", poison(5, math.nan), b"weights"), ("weight inf", poison(11, -math.inf), b"weights"),
           ("n_rows_in with the cube", setter(n_rows_in=4), b"n_rows_in"), ("n_rows_in with the map", setter(source=L.RTS_BEAM_FROM_MAP, n_rows_in=4), b"n_rows_in"),
           ("device_in with the cube", setter(device_in=inp.ctypes.data), b"device_in"),
           ("pointer without n_rows_in", setter(source=L.RTS_BEAM_FROM_POINTER), b"n_rows_in"),
           ("pointer with other rows", setter(source=L.RTS_BEAM_FROM_POINTER, n_rows_in=5), b"n_rows_in"),
           ("first_row beyond", setter(first_row=4, n_rows=0), b"first_row"), ("rows beyond", setter(first_row=3), b"n_rows"),
           ("wrapping rows", setter(first_row=2, n_rows=0xffffffff), b"n_rows")]
    for name, mutate, word in bad:
        q, inp, rows_in, p, keep = eval_case(L)
        mutate(p, keep)
        out[:] = 7.25
        assert call(q, inp, rows_in, p, out) == L.RTS_ERR_INVALID, name
        assert word in lib.rts_last_error(), (name, lib.rts_last_error())
        assert np.all(out == 7.25), name
    q, inp, rows_in, p, keep = eval_case(L)
    assert call(None, inp, rows_in, p, out) == L.RTS_ERR_INVALID and call(q, None, rows_in, p, out) == L.RTS_ERR_INVALID
    assert call(q, inp, rows_in, None, out) == L.RTS_ERR_INVALID and call(q, inp, rows_in, p, None) == L.RTS_ERR_INVALID
    assert call(q, inp, 0, p, out) == L.RTS_ERR_INVALID and b"n_rows_in" in lib.rts_last_error()
    assert call(L.RtsCubeParams(0, 4, 5, 0, 0.0, 1.0), inp, rows_in, p, out) == L.RTS_ERR_INVALID
    assert call(L.RtsCubeParams(3, 4, 0, 0, 0.0, 1.0), inp, rows_in, p, out) == L.RTS_ERR_INVALID
    # the limits: 65 receivers; 64 receivers x 65 beams (the weight table); 2^32 - 1 rows of 2^32 - 1 bins (the launch grid) -- each is
    # refused before a sample is read
    wide = np.ones(2 * 65 * 65)
    p.weights = wide.ctypes.data
    assert call(L.RtsCubeParams(65, 4, 5, 0, 0.0, 1.0), inp, rows_in, p, out) == L.RTS_ERR_INVALID and b"n_rx" in lib.rts_last_error()
    p.n_beams = 65
    assert call(L.RtsCubeParams(64, 4, 5, 0, 0.0, 1.0), inp, rows_in, p, out) == L.RTS_ERR_INVALID and b"n_beams * n_rx" in lib.rts_last_error()
    q, inp, rows_in, p, keep = eval_case(L)
    p.first_row, p.n_rows = 0, 0
    assert call(L.RtsCubeParams(3, 4, 0xffffffff, 0, 0.0, 1.0), inp, 0xffffffff, p, out) == L.RTS_ERR_INVALID and b"launch grid" in lib.rts_last_error()
    assert np.all(out == 7.25)
    # accepted edges: the pointer source with its rows, n_rows 0 (to the last row), the last row alone, each form
    for kw, shape in ((dict(source=L.RTS_BEAM_FROM_POINTER, n_rows_in=4), (2, 2, 5, 2)), (dict(source=L.RTS_BEAM_FROM_MAP), (2, 2, 5, 2)),
                      (dict(n_rows=0), (2, 3, 5, 2)), (dict(first_row=3, n_rows=1), (2, 1, 5, 2)), (dict(first_row=3, n_rows=0), (2, 1, 5, 2)),
                      (dict(flags=L.RTS_BEAM_POWER), (2, 2, 5)), (dict(flags=L.RTS_BEAM_PEAK), (2, 5, 2))):
        q, inp, rows_in, p, keep = eval_case(L)
        setter(**kw)(p, keep)
        full = np.full(int(np.prod(shape)) + 1, 7.25)
        assert call(q, inp, rows_in, p, full) == L.RTS_OK, kw
        assert not np.any(full[:-1] == 7.25) and full[-1] == 7.25, kw
    with pytest.raises(ValueError):
        rts.beamform_eval(np.zeros((3, 2, 4)), np.ones((2, 4)))
    with pytest.raises(L.RtsError):
        rts.beamform_eval(np.zeros((3, 2, 4)), np.ones((2, 3)), power=True, peak=True)


def test_steering_refusals(rts):
    from rts_amd import _lib as L
    lib = L.lib()
    pos = np.array([[0.0, 0.0, 0.0], [0.0, 0.015, 0.0]]); d = np.array([[0.1, 0.0], [0.2, 0.1], [0.3, 0.2]]); t = np.array([1.0, 0.5])
    out = np.full((3, 2, 2), 7.25)

    def call(pos_, n_rx, d_, n_beams, wl, t_, out_):
        a = lambda x: x.ctypes.data if x is not None else None
        return lib.rts_steering_make(a(pos_), n_rx, a(d_), n_beams, wl, a(t_), a(out_))
    assert call(pos, 2, d, 3, 0.03, t, out) == L.RTS_OK and not np.any(out == 7.25)
    out[:] = 7.25
    nan_pos = pos.copy(); nan_pos[1, 2] = math.nan
    inf_d = d.copy(); inf_d[2, 0] = math.inf
    nan_t = t.copy(); nan_t[0] = math.nan
    for name, args, word in (("null positions", (None, 2, d, 3, 0.03, t, out), b"null"), ("null directions", (pos, 2, None, 3, 0.03, t, out), b"null"),
                             ("null output", (pos, 2, d, 3, 0.03, t, None), b"null"),
                             ("no receivers", (pos, 0, d, 3, 0.03, t, out), b"n_rx"), ("no beams", (pos, 2, d, 0, 0.03, t, out), b"n_beams"),
                             ("wavelength 0", (pos, 2, d, 3, 0.0, t, out), b"wavelength"), ("wavelength < 0", (pos, 2, d, 3, -0.03, t, out), b"wavelength"),
                             ("wavelength nan", (pos, 2, d, 3, math.nan, t, out), b"wavelength"), ("wavelength inf", (pos, 2, d, 3, math.inf, t, out), b"wavelength"),
                             ("position nan", (nan_pos, 2, d, 3, 0.03, t, out), b"position"), ("direction inf", (pos, 2, inf_d, 3, 0.03, t, out), b"direction"),
                             ("taper nan", (pos, 2, d, 3, 0.03, nan_t, out), b"taper")):
        assert call(*args) == L.RTS_ERR_INVALID, name
        assert word in lib.rts_last_error(), (name, lib.rts_last_error())
        assert np.all(out == 7.25), name
    assert call(pos, 2, d, 3, 0.03, None, out) == L.RTS_OK and not np.any(out == 7.25)    # a NULL taper is no refusal


# ----------------------------------------------------------------------------- 6. rts_beam.h alone, under the sanitizers
@pytest.fixture(scope="module")
def beam_main(tmp_path_factory):
    gxx = shutil.which("g++")
    if not gxx:
        pytest.skip("no g++")
    rt = subprocess.run([gxx, "-print-file-name=libasan.so"], capture_output=True, text=True).stdout.strip()
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"] if os.path.isabs(rt) and os.path.exists(rt) else []
    exe = str(tmp_path_factory.mktemp("beam") / "beam_main")
    subprocess.check_call([gxx, "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-ffp-contract=off"] + san + ["-I", os.path.join(ROOT, "rts_amd", "csrc"),
                           os.path.join(ROOT, "tests", "beam", "beam_main.cpp"), "-o", exe])
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
    """the input tests/beam/beam_main.cpp fills"""
    r = np.arange(n_rx)[:, None, None]; p = np.arange(rows)[None, :, None]; b = np.arange(nb)[None, None, :]
    return (((r * 131 + p * 17 + b * 7) % 23) - 11.0 + 0.25 * p) + 1j * (((r * 5 + p * 3 + b * 11) % 19) - 9.0 - 0.5 * b)


def main_weights(n_beams, n_rx):
    """the weights tests/beam/beam_main.cpp fills"""
    b = np.arange(n_beams)[:, None]; r = np.arange(n_rx)[None, :]
    return (((b * 7 + r * 3) % 11) - 5.0) / 8.0 + 1j * (((b * 5 + r * 13) % 9) - 4.0) / 16.0


def test_header_alone_reads_only_what_it_is_given(beam_main):
    """input, weights and output are heap arrays of exactly their sizes, and every input row outside the span is poisoned in the driver: a
    read or write beyond them ends the run.  The values: the restatement's, bit for bit (small integers and eighths: every sum is exact
    or rounds as Python's)"""
    cases = [("beam", n_rx, rows_in, nb, first, rows, beams, flags)
             for (n_rx, beams) in ((1, 1), (3, 5), (8, 16), (9, 17), (17, 2))
             for (rows_in, first, rows) in ((1, 0, 1), (4, 1, 2), (4, 3, 1), (4, 0, 4))
             for nb in (1, 6) for flags in (0, 1, 2)]
    for c, g in zip(cases, beam_main(cases)):
        _, n_rx, rows_in, nb, first, rows, beams, flags = c
        y = B.beam_restated(main_input(n_rx, rows_in, nb), main_weights(beams, n_rx), first, rows)
        got = np.array(g)
        if flags == 0:
            assert np.array_equal(got, bits(y).ravel()), c
        elif flags == 1:
            assert np.array_equal(got, B.power_restated(y).ravel()), c
        else:
            want = B.peak_restated(B.power_restated(y)).ravel()
            assert np.array_equal(got[0::2], want[0::2]) and np.array_equal(np.rint(got[1::2]), np.rint(want[1::2])), c
            np.testing.assert_allclose(got[1::2], want[1::2], rtol=1e-12, atol=0, err_msg=str(c))
    # the streaming peak and the refinement it calls, on lists of their own
    lists = [[1.0], [1.0, 2.0], [2.0, 1.0], [1.0, 4.0, 2.0], [1.0, 4.0, 4.0, 1.0], [0.5] * 9, [1.0, 2.0, 3.0, 4.0, 5.0, 4.5], [5.0, 4.0, 6.0, 1.0, 6.0, 2.0],
             [float(1 + (i * 37) % 101) for i in range(300)]]
    got = beam_main([("peak",) + tuple(v) for v in lists])
    for v, (P, c) in zip(lists, got):
        b = v.index(max(v))
        off = 0.0 if b in (0, len(v) - 1) else beam_main([("delta", v[b - 1], v[b], v[b + 1])])[0][0]
        assert (P, c) == (max(v), b + off), v


def test_plan(beam_main):
    T, RT, BT, GRID, MAX_RX, MAX_BEAMS, MAX_W = beam_main([("consts",)], int)[0]
    assert (T, RT, BT, GRID, MAX_RX, MAX_BEAMS, MAX_W) == (256, 8, 16, 2 ** 31 - 1, 64, 1024, 4096)
    plan = lambda *a: beam_main([("plan",) + a], int)[0]          # n_rx n_beams n_rows n_bins flags -> groups rx_tiles beam_tiles cells lds out_doubles supported
    assert plan(1, 1, 1, 1, 0) == [1, 1, 1, 1, 16, 2, 1]
    assert plan(8, 16, 256, 4096, 0) == [4096, 1, 1, 2 ** 20, 2048, 2 * 16 * 2 ** 20, 1]
    assert plan(8, 16, 256, 4096, 1)[5] == 16 * 2 ** 20 and plan(8, 16, 256, 4096, 2)[5] == 2 * 2 ** 20
    # the workgroup's cells, the receiver tile and the beam tile at T - 1, T, T + 1
    assert [plan(3, 5, 1, n, 0)[0] for n in (T - 1, T, T + 1, 2 * T, 2 * T + 1)] == [1, 1, 2, 2, 3]
    assert [plan(n, 2, 1, 1, 0)[1] for n in (1, RT - 1, RT, RT + 1, 2 * RT, 2 * RT + 1, 64)] == [1, 1, 1, 2, 2, 3, 8]
    assert [plan(2, n, 1, 1, 0)[2] for n in (1, BT - 1, BT, BT + 1, 2 * BT + 1, 1024)] == [1, 1, 1, 2, 3, 64]
    # the limits: receivers, beams, the weight table (64 KiB of LDS), the grid
    assert plan(64, 64, 3, 5, 0)[4:] == [65536, 2 * 64 * 15, 1] and plan(4, 1024, 3, 5, 0)[4:] == [65536, 2 * 1024 * 15, 1]
    assert plan(65, 1, 3, 5, 0)[6] == 0 and plan(1, 1025, 3, 5, 0)[6] == 0 and plan(64, 65, 3, 5, 0)[6] == 0 and plan(5, 820, 3, 5, 0)[6] == 0
    assert plan(5, 819, 3, 5, 0)[6] == 1 and plan(0, 1, 3, 5, 0)[6] == 0 and plan(1, 0, 3, 5, 0)[6] == 0 and plan(1, 1, 0, 5, 0)[6] == 0
    assert plan(1, 1, 2 ** 31 - 1, T, 0)[::6] == [2 ** 31 - 1, 1] and plan(1, 1, 2 ** 31, T, 0)[::6] == [0, 0]
    assert plan(1, 1, 2 ** 32 - 1, 2 ** 32 - 1, 0)[3] == (2 ** 32 - 1) ** 2 and plan(1, 1, 2 ** 32 - 1, 2 ** 32 - 1, 0)[6] == 0


# ----------------------------------------------------------------------------- 7. the whole chain, on the host
def test_chain_on_the_host(rts):
    """the run that fixed tests/beam_ref.py's CHAIN: both targets are detected at their (beam, Doppler bin, range bin), every detection
    lies in a target's range bin, and the weak target -- 10 dB below the per-element noise -- is in no single element's list"""
    cube, w, beams, det, det_el = B.chain_host(rts)
    strong, weak = B.chain_target_cells()
    found = B.cells(det)
    print("beams:", sorted(found)); print("elements:", sorted(B.cells(det_el)))
    assert strong in found and weak in found
    assert {c[2] for c in found} == {strong[2], weak[2]}
    assert len(det) == 12
    assert not any(abs(c[1] - weak[1]) <= 1 and abs(c[2] - weak[2]) <= 1 for c in B.cells(det_el))
    assert all(any(c == (rx,) + strong[1:] for c in B.cells(det_el)) for rx in range(8))  # the strong one is in every element's
    # the array gain, measured on the clean cube: a beam at the target holds n_rx^2 times an element's power
    clean = rts.beamform_eval(B.chain_clean_cube(), w, power=True)
    for t in B.CHAIN["targets"]:
        np.testing.assert_allclose(clean[t["beam"], :, t["range_bin"]], 64 * t["power"], rtol=1e-9)
    # the peak form points at the strong target's beam in its range bin
    peak = rts.beamform_eval(cube, w, peak=True)
    assert np.all(np.rint(peak[:, strong[2], 1]) == strong[0])
