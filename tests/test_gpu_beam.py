"""Receive-array beamforming on the device (rts_cube_beamform): the kernel against the host evaluator rts_beamform_eval BIT FOR BIT in
its complex and power forms (the tree holds no transcendental) over the smallest shapes at which it can go wrong -- one cell, odd
sizes, the workgroup's cells and both tile constants of rts_amd/csrc/rts_beam.h at T - 1, T, T + 1, the limits of receivers, beams
and the weight table; sentinel cells around a caller-owned output; the three sources; linearity across the chain; the whole chain
of tests/beam_ref.py against its host run; run-to-run equality; and the error / lifetime rules on a live handle.

The peak form's power and beam are compared bit for bit; its offset goes through a logarithm, which the device's library and libm
round differently: it is compared as tests/test_gpu_cfar_os.py compares a detection's range_offset (tests/cfar_os_ref.py:
assert_same_list), rtol 1e-12 and atol 1e-12 of the largest offset.  Where sums associate differently (linearity) the bound is the
project's for a kernel against its evaluator, rtol 1e-10 and atol 1e-12 max|ref|."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

import beam_ref as B

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def header_constant(name):
    with open(os.path.join(ROOT, "rts_amd", "csrc", "rts_beam.h")) as f:
        return int(re.search(r"#define %s (\d+)u" % name, f.read()).group(1))


T, RT, BT = header_constant("RTS_BEAM_THREADS"), header_constant("RTS_BEAM_RX_TILE"), header_constant("RTS_BEAM_BEAM_TILE")


def dev(a, dtype=np.complex128):
    """(torch's stream is not the handles': the buffer is finished before a handle reads it, and a handle's work before torch reads it)"""
    import torch
    buf = torch.from_numpy(np.array(a, dtype, order="C")).to("cuda")
    torch.cuda.synchronize()
    return buf


def filled(n, value, dtype):
    import torch
    buf = torch.full((n,), value, dtype=dtype, device="cuda")
    torch.cuda.synchronize()
    return buf


def host(buf):
    import torch
    torch.cuda.synchronize()
    return buf.cpu().numpy()


def bits(a):
    return np.ascontiguousarray(a).view(np.float64)


def assert_bound(got, ref, what=""):
    np.testing.assert_allclose(got, ref, rtol=1e-10, atol=1e-12 * np.abs(ref).max(), err_msg=str(what))


def assert_peak(got, want, what=""):
    """power and beam bit for bit, the offset as a detection's range_offset"""
    assert np.array_equal(got[..., 0], want[..., 0]), what
    b_got, b_want = np.rint(got[..., 1]), np.rint(want[..., 1])
    assert np.array_equal(b_got, b_want), what
    off_got, off_want = got[..., 1] - b_got, want[..., 1] - b_want
    scale = max(np.abs(off_want).max(initial=0.0), 1e-300)
    np.testing.assert_allclose(off_got, off_want, rtol=1e-12, atol=1e-12 * scale, err_msg=str(what))


def attached(rts, inp):
    """a handle with the host array [n_rx][rows][n_bins] attached as its cube: (handle, the device tensor)"""
    d = dev(inp)
    tr = rts.Tracer(8, 1)
    tr.cube_attach(inp.shape[0], inp.shape[1], inp.shape[2], 0.0, 1.0, device_ptr=d.data_ptr())
    return tr, d


# ----------------------------------------------------------------------------- 1. against the evaluator
SHAPES = [  # n_rx, n_beams, rows of the cube, first_row, n_rows, n_bins
    (1, 1, 1, 0, 1, 1), (2, 2, 3, 2, 1, 63), (3, 5, 5, 2, 3, 64), (8, 64, 3, 0, 3, 65), (64, 64, 1, 0, 1, 130), (4, 1024, 3, 2, 1, 65),
    (3, 2, 3, 0, 3, 130), (8, 5, 1, 0, 1, 1), (64, 1, 3, 2, 1, 63),
    # the workgroup's cells at T - 1, T, T + 1 (one row, and three rows that cross it)
    (2, 3, 1, 0, 1, T - 1), (2, 3, 1, 0, 1, T), (2, 3, 1, 0, 1, T + 1), (2, 3, 4, 1, 3, (T + 1) // 3 + 1),
    # the receiver tile and the beam tile at their edges, and at the edges of two tiles
    (RT - 1, 3, 1, 0, 1, 65), (RT, BT - 1, 1, 0, 1, 65), (RT + 1, BT, 1, 0, 1, 65), (2 * RT, BT + 1, 1, 0, 1, 65), (2 * RT + 1, 2 * BT + 1, 3, 0, 3, 7),
]


@pytest.mark.parametrize("n_rx,n_beams,rows_in,first,rows,nb", SHAPES)
def test_device_against_the_evaluator(rts, n_rx, n_beams, rows_in, first, rows, nb):
    rng = np.random.default_rng(n_rx * 100003 + n_beams * 1009 + nb)
    inp = B.random_complex(rng, (n_rx, rows_in, nb)); w = B.random_complex(rng, (n_beams, n_rx))
    tr, d = attached(rts, inp)
    what = (n_rx, n_beams, rows_in, first, rows, nb)
    for form in (dict(), dict(power=True), dict(peak=True)):
        want = rts.beamform_eval(inp, w, first=first, count=rows, **form)
        got = tr.cube_beamform(w, first=first, count=rows, **form)
        assert got.shape == want.shape and got.dtype == want.dtype
        if "peak" in form:
            assert_peak(got, want, what)
        else:
            assert np.array_equal(bits(got), bits(want)), (what, form)
    assert np.array_equal(bits(tr.cube_beamform(w, first=first)), bits(rts.beamform_eval(inp, w, first=first)))          # n_rows 0: to the last row
    tr.close()


def test_peak_ties_edges_and_nan(rts):
    """one receiver, z = 1 in every cell but one NaN, real weights: the streaming peak's rules on the device, in two beam tiles"""
    amps = np.array([1.0, 2.0, 2.0, 1.0] + [0.5] * (BT - 4) + [2.0, 1.0])
    inp = np.ones((1, 1, 5), np.complex128); inp[0, 0, 3] = math.nan
    tr, d = attached(rts, inp)
    got = tr.cube_beamform(amps.reshape(-1, 1), peak=True)
    want = rts.beamform_eval(inp, amps.reshape(-1, 1), peak=True)
    assert np.array_equal(got[0, [0, 1, 2, 4]], want[0, [0, 1, 2, 4]]) and tuple(got[0, 0]) == (4.0, 1.5)                  # the lowest beam of the ties
    assert 0.0 <= got[0, 3, 1] <= len(amps) - 1 or math.isnan(got[0, 3, 1])                                                # NaN: some beam, unspecified
    last = np.arange(1.0, BT + 3.0)
    assert tuple(tr.cube_beamform(last.reshape(-1, 1), peak=True)[0, 0]) == (float((BT + 2) ** 2), float(BT + 1))         # the last beam: no offset
    assert tuple(tr.cube_beamform(last[::-1].copy().reshape(-1, 1), peak=True)[0, 0]) == (float((BT + 2) ** 2), 0.0)      # the first beam
    tr.close()


# ----------------------------------------------------------------------------- 2. sentinels; the library-owned output
@pytest.mark.parametrize("form", ["complex", "power", "peak"])
def test_sentinels_and_owned_output(rts, form):
    import torch
    rng = np.random.default_rng(17)
    inp = B.random_complex(rng, (5, 4, 67)); w = B.random_complex(rng, (BT + 1, 5))
    kw = dict(power=form == "power", peak=form == "peak")
    want = rts.beamform_eval(inp, w, first=1, count=2, **kw)
    tr, d = attached(rts, inp)
    PAD = 16
    if form == "complex":
        buf = filled(want.size + 2 * PAD, complex(7.25, -3.5), torch.complex128); step = 16
    else:
        buf = filled(want.size + 2 * PAD, 7.25, torch.float64); step = 8
    assert tr.cube_beamform(w, first=1, count=2, device_ptr=buf.data_ptr() + step * PAD, **kw) is None
    tr.cube()                                                                    # (the handle's stream drained)
    got = host(buf)
    assert np.all(got[:PAD] == got[0]) and np.all(got[-PAD:] == got[0]) and got[0] in (7.25, complex(7.25, -3.5))
    body = got[PAD:-PAD].reshape(want.shape)
    owned = tr.cube_beamform(w, first=1, count=2, **kw)
    assert np.array_equal(bits(owned), bits(body)) and np.array_equal(bits(tr.beam_map()), bits(body))
    if form == "peak":
        assert_peak(body, want)
    else:
        assert np.array_equal(bits(body), bits(want))
    assert np.array_equal(bits(host(d)), bits(inp))                              # the input is only read
    tr.close()


# ----------------------------------------------------------------------------- 3. the three sources
def test_three_sources(rts):
    rng = np.random.default_rng(23)
    n_rx, n_p, nb, n_fft = 3, 6, 37, 8
    inp = B.random_complex(rng, (n_rx, n_p, nb)); w = B.random_complex(rng, (4, n_rx))
    tr, d = attached(rts, inp)
    dmap = tr.cube_doppler(n_fft)                                                # library-owned
    from_map = tr.cube_beamform(w, source="map", first=1, count=5)
    dm = dev(dmap)
    from_ptr = tr.cube_beamform(w, source="pointer", device_in=dm.data_ptr(), n_rows_in=n_fft, first=1, count=5)
    assert from_map.shape == (4, 5, nb) and np.count_nonzero(from_map) == from_map.size
    assert np.array_equal(bits(from_map), bits(from_ptr))
    assert np.array_equal(bits(from_map), bits(rts.beamform_eval(dmap, w, first=1, count=5)))
    assert np.array_equal(bits(tr.cube_beamform(w, source="map")), bits(rts.beamform_eval(dmap, w)))                      # every row of the map
    from_cube = tr.cube_beamform(w, source="cube", first=2, count=3)
    again = tr.cube_beamform(w, source="pointer", device_in=d.data_ptr(), n_rows_in=n_p, first=2, count=3)
    assert np.array_equal(bits(from_cube), bits(again)) and np.array_equal(bits(from_cube), bits(rts.beamform_eval(inp, w, first=2, count=3)))
    # a pointer source of other rows than the cube's
    other = B.random_complex(rng, (n_rx, 2, nb)); do = dev(other)
    assert np.array_equal(bits(tr.cube_beamform(w, source="pointer", device_in=do.data_ptr(), n_rows_in=2)), bits(rts.beamform_eval(other, w)))
    tr.close()


# ----------------------------------------------------------------------------- 4. linearity across the chain
def test_beamform_and_doppler_commute(rts):
    import torch
    rng = np.random.default_rng(29)
    n_rx, n_p, nb, n_fft, n_beams = 4, 12, 33, 16, 6
    inp = B.random_complex(rng, (n_rx, n_p, nb)); w = B.random_complex(rng, (n_beams, n_rx))
    tr, d = attached(rts, inp)
    beams = filled(n_beams * n_p * nb, 0j, torch.complex128)
    tr.cube_beamform(w, device_ptr=beams.data_ptr())
    tr.cube()                                                                    # (drained: the second handle's stream reads the beams)
    t2 = rts.Tracer(8, 1); t2.cube_attach(n_beams, n_p, nb, 0.0, 1.0, device_ptr=beams.data_ptr())
    beams_then_doppler = t2.cube_doppler(n_fft)
    tr.cube_doppler(n_fft, fetch=False)
    doppler_then_beams = tr.cube_beamform(w, source="map")
    assert beams_then_doppler.shape == doppler_then_beams.shape == (n_beams, n_fft, nb)
    print("max difference %.3g of max %.3g" % (np.abs(beams_then_doppler - doppler_then_beams).max(), np.abs(doppler_then_beams).max()))
    assert_bound(beams_then_doppler, doppler_then_beams)
    tr.close(); t2.close()


# ----------------------------------------------------------------------------- 5. the whole chain
def assert_same_detections(got, want):
    assert len(got) == len(want), (len(got), len(want))
    for f in ("rx", "doppler_bin", "range_bin", "n_train"):
        assert np.array_equal(got[f], want[f]), f
    for f in ("power", "noise", "threshold", "range_offset", "doppler_offset", "delay", "doppler"):
        scale = max(np.abs(want[f]).max(initial=0.0), 1e-300)
        np.testing.assert_allclose(got[f], want[f], rtol=1e-10, atol=1e-12 * scale, err_msg=f)


def test_whole_chain(rts):
    """tests/beam_ref.py's scenario on the device: noise, a 17-beam fan, the beams attached to a second handle, its Doppler map and
    OS-CFAR with the local-maximum rule.  The list is the host chain's (tests/test_beam_host.py: test_chain_on_the_host)."""
    import torch
    ch = B.CHAIN
    n_rx, n_p, nb = ch["n_rx"], ch["n_pulses"], ch["n_bins"]
    cube_h, w, beams_h, det_h, det_el_h = B.chain_host(rts)
    strong, weak = B.chain_target_cells()
    tr, d = attached(rts, B.chain_clean_cube())
    tr.cube_add_noise(ch["noise_power"], ch["seed"])
    beams = filled(17 * n_p * nb, 0j, torch.complex128)
    tr.cube_beamform(w, device_ptr=beams.data_ptr())
    noisy = tr.cube()                                                            # (drains the stream: the second handle reads the beams)
    assert_bound(noisy, cube_h, "noisy cube")
    assert np.array_equal(bits(host(beams).reshape(17, n_p, nb)), bits(rts.beamform_eval(noisy, w)))                      # of the device's own cube: bit for bit
    t2 = rts.Tracer(8, 1); t2.cube_attach(17, n_p, nb, 0.0, 1.0, device_ptr=beams.data_ptr())
    t2.cube_doppler(n_p, fetch=False)
    det = t2.cube_detect_os(ch["guard"], ch["train"], None, pfa=ch["pfa"], local_max=True)
    assert_same_detections(det, det_h)
    assert strong in B.cells(det) and weak in B.cells(det)
    # the same detector on the elements: the strong target in every one, the weak one in none
    tr.cube_doppler(n_p, fetch=False)
    det_el = tr.cube_detect_os(ch["guard"], ch["train"], None, pfa=ch["pfa"], local_max=True)
    assert_same_detections(det_el, det_el_h)
    assert all((rx,) + strong[1:] in B.cells(det_el) for rx in range(n_rx))
    assert not any(c[1:] == weak[1:] for c in B.cells(det_el))
    # the peak form reports the strong target's beam in its range bin
    peak = tr.cube_beamform(w, peak=True)
    assert np.all(np.rint(peak[:, strong[2], 1]) == strong[0])
    tr.close(); t2.close()


# ----------------------------------------------------------------------------- 6. run to run
def test_run_to_run(rts):
    rng = np.random.default_rng(31)
    inp = B.random_complex(rng, (2 * RT + 1, 3, 2 * T + 5)); w = B.random_complex(rng, (BT + 3, 2 * RT + 1))
    runs = []
    for _ in range(2):
        tr, d = attached(rts, inp)
        runs.append([tr.cube_beamform(w, **form).tobytes() for form in (dict(), dict(power=True), dict(peak=True))])
        runs.append([tr.cube_beamform(w, **form).tobytes() for form in (dict(), dict(power=True), dict(peak=True))])
        tr.close()
    assert runs[0] == runs[1] == runs[2] == runs[3]


# ----------------------------------------------------------------------------- 7. errors and lifetime
def test_errors_and_lifetime(rts):
    from rts_amd import _lib as L
    import torch
    lib = L.lib()
    rng = np.random.default_rng(37)
    n_rx, n_p, nb, n_beams = 3, 4, 40, 2
    inp = B.random_complex(rng, (n_rx, n_p, nb))
    wts = np.ascontiguousarray(B.random_complex(rng, (n_beams, n_rx)))
    out = np.full(2 * n_beams * n_p * nb + 2, 7.25)

    def params(**kw):
        p = L.RtsBeamParams()
        p.n_beams, p.source, p.weights = n_beams, L.RTS_BEAM_FROM_CUBE, wts.ctypes.data
        for k, v in kw.items():
            setattr(p, k, v)
        return p
    tr = rts.Tracer(8, 1)
    # no cube
    assert lib.rts_cube_beamform(tr.h, C.byref(params()), None) == L.RTS_ERR_INVALID and b"attach" in lib.rts_last_error()
    assert lib.rts_cube_beam_get(tr.h, out.ctypes.data, out.size) == L.RTS_ERR_INVALID
    d = dev(inp)
    tr.cube_attach(n_rx, n_p, nb, 0.0, 1.0, device_ptr=d.data_ptr())
    assert lib.rts_cube_beam_get(tr.h, out.ctypes.data, out.size) == L.RTS_ERR_INVALID and b"beam" in lib.rts_last_error()     # no output yet
    first = tr.cube_beamform(wts)                                                # a library-owned output the refusals must leave alone
    assert np.array_equal(bits(first), bits(rts.beamform_eval(inp, wts)))
    caller = filled(n_beams * n_p * nb + 1, 0j, torch.complex128)
    other = dev(B.random_complex(rng, (n_rx, 2, nb)))
    bad_w = wts.copy(); bad_w[1, 2] = complex(1.0, math.inf)
    many = np.ones((1025, n_rx), np.complex128)
    res1 = params(); res1.reserved[1] = 1
    cases = [("null p", None, None, b"null"), ("null weights", params(weights=None), None, b"weights"), ("reserved", res1, None, b"reserved"),
             ("source", params(source=3), None, b"source"), ("flags", params(flags=4), None, b"flags"),
             ("peak and power", params(flags=L.RTS_BEAM_PEAK | L.RTS_BEAM_POWER), None, b"RTS_BEAM_PEAK"),
             ("no beams", params(n_beams=0), None, b"n_beams"), ("too many beams", params(n_beams=1025, weights=many.ctypes.data), None, b"n_beams"),
             ("weight inf", params(weights=bad_w.ctypes.data), None, b"weights"),
             ("no map", params(source=L.RTS_BEAM_FROM_MAP), None, b"RTS_BEAM_FROM_MAP"),
             ("pointer null", params(source=L.RTS_BEAM_FROM_POINTER, n_rows_in=2), None, b"device_in"),
             ("pointer misaligned", params(source=L.RTS_BEAM_FROM_POINTER, n_rows_in=1, device_in=other.data_ptr() + 8), None, b"device_in"),
             ("pointer without rows", params(source=L.RTS_BEAM_FROM_POINTER, device_in=other.data_ptr()), None, b"n_rows_in"),
             ("n_rows_in with the cube", params(n_rows_in=2), None, b"n_rows_in"), ("device_in with the cube", params(device_in=other.data_ptr()), None, b"device_in"),
             ("first_row beyond", params(first_row=n_p), None, b"first_row"), ("rows beyond", params(first_row=2, n_rows=3), None, b"n_rows"),
             ("rows beyond the pointer's", params(source=L.RTS_BEAM_FROM_POINTER, n_rows_in=2, device_in=other.data_ptr(), n_rows=3), None, b"n_rows"),
             ("device_out misaligned", params(), caller.data_ptr() + 8, b"device_out"),
             ("in place", params(), d.data_ptr(), b"overlaps"), ("overlapping the last receiver", params(first_row=3, n_rows=1), d.data_ptr() + 16 * ((2 * n_p + 3) * nb + nb - 1), b"overlaps")]
    for name, p, device_out, word in cases:
        rc = lib.rts_cube_beamform(tr.h, C.byref(p) if p is not None else None, C.c_void_p(device_out) if device_out else None)
        assert rc == L.RTS_ERR_INVALID, name
        assert word in lib.rts_last_error(), (name, lib.rts_last_error())
    assert np.array_equal(bits(tr.beam_map()), bits(first))                      # the previous output is still there, and readable
    assert np.array_equal(bits(host(d)), bits(inp)) and np.count_nonzero(host(caller)) == 0
    # an output just beside the rows the call reads is no overlap: row 3 of the last receiver is read, the output ends where it begins
    tr2 = rts.Tracer(8, 1); tr2.cube_attach(1, n_p, nb, 0.0, 1.0, device_ptr=d.data_ptr() + 16 * 2 * n_p * nb)
    one = np.ones((1, 1), np.complex128)
    p1 = L.RtsBeamParams(); p1.n_beams, p1.first_row, p1.n_rows, p1.weights = 1, 3, 1, one.ctypes.data
    assert lib.rts_cube_beamform(tr2.h, C.byref(p1), C.c_void_p(d.data_ptr() + 16 * (2 * n_p + 2) * nb)) == L.RTS_OK
    tr2.cube()
    after = host(d)
    assert np.array_equal(bits(after[2, 2]), bits(inp[2, 3])) and np.array_equal(bits(after[2, 3]), bits(inp[2, 3])) and np.array_equal(bits(after[:2]), bits(inp[:2]))
    tr2.close()
    inp = after                                                                  # (what the cube holds from here on)
    # a shape the launch grid cannot take: 2^32 - 1 rows of 256 bins are 2^32 - 1 workgroups; refused before anything is enqueued
    tg = rts.Tracer(8, 1); tg.cube_attach(1, 1, 256, 0.0, 1.0)
    pg = L.RtsBeamParams(); pg.n_beams, pg.source, pg.n_rows_in, pg.device_in, pg.weights = 1, L.RTS_BEAM_FROM_POINTER, 0xffffffff, other.data_ptr(), one.ctypes.data
    assert lib.rts_cube_beamform(tg.h, C.byref(pg), C.c_void_p(caller.data_ptr())) == L.RTS_ERR_INVALID and b"launch grid" in lib.rts_last_error()
    tg.close()
    # limits that need a cube of their own: 65 receivers; 64 receivers and 65 beams
    for rx_big, beams_big, word in ((65, 1, b"n_rx"), (64, 65, b"n_beams * n_rx")):
        tb = rts.Tracer(8, 1); tb.cube_attach(rx_big, 1, 1, 0.0, 1.0)
        wb = np.ones((beams_big, rx_big), np.complex128)
        pb = L.RtsBeamParams(); pb.n_beams, pb.weights = beams_big, wb.ctypes.data
        assert lib.rts_cube_beamform(tb.h, C.byref(pb), None) == L.RTS_ERR_INVALID and word in lib.rts_last_error(), word
        tb.close()
    # a caller-owned output is not recorded; capacity; another size replaces the library-owned output; the beams end at rts_cube_attach
    assert lib.rts_cube_beamform(tr.h, C.byref(params(flags=L.RTS_BEAM_POWER)), C.c_void_p(caller.data_ptr())) == L.RTS_OK
    assert np.array_equal(bits(tr.beam_map()), bits(first))
    assert lib.rts_cube_beam_get(tr.h, out.ctypes.data, 2 * n_beams * n_p * nb - 1) == L.RTS_ERR_CAPACITY
    assert np.all(out == 7.25)
    assert lib.rts_cube_beam_get(tr.h, None, out.size) == L.RTS_ERR_INVALID
    assert lib.rts_cube_beam_get(tr.h, out.ctypes.data, out.size) == L.RTS_OK and out[-1] == 7.25 and out[-2] == 7.25
    assert np.array_equal(out[:-2], bits(first).ravel())
    big = tr.cube_beamform(np.concatenate([wts, wts, wts]), first=1)             # a larger output, then a smaller one
    assert big.shape == (6, 3, nb) and np.array_equal(bits(big[2:4]), bits(rts.beamform_eval(inp, wts, first=1)))
    small = tr.cube_beamform(wts, first=3, peak=True)
    assert small.shape == (1, nb, 2) and lib.rts_cube_beam_get(tr.h, out.ctypes.data, 2 * nb - 1) == L.RTS_ERR_CAPACITY
    tr.cube_doppler(4, fetch=False)                                              # with a library-owned map the map source works
    assert tr.cube_beamform(wts, source="map").shape == (n_beams, 4, nb)
    keep = zeros = filled(n_rx * 4 * nb, 0j, torch.complex128)
    tr.cube_doppler(4, device_ptr=zeros.data_ptr(), fetch=False)                 # ... and a caller-owned map is not it
    assert lib.rts_cube_beamform(tr.h, C.byref(params(source=L.RTS_BEAM_FROM_MAP)), None) == L.RTS_ERR_INVALID and b"RTS_BEAM_FROM_MAP" in lib.rts_last_error()
    tr.cube_attach(n_rx, n_p, nb, 0.0, 1.0, device_ptr=d.data_ptr())
    assert lib.rts_cube_beam_get(tr.h, out.ctypes.data, out.size) == L.RTS_ERR_INVALID and b"rts_cube_attach" in lib.rts_last_error()
    tr.close()
    del keep
    for call in (lambda: tr.cube_beamform(wts), lambda: tr.beam_map()):
        with pytest.raises(L.RtsError):
            call()


def test_output_right_behind_the_last_cell_read(rts):
    """the accepted neighbour of the two overlap refusals of test_errors_and_lifetime: the caller's output starts at the first byte behind
    the last receiver's last cell read, inside the cube's own allocation: RTS_OK, the library-owned call's bytes, the sentinel behind it
    and the cube untouched"""
    from rts_amd import _lib as L
    import torch
    lib = L.lib()
    rng = np.random.default_rng(41)
    n_rx, n_p, nb, n_beams = 3, 4, 7, 2
    inp = B.random_complex(rng, (n_rx, n_p, nb))
    wts = np.ascontiguousarray(B.random_complex(rng, (n_beams, n_rx)))
    block = torch.empty(inp.size + n_beams * n_p * nb + 1, dtype=torch.complex128, device="cuda")      # ONE allocation: [the cube | the caller's output | a sentinel]
    block[:inp.size] = torch.from_numpy(inp.ravel()); block[inp.size:] = complex(7.25, -7.25)
    torch.cuda.synchronize()
    tr = rts.Tracer(8, 1)
    tr.cube_attach(n_rx, n_p, nb, 0.0, 1.0, device_ptr=block.data_ptr())
    owned = tr.cube_beamform(wts)
    p = L.RtsBeamParams(); p.n_beams, p.source, p.weights = n_beams, L.RTS_BEAM_FROM_CUBE, wts.ctypes.data
    assert lib.rts_cube_beamform(tr.h, C.byref(p), C.c_void_p(block.data_ptr() + 16 * inp.size)) == L.RTS_OK, lib.rts_last_error()
    tr.cube()                                                                    # (drains the handle's stream)
    after = host(block)
    assert np.array_equal(bits(after[inp.size:-1]), bits(np.asarray(owned).ravel()))
    assert after[-1] == complex(7.25, -7.25) and np.array_equal(bits(after[:inp.size]), bits(inp.ravel()))
    tr.close()
