"""Backprojection imaging on the device (rts_cube_backproject, rts_cube_image_get) against the host evaluator rts_backproject_eval
(itself checked against a numpy restatement in tests/test_image_host.py): the shapes of that comparison, guarded caller-owned
outputs, the pulse-chunk edges on both launch shapes, output ownership and accumulation, the image behind the real chain
trace -> finalise -> render -> compress, and the error cases.

Device against evaluator: rtol 1e-10, atol 1e-12 max|ref| -- the project's bound for the render against its restatement
(tests/test_gpu_render.py).  It applies because both sides form carrier * tau from the same correctly rounded operations and reduce
it identically; what remains are the libraries' sincospi, cos and sinpi, a few ulp of a term each."""
import ctypes as C
import math

import numpy as np
import pytest

import helpers as H
import test_image_host as TH

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -52


def to_device(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def attach(rts, cube, g):
    """a handle with the host cube attached as a caller-owned device tensor: (tracer, the tensor)"""
    buf = to_device(cube)
    t = rts.Tracer(8, 1)
    t.cube_attach(cube.shape[0], cube.shape[1], cube.shape[2], g["t0"], g["dt"], device_ptr=buf.data_ptr())
    return t, buf


def device_image(t, g, taps, first, weights=None, **kw):
    return t.cube_backproject(g["origin"], g["step_x"], g["step_y"], g["n_x"], g["n_y"], g["tx"], g["rx"], g["c"], g["fc"], taps=taps, first=first,
                              weights=weights, **kw)


def assert_close(got, ref, what=""):
    err = float(np.abs(got - ref).max())
    print("%s: max |device - evaluator| %.3g, max |evaluator| %.3g" % (what, err, np.abs(ref).max()))
    np.testing.assert_allclose(got, ref, rtol=1e-10, atol=1e-12 * np.abs(ref).max(), err_msg=str(what))


# ----------------------------------------------------------------------------- G1
@pytest.mark.parametrize("P", [1, 5, 65])
def test_device_against_evaluator(rts, P):
    g = TH.geometry(P)
    cube = TH.random_cube(900 + P)
    t, buf = attach(rts, cube, g)
    for taps in (1, 2, 8):
        for weights in (None, TH.hann(P)):
            got = device_image(t, g, taps, 3, weights)
            ref = TH.call_eval(rts, cube, g, taps, 3, weights)
            assert np.count_nonzero(ref) > 20
            assert_close(got, ref, (P, taps, weights is not None))
    t.close()


# ----------------------------------------------------------------------------- G2
@pytest.mark.parametrize("P", [5, 65])
def test_guarded_output(rts, P):
    import torch
    cube = TH.random_cube(40 + P)
    sentinel = complex(-7.5e300, 3.25e-300)
    for n_x, n_y in ((1, 1), (17, 3), (16, 16), (33, 1), (1, 33)):
        g = TH.geometry(P, n_x=n_x, n_y=n_y)
        g["step_x"] = (0.9, 0.0, 0.0); g["step_y"] = (0.0, 0.9, 0.0)
        t, buf = attach(rts, cube, g)
        plane = n_x * n_y
        guard = torch.full(((2 + 2) * plane,), sentinel, dtype=torch.complex128, device="cuda")
        device_image(t, g, 8, 0, device_ptr=guard.data_ptr() + 16 * plane)
        t.cube()                                           # (drains the handle's stream)
        out = guard.cpu().numpy()
        assert np.all(out[:plane] == sentinel) and np.all(out[3 * plane:] == sentinel), (n_x, n_y)
        img = out[plane:3 * plane].reshape(2, n_y, n_x)
        assert not np.any(img == sentinel), (n_x, n_y)
        assert_close(img, TH.call_eval(rts, cube, g, 8, 0), (n_x, n_y, P))
        t.close()


# ----------------------------------------------------------------------------- G3
@pytest.mark.parametrize("split_below", [None, "0", "65536"])
def test_chunk_edges(rts, monkeypatch, split_below):
    """P at the edges of the 64-pulse chunks, at both ends of the cube; with the chunks on the grid (a small image: the default),
    walked by each thread (RTS_IMAGE_SPLIT_BELOW=0) and on the grid whenever there are two: the same bits"""
    if split_below is not None:
        monkeypatch.setenv("RTS_IMAGE_SPLIT_BELOW", split_below)
    rows = 130
    cube = TH.random_cube(5, rows=rows)
    t = None
    for P in (1, 63, 64, 65, 129):
        g = TH.geometry(P)
        if t is None:
            t, buf = attach(rts, cube, g)
        t.cube_attach(2, rows, 48, g["t0"], g["dt"], device_ptr=buf.data_ptr())
        for first in (0, rows - P):
            a = device_image(t, g, 8, first)
            b = device_image(t, g, 8, first)
            assert np.array_equal(a.view(np.float64), b.view(np.float64)), (P, first)
            assert_close(a, TH.call_eval(rts, cube, g, 8, first), (P, first, split_below))
            if split_below is not None:
                monkeypatch.delenv("RTS_IMAGE_SPLIT_BELOW")
                d, _ = attach(rts, cube, g)
                monkeypatch.setenv("RTS_IMAGE_SPLIT_BELOW", split_below)
                assert np.array_equal(device_image(d, g, 8, first).view(np.float64), a.view(np.float64)), (P, first, split_below)
                d.close()
    t.close()


# ----------------------------------------------------------------------------- G4
def test_output_ownership_and_accumulation(rts):
    import torch
    from rts_amd import _lib as L
    P, rows = 129, 130
    g = TH.geometry(P)
    cube = TH.random_cube(6, rows=rows)
    w = TH.hann(P)
    t, buf = attach(rts, cube, g)
    mine = torch.zeros((2, g["n_y"], g["n_x"]), dtype=torch.complex128, device="cuda")
    device_image(t, g, 8, 1, w, device_ptr=mine.data_ptr())
    with pytest.raises(L.RtsError):
        t.image()                                          # a caller-owned output is not the library's image: there is none yet
    owned = device_image(t, g, 8, 1, w)
    assert np.array_equal(owned.view(np.float64), mine.cpu().numpy().view(np.float64))
    assert np.array_equal(t.image().view(np.float64), owned.view(np.float64))
    # accumulate over pulse subsets, library-owned and caller-owned
    _, B = TH.bound(g, 8, w, float(np.abs(cube).max()))
    parts = [(0, 64), (64, 129)]
    mine.zero_()
    for k, (lo, hi) in enumerate(parts):
        part = dict(g, tx=g["tx"][lo:hi], rx=g["rx"][:, lo:hi])
        device_image(t, part, 8, 1 + lo, w[lo:hi], accumulate=k > 0, fetch=False)
        device_image(t, part, 8, 1 + lo, w[lo:hi], accumulate=True, device_ptr=mine.data_ptr())
    acc = t.image()
    assert np.abs(acc - owned).max() <= 16 * EPS * B
    assert np.abs(mine.cpu().numpy() - owned).max() <= 16 * EPS * B
    # an image ends at rts_cube_attach
    t.cube_attach(2, rows, 48, g["t0"], g["dt"], device_ptr=buf.data_ptr())
    with pytest.raises(L.RtsError):
        t.image()
    with pytest.raises(L.RtsError):
        device_image(t, g, 8, 1, w, accumulate=True)       # ... and so does what an accumulation could add to
    t.close()


# ----------------------------------------------------------------------------- G5
def chain_case():
    """a sphere of 5 m at 1 km that walks 0.3 m in range and a few millimetres across per pulse (ISAR: the radar stands still), seen
    through a beam 0.2 m wide around its specular point: every ray leaves the sphere within 0.06 rad of the line of sight and ends on
    the receiver's capture surface -- the cap, through the receiver's position, of a sphere of 400 m centred 400 m nearer the scene
    (rts_rx_sphere).  A ray that arrives y metres beside the receiver ends y^2 / 800 m before the receiver's plane, so the path
    lengths of one pulse spread over less than 3 m (the cap's sag at 56 m less the slant's own excess): within the range cell of the
    LFM below, 2 samples of 1.5 m of path.  The receiver's own position is therefore the one to backproject with."""
    from rts_amd import scenes as S
    spec = S.config2(subdiv=2, W=24, rx_radius=400.0)
    spec["tx"] = dict(spec["tx"], span=(0.0002, 0.0002, 0.1))
    n_p = 16
    motions = [[dict(position=(-2.4 + 0.3 * k, -0.02 + 0.003 * k, 0.0), velocity=(30.0, 0.0, 0.0))] for k in range(n_p)]
    return spec, n_p, motions


def test_image_behind_the_real_chain(rts):
    spec, n_p, motions = chain_case()
    cs, fc = spec["c"], spec["carrier"]; wl = cs / fc
    dt, nb = 5.0e-9, 128
    t0 = (2 * 992.5 - 40.0) / cs
    tr = H.gpu_tracer(rts, spec)
    tr.cube_attach(1, n_p, nb, t0, dt)
    tr.cube_set_waveform(rts.Waveform.lfm(64, 0.5, 8))
    n_recv = []
    for k in range(n_p):
        H.gpu_trace(rts, spec, tr=tr, motion=motions[k])
        tr.finalise_uniform(None, wl, 1.0, 1.0, fc, cs)
        n_recv.append(tr.received_count())
        tr.cube_render(k, "rays", cs, fc)
    assert min(n_recv) >= 20, n_recv
    # the radar (the receiver rides with the transmitter) in the target's frame, pulse by pulse
    tx_world = np.tile(np.asarray(spec["tx"]["origin"], np.float64), (n_p, 1))
    rx_world = tx_world
    frame = [dict(position=m[0]["position"]) for m in motions]
    tx_img, rx_img = rts.image_frame(tx_world, frame), rts.image_frame(rx_world, frame)[None]
    g = dict(n_x=33, n_y=5, origin=(-16.0, -4.0, 0.0), step_x=(1.0, 0.0, 0.0), step_y=(0.0, 2.0, 0.0), tx=tx_img, rx=rx_img, c=cs, fc=fc, t0=t0, dt=dt)
    tr.cube_compress()
    tr.cube_backproject(g["origin"], g["step_x"], g["step_y"], g["n_x"], g["n_y"], g["tx"], g["rx"], cs, fc, taps=8, fetch=False)      # (enqueued behind the compression: no host wait between them)
    img = tr.image()
    cube = tr.cube()
    assert np.abs(cube).max() > 0
    ref = TH.call_eval(rts, cube, g, 8, 0)
    assert_close(img, ref, "chain")
    # where the peak lies: checked on the numpy backprojection of the same cube, then on the device's image
    slow = TH.backproject_ref(cube, g, 8, 0)
    limit = 5.0 + math.hypot(1.0, 2.0)
    for name, im in (("numpy", slow), ("device", img)):
        iy, ix = np.unravel_index(int(np.argmax(np.abs(im[0]))), im[0].shape)
        x = np.asarray(g["origin"]) + ix * np.asarray(g["step_x"]) + iy * np.asarray(g["step_y"])
        print("%s peak at pixel (%d, %d) = %s, %.2f m from the sphere's centre (limit %.2f)" % (name, ix, iy, x, np.linalg.norm(x), limit))
        assert np.linalg.norm(x) <= limit, (name, ix, iy)
        assert x[0] < 0                                    # the specular point faces the radar
    tr.close()


# ----------------------------------------------------------------------------- G6
def test_error_cases_on_a_live_handle(rts):
    import torch
    from rts_amd import _lib as L
    lib = L.lib()
    q, cube, p, keep = TH.raw_case(L)
    t = rts.Tracer(8, 1)
    sentinel = complex(1.5, -2.5)
    out = torch.full((2, 2, 3), sentinel, dtype=torch.complex128, device="cuda")
    assert lib.rts_cube_backproject(t.h, C.byref(p), C.c_void_p(out.data_ptr())) == L.RTS_ERR_INVALID and b"cube" in lib.rts_last_error()      # no cube attached
    buf = to_device(cube[..., 0] + 1j * cube[..., 1])
    t.cube_attach(q.n_rx, q.n_pulses, q.n_bins, q.t0, q.dt, device_ptr=buf.data_ptr())
    for name, mutate, word in TH.bad_image_params(L):
        q, cube, p, keep = TH.raw_case(L)
        mutate(p, keep)
        assert lib.rts_cube_backproject(t.h, C.byref(p), C.c_void_p(out.data_ptr())) == L.RTS_ERR_INVALID, name
        assert word in lib.rts_last_error(), (name, lib.rts_last_error())
    q, cube, p, keep = TH.raw_case(L)
    assert lib.rts_cube_backproject(t.h, None, C.c_void_p(out.data_ptr())) == L.RTS_ERR_INVALID
    assert lib.rts_cube_backproject(t.h, C.byref(p), C.c_void_p(out.data_ptr() + 8)) == L.RTS_ERR_INVALID and b"aligned" in lib.rts_last_error()
    p.flags = L.RTS_IMAGE_ACCUMULATE
    assert lib.rts_cube_backproject(t.h, C.byref(p), None) == L.RTS_ERR_INVALID and b"ACCUMULATE" in lib.rts_last_error()       # nothing to add to
    host = np.zeros(24)
    assert lib.rts_cube_image_get(t.h, host.ctypes.data, 24) == L.RTS_ERR_INVALID
    t.cube()
    assert np.all(out.cpu().numpy() == sentinel)           # nothing was written by the refused calls
    # the valid descriptor runs, and a too small host array is refused
    p.flags = 0
    assert lib.rts_cube_backproject(t.h, C.byref(p), None) == L.RTS_OK
    assert lib.rts_cube_image_get(t.h, host.ctypes.data, 23) == L.RTS_ERR_CAPACITY
    assert lib.rts_cube_image_get(t.h, host.ctypes.data, 24) == L.RTS_OK and np.count_nonzero(host) == 24
    t.close()
    with pytest.raises(L.RtsError):
        t.image()
