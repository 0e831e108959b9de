"""The derived outputs of the return cube through the C-ABI (-m gpu): the lifetime of the Doppler map, the image and the spectrogram
(one record, RtsCubeProduct, and one copy-out behind the three getters: every product and the detection list end at
rts_cube_attach), and the staged uploads of rts_cube_spectrogram's window and rts_cube_backproject's geometry reused by a second
call while the first may still be in flight (StagedUpload, whose rules tests/test_owned_host.py has without a GPU).

Device against evaluator: the comparisons of tests/test_gpu_stft.py and tests/test_gpu_image.py, imported, not restated."""
import ctypes as C

import numpy as np
import pytest

import test_gpu_image as GI
import test_gpu_stft as GS

pytestmark = pytest.mark.gpu
CS = 299792458.0
DT = 2.0e-9


def random_cube(seed, n_rx, rows, nb):
    rng = np.random.default_rng(seed)
    return rng.standard_normal((n_rx, rows, nb)) + 1j * rng.standard_normal((n_rx, rows, nb))


def arc(P, n_x, n_y, nb=8):
    """the radar on an arc of +-5 degrees of a circle of 1 km around the pixel grid (receiver 0 rides with the transmitter, receiver 1
    two degrees on): every two-way delay is within a range cell of 2 R / c, which t0 puts on the middle bin"""
    R = 1000.0
    th = np.deg2rad(np.linspace(-5.0, 5.0, P)) if P > 1 else np.zeros(1)
    on = lambda a: np.stack([-R * np.cos(a), R * np.sin(a), np.zeros_like(a)], axis=1)
    tx = on(th)
    return dict(n_x=n_x, n_y=n_y, origin=(-0.1, -0.1, 0.0), step_x=(0.2, 0.0, 0.0), step_y=(0.0, 0.2, 0.0), tx=tx, rx=np.stack([tx, on(th + np.deg2rad(2.0))]),
                c=CS, fc=1.5e9, dt=DT, t0=2.0 * R / CS - (nb // 2) * DT)


def attach(rts, cube, t0=0.0, dt=1.0):
    buf = GS.to_device(cube)
    t = rts.Tracer(8, 1)
    t.cube_attach(cube.shape[0], cube.shape[1], cube.shape[2], t0, dt, device_ptr=buf.data_ptr())
    return t, buf


# ----------------------------------------------------------------------------- 1
def test_product_lifetimes(rts):
    """Cube 2 x 4 x 8 in a caller's tensor.  Doppler map (n_fft 4: 128 doubles), image 3 x 2 (24), spectrogram of one frame (128): the
    getter refuses before the product exists, copies with exactly the product's size, reports RTS_ERR_CAPACITY with one double
    fewer and RTS_ERR_INVALID with a null output; after rts_cube_attach of a SMALLER cube (one receiver) all three getters and
    rts_cube_detections_get refuse and rts_cube_detect without a map has none.  (Smaller on purpose: a getter that wrongly served
    the stale Doppler map, sized from the new cube's parameters, would still read inside the old allocation.)"""
    from rts_amd import _lib as L
    lib = L.lib()
    cube = random_cube(41, 2, 4, 8)
    g = arc(4, 3, 2)
    t, buf = attach(rts, cube, g["t0"], g["dt"])
    products = [
        ("doppler", lib.rts_cube_doppler_get, 2 * 2 * 4 * 8, lambda: t.cube_doppler(4, fetch=False)),
        ("image", lib.rts_cube_image_get, 2 * 2 * 2 * 3, lambda: GI.device_image(t, g, 2, 0, fetch=False)),
        ("spectrogram", lib.rts_cube_spectrogram_get, 2 * 2 * 1 * 4 * 8, lambda: t.cube_spectrogram(4, 1, 4, window=rts.window("hann", 4), fetch=False)),
    ]
    for name, get, doubles, make in products:
        host = np.full(doubles + 1, 7.5)
        assert get(t.h, host.ctypes.data, 1 << 40) == L.RTS_ERR_INVALID, name                 # no product yet
        make()
        assert get(t.h, host.ctypes.data, doubles) == L.RTS_OK, (name, lib.rts_last_error())
        assert host[doubles] == 7.5 and np.count_nonzero(host[:doubles] != 7.5) > doubles // 2, name      # exactly the product's size was written
        assert get(t.h, host.ctypes.data, doubles - 1) == L.RTS_ERR_CAPACITY, name
        assert get(t.h, None, 1 << 40) == L.RTS_ERR_INVALID, name
    t.cube_detect(guard=(1, 0), train=(2, 1), pfa=1e-3)                                        # (on the library's map: a list exists)
    n = C.c_uint32(0)
    assert lib.rts_cube_detections_get(t.h, None, 0, C.byref(n)) in (L.RTS_OK, L.RTS_ERR_CAPACITY)
    t.cube_attach(1, 4, 8, g["t0"], g["dt"], device_ptr=buf.data_ptr())
    for name, get, doubles, make in products:
        host = np.full(doubles, 7.5)
        assert get(t.h, host.ctypes.data, 1 << 40) == L.RTS_ERR_INVALID, name                 # (the Doppler row: the parent commit copied here)
        assert np.all(host == 7.5), name
    assert lib.rts_cube_detections_get(t.h, None, 0, C.byref(n)) == L.RTS_ERR_INVALID
    with pytest.raises(L.RtsError, match="map"):
        t.cube_detect(guard=(1, 0), train=(2, 1), pfa=1e-3, fetch=False)
    t.close()


# ----------------------------------------------------------------------------- 2
def test_spectrogram_window_staging_is_reused_safely(rts):
    """two windowed calls back to back, nothing between them on the host: the second call's window (4 values) goes into the staging
    the first call's (3 values) went through"""
    import torch
    cube = random_cube(42, 2, 4, 8)
    t, buf = attach(rts, cube)
    w3, w4 = np.array([0.25, 1.0, 0.5]), rts.window("hamming", 4)
    out3 = torch.zeros((2, 2, 4, 8), dtype=torch.complex128, device="cuda"); out4 = torch.zeros((2, 1, 4, 8), dtype=torch.complex128, device="cuda")
    t.cube_spectrogram(3, 1, 4, window=w3, device_ptr=out3.data_ptr())
    t.cube_spectrogram(4, 1, 4, window=w4, device_ptr=out4.data_ptr())
    t.cube()                                                                                   # (drains the handle's stream)
    GS.assert_close(out3.cpu().numpy(), rts.stft_eval(cube, 3, 1, 4, window=w3), "window of 3")
    GS.assert_close(out4.cpu().numpy(), rts.stft_eval(cube, 4, 1, 4, window=w4), "window of 4")
    t.close()


def test_backprojection_geometry_staging_is_reused_and_regrown_safely(rts):
    """two calls back to back, nothing between them on the host: 4 pulses (40 doubles of geometry, in the first pinned block of 4 096),
    then 416 pulses at two receivers: 416 (4 + 3 x 2) = 4 160 doubles, which replaces the block while the first copy may be in flight"""
    import torch
    P = 416
    assert 4 * (4 + 3 * 2) <= 4096 < P * (4 + 3 * 2)
    cube = random_cube(43, 2, P, 8)
    g = arc(P, 2, 2)
    few = dict(g, tx=g["tx"][:4], rx=g["rx"][:, :4])
    t, buf = attach(rts, cube, g["t0"], g["dt"])
    out_few = torch.zeros((2, 2, 2), dtype=torch.complex128, device="cuda"); out_all = torch.zeros((2, 2, 2), dtype=torch.complex128, device="cuda")
    GI.device_image(t, few, 8, 0, device_ptr=out_few.data_ptr())
    GI.device_image(t, g, 8, 0, GI.TH.hann(P), device_ptr=out_all.data_ptr())
    t.cube()
    ref_few = GI.TH.call_eval(rts, cube, few, 8, 0); ref_all = GI.TH.call_eval(rts, cube, g, 8, 0, GI.TH.hann(P))
    assert np.count_nonzero(ref_few) == ref_few.size and np.count_nonzero(ref_all) == ref_all.size
    GI.assert_close(out_few.cpu().numpy(), ref_few, "4 pulses")
    GI.assert_close(out_all.cpu().numpy(), ref_all, "416 pulses")
    t.close()
