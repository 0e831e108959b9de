"""The tapered slow-time spectrogram on the device (rts_cube_spectrogram, rts_cube_spectrogram_get) against the host evaluator
rts_stft_eval (itself checked against a numpy restatement in tests/test_stft_host.py): the cases of that comparison, the degenerate
case against rts_cube_doppler bit for bit, the three output forms against each other bit for bit, guarded caller-owned outputs, the
size limits, output ownership, the hand-over to rts_cube_detect, and the spectrogram behind the real chain trace -> finalise ->
accumulate.

Device against evaluator: rtol 1e-10, atol 1e-12 max|ref| -- the project's bound for a kernel against its evaluator
(tests/test_gpu_render.py, tests/test_gpu_image.py).  It applies because both sides run the same tree of rts_stft.h on the same
window bits and differ only in the two libraries' sincospi of the twiddle table, a few ulp of a term each."""
import ctypes as C

import numpy as np
import pytest

import helpers as H
import test_stft_host as TH

pytestmark = pytest.mark.gpu


def to_device(a):
    import torch
    return torch.from_numpy(np.array(a, order="C")).cuda()              # (a copy: the shared cube is read-only)


def attach(rts, cube):
    """a handle with the host cube attached as a caller-owned device tensor: (tracer, the tensor)"""
    buf = to_device(np.asarray(cube, np.complex128))
    t = rts.Tracer(8, 1)
    t.cube_attach(cube.shape[0], cube.shape[1], cube.shape[2], 0.0, 1.0, device_ptr=buf.data_ptr())
    return t, buf


def assert_close(got, ref, what=""):
    err = float(np.abs(got - ref).max())
    print("%s: max |device - evaluator| %.3g, max |evaluator| %.3g" % (what, err, np.abs(ref).max()))
    assert got.shape == ref.shape and got.dtype == ref.dtype, what
    np.testing.assert_allclose(got, ref, rtol=1e-10, atol=1e-12 * np.abs(ref).max(), err_msg=str(what))


def bits(a):
    return np.ascontiguousarray(a).view(np.float64)


@pytest.fixture(scope="module")
def cube130():
    c = TH.random_cube(2024)
    c.setflags(write=False)
    return c


# ----------------------------------------------------------------------------- G1
@pytest.mark.parametrize("window_len,hop,n_fft", TH.CASES)
def test_device_against_evaluator(rts, cube130, window_len, hop, n_fft):
    cube = cube130
    t, buf = attach(rts, cube)
    for first in (0, 3):
        for window in (None, rts.window("hann", window_len)):
            for first_bin, n_bins in TH.GATES:
                for form in TH.FORMS:
                    kw = dict(window=window, first=first, count=120, first_bin=first_bin, n_bins=n_bins, **form)
                    got = t.cube_spectrogram(window_len, hop, n_fft, **kw)
                    ref = rts.stft_eval(cube, window_len, hop, n_fft, **kw)
                    assert np.count_nonzero(ref) > ref.size // 2
                    assert_close(got, ref, (window_len, hop, n_fft, first, window is not None, first_bin, n_bins, form))
    t.close()


# ----------------------------------------------------------------------------- G2
@pytest.mark.parametrize("rows,n_fft", [(2, 2), (2, 8), (2, 64), (2, 128), (5, 8), (5, 64), (5, 128), (64, 64), (64, 128), (65, 128), (70, 4096)])
def test_degenerate_case_is_the_doppler_map(rts, rows, n_fft):
    """NULL window, one frame over all rows, all bins, complex: the same tree on the same samples as rts_cube_doppler"""
    for nb in (1, 9, 48):
        cube = TH.random_cube(rows * 100 + nb, rows=rows, nb=nb)
        t, buf = attach(rts, cube)
        want = t.cube_doppler(n_fft)
        got = t.cube_spectrogram(rows, 1, n_fft)
        assert got.shape == (2, 1, n_fft, nb)
        assert np.count_nonzero(want) == want.size
        assert np.array_equal(bits(got[:, 0]), bits(want)), (rows, n_fft, nb)
        t.close()


# ----------------------------------------------------------------------------- G3
def sum_in_header_order(p):
    """[n_rx][n_frames][n_fft][G] -> [n_rx][n_frames][n_fft]: tiles of 8 gate bins from bin 0, ascending inside a tile and then
    over the tiles, the first value the start value each time (an explicit loop: numpy's sum adds pairwise)"""
    G = p.shape[-1]
    total = None
    for g0 in range(0, G, 8):
        ts = p[..., g0].copy()
        for g in range(g0 + 1, min(g0 + 8, G)):
            ts = ts + p[..., g]
        total = ts if total is None else total + ts
    return total


@pytest.mark.parametrize("n_fft,rows", [(64, 130), (2048, 40), (4096, 40)])
def test_forms_against_each_other(rts, cube130, n_fft, rows):
    """on the device's own output, bit for bit: the power form is re re + im im of the complex form, the summed form the power
    form added in the header's order.  n_fft 2048 and 4096 hold 4 and 2 bins in LDS, so a summation tile takes 2 and 4 passes.
    Gate lengths 1, 7, 8, 9, 17 and 48 from bin 0; from bin 3 the same but 45 (to the last of the cube's 48 bins) for 48."""
    cube = cube130[:, :rows]
    t, buf = attach(rts, cube)
    w = rts.window("hann", 33)
    gates = [(fb, g) for fb in (0, 3) for g in (1, 7, 8, 9, 17, 48 - fb)] if n_fft == 64 else [(0, 9), (3, 17)]
    for first_bin, n_bins in gates:
        kw = dict(window=w, first_bin=first_bin, n_bins=n_bins)
        z = t.cube_spectrogram(33, 7, n_fft, **kw)
        p = t.cube_spectrogram(33, 7, n_fft, power=True, **kw)
        s = t.cube_spectrogram(33, 7, n_fft, power=True, sum_bins=True, **kw)
        assert z.shape == (2, 1 + (rows - 33) // 7, n_fft, n_bins) and np.count_nonzero(z) == z.size
        assert np.array_equal(p, z.real * z.real + z.imag * z.imag), (first_bin, n_bins)
        assert s.shape == z.shape[:3]
        assert np.array_equal(s, sum_in_header_order(p)), (first_bin, n_bins)
        if n_bins == 9:
            assert_close(s, rts.stft_eval(cube, 33, 7, n_fft, power=True, sum_bins=True, **kw), (n_fft, first_bin, n_bins))
    t.close()


# ----------------------------------------------------------------------------- G4
@pytest.mark.parametrize("n_frames", [1, 2])
def test_guarded_output(rts, cube130, n_frames):
    import torch
    cube = cube130[:, :40]
    t, buf = attach(rts, cube)
    sentinel, pad = -7.5e300, 64
    wl, hop, n_fft = 16, 20, 32
    count = wl + (n_frames - 1) * hop + 3
    w = rts.window("hamming", wl)
    for n_bins in (1, 7, 8, 9, 17):
        for form in TH.FORMS:
            kw = dict(window=w, first=1, count=count, first_bin=2, n_bins=n_bins, **form)
            ref = rts.stft_eval(cube, wl, hop, n_fft, **kw)
            assert ref.shape[1] == n_frames
            n = ref.size * (1 if form["power"] else 2)
            guard = torch.full((pad + n + pad,), sentinel, dtype=torch.float64, device="cuda")
            t.cube_spectrogram(wl, hop, n_fft, device_ptr=guard.data_ptr() + 8 * pad, **kw)
            t.cube()                                           # (drains the handle's stream)
            out = guard.cpu().numpy()
            assert np.all(out[:pad] == sentinel) and np.all(out[pad + n:] == sentinel), (n_bins, form)
            inner = out[pad:pad + n]
            assert not np.any(inner == sentinel), (n_bins, form)
            assert_close(inner.view(ref.dtype).reshape(ref.shape), ref, (n_frames, n_bins, form))
    t.close()


# ----------------------------------------------------------------------------- G5
def test_size_limits(rts):
    """the longest transform (two columns and the twiddle table fill the workgroup's LDS; a summation tile is walked in passes) on
    overlapping frames, and the shortest"""
    cube = TH.random_cube(41, n_rx=1, rows=4100, nb=3)
    t, buf = attach(rts, cube)
    w = rts.window("hann", 4096)
    for form in TH.FORMS:
        a = t.cube_spectrogram(4096, 2, 4096, window=w, **form)
        b = t.cube_spectrogram(4096, 2, 4096, window=w, **form)
        assert a.shape[:3] == (1, 3, 4096)
        assert np.array_equal(bits(a), bits(b)), form
        assert_close(a, rts.stft_eval(cube, 4096, 2, 4096, window=w, **form), ("4096", form))
    small = cube[:, :9]
    t2, buf2 = attach(rts, small)
    for form in TH.FORMS:
        got = t2.cube_spectrogram(1, 1, 2, window=[0.75], **form)
        assert got.shape[:3] == (1, 9, 2)
        assert_close(got, rts.stft_eval(small, 1, 1, 2, window=[0.75], **form), ("2", form))
    t.close(); t2.close()


# ----------------------------------------------------------------------------- G6
def test_output_ownership(rts, cube130):
    import torch
    from rts_amd import _lib as L
    lib = L.lib()
    cube = cube130
    t, buf = attach(rts, cube)
    w = rts.window("blackman", 33)
    host = np.zeros(16)
    assert lib.rts_cube_spectrogram_get(t.h, host.ctypes.data, 16) == L.RTS_ERR_INVALID        # no spectrogram yet
    mine = torch.zeros((2, 14, 64, 48), dtype=torch.complex128, device="cuda")
    assert t.cube_spectrogram(33, 7, 64, window=w, device_ptr=mine.data_ptr()) is None
    assert lib.rts_cube_spectrogram_get(t.h, host.ctypes.data, 16) == L.RTS_ERR_INVALID        # a caller-owned output is not the library's
    owned = t.cube_spectrogram(33, 7, 64, window=w)
    assert np.array_equal(bits(owned), bits(mine.cpu().numpy()))
    assert np.array_equal(bits(t.spectrogram()), bits(owned))
    small = np.zeros(owned.size * 2 - 1)
    assert lib.rts_cube_spectrogram_get(t.h, small.ctypes.data, small.size) == L.RTS_ERR_CAPACITY
    assert lib.rts_cube_spectrogram_get(t.h, None, 1 << 40) == L.RTS_ERR_INVALID
    assert not np.any(small)
    # a second call of another size reallocates (larger), and a smaller one after it is served from the same storage
    big = t.cube_spectrogram(64, 1, 128, window=None)
    assert big.shape == (2, 67, 128, 48) and big.size > owned.size
    assert_close(big, rts.stft_eval(cube, 64, 1, 128), "regrown")
    again = t.cube_spectrogram(33, 7, 64, window=w)
    assert np.array_equal(bits(again), bits(owned))
    # misaligned caller memory is refused; a spectrogram ends at rts_cube_attach
    p, keep = rts._stft_params(33, 7, 64, w, 0, None, 0, 0, False, False, 130)
    assert lib.rts_cube_spectrogram(t.h, C.byref(p), C.c_void_p(mine.data_ptr() + 8), None) == L.RTS_ERR_INVALID and b"aligned" in lib.rts_last_error()
    t.cube_attach(2, 130, 48, 0.0, 1.0, device_ptr=buf.data_ptr())
    with pytest.raises(L.RtsError):
        t.spectrogram()
    assert lib.rts_cube_spectrogram_get(t.h, host.ctypes.data, 1 << 40) == L.RTS_ERR_INVALID
    t.close()


def test_error_cases_on_a_live_handle(rts):
    import torch
    from rts_amd import _lib as L
    lib = L.lib()
    q, cube, p, keep = TH.raw_case(L)
    t = rts.Tracer(8, 1)
    sentinel = complex(1.5, -2.5)
    out = torch.full((2, 3, 8, 4), sentinel, dtype=torch.complex128, device="cuda")
    nf = C.c_uint32(99)
    assert lib.rts_cube_spectrogram(t.h, C.byref(p), C.c_void_p(out.data_ptr()), C.byref(nf)) == L.RTS_ERR_INVALID and b"cube" in lib.rts_last_error()
    buf = to_device(cube[..., 0] + 1j * cube[..., 1])
    t.cube_attach(q.n_rx, q.n_pulses, q.n_bins, 0.0, 1.0, device_ptr=buf.data_ptr())
    for name, mutate, word in TH.bad_stft_params(L):
        q, cube, p, keep = TH.raw_case(L)
        mutate(p, keep)
        assert lib.rts_cube_spectrogram(t.h, C.byref(p), C.c_void_p(out.data_ptr()), C.byref(nf)) == L.RTS_ERR_INVALID, name
        assert word in lib.rts_last_error(), (name, lib.rts_last_error())
    assert lib.rts_cube_spectrogram(t.h, None, C.c_void_p(out.data_ptr()), C.byref(nf)) == L.RTS_ERR_INVALID
    t.cube()
    assert np.all(out.cpu().numpy() == sentinel) and nf.value == 99          # nothing was written by the refused calls
    q, cube, p, keep = TH.raw_case(L)
    assert lib.rts_cube_spectrogram(t.h, C.byref(p), C.c_void_p(out.data_ptr()), C.byref(nf)) == L.RTS_OK and nf.value == 3
    t.cube()
    assert not np.any(out.cpu().numpy() == sentinel)
    t.close()


# ----------------------------------------------------------------------------- G7
def test_into_the_detector(rts):
    """the single-frame NULL-window map, in caller memory, is a device_map of rts_cube_detect: the same detections as from
    rts_cube_doppler's own map of the same cube (a few planted scatterers in receiver noise)"""
    import torch
    n_rx, n_p, nb = 2, 32, 48
    rng = np.random.default_rng(17)
    cube = np.zeros((n_rx, n_p, nb), np.complex128)
    i = np.arange(n_p)
    planted = [(0, 7.0, 11), (0, 20.5, 30), (1, 3.0, 40), (1, 27.0, 5)]
    for r, k, b in planted:
        cube[r, :, b] += 6.0 * np.exp(2j * np.pi * (k * i / n_p + rng.random()))
    t, buf = attach(rts, cube)
    t.cube_add_noise(1.0, 4242)
    t.cube_doppler(n_p, fetch=False)
    det = dict(guard=(1, 1), train=(4, 4), mode="ca", pfa=1e-4, local_max=True, pri=1e-3)
    want = t.cube_detect(**det)
    m = torch.zeros((n_rx, 1, n_p, nb), dtype=torch.complex128, device="cuda")
    t.cube_spectrogram(n_p, 1, n_p, device_ptr=m.data_ptr())
    got = t.cube_detect(device_ptr=m.data_ptr(), n_doppler=n_p, **det)
    assert len(want) >= len(planted)
    for r, k, b in planted:
        assert np.any((want["rx"] == r) & (want["range_bin"] == b) & (np.abs(want["doppler_bin"] - k) <= 1)), (r, k, b)
    assert got.tobytes() == want.tobytes()
    t.close()


def test_masking_on_the_device(rts):
    """the masking cube of tests/test_stft_host.py: the strong tone's leak at row 29 against the weak tone's power there, above 100
    under the rectangular window, below 0.1 under the Blackman taper"""
    strong, weak = TH.masking_cubes()
    ts, bs = attach(rts, strong)
    tw, bw = attach(rts, weak)
    for window, check in ((None, lambda r: r > 100), (rts.window("blackman", 64), lambda r: r < 0.1)):
        ps = ts.cube_spectrogram(64, 1, 64, window=window, power=True)[0, 0, :, 0]
        pw = tw.cube_spectrogram(64, 1, 64, window=window, power=True)[0, 0, :, 0]
        print("window %s: leak / weak at row 29 = %.4g" % (window is not None, ps[29] / pw[29]))
        assert check(ps[29] / pw[29])
    tb, bb = attach(rts, strong + weak)
    both = tb.cube_spectrogram(64, 1, 64, window=rts.window("blackman", 64), power=True)[0, 0, :, 0]
    assert both[29] > both[28] and both[29] > both[30]
    ts.close(); tw.close(); tb.close()


# ----------------------------------------------------------------------------- G8
def chain_case(rts, n_p=64):
    """a sphere of 4 m whose centre sits 6 m off the target's axis of rotation, turning 0.4 mrad per pulse about z, 200 m from the
    radar: its centre circles the axis, so its range -- and with it the Doppler -- changes from pulse to pulse"""
    from rts_amd import scenes as S
    spec = S.config_multi(W=16, max_refl=1)
    m = dict(spec["meshes"][0])
    m["verts"] = np.asarray(m["verts"], np.float64) + np.array([0.0, 6.0, 0.0])
    spec["meshes"], spec["motion"] = [m], spec["motion"][:1]
    motions = [[dict(position=(0.0, 0.0, 0.0), velocity=(0.0, 0.0, 0.0), rotation=rts.rotation_matrix(4.0e-4 * k, 0.0, 0.0))] for k in range(n_p)]
    return spec, motions


def test_spectrogram_behind_the_real_chain(rts):
    spec, motions = chain_case(rts)
    cs, fc = spec["c"], spec["carrier"]; wl = cs / fc
    n_rx, n_p, nb = len(spec["rx"]), len(motions), 224
    t0, dt = 1.1e-6, 5.0e-9
    tr = H.gpu_tracer(rts, spec)
    tr.cube_attach(n_rx, n_p, nb, t0, dt)
    n_recv = []
    for k in range(n_p):
        H.gpu_trace(rts, spec, tr=tr, motion=motions[k])
        tr.finalise_uniform(None, wl, 1.0, 1.0, fc, cs)
        n_recv.append(tr.received_count())
        tr.cube_accumulate(k, cs, fc)
    assert min(n_recv) >= 5, n_recv
    w = rts.window("hann", 16)
    tr.cube_spectrogram(16, 8, 32, window=w, fetch=False)          # (enqueued behind the accumulation: no host wait between them)
    z = tr.spectrogram()
    cube = tr.cube()
    assert z.shape == (n_rx, 7, 32, nb)
    assert_close(z, rts.stft_eval(cube, 16, 8, 32, window=w), "chain")
    # the gate that holds the target: the bins any pulse of receiver 0 wrote
    lit = np.flatnonzero(np.abs(cube[0]).max(axis=0) > 0)
    assert len(lit) >= 1
    lo, n_gate = int(lit[0]), int(lit[-1] - lit[0] + 1)
    ridge = tr.cube_spectrogram(16, 8, 32, window=w, first_bin=lo, n_bins=n_gate, power=True, sum_bins=True)
    assert_close(ridge, rts.stft_eval(cube, 16, 8, 32, window=w, first_bin=lo, n_bins=n_gate, power=True, sum_bins=True), "ridge")
    centres, doppler = rts.spectrogram_axes(16, 8, 32, n_p, 1.0)
    peak = np.argmax(ridge[0], axis=1)
    print("gate bins %d .. %d; peak rows per frame %s (cycles per pulse %s)" % (lo, lo + n_gate - 1, peak, doppler[peak]))
    assert np.all(ridge[0].max(axis=1) > 0)                        # a ridge in every frame
    tr.close()
