"""Adaptive (MVDR) beamforming on the device (rts_cube_covariance, rts_cube_mvdr): the kernels against the host evaluators
rts_covariance_eval / rts_mvdr_eval BIT FOR BIT (the trees hold + - * / and sqrt only) over the smallest shapes at which they can go
wrong -- one cell, the tile and the parts cap of include/rts_amd.h at their edges, the per-thread entry block and the solve's
workgroup of rts_amd/csrc/rts_adapt.h at B - 1, B, B + 1, the limits of receivers and beams, the skip interval at each edge, the three
sources; sentinel cells around caller-owned outputs; run-to-run equality; the failed solve; the whole chain of tests/adapt_ref.py
against its host run with the MVDR properties on the device's weights; and the error / lifetime rules on a live handle."""
import ctypes as C
import math

import numpy as np
import pytest

import adapt_ref as A
import beam_ref as B

pytestmark = pytest.mark.gpu
TILE, PARTS, BLK, MT = A.TILE, A.MAX_PARTS, A.BLOCK, A.SOLVE_THREADS


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


def attached(rts, inp):
    """a handle with the host array [n_rx][rows][n_bins] attached as its cube: (handle, the device tensor)"""
    d = dev(inp)
    tr = rts.Tracer(8, 1)
    tr.cube_attach(inp.shape[0], inp.shape[1], inp.shape[2], 0.0, 1.0, device_ptr=d.data_ptr())
    return tr, d


# ----------------------------------------------------------------------------- 1. the covariance against the evaluator
COV_SHAPES = [(n_rx, K) for K in (1, TILE - 1, TILE, TILE + 1) for n_rx in (1, 3)] + \
             [(2, TILE * (PARTS - 1)), (2, TILE * PARTS), (2, TILE * (PARTS + 1) - 7)] + \
             [(n_rx, 2 * TILE + 3) for n_rx in (2, BLK - 1 or 1, BLK, BLK + 1, 2 * BLK + 1, 21, 63, 64)]


@pytest.mark.parametrize("n_rx,K", sorted(set(COV_SHAPES)))
def test_covariance_against_the_evaluator(rts, n_rx, K):
    rng = np.random.default_rng(n_rx * 100003 + K)
    rows, bins = A.shape_for(K)
    inp = B.random_complex(rng, (n_rx, rows + 2, bins)); inp[:, 0] = np.nan; inp[:, -1] = np.nan       # rows outside the span: never read
    tr, d = attached(rts, inp)
    got = tr.cube_covariance(first=1, count=rows)
    want = rts.covariance_eval(inp, first=1, count=rows)
    assert got.shape == (n_rx, n_rx) and np.all(np.isfinite(bits(got)))
    assert np.array_equal(bits(got), bits(want)), (n_rx, K)
    tr.close()


@pytest.mark.parametrize("skip", [None, (2, 3), (13, 4), (3, 1), (2, 14), (3, 14)], ids=["none", "first", "last", "one", "leaves-last", "leaves-first"])
def test_covariance_skip_interval(rts, skip):
    rng = np.random.default_rng(99)
    inp = B.random_complex(rng, (5, 40, 19)); inp[:, 0] = np.nan; inp[:, 39] = np.nan; inp[:, :, :2] = np.nan; inp[:, :, 17:] = np.nan
    if skip:
        inp[:, :, skip[0]:skip[0] + skip[1]] = np.nan                              # the skipped bins are never read
    train = dict(first=1, count=38, first_bin=2, n_bins=15, skip=skip)             # 38 rows: several tiles, cells that cross rows inside a tile
    tr, d = attached(rts, inp)
    got = tr.cube_covariance(**train)
    assert np.all(np.isfinite(bits(got))) and np.array_equal(bits(got), bits(rts.covariance_eval(inp, **train)))
    tr.close()


def test_covariance_three_sources(rts):
    rng = np.random.default_rng(23)
    n_rx, n_p, nb, n_fft = 3, 6, 37, 8
    inp = B.random_complex(rng, (n_rx, n_p, nb))
    tr, d = attached(rts, inp)
    dmap = tr.cube_doppler(n_fft)                                                  # library-owned
    train = dict(first=1, count=5, first_bin=3, skip=(10, 4))
    from_map = tr.cube_covariance(source="map", **train)
    dm = dev(dmap)
    from_ptr = tr.cube_covariance(source="pointer", device_in=dm.data_ptr(), n_rows_in=n_fft, **train)
    assert np.array_equal(bits(from_map), bits(from_ptr)) and np.array_equal(bits(from_map), bits(rts.covariance_eval(dmap, **train)))
    assert np.array_equal(bits(tr.cube_covariance(source="map")), bits(rts.covariance_eval(dmap)))                          # every cell of the map
    from_cube = tr.cube_covariance(first=2, count=3)
    again = tr.cube_covariance(source="pointer", device_in=d.data_ptr(), n_rows_in=n_p, first=2, count=3)
    assert np.array_equal(bits(from_cube), bits(again)) and np.array_equal(bits(from_cube), bits(rts.covariance_eval(inp, first=2, count=3)))
    other = B.random_complex(rng, (n_rx, 2, nb)); do = dev(other)                  # a pointer source of other rows than the cube's
    assert np.array_equal(bits(tr.cube_covariance(source="pointer", device_in=do.data_ptr(), n_rows_in=2)), bits(rts.covariance_eval(other)))
    tr.close()


# ----------------------------------------------------------------------------- 2. the solve against the evaluator
MVDR_SHAPES = [(n_rx, 3) for n_rx in (1, 2, 3, 63, 64)] + [(5, n) for n in (1, MT - 1, MT, MT + 1)] + [(4, 1024), (64, 64)]


@pytest.mark.parametrize("loading", [0.0, 0.75])
@pytest.mark.parametrize("n_rx,n_beams", MVDR_SHAPES)
def test_mvdr_against_the_evaluator(rts, n_rx, n_beams, loading):
    rng = np.random.default_rng(n_rx * 1009 + n_beams)
    cov = A.hermitian_pd(rng, n_rx); s = B.random_complex(rng, (n_beams, n_rx))
    dc = dev(cov)
    tr = rts.Tracer(8, 1); tr.cube_attach(n_rx, 1, 1, 0.0, 1.0)
    got = tr.cube_mvdr(s, loading, device_cov=dc.data_ptr())
    want = rts.mvdr_eval(cov, s, loading)
    assert got.shape == (n_beams, n_rx) and np.all(np.isfinite(bits(got)))
    assert np.array_equal(bits(got), bits(want)), (n_rx, n_beams, loading)
    tr.close()


# ----------------------------------------------------------------------------- 3. caller-owned outputs, run to run
def test_sentinels_and_owned_outputs(rts):
    import torch
    rng = np.random.default_rng(17)
    n_rx, n_beams, PAD = 5, MT + 1, 16
    inp = B.random_complex(rng, (n_rx, 4, 67)); s = B.random_complex(rng, (n_beams, n_rx))
    train = dict(first=1, count=2, skip=(30, 5))
    cov_h = rts.covariance_eval(inp, **train); w_h = rts.mvdr_eval(cov_h, s, 0.25)
    tr, d = attached(rts, inp)
    cbuf = filled(n_rx * n_rx + 2 * PAD, complex(7.25, -3.5), torch.complex128)
    wbuf = filled(n_beams * n_rx + 2 * PAD, complex(7.25, -3.5), torch.complex128)
    assert tr.cube_covariance(device_ptr=cbuf.data_ptr() + 16 * PAD, **train) is None
    assert tr.cube_mvdr(s, 0.25, device_cov=cbuf.data_ptr() + 16 * PAD, device_ptr=wbuf.data_ptr() + 16 * PAD) is None
    tr.cube()                                                                    # (the handle's stream drained)
    for buf, want in ((host(cbuf), cov_h), (host(wbuf), w_h)):
        assert np.all(buf[:PAD] == complex(7.25, -3.5)) and np.all(buf[-PAD:] == complex(7.25, -3.5))
        assert np.array_equal(bits(buf[PAD:-PAD].reshape(want.shape)), bits(want))
    # the library-owned outputs hold the same bits, from the library-owned covariance too; a caller-owned run is not recorded
    assert np.array_equal(bits(tr.cube_covariance(**train)), bits(cov_h)) and np.array_equal(bits(tr.covariance()), bits(cov_h))
    assert np.array_equal(bits(tr.cube_mvdr(s, 0.25)), bits(w_h)) and np.array_equal(bits(tr.mvdr_weights()), bits(w_h))
    tr.cube_covariance(device_ptr=cbuf.data_ptr() + 16 * PAD, first=3, count=1)
    assert np.array_equal(bits(tr.covariance()), bits(cov_h))
    assert np.array_equal(bits(host(d)), bits(inp))                              # the input is only read
    tr.close()


def test_run_to_run(rts):
    rng = np.random.default_rng(31)
    inp = B.random_complex(rng, (2 * BLK + 1, 3, TILE * (PARTS + 2) // 3 + 5)); s = B.random_complex(rng, (MT + 3, 2 * BLK + 1))
    runs = []
    for _ in range(2):
        tr, d = attached(rts, inp)
        for _ in range(2):
            cov = tr.cube_covariance(skip=(7, 9))
            runs.append((cov.tobytes(), tr.cube_mvdr(s, 0.5).tobytes()))
        tr.close()
    assert runs[0] == runs[1] == runs[2] == runs[3]
    assert runs[0][0] == rts.covariance_eval(inp, skip=(7, 9)).tobytes()


# ----------------------------------------------------------------------------- 4. the failed solve
def test_failed_solve(rts):
    from rts_amd import _lib as L
    lib = L.lib()
    bad = dev(np.array([[1.0, 2.0], [2.0, 1.0]])); s = np.ones((3, 2), np.complex128)
    tr = rts.Tracer(8, 1); tr.cube_attach(2, 1, 4, 0.0, 1.0)
    p = L.RtsMvdrParams(); p.n_beams, p.n_rx, p.steering, p.device_cov = 3, 2, s.ctypes.data, bad.data_ptr()
    assert lib.rts_cube_mvdr(tr.h, C.byref(p), None) == L.RTS_OK                 # enqueued; the failure is the device's to find
    out = np.full(12, 7.25)
    assert lib.rts_cube_mvdr_get(tr.h, out.ctypes.data, out.size) == L.RTS_ERR_INVALID and b"pivot 1" in lib.rts_last_error()
    assert np.all(out == 7.25)
    import torch
    wbuf = filled(6, 0j, torch.complex128)
    assert lib.rts_cube_mvdr(tr.h, C.byref(p), C.c_void_p(wbuf.data_ptr())) == L.RTS_OK
    tr.cube()
    assert np.all(np.isnan(bits(host(wbuf))))                                    # every weight NaN
    # the handle remains usable: the same matrix loaded is positive definite
    got = tr.cube_mvdr(s, 1.5, device_cov=bad.data_ptr())
    assert np.array_equal(bits(got), bits(rts.mvdr_eval(np.array([[1.0, 2.0], [2.0, 1.0]]), s, 1.5)))
    tr.close()


# ----------------------------------------------------------------------------- 5. the whole chain
def test_whole_chain(rts):
    """tests/adapt_ref.py's scene on the device: noise, the covariance without the target's bins, the weights, the beams.  Against
    the host chain run on the device's own noisy cube, bit for bit in the complex form; the properties hold on the device's weights"""
    sc = A.SCENE
    pos, directions, fc = A.scene_geometry()
    tr, d = attached(rts, A.scene_clean_cube())
    tr.cube_add_noise(sc["noise_power"], sc["seed"])
    s = rts.steering(pos, directions, sc["wavelength"])
    beams = tr.cube_adaptive_beamform(s, train=dict(skip=sc["skip"]), loading=sc["noise_power"])
    noisy = tr.cube()
    cube_h = A.scene_host(rts)[0]
    np.testing.assert_allclose(noisy, cube_h, rtol=1e-10, atol=1e-12 * np.abs(cube_h).max())
    cov_h = rts.covariance_eval(noisy, skip=sc["skip"]); w_h = rts.mvdr_eval(cov_h, s, sc["noise_power"])
    assert np.array_equal(bits(tr.covariance()), bits(cov_h)) and np.array_equal(bits(tr.mvdr_weights()), bits(w_h))
    assert beams.shape == (len(s), sc["n_pulses"], sc["n_bins"]) and np.array_equal(bits(beams), bits(rts.beamform_eval(noisy, w_h)))
    sj = rts.steering(pos, [[sc["jammer_az"], 0.0]], sc["wavelength"])[0]
    A.assert_mvdr_properties(tr.mvdr_weights(), s, tr.covariance(), sc["noise_power"], sj, sc["jammer_beam"])
    # the other forms of the beamformer pass through
    power = tr.cube_adaptive_beamform(s, train=dict(skip=sc["skip"]), loading=sc["noise_power"], power=True, first=2, count=3)
    assert np.array_equal(power, B.power_restated(beams[:, 2:5]))
    tr.close()


# ----------------------------------------------------------------------------- 6. errors and lifetime
def test_errors_and_lifetime(rts):
    from rts_amd import _lib as L
    import torch
    lib = L.lib()
    rng = np.random.default_rng(37)
    n_rx, n_p, nb = 3, 4, 40
    inp = B.random_complex(rng, (n_rx, n_p, nb)); s = np.ascontiguousarray(B.random_complex(rng, (2, n_rx)))
    out = np.full(2 * n_rx * n_rx + 2, 7.25)

    def cparams(**kw):
        p = L.RtsCovParams()
        for k, v in kw.items():
            setattr(p, k, v)
        return p

    def mparams(**kw):
        p = L.RtsMvdrParams(); p.n_beams, p.steering = 2, s.ctypes.data
        for k, v in kw.items():
            setattr(p, k, v)
        return p
    tr = rts.Tracer(8, 1)
    assert lib.rts_cube_covariance(tr.h, C.byref(cparams()), None) == L.RTS_ERR_INVALID and b"attach" in lib.rts_last_error()      # no cube
    assert lib.rts_cube_mvdr(tr.h, C.byref(mparams()), None) == L.RTS_ERR_INVALID and b"attach" in lib.rts_last_error()
    assert lib.rts_cube_covariance_get(tr.h, out.ctypes.data, out.size) == L.RTS_ERR_INVALID
    d = dev(inp)
    tr.cube_attach(n_rx, n_p, nb, 0.0, 1.0, device_ptr=d.data_ptr())
    assert lib.rts_cube_covariance_get(tr.h, out.ctypes.data, out.size) == L.RTS_ERR_INVALID and b"covariance" in lib.rts_last_error()
    assert lib.rts_cube_mvdr_get(tr.h, out.ctypes.data, out.size) == L.RTS_ERR_INVALID and b"weights" in lib.rts_last_error()
    assert lib.rts_cube_mvdr(tr.h, C.byref(mparams()), None) == L.RTS_ERR_INVALID and b"no covariance" in lib.rts_last_error()
    first = tr.cube_covariance()                                                 # library-owned products the refusals must leave alone
    w_first = tr.cube_mvdr(s, 0.5)
    assert np.array_equal(bits(first), bits(rts.covariance_eval(inp))) and np.array_equal(bits(w_first), bits(rts.mvdr_eval(first, s, 0.5)))
    caller = filled(n_rx * n_rx + 1, 0j, torch.complex128)
    other = dev(B.random_complex(rng, (n_rx, 2, nb)))
    res1 = cparams(); res1.reserved[1] = 1
    cov_cases = [("null p", None, None, b"null"), ("reserved", res1, None, b"reserved"), ("source", cparams(source=3), None, b"source"),
                 ("no map", cparams(source=L.RTS_BEAM_FROM_MAP), None, b"RTS_BEAM_FROM_MAP"),
                 ("pointer null", cparams(source=L.RTS_BEAM_FROM_POINTER, n_rows_in=2), None, b"device_in"),
                 ("pointer misaligned", cparams(source=L.RTS_BEAM_FROM_POINTER, n_rows_in=1, device_in=other.data_ptr() + 8), None, b"device_in"),
                 ("pointer without rows", cparams(source=L.RTS_BEAM_FROM_POINTER, device_in=other.data_ptr()), None, b"n_rows_in"),
                 ("n_rows_in with the cube", cparams(n_rows_in=2), None, b"n_rows_in"), ("device_in with the cube", cparams(device_in=other.data_ptr()), None, b"device_in"),
                 ("first_row beyond", cparams(first_row=n_p), None, b"first_row"), ("rows beyond", cparams(first_row=2, n_rows=3), None, b"n_rows"),
                 ("bins beyond", cparams(first_bin=30, n_bins=11), None, b"n_bins"), ("skip outside", cparams(first_bin=5, skip_first_bin=4, skip_n_bins=2), None, b"skip_first_bin"),
                 ("skip leaves nothing", cparams(skip_n_bins=nb), None, b"leaves no bin"),
                 ("device_out misaligned", cparams(), caller.data_ptr() + 8, b"device_out"),
                 ("in place", cparams(), d.data_ptr(), b"overlaps"),
                 ("overlapping the last receiver's last cell", cparams(first_row=3, n_rows=1), d.data_ptr() + 16 * (3 * n_p * nb - 1), b"overlaps")]
    for name, p, device_out, word in cov_cases:
        rc = lib.rts_cube_covariance(tr.h, C.byref(p) if p is not None else None, C.c_void_p(device_out) if device_out else None)
        assert rc == L.RTS_ERR_INVALID, name
        assert word in lib.rts_last_error(), (name, lib.rts_last_error())
    bad_s = s.copy(); bad_s[1, 2] = complex(1.0, math.inf)
    many = np.ones((1025, n_rx), np.complex128)
    mres = mparams(); mres.reserved[0] = 1
    wcaller = filled(2 * n_rx + 1, 0j, torch.complex128)
    mvdr_cases = [("null p", None, None, b"null"), ("reserved", mres, None, b"reserved"), ("no beams", mparams(n_beams=0), None, b"n_beams"),
                  ("too many beams", mparams(n_beams=1025, steering=many.ctypes.data), None, b"n_beams"), ("null steering", mparams(steering=None), None, b"steering"),
                  ("steering inf", mparams(steering=bad_s.ctypes.data), None, b"steering"), ("loading < 0", mparams(loading=-1.0), None, b"loading"),
                  ("loading nan", mparams(loading=math.nan), None, b"loading"), ("other n_rx", mparams(n_rx=2), None, b"n_rx"),
                  ("device_cov without n_rx", mparams(device_cov=caller.data_ptr()), None, b"n_rx"),
                  ("device_cov misaligned", mparams(device_cov=caller.data_ptr() + 8, n_rx=n_rx), None, b"device_cov"),
                  ("device_out misaligned", mparams(), wcaller.data_ptr() + 8, b"device_out"),
                  ("in place", mparams(device_cov=caller.data_ptr(), n_rx=n_rx), caller.data_ptr() + 16 * 4, b"overlaps")]
    for name, p, device_out, word in mvdr_cases:
        rc = lib.rts_cube_mvdr(tr.h, C.byref(p) if p is not None else None, C.c_void_p(device_out) if device_out else None)
        assert rc == L.RTS_ERR_INVALID, name
        assert word in lib.rts_last_error(), (name, lib.rts_last_error())
    # the previous products are still there, and readable; nothing was written
    assert np.array_equal(bits(tr.covariance()), bits(first)) and np.array_equal(bits(tr.mvdr_weights()), bits(w_first))
    assert np.array_equal(bits(host(d)), bits(inp)) and np.count_nonzero(host(caller)) == 0 and np.count_nonzero(host(wcaller)) == 0
    # limits that need a cube of their own: 65 receivers
    tb = rts.Tracer(8, 1); tb.cube_attach(65, 1, 1, 0.0, 1.0)
    assert lib.rts_cube_covariance(tb.h, C.byref(cparams()), None) == L.RTS_ERR_INVALID and b"n_rx" in lib.rts_last_error()
    tb.close()
    # capacity; a NULL output; the exact capacity
    assert lib.rts_cube_covariance_get(tr.h, out.ctypes.data, 2 * n_rx * n_rx - 1) == L.RTS_ERR_CAPACITY and np.all(out == 7.25)
    assert lib.rts_cube_mvdr_get(tr.h, out.ctypes.data, 2 * 2 * n_rx - 1) == L.RTS_ERR_CAPACITY and np.all(out == 7.25)
    assert lib.rts_cube_covariance_get(tr.h, None, out.size) == L.RTS_ERR_INVALID and lib.rts_cube_mvdr_get(tr.h, None, out.size) == L.RTS_ERR_INVALID
    assert lib.rts_cube_covariance_get(tr.h, out.ctypes.data, out.size) == L.RTS_OK and out[-1] == 7.25 and out[-2] == 7.25
    assert np.array_equal(out[:-2], bits(first).ravel())
    # a failed caller-owned solve does not change what the library-owned weights report
    badc = dev(np.array([[1.0, 2.0, 0], [2.0, 1.0, 0], [0, 0, 1.0]]))
    assert lib.rts_cube_mvdr(tr.h, C.byref(mparams(device_cov=badc.data_ptr(), n_rx=n_rx)), C.c_void_p(wcaller.data_ptr())) == L.RTS_OK
    assert np.array_equal(bits(tr.mvdr_weights()), bits(w_first))
    # the products end at rts_cube_attach
    tr.cube_attach(n_rx, n_p, nb, 0.0, 1.0, device_ptr=d.data_ptr())
    assert lib.rts_cube_covariance_get(tr.h, out.ctypes.data, out.size) == L.RTS_ERR_INVALID and b"rts_cube_attach" in lib.rts_last_error()
    assert lib.rts_cube_mvdr_get(tr.h, out.ctypes.data, out.size) == L.RTS_ERR_INVALID and b"rts_cube_attach" in lib.rts_last_error()
    assert lib.rts_cube_mvdr(tr.h, C.byref(mparams()), None) == L.RTS_ERR_INVALID and b"no covariance" in lib.rts_last_error()
    tr.close()
    for call in (lambda: tr.cube_covariance(), lambda: tr.covariance(), lambda: tr.cube_mvdr(s), lambda: tr.mvdr_weights()):
        with pytest.raises(L.RtsError):
            call()


def test_output_right_behind_the_last_cell_read(rts):
    """the accepted neighbour of the covariance's two overlap refusals of test_errors_and_lifetime: the caller's output starts at the first
    byte behind the last receiver's last training cell, inside the cube's own allocation: RTS_OK, the library-owned call's bytes, the
    sentinel behind it and the cube untouched"""
    from rts_amd import _lib as L
    import torch
    lib = L.lib()
    rng = np.random.default_rng(41)
    n_rx, n_p, nb = 3, 4, 7
    inp = B.random_complex(rng, (n_rx, n_p, nb))
    block = torch.empty(inp.size + n_rx * n_rx + 1, dtype=torch.complex128, device="cuda")      # ONE allocation: [the cube | the caller's output | a sentinel]
    block[:inp.size] = torch.from_numpy(inp.ravel()); block[inp.size:] = complex(7.25, -7.25)
    torch.cuda.synchronize()
    tr = rts.Tracer(8, 1)
    tr.cube_attach(n_rx, n_p, nb, 0.0, 1.0, device_ptr=block.data_ptr())
    owned = tr.cube_covariance()
    p = L.RtsCovParams()
    assert lib.rts_cube_covariance(tr.h, C.byref(p), C.c_void_p(block.data_ptr() + 16 * inp.size)) == L.RTS_OK, lib.rts_last_error()
    tr.cube()                                                                    # (drains the handle's stream)
    after = host(block)
    assert np.array_equal(bits(after[inp.size:-1]), bits(np.asarray(owned).ravel()))
    assert after[-1] == complex(7.25, -7.25) and np.array_equal(bits(after[:inp.size]), bits(inp.ravel()))
    tr.close()
