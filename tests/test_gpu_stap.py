"""Space-time adaptive processing on the device (rts_cube_st_covariance, rts_cube_st_apply): the kernels against the host evaluators
rts_st_covariance_eval / rts_st_apply_eval BIT FOR BIT (the trees hold + - * / only) over the smallest shapes at which they can go
wrong -- the covariance's tile and parts cap at their edges with stacked rows, one snapshot row, cells that cross rows inside a tile,
the skip interval at each edge; every tap count of the filter with as many rows as taps and one more, the strip, the wave, the
filter tile and the receiver tile of rts_amd/csrc/rts_stap.h at their edges, D = 64 both ways, the power form; the three sources;
NaN wherever nothing may be read; sentinel cells around a caller-owned output; run-to-run equality; n_taps = 1 against
rts_cube_covariance / rts_cube_beamform; the lifetime and error rules on a live handle; and the whole chain of tests/stap_ref.py
against its host run, its output attached to a second handle for the Doppler map."""
import ctypes as C
import math

import numpy as np
import pytest

import adapt_ref as A
import beam_ref as B
import stap_ref as S

pytestmark = pytest.mark.gpu
TILE, PARTS, STRIP, RXT = S.TILE, S.MAX_PARTS, S.STRIP, S.RX_TILE


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


def framed(rng, N, rows, bins):
    """a random input whose first and last row are NaN: the span is rows 1 .. rows"""
    inp = B.random_complex(rng, (N, rows + 2, bins)); inp[:, 0] = np.nan; inp[:, -1] = np.nan
    return inp


# ----------------------------------------------------------------------------- 1. the covariance against the evaluator
COV_SHAPES = [(N, M, 2 * TILE + 3) for (N, M) in ((1, 1), (1, 2), (3, 2), (2, 16), (4, 16), (8, 8), (21, 3), (63, 1))] + \
             [(3, 2, K) for K in (1, TILE - 1, TILE, TILE + 1)] + \
             [(1, 2, K) for K in (TILE * (PARTS - 1), TILE * PARTS, TILE * (PARTS + 1) - 7)]


@pytest.mark.parametrize("N,M,K", COV_SHAPES)
def test_covariance_against_the_evaluator(rts, N, M, K):
    rng = np.random.default_rng(N * 100003 + M * 1009 + K)
    srows, bins = A.shape_for(K)
    rows = srows + M - 1
    inp = framed(rng, N, rows, bins)
    tr, d = attached(rts, inp)
    got = tr.cube_st_covariance(M, first=1, count=rows)
    want = rts.st_covariance_eval(inp, M, first=1, count=rows)
    assert got.shape == (N * M, N * M) and np.all(np.isfinite(bits(got)))
    assert np.array_equal(bits(got), bits(want)), (N, M, K)
    tr.close()


@pytest.mark.parametrize("skip", [None, (2, 3), (13, 4), (3, 1), (2, 14), (3, 14)], ids=["none", "first", "last", "one", "leaves-last", "leaves-first"])
def test_covariance_skip_interval(rts, skip):
    """15 bins of 19 (less the skipped ones) in 38 snapshot rows: several tiles, cells that cross rows inside a tile; NaN in every row
    and bin outside the span and in the skipped bins"""
    rng = np.random.default_rng(99)
    inp = B.random_complex(rng, (3, 42, 19)); inp[:, 0] = np.nan; inp[:, 41] = np.nan; inp[:, :, :2] = np.nan; inp[:, :, 17:] = np.nan
    if skip:
        inp[:, :, skip[0]:skip[0] + skip[1]] = np.nan
    train = dict(first=1, count=40, first_bin=2, n_bins=15, skip=skip)             # 3 taps: 38 snapshot rows
    tr, d = attached(rts, inp)
    got = tr.cube_st_covariance(3, **train)
    assert np.all(np.isfinite(bits(got))) and np.array_equal(bits(got), bits(rts.st_covariance_eval(inp, 3, **train)))
    one = tr.cube_st_covariance(3, first=5, count=3, first_bin=2, n_bins=15, skip=skip)            # as many rows as taps: one snapshot row
    assert np.array_equal(bits(one), bits(rts.st_covariance_eval(inp, 3, first=5, count=3, first_bin=2, n_bins=15, skip=skip)))
    tr.close()


def test_covariance_three_sources_and_one_tap(rts):
    rng = np.random.default_rng(23)
    n_rx, n_p, nb, n_fft = 3, 6, 37, 8
    inp = B.random_complex(rng, (n_rx, n_p, nb))
    tr, d = attached(rts, inp)
    dmap = tr.cube_doppler(n_fft)                                                  # library-owned
    train = dict(first=1, count=5, first_bin=3, skip=(10, 4))
    from_map = tr.cube_st_covariance(2, source="map", **train)
    dm = dev(dmap)
    from_ptr = tr.cube_st_covariance(2, source="pointer", device_in=dm.data_ptr(), n_rows_in=n_fft, **train)
    assert np.array_equal(bits(from_map), bits(from_ptr)) and np.array_equal(bits(from_map), bits(rts.st_covariance_eval(dmap, 2, **train)))
    from_cube = tr.cube_st_covariance(4, first=2)
    assert np.array_equal(bits(from_cube), bits(rts.st_covariance_eval(inp, 4, first=2)))
    # one tap: rts_cube_covariance's bits
    assert np.array_equal(bits(tr.cube_st_covariance(1, **train)), bits(tr.cube_covariance(**train)))
    assert np.array_equal(bits(tr.cube_st_covariance(1)), bits(rts.covariance_eval(inp)))
    tr.close()


# ----------------------------------------------------------------------------- 2. the filter against the evaluator
def apply_case(rts, N, M, F, rows, bins, seed, power=False):
    rng = np.random.default_rng(seed)
    inp = framed(rng, N, rows, bins)
    w = B.random_complex(rng, (F, N * M))
    tr, d = attached(rts, inp)
    got = tr.cube_st_apply(w, M, first=1, count=rows, power=power)
    want = rts.st_apply_eval(inp, w, M, first=1, count=rows, power=power)
    assert got.shape == (F, rows - M + 1, bins) and np.all(np.isfinite(bits(got)))
    assert np.array_equal(bits(got), bits(want)), (N, M, F, rows, bins, power)
    tr.close()


@pytest.mark.parametrize("M", range(1, S.MAX_TAPS + 1))
def test_apply_every_tap_count(rts, M):
    for rows in (M, M + 1):
        apply_case(rts, 2, M, 3, rows, 5, 7000 + 10 * M + rows)


@pytest.mark.parametrize("out_rows", [STRIP - 1, STRIP, STRIP + 1, 2 * STRIP + 1])
def test_apply_strips(rts, out_rows):
    apply_case(rts, 2, 3, 3, out_rows + 2, 3, 7300 + out_rows)


@pytest.mark.parametrize("bins", [1, 63, 64, 65, 255, 256, 257])
def test_apply_bins(rts, bins):
    apply_case(rts, 2, 3, 2, 4, bins, 7500 + bins)


@pytest.mark.parametrize("N,M,F", [(2, 3, 7), (2, 3, 8), (2, 3, 9), (2, 3, 17), (2, 2, 15), (2, 2, 16), (2, 2, 17), (2, 6, 5), (1, 9, 3), (2, 2, 1024)] +
                         [(N, 2, 3) for N in (1, RXT - 1, RXT, RXT + 1, 2 * RXT + 1, 32)] + [(8, 8, 5), (4, 16, 3)])
def test_apply_tiles(rts, N, M, F):
    """F at the filter tile's edges (and 1024 filters at D = 4), N at the receiver tile's edges with two taps, D = 64 both ways"""
    apply_case(rts, N, M, F, M + 2, 5, 7700 + 100 * N + 10 * M + F)


def test_apply_power_sources_sentinels_and_runs(rts):
    import torch
    rng = np.random.default_rng(29)
    n_rx, n_p, nb, n_fft, M, F, PAD = 3, 6, 67, 8, 3, 5, 16
    inp = B.random_complex(rng, (n_rx, n_p, nb)); w = B.random_complex(rng, (F, n_rx * M))
    apply_case(rts, 3, 3, 9, 37, 70, 31, power=True)
    tr, d = attached(rts, inp)
    # the three sources
    dmap = tr.cube_doppler(n_fft)
    from_map = tr.cube_st_apply(w, M, source="map", first=1, count=6)
    dm = dev(dmap)
    from_ptr = tr.cube_st_apply(w, M, source="pointer", device_in=dm.data_ptr(), n_rows_in=n_fft, first=1, count=6)
    assert np.array_equal(bits(from_map), bits(from_ptr)) and np.array_equal(bits(from_map), bits(rts.st_apply_eval(dmap, w, M, first=1, count=6)))
    from_cube = tr.cube_st_apply(w, M, first=2)
    want = rts.st_apply_eval(inp, w, M, first=2)
    assert from_cube.shape == (F, 2, nb) and np.array_equal(bits(from_cube), bits(want)) and np.array_equal(bits(tr.st_map()), bits(want))
    # sentinels before and after a caller-owned output, complex and power; a caller-owned run is not recorded
    for power, dtype, fill in ((False, torch.complex128, complex(7.25, -3.5)), (True, torch.float64, 7.25)):
        buf = filled(F * 2 * nb + 2 * PAD, fill, dtype)
        assert tr.cube_st_apply(w, M, first=2, power=power, device_ptr=buf.data_ptr() + buf.element_size() * PAD) is None
        tr.cube()                                                                # (the handle's stream drained)
        h = host(buf)
        assert np.all(h[:PAD] == fill) and np.all(h[-PAD:] == fill)
        assert np.array_equal(bits(h[PAD:-PAD].reshape(want.shape)), bits(rts.st_apply_eval(inp, w, M, first=2, power=power)))
    assert np.array_equal(bits(tr.st_map()), bits(want))
    # two runs equal; the input is only read
    assert tr.cube_st_apply(w, M, first=2).tobytes() == from_cube.tobytes()
    assert np.array_equal(bits(host(d)), bits(inp))
    # one tap: rts_cube_beamform's bits, in both forms
    w1 = w[:, :n_rx]
    assert np.array_equal(bits(tr.cube_st_apply(w1, 1, first=1, count=4)), bits(tr.cube_beamform(w1, first=1, count=4)))
    assert np.array_equal(tr.cube_st_apply(w1, 1, power=True), tr.cube_beamform(w1, power=True))
    tr.close()


# ----------------------------------------------------------------------------- 3. lifetime and errors on a live handle
def test_errors_and_lifetime(rts):
    from rts_amd import _lib as L
    import torch
    lib = L.lib()
    rng = np.random.default_rng(37)
    n_rx, n_p, nb, M = 3, 5, 40, 2
    D = n_rx * M
    inp = B.random_complex(rng, (n_rx, n_p, nb)); w = np.ascontiguousarray(B.random_complex(rng, (2, D))); s = np.ascontiguousarray(B.random_complex(rng, (2, D)))
    out = np.full(2 * D * D + 2, 7.25)

    def cparams(**kw):
        p = L.RtsStCovParams(); p.n_taps = M
        for k, v in kw.items():
            setattr(p, k, v)
        return p

    def aparams(**kw):
        p = L.RtsStApplyParams(); p.n_taps, p.n_filters, p.weights = M, 2, w.ctypes.data
        for k, v in kw.items():
            setattr(p, k, v)
        return p
    tr = rts.Tracer(8, 1)
    assert lib.rts_cube_st_covariance(tr.h, C.byref(cparams()), None) == L.RTS_ERR_INVALID and b"attach" in lib.rts_last_error()      # no cube
    assert lib.rts_cube_st_apply(tr.h, C.byref(aparams()), None) == L.RTS_ERR_INVALID and b"attach" in lib.rts_last_error()
    assert lib.rts_cube_st_get(tr.h, out.ctypes.data, out.size) == L.RTS_ERR_INVALID
    d = dev(inp)
    tr.cube_attach(n_rx, n_p, nb, 0.0, 1.0, device_ptr=d.data_ptr())
    assert lib.rts_cube_st_get(tr.h, out.ctypes.data, out.size) == L.RTS_ERR_INVALID and b"filter output" in lib.rts_last_error()
    # a library-owned st-covariance is the handle's covariance: covariance() and cube_mvdr(device_cov=None) take it as it is
    cov = tr.cube_st_covariance(M, skip=(10, 3))
    assert cov.shape == (D, D) and np.array_equal(bits(cov), bits(rts.st_covariance_eval(inp, M, skip=(10, 3)))) and np.array_equal(bits(tr.covariance()), bits(cov))
    w_first = tr.cube_mvdr(s, 0.5)
    assert w_first.shape == (2, D) and np.array_equal(bits(w_first), bits(rts.mvdr_eval(cov, s, 0.5)))
    y_first = tr.cube_st_apply(w_first, M)
    assert np.array_equal(bits(y_first), bits(rts.st_apply_eval(inp, w_first, M)))
    mp = L.RtsMvdrParams(); mp.n_beams, mp.n_rx, mp.steering = 2, n_rx, s.ctypes.data       # the record's n_rx: 0 or the covariance's order
    assert lib.rts_cube_mvdr(tr.h, C.byref(mp), None) == L.RTS_ERR_INVALID and b"n_rx" in lib.rts_last_error()
    # refusals
    caller = filled(2 * (n_p - M + 1) * nb + 1, 0j, torch.complex128)
    ccaller = filled(D * D + 1, 0j, torch.complex128)
    other = dev(B.random_complex(rng, (n_rx, 2, nb)))
    cres = cparams(); cres.reserved[1] = 1
    cov_cases = [("null p", None, None, b"null"), ("reserved", cres, None, b"reserved"), ("reserved0", cparams(reserved0=1), None, b"reserved"),
                 ("source", cparams(source=3), None, b"source"), ("no taps", cparams(n_taps=0), None, b"n_taps"), ("too many taps", cparams(n_taps=17), None, b"n_taps"),
                 ("rows below the taps", cparams(n_rows=1), None, b"n_taps"), ("default rows below the taps", cparams(first_row=4), None, b"n_taps"),
                 ("no map", cparams(source=L.RTS_BEAM_FROM_MAP), None, b"RTS_BEAM_FROM_MAP"),
                 ("pointer null", cparams(source=L.RTS_BEAM_FROM_POINTER, n_rows_in=2), None, b"device_in"),
                 ("pointer misaligned", cparams(source=L.RTS_BEAM_FROM_POINTER, n_rows_in=2, device_in=other.data_ptr() + 8), None, b"device_in"),
                 ("pointer without rows", cparams(source=L.RTS_BEAM_FROM_POINTER, device_in=other.data_ptr()), None, b"n_rows_in"),
                 ("n_rows_in with the cube", cparams(n_rows_in=2), None, b"n_rows_in"), ("first_row beyond", cparams(first_row=n_p), None, b"first_row"),
                 ("rows beyond", cparams(first_row=2, n_rows=4), None, b"n_rows"), ("bins beyond", cparams(first_bin=30, n_bins=11), None, b"n_bins"),
                 ("skip leaves nothing", cparams(skip_n_bins=nb), None, b"leaves no bin"),
                 ("device_out misaligned", cparams(), ccaller.data_ptr() + 8, b"device_out"), ("in place", cparams(), d.data_ptr(), b"overlaps"),
                 # rows 2 .. 3, two taps: the last start row is 2, its second tap reads row 3 -- the last element of the last receiver's row 3
                 ("overlapping the last tap's last cell", cparams(first_row=2, n_rows=2), d.data_ptr() + 16 * ((2 * n_p + 4) * nb - 1), b"overlaps")]
    for name, p, device_out, word in cov_cases:
        rc = lib.rts_cube_st_covariance(tr.h, C.byref(p) if p is not None else None, C.c_void_p(device_out) if device_out else None)
        assert rc == L.RTS_ERR_INVALID, name
        assert word in lib.rts_last_error(), (name, lib.rts_last_error())
    bad_w = w.copy(); bad_w[1, 2] = complex(1.0, math.inf)
    ares = aparams(); ares.reserved[0] = 1
    apply_cases = [("null p", None, None, b"null"), ("reserved", ares, None, b"reserved"), ("reserved0", aparams(reserved0=1), None, b"reserved"),
                   ("source", aparams(source=3), None, b"source"), ("peak", aparams(flags=L.RTS_BEAM_PEAK), None, b"flags"),
                   ("no taps", aparams(n_taps=0), None, b"n_taps"), ("too many taps", aparams(n_taps=17), None, b"n_taps"),
                   ("no filters", aparams(n_filters=0), None, b"n_filters"), ("null weights", aparams(weights=None), None, b"weights"),
                   ("weights inf", aparams(weights=bad_w.ctypes.data), None, b"weights"), ("rows below the taps", aparams(n_rows=1), None, b"n_taps"),
                   ("no map", aparams(source=L.RTS_BEAM_FROM_MAP), None, b"RTS_BEAM_FROM_MAP"),
                   ("pointer null", aparams(source=L.RTS_BEAM_FROM_POINTER, n_rows_in=2), None, b"device_in"),
                   ("pointer misaligned", aparams(source=L.RTS_BEAM_FROM_POINTER, n_rows_in=2, device_in=other.data_ptr() + 8), None, b"device_in"),
                   ("n_rows_in with the cube", aparams(n_rows_in=2), None, b"n_rows_in"), ("first_row beyond", aparams(first_row=n_p), None, b"first_row"),
                   ("rows beyond", aparams(first_row=2, n_rows=4), None, b"n_rows"),
                   ("device_out misaligned", aparams(), caller.data_ptr() + 8, b"device_out"), ("in place", aparams(), d.data_ptr(), b"overlaps"),
                   # rows 2 .. 3, two taps: one output row, whose second tap reads row 3 -- the last element of the last receiver's row 3
                   ("overlapping the last tap's last cell", aparams(first_row=2, n_rows=2), d.data_ptr() + 16 * ((2 * n_p + 4) * nb - 1), b"overlaps")]
    for name, p, device_out, word in apply_cases:
        rc = lib.rts_cube_st_apply(tr.h, C.byref(p) if p is not None else None, C.c_void_p(device_out) if device_out else None)
        assert rc == L.RTS_ERR_INVALID, name
        assert word in lib.rts_last_error(), (name, lib.rts_last_error())
    tb = rts.Tracer(8, 1); tb.cube_attach(5, 13, 2, 0.0, 1.0)                    # 13 taps of 5 receivers: 65 entries
    wide = np.ones((1, 65), np.complex128)
    assert lib.rts_cube_st_covariance(tb.h, C.byref(cparams(n_taps=13)), None) == L.RTS_ERR_INVALID and b"n_taps * n_rx" in lib.rts_last_error()
    assert lib.rts_cube_st_apply(tb.h, C.byref(aparams(n_taps=13, n_filters=1, weights=wide.ctypes.data)), None) == L.RTS_ERR_INVALID and b"n_taps * n_rx" in lib.rts_last_error()
    tb.close()
    # the previous products are still there, and readable; nothing was written
    assert np.array_equal(bits(tr.covariance()), bits(cov)) and np.array_equal(bits(tr.mvdr_weights()), bits(w_first)) and np.array_equal(bits(tr.st_map()), bits(y_first))
    assert np.array_equal(bits(host(d)), bits(inp)) and np.count_nonzero(host(caller)) == 0 and np.count_nonzero(host(ccaller)) == 0
    # capacity; a NULL output; the exact capacity
    big = np.full(y_first.size * 2 + 2, 7.25)
    assert lib.rts_cube_st_get(tr.h, big.ctypes.data, 2 * y_first.size - 1) == L.RTS_ERR_CAPACITY and np.all(big == 7.25)
    assert lib.rts_cube_st_get(tr.h, None, big.size) == L.RTS_ERR_INVALID
    assert lib.rts_cube_st_get(tr.h, big.ctypes.data, 2 * y_first.size) == L.RTS_OK and big[-1] == 7.25 and big[-2] == 7.25
    assert np.array_equal(big[:-2], bits(y_first).ravel())
    # a caller-owned st-covariance is not recorded; rts_cube_covariance replaces the library-owned one, with its own order
    tr.cube_st_covariance(M, first=1, device_ptr=ccaller.data_ptr())
    assert np.array_equal(bits(tr.covariance()), bits(cov))
    assert tr.cube_covariance().shape == (n_rx, n_rx)
    # the products end at rts_cube_attach
    tr.cube_st_covariance(M, fetch=False)
    tr.cube_attach(n_rx, n_p, nb, 0.0, 1.0, device_ptr=d.data_ptr())
    assert lib.rts_cube_st_get(tr.h, big.ctypes.data, big.size) == L.RTS_ERR_INVALID and b"rts_cube_attach" in lib.rts_last_error()
    assert lib.rts_cube_covariance_get(tr.h, out.ctypes.data, out.size) == L.RTS_ERR_INVALID and b"rts_cube_attach" in lib.rts_last_error()
    mp.n_rx = 0
    assert lib.rts_cube_mvdr(tr.h, C.byref(mp), None) == L.RTS_ERR_INVALID and b"no covariance" in lib.rts_last_error()
    tr.close()
    for call in (lambda: tr.cube_st_covariance(M), lambda: tr.cube_st_apply(w, M), lambda: tr.st_map()):
        with pytest.raises(L.RtsError):
            call()


def test_covariance_output_right_behind_the_last_cell_read(rts):
    """the accepted neighbour of the stacked covariance's two overlap refusals of test_errors_and_lifetime: the caller's output starts at the
    first byte behind the last receiver's last tap's last cell, inside the cube's own allocation: RTS_OK, the library-owned call's
    bytes, the sentinel behind it and the cube untouched"""
    from rts_amd import _lib as L
    import torch
    lib = L.lib()
    rng = np.random.default_rng(41)
    n_rx, n_p, nb, M = 3, 4, 7, 2
    inp = B.random_complex(rng, (n_rx, n_p, nb))
    block = torch.empty(inp.size + (n_rx * M) * (n_rx * M) + 1, dtype=torch.complex128, device="cuda")      # ONE allocation: [the cube | the caller's output | a sentinel]
    block[:inp.size] = torch.from_numpy(inp.ravel()); block[inp.size:] = complex(7.25, -7.25)
    torch.cuda.synchronize()
    tr = rts.Tracer(8, 1)
    tr.cube_attach(n_rx, n_p, nb, 0.0, 1.0, device_ptr=block.data_ptr())
    owned = tr.cube_st_covariance(M)
    p = L.RtsStCovParams(); p.n_taps = M
    assert lib.rts_cube_st_covariance(tr.h, C.byref(p), C.c_void_p(block.data_ptr() + 16 * inp.size)) == L.RTS_OK, lib.rts_last_error()
    tr.cube()                                                                    # (drains the handle's stream)
    after = host(block)
    assert np.array_equal(bits(after[inp.size:-1]), bits(np.asarray(owned).ravel()))
    assert after[-1] == complex(7.25, -7.25) and np.array_equal(bits(after[:inp.size]), bits(inp.ravel()))
    tr.close()


def test_apply_output_right_behind_the_last_cell_read(rts):
    """... and of the filter's: the last output row's last tap reads the last receiver's last row"""
    from rts_amd import _lib as L
    import torch
    lib = L.lib()
    rng = np.random.default_rng(43)
    n_rx, n_p, nb, M, F = 3, 4, 7, 2, 2
    inp = B.random_complex(rng, (n_rx, n_p, nb))
    w = np.ascontiguousarray(B.random_complex(rng, (F, n_rx * M)))
    block = torch.empty(inp.size + F * (n_p - M + 1) * nb + 1, dtype=torch.complex128, device="cuda")      # ONE allocation: [the cube | the caller's output | a sentinel]
    block[:inp.size] = torch.from_numpy(inp.ravel()); block[inp.size:] = complex(7.25, -7.25)
    torch.cuda.synchronize()
    tr = rts.Tracer(8, 1)
    tr.cube_attach(n_rx, n_p, nb, 0.0, 1.0, device_ptr=block.data_ptr())
    owned = tr.cube_st_apply(w, M)
    p = L.RtsStApplyParams(); p.n_taps, p.n_filters, p.weights = M, F, w.ctypes.data
    assert lib.rts_cube_st_apply(tr.h, C.byref(p), C.c_void_p(block.data_ptr() + 16 * inp.size)) == L.RTS_OK, lib.rts_last_error()
    tr.cube()                                                                    # (drains the handle's stream)
    after = host(block)
    assert np.array_equal(bits(after[inp.size:-1]), bits(np.asarray(owned).ravel()))
    assert after[-1] == complex(7.25, -7.25) and np.array_equal(bits(after[:inp.size]), bits(inp.ravel()))
    tr.close()


# ----------------------------------------------------------------------------- 4. the whole chain
def test_whole_chain(rts):
    """tests/stap_ref.py's scene on the device: noise, the stacked covariance without the target's bins, the weights, the filter --
    against the host chain run on the device's own noisy cube, bit for bit; the output, attached to a second handle as a cube of one
    receiver and 14 pulses, peaks at (Doppler row 4, bin 24) of its 16-point map"""
    import torch
    sc = S.SCENE
    taps = sc["taps"]
    tr, d = attached(rts, S.scene_clean_cube())
    tr.cube_add_noise(sc["noise_power"], sc["seed"])
    spatial = S.scene_spatial_steering(rts)
    out_rows = sc["n_pulses"] - taps + 1
    ybuf = filled(out_rows * sc["n_bins"], 0j, torch.complex128)
    y = tr.cube_stap(spatial, [sc["target_f"]], taps, train=dict(skip=sc["skip"]), loading=sc["noise_power"])
    noisy = tr.cube()
    cube_h = S.scene_noisy_cube(rts)
    np.testing.assert_allclose(noisy, cube_h, rtol=1e-10, atol=1e-12 * np.abs(cube_h).max())
    _, s_h, cov_h, w_h, y_h = S.scene_host(rts, taps, noisy)
    assert np.array_equal(bits(tr.covariance()), bits(cov_h)) and np.array_equal(bits(tr.mvdr_weights()), bits(w_h))
    assert y.shape == (1, out_rows, sc["n_bins"]) and np.array_equal(bits(y), bits(y_h))
    # the two-handle chain: the same filter into caller memory, which a second handle attaches
    assert tr.cube_st_apply(tr.mvdr_weights(), taps, device_ptr=ybuf.data_ptr()) is None
    tr.cube()
    t2 = rts.Tracer(8, 1)
    t2.cube_attach(1, out_rows, sc["n_bins"], 0.0, 1.0, device_ptr=ybuf.data_ptr())
    assert np.array_equal(bits(t2.cube()), bits(y))
    power = np.abs(t2.cube_doppler(sc["n_fft"])[0]) ** 2
    assert np.unravel_index(power.argmax(), power.shape) == (sc["doppler_row"], sc["target_bin"])
    # the power form passes through
    p = tr.cube_stap(spatial, [sc["target_f"]], taps, train=dict(skip=sc["skip"]), loading=sc["noise_power"], power=True, first=2, count=5)
    assert np.array_equal(p, B.power_restated(y[:, 2:5]))
    t2.close(); tr.close()
