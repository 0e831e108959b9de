"""The MIMO matched-filter bank on the device (rts_cube_bank): the kernel against the host evaluator rts_bank_eval BIT FOR BIT over the
edge shapes of tests/mimo_ref.py -- bins around the output tile and beyond the compression's limit, waveform lengths around the tile,
at the row's length, beyond it and at their maximum, one, two and sixteen waveforms on one and four receivers, every group size a
thread may hold with full and partial last groups, mixed lengths in one set, a row range inside a cube, every kind of code table --;
sentinel cells around a caller-owned output and the cube unchanged; library-owned against caller-owned, the regrow and the product's
lifetime; a second call with a smaller set; one waveform against rts_cube_compress of a copy of the cube; the error rules on a live
handle."""
import numpy as np
import pytest

import mimo_ref as M

pytestmark = pytest.mark.gpu
same = M.same
CASES = M.cases()


def dev(a, dtype=np.complex128):
    """(torch's stream is not the handles': the buffer is finished before a handle reads it, and a handle's work before torch reads it)"""
    import torch
    buf = torch.from_numpy(np.array(a, dtype, order="C")).to("cuda")
    torch.cuda.synchronize()
    return buf


def host(buf):
    import torch
    torch.cuda.synchronize()
    return buf.cpu().numpy()


def attached(rts, inp):
    d = dev(inp)
    tr = rts.Tracer(8, 1)
    tr.cube_attach(inp.shape[0], inp.shape[1], inp.shape[2], 0.0, 1.0, device_ptr=d.data_ptr())
    return tr, d


def waves_of(rts, samples):
    return [rts.Waveform(s, 1) for s in samples]


def sentinel_buffer(n, pad=8):
    import torch
    buf = torch.full((n + 2 * pad,), complex(-7.0, 3.0), dtype=torch.complex128, device="cuda")
    torch.cuda.synchronize()
    return buf, pad


# ----------------------------------------------------------------------------- 1. against the evaluator
@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_bank_against_the_evaluator(rts, case):
    name, n_rx, n_p, N, lengths, code, first, count = case
    cube, samples, table = M.case_input(*case)                       # (rows outside the span are NaN: never read)
    waves = waves_of(rts, samples)
    want = rts.bank_eval(cube, waves, table, first, count)
    tr, d = attached(rts, cube)
    own = tr.cube_bank(waves, table, first, count)
    assert own.shape == want.shape and same(own, want)
    # caller-owned, between sentinels
    buf, pad = sentinel_buffer(want.size)
    assert tr.cube_bank(waves, table, first, count, device_ptr=buf.data_ptr() + 16 * pad) is None
    flat = host(buf)
    assert np.all(flat[:pad] == complex(-7.0, 3.0)) and np.all(flat[-pad:] == complex(-7.0, 3.0))
    assert same(flat[pad:-pad].reshape(want.shape), want)
    assert same(tr.bank_map(), want)                                 # the library-owned product is still the earlier call's
    assert same(host(d), cube)                                       # out of place: the cube, the rows outside the span too, is as it was
    tr.close()


def test_run_to_run_and_a_smaller_set_after_a_larger(rts):
    """the staged table and the library's output are sized by the larger call; the smaller call after it reuses both and gives its own
    result, and the larger one again gives its first bits"""
    rng = np.random.default_rng(21)
    cube = M.random_complex(rng, (2, 3, 100))
    big = [M.random_complex(rng, m) for m in (40, 7, 64, 3, 9)]; small = [M.random_complex(rng, 5)]
    code = M.random_complex(rng, (5, 3))
    tr, d = attached(rts, cube)
    first = tr.cube_bank(waves_of(rts, big), code)
    assert same(first, rts.bank_eval(cube, waves_of(rts, big), code))
    got = tr.cube_bank(waves_of(rts, small), None, 1, 2)
    assert got.shape == (2, 2, 100) and same(got, rts.bank_eval(cube, waves_of(rts, small), None, 1, 2))
    assert same(tr.cube_bank(waves_of(rts, big), code), first)
    tr.close()


def test_output_ownership_regrow_and_lifetime(rts):
    rng = np.random.default_rng(22)
    cube = M.random_complex(rng, (2, 2, 50))
    w = waves_of(rts, [M.random_complex(rng, 6)])
    tr, d = attached(rts, cube)
    with pytest.raises(rts.L.RtsError):
        tr.bank_map()                                                # nothing yet
    buf, pad = sentinel_buffer(2 * 2 * 50)
    tr.cube_bank(w, device_ptr=buf.data_ptr() + 16 * pad)
    with pytest.raises(rts.L.RtsError):
        tr.bank_map()                                                # a caller-owned output leaves no library product
    small = tr.cube_bank(w)
    # a much larger output regrows the library's block; the record names the new one
    many = waves_of(rts, [M.random_complex(rng, 4) for _ in range(16)])
    wide = M.random_complex(rng, (4, 64, 300))
    d2 = dev(wide)
    tr.cube_attach(4, 64, 300, 0.0, 1.0, device_ptr=d2.data_ptr())
    with pytest.raises(rts.L.RtsError) as e:
        tr.bank_map()                                                # the product ended at rts_cube_attach
    assert e.value.code == rts.L.RTS_ERR_INVALID
    large = tr.cube_bank(many)
    assert large.shape == (64, 64, 300) and same(large, rts.bank_eval(wide, many))
    d3 = dev(cube)
    tr.cube_attach(2, 2, 50, 0.0, 1.0, device_ptr=d3.data_ptr())
    assert same(tr.cube_bank(w), small)
    tr.close()


# ----------------------------------------------------------------------------- 2. against the compression
@pytest.mark.parametrize("N,m", [(1, 1), (M.TILE, 7), (M.TILE + 1, M.TILE + 1), (2 * M.TILE + 3, 300), (M.MAX_BINS, 64), (300, M.MAX_SAMPLES)])
def test_one_waveform_no_code_is_rts_cube_compress(rts, N, m):
    """rts_cube_compress (in place, one workgroup per row, the whole row in LDS) is the reference here, not the code under test: the
    bank of the same cube with the same waveform into a caller's buffer equals it bit for bit"""
    import torch
    rng = np.random.default_rng(N + m)
    cube = M.random_complex(rng, (2, 3, N)); s = M.random_complex(rng, m)
    tr, d = attached(rts, cube)
    out = torch.zeros((2, 3, N), dtype=torch.complex128, device="cuda")
    torch.cuda.synchronize()
    tr.cube_bank(waves_of(rts, [s]), device_ptr=out.data_ptr())
    got = host(out)
    copy = dev(cube)
    tr.cube_attach(2, 3, N, 0.0, 1.0, device_ptr=copy.data_ptr())
    tr.cube_set_waveform(rts.Waveform(s, 1))
    tr.cube_compress()
    assert same(got, host(copy)) and same(host(d), cube)
    tr.close()


# ----------------------------------------------------------------------------- 3. refusals on a live handle
def test_error_rules_on_a_live_handle(rts):
    L = rts.L
    rng = np.random.default_rng(2)
    tr = rts.Tracer(8, 1)
    tr._cube_shape = (3, 4, 32)
    w = waves_of(rts, [M.random_complex(rng, 5), M.random_complex(rng, 3)])
    with pytest.raises(L.RtsError) as e:
        tr.cube_bank(w)
    assert "no cube" in str(e.value)
    cube = M.random_complex(rng, (3, 4, 32))
    d = dev(cube)
    tr.cube_attach(3, 4, 32, 0.0, 1.0, device_ptr=d.data_ptr())
    good = tr.cube_bank(w)
    buf, pad = sentinel_buffer(6 * 4 * 32)
    nan_code = np.ones((2, 4), np.complex128); nan_code[1, 3] = np.nan
    bad = [(dict(waves=[]), "n_waves"), (dict(waves=w * 9), "n_waves"), (dict(waves=[rts.Waveform([1.0], taps=3)]), "taps"),
           (dict(waves=[w[0], rts.Waveform([np.inf])]), "waves[1]: sample 0 is not finite"), (dict(waves=[rts.Waveform(np.ones(M.MAX_SAMPLES + 1))]), "samples"),
           (dict(waves=w, first=4), "pulse"), (dict(waves=w, count=0), "pulse"), (dict(waves=w, first=2, count=3), "pulse"), (dict(waves=w, code=nan_code), "code[1][3]")]
    for kw, word in bad:
        with pytest.raises(L.RtsError) as e:
            tr.cube_bank(device_ptr=buf.data_ptr() + 16 * pad, **kw)
        assert e.value.code == L.RTS_ERR_INVALID and word in str(e.value), (kw, str(e.value))
    with pytest.raises(L.RtsError) as e:
        tr.cube_bank(w, device_ptr=buf.data_ptr() + 8)
    assert "aligned" in str(e.value)
    with pytest.raises(L.RtsError) as e:
        tr.cube_bank(w, device_ptr=d.data_ptr() + 16 * 40)
    assert "overlaps" in str(e.value)
    assert np.all(host(buf) == complex(-7.0, 3.0))                   # a refused call leaves the output untouched ...
    assert same(tr.bank_map(), good) and same(host(d), cube)         # ... and the previous product valid
    import ctypes as C
    out = np.zeros(3, np.float64)
    assert L.lib().rts_cube_bank_get(tr.h, out.ctypes.data_as(C.c_void_p), 3) == L.RTS_ERR_CAPACITY
    tr.close()
