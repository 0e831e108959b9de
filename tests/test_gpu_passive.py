"""Passive radar on the device (rts_cube_cancel, rts_cube_xcorr): the kernels against the host evaluators rts_cancel_eval /
rts_xcorr_eval BIT FOR BIT (the trees hold + - * / and sqrt only) over the edge shapes of tests/passive_ref.py -- the taps at their
ends, bins around the taps and the tile, parts around a block's cap, every rows_per_block against the span, a short last block, the
reference first and last, one receiver, a mask, lags beyond the row, two groups of lags --; the coefficients, the info record and the
cancelled cube; failed blocks; sentinel cells around a caller-owned correlation; library-owned against caller-owned; run-to-run
equality; the lifetime of the products; the error rules on a live handle; and the chain of tests/passive_chain_ref.py on the device
against its host run."""
import numpy as np
import pytest

import passive_ref as P

pytestmark = pytest.mark.gpu
bits = P.bits


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


def same(a, b):
    return np.array_equal(bits(a), bits(b), equal_nan=True)


# ----------------------------------------------------------------------------- 1. cancellation against the evaluator
CANCEL = P.cancel_cases() + P.cancel_cases_evaluator_only()


@pytest.mark.parametrize("case", CANCEL, ids=[c[0] for c in CANCEL])
def test_cancel_against_the_evaluator(rts, case):
    name, n_rx, n_p, N, kw = case
    cube = P.cancel_input(name, n_rx, n_p, N, kw)                  # (rows outside the span are NaN: never read, never written)
    want_cube, want_c, want_info = rts.cancel_eval(cube, **kw)
    tr, d = attached(rts, cube)
    tr.cube_cancel(**kw)
    assert tr.cancel_info() == want_info and want_info[1] == 0
    got_c = tr.cancel_coeffs()
    assert got_c.shape == want_c.shape and same(got_c, want_c)
    got = host(d)
    assert same(got, want_cube)
    assert same(got[kw["ref_rx"]], cube[kw["ref_rx"]])             # the reference rows are never written
    # run to run: the same call on the same input again
    d2 = dev(cube)
    tr.cube_attach(n_rx, n_p, N, 0.0, 1.0, device_ptr=d2.data_ptr())
    tr.cube_cancel(**kw)
    assert same(host(d2), got) and same(tr.cancel_coeffs(), got_c)
    tr.close()


def test_mask_leaves_the_other_receivers_alone(rts):
    name, n_rx, n_p, N, kw = [c for c in CANCEL if c[0] == "mask"][0]
    cube = P.cancel_input(name, n_rx, n_p, N, kw)
    tr, d = attached(rts, cube)
    tr.cube_cancel(**kw)
    got = host(d)
    assert same(got[2], cube[2]) and same(got[1], cube[1]) and not same(got[0], cube[0]) and not same(got[3], cube[3])
    c = tr.cancel_coeffs()
    assert not c[1].any() and not c[2].any() and c[0].all() and c[3].all()
    tr.close()


@pytest.mark.parametrize("why", ["few_samples", "zero_reference", "nan_reference"])
def test_failed_blocks(rts, why):
    """three blocks of two rows, the middle one fails: its rows untouched, its coefficients 0, one failed block counted"""
    rng = np.random.default_rng(5)
    K, N = (4, 1) if why == "few_samples" else (3, 20)
    cube = P.random_complex(rng, (3, 6, N))
    kw = dict(ref_rx=0, n_taps=K, rows_per_block=2)
    if why == "zero_reference":
        cube[0, 2:4] = 0.0
    if why == "nan_reference":
        cube[0, 3, 7] = np.nan
    want_cube, want_c, want_info = rts.cancel_eval(cube, **kw)
    assert want_info == ((3, 3) if why == "few_samples" else (3, 1))
    tr, d = attached(rts, cube)
    tr.cube_cancel(**kw)
    assert tr.cancel_info() == want_info
    got, c = host(d), tr.cancel_coeffs()
    assert same(got, want_cube) and same(c, want_c)
    bad = slice(0, 6) if why == "few_samples" else slice(2, 4)
    assert same(got[:, bad], cube[:, bad]) and not c[:, 1].any()
    tr.close()


# ----------------------------------------------------------------------------- 2. correlation against the evaluator
XCORR = P.xcorr_cases()


@pytest.mark.parametrize("case", XCORR, ids=[c[0] for c in XCORR])
def test_xcorr_against_the_evaluator(rts, case):
    import torch
    name, n_rx, n_p, N, kw = case
    cube = P.xcorr_input(name, n_rx, n_p, N, kw)
    want = rts.xcorr_eval(cube, **kw)
    tr, d = attached(rts, cube)
    own = tr.cube_xcorr(**kw)
    assert own.shape == want.shape and same(own, want)
    if kw.get("first_lag", 0) + kw["n_lags"] > N:                  # lags at or beyond the row: exact zeros
        assert not own[:, :, max(N - kw.get("first_lag", 0), 0):].any()
    # caller-owned, between sentinels
    pad = 8
    buf = torch.full((want.size + 2 * pad,), complex(-7.0, 3.0), dtype=torch.complex128, device="cuda")
    torch.cuda.synchronize()
    assert tr.cube_xcorr(device_ptr=buf.data_ptr() + 16 * pad, **kw) is None
    flat = host(buf)
    assert np.all(flat[:pad] == complex(-7.0, 3.0)) and np.all(flat[-pad:] == complex(-7.0, 3.0))
    assert same(flat[pad:-pad].reshape(want.shape), want)
    assert same(tr.xcorr_map(), want)                               # the library-owned product is still the earlier call's
    assert same(host(d), cube)                                      # out of place: the cube is as it was
    assert same(tr.cube_xcorr(**kw), own)                           # run to run
    tr.close()


def test_cube_passive_and_the_products_lifetime(rts):
    rng = np.random.default_rng(11)
    cube = P.random_complex(rng, (3, 4, 64)); cube[1] += 5.0 * cube[0]; cube[2] += (2.0 - 1.0j) * cube[0]
    want_cube, want_c, info = rts.cancel_eval(cube, 0, 2, 2)
    want = rts.xcorr_eval(want_cube, 0, 16, 1)
    tr, d = attached(rts, cube)
    got = tr.cube_passive(0, 2, 16, rows_per_block=2, first_lag=1)
    assert same(got, want) and same(tr.cancel_coeffs(), want_c) and tr.cancel_info() == info
    d2 = dev(cube)
    tr.cube_attach(3, 4, 64, 0.0, 1.0, device_ptr=d2.data_ptr())    # every product ends at rts_cube_attach
    for call in (tr.xcorr_map, tr.cancel_coeffs, tr.cancel_info):
        with pytest.raises(rts.L.RtsError) as e:
            call()
        assert e.value.code == rts.L.RTS_ERR_INVALID
    tr.close()


def test_error_rules_on_a_live_handle(rts):
    import torch
    L = rts.L
    tr = rts.Tracer(8, 1)
    tr._cube_shape = (3, 4, 32)
    with pytest.raises(L.RtsError) as e:
        tr.cube_cancel(0, 2)
    assert "no cube" in str(e.value)
    with pytest.raises(L.RtsError) as e:
        tr.cube_xcorr(0, 4)
    assert "no cube" in str(e.value)
    cube = P.random_complex(np.random.default_rng(2), (3, 4, 32))
    d = dev(cube)
    tr.cube_attach(3, 4, 32, 0.0, 1.0, device_ptr=d.data_ptr())
    bad_cancel = [(dict(ref_rx=3, n_taps=2), "ref_rx"), (dict(ref_rx=0, n_taps=0), "n_taps"), (dict(ref_rx=0, n_taps=65), "n_taps"),
                  (dict(ref_rx=0, n_taps=2, first=4), "pulse"), (dict(ref_rx=0, n_taps=2, count=0), "pulse"), (dict(ref_rx=0, n_taps=2, count=5), "pulse"),
                  (dict(ref_rx=0, n_taps=2, loading=-1.0), "loading"), (dict(ref_rx=0, n_taps=2, loading=float("nan")), "loading"),
                  (dict(ref_rx=1, n_taps=2, rx=[0, 1]), "rx_mask"), (dict(ref_rx=0, n_taps=2, rx=[3]), "rx_mask")]
    for kw, word in bad_cancel:
        with pytest.raises(L.RtsError) as e:
            tr.cube_cancel(**kw)
        assert e.value.code == L.RTS_ERR_INVALID and word in str(e.value), (kw, str(e.value))
    bad_xcorr = [(dict(ref_rx=3, n_lags=4), "ref_rx"), (dict(ref_rx=0, n_lags=0), "n_lags"), (dict(ref_rx=0, n_lags=P.MAX_LAGS + 1), "n_lags"),
                 (dict(ref_rx=0, n_lags=4, first_lag=0x7fff0001), "first_lag"), (dict(ref_rx=0, n_lags=4, first=4), "pulse"), (dict(ref_rx=0, n_lags=4, count=0), "pulse")]
    for kw, word in bad_xcorr:
        with pytest.raises(L.RtsError) as e:
            tr.cube_xcorr(**kw)
        assert e.value.code == L.RTS_ERR_INVALID and word in str(e.value), (kw, str(e.value))
    with pytest.raises(L.RtsError) as e:
        tr.cube_xcorr(0, 4, device_ptr=d.data_ptr() + 8)
    assert "aligned" in str(e.value)
    with pytest.raises(L.RtsError) as e:
        tr.cube_xcorr(0, 4, device_ptr=d.data_ptr() + 16 * 40)
    assert "overlaps" in str(e.value)
    for call in (tr.xcorr_map, tr.cancel_coeffs, tr.cancel_info):     # nothing was made: the refused calls left no product
        with pytest.raises(L.RtsError):
            call()
    assert same(host(d), cube)
    tr.cube_cancel(0, 2)                                              # the handle stays usable
    out = np.zeros(3, np.float64)
    import ctypes as C
    assert L.lib().rts_cube_cancel_coeffs_get(tr.h, out.ctypes.data_as(C.c_void_p), 3) == L.RTS_ERR_CAPACITY
    del torch
    tr.close()


# ----------------------------------------------------------------------------- 3. the chain on a traced scene
def test_traced_passive_chain(rts, oracle):
    """tests/passive_chain_ref.py's scenario on the device: per pulse a new waveform segment and the render of the traced rays into a
    caller-owned cube, the receiver noise, the caller's reference rows, direct signal and clutter written through the cube's tensor;
    then xcorr without and with cube_cancel, each output re-attached as a cube of 64 bins for cube_doppler and cube_detect_os.
    (a) without the cancellation no target cell is reported, (b) with it all nine are and the clutter is down by the numpy
    restatement's factor (PC.check_chain, as on the host).  (c) against the host: the device's cube equals the host chain's within the
    render's re-association (a sum of at most 150 rays per sample: 1e-10 of the largest echo sample is generous); on the DEVICE'S
    cube the evaluators give the device's cancelled cube, coefficients and both correlations bit for bit; the Doppler maps lie within
    1e-12 of their largest cell of the longdouble transform of the device's correlations (the map's tolerance in
    tests/test_gpu_detect.py, with room for 16 terms); and the detections are the host chain's, cell by cell."""
    import torch
    import helpers as H
    import cube_ref as CR
    import passive_chain_ref as PC
    hc = PC.host_chain(rts, oracle)
    spec = PC.spec(rts)
    tr = H.gpu_tracer(rts, spec)
    cube_t = torch.zeros((PC.N_RX, PC.N_PULSES, PC.N_BINS), dtype=torch.complex128, device="cuda")
    torch.cuda.synchronize()
    tr.cube_attach(PC.N_RX, PC.N_PULSES, PC.N_BINS, PC.T0, PC.DT, device_ptr=cube_t.data_ptr())
    seg = PC.segments()
    for m in range(PC.N_PULSES):
        H.gpu_trace(rts, spec, tr=tr, motion=PC.LC.motion(m))
        tr.finalise_uniform(None, PC.WL, 1.0, 1.0, PC.FC, PC.CS)
        tr.cube_set_waveform(rts.Waveform(seg[m], taps=1))
        tr.cube_render(m, "rays", PC.CS, PC.FC, doppler=True)
    tr.cube_add_noise(PC.NOISE_POWER, PC.NOISE_SEED)
    echoes_noise = host(cube_t)                                      # (synchronises: the handle's work is done before torch writes)
    cube_t[PC.REF] = dev(PC.reference_rows())
    cube_t[:PC.N_SURV] += dev(PC.caller_terms())
    cube = host(cube_t)
    # no ray reaches the reference slot: it held the noise alone (the device's noise against rts_noise_eval: tests/test_gpu_detect.py's 1e-13)
    np.testing.assert_allclose(echoes_noise[PC.REF], PC.noise(rts)[PC.REF], rtol=1e-13, atol=1e-13 * np.sqrt(PC.NOISE_POWER))
    np.testing.assert_allclose(cube, hc["cube"], rtol=0, atol=1e-10 * np.abs(hc["echoes"]).max())
    # the two correlations into caller-owned tensors, the cancellation between them
    z_raw = torch.zeros((PC.N_RX, PC.N_PULSES, PC.N_LAGS), dtype=torch.complex128, device="cuda")
    z_can = torch.zeros_like(z_raw)
    torch.cuda.synchronize()
    tr.cube_xcorr(PC.REF, PC.N_LAGS, device_ptr=z_raw.data_ptr())
    tr.cube_cancel(PC.REF, PC.K)
    tr.cube_xcorr(PC.REF, PC.N_LAGS, device_ptr=z_can.data_ptr())
    want_clean, want_c, want_info = rts.cancel_eval(cube, PC.REF, PC.K)
    assert tr.cancel_info() == want_info == (1, 0) and same(tr.cancel_coeffs(), want_c)
    assert same(host(cube_t), want_clean)
    assert same(host(z_raw), rts.xcorr_eval(cube, PC.REF, PC.N_LAGS)) and same(host(z_can), rts.xcorr_eval(want_clean, PC.REF, PC.N_LAGS))
    out = dict(cells=hc["cells"], cube=cube)
    for name, z in (("raw", z_raw), ("", z_can)):
        tr.cube_attach(PC.N_RX, PC.N_PULSES, PC.N_LAGS, 0.0, PC.DT, device_ptr=z.data_ptr())
        zmap = tr.cube_doppler(PC.N_PULSES)
        want_map = CR.to_double(CR.dft_ref(host(z), PC.N_PULSES))
        np.testing.assert_allclose(zmap, want_map, rtol=0, atol=1e-12 * np.abs(want_map).max())
        det = tr.cube_detect_os(**PC.CFAR)
        host_det = hc["raw_det" if name else "det"]
        assert [tuple(d) for d in det[["rx", "doppler_bin", "range_bin"]]] == [tuple(d) for d in host_det[["rx", "doppler_bin", "range_bin"]]]
        out["raw_map" if name else "map"] = zmap; out["raw_det" if name else "det"] = det
    PC.check_chain(out)
    tr.close()
