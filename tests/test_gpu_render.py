"""Received signal on the device (rts_cube_set_waveform, rts_cube_render, rts_cube_compress): the render of both contribution
sources against an independent numpy restatement of include/rts_amd.h (RtsWaveform) fed by the ORACLE's rays and literal
aggregation, its ties to the impulse cube, a known-answer Doppler phase, determinism after the fused pulse end, ray sharding
with rts_cube_reduce, the matched filter against numpy, and the error / lifetime rules."""
import ctypes as C
import math

import numpy as np
import pytest

import helpers as H
from test_waveform_host import h_ref

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def scenes():
    from rts_amd import scenes as S
    return S


# ----------------------------------------------------------------------------- numpy restatement
def envelope_local(s, L, x):
    """s(x) = sum_m s[m] h_L(x - m) over the taps that can be non-zero (m within L/2 + 1 of x)"""
    s = np.asarray(s, np.complex128); M = len(s); hl = L // 2
    m = np.floor(x)[:, None].astype(np.int64) + np.arange(-hl - 1, hl + 2)[None, :]
    ok = (m >= 0) & (m < M)
    h = h_ref(x[:, None] - m, L) * ok
    return (h * s[np.clip(m, 0, M - 1)]).sum(axis=1)


def render_ref(cube, pulse, contribs, s, L, t0, dt, doppler):
    """cube[rx, pulse, n] += a s(n - d) e^{j 2 pi f (n - d) dt}, d = (tau - t0) / dt, for every (rx, a, tau, f)"""
    n_bins = cube.shape[2]; M = len(s)
    q0 = 0 if L == 1 else 1 - L // 2
    for rx, a, tau, f in contribs:
        if rx < 0 or rx >= cube.shape[0]:
            continue
        d = (tau - t0) / dt
        if not math.isfinite(d):
            continue
        D = math.floor(d)
        lo, hi = max(D + q0, 0), min(D + q0 + L - 1 + M - 1, n_bins - 1)
        if lo > hi:
            continue
        n = np.arange(lo, hi + 1, dtype=np.float64)
        y = a * envelope_local(s, L, n - d)
        if doppler:
            y = y * np.exp(2j * np.pi * f * ((n - d) * dt))
        cube[rx, pulse, lo:hi + 1] += y
    return cube


def contribs_rays(rx_records, cspeed, carrier):
    out = []
    for r in rx_records:
        tau = r["rayLength"] / cspeed
        ph = -math.fmod(tau * 2 * math.pi * carrier, 2 * math.pi)
        out.append((int(r["received"]), math.sqrt(r["power"]) * complex(math.cos(ph), math.sin(ph)), tau, float(r["doppler"])))
    return out


def contribs_paths(lit):
    res, pm = lit["results"], lit["pathMatch"]
    out = []
    for i in range(len(res)):
        if int(pm[i]) != i:
            continue
        ph = float(lit["phase"][i])
        out.append((int(res[i]["received"]), math.sqrt(res[i]["power"]) * complex(math.cos(ph), math.sin(ph)), float(lit["delay"][i]), float(res[i]["doppler"])))
    return out


def correlate_ref(y, s):
    """z[n] = sum_m y[n + m] conj(s[m]), y = 0 past its end"""
    return np.correlate(y, s, "full")[len(s) - 1:len(s) - 1 + len(y)]


def zeros_cube(shape):
    import torch
    return torch.zeros(shape, dtype=torch.complex128, device="cuda")


def host(buf):
    return buf.cpu().numpy()


def moved(spec, k, step=0.5):
    return [dict(position=tuple(np.add(m["position"], (step * k, 0, 0))), velocity=m["velocity"]) for m in spec["motion"]]


T0, DT, NB = 1.1e-6, 5.0e-9, 224


# ----------------------------------------------------------------------------- 1. against the restatement
def test_render_against_oracle_restatement(rts, oracle, scenes):
    spec = scenes.config_multi(W=20)
    cs, fc = spec["c"], spec["carrier"]; wl = cs / fc
    n_rx, n_p = len(spec["rx"]), 3
    rng = np.random.default_rng(5)
    waves = [rts.Waveform(rng.standard_normal(24) + 1j * rng.standard_normal(24), 8), rts.Waveform.lfm(48, 0.6, 16)]
    combos = [(w, dop) for w in waves for dop in (False, True)]
    tr = H.gpu_tracer(rts, spec); tp = H.gpu_tracer(rts, spec)
    bufs = {(src, j): zeros_cube((n_rx, n_p, NB)) for src in ("rays", "paths") for j in range(len(combos))}
    want = {key: np.zeros((n_rx, n_p, NB), np.complex128) for key in bufs}
    for k in range(n_p):
        mo = moved(spec, k)
        for t in (tr, tp):
            H.gpu_trace(rts, spec, tr=t, motion=mo)
            t.finalise_uniform(None, wl, 1.0, 1.0, fc, cs)
        tp.aggregate(cs, fc)
        o = H.oracle_trace(oracle, spec, motion=mo)
        rx, rxi, _ = oracle.filter_finalise(o["results"], o["path"], [1.0] * len(spec["meshes"]), wl, 1.0, 1.0, fc, cs)
        lit = oracle.aggregate_literal(rx, rxi, cs, fc, spec["W"] ** 3)
        cr, cp = contribs_rays(rx, cs, fc), contribs_paths(lit)
        for j, (w, dop) in enumerate(combos):
            for src, t, cb in (("rays", tr, cr), ("paths", tp, cp)):
                t.cube_attach(n_rx, n_p, NB, T0, DT, device_ptr=bufs[(src, j)].data_ptr())
                t.cube_set_waveform(w)
                t.cube_render(k, src, cs, fc, doppler=dop)
                render_ref(want[(src, j)], k, cb, w.samples, w.taps, T0, DT, dop)
    tr.cube(); tp.cube()                      # (the handles' streams drained: the torch reads below see every render)
    for key, buf in bufs.items():
        got, ref = host(buf), want[key]
        assert np.count_nonzero(ref) > 50, key
        np.testing.assert_allclose(got, ref, rtol=1e-10, atol=1e-12 * np.abs(ref).max(), err_msg=str(key))
    # the Doppler term is visible, and the two sources differ (by design)
    assert not np.allclose(want[("rays", 2)], want[("rays", 3)], rtol=1e-10, atol=0)
    assert not np.allclose(want[("rays", 0)], want[("paths", 0)])
    tr.close(); tp.close()


# ----------------------------------------------------------------------------- 2. ties to the impulse cube
def test_unit_sample_and_hold_equals_the_impulse_cube(rts, scenes):
    spec = scenes.config_multi(W=20)
    cs, fc = spec["c"], spec["carrier"]; wl = cs / fc
    n_rx, n_p, nb = len(spec["rx"]), 3, 64
    one = rts.Waveform([1.0 + 0.0j], 1)
    out = {}
    for src in ("rays", "paths"):
        ta = H.gpu_tracer(rts, spec); ta.cube_attach(n_rx, n_p, nb, T0, DT)
        tb = H.gpu_tracer(rts, spec); tb.cube_attach(n_rx, n_p, nb, T0, DT); tb.cube_set_waveform(one)
        for k in range(n_p):
            for t in (ta, tb):
                H.gpu_trace(rts, spec, tr=t, motion=moved(spec, k))
                t.finalise_uniform(None, wl, 1.0, 1.0, fc, cs)
            if src == "rays":
                ta.cube_accumulate(k, cs, fc); tb.cube_render(k, "rays", cs, fc, doppler=False)
            else:
                ta.aggregate(cs, fc); tb.aggregate(cs, fc)
                ta.cube_accumulate_paths(k); tb.cube_render(k, "paths", doppler=False)
        a, b = ta.cube(), tb.cube()
        assert np.count_nonzero(a) >= 3, src
        assert np.array_equal(a != 0, b != 0), src                                  # the same cells
        np.testing.assert_allclose(b, a, rtol=1e-12, atol=1e-12 * np.abs(a).max(), err_msg=src)
        out[src] = a
        ta.close(); tb.close()
    assert not np.allclose(out["rays"], out["paths"])


# ----------------------------------------------------------------------------- 3. known-answer Doppler
def test_doppler_phase_advances_by_2_pi_f_dt(rts, scenes):
    spec = scenes.config_multi(W=20)
    cs, fc = spec["c"], spec["carrier"]
    M, nb = 40, NB
    tr = H.gpu_tracer(rts, spec); tr.cube_attach(len(spec["rx"]), 1, nb, T0, DT)
    H.gpu_trace(rts, spec, tr=tr)
    rec = tr.received()["results"]
    picks, fs = [], {0: 2.0e6, 1: -3.5e6}
    for rx in (0, 1):
        for i, r in enumerate(rec):
            d = (r["rayLength"] / cs - T0) / DT
            if r["received"] == rx and 0 <= d < nb - M:
                picks.append(i); break
    assert len(picks) == 2
    power = np.zeros(len(rec)); doppler = np.zeros(len(rec))
    for i in picks:
        power[i] = 4.0; doppler[i] = fs[int(rec[i]["received"])]
    tr.finalise_values(power, doppler)
    tr.cube_set_waveform(rts.Waveform(np.full(M, 1.0 + 0.0j), 1))
    tr.cube_render(0, "rays", cs, fc, doppler=True)
    cube = tr.cube()
    for i in picks:
        rx = int(rec[i]["received"]); f = fs[rx]
        tau = rec[i]["rayLength"] / cs; d = (tau - T0) / DT; D = math.floor(d)
        row = cube[rx, 0]
        assert np.count_nonzero(row) == M and np.count_nonzero(row[D:D + M]) == M
        seg = row[D:D + M]
        np.testing.assert_allclose(np.abs(seg), 2.0, rtol=1e-12)
        step = np.angle(seg[1:] * np.conj(seg[:-1]))
        np.testing.assert_allclose(step, 2 * math.pi * f * DT, rtol=1e-9, atol=1e-12)
        ph = -math.fmod(tau * 2 * math.pi * fc, 2 * math.pi)
        np.testing.assert_allclose(seg[0], 2.0 * np.exp(1j * (ph + 2 * math.pi * f * (D - d) * DT)), rtol=1e-12)
    tr.close()


# ----------------------------------------------------------------------------- 4. determinism, fused pulse end
def test_render_is_deterministic_and_fused_equals_separate(rts, scenes):
    spec = scenes.config_multi(W=20)
    cs, fc = spec["c"], spec["carrier"]; wl = cs / fc; tx = spec["tx"]
    n_rx, n_p = len(spec["rx"]), 4
    w = rts.Waveform.lfm(64, 0.5, 16)
    tr = H.gpu_tracer(rts, spec); H.gpu_trace(rts, spec, tr=tr); tr.finalise_uniform(None, wl, 1.0, 1.0, fc, cs)
    tr.cube_set_waveform(w)
    a, b = zeros_cube((n_rx, 1, NB)), zeros_cube((n_rx, 1, NB))
    for buf in (a, b):
        tr.cube_attach(n_rx, 1, NB, T0, DT, device_ptr=buf.data_ptr()); tr.cube_render(0, "rays", cs, fc)
    tr.cube()
    assert np.count_nonzero(host(a)) > 50 and np.array_equal(host(a), host(b))
    tr.close()
    # the fused pulse end (its chain on the device-side count from the second pulse on) against the separate calls
    out = {}
    for mode in ("separate", "fused"):
        t = H.gpu_tracer(rts, spec); t.cube_set_waveform(w)
        bufs = {src: zeros_cube((n_rx, n_p, NB)) for src in ("rays", "paths")}
        for k in range(n_p):
            t.trace_begin(tx["origin"], tx["span"], tx["dir"], moved(spec, k))
            if mode == "separate":
                t.trace_end(); t.finalise_uniform(None, wl, 1.0, 1.0, fc, cs); t.aggregate(cs, fc)
            else:
                t.trace_end_uniform(None, wl, 1.0, 1.0, fc, cs, cube_pulse=-1)
            for src in ("rays", "paths"):
                t.cube_attach(n_rx, n_p, NB, T0, DT, device_ptr=bufs[src].data_ptr())
                t.cube_render(k, src, cs, fc)
        t.cube()
        out[mode] = {src: host(buf) for src, buf in bufs.items()}
        t.close()
    for src in ("rays", "paths"):
        assert np.count_nonzero(out["separate"][src]) > 50
        assert np.array_equal(out["separate"][src], out["fused"][src]), src


# ----------------------------------------------------------------------------- 5. ray sharding + rts_cube_reduce
def test_sharded_renders_reduce_to_the_whole(rts, scenes):
    from rts_amd import _lib
    spec = scenes.config_multi(W=16)
    cs, fc = spec["c"], spec["carrier"]; wl = cs / fc; tx = spec["tx"]
    n_rx = len(spec["rx"])
    w = rts.Waveform.lfm(32, 0.5, 16)
    trs = []
    for part in range(3):
        t = H.gpu_tracer(rts, spec); t.cube_attach(n_rx, 2, NB, T0, DT); t.cube_set_waveform(w)
        t.trace(tx["origin"], tx["span"], tx["dir"], spec["motion"], interleave=(64, 3, part), want_stats=False)
        t.finalise_uniform(None, wl, 1.0, 1.0, fc, cs); t.cube_render(1, "rays", cs, fc)
        trs.append(t)
    parts = [t.cube() for t in trs]
    whole = H.gpu_tracer(rts, spec); whole.cube_attach(n_rx, 2, NB, T0, DT); whole.cube_set_waveform(w)
    whole.trace(tx["origin"], tx["span"], tx["dir"], spec["motion"], want_stats=False)
    whole.finalise_uniform(None, wl, 1.0, 1.0, fc, cs); whole.cube_render(1, "rays", cs, fc)
    arr = (C.c_void_p * 3)(*[t.h for t in trs])
    _lib.check(_lib.lib().rts_cube_reduce(arr, 3, 2))
    want = parts[0] + parts[1] + parts[2]
    for t in trs:
        assert np.array_equal(t.cube(), want)
    ref = whole.cube()
    assert np.count_nonzero(ref) > 50
    np.testing.assert_allclose(want, ref, rtol=1e-9, atol=1e-12 * np.abs(ref).max())
    for t in trs + [whole]:
        t.close()


# ----------------------------------------------------------------------------- 6. range compression
@pytest.mark.parametrize("n_rx,n_p,nb,M,L", [(2, 3, 64, 16, 1), (3, 5, 1000, 77, 8), (1, 2, 8192, 4096, 16), (2, 4, 8192, 300, 2), (1, 3, 37, 100, 1)])
def test_compress_against_numpy(rts, n_rx, n_p, nb, M, L):
    rng = np.random.default_rng(nb + M)
    data = rng.standard_normal((n_rx, n_p, nb)) + 1j * rng.standard_normal((n_rx, n_p, nb))
    s = rng.standard_normal(M) + 1j * rng.standard_normal(M)
    import torch
    buf = torch.from_numpy(np.ascontiguousarray(data)).cuda()
    t = rts.Tracer(8, 1); t.cube_attach(n_rx, n_p, nb, 0.0, 1.0, device_ptr=buf.data_ptr()); t.cube_set_waveform(rts.Waveform(s, L))
    first, count = (1, n_p - 1) if n_p > 2 else (0, n_p)
    t.cube_compress(first, count)
    got = t.cube()                            # (rts_cube_get drains the handle's stream first)
    for r in range(n_rx):
        for p in range(n_p):
            if first <= p < first + count:
                want = correlate_ref(data[r, p], s)
                np.testing.assert_allclose(got[r, p], want, rtol=0, atol=1e-13 * M * np.abs(data).max() * np.abs(s).max())
            else:
                assert np.array_equal(got[r, p], data[r, p])                 # rows outside the range are untouched
    t.close()


def test_on_grid_response_peaks_at_its_delay(rts, scenes):
    """sample-and-hold puts an on-grid copy a s[m] at floor(d) + m; the matched filter peaks there with a sum |s|^2"""
    spec = scenes.config_multi(W=20)
    cs, fc = spec["c"], spec["carrier"]
    s = rts.Waveform.lfm(64, 0.8, 1)
    tr = H.gpu_tracer(rts, spec); tr.cube_attach(len(spec["rx"]), 1, NB, T0, DT); tr.cube_set_waveform(s)
    H.gpu_trace(rts, spec, tr=tr)
    rec = tr.received()["results"]
    i = next(i for i, r in enumerate(rec) if 5 <= (r["rayLength"] / cs - T0) / DT < NB - 70)
    power = np.zeros(len(rec)); power[i] = 9.0
    tr.finalise_values(power, np.zeros(len(rec)))
    tr.cube_render(0, "rays", cs, fc, doppler=False)
    tr.cube_compress()
    z = tr.cube()[int(rec[i]["received"]), 0]
    tau = rec[i]["rayLength"] / cs; n0 = math.floor((tau - T0) / DT)
    ph = -math.fmod(tau * 2 * math.pi * fc, 2 * math.pi); a = 3.0 * complex(math.cos(ph), math.sin(ph))
    assert int(np.argmax(np.abs(z))) == n0
    np.testing.assert_allclose(z[n0], a * np.sum(np.abs(s.samples) ** 2), rtol=1e-12)
    tr.close()


def test_render_compress_doppler_map(rts, scenes):
    """16 pulses of a moving target rendered (paths, Doppler on), range-compressed and Doppler-transformed: the strongest
    response's range peak lies within one bin of its delay, pulse by pulse and in the range-Doppler map"""
    spec = scenes.config_multi(W=20)
    cs, fc = spec["c"], spec["carrier"]; wl = cs / fc
    n_rx, n_p = len(spec["rx"]), 16
    w = rts.Waveform.lfm(64, 0.6, 16)
    tr = H.gpu_tracer(rts, spec); tr.cube_attach(n_rx, n_p, NB, T0, DT); tr.cube_set_waveform(w)
    strongest = []
    for k in range(n_p):
        H.gpu_trace(rts, spec, tr=tr, motion=moved(spec, k, step=0.02))
        tr.finalise_uniform(None, wl, 1.0, 1.0, fc, cs)
        resp = rts.groups_to_responses(tr.aggregate(cs, fc))
        j = int(np.argmax(resp["power"]))
        strongest.append((int(resp["rx"][j]), (float(resp["delay"][j]) - T0) / DT))
        tr.cube_render(k, "paths", doppler=True)
    tr.cube_compress()
    z = tr.cube()
    for k, (rx, d) in enumerate(strongest):
        assert abs(int(np.argmax(np.abs(z[rx, k]))) - d) <= 1.0, (k, rx, d)
    rd = tr.cube_doppler(16)
    rx0 = strongest[0][0]
    kk, nn = np.unravel_index(int(np.argmax(np.abs(rd[rx0]))), rd[rx0].shape)
    assert abs(nn - np.mean([d for r, d in strongest if r == rx0])) <= 1.0, (kk, nn, strongest)
    tr.close()


# ----------------------------------------------------------------------------- 7. errors and lifetime
def test_errors_and_lifetime(rts, scenes):
    from rts_amd import _lib as L
    lib = L.lib()
    spec = scenes.config_multi(W=16)
    cs, fc = spec["c"], spec["carrier"]; wl = cs / fc
    n_rx = len(spec["rx"])
    w1, w2 = rts.Waveform.lfm(32, 0.5, 16), rts.Waveform(np.exp(1j * np.arange(20) * 0.3), 4)
    tr = H.gpu_tracer(rts, spec)
    H.gpu_trace(rts, spec, tr=tr); tr.finalise_uniform(None, wl, 1.0, 1.0, fc, cs)
    # no cube, no waveform
    assert lib.rts_cube_render(tr.h, 0, 0, 0, cs, fc) == L.RTS_ERR_INVALID and b"attach" in lib.rts_last_error()
    assert lib.rts_cube_compress(tr.h, 0, 1) == L.RTS_ERR_INVALID
    tr.cube_attach(n_rx, 2, NB, T0, DT)
    assert lib.rts_cube_render(tr.h, 0, 0, 0, cs, fc) == L.RTS_ERR_INVALID and b"waveform" in lib.rts_last_error()
    assert lib.rts_cube_compress(tr.h, 0, 1) == L.RTS_ERR_INVALID and b"waveform" in lib.rts_last_error()
    # malformed waveforms are refused
    bad = [rts.Waveform([], 1), rts.Waveform(np.ones(4097), 1), rts.Waveform([1.0, math.nan], 1), rts.Waveform([1.0], 3),
           rts.Waveform([1.0], 0), rts.Waveform([1.0], 66)]
    for b in bad:
        with pytest.raises(L.RtsError):
            tr.cube_set_waveform(b)
    d = w1.desc(); d.reserved[1] = 1
    assert lib.rts_cube_set_waveform(tr.h, C.byref(d)) == L.RTS_ERR_INVALID
    tr.cube_set_waveform(w1)
    # pulses outside the cube, unknown source / flags, paths before rts_aggregate
    assert lib.rts_cube_render(tr.h, 2, 0, 0, cs, fc) == L.RTS_ERR_INVALID
    assert lib.rts_cube_render(tr.h, 0, 2, 0, cs, fc) == L.RTS_ERR_INVALID
    assert lib.rts_cube_render(tr.h, 0, 0, 2, cs, fc) == L.RTS_ERR_INVALID
    assert lib.rts_cube_render(tr.h, 0, L.RTS_RENDER_PATHS, 0, cs, fc) == L.RTS_ERR_INVALID and b"rts_aggregate" in lib.rts_last_error()
    assert lib.rts_cube_compress(tr.h, 2, 1) == L.RTS_ERR_INVALID and lib.rts_cube_compress(tr.h, 1, 2) == L.RTS_ERR_INVALID
    assert lib.rts_cube_compress(tr.h, 0, 0xffffffff) == L.RTS_ERR_INVALID
    assert np.count_nonzero(tr.cube()) == 0                                   # nothing was written by the refused calls
    # a refused waveform keeps the previous one; a waveform replaced between pulses renders each pulse with its own
    with pytest.raises(L.RtsError):
        tr.cube_set_waveform(rts.Waveform([1.0], 5))
    tr.cube_render(0, "rays", cs, fc)
    rays0 = tr.received()["results"]
    H.gpu_trace(rts, spec, tr=tr, motion=moved(spec, 1)); tr.finalise_uniform(None, wl, 1.0, 1.0, fc, cs)
    tr.cube_set_waveform(w2)
    tr.cube_render(1, "rays", cs, fc)
    rays1 = tr.received()["results"]
    want = np.zeros((n_rx, 2, NB), np.complex128)
    render_ref(want, 0, contribs_rays(rays0, cs, fc), w1.samples, w1.taps, T0, DT, True)
    render_ref(want, 1, contribs_rays(rays1, cs, fc), w2.samples, w2.taps, T0, DT, True)
    np.testing.assert_allclose(tr.cube(), want, rtol=1e-10, atol=1e-12 * np.abs(want).max())
    # too many range bins for the matched filter
    big = rts.Tracer(8, 1); big.cube_attach(1, 1, 8193, 0.0, 1.0); big.cube_set_waveform(w1)
    assert lib.rts_cube_compress(big.h, 0, 1) == L.RTS_ERR_INVALID and b"8192" in lib.rts_last_error()
    big.close()
    # a closed handle
    tr.close()
    for call in (lambda: tr.cube_set_waveform(w1), lambda: tr.cube_render(0, "rays", cs, fc), lambda: tr.cube_compress(0, 1)):
        with pytest.raises(L.RtsError):
            call()
    with pytest.raises(ValueError):
        rts.Tracer(8, 1).cube_render(0, "rays")
