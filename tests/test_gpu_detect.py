"""Receiver noise and CFAR detection on the device (rts_cube_add_noise, rts_cube_detect, rts_cube_detections_get): the noise against
rts_noise_eval, its determinism and row splits; the detector against an independent numpy restatement of include/rts_amd.h
(RtsCfarParams) on planted maps, across 120 dB of dynamic range, its false-alarm rate end to end, a moving target end to end, the
two map sources, and the error / lifetime rules."""
import ctypes as C
import math

import numpy as np
import pytest

import helpers as H

pytestmark = pytest.mark.gpu


def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, np.complex128)).to("cuda")


def zeros_cube(shape):
    import torch
    return torch.zeros(shape, dtype=torch.complex128, device="cuda")


def handle(rts, n_rx, n_p, nb, t0=0.0, dt=1.0, device_ptr=None):
    tr = rts.Tracer(8, 1)
    tr.cube_attach(n_rx, n_p, nb, t0, dt, device_ptr=device_ptr)
    return tr


# ----------------------------------------------------------------------------- numpy restatement of the detector
def window_sums(P, gr, gd, tr, td):
    """direct sums over the training annulus: (left half dr < 0, right half dr > 0, centre dr = 0) and their cell counts"""
    n_rx, nd, nb = P.shape
    Or, Od = gr + tr, gd + td
    S = {h: np.zeros(P.shape) for h in "lrc"}
    N = {h: np.zeros(nb, np.int64) for h in "lrc"}
    r = np.arange(nb)
    for dk in range(-Od, Od + 1):
        rolled = np.roll(P, -dk, axis=1)                      # rolled[:, k] = P[:, (k + dk) mod nd]
        for dr in range(-Or, Or + 1):
            if abs(dk) <= gd and abs(dr) <= gr:
                continue
            ok = (r + dr >= 0) & (r + dr < nb)
            v = np.zeros(P.shape)
            v[:, :, ok] = rolled[:, :, r[ok] + dr]
            h = "l" if dr < 0 else "r" if dr > 0 else "c"
            S[h] += v
            N[h] += ok
    return S, N


def cfar_ref(P, gr, gd, tr, td, mode="ca", pfa=None, alpha=None, local_max=False):
    """every cell's (noise, threshold, n_train) and the detection mask"""
    S, N = window_sums(P, gr, gd, tr, td)
    n = (N["l"] + N["r"] + N["c"])[None, None, :].astype(np.float64)
    if mode == "ca":
        noise = (S["l"] + S["r"] + S["c"]) / n
    else:
        with np.errstate(invalid="ignore", divide="ignore"):
            ml, mr = S["l"] / N["l"], S["r"] / N["r"]
        pick = np.maximum(ml, mr) if mode == "go" else np.minimum(ml, mr)
        noise = np.where(N["l"] == 0, mr, np.where(N["r"] == 0, ml, pick))
    a = n * np.expm1(-math.log(pfa) / n) if pfa is not None else alpha
    thr = a * noise
    det = P > thr
    if local_max:
        nb = P.shape[2]
        for dk in (-1, 0, 1):
            for dr in (-1, 0, 1):
                if dk == 0 and dr == 0:
                    continue
                q = np.roll(P, -dk, axis=1)
                q = np.roll(q, -dr, axis=2)
                below = dk < 0 or (dk == 0 and dr < 0)
                cmp = P > q if below else P >= q
                if dr == -1:
                    cmp[:, :, 0] = True                         # (range truncated: no neighbour)
                if dr == 1:
                    cmp[:, :, nb - 1] = True
                det &= cmp
    return noise, thr, np.broadcast_to(n, P.shape), det


def delta_ref(pm, p0, pp):
    if pm is None or pp is None or pm <= 0 or p0 <= 0 or pp <= 0:
        return 0.0
    lm, l0, lp = math.log(pm), math.log(p0), math.log(pp)
    den = lm - 2 * l0 + lp
    if den >= 0:
        return 0.0
    return min(0.5, max(-0.5, 0.5 * (lm - lp) / den))


def detections_ref(P, noise, thr, n, det, t0, dt, pri):
    nd, nb = P.shape[1], P.shape[2]
    out = []
    for rx, k, r in zip(*np.nonzero(det)):                    # C order: ascending flat (rx, k, r)
        p0 = P[rx, k, r]
        d_r = delta_ref(P[rx, k, r - 1] if r >= 1 else None, p0, P[rx, k, r + 1] if r + 1 < nb else None)
        d_d = delta_ref(P[rx, (k - 1) % nd, r], p0, P[rx, (k + 1) % nd, r])
        w = k + d_d
        if w >= nd / 2:
            w -= nd
        elif w < -nd / 2:
            w += nd
        out.append((rx, k, r, int(n[rx, k, r]), p0, noise[rx, k, r], thr[rx, k, r], d_r, d_d, t0 + (r + d_r) * dt,
                    w / (nd * pri) if pri > 0 else 0.0))
    from rts_amd import _lib as L
    return np.array(out, dtype=L.DETECTION_DTYPE) if out else np.zeros(0, L.DETECTION_DTYPE)


def assert_margin(P, thr, rel=1e-9):
    """no cell sits within rel of its threshold: the decision cannot depend on rounding"""
    assert np.all(np.abs(P - thr) > rel * np.abs(thr)), "a cell lies on its threshold"


def assert_same_list(got, want):
    assert len(got) == len(want), (len(got), len(want))
    for f in ("rx", "doppler_bin", "range_bin", "n_train"):
        assert np.array_equal(got[f], want[f]), f
    for f in ("power", "noise", "threshold", "range_offset", "doppler_offset", "delay", "doppler"):
        scale = max(np.abs(want[f]).max(initial=0.0), 1e-300)
        np.testing.assert_allclose(got[f], want[f], rtol=1e-12, atol=1e-12 * scale if f in ("range_offset", "doppler_offset", "doppler") else 0, err_msg=f)


def planted_map(rng, n_rx, nd, nb, noise_power=1.0, snr=1e3):
    """exponential noise, targets with sloped neighbours at the Doppler wrap and the range edges, and a 2 x 2 plateau"""
    z = rng.standard_normal((n_rx, nd, nb)) + 1j * rng.standard_normal((n_rx, nd, nb))
    z *= math.sqrt(noise_power / 2)
    amp = math.sqrt(snr * noise_power)
    for rx in range(n_rx):
        for k, r in ((0, 0), (nd - 1, nb - 1), (0, nb - 1), (nd - 1, 0), (nd // 2, nb // 2 + 3)):
            z[rx, k, r] = amp * np.exp(1j * rng.uniform(0, 2 * np.pi))
            for dk, dr, f in ((0, -1, 0.6), (0, 1, 0.35), (-1, 0, 0.5), (1, 0, 0.3)):
                if 0 <= r + dr < nb:
                    z[rx, (k + dk) % nd, r + dr] = f * amp
        kp, rp = min(3, nd - 2), min(20, nb - 3)
        z[rx, kp:kp + 2, rp:rp + 2] = 0.8 * amp                # plateau of equal cells
    return z


CASES = [  # mode, local max, (Gr, Gd), (Tr, Td), n_rx, n_doppler, n_bins, pfa, alpha
    ("ca", False, (2, 2), (8, 4), 2, 64, 300, 1e-3, None),
    ("ca", True, (1, 0), (3, 2), 3, 8, 200, 1e-2, None),
    ("go", True, (3, 1), (5, 6), 2, 37, 150, None, 8.0),
    ("so", False, (0, 2), (16, 0), 2, 24, 90, None, 5.0),
    ("ca", True, (0, 0), (0, 16), 2, 1024, 70, 1e-4, None),
    ("go", False, (0, 3), (16, 13), 1, 100, 40, None, 6.0),
    ("so", True, (4, 0), (2, 1), 2, 12, 129, None, 4.0),
    ("ca", False, (16, 0), (0, 1), 1, 3, 64, None, 3.0),
]


@pytest.mark.parametrize("mode,local_max,guard,train,n_rx,nd,nb,pfa,alpha", CASES)
def test_cfar_against_restatement(rts, mode, local_max, guard, train, n_rx, nd, nb, pfa, alpha):
    rng = np.random.default_rng(nd * 1000 + nb)
    z = planted_map(rng, n_rx, nd, nb)
    P = z.real * z.real + z.imag * z.imag
    t0, dt, pri = 2.0e-6, 5.0e-9, 1.0e-3
    noise, thr, n, det = cfar_ref(P, guard[0], guard[1], train[0], train[1], mode, pfa, alpha, local_max)
    assert_margin(P, thr)
    want = detections_ref(P, noise, thr, n, det, t0, dt, pri)
    assert len(want) >= 5 * n_rx
    m = dev(z)
    tr = handle(rts, n_rx, 1, nb, t0, dt)
    got = tr.cube_detect(guard, train, mode, pfa=pfa, alpha=alpha, local_max=local_max, pri=pri, device_ptr=m.data_ptr(), n_doppler=nd)
    assert_same_list(got, want)
    if local_max:                                              # one detection per plateau
        kp, rp = min(3, nd - 2), min(20, nb - 3)
        sel = (got["doppler_bin"] >= kp) & (got["doppler_bin"] <= kp + 1) & (got["range_bin"] >= rp) & (got["range_bin"] <= rp + 1)
        assert np.count_nonzero(sel) <= n_rx
    tr.close()


@pytest.mark.parametrize("mode", ["ca", "go", "so"])
def test_dynamic_range_of_the_noise_estimate(rts, mode):
    """a cell 10^12 x the noise in the guard or training window of its neighbours: every cell's estimate still matches the direct
    sums of the restatement (alpha small enough that every cell is reported; SO takes the quiet half)"""
    rng = np.random.default_rng(7)
    n_rx, nd, nb = 2, 32, 128
    z = (rng.standard_normal((n_rx, nd, nb)) + 1j * rng.standard_normal((n_rx, nd, nb))) * math.sqrt(0.5)
    z[0, 5, 40] = 1e6
    z[1, 31, 0] = 1e6 * np.exp(0.3j)
    P = z.real * z.real + z.imag * z.imag
    g, t = (2, 2), (6, 3)
    noise, thr, n, det = cfar_ref(P, g[0], g[1], t[0], t[1], mode, None, 1e-20, False)
    assert det.all()
    assert_margin(P, thr)
    want = detections_ref(P, noise, thr, n, det, 0.0, 1.0, 0.0)
    m = dev(z)
    tr = handle(rts, n_rx, 1, nb)
    got = tr.cube_detect(g, t, mode, alpha=1e-20, local_max=False, device_ptr=m.data_ptr(), n_doppler=nd, max_detections=n_rx * nd * nb)
    assert_same_list(got, want)
    # the neighbours of the strong cell: inside its guard their estimates stay at the noise, in its window they carry it
    k = got[(got["rx"] == 0) & (got["doppler_bin"] == 5) & (got["range_bin"] == 41)]
    assert k["noise"][0] < 10.0
    k = got[(got["rx"] == 0) & (got["doppler_bin"] == 5) & (got["range_bin"] == 46)]
    assert k["noise"][0] > 1e9 if mode != "so" else k["noise"][0] < 10.0
    tr.close()


# ----------------------------------------------------------------------------- noise
def test_noise_matches_eval_and_splits(rts):
    n_rx, n_p, nb = 3, 7, 100
    tr = handle(rts, n_rx, n_p, nb)
    tr.cube_add_noise(2.0, 99)
    got = tr.cube()
    want = rts.noise_eval(99, np.arange(n_rx * n_p * nb, dtype=np.uint64), 2.0).reshape(n_rx, n_p, nb)
    np.testing.assert_allclose(got.real, want.real, rtol=1e-13, atol=1e-13)
    np.testing.assert_allclose(got.imag, want.imag, rtol=1e-13, atol=1e-13)
    # same seed twice: identical bytes; rows [0, 5) + [5, n) equal one call
    t2 = handle(rts, n_rx, n_p, nb)
    t2.cube_add_noise(2.0, 99, 0, 5); t2.cube_add_noise(2.0, 99, 5)
    assert got.tobytes() == t2.cube().tobytes()
    t3 = handle(rts, n_rx, n_p, nb); t3.cube_add_noise(2.0, 99)
    assert got.tobytes() == t3.cube().tobytes()
    # other rows untouched; power 0 is a no-op
    t4 = handle(rts, n_rx, n_p, nb)
    t4.cube_add_noise(2.0, 99, 2, 3); t4.cube_add_noise(0.0, 5)
    c4 = t4.cube()
    assert np.count_nonzero(c4[:, :2]) == 0 and np.count_nonzero(c4[:, 5:]) == 0
    assert c4[:, 2:5].tobytes() == got[:, 2:5].tobytes()
    # on a filled cube (caller memory): the cube plus the noise, to rounding of one addition
    rng = np.random.default_rng(3)
    pre = rng.standard_normal((n_rx, n_p, nb)) + 1j * rng.standard_normal((n_rx, n_p, nb))
    m = dev(pre)
    t5 = handle(rts, n_rx, n_p, nb, device_ptr=m.data_ptr())
    t5.cube_add_noise(2.0, 99)
    after = t5.cube()
    assert np.array_equal(after.real, pre.real + got.real) and np.array_equal(after.imag, pre.imag + got.imag)
    for t in (tr, t2, t3, t4, t5):
        t.close()


def test_false_alarm_rate_end_to_end(rts):
    """zeroed 4 x 256 x 2048 cube -> noise -> slow-time DFT (iid complex Gaussian) -> CA at pfa 1e-3: the count is binomial"""
    n_rx, n_p, nb, pfa = 4, 256, 2048, 1e-3
    tr = handle(rts, n_rx, n_p, nb)
    tr.cube_add_noise(1.0, 12345)
    tr.cube_doppler(256, fetch=False)
    got = tr.cube_detect((2, 2), (8, 4), "ca", pfa=pfa, local_max=False)
    cells = n_rx * n_p * nb
    mean, sd = cells * pfa, math.sqrt(cells * pfa * (1 - pfa))
    assert abs(len(got) - mean) < 5 * sd, (len(got), mean, sd)
    assert np.all(got["power"] > got["threshold"])
    edge = (got["range_bin"] < 10) | (got["range_bin"] >= nb - 10)      # range edges hold their share too
    assert np.count_nonzero(edge) > 0
    tr.close()


# ----------------------------------------------------------------------------- a scene, end to end
def test_moving_target_end_to_end(rts, oracle):
    """64 pulses of a target closing at constant velocity: trace, finalise, render (LFM), noise, compress, Doppler, CA at pfa 1e-6:
    the strongest detection of each receiver lies within a range bin of the strongest oracle group's mean delay (of its rays' delay
    span, for a group wider than a bin) and within a Doppler bin of -fc dtau / pri; a noise-only control detects nothing beyond the binomial bound"""
    from rts_amd import scenes as S
    spec = S.config_multi(W=16, max_refl=1)
    spec["meshes"], spec["motion"] = spec["meshes"][:1], spec["motion"][:1]          # the sphere alone
    cs, fc = spec["c"], spec["carrier"]; wl = cs / fc
    n_rx, n_p, nb, pri = len(spec["rx"]), 64, 224, 1e-3
    t0, dt = 1.1e-6, 5.0e-9
    v = 2.5                                                     # m/s towards the radar along -x
    assert 2 * v * fc / cs < 0.5 / pri                          # Doppler unaliased
    assert 2 * v * n_p * pri / cs < 0.5 * dt                    # range migration under half a bin
    w = rts.Waveform.lfm(32, 0.6, 16)
    tr = H.gpu_tracer(rts, spec); tr.cube_attach(n_rx, n_p, nb, t0, dt); tr.cube_set_waveform(w)
    motions = []
    for k in range(n_p):
        mo = [dict(position=tuple(np.add(m["position"], (-v * pri * k, 0.0, 0.0))), velocity=(-v, 0.0, 0.0)) for m in spec["motion"]]
        motions.append(mo)
        H.gpu_trace(rts, spec, tr=tr, motion=mo)
        tr.finalise_uniform(None, wl, 1.0, 1.0, fc, cs)
        tr.cube_render(k, "rays", cs, fc, doppler=True)
    lits = []
    for k in (0, n_p - 1):                                     # the oracle at the first and the last pulse
        o = H.oracle_trace(oracle, spec, motion=motions[k])
        rx, rxi, _ = oracle.filter_finalise(o["results"], o["path"], [1.0], wl, 1.0, 1.0, fc, cs)
        lits.append(oracle.aggregate_literal(rx, rxi, cs, fc, spec["W"] ** 3))
    noise_power = float((np.abs(tr.cube()) ** 2).max()) / 1e3         # 30 dB below the strongest sample, before compression
    tr.cube_add_noise(noise_power, 77)
    tr.cube_compress()
    tr.cube_doppler(n_p, fetch=False)
    got = tr.cube_detect((2, 2), (8, 4), "ca", pfa=1e-6, local_max=True, pri=pri)
    checked = 0
    for r in range(n_rx):
        strongest = []
        for lit in lits:
            res, pm = lit["results"], lit["pathMatch"]
            sel = [i for i in range(len(res)) if int(pm[i]) == i and int(res[i]["received"]) == r]
            strongest.append(max(sel, key=lambda i: res[i]["power"]) if sel else None)
        if strongest[0] is None or strongest[1] is None:
            continue
        d0, d1 = float(lits[0]["delay"][strongest[0]]), float(lits[1]["delay"][strongest[1]])
        # the group's rays at the first pulse: a wide bistatic group peaks where its rays crowd, not at their mean delay
        res0, pm0 = lits[0]["results"], lits[0]["pathMatch"]
        member = [res0[j]["rayLength"] / cs for j in range(len(res0)) if int(pm0[j]) == strongest[0]]
        lo, hi = (min(member) - t0) / dt, (max(member) - t0) / dt
        mine = got[got["rx"] == r]
        assert len(mine), r
        best = mine[np.argmax(mine["power"])]
        at = float(best["range_bin"]) + float(best["range_offset"])
        if hi - lo < 1.0:
            assert abs(int(best["range_bin"]) - ((d0 + d1) / 2 - t0) / dt) <= 1.0, (r, best, d0, d1)
        else:
            assert lo - 1.0 <= at <= hi + 1.0, (r, best, lo, hi)
        f_want = -fc * (d1 - d0) / (n_p - 1) / pri
        assert f_want > 0                                       # closing: positive Doppler
        assert abs(best["doppler"] - f_want) <= 1.0 / (n_p * pri), (r, best["doppler"], f_want)
        checked += 1
    assert checked >= 1
    # control: the same noise alone
    ctl = handle(rts, n_rx, n_p, nb, t0, dt); ctl.cube_set_waveform(w)
    ctl.cube_add_noise(noise_power, 77); ctl.cube_compress(); ctl.cube_doppler(n_p, fetch=False)
    none = ctl.cube_detect((2, 2), (8, 4), "ca", pfa=1e-6, local_max=True, pri=pri)
    cells = n_rx * n_p * nb
    assert len(none) <= cells * 1e-6 + 5 * math.sqrt(cells * 1e-6), len(none)
    tr.close(); ctl.close()


# ----------------------------------------------------------------------------- determinism, map sources
def test_determinism_and_map_sources(rts):
    n_rx, n_p, nb = 2, 16, 256
    tr = handle(rts, n_rx, n_p, nb, 1e-6, 1e-8)
    tr.cube_add_noise(1.0, 5)
    tr.cube_doppler(32, fetch=False)
    a = tr.cube_detect((1, 1), (4, 4), "ca", pfa=1e-2, local_max=True, pri=1e-3)
    b = tr.cube_detect((1, 1), (4, 4), "ca", pfa=1e-2, local_max=True, pri=1e-3)
    assert len(a) > 10 and a.tobytes() == b.tobytes()
    rd = tr.cube_doppler(32)
    m = dev(rd)
    c = tr.cube_detect((1, 1), (4, 4), "ca", pfa=1e-2, local_max=True, pri=1e-3, device_ptr=m.data_ptr(), n_doppler=32)
    assert a.tobytes() == c.tobytes()
    # the handle's transform into caller memory is the map of the next detection without a pointer
    out = zeros_cube((n_rx, 32, nb))
    tr.cube_doppler(32, device_ptr=out.data_ptr(), fetch=False)
    d = tr.cube_detect((1, 1), (4, 4), "ca", pfa=1e-2, local_max=True, pri=1e-3)
    assert a.tobytes() == d.tobytes()
    tr.close()


# ----------------------------------------------------------------------------- errors and lifetime
def test_errors_and_lifetime(rts):
    from rts_amd import _lib as L
    lib = L.lib()
    n_rx, nd, nb = 2, 16, 64
    rng = np.random.default_rng(1)
    z = planted_map(rng, n_rx, nd, nb)
    m = dev(z)
    mp = C.c_void_p(m.data_ptr())

    def params(gr=1, gd=1, tr_=4, td=2, mode=0, flags=0, pfa=1e-3, alpha=0.0, pri=0.0, max_det=0):
        p = L.RtsCfarParams()
        p.guard_range, p.guard_doppler, p.train_range, p.train_doppler = gr, gd, tr_, td
        p.mode, p.flags, p.pfa, p.alpha, p.pri, p.max_detections = mode, flags, pfa, alpha, pri, max_det
        return p

    def det(p, ptr_=mp, n=nd, h=None):
        return lib.rts_cube_detect((h or tr).h, C.byref(p), ptr_, n)

    tr = rts.Tracer(8, 1)
    n_out = C.c_uint32(0)
    # no cube; no list yet; noise without a cube
    assert det(params()) == L.RTS_ERR_INVALID and b"cube" in lib.rts_last_error()
    assert lib.rts_cube_add_noise(tr.h, 0, 1, 1.0, 1) == L.RTS_ERR_INVALID
    assert lib.rts_cube_detections_get(tr.h, None, 0, C.byref(n_out)) == L.RTS_ERR_INVALID
    tr.cube_attach(n_rx, 4, nb, 0.0, 1.0)
    # no map (no rts_cube_doppler) and no pointer; a pointer without n_doppler
    assert det(params(), None, 0) == L.RTS_ERR_INVALID and b"map" in lib.rts_last_error()
    assert det(params(), mp, 0) == L.RTS_ERR_INVALID and b"n_doppler" in lib.rts_last_error()
    assert lib.rts_cube_detect(tr.h, None, mp, nd) == L.RTS_ERR_INVALID
    cases = [
        (params(mode=3), b"mode"), (params(flags=2), b"flags"),
        (params(tr_=0, td=0), b"train"), (params(gr=9, tr_=8), b"guard_range"), (params(gd=10, td=7), b"guard_doppler"),
        (params(gd=4, td=4), b"n_doppler"), (params(gr=60, tr_=4), b"guard_range"),
        (params(pfa=1.0), b"pfa"), (params(pfa=-0.1), b"pfa"), (params(pfa=math.nan), b"pfa"),
        (params(pfa=1e-3, alpha=2.0), b"pfa"), (params(pfa=0.0, alpha=0.0), b"pfa"), (params(pfa=0.0, alpha=-1.0), b"alpha"),
        (params(mode=1, pfa=1e-3), b"pfa"), (params(mode=2, pfa=0.0, alpha=3.0, tr_=0, td=2), b"train_range"),
        (params(pri=-1.0), b"pri"), (params(pri=math.inf), b"pri"), (params(pri=math.nan), b"pri"),
    ]
    for p, word in cases:
        assert det(p) == L.RTS_ERR_INVALID, word
        assert word in lib.rts_last_error(), (word, lib.rts_last_error())
    for field in ("reserved0",):
        p = params(); setattr(p, field, 1)
        assert det(p) == L.RTS_ERR_INVALID and b"reserved" in lib.rts_last_error()
    p = params(); p.reserved[1] = 1
    assert det(p) == L.RTS_ERR_INVALID and b"reserved" in lib.rts_last_error()
    # Gr + Tr >= n_bins (a cube of 16 bins)
    small = handle(rts, 1, 1, 16)
    assert det(params(gr=4, tr_=12), mp, nd, small) == L.RTS_ERR_INVALID and b"n_bins" in lib.rts_last_error()
    small.close()
    # noise arguments
    for bad in (-1.0, math.nan, math.inf):
        assert lib.rts_cube_add_noise(tr.h, 0, 1, bad, 1) == L.RTS_ERR_INVALID and b"noise_power" in lib.rts_last_error()
    assert lib.rts_cube_add_noise(tr.h, 4, 1, 1.0, 1) == L.RTS_ERR_INVALID
    assert lib.rts_cube_add_noise(tr.h, 1, 4, 1.0, 1) == L.RTS_ERR_INVALID
    assert np.count_nonzero(tr.cube()) == 0
    # max_detections and capacity below the total: RTS_ERR_CAPACITY, *n_out = the total, the first K records in order
    full = tr.cube_detect((1, 1), (4, 2), "ca", pfa=1e-1, local_max=False, device_ptr=m.data_ptr(), n_doppler=nd)
    total = len(full)
    assert total > 20
    assert det(params(pfa=1e-1, max_det=7)) == L.RTS_OK
    out = np.zeros(total, L.DETECTION_DTYPE)
    assert lib.rts_cube_detections_get(tr.h, out.ctypes.data_as(C.c_void_p), total, C.byref(n_out)) == L.RTS_ERR_CAPACITY
    assert n_out.value == total and out[:7].tobytes() == full[:7].tobytes() and np.count_nonzero(out[7:]["power"]) == 0
    assert det(params(pfa=1e-1)) == L.RTS_OK
    out = np.zeros(total, L.DETECTION_DTYPE)
    assert lib.rts_cube_detections_get(tr.h, out.ctypes.data_as(C.c_void_p), 5, C.byref(n_out)) == L.RTS_ERR_CAPACITY
    assert n_out.value == total and out[:5].tobytes() == full[:5].tobytes() and np.count_nonzero(out[5:]["power"]) == 0
    assert lib.rts_cube_detections_get(tr.h, out.ctypes.data_as(C.c_void_p), total, C.byref(n_out)) == L.RTS_OK
    assert out.tobytes() == full.tobytes()
    assert lib.rts_cube_detections_get(tr.h, out.ctypes.data_as(C.c_void_p), total, None) == L.RTS_ERR_INVALID
    # a refused detection ends the previous list; so does rts_cube_attach
    assert det(params(mode=9)) == L.RTS_ERR_INVALID
    assert det(params(pfa=1e-1)) == L.RTS_OK
    tr.cube_attach(n_rx, 4, nb, 0.0, 1.0)
    assert lib.rts_cube_detections_get(tr.h, out.ctypes.data_as(C.c_void_p), total, C.byref(n_out)) == L.RTS_ERR_INVALID
    tr.close()
    with pytest.raises(L.RtsError):
        tr.cube_detect(device_ptr=m.data_ptr(), n_doppler=nd, pfa=1e-3)
    # nothing leaks across create / detect / destroy cycles
    import torch
    torch.cuda.synchronize()
    free0 = torch.cuda.mem_get_info()[0]
    for i in range(100):
        t = handle(rts, n_rx, 4, nb)
        t.cube_add_noise(1.0, i)
        t.cube_detect((1, 1), (4, 2), "ca", pfa=1e-2, device_ptr=m.data_ptr(), n_doppler=nd)
        t.close()
    torch.cuda.synchronize()
    assert free0 - torch.cuda.mem_get_info()[0] < 64 << 20
