"""Ordered-statistic CFAR on the device (rts_cube_detect_os, k_cfar_os): against the numpy restatement of include/rts_amd.h
(tests/cfar_os_ref.py) and, bit for bit, against the host evaluator rts_cfar_os_eval on eight shapes that cover the kernel's paths;
the masking that hides a target from cell averaging; both detectors' lists byte for byte on a map where their estimates coincide; the false-alarm rate and a moving target end to end; determinism, the two map
sources, the shared detection list; and the error / lifetime rules.

Integer fields, power and noise are compared exactly with the restatement (an order statistic has no summation order), the
threshold exactly when alpha is given and to 1e-11 relative with pfa (the restatement's alpha is its own bisection; 1e-11 is the
bound rts_cfar_os_alpha documents).  Against rts_cfar_os_eval every field but the refinement is byte-equal: both take their alphas
from one function.  Case 7 of the shared shapes carries extra planted cells: see tests/cfar_os_ref.py."""
import ctypes as C
import math

import numpy as np
import pytest

import cfar_os_ref as R
import helpers as H

pytestmark = pytest.mark.gpu
T0, DT, PRI = 2.0e-6, 5.0e-9, 1.0e-3
BYTE_EQUAL = ("rx", "doppler_bin", "range_bin", "n_train", "power", "noise", "threshold")


def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, np.complex128)).to("cuda")


def handle(rts, n_rx, n_p, nb, t0=0.0, dt=1.0, device_ptr=None):
    tr = rts.Tracer(8, 1)
    tr.cube_attach(n_rx, n_p, nb, t0, dt, device_ptr=device_ptr)
    return tr


# ----------------------------------------------------------------------------- against the restatement and the host evaluator
@pytest.mark.parametrize("index", range(len(R.CASES)))
def test_os_against_restatement_and_eval(rts, index):
    guard, train, _, n_rx, nd, nb, pfa, alpha, local_max = R.CASES[index]
    rank = R.case_rank(R.CASES[index])
    z, P, want = R.case_expectation(index, T0, DT, PRI)        # (checks the margin and the 5 n_rx detections)
    m = dev(z)
    tr = handle(rts, n_rx, 1, nb, T0, DT)
    got = tr.cube_detect_os(guard, train, rank, pfa=pfa, alpha=alpha, local_max=local_max, pri=PRI, device_ptr=m.data_ptr(), n_doppler=nd)
    tr.close()
    R.assert_same_list(got, want, threshold_rtol=0.0 if alpha is not None else 1e-11)
    host = rts.cfar_os_eval(z, guard, train, rank, pfa=pfa, alpha=alpha, local_max=local_max, pri=PRI, t0=T0, dt=DT)
    assert len(got) == len(host)
    for f in BYTE_EQUAL:
        assert got[f].tobytes() == host[f].tobytes(), f
    R.assert_same_list(got, host)
    if local_max:                                              # one detection per plateau
        kp, rp = min(3, nd - 2), min(20, nb - 3)
        sel = (got["doppler_bin"] >= kp) & (got["doppler_bin"] <= kp + 1) & (got["range_bin"] >= rp) & (got["range_bin"] <= rp + 1)
        assert np.count_nonzero(sel) <= n_rx


# ----------------------------------------------------------------------------- masking
def test_masking(rts):
    """five 40 dB cells and a 16 dB cell four bins from one of them: cell averaging at pfa 1e-4 reports the five and misses the
    weak cell, OS at rank 186 of 248 reports all six"""
    z, strong, weak = R.masking_map()
    m = dev(z)
    tr = handle(rts, 1, 1, 128)
    ca = tr.cube_detect((2, 2), (8, 4), "ca", pfa=1e-4, local_max=False, device_ptr=m.data_ptr(), n_doppler=32)
    assert sorted(zip(ca["doppler_bin"].tolist(), ca["range_bin"].tolist())) == sorted(strong)
    got = tr.cube_detect_os((2, 2), (8, 4), 186, pfa=1e-4, local_max=False, device_ptr=m.data_ptr(), n_doppler=32)
    assert sorted(zip(got["doppler_bin"].tolist(), got["range_bin"].tolist())) == sorted(strong + [weak])
    w = got[(got["doppler_bin"] == weak[0]) & (got["range_bin"] == weak[1])][0]
    assert abs(w["noise"] - 1.3017) < 1e-3 and abs(w["threshold"] - 8.94) < 1e-2 and w["n_train"] == 248
    tr.close()


# ----------------------------------------------------------------------------- false-alarm rate
def test_false_alarm_rate_end_to_end(rts):
    """zeroed 2 x 64 x 1 024 cube -> noise -> slow-time DFT (iid complex Gaussian of power 64: the transform is unnormalised) -> OS at
    rank 186 of 248, pfa 1e-2.  The detector is scale-free, so the count conditions are those of the host test: within 5 sd of the
    binomial mean, 1 310.72 +- 5 x 36.0, and between 1 and 51 in the first and last ten range bins.  The scale shows in the
    estimates: the 186th of 248 unit exponentials has mean sum_{i<186} 1 / (248 - i) = 1.38 and sd 0.11, so every reported noise
    lies within 64 x (1.38 +- 6 x 0.11)"""
    n_rx, n_p, nb, pfa = 2, 64, 1024, 1e-2
    tr = handle(rts, n_rx, n_p, nb)
    tr.cube_add_noise(1.0, 12345)
    tr.cube_doppler(64, fetch=False)
    got = tr.cube_detect_os((2, 2), (8, 4), 186, pfa=pfa, local_max=False)
    tr.close()
    cells = n_rx * n_p * nb
    mean, sd = cells * pfa, math.sqrt(cells * pfa * (1 - pfa))
    edge = int(np.count_nonzero((got["range_bin"] < 10) | (got["range_bin"] >= nb - 10)))
    print("false alarms: %d (%.2f sd from the mean), %d in the edge bins" % (len(got), (len(got) - mean) / sd, edge))
    assert abs(len(got) - mean) < 5 * sd, (len(got), mean, sd)
    assert 1 <= edge <= 51, edge
    assert np.all(got["power"] > got["threshold"])
    full = got[got["n_train"] == 248]
    q = sum(1.0 / (248 - i) for i in range(186))
    assert len(full) > 1000 and np.all(np.abs(full["noise"] / 64.0 - q) < 6 * 0.11), (full["noise"].min() / 64, full["noise"].max() / 64, q)


# ----------------------------------------------------------------------------- a scene, end to end
def test_moving_target_end_to_end(rts):
    """the chain of tests/test_gpu_detect.py's moving target -- 64 pulses of a sphere closing at constant velocity: trace, finalise,
    render (LFM), noise, compress, Doppler -- then both detectors on the same map at pfa 1e-6: every receiver's strongest OS
    detection has the doppler_bin and range_bin of its strongest CA detection"""
    from rts_amd import scenes as S
    spec = S.config_multi(W=16, max_refl=1)
    spec["meshes"], spec["motion"] = spec["meshes"][:1], spec["motion"][:1]          # the sphere alone
    cs, fc = spec["c"], spec["carrier"]; wl = cs / fc
    n_rx, n_p, nb, pri = len(spec["rx"]), 64, 224, 1e-3
    t0, dt = 1.1e-6, 5.0e-9
    v = 2.5                                                     # m/s towards the radar along -x
    w = rts.Waveform.lfm(32, 0.6, 16)
    tr = H.gpu_tracer(rts, spec); tr.cube_attach(n_rx, n_p, nb, t0, dt); tr.cube_set_waveform(w)
    for k in range(n_p):
        mo = [dict(position=tuple(np.add(m["position"], (-v * pri * k, 0.0, 0.0))), velocity=(-v, 0.0, 0.0)) for m in spec["motion"]]
        H.gpu_trace(rts, spec, tr=tr, motion=mo)
        tr.finalise_uniform(None, wl, 1.0, 1.0, fc, cs)
        tr.cube_render(k, "rays", cs, fc, doppler=True)
    noise_power = float((np.abs(tr.cube()) ** 2).max()) / 1e3         # 30 dB below the strongest sample, before compression
    tr.cube_add_noise(noise_power, 77)
    tr.cube_compress()
    tr.cube_doppler(n_p, fetch=False)
    ca = tr.cube_detect((2, 2), (8, 4), "ca", pfa=1e-6, local_max=True, pri=pri)
    got = tr.cube_detect_os((2, 2), (8, 4), None, pfa=1e-6, local_max=True, pri=pri)          # rank (3 N0) // 4 = 186
    tr.close()
    checked = 0
    for r in range(n_rx):
        a, b = ca[ca["rx"] == r], got[got["rx"] == r]
        if not len(a):
            continue
        assert len(b), r
        sa, sb = a[np.argmax(a["power"])], b[np.argmax(b["power"])]
        assert (sa["doppler_bin"], sa["range_bin"]) == (sb["doppler_bin"], sb["range_bin"]), (r, sa, sb)
        assert sa["power"] == sb["power"] and sb["doppler"] > 0          # (closing: positive Doppler)
        checked += 1
    assert checked >= 1


# ----------------------------------------------------------------------------- both detectors, one list
def flat_noise_map():
    """2 x 20 x 130, one tile and a bit on each axis: background 1, in receiver rx peaks of amplitude 10 + rx with sloped neighbours
    (3.0 at r - 1, 2.25 at r + 1, 2.5 at k - 1, 1.5 at k + 1; Doppler wrapped, range neighbours outside the map omitted)"""
    n_rx, nd, nb = 2, 20, 130
    peaks = [(0, 0), (3, 63), (8, 64), (15, 100), (16, 129), (19, 30)]
    z = np.ones((n_rx, nd, nb), np.complex128)
    for rx in range(n_rx):
        for k, r in peaks:
            z[rx, k, r] = 10.0 + rx
            for dk, dr, amp in ((0, -1, 3.0), (0, 1, 2.25), (-1, 0, 2.5), (1, 0, 1.5)):
                if 0 <= r + dr < nb:
                    z[rx, (k + dk) % nd, r + dr] = amp
    return z, peaks


def test_both_detectors_one_list(rts):
    """Every training cell of every peak of flat_noise_map is exactly 1.0 under guard (1, 1), train (2, 2): the mean (a sum of at most
    40 ones, exact) and every order statistic are 1.0 and the threshold is 4.0 in both detectors, and with the local-maximum rule
    neither reports another cell.  So cell averaging and OS at ranks 1, 20 and 36 of N0 = 40 write the same 12 records byte for
    byte: frame, refinement, delay and Doppler included.  Without the rule the neighbours are reported too, 44 records from each,
    and the noise estimates differ: the comparison is not vacuous."""
    z, peaks = flat_noise_map()
    n_rx, nd, nb = z.shape
    m = dev(z)
    tr = handle(rts, n_rx, 1, nb, T0, DT)
    kw = dict(guard=(1, 1), train=(2, 2), alpha=4.0, pri=PRI, device_ptr=m.data_ptr(), n_doppler=nd)
    assert R.n0_of((1, 1), (2, 2)) == 40
    ca = tr.cube_detect(mode="ca", local_max=True, **kw)
    lists = [tr.cube_detect_os(rank=rank, local_max=True, **kw) for rank in (1, 20, 36)]
    ca_all = tr.cube_detect(mode="ca", local_max=False, **kw)
    os_all = tr.cube_detect_os(rank=20, local_max=False, **kw)
    tr.close()
    for got in [ca] + lists:
        assert len(got) == 12
        assert list(zip(got["rx"].tolist(), got["doppler_bin"].tolist(), got["range_bin"].tolist())) == [(rx, k, r) for rx in range(n_rx) for k, r in peaks]
        assert got["n_train"].tolist() == [22 if r in (0, nb - 1) else 40 for rx in range(n_rx) for k, r in peaks]
        assert np.all(got["noise"] == 1.0) and np.all(got["threshold"] == 4.0)
        assert got.tobytes() == ca.tobytes()
    print("records: %d and %d with the rule, %d and %d without" % (len(ca), len(lists[0]), len(ca_all), len(os_all)))
    assert len(ca_all) == 44 and len(os_all) == 44
    assert np.any(ca_all["noise"] != os_all["noise"])


# ----------------------------------------------------------------------------- determinism, map sources, the shared list
def test_determinism_sources_and_shared_list(rts):
    from rts_amd import _lib as L
    n_rx, n_p, nb = 2, 16, 256
    tr = handle(rts, n_rx, n_p, nb, 1e-6, 1e-8)
    tr.cube_add_noise(1.0, 5)
    tr.cube_doppler(32, fetch=False)
    kw = dict(guard=(1, 1), train=(4, 4), rank=60, pfa=1e-2, local_max=True, pri=1e-3)
    a = tr.cube_detect_os(**kw)
    b = tr.cube_detect_os(**kw)
    assert len(a) > 10 and a.tobytes() == b.tobytes()
    rd = tr.cube_doppler(32)
    m = dev(rd)
    c = tr.cube_detect_os(device_ptr=m.data_ptr(), n_doppler=32, **kw)
    assert a.tobytes() == c.tobytes()
    # one list per handle: a CA list replaces the OS list and the other way round
    ca = tr.cube_detect((1, 1), (4, 4), "ca", pfa=1e-2, local_max=True, pri=1e-3)
    assert tr.detections().tobytes() == ca.tobytes() and ca.tobytes() != a.tobytes()
    tr.cube_detect_os(fetch=False, **kw)
    assert tr.detections().tobytes() == a.tobytes()
    tr.cube_detect((1, 1), (4, 4), "ca", pfa=1e-2, local_max=True, pri=1e-3, fetch=False)
    assert tr.detections().tobytes() == ca.tobytes()
    # max_detections = 3: RTS_ERR_CAPACITY, the total, the first three records of the full list
    lib = L.lib()
    p = L.RtsCfarOsParams()
    (p.guard_range, p.guard_doppler), (p.train_range, p.train_doppler) = kw["guard"], kw["train"]
    p.rank, p.flags, p.pfa, p.pri, p.max_detections = kw["rank"], L.RTS_CFAR_LOCAL_MAX, kw["pfa"], kw["pri"], 3
    assert lib.rts_cube_detect_os(tr.h, C.byref(p), None, 0) == L.RTS_OK
    out = np.zeros(len(a), L.DETECTION_DTYPE)
    n_out = C.c_uint32(0)
    assert lib.rts_cube_detections_get(tr.h, out.ctypes.data_as(C.c_void_p), len(a), C.byref(n_out)) == L.RTS_ERR_CAPACITY
    assert n_out.value == len(a) and out[:3].tobytes() == a[:3].tobytes() and np.count_nonzero(out[3:]["power"]) == 0
    tr.close()


# ----------------------------------------------------------------------------- errors and lifetime
def test_errors_and_lifetime(rts):
    from rts_amd import _lib as L
    lib = L.lib()
    n_rx, nd, nb = 2, 16, 64
    rng = np.random.default_rng(1)
    z = R.planted_map(rng, n_rx, nd, nb)
    m = dev(z)
    mp = C.c_void_p(m.data_ptr())

    def params(gr=1, gd=1, tr_=4, td=2, rank=30, flags=0, pfa=1e-3, alpha=0.0, pri=0.0, max_det=0):      # N0 = 11 x 7 - 3 x 3 = 68
        p = L.RtsCfarOsParams()
        p.guard_range, p.guard_doppler, p.train_range, p.train_doppler = gr, gd, tr_, td
        p.rank, p.flags, p.pfa, p.alpha, p.pri, p.max_detections = rank, flags, pfa, alpha, pri, max_det
        return p

    def det(p, ptr_=mp, n=nd, h=None):
        return lib.rts_cube_detect_os((h or tr).h, C.byref(p), ptr_, n)

    tr = rts.Tracer(8, 1)
    n_out = C.c_uint32(0)
    assert det(params()) == L.RTS_ERR_INVALID and b"cube" in lib.rts_last_error()
    tr.cube_attach(n_rx, 4, nb, 0.0, 1.0)
    assert det(params(), None, 0) == L.RTS_ERR_INVALID and b"map" in lib.rts_last_error()
    assert det(params(), mp, 0) == L.RTS_ERR_INVALID and b"n_doppler" in lib.rts_last_error()
    assert det(params(), C.c_void_p(m.data_ptr() + 8), nd) == L.RTS_ERR_INVALID and b"aligned" in lib.rts_last_error()
    assert lib.rts_cube_detect_os(tr.h, None, mp, nd) == L.RTS_ERR_INVALID
    cases = [
        (params(flags=2), b"flags"),
        (params(tr_=0, td=0), b"train"), (params(gr=9, tr_=8), b"guard_range"), (params(gd=10, td=7), b"guard_doppler"),
        (params(gd=4, td=4), b"n_doppler"), (params(gr=60, tr_=4), b"guard_range"),
        (params(pfa=1.0), b"pfa"), (params(pfa=-0.1), b"pfa"), (params(pfa=math.nan), b"pfa"),
        (params(pfa=1e-3, alpha=2.0), b"pfa"), (params(pfa=0.0, alpha=0.0), b"pfa"), (params(pfa=0.0, alpha=-1.0), b"alpha"),
        (params(pri=-1.0), b"pri"), (params(pri=math.inf), b"pri"), (params(pri=math.nan), b"pri"),
        (params(rank=0), b"rank"), (params(rank=69), b"rank"),
    ]
    for p, word in cases:
        assert det(p) == L.RTS_ERR_INVALID, word
        assert word in lib.rts_last_error(), (word, lib.rts_last_error())
    p = params(); p.reserved0 = 1
    assert det(p) == L.RTS_ERR_INVALID and b"reserved" in lib.rts_last_error()
    p = params(); p.reserved[1] = 1
    assert det(p) == L.RTS_ERR_INVALID and b"reserved" in lib.rts_last_error()
    assert det(params(rank=68)) == L.RTS_OK                    # the largest rank is accepted
    small = handle(rts, 1, 1, 16)                              # Gr + Tr >= n_bins (a cube of 16 bins)
    assert det(params(gr=4, tr_=12), mp, nd, small) == L.RTS_ERR_INVALID and b"n_bins" in lib.rts_last_error()
    small.close()
    # the shipped detector still refuses a fourth mode
    q = L.RtsCfarParams()
    q.guard_range, q.guard_doppler, q.train_range, q.train_doppler, q.mode, q.pfa = 1, 1, 4, 2, 3, 1e-3
    assert lib.rts_cube_detect(tr.h, C.byref(q), mp, nd) == L.RTS_ERR_INVALID and b"mode" in lib.rts_last_error()
    # rts_cube_attach ends the list
    out = np.zeros(4096, L.DETECTION_DTYPE)
    assert det(params(pfa=1e-1)) == L.RTS_OK
    assert lib.rts_cube_detections_get(tr.h, out.ctypes.data_as(C.c_void_p), 4096, C.byref(n_out)) == L.RTS_OK and n_out.value > 20
    assert det(params(rank=0)) == L.RTS_ERR_INVALID
    assert det(params(pfa=1e-1)) == L.RTS_OK
    tr.cube_attach(n_rx, 4, nb, 0.0, 1.0)
    assert lib.rts_cube_detections_get(tr.h, out.ctypes.data_as(C.c_void_p), 4096, C.byref(n_out)) == L.RTS_ERR_INVALID
    tr.close()
    with pytest.raises(L.RtsError):
        tr.cube_detect_os(device_ptr=m.data_ptr(), n_doppler=nd, pfa=1e-3)
