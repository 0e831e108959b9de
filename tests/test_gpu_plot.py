"""Plot extraction on the device (rts_cube_plots: k_plot_link, k_plot_flatten, the sort, k_plot_flag, k_plot_reduce): every field of
every record bit for bit against the host evaluator rts_plots_eval, on the cases of tests/plot_ref.py (which tests/test_plot_host.py
holds the evaluator to, against an independent restatement).  Every case goes through device_list -- the list uploaded as a torch byte
tensor -- so any mask is reachable without crafting a map.  Then the handle's own list (a caller map with blobs, and a noise cube
through rts_cube_doppler), the lifetime and capacity rules, and one traced scenario: two plates give two plots."""
import ctypes as C
import math

import numpy as np
import pytest

import helpers as H
import plot_ref as R

pytestmark = pytest.mark.gpu


def dev_bytes(a):
    import torch
    raw = np.frombuffer(np.ascontiguousarray(a).tobytes() + b"\0" * 8, np.uint8).copy()      # (never empty: an empty tensor has no address)
    return torch.from_numpy(raw).to("cuda")


def handle(rts, n_rx, nb, t0=R.T0, dt=R.DT, n_p=1):
    tr = rts.Tracer(8, 1)
    tr.cube_attach(n_rx, n_p, nb, t0, dt)
    return tr


def on_device(rts, name, **kw):
    """the case's list through device_list: (device plots, evaluator's plots, the list)"""
    n_rx, nd, nb, _, link, min_cells = R.CASES[name]
    det = R.case_list(name)
    buf = dev_bytes(det)
    tr = handle(rts, n_rx, nb)
    got = tr.cube_plots(link, min_cells, pri=R.PRI, device_list=buf.data_ptr(), n_list=len(det), n_doppler=nd, **kw)
    tr.close()
    want = rts.plots_eval(det, nd, link, min_cells, pri=R.PRI, t0=R.T0, dt=R.DT, n_rx=n_rx, n_bins=nb)
    return got, want, det


# ----------------------------------------------------------------------------- 1. every case, bit for bit
@pytest.mark.parametrize("name", list(R.CASES))
def test_device_equals_evaluator(rts, name):
    got, want, det = on_device(rts, name)
    R.same_bytes(got, want)
    if name in R.EXPECT_PLOTS:
        assert len(got) == R.EXPECT_PLOTS[name]


def test_min_cells_keeps_the_survivors_order(rts):
    all_, two, five = (on_device(rts, n)[0] for n in ("min1", "min2", "min5"))
    assert len(all_) > len(two) > len(five) > 0
    for kept, m in ((two, 2), (five, 5)):
        R.same_bytes(kept, all_[all_["n_cells"] >= m])
        assert np.all(np.diff(kept["first_index"].astype(np.int64)) > 0)


def test_two_runs_give_the_same_bytes(rts):
    n_rx, nd, nb, _, link, _ = R.CASES["random_0.3_1"]
    det = R.case_list("random_0.3_1")
    buf = dev_bytes(det)
    tr = handle(rts, n_rx, nb)
    kw = dict(pri=R.PRI, device_list=buf.data_ptr(), n_list=len(det), n_doppler=nd)
    a = tr.cube_plots(link, **kw); b = tr.cube_plots(link, **kw)
    tr2 = handle(rts, n_rx, nb)
    c = tr2.cube_plots(link, **kw)
    tr.close(); tr2.close()
    assert len(a) > 10 and a.tobytes() == b.tobytes() == c.tobytes()


def test_max_plots_cuts_the_list(rts):
    L = rts.L
    n_rx, nd, nb, _, link, _ = R.CASES["min1"]
    det = R.case_list("min1")
    want = rts.plots_eval(det, nd, link, pri=R.PRI, t0=R.T0, dt=R.DT, n_rx=n_rx, n_bins=nb)
    buf = dev_bytes(det)
    tr = handle(rts, n_rx, nb)
    tr.cube_plots(link, pri=R.PRI, max_plots=7, device_list=buf.data_ptr(), n_list=len(det), n_doppler=nd, fetch=False)
    out = np.full(len(want), 0x5a, np.uint8).repeat(104).view(L.PLOT_DTYPE); tail = out[7:].tobytes()
    n = C.c_uint32(0)
    rc = L.lib().rts_cube_plots_get(tr.h, rts.ptr(out), len(out), C.byref(n))
    assert rc == L.RTS_ERR_CAPACITY and n.value == len(want) > 7
    R.same_bytes(out[:7], want[:7])
    assert out[7:].tobytes() == tail
    # a capacity below the stored count: the prefix, the total, RTS_ERR_CAPACITY
    tr.cube_plots(link, pri=R.PRI, device_list=buf.data_ptr(), n_list=len(det), n_doppler=nd, fetch=False)
    rc = L.lib().rts_cube_plots_get(tr.h, rts.ptr(out), 3, C.byref(n))
    assert rc == L.RTS_ERR_CAPACITY and n.value == len(want)
    R.same_bytes(out[:3], want[:3])
    assert L.lib().rts_cube_plots_get(tr.h, rts.ptr(out), len(out), C.byref(n)) == L.RTS_OK
    R.same_bytes(out, want)
    tr.close()


# ----------------------------------------------------------------------------- 2. the handle's own list
def blob_map(n_rx=2, nd=16, nb=96):
    """a unit background with a few bright blobs: one across the Doppler wrap, one at a range edge, two one cell apart"""
    z = np.ones((n_rx, nd, nb), np.complex128)
    for rx, k, r, hk, hr, amp in [(0, 0, 20, 1, 2, 30.0), (0, 8, 0, 1, 1, 20.0), (1, 5, 50, 2, 1, 25.0), (1, 5, 54, 0, 1, 25.0), (1, 12, 95, 1, 1, 40.0)]:
        for dk in range(-hk, hk + 1):
            for dr in range(-hr, hr + 1):
                if 0 <= r + dr < nb:
                    z[rx, (k + dk) % nd, r + dr] = amp / (1 + abs(dk) + abs(dr))
    return z


def test_handles_list_from_a_caller_map(rts):
    import torch
    L = rts.L
    z = blob_map()
    n_rx, nd, nb = z.shape
    m = torch.from_numpy(z).to("cuda")
    tr = handle(rts, n_rx, nb)
    kw = dict(guard=(1, 1), train=(4, 2), rank=30, alpha=6.0, local_max=False, pri=R.PRI, device_ptr=m.data_ptr(), n_doppler=nd)
    det = tr.cube_detect_os(**kw)
    assert len(det) == 45                                                   # (every blob cell: the host evaluator finds the same)
    got = tr.cube_plots((1, 1), pri=R.PRI)
    want = rts.plots_eval(det, nd, (1, 1), pri=R.PRI, t0=R.T0, dt=R.DT, n_rx=n_rx, n_bins=nb)
    R.same_bytes(got, want)
    assert len(got) == 5 and np.all(got["n_cells"] > 1)
    assert len(tr.cube_plots((2, 1), pri=R.PRI)) == 4                       # the two blobs one empty cell apart join
    # plots end with their list: a new detection, an attach
    n = C.c_uint32(0)
    tr.cube_detect_os(fetch=False, **kw)
    assert L.lib().rts_cube_plots_get(tr.h, None, 0, C.byref(n)) == L.RTS_ERR_INVALID
    tr.cube_plots((1, 1), fetch=False)
    tr.cube_detect((1, 1), (4, 2), "ca", alpha=6.0, local_max=False, device_ptr=m.data_ptr(), n_doppler=nd, fetch=False)
    assert L.lib().rts_cube_plots_get(tr.h, None, 0, C.byref(n)) == L.RTS_ERR_INVALID
    tr.cube_plots((1, 1), fetch=False)
    tr.cube_attach(n_rx, 1, nb, R.T0, R.DT)
    assert L.lib().rts_cube_plots_get(tr.h, None, 0, C.byref(n)) == L.RTS_ERR_INVALID
    with pytest.raises(rts.L.RtsError, match="no detection list"):
        tr.cube_plots((1, 1))
    # a truncated detection list: the plots of the stored prefix, RTS_ERR_CAPACITY
    tr.cube_detect_os(max_detections=10, fetch=False, **kw)
    tr.cube_plots((1, 1), pri=R.PRI, fetch=False)
    out = np.zeros(16, L.PLOT_DTYPE)
    rc = L.lib().rts_cube_plots_get(tr.h, rts.ptr(out), len(out), C.byref(n))
    assert rc == L.RTS_ERR_CAPACITY and "truncated" in L.lib().rts_last_error().decode()
    R.same_bytes(out[:n.value], rts.plots_eval(det[:10], nd, (1, 1), pri=R.PRI, t0=R.T0, dt=R.DT, n_rx=n_rx, n_bins=nb))
    tr.close()


def test_handles_list_from_its_doppler_map(rts):
    """the detect call records the n_doppler of the handle's own map"""
    n_rx, n_p, nb, nd = 2, 16, 128, 32
    tr = handle(rts, n_rx, nb, n_p=n_p)
    tr.cube_add_noise(1.0, 11)
    tr.cube_doppler(nd, fetch=False)
    det = tr.cube_detect((1, 1), (4, 4), "ca", pfa=3e-2, local_max=False, pri=R.PRI)
    got = tr.cube_plots((1, 1), min_cells=2, pri=R.PRI)
    tr.close()
    want = rts.plots_eval(det, nd, (1, 1), 2, pri=R.PRI, t0=R.T0, dt=R.DT, n_rx=n_rx, n_bins=nb)
    assert len(det) > 100 and len(want) > 3
    R.same_bytes(got, want)


def test_refusals(rts):
    L = rts.L
    tr = rts.Tracer(8, 1)
    with pytest.raises(L.RtsError, match="no cube"):
        tr.cube_plots()
    tr.cube_attach(1, 1, 16, 0.0, 1.0)
    buf = dev_bytes(R.case_list("one"))
    for kw, word in ((dict(link=(5, 1)), "link_range"), (dict(link=(1, 5)), "link_doppler"), (dict(pri=-1.0), "pri"), (dict(pri=math.inf), "pri"),
                     (dict(device_list=buf.data_ptr(), n_list=1, n_doppler=0), "n_doppler"), (dict(device_list=buf.data_ptr() + 4, n_list=1, n_doppler=4), "8-byte"),
                     (dict(n_list=1), "without a device_list"), (dict(n_doppler=4), "without a device_list"), (dict(), "no detection list")):
        with pytest.raises(L.RtsError, match=word):
            tr.cube_plots(**kw)
    p = L.RtsPlotParams(); p.reserved[1] = 1
    assert L.lib().rts_cube_plots(tr.h, C.byref(p)) == L.RTS_ERR_INVALID and "reserved" in L.lib().rts_last_error().decode()
    assert L.lib().rts_cube_plots(tr.h, None) == L.RTS_ERR_INVALID
    tr.close()


# ----------------------------------------------------------------------------- 3. a scene, end to end
def test_two_plates_give_two_plots(rts):
    """two 3 m plates facing the radar, 2 m either side of the beam axis and 30 m apart in range: trace at a 40 x 40 lattice, render
    (LFM), noise, compress, Doppler over four pulses, OS-CFAR without the local-maximum rule, plots with link (2, 1) and min_cells 2.
    Exactly two plots; each spans the bin of its plate's geometric delay -- transmitter to the plate's centre and back, the receiver
    sphere being centred on the transmitter -- and holds more than one cell.  (The far plate's detections have one-cell gaps between
    the main lobe and the first sidelobes: link_range 2 is what makes them one plot.)"""
    from rts_amd import scenes as S
    spec = S.config1()
    v, t, n = S.plate_mesh(3.0)
    centres = [(0.0, -2.0, 0.0), (30.0, 2.0, 0.0)]
    spec["meshes"] = [dict(tris=t, verts=v, normals=n, refl_coeff=0.9, refr_index=1.0) for _ in centres]
    spec["motion"] = [dict(position=c, velocity=(0.0, 0.0, 0.0)) for c in centres]
    spec["W"], radius, origin = 40, 50.0, np.array(spec["tx"]["origin"])
    spec["rx"] = [S._rx_at(tuple(origin), (0, 0, 0), radius, math.pi / 2)]
    cs, fc = spec["c"], spec["carrier"]; wl = cs / fc
    n_p, nb, dt = 4, 128, 1.0e-8
    taus = [2.0 * float(np.linalg.norm(np.array(c) - origin)) / cs for c in centres]
    t0 = taus[0] - radius / cs - 30.5 * dt                      # the window opens some 47 bins before the near plate's return
    tr = H.gpu_tracer(rts, spec); tr.cube_attach(1, n_p, nb, t0, dt); tr.cube_set_waveform(rts.Waveform.lfm(32, 0.6, 16))
    for k in range(n_p):
        H.gpu_trace(rts, spec, tr=tr)
        tr.finalise_uniform(None, wl, 1.0, 1.0, fc, cs)
        tr.cube_render(k, "rays", cs, fc, doppler=False)
    rays = tr.received()["results"]
    assert len(rays) > 0
    print("received rays: %d, delays in bins %.2f .. %.2f; geometric %s" % (len(rays), (rays["rayLength"].min() / cs - t0) / dt, (rays["rayLength"].max() / cs - t0) / dt,
                                                                            [(x - t0) / dt for x in taus]))
    tr.cube_add_noise(float((np.abs(tr.cube()) ** 2).max()) / 10.0, 5)      # 10 dB below the strongest sample, before compression
    tr.cube_compress()
    tr.cube_doppler(n_p, fetch=False)
    det = tr.cube_detect_os((4, 0), (8, 1), None, pfa=1e-6, local_max=False)
    got = tr.cube_plots((2, 1), min_cells=2)
    tr.close()
    print("detections (k, r):", list(zip(det["doppler_bin"].tolist(), det["range_bin"].tolist())))
    print("plots:", [(int(p["n_cells"]), int(p["range_min"]), int(p["range_max"]), float(p["range_centroid"])) for p in got])
    R.same_bytes(got, rts.plots_eval(det, n_p, (2, 1), 2, t0=t0, dt=dt, n_rx=1, n_bins=nb))
    assert len(got) == 2
    for p, tau in zip(got, taus):
        b = int(round((tau - t0) / dt))
        assert p["range_min"] <= b <= p["range_max"] and p["n_cells"] > 1, (p, b)
