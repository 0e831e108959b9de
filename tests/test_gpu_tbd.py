"""Track-before-detect on the device (rts_cube_tbd_step: k_tbd_step; rts_cube_tbd_extract: k_tbd_cand, the scan): the merit map of
every frame, the pointer ring with its shift tables, the records and the paths byte for byte against the host evaluators
rts_tbd_step_eval and rts_tbd_extract_eval, on the cases of tests/tbd_ref.py (which tests/test_tbd_host.py holds the evaluators to,
against an independent restatement).  Every map is uploaded as a torch tensor and passed as the caller's device map.  Then
determinism, the full list, the handle's own Doppler map, the state across rts_cube_attach, the other products of the handle, reset
and the refusals."""
import ctypes as C
import functools
import math

import numpy as np
import pytest

import tbd_ref as R

pytestmark = pytest.mark.gpu


def upload(z):
    import torch
    return torch.from_numpy(np.ascontiguousarray(z, np.complex128)).to("cuda")


@functools.lru_cache(maxsize=None)
def _evaluated(name):
    """the evaluators chained on the host over the case's frames (computed once, read-only): per frame the merit; the stored ring; the
    records and paths of the case's extraction"""
    from rts_amd import api
    c = R.case(name); p = c["par"]
    merit, merits, ptrs, tabs = None, [], [], []
    for n, z in enumerate(c["maps"]):
        merit, code, s = api.tbd_step_eval(z, merit, c["times"][n] - c["times"][n - 1] if n else 0.0, dt=c["dt"], **p)
        merits.append(merit); ptrs.append(code); tabs.append(s)
    keep = min(len(ptrs), p["depth"])
    ring = (np.stack(ptrs[-keep:]), np.stack(tabs[-keep:]))
    rec, paths = api.tbd_extract_eval(merit, ring[0], ring[1], R.run(name)["threshold"], p["half"], p["depth"], c["local_max"], c["max_tracks"], p["pri"], c["t0"], c["dt"])
    for a in merits + list(ring) + [rec, paths]:
        a.setflags(write=False)
    return dict(merits=merits, ring=ring, rec=rec, paths=paths)


def steps(tr, c, check_each=None):
    """the case's frames on the handle, from a fresh state on a cube of the case's shape"""
    n_rx, nd, nb = c["maps"][0].shape
    tr.cube_tbd_reset()
    tr.cube_attach(n_rx, 1, nb, c["t0"], c["dt"])
    for n, z in enumerate(c["maps"]):
        m = upload(z)
        tr.cube_tbd_step(c["times"][n], device_ptr=m.data_ptr(), n_doppler=nd, **c["par"])
        if check_each:
            check_each(n)
        else:
            tr.tbd_merit()                                              # (synchronises: the tensor may go)


@pytest.fixture(scope="module")
def tracer(rts):
    tr = rts.Tracer(8, 1)
    yield tr
    tr.close()


# ----------------------------------------------------------------------------- 1. every case, byte for byte
@pytest.mark.parametrize("name", R.ALL)
def test_device_equals_evaluators(rts, tracer, name):
    c = R.case(name); want = _evaluated(name); ref = R.run(name)

    def merit_of_frame(n):
        R.same_bytes(tracer.tbd_merit(), want["merits"][n])
    steps(tracer, c, merit_of_frame)
    shape, frames = tracer.tbd_info()
    assert shape == c["maps"][0].shape + (c["par"]["depth"],) and frames == len(c["maps"])
    codes, shifts = tracer.tbd_ring()
    R.same_bytes(codes, want["ring"][0]); R.same_bytes(shifts, want["ring"][1])
    tracer.cube_tbd_extract(ref["threshold"], c["local_max"], c["max_tracks"], fetch=False)
    L = rts.L
    n = C.c_uint32(0)
    cap = len(want["rec"])
    rec = np.zeros(max(cap, 1), L.TBD_TRACK_DTYPE); paths = np.zeros((max(cap, 1), c["par"]["depth"], 2), np.uint32)
    rc = L.lib().rts_cube_tbd_tracks_get(tracer.h, rts.ptr(rec), cap, C.byref(n))
    assert rc == (L.RTS_ERR_CAPACITY if c["max_tracks"] else L.RTS_OK) and n.value == ref["total"]
    assert L.lib().rts_cube_tbd_paths_get(tracer.h, rts.ptr(paths), cap) == rc
    R.same_bytes(rec[:cap], want["rec"]); R.same_bytes(paths[:cap], want["paths"])
    R.same_bytes(rec[:cap].view(R.TBD), ref["rec"]); R.same_bytes(paths[:cap], ref["paths"])      # ... and the restatement's


def test_two_runs_and_two_handles_give_the_same_bytes(rts, tracer):
    c = R.case("three_receivers"); thr = R.run("three_receivers")["threshold"]
    got = []
    tr2 = rts.Tracer(8, 1)
    for tr in (tracer, tracer, tr2):
        steps(tr, c)
        rec, paths = tr.cube_tbd_extract(thr)
        codes, shifts = tr.tbd_ring()
        got.append(tr.tbd_merit().tobytes() + codes.tobytes() + shifts.tobytes() + rec.tobytes() + paths.tobytes())
    tr2.close()
    assert len(rec) > 10 and got[0] == got[1] == got[2]


def test_full_list(rts, tracer):
    """max_tracks = 10 of 512 candidates: RTS_ERR_CAPACITY, the stored prefix, the total; nothing written beyond the capacity given"""
    L = rts.L
    c = R.case("full_list"); want = _evaluated("full_list"); ref = R.run("full_list")
    steps(tracer, c)
    tracer.cube_tbd_extract(ref["threshold"], c["local_max"], c["max_tracks"], fetch=False)
    with pytest.raises(L.RtsError, match="of 512"):
        tracer.tbd_tracks()
    rec = np.full(16, 0x5a, np.uint8).repeat(48).view(L.TBD_TRACK_DTYPE); paths = np.full((16, 8, 2), 0x5a5a5a5a, np.uint32)
    n = C.c_uint32(0)
    assert L.lib().rts_cube_tbd_tracks_get(tracer.h, rts.ptr(rec), 4, C.byref(n)) == L.RTS_ERR_CAPACITY and n.value == ref["total"] == 512
    assert L.lib().rts_cube_tbd_paths_get(tracer.h, rts.ptr(paths), 4) == L.RTS_ERR_CAPACITY
    R.same_bytes(rec[:4].copy(), want["rec"][:4].copy()); R.same_bytes(paths[:4].copy(), want["paths"][:4].copy())
    assert rec[4:].tobytes() == b"\x5a" * (48 * 12) and np.all(paths[4:] == 0x5a5a5a5a)
    assert L.lib().rts_cube_tbd_tracks_get(tracer.h, rts.ptr(rec), 16, C.byref(n)) == L.RTS_ERR_CAPACITY and n.value == 512      # 10 stored
    R.same_bytes(rec[:10].copy(), want["rec"]); assert rec[10:].tobytes() == b"\x5a" * (48 * 6)
    # every candidate with max_tracks 0
    rec, paths = tracer.cube_tbd_extract(ref["threshold"], c["local_max"], 0)
    assert len(rec) == 512 and rec[:10].tobytes() == want["rec"].tobytes() and np.all(np.diff(rec["doppler_bin"].astype(np.int64) * 128 + rec["range_bin"]) > 0)


# ----------------------------------------------------------------------------- 2. the handle and its other products
def noisy_cube(tr, n_rx, n_pulses, nb, seed):
    tr.cube_attach(n_rx, n_pulses, nb, 1e-6, 1e-8)
    tr.cube_add_noise(1.0, seed)


def test_handles_own_doppler_map(rts):
    """the handle's last rts_cube_doppler map gives the state the same map gives when passed by pointer; the state spans the cubes"""
    n_rx, n_p, nb = 2, 8, 150
    p = R.par(depth=4, scale=1.0 / 8.0, delay_rate_per_hz=3e-9, pri=1e-3)
    a, b = rts.Tracer(8, 1), rts.Tracer(8, 1)
    b.cube_attach(n_rx, 1, nb, 1e-6, 1e-8)
    merit = None
    for n, seed in enumerate((11, 12, 13)):
        noisy_cube(a, n_rx, n_p, nb, seed)                             # a new cube every frame: the state survives rts_cube_attach
        z = a.cube_doppler(n_p)
        a.cube_tbd_step(0.5 * n, **p)
        m = upload(z)
        b.cube_tbd_step(0.5 * n, device_ptr=m.data_ptr(), n_doppler=n_p, **p)
        merit, _, _ = rts.tbd_step_eval(z, merit, 0.5, dt=1e-8, **p)
        R.same_bytes(a.tbd_merit(), merit); R.same_bytes(b.tbd_merit(), merit)
    (ca, sa), (cb, sb) = a.tbd_ring(), b.tbd_ring()
    assert len(ca) == 3 and ca.tobytes() == cb.tobytes() and sa.tobytes() == sb.tobytes() and np.any(sa != 0)
    ra, pa = a.cube_tbd_extract(float(np.quantile(merit, 0.99)))
    rb, pb = b.cube_tbd_extract(float(np.quantile(merit, 0.99)))
    assert len(ra) > 0 and ra.tobytes() == rb.tobytes() and pa.tobytes() == pb.tobytes() and np.all(ra["delay"] == 1e-6 + ra["range_bin"] * 1e-8)
    # without a map: refused, the state untouched
    a.cube_attach(n_rx, n_p, nb, 1e-6, 1e-8)
    with pytest.raises(rts.L.RtsError, match="no map"):
        a.cube_tbd_step(2.0, **p)
    R.same_bytes(a.tbd_merit(), merit)
    a.close(); b.close()


def test_state_across_attach_and_a_cube_of_another_shape(rts, tracer):
    c = R.case("three_receivers"); want = _evaluated("three_receivers")
    n_rx, nd, nb = c["maps"][0].shape
    tracer.cube_tbd_reset()
    for n, z in enumerate(c["maps"]):
        tracer.cube_attach(n_rx, 1, nb, c["t0"], c["dt"])              # the same shape again: the state goes on
        m = upload(z)
        tracer.cube_tbd_step(c["times"][n], device_ptr=m.data_ptr(), n_doppler=nd, **c["par"])
        R.same_bytes(tracer.tbd_merit(), want["merits"][n])
    tracer.cube_attach(n_rx, 1, nb + 1, c["t0"], c["dt"])
    m = upload(np.zeros((n_rx, nd, nb + 1), np.complex128))
    with pytest.raises(rts.L.RtsError, match="the state has"):
        tracer.cube_tbd_step(100.0, device_ptr=m.data_ptr(), n_doppler=nd, **c["par"])
    R.same_bytes(tracer.tbd_merit(), want["merits"][-1])
    codes, shifts = tracer.tbd_ring()
    R.same_bytes(codes, want["ring"][0]); R.same_bytes(shifts, want["ring"][1])
    # reset, then the other shape and another window
    tracer.cube_tbd_reset()
    assert tracer.tbd_info() == ((0, 0, 0, 0), 0)
    with pytest.raises(rts.L.RtsError, match="no track-before-detect state"):
        tracer.tbd_merit()
    z = R.noise(np.random.default_rng(5), (n_rx, nd, nb + 1)); m = upload(z)
    tracer.cube_tbd_step(-3.0, half=(2, 1), depth=2, device_ptr=m.data_ptr(), n_doppler=nd)
    R.same_bytes(tracer.tbd_merit(), rts.tbd_step_eval(z, None, 0.0, half=(2, 1), depth=2)[0])
    assert tracer.tbd_info() == ((n_rx, nd, nb + 1, 2), 1)


def test_interleaved_with_detect_plots_and_track(rts):
    """steps between cube_detect, cube_plots and cube_track on one handle: each product's bytes are what they are alone, and the
    state is what the evaluators give"""
    n_rx, nd, nb = 2, 16, 96
    rng = np.random.default_rng(21)
    maps = [R.noise(rng, (n_rx, nd, nb)) for _ in range(3)]
    for z in maps:
        z[0, 3, 40] += 9.0; z[1, 12, 70] += 8.0
    det = dict(guard=(1, 1), train=(4, 2), pfa=1e-4, local_max=False, pri=1e-3, n_doppler=nd)
    trk = dict(sigma=(1.0, 30.0), doppler_period=1e3, confirm_hits=2)
    p = R.par(depth=2, pri=1e-3)
    alone, mixed = rts.Tracer(8, 1), rts.Tracer(8, 1)
    alone.cube_attach(n_rx, 1, nb, 0.0, 1.0); mixed.cube_attach(n_rx, 1, nb, 0.0, 1.0)
    merit = None
    for n, z in enumerate(maps):
        m = upload(z)
        d0 = alone.cube_detect(device_ptr=m.data_ptr(), **det); p0 = alone.cube_plots((1, 1), pri=1e-3); t0, i0 = alone.cube_track(0.1 * n, **trk)
        mixed.cube_detect(device_ptr=m.data_ptr(), fetch=False, **det)
        mixed.cube_tbd_step(0.1 * n, device_ptr=m.data_ptr(), n_doppler=nd, **p)
        mixed.cube_plots((1, 1), pri=1e-3, fetch=False)
        mixed.cube_tbd_extract(0.0, fetch=False)
        mixed.cube_track(0.1 * n, fetch=False, **trk)
        d1, p1, (t1, i1) = mixed.detections(), mixed.plots(), mixed.tracks()
        assert len(d0) >= 2 and d0.tobytes() == d1.tobytes() and p0.tobytes() == p1.tobytes() and t0.tobytes() == t1.tobytes() and i0 == i1
        merit, _, _ = rts.tbd_step_eval(z, merit, 0.1 * n - 0.1 * (n - 1), **p)
        R.same_bytes(mixed.tbd_merit(), merit)
        assert len(mixed.tbd_tracks()[0]) > 0
    alone.close(); mixed.close()


# ----------------------------------------------------------------------------- 3. the device refuses what the evaluators refuse
def test_refusals(rts):
    L = rts.L
    tr = rts.Tracer(8, 1)
    n_rx, nd, nb = 1, 4, 20
    z = R.noise(np.random.default_rng(3), (n_rx, nd, nb)); m = upload(z)
    ok = dict(device_ptr=m.data_ptr(), n_doppler=nd)
    with pytest.raises(L.RtsError, match="no cube"):
        tr.cube_tbd_step(0.0, **ok)
    tr.cube_attach(n_rx, 1, nb, 0.0, 1.0)
    with pytest.raises(L.RtsError, match="no track-before-detect state"):
        tr.cube_tbd_extract(1.0)
    bad = ((dict(half=(4, 2)), "half_doppler"), (dict(half=(1, 16)), "half_range"), (dict(half=(2, 2)), "exceeds n_doppler"),
           (dict(depth=0), "depth"), (dict(depth=65), "depth"), (dict(score=2), "score"), (dict(scale=0.0), "scale"), (dict(scale=math.inf), "scale"),
           (dict(decay=0.0), "decay"), (dict(decay=1.5), "decay"), (dict(decay=math.nan), "decay"), (dict(delay_rate_per_hz=math.inf), "delay_rate_per_hz"),
           (dict(pri=-1.0), "pri"), (dict(device_ptr=m.data_ptr() + 8), "16-byte"), (dict(n_doppler=0), "n_doppler"))
    for kw, word in bad:
        with pytest.raises(L.RtsError, match=word):
            tr.cube_tbd_step(0.0, **dict(ok, **kw))
        if "device_ptr" not in kw and "n_doppler" not in kw:            # ... and so does the evaluator
            with pytest.raises(L.RtsError, match=word):
                rts.tbd_step_eval(z, None, 0.0, **kw)
    with pytest.raises(L.RtsError, match="time"):
        tr.cube_tbd_step(math.nan, **ok)
    for field in ("flags", "reserved0", "reserved"):
        p = rts._tbd_params((1, 2), 8, "power", 1.0, 1.0, 0.0, 0.0)
        if field == "reserved":
            p.reserved[1] = 1
        else:
            setattr(p, field, 1)
        assert L.lib().rts_cube_tbd_step(tr.h, C.byref(p), 0.0, C.c_void_p(m.data_ptr()), nd) == L.RTS_ERR_INVALID
        assert ("flags" if field == "flags" else "reserved") in L.lib().rts_last_error().decode()
    assert L.lib().rts_cube_tbd_step(tr.h, None, 0.0, C.c_void_p(m.data_ptr()), nd) == L.RTS_ERR_INVALID
    assert tr.tbd_info() == ((0, 0, 0, 0), 0)                           # nothing above made a state
    # the state has a time after the first frame: T positive and finite; the window and the depth are fixed; a shift beyond 2^30
    tr.cube_tbd_step(10.0, **ok)
    first = tr.tbd_merit()
    for t, word in ((10.0, "T = "), (9.0, "T = "), (math.inf, "time")):
        with pytest.raises(L.RtsError, match=word):
            tr.cube_tbd_step(t, **ok)
    for kw in (dict(half=(1, 1)), dict(half=(0, 2)), dict(depth=4)):
        with pytest.raises(L.RtsError, match="the state was made with"):
            tr.cube_tbd_step(11.0, **dict(ok, **kw))
    with pytest.raises(L.RtsError, match="shift of Doppler row 1"):
        tr.cube_tbd_step(11.0, delay_rate_per_hz=1e10, pri=0.25, **ok)
    with pytest.raises(L.RtsError, match="shift of Doppler row 1"):
        rts.tbd_step_eval(z, first, 1.0, delay_rate_per_hz=1e10, pri=0.25)
    assert tr.tbd_info()[1] == 1 and tr.tbd_merit().tobytes() == first.tobytes()
    with pytest.raises(L.RtsError, match="no extraction"):
        tr.tbd_tracks()
    for kw, word in ((dict(threshold=math.nan), "threshold"), (dict(pri=-1.0), "pri"), (dict(max_tracks=65537), "max_tracks")):
        with pytest.raises(L.RtsError, match=word):
            tr.cube_tbd_extract(**dict(dict(threshold=1.0), **kw))
    e = rts._tbd_extract_params(1.0, True, 0, 0.0); e.flags = 2
    assert L.lib().rts_cube_tbd_extract(tr.h, C.byref(e)) == L.RTS_ERR_INVALID and "flags" in L.lib().rts_last_error().decode()
    tr.close()
