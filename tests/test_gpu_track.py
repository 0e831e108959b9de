"""The tracker step on the device (rts_cube_track: k_track_prep, k_track_gate, k_track_match, k_track_flag, the scan, k_track_write):
every field of every track byte for byte against the host evaluator rts_tracks_eval, on the cases of tests/track_ref.py (which
tests/test_track_host.py holds the evaluator to, against an independent restatement).  Every case goes through device_plots -- the
list uploaded as a torch byte tensor -- and rts_cube_tracks_set.  Then determinism, the full table, the refusals, a 40-frame sequence
whose table never leaves the device, and the handle's own plots over two cubes."""
import ctypes as C
import math

import numpy as np
import pytest

import plot_ref as PR
import track_ref as R

pytestmark = pytest.mark.gpu


def dev_bytes(a):
    import torch
    raw = np.frombuffer(np.ascontiguousarray(a).tobytes() + b"\0" * 8, np.uint8).copy()      # (never empty: an empty tensor has no address)
    return torch.from_numpy(raw).to("cuda")


def on_device(rts, tr, c, time0=0.0):
    """the case's table through rts_cube_tracks_set, its plots through device_plots: ((device tracks, next id), keep-alive).  The table
    stands at time 0, so the interval the device forms, (0 + T) - 0, is the evaluator's T bit for bit"""
    buf = dev_bytes(c["plots"])
    tr.cube_tracks_set(c["tracks"], c["next_id"], time0)
    return tr.cube_track(time0 + c["T"], device_plots=buf.data_ptr(), n_plots=len(c["plots"]), **c["par"]), buf


def evaluate(rts, c):
    return rts.tracks_eval(c["tracks"], c["next_id"], c["T"], c["plots"], **c["par"])


@pytest.fixture(scope="module")
def tracer(rts):
    tr = rts.Tracer(8, 1)
    yield tr
    tr.close()


# ----------------------------------------------------------------------------- 1. every case, byte for byte
@pytest.mark.parametrize("name", list(R.CASES))
def test_device_equals_evaluator(rts, tracer, name):
    c = R.case(name)
    L = rts.L
    if c["par"]["max_tracks"] == 0:
        (got, nid), _ = on_device(rts, tracer, c)
    else:                                                       # a full table: the stored prefix, the total, RTS_ERR_CAPACITY
        buf = dev_bytes(c["plots"])
        tracer.cube_tracks_set(c["tracks"], c["next_id"], 0.0)
        tracer.cube_track(c["T"], device_plots=buf.data_ptr(), n_plots=len(c["plots"]), fetch=False, **c["par"])
        out = np.full(8, 0x5a, np.uint8).repeat(88).view(L.TRACK_DTYPE)
        n, nid = C.c_uint32(0), C.c_uint64(0)
        rc = L.lib().rts_cube_tracks_get(tracer.h, rts.ptr(out), len(out), C.byref(n), C.byref(nid))
        stored = c["par"]["max_tracks"]
        assert rc == L.RTS_ERR_CAPACITY and n.value == R.expected(name)[1] == 6 and out[stored:].tobytes() == b"\x5a" * (88 * (8 - stored))
        got, nid = out[:stored].copy(), nid.value
    want, want_id = evaluate(rts, c)
    R.same_bytes(got, want)
    assert nid == want_id
    R.same_bytes(got, R.expected(name)[0].copy())


def test_rounds_of_the_matching(rts, tracer):
    """the chain locks one pair per round -- 70 rounds, more than a wave of tracks -- and ends by itself; disjoint pairs take one round;
    no edge takes none"""
    L = rts.L
    for name, want in (("chain70", 70), ("pairs1025", 1), ("abc", 2), ("no_plots", 0), ("gate_above", 0)):
        on_device(rts, tracer, R.case(name))
        rounds = C.c_uint32(99)
        assert L.lib().rts_cube_track_rounds(tracer.h, C.byref(rounds)) == L.RTS_OK and rounds.value == want, (name, rounds.value)


def test_two_runs_and_two_handles_give_the_same_bytes(rts, tracer):
    c = R.case("random_grid")
    (a, ia), _ = on_device(rts, tracer, c)
    (b, ib), _ = on_device(rts, tracer, c)
    tr2 = rts.Tracer(8, 1)
    (d, i_d), _ = on_device(rts, tr2, c)
    tr2.close()
    assert len(a) > 300 and a.tobytes() == b.tobytes() == d.tobytes() and ia == ib == i_d


def test_capacity_of_the_get(rts, tracer):
    L = rts.L
    c = R.case("lifecycle")
    want, want_id = evaluate(rts, c)
    buf = dev_bytes(c["plots"])
    tracer.cube_tracks_set(c["tracks"], c["next_id"], 0.0)
    tracer.cube_track(c["T"], device_plots=buf.data_ptr(), n_plots=len(c["plots"]), fetch=False, **c["par"])
    out = np.full(8, 0x5a, np.uint8).repeat(88).view(L.TRACK_DTYPE); tail = out[3:].tobytes()
    n, nid = C.c_uint32(0), C.c_uint64(0)
    rc = L.lib().rts_cube_tracks_get(tracer.h, rts.ptr(out), 3, C.byref(n), C.byref(nid))
    assert rc == L.RTS_ERR_CAPACITY and n.value == len(want) == 7 and nid.value == want_id and out[3:].tobytes() == tail
    R.same_bytes(out[:3].copy(), want[:3].copy())
    assert L.lib().rts_cube_tracks_get(tracer.h, rts.ptr(out), 8, C.byref(n), None) == L.RTS_OK and n.value == 7
    R.same_bytes(out[:7].copy(), want)
    # reset: an empty table without a time, ids go on; a first frame then only starts tracks
    tracer.cube_tracks_reset()
    got, nid2 = tracer.tracks()
    assert len(got) == 0 and nid2 == want_id
    got, nid3 = tracer.cube_track(-5.0, device_plots=buf.data_ptr(), n_plots=len(c["plots"]), **c["par"])
    want2, want_id2 = rts.tracks_eval(np.zeros(0, R.TRACK), want_id, 1.0, c["plots"], **c["par"])
    R.same_bytes(got, want2)
    assert nid3 == want_id2 == want_id + 5


def test_refusals(rts):
    L = rts.L
    tr = rts.Tracer(8, 1)
    c = R.case("lifecycle")
    buf = dev_bytes(c["plots"])
    ok = dict(device_plots=buf.data_ptr(), n_plots=len(c["plots"]), sigma=(1.0, 1.0))
    with pytest.raises(L.RtsError, match="no plots"):
        tr.cube_track(0.0, sigma=(1.0, 1.0))
    for kw, word in ((dict(gate=0.0), "gate"), (dict(sigma=(0.0, 1.0)), "sigma_delay"), (dict(sigma=(1.0, math.nan)), "sigma_doppler"), (dict(q=-1.0), "q ="),
                     (dict(doppler_period=-1.0), "doppler_period"), (dict(confirm_hits=0), "confirm_hits"), (dict(max_candidates=17), "max_candidates"),
                     (dict(max_tracks=65537), "max_tracks"), (dict(device_plots=None), "without device_plots"), (dict(device_plots=buf.data_ptr() + 4), "8-byte")):
        with pytest.raises(L.RtsError, match=word):
            tr.cube_track(0.0, **dict(ok, **kw))
    p = rts._track_params(9.21, (1.0, 1.0), 0.0, 0.0, 0.0, 3, 3, 0, 16, 0, buf.data_ptr(), 5); p.reserved[0] = 1
    assert L.lib().rts_cube_track(tr.h, C.byref(p), 0.0) == L.RTS_ERR_INVALID and "reserved" in L.lib().rts_last_error().decode()
    assert L.lib().rts_cube_track(tr.h, None, 0.0) == L.RTS_ERR_INVALID
    # the table has a time after the first frame: T must be positive; max_tracks may not change
    first, _ = tr.cube_track(10.0, **ok)
    for t in (10.0, 9.0, math.inf, math.nan):
        with pytest.raises(L.RtsError, match="time"):
            tr.cube_track(t, **ok)
    with pytest.raises(L.RtsError, match="max_tracks"):
        tr.cube_track(11.0, max_tracks=100, **ok)
    again, _ = tr.tracks()
    assert again.tobytes() == first.tobytes() and len(first) == 5      # a refused call leaves the table untouched
    with pytest.raises(L.RtsError, match="max_tracks"):
        tr.cube_tracks_set(c["tracks"], 0, 0.0); tr.cube_track(1.0, max_tracks=6, **ok)      # 7 tracks loaded
    bad = c["tracks"].copy(); bad["p_dd"][2] = -1.0
    with pytest.raises(L.RtsError, match=r"tracks\[2\]"):
        tr.cube_tracks_set(bad, 0, 0.0)
    tr.close()


# ----------------------------------------------------------------------------- 2. a sequence: the table stays on the device
def test_sequence_on_the_device(rts):
    """40 frames, the table carried on the device only and compared each frame with the evaluator chained on the host: four targets
    (two of them five bins apart) with missed frames among five false plots a frame; exactly the four are confirmed, from the third
    frame to the last, each under one id (the outcome tests/test_track_host.py holds the restatement to, for the same seed)"""
    tr = rts.Tracer(8, 1)
    tab, nid, tables, keep = np.zeros(0, R.TRACK), 0, [], []
    for n, z in enumerate(R.sequence(0)):
        buf = dev_bytes(z); keep.append(buf)
        got, got_id = tr.cube_track(R.SEQ_T * n, device_plots=buf.data_ptr(), n_plots=len(z), **R.SEQ_PAR)
        tab, nid = rts.tracks_eval(tab, nid, R.SEQ_T * n - R.SEQ_T * (n - 1), z, **R.SEQ_PAR)
        R.same_bytes(got, tab)
        assert got_id == nid
        tables.append(got)
    tr.close()
    R.check_sequence(tables)


# ----------------------------------------------------------------------------- 3. the handle's own plots, over two cubes
def blob_map(shift, n_rx=2, nd=16, nb=96):
    z = np.ones((n_rx, nd, nb), np.complex128)
    for rx, k, r, hk, hr, amp in [(0, 0, 20, 1, 2, 30.0), (0, 8, 40, 1, 1, 20.0), (1, 5, 50, 2, 1, 25.0), (1, 12, 80, 1, 1, 40.0)]:
        for dk in range(-hk, hk + 1):
            for dr in range(-hr, hr + 1):
                z[rx, (k + dk) % nd, r + shift + dr] = amp / (1 + abs(dk) + abs(dr))
    return z


def test_handles_plots_over_two_cubes(rts):
    import torch
    L = rts.L
    n_rx, nd, nb = 2, 16, 96
    par = R.par(sigma=(1.0 * PR.DT, 30.0), doppler_period=1.0 / PR.PRI, q=10.0, confirm_hits=2)
    tr = rts.Tracer(8, 1)
    tab, nid = np.zeros(0, R.TRACK), 0
    for frame, shift in enumerate((0, 1)):
        tr.cube_attach(n_rx, 1, nb, PR.T0, PR.DT)                           # a new cube: the plots end, the tracks do not
        if frame:
            n = C.c_uint32(0)
            assert L.lib().rts_cube_plots_get(tr.h, None, 0, C.byref(n)) == L.RTS_ERR_INVALID
            with pytest.raises(L.RtsError, match="no plots"):
                tr.cube_track(1.0, **par)
            kept, _ = tr.tracks()
            assert kept.tobytes() == tab.tobytes()
        m = torch.from_numpy(blob_map(shift)).to("cuda")
        tr.cube_detect_os(guard=(1, 1), train=(4, 2), rank=30, alpha=6.0, local_max=False, pri=PR.PRI, device_ptr=m.data_ptr(), n_doppler=nd, fetch=False)
        plots = tr.cube_plots((1, 1), pri=PR.PRI)
        assert len(plots) == 4
        got, got_id = tr.cube_track(0.1 * frame, **par)
        tab, nid = rts.tracks_eval(tab, nid, 0.1, plots, **par)
        R.same_bytes(got, tab)
        assert got_id == nid
    tr.close()
    assert len(tab) == 4 and np.all(tab["hits"] == 2) and np.all(tab["flags"] == R.CONFIRMED) and tab["id"].tolist() == [0, 1, 2, 3]
