"""The lifecycle of a handle's pulse on the GPU (-m gpu): the per-device count of open pulses through every way a pulse can be
closed (rts_pulse_state.h; seen through the grid of another handle's launch), what the accessors say once the previous results
were forgotten (RtsPulseResults::forget), and the block timeline of a pulse whose end was chained on the device-side count."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import helpers as H  # noqa: E402

pytestmark = pytest.mark.gpu
CS, FC, WL = 299792458.0, 1.0e10, 0.03


@pytest.fixture(scope="module")
def scenes():
    from rts_amd import scenes as S
    return S


def _same_set(a, b, what):
    assert np.array_equal(a["slots"], b["slots"]) and np.array_equal(a["path"], b["path"]) and a["rcs_angle"].tobytes() == b["rcs_angle"].tobytes(), what
    H.assert_prd_equal(a["results"], b["results"], what)


def test_open_pulse_count_through_every_closing_path(rts, scenes, monkeypatch):
    """Handle A (RTS_TIMELINE_BLOCKS=1: its block timeline's `blocks` is the launch's grid) traces the whole lattice of 72^3 =
    373 248 launch indices -- 1 458 blocks wanted, more than four per CU on any part up to 304 CUs -- so its grid is the resident
    set: the whole one (g1) when no other pulse of the device is open, the one that leaves block slots free (g2 < g1) while handle
    B has a pulse begun and not ended, or ended through a chain that is not resolved yet.  Every way B's pulse can be closed gives
    the count back: rts_trace_pulse_end, the resolution of a chained end, a chained end that does not speculate, rts_destroy of an
    open and of a chained pulse.  A's received set is the same bits in every launch."""
    spec = scenes.config3(W=72, detail=0.3, rx_radius=300.0)
    tx = spec["tx"]
    assert spec["W"] ** 3 == 373248 and -(-spec["W"] ** 3 // 256) == 1458
    monkeypatch.setenv("RTS_TIMELINE_BLOCKS", "1")
    A = H.gpu_tracer(rts, spec)
    monkeypatch.delenv("RTS_TIMELINE_BLOCKS")
    sets = []

    def grid_of_A():
        A.trace(tx["origin"], tx["span"], tx["dir"], spec["motion"])
        sets.append(A.received())
        return int(A.block_timeline()["blocks"])

    def neighbour(speculate):
        monkeypatch.setenv("RTS_SPECULATE", speculate)
        b = rts.Tracer(spec["W"], spec["max_refl"], spec.get("max_refr", 0), spec["smooth"])
        monkeypatch.delenv("RTS_SPECULATE")
        b.share_scene(A); b.set_receivers(spec["rx"])
        return b

    def begin(b):
        b.trace_begin(tx["origin"], tx["span"], tx["dir"], spec["motion"], ray_first=b_first, ray_count=4096)
    g1 = grid_of_A()                                                       # 1: nothing else open
    # B's pulses: 4 096 launch indices that receive few rays (at most 1 000: under 3/4 of the smaller one-block capacity, 2 048), so that
    # a chained end of B's second pulse is enqueued on the device-side count -- some if there is such a window, else none
    per_window = np.bincount((sets[0]["slots"] // 4096).astype(np.int64), minlength=spec["W"] ** 3 // 4096)[:spec["W"] ** 3 // 4096]
    few = np.flatnonzero((per_window > 0) & (per_window <= 1000))
    b_first = int(few[0] if len(few) else np.argmin(per_window)) * 4096
    assert per_window[b_first // 4096] <= 1000, per_window
    B = neighbour("1")
    begin(B)
    g2 = grid_of_A()                                                       # 2: B begun and not ended
    assert 0 < g2 < g1 < 1458, (g1, g2)
    B.trace_end()
    assert B.received_count() == per_window[b_first // 4096]
    assert grid_of_A() == g1                                               # 3: ended
    begin(B)                                                               # 4: B's second pulse ends through a chain on the device-side count
    B.trace_end_uniform(None, WL, 1.0, 1.0, FC, CS)
    assert grid_of_A() == g2                                               #    ... and stays counted until it is resolved
    B.groups()
    assert grid_of_A() == g1
    B0 = neighbour("0")                                                    # 5: without speculation the chained end is an ordinary end
    for _ in range(2):
        begin(B0)
        B0.trace_end_uniform(None, WL, 1.0, 1.0, FC, CS)
        assert grid_of_A() == g1
    B0.close()
    begin(B)                                                               # 6: destroyed with its pulse open
    assert grid_of_A() == g2
    B.close()
    assert grid_of_A() == g1
    B = neighbour("1")                                                     # 7: destroyed while chained (a first pulse gives it a count to judge by)
    begin(B); B.trace_end()
    begin(B)
    B.trace_end_uniform(None, WL, 1.0, 1.0, FC, CS)
    assert grid_of_A() == g2
    B.close()
    assert grid_of_A() == g1
    assert len(sets[0]["results"]) > 0
    for k, s in enumerate(sets[1:]):
        _same_set(s, sets[0], "A's launch %d" % (k + 1))
    A.close()


def _raw_received_view(L, tr):
    ps = [C.c_void_p(1) for _ in range(4)]; n = C.c_uint64(99)
    L.check(L.lib().rts_received_view(tr.h, *[C.byref(p) for p in ps], C.byref(n)))
    return n.value, [p.value for p in ps]


def test_previous_results_are_forgotten(rts, scenes):
    """rts_kernel_wrapper_on overwrites the handle's received set: afterwards the handle has no received rays, no aggregation and
    no traced pulse, and its next pulse is the first one's bits.  And a new pulse forgets the views' fall-back copies of the previous
    one (a set beyond the host mirror's 4 096 rows): its view is its own set."""
    from rts_amd import _lib as L
    spec = scenes.config1()
    tx = spec["tx"]

    def message(fn, *a):
        with pytest.raises(L.RtsError) as e:
            fn(*a)
        assert e.value.code == L.RTS_ERR_INVALID
        return str(e.value)
    tr = H.gpu_tracer(rts, spec)
    P = rts.Pattern.constant
    tr.set_patterns(P(1.0), [P(1.0)] * len(spec["rx"]), [P(1.0)] * len(spec["meshes"]))
    fin = (np.array([r["centre"] for r in spec["rx"]], np.float64), np.zeros((len(spec["rx"]), 4)), WL, FC, CS)
    tr.trace(tx["origin"], tx["span"], tx["dir"], spec["motion"])
    first = tr.received()
    assert len(first["results"]) > 0
    tr.finalise_patterns(*fin)
    assert len(tr.aggregate(CS, FC)) > 0 and tr.aggregated_view()["power"].shape[0] == len(first["results"])
    Rk, D = 8, tr.depth
    rays = np.zeros(Rk, L.PRD_DTYPE); rays["power"] = 1.0; rays["received"] = 0; rays["rayLength"] = 400.0
    paths = np.full((Rk, D), -1, np.int32); dl = np.zeros(Rk); ph = np.zeros(Rk); pm = np.full(Rk, Rk + 1, np.int32)
    L.check(L.lib().rts_kernel_wrapper_on(tr.h, L.ptr(rays), L.ptr(paths), Rk, D, 1024, 65535, CS, FC, None, None, None, L.ptr(dl), L.ptr(ph), L.ptr(pm)))
    assert tr.received_count() == 0
    assert _raw_received_view(L, tr) == (0, [None] * 4)
    assert "call rts_aggregate first" in message(tr.groups)
    assert "call rts_aggregate first" in message(tr.aggregated_view)
    assert "not a traced pulse's" in message(tr.finalise_patterns, *fin)
    tr.trace(tx["origin"], tx["span"], tx["dir"], spec["motion"])
    _same_set(tr.received(), first, "the pulse after rts_kernel_wrapper_on")
    tr.close()

    c3 = scenes.config3(W=64, detail=0.3, rx_radius=300.0)
    tx = c3["tx"]; n_all = c3["W"] ** 3
    ref = H.gpu_tracer(rts, c3)

    def prefix_with(lo_R, hi_R):                            # a prefix of the lattice that receives between lo_R and hi_R rays
        lo, hi = 1, n_all
        for _ in range(40):
            mid = (lo + hi) // 2
            _, st = H.gpu_trace(rts, c3, tr=ref, ray_first=0, ray_count=mid)
            if st["received"] > hi_R: hi = mid
            elif st["received"] < lo_R: lo = mid
            else: return mid
        raise AssertionError("no prefix")
    big, small = prefix_with(5000, 9000), prefix_with(1500, 1800)      # more rays than the mirror has rows, then fewer
    want = []
    for count in (big, small):
        ref.trace(tx["origin"], tx["span"], tx["dir"], c3["motion"], ray_first=0, ray_count=count); want.append(ref.received())
    ref.close()
    assert len(want[0]["results"]) > 4096 and 0 < len(want[1]["results"]) != len(want[0]["results"])
    tr = H.gpu_tracer(rts, c3)
    for count, w in zip((big, small), want):
        tr.trace_begin(tx["origin"], tx["span"], tx["dir"], c3["motion"], ray_first=0, ray_count=count)
        for again in range(2):
            _same_set(tr.received_view(), w, "view %d of the pulse of %d launch indices" % (again, count))
    tr.close()


def test_block_timeline_of_a_chained_end(rts, scenes, monkeypatch):
    """rts_get_block_timeline reports the LAST launch also when the pulse was ended through a chain on the device-side count
    (rts_trace_pulse_end_uniform, rts_received_prefetch from the handle's second pulse on): pulses of 768 and 1 280 launch indices
    alternate, so the grids are 3, 5, 3, 5 blocks.  Same received sets as a handle that records no timeline."""
    spec = scenes.config3(W=56, detail=0.3, rx_radius=300.0)
    tx = spec["tx"]
    counts = (768, 1280, 768, 1280)
    plain = H.gpu_tracer(rts, spec)
    plain.trace(tx["origin"], tx["span"], tx["dir"], spec["motion"])
    first = int(np.median(plain.received()["slots"])) // 64 * 64 - 256      # a window of the lattice that receives rays
    assert 0 <= first and first + max(counts) <= spec["W"] ** 3
    want = {"prefetch": [], "end_uniform": []}                               # the sets as received, and after the four calls a uniform end stands for
    for n in counts:
        plain.trace(tx["origin"], tx["span"], tx["dir"], spec["motion"], ray_first=first, ray_count=n); want["prefetch"].append(plain.received())
        plain.finalise_uniform(None, WL, 1.0, 1.0, FC, CS); plain.aggregate(CS, FC); want["end_uniform"].append(plain.received())
    plain.close()
    assert all(len(w["results"]) > 0 for w in want["prefetch"])
    monkeypatch.setenv("RTS_TIMELINE_BLOCKS", "1"); monkeypatch.setenv("RTS_SPECULATE", "1")
    tr = H.gpu_tracer(rts, spec)
    monkeypatch.delenv("RTS_TIMELINE_BLOCKS"); monkeypatch.delenv("RTS_SPECULATE")
    for way in ("end_uniform", "prefetch"):
        for n, w in zip(counts, want[way]):
            tr.trace_begin(tx["origin"], tx["span"], tx["dir"], spec["motion"], ray_first=first, ray_count=n)
            if way == "end_uniform":
                tr.trace_end_uniform(None, WL, 1.0, 1.0, FC, CS)
            else:
                tr.received_prefetch()
                _same_set(tr.received_view(), w, (way, n))
            b = tr.block_timeline(); st = tr.stats()
            print(way, n, b, st["ms_trace"], st["received"])
            assert b["blocks"] == -(-n // 256), (way, n, b)
            assert 0.0 == b["start_first"] <= b["start_p50"] <= b["start_last"], (way, n, b)
            assert 0.0 < b["end_first"] <= b["end_p10"] <= b["end_p50"] <= b["end_p90"] <= b["end_last"] <= st["ms_trace"] * 1e3 + 50.0, (way, n, b, st["ms_trace"])
            assert st["received"] == len(w["results"])
            if way == "end_uniform":
                _same_set(tr.received(), w, (way, n))
    tr.close()
