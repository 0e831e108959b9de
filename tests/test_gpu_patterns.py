"""Device-side finalisation with tabulated antenna gain and RCS patterns (rts_set_patterns, rts_finalise_patterns,
rts_trace_pulse_end_patterns): constant tables against the uniform path bit for bit, general tables against the oracle's
callback finalisation (ray_tracer.cpp:1198-1253) with independently written callbacks, the fused chain against the separate
calls, and the error / lifetime rules of include/rts_amd.h."""
import math

import numpy as np
import pytest

import helpers as H
from test_patterns_host import grid_ref, separable_ref

pytestmark = pytest.mark.gpu
CS, FC = 299792458.0, 1.0e10
TWO_PI = 2.0 * math.pi


@pytest.fixture(scope="module")
def scenes():
    from rts_amd import scenes as S
    return S


def wrap(x):
    return x - TWO_PI * math.floor((x + math.pi) / TWO_PI)


def angles(vec, ref_az, ref_el):
    x, y, z = vec
    n = math.sqrt(x * x + y * y + z * z)
    el = math.asin(max(-1.0, min(1.0, z / n))) if n > 0 else 0.0
    return wrap(math.atan2(y, x) - ref_az), el - ref_el


def rx_positions(spec):
    return np.array([r["centre"] for r in spec["rx"]], np.float64)


def refraction_spec(scenes):
    """config_multi with refraction on, as test_gpu_parity.test_refraction sets it up"""
    spec = scenes.config_multi(W=14, max_refl=3)
    spec["max_refr"] = 1
    spec["meshes"][0]["refr_index"] = 1.5; spec["meshes"][0]["refl_coeff"] = 0.5
    spec["meshes"][1]["refr_index"] = 2.2; spec["meshes"][1]["refl_coeff"] = -0.6
    spec["meshes"][2]["refl_coeff"] = 1.0
    spec["rx"] = spec["rx"] + [scenes._rx_at((200.0, 0.0, 0.0), (0, 0, 0), 90.0, 2.6)]
    return spec


# ---------------------------------------------------------------------------------------------------- a general pattern set
class Tables:
    """seeded tables (as numpy arrays) + the Pattern objects built from them + independent evaluators (math / numpy)"""

    def __init__(self, rts, n_rx, n_targets, seed=5):
        rng = np.random.default_rng(seed)
        self.rts = rts
        # transmitter: GRID over the whole sphere, the columns at -pi and +pi equal
        nu, nv = 33, 17
        g = rng.uniform(0.2, 1.5, (nv, nu)); g[:, -1] = g[:, 0]
        self.tx = ("grid", g, -math.pi, TWO_PI / (nu - 1), -math.pi / 2, math.pi / (nv - 1), 1.3)
        # receivers: SEPARABLE, ABS flags differing per receiver
        self.rx = []
        for k in range(n_rx):
            us = np.sort(np.concatenate([[-math.pi, math.pi], rng.uniform(-math.pi, math.pi, 9)]))
            vs = np.sort(np.concatenate([[-math.pi / 2, math.pi / 2], rng.uniform(-1.5, 1.5, 5)]))
            uy = rng.uniform(0.3, 2.0, len(us)); uy[-1] = uy[0]                  # (continuous across the wrap at +-pi)
            self.rx.append(("sep", us, uy, vs, rng.uniform(0.3, 2.0, len(vs)), 0.8 + 0.1 * k, k % 2 == 0, k % 3 == 1))
        # targets: GRID, SEPARABLE, CONSTANT in turn
        self.rcs = []
        for t in range(n_targets):
            if t % 3 == 0:
                g = rng.uniform(0.5, 4.0, (9, 21)); g[:, -1] = g[:, 0]
                self.rcs.append(("grid", g, -math.pi, TWO_PI / 20, -math.pi / 2, math.pi / 8, 2.0))
            elif t % 3 == 1:
                us = np.linspace(-math.pi, math.pi, 15); vs = np.linspace(-1.2, 1.2, 7)
                self.rcs.append(("sep", us, rng.uniform(0.5, 3.0, 15), vs, rng.uniform(0.5, 3.0, 7), 1.1, True, False))
            else:
                self.rcs.append(("const", 0.7 + 0.2 * t))
        self.rot = np.array([[0.3 - 0.2 * k, -0.05 + 0.03 * k, 2.0e5 * (1 + k), -1.0e5 * (1 + 0.5 * k)] for k in range(n_rx)])

    def pattern(self, t):
        P = self.rts.Pattern
        if t[0] == "grid":
            return P.grid(t[1], t[2], t[3], t[4], t[5], scale=t[6])
        if t[0] == "sep":
            return P.separable(t[1], t[2], t[3], t[4], scale=t[5], abs_u=t[6], abs_v=t[7])
        return P.constant(t[1])

    def install(self, tr):
        tr.set_patterns(self.pattern(self.tx), [self.pattern(t) for t in self.rx], [self.pattern(t) for t in self.rcs])

    @staticmethod
    def value(t, u, v):
        if t[0] == "grid":
            return t[6] * grid_ref(t[1], t[2], t[3], t[4], t[5], u, v)
        if t[0] == "sep":
            return separable_ref(t[1], t[2], t[3], t[4], t[5], t[6], t[7], u, v)
        return t[1]


def constant_set(rts, n_rx, rcs):
    P = rts.Pattern
    return P.constant(1.7), [P.constant(0.6)] * n_rx, [P.constant(r) for r in rcs]


# ---------------------------------------------------------------------------------------------------- 1. constant == uniform
@pytest.mark.parametrize("which", ["c3", "refraction"])
def test_constant_patterns_equal_uniform_bit_for_bit(rts, scenes, which):
    spec = scenes.config3(W=64, detail=0.3, rx_radius=300.0) if which == "c3" else refraction_spec(scenes)
    n_t, n_rx = len(spec["meshes"]), len(spec["rx"])
    rcs = [1.3, 0.8, 2.1][:n_t]; wl = spec["c"] / spec["carrier"]
    tx = spec["tx"]; n_all = spec["W"] ** 3
    r0 = 2.0 * float(np.linalg.norm(np.asarray(tx["origin"]))); t0 = (r0 - 400.0) / CS; dt = 800.0 / CS / 128
    out = []
    for mode in ("uniform", "patterns"):
        tr = H.gpu_tracer(rts, spec)
        tr.cube_attach(n_rx, 1, 128, t0, dt)
        tr.trace(tx["origin"], tx["span"], tx["dir"], spec["motion"])
        if mode == "uniform":
            tr.finalise_uniform(rcs, wl, 1.7, 0.6, spec["carrier"], spec["c"])
        else:
            t_, r_, c_ = constant_set(rts, n_rx, rcs)
            tr.set_patterns(t_, r_, c_)
            tr.finalise_patterns(rx_positions(spec), np.zeros((n_rx, 4)), wl, spec["carrier"], spec["c"])
        rec = tr.received()
        tr.cube_accumulate(0, spec["c"], spec["carrier"])
        g = tr.aggregate(spec["c"], spec["carrier"])
        out.append((rec, g, tr.aggregated(), tr.cube().copy()))
        tr.close()
    (ra, ga, aa, ca), (rb, gb, ab, cb) = out
    assert len(ra["slots"]) > 50
    assert ra["results"].tobytes() == rb["results"].tobytes() and np.array_equal(ra["path"], rb["path"])
    assert ga.tobytes() == gb.tobytes()
    for f in ("results", "delay", "phase", "pathMatch"):
        assert aa[f].tobytes() == ab[f].tobytes(), f
    big = np.nanmax(np.abs(ca))                                     # (NaN bins: rays of negative power from a negative reflection coefficient)
    assert big > 0
    np.testing.assert_allclose(cb, ca, rtol=0, atol=1e-13 * big)    # (f64 atomics: a bin's sum may round differently)
    if which == "refraction":
        assert (ra["results"]["refrDepth"] > 0).any()


# ---------------------------------------------------------------------------------------------------- 2. against the oracle
def test_patterns_against_the_oracle(rts, oracle, scenes):
    spec = scenes.config_multi(W=26)
    n_t, n_rx = len(spec["meshes"]), len(spec["rx"])
    T = Tables(rts, n_rx, n_t)
    wl = spec["c"] / spec["carrier"]; tx = spec["tx"]; pos = rx_positions(spec)
    seen = dict(rcs=[], gt=[], gr=[], gr_still=[])

    def get_rcs(targ, az, el, wl_):
        v = Tables.value(T.rcs[targ], wrap(az / 2), el / 2)
        seen["rcs"].append(v)
        return v

    def get_gain(is_rx, index, vec, t, wl_):
        if not is_rx:
            v = Tables.value(T.tx, *angles(vec, tx["dir"][0], tx["dir"][1]))
            seen["gt"].append(v)
            return v
        az, el, raz, rel = T.rot[index]
        v = Tables.value(T.rx[index], *angles(vec, az + raz * t, el + rel * t))
        seen["gr"].append(v); seen["gr_still"].append(Tables.value(T.rx[index], *angles(vec, az, el)))
        return v

    tr = H.gpu_tracer(rts, spec, keep_all=True)
    T.install(tr)
    r0 = 2.0 * abs(tx["origin"][0]); t0 = 0.0; dt = r0 * 2.0 / CS / 256
    tr.cube_attach(n_rx, 1, 256, t0, dt)
    tr.trace(tx["origin"], tx["span"], tx["dir"], spec["motion"])
    o = H.oracle_trace(oracle, spec)
    g = tr.all_rays(spec["W"] ** 3)
    H.compare_full(o, g, spec["W"] ** 3)
    # the RCS angles come from libm's / OCML's atan2 (equal within 1e-12 rad, not in bits): the callbacks see the device's, so
    # that the comparison below is one of the finalisation alone
    rx, rxi, _ = oracle.filter_finalise_cb(o["results"], o["path"], g["rcs_angle"], tx["origin"], pos, 0, 0.0, wl,
                                           spec["carrier"], spec["c"], get_rcs, get_gain)
    R = len(rx)
    assert R > 100
    # the test has teeth: the tables' values vary over the received set, and the receivers' rotation during the delay matters
    for k in ("rcs", "gt", "gr"):
        a = np.array(seen[k]); assert a.max() > 1.05 * a.min(), k
    gr, still = np.array(seen["gr"]), np.array(seen["gr_still"])
    assert (np.abs(gr - still) > 1e-9 * np.abs(still)).any()
    lit = oracle.aggregate_literal(rx, rxi, spec["c"], spec["carrier"], len(o["results"]))
    uniq = oracle.unique_paths(lit["pathMatch"])
    cube_ref = np.zeros((n_rx, 1, 256), np.complex128)
    oracle.cube_accumulate(cube_ref, 0, rx, t0, dt, spec["c"], spec["carrier"])

    tr.finalise_patterns(pos, T.rot, wl, spec["carrier"], spec["c"])
    rec = tr.received()["results"]
    assert len(rec) == R
    np.testing.assert_allclose(rec["power"], rx["power"], rtol=1e-12, atol=0)
    assert rec["doppler"].tobytes() == rx["doppler"].tobytes()
    tr.cube_accumulate(0, spec["c"], spec["carrier"])
    groups = tr.aggregate(spec["c"], spec["carrier"])
    ag = tr.aggregated()
    assert np.array_equal(ag["pathMatch"], lit["pathMatch"])
    np.testing.assert_allclose(ag["results"]["power"], lit["results"]["power"], rtol=1e-11, atol=0)
    np.testing.assert_allclose(ag["delay"], lit["delay"], rtol=1e-11, atol=0)
    np.testing.assert_allclose(ag["phase"], lit["phase"], rtol=1e-11, atol=1e-300)
    resp = rts.groups_to_responses(groups)
    assert np.array_equal(resp["ray"].astype(np.int64), uniq.astype(np.int64))
    cube = tr.cube()
    assert np.abs(cube_ref).max() > 0
    np.testing.assert_allclose(cube, cube_ref, rtol=0, atol=1e-11 * np.abs(cube_ref).max())
    tr.close()


# ---------------------------------------------------------------------------------------------------- 3. fused == separate calls
def _prefix_with(rts, spec, lo_R, hi_R):
    tr = H.gpu_tracer(rts, spec); lo, hi = 1, spec["W"] ** 3
    for _ in range(40):
        mid = (lo + hi) // 2
        _, st = H.gpu_trace(rts, spec, tr=tr, ray_first=0, ray_count=mid)
        if st["received"] > hi_R: hi = mid
        elif st["received"] < lo_R: lo = mid
        else: tr.close(); return mid
    raise AssertionError("no prefix")


def test_pulse_end_patterns_equals_the_separate_calls(rts, scenes, monkeypatch):
    c3 = scenes.config3(W=64, detail=0.3, rx_radius=300.0)
    tx = c3["tx"]; n_rx = len(c3["rx"]); pos = rx_positions(c3); wl = 0.03
    T = Tables(rts, n_rx, 1, seed=11)
    small, big = _prefix_with(rts, c3, 1500, 1800), _prefix_with(rts, c3, 5000, 9000)
    plan = [small, small, 3, big, small, big, big, small]

    def rot(k):                                                     # receiver rotations that change every pulse
        r = T.rot.copy(); r[:, 0] += 0.01 * k; r[:, 1] -= 0.004 * k; r[:, 2] *= 1.0 + 0.1 * k
        return r
    cube_shape = (n_rx, len(plan), 64)
    r0 = 2.0 * float(np.linalg.norm(np.asarray(tx["origin"]) - np.asarray(c3["motion"][0]["position"]))); t0 = (r0 - 150.0) / CS; dt = 300.0 / CS / 64

    def run(mode):
        monkeypatch.setenv("RTS_SPECULATE", "0" if mode == "nospec" else "1")
        tr = H.gpu_tracer(rts, c3); T.install(tr)
        tr.cube_attach(*cube_shape, t0, dt)
        out = []
        for k, count in enumerate(plan):
            tr.trace_begin(tx["origin"], tx["span"], tx["dir"], c3["motion"], ray_first=0, ray_count=count)
            if mode == "four":
                tr.trace_end(); tr.finalise_patterns(pos, rot(k), wl, FC, CS); tr.cube_accumulate(k, CS, FC); g = tr.aggregate(CS, FC)
            else:
                tr.trace_end_patterns(pos, rot(k), wl, FC, CS, cube_pulse=k); g = tr.groups()
            st = tr.stats(); rec = tr.received(); agg = tr.aggregated()
            out.append((g, {k2: st[k2] for k2 in ("segments", "shaded", "received")}, rec, agg))
        cube = tr.cube().copy(); tr.close()
        return out, cube
    ref, cube_ref = run("four")
    assert [o[1]["received"] for o in ref][2] < 5 and max(o[1]["received"] for o in ref) > 2048 > min(o[1]["received"] for o in ref if o[1]["received"] > 100)
    for mode in ("spec", "nospec"):
        got, cube = run(mode)
        for k, ((ga, sa, ra, aa), (gb, sb, rb, ab)) in enumerate(zip(ref, got)):
            assert sa == sb, (mode, k, sa, sb)
            assert ga.tobytes() == gb.tobytes(), (mode, k)
            assert np.array_equal(ra["slots"], rb["slots"]) and ra["results"].tobytes() == rb["results"].tobytes() and np.array_equal(ra["path"], rb["path"]), (mode, k)
            for f in ("results", "delay", "phase", "pathMatch"):
                assert aa[f].tobytes() == ab[f].tobytes(), (mode, k, f)
        np.testing.assert_allclose(cube, cube_ref, rtol=0, atol=1e-18 + 1e-12 * np.abs(cube_ref).max())

    # three handles pipelined against one serial handle, rotations changing every pulse
    monkeypatch.setenv("RTS_SPECULATE", "1")
    seq = H.gpu_tracer(rts, c3); T.install(seq)
    want = []
    for k, count in enumerate(plan):
        seq.trace(tx["origin"], tx["span"], tx["dir"], c3["motion"], ray_first=0, ray_count=count)
        seq.finalise_patterns(pos, rot(k), wl, FC, CS)
        g = seq.aggregate(CS, FC)
        want.append((g, seq.received(), seq.aggregated()))
    seq.close()
    hs = [H.gpu_tracer(rts, c3) for _ in range(3)]
    for t in hs:
        T.install(t)
    got = [None] * len(plan); pending = []

    def finish(t, k):
        t.trace_end_patterns(pos, rot(k), wl, FC, CS)
        got[k] = (t.groups(), t.received(), t.aggregated())
    for k, count in enumerate(plan):
        t = hs[k % 3]
        t.trace_begin(tx["origin"], tx["span"], tx["dir"], c3["motion"], ray_first=0, ray_count=count)
        pending.append((t, k))
        if len(pending) == 3:
            finish(*pending.pop(0))
    while pending:
        finish(*pending.pop(0))
    for t in hs:
        t.close()
    for k in range(len(plan)):
        (ga, ra, aa), (gb, rb, ab) = want[k], got[k]
        assert ga.tobytes() == gb.tobytes(), k
        assert ra["results"].tobytes() == rb["results"].tobytes() and np.array_equal(ra["slots"], rb["slots"]), k
        for f in ("results", "delay", "phase", "pathMatch"):
            assert aa[f].tobytes() == ab[f].tobytes(), (k, f)


# ---------------------------------------------------------------------------------------------------- 4. errors and lifetime
def test_pattern_errors_and_lifetime(rts, scenes, monkeypatch):
    from rts_amd import _lib as L
    monkeypatch.setenv("RTS_SPECULATE", "1")
    spec = scenes.config_multi(W=20)
    n_t, n_rx = len(spec["meshes"]), len(spec["rx"])
    tx = spec["tx"]; pos = rx_positions(spec); wl = spec["c"] / spec["carrier"]
    T1 = Tables(rts, n_rx, n_t, seed=1); T2 = Tables(rts, n_rx, n_t, seed=2)

    def code(fn, *a):
        with pytest.raises(L.RtsError) as e:
            fn(*a)
        return e.value.code

    def reference(T, motion):
        t = H.gpu_tracer(rts, spec); T.install(t)
        t.trace(tx["origin"], tx["span"], tx["dir"], motion)
        t.finalise_patterns(pos, T.rot, wl, spec["carrier"], spec["c"])
        r = t.received()["results"]; t.close()
        return r

    tr = H.gpu_tracer(rts, spec)
    tr.trace(tx["origin"], tx["span"], tx["dir"], spec["motion"])
    fin = (pos, T1.rot, wl, spec["carrier"], spec["c"])
    assert code(tr.finalise_patterns, *fin) == L.RTS_ERR_INVALID                                    # no patterns set
    P = rts.Pattern.constant
    tr.set_patterns(P(1.0), [P(1.0)] * (n_rx + 1), [P(1.0)] * n_t)
    assert code(tr.finalise_patterns, *fin) == L.RTS_ERR_INVALID                                    # receivers differ
    tr.set_patterns(P(1.0), [P(1.0)] * n_rx, [P(1.0)] * (n_t - 1))
    assert code(tr.finalise_patterns, *fin) == L.RTS_ERR_INVALID                                    # targets differ
    tr.trace_begin(tx["origin"], tx["span"], tx["dir"], spec["motion"])
    assert code(tr.trace_end_patterns, *fin) == L.RTS_ERR_INVALID                                   # ... also for the fused call
    tr.trace_end()
    # a received set uploaded through rts_kernel_wrapper_on is not a traced pulse's
    T1.install(tr)
    Rk, D = 8, tr.depth
    rays = np.zeros(Rk, L.PRD_DTYPE); rays["power"] = 1.0; rays["received"] = 0; rays["rayLength"] = 400.0
    paths = np.full((Rk, D), -1, np.int32); dl = np.zeros(Rk); ph = np.zeros(Rk); pm = np.full(Rk, Rk + 1, np.int32)
    L.check(L.lib().rts_kernel_wrapper_on(tr.h, L.ptr(rays), L.ptr(paths), Rk, D, 1024, 65535, CS, FC, None, None, None, L.ptr(dl), L.ptr(ph), L.ptr(pm)))
    assert code(tr.finalise_patterns, *fin) == L.RTS_ERR_INVALID
    tr.close()

    # a failed rts_set_patterns leaves the previous tables working
    want1 = reference(T1, spec["motion"])
    tr = H.gpu_tracer(rts, spec); T1.install(tr)
    bad = rts.Pattern.separable([0.0, 0.0], [1.0, 1.0], [0.0], [1.0])
    assert code(tr.set_patterns, bad, [T1.pattern(t) for t in T1.rx], [T1.pattern(t) for t in T1.rcs]) == L.RTS_ERR_INVALID
    assert code(tr.set_patterns, T1.pattern(T1.tx), [T1.pattern(t) for t in T1.rx], [T1.pattern(t) for t in T1.rcs[:-1]] + [rts.Pattern.constant(-1.0)]) == L.RTS_ERR_INVALID
    tr.trace(tx["origin"], tx["span"], tx["dir"], spec["motion"])
    tr.finalise_patterns(pos, T1.rot, wl, spec["carrier"], spec["c"])
    assert tr.received()["results"].tobytes() == want1.tobytes()
    tr.close()

    # rts_set_patterns between two pipelined pulses takes effect from the next finalisation
    moved = [dict(m, position=tuple(np.add(m["position"], (0.4, 0.1, 0.0)))) for m in spec["motion"]]
    want2 = reference(T2, moved)
    assert want1.tobytes() != want2.tobytes()
    a, b = H.gpu_tracer(rts, spec), H.gpu_tracer(rts, spec)
    T1.install(a); T1.install(b)
    for t in (a, b):                                                 # a first pulse each: the next ones speculate
        t.trace(tx["origin"], tx["span"], tx["dir"], spec["motion"])
    a.trace_begin(tx["origin"], tx["span"], tx["dir"], spec["motion"])
    b.trace_begin(tx["origin"], tx["span"], tx["dir"], moved)
    a.trace_end_patterns(pos, T1.rot, wl, spec["carrier"], spec["c"])
    T2.install(a)                                                     # while a's chain may still be in flight
    b.trace_end_patterns(pos, T1.rot, wl, spec["carrier"], spec["c"])
    ra = a.received()["results"]
    a.trace_begin(tx["origin"], tx["span"], tx["dir"], moved)
    a.trace_end_patterns(pos, T2.rot, wl, spec["carrier"], spec["c"])
    ra2 = a.received()["results"]
    a.close(); b.close()
    # a's received() after the aggregation inside trace_end_patterns carries group values: compare against the same calls serially
    ref = H.gpu_tracer(rts, spec); T1.install(ref)
    ref.trace(tx["origin"], tx["span"], tx["dir"], spec["motion"])
    ref.finalise_patterns(pos, T1.rot, wl, spec["carrier"], spec["c"]); ref.aggregate(spec["c"], spec["carrier"])
    w1 = ref.received()["results"]
    T2.install(ref)
    ref.trace(tx["origin"], tx["span"], tx["dir"], moved)
    ref.finalise_patterns(pos, T2.rot, wl, spec["carrier"], spec["c"]); ref.aggregate(spec["c"], spec["carrier"])
    w2 = ref.received()["results"]
    ref.close()
    assert ra.tobytes() == w1.tobytes()
    assert ra2.tobytes() == w2.tobytes()
