"""Multistatic localisation on the device (rts_cube_locate: k_locate_plots / k_locate_track_*, k_locate_segs, k_locate_pairs, the scans,
k_locate_resolve, k_locate_write): every field of every target byte for byte against the host evaluator rts_locate_eval, on the cases
of tests/locate_ref.py (which tests/test_locate_host.py holds the evaluator to, against an independent restatement).  Every list goes
through device_list as a torch byte tensor.  Then the rounds of the resolution, determinism, both truncations, the track table as the
source, the handle's own plots from a painted range-Doppler map (plumbing: device_list NULL, the count read on the device), and the
whole chain on a scene the device traces itself (tests/locate_chain_ref.py; tests/test_locate_chain_host.py is the same chain on the
oracle's rays)."""
import ctypes as C
import math

import numpy as np
import pytest

import locate_ref as R

pytestmark = pytest.mark.gpu

SEGMENTS = ["seg0", "seg1", "seg63", "seg64", "seg65", "seg257"]      # anchor segments across a wave, a workgroup, a pair tile; 257: evaluator only
GROUND = np.array([[7000.0, 5000.0, 0.0], [20000.0, 0.0, 0.0], [-19000.0, -14000.0, 0.0], [-10000.0, 7000.0, 2000.0]])
WIDE = ((-4e4, -4e4, -13e3), (4e4, 4e4, 13e3))


def dev_bytes(a):
    import torch
    raw = np.frombuffer(np.ascontiguousarray(a).tobytes() + b"\0" * 8, np.uint8).copy()      # (never empty: an empty tensor has no address)
    return torch.from_numpy(raw).to("cuda")


def on_device(tr, c, **kw):
    buf = dev_bytes(c["list"])
    return tr.cube_locate(device_list=buf.data_ptr(), n_list=len(c["list"]), **dict(c["par"], **kw)), buf


def exact(tx, rx, x, v=(0.0, 0.0, 0.0)):
    return R.make_plots([(m, d, f, 2.0 + m) for m, (d, f) in enumerate(R.measure(tx, rx, x, v))])


def known(name):
    x = np.array([-9000.0, -11000.0, 5000.0])
    if name == "ground3":          # transmitter and anchors in the plane z = 0: both mirror roots are candidates of one set of records
        return dict(par=R.par(tx=np.zeros(3), rx_positions=GROUND[:3], carrier=0.0, box=WIDE), list=exact(np.zeros(3), GROUND[:3], x))
    if name == "ground4":          # ... and the fourth receiver decides
        return dict(par=R.par(tx=np.zeros(3), rx_positions=GROUND, box=WIDE), list=exact(np.zeros(3), GROUND, x, (30.0, -20.0, 10.0)))
    if name == "unrefined":        # everything in the plane, the target too: the third pivot of J^T J is 0
        flat = GROUND * [1.0, 1.0, 0.0]
        return dict(par=R.par(tx=np.zeros(3), rx_positions=flat, carrier=0.0, n_iters=2, box=((-4e4, -4e4, -1.0), (4e4, 4e4, 1.0))), list=exact(np.zeros(3), flat, x * [1.0, 1.0, 0.0]))
    if name == "nonfinite":        # records that take no part keep their places in the segments
        z = R.case("five_rx")["list"].copy()
        z["delay"][3] = math.nan; z["doppler"][20] = math.inf; z["power_sum"][41] = math.nan; z["delay"][70] = -math.inf
        return dict(par=R.case("five_rx")["par"], list=z)
    if name == "rx_beyond":        # records of receivers the call does not name are ignored
        z = R.case("five_rx")["list"]
        return dict(par=R.par(), list=z)
    raise KeyError(name)


KNOWN = ["ground3", "ground4", "unrefined", "nonfinite", "rx_beyond"]


def get_case(name):
    return known(name) if name in KNOWN else R.case(name)


@pytest.fixture(scope="module")
def tracer(rts):
    tr = rts.Tracer(8, 1)
    yield tr
    tr.close()


# ----------------------------------------------------------------------------- 1. every case, byte for byte
@pytest.mark.parametrize("name", [n for n in R.CASES if n not in SEGMENTS] + SEGMENTS + KNOWN)
def test_device_equals_evaluator(rts, tracer, name):
    c = get_case(name)
    got, _ = on_device(tracer, c)
    want = rts.locate_eval(c["list"], **c["par"])
    R.same_bytes(got, want)
    if name in R.CASES:
        assert len(got) == len(R.expected(name)[0])
    if name == "unrefined":
        assert got["flags"].tolist() == [rts.L.RTS_TARGET_UNREFINED]
    if name in ("seg257", "ground3", "ground4", "nonfinite", "rx_beyond"):
        assert len(got) >= 1


# ----------------------------------------------------------------------------- 2. the resolution alone, and its rounds
@pytest.mark.parametrize("name", list(R.CANDIDATES))
def test_resolution_and_its_rounds(rts, tracer, name):
    """the chain locks one candidate per round -- 70 rounds, more than a wave of candidates -- and ends by itself; disjoint candidates
    take one round; an empty list takes none"""
    L = rts.L
    c = R.CANDIDATES[name]
    buf = dev_bytes(c)
    got = tracer.cube_locate(device_list=buf.data_ptr(), n_list=len(c), **R.par(source="candidates"))
    assert got["candidate"].tolist() == R.CANDIDATE_WINNERS[name]
    R.same_bytes(got, rts.locate_eval(c, **R.par(source="candidates")))
    rounds = C.c_uint32(99)
    assert L.lib().rts_cube_locate_rounds(tracer.h, C.byref(rounds)) == L.RTS_OK and rounds.value == R.CANDIDATE_ROUNDS[name], rounds.value


def test_empty_plot_list_takes_no_round(rts, tracer):
    L = rts.L
    c = R.case("four_rx")
    buf = dev_bytes(c["list"])
    got = tracer.cube_locate(device_list=buf.data_ptr(), n_list=0, **c["par"])
    rounds = C.c_uint32(99)
    assert len(got) == 0 and L.lib().rts_cube_locate_rounds(tracer.h, C.byref(rounds)) == L.RTS_OK and rounds.value == 0


# ----------------------------------------------------------------------------- 3. determinism
def test_two_runs_and_two_handles_give_the_same_bytes(rts, tracer):
    c = R.case("five_rx")
    a, _ = on_device(tracer, c)
    b, _ = on_device(tracer, c)
    tr2 = rts.Tracer(8, 1)
    d, _ = on_device(tr2, c)
    tr2.close()
    assert len(a) == 16 and a.tobytes() == b.tobytes() == d.tobytes()


# ----------------------------------------------------------------------------- 4. the truncations
def test_truncations(rts, tracer):
    L = rts.L
    c = R.case("four_rx")
    full = rts.locate_eval(c["list"], **c["par"])
    assert len(full) == 12

    def get(capacity):
        out = np.full(16, 0x5a, np.uint8).repeat(144).view(R.TARGET)
        n = C.c_uint32(0)
        rc = L.lib().rts_cube_targets_get(tracer.h, rts.ptr(out), capacity, C.byref(n))
        return rc, n.value, out

    _, buf = on_device(tracer, c, fetch=False)
    rc, n, out = get(5)                                                 # the caller's array
    assert rc == L.RTS_ERR_CAPACITY and n == 12 and out[5:].tobytes() == b"\x5a" * (144 * 11)
    R.same_bytes(out[:5].copy(), full[:5].copy())
    rc, n, out = get(16)
    assert rc == L.RTS_OK and n == 12
    R.same_bytes(out[:12].copy(), full)
    on_device(tracer, c, fetch=False, max_targets=7)                    # the library's list
    rc, n, out = get(16)
    assert rc == L.RTS_ERR_CAPACITY and n == 12 and "max_targets 7" in L.lib().rts_last_error().decode() and out[7:].tobytes() == b"\x5a" * (144 * 9)
    R.same_bytes(out[:7].copy(), full[:7].copy())
    on_device(tracer, c, fetch=False, max_candidates=4)                 # the candidates: the stored prefix is resolved
    want = np.zeros(16, R.TARGET); nw = C.c_uint32(0)
    p, keep = rts._locate_params(**dict(c["par"], max_candidates=4))
    assert L.lib().rts_locate_eval(C.byref(p), rts.ptr(c["list"]), len(c["list"]), rts.ptr(want), 16, C.byref(nw)) == L.RTS_ERR_CAPACITY
    rc, n, out = get(16)
    assert rc == L.RTS_ERR_CAPACITY and "max_candidates" in L.lib().rts_last_error().decode() and n == nw.value and 1 <= n <= 4
    R.same_bytes(out[:n].copy(), want[:n].copy())
    assert out[n:].tobytes() == b"\x5a" * (144 * (16 - n))
    # an anchor's segment beyond RTS_LOCATE_MAX_PER_RX: its first 1024 records are used
    x = np.array([5000.0, -12000.0, 7000.0])
    m = R.measure(R.TX, R.RX5[:4], x)
    z = R.make_plots([(0, 1e-6, 0.0, 0.5)] * 1024 + [(0,) + m[0] + (1.0,)] + [(r,) + m[r] + (1.0,) for r in (1, 2, 3)])
    on_device(tracer, dict(par=R.par(), list=z), fetch=False)
    rc, n, out = get(16)
    assert rc == L.RTS_ERR_CAPACITY and n == 0 and "RTS_LOCATE_MAX_PER_RX" in L.lib().rts_last_error().decode()
    got, _ = on_device(tracer, dict(par=R.par(), list=z[1:].copy()))
    assert len(got) == 1 and got["plot"][0][0] == 1023


def test_refusals(rts):
    L = rts.L
    tr = rts.Tracer(8, 1)
    c = R.case("four_rx")
    buf = dev_bytes(c["list"])
    n = C.c_uint32(7)
    assert L.lib().rts_cube_targets_get(tr.h, None, 0, C.byref(n)) == L.RTS_ERR_INVALID and "no targets" in L.lib().rts_last_error().decode()
    ok = dict(c["par"], device_list=buf.data_ptr(), n_list=len(c["list"]))
    with pytest.raises(L.RtsError, match="no plots"):
        tr.cube_locate(**c["par"])
    with pytest.raises(L.RtsError, match="without device_list"):
        tr.cube_locate(**dict(c["par"], source="candidates"))
    first = tr.cube_locate(**ok)
    for kw, word in ((dict(gate=0.0), "gate"), (dict(sigma=(0.0, 1.0)), "sigma_delay"), (dict(anchors=(0, 0, 1)), "anchors"), (dict(min_receivers=2), "min_receivers"),
                     (dict(n_iters=9), "n_iters"), (dict(device_list=None), "without device_list"), (dict(device_list=buf.data_ptr() + 4), "8-byte"),
                     (dict(source="tracks"), "RTS_LOCATE_FROM_TRACKS"), (dict(box=((0, 0, 1.0), (1, 1, 0.0))), "box_lo")):
        with pytest.raises(L.RtsError, match=word):
            tr.cube_locate(**dict(ok, **kw))
    assert L.lib().rts_cube_locate(tr.h, None) == L.RTS_ERR_INVALID
    assert tr.cube_targets().tobytes() == first.tobytes() and len(first) == 12      # a refused call leaves the targets untouched
    tr.close()


# ----------------------------------------------------------------------------- 5. the track table as the source
def test_tracks_as_source(rts, tracer):
    """confirmed tracks that are not coasting, ordered by (rx, table index) on the device; plot[] holds table indices; the targets
    survive a new cube"""
    c = R.case("five_rx")
    z = c["list"]
    rng = np.random.default_rng(5)
    order = rng.permutation(len(z))
    tab = np.zeros(len(z) + 6, R.TRACK)
    for i, e in enumerate(order):
        tab[i]["id"], tab[i]["rx"], tab[i]["flags"], tab[i]["hits"] = i, z["rx"][e], rts.L.RTS_TRACK_CONFIRMED, 3
        tab[i]["delay"], tab[i]["doppler"], tab[i]["power_sum"], tab[i]["p_dd"], tab[i]["p_ff"] = z["delay"][e], z["doppler"][e], z["power_sum"][e], 1e-16, 4.0
    tab[len(z):] = tab[:6]
    tab["flags"][len(z):] = [0, 2, 3, 4, 1, 1]                          # tentative, coasted, confirmed and coasted, new: no part; two at a receiver beyond n_rx
    tab["rx"][len(z) + 4:] = [5, 200]
    tracer.cube_tracks_set(tab, 1000, 0.0)
    got = tracer.cube_locate(**dict(c["par"], source="tracks"))
    want = rts.locate_eval(tab, **dict(c["par"], source="tracks"))
    R.same_bytes(got, want)
    direct = rts.locate_eval(z, **c["par"])
    assert len(got) == len(direct) == 16 and sorted(got["power_sum"].tolist()) == sorted(direct["power_sum"].tolist())
    tracer.cube_attach(2, 1, 16, 0.0, 1e-8)
    assert tracer.cube_targets().tobytes() == got.tobytes()
    tracer.cube_tracks_reset()


# ----------------------------------------------------------------------------- 6. the handle's own plots
NB, ND, DT, PRI, WL = 256, 16, 20e-9, 1e-3, 0.5
S_TX = np.array([0.0, 0.0, 2.0])
S_RX = np.array([[150.0, 20.0, 5.0], [-90.0, 140.0, 40.0], [30.0, -160.0, 1.0], [-120.0, -100.0, 25.0]])
S_X = np.array([[60.0, 80.0, 150.0], [-220.0, -60.0, 130.0], [120.0, -150.0, 220.0]])
S_V = np.array([[20.0, -5.0, 3.0], [-12.0, 18.0, -6.0], [4.0, 9.0, 25.0]])


def test_handles_own_plots_from_a_painted_map(rts):
    """(plumbing, not accuracy -- each blob sits at the rounded cell of the exact measurement; the accuracy test is the traced scene below.)
    A range-Doppler map of four receivers with a 3 x 3 blob per (target, receiver) at the cell its bistatic delay and Doppler fall
    in -> OS-CFAR -> plots -> locate, nothing fetched in between.  The device targets equal the evaluator on the fetched plots byte
    for byte, and each lies within 2 |J+|_2 sqrt(K) delta of a true position: delta = cspeed dt / 2, the range-sum error of a cell's
    centre, J at the true position, the factor 2 for the linearisation"""
    import torch
    z = np.ones((4, ND, NB), np.complex128)
    for t in range(3):
        for m, (d, f) in enumerate(R.measure(S_TX, S_RX, S_X[t], S_V[t], WL)):
            r, k = int(round(d / DT)), int(round(f * ND * PRI)) % ND
            assert 4 < r < NB - 4 and abs(f) < 0.5 / PRI
            for dk in (-1, 0, 1):
                for dr in (-1, 0, 1):
                    z[m, (k + dk) % ND, r + dr] = 40.0 / (1 + abs(dk) + abs(dr))
    tr = rts.Tracer(8, 1)
    tr.cube_attach(4, 1, NB, 0.0, DT)
    m_dev = torch.from_numpy(z).to("cuda")
    tr.cube_detect_os(guard=(1, 1), train=(4, 2), rank=30, alpha=6.0, local_max=False, pri=PRI, device_ptr=m_dev.data_ptr(), n_doppler=ND, fetch=False)
    tr.cube_plots((1, 1), pri=PRI, fetch=False)
    par = dict(tx=S_TX, rx_positions=S_RX, cspeed=R.C0, carrier=R.C0 / WL, sigma=(DT / 2, 0.5 / (ND * PRI)), gate=9.21, assoc_delay=20 * DT,
               box=((-400.0, -400.0, 0.0), (400.0, 400.0, 400.0)), n_iters=4)
    got = tr.cube_locate(**par)
    plots = tr.plots()
    assert len(plots) == 12
    R.same_bytes(got, rts.locate_eval(plots, **par))
    assert len(got) == 3
    delta = R.C0 * DT / 2
    for x in S_X:
        J = np.array([(x - S_TX) / np.linalg.norm(x - S_TX) + (x - s) / np.linalg.norm(x - s) for s in S_RX])
        bound = 2.0 * np.linalg.norm(np.linalg.pinv(J), 2) * math.sqrt(4) * delta
        err = min(float(np.linalg.norm(g["pos"] - x)) for g in got)
        print("target", x, "error", err, "bound", bound)
        assert err <= bound
    tr.close()


# ----------------------------------------------------------------------------- 7. the whole chain on a traced scene
def test_traced_scene_end_to_end(rts):
    """one tracing handle, four receiver spheres that do not lie in one plane with the transmitter, three small moving bodies (faceted:
    tests/locate_chain_ref.py says why), a [4][16][64] cube: trace, accumulate, noise, Doppler, detect, plots, locate, nothing fetched
    in between.  The device targets equal the evaluator on the fetched plots byte for byte; the plots are the twelve of the scene;
    each target lies within 2 |J+|_2 sqrt(K) delta of a body's centre, delta = cspeed dt / 2 + 2 REACH (tests/test_locate_chain_host.py
    certifies the scene on the oracle's rays)"""
    import helpers as H
    import locate_chain_ref as LC
    spec = LC.spec(rts)
    tr = H.gpu_tracer(rts, spec)
    tr.cube_attach(LC.N_RX, LC.N_PULSES, LC.N_BINS, LC.T0, LC.DT)
    for m in range(LC.N_PULSES):
        H.gpu_trace(rts, spec, tr=tr, motion=LC.motion(m))
        tr.finalise_uniform(None, LC.WL, 1.0, 1.0, LC.FC, LC.CS)
        tr.cube_accumulate(m, LC.CS, LC.FC)
    tr.cube_add_noise(LC.NOISE_POWER, LC.NOISE_SEED)
    tr.cube_doppler(LC.N_PULSES, fetch=False)
    tr.cube_detect_os(fetch=False, **LC.CFAR)
    tr.cube_plots((0, 0), pri=LC.PRI, fetch=False)
    got = tr.cube_locate(**LC.PAR)
    plots = tr.plots()
    LC.check_plots(plots)
    R.same_bytes(got, rts.locate_eval(plots, **LC.PAR))
    LC.check_targets(got)
    tr.close()
