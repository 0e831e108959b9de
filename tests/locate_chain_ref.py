"""What tests/test_locate_chain_host.py and tests/test_gpu_locate.py share: the one scene in which the ray tracer itself makes the cube
that multistatic localisation works on -- a transmitter, four capture spheres that do not lie in one plane with it, three small
bodies that move a few millimetres per pulse -- and the chain accumulate -> Doppler -> detect -> plots -> locate on that cube through
the library's own host evaluators, with the bound the targets are held to.

Why the bodies are faceted, not smooth.  A smooth sphere reflects into a capture sphere the few rays of the launch lattice that hit
its specular patch: some dozens of 10^6, a set that changes from pulse to pulse as the body moves, each ray with its own path length
of many wavelengths -- the slow-time spectrum of such a return is splatter (measured on the oracle: 0 to 68 rays per pair and pulse,
61 plots where 12 were due).  A coherent return from few rays needs a flat facet that sends EVERY ray it receives to one receiver,
as the plate of tests/array_ref.py does.  So a body here is four square facets of 0.6 m around its centre, facet k on the side of
receiver k and turned so that the transmitter's rays leave it towards receiver k (its normal bisects the two directions at pulse 0;
the bodies only translate).  Each body moves along the transmitter's ray through its centre, so a lattice ray that hits a facet at one pulse
hits it at every pulse: test a of the host twin holds the ray counts to be the same at all 16 pulses.

What the cube's delay is.  The reflecting point lies on a facet, at most REACH = 1.3 + 0.3 sqrt(2) m from the body's centre, which
moves the range sum by at most 2 REACH; so a range sum read from the cube is within
    delta = cspeed dt / 2  (the cell)  +  2 REACH  (the reflecting point: the issue's 2 radius, the body's reach for the sphere's)
of |x - tx| + |x - s_k|.  The capture spheres (radius RHO) add nothing to it: measured on the oracle, every received ray's length is
0.79 to 1.39 m short of its body's range sum with capture spheres of 6 m, and 0.79 to 1.68 m with 3 m ones and facets twice as
wide -- the facets' reach, not RHO.  Test a of the host twin holds every ray to 2 REACH.  The cube's first delay is chosen so that
every return stays in ONE range cell while its body moves (a return that straddles two cells is modulated in both).

The noise.  A facet's return is the sum of ~900 rays whose lengths spread over tens of wavelengths, so its amplitude wanders by a
fraction of a percent from pulse to pulse and leaves slow-time leakage some 40 dB under its peak; on a noise-free map, where the
CFAR threshold is 0, that leakage would be detected.  The cube therefore gets the library's receiver noise (rts_cube_add_noise /
rts_noise_eval, one seed) 30 dB under the weakest return's peak in the map (1.5e-9; the strongest is 2.5e-8), and the detector a
threshold 23 dB over the noise: about 4e-10, above the far slow-time leakage of the strongest return (24 dB under its peak: 1e-10,
where the noise would otherwise make local maxima of it) and under the weakest peak.

The chain.  Impulse accumulation (rts_cube_accumulate's rule, tests/cube_ref.py) into [4][16][64], the noise, the 16-point slow-time
DFT, OS-CFAR with range-only training (rank 6 of 8: two training cells may hold another body's return) WITH the
local-maximum rule -- along Doppler the leakage of a constant-amplitude return falls monotonically away from its peak, so each
(body, receiver) gives one detection, refined to a fraction of a cell --, plots with link (0, 0), which pass the detections'
refinement through, and locate."""
import functools
import math

import numpy as np

import cube_ref as CR
import locate_ref as R
from rts_amd import scenes

CS, FC = scenes.C0, scenes.FC
WL = CS / FC
TX = np.array([-300.0, 0.0, 0.0])
SX = np.array([[0.0, 0.0, 0.0], [25.0, 5.5, -3.5], [-30.0, -5.0, 4.5]])           # the bodies' centres at pulse 0
SPEED = np.array([6.0, -4.5, 3.0])                                               # m / s, away from the transmitter along its ray through the centre
SV = np.array([v * (x - TX) / np.linalg.norm(x - TX) for v, x in zip(SPEED, SX)])
RXP = np.array([[-60.0, 80.0, 10.0], [-50.0, -85.0, 30.0], [-70.0, 20.0, 75.0], [-45.0, -15.0, -80.0]])
OUT, HALF = 1.3, 0.3                                                              # a facet's centre from the body's, its half side
REACH = OUT + HALF * math.sqrt(2.0)
RHO, W, SPAN = 6.0, 100, 0.0613
N_RX, N_PULSES, N_BINS, DT, PRI = 4, 16, 64, 40.0e-9, 5.0e-4
CFAR = dict(guard=(1, 0), train=(4, 0), rank=6, alpha=200.0, local_max=True, pri=PRI)
NOISE_POWER, NOISE_SEED = 1.0e-13, 20264                                        # per cube sample: 1.6e-12 in a cell of the 16-point map, whose weakest return peaks at 1.5e-9
BOX = ((-60.0, -30.0, -30.0), (60.0, 30.0, 30.0))


def true_range_sum(x, m):
    return float(np.linalg.norm(x - TX) + np.linalg.norm(x - RXP[m]))


SHORT = (0.7, 1.5)      # a received ray's length is this much short of its body's |x - tx| + |x - s_k| (what the host twin measures: 0.79 .. 1.39 m)


def _t0():
    """the cube's first delay: 40 to 52 m before the nearest return, chosen so that at every pulse every (body, receiver) pair's rays
    fall into ONE range cell, at least 0.25 m inside it -- a return that straddles two cells while its body moves is modulated in both"""
    first = min(true_range_sum(SX[s], m) for s in range(3) for m in range(N_RX)) - 40.0
    for step in range(48):
        start = first - 0.25 * step
        ok = True
        for s in range(3):
            for m in range(N_RX):
                cells = [(true_range_sum(SX[s] + SV[s] * (pulse * PRI), m) - short - start) / (CS * DT) for pulse in (0, N_PULSES - 1) for short in SHORT]
                inside = 0.25 / (CS * DT)
                ok = ok and math.floor(min(cells) - inside) == math.floor(max(cells) + inside)
        if ok:
            return start / CS
    raise AssertionError("no first delay keeps every return in one cell")




T0 = _t0()
PAR = dict(tx=TX, rx_positions=RXP, cspeed=CS, carrier=FC, sigma=(DT / 2, 0.25 / (N_PULSES * PRI)), gate=9.21, assoc_delay=2 * DT, box=BOX, anchors=(0, 1, 2),
           min_receivers=None, n_iters=4, max_candidates=0, max_targets=0, source="plots")


def centre(s, pulse):
    return SX[s] + SV[s] * (pulse * PRI)


def motion(pulse):
    return [dict(position=tuple(centre(s, pulse)), velocity=tuple(SV[s])) for s in range(3)]


def unit(a):
    return a / np.linalg.norm(a)


def body_mesh(s):
    """four facets in the body's own frame (its centre at the origin): facet k sits OUT towards receiver k, across the transmitter's
    ray, and its normal bisects the directions to the transmitter and to receiver k"""
    ray = unit(SX[s] - TX)
    verts, tris, normals = [], [], []
    for k in range(N_RX):
        side = RXP[k] - SX[s]
        side = unit(side - (side @ ray) * ray)
        c = OUT * side
        n = unit(unit(TX - (SX[s] + c)) + unit(RXP[k] - (SX[s] + c)))
        e1 = unit(np.cross(n, ray)); e2 = np.cross(n, e1)
        q = [c - HALF * e1 - HALF * e2, c + HALF * e1 - HALF * e2, c + HALF * e1 + HALF * e2, c - HALF * e1 + HALF * e2]
        for a, b, d in ((0, 2, 1), (0, 3, 2)):      # (the winding of scenes.plate_mesh: the stated normal against the geometric one)
            base = len(verts)
            verts += [q[a], q[b], q[d]]; normals += [n, n, n]; tris.append([base, base + 1, base + 2])
    return np.array(verts, np.float64), np.array(tris, np.uint32), np.array(normals, np.float64)


def spec(rts):
    meshes = []
    for s in range(3):
        v, t, n = body_mesh(s)
        meshes.append(dict(tris=t, verts=v, normals=n, refl_coeff=0.9, refr_index=1.0))
    rx = [scenes._rx_at(p, (0.0, 0.0, 0.0), RHO, 2.6) for p in RXP]
    return dict(name="locate-chain", W=W, max_refl=1, smooth=True, n_pulses=N_PULSES, meshes=meshes, motion=motion(0),
                tx=dict(origin=tuple(TX), span=(SPAN, SPAN, 0.0), dir=(0.0, 0.0)), rx=rx, carrier=FC, c=CS)


@functools.lru_cache(maxsize=None)
def oracle_launches(rts, oracle):
    """per pulse the finalised received records of one oracle launch"""
    import helpers as H
    out = []
    for m in range(N_PULSES):
        o = H.oracle_trace(oracle, spec(rts), motion=motion(m))
        rec, _, _ = oracle.filter_finalise(o["results"], o["path"], [1.0, 1.0, 1.0], WL, 1.0, 1.0, FC, CS)
        out.append(rec)
    return out


def pair_counts(launches):
    """[pulse][receiver][body]: the received rays whose first hit lies on that body"""
    n = np.zeros((N_PULSES, N_RX, 3), np.int64)
    for m, rec in enumerate(launches):
        for s in range(3):
            on = np.linalg.norm(rec["firstHitPoint"] - centre(s, m), axis=1) < REACH + 0.5
            for k in range(N_RX):
                n[m, k, s] = int(np.sum(on & (rec["received"] == k)))
    return n


def shortfalls(launches):
    """per received ray: |x - tx| + |x - s_k| of its body's centre minus its length"""
    out = []
    for m, rec in enumerate(launches):
        for s in range(3):
            on = np.linalg.norm(rec["firstHitPoint"] - centre(s, m), axis=1) < REACH + 0.5
            for k in range(N_RX):
                sel = on & (rec["received"] == k)
                out.extend((true_range_sum(centre(s, m), k) - rec["rayLength"][sel]).tolist())
    return np.array(out)


def noise(rts):
    n = N_RX * N_PULSES * N_BINS
    return rts.noise_eval(NOISE_SEED, np.arange(n, dtype=np.uint64), NOISE_POWER).reshape(N_RX, N_PULSES, N_BINS)


def plots_of(rts, cube):
    """the library's host evaluators from a cube [4][16][64] to plots"""
    zmap = CR.to_double(CR.dft_ref(cube, N_PULSES))
    det = rts.cfar_os_eval(zmap, t0=T0, dt=DT, **CFAR)
    return rts.plots_eval(det, N_PULSES, link=(0, 0), pri=PRI, t0=T0, dt=DT, n_rx=N_RX, n_bins=N_BINS)


@functools.lru_cache(maxsize=None)
def host_chain(rts, oracle):
    launches = oracle_launches(rts, oracle)
    cube = np.zeros((N_RX, N_PULSES, N_BINS), CR.CLD)
    for m, rec in enumerate(launches):
        CR.accumulate_ref(cube, m, CR.contribs_rays(rec, CS, FC), T0, DT)
    clean = CR.to_double(cube)
    cube = clean + noise(rts)
    plots = plots_of(rts, cube)
    return dict(counts=pair_counts(launches), short=shortfalls(launches), clean=clean, cube=cube, plots=plots, targets=rts.locate_eval(plots, **PAR))


def delta():
    """the range-sum error a cell's centroid and the reflecting point can cause (the module's docstring)"""
    return CS * DT / 2 + 2 * REACH


def position_bound(x, K=N_RX):
    """2 |J+|_2 sqrt(K) delta, J at the true position x; the factor 2 is the margin for the linearisation"""
    J = np.array([(x - TX) / np.linalg.norm(x - TX) + (x - s) / np.linalg.norm(x - s) for s in RXP])
    return 2.0 * float(np.linalg.norm(np.linalg.pinv(J), 2)) * math.sqrt(K) * delta()


def doppler_of(s, k):
    x = centre(s, (N_PULSES - 1) / 2.0)
    return -(1.0 / WL) * float((unit(x - TX) + unit(x - RXP[k])) @ SV[s])


def check_plots(plots, show=print):
    """twelve plots, per receiver one per body: its Doppler within a cell of the body's, its range sum within a cell + 2 REACH (an
    impulse lands in the cell that holds its delay and a one-cell plot reports the cell's START, so a plot's delay is early by up to a
    whole cell; the targets below are still held to the issue's delta, which has half a cell)"""
    assert len(plots) == 12 and [int(np.sum(plots["rx"] == m)) for m in range(N_RX)] == [3, 3, 3, 3], len(plots)
    cell = 1.0 / (N_PULSES * PRI)
    for z in plots:
        k = int(z["rx"])
        err = [(abs(CS * z["delay"] - true_range_sum(centre(s, 7.5), k)), abs(z["doppler"] - doppler_of(s, k))) for s in range(3)]
        s = int(np.argmin([e[0] for e in err]))
        show("receiver %d body %d: range sum off by %.2f m (a cell + 2 REACH: %.2f), Doppler off by %.1f Hz (cell %.0f)" % (k, s, err[s][0], CS * DT + 2 * REACH, err[s][1], cell))
        assert err[s][0] <= CS * DT + 2 * REACH and err[s][1] <= cell, (k, s, err[s])


def check_targets(targets, show=print):
    """three targets, each within its bound of a body's centre at mid-interval, made of four receivers' plots"""
    assert len(targets) == 3, len(targets)
    mid = (N_PULSES - 1) / 2.0
    for s in range(3):
        x = centre(s, mid)
        err = [float(np.linalg.norm(t["pos"] - x)) for t in targets]
        k = int(np.argmin(err))
        show("body %d: position error %.3f m (bound %.3f m), velocity error %.3f m/s, K = %d, cost %.3g" % (
            s, err[k], position_bound(x), float(np.linalg.norm(targets[k]["vel"] - SV[s])), targets[k]["n_receivers"], targets[k]["cost"]))
        assert err[k] <= position_bound(x), (s, err[k], position_bound(x))
        assert targets[k]["n_receivers"] == N_RX


def margins(plots):
    """the least relative distance of a decision from its threshold, in the longdouble restatement of tests/locate_ref.py"""
    mg = R.Margins()
    ref, cut = R.locate(PAR, plots, np.longdouble, mg)
    return mg.least, R.records(ref), cut
