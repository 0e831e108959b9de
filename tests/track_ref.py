"""An independent restatement of the tracker step (include/rts_amd.h: RtsTrackParams, RtsTrack) in plain Python floats, and the cases
the host and the GPU tests share.  Nothing here is the library's code: every expression is written out again from the header text, the
candidates come from a full sort per track, and the matching is the SERIAL greedy pass over all kept edges sorted by (d2, track, plot)
-- the kernels reach it by rounds of locally dominant edges, the evaluator by its own sort.

    step(par, tracks, next_id, T, plots) -> (the stored TRACK array, total, next_id)
    CASES: name -> a function returning dict(par, tracks, next_id, T, plots);  case(name) builds it (cached)
    sequence(seed) -> the 40-frame scene of the sequence test"""
import functools
import math
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TRACK = np.dtype([("id", "<u8"), ("rx", "<u4"), ("flags", "<u4"), ("hits", "<u4"), ("misses", "<u4"), ("age", "<u4"), ("plot_index", "<u4"),
                  ("delay", "<f8"), ("doppler", "<f8"), ("p_dd", "<f8"), ("p_df", "<f8"), ("p_ff", "<f8"), ("d2", "<f8"), ("power_sum", "<f8")])
PLOT = np.dtype([("rx", "<u4"), ("n_cells", "<u4"), ("first_index", "<u4"), ("peak_index", "<u4"), ("range_min", "<u4"), ("range_max", "<u4"),
                 ("doppler_lo", "<u4"), ("doppler_span", "<u4"), ("power_sum", "<f8"), ("peak_power", "<f8"), ("noise_sum", "<f8"),
                 ("range_centroid", "<f8"), ("doppler_centroid", "<f8"), ("range_spread", "<f8"), ("doppler_spread", "<f8"), ("delay", "<f8"),
                 ("doppler", "<f8")])
assert TRACK.itemsize == 88 and PLOT.itemsize == 104
CONFIRMED, COASTED, NEW, NONE = 1, 2, 4, 0xffffffff
DEFAULT_TRACKS = 16384
PAR = dict(gate=9.21, sigma=(1.0, 1.0), q=0.0, delay_rate_per_hz=0.0, doppler_period=0.0, confirm_hits=3, max_misses=3, tentative_misses=0,
           max_candidates=16, max_tracks=0)


def par(**kw):
    p = dict(PAR); p.update(kw)
    return p


# ----------------------------------------------------------------------------- the restatement
def wrap(x, period):
    if not period > 0.0:
        return x
    h = 0.5 * period
    r = x - period * float(math.floor((x + h) / period))
    if r >= h:
        r -= period
    elif r < -h:
        r += period
    return r


def predict(t, p, T):
    a = p["delay_rate_per_hz"] * T
    sd, sf = p["sigma"]
    d = t["delay"] + a * t["doppler"]
    u = t["p_df"] + a * t["p_ff"]
    pdd = ((t["p_dd"] + a * t["p_df"]) + a * u) + p["q"] * (((a * a) * T) / 3.0)
    pdf = u + p["q"] * ((a * T) / 2.0)
    pff = t["p_ff"] + p["q"] * T
    s_dd = pdd + sd * sd
    s_ff = pff + sf * sf
    return dict(d=d, f=t["doppler"], pdd=pdd, pdf=pdf, pff=pff, s_dd=s_dd, s_ff=s_ff, det=s_dd * s_ff - pdf * pdf)


def innovation(r, zd, zf, period):
    return zd - r["d"], wrap(zf - r["f"], period)


def distance(r, zd, zf, period):
    vd, vf = innovation(r, zd, zf, period)
    return ((((vd * vd) * r["s_ff"]) - ((2.0 * (vd * vf)) * r["pdf"])) + ((vf * vf) * r["s_dd"])) / r["det"] + 0.0


def step(p, tracks, next_id, T, plots):
    """one frame: (the records a table of max_tracks stores, the total, the next id)"""
    period, gate, K = p["doppler_period"], p["gate"], p["max_candidates"]
    table = p["max_tracks"] or DEFAULT_TRACKS
    tr = [{k: (float(t[k]) if TRACK[k].kind == "f" else int(t[k])) for k in TRACK.names} for t in tracks]
    z = [(int(q["rx"]), float(q["delay"]), float(q["doppler"]), float(q["power_sum"])) for q in plots]
    finite = [math.isfinite(q[1]) and math.isfinite(q[2]) for q in z]
    pred = [predict(t, p, T) for t in tr]
    edges = []
    for i, (t, r) in enumerate(zip(tr, pred)):
        mine = []
        for j, (rx, zd, zf, _) in enumerate(z):
            if rx != t["rx"] or not finite[j]:
                continue
            d2 = distance(r, zd, zf, period)
            if 0.0 <= d2 <= gate:
                mine.append((d2, j))
        mine.sort()
        edges.extend((d2, i, j) for d2, j in mine[:K])
    edges.sort()
    of_track, of_plot = {}, {}
    for d2, i, j in edges:
        if i not in of_track and j not in of_plot:
            of_track[i] = (j, d2); of_plot[j] = i
    out = []
    for i, (t, r) in enumerate(zip(tr, pred)):
        o = dict(t)
        o["age"] = (t["age"] + 1) & 0xffffffff
        if i in of_track:
            j, d2 = of_track[i]
            _, zd, zf, pw = z[j]
            vd, vf = innovation(r, zd, zf, period)
            k_dd = ((r["pdd"] * r["s_ff"]) - (r["pdf"] * r["pdf"])) / r["det"]
            k_df = ((r["pdf"] * r["s_dd"]) - (r["pdd"] * r["pdf"])) / r["det"]
            k_fd = ((r["pdf"] * r["s_ff"]) - (r["pff"] * r["pdf"])) / r["det"]
            k_ff = ((r["pff"] * r["s_dd"]) - (r["pdf"] * r["pdf"])) / r["det"]
            o["delay"] = r["d"] + ((k_dd * vd) + (k_df * vf))
            o["doppler"] = wrap(r["f"] + ((k_fd * vd) + (k_ff * vf)), period)
            o["p_dd"] = r["pdd"] - ((k_dd * r["pdd"]) + (k_df * r["pdf"]))
            o["p_df"] = r["pdf"] - ((k_dd * r["pdf"]) + (k_df * r["pff"]))
            o["p_ff"] = r["pff"] - ((k_fd * r["pdf"]) + (k_ff * r["pff"]))
            o["hits"] = (t["hits"] + 1) & 0xffffffff; o["misses"] = 0
            o["flags"] = (t["flags"] & CONFIRMED) | (CONFIRMED if o["hits"] >= p["confirm_hits"] else 0)
            o["plot_index"] = j; o["d2"] = d2; o["power_sum"] = pw
        else:
            o["delay"], o["doppler"], o["p_dd"], o["p_df"], o["p_ff"] = r["d"], r["f"], r["pdd"], r["pdf"], r["pff"]
            o["misses"] = (t["misses"] + 1) & 0xffffffff
            o["flags"] = (t["flags"] & CONFIRMED) | COASTED
            o["plot_index"] = NONE; o["d2"] = 0.0; o["power_sum"] = 0.0
            if o["misses"] > (p["max_misses"] if t["flags"] & CONFIRMED else p["tentative_misses"]):
                continue
        out.append(o)
    survivors = len(out)
    sd, sf = p["sigma"]
    for j, (rx, zd, zf, pw) in enumerate(z):
        if j in of_plot or not finite[j]:
            continue
        out.append(dict(id=next_id + (len(out) - survivors), rx=rx, flags=NEW | (CONFIRMED if 1 >= p["confirm_hits"] else 0), hits=1, misses=0, age=1, plot_index=j,
                        delay=zd, doppler=wrap(zf, period), p_dd=sd * sd, p_df=0.0, p_ff=sf * sf, d2=0.0, power_sum=pw))
    total = len(out)
    stored = min(total, table)
    rec = np.zeros(stored, TRACK)
    for k, o in enumerate(out[:stored]):
        rec[k] = tuple(o[name] for name in TRACK.names)
    return rec, total, next_id + (stored - survivors)


def same_bytes(got, want):
    assert got.dtype == want.dtype == TRACK
    assert len(got) == len(want), (len(got), len(want))
    if got.tobytes() != want.tobytes():
        for i, (a, b) in enumerate(zip(got, want)):
            for name in TRACK.names:
                assert a[name].tobytes() == b[name].tobytes(), "record %d, %s: %r != %r" % (i, name, a[name], b[name])


# ----------------------------------------------------------------------------- building blocks
def make_plots(rows):
    """rows of (rx, delay, doppler[, power_sum]); the other fields carry a pattern the step must not read"""
    z = np.zeros(len(rows), PLOT)
    for j, row in enumerate(rows):
        z[j]["rx"], z[j]["delay"], z[j]["doppler"] = row[0], row[1], row[2]
        z[j]["power_sum"] = row[3] if len(row) > 3 else 1.0 + j
    z["n_cells"] = 7; z["first_index"] = 0xdeadbeef; z["peak_power"] = math.nan; z["range_centroid"] = -1.0; z["doppler_centroid"] = math.inf
    return z


def make_tracks(rows, first_id=100):
    """rows of dict(rx, delay, doppler, ...); the defaults: a tentative track of one hit with covariance diag(1, 1)"""
    t = np.zeros(len(rows), TRACK)
    for i, row in enumerate(rows):
        d = dict(id=first_id + i, rx=0, flags=0, hits=1, misses=0, age=1, plot_index=NONE, delay=0.0, doppler=0.0, p_dd=1.0, p_df=0.0, p_ff=1.0, d2=0.0, power_sum=0.0)
        d.update(row)
        t[i] = tuple(d[name] for name in TRACK.names)
    return t


def frame(p, tracks, plots, next_id=1000, T=1.0):
    return dict(par=p, tracks=make_tracks(tracks) if not isinstance(tracks, np.ndarray) else tracks,
                plots=make_plots(plots) if not isinstance(plots, np.ndarray) else plots, next_id=next_id, T=T)


def line(xs, rx=0, f=0.0):
    return [(rx, float(x), f) for x in xs]


# S = diag(1, 1): a track that stands exactly where it was measured (covariance 0) and unit sigmas, so d2 is the squared distance
EXACT = dict(p_dd=0.0, p_ff=0.0)


def c_gate(above):
    # P = diag(3, 3), sigma 1: S = diag(4, 4), det 16; v = (4, 0): d2 = (16 * 4) / 16 = 4 exactly.  One ulp more delay: above.
    zd = 4.0 + (2.0 ** -50 if above else 0.0)
    return frame(par(gate=4.0), [dict(p_dd=3.0, p_ff=3.0)], [(0, zd, 0.0)])


def c_abc():
    # d2: A-1 = 0.5, B-1 = 1, B-2 = 2, C-2 = 3; A-2 and C-1 lie outside the gate.  Greedy: A-1, B-2, C coasts.
    a, p2 = -math.sqrt(0.5), 1.0 + math.sqrt(2.0)
    return frame(par(gate=3.5), [dict(delay=a, **EXACT), dict(delay=1.0, **EXACT), dict(delay=p2 + math.sqrt(3.0), **EXACT)], line([0.0, p2]))


def c_chain(n):
    # plot 0 < track 0 < plot 1 < track 1 < ..: the gaps shrink along the chain, so every track prefers its right plot and every plot
    # its right track; only the last pair is locally dominant, then the one before it: one pair locks per round
    gap = lambda m: 1.9 - 0.005 * m
    x, plots, tracks = 0.0, [], []
    for k in range(n):
        plots.append(x); x += gap(2 * k); tracks.append(x); x += gap(2 * k + 1)
    plots.append(x)
    return frame(par(gate=4.5), [dict(delay=v, **EXACT) for v in tracks], line(plots))


def c_pairs(n):
    return frame(par(), [dict(delay=10.0 * k, doppler=float(k % 7), rx=k % 3) for k in range(n)],
                 sorted([(k % 3, 10.0 * k + 0.25, float(k % 7) - 0.5) for k in range(n)], key=lambda r: r[0]))


def c_truncate(n_plots, K):
    # track 0 gates n_plots plots at 0.01, 0.02, ..; 16 tracks stand ON the 16 nearest and take them.  With the 17th edge kept the greedy
    # pass would give it to track 0; it is dropped before the matching, so track 0 coasts.
    xs = [0.01 * (m + 1) for m in range(n_plots)]
    return frame(par(gate=9.0, max_candidates=K), [dict(delay=0.0, **EXACT)] + [dict(delay=xs[m], **EXACT) for m in range(16)], line(xs))


def c_wrap(kappa, period):
    # innovations across +-period / 2, a state that leaves [-period / 2, period / 2) in the update and is wrapped back
    a = kappa * 0.5
    tracks = [dict(delay=10.0, doppler=498.0), dict(delay=50.0, doppler=-499.0), dict(delay=90.0, doppler=499.9, p_ff=4.0), dict(delay=130.0, doppler=100.0)]
    plots = [(0, 10.2 + a * 498.0, -499.0), (0, 50.1 - a * 499.0, 499.5), (0, 89.9 + a * 499.9, -498.9), (0, 130.0 + a * 100.0, 100.5), (0, 300.0, 1700.0)]
    return frame(par(delay_rate_per_hz=kappa, doppler_period=period, q=0.5), tracks, plots, T=0.5)


def c_receivers():
    tracks = [dict(rx=0, delay=5.0, doppler=5.0), dict(rx=1, delay=20.0), dict(rx=2, delay=7.0), dict(rx=3, delay=5.0, doppler=5.0)]
    return frame(par(), tracks, [(0, 20.0, 0.0), (1, 5.0, 5.0), (3, 5.5, 5.0), (5, 7.0, 0.0)])      # (receivers 2 and 4 have no plots)


def c_nonfinite():
    tracks = [dict(delay=0.0), dict(delay=10.0), dict(delay=20.0)]
    return frame(par(), tracks, [(0, math.nan, 0.0), (0, 0.5, 0.0), (0, 10.0, math.inf), (0, -math.inf, 0.0), (0, 10.0, math.nan), (0, 20.0, 0.25), (0, 99.0, -math.inf)])


def c_lifecycle():
    # confirm_hits 3, max_misses 2, tentative_misses 1.  Matched: hits 1 -> 2 (tentative), 2 -> 3 (confirmed now), confirmed stays.
    # Unmatched: tentative with misses 0 (kept: 1), misses 1 (deleted: 2 > 1); confirmed with misses 1 (kept), misses 2 (deleted: 3 > 2).
    far = 1000.0
    tracks = [dict(delay=0.0, hits=1), dict(delay=far, misses=1), dict(delay=10.0, hits=2), dict(delay=2 * far, flags=CONFIRMED, hits=5, misses=2),
              dict(delay=20.0, flags=CONFIRMED | COASTED, hits=7, misses=2), dict(delay=3 * far, misses=0), dict(delay=4 * far, flags=CONFIRMED | NEW, hits=3, misses=1)]
    return frame(par(max_misses=2, tentative_misses=1), tracks, line([500.0, 0.1, 20.2, 10.3, 600.0]), next_id=(1 << 40) + 5)


def c_full(max_tracks, third):
    # four tracks: the second coasts and stays (tentative_misses 1), the third is deleted (at 1000) or matched (at 100)
    tracks = [dict(delay=0.0), dict(delay=10.0), dict(delay=third, misses=1), dict(delay=20.0)]
    return frame(par(max_tracks=max_tracks, tentative_misses=1), tracks, line([0.5, 100.0, 200.0, 20.5, 300.0]), next_id=7)


def c_random(seed, grid):
    rng = np.random.default_rng(seed)
    nT, nP = 300, 500
    if grid:      # integer coordinates on a small lattice, S = diag(1, 1): exact ties abound
        td, tf, zd, zf = (rng.integers(0, 24, n).astype(float) for n in (nT, nT, nP, nP))
        tracks = [dict(rx=int(rng.integers(0, 2)), delay=td[i], doppler=tf[i], hits=int(rng.integers(1, 5)), misses=int(rng.integers(0, 3)),
                       flags=int(rng.integers(0, 2)), **EXACT) for i in range(nT)]
        p = par(gate=8.0, max_candidates=int(4))
    else:
        td, zd = rng.uniform(0, 300, nT), rng.uniform(0, 300, nP)
        tf, zf = rng.uniform(-50, 50, nT), rng.uniform(-50, 50, nP)
        tracks = [dict(rx=int(rng.integers(0, 2)), delay=td[i], doppler=tf[i], hits=int(rng.integers(1, 5)), misses=int(rng.integers(0, 3)),
                       flags=int(rng.integers(0, 2)), p_dd=float(rng.uniform(0.5, 4)), p_df=float(rng.uniform(-0.5, 0.5)), p_ff=float(rng.uniform(0.5, 9))) for i in range(nT)]
        p = par(gate=9.21, sigma=(1.5, 2.5), q=0.3, delay_rate_per_hz=-0.02, doppler_period=100.0)
    rx = np.sort(rng.integers(0, 2, nP))
    return frame(p, tracks, [(int(rx[j]), float(zd[j]), float(zf[j])) for j in range(nP)], T=0.7)


CASES = {
    "empty_empty": lambda: frame(par(), [], []),
    "no_tracks": lambda: frame(par(), [], [(0, 1.0, 2.0), (0, 3.0, 4.0), (2, 5.0, 6.0)]),
    "no_plots": lambda: frame(par(), [dict(delay=1.0), dict(delay=2.0, rx=1, flags=CONFIRMED, hits=4), dict(delay=3.0, misses=0)], []),
    "gate_on": lambda: c_gate(False),
    "gate_above": lambda: c_gate(True),
    "tie_two_tracks": lambda: frame(par(), [dict(delay=-1.0, **EXACT), dict(delay=1.0, **EXACT)], line([0.0])),
    "tie_two_plots": lambda: frame(par(), [dict(delay=0.0, **EXACT)], line([1.0, -1.0])),
    "abc": c_abc,
    "chain70": lambda: c_chain(70),
    "pairs257": lambda: c_pairs(257),
    "pairs1025": lambda: c_pairs(1025),
    "truncate19_k1": lambda: c_truncate(19, 1),
    "truncate19_k16": lambda: c_truncate(19, 16),
    "truncate130_k1": lambda: c_truncate(130, 1),
    "truncate130_k16": lambda: c_truncate(130, 16),
    "wrap_k0": lambda: c_wrap(0.0, 1000.0),
    "wrap_k": lambda: c_wrap(-0.01, 1000.0),
    "nowrap_k0": lambda: c_wrap(0.0, 0.0),
    "nowrap_k": lambda: c_wrap(-0.01, 0.0),
    "receivers": c_receivers,
    "nonfinite": c_nonfinite,
    "lifecycle": c_lifecycle,
    "full4": lambda: c_full(4, 1000.0),          # three survivors, room for one of the three new tracks
    "full5": lambda: c_full(5, 1000.0),
    "full4_survivors": lambda: c_full(4, 100.0),  # the survivors fill the table: no new track is stored, no id consumed
    "random_grid": lambda: c_random(1, True),
    "random_continuous": lambda: c_random(2, False),
}


@functools.lru_cache(maxsize=None)
def case(name):
    return CASES[name]()


@functools.lru_cache(maxsize=None)
def expected(name):
    """the restatement's answer for a case: computed once, shared by the tests, never modified"""
    c = case(name)
    rec, total, nid = step(c["par"], c["tracks"], c["next_id"], c["T"], c["plots"])
    rec.setflags(write=False)
    return rec, total, nid


# ----------------------------------------------------------------------------- the sequence
BIN = 5.0e-9                       # s per delay bin
SEQ_T, SEQ_FRAMES, SEQ_CARRIER, SEQ_PERIOD = 0.05, 40, 1.0e9, 1000.0
SEQ_PAR = par(gate=9.21, sigma=(0.5 * BIN, 2.0), q=1.0, delay_rate_per_hz=-1.0 / SEQ_CARRIER, doppler_period=SEQ_PERIOD, confirm_hits=3, max_misses=3, tentative_misses=0)
# (delay bin at frame 0, Doppler in Hz): the last two fly five bins apart at the same Doppler; target -> the frames it is not detected in
SEQ_TARGETS = [(400.0, 200.0), (900.0, -320.0), (1500.0, 60.0), (1505.0, 60.0)]
SEQ_MISSED = {0: (10, 11), 1: (20,), 2: (30, 31, 32), 3: (5, 17)}
SEQ_FALSE, SEQ_BINS = 5, 2000


def truth(k, frame_index):
    """target k at a frame: (delay in s, Doppler in Hz) -- a closing target (positive Doppler) comes nearer"""
    b, f = SEQ_TARGETS[k]
    return b * BIN - f / SEQ_CARRIER * (SEQ_T * frame_index), f


@functools.lru_cache(maxsize=None)
def sequence(seed):
    """per frame the PLOT array: detected targets with Gaussian noise of 0.3 bin and 1 Hz, five uniform false plots, shuffled"""
    rng = np.random.default_rng(seed)
    frames = []
    for n in range(SEQ_FRAMES):
        rows = []
        for k in range(len(SEQ_TARGETS)):
            d, f = truth(k, n)
            nd, nf = rng.normal(0.0, 0.3 * BIN), rng.normal(0.0, 1.0)
            if n not in SEQ_MISSED[k]:
                rows.append((0, d + nd, wrap(f + nf, SEQ_PERIOD), 10.0 + k))
        for _ in range(SEQ_FALSE):
            rows.append((0, rng.uniform(0.0, SEQ_BINS) * BIN, rng.uniform(-0.5, 0.5) * SEQ_PERIOD, 1.0))
        order = rng.permutation(len(rows))
        frames.append(make_plots([rows[i] for i in order]))
    return frames


def is_target(t, frame_index):
    """the track's state lies within 2 bins and 8 Hz of a target's truth: the target's number, else None"""
    for k in range(len(SEQ_TARGETS)):
        d, f = truth(k, frame_index)
        if abs(float(t["delay"]) - d) <= 2.0 * BIN and abs(wrap(float(t["doppler"]) - f, SEQ_PERIOD)) <= 8.0:
            return k
    return None


def check_sequence(tables):
    """the expected outcome, a condition: tables[n] is the table after frame n"""
    ids = None
    for n, t in enumerate(tables):
        conf = t[(t["flags"] & CONFIRMED) != 0]
        if n < SEQ_PAR["confirm_hits"] - 1:
            assert len(conf) == 0, n
            continue
        assert len(conf) == len(SEQ_TARGETS), (n, len(conf))
        who = [is_target(c, n) for c in conf]
        assert sorted(who) == list(range(len(SEQ_TARGETS))), (n, who)
        now = {k: int(c["id"]) for k, c in zip(who, conf)}
        assert ids is None or ids == now, (n, ids, now)
        ids = now
