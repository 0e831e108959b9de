"""An independent restatement of track-before-detect by dynamic programming (include/rts_amd.h: RtsTbdParams, RtsTbdExtractParams,
RtsTbdTrack) in numpy, and the cases the host and the GPU tests share.  Nothing here is the library's code: the shift table, the
score, the recursion, the candidate rule and the walk are written out again from the header text -- the recursion as whole-array
gathers, one per window offset in ascending (dd, dr), the local maximum as shifted comparisons, the walk as a Python loop.

    shifts(nd, k, pri, T, dt) -> (int32 table, the quotients)
    step(map, merit_in, T, par, dt) -> (merit, pointers uint8, shifts int32)
    extract(merit, ptrs, shifts, threshold, par, local_max, max_tracks, pri, t0, dt) -> (TBD records, paths, total)
    CASES: name -> a function returning dict(maps, times, par, dt, t0, threshold, local_max, max_tracks);  case(name), run(name) cached
    weak_target(seed) -> the weak-target scene and its truth"""
import functools
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TBD = np.dtype([("rx", "<u4"), ("doppler_bin", "<u4"), ("range_bin", "<u4"), ("n_cells", "<u4"), ("first_doppler_bin", "<u4"),
                ("first_range_bin", "<u4"), ("merit", "<f8"), ("delay", "<f8"), ("doppler", "<f8")])
assert TBD.itemsize == 48
NONE, ABSENT = 0xff, 0xffffffff
TILE = 1024                      # RTS_TBD_TILE (tests/test_tbd_host.py reads it out of rts_tbd.h and compares)
MAX_TRACKS = 65536
PAR = dict(half=(1, 2), depth=8, score="power", scale=1.0, decay=1.0, delay_rate_per_hz=0.0, pri=0.0)


def par(**kw):
    p = dict(PAR); p.update(kw)
    return p


# ----------------------------------------------------------------------------- the restatement
def signed_bin(nd):
    kd = np.arange(nd, dtype=np.float64)
    return np.where(kd >= 0.5 * nd, kd - nd, kd)


def hertz(nd, pri):
    return signed_bin(nd) / (float(nd) * pri) if pri > 0.0 else np.zeros(nd)


def shifts(nd, k, pri, T, dt):
    with np.errstate(all="ignore"):
        q = ((k * hertz(nd, pri)) * T) / dt
    ok = np.isfinite(q) & (np.abs(q) <= 2.0 ** 30)
    return np.rint(np.where(ok, q, 0.0)).astype(np.int32), q


def score(z, mode, scale):
    with np.errstate(all="ignore"):
        x = (z.real * z.real + z.imag * z.imag) * scale
        if mode == "amplitude":
            x = np.sqrt(x)
    return np.where(np.isfinite(x), x, 0.0)


def step(z, merit_in, T, p, dt=1.0):
    z = np.asarray(z, np.complex128)
    n_rx, nd, nb = z.shape
    Hd, Hr = p["half"]
    x = score(z, p["score"], p["scale"])
    if merit_in is None:
        return x, np.full(z.shape, NONE, np.uint8), np.zeros(nd, np.int32)
    s, _ = shifts(nd, p["delay_rate_per_hz"], p["pri"], T, dt)
    best = np.zeros(z.shape); code = np.full(z.shape, NONE, np.uint8)
    kd = np.arange(nd); r = np.arange(nb, dtype=np.int64)
    for dd in range(-Hd, Hd + 1):
        rows = (kd + dd) % nd
        for dr in range(-Hr, Hr + 1):
            idx = r[None, :] - s.astype(np.int64)[:, None] + dr                          # [nd][nb]: the predecessor's range bin
            there = (idx >= 0) & (idx < nb)
            v = np.where(there[None], merit_in[:, rows[:, None], np.clip(idx, 0, nb - 1)], 0.0)
            better = v > best
            best = np.where(better, v, best)
            code = np.where(better, np.uint8((dd + Hd) * (2 * Hr + 1) + (dr + Hr)), code)
    return x + p["decay"] * best, code, s


def local_maxima(m):
    """[n_rx][nd][nb] bool: strictly greater than the 3 x 3 neighbours before the cell in flat order, >= those after; Doppler wraps
    (as it stands, also on one and two rows), range is truncated"""
    peak = np.ones(m.shape, bool)
    nb = m.shape[2]
    for dk in (-1, 0, 1):
        for dr in (-1, 0, 1):
            if dk == 0 and dr == 0:
                continue
            q = np.roll(m, -dk, axis=1)                                                  # q[:, k] = m[:, (k + dk) % nd]
            nbr = np.full(m.shape, -np.inf); exists = np.zeros(m.shape, bool)
            if dr < 0:
                nbr[:, :, 1:] = q[:, :, :-1]; exists[:, :, 1:] = True
            elif dr > 0:
                nbr[:, :, :-1] = q[:, :, 1:]; exists[:, :, :nb - 1] = True
            else:
                nbr = q; exists[:] = True
            before = dk < 0 or (dk == 0 and dr < 0)
            peak &= ~exists | ((m > nbr) if before else (m >= nbr))
    return peak


def walk(ptrs, shift_tables, rx, kd, r, p, nd, nb):
    """the cells from the end cell back, newest first; ptrs and shift_tables oldest first"""
    Hd, Hr = p["half"]
    W = 2 * Hr + 1
    n_frames = len(ptrs)
    cells = []
    for j in range(min(n_frames, p["depth"])):
        cells.append((kd, r))
        if j + 1 == min(n_frames, p["depth"]):
            break
        c = int(ptrs[n_frames - 1 - j][rx, kd, r])
        if c >= (2 * Hd + 1) * W:
            break
        dd, dr = c // W - Hd, c % W - Hr
        rp = r - int(shift_tables[n_frames - 1 - j][kd]) + dr
        if rp < 0 or rp >= nb:
            break
        kd, r = (kd + dd) % nd, rp
    return cells


def extract(merit, ptrs, shift_tables, threshold, p, local_max=True, max_tracks=0, pri=0.0, t0=0.0, dt=1.0):
    n_rx, nd, nb = merit.shape
    cand = merit > threshold
    if local_max:
        cand &= local_maxima(merit)
    where = np.argwhere(cand)                                                            # C order: ascending flat (rx, kd, r)
    total = len(where)
    n = min(total, max_tracks or MAX_TRACKS)
    rec = np.zeros(n, TBD); paths = np.full((n, p["depth"], 2), ABSENT, np.uint32)
    hz = hertz(nd, pri)
    for i, (rx, kd, r) in enumerate(where[:n]):
        cells = walk(ptrs, shift_tables, int(rx), int(kd), int(r), p, nd, nb)
        paths[i, :len(cells)] = cells
        rec[i] = (rx, kd, r, len(cells), cells[-1][0], cells[-1][1], merit[rx, kd, r], t0 + float(r) * dt, hz[kd])
    return rec, paths, total


def same_bytes(got, want):
    assert got.dtype == want.dtype and got.shape == want.shape, (got.dtype, got.shape, want.dtype, want.shape)
    a, b = np.frombuffer(got.tobytes(), np.uint8), np.frombuffer(want.tobytes(), np.uint8)
    if not np.array_equal(a, b):
        i = int(np.argmax(a != b)) // got.dtype.itemsize
        raise AssertionError("bytes differ, first at element %d: got %s, want %s" % (i, got.reshape(-1)[i], want.reshape(-1)[i]))


# ----------------------------------------------------------------------------- the cases
def noise(rng, shape):
    return (rng.standard_normal(shape) + 1j * rng.standard_normal(shape)) / np.sqrt(2.0)


def _frames(seed, shape, n, gen=noise):
    rng = np.random.default_rng(seed)
    return [gen(rng, shape) for _ in range(n)]


def _ints(rng, shape):
    return rng.integers(0, 3, shape).astype(np.float64) + 0j                            # powers 0, 1, 4: full of ties


def _case(maps, times, p, quantile=0.98, dt=1.0, t0=0.0, local_max=True, max_tracks=0):
    return dict(maps=maps, times=times, par=p, dt=dt, t0=t0, quantile=quantile, local_max=local_max, max_tracks=max_tracks)


def _nonfinite():
    maps = _frames(7, (2, 6, 70), 4)
    maps[1][0, 2, 10] = np.nan; maps[1][1, 5, 69] = np.inf; maps[2][0, 0, 0] = complex(np.nan, 1.0); maps[3][1, 3, 35] = 1e200 + 1e200j
    return _case(maps, [0.0, 1.0, 2.5, 3.0], par(score="amplitude", decay=0.5, depth=3, delay_rate_per_hz=1.5, pri=1.0 / 6.0))


CASES = {
    # n_bins = tile + 1: the second tile holds one bin; shifts of a few bins both ways
    "tile_plus_1": lambda: _case(_frames(1, (1, 4, TILE + 1), 3), [0.0, 1.0, 2.0], par(delay_rate_per_hz=2.0, pri=0.25)),
    # n_bins = 2 tile - 1, n_doppler = 2 Hd + 1, shifts of +-(tile + 3) pull the predecessors across the tile border
    "two_tiles_minus_1": lambda: _case(_frames(2, (1, 3, 2 * TILE - 1), 3), [0.0, 1.0, 2.0], par(delay_rate_per_hz=float(TILE + 3), pri=1.0 / 3.0)),
    # n_bins no multiple of 64, three receivers with a map each, more frames than the ring holds, a different T per frame
    "three_receivers": lambda: _case(_frames(3, (3, 8, 200), 7), [0.0, 1.0, 3.0, 3.5, 5.5, 6.5, 9.5], par(depth=4, delay_rate_per_hz=1.0, pri=0.125)),
    # the widest window on the fewest rows it fits
    "wide_window": lambda: _case(_frames(4, (2, 7, 70), 3), [0.0, 1.0, 2.0], par(half=(3, 15), depth=2, delay_rate_per_hz=-3.0, pri=1.0 / 7.0), quantile=0.9),
    # no window at all: the predecessor is the displaced cell alone
    "no_window": lambda: _case(_frames(5, (1, 5, 65), 3), [0.0, 1.0, 2.0], par(half=(0, 0), delay_rate_per_hz=1.0, pri=0.2)),
    # integer maps: every window is full of ties, the first maximum in ascending (dd, dr) decides
    "ties": lambda: _case(_frames(6, (2, 6, 130), 4, _ints), [0.0, 1.0, 2.0, 3.0], par(delay_rate_per_hz=1.0, pri=1.0 / 6.0), quantile=0.5),
    # amplitude score, decay 0.5, cells that are not finite
    "nonfinite": _nonfinite,
    # one Doppler row: no local maximum exists by the rule, so without it
    "one_row": lambda: _case(_frames(8, (2, 1, 97), 3), [0.0, 1.0, 2.0], par(half=(0, 3)), local_max=False, quantile=0.95),
    # depth 1: only the newest pointer map is kept and a path is one cell
    "depth_1": lambda: _case(_frames(9, (1, 4, 64), 3), [0.0, 1.0, 2.0], par(depth=1)),
    # max_tracks cuts the list: the stored prefix and the total
    "full_list": lambda: _case(_frames(10, (1, 8, 128), 3), [0.0, 1.0, 2.0], par(), quantile=0.5, local_max=False, max_tracks=10),
}


@functools.lru_cache(maxsize=None)
def case(name):
    return weak_case() if name == "weak_target" else CASES[name]()


ALL = list(CASES) + ["weak_target"]


@functools.lru_cache(maxsize=None)
def run(name):
    """the restatement on the case: dict(merits, ptrs, shifts: per frame; threshold; ring: the stored (ptrs, shifts) oldest first;
    rec, paths, total)"""
    c = case(name)
    p = c["par"]
    merit, merits, ptrs, tabs = None, [], [], []
    for n, z in enumerate(c["maps"]):
        merit, code, s = step(z, merit, c["times"][n] - c["times"][n - 1] if n else 0.0, p, c["dt"])
        merits.append(merit); ptrs.append(code); tabs.append(s)
    keep = min(len(ptrs), p["depth"])
    threshold = float(np.quantile(merit, c["quantile"]))
    rec, paths, total = extract(merit, ptrs[-keep:], tabs[-keep:], threshold, p, c["local_max"], c["max_tracks"], p["pri"], c["t0"], c["dt"])
    for a in merits + ptrs + tabs + [rec, paths]:
        a.setflags(write=False)
    return dict(merits=merits, ptrs=ptrs, shifts=tabs, threshold=threshold, ring=(np.stack(ptrs[-keep:]), np.stack(tabs[-keep:])), rec=rec, paths=paths, total=total)


# ----------------------------------------------------------------------------- the weak target
WEAK_SEED = 0
WEAK_ROW, WEAK_SHIFT, WEAK_START, WEAK_POWER, WEAK_FRAMES, CFAR_LEVEL = 5, -3, 100, 6.0, 8, 13.8


def weak_target(seed):
    """8 frames of unit-power noise, 32 x 256, and a steady target of power 6 on Doppler row 5 that moves by s[5] = -3 bins a frame
    (the predecessor of (5, r) is (5, r + 3)).  Returns (maps, the true cells oldest first)"""
    rng = np.random.default_rng(seed)
    maps, truth = [], []
    for n in range(WEAK_FRAMES):
        z = noise(rng, (1, 32, 256))
        r = WEAK_START + WEAK_SHIFT * n
        z[0, WEAK_ROW, r] += np.sqrt(WEAK_POWER)
        maps.append(z); truth.append((WEAK_ROW, r))
    return maps, truth


def weak_case(seed=WEAK_SEED):
    maps, _ = weak_target(seed)
    # nd pri = 1: f = w hertz, and s[5] = rint(-0.6 * 5) = -3
    return _case(maps, [float(n) for n in range(WEAK_FRAMES)], par(delay_rate_per_hz=-0.6, pri=1.0 / 32.0), quantile=0.999)


def weak_outcome(merit, rec, paths, maps, truth):
    """(the record of the largest merit is within the window of the true end cell, cells of its path on the truth, frames in which the
    target cell crosses the CFAR level)"""
    i = int(np.argmax(rec["merit"]))
    assert rec["merit"][i] == merit.max()
    end = truth[-1]
    near = abs(int(rec["doppler_bin"][i]) - end[0]) <= 1 and abs(int(rec["range_bin"][i]) - end[1]) <= 2
    on = sum(1 for j, cell in enumerate(reversed(truth)) if j < rec["n_cells"][i] and tuple(int(v) for v in paths[i, j]) == cell)
    crossed = sum(1 for z, (k, r) in zip(maps, truth) if abs(z[0, k, r]) ** 2 > CFAR_LEVEL)
    return near, on, crossed
