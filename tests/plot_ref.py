"""An independent restatement of plot extraction (include/rts_amd.h: RtsPlotParams, RtsPlot) and the cases the host and the GPU tests
share.  Nothing here is the library's algorithm: the components come from a flood fill on a DENSE mask built from the list (the
library unites neighbours found by binary search in the sparse list), and the sums are written out from the rule -- members in
ascending list index, left to right from 0 inside blocks of 64, the block sums left to right from 0, every product rounded before it
is added (numpy's float64 arithmetic does not contract).

    plots(det, n_rx, nd, nb, link, min_cells, pri, t0, dt) -> PLOT array in ascending first_index
    CASES: name -> (n_rx, nd, nb, cells, link, min_cells); case_list(name) -> the DETECTION array of its cells, in flat order"""
import os
import zlib
from collections import deque

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DETECTION = np.dtype([("rx", "<u4"), ("doppler_bin", "<u4"), ("range_bin", "<u4"), ("n_train", "<u4"), ("power", "<f8"), ("noise", "<f8"),
                      ("threshold", "<f8"), ("range_offset", "<f8"), ("doppler_offset", "<f8"), ("delay", "<f8"), ("doppler", "<f8")])
PLOT = np.dtype([("rx", "<u4"), ("n_cells", "<u4"), ("first_index", "<u4"), ("peak_index", "<u4"), ("range_min", "<u4"), ("range_max", "<u4"),
                 ("doppler_lo", "<u4"), ("doppler_span", "<u4"), ("power_sum", "<f8"), ("peak_power", "<f8"), ("noise_sum", "<f8"),
                 ("range_centroid", "<f8"), ("doppler_centroid", "<f8"), ("range_spread", "<f8"), ("doppler_spread", "<f8"), ("delay", "<f8"),
                 ("doppler", "<f8")])
assert DETECTION.itemsize == 72 and PLOT.itemsize == 104
BLOCK = 64
T0, DT, PRI = 2.0e-6, 5.0e-9, 1.0e-3


# ----------------------------------------------------------------------------- the restatement
def components(det, n_rx, nd, nb, link):
    """the connected components by flood fill: a list of ascending member-index lists, in ascending first member"""
    lr, ld = link
    n = len(det)
    where = np.full(n_rx * nd * nb, -1, np.int64)
    rx = det["rx"].astype(np.int64); kk = det["doppler_bin"].astype(np.int64); rr = det["range_bin"].astype(np.int64)
    where[(rx * nd + kk) * nb + rr] = np.arange(n)
    where = where.tolist(); rx = rx.tolist(); kk = kk.tolist(); rr = rr.tolist()
    offsets = [(dk, dr) for dk in range(-ld, ld + 1) for dr in range(-lr, lr + 1)]
    seen = [False] * n
    out = []
    for i in range(n):
        if seen[i]:
            continue
        seen[i] = True
        members, todo = [i], deque([i])
        while todo:
            a = todo.popleft()
            for dk, dr in offsets:
                r = rr[a] + dr
                if r < 0 or r >= nb:
                    continue
                k = (kk[a] + dk) % nd
                if k == kk[a] and r == rr[a]:                      # the same cell (also through the wrap of a short map)
                    continue
                b = where[(rx[a] * nd + k) * nb + r]
                if b >= 0 and not seen[b]:
                    seen[b] = True; members.append(b); todo.append(b)
        out.append(sorted(members))
    return out


def blocked_sum(x):
    """the sum of x in the rule's order"""
    x = np.asarray(x, np.float64)
    nblk = (len(x) + BLOCK - 1) // BLOCK
    pad = np.zeros(nblk * BLOCK); pad[:len(x)] = x                  # (adding +0.0 to a sum that began at +0.0 changes nothing)
    pad = pad.reshape(nblk, BLOCK)
    acc = np.zeros(nblk)
    for j in range(BLOCK):
        acc = acc + pad[:, j]
    total = np.float64(0.0)
    for b in acc:
        total = total + b
    return total


def wrap_w(w, nd):
    half = np.float64(0.5) * np.float64(nd)
    if w >= half:
        w = w - np.float64(nd)
    elif w < -half:
        w = w + np.float64(nd)
    return w


def plots(det, n_rx, nd, nb, link=(1, 1), min_cells=1, pri=0.0, t0=0.0, dt=1.0):
    det = np.asarray(det, DETECTION)
    out = []
    f = np.float64
    for mem in components(det, n_rx, nd, nb, link):
        if len(mem) < max(1, min_cells):
            continue
        m = det[mem]; root = det[mem[0]]
        k0, r0 = int(root["doppler_bin"]), int(root["range_bin"])
        dri = m["range_bin"].astype(np.int64) - r0
        dki = m["doppler_bin"].astype(np.int64) - k0
        dki = np.where(2 * dki >= nd, dki - nd, np.where(2 * dki < -nd, dki + nd, dki))
        P = m["power"]; dr = dri.astype(np.float64); dk = dki.astype(np.float64)
        S, Sr, Sk = blocked_sum(P), blocked_sum(P * dr), blocked_sum(P * dk)
        Srr, Skk, N = blocked_sum(P * (dr * dr)), blocked_sum(P * (dk * dk)), blocked_sum(m["noise"])
        p = np.zeros((), PLOT)
        p["rx"], p["n_cells"], p["first_index"] = root["rx"], len(mem), mem[0]
        best = 0
        for j in range(1, len(mem)):
            if P[j] > P[best]:
                best = j
        p["peak_index"], p["peak_power"] = mem[best], P[best]
        p["range_min"], p["range_max"] = m["range_bin"].min(), m["range_bin"].max()
        p["doppler_lo"] = (k0 + int(dki.min())) % nd
        p["doppler_span"] = min(nd, int(dki.max()) - int(dki.min()) + 1)
        p["power_sum"], p["noise_sum"] = S, N
        sr = sk = f(0.0)
        if len(mem) == 1:
            rc = f(r0) + root["range_offset"]; w = f(k0) + root["doppler_offset"]
        elif not S > 0.0:
            rc, w = f(r0), f(k0)
        else:
            mr, mk = Sr / S, Sk / S
            rc, w = f(r0) + mr, f(k0) + mk
            sr = np.sqrt(max(f(0.0), Srr / S - mr * mr)); sk = np.sqrt(max(f(0.0), Skk / S - mk * mk))
        w = wrap_w(w, nd)
        p["range_centroid"], p["doppler_centroid"], p["range_spread"], p["doppler_spread"] = rc, w, sr, sk
        p["delay"] = f(t0) + rc * f(dt)
        p["doppler"] = w / (f(nd) * f(pri)) if pri > 0.0 else 0.0
        out.append(p)
    return np.array(out, PLOT) if out else np.zeros(0, PLOT)


# ----------------------------------------------------------------------------- lists
def make_list(cells, nd, nb, seed=1, t0=T0, dt=DT, pri=PRI, decades=12.0):
    """the DETECTION list of cells [(rx, k, r)] in flat order: powers over `decades` decades, refinements in [-0.5, 0.5], delay and
    doppler by RtsDetection's expressions"""
    cells = sorted(set((int(a), int(b), int(c)) for a, b, c in cells))
    rng = np.random.default_rng(seed)
    d = np.zeros(len(cells), DETECTION)
    if not cells:
        return d
    c = np.array(cells, np.int64).reshape(-1, 3)
    d["rx"], d["doppler_bin"], d["range_bin"] = c[:, 0], c[:, 1], c[:, 2]
    d["n_train"] = 248
    d["power"] = 10.0 ** rng.uniform(-decades / 2, decades / 2, len(d))
    d["noise"] = rng.uniform(0.5, 1.5, len(d))
    d["threshold"] = 10.0 * d["noise"]
    d["range_offset"] = rng.uniform(-0.5, 0.5, len(d)); d["doppler_offset"] = rng.uniform(-0.5, 0.5, len(d))
    d["delay"] = t0 + (d["range_bin"].astype(np.float64) + d["range_offset"]) * dt
    w = d["doppler_bin"].astype(np.float64) + d["doppler_offset"]
    w = np.where(w >= 0.5 * nd, w - nd, np.where(w < -0.5 * nd, w + nd, w))
    d["doppler"] = w / (np.float64(nd) * pri)
    return d


def mask_cells(mask, k_off=0):
    """[(rx, k + k_off, r)] of a boolean mask [n_rx][nd][nb]"""
    m = np.asarray(mask)
    if m.ndim == 2:
        m = m[None]
    return [(int(a), int(b) + k_off, int(c)) for a, b, c in zip(*np.nonzero(m))]


def shape_u():
    g = np.zeros((16, 16), bool)
    g[2:13, 3] = True; g[2:13, 10] = True; g[12, 3:11] = True       # the arms meet in the last row
    return g


def shape_spiral(n=16):
    g = np.zeros((n, n), bool)
    k = r = 0; dk, dr = 0, 1
    g[0, 0] = True
    while True:
        moved = False
        for _ in range(2):
            nk, nr, fk, fr = k + dk, r + dr, k + 2 * dk, r + 2 * dr
            if 0 <= nk < n and 0 <= nr < n and not g[nk, nr] and not (0 <= fk < n and 0 <= fr < n and g[fk, fr]):
                k, r = nk, nr; g[k, r] = True; moved = True
                break
            dk, dr = dr, -dk
        if not moved:
            return g


def shape_snake(n=32):
    g = np.zeros((n, n), bool)
    for k in range(n):
        if k % 2 == 0:
            g[k, :] = True
        else:
            g[k, n - 1 if (k // 2) % 2 == 0 else 0] = True
    return g


def shape_comb():
    g = np.zeros((11, 32), bool)
    g[0:10, 0:32:2] = True; g[10, :] = True                          # the teeth come first in flat order, the spine last
    return g


def random_mask(n_rx, nd, nb, density, seed):
    return np.random.default_rng(seed).random((n_rx, nd, nb)) < density


def _row(n):
    return [(0, 1, r) for r in range(n)]


_checker = [(0, k, r) for k in range(8) for r in range(8) if (k + r) % 2 == 0]
_short = [(0, k, r) for k, r in [(0, 0), (0, 1), (0, 2), (0, 5), (0, 7), (0, 8), (0, 12)]]
_short2 = _short + [(0, 1, r) for r in (3, 5, 10, 14, 15)]
# name -> (n_rx, nd, nb, cells, link, min_cells)
CASES = {
    "empty": (1, 4, 4, [], (1, 1), 1),
    "one": (1, 4, 4, [(0, 2, 3)], (1, 1), 1),
    "row63": (1, 4, 63, _row(63), (1, 1), 1),
    "row64": (1, 4, 64, _row(64), (1, 1), 1),
    "row65": (1, 4, 65, _row(65), (1, 1), 1),
    "row4097": (1, 4, 4097, _row(4097), (1, 1), 1),
    "dense65536": (1, 256, 256, mask_cells(np.ones((256, 256), bool)), (1, 1), 1),
    "wrap": (1, 8, 16, [(0, 7, 5), (0, 0, 5), (0, 0, 6), (0, 3, 9)], (1, 1), 1),
    "range_edges": (1, 8, 16, [(0, 2, 0), (0, 2, 15)], (4, 4), 1),
    "rx_boundary": (2, 8, 16, [(0, 7, 15), (1, 0, 0)], (4, 4), 1),
    "nd1_ld1": (1, 1, 16, _short, (1, 1), 1),
    "nd2_ld1": (1, 2, 16, _short2, (1, 1), 1),
    "nd2_ld4": (1, 2, 16, _short2, (1, 4), 1),
    "u": (1, 20, 16, mask_cells(shape_u(), 2), (1, 1), 1),
    "spiral": (1, 20, 16, mask_cells(shape_spiral(), 2), (1, 1), 1),
    "snake": (1, 36, 32, mask_cells(shape_snake(), 2), (1, 1), 1),
    "comb": (1, 16, 32, mask_cells(shape_comb(), 2), (1, 1), 1),
    "checker_11": (1, 8, 8, _checker, (1, 1), 1),
    "checker_10": (1, 8, 8, _checker, (1, 0), 1),
    "checker_01": (1, 8, 8, _checker, (0, 1), 1),
    "checker_00": (1, 8, 8, _checker, (0, 0), 1),
    "two_apart_20": (1, 8, 8, [(0, 3, 2), (0, 3, 4)], (2, 0), 1),
    "two_apart_14": (1, 8, 8, [(0, 3, 2), (0, 3, 4)], (1, 4), 1),
    "link44": (1, 16, 64, mask_cells(random_mask(1, 16, 64, 0.05, 5)), (4, 4), 1),
    "min1": (2, 16, 64, mask_cells(random_mask(2, 16, 64, 0.2, 9)), (1, 1), 1),
    "min2": (2, 16, 64, mask_cells(random_mask(2, 16, 64, 0.2, 9)), (1, 1), 2),
    "min5": (2, 16, 64, mask_cells(random_mask(2, 16, 64, 0.2, 9)), (1, 1), 5),
}
for _d in (0.05, 0.3, 0.6):
    for _s in (1, 2, 3):
        CASES["random_%g_%d" % (_d, _s)] = (2, 16, 64, mask_cells(random_mask(2, 16, 64, _d, 100 * _s + int(100 * _d))), (1, 1), 1)
# what the shapes are for: the number of plots each must give
EXPECT_PLOTS = {"empty": 0, "one": 1, "row63": 1, "row64": 1, "row65": 1, "row4097": 1, "dense65536": 1, "wrap": 2, "range_edges": 2, "rx_boundary": 2,
                "nd1_ld1": 4, "u": 1, "spiral": 1, "snake": 1, "comb": 1, "checker_11": 1, "checker_10": 32, "checker_01": 32, "checker_00": 32,
                "two_apart_20": 1, "two_apart_14": 2}


def case_list(name):
    n_rx, nd, nb, cells, link, min_cells = CASES[name]
    return make_list(cells, nd, nb, seed=zlib.crc32(np.array(cells, np.int64).tobytes()))      # (cases on the same cells share the list)


def same_bytes(a, b):
    """every field of every record, as bits"""
    assert len(a) == len(b), (len(a), len(b))
    for f in PLOT.names:
        assert np.ascontiguousarray(a[f]).tobytes() == np.ascontiguousarray(b[f]).tobytes(), (f, a[f][:8], b[f][:8])
