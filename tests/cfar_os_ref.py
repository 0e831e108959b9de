"""An independent numpy restatement of ordered-statistic CFAR, written from the text of include/rts_amd.h (RtsCfarOsParams), for
tests/test_cfar_os_host.py and tests/test_gpu_cfar_os.py: the training powers of every cell gathered with np.roll (+inf where the
range is truncated), sorted along the offset axis, element k - 1 taken per column; its own bisection for alpha; and the helpers of
tests/test_gpu_detect.py that the comparisons need, restated (they are helpers there, not importable fixtures)."""
import math

import numpy as np

# (G (r, d), T (r, d), rank or a function of N0, n_rx, n_doppler, n_bins, pfa, alpha, local max): the shapes of both test files.
# On the 3-row map of case 7 the noise estimate is the LARGEST cell of the two other rows within 16 bins, and planted_map's targets
# and their sloped neighbours sit in each other's windows there: it alone leaves one detection, short of the 5 per receiver that
# every comparison asks of its expectation.  That case therefore gets EXTRA_CELLS on top: five cells in one row (a cell's own row
# is guard when Gd = 0), strong enough to clear three times the plateau.
CASES = [
    ((2, 2), (8, 4), 186, 2, 64, 300, 1e-3, None, False),                  # several range tiles, ragged last tile
    ((1, 0), (3, 2), lambda n0: n0 // 2, 3, 8, 200, 1e-2, None, True),     # n_doppler below one tile
    ((0, 0), (16, 16), 816, 1, 33, 70, None, 6.0, False),                  # N0 = 1 088; the window wraps the whole Doppler axis exactly once
    ((0, 2), (16, 0), 120, 2, 24, 90, None, 5.0, False),                   # Td = 0
    ((0, 0), (0, 16), 24, 2, 1024, 70, 1e-4, None, True),                  # Tr = 0; many Doppler tiles
    ((4, 0), (2, 1), 1, 2, 12, 129, None, 4.0, True),                      # smallest rank; one bin past a tile
    ((16, 0), (0, 1), lambda n0: n0, 1, 3, 64, None, 3.0, False),          # largest rank; guard at its limit
    ((0, 0), (16, 1), lambda n0: (3 * n0) // 4, 3, 5, 17, 1e-2, None, False),   # n_bins = Gr + Tr + 1: every cell lies at both range edges
]


EXTRA_CELLS = {6: [(0, 8, 2.0), (0, 20, 2.2), (0, 32, 2.4), (0, 44, 2.6), (0, 56, 2.8)]}      # case index -> (k, r, amplitude / planted_map's)


def n0_of(guard, train):
    (gr, gd), (tr, td) = guard, train
    return (2 * (gr + tr) + 1) * (2 * (gd + td) + 1) - (2 * gr + 1) * (2 * gd + 1)


def case_rank(case):
    rank = case[2]
    return rank(n0_of(case[0], case[1])) if callable(rank) else rank


def law(n, k, alpha):
    """prod_{i<k} (N - i) / (N - i + alpha): the false-alarm rate of the k-th of N cells at threshold factor alpha"""
    out = 1.0
    for i in range(k):
        out *= (n - i) / (n - i + alpha)
    return out


def alpha_ref(n, k, pfa):
    """the root of law(n, k, alpha) = pfa by bisection (law falls as alpha rises)"""
    lo, hi = 0.0, 1.0
    while law(n, k, hi) > pfa:
        hi *= 2.0
    for _ in range(200):
        mid = 0.5 * (lo + hi)
        if law(n, k, mid) > pfa:
            lo = mid
        else:
            hi = mid
    return 0.5 * (lo + hi)


def os_ref(P, gr, gd, tr, td, rank, pfa=None, alpha=None, local_max=False):
    """every cell's (noise, threshold, n_train) and the detection mask"""
    n_rx, nd, nb = P.shape
    Or, Od = gr + tr, gd + td
    n0 = n0_of((gr, gd), (tr, td))
    r = np.arange(nb)
    stack = np.empty((n0,) + P.shape)
    n = np.zeros(nb, np.int64)
    j = 0
    for dk in range(-Od, Od + 1):
        rolled = np.roll(P, -dk, axis=1)                      # rolled[:, k] = P[:, (k + dk) mod nd]
        for dr in range(-Or, Or + 1):
            if abs(dk) <= gd and abs(dr) <= gr:
                continue
            ok = (r + dr >= 0) & (r + dr < nb)
            v = np.full(P.shape, np.inf)
            v[:, :, ok] = rolled[:, :, r[ok] + dr]
            stack[j] = v
            n += ok
            j += 1
    assert j == n0 and n.min() >= 1
    stack.sort(axis=0)
    k = (rank * n + n0 - 1) // n0                             # per range bin
    noise = np.take_along_axis(stack, np.broadcast_to((k - 1)[None, None, None, :], (1,) + P.shape), axis=0)[0]
    if pfa is not None:
        table = {int(m): alpha_ref(int(m), int((rank * int(m) + n0 - 1) // n0), pfa) for m in np.unique(n)}
        a = np.array([table[int(m)] for m in n])[None, None, :]
    else:
        a = alpha
    thr = a * noise
    det = P > thr
    if local_max:
        for dk in (-1, 0, 1):
            for dr in (-1, 0, 1):
                if dk == 0 and dr == 0:
                    continue
                q = np.roll(np.roll(P, -dk, axis=1), -dr, axis=2)
                below = dk < 0 or (dk == 0 and dr < 0)
                cmp = P > q if below else P >= q
                if dr == -1:
                    cmp[:, :, 0] = True                         # (range truncated: no neighbour)
                if dr == 1:
                    cmp[:, :, nb - 1] = True
                det &= cmp
    return noise, thr, np.broadcast_to(n[None, None, :], P.shape), det


def ca_ref(P, gr, gd, tr, td, pfa):
    """cell averaging at pfa, the expression of cfar_ref in tests/test_gpu_detect.py: (threshold, detection mask)"""
    nb = P.shape[2]
    Or, Od = gr + tr, gd + td
    S = np.zeros(P.shape); N = np.zeros(nb)
    r = np.arange(nb)
    for dk in range(-Od, Od + 1):
        rolled = np.roll(P, -dk, axis=1)
        for dr in range(-Or, Or + 1):
            if abs(dk) <= gd and abs(dr) <= gr:
                continue
            ok = (r + dr >= 0) & (r + dr < nb)
            S[:, :, ok] += rolled[:, :, r[ok] + dr]
            N += ok
    n = N[None, None, :]
    thr = n * np.expm1(-math.log(pfa) / n) * (S / n)
    return thr, P > thr


def delta_ref(pm, p0, pp):
    if pm is None or pp is None or pm <= 0 or p0 <= 0 or pp <= 0:
        return 0.0
    lm, l0, lp = math.log(pm), math.log(p0), math.log(pp)
    den = lm - 2 * l0 + lp
    if den >= 0:
        return 0.0
    return min(0.5, max(-0.5, 0.5 * (lm - lp) / den))


def detections_ref(P, noise, thr, n, det, t0, dt, pri):
    from rts_amd import _lib as L
    nd, nb = P.shape[1], P.shape[2]
    out = []
    for rx, k, r in zip(*np.nonzero(det)):                    # C order: ascending flat (rx, k, r)
        p0 = P[rx, k, r]
        d_r = delta_ref(P[rx, k, r - 1] if r >= 1 else None, p0, P[rx, k, r + 1] if r + 1 < nb else None)
        d_d = delta_ref(P[rx, (k - 1) % nd, r], p0, P[rx, (k + 1) % nd, r])
        w = k + d_d
        if w >= nd / 2:
            w -= nd
        elif w < -nd / 2:
            w += nd
        out.append((rx, k, r, int(n[rx, k, r]), p0, noise[rx, k, r], thr[rx, k, r], d_r, d_d, t0 + (r + d_r) * dt,
                    w / (nd * pri) if pri > 0 else 0.0))
    return np.array(out, dtype=L.DETECTION_DTYPE) if out else np.zeros(0, L.DETECTION_DTYPE)


def assert_margin(P, thr, rel=1e-9):
    """no cell sits within rel of its threshold: the decision cannot depend on rounding"""
    assert np.all(np.abs(P - thr) > rel * np.abs(thr)), "a cell lies on its threshold"


def assert_same_list(got, want, exact=("power", "noise"), threshold_rtol=0.0):
    """the comparison of tests/test_gpu_detect.py, with the fields an order statistic makes exact compared exactly: integer fields,
    `exact` and (threshold_rtol 0) the threshold bit for bit; the refinement fields to rtol / atol 1e-12 of their scale"""
    assert len(got) == len(want), (len(got), len(want))
    for f in ("rx", "doppler_bin", "range_bin", "n_train") + tuple(exact):
        assert np.array_equal(got[f], want[f]), f
    if threshold_rtol == 0.0:
        assert np.array_equal(got["threshold"], want["threshold"]), "threshold"
    else:
        np.testing.assert_allclose(got["threshold"], want["threshold"], rtol=threshold_rtol, atol=0, err_msg="threshold")
    for f in ("range_offset", "doppler_offset", "delay", "doppler"):
        scale = max(np.abs(want[f]).max(initial=0.0), 1e-300)
        np.testing.assert_allclose(got[f], want[f], rtol=1e-12, atol=1e-12 * scale if f != "delay" else 0, err_msg=f)


def planted_map(rng, n_rx, nd, nb, noise_power=1.0, snr=1e3):
    """exponential noise, targets with sloped neighbours at the Doppler wrap and the range edges, and a 2 x 2 plateau"""
    z = rng.standard_normal((n_rx, nd, nb)) + 1j * rng.standard_normal((n_rx, nd, nb))
    z *= math.sqrt(noise_power / 2)
    amp = math.sqrt(snr * noise_power)
    for rx in range(n_rx):
        for k, r in ((0, 0), (nd - 1, nb - 1), (0, nb - 1), (nd - 1, 0), (nd // 2, nb // 2 + 3)):
            z[rx, k, r] = amp * np.exp(1j * rng.uniform(0, 2 * np.pi))
            for dk, dr, f in ((0, -1, 0.6), (0, 1, 0.35), (-1, 0, 0.5), (1, 0, 0.3)):
                if 0 <= r + dr < nb:
                    z[rx, (k + dk) % nd, r + dr] = f * amp
        kp, rp = min(3, nd - 2), min(20, nb - 3)
        z[rx, kp:kp + 2, rp:rp + 2] = 0.8 * amp                # plateau of equal cells
    return z


_cache = {}


def case_expectation(index, t0=2.0e-6, dt=5.0e-9, pri=1.0e-3):
    """(z, P, want) of CASES[index], computed once and shared by the tests that need it (read-only)"""
    if index not in _cache:
        guard, train, _, n_rx, nd, nb, pfa, alpha, local_max = CASES[index]
        rank = case_rank(CASES[index])
        rng = np.random.default_rng(nd * 1000 + nb)
        z = planted_map(rng, n_rx, nd, nb)
        for k, r, f in EXTRA_CELLS.get(index, ()):
            z[:, k, r] = f * math.sqrt(1e3)
        P = z.real * z.real + z.imag * z.imag
        noise, thr, n, det = os_ref(P, guard[0], guard[1], train[0], train[1], rank, pfa, alpha, local_max)
        assert_margin(P, thr, 1e-9)
        want = detections_ref(P, noise, thr, n, det, t0, dt, pri)
        assert len(want) >= 5 * n_rx, (len(want), n_rx)
        for a in (z, P, want):
            a.setflags(write=False)
        _cache[index] = (z, P, want)
    return _cache[index]


def masking_map():
    """five 40 dB cells and a 16 dB cell four range bins from the first, in unit-power noise: (z, strong cells, weak cell) as (k, r)"""
    rng = np.random.default_rng(11)
    z = (rng.standard_normal((1, 32, 128)) + 1j * rng.standard_normal((1, 32, 128))) * math.sqrt(0.5)
    strong = [(10, 64), (11, 67), (9, 56), (12, 70), (8, 53)]
    for k, r in strong:
        z[0, k, r] = 100
    z[0, 10, 60] = math.sqrt(10 ** 1.6)
    return z, strong, (10, 60)
