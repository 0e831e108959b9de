"""A numpy restatement of the autofocus operations of include/rts_amd.h (RtsAlignParams, RtsPgaParams, RtsCorrectParams) in the
operation order the header specifies, and the scene generator of their end-to-end tests.  The alignment is restated operation by
operation (chunked and blocked sums, rounded products), so its shifts can be compared exactly; the PGA uses numpy.fft -- a
different transform tree on purpose -- and the correction the interpolator's restatement of tests/test_image_host.py."""
import numpy as np

from test_image_host import interp_ref

PULSE_CHUNK, BIN_BLOCK, PGA_TILE = 64, 64, 8


def gate_of(gate, nb):
    fb, G = (0, 0) if gate is None else gate
    return fb, (G if G else nb - fb)


# ----------------------------------------------------------------------------- alignment
def pick_ref(C, L, integer):
    """the shift of one row from its correlation C[l + L]"""
    best, bv = 0, C[L]
    if bv != bv:
        bv = -np.inf
    for m in range(1, L + 1):
        if C[L - m] > bv:
            bv, best = C[L - m], -m
        if C[L + m] > bv:
            bv, best = C[L + m], m
    delta = 0.0
    if not integer and abs(best) < L:
        cm, c0, cp = C[L + best - 1], C[L + best], C[L + best + 1]
        den = cm - 2.0 * c0 + cp
        if den < 0.0:
            d = 0.5 * (cm - cp) / den
            delta = -0.5 if d < -0.5 else 0.5 if d > 0.5 else d if d == d else 0.0
    return float(best) + delta


def align_ref(cube, first=0, count=None, gate=None, max_lag=8, n_iters=4, integer=False):
    """the range shifts float64 [n_rx][count]"""
    n_rx, n_p, nb = cube.shape
    P = n_p - first if count is None else count
    fb, G = gate_of(gate, nb)
    L = max_lag
    rows = cube[:, first:first + P]
    pad = L + 1
    ep = np.zeros((n_rx, P, nb + 2 * pad))
    ep[:, :, pad:pad + nb] = np.sqrt(rows.real * rows.real + rows.imag * rows.imag)
    S = np.zeros((n_rx, P))
    g = np.arange(G)
    for _ in range(n_iters):
        R = np.floor(S + 0.5).astype(np.int64)
        ref = None
        for j0 in range(0, P, PULSE_CHUNK):
            s = np.zeros((n_rx, G))
            for j in range(j0, min(P, j0 + PULSE_CHUNK)):
                for r in range(n_rx):
                    s[r] += ep[r, j, pad + fb + R[r, j] + g]
            ref = s if ref is None else ref + s
        C = np.zeros((n_rx, P, 2 * L + 1))
        for g0 in range(0, G, BIN_BLOCK):
            bs = np.zeros((n_rx, P, 2 * L + 1))
            for gg in range(g0, min(G, g0 + BIN_BLOCK)):
                lo = pad + fb + gg - L
                bs += ref[:, None, gg, None] * ep[:, :, lo:lo + 2 * L + 1]
            C += bs
        S = np.array([[pick_ref(C[r, j], L, integer) for j in range(P)] for r in range(n_rx)])
    return S


# ----------------------------------------------------------------------------- phase-gradient autofocus
def pga_ref(cube, first=0, count=None, gate=None, n_iters=6, window0=0, window_min=0):
    """(phase [n_rx][N] in cycles, rms [n_rx][n_iters], the least ratio of a column's largest |X[k]|^2 to its second largest over
    all iterations -- inf for all-zero columns)"""
    n_rx, n_p, nb = cube.shape
    N = n_p - first if count is None else count
    fb, G = gate_of(gate, nb)
    y = cube[:, first:first + N, fb:fb + G]
    phi = np.zeros((n_rx, N))
    rms = np.zeros((n_rx, n_iters))
    W = window0 if window0 else N // 2
    wmin = window_min if window_min else 8
    k = np.arange(N)
    keep = np.minimum(k, N - k) <= W // 2
    xp = k.astype(np.float64) - (N - 1) / 2.0
    margin = np.inf
    for it in range(n_iters):
        f = phi - np.floor(phi)
        x = y * np.exp(-2j * np.pi * f)[:, :, None]
        X = np.fft.fft(x, axis=1)
        pw = X.real * X.real + X.imag * X.imag
        ks = np.argmax(pw, axis=1)                                          # the first maximum
        top = np.sort(pw, axis=1)[:, -2:, :]
        with np.errstate(divide="ignore", invalid="ignore"):
            ratio = np.where(top[:, 1] > 0, top[:, 1] / top[:, 0], np.inf)
        margin = min(margin, float(ratio.min()))
        keep = np.minimum(k, N - k) <= W // 2
        idx = (k[None, :, None] + ks[:, None, :]) % N
        Y = np.take_along_axis(X, idx, axis=1) * keep[None, :, None]
        g = N * np.fft.ifft(Y, axis=1)
        a = np.zeros_like(g)
        a[:, 1:] = g[:, 1:] * np.conj(g[:, :-1])
        A = None
        for g0 in range(0, G, PGA_TILE):
            ts = np.zeros((n_rx, N), np.complex128)
            for gg in range(g0, min(G, g0 + PGA_TILE)):
                ts = ts + a[:, :, gg]
            A = ts if A is None else A + ts
        D = np.where((A.real == 0) & (A.imag == 0), 0.0, np.arctan2(A.imag, A.real) / (2 * np.pi))
        D[:, 0] = 0.0
        psi = np.cumsum(D, axis=1)
        mean = psi.sum(axis=1) / N
        slope = (xp * psi).sum(axis=1) / (xp * xp).sum()
        psi = psi - mean[:, None] - slope[:, None] * xp
        phi = phi + psi
        rms[:, it] = np.sqrt((psi * psi).sum(axis=1) / N)
        W = max(wmin, W // 2)
    return phi, rms, margin


# ----------------------------------------------------------------------------- correction
def correct_ref(cube, shifts=None, phase=None, first=0, count=None, taps=8):
    """a copy of the cube with rows first .. first + count - 1 resampled at n + shifts and rotated by -phase (cycles)"""
    out = np.array(cube, np.complex128, copy=True)
    n_rx, n_p, nb = out.shape
    P = n_p - first if count is None else count
    n = np.arange(nb, dtype=np.float64)
    for r in range(n_rx):
        for j in range(P):
            row = cube[r, first + j]
            v = row
            if shifts is not None:
                d = n + shifts[r][j]
                v = interp_ref(row.real, d, taps) + 1j * interp_ref(row.imag, d, taps)
            if phase is not None:
                f = phase[r][j] - np.floor(phase[r][j])
                v = v * np.exp(-2j * np.pi * f)
            out[r, first + j] = v
    return out


# ----------------------------------------------------------------------------- the end-to-end scenes
SCENES = [((64, 96), (5.0, 2.0)), ((128, 256), (6.0, 3.0))]      # ((N, n_bins), (w, q) bins of range walk w t + q t^2)


def scene(shape, walk, seed):
    """8 point scatterers behind an unknown motion: dict(raw=the cube [1][N][n_bins], walk=[N] bins, phase=[N] rad, ideal=the cube
    without walk and phase error).  Ranges uniform in [0.3, 0.7] n_bins, Doppler uniform in +-0.3 cycles per pulse, amplitudes
    uniform in [0.3, 1] with random phase (the first scatterer 3); a scatterer's range profile is sinc(d) times a raised cosine of
    half-width 3 bins; walk w t + q t^2 with t = (p - N / 2) / N; phase error 40 t^2 rad plus the running sum of N(0, 0.6^2) rad;
    complex white noise 20 dB below unit amplitude"""
    N, nb = shape
    w, q = walk
    rng = np.random.default_rng(seed)
    K = 8
    rg = rng.uniform(0.3, 0.7, K) * nb
    fd = rng.uniform(-0.3, 0.3, K)
    amp = rng.uniform(0.3, 1.0, K) * np.exp(2j * np.pi * rng.uniform(0, 1, K))
    amp[0] = 3.0 * amp[0] / abs(amp[0])
    p = np.arange(N)
    t = (p - N / 2) / N
    walk_bins = w * t + q * t * t
    phase = 40.0 * t * t + np.cumsum(rng.normal(0.0, 0.6, N))
    n = np.arange(nb, dtype=np.float64)

    def render(walk_p, phase_p):
        c = np.zeros((N, nb), np.complex128)
        for k in range(K):
            d = n[None, :] - (rg[k] + walk_p[:, None])
            prof = np.sinc(d) * np.where(np.abs(d) < 3.0, 0.5 + 0.5 * np.cos(np.pi * d / 3.0), 0.0)
            c += amp[k] * np.exp(2j * np.pi * fd[k] * p)[:, None] * prof
        return c * np.exp(1j * phase_p)[:, None]

    noise = 0.1 * (rng.standard_normal((N, nb)) + 1j * rng.standard_normal((N, nb))) / np.sqrt(2.0)
    raw = render(walk_bins, phase) + noise
    ideal = render(np.zeros(N), np.zeros(N)) + noise
    return dict(raw=raw[None], walk=walk_bins, phase=phase, ideal=ideal[None])


def contrast(cube):
    """std / mean of the Doppler-map power of a cube [n_rx][N][n_bins]"""
    pw = np.abs(np.fft.fft(cube, axis=1)) ** 2
    return float(pw.std() / pw.mean())


def detrended(v):
    """v less its constant and its least-squares line"""
    x = np.arange(len(v)) - (len(v) - 1) / 2.0
    v = v - v.mean()
    return v - x * (x * v).sum() / (x * x).sum()


def autofocus_metrics(sc, shifts, phase, focused, aligned):
    """(largest shift error after removing its mean [bins], residual phase rms after removing constant and line [rad], contrast of
    the focused cube over the aligned-only cube's, over the raw cube's)"""
    es = shifts[0] - sc["walk"]
    es = es - es.mean()
    res = detrended(2 * np.pi * phase[0] - sc["phase"])
    return float(np.abs(es).max()), float(np.sqrt((res * res).mean())), contrast(focused) / contrast(aligned), contrast(focused) / contrast(sc["raw"])


def autofocus_ref(raw, max_lag=8, align_iters=4, taps=8, n_iters=6, window_min=8):
    """the chain on the restatement: (shifts, phase, rms, the aligned cube, the focused cube)"""
    S = align_ref(raw, max_lag=max_lag, n_iters=align_iters)
    aligned = correct_ref(raw, shifts=S, taps=taps)
    phase, rms, _ = pga_ref(aligned, n_iters=n_iters, window_min=window_min)
    return S, phase, rms, aligned, correct_ref(aligned, phase=phase, taps=taps)
