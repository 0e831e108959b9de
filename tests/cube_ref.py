"""High-precision restatement of the return-cube operations, written from include/rts_amd.h alone (RtsCubeParams, RtsWaveform,
rts_cube_doppler): the impulse cube, the waveform render, range compression and the slow-time DFT.  Everything is accumulated
in np.longdouble with plain loops over contributions and output samples -- no tiles, no chunks, no precomputed weights -- so it
shares no structure with the kernels it checks.

A contribution is a tuple (rx, a, tau, f): receiver index, complex amplitude a = sqrt(P) e^{j phi} (np.clongdouble), delay tau
(float64) and Doppler frequency f (float64).  Its fractional start d = (tau - t0) / dt is formed in float64, the format in which
the header states it (tau, t0 and dt are doubles): an on-grid start is a property of THAT number, and sample-and-hold is
discontinuous there.  Everything after d is longdouble.
"""
import math

import numpy as np

LD = np.longdouble
CLD = np.clongdouble
PI = LD(4) * np.arctan(LD(1))


def cexp(x):
    """e^{j x} for a longdouble x"""
    x = LD(x)
    return CLD(np.cos(x)) + CLD(1j) * CLD(np.sin(x))


def start_of(tau, t0, dt):
    """d = (tau - t0) / dt in float64 (one subtraction, one division)"""
    return float((np.float64(tau) - np.float64(t0)) / np.float64(dt))


def h_L(u, L):
    """the interpolation kernel h_L at the longdouble points u (array): L = 1 sample-and-hold, 1 on -1 < u <= 0; L even the
    Blackman-windowed sinc on |u| < L/2 with h_L(0) = 1 and h_L = 0 at every other integer"""
    u = np.asarray(u, LD)
    if L == 1:
        return ((u > -1) & (u <= 0)).astype(LD)
    out = np.zeros(u.shape, LD)
    inside = (np.abs(u) < LD(L) / 2) & (u != np.rint(u))
    v = u[inside]
    w = LD("0.42") + LD("0.5") * np.cos(2 * PI * v / L) + LD("0.08") * np.cos(4 * PI * v / L)
    out[inside] = np.sin(PI * v) / (PI * v) * w
    out[u == 0] = 1
    return out


def envelope(s, L, x):
    """s(x) = sum_m s[m] h_L(x - m) at ONE longdouble x; only the m with |x - m| <= L/2 + 1 are visited (h_L is 0 beyond)"""
    M = len(s)
    x = LD(x)
    lo = max(int(np.floor(x)) - L // 2 - 2, 0); hi = min(int(np.floor(x)) + L // 2 + 2, M - 1)
    if lo > hi:
        return CLD(0)
    m = np.arange(lo, hi + 1)
    return (np.asarray(s[lo:hi + 1], CLD) * h_L(x - m.astype(LD), L)).sum()


def render_terms(contribs, s, L, t0, dt, n_rx, n_bins):
    """every non-zero term of the render: (rx, n, a s(n - d), e^{j 2 pi f (n - d) dt}) for every contribution (rx, a, tau, f) and
    every output sample n of the row; samples outside [0, n_bins) and receivers outside the cube are dropped"""
    s = np.asarray(s, CLD)
    M = len(s)
    for rx, a, tau, f in contribs:
        if rx < 0 or rx >= n_rx or a == 0:
            continue
        d = start_of(tau, t0, dt)
        if not math.isfinite(d):
            continue
        # the envelope's support is inside (d - L/2 - 1, d + M + L/2): every n outside it adds exactly 0
        lo = max(int(math.floor(d)) - L // 2 - 2, 0); hi = min(int(math.floor(d)) + M + L // 2 + 2, n_bins - 1)
        dl = LD(d)
        for n in range(lo, hi + 1):
            x = LD(n) - dl
            e = envelope(s, L, x)
            if e == 0:
                continue
            yield rx, n, CLD(a) * e, cexp(2 * PI * LD(f) * (x * LD(dt)))


def render_ref(cube, pulse, contribs, s, L, t0, dt, doppler):
    """cube[rx, pulse, n] += a s(n - d) e^{j 2 pi f (n - d) dt} (f = 0 without doppler).  cube: np.clongdouble [n_rx][n_p][n_bins]."""
    for rx, n, y, rot in render_terms(contribs, s, L, t0, dt, cube.shape[0], cube.shape[2]):
        cube[rx, pulse, n] += y * rot if doppler else y
    return cube


def render_ref_pair(shape, pulse, contribs, s, L, t0, dt):
    """{False: the render without the Doppler term, True: with it}, from one pass over the terms"""
    out = {False: np.zeros(shape, CLD), True: np.zeros(shape, CLD)}
    for rx, n, y, rot in render_terms(contribs, s, L, t0, dt, shape[0], shape[2]):
        out[False][rx, pulse, n] += y
        out[True][rx, pulse, n] += y * rot
    return out


def accumulate_ref(cube, pulse, contribs, t0, dt):
    """the impulse cube: cube[rx, pulse, floor(d)] += a; bins outside [0, n_bins) and receivers outside the cube are dropped"""
    n_rx, _, n_bins = cube.shape
    for rx, a, tau, _f in contribs:
        if rx < 0 or rx >= n_rx:
            continue
        d = start_of(tau, t0, dt)
        if not math.isfinite(d):
            continue
        b = math.floor(d)
        if 0 <= b < n_bins:
            cube[rx, pulse, b] += CLD(a)
    return cube


def amplitude(power, phase):
    return CLD(np.sqrt(LD(power))) * cexp(LD(phase))


def contribs_rays(records, cspeed, carrier):
    """RTS_RENDER_RAYS / rts_cube_accumulate: every received ray, tau = rayLength / cspeed (float64, as stated),
    phi = -fmod(2 pi carrier tau, 2 pi)"""
    out = []
    for r in records:
        tau = float(np.float64(r["rayLength"]) / np.float64(cspeed))
        ph = -np.fmod(2 * PI * LD(carrier) * LD(tau), 2 * PI)
        out.append((int(r["received"]), amplitude(r["power"], ph), tau, float(r["doppler"])))
    return out


def contribs_paths(received, power, doppler, delay, phase, path_match):
    """RTS_RENDER_PATHS / rts_cube_accumulate_paths: the representative (pathMatch[i] == i) of each group with the group's
    power, delay, phase and Doppler"""
    out = []
    for i in range(len(received)):
        if int(path_match[i]) != i:
            continue
        out.append((int(received[i]), amplitude(power[i], phase[i]), float(delay[i]), float(doppler[i])))
    return out


def correlate_ref(y, s):
    """z[n] = sum_m y[n + m] conj(s[m]), y[j] = 0 for j >= len(y) (one pass over the row per waveform sample)"""
    y = np.asarray(y, CLD); s = np.asarray(s, CLD)
    N = len(y)
    z = np.zeros(N, CLD)
    for m in range(min(len(s), N)):
        z[:N - m] += y[m:] * np.conj(s[m])
    return z


def dft_ref(x, n_fft):
    """out[..., k, :] = sum_p x[..., p, :] e^{-2 pi j k p / n_fft} over axis 1 of x [n_rx][n_pulses][n_bins], pulses beyond
    n_pulses counting as zeros: the direct sum, with the twiddle taken at the exact integer k p mod n_fft"""
    x = np.asarray(x, CLD)
    n_rx, n_p, n_bins = x.shape
    r = np.arange(n_fft)
    tw = np.cos(2 * PI * r.astype(LD) / n_fft).astype(CLD) - CLD(1j) * np.sin(2 * PI * r.astype(LD) / n_fft).astype(CLD)
    out = np.zeros((n_rx, n_fft, n_bins), CLD)
    k = np.arange(n_fft)
    for p in range(n_p):
        w = tw[(k * p) % n_fft]
        out += w[None, :, None] * x[:, p, None, :]
    return out


def to_double(z):
    return np.asarray(z).astype(np.complex128)
