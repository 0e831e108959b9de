"""What tests/test_stap_host.py and tests/test_gpu_stap.py share: the plain-Python restatement of the two trees of space-time
adaptive processing and of the steering product from the text of include/rts_amd.h alone (RtsStCovParams, RtsStApplyParams --
Python floats never contract, no numpy arithmetic in a sum), numpy references, the header's constants, and the clutter scene of the
whole chain with its true covariance."""
import math

import numpy as np

import adapt_ref as A
import beam_ref as B

ROOT = A.ROOT
TILE, MAX_PARTS = A.TILE, A.MAX_PARTS


def stap_constant(name):
    import os
    import re
    for path in (os.path.join(ROOT, "include", "rts_amd.h"), os.path.join(ROOT, "rts_amd", "csrc", "rts_stap.h")):
        with open(path) as f:
            m = re.search(r"#define %s\s+(\d+)u" % name, f.read())
        if m:
            return int(m.group(1))
    raise KeyError(name)


MAX_TAPS, STRIP, RX_TILE, THREADS = (stap_constant(n) for n in ("RTS_ST_MAX_TAPS", "RTS_ST_STRIP", "RTS_ST_RX_TILE", "RTS_ST_THREADS"))
MAX_RX, MAX_BEAMS, MAX_WEIGHTS = (A.header_constant(n) for n in ("RTS_BEAM_MAX_RX", "RTS_BEAM_MAX_BEAMS", "RTS_BEAM_MAX_WEIGHTS"))


def filter_tile(taps):
    """RTS_ST_FILTER_TILE of rts_stap.h: the running sums of a thread stay at most 32"""
    return 16 if taps <= 2 else 8 if taps <= 4 else 4 if taps <= 8 else 2


# ----------------------------------------------------------------------------- the snapshot and the two trees, literally
def snapshot_element(inp, d, p, b):
    """x[d] of the snapshot at (row p, bin b): z[d % N][p + d / N][b]"""
    N = inp.shape[0]
    return inp[d % N, p + d // N, b]


def st_cov_restated(inp, taps, first=0, count=None, **bins):
    """R [D][D]: adapt_ref.cov_restated's tree over the snapshots whose START rows are first .. first + count - taps"""
    N, rows, nb = inp.shape
    count = rows - first if not count else count
    cells = A.training_cells(rows, nb, first=first, count=count - taps + 1, **bins)
    K, D = len(cells), N * taps
    x = [[(float(snapshot_element(inp, d, p, b).real), float(snapshot_element(inp, d, p, b).imag)) for (p, b) in cells] for d in range(D)]
    out = np.zeros((D, D), np.complex128)
    for i in range(D):
        for j in range(i + 1):
            sr = si = None
            for c0, c1 in A.partition(K):
                pr = pi = None
                for c in range(c0, c1):
                    ar, ai = x[i][c]; br, bi = x[j][c]
                    tr, ti = ar * br + ai * bi, ai * br - ar * bi
                    pr, pi = (tr, ti) if pr is None else (pr + tr, pi + ti)
                sr, si = (pr, pi) if sr is None else (sr + pr, si + pi)
            sr, si = sr / float(K), si / float(K)
            if i == j:
                out[i, i] = complex(sr, 0.0)
            else:
                out[i, j] = complex(sr, si); out[j, i] = complex(sr, -si)
    return out


def st_apply_restated(inp, w, taps, first=0, count=None):
    """y[f][p][b] = the sum of conj(w[f][d]) x[d] over ascending d, the d = 0 term the start value; complex [F][count - taps + 1][n_bins]"""
    N, rows, nb = inp.shape
    count = rows - first if not count else count
    out = np.zeros((w.shape[0], count - taps + 1, nb), np.complex128)
    for f in range(w.shape[0]):
        for p in range(count - taps + 1):
            for b in range(nb):
                yr, yi = B.term(w[f, 0], snapshot_element(inp, 0, first + p, b))
                for d in range(1, N * taps):
                    tr, ti = B.term(w[f, d], snapshot_element(inp, d, first + p, b))
                    yr, yi = yr + tr, yi + ti
                out[f, p, b] = complex(yr, yi)
    return out


def snapshots_numpy(inp, taps, first=0, count=None):
    """X [D][count - taps + 1][n_bins]: every snapshot of the span, stacked"""
    count = inp.shape[1] - first if not count else count
    return np.concatenate([inp[:, first + m:first + m + count - taps + 1] for m in range(taps)], axis=0)


def st_steering_restated(spatial, dopplers, taps, tap_taper, cos_sin):
    """out[beam n_doppler + k][m N + rx] = t_m spatial[beam][rx] = (tr ar - ti ai, tr ai + ti ar); t_m = taper[m] (cos, sin)(2 pi fr),
    fr = x - floor(x), x = f m.  cos_sin(fr): the library's cosine and sine of 2 pi fr (the caller takes them from rts_steering_make)"""
    nb, N = spatial.shape
    out = np.zeros((nb * len(dopplers), taps * N), np.complex128)
    for b in range(nb):
        for k, f in enumerate(dopplers):
            for m in range(taps):
                x = float(f) * float(m)
                c, s = cos_sin(x - math.floor(x))
                tr, ti = (c, s) if tap_taper is None else (float(tap_taper[m]) * c, float(tap_taper[m]) * s)
                for r in range(N):
                    ar, ai = float(spatial[b, r].real), float(spatial[b, r].imag)
                    out[b * len(dopplers) + k, m * N + r] = complex(tr * ar - ti * ai, tr * ai + ti * ar)
    return out


# ----------------------------------------------------------------------------- the clutter scene
# 8 elements on a half-wavelength line, 16 pulses of 48 bins on a platform moving along the array: 89 clutter patches at azimuths
# -88 .. 88 degrees on the ridge f = 0.5 sin az cycles per pulse, together 30 dB above the unit noise per element and pulse, each
# with a new random amplitude per bin, constant over the pulses; one target at broadside with f = 0.25, 0 dB, in bin 24 of every
# pulse.  The processor: 3 taps (D = 24), trained on every bin but 22 .. 26 (14 x 43 = 602 snapshots), loaded with the noise power.
SCENE = dict(n_rx=8, n_pulses=16, n_bins=48, wavelength=0.03, noise_power=1.0, seed=2027, n_patches=89, cnr=1000.0, ridge=0.5,
             target_az=0.0, target_f=0.25, target_bin=24, target_power=1.0, taps=3, skip=(22, 5), n_fft=16, doppler_row=4)


def scene_geometry():
    wl = SCENE["wavelength"]
    return B.line_array(SCENE["n_rx"], wl), B.C0 / wl


def patch_azimuths():
    return np.radians(np.linspace(-88.0, 88.0, SCENE["n_patches"]))


def space_time_vector(az, f, n_rows):
    """v [n_rows N], tap-major: e^{+2 pi j f p} times the plane wave of direction az on the array (the cube's phase convention)"""
    pos, fc = scene_geometry()
    return np.kron(np.exp(2j * np.pi * f * np.arange(n_rows)), B.snapshot(pos, az, 0.0, fc))


def scene_true_covariance(taps):
    """clutter plus noise of a snapshot of `taps` taps: sum_k (cnr / patches) v_k v_k^H + noise_power I"""
    D = SCENE["n_rx"] * taps
    R = SCENE["noise_power"] * np.eye(D, dtype=np.complex128)
    for az in patch_azimuths():
        v = space_time_vector(az, SCENE["ridge"] * math.sin(az), taps)
        R += SCENE["cnr"] / SCENE["n_patches"] * np.outer(v, v.conj())
    return R


def scene_clean_cube():
    """clutter + target, complex [n_rx][n_pulses][n_bins]; the noise is added by rts_noise_eval / rts_cube_add_noise"""
    n_rx, n_p, nb = SCENE["n_rx"], SCENE["n_pulses"], SCENE["n_bins"]
    rng = np.random.default_rng(SCENE["seed"])
    cube = np.zeros((n_rx, n_p, nb), np.complex128)
    for az in patch_azimuths():
        v = space_time_vector(az, SCENE["ridge"] * math.sin(az), n_p).reshape(n_p, n_rx).T
        amp = math.sqrt(SCENE["cnr"] / SCENE["n_patches"] / 2.0) * B.random_complex(rng, nb)
        cube += v[:, :, None] * amp[None, None, :]
    t = space_time_vector(SCENE["target_az"], SCENE["target_f"], n_p).reshape(n_p, n_rx).T
    cube[:, :, SCENE["target_bin"]] += math.sqrt(SCENE["target_power"]) * t
    return cube


def scene_noisy_cube(rts):
    n_rx, n_p, nb = SCENE["n_rx"], SCENE["n_pulses"], SCENE["n_bins"]
    return scene_clean_cube() + rts.noise_eval(SCENE["seed"], np.arange(n_rx * n_p * nb, dtype=np.uint64), SCENE["noise_power"]).reshape(n_rx, n_p, nb)


def scene_spatial_steering(rts):
    pos, _ = scene_geometry()
    return rts.steering(pos, [[SCENE["target_az"], 0.0]], SCENE["wavelength"])


def scene_host(rts, taps, cube=None):
    """the host chain on `cube` (default: the noisy scene): (cube, steering [1][D], covariance, weights [1][D], output [1][n_pulses - taps + 1][n_bins])"""
    cube = scene_noisy_cube(rts) if cube is None else cube
    s = rts.st_steering(scene_spatial_steering(rts), [SCENE["target_f"]], taps)
    cov = rts.st_covariance_eval(cube, taps, skip=SCENE["skip"])
    w = rts.mvdr_eval(cov, s, SCENE["noise_power"])
    return cube, s, cov, w, rts.st_apply_eval(cube, w, taps)


def sinr(w, s, R):
    """of a target of unit power with the space-time vector s behind the weights w, in the true covariance R"""
    return abs(np.vdot(w, s)) ** 2 / np.vdot(w, R @ w).real


def doppler_map(y, n_fft):
    """sum_p y[p] e^{-2 pi j k p / n_fft}: rts_cube_doppler's sign"""
    return np.fft.fft(y, n_fft, axis=-2)


def db(x):
    return 10.0 * math.log10(x)
