"""What tests/test_adapt_host.py and tests/test_gpu_adapt.py share: the plain-Python restatement of the two trees of adaptive
beamforming from the text of include/rts_amd.h alone (RtsCovParams, RtsMvdrParams -- Python floats never contract, no numpy
arithmetic in a sum), the header's constants, seeded inputs and the jammer scenario of the properties and of the whole chain."""
import math
import os
import re

import numpy as np

import beam_ref as B

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def header_constant(name):
    for path in (os.path.join(ROOT, "include", "rts_amd.h"), os.path.join(ROOT, "rts_amd", "csrc", "rts_adapt.h")):
        with open(path) as f:
            m = re.search(r"#define %s\s+(\d+)u" % name, f.read())
        if m:
            return int(m.group(1))
    raise KeyError(name)


TILE, MAX_PARTS = header_constant("RTS_ADAPT_TILE"), header_constant("RTS_ADAPT_MAX_PARTS")
BLOCK, SOLVE_THREADS = header_constant("RTS_ADAPT_BLOCK"), header_constant("RTS_MVDR_THREADS")
EPS = 2.0 ** -52


# ----------------------------------------------------------------------------- the covariance's tree, literally
def training_cells(rows, bins, first=0, count=None, first_bin=0, n_bins=None, skip=None):
    """the (row, bin) of the training cells c = 0 .. K - 1: row-major over the included bins"""
    count = rows - first if not count else count
    n_bins = bins - first_bin if not n_bins else n_bins
    lo, n = skip if skip is not None else (0, 0)
    keep = [b for b in range(first_bin, first_bin + n_bins) if not (n and lo <= b < lo + n)]
    return [(r, b) for r in range(first, first + count) for b in keep]


def partition(K):
    """the cell ranges [c0, c1) of the parts"""
    tiles = (K + TILE - 1) // TILE
    parts = min(MAX_PARTS, tiles)
    return [(p * tiles // parts * TILE, min((p + 1) * tiles // parts * TILE, K)) for p in range(parts)]


def cov_restated(inp, **train):
    """R [n_rx][n_rx]: per part the sum of z_i conj(z_j) over ascending cells, the first term the start value; the parts summed in
    ascending order, part 0 the start value; each component divided once by K; the upper triangle the conjugate, the diagonal's
    imaginary part +0.0"""
    n_rx, rows, bins = inp.shape
    cells = training_cells(rows, bins, **train)
    K = len(cells)
    z = [[(float(inp[r, row, b].real), float(inp[r, row, b].imag)) for (row, b) in cells] for r in range(n_rx)]
    out = np.zeros((n_rx, n_rx), np.complex128)
    for i in range(n_rx):
        for j in range(i + 1):
            sr = si = None
            for c0, c1 in partition(K):
                pr = pi = None
                for c in range(c0, c1):
                    ar, ai = z[i][c]; br, bi = z[j][c]
                    tr, ti = ar * br + ai * bi, ai * br - ar * bi
                    pr, pi = (tr, ti) if pr is None else (pr + tr, pi + ti)
                sr, si = (pr, pi) if sr is None else (sr + pr, si + pi)
            sr, si = sr / float(K), si / float(K)
            if i == j:
                out[i, i] = complex(sr, 0.0)
            else:
                out[i, j] = complex(sr, si); out[j, i] = complex(sr, -si)
    return out


# ----------------------------------------------------------------------------- the weight tree, literally
class SolveFailed(Exception):
    def __init__(self, pivot):
        super().__init__("pivot %d" % pivot)
        self.pivot = pivot


def mvdr_restated(cov, steering, loading=0.0):
    """w [n_beams][n_rx]: A = R + loading I on the diagonal's real part, column Cholesky by running subtraction, per beam the forward
    substitution, den, the back substitution and the division"""
    n = cov.shape[0]
    L = [[[float(cov[i, j].real), float(cov[i, j].imag)] for j in range(n)] for i in range(n)]
    for i in range(n):
        L[i][i][0] = L[i][i][0] + float(loading)
    for j in range(n):
        d = L[j][j][0]
        for k in range(j):
            d = d - (L[j][k][0] * L[j][k][0] + L[j][k][1] * L[j][k][1])
        if not (d > 0.0 and d <= 1.7976931348623157e308):
            raise SolveFailed(j)
        ljj = math.sqrt(d)
        L[j][j] = [ljj, 0.0]
        for i in range(j + 1, n):
            xr, xi = L[i][j]
            for k in range(j):
                ar, ai = L[i][k]; br, bi = L[j][k]
                xr, xi = xr - (ar * br + ai * bi), xi - (ai * br - ar * bi)
            L[i][j] = [xr / ljj, xi / ljj]
    out = np.zeros(steering.shape, np.complex128)
    for b in range(steering.shape[0]):
        u = []
        for i in range(n):
            xr, xi = float(steering[b, i].real), float(steering[b, i].imag)
            for k in range(i):
                lr, li = L[i][k]; ur, ui = u[k]
                xr, xi = xr - (lr * ur - li * ui), xi - (lr * ui + li * ur)
            u.append((xr / L[i][i][0], xi / L[i][i][0]))
        den = u[0][0] * u[0][0] + u[0][1] * u[0][1]
        for k in range(1, n):
            den = den + (u[k][0] * u[k][0] + u[k][1] * u[k][1])
        v = list(u)
        for i in range(n - 1, -1, -1):
            xr, xi = v[i]
            for k in range(i + 1, n):
                lr, li = L[k][i]; vr, vi = v[k]
                xr, xi = xr - (lr * vr + li * vi), xi - (lr * vi - li * vr)
            v[i] = (xr / L[i][i][0], xi / L[i][i][0])
        for i in range(n):
            out[b, i] = complex(v[i][0] / den, v[i][1] / den)
    return out


# ----------------------------------------------------------------------------- inputs
def shape_for(K, odd=True):
    """(rows, bins) with rows * bins == K: more than one row where K allows it"""
    for rows in (3, 2):
        if K % rows == 0 and K > rows:
            return rows, K // rows
    return 1, K


def hermitian_pd(rng, n, cond=10.0):
    """a random Hermitian positive definite matrix with the exact conjugate symmetry and a real diagonal the kernels expect"""
    x = B.random_complex(rng, (n, 4 * n))
    a = x @ x.conj().T / (4 * n) + np.eye(n) / cond
    a = np.tril(a) + np.tril(a, -1).conj().T
    a[np.diag_indices(n)] = a.diagonal().real
    return a


def loaded(cov, loading):
    return cov + loading * np.eye(cov.shape[0])


def solve_bound(A):
    """the forward error of a Cholesky solve relative to the solution's largest entry: n eps cond(A)"""
    return A.shape[0] * EPS * np.linalg.cond(A)


def mvdr_numpy(cov, steering, loading=0.0):
    A = loaded(cov, loading)
    x = np.linalg.solve(A, steering.T).T                    # rows A^-1 s_b
    return x / np.einsum("bi,bi->b", steering.conj(), x)[:, None]


# ----------------------------------------------------------------------------- the jammer scenario
# 8 elements on a half-wavelength line, 16 pulses of 48 bins; white noise of unit power per element, a jammer plane wave 30 dB above
# it in every cell (a new random amplitude per cell), and one target of power 4 in bin 20 of every pulse.  The training set leaves
# bins 18 .. 22 out: the target and a guard of two on each side.  The fan holds the target's beam, the jammer's and three others.
SCENE = dict(n_rx=8, n_pulses=16, n_bins=48, wavelength=0.03, noise_power=1.0, seed=4711, jammer_az=math.radians(-25.0), jnr=1000.0,
             target_az=math.radians(10.0), target_bin=20, target_power=4.0, skip=(18, 5),
             fan=np.radians([10.0, -25.0, -50.0, 0.0, 35.0]), target_beam=0, jammer_beam=1)


def scene_geometry():
    wl = SCENE["wavelength"]
    pos = B.line_array(SCENE["n_rx"], wl)
    directions = np.stack([SCENE["fan"], np.zeros(len(SCENE["fan"]))], axis=1)
    return pos, directions, B.C0 / wl


def scene_clean_cube():
    """jammer + target, complex [n_rx][n_pulses][n_bins]; the noise is added by rts_noise_eval / rts_cube_add_noise"""
    pos, _, fc = scene_geometry()
    n_rx, n_p, nb = SCENE["n_rx"], SCENE["n_pulses"], SCENE["n_bins"]
    rng = np.random.default_rng(SCENE["seed"])
    amp = math.sqrt(SCENE["jnr"] / 2.0) * B.random_complex(rng, (n_p, nb))
    cube = B.snapshot(pos, SCENE["jammer_az"], 0.0, fc)[:, None, None] * amp[None]
    cube[:, :, SCENE["target_bin"]] += (math.sqrt(SCENE["target_power"]) * B.snapshot(pos, SCENE["target_az"], 0.0, fc))[:, None]
    return cube


def scene_host(rts):
    """the host chain: (noisy cube, steering, covariance, weights, beams [5][n_pulses][n_bins])"""
    pos, directions, _ = scene_geometry()
    n_rx, n_p, nb = SCENE["n_rx"], SCENE["n_pulses"], SCENE["n_bins"]
    cube = scene_clean_cube() + rts.noise_eval(SCENE["seed"], np.arange(n_rx * n_p * nb, dtype=np.uint64), SCENE["noise_power"]).reshape(n_rx, n_p, nb)
    s = rts.steering(pos, directions, SCENE["wavelength"])
    cov = rts.covariance_eval(cube, skip=SCENE["skip"])
    w = rts.mvdr_eval(cov, s, SCENE["noise_power"])
    return cube, s, cov, w, rts.beamform_eval(cube, w)


def assert_mvdr_properties(w, s, cov, loading, jammer_steering, jammer_beam):
    """distortionless, no more output power than the conventional beam, and a deeper null on the jammer in every other beam"""
    A = loaded(cov, loading)
    n = A.shape[0]
    bound = solve_bound(A)
    for b in range(len(w)):
        c = s[b] / n
        assert abs(np.vdot(w[b], s[b]) - 1.0) <= bound, (b, abs(np.vdot(w[b], s[b]) - 1.0), bound)
        pw, pc = np.vdot(w[b], A @ w[b]).real, np.vdot(c, A @ c).real
        assert pw <= pc * (1.0 + bound), (b, pw, pc)
        if b != jammer_beam:
            gw, gc = abs(np.vdot(w[b], jammer_steering)) ** 2, abs(np.vdot(c, jammer_steering)) ** 2
            print("beam %d: the jammer %.1f dB below the conventional beam's" % (b, 10.0 * math.log10(gc / gw)))
            assert gw < gc, (b, gw, gc)
