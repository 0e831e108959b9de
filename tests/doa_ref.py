"""What tests/test_doa_host.py and tests/test_gpu_doa.py share: the plain-Python restatement of the eigensolver's and the angular
scan's trees and of the round-robin pairing from the text of include/rts_amd.h alone (RtsEigParams, RtsDoaScanParams -- Python floats
never contract, no numpy arithmetic in a sum), the header's constants, seeded matrices, the accuracy figures against numpy and the
two-source scenario of the whole chain."""
import math
import os
import re

import numpy as np

import beam_ref as B

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def header_constant(name):
    for path in (os.path.join(ROOT, "include", "rts_amd.h"), os.path.join(ROOT, "rts_amd", "csrc", "rts_doa.h")):
        with open(path) as f:
            m = re.search(r"#define %s\s+(\d+)u" % name, f.read())
        if m:
            return int(m.group(1))
    raise KeyError(name)


MAX_SWEEPS, MAX_N = header_constant("RTS_EIG_MAX_SWEEPS"), header_constant("RTS_BEAM_MAX_RX")
EIG_THREADS, SCAN_THREADS = header_constant("RTS_EIG_THREADS"), header_constant("RTS_DOA_THREADS")
RX_TILE, VEC_TILE = header_constant("RTS_DOA_RX_TILE"), header_constant("RTS_DOA_VEC_TILE")
EPS = 2.0 ** -52
TOL2, EPS2, DBL_MAX = 2.0 ** -100, 2.0 ** -104, 1.7976931348623157e308


# ----------------------------------------------------------------------------- the pairing, literally
def rounds(n):
    """the rounds of a sweep: lists of (p, q), p < q < n (the bye of an odd n left out)"""
    M = n + (n & 1)
    out = []
    for r in range(M - 1):
        pairs = []
        for k in range(M // 2):
            a, b = (M - 1, r) if k == 0 else ((r + k) % (M - 1), (r + M - 1 - k) % (M - 1))
            p, q = min(a, b), max(a, b)
            if q < n:
                pairs.append((p, q))
        out.append(pairs)
    return out


# ----------------------------------------------------------------------------- the eigensolver's tree, literally
class EigFailed(Exception):
    def __init__(self, status):
        super().__init__("status %d" % status)
        self.status = status


def eig_restated(A):
    """(values [n] descending, vectors [n][n] with ROW k the eigenvector k, sweeps that rotated)"""
    n = A.shape[0]
    finite = lambda x: -DBL_MAX <= x <= DBL_MAX
    X = [[[0.0, 0.0] for _ in range(n)] for _ in range(n)]
    V = [[[1.0 if i == j else 0.0, 0.0] for j in range(n)] for i in range(n)]
    for i in range(n):
        for j in range(i + 1):
            re, im = float(A[i, j].real), float(A[i, j].imag)
            if not finite(re) or (i != j and not finite(im)):
                raise EigFailed(2)
            if i == j:
                X[i][i] = [re, 0.0]
            else:
                X[i][j] = [re, im]; X[j][i] = [re, -im]

    def norm2(col):
        s = X[0][col][0] * X[0][col][0] + X[0][col][1] * X[0][col][1]
        for i in range(1, n):
            s = s + (X[i][col][0] * X[i][col][0] + X[i][col][1] * X[i][col][1])
        return s

    def rotate(M, p, q, c, sr, si):
        for i in range(n):
            (ar, ai), (br, bi) = M[i][p], M[i][q]
            M[i][p] = [c * ar - (sr * br + si * bi), c * ai - (sr * bi - si * br)]
            M[i][q] = [(sr * ar - si * ai) + c * br, (sr * ai + si * ar) + c * bi]

    table = rounds(n)
    sweeps = 0
    while True:
        m2 = norm2(0)
        for col in range(1, n):
            v = norm2(col)
            if v > m2:
                m2 = v
        floor2 = EPS2 * m2
        rotated = False
        for pairs in table:
            for p, q in pairs:
                alpha, beta = norm2(p), norm2(q)
                gr = gi = None
                for i in range(n):
                    (pr, pi), (qr, qi) = X[i][p], X[i][q]
                    tr, ti = pr * qr + pi * qi, pr * qi - pi * qr
                    gr, gi = (tr, ti) if gr is None else (gr + tr, gi + ti)
                g2 = gr * gr + gi * gi
                if g2 <= TOL2 * (alpha * beta) or alpha <= floor2 or beta <= floor2:
                    continue
                g = math.sqrt(g2); er, ei = gr / g, gi / g
                zeta = (beta - alpha) / (2.0 * g)
                d = (-zeta if zeta < 0.0 else zeta) + math.sqrt(1.0 + zeta * zeta)
                t = -1.0 / d if zeta < 0.0 else 1.0 / d
                c = 1.0 / math.sqrt(1.0 + t * t); s = c * t
                sr, si = s * er, s * ei
                rotate(X, p, q, c, sr, si); rotate(V, p, q, c, sr, si)
                rotated = True
        if not rotated:
            break
        sweeps += 1
        if sweeps == MAX_SWEEPS:
            raise EigFailed(1)
    lam = []
    for col in range(n):
        s = V[0][col][0] * X[0][col][0] + V[0][col][1] * X[0][col][1]
        for i in range(1, n):
            s = s + (V[i][col][0] * X[i][col][0] + V[i][col][1] * X[i][col][1])
        lam.append(s)
    values = np.zeros(n); vectors = np.zeros((n, n), np.complex128)
    for col in range(n):
        k = sum(1 for j in range(n) if lam[j] > lam[col] or (lam[j] == lam[col] and j < col))
        values[k] = lam[col]
        for i in range(n):
            vectors[k, i] = complex(V[i][col][0], V[i][col][1])
    return values, vectors, sweeps


# ----------------------------------------------------------------------------- the scan's tree, literally
def scan_restated(vectors, g, table, inverse=False):
    """out [n_dirs] of the vectors [m][n], the weights g [m] and the host table [n_dirs][n]"""
    out = np.zeros(len(table))
    for d in range(len(table)):
        q = None
        for k in range(len(vectors)):
            yr, yi = B.term(vectors[k, 0], table[d, 0])
            for rx in range(1, vectors.shape[1]):
                tr, ti = B.term(vectors[k, rx], table[d, rx])
                yr, yi = yr + tr, yi + ti
            gp = float(g[k]) * (yr * yr + yi * yi)
            q = gp if q is None else q + gp
        out[d] = (1.0 / q if q != 0.0 else math.copysign(math.inf, q)) if inverse else q
    return out


# ----------------------------------------------------------------------------- inputs
def hermitian(a):
    """the exact conjugate symmetry and the real diagonal of a's lower triangle"""
    a = np.tril(a) + np.tril(a, -1).conj().T
    a[np.diag_indices(len(a))] = a.diagonal().real
    return a


def sample_cov(rng, n, K):
    """the sample covariance of K snapshots of n elements: rank min(n, K)"""
    z = B.random_complex(rng, (n, K))
    return hermitian(z @ z.conj().T / K)


def matrix(kind, n, seed=0):
    """the test matrices: "full" (K = 4 n snapshots), "square" (K = n: full rank, barely), "deficient" (K = n // 3 or 1), "one" (K = 1),
    "identity", "diagonal" (a repeated and a zero entry)"""
    rng = np.random.default_rng(1000 * n + seed)
    if kind == "full":
        return sample_cov(rng, n, 4 * n)
    if kind == "square":
        return sample_cov(rng, n, n)
    if kind == "deficient":
        return sample_cov(rng, n, max(n // 3, 1))
    if kind == "one":
        return sample_cov(rng, n, 1)
    if kind == "identity":
        return np.eye(n, dtype=np.complex128)
    d = np.array([float((3 * i) % 5) for i in range(n)])           # 0, 3, 1, 4, 2, 0, ...: a zero and, from n = 6 on, repeats
    if n >= 2:
        d[-1] = d[0] = 3.0
        if n >= 3:
            d[1] = 0.0
    return np.diag(d).astype(np.complex128)


def accuracy(A, values, vectors):
    """(max |lambda - lambda_ref| / (eps |A|_2), |A V - V Lambda|_2 / (eps |A|_2), |V^H V - I|_2 / eps) against numpy.linalg.eigh; the
    columns of V are the rows of `vectors`"""
    ref = np.linalg.eigvalsh(A)[::-1]
    nA = max(abs(ref[0]), abs(ref[-1]))
    V = vectors.T
    return (float(np.max(np.abs(values - ref)) / (EPS * nA)), float(np.linalg.norm(A @ V - V * values[None, :], 2) / (EPS * nA)),
            float(np.linalg.norm(V.conj().T @ V - np.eye(len(A)), 2) / EPS))


# ----------------------------------------------------------------------------- the two-source scenario
# 8 elements on a half-wavelength line; two equal sources 6 degrees apart, circular complex Gaussian of unit power (the signal model
# AIC and MDL are derived for), complex noise of amplitude 0.1 (20 dB SNR), 256 snapshots in one row of 256 bins; a grid of -30 .. 30 degrees in steps of 0.25.
# The conventional (Bartlett) spectrum cannot separate them; MUSIC and Capon can.
SCENE = dict(n_rx=8, wavelength=0.03, K=256, seed=1, sources=np.radians([-3.0, 3.0]), noise_amp=0.1,
             grid=np.radians(np.arange(-30.0, 30.0 + 0.125, 0.25)), step=math.radians(0.25))


def scene_geometry():
    pos = B.line_array(SCENE["n_rx"], SCENE["wavelength"])
    directions = np.stack([SCENE["grid"], np.zeros(len(SCENE["grid"]))], axis=1)
    return pos, directions


def scene_cube(rts):
    """complex [n_rx][1][K]: the sources' steering vectors (the library's own, so that the grid holds them exactly) times their
    amplitudes, plus the noise"""
    pos, _ = scene_geometry()
    rng = np.random.default_rng(SCENE["seed"])
    a = rts.steering(pos, np.stack([SCENE["sources"], np.zeros(2)], axis=1), SCENE["wavelength"])           # [2][n_rx]
    s = B.random_complex(rng, (2, SCENE["K"])) / math.sqrt(2.0)
    noise = SCENE["noise_amp"] / math.sqrt(2.0) * B.random_complex(rng, (SCENE["n_rx"], SCENE["K"]))
    return (a.T @ s + noise)[:, None, :]


def scene_host(rts, method, n_sources=None, loading=0.0):
    """the host chain: covariance_eval -> eig_eval -> doa_weights -> doa_scan_eval: (spectrum [n_dirs], eigenvalues)"""
    pos, directions = scene_geometry()
    table = rts.steering(pos, directions, SCENE["wavelength"])
    values, vectors = rts.eig_eval(rts.covariance_eval(scene_cube(rts)))
    if n_sources is None and method == "music":
        n_sources = rts.source_count(values, SCENE["K"], "mdl")
    first, g, inverse = rts.doa_weights(method, values, n_sources or 0, loading)
    return rts.doa_scan_eval(vectors[first:first + len(g)], g, table, inverse), values


def peaks(spectrum, floor=0.1):
    """the indices of the local maxima above floor times the largest value"""
    s = np.asarray(spectrum); top = floor * s.max()
    return [i for i in range(1, len(s) - 1) if s[i] > s[i - 1] and s[i] >= s[i + 1] and s[i] > top]
