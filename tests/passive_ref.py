"""Independent restatements of the passive radar's two steps (include/rts_amd.h: RtsCancelParams, RtsXcorrParams), written from the
header's text and not from rts_amd/csrc/rts_passive.h:

  * cancel_restated / xcorr_restated: the two trees literally, in plain Python floats (which never contract): the lagged read, the
    term, the tiles and parts of the sums, the loading, the column Cholesky and the two substitutions, the failed block, the
    subtraction in ascending k; for BIT equality with the evaluators;
  * cancel_numpy / xcorr_numpy: the definition -- np.linalg.lstsq on the stacked lag matrix of each block, sums of shifted products --
    in float64, and the normal equations solved in longdouble (coeffs_longdouble), for the bounds.

The seeded inputs and the edge shapes the host and the GPU tests share are here too (the chain's scenario: tests/passive_chain_ref.py)."""
import math
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = 2.0 ** -52


def header_constant(name):
    with open(os.path.join(ROOT, "include", "rts_amd.h")) as f:
        m = re.search(r"#define %s\s+(\d+)u" % name, f.read())
    if not m:
        raise KeyError(name)
    return int(m.group(1))


TILE, MAX_PARTS, MAX_TAPS, MAX_BLOCKS = (header_constant("RTS_PASSIVE_" + n) for n in ("TILE", "MAX_PARTS", "MAX_TAPS", "MAX_BLOCKS"))
MAX_LAGS, MAX_BINS = header_constant("RTS_XCORR_MAX_LAGS"), header_constant("RTS_COMPRESS_MAX_BINS")


def random_complex(rng, shape):
    return rng.standard_normal(shape) + 1j * rng.standard_normal(shape)


def bits(a):
    return np.ascontiguousarray(a).view(np.float64)


# ----------------------------------------------------------------------------- the partition
def blocks(n_rows, rows_per_block):
    """[(first row inside the span, rows)] of the blocks"""
    R = n_rows if rows_per_block == 0 or rows_per_block > n_rows else rows_per_block
    return [(r0, min(R, n_rows - r0)) for r0 in range(0, n_rows, R)]


def parts(n_rows_block, n_bins, n_blocks):
    """the parts of one block: each a list of cells (row inside the block, bin) in ascending order"""
    tpr = (n_bins + TILE - 1) // TILE
    tiles = [(row, t * TILE, min(n_bins, (t + 1) * TILE)) for row in range(n_rows_block) for t in range(tpr)]
    n_parts = min(len(tiles), max(1, MAX_PARTS // n_blocks))
    out = []
    for q in range(n_parts):
        cells = []
        for row, n0, n1 in tiles[q * len(tiles) // n_parts:(q + 1) * len(tiles) // n_parts]:
            cells.extend((row, n) for n in range(n0, n1))
        out.append(cells)
    return out


# ----------------------------------------------------------------------------- the trees, literally
def _term(ar, ai, br, bi):
    return ar * br + ai * bi, ai * br - ar * bi


def _tree_sum(part_list, a_of, b_of):
    """sum of a conj(b) over the parts' cells: ascending inside a part, the first term the start value; parts ascending, part 0 the start value"""
    sr = si = 0.0
    for q, cells in enumerate(part_list):
        pr = pi = 0.0
        for c, cell in enumerate(cells):
            tr, ti = _term(*a_of(cell), *b_of(cell))
            if c == 0:
                pr, pi = tr, ti
            else:
                pr += tr; pi += ti
        if q == 0:
            sr, si = pr, pi
        else:
            sr += pr; si += pi
    return sr, si


def _pivot_ok(d):
    return d > 0.0 and d <= 1.7976931348623157e308


def _solve(A, bs):
    """A: lower triangle as lists of (re, im) (the diagonal's imaginary part unused); bs: right sides.  None on a failed pivot"""
    K = len(A)
    Lr = [[A[i][j][0] for j in range(i + 1)] for i in range(K)]; Li = [[A[i][j][1] for j in range(i + 1)] for i in range(K)]
    for j in range(K):
        d = Lr[j][j]
        for k in range(j):
            d -= Lr[j][k] * Lr[j][k] + Li[j][k] * Li[j][k]
        if not _pivot_ok(d):
            return None
        ljj = math.sqrt(d); Lr[j][j] = ljj
        for i in range(j + 1, K):
            xr, xi = Lr[i][j], Li[i][j]
            for k in range(j):
                tr, ti = _term(Lr[i][k], Li[i][k], Lr[j][k], Li[j][k])
                xr -= tr; xi -= ti
            Lr[i][j] = xr / ljj; Li[i][j] = xi / ljj
    out = []
    for b in bs:
        ur, ui = [0.0] * K, [0.0] * K
        for i in range(K):
            xr, xi = b[i]
            for k in range(i):
                xr -= Lr[i][k] * ur[k] - Li[i][k] * ui[k]; xi -= Lr[i][k] * ui[k] + Li[i][k] * ur[k]
            ur[i] = xr / Lr[i][i]; ui[i] = xi / Lr[i][i]
        for i in range(K - 1, -1, -1):
            xr, xi = ur[i], ui[i]
            for k in range(i + 1, K):
                xr -= Lr[k][i] * ur[k] + Li[k][i] * ui[k]; xi -= Lr[k][i] * ui[k] - Li[k][i] * ur[k]
            ur[i] = xr / Lr[i][i]; ui[i] = xi / Lr[i][i]
        out.append(list(zip(ur, ui)))
    return out


def selected(n_rx, ref_rx, rx=None):
    if rx is None:
        return [r for r in range(n_rx) if r != ref_rx]
    if isinstance(rx, (int, np.integer)):
        return [r for r in range(64) if (int(rx) >> r) & 1]
    return sorted(int(r) for r in rx)


def cancel_restated(cube, ref_rx, n_taps, rows_per_block=0, first=0, count=None, rx=None, loading=0.0):
    """-> (cancelled cube, coefficients [n_rx][n_blocks][K], (n_blocks, n_failed))"""
    cube = np.array(cube, np.complex128)
    n_rx, n_p, N = cube.shape
    count = n_p - first if count is None else count
    K = n_taps
    blks = blocks(count, rows_per_block)
    coeffs = np.zeros((n_rx, len(blks), K), np.complex128)
    failed = 0
    for b, (r0, rb) in enumerate(blks):
        ref = [[(float(v.real), float(v.imag)) for v in cube[ref_rx, first + r0 + row]] for row in range(rb)]
        lag = lambda k: (lambda cell: ref[cell[0]][cell[1] - k] if cell[1] >= k else (0.0, 0.0))
        pl = parts(rb, N, len(blks))
        A = [[None] * (i + 1) for i in range(K)]
        for i in range(K):
            for j in range(i + 1):
                gr, gi = _tree_sum(pl, lag(j), lag(i))
                A[i][j] = (gr + loading, gi) if i == j else (gr, gi)
        sel = selected(n_rx, ref_rx, rx)
        ys = {r: [[(float(v.real), float(v.imag)) for v in cube[r, first + r0 + row]] for row in range(rb)] for r in sel}
        bs = [[_tree_sum(pl, (lambda cell, y=ys[r]: y[cell[0]][cell[1]]), lag(i)) for i in range(K)] for r in sel]
        cs = _solve(A, bs)
        if cs is None:
            failed += 1
            continue
        for r, c in zip(sel, cs):
            coeffs[r, b] = [complex(*v) for v in c]
            for row in range(rb):
                x = ref[row]
                for n in range(N):
                    yr, yi = ys[r][row][n]
                    for k in range(K):
                        xr, xi = x[n - k] if n >= k else (0.0, 0.0)
                        yr -= c[k][0] * xr - c[k][1] * xi; yi -= c[k][0] * xi + c[k][1] * xr
                    cube[r, first + r0 + row, n] = complex(yr, yi)
    return cube, coeffs, (len(blks), failed)


def xcorr_restated(cube, ref_rx, n_lags, first_lag=0, first=0, count=None):
    cube = np.asarray(cube, np.complex128)
    n_rx, n_p, N = cube.shape
    count = n_p - first if count is None else count
    out = np.zeros((n_rx, count, n_lags), np.complex128)
    for row in range(count):
        x = [(float(v.real), float(v.imag)) for v in cube[ref_rx, first + row]]
        for r in range(n_rx):
            y = [(float(v.real), float(v.imag)) for v in cube[r, first + row]]
            for li in range(n_lags):
                l = first_lag + li
                sr = si = 0.0
                for n in range(max(N - l, 0)):
                    tr, ti = _term(*y[n + l], *x[n])
                    if n == 0:
                        sr, si = tr, ti
                    else:
                        sr += tr; si += ti
                out[r, row, li] = complex(sr, si)
    return out


# ----------------------------------------------------------------------------- the definition, in numpy
def lag_matrix(ref_rows, K, dtype=np.complex128):
    """ref_rows [rows][N] -> X [rows N][K]: column k the rows shifted by k bins, zeros shifted in"""
    rows, N = ref_rows.shape
    X = np.zeros((rows, N, K), dtype)
    for k in range(min(K, N)):
        X[:, k:, k] = ref_rows[:, :N - k]
    return X.reshape(rows * N, K)


def cancel_numpy(cube, ref_rx, n_taps, rows_per_block=0, first=0, count=None, rx=None):
    """least squares per block by np.linalg.lstsq (loading 0) -> (cancelled cube, coefficients)"""
    cube = np.array(cube, np.complex128)
    n_rx, n_p, N = cube.shape
    count = n_p - first if count is None else count
    blks = blocks(count, rows_per_block)
    coeffs = np.zeros((n_rx, len(blks), n_taps), np.complex128)
    for b, (r0, rb) in enumerate(blks):
        sl = slice(first + r0, first + r0 + rb)
        X = lag_matrix(cube[ref_rx, sl], n_taps)
        for r in selected(n_rx, ref_rx, rx):
            c = np.linalg.lstsq(X, cube[r, sl].reshape(-1), rcond=None)[0]
            coeffs[r, b] = c
            cube[r, sl] -= (X @ c).reshape(rb, N)
    return cube, coeffs


def gram_longdouble(ref_rows, y_rows, K, loading=0.0):
    """(G + loading I, b) of one block in longdouble"""
    X = lag_matrix(ref_rows.astype(np.clongdouble), K, np.clongdouble)
    G = X.conj().T @ X + np.longdouble(loading) * np.eye(K, dtype=np.clongdouble)
    return G, X.conj().T @ y_rows.astype(np.clongdouble).reshape(-1)


def solve_longdouble(A, b):
    """Gaussian elimination with partial pivoting in longdouble"""
    A = np.array(A, np.clongdouble); b = np.array(b, np.clongdouble); n = len(b)
    for j in range(n):
        p = j + int(np.argmax(np.abs(A[j:, j])))
        if p != j:
            A[[j, p]] = A[[p, j]]; b[[j, p]] = b[[p, j]]
        f = A[j + 1:, j] / A[j, j]
        A[j + 1:] -= f[:, None] * A[j][None, :]; b[j + 1:] -= f * b[j]
    x = np.zeros(n, np.clongdouble)
    for i in range(n - 1, -1, -1):
        x[i] = (b[i] - A[i, i + 1:] @ x[i + 1:]) / A[i, i]
    return x


def solve_bound(A):
    """the forward error of a Cholesky solve relative to the solution's largest entry: K eps cond(A) (tests/adapt_ref.py's bound)"""
    return A.shape[0] * EPS * np.linalg.cond(np.asarray(A, np.complex128))


def xcorr_numpy(cube, ref_rx, n_lags, first_lag=0, first=0, count=None, dtype=np.complex128):
    cube = np.asarray(cube).astype(dtype)
    n_rx, n_p, N = cube.shape
    count = n_p - first if count is None else count
    out = np.zeros((n_rx, count, n_lags), dtype)
    for li in range(n_lags):
        l = first_lag + li
        if l < N:
            out[:, :, li] = np.einsum("rpn,pn->rp", cube[:, first:first + count, l:], cube[ref_rx, first:first + count, :N - l].conj())
    return out


# ----------------------------------------------------------------------------- the edge shapes both suites run
# (name, n_rx, n_pulses, n_bins, dict of cancel arguments).  K at its ends; bins around K and around the tile; every rows_per_block
# against the span; a short last block; the reference first and last; one receiver; a mask; parts around the cap of a block
def cancel_cases():
    c = []
    for K in (1, 2, 63, 64):
        for N in sorted({1, max(K - 1, 1), K, K + 1}):
            c.append(("K%d_N%d" % (K, N), 2, 2, N, dict(ref_rx=0, n_taps=K, loading=1e-3)))
    for N in (TILE - 1, TILE, TILE + 1):
        c.append(("tile_N%d" % N, 3, 2, N, dict(ref_rx=1, n_taps=3)))
    span = 5
    for R in (0, 1, span - 1, span, span + 1):
        c.append(("R%d" % R, 3, span + 2, 37, dict(ref_rx=2, n_taps=4, rows_per_block=R, first=1, count=span)))
    c.append(("short_last", 2, 7, 21, dict(ref_rx=0, n_taps=2, rows_per_block=3)))
    c.append(("ref_last", 4, 3, 40, dict(ref_rx=3, n_taps=5, rows_per_block=2)))
    c.append(("one_rx", 1, 3, 33, dict(ref_rx=0, n_taps=3)))
    c.append(("mask", 4, 3, 33, dict(ref_rx=1, n_taps=3, rx=[0, 3])))
    # MAX_PARTS / 128 blocks = 4 parts per block: 3, 4 and 5 tiles of one row
    for tiles in (3, 4, 5):
        c.append(("cap_%dtiles" % tiles, 2, 128, (tiles - 1) * TILE + 7, dict(ref_rx=0, n_taps=1, rows_per_block=1)))
    # a part that owns SEVERAL tiles with several taps: sums carried in registers across tiles, the first term only at the part's first
    # tile, the history staged again at each later tile.  257 and 260 blocks leave one part per block: three tiles in three rows, and
    # two tiles of one row
    c.append(("part_rows_K5", 2, 771, 9, dict(ref_rx=0, n_taps=5, rows_per_block=3)))
    c.append(("part_tiles_K3", 2, 260, TILE + 9, dict(ref_rx=1, n_taps=3, rows_per_block=1)))
    return c


def cancel_cases_evaluator_only():
    """as cancel_cases, too large for the plain-Python restatement: the evaluator against numpy on the host, the device against the
    evaluator.  64 taps (nine waves of entry blocks) with three tiles, in two rows and two tiles of a row, in each block's one part"""
    return [("part_K64", 2, 514, TILE + 14, dict(ref_rx=0, n_taps=64, rows_per_block=2, loading=1e-3))]


def cancel_input(name, n_rx, n_p, N, kw):
    """seeded: a noise reference, surveillance rows = a few lagged copies of it + an independent part; rows outside the span NaN"""
    rng = np.random.default_rng(sum(ord(ch) for ch in name) * 7919 + N)
    cube = random_complex(rng, (n_rx, n_p, N))
    ref = cube[kw["ref_rx"]].copy()
    for r in range(n_rx):
        if r == kw["ref_rx"]:
            continue
        for k in range(min(kw["n_taps"], 3, N)):
            sh = np.zeros_like(ref); sh[:, k:] = ref[:, :N - k]
            cube[r] += (3.0 - k) * np.exp(1j * (r + k)) * sh
    first = kw.get("first", 0); count = kw.get("count", None)
    if first or count is not None:
        count = n_p - first if count is None else count
        cube[:, :first] = np.nan; cube[:, first + count:] = np.nan
    return cube


def xcorr_cases():
    """(name, n_rx, n_pulses, n_bins, dict of xcorr arguments)"""
    c = []
    for N in (1, 5, TILE - 1, TILE, TILE + 1, 2 * TILE + 3):
        for n_lags in sorted({1, N, N + 3}):
            c.append(("N%d_L%d" % (N, n_lags), 2, 2, N, dict(ref_rx=0, n_lags=n_lags)))
    c.append(("first_lag", 3, 4, 50, dict(ref_rx=2, n_lags=20, first_lag=7, first=1, count=2)))
    c.append(("first_lag_past", 2, 2, 30, dict(ref_rx=1, n_lags=5, first_lag=28)))
    c.append(("one_rx", 1, 3, 40, dict(ref_rx=0, n_lags=40)))
    c.append(("two_groups", 2, 1, 300, dict(ref_rx=1, n_lags=260, first_lag=3)))
    return c


def xcorr_input(name, n_rx, n_p, N, kw):
    rng = np.random.default_rng(sum(ord(ch) for ch in name) * 104729 + N)
    cube = random_complex(rng, (n_rx, n_p, N))
    first = kw.get("first", 0); count = kw.get("count", None)
    if first or count is not None:
        count = n_p - first if count is None else count
        cube[:, :first] = np.nan; cube[:, first + count:] = np.nan
    return cube
