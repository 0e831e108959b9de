"""Independent restatements of the MIMO matched-filter bank (include/rts_amd.h: RtsBankParams), written from the header's text and
not from rts_amd/csrc/rts_mimo.h:

  * bank_restated: the tree literally -- per output the sum over m ascending from +0.0, no term beyond the row, every product and
    every sum an operation of its own, then the code multiply -- in plain Python floats for the small shapes and, for the large ones,
    in numpy float64 one m at a time over all bins (element-wise numpy operations round each on their own and never contract); for
    BIT equality with the evaluator;
  * bank_longdouble and term_magnitudes: the correlation in longdouble (tests/cube_ref.py's statement of the compression) and the
    sum of |y[n + m]| |s_t[m]|, for the accuracy bound.

The seeded inputs and the edge shapes the host and the GPU tests share are here too (the chain's scenario: tests/mimo_chain_ref.py)."""
import os
import re

import numpy as np

import cube_ref as CR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = 2.0 ** -52


def header_constant(name):
    with open(os.path.join(ROOT, "include", "rts_amd.h")) as f:
        m = re.search(r"#define %s\s+(\d+)u" % name, f.read())
    if not m:
        raise KeyError(name)
    return int(m.group(1))


TILE, MAX_WAVES, MAX_SAMPLES, MAX_BINS = (header_constant(n) for n in ("RTS_BANK_TILE", "RTS_BANK_MAX_WAVES", "RTS_WAVEFORM_MAX_SAMPLES", "RTS_COMPRESS_MAX_BINS"))


def random_complex(rng, shape):
    return rng.standard_normal(shape) + 1j * rng.standard_normal(shape)


def bits(a):
    return np.ascontiguousarray(a).view(np.float64)


def same(a, b):
    return np.array_equal(bits(a), bits(b), equal_nan=True)


# ----------------------------------------------------------------------------- the tree, literally
def _row_python(y, s):
    N, M = len(y), len(s)
    out = np.zeros(N, np.complex128)
    yr, yi = [float(v) for v in y.real], [float(v) for v in y.imag]
    sr, si = [float(v) for v in s.real], [float(v) for v in s.imag]
    for n in range(N):
        zr = zi = 0.0
        for m in range(M):
            if n + m >= N:
                break
            zr += yr[n + m] * sr[m] + yi[n + m] * si[m]
            zi += yi[n + m] * sr[m] - yr[n + m] * si[m]
        out[n] = complex(zr, zi)
    return out


def _row_numpy(y, s):
    N, M = len(y), len(s)
    yr, yi = np.ascontiguousarray(y.real), np.ascontiguousarray(y.imag)
    zr, zi = np.zeros(N), np.zeros(N)
    for m in range(min(M, N)):
        sr, si = float(s[m].real), float(s[m].imag)
        k = N - m
        zr[:k] = zr[:k] + (yr[m:] * sr + yi[m:] * si)
        zi[:k] = zi[:k] + (yi[m:] * sr - yr[m:] * si)
    return zr + 1j * zi


def bank_restated(cube, waves, code=None, first=0, count=None):
    """waves: a list of complex sample arrays; code: complex [n_waves][count] or None -> complex [n_waves * n_rx][count][n_bins]"""
    cube = np.asarray(cube, np.complex128)
    n_rx, n_p, N = cube.shape
    count = n_p - first if count is None else count
    out = np.zeros((len(waves) * n_rx, count, N), np.complex128)
    for t, s in enumerate(waves):
        s = np.asarray(s, np.complex128)
        row_fn = _row_python if N * min(len(s), N) <= 20000 else _row_numpy
        for r in range(n_rx):
            for p in range(count):
                z = row_fn(cube[r, first + p], s)
                if code is not None:
                    cr, ci = float(code[t][p].real), float(code[t][p].imag)
                    z = (cr * z.real + ci * z.imag) + 1j * (cr * z.imag - ci * z.real)
                out[t * n_rx + r, p] = z
    return out


def bank_longdouble(cube, waves, first=0, count=None):
    """the correlations without a code, in longdouble"""
    cube = np.asarray(cube, np.complex128)
    n_rx, n_p, N = cube.shape
    count = n_p - first if count is None else count
    out = np.zeros((len(waves) * n_rx, count, N), CR.CLD)
    for t, s in enumerate(waves):
        for r in range(n_rx):
            for p in range(count):
                out[t * n_rx + r, p] = CR.correlate_ref(cube[r, first + p], s)
    return out


def term_magnitudes(cube, waves, first=0, count=None):
    """sum over m of |y[n + m]| |s_t[m]|, the layout of the bank's output, in longdouble"""
    mag = np.abs(np.asarray(cube, np.complex128)).astype(np.complex128)
    return bank_longdouble(mag, [np.abs(np.asarray(s, np.complex128)) for s in waves], first, count).real


# ----------------------------------------------------------------------------- the edge shapes (name, n_rx, n_pulses, n_bins, the waveforms' lengths, code, first, count)
# code: None, "ones", "zeros" (TDM: transmitter t sends at the pulses p with p mod n_waves == t), "ramp" (DDMA: e^{2 pi j t p / n_waves} ... scaled)
def cases():
    T = TILE
    out = []
    for nb in (1, T - 1, T, T + 1, 2 * T + 3):                    # bins around the tile; more than one workgroup per row
        out.append(("bins%d" % nb, 1, 2, nb, [5, 3], None, 0, None))
    out.append(("bins_beyond_compress", 1, 1, MAX_BINS + 1, [3], None, 0, None))
    for M in (1, 2, T, T + 1):                                    # lengths around the tile: the staged window's steps
        out.append(("M%d" % M, 1, 2, T + 9, [M], None, 0, None))
    out.append(("M_is_bins", 1, 2, 77, [77], None, 0, None))
    out.append(("M_beyond_bins", 1, 2, 77, [82], "ramp", 0, None))
    out.append(("M_max", 1, 1, 300, [MAX_SAMPLES], None, 0, None))
    for nw in (1, 2, MAX_WAVES):                                  # one waveform, a pair, every group size and a full last group
        for n_rx in (1, 4):
            out.append(("waves%d_rx%d" % (nw, n_rx), n_rx, 3, 70, [6 + (t % 5) for t in range(nw)], "ramp" if nw > 1 else None, 0, None))
    out.append(("waves5_partial_group", 2, 2, 40, [4, 9, 2, 7, 5], "ones", 0, None))
    # enough workgroups for the larger groups (the plan halves the group while the grid has fewer than 1 024 workgroups; GROUPS below):
    # four full groups of four; a group of four of mixed lengths and a last group of one; groups of two, the last of one
    out.append(("group4_waves16", 4, 64, 20, [3 + (t % 7) for t in range(16)], "ramp", 0, None))
    out.append(("group4_waves5", 4, 128, 20, [1, 7, 30, 2, 5], None, 0, None))
    out.append(("group2_waves3", 4, 128, 20, [6, 2, 9], "ramp", 0, None))
    out.append(("mixed_lengths", 2, 2, 310, [1, 7, 300], "zeros", 0, None))
    out.append(("row_range", 3, 6, 90, [11, 4], "ramp", 2, 3))
    out.append(("code_ones", 2, 4, 33, [8, 8], "ones", 0, None))
    out.append(("code_zeros", 2, 4, 33, [8, 8], "zeros", 1, 3))
    return out


# the waveforms a thread holds in the cases named for it (tests/test_mimo_host.py holds the plan to this)
GROUPS = {"group4_waves16": 4, "group4_waves5": 4, "group2_waves3": 2, "waves16_rx4": 1, "bins1": 1}


def case_input(name, n_rx, n_p, N, lengths, code, first, count):
    """(cube, waves, code table): seeded by the name; the rows outside the span are NaN -- never read"""
    rng = np.random.default_rng(sum(ord(c) for c in name) + 1000 * N)
    count = n_p - first if count is None else count
    cube = random_complex(rng, (n_rx, n_p, N))
    cube[:, :first] = np.nan; cube[:, first + count:] = np.nan
    waves = [random_complex(rng, M) for M in lengths]
    nw = len(lengths)
    t, p = np.meshgrid(np.arange(nw), np.arange(count), indexing="ij")
    table = {None: None, "ones": np.ones((nw, count), np.complex128), "zeros": (p % nw == t).astype(np.complex128),
             "ramp": (0.5 + 0.25 * t) * np.exp(2j * np.pi * t * p / max(nw, 2) + 0.3j)}[code]
    return cube, waves, table
