"""What tests/test_passive_chain_host.py and tests/test_gpu_passive.py share: ONE small traced passive-radar scenario and its chain.

The scene is tests/locate_chain_ref.py's (imported, not edited): a transmitter of opportunity, three faceted bodies that move a few
millimetres per pulse, capture spheres at its first three receiver positions: the surveillance receivers 0 .. 2 of a cube
[4][16][512].  Receiver 3 of the cube is the REFERENCE slot: no ray reaches it, the caller writes it.  The launch lattice is W = 50
(a quarter of the rays of the localisation chain per facet: enough for a coherent return).

Per pulse a fresh noise-like segment of M = 448 unit-power complex Gaussian samples (one seeded generator) is set as the waveform
(taps 1: sample-and-hold, so a delay d lands the segment on the grid at lag floor(d)) and the pulse's rays are rendered with Doppler.
The cube's first delay is LAG0 = 16 cells earlier than the localisation chain's, which keeps every return in one cell and puts every
echo at a lag >= 19 > K = 8: the cancellation does not see it whatever its Doppler (rts_passive.h: the notch covers the lags below K).
Receiver noise (rts_cube_add_noise, NOISE_POWER per sample) is added to the whole cube -- where thermal noise enters a receiver:
before the cancellation.  Then the caller's terms, written through the caller-owned cube:
  * the reference row of pulse p: the segment on grid from bin 0 (this also replaces the noise there: a clean reference);
  * on each surveillance row the direct signal DIRECT[r] x seg at lag 0 and static clutter CLUTTER[r][i] x seg at the lags
    CLUTTER_LAGS = (2, 5), the same complex gains at every pulse.

The amplitudes.  Measured on the numpy restatement alone (tests/passive_ref.py; figures in tests/test_passive_chain_host.py): the
nine echoes have 0.76e-6 .. 2.0e-6 per sample.  The integration gain of N P = 448 x 16 samples is 38.6 dB, so a direct signal more
than that above an echo buries it under its own correlation sidelobes.  DIRECT = 0.03 is 83 .. 92 dB above the echoes, CLUTTER =
0.003 .. 0.006 some 63 .. 78 dB; NOISE_POWER = 1e-12 puts each echo -2 .. +6 dB against the noise per sample, 36 .. 45 dB after
integration.

The chain: [cancel ->] xcorr at lags 0 .. 63 -> attach the result as a cube of 64 bins -> 16-point Doppler -> OS-CFAR with range-only
training (the localisation chain's detector) -> detections."""
import functools
import math

import numpy as np

import cube_ref as CR
import locate_chain_ref as LC
import passive_ref as P

CS, FC, WL, DT, PRI = LC.CS, LC.FC, LC.WL, LC.DT, LC.PRI
N_SURV, REF, N_RX, N_PULSES, N_BINS, M = 3, 3, 4, 16, 512, 448
W, LAG0, K, N_LAGS = 50, 16, 8, 64
T0 = LC.T0 - LAG0 * DT
SEG_SEED, NOISE_POWER, NOISE_SEED = 90210, 1.0e-12, 31337
DIRECT = 0.03 * np.exp(1j * np.array([0.3, -1.1, 2.0]))
CLUTTER_LAGS = (2, 5)
CLUTTER = np.array([[0.006 * np.exp(0.7j), 0.003 * np.exp(-2.1j)], [0.004 * np.exp(1.9j), 0.005 * np.exp(0.4j)], [0.003 * np.exp(-0.5j), 0.006 * np.exp(2.6j)]])
CFAR = dict(guard=(1, 0), train=(4, 0), rank=6, alpha=200.0, local_max=True, pri=PRI)


def spec(rts):
    s = LC.spec(rts)
    return dict(s, name="passive-chain", W=W, rx=s["rx"][:N_SURV])


@functools.lru_cache(maxsize=None)
def segments():
    """[N_PULSES][M]: the transmitter's signal during each coherent row"""
    rng = np.random.default_rng(SEG_SEED)
    return P.random_complex(rng, (N_PULSES, M)) / math.sqrt(2.0)


@functools.lru_cache(maxsize=None)
def oracle_launches(rts, oracle):
    import helpers as H
    out = []
    for m in range(N_PULSES):
        o = H.oracle_trace(oracle, spec(rts), motion=LC.motion(m))
        rec, _, _ = oracle.filter_finalise(o["results"], o["path"], [1.0, 1.0, 1.0], WL, 1.0, 1.0, FC, CS)
        out.append(rec)
    return out


def render_numpy(rec, seg):
    """the render with taps 1 and Doppler (include/rts_amd.h: y[n] += a s(n - d) e^{j 2 pi f (n - d) dt}, s(x) = s[ceil(x)]) of one
    pulse's received records, in float64 numpy, a ray at a time: [N_SURV][N_BINS]"""
    rows = np.zeros((N_SURV, N_BINS), np.complex128)
    n = np.arange(N_BINS, dtype=np.float64)
    for rx, a, tau, f in CR.contribs_rays(rec, CS, FC):
        if not 0 <= rx < N_SURV:
            continue
        x = n - CR.start_of(tau, T0, DT)
        m = np.ceil(x).astype(np.int64)
        ok = (m >= 0) & (m < M)
        rows[rx, ok] += complex(a) * seg[m[ok]] * np.exp(2j * np.pi * f * DT * x[ok])
    return rows


def noise(rts):
    n = N_RX * N_PULSES * N_BINS
    return rts.noise_eval(NOISE_SEED, np.arange(n, dtype=np.uint64), NOISE_POWER).reshape(N_RX, N_PULSES, N_BINS)


def reference_rows():
    ref = np.zeros((N_PULSES, N_BINS), np.complex128)
    ref[:, :M] = segments()
    return ref


def caller_terms():
    """[N_SURV][N_PULSES][N_BINS]: the direct signal and the static clutter the caller adds to the surveillance rows"""
    ref = reference_rows()
    out = np.zeros((N_SURV, N_PULSES, N_BINS), np.complex128)
    for r in range(N_SURV):
        out[r] += DIRECT[r] * ref
        for lag, g in zip(CLUTTER_LAGS, CLUTTER[r]):
            out[r, :, lag:] += g * ref[:, :N_BINS - lag]
    return out


def assemble(echoes, noise_cube):
    """echoes [N_SURV][N_PULSES][N_BINS] (the rendered rows) -> the cube the chain works on, in the order the device test uses: the
    noise on the rendered cube, then the reference rows written, then the caller's terms added to the surveillance rows"""
    cube = np.zeros((N_RX, N_PULSES, N_BINS), np.complex128)
    cube[:N_SURV] = echoes
    cube = cube + noise_cube
    cube[REF] = reference_rows()
    cube[:N_SURV] = cube[:N_SURV] + caller_terms()
    return cube


def expected_cells(echoes):
    """per (receiver, body) the (Doppler bin, lag) of its echo: the largest cell of the numpy restatement's map of the ECHOES ALONE
    near the lag geometry predicts"""
    cube = np.zeros((N_RX, N_PULSES, N_BINS), np.complex128)
    cube[:N_SURV] = echoes; cube[REF] = reference_rows()
    zmap = np.abs(np.fft.fft(P.xcorr_numpy(cube, REF, N_LAGS), axis=1)) ** 2
    cells = {}
    for r in range(N_SURV):
        for s in range(3):
            lag = (LC.true_range_sum(LC.centre(s, 7.5), r) - 0.5 * (LC.SHORT[0] + LC.SHORT[1])) / CS / DT - T0 / DT
            lo = max(int(math.floor(lag)) - 1, 0)
            win = zmap[r, :, lo:lo + 3]
            kd, kl = np.unravel_index(np.argmax(win), win.shape)
            cells[(r, s)] = (int(kd), lo + int(kl), float(win[kd, kl]))
    return cells


def detect_host(rts, z):
    """z: the correlation [N_RX][N_PULSES][N_LAGS] -> (the map's power, the detections) through the library's host evaluators"""
    zmap = CR.to_double(CR.dft_ref(z, N_PULSES))
    return zmap, rts.cfar_os_eval(zmap, t0=0.0, dt=DT, **CFAR)


def reported(det, r, cell):
    return bool(np.any((det["rx"] == r) & (det["doppler_bin"] == cell[0]) & (det["range_bin"] == cell[1])))


@functools.lru_cache(maxsize=None)
def host_chain(rts, oracle):
    launches = oracle_launches(rts, oracle)
    seg = segments()
    echoes = np.stack([render_numpy(rec, seg[m]) for m, rec in enumerate(launches)], axis=1)
    cube = assemble(echoes, noise(rts))
    raw_map, raw_det = detect_host(rts, rts.xcorr_eval(cube, REF, N_LAGS))
    clean, coeffs, info = rts.cancel_eval(cube, REF, K)
    map_, det = detect_host(rts, rts.xcorr_eval(clean, REF, N_LAGS))
    return dict(echoes=echoes, cube=cube, raw_map=raw_map, raw_det=raw_det, clean=clean, coeffs=coeffs, info=info, map=map_, det=det, cells=expected_cells(echoes))


CLUTTER_CELLS = (0,) + CLUTTER_LAGS      # the lags that hold the direct signal and the clutter, at Doppler bin 0


def lag_power(zmap):
    """[N_SURV][len(CLUTTER_CELLS)]: the power of a map [rx][Doppler][lag] at the clutter's lags, summed over the Doppler bins"""
    p = np.abs(np.asarray(zmap)) ** 2
    return np.array([[float(p[r, :, lag].sum()) for lag in CLUTTER_CELLS] for r in range(N_SURV)])


def numpy_factors(cube):
    """by how much the numpy restatement (np.linalg.lstsq per block, shifted products, np.fft) brings the clutter lags' power down"""
    raw = np.fft.fft(P.xcorr_numpy(cube, REF, N_LAGS), axis=1)
    clean, _ = P.cancel_numpy(cube, REF, K)
    return lag_power(raw) / lag_power(np.fft.fft(P.xcorr_numpy(clean, REF, N_LAGS), axis=1))


def check_chain(c, show=print):
    """a: without the cancellation no target cell is reported; b: with it every one is, the clutter cells at Doppler 0 are nulled
    (a least-squares residual is orthogonal to every lagged copy: what is left there is rounding, held to 1e-20 of the cell before)
    and the clutter lags' power over all Doppler bins is down by the numpy restatement's factor.  That factor compares noise floors:
    the coefficients' error, K eps cond = 1e-13 relative, moves a 0.03 clutter amplitude by 3e-15 against a noise of 1e-6 per sample,
    3e-9 of the floor; the bound is 1e-6."""
    raw, clean = np.abs(c["raw_map"]) ** 2, np.abs(c["map"]) ** 2
    for (r, s), cell in sorted(c["cells"].items()):
        kd, kl = cell[:2]
        ring = sorted(clean[r, kd, j] for j in range(kl - 5, kl + 6) if abs(j - kl) > 1)[5] * CFAR["alpha"]
        ring_raw = sorted(raw[r, kd, j] for j in range(kl - 5, kl + 6) if abs(j - kl) > 1)[5] * CFAR["alpha"]
        show("receiver %d body %d, cell (%d, %d): without %.3g of its threshold, with %.3g" % (r, s, kd, kl, raw[r, kd, kl] / ring_raw, clean[r, kd, kl] / ring))
        assert not reported(c["raw_det"], r, cell), (r, s, cell)
        assert reported(c["det"], r, cell), (r, s, cell)
    for r in range(N_SURV):
        for lag in CLUTTER_CELLS:
            assert clean[r, 0, lag] <= 1e-20 * raw[r, 0, lag], (r, lag, clean[r, 0, lag], raw[r, 0, lag])
    got, want = lag_power(c["raw_map"]) / lag_power(c["map"]), numpy_factors(c["cube"])
    show("clutter lags down by %.1f .. %.1f dB (numpy: %.1f .. %.1f dB)" % (10 * np.log10(got.min()), 10 * np.log10(got.max()), 10 * np.log10(want.min()), 10 * np.log10(want.max())))
    np.testing.assert_allclose(got, want, rtol=1e-6)
    assert np.all(want > 1e3)
