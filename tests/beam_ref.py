"""What tests/test_beam_host.py and tests/test_gpu_beam.py share: the plain-Python restatement of the beamformer's tree
(include/rts_amd.h: RtsBeamParams -- Python floats never contract), seeded inputs, and the whole-chain scenario with the
parameters that were fixed by running the host chain on the CPU."""
import math

import numpy as np


# ----------------------------------------------------------------------------- the tree, literally
def term(w, z):
    """conj(w) z = (wr zr + wi zi, wr zi - wi zr)"""
    wr, wi, zr, zi = float(w.real), float(w.imag), float(z.real), float(z.imag)
    return wr * zr + wi * zi, wr * zi - wi * zr


def beam_restated(inp, w, first, count):
    """y[b][row][bin] = the sum of term(b, rx) over ascending rx, the rx = 0 term the start value; complex [n_beams][count][n_bins]"""
    n_rx, _, nb = inp.shape
    out = np.zeros((w.shape[0], count, nb), np.complex128)
    for b in range(w.shape[0]):
        for j in range(count):
            for n in range(nb):
                yr, yi = term(w[b, 0], inp[0, first + j, n])
                for r in range(1, n_rx):
                    tr, ti = term(w[b, r], inp[r, first + j, n])
                    yr, yi = yr + tr, yi + ti
                out[b, j, n] = complex(yr, yi)
    return out


def power_restated(y):
    """re re + im im with Python floats (numpy's abs ** 2 rounds differently)"""
    flat = [float(v.real) * float(v.real) + float(v.imag) * float(v.imag) for v in y.ravel()]
    return np.array(flat, np.float64).reshape(y.shape)


def delta_restated(pm, p0, pp):
    """the log-parabola of the detection records: the vertex offset in [-0.5, 0.5], 0 when it is not a peak of positive powers"""
    if not (pm > 0.0 and p0 > 0.0 and pp > 0.0):
        return 0.0
    lm, l0, lp = math.log(pm), math.log(p0), math.log(pp)
    den = lm - 2.0 * l0 + lp
    if not den < 0.0:
        return 0.0
    return min(0.5, max(-0.5, 0.5 * (lm - lp) / den))


def peak_restated(P, delta=delta_restated):
    """(P*, coordinate) of powers [n_beams][...]: the lowest beam that attains the largest power, the offset 0 at the first and last beam"""
    nbm = P.shape[0]
    out = np.zeros(P.shape[1:] + (2,), np.float64)
    for idx in np.ndindex(*P.shape[1:]):
        col = [float(P[(b,) + idx]) for b in range(nbm)]
        best = max(col)
        b = col.index(best)
        off = 0.0 if b == 0 or b == nbm - 1 else delta(col[b - 1], col[b], col[b + 1])
        out[idx] = (best, float(b) + off)
    return out


def random_complex(rng, shape):
    return rng.standard_normal(shape) + 1j * rng.standard_normal(shape)


# ----------------------------------------------------------------------------- plane waves on an array
C0 = 299792458.0


def direction(az, el=0.0):
    return np.array([math.cos(el) * math.cos(az), math.cos(el) * math.sin(az), math.sin(el)])


def line_array(n, wavelength):
    """n elements half a wavelength apart along y, centred on the origin"""
    pos = np.zeros((n, 3))
    pos[:, 1] = (np.arange(n) - (n - 1) / 2.0) * wavelength / 2.0
    return pos


def planar_array(wavelength):
    """3 x 3 elements half a wavelength apart in the y-z plane"""
    return np.array([(0.0, (i - 1) * wavelength / 2.0, (k - 1) * wavelength / 2.0) for i in range(3) for k in range(3)])


def snapshot(pos, az, el, fc, amp=1.0, tau0=1.0e-6):
    """z[rx] = A e^{-2 pi j fc tau_rx}, tau_rx = tau0 - (u0 . p_rx) / c: the cube's phase convention"""
    tau = tau0 - pos @ direction(az, el) / C0
    return amp * np.exp(-2j * np.pi * fc * tau)


# ----------------------------------------------------------------------------- the whole chain (tests 5 of both files)
# 8 elements on a half-wavelength line, 32 pulses, 96 bins; two plane-wave point targets, each in one range bin with a slow-time
# phase ramp of a whole number of Doppler bins; unit noise per element.  The weak target is 10 dB below the per-element noise: a
# single element's Doppler map holds it 5 dB above the noise (gain 32), a beam's 14 dB (gain 8 x 32).  Amplitudes, pfa and seed were
# fixed by running the host chain (rts_noise_eval -> rts_beamform_eval -> rts_stft_eval -> rts_cfar_os_eval) on the CPU until both
# targets are detected in their beams and the weak one in no single element (tests/test_beam_host.py keeps that run as a test).
CHAIN = dict(n_rx=8, n_pulses=32, n_bins=96, wavelength=0.03, noise_power=1.0, seed=2026, pfa=1.0e-5, guard=(1, 1), train=(6, 3),
             fan=np.linspace(-math.pi / 3, math.pi / 3, 17),
             targets=[dict(beam=11, doppler_bin=5, range_bin=30, power=4.0), dict(beam=4, doppler_bin=27, range_bin=61, power=0.1)])


def chain_geometry():
    wl = CHAIN["wavelength"]
    pos = line_array(CHAIN["n_rx"], wl)
    directions = np.stack([CHAIN["fan"], np.zeros(17)], axis=1)
    return pos, directions, C0 / wl


def chain_clean_cube():
    """the targets alone, complex [n_rx][n_pulses][n_bins]"""
    pos, directions, fc = chain_geometry()
    n_rx, n_p, nb = CHAIN["n_rx"], CHAIN["n_pulses"], CHAIN["n_bins"]
    cube = np.zeros((n_rx, n_p, nb), np.complex128)
    ramp = np.arange(n_p) / n_p
    for t in CHAIN["targets"]:
        az = float(directions[t["beam"], 0])
        z = snapshot(pos, az, 0.0, fc, math.sqrt(t["power"]))
        cube[:, :, t["range_bin"]] += z[:, None] * np.exp(2j * np.pi * t["doppler_bin"] * ramp)[None, :]
    return cube


def chain_host(rts):
    """the host chain: (noisy cube, weights, beams [17][32][96], detections on the beams, detections on the elements)"""
    pos, directions, _ = chain_geometry()
    n_rx, n_p, nb = CHAIN["n_rx"], CHAIN["n_pulses"], CHAIN["n_bins"]
    cube = chain_clean_cube() + rts.noise_eval(CHAIN["seed"], np.arange(n_rx * n_p * nb, dtype=np.uint64), CHAIN["noise_power"]).reshape(n_rx, n_p, nb)
    w = rts.steering(pos, directions, CHAIN["wavelength"])
    beams = rts.beamform_eval(cube, w)
    det = chain_detect_host(rts, beams)
    return cube, w, beams, det, chain_detect_host(rts, cube)


def chain_detect_host(rts, cube):
    """slow-time transform (rts_stft_eval: one frame of every pulse, no taper -- the Doppler map's tree) and OS-CFAR with the local-maximum rule"""
    n, n_p, nb = cube.shape
    dmap = rts.stft_eval(cube, n_p, 1, n_p)[:, 0]                                 # [n][n_fft][n_bins]
    return rts.cfar_os_eval(dmap, CHAIN["guard"], CHAIN["train"], None, pfa=CHAIN["pfa"], local_max=True)


def cells(det):
    return {(int(d["rx"]), int(d["doppler_bin"]), int(d["range_bin"])) for d in det}


def chain_target_cells():
    return [(t["beam"], t["doppler_bin"], t["range_bin"]) for t in CHAIN["targets"]]
