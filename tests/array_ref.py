"""What tests/test_array_chain_host.py and tests/test_gpu_array_chain.py share: the one scene in which the ray tracer itself makes the
cube of a receive array -- a tilted plate that closes on the radar, an eight-element half-wavelength line in its specular direction --
and the chain of the array families on that cube through the library's own host evaluators, with the figures the conditions of both
test files are stated on.

The recipe.  A ray is delivered to ONE receiver (the reference's behaviour, quirk 4, tests/test_capture_branches.py): capture spheres
that overlap -- and those of elements half a wavelength apart always do -- hand every ray to the last receiver of the list.  So a
dense array is traced one launch per element, the element alone in the receiver list, and its one-receiver cube is attached at its
slab of a shared [n_rx][n_pulses][n_bins] buffer.  element_launches() below is that loop on the oracle.

Geometry.  The plate's normal is (-cos psi, -sin psi, 0); the transmitter's rays travel along +x and leave the plate along
(-cos 2 psi, -sin 2 psi, 0).  The array's centre lies 1000 m down that line, so the wave reaches it FROM az = 2 psi, el = 0, the
direction rts_steering_make's rows are made for.  Moving the plate by delta along x changes the two-way length by
delta (1 + cos 2 psi); delta = -f lambda / (1 + cos 2 psi) per pulse shortens it by f wavelengths per pulse: the cube's phase
-2 pi fc tau then ADVANCES by f cycles per pulse, a Doppler frequency of +f for a closing target (tests/test_gpu_detect.py)."""
import functools
import math

import numpy as np

import cube_ref as R
from rts_amd import scenes

CS, FC = scenes.C0, scenes.FC
WL = CS / FC
PSI = math.radians(10.0)
AZ = 2.0 * PSI                                   # the wave's direction of arrival at the array
F_TARGET = 0.2                                   # cycles per pulse
N_RX, N_PULSES, N_BINS, DT, BIN = 8, 16, 32, 5.0e-9, 10
RADIUS, W = 200.0, 22
RAYS = 2200                                      # received rays of each element at each pulse
GRID_DEG = np.arange(-120, 121) * 0.5            # -60 .. 60 degrees in steps of 0.5
GRID_STEP = 0.5
TAPS = 4
DOPPLERS = np.arange(-10, 10) * 0.05             # -0.5 .. 0.45 cycles per pulse
SNR, JNR = 100.0, 1000.0                         # the target cell over the noise, the jammer over the target cell
JAMMER_AZ = math.radians(-25.0)
NOISE_SEED, JAMMER_SEED, PATCH_SEED = 20261, 20262, 20263
METHODS = ("bartlett", "capon", "music")


# ----------------------------------------------------------------------------- the scene
def plate():
    v, t, n = scenes.plate_mesh(10.0)
    c, s = math.cos(PSI), math.sin(PSI)
    Rz = np.array([[c, -s, 0.0], [s, c, 0.0], [0.0, 0.0, 1.0]])
    return dict(tris=t, verts=v @ Rz.T, normals=n @ Rz.T, refl_coeff=0.9, refr_index=1.0)


def motion(pulse):
    delta = -F_TARGET * WL / (1.0 + math.cos(2.0 * PSI))
    return [dict(position=(delta * pulse, 0.0, 0.0), velocity=(0.0, 0.0, 0.0))]


def positions():
    """the element positions [8][3]: half a wavelength apart along y about the centre 1000 (-cos 2 psi, -sin 2 psi, 0)"""
    centre = 1000.0 * np.array([-math.cos(AZ), -math.sin(AZ), 0.0])
    return centre[None, :] + (np.arange(N_RX) - (N_RX - 1) / 2.0)[:, None] * np.array([0.0, WL / 2.0, 0.0])[None, :]


def receivers(rts):
    """one capture sphere per element, every one with the SAME look angles (rts_rx_sphere places the sphere by cosf / sinf of them:
    angles of their own would move the spheres apart by fractions of a wavelength)"""
    return [rts.rx_sphere(p, AZ, 0.0, RADIUS, math.pi / 2, math.pi / 2) for p in positions()]


def spec(rts, elements=None):
    """the scene in tests/helpers.py's form with the receivers `elements` (default: all eight in one list -- what does NOT work)"""
    rx = receivers(rts)
    return dict(name="array-chain", W=W, max_refl=1, smooth=True, n_pulses=N_PULSES, meshes=[plate()], motion=motion(0),
                tx=dict(origin=(-1000.0, 0.0, 0.0), span=(0.02, 0.02, 0.0), dir=(0.0, 0.0)),
                rx=rx if elements is None else [rx[k] for k in elements], carrier=FC, c=CS)


def oracle_received(rts, oracle, elements, pulse):
    """the finalised received records of one oracle launch with the receivers `elements`"""
    import helpers as H
    o = H.oracle_trace(oracle, spec(rts, elements), motion=motion(pulse))
    rx, _, _ = oracle.filter_finalise(o["results"], o["path"], [1.0], WL, 1.0, 1.0, FC, CS)
    return rx


@functools.lru_cache(maxsize=None)
def element_launches(rts, oracle):
    """one launch per element and pulse on the oracle: {(element, pulse): received records}"""
    return {(k, m): oracle_received(rts, oracle, [k], m) for k in range(N_RX) for m in range(N_PULSES)}


def contributions(records, element):
    """cube_ref.contribs_rays of a one-receiver launch, delivered to `element`"""
    return [(element, a, tau, f) for (_rx, a, tau, f) in R.contribs_rays(records, CS, FC)]


@functools.lru_cache(maxsize=None)
def traced(rts, oracle):
    """(the clean cube complex128 [8][16][32], t0, ray counts [8][16]): every launch's rays accumulated as impulses, t0 from the
    smallest traced delay so that every return falls in bin BIN (the delays span about 1.4 ns of the bin's 5)"""
    launches = element_launches(rts, oracle)
    contribs = {key: contributions(rec, key[0]) for key, rec in launches.items()}
    taus = np.array([c[2] for cs in contribs.values() for c in cs])
    assert taus.max() - taus.min() < 0.5 * DT, (taus.min(), taus.max())
    t0 = float(taus.min()) - (BIN + 0.25) * DT
    cube = np.zeros((N_RX, N_PULSES, N_BINS), R.CLD)
    for (k, m), cs in contribs.items():
        R.accumulate_ref(cube, m, cs, t0, DT)
    cube = R.to_double(cube)
    assert np.count_nonzero(cube[:, :, BIN]) == N_RX * N_PULSES and np.count_nonzero(cube) == N_RX * N_PULSES
    counts = np.array([[len(launches[(k, m)]) for m in range(N_PULSES)] for k in range(N_RX)])
    return cube, t0, counts


# ----------------------------------------------------------------------------- the tables of the chain
def directions(az):
    az = np.atleast_1d(np.asarray(az, np.float64))
    return np.stack([az, np.zeros(len(az))], axis=1)


def grid_table(rts):
    """steering rows [241][8] over the grid"""
    return rts.steering(positions(), directions(np.radians(GRID_DEG)), WL)


def steering_at(rts, az):
    return rts.steering(positions(), directions(az), WL)


def filter_bank(rts):
    """space-time steering [2 * 20][4 * 8]: beam 0 at +az, beam 1 at -az, every Doppler of DOPPLERS"""
    return rts.st_steering(steering_at(rts, [AZ, -AZ]), DOPPLERS, TAPS)


def target_power(clean):
    """the mean power of the target's cell over elements and pulses"""
    return float(np.mean(np.abs(clean[:, :, BIN]) ** 2))


def noise_power(clean):
    return target_power(clean) / SNR


def noise(rts, power):
    n = N_RX * N_PULSES * N_BINS
    return rts.noise_eval(NOISE_SEED, np.arange(n, dtype=np.uint64), power).reshape(N_RX, N_PULSES, N_BINS)


def jammer(rts, clean):
    """keyword arguments of sources_eval / cube_add_sources: a noise jammer (rho = 0) at -25 degrees in every bin"""
    return dict(spatial=steering_at(rts, [JAMMER_AZ]), power=[JNR * target_power(clean)], doppler=[0.0], rho=[0.0], seed=JAMMER_SEED)


def patch(rts, clean, doppler):
    """a fully correlated patch (rho = 1) at the target's direction and the Doppler frequency `doppler`"""
    return dict(spatial=steering_at(rts, [AZ]), power=[target_power(clean)], doppler=[doppler], rho=[1.0], seed=PATCH_SEED)


def doa_train():
    return dict(first_bin=BIN, n_bins=1)


def doa_host(rts, cube, method, loading):
    """covariance_eval over the target's bin -> eig_eval -> doa_weights -> doa_scan_eval over the grid (MUSIC: one source)"""
    values, vectors = rts.eig_eval(rts.covariance_eval(cube, **doa_train()))
    first, g, inverse = rts.doa_weights(method, values, 1 if method == "music" else 0, loading)
    return rts.doa_scan_eval(vectors[first:first + len(g)], g, grid_table(rts), inverse)


def mvdr_host(rts, cube, loading):
    """(covariance without the target's bin, the weights of the beam at +az [1][8], the beam [1][16][32])"""
    cov = rts.covariance_eval(cube, skip=(BIN, 1))
    w = rts.mvdr_eval(cov, steering_at(rts, [AZ]), loading)
    return cov, w, rts.beamform_eval(cube, w)


# ----------------------------------------------------------------------------- the figures of the conditions
def grid_index(deg):
    return int(np.argmin(np.abs(GRID_DEG - deg)))


def spectrum_figures(spectrum):
    """(the peak's direction in degrees, the spectrum at -20 degrees over its peak)"""
    s = np.asarray(spectrum, np.float64)
    return float(GRID_DEG[int(np.argmax(s))]), float(s[grid_index(-math.degrees(AZ))] / s.max())


def beam_figures(cube, beams):
    """of the grid's beams [241][16][32] of `cube`: (the peak's direction, its power over (sum_k |z_k|)^2, the power at -20 degrees
    over the peak) -- powers of the target's bin summed over the pulses"""
    p = np.sum(np.abs(beams[:, :, BIN]) ** 2, axis=1)
    full = float(np.sum(np.sum(np.abs(cube[:, :, BIN]), axis=0) ** 2))
    direction, mirror = spectrum_figures(p)
    return direction, float(p.max() / full), mirror


def bank_table(y):
    """the filter bank's output [40][13][32] as powers [2][20] of the target's bin summed over the output pulses"""
    return np.sum(np.abs(y[:, :, BIN]) ** 2, axis=1).reshape(2, len(DOPPLERS))


def doppler_index(f):
    return int(np.argmin(np.abs(DOPPLERS - f)))


def bank_figures(table):
    """((beam, Doppler) of the peak, the power at (+az, -f) over the peak, the power at (-az, +f) over the peak)"""
    b, d = np.unravel_index(int(np.argmax(table)), table.shape)
    return (int(b), float(DOPPLERS[d])), float(table[0, doppler_index(-F_TARGET)] / table.max()), float(table[1, doppler_index(F_TARGET)] / table.max())


def db(x):
    return 10.0 * math.log10(x)


def cell_ratio_db(beam):
    """the target's bin over the mean of the other bins, powers of a beam [16][32] averaged over the pulses, in dB"""
    p = np.mean(np.abs(beam) ** 2, axis=0)
    return db(p[BIN] / np.mean(np.delete(p, BIN)))


def mvdr_figures(rts, clean, cube, w, beam):
    """of the MVDR weights w [1][8] and their beam [1][16][32] of the jammed cube: (|w^H s - 1|, the cell ratio of the MVDR beam in dB,
    that of the conventional beam s / 8, the MVDR beam's target-cell power over the clean coherent sum |s^H z / 8|^2, |w^H s_j|,
    |s^H s_j| / 8)"""
    s = steering_at(rts, [AZ])[0]; sj = steering_at(rts, [JAMMER_AZ])[0]
    conv = rts.beamform_eval(cube, s[None, :] / N_RX)
    coherent = np.mean(np.abs(np.einsum("k,kp->p", s.conj() / N_RX, clean[:, :, BIN])) ** 2)
    return (float(abs(np.vdot(w[0], s) - 1.0)), cell_ratio_db(beam[0]), cell_ratio_db(conv[0]),
            float(np.mean(np.abs(beam[0, :, BIN]) ** 2) / coherent), float(abs(np.vdot(w[0], sj))), float(abs(np.vdot(s, sj)) / N_RX))


def check_beam(fig, what="the conventional beam"):
    """b: (the peak's direction, its power over (sum_k |z_k|)^2, the power at -20 degrees over the peak)"""
    print("%s: peak at %.1f degrees, %.5f of (sum |z_k|)^2, %.5f of the peak at %.1f degrees" % ((what,) + tuple(fig) + (-math.degrees(AZ),)))
    direction, gain, mirror = fig
    assert abs(direction - math.degrees(AZ)) <= GRID_STEP + 1e-9 and gain >= 0.99 and mirror <= 0.1, (what, fig)


def check_spectrum(fig, method):
    """c: (the peak's direction, the spectrum at -20 degrees over the peak)"""
    print("%s: peak at %.1f degrees, %.5f of the peak at %.1f degrees" % ((method,) + tuple(fig) + (-math.degrees(AZ),)))
    direction, mirror = fig
    assert abs(direction - math.degrees(AZ)) <= GRID_STEP + 1e-9 and mirror <= 0.1, (method, fig)


def check_bank(fig):
    """d: the filter bank on the traced target: the peak at (+az, +f), a positive frequency for a closing target"""
    (beam, f), other_sign, other_side = fig
    print("filter bank: peak at (beam %d, %+.2f); %.4f of it at (+az, %+.2f), %.4f at (-az, %+.2f)" % (beam, f, other_sign, -F_TARGET, other_side, F_TARGET))
    assert beam == 0 and abs(f - F_TARGET) < 1e-9, fig
    assert other_sign <= 0.25 and other_side <= 0.1, fig


def check_patch(fig, doppler):
    """e: an injected patch peaks at its own sign, in the beam at +az"""
    (beam, f), _, _ = fig
    print("patch of doppler %+.2f: peak at (beam %d, %+.2f)" % (doppler, beam, f))
    assert beam == 0 and abs(f - doppler) < 1e-9, (doppler, fig)


def check_mvdr(fig):
    """f: MVDR against the jammer"""
    print("mvdr: |w^H s - 1| = %.3g; target cell over the others %.1f dB (conventional %.1f dB); cell power %.4f of the clean coherent sum; "
          "|w^H s_j| = %.3g (conventional %.3g)" % tuple(fig))
    distortion, ratio, ratio_conv, cell, toward_jammer, _ = fig
    assert distortion <= 1e-12 and ratio >= 20.0 and ratio_conv <= 10.0, fig
    assert abs(cell - 1.0) <= 0.1 and toward_jammer <= 1e-3, fig


def assert_conditions(fig):
    """the conditions b .. f on host_chain's figures; every figure is printed before it is held to its condition"""
    check_beam(fig["beam_clean"], "the conventional beam of the cube as traced")
    check_beam(fig["beam"], "the conventional beam of the noisy cube")
    for method in METHODS:
        check_spectrum(fig[method], method)
    check_bank(fig["bank"])
    for sign in (1.0, -1.0):
        check_patch(fig["patch%+.1f" % (sign * F_TARGET)], sign * F_TARGET)
    check_mvdr(fig["mvdr"])


# ----------------------------------------------------------------------------- the host chain
@functools.lru_cache(maxsize=None)
def host_chain(rts, oracle):
    """everything on the host: dict(clean, t0, counts, noise_power, noisy, jammed, figures)"""
    clean, t0, counts = traced(rts, oracle)
    npow = noise_power(clean)
    noisy = clean + noise(rts, npow)
    fig = {}
    fig["beam_clean"] = beam_figures(clean, rts.beamform_eval(clean, grid_table(rts)))
    fig["beam"] = beam_figures(noisy, rts.beamform_eval(noisy, grid_table(rts)))
    for method in METHODS:
        fig[method] = spectrum_figures(doa_host(rts, noisy, method, npow))
    bank = filter_bank(rts)
    fig["bank"] = bank_figures(bank_table(rts.st_apply_eval(noisy, bank, TAPS)))
    for sign in (1.0, -1.0):
        alone = rts.sources_eval(np.zeros_like(clean), **patch(rts, clean, sign * F_TARGET))
        fig["patch%+.1f" % (sign * F_TARGET)] = bank_figures(bank_table(rts.st_apply_eval(alone, bank, TAPS)))
    jammed = rts.sources_eval(noisy, **jammer(rts, clean))
    cov, w, beam = mvdr_host(rts, jammed, npow)
    fig["mvdr"] = mvdr_figures(rts, clean, jammed, w, beam)
    return dict(clean=clean, t0=t0, counts=counts, noise_power=npow, noisy=noisy, jammed=jammed, figures=fig)
