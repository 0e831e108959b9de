"""What tests/test_mimo_chain_host.py and tests/test_gpu_mimo_chain.py share: the one scene in which the ray tracer itself makes the
cube of a MIMO radar -- two transmitters with orthogonal phase codes and four receive elements on one line, a plate facing them --
and the chain render -> matched-filter bank -> virtual array on that cube, with the figures both test files state their conditions on.

The recipe is tests/array_ref.py's: a ray is delivered to ONE receiver, so a dense array is traced one launch per element -- here one
per (transmitter, element, pulse): the transmitter at its own origin, the element alone in the receiver list, the launch rendered
with that transmitter's waveform times its slow-time code into the element's row of ONE cube.  Both transmitters' echoes arrive
together, in the same bins of the same rows.

Geometry.  The tracer is geometric optics: the target is a mirror.  The plate FACES the radar (normal -l, l = +x the line of sight)
and the transmitters and elements lie on one line OBLIQUE to l (direction u, GAMMA from l).  The plate's image of a transmitter moved
by a is moved by a - 2 (a.l) l, so an element at offset o hears transmitter a over the two-way length 2 R - l.(o + a) to first order:
a genuine virtual element at o + a for a wave from l.  (array_ref's plate in its specular direction will not do: there a transverse
transmitter offset drops out of the phase.)  The plate closes by F_TARGET / 2 wavelengths per pulse.

Four elements half a wavelength apart and two transmitters two wavelengths apart give the virtual offsets 0 .. 7 half wavelengths: the
REFERENCE, independent of the bank, is the same scene traced with transmitter 0 alone onto the eight-element half-wavelength line,
rendered with its waveform and compressed.

The capture sphere.  The tracer delivers a ray's length to an element from where the ray ENTERS the element's capture sphere, and
that delivery is exact only for the sphere's own centre line: with the 200 m sphere of array_ref the target cell's amplitude falls by
30 % and its phase turns by 0.13 rad over 10 cm of separation between transmitter and element, which a virtual element (separation
|a - o|) and its physical twin (separation a + o) do not share.  The larger the sphere, the nearer to the plate a ray enters it and
the truer the length: the residual below is 0.127 at 200 m, 0.011 at 600 m, 0.0047 at 950 m (the plate is 1000 m away).  950 m it is.
A transmitter inside a sphere and off its centre also delivers the rays that miss the plate (echoes() below).

The bound of condition (b), measured on the oracle's rays (tests/test_mimo_chain_host.py prints it): after the least-squares common
factor, the eight virtual snapshots of the target cell over the eight pulses differ from the eight physical ones by RESIDUAL_MEASURED
= 0.0047 of their norm.  That is the sum of the codes' cross-talk (exactly orthogonal chips that land in the same bins: rounding
alone), the far-field term (the second order of the lengths, a o sin^2 GAMMA / R: 3 lambda^2 0.88 / 1000 m, 8e-5 wavelengths) and,
the most of it, the sphere's term above.  RESIDUAL_BOUND is that with a margin of a factor 2, so that the last digits of a different
ray set do not trip it."""
import functools
import math

import numpy as np

import array_ref as AR
import cube_ref as CR

CS, FC, WL, DT = AR.CS, AR.FC, AR.WL, AR.DT
GAMMA = math.radians(70.0)
U = np.array([math.cos(GAMMA), math.sin(GAMMA), 0.0])
CENTRE = np.array([-1000.0, 0.0, 0.0])
N_EL, N_TX, N_VIRT, N_PULSES, N_BINS, BIN = 4, 2, 8, 8, 64, 10
F_TARGET = 0.2
RADIUS, W, RAYS = 950.0, AR.W, AR.RAYS
GRID_DEG, GRID_STEP = AR.GRID_DEG, AR.GRID_STEP
M_CHIPS = 16
RESIDUAL_MEASURED = 0.0047
RESIDUAL_BOUND = 2.0 * RESIDUAL_MEASURED


# ----------------------------------------------------------------------------- the radar
def rx_positions():
    return CENTRE[None, :] + (np.arange(N_EL) * WL / 2.0)[:, None] * U[None, :]


def tx_offsets():
    return (np.arange(N_TX) * 2.0 * WL)[:, None] * U[None, :]


def line_positions():
    """the eight-element half-wavelength line of the reference"""
    return CENTRE[None, :] + (np.arange(N_VIRT) * WL / 2.0)[:, None] * U[None, :]


@functools.lru_cache(maxsize=None)
def chips():
    """two rows of the 16 x 16 Hadamard matrix: orthogonal at zero lag"""
    h = np.array([[1.0]])
    while h.shape[0] < M_CHIPS:
        h = np.block([[h, h], [h, -h]])
    return np.stack([h[5], h[10]]).astype(np.complex128)


def slow_code():
    """[2][8]: transmitter 0 sends every pulse as it is, transmitter 1 with alternating sign"""
    return np.stack([np.ones(N_PULSES), (-1.0) ** np.arange(N_PULSES)]).astype(np.complex128)


def waveforms(rts):
    return [rts.Waveform.coded(c, 1, taps=1) for c in chips()]


def sent(t, p):
    """what transmitter t sends at pulse p: its slow-time code times its waveform (the render side has no code of its own)"""
    return slow_code()[t, p] * chips()[t]


# ----------------------------------------------------------------------------- the scene
def plate():
    v, t, n = AR.scenes.plate_mesh(10.0)
    return dict(tris=t, verts=v, normals=n, refl_coeff=0.9, refr_index=1.0)


def motion(pulse):
    return [dict(position=(-F_TARGET * WL / 2.0 * pulse, 0.0, 0.0), velocity=(0.0, 0.0, 0.0))]


def spec(rts, positions, element, t):
    """tests/helpers.py's form: transmitter t at its origin, the element `element` of `positions` alone in the receiver list (every
    sphere with the same look angles, as in array_ref)"""
    origin = CENTRE + tx_offsets()[t]
    rx = rts.rx_sphere(positions[element], 0.0, 0.0, RADIUS, math.pi / 2, math.pi / 2)
    return dict(name="mimo-chain", W=W, max_refl=1, smooth=True, n_pulses=N_PULSES, meshes=[plate()], motion=motion(0),
                tx=dict(origin=tuple(float(x) for x in origin), span=(0.02, 0.02, 0.0), dir=(0.0, 0.0)), rx=[rx], carrier=FC, c=CS)


def oracle_received(rts, oracle, positions, element, t, pulse):
    import helpers as H
    o = H.oracle_trace(oracle, spec(rts, positions, element, t), motion=motion(pulse))
    rx, _, _ = oracle.filter_finalise(o["results"], o["path"], [1.0], WL, 1.0, 1.0, FC, CS)
    return rx


@functools.lru_cache(maxsize=None)
def launches(rts, oracle):
    """{("mimo", t, r, p): records} for the radar and {("line", 0, k, p): records} for the reference"""
    out = {}
    for p in range(N_PULSES):
        for t in range(N_TX):
            for r in range(N_EL):
                out[("mimo", t, r, p)] = oracle_received(rts, oracle, rx_positions(), r, t, p)
        for k in range(N_VIRT):
            out[("line", 0, k, p)] = oracle_received(rts, oracle, line_positions(), k, 0, p)
    return out


def echoes(rec):
    """the records that came off the plate.  A transmitter INSIDE an element's capture sphere and off its centre -- every pair here but
    transmitter 0 with element 0 -- also delivers the rays that miss the plate, straight from the origin with a length of centimetres
    (the reference's behaviour); their delay lies more than a thousand bins before the cube, where every render drops them"""
    return rec[rec["reflDepth"] >= 1]


def render_numpy(rec, s, t0):
    """the render with taps 1 and no Doppler term (include/rts_amd.h: y[n] += a s(n - d), s(x) = s[ceil(x)]) of one launch's received
    records in float64 numpy, all rays at once: one row [N_BINS]"""
    c = CR.contribs_rays(rec, CS, FC)
    a = np.array([complex(x[1]) for x in c]); d = np.array([CR.start_of(x[2], t0, DT) for x in c])
    m = np.ceil(np.arange(N_BINS, dtype=np.float64)[None, :] - d[:, None]).astype(np.int64)
    ok = (m >= 0) & (m < len(s))
    return np.sum(np.where(ok, a[:, None] * s[np.clip(m, 0, len(s) - 1)], 0.0), axis=0)


# ----------------------------------------------------------------------------- the figures
def directions(az):
    return AR.directions(az)


def grid_table(rts, positions):
    return rts.steering(positions, directions(np.radians(GRID_DEG)), WL)


def bartlett(rts, cube, positions):
    """the Bartlett spectrum over the grid: the conventional beams' power in the target's bin summed over the pulses"""
    beams = rts.beamform_eval(cube, grid_table(rts, positions))
    return np.sum(np.abs(beams[:, :, BIN]) ** 2, axis=1)


def peak_and_width(spectrum):
    """(the peak's direction in degrees, the -3 dB width in degrees: the half-power crossings on either side, interpolated linearly)"""
    s = np.asarray(spectrum, np.float64); i = int(np.argmax(s)); half = s[i] / 2.0
    lo = i
    while lo > 0 and s[lo - 1] >= half:
        lo -= 1
    hi = i
    while hi < len(s) - 1 and s[hi + 1] >= half:
        hi += 1
    assert lo > 0 and hi < len(s) - 1, "the main lobe leaves the grid"
    left = GRID_DEG[lo] - GRID_STEP * (s[lo] - half) / (s[lo] - s[lo - 1])
    right = GRID_DEG[hi] + GRID_STEP * (s[hi] - half) / (s[hi] - s[hi + 1])
    return float(GRID_DEG[i]), float(right - left)


def residual(virtual, physical):
    """the target cell's snapshots [8][N_PULSES] of both: |virtual - alpha physical| / |alpha physical| with alpha the least-squares common factor"""
    v, q = virtual[:, :, BIN].reshape(-1), physical[:, :, BIN].reshape(-1)
    alpha = np.vdot(q, v) / np.vdot(q, q)
    return float(np.linalg.norm(v - alpha * q) / np.linalg.norm(alpha * q)), complex(alpha)


def figures(rts, virtual, physical4, line):
    """of the bank's output [8][P][N], the four physical receivers' own compression [4][P][N] and the compressed eight-element line
    [8][P][N]: dict(virtual=(peak, width), line=..., four=..., residual, alpha)"""
    res, alpha = residual(virtual, line)
    return dict(virtual=peak_and_width(bartlett(rts, virtual, rts.virtual_positions(tx_offsets(), rx_positions()))),
                line=peak_and_width(bartlett(rts, line, line_positions())),
                four=peak_and_width(bartlett(rts, physical4, rx_positions())), residual=res, alpha=alpha)


def check(fig):
    """conditions (a) and (b); every figure is printed before it is held to its condition"""
    print("virtual array: peak at %.1f degrees, -3 dB width %.2f degrees; eight-element line: %.1f, %.2f; the four receivers alone: %.1f, %.2f" %
          (fig["virtual"] + fig["line"] + fig["four"]))
    print("target cell: virtual against physical snapshots, residual %.3g of their norm after the common factor %.6f%+.6fj (bound %.3g)" %
          (fig["residual"], fig["alpha"].real, fig["alpha"].imag, RESIDUAL_BOUND))
    assert abs(fig["virtual"][0] - fig["line"][0]) <= GRID_STEP + 1e-9 and abs(fig["line"][0]) <= GRID_STEP + 1e-9, fig
    assert abs(fig["virtual"][1] - fig["line"][1]) <= GRID_STEP + 1e-9, fig
    assert 1.7 <= fig["four"][1] / fig["line"][1] <= 2.3, fig          # "near twice": a uniform line's width goes as 1 / N, 2.0 for 4 against 8 but for the lobe's curvature
    assert fig["residual"] <= RESIDUAL_BOUND, fig


# ----------------------------------------------------------------------------- the host chain
@functools.lru_cache(maxsize=None)
def host_chain(rts, oracle):
    """everything on the host: dict(cube [4][8][64], line_raw [8][8][64], t0, counts (echoes) and sizes (records) per launch, virtual,
    four, line, figures)"""
    L = launches(rts, oracle)
    taus = np.concatenate([[c[2] for c in CR.contribs_rays(echoes(rec), CS, FC)] for rec in L.values()])
    assert taus.max() - taus.min() < 0.5 * DT, (taus.min(), taus.max())
    t0 = float(taus.min()) - (BIN + 0.25) * DT
    cube = np.zeros((N_EL, N_PULSES, N_BINS), np.complex128); line_raw = np.zeros((N_VIRT, N_PULSES, N_BINS), np.complex128)
    for (what, t, k, p), rec in L.items():
        if what == "mimo":
            cube[k, p] += render_numpy(rec, sent(t, p), t0)
        else:
            line_raw[k, p] += render_numpy(rec, sent(0, p), t0)
    counts = {key: len(echoes(rec)) for key, rec in L.items()}
    out = dict(cube=cube, line_raw=line_raw, t0=t0, counts=counts, sizes={key: len(rec) for key, rec in L.items()})
    out.update(products(rts, cube, line_raw, lambda c, w, code: rts.bank_eval(c, w, code)))
    return out


def compress_ref(cube, s):
    """tests/cube_ref.py's statement of the compression on every row"""
    return np.array([[CR.to_double(CR.correlate_ref(row, s)) for row in rx] for rx in cube])


def products(rts, cube, line_raw, bank, compress=compress_ref):
    """the bank of the radar's cube (`bank`: the evaluator or the device), the four receivers' own compression with waveform 0 and the
    line's compression (`compress`: cube_ref's statement, or the device's rts_cube_compress), and their figures"""
    virtual = bank(cube, waveforms(rts), slow_code())
    four = compress(cube, chips()[0]); line = compress(line_raw, chips()[0])
    return dict(virtual=virtual, four=four, line=line, figures=figures(rts, virtual, four, line))
