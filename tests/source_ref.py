"""What tests/test_source_host.py and tests/test_gpu_source.py share: the plain-Python restatement of the clutter and jammer sources
from the text of include/rts_amd.h alone (RtsSourceParams: Python floats for every sum and product, Philox in integer arithmetic,
math.log, math.cos and math.sin), the agreement bound, the header's constants, seeded patch sets and the two recipes (a jammer for
tests/adapt_ref.py's scene, the clutter ridge for tests/stap_ref.py's).

The agreement bound.  Device, evaluator and restatement run the same tree of IEEE operations on the same inputs; they differ only
in the draws w(k, r, p), through log, cos and sin (OCML on the device, libm on the host).  The project holds its generator to
rtol = atol = 1e-13 per component at unit scale (tests/test_gpu_detect.py: test_noise_matches_eval_and_splits), that is
|dw_c| <= 1e-13 (1 + |w_c|) for a component w_c of a draw.  A component is at most sqrt(0.5) sqrt(-2 ln 2^-53) = sqrt(-ln 2^-53) =
6.0611 < 6.07 (u1 >= 2^-53), so |dw_c| <= 1e-13 * 7.07 and the complex difference of one draw has modulus at most
sqrt(2) * 7.07e-13 < 1e-13 * 10.0.  The draw of pulse q enters c_krp linearly, as pole^(p - q) s_kr (g_k or 1) dw with |pole| <= 1 and
g <= 1, so it persists with at most its own size: |dc_krp| <= (p + 1) s_kr * 10.0e-13.  The sample is sum_k spatial[k][rx] (x) c_krp,
whose difference is at most sum_k |spatial[k][rx]| |dc_krp| in each component.  With a cube that is not zero the final addition
rounds a sum that differs: one more half ulp of the result on each side, 2^-52 |value before| covers it for values that dominate.
Hence, for sample (rx, p, r),
    bound = 1e-13 (p + 1) A[rx][r] + 2^-52 |cube value before|,   A[rx][r] = C sum_k |spatial[k][rx]| sqrt(power_k profile_r),
with C = 10.0 from this derivation.  (The issue that introduced the feature proposed C = 6.07, the largest component alone; that
form drops the absolute term of the generator's tolerance and the sqrt(2) of a complex modulus.  The derivation wins: C = 10.0.
Second-order terms -- roundings of the recursion that act on slightly different operands -- are of size 2^-53 per step relative to
c and three orders below 1e-13.)  The bound is NOT fitted to what the code gives: observed differences are around 1e-15 A."""
import math
import os
import re

import numpy as np

import adapt_ref as A
import beam_ref as B
import stap_ref as S

ROOT = A.ROOT
BOUND_C = 10.0
EPS = 2.0 ** -52


def header_constant(name, files=("include/rts_amd.h", "rts_amd/csrc/rts_source.h")):
    for rel in files:
        with open(os.path.join(ROOT, rel)) as f:
            m = re.search(r"#define %s\s+(\d+)u" % name, f.read())
        if m:
            return int(m.group(1))
    raise KeyError(name)


MAX_PATCHES, MAX_TABLE = header_constant("RTS_SRC_MAX_PATCHES"), header_constant("RTS_SRC_MAX_TABLE")
TILE = header_constant("RTS_SRC_WAVES")                  # the workgroup's tile: RTS_SRC_TILE = RTS_SRC_WAVES adjacent bins
MAX_RX = A.header_constant("RTS_BEAM_MAX_RX")

# ----------------------------------------------------------------------------- the generator, in integers
M0, M1, W0, W1 = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85
MASK = 0xFFFFFFFF


def philox(counter, key):
    c = list(counter); k0, k1 = key
    for r in range(10):
        if r:
            k0 = (k0 + W0) & MASK; k1 = (k1 + W1) & MASK
        p0, p1 = M0 * c[0], M1 * c[2]
        c = [(p1 >> 32) ^ c[1] ^ k0, p1 & MASK, (p0 >> 32) ^ c[3] ^ k1, p0 & MASK]
    return c


def gaussian(counter, seed, sigma):
    """the generator of rts_cube_add_noise on a counter of four words"""
    x = philox(counter, (seed & MASK, (seed >> 32) & MASK))
    a, b = ((x[0] << 32) | x[1]) >> 11, ((x[2] << 32) | x[3]) >> 11
    u1, u2 = float(a + 1) * 2.0 ** -53, float(b) * 2.0 ** -53
    sr = sigma * math.sqrt(-2.0 * math.log(u1))
    ang = 2.0 * math.pi * u2
    return sr * math.cos(ang), sr * math.sin(ang)


def draw(seed, r, p, k):
    """w(k, r, p): unit power, Philox counter (r, p, k, 1)"""
    return gaussian((r, p, k, 1), seed, math.sqrt(0.5))


def cos_sin_turns(x):
    """(cos, sin)(2 pi f), f = x - floor(x): the exact reflections about 1 and 1/2, then libm -- rts_steering_make's rule"""
    t, sgn = 2.0 * (x - math.floor(x)), 1.0
    if t >= 2.0:
        t -= 2.0
    if t >= 1.0:
        t -= 1.0; sgn = -1.0
    if t > 0.5:
        s, c = math.sin(math.pi * (1.0 - t)), -math.cos(math.pi * (1.0 - t))
    else:
        s, c = math.sin(math.pi * t), math.cos(math.pi * t)
    if t == 0.5:
        c = 0.0
    return sgn * c, sgn * s


def mul(a, b):
    return a[0] * b[0] - a[1] * b[1], a[0] * b[1] + a[1] * b[0]


def tree(part):
    """part: 64 entries, None where the partial has no patch; j takes j + s for s = 32 .. 1"""
    part = list(part)
    s = 32
    while s >= 1:
        for j in range(s):
            hi = part[j + s]
            if hi is not None:
                part[j] = hi if part[j] is None else (part[j][0] + hi[0], part[j][1] + hi[1])
        part = part[:s]
        s //= 2
    return part[0]


def sources_restated(cube, spatial, power, doppler, rho=None, range_profile=None, seed=0):
    """the header's text, literally; returns the new array"""
    out = np.array(cube, np.complex128, copy=True)
    n_rx, n_p, nb = out.shape
    K = len(power)
    sp = [[(float(spatial[k][rx].real), float(spatial[k][rx].imag)) for rx in range(n_rx)] for k in range(K)]
    live = [k for k in range(K) if float(power[k]) > 0.0]
    if not live:
        return out
    pole, g = {}, {}
    for k in live:
        rh = 1.0 if rho is None else float(rho[k])
        c, s = cos_sin_turns(float(doppler[k]))
        pole[k] = (rh * c, rh * s); g[k] = math.sqrt(1.0 - rh * rh)
    for r in range(nb):
        profile = 1.0 if range_profile is None else float(range_profile[r])
        if profile == 0.0:
            continue
        c, gs = {}, {}
        for k in live:
            s = math.sqrt(float(power[k]) * profile)
            w = draw(seed, r, 0, k)
            c[k] = (s * w[0], s * w[1]); gs[k] = g[k] * s
        for p in range(n_p):
            if p:
                for k in live:
                    c[k] = mul(pole[k], c[k])
                    if g[k] != 0.0:
                        w = draw(seed, r, p, k)
                        c[k] = (c[k][0] + gs[k] * w[0], c[k][1] + gs[k] * w[1])
            for rx in range(n_rx):
                part = [None] * 64
                for k in live:
                    t = mul(sp[k][rx], c[k])
                    j = k % 64
                    part[j] = t if part[j] is None else (part[j][0] + t[0], part[j][1] + t[1])
                total = tree(part)
                z = out[rx, p, r]
                out[rx, p, r] = complex(float(z.real) + total[0], float(z.imag) + total[1])
    return out


def bound(before, spatial, power, range_profile=None):
    """the agreement bound of every sample of a cube of before's shape (the module's docstring)"""
    before = np.asarray(before)
    n_rx, n_p, nb = before.shape
    profile = np.ones(nb) if range_profile is None else np.asarray(range_profile, np.float64)
    Aa = BOUND_C * np.einsum("kx,kr->xr", np.abs(np.asarray(spatial)), np.sqrt(np.outer(np.asarray(power, np.float64), profile)))
    return 1e-13 * np.arange(1, n_p + 1)[None, :, None] * Aa[:, None, :] + EPS * np.abs(before)


def assert_within(got, want, bnd):
    d = np.maximum(np.abs(got.real - want.real), np.abs(got.imag - want.imag))
    worst = np.unravel_index(np.argmax(d - bnd), d.shape)
    assert np.all(d <= bnd), (worst, d[worst], bnd[worst])
    return float((d / np.where(bnd > 0, bnd, 1.0)).max())


def bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


# ----------------------------------------------------------------------------- seeded patch sets
RHOS = (0.0, 0.5, 0.9, 1.0)


def patches(seed, K, n_rx, n_bins, rho="mixed", profile=None):
    """K patches: random responses, powers in (0.5, 2), Dopplers in (-1.5, 1.5); rho mixed from RHOS, "ones" (NULL) or a value;
    profile None, "random" (positive) or "edges": zeros at the first bin, the last bin and on both sides of every tile edge"""
    rng = np.random.default_rng(seed)
    d = dict(spatial=B.random_complex(rng, (K, n_rx)), power=rng.uniform(0.5, 2.0, K), doppler=rng.uniform(-1.5, 1.5, K))
    if rho == "mixed":
        d["rho"] = rng.choice(RHOS, K); d["rho"][:len(RHOS)] = RHOS[:K]
    elif rho != "ones":
        d["rho"] = np.full(K, float(rho))
    if profile is not None:
        pr = rng.uniform(0.25, 4.0, n_bins)
        if profile == "edges":
            pr[0] = 0.0; pr[-1] = 0.0
            for e in range(TILE, n_bins, TILE):
                pr[e - 1] = 0.0; pr[e] = 0.0
        d["range_profile"] = pr
    return d


# ----------------------------------------------------------------------------- the two recipes
def jammer_recipe(rts):
    """tests/adapt_ref.py's scene with the jammer from the library: keyword arguments of sources_eval / cube_add_sources (K = 1, rho = 0,
    the jammer's steering row, power jnr) and the target alone as the cube to start from"""
    sc = A.SCENE
    pos, _, fc = A.scene_geometry()
    src = dict(spatial=rts.steering(pos, [[sc["jammer_az"], 0.0]], sc["wavelength"]), power=[sc["jnr"]], doppler=[0.0], rho=[0.0], seed=sc["seed"])
    cube = np.zeros((sc["n_rx"], sc["n_pulses"], sc["n_bins"]), np.complex128)
    cube[:, :, sc["target_bin"]] += (math.sqrt(sc["target_power"]) * B.snapshot(pos, sc["target_az"], 0.0, fc))[:, None]
    return src, cube


def clutter_recipe(rts):
    """tests/stap_ref.py's scene with the ridge from the library: 89 patches, rho = 1 (NULL), doppler = 0.5 sin az, cnr spread equally"""
    sc = S.SCENE
    pos, _ = S.scene_geometry()
    az = S.patch_azimuths()
    src = dict(spatial=rts.steering(pos, np.stack([az, np.zeros(len(az))], axis=1), sc["wavelength"]), power=np.full(len(az), sc["cnr"] / sc["n_patches"]),
               doppler=sc["ridge"] * np.sin(az), seed=sc["seed"])
    return src, np.zeros((sc["n_rx"], sc["n_pulses"], sc["n_bins"]), np.complex128)


def noise(rts, sc):
    n = sc["n_rx"] * sc["n_pulses"] * sc["n_bins"]
    return rts.noise_eval(sc["seed"], np.arange(n, dtype=np.uint64), sc["noise_power"]).reshape(sc["n_rx"], sc["n_pulses"], sc["n_bins"])


def stap_figures(rts, cube, w=None):
    """(improvement over the conventional space-time beam, loss against the optimum) in dB of weights trained on `cube` the scene's
    way (or of w), scored in the scene's TRUE covariance"""
    sc = S.SCENE
    taps = sc["taps"]
    if w is None:
        w = S.scene_host(rts, taps, cube)[3]
    v = S.space_time_vector(sc["target_az"], sc["target_f"], taps)
    R = S.scene_true_covariance(taps)
    adaptive, conventional, optimum = S.sinr(w[0], v, R), S.sinr(v / len(v), v, R), np.vdot(v, np.linalg.solve(R, v)).real
    return S.db(adaptive / conventional), S.db(optimum / adaptive)
