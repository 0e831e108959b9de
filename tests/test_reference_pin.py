"""The oracle against the reference's OWN device programs (CPU; needs oracle/_ref/librts_ref.so).

Every GPU parity test compares the HIP path with oracle/rts_oracle.cpp; this file compares the oracle with the text it
restates.  build() compiles the reference's triangle_mesh.cu, normal_shader.cu, ray_tracer.cu and the two kernels of
aggregation.cu, unmodified, as host C++ against the stand-in headers of oracle/refshim (oracle/Makefile: ref); the tests
here drive both through the same Python wrapper and compare BITS.  Where the library is absent (no reference sources on the
machine) every test of this file skips with one reason; tests/test_golden.py then still checks the oracle against the
fixtures recorded from these programs (tests/golden/ref_*.npz).

What stays outside the pin: the OptiX traversal (rtTrace is the harness's brute force, ties to the lowest global id), CUDA's
atan2f bits (exercised both ways below) and the reference's host program.
"""
import functools
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, "golden"))
import helpers as H  # noqa: E402
from test_host_logic import random_received_set  # noqa: E402

C0 = 299792458.0
SKIP_REASON = "oracle/_ref/librts_ref.so is absent: build() makes it where the reference's sources are (oracle.build_ref)"


@pytest.fixture(scope="module")
def O(oracle):
    if oracle.ref_lib() is None:
        pytest.skip(SKIP_REASON)
    return oracle


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


# ------------------------------------------------------------------------------------------------ bound
def bound_cases():
    rng = np.random.default_rng(11)
    n = 100000
    scale = 10.0 ** rng.uniform(-30, 30, (n, 1, 1))
    tri = rng.normal(size=(n, 3, 3)) * scale
    tri[: n // 4] += (rng.normal(size=(n // 4, 1, 3)) * scale[: n // 4] * 100.0)          # small triangles far from the origin
    tri[n // 4: n // 2] *= 10.0 ** rng.uniform(-3, 3, (n // 4, 3, 3))                     # slivers: per-coordinate magnitudes
    f32 = tri[:2000].astype(np.float32).astype(np.float64)                                # exactly representable in f32
    half = f32 + 0.5 * np.spacing(np.abs(f32).astype(np.float32)).astype(np.float64)       # half an f32 ulp above: a tie
    below = np.nextafter(f32, -np.inf); above = np.nextafter(f32, np.inf)                  # one f64 ulp either side of an f32
    p = rng.normal(size=(500, 3))
    zero = np.repeat(p[:, None, :], 3, 1)                                                  # zero area: one point three times
    two = np.stack([p, p, p + 1.0], 1)                                                     # zero area: two vertices equal
    d = rng.normal(size=(500, 3))
    col = np.stack([p, p + d, p + 2.0 * d], 1)                                             # collinear (area 0 or rounding dust)
    col_exact = np.stack([np.round(p * 8), np.round(p * 8) + np.round(d * 4), np.round(p * 8) + 3 * np.round(d * 4)], 1)
    inf = tri[:600].copy(); nan = tri[:600].copy()
    k = np.arange(600)
    inf[k, k % 3, (k // 3) % 3] = np.where(k % 2 == 0, np.inf, -np.inf)
    nan[k, k % 3, (k // 3) % 3] = np.nan
    huge = rng.normal(size=(300, 3, 3)) * 1e160                                            # the area overflows to inf
    tiny = rng.normal(size=(300, 3, 3)) * 1e-170                                           # the area underflows to 0
    beyond = rng.normal(size=(300, 3, 3)) * 1e39                                           # finite in f64, past f32's range
    return np.concatenate([tri, f32, half, below, above, zero, two, col, col_exact, inf, nan, huge, tiny, beyond])


def test_bound_bit_equal(O):
    """triangle_mesh.cu's bound program on 100 000 random triangles (1e-30 .. 1e30) and the planted edge cases: validity and
    all six f32 bit patterns (round down / round up of the f64 extremes) equal"""
    tri = bound_cases()
    ov, ob = O.bound_n(tri)
    rv, rb = O.ref_bound_n(tri)
    assert rv[:100000].mean() > 0.99 and (~rv[100000:]).sum() >= 2500                      # both arms are really taken
    assert np.array_equal(ov, rv), "validity differs at %s" % np.nonzero(ov != rv)[0][:10]
    same = bits(ob) == bits(rb)
    assert same.all(), "boxes differ at %s" % np.argwhere(~same)[:10]
    # the directed roundings do something: of the half-ulp ties every box side moved outward
    half = slice(102000, 104000)
    lo = tri[half].min(1); hi = tri[half].max(1)
    assert (rb[half, :3].astype(np.float64) < lo).all() and (rb[half, 3:].astype(np.float64) > hi).all()


# ------------------------------------------------------------------------------------------------ intersect
def random_pairs(rng, n):
    tri = rng.normal(size=(n, 3, 3)) * 10.0 ** rng.uniform(-1, 2, (n, 1, 1)) + rng.normal(size=(n, 1, 3)) * 20.0
    w = rng.dirichlet([1.0, 1.0, 1.0], n)
    w = np.where(rng.random((n, 1)) < 0.5, w, w * 3.0 - 1.0)                               # half of the aim points lie outside
    aim = (tri * w[:, :, None]).sum(1)
    origin = aim + rng.normal(size=(n, 3)) * 10.0 ** rng.uniform(-2, 3, (n, 1))
    d = aim - origin
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    d = d.astype(np.float32).astype(np.float64)                                            # a traced ray's direction is an f32 widened
    flip = rng.random(n) < 0.1
    d[flip] = -d[flip]                                                                     # t < 0
    long = rng.random(n) < 0.2
    d[long] *= 10.0 ** rng.uniform(-3, 3, (long.sum(), 1))                                 # and some that are no unit vectors
    tmin = np.full(n, 0.005, np.float32)
    tmax = np.where(rng.random(n) < 0.3, 10.0 ** rng.uniform(-2, 3, n), 1e27).astype(np.float32)
    return origin, d, tmin, tmax, tri


def planted_pairs():
    """p0 = (0,0,0), p1 = (4,0,0), p2 = (0,4,0), rays along +z from z = -8: every term of the test is exact, beta = x/4,
    gamma = y/4, t = 8.  Returns the pairs and the decision the reference's text gives them."""
    tri = np.array([[0.0, 0, 0], [4, 0, 0], [0, 4, 0]])
    e = 2.0 ** -40
    rows = []                                                                              # (x, y, z0, dz, tmin, tmax, hit)

    def add(x, y, hit, z0=-8.0, dz=1.0, tmin=0.005, tmax=1e27):
        rows.append((x, y, z0, dz, tmin, tmax, hit))
    add(1, 0, True); add(3, 0, True)                                                       # gamma == 0
    add(0, 1, True); add(0, 3, True)                                                       # beta == 0
    add(2, 2, True); add(1, 3, True); add(3.5, 0.5, True)                                  # beta + gamma == 1
    add(0, 0, True); add(4, 0, True); add(0, 4, True)                                      # the vertices
    add(1, -e, False); add(-e, 1, False); add(2 + e, 2, False); add(-e, -e, False); add(4 + 4 * e, 0, False)   # just outside
    add(1, e, True); add(e, 1, True); add(2 - e, 2, True)                                  # just inside
    add(1, 1, True)                                                                        # t == 8: strictly inside (tmin, tmax)
    add(1, 1, False, tmin=8.0); add(1, 1, False, tmax=8.0)                                 # t on tmin, t on tmax
    add(1, 1, True, tmin=float(np.nextafter(np.float32(8), np.float32(0)))); add(1, 1, True, tmax=float(np.nextafter(np.float32(8), np.float32(9))))
    add(1, 1, False, z0=-(8.0 + 2.0 ** -30), tmin=8.0)                                     # f64 t > tmin, its f32 is ON tmin: the f32 test decides
    add(1, 1, False, z0=-(8.0 - 2.0 ** -30), tmax=8.0)
    add(1, 1, True, z0=8.0, dz=-1.0); add(1, 0, True, z0=8.0, dz=-1.0); add(2, 2, True, z0=8.0, dz=-1.0)   # back face
    add(1, 1, False, z0=8.0, dz=1.0)                                                       # behind the origin
    r = np.array(rows)
    n = len(r)
    origin = np.stack([r[:, 0], r[:, 1], r[:, 2]], 1); d = np.stack([np.zeros(n), np.zeros(n), r[:, 3]], 1)
    # parallel to the plane (1 / 0): in the plane through the triangle, in the plane beside it, above the plane
    po = np.array([[-1.0, 1, 0], [-1, 9, 0], [-1, 1, 2], [1, 1, 0], [0, 0, 0]]); pd = np.array([[1.0, 0, 0], [1, 0, 0], [1, 0, 0], [0, 1, 0], [1, 1, 0]])
    origin = np.concatenate([origin, po]); d = np.concatenate([d, pd])
    tmin = np.concatenate([r[:, 4], np.full(len(po), 0.005)]).astype(np.float32)
    tmax = np.concatenate([r[:, 5], np.full(len(po), 1e27)]).astype(np.float32)
    want = np.concatenate([r[:, 6] > 0, np.zeros(len(po), bool)])
    return origin, d, tmin, tmax, np.repeat(tri[None], len(origin), 0), want


@pytest.mark.parametrize("smooth,k", [(True, 3), (False, 3), (True, 5), (False, 5)])
def test_intersect_bit_equal(O, smooth, k):
    """triangle_mesh.cu's intersection program, one ray against one triangle: 4 x 50 000 random pairs plus the planted ones,
    with interpolated vertex normals (smooth, 3 normals), the flat face normal, and the "more normals than vertices" rule
    (5 normals: normal = normals[prim]).  Hit decision, f32 t and the f64 attribute normal are bit-equal."""
    rng = np.random.default_rng(100 + 2 * k + smooth)
    parts = [random_pairs(rng, 50000), planted_pairs()[:5]]
    origin, d, tmin, tmax, tri = [np.concatenate(x) for x in zip(*parts)]
    n = len(origin)
    nrm = rng.normal(size=(n, k, 3))
    unit = rng.random(n) < 0.7
    nrm[unit] /= np.linalg.norm(nrm[unit], axis=2, keepdims=True)
    nrm[-7] = 0.0                                                                          # a zero normal: 0 / 0 in the normalisation
    oh, ot, on = O.intersect_n(origin, d, tmin, tmax, tri, nrm, smooth)
    rh, rt, rn = O.ref_intersect_n(origin, d, tmin, tmax, tri, nrm, smooth)
    want = planted_pairs()[5]
    assert np.array_equal(rh[50000:], want), "the reference's own decision on the planted pairs: %s" % np.nonzero(rh[50000:] != want)[0]
    assert 0.2 < rh[:50000].mean() < 0.6
    assert np.array_equal(oh, rh), "hit decisions differ at %s" % np.nonzero(oh != rh)[0][:10]
    assert np.array_equal(bits(ot), bits(rt)), "f32 t differs at %s" % np.nonzero(bits(ot) != bits(rt))[0][:10]
    same = bits(on) == bits(rn)
    assert same.all(), "attribute normals differ at %s" % np.argwhere(~same)[:10]
    if smooth and k == 5:                                                                  # the rule really is "normals[prim_index]"
        hit = rh & np.isfinite(rn).all(1) & (np.linalg.norm(nrm[:, 0], axis=1) > 0)
        np.testing.assert_allclose(rn[hit], nrm[hit, 0] / np.linalg.norm(nrm[hit, 0], axis=1, keepdims=True), rtol=0, atol=1e-15)


# ------------------------------------------------------------------------------------------------ whole traces
def _refraction(S, max_refl):
    spec = S.config_multi(W=12, max_refl=max_refl)                                         # the scene of test_gpu_parity.test_refraction
    spec["max_refr"] = 1
    spec["meshes"][0]["refr_index"] = 1.5; spec["meshes"][0]["refl_coeff"] = 0.5
    spec["meshes"][1]["refr_index"] = 2.2; spec["meshes"][1]["refl_coeff"] = -0.6
    spec["meshes"][2]["refl_coeff"] = 1.0
    spec["rx"] = spec["rx"] + [S._rx_at((200.0, 0.0, 0.0), (0, 0, 0), 90.0, 2.6)]
    return spec


def _moving(S, api):
    spec = S.config_multi(W=12)
    spec["motion"] = [dict(position=(0.6, 0.2, 0.0), velocity=(300.0, 100.0, 0.0), rotation=api.rotation_matrix(0.4, 0.1, -0.2)),
                      dict(position=(2.0, 8.0, 1.0), velocity=(0.0, -500.0, 0.0)),
                      dict(position=(9.0, -7.0, 0.4), velocity=(0.0, 0.0, 200.0), rotation=api.rotation_matrix(0.0, 0.0, 0.6))]
    return spec


def trace_specs():
    from rts_amd import scenes as S, api
    c2 = S.config2(subdiv=2, W=12, rx_radius=400.0)
    return {
        "c1_plate": dict(S.config1(), W=12),
        "c2_smooth": c2,
        "c2_flat": dict(c2, smooth=False),
        "multi_refl0": S.config_multi(W=16, max_refl=0),
        "multi_refl1": S.config_multi(W=16, max_refl=1),
        "multi_refl4": S.config_multi(W=16, max_refl=4),
        "multi_flat": S.config_multi(W=16, max_refl=4, smooth=False),
        "refraction_refl1": _refraction(S, 1),
        "refraction_refl3": _refraction(S, 3),
        "miss_branches": S.config_miss_branches(W=15),
        "earth_equator": S.translate(S.config_miss_branches(W=15), S.ecef_offset()),
        "earth_oblique": S.translate(S.config_miss_branches(W=15), S.ecef_offset(lat=0.6, lon=-2.0)),
        "pole_up": dict(S.config_pole(True), W=8),
        "pole_down": dict(S.config_pole(False), W=8),
        "moving": _moving(S, api),
    }


TRACE_NAMES = ["c1_plate", "c2_smooth", "c2_flat", "multi_refl0", "multi_refl1", "multi_refl4", "multi_flat", "refraction_refl1",
               "refraction_refl3", "miss_branches", "earth_equator", "earth_oblique", "pole_up", "pole_down", "moving"]


@functools.lru_cache(maxsize=None)
def traced(name):
    """(oracle trace, its miss-program coverage, reference trace with the oracle's atan2f, reference trace with libm's),
    computed once per scene and shared; nobody writes to them"""
    from oracle import oracle as O
    spec = trace_specs()[name]
    O.coverage()
    o = H.oracle_trace(O, spec, use_bvh=False)
    cov = O.coverage()
    O.ref_pin_atan2f(True)
    pinned = H.oracle_trace(O.REF, spec)
    O.ref_pin_atan2f(False)
    libm = H.oracle_trace(O.REF, spec)
    O.ref_pin_atan2f(True)
    return o, cov, pinned, libm


@pytest.mark.parametrize("name", TRACE_NAMES)
def test_trace_bit_equal_pinned_atan2f(O, name):
    """ray_generation, intersect, closest_hit and miss of the reference, run over a whole launch with the oracle's atan2f in
    the miss program, against oracle.trace(use_bvh=False): every PerRayData field of every row, the path rows, the hit
    primitive and f32 t per bounce and the segment / shaded / triangle-test counts equal; RCS angles to 1e-12 rad"""
    o, cov, r, _ = traced(name)
    spec = trace_specs()[name]
    rows = len(o["results"])
    assert rows == spec["W"] ** 3 * (spec["max_refl"] + 3 if spec.get("max_refr", 0) else 1) == len(r["results"])
    H.assert_prd_equal(o["results"], r["results"], name + ": per-ray records, oracle vs reference programs")
    assert np.array_equal(o["path"], r["path"]), "path rows differ"
    assert np.array_equal(o["hit_prim"], r["hit_prim"]), "hit primitives differ"
    assert np.array_equal(bits(o["hit_t"]), bits(r["hit_t"])), "f32 hit distances differ"
    for c in ("segments", "shaded", "tri_tests"):
        assert o["counters"][c] == r["counters"][c], (c, o["counters"], r["counters"])
    np.testing.assert_allclose(o["rcs_angle"], r["rcs_angle"], rtol=0, atol=1e-12)
    if spec["max_refl"] > 0 and not name.startswith("pole"):                              # (the pole scenes are direct rays only)
        assert r["counters"]["shaded"] > 0 and (r["hit_prim"][:, 0] >= 0).any()
    if spec.get("max_refr", 0):                                                            # the three row chains are live
        n = spec["W"] ** 3
        res = r["results"]
        assert (res["refrDepth"][n:2 * n] >= 1).any() and (res["refrDepth"][2 * n:3 * n] == 2).any() and (res["received"][2 * n:3 * n] >= 0).any()
    if name == "moving":
        assert np.abs(r["results"]["doppler"]).max() > 100.0


def test_traces_reach_every_miss_branch(O):
    """the agreement above is not vacuous: over the scenes every named branch of the miss program was taken, and every
    scene but the absorbing one has received rays"""
    total = {}
    for name in TRACE_NAMES:
        o, cov, r, _ = traced(name)
        for k, v in cov.items():
            total[k] = total.get(k, 0) + v
        if name != "multi_refl0":
            assert (r["results"]["received"] >= 0).sum() > 0, name
    assert sorted(total) == sorted(O.COVERAGE_NAMES)
    missing = [k for k in O.COVERAGE_NAMES if total[k] == 0]
    assert not missing, missing


@pytest.mark.parametrize("name", TRACE_NAMES)
def test_trace_libm_atan2f_changes_at_most_one_in_a_thousand(O, name):
    """the project's one flagged deviation ([D1]: atan2f from basic f64 operations rounded once, where the reference calls
    its platform's atan2f) left IN: the reference's programs with libm's atan2f against themselves with the oracle's.
    Condition: the rays whose `received` differs are at most 0.1 % of the scene's received rays.

    Observed (glibc 2.35): 0 differing rays in every scene -- received rays per scene: c1_plate 192, c2_smooth 48, c2_flat 48,
    multi_refl0 0, multi_refl1 32, multi_refl4 48, multi_flat 16, refraction_refl1 1506, refraction_refl3 1506,
    miss_branches 2127, earth_equator 2127, earth_oblique 2127, pole_up 512, pole_down 512, moving 24."""
    o, cov, pinned, libm = traced(name)
    a, b = pinned["results"]["received"], libm["results"]["received"]
    differ = int((a != b).sum()); received = int((a >= 0).sum())
    print("%s: received %d, differing %d" % (name, received, differ))
    assert differ <= 0.001 * received, (name, differ, received)


# ------------------------------------------------------------------------------------------------ aggregation
ARMS = {"one_block": (1024, 65535), "small": (32, 4), "mid": (64, 1000)}


def expected_launch(R, mt, mb):
    if R <= mt:
        return "one_block", (1, R)
    if R > mt * mb:
        return "grid_stride", (mb, mt)
    return "partial_grid", ((R + mt - 1) // mt, mt)


def test_aggregate_cases_cover_all_launch_arms():
    arms = {(R, s): expected_launch(R, *ARMS[s])[0] for R in (1, 50, 700, 3000) for s in ARMS}
    assert set(arms.values()) == {"one_block", "partial_grid", "grid_stride"}
    assert arms[(700, "small")] == arms[(3000, "small")] == "grid_stride" and arms[(3000, "one_block")] == "partial_grid"


MAX_POWER_ULP = 0       # measured over all 72 cases below: pow(x, 2) of the reference and x*x of the oracle ([D2]) never differed


@pytest.mark.parametrize("shape", sorted(ARMS))
@pytest.mark.parametrize("D", [1, 2, 3, 4, 5, 6])
@pytest.mark.parametrize("R", [1, 50, 700, 3000])
def test_aggregate_bit_equal(O, R, D, shape):
    """myKernel1 + myKernel2 of the reference, launched serially as its kernel_wrapper would (one block / a partial grid /
    the grid-stride arm), against oracle.aggregate_literal: pathMatch, npath, delay, phase, Doppler and the running sums
    bit-equal.  power = pow(v, 2) there and v*v here ([D2]): the issue allows 1 ulp; the largest difference measured over
    all cases is 0 ulp, so 0 is asserted."""
    rng = np.random.default_rng(1000 * D + R)
    a, paths = random_received_set(O, rng, R, D, n_rx=3, n_targ=2, p_direct=0.25)
    a["refrDepth"][::5] = 2                              # refracted rows, some with no reflection: only reflDepth == 0 AND refrDepth == 0 is "direct"
    if R >= 50:
        assert ((a["reflDepth"] == 0) & (a["refrDepth"] == 0)).any() and ((a["reflDepth"] == 0) & (a["refrDepth"] == 2)).any()
    mt, mb = ARMS[shape]
    lit = O.aggregate_literal(a, paths, C0, 10e9, 10 ** 6)
    ref = O.ref_aggregate(a, paths, C0, 10e9, 10 ** 6, mt, mb)
    assert ref["launch"] == expected_launch(R, mt, mb)[1]
    assert np.array_equal(lit["pathMatch"], ref["pathMatch"])
    for f in ("npath", "delay", "phase", "power_sum", "doppler_sum"):
        assert np.array_equal(bits(lit[f]), bits(ref[f])), f
    assert np.array_equal(bits(lit["results"]["doppler"]), bits(ref["results"]["doppler"]))
    for f in H.PRD_EXACT_FIELDS:
        if f not in ("power", "doppler"):
            assert np.array_equal(lit["results"][f], ref["results"][f]), f
    ulp = np.abs(bits(lit["results"]["power"]).astype(np.int64) - bits(ref["results"]["power"]).astype(np.int64))
    print("R %d D %d %s: launch %s, largest power difference %d ulp" % (R, D, shape, ref["launch"], ulp.max()))
    assert ulp.max() <= MAX_POWER_ULP
    assert (lit["npath"] > 1).any() or R == 1


# ------------------------------------------------------------------------------------------------ the recorded fixtures
@pytest.mark.parametrize("name", ["refraction_w12", "miss_branches_w12", "earth_oblique_w12", "flat_w14", "rect_w14", "moving_w12"])
def test_generator_reproduces_committed_fixture(O, name):
    """tests/golden/make_ref_golden.py, run on the reference's programs as built here, gives the committed ref_<name>.npz array
    for array; and the reference's sources are the ones the fixtures were recorded from (ref_MANIFEST.txt)"""
    import make_ref_golden
    g = np.load(os.path.join(HERE, "golden", "ref_" + name + ".npz"), allow_pickle=False)
    a = make_ref_golden.record(name, make_ref_golden.ref_golden_specs()[name])
    assert sorted(a) == sorted(g.files)
    for k in g.files:
        assert a[k].dtype == g[k].dtype and a[k].shape == g[k].shape, k
        assert np.array_equal(np.ascontiguousarray(a[k]).view(np.uint8), np.ascontiguousarray(g[k]).view(np.uint8)), k   # (zeroed padding included)
    reference = os.environ.get("RTS_REFERENCE_DIR") or O.REFERENCE_DIR
    if os.path.isdir(reference):
        with open(os.path.join(HERE, "golden", "ref_MANIFEST.txt")) as fh:
            assert make_ref_golden.manifest(reference) == fh.read()
