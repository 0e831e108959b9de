"""The horizon by azimuth sector (rts_horizon.hip, rts_shade): a bounce ray that the isotropic rule keeps walking is tested again
against the horizon of the quadrant of its in-plane azimuth in its triangle's own frame (u = e0, w = n x e0), four bytes per side.
Every case runs the same launch three ways -- sectors on (the default), RTS_FLAG_NO_HORIZON_SECTORS (the isotropic rule only) and
RTS_FLAG_NO_HORIZON -- against the oracle's brute force, every depth's hit record included.  The counting build tells the two rules
apart (walk_stats()[5]: isotropic, [11]: by a sector only) and both counts are bracketed by a numpy restatement of the rule on the
launch's own hit records; no launch index whose bounce meets its own target again is ever named by the restated sector rule; and
every decoded sector bounds a numpy brute force of sup h(x) / |x - q| over the pairs whose azimuth falls into that quadrant."""
import math
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import test_gpu_horizon as B      # the isotropic file's scenes and helpers (grid_plate, corner_mesh, one_mesh_spec, make_spec, world_tris)

pytestmark = pytest.mark.gpu

H0, RHO, MARGIN, TMIN = B.H0, B.RHO, B.MARGIN, B.TMIN
AZ_EXCLUDE = 1e-6                 # launch indices whose in-plane azimuth is this close [rad] to a quadrant boundary are left out of both counts


@pytest.fixture(scope="module")
def env():
    import rts_amd
    from rts_amd import api, scenes
    from oracle import oracle as O
    import helpers as H
    if api.device_count() < 1:
        pytest.skip("no HIP device")
    return api, scenes, O, H


# ------------------------------------------------------------------------------------------------ scenes
def fin_mesh(scenes):
    """a body (an ellipsoid, long axis across the beam) and a thin fin crossing its illuminated side: ONE mesh.  The fin rises over
    the planes of the body's triangles around it in the quadrants that look towards it only"""
    return scenes._merge([scenes._ico_ellipsoid(2, (1.5, 6.0, 1.5)), scenes._ico_ellipsoid(2, (2.0, 0.15, 1.2), centre=(-1.5, 2.0, 0.0))])


def axis_plate(origin, eu, ev, k):
    """a plate origin + a eu + b ev, a, b in [0, 1], as k x k cells of two triangles whose FIRST edge e0 = p1 - p0 runs along +eu
    (lower triangle) or -eu (upper): the quadrant boundaries of every triangle's frame run along the grid's own axes"""
    o, eu, ev = (np.asarray(x, np.float64) for x in (origin, eu, ev))
    a = np.linspace(0.0, 1.0, k + 1)
    v = np.array([o + x * eu + y * ev for y in a for x in a])
    t = []
    for j in range(k):
        for i in range(k):
            p = j * (k + 1) + i
            t += [[p, p + 1, p + k + 2], [p + k + 2, p + k + 1, p]]
    return v, np.array(t, np.uint32)


def post_mesh(scenes, along):
    """an 8 m plate tilted 45 degrees to the beam (+x), gridded along its own axes in 0.5 m cells, and a slender post (0.2 m square,
    4 m tall, in 16 levels) standing on it 1 m from its centre, exactly along +e0 of the lower triangles (along = "u") or exactly along
    their +w = n x e0 (along = "w").  The beam's in-plane component points from the illuminated patch (around the plate's centre, a
    grid vertex) at the post: reflected rays that land before the post leave ON the quadrant boundary and hit it; those that land
    beyond it leave with the post behind them -- the isotropic rule keeps them walking, their sector lets them go"""
    s = 1.0 / math.sqrt(2.0)
    up = np.array([s, 0.0, s]); side = np.array([0.0, 1.0, 0.0])      # in-plane: `up` carries the beam's in-plane component; normal (-s, 0, s)
    if along == "u":
        eu, ev = up, -side                                            # n = e1 x e0 ~ ev x eu... orientation fixed below by the check on n
    else:
        eu, ev = side, up
    L = 8.0
    v, t = axis_plate(-0.5 * L * (eu + ev), L * eu, L * ev, 16)
    p = v[t[0].astype(np.int64)]
    n = np.cross(p[0] - p[2], p[1] - p[0]); n /= np.linalg.norm(n)     # the record's normal of the plate's triangles (all alike)
    w = np.cross(n, eu)                                               # +w of the lower triangles
    towards = eu if along == "u" else w
    assert abs(float(towards @ up)) > 0.999, "the post's direction is the beam's in-plane direction"
    if float(towards @ up) < 0:                                       # (turn the plate about its normal so that +e0 / +w is where the reflected rays go)
        v = -v; p = v[t[0].astype(np.int64)]; n = np.cross(p[0] - p[2], p[1] - p[0]); n /= np.linalg.norm(n)
    nrm = np.array([-s, 0.0, s])                                      # the side the beam sees
    base = 1.0 * up; hw = 0.1; hgt = 4.0; levels = 16
    c = [base + sx * hw * up + sy * hw * side for sx, sy in ((-1, -1), (1, -1), (1, 1), (-1, 1))]
    pv = np.array([x + (hgt * l / levels) * nrm for l in range(levels + 1) for x in c])
    pt = []
    for l in range(levels):
        for i in range(4):
            a, b = 4 * l + i, 4 * l + (i + 1) % 4
            pt += [[a, b, b + 4], [a, b + 4, a + 4]]
    top = 4 * levels
    pt += [[top, top + 1, top + 2], [top, top + 2, top + 3]]
    vv = np.concatenate([v, pv]); tt = np.concatenate([t, np.array(pt, np.uint32) + len(v)]).astype(np.uint32)
    return vv, tt, np.tile(nrm, (len(vv), 1)), len(t)


def make_spec(scenes, api, name):
    one = name.endswith("1")
    if name.startswith("finrot"):
        s = B.one_mesh_spec(scenes, name, fin_mesh(scenes), 24, 1 if one else 4, span=(0.07, 0.07, 0.05))
        s["motion"] = [dict(m, rotation=tuple(api.rotation_matrix(0.3, -0.2, 0.15).ravel())) for m in s["motion"]]
        return s
    if name.startswith("finecef"):
        return scenes.translate(make_spec(scenes, api, "fin" + name[7:]), scenes.ecef_offset(lat=0.6, lon=-1.1))
    if name.startswith("fin"):
        return B.one_mesh_spec(scenes, name, fin_mesh(scenes), 24, 1 if one else 4, span=(0.07, 0.07, 0.05))
    if name.startswith("post"):                                     # post<u|w>1
        v, t, n, _ = post_mesh(scenes, name[4])
        return B.one_mesh_spec(scenes, name, (v, t, n), 24, 1, smooth=False, span=(0.0203, 0.0197, 0.05))
    return B.make_spec(scenes, api, name)


# ------------------------------------------------------------------------------------------------ the rule, restated
def rule_parts(scenes, spec, g, hzs):
    """one-bounce launch: per launch index the terms of the rule (rts_shade) from the full per-ray output g and the device's sector
    bytes hzs [n_prims][2][4] -- as rule_counts of the isotropic file forms them, plus the quadrant of the bounce direction in the
    hit triangle's frame and its in-plane azimuth"""
    P, targ, E = B.world_tris(scenes, spec)
    prim = g["hit_prim"][:, 0].astype(np.int64)
    hit = prim >= 0
    res = g["results"]
    o = res["prevHitPoint"]; ht = np.abs(g["hit_t"][:, 0].astype(np.float64))
    with np.errstate(all="ignore"):
        k0 = res["firstHitPoint"] - np.asarray(spec["tx"]["origin"], np.float64); k0 /= np.linalg.norm(k0, axis=1, keepdims=True)
        a1 = g["rcs_angle"][:len(prim), 0, 0] - np.arctan2(k0[:, 1], k0[:, 0]); e1 = g["rcs_angle"][:len(prim), 0, 1] - np.arctan2(k0[:, 2], np.hypot(k0[:, 0], k0[:, 1]))
    d = -np.stack([np.cos(e1) * np.cos(a1), np.cos(e1) * np.sin(a1), np.sin(e1)], axis=1)
    d = np.where(hit[:, None], d, 0.0)
    pi = np.where(hit, prim, 0)
    p = P[pi]
    e0 = p[:, 1] - p[:, 0]
    n = np.cross(p[:, 0] - p[:, 2], e0)
    w = np.cross(n, e0)
    dn = np.einsum("ij,ij->i", d, n); dl = np.linalg.norm(d, axis=1); nl = np.linalg.norm(n, axis=1)
    with np.errstate(all="ignore"):
        du = np.einsum("ij,ij->i", d, e0) / np.linalg.norm(e0, axis=1); dw = np.einsum("ij,ij->i", d, w) / np.linalg.norm(w, axis=1)
        az = np.arctan2(dw, du)
        c = np.abs(dn) / (dl * nl)
        side = np.where(dn > 0, 0, 1)
        delta = ht * 2.0 ** -22 + (np.abs(o).max(axis=1) + ht) * 2.0 ** -45
        reach = dl * TMIN
        e = E[targ[pi]]
        h0 = np.float32(H0 * e).astype(np.float64) * np.float64(np.float32(1.000001)); rho = np.float32(RHO * e).astype(np.float64) * np.float64(np.float32(0.999999))
    by = hzs[pi, side].astype(np.float64) * (1.0 / 255.0)            # [rays][4], RTS_HZ_DECODE
    near = boundary_distance(az) <= AZ_EXCLUDE
    bounced = hit & (res["reflDepth"] >= 1)
    return dict(c=c, delta=delta, reach=reach, h0=h0, rho=rho, by=by, az=az, near=near & bounced, bounced=bounced, du=du, dw=dw)


def boundary_distance(az):
    """how far [rad] an in-plane azimuth is from the nearest quadrant boundary"""
    return np.abs(az / (math.pi / 2) - np.round(az / (math.pi / 2))) * (math.pi / 2)


def quadrant(az):
    return np.where(np.cos(az) < 0, 1, 0) | np.where(np.sin(az) < 0, 2, 0)


def rule_eval(r, slack, S):
    """the three inequalities with a given S per launch index; slack > 0 tightens, < 0 loosens (relative), as in rule_counts"""
    k = 1.0 + slack
    with np.errstate(all="ignore"):
        return (r["c"] - r["delta"] / r["reach"] > (S + MARGIN) * k) & (r["c"] * r["reach"] >= 2.0 * (r["h0"] + r["delta"]) * k) & (4.0 * r["delta"] * k <= r["rho"]) & r["bounced"]


def sector_S(r, shift=0.0):
    q = quadrant(r["az"] + shift)
    return np.take_along_axis(r["by"], q[:, None], axis=1)[:, 0]


def counts(r, slack):
    """(isotropic, by a sector only) with every inequality tightened (slack > 0) or loosened: a sector-only skip is one the isotropic
    rule does NOT take, so its tightened count takes the loosened isotropic rule's complement and the other way round"""
    iso = rule_eval(r, slack, r["by"].max(axis=1))
    sec = rule_eval(r, slack, sector_S(r)) & ~rule_eval(r, -slack, r["by"].max(axis=1))
    return iso & ~r["near"], sec & ~r["near"]


def named_by_sector_rule(r):
    """every launch index the loosened sector rule could name -- near a quadrant boundary by either neighbour"""
    return rule_eval(r, -1e-5, sector_S(r)) | rule_eval(r, -1e-5, sector_S(r, AZ_EXCLUDE)) | rule_eval(r, -1e-5, sector_S(r, -AZ_EXCLUDE))


# ------------------------------------------------------------------------------------------------ the comparison
_cache = {}
WAYS = (("sec", dict()), ("iso", dict(horizon_sectors=False)), ("off", dict(horizon=False)))


def run(env, name):
    """oracle brute force once; the counting KEEP_ALL build with sectors, with the isotropic rule only, and without the horizon"""
    if name in _cache:
        return _cache[name]
    api, scenes, O, H = env
    spec = make_spec(scenes, api, name)
    n = spec["W"] ** 3
    out = dict(spec=spec, o=H.oracle_trace(O, spec), n=n)
    n_prims = sum(len(m["tris"]) for m in spec["meshes"])
    for key, kw in WAYS:
        tr = H.gpu_tracer(api, spec, keep_all=True, count_traversal=True, **kw)
        _, st = H.gpu_trace(api, spec, tr=tr)
        out[key] = dict(g=tr.all_rays(n), st=st, recv=tr.received(), walk=tr.walk_stats(), hz=tr.horizon(n_prims), hzs=tr.horizon_sectors(n_prims), info=tr.scene_info())
        tr.close()
    _cache[name] = out
    return out


def check_identical(env, r):
    H = env[3]
    for key, _ in WAYS:
        H.compare_full(r["o"], r[key]["g"], r["n"])
    a = r["sec"]
    for key in ("iso", "off"):
        b = r[key]
        for f in ("rays", "segments", "shaded", "received"):
            assert a["st"][f] == b["st"][f], (key, f, a["st"][f], b["st"][f])
        assert np.array_equal(a["recv"]["slots"], b["recv"]["slots"]) and np.array_equal(a["recv"]["path"], b["recv"]["path"])
        H.assert_prd_equal(a["recv"]["results"], b["recv"]["results"], "received sets")
        assert np.array_equal(a["g"]["hit_prim"], b["g"]["hit_prim"]) and np.array_equal(a["g"]["hit_t"].view(np.uint32), b["g"]["hit_t"].view(np.uint32))
        assert np.array_equal(a["hzs"], b["hzs"]) and np.array_equal(a["hz"], b["hz"])      # the build does not depend on the flags
    assert len(a["walk"]) == 12
    assert r["off"]["walk"][5] == 0 and r["off"]["walk"][11] == 0      # RTS_FLAG_NO_HORIZON: nothing skips
    assert r["iso"]["walk"][11] == 0 and r["iso"]["walk"][5] == a["walk"][5]      # RTS_FLAG_NO_HORIZON_SECTORS: the isotropic rule alone, and it is tested first
    for lo, hi in (("sec", "iso"), ("iso", "off")):
        assert r[lo]["st"]["tri_tests"] <= r[hi]["st"]["tri_tests"] and r[lo]["st"]["node_visits"] <= r[hi]["st"]["node_visits"]
    print("%s: segments %d shaded %d received %d | skipped walks: isotropic %d, by a sector only %d | node visits %d -> %d -> %d, triangle tests %d -> %d -> %d (off, isotropic, sectors)" % (
        r["spec"]["name"], a["st"]["segments"], a["st"]["shaded"], a["st"]["received"], a["walk"][5], a["walk"][11],
        r["off"]["st"]["node_visits"], r["iso"]["st"]["node_visits"], a["st"]["node_visits"], r["off"]["st"]["tri_tests"], r["iso"]["st"]["tri_tests"], a["st"]["tri_tests"]))


def check_counts(env, r):
    """one bounce: both device counts lie between the restated rule tightened and loosened by 1e-5 (the restated direction's
    length); at most 1 % of the bounce segments are left out for an azimuth within 1e-6 rad of a quadrant boundary; and no launch
    index whose bounce segment meets its own target again (the oracle's second hit record) is named by either rule"""
    scenes = env[1]
    a = r["sec"]
    parts = rule_parts(scenes, r["spec"], a["g"], a["hzs"])
    iso_t, sec_t = counts(parts, 1e-5); iso_l, sec_l = counts(parts, -1e-5)
    near = int(parts["near"].sum()); bounces = int(parts["bounced"].sum())
    # the excluded launch indices may have gone either way on the device: each adds one to the upper bracket of the rule that could name it
    near_iso = int((rule_eval(parts, -1e-5, parts["by"].max(axis=1)) & parts["near"]).sum()); near_sec = int((named_by_sector_rule(parts) & parts["near"]).sum())
    print(r["spec"]["name"], "isotropic rule: %d .. %d, device %d | sector only: %d .. %d, device %d | bounce segments %d, within 1e-6 rad of a boundary %d" % (
        iso_t.sum(), iso_l.sum() + near_iso, a["walk"][5], sec_t.sum(), sec_l.sum() + near_sec, a["walk"][11], bounces, near))
    assert near <= 0.01 * bounces, (near, bounces)
    assert iso_t.sum() <= a["walk"][5] <= iso_l.sum() + near_iso
    assert sec_t.sum() <= a["walk"][11] <= sec_l.sum() + near_sec
    again = r["o"]["hit_prim"][:, 1] >= 0
    P, targ, _ = B.world_tris(scenes, r["spec"])
    same = again & (targ[np.where(again, r["o"]["hit_prim"][:, 1], 0)] == targ[np.where(r["o"]["hit_prim"][:, 0] >= 0, r["o"]["hit_prim"][:, 0], 0)])
    named = named_by_sector_rule(parts) | rule_eval(parts, -1e-5, parts["by"].max(axis=1))
    assert not np.any(named & same), "a bounce segment that meets its own target again would have skipped that target's walk"
    return parts, same


@pytest.mark.parametrize("name", ["fin", "finrot", "finecef", "corner2", "corner3", "cross"])
def test_results_identical_with_sectors_isotropic_and_off(env, name):
    check_identical(env, run(env, name))


@pytest.mark.parametrize("name", ["fin1", "finrot1", "finecef1", "cross1"])
def test_body_with_a_fin_skips_by_sector(env, name):
    r = run(env, name)
    check_identical(env, r)
    check_counts(env, r)
    if name.startswith("fin"):
        assert r["sec"]["walk"][11] > 0                            # a test that passes because nothing engages proves nothing
        by = r["sec"]["hzs"]
        one_sided = ((by.max(axis=2) > 0) & (by.min(axis=2) == 0)).sum()
        print(name, "sides with the mesh over their plane in some quadrants only: %d of %d" % (one_sided, by.shape[0] * 2))
        assert one_sided > 0


@pytest.mark.parametrize("name", ["postu1", "postw1"])
def test_post_on_a_quadrant_boundary(env, name):
    """the case eps_az exists for: reflected rays leave the plate exactly along a quadrant boundary of its triangles' frames and hit
    the post that stands there"""
    r = run(env, name)
    check_identical(env, r)
    parts, same = check_counts(env, r)
    _, _, _, n_plate = post_mesh(env[1], name[4])
    o = r["o"]
    on_post = (o["hit_prim"][:, 0] >= 0) & (o["hit_prim"][:, 0] < n_plate) & (o["hit_prim"][:, 1] >= n_plate)
    print(name, "bounce segments off the plate that hit the post: %d; smallest |azimuth off the boundary| among them %.3g rad" % (
        on_post.sum(), float(boundary_distance(parts["az"][on_post]).min()) if on_post.any() else float("nan")))
    assert on_post.sum() > 0
    assert not np.any(named_by_sector_rule(parts) & on_post)
    assert r["sec"]["walk"][11] > 0                                # the rule is engaged on this plate: rays that land beyond the post go by their sector alone


@pytest.mark.parametrize("name", ["corner21", "corner31"])
def test_corner_reflectors(env, name):
    r = run(env, name)
    check_identical(env, r)
    _, same = check_counts(env, r)
    assert same.sum() > 0                                          # the reflector does what it is for: bounce rays MUST hit again
    assert r["sec"]["walk"][5] == 0                                # (the inner sides are closed for the isotropic rule; a ray leaving away from the other plate is free to go by its sector)


def test_icosphere_bytes_and_decoded_maxima(env):
    r = run(env, "ico3f1")
    check_identical(env, r)
    check_counts(env, r)
    by = r["sec"]["hzs"]; hz = r["sec"]["hz"]
    outward = by.reshape(len(by), 2, 4).max(axis=2).min(axis=1)
    assert np.all(outward == 0)                                    # every outward byte is 0 ...
    inward = np.where(by.max(axis=2)[:, :1] == 0, by[:, 1], by[:, 0])
    assert np.all(inward == 255)                                   # ... and every inward byte 255
    dec = by.max(axis=2).astype(np.float64) / 255.0
    assert np.all(hz.astype(np.float64) >= dec) and np.all(hz.astype(np.float64) <= dec * (1 + 2.0 ** -23)) and np.all((hz == 0) == (dec == 0)) and np.all((hz == 1) == (dec == 1))
    assert r["sec"]["walk"][11] == 0 and r["sec"]["walk"][5] > 0   # a convex mesh escapes by the isotropic rule alone


def test_lone_plate_and_degenerate_mesh_never_skip(env):
    g = run(env, "graze1")
    check_identical(env, g)
    assert g["sec"]["st"]["shaded"] > 0 and g["sec"]["walk"][5] == 0 and g["sec"]["walk"][11] == 0
    assert np.all(g["sec"]["hzs"] == 0)
    d = run(env, "degen1")
    check_identical(env, d)
    assert d["sec"]["st"]["shaded"] > 0 and d["sec"]["walk"][5] == 0 and d["sec"]["walk"][11] == 0
    assert np.all(d["sec"]["hzs"] == 255)


# ------------------------------------------------------------------------------------------------ the bound itself
def brute_sectors(v, t, h0):
    """numpy brute force of sup h(x) / |x - q| per primitive, side and UN-WIDENED quadrant: x over a barycentric lattice of every other
    triangle (heights above h0 only), q over the lattice of the triangle itself (rho = 0); the quadrant of (x - q) by the signs the
    kernel tests.  A lower bound of what S_k must cover, as brute_horizon is for S"""
    k = 4
    wts = np.array([[i, j, k - i - j] for i in range(k + 1) for j in range(k + 1 - i)], np.float64) / k
    p = v[t.astype(np.int64)]
    X = np.einsum("sa,nad->nsd", wts, p)
    e0 = p[:, 1] - p[:, 0]
    nrm = np.cross(p[:, 0] - p[:, 2], e0); nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
    u = e0 / np.linalg.norm(e0, axis=1, keepdims=True); w = np.cross(nrm, u)
    out = np.zeros((len(t), 2, 4))
    allx = X.reshape(-1, 3); owner = np.repeat(np.arange(len(t)), wts.shape[0])
    for i in range(len(t)):
        h = (allx - p[i, 0]) @ nrm[i]
        for side, hs in ((0, h), (1, -h)):
            m = (hs > h0) & (owner != i)
            if not m.any():
                continue
            dv = allx[m][:, None, :] - X[i][None, :, :]
            dist = np.linalg.norm(dv, axis=2)
            q = np.where(dv @ u[i] < 0, 1, 0) | np.where(dv @ w[i] < 0, 2, 0)
            with np.errstate(divide="ignore"):
                ratio = hs[m][:, None] / dist
            for s in range(4):
                sel = q == s
                if sel.any():
                    out[i, side, s] = min(1.0, float(ratio[sel].max()))
    return out


@pytest.mark.parametrize("name", ["fin1", "corner31", "cross1"])
def test_every_sector_bounds_the_brute_force(env, name):
    r = run(env, name)
    m = r["spec"]["meshes"][0]
    v = np.asarray(m["verts"], np.float64); t = np.asarray(m["tris"], np.uint32)
    used = v[np.unique(t.astype(np.int64))]
    ref = brute_sectors(v, t, H0 * float(np.linalg.norm(used.max(axis=0) - used.min(axis=0))))
    dec = r["sec"]["hzs"].astype(np.float64) / 255.0
    assert dec.shape == ref.shape
    assert np.all(dec >= ref), (int((dec < ref).sum()), float((ref - dec).max()))
    print(name, "sector bytes: 0 on %d of %d, 255 on %d; brute force 0 on %d; mean slack of the open sectors %.3f" % (
        (dec == 0).sum(), dec.size, (dec == 1).sum(), (ref == 0).sum(), float((dec - ref)[dec < 1].mean()) if (dec < 1).any() else 0.0))
