"""The horizon (rts_horizon.hip, rts_shade): a bounce ray that leaves its triangle above the triangle's horizon skips the walk of the
target it left.  Results must be what the oracle's brute force computes and what the same launches give with RTS_FLAG_NO_HORIZON:
received sets, per-ray records, the hit records of every depth (primitive and f32 t), segments / shaded / received.  And the rule must
actually fire where it can and never where the oracle shows a second hit: the counting build's count of skipped walks is compared with
a restatement of the rule in numpy on the launch's own hit records (one-bounce launches, where every bounce segment's origin,
direction and triangle can be read off the full per-ray output)."""
import math
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

pytestmark = pytest.mark.gpu

H0, RHO, MARGIN, TMIN = 2.0 ** -20, 2.0 ** -8, 2.0 ** -8, 0.005      # rts_internal.h: RTS_HZ_H0, RTS_HZ_RHO, RTS_HZ_MARGIN; SCENE_EPS_R


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
def grid_plate(origin, eu, ev, k, normal):
    """a plate origin + a eu + b ev, a, b in [0, 1], as k x k cells of two triangles, shared vertices, one normal per vertex"""
    o, eu, ev = (np.asarray(x, np.float64) for x in (origin, eu, ev))
    a = np.linspace(0.0, 1.0, k + 1)
    v = np.array([o + x * eu + y * ev for y in a for x in a])
    t = []
    for j in range(k):
        for i in range(k):
            p = j * (k + 1) + i
            t += [[p, p + 1, p + k + 2], [p, p + k + 2, p + k + 1]]
    return v, np.array(t, np.uint32), np.tile(np.asarray(normal, np.float64), (v.shape[0], 1))


def corner_mesh(scenes, n_plates, L=6.0, k=6):
    """two or three plates at right angles, ONE mesh; its opening -- the (1, 1, 1) diagonal -- turned towards -x"""
    parts = [grid_plate((0, 0, 0), (L, 0, 0), (0, L, 0), k, (0, 0, 1)), grid_plate((0, 0, 0), (0, L, 0), (0, 0, L), k, (1, 0, 0))]
    if n_plates == 3:
        parts.append(grid_plate((0, 0, 0), (0, 0, L), (L, 0, 0), k, (0, 1, 0)))
    v, t, n = scenes._merge(parts)
    u = np.array([1.0, 1.0, 1.0]) / math.sqrt(3.0); w = np.array([1.0, -1.0, 0.0]) / math.sqrt(2.0)
    R = np.array([-u, w, np.cross(-u, w)])
    return v @ R.T, t, n @ R.T


def one_mesh_spec(scenes, name, mesh, W, max_refl, smooth=True, span=(0.08, 0.08, 0.05), refl=0.9):
    v, t, n = mesh
    return dict(name=name, W=W, max_refl=max_refl, smooth=smooth, n_pulses=1,
                meshes=[dict(tris=t, verts=v, normals=n, refl_coeff=refl, refr_index=1.0)],
                motion=scenes._static_motion(1, [(0.0, 0.0, 0.0)], [(5.0, 0.0, 0.0)]),
                tx=dict(origin=(-200.0, 0.0, 0.0), span=span, dir=(0.0, 0.0)),
                rx=[scenes._rx_at((-200.0, 0.0, 0.0), (0, 0, 0), 90.0, 2.6), scenes._rx_at((-150.0, 130.0, 10.0), (0, 0, 0), 90.0, 2.6)],
                carrier=scenes.FC, c=scenes.C0)


def make_spec(scenes, api, name):
    if name.startswith("ico"):                                   # ico<subdiv><s|f>[1]: icosphere, smooth / flat normals, a trailing 1: one bounce
        s = scenes.config2(subdiv=int(name[3]), W=24, rx_radius=400.0)
        s["smooth"] = name[4] == "s"
        s["max_refl"] = 1 if name.endswith("1") else 4
        return s
    if name.startswith("multi"):
        return scenes.config_multi(W=16, max_refl=1 if name.endswith("1") else 4)
    if name.startswith("corner"):                                # corner<2|3>[1]
        return one_mesh_spec(scenes, name, corner_mesh(scenes, int(name[6])), 24, 1 if name.endswith("1") else 4, span=(0.06, 0.06, 0.05))
    if name.startswith("cross"):                                 # two crossing ellipsoids in one mesh: concave creases where they meet
        m = scenes._merge([scenes._ico_ellipsoid(2, (6.0, 1.5, 1.5)), scenes._ico_ellipsoid(2, (1.5, 6.0, 1.2), centre=(0.5, 0.0, 0.3))])
        return one_mesh_spec(scenes, name, m, 24, 1 if name.endswith("1") else 4, span=(0.07, 0.07, 0.05))
    if name.startswith("rot"):                                   # every target of the three-target scene turned by its placement
        s = scenes.config_multi(W=16, max_refl=1 if name.endswith("1") else 4)
        s["motion"] = [dict(m, rotation=tuple(api.rotation_matrix(0.3 + 0.4 * i, -0.2 * i, 0.15).ravel())) for i, m in enumerate(s["motion"])]
        return s
    if name.startswith("ecef"):
        return scenes.translate(make_spec(scenes, api, "multi" + name[4:]), scenes.ecef_offset(lat=0.6, lon=-1.1))
    if name.startswith("graze"):                                 # a plate seen almost edge-on: |c| below the height condition at this range
        v, t, n = grid_plate((0, -4, -4), (0, 8, 0), (0, 0, 8), 4, (-1, 0, 0))
        Rz = api.rotation_matrix(math.radians(85.0), 0.0, 0.0).reshape(3, 3)      # sine of the elevation 0.087; at 2 km the height condition asks for ~0.2
        s = one_mesh_spec(scenes, name, (v @ Rz.T, t, n @ Rz.T), 24, 1)
        s["tx"] = dict(s["tx"], origin=(-2000.0, 0.0, 0.0), span=(0.005, 0.005, 0.05))
        return s
    if name.startswith("degen"):                                 # the icosphere with one zero-area triangle: the mesh's horizon is off
        s = make_spec(scenes, api, "ico2s1")
        m = s["meshes"][0]
        s["meshes"] = [dict(m, tris=np.concatenate([np.asarray(m["tris"], np.uint32), np.array([[0, 0, 1]], np.uint32)]))]
        return s
    raise KeyError(name)


# ------------------------------------------------------------------------------------------------ the rule, restated
def world_tris(scenes, spec):
    """[n_prims][3][3] world-space vertices, [n_prims] target, by global primitive id; per target the extent of the LOCAL mesh"""
    P, T, E = [], [], []
    for k, (m, mo) in enumerate(zip(spec["meshes"], spec["motion"])):
        vw, _ = scenes.world_vertices(m, mo)
        P.append(vw[np.asarray(m["tris"], np.int64)]); T += [k] * len(m["tris"])
        v = np.asarray(m["verts"], np.float64)[np.unique(np.asarray(m["tris"], np.int64))]
        E.append(float(np.linalg.norm(v.max(axis=0) - v.min(axis=0))))
    return np.concatenate(P), np.array(T), np.array(E)


def rule_counts(scenes, spec, g, hz, slack):
    """one-bounce launch: which launch indices' bounce segment skips its target's walk by the rule (rts_shade), from the full per-ray
    output g and the device's horizon hz.  slack > 0 tightens, < 0 loosens every inequality (relative): the device's count must lie
    between the two.  Returns the boolean array."""
    P, targ, E = world_tris(scenes, spec)
    prim = g["hit_prim"][:, 0].astype(np.int64)
    hit = prim >= 0
    res = g["results"]
    o = res["prevHitPoint"]; ht = np.abs(g["hit_t"][:, 0].astype(np.float64))
    # the bounce direction: the record does not keep it, the RCS angles of depth 0 do -- sph(k0) + sph(-k1) with k0 the primary's unit
    # direction (towards the first hit point) and k1 the reflected one; good to ~1e-12 rad, its length 1 where the device's is 1 +- 1e-6
    with np.errstate(all="ignore"):
        k0 = res["firstHitPoint"] - np.asarray(spec["tx"]["origin"], np.float64); k0 /= np.linalg.norm(k0, axis=1, keepdims=True)
        a1 = g["rcs_angle"][:len(prim), 0, 0] - np.arctan2(k0[:, 1], k0[:, 0]); e1 = g["rcs_angle"][:len(prim), 0, 1] - np.arctan2(k0[:, 2], np.hypot(k0[:, 0], k0[:, 1]))
    d = -np.stack([np.cos(e1) * np.cos(a1), np.cos(e1) * np.sin(a1), np.sin(e1)], axis=1)
    d = np.where(hit[:, None], d, 0.0)
    p = P[np.where(hit, prim, 0)]
    n = np.cross(p[:, 0] - p[:, 2], p[:, 1] - p[:, 0])
    dn = np.einsum("ij,ij->i", d, n); dl = np.linalg.norm(d, axis=1); nl = np.linalg.norm(n, axis=1)
    with np.errstate(all="ignore"):
        c = np.abs(dn) / (dl * nl)
        S = np.where(dn > 0, hz[np.where(hit, prim, 0), 0], hz[np.where(hit, prim, 0), 1]).astype(np.float64)
        delta = ht * 2.0 ** -22 + (np.abs(o).max(axis=1) + ht) * 2.0 ** -45
        reach = dl * TMIN
        e = E[targ[np.where(hit, prim, 0)]]
        h0 = np.float32(H0 * e).astype(np.float64) * np.float64(np.float32(1.000001)); rho = np.float32(RHO * e).astype(np.float64) * np.float64(np.float32(0.999999))
        k = 1.0 + slack
        ok = (c - delta / reach > (S + MARGIN) * k) & (c * reach >= 2.0 * (h0 + delta) * k) & (4.0 * delta * k <= rho)
    bounced = hit & (res["reflDepth"] >= 1)
    return ok & bounced


# ------------------------------------------------------------------------------------------------ the comparison
_cache = {}


def run(env, name):
    """oracle brute force once; the counting KEEP_ALL build with the horizon and without it"""
    if name in _cache:
        return _cache[name]
    api, scenes, O, H = env
    spec = make_spec(scenes, api, name)
    n = spec["W"] ** 3
    o = H.oracle_trace(O, spec)
    out = dict(spec=spec, o=o, n=n)
    for key, on in (("on", True), ("off", False)):
        tr = H.gpu_tracer(api, spec, keep_all=True, count_traversal=True, horizon=on)
        _, st = H.gpu_trace(api, spec, tr=tr)
        out[key] = dict(g=tr.all_rays(n), st=st, recv=tr.received(), walk=tr.walk_stats(), hz=tr.horizon(sum(len(m["tris"]) for m in spec["meshes"])), info=tr.scene_info())
        tr.close()
    _cache[name] = out
    return out


def check_identical(env, r):
    H = env[3]
    for key in ("on", "off"):
        H.compare_full(r["o"], r[key]["g"], r["n"])
    a, b = r["on"], r["off"]
    for f in ("rays", "segments", "shaded", "received"):
        assert a["st"][f] == b["st"][f], (f, a["st"][f], b["st"][f])
    assert np.array_equal(a["recv"]["slots"], b["recv"]["slots"]) and np.array_equal(a["recv"]["path"], b["recv"]["path"])
    H.assert_prd_equal(a["recv"]["results"], b["recv"]["results"], "received sets")
    assert np.array_equal(a["g"]["hit_prim"], b["g"]["hit_prim"]) and np.array_equal(a["g"]["hit_t"].view(np.uint32), b["g"]["hit_t"].view(np.uint32))
    assert b["walk"][5] == 0                                       # RTS_FLAG_NO_HORIZON: nothing skips
    assert a["st"]["tri_tests"] <= b["st"]["tri_tests"] and a["st"]["node_visits"] <= b["st"]["node_visits"]
    print("%s: segments %d shaded %d received %d | skipped walks %d | node visits %d -> %d, triangle tests %d -> %d | scene build %.2f ms, horizon %d bytes" % (
        r["spec"]["name"], a["st"]["segments"], a["st"]["shaded"], a["st"]["received"], a["walk"][5], b["st"]["node_visits"], a["st"]["node_visits"],
        b["st"]["tri_tests"], a["st"]["tri_tests"], a["info"]["build_ms"], a["info"]["horizon_bytes"]))


@pytest.mark.parametrize("name", ["ico2s", "ico3f", "multi", "corner2", "corner3", "cross", "rot", "ecef", "graze1", "degen1"])
def test_results_identical_with_and_without_the_horizon(env, name):
    check_identical(env, run(env, name))


@pytest.mark.parametrize("name", ["ico2s1", "ico3f1", "multi1", "corner21", "corner31", "cross1", "rot1", "ecef1"])
def test_skipped_walks_are_those_the_rule_names(env, name):
    """one bounce: the device's count of skipped walks lies between the rule's count with every inequality tightened and loosened
    by 1e-5 (the restated direction's length), and no launch index whose bounce segment hits again (the oracle's second hit record) is among them"""
    r = run(env, name)
    check_identical(env, r)
    scenes = env[1]
    a = r["on"]
    tight = rule_counts(scenes, r["spec"], a["g"], a["hz"], 1e-5); loose = rule_counts(scenes, r["spec"], a["g"], a["hz"], -1e-5)
    print(name, "rule: %d .. %d, device: %d, bounce segments: %d" % (tight.sum(), loose.sum(), a["walk"][5], (a["g"]["results"]["reflDepth"] >= 1).sum()))
    assert tight.sum() <= a["walk"][5] <= loose.sum()
    again = r["o"]["hit_prim"][:, 1] >= 0
    P, targ, _ = world_tris(scenes, r["spec"])
    same = again & (targ[np.where(again, r["o"]["hit_prim"][:, 1], 0)] == targ[np.where(r["o"]["hit_prim"][:, 0] >= 0, r["o"]["hit_prim"][:, 0], 0)])
    assert not np.any(loose & same), "a bounce segment that meets its own target again would have skipped that target's walk"
    if name.startswith("corner"):
        assert same.sum() > 0                                      # the reflector does what it is for: bounce rays MUST hit again
        assert a["walk"][5] == 0                                   # ... off plates whose inner sides are closed (S = 1): nothing skips
    else:
        assert a["walk"][5] > 0                                    # a test that passes because nothing ever skips proves nothing


def test_icosphere_every_eligible_bounce_skips(env):
    """a convex mesh: S = 0 on the outward side of every primitive and 1 on the inward side, so every bounce segment that passes the
    height condition skips the walk (the count against the restated rule: test_skipped_walks_are_those_the_rule_names) -- with flat
    normals at 1 km that is every bounce but those off the limb, whose elevation is below ~0.1"""
    r = run(env, "ico3f1")
    a = r["on"]
    outward = a["hz"].min(axis=1)
    assert np.all(outward == 0.0) and np.all(a["hz"].max(axis=1) == 1.0)
    bounces = int((a["g"]["results"]["reflDepth"] >= 1).sum())
    zero = a["hz"].copy(); zero[:, :] = np.where(a["hz"] == 0.0, 0.0, 1.0)
    tight = rule_counts(env[1], r["spec"], a["g"], zero, 1e-5).sum(); loose = rule_counts(env[1], r["spec"], a["g"], zero, -1e-5).sum()
    print("icosphere: %d bounce segments, %d skip (rule %d .. %d); bounce rounds %d, without any walk %d" % (bounces, a["walk"][5], tight, loose, a["walk"][8], a["walk"][7]))
    assert bounces > 100 and tight <= a["walk"][5] <= loose and a["walk"][5] >= 0.8 * bounces, (a["walk"][5], bounces)
    assert a["st"]["walked_segments"] < r["off"]["st"]["walked_segments"]


def test_grazing_plate_and_degenerate_mesh_never_skip(env):
    g = run(env, "graze1")
    assert g["on"]["st"]["shaded"] > 0 and g["on"]["walk"][5] == 0
    assert np.all(g["on"]["hz"] == 0.0)                            # a lone plate: nothing rises above its plane -- only the height condition holds the rule back
    d = run(env, "degen1")
    assert d["on"]["st"]["shaded"] > 0 and d["on"]["walk"][5] == 0
    assert np.all(d["on"]["hz"] == 1.0)


# ------------------------------------------------------------------------------------------------ the bound itself
def brute_horizon(v, t, h0):
    """numpy brute force of sup h(x) / |x - q| per primitive and side: x over a barycentric lattice of every OTHER triangle (heights
    above h0 only), q over the same lattice of the triangle itself (rho = 0: a lower bound of what S must cover)"""
    k = 4
    w = np.array([[i, j, k - i - j] for i in range(k + 1) for j in range(k + 1 - i)], np.float64) / k
    p = v[t.astype(np.int64)]                                     # [n][3][3]
    X = np.einsum("sa,nad->nsd", w, p)                            # [n][samples][3]
    nrm = np.cross(p[:, 0] - p[:, 2], p[:, 1] - p[:, 0]); nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
    out = np.zeros((len(t), 2))
    allx = X.reshape(-1, 3); owner = np.repeat(np.arange(len(t)), w.shape[0])
    for i in range(len(t)):
        h = (allx - p[i, 0]) @ nrm[i]
        for side, hs in ((0, h), (1, -h)):
            m = (hs > h0) & (owner != i)
            if not m.any():
                continue
            dist = np.linalg.norm(allx[m][:, None, :] - X[i][None, :, :], axis=2)
            with np.errstate(divide="ignore"):
                out[i, side] = min(1.0, float((hs[m][:, None] / dist).max()))
    return out


@pytest.mark.parametrize("name", ["ico2s1", "corner31", "cross1"])
def test_device_horizon_bounds_the_brute_force(env, name):
    r = run(env, name)
    m = r["spec"]["meshes"][0]
    v = np.asarray(m["verts"], np.float64); t = np.asarray(m["tris"], np.uint32)
    used = v[np.unique(t.astype(np.int64))]
    ref = brute_horizon(v, t, H0 * float(np.linalg.norm(used.max(axis=0) - used.min(axis=0))))
    hz = r["on"]["hz"].astype(np.float64)
    assert hz.shape == ref.shape and np.all(hz >= 0.0) and np.all(hz <= 1.0)
    assert np.all(hz >= ref), (int((hz < ref).sum()), float((ref - hz).max()))
    print(name, "S = 0 on %d of %d sides, S = 1 on %d; brute force: 0 on %d, mean slack of the open sides %.3f" % (
        (hz == 0).sum(), hz.size, (hz == 1).sum(), (ref == 0).sum(), float((hz - ref)[hz < 1].mean()) if (hz < 1).any() else 0.0))
    if name.startswith("ico"):
        assert np.all(hz.min(axis=1) == 0.0)                      # the outward side of a convex mesh: exactly 0
