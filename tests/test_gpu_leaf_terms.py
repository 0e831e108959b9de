"""GPU tests (-m gpu) of the leaf record that carries the triangle test's ray-free terms (RtsLeafTri: p0, e0, e1, n, written once
per pulse by k_leaves from the PLACED vertices; tri_test starts at 1 / dot(n, d)).  The terms are formed with the operands,
operations and order the test used per lane and per step, so nothing may move: every case goes through the C-ABI and is compared
record for record, bit for bit (tests/helpers.py), against the oracle's brute force over all primitives (which forms the terms
per test, like the reference) or against another launch of the library that must see the same bits.

The scene generators below only build inputs; the oracle's results are computed once per scene and shared."""
import numpy as np
import pytest

import helpers as H

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def scenes():
    from rts_amd import scenes as S
    return S


def _placements(rts, k):
    """pulse k's placement of the three targets of config_multi: every target rotated (has_rotation, the kind of motion of BASELINE
    configs[4]) and displaced, differently per pulse"""
    return [dict(position=(0.3 + 0.4 * k, 0.1 * k, -0.2), velocity=(300.0, 100.0, 0.0), rotation=rts.rotation_matrix(0.2 + 0.15 * k, 0.05 * k, -0.1 - 0.05 * k)),
            dict(position=(2.0, 9.0 - 0.5 * k, 1.0), velocity=(0.0, -500.0, 0.0), rotation=rts.rotation_matrix(-0.3 * k, 0.1, 0.2 * k)),
            dict(position=(9.0, -7.0, 0.2 * k), velocity=(0.0, 0.0, 200.0), rotation=rts.rotation_matrix(0.1, 0.0, 0.3 + 0.3 * k))]


def _received_of(o):
    idx = np.nonzero(o["results"]["received"] >= 0)[0]
    return idx, dict(results=o["results"][idx], path=o["path"][idx], rcs_angle=o["rcs_angle"][idx], slots=idx.astype(np.uint64))


def _same_received(a, b, what, exact=True):
    """two received sets, record for record.  Between two launches of the library every byte must agree; against the oracle the RCS
    angles alone have a tolerance (exact=False: libm and OCML atan2 differ in last bits, tests/test_gpu_parity.py)"""
    assert np.array_equal(a["slots"], b["slots"]), what
    assert np.array_equal(a["path"], b["path"]), what
    H.assert_prd_equal(a["results"], b["results"], what)
    if exact:
        assert a["rcs_angle"].tobytes() == b["rcs_angle"].tobytes(), what
    else:
        np.testing.assert_allclose(a["rcs_angle"], b["rcs_angle"], rtol=0, atol=1e-12)


def _all_equal(a, b, what):
    H.assert_prd_equal(a["results"], b["results"], what)
    for k in ("path", "rcs_angle", "hit_prim"):
        np.testing.assert_array_equal(a[k], b[k], err_msg="%s: %s" % (what, k))
    assert np.array_equal(a["hit_t"].view(np.uint32), b["hit_t"].view(np.uint32)), what


def _against_oracle(rts, oracle, spec, motions, what):
    """the product build and the KEEP_ALL build trace the pulses `motions` one after the other on ONE handle each; per pulse: the
    KEEP_ALL build's every launch index and the product build's received set against the oracle's brute force, and the KEEP_ALL
    build's received set against the product build's.  Returns the oracle's traces."""
    n = spec["W"] ** 3
    tk = H.gpu_tracer(rts, spec, keep_all=True)
    tp = H.gpu_tracer(rts, spec)
    out = []
    for k, mo in enumerate(motions):
        _, sk = H.gpu_trace(rts, spec, tr=tk, motion=mo)
        _, sp = H.gpu_trace(rts, spec, tr=tp, motion=mo)
        o = H.oracle_trace(oracle, spec, motion=mo)
        H.compare_full(o, tk.all_rays(n), n)
        idx, want = _received_of(o)
        assert sp["received"] == sk["received"] == len(idx), (what, k)
        assert (sp["segments"], sp["shaded"]) == (sk["segments"], sk["shaded"]) == (o["counters"]["segments"], o["counters"]["shaded"]), (what, k)
        got = tp.received()
        _same_received(want, got, "%s, pulse %d: product build against the oracle" % (what, k), exact=False)
        _same_received(got, tk.received(), "%s, pulse %d: KEEP_ALL build against the product build" % (what, k))
        out.append((o, sp))
    tk.close(); tp.close()
    return out


@pytest.mark.parametrize("smooth", [True, False])
def test_rotated_target_two_pulses(rts, oracle, scenes, smooth):
    """the terms are formed from ROTATED and translated vertices and rewritten each pulse: two consecutive pulses with different
    placements on one handle, W = 16, 3 bounces, interpolated and flat normals (flat: shading normalises the record's n)"""
    spec = scenes.config_multi(W=16, max_refl=3, smooth=smooth)
    res = _against_oracle(rts, oracle, spec, [_placements(rts, 0), _placements(rts, 1)], "rotated targets, smooth=%s" % smooth)
    for (o, st) in res:
        assert st["bvh_rebuilt"] == 1
        assert st["shaded"] > 300 and st["received"] > 20 and o["results"]["reflDepth"].max() >= 2
    a, b = res[0][0]["results"], res[1][0]["results"]
    assert not np.array_equal(a["rayLength"].view(np.uint64), b["rayLength"].view(np.uint64))       # the second pulse is another scene


def test_two_targets_perface_and_pervertex_normals(rts, oracle, scenes):
    """an icosphere (per-vertex normals, interpolated with the test's beta / gamma) and a "rect" box (per-face normals, looked up by
    the record's prim; triangle_mesh.cu:178): prim and targ sit where shading reads them -- the path columns carry targ, the
    normals are indexed by prim"""
    spec = scenes.config_multi(W=16, max_refl=3)
    spec["meshes"] = spec["meshes"][:2]
    mo = _placements(rts, 1)[:2]
    spec["motion"] = mo
    (o, st), = _against_oracle(rts, oracle, spec, [mo], "sphere + box")
    recv = o["results"]["received"] >= 0
    seen = set(np.unique(o["path"][recv]).tolist())
    assert {0, 1} <= seen, seen                                              # received paths touch BOTH targets
    hp = o["hit_prim"][:, 0]; n_sphere = spec["meshes"][0]["tris"].shape[0]
    assert ((hp >= 0) & (hp < n_sphere)).sum() > 50 and (hp >= n_sphere).sum() > 50


def degenerate_spec(scenes):
    """C1's beam (transmitter at (-1000, 0, 0) looking along +x, spans 0.02 x 0.02 rad) at W = 9.  The lattice's step is (end -
    start) / (W - 1) with start = -end in y and z: a division by 8 and a product with 4 are exact, so the middle layer lz = 4 has
    d.z = 0 EXACTLY (and the middle row ly = 4 d.y = 0).  In the beam, one mesh of seven triangles:
      0, 1  a square on its corner in the plane x = 0 whose two triangles share the edge (0, -9, 0) - (0, 9, 0): the rays of the
            middle layer run through that edge, both triangles accept them with the same t, and the tie rule on (f32 t, primitive
            id) decides;
      2, 3  a triangle whose three vertices coincide and one whose vertices are collinear, in front of the square: n = 0, the
            division gives +-inf or NaN, every comparison is false;
      4     a triangle in the plane z = 0, which holds the transmitter, in front of the square: the middle layer's rays lie in its
            plane, dot(n, d) = 0 and the test divides by zero;
      5, 6  a plate of C1's kind, 20 m wide, 5 m behind the square (what passes the square's corners is reflected there)."""
    spec = scenes.config1()
    pv, pt, pn = scenes.plate_mesh(20.0)
    verts = np.concatenate([np.array([[0.0, -9.0, 0.0], [0.0, 9.0, 0.0], [0.0, 0.0, 9.0], [0.0, 0.0, -9.0],
                                      [-2.0, 1.0, 1.0], [-2.0, 1.0, 1.0], [-2.0, 1.0, 1.0],
                                      [-3.0, -4.0, -2.0], [-3.0, 0.0, 0.0], [-3.0, 4.0, 2.0],
                                      [-6.0, -4.0, 0.0], [-6.0, 4.0, 0.0], [-1.0, 0.5, 0.0]], np.float64), pv + np.array([5.0, 0.0, 0.0])])
    tris = np.concatenate([np.array([[0, 1, 2], [0, 3, 1], [4, 5, 6], [7, 8, 9], [10, 11, 12]], np.uint32), pt + 13])
    normals = np.tile(np.array([[-1.0, 0.0, 0.0]]), (verts.shape[0], 1))
    spec.update(W=9, max_refl=2, meshes=[dict(tris=tris, verts=verts, normals=normals, refl_coeff=0.9, refr_index=1.0)])
    return spec


def test_degenerate_geometry(rts, oracle, scenes):
    """zero-area triangles, a triangle in whose plane rays lie, rays through the edge two triangles share: the outcome is the
    oracle's, hit by hit -- smooth and flat normals (flat: the normal shading normalises is the record's n), the mesh where it was
    built and moved 7 m along the beam under a placement with has_rotation (the identity: the placed vertices are exact, the
    edge stays on the rays, and the terms are formed again from other vertices)"""
    for smooth in (True, False):
        spec = degenerate_spec(scenes); spec["smooth"] = smooth
        W = spec["W"]
        moved = [dict(position=(7.0, 0.0, 0.0), velocity=(0.0, 0.0, 0.0), rotation=(1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0))]
        for (o, st) in _against_oracle(rts, oracle, spec, [spec["motion"], moved], "degenerate geometry, smooth=%s" % smooth):
            hp = o["hit_prim"][:, 0]
            idx = np.arange(W ** 3); ly, lz = (idx // W) % W, idx // (W * W)       # rayIndex = z W W + y W + x (ray_tracer.cu:151)
            assert not np.isin(hp, (2, 3, 4)).any(), "zero-area triangles and a triangle seen edge-on are never hit"
            edge = (lz == 4) & (ly >= 1) & (ly <= 7)                                 # |y| <= 7.5 m at the square, on its diagonal
            assert edge.sum() == 7 * W and (hp[edge] == 0).all(), "both triangles accept a ray through their edge: the lower primitive id wins"
            assert (hp == 0).sum() > edge.sum() and (hp == 1).sum() > 0 and (hp == 5).sum() > 0 and (hp == 6).sum() > 0 and st["received"] > 0


def test_cooperative_walk_reads_the_same_records(rts, scenes, monkeypatch):
    """the rotated scene again with EVERY tile that cost anything handed to the cooperative kernel (RTS_COOP_FRAC tiny,
    RTS_COOP_STEPS=0, as test_cooperative_units_are_invisible does), against the launch without cooperative units, bit for bit.
    Both widths of a cooperative unit: the product handle's cooperative kernel walks the octant versions with RTS_COOP_GROUP = 32
    lanes per ray (two rays per unit); with RTS_COOP_VERSIONS=0, and on a KEEP_ALL handle, a unit is one ray on 64 lanes and reads
    its records through the plain fetch.  (RTS_COOP_GROUP is a constant of the build: both widths are instantiations of ONE
    library.)  W = 42: a cost order -- and with it a cooperative head -- exists only for launches of more wave tiles than the
    grid has waves, 65 536 launch indices at RTS_GRID_MULT=1; the scene, depth and placements are the first test's."""
    monkeypatch.setenv("RTS_GRID_MULT", "1")
    spec = scenes.config_multi(W=42, max_refl=3)
    n = spec["W"] ** 3
    mo = _placements(rts, 1)
    out = {}
    for mode, env in (("off", {"RTS_COOP_FRAC": "0"}), ("group 32", {"RTS_COOP_FRAC": "1e-12"}), ("group 64", {"RTS_COOP_FRAC": "1e-12", "RTS_COOP_VERSIONS": "0"})):
        monkeypatch.setenv("RTS_COOP_FLOOR", "0"); monkeypatch.setenv("RTS_COOP_STEPS", "0"); monkeypatch.setenv("RTS_COOP_SEG", "0")
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        tk = H.gpu_tracer(rts, spec, keep_all=True)
        tp = H.gpu_tracer(rts, spec)
        for rep in range(3):                                                    # (launches 2 and 3 have a cost history)
            _, sk = H.gpu_trace(rts, spec, tr=tk, motion=mo); _, sp = H.gpu_trace(rts, spec, tr=tp, motion=mo)
        out[mode] = (tk.all_rays(n), tk.received(), sk, tp.received(), sp)
        tk.close(); tp.close()
        for k in env:
            monkeypatch.delenv(k)
    a, ra, sa, pa, spa = out["off"]
    assert sa["coop_tiles"] == 0 and spa["coop_tiles"] == 0 and spa["received"] > 100 and spa["shaded"] > 1000
    for mode in ("group 32", "group 64"):
        b, rb, sb, pb, spb = out[mode]
        assert sb["coop_tiles"] > 0 and spb["coop_tiles"] > 0, (mode, sb["coop_tiles"], spb["coop_tiles"])
        _all_equal(a, b, mode)
        _same_received(ra, rb, mode + ": KEEP_ALL build")
        _same_received(pa, pb, mode + ": product build")
        _same_received(ra, pb, mode + ": product build against the KEEP_ALL build without cooperative units")
        assert (sa["segments"], sa["shaded"], sa["received"]) == (spb["segments"], spb["shaded"], spb["received"]), mode


def test_beam_only_pulse_keeps_the_leaves(rts, oracle, scenes):
    """a pulse that only moves the BEAM after one that moved the targets: the mask-only pass runs (bvh_rebuilt == 0), the leaf
    records -- terms included -- are not rewritten; the received set is a fresh handle's, and the oracle's"""
    spec = scenes.config_multi(W=16, max_refl=3)
    mo = _placements(rts, 1)
    tx2 = dict(spec["tx"], dir=(0.02, -0.015))
    tp = H.gpu_tracer(rts, spec)
    _, st = H.gpu_trace(rts, spec, tr=tp, motion=mo)
    assert st["bvh_rebuilt"] == 1
    first = tp.received()
    spec2 = dict(spec, tx=tx2)
    _, st2 = H.gpu_trace(rts, spec2, tr=tp, motion=mo)
    assert st2["bvh_rebuilt"] == 0
    moved = tp.received()
    fresh = H.gpu_tracer(rts, spec2)
    _, st3 = H.gpu_trace(rts, spec2, tr=fresh, motion=mo)
    assert st3["bvh_rebuilt"] == 1
    _same_received(fresh.received(), moved, "beam-only pulse against a fresh handle")
    assert (st2["segments"], st2["shaded"], st2["received"]) == (st3["segments"], st3["shaded"], st3["received"])
    idx, want = _received_of(H.oracle_trace(oracle, spec2, motion=mo))
    _same_received(want, moved, "beam-only pulse against the oracle", exact=False)
    assert len(idx) > 20 and not np.array_equal(first["slots"], moved["slots"])      # the beam did move
    tp.close(); fresh.close()
