"""Every hierarchy builder over every edge mesh (-m gpu): the host builder, the device's binned-SAH tree with and without split
references, with crowding rounds and with the gain rule off, and the Morton / Karras tree (k_morton, k_hierarchy, k_refit, the
non-compacted k_collapse4) -- each held to the structural invariants of tests/bvh_check.py (exact comparisons, proved on the CPU
by tests/test_bvh_check_host.py) at the sizes where the code changes behaviour: 1..5 references, the 256-thread block edge, the
1024-leaf refit chunk edge, coincident centroids and equal Morton codes, invalid triangles, empty and single-triangle meshes
between others.  A failed device build is an error here (RTS_DEVICE_BUILD_FALLBACK=0), never a host tree.  Then the walk over
these trees: one launch per variant against the oracle's brute force, closest hits identical across all seven."""
import numpy as np
import pytest

import bvh_check as B
import helpers as H

pytestmark = pytest.mark.gpu

#             RTS_BUILDER  RTS_DEVICE_TREE  RTS_SPLIT_BUDGET  RTS_CROWD_ROUNDS  RTS_REF_GAIN_RULE
VARIANTS = {"host":       ("host",   "sah",  "2", "0", "1"),
            "sah":        ("device", "sah",  "2", "0", "1"),       # the default
            "sah-b0":     ("device", "sah",  "0", "0", "1"),       # one reference per triangle
            "sah-crowd":  ("device", "sah",  "2", "2", "1"),
            "sah-cutall": ("device", "sah",  "2", "0", "0"),
            "lbvh":       ("device", "lbvh", "2", "0", "1"),
            "lbvh-b0":    ("device", "lbvh", "0", "0", "1")}
W, MAX_REFL = 8, 2


def pin(monkeypatch, variant):
    """every per-scene switch of the table pinned (nothing leaks in from outside), a failed device build an error"""
    for k, v in zip(("RTS_BUILDER", "RTS_DEVICE_TREE", "RTS_SPLIT_BUDGET", "RTS_CROWD_ROUNDS", "RTS_REF_GAIN_RULE"), VARIANTS[variant]):
        monkeypatch.setenv(k, v)
    monkeypatch.setenv("RTS_DEVICE_BUILD_FALLBACK", "0")
    monkeypatch.delenv("RTS_DEBUG_FAIL_DEVICE_BUILD", raising=False)


def build_and_check(rts, tr, variant, meshes, what):
    """set_scene, bvh(), check_hierarchy, the scene's totals; returns the arrays and the per-mesh figures"""
    tr.set_scene(meshes)
    info = tr.scene_info()
    assert info["builder"] == (0 if variant == "host" else 1), "the scene was built by builder %d" % info["builder"]
    nodes, leaf, roots = tr.bvh()
    assert info["n_nodes"] == len(nodes) and info["n_leaves"] == len(leaf) and info["n_targets"] == len(roots) == len(meshes)
    fig = B.check_hierarchy(nodes, leaf, roots, meshes, max_refs=None if variant == "host" else 8, all_reachable=not variant.startswith("lbvh"))
    for t, f in enumerate(fig):
        print("%-10s %-10s mesh %d: %5d records reachable, %5d slots, max refs %d, depth %d" % (variant, what, t, f["nodes"], f["slots"], f["max_refs"], f["depth"]))
    print("%-10s %-10s scene: %d records, %d reachable, %d slots" % (variant, what, len(nodes), sum(f["nodes"] for f in fig), len(leaf)))
    _, prim_mesh, valid = B.triangle_table(meshes)
    if VARIANTS[variant][2] == "0":                                          # one reference per triangle: nv is exactly the valid triangle count
        for t, f in enumerate(fig):
            assert f["slots"] == int(valid[prim_mesh == t].sum()) and f["max_refs"] <= 1
    return (nodes, leaf, roots), fig


_slots_of_huge = {}


@pytest.mark.parametrize("name", list(B.CASES))
@pytest.mark.parametrize("variant", list(VARIANTS))
def test_structure(rts, monkeypatch, variant, name):
    pin(monkeypatch, variant)
    meshes = B.case_meshes(name)
    tr = rts.Tracer(W, MAX_REFL, 0, True, keep_all=True)
    (nodes, leaf, roots), fig = build_and_check(rts, tr, variant, meshes, name)
    refs = np.bincount(leaf, minlength=sum(len(m["tris"]) for m in meshes))
    if name == "huge260":
        _slots_of_huge[variant] = len(leaf)
        if variant in ("sah", "lbvh", "sah-cutall"):
            assert refs.max() > 1, "no primitive of the huge-triangle mesh has more than one slot"
    if name == "degen32":
        assert (refs[list(B.DEGENERATE_PRIMS)] == 1).all()                   # the point and the collinear triangle: valid, one reference each
    # the same scene once more on the same handle: every atomic of the builders is a min, a max or a counter
    tr.set_scene(meshes)
    nodes2, leaf2, roots2 = tr.bvh()
    assert np.array_equal(roots, roots2) and np.array_equal(leaf, leaf2), "the second build's leaf order differs at %d of %d slots" % ((leaf != leaf2).sum() if len(leaf) == len(leaf2) else -1, len(leaf))
    assert nodes.shape == nodes2.shape and np.array_equal(nodes.view(np.uint32), nodes2.view(np.uint32)), "the second build's records differ"
    tr.close()


def test_split_variants_add_references(rts, monkeypatch):
    """the huge-triangle mesh: cutting whether or not it pays, and crowding rounds, give at least the slots of the default; the
    default and the Morton tree give more than one per triangle (else the variants prove nothing)"""
    meshes = B.case_meshes("huge260")
    n_tris = len(meshes[0]["tris"])
    for variant in ("sah", "sah-crowd", "sah-cutall", "sah-b0", "lbvh"):
        if variant not in _slots_of_huge:                                    # (run alone: build what test_structure has not)
            pin(monkeypatch, variant)
            tr = rts.Tracer(W, MAX_REFL, 0, True)
            (_, leaf, _), _ = build_and_check(rts, tr, variant, meshes, "huge260")
            _slots_of_huge[variant] = len(leaf)
            tr.close()
    s = _slots_of_huge
    print("slots on the huge-triangle mesh:", s)
    assert s["sah-b0"] == n_tris < s["sah"] and s["lbvh"] > n_tris
    assert s["sah-cutall"] >= s["sah"] and s["sah-crowd"] >= s["sah"]


# ------------------------------------------------------------------------------------------------ the walk over these trees
def walk_spec(api, scenes, name):
    """the case as a scene of the parity tests: aimed the way the soup test aims (from 300 m down the x axis, two receivers), the
    beam fitted to the valid triangles' extent so that rays are shaded whatever the mesh's size"""
    meshes = B.case_meshes(name)
    positions = B.FIVE_POSITIONS if name == "five" else ((0.0, 0.0, 0.0),) * len(meshes)
    pts = []
    for m, p in zip(meshes, positions):
        tv, _, valid = B.triangle_table([m])
        pts.append(tv[valid].reshape(-1, 3) + np.asarray(p))
    pts = np.concatenate(pts)
    lo, hi = pts.min(axis=0), pts.max(axis=0)
    if len(pts) >= 96:                                                       # the bulk of a soup: its few long slivers would thin the beam out
        lo, hi = np.percentile(pts, 10, axis=0), np.percentile(pts, 90, axis=0)
    c = 0.5 * (lo + hi); half = np.maximum(0.5 * (hi - lo), 1e-6)
    spec = scenes.config1()
    spec.update(W=W, max_refl=MAX_REFL, smooth=True, meshes=meshes,
                motion=[dict(position=tuple(p), velocity=(0.0, 0.0, 0.0)) for p in positions])
    dist = 300.0 + (c[0] - lo[0])
    spec["tx"] = dict(origin=tuple(c + (-300.0, 0.0, 0.0)), span=(2.2 * half[1] / dist, 2.2 * half[2] / dist, 0.08), dir=(0.0, 0.0))      # (azimuth, elevation, stretch)
    spec["rx"] = [api.rx_sphere(tuple(c + (-300.0, 2.0, 1.0)), 0.0, 0.0, 120.0, 2.6, 2.6), api.rx_sphere(tuple(c + (-100.0, 200.0, 30.0)), -1.1, -0.1, 150.0, 2.6, 2.6)]
    return spec


@pytest.mark.parametrize("name", B.WALK_CASES)
def test_walk(rts, oracle, scenes, monkeypatch, name):
    """one keep_all launch of 512 rays per variant against the oracle's brute-force closest hit (computed once per mesh), and the
    closest-hit primitives and the bits of their distances identical across the seven variants"""
    spec = walk_spec(rts, scenes, name)
    n = W ** 3
    o = H.oracle_trace(oracle, spec)
    assert o["counters"]["shaded"] > 0, "the beam misses the mesh: the comparison would be vacuous"
    first = None
    for variant in VARIANTS:
        pin(monkeypatch, variant)
        tr, st = H.gpu_trace(rts, spec)
        assert tr.scene_info()["builder"] == (0 if variant == "host" else 1)
        g = tr.all_rays(n)
        H.compare_full(o, g, n)
        assert st["shaded"] == o["counters"]["shaded"] and st["segments"] == o["counters"]["segments"]
        print("%-10s %-10s %d of %d rays hit, %d shaded" % (variant, name, (g["hit_prim"][:, 0] >= 0).sum(), n, st["shaded"]))
        if first is None:
            first = g
        assert np.array_equal(first["hit_prim"], g["hit_prim"]) and np.array_equal(first["hit_t"].view(np.uint32), g["hit_t"].view(np.uint32)), variant
        tr.close()


@pytest.fixture(scope="module")
def scenes():
    from rts_amd import scenes as S
    return S
