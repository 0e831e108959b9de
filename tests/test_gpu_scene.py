"""GPU tests (-m gpu) of rts_set_scene as a sequence (rts_amd/csrc/rts_scene.hip: flatten, upload, build, finish, swap): what the
sequence guarantees whichever step ends it, and what the host builder's trees look like once they have been through the device.
The cases are small on purpose: nothing here depends on size, only on which path runs."""
import numpy as np
import pytest

import helpers as H

pytestmark = pytest.mark.gpu

ONE = dict(tris=np.array([[0, 1, 2]], np.uint32), verts=np.array([[3.0, -2, -2], [3.0, 2, -2], [3.2, 0, 2.5]]), normals=np.array([[-1.0, 0, 0]] * 3), refl_coeff=0.6, refr_index=1.0)
EMPTY = dict(tris=np.zeros((0, 3), np.uint32), verts=np.zeros((0, 3)), normals=np.zeros((1, 3)), refl_coeff=0.9, refr_index=1.0)
STILL = dict(position=(-6.0, 1.0, 0.5), velocity=(0.0, 0.0, 0.0))


@pytest.fixture(scope="module")
def scenes():
    from rts_amd import scenes as S
    return S


def assert_same_rays(a, b, what):
    """two rts_get_all_rays results, bit for bit: records, paths, hit primitives and the bits of hit_t"""
    H.assert_prd_equal(a["results"], b["results"], what)
    assert np.array_equal(a["path"], b["path"]), what
    assert np.array_equal(a["hit_prim"], b["hit_prim"]), what
    assert np.array_equal(a["hit_t"].view(np.uint32), b["hit_t"].view(np.uint32)), what


def test_a_failed_set_scene_leaves_the_old_scene_in_place(rts, scenes, monkeypatch):
    """every step of rts_set_scene works on a scene object of its own, swapped in at the end: a call that is refused -- by the
    flattening (a vertex index out of range; a mesh without normals on a handle that interpolates them) or after a whole device
    build into the new object (the injected builder failure with the fall-back switched off) -- leaves the handle tracing the
    scene it had: scene_info() equal field for field, the same pulse bit for bit"""
    from rts_amd import _lib
    spec = scenes.config_multi(W=8)
    n = spec["W"] ** 3
    tr = rts.Tracer(spec["W"], spec["max_refl"], 0, spec["smooth"], keep_all=True, device_build=True)
    tr.set_scene(spec["meshes"]); tr.set_receivers(spec["rx"])
    H.gpu_trace(rts, spec, tr=tr)
    info, rays = tr.scene_info(), tr.all_rays(n)
    assert spec["smooth"] and info["n_targets"] == 3 and info["n_nodes"] > 0

    bad_index = dict(spec["meshes"][1]); t = bad_index["tris"].copy(); t[-1, 2] = bad_index["verts"].shape[0]; bad_index["tris"] = t
    no_normals = dict(spec["meshes"][0]); no_normals["normals"] = np.zeros((0, 3))
    refusals = [("vertex index", [spec["meshes"][0], bad_index], {}, _lib.RTS_ERR_INVALID, "references vertex"),
                ("no normals", [no_normals, spec["meshes"][2]], {}, _lib.RTS_ERR_INVALID, "has no normals but interpolate_smooth is set"),
                ("device build", [spec["meshes"][2], ONE], {"RTS_DEBUG_FAIL_DEVICE_BUILD": "1", "RTS_DEVICE_BUILD_FALLBACK": "0"}, _lib.RTS_ERR_HIP, "injected")]
    for what, meshes, env, code, text in refusals:
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        with pytest.raises(_lib.RtsError) as e:
            tr.set_scene(meshes)
        for k in env:
            monkeypatch.delenv(k)
        assert e.value.code == code and text in str(e.value), what
        assert tr.scene_info() == info, what
        H.gpu_trace(rts, spec, tr=tr)
        assert_same_rays(rays, tr.all_rays(n), "after the refusal: " + what)
    tr.close()


def test_host_built_trees_through_the_device(rts, scenes):
    """a host-built scene (rts_sah.cpp, one tree per mesh) read back with rts_get_bvh is the per-mesh trees of
    rts_build_hierarchy_host concatenated: node children moved by the nodes in front, leaf children (~slot) by the slots in
    front, unused children left alone, leaf primitives by the mesh's first primitive, roots by the nodes, -1 for the mesh without
    triangles.  The device keeps the nodes' leaf children as ~primitive and parks the slot form in pad[] (k_children_to_prims):
    rts_get_bvh undoes that -- leaf children come back as ~slot, pad as 0.  All three meshes of config_multi (sphere, per-face
    box, plate), a single triangle and an empty mesh."""
    spec = scenes.config_multi(W=4)
    spec["meshes"] = spec["meshes"] + [ONE, EMPTY]; spec["motion"] = spec["motion"] + [STILL, STILL]
    tr = rts.Tracer(spec["W"], spec["max_refl"], 0, spec["smooth"], device_build=False)
    tr.set_scene(spec["meshes"]); tr.set_receivers(spec["rx"])
    H.gpu_trace(rts, spec, tr=tr)
    info = tr.scene_info()
    nodes, leaf_prim, roots = tr.bvh()
    assert info["builder"] == 0
    want_nodes, want_leaf, want_roots = [], [], []
    node_base = leaf_base = tri_base = 0
    for m in spec["meshes"]:
        mn, ml, root = rts.build_hierarchy_host(m["verts"], m["tris"])
        w = mn.view(np.uint32).copy()
        c = w[:, 24:28].view(np.int32).astype(np.int64)
        c = np.where(c == 0x7fffffff, c, np.where(c >= 0, c + node_base, ~(~c + leaf_base)))
        w[:, 24:28] = c.astype(np.int32).view(np.uint32)
        assert not w[:, 28:32].any()
        want_nodes.append(w); want_leaf.append(ml.astype(np.int64) + tri_base)
        want_roots.append(root + node_base if root >= 0 else root)
        node_base += len(mn); leaf_base += len(ml); tri_base += m["tris"].shape[0]
    want_nodes = np.concatenate(want_nodes); want_leaf = np.concatenate(want_leaf)
    assert want_roots[-1] == -1 and want_roots[-2] >= 0 and len(want_nodes) > len(spec["meshes"])
    assert info["n_nodes"] == len(want_nodes) and info["n_leaves"] == len(want_leaf) and info["n_prims"] == tri_base
    assert np.array_equal(nodes.view(np.uint32), want_nodes)                   # the node bytes: boxes, children as ~slot, pad 0
    assert np.array_equal(leaf_prim.astype(np.int64), want_leaf)
    assert roots.tolist() == want_roots
    tr.close()


@pytest.mark.parametrize("device_build", [False, True])
def test_replacing_a_scene_on_a_handle(rts, scenes, device_build):
    """set_scene(A), trace, set_scene(B), trace: the second pulse is a fresh handle's on B bit for bit -- nothing of A (leaf
    records, placement, primitive order, octant versions, the per-handle buffers sized by A) survives the swap"""
    a = scenes.config_multi(W=8)
    b = scenes.config_multi(W=8)
    b["meshes"] = [a["meshes"][1], ONE, a["meshes"][0], a["meshes"][2]]; b["motion"] = [a["motion"][1], STILL, a["motion"][0], a["motion"][2]]
    n = a["W"] ** 3

    def handle(spec):
        tr = rts.Tracer(spec["W"], spec["max_refl"], 0, spec["smooth"], keep_all=True, device_build=device_build)
        tr.set_scene(spec["meshes"]); tr.set_receivers(spec["rx"])
        return tr
    fresh = handle(b)
    _, st_fresh = H.gpu_trace(rts, b, tr=fresh)
    tr = handle(a)
    _, st_a = H.gpu_trace(rts, a, tr=tr)
    assert st_a["shaded"] > 0
    tr.set_scene(b["meshes"])
    _, st_b = H.gpu_trace(rts, b, tr=tr)
    assert_same_rays(fresh.all_rays(n), tr.all_rays(n), "the replaced scene")
    assert (st_b["segments"], st_b["shaded"], st_b["received"]) == (st_fresh["segments"], st_fresh["shaded"], st_fresh["received"])
    ia, ib = fresh.scene_info(), tr.scene_info()
    assert {k: v for k, v in ia.items() if k != "build_ms"} == {k: v for k, v in ib.items() if k != "build_ms"}
    fresh.close(); tr.close()
