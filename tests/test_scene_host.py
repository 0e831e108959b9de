"""The host arithmetic of rts_set_scene (rts_amd/csrc/rts_scene_host.h) without a GPU and without HIP: the flattening of the
caller's meshes into the scene's global arrays with its index checks, the concatenation of the host builder's per-mesh trees, and
a mesh's f64 bounds.  tests/scene_host/scene_host_main.cpp includes the header alone and is built with g++ (under
AddressSanitizer + UndefinedBehaviorSanitizer where g++ has them); every array it hands over is a heap block of exactly its
size.  Every expectation is written out or restated here in Python."""
import math

import numpy as np
import pytest

import helpers as H

INVALID, UNSUPPORTED = 1, 4          # RTS_ERR_INVALID, RTS_ERR_UNSUPPORTED (include/rts_amd.h)
UNUSED = 0x7fffffff


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    run = H.host_driver(tmp_path_factory, "scene_host/scene_host_main.cpp")

    def ask(lines):
        """one answer per case: key -> list of the token lists of its lines"""
        out = run("".join(line + "\n" for line in lines))
        answers = []
        for block in out.split("end\n")[:-1]:
            d = {}
            for ln in block.split("\n")[:-1]:
                key, _, rest = ln.partition(" ")
                d.setdefault(key, []).append(rest if key == "err" else rest.split())
            answers.append(d)
        assert len(answers) == len(lines)
        return answers
    return ask


def mesh(tris, verts, normals, refl=0.9, refr=1.0, counts=None, null=()):
    """a mesh of the driver's input; counts: (n_triangles, n_vertices, n_normals) other than the arrays' own; null: arrays handed over as null pointers"""
    t = np.asarray(tris, np.int64).reshape(-1, 3); v = np.asarray(verts, np.float64).reshape(-1, 3); n = np.asarray(normals, np.float64).reshape(-1, 3)
    return dict(t=t, v=v, n=n, refl=refl, refr=refr, counts=counts or (len(t), len(v), len(n)), null=null)


def case(cmd, meshes, smooth=False, n_targets=None, null_meshes=False):
    tok = [cmd, "1" if smooth else "0", str(len(meshes) if n_targets is None else n_targets), "-1" if null_meshes else str(len(meshes))]
    for m in ([] if null_meshes else meshes):
        tok += [str(c) for c in m["counts"]] + [repr(m["refl"]), repr(m["refr"])]
        for key, a in (("t", m["t"]), ("v", m["v"]), ("n", m["n"])):
            tok += ["-1"] if key in m["null"] else [str(a.size)] + [str(int(x)) if key == "t" else repr(float(x)) for x in a.ravel()]
    return " ".join(tok)


def restated_flat(meshes):
    """the scene's arrays as rts_set_scene defines them: targets concatenated in order, indices rebased; a normal index is the
    vertex index, the triangle index for per-face normals (more normals than vertices), normal_base without normals"""
    out = dict(mesh=[], vidx=[], nidx=[], ptarg=[], vtarg=[], ntarg=[], verts=[], normals=[])
    nt = nv = nn = 0
    for ti, m in enumerate(meshes):
        t, v, n = m["t"], m["v"], m["n"]
        perface = len(n) > len(v)
        out["mesh"].append((len(t), len(v), len(n), nt, nv, nn, m["refl"], m["refr"], int(perface)))
        for i, tri in enumerate(t):
            for vi in tri:
                out["vidx"].append(nv + int(vi))
                out["nidx"].append(nn + (0 if len(n) == 0 else (i if perface else int(vi))))
            out["ptarg"].append(ti)
        out["vtarg"] += [ti] * len(v); out["ntarg"] += [ti] * len(n)
        out["verts"] += v.ravel().tolist(); out["normals"] += n.ravel().tolist()
        nt += len(t); nv += len(v); nn += len(n)
    out["totals"] = [nt, nv, nn]
    return out


def ints(ans, key):
    return [int(x) for x in ans[key][0]]


def floats(ans, key, i=0):
    return [float.fromhex(x) for x in ans[key][i]]


def check_flat(ans, meshes):
    want = restated_flat(meshes)
    assert ints(ans, "rc") == [0] and ans["err"] == [""]
    got_meshes = [tuple([int(x) for x in m[:6]] + [float.fromhex(m[6]), float.fromhex(m[7]), int(m[8])]) for m in ans.get("mesh", [])]
    assert got_meshes == want["mesh"]
    for key in ("vidx", "nidx", "ptarg", "vtarg", "ntarg", "totals"):
        assert ints(ans, key) == want[key], key
    for key in ("verts", "normals"):
        assert np.array_equal(np.array(floats(ans, key)).view(np.uint64), np.array(want[key], np.float64).view(np.uint64)), key


RNG = np.random.default_rng(11)
TRI_V = [[0, 0, 0], [1, 0, 0], [0, 1, 0]]


def some_mesh(n_v, n_t, normals, refl=0.7, refr=1.3):
    """normals: "vertex" (one per vertex), "face" (one per triangle, more than vertices), "none" """
    v = RNG.normal(size=(n_v, 3)); t = RNG.integers(0, n_v, size=(n_t, 3))
    n_n = {"vertex": n_v, "face": n_t, "none": 0}[normals]
    assert normals != "face" or n_t > n_v
    return mesh(t, v, RNG.normal(size=(n_n, 3)), refl, refr)


def test_flatten_accepted(driver):
    empty = mesh([], [], [])
    scenes = [[],                                                            # no targets
              [mesh([], TRI_V, [[0, 0, 1]] * 3)],                            # one mesh without triangles
              [mesh([[0, 1, 2]], TRI_V, [[0, 0, 1]] * 3)],                   # a single triangle
              [some_mesh(5, 4, "vertex"), empty, some_mesh(4, 7, "face")],   # the middle one empty: the bases behind it do not move
              [some_mesh(6, 9, "vertex")],                                   # n_normals == n_vertices: indexed by vertex
              [some_mesh(3, 5, "face", 0.5), some_mesh(4, 6, "face", 0.6)],  # n_normals > n_vertices: indexed by triangle
              [some_mesh(5, 3, "vertex"), some_mesh(4, 6, "none"), some_mesh(3, 2, "vertex")]]      # no normals, smoothing off: normal_base
    answers = driver([case("flatten", s) for s in scenes])
    for s, a in zip(scenes, answers):
        check_flat(a, s)
    # written out: the single triangle, and where the mesh without normals points its triangles
    assert ints(answers[2], "vidx") == [0, 1, 2] and ints(answers[2], "nidx") == [0, 1, 2] and ints(answers[2], "totals") == [1, 3, 3]
    assert ints(answers[3], "ptarg") == [0] * 4 + [2] * 7 and ints(answers[3], "nidx")[12:] == [5 + i for i in range(7) for _ in range(3)]
    assert set(ints(answers[6], "nidx")[9:27]) == {5} and min(ints(answers[6], "nidx")[27:]) >= 5
    # a mesh without normals is fine on a smoothing handle as long as it has no triangles
    check_flat(driver([case("flatten", [mesh([], TRI_V, [])], smooth=True)])[0], [mesh([], TRI_V, [])])


def test_flatten_refused(driver):
    ok = mesh([[0, 1, 2]], TRI_V, [[0, 0, 1]] * 3)
    tri = [[0, 1, 2], [2, 1, 0], [1, 2, 0], [0, 2, 1], [1, 0, 2]]
    cases = [
        (case("flatten", [], n_targets=2, null_meshes=True), INVALID, "rts_set_scene: null meshes"),
        (case("flatten", [ok, mesh([[0, 1, 2]], TRI_V, [[0, 0, 1]] * 3, null=("t",))]), INVALID, "rts_set_scene: target 1 has null arrays"),
        (case("flatten", [mesh([[0, 1, 2]], TRI_V, [[0, 0, 1]] * 3, null=("v",))]), INVALID, "rts_set_scene: target 0 has null arrays"),
        (case("flatten", [ok, ok, mesh([[0, 1, 2]], TRI_V, [[0, 0, 1]] * 3, null=("n",))]), INVALID, "rts_set_scene: target 2 has null arrays"),
        (case("flatten", [mesh([], [], [])] * 255), UNSUPPORTED, "rts_set_scene: more than 254 targets"),
        (case("flatten", [ok, mesh([[0, 1, 2], [0, 3, 1]], TRI_V, [[0, 0, 1]] * 3)]), INVALID, "rts_set_scene: target 1 triangle 1 references vertex 3 >= 3"),
        (case("flatten", [mesh([[0, 0xffffffff, 1]], TRI_V, [[0, 0, 1]] * 3)]), INVALID, "rts_set_scene: target 0 triangle 0 references vertex 4294967295 >= 3"),
        (case("flatten", [mesh(tri, TRI_V, [[0, 0, 1]] * 4)]), INVALID, "rts_set_scene: target 0 normal index 4 >= 4"),       # per-face (4 > 3 vertices), five triangles
        (case("flatten", [ok, mesh([[0, 1, 2]], TRI_V, [])], smooth=True), INVALID, "rts_set_scene: target 1 has no normals but interpolate_smooth is set"),
        # totals above 0x7ffffff0 as COUNTS ONLY, three-element blocks behind the pointers: refused before anything is read
        (case("flatten", [mesh([[0, 1, 2]], [[0, 0, 0]], [[0, 0, 1]], counts=(0x7ffffff1, 1, 1))]), UNSUPPORTED, "rts_set_scene: scene too large"),
        (case("flatten", [mesh([[0, 1, 2]], [[0, 0, 0]], [[0, 0, 1]], counts=(1, 0x7ffffff1, 1))]), UNSUPPORTED, "rts_set_scene: scene too large"),
        (case("flatten", [mesh([[0, 1, 2]], [[0, 0, 0]], [[0, 0, 1]], counts=(1, 1, 0xffffffff))]), UNSUPPORTED, "rts_set_scene: scene too large"),
        (case("flatten", [mesh([[0, 0, 0]], [[0, 0, 0]], [[0, 0, 1]], counts=(0x40000000, 1, 1))] * 2), UNSUPPORTED, "rts_set_scene: scene too large"),     # the SUM of two meshes
    ]
    answers = driver([c for c, _, _ in cases])
    for (_, code, text), a in zip(cases, answers):
        assert ints(a, "rc") == [code] and a["err"] == [text]
        assert "vidx" not in a
    # 254 targets are accepted, and the checks come in this order: null arrays in front of the limits, the limits in front of the indices
    assert ints(driver([case("flatten", [mesh([], [], [])] * 254)])[0], "rc") == [0]
    both = driver([case("flatten", [mesh([[0, 1, 9]], TRI_V, [], counts=(0x7ffffff1, 3, 0), null=("v",))]),
                   case("flatten", [mesh([[0, 1, 9]], TRI_V, []), mesh([[0, 0, 0]], [[0, 0, 0]], [], counts=(0x7ffffff1, 1, 0))], smooth=True)])
    assert both[0]["err"] == ["rts_set_scene: target 0 has null arrays"] and both[1]["err"] == ["rts_set_scene: scene too large"]


def words(tokens):
    w = np.array([int(x) for x in tokens], np.uint32)
    return w, w[24:28].view(np.int32)


@pytest.mark.parametrize("k", [2, 3])
def test_concatenation(driver, k):
    a = driver(["concat %d" % k])[0]
    in_trees = [(int(r), int(tb)) for r, tb in a["in_tree"]]
    assert len(in_trees) == k and [tb for _, tb in in_trees] == ([0, 5] if k == 2 else [0, 5, 5])
    in_nodes = [words(t) for t in a.get("in_node", [])]; in_leaf = [[int(x) for x in t] for t in a["in_leaf"]]
    sizes = [int(r[1]) for r in a["root"]]; n_slots = [len(x) for x in in_leaf]
    assert sizes == ([3, 1] if k == 2 else [3, 0, 1]) and n_slots == ([7, 1] if k == 2 else [7, 0, 1])
    # the hand-written trees hold what the shifts distinguish: an unused slot, the leaf child ~0, a mesh with no nodes and no root
    kids = np.concatenate([c for _, c in in_nodes])
    assert (kids == UNUSED).any() and (kids == ~0).any() and (kids > 0).any() and (k == 2 or (-1, 5) in in_trees)
    want_nodes, want_leaf, want_roots = [], [], []
    node_base = leaf_base = 0; at = 0
    for (root, tri_base), n_nodes, leaf in zip(in_trees, sizes, in_leaf):
        for w, c in in_nodes[at:at + n_nodes]:
            w = w.copy(); c = c.astype(np.int64)
            c = np.where(c == UNUSED, c, np.where(c >= 0, c + node_base, ~(~c + leaf_base)))
            w[24:28] = c.astype(np.int32).view(np.uint32)
            want_nodes.append(w)
        want_leaf += [p + tri_base for p in leaf]
        want_roots.append(root + node_base if root >= 0 else root)
        at += n_nodes; node_base += n_nodes; leaf_base += len(leaf)
    got_nodes = [words(t)[0] for t in a["node"]]
    assert len(got_nodes) == len(want_nodes) == 4 and all(np.array_equal(g, w) for g, w in zip(got_nodes, want_nodes))      # boxes and pad unchanged
    assert ints(a, "leaf") == want_leaf and [int(r[0]) for r in a["root"]] == want_roots
    # written out
    got_kids = [words(t)[1].tolist() for t in a["node"]]
    assert got_kids == [[1, ~0, 2, UNUSED], [~1, ~2, UNUSED, UNUSED], [~3, ~4, ~5, ~6], [~7, UNUSED, UNUSED, UNUSED]]
    assert ints(a, "leaf") == [0, 1, 2, 1, 3, 4, 0, 5] and want_roots == ([0, 3] if k == 2 else [0, -1, 3])


def restated_bounds(m):
    tv = m["v"][m["t"]] if len(m["t"]) else np.zeros((0, 3, 3))
    with np.errstate(invalid="ignore"):
        tv = tv[(np.abs(tv) < 3.0e38).all(axis=(1, 2))]                            # finite, and inside the range of a padded f32 box (rts_coord_valid)
    if len(tv) == 0:
        return [0.0] * 7
    lo = tv.min(axis=(0, 1)); hi = tv.max(axis=(0, 1))
    return lo.tolist() + hi.tolist() + [float(max(np.abs(lo).max(), np.abs(hi).max()))]


def test_bounds(driver):
    quad = [[0, 1, 2], [1, 2, 3], [2, 3, 4]]
    v = np.array([[1.0, 2, 3], [-4, 5, 6], [7, -8, 9], [0.5, 0.25, -10], [100, 200, 300]])
    one_bad = v.copy(); one_bad[4, 1] = math.nan                               # the last triangle is left out, and with it vertex 4's 100 / 300
    all_bad = v.copy(); all_bad[2, 0] = math.inf                               # vertex 2 is in every triangle
    neg = -np.abs(RNG.normal(size=(6, 3))) - 1.0
    too_big = v.copy(); too_big[4, 2] = -3.5e38                                # finite in f64, beyond a padded f32 box: left out like the NaN
    meshes = [mesh(quad, one_bad, []), mesh(quad, all_bad, []), mesh([], [], []), mesh(RNG.integers(0, 6, size=(8, 3)), neg, []),
              mesh(quad, v, []), mesh(quad, too_big, [])]
    a = driver([case("bounds", meshes)])[0]
    check_flat(a, meshes)
    got = [floats(a, "bounds", i) for i in range(len(meshes))]
    for m, g in zip(meshes, got):
        assert np.array_equal(np.array(g).view(np.uint64), np.array(restated_bounds(m)).view(np.uint64))
    assert got[0] == [-4.0, -8.0, -10.0, 7.0, 5.0, 9.0, 10.0]
    assert got[1] == [0.0] * 7 and got[2] == [0.0] * 7
    assert got[3][6] == -min(got[3][:3]) and max(got[3][3:6]) < 0                 # negative-only coordinates: max_abs comes from lo
    assert got[4] == [-4.0, -8.0, -10.0, 100.0, 200.0, 300.0, 300.0] and got[5] == got[0]
