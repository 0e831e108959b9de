"""The hierarchy checker of tests/bvh_check.py proved without a GPU: every edge mesh of tests/test_gpu_builders.py built by the
host builder (rts_build_hierarchy_host, split budgets 0 and 2) passes it -- so the meshes satisfy every invariant under a correct
builder -- and a correct tree with ONE thing wrong (a box off by one f32 ulp, a lost, shared, dangling or cyclic link, a foreign
primitive, a lost root) is rejected with the violated invariant in the message."""
import re

import numpy as np
import pytest

import bvh_check as B


@pytest.mark.parametrize("budget", [0, 2])
@pytest.mark.parametrize("name", list(B.CASES))
def test_host_built_trees_pass(rts, name, budget):
    meshes = B.case_meshes(name)
    nodes, leaf, roots = B.host_scene(rts, meshes, budget)
    fig = B.check_hierarchy(nodes, leaf, roots, meshes, max_refs=1 if budget == 0 else None, all_reachable=True)
    _, prim_mesh, valid = B.triangle_table(meshes)
    print(name, "budget", budget, fig)
    for t, f in enumerate(fig):
        nv = int(valid[prim_mesh == t].sum())
        if budget == 0:
            assert f["slots"] == nv                                  # one reference per triangle
        assert (f["nodes"] == 0) == (nv == 0) and (f["depth"] == 0) == (nv == 0) and f["slots"] >= nv
    if name == "degen32" and len(leaf):
        assert (np.bincount(leaf, minlength=32)[list(B.DEGENERATE_PRIMS)] == 1).all()      # the point and the collinear triangle keep one reference


# ------------------------------------------------------------------------------------------------ mutations
@pytest.fixture(scope="module")
def good(rts):
    """a correct host tree over the 257-triangle soup and a second mesh (the soup of 5): arrays, meshes, the walk's bookkeeping"""
    meshes = [B.mesh_of(B.soup(257, 257)), B.mesh_of(B.soup(5, 902))]
    nodes, leaf, roots = B.host_scene(rts, meshes, 2)
    B.check_hierarchy(nodes, leaf, roots, meshes, all_reachable=True)
    child, lo, hi = B.unpack(nodes)
    level = np.full(len(nodes), -1); parent = np.full((len(nodes), 2), -1)       # plain walk of mesh 0, for picking victims
    level[roots[0]] = 0; todo = [int(roots[0])]
    while todo:
        i = todo.pop()
        for k in range(4):
            c = child[i, k]
            if c != B.UNUSED and c >= 0:
                level[c] = level[i] + 1; parent[c] = (i, k); todo.append(int(c))
    return dict(nodes=nodes, leaf=leaf, roots=roots, meshes=meshes, child=child, level=level, parent=parent)


# word offsets in a 32-word record
def LO(axis, k): return 4 * axis + k
def HI(axis, k): return 12 + 4 * axis + k
def CHILD(k): return 24 + k


def set_child(nodes, i, k, link):
    nodes.view(np.int32)[i, CHILD(k)] = link


def mutate(good, what):
    nodes, leaf, roots = good["nodes"].copy(), good["leaf"].copy(), good["roots"].copy()
    child, level, parent, meshes = good["child"], good["level"], good["parent"], good["meshes"]
    tv, _, _ = B.triangle_table(meshes)
    refs = np.bincount(leaf, minlength=len(tv))
    inner = [(i, k) for i in np.nonzero(level >= 0)[0] for k in range(4) if child[i, k] != B.UNUSED and child[i, k] >= 0]
    leaves = [(i, k) for i in np.nonzero(level >= 0)[0] for k in range(4) if child[i, k] < 0]
    if what == "leaf lo one ulp past a vertex":
        i, k = next((i, k) for i, k in leaves if refs[leaf[~child[i, k]]] == 1)
        v = tv[leaf[~child[i, k]]][:, 0].min()
        f = np.float32(v)
        if float(f) <= v:
            f = np.nextafter(f, np.float32(np.inf))
        assert float(np.nextafter(f, np.float32(-np.inf))) <= v < float(f)       # the first f32 above the vertex
        nodes[i, LO(0, k)] = f
    elif what == "inner box one ulp inside its child":
        i, k = next((i, k) for i, k in inner if level[i] >= 1)
        c = child[i, k]; used = child[c] != B.UNUSED
        m = nodes[c, LO(1, 0):LO(1, 0) + 4][used].min()                           # the lowest y of the record's own child boxes
        nodes[i, LO(1, k)] = np.nextafter(m, np.float32(np.inf))                  # its slot box now starts one ulp above it
    elif what == "leaf link lost":
        i, k = leaves[len(leaves) // 2]
        set_child(nodes, i, k, B.UNUSED)
    elif what == "shared node":
        a = next(x for x in inner if level[x[0]] == 2)
        b = next(x for x in inner if level[x[0]] == 2 and x[0] != a[0])
        set_child(nodes, a[0], a[1], child[b[0], b[1]])
    elif what == "shared leaf":
        a = leaves[3]; b = next(x for x in leaves if x[0] != a[0])
        set_child(nodes, a[0], a[1], child[b[0], b[1]])
    elif what == "link past the records":
        i, k = inner[len(inner) // 2]
        set_child(nodes, i, k, len(nodes))
    elif what == "foreign primitive":
        leaf[7] = len(meshes[0]["tris"]) + 2
    elif what == "root lost":
        roots[0] = -1
    elif what == "cycle":
        i, k = next(x for x in inner if level[x[0]] >= 3)
        set_child(nodes, i, k, parent[parent[i, 0], 0])                           # back to its grandparent
    else:
        raise KeyError(what)
    return nodes, leaf, roots


MUTATIONS = [("leaf lo one ulp past a vertex", r"^point coverage: .*primitive \d+"),
             ("inner box one ulp inside its child", r"^nesting: "),
             ("leaf link lost", r"^unused slot: "),
             ("shared node", r"^node reached twice: "),
             ("shared leaf", r"^leaf slot reached twice: "),
             ("link past the records", r"^link: child link 1?\d+ "),
             ("foreign primitive", r"^leaf_prim: leaf slot 7 names primitive 259, which belongs to mesh 1: mesh 0"),
             ("root lost", r"^roots: .*: mesh 0"),
             ("cycle", r"^node reached twice: ")]


@pytest.mark.parametrize("what,message", MUTATIONS, ids=[m[0].replace(" ", "-") for m in MUTATIONS])
def test_mutation_is_rejected(good, what, message):
    nodes, leaf, roots = mutate(good, what)
    changed = (nodes.view(np.uint32) != good["nodes"].view(np.uint32)).sum() + (leaf != good["leaf"]).sum() + (roots != good["roots"]).sum()
    assert changed == 1                                                           # one word of one array
    with pytest.raises(AssertionError) as e:
        B.check_hierarchy(nodes, leaf, roots, good["meshes"], all_reachable=True)          # (the cycle: returns -- the walk stops at the first record seen twice)
    text = str(e.value)
    assert re.search(message, text), text
    assert re.search(r"mesh \d+", text)


def test_figures_and_unreachable_records(good):
    """what check_hierarchy returns, and its two reachability rules: an appended record no root leads to fails all_reachable=True
    and the count rule of all_reachable=False alike (a host tree has fewer records than one per binary node)"""
    fig = B.check_hierarchy(good["nodes"], good["leaf"], good["roots"], good["meshes"], all_reachable=True)
    assert [f["slots"] for f in fig] == [int((np.asarray(good["leaf"]) < 257).sum()), int((np.asarray(good["leaf"]) >= 257).sum())]
    assert sum(f["nodes"] for f in fig) == len(good["nodes"]) and fig[0]["depth"] == good["level"].max() + 1 and fig[0]["max_refs"] > 1
    more = np.concatenate([good["nodes"], good["nodes"][-1:]])
    with pytest.raises(AssertionError, match="^reachability: record %d " % len(good["nodes"])):
        B.check_hierarchy(more, good["leaf"], good["roots"], good["meshes"], all_reachable=True)
    with pytest.raises(AssertionError, match="^reachability: %d records" % len(good["nodes"])):
        B.check_hierarchy(good["nodes"], good["leaf"], good["roots"], good["meshes"], all_reachable=False)
    with pytest.raises(AssertionError, match="^reference count: primitive"):
        B.check_hierarchy(good["nodes"], good["leaf"], good["roots"], good["meshes"], max_refs=1, all_reachable=True)
