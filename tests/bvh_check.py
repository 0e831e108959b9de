"""Structural checker of the static target-space hierarchy (BVH4 records as Tracer.bvh() returns them) and the edge-size meshes
the builders are held to.  Plain numpy, no GPU, no library call: tests/test_bvh_check_host.py proves the checker itself on
host-built trees and on mutated copies, tests/test_gpu_builders.py runs every device builder through it.

What the walk relies on: for any point of any valid triangle there is a chain of boxes from the target's root down to a leaf
slot of that triangle, and every box of the chain contains the point.  check_hierarchy() establishes it from two halves: NESTING
(every used child box of a reached record lies inside the slot box through which the record was reached) and POINT COVERAGE
(every point of the k = 4 barycentric lattice of every valid triangle lies inside the leaf box of one of its slots).  Every
comparison is exact: f32 boxes widened to f64, closed inequalities, no tolerance.
"""
import numpy as np

UNUSED = 0x7fffffff
COORD_LIMIT = 3.0e38            # a triangle is valid when every coordinate is finite and below this in magnitude (load_tri, rts_coord_valid)

# the 15 points of the k = 4 barycentric lattice, weights [15][3]
LATTICE = np.array([(i, j, 4 - i - j) for i in range(5) for j in range(5 - i)], np.float64) / 4.0


def unpack(nodes):
    """[n][32] f32 records -> child links int32 [n][4], lo / hi f64 [n][4][3] (record, slot, axis)"""
    nodes = np.ascontiguousarray(nodes, np.float32).reshape(-1, 32)
    child = nodes[:, 24:28].copy().view(np.int32)
    lo = np.stack([nodes[:, 0:4], nodes[:, 4:8], nodes[:, 8:12]], axis=2).astype(np.float64)
    hi = np.stack([nodes[:, 12:16], nodes[:, 16:20], nodes[:, 20:24]], axis=2).astype(np.float64)
    return child, lo, hi


def triangle_table(meshes):
    """the scene's triangles by global primitive id: vertices f64 [nprim][3][3], mesh of each primitive, validity"""
    tv = [np.asarray(m["verts"], np.float64).reshape(-1, 3)[np.asarray(m["tris"], np.int64).reshape(-1, 3)] for m in meshes]
    tv = np.concatenate(tv) if tv else np.zeros((0, 3, 3))
    pm = [np.full(np.asarray(m["tris"]).reshape(-1, 3).shape[0], i, np.int64) for i, m in enumerate(meshes)]
    pm = np.concatenate(pm) if pm else np.zeros(0, np.int64)
    with np.errstate(invalid="ignore"):
        valid = (np.abs(tv) < COORD_LIMIT).all(axis=(1, 2))          # (NaN compares false)
    return tv, pm, valid


def _fail(what, mesh, node=None, slot=None, more=""):
    where = "mesh %d" % mesh + ("" if node is None else ", node %d" % node) + ("" if slot is None else ", slot %d" % slot)
    raise AssertionError("%s: %s%s" % (what, where, (" -- " + more) if more else ""))


def check_hierarchy(nodes, leaf_prim, roots, meshes, *, max_refs=None, all_reachable):
    """Raises AssertionError("<invariant>: mesh m, node i, slot k ...") at the first violated invariant, the tree's shape before its
    boxes; returns per mesh dict(nodes, slots, max_refs, depth): reachable records, leaf slots, the largest number of slots of one
    primitive, and the number of record levels below (and including) the root.
    `slot` in a message is the child slot 0..3 of record `node`, or a leaf slot of leaf_prim where the message says "leaf slot"."""
    child, lo, hi = unpack(nodes)
    leaf_prim = np.asarray(leaf_prim).astype(np.int64).reshape(-1)
    roots = np.asarray(roots).astype(np.int64).reshape(-1)
    n_nodes, n_slots, n_mesh = child.shape[0], leaf_prim.shape[0], len(meshes)
    tv, prim_mesh, valid = triangle_table(meshes)
    nprim = tv.shape[0]

    # ---- roots
    assert roots.shape[0] == n_mesh, "roots: %d roots for %d meshes" % (roots.shape[0], n_mesh)
    has_valid = np.bincount(prim_mesh[valid], minlength=n_mesh) > 0 if n_mesh else np.zeros(0, bool)
    for t in range(n_mesh):
        if has_valid[t] and not (0 <= roots[t] < n_nodes):
            _fail("roots: a mesh with a valid triangle has root %d outside the %d records" % (roots[t], n_nodes), t)
        if not has_valid[t] and roots[t] != -1:
            _fail("roots: a mesh without a valid triangle has root %d, not -1" % roots[t], t)

    # ---- tree shape: breadth first over all meshes at once, frontier arrays (one numpy pass per level)
    node_mesh = np.full(n_nodes, -1, np.int64)              # the mesh whose root led to the record
    node_from = np.full((n_nodes, 2), -1, np.int64)         # (record, child slot) through which it was reached; root: -1
    slot_mesh = np.full(n_slots, -1, np.int64)
    slot_from = np.full((n_slots, 2), -1, np.int64)
    depth = np.zeros(n_mesh, np.int64)
    f_node = roots[roots >= 0]; f_mesh = np.nonzero(roots >= 0)[0]; f_from = np.full((len(f_node), 2), -1, np.int64)
    while len(f_node):
        # no record twice: not from this level's links, not from an earlier level's (which also ends every cycle here)
        order = np.argsort(f_node, kind="stable"); s = f_node[order]
        dup = np.nonzero(s[1:] == s[:-1])[0]
        if len(dup):
            a, b = order[dup[0]], order[dup[0] + 1]
            _fail("node reached twice: record %d is a child of (node %d, slot %d) and of (node %d, slot %d) of mesh %d"
                  % (f_node[a], f_from[a, 0], f_from[a, 1], f_from[b, 0], f_from[b, 1], f_mesh[b]), f_mesh[a], f_node[a])
        seen = np.nonzero(node_mesh[f_node] >= 0)[0]
        if len(seen):
            a = seen[0]
            _fail("node reached twice: record %d, reached before for mesh %d, is again a child of (node %d, slot %d)"
                  % (f_node[a], node_mesh[f_node[a]], f_from[a, 0], f_from[a, 1]), f_mesh[a], f_node[a])
        node_mesh[f_node] = f_mesh; node_from[f_node] = f_from
        depth[np.unique(f_mesh)] += 1
        c = child[f_node].astype(np.int64)                                        # [m][4]
        used = c != UNUSED
        # unused slots: the point lo == hi > 1e38 on all three axes
        bad = ~used & ~((lo[f_node] == hi[f_node]) & (lo[f_node] > 1e38)).all(axis=2)
        if bad.any():
            a, k = np.argwhere(bad)[0]
            _fail("unused slot: its box is not the point lo == hi > 1e38", f_mesh[a], f_node[a], k, "lo %r hi %r" % (lo[f_node[a], k], hi[f_node[a], k]))
        empty = np.nonzero(~used.any(axis=1))[0]
        if len(empty):
            _fail("empty record: a reached record has no used child", f_mesh[empty[0]], f_node[empty[0]])
        is_leaf = used & (c < 0); is_node = used & (c >= 0)
        bad = (is_node & (c >= n_nodes)) | (is_leaf & (~c >= n_slots))
        if bad.any():
            a, k = np.argwhere(bad)[0]
            _fail("link: child link %d is neither 0x7fffffff, a record index below %d nor ~slot with slot below %d" % (c[a, k], n_nodes, n_slots),
                  f_mesh[a], f_node[a], k)
        # leaf links
        la, lk = np.nonzero(is_leaf)
        ls = ~c[la, lk]
        order = np.argsort(ls, kind="stable"); s = ls[order]
        dup = np.nonzero(s[1:] == s[:-1])[0]
        if len(dup):
            a, b = order[dup[0]], order[dup[0] + 1]
            _fail("leaf slot reached twice: leaf slot %d is a child of (node %d, slot %d) and of (node %d, slot %d)"
                  % (ls[a], f_node[la[a]], lk[a], f_node[la[b]], lk[b]), f_mesh[la[a]], f_node[la[a]], lk[a])
        seen = np.nonzero(slot_mesh[ls] >= 0)[0]
        if len(seen):
            a = seen[0]
            _fail("leaf slot reached twice: leaf slot %d, reached before from (node %d, slot %d) of mesh %d"
                  % (ls[a], slot_from[ls[a], 0], slot_from[ls[a], 1], slot_mesh[ls[a]]), f_mesh[la[a]], f_node[la[a]], lk[a])
        slot_mesh[ls] = f_mesh[la]; slot_from[ls, 0] = f_node[la]; slot_from[ls, 1] = lk
        p = leaf_prim[ls]
        bad = np.nonzero((p < 0) | (p >= nprim))[0]
        if len(bad):
            _fail("leaf_prim: leaf slot %d names primitive %d of %d" % (ls[bad[0]], p[bad[0]], nprim), f_mesh[la[bad[0]]], f_node[la[bad[0]]], lk[bad[0]])
        bad = np.nonzero(prim_mesh[p] != f_mesh[la])[0]
        if len(bad):
            a = bad[0]
            _fail("leaf_prim: leaf slot %d names primitive %d, which belongs to mesh %d" % (ls[a], p[a], prim_mesh[p[a]]), f_mesh[la[a]], f_node[la[a]], lk[a])
        # the next level
        na, nk = np.nonzero(is_node)
        f_from = np.stack([f_node[na], nk], axis=1) if len(na) else np.zeros((0, 2), np.int64)
        f_node, f_mesh = c[na, nk], f_mesh[na]

    missing = np.nonzero(slot_mesh < 0)[0]
    if len(missing):
        p = leaf_prim[missing[0]]
        _fail("leaf slot not reached: leaf slot %d (primitive %d) hangs under no root (%d of %d slots unreached)" % (missing[0], p, len(missing), n_slots),
              int(prim_mesh[p]) if 0 <= p < nprim else -1)
    # a mesh without a root owns nothing: implied -- every slot and every reached record hangs under a root >= 0

    # ---- reachability
    slots_of = np.bincount(slot_mesh, minlength=n_mesh) if n_mesh else np.zeros(0, np.int64)
    nodes_of = np.bincount(node_mesh[node_mesh >= 0], minlength=n_mesh) if n_mesh else np.zeros(0, np.int64)
    unreached = np.nonzero(node_mesh < 0)[0]
    if all_reachable:
        if len(unreached):
            raise AssertionError("reachability: record %d is reached from no root (%d of %d records unreached)" % (unreached[0], len(unreached), n_nodes))
    else:
        # one record per binary node, opened ones included: max(nv - 1, 1) per mesh of nv >= 1 leaf slots, none for a mesh without slots
        want = int(np.where(slots_of > 0, np.maximum(slots_of - 1, 1), 0).sum())
        if n_nodes != want:
            raise AssertionError("reachability: %d records, the meshes' leaf slots %r ask for sum max(nv - 1, 1) = %d" % (n_nodes, slots_of.tolist(), want))

    # ---- nesting: the used child boxes of a reached, non-root record inside the slot box it was reached through
    r = np.nonzero((node_mesh >= 0) & (node_from[:, 0] >= 0))[0]
    if len(r):
        plo = lo[node_from[r, 0], node_from[r, 1]][:, None, :]; phi = hi[node_from[r, 0], node_from[r, 1]][:, None, :]
        used = child[r] != UNUSED
        bad = used & ~((lo[r] >= plo) & (hi[r] <= phi)).all(axis=2)
        if bad.any():
            a, k = np.argwhere(bad)[0]
            _fail("nesting: child box lo %r hi %r sticks out of the box lo %r hi %r of (node %d, slot %d) it is reached through"
                  % (lo[r[a], k], hi[r[a], k], plo[a, 0], phi[a, 0], node_from[r[a], 0], node_from[r[a], 1]), node_mesh[r[a]], r[a], k)

    # ---- reference counts
    refs = np.bincount(leaf_prim, minlength=nprim)[:nprim] if nprim else np.zeros(0, np.int64)
    bad = np.nonzero(valid & (refs < 1))[0]
    if len(bad):
        _fail("reference count: valid primitive %d has no leaf slot" % bad[0], prim_mesh[bad[0]])
    bad = np.nonzero(~valid & (refs > 0))[0]
    if len(bad):
        _fail("reference count: invalid primitive %d has %d leaf slots" % (bad[0], refs[bad[0]]), prim_mesh[bad[0]])
    if max_refs is not None:
        bad = np.nonzero(refs > max_refs)[0]
        if len(bad):
            _fail("reference count: primitive %d has %d leaf slots, more than %d" % (bad[0], refs[bad[0]], max_refs), prim_mesh[bad[0]])

    # ---- point coverage (a primitive with ONE slot: that box holds all 15 points, its three vertices among them)
    if n_slots:
        sp = leaf_prim                                                            # primitive of every slot (all valid by now)
        pts = np.einsum("lk,pkc->plc", LATTICE, tv[sp])                           # [slot][15][3] f64
        blo = lo[slot_from[:, 0], slot_from[:, 1]][:, None, :]; bhi = hi[slot_from[:, 0], slot_from[:, 1]][:, None, :]
        inside = ((pts >= blo) & (pts <= bhi)).all(axis=2)                        # [slot][15]
        cover = np.zeros((nprim, LATTICE.shape[0]), np.int64)
        np.add.at(cover, sp, inside.astype(np.int64))
        bad = valid[:, None] & (cover == 0)
        if bad.any():
            p, l = np.argwhere(bad)[0]
            s0 = np.nonzero(sp == p)[0][0]
            _fail("point coverage: lattice point %d %r of primitive %d (%d slots) lies in none of its leaf boxes; first leaf box lo %r hi %r"
                  % (l, LATTICE[l] @ tv[p], p, refs[p], blo[s0, 0], bhi[s0, 0]), prim_mesh[p], slot_from[s0, 0], slot_from[s0, 1])

    out = []
    for t in range(n_mesh):
        mine = prim_mesh == t
        out.append(dict(nodes=int(nodes_of[t]), slots=int(slots_of[t]), max_refs=int(refs[mine].max()) if mine.any() else 0, depth=int(depth[t])))
    return out


def host_scene(api, meshes, split_budget):
    """adapter: the host builder's per-mesh trees (rts_build_hierarchy_host) concatenated the way a scene holds them -- the three
    arrays Tracer.bvh() returns (node children moved by the records in front, ~slot by the slots, primitives by the triangles)"""
    all_nodes, all_leaf, roots = [], [], []
    node_base = leaf_base = tri_base = 0
    for m in meshes:
        mn, ml, root = api.build_hierarchy_host(m["verts"], m["tris"], split_budget=float(split_budget))
        w = mn.view(np.uint32).copy()
        c = w[:, 24:28].view(np.int32).astype(np.int64)
        c = np.where(c == UNUSED, c, np.where(c >= 0, c + node_base, ~(~c + leaf_base)))
        w[:, 24:28] = c.astype(np.int32).view(np.uint32)
        all_nodes.append(w.view(np.float32)); all_leaf.append(ml.astype(np.int64) + tri_base)
        roots.append(root + node_base if root >= 0 else -1)
        node_base += len(mn); leaf_base += len(ml); tri_base += np.asarray(m["tris"]).reshape(-1, 3).shape[0]
    nodes = np.concatenate(all_nodes) if all_nodes else np.zeros((0, 32), np.float32)
    leaf = np.concatenate(all_leaf).astype(np.uint32) if all_leaf else np.zeros(0, np.uint32)
    return nodes.reshape(-1, 32), leaf, np.array(roots, np.int32)


# ------------------------------------------------------------------------------------------------ the edge meshes
def mesh_of(tri_verts, refl_coeff=0.8):
    """[n][3][3] triangle vertices -> mesh dict with a vertex triple of its own per triangle and flat normals"""
    v = np.asarray(tri_verts, np.float64).reshape(-1, 3)
    t = np.arange(len(v), dtype=np.uint32).reshape(-1, 3)
    nrm = np.repeat(np.cross(v[1::3] - v[0::3], v[2::3] - v[0::3]) + 1e-30, 3, axis=0) if len(v) else np.zeros((1, 3))
    if len(v):
        nrm = nrm / np.linalg.norm(nrm, axis=1, keepdims=True)
    return dict(tris=t, verts=v, normals=nrm, refl_coeff=refl_coeff, refr_index=1.0)


def soup(n, seed):
    """n triangles of the mix of test_random_triangle_soups_brute_force: ordinary triangles of mixed size, long thin diagonal
    slivers and a fan of thin wedges around one vertex, shuffled so that a cut to any n keeps the mix"""
    rng = np.random.default_rng(seed)
    n_reg, n_sliver, n_fan = n // 2 + 1, n // 5 + 1, (3 * n) // 10 + 1
    tris = []
    for _ in range(n_reg):
        c = rng.normal(0, 6.0, 3); s = 10 ** rng.uniform(-1.5, 0.7)
        tris.append(c + rng.normal(0, s, (3, 3)))
    for _ in range(n_sliver):
        a = rng.normal(0, 6.0, 3); d = rng.normal(0, 1, 3); d /= np.linalg.norm(d)
        L = rng.uniform(5, 25); w = rng.normal(0, 1, 3) * 10 ** rng.uniform(-4, -1.5)
        tris.append(np.stack([a, a + L * d, a + 0.5 * L * d + w]))
    hub = rng.normal(0, 3.0, 3)
    ang = np.sort(rng.uniform(0, 2 * np.pi, n_fan + 1)); rad = rng.uniform(2, 8)
    e1 = np.array([0.0, 1.0, 0.2]); e2 = np.array([0.1, -0.2, 1.0])
    for i in range(n_fan):
        tris.append(np.stack([hub, hub + rad * (np.cos(ang[i]) * e1 + np.sin(ang[i]) * e2), hub + rad * (np.cos(ang[i + 1]) * e1 + np.sin(ang[i + 1]) * e2)]))
    tris = np.stack(tris)[rng.permutation(len(tris))[:n]]
    assert tris.shape[0] == n
    return tris


SOUP_SIZES = (1, 2, 3, 4, 5, 255, 256, 257, 1023, 1024, 1025, 2049)
FAR_SHIFT = np.array([41234.5, -30987.25, 20011.125])
SHAPE = np.array([[0.0, 0.0, 0.0], [0.0, 1.0, 0.0], [0.0, 0.0, 1.0]])          # faces -x, where the walk test's beam comes from


def invalid_mesh():
    """five triangles, every one with a bad x coordinate: NaN, +Inf, -Inf, 3.5e38 (finite in f64, beyond a padded f32 box), NaN"""
    tris = soup(5, 905)
    m = mesh_of(tris)                                        # (normals from the clean vertices)
    for i, (k, bad) in enumerate([(0, np.nan), (1, np.inf), (2, -np.inf), (0, 3.5e38), (2, np.nan)]):
        m["verts"][3 * i + k, 0] = bad
    return m


def _soup_with_invalid():
    m = mesh_of(soup(257, 257))
    m["verts"][3 * 0 + 0, 0] = np.nan; m["verts"][3 * 128 + 1, 1] = np.inf; m["verts"][3 * 256 + 2, 2] = 3.5e38
    return [m, invalid_mesh()]


def _duplicates():
    rng = np.random.default_rng(11)
    one = np.array([2.0, -1.0, 0.5]) + rng.normal(0, 3.0, (3, 3))
    return [mesh_of(np.tile(one, (1025, 1, 1)))]


def _line():
    """one shape, stretched and moved along x only: the y and z of every box centre are the same bits"""
    rng = np.random.default_rng(12)
    shape = rng.normal(0, 0.01, (3, 3))
    tris = shape[None] * np.stack([rng.uniform(0.5, 2.0, 300), np.ones(300), np.ones(300)], axis=1)[:, None, :]
    tris = tris + np.stack([rng.uniform(-5, 5, 300), np.zeros(300), np.zeros(300)], axis=1)[:, None, :]
    return [mesh_of(tris)]


def _geometric():
    tris = (1e-3 * SHAPE)[None] + np.stack([2.0 ** -np.arange(48.0), np.zeros(48), np.zeros(48)], axis=1)[:, None, :]
    return [mesh_of(tris)]


def _huge():
    rng = np.random.default_rng(13)
    tiny = rng.normal(0, 3.0, (256, 1, 3)) + rng.normal(0, 0.01, (256, 3, 3))
    d = np.array([1.0, 1.0, 1.0]) / np.sqrt(3.0)
    sliver = np.stack([-20 * d, 20 * d, np.array([1e-3, -1e-3, 0.0])])                               # long, thin, diagonal
    flat = np.array([[-20.0, -20.0, 0.5], [20.0, -20.0, 0.5], [-20.0, 20.0, 0.5]])                   # axis-aligned, a box of zero thickness
    eq1 = np.array([[0.0, 17.0, 3.0], [-15.0, -9.0, -2.0], [15.0, -8.0, 1.0]])                       # large, near equilateral
    eq2 = np.array([[2.0, 1.0, 16.0], [-3.0, 14.0, -9.0], [1.0, -15.0, -8.0]])
    return [mesh_of(np.concatenate([tiny, np.stack([sliver, flat, eq1, eq2])]))]


DEGENERATE_PRIMS = (30, 31)          # of _degenerate(): the point and the collinear triangle


def _degenerate():
    rng = np.random.default_rng(14)
    ordinary = rng.normal(0, 4.0, (30, 1, 3)) + rng.normal(0, 1.0, (30, 3, 3))
    p = np.array([1.5, -2.25, 0.75]); a = np.array([-1.0, 2.0, 0.5]); d = np.array([0.015625, 0.03125, -0.015625])
    return [mesh_of(np.concatenate([ordinary, np.stack([np.stack([p, p, p]), np.stack([a, a + d, a + 2 * d])])]))]


def _five():
    empty = dict(tris=np.zeros((0, 3), np.uint32), verts=np.zeros((0, 3)), normals=np.zeros((1, 3)), refl_coeff=0.9, refr_index=1.0)
    return [mesh_of(soup(300, 300)), empty, mesh_of(soup(1, 901)), invalid_mesh(), mesh_of(soup(5, 902))]


def _cases():
    cases = {"soup%d" % n: (lambda n=n: [mesh_of(soup(n, n))]) for n in SOUP_SIZES}
    cases.update(dup1025=_duplicates, line300=_line, geo48=_geometric, invalid257=_soup_with_invalid, huge260=_huge, degen32=_degenerate,
                 far257=lambda: [mesh_of(soup(257, 258) + FAR_SHIFT)], five=_five)
    return cases


CASES = _cases()                       # name -> () -> list of meshes (one scene)
WALK_CASES = ("soup1", "soup5", "soup257", "soup1025", "dup1025", "geo48", "five")
# where the five meshes of "five" stand in the walk test (the mesh without a valid triangle far off the beam: the oracle's brute force
# tests the f64 triangle with the 3.5e38 vertex, which no hierarchy holds)
FIVE_POSITIONS = ((0.0, 0.0, 0.0), (0.0, 0.0, 0.0), (-25.0, 3.0, -2.0), (0.0, 500.0, 0.0), (-30.0, -4.0, 5.0))
_built = {}


def case_meshes(name):
    """the meshes of a case, built once (seeded: the same arrays in every test and on every machine's numpy Generator)"""
    if name not in _built:
        _built[name] = CASES[name]()
    return _built[name]
