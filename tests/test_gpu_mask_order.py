"""GPU tests (-m gpu) of the order in which the per-pulse scene update walks the primitives (RtsScene::d_prim_order: by first
appearance in the hierarchy's leaf slots, rts_amd/csrc/rts_prim_order.h) and of the primary-ray mask it rasterises in that order
(rts_mask_mark, rts_bvh.hip: an LDS tile per block, a patch larger than the tile cut into bands of rows).

Nothing a caller can observe may depend on either: every case traces the same pulse on a default handle (pre-filter and mask
on) and on a handle created with RTS_FLAG_NO_PREFILTER (no mask) and compares the received sets and the responses bit for
bit, the RtsStats segments / shaded / received, and both against the oracle's brute force over all primitives.  A mask cell
that a triangle should have marked and did not loses that triangle's primary hits on the default handle only; a leaf record
written at another index than its primitive's, or not at all, changes the hits of both against the oracle.

All scenes: the transmitter at (-1000, 0, 0) looking along +x, small triangles facing it in the plane x = 0, a capture
sphere around the transmitter wide enough for their mirror reflections.  The mask has 1024 x 1024 cells over the beam (spans of
at least 0.0103 rad), u along y (32 cells per word), v along z (rows); a span of 0.02 rad is 20 m at the targets, 51 cells per
metre.  W = 24: 13 824 launch indices on 24 x 24 lattice directions 20 / 23 = 0.87 m apart at the targets (span 0.02), which the
24 x layers of the lattice pull towards the boresight by up to 10 % -- the primary rays lie on 576 short radial lines.  Where a
case wants every triangle hit, the triangles are centred on lattice directions (lattice_centres)."""
import math

import numpy as np
import pytest

import helpers as H

pytestmark = pytest.mark.gpu

W = 24
ORIGIN = (-1000.0, 0.0, 0.0)


# ------------------------------------------------------------------------------- scenes (inputs only)
def tri_mesh(centres, size, x=0.0):
    """one triangle of width and height `size` per centre (y, z), facing -x, each with its own three vertices"""
    c = np.asarray(centres, np.float64).reshape(-1, 2)
    h = size / 2.0
    v = np.zeros((c.shape[0], 3, 3))
    v[:, :, 0] = x
    v[:, 0, 1] = c[:, 0] - h; v[:, 0, 2] = c[:, 1] - h
    v[:, 1, 1] = c[:, 0] + h; v[:, 1, 2] = c[:, 1] - h
    v[:, 2, 1] = c[:, 0];     v[:, 2, 2] = c[:, 1] + h
    verts = v.reshape(-1, 3)
    return dict(tris=np.arange(verts.shape[0], dtype=np.uint32).reshape(-1, 3), verts=verts,
                normals=np.tile(np.array([[-1.0, 0.0, 0.0]]), (verts.shape[0], 1)), refl_coeff=0.9, refr_index=1.0)


def grid_centres(lo, hi, n, cols=17):
    """n centres on a grid of `cols` columns over the square [lo, hi]^2, row by row"""
    pitch = (hi - lo) / cols
    k = np.arange(n)
    return np.stack([lo + pitch * (k % cols + 0.5), lo + pitch * (k // cols + 0.5)], 1), pitch


PITCH = 20.0 / (W - 1)                    # of the lattice directions at the targets, span 0.02


def lattice_centres(n, cols):
    """n centres ON lattice directions of the span-0.02 beam (`cols` even), row by row, the block of columns centred on the
    boresight and the rows starting as far below it"""
    first = -PITCH * (cols - 1) / 2.0
    k = np.arange(n)
    return np.stack([first + PITCH * (k % cols), first + PITCH * (k // cols)], 1)


def interleaved_clusters(lo, hi):
    """514 triangles, 257 in the square [-hi, -lo]^2 and 257 in [lo, hi]^2: even ids in the first, odd ids in the second"""
    a, pitch = grid_centres(lo, hi, 257)
    c = np.zeros((514, 2))
    c[0::2] = -a
    c[1::2] = a
    return tri_mesh(c, 0.7 * pitch)


def make_spec(rts, meshes, span=0.02, positions=None, max_refl=2):
    positions = positions or [(0.0, 0.0, 0.0)] * len(meshes)
    return dict(name="mask-order", W=W, max_refl=max_refl, smooth=True, n_pulses=1, meshes=meshes,
                motion=[dict(position=p, velocity=(0.0, 0.0, 0.0)) for p in positions],
                tx=dict(origin=ORIGIN, span=(span, span, 0.1), dir=(0.0, 0.0)),
                rx=[rts.rx_sphere(ORIGIN, 0.0, 0.0, 60.0, math.pi / 2, math.pi / 2)], carrier=10.0e9, c=299792458.0)


# ------------------------------------------------------------------------------- comparisons
def _received_of(o):
    idx = np.nonzero(o["results"]["received"] >= 0)[0]
    return dict(results=o["results"][idx], path=o["path"][idx], rcs_angle=o["rcs_angle"][idx], slots=idx.astype(np.uint64))


def _same_received(a, b, what, exact=True):
    """between two handles every byte agrees; against the oracle the RCS angles have the tolerance of tests/test_gpu_parity.py
    (libm and OCML atan2 differ in last bits)"""
    assert np.array_equal(a["slots"], b["slots"]), what
    assert np.array_equal(a["path"], b["path"]), what
    H.assert_prd_equal(a["results"], b["results"], what)
    if exact:
        assert a["rcs_angle"].tobytes() == b["rcs_angle"].tobytes(), what
    else:
        np.testing.assert_allclose(a["rcs_angle"], b["rcs_angle"], rtol=0, atol=1e-12)


def _responses(rts, tr, spec):
    tr.finalise_uniform(None, spec["c"] / spec["carrier"], 1.0, 1.0, spec["carrier"], spec["c"])
    return rts.groups_to_responses(tr.aggregate(spec["c"], spec["carrier"]))


def _oracle_responses(O, o, spec):
    """the reference's filter / finalise / O(R^2) aggregation on the oracle's trace, as __graft_entry__.smoke() forms them"""
    wl = spec["c"] / spec["carrier"]
    rx, rxi, _ = O.filter_finalise(o["results"], o["path"], [1.0] * len(spec["meshes"]), wl, 1.0, 1.0, spec["carrier"], spec["c"])
    lit = O.aggregate_literal(rx, rxi, spec["c"], spec["carrier"], spec["W"] ** 3)
    uniq = O.unique_paths(lit["pathMatch"])
    return uniq, lit["results"]["power"][uniq], lit["delay"][uniq]


def _pulse(rts, spec, tr, motion):
    _, st = H.gpu_trace(rts, spec, tr=tr, motion=motion)
    got = tr.received()                                      # (before the finaliser rewrites power and Doppler in place)
    return st, got, _responses(rts, tr, spec)


def check_pulse(rts, oracle, spec, masked, plain, others=(), motion=None, what="", rebuilt=None):
    """one pulse of `spec` on the default handle `masked`, on the RTS_FLAG_NO_PREFILTER handle `plain` and on every handle of
    `others` (default handles: another builder, a shared scene): the three comparisons of this file.  Returns the default
    handle's stats and the oracle's trace."""
    motion = motion if motion is not None else spec["motion"]
    sm, gm, rm = _pulse(rts, spec, masked, motion)
    sp, gp, rp = _pulse(rts, spec, plain, motion)
    _same_received(gm, gp, what + ": default handle against NO_PREFILTER")
    assert rm.tobytes() == rp.tobytes(), what + ": responses, default handle against NO_PREFILTER"
    assert (sm["segments"], sm["shaded"], sm["received"]) == (sp["segments"], sp["shaded"], sp["received"]), what
    if rebuilt is not None:
        assert sm["bvh_rebuilt"] == rebuilt and sp["bvh_rebuilt"] == rebuilt, what
    for k, tr in enumerate(others):
        so, go, ro = _pulse(rts, spec, tr, motion)
        _same_received(gm, go, "%s: handle %d against the default handle" % (what, k))
        assert rm.tobytes() == ro.tobytes(), "%s: responses of handle %d" % (what, k)
        assert (sm["segments"], sm["shaded"], sm["received"]) == (so["segments"], so["shaded"], so["received"]), (what, k)
    o = H.oracle_trace(oracle, spec, motion=motion)
    _same_received(_received_of(o), gm, what + ": default handle against the oracle", exact=False)
    assert (sm["segments"], sm["shaded"]) == (o["counters"]["segments"], o["counters"]["shaded"]), what
    uniq, power, delay = _oracle_responses(oracle, o, spec)
    assert np.array_equal(rm["ray"].astype(np.int64), uniq.astype(np.int64)), what
    np.testing.assert_allclose(rm["power"], power, rtol=1e-9)
    np.testing.assert_allclose(rm["delay"], delay, rtol=1e-9)
    return sm, o


def pair(rts, spec, **kw):
    return H.gpu_tracer(rts, spec, **kw), H.gpu_tracer(rts, spec, pre_filter=False, **kw)


def hit_counts(o, n_prims):
    hp = o["hit_prim"][:, 0]
    return np.bincount(hp[hp >= 0], minlength=n_prims)


# ------------------------------------------------------------------------------- cases
@pytest.mark.parametrize("span,lo,hi", [(0.02, 6.0, 9.5), (0.011, 1.5, 5.2)])
def test_interleaved_clusters(rts, oracle, span, lo, hi):
    """Two clusters at opposite corners of the beam (+-10 m, +-5.5 m at the targets), even ids in one and odd ids in the other: in
    mesh order the patch of each of the three blocks spans both clusters (15-19 m of 20: some 20 000 tile words); the leaf
    order must undo that.  span 0.02: one cluster is 3.5 m = 180 cells, 7 words x 182 rows -- it fits the 2 048-word tile.
    span 0.011 (the same layout scaled with the beam): one cluster is 3.7 m = 345 cells, 12 words x 347 rows = 4 164 words, three
    bands of 170 rows.  Whatever the leaf order, 514 triangles are 257 + 257: one block holds triangles of both clusters and
    goes through the bands too.  The triangles (0.14 m) are finer than the lattice: the primary rays hit a quarter to a half
    of them, in both clusters."""
    mesh = interleaved_clusters(lo, hi)
    spec = make_spec(rts, [mesh], span=span)
    masked, plain = pair(rts, spec)
    st, o = check_pulse(rts, oracle, spec, masked, plain, what="interleaved clusters, span %g" % span, rebuilt=1)
    cnt = hit_counts(o, 514)
    assert (cnt[0::2] > 0).sum() > 50 and (cnt[1::2] > 0).sum() > 50 and st["received"] > 250
    masked.close(); plain.close()


@pytest.mark.parametrize("n_prims", [1, 255, 256, 257])
def test_block_edges(rts, oracle, n_prims):
    """the last thread of a block, a full block, one primitive in the second block; each triangle has three normals of its own,
    so the trailing normals blocks start at 3, 765, 768 and 771 normals (256: exactly three blocks; 257: the fourth)"""
    c = lattice_centres(272, 16)                                               # 16 columns x 17 rows, each centre on a lattice direction
    order = np.argsort(np.abs(c).max(axis=1), kind="stable")[:n_prims]        # from the middle of the beam outwards
    spec = make_spec(rts, [tri_mesh(c[order], 0.6 * PITCH)])
    masked, plain = pair(rts, spec)
    st, o = check_pulse(rts, oracle, spec, masked, plain, what="%d primitives" % n_prims, rebuilt=1)
    assert (hit_counts(o, n_prims) > 0).all() and st["received"] > 0
    masked.close(); plain.close()


def sliver_fan(n=64, radius=8.0):
    """a disc of n slivers around one shared centre vertex: the boxes of the diagonal ones are mostly empty"""
    a = 2.0 * math.pi * np.arange(n) / n
    verts = np.concatenate([np.zeros((1, 3)), np.stack([np.zeros(n), radius * np.cos(a), radius * np.sin(a)], 1)])
    tris = np.stack([np.zeros(n, np.int64), 1 + np.arange(n), 1 + (np.arange(n) + 1) % n], 1).astype(np.uint32)
    return dict(tris=tris, verts=verts, normals=np.tile(np.array([[-1.0, 0.0, 0.0]]), (n + 1, 1)), refl_coeff=0.9, refr_index=1.0)


@pytest.mark.parametrize("builder", ["device", "host"])
def test_sliver_fan_every_record_at_its_own_index(rts, oracle, monkeypatch, builder):
    """64 slivers that the builders cut into several references each (more leaf slots than primitives: the order keeps the first
    slot of each), on RTS_FLAG_KEEP_ALL_RAYS handles: hit_prim of every launch index is the oracle's, and the primary rays
    hit every one of the 64 primitives -- every record was written, and at its own index (a record at another index would
    answer with another triangle's geometry: other hits, other distances)."""
    monkeypatch.setenv("RTS_BUILDER", builder)
    spec = make_spec(rts, [sliver_fan()])
    n = W ** 3
    masked, plain = pair(rts, spec, keep_all=True)
    info = masked.scene_info()
    assert info["builder"] == (1 if builder == "device" else 0) and info["n_prims"] == 64
    assert info["n_leaves"] > 64, info
    st, o = check_pulse(rts, oracle, spec, masked, plain, what="sliver fan, %s builder" % builder, rebuilt=1)
    assert (hit_counts(o, 64) > 0).all()
    a, b = masked.all_rays(n), plain.all_rays(n)
    H.compare_full(o, a, n)
    H.compare_full(o, b, n)
    masked.close(); plain.close()


def _with_background(extra):
    """a 4 x 4 grid of 0.5 m triangles on the lattice directions around the boresight (each inside the 4 096-cell limit: 26 x 26
    cells + the margin) and, behind them at x = 5, the triangle under test"""
    bg = tri_mesh(lattice_centres(16, 4), 0.5)
    verts = np.concatenate([bg["verts"], np.asarray(extra, np.float64)])
    tris = np.concatenate([bg["tris"], np.array([[48, 49, 50]], np.uint32)])
    return dict(tris=tris, verts=verts, normals=np.tile(np.array([[-1.0, 0.0, 0.0]]), (51, 1)), refl_coeff=0.9, refr_index=1.0)


DISABLING = {
    # 1 m wide (51 cells: two or three words of a row) across the rim of the mask at y = +10.02 m and its upper rim at z = +10.02 m
    "rim and word boundary": [[5.0, 9.4, 9.3], [5.0, 10.4, 9.3], [5.0, 9.9, 10.4]],
    # 6 m x 6 m: 307 x 307 cells > RTS_MASK_MAX_CELLS -- no mask for the pulse; the small triangles in front shadow part of it
    "larger than the cell limit": [[5.0, -3.0, -3.0], [5.0, 3.0, -3.0], [5.0, 0.0, 3.0]],
    # one vertex 100 m behind the transmitter: its projection is not a triangle -- no mask for the pulse; the part in the beam is hit
    "a vertex behind the transmitter": [[-1100.0, 0.0, -6.0], [200.0, 1.5, -6.0], [200.0, -1.5, -6.0]],
}


@pytest.mark.parametrize("case", sorted(DISABLING))
def test_disabling_cases(rts, oracle, case):
    """a triangle on the mask's rim is clipped to it; a triangle too large to rasterise, or not wholly in front of the
    transmitter, voids the mask for the pulse: in none of them a hit is lost -- the triangle under test (primitive 16) and the
    16 small ones are all hit, as the oracle says, with and without the pre-filter"""
    spec = make_spec(rts, [_with_background(DISABLING[case])])
    masked, plain = pair(rts, spec)
    st, o = check_pulse(rts, oracle, spec, masked, plain, what=case, rebuilt=1)
    assert (hit_counts(o, 17) > 0).all(), hit_counts(o, 17)
    masked.close(); plain.close()


@pytest.mark.parametrize("builder", ["device", "host"])
def test_two_targets_shared_scene_and_a_beam_only_pulse(rts, oracle, monkeypatch, builder):
    """two targets (the interleaved clusters and, placed 4 m further and 1 m up, a 10 x 10 grid in the gap between them: global
    primitive ids 514 ..., an order over both hierarchies), the builder named by RTS_BUILDER, a second default handle that SHARES
    the first one's scene (and with it the order).  Pulse 1 places the targets; pulse 2 moves a target (records and mask in one
    pass); pulse 3 only turns the beam: the mask-only pass walks the same order over the world vertices."""
    monkeypatch.setenv("RTS_BUILDER", builder)
    c, pitch = grid_centres(-4.0, 4.0, 100, cols=10)
    spec = make_spec(rts, [interleaved_clusters(6.0, 9.5), tri_mesh(c, 0.6 * pitch)], positions=[(0.0, 0.0, 0.0), (4.0, 0.0, 1.0)])
    masked, plain = pair(rts, spec)
    shared = rts.Tracer(spec["W"], spec["max_refl"], 0, spec["smooth"])
    shared.share_scene(masked); shared.set_receivers(spec["rx"])
    info = masked.scene_info()
    assert info["builder"] == (1 if builder == "device" else 0) and info["n_prims"] == 614 and info["handles_sharing"] == 2
    what = "two targets, %s builder" % builder
    st, o = check_pulse(rts, oracle, spec, masked, plain, others=[shared], what=what + ", pulse 1", rebuilt=1)
    cnt = hit_counts(o, 614)
    assert (cnt[:514] > 0).sum() > 100 and (cnt[514:] > 0).sum() > 50
    rot = rts.rotation_matrix(0.0, 0.0, 0.3)                                   # the grid rolls about the beam axis and shifts
    moved = [spec["motion"][0], dict(position=(4.0, -0.7, 0.4), velocity=(0.0, 0.0, 0.0), rotation=rot)]
    check_pulse(rts, oracle, spec, masked, plain, others=[shared], motion=moved, what=what + ", pulse 2", rebuilt=1)
    turned = dict(spec, tx=dict(spec["tx"], dir=(0.002, -0.0015)))
    st3, o3 = check_pulse(rts, oracle, turned, masked, plain, others=[shared], motion=moved, what=what + ", pulse 3", rebuilt=0)
    assert st3["received"] > 100
    masked.close(); plain.close(); shared.close()
