"""Clutter and jammer sources on the device (rts_cube_add_sources, rts_amd/csrc/rts_source.hip) against the host evaluator
rts_sources_eval within the agreement bound of tests/source_ref.py (the two run the same tree and differ only through log, cos and
sin of the draws), over the smallest shapes at which the kernel can go wrong:
  * patches 1, 63, 64, 65 (one lane, the last lane empty, every lane, the second register slot), 130, 360 and 1024 (4, 8 and 16 slots);
  * receivers 1, 8, 9 and 64 (the staging holds 16, 16, 14 and 2 pulses);
  * bins 1, 3, 4, 5, 255, 256, 257 and -- the workgroup's tile is RTS_SRC_TILE = 8 adjacent bins -- 7, 8, 9, 15, 16, 17;
  * pulses 1, 2, 33 (two full stagings of 16 and one more) and 4 096;
  * rho mixed from {0, 0.5, 0.9, 1} and all 1 (no draw after pulse 0); a profile with zeros at the first bin, the last bin and both
    sides of a tile edge.
Then what must hold byte for byte on the device (run to run, across launch histories, one call against two with disjoint gates), a
pre-filled caller-owned cube, the gated bins, the refusals, and the two recipes end to end."""
import ctypes as C
import math

import numpy as np
import pytest

import adapt_ref as A
import source_ref as R
import stap_ref as S

pytestmark = pytest.mark.gpu
T = R.TILE


def handle(rts, n_rx, n_p, nb, device_ptr=None):
    tr = rts.Tracer(8, 1)
    tr.cube_attach(n_rx, n_p, nb, 0.0, 1.0, device_ptr=device_ptr)
    return tr


def device_result(rts, shape, src):
    tr = handle(rts, *shape)
    tr.cube_add_sources(**src)
    out = tr.cube()
    tr.close()
    return out


def dev(a):
    """(torch's stream is not the handles': the buffer is finished before a handle reads it, and a handle's work before torch reads it)"""
    import torch
    buf = torch.from_numpy(np.array(a, np.complex128, order="C")).to("cuda")
    torch.cuda.synchronize()
    return buf


def host(buf):
    import torch
    torch.cuda.synchronize()
    return buf.cpu().numpy()


# ----------------------------------------------------------------------------- 1. against the evaluator
#        K, n_rx, n_pulses, n_bins, rho, profile
CASES = [(K, 2, 3, 9, "mixed", None) for K in (1, 63, 64, 65, 130, 360)] + [(1024, 4, 2, 3, "mixed", None), (1024, 4, 2, 3, "ones", None)] + \
        [(5, n_rx, 3, 9, "mixed", "edges") for n_rx in (1, 8, 9)] + [(64, 64, 3, 3, "mixed", None)] + \
        [(5, 2, 2, nb, "mixed", None) for nb in (1, 3, 4, 5, T - 1, T, T + 1, 2 * T - 1, 2 * T, 2 * T + 1, 255, 256)] + [(70, 3, 2, 257, "mixed", "edges")] + \
        [(5, 2, n_p, 5, "mixed", None) for n_p in (1, 2, 33)] + [(65, 2, 33, 5, "ones", "edges"), (3, 9, 33, 9, 0.9, None), (65, 1, 4096, 2, "mixed", None), (65, 1, 4096, 2, "ones", None)]


@pytest.mark.parametrize("K,n_rx,n_pulses,n_bins,rho,profile", CASES)
def test_device_against_the_evaluator(rts, K, n_rx, n_pulses, n_bins, rho, profile):
    src = R.patches(K * 7 + n_bins, K, n_rx, n_bins, rho=rho, profile=profile)
    src["seed"] = (K << 40) + n_bins
    shape = (n_rx, n_pulses, n_bins)
    zero = np.zeros(shape, np.complex128)
    got, want = device_result(rts, shape, src), rts.sources_eval(zero, **src)
    worst = R.assert_within(got, want, R.bound(zero, src["spatial"], src["power"], src.get("range_profile")))
    print("worst difference / bound %.3g, byte-equal %s" % (worst, got.tobytes() == want.tobytes()))
    on = np.ones(n_bins, bool) if profile is None else src["range_profile"] != 0.0
    assert np.all(got[:, :, on] != 0) and not np.any(R.bits(got[:, :, ~on]))


# ----------------------------------------------------------------------------- 2. byte for byte on the device
def test_the_same_call_gives_the_same_bytes_whatever_came_before(rts):
    shape = (3, 20, 21)
    src = R.patches(31, 130, 3, 21, profile="edges"); src["seed"] = 99
    first = device_result(rts, shape, src)
    assert device_result(rts, shape, src).tobytes() == first.tobytes()                 # fresh handles, twice
    # another launch history: a larger cube with other tables (the staged upload and its device table regrow), noise, then the call
    tr = handle(rts, 8, 4, 300)
    tr.cube_add_sources(**R.patches(32, 360, 8, 300, profile="random"))
    tr.cube_add_noise(1.0, 5)
    tr.cube_attach(*shape, 0.0, 1.0)
    tr.cube_add_sources(**R.patches(33, 7, 3, 21))
    tr.cube_attach(*shape, 0.0, 1.0)
    tr.cube_add_sources(**src)
    assert tr.cube().tobytes() == first.tobytes()
    tr.close()


def test_disjoint_gates_equal_their_union(rts):
    shape = (2, 18, 2 * T + 3)
    src = R.patches(34, 65, 2, shape[2], profile="random"); src["seed"] = 3
    g1 = src["range_profile"].copy(); g2 = src["range_profile"].copy()
    g1[T + 1:] = 0.0; g2[:T + 1] = 0.0                                                # (the cut lies inside a tile)
    tr = handle(rts, *shape)
    tr.cube_add_sources(**dict(src, range_profile=g1)); tr.cube_add_sources(**dict(src, range_profile=g2))
    both = tr.cube()
    tr.close()
    assert both.tobytes() == device_result(rts, shape, src).tobytes()


# ----------------------------------------------------------------------------- 3. a pre-filled cube, the gated bins
def test_prefilled_caller_cube_and_gated_bins(rts):
    """a caller-owned cube (a torch tensor) ends as its values plus the zero-cube result, to the one rounding of the addition -- the
    same addition numpy makes; bins of profile 0 keep their bytes (a -0.0 among them: adding +0 would change it)"""
    shape = (3, 18, 2 * T + 1)
    rng = np.random.default_rng(35)
    before = R.B.random_complex(rng, shape) * 100.0
    src = R.patches(36, 66, 3, shape[2], profile="edges"); src["seed"] = 17
    off = src["range_profile"] == 0.0
    before[0, 0, 0] = complex(-0.0, -0.0)
    assert off[0] and off[-1] and off[T - 1] and off[2 * T] and off.sum() == 5
    d = dev(before)
    tr = handle(rts, *shape, device_ptr=d.data_ptr())
    tr.cube_add_sources(**src)
    tr.cube()                                                                           # (waits for the handle's stream)
    got = host(d)
    tr.close()
    z = device_result(rts, shape, src)
    assert np.array_equal(got[:, :, ~off], (before + z)[:, :, ~off])
    assert R.bits(got[:, :, off]).tobytes() == R.bits(before[:, :, off]).tobytes()
    R.assert_within(got, rts.sources_eval(before, **src), R.bound(before, src["spatial"], src["power"], src["range_profile"]))


# ----------------------------------------------------------------------------- 4. refusals
def test_refusals_leave_the_cube_and_the_handle_intact(rts):
    L = rts.L
    shape = (2, 5, 11)
    rng = np.random.default_rng(37)
    before = R.B.random_complex(rng, shape)
    base = R.patches(38, 9, 2, 11, profile="random"); base["seed"] = 8
    d = dev(before)
    tr = rts.Tracer(8, 1)
    with pytest.raises(rts.L.RtsError, match="no cube"):
        tr.cube_add_sources(**base)
    tr.cube_attach(*shape, 0.0, 1.0, device_ptr=d.data_ptr())

    def refused(word, null=None, flags=0, reserved=(0, 0), n_patches=None, **kw):
        s = dict(base); s.update(kw)
        p, alive = rts._source_params(s["spatial"], s["power"], s["doppler"], s.get("rho"), s.get("range_profile"), s["seed"], 2, 11)
        if null and null != "p":
            setattr(p, null, None)
        p.flags = flags; p.reserved[0], p.reserved[1] = reserved
        if n_patches is not None:
            p.n_patches = n_patches
        rc = L.lib().rts_cube_add_sources(tr.h, C.byref(p) if null != "p" else None)
        msg = L.lib().rts_last_error().decode()
        assert rc == L.RTS_ERR_INVALID and word in msg, (word, rc, msg)

    edit = lambda name, i, v: {name: (lambda x: (x.__setitem__(i, v), x)[1])(np.array(base.get(name, np.ones(9)), copy=True))}
    refused("null parameters", null="p"); refused("spatial", null="spatial"); refused("power", null="power"); refused("doppler", null="doppler")
    refused("flags", flags=2); refused("reserved", reserved=(0, 1)); refused("n_patches", n_patches=0); refused("n_patches", n_patches=R.MAX_PATCHES + 1)
    refused("spatial[4][1]", **edit("spatial", (4, 1), complex(math.nan, 0.0))); refused("power[3]", **edit("power", 3, -1.0)); refused("power[3]", **edit("power", 3, math.inf))
    refused("doppler[0]", **edit("doppler", 0, math.nan)); refused("rho[8]", **edit("rho", 8, 1.5)); refused("rho[8]", **edit("rho", 8, math.nan))
    refused("range_profile[10]", **edit("range_profile", 10, -1.0)); refused("range_profile[0]", **edit("range_profile", 0, math.inf))
    tr.cube()
    assert host(d).tobytes() == before.tobytes()
    # the limits that depend on the cube: n_rx above RTS_BEAM_MAX_RX, n_patches * n_rx above RTS_SRC_MAX_TABLE
    t2 = handle(rts, R.MAX_RX + 1, 1, 1)
    with pytest.raises(rts.L.RtsError, match="n_rx"):
        t2.cube_add_sources(np.ones((1, R.MAX_RX + 1)), [1.0], [0.0])
    t2.cube_attach(8, 1, 1, 0.0, 1.0)
    with pytest.raises(rts.L.RtsError, match="n_patches \\* n_rx"):
        t2.cube_add_sources(np.ones((513, 8)), np.ones(513), np.zeros(513))
    assert not np.any(t2.cube())
    t2.close()
    # the refused calls left no trace: a valid call now gives a fresh handle's bytes
    tr.cube_attach(*shape, 0.0, 1.0)
    tr.cube_add_sources(**base)
    assert tr.cube().tobytes() == device_result(rts, shape, base).tobytes()
    tr.close()


# ----------------------------------------------------------------------------- 5. the two recipes, end to end on the device
def test_jammer_recipe_on_the_device(rts):
    """zeroed cube -> cube_add_sources (K = 1, rho = 0, the jammer's steering row, 30 dB) -> cube_add_noise -> cube_covariance -> cube_mvdr:
    tests/adapt_ref.py's properties hold on the device's weights; the cube agrees with the host chain's within the sources' bound plus
    the noise generator's tolerance, covariance and weights with the evaluators on the device's own cube bit for bit (their agreement)"""
    sc = A.SCENE
    src, _ = R.jammer_recipe(rts)
    pos, directions, _ = A.scene_geometry()
    s = rts.steering(pos, directions, sc["wavelength"])
    tr = handle(rts, sc["n_rx"], sc["n_pulses"], sc["n_bins"])
    tr.cube_add_sources(**src)
    tr.cube_add_noise(sc["noise_power"], sc["seed"])
    tr.cube_covariance(skip=sc["skip"], fetch=False)
    w = tr.cube_mvdr(s, sc["noise_power"])
    cube, cov = tr.cube(), tr.covariance()
    tr.close()
    zero = np.zeros_like(cube)
    noise_h = R.noise(rts, sc)
    cube_h = rts.sources_eval(zero, **src) + noise_h
    R.assert_within(cube, cube_h, R.bound(zero, src["spatial"], src["power"]) + 1e-13 * (1.0 + np.abs(noise_h)) + R.EPS * np.abs(cube_h))
    cov_h = rts.covariance_eval(cube, skip=sc["skip"]); w_h = rts.mvdr_eval(cov_h, s, sc["noise_power"])
    assert cov.tobytes() == cov_h.tobytes() and np.asarray(w).tobytes() == w_h.tobytes()
    A.assert_mvdr_properties(w, s, cov, sc["noise_power"], src["spatial"][0], sc["jammer_beam"])


def test_clutter_recipe_on_the_device(rts):
    """zeroed cube -> cube_add_sources (the 89-patch ridge, rho = 1, seed 2027) -> cube_add_noise -> cube_st_covariance -> cube_mvdr ->
    cube_st_apply: scored in the scene's true covariance the device's weights are within 1 dB of the optimum and at least 20 dB above the
    conventional space-time beam; covariance, weights and output equal the evaluators' on the device's own cube bit for bit"""
    sc = S.SCENE
    taps = sc["taps"]
    src, _ = R.clutter_recipe(rts)
    tr = handle(rts, sc["n_rx"], sc["n_pulses"], sc["n_bins"])
    tr.cube_add_sources(**src)
    tr.cube_add_noise(sc["noise_power"], sc["seed"])
    y = tr.cube_stap(S.scene_spatial_steering(rts), [sc["target_f"]], taps, train=dict(skip=sc["skip"]), loading=sc["noise_power"])
    cube, cov, w = tr.cube(), tr.covariance(), tr.mvdr_weights()
    tr.close()
    zero = np.zeros_like(cube)
    noise_h = R.noise(rts, sc)
    cube_h = rts.sources_eval(zero, **src) + noise_h
    R.assert_within(cube, cube_h, R.bound(zero, src["spatial"], src["power"]) + 1e-13 * (1.0 + np.abs(noise_h)) + R.EPS * np.abs(cube_h))
    _, _, cov_h, w_h, y_h = S.scene_host(rts, taps, cube)
    assert cov.tobytes() == cov_h.tobytes() and w.tobytes() == w_h.tobytes() and np.asarray(y).tobytes() == y_h.tobytes()
    improvement, loss = R.stap_figures(rts, cube, w)
    print("improvement %.2f dB, loss %.2f dB" % (improvement, loss))
    assert loss <= 1.0
    assert improvement >= 20.0
