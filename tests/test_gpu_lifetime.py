"""Lifetime of a handle's device and pinned memory (-m gpu): what handles take they give back when they are destroyed, in either
order of destruction, and a shared scene lives exactly as long as its last user.  The buffers free themselves (rts_owned.h:
DevBuf, PinBuf, StagedUpload -- tests/test_owned_host.py has their rules without a GPU); this file checks the handle built from them."""
import math

import numpy as np
import pytest

import helpers as H

pytestmark = pytest.mark.gpu
CS, FC = 299792458.0, 1.0e10
T0, DT, NB = 6.0e-6, 2.0e-8, 64                  # the sphere's returns arrive after 2 x 1 km / c = 6.67 us


@pytest.fixture(scope="module")
def spec():
    """the smallest scene that still reaches every buffer: W = 8, one icosphere of 20 triangles, two receivers"""
    from rts_amd import scenes as S
    s = S.config2(subdiv=0, W=8, rx_radius=400.0)
    assert s["meshes"][0]["tris"].shape[0] == 20
    s["rx"] = [S._rx_at((-1000.0, 30.0 * k, 0.0), (0, 0, 0), 400.0, math.pi / 2) for k in range(2)]
    s["rx70"] = [S._rx_at((-1000.0, 3.0 * k, 1.0 * k), (0, 0, 0), 400.0, math.pi / 2) for k in range(70)]
    return s


def _trace(t, s):
    tx = s["tx"]
    return t.trace(tx["origin"], tx["span"], tx["dir"], s["motion"])


def _cycle(rts, s, owner_first):
    """three handles, two pulses each, every feature that owns memory; then all three destroyed"""
    tx = s["tx"]; wl = CS / FC; P = rts.Pattern.constant
    # plain handle: device-built scene, patterns, the host mirror, a receiver set that grows (the pinned receiver staging regrows),
    # a cube of its own, a waveform, render / compress / Doppler / detect / spectrogram / backprojection
    a = H.gpu_tracer(rts, s)
    # host-build handle: builds a scene of its own, drops it for a's, joins a's link group
    h = H.gpu_tracer(rts, s, device_build=False)
    assert h.scene_info()["builder"] == 0 and a.scene_info()["builder"] == 1
    h.share_scene(a); h.link(a); h.set_receivers(s["rx"])
    assert a.scene_info()["handles_sharing"] == 2
    # keep-all handle with refraction: child slab, hit rows, 64-bit ordering keys
    k = rts.Tracer(s["W"], s["max_refl"], 1, s["smooth"], keep_all=True); k.set_scene(s["meshes"]); k.set_receivers(s["rx"])

    for n, rx in ((2, s["rx"]), (70, s["rx70"])):
        a.set_receivers(rx); a.set_patterns(P(1.0), [P(1.0)] * n, [P(0.5)])
        pos = np.array([r["centre"] for r in rx]); rot = np.zeros((n, 4))
        a.trace_begin(tx["origin"], tx["span"], tx["dir"], s["motion"])
        a.received_prefetch()
        assert len(a.received_view()["results"]) == a.received_count() > 0
        a.finalise_patterns(pos, rot, wl, FC, CS)
        a.aggregate(CS, FC)
    a.cube_attach(70, 2, NB, T0, DT); a.cube_set_waveform(rts.Waveform.lfm(32, 0.5, 8))
    a.cube_render(0, "rays", CS, FC); a.cube_render(1, "paths")
    a.cube_compress(); a.cube_doppler(4, fetch=False); a.cube_detect(guard=(1, 0), train=(2, 1), pfa=1e-3)
    # ... and the two products behind a staged upload (library-owned outputs): with the pattern rows above, all three are armed at the end
    a.cube_spectrogram(2, 1, 2, window=[1.0, 0.5], fetch=False)
    a.cube_backproject((0.0, 0.0, 0.0), (1.0, 0.0, 0.0), (0.0, 1.0, 0.0), 2, 2, np.tile(tx["origin"], (2, 1)), np.repeat(pos[:, None, :], 2, axis=1), CS, FC, fetch=False)
    for _ in range(2):
        _trace(h, s); h.finalise_uniform(None, wl, 1.0, 1.0, FC, CS); h.aggregate(CS, FC)
        _trace(k, s); k.all_rays(s["W"] ** 3); k.received()
    for t in ((a, k, h) if owner_first else (h, k, a)):
        t.close()


N_CYCLES = 8


def test_handles_give_back_what_they_took(rts, spec):
    """Free device memory (torch.cuda.mem_get_info) after one warm-up cycle and after N_CYCLES more cycles of _cycle, odd cycles
    destroying the scene's owner first and even cycles last.

    Allowed loss: the largest loss of this same body on the parent commit, whose rts_destroy released every buffer by hand, plus
    half of N_CYCLES x 64 KiB -- 64 KiB is the smallest block a forgotten DevBuf<char> keeps, so one leaked buffer per cycle is
    twice the margin.

    NOT MEASURED: the parent's three figures were never taken, and no build with one member's release taken out has been run
    against this test, so it is not shown that mem_get_info resolves one leaked 64 KiB block per cycle
    (profiles/owned_buffers_refactor.txt says the same).  PARENT_LOSS_BYTES is therefore set to the smallest loss the parent can
    have, none at all: that makes the bound the tightest the rule allows (a measured parent loss could only widen it), and
    N_CYCLES = 8 satisfies "N x 64 KiB is at least four times the parent's largest loss" trivially.  Whoever measures the parent
    replaces the three zeros, raises N_CYCLES if the rule then asks for it, and records the mutation's result."""
    import torch
    PARENT_LOSS_BYTES = (0, 0, 0)                   # placeholder, see above: not a measurement
    assert N_CYCLES * 65536 >= 4 * max(PARENT_LOSS_BYTES)
    _cycle(rts, spec, True)
    torch.cuda.synchronize()
    before = torch.cuda.mem_get_info()[0]
    for i in range(1, N_CYCLES + 1):
        _cycle(rts, spec, i % 2 == 1)
    torch.cuda.synchronize()
    after = torch.cuda.mem_get_info()[0]
    print("free device memory: before %d, after %d cycles %d, lost %d bytes" % (before, N_CYCLES, after, before - after))
    assert before - after <= max(PARENT_LOSS_BYTES) + N_CYCLES * 65536 // 2


@pytest.mark.parametrize("first_gone", ["builder", "sharer"])
def test_shared_scene_outlives_either_owner(rts, spec, first_gone):
    """A builds the scene, B shares it and is linked to A.  The one that stays traces a pulse, the other is destroyed, the same
    pulse again: every field of the received records bit for bit, and rts_scene_info unchanged but for the count of handles"""
    a = H.gpu_tracer(rts, spec)
    b = rts.Tracer(spec["W"], spec["max_refl"], 0, spec["smooth"]); b.share_scene(a); b.link(a); b.set_receivers(spec["rx"])
    stay, go = (b, a) if first_gone == "builder" else (a, b)
    _trace(stay, spec); want = stay.received(); info = stay.scene_info()
    assert info["handles_sharing"] == 2 and len(want["results"]) > 0
    go.close()
    _trace(stay, spec); got = stay.received(); info2 = stay.scene_info()
    H.assert_prd_equal(want["results"], got["results"], "after the %s went" % first_gone)
    assert np.array_equal(want["path"], got["path"]) and np.array_equal(want["slots"], got["slots"])
    assert want["rcs_angle"].tobytes() == got["rcs_angle"].tobytes()
    assert info2.pop("handles_sharing") == 1 and info.pop("handles_sharing") == 2 and info2 == info
    stay.close()
