"""The return-cube kernels at their size limits and at the cube's edges (k_cube_render, k_cube_accumulate[_paths], k_cube_compress,
k_cube_doppler) against the longdouble restatement of tests/cube_ref.py.

Planted contributions.  One pulse of a scene is traced once; rts_finalise_values then sets every received ray's power and Doppler
(power 0 masks a ray), the cube's t0 / dt are free per rts_cube_attach, and with cspeed = 1 a ray's delay IS its rayLength.  So a
case picks a ray and solves t0 for the start d = (tau - t0) / dt it needs; d is formed on the host in float64 exactly as the
kernels form it, and the intended property of d is asserted before anything is launched.

Guarded buffers.  Every cube and transform output is caller-owned torch memory with one receiver plane of a finite sentinel
before and after it; the planes must come back bit-identical, so a write outside the cube fails an assertion.

Tolerances are the project's own (test_gpu_render.py, test_gpu_parity.py); rows that hold no live contribution must be exactly 0.
"""
import math
import time

import numpy as np
import pytest

import cube_ref as R
import helpers as H

pytestmark = pytest.mark.gpu

SENT = complex(12345.678901234567, -7654.321098765432)        # finite, odd: a stray atomic add leaves "not the sentinel"
CS, FC = 1.0, 0.4321          # cspeed 1: tau = rayLength bit for bit; carrier in cycles per unit length (phase argument ~1e3 rad)
DT = 0.125                    # a power of two: D * DT is exact
F0 = 0.11                     # planted Doppler: F0 * DT = 0.014 cycles per sample
P0 = 2.25                     # planted power (amplitude 1.5)
PULSES, ROW = 3, 1            # every cube has three rows per receiver and the middle one is rendered: rows 0 and 2 stay 0

WORST = {}                    # operation -> largest observed |device - reference| / max |reference|


@pytest.fixture(scope="module", autouse=True)
def report():
    t = time.time()
    yield
    print("\n[cube edges] wall %.1f s; largest observed error / max|ref| per operation: %s"
          % (time.time() - t, ", ".join("%s %.3g" % kv for kv in sorted(WORST.items()))))


def check(op, got, ref, rtol, atol, what=""):
    ref = R.to_double(ref)
    scale = np.abs(ref).max()
    err = float(np.abs(got - ref).max() / scale) if scale > 0 else float(np.abs(got).max())
    WORST[op] = max(WORST.get(op, 0.0), err)
    print("[cube edges] %-10s %-60s max|err|/max|ref| = %.3g" % (op, what, err))
    np.testing.assert_allclose(got, ref, rtol=rtol, atol=atol, err_msg="%s %s" % (op, what))


def check_render(got, ref, what):
    check("render", got, ref, 1e-10, 1e-12 * np.abs(R.to_double(ref)).max(), what)            # test_gpu_render.py:127


def check_impulse(got, ref, what):
    check("impulse", got, ref, 1e-10, 1e-13 * np.abs(R.to_double(ref)).max(), what)           # test_gpu_parity.py:553


# ----------------------------------------------------------------------------- guarded caller memory
class Guarded:
    """[n_rx][n_rows][n_bins] complex128 on the device between two receiver planes of SENT; fill: initial content (default 0)"""

    def __init__(self, n_rx, n_rows, n_bins, fill=None):
        import torch
        self.shape = (n_rx, n_rows, n_bins)
        self.plane = n_rows * n_bins
        self.buf = torch.full(((n_rx + 2) * self.plane,), SENT, dtype=torch.complex128, device="cuda")
        inner = self.buf[self.plane:(n_rx + 1) * self.plane]
        if fill is None:
            inner.zero_()
        else:
            inner.copy_(torch.from_numpy(np.ascontiguousarray(fill, np.complex128).ravel()))
        torch.cuda.synchronize()                       # (the library works on its handles' own streams)
        self.ptr = inner.data_ptr()

    def read(self):
        """the cube; asserts the guard planes.  The handle's stream must have been drained (Tracer.cube(), cube_doppler(fetch=True))."""
        import torch
        torch.cuda.synchronize()
        h = self.buf.cpu().numpy()
        want = np.full(self.plane, SENT, np.complex128).view(np.uint64)
        assert np.array_equal(h[:self.plane].view(np.uint64), want), "the plane BEFORE the cube was written"
        assert np.array_equal(h[-self.plane:].view(np.uint64), want), "the plane AFTER the cube was written"
        return h[self.plane:-self.plane].reshape(self.shape).copy()


# ----------------------------------------------------------------------------- planting
def solve_t0(tau, d_want, dt):
    """t0 with (tau - t0) / dt == d_want in float64 when d_want is an integer (a search over neighbouring doubles), and the
    nearest double to tau - d_want dt otherwise (the caller asserts what it needs of the resulting d)"""
    t0 = float(np.float64(tau) - np.float64(d_want) * np.float64(dt))
    if d_want != math.floor(d_want):
        return t0
    up = down = t0
    for _ in range(64):
        for cand in (up, down):
            if R.start_of(tau, cand, dt) == d_want:
                return cand
        up, down = float(np.nextafter(up, math.inf)), float(np.nextafter(down, -math.inf))
    raise AssertionError("no t0 puts tau = %r on grid point %r" % (tau, d_want))


def planted_start(tau, D, phi, dt=DT):
    """(t0, d): the cube origin that starts the contribution at D + phi, with the property asserted on the float64 d"""
    t0 = solve_t0(tau, D + phi, dt)
    d = R.start_of(tau, t0, dt)
    assert math.floor(d) == D, (d, D)
    assert (d == D) if phi == 0 else (0.0 < d - D < 1.0), (d, D, phi)
    return t0, d


def support(L, M):
    """(q0, reach): a start with floor(d) = D and a fractional part touches output samples D + q0 .. D + reach (header: h_L is
    non-zero on |u| < L/2; L = 1: sample m lands in floor(d) + m)"""
    q0 = 0 if L == 1 else 1 - L // 2
    return q0, q0 + (L - 1) + (M - 1)


def picks_of(rec):
    """a few rays to plant, alternating receivers, first and last of each receiver's rays"""
    out = []
    for rx in sorted(set(int(r) for r in rec["received"])):
        idx = np.flatnonzero(rec["received"] == rx)
        out += [int(idx[0]), int(idx[-1]), int(idx[len(idx) // 2])]
    return out[0::3] + out[1::3] + out[2::3]


def masked(rec, live):
    """the received records with power / Doppler as rts_finalise_values sets them: live = {index: (power, doppler)}, all others 0"""
    out = rec.copy(); out["power"] = 0.0; out["doppler"] = 0.0
    for i, (p, f) in live.items():
        out["power"][i] = p; out["doppler"][i] = f
    return out


def all_live(rec, seed):
    rng = np.random.default_rng(seed)
    out = rec.copy()
    out["power"] = rng.uniform(0.5, 2.0, len(rec)); out["doppler"] = rng.uniform(-0.2, 0.2, len(rec))
    return out


def finalise(tr, vals):
    tr.finalise_values(vals["power"], vals["doppler"])


def wave_of(rts, M, L, seed=0):
    rng = np.random.default_rng(1000 * L + M + seed)
    return rts.Waveform(rng.standard_normal(M) + 1j * rng.standard_normal(M), L)


class Base:
    def __init__(self, rts, spec, motion=None):
        self.spec = spec; self.n_rx = len(spec["rx"])
        self.tr = H.gpu_tracer(rts, spec)
        H.gpu_trace(rts, spec, tr=self.tr, motion=motion)
        self.rec = self.tr.received()["results"]
        self.picks = picks_of(self.rec)


@pytest.fixture(scope="module")
def base(rts):
    from rts_amd import scenes
    b = Base(rts, scenes.config_multi(W=20))
    assert b.n_rx == 2 and len(b.rec) >= 50 and set(int(r) for r in b.rec["received"]) == {0, 1}
    yield b
    b.tr.close()


@pytest.fixture(scope="module")
def grouped(rts):
    """the same pulse with every ray live and aggregated: the contributions of RTS_RENDER_PATHS / rts_cube_accumulate_paths"""
    from rts_amd import scenes
    b = Base(rts, scenes.config_multi(W=20))
    finalise(b.tr, all_live(b.rec, 77))
    b.tr.aggregate(CS, FC)
    v = b.tr.aggregated_view()
    b.contribs = R.contribs_paths(b.rec["received"], v["power"], v["doppler"], v["delay"], v["phase"], v["pathMatch"])
    assert len(b.contribs) >= 2 and {c[0] for c in b.contribs} == {0, 1}      # at least one group per receiver
    yield b
    b.tr.close()


def render_single(rts, base, w, n_bins, D, phi, pick, expect):
    """one planted ray starting at D + phi, rendered with and without the Doppler term into guarded cubes; expect: the output
    samples of its row that must be hit (a list, asserted on the reference), "zero" (nothing may be written) or None"""
    tr, rec = base.tr, base.rec
    s, L = w.samples, w.taps
    tau = float(rec["rayLength"][pick]) / CS
    t0, d = planted_start(tau, D, phi)
    vals = masked(rec, {pick: (P0, F0)})
    rx = int(rec["received"][pick])
    finalise(tr, vals)
    ref = R.render_ref_pair((base.n_rx, PULSES, n_bins), ROW, R.contribs_rays(vals, CS, FC), s, L, t0, DT)
    what = "L=%d n_bins=%d D=%d phi=%g rx=%d" % (L, n_bins, D, phi, rx)
    for dop in (False, True):
        want = R.to_double(ref[dop])
        hit = np.flatnonzero(want[rx, ROW])
        if expect == "zero":
            assert len(hit) == 0, what
        elif expect is not None:
            assert list(hit) == list(expect), (what, hit)
        g = Guarded(base.n_rx, PULSES, n_bins)
        tr.cube_attach(base.n_rx, PULSES, n_bins, t0, DT, device_ptr=g.ptr)
        tr.cube_render(ROW, "rays", CS, FC, doppler=dop)
        tr.cube()
        got = g.read()
        live = np.zeros(got.shape, bool); live[rx, ROW, :] = True
        assert not got[~live].any(), what                                   # other receivers, other rows: exactly 0
        assert np.array_equal(got != 0, want != 0), what                      # the same cells, sample for sample
        if expect != "zero":
            check_render(got, ref[dop], what + " doppler=%d" % dop)
    if F0 and expect != "zero" and phi != 0 and len(hit) > 1:
        assert not np.allclose(R.to_double(ref[True]), R.to_double(ref[False]), rtol=1e-6, atol=0)      # the Doppler term is visible


M_EDGE = 40
TAPS = [1, 2, 16, 64]


# ----------------------------------------------------------------------------- render: first sample, last sample
@pytest.mark.parametrize("L", TAPS)
def test_render_first_sample_edge(rts, base, L):
    w = wave_of(rts, M_EDGE, L); base.tr.cube_set_waveform(w)
    q0, reach = support(L, M_EDGE)
    nb = 64
    cases = [(-reach, 0.375, [0]),                    # the support's last sample is the cube's sample 0
             (-reach - 1, 0.375, "zero"),             # ... is sample -1: nothing is written
             (-1, 0.625, None),                       # d in (-1, 0): floor and truncation differ
             (-7, 0.0, list(range(0, M_EDGE - 7))),   # an exact negative integer: samples 7 .. M - 1 land in 0 .. M - 8
             (-M_EDGE, 0.0, "zero")]                  # on grid, the last sample in -1
    for k, (D, phi, expect) in enumerate(cases):
        render_single(rts, base, w, nb, D, phi, base.picks[(k + L) % len(base.picks)], expect)


@pytest.mark.parametrize("L", TAPS)
def test_render_far_edge(rts, base, L):
    w = wave_of(rts, M_EDGE, L); base.tr.cube_set_waveform(w)
    q0, reach = support(L, M_EDGE)
    nb = 64
    cases = [(nb - 1 - q0, 0.375, [nb - 1]),          # the support's first sample is the cube's last
             (nb - q0, 0.375, "zero"),                # ... is n_bins: nothing is written
             (nb - 1, 0.0, [nb - 1]),                 # on grid: sample 0 in the last cell
             (nb, 0.0, "zero"),
             (nb - 10, 0.5, None)]                    # runs past the end
    for k, (D, phi, expect) in enumerate(cases):
        render_single(rts, base, w, nb, D, phi, base.picks[(k + L + 1) % len(base.picks)], expect)


# ----------------------------------------------------------------------------- render: the 128-sample tile seam, small cubes
@pytest.mark.parametrize("L", TAPS)
def test_render_tile_seam(rts, base, L):
    w = wave_of(rts, M_EDGE, L); base.tr.cube_set_waveform(w)
    q0, reach = support(L, M_EDGE)
    k = 0
    for nb in (129, 256, 300):
        width = reach - q0 + 1
        cases = [(127 - reach, 0.375, list(range(128 - width, 128))),                       # ends at sample 127
                 (128 - q0, 0.375, list(range(128, min(128 + width, nb)))),                 # starts at sample 128
                 (128 - q0 - width // 2, 0.375, list(range(128 - width // 2, min(128 - width // 2 + width, nb))))]      # straddles 127 / 128
        for D, phi, expect in cases:
            render_single(rts, base, w, nb, D, phi, base.picks[(k + L) % len(base.picks)], expect)
            k += 1


@pytest.mark.parametrize("L", TAPS)
def test_render_cubes_smaller_than_a_tile_and_than_the_waveform(rts, base, L):
    w = wave_of(rts, M_EDGE, L); base.tr.cube_set_waveform(w)
    q0, reach = support(L, M_EDGE)
    k = 0
    for nb in (1, 37):
        for D, phi, expect in [(-q0 - 3, 0.375, list(range(nb))), (-2, 0.0, list(range(min(nb, M_EDGE - 2)))), (nb - 1 - q0, 0.25, [nb - 1]),
                               (-reach, 0.75, [0]), (nb - q0, 0.25, "zero")]:
            render_single(rts, base, w, nb, D, phi, base.picks[(k + L) % len(base.picks)], expect)
            k += 1


# ----------------------------------------------------------------------------- render: on-grid L = 16 == L = 1, bytes
def test_on_grid_windowed_sinc_gives_the_bytes_of_sample_and_hold(rts, base):
    """an on-grid start feeds exactly one unit weight (h_L(0) = 1, h_L = 0 at the other integers) into the same arithmetic"""
    tr, rec = base.tr, base.rec
    nb, D = 64, 5
    s = wave_of(rts, M_EDGE, 1).samples
    for pick in base.picks[:2]:
        tau = float(rec["rayLength"][pick]) / CS
        t0, d = planted_start(tau, D, 0.0)
        vals = masked(rec, {pick: (P0, F0)}); finalise(tr, vals)
        ref = R.render_ref_pair((base.n_rx, PULSES, nb), ROW, R.contribs_rays(vals, CS, FC), s, 1, t0, DT)
        for dop in (False, True):
            got = {}
            for L in (16, 1):
                g = Guarded(base.n_rx, PULSES, nb)
                tr.cube_set_waveform(rts.Waveform(s, L))
                tr.cube_attach(base.n_rx, PULSES, nb, t0, DT, device_ptr=g.ptr)
                tr.cube_render(ROW, "rays", CS, FC, doppler=dop)
                tr.cube(); got[L] = g.read()
            assert np.count_nonzero(got[1]) == M_EDGE
            assert np.array_equal(got[16].view(np.uint64), got[1].view(np.uint64))
            check_render(got[16], ref[dop], "on grid, L=16 against the L=1 reference, doppler=%d" % dop)


# ----------------------------------------------------------------------------- render: the size limit
def plan_size_limit(rec, n_bins, M, L, count=64):
    """(t0, dt, indices): `count` rays, every receiver among them, spread by delay so that the first ones start well before sample 0
    and the last ones run past the end"""
    q0, reach = support(L, M)
    order = np.argsort(rec["rayLength"], kind="stable")
    chosen = order[np.unique(np.linspace(0, len(order) - 1, count).astype(int))]
    lo, hi = float(rec["rayLength"][chosen[0]]), float(rec["rayLength"][chosen[-1]])
    dt = (hi - lo) / CS / (n_bins + 2600.0)                  # first start near -3000, last near n_bins - 400
    t0 = lo / CS + 3000.0 * dt
    D = np.array([math.floor(R.start_of(float(rec["rayLength"][i]) / CS, t0, dt)) for i in chosen])
    assert set(int(r) for r in rec["received"][chosen]) == set(int(r) for r in rec["received"])
    assert np.sum(D + q0 < 0) >= 3 and np.sum((D + reach >= 0) & (D + q0 < 0)) >= 1           # start before the cube, reach into it
    assert np.sum(D + reach >= n_bins) >= 3 and np.sum((D + q0 < n_bins) & (D + reach >= n_bins)) >= 1      # run past its end
    return t0, dt, [int(i) for i in chosen]


def test_render_at_the_size_limit(rts, base):
    """M = 4096 samples and L = 64 taps: 64 KiB + 16 KiB of dynamic LDS, the first launch above 64 KiB in this kernel"""
    tr, rec = base.tr, base.rec
    M, L, nb = 4096, 64, 4500
    w = wave_of(rts, M, L); tr.cube_set_waveform(w)
    t0, dt, chosen = plan_size_limit(rec, nb, M, L)
    assert len(chosen) <= 64
    rng = np.random.default_rng(4096)
    span = (M + nb) * dt
    vals = masked(rec, {i: (rng.uniform(0.5, 2.0), rng.uniform(-3.0, 3.0) / span) for i in chosen})      # up to 3 cycles over the record
    finalise(tr, vals)
    t = time.time()
    ref = R.render_ref_pair((base.n_rx, PULSES, nb), ROW, R.contribs_rays(vals, CS, FC), w.samples, L, t0, dt)
    print("[cube edges] size-limit reference: %.1f s" % (time.time() - t))
    for dop in (False, True):
        g = Guarded(base.n_rx, PULSES, nb)
        tr.cube_attach(base.n_rx, PULSES, nb, t0, dt, device_ptr=g.ptr)
        tr.cube_render(ROW, "rays", CS, FC, doppler=dop)
        tr.cube(); got = g.read()
        want = R.to_double(ref[dop])
        assert np.count_nonzero(want[:, ROW]) > 2000 and not got[:, 0].any() and not got[:, 2].any()
        check_render(got, ref[dop], "M=4096 L=64 n_bins=4500, %d planted, doppler=%d" % (len(chosen), dop))
    assert not np.allclose(R.to_double(ref[True]), R.to_double(ref[False]), rtol=1e-6, atol=0)


# ----------------------------------------------------------------------------- render: a dense received set
def plan_dense(rec, n_bins, M, L, tile=128, sub=32):
    """(t0, dt, rx): the receiver with the most rays and a cube origin for which every ray's support reaches every tile of
    the cube; asserts that the set spans several 128-record chunks and that every FULL chunk holds more than `sub` rays of that
    receiver (each of them kept for every tile: more than one weight batch per chunk)"""
    q0, reach = support(L, M)
    counts = np.bincount(rec["received"])
    rx = int(np.argmax(counts))
    assert counts[rx] >= 400, counts
    lo, hi = float(rec["rayLength"].min()), float(rec["rayLength"].max())
    d_lo, d_hi = (n_bins - tile) - reach, (tile - 1) - q0    # a start D reaches the last tile from D + reach >= n_bins - 128 and the first up to D + q0 <= 127
    assert d_hi - d_lo > 64
    dt = (hi - lo) / CS / (d_hi - d_lo - 16.0)
    t0 = lo / CS - (d_lo + 8.0) * dt
    D = np.array([math.floor(R.start_of(float(l) / CS, t0, dt)) for l in rec["rayLength"]])
    n_tiles = (n_bins + tile - 1) // tile
    for k in range(n_tiles):
        first, last = k * tile, min(k * tile + tile, n_bins) - 1
        assert np.all((D + q0 <= last) & (D + reach >= first)), k   # every ray contributes to every tile
    chunks = [rec["received"][c:c + tile] for c in range(0, len(rec), tile)]
    assert len(chunks) >= 4
    full = [c for c in chunks if len(c) == tile]
    assert len(full) >= 4 and all(np.sum(c == rx) > sub for c in full), [int(np.sum(c == rx)) for c in chunks]
    return t0, dt, rx


def test_render_dense_set(rts):
    """more than RTS_RENDER_SUB = 32 kept contributions per (receiver, tile) in every full chunk of a set that spans many chunks"""
    from rts_amd import scenes
    b = Base(rts, scenes.config_multi(W=40))
    tr, rec = b.tr, b.rec
    M, L, nb = 512, 8, 256
    t0, dt, rx = plan_dense(rec, nb, M, L)
    w = wave_of(rts, M, L); tr.cube_set_waveform(w)
    vals = all_live(rec, 40); finalise(tr, vals)
    t = time.time()
    ref = R.render_ref_pair((b.n_rx, PULSES, nb), ROW, R.contribs_rays(vals, CS, FC), w.samples, L, t0, dt)
    print("[cube edges] dense reference: %d rays, %.1f s" % (len(rec), time.time() - t))
    for dop in (False, True):
        g = Guarded(b.n_rx, PULSES, nb)
        tr.cube_attach(b.n_rx, PULSES, nb, t0, dt, device_ptr=g.ptr)
        tr.cube_render(ROW, "rays", CS, FC, doppler=dop)
        tr.cube(); got = g.read()
        assert not got[:, 0].any() and not got[:, 2].any() and np.count_nonzero(got[rx, ROW]) == nb
        check_render(got, ref[dop], "dense: %d rays, M=512 L=8, doppler=%d" % (len(rec), dop))
    tr.close()


# ----------------------------------------------------------------------------- cubes narrower / wider than the scene
@pytest.mark.parametrize("n_rx", [1, 3])
def test_cube_with_fewer_and_more_receivers_than_the_scene(rts, base, grouped, n_rx):
    """n_rx = 1 of 2: the rays of receiver 1 vanish (its plane would be the guard plane); n_rx = 3: the extra plane stays 0"""
    nb = 160
    lo, hi = float(base.rec["rayLength"].min()), float(base.rec["rayLength"].max())
    dt = (hi - lo) / (nb - 8.0); t0 = lo - 4.0 * dt
    w = wave_of(rts, 24, 8)
    vals = all_live(base.rec, 5)
    contribs = R.contribs_rays(vals, CS, FC)
    assert {c[0] for c in contribs} == {0, 1}
    # render, rays
    tr = base.tr
    finalise(tr, vals); tr.cube_set_waveform(w)
    ref = R.render_ref_pair((n_rx, PULSES, nb), ROW, contribs, w.samples, w.taps, t0, dt)
    for dop in (False, True):
        g = Guarded(n_rx, PULSES, nb)
        tr.cube_attach(n_rx, PULSES, nb, t0, dt, device_ptr=g.ptr); tr.cube_render(ROW, "rays", CS, FC, doppler=dop)
        tr.cube(); got = g.read()
        assert np.count_nonzero(got[0, ROW]) > 20 and not got[:, 0].any() and not got[:, 2].any() and not got[2:].any()
        check_render(got, ref[dop], "render, cube of %d receivers, doppler=%d" % (n_rx, dop))
    # impulse cube, rays
    g = Guarded(n_rx, PULSES, nb)
    tr.cube_attach(n_rx, PULSES, nb, t0, dt, device_ptr=g.ptr); tr.cube_accumulate(ROW, CS, FC)
    tr.cube(); got = g.read()
    want = R.accumulate_ref(np.zeros((n_rx, PULSES, nb), R.CLD), ROW, contribs, t0, dt)
    assert np.array_equal(got != 0, R.to_double(want) != 0) and got[0].any() and not got[2:].any()
    check_impulse(got, want, "accumulate, cube of %d receivers" % n_rx)
    # the same per unique path
    tp = grouped.tr
    tp.cube_set_waveform(w)
    refp = R.render_ref_pair((n_rx, PULSES, nb), ROW, grouped.contribs, w.samples, w.taps, t0, dt)
    for dop in (False, True):
        g = Guarded(n_rx, PULSES, nb)
        tp.cube_attach(n_rx, PULSES, nb, t0, dt, device_ptr=g.ptr); tp.cube_render(ROW, "paths", doppler=dop)
        tp.cube(); got = g.read()
        assert got[0, ROW].any() and not got[:, 0].any() and not got[:, 2].any() and not got[2:].any()
        check_render(got, refp[dop], "render paths, cube of %d receivers, doppler=%d" % (n_rx, dop))
    g = Guarded(n_rx, PULSES, nb)
    tp.cube_attach(n_rx, PULSES, nb, t0, dt, device_ptr=g.ptr); tp.cube_accumulate_paths(ROW)
    tp.cube(); got = g.read()
    want = R.accumulate_ref(np.zeros((n_rx, PULSES, nb), R.CLD), ROW, grouped.contribs, t0, dt)
    assert np.array_equal(got != 0, R.to_double(want) != 0) and got[0].any() and not got[2:].any()
    check_impulse(got, want, "accumulate_paths, cube of %d receivers" % n_rx)


# ----------------------------------------------------------------------------- two handles, one cube
def test_two_handles_render_into_the_same_rows(rts, base):
    """two handles with their own streams render different pulses into the SAME rows of one caller cube: the atomic adds sum"""
    from rts_amd import scenes
    spec = base.spec
    mo = [dict(position=tuple(np.add(m["position"], (0.5, 0, 0))), velocity=m["velocity"]) for m in spec["motion"]]
    other = Base(rts, spec, motion=mo)
    assert not np.array_equal(other.rec["rayLength"][:20], base.rec["rayLength"][:20])
    nb = 224
    lo, hi = float(base.rec["rayLength"].min()), float(base.rec["rayLength"].max())
    dt = (hi - lo) / (nb - 40.0); t0 = lo - 20.0 * dt
    w = wave_of(rts, 64, 16)
    va, vb = all_live(base.rec, 1), all_live(other.rec, 2)
    contribs = R.contribs_rays(va, CS, FC) + R.contribs_rays(vb, CS, FC)
    ref = R.render_ref_pair((base.n_rx, PULSES, nb), ROW, contribs, w.samples, w.taps, t0, dt)
    for dop in (False, True):
        g = Guarded(base.n_rx, PULSES, nb)
        for b, v in ((base, va), (other, vb)):
            finalise(b.tr, v); b.tr.cube_set_waveform(w); b.tr.cube_attach(base.n_rx, PULSES, nb, t0, dt, device_ptr=g.ptr)
        base.tr.cube_render(ROW, "rays", CS, FC, doppler=dop); other.tr.cube_render(ROW, "rays", CS, FC, doppler=dop)      # both enqueued, then both drained
        base.tr.cube(); other.tr.cube()
        got = g.read()
        assert np.count_nonzero(got[:, ROW]) > 200 and not got[:, 0].any() and not got[:, 2].any()
        check_render(got, ref[dop], "two handles, one cube, doppler=%d" % dop)
    other.tr.close()


# ----------------------------------------------------------------------------- render, source paths: far edge and tile seam
@pytest.mark.parametrize("L", [1, 16])
def test_render_paths_far_edge_and_tile_seam(rts, grouped, L):
    tr = grouped.tr
    w = wave_of(rts, M_EDGE, L); tr.cube_set_waveform(w)
    q0, reach = support(L, M_EDGE)
    width = reach - q0 + 1
    cases = [(64, 64 - 1 - q0, 0.375), (64, 64 - q0, 0.375), (64, 64, 0.0), (64, 63, 0.0)]
    for nb in (129, 256, 300):
        cases += [(nb, 127 - reach, 0.375), (nb, 128 - q0, 0.375), (nb, 128 - q0 - width // 2, 0.375)]
    for k, (nb, D, phi) in enumerate(cases):
        rx, a, tau, f = grouped.contribs[k % len(grouped.contribs)]
        t0, d = planted_start(tau, D, phi)
        ref = R.render_ref_pair((grouped.n_rx, PULSES, nb), ROW, grouped.contribs, w.samples, L, t0, DT)
        for dop in (False, True):
            g = Guarded(grouped.n_rx, PULSES, nb)
            tr.cube_attach(grouped.n_rx, PULSES, nb, t0, DT, device_ptr=g.ptr); tr.cube_render(ROW, "paths", doppler=dop)
            tr.cube(); got = g.read()
            want = R.to_double(ref[dop])
            assert not got[:, 0].any() and not got[:, 2].any()
            assert np.array_equal(got != 0, want != 0)
            if want.any():
                check_render(got, ref[dop], "paths L=%d n_bins=%d D=%d phi=%g doppler=%d" % (L, nb, D, phi, dop))


# ----------------------------------------------------------------------------- impulse cube
IMPULSE_CASES = [(-1, 0.625, None), (0, 0.0, 0), (31, 0.625, 31), (32, 0.0, None)]      # (D, phi, the bin that is written) for n_bins = 32


def test_impulse_cube_edges_rays(rts, base):
    """d in (-1, 0) and d = n_bins exactly are dropped; d = 0 exactly and d in (n_bins - 1, n_bins) land in the first and last bin"""
    tr, rec = base.tr, base.rec
    nb = 32
    for k, (D, phi, cell) in enumerate(IMPULSE_CASES):
        pick = base.picks[k % len(base.picks)]
        rx = int(rec["received"][pick])
        t0, d = planted_start(float(rec["rayLength"][pick]) / CS, D, phi)
        vals = masked(rec, {pick: (P0, F0)}); finalise(tr, vals)
        g = Guarded(base.n_rx, PULSES, nb)
        tr.cube_attach(base.n_rx, PULSES, nb, t0, DT, device_ptr=g.ptr); tr.cube_accumulate(ROW, CS, FC)
        tr.cube(); got = g.read()
        want = R.accumulate_ref(np.zeros((base.n_rx, PULSES, nb), R.CLD), ROW, R.contribs_rays(vals, CS, FC), t0, DT)
        hit = np.argwhere(got != 0)
        assert [list(h) for h in hit] == ([] if cell is None else [[rx, ROW, cell]]), (D, phi, hit)
        assert np.array_equal(got != 0, R.to_double(want) != 0)
        if cell is not None:
            assert abs(abs(got[rx, ROW, cell]) - 1.5) < 1e-14
            check_impulse(got, want, "accumulate D=%d phi=%g" % (D, phi))


def test_impulse_cube_edges_paths(rts, grouped):
    tr = grouped.tr
    nb = 32
    for k, (D, phi, cell) in enumerate(IMPULSE_CASES):
        rx, a, tau, f = grouped.contribs[(k + 1) % len(grouped.contribs)]
        t0, d = planted_start(tau, D, phi)
        g = Guarded(grouped.n_rx, PULSES, nb)
        tr.cube_attach(grouped.n_rx, PULSES, nb, t0, DT, device_ptr=g.ptr); tr.cube_accumulate_paths(ROW)
        tr.cube(); got = g.read()
        only = R.to_double(R.accumulate_ref(np.zeros((grouped.n_rx, PULSES, nb), R.CLD), ROW, [(rx, a, tau, f)], t0, DT))
        assert [list(h) for h in np.argwhere(only != 0)] == ([] if cell is None else [[rx, ROW, cell]])      # the planted group alone
        want = R.accumulate_ref(np.zeros((grouped.n_rx, PULSES, nb), R.CLD), ROW, grouped.contribs, t0, DT)
        assert np.array_equal(got != 0, R.to_double(want) != 0), (D, phi)
        if R.to_double(want).any():
            check_impulse(got, want, "accumulate_paths D=%d phi=%g" % (D, phi))


# ----------------------------------------------------------------------------- range compression
@pytest.mark.parametrize("M", [1, 2, 4096])
@pytest.mark.parametrize("nb", [2048, 2049, 4097, 8191])
def test_compress_past_the_pass_boundaries(rts, nb, M):
    """each pass of k_cube_compress covers 2048 outputs: bin counts at and just past one, two and (nearly) four passes"""
    rng = np.random.default_rng(nb + M)
    n_rx, n_p = 2, 3
    data = rng.standard_normal((n_rx, n_p, nb)) + 1j * rng.standard_normal((n_rx, n_p, nb))
    s = rng.standard_normal(M) + 1j * rng.standard_normal(M)
    g = Guarded(n_rx, n_p, nb, fill=data)
    t = rts.Tracer(8, 1); t.cube_attach(n_rx, n_p, nb, 0.0, 1.0, device_ptr=g.ptr); t.cube_set_waveform(rts.Waveform(s, 1))
    t.cube_compress(1, 1)                                   # a sub-range strictly inside the cube
    t.cube(); got = g.read()
    for r in range(n_rx):
        for p in (0, 2):
            assert np.array_equal(got[r, p].view(np.uint64), data[r, p].view(np.uint64))           # rows outside it: byte-identical
        want = R.correlate_ref(data[r, 1], s)
        check("compress", got[r, 1], want, 0, 1e-13 * M * np.abs(data).max() * np.abs(s).max(), "n_bins=%d M=%d rx=%d" % (nb, M, r))      # test_gpu_render.py:279
    t.close()


# ----------------------------------------------------------------------------- slow-time transform
TRANSFORM_CASES = [(2, 2, 65), (2, 1, 7), (4, 4, 9), (4, 1, 1), (4, 3, 65), (32, 32, 7), (32, 1, 65), (32, 17, 9), (64, 64, 65), (64, 1, 9), (64, 33, 1),
                   (128, 128, 9), (128, 1, 7), (128, 65, 65), (256, 256, 1), (256, 1, 65), (256, 129, 7), (2048, 2048, 9), (2048, 1, 65), (2048, 1025, 7)]


@pytest.mark.parametrize("n_fft,n_p,nb", TRANSFORM_CASES)
def test_doppler_transform_sizes(rts, n_fft, n_p, nb):
    """n_pulses == n_fft, n_pulses = 1 and n_pulses = n_fft / 2 + 1 at bin counts that are no multiple of the block's bin tile,
    into a guarded caller buffer"""
    rng = np.random.default_rng(n_fft + n_p + nb)
    n_rx = 2
    data = rng.standard_normal((n_rx, n_p, nb)) + 1j * rng.standard_normal((n_rx, n_p, nb))
    src = Guarded(n_rx, n_p, nb, fill=data); out = Guarded(n_rx, n_fft, nb)
    t = rts.Tracer(8, 1); t.cube_attach(n_rx, n_p, nb, 0.0, 1.0, device_ptr=src.ptr)
    fetched = t.cube_doppler(n_fft, device_ptr=out.ptr)      # (rts_cube_doppler_get drains the handle's stream)
    got = out.read()
    assert np.array_equal(fetched.view(np.uint64), got.view(np.uint64))
    assert np.array_equal(src.read().view(np.uint64), data.view(np.uint64))                          # the cube itself is only read
    check("transform", got, R.dft_ref(data, n_fft), 0, 1e-10 * np.abs(data).max() * math.sqrt(n_fft), "n_fft=%d n_pulses=%d n_bins=%d" % (n_fft, n_p, nb))      # test_gpu_parity.py:570
    t.close()
