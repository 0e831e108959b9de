"""FMCW mode on the device (rts_cube_render_beat, rts_cube_range_transform): the beat render of both contribution sources against
the host evaluator rts_beat_eval fed by the ORACLE's rays and literal aggregation; the part plan (forced to one part and to the
maximum split: bit-identical to itself, equal within the bound to each other); additivity and two handles sharing a cube; the range
transform against rts_range_eval over its sizes, gates and flags, with sentinel cells around a caller-owned output; the same tree
as rts_cube_doppler, bit for bit; the whole chain -- beat render, noise, range transform, a second handle's Doppler map and OS-CFAR
-- on a closing target; and the error / lifetime rules on a live handle.

Tolerance: the project's bound for a kernel against its evaluator, rtol 1e-10 and atol 1e-12 max|ref| (tests/test_gpu_render.py,
tests/test_gpu_stft.py): kernel and evaluator run the same tree (rts_amd/csrc/rts_beat.h, rts_stft.h) and differ only in the two
libraries' sincospi / sincos.  "Bit for bit" is meant literally."""
import ctypes as C
import math

import numpy as np
import pytest

import helpers as H

pytestmark = pytest.mark.gpu
T0, DT, NB = 1.1e-6, 5.0e-9, 200                 # the row spans 1.1 us .. 2.095 us; 200 is not a multiple of the strip (16)
SLOPE = 2.0e13                                   # |S tau| dt = 0.2 at tau = 2 us: below 1/2
T_CUT = 1.9e-6                                   # the oscillator stops inside the row, at sample 160


@pytest.fixture(scope="module")
def scenes():
    from rts_amd import scenes as S
    return S


# ----------------------------------------------------------------------------- the contributions, from the oracle (as tests/test_gpu_render.py)
def contribs_rays(rx_records, cspeed, carrier):
    out = []
    for r in rx_records:
        tau = r["rayLength"] / cspeed
        ph = -math.fmod(tau * 2 * math.pi * carrier, 2 * math.pi)
        out.append((int(r["received"]), math.sqrt(r["power"]) * complex(math.cos(ph), math.sin(ph)), tau, float(r["doppler"])))
    return out


def contribs_paths(lit):
    res, pm = lit["results"], lit["pathMatch"]
    out = []
    for i in range(len(res)):
        if int(pm[i]) != i:
            continue
        ph = float(lit["phase"][i])
        out.append((int(res[i]["received"]), math.sqrt(res[i]["power"]) * complex(math.cos(ph), math.sin(ph)), float(lit["delay"][i]), float(res[i]["doppler"])))
    return out


def zeros_cube(shape):
    """(torch's stream is not the handles': the buffer is finished before a handle writes it, and a handle's work before torch reads it)"""
    import torch
    buf = torch.zeros(shape, dtype=torch.complex128, device="cuda")
    torch.cuda.synchronize()
    return buf


def dev(a):
    import torch
    buf = torch.from_numpy(np.array(a, np.complex128, order="C")).to("cuda")          # (a contiguous copy: torch wants a writable array)
    torch.cuda.synchronize()
    return buf


def host(buf):
    import torch
    torch.cuda.synchronize()
    return buf.cpu().numpy()


def moved(spec, k, step=0.5):
    return [dict(position=tuple(np.add(m["position"], (step * k, 0, 0))), velocity=m["velocity"]) for m in spec["motion"]]


def assert_bound(got, ref, what=""):
    np.testing.assert_allclose(got, ref, rtol=1e-10, atol=1e-12 * np.abs(ref).max(), err_msg=str(what))


# ----------------------------------------------------------------------------- 1. against the evaluator
def test_beat_render_against_the_evaluator(rts, oracle, scenes):
    spec = scenes.config_multi(W=20)
    cs, fc = spec["c"], spec["carrier"]; wl = cs / fc
    n_rx, n_p = len(spec["rx"]), 3
    combos = [(slope, dop) for slope in (SLOPE, -SLOPE) for dop in (False, True)]
    tr = H.gpu_tracer(rts, spec); tp = H.gpu_tracer(rts, spec)
    bufs = {(src, j): zeros_cube((n_rx, n_p, NB)) for src in ("rays", "paths") for j in range(len(combos))}
    want = {key: np.zeros((n_rx, n_p, NB), np.complex128) for key in bufs}
    for k in range(n_p):
        mo = moved(spec, k)
        for t in (tr, tp):
            H.gpu_trace(rts, spec, tr=t, motion=mo)
            t.finalise_uniform(None, wl, 1.0, 1.0, fc, cs)
        tp.aggregate(cs, fc)
        o = H.oracle_trace(oracle, spec, motion=mo)
        rx, rxi, _ = oracle.filter_finalise(o["results"], o["path"], [1.0] * len(spec["meshes"]), wl, 1.0, 1.0, fc, cs)
        lit = oracle.aggregate_literal(rx, rxi, cs, fc, spec["W"] ** 3)
        cr, cp = contribs_rays(rx, cs, fc), contribs_paths(lit)
        for j, (slope, dop) in enumerate(combos):
            for src, t, cb in (("rays", tr, cr), ("paths", tp, cp)):
                t.cube_attach(n_rx, n_p, NB, T0, DT, device_ptr=bufs[(src, j)].data_ptr())
                t.cube_render_beat(k, slope, T_CUT, src, cs, fc, doppler=dop)
                rts.beat_eval(want[(src, j)], k, cb, slope, T_CUT, T0, DT, doppler=dop)
    tr.cube(); tp.cube()                      # (the handles' streams drained: the torch reads below see every render)
    for key, buf in bufs.items():
        got, ref = host(buf), want[key]
        assert np.count_nonzero(ref) > 50, key
        assert np.all(ref[:, :, 160:] == 0) and np.all(got[:, :, 160:] == 0), key          # t >= T
        print(key, "max error %.3g of max |ref| %.3g" % (np.abs(got - ref).max(), np.abs(ref).max()))
        assert_bound(got, ref, key)
    # the slope's sign and the sources are visible (the Doppler term, some hundred Hz over a microsecond, is below the bound here:
    # tests/test_beat_host.py shows it)
    assert not np.allclose(want[("rays", 0)], want[("rays", 2)], rtol=1e-6, atol=0)
    assert not np.allclose(want[("rays", 0)], want[("paths", 0)])
    tr.close(); tp.close()


# ----------------------------------------------------------------------------- 2. parts
def test_parts_are_deterministic_and_agree(rts, scenes, monkeypatch):
    from rts_amd import _lib as L
    spec = scenes.config_multi(W=24)
    cs, fc = spec["c"], spec["carrier"]; wl = cs / fc
    n_rx = len(spec["rx"])
    out = {}
    for parts in ("1", str(L.RTS_BEAT_MAX_PARTS), None):                          # forced to one launch, to the maximum split, the plan's own
        if parts is None:
            monkeypatch.delenv("RTS_BEAT_PARTS", raising=False)
        else:
            monkeypatch.setenv("RTS_BEAT_PARTS", parts)
        tr = H.gpu_tracer(rts, spec)                                               # (the switch is read at rts_create)
        H.gpu_trace(rts, spec, tr=tr); tr.finalise_uniform(None, wl, 1.0, 1.0, fc, cs)
        assert tr.received_count() >= 3 * L.RTS_BEAT_MAX_PARTS                     # three records in every part of the maximum split
        a, b = zeros_cube((n_rx, 2, NB)), zeros_cube((n_rx, 2, NB))
        for buf in (a, b):
            tr.cube_attach(n_rx, 2, NB, T0, DT, device_ptr=buf.data_ptr()); tr.cube_render_beat(1, SLOPE, T_CUT, "rays", cs, fc)
        tr.cube()
        assert np.count_nonzero(host(a)) > 50 and np.array_equal(host(a).view(np.float64), host(b).view(np.float64)), parts
        assert np.count_nonzero(host(a)[:, 0]) == 0
        out[parts] = host(a)
        tr.close()
    assert_bound(out[str(L.RTS_BEAT_MAX_PARTS)], out["1"], "maximum split against one part")
    assert_bound(out[None], out["1"], "the plan's parts against one part")


# ----------------------------------------------------------------------------- 3. additivity, sharing
def test_render_adds_and_handles_share_a_cube(rts, scenes):
    import torch
    spec = scenes.config_multi(W=20)
    cs, fc = spec["c"], spec["carrier"]; wl = cs / fc; tx = spec["tx"]
    n_rx = len(spec["rx"])
    whole = H.gpu_tracer(rts, spec); H.gpu_trace(rts, spec, tr=whole); whole.finalise_uniform(None, wl, 1.0, 1.0, fc, cs)
    zero = zeros_cube((n_rx, 1, NB))
    whole.cube_attach(n_rx, 1, NB, T0, DT, device_ptr=zero.data_ptr()); whole.cube_render_beat(0, -SLOPE, T_CUT, "rays", cs, fc)
    rng = np.random.default_rng(8)
    pre = rng.standard_normal((n_rx, 1, NB)) + 1j * rng.standard_normal((n_rx, 1, NB))
    full = dev(pre)
    whole.cube_attach(n_rx, 1, NB, T0, DT, device_ptr=full.data_ptr()); whole.cube_render_beat(0, -SLOPE, T_CUT, "rays", cs, fc)
    whole.cube()
    ref = host(zero)
    assert np.count_nonzero(ref) > 50
    assert np.array_equal(host(full), pre + ref)                                  # one add per component and sample onto what the row held
    # two handles, disjoint ray shards, one cube
    shared = zeros_cube((n_rx, 1, NB))
    trs = []
    for part in range(2):
        t = H.gpu_tracer(rts, spec); t.cube_attach(n_rx, 1, NB, T0, DT, device_ptr=shared.data_ptr())
        t.trace(tx["origin"], tx["span"], tx["dir"], spec["motion"], interleave=(64, 2, part), want_stats=False)
        t.finalise_uniform(None, wl, 1.0, 1.0, fc, cs)
        assert t.received_count() > 0
        t.cube_render_beat(0, -SLOPE, T_CUT, "rays", cs, fc)
        trs.append(t)
    for t in trs:
        t.cube()
    torch.cuda.synchronize()
    assert_bound(host(shared), ref, "two shards into one cube")
    for t in trs + [whole]:
        t.close()


# ----------------------------------------------------------------------------- 4. range transform against the evaluator
@pytest.fixture(scope="module")
def range_cubes():
    """random cubes [2][5][130] and [2][5][4099], on the host (read-only) and on the device"""
    rng = np.random.default_rng(41)
    out = {}
    for nb in (130, 4099):
        c = rng.standard_normal((2, 5, nb)) + 1j * rng.standard_normal((2, 5, nb))
        c.setflags(write=False)
        out[nb] = (c, dev(c))
    return out


@pytest.mark.parametrize("n_fft", [2, 8, 64, 256, 4096])
def test_range_transform_against_the_evaluator(rts, range_cubes, n_fft):
    import torch
    PAD, SENT = 8, complex(7.25, -3.5)
    first, count, n_rx = 1, 3, 2
    done = 0
    for nb, (cube, dcube) in range_cubes.items():
        tr = rts.Tracer(8, 1); tr.cube_attach(n_rx, 5, nb, 0.0, 1.0, device_ptr=dcube.data_ptr())
        for ns in sorted({1, n_fft - 1, n_fft}):
            for first_bin in (0, 3):
                if first_bin + ns > nb:
                    continue                                                     # (the gate does not fit this cube: the other one takes the size)
                for tapered in (False, True):
                    w = rts.window("hann", ns) + 0.125 if tapered else None
                    full = {rev: rts.range_eval(cube, n_fft, window=w, first=first, count=count, first_bin=first_bin, n_samples=ns, reverse=rev) for rev in (False, True)}
                    for n_out in sorted({1, n_fft // 2, n_fft}):
                        for rev in (False, True):
                            ref = full[rev][:, :, :n_out]
                            buf = torch.full((n_rx * count * n_out + 2 * PAD,), SENT, dtype=torch.complex128, device="cuda")
                            torch.cuda.synchronize()
                            tr.cube_range_transform(n_fft, window=w, first=first, count=count, first_bin=first_bin, n_samples=ns, n_out=n_out, reverse=rev,
                                                    device_ptr=buf.data_ptr() + 16 * PAD)
                            got = host(buf)
                            assert np.all(got[:PAD] == SENT) and np.all(got[-PAD:] == SENT), (nb, ns, first_bin, tapered, n_out, rev)
                            assert_bound(got[PAD:-PAD].reshape(ref.shape), ref, (nb, ns, first_bin, tapered, n_out, rev))
                            done += 1
        # n_samples 0: to the row's end, where that fits the transform; the library-owned output and its getter
        if nb - 3 <= n_fft:
            ref = rts.range_eval(cube, n_fft, first=first, count=count, first_bin=3)
            assert_bound(tr.cube_range_transform(n_fft, first=first, count=count, first_bin=3), ref, (nb, "to the row's end"))
            done += 1
        tr.close()
    assert done >= 48


def test_range_transform_many_rows(rts):
    """more rows than one workgroup takes, the last workgroup partly filled, rows of one workgroup in two receivers"""
    rng = np.random.default_rng(5)
    cube = rng.standard_normal((3, 12, 37)) + 1j * rng.standard_normal((3, 12, 37))
    d = dev(cube)
    tr = rts.Tracer(8, 1); tr.cube_attach(3, 12, 37, 0.0, 1.0, device_ptr=d.data_ptr())
    for n_fft in (64, 512, 2048):                                                # 16, 8 and 2 rows per workgroup
        w = rts.window("hamming", 37)
        got = tr.cube_range_transform(n_fft, window=w, first=1, count=11, reverse=True)
        ref = rts.range_eval(cube, n_fft, window=w, first=1, count=11, reverse=True)
        assert got.shape == (3, 11, n_fft)
        assert_bound(got, ref, n_fft)
        assert np.array_equal(tr.range_map(), got)
    tr.close()


# ----------------------------------------------------------------------------- 5. the Doppler map's tree
@pytest.mark.parametrize("n_fft", [8, 128, 4096])
def test_same_tree_as_the_doppler_map(rts, n_fft):
    rng = np.random.default_rng(n_fft)
    nb = n_fft - 3 if n_fft > 8 else n_fft                                       # (zero padding, and none)
    cube = rng.standard_normal((2, 3, nb)) + 1j * rng.standard_normal((2, 3, nb))
    d = dev(cube); ds = dev(cube.transpose(0, 2, 1))
    out_r = zeros_cube((2, 3, n_fft)); out_d = zeros_cube((2, n_fft, 3))
    tr = rts.Tracer(8, 1); tr.cube_attach(2, 3, nb, 0.0, 1.0, device_ptr=d.data_ptr())
    tr.cube_range_transform(n_fft, n_samples=nb, device_ptr=out_r.data_ptr())
    ts = rts.Tracer(8, 1); ts.cube_attach(2, nb, 3, 0.0, 1.0, device_ptr=ds.data_ptr())
    ts.cube_doppler(n_fft, device_ptr=out_d.data_ptr(), fetch=False)
    tr.cube(); ts.cube()
    a, b = host(out_r), np.ascontiguousarray(host(out_d).transpose(0, 2, 1))
    assert np.count_nonzero(a) == a.size
    assert np.array_equal(a.view(np.float64), b.view(np.float64))
    tr.close(); ts.close()


# ----------------------------------------------------------------------------- 6. the chain
def test_chain_closing_target(rts, oracle, scenes):
    """16 pulses of a sphere closing at 2.5 m/s: beat render (up-chirp), noise 30 dB below the strongest sample, Hann-tapered range
    transform (REVERSE, the lower half of the bins kept), the output attached as a second handle's cube on beat_axis's delay step,
    slow-time DFT, OS-CFAR.  The strongest detection sits within one output bin of the oracle's group delay and within one Doppler
    bin of fc |d tau / d pulse| / pri, positive (closing)."""
    spec = scenes.config_multi(W=16, max_refl=1)
    spec["meshes"], spec["motion"] = spec["meshes"][:1], spec["motion"][:1]          # the sphere alone
    cs, fc = spec["c"], spec["carrier"]; wl = cs / fc
    n_rx, n_p, nb, pri, v = len(spec["rx"]), 16, 256, 1e-3, 2.5
    t0, dt, n_fft, n_out = 1.4e-6, 5.0e-9, 256, 128                                  # sampling starts after the echo has arrived
    duration = 3.0e-6                                                                # ... and ends before the chirp does

    def motion(k):
        return [dict(position=tuple(np.add(m["position"], (-v * pri * k, 0.0, 0.0))), velocity=(-v, 0.0, 0.0)) for m in spec["motion"]]
    tr = H.gpu_tracer(rts, spec); tr.cube_attach(n_rx, n_p, nb, t0, dt)
    for k in range(n_p):
        H.gpu_trace(rts, spec, tr=tr, motion=motion(k))
        tr.finalise_uniform(None, wl, 1.0, 1.0, fc, cs)
        tr.cube_render_beat(k, SLOPE, duration, "rays", cs, fc, doppler=True)
    noise_power = float((np.abs(tr.cube()) ** 2).max()) / 1e3
    assert noise_power > 0
    tr.cube_add_noise(noise_power, 77)
    delays, reverse = rts.beat_axis(SLOPE, n_fft, dt, n_out)
    assert reverse and len(delays) == n_out
    rmap = zeros_cube((n_rx, n_p, n_out))
    tr.cube_range_transform(n_fft, window=rts.window("hann", nb), n_out=n_out, reverse=reverse, device_ptr=rmap.data_ptr())
    tr.cube()                                                                        # (drained: the second handle's stream reads the map)
    t2 = rts.Tracer(8, 1); t2.cube_attach(n_rx, n_p, n_out, 0.0, float(delays[1]), device_ptr=rmap.data_ptr())
    t2.cube_doppler(n_p, fetch=False)
    det = t2.cube_detect_os((2, 2), (8, 4), None, pfa=1e-6, local_max=True, pri=pri)
    tr.close(); t2.close()
    assert len(det) >= 1
    s = det[np.argmax(det["power"])]
    # the oracle's strongest group of that receiver at the first and the last pulse
    tau = []
    for k in (0, n_p - 1):
        o = H.oracle_trace(oracle, spec, motion=motion(k))
        rx, rxi, _ = oracle.filter_finalise(o["results"], o["path"], [1.0], wl, 1.0, 1.0, fc, cs)
        lit = oracle.aggregate_literal(rx, rxi, cs, fc, spec["W"] ** 3)
        reps = [i for i in range(len(rx)) if int(lit["pathMatch"][i]) == i and int(lit["results"][i]["received"]) == int(s["rx"])]
        assert reps
        i = max(reps, key=lambda i: lit["results"][i]["power"])
        tau.append(float(lit["delay"][i]))
    bin_s, dop_bin = float(delays[1]), 1.0 / (n_p * pri)
    want_delay, want_doppler = 0.5 * (tau[0] + tau[1]), fc * abs(tau[1] - tau[0]) / (n_p - 1) / pri
    assert tau[1] < tau[0]                                                           # closing
    coupling = want_doppler / SLOPE                                                  # the apparent delay moves by -f / S
    print("detection: delay %.6e (oracle %.6e, bin %.3e), doppler %.2f (oracle %.2f, bin %.2f), coupling %.3g bins" %
          (s["delay"], want_delay, bin_s, s["doppler"], want_doppler, dop_bin, coupling / bin_s))
    assert coupling < 0.1 * bin_s
    assert abs(s["delay"] - want_delay) <= bin_s, (s, want_delay, bin_s)
    assert s["doppler"] > 0 and abs(s["doppler"] - want_doppler) <= dop_bin, (s, want_doppler, dop_bin)


# ----------------------------------------------------------------------------- 7. errors and lifetime
def test_errors_and_lifetime(rts, scenes):
    from rts_amd import _lib as L
    lib = L.lib()
    spec = scenes.config_multi(W=16)
    cs, fc = spec["c"], spec["carrier"]; wl = cs / fc; tx = spec["tx"]
    n_rx = len(spec["rx"])
    tr = H.gpu_tracer(rts, spec)
    H.gpu_trace(rts, spec, tr=tr); tr.finalise_uniform(None, wl, 1.0, 1.0, fc, cs)
    bp = L.RtsBeatParams(); bp.slope, bp.duration, bp.source, bp.flags = SLOPE, T_CUT, L.RTS_RENDER_RAYS, L.RTS_RENDER_DOPPLER
    rp = L.RtsRangeParams(); rp.first_pulse, rp.n_pulses, rp.n_fft = 0, 2, 256
    out = np.full(2 * n_rx * 2 * 256 + 2, 7.25)
    # no cube
    assert lib.rts_cube_render_beat(tr.h, 0, C.byref(bp), cs, fc) == L.RTS_ERR_INVALID and b"attach" in lib.rts_last_error()
    assert lib.rts_cube_range_transform(tr.h, C.byref(rp), None) == L.RTS_ERR_INVALID and b"attach" in lib.rts_last_error()
    assert lib.rts_cube_range_get(tr.h, out.ctypes.data, out.size) == L.RTS_ERR_INVALID
    tr.cube_attach(n_rx, 2, NB, T0, DT)
    # the render's refusals on a live handle
    assert lib.rts_cube_render_beat(tr.h, 0, None, cs, fc) == L.RTS_ERR_INVALID
    assert lib.rts_cube_render_beat(tr.h, 2, C.byref(bp), cs, fc) == L.RTS_ERR_INVALID and b"pulse_index" in lib.rts_last_error()
    for field, value, word in (("slope", 0.0, b"slope"), ("slope", math.inf, b"slope"), ("duration", 0.0, b"duration"), ("duration", math.nan, b"duration"),
                               ("source", 2, b"source"), ("flags", 2, b"flags")):
        bad = L.RtsBeatParams(); bad.slope, bad.duration, bad.source, bad.flags = SLOPE, T_CUT, L.RTS_RENDER_RAYS, 0
        setattr(bad, field, value)
        assert lib.rts_cube_render_beat(tr.h, 0, C.byref(bad), cs, fc) == L.RTS_ERR_INVALID and word in lib.rts_last_error(), field
    bad = L.RtsBeatParams(); bad.slope, bad.duration = SLOPE, T_CUT; bad.reserved[1] = 1
    assert lib.rts_cube_render_beat(tr.h, 0, C.byref(bad), cs, fc) == L.RTS_ERR_INVALID and b"reserved" in lib.rts_last_error()
    assert lib.rts_cube_render_beat(tr.h, 0, C.byref(bp), 0.0, fc) == L.RTS_ERR_INVALID and b"cspeed" in lib.rts_last_error()
    assert lib.rts_cube_render_beat(tr.h, 0, C.byref(bp), cs, math.nan) == L.RTS_ERR_INVALID and b"carrier" in lib.rts_last_error()
    bp.source = L.RTS_RENDER_PATHS
    assert lib.rts_cube_render_beat(tr.h, 0, C.byref(bp), cs, fc) == L.RTS_ERR_INVALID and b"rts_aggregate" in lib.rts_last_error()
    bp.source = L.RTS_RENDER_RAYS
    with pytest.raises(ValueError):
        tr.cube_render_beat(0, SLOPE, T_CUT, "rays")
    assert np.count_nonzero(tr.cube()) == 0                                   # nothing was written by the refused calls
    # the transform's refusals on a live handle; no library-owned map yet
    assert lib.rts_cube_range_get(tr.h, out.ctypes.data, out.size) == L.RTS_ERR_INVALID and b"range" in lib.rts_last_error()
    caller = zeros_cube((n_rx * 2 * 256 + 1,))
    assert lib.rts_cube_range_transform(tr.h, C.byref(rp), C.c_void_p(caller.data_ptr() + 8)) == L.RTS_ERR_INVALID and b"aligned" in lib.rts_last_error()
    assert lib.rts_cube_range_transform(tr.h, C.byref(rp), C.c_void_p(caller.data_ptr())) == L.RTS_OK
    assert lib.rts_cube_range_get(tr.h, out.ctypes.data, out.size) == L.RTS_ERR_INVALID          # (a caller-owned output is not recorded)
    for field, value, word in (("n_fft", 100, b"n_fft"), ("n_fft", 128, b"n_samples"), ("n_out", 257, b"n_out"), ("n_pulses", 3, b"n_pulses"),
                               ("first_bin", NB, b"first_bin"), ("flags", 2, b"flags"), ("reserved0", 1, b"reserved")):
        bad = L.RtsRangeParams(); bad.first_pulse, bad.n_pulses, bad.n_fft = 0, 2, 256
        setattr(bad, field, value)
        assert lib.rts_cube_range_transform(tr.h, C.byref(bad), None) == L.RTS_ERR_INVALID and word in lib.rts_last_error(), field
    assert lib.rts_cube_range_transform(tr.h, None, None) == L.RTS_ERR_INVALID
    w = np.ones(NB); w[7] = math.inf
    bad = L.RtsRangeParams(); bad.first_pulse, bad.n_pulses, bad.n_fft, bad.window = 0, 2, 256, w.ctypes.data
    assert lib.rts_cube_range_transform(tr.h, C.byref(bad), None) == L.RTS_ERR_INVALID and b"window" in lib.rts_last_error()
    # a render and a library-owned map; capacity; the map ends at rts_cube_attach
    tr.cube_render_beat(1, SLOPE, T_CUT, "rays", cs, fc)
    got = tr.cube_range_transform(256, reverse=True)
    assert got.shape == (n_rx, 2, 256) and np.count_nonzero(got[:, 0]) == 0 and np.count_nonzero(got[:, 1]) > 50
    assert_bound(got, rts.range_eval(tr.cube(), 256, reverse=True))
    assert lib.rts_cube_range_get(tr.h, out.ctypes.data, 2 * n_rx * 2 * 256 - 1) == L.RTS_ERR_CAPACITY
    assert np.all(out == 7.25)
    assert lib.rts_cube_range_get(tr.h, None, out.size) == L.RTS_ERR_INVALID
    assert lib.rts_cube_range_get(tr.h, out.ctypes.data, out.size) == L.RTS_OK and out[-1] == 7.25 and out[-2] == 7.25
    tr.cube_attach(n_rx, 2, NB, T0, DT)
    assert lib.rts_cube_range_get(tr.h, out.ctypes.data, out.size) == L.RTS_ERR_INVALID and b"rts_cube_attach" in lib.rts_last_error()
    tr.close()
    # after a fused pulse end (its chain on the device-side count from the second pulse on): both sources, the same bits as the separate calls
    res = {}
    for mode in ("separate", "fused"):
        t = H.gpu_tracer(rts, spec)
        bufs = {src: zeros_cube((n_rx, 3, NB)) for src in ("rays", "paths")}
        for k in range(3):
            t.trace_begin(tx["origin"], tx["span"], tx["dir"], moved(spec, k))
            if mode == "separate":
                t.trace_end(); t.finalise_uniform(None, wl, 1.0, 1.0, fc, cs); t.aggregate(cs, fc)
            else:
                t.trace_end_uniform(None, wl, 1.0, 1.0, fc, cs, cube_pulse=-1)
            for src in ("rays", "paths"):
                t.cube_attach(n_rx, 3, NB, T0, DT, device_ptr=bufs[src].data_ptr())
                t.cube_render_beat(k, SLOPE, T_CUT, src, cs, fc)
        rmap = t.cube_range_transform(256, window=rts.window("hann", NB), reverse=True)       # (of the paths cube, attached last)
        res[mode] = dict({src: host(buf) for src, buf in bufs.items()}, map=rmap)
        t.close()
    for key in ("rays", "paths", "map"):
        assert np.count_nonzero(res["separate"][key]) > 50
        assert np.array_equal(res["separate"][key], res["fused"][key]), key
    # a closed handle
    for call in (lambda: tr.cube_render_beat(0, SLOPE, T_CUT, "rays", cs, fc), lambda: tr.cube_range_transform(256), lambda: tr.range_map()):
        with pytest.raises(L.RtsError):
            call()
