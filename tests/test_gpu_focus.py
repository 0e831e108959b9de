"""Autofocus on the device (rts_cube_align, rts_cube_pga, rts_cube_correct) against the host evaluators (themselves checked against
a numpy restatement in tests/test_focus_host.py), on caller-owned device cubes: the alignment bit for bit, the correction to the
image's tolerance (rtol 1e-10, atol 1e-12 max|ref|: the same interpolator and rotation, the libraries' sincospi, cos and sinpi a few
ulp apart), the PGA to 10 times the evaluator's measured distance from numpy (tests/test_focus_host.py: EVAL_VS_NUMPY) -- the device
differs from the evaluator only in the twiddles, sincospi and atan2, the restatement in the whole transform.  Guarded caller-owned
outputs, the library-owned tables, the chain end to end on a synthetic scene and behind the real trace -> render -> compress chain,
and the error cases."""
import ctypes as C

import numpy as np
import pytest

import helpers as H
import focus_ref as F
import test_focus_host as TH

pytestmark = pytest.mark.gpu

PGA_DEVICE_BOUND = 10 * TH.EVAL_VS_NUMPY


def to_device(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def restore(buf, a):
    """the device tensor <- the host array, finished before the handle's stream (the library's own, which torch's stream is not
    ordered with) is given work on it"""
    import torch
    buf.copy_(torch.from_numpy(np.ascontiguousarray(a)).reshape(buf.shape))
    torch.cuda.synchronize()


def attach(rts, cube, t=None):
    """a handle with the host cube attached as a caller-owned device tensor: (tracer, the tensor)"""
    buf = to_device(cube)
    t = t or rts.Tracer(8, 1)
    t.cube_attach(cube.shape[0], cube.shape[1], cube.shape[2], 0.0, 1.0, device_ptr=buf.data_ptr())
    return t, buf


def assert_close(got, ref, what=""):
    err = float(np.abs(got - ref).max())
    print("%s: max |device - evaluator| %.3g, max |evaluator| %.3g" % (what, err, np.abs(ref).max()))
    np.testing.assert_allclose(got, ref, rtol=1e-10, atol=1e-12 * np.abs(ref).max(), err_msg=str(what))


# ----------------------------------------------------------------------------- G1: alignment, bit for bit
@pytest.mark.parametrize("P", [1, 2, 63, 64, 65, 130])
def test_align_bit_equal(rts, P):
    """every gate length at every offset with every max_lag; the receivers, the flag and the iteration count go round their eight
    combinations over those sixty shapes"""
    nb, first = 140, 3
    cubes = {n_rx: TH.align_cube(40 + P + n_rx, n_rx, P + 4, nb) for n_rx in (1, 3)}
    t = rts.Tracer(8, 1)
    bufs = {}
    i, moved = 0, 0.0
    for G in (1, 63, 64, 65, 130):
        for fb in (0, 5, nb - G):
            for L in (0, 1, 9, 64):
                n_rx, integer, iters = (1, 3)[i & 1], bool(i & 2), (1, 3)[(i >> 2) & 1]
                i += 1
                _, bufs[n_rx] = attach(rts, cubes[n_rx], t)
                got = t.cube_align(first, P, (fb, G), L, iters, integer)
                ref = rts.align_eval(cubes[n_rx], first, P, (fb, G), L, iters, integer)
                assert got.shape == (n_rx, P) and np.array_equal(got.view(np.uint64), ref.view(np.uint64)), (P, G, fb, L, n_rx, integer, iters)
                moved = max(moved, float(np.abs(ref).max()))
    assert i == 60 and (P == 1 or moved > 0)
    t.close()


# ----------------------------------------------------------------------------- G2: the correction
def correct_tables(n_rx, P, nb, seed):
    rng = np.random.default_rng(seed)
    sh = rng.uniform(-3, 3, (n_rx, P)); ph = rng.uniform(-3, 3, (n_rx, P))
    special = (0.0, 2.0, -3.0, 0.5, -0.5, float(nb + 20), -float(nb + 20), nb - 0.5, 0.5 - nb)
    k = min(P, len(special))
    sh[0, :k] = special[:k]
    ph[0, :min(P, 3)] = (0.0, 1.0, -2.25)[:min(P, 3)]
    return sh, ph


@pytest.mark.parametrize("taps", [1, 2, 8])
def test_correct_against_evaluator(rts, taps):
    n_rx, rows, nb, first, P = 3, 14, 300, 2, 10            # 300 bins: two workgroups per row
    rng = np.random.default_rng(50 + taps)
    cube = rng.standard_normal((n_rx, rows, nb)) + 1j * rng.standard_normal((n_rx, rows, nb))
    sh, ph = correct_tables(n_rx, P, nb, 60 + taps)
    t, buf = attach(rts, cube)
    for s, p in ((sh, ph), (sh, None), (None, ph)):
        restore(buf, cube)
        t.cube_correct(s, p, first, P, taps)
        got = t.cube()
        ref = rts.correct_eval(cube, s, p, first, P, taps)
        assert_close(got, ref, (taps, s is not None, p is not None))
        assert np.array_equal(got[:, :first], cube[:, :first]) and np.array_equal(got[:, first + P:], cube[:, first + P:])      # rows outside the range
        if s is not None:
            assert np.array_equal(got[0, first + 1, :nb - 2], ref[0, first + 1, :nb - 2]) and np.all(got[0, first + 5] == 0) and np.all(got[0, first + 6] == 0)
        if p is None:
            assert np.array_equal(got[0, first], cube[0, first])                                   # S == 0: bit for bit
            assert np.array_equal(got[0, first + 1, :nb - 2], cube[0, first + 1, 2:])                # an integer shift copies
        if s is None:
            assert np.array_equal(got[0, first], cube[0, first]) and np.array_equal(got[0, first + 1], cube[0, first + 1])      # phi 0 and 1
    t.close()


def test_correct_from_the_handles_tables(rts):
    """RTS_CORRECT_USE_ALIGN / RTS_CORRECT_USE_PGA: what the device applies is its own table, which the getters return"""
    sc = F.scene((64, 96), (5.0, 2.0), 1)
    raw = np.concatenate([sc["raw"], np.conj(sc["raw"])[:, ::-1]], axis=0)          # two receivers
    pad = np.zeros((2, 70, 96), np.complex128); pad[:, 3:67] = raw; pad[:, :3] = 1.5 - 0.5j; pad[:, 67:] = -2.0 + 1j
    t, buf = attach(rts, pad)
    S = t.cube_align(3, 64, None, 8, 4)
    assert np.array_equal(S, rts.align_eval(pad, 3, 64, None, 8, 4))
    t.cube_correct(first=3, count=64, taps=8, use_align=True)
    aligned = t.cube()
    ref = rts.correct_eval(pad, S, None, 3, 64, 8)
    assert_close(aligned, ref, "use_align")
    assert np.array_equal(aligned[:, :3], pad[:, :3]) and np.array_equal(aligned[:, 67:], pad[:, 67:])
    phase, rms = t.cube_pga(3, 64, None, 6, 0, 8)
    t.cube_correct(first=3, count=64, taps=8, use_pga=True)
    focused = t.cube()
    assert_close(focused, rts.correct_eval(aligned, None, phase, 3, 64, 8), "use_pga")
    # both tables at once on the restored cube: the shift, then the rotation
    restore(buf, pad)
    t.cube_correct(first=3, count=64, taps=8, use_align=True, use_pga=True)
    assert_close(t.cube(), rts.correct_eval(pad, S, phase, 3, 64, 8), "both tables")
    # a host array beside the other table
    restore(buf, pad)
    t.cube_correct(phase=phase, first=3, count=64, taps=8, use_align=True)
    assert_close(t.cube(), rts.correct_eval(pad, S, phase, 3, 64, 8), "table and array")
    t.close()


# ----------------------------------------------------------------------------- G3: the PGA
def run_pga_case(rts, t, i, case):
    N, G, it, n_rx = case
    cube, _ = TH.pga_cube(300 + i, n_rx, N, G)
    ref, ref_rms, m = F.pga_ref(cube, first=1, count=N, gate=(2, G), n_iters=it)
    assert m >= 1 + 1e-6, (case, m)
    want, want_rms = rts.pga_eval(cube, 1, N, (2, G), it)
    _, buf = attach(rts, cube, t)
    got, got_rms = t.cube_pga(1, N, (2, G), it)
    assert np.array_equal(t.cube(), cube)                      # the cube is not changed
    return float(np.abs(got - want).max()), float(np.abs(got_rms - want_rms).max())


@pytest.mark.parametrize("N", [4, 8, 64, 512, 4096])
def test_pga_against_evaluator(rts, N):
    t = rts.Tracer(8, 1)
    worst = 0.0
    for i, case in enumerate(TH.PGA_CASES):
        if case[0] != N:
            continue
        d, d_rms = run_pga_case(rts, t, i, case)
        print("PGA %s: max |device - evaluator| %.3g cycles (rms record %.3g); bound %.3g" % (case, d, d_rms, PGA_DEVICE_BOUND))
        worst = max(worst, d, d_rms)
    assert worst <= PGA_DEVICE_BOUND, (N, worst)
    t.close()


# ----------------------------------------------------------------------------- G4: guarded outputs
def test_guarded_outputs(rts):
    import torch
    sentinel = -7.5e300
    cube = TH.align_cube(7, 3, 70)
    t, buf = attach(rts, cube)
    for P, gate, L in ((1, (0, 1), 0), (65, (5, 130), 9), (70, None, 64)):
        guard = torch.full((3 * P + 2,), sentinel, dtype=torch.float64, device="cuda")
        torch.cuda.synchronize()                               # (torch's fill is on torch's stream, the library's writes on the handle's)
        t.cube_align(70 - P, P, gate, L, 2, device_ptr=guard.data_ptr() + 8)
        t.cube()
        out = guard.cpu().numpy()
        assert out[0] == sentinel and out[-1] == sentinel and not np.any(out[1:-1] == sentinel), P
        assert np.array_equal(out[1:-1].reshape(3, P), rts.align_eval(cube, 70 - P, P, gate, L, 2))
    for i, (N, G, it, n_rx) in enumerate(((4, 1, 1, 1), (64, 9, 3, 3), (512, 17, 2, 2))):
        pc, _ = TH.pga_cube(500 + i, n_rx, N, G)
        _, pbuf = attach(rts, pc, t)
        guard = torch.full((n_rx * (N + it) + 2,), sentinel, dtype=torch.float64, device="cuda")
        torch.cuda.synchronize()                               # (torch's fill is on torch's stream, the library's writes on the handle's)
        t.cube_pga(1, N, (2, G), it, device_ptr=guard.data_ptr() + 8)
        t.cube()
        out = guard.cpu().numpy()
        assert out[0] == sentinel and out[-1] == sentinel and not np.any(out[1:-1] == sentinel), N
        want, want_rms = rts.pga_eval(pc, 1, N, (2, G), it)
        assert np.abs(out[1:1 + n_rx * N].reshape(n_rx, N) - want).max() <= PGA_DEVICE_BOUND
        assert np.abs(out[1 + n_rx * N:-1].reshape(n_rx, it) - want_rms).max() <= PGA_DEVICE_BOUND
    # the correction writes the cube: one element of guard on each side of it
    for nb in (1, 255, 257):
        rng = np.random.default_rng(nb)
        c = rng.standard_normal((2, 5, nb)) + 1j * rng.standard_normal((2, 5, nb))
        guard = torch.full((c.size + 2,), complex(sentinel, 3.25e-300), dtype=torch.complex128, device="cuda")
        torch.cuda.synchronize()                               # (torch's fill is on torch's stream, the library's writes on the handle's)
        restore(guard[1:-1], c)
        t.cube_attach(2, 5, nb, 0.0, 1.0, device_ptr=guard.data_ptr() + 16)
        sh, ph = correct_tables(2, 5, nb, nb)
        for first, P in ((0, 5), (4, 1), (0, 1)):
            t.cube_correct(sh[:, :P], ph[:, :P], first, P, 8)
            c = rts.correct_eval(c, sh[:, :P], ph[:, :P], first, P, 8)
        got = t.cube()
        out = guard.cpu().numpy()
        assert out[0] == complex(sentinel, 3.25e-300) and out[-1] == complex(sentinel, 3.25e-300), nb
        assert_close(got, c, ("guarded correction", nb))
    t.close()


# ----------------------------------------------------------------------------- G5: the library-owned tables
def test_library_owned_tables(rts):
    import torch
    from rts_amd import _lib as L
    lib = L.lib()
    cube = TH.align_cube(9, 2, 70)
    t, buf = attach(rts, cube)
    mine = torch.zeros((2, 64), dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()                               # (torch's fill is on torch's stream, the library's writes on the handle's)
    t.cube_align(3, 64, None, 9, 2, device_ptr=mine.data_ptr())
    with pytest.raises(L.RtsError):
        t.align_shifts()                                       # a caller-owned output is not the handle's table
    with pytest.raises(L.RtsError):
        t.cube_correct(first=3, count=64, use_align=True)
    a = t.cube_align(3, 64, None, 9, 2)
    b = t.cube_align(3, 64, None, 9, 2)
    assert np.array_equal(a.view(np.uint64), b.view(np.uint64)) and np.array_equal(a, mine.cpu().numpy())
    host = np.zeros(128)
    assert lib.rts_cube_align_get(t.h, host.ctypes.data, 127) == L.RTS_ERR_CAPACITY
    assert lib.rts_cube_align_get(t.h, host.ctypes.data, 128) == L.RTS_OK and np.array_equal(host.reshape(2, 64), a)
    assert lib.rts_cube_align_get(t.h, None, 128) == L.RTS_ERR_INVALID
    with pytest.raises(L.RtsError):
        t.cube_correct(first=2, count=64, use_align=True)      # a table of other rows
    with pytest.raises(L.RtsError):
        t.cube_correct(first=3, count=63, use_align=True)
    # two corrections of the same cube give the same bytes
    t.cube_correct(first=3, count=64, use_align=True)
    one = t.cube()
    restore(buf, cube)
    t.cube_correct(first=3, count=64, use_align=True)
    assert np.array_equal(one.view(np.float64), t.cube().view(np.float64))
    # the phase table
    with pytest.raises(L.RtsError):
        t.pga_phase()
    with pytest.raises(L.RtsError):
        t.cube_correct(first=3, count=64, use_pga=True)
    phase, rms = t.cube_pga(3, 64, (40, 40), 3)
    ph = np.zeros(128); rm = np.zeros(6)
    assert lib.rts_cube_pga_get(t.h, ph.ctypes.data, rm.ctypes.data, 127, 6) == L.RTS_ERR_CAPACITY
    assert lib.rts_cube_pga_get(t.h, ph.ctypes.data, rm.ctypes.data, 128, 5) == L.RTS_ERR_CAPACITY
    assert lib.rts_cube_pga_get(t.h, None, None, 128, 6) == L.RTS_ERR_INVALID
    assert lib.rts_cube_pga_get(t.h, ph.ctypes.data, None, 128, 0) == L.RTS_OK and np.array_equal(ph.reshape(2, 64), phase)
    assert lib.rts_cube_pga_get(t.h, None, rm.ctypes.data, 0, 6) == L.RTS_OK and np.array_equal(rm.reshape(2, 3), rms)
    # the Doppler map is not invalidated by a correction; every table ends at rts_cube_attach
    t.cube_doppler(128, fetch=False)
    t.cube_correct(first=3, count=64, use_pga=True)
    assert lib.rts_cube_doppler_get(t.h, np.zeros(2 * 2 * 128 * 140).ctypes.data, 2 * 2 * 128 * 140) == L.RTS_OK
    t.cube_attach(2, 70, 140, 0.0, 1.0, device_ptr=buf.data_ptr())
    for call in (t.align_shifts, t.pga_phase, lambda: t.cube_correct(first=3, count=64, use_align=True), lambda: t.cube_correct(first=3, count=64, use_pga=True)):
        with pytest.raises(L.RtsError):
            call()
    t.close()


# ----------------------------------------------------------------------------- G6: the error cases through the handle
def test_error_cases_on_a_live_handle(rts):
    import torch
    from rts_amd import _lib as L
    lib = L.lib()
    t = rts.Tracer(8, 1)
    sentinel = 1.5
    out = torch.full((64,), sentinel, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()                               # (torch's fill is on torch's stream, the library's writes on the handle's)
    pa = L.RtsAlignParams(); pa.first_pulse, pa.n_pulses, pa.first_bin, pa.n_gate, pa.max_lag, pa.n_iters = 1, 8, 2, 10, 3, 2
    pp = L.RtsPgaParams(); pp.first_pulse, pp.n_pulses, pp.first_bin, pp.n_gate, pp.n_iters = 1, 8, 2, 10, 2
    sh = np.linspace(-1, 1, 16); ph = np.linspace(-2, 2, 16)
    pc = L.RtsCorrectParams(); pc.first_pulse, pc.n_pulses, pc.taps = 1, 8, 8
    pc.shifts = sh.ctypes.data; pc.phase = ph.ctypes.data
    optr = C.c_void_p(out.data_ptr())
    assert lib.rts_cube_align(t.h, C.byref(pa), optr) == L.RTS_ERR_INVALID and b"cube" in lib.rts_last_error()             # no cube attached
    assert lib.rts_cube_pga(t.h, C.byref(pp), optr) == L.RTS_ERR_INVALID and b"cube" in lib.rts_last_error()
    assert lib.rts_cube_correct(t.h, C.byref(pc)) == L.RTS_ERR_INVALID and b"cube" in lib.rts_last_error()
    rng = np.random.default_rng(3)
    cube = rng.standard_normal((2, 12, 16)) + 1j * rng.standard_normal((2, 12, 16))
    _, buf = attach(rts, cube, t)

    def mutated(p, **kw):
        q = type(p)(); C.memmove(C.byref(q), C.byref(p), C.sizeof(p))
        for k, v in kw.items():
            if k.startswith("reserved_"):
                q.reserved[int(k[-1])] = v
            else:
                setattr(q, k, v)
        return q
    for kw, word in ((dict(reserved0=1), b"reserved"), (dict(reserved_1=1), b"reserved"), (dict(flags=2), b"flags"), (dict(n_pulses=0), b"n_pulses"), (dict(first_pulse=5), b"n_pulses"),
                     (dict(first_bin=16), b"first_bin"), (dict(n_gate=15), b"n_gate"), (dict(max_lag=65), b"max_lag"), (dict(n_iters=0), b"n_iters"), (dict(n_iters=9), b"n_iters")):
        assert lib.rts_cube_align(t.h, C.byref(mutated(pa, **kw)), optr) == L.RTS_ERR_INVALID and word in lib.rts_last_error(), kw
    for kw, word in ((dict(reserved0=1), b"reserved"), (dict(reserved_0=1), b"reserved"), (dict(n_pulses=6), b"n_pulses"), (dict(n_pulses=2), b"n_pulses"), (dict(n_pulses=16), b"n_pulses"),
                     (dict(first_pulse=5), b"n_pulses"), (dict(first_bin=16), b"first_bin"), (dict(n_gate=15), b"n_gate"), (dict(n_iters=0), b"n_iters"), (dict(n_iters=17), b"n_iters")):
        assert lib.rts_cube_pga(t.h, C.byref(mutated(pp, **kw)), optr) == L.RTS_ERR_INVALID and word in lib.rts_last_error(), kw
    for kw, word in ((dict(reserved_0=1), b"reserved"), (dict(flags=4), b"flags"), (dict(flags=1), b"USE_ALIGN"), (dict(flags=2), b"USE_PGA"), (dict(n_pulses=0), b"n_pulses"),
                     (dict(first_pulse=5), b"n_pulses"), (dict(taps=3), b"taps"), (dict(shifts=None, phase=None), b"neither"),
                     (dict(flags=1, shifts=None), b"USE_ALIGN"), (dict(flags=2, phase=None), b"USE_PGA")):
        assert lib.rts_cube_correct(t.h, C.byref(mutated(pc, **kw)), ) == L.RTS_ERR_INVALID and word in lib.rts_last_error(), kw
    sh[5] = np.nan
    assert lib.rts_cube_correct(t.h, C.byref(pc)) == L.RTS_ERR_INVALID and b"shifts" in lib.rts_last_error()
    sh[5] = 0.0; ph[15] = np.inf
    assert lib.rts_cube_correct(t.h, C.byref(pc)) == L.RTS_ERR_INVALID and b"phase" in lib.rts_last_error()
    ph[15] = 0.0
    assert lib.rts_cube_align(t.h, None, optr) == L.RTS_ERR_INVALID and lib.rts_cube_pga(t.h, None, optr) == L.RTS_ERR_INVALID and lib.rts_cube_correct(t.h, None) == L.RTS_ERR_INVALID
    assert lib.rts_cube_align(t.h, C.byref(pa), C.c_void_p(out.data_ptr() + 4)) == L.RTS_ERR_INVALID and b"aligned" in lib.rts_last_error()
    assert lib.rts_cube_pga(t.h, C.byref(pp), C.c_void_p(out.data_ptr() + 4)) == L.RTS_ERR_INVALID and b"aligned" in lib.rts_last_error()
    host = np.zeros(64)
    assert lib.rts_cube_align_get(t.h, host.ctypes.data, 64) == L.RTS_ERR_INVALID
    assert lib.rts_cube_pga_get(t.h, host.ctypes.data, None, 64, 0) == L.RTS_ERR_INVALID
    got = t.cube()
    assert np.all(out.cpu().numpy() == sentinel) and np.array_equal(got, cube)       # nothing was written by the refused calls
    # the valid descriptors run
    assert lib.rts_cube_align(t.h, C.byref(pa), optr) == L.RTS_OK and lib.rts_cube_pga(t.h, C.byref(pp), C.c_void_p(out.data_ptr() + 8 * 16)) == L.RTS_OK
    assert lib.rts_cube_correct(t.h, C.byref(pc)) == L.RTS_OK
    t.cube()
    res = out.cpu().numpy()
    assert not np.any(res[:16 + 16 + 4] == sentinel) and np.all(res[36:] == sentinel)
    t.close()


# ----------------------------------------------------------------------------- G7: end to end
def test_autofocus_end_to_end(rts):
    """the first scene of tests/test_focus_host.py on the device: Tracer.cube_autofocus, nothing fetched between its four calls"""
    shape, walk = F.SCENES[0]
    sc = F.scene(shape, walk, 0)
    t, buf = attach(rts, sc["raw"])
    S, phase, rms = t.cube_autofocus(max_lag=8, taps=8, align_iters=4, n_iters=6, window_min=8)
    focused = t.cube()
    assert np.array_equal(S, rts.align_eval(sc["raw"], max_lag=8, n_iters=4))
    aligned = rts.correct_eval(sc["raw"], shifts=S, taps=8)
    es, pr, ca, cr = F.autofocus_metrics(sc, S, phase, focused, aligned)
    print("device: shift error %.3f bin, residual phase %.3f rad rms, contrast x%.2f over aligned, x%.2f over raw; rms record %s" % (es, pr, ca, cr, rms[0]))
    assert es < 0.5 and pr < 0.6 and ca >= 1.5 and cr >= 3.0
    want, want_rms = rts.pga_eval(aligned, n_iters=6, window_min=8)
    print("device phase against the evaluator's on the evaluator's aligned cube: %.3g cycles" % np.abs(phase - want).max())
    t.close()


def test_alignment_behind_the_real_chain(rts):
    """a sphere of 5 m at 1 km seen through a narrow beam around its specular point (tests/test_gpu_image.py: chain_case), traced,
    rendered and compressed over 32 pulses while it recedes 0.6 m per pulse.  The path lengths of one pulse spread over up to 3 m
    (chain_case), so the bin is made 6 m of path (dt = 20 ns): the return is then point-like, half a bin wide before the waveform's
    own width, which is the regime the alignment is for -- at the image test's 1.5 m bins the envelope's shape changes from pulse to
    pulse by as much as the walk.  2 * 0.6 m of path per pulse over c dt = 5.996 m per bin is 0.2001 bin per pulse, 6.2 bins in all.
    The shifts follow that walk to within 0.5 bin after removing the mean (measured: 0.20 bin)."""
    from rts_amd import scenes as S
    spec = S.config2(subdiv=2, W=24, rx_radius=400.0)
    spec["tx"] = dict(spec["tx"], span=(0.0002, 0.0002, 0.1))
    n_p, step = 32, 0.6
    cs, fc = spec["c"], spec["carrier"]; wl = cs / fc
    dt, nb = 2.0e-8, 128
    t0 = (2 * 992.5 - 240.0) / cs
    tr = H.gpu_tracer(rts, spec)
    tr.cube_attach(1, n_p, nb, t0, dt)
    tr.cube_set_waveform(rts.Waveform.lfm(64, 0.5, 8))
    n_recv = []
    for k in range(n_p):
        H.gpu_trace(rts, spec, tr=tr, motion=[dict(position=(-2.4 + step * k, 0.0, 0.0), velocity=(30.0, 0.0, 0.0))])
        tr.finalise_uniform(None, wl, 1.0, 1.0, fc, cs)
        n_recv.append(tr.received_count())
        tr.cube_render(k, "rays", cs, fc)
    assert min(n_recv) >= 20, n_recv
    tr.cube_compress()
    S_dev = tr.cube_align(max_lag=8, n_iters=4)
    cube = tr.cube()
    assert np.array_equal(S_dev, rts.align_eval(cube, max_lag=8, n_iters=4))
    want = 2 * step / (cs * dt) * np.arange(n_p)
    err = (S_dev[0] - want) - (S_dev[0] - want).mean()
    print("walk %.4f bin per pulse; shifts %.2f .. %.2f; largest error after removing the mean %.3f bin" % (2 * step / (cs * dt), S_dev[0].min(), S_dev[0].max(), np.abs(err).max()))
    assert np.abs(err).max() < 0.5
    assert S_dev[0].max() - S_dev[0].min() > 4.0
    tr.close()
