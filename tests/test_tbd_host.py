"""Track-before-detect on the host (rts_tbd_step_eval, rts_tbd_extract_eval, rts_amd/csrc/rts_tbd.h): byte for byte against the
independent restatement (tests/tbd_ref.py) on every case the GPU tests run; hand-computed answers on a 1 x 4 x 6 map of small
integers; the shift table; the ring; every refusal, each leaving the outputs untouched; the ABI sizes; the weak target; and the header
alone under the sanitizers (tests/tbd/tbd_main.cpp) on the edge sizes."""
import ctypes as C
import math
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import tbd_ref as R

ROOT = R.ROOT


def chain(rts, c, n_frames=None):
    """the evaluator over the case's frames: per frame (merit, pointers, shifts)"""
    out, merit = [], None
    for n, z in enumerate(c["maps"][:n_frames]):
        merit, code, s = rts.tbd_step_eval(z, merit, c["times"][n] - c["times"][n - 1] if n else 0.0, dt=c["dt"], **c["par"])
        out.append((merit, code, s))
    return out


def extraction(rts, c, frames, threshold, **kw):
    p = c["par"]
    keep = min(len(frames), p["depth"])
    args = dict(local_max=c["local_max"], max_tracks=c["max_tracks"], pri=p["pri"], t0=c["t0"], dt=c["dt"]); args.update(kw)
    return rts.tbd_extract_eval(frames[-1][0], np.stack([f[1] for f in frames[-keep:]]), np.stack([f[2] for f in frames[-keep:]]), threshold, p["half"], p["depth"], **args)


# ----------------------------------------------------------------------------- 1. against the restatement, byte for byte
@pytest.mark.parametrize("name", R.ALL)
def test_evaluators_against_restatement(rts, name):
    c = R.case(name); want = R.run(name)
    frames = chain(rts, c)
    for n, (merit, code, s) in enumerate(frames):
        R.same_bytes(merit, want["merits"][n]); R.same_bytes(code, want["ptrs"][n]); R.same_bytes(s, want["shifts"][n])
    rec, paths = extraction(rts, c, frames, want["threshold"])
    R.same_bytes(rec.view(R.TBD), want["rec"]); R.same_bytes(paths, want["paths"])
    assert want["total"] >= len(rec) and (len(rec) > 0 or name == "never")
    if name != "full_list":
        assert want["total"] == len(rec)
    assert np.all(np.diff((rec["rx"].astype(np.int64) * merit.shape[1] + rec["doppler_bin"]) * merit.shape[2] + rec["range_bin"]) > 0)      # ascending flat order


# ----------------------------------------------------------------------------- 2. hand-computed answers, 1 x 4 x 6
# x = re^2 of the first frame; the second frame is all ones (x = 1).  Window half (1, 1): code = (dd + 1) 3 + (dr + 1).
X0 = np.array([[1, 0, 0, 0, 0, 2],
               [0, 2, 0, 2, 0, 0],
               [0, 0, 0, 0, 0, 0],
               [0, 0, 3, 0, 0, 0]], np.float64)[None]                   # re; x0 = re^2: 1, 4, 9
SMALL = dict(half=(1, 1), depth=4)


def two_frames(rts, second=None, **kw):
    p = dict(SMALL); p.update(kw)
    m0, c0, s0 = rts.tbd_step_eval(X0 + 0j, None, 0.0, **p)
    x0 = X0 * X0 * p.get("scale", 1.0)                                  # (small integers: exact, and so are their roots below)
    x0 = np.sqrt(x0) if p.get("score") == "amplitude" else x0
    assert m0.tolist() == x0.tolist() and np.all(c0 == R.NONE) and np.all(s0 == 0)      # first frame: merit = x, every pointer NONE
    z1 = np.ones((1, 4, 6), np.complex128) if second is None else second
    return rts.tbd_step_eval(z1, m0, 1.0, **p)


def test_known_answers(rts):
    m, c, s = two_frames(rts)
    assert np.all(s == 0)
    # a tie: (1, 2) sees 4 at (dd, dr) = (0, -1) and at (0, +1); the first in ascending (dd, dr) wins: code 1 * 3 + 0
    assert (m[0, 1, 2], c[0, 1, 2]) == (5.0, 3)
    # Doppler wrap at kd = 0: row -1 is row 3, whose 9 lies at dr = 0: code 0 * 3 + 1
    assert (m[0, 0, 2], c[0, 0, 2]) == (10.0, 1)
    # ... and at kd = n_doppler - 1: row 4 is row 0, whose 1 at r = 0 lies at (dd, dr) = (+1, 0): code 2 * 3 + 1; dr = -1 is off the edge
    assert (m[0, 3, 0], c[0, 3, 0]) == (2.0, 7)
    # a window of zeros: nothing is greater than 0, no predecessor
    assert (m[0, 2, 5], c[0, 2, 5]) == (1.0, R.NONE) and (m[0, 1, 5], c[0, 1, 5]) == (5.0, 1)
    # decay 0.5
    m, c, _ = two_frames(rts, decay=0.5)
    assert (m[0, 1, 2], c[0, 1, 2]) == (3.0, 3) and (m[0, 0, 2], c[0, 0, 2]) == (5.5, 1)
    # a NaN and an Inf input cell score 0 and still take their best predecessor
    z = np.ones((1, 4, 6), np.complex128); z[0, 2, 4] = np.nan; z[0, 2, 0] = np.inf
    m, c, _ = two_frames(rts, z)
    assert (m[0, 2, 4], c[0, 2, 4]) == (4.0, 0) and (m[0, 2, 0], c[0, 2, 0]) == (4.0, 2) and np.all(np.isfinite(m))
    # amplitude: x = sqrt(P scale)
    m, c, _ = two_frames(rts, 3.0 * np.ones((1, 4, 6), np.complex128), score="amplitude", scale=4.0)
    assert (m[0, 1, 2], c[0, 1, 2]) == (6.0 + 4.0, 3)                  # sqrt(9 * 4) + sqrt(4 * 4)


def test_predecessors_off_the_range_edge(rts):
    """n_doppler pri = 1, so f = w = 0, 1, -2, -1 and s = 7 w: rows 1 and 2 look 7 below and 14 above a 6-bin map -- merit = score, NONE"""
    m, c, s = two_frames(rts, delay_rate_per_hz=7.0, pri=0.25)
    assert s.tolist() == [0, 7, -14, -7]
    assert np.all(c[0, 1:] == R.NONE) and np.all(m[0, 1:] == 1.0)
    assert (m[0, 0, 2], c[0, 0, 2]) == (10.0, 1)                       # row 0 does not move
    rec, paths = rts.tbd_extract_eval(m, np.stack([np.full((1, 4, 6), R.NONE, np.uint8), c]), np.stack([np.zeros(4, np.int32), s]), 0.5, local_max=False, **SMALL)
    assert len(rec) == 24 and np.all(rec["n_cells"][6:] == 1) and np.all(paths[6:, 1:] == R.ABSENT)
    assert rec[2]["n_cells"] == 2 and paths[2].tolist()[:2] == [[0, 2], [3, 2]] and (rec[2]["first_doppler_bin"], rec[2]["first_range_bin"]) == (3, 2)


def test_shift_table(rts):
    z = np.zeros((1, 8, 4), np.complex128); m0 = np.zeros((1, 8, 4))
    table = lambda **kw: rts.tbd_step_eval(z, m0, kw.pop("T", 1.0), half=(1, 1), **kw)[2].tolist()
    # n_doppler pri = 1: f = w = 0 1 2 3 -4 -3 -2 -1; halves round to even, on both halves of the axis
    assert table(delay_rate_per_hz=0.5, pri=0.125) == [0, 0, 1, 2, -2, -2, -1, 0]
    assert table(delay_rate_per_hz=-0.5, pri=0.125) == [0, 0, -1, -2, 2, 2, 1, 0]
    assert table(delay_rate_per_hz=2.5, pri=0.125) == [0, 2, 5, 8, -10, -8, -5, -2]
    assert table(delay_rate_per_hz=1.0, pri=0.125, T=3.0, dt=2.0) == [0, 2, 3, 4, -6, -4, -3, -2]      # 1.5 -> 2, 4.5 -> 4
    assert table(delay_rate_per_hz=123.0, pri=0.0) == [0] * 8          # no pri: no shift
    assert rts.tbd_step_eval(z, None, math.nan, half=(1, 1), delay_rate_per_hz=5.0, pri=0.125)[2].tolist() == [0] * 8      # first frame: T ignored
    want, _ = R.shifts(8, 0.37, 1e-3, 0.7, 1e-2)
    assert table(delay_rate_per_hz=0.37, pri=1e-3, T=0.7, dt=1e-2) == want.tolist() and len(set(want.tolist())) == 8


def test_ring(rts):
    """frames = depth + 3: the walk goes back exactly depth cells, each through its own frame's table (T differs per frame)"""
    c = R.case("three_receivers"); p = c["par"]
    assert len(c["maps"]) == p["depth"] + 3 and len(set(np.diff(c["times"]).tolist())) > 2
    frames = chain(rts, c)
    assert len({f[2].tobytes() for f in frames[1:]}) > 2                 # the tables differ
    rec, paths = extraction(rts, c, frames, R.run("three_receivers")["threshold"])
    assert len(rec) > 10 and np.all(rec["n_cells"] == p["depth"]) and np.all(paths != R.ABSENT)
    for r, path in zip(rec, paths):                                       # every hop is the pointer's, with the hop's own table
        kd, b = int(r["doppler_bin"]), int(r["range_bin"])
        for j in range(p["depth"]):
            assert path[j].tolist() == [kd, b]
            merit, code, s = frames[len(frames) - 1 - j]
            k = int(code[r["rx"], kd, b])
            if j + 1 < p["depth"]:
                assert k != R.NONE
                kd, b = (kd + k // 5 - 1) % 8, b - int(s[kd]) + k % 5 - 2
        assert (r["first_doppler_bin"], r["first_range_bin"]) == tuple(path[-1])
    # fewer frames than the ring holds: the walk ends at the first frame's NONE
    short = chain(rts, c, 3)
    rec, paths = extraction(rts, c, short, 0.0, local_max=False)
    assert set(rec["n_cells"].tolist()) <= {1, 2, 3} and 3 in rec["n_cells"] and np.all(paths[:, 3:] == R.ABSENT)


def test_one_row_has_no_local_maximum(rts):
    c = R.case("one_row"); frames = chain(rts, c)
    assert len(extraction(rts, c, frames, -1.0, local_max=True)[0]) == 0      # the neighbour (-1, 0) is the cell itself
    assert len(extraction(rts, c, frames, -1.0, local_max=False)[0]) == frames[-1][0].size


# ----------------------------------------------------------------------------- 3. refusals, capacity, ABI
def test_refusals_leave_outputs_untouched(rts):
    L = rts.L
    z = R.noise(np.random.default_rng(1), (1, 4, 6)); prev = np.ones((1, 4, 6))
    q = L.RtsCubeParams(1, 1, 6, 0, 0.0, 1.0)
    merit = np.full((1, 4, 6), 7.0); code = np.full((1, 4, 6), 7, np.uint8); s = np.full(4, 7, np.int32)

    def step(p, T=1.0, qq=q, nd=4, merit_in=prev, zz=z):
        rc = L.lib().rts_tbd_step_eval(C.byref(qq) if qq else None, rts.ptr(zz.view(np.float64)) if zz is not None else None, nd, rts.ptr(merit_in), C.byref(p) if p else None, T,
                                       rts.ptr(merit), rts.ptr(code), rts.ptr(s))
        assert np.all(merit == 7.0) and np.all(code == 7) and np.all(s == 7)
        return rc, L.lib().rts_last_error().decode()
    P = lambda **kw: rts._tbd_params(kw.pop("half", (1, 2)), kw.pop("depth", 8), kw.pop("score", "power"), kw.pop("scale", 1.0), kw.pop("decay", 1.0),
                                     kw.pop("delay_rate_per_hz", 0.0), kw.pop("pri", 0.0))
    for kw, word in ((dict(half=(4, 2)), "half_doppler"), (dict(half=(1, 16)), "half_range"), (dict(half=(2, 2)), "exceeds n_doppler"), (dict(half=(1, 6)), "n_bins"),
                     (dict(depth=0), "depth"), (dict(depth=65), "depth"), (dict(score=2), "score"), (dict(scale=0.0), "scale"), (dict(scale=-1.0), "scale"),
                     (dict(scale=math.inf), "scale"), (dict(scale=math.nan), "scale"), (dict(decay=0.0), "decay"), (dict(decay=1.0000001), "decay"), (dict(decay=math.nan), "decay"),
                     (dict(delay_rate_per_hz=math.nan), "delay_rate_per_hz"), (dict(pri=-1.0), "pri"), (dict(pri=math.inf), "pri")):
        rc, msg = step(P(**kw))
        assert rc == L.RTS_ERR_INVALID and word in msg, (kw, msg)
    for field in ("flags", "reserved0", "reserved"):
        p = P()
        if field == "reserved":
            p.reserved[0] = 1
        else:
            setattr(p, field, 1)
        rc, msg = step(p)
        assert rc == L.RTS_ERR_INVALID and ("flags" if field == "flags" else "reserved") in msg
    for T in (0.0, -1.0, math.inf, math.nan):
        rc, msg = step(P(), T)
        assert rc == L.RTS_ERR_INVALID and "T = " in msg
    rc, msg = step(P(delay_rate_per_hz=2.0 ** 31, pri=0.25))            # f = 1 Hz on row 1: quotient 2^31
    assert rc == L.RTS_ERR_INVALID and "row 1" in msg
    rc, msg = step(P(delay_rate_per_hz=1e308, pri=1e-300))              # overflows: not finite
    assert rc == L.RTS_ERR_INVALID and "row 1" in msg
    assert step(P(delay_rate_per_hz=2.0 ** 32, pri=0.25), T=0.25)[0] == L.RTS_ERR_INVALID       # exactly 2^30 on row 1 is allowed, 2^31 on row 2 is not
    for kw in (dict(p=None), dict(qq=None), dict(nd=0), dict(zz=None), dict(qq=L.RtsCubeParams(1, 1, 6, 0, 0.0, 0.0)), dict(qq=L.RtsCubeParams(0, 1, 6, 0, 0.0, 1.0))):
        kw.setdefault("p", P())
        assert step(**kw)[0] == L.RTS_ERR_INVALID
    rc = L.lib().rts_tbd_step_eval(C.byref(q), rts.ptr(z.view(np.float64)), 4, rts.ptr(prev), C.byref(P()), 1.0, rts.ptr(prev), rts.ptr(code), rts.ptr(s))
    assert rc == L.RTS_ERR_INVALID and np.all(prev == 1.0)               # merit_out must not be merit_in
    # the extraction
    rec = np.full(4, 0x5a, np.uint8).repeat(48).view(L.TBD_TRACK_DTYPE); paths = np.full((4, 8, 2), 0x5a5a5a5a, np.uint32); n = C.c_uint32(99)
    ring = np.full((2, 1, 4, 6), R.NONE, np.uint8); tabs = np.zeros((2, 4), np.int32)

    def ext(e, p=None, n_frames=2):
        rc = L.lib().rts_tbd_extract_eval(C.byref(q), 4, C.byref(p or P()), rts.ptr(prev), rts.ptr(ring), rts.ptr(tabs), n_frames, C.byref(e) if e else None, rts.ptr(rec), rts.ptr(paths), 4, C.byref(n))
        assert rec.tobytes() == b"\x5a" * 192 and np.all(paths == 0x5a5a5a5a) and n.value == 99
        return rc, L.lib().rts_last_error().decode()
    E = rts._tbd_extract_params
    for e, word in ((E(math.nan, True, 0, 0.0), "threshold"), (E(1.0, True, 0, -1.0), "pri"), (E(1.0, True, 0, math.nan), "pri"), (E(1.0, True, 65537, 0.0), "max_tracks")):
        rc, msg = ext(e)
        assert rc == L.RTS_ERR_INVALID and word in msg
    e = E(1.0, True, 0, 0.0); e.flags = 2
    assert ext(e)[0] == L.RTS_ERR_INVALID and "flags" in L.lib().rts_last_error().decode()
    e = E(1.0, True, 0, 0.0); e.reserved[1] = 1
    assert ext(e)[0] == L.RTS_ERR_INVALID and "reserved" in L.lib().rts_last_error().decode()
    assert ext(None)[0] == L.RTS_ERR_INVALID
    assert ext(E(1.0, True, 0, 0.0), n_frames=0)[0] == L.RTS_ERR_INVALID and ext(E(1.0, True, 0, 0.0), n_frames=9)[0] == L.RTS_ERR_INVALID
    assert ext(E(1.0, True, 0, 0.0), P(half=(2, 2)))[0] == L.RTS_ERR_INVALID


def test_capacity_of_the_extraction(rts):
    """capacity or max_tracks below the total: the prefix, nothing beyond it, the total, RTS_ERR_CAPACITY"""
    L = rts.L
    c = R.case("full_list"); want = R.run("full_list"); frames = chain(rts, c)
    p = c["par"]; nd = frames[-1][0].shape[1]
    q = L.RtsCubeParams(1, 1, frames[-1][0].shape[2], 0, 0.0, 1.0)
    ring = np.stack([f[1] for f in frames]); tabs = np.stack([f[2] for f in frames])
    everything, all_paths = extraction(rts, c, frames, want["threshold"], max_tracks=0)
    assert len(everything) == want["total"] == 512
    for capacity, max_tracks, stored in ((16, 10, 10), (4, 10, 4), (4, 0, 4), (0, 0, 0)):
        rec = np.full(16, 0x5a, np.uint8).repeat(48).view(L.TBD_TRACK_DTYPE); paths = np.full((16, 8, 2), 0x5a5a5a5a, np.uint32); n = C.c_uint32(0)
        rc = L.lib().rts_tbd_extract_eval(C.byref(q), nd, C.byref(rts._tbd_params(p["half"], p["depth"], "power", 1.0, 1.0, 0.0, 0.0)), rts.ptr(frames[-1][0]), rts.ptr(ring), rts.ptr(tabs), 3,
                                          C.byref(rts._tbd_extract_params(want["threshold"], False, max_tracks, 0.0)), rts.ptr(rec), rts.ptr(paths), capacity, C.byref(n))
        assert rc == L.RTS_ERR_CAPACITY and n.value == 512
        assert rec[:stored].tobytes() == everything[:stored].tobytes() and paths[:stored].tobytes() == all_paths[:stored].tobytes()
        assert rec[stored:].tobytes() == b"\x5a" * (48 * (16 - stored)) and np.all(paths[stored:] == 0x5a5a5a5a)


def test_abi(rts):
    L = rts.L
    assert (C.sizeof(L.RtsTbdParams), C.sizeof(L.RtsTbdExtractParams), L.TBD_TRACK_DTYPE.itemsize) == (72, 40, 48) and L.TBD_TRACK_DTYPE == R.TBD
    assert (L.RTS_TBD_MAX_HALF_DOPPLER, L.RTS_TBD_MAX_HALF_RANGE, L.RTS_TBD_MAX_DEPTH, L.RTS_TBD_NONE, L.RTS_TBD_MAX_TRACKS) == (3, 15, 64, R.NONE, R.MAX_TRACKS)
    assert (2 * 3 + 1) * (2 * 15 + 1) - 1 == 216 < R.NONE
    text = open(os.path.join(ROOT, "rts_amd", "csrc", "rts_internal.h")).read()
    assert "sizeof(RtsTbdParams) == 72 && sizeof(RtsTbdExtractParams) == 40 && sizeof(RtsTbdTrack) == 48" in text
    tile = int(re.search(r"#define RTS_TBD_TILE (\d+)u", open(os.path.join(ROOT, "rts_amd", "csrc", "rts_tbd.h")).read()).group(1))
    assert tile == L.RTS_TBD_TILE == R.TILE                            # the GPU cases are sized by the kernel's tile
    hdr = open(os.path.join(ROOT, "include", "rts_amd.h")).read()
    for name, value in (("MAX_HALF_DOPPLER", "3u"), ("MAX_HALF_RANGE", "15u"), ("MAX_DEPTH", "64u"), ("NONE", "0xffu")):
        assert re.search(r"#define RTS_TBD_%s %s\b" % (name, value), hdr)


# ----------------------------------------------------------------------------- 4. the weak target
def test_weak_target(rts):
    """a steady target of power 6 (7.8 dB) in unit noise, below the CA level for pfa 1e-6 in most frames, is recovered from 8 frames:
    the largest merit ends within the transition window of the true end cell and its path lies on the truth in at least 7 of 8 cells.
    The restatement alone meets the three conditions for the seed (checked first), then the evaluator"""
    maps, truth = R.weak_target(R.WEAK_SEED)
    c = R.case("weak_target"); ref = R.run("weak_target")
    assert ref["shifts"][-1][R.WEAK_ROW] == R.WEAK_SHIFT
    near, on, crossed = R.weak_outcome(ref["merits"][-1], ref["rec"], ref["paths"], maps, truth)
    assert near and on >= 7 and crossed <= 3, (near, on, crossed)
    frames = chain(rts, c)
    rec, paths = extraction(rts, c, frames, ref["threshold"])
    near, on, crossed = R.weak_outcome(frames[-1][0], rec, paths, maps, truth)
    assert near and on >= 7 and crossed <= 3, (near, on, crossed)
    assert rec["n_cells"][np.argmax(rec["merit"])] == 8


# ----------------------------------------------------------------------------- 5. rts_tbd.h alone, under the sanitizers
@pytest.fixture(scope="module")
def tbd_main(tmp_path_factory):
    gxx = shutil.which("g++")
    if not gxx:
        pytest.skip("no g++")
    rt = subprocess.run([gxx, "-print-file-name=libasan.so"], capture_output=True, text=True).stdout.strip()
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"] if os.path.isabs(rt) and os.path.exists(rt) else []
    exe = str(tmp_path_factory.mktemp("tbd") / "tbd_main")
    subprocess.check_call([gxx, "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-ffp-contract=off"] + san + ["-I", os.path.join(ROOT, "rts_amd", "csrc"),
                           os.path.join(ROOT, "tests", "tbd", "tbd_main.cpp"), "-o", exe])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:verify_asan_link_order=0", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")

    def ask(cases):
        """cases: dict(par, maps, T, dt, t0, threshold, local_max, max_tracks, pri, capacity [, reserved, flags, ext_flags, ext_reserved])
        -> per case dict(codes, total, written, clean, merit, ptrs, shifts, rec, paths)"""
        hx = lambda v: float(v).hex()
        text = []
        for c in cases:
            p = c["par"]; n_rx, nd, nb = c["maps"][0].shape
            text.append("%d %d %d %d %d %d %s %s %s %s %d %d %d %s %s %s %d %s %s %d %d %d %d" % (
                p["half"][0], p["half"][1], p["depth"], {"power": 0, "amplitude": 1}.get(p["score"], p["score"]), c.get("flags", 0), c.get("reserved", 0), hx(p["scale"]), hx(p["decay"]),
                hx(p["delay_rate_per_hz"]), hx(p["pri"]), n_rx, nd, nb, hx(c.get("t0", 0.0)), hx(c.get("dt", 1.0)), hx(c["T"]), len(c["maps"]), hx(c["threshold"]), hx(c.get("pri", 0.0)),
                c.get("ext_flags", 1 if c.get("local_max", True) else 0), c.get("max_tracks", 0), c.get("ext_reserved", 0), c["capacity"]))
            for z in c["maps"]:
                text.append(" ".join(hx(v) for v in np.ascontiguousarray(z, np.complex128).view(np.float64).ravel()))
        r = subprocess.run([exe], input="\n".join(text) + "\n", capture_output=True, text=True, env=env, timeout=120)
        assert r.returncode == 0, r.stderr[-3000:]
        lines = r.stdout.splitlines()
        assert len(lines) == len(cases)
        out = []
        for c, line in zip(cases, lines):
            t = line.split()
            pc, sc, ec, total, written, clean, keep = (int(v) for v in t[:7])
            d = dict(codes=(pc, sc, ec), total=total, written=written, clean=clean, keep=keep)
            if keep:
                shape = c["maps"][0].shape; cells = int(np.prod(shape)); depth = c["par"]["depth"]
                at = 7
                d["merit"] = np.array([float.fromhex(v) for v in t[at:at + cells]]).reshape(shape); at += cells
                d["ptrs"] = np.array(t[at:at + keep * cells], np.int64).astype(np.uint8).reshape((keep,) + shape); at += keep * cells
                d["shifts"] = np.array(t[at:at + keep * shape[1]], np.int64).astype(np.int32).reshape(keep, shape[1]); at += keep * shape[1]
                rec = np.zeros(written, R.TBD)
                for i in range(written):
                    f = t[at:at + 9]; at += 9
                    rec[i] = tuple(int(v) for v in f[:6]) + tuple(float.fromhex(v) for v in f[6:])
                d["rec"] = rec
                d["paths"] = np.array(t[at:at + written * depth * 2], np.int64).astype(np.uint32).reshape(written, depth, 2); at += written * depth * 2
                assert at == len(t)
            out.append(d)
        return out
    return ask


def test_header_alone_reads_and_writes_only_what_it_is_given(rts, tbd_main):
    """maps, merit, pointers, shifts, records and paths are heap arrays of exactly their sizes in the driver; what it writes equals the
    library's byte for byte; the edge sizes: n_doppler = 1 with Hd 0, n_bins = Hr + 1, depth 1, shifts far beyond n_bins"""
    rng = np.random.default_rng(17)
    mk = lambda shape, n: [R.noise(rng, shape) for _ in range(n)]
    base = dict(T=1.0, threshold=0.5, local_max=False, capacity=64)
    cases = [
        dict(base, par=R.par(half=(0, 2)), maps=mk((2, 1, 9), 3)),                                               # one Doppler row
        dict(base, par=R.par(half=(0, 0), depth=1), maps=mk((1, 1, 1), 3)),                                      # one cell, depth 1
        dict(base, par=R.par(half=(1, 15)), maps=mk((1, 3, 16), 3)),                                             # n_bins = Hr + 1, n_doppler = 2 Hd + 1
        dict(base, par=R.par(half=(3, 4), depth=1), maps=mk((1, 7, 5), 4)),                                      # depth 1, n_bins = Hr + 1
        dict(base, par=R.par(half=(1, 2), delay_rate_per_hz=1000.0, pri=0.25), maps=mk((1, 4, 12), 3)),          # shifts of +-1000, +-2000 bins: all predecessors off the map
        dict(base, par=R.par(half=(1, 2), delay_rate_per_hz=2.0 ** 30, pri=0.25), T=0.5, maps=mk((1, 4, 12), 3)),   # ... of 2^29 and 2^30
        dict(base, par=R.par(half=(1, 2), delay_rate_per_hz=5.0, pri=0.25, depth=2), maps=mk((2, 4, 12), 5), local_max=True, threshold=1.0, pri=0.25),
        dict(base, par=R.par(half=(1, 2), score="amplitude", decay=0.25), maps=mk((1, 4, 12), 3), capacity=5, max_tracks=3),
        dict(base, par=R.par(), maps=mk((1, 4, 12), 2), capacity=0),
    ]
    cases[4]["maps"][1][0, 1, 3] = np.nan
    got = tbd_main(cases)
    for c, g in zip(cases, got):
        p = c["par"]
        assert g["codes"] == (0, 0, 0) and g["clean"] == 1
        frames, merit = [], None
        for n, z in enumerate(c["maps"]):
            merit, code, s = rts.tbd_step_eval(z, merit, c["T"], **p)
            frames.append((merit, code, s))
        keep = min(len(frames), p["depth"])
        assert g["keep"] == keep
        R.same_bytes(g["merit"], merit)
        R.same_bytes(g["ptrs"], np.stack([f[1] for f in frames[-keep:]])); R.same_bytes(g["shifts"], np.stack([f[2] for f in frames[-keep:]]))
        rec, paths = rts.tbd_extract_eval(merit, g["ptrs"], g["shifts"], c["threshold"], p["half"], p["depth"], c["local_max"], 0, c.get("pri", 0.0))
        stored = min(len(rec), c["capacity"], c.get("max_tracks") or R.MAX_TRACKS)
        assert g["total"] == len(rec) and g["written"] == stored
        R.same_bytes(g["rec"], rec[:stored].view(R.TBD).copy()); R.same_bytes(g["paths"], paths[:stored].copy())
    assert np.all(got[4]["ptrs"][1:, :, 1:] == R.NONE) and np.all(got[5]["ptrs"][1:, :, 1:] == R.NONE) and got[5]["shifts"][-1].tolist() == [0, 2 ** 29, -2 ** 30, -2 ** 29]
    assert got[0]["total"] > 0 and got[7]["total"] > 5


def test_header_alone_refuses(tbd_main):
    z = [np.ones((1, 4, 6), np.complex128)] * 2
    ok = dict(par=R.par(), maps=z, T=1.0, threshold=1.0, capacity=4)
    cases, want = [], []
    for code, kw in ((1, dict(half=(4, 2))), (2, dict(half=(1, 16))), (3, dict(depth=0)), (3, dict(depth=65)), (4, dict(score=2)), (7, dict(scale=0.0)), (7, dict(scale=math.inf)),
                     (8, dict(decay=0.0)), (8, dict(decay=2.0)), (8, dict(decay=math.nan)), (9, dict(delay_rate_per_hz=math.inf)), (10, dict(pri=-1.0)), (10, dict(pri=math.nan)),
                     (11, dict(half=(2, 2))), (12, dict(half=(1, 6)))):
        cases.append(dict(ok, par=R.par(**kw))); want.append((code, 0, 0))
    cases.append(dict(ok, flags=1)); want.append((5, 0, 0))
    cases.append(dict(ok, reserved=1)); want.append((6, 0, 0))
    for T in (0.0, -1.0, math.inf, math.nan):
        cases.append(dict(ok, T=T)); want.append((0, 2, 0))
    cases.append(dict(ok, par=R.par(delay_rate_per_hz=2.0 ** 31, pri=0.25))); want.append((0, 1, 0))
    cases.append(dict(ok, threshold=math.nan)); want.append((0, 0, 1))
    cases.append(dict(ok, pri=-1.0)); want.append((0, 0, 2))
    cases.append(dict(ok, ext_flags=2)); want.append((0, 0, 3))
    cases.append(dict(ok, max_tracks=65537)); want.append((0, 0, 4))
    cases.append(dict(ok, ext_reserved=1)); want.append((0, 0, 5))
    got = tbd_main(cases)
    for g, w in zip(got, want):
        assert g["codes"] == w and (g["total"], g["written"], g["clean"], g["keep"]) == (0, 0, 1, 0), (g, w)      # refused: nothing evaluated, the output untouched
