"""The tracker step on the host (rts_tracks_eval, rts_amd/csrc/rts_track.h): byte for byte against the independent restatement
(tests/track_ref.py: plain Python floats, the serial greedy pass over the sorted edges) on every case the GPU tests run; the known
answers of the small cases; the 40-frame sequence and its expected outcome; every refusal, each leaving the outputs untouched; the
capacity rule; and the header alone under the sanitizers (tests/track/track_main.cpp) on the edge sizes."""
import ctypes as C
import math
import os
import shutil
import subprocess

import numpy as np
import pytest

import track_ref as R

ROOT = R.ROOT
SEED = 0


def evaluate(rts, c):
    p = c["par"]
    return rts.tracks_eval(c["tracks"], c["next_id"], c["T"], c["plots"], **p)


# ----------------------------------------------------------------------------- 1. against the restatement, byte for byte
@pytest.mark.parametrize("name", list(R.CASES))
def test_eval_against_restatement(rts, name):
    got, nid = evaluate(rts, R.case(name))
    want, total, want_id = R.expected(name)
    R.same_bytes(got, want)
    assert nid == want_id


def by_id(rec):
    return {int(r["id"]): r for r in rec}


def test_known_answers(rts):
    ev = lambda name: evaluate(rts, R.case(name))[0]
    g = ev("gate_on")[0]
    assert (g["id"], g["plot_index"], g["d2"], g["hits"]) == (100, 0, 4.0, 2)          # d2 == gate exactly: an edge
    a = ev("gate_above")
    assert a["id"].tolist() == [1000] and a["flags"][0] == R.NEW                       # one ulp above: the track dies, the plot starts one
    t = by_id(ev("tie_two_tracks"))
    assert list(t) == [100] and t[100]["d2"] == 1.0                                    # the lower track index wins, the other is deleted
    t = ev("tie_two_plots")
    assert (t["id"].tolist(), t["plot_index"].tolist()) == ([100, 1000], [0, 1])       # the lower plot index wins, the other starts a track
    t = by_id(ev("abc"))
    assert sorted(t) == [100, 101] and t[100]["plot_index"] == 0 and t[101]["plot_index"] == 1      # A-1, B-2, C gets nothing
    assert abs(t[100]["d2"] - 0.5) < 1e-12 and abs(t[101]["d2"] - 2.0) < 1e-12
    t = ev("chain70")
    assert t["plot_index"].tolist() == list(range(1, 71)) + [0] and t["id"][-1] == 1000
    for name in ("pairs257", "pairs1025"):
        t = ev(name)
        assert np.all(t["hits"] == 2) and len(set(t["plot_index"].tolist())) == len(t)
    for name, n in (("truncate19_k1", 19), ("truncate19_k16", 19), ("truncate130_k1", 130), ("truncate130_k16", 130)):
        t = ev(name)
        assert 100 not in by_id(t)                                                     # its kept edges were all taken; the next one was dropped
        assert t["plot_index"][:16].tolist() == list(range(16)) and t["plot_index"][16:].tolist() == list(range(16, n))
        assert np.all(t["flags"][16:] == R.NEW)                                         # plot 16, gated by track 0, starts a track instead
    t = ev("receivers")
    assert t["id"].tolist() == [103, 1000, 1001, 1002] and t["rx"].tolist() == [3, 0, 1, 5]
    t = ev("nonfinite")
    assert t["id"].tolist() == [100, 102] and t["plot_index"].tolist() == [1, 5]


def test_wrap_reaches_across_the_edge(rts):
    w, _ = evaluate(rts, R.case("wrap_k0"))
    n, _ = evaluate(rts, R.case("nowrap_k0"))
    assert w["id"].tolist() == [100, 101, 102, 103, 1000] and np.all(w["hits"][:4] == 2)
    assert np.all(w["doppler"] >= -500.0) and np.all(w["doppler"] < 500.0)
    assert w["doppler"][0] > 498.0 and w["doppler"][1] < -499.0                        # pulled towards the plot THROUGH the edge
    assert w["doppler"][2] < 0.0 and w["doppler"][4] == -300.0                         # 499.9 went over the edge; 1700 Hz starts at -300
    assert n["id"].tolist() == [103, 1000, 1001, 1002, 1003] and n["doppler"][4] == 1700.0
    k, _ = evaluate(rts, R.case("wrap_k"))
    assert np.all(k["hits"][:4] == 2) and k["p_df"][0] != 0.0 and w["p_df"][0] == 0.0   # the coupling shows in the covariance


def test_lifecycle(rts):
    t, nid = evaluate(rts, R.case("lifecycle"))
    base = (1 << 40) + 5
    assert t["id"].tolist() == [100, 102, 104, 105, 106, base, base + 1] and nid == base + 2
    assert t["flags"].tolist() == [0, R.CONFIRMED, R.CONFIRMED, R.COASTED, R.CONFIRMED | R.COASTED, R.NEW, R.NEW]
    assert t["hits"].tolist() == [2, 3, 8, 1, 3, 1, 1] and t["misses"].tolist() == [0, 0, 0, 1, 2, 0, 0] and t["age"].tolist() == [2, 2, 2, 2, 2, 1, 1]
    assert t["plot_index"].tolist() == [1, 3, 2, R.NONE, R.NONE, 0, 4]
    assert t["power_sum"].tolist() == [2.0, 4.0, 3.0, 0.0, 0.0, 1.0, 5.0]


def test_full_table(rts):
    for name, ids, next_id in (("full4", [100, 101, 103, 7], 8), ("full5", [100, 101, 103, 7, 8], 9), ("full4_survivors", [100, 101, 102, 103], 7)):
        t, nid = evaluate(rts, R.case(name))
        assert t["id"].tolist() == ids and nid == next_id      # only stored tracks consume ids
        assert R.expected(name)[1] == 6                        # what a table without end would hold


def test_sequence_holds_its_outcome(rts):
    """four targets, missed frames, five false plots per frame: exactly the four confirmed, each with one id, from frame 2 on"""
    tab, nid, tables = np.zeros(0, R.TRACK), 0, []
    ref_tab, ref_id = tab, 0
    for z in R.sequence(SEED):
        tab, nid = rts.tracks_eval(tab, nid, R.SEQ_T, z, **R.SEQ_PAR)
        ref_tab, _, ref_id = R.step(R.SEQ_PAR, ref_tab, ref_id, R.SEQ_T, z)
        R.same_bytes(tab, ref_tab)
        assert nid == ref_id
        tables.append(tab)
    R.check_sequence(tables)


# ----------------------------------------------------------------------------- 2. refusals and the capacity rule
def params(rts, **kw):
    p = rts._track_params(9.21, (1.0, 1.0), 0.0, 0.0, 0.0, 3, 3, 0, 16)
    for k, v in kw.items():
        if k == "reserved":
            p.reserved[v] = 1
        else:
            setattr(p, k, v)
    return p


def raw_eval(rts, p, tracks, plots, out, capacity, T=1.0, null=()):
    n, nid = C.c_uint32(77), C.c_uint64(88)
    rc = rts.L.lib().rts_tracks_eval(C.byref(p) if p is not None else None, None if "in" in null else rts.ptr(tracks), len(tracks), 5, T,
                                     None if "plots" in null else rts.ptr(plots), len(plots), None if "out" in null else rts.ptr(out), capacity,
                                     None if "n" in null else C.byref(n), None if "id" in null else C.byref(nid))
    return rc, n.value, nid.value


REFUSED = [("gate", dict(gate=0.0)), ("gate", dict(gate=-1.0)), ("gate", dict(gate=math.inf)), ("gate", dict(gate=math.nan)),
           ("sigma_delay", dict(sigma_delay=0.0)), ("sigma_delay", dict(sigma_delay=math.nan)), ("sigma_doppler", dict(sigma_doppler=-2.0)),
           ("sigma_doppler", dict(sigma_doppler=math.inf)), ("q =", dict(q=-1e-9)), ("q =", dict(q=math.inf)), ("delay_rate_per_hz", dict(delay_rate_per_hz=math.nan)),
           ("doppler_period", dict(doppler_period=-1.0)), ("doppler_period", dict(doppler_period=math.inf)), ("confirm_hits", dict(confirm_hits=0)),
           ("max_candidates", dict(max_candidates=0)), ("max_candidates", dict(max_candidates=17)), ("max_tracks", dict(max_tracks=65537)),
           ("reserved", dict(reserved=0)), ("reserved", dict(reserved=1)), ("without device_plots", dict(n_plots=3)),
           ("RTS_TRACK_MAX_PLOTS", dict(device_plots=4096, n_plots=(1 << 24) + 1)), ("8-byte", dict(device_plots=4100))]


@pytest.mark.parametrize("field,kw", REFUSED)
def test_refused_parameters(rts, field, kw):
    c = R.case("lifecycle")
    out = np.full(16, 0x5a, np.uint8).repeat(88).view(R.TRACK); before = out.tobytes()
    rc, n, nid = raw_eval(rts, params(rts, **kw), c["tracks"], c["plots"], out, len(out))
    assert rc == rts.L.RTS_ERR_INVALID and field in rts.L.lib().rts_last_error().decode() and out.tobytes() == before and (n, nid) == (77, 88)


def test_refused_lists_and_arguments(rts):
    L = rts.L
    c = R.case("lifecycle")
    tracks, plots = c["tracks"], c["plots"]
    out = np.full(16, 0x5a, np.uint8).repeat(88).view(R.TRACK); before = out.tobytes()

    def refused(word, p=None, t=tracks, z=plots, **kw):
        rc, n, nid = raw_eval(rts, params(rts) if p is None else p, np.ascontiguousarray(t), np.ascontiguousarray(z), out, len(out), **kw)
        assert rc == L.RTS_ERR_INVALID and word in L.lib().rts_last_error().decode() and out.tobytes() == before and (n, nid) == (77, 88), word

    down = R.make_plots([(1, 0.0, 0.0), (0, 1.0, 0.0)])
    refused("rx must not decrease", z=down)
    for T in (0.0, -1.0, math.inf, math.nan):
        refused("T =", T=T)
    for field, v in (("delay", math.nan), ("doppler", math.inf), ("p_dd", -1.0), ("p_ff", -0.5), ("p_df", math.nan)):
        bad = tracks.copy(); bad[field][3] = v
        refused("tracks[3]", t=bad)
    bad = tracks.copy(); bad["flags"][2] = 8
    refused("unknown flags", t=bad)
    refused("max_tracks", p=params(rts, max_tracks=6))                     # 7 tracks in a table of 6
    for null in ("in", "plots", "out", "n", "id"):
        refused("null", null=(null,))
    assert raw_eval(rts, None, tracks, plots, out, len(out))[0] == L.RTS_ERR_INVALID and out.tobytes() == before
    # no tracks: T is not looked at; empty sides may be NULL
    rc, n, nid = raw_eval(rts, params(rts), tracks[:0].copy(), plots, out, len(out), T=math.nan, null=("in",))
    assert (rc, n, nid) == (L.RTS_OK, 5, 10)
    rc, n, nid = raw_eval(rts, params(rts), tracks[:0].copy(), plots[:0].copy(), None, 0, null=("in", "plots", "out"))
    assert (rc, n, nid) == (L.RTS_OK, 0, 5)


def test_capacity(rts):
    L = rts.L
    c = R.case("lifecycle")
    full, _ = evaluate(rts, c)
    p = params(rts, max_misses=2, tentative_misses=1)
    out = np.full(8, 0x5a, np.uint8).repeat(88).view(R.TRACK); tail = out[6:].tobytes()
    rc, n, nid = raw_eval(rts, p, c["tracks"], c["plots"], out, 6)
    assert rc == L.RTS_ERR_CAPACITY and n == 7 and nid == 7 and "6 of 7" in L.lib().rts_last_error().decode()      # ids: by what the table stores
    want = full.copy(); want["id"][5:] = [5, 6]
    R.same_bytes(out[:6].copy(), want[:6])
    assert out[6:].tobytes() == tail
    rc, n, nid = raw_eval(rts, p, c["tracks"], c["plots"], None, 0, null=("out",))
    assert (rc, n, nid) == (L.RTS_ERR_CAPACITY, 7, 7)


def test_abi_sizes(rts):
    L = rts.L
    assert L.TRACK_DTYPE.itemsize == 88 == R.TRACK.itemsize and C.sizeof(L.RtsTrackParams) == 96 and L.TRACK_DTYPE == R.TRACK
    assert (L.RTS_TRACK_MAX_CAND, L.RTS_TRACK_MAX_TRACKS, L.RTS_TRACK_DEFAULT_TRACKS) == (16, 65536, R.DEFAULT_TRACKS)
    assert (L.RTS_TRACK_CONFIRMED, L.RTS_TRACK_COASTED, L.RTS_TRACK_NEW) == (R.CONFIRMED, R.COASTED, R.NEW)
    text = open(os.path.join(ROOT, "rts_amd", "csrc", "rts_internal.h")).read()
    assert "sizeof(RtsTrack) == 88 && sizeof(RtsTrackParams) == 96" in text


# ----------------------------------------------------------------------------- 3. rts_track.h alone, under the sanitizers
@pytest.fixture(scope="module")
def track_main(tmp_path_factory):
    gxx = shutil.which("g++")
    if not gxx:
        pytest.skip("no g++")
    rt = subprocess.run([gxx, "-print-file-name=libasan.so"], capture_output=True, text=True).stdout.strip()
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"] if os.path.isabs(rt) and os.path.exists(rt) else []
    exe = str(tmp_path_factory.mktemp("track") / "track_main")
    subprocess.check_call([gxx, "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-ffp-contract=off"] + san + ["-I", os.path.join(ROOT, "rts_amd", "csrc"),
                           os.path.join(ROOT, "tests", "track", "track_main.cpp"), "-o", exe])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:verify_asan_link_order=0", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")

    def ask(cases):
        """cases: (par, tracks, next_id, T, plots, capacity) -> per case (params code, interval ok, table code, plots code, total,
        next id, output untouched beyond what was written, TRACK records written)"""
        hx = lambda v: float(v).hex()
        text = []
        for p, tracks, next_id, T, plots, capacity in cases:
            text.append("%s %s %s %s %s %s %d %d %d %d %d %d %d %s %d %d %d" % (
                hx(p["gate"]), hx(p["sigma"][0]), hx(p["sigma"][1]), hx(p["q"]), hx(p["delay_rate_per_hz"]), hx(p["doppler_period"]), p["confirm_hits"], p["max_misses"],
                p["tentative_misses"], p["max_candidates"], p["max_tracks"], p.get("reserved", 0), next_id, hx(T), capacity, len(tracks), len(plots)))
            text.extend("%d %d %d %d %d %d %d %s %s %s %s %s" % (t["id"], t["rx"], t["flags"], t["hits"], t["misses"], t["age"], t["plot_index"], hx(t["delay"]), hx(t["doppler"]),
                                                              hx(t["p_dd"]), hx(t["p_df"]), hx(t["p_ff"])) for t in tracks)
            text.extend("%d %s %s %s" % (z["rx"], hx(z["delay"]), hx(z["doppler"]), hx(z["power_sum"])) for z in plots)
        r = subprocess.run([exe], input="\n".join(text) + "\n", capture_output=True, text=True, env=env, timeout=120)
        assert r.returncode == 0, r.stderr[-3000:]
        lines = r.stdout.splitlines()
        assert len(lines) == len(cases)
        out = []
        for line in lines:
            t = line.split()
            rec = np.zeros((len(t) - 7) // 14, R.TRACK)
            for i in range(len(rec)):
                f = t[7 + 14 * i: 21 + 14 * i]
                rec[i] = tuple(int(x) for x in f[:7]) + tuple(float.fromhex(x) for x in f[7:])
            out.append(tuple(int(x) for x in t[:7]) + (rec,))
        return out
    return ask


MAIN_CASES = ["empty_empty", "no_tracks", "no_plots", "gate_on", "gate_above", "tie_two_tracks", "tie_two_plots", "abc", "chain70", "pairs257", "truncate19_k1",
              "truncate130_k16", "wrap_k", "nowrap_k0", "receivers", "nonfinite", "lifecycle", "full4", "full5", "full4_survivors", "random_grid"]


def test_header_alone_reads_and_writes_only_what_it_is_given(rts, track_main):
    """tables, lists and outputs are heap arrays of exactly their sizes in the driver; the records equal the library's byte for byte;
    a capacity below the total writes the prefix and nothing more"""
    cases = []
    for name in MAIN_CASES:
        c = R.case(name)
        cases.append((c["par"], c["tracks"], c["next_id"], c["T"], c["plots"], len(c["tracks"]) + len(c["plots"])))
    c = R.case("lifecycle")
    cases.append((c["par"], c["tracks"], c["next_id"], c["T"], c["plots"], 3))
    cases.append((c["par"], c["tracks"], c["next_id"], c["T"], c["plots"], 0))
    got = track_main(cases)
    for name, (pc, ok, tc, zc, total, nid, clean, rec) in zip(MAIN_CASES, got):
        want, want_total, want_id = R.expected(name)
        assert (pc, ok, tc, zc, total, nid, clean) == (0, 1, 0, 0, want_total, want_id, 1), name
        R.same_bytes(rec, want)
    full, full_total, full_id = R.expected("lifecycle")
    assert got[-2][4:7] == (full_total, full_id, 1) and got[-1][4:7] == (full_total, full_id, 1) and len(got[-1][7]) == 0
    R.same_bytes(got[-2][7], full[:3].copy())


def test_header_alone_refuses(track_main):
    c = R.case("lifecycle")
    ok = (c["par"], c["tracks"], c["next_id"], c["T"], c["plots"], 16)
    cases, want = [], []
    for code, kw in ((1, dict(gate=0.0)), (1, dict(gate=math.nan)), (2, dict(sigma=(0.0, 1.0))), (3, dict(sigma=(1.0, math.inf))), (4, dict(q=-1.0)),
                     (5, dict(delay_rate_per_hz=math.inf)), (6, dict(doppler_period=-1.0)), (7, dict(confirm_hits=0)), (8, dict(max_candidates=0)),
                     (8, dict(max_candidates=17)), (9, dict(max_tracks=65537)), (10, dict(reserved=1))):
        cases.append((R.par(**kw),) + ok[1:]); want.append((code, 1, 0, 0))
    cases.append(ok[:3] + (0.0,) + ok[4:]); want.append((0, 0, 0, 0))
    bad = c["tracks"].copy(); bad["p_dd"][4] = -1.0
    cases.append(ok[:1] + (bad,) + ok[2:]); want.append((0, 1, 1, 0))
    bad = c["tracks"].copy(); bad["flags"][1] = 16
    cases.append(ok[:1] + (bad,) + ok[2:]); want.append((0, 1, 2, 0))
    cases.append(ok[:4] + (R.make_plots([(2, 0.0, 0.0), (1, 0.0, 0.0)]),) + ok[5:]); want.append((0, 1, 0, 1))
    got = track_main(cases)
    for g, w in zip(got, want):
        assert g[:4] == w and g[4:7] == (0, 0, 1) and len(g[7]) == 0, (g[:7], w)      # refused: nothing evaluated, the output untouched
