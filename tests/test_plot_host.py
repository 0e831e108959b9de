"""Plot extraction on the host (rts_plots_eval, rts_amd/csrc/rts_plot.h): bit for bit against the independent restatement
(tests/plot_ref.py: a flood fill on a dense mask, the blocked sums written out) on every case the GPU tests run; every refusal, each
leaving the output untouched; the capacity rule; the pass-through of single-cell plots on a list made by cfar_os_eval(..., local_max=True);
known answers whose arithmetic is exact; and the header alone under the sanitizers (tests/plot/plot_main.cpp) on the edge sizes."""
import ctypes as C
import math
import os
import shutil
import subprocess

import numpy as np
import pytest

import plot_ref as R

ROOT = R.ROOT


def evaluate(rts, name, **kw):
    n_rx, nd, nb, _, link, min_cells = R.CASES[name]
    return rts.plots_eval(R.case_list(name), nd, link, min_cells, pri=R.PRI, t0=R.T0, dt=R.DT, n_rx=n_rx, n_bins=nb, **kw)


# ----------------------------------------------------------------------------- 1. against the restatement, bit for bit
@pytest.mark.parametrize("name", list(R.CASES))
def test_eval_against_restatement(rts, name):
    n_rx, nd, nb, _, link, min_cells = R.CASES[name]
    det = R.case_list(name)
    got = evaluate(rts, name)
    want = R.plots(det, n_rx, nd, nb, link, min_cells, R.PRI, R.T0, R.DT)
    R.same_bytes(got, want)
    if name in R.EXPECT_PLOTS:
        assert len(got) == R.EXPECT_PLOTS[name]
    assert np.all(np.diff(got["first_index"].astype(np.int64)) > 0)
    if min_cells == 1:
        assert int(got["n_cells"].sum()) == len(det)


def test_min_cells_keeps_the_survivors_order(rts):
    all_, two, five = (evaluate(rts, n) for n in ("min1", "min2", "min5"))
    assert len(all_) > len(two) > len(five) > 0
    for kept, m in ((two, 2), (five, 5)):
        R.same_bytes(kept, all_[all_["n_cells"] >= m])
    n_rx, nd, nb, _, link, _ = R.CASES["min1"]
    zero = rts.plots_eval(R.case_list("min1"), nd, link, 0, pri=R.PRI, t0=R.T0, dt=R.DT, n_rx=n_rx, n_bins=nb)      # 0 is taken as 1
    R.same_bytes(zero, all_)


def test_shapes_mean_what_they_say(rts):
    w = evaluate(rts, "wrap")
    assert (w["n_cells"].tolist(), w["doppler_lo"].tolist(), w["doppler_span"].tolist()) == ([3, 1], [7, 3], [2, 1])
    assert -4.0 <= w["doppler_centroid"][0] < 4.0 and abs(w["doppler_centroid"][0]) <= 1.0          # between rows 7 (= -1) and 0
    d = evaluate(rts, "dense65536")
    assert (d["n_cells"][0], d["range_min"][0], d["range_max"][0], d["doppler_span"][0]) == (65536, 0, 255, 256)
    assert len(evaluate(rts, "nd2_ld1")) == len(evaluate(rts, "nd2_ld4"))      # two rows: every reach >= 1 names both


# ----------------------------------------------------------------------------- 2. known answers
def block_list(power):
    d = R.make_list([(0, k, r) for k in (3, 4, 5) for r in (6, 7, 8)], 16, 16)
    d["power"] = power
    return d


@pytest.mark.parametrize("e", [-40, 0, 3, 100])
def test_three_by_three_block(rts, e):
    """equal powers 2^e: every product and sum is exact, the centroid is the centre cell, both variances are exactly 2/3"""
    p = rts.plots_eval(block_list(2.0 ** e), 16, n_rx=1, n_bins=16)
    assert len(p) == 1
    p = p[0]
    assert (p["n_cells"], p["first_index"], p["peak_index"]) == (9, 0, 0)
    assert (p["range_min"], p["range_max"], p["doppler_lo"], p["doppler_span"]) == (6, 8, 3, 3)
    assert p["range_centroid"] == 7.0 and p["doppler_centroid"] == 4.0 and p["power_sum"] == 9 * 2.0 ** e
    # S_xx / S = 15 / 9 is the one rounded division (half an ulp of 1.67 = 1.25 ulp of 2/3); minus (S_x / S)^2 = 1 is exact; the root
    # halves that and adds its own half ulp: under 1.2 ulp of sqrt(2/3) in all
    var = np.float64(15 * 2.0 ** e) / np.float64(9 * 2.0 ** e) - np.float64(1.0)
    assert p["range_spread"] == np.sqrt(var) and p["doppler_spread"] == np.sqrt(var)
    want = math.sqrt(2.0 / 3.0)
    assert abs(p["range_spread"] - want) <= 2 * np.finfo(np.float64).eps * want


def test_two_cells_one_and_three(rts):
    d = R.make_list([(0, 2, 4), (0, 2, 5)], 8, 16)
    d["power"] = [1.0, 3.0]
    p = rts.plots_eval(d, 8, t0=0.0, dt=1.0, n_rx=1, n_bins=16)[0]
    assert p["range_centroid"] == 4.75 and p["doppler_centroid"] == 2.0 and p["delay"] == 4.75
    assert p["range_spread"] == math.sqrt(0.75 - 0.75 * 0.75) and p["doppler_spread"] == 0.0
    assert (p["peak_index"], p["peak_power"], p["power_sum"]) == (1, 3.0, 4.0)


def test_zero_powers_sit_at_the_root(rts):
    d = R.make_list([(0, 2, 4), (0, 2, 5), (0, 3, 5)], 8, 16)
    d["power"] = 0.0
    p = rts.plots_eval(d, 8, n_rx=1, n_bins=16)[0]
    assert (p["range_centroid"], p["doppler_centroid"], p["range_spread"], p["doppler_spread"], p["peak_index"]) == (4.0, 2.0, 0.0, 0.0, 0)


def test_equal_peaks_go_to_the_lowest_index(rts):
    d = R.make_list([(0, 2, r) for r in range(4, 10)], 8, 16)
    d["power"] = [1.0, 5.0, 2.0, 5.0, 5.0, 1.0]
    assert rts.plots_eval(d, 8, n_rx=1, n_bins=16)[0]["peak_index"] == 1


# ----------------------------------------------------------------------------- 3. single-cell plots pass a local-maximum list through
def test_single_cells_pass_through(rts):
    rng = np.random.default_rng(3)
    n_rx, nd, nb = 2, 16, 96
    z = (rng.standard_normal((n_rx, nd, nb)) + 1j * rng.standard_normal((n_rx, nd, nb))) * math.sqrt(0.5)
    for rx, k, r, a in [(0, 0, 10, 30.0), (0, 15, 40, 25.0), (1, 7, 0, 40.0), (1, 8, 95, 35.0), (0, 9, 50, 20.0), (0, 9, 52, 22.0)]:
        z[rx, k, r] += a
    det = rts.cfar_os_eval(z, (1, 1), (4, 2), alpha=12.0, local_max=True, pri=R.PRI, t0=R.T0, dt=R.DT)
    assert len(det) >= 6
    p = rts.plots_eval(det, nd, (0, 0), pri=R.PRI, t0=R.T0, dt=R.DT, n_rx=n_rx, n_bins=nb)
    assert len(p) == len(det) and np.array_equal(p["first_index"], np.arange(len(det))) and np.all(p["n_cells"] == 1)
    for a, b in (("delay", "delay"), ("doppler", "doppler"), ("peak_power", "power"), ("power_sum", "power"), ("noise_sum", "noise")):
        assert p[a].tobytes() == det[b].tobytes(), a
    assert np.array_equal(p["range_centroid"], det["range_bin"] + det["range_offset"]) and np.all(p["range_spread"] == 0.0) and np.all(p["doppler_spread"] == 0.0)


# ----------------------------------------------------------------------------- 4. refusals and the capacity rule
def raw_eval(rts, det, nd, p, n_rx, nb, out, capacity, dt=1.0, null_list=False, null_n=False):
    q = rts.L.RtsCubeParams(n_rx, 1, nb, 0, 0.0, dt)
    n = C.c_uint32(77)
    rc = rts.L.lib().rts_plots_eval(C.byref(q), None if null_list else rts.ptr(det), len(det), nd, C.byref(p) if p is not None else None,
                                    rts.ptr(out) if out is not None else None, capacity, None if null_n else C.byref(n))
    return rc, n.value


def params(rts, **kw):
    p = rts.L.RtsPlotParams()
    p.link_range = p.link_doppler = 1
    for k, v in kw.items():
        if k == "reserved":
            p.reserved[v] = 1
        else:
            setattr(p, k, v)
    return p


REFUSED = [("link_range", dict(link_range=5)), ("link_doppler", dict(link_doppler=5)), ("reserved", dict(reserved=0)), ("reserved", dict(reserved=1)),
           ("pri", dict(pri=-1.0)), ("pri", dict(pri=math.inf)), ("pri", dict(pri=math.nan)), ("n_doppler", dict(device_list=4096, n_doppler=0)),
           ("8-byte", dict(device_list=4100, n_doppler=8)), ("without a device_list", dict(n_list=3)), ("without a device_list", dict(n_doppler=8))]


@pytest.mark.parametrize("field,kw", REFUSED)
def test_refused_parameters(rts, field, kw):
    det = R.make_list([(0, 1, 1), (0, 1, 2), (0, 5, 5)], 8, 16)
    out = np.full(4, 0x5a, np.uint8).repeat(104).view(rts.L.PLOT_DTYPE); before = out.tobytes()
    rc, _ = raw_eval(rts, det, 8, params(rts, **kw), 1, 16, out, len(out))
    assert rc == rts.L.RTS_ERR_INVALID and field in rts.L.lib().rts_last_error().decode() and out.tobytes() == before


def test_refused_lists_and_arguments(rts):
    L = rts.L
    good = R.make_list([(0, 1, 1), (0, 1, 2), (0, 5, 5)], 8, 16)
    out = np.full(4, 0x5a, np.uint8).repeat(104).view(L.PLOT_DTYPE); before = out.tobytes()
    swapped = good[[1, 0, 2]]; twice = good[[0, 1, 1]]
    high_r = good.copy(); high_r["range_bin"][2] = 16
    high_k = good.copy(); high_k["doppler_bin"][2] = 8
    high_rx = good.copy(); high_rx["rx"][2] = 1
    for det, word in ((swapped, "order"), (twice, "order"), (high_r, "outside"), (high_k, "outside"), (high_rx, "outside")):
        rc, _ = raw_eval(rts, np.ascontiguousarray(det), 8, params(rts), 1, 16, out, len(out))
        assert rc == L.RTS_ERR_INVALID and word in L.lib().rts_last_error().decode() and out.tobytes() == before
    assert raw_eval(rts, good, 0, params(rts), 1, 16, out, 4)[0] == L.RTS_ERR_INVALID                    # n_doppler = 0
    assert raw_eval(rts, good, 8, None, 1, 16, out, 4)[0] == L.RTS_ERR_INVALID                           # null parameters
    assert raw_eval(rts, good, 8, params(rts), 1, 16, out, 4, null_list=True)[0] == L.RTS_ERR_INVALID
    assert raw_eval(rts, good, 8, params(rts), 1, 16, out, 4, null_n=True)[0] == L.RTS_ERR_INVALID
    assert raw_eval(rts, good, 8, params(rts), 1, 16, None, 4)[0] == L.RTS_ERR_INVALID                   # null out with capacity
    assert raw_eval(rts, good, 8, params(rts), 0, 16, out, 4)[0] == L.RTS_ERR_INVALID                    # bad cube parameters
    assert raw_eval(rts, good, 8, params(rts), 1, 16, out, 4, dt=0.0)[0] == L.RTS_ERR_INVALID
    n = C.c_uint32(0)
    assert L.lib().rts_plots_eval(None, rts.ptr(good), 3, 8, C.byref(params(rts)), rts.ptr(out), 4, C.byref(n)) == L.RTS_ERR_INVALID
    assert out.tobytes() == before
    rc, total = raw_eval(rts, good, 8, params(rts), 1, 16, None, 0)                                      # out may be NULL when capacity is 0
    assert rc == L.RTS_ERR_CAPACITY and total == 2
    empty = good[:0].copy()
    assert raw_eval(rts, empty, 8, params(rts), 1, 16, None, 0, null_list=True) == (L.RTS_OK, 0)


def test_capacity(rts):
    L = rts.L
    n_rx, nd, nb, _, link, _ = R.CASES["min1"]
    det = R.case_list("min1")
    full = rts.plots_eval(det, nd, link, n_rx=n_rx, n_bins=nb)
    p = params(rts)
    out = np.full(6, 0x5a, np.uint8).repeat(104).view(L.PLOT_DTYPE); tail = out[5:].tobytes()
    rc, total = raw_eval(rts, det, nd, p, n_rx, nb, out, 5)
    assert rc == L.RTS_ERR_CAPACITY and total == len(full) and "5 of %d" % len(full) in L.lib().rts_last_error().decode()
    R.same_bytes(out[:5], full[:5])
    assert out[5:].tobytes() == tail
    big = np.zeros(len(full), L.PLOT_DTYPE)
    assert raw_eval(rts, det, nd, p, n_rx, nb, big, len(big)) == (L.RTS_OK, len(full))


def test_abi_sizes(rts):
    assert rts.L.PLOT_DTYPE.itemsize == 104 == R.PLOT.itemsize and C.sizeof(rts.L.RtsPlotParams) == 56 and rts.L.RTS_PLOT_MAX_LINK == 4
    assert rts.L.PLOT_DTYPE == R.PLOT
    text = open(os.path.join(ROOT, "rts_amd", "csrc", "rts_internal.h")).read()
    assert "sizeof(RtsPlot) == 104 && sizeof(RtsPlotParams) == 56" in text


# ----------------------------------------------------------------------------- 5. rts_plot.h alone, under the sanitizers
@pytest.fixture(scope="module")
def plot_main(tmp_path_factory):
    gxx = shutil.which("g++")
    if not gxx:
        pytest.skip("no g++")
    rt = subprocess.run([gxx, "-print-file-name=libasan.so"], capture_output=True, text=True).stdout.strip()
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"] if os.path.isabs(rt) and os.path.exists(rt) else []
    exe = str(tmp_path_factory.mktemp("plot") / "plot_main")
    subprocess.check_call([gxx, "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-ffp-contract=off"] + san + ["-I", os.path.join(ROOT, "rts_amd", "csrc"),
                           os.path.join(ROOT, "tests", "plot", "plot_main.cpp"), "-o", exe])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:verify_asan_link_order=0", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")

    def ask(cases):
        """cases: (n_rx, nd, nb, link, min_cells, capacity, det) -> per case (params code, list code, total, PLOT records written,
        pairs on which the enumeration and the predicate disagree)"""
        text = []
        for n_rx, nd, nb, link, min_cells, capacity, det in cases:
            text.append("%d %d %d %s %s %d %d %d %s %d %d" % (n_rx, nd, nb, R.T0.hex(), R.DT.hex(), link[0], link[1], min_cells, R.PRI.hex(), capacity, len(det)))
            text.extend("%d %d %d %s %s %s %s" % (d["rx"], d["doppler_bin"], d["range_bin"], float(d["power"]).hex(), float(d["noise"]).hex(),
                                                  float(d["range_offset"]).hex(), float(d["doppler_offset"]).hex()) for d in det)
        r = subprocess.run([exe], input="\n".join(text) + "\n", capture_output=True, text=True, env=env, timeout=120)
        assert r.returncode == 0, r.stderr[-3000:]
        lines = r.stdout.splitlines()
        assert len(lines) == len(cases)
        out = []
        for line in lines:
            t = line.split()
            rec = np.zeros((len(t) - 4) // 17, R.PLOT)
            for i in range(len(rec)):
                f = t[4 + 17 * i: 21 + 17 * i]
                rec[i] = tuple(int(x) for x in f[:8]) + tuple(float.fromhex(x) for x in f[8:])
            out.append((int(t[0]), int(t[1]), int(t[2]), rec, int(t[3])))
        return out
    return ask


MAIN_CASES = ["empty", "one", "row63", "row64", "row65", "row4097", "wrap", "range_edges", "rx_boundary", "nd1_ld1", "nd2_ld1", "nd2_ld4", "snake", "checker_11",
              "checker_10", "checker_01", "two_apart_20", "two_apart_14", "link44", "min5", "random_0.6_1"]


def test_header_alone_reads_and_writes_only_what_it_is_given(rts, plot_main):
    """lists and outputs are heap arrays of exactly their sizes in the driver; the records equal the library's, bit for bit; the
    neighbour enumeration meets exactly the pairs the adjacency predicate names; a capacity below the total writes the prefix and
    nothing more"""
    cases = []
    for name in MAIN_CASES:
        n_rx, nd, nb, _, link, min_cells = R.CASES[name]
        det = R.case_list(name)
        cases.append((n_rx, nd, nb, link, min_cells, max(len(det), 1), det))
    n_rx, nd, nb, _, link, _ = R.CASES["min1"]
    cases.append((n_rx, nd, nb, link, 1, 3, R.case_list("min1")))
    cases.append((n_rx, nd, nb, link, 1, 0, R.case_list("min1")))
    got = plot_main(cases)
    for name, (pc, lc, total, rec, wrong) in zip(MAIN_CASES, got):
        want = evaluate(rts, name)
        assert (pc, lc, total, wrong) == (0, 0, len(want), 0), name
        R.same_bytes(rec, want)
    full = evaluate(rts, "min1")
    assert got[-2][2] == len(full) and got[-1][2] == len(full) and len(got[-1][3]) == 0
    R.same_bytes(got[-2][3], full[:3])


def test_header_alone_refuses(plot_main):
    good = R.make_list([(0, 1, 1), (0, 1, 2), (0, 5, 5)], 8, 16)
    swapped = good[[1, 0, 2]]
    outside = good.copy(); outside["range_bin"][2] = 16
    got = plot_main([(1, 8, 16, (5, 1), 1, 4, good), (1, 8, 16, (1, 5), 1, 4, good), (1, 8, 16, (1, 1), 1, 4, swapped), (1, 8, 16, (1, 1), 1, 4, outside)])
    assert [g[:3] for g in got] == [(1, 0, 0), (2, 0, 0), (0, 2, 0), (0, 1, 0)]
