"""Multistatic localisation on the host (rts_locate_eval, rts_amd/csrc/rts_locate.h): against the independent restatement
(tests/locate_ref.py: numpy, np.linalg, the serial greedy pass) -- the same discrete outcome and positions, velocities and costs within
the bound the restatement measures on itself; the known answers of the small geometries; the resolution alone on candidate lists;
every refusal, each leaving the outputs untouched; both capacities; and the header alone under the sanitizers
(tests/locate/locate_main.cpp) on the edge sizes."""
import ctypes as C
import math
import os
import shutil
import subprocess

import numpy as np
import pytest

import locate_ref as R

ROOT = R.ROOT
C0 = R.C0


def evaluate(rts, c):
    return rts.locate_eval(c["list"], **c["par"])


# ----------------------------------------------------------------------------- 1. against the restatement
@pytest.mark.parametrize("name", list(R.CASES))
def test_eval_against_restatement(rts, name):
    got = evaluate(rts, R.case(name))
    want, cut = R.expected(name)
    assert len(got) == len(want) and not cut
    for f in R.DISCRETE:
        assert np.array_equal(got[f], want[f]), f
    for f, key in (("pos", "pos"), ("vel", "vel"), ("cost", "cost")):
        diff = float(np.max(np.abs(got[f] - want[f]))) if len(got) else 0.0
        print(name, f, diff, R.bound(key))
        assert diff <= R.bound(key), (f, diff, R.bound(key))


def test_the_cases_find_their_targets():
    """the restatement's own outcome: most targets of every scene, each made of the records of ONE true target (power_sum 1 + t)"""
    for name, n in (("four_rx", 12), ("five_rx", 16), ("missing", 9), ("no_doppler", 8), ("seg63", 5), ("seg64", 5), ("seg65", 5)):
        t, _ = R.expected(name)
        assert len(t) >= n - 1, name
        z = R.case(name)["list"]
        for o in t:
            pw = {z["power_sum"][e] for e in o["plot"] if e != R.NONE}
            assert len(pw) == 1, (name, pw)
    assert len(R.expected("seg0")[0]) == 0 and len(R.expected("seg1")[0]) == 1


# ----------------------------------------------------------------------------- 2. known answers
GROUND = np.array([[7000.0, 5000.0, 0.0], [20000.0, 0.0, 0.0], [-19000.0, -14000.0, 0.0], [-10000.0, 7000.0, 2000.0]])      # three anchors in the plane of the transmitter
ORIGIN = np.zeros(3)
WIDE = ((-4e4, -4e4, -13e3), (4e4, 4e4, 13e3))


def exact(tx, rx, x, v=(0.0, 0.0, 0.0), skip=()):
    return R.make_plots([(m, d, f, 2.0 + m) for m, (d, f) in enumerate(R.measure(tx, rx, x, v)) if m not in skip])


def test_one_target_four_receivers(rts):
    x, v = np.array([5000.0, -12000.0, 7000.0]), np.array([120.0, -40.0, 15.0])
    t = rts.locate_eval(exact(R.TX, R.RX5[:4], x, v), **R.par())
    assert len(t) == 1 and t["n_receivers"][0] == 4 and t["flags"][0] == 0 and t["plot"][0][:4].tolist() == [0, 1, 2, 3] and np.all(t["plot"][0][4:] == R.NONE)
    assert np.max(np.abs(t["pos"][0] - x)) < 1e-6 and np.max(np.abs(t["vel"][0] - v)) < 1e-6 and t["cost"][0] < 1e-12 and t["power_sum"][0] == 2.0 + 3.0 + 4.0 + 5.0
    assert t["candidate"][0] in (0, 1)


def test_mirror_root_and_the_box(rts):
    """transmitter and anchors in the plane z = 0: the two roots are mirror images with the same r; the box decides, and the root
    numbers are the two halves of one triple"""
    x = np.array([-9000.0, -11000.0, 5000.0])
    z = exact(ORIGIN, GROUND[:3], x)
    kw = dict(tx=ORIGIN, rx_positions=GROUND[:3], carrier=0.0)
    up = rts.locate_eval(z, **R.par(box=((-4e4, -4e4, 0.0), (4e4, 4e4, 13e3)), **kw))
    down = rts.locate_eval(z, **R.par(box=((-4e4, -4e4, -13e3), (4e4, 4e4, 0.0)), **kw))
    assert len(up) == len(down) == 1 and np.max(np.abs(up["pos"][0] - x)) < 1e-6 and np.max(np.abs(down["pos"][0] - x * [1, 1, -1])) < 1e-6
    assert sorted([int(up["candidate"][0]), int(down["candidate"][0])]) == [0, 1]
    assert len(rts.locate_eval(z, **R.par(box=((-4e4, -4e4, 6000.0), (4e4, 4e4, 13e3)), **kw))) == 0
    both = rts.locate_eval(z, **R.par(box=WIDE, **kw))          # both roots accepted, one set of records: one target
    assert len(both) == 1 and abs(abs(both["pos"][0][2]) - 5000.0) < 1e-6


def test_both_roots_in_the_box_decided_by_the_fourth_receiver(rts):
    x = np.array([-9000.0, -11000.0, 5000.0])
    t = rts.locate_eval(exact(ORIGIN, GROUND, x), **R.par(tx=ORIGIN, rx_positions=GROUND, box=WIDE, carrier=0.0))
    assert len(t) == 1 and t["n_receivers"][0] == 4 and np.max(np.abs(t["pos"][0] - x)) < 1e-6


def test_coplanar_in_a_tilted_plane(rts):
    """transmitter and anchors in one plane that is no coordinate plane: det D is rounding noise; the closed form does not invert D"""
    rot = np.array([[1.0, 0.0, 0.0], [0.0, math.cos(0.3), -math.sin(0.3)], [0.0, math.sin(0.3), math.cos(0.3)]])
    rx = GROUND @ rot.T
    tx = np.array([100.0, 200.0, 300.0])
    x = np.array([-9000.0, -11000.0, 5000.0]) @ rot.T + tx
    t = rts.locate_eval(exact(tx, rx + tx, x), **R.par(tx=tx, rx_positions=rx + tx, box=WIDE, carrier=0.0))
    assert len(t) == 1 and t["n_receivers"][0] == 4 and np.max(np.abs(t["pos"][0] - x)) < 1e-5


def test_three_receivers_make_ghosts(rts):
    """with exactly three receivers every feasible triple is a zero-cost candidate (the header: inherent, not repaired): of the 8
    triples of two targets 1.5 km apart all are feasible here, the 2 true ones and 6 ghosts -- the restatement counts the same; the
    resolution still returns 2 targets, every record once, but nothing says they are the true ones"""
    xs = [np.array([5000.0, -12000.0, 7000.0]), np.array([6000.0, -11000.0, 7500.0])]
    rows = [[R.measure(R.TX, R.RX5[m:m + 1], x)[0] for x in xs] for m in range(3)]
    kw = R.par(rx_positions=R.RX5[:3], carrier=0.0)
    feasible = 0
    for i in range(2):
        for j in range(2):
            for k in range(2):
                z = R.make_plots([(0,) + rows[0][i] + (1.0,), (1,) + rows[1][j] + (1.0,), (2,) + rows[2][k] + (1.0,)])
                n = len(rts.locate_eval(z, **kw))
                assert n <= 1 and (n == 1 or not i == j == k) and n == len(R.locate(kw, z)[0])
                feasible += n
    assert feasible == 2 + GHOST_TRIPLES
    z = R.make_plots([(m,) + rows[m][t] + (1.0,) for m in range(3) for t in range(2)])
    t = rts.locate_eval(z, **kw)
    assert len(t) == 2 and sorted(t["plot"][:, :3].ravel().tolist()) == [0, 1, 2, 3, 4, 5] and np.all(t["cost"] < 1e-12)


GHOST_TRIPLES = 6


def test_no_carrier_no_velocity(rts):
    c = R.case("no_doppler")
    t = evaluate(rts, c)
    assert len(t) == 8 and np.all(t["vel"] == 0.0)
    with_f = rts.locate_eval(c["list"], **dict(c["par"], carrier=C0 / R.LAM))
    assert len(with_f) >= 7 and np.all(np.any(with_f["vel"] != 0.0, axis=1))


def test_receiver_without_a_record_and_min_receivers(rts):
    x = np.array([5000.0, -12000.0, 7000.0])
    z = exact(R.TX, R.RX5, x, skip=(3,))
    t = rts.locate_eval(z, **R.par(rx_positions=R.RX5, min_receivers=4))
    assert len(t) == 1 and t["n_receivers"][0] == 4 and t["plot"][0][:5].tolist() == [0, 1, 2, R.NONE, 3]
    assert len(rts.locate_eval(z, **R.par(rx_positions=R.RX5, min_receivers=5))) == 0
    far = z.copy(); far["delay"][3] += 41.0 / C0                        # beyond assoc_delay (40 m): receiver 4 has none either
    t = rts.locate_eval(far, **R.par(rx_positions=R.RX5, min_receivers=3))
    assert len(t) == 1 and t["n_receivers"][0] == 3 and t["plot"][0][4] == R.NONE
    nan = z.copy(); nan["doppler"][3] = math.nan                        # a record that is not finite takes no part
    t = rts.locate_eval(nan, **R.par(rx_positions=R.RX5, min_receivers=3))
    assert len(t) == 1 and t["n_receivers"][0] == 3
    nan = z.copy(); nan["delay"][1] = math.inf                          # ... nor forms a triple
    assert len(rts.locate_eval(nan, **R.par(rx_positions=R.RX5, min_receivers=3))) == 0


UNREFINED = dict(tx=ORIGIN, rx_positions=GROUND * [1.0, 1.0, 0.0], carrier=0.0, n_iters=2, box=((-4e4, -4e4, -1.0), (4e4, 4e4, 1.0)))


def unrefined_list():
    return exact(ORIGIN, GROUND * [1.0, 1.0, 0.0], np.array([-9000.0, -11000.0, 0.0]))


def test_unrefined_flag(rts):
    """everything in the plane z = 0, the target too: the closed form lands in the plane exactly (a double root), every row of J has
    a zero z component, the third pivot of J^T J is 0: the refinement ends where it stands and says so"""
    t = rts.locate_eval(unrefined_list(), **R.par(**UNREFINED))
    assert len(t) == 1 and t["flags"][0] == rts.L.RTS_TARGET_UNREFINED and t["n_receivers"][0] == 4
    assert np.max(np.abs(t["pos"][0] - [-9000.0, -11000.0, 0.0])) < 1e-6 and t["pos"][0][2] == 0.0 and t["cost"][0] < 1e-12
    t = rts.locate_eval(unrefined_list(), **R.par(**dict(UNREFINED, n_iters=0)))
    assert len(t) == 1 and t["flags"][0] == 0


def test_tracks_as_source(rts):
    """confirmed tracks that are not coasting take part, in (rx, table index) order; plot[] holds table indices"""
    x = np.array([5000.0, -12000.0, 7000.0])
    m = R.measure(R.TX, R.RX5[:4], x)
    tab = np.zeros(7, R.TRACK)
    for i, (rx, flags) in enumerate([(3, 1), (1, 1), (0, 0), (2, 1), (0, 1), (1, 3), (9, 1)]):
        tab[i]["rx"], tab[i]["flags"], tab[i]["delay"], tab[i]["doppler"], tab[i]["power_sum"] = rx, flags, m[rx % 4][0], m[rx % 4][1], 1.0 + i
    t = rts.locate_eval(tab, **R.par(source="tracks"))
    assert len(t) == 1 and t["plot"][0][:4].tolist() == [4, 1, 3, 0] and t["power_sum"][0] == 5.0 + 2.0 + 4.0 + 1.0 and np.max(np.abs(t["pos"][0] - x)) < 1e-6


# ----------------------------------------------------------------------------- 3. the resolution alone
@pytest.mark.parametrize("name", list(R.CANDIDATES))
def test_resolution_from_candidates(rts, name):
    c = R.CANDIDATES[name]
    t = rts.locate_eval(c, **R.par(source="candidates"))
    assert t["candidate"].tolist() == R.CANDIDATE_WINNERS[name]
    want = c[np.isin(c["candidate"], R.CANDIDATE_WINNERS[name])]
    R.same_bytes(t, want.copy())                                        # the records pass through as they are
    ref = R.resolve([dict(n_receivers=int(o["n_receivers"]), cost=float(o["cost"]), candidate=int(o["candidate"]), plot=o["plot"].tolist()) for o in c])
    assert [r["candidate"] for r in ref] == R.CANDIDATE_WINNERS[name]


# ----------------------------------------------------------------------------- 4. refusals and the capacities
def params(rts, **kw):
    c = R.case("four_rx")
    p, keep = rts._locate_params(**dict(c["par"], rx_positions=c["par"]["rx_positions"].copy()))      # (keep: the array p points to; a case may spoil it)
    for k, v in kw.items():
        if k == "reserved":
            p.reserved[v] = 1
        elif k in ("tx", "box_lo", "box_hi", "anchors"):
            getattr(p, k)[v[0]] = v[1]
        elif k == "rx_value":
            keep[v[0], v[1]] = v[2]
        else:
            setattr(p, k, v)
    return p, keep


def raw_eval(rts, p, z, out, capacity, null=()):
    n = C.c_uint32(77)
    rc = rts.L.lib().rts_locate_eval(C.byref(p) if p is not None else None, None if "list" in null else rts.ptr(z), len(z), None if "out" in null else rts.ptr(out), capacity,
                                     None if "n" in null else C.byref(n))
    return rc, n.value


REFUSED = [("n_rx", dict(n_rx=2)), ("n_rx", dict(n_rx=17)), ("rx_positions", dict(rx_positions=None)), ("finite", dict(tx=(1, math.nan))), ("finite", dict(rx_value=(2, 1, math.inf))),
           ("anchors", dict(anchors=(1, 0))), ("anchors", dict(anchors=(2, 4))), ("cspeed", dict(cspeed=0.0)), ("cspeed", dict(cspeed=math.inf)), ("carrier", dict(carrier=-1.0)),
           ("carrier", dict(carrier=math.nan)), ("sigma_delay", dict(sigma_delay=0.0)), ("sigma_delay", dict(sigma_delay=math.nan)), ("sigma_doppler", dict(sigma_doppler=-2.0)),
           ("sigma_doppler", dict(sigma_doppler=math.inf)), ("gate", dict(gate=0.0)), ("gate", dict(gate=math.nan)), ("assoc_delay", dict(assoc_delay=0.0)),
           ("assoc_delay", dict(assoc_delay=math.inf)), ("box_lo", dict(box_lo=(0, 5e4))), ("box_lo", dict(box_hi=(2, math.nan))), ("min_receivers", dict(min_receivers=2)),
           ("min_receivers", dict(min_receivers=5)), ("n_iters", dict(n_iters=9)), ("max_candidates", dict(max_candidates=(1 << 20) + 1)), ("max_targets", dict(max_targets=65537)),
           ("source", dict(source=3)), ("without device_list", dict(n_list=3)), ("n_list", dict(device_list=4096, n_list=(1 << 24) + 1)), ("8-byte", dict(device_list=4100)),
           ("reserved", dict(reserved=0)), ("reserved", dict(reserved=1)), ("RTS_LOCATE_FROM_TRACKS", dict(source=1, device_list=4096))]


@pytest.mark.parametrize("field,kw", REFUSED)
def test_refused_parameters(rts, field, kw):
    c = R.case("four_rx")
    out = np.full(16, 0x5a, np.uint8).repeat(144).view(R.TARGET); before = out.tobytes()
    p, keep = params(rts, **kw)
    rc, n = raw_eval(rts, p, c["list"], out, len(out))
    assert rc == rts.L.RTS_ERR_INVALID and field in rts.L.lib().rts_last_error().decode() and out.tobytes() == before and n == 77


def test_refused_collinear_anchors(rts):
    c = R.case("four_rx")
    rx = np.array([[1000.0, 0.0, 0.0], [2000.0, 0.0, 0.0], [5000.0, 0.0, 1e-6], [0.0, 3000.0, 0.0]])
    with pytest.raises(rts.L.RtsError, match="collinear"):
        rts.locate_eval(c["list"], **R.par(rx_positions=rx))
    assert len(rts.locate_eval(c["list"], **R.par(rx_positions=rx, anchors=(0, 1, 3)))) == 0      # (the transmitter may lie on a baseline's line)


def test_refused_lists_and_arguments(rts):
    L = rts.L
    c = R.case("four_rx")
    out = np.full(16, 0x5a, np.uint8).repeat(144).view(R.TARGET); before = out.tobytes()

    def refused(word, p, z, **kw):
        rc, n = raw_eval(rts, p, np.ascontiguousarray(z), out, len(out), **kw)
        assert rc == L.RTS_ERR_INVALID and word in L.lib().rts_last_error().decode() and out.tobytes() == before and n == 77, word

    p, keep = params(rts)
    refused("rx must not decrease", p, c["list"][::-1])
    for null in ("list", "out", "n"):
        refused("null", p, c["list"], null=(null,))
    assert raw_eval(rts, None, c["list"], out, len(out))[0] == L.RTS_ERR_INVALID and out.tobytes() == before
    pc, keep2 = params(rts, source=L.RTS_LOCATE_FROM_CANDIDATES)
    good = R.CANDIDATES["shared"]
    refused("candidate", pc, good[::-1])
    bad = good.copy(); bad["plot"][1][2] = 1 << 20
    refused("RTS_LOCATE_MAX_INDEX", pc, bad)
    for k in (0, 17):
        bad = good.copy(); bad["n_receivers"][3] = k
        refused("n_receivers", pc, bad)
    for v in (-1.0, math.nan):
        bad = good.copy(); bad["cost"][0] = v
        refused("cost", pc, bad)
    # an empty list may be NULL
    rc, n = raw_eval(rts, p, c["list"][:0].copy(), None, 0, null=("list", "out"))
    assert (rc, n) == (L.RTS_OK, 0)


def test_both_capacities(rts):
    L = rts.L
    c = R.case("four_rx")
    full = evaluate(rts, c)
    assert len(full) == 12
    # the caller's array: the prefix, the total, the tail untouched
    out = np.full(16, 0x5a, np.uint8).repeat(144).view(R.TARGET); tail = out[5:].tobytes()
    p, keep = params(rts)
    rc, n = raw_eval(rts, p, c["list"], out, 5)
    assert rc == L.RTS_ERR_CAPACITY and n == 12 and "5 of 12" in L.lib().rts_last_error().decode() and out[5:].tobytes() == tail
    R.same_bytes(out[:5].copy(), full[:5].copy())
    # max_targets: the same through the library's own limit
    p, keep = params(rts, max_targets=7)
    rc, n = raw_eval(rts, p, c["list"], out, len(out))
    assert rc == L.RTS_ERR_CAPACITY and n == 12 and out[7:].tobytes() == b"\x5a" * (144 * 9)
    R.same_bytes(out[:7].copy(), full[:7].copy())
    # max_candidates: the stored prefix of the accepted candidates is resolved
    p, keep = params(rts, max_candidates=4)
    out[:] = np.full(16, 0x5a, np.uint8).repeat(144).view(R.TARGET)
    rc, n = raw_eval(rts, p, c["list"], out, len(out))
    assert rc == L.RTS_ERR_CAPACITY and "max_candidates" in L.lib().rts_last_error().decode() and 1 <= n <= 4 and out[n:].tobytes() == b"\x5a" * (144 * (16 - n))
    ref, cut = R.locate(dict(c["par"], max_candidates=4), c["list"])
    assert cut and R.records(ref)["candidate"].tolist() == out["candidate"][:n].tolist()
    rc, n = raw_eval(rts, params(rts)[0], c["list"], None, 0, null=("out",))
    assert (rc, n) == (L.RTS_ERR_CAPACITY, 12)


def test_anchor_segment_is_cut_at_1024(rts):
    L = rts.L
    x = np.array([5000.0, -12000.0, 7000.0])
    m = R.measure(R.TX, R.RX5[:4], x)
    rows = [(0, 1e-6, 0.0, 0.5)] * 1024 + [(0,) + m[0] + (1.0,)] + [(r,) + m[r] + (1.0,) for r in (1, 2, 3)]      # the target's record is number 1025 of anchor 0
    z = R.make_plots(rows)
    out = np.zeros(4, R.TARGET)
    p, keep = params(rts)
    rc, n = raw_eval(rts, p, z, out, len(out))
    assert rc == L.RTS_ERR_CAPACITY and n == 0 and "RTS_LOCATE_MAX_PER_RX" in L.lib().rts_last_error().decode()
    rc, n = raw_eval(rts, p, z[1:].copy(), out, len(out))
    assert rc == L.RTS_OK and n == 1 and out["plot"][0][0] == 1023


def test_abi_sizes(rts):
    L = rts.L
    assert L.TARGET_DTYPE.itemsize == 144 and C.sizeof(L.RtsLocateParams) == 192
    assert (L.RTS_LOCATE_MAX_RX, L.RTS_LOCATE_MAX_PER_RX, L.RTS_LOCATE_MAX_ITERS, L.RTS_TARGET_UNREFINED) == (16, R.MAX_PER_RX, 8, 1)
    text = open(os.path.join(ROOT, "rts_amd", "csrc", "rts_internal.h")).read()
    assert "sizeof(RtsTarget) == 144 && sizeof(RtsLocateParams) == 192" in text
    hdr = open(os.path.join(ROOT, "include", "rts_amd.h")).read()
    assert "} RtsLocateParams;                                            /* 192 bytes */" in hdr and "} RtsTarget;                                                  /* 144 bytes */" in hdr


# ----------------------------------------------------------------------------- 5. rts_locate.h alone, under the sanitizers
@pytest.fixture(scope="module")
def locate_main(tmp_path_factory):
    gxx = shutil.which("g++")
    if not gxx:
        pytest.skip("no g++")
    rt = subprocess.run([gxx, "-print-file-name=libasan.so"], capture_output=True, text=True).stdout.strip()
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"] if os.path.isabs(rt) and os.path.exists(rt) else []
    exe = str(tmp_path_factory.mktemp("locate") / "locate_main")
    subprocess.check_call([gxx, "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-ffp-contract=off"] + san + ["-I", os.path.join(ROOT, "rts_amd", "csrc"),
                           os.path.join(ROOT, "tests", "locate", "locate_main.cpp"), "-o", exe])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:verify_asan_link_order=0", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    sources = {"plots": 0, "tracks": 1, "candidates": 2}

    def ask(cases):
        """cases: (par, list, capacity[, reserved]) -> per case (params code, list code, total, cut, clean, TARGET records written)"""
        hx = lambda v: float(v).hex()
        text = []
        for case in cases:
            p, z, capacity = case[:3]
            rx = np.asarray(p["rx_positions"], float).reshape(-1, 3)
            n_rx = p.get("n_rx", len(rx))
            head = [n_rx] + list(p["anchors"]) + [n_rx if p["min_receivers"] is None else p["min_receivers"], p["n_iters"], p["max_candidates"], p["max_targets"], sources[p["source"]],
                                                   case[3] if len(case) > 3 else 0, capacity, len(z)]
            text.append(" ".join(str(int(v)) for v in head))
            vals = list(p["tx"]) + list(rx[:n_rx].ravel()) + [p["cspeed"], p["carrier"], p["sigma"][0], p["sigma"][1], p["gate"], p["assoc_delay"]] + list(p["box"][0]) + list(p["box"][1])
            text.append(" ".join(hx(v) for v in vals))
            if p["source"] == "candidates":
                text.extend("%d %d %s %s" % (t["candidate"], t["n_receivers"], hx(t["cost"]), " ".join(str(int(e)) for e in t["plot"])) for t in z)
            else:
                text.extend("%d %d %s %s %s" % (t["rx"], t["flags"] if p["source"] == "tracks" else 0, hx(t["delay"]), hx(t["doppler"]), hx(t["power_sum"])) for t in z)
        r = subprocess.run([exe], input="\n".join(text) + "\n", capture_output=True, text=True, env=env, timeout=120)
        assert r.returncode == 0, r.stderr[-3000:]
        lines = r.stdout.splitlines()
        assert len(lines) == len(cases)
        out = []
        for line in lines:
            t = line.split()
            rec = np.zeros(int(t[5]), R.TARGET)
            for i in range(len(rec)):
                f = t[6 + 27 * i: 33 + 27 * i]
                rec[i]["candidate"], rec[i]["n_receivers"], rec[i]["flags"] = int(f[0]), int(f[1]), int(f[2])
                rec[i]["plot"] = [int(v) for v in f[3:19]]
                vals = [float.fromhex(v) for v in f[19:]]
                rec[i]["pos"], rec[i]["vel"], rec[i]["cost"], rec[i]["power_sum"] = vals[0:3], vals[3:6], vals[6], vals[7]
            out.append(tuple(int(v) for v in t[:5]) + (rec,))
        return out
    return ask


MAIN_CASES = ["four_rx", "five_rx_anchors", "missing", "no_doppler", "iters0", "seg0", "seg1", "seg63", "seg64", "seg65", "seg257"]


def test_header_alone_reads_and_writes_only_what_it_is_given(rts, locate_main):
    """lists, receiver arrays and outputs are heap arrays of exactly their sizes in the driver; the records equal the library's byte for
    byte, the candidate lists pass through; a capacity below the total writes the prefix and nothing more"""
    cases = [(R.case(n)["par"], R.case(n)["list"], 32) for n in MAIN_CASES]
    cases += [(R.par(source="candidates"), R.CANDIDATES[n], len(R.CANDIDATES[n])) for n in R.CANDIDATES]
    cases.append((R.par(**UNREFINED), unrefined_list(), 4))
    c = R.case("four_rx")
    cases += [(c["par"], c["list"], 3), (c["par"], c["list"], 0)]
    got = locate_main(cases)
    for n, g in zip(MAIN_CASES, got):
        want = evaluate(rts, R.case(n))
        assert g[:5] == (0, 0, len(want), 0, 1), (n, g[:5])
        R.same_bytes(g[5], want)
    for n, g in zip(R.CANDIDATES, got[len(MAIN_CASES):]):
        assert g[:2] == (0, 0) and g[4] == 1 and g[5]["candidate"].tolist() == R.CANDIDATE_WINNERS[n], n
    assert got[-3][5]["flags"].tolist() == [1]
    full = evaluate(rts, c)
    assert got[-2][:5] == (0, 0, 12, 0, 1) and got[-1][:5] == (0, 0, 12, 0, 1) and len(got[-1][5]) == 0
    R.same_bytes(got[-2][5], full[:3].copy())


def test_header_alone_refuses(locate_main):
    c = R.case("four_rx")
    cases, want = [], []
    for code, kw in ((1, dict(n_rx=2)), (4, dict(anchors=(0, 0, 2))), (4, dict(anchors=(0, 1, 4))), (6, dict(cspeed=0.0)), (7, dict(carrier=-1.0)), (8, dict(sigma=(0.0, 1.0))),
                     (9, dict(sigma=(1e-8, math.inf))), (10, dict(gate=math.nan)), (11, dict(assoc_delay=0.0)), (12, dict(box=((0, 0, 1.0), (1, 1, 0.0)))), (13, dict(min_receivers=5)),
                     (14, dict(n_iters=9)), (15, dict(max_candidates=(1 << 20) + 1)), (16, dict(max_targets=65537)),
                     (5, dict(rx_positions=np.array([[1e3, 0, 0], [2e3, 0, 0], [5e3, 0, 0], [0, 3e3, 0.0]]))), (3, dict(tx=(0.0, math.nan, 0.0)))):
        cases.append((dict(c["par"], **kw), c["list"], 8)); want.append((code, 0))
    cases.append((c["par"], c["list"], 8, 1)); want.append((21, 0))
    cases.append((c["par"], c["list"][::-1], 8)); want.append((0, 1))
    cases.append((R.par(source="candidates"), R.CANDIDATES["shared"][::-1], 8)); want.append((0, 1))
    got = locate_main(cases)
    for g, w in zip(got, want):
        assert g[:2] == w and g[2:5] == (0, 0, 1) and len(g[5]) == 0, (g[:5], w)      # refused: nothing evaluated, the output untouched
