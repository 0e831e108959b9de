"""The host-only plan of a pulse's post-processing (rts_amd/csrc/rts_post_plan.h) without a GPU: tests/post_plan/post_plan_main.cpp
includes the header alone, is built with g++ under AddressSanitizer + UndefinedBehaviorSanitizer (without them where g++ has no
libasan, as tests/test_sanitizers.py probes) and answers one case per line.  Every expectation here is an independent
statement -- Python's bit_length, the range of values a field has to hold, the reserve calls of the functions the plan was
taken out of written out -- never the header's own formula."""
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MAX_DEPTH, THREADS, CAP32, CAP64, AGG_TILE = 16, 256, 4096, 2048, 256

DEPTHS = range(17)
TARGETS = (0, 1, 2, 3, 7, 8, 255, 256, 2 ** 20)
RECEIVERS = (0, 1, 2, 3, 16, 17, 2 ** 20)
GRID = [(D, nt, nr) for D in DEPTHS for nt in TARGETS for nr in RECEIVERS]
NAMED = {(10, 7, 2): 31, (10, 7, 4): 32, (15, 15, 16): 64, (15, 15, 17): 65}      # (D, n_targets, n_rx): key bits -- the boundaries of the plan


@pytest.fixture(scope="module")
def plan(tmp_path_factory):
    gxx = shutil.which("g++")
    if not gxx:
        pytest.skip("no g++")
    rt = subprocess.run([gxx, "-print-file-name=libasan.so"], capture_output=True, text=True).stdout.strip()
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"] if os.path.isabs(rt) and os.path.exists(rt) else []
    exe = str(tmp_path_factory.mktemp("post_plan") / "post_plan_main")
    subprocess.check_call([gxx, "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror"] + san + ["-I", os.path.join(ROOT, "rts_amd", "csrc"),
                           os.path.join(ROOT, "tests", "post_plan", "post_plan_main.cpp"), "-o", exe])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:verify_asan_link_order=0", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")

    def ask(cases):
        """cases: tuples (name, integers ...) -> one list of integers per case"""
        text = "".join(" ".join(str(x) for x in c) + "\n" for c in cases)
        r = subprocess.run([exe], input=text, capture_output=True, text=True, env=env, timeout=120)
        assert r.returncode == 0, r.stderr[-3000:]
        out = [[int(x) for x in line.split()] for line in r.stdout.splitlines()]
        assert len(out) == len(cases)
        return out
    return ask


def key_case(D, n_targets, n_rx, max_refr=0):
    """the handle's call: the largest path entry is the last target, the largest receiver index the last receiver (one receiver at least)"""
    return ("key", D, n_targets - 1, max(n_rx, 1) - 1, max_refr)


def key_widths(D, n_targets, n_rx):
    """a path entry + 1 runs over 0 .. n_targets, a receiver index over 0 .. max(n_rx, 1) - 1; a field of either has one bit at least"""
    B = max(1, n_targets.bit_length()) if D else 0
    RXB = max(1, (max(n_rx, 1) - 1).bit_length())
    return B, RXB, D * B + RXB


def test_constants(plan):
    assert plan([("consts",)]) == [[MAX_DEPTH, THREADS, CAP32, CAP64, AGG_TILE]]


def test_bits_for(plan):
    ns = list(range(70001))
    for k in range(33):
        ns += [n for n in (2 ** k - 1, 2 ** k, 2 ** k + 1) if n <= 2 ** 32 + 1]
    got = plan([("bits", n) for n in ns])
    assert [g[0] for g in got] == [max(1, (n - 1).bit_length()) for n in ns]
    assert 2 ** 32 in ns and 2 ** 32 + 1 in ns and 2 ** 32 - 1 in ns


def test_key_plan_over_the_grid(plan):
    got = plan([key_case(*p) for p in GRID])
    n_wide = n_cap32 = 0
    for (D, nt, nr), g in zip(GRID, got):
        B, RXB, key_bits, shift, n_words, n_rx_tab, wide, supported, cap, key64, spec_cap = g
        wB, wRXB, want = key_widths(D, nt, nr)
        assert (B, RXB, key_bits) == (wB, wRXB, want), (D, nt, nr)
        assert wide == (1 if key_bits > 64 else 0)
        assert n_words == -(-key_bits // 64)
        assert supported == (1 if D <= MAX_DEPTH and key_bits <= 256 else 0)
        assert shift == (32 if wide else D * B) and shift < 64
        assert n_rx_tab == max(nr, 1)
        assert (cap == CAP32) == (key_bits < 32) and cap in (CAP32, CAP64) and key64 == (0 if key_bits < 32 else 1)
        assert spec_cap == (0 if wide else cap)                    # (max_refr = 0: the row keys are 32 bits)
        n_wide += wide; n_cap32 += cap == CAP32
    assert n_wide and n_cap32 and any(not g[7] for g in got)       # every branch was met: wide, 32-bit, unsupported
    # the boundaries by name
    got = plan([key_case(*p) for p in NAMED])
    for (p, bits), g in zip(NAMED.items(), got):
        assert g[2] == bits, p
        assert (g[8], g[6]) == {31: (CAP32, 0), 32: (CAP64, 0), 64: (CAP64, 0), 65: (CAP64, 1)}[bits]
    assert got[2][3] == 60                                          # 64 bits: the key fills the word, the receiver sits at bit 60
    # a depth beyond the limit is not supported whatever the width; a chain with refraction rows never takes more than 2 048
    assert plan([("key", 17, 0, 0, 0)])[0][7] == 0
    for p, g in zip(GRID, plan([key_case(*p, max_refr=1) for p in GRID])):
        assert g[10] == (0 if g[6] else CAP64), p


def test_encode_then_decode(plan):
    """seeded random path rows and receivers at every narrow grid point and named boundary: the decoded key is the row and the receiver, two rows
    have one key iff they are one row with one receiver, and the padding key of the one-block sort lies above every real key"""
    rng = np.random.default_rng(20)
    cases, rows = [], []
    for D, nt, nr in GRID + list(NAMED):
        if key_widths(D, nt, nr)[2] > 64:
            continue
        mp, mr = nt - 1, max(nr, 1) - 1
        mine = [(mr, [mp] * D), (0, [-1] * D)]                      # the largest key and the smallest
        for _ in range(6):
            mine.append((int(rng.integers(0, mr + 1)), [int(x) for x in rng.integers(-1, mp + 1, D)]))
        rx, path = mine[-1]
        mine.append((rx, list(path)))                              # the same row again
        if D and mp >= 0:                                          # ... and with one entry changed, with another receiver
            other = list(path); j = int(rng.integers(0, D)); other[j] = path[j] - 1 if path[j] >= 0 else mp
            mine.append((rx, other))
        if mr:
            mine.append(((rx + 1) % (mr + 1), list(path)))
        for rx, path in mine:
            cases.append(("code", D, mp, mr, rx) + tuple(path)); rows.append((D, nt, nr, rx, tuple(path)))
    got = plan(cases)
    seen = {}
    for (D, nt, nr, rx, path), g in zip(rows, got):
        key = g[0]
        assert g[1] == rx and tuple(g[2:]) == path, (D, nt, nr, rx, path)
        bits = key_widths(D, nt, nr)[2]
        assert key < 1 << bits and (bits == 64 or (1 << bits) > key)
        seen.setdefault((D, nt, nr), {}).setdefault(key, set()).add((rx, path))
    assert all(len(v) == 1 for point in seen.values() for v in point.values())                # one key, one (receiver, row)
    for point in seen.values():
        pairs = [p for v in point.values() for p in v]
        assert len(set(pairs)) == len(pairs) == len(point)                                      # one (receiver, row), one key
    assert len(seen) > 500 and (15, 15, 16) in seen and max(k for k in seen[(15, 15, 16)]) >= 1 << 63


def test_recv_sort_bits(plan):
    cases = [(n, r) for n in (1, 63, 64, 2 ** 20, 2 ** 32 - 1) for r in (0, 1, 7)]
    for (n, r), (bits, key64, cap) in zip(cases, plan([("recv",) + c for c in cases])):
        chains = 3 if r else 1
        assert 1 <= bits <= 40
        assert 2 ** bits - 1 > n * chains - 1, (n, r)               # the padding key sorts behind the last row
        assert bits == 1 or 2 ** (bits - 1) - 1 <= n * chains - 1   # ... with no bit to spare
        assert key64 == (1 if r else 0) and cap == (CAP64 if r else CAP32)
        assert key64 or bits <= 32                                  # a 32-bit sort holds every row of a lattice without chains
    # the cap: rows beyond 2^40 cannot occur (3 x 2^32), and the loop stops there all the same
    assert max(g[0] for g in plan([("recv", 2 ** 32 - 1, 1)])) == 34


def test_items_per_thread(plan):
    caps = list(range(1, CAP32 + 1))
    got = [g[0] for g in plan([("items", c) for c in caps])]
    for cap, items in zip(caps, got):
        assert items == min(i for i in (4, 8, 16) if i * THREADS >= cap), cap
        assert cap > CAP64 or items <= 8                           # what a 64-bit sort takes never asks for 16
    assert set(got) == {4, 8, 16}


def test_aggregation_scratch_layout(plan):
    cases = [(R, n) for R in (1, 255, 256, 257, 4096, 2 ** 31 - 1) for n in (1, 17, 2 ** 20)]
    for (R, n), g in zip(cases, plan([("layout",) + c for c in cases])):
        ntiles, per_ray, gcount, gsum, rcs, o_G, o_first, o_last, o_rxmin = g
        # the counts: the reserve calls of rts_post_all_small / rts_aggregate_device before the plan, written out
        assert ntiles == (R + AGG_TILE - 1) // AGG_TILE
        assert per_ray == R and gcount == R + 4 and gsum == 5 * (R + 2 * ntiles) + 16 and rcs == 5 * n + n + 8
        # d_gcount: group starts [R + 1] (one per group and the end), the group count
        slices = [(0, R + 1), (o_G, o_G + 1)]
        assert slices[0][1] <= slices[1][0] and slices[1][1] <= gcount
        # d_gsum: five sums per group (R at most), per tile's first run, per tile's last run
        slices = [(0, 5 * R), (o_first, o_first + 5 * ntiles), (o_last, o_last + 5 * ntiles)]
        assert all(a[1] <= b[0] for a, b in zip(slices, slices[1:])) and slices[-1][1] <= gsum
        # d_rcs, in doubles: five totals per receiver, then the receivers' smallest ray index, 32 bits each
        assert o_rxmin >= 5 * n and o_rxmin + (n + 1) // 2 <= rcs
