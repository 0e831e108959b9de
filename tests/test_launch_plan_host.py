"""The host-only plan of a pulse's launch (rts_amd/csrc/rts_launch_plan.h) without a GPU: tests/launch_plan/launch_plan_main.cpp
includes the header alone, is built with g++ under AddressSanitizer + UndefinedBehaviorSanitizer (without them where g++ has no
libasan, as tests/test_sanitizers.py probes) and answers one case per line.  Every expectation here is an independent
statement -- Python integer division, brute-force enumeration of launch indices, the buffers' documented layouts
(rts_internal.h: RtsTraceArgs) -- never the header's own formula."""
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIST = 0xffffffff                                     # RTS_INTERLEAVE_LIST (include/rts_amd.h)
OK, E_LIST_TILE, E_INTERLEAVE, E_OUTSIDE, E_LIST_BEYOND = range(5)
WTILE, BLOCK, COOP_GROUP, STACK_OVF = 64, 256, 32, 128


@pytest.fixture(scope="module")
def plan(tmp_path_factory):
    gxx = shutil.which("g++")
    if not gxx:
        pytest.skip("no g++")
    rt = subprocess.run([gxx, "-print-file-name=libasan.so"], capture_output=True, text=True).stdout.strip()
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"] if os.path.isabs(rt) and os.path.exists(rt) else []
    exe = str(tmp_path_factory.mktemp("launch_plan") / "launch_plan_main")
    subprocess.check_call([gxx, "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror"] + san + ["-I", os.path.join(ROOT, "rts_amd", "csrc"),
                           os.path.join(ROOT, "tests", "launch_plan", "launch_plan_main.cpp"), "-o", exe])
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


def test_constants_and_small_helpers(plan):
    assert plan([("consts",)]) == [[WTILE, BLOCK, COOP_GROUP, STACK_OVF]]
    cases = [(n, W, r) for n, W, r in [(0, 1, 0), (1, 2, 1), (63, 3, 2), (64, 20, 0), (65, 1625, 6), (2 ** 32 - 1, 1626, 7)]]
    got = plan([("small",) + c for c in cases])
    assert got == [[-(-n // WTILE), W ** 3, 3 if r else 1, r + 1] for n, W, r in cases]


def _quotients(W, magic, more, g):
    """rts_lattice_coords (rts_raygen.h): q = (((g - t) >> 1) + t) >> more with t = mulhi(magic, g), in 32-bit arithmetic"""
    g = g.astype(np.uint64)
    t = (np.uint64(magic) * g) >> np.uint64(32)
    return ((((g - t) >> np.uint64(1)) + t) & np.uint64(0xffffffff)) >> np.uint64(more)


def test_div_magic_divides_exactly(plan):
    """every W whose lattice fits 32 bits (1625^3 < 2^32): the multiply-shift quotient of the device equals g // W at the edges of
    the lattice, at 2^32 - 1, around 64 seeded multiples of W, and -- seven widths, powers of two (magic == 0) among them -- at
    every g below min(W^3, 2^22)"""
    Ws = list(range(2, 1626))
    assert 1625 ** 3 < 2 ** 32 <= 1626 ** 3
    consts = plan([("magic", W) for W in Ws])
    assert plan([("magic", 0), ("magic", 1)]) == [[0, 0], [0, 0]]
    rng = np.random.default_rng(1625)
    for W, (magic, more) in zip(Ws, consts):
        assert (magic == 0) == (W & (W - 1) == 0), W
        k = rng.integers(1, 2 ** 32 // W + 1, 64, dtype=np.uint64) * np.uint64(W)
        g = np.concatenate([np.array([0, 1, W - 1, W, W + 1, W * W - 1, W * W, W ** 3 - 1, 2 ** 32 - 1], np.uint64), k - np.uint64(1), k[k < 2 ** 32]])
        assert np.array_equal(_quotients(W, magic, more, g), g // np.uint64(W)), W
        q = g[g < W ** 3] // np.uint64(W)                       # the second division of rts_lattice_coords: the quotient by W again
        assert np.array_equal(_quotients(W, magic, more, q), q // np.uint64(W)), W
    for W in (2, 3, 5, 7, 641, 1024, 1625):
        magic, more = consts[W - 2]
        g = np.arange(min(W ** 3, 2 ** 22), dtype=np.uint64)
        assert np.array_equal(_quotients(W, magic, more, g), g // np.uint64(W)), W


def _brute(span, tile, parts=None, part=None, tiles=None):
    """launch indices of a range of span that belong to interleaved part `part`, or to the listed tiles"""
    j = np.arange(span, dtype=np.int64) // tile
    return int(np.count_nonzero(j % parts == part)) if tiles is None else int(np.count_nonzero(np.isin(j, np.array(tiles, np.int64))))


TOTALS = (1, 63, 64, 65, 125, 4095, 4096, 8000)
TILES = (1, 64, 100, 4096)


def _ranges(total):
    """(ray_first, ray_count) pairs of a lattice of `total`: to the end, and counts that end in the middle of a tile"""
    out = []
    for first in sorted({0, 1, 64, total - 1} & set(range(total))):
        left = total - first
        for count in sorted({0, left, left - 1, left // 2 + 1, 33} & set(range(left + 1))):
            out.append((first, count, count if count else left))
    return out


def test_part_count_and_ray_range_against_enumeration(plan):
    """interleaved parts: every launch index of the range is enumerated and dealt to part (i // tile) % parts; the library's
    count, the resolved range and rts_amd.multigpu.part_ray_count agree with it, and the parts cover the range"""
    from rts_amd import multigpu
    cases, want = [], []
    for total in TOTALS:
        for first, count, span in _ranges(total):
            cases.append(("range", first, count, total, 0, 0, 0, LIST, 0, 0, 0, 0)); want.append([OK, first, span, span, 0, 0, 0, 0, 0])      # contiguous
            cases.append(("range", first, count, total, 64, 1, 0, LIST, 64, 3, 2, 9)); want.append([OK, first, span, span, 0, 0, 0, 0, 0])    # parts <= 1: the interleave fields are not looked at
            for tile in TILES:
                for parts in (2, 3, 5):
                    mine = [_brute(span, tile, parts, part) for part in range(parts)]
                    assert sum(mine) == span
                    for part in range(parts):
                        assert multigpu.part_ray_count(span, (tile, parts, part)) == mine[part]
                        cases.append(("range", first, count, total, tile, parts, part, LIST, 0, 0, 0, 0)); want.append([OK, first, span, mine[part], 0, tile, parts, part, 0])
                        cases.append(("part", span, tile, parts, part)); want.append([mine[part]])
    assert plan(cases) == want


def test_ray_range_over_dealt_lists(plan):
    """dealt tile lists: empty, one tile, the (partial) last tile of the range, several tiles; a list that names a tile beyond the
    range is that error, and the launch constants carry the list's mark and generation"""
    cases, want = [], []
    for total in TOTALS:
        for first, count, span in _ranges(total):
            for tile in TILES:
                n_t = -(-span // tile)
                lists = [[], [0], [n_t - 1], sorted({0, n_t // 2, n_t - 1})] if n_t else [[]]
                for ids in lists:
                    cases.append(("range", first, count, total, tile, LIST, 5, LIST, tile, len(ids), ids[-1] if ids else 0, 7))
                    want.append([OK, first, span, _brute(span, tile, tiles=ids), n_t, tile, LIST, 7, 1])
                for last in (n_t, n_t + 3):
                    if n_t:
                        cases.append(("range", first, count, total, tile, LIST, 0, LIST, tile, 2, last, 7))
                        want.append([E_LIST_BEYOND, first, span, 0, n_t, tile, LIST, 7, 1])
    got = plan(cases)
    assert got == want
    assert any(w[0] == OK and 0 < w[3] % w[5] for w in want)          # a listed partial last tile was among them


def test_ray_range_errors_and_their_precedence(plan):
    """every error value, and which one is reported when several arguments are wrong at once: the list's tile, then the
    interleave, then the range, then the list's extent"""
    T = 8000
    cases = [
        ("range", 0, 0, T, 64, LIST, 0, LIST, 0, 0, 0, 1),            # no list on the handle
        ("range", 0, 0, T, 128, LIST, 0, LIST, 64, 2, 1, 1),          # a list of another tile size
        ("range", T + 1, 0, T, 128, LIST, 0, LIST, 64, 2, 900, 1),    # ... whatever else is wrong
        ("range", 0, 0, T, 0, 3, 1, LIST, 0, 0, 0, 0),                # tile 0
        ("range", 0, 0, T, 64, 3, 3, LIST, 0, 0, 0, 0),               # part == parts
        ("range", T + 1, 0, T, 64, 2, 2, LIST, 0, 0, 0, 0),           # ... and a bad range
        ("range", T + 1, 0, T, 0, 0, 0, LIST, 0, 0, 0, 0),            # first beyond the lattice
        ("range", 1, T, T, 0, 0, 0, LIST, 0, 0, 0, 0),                # count beyond the end
        ("range", 0, T + 1, T, 64, 2, 1, LIST, 0, 0, 0, 0),
        ("range", 0, T + 64, T, 64, LIST, 0, LIST, 64, 1, 999, 1),    # ... before the list's extent is looked at
        ("range", 0, 0, T, 64, LIST, 0, LIST, 64, 1, 125, 1),         # tiles 0 .. 124 exist
        ("range", T, 0, T, 0, 0, 0, LIST, 0, 0, 0, 0),                # first == W^3: an empty range, not an error
    ]
    want = [E_LIST_TILE, E_LIST_TILE, E_LIST_TILE, E_INTERLEAVE, E_INTERLEAVE, E_INTERLEAVE, E_OUTSIDE, E_OUTSIDE, E_OUTSIDE, E_OUTSIDE, E_LIST_BEYOND, OK]
    got = plan(cases)
    assert [g[0] for g in got] == want
    assert set(want) == {OK, E_LIST_TILE, E_INTERLEAVE, E_OUTSIDE, E_LIST_BEYOND}
    assert got[-1][1:4] == [T, 0, 0]


def _resident(n_cu, mult, spare):
    """blocks of the trace kernel's resident set: mult per CU, less `spare` block slots per 256 CUs, at least one per CU"""
    return max(n_cu * mult - spare * n_cu // 256, n_cu)


def test_trace_and_coop_grids(plan):
    cases = [("grid", 0, 256, 4, 0), ("grid", 1, 256, 4, 0), ("grid", 256, 256, 4, 0), ("grid", 257, 256, 4, 0),
             ("grid", 216 ** 3, 256, 4, 0), ("grid", 216 ** 3, 256, 4, 160), ("grid", 2 ** 32 - 16, 256, 4, 160), ("grid", 216 ** 3, 1, 4, 160), ("grid", 216 ** 3, 1, 4, 1024), ("grid", 1023 * 256 + 1, 256, 4, 0),
             ("coop", 0, 0, 1024), ("coop", 0, 1, 1024), ("coop", 1, 0, 1024), ("coop", 1, 1, 1024), ("coop", 2, 1, 1024), ("coop", 5, 0, 1024),
             ("coop", 63, 0, 1024), ("coop", 64, 0, 1024), ("coop", 128, 1, 1024), ("coop", 16384, 0, 1024), ("coop", 2 ** 32 - 1, 0, 4096), ("coop", 1, 0, 1)]
    want = [1, 1, 1, 2, 1024, 864, 864, 4, 1, 1024,
            0, 0, 16, 16, 16, 80, 1008, 1024, 1024, 1024, 4096, 1]
    assert (_resident(256, 4, 0), _resident(256, 4, 160), _resident(1, 4, 160), _resident(1, 4, 1024)) == (1024, 864, 4, 1)
    assert [g[0] for g in plan(cases)] == want


def test_reserve_covers_every_launch(plan):
    """rts_launch_sizes given the bounds rts_reserve documents (n_cu * 64 blocks of threads for the child slab, n_cu * 1024 threads
    for the overflow stack, n_cu * 64 blocks plus the cooperative grid; restated here, not read from rts_api.hip) is no smaller
    in any buffer than given a launch's own values at the default four blocks per CU -- and every buffer of the launch holds
    what its layout says (RtsTraceArgs).  What rts_reserve itself passes is not seen from here."""
    cases, keys = [], []
    for W in (1, 2, 20):
        n = W ** 3
        for refl in (0, 1, 6):
            for refr in (0, 2):
                for keep in (0, 1):
                    for n_cu in (1, 256):
                        for coop_max, coop_on in ((1024, 1), (1024, 0), (4096, 1)):
                            coop_threads = coop_max * BLOCK if coop_on else 0
                            cases.append(("sizes", n, n_cu * 64 * BLOCK, n_cu * 1024, coop_threads, n_cu * 64 + coop_max, refl, refr, keep))
                            keys.append(None)
                            for spare in (0, 160):
                                grid = max(min(-(-n // BLOCK), _resident(n_cu, 4, spare)), 1)
                                cases.append(("grid", n, n_cu, 4, spare)); keys.append(("grid", grid))
                                cases.append(("sizes", n, grid * BLOCK, grid * BLOCK, coop_threads, grid + coop_max, refl, refr, keep))
                                keys.append((n, grid, coop_threads, coop_max, refl, refr, keep))
    got = plan(cases)
    reserve = None
    for out, key in zip(got, keys):
        if key is None:
            reserve = out
        elif key[0] == "grid":
            assert out == [key[1]]
        else:
            n, grid, coop_threads, coop_max, refl, refr, keep = key
            assert all(a <= b for a, b in zip(out, reserve)), (key, out, reserve)
            recv, dir_hist, child, stack, blockc, all_, hit_prim, hit_t = out
            chains, rows = (3 if refr else 1), grid * BLOCK + coop_threads
            assert recv >= n * chains and dir_hist >= (3 * (refl + 1) if refr else refl) * 3 * n
            assert child >= (2 * rows if refr else 0) and stack >= STACK_OVF * rows and blockc >= (grid + coop_max) * 8
            assert (all_ >= n * chains and hit_prim >= n * (refl + 1) and hit_t >= n * (refl + 1)) if keep else (all_, hit_prim, hit_t) == (0, 0, 0)


def test_launch_shape(plan):
    """signature, alignment and tile counts of a launch: aligned means wave tiles of 64 consecutive launch indices on the lattice's own tile grid"""
    T = 20 ** 3
    cases = [("shape", 8000, 0, 0, 0, 0, T), ("shape", 7999, 1, 0, 0, 0, T), ("shape", 7936, 64, 0, 0, 0, T), ("shape", 2688, 0, 64, 3, 1, T),
             ("shape", 2700, 0, 100, 3, 1, T), ("shape", 128, 0, 64, LIST, 7, T), ("shape", 0, 0, 64, LIST, 7, 1)]
    want = [[8000, 0, 0, 0, 1, 125, 125], [7999, 1, 0, 0, 0, 125, 125], [7936, 64, 0, 0, 1, 124, 125], [2688, 0, (3 << 32) | 64, 1, 1, 42, 125],
            [2700, 0, (3 << 32) | 100, 1, 0, 43, 125], [128, 0, (LIST << 32) | 64, 7, 1, 2, 125], [0, 0, (LIST << 32) | 64, 7, 1, 0, 1]]
    assert plan(cases) == want
