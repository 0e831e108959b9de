"""The owning types (rts_amd/csrc/rts_owned.h: DevBuf, PinBuf, StagedUpload) without a GPU and without the HIP runtime:
tests/owned/owned_main.cpp includes the header alone, supplies its own hipMalloc / hipFree / hipHostMalloc / hipHostFree /
hipHostGetDevicePointer, the four event calls and hipMemcpyAsync (which copies the bytes) -- which log every call, know which
blocks and events are live and can be told to fail -- and is built with g++ under
AddressSanitizer + UndefinedBehaviorSanitizer (without them where g++ has no libasan).  One case per line; the driver answers with
the log of allocator calls and the buffers' states (the token format is described at the top of the driver).  Every expectation
here is written out or formed by the growth rule as restated below, never read back from the header."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ESIZES = (1, 8, 144, 145)                             # both sides of the `sizeof(T) <= 144` floor (144: PerRayData)


def _rocm_include():
    for d in (os.environ.get("ROCM_PATH"), os.environ.get("HIP_PATH"), "/opt/rocm"):
        if d and os.path.exists(os.path.join(d, "include", "hip", "hip_runtime_api.h")):
            return os.path.join(d, "include")
    return None


@pytest.fixture(scope="module")
def owned(tmp_path_factory):
    gxx, inc = shutil.which("g++"), _rocm_include()
    if not gxx or not inc:
        pytest.skip("needs g++ and the ROCm include directory")
    rt = subprocess.run([gxx, "-print-file-name=libasan.so"], capture_output=True, text=True).stdout.strip()
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"] if os.path.isabs(rt) and os.path.exists(rt) else []
    exe = str(tmp_path_factory.mktemp("owned") / "owned_main")
    subprocess.check_call([gxx, "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-D__HIP_PLATFORM_AMD__"] + san +
                          ["-I", inc, "-I", os.path.join(ROOT, "rts_amd", "csrc"),
                           os.path.join(ROOT, "tests", "owned", "owned_main.cpp"), "-o", exe])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:verify_asan_link_order=0", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")

    def ask(cases):
        """cases: tuples (name, kind, element size, integers ...) -> the driver's line per case, split into tokens"""
        text = "".join(" ".join(str(x) for x in c) + "\n" for c in cases)
        r = subprocess.run([exe], input=text, capture_output=True, text=True, env=env, timeout=120)
        assert r.returncode == 0, r.stderr[-3000:]
        out = [line.split() for line in r.stdout.splitlines()]
        assert len(out) == len(cases)
        for c, line in zip(cases, out):
            assert not [t for t in line if t.startswith("BAD")], (c, line)      # no free of a dead address (a double free), no bad flags
        return out
    return ask


def dev_want(n, cap, esize):
    """DevBuf::reserve's growth rule, restated: an eighth and 16 elements of headroom, at least twice the old capacity, and at
    least 65 536 elements for element types of up to 144 bytes"""
    want = max(n + n // 8 + 16, 2 * cap)
    return max(want, 65536) if esize <= 144 else want


def expect_grow(ns, esize, kind):
    """the driver's line for `grow`: reserve(n) for every n on ONE buffer, state after each, then the buffer leaves scope"""
    out, cap, blk, nid = [], 0, 0, 1
    for n in ns:
        if n > cap:
            new = dev_want(n, cap, esize) if kind == "dev" else n          # (PinBuf: the caller's size, no rule)
            if blk:
                out.append("%s:%d" % ("F" if kind == "dev" else "HF", blk))           # the old block goes first, once
            out.append("%s:%d:%d" % ("M" if kind == "dev" else "HM", nid, new * esize))
            if kind == "pindev":
                out.append("GP:%d" % nid)
            blk, cap, nid = nid, new, nid + 1
        out += ["E:0", "S:%d:%d:%d" % (blk, cap, 1 if kind == "pindev" and blk else 0)]
    if blk:
        out.append("%s:%d" % ("F" if kind == "dev" else "HF", blk))
    return out + ["LIVE:0"]


def test_growth_rule_written_out(owned):
    """the capacities asked of the allocator at the sizes around the floor, element sizes on both sides of 144 bytes: literal"""
    got = owned([("grow", "dev", 8, 0), ("grow", "dev", 8, 1), ("grow", "dev", 144, 65535), ("grow", "dev", 1, 65536), ("grow", "dev", 8, 65537),
                 ("grow", "dev", 145, 0), ("grow", "dev", 145, 1), ("grow", "dev", 145, 65535), ("grow", "dev", 145, 65537),
                 ("grow", "dev", 145, 1, 17, 18, 37), ("grow", "dev", 8, 1, 65536, 65537)])
    assert got[0] == ["E:0", "S:0:0:0", "LIVE:0"]                                          # nothing asked for, nothing allocated
    assert got[1] == ["M:1:%d" % (65536 * 8), "E:0", "S:1:65536:0", "F:1", "LIVE:0"]       # the floor
    assert got[2] == ["M:1:%d" % (73742 * 144), "E:0", "S:1:73742:0", "F:1", "LIVE:0"]     # 65 535 + 8 191 + 16
    assert got[3] == ["M:1:73744", "E:0", "S:1:73744:0", "F:1", "LIVE:0"]
    assert got[4] == ["M:1:%d" % (73745 * 8), "E:0", "S:1:73745:0", "F:1", "LIVE:0"]
    assert got[5] == ["E:0", "S:0:0:0", "LIVE:0"]
    assert got[6] == ["M:1:%d" % (17 * 145), "E:0", "S:1:17:0", "F:1", "LIVE:0"]           # no floor above 144 bytes
    assert got[7] == ["M:1:%d" % (73742 * 145), "E:0", "S:1:73742:0", "F:1", "LIVE:0"]
    assert got[8] == ["M:1:%d" % (73745 * 145), "E:0", "S:1:73745:0", "F:1", "LIVE:0"]
    # regrows: the old block is freed once, before the new allocation; 18 -> 36 by the headroom, 37 -> 72 and 65 537 -> 131 072 by the doubling
    assert got[9] == ["M:1:%d" % (17 * 145), "E:0", "S:1:17:0", "E:0", "S:1:17:0", "F:1", "M:2:%d" % (36 * 145), "E:0", "S:2:36:0",
                      "F:2", "M:3:%d" % (72 * 145), "E:0", "S:3:72:0", "F:3", "LIVE:0"]
    assert got[10] == ["M:1:%d" % (65536 * 8), "E:0", "S:1:65536:0", "E:0", "S:1:65536:0", "F:1", "M:2:%d" % (131072 * 8), "E:0", "S:2:131072:0", "F:2", "LIVE:0"]


@pytest.mark.parametrize("esize", ESIZES)
def test_growth_regrow_and_no_growth(owned, esize):
    """one buffer through n = 0, 1, 65 535, 65 536, 65 537, a size the doubling decides, sizes below the capacity in between: an
    allocator call only when n > cap, the old block freed exactly once BEFORE the new allocation, the capacity by the rule"""
    first = dev_want(1, 0, esize)
    seqs = [[0, 1, 1, first, 0], [0, 1, first + 1, 2], [65535, 65536, 65537, 65536, 1], [65536, 65537], [65537, 131074, 131075, 1 << 20],
            [1, first + 1, 2 * first + 1, 5 * first]]
    got = owned([("grow", "dev", esize) + tuple(s) for s in seqs])
    for s, g in zip(seqs, got):
        assert g == expect_grow(s, esize, "dev"), (esize, s)


@pytest.mark.parametrize("kind", ["dev", "pin", "pindev"])
def test_release_twice_is_harmless(owned, kind):
    a, f = ("M", "F") if kind == "dev" else ("HM", "HF")
    gp = ["GP:1"] if kind == "pindev" else []
    gp2 = ["GP:2"] if kind == "pindev" else []
    cap1, cap2 = (17, 26) if kind == "dev" else (1, 9)
    got = owned([("release", kind, 145, 1, 9)])[0]
    assert got == ["%s:1:%d" % (a, cap1 * 145)] + gp + ["%s:1" % f, "S:0:0:0", "S:0:0:0", "%s:2:%d" % (a, cap2 * 145)] + gp2 + \
        ["S:2:%d:%d" % (cap2, 1 if kind == "pindev" else 0), "%s:2" % f, "S:0:0:0", "LIVE:0"]


def test_failed_allocation_leaves_the_buffer_empty(owned):
    """a failed first allocation; a failed regrow (the old block is gone, the buffer empty, the destructor frees nothing); the
    buffer is usable again afterwards"""
    got = owned([("fail", "dev", 145, 1, 0, 5), ("fail", "dev", 145, 2, 0, 5, 100, 7), ("fail", "pin", 8, 1, 0, 5), ("fail", "pin", 8, 2, 0, 5, 100, 7),
                 ("fail", "pindev", 8, 2, 0, 5, 100, 7)])
    assert got[0] == ["X:M", "E:1", "S:0:0:0", "LIVE:0"]
    assert got[1] == ["M:1:%d" % (21 * 145), "E:0", "S:1:21:0", "F:1", "X:M", "E:1", "S:0:0:0", "M:2:%d" % (23 * 145), "E:0", "S:2:23:0", "F:2", "LIVE:0"]
    assert got[2] == ["X:HM", "E:1", "S:0:0:0", "LIVE:0"]
    assert got[3] == ["HM:1:40", "E:0", "S:1:5:0", "HF:1", "X:HM", "E:1", "S:0:0:0", "HM:2:56", "E:0", "S:2:7:0", "HF:2", "LIVE:0"]
    assert got[4] == ["HM:1:40", "GP:1", "E:0", "S:1:5:1", "HF:1", "X:HM", "E:1", "S:0:0:0", "HM:2:56", "GP:2", "E:0", "S:2:7:1", "HF:2", "LIVE:0"]


def test_failed_device_address_query_leaves_the_buffer_empty(owned):
    """PinBuf: the block of a reserve whose device-address query fails is given back at once"""
    got = owned([("fail", "pindev", 8, 0, 1, 5, 6), ("fail", "pindev", 8, 0, 2, 5, 6)])
    assert got[0] == ["HM:1:40", "X:GP", "HF:1", "E:1", "S:0:0:0", "HM:2:48", "GP:2", "E:0", "S:2:6:1", "HF:2", "LIVE:0"]
    assert got[1] == ["HM:1:40", "GP:1", "E:0", "S:1:5:1", "HF:1", "HM:2:48", "X:GP", "HF:2", "E:1", "S:0:0:0", "LIVE:0"]


@pytest.mark.parametrize("kind", ["dev", "pin", "pindev"])
def test_moves(owned, kind):
    """move construction and move assignment leave the source empty (and usable), the assignment target's old block is freed once,
    self-move-assignment changes nothing, nothing is freed twice (the driver flags it) and nothing is live at the end"""
    a, f = ("M", "F") if kind == "dev" else ("HM", "HF")
    d = 1 if kind == "pindev" else 0
    cap = (lambda n: dev_want(n, 0, 145)) if kind == "dev" else (lambda n: n)
    al = lambda i, n: ["%s:%d:%d" % (a, i, cap(n) * 145)] + (["GP:%d" % i] if d else [])
    got = owned([("movector", kind, 145, 5), ("moveassign", kind, 145, 5, 9, 3), ("selfmove", kind, 145, 5), ("moveassign", kind, 145, 5, 0, 0)])
    assert got[0] == al(1, 5) + ["S:0:0:0", "S:1:%d:%d" % (cap(5), d), "%s:1" % f, "LIVE:0"]
    assert got[1] == al(1, 5) + al(2, 9) + ["|", "%s:2" % f, "S:0:0:0", "S:1:%d:%d" % (cap(5), d)] + al(3, 3) + ["S:3:%d:%d" % (cap(3), d)] + \
        ["%s:1" % f, "%s:3" % f, "LIVE:0"]                     # (b before a: reverse order of declaration)
    assert got[2] == al(1, 5) + ["|", "S:1:%d:%d" % (cap(5), d), "%s:1" % f, "LIVE:0"]
    assert got[3] == al(1, 5) + ["|", "S:0:0:0", "S:1:%d:%d" % (cap(5), d), "S:0:0:0", "%s:1" % f, "LIVE:0"]      # an empty target: nothing to free


@pytest.mark.parametrize("kind,esize", [("pin", 1), ("pin", 8), ("pindev", 144), ("pindev", 145)])
def test_pinned_growth(owned, kind, esize):
    """PinBuf: exactly the size asked for (the callers bring their own growth), no call when n <= cap, the old block freed once
    before the new allocation, the device address fetched only when asked and anew after every regrow"""
    seqs = [[0, 1, 1, 0], [64, 64, 70, 65, 1024], [512, 520, 8, 521], [65535, 65536, 65537]]
    got = owned([("grow", kind, esize) + tuple(s) for s in seqs])
    for s, g in zip(seqs, got):
        assert g == expect_grow(s, esize, kind), (kind, esize, s)
        assert ("GP:1" in g) == (kind == "pindev")
    d = 1 if kind == "pindev" else 0
    gp = (lambda i: ["GP:%d" % i]) if d else (lambda i: [])
    assert got[1] == ["HM:1:%d" % (64 * esize)] + gp(1) + ["E:0", "S:1:64:%d" % d] * 2 + ["HF:1", "HM:2:%d" % (70 * esize)] + gp(2) + \
        ["E:0", "S:2:70:%d" % d] * 2 + ["HF:2", "HM:3:%d" % (1024 * esize)] + gp(3) + ["E:0", "S:3:1024:%d" % d, "HF:3", "LIVE:0"]


def test_a_struct_of_owners_moves_as_a_whole(owned):
    """(that it cannot be copied is a static_assert in the driver)"""
    got = owned([("holder", "dev", 1, 100)])[0]
    i = got.index("|")
    assert got[:i] == ["M:1:%d" % (65536 * 4), "M:2:%d" % (65536 * 4), "M:3:%d" % (65536 * 8), "HM:4:100", "GP:4"]
    assert got[i + 1:i + 6] == ["S:0:0:0", "S:0:0:0", "S:1:65536:0", "S:0:0:0", "S:4:100:1"]
    assert sorted(got[i + 6:-1]) == ["F:1", "F:2", "F:3", "HF:4"] and got[-1] == "LIVE:0"


# ---- StagedUpload<double>: a step is begin(need, grow_to, dev_need) and, when n != 0, a fill of n elements and send(n).  Blocks and
# events are numbered apart, each from 1; the device buffer of a few doubles is DevBuf's floor of 65 536 elements (524 288 bytes).
# U:<pinned block>:<cap>:<device block>:<cap>:<event>:<armed>
FIRST = ["HM:1:128", "EC:1", "M:2:524288", "E:0", "U:1:16:2:65536:1:0", "W:1", "CP:2:1:80", "ER:1", "E:0", "EQ:1", "U:1:16:2:65536:1:1"]      # the step (10, 16, 10, 10) on a new object
EMPTY = "U:0:0:0:0:0:0"


def test_staged_first_use_creates_one_event_and_the_scope_end_destroys_it_once(owned):
    """room on both sides (the pinned block of the size to grow to, not of the need), ONE event, the copy of n elements from the
    pinned block to the device block, the record; the device bytes are the staged ones; the scope end destroys the event first and
    exactly once, then frees the two blocks"""
    got = owned([("steps", "staged", 0, 0, 10, 16, 10, 10)])[0]
    assert got == FIRST + ["|", "ED:1", "F:2", "HF:1", "LIVE:0"]


def test_staged_second_begin_waits_before_the_staging_is_touched_or_regrown(owned):
    got = owned([("steps", "staged", 0, 0, 10, 16, 10, 10, 12, 16, 12, 12), ("steps", "staged", 0, 0, 10, 16, 10, 10, 20, 30, 20, 20)])
    # room enough: the wait, then the fill, no allocator call, no second event
    assert got[0] == FIRST + ["ES:1", "E:0", "U:1:16:2:65536:1:0", "W:1", "CP:2:1:96", "ER:1", "E:0", "EQ:1", "U:1:16:2:65536:1:1", "|", "ED:1", "F:2", "HF:1", "LIVE:0"]
    # too small: the wait comes BEFORE the old pinned block is freed (once) and replaced by one of grow_to = 30 elements
    assert got[1] == FIRST + ["ES:1", "HF:1", "HM:3:240", "E:0", "U:3:30:2:65536:1:0", "W:3", "CP:2:3:160", "ER:1", "E:0", "EQ:1", "U:3:30:2:65536:1:1",
                              "|", "ED:1", "F:2", "HF:3", "LIVE:0"]
    for g in got:
        assert g.count("EC:1") == 1 and not [t for t in g if t.startswith("EC:") and t != "EC:1"]
        assert g.count("HF:1") == 1 and g.count("ED:1") == 1


def test_staged_begin_without_a_send_arms_nothing(owned):
    """nothing to upload (the pattern rows of a pulse without receivers): the next begin does not wait, a regrow needs no wait either"""
    got = owned([("steps", "staged", 0, 0, 10, 16, 10, 0, 20, 30, 20, 0, 5, 5, 5, 5)])[0]
    assert got == ["HM:1:128", "EC:1", "M:2:524288", "E:0", "U:1:16:2:65536:1:0", "HF:1", "HM:3:240", "E:0", "U:3:30:2:65536:1:0",
                   "E:0", "U:3:30:2:65536:1:0", "W:3", "CP:2:3:40", "ER:1", "E:0", "EQ:1", "U:3:30:2:65536:1:1", "|", "ED:1", "F:2", "HF:3", "LIVE:0"]
    assert not [t for t in got if t.startswith("ES:")]


def test_staged_failures_leave_the_object_destructible_and_usable(owned):
    got = owned([("steps", "staged", 1, 0, 10, 16, 10, 10, 10, 16, 10, 10), ("steps", "staged", 0, 1, 10, 16, 10, 10, 10, 16, 10, 10),
                 ("steps", "staged", 2, 0, 10, 16, 10, 10, 10, 16, 10, 10), ("steps", "staged", 0, 1, 10, 16, 10, 10)])
    tail = ["|", "ED:1", "F:2", "HF:1", "LIVE:0"]
    assert got[0] == ["X:HM", "E:1", EMPTY] + FIRST + tail                                       # the pinned block: nothing exists, no event yet
    assert got[1] == ["HM:1:128", "X:EC", "E:1", "U:1:16:0:0:0:0", "EC:1", "M:2:524288"] + FIRST[3:] + tail        # the event: no handle kept
    assert got[2] == ["HM:1:128", "EC:1", "X:M", "E:1", "U:1:16:0:0:1:0", "M:2:524288"] + FIRST[3:] + tail         # the device buffer
    assert got[3] == ["HM:1:128", "X:EC", "E:1", "U:1:16:0:0:0:0", "|", "HF:1", "LIVE:0"]        # destroyed as the failure left it: no event to destroy


def test_staged_moves(owned):
    """move construction and move assignment leave the source empty (and usable) and carry the armed event along: the new owner's
    next begin waits for it; the assignment target gives up its own event and blocks once; nothing is destroyed twice"""
    again = ["ES:1", "E:0", "U:1:16:2:65536:1:0", "W:1", "CP:2:1:80", "ER:1", "E:0", "EQ:1", "U:1:16:2:65536:1:1"]
    got = owned([("movector", "staged", 10, 16, 10, 10), ("moveassign", "staged", 10, 16, 10, 10, 5, 8, 5, 5), ("selfmove", "staged", 10, 16, 10, 10)])
    assert got[0] == FIRST + ["|", EMPTY, "U:1:16:2:65536:1:1"] + again + ["|", "ED:1", "F:2", "HF:1", "LIVE:0"]
    second = ["HM:3:64", "EC:2", "M:4:524288", "E:0", "U:3:8:4:65536:2:0", "W:3", "CP:4:3:40", "ER:2", "E:0", "EQ:1", "U:3:8:4:65536:2:1"]
    third = ["HM:5:128", "EC:3", "M:6:524288", "E:0", "U:5:16:6:65536:3:0", "W:5", "CP:6:5:80", "ER:3", "E:0", "EQ:1", "U:5:16:6:65536:3:1"]
    assert got[1] == FIRST + second + ["|", "ED:2", "HF:3", "F:4", EMPTY, "U:1:16:2:65536:1:1"] + third + \
        ["|", "ED:1", "F:2", "HF:1", "ED:3", "F:6", "HF:5", "LIVE:0"]                         # (b before a: reverse order of declaration)
    assert got[2] == FIRST + ["|", "U:1:16:2:65536:1:1", "|", "ED:1", "F:2", "HF:1", "LIVE:0"]
