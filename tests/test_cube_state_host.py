"""The cube part of a handle (rts_amd/csrc/rts_cube_state.h: RtsCubeProduct, RtsCubeState and its families) without a GPU and without
the HIP runtime: tests/cube_state/cube_state_main.cpp includes the header alone on the stand-ins of tests/owned/fake_hip.h and is built
with g++ under AddressSanitizer + UndefinedBehaviorSanitizer (without them where g++ has no libasan), the way tests/test_owned_host.py
builds its driver.  The driver takes no input and prints lines that begin with a case's name (the tokens are described at its top).
Every expectation here is written out, never read back from the header -- but for ONE count: the RtsCubeProduct members the header
declares, which the driver's end_products case must list one by one."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FLOOR = 65536                      # DevBuf's floor for small element types, in elements (tests/test_owned_host.py pins it): 524 288 bytes of doubles


def _rocm_include():
    for d in (os.environ.get("ROCM_PATH"), os.environ.get("HIP_PATH"), "/opt/rocm"):
        if d and os.path.exists(os.path.join(d, "include", "hip", "hip_runtime_api.h")):
            return os.path.join(d, "include")
    return None


@pytest.fixture(scope="module")
def cases(tmp_path_factory):
    """case name -> the driver's lines of that case, each split into tokens (the name dropped)"""
    gxx, inc = shutil.which("g++"), _rocm_include()
    if not gxx or not inc:
        pytest.skip("needs g++ and the ROCm include directory")
    rt = subprocess.run([gxx, "-print-file-name=libasan.so"], capture_output=True, text=True).stdout.strip()
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"] if os.path.isabs(rt) and os.path.exists(rt) else []
    exe = str(tmp_path_factory.mktemp("cube_state") / "cube_state_main")
    subprocess.check_call([gxx, "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-D__HIP_PLATFORM_AMD__"] + san +
                          ["-I", inc, "-I", os.path.join(ROOT, "rts_amd", "csrc"),
                           os.path.join(ROOT, "tests", "cube_state", "cube_state_main.cpp"), "-o", exe])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:verify_asan_link_order=0", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=120)
    assert r.returncode == 0, r.stderr[-3000:]
    out = {}
    for line in r.stdout.splitlines():
        t = line.split()
        assert not [x for x in t if x.startswith("BAD")], line      # no free of a dead address (a double free), no destroyed event used
        out.setdefault(t[0], []).append(t[1:])
    return out


def one(cases, name):
    assert len(cases[name]) == 1
    return cases[name][0]


def test_place_with_a_callers_pointer(cases):
    """the pointer comes back, nothing is allocated, and the record stays as it was -- empty, or a valid library-owned one, whatever
    the size asked for"""
    assert one(cases, "caller") == ["E:0", "O:2", "R:0:0:0", "C:0", "|", "M:1:%d" % (FLOOR * 8), "|", "E:0", "O:2", "R:1:10:1", "C:%d" % FLOOR, "F:1", "LIVE:0"]


def test_place_that_fits_keeps_a_valid_record(cases):
    """n <= own.cap, the capacity itself included: no allocator call, the own block handed back, p / doubles / valid kept"""
    assert one(cases, "fits") == ["M:1:%d" % (FLOOR * 8), "|", "C:%d" % FLOOR, "E:0", "O:1", "R:1:10:1", "E:0", "O:1", "R:1:10:1", "C:%d" % FLOOR, "F:1", "LIVE:0"]


def test_failed_regrow_leaves_an_ended_record_and_no_block(cases):
    """the allocation of the regrow is told to fail: place returns the error, the old block has been freed exactly once, nothing is
    handed back and the record is ended (p null, doubles 0, not valid) -- a getter asked now refuses, it does not name the freed block"""
    got = one(cases, "regrow_fails")
    assert got == ["M:1:%d" % (FLOOR * 8), "|", "F:1", "X:M", "E:1", "O:0", "R:0:0:0", "C:0", "LIVE:0"]
    assert got.count("F:1") == 1


def test_regrow_ends_the_record_until_record(cases):
    """cap + 1 doubles: the old block goes once, before the new one comes (twice the capacity, the doubling of DevBuf's rule); the own
    block is handed back; the record is ended until record() names the new block"""
    assert one(cases, "regrow") == ["M:1:%d" % (FLOOR * 8), "|", "F:1", "M:2:%d" % (2 * FLOOR * 8), "E:0", "O:1", "R:0:0:0", "R:1:%d:1" % (FLOOR + 1), "F:2", "LIVE:0"]


def test_record_sets_the_three_fields(cases):
    assert one(cases, "record") == ["R:0:0:0", "R:2:7:1", "LIVE:0"]


def test_end_products_ends_every_product_and_nothing_else(cases):
    """every product recorded, the detection list and the plots valid, the tracker live with a time, track-before-detect with 3
    frames and a valid extraction, the waveform set, the alpha cache filled: afterwards every product and the two lists are ended; the
    cube itself (set, params, p), the waveform, the tracker (live, time, cur, max), track-before-detect (frames, shape, ext_valid), the
    alpha cache (table, key, pfa, sent) and the plots' own_list are as they were.  The driver has one line per RtsCubeProduct the
    header declares: a product added without a line there -- and so without a look at its family's end() -- fails here"""
    lines = cases["end_products"]
    prod = [t for t in lines if t[0] == "product"]
    assert [t[1] for t in prod] == ["doppler.map", "image.out", "stft.out", "fmcw.range", "beam.out", "adapt.cov", "adapt.mvdr", "stap.out",
                                    "doa.eig_val", "doa.eig_vec", "doa.spectrum", "focus.align", "focus.pga"]
    assert all(t[2:] == ["1", "0"] for t in prod), prod
    assert [t for t in lines if t[0] == "list"] == [["list", "detect", "1", "0"], ["list", "plot", "1", "0"]]
    assert [t for t in lines if t[0] == "kept"] == [["kept", "1", "1", "1", "1", "1", "1"]]
    assert lines[-1] == ["LIVE:0"]
    header = open(os.path.join(ROOT, "rts_amd", "csrc", "rts_cube_state.h")).read()
    code = re.sub(r"//[^\n]*", "", header)
    declared = sum(len(m.group(1).split(",")) for m in re.finditer(r"\bRtsCubeProduct\s+([A-Za-z_][\w\s,]*);", code))
    assert declared == len(prod) == 13


def test_a_moved_state_frees_everything_once(cases):
    """buffers, products and staged uploads in nine families; the state is move-constructed and both objects leave the scope: the
    source is empty, every block and event is freed exactly once, nothing is live (a second free would be a BAD token)"""
    got = one(cases, "scope")
    i = got.index("|")
    made = [t.split(":") for t in got[:i]]
    blocks = [t[1] for t in made if t[0] == "M"]; pinned = [t[1] for t in made if t[0] == "HM"]; events = [t[1] for t in made if t[0] == "EC"]
    assert (len(blocks), len(pinned), len(events)) == (14, 4, 4)
    assert got[i + 1] == "MOVED:1:1" and got[-1] == "LIVE:0"
    freed = got[i + 2:-1]
    assert sorted(freed) == sorted(["F:" + b for b in blocks] + ["HF:" + b for b in pinned] + ["ED:" + e for e in events])
