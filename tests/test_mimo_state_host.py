"""The MIMO family's record in the cube part of a handle (rts_amd/csrc/rts_cube_state.h: RtsMimoState) without a GPU and without the
HIP runtime: tests/mimo/mimo_state_main.cpp, built the way tests/test_cube_state_host.py builds its driver.  That driver lists the
products declared under RtsCubeProduct's own name and stays as it is; the bank's output is declared through the alias
RtsBankProduct, and this file holds it to the same rule: rts_cube_attach (end_products) ends it and keeps the blocks, a regrow of the
library-owned output ends the record before the block is freed, a smaller staged table allocates nothing, and a moved state frees
every block once."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _rocm_include():
    for d in (os.environ.get("ROCM_PATH"), os.environ.get("HIP_PATH"), "/opt/rocm"):
        if d and os.path.exists(os.path.join(d, "include", "hip", "hip_runtime_api.h")):
            return os.path.join(d, "include")
    return None


@pytest.fixture(scope="module")
def cases(tmp_path_factory):
    gxx, inc = shutil.which("g++"), _rocm_include()
    if not gxx or not inc:
        pytest.skip("needs g++ and the ROCm include directory")
    rt = subprocess.run([gxx, "-print-file-name=libasan.so"], capture_output=True, text=True).stdout.strip()
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"] if os.path.isabs(rt) and os.path.exists(rt) else []
    exe = str(tmp_path_factory.mktemp("mimo_state") / "mimo_state_main")
    subprocess.check_call([gxx, "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-D__HIP_PLATFORM_AMD__"] + san +
                          ["-I", inc, "-I", os.path.join(ROOT, "rts_amd", "csrc"), os.path.join(ROOT, "tests", "mimo", "mimo_state_main.cpp"), "-o", exe])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:verify_asan_link_order=0", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=120)
    assert r.returncode == 0, r.stderr[-3000:]
    out = {}
    for line in r.stdout.splitlines():
        t = line.split()
        assert not [x for x in t if x.startswith("BAD")], line
        out.setdefault(t[0], []).append(t[1:])
    return out


def test_attach_ends_the_banks_output_and_keeps_its_blocks(cases):
    lines = cases["end_products"]
    assert ["product", "mimo.out", "1", "0"] in lines and ["product", "doppler.map", "1", "0"] in lines
    assert ["kept", "1"] in lines and lines[-1][-1] == "LIVE:0"


def test_a_regrow_of_the_library_owned_output_ends_the_record_first(cases):
    assert cases["regrow"] == [["1", "1", "0", "1"]]


def test_a_smaller_set_reuses_the_staged_upload(cases):
    assert cases["reuse"] == [["1"]]


def test_a_moved_state_frees_every_block_once(cases):
    (got,) = cases["scope"]
    i = got.index("|")
    blocks = [t.split(":")[1] for t in got[:i] if t.startswith("M:")]
    pinned = [t.split(":")[1] for t in got[:i] if t.startswith("HM:")]
    assert len(blocks) == 2 and len(pinned) == 1 and got[i + 1] == "MOVED:1:1" and got[-1] == "LIVE:0"
    frees = [t for t in got[i + 2:-1] if not t.startswith("ED:")]
    assert sorted(frees) == sorted(["F:" + b for b in blocks] + ["HF:" + b for b in pinned])


def test_the_alias_is_the_only_product_of_the_family():
    header = open(os.path.join(ROOT, "rts_amd", "csrc", "rts_cube_state.h")).read()
    code = re.sub(r"//[^\n]*", "", header)
    assert len(re.findall(r"\bRtsBankProduct\s+\w+\s*;", code)) == 1 and "using RtsBankProduct = RtsCubeProduct;" in code
    assert re.search(r"void end_products\(\)[^}]*mimo\.end\(\);", code)
