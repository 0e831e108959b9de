"""The passive family's record in the cube part of a handle (rts_amd/csrc/rts_cube_state.h: RtsPassiveState) without a GPU and without
the HIP runtime: tests/passive/passive_state_main.cpp, built the way tests/test_cube_state_host.py builds its driver.  That driver
lists the thirteen products declared under RtsCubeProduct's own name and stays as it is; the correlation's output is the fourteenth,
declared through the alias RtsXcorrProduct, and this file holds it to the same rule: rts_cube_attach (end_products) ends it and the
cancellation's record, keeps the buffers and the shape, and a moved state frees every block once."""
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
    exe = str(tmp_path_factory.mktemp("passive_state") / "passive_state_main")
    subprocess.check_call([gxx, "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-D__HIP_PLATFORM_AMD__"] + san +
                          ["-I", inc, "-I", os.path.join(ROOT, "rts_amd", "csrc"), os.path.join(ROOT, "tests", "passive", "passive_state_main.cpp"), "-o", exe])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:verify_asan_link_order=0", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=120)
    assert r.returncode == 0, r.stderr[-3000:]
    out = {}
    for line in r.stdout.splitlines():
        t = line.split()
        assert not [x for x in t if x.startswith("BAD")], line
        out.setdefault(t[0], []).append(t[1:])
    return out


def test_attach_ends_the_correlation_and_the_cancellations_record(cases):
    lines = cases["end_products"]
    assert ["product", "passive.xcorr", "1", "0"] in lines and ["record", "passive.cancel", "1", "0"] in lines and ["product", "doppler.map", "1", "0"] in lines
    assert ["kept", "1"] in lines and lines[-1][-1] == "LIVE:0"


def test_a_moved_state_frees_every_block_once(cases):
    (got,) = cases["scope"]
    i = got.index("|")
    blocks = [t.split(":")[1] for t in got[:i] if t.startswith("M:")]
    assert len(blocks) == 5 and got[i + 1] == "MOVED:1:1" and got[-1] == "LIVE:0"
    assert sorted(got[i + 2:-1]) == sorted("F:" + b for b in blocks)


def test_the_alias_is_the_only_product_outside_the_older_drivers_list():
    header = open(os.path.join(ROOT, "rts_amd", "csrc", "rts_cube_state.h")).read()
    code = re.sub(r"//[^\n]*", "", header)
    assert len(re.findall(r"\bRtsXcorrProduct\s+\w+\s*;", code)) == 1 and "using RtsXcorrProduct = RtsCubeProduct;" in code
