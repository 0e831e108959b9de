"""The static primitive order of the per-pulse scene update (rts_amd/csrc/rts_prim_order.h) without a GPU and without HIP:
tests/prim_order/prim_order_main.cpp includes the header alone and is built with g++ (under AddressSanitizer +
UndefinedBehaviorSanitizer where g++ has them).  The order is the primitives by FIRST appearance in the leaf slots -- split
references name a primitive several times -- with every primitive no slot names appended, ascending: a permutation of
0 .. n_prims - 1 whatever the slots hold.  Every expectation is written out or restated here in Python."""
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def order_of(tmp_path_factory):
    gxx = shutil.which("g++")
    if not gxx:
        pytest.skip("needs g++")
    rt = subprocess.run([gxx, "-print-file-name=libasan.so"], capture_output=True, text=True).stdout.strip()
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"] if os.path.isabs(rt) and os.path.exists(rt) else []
    exe = str(tmp_path_factory.mktemp("prim_order") / "prim_order_main")
    subprocess.check_call([gxx, "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror"] + san +
                          ["-I", os.path.join(ROOT, "rts_amd", "csrc"), os.path.join(ROOT, "tests", "prim_order", "prim_order_main.cpp"), "-o", exe])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:verify_asan_link_order=0", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")

    def ask(cases):
        """cases: (n_prims, slots) -> the order per case"""
        text = "".join(" ".join(str(x) for x in [n] + list(slots)) + "\n" for n, slots in cases)
        r = subprocess.run([exe], input=text, capture_output=True, text=True, env=env, timeout=120)
        assert r.returncode == 0, r.stderr[-3000:]
        out = [[int(t) for t in line.split()] for line in r.stdout.split("\n")[:-1]]
        assert len(out) == len(cases)
        return out
    return ask


def restated(n_prims, slots):
    seen, out = set(), []
    for g in slots:
        if g < n_prims and g not in seen:
            seen.add(g); out.append(g)
    return out + [g for g in range(n_prims) if g not in seen]


def test_written_out(order_of):
    got = order_of([(3, [2, 0, 2, 1, 0]), (5, [2, 0, 2, 1, 0]), (6, [4, 4, 4]), (4, []), (0, []), (1, [0]), (3, [1, 7, 1, 4294967295, 0])])
    assert got[0] == [2, 0, 1]                      # the later slots of a split triangle are dropped
    assert got[1] == [2, 0, 1, 3, 4]                # primitives no slot names: appended, ascending
    assert got[2] == [4, 0, 1, 2, 3, 5]
    assert got[3] == [0, 1, 2, 3]                   # no slots at all (a scene without a hierarchy): the identity
    assert got[4] == []
    assert got[5] == [0]
    assert got[6] == [1, 0, 2]                      # a slot that names no primitive of the scene is skipped


def test_always_a_permutation(order_of):
    rng = np.random.default_rng(7)
    cases = []
    for n in (1, 2, 255, 256, 257, 1000):
        for rep in (1, 3):
            slots = rng.integers(0, n, size=rep * n).tolist()         # with repetitions, some primitives never named
            cases.append((n, slots))
        cases.append((n, rng.permutation(n).tolist()))
    for (n, slots), got in zip(cases, order_of(cases)):
        assert sorted(got) == list(range(n))
        assert got == restated(n, slots)
