"""The phase of a handle's pulse and the per-device count of open pulses (rts_amd/csrc/rts_pulse_state.h) without a GPU:
tests/pulse_state/pulse_state_main.cpp includes the header alone, is built with g++ under AddressSanitizer +
UndefinedBehaviorSanitizer (without them where g++ has no libasan, as tests/test_sanitizers.py probes) and answers one case per
line.  Every expectation here is the transition table restated in Python (TABLE below) -- never the header's code:

    begin IDLE -> OPEN +1 | end OPEN -> IDLE -1 | chain OPEN -> CHAINED 0 | resolve CHAINED -> IDLE -1 | abandon any -> IDLE, -1 unless IDLE

a transition from another phase changes nothing and says so; devices share a slot modulo 64."""
import itertools
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
IDLE, OPEN, CHAINED = 0, 1, 2
OPS = "becra"                                          # begin, end, chain, resolve, abandon
# (transition, phase before) -> (phase after, change of the count); absent: refused
TABLE = {("b", IDLE): (OPEN, +1), ("e", OPEN): (IDLE, -1), ("c", OPEN): (CHAINED, 0), ("r", CHAINED): (IDLE, -1),
         ("a", OPEN): (IDLE, -1), ("a", CHAINED): (IDLE, -1)}


@pytest.fixture(scope="module")
def ask(tmp_path_factory):
    gxx = shutil.which("g++")
    if not gxx:
        pytest.skip("no g++")
    rt = subprocess.run([gxx, "-print-file-name=libasan.so"], capture_output=True, text=True).stdout.strip()
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"] if os.path.isabs(rt) and os.path.exists(rt) else []
    exe = str(tmp_path_factory.mktemp("pulse_state") / "pulse_state_main")
    subprocess.check_call([gxx, "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror"] + san + ["-I", os.path.join(ROOT, "rts_amd", "csrc"),
                           os.path.join(ROOT, "tests", "pulse_state", "pulse_state_main.cpp"), "-o", exe])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:verify_asan_link_order=0", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")

    def run(lines):
        r = subprocess.run([exe], input="".join(l + "\n" for l in lines), capture_output=True, text=True, env=env, timeout=120)
        assert r.returncode == 0, r.stderr[-3000:]
        return r.stdout
    return run


def model(devices, steps):
    """the table applied to a walk: per step [accepted, phases ..., counts of the devices' slots ..., sum of all slots]"""
    phase = [IDLE] * len(devices); slot = {}; count_at = [None] * len(devices); out = []
    for op, k in steps:
        hit = TABLE.get((op, phase[k]))
        if hit:
            if op == "b":
                count_at[k] = devices[k] % 64                      # the slot begin counted on is the one the later transitions give back
            phase[k] = hit[0]; slot[count_at[k]] = slot.get(count_at[k], 0) + hit[1]
        out += [1 if hit else 0] + phase + [slot.get(d % 64, 0) for d in devices] + [sum(slot.values())]
    return out


def walks(ask, devices, walks_):
    lines = ["walk %d %d %d " % tuple(devices) + " ".join("%s%d" % s for s in w) for w in walks_]
    got = [[int(x) for x in l.split()] for l in ask(lines).splitlines()]
    assert len(got) == len(walks_)
    for w, g in zip(walks_, got):
        assert g == model(devices, w), (devices, w)
    return got


def test_legal_walks_return_the_count_to_zero(ask):
    legal = [[("b", 0), ("e", 0)], [("b", 0), ("c", 0), ("r", 0)], [("b", 0), ("a", 0)], [("b", 0), ("c", 0), ("a", 0)]]
    for g in walks(ask, (0, 0, 0), legal + [w + w for w in legal]):
        assert all(g[8 * i] == 1 for i in range(len(g) // 8))                 # every step accepted
        assert max(g[4::8]) == 1 and g[-8:] == [1, IDLE, IDLE, IDLE, 0, 0, 0, 0]


def test_wrong_phase_is_refused_and_changes_nothing(ask):
    reach = {IDLE: [], OPEN: [("b", 0)], CHAINED: [("b", 0), ("c", 0)]}
    cases = [(ph, op) for ph in reach for op in OPS if (op, ph) not in TABLE]
    assert len(cases) == 5 * 3 - len(TABLE) and ("a", IDLE) in [(op, ph) for ph, op in cases]      # abandon from IDLE among them: a no-op
    got = walks(ask, (3, 3, 3), [reach[ph] + [(op, 0)] for ph, op in cases])
    for (ph, op), g in zip(cases, got):
        before = g[-16:-8] if reach[ph] else [1, IDLE, IDLE, IDLE, 0, 0, 0, 0]
        assert g[-8] == 0 and g[-7:] == before[1:] and g[-7] == ph, (ph, op, g)


def test_handles_on_one_slot_count_independently(ask):
    """two and three handles: every order of beginning, every mix of chained and plain, every closing order"""
    ws = []
    for n in (2, 3):
        for chained in itertools.product((False, True), repeat=n):
            for order in itertools.permutations(range(n)):
                w = [("b", k) for k in range(n)] + [("c", k) for k in range(n) if chained[k]]
                ws.append(w + [("r" if chained[k] else "e", k) for k in order])
                ws.append(w + [("a", k) for k in order])
    for w, g in zip(ws, walks(ask, (7, 7, 7), ws)):
        n = sum(1 for op, _ in w if op == "b")
        assert g[8 * (n - 1) + 4] == n and g[-8:] == [1, IDLE, IDLE, IDLE, 0, 0, 0, 0], w


def test_devices_share_a_slot_modulo_64(ask):
    g = walks(ask, (1, 65, 2), [[("b", 0), ("b", 1), ("b", 2), ("e", 0), ("c", 1), ("a", 2), ("r", 1)]])[0]
    rows = [g[8 * i:8 * i + 8] for i in range(7)]
    assert [r[4:] for r in rows] == [[1, 1, 0, 1], [2, 2, 0, 2], [2, 2, 1, 3], [1, 1, 1, 2], [1, 1, 1, 2], [1, 1, 0, 1], [0, 0, 0, 0]]


def test_every_sequence_up_to_six_steps_over_two_handles(ask):
    """all 10 + 100 + ... + 10^6 sequences of the five transitions on two handles of one slot: after every step the transition was
    accepted exactly where the table has it, the phases are the table's, and the count is the number of handles that are not IDLE"""
    nxt = np.full((5, 3), -1, np.int64)
    for (op, ph), (to, _) in TABLE.items():
        nxt[OPS.index(op), ph] = to
    for L in range(1, 7):
        got = np.array(ask(["enum %d" % L]).split(), dtype=np.int64).reshape(10 ** L, L)
        q = np.arange(10 ** L, dtype=np.int64)
        ph = [np.zeros(10 ** L, np.int64), np.zeros(10 ** L, np.int64)]
        for i in range(L):
            d = q // 10 ** (L - 1 - i) % 10
            h, op = d // 5, d % 5
            ok = np.zeros(10 ** L, np.int64)
            for k in (0, 1):
                to = nxt[op, ph[k]]
                take = (h == k) & (to >= 0)
                ph[k] = np.where(take, to, ph[k]); ok |= take
            count = (ph[0] != IDLE).astype(np.int64) + (ph[1] != IDLE)
            assert np.array_equal(got[:, i], ok * 1000 + ph[0] * 100 + ph[1] * 10 + count), (L, i)
