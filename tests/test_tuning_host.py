"""The library's RTS_* environment switches (rts_amd/csrc/rts_tuning.h: the records, the table, the readers) without a GPU:
tests/tuning/tuning_main.cpp includes the header alone, is built with g++ under AddressSanitizer + UndefinedBehaviorSanitizer
(without them where g++ has no libasan, as tests/test_sanitizers.py probes), serves the readers from the NAME=VALUE pairs of a
line and prints every field of every record.  Every expectation here is a literal written out from the one-liners the table
replaced (rts_create, rts_set_scene, rts_lbvh_build_device as they read the environment before) -- defaults, rules and the C
library's atoi / atof / strtoull on these very strings -- never the header's own table or member initialisers."""
import math
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "rts_amd", "csrc")
STACK_LDS = 24                                        # RTS_STACK_LDS
U64_MAX = 2 ** 64 - 1
KEEP = None                                           # the switch is set and the field keeps its default

# every field of the four records (t: a handle's, s: a scene's, p: the process's, l: a launch's) with nothing set
DEFAULTS = {
    "t.use_pmask": 1, "t.grid_mult": 4, "t.grid_spare": 160, "t.grid_spare_forced": 0, "t.tile_lpt": 1, "t.ew_rel": 2.0 ** -49,
    "t.stack_lds": STACK_LDS, "t.rx_window_screen": 1, "t.batch_dead": 1, "t.node_versions": 1, "t.share_history": 1,
    "t.trace_own_stream": 1, "t.spin_wait": 1, "t.coop_frac": 0.5, "t.coop_floor": 7500, "t.coop_walk_steps": 1000,
    "t.coop_walk_steps_lo": 400, "t.coop_mid": 1.5, "t.coop_big": 0.0, "t.coop_big_part": 1.5, "t.coop_spread": 1,
    "t.coop_grid_max": 1024, "t.coop_versions": 1, "t.post_small": 1, "t.post_one_max": 1024, "t.post_prio": 3, "t.spec_enabled": 1,
    "t.img_split_below": 1024, "t.beat_force_parts": 0, "t.timeline_blocks": 0, "t.debug_coop": 0,
    "s.device_build": 1, "s.split_budget": 2.0, "s.build_fallback": 1, "s.fail_device_build": 0, "s.node_versions": 1,
    "s.version_key_centre": 1, "s.sah_tree": 1, "s.crowd_rounds": 0, "s.ref_gain_rule": 1, "s.debug_build": 0,
    "p.lap": 0, "p.debug_sync": 0, "l.timeline": "(null)",
}

# the four spellings of a flag, each over the same strings (and a few of its own)
NOT_0 = {"": 1, "0": 0, "00": 0, "1": 1, "yes": 1, " 1": 1, "no": 1, " 0": 1, "0x": 0}          # e[0] != '0'
NONZERO = {"": 0, "0": 0, "00": 0, "1": 1, "yes": 0, " 1": 1, "2": 1, "-1": 1, "1x": 1, " 0": 0}   # atoi(e) != 0
IS_1 = {"": 0, "0": 0, "00": 0, "1": 1, "yes": 0, " 1": 0, "10": 1, "2": 0}                       # e[0] == '1'
PRESENT = {"": 1, "0": 1, "00": 1, "1": 1, "yes": 1, " 1": 1}                                     # getenv(...) != nullptr
FLOOR_0 = {"0": 0, "-1": 0, "": 0, "abc": 0}                                                       # max(0, atoi(e)) at its edges

# (name, scope, field, {value: what the field holds then -- KEEP: its default -- or {field: value} where more than one moves})
SWITCHES = [
    ("RTS_PRIMARY_MASK", "handle", "t.use_pmask", NOT_0),
    ("RTS_GRID_MULT", "handle", "t.grid_mult", {"1": 1, "8": 8, "0": 1, "-3": 1, "": 1, "abc": 1, " 6": 6, "2x": 2}),
    ("RTS_GRID_SPARE", "handle", "t.grid_spare", {v: {"t.grid_spare": n, "t.grid_spare_forced": 1}
                                                  for v, n in {"160": 160, "0": 0, "256": 256, "-1": 0, "": 0, "abc": 0}.items()}),
    ("RTS_TILE_LPT", "handle", "t.tile_lpt", NOT_0),
    ("RTS_COOP_BIG_PART", "handle", "t.coop_big_part", {"0": 0.0, "2.5": 2.5, "-1": KEEP, "": 0.0, "abc": 0.0, "nan": KEEP}),
    ("RTS_COOP_FRAC", "handle", "t.coop_frac", {"0": 0.0, "1e-12": 1e-12, "0.25": 0.25, "-1": KEEP, "-1e-300": KEEP, "": 0.0, "abc": 0.0,
                                               "nan": KEEP, "inf": math.inf}),
    ("RTS_COOP_FLOOR", "handle", "t.coop_floor", dict(FLOOR_0, **{"7500": 7500, "100000": 100000})),
    ("RTS_DEBUG_COOP", "handle", "t.debug_coop", PRESENT),
    ("RTS_SHARE_HISTORY", "handle", "t.share_history", NOT_0),
    ("RTS_RX_WINDOW_SCREEN", "handle", "t.rx_window_screen", NOT_0),
    ("RTS_TIMELINE_BLOCKS", "handle", "t.timeline_blocks", NOT_0),
    ("RTS_COOP_VERSIONS", "handle", "t.coop_versions", NOT_0),
    ("RTS_DEAD_BATCH", "handle", "t.batch_dead", {"all": 2, "0": 0, "1": 1, "": 1, "00": 0, "yes": 1, " 1": 1, "ALL": 1, "all ": 1, "al": 1}),
    ("RTS_WALK_VERSIONS", "handle", "t.node_versions", NOT_0),
    ("RTS_SPIN_WAIT", "handle", "t.spin_wait", NONZERO),
    ("RTS_TRACE_OWN_STREAM", "handle", "t.trace_own_stream", NONZERO),
    ("RTS_SPECULATE", "handle", "t.spec_enabled", NONZERO),
    ("RTS_POST_SMALL", "handle", "t.post_small", NONZERO),
    ("RTS_POST_ONE_MAX", "handle", "t.post_one_max", {"0": 0, "1024": 1024, "4096": 4096, "": 0, "abc": 0, "18446744073709551615": U64_MAX,
                                                     "-1": U64_MAX, " 7": 7, "12x": 12}),
    ("RTS_IMAGE_SPLIT_BELOW", "handle", "t.img_split_below", dict(FLOOR_0, **{"65536": 65536, "70000": 65536, "65537": 65536, "1024": 1024})),
    ("RTS_BEAT_PARTS", "handle", "t.beat_force_parts", dict(FLOOR_0, **{"1": 1, "64": 64, "65": 64})),
    ("RTS_POST_PRIO", "handle", "t.post_prio", dict(FLOOR_0, **{"3": 3, "9": 3, "4": 3, "2": 2})),
    ("RTS_COOP_STEPS", "handle", "t.coop_walk_steps", dict(FLOOR_0, **{"500": 500, "1000": 1000})),
    ("RTS_COOP_STEPS_LO", "handle", "t.coop_walk_steps_lo", dict(FLOOR_0, **{"200": 200, "400": 400})),
    ("RTS_COOP_MID", "handle", "t.coop_mid", {"3": 3.0, "1.5": 1.5, "0": 0.0, "-1": 0.0, "": 0.0, "abc": 0.0, "nan": 0.0}),
    ("RTS_COOP_SEG", "handle", "t.coop_walk_steps", {"0": 0, "1": KEEP, "": 0, "abc": 0, "00": 0, " 1": KEEP, "2": KEEP}),
    ("RTS_COOP_BIG", "handle", "t.coop_big", {"0.8": 0.8, "1.3": 1.3, "0": 0.0, "-2": 0.0, "": 0.0, "abc": 0.0, "nan": 0.0}),
    ("RTS_COOP_SPREAD", "handle", "t.coop_spread", {"1": 1, "2": 2, "4": 4, "8": 8, "3": KEEP, "0": KEEP, "16": KEEP, "32": KEEP, "33": KEEP,
                                                   "-2": KEEP, "": KEEP, "abc": KEEP}),
    ("RTS_COOP_GRID", "handle", "t.coop_grid_max", {"0": 1, "5000": 4096, "1": 1, "4096": 4096, "4097": 4096, "256": 256, "-1": 1, "": 1, "abc": 1}),
    ("RTS_EW_REL", "handle", "t.ew_rel", {"1e-12": 1e-12, "1e-300": 1e-300, "0": KEEP, "-1": KEEP, "": KEEP, "abc": KEEP, "nan": KEEP}),
    ("RTS_STACK_LDS_DEBUG", "handle", "t.stack_lds", {"2": 2, "3": 3, "1": 1, str(STACK_LDS): STACK_LDS, "0": KEEP, str(STACK_LDS + 1): KEEP,
                                                     "-1": KEEP, "": KEEP, "abc": KEEP}),
    ("RTS_BUILDER", "scene", "s.device_build", {"host": 0, "device": 1, "": 1, "HOST": 1, "host ": 1, "0": 1}),
    ("RTS_SPLIT_BUDGET", "scene", "s.split_budget", {"0": 0.0, "2": 2.0, "8": 8.0, "9": KEEP, "8.0001": KEEP, "-0.5": KEEP, "": 0.0, "abc": 0.0,
                                                    "nan": KEEP}),
    ("RTS_DEBUG_FAIL_DEVICE_BUILD", "scene", "s.fail_device_build", PRESENT),
    ("RTS_DEVICE_BUILD_FALLBACK", "scene", "s.build_fallback", NOT_0),
    ("RTS_NODE_VERSIONS", "scene", "s.node_versions", NOT_0),
    ("RTS_VERSION_KEY", "scene", "s.version_key_centre", {"corner": 0, "centre": 1, "": 1, "Corner": 1, "corner ": 1, "0": 1}),
    ("RTS_DEVICE_TREE", "scene", "s.sah_tree", {"lbvh": 0, "sah": 1, "": 1, "LBVH": 1, "0": 1}),
    ("RTS_CROWD_ROUNDS", "scene", "s.crowd_rounds", dict(FLOOR_0, **{"1": 1, "2": 2, "3": 3, "4": 3})),
    ("RTS_REF_GAIN_RULE", "scene", "s.ref_gain_rule", NONZERO),
    ("RTS_DEBUG_BUILD", "scene", "s.debug_build", PRESENT),
    ("RTS_LAP", "process", "p.lap", IS_1),
    ("RTS_DEBUG_SYNC", "process", "p.debug_sync", IS_1),
    ("RTS_TIMELINE", "launch", "l.timeline", {"/tmp/timeline.bin": "/tmp/timeline.bin", "": "", "a b": "a b", "x": "x"}),
]
NAMES = [s[0] for s in SWITCHES]


def expected(pairs, host_build=False):
    """the records after the switches of `pairs` (in the order the library reads them, which is SWITCHES')"""
    want = dict(DEFAULTS)
    if host_build:
        want["s.device_build"] = 0
    for name, _, field, cases in SWITCHES:
        if name in pairs:
            effect = cases[pairs[name]]
            if effect is not KEEP:
                want.update(effect if isinstance(effect, dict) else {field: effect})
    return want


@pytest.fixture(scope="module")
def tuning(tmp_path_factory):
    gxx = shutil.which("g++")
    if not gxx:
        pytest.skip("no g++")
    rt = subprocess.run([gxx, "-print-file-name=libasan.so"], capture_output=True, text=True).stdout.strip()
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"] if os.path.isabs(rt) and os.path.exists(rt) else []
    exe = str(tmp_path_factory.mktemp("tuning") / "tuning_main")
    subprocess.check_call([gxx, "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror"] + san + ["-I", CSRC,
                           os.path.join(ROOT, "tests", "tuning", "tuning_main.cpp"), "-o", exe])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:verify_asan_link_order=0", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")

    def run(text):
        r = subprocess.run([exe], input=text, capture_output=True, text=True, env=env, timeout=120)
        assert r.returncode == 0, r.stderr[-3000:]
        return [block.splitlines() for block in r.stdout.split(".\n")[:-1]]

    def ask(cases):
        """cases: (pairs, host_build) -> one {record.field: value} per case"""
        for pairs, _ in cases:
            assert not any(c in v for v in pairs.values() for c in "\t\n")
        blocks = run("".join("\t".join((["@host_build"] if hb else []) + ["%s=%s" % kv for kv in pairs.items()]) + "\n" for pairs, hb in cases))
        assert len(blocks) == len(cases)
        out = []
        for block in blocks:
            rec = {}
            for line in block:
                key, _, val = line.partition(" ")
                if key != "l.timeline":
                    try:
                        val = int(val)
                    except ValueError:
                        val = float(val)
                rec[key] = val
            out.append(rec)
        return out
    ask.table = lambda: [tuple(line.split()) for line in run("!table\n")[0]]
    return ask


def test_the_table_is_the_44_switches_in_reading_order(tuning):
    assert len(SWITCHES) == 44 and len(set(NAMES)) == 44
    assert tuning.table() == [(name, scope) for name, scope, _, _ in SWITCHES]
    assert NAMES.index("RTS_COOP_STEPS") < NAMES.index("RTS_COOP_SEG")
    assert {s[2] for s in SWITCHES} | {"t.grid_spare_forced"} == set(DEFAULTS)      # every field has its switch


def test_nothing_set_gives_the_defaults(tuning):
    assert tuning([({}, False)]) == [DEFAULTS]
    assert tuning([({}, True)]) == [dict(DEFAULTS, **{"s.device_build": 0})]       # RTS_FLAG_HOST_BUILD
    assert tuning([({"RTS_UNKNOWN": "1", "RTS_XCD_AFFINE": "1", "RTS_TILE_SORT": "1"}, False)]) == [DEFAULTS]


def test_every_switch_alone_every_value(tuning):
    """the values the tests and tools set, each edge of the switch's rule, text that is no number -- and every other field of every
    record at its default, for all 44"""
    cases = [({name: value}, False) for name, _, _, values in SWITCHES for value in values]
    got = tuning(cases)
    seen = set()
    for (pairs, _), rec in zip(cases, got):
        assert rec == expected(pairs), pairs
        seen |= set(pairs)
    assert seen == set(NAMES)
    for name, _, field, values in SWITCHES:                           # the table above moves every field somewhere
        assert any(expected({name: v}) != DEFAULTS for v in values), name
    used = {"RTS_COOP_FRAC": "1e-12", "RTS_STACK_LDS_DEBUG": "2", "RTS_DEAD_BATCH": "all", "RTS_BEAT_PARTS": "64", "RTS_GRID_MULT": "1",
            "RTS_COOP_FLOOR": "0", "RTS_COOP_SEG": "0", "RTS_SPECULATE": "0", "RTS_IMAGE_SPLIT_BELOW": "65536", "RTS_BUILDER": "host",
            "RTS_VERSION_KEY": "corner", "RTS_SPLIT_BUDGET": "0", "RTS_TILE_LPT": "0", "RTS_TIMELINE_BLOCKS": "1"}
    for name, value in used.items():
        assert value in SWITCHES[NAMES.index(name)][3], name


def test_rules_are_not_normalised(tuning):
    """`yes` is off for an integer flag and on for a first-character flag; a leading space is skipped by the one and seen by the other"""
    got = tuning([({"RTS_SPIN_WAIT": "yes", "RTS_SHARE_HISTORY": "yes", "RTS_LAP": "yes"}, False),
                  ({"RTS_SPIN_WAIT": " 1", "RTS_SHARE_HISTORY": " 0", "RTS_LAP": " 1"}, False)])
    assert [(g["t.spin_wait"], g["t.share_history"], g["p.lap"]) for g in got] == [(0, 1, 0), (1, 1, 0)]


def test_interactions(tuning):
    cases = [({"RTS_COOP_STEPS": "500", "RTS_COOP_SEG": "0"}, False), ({"RTS_COOP_SEG": "0", "RTS_COOP_STEPS": "500"}, False),
             ({"RTS_COOP_STEPS": "500", "RTS_COOP_SEG": "1"}, False), ({"RTS_COOP_SEG": "1"}, False),
             ({"RTS_GRID_SPARE": "160"}, False),
             ({"RTS_BUILDER": "device"}, True), ({"RTS_BUILDER": "host"}, True), ({"RTS_BUILDER": "host"}, False),
             ({"RTS_NODE_VERSIONS": "0"}, False), ({"RTS_WALK_VERSIONS": "0"}, False),
             ({name: {"RTS_TIMELINE": "x"}.get(name, "0") for name in NAMES}, False)]
    got = tuning(cases)
    for (pairs, hb), rec in zip(cases, got):
        assert rec == expected(pairs, hb), pairs
    assert [g["t.coop_walk_steps"] for g in got[:4]] == [0, 0, 500, 1000]        # the alias wins whichever way the caller wrote them
    assert (got[4]["t.grid_spare"], got[4]["t.grid_spare_forced"]) == (160, 1) and got[4] != DEFAULTS
    assert [g["s.device_build"] for g in got[5:8]] == [1, 0, 0]
    assert (got[8]["s.node_versions"], got[8]["t.node_versions"], got[9]["s.node_versions"], got[9]["t.node_versions"]) == (0, 1, 1, 0)
    everything_0 = got[10]
    assert everything_0["t.batch_dead"] == 0 and everything_0["t.coop_spread"] == 1 and everything_0["t.stack_lds"] == STACK_LDS
    assert everything_0["t.debug_coop"] == 1 and everything_0["s.device_build"] == 1 and everything_0["t.coop_grid_max"] == 1


def test_the_environment_is_read_in_one_place():
    """getenv appears in the library's sources once, in the lookup that rts_api.hip hands to the readers, and every reader call
    is given that lookup"""
    hits, reads = [], []
    for fn in sorted(os.listdir(CSRC)):
        if fn.endswith((".hip", ".cpp", ".h")):
            with open(os.path.join(CSRC, fn)) as f:
                for line in f:
                    if re.search(r"\bgetenv\b", line):
                        hits.append((fn, line.strip()))
                    if fn != "rts_tuning.h":
                        reads += [(fn, m) for m in re.findall(r"\brts_tuning_read\(([^)]*)\)", line)]
    assert hits == [("rts_api.hip", "const char* rts_env(const char* name) { return getenv(name); }")]
    assert len(reads) == 4 and all(args.endswith(", rts_env") for fn, args in reads), reads
    assert sorted(fn for fn, _ in reads) == ["rts_api.hip"] * 3 + ["rts_scene.hip"]                 # (the scene's switches: rts_set_scene)


def test_integration_md_lists_exactly_these_switches():
    with open(os.path.join(ROOT, "INTEGRATION.md")) as f:
        text = f.read()
    section = text.split("### Environment switches", 1)[1].split("\n#", 1)[0]
    rows = re.findall(r"^\| `(RTS_[A-Z0-9_]+)` \| (\w+) \|", section, re.M)
    assert sorted(rows) == sorted((name, scope) for name, scope, _, _ in SWITCHES)
    assert set(re.findall(r"`(RTS_[A-Z0-9_]+)=", text)) <= set(NAMES)            # no switch is described that the library does not read
