#!/usr/bin/env python3
"""Pipelined ms/pulse of rts_trace_pulse_end_patterns against rts_trace_pulse_end_uniform on BASELINE configs[2] (bench.py's c3
scene), alternated block by block in ONE process on the same handles, so that both see the same clocks and the same tile history.
Three handles share the scene; pulse k is begun on handle k % 3 (after its previous pulse's group table was collected) and
pulse k - 1 is then ended with the fused call -- one pulse's post-processing running while the others trace.  The target moves
every pulse.  Patterns: a 33 x 17 grid transmitter beam, separable receivers with rotation rates, a 21 x 9 grid RCS.
    python tools/pattern_pulse_bench.py [pulses_per_block] [rounds]
Prints one line per block and a JSON summary (median and range of each mode's blocks)."""
import json
import math
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from rts_amd import api, scenes  # noqa: E402
import rts_amd._lib  # noqa: E402
rts_amd._lib.require_built()        # a timed tool never builds, and never measures a stale library

per_block = int(sys.argv[1]) if len(sys.argv) > 1 else 64
rounds = int(sys.argv[2]) if len(sys.argv) > 2 else 4
spec = scenes.config3(rx_radius=50.0)
tx = spec["tx"]; n_rx = len(spec["rx"]); cs, fc = spec["c"], spec["carrier"]; wl = cs / fc
pos = np.array([r["centre"] for r in spec["rx"]])
rng = np.random.default_rng(3)
g_tx = rng.uniform(0.2, 1.5, (17, 33)); g_tx[:, -1] = g_tx[:, 0]
P = api.Pattern
p_tx = P.grid(g_tx, -math.pi, 2 * math.pi / 32, -math.pi / 2, math.pi / 16, scale=1.3)
p_rx = [P.separable(np.linspace(-math.pi, math.pi, 12), rng.uniform(0.3, 2.0, 12), np.linspace(-1.5, 1.5, 7), rng.uniform(0.3, 2.0, 7), abs_u=k % 2 == 0)
        for k in range(n_rx)]
p_rcs = [P.grid(rng.uniform(0.5, 4.0, (9, 21)), -math.pi, 2 * math.pi / 20, -math.pi / 2, math.pi / 8)]
rot = np.array([[0.3 - 0.2 * k, 0.01 * k, 2.0e3, -1.0e3] for k in range(n_rx)])

hs = [api.Tracer(spec["W"], spec["max_refl"], 0, spec["smooth"]) for _ in range(3)]
hs[0].set_scene(spec["meshes"])
for t in hs[1:]:
    t.share_scene(hs[0])
for t in hs:
    t.set_receivers(spec["rx"]); t.reserve(); t.set_patterns(p_tx, p_rx, p_rcs)


def motion(k):
    return [dict(position=tuple(np.add(m["position"], (0.2 * (k % 64), 0.02 * (k % 64), 0.0))), velocity=m["velocity"]) for m in spec["motion"]]


k_next = [0]


def block(mode, n):
    """n pulses through the three handles; returns ms per pulse (wall clock, the pipeline drained at both ends)"""
    def end(t, k):
        if mode == "uniform":
            t.trace_end_uniform(None, wl, 1.0, 1.0, fc, cs)
        else:
            r = rot.copy(); r[:, 0] += 1e-3 * k
            t.trace_end_patterns(pos, r, wl, fc, cs)
    posted = {}; last = None; recv = 0
    t0 = time.perf_counter()
    for i in range(n):
        k = k_next[0]; k_next[0] += 1
        t = hs[k % 3]
        if t in posted:
            recv += len(t.groups()); del posted[t]
        t.trace_begin(tx["origin"], tx["span"], tx["dir"], motion(k))
        if last is not None:
            end(*last); posted[last[0]] = last[1]
        last = (t, k)
    end(*last); posted[last[0]] = last[1]
    for t in list(posted):
        recv += len(t.groups())
    return (time.perf_counter() - t0) * 1e3 / n, recv


block("uniform", per_block); block("patterns", per_block)          # warm-up: allocations, tile history, speculation history
res = {"uniform": [], "patterns": []}
for r in range(rounds):
    for mode in (("uniform", "patterns") if r % 2 == 0 else ("patterns", "uniform")):
        ms, groups = block(mode, per_block)
        res[mode].append(ms)
        print("round %d %-8s %.4f ms/pulse (%d groups)" % (r, mode, ms, groups), flush=True)
summary = {m: dict(median=float(np.median(v)), min=float(np.min(v)), max=float(np.max(v)), blocks=[round(x, 4) for x in v]) for m, v in res.items()}
summary["ratio_patterns_over_uniform"] = summary["patterns"]["median"] / summary["uniform"]["median"]
summary["config"] = "BASELINE configs[2] (%s, W=%d), 3 handles, %d pulses x %d blocks per mode" % (spec["name"], spec["W"], per_block, rounds)
print(json.dumps(summary))
for t in hs:
    t.close()
