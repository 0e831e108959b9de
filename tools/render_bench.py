#!/usr/bin/env python3
"""Cost of the received-signal products (rts_cube_render, rts_cube_compress) on the scene bench.py times by default (BASELINE
configs[2]: scenes.config3(), 4 receivers), with a 256-sample LFM (L = 16) and 2 048 range bins:
  * per-pulse render time, rays and paths, in isolation: `reps` renders of one finalised, aggregated pulse, timed by the host
    clock up to a stream synchronise (the rays are the pulse's, carrying their group values after rts_aggregate: the same count)
  * compression of a 256-pulse cube (4 x 256 x 2 048), the same way
  * the pipelined interval (three handles sharing the scene, fused pulse ends, as tools/pattern_pulse_bench.py) without a render,
    and with one paths or rays render per pulse issued when the handle's group table is collected, alternated block by block
    python tools/render_bench.py [pulses_per_block] [rounds] [reps]
Prints one line per measurement and a JSON summary.  Kernel times: run it under rocprofv3 --kernel-trace --stats."""
import json
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
reps = int(sys.argv[3]) if len(sys.argv) > 3 else 200
N_BINS, N_PULSES, M, TAPS, BDT = 2048, 256, 256, 16, 0.8
spec = scenes.config3()
tx = spec["tx"]; n_rx = len(spec["rx"]); cs, fc = spec["c"], spec["carrier"]; wl = cs / fc
wave = api.Waveform.lfm(M, BDT, TAPS)

hs = [api.Tracer(spec["W"], spec["max_refl"], 0, spec["smooth"]) for _ in range(3)]
hs[0].set_scene(spec["meshes"])
for t in hs[1:]:
    t.share_scene(hs[0])
for t in hs:
    t.set_receivers(spec["rx"]); t.reserve(); t.cube_set_waveform(wave)


def motion(k):
    return [dict(position=tuple(np.add(m["position"], (0.2 * (k % 64), 0.02 * (k % 64), 0.0))), velocity=m["velocity"]) for m in spec["motion"]]


# ---- the cube's window from a first pulse: every response inside, M samples of room behind the last
t = hs[0]
t.trace(tx["origin"], tx["span"], tx["dir"], motion(0), want_stats=False); t.finalise_uniform(None, wl, 1.0, 1.0, fc, cs)
resp = api.groups_to_responses(t.aggregate(cs, fc))
dmin, dmax = float(resp["delay"].min()), float(resp["delay"].max())
dt = max((dmax - dmin) / (N_BINS - M - 64), 2.0e-10)
t0 = dmin - 16 * dt
for h in hs:
    h.cube_attach(n_rx, N_PULSES, N_BINS, t0, dt)          # (library-owned, one per handle)
recv = t.received_count()
print("scene %s W=%d: %d received rays, %d responses; dt = %.3e s, t0 = %.6e s" % (spec["name"], spec["W"], recv, len(resp), dt, t0), flush=True)


def sync(h):
    h.cube_set_waveform(wave)          # (drains the handle's stream, then a 4 KB copy)


def timed(fn, n):
    fn(); sync(t)
    a = time.perf_counter()
    for i in range(n):
        fn()
    sync(t)
    return (time.perf_counter() - a) * 1e3 / n


iso = {}
for src in ("rays", "paths"):
    iso["render_%s_ms" % src] = timed(lambda: t.cube_render(1, src, cs, fc), reps)
    print("render %-5s %.4f ms per pulse (%d renders, %d received rays)" % (src, iso["render_%s_ms" % src], reps, recv), flush=True)
iso["compress_256_pulses_ms"] = timed(lambda: t.cube_compress(0, N_PULSES), 5)
print("compress %d x %d x %d: %.4f ms" % (n_rx, N_PULSES, N_BINS, iso["compress_256_pulses_ms"]), flush=True)
k_next = [0]


def block(mode, n):
    """n pulses through the three handles; returns ms per pulse (wall clock, the pipeline drained at both ends)"""
    posted = {}; last = None; groups = 0

    def collect(h):
        nonlocal groups
        groups += len(h.groups())
        if mode != "none":
            h.cube_render(posted[h] % N_PULSES, mode, cs, fc)
        del posted[h]
    a = time.perf_counter()
    for i in range(n):
        k = k_next[0]; k_next[0] += 1
        h = hs[k % 3]
        if h in posted:
            collect(h)
        h.trace_begin(tx["origin"], tx["span"], tx["dir"], motion(k))
        if last is not None:
            last[0].trace_end_uniform(None, wl, 1.0, 1.0, fc, cs); posted[last[0]] = last[1]
        last = (h, k)
    last[0].trace_end_uniform(None, wl, 1.0, 1.0, fc, cs); posted[last[0]] = last[1]
    for h in list(posted):
        collect(h)
    for h in hs:
        sync(h)
    return (time.perf_counter() - a) * 1e3 / n, groups


modes = ("none", "paths", "rays")
for m in modes:
    block(m, per_block)                 # warm-up: allocations, tile history, speculation history
res = {m: [] for m in modes}
for r in range(rounds):
    for m in (modes if r % 2 == 0 else modes[::-1]):
        ms, groups = block(m, per_block)
        res[m].append(ms)
        print("round %d %-5s %.4f ms/pulse (%d groups)" % (r, m, ms, groups), flush=True)
summary = dict(iso)
summary.update({"pipelined_%s" % m: dict(median=float(np.median(v)), min=float(np.min(v)), max=float(np.max(v))) for m, v in res.items()})
summary["config"] = "BASELINE configs[2] (%s, W=%d), %d rx, LFM M=%d L=%d, %d bins, %d received rays, 3 handles, %d pulses x %d blocks per mode" % (
    spec["name"], spec["W"], n_rx, M, TAPS, N_BINS, recv, per_block, rounds)
print(json.dumps(summary))
for h in hs:
    h.close()
