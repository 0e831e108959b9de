#!/usr/bin/env python3
"""Cost of the FMCW products (rts_cube_render_beat, rts_cube_range_transform) on the scene bench.py times by default (BASELINE
configs[2]: scenes.config3(), 4 receivers):
  * per-pulse beat render time, rays and paths, at 1 024 and 4 096 samples per row, in isolation: `reps` renders of one finalised,
    aggregated pulse, timed by the host clock up to a device synchronise.  The rows start after the last echo has arrived and end
    before the chirp does, so every contribution reaches every sample: the render's worst case
  * for scale, the same pulse's rts_cube_render (256-sample LFM, L = 16) into rows of the same lengths, and its trace time
  * the range transform of a 256-pulse x 4 096-sample cube (n_fft 4 096, Hann, all bins), the same way
with the operation counts of the beat render (complex multiply-adds: contributions kept x samples, two per sample: the term and the
rotation) beside its times.
    python tools/beat_bench.py [reps] [--out FILE]
Prints one line per measurement and a JSON summary (also written to FILE).  Kernel times: run it under rocprofv3 --kernel-trace --stats."""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402  (before the library: one HIP runtime serves both; torch.cuda.synchronize drains the handle's stream)
from rts_amd import api, scenes  # noqa: E402
import rts_amd._lib  # noqa: E402
rts_amd._lib.require_built()        # a timed tool never builds, and never measures a stale library

args = sys.argv[1:]
out_path = None
if "--out" in args:
    k = args.index("--out"); out_path = args[k + 1]; del args[k:k + 2]
reps = int(args[0]) if args else 200
N_PULSES, M, TAPS, BDT = 256, 256, 16, 0.8
spec = scenes.config3()
tx = spec["tx"]; n_rx = len(spec["rx"]); cs, fc = spec["c"], spec["carrier"]; wl = cs / fc

t = api.Tracer(spec["W"], spec["max_refl"], 0, spec["smooth"])
t.set_scene(spec["meshes"]); t.set_receivers(spec["rx"]); t.reserve()
t.trace(tx["origin"], tx["span"], tx["dir"], spec["motion"], want_stats=False)       # warm-up: allocations, tile history
trace_ms = [t.trace(tx["origin"], tx["span"], tx["dir"], spec["motion"])["ms_trace"] for _ in range(5)]
t.finalise_uniform(None, wl, 1.0, 1.0, fc, cs)
resp = api.groups_to_responses(t.aggregate(cs, fc))
recv = t.received_count()
per_rx = np.bincount(t.received()["results"]["received"], minlength=n_rx)
per_rx_paths = np.bincount(resp["rx"], minlength=n_rx)
dmin, dmax = float(resp["delay"].min()), float(resp["delay"].max())
print("scene %s W=%d: %d received rays, %d responses, delays %.4e .. %.4e s; trace %.3f ms (median of 5)" %
      (spec["name"], spec["W"], recv, len(resp), dmin, dmax, float(np.median(trace_ms))), flush=True)
summary = {"reps": reps, "scene": spec["name"], "W": spec["W"], "n_rx": n_rx, "received_rays": int(recv), "responses": int(len(resp)),
           "trace_ms_median": float(np.median(trace_ms))}


def timed(fn, n):
    """ms per call of n calls up to a device synchronise, after one warm-up call"""
    fn(); torch.cuda.synchronize()
    a = time.perf_counter()
    for _ in range(n):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - a) * 1e3 / n


wave = api.Waveform.lfm(M, BDT, TAPS)
t.cube_set_waveform(wave)
for n_bins in (1024, 4096):
    dt = 1.0e-8
    t0 = dmax + dt                                   # every echo has arrived at the first sample
    slope = 0.4 / (dmax * dt)                        # |S tau| dt <= 0.4
    duration = t0 + (n_bins + 1) * dt                # ... and the chirp outlasts the row
    t.cube_attach(n_rx, 2, n_bins, t0, dt)
    for src, kept in (("rays", per_rx), ("paths", per_rx_paths)):
        ms = timed(lambda: t.cube_render_beat(1, slope, duration, src, cs, fc), reps)
        cmadd = 2 * int(kept.sum()) * n_bins
        summary["beat_%s_%d_ms" % (src, n_bins)] = ms
        summary["beat_%s_%d_complex_multiply_adds" % (src, n_bins)] = cmadd
        print("beat render %-5s %4d samples: %.4f ms per pulse (%d contributions kept, %.3g complex multiply-adds, %.3g per s)" %
              (src, n_bins, ms, int(kept.sum()), cmadd, cmadd / (ms * 1e-3)), flush=True)
    # the pulsed render of the same pulse into rows of the same length, its window on the responses (tools/render_bench.py)
    dtr = max((dmax - dmin) / max(n_bins - M - 64, 1), 2.0e-10)
    t.cube_attach(n_rx, 2, n_bins, dmin - 16 * dtr, dtr)
    for src in ("rays", "paths"):
        ms = timed(lambda: t.cube_render(1, src, cs, fc), reps)
        summary["render_%s_%d_ms" % (src, n_bins)] = ms
        print("rts_cube_render %-5s %4d bins (LFM M=%d L=%d): %.4f ms per pulse" % (src, n_bins, M, TAPS, ms), flush=True)

# ---- the range transform of a 256 x 4096 cube
N_BINS = 4096
gen = torch.Generator(device="cuda"); gen.manual_seed(7)
cube = torch.randn((n_rx, N_PULSES, N_BINS), dtype=torch.complex128, device="cuda", generator=gen)
out = torch.zeros((n_rx, N_PULSES, N_BINS), dtype=torch.complex128, device="cuda")
torch.cuda.synchronize()
t.cube_attach(n_rx, N_PULSES, N_BINS, 0.0, 1.0, device_ptr=cube.data_ptr())
w = api.window("hann", N_BINS)
ms = timed(lambda: t.cube_range_transform(N_BINS, window=w, reverse=True, device_ptr=out.data_ptr()), max(reps // 10, 5))
ms_nw = timed(lambda: t.cube_range_transform(N_BINS, reverse=True, device_ptr=out.data_ptr()), max(reps // 10, 5))
moved = 2 * n_rx * N_PULSES * N_BINS * 16
summary["range_%dx%dx%d_hann_ms" % (n_rx, N_PULSES, N_BINS)] = ms
summary["range_%dx%dx%d_no_window_ms" % (n_rx, N_PULSES, N_BINS)] = ms_nw
summary["range_bytes_moved"] = moved
print("range transform %d x %d x %d, n_fft %d: %.4f ms with a Hann window, %.4f ms without (%d bytes read + written: %.3g B/s)" %
      (n_rx, N_PULSES, N_BINS, N_BINS, ms, ms_nw, moved, moved / (ms_nw * 1e-3)), flush=True)
t.close()
summary["build_id"] = rts_amd._lib.build_id()
line = json.dumps(summary)
print(line)
if out_path:
    with open(out_path, "w") as f:
        f.write(line + "\n")
