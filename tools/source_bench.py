#!/usr/bin/env python3
"""Cost of the clutter and jammer sources (rts_cube_add_sources: k_cube_sources) on a cube of 8 receivers x 256 pulses x 4 096 bins:
  * 360 patches, rho all 1   (ground clutter: no draw after pulse 0)
  * 360 patches, rho all 0.9 (clutter with internal motion: one draw per patch, bin and pulse)
  * 1 patch, rho 0           (a noise jammer)
Each call is timed on its own by the host clock between two device synchronisations (the handle's stream is the library's own, so
the tool cannot put events on it); the figure is the median of `reps` calls after `warmup` calls, with the spread (min .. max).  A
call is the staged upload of its table and the kernel behind it.
Two floors, measured in the same run and the same way:
  * memory: a device-to-device copy of twice the cube's bytes (the call reads and writes every sample once);
  * arithmetic: the f64 multiplies and adds the header's rules NEED -- per bin and pulse 6 per patch for the turn by the pole, 4 more
    per patch that draws, per receiver 8 per patch for the term and its sum and 126 for the tree of 64 partials -- over the rate at
    which this device issues uncontracted f64 multiplies and adds (tools/f64_rate, built from tools/f64_rate.hip; without the binary
    the nominal 256 CUs x 4 SIMDs x 16 lanes x 2.4 GHz is used and said so).  The draws' own work (Philox, log, sqrt, cos, sin) is
    NOT in this count: the floor is a floor.
    python tools/source_bench.py [reps] [warmup] [--out FILE]
Prints one line per measurement and a JSON summary (also written to FILE)."""
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

args = sys.argv[1:]
out_path = None
if "--out" in args:
    k = args.index("--out"); out_path = args[k + 1]; del args[k:k + 2]
reps = int(args[0]) if args else 20
warmup = int(args[1]) if len(args) > 1 else 5

# the f64 rate first, in a child process of its own (this process has not touched the device yet)
rate, rate_source = 256 * 4 * 16 * 2.4e9, "nominal: 256 CUs x 4 SIMDs x 16 lanes x 2.4 GHz"
calib = os.path.join(ROOT, "tools", "f64_rate")
if os.path.exists(calib):
    r = subprocess.run([calib], capture_output=True, text=True, timeout=120)
    if r.returncode == 0:
        rate, rate_source = float(r.stdout.split()[0]), "measured: " + r.stdout.strip()

import torch  # noqa: E402  (before the library: one HIP runtime serves both; torch.cuda.synchronize drains the handle's stream)
from rts_amd import api  # noqa: E402
import rts_amd._lib  # noqa: E402
rts_amd._lib.require_built()        # a timed tool never builds, and never measures a stale library


def timed(fn):
    """ms per call: (median, min, max) of `reps` calls after `warmup`"""
    ms = []
    for i in range(warmup + reps):
        torch.cuda.synchronize()
        a = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        if i >= warmup:
            ms.append((time.perf_counter() - a) * 1e3)
    return float(np.median(ms)), float(min(ms)), float(max(ms))


n_rx, n_p, nb = 8, 256, 4096
rng = np.random.default_rng(7)
cube = torch.zeros((n_rx, n_p, nb), dtype=torch.complex128, device="cuda")
src = torch.zeros(2 * n_rx * n_p * nb, dtype=torch.float64, device="cuda"); dst = torch.empty_like(src)      # the cube's bytes: read + written = twice
torch.cuda.synchronize()
t = api.Tracer(8, 1)
t.cube_attach(n_rx, n_p, nb, 0.0, 1.0, device_ptr=cube.data_ptr())
copy = timed(lambda: dst.copy_(src, non_blocking=True))
summary = {"reps": reps, "warmup": warmup, "cube": [n_rx, n_p, nb], "copy_ms": copy, "f64_ops_per_s": rate, "f64_rate_source": rate_source, "cases": []}
print("device-to-device copy of twice the cube's bytes (%d MB moved): %.4f ms (%.4f .. %.4f)" % (2 * 16 * n_rx * n_p * nb // 10 ** 6, copy[0], copy[1], copy[2]), flush=True)
print("f64 multiply / add rate: %.3e per s (%s)" % (rate, rate_source), flush=True)
for name, K, rho in (("clutter, rho 1", 360, 1.0), ("clutter, rho 0.9", 360, 0.9), ("jammer, rho 0", 1, 0.0)):
    sp = rng.standard_normal((K, n_rx)) + 1j * rng.standard_normal((K, n_rx))
    power, doppler = rng.uniform(0.5, 2.0, K), rng.uniform(-0.5, 0.5, K)
    cube.zero_(); torch.cuda.synchronize()
    ms = timed(lambda: t.cube_add_sources(sp, power, doppler, rho=np.full(K, rho), seed=7))
    draws = K if rho < 1.0 else 0
    ops = float(nb) * n_p * (6 * K + 4 * draws + n_rx * (8 * K + 126))
    floor = ops / rate * 1e3
    rec = {"name": name, "n_patches": K, "rho": rho, "ms": ms, "f64_ops": ops, "f64_floor_ms": floor, "over_copy": ms[0] / copy[0], "over_f64_floor": ms[0] / floor,
           "draws": float(nb) * n_p * draws + float(nb) * K}
    summary["cases"].append(rec)
    print("%-17s K = %3d: %.4f ms (%.4f .. %.4f);  %.2f x the copy;  f64 floor %.4f ms (%.3g operations), %.2f x the floor;  %.3g draws" %
          (name, K, ms[0], ms[1], ms[2], rec["over_copy"], floor, ops, rec["over_f64_floor"], rec["draws"]), flush=True)
t.close()
summary["build_id"] = rts_amd._lib.build_id()
line = json.dumps(summary)
print(line)
if out_path:
    with open(out_path, "w") as f:
        f.write(line + "\n")
