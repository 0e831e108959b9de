#!/usr/bin/env python3
"""Cost of the track-before-detect step (rts_cube_tbd_step: k_tbd_step) at n_rx 8, n_doppler 256, n_bins 4 096, half (1, 2), depth 8,
from a caller's device map, against device-to-device copies in the same process, and of the extraction (rts_cube_tbd_extract:
k_tbd_cand twice and the scan) at 1 000 candidates.
  The step's floor is 33 bytes per cell and frame: 16 read of the map, 8 read and 8 written of merit, 1 written of pointer.  Two
copies stand beside it: of a buffer of 33 bytes per cell (it reads 33 and writes 33: 66 bytes of traffic per cell) and of one of
16.5 bytes per cell (33 bytes of traffic: the step's own floor as a copy).
  The maps: unit-power complex Gaussian noise, two of them taken in turn; n_doppler pri = 1 and delay_rate_per_hz = 0.05, so the
shift table spans -6 .. +6 bins.  The threshold of the extraction is the 1 001st largest merit, without the local-maximum rule.
  Each: `batches` batches of `reps` calls, every batch timed by the host clock between two device synchronisations after a warm-up
batch (`reps` back-to-back calls on one stream hide the launch); ms per call = batch time / reps; the median of the batches
(min .. max).
    python tools/tbd_bench.py [reps] [batches] [--out FILE]
Prints one line per measurement and a JSON summary (also written to FILE).  RTS_AMD_LIB names another build for A/B runs."""
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402  (before the library: one HIP runtime serves both; torch.cuda.synchronize drains the handle's stream)
from rts_amd import api  # noqa: E402
import rts_amd._lib as L  # noqa: E402
L.require_built()        # a timed tool never builds, and never measures a stale library

args = sys.argv[1:]
out_path = None
if "--out" in args:
    k = args.index("--out"); out_path = args[k + 1]; del args[k:k + 2]
reps = int(args[0]) if args else 20
batches = int(args[1]) if len(args) > 1 else 7
N_RX, ND, NB, HALF, DEPTH = 8, 256, 4096, (1, 2), 8
CELLS = N_RX * ND * NB


def timed(fn, n, n_batches):
    ms = []
    for b in range(n_batches + 1):
        torch.cuda.synchronize()
        a = time.perf_counter()
        for _ in range(n):
            fn()
        torch.cuda.synchronize()
        if b:
            ms.append((time.perf_counter() - a) * 1e3 / n)
    return float(np.median(ms)), float(min(ms)), float(max(ms))


gen = torch.Generator(device="cuda"); gen.manual_seed(1)
maps = [torch.view_as_complex(torch.randn((N_RX, ND, NB, 2), dtype=torch.float64, device="cuda", generator=gen) * (0.5 ** 0.5)) for _ in range(2)]
t = api.Tracer(8, 1)
t.cube_attach(N_RX, 1, NB, 0.0, 1.0)
p = api._tbd_params(HALF, DEPTH, "power", 1.0, 1.0, 0.05, 1.0 / ND)
clock = [0]


def step():
    m = maps[clock[0] & 1]
    api.check(L.lib().rts_cube_tbd_step(t.h, C.byref(p), float(clock[0]), C.c_void_p(m.data_ptr()), ND))
    clock[0] += 1


step(); step()
# the device against the evaluator once, on the first receiver's rows (the evaluator takes a second per 10^6 cells and window offset)
host0 = api.tbd_step_eval(maps[0][:1].cpu().numpy(), None, 0.0, HALF, DEPTH, delay_rate_per_hz=0.05, pri=1.0 / ND)
host1 = api.tbd_step_eval(maps[1][:1].cpu().numpy(), host0[0], 1.0, HALF, DEPTH, delay_rate_per_hz=0.05, pri=1.0 / ND)
codes, shifts = t.tbd_ring()
same = bool(t.tbd_merit()[:1].tobytes() == host1[0].tobytes() and codes[1][:1].tobytes() == host1[1].tobytes() and shifts[1].tobytes() == host1[2].tobytes())
step_ms = timed(step, reps, batches)

src33 = torch.empty(33 * CELLS, dtype=torch.uint8, device="cuda"); dst33 = torch.empty_like(src33)
copy33_ms = timed(lambda: dst33.copy_(src33), reps, batches)
half_bytes = 33 * CELLS // 2
copy16_ms = timed(lambda: dst33[:half_bytes].copy_(src33[:half_bytes]), reps, batches)
del src33, dst33

merit = t.tbd_merit()
threshold = float(np.partition(merit.ravel(), CELLS - 1001)[CELLS - 1001])
e = api._tbd_extract_params(threshold, False, 0, 1.0 / ND)


def extract():
    api.check(L.lib().rts_cube_tbd_extract(t.h, C.byref(e)))


extract()
rec, paths = t.tbd_tracks()
extract_ms = timed(extract, reps, batches)
t.close()

summary = {"reps": reps, "batches": batches, "n_rx": N_RX, "n_doppler": ND, "n_bins": NB, "half": HALF, "depth": DEPTH, "cells": CELLS,
           "shift_span": [int(shifts[1].min()), int(shifts[1].max())], "step_ms": step_ms, "copy_33_bytes_per_cell_ms": copy33_ms, "copy_16p5_bytes_per_cell_ms": copy16_ms,
           "step_over_copy_33": step_ms[0] / copy33_ms[0], "step_over_copy_16p5": step_ms[0] / copy16_ms[0], "step_floor_GBps": 33e-6 * CELLS / step_ms[0],
           "candidates": int(len(rec)), "path_cells": sorted(set(rec["n_cells"].tolist())), "extract_ms": extract_ms, "equal_bytes": same, "build_id": L.build_id()}
print("rts_cube_tbd_step, %d x %d x %d cells, half %s, depth %d, shifts %d .. %d: %.4f ms (%.4f .. %.4f) = %.0f GB/s of its 33-byte floor;  device == host bytes: %s" %
      ((N_RX, ND, NB, HALF, DEPTH, summary["shift_span"][0], summary["shift_span"][1]) + step_ms + (summary["step_floor_GBps"], same)))
print("device-to-device copy of 33 bytes per cell: %.4f ms (%.4f .. %.4f): step / copy = %.2f" % (copy33_ms + (summary["step_over_copy_33"],)))
print("device-to-device copy of 16.5 bytes per cell (33 bytes of traffic): %.4f ms (%.4f .. %.4f): step / copy = %.2f" % (copy16_ms + (summary["step_over_copy_16p5"],)))
print("rts_cube_tbd_extract, %d candidates, paths of %s cells: %.4f ms (%.4f .. %.4f)" % ((len(rec), summary["path_cells"]) + extract_ms))
line = json.dumps(summary)
print(line)
if out_path:
    with open(out_path, "w") as f:
        f.write(line + "\n")
