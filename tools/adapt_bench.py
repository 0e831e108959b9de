#!/usr/bin/env python3
"""Cost of adaptive beamforming (rts_cube_covariance: k_cube_cov + k_cube_cov_reduce; rts_cube_mvdr: k_mvdr):
  * the covariance of 8 and of 64 receivers over 256 rows x 4 096 bins (2^20 training cells)
  * the solve of 64 receivers x 64 beams
Each: `batches` batches of `reps` calls into a caller-owned output, every batch timed by the host clock between two device
synchronisations after a warm-up batch (the handle's stream is the library's own, so the tool cannot put events on it; `reps`
back-to-back calls on one stream hide the launch), the time of a call being the batch's time over `reps`; the median of the batches
and their spread (min .. max).
Two yardsticks per covariance:
  * timed the same way in the same run, a device-to-device asynchronous copy (torch's copy_) that moves the bytes the call reads,
    16 n_rx K: a copy of half of them, which reads one half and writes the other;
  * computed, the f64 issue floor: a wave64 f64 instruction issues in 4 cycles on one of 1 024 SIMDs at 2.4 GHz.  Of the tree alone,
    K n_rx (n_rx + 1) / 2 entries x 8 instructions (four multiplies, an add, a subtract, the two adds of the sum) over 64 lanes; and
    of the kernel as built, K cells x the workgroup's waves x 8 B^2 instructions (rts_adapt.h's plan: blocks on the diagonal form
    entries nobody stores, the last wave is partly idle).
    python tools/adapt_bench.py [reps] [batches] [--out FILE]
Prints one line per measurement and a JSON summary (also written to FILE).  Kernel times: run it under rocprofv3 --kernel-trace --stats."""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402  (before the library: one HIP runtime serves both; torch.cuda.synchronize drains the handle's stream)
from rts_amd import api  # noqa: E402
import rts_amd._lib  # noqa: E402
rts_amd._lib.require_built()        # a timed tool never builds, and never measures a stale library

args = sys.argv[1:]
out_path = None
if "--out" in args:
    k = args.index("--out"); out_path = args[k + 1]; del args[k:k + 2]
reps = int(args[0]) if args else 10
batches = int(args[1]) if len(args) > 1 else 7
SIMDS, HZ, BLOCK, WAVE = 1024, 2.4e9, 2, 64


def timed(fn):
    """ms per call: (median, min, max) over the batches, after one warm-up batch"""
    ms = []
    for b in range(batches + 1):
        torch.cuda.synchronize()
        a = time.perf_counter()
        for _ in range(reps):
            fn()
        torch.cuda.synchronize()
        if b:
            ms.append((time.perf_counter() - a) * 1e3 / reps)
    return float(np.median(ms)), float(min(ms)), float(max(ms))


summary = {"reps": reps, "batches": batches, "covariance": []}
gen = torch.Generator(device="cuda"); gen.manual_seed(7)
t = api.Tracer(8, 1)
rows, nb = 256, 4096
K = rows * nb
for n_rx in (8, 64):
    cube = torch.randn((n_rx, rows, nb), dtype=torch.complex128, device="cuda", generator=gen)
    out = torch.zeros(n_rx * n_rx, dtype=torch.complex128, device="cuda")
    read = 16 * n_rx * K
    src = torch.zeros(read // 16, dtype=torch.float64, device="cuda"); dst = torch.empty_like(src)       # half the bytes each
    torch.cuda.synchronize()
    t.cube_attach(n_rx, rows, nb, 0.0, 1.0, device_ptr=cube.data_ptr())
    ms = timed(lambda: t.cube_covariance(device_ptr=out.data_ptr()))
    cp = timed(lambda: dst.copy_(src, non_blocking=True))
    block_rows = (n_rx + BLOCK - 1) // BLOCK
    waves = (block_rows * (block_rows + 1) // 2 + WAVE - 1) // WAVE
    floor_tree = K * (n_rx * (n_rx + 1) // 2) * 8 / 64 * 4 / SIMDS / HZ * 1e3
    floor_kernel = K * waves * 8 * BLOCK * BLOCK * 4 / SIMDS / HZ * 1e3
    rec = {"n_rx": n_rx, "rows": rows, "n_bins": nb, "cells": K, "bytes_read": read, "cov_ms": ms, "copy_ms": cp,
           "f64_floor_tree_ms": floor_tree, "f64_floor_kernel_ms": floor_kernel,
           "copy_over_cov": cp[0] / ms[0], "tree_floor_over_cov": floor_tree / ms[0], "kernel_floor_over_cov": floor_kernel / ms[0]}
    summary["covariance"].append(rec)
    print("covariance %2d rx x %d cells: %.4f ms (%.4f .. %.4f);  copy of the bytes read (%d MB) %.4f ms (%.4f .. %.4f), %.2f of the call;  "
          "f64 issue floor: the tree %.4f ms (%.2f of the call), the kernel as built %.4f ms (%.2f)" %
          (n_rx, K, ms[0], ms[1], ms[2], read // 10 ** 6, cp[0], cp[1], cp[2], rec["copy_over_cov"], floor_tree, rec["tree_floor_over_cov"],
           floor_kernel, rec["kernel_floor_over_cov"]), flush=True)
    if n_rx == 64:
        rng = np.random.default_rng(7)
        s = rng.standard_normal((64, 64)) + 1j * rng.standard_normal((64, 64))
        w = torch.zeros(64 * 64, dtype=torch.complex128, device="cuda")
        torch.cuda.synchronize()
        mv = timed(lambda: t.cube_mvdr(s, 1.0, device_cov=out.data_ptr(), device_ptr=w.data_ptr()))
        summary["mvdr_64rx_64beams_ms"] = mv
        print("mvdr 64 rx x 64 beams (steering upload + k_mvdr): %.4f ms (%.4f .. %.4f)" % mv, flush=True)
        assert bool(torch.isfinite(torch.view_as_real(w)).all())
    del cube, out, src, dst
t.close()
summary["build_id"] = rts_amd._lib.build_id()
line = json.dumps(summary)
print(line)
if out_path:
    with open(out_path, "w") as f:
        f.write(line + "\n")
