#!/usr/bin/env python3
"""Cost of space-time adaptive processing (rts_cube_st_covariance: k_cube_cov's stacked form + k_cube_cov_reduce; rts_cube_st_apply:
k_st_apply) at 8 receivers, 3 and 8 taps, 16 filters, 256 rows x 4 096 bins.
Each: `batches` batches of `reps` calls into a caller-owned output, every batch timed by the host clock between two device
synchronisations after a warm-up batch (the handle's stream is the library's own, so the tool cannot put events on it; `reps`
back-to-back calls on one stream hide the launch), the time of a call being the batch's time over `reps`; the median of the batches
and their spread (min .. max).
Yardsticks, timed the same way in the same run:
  * the covariance: rts_cube_covariance of n_rx = D = taps x 8 receivers over the same number of cells (the same tree);
  * the filter: (a) a device-to-device asynchronous copy (torch's copy_) that moves the bytes the call must move once, 16 N rows bins
    read and 16 F out_rows bins written (a copy of half their sum: it reads one half and writes the other); (b) rts_cube_beamform
    with n_rx = N, n_beams = F on the same rows, times the taps: what a filter that reads every row once per tap would cost.
    python tools/stap_bench.py [reps] [batches] [--out FILE]
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


summary = {"reps": reps, "batches": batches, "shapes": []}
gen = torch.Generator(device="cuda"); gen.manual_seed(7)
rng = np.random.default_rng(7)
N, F, rows, nb = 8, 16, 256, 4096
t = api.Tracer(8, 1)
wide = api.Tracer(8, 1)
cube = torch.randn((N, rows, nb), dtype=torch.complex128, device="cuda", generator=gen)
torch.cuda.synchronize()
t.cube_attach(N, rows, nb, 0.0, 1.0, device_ptr=cube.data_ptr())
w1 = rng.standard_normal((F, N)) + 1j * rng.standard_normal((F, N))
beams = torch.zeros(F * rows * nb, dtype=torch.complex128, device="cuda")
torch.cuda.synchronize()
bf = timed(lambda: t.cube_beamform(w1, device_ptr=beams.data_ptr()))
summary["beamform_ms"] = bf
print("beamform %d rx -> %d beams, %d rows x %d bins: %.4f ms (%.4f .. %.4f)" % ((N, F, rows, nb) + bf), flush=True)
del beams
for M in (3, 8):
    D, out_rows = N * M, rows - M + 1
    K = out_rows * nb
    # the covariance and its yardstick
    cov = torch.zeros(D * D, dtype=torch.complex128, device="cuda")
    torch.cuda.synchronize()
    st_cov = timed(lambda: t.cube_st_covariance(M, device_ptr=cov.data_ptr()))
    stacked = torch.randn((D, out_rows, nb), dtype=torch.complex128, device="cuda", generator=gen)
    torch.cuda.synchronize()
    wide.cube_attach(D, out_rows, nb, 0.0, 1.0, device_ptr=stacked.data_ptr())
    plain_cov = timed(lambda: wide.cube_covariance(device_ptr=cov.data_ptr()))
    del stacked
    # the filter and its yardsticks
    w = rng.standard_normal((F, D)) + 1j * rng.standard_normal((F, D))
    y = torch.zeros(F * K, dtype=torch.complex128, device="cuda")
    moved = 16 * N * rows * nb + 16 * F * K
    src = torch.zeros(moved // 16, dtype=torch.float64, device="cuda"); dst = torch.empty_like(src)       # half the bytes each
    torch.cuda.synchronize()
    st_apply = timed(lambda: t.cube_st_apply(w, M, device_ptr=y.data_ptr()))
    cp = timed(lambda: dst.copy_(src, non_blocking=True))
    assert bool(torch.isfinite(torch.view_as_real(y)).all())
    rec = {"n_rx": N, "n_taps": M, "D": D, "n_filters": F, "rows": rows, "n_bins": nb, "cells": K, "st_cov_ms": st_cov, "cov_of_D_receivers_ms": plain_cov,
           "st_cov_over_cov": st_cov[0] / plain_cov[0], "st_apply_ms": st_apply, "bytes_moved_once": moved, "copy_ms": cp, "copy_over_st_apply": cp[0] / st_apply[0],
           "beamform_times_taps_ms": bf[0] * M, "st_apply_over_beamform_times_taps": st_apply[0] / (bf[0] * M)}
    summary["shapes"].append(rec)
    print("%d taps (D = %d), %d cells: st_covariance %.4f ms (%.4f .. %.4f);  covariance of %d receivers %.4f ms (%.4f .. %.4f);  ratio %.3f" %
          ((M, D, K) + st_cov + (D,) + plain_cov + (rec["st_cov_over_cov"],)), flush=True)
    print("%d taps, %d filters: st_apply %.4f ms (%.4f .. %.4f);  (a) copy of the bytes moved once (%d MB) %.4f ms (%.4f .. %.4f), %.2f of the call;  "
          "(b) beamform x %d = %.4f ms, the call is %.2f of it" %
          ((M, F) + st_apply + (moved // 10 ** 6,) + cp + (rec["copy_over_st_apply"], M, rec["beamform_times_taps_ms"], rec["st_apply_over_beamform_times_taps"])), flush=True)
    del cov, y, src, dst
t.close(); wide.close()
summary["build_id"] = rts_amd._lib.build_id()
line = json.dumps(summary)
print(line)
if out_path:
    with open(out_path, "w") as f:
        f.write(line + "\n")
