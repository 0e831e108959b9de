#!/usr/bin/env python3
"""Cost of the passive radar's two steps (rts_cube_cancel: k_passive_gram, k_passive_cross, k_passive_reduce, k_passive_solve,
k_passive_apply; rts_cube_xcorr: k_passive_xcorr) on a cube of 4 receivers (one the reference) x 256 rows x 4 096 and 8 192 bins:
  * the cancellation with K = 16 and 64 taps and rows_per_block = 1, 16 and 0 (the whole span);
  * the correlation at 256 and 1 024 lags.
Each: `batches` batches of `reps` calls, every batch timed by the host clock between two device synchronisations after a warm-up
batch (the handle's stream is the library's own, so the tool cannot put events on it; `reps` back-to-back calls on one stream hide
the launch), the time of a call being the batch's time over `reps`; the median of the batches and their spread (min .. max).  The
cancellation works in place: every call after the first cancels an already cancelled cube -- the reference rows never change, so G,
the factor and every launch are the same; only the values of b and c differ.
Two floors per step, in the same run:
  * timed the same way, a device-to-device asynchronous copy (torch's copy_) that moves the bytes the step must move -- the
    cancellation reads the cube once and writes the surveillance rows, the correlation reads the cube and writes its output: a copy
    of half of them, which reads one half and writes the other;
  * computed, the f64 issue floor: the step's f64 operations over 64 lanes, at the cycles per wave-instruction that
    profiles/r03_valu_calib.json calibrates for v_mul_f64 / v_add_f64 with four waves per SIMD, on 1 024 SIMDs at 2.4 GHz.  Per
    cell the cancellation forms K (K + 1) / 2 entries of G, 3 K of the b and 3 K steps of the subtraction, 8 operations each; the
    correlation 8 per (lag, sample) pair inside the row.
    python tools/passive_bench.py [reps] [batches] [--out FILE]
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
reps = int(args[0]) if args else 5
batches = int(args[1]) if len(args) > 1 else 5
with open(os.path.join(ROOT, "profiles", "r03_valu_calib.json")) as f:
    calib = json.load(f)["classes"]
CYCLES = 0.5 * (calib["v_mul_f64"]["waves_per_simd_4"]["cycles_per_wave_inst_per_simd"] + calib["v_add_f64"]["waves_per_simd_4"]["cycles_per_wave_inst_per_simd"])
SIMDS, HZ = 1024, 2.4e9


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


def copy_of(n_bytes):
    src = torch.zeros(n_bytes // 16, dtype=torch.float64, device="cuda"); dst = torch.empty_like(src)       # half the bytes each
    torch.cuda.synchronize()
    return timed(lambda: dst.copy_(src, non_blocking=True))


def floor_ms(ops):
    return ops / 64 * CYCLES / SIMDS / HZ * 1e3


summary = {"reps": reps, "batches": batches, "f64_cycles_per_wave_inst": CYCLES, "cancel": [], "xcorr": []}
gen = torch.Generator(device="cuda"); gen.manual_seed(7)
t = api.Tracer(8, 1)
n_rx, rows, REF = 4, 256, 3
for nb in (4096, 8192):
    cube = torch.randn((n_rx, rows, nb), dtype=torch.complex128, device="cuda", generator=gen)
    cube[:REF] += 10.0 * cube[REF]
    torch.cuda.synchronize()
    t.cube_attach(n_rx, rows, nb, 0.0, 1.0, device_ptr=cube.data_ptr())
    cells = rows * nb
    moved = 16 * cells * (n_rx + n_rx - 1)
    cp = copy_of(moved)
    for K in (16, 64):
        ops = cells * 8 * (K * (K + 1) // 2 + 2 * (n_rx - 1) * K)
        for R in (1, 16, 0):
            ms = timed(lambda: t.cube_cancel(REF, K, R))
            info = t.cancel_info()
            assert info[1] == 0, info
            rec = {"n_bins": nb, "K": K, "rows_per_block": R, "blocks": info[0], "cancel_ms": ms, "bytes_moved": moved, "copy_ms": cp, "f64_ops": ops, "f64_floor_ms": floor_ms(ops),
                   "copy_over_call": cp[0] / ms[0], "f64_floor_over_call": floor_ms(ops) / ms[0]}
            summary["cancel"].append(rec)
            print("cancel %d bins K %2d rows_per_block %2d (%3d blocks): %.4f ms (%.4f .. %.4f);  copy of the bytes moved (%d MB) %.4f ms, %.2f of the call;  f64 floor %.4f ms (%.2f)" %
                  (nb, K, R, info[0], ms[0], ms[1], ms[2], moved // 10 ** 6, cp[0], rec["copy_over_call"], rec["f64_floor_ms"], rec["f64_floor_over_call"]), flush=True)
    for n_lags in (256, 1024):
        out = torch.zeros((n_rx, rows, n_lags), dtype=torch.complex128, device="cuda")
        torch.cuda.synchronize()
        moved_x = 16 * cells * n_rx + 16 * n_rx * rows * n_lags
        cpx = copy_of(moved_x)
        ops = 8 * n_rx * rows * sum(nb - l for l in range(n_lags))
        ms = timed(lambda: t.cube_xcorr(REF, n_lags, device_ptr=out.data_ptr()))
        rec = {"n_bins": nb, "n_lags": n_lags, "xcorr_ms": ms, "bytes_moved": moved_x, "copy_ms": cpx, "f64_ops": ops, "f64_floor_ms": floor_ms(ops),
               "copy_over_call": cpx[0] / ms[0], "f64_floor_over_call": floor_ms(ops) / ms[0]}
        summary["xcorr"].append(rec)
        print("xcorr %d bins %4d lags: %.4f ms (%.4f .. %.4f);  copy of the bytes moved (%d MB) %.4f ms, %.2f of the call;  f64 floor %.4f ms (%.2f)" %
              (nb, n_lags, ms[0], ms[1], ms[2], moved_x // 10 ** 6, cpx[0], rec["copy_over_call"], rec["f64_floor_ms"], rec["f64_floor_over_call"]), flush=True)
        assert bool(torch.isfinite(torch.view_as_real(out)).all())
        del out
    del cube
t.close()
summary["build_id"] = rts_amd._lib.build_id()
line = json.dumps(summary)
print(line)
if out_path:
    with open(out_path, "w") as f:
        f.write(line + "\n")
