#!/usr/bin/env python3
"""Cost of the MIMO matched-filter bank (rts_cube_bank: k_mimo_bank) on one MI355X: a cube of 4 receivers x 256 rows x 4 096 bins with
2, 4 and 8 waveforms of 256 and 1 024 samples, and a small [4][16][512] cube with the same sets.
Each: `batches` batches of `reps` calls, every batch timed by the host clock between two device synchronisations after a warm-up
batch (the handle's stream is the library's own, so the tool cannot put events on it; `reps` back-to-back calls on one stream hide
the launch), the time of a call being the batch's time over `reps`; the median of the batches and their spread (min .. max).
Beside each time, from the same run:
  * the baseline, the way to the same result without the bank, timed the same way: per waveform rts_cube_set_waveform, a
    device-to-device copy of the cube (torch's copy_) and rts_cube_compress of the copy on the handle that has it attached.  (The
    copy runs on torch's stream and the compression on the handle's: rts_cube_set_waveform comes first because it drains the
    handle's stream -- the previous compression no longer writes the copy --, and a device synchronisation stands between the
    copy and the compression.  That is what a caller of the parent's library has to do, and it is part of the baseline.)  The last
    compression is compared with the bank's last virtual rows: the same bits.
  * computed, the f64 issue floor: 8 operations per term inside the row over 64 lanes, at the cycles per wave-instruction that
    profiles/r03_valu_calib.json calibrates for v_mul_f64 / v_add_f64 with four waves per SIMD, on 1 024 SIMDs at 2.4 GHz.
    python tools/mimo_bench.py [reps] [batches] [--out FILE]
Prints one line per measurement and a JSON summary (also written to FILE).  Kernel times and counters: not taken here."""
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


def floor_ms(ops):
    return ops / 64 * CYCLES / SIMDS / HZ * 1e3


summary = {"reps": reps, "batches": batches, "f64_cycles_per_wave_inst": CYCLES, "bank": []}
gen = torch.Generator(device="cuda"); gen.manual_seed(7)
rng = np.random.default_rng(7)
t = api.Tracer(8, 1); base = api.Tracer(8, 1)
for n_rx, rows, nb in ((4, 256, 4096), (4, 16, 512)):
    cube = torch.randn((n_rx, rows, nb), dtype=torch.complex128, device="cuda", generator=gen)
    copy = torch.empty_like(cube)
    torch.cuda.synchronize()
    t.cube_attach(n_rx, rows, nb, 0.0, 1.0, device_ptr=cube.data_ptr())
    base.cube_attach(n_rx, rows, nb, 0.0, 1.0, device_ptr=copy.data_ptr())
    for M in (256, 1024):
        for nw in (2, 4, 8):
            waves = [api.Waveform(rng.standard_normal(M) + 1j * rng.standard_normal(M), 1) for _ in range(nw)]
            out = torch.zeros((nw * n_rx, rows, nb), dtype=torch.complex128, device="cuda")
            torch.cuda.synchronize()
            ms = timed(lambda: t.cube_bank(waves, device_ptr=out.data_ptr()))

            def parent():
                for w in waves:
                    base.cube_set_waveform(w)         # (drains the handle's stream: the previous compression no longer writes the copy)
                    copy.copy_(cube, non_blocking=True)
                    torch.cuda.synchronize()          # (the compression's stream is not torch's: the copy must have landed)
                    base.cube_compress()
            pm = timed(parent)
            # the last compression against the bank's last virtual rows: the same bits
            torch.cuda.synchronize()
            assert torch.equal(torch.view_as_real(copy), torch.view_as_real(out[(nw - 1) * n_rx:]))
            terms = sum(min(M, nb - n) for n in range(nb))
            ops = 8 * nw * n_rx * rows * terms
            rec = {"n_rx": n_rx, "rows": rows, "n_bins": nb, "n_waves": nw, "M": M, "bank_ms": ms, "baseline_ms": pm, "f64_ops": ops, "f64_floor_ms": floor_ms(ops),
                   "baseline_over_bank": pm[0] / ms[0], "f64_floor_over_bank": floor_ms(ops) / ms[0]}
            summary["bank"].append(rec)
            print("bank [%d][%3d][%4d] %d waveforms of %4d: %.4f ms (%.4f .. %.4f);  copy + set_waveform + compress per waveform %.4f ms (%.4f .. %.4f), %.2f of the bank;  f64 floor %.4f ms (%.2f)" %
                  (n_rx, rows, nb, nw, M, ms[0], ms[1], ms[2], pm[0], pm[1], pm[2], rec["baseline_over_bank"], rec["f64_floor_ms"], rec["f64_floor_over_bank"]), flush=True)
            del out
    del cube, copy
t.close(); base.close()
summary["build_id"] = rts_amd._lib.build_id()
line = json.dumps(summary)
print(line)
if out_path:
    with open(out_path, "w") as f:
        f.write(line + "\n")
