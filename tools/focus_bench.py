#!/usr/bin/env python3
"""Cost of the autofocus calls (rts_cube_align: k_focus_envelope, k_align_ref, k_align_corr; rts_cube_pga: k_pga_tile,
k_pga_sum_tiles, k_pga_update; rts_cube_correct: k_focus_copy_rows, k_focus_correct) on a cube of 1 receiver, 256 pulses x 4 096 bins:
the alignment with max_lag 16 and 4 iterations, the PGA with 6 iterations, one correction with both tables and 8 taps.
Each: `batches` batches of `reps` calls into caller-owned outputs, every batch timed by the host clock between two device
synchronisations after a warm-up batch (the handle's stream is the library's own, so the tool cannot put events on it), the time
of a call being the batch's time over `reps`; the median of the batches and their spread (min .. max).  For the record only:
nothing is asserted on these numbers.
Also printed: "evaluator vs numpy", the distance of rts_pga_eval from the numpy restatement over the shapes of
tests/test_focus_host.py (no device in it), which the tests' PGA bounds are multiples of.
    python tools/focus_bench.py [reps] [batches] [--out FILE]
Prints one line per measurement (also written to FILE).  Kernel times: run it under rocprofv3 --kernel-trace --stats."""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch  # noqa: E402  (before the library: one HIP runtime serves both; torch.cuda.synchronize drains the handle's stream)
from rts_amd import api  # noqa: E402
import rts_amd._lib  # noqa: E402
rts_amd._lib.require_built()        # a timed tool never builds, and never measures a stale library
import test_focus_host as TH  # noqa: E402

args = sys.argv[1:]
out_path = None
if "--out" in args:
    k = args.index("--out"); out_path = args[k + 1]; del args[k:k + 2]
reps = int(args[0]) if args else 10
batches = int(args[1]) if len(args) > 1 else 7
lines = []


def say(text):
    print(text, flush=True)
    lines.append(text)


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


worst, worst_rms, margin = TH.pga_distance(api)
say("evaluator vs numpy: largest |phase difference| %.3g cycles (rms record %.3g) over %d cases, least peak margin %.4g" % (worst, worst_rms, len(TH.PGA_CASES), margin))

n_rx, rows, nb = 1, 256, 4096
gen = torch.Generator(device="cuda"); gen.manual_seed(11)
cube = torch.randn((n_rx, rows, nb), dtype=torch.complex128, device="cuda", generator=gen)
cube[:, :, nb // 2] += 40.0
torch.cuda.synchronize()
t = api.Tracer(8, 1)
t.cube_attach(n_rx, rows, nb, 0.0, 1.0, device_ptr=cube.data_ptr())
shifts = torch.zeros(n_rx * rows, dtype=torch.float64, device="cuda")
phase = torch.zeros(n_rx * (rows + 6), dtype=torch.float64, device="cuda")
torch.cuda.synchronize()
al = timed(lambda: t.cube_align(max_lag=16, n_iters=4, device_ptr=shifts.data_ptr()))
say("align  %d rx, %d rows x %d bins, max_lag 16, 4 iterations: %.4f ms (%.4f .. %.4f)" % ((n_rx, rows, nb) + al))
pg = timed(lambda: t.cube_pga(n_iters=6, device_ptr=phase.data_ptr()))
say("pga    %d rx, %d rows x %d bins, 6 iterations: %.4f ms (%.4f .. %.4f)" % ((n_rx, rows, nb) + pg))
sh = np.random.default_rng(3).uniform(-2, 2, (n_rx, rows)); ph = np.random.default_rng(4).uniform(-1, 1, (n_rx, rows))
co = timed(lambda: t.cube_correct(sh, ph, taps=8))
say("correct %d rx, %d rows x %d bins, shifts and phases, 8 taps: %.4f ms (%.4f .. %.4f)" % ((n_rx, rows, nb) + co))
assert bool(torch.isfinite(shifts).all()) and bool(torch.isfinite(phase).all())
t.close()
say(json.dumps({"reps": reps, "batches": batches, "align_ms": al, "pga_ms": pg, "correct_ms": co, "evaluator_vs_numpy_cycles": worst, "build_id": rts_amd._lib.build_id()}))
if out_path:
    with open(out_path, "w") as f:
        f.write("\n".join(lines) + "\n")
