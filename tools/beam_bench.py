#!/usr/bin/env python3
"""Cost of receive-array beamforming (rts_cube_beamform: k_cube_beam) against the device's own copy rate:
  * 8 receivers x 256 rows x 4 096 bins to 16 and to 64 beams, in each of the three output forms (complex, power, peak)
  * 64 receivers x 64 rows x 4 096 bins to 64 beams, complex
Each shape: `batches` batches of `reps` calls into a caller-owned output, every batch timed by the host clock between two device
synchronisations after a warm-up batch (the handle's stream is the library's own, so the tool cannot put events on it; `reps`
back-to-back calls on one stream hide the launch), the time of a call being the batch's time over `reps`; the median of the batches
and their spread (min .. max).
The yardstick, timed the same way in the same run: a device-to-device asynchronous copy (torch's copy_ of a contiguous tensor) that
moves as many bytes as the call does -- the call reads 16 n_rx bytes and writes 16 n_beams (power: 8 n_beams; peak: 16) per cell, B
in all; the copy is one of B / 2 bytes, which reads B / 2 and writes B / 2.  Both figures, their byte rates and the ratio are printed.
    python tools/beam_bench.py [reps] [batches] [--out FILE]
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
reps = int(args[0]) if args else 20
batches = int(args[1]) if len(args) > 1 else 9


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


SHAPES = [(8, 256, 4096, 16, "complex"), (8, 256, 4096, 16, "power"), (8, 256, 4096, 16, "peak"),
          (8, 256, 4096, 64, "complex"), (8, 256, 4096, 64, "power"), (8, 256, 4096, 64, "peak"),
          (64, 64, 4096, 64, "complex")]
summary = {"reps": reps, "batches": batches, "shapes": []}
gen = torch.Generator(device="cuda"); gen.manual_seed(7)
rng = np.random.default_rng(7)
t = api.Tracer(8, 1)
for n_rx, rows, nb, n_beams, form in SHAPES:
    cells = rows * nb
    cube = torch.randn((n_rx, rows, nb), dtype=torch.complex128, device="cuda", generator=gen)
    out_bytes = {"complex": 16 * n_beams, "power": 8 * n_beams, "peak": 16}[form] * cells
    out = torch.zeros(out_bytes // 8, dtype=torch.float64, device="cuda")
    moved = 16 * n_rx * cells + out_bytes
    src = torch.zeros(moved // 16, dtype=torch.float64, device="cuda"); dst = torch.empty_like(src)       # B / 2 bytes each
    torch.cuda.synchronize()
    t.cube_attach(n_rx, rows, nb, 0.0, 1.0, device_ptr=cube.data_ptr())
    w = rng.standard_normal((n_beams, n_rx)) + 1j * rng.standard_normal((n_beams, n_rx))
    ms = timed(lambda: t.cube_beamform(w, power=form == "power", peak=form == "peak", device_ptr=out.data_ptr()))
    cp = timed(lambda: dst.copy_(src, non_blocking=True))
    rec = {"n_rx": n_rx, "rows": rows, "n_bins": nb, "n_beams": n_beams, "form": form, "bytes_moved": moved,
           "beam_ms": ms, "copy_ms": cp, "beam_bytes_per_s": moved / (ms[0] * 1e-3), "copy_bytes_per_s": moved / (cp[0] * 1e-3), "beam_over_copy_rate": cp[0] / ms[0]}
    summary["shapes"].append(rec)
    print("%2d rx x %3d rows x %4d bins -> %2d beams, %-7s: %.4f ms (%.4f .. %.4f), %.3g B/s;  copy of the same bytes %.4f ms (%.4f .. %.4f), %.3g B/s;  rate ratio %.2f" %
          (n_rx, rows, nb, n_beams, form, ms[0], ms[1], ms[2], rec["beam_bytes_per_s"], cp[0], cp[1], cp[2], rec["copy_bytes_per_s"], rec["beam_over_copy_rate"]), flush=True)
    del cube, out, src, dst
t.close()
summary["build_id"] = rts_amd._lib.build_id()
line = json.dumps(summary)
print(line)
if out_path:
    with open(out_path, "w") as f:
        f.write(line + "\n")
