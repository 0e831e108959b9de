#!/usr/bin/env python3
"""Cost of plot extraction (rts_cube_plots: k_plot_init, k_plot_link, k_plot_flatten, the radix sort, k_plot_flag, the scan,
k_plot_reduce) on the handle's own detection list, for
  * lists of about 1 024 and 65 536 detections made of 3 x 3 blobs (9 cells each, link (1, 1)), and
  * one component of 65 536 cells (a dense 256 x 256 map),
against what a caller had before: rts_cube_detections_get (a synchronisation and a copy of 72 bytes per record) followed by
rts_plots_eval on the host.  The lists come from the detectors themselves: a caller map with the mask cells bright on a unit
background (OS-CFAR at rank 1 for the blobs, cell averaging at alpha 0.5 for the dense map, where every cell equals its mean).
Each: `batches` batches of `reps` calls, every batch timed by the host clock between two device synchronisations after a warm-up
batch (the handle's stream is the library's own, so the tool cannot put events on it; `reps` back-to-back calls on one stream hide
the launch); the time of a call is the batch's time over `reps`; the median of the batches and their spread (min .. max).  The host
alternative is timed per call (it synchronises by itself).
    python tools/plot_bench.py [reps] [batches] [--out FILE] [--only I]
Prints one line per measurement and a JSON summary (also written to FILE).  Per stage: run it under rocprofv3 --kernel-trace --stats
with --only I (case 0, 1 or 2 alone), so that the kernels' statistics are one list's."""
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
only = None
if "--only" in args:
    k = args.index("--only"); only = int(args[k + 1]); del args[k:k + 2]
reps = int(args[0]) if args else 20
batches = int(args[1]) if len(args) > 1 else 7


def timed(fn, n):
    """ms per call: (median, min, max) over the batches, after one warm-up batch"""
    ms = []
    for b in range(batches + 1):
        torch.cuda.synchronize()
        a = time.perf_counter()
        for _ in range(n):
            fn()
        torch.cuda.synchronize()
        if b:
            ms.append((time.perf_counter() - a) * 1e3 / n)
    return float(np.median(ms)), float(min(ms)), float(max(ms))


def blob_map(n_det):
    """a unit background with n_det // 9 blobs of 3 x 3 cells of power 1e6, five cells apart"""
    n_blobs = n_det // 9
    side = int(np.ceil(np.sqrt(n_blobs)))
    z = np.ones((1, 5 * side, 5 * side), np.complex128)
    for b in range(n_blobs):
        k, r = 5 * (b // side) + 1, 5 * (b % side) + 1
        z[0, k:k + 3, r:r + 3] = 1000.0
    return z, 9 * n_blobs


summary = {"reps": reps, "batches": batches, "cases": []}
for index, (name, n_det) in enumerate((("blobs", 1024), ("blobs", 65536), ("dense", 65536))):
    if only is not None and index != only:
        continue
    if name == "blobs":
        z, n_want = blob_map(n_det)
    else:
        z, n_want = np.full((1, 256, 256), 3.0 + 0.0j), 65536
    _, nd, nb = z.shape
    m = torch.from_numpy(z).to("cuda")
    t = api.Tracer(8, 1); t.cube_attach(1, 1, nb, 0.0, 1.0)
    if name == "blobs":
        det = t.cube_detect_os((0, 0), (2, 2), 1, alpha=10.0, local_max=False, device_ptr=m.data_ptr(), n_doppler=nd)
    else:
        det = t.cube_detect((0, 0), (2, 2), "ca", alpha=0.5, local_max=False, device_ptr=m.data_ptr(), n_doppler=nd)
    assert len(det) == n_want, (len(det), n_want)
    plots = t.cube_plots((1, 1))
    host = api.plots_eval(det, nd, (1, 1), n_rx=1, n_bins=nb)
    same = plots.tobytes() == host.tobytes()
    dev = timed(lambda: t.cube_plots((1, 1), fetch=False), reps)
    buf = np.zeros(65536, L.DETECTION_DTYPE); n = C.c_uint32(0)
    q = L.RtsCubeParams(1, 1, nb, 0, 0.0, 1.0); p = api._plot_params((1, 1), 1, 0.0); out = np.zeros(65536, L.PLOT_DTYPE); np_ = C.c_uint32(0)

    def get_only():
        api.check(L.lib().rts_cube_detections_get(t.h, api.ptr(buf), len(buf), C.byref(n)))

    def alternative():
        get_only()
        api.check(L.lib().rts_plots_eval(C.byref(q), api.ptr(buf), n.value, nd, C.byref(p), api.ptr(out), len(out), C.byref(np_)))
    alt = timed(alternative, max(1, reps // 4)); get = timed(get_only, max(1, reps // 4))
    fetch = timed(lambda: t.plots(), max(1, reps // 4))
    t.close()
    rec = {"case": name, "detections": len(det), "plots": len(plots), "map": [nd, nb], "plots_ms": dev, "host_alternative_ms": alt, "detections_get_ms": get,
           "plots_get_ms": fetch, "device_median_below_alternative_min": dev[0] < alt[1], "equal_bytes": same}
    summary["cases"].append(rec)
    print("%s, %d detections -> %d plots: rts_cube_plots %.4f ms (%.4f .. %.4f);  rts_cube_detections_get + rts_plots_eval %.4f ms (%.4f .. %.4f), of which the get "
          "%.4f ms: the device path %s;  rts_cube_plots_get of the records (twice: count, then copy) %.4f ms;  device == host bytes: %s" %
          ((name, len(det), len(plots)) + dev + alt + (get[0], "wins" if rec["device_median_below_alternative_min"] else "LOSES", fetch[0], same)), flush=True)
summary["build_id"] = L.build_id()
line = json.dumps(summary)
print(line)
if out_path:
    with open(out_path, "w") as f:
        f.write(line + "\n")
