#!/usr/bin/env python3
"""Cost of receiver noise (rts_cube_add_noise) and CFAR detection (rts_cube_detect) on the bench shape: 4 receivers x 256 pulses x
1 024 range bins, and 2 048 bins:
  * noise over the whole cube, `reps` calls, timed by the host clock up to a stream synchronise
  * CA detection with G = (2, 2), T = (8, 4), pfa 1e-6, local maxima, on the handle's 256-point range-Doppler map of a noise-only
    cube (a few detections: the write pass skips nearly every tile) and at pfa 1e-3 (about one detection per tile: both passes
    run in full), the same way
  * the same map through OS detection (rts_cube_detect_os) with the same window, rank 186 of 248, at both rates: the time per call up
    to a synchronise, the HOST time of one call (it never waits for the device), and the LDS bytes the COUNT pass reads per call --
    N x 8 B per cell, one 8-byte read per training cell -- with the time the LDS arrays of 256 CUs need for them at 256 B/clk/CU
Also prints the bytes each kernel must move (noise: the cube read and written; detection: the map read once per pass), so that a
`rocprofv3 --kernel-trace --stats` run of this script gives each kernel's share of HBM peak.
    python tools/detect_bench.py [reps]
Prints one line per measurement and a JSON summary."""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402  (before the library: one HIP runtime serves both; torch.cuda.synchronize drains the handle's stream)
from rts_amd import api  # noqa: E402
import rts_amd._lib  # noqa: E402
rts_amd._lib.require_built()        # a timed tool never builds, and never measures a stale library

reps = int(sys.argv[1]) if len(sys.argv) > 1 else 200
N_RX, N_PULSES, N_FFT = 4, 256, 256
N_CU, LDS_BYTES_PER_CLK, CLK_HZ = 256, 256, 2.4e9        # the LDS arrays' peak: 256 B/clk/CU
G, T, OS_RANK = (2, 2), (8, 4), 186


def os_lds_bytes(n_bins):
    """8 B per training cell of every cell of the map: N varies with the range bin alone"""
    (gr, gd), (tr, td) = G, T
    total = 0
    for r in range(n_bins):
        cols = [dr for dr in range(-(gr + tr), gr + tr + 1) if 0 <= r + dr < n_bins]
        total += sum((2 * td) if abs(dr) <= gr else (2 * (gd + td) + 1) for dr in cols)
    return 8 * total * N_RX * N_FFT
summary = {}
for n_bins in (1024, 2048):
    tr = api.Tracer(8, 1)
    tr.cube_attach(N_RX, N_PULSES, n_bins, 0.0, 1e-8)
    cube_bytes = 16 * N_RX * N_PULSES * n_bins
    map_bytes = 16 * N_RX * N_FFT * n_bins
    tr.cube_add_noise(1.0, 1)
    torch.cuda.synchronize()
    t = time.perf_counter()
    for i in range(reps):
        tr.cube_add_noise(1.0, i + 2)
    torch.cuda.synchronize()
    ms = (time.perf_counter() - t) / reps * 1e3
    summary["noise_%d_ms" % n_bins] = ms
    print("noise %d x %d x %d: %.4f ms per call (kernel moves %.1f MB: read + write)" % (N_RX, N_PULSES, n_bins, ms, 2 * cube_bytes / 1e6), flush=True)
    tr.cube_doppler(N_FFT, fetch=False)
    for pfa in (1e-6, 1e-3):
        n = len(tr.cube_detect((2, 2), (8, 4), "ca", pfa=pfa, local_max=pfa < 1e-4))
        t = time.perf_counter()
        for i in range(reps):
            tr.cube_detect((2, 2), (8, 4), "ca", pfa=pfa, local_max=pfa < 1e-4, fetch=False)
        torch.cuda.synchronize()
        ms = (time.perf_counter() - t) / reps * 1e3
        summary["detect_%d_pfa%g_ms" % (n_bins, pfa)] = ms
        summary["detect_%d_pfa%g_n" % (n_bins, pfa)] = n
        print("detect CA G=(2,2) T=(8,4) pfa %g on %d x %d x %d: %.4f ms per call, %d detections (map %.1f MB, read once per pass; "
              "halo of the 16 x 64 tiles: x %.2f)" % (pfa, N_RX, N_FFT, n_bins, ms, n, map_bytes / 1e6, (16 + 12) * (64 + 20) / (16 * 64)), flush=True)
        ca_ms = ms
        kw = dict(guard=G, train=T, rank=OS_RANK, pfa=pfa, local_max=pfa < 1e-4)
        n = len(tr.cube_detect_os(**kw))
        host_ms = 0.0
        for i in range(20):                                  # one call on an idle stream: what the host spends enqueueing it
            torch.cuda.synchronize()
            t = time.perf_counter()
            tr.cube_detect_os(fetch=False, **kw)
            host_ms += (time.perf_counter() - t) / 20 * 1e3
        torch.cuda.synchronize()
        t = time.perf_counter()
        for i in range(reps):
            tr.cube_detect_os(fetch=False, **kw)
        torch.cuda.synchronize()
        ms = (time.perf_counter() - t) / reps * 1e3
        lds = os_lds_bytes(n_bins)
        floor_ms = lds / (N_CU * LDS_BYTES_PER_CLK * CLK_HZ) * 1e3
        summary["detect_os_%d_pfa%g_ms" % (n_bins, pfa)] = ms
        summary["detect_os_%d_pfa%g_host_ms" % (n_bins, pfa)] = host_ms
        summary["detect_os_%d_pfa%g_n" % (n_bins, pfa)] = n
        summary["detect_os_%d_pfa%g_lds_fraction" % (n_bins, pfa)] = floor_ms / ms
        print("detect OS G=(2,2) T=(8,4) rank %d pfa %g on %d x %d x %d: %.4f ms per call (CA above: %.4f), host %.4f ms to enqueue one, %d detections; "
              "COUNT pass reads %.1f MB of LDS = %.4f ms at %d B/clk/CU x %d CUs x %.1f GHz: %.1f %% of that rate over the whole call"
              % (OS_RANK, pfa, N_RX, N_FFT, n_bins, ms, ca_ms, host_ms, n, lds / 1e6, floor_ms, LDS_BYTES_PER_CLK, N_CU, CLK_HZ / 1e9, 100 * floor_ms / ms), flush=True)
    tr.close()
print(json.dumps(summary))
