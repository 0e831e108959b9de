#!/usr/bin/env python3
"""Cost of direction finding (rts_cube_doa_scan: k_doa_scan; rts_cube_eig: k_eig): the MUSIC scan with 2 sources over 2^20 directions at
64 receivers (m = 62 noise vectors) and at 8 (m = 6), and the solve at n = 8 and 64.
Each: `batches` batches of `reps` calls into a caller-owned output, every batch timed by the host clock between two device
synchronisations after a warm-up batch (the handle's stream is the library's own, so the tool cannot put events on it; `reps`
back-to-back calls on one stream hide the launch), the time of a call being the batch's time over `reps`; the median of the batches
and their spread (min .. max).
Yardsticks of the scan, timed the same way in the same run:
  (a) the composition a caller had before the scan: the steering table attached as a cube of one row whose bins are the directions,
      rts_cube_beamform with the m vectors and RTS_BEAM_POWER into a caller-owned buffer [m][n_dirs], a device synchronisation (the
      handle's stream is not torch's: the caller has no other way to order them) and torch.sum over the beams;
  (b) a device-to-device asynchronous copy (torch's copy_) that moves the bytes the scan must move once, 16 n n_dirs read and
      8 n_dirs written (a copy of half their sum: it reads one half and writes the other);
  computed: the f64 issue floor of the tree -- a wave64 f64 instruction issues in 4 cycles on one of 1 024 SIMDs at 2.4 GHz; per
      direction m vectors x (n terms of 4 multiplies, an add, a subtract and the two adds of the running sum, + 3 for the power and
      2 for g p and its add) = m (8 n + 5) instructions over 64 lanes.
    python tools/doa_bench.py [reps] [batches] [--out FILE]
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


summary = {"reps": reps, "batches": batches, "scan": [], "eig": []}
gen = torch.Generator(device="cuda"); gen.manual_seed(7)
rng = np.random.default_rng(7)
n_dirs, n_sources = 1 << 20, 2
t = api.Tracer(8, 1); t.cube_attach(1, 1, 1, 0.0, 1.0)
comp = api.Tracer(8, 1)
for n in (64, 8):
    m = n - n_sources
    table = torch.randn((n, 1, n_dirs), dtype=torch.complex128, device="cuda", generator=gen)            # element-major: a cube of one row
    z = rng.standard_normal((n, 4 * n)) + 1j * rng.standard_normal((n, 4 * n))
    values, vectors = api.eig_eval(z @ z.conj().T / (4 * n))
    vec = torch.from_numpy(vectors).to("cuda")
    out = torch.zeros(n_dirs, dtype=torch.float64, device="cuda")
    powers = torch.zeros((m, n_dirs), dtype=torch.float64, device="cuda"); total = torch.zeros(n_dirs, dtype=torch.float64, device="cuda")
    moved = 16 * n * n_dirs + 8 * n_dirs
    src = torch.zeros(moved // 16, dtype=torch.float64, device="cuda"); dst = torch.empty_like(src)       # half the bytes each
    torch.cuda.synchronize()
    comp.cube_attach(n, 1, n_dirs, 0.0, 1.0, device_ptr=table.data_ptr())
    g = np.ones(m)
    scan = timed(lambda: t.cube_doa_scan(table.data_ptr(), g, first_vector=n_sources, inverse=True, n_dirs=n_dirs, device_vectors=vec.data_ptr(), n=n,
                                         device_ptr=out.data_ptr()))
    noise = vectors[n_sources:]

    def composition():
        comp.cube_beamform(noise, power=True, device_ptr=powers.data_ptr())
        torch.cuda.synchronize()
        torch.sum(powers, dim=0, out=total)
    composed = timed(composition)
    cp = timed(lambda: dst.copy_(src, non_blocking=True))
    q = 1.0 / total
    same = bool(torch.allclose(q, out, rtol=1e-12, atol=0.0)) and bool(torch.isfinite(out).all())
    floor = n_dirs / 64 * m * (8 * n + 5) * 4 / SIMDS / HZ * 1e3
    rec = {"n": n, "m": m, "n_dirs": n_dirs, "scan_ms": scan, "composition_ms": composed, "scan_median_below_composition_min": scan[0] < composed[1],
           "composition_bytes_written": 8 * m * n_dirs, "bytes_moved_once": moved, "copy_ms": cp, "copy_over_scan": cp[0] / scan[0],
           "f64_floor_tree_ms": floor, "floor_over_scan": floor / scan[0], "agrees_with_composition": same}
    summary["scan"].append(rec)
    print("scan %2d rx, %2d vectors, %d directions: %.4f ms (%.4f .. %.4f);  (a) beamform + sync + torch.sum (%d MB of powers) %.4f ms (%.4f .. %.4f): the scan %s;  "
          "(b) copy of the bytes moved once (%d MB) %.4f ms (%.4f .. %.4f), %.2f of the call;  f64 issue floor of the tree %.4f ms (%.2f of the call);  agrees with (a): %s" %
          ((n, m, n_dirs) + scan + (8 * m * n_dirs // 10 ** 6,) + composed + ("wins" if rec["scan_median_below_composition_min"] else "LOSES", moved // 10 ** 6) + cp +
           (rec["copy_over_scan"], floor, rec["floor_over_scan"], same)), flush=True)
    del table, powers, total, src, dst, out, q
for n in (8, 64):
    z = rng.standard_normal((n, 4 * n)) + 1j * rng.standard_normal((n, 4 * n))
    cov = z @ z.conj().T / (4 * n)
    sweeps = api.eig_eval(cov, sweeps=True)[2]
    dc = torch.from_numpy(cov).to("cuda")
    vals = torch.zeros(n, dtype=torch.float64, device="cuda"); vecs = torch.zeros((n, n), dtype=torch.complex128, device="cuda")
    torch.cuda.synchronize()
    ms = timed(lambda: t.cube_eig(n=n, device_cov=dc.data_ptr(), device_values=vals.data_ptr(), device_vectors=vecs.data_ptr()))
    summary["eig"].append({"n": n, "sweeps": sweeps, "eig_ms": ms})
    print("eig %2d x %2d, %d sweeps: %.4f ms (%.4f .. %.4f)   (k_mvdr at 64 receivers x 64 beams: 0.41 ms, profiles/adapt_bench.txt)" % ((n, n, sweeps) + ms), flush=True)
t.close(); comp.close()
summary["build_id"] = rts_amd._lib.build_id()
line = json.dumps(summary)
print(line)
if out_path:
    with open(out_path, "w") as f:
        f.write(line + "\n")
