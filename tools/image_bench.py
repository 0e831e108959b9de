#!/usr/bin/env python3
"""Cost of backprojection imaging (rts_cube_backproject) on two shapes, taps 8:
  * a 512 x 512 image from a 1 x 1024 x 2048 cube (one receiver, a long interval: every thread walks the 16 pulse chunks itself)
  * a 128 x 128 image from a 4 x 256 x 1024 cube (a small image: the 4 pulse chunks go on the grid, a second kernel adds them)
each timed by the host clock up to a device synchronise, `reps` calls after one warm-up call.  As a yardstick the same sum written
with torch complex128 gathers on the same GPU (16 pulses per batch of tensor operations), once after a warm-up; the two images
are compared.  Also times taps 1 and 2 on the first shape: what the interpolation weights cost beside the two square roots and
the carrier phase.
    python tools/image_bench.py [reps] [--out FILE]
Prints one line per measurement and a JSON summary (also written to FILE)."""
import json
import math
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402  (before the library: one HIP runtime serves both; torch.cuda.synchronize drains the handle's stream)
from rts_amd import api  # noqa: E402
import rts_amd._lib  # noqa: E402
rts_amd._lib.require_built()        # a timed tool never builds, and never measures a stale library

args = sys.argv[1:]
out_path = None
if "--out" in args:
    k = args.index("--out"); out_path = args[k + 1]; del args[k:k + 2]
reps = int(args[0]) if args else 5
CS, FC, DT = 299792458.0, 1.0e10, 1.0e-9


def case(n_rx, n_p, n_bins, n):
    """a side-looking track 1 km from an n x n grid of 0.25 m pixels; receiver r rides 10 r m behind the transmitter"""
    j = np.arange(n_p, dtype=np.float64)
    tx = np.stack([np.full(n_p, -1000.0), (j - n_p / 2) * 0.05, np.full(n_p, 40.0)], axis=1)
    rx = np.stack([tx + np.array([0.0, -10.0 * r, 0.0]) for r in range(n_rx)])
    origin = np.array([-n * 0.125, -n * 0.125, 0.0])
    t0 = 2 * math.sqrt(1000.0 ** 2 + 40.0 ** 2) / CS - (n_bins / 2) * DT
    return dict(origin=origin, step_x=np.array([0.25, 0.0, 0.0]), step_y=np.array([0.0, 0.25, 0.0]), n=n, tx=tx, rx=rx, t0=t0)


def torch_backproject(cube, g, taps, batch=16):
    """the header's sum with torch: per batch of pulses the delays of every pixel, the taps gathered from the rows, the carrier phase"""
    dev = cube.device
    n_rx, n_p, n_bins = cube.shape
    n = g["n"]
    ix = torch.arange(n, dtype=torch.float64, device=dev)
    x = (torch.tensor(g["origin"], device=dev)[None, None, :] + ix[None, :, None] * torch.tensor(g["step_x"], device=dev) +
         ix[:, None, None] * torch.tensor(g["step_y"], device=dev))                       # [n_y][n_x][3]
    tx = torch.tensor(g["tx"], device=dev); rx = torch.tensor(g["rx"], device=dev)
    img = torch.zeros((n_rx, n, n), dtype=torch.complex128, device=dev)
    hl = taps // 2
    for r in range(n_rx):
        for j0 in range(0, n_p, batch):
            j1 = min(n_p, j0 + batch)
            dT = torch.linalg.vector_norm(x[None] - tx[j0:j1, None, None, :], dim=-1)
            dR = torch.linalg.vector_norm(x[None] - rx[r, j0:j1, None, None, :], dim=-1)
            tau = (dT + dR) / CS
            d = (tau - g["t0"]) / DT
            rows = cube[r, j0:j1].reshape(j1 - j0, 1, n_bins).expand(j1 - j0, n, n_bins)
            if taps == 1:
                m = torch.floor(d + 0.5).long()
                ok = (m >= 0) & (m < n_bins)
                v = torch.gather(rows, 2, m.clamp(0, n_bins - 1)) * ok
            else:
                i = torch.floor(d); phi = d - i; i = i.long()
                v = torch.zeros_like(d, dtype=torch.complex128)
                for k in range(taps):
                    m = i - hl + 1 + k
                    u = phi + (hl - 1 - k)
                    h = torch.special.sinc(u) * (0.42 + 0.5 * torch.cos(2 * math.pi * u / taps) + 0.08 * torch.cos(4 * math.pi * u / taps))
                    ok = (m >= 0) & (m < n_bins)
                    v += torch.gather(rows, 2, m.clamp(0, n_bins - 1)) * (h * ok)
            c = FC * tau
            img[r] += (v * torch.exp(2j * math.pi * (c - torch.floor(c)))).sum(dim=0)
    return img


summary = {"reps": reps}
for name, n_rx, n_p, n_bins, n in (("512x512_from_1x1024x2048", 1, 1024, 2048, 512), ("128x128_from_4x256x1024", 4, 256, 1024, 128)):
    g = case(n_rx, n_p, n_bins, n)
    gen = torch.Generator(device="cuda"); gen.manual_seed(n)
    cube = torch.randn((n_rx, n_p, n_bins), dtype=torch.complex128, device="cuda", generator=gen)
    out = torch.zeros((n_rx, n, n), dtype=torch.complex128, device="cuda")
    tr = api.Tracer(8, 1)
    tr.cube_attach(n_rx, n_p, n_bins, g["t0"], DT, device_ptr=cube.data_ptr())
    for taps in ((8, 1, 2) if n == 512 else (8,)):
        def run():
            tr.cube_backproject(g["origin"], g["step_x"], g["step_y"], n, n, g["tx"], g["rx"], CS, FC, taps=taps, device_ptr=out.data_ptr())
        run(); torch.cuda.synchronize()
        t = time.perf_counter()
        for _ in range(reps):
            run()
        torch.cuda.synchronize()
        ms = (time.perf_counter() - t) / reps * 1e3
        rate = n_rx * n * n * n_p / (ms * 1e-3)
        key = name if taps == 8 else "%s_taps%d" % (name, taps)
        summary[key + "_ms"] = ms; summary[key + "_pixel_pulses_per_s"] = rate
        print("backproject %s taps %d: %.3f ms per call, %.3g pixel-pulses/s" % (name, taps, ms, rate), flush=True)
    mine = out.clone()                                           # (the last call of the loop: taps 8 on the small shape, taps 2 on the large)
    last = 8 if n != 512 else 2
    torch_backproject(cube[:, :32], dict(g, tx=g["tx"][:32], rx=g["rx"][:, :32]), 8); torch.cuda.synchronize()       # warm-up
    t = time.perf_counter()
    ref8 = torch_backproject(cube, g, 8)
    torch.cuda.synchronize()
    ms_t = (time.perf_counter() - t) * 1e3
    summary[name + "_torch_ms"] = ms_t
    ref = ref8 if last == 8 else torch_backproject(cube, g, last)
    err = float((mine - ref).abs().max()); scale = float(ref.abs().max())
    summary[name + "_max_abs_diff_vs_torch"] = err; summary[name + "_max_abs_torch"] = scale
    print("torch   %s taps 8: %.1f ms (x %.1f of the kernel); taps %d images differ by %.3g at most (max |image| %.3g)" %
          (name, ms_t, ms_t / summary[name + "_ms"], last, err, scale), flush=True)
    tr.close()
summary["build_id"] = rts_amd._lib.build_id()
line = json.dumps(summary)
print(line)
if out_path:
    with open(out_path, "w") as f:
        f.write(line + "\n")
