#!/usr/bin/env python3
"""Cost of the slow-time spectrogram (rts_cube_spectrogram) on two shapes:
  (a) a 4 x 1024 x 4096 cube, one NULL-window frame with n_fft 1024 over all bins -- the same butterflies as rts_cube_doppler on the
      same cube, timed beside it: the two alternate inside `rounds` rounds of `reps` calls each, so the run-to-run spread of
      rts_cube_doppler itself (max - min of its rounds over their median) is measured in the same job as the ratio it qualifies
  (b) micro-Doppler: the same cube, window 64 (Hann), hop 16, n_fft 128 on a 64-bin gate, summed over the gate (RTS_STFT_SUM_BINS)
      and as the full complex output
each timed by the host clock up to a device synchronise, after one warm-up call per shape.
    python tools/spectrogram_bench.py [reps] [rounds] [--out FILE]
Prints one line per measurement and a JSON summary (also written to FILE)."""
import json
import os
import statistics
import sys
import time

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
rounds = int(args[1]) if len(args) > 1 else 7
N_RX, N_P, N_BINS = 4, 1024, 4096

gen = torch.Generator(device="cuda"); gen.manual_seed(7)
cube = torch.randn((N_RX, N_P, N_BINS), dtype=torch.complex128, device="cuda", generator=gen)
tr = api.Tracer(8, 1)
tr.cube_attach(N_RX, N_P, N_BINS, 0.0, 1.0, device_ptr=cube.data_ptr())


def timed(run):
    """ms per call of `reps` calls up to a device synchronise"""
    torch.cuda.synchronize()
    t = time.perf_counter()
    for _ in range(reps):
        run()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) / reps * 1e3


def rounds_of(runs):
    """the runs alternating, `rounds` rounds each after a warm-up call: name -> the list of ms per call"""
    for run in runs.values():
        run()
    out = {name: [] for name in runs}
    for _ in range(rounds):
        for name, run in runs.items():
            out[name].append(timed(run))
    return out


def stats(ms):
    med = statistics.median(ms)
    return dict(median_ms=med, min_ms=min(ms), max_ms=max(ms), spread=(max(ms) - min(ms)) / med)


summary = {"reps": reps, "rounds": rounds, "cube": [N_RX, N_P, N_BINS]}

# ---- (a)
map_d = torch.zeros((N_RX, N_P, N_BINS), dtype=torch.complex128, device="cuda")
map_s = torch.zeros((N_RX, 1, N_P, N_BINS), dtype=torch.complex128, device="cuda")
got = rounds_of({"doppler": lambda: tr.cube_doppler(N_P, device_ptr=map_d.data_ptr(), fetch=False),
                 "spectrogram": lambda: tr.cube_spectrogram(N_P, 1, N_P, device_ptr=map_s.data_ptr())})
torch.cuda.synchronize()
same = bool(torch.equal(torch.view_as_real(map_d), torch.view_as_real(map_s[:, 0])))
d, s = stats(got["doppler"]), stats(got["spectrogram"])
summary["a_doppler"] = d; summary["a_spectrogram"] = s
summary["a_ratio_spectrogram_over_doppler"] = s["median_ms"] / d["median_ms"]
summary["a_outputs_bit_identical"] = same
summary["a_output_bytes"] = map_s.numel() * 16
print("(a) rts_cube_doppler %.3f ms (rounds %.3f .. %.3f, spread %.1f %%); rts_cube_spectrogram %.3f ms (spread %.1f %%); ratio %.3f; same bits: %s" %
      (d["median_ms"], d["min_ms"], d["max_ms"], 100 * d["spread"], s["median_ms"], 100 * s["spread"], s["median_ms"] / d["median_ms"], same), flush=True)
del map_d, map_s

# ---- (b)
WL, HOP, NF, GATE, FIRST_BIN = 64, 16, 128, 64, 2000
w = api.window("hann", WL)
n_frames = api.stft_frames(N_P, WL, HOP)
out_sum = torch.zeros((N_RX, n_frames, NF), dtype=torch.float64, device="cuda")
out_cpx = torch.zeros((N_RX, n_frames, NF, GATE), dtype=torch.complex128, device="cuda")
got = rounds_of({"sum_bins": lambda: tr.cube_spectrogram(WL, HOP, NF, window=w, first_bin=FIRST_BIN, n_bins=GATE, power=True, sum_bins=True, device_ptr=out_sum.data_ptr()),
                 "complex": lambda: tr.cube_spectrogram(WL, HOP, NF, window=w, first_bin=FIRST_BIN, n_bins=GATE, device_ptr=out_cpx.data_ptr())})
torch.cuda.synchronize()
p = torch.view_as_real(out_cpx).square().sum(dim=-1).sum(dim=-1)
summary["b_shape"] = dict(window_len=WL, hop=HOP, n_fft=NF, gate=GATE, n_frames=n_frames)
summary["b_sum_bins"] = dict(stats(got["sum_bins"]), output_bytes=out_sum.numel() * 8)
summary["b_complex"] = dict(stats(got["complex"]), output_bytes=out_cpx.numel() * 16)
summary["b_sum_vs_complex_max_rel_diff"] = float(((out_sum - p).abs() / p).max())
print("(b) window %d hop %d n_fft %d gate %d, %d frames: summed %.3f ms (%d bytes out), complex %.3f ms (%d bytes out)" %
      (WL, HOP, NF, GATE, n_frames, summary["b_sum_bins"]["median_ms"], out_sum.numel() * 8, summary["b_complex"]["median_ms"], out_cpx.numel() * 16), flush=True)
tr.close()
summary["build_id"] = rts_amd._lib.build_id()
line = json.dumps(summary)
print(line)
if out_path:
    with open(out_path, "w") as f:
        f.write(line + "\n")
