#!/usr/bin/env python3
"""Cost of the tracker step (rts_cube_track: k_track_prep, k_track_gate, k_track_match, k_track_flag, the scan, k_track_write) at
(tracks, plots) of about (64, 1 000), (4 096, 4 096) and (16 384, 65 536), on one receiver and on eight, against the path a caller
had before: the plots copied to the host, rts_tracks_eval there, and the table uploaded again (rts_cube_tracks_set).
  The scene: track i of a receiver stands at delay 10 i (sigma 1, Doppler 0, covariance diag(1, 1), confirmed); the first plots of
the receiver are the tracks' positions with a jitter of up to 0.5, the others lie uniformly over the receiver's span, so a few
false plots fall into most gates (farther out than the track's own plot: the matching still ends after one round).  max_tracks is the track count: the table is full, the
new tracks of the false plots are turned away, and every frame of a batch sees the same (tracks, plots).  The plots go through
device_plots (a torch byte tensor), as in the tests.
  Each: `batches` batches of `reps` frames, every batch timed by the host clock between two device synchronisations after a warm-up
batch (the handle's stream is the library's own; `reps` back-to-back calls on one stream hide the launch); ms per frame = batch time
/ reps; the median of the batches (min .. max).  The host path is timed per call (it synchronises by itself), `host_reps` calls.
    python tools/track_bench.py [reps] [batches] [--out FILE] [--only I] [--host-reps N]
Prints one line per measurement and a JSON summary (also written to FILE).  RTS_AMD_LIB names another build for A/B runs."""
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


def option(name, default):
    if name in args:
        k = args.index(name); v = args[k + 1]; del args[k:k + 2]
        return v
    return default


out_path = option("--out", None)
only = option("--only", None)
host_reps = int(option("--host-reps", 3))
reps = int(args[0]) if args else 20
batches = int(args[1]) if len(args) > 1 else 7
PAR = dict(sigma=(1.0, 1.0), gate=9.21, q=0.01, delay_rate_per_hz=-0.001, doppler_period=1000.0, confirm_hits=3, max_misses=3, tentative_misses=0, max_candidates=16)


def timed(fn, n, n_batches, warm=True):
    ms = []
    for b in range(n_batches + (1 if warm else 0)):
        torch.cuda.synchronize()
        a = time.perf_counter()
        for _ in range(n):
            fn()
        torch.cuda.synchronize()
        if b or not warm:
            ms.append((time.perf_counter() - a) * 1e3 / n)
    return float(np.median(ms)), float(min(ms)), float(max(ms))


def scene(n_t, n_p, n_rx, seed=1):
    rng = np.random.default_rng(seed)
    tracks = np.zeros(n_t, L.TRACK_DTYPE); plots = np.zeros(n_p, L.PLOT_DTYPE)
    tracks["id"] = np.arange(n_t); tracks["rx"] = np.arange(n_t) % n_rx; tracks["flags"] = L.RTS_TRACK_CONFIRMED; tracks["hits"] = 5; tracks["age"] = 5
    tracks["delay"] = 10.0 * (np.arange(n_t) // n_rx); tracks["p_dd"] = 1.0; tracks["p_ff"] = 1.0; tracks["plot_index"] = 0xffffffff
    at = 0
    for rx in range(n_rx):
        mine = tracks[tracks["rx"] == rx]
        n_here = n_p // n_rx + (1 if rx < n_p % n_rx else 0)
        z = plots[at:at + n_here]; at += n_here
        k = min(len(mine), n_here)
        z["rx"] = rx; z["power_sum"] = 1.0
        z["delay"][:k] = mine["delay"][:k] + rng.uniform(-0.5, 0.5, k); z["doppler"][:k] = rng.uniform(-0.5, 0.5, k)
        z["delay"][k:] = rng.uniform(0.0, 10.0 * max(len(mine), 1), n_here - k); z["doppler"][k:] = rng.uniform(-3.0, 3.0, n_here - k)
        order = rng.permutation(n_here); z[:] = z[order]
    return tracks, plots


summary = {"reps": reps, "batches": batches, "host_reps": host_reps, "cases": []}
for index, (n_t, n_p, n_rx) in enumerate(((64, 1000, 1), (64, 1000, 8), (4096, 4096, 1), (4096, 4096, 8), (16384, 65536, 1), (16384, 65536, 8))):
    if only is not None and index != int(only):
        continue
    tracks, plots = scene(n_t, n_p, n_rx)
    par = dict(PAR, max_tracks=n_t)
    raw = np.frombuffer(plots.tobytes() + b"\0" * 8, np.uint8).copy()
    buf = torch.from_numpy(raw).to("cuda")
    t = api.Tracer(8, 1)
    clock = [0.0]

    def step():
        clock[0] += 1.0
        p = api._track_params(par["gate"], par["sigma"], par["q"], par["delay_rate_per_hz"], par["doppler_period"], par["confirm_hits"], par["max_misses"],
                              par["tentative_misses"], par["max_candidates"], n_t, buf.data_ptr(), n_p)
        api.check(L.lib().rts_cube_track(t.h, C.byref(p), clock[0]))

    out = np.zeros(n_t, L.TRACK_DTYPE); n = C.c_uint32(0); nid = C.c_uint64(0); rounds = C.c_uint32(0)
    t.cube_tracks_set(tracks, n_t, 0.0); step()
    rc = L.lib().rts_cube_tracks_get(t.h, api.ptr(out), n_t, C.byref(n), C.byref(nid))
    assert rc in (L.RTS_OK, L.RTS_ERR_CAPACITY), rc
    api.check(L.lib().rts_cube_track_rounds(t.h, C.byref(rounds)))
    host, host_id = api.tracks_eval(tracks, n_t, 1.0, plots, **par)
    same = out.tobytes() == host.tobytes() and nid.value == host_id
    matched = int((out["plot_index"] != 0xffffffff).sum())
    dev = timed(step, reps, batches)
    # the path a caller had: the plots to the host, the evaluator, the table back up
    table = [out.copy()]
    hp = api._track_params(par["gate"], par["sigma"], par["q"], par["delay_rate_per_hz"], par["doppler_period"], par["confirm_hits"], par["max_misses"],
                           par["tentative_misses"], par["max_candidates"], n_t)
    h_out = np.zeros(n_t + n_p, L.TRACK_DTYPE)

    def host_path():
        z = buf[:n_p * 104].cpu().numpy().view(L.PLOT_DTYPE)
        rc = L.lib().rts_tracks_eval(C.byref(hp), api.ptr(table[0]), n_t, n_t, 1.0, api.ptr(z), n_p, api.ptr(h_out), len(h_out), C.byref(n), C.byref(nid))
        assert rc in (L.RTS_OK, L.RTS_ERR_CAPACITY), rc
        table[0] = h_out[:n_t].copy()
        clock[0] += 1.0
        t.cube_tracks_set(table[0], nid.value, clock[0])
    big = n_t * n_p // n_rx > 50_000_000
    alt = timed(host_path, 1, 1 if big else host_reps, warm=not big)
    t.close()
    rec = {"tracks": n_t, "plots": n_p, "receivers": n_rx, "matched": matched, "rounds": rounds.value, "track_ms": dev, "host_path_ms": alt,
           "device_median_below_host_min": dev[0] < alt[1], "equal_bytes": bool(same)}
    summary["cases"].append(rec)
    print("%d tracks x %d plots on %d receiver(s), %d matched in %d rounds: rts_cube_track %.4f ms (%.4f .. %.4f);  plots to the host + rts_tracks_eval + "
          "rts_cube_tracks_set %.4f ms (%.4f .. %.4f): the device step %s;  device == host bytes: %s" %
          ((n_t, n_p, n_rx, matched, rounds.value) + dev + alt + ("wins" if rec["device_median_below_host_min"] else "LOSES", same)), flush=True)
summary["build_id"] = L.build_id()
line = json.dumps(summary)
print(line)
if out_path:
    with open(out_path, "w") as f:
        f.write(line + "\n")
