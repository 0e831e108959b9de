#!/usr/bin/env python3
"""Cost of multistatic localisation (rts_cube_locate: k_locate_plots, k_locate_segs, k_locate_pairs twice around a scan,
k_locate_resolve, the scan, k_locate_write) at 64, 256 and 1024 plots per receiver with four receivers, against the path a caller had
before: the plots on the host and rts_locate_eval there.
  The scene: the transmitter and four receivers of tests/locate_ref.py (8 - 25 km apart); a quarter of a receiver's plots are targets
in the 62 km x 62 km x 13 km box seen by all four with 5 m and 2 Hz of noise, the others clutter: a third of it below the receiver's
baseline (screened at once), the rest anywhere up to 150 km.  gate 9.21, assoc 40 m, four Gauss-Newton steps.  The plots go through
device_list (a torch byte tensor), as in the tests.
  Each: `batches` batches of `reps` calls, every batch timed by the host clock between two device synchronisations after a warm-up
batch; ms per call = batch time / reps; the median of the batches (min .. max).  The host path is timed per call (ONE call at 1024).
  The share of triples that pass the screen and of those that then have a root in the box is estimated on `sample` triples drawn
uniformly, with the closed form of include/rts_amd.h restated in numpy (batched np.linalg.solve).
    python tools/locate_bench.py [reps] [batches] [--out FILE] [--only N] [--sample N]
Prints one line per measurement and a JSON summary (also written to FILE).  RTS_AMD_LIB names another build for A/B runs."""
import ctypes as C
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
import rts_amd._lib as L  # noqa: E402
L.require_built()        # a timed tool never builds, and never measures a stale library
import locate_ref as R  # noqa: E402

args = sys.argv[1:]


def option(name, default):
    if name in args:
        k = args.index(name); v = args[k + 1]; del args[k:k + 2]
        return v
    return default


out_path = option("--out", None)
only = option("--only", None)
sample = int(option("--sample", 2000000))
reps = int(args[0]) if args else 10
batches = int(args[1]) if len(args) > 1 else 5
RX = R.RX5[:4]


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


def scene(n):
    """n plots per receiver, n / 4 of them targets"""
    t = n // 4
    return R.scene(1000 + n, t, RX, clutter=(n - t, n - t, n - t))[0] if n > 4 else R.scene(1000 + n, n, RX)[0]


def fill_out(z, n):
    """the fourth receiver gets its clutter too (R.scene gives clutter to the anchors)"""
    rng = np.random.default_rng(n)
    have = int(np.sum(z["rx"] == 3))
    base = np.linalg.norm(RX[3] - R.TX)
    extra = R.make_plots([(3, rng.uniform(1.1 * base, 150e3) / R.C0, rng.normal(0.0, 3000.0), 0.25) for _ in range(n - have)])
    return np.concatenate([z, extra])


def shares(z, n_sample):
    """of n_sample triples drawn uniformly: the share that passes the screen, and the share of all that then has a root in the box"""
    rng = np.random.default_rng(7)
    tx, S = R.TX, RX
    Rs = [R.C0 * z["delay"][z["rx"] == m] for m in range(3)]
    Rt = np.stack([Rs[a][rng.integers(0, len(Rs[a]), n_sample)] for a in range(3)], axis=1)
    D = S[:3] - tx
    dn = np.linalg.norm(D, axis=1)
    ok = np.all(Rt >= dn, axis=1)
    for a, b in ((0, 1), (0, 2), (1, 2)):
        ok &= np.abs(Rt[:, a] - Rt[:, b]) <= np.linalg.norm(S[a] - S[b])
    Rk = Rt[ok]
    A = D @ D.T + Rk[:, :, None] * Rk[:, None, :]
    c = (dn * dn - Rk * Rk) / 2
    y = np.linalg.solve(A, c[:, :, None])[:, :, 0]
    u0 = y @ D
    r0 = -np.sum(Rk * y, axis=1)
    col = D.T
    X12, X02, X01 = np.cross(col[1], col[2]), np.cross(col[0], col[2]), np.cross(col[0], col[1])
    nv = np.stack([-(Rk @ X12), Rk @ X02, -(Rk @ X01)], axis=1)
    nr = -float(col[2] @ X01)
    qa = np.sum(nv * nv, axis=1) - nr * nr; qb = np.sum(u0 * nv, axis=1) - r0 * nr; qc = np.sum(u0 * u0, axis=1) - r0 * r0
    disc = qb * qb - qa * qc
    lo, hi = np.array(R.BOX[0]), np.array(R.BOX[1])
    any_root = np.zeros(len(Rk), bool)
    with np.errstate(invalid="ignore", divide="ignore"):
        for sign in (-1.0, 1.0):
            ell = (-qb + sign * np.sqrt(disc)) / qa
            r = r0 + ell * nr
            x = tx + u0 + ell[:, None] * nv
            any_root |= (disc >= 0) & (r > 0) & np.all(Rk - r[:, None] > 0, axis=1) & np.all((x >= lo) & (x <= hi), axis=1)
    return float(np.mean(ok)), float(np.sum(any_root) / n_sample)


tr = api.Tracer(8, 1)
cases = []
for n in (64, 256, 1024):
    if only is not None and int(only) != n:
        continue
    z = fill_out(scene(n), n)
    z = z[np.argsort(z["rx"], kind="stable")]
    par = R.par()
    buf = torch.from_numpy(np.frombuffer(z.tobytes() + b"\0" * 8, np.uint8).copy()).to("cuda")
    got = tr.cube_locate(device_list=buf.data_ptr(), n_list=len(z), **par)
    rounds = C.c_uint32(0)
    L.check(L.lib().rts_cube_locate_rounds(tr.h, C.byref(rounds)))
    t0 = time.perf_counter()
    want = api.locate_eval(z, **par)
    first_host = (time.perf_counter() - t0) * 1e3 / 2                   # (locate_eval calls the evaluator twice: the count, then the records)
    dev = timed(lambda: tr.cube_locate(device_list=buf.data_ptr(), n_list=len(z), fetch=False, **par), reps, batches)
    host = (first_host,) * 3 if n >= 1024 else timed(lambda: api.locate_eval(z, **par), 1, 3)
    if n < 1024:
        host = tuple(v / 2 for v in host)
    screen, box = shares(z, sample)
    case = dict(plots_per_receiver=n, triples=n ** 3, targets=len(got), true_targets=n // 4 if n > 4 else n, rounds=rounds.value, locate_ms=dev, host_eval_ms=host,
                share_pass_screen=screen, share_root_in_box=box, equal_bytes=got.tobytes() == want.tobytes())
    cases.append(case)
    print(" %d plots per receiver (%d triples, %.3g pass the screen, %.3g have a root in the box), %d targets of %d in %d rounds: rts_cube_locate %.4f ms (%.4f .. %.4f);  "
          "rts_locate_eval on the host %.1f ms (%.1f .. %.1f);  device == host bytes: %s" % ((n, n ** 3, screen, box, len(got), case["true_targets"], rounds.value) + dev + tuple(host) + (case["equal_bytes"],)))
tr.close()
summary = dict(reps=reps, batches=batches, sample=sample, cases=cases, build_id=L.build_id() if hasattr(L, "build_id") else None)
print(" " + json.dumps(summary))
if out_path:
    with open(out_path, "w") as f:
        json.dump(summary, f)
