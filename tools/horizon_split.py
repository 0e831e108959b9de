#!/usr/bin/env python3
"""step 0 and its after-run in one: the counting build on configs[2] (and c2, sphere-like), one lone pulse, with the horizon off, by its
isotropic rule only and by azimuth sector: walk iterations of the waves split by bounce round, rounds without any walk, skipped walks split
into isotropic / by a sector only, node visits and triangle tests"""
import os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from rts_amd import api, scenes
import rts_amd._lib
rts_amd._lib.require_built()
cases = {"c3": lambda: scenes.config3(), "c2": lambda: scenes.config2(rx_radius=200.0)}
for name in (sys.argv[1:] or ["c3", "c2"]):
    spec = cases[name]()
    for mode, kw in (("off", dict(horizon=False)), ("isotropic", dict(horizon_sectors=False)), ("sectors", dict())):
        tr = api.Tracer(spec["W"], spec["max_refl"], 0, spec["smooth"], count_traversal=True, **kw)
        t0 = time.perf_counter(); tr.set_scene(spec["meshes"]); t_scene = time.perf_counter() - t0
        tr.set_receivers(spec["rx"])
        tx = spec["tx"]
        st = tr.trace(tx["origin"], tx["span"], tx["dir"], spec["motion"])
        st = tr.trace(tx["origin"], tx["span"], tx["dir"], spec["motion"])      # the second launch: the tile order has settled
        w = tr.walk_stats(); info = tr.scene_info()
        hz = tr.horizon(info["n_prims"]); by = tr.horizon_sectors(info["n_prims"])
        skipped = w[5] + w[11]
        bounce_segs = st["segments"] - st["rays"]
        print("%s horizon=%s: segments %d (bounce %d) shaded %d received %d | walked segments %d | skipped walks %d = %.1f %% of bounce segments (isotropic %d, by a sector only %d) | wave iterations: round 0 %d in %d rounds, rounds >= 1 %d in %d rounds, %d of them (%.1f %%) without any walk | lane-steps issued (lane 0's rounds) %d | node visits %d tri tests %d | trace %.3f ms | set_scene %.3f s (build %.2f ms), horizon %d bytes; S = 0 on %.1f %% of sides, S < 0.5 on %.1f %%, S = 1 on %.1f %%; sector bytes: 0 on %.1f %%, 255 on %.1f %%" % (
            name, mode, st["segments"], bounce_segs, st["shaded"], st["received"], st["walked_segments"], skipped, 100.0 * skipped / max(bounce_segs, 1), w[5], w[11], w[9], w[10], w[6], w[8], w[7], 100.0 * w[7] / max(w[8], 1),
            w[0], st["node_visits"], st["tri_tests"], st["ms_trace"], t_scene, info["build_ms"], info["horizon_bytes"], 100.0 * (hz == 0).mean(), 100.0 * (hz < 0.5).mean(), 100.0 * (hz == 1).mean(), 100.0 * (by == 0).mean(), 100.0 * (by == 255).mean()))
        tr.close()
