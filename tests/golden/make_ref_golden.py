#!/usr/bin/env python3
"""Records tests/golden/ref_<name>.npz from the REFERENCE'S OWN device programs.

Where make_golden.py writes what the oracle computes, this writes what the reference's triangle_mesh.cu, normal_shader.cu,
ray_tracer.cu and aggregation kernels compute, compiled unmodified as host C++ against the stand-in headers of oracle/refshim
(oracle/Makefile: ref -> oracle/_ref/librts_ref.so, which must exist: __graft_entry__.build() makes it where the
reference's sources are).  The files hold the keys check_against_golden (tests/test_golden.py) reads; tests/test_golden.py
checks the oracle against them and tests/test_gpu_reference.py the HIP path, neither needing the reference.

Two steps of the pipeline are NOT the reference's programs, because they are host code of its ray_tracer.cpp, which is
outside this pin: the filter + finalise between trace and aggregation (oracle.filter_finalise) and the sort + unique of
pathMatch (oracle.unique_paths).  The trace runs with the oracle's atan2f installed in the miss program (the project's one
flagged deviation, [D1]: CUDA's atan2f bits are unknowable), the traversal is the harness's brute force.

Data only: inputs are regenerated from rts_amd.scenes by name.  ref_MANIFEST.txt records the sha256 of every reference file
the recording was compiled from.

    python tests/golden/make_ref_golden.py
"""
import hashlib
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))

from oracle import oracle as O          # noqa: E402
from rts_amd import api, scenes         # noqa: E402
import helpers as H                     # noqa: E402

REF_FILES = ["aggregation.cu", "aggregation.cuh", "normal_shader.cu", "ray_tracer.cu", "ray_tracer.h", "triangle_mesh.cu"]


def ref_golden_specs():
    """scenes the oracle's own goldens (make_golden.py) do not cover, W <= 14"""
    refr = scenes.config_multi(W=12, max_refl=3)
    refr["max_refr"] = 1
    refr["meshes"][0]["refr_index"] = 1.5; refr["meshes"][0]["refl_coeff"] = 0.5
    refr["meshes"][1]["refr_index"] = 2.2; refr["meshes"][1]["refl_coeff"] = -0.6
    refr["meshes"][2]["refl_coeff"] = 1.0
    refr["rx"] = refr["rx"] + [scenes._rx_at((200.0, 0.0, 0.0), (0, 0, 0), 90.0, 2.6)]
    # the "rect" rule (more normals than vertices: normal = normals[prim]) alone in the beam: a rotated box, two bounces off its faces
    bv, bt, bn = api.rect_mesh(9.0, 7.0, 5.0, 0.5, 0.2, 0.1)
    rect = dict(name="rect-box", W=14, max_refl=2, smooth=True, n_pulses=1,
                meshes=[dict(tris=bt, verts=bv, normals=bn, refl_coeff=0.8, refr_index=1.0)],
                motion=[dict(position=(0.0, 0.0, 0.0), velocity=(0.0, 0.0, 0.0))],
                tx=dict(origin=(-200.0, 0.0, 0.0), span=(0.06, 0.05, 0.0), dir=(0.0, 0.0)),
                rx=[scenes._rx_at((-200.0, 0.0, 0.0), (0, 0, 0), 90.0, 2.6), scenes._rx_at((-108.0, -168.0, 0.0), (0, 0, 0), 120.0, 2.6)],
                carrier=scenes.FC, c=scenes.C0)
    moving = scenes.config_multi(W=12)
    moving["motion"] = [dict(position=(0.6, 0.2, 0.0), velocity=(300.0, 100.0, 0.0), rotation=api.rotation_matrix(0.4, 0.1, -0.2)),
                        dict(position=(2.0, 8.0, 1.0), velocity=(0.0, -500.0, 0.0)),
                        dict(position=(9.0, -7.0, 0.4), velocity=(0.0, 0.0, 200.0), rotation=api.rotation_matrix(0.0, 0.0, 0.6))]
    return {
        "refraction_w12": refr,
        "miss_branches_w12": scenes.config_miss_branches(W=12),
        "earth_oblique_w12": scenes.translate(scenes.config_miss_branches(W=12), scenes.ecef_offset(lat=0.6, lon=-2.0)),
        "flat_w14": scenes.config_multi(W=14, smooth=False),
        "rect_w14": rect,
        "moving_w12": moving,
    }


def record(name, spec):
    """the arrays of ref_<name>.npz, from the reference's programs"""
    if O.ref_lib() is None:
        raise RuntimeError("oracle/_ref/librts_ref.so is absent: run __graft_entry__.build() where the reference's sources are")
    O.ref_pin_atan2f(True)
    r = H.oracle_trace(O.REF, spec)
    res = r["results"]
    wl = spec["c"] / spec["carrier"]
    rx, rxi, slots = O.filter_finalise(res, r["path"], [1.0] * len(spec["meshes"]), wl, 1.0, 1.0, spec["carrier"], spec["c"])   # host code: the oracle's
    agg = O.ref_aggregate(rx, rxi, spec["c"], spec["carrier"], len(res))
    uniq = O.unique_paths(agg["pathMatch"])                                                                                      # host code: the oracle's
    s = slots.astype(np.int64)
    rec = np.zeros(len(s), O.PRD_DTYPE)                 # field by field into zeroed records: struct padding is not data, and is 0 in the file
    for f in O.PRD_DTYPE.names:
        rec[f] = res[f][s]
    return dict(received=res["received"].astype(np.int16), reflDepth=res["reflDepth"].astype(np.uint8),
                hit_prim=r["hit_prim"], hit_t=r["hit_t"], path=r["path"].astype(np.int8),
                rx_slots=slots.astype(np.uint32), rx_records=rec.view(np.uint8).reshape(-1, 144),
                rx_rcs_angle=r["rcs_angle"][s],
                fin_power=rx["power"], fin_doppler=rx["doppler"],
                agg_power=agg["results"]["power"], agg_doppler=agg["results"]["doppler"], agg_delay=agg["delay"],
                agg_phase=agg["phase"], agg_pathMatch=agg["pathMatch"], unique=uniq,
                counters=np.array([r["counters"]["segments"], r["counters"]["shaded"]], np.int64))


def manifest(reference):
    lines = []
    for f in REF_FILES:
        with open(os.path.join(reference, f), "rb") as fh:
            lines.append("%s  %s" % (hashlib.sha256(fh.read()).hexdigest(), f))
    return "\n".join(lines) + "\n"


if __name__ == "__main__":
    reference = os.environ.get("RTS_REFERENCE_DIR") or O.REFERENCE_DIR
    for name, spec in ref_golden_specs().items():
        a = record(name, spec)
        path = os.path.join(HERE, "ref_" + name + ".npz")
        np.savez_compressed(path, **a)
        print("ref_" + name, "rows", len(a["received"]), "received", len(a["rx_slots"]), "responses", len(a["unique"]),
              "segments", a["counters"][0], "bytes", os.path.getsize(path))
    with open(os.path.join(HERE, "ref_MANIFEST.txt"), "w") as fh:
        fh.write(manifest(reference))
