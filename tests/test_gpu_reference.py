"""GPU (-m gpu): the HIP path against fixtures recorded from the reference's OWN device programs.

tests/golden/ref_*.npz hold what the reference's intersection, closest-hit, miss and ray-generation programs and its two
aggregation kernels computed on the CPU (tests/golden/make_ref_golden.py: compiled unmodified against stand-in headers, the
project's atan2f installed in the miss program, brute-force closest hit).  Here the device traces the same scenes, with the
host-built and with the device-built hierarchy, and must give those records bit for bit; finalise, aggregation and the
response list follow as in test_gpu_parity.test_gpu_matches_golden.  Reads nothing but tests/golden/.
"""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))
import helpers as H  # noqa: E402
import make_ref_golden  # noqa: E402
from test_golden import check_against_golden, REF_NAMES  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def specs():
    return make_ref_golden.ref_golden_specs()


@pytest.mark.parametrize("device_build", [False, True], ids=["host_build", "device_build"])
@pytest.mark.parametrize("name", REF_NAMES)
def test_gpu_matches_reference_golden(rts, specs, name, device_build):
    spec = specs[name]
    g = np.load(os.path.join(HERE, "golden", "ref_" + name + ".npz"), allow_pickle=False)
    n = spec["W"] ** 3
    rows = n * (spec["max_refl"] + 3 if spec.get("max_refr", 0) else 1)
    assert len(g["received"]) == rows
    tr = H.gpu_tracer(rts, spec, keep_all=True, device_build=device_build)
    _, st = H.gpu_trace(rts, spec, tr=tr)
    if "RTS_BUILDER" not in os.environ:
        assert tr.scene_info()["builder"] == (1 if device_build else 0)
    a = tr.all_rays(n)
    check_against_golden(g, a["results"][:rows], a["path"][:rows], a["hit_prim"][:n], a["hit_t"][:n], a["rcs_angle"][:rows])
    assert st["segments"] == g["counters"][0] and st["shaded"] == g["counters"][1]
    assert st["received"] == len(g["rx_slots"])
    # finalise + aggregate on the device vs what the reference's kernels made of the same received rays
    wl = spec["c"] / spec["carrier"]
    tr.finalise_uniform([1.0] * len(spec["meshes"]), wl, 1.0, 1.0, spec["carrier"], spec["c"])
    fin = tr.received()["results"]
    assert np.array_equal(fin["power"], g["fin_power"]) and np.array_equal(fin["doppler"], g["fin_doppler"])
    groups = tr.aggregate(spec["c"], spec["carrier"])
    ag = tr.aggregated()
    assert np.array_equal(ag["pathMatch"], g["agg_pathMatch"])
    np.testing.assert_allclose(ag["results"]["power"], g["agg_power"], rtol=1e-12)
    np.testing.assert_allclose(ag["results"]["doppler"], g["agg_doppler"], rtol=1e-12, atol=1e-9)
    np.testing.assert_allclose(ag["delay"], g["agg_delay"], rtol=1e-12)
    np.testing.assert_allclose(ag["phase"], g["agg_phase"], rtol=1e-9, atol=1e-12)
    resp = rts.groups_to_responses(groups)
    assert np.array_equal(resp["ray"].astype(np.int64), g["unique"].astype(np.int64))
    tr.close()
