"""The array, space-time and direction-finding chains on the device, on a receive array that the device's own ray tracer made
(tests/array_ref.py's scene; tests/test_array_chain_host.py is the same chain on the oracle and the host evaluators).

The cube is built by the recipe for a dense array: one tracing handle, one zeroed [8][16][32] buffer; per element the element alone
in the receiver list and its one-receiver cube attached at its slab of the buffer; per pulse trace, finalise, accumulate.  A second
handle without a scene attaches the whole buffer with n_rx = 8 and runs the families.  Held to
  * the host cube of tests/array_ref.py within the project's bound for a device cube against its host restatement (rtol 1e-10,
    atol 1e-12 max |ref|: tests/test_gpu_beat.py, tests/test_gpu_adapt.py::test_whole_chain), with the oracle's ray count in
    every launch;
  * every family against its host evaluator run on the device's own fetched cube, under the rule of that family's own test: noise
    as the whole chains of tests/test_gpu_adapt.py and tests/test_gpu_stap.py hold it, the sources within tests/source_ref.py's
    bound, beams, covariance, weights, eigen spectra and the space-time filter bit for bit;
  * the conditions of tests/test_array_chain_host.py, on the device's results."""
import numpy as np
import pytest

import array_ref as AR
import helpers as H
import source_ref as R

pytestmark = pytest.mark.gpu


def zeros_cube(shape):
    """(torch's stream is not the handles': the buffer is finished before a handle writes it, and a handle's work before torch reads it)"""
    import torch
    buf = torch.zeros(shape, dtype=torch.complex128, device="cuda")
    torch.cuda.synchronize()
    return buf


def dev(a):
    import torch
    buf = torch.from_numpy(np.array(a, np.complex128, order="C")).to("cuda")
    torch.cuda.synchronize()
    return buf


def bits(a):
    return np.ascontiguousarray(a).view(np.float64)


def assert_bound(got, ref, what=""):
    np.testing.assert_allclose(got, ref, rtol=1e-10, atol=1e-12 * np.abs(ref).max(), err_msg=str(what))


def attached(rts, cube):
    """a handle without a scene with the host array [8][16][32] attached as its cube: (handle, the device tensor)"""
    d = dev(cube)
    tr = rts.Tracer(8, 1)
    tr.cube_attach(cube.shape[0], cube.shape[1], cube.shape[2], 0.0, 1.0, device_ptr=d.data_ptr())
    return tr, d


@pytest.fixture(scope="module")
def chain(rts, oracle):
    return AR.host_chain(rts, oracle)


@pytest.fixture(scope="module")
def traced(rts, chain):
    """the device's cube by the recipe: dict(buf: the device tensor, tr: the scene-less handle that has all of it attached, clean: its
    fetched copy, counts: the received rays of every launch [8][16])"""
    spec = AR.spec(rts)
    t0 = chain["t0"]
    buf = zeros_cube((AR.N_RX, AR.N_PULSES, AR.N_BINS))
    slab = 16 * AR.N_PULSES * AR.N_BINS
    counts = np.zeros((AR.N_RX, AR.N_PULSES), np.int64)
    tracer = H.gpu_tracer(rts, spec)
    for k in range(AR.N_RX):
        tracer.set_receivers([spec["rx"][k]])
        tracer.cube_attach(1, AR.N_PULSES, AR.N_BINS, t0, AR.DT, device_ptr=buf.data_ptr() + k * slab)
        for m in range(AR.N_PULSES):
            H.gpu_trace(rts, spec, tr=tracer, motion=AR.motion(m))
            counts[k, m] = tracer.received_count()
            tracer.finalise_uniform(None, AR.WL, 1.0, 1.0, AR.FC, AR.CS)
            tracer.cube_accumulate(m, AR.CS, AR.FC)
        tracer.cube()                                                              # (the handle's stream drained before the next attach)
    tracer.close()
    tr = rts.Tracer(8, 1)
    tr.cube_attach(AR.N_RX, AR.N_PULSES, AR.N_BINS, t0, AR.DT, device_ptr=buf.data_ptr())
    out = dict(buf=buf, tr=tr, clean=tr.cube(), counts=counts)
    yield out
    tr.close()


# ----------------------------------------------------------------------------- 1. the cube
def test_device_cube_against_the_host_cube(chain, traced):
    got, want = traced["clean"], chain["clean"]
    assert np.array_equal(traced["counts"], chain["counts"]) and np.all(traced["counts"] == AR.RAYS)
    assert np.array_equal(got != 0, want != 0) and np.count_nonzero(got) == AR.N_RX * AR.N_PULSES
    print("max error %.3g of max |ref| %.3g" % (np.abs(got - want).max(), np.abs(want).max()))
    assert_bound(got, want)


# ----------------------------------------------------------------------------- 2. every family against its evaluator, and the conditions
@pytest.fixture(scope="module")
def tables(rts):
    return dict(grid=AR.grid_table(rts), bank=AR.filter_bank(rts))


@pytest.fixture(scope="module")
def noisy(rts, chain, traced):
    """a copy of the device's cube with rts_cube_add_noise's noise: dict(tr: its handle, d: its device tensor, cube: its fetched copy)"""
    tr, d = attached(rts, traced["clean"])
    tr.cube_add_noise(chain["noise_power"], AR.NOISE_SEED)
    out = dict(tr=tr, d=d, cube=tr.cube())
    yield out
    tr.close()


def test_beam_of_the_cube_as_traced(rts, traced, tables):
    beams = traced["tr"].cube_beamform(tables["grid"])
    assert beams.shape == (len(tables["grid"]), AR.N_PULSES, AR.N_BINS)
    assert np.array_equal(bits(beams), bits(rts.beamform_eval(traced["clean"], tables["grid"])))
    AR.check_beam(AR.beam_figures(traced["clean"], beams), "the conventional beam of the cube as traced")
    assert np.array_equal(bits(traced["tr"].cube()), bits(traced["clean"]))       # the traced buffer was only read


def test_noise(rts, chain, traced, noisy):
    assert_bound(noisy["cube"], traced["clean"] + AR.noise(rts, chain["noise_power"]), "the device's cube plus rts_noise_eval")
    assert_bound(noisy["cube"], chain["noisy"], "the host chain's noisy cube")


def test_beam_of_the_noisy_cube(rts, noisy, tables):
    beams = noisy["tr"].cube_beamform(tables["grid"])
    assert np.array_equal(bits(beams), bits(rts.beamform_eval(noisy["cube"], tables["grid"])))
    AR.check_beam(AR.beam_figures(noisy["cube"], beams), "the conventional beam of the noisy cube")


@pytest.mark.parametrize("method", AR.METHODS)
def test_direction_finding(rts, chain, noisy, tables, method):
    npow = chain["noise_power"]
    got = noisy["tr"].cube_doa(tables["grid"], method=method, n_sources=1 if method == "music" else None, loading=npow, train=AR.doa_train())
    assert got.shape == (len(tables["grid"]),) and np.array_equal(bits(got), bits(AR.doa_host(rts, noisy["cube"], method, npow))), method
    AR.check_spectrum(AR.spectrum_figures(got), method)


def test_space_time_filter_bank(rts, noisy, tables):
    y = noisy["tr"].cube_st_apply(tables["bank"], AR.TAPS)
    assert y.shape == (len(tables["bank"]), AR.N_PULSES - AR.TAPS + 1, AR.N_BINS)
    assert np.array_equal(bits(y), bits(rts.st_apply_eval(noisy["cube"], tables["bank"], AR.TAPS)))
    AR.check_bank(AR.bank_figures(AR.bank_table(y)))


@pytest.mark.parametrize("sign", [1.0, -1.0], ids=["positive", "negative"])
def test_injected_patch_peaks_at_its_own_sign(rts, traced, tables, sign):
    src = AR.patch(rts, traced["clean"], sign * AR.F_TARGET)
    zero = np.zeros_like(traced["clean"])
    tr, d = attached(rts, zero)
    tr.cube_add_sources(**src)
    alone = tr.cube()
    R.assert_within(alone, rts.sources_eval(zero, **src), R.bound(zero, src["spatial"], src["power"]))
    y = tr.cube_st_apply(tables["bank"], AR.TAPS)
    assert np.array_equal(bits(y), bits(rts.st_apply_eval(alone, tables["bank"], AR.TAPS)))
    AR.check_patch(AR.bank_figures(AR.bank_table(y)), sign * AR.F_TARGET)
    tr.close()


def test_jammer_and_mvdr(rts, chain, traced, noisy):
    npow, clean = chain["noise_power"], traced["clean"]
    src = AR.jammer(rts, clean)
    tr, d = attached(rts, noisy["cube"])                                           # (a copy: the noisy cube stays as it is)
    tr.cube_add_sources(**src)
    jammed = tr.cube()
    R.assert_within(jammed, rts.sources_eval(noisy["cube"], **src), R.bound(noisy["cube"], src["spatial"], src["power"]))
    beam = tr.cube_adaptive_beamform(AR.steering_at(rts, [AR.AZ]), train=dict(skip=(AR.BIN, 1)), loading=npow)
    cov_h, w_h, beam_h = AR.mvdr_host(rts, jammed, npow)
    assert np.array_equal(bits(tr.covariance()), bits(cov_h)) and np.array_equal(bits(tr.mvdr_weights()), bits(w_h))
    assert beam.shape == (1, AR.N_PULSES, AR.N_BINS) and np.array_equal(bits(beam), bits(beam_h))
    AR.check_mvdr(AR.mvdr_figures(rts, clean, jammed, tr.mvdr_weights(), beam))
    tr.close()
