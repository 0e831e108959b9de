"""The MIMO chain on the device, on a cube that the device's own ray tracer made (tests/mimo_chain_ref.py's scene and recipe;
tests/test_mimo_chain_host.py is the same chain on the oracle and the host evaluators).

One tracing handle and one zeroed [4][8][64] buffer: per (transmitter, element) the element alone in the receiver list and its
one-receiver cube attached at its slab of the buffer; per pulse the trace from that transmitter's origin, the finalisation, the
waveform code[t][p] * s_t and the render -- both transmitters ADD into the same rows.  The reference cube [8][8][64] is made the same
way with transmitter 0 alone on the eight-element line.  A second handle without a scene attaches the radar's buffer, runs
rts_cube_bank into a caller-owned tensor and attaches THAT as a cube of eight receivers for the beamformer.  Held to
  * the host cubes of tests/mimo_chain_ref.py within the render's re-association (1e-10 of the largest sample, as
    tests/test_gpu_passive.py holds its traced cube), with the oracle's record count in every launch;
  * (c) the device's bank against rts_bank_eval on the device's own fetched cube, and the beams of the attached virtual cube against
    rts_beamform_eval on the device's own fetched bank output, bit for bit;
  * (a) and (b) of tests/test_mimo_chain_host.py on the device's results, the reference compressed by rts_cube_compress."""
import numpy as np
import pytest

import helpers as H
import mimo_chain_ref as MC

pytestmark = pytest.mark.gpu


def zeros_cube(shape):
    """(torch's stream is not the handles': the buffer is finished before a handle writes it, and a handle's work before torch reads it)"""
    import torch
    buf = torch.zeros(shape, dtype=torch.complex128, device="cuda")
    torch.cuda.synchronize()
    return buf


def host(buf):
    import torch
    torch.cuda.synchronize()
    return buf.cpu().numpy()


def bits(a):
    return np.ascontiguousarray(a).view(np.float64)


@pytest.fixture(scope="module")
def chain(rts, oracle):
    return MC.host_chain(rts, oracle)


def trace_into(rts, buf, positions, transmitters, t0):
    """the recipe: every (transmitter, element, pulse) launch rendered into the element's slab of buf; returns the echo counts"""
    slab = 16 * MC.N_PULSES * MC.N_BINS
    counts = {}
    tracer = H.gpu_tracer(rts, MC.spec(rts, positions, 0, 0))
    for t in transmitters:
        for k in range(len(positions)):
            spec = MC.spec(rts, positions, k, t)
            tracer.set_receivers(spec["rx"])
            tracer.cube_attach(1, MC.N_PULSES, MC.N_BINS, t0, MC.DT, device_ptr=buf.data_ptr() + k * slab)
            for p in range(MC.N_PULSES):
                H.gpu_trace(rts, spec, tr=tracer, motion=MC.motion(p))
                counts[(t, k, p)] = tracer.received_count()
                tracer.finalise_uniform(None, MC.WL, 1.0, 1.0, MC.FC, MC.CS)
                tracer.cube_set_waveform(rts.Waveform(MC.sent(t, p), taps=1))
                tracer.cube_render(p, "rays", MC.CS, MC.FC)
            tracer.cube()                                                          # (the handle's stream drained before the next attach)
    tracer.close()
    return counts


@pytest.fixture(scope="module")
def traced(rts, chain):
    """dict(cube_t: the radar's device tensor, cube / line_raw: the fetched cubes, counts)"""
    cube_t = zeros_cube((MC.N_EL, MC.N_PULSES, MC.N_BINS)); line_t = zeros_cube((MC.N_VIRT, MC.N_PULSES, MC.N_BINS))
    counts = trace_into(rts, cube_t, MC.rx_positions(), range(MC.N_TX), chain["t0"])
    line_counts = trace_into(rts, line_t, MC.line_positions(), [0], chain["t0"])
    return dict(cube_t=cube_t, line_t=line_t, cube=host(cube_t), line_raw=host(line_t), counts=counts, line_counts=line_counts)


def test_device_cubes_against_the_host_cubes(chain, traced):
    """the received count of a launch holds the echoes and, where the transmitter lies off the centre of the element's sphere, the
    rays that missed the plate (mimo_chain_ref.echoes): the oracle's launch holds the same number.  The cubes: within the render's
    re-association (a sum of 2200 rays per transmitter and sample: 1e-10 of the largest sample is generous, tests/test_gpu_passive.py)"""
    sizes = chain["sizes"]
    assert traced["counts"] == {k[1:]: v for k, v in sizes.items() if k[0] == "mimo"}
    assert traced["line_counts"] == {k[1:]: v for k, v in sizes.items() if k[0] == "line"}
    for name, got, ref in (("radar", traced["cube"], chain["cube"]), ("line", traced["line_raw"], chain["line_raw"])):
        print("%s: max error %.3g of max |ref| %.3g" % (name, np.abs(got - ref).max(), np.abs(ref).max()))
        assert np.array_equal(got != 0, ref != 0)
        np.testing.assert_allclose(got, ref, rtol=0, atol=1e-10 * np.abs(ref).max(), err_msg=name)


def test_bank_virtual_array_and_conditions(rts, chain, traced):
    import torch
    tr = rts.Tracer(8, 1)
    tr.cube_attach(MC.N_EL, MC.N_PULSES, MC.N_BINS, chain["t0"], MC.DT, device_ptr=traced["cube_t"].data_ptr())
    virt_t = zeros_cube((MC.N_VIRT, MC.N_PULSES, MC.N_BINS))
    assert tr.cube_bank(MC.waveforms(rts), MC.slow_code(), device_ptr=virt_t.data_ptr()) is None
    virtual = host(virt_t)
    # (c) bit for bit wherever the inputs agree: the evaluator on the device's own cube
    assert np.array_equal(bits(virtual), bits(rts.bank_eval(traced["cube"], MC.waveforms(rts), MC.slow_code())))
    assert np.array_equal(bits(host(traced["cube_t"])), bits(traced["cube"]))       # the cube was only read
    # the virtual cube attached as eight receivers: the array families take it as it stands
    positions = rts.virtual_positions(MC.tx_offsets(), MC.rx_positions())
    table = MC.grid_table(rts, positions)
    tr.cube_attach(MC.N_VIRT, MC.N_PULSES, MC.N_BINS, chain["t0"], MC.DT, device_ptr=virt_t.data_ptr())
    beams = tr.cube_beamform(table)
    assert np.array_equal(bits(beams), bits(rts.beamform_eval(virtual, table)))
    spectrum = np.sum(np.abs(beams[:, :, MC.BIN]) ** 2, axis=1)
    assert np.array_equal(spectrum, MC.bartlett(rts, virtual, positions))
    # the reference and the four receivers alone: rts_cube_compress with waveform 0 on copies
    def compress(cube, s):
        d = torch.from_numpy(np.array(cube, np.complex128, order="C")).to("cuda")
        torch.cuda.synchronize()
        tr.cube_attach(cube.shape[0], cube.shape[1], cube.shape[2], chain["t0"], MC.DT, device_ptr=d.data_ptr())
        tr.cube_set_waveform(rts.Waveform(s, taps=1))
        tr.cube_compress()
        return host(d)
    four, line = compress(traced["cube"], MC.chips()[0]), compress(traced["line_raw"], MC.chips()[0])
    assert np.array_equal(bits(four), bits(virtual[:MC.N_EL]))                      # code[0] is all ones: transmitter 0's filter IS the compression
    fig = MC.figures(rts, virtual, four, line)
    MC.check(fig)
    host_fig = chain["figures"]
    assert fig["virtual"][0] == host_fig["virtual"][0] and abs(fig["virtual"][1] - host_fig["virtual"][1]) <= 1e-6
    tr.close()
