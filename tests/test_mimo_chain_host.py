"""The MIMO chain on a cube that the RAY TRACER made (CPU only: the oracle's rays, the library's host evaluators; the scene and the
recipe are tests/mimo_chain_ref.py's): two transmitters two wavelengths apart with orthogonal 16-chip codes and four elements half a
wavelength apart on one line oblique to the line of sight, a plate facing them, one launch per (transmitter, element, pulse), every
launch rendered with its transmitter's waveform times its slow-time code into ONE cube [4][8][64].  rts_bank_eval takes the two
transmitters apart into eight virtual elements.  The reference, independent of the bank: transmitter 0 alone onto the eight-element
half-wavelength line, compressed by tests/cube_ref.py's statement.

  a  the virtual cube's Bartlett spectrum peaks within one grid step (0.5 degrees) of the eight-element line's peak, its -3 dB width is
     the line's within one grid step, and the four physical receivers alone give a width near twice that;
  b  at the target cell the eight virtual snapshots equal the eight physical ones up to a common factor, within RESIDUAL_BOUND.

Measured here: 2200 echoes in each of the 128 launches; virtual array: peak at 0.0 degrees, width 13.65 degrees; the line: 0.0, 13.64;
the four receivers alone: 0.0, 28.16 (2.07 times the line's); residual 0.0047 after the common factor 0.9983 + 0.0021j.

(a) needs the bank: without it the cube has four receivers and nothing gives the narrow lobe."""
import numpy as np
import pytest

import mimo_chain_ref as MC


@pytest.fixture(scope="module")
def chain(rts, oracle):
    return MC.host_chain(rts, oracle)


def test_every_launch_delivers_the_same_echoes(chain):
    counts = chain["counts"]
    print("echoes per launch: min %d, max %d over %d launches" % (min(counts.values()), max(counts.values()), len(counts)))
    assert len(counts) == (MC.N_TX * MC.N_EL + MC.N_VIRT) * MC.N_PULSES and set(counts.values()) == {MC.RAYS}
    cube = chain["cube"]
    # both transmitters' echoes arrive together: the same 16 bins of every row, nothing elsewhere
    assert np.all(cube[:, :, MC.BIN:MC.BIN + MC.M_CHIPS] != 0) and np.count_nonzero(cube) == MC.N_EL * MC.N_PULSES * MC.M_CHIPS


def test_conditions_on_the_traced_radar(chain):
    MC.check(chain["figures"])


def test_the_four_receivers_without_the_bank_do_not_meet_condition_a(rts, chain):
    """what the code offered before the bank: rts_cube_compress's result on the four receivers.  Its lobe is twice the line's"""
    fig = dict(chain["figures"], virtual=chain["figures"]["four"])
    with pytest.raises(AssertionError):
        MC.check(fig)


def test_cross_talk_at_the_target_cell_is_rounding(rts, chain):
    """the other transmitter's echo through this transmitter's filter at the target cell: the chips' zero-lag inner product, exactly 0,
    times its amplitude -- a cube rendered with transmitter 1 alone leaves rounding in transmitter 0's virtual elements"""
    assert np.vdot(MC.chips()[0], MC.chips()[1]) == 0
    v = chain["virtual"]
    own = np.abs(v[:, :, MC.BIN]).min()
    only0 = rts.bank_eval(chain["line_raw"][:MC.N_EL], MC.waveforms(rts), MC.slow_code())      # transmitter 0 alone on the same four elements
    leak = np.abs(only0[MC.N_EL:, :, MC.BIN]).max()
    print("transmitter 1's filter on transmitter 0's echo at the target cell: %.3g of the smallest own echo" % (leak / own))
    # M eps sum |y| |s| (tests/test_mimo_host.py's bound): the sum of the sixteen terms' magnitudes IS the own echo's magnitude
    assert leak <= MC.M_CHIPS * 2.0 ** -52 * np.abs(only0[:MC.N_EL, :, MC.BIN]).max()
