"""The chain from the tracer to targets on the host (CPU only: the oracle's rays, the library's host evaluators), on the scene of
tests/locate_chain_ref.py that tests/test_gpu_locate.py traces on the device: three small moving bodies, one transmitter, four
receivers that do not lie in one plane with it, a [4][16][64] cube.  It establishes, before any GPU is asked,

  a  that every receiver receives every body at every pulse, by the SAME rays at all 16 pulses, each ray's length within 2 REACH of its
     body's range sum, and each (body, receiver) return in one range cell throughout;
  b  that the cube gives twelve plots, one per (body, receiver), each at its body's Doppler within a cell, and three targets, each
     made of the four plots of one body and within 2 |J+|_2 sqrt(K) delta of its centre (delta = cspeed dt / 2 + 2 REACH);
  c  that in the longdouble restatement of tests/locate_ref.py no screen, box, association or cost decision on these plots lies
     within 1e-6 relative of its threshold, so the device's outcome on its own plots does not hang on a rounding, and that the
     restatement gives the evaluator's targets.

Measured here: 800 to 1200 rays per pair, lengths 0.79 to 1.39 m short of the body's range sum; plots' range sums 2.1 to 12.3 m
early (the cell's start), Dopplers within 25 Hz; positions 4.3, 6.6 and 7.0 m from the centres against bounds of 34.0, 39.7 and
29.5 m, velocities within 1 m/s; least margin 1.9e-3."""
import numpy as np
import pytest

import locate_chain_ref as LC
import locate_ref as R


@pytest.fixture(scope="module")
def chain(rts, oracle):
    return LC.host_chain(rts, oracle)


def test_every_receiver_receives_every_body_by_the_same_rays(chain):
    n, short = chain["counts"], chain["short"]
    print("rays per (receiver, body): min %d, max %d; lengths %.2f .. %.2f m short" % (n.min(), n.max(), short.min(), short.max()))
    assert n.shape == (LC.N_PULSES, LC.N_RX, 3) and n.min() >= 100 and np.all(n == n[0])
    assert np.all(np.abs(short) <= 2 * LC.REACH) and LC.SHORT[0] < short.min() and short.max() < LC.SHORT[1]
    filled = np.count_nonzero(chain["clean"], axis=2)                      # per (receiver, pulse): the cells that hold a return
    assert np.all(filled == 3) and np.count_nonzero(np.abs(chain["clean"]).sum(axis=1)) == 12


def test_twelve_plots_three_targets_within_the_bound(chain):
    plots, targets = chain["plots"], chain["targets"]
    LC.check_plots(plots)
    LC.check_targets(targets)
    used = sorted(int(e) for t in targets for e in t["plot"][:LC.N_RX])
    assert used == list(range(12))


def test_the_scene_meets_the_margin_condition(chain):
    least, ref, cut = LC.margins(chain["plots"])
    print("least margin %.3g" % least)
    assert least > R.MARGIN and not cut
    got = chain["targets"]
    assert len(ref) == len(got) == 3
    for f in R.DISCRETE:
        assert np.array_equal(ref[f], got[f]), f
    assert np.max(np.abs(ref["pos"] - got["pos"])) < 1e-6
