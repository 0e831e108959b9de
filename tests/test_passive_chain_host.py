"""The passive chain on the host (CPU only: the oracle's rays, the numpy render of tests/passive_chain_ref.py, the library's host
evaluators), on the one scenario tests/test_gpu_passive.py repeats on the device: a transmitter of opportunity with a new noise-like
segment per pulse, three moving bodies, three surveillance receivers and a reference slot, a cube [4][16][512], a direct signal 83 ..
92 dB and static clutter 63 .. 78 dB above the nine echoes.

  a  Without rts_cancel_eval the chain xcorr -> Doppler -> OS-CFAR reports none of the nine target cells.
  b  With it every one is reported at the lag and Doppler bin the numpy restatement of the echoes alone gives (and geometry predicts),
     the clutter cells are nulled and the clutter lags' power is down by the numpy restatement's factor.

Measured margins (target cell over its OS-CFAR threshold, the nine cells): without the cancellation 7.0e-5 .. 3.4e-3 of the
threshold; with it 1.7 .. 8.5 times the threshold.  The clutter lags' power over all Doppler bins falls by 87.7 .. 108.4 dB."""
import numpy as np
import pytest

import locate_chain_ref as LC
import passive_chain_ref as PC


@pytest.fixture(scope="module")
def chain(rts, oracle):
    return PC.host_chain(rts, oracle)


def test_every_receiver_receives_every_body(chain, rts, oracle):
    launches = PC.oracle_launches(rts, oracle)
    n = LC.pair_counts(launches)[:, :PC.N_SURV]
    print("rays per (receiver, body): %d .. %d" % (n.min(), n.max()))
    assert n.min() >= 25 and np.all(n == n[0])      # (the localisation chain holds 100 at W = 100: a quarter of the rays per facet here)
    assert not chain["echoes"][:, :, :PC.K + 8].any()                   # every echo lies beyond the taps
    assert chain["info"] == (1, 0) and not chain["coeffs"][PC.REF].any()


def test_cells_are_where_geometry_puts_them(chain):
    for (r, s), (kd, kl, _) in chain["cells"].items():
        f = LC.doppler_of(s, r) * PC.N_PULSES * PC.PRI
        assert abs((kd - f + 8) % 16 - 8) <= 1.0, (r, s, kd, f)
        assert kl >= PC.K + 8


def test_undetectable_without_cancellation_detected_with_it(chain):
    PC.check_chain(chain)


def test_the_cancellation_removes_what_the_caller_wrote(chain, rts):
    """the caller's terms lie in the span of the lagged copies, so what is left of a surveillance receiver is the projection of its
    echoes and noise off that span: never more energy than they have (a projection contracts; 1e-9 for the rounding), and -- K = 8
    directions out of N P = 7168, 0.1 % of the energy of a vector that knows nothing of them -- no less than 99 % of it"""
    rest = chain["echoes"] + PC.noise(rts)[:PC.N_SURV]
    assert np.abs(PC.caller_terms()).max() > 0.02
    for r in range(PC.N_SURV):
        left, had = np.linalg.norm(chain["clean"][r]), np.linalg.norm(rest[r])
        print("receiver %d: %.6f of the echoes' and the noise's norm is left" % (r, left / had))
        assert 0.99 * had <= left <= had * (1 + 1e-9)
