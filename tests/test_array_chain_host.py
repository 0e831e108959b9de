"""The array, space-time and direction-finding chains on a receive array that the RAY TRACER made (CPU only: the oracle's rays, the
library's host evaluators).  Every other test of these families builds its cube from random numbers or from rts_steering_make's own
rows, so the sign conventions of steering, space-time steering and source injection are tested against themselves there; here the
plane wave comes out of the tracer (tests/array_ref.py: a tilted plate closing by 0.2 wavelengths of two-way length per pulse, seen by
eight elements half a wavelength apart from az = +20 degrees) and the conventions are held to it:

  a  every element receives the same 2200 rays' worth at every pulse;
  b  the conventional beam peaks within a grid step of +20 degrees, with at least 0.99 of (sum_k |z_k|)^2, and holds at most 0.1 of
     the peak at -20 degrees;
  c  Bartlett, Capon and MUSIC peak within a grid step of +20 degrees, at most 0.1 of the peak at -20 degrees;
  d  a bank of four-tap space-time filters peaks at (beam +az, Doppler +0.2 cycles per pulse) -- positive for a closing target, as in
     tests/test_gpu_detect.py --, with at most 0.25 of the peak at (+az, -0.2) and at most 0.1 at (-az, +0.2);
  e  a patch injected by rts_sources_eval at az with doppler = +0.2 / -0.2 peaks at its own sign in the same bank;
  f  MVDR against a noise jammer 30 dB above the target: |w^H s - 1| <= 1e-12, the target's cell at least 20 dB above the mean of the
     others where the conventional beam has at most 10 dB, the cell's power within 10 % of the clean coherent sum, |w^H s_j| <= 1e-3.

Measured here (the library's noise generator, seeds of tests/array_ref.py):
  a  2200 rays in each of the 128 launches
  b  noise-free cube: peak at 20.0 degrees, 0.99986 of (sum |z_k|)^2, 0.00999 at -20 degrees
     noisy cube (20 dB SNR per element; the noise alone costs about (7/8) / (2 SNR) = 0.0044): 20.0 degrees, 0.99482, 0.01293
  c  peak at 20.0 degrees for all three; at -20 degrees Bartlett 0.01293, Capon 0.00364, MUSIC 0.00149
  d  peak at (+az, +0.20); 0.0630 at (+az, -0.20) (the four-tap pattern: 1/16 = 0.0625 without noise); 0.0129 at (-az, +0.20)
  e  doppler +0.2 peaks at (+az, +0.20), doppler -0.2 at (+az, -0.20)
  f  |w^H s - 1| = 2.2e-16; MVDR 29.1 dB, conventional 5.4 dB; cell power 1.0019 of the clean coherent sum; |w^H s_j| = 8.0e-5
     (conventional 2.45e-2)

Flipping the sign of the phase in rts_steering_make mirrors b, c, d and f; flipping the frequency's sign in rts_st_steering_make or in
the sources' pole moves d or e to the other sign."""
import numpy as np
import pytest

import array_ref as AR


@pytest.fixture(scope="module")
def chain(rts, oracle):
    return AR.host_chain(rts, oracle)


def test_every_element_receives_the_same_rays(chain):
    print("rays per launch: min %d, max %d" % (chain["counts"].min(), chain["counts"].max()))
    assert chain["counts"].shape == (AR.N_RX, AR.N_PULSES) and np.all(chain["counts"] == AR.RAYS)
    clean = chain["clean"]
    assert np.count_nonzero(clean) == AR.N_RX * AR.N_PULSES and np.all(clean[:, :, AR.BIN] != 0)


def test_conditions_on_the_traced_array(chain):
    AR.assert_conditions(chain["figures"])


def test_overlapping_spheres_deliver_every_ray_to_the_last_element(rts, oracle, chain):
    """why the recipe is one launch per element: all eight spheres in one receiver list, and every received record carries
    received == 7 with a length that the earlier spheres' entry distances have been added to (quirk 4)"""
    together = AR.oracle_received(rts, oracle, None, 0)
    alone = AR.element_launches(rts, oracle)[(AR.N_RX - 1, 0)]
    print("one launch of eight overlapping spheres: %d records, received in %s" % (len(together), sorted(set(together["received"].tolist()))))
    assert len(together) == AR.RAYS and np.all(together["received"] == AR.N_RX - 1)
    assert len(alone) == AR.RAYS and np.all(together["rayLength"] > alone["rayLength"] + AR.RADIUS)
