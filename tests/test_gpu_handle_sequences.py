"""One handle through many calls: the host-side state the cube kernels are launched from (RtsCubeState, rts_amd/csrc/rts_cube_state.h)
across regrows of its buffers, a short table after a long one, the OS-CFAR alpha cache, the records of every product across the other
products' calls and across rts_cube_attach, and two handles whose calls alternate.  No kernel is new here and no tolerance is: at
every step of every sequence a result is held to

  (a) its host evaluator (the numpy transform of tests/cube_ref.py for the Doppler map), compared as the product's own GPU test
      compares it -- bit for bit for the beams, the covariances, the MVDR weights, the space-time filter, the eigenpairs, the scan and
      the shift table (tests/test_gpu_beam.py, _adapt.py, _stap.py, _doa.py, _focus.py; the phase table within _focus.py's bound), field by field for a detection list (tests/test_gpu_cfar_os.py: BYTE_EQUAL,
      then assert_same_list), byte for byte for plots and tracks (tests/test_gpu_plot.py, _track.py), rtol 1e-10 and atol 1e-12
      max|ref| for the spectrogram, the range transform and the image (tests/test_gpu_stft.py, _beat.py, _image.py), atol 1e-10
      max|cube| sqrt(n_fft) for the Doppler map (tests/test_gpu_cube_edges.py);
  (b) the same call on a handle created for that call alone, byte for byte: what catches plausible stale numbers where (a) is a bound.

1. Grow, shrink, grow.  DevBuf::reserve(n) (rts_amd/csrc/rts_owned.h) keeps a buffer that holds n; otherwise it frees it and allocates
   max(n + n / 8 + 16, 2 cap, 65 536) elements.  So on one handle a first small call leaves cap = 65 536, a call with 65 536 < n <=
   131 072 leaves max(n + n / 8 + 16, 131 072), a small call keeps that, and a call above it regrows again.  Each family's four sizes
   and the capacities they leave are written next to its sequence; the buffers each regrows twice:
     Doppler               doppler.map.own        (doubles: 2 n_rx n_fft n_bins)
     spectrogram, summed   stft.out.own, stft.d_part (n_rx n_frames n_fft; that times the tiles of 8 gate bins, rts_stft_plan)
     range transform       fmcw.range.own         (2 n_rx n_pulses n_out)
     beamform              beam.out.own           (2 n_beams n_rows n_bins)
     covariance / stacked  adapt.d_cov_part       (2 parts D^2, parts = min(ceil(K / 64), 512): rts_cov_plan; adapt.cov.own holds 2 D^2 <= 8 192
                                                   doubles and never leaves its first 65 536)
     space-time apply      stap.out.own           (2 n_filters out_rows n_bins)
     DOA scan              doa.spectrum.own       (n_dirs)
     backprojection, split image.out.own, image.d_scratch (2 n_rx n_y n_x; 2 n_chunks n_rx n_y n_x with n_chunks = ceil(P / 64) > 1 and fewer than
                                                   1 024 workgroups: rts_image_plan)
     OS-CFAR, then plots   detect.d_list (max_detections records), plot.d_key .. d_off, plot.d_list (the list capacity, which is max_detections)
     track                 track.d_zd, d_zf, d_pw, d_zrx, d_of_plot, d_best_d, d_best_t (n_plots), d_flag, d_off (table + n_plots + 1);
                           d_cd, d_cj (16 candidates per track of the table: 16 max_tracks)
   After each large step an older product of the handle is read again through its getter and must hold the bytes it was made with.
   A getter is asked right after the call that regrew its buffer: it returns the new product (both oracles), and a capacity one
   double short of the new size is refused, so the record names the new block and size.  The window between RtsCubeProduct::place
   and ::record is not reachable through the C ABI short of a failing allocation, so "refuses" is checked where it is reachable:
   after rts_cube_attach (part 4).
   NOT exercised: fmcw.d_beat_part.  rts_cube_render_beat reads the received set of a traced pulse and returns before it reserves anything
   when there is none (rts_cube_beat_device: R == 0), and this file traces nothing; the pulse path has its own tests.  Nor detect.d_cnt,
   d_off and d_tmp, which the map's segments size (n_rx n_doppler ceil(n_bins / tile) + 1: past 65 536 only with a map of
   millions of cells, whose evaluator run takes far longer than a test may), nor track.d_pred, d_cn, d_of_track and d_md2, which hold one
   element per track of a table of at most 65 536: their first 65 536 are all they ever need.

2. A short table after a long one.  beam.w, stap.w, adapt.mvdr_s, doa.g, stft.win, fmcw.range_win, image.geo and detect.os_alpha keep one device block; the
   long call fills it with values near 1e6, the short call that follows must not read past its own.

3. The OS-CFAR alpha cache (rts_cube_detect_os: detect.os_tab, os_key, os_pfa, os_sent) through eight calls: a hit, new training
   counts under the same key, pfa, rank and window changed one at a time (the last to a window of the same N0), a fixed alpha, and the
   first key again.  The maps are unit power with cells planted 1e-3 above and below the thresholds of every key in the sequence, so
   a wrong table changes the list itself.

4. One table over all products: records across the other products' calls, the neighbour pairs, caller-owned outputs, rts_cube_attach.

5. Two handles, calls alternating without a fetch, so that one handle's regrow (hipFree, device-wide) meets the other's enqueued work.
"""
import ctypes as C

import numpy as np
import pytest

import adapt_ref as A
import beam_ref as B
import cfar_os_ref as OR
import cube_ref as CR
import plot_ref as PR
import test_image_host as TH
import track_ref as TR
from test_gpu_beam import assert_peak           # the peak form's comparison: power and beam bit for bit, the offset as a range_offset
from test_gpu_cfar_os import BYTE_EQUAL         # the fields a device list shares with the evaluator's byte for byte
from test_gpu_focus import PGA_DEVICE_BOUND     # the PGA against its evaluator: 10 times the evaluator's measured distance from numpy

pytestmark = pytest.mark.gpu


# ----------------------------------------------------------------------------- helpers
def dev(a, dtype=np.complex128):
    """(torch's stream is not the handles': the buffer is finished before a handle reads it)"""
    import torch
    buf = torch.from_numpy(np.array(a, dtype, order="C")).to("cuda")
    torch.cuda.synchronize()
    return buf


def dev_bytes(a):
    import torch
    raw = np.frombuffer(np.ascontiguousarray(a).tobytes() + b"\0" * 8, np.uint8).copy()      # (never empty: an empty tensor has no address)
    buf = torch.from_numpy(raw).to("cuda")
    torch.cuda.synchronize()
    return buf


def filled(n, value, dtype):
    import torch
    buf = torch.full((n,), value, dtype=dtype, device="cuda")
    torch.cuda.synchronize()
    return buf


def bits(a):
    return np.ascontiguousarray(a).view(np.float64)


def blob(x):
    """the bytes of a result: an array, a structured array, or a tuple of them and integers (tracks(): the table and the next id)"""
    if isinstance(x, tuple):
        return b"|".join(blob(y) for y in x)
    if isinstance(x, (int, np.integer)):
        return int(x).to_bytes(8, "little")
    return np.ascontiguousarray(x).tobytes()


def exact(got, want, what=""):
    """bit for bit, as the product's own test compares it with its evaluator"""
    if isinstance(want, tuple):
        assert len(got) == len(want), what
        for k, (g, w) in enumerate(zip(got, want)):
            exact(g, w, (what, k))
        return
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape)
    assert np.all(np.isfinite(bits(got))) and np.array_equal(bits(got), bits(want)), what


def bound(got, ref, what=""):
    """the project's bound for a kernel against its evaluator (tests/test_gpu_stft.py, test_gpu_beat.py, test_gpu_image.py)"""
    assert got.shape == ref.shape and got.dtype == ref.dtype, (what, got.shape, ref.shape)
    np.testing.assert_allclose(got, ref, rtol=1e-10, atol=1e-12 * np.abs(ref).max(), err_msg=str(what))


def pga_bound(got, want, what=""):
    """tests/test_gpu_focus.py: the phase table and the iterations' rms within PGA_DEVICE_BOUND of the evaluator's"""
    assert len(got) == len(want) == 2
    for g, w in zip(got, want):
        assert g.shape == w.shape and np.all(np.isfinite(g)) and np.abs(g - w).max() <= PGA_DEVICE_BOUND, what


def doppler_bound(got, cube, n_fft, what=""):
    """tests/test_gpu_cube_edges.py: test_doppler_transform_sizes"""
    ref = CR.to_double(CR.dft_ref(cube, n_fft))
    assert got.shape == ref.shape
    np.testing.assert_allclose(got, ref, rtol=0, atol=1e-10 * np.abs(cube).max() * np.sqrt(n_fft), err_msg=str(what))


def same_list(rts, got, z, what="", t0=0.0, dt=1.0, **par):
    """a detection list against rts_cfar_os_eval on the host map z, as tests/test_gpu_cfar_os.py compares them"""
    want = rts.cfar_os_eval(z, t0=t0, dt=dt, **par)
    assert len(got) == len(want), (what, len(got), len(want))
    for f in BYTE_EQUAL:
        assert got[f].tobytes() == want[f].tobytes(), (what, f)
    OR.assert_same_list(got, want)
    return want


def attached(rts, dcube, shape, t0=0.0, dt=1.0):
    tr = rts.Tracer(8, 1)
    tr.cube_attach(shape[0], shape[1], shape[2], t0, dt, device_ptr=dcube.data_ptr() if dcube is not None else None)
    return tr


def both(used, fresh, call, want, compare, what):
    """one step: `call` on the used handle against the evaluator's `want` (a), then on a handle made for it alone, byte for byte (b)"""
    got = call(used)
    compare(got, want, what)
    f = fresh()
    try:
        again = call(f)
    finally:
        f.close()
    assert blob(got) == blob(again), "%s: the used handle's bytes are not a fresh handle's" % (what,)
    return got


def doppler_get(rts, tr, shape):
    """rts_cube_doppler_get alone (Tracer.cube_doppler is the call and the getter)"""
    out = np.zeros(tuple(shape) + (2,), np.float64)
    rts.L.check(rts.L.lib().rts_cube_doppler_get(tr.h, rts.ptr(out), out.size))
    return out[..., 0] + 1j * out[..., 1]


def one_short_is_refused(rts, tr, getter, doubles):
    """the record's size is the last call's: a capacity one double short is refused and nothing is written"""
    out = np.full(4, 7.25)
    assert getattr(rts.L.lib(), getter)(tr.h, rts.ptr(out), int(doubles) - 1) == rts.L.RTS_ERR_CAPACITY, getter
    assert np.all(out == 7.25)


class Older:
    """a product made before the sequence: read again after each large step, it holds the bytes it was made with"""

    def __init__(self, made, get):
        self.bytes, self.get = blob(made), get
        assert self.bytes == blob(get())

    def still(self, what=""):
        assert blob(self.get()) == self.bytes, "%s: an older product changed" % (what,)


def random_window(rng, n, scale=1.0):
    return (rng.random(n) + 0.5) * scale


# ============================================================================= 1. grow, shrink, grow
def test_regrow_doppler(rts):
    """doppler.own, doubles = 2 * 1 * n_fft * 137: n_fft 4 -> 1 096 (cap 65 536), 256 -> 70 144 (cap 131 072), 4 -> 1 096 (kept),
    512 -> 140 288 (cap 262 144).  The older product is a beam map."""
    rng = np.random.default_rng(101)
    shape = (1, 2, 137)
    cube = B.random_complex(rng, shape); d = dev(cube)
    fresh = lambda: attached(rts, d, shape)
    tr = fresh()
    w = B.random_complex(rng, (3, 1))
    older = Older(tr.cube_beamform(w), tr.beam_map)
    for n_fft in (4, 256, 4, 512):
        got = both(tr, fresh, lambda t: t.cube_doppler(n_fft), cube, lambda g, c, what: doppler_bound(g, c, n_fft, what), ("doppler", n_fft))
        assert blob(doppler_get(rts, tr, got.shape)) == blob(got)
        one_short_is_refused(rts, tr, "rts_cube_doppler_get", 2 * got.size)
        if n_fft > 4:
            older.still(n_fft)
    tr.close()


def test_regrow_spectrogram_summed(rts):
    """RTS_STFT_SUM_BINS over a gate of 9 bins (two tiles of 8: the tile sums go through d_stft_part), n_rx = 2, window_len 2, hop 1.
    stft.own = 2 n_frames n_fft doubles, d_stft_part = twice that:
      n_fft 64, 1 frame      128 and     256   (cap 65 536 both)
      n_fft 4 096, 9 frames  73 728 and 147 456 (cap 131 072 and 147 456 + 18 432 + 16 = 165 904)
      n_fft 64, 1 frame      kept
      n_fft 4 096, 18 frames 147 456 and 294 912 (above 131 072 and 165 904: both regrow)"""
    rng = np.random.default_rng(102)
    shape = (2, 20, 9)
    cube = B.random_complex(rng, shape); d = dev(cube)
    fresh = lambda: attached(rts, d, shape)
    tr = fresh()
    older = Older(tr.cube_doppler(32), lambda: doppler_get(rts, tr, (2, 32, 9)))
    win = random_window(rng, 2)
    for n_fft, count in ((64, 2), (4096, 10), (64, 2), (4096, 19)):
        kw = dict(window=win, first=1 if count < 19 else 0, count=count, power=True, sum_bins=True)
        want = rts.stft_eval(cube, 2, 1, n_fft, **kw)
        assert want.shape == (2, count - 1, n_fft)
        got = both(tr, fresh, lambda t: t.cube_spectrogram(2, 1, n_fft, **kw), want, bound, ("stft", n_fft, count))
        assert blob(tr.spectrogram()) == blob(got)
        one_short_is_refused(rts, tr, "rts_cube_spectrogram_get", got.size)
        if n_fft > 64:
            older.still((n_fft, count))
    tr.close()


def test_regrow_range_transform(rts):
    """range.own, doubles = 2 * 2 * count * n_out: (n_fft 1 024, 1 row, n_out 250) -> 1 000 (cap 65 536), (4 096, 5 rows, every bin)
    -> 81 920 (cap 131 072), the first again (kept), (4 096, 9 rows) -> 147 456 (cap 262 144)"""
    rng = np.random.default_rng(103)
    shape = (2, 9, 547)
    cube = B.random_complex(rng, shape); d = dev(cube)
    fresh = lambda: attached(rts, d, shape)
    tr = fresh()
    older = Older(tr.cube_doppler(16), lambda: doppler_get(rts, tr, (2, 16, 547)))
    win = random_window(rng, 547)
    for n_fft, count, n_out in ((1024, 1, 250), (4096, 5, 0), (1024, 1, 250), (4096, 9, 0)):
        kw = dict(window=win, first=9 - count, count=count, n_out=n_out, reverse=count == 5)
        want = rts.range_eval(cube, n_fft, **kw)
        got = both(tr, fresh, lambda t: t.cube_range_transform(n_fft, **kw), want, bound, ("range", n_fft, count))
        assert blob(tr.range_map()) == blob(got)
        one_short_is_refused(rts, tr, "rts_cube_range_get", 2 * got.size)
        if count > 1:
            older.still((n_fft, count))
    tr.close()


def test_regrow_beamform(rts):
    """beam.own, doubles = 2 * n_beams * 1 row * 547: 1 beam -> 1 094 (cap 65 536), 64 -> 70 016 (cap 131 072), 1 (kept),
    128 -> 140 032 (cap 262 144)"""
    rng = np.random.default_rng(104)
    shape = (2, 3, 547)
    cube = B.random_complex(rng, shape); d = dev(cube)
    fresh = lambda: attached(rts, d, shape)
    tr = fresh()
    older = Older(tr.cube_doppler(4), lambda: doppler_get(rts, tr, (2, 4, 547)))
    for n_beams in (1, 64, 1, 128):
        w = B.random_complex(rng, (n_beams, 2))
        want = rts.beamform_eval(cube, w, first=1, count=1)
        got = both(tr, fresh, lambda t: t.cube_beamform(w, first=1, count=1), want, exact, ("beam", n_beams))
        assert blob(tr.beam_map()) == blob(got)
        one_short_is_refused(rts, tr, "rts_cube_beam_get", 2 * got.size)
        if n_beams > 1:
            older.still(n_beams)
    tr.close()


def test_regrow_covariance_parts(rts):
    """d_cov_part = 2 * parts * D^2 doubles, parts = ceil(K / 64) tiles (below the cap of 512), on a cube of 4 receivers and 300 bins:
      the receivers' covariance, 2 rows of 33 bins      D = 4,  K = 66,    2 parts ->      64 (cap 65 536)
      16 taps stacked, a span of 17 rows                D = 64, K = 600,   10 parts ->  81 920 (cap 131 072)
      the first again                                                                          (kept; the order goes back to 4)
      16 taps stacked, a span of 19 rows                D = 64, K = 1 200, 19 parts -> 155 648 (cap 262 144)
    The weights and the eigenpairs of each step follow the covariance the step made (rts_cube_mvdr, rts_cube_eig without device_cov)."""
    rng = np.random.default_rng(105)
    shape = (4, 20, 300)
    cube = B.random_complex(rng, shape); d = dev(cube)
    fresh = lambda: attached(rts, d, shape)
    tr = fresh()
    older = Older(tr.cube_doppler(32), lambda: doppler_get(rts, tr, (4, 32, 300)))
    for taps, count in ((1, 2), (16, 17), (1, 2), (16, 19)):
        D = 4 * taps
        s = B.random_complex(rng, (3, D))
        if taps == 1:
            train = dict(first=1, count=count, first_bin=5, n_bins=33)
            cov_h = rts.covariance_eval(cube, **train)
            make = lambda t: t.cube_covariance(**train)
        else:
            train = dict(first=20 - count, count=count)
            cov_h = rts.st_covariance_eval(cube, taps, **train)
            make = lambda t: t.cube_st_covariance(taps, **train)
        want = (cov_h, rts.mvdr_eval(cov_h, s, 0.5)) + rts.eig_eval(cov_h)
        got = both(tr, fresh, lambda t: (make(t), t.cube_mvdr(s, 0.5)) + t.cube_eig(), want, exact, ("covariance", taps, count))
        assert got[0].shape == (D, D) and blob(tr.covariance()) == blob(got[0]) and blob(tr.mvdr_weights()) == blob(got[1])
        one_short_is_refused(rts, tr, "rts_cube_covariance_get", 2 * D * D)
        if taps > 1:
            older.still((taps, count))
    tr.close()


def test_regrow_st_apply(rts):
    """st.own, doubles = 2 * n_filters * out_rows * 300 with 2 taps: (1 filter, 2 rows -> 1 output row) -> 600 (cap 65 536), (8 filters,
    16 rows -> 15) -> 72 000 (cap 131 072), the first again (kept), (16 filters, 16 rows) -> 144 000 (cap 262 144)"""
    rng = np.random.default_rng(106)
    shape = (4, 20, 300)
    cube = B.random_complex(rng, shape); d = dev(cube)
    fresh = lambda: attached(rts, d, shape)
    tr = fresh()
    older = Older(tr.cube_beamform(B.random_complex(rng, (2, 4)), first=3, count=2), tr.beam_map)
    for n_filters, count in ((1, 2), (8, 16), (1, 2), (16, 16)):
        w = B.random_complex(rng, (n_filters, 8))
        want = rts.st_apply_eval(cube, w, 2, first=2, count=count)
        got = both(tr, fresh, lambda t: t.cube_st_apply(w, 2, first=2, count=count), want, exact, ("st_apply", n_filters, count))
        assert blob(tr.st_map()) == blob(got)
        one_short_is_refused(rts, tr, "rts_cube_st_get", 2 * got.size)
        if n_filters > 1:
            older.still((n_filters, count))
    tr.close()


def test_regrow_doa_scan(rts):
    """doa.own = n_dirs doubles with vectors of 2 elements: 1 000 (cap 65 536), 70 000 (cap 131 072), 1 000 (kept), 140 000 (cap 262 144)"""
    rng = np.random.default_rng(107)
    shape = (2, 2, 5)
    cube = B.random_complex(rng, shape); d = dev(cube)
    fresh = lambda: attached(rts, d, shape)
    tr = fresh()
    older = Older(tr.cube_doppler(2), lambda: doppler_get(rts, tr, (2, 2, 5)))
    vectors = B.random_complex(rng, (2, 2)); dv = dev(vectors)
    for n_dirs in (1000, 70000, 1000, 140000):
        table = B.random_complex(rng, (n_dirs, 2)); dt = dev(np.ascontiguousarray(table.T))
        g = rng.random(2) + 0.25
        want = rts.doa_scan_eval(vectors, g, table, n_dirs > 1000)
        kw = dict(inverse=n_dirs > 1000, n_dirs=n_dirs, device_vectors=dv.data_ptr(), n=2)
        got = both(tr, fresh, lambda t: t.cube_doa_scan(dt.data_ptr(), g, **kw), want, exact, ("doa", n_dirs))
        assert blob(tr.doa_spectrum()) == blob(got)
        one_short_is_refused(rts, tr, "rts_cube_doa_get", got.size)
        if n_dirs > 1000:
            older.still(n_dirs)
    tr.close()


def test_regrow_backprojection_split(rts):
    """65 pulses are two chunks of 64, and an image of fewer than 1 024 workgroups (16 x 16 pixels each) puts the chunks on the grid
    (rts_image_plan: split), their sums in d_img_scratch.  One receiver: image.own = 2 n_y n_x doubles, d_img_scratch = twice that:
      7 x 5         70 and     140 (cap 65 536 both; 1 workgroup)
      188 x 188     70 688 and 141 376 (cap 131 072 and 141 376 + 17 672 + 16 = 159 064; 144 workgroups)
      7 x 5         kept
      265 x 265     140 450 and 280 900 (above 131 072 and 159 064: both regrow; 289 workgroups)
    Two taps keep the evaluator quick; the grid's extent is the same at every size."""
    P = 65
    cube = TH.random_cube(108, n_rx=1, rows=70)
    d = dev(cube)
    g0 = TH.geometry(P, n_rx=1)
    fresh = lambda: attached(rts, d, cube.shape, g0["t0"], g0["dt"])
    tr = fresh()
    older = Older(tr.cube_doppler(128), lambda: doppler_get(rts, tr, (1, 128, cube.shape[2])))
    for n_x, n_y in ((7, 5), (188, 188), (7, 5), (265, 265)):
        g = dict(g0, n_x=n_x, n_y=n_y, step_x=(18.2 / n_x, 0.0, 0.0), step_y=(0.35 / n_y, 5.0 / n_y, 0.0))
        want = TH.call_eval(rts, cube, g, 2, 3)
        assert np.count_nonzero(want) > 20
        call = lambda t: t.cube_backproject(g["origin"], g["step_x"], g["step_y"], n_x, n_y, g["tx"], g["rx"], g["c"], g["fc"], taps=2, first=3)
        got = both(tr, fresh, call, want, bound, ("image", n_x, n_y))
        assert blob(tr.image()) == blob(got)
        one_short_is_refused(rts, tr, "rts_cube_image_get", 2 * got.size)
        if n_x > 7:
            older.still((n_x, n_y))
    tr.close()


def blob_map(shift, n_rx=2, nd=16, nb=96):
    """a unit background with four bright blobs, moved by `shift` range bins (tests/test_gpu_track.py)"""
    z = np.ones((n_rx, nd, nb), np.complex128)
    for rx, k, r, hk, hr, amp in [(0, 0, 20, 1, 2, 30.0), (0, 8, 40, 1, 1, 20.0), (1, 5, 50, 2, 1, 25.0), (1, 12, 80, 1, 1, 40.0)]:
        for dk in range(-hk, hk + 1):
            for dr in range(-hr, hr + 1):
                z[rx, (k + dk) % nd, r + shift + dr] = amp / (1 + abs(dk) + abs(dr))
    return z


def test_regrow_detections_then_plots(rts):
    """d_det holds max_detections records and the plots' buffers the list's capacity, which is max_detections too: 1 000 (cap
    65 536), 70 000 (cap 131 072), 1 000 (kept), 140 000 (cap 262 144); d_plot_flag and d_plot_off hold one element more.  The map is a
    caller's and changes with the step, so a list or a plot left over from the step before is another one."""
    n_rx, nd, nb = 2, 16, 96
    par = dict(guard=(1, 1), train=(4, 2), rank=30, alpha=6.0, local_max=False, pri=PR.PRI)
    maps = {s: blob_map(s) for s in (0, 3)}
    dmaps = {s: dev(z) for s, z in maps.items()}
    fresh = lambda: attached(rts, None, (n_rx, 1, nb), PR.T0, PR.DT)
    tr = fresh()
    older = Older(tr.cube_doppler(2), lambda: doppler_get(rts, tr, (n_rx, 2, nb)))
    for max_det, shift in ((1000, 0), (70000, 3), (1000, 0), (140000, 3)):
        z, dz = maps[shift], dmaps[shift]
        want_det = rts.cfar_os_eval(z, t0=PR.T0, dt=PR.DT, **par)
        want_plots = rts.plots_eval(want_det, nd, (1, 1), 1, pri=PR.PRI, t0=PR.T0, dt=PR.DT, n_rx=n_rx, n_bins=nb)
        assert len(want_plots) == 4 and 4 < len(want_det) < 1000

        def call(t):
            det = t.cube_detect_os(device_ptr=dz.data_ptr(), n_doppler=nd, max_detections=max_det, **par)
            return det, t.cube_plots((1, 1), pri=PR.PRI)

        def compare(got, want, what):
            same_list(rts, got[0], z, what, PR.T0, PR.DT, **par)
            PR.same_bytes(got[1], want_plots)
        got = both(tr, fresh, call, None, compare, ("detections", max_det))
        assert blob(tr.detections()) == blob(got[0]) and blob(tr.plots()) == blob(got[1])
        if max_det > 1000:
            older.still(max_det)
    tr.close()


def test_regrow_track_plots(rts):
    """A device_plots list of n_plots records sizes d_trk_zd, _zf, _pw, _zrx, _of_plot, _best_d and _best_t (n_plots elements) and
    d_trk_flag, _off (16 384 + n_plots + 1): 1 000 (cap 65 536 all), 70 000 (cap 131 072), 1 000 (kept), 140 000 (cap 262 144).  The
    frames are those of tests/track_ref.py's sequence; the surplus records have a NaN delay, which the step ignores.  The table
    lives in buffers of full size from the start (a DevBuf that grows drops what it held): it is carried on the device alone
    through the regrows and compared with the evaluator chained on the host."""
    frames = TR.sequence(0)[:4]
    tr = rts.Tracer(8, 1)
    tab, nid = np.zeros(0, TR.TRACK), 0
    for n, (z, n_plots) in enumerate(zip(frames, (1000, 70000, 1000, 140000))):
        plots = np.zeros(n_plots, TR.PLOT)
        plots[:len(z)] = z
        plots["rx"][len(z):] = z["rx"].max(); plots["delay"][len(z):] = np.nan
        buf = dev_bytes(plots)
        time, prev = TR.SEQ_T * n, TR.SEQ_T * (n - 1)
        got, got_id = tr.cube_track(time, device_plots=buf.data_ptr(), n_plots=n_plots, **TR.SEQ_PAR)
        f = rts.Tracer(8, 1)                                    # (b): the table as it stood, loaded into a handle of its own
        f.cube_tracks_set(tab, nid, prev)
        again, again_id = f.cube_track(time, device_plots=buf.data_ptr(), n_plots=n_plots, **TR.SEQ_PAR)
        f.close()
        tab, nid = rts.tracks_eval(tab, nid, time - prev, plots, **TR.SEQ_PAR)
        TR.same_bytes(got, tab)
        assert got_id == nid and len(tab) >= len(z)
        assert blob((got, got_id)) == blob((again, again_id)) == blob(tr.tracks()), n_plots
    tr.close()


def test_regrow_track_candidates(rts):
    """d_trk_cd and d_trk_cj hold RTS_TRACK_MAX_CAND = 16 entries per track of the TABLE.  A loaded table (rts_cube_tracks_set) lets the
    next step choose the table's size: max_tracks 1 000 -> 16 000 elements (cap 65 536), the default 16 384 -> 262 144 (cap 262 144 +
    32 768 + 16 = 294 928), 1 000 (kept), 65 536 -> 1 048 576 (cap 1 179 664); d_trk_flag and _off (max_tracks + 500 plots + 1) pass
    65 536 at the last.  tests/track_ref.py's random_grid case: 300 tracks, 500 plots, ties."""
    c = TR.case("random_grid")
    buf = dev_bytes(c["plots"])
    tr = rts.Tracer(8, 1)
    for max_tracks in (1000, 0, 1000, 65536):
        par = dict(c["par"], max_tracks=max_tracks)
        want, want_id = rts.tracks_eval(c["tracks"], c["next_id"], c["T"], c["plots"], **par)
        assert 300 < len(want) < 1000

        def call(t):
            t.cube_tracks_set(c["tracks"], c["next_id"], 0.0)
            return t.cube_track(c["T"], device_plots=buf.data_ptr(), n_plots=len(c["plots"]), **par)

        def compare(got, _, what):
            TR.same_bytes(got[0], want)
            assert got[1] == want_id, what
        both(tr, lambda: rts.Tracer(8, 1), call, None, compare, ("track table", max_tracks))
    tr.close()


# ============================================================================= 2. a short table after a long one
BIG = 1.0e6


def test_short_weights_after_long_beamform_and_st_apply(rts):
    """beam_w and st_w hold RTS_BEAM_MAX_WEIGHTS = 4 096 weights: 1 024 beams (512 filters of 2 taps) over 4 receivers, then one"""
    rng = np.random.default_rng(201)
    shape = (4, 3, 67)
    cube = B.random_complex(rng, shape); d = dev(cube)
    fresh = lambda: attached(rts, d, shape)
    tr = fresh()
    for n_beams in (1024, 1):
        w = B.random_complex(rng, (n_beams, 4)) * (BIG if n_beams > 1 else 1.0)
        for form in (dict(), dict(power=True), dict(peak=True)):
            want = rts.beamform_eval(cube, w, **form)
            both(tr, fresh, lambda t: t.cube_beamform(w, **form), want, exact if "peak" not in form else assert_peak, ("beam", n_beams, form))
    for n_filters in (512, 1):
        w = B.random_complex(rng, (n_filters, 8)) * (BIG if n_filters > 1 else 1.0)
        for power in (False, True):
            want = rts.st_apply_eval(cube, w, 2, power=power)
            both(tr, fresh, lambda t: t.cube_st_apply(w, 2, power=power), want, exact, ("st_apply", n_filters, power))
    tr.close()


def test_short_steering_after_long_mvdr(rts):
    """mvdr_s: 1 024 steering rows over 4 receivers, then one, against the library-owned covariance"""
    rng = np.random.default_rng(202)
    shape = (4, 3, 67)
    cube = B.random_complex(rng, shape); d = dev(cube)
    fresh = lambda: attached(rts, d, shape)
    tr = fresh()
    cov_h = rts.covariance_eval(cube)
    for n_beams in (1024, 1):
        s = B.random_complex(rng, (n_beams, 4)) * (BIG if n_beams > 1 else 1.0)
        want = rts.mvdr_eval(cov_h, s, 0.25)

        def call(t):
            t.cube_covariance(fetch=False)
            return t.cube_mvdr(s, 0.25)
        both(tr, fresh, call, want, exact, ("mvdr", n_beams))
    tr.close()


def test_short_g_after_long_doa_scan(rts):
    """doa_g: 64 weights over 64 vectors, then one"""
    rng = np.random.default_rng(203)
    n, n_dirs = 64, 130
    vectors = B.random_complex(rng, (n, n)); dv = dev(vectors)
    table = B.random_complex(rng, (n_dirs, n)); dt = dev(np.ascontiguousarray(table.T))
    fresh = lambda: attached(rts, None, (1, 1, 1))
    tr = fresh()
    for m, first in ((n, 0), (1, 17)):
        g = (rng.random(m) + 0.25) * (BIG if m > 1 else 1.0)
        want = rts.doa_scan_eval(vectors[first:first + m], g, table)
        kw = dict(first_vector=first, n_dirs=n_dirs, device_vectors=dv.data_ptr(), n=n)
        both(tr, fresh, lambda t: t.cube_doa_scan(dt.data_ptr(), g, **kw), want, exact, ("doa", m))
    tr.close()


def test_short_window_after_long_spectrogram_and_range(rts):
    """stft_win and range_win hold 4 096 values: a window of 4 096, then of one"""
    rng = np.random.default_rng(204)
    for axis in ("slow", "fast"):
        shape = (1, 4096, 1) if axis == "slow" else (1, 1, 4096)
        cube = B.random_complex(rng, shape); d = dev(cube)
        fresh = lambda: attached(rts, d, shape)
        tr = fresh()
        for n in (4096, 1):
            win = random_window(rng, n, BIG if n > 1 else 1.0)
            n_fft = max(n, 2)
            if axis == "slow":
                for form in (dict(), dict(power=True), dict(power=True, sum_bins=True)):
                    kw = dict(window=win, first=4096 - n, count=n, **form)
                    want = rts.stft_eval(cube, n, 1, n_fft, **kw)
                    both(tr, fresh, lambda t: t.cube_spectrogram(n, 1, n_fft, **kw), want, bound, ("stft window", n, form))
            else:
                kw = dict(window=win, first_bin=4096 - n, n_samples=n)
                want = rts.range_eval(cube, n_fft, **kw)
                both(tr, fresh, lambda t: t.cube_range_transform(n_fft, **kw), want, bound, ("range window", n))
        tr.close()


def test_short_geometry_after_long_backprojection(rts):
    """img_geo holds [tx | rx | weight] of the call's pulses: 129 pulses with weights near 1e6, then one pulse"""
    cube = TH.random_cube(205, rows=130)
    d = dev(cube)
    g129 = TH.geometry(129)
    fresh = lambda: attached(rts, d, cube.shape, g129["t0"], g129["dt"])
    tr = fresh()
    for P, first in ((129, 1), (1, 64)):
        g = dict(g129, tx=g129["tx"][first - 1:first - 1 + P], rx=g129["rx"][:, first - 1:first - 1 + P])
        weights = TH.hann(P) * BIG if P > 1 else np.array([0.75])
        want = TH.call_eval(rts, cube, g, 8, first, weights)
        assert np.count_nonzero(want) > 0
        call = lambda t: t.cube_backproject(g["origin"], g["step_x"], g["step_y"], g["n_x"], g["n_y"], g["tx"], g["rx"], g["c"], g["fc"], taps=8, first=first,
                                            weights=weights)
        both(tr, fresh, call, want, bound, ("image geometry", P))
    tr.close()


def test_short_alpha_table_after_long(rts):
    """os_alpha holds RTS_CFAR_OS_MAX_TRAIN + 1 alphas: the window of 1 088 training cells (tests/cfar_os_ref.py, case 2's), then the
    smallest window there is, one training cell on either side in range"""
    rng = np.random.default_rng(206)
    n_rx, nd, nb = 1, 33, 70
    z = OR.planted_map(rng, n_rx, nd, nb); dz = dev(z)
    fresh = lambda: attached(rts, None, (n_rx, 1, nb))
    tr = fresh()
    for par in (dict(guard=(0, 0), train=(16, 16), rank=816, pfa=1e-6, local_max=False), dict(guard=(0, 0), train=(1, 0), rank=2, pfa=0.05, local_max=False)):
        assert rts.cfar_os_n0(par["guard"], par["train"]) in (1088, 2)
        want = rts.cfar_os_eval(z, **par)
        assert 5 <= len(want) < z.size // 4
        both(tr, fresh, lambda t: t.cube_detect_os(device_ptr=dz.data_ptr(), n_doppler=nd, **par), None, lambda got, _, what: same_list(rts, got, z, what, **par),
             ("alpha table", par["train"]))
    tr.close()


# ============================================================================= 3. the OS-CFAR alpha cache
def train_counts(guard, train, nb):
    """the training cells of a cell at each range bin (the Doppler axis wraps, the range axis is cut: include/rts_amd.h)"""
    (gr, gd), (tr_, td) = guard, train
    r = np.arange(nb)
    cols = np.minimum(r + gr + tr_, nb - 1) - np.maximum(r - gr - tr_, 0) + 1
    inner = np.minimum(r + gr, nb - 1) - np.maximum(r - gr, 0) + 1
    return cols * (2 * (gd + td) + 1) - inner * (2 * gd + 1)


def thresholds(rts, par, nb):
    """the threshold of each range bin of a unit-power map: alpha times a noise estimate of exactly 1"""
    if par.get("alpha"):
        return np.full(nb, par["alpha"])
    n0 = rts.cfar_os_n0(par["guard"], par["train"])
    return np.array([rts.cfar_os_alpha(m, (par["rank"] * m + n0 - 1) // n0, par["pfa"]) for m in train_counts(par["guard"], par["train"], nb)])


ROW_STEP = 12          # Doppler rows between planted rows: more than the tallest window of the sequence (2 * 4 + 1 = 9 rows)


def planted_unit_map(rts, sets, nb, bins):
    """unit power everywhere but for cells 1e-3 above and 1e-3 below the threshold of each parameter set at each of `bins`, one row per
    (set, sign): at most two planted cells lie in any window, so the order statistic of every cell stays exactly 1.
    Returns (the map [1][nd][nb], {(row, bin): power})"""
    nd = ROW_STEP * 2 * len(sets)
    z = np.ones((1, nd, nb), np.complex128)
    planted = {}
    for i, par in enumerate(sets):
        thr = thresholds(rts, par, nb)
        for j, sign in enumerate((1.0, -1.0)):
            k = ROW_STEP * (2 * i + j) + 3
            for r in bins:
                amp = np.sqrt(thr[r] * (1.0 + sign * 1e-3))
                z[0, k, r] = amp
                planted[(k, r)] = amp * amp
    return z, planted


def expected_cells(rts, par, planted, nb):
    thr = thresholds(rts, par, nb)
    for (k, r), p in planted.items():
        assert abs(p - thr[r]) > 1e-9 * thr[r], "a planted cell lies on a threshold"
    return sorted((k, r) for (k, r), p in planted.items() if p > thr[r])


def cells(det):
    return sorted(zip(det["doppler_bin"].tolist(), det["range_bin"].tolist()))


def test_os_alpha_cache(rts):
    nb, nb_cut = 48, 4
    K1 = dict(guard=(1, 1), train=(2, 2))
    n0 = rts.cfar_os_n0(K1["guard"], K1["train"])
    # a window of the same N0 under another key (step 6), the first in this order whose height fits between the planted rows
    K6 = next(dict(guard=(gr, gd), train=(t_r, td)) for gr in range(3) for gd in range(3) for t_r in range(5) for td in range(5)
              if t_r + td > 0 and rts.cfar_os_n0((gr, gd), (t_r, td)) == n0 and ((gr, gd), (t_r, td)) != (K1["guard"], K1["train"]) and 2 * (gd + td) + 1 < ROW_STEP)
    assert rts.cfar_os_n0(K6["guard"], K6["train"]) == rts.cfar_os_n0(K1["guard"], K1["train"]) == 40 and K6 != K1
    p1, p2, r1, r2 = 1e-3, 1e-4, 30, 24
    S1, S4, S5 = dict(K1, rank=r1, pfa=p1), dict(K1, rank=r1, pfa=p2), dict(K1, rank=r2, pfa=p2)
    S6, S7 = dict(K6, rank=r2, pfa=p2), dict(K6, rank=r2, alpha=3.0)
    sets = [S1, S4, S5, S6, S7]
    z, planted = planted_unit_map(rts, sets, nb, (0, 1, nb // 2))
    z_cut, planted_cut = planted_unit_map(rts, [S1], nb_cut, (0, 1))
    dz, dz_cut = dev(z), dev(z_cut)
    # step 3 meets training counts step 1 never solved, step 6 counts that the first key never had: their table entries are 0 until solved,
    # and a zero alpha reports every cell of the bin
    counts1, counts_cut, counts6 = (set(train_counts(k["guard"], k["train"], n).tolist()) for k, n in ((K1, nb), (K1, nb_cut), (K6, nb)))
    assert counts_cut - counts1 and counts6 - counts1
    assert train_counts(K1["guard"], K1["train"], nb_cut)[1] not in counts1 and train_counts(K6["guard"], K6["train"], nb)[1] not in counts1
    #        parameters, the map, the step whose table a stale cache would apply (None: the same list is expected)
    steps = [(S1, "full", None), (S1, "full", None), (S1, "cut", None), (S4, "full", S1), (S5, "full", S4), (S6, "full", S5), (S7, "full", S6), (S1, "full", S7)]
    tr = rts.Tracer(8, 1)
    tr.cube_attach(1, 1, nb, 0.0, 1.0)
    shape_now = nb
    for n, (par, which, stale) in enumerate(steps):
        zz, dzz, pl, bins = (z, dz, planted, nb) if which == "full" else (z_cut, dz_cut, planted_cut, nb_cut)
        if bins != shape_now:
            tr.cube_attach(1, 1, bins, 0.0, 1.0); shape_now = bins
        kw = dict(local_max=False, **par)
        want = rts.cfar_os_eval(zz, **kw)
        assert cells(want) == expected_cells(rts, par, pl, bins) and np.all(want["noise"] == 1.0), n        # the map does what it was built for
        below = [(k, r) for (k, r), p in pl.items() if r == 1 and (k, r) not in cells(want)]
        assert len(want) >= 2 and below, n                     # cells above and below; one below at the bin whose count is new in steps 3 and 6
        if stale is not None:                                 # the previous table would give another list: the test cannot pass on a stale one
            assert cells(rts.cfar_os_eval(zz, local_max=False, **stale)) != cells(want), n
        got = tr.cube_detect_os(device_ptr=dzz.data_ptr(), n_doppler=zz.shape[1], **kw)
        same_list(rts, got, zz, ("alpha cache step", n + 1), **kw)
        f = rts.Tracer(8, 1); f.cube_attach(1, 1, bins, 0.0, 1.0)
        again = f.cube_detect_os(device_ptr=dzz.data_ptr(), n_doppler=zz.shape[1], **kw)
        f.close()
        assert blob(got) == blob(again), n
    tr.close()


# ============================================================================= 4. records across other products and across attach
class Table:
    """every product of one cube: name -> (make on a handle, its getter, the evaluator's result, the comparison).  The dependent
    products (weights, eigenpairs, spectrum, plots) follow the library-owned product before them, as include/rts_amd.h states."""

    def __init__(self, rts, seed):
        rng = np.random.default_rng(seed)
        self.rts, self.shape = rts, (3, 8, 40)
        self.cube = c = B.random_complex(rng, self.shape)
        c[0, :, 20] *= 40.0; c[2, :, 31] *= 30.0                                  # two range bins that stand out of the map in every Doppler row
        self.d = dev(c)
        w = B.random_complex(rng, (2, 3)); s = B.random_complex(rng, (2, 3)); wst = B.random_complex(rng, (2, 6))
        win = random_window(rng, 4); rwin = random_window(rng, 40)
        table = B.random_complex(rng, (33, 3)); self.dtable = dev(np.ascontiguousarray(table.T))
        g = TH.geometry(5, n_x=6, n_y=4, n_rx=3, nb=40)
        g["rx"] = np.stack([g["tx"], g["tx"] + (10.0, 5.0, -5.0), g["tx"] + (-7.0, 3.0, 2.0)])
        self.t0, self.dt = g["t0"], g["dt"]
        os_par = dict(guard=(1, 0), train=(3, 1), rank=9, pfa=1e-2, local_max=False, pri=1e-3)
        dmap = CR.to_double(CR.dft_ref(c, 8))
        cov = rts.covariance_eval(c, first=1, count=6)
        vals, vecs = rts.eig_eval(cov)
        gd = np.array([0.5, 1.5])
        self.os_par, self.n_fft = os_par, 8
        image = lambda t: t.cube_backproject(g["origin"], g["step_x"], g["step_y"], 6, 4, g["tx"], g["rx"], g["c"], g["fc"], taps=2, first=2)
        self.rows = [
            ("doppler", lambda t: t.cube_doppler(8), lambda t: doppler_get(rts, t, (3, 8, 40)), c, lambda got, cube, what: doppler_bound(got, cube, 8, what)),
            ("spectrogram", lambda t: t.cube_spectrogram(4, 2, 4, window=win), lambda t: t.spectrogram(), rts.stft_eval(c, 4, 2, 4, window=win), bound),
            ("range", lambda t: t.cube_range_transform(64, window=rwin, first=1, count=3), lambda t: t.range_map(), rts.range_eval(c, 64, window=rwin, first=1, count=3), bound),
            ("beam", lambda t: t.cube_beamform(w, first=2, count=4), lambda t: t.beam_map(), rts.beamform_eval(c, w, first=2, count=4), exact),
            ("covariance", lambda t: t.cube_covariance(first=1, count=6), lambda t: t.covariance(), cov, exact),
            ("mvdr", lambda t: t.cube_mvdr(s, 0.5), lambda t: t.mvdr_weights(), rts.mvdr_eval(cov, s, 0.5), exact),
            ("st_apply", lambda t: t.cube_st_apply(wst, 2, power=True), lambda t: t.st_map(), rts.st_apply_eval(c, wst, 2, power=True), exact),
            ("eig", lambda t: t.cube_eig(), lambda t: t.eigenpairs(), (vals, vecs), exact),
            ("doa", lambda t: t.cube_doa_scan(self.dtable.data_ptr(), gd, first_vector=1, n_dirs=33), lambda t: t.doa_spectrum(), rts.doa_scan_eval(vecs[1:3], gd, table), exact),
            ("image", image, lambda t: t.image(), rts.backproject_eval(c, self.t0, self.dt, g["origin"], g["step_x"], g["step_y"], 6, 4, g["tx"], g["rx"], g["c"], g["fc"], taps=2, first=2), bound),
            ("align", lambda t: t.cube_align(1, 6, (2, 30), 4, 2), lambda t: t.align_shifts(), rts.align_eval(c, 1, 6, (2, 30), 4, 2), exact),
            ("pga", lambda t: t.cube_pga(0, 8, (2, 30), 3), lambda t: t.pga_phase(), rts.pga_eval(c, 0, 8, (2, 30), 3), pga_bound),
            ("detections", lambda t: t.cube_detect_os(**os_par), lambda t: t.detections(), None, self.compare_detections),
            ("plots", lambda t: t.cube_plots((1, 1), pri=1e-3), lambda t: t.plots(), None, self.compare_plots),
        ]
        self.want_det = rts.cfar_os_eval(dmap, t0=self.t0, dt=self.dt, **os_par)
        assert len(self.want_det) >= 8

    def compare_detections(self, got, _, what):
        """the handle's own map is the device's transform, within its bound of the reference's: the list is the evaluator's on that map"""
        self.det_map = self.last["doppler"]
        same_list(self.rts, got, self.det_map, what, self.t0, self.dt, **self.os_par)
        assert cells(got) == cells(self.want_det)

    def compare_plots(self, got, _, what):
        want = self.rts.plots_eval(self.last["detections"], self.n_fft, (1, 1), 1, pri=1e-3, t0=self.t0, dt=self.dt, n_rx=3, n_bins=40)
        PR.same_bytes(got, want)
        assert len(got) >= 2

    def handle(self):
        return attached(self.rts, self.d, self.shape, self.t0, self.dt)

    def make_all(self, t):
        """every product once, in the table's order, each against its evaluator: name -> its bytes"""
        self.last, out = {}, {}
        for name, make, get, want, compare in self.rows:
            self.last[name] = got = make(t)
            compare(got, want, name)
            out[name] = blob(got)
        return out

    def read_all(self, t):
        return {name: blob(get(t)) for name, make, get, want, compare in self.rows}

    def all_refuse(self, t):
        for name, make, get, want, compare in self.rows:
            with pytest.raises(self.rts.L.RtsError):
                get(t)


def mvdr_is_refused(rts, tr, steering):
    """rts_cube_mvdr itself (Tracer.cube_mvdr checks the rows' width against its own note of the order first)"""
    p, keep = rts._mvdr_params(steering, 0, 0.5, None)
    assert rts.L.lib().rts_cube_mvdr(tr.h, C.byref(p), None) == rts.L.RTS_ERR_INVALID and b"n_rx" in rts.L.lib().rts_last_error()


def test_records_across_products_and_attach(rts):
    import torch
    L = rts.L
    T = Table(rts, 401)
    make = {name: mk for name, mk, get, want, compare in T.rows}
    c, rng = T.cube, np.random.default_rng(402)
    tr = T.handle()
    made = T.make_all(tr)
    f = T.handle(); assert T.make_all(f) == made; f.close()                     # (b), every product
    assert T.read_all(tr) == made                                               # every record outlives the calls of all the others
    # a track table, which is no product of the cube
    plots = TR.sequence(0)[0]; pbuf = dev_bytes(plots)
    tracks = tr.cube_track(0.0, device_plots=pbuf.data_ptr(), n_plots=len(plots), **TR.SEQ_PAR)
    assert len(tracks[0]) == len(plots)

    # ---- neighbours: the stacked covariance replaces the receivers' and back; the weights and the eigenpairs follow the LAST one
    cov3_h, cov6_h = rts.covariance_eval(c, first=1, count=6), rts.st_covariance_eval(c, 2, first=1, count=6)
    s3, s6 = B.random_complex(rng, (2, 3)), B.random_complex(rng, (2, 6))
    exact(tr.cube_st_covariance(2, first=1, count=6), cov6_h, "stacked")
    exact(tr.covariance(), cov6_h)
    mvdr_is_refused(rts, tr, s3)
    with pytest.raises(L.RtsError, match="n = 3"):
        tr.cube_eig(n=3)
    assert blob(tr.mvdr_weights()) == made["mvdr"] and blob(tr.eigenpairs()) == made["eig"]          # the refusals left the records alone
    exact(tr.cube_mvdr(s6, 0.5), rts.mvdr_eval(cov6_h, s6, 0.5), "mvdr of the stacked covariance")
    exact(tr.cube_eig(), rts.eig_eval(cov6_h), "eig of the stacked covariance")
    assert blob(tr.cube_covariance(first=1, count=6)) == made["covariance"]
    mvdr_is_refused(rts, tr, s6)
    with pytest.raises(L.RtsError, match="n = 6"):
        tr.cube_eig(n=6)
    exact(tr.cube_mvdr(s3, 0.5), rts.mvdr_eval(cov3_h, s3, 0.5), "mvdr of the receivers' covariance")
    # ---- rts_cube_eig with and without device_cov: the scan follows the last library-owned eigenvectors' order
    cov4 = A.hermitian_pd(rng, 4); d4 = dev(cov4)
    pairs4 = tr.cube_eig(n=4, device_cov=d4.data_ptr())
    exact(pairs4, rts.eig_eval(cov4), "eig of a caller's covariance")
    table4 = B.random_complex(rng, (9, 4)); dt4 = dev(np.ascontiguousarray(table4.T))
    exact(tr.cube_doa_scan(dt4.data_ptr(), [1.0, 2.0], first_vector=2, n_dirs=9), rts.doa_scan_eval(pairs4[1][2:4], [1.0, 2.0], table4), "scan of 4 elements")
    with pytest.raises(L.RtsError, match="n = 3"):
        tr.cube_doa_scan(T.dtable.data_ptr(), [1.0], n_dirs=33, n=3)
    assert blob(tr.covariance()) == made["covariance"]                          # a caller's covariance is no record
    assert blob(tr.cube_eig()) == made["eig"]                                   # ... and without it the solve is the library-owned covariance's again
    # ---- plots end at either detector
    ca = lambda t: t.cube_detect((1, 0), (3, 1), "ca", pfa=1e-2, local_max=False, pri=1e-3)
    for detect in (ca, make["detections"]):
        assert blob(tr.plots()) == made["plots"]
        det = detect(tr)
        with pytest.raises(L.RtsError, match="no plots"):
            tr.plots()
        f = T.handle(); f.cube_doppler(8, fetch=False)
        assert blob(det) == blob(detect(f)) and (detect is not ca or blob(det) != made["detections"])
        f.close()
        assert blob(make["detections"](tr)) == made["detections"] and blob(make["plots"](tr)) == made["plots"]
    # ---- the table's own weights and spectrum again, then caller-owned outputs: they leave every library-owned record untouched (the
    # Doppler map apart, which is recorded wherever it goes: rts_cube_detect without a map takes it)
    assert blob(make["mvdr"](tr)) == made["mvdr"] and blob(make["doa"](tr)) == made["doa"]
    assert T.read_all(tr) == made
    cal = filled(1 << 14, 0j, torch.complex128)
    p = cal.data_ptr()
    tr.cube_spectrogram(2, 1, 2, device_ptr=p)
    tr.cube_range_transform(128, device_ptr=p)
    tr.cube_beamform(B.random_complex(rng, (5, 3)), device_ptr=p)
    tr.cube_covariance(device_ptr=p)
    tr.cube_mvdr(s3, 0.0, device_ptr=p)
    tr.cube_st_covariance(2, device_ptr=p)
    tr.cube_st_apply(s6, 2, device_ptr=p)
    tr.cube_eig(device_values=p, device_vectors=p + 4096)
    tr.cube_doa_scan(T.dtable.data_ptr(), [2.0], n_dirs=33, device_ptr=p)
    tr.cube_backproject((0.0, 0.0, 0.0), (1.0, 0.0, 0.0), (0.0, 1.0, 0.0), 3, 3, np.zeros((1, 3)) - 100.0, np.zeros((3, 1, 3)) + 100.0, TH.CS, 1e9, count=1, device_ptr=p)
    assert T.read_all(tr) == made
    assert np.count_nonzero(cal.cpu().numpy()) > 0
    # ---- rts_cube_attach: every product ends, the tracks do not
    tr.cube_attach(*T.shape, T.t0, T.dt, device_ptr=T.d.data_ptr())
    T.all_refuse(tr)
    assert blob(tr.tracks()) == blob(tracks)
    with pytest.raises(L.RtsError, match="no covariance"):
        tr.cube_mvdr(s3, 0.5)
    with pytest.raises(L.RtsError, match="no covariance"):
        tr.cube_eig()
    with pytest.raises(L.RtsError, match="no eigenvectors"):
        tr.cube_doa_scan(T.dtable.data_ptr(), [1.0], n_dirs=33)
    with pytest.raises(L.RtsError, match="no map"):
        tr.cube_detect_os(**T.os_par)
    with pytest.raises(L.RtsError, match="no detection list"):
        tr.cube_plots((1, 1))
    assert T.make_all(tr) == made                                               # the next call of every product: (a) inside, and the bytes of the first round, which were a fresh handle's
    assert T.read_all(tr) == made and blob(tr.tracks()) == blob(tracks)
    tr.close()


# ============================================================================= 5. two handles interleaved
def test_two_handles_interleaved(rts):
    """Handles A and B, each with its own cube, through the beamform and the summed-spectrogram sequences of part 1, every call
    enqueued without a fetch: in the odd steps B's calls are enqueued first and A's regrow meets them, in the even steps the other way
    round.  Only then are the step's four outputs read."""
    rng = np.random.default_rng(501)
    shape = (2, 20, 547)
    hs = []
    for _ in range(2):
        cube = B.random_complex(rng, shape); d = dev(cube)
        hs.append(dict(cube=cube, d=d, tr=attached(rts, d, shape)))
    win = random_window(rng, 2)
    # beam.own: 2 * n_beams * 547 -> 1 094, 70 016, 1 094, 140 032; stft.own: 2 * frames * n_fft -> 128, 73 728, 128, 147 456 and d_stft_part
    # (a gate of 9 bins: two tiles) twice that -- the sizes of test_regrow_beamform and test_regrow_spectrogram_summed
    for step, (n_beams, n_fft, count) in enumerate(((1, 64, 2), (64, 4096, 10), (1, 64, 2), (128, 4096, 19))):
        w = {id(h["tr"]): B.random_complex(rng, (n_beams, 2)) for h in hs}
        kw = dict(window=win, first=0, count=count, first_bin=100, n_bins=9, power=True, sum_bins=True)
        order = hs[::-1] if step % 2 == 0 else hs
        for h in order:
            h["tr"].cube_beamform(w[id(h["tr"])], first=1, count=1, fetch=False)
        for h in order:
            h["tr"].cube_spectrogram(2, 1, n_fft, fetch=False, **kw)
        for h in hs:
            t = h["tr"]
            beams, spec = t.beam_map(), t.spectrogram()
            exact(beams, rts.beamform_eval(h["cube"], w[id(t)], first=1, count=1), ("beam", step))
            bound(spec, rts.stft_eval(h["cube"], 2, 1, n_fft, **kw), ("stft", step))
            f = attached(rts, h["d"], shape)
            assert blob(f.cube_beamform(w[id(t)], first=1, count=1)) == blob(beams) and blob(f.cube_spectrogram(2, 1, n_fft, **kw)) == blob(spec), step
            f.close()
    for h in hs:
        h["tr"].close()
