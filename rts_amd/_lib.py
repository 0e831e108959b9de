"""Loader + ctypes signatures for librts_amd.so (the C-ABI of include/rts_amd.h).

The library is built in-tree (rts_amd/librts_amd.so) by `make -C rts_amd/csrc` /
__graft_entry__.build().  There is no Python or CPU implementation behind this module: if the
shared library is missing or cannot be loaded, importing a compute entry point raises.
"""
import ctypes as C
import os
import subprocess

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("RTS_AMD_LIB", os.path.join(_HERE, "librts_amd.so"))   # override: kernel A/B experiments
CSRC = os.path.join(_HERE, "csrc")

RTS_OK, RTS_ERR_INVALID, RTS_ERR_NO_DEVICE, RTS_ERR_HIP, RTS_ERR_UNSUPPORTED, RTS_ERR_CAPACITY, RTS_ERR_IO = range(7)
RTS_FLAG_KEEP_ALL_RAYS = 1
RTS_FLAG_COUNT_TRAVERSAL = 2
RTS_FLAG_DEVICE_BUILD = 4
RTS_FLAG_HOST_BUILD = 16
RTS_FLAG_NO_PREFILTER = 8
RTS_FLAG_NO_HORIZON = 32
RTS_FLAG_NO_HORIZON_SECTORS = 64
RTS_MAX_DEPTH = 16
RTS_BASE_USE_ROWS = 0xffffffffffffffff

# PerRayData (include/rts_prd.h == reference ray_tracer.h:13-28)
PRD_DTYPE = np.dtype({
    "names": ["rayLength", "refrIndex", "reflDepth", "refrDepth", "maxRayIndex", "rayDirection",
              "firstHitPoint", "prevHitPoint", "power", "doppler", "received", "end"],
    "formats": ["<f8", ("<f8", 2), "<u4", "<u4", "<u4", ("<f8", 3), ("<f8", 3), ("<f8", 3), "<f8", "<f8", "<i4", "u1"],
    "offsets": [0, 16, 32, 36, 40, 48, 72, 96, 120, 128, 136, 140],
    "itemsize": 144,
})


class RtsParams(C.Structure):
    _fields_ = [("width", C.c_uint32), ("max_refl", C.c_uint32), ("max_refr", C.c_uint32),
                ("interpolate_smooth", C.c_uint32), ("device", C.c_int32), ("flags", C.c_uint32)]


class RtsMesh(C.Structure):
    _fields_ = [("triangles", C.c_void_p), ("vertices", C.c_void_p), ("normals", C.c_void_p),
                ("n_triangles", C.c_uint32), ("n_vertices", C.c_uint32), ("n_normals", C.c_uint32),
                ("reserved", C.c_uint32), ("refl_coeff", C.c_double), ("refr_index", C.c_double)]


class RtsTargetMotion(C.Structure):
    _fields_ = [("position", C.c_double * 3), ("velocity", C.c_double * 3), ("rotation", C.c_double * 9),
                ("has_rotation", C.c_int32), ("reserved", C.c_int32)]


class RtsReceiverSphere(C.Structure):
    _fields_ = [("centre", C.c_double * 3), ("radius", C.c_double), ("min_theta", C.c_double),
                ("max_theta", C.c_double), ("min_phi", C.c_double), ("max_phi", C.c_double)]


class RtsPulse(C.Structure):
    _fields_ = [("ray_origin", C.c_double * 3), ("tx_span", C.c_double * 3), ("tx_dir", C.c_double * 2),
                ("ray_first", C.c_uint64), ("ray_count", C.c_uint64), ("motion", C.POINTER(RtsTargetMotion)),
                ("interleave_tile", C.c_uint32), ("interleave_parts", C.c_uint32), ("interleave_part", C.c_uint32), ("reserved", C.c_uint32)]


class RtsCubeParams(C.Structure):
    _fields_ = [("n_rx", C.c_uint32), ("n_pulses", C.c_uint32), ("n_bins", C.c_uint32), ("reserved", C.c_uint32),
                ("t0", C.c_double), ("dt", C.c_double)]


class RtsPlanItem(C.Structure):
    _fields_ = [("pulse", C.c_uint32), ("interleave_tile", C.c_uint32), ("interleave_parts", C.c_uint32), ("interleave_part", C.c_uint32),
                ("ray_first", C.c_uint64), ("ray_count", C.c_uint64)]


RTS_SHARD_PULSES, RTS_SHARD_RAYS, RTS_SHARD_PULSES_WHOLE = 0, 1, 2


RTS_PATTERN_CONSTANT, RTS_PATTERN_SEPARABLE, RTS_PATTERN_GRID = 0, 1, 2
RTS_PATTERN_ABS_U, RTS_PATTERN_ABS_V = 1, 2
RTS_PATTERN_MAX_AXIS, RTS_PATTERN_MAX_GRID = 65536, 4194304


class RtsPattern(C.Structure):
    _fields_ = [("kind", C.c_uint32), ("flags", C.c_uint32), ("n_u", C.c_uint32), ("n_v", C.c_uint32), ("scale", C.c_double),
                ("u_samples", C.c_void_p), ("u_values", C.c_void_p), ("v_samples", C.c_void_p), ("v_values", C.c_void_p),
                ("u0", C.c_double), ("du", C.c_double), ("v0", C.c_double), ("dv", C.c_double), ("grid", C.c_void_p),
                ("reserved", C.c_uint64 * 2)]


class RtsPatternPulse(C.Structure):
    _fields_ = [("wavelength", C.c_double), ("carrier", C.c_double), ("cspeed", C.c_double),
                ("rx_position", C.c_void_p), ("rx_rotation", C.c_void_p)]


RTS_RENDER_RAYS, RTS_RENDER_PATHS = 0, 1
RTS_RENDER_DOPPLER = 1
RTS_WAVEFORM_MAX_SAMPLES, RTS_WAVEFORM_MAX_TAPS, RTS_COMPRESS_MAX_BINS = 4096, 64, 8192


class RtsWaveform(C.Structure):
    _fields_ = [("samples", C.c_void_p), ("n_samples", C.c_uint32), ("taps", C.c_uint32), ("reserved", C.c_uint64 * 2)]


RTS_CFAR_CA, RTS_CFAR_GO, RTS_CFAR_SO = 0, 1, 2
RTS_CFAR_LOCAL_MAX = 1
RTS_CFAR_MAX_HALF, RTS_CFAR_DEFAULT_MAX_DETECTIONS = 16, 65536


class RtsCfarParams(C.Structure):
    _fields_ = [("guard_range", C.c_uint32), ("guard_doppler", C.c_uint32), ("train_range", C.c_uint32), ("train_doppler", C.c_uint32),
                ("mode", C.c_uint32), ("flags", C.c_uint32), ("pfa", C.c_double), ("alpha", C.c_double), ("pri", C.c_double),
                ("max_detections", C.c_uint32), ("reserved0", C.c_uint32), ("reserved", C.c_uint64 * 2)]


# RtsDetection (include/rts_amd.h), 72 bytes
DETECTION_DTYPE = np.dtype([("rx", "<u4"), ("doppler_bin", "<u4"), ("range_bin", "<u4"), ("n_train", "<u4"), ("power", "<f8"),
                            ("noise", "<f8"), ("threshold", "<f8"), ("range_offset", "<f8"), ("doppler_offset", "<f8"),
                            ("delay", "<f8"), ("doppler", "<f8")])
assert DETECTION_DTYPE.itemsize == 72 and C.sizeof(RtsCfarParams) == 72

RTS_CFAR_OS_MAX_TRAIN = 1088


class RtsCfarOsParams(C.Structure):
    _fields_ = [("guard_range", C.c_uint32), ("guard_doppler", C.c_uint32), ("train_range", C.c_uint32), ("train_doppler", C.c_uint32),
                ("rank", C.c_uint32), ("flags", C.c_uint32), ("pfa", C.c_double), ("alpha", C.c_double), ("pri", C.c_double),
                ("max_detections", C.c_uint32), ("reserved0", C.c_uint32), ("reserved", C.c_uint64 * 2)]


assert C.sizeof(RtsCfarOsParams) == 72

RTS_PLOT_MAX_LINK = 4


class RtsPlotParams(C.Structure):
    _fields_ = [("link_range", C.c_uint32), ("link_doppler", C.c_uint32), ("min_cells", C.c_uint32), ("max_plots", C.c_uint32),
                ("pri", C.c_double), ("device_list", C.c_void_p), ("n_list", C.c_uint32), ("n_doppler", C.c_uint32),
                ("reserved", C.c_uint64 * 2)]


# RtsPlot (include/rts_amd.h), 104 bytes
PLOT_DTYPE = np.dtype([("rx", "<u4"), ("n_cells", "<u4"), ("first_index", "<u4"), ("peak_index", "<u4"), ("range_min", "<u4"),
                       ("range_max", "<u4"), ("doppler_lo", "<u4"), ("doppler_span", "<u4"), ("power_sum", "<f8"), ("peak_power", "<f8"),
                       ("noise_sum", "<f8"), ("range_centroid", "<f8"), ("doppler_centroid", "<f8"), ("range_spread", "<f8"),
                       ("doppler_spread", "<f8"), ("delay", "<f8"), ("doppler", "<f8")])
assert PLOT_DTYPE.itemsize == 104 and C.sizeof(RtsPlotParams) == 56

RTS_TRACK_MAX_CAND, RTS_TRACK_MAX_TRACKS, RTS_TRACK_DEFAULT_TRACKS, RTS_TRACK_MAX_PLOTS = 16, 65536, 16384, 16777216
RTS_TRACK_CONFIRMED, RTS_TRACK_COASTED, RTS_TRACK_NEW = 1, 2, 4


class RtsTrackParams(C.Structure):
    _fields_ = [("gate", C.c_double), ("sigma_delay", C.c_double), ("sigma_doppler", C.c_double), ("q", C.c_double),
                ("delay_rate_per_hz", C.c_double), ("doppler_period", C.c_double), ("confirm_hits", C.c_uint32), ("max_misses", C.c_uint32),
                ("tentative_misses", C.c_uint32), ("max_candidates", C.c_uint32), ("max_tracks", C.c_uint32), ("n_plots", C.c_uint32),
                ("device_plots", C.c_void_p), ("reserved", C.c_uint64 * 2)]


# RtsTrack (include/rts_amd.h), 88 bytes
TRACK_DTYPE = np.dtype([("id", "<u8"), ("rx", "<u4"), ("flags", "<u4"), ("hits", "<u4"), ("misses", "<u4"), ("age", "<u4"), ("plot_index", "<u4"),
                        ("delay", "<f8"), ("doppler", "<f8"), ("p_dd", "<f8"), ("p_df", "<f8"), ("p_ff", "<f8"), ("d2", "<f8"), ("power_sum", "<f8")])
assert TRACK_DTYPE.itemsize == 88 and C.sizeof(RtsTrackParams) == 96

RTS_LOCATE_MAX_RX, RTS_LOCATE_MAX_PER_RX, RTS_LOCATE_MAX_ITERS, RTS_LOCATE_MAX_LIST, RTS_LOCATE_MAX_INDEX = 16, 1024, 8, 16777216, 1048576
RTS_LOCATE_DEFAULT_CANDIDATES, RTS_LOCATE_MAX_CANDIDATES, RTS_LOCATE_DEFAULT_TARGETS, RTS_LOCATE_MAX_TARGETS = 65536, 1048576, 4096, 65536
RTS_LOCATE_FROM_PLOTS, RTS_LOCATE_FROM_TRACKS, RTS_LOCATE_FROM_CANDIDATES, RTS_TARGET_UNREFINED = 0, 1, 2, 1


class RtsLocateParams(C.Structure):
    _fields_ = [("tx", C.c_double * 3), ("rx_positions", C.c_void_p), ("cspeed", C.c_double), ("carrier", C.c_double), ("sigma_delay", C.c_double),
                ("sigma_doppler", C.c_double), ("gate", C.c_double), ("assoc_delay", C.c_double), ("box_lo", C.c_double * 3), ("box_hi", C.c_double * 3),
                ("n_rx", C.c_uint32), ("anchors", C.c_uint32 * 3), ("min_receivers", C.c_uint32), ("n_iters", C.c_uint32), ("max_candidates", C.c_uint32),
                ("max_targets", C.c_uint32), ("source", C.c_uint32), ("n_list", C.c_uint32), ("device_list", C.c_void_p), ("reserved", C.c_uint64 * 2)]


# RtsTarget (include/rts_amd.h), 144 bytes
TARGET_DTYPE = np.dtype([("pos", "<f8", (3,)), ("vel", "<f8", (3,)), ("cost", "<f8"), ("power_sum", "<f8"), ("candidate", "<u8"), ("n_receivers", "<u4"),
                         ("flags", "<u4"), ("plot", "<u4", (16,))])
assert TARGET_DTYPE.itemsize == 144 and C.sizeof(RtsLocateParams) == 192

RTS_TBD_POWER, RTS_TBD_AMPLITUDE, RTS_TBD_LOCAL_MAX, RTS_TBD_NONE = 0, 1, 1, 0xff
RTS_TBD_MAX_HALF_DOPPLER, RTS_TBD_MAX_HALF_RANGE, RTS_TBD_MAX_DEPTH, RTS_TBD_MAX_TRACKS, RTS_TBD_MAX_CELLS = 3, 15, 64, 65536, 0x40000000
RTS_TBD_TILE = 1024      # rts_amd/csrc/rts_tbd.h: the range bins a workgroup of the step takes


class RtsTbdParams(C.Structure):
    _fields_ = [("half_doppler", C.c_uint32), ("half_range", C.c_uint32), ("depth", C.c_uint32), ("score", C.c_uint32), ("flags", C.c_uint32),
                ("reserved0", C.c_uint32), ("scale", C.c_double), ("decay", C.c_double), ("delay_rate_per_hz", C.c_double), ("pri", C.c_double),
                ("reserved", C.c_uint64 * 2)]


class RtsTbdExtractParams(C.Structure):
    _fields_ = [("threshold", C.c_double), ("pri", C.c_double), ("flags", C.c_uint32), ("max_tracks", C.c_uint32), ("reserved", C.c_uint64 * 2)]


# RtsTbdTrack (include/rts_amd.h), 48 bytes
TBD_TRACK_DTYPE = np.dtype([("rx", "<u4"), ("doppler_bin", "<u4"), ("range_bin", "<u4"), ("n_cells", "<u4"), ("first_doppler_bin", "<u4"),
                            ("first_range_bin", "<u4"), ("merit", "<f8"), ("delay", "<f8"), ("doppler", "<f8")])
assert TBD_TRACK_DTYPE.itemsize == 48 and C.sizeof(RtsTbdParams) == 72 and C.sizeof(RtsTbdExtractParams) == 40


RTS_IMAGE_ACCUMULATE, RTS_IMAGE_PULSE_CHUNK, RTS_IMAGE_MAX_PIXELS = 1, 64, 16777216


class RtsImageParams(C.Structure):
    _fields_ = [("n_x", C.c_uint32), ("n_y", C.c_uint32), ("taps", C.c_uint32), ("flags", C.c_uint32),
                ("first_pulse", C.c_uint32), ("n_pulses", C.c_uint32),
                ("origin", C.c_double * 3), ("step_x", C.c_double * 3), ("step_y", C.c_double * 3),
                ("cspeed", C.c_double), ("carrier", C.c_double),
                ("tx_position", C.c_void_p), ("rx_position", C.c_void_p), ("pulse_weight", C.c_void_p),
                ("reserved", C.c_uint64 * 2)]


assert C.sizeof(RtsImageParams) == 152


RTS_STFT_POWER, RTS_STFT_SUM_BINS = 1, 2
RTS_STFT_MAX_FFT, RTS_STFT_BIN_TILE, RTS_STFT_MAX_RX, RTS_STFT_MAX_GRID_X = 4096, 8, 65535, 2147483647
RTS_WINDOW_RECT, RTS_WINDOW_HANN, RTS_WINDOW_HAMMING, RTS_WINDOW_BLACKMAN = 0, 1, 2, 3


class RtsStftParams(C.Structure):
    _fields_ = [("first_pulse", C.c_uint32), ("n_pulses", C.c_uint32), ("window_len", C.c_uint32), ("hop", C.c_uint32),
                ("n_fft", C.c_uint32), ("first_bin", C.c_uint32), ("n_bins", C.c_uint32), ("flags", C.c_uint32),
                ("window", C.c_void_p), ("reserved", C.c_uint64 * 2)]


assert C.sizeof(RtsStftParams) == 56


RTS_ALIGN_INTEGER, RTS_ALIGN_MAX_LAG, RTS_ALIGN_MAX_ITERS, RTS_ALIGN_PULSE_CHUNK, RTS_ALIGN_BIN_BLOCK = 1, 64, 8, 64, 64
RTS_PGA_MAX_PULSES, RTS_PGA_MAX_ITERS, RTS_PGA_BIN_TILE = 4096, 16, 8
RTS_CORRECT_USE_ALIGN, RTS_CORRECT_USE_PGA = 1, 2


class RtsAlignParams(C.Structure):
    _fields_ = [("first_pulse", C.c_uint32), ("n_pulses", C.c_uint32), ("first_bin", C.c_uint32), ("n_gate", C.c_uint32),
                ("max_lag", C.c_uint32), ("n_iters", C.c_uint32), ("flags", C.c_uint32), ("reserved0", C.c_uint32),
                ("reserved", C.c_uint64 * 2)]


class RtsPgaParams(C.Structure):
    _fields_ = [("first_pulse", C.c_uint32), ("n_pulses", C.c_uint32), ("first_bin", C.c_uint32), ("n_gate", C.c_uint32),
                ("n_iters", C.c_uint32), ("window0", C.c_uint32), ("window_min", C.c_uint32), ("reserved0", C.c_uint32),
                ("reserved", C.c_uint64 * 2)]


class RtsCorrectParams(C.Structure):
    _fields_ = [("first_pulse", C.c_uint32), ("n_pulses", C.c_uint32), ("taps", C.c_uint32), ("flags", C.c_uint32),
                ("shifts", C.c_void_p), ("phase", C.c_void_p), ("reserved", C.c_uint64 * 2)]


assert C.sizeof(RtsAlignParams) == 48 and C.sizeof(RtsPgaParams) == 48 and C.sizeof(RtsCorrectParams) == 48


RTS_BEAT_STRIP, RTS_BEAT_MAX_PARTS = 16, 64
RTS_RANGE_REVERSE, RTS_RANGE_MAX_FFT = 1, 4096


class RtsBeatParams(C.Structure):
    _fields_ = [("slope", C.c_double), ("duration", C.c_double), ("source", C.c_uint32), ("flags", C.c_uint32), ("reserved", C.c_uint64 * 2)]


# RtsBeatContribution (include/rts_amd.h), 40 bytes
BEAT_CONTRIBUTION_DTYPE = np.dtype([("rx", "<i4"), ("reserved", "<i4"), ("re", "<f8"), ("im", "<f8"), ("delay", "<f8"), ("doppler", "<f8")])


class RtsRangeParams(C.Structure):
    _fields_ = [("first_pulse", C.c_uint32), ("n_pulses", C.c_uint32), ("first_bin", C.c_uint32), ("n_samples", C.c_uint32),
                ("n_fft", C.c_uint32), ("n_out", C.c_uint32), ("flags", C.c_uint32), ("reserved0", C.c_uint32),
                ("window", C.c_void_p), ("reserved", C.c_uint64 * 2)]


assert C.sizeof(RtsBeatParams) == 40 and BEAT_CONTRIBUTION_DTYPE.itemsize == 40 and C.sizeof(RtsRangeParams) == 56


RTS_BEAM_FROM_CUBE, RTS_BEAM_FROM_MAP, RTS_BEAM_FROM_POINTER = 0, 1, 2
RTS_BEAM_POWER, RTS_BEAM_PEAK = 1, 2
RTS_BEAM_MAX_RX, RTS_BEAM_MAX_BEAMS, RTS_BEAM_MAX_WEIGHTS = 64, 1024, 4096


class RtsBeamParams(C.Structure):
    _fields_ = [("n_beams", C.c_uint32), ("source", C.c_uint32), ("first_row", C.c_uint32), ("n_rows", C.c_uint32),
                ("n_rows_in", C.c_uint32), ("flags", C.c_uint32), ("weights", C.c_void_p), ("device_in", C.c_void_p),
                ("reserved", C.c_uint64 * 2)]


assert C.sizeof(RtsBeamParams) == 56


RTS_SRC_MAX_PATCHES, RTS_SRC_MAX_TABLE, RTS_SRC_TILE = 1024, 4096, 8      # (RTS_SRC_TILE: rts_source.h's workgroup tile, bins)


class RtsSourceParams(C.Structure):
    _fields_ = [("n_patches", C.c_uint32), ("flags", C.c_uint32), ("spatial", C.c_void_p), ("power", C.c_void_p), ("doppler", C.c_void_p),
                ("rho", C.c_void_p), ("range_profile", C.c_void_p), ("seed", C.c_uint64), ("reserved", C.c_uint64 * 2)]


assert C.sizeof(RtsSourceParams) == 72


RTS_ADAPT_TILE, RTS_ADAPT_MAX_PARTS = 64, 512


class RtsCovParams(C.Structure):
    _fields_ = [("source", C.c_uint32), ("n_rows_in", C.c_uint32), ("first_row", C.c_uint32), ("n_rows", C.c_uint32),
                ("first_bin", C.c_uint32), ("n_bins", C.c_uint32), ("skip_first_bin", C.c_uint32), ("skip_n_bins", C.c_uint32),
                ("device_in", C.c_void_p), ("reserved", C.c_uint64 * 2)]


class RtsMvdrParams(C.Structure):
    _fields_ = [("n_beams", C.c_uint32), ("n_rx", C.c_uint32), ("loading", C.c_double), ("steering", C.c_void_p),
                ("device_cov", C.c_void_p), ("reserved", C.c_uint64 * 2)]


assert C.sizeof(RtsCovParams) == 56 and C.sizeof(RtsMvdrParams) == 48


# passive radar (include/rts_amd.h)
RTS_PASSIVE_MAX_TAPS, RTS_PASSIVE_MAX_RX, RTS_PASSIVE_TILE, RTS_PASSIVE_MAX_PARTS, RTS_PASSIVE_MAX_BLOCKS = 64, 64, 256, 512, 4096
RTS_XCORR_MAX_LAGS, RTS_XCORR_MAX_FIRST_LAG = 16384, 0x7fff0000


class RtsCancelParams(C.Structure):
    _fields_ = [("ref_rx", C.c_uint32), ("n_taps", C.c_uint32), ("first_pulse", C.c_uint32), ("n_pulses", C.c_uint32),
                ("rows_per_block", C.c_uint32), ("reserved0", C.c_uint32), ("rx_mask", C.c_uint64), ("loading", C.c_double),
                ("reserved", C.c_uint64 * 2)]


class RtsXcorrParams(C.Structure):
    _fields_ = [("ref_rx", C.c_uint32), ("reserved0", C.c_uint32), ("first_pulse", C.c_uint32), ("n_pulses", C.c_uint32),
                ("first_lag", C.c_uint32), ("n_lags", C.c_uint32), ("reserved", C.c_uint64 * 2)]


assert C.sizeof(RtsCancelParams) == 56 and C.sizeof(RtsXcorrParams) == 40


# MIMO radar: the matched-filter bank (include/rts_amd.h)
RTS_BANK_MAX_WAVES, RTS_BANK_TILE, RTS_BANK_MAX_CELLS = 16, 512, 1 << 39


class RtsBankParams(C.Structure):
    _fields_ = [("waves", C.POINTER(RtsWaveform)), ("n_waves", C.c_uint32), ("code", C.c_void_p), ("first_pulse", C.c_uint32), ("n_pulses", C.c_uint32),
                ("reserved", C.c_uint64 * 2)]


assert C.sizeof(RtsBankParams) == 48


RTS_ST_MAX_TAPS = 16


class RtsStCovParams(C.Structure):
    _fields_ = [("source", C.c_uint32), ("n_rows_in", C.c_uint32), ("first_row", C.c_uint32), ("n_rows", C.c_uint32),
                ("first_bin", C.c_uint32), ("n_bins", C.c_uint32), ("skip_first_bin", C.c_uint32), ("skip_n_bins", C.c_uint32),
                ("n_taps", C.c_uint32), ("reserved0", C.c_uint32), ("device_in", C.c_void_p), ("reserved", C.c_uint64 * 2)]


class RtsStApplyParams(C.Structure):
    _fields_ = [("n_filters", C.c_uint32), ("source", C.c_uint32), ("first_row", C.c_uint32), ("n_rows", C.c_uint32),
                ("n_rows_in", C.c_uint32), ("flags", C.c_uint32), ("n_taps", C.c_uint32), ("reserved0", C.c_uint32),
                ("weights", C.c_void_p), ("device_in", C.c_void_p), ("reserved", C.c_uint64 * 2)]


assert C.sizeof(RtsStCovParams) == 64 and C.sizeof(RtsStApplyParams) == 64


RTS_EIG_MAX_SWEEPS = 30
RTS_DOA_INVERSE = 1
RTS_DOA_BARTLETT, RTS_DOA_CAPON, RTS_DOA_MUSIC = 0, 1, 2
RTS_DOA_AIC, RTS_DOA_MDL = 0, 1


class RtsEigParams(C.Structure):
    _fields_ = [("n", C.c_uint32), ("reserved0", C.c_uint32), ("device_cov", C.c_void_p), ("reserved", C.c_uint64 * 2)]


class RtsDoaScanParams(C.Structure):
    _fields_ = [("n", C.c_uint32), ("first_vector", C.c_uint32), ("m", C.c_uint32), ("flags", C.c_uint32), ("n_dirs", C.c_uint64),
                ("g", C.c_void_p), ("device_steering", C.c_void_p), ("device_vectors", C.c_void_p), ("reserved", C.c_uint64 * 2)]


assert C.sizeof(RtsEigParams) == 32 and C.sizeof(RtsDoaScanParams) == 64


class RtsSceneInfo(C.Structure):
    _fields_ = [("n_targets", C.c_uint32), ("n_prims", C.c_uint32), ("n_nodes", C.c_uint32), ("n_leaves", C.c_uint32),
                ("handles_sharing", C.c_uint32), ("builder", C.c_uint32), ("build_ms", C.c_double),
                ("shared_device_bytes", C.c_uint64), ("handle_device_bytes", C.c_uint64), ("version_bytes", C.c_uint64),
                ("horizon_bytes", C.c_uint64)]


class RtsStats(C.Structure):
    _fields_ = [("rays", C.c_uint64), ("segments", C.c_uint64), ("shaded", C.c_uint64), ("received", C.c_uint64),
                ("node_visits", C.c_uint64), ("tri_tests", C.c_uint64), ("n_prims", C.c_uint32), ("n_nodes", C.c_uint32),
                ("ms_scene", C.c_float), ("ms_trace", C.c_float), ("ms_compact", C.c_float), ("ms_aggregate", C.c_float),
                ("bvh_rebuilt", C.c_uint32), ("stack_overflows", C.c_uint32), ("walked_segments", C.c_uint64), ("coop_tiles", C.c_uint32), ("cost_records_dropped", C.c_uint32)]


RESPONSE_DTYPE = np.dtype([("ray", "<u8"), ("rx", "<i4"), ("n", "<u4"), ("power", "<f8"), ("delay", "<f8"),
                           ("doppler", "<f8"), ("phase", "<f8")])
GROUP_DTYPE = np.dtype([("rx", "<i4"), ("direct", "<u4"), ("path", "<i4", (RTS_MAX_DEPTH,)), ("min_ray", "<u8"),
                        ("n", "<f8"), ("sum_sqrt_power", "<f8"), ("sum_delay", "<f8"), ("sum_phase", "<f8"),
                        ("sum_doppler", "<f8")])
assert RESPONSE_DTYPE.itemsize == 48 and GROUP_DTYPE.itemsize == 120


def is_stale():
    """True if librts_amd.so is missing or was built from other sources than the tree's (hash baked in by the Makefile)"""
    if not os.path.exists(LIB_PATH):
        return True
    try:
        return build_id() != source_hash()
    except (OSError, AttributeError):              # unloadable, or a library from before rts_build_id
        return True


def source_hash():
    """the hash rts_amd/csrc/Makefile bakes into the library (rts_build_id): SHA-256, first 16 hex digits, of the sources in
    byte order of their names, then the two public headers"""
    import hashlib
    names = sorted(f for f in os.listdir(CSRC) if f.endswith((".hip", ".cpp", ".h")) and f != "rts_build_id.h")
    h = hashlib.sha256()
    for path in [os.path.join(CSRC, f) for f in names] + [os.path.join(_HERE, "..", "include", f) for f in ("rts_amd.h", "rts_prd.h")]:
        with open(path, "rb") as f:
            h.update(f.read())
    return h.hexdigest()[:16]


def build_id(path=None):
    """rts_build_id() of a built library (default: the one lib() loads), without going through lib()'s prototypes"""
    L = C.CDLL(path or LIB_PATH)
    L.rts_build_id.restype = C.c_char_p
    return L.rts_build_id().decode()


def require_built():
    """bench.py and the timed tools never build: under `rocprofv3 -- python bench.py` a make -> sh -> hipcc chain would be
    an exec from a process whose GPU the profiler's preload has already initialised.  Build beforehand
    (__graft_entry__.build() or make -C rts_amd/csrc).  A library that was built from other sources than the tree's is an
    error too (file times do not survive the copy to a GPU box; the hash baked into the library does) -- unless RTS_AMD_LIB
    names another build on purpose (same-box A/B runs)."""
    if not os.path.exists(LIB_PATH):
        raise SystemExit("librts_amd.so is not built: run `python __graft_entry__.py` (or make -C rts_amd/csrc) first")
    if "RTS_AMD_LIB" not in os.environ:
        have, want = build_id(), source_hash()
        if have != want:
            raise SystemExit("librts_amd.so is stale: built from sources %s, the tree is %s -- run `python __graft_entry__.py` first" % (have, want))


def build(force=False, verbose=False):
    """Compile librts_amd.so for gfx950 in-tree (hipcc cross-compiles without a GPU)."""
    if force or is_stale():
        cmd = ["make", "-C", CSRC, "-j", "5"] + ([] if verbose else ["-s"])
        subprocess.check_call(cmd)
    return LIB_PATH


_lib = None

# every symbol include/rts_amd.h declares
EXPORTS = ["rts_create", "rts_destroy", "rts_last_error", "rts_device_count", "rts_set_scene", "rts_share_scene", "rts_scene_info", "rts_set_receivers",
           "rts_trace_pulse", "rts_reserve", "rts_trace_pulse_begin", "rts_trace_pulse_end", "rts_link_handles", "rts_get_stats", "rts_get_block_timeline", "rts_received_count", "rts_get_received", "rts_get_all_rays",
           "rts_finalise_uniform", "rts_trace_pulse_end_uniform", "rts_aggregate", "rts_group_count", "rts_get_groups", "rts_get_aggregated",
           "rts_merge_groups", "rts_groups_to_responses", "rts_kernel_wrapper", "rts_vertex_rotation",
           "rts_rotation_matrix", "rts_rect_mesh", "rts_sphere_mesh", "rts_file_mesh", "rts_rx_sphere", "rts_get_bvh",
           "rts_build_id", "rts_bind_host_to_device", "rts_get_lane_stats", "rts_get_walk_stats", "rts_get_horizon", "rts_get_horizon_sectors", "rts_self_test_math", "rts_cube_attach", "rts_cube_accumulate", "rts_cube_get", "rts_cube_accumulate_paths", "rts_cube_doppler", "rts_cube_doppler_get", "rts_plan_cpi", "rts_cube_reduce", "rts_kernel_wrapper_on",
           "rts_received_prefetch", "rts_received_view", "rts_finalise_values", "rts_aggregated_view", "rts_build_hierarchy_host",
           "rts_tile_records_get", "rts_tile_records_set", "rts_deal_tiles", "rts_set_tile_list",
           "rts_set_patterns", "rts_finalise_patterns", "rts_trace_pulse_end_patterns", "rts_pattern_eval",
           "rts_cube_set_waveform", "rts_cube_render", "rts_cube_compress", "rts_waveform_eval",
           "rts_cube_add_noise", "rts_noise_eval", "rts_cube_add_sources", "rts_sources_eval", "rts_cube_detect", "rts_cube_detections_get",
           "rts_cube_detect_os", "rts_cfar_os_alpha", "rts_cfar_os_eval",
           "rts_cube_plots", "rts_cube_plots_get", "rts_plots_eval",
           "rts_cube_track", "rts_cube_tracks_get", "rts_cube_tracks_set", "rts_cube_tracks_reset", "rts_cube_track_rounds", "rts_tracks_eval",
           "rts_cube_locate", "rts_cube_targets_get", "rts_cube_locate_rounds", "rts_locate_eval",
           "rts_cube_tbd_step", "rts_cube_tbd_extract", "rts_cube_tbd_tracks_get", "rts_cube_tbd_paths_get", "rts_cube_tbd_merit_get", "rts_cube_tbd_ring_get",
           "rts_cube_tbd_info", "rts_cube_tbd_reset", "rts_tbd_step_eval", "rts_tbd_extract_eval",
           "rts_cube_backproject", "rts_cube_image_get", "rts_backproject_eval",
           "rts_cube_spectrogram", "rts_cube_spectrogram_get", "rts_stft_eval", "rts_window_make",
           "rts_cube_align", "rts_cube_align_get", "rts_cube_pga", "rts_cube_pga_get", "rts_cube_correct", "rts_align_eval", "rts_pga_eval", "rts_correct_eval",
           "rts_cube_render_beat", "rts_beat_eval", "rts_cube_range_transform", "rts_cube_range_get", "rts_range_eval",
           "rts_cube_beamform", "rts_cube_beam_get", "rts_beamform_eval", "rts_steering_make",
           "rts_cube_covariance", "rts_cube_covariance_get", "rts_covariance_eval", "rts_cube_mvdr", "rts_cube_mvdr_get", "rts_mvdr_eval",
           "rts_cube_st_covariance", "rts_st_covariance_eval", "rts_cube_st_apply", "rts_cube_st_get", "rts_st_apply_eval", "rts_st_steering_make",
           "rts_cube_eig", "rts_cube_eig_get", "rts_eig_eval", "rts_cube_doa_scan", "rts_cube_doa_get", "rts_doa_scan_eval", "rts_doa_weights", "rts_source_count",
           "rts_cube_cancel", "rts_cube_cancel_info", "rts_cube_cancel_coeffs_get", "rts_cancel_eval", "rts_cube_xcorr", "rts_cube_xcorr_get", "rts_xcorr_eval",
           "rts_cube_bank", "rts_cube_bank_get", "rts_bank_eval"]


def lib():
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RuntimeError("librts_amd.so is not built (run `make -C rts_amd/csrc` or __graft_entry__.build()); "
                           "there is no Python/CPU fallback for the RTS hot path")
    L = C.CDLL(LIB_PATH)
    vp, u32, u64, dbl, i32 = C.c_void_p, C.c_uint32, C.c_uint64, C.c_double, C.c_int32
    L.rts_last_error.restype = C.c_char_p
    sig = {
        "rts_create": [C.POINTER(RtsParams), C.POINTER(vp)],
        "rts_destroy": [vp],
        "rts_device_count": [C.POINTER(C.c_int)],
        "rts_set_scene": [vp, C.POINTER(RtsMesh), u32],
        "rts_share_scene": [vp, vp],
        "rts_scene_info": [vp, C.POINTER(RtsSceneInfo)],
        "rts_set_receivers": [vp, C.POINTER(RtsReceiverSphere), u32],
        "rts_trace_pulse": [vp, C.POINTER(RtsPulse)],
        "rts_reserve": [vp, u64],
        "rts_trace_pulse_begin": [vp, C.POINTER(RtsPulse)],
        "rts_get_block_timeline": [vp, vp, u32],
        "rts_trace_pulse_end": [vp],
        "rts_link_handles": [vp, vp],
        "rts_get_stats": [vp, C.POINTER(RtsStats)],
        "rts_received_count": [vp, C.POINTER(u64)],
        "rts_get_received": [vp, vp, vp, vp, vp, u64],
        "rts_get_all_rays": [vp, vp, vp, vp, vp, vp, u64],
        "rts_finalise_uniform": [vp, vp, dbl, dbl, dbl, dbl, dbl],
        "rts_build_hierarchy_host": [vp, vp, u32, dbl, vp, u32, vp, u32, C.POINTER(u32), C.POINTER(u32), C.POINTER(C.c_int32)],
        "rts_received_prefetch": [vp],
        "rts_received_view": [vp, C.POINTER(vp), C.POINTER(vp), C.POINTER(vp), C.POINTER(vp), C.POINTER(u64)],
        "rts_finalise_values": [vp, vp, vp, u64],
        "rts_aggregated_view": [vp, C.POINTER(vp), C.POINTER(vp), C.POINTER(vp), C.POINTER(vp), C.POINTER(vp), C.POINTER(u64)],
        "rts_aggregate": [vp, dbl, dbl, u64],
        "rts_trace_pulse_end_uniform": [vp, vp, dbl, dbl, dbl, dbl, dbl, C.c_int32, u64],
        "rts_group_count": [vp, C.POINTER(u32)],
        "rts_get_groups": [vp, vp, u32],
        "rts_get_aggregated": [vp, vp, vp, vp, vp, u64],
        "rts_merge_groups": [vp, u32, u32, vp, C.POINTER(u32)],
        "rts_groups_to_responses": [vp, u32, vp, u32, C.POINTER(u32)],
        "rts_kernel_wrapper": [vp, vp, C.c_uint, C.c_uint, C.c_uint, C.c_uint, dbl, dbl, vp, vp, vp, vp, vp, vp],
        "rts_kernel_wrapper_on": [vp, vp, vp, C.c_uint, C.c_uint, C.c_uint, C.c_uint, dbl, dbl, vp, vp, vp, vp, vp, vp],
        "rts_vertex_rotation": [vp, u32, C.c_float, C.c_float, C.c_float],
        "rts_rotation_matrix": [C.c_float, C.c_float, C.c_float, vp],
        "rts_rect_mesh": [C.c_float] * 6 + [vp, vp, vp],
        "rts_sphere_mesh": [u32, C.c_float, C.c_float, C.c_float, C.c_float, vp, C.POINTER(u32), vp, C.POINTER(u32), vp],
        "rts_file_mesh": [C.c_char_p, C.c_char_p, C.c_float, C.c_float, C.c_float, vp, vp, vp, C.POINTER(u32)],
        "rts_rx_sphere": [vp, dbl, dbl, dbl, dbl, dbl, C.POINTER(RtsReceiverSphere)],
        "rts_get_bvh": [vp, vp, vp, vp, u32, u32, vp],
        "rts_cube_attach": [vp, C.POINTER(RtsCubeParams), vp],
        "rts_cube_accumulate": [vp, u32, dbl, dbl],
        "rts_cube_get": [vp, vp, u64], "rts_get_lane_stats": [vp, vp], "rts_get_walk_stats": [vp, vp, C.c_uint32], "rts_get_horizon": [vp, vp, u32], "rts_get_horizon_sectors": [vp, vp, u32], "rts_bind_host_to_device": [C.c_int, C.POINTER(C.c_int)],
        "rts_cube_accumulate_paths": [vp, u32], "rts_cube_doppler": [vp, u32, vp], "rts_cube_doppler_get": [vp, vp, u64],
        "rts_plan_cpi": [u64, u32, u32, u32, u32, u32, u32, vp, u32, C.POINTER(u32)],
        "rts_cube_reduce": [vp, u32, C.c_int],
        "rts_tile_records_get": [vp, vp, u32], "rts_tile_records_set": [vp, vp, u32], "rts_deal_tiles": [vp, u32, u64, u32, u32, vp, vp], "rts_set_tile_list": [vp, u32, vp, u32],
        "rts_self_test_math": [vp, vp, vp, vp, vp, vp, vp, vp, u32],
        "rts_set_patterns": [vp, C.POINTER(RtsPattern), C.POINTER(RtsPattern), u32, C.POINTER(RtsPattern), u32],
        "rts_finalise_patterns": [vp, C.POINTER(RtsPatternPulse)],
        "rts_trace_pulse_end_patterns": [vp, C.POINTER(RtsPatternPulse), C.c_int32, u64],
        "rts_pattern_eval": [C.POINTER(RtsPattern), vp, vp, u32, vp],
        "rts_cube_set_waveform": [vp, C.POINTER(RtsWaveform)],
        "rts_cube_render": [vp, u32, u32, u32, C.c_double, C.c_double],
        "rts_cube_compress": [vp, u32, u32],
        "rts_waveform_eval": [C.POINTER(RtsWaveform), vp, u32, vp],
        "rts_cube_add_noise": [vp, u32, u32, C.c_double, u64],
        "rts_noise_eval": [u64, vp, u32, C.c_double, vp],
        "rts_cube_add_sources": [vp, C.POINTER(RtsSourceParams)],
        "rts_sources_eval": [C.POINTER(RtsCubeParams), C.POINTER(RtsSourceParams), vp],
        "rts_cube_detect": [vp, C.POINTER(RtsCfarParams), vp, u32],
        "rts_cube_detections_get": [vp, vp, u32, C.POINTER(u32)],
        "rts_cube_detect_os": [vp, C.POINTER(RtsCfarOsParams), vp, u32],
        "rts_cfar_os_alpha": [u32, u32, C.c_double, C.POINTER(C.c_double)],
        "rts_cfar_os_eval": [C.POINTER(RtsCubeParams), vp, u32, C.POINTER(RtsCfarOsParams), vp, u32, C.POINTER(u32)],
        "rts_cube_plots": [vp, C.POINTER(RtsPlotParams)],
        "rts_cube_plots_get": [vp, vp, u32, C.POINTER(u32)],
        "rts_plots_eval": [C.POINTER(RtsCubeParams), vp, u32, u32, C.POINTER(RtsPlotParams), vp, u32, C.POINTER(u32)],
        "rts_cube_track": [vp, C.POINTER(RtsTrackParams), C.c_double],
        "rts_cube_tracks_get": [vp, vp, u32, C.POINTER(u32), C.POINTER(u64)],
        "rts_cube_tracks_set": [vp, vp, u32, u64, C.c_double],
        "rts_cube_tracks_reset": [vp],
        "rts_cube_track_rounds": [vp, C.POINTER(u32)],
        "rts_tracks_eval": [C.POINTER(RtsTrackParams), vp, u32, u64, C.c_double, vp, u32, vp, u32, C.POINTER(u32), C.POINTER(u64)],
        "rts_cube_locate": [vp, C.POINTER(RtsLocateParams)],
        "rts_cube_targets_get": [vp, vp, u32, C.POINTER(u32)],
        "rts_cube_locate_rounds": [vp, C.POINTER(u32)],
        "rts_locate_eval": [C.POINTER(RtsLocateParams), vp, u32, vp, u32, C.POINTER(u32)],
        "rts_cube_tbd_step": [vp, C.POINTER(RtsTbdParams), C.c_double, vp, u32],
        "rts_cube_tbd_extract": [vp, C.POINTER(RtsTbdExtractParams)],
        "rts_cube_tbd_tracks_get": [vp, vp, u32, C.POINTER(u32)],
        "rts_cube_tbd_paths_get": [vp, vp, u32],
        "rts_cube_tbd_merit_get": [vp, vp, u64],
        "rts_cube_tbd_ring_get": [vp, vp, vp, u32, C.POINTER(u32)],
        "rts_cube_tbd_info": [vp, C.POINTER(u32 * 4), C.POINTER(u64)],
        "rts_cube_tbd_reset": [vp],
        "rts_tbd_step_eval": [C.POINTER(RtsCubeParams), vp, u32, vp, C.POINTER(RtsTbdParams), C.c_double, vp, vp, vp],
        "rts_tbd_extract_eval": [C.POINTER(RtsCubeParams), u32, C.POINTER(RtsTbdParams), vp, vp, vp, u32, C.POINTER(RtsTbdExtractParams), vp, vp, u32, C.POINTER(u32)],
        "rts_cube_backproject": [vp, C.POINTER(RtsImageParams), vp],
        "rts_cube_image_get": [vp, vp, u64],
        "rts_backproject_eval": [C.POINTER(RtsCubeParams), vp, C.POINTER(RtsImageParams), vp],
        "rts_cube_spectrogram": [vp, C.POINTER(RtsStftParams), vp, C.POINTER(u32)],
        "rts_cube_spectrogram_get": [vp, vp, u64],
        "rts_stft_eval": [C.POINTER(RtsCubeParams), vp, C.POINTER(RtsStftParams), vp, C.POINTER(u32)],
        "rts_window_make": [u32, u32, vp],
        "rts_cube_align": [vp, C.POINTER(RtsAlignParams), vp],
        "rts_cube_align_get": [vp, vp, u64],
        "rts_cube_pga": [vp, C.POINTER(RtsPgaParams), vp],
        "rts_cube_pga_get": [vp, vp, vp, u64, u64],
        "rts_cube_correct": [vp, C.POINTER(RtsCorrectParams)],
        "rts_align_eval": [C.POINTER(RtsCubeParams), vp, C.POINTER(RtsAlignParams), vp],
        "rts_pga_eval": [C.POINTER(RtsCubeParams), vp, C.POINTER(RtsPgaParams), vp, vp],
        "rts_correct_eval": [C.POINTER(RtsCubeParams), vp, C.POINTER(RtsCorrectParams)],
        "rts_cube_render_beat": [vp, u32, C.POINTER(RtsBeatParams), C.c_double, C.c_double],
        "rts_beat_eval": [C.POINTER(RtsCubeParams), C.POINTER(RtsBeatParams), vp, u32, u32, vp],
        "rts_cube_range_transform": [vp, C.POINTER(RtsRangeParams), vp],
        "rts_cube_range_get": [vp, vp, u64],
        "rts_range_eval": [C.POINTER(RtsCubeParams), vp, C.POINTER(RtsRangeParams), vp],
        "rts_cube_beamform": [vp, C.POINTER(RtsBeamParams), vp],
        "rts_cube_beam_get": [vp, vp, u64],
        "rts_beamform_eval": [C.POINTER(RtsCubeParams), vp, u32, C.POINTER(RtsBeamParams), vp],
        "rts_steering_make": [vp, u32, vp, u32, C.c_double, vp, vp],
        "rts_cube_covariance": [vp, C.POINTER(RtsCovParams), vp],
        "rts_cube_covariance_get": [vp, vp, u64],
        "rts_covariance_eval": [C.POINTER(RtsCubeParams), vp, u32, C.POINTER(RtsCovParams), vp],
        "rts_cube_mvdr": [vp, C.POINTER(RtsMvdrParams), vp],
        "rts_cube_mvdr_get": [vp, vp, u64],
        "rts_mvdr_eval": [vp, u32, C.POINTER(RtsMvdrParams), vp],
        "rts_cube_cancel": [vp, C.POINTER(RtsCancelParams)],
        "rts_cube_cancel_info": [vp, C.POINTER(u32), C.POINTER(u32)],
        "rts_cube_cancel_coeffs_get": [vp, vp, u64],
        "rts_cancel_eval": [C.POINTER(RtsCubeParams), vp, C.POINTER(RtsCancelParams), vp, C.POINTER(u32), C.POINTER(u32)],
        "rts_cube_xcorr": [vp, C.POINTER(RtsXcorrParams), vp],
        "rts_cube_xcorr_get": [vp, vp, u64],
        "rts_xcorr_eval": [C.POINTER(RtsCubeParams), vp, C.POINTER(RtsXcorrParams), vp],
        "rts_cube_bank": [vp, C.POINTER(RtsBankParams), vp],
        "rts_cube_bank_get": [vp, vp, u64],
        "rts_bank_eval": [C.POINTER(RtsCubeParams), vp, C.POINTER(RtsBankParams), vp],
        "rts_cube_st_covariance": [vp, C.POINTER(RtsStCovParams), vp],
        "rts_st_covariance_eval": [C.POINTER(RtsCubeParams), vp, u32, C.POINTER(RtsStCovParams), vp],
        "rts_cube_st_apply": [vp, C.POINTER(RtsStApplyParams), vp],
        "rts_cube_st_get": [vp, vp, u64],
        "rts_st_apply_eval": [C.POINTER(RtsCubeParams), vp, u32, C.POINTER(RtsStApplyParams), vp],
        "rts_st_steering_make": [vp, u32, u32, vp, u32, u32, vp, vp],
        "rts_cube_eig": [vp, C.POINTER(RtsEigParams), vp, vp],
        "rts_cube_eig_get": [vp, vp, vp, u64, u64],
        "rts_eig_eval": [vp, u32, vp, vp, C.POINTER(u32)],
        "rts_cube_doa_scan": [vp, C.POINTER(RtsDoaScanParams), vp],
        "rts_cube_doa_get": [vp, vp, u64],
        "rts_doa_scan_eval": [vp, vp, u32, u32, vp, u64, u32, vp],
        "rts_doa_weights": [u32, vp, u32, u32, C.c_double, C.POINTER(u32), C.POINTER(u32), vp, C.POINTER(u32)],
        "rts_source_count": [vp, u32, u64, u32, C.POINTER(u32)],
    }
    for name, args in sig.items():
        fn = getattr(L, name, None)
        if fn is None:                     # an older build named by RTS_AMD_LIB (same-box A/B runs): its missing entry points raise on use
            continue
        fn.argtypes = args
        fn.restype = C.c_int
    _lib = L
    return L


class RtsError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__("rts error %d: %s" % (code, msg))
        self.code = code


def check(rc):
    if rc != RTS_OK:
        raise RtsError(rc, lib().rts_last_error().decode(errors="replace"))


def ptr(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None else None
