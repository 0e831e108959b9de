#!/usr/bin/env python3
"""What one build of librts_amd.so answers to a fixed list of calls, as JSON, and the difference of two such files.

    RTS_AMD_LIB=/path/to/librts_amd.so python tools/api_diff.py run [--handle] out.json     (one fresh process per library)
    python tools/api_diff.py diff parent.json new.json                                      (prints the differing rows; exit 1 if any)

A row is (entry point, case, rc, rts_last_error() when rc != 0, sha256 of every output array).  It is what a refactor of the host
side of the C-ABI must leave alone: return codes, messages byte for byte, outputs bit for bit.

Host part (default, no GPU): every pure-host export -- the rts_*_eval evaluators, rts_waveform_eval, rts_noise_eval,
rts_window_make, rts_cfar_os_alpha, rts_steering_make, rts_st_steering_make, rts_doa_weights, rts_source_count -- with one valid
call at a small shape (2 receivers, 8 pulses, 16 bins), every single mutation of its arguments from a per-record list (each
field to a refused value, each pointer to null, each reserved word to 1, each array with a NaN), and EVERY PAIR of those
mutations: with two fields wrong, the message says which check comes first, so the pairs pin the order of the checks.
A size is only ever mutated to a value that is refused whatever the other arguments are (0, or beyond the ABI's limit), so no
case can make an evaluator read beyond the arrays it is given -- as long as the library refuses that value before it reads.  Where
the array can hold the refused count it does (rts_tracks_eval's 17 tracks); n_plots = 16 777 217 and n_list = 0x40000001 cannot be
backed by arrays: a library that accepted one of them would read out of bounds in this tool's process.

Handle part (--handle, needs a GPU; run it under `timeout`): each rts_cube_* entry point on one handle with an attached
2 x 8 x 16 cube -- the same single and paired mutations of its record, the state refusals (no cube, no waveform, no map, no list,
no covariance, no eigenvectors, no extraction, no track-before-detect state, a misaligned or overlapping device_out), one valid
call each with its output hashed, and the counted lists (detections, plots, tracks, track-before-detect records and paths) at
capacities at and below what is stored.  NOT covered, because they need a traced pulse: a valid rts_cube_accumulate,
rts_cube_accumulate_paths, rts_cube_render and rts_cube_render_beat (their refusals are).  Refusals return before anything is
launched; the valid calls are the ones the test suite makes."""
import ctypes as C
import hashlib
import itertools
import json
import math
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

N_RX, N_P, N_B, N_D = 2, 8, 16, 8
NAN, INF = math.nan, math.inf
U32MAX = 0xffffffff
BAD_PTR = 0x1004            # non-null, not 8-byte aligned: every check that sees it refuses it, nothing reads it


class Named:
    """a refused value whose text must not enter a case's name (a device address differs from process to process)"""
    def __init__(self, label, value):
        self.label, self.value = label, value

    def __repr__(self):
        return self.label


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()[:16]


def rnd(seed, *shape):
    return np.random.default_rng(seed).standard_normal(shape)


# ---------------------------------------------------------------------------------------------- arguments and their mutations
class Scalar:
    """by value; bad: the refused values"""
    def __init__(self, name, ctype, value, bad=()):
        self.name, self.ctype, self.value, self.bad = name, ctype, value, bad

    def mutations(self):
        return [("%s=%r" % (self.name, b), self.name, ("val", b)) for b in self.bad]

    def make(self, m, keep):
        return self.ctype(dict(m).get("val", self.value))


class Array:
    """a pointer to a host array; out: hashed after the call; nan: the element a NaN goes to (float inputs); alts: label -> f(copy)"""
    def __init__(self, name, array, out=False, nan=None, null=True, alts=None, cast=None):
        self.name, self.array, self.out, self.nan, self.null, self.alts, self.cast = name, np.ascontiguousarray(array), out, nan, null, alts or {}, cast

    def mutations(self):
        ms = [("%s=NULL" % self.name, self.name, ("null", True))] if self.null else []
        if self.nan is not None:
            ms.append(("%s[%d]=NaN" % (self.name, self.nan), self.name, ("nan", self.nan)))
        return ms + [("%s:%s" % (self.name, k), self.name, ("alt", k)) for k in self.alts]

    def make(self, m, keep):
        m = dict(m)
        a = self.array.copy()
        if "nan" in m:
            a.reshape(-1).view(np.float64)[m["nan"]] = NAN
        if "alt" in m:
            self.alts[m["alt"]](a)
        keep.append((self.name, a, self.out))
        if m.get("null"):
            return None
        return C.cast(a.ctypes.data, self.cast) if self.cast else C.c_void_p(a.ctypes.data)      # (cast: the prototype names a typed pointer)


class Out:
    """a pointer to one scalar the call writes"""
    def __init__(self, name, ctype):
        self.name, self.ctype = name, ctype

    def mutations(self):
        return [("%s=NULL" % self.name, self.name, ("null", True))]

    def make(self, m, keep):
        v = self.ctype(0)
        keep.append((self.name, v, True))
        return None if dict(m).get("null") else C.byref(v)


class Record:
    """a pointer to a parameter record.  fields: name -> value, or an array a pointer field names; bad: name -> refused values;
    reserved: the words that must be 0; nan: array field -> element"""
    def __init__(self, name, cls, fields, bad=None, reserved=("reserved",), nan=None, null=True, null_fields=()):
        self.name, self.cls, self.fields, self.bad, self.reserved, self.nan, self.null, self.null_fields = name, cls, fields, bad or {}, reserved, nan or {}, null, null_fields

    def mutations(self):
        ms = [("%s=NULL" % self.name, self.name, ("null", True))] if self.null else []
        for f, values in self.bad.items():
            ms += [("%s.%s=%r" % (self.name, f, b), "%s.%s" % (self.name, f), ("set", (f, b))) for b in values]
        for f in self.reserved:
            if isinstance(getattr(self.cls(), f), int):
                ms.append(("%s.%s=1" % (self.name, f), "%s.%s" % (self.name, f), ("set", (f, 1))))
            else:
                ms += [("%s.%s[%d]=1" % (self.name, f, i), "%s.%s" % (self.name, f), ("res", (f, i))) for i in range(len(getattr(self.cls(), f)))]
        for f, v in self.fields.items():
            if isinstance(v, np.ndarray) and f not in self.null_fields:
                ms.append(("%s.%s=NULL" % (self.name, f), "%s.%s" % (self.name, f), ("set", (f, None))))
        for f, i in self.nan.items():
            ms.append(("%s.%s[%d]=NaN" % (self.name, f, i), "%s.%s" % (self.name, f), ("nanf", (f, i))))
        return ms

    def make(self, m, keep):
        r = self.cls()
        arrays = {}
        for f, v in self.fields.items():
            if isinstance(v, np.ndarray):
                arrays[f] = np.ascontiguousarray(v).copy(); keep.append(("%s.%s" % (self.name, f), arrays[f], False))
                setattr(r, f, arrays[f].ctypes.data)
            else:
                self.put(r, f, v)
        null = False
        for kind, arg in m:
            if kind == "null":
                null = True
            elif kind == "set":
                self.put(r, arg[0], arg[1])
            elif kind == "res":
                getattr(r, arg[0])[arg[1]] = 1
            elif kind == "nanf":
                arrays[arg[0]].reshape(-1).view(np.float64)[arg[1]] = NAN
        keep.append((self.name, r, False))
        return None if null else C.byref(r)

    @staticmethod
    def put(r, f, v):
        if isinstance(v, Named):
            v = v.value
        if isinstance(v, tuple):
            v = type(getattr(r, f))(*v)
        setattr(r, f, v)


def rows_of(L, entry, args, pairs=True, tag="", bare=True):
    """the bare call (valid where its state allows), every single mutation, every pair of mutations of different targets"""
    fn = getattr(L, entry)
    muts = [m for a in args for m in a.mutations()]
    cases = ([("valid", [])] if bare else []) + [(m[0], [m]) for m in muts]
    if pairs:
        cases += [("%s + %s" % (a[0], b[0]), [a, b]) for a, b in itertools.combinations(muts, 2) if a[1] != b[1]]
    rows = []
    for label, active in cases:
        keep, cargs = [], []
        for a in args:
            mine = [m[2] for m in active if m[1] == a.name or m[1].startswith(a.name + ".")]
            cargs.append(a.make(mine, keep))
        rc = fn(*cargs)
        err = L.rts_last_error().decode(errors="replace") if rc else ""
        outs = []
        for name, v, out in keep:
            if out:
                outs.append([name, sha(v) if isinstance(v, np.ndarray) else repr(v.value)])
        rows.append({"entry": entry + tag, "case": label, "rc": rc, "err": err, "out": outs})
    return rows


# ---------------------------------------------------------------------------------------------- the records, once for both parts
def cube_params(lib_mod, **kw):
    f = dict(n_rx=N_RX, n_pulses=N_P, n_bins=N_B, t0=0.0, dt=1e-8); f.update(kw)
    return Record("q", lib_mod.RtsCubeParams, f, bad=dict(n_rx=[0], n_pulses=[0], n_bins=[0], dt=[0.0, NAN], t0=[INF]), reserved=())


def complex_cube(seed=1, rows=N_P):
    return rnd(seed, N_RX, rows, N_B, 2)


SRC_FIELDS = dict(source=[3, 2], n_rows_in=[4, N_P], first_row=[N_P], n_rows=[N_P + 1], device_in=[BAD_PTR])


def rec_source(M):
    return Record("p", M.RtsSourceParams, dict(n_patches=2, flags=0, spatial=rnd(2, 2, N_RX, 2), power=np.array([1.0, 0.5]), doppler=np.array([0.1, -0.2]), rho=np.array([0.5, 0.9]), seed=7),
                  bad=dict(n_patches=[0, 1025], flags=[1]), nan=dict(spatial=1, power=1, doppler=0, rho=1), null_fields=())


def rec_cfar_os(M):
    return Record("p", M.RtsCfarOsParams, dict(guard_range=1, guard_doppler=1, train_range=2, train_doppler=1, rank=20, flags=0, pfa=1e-2, alpha=0.0, pri=1e-3, max_detections=0),
                  bad=dict(guard_range=[17], guard_doppler=[17], train_range=[17, 0], train_doppler=[17, 4], rank=[0, U32MAX], flags=[2], pfa=[1.5, 0.0], alpha=[2.0, NAN], pri=[-1.0, NAN]),
                  reserved=("reserved0", "reserved"))


def rec_cfar(M):
    return Record("p", M.RtsCfarParams, dict(guard_range=1, guard_doppler=1, train_range=2, train_doppler=1, mode=0, flags=0, pfa=1e-2, alpha=0.0, pri=1e-3, max_detections=0),
                  bad=dict(guard_range=[17], guard_doppler=[17], train_range=[17, 0], train_doppler=[17, 4], mode=[3, 1], flags=[2], pfa=[1.5, 0.0], alpha=[2.0, NAN], pri=[-1.0, NAN]),
                  reserved=("reserved0", "reserved"))


def rec_plot(M):
    return Record("p", M.RtsPlotParams, dict(link_range=1, link_doppler=1, min_cells=1, max_plots=0, pri=1e-3, device_list=0, n_list=0, n_doppler=0),
                  bad=dict(link_range=[5], link_doppler=[5], pri=[-1.0, NAN], device_list=[BAD_PTR], n_list=[3], n_doppler=[4]))


def rec_track(M):
    return Record("p", M.RtsTrackParams, dict(gate=9.0, sigma_delay=1e-8, sigma_doppler=10.0, q=1.0, delay_rate_per_hz=0.0, doppler_period=0.0, confirm_hits=2, max_misses=2,
                                              tentative_misses=1, max_candidates=4, max_tracks=16, n_plots=0, device_plots=0),
                  bad=dict(gate=[0.0, NAN], sigma_delay=[0.0], sigma_doppler=[-1.0], q=[-1.0], delay_rate_per_hz=[NAN], doppler_period=[-1.0], confirm_hits=[0], max_candidates=[0, 17],
                           max_tracks=[65537], n_plots=[5], device_plots=[BAD_PTR]))


def rec_tbd(M):
    return Record("p", M.RtsTbdParams, dict(half_doppler=1, half_range=2, depth=4, score=0, flags=0, scale=1.0, decay=0.9, delay_rate_per_hz=0.0, pri=1e-3),
                  bad=dict(half_doppler=[4], half_range=[16], depth=[0, 65], score=[2], flags=[2], scale=[0.0, NAN], decay=[0.0, 1.5], delay_rate_per_hz=[NAN], pri=[-1.0]),
                  reserved=("reserved0", "reserved"))


def rec_tbd_extract(M):
    return Record("e", M.RtsTbdExtractParams, dict(threshold=100.0, pri=1e-3, flags=0, max_tracks=8), bad=dict(threshold=[NAN], pri=[-1.0], flags=[2], max_tracks=[65537]))


def rec_stft(M):
    return Record("p", M.RtsStftParams, dict(first_pulse=0, n_pulses=N_P, window_len=4, hop=2, n_fft=4, first_bin=0, n_bins=0, flags=0, window=np.array([0.5, 1.0, 1.0, 0.5])),
                  bad=dict(first_pulse=[N_P], n_pulses=[0, N_P + 1], window_len=[0, 5], hop=[0], n_fft=[3, 0, 8192], first_bin=[N_B], n_bins=[N_B + 1], flags=[4, 2]), nan=dict(window=2))


def rec_align(M):
    return Record("p", M.RtsAlignParams, dict(first_pulse=0, n_pulses=N_P, first_bin=0, n_gate=0, max_lag=2, n_iters=1, flags=0),
                  bad=dict(first_pulse=[N_P], n_pulses=[0, N_P + 1], first_bin=[N_B], n_gate=[N_B + 1], max_lag=[65], n_iters=[0, 9], flags=[2]), reserved=("reserved0", "reserved"))


def rec_pga(M):
    return Record("p", M.RtsPgaParams, dict(first_pulse=0, n_pulses=N_P, first_bin=0, n_gate=0, n_iters=2, window0=0, window_min=0),
                  bad=dict(first_pulse=[N_P], n_pulses=[0, 6, 8192], first_bin=[N_B], n_gate=[N_B + 1], n_iters=[0, 17]), reserved=("reserved0", "reserved"))


def rec_correct(M, handle=False):
    return Record("p", M.RtsCorrectParams, dict(first_pulse=0, n_pulses=N_P, taps=4, flags=0, shifts=0.25 * rnd(3, N_RX, N_P), phase=rnd(4, N_RX, N_P)),
                  bad=dict(first_pulse=[N_P], n_pulses=[0, N_P + 1], taps=[3, 66, 0], flags=[1, 2, 4]), nan=dict(shifts=3, phase=5))


def rec_beat(M):
    return Record("p", M.RtsBeatParams, dict(slope=1e12, duration=1e-6, source=0, flags=0), bad=dict(slope=[0.0, NAN], duration=[0.0, INF], source=[2], flags=[2]))


def rec_range(M):
    return Record("p", M.RtsRangeParams, dict(first_pulse=0, n_pulses=N_P, first_bin=0, n_samples=0, n_fft=16, n_out=0, flags=0, window=np.hanning(N_B) + 0.1),
                  bad=dict(first_pulse=[N_P], n_pulses=[0, N_P + 1], first_bin=[N_B], n_samples=[N_B + 1], n_fft=[3, 8, 8192], n_out=[17], flags=[2]), reserved=("reserved0", "reserved"),
                  nan=dict(window=7))


def rec_image(M):
    tx = np.tile(np.array([0.0, -100.0, 10.0]), (N_P, 1)) + 0.1 * rnd(5, N_P, 3)
    rx = np.tile(np.array([1.0, -100.0, 10.0]), (N_RX, N_P, 1)) + 0.1 * rnd(6, N_RX, N_P, 3)
    return Record("p", M.RtsImageParams, dict(n_x=3, n_y=2, taps=4, flags=0, first_pulse=0, n_pulses=N_P, origin=(0.0, 0.0, 0.0), step_x=(0.5, 0.0, 0.0), step_y=(0.0, 0.5, 0.0),
                                              cspeed=3e8, carrier=1e9, tx_position=tx, rx_position=rx, pulse_weight=np.ones(N_P)),
                  bad=dict(n_x=[0], n_y=[0], taps=[3], flags=[2], first_pulse=[N_P], n_pulses=[0, N_P + 1], origin=[(0.0, NAN, 0.0)], step_x=[(INF, 0.0, 0.0)], step_y=[(0.0, 0.0, NAN)],
                           cspeed=[0.0, NAN], carrier=[-1.0]), nan=dict(tx_position=4, rx_position=7, pulse_weight=2))


def rec_beam(M):
    return Record("p", M.RtsBeamParams, dict(n_beams=2, source=0, first_row=0, n_rows=0, n_rows_in=0, flags=0, weights=rnd(7, 2, N_RX, 2), device_in=0),
                  bad=dict(n_beams=[0, 1025], flags=[4, 3], **SRC_FIELDS), nan=dict(weights=3))


def rec_cov(M):
    return Record("p", M.RtsCovParams, dict(source=0, n_rows_in=0, first_row=0, n_rows=0, first_bin=0, n_bins=0, skip_first_bin=0, skip_n_bins=0, device_in=0),
                  bad=dict(first_bin=[N_B], n_bins=[N_B + 1], skip_first_bin=[3], skip_n_bins=[N_B, N_B + 1], **SRC_FIELDS))


def rec_mvdr(M, n_rx=N_RX):
    return Record("p", M.RtsMvdrParams, dict(n_beams=2, n_rx=n_rx, loading=0.1, steering=rnd(8, 2, N_RX, 2), device_cov=0),
                  bad=dict(n_beams=[0, 1025], n_rx=[3], loading=[-1.0, NAN]), nan=dict(steering=2))


def rec_st_cov(M):
    return Record("p", M.RtsStCovParams, dict(source=0, n_rows_in=0, first_row=0, n_rows=0, first_bin=0, n_bins=0, skip_first_bin=0, skip_n_bins=0, n_taps=2, device_in=0),
                  bad=dict(first_bin=[N_B], n_bins=[N_B + 1], skip_first_bin=[3], skip_n_bins=[N_B, N_B + 1], n_taps=[0, 17, 33], **SRC_FIELDS), reserved=("reserved0", "reserved"))


def rec_st_apply(M):
    f = dict(SRC_FIELDS); f["n_rows"] = [N_P + 1, 1]
    return Record("p", M.RtsStApplyParams, dict(n_filters=2, source=0, first_row=0, n_rows=0, n_rows_in=0, flags=0, n_taps=2, weights=rnd(9, 2, 2 * N_RX, 2), device_in=0),
                  bad=dict(n_filters=[0, 1025], flags=[2, 4], n_taps=[0, 17, 33], **f), reserved=("reserved0", "reserved"), nan=dict(weights=5))


def hermitian(n, seed):
    a = rnd(seed, n, n) + 1j * rnd(seed + 1, n, n)
    return np.ascontiguousarray(a @ a.conj().T + n * np.eye(n)).view(np.float64).reshape(n, n, 2)


# ---------------------------------------------------------------------------------------------- the host part
def host_rows(M):
    L = M.lib()
    u32, u64, dbl = C.c_uint32, C.c_uint64, C.c_double
    q = lambda **kw: cube_params(M, **kw)
    cube = complex_cube()
    rows = []
    add = lambda entry, args, **kw: rows.extend(rows_of(L, entry, args, **kw))

    add("rts_sources_eval", [q(), rec_source(M), Array("cube_inout", cube, out=True)])
    dmap = np.abs(rnd(10, N_RX, N_D, N_B, 2)) + 0.1; dmap[1, 3, 7] = 400.0; dmap[0, 5, 9] = 300.0
    det = np.zeros(64, M.DETECTION_DTYPE)
    add("rts_cfar_os_eval", [q(), Array("map", dmap, nan=40), Scalar("n_doppler", u32, N_D, [0]), rec_cfar_os(M), Array("out", det, out=True), Scalar("capacity", u32, 64), Out("n_out", u32)])
    lst = np.zeros(3, M.DETECTION_DTYPE); lst["rx"] = [0, 0, 1]; lst["doppler_bin"] = [2, 2, 3]; lst["range_bin"] = [4, 5, 7]; lst["power"] = [3.0, 2.0, 5.0]; lst["noise"] = 1.0

    def swap(a):
        a[[0, 1]] = a[[1, 0]]

    def outside(a):
        a["rx"][1] = 99
    add("rts_plots_eval", [q(), Array("list", lst, alts=dict(unsorted=swap, outside=outside)), Scalar("n_list", u32, 3, [0x40000001]), Scalar("n_doppler", u32, N_D, [0]), rec_plot(M),
                           Array("out", np.zeros(8, M.PLOT_DTYPE), out=True), Scalar("capacity", u32, 8), Out("n_out", u32)])
    trk = np.zeros(2, M.TRACK_DTYPE); trk["id"] = [1, 2]; trk["rx"] = [0, 1]; trk["delay"] = [1e-7, 2e-7]; trk["doppler"] = [5.0, -5.0]; trk["p_dd"] = 1e-16; trk["p_ff"] = 100.0
    plots = np.zeros(3, M.PLOT_DTYPE); plots["rx"] = [0, 0, 1]; plots["delay"] = [1e-7, 5e-7, 2e-7]; plots["doppler"] = [5.0, 50.0, -5.0]; plots["power_sum"] = 1.0

    def nan_delay(a):
        a["delay"][0] = NAN

    def bad_flags(a):
        a["flags"][1] = 0x80

    def rx_down(a):
        a["rx"][2] = 0; a["rx"][1] = 1
    add("rts_tracks_eval", [rec_track(M), Array("in", np.concatenate([trk, np.zeros(15, M.TRACK_DTYPE)]), alts=dict(nan=nan_delay, flags=bad_flags)), Scalar("n_in", u32, 2, [17]), Scalar("next_id", u64, 3), Scalar("T", dbl, 1.0, [0.0, NAN]),
                            Array("plots", plots, alts=dict(rx_decreases=rx_down)), Scalar("n_plots", u32, 3, [16777217]), Array("out", np.zeros(16, M.TRACK_DTYPE), out=True), Scalar("capacity", u32, 16),
                            Out("n_out", u32), Out("next_id_out", u64)])
    cells = N_RX * N_D * N_B
    merit_in = np.abs(rnd(11, cells))
    tbd_args = lambda: [q(), Array("map", dmap, nan=9), Scalar("n_doppler", u32, N_D, [0]), Array("merit_in", merit_in), rec_tbd(M), Scalar("T", dbl, 1.0, [0.0, NAN]),
                        Array("merit_out", np.zeros(cells), out=True), Array("ptr_out", np.zeros(cells, np.uint8), out=True), Array("shifts_out", np.zeros(N_D, np.int32), out=True)]
    add("rts_tbd_step_eval", tbd_args())
    # a ring of one frame for the extraction: the step's own outputs (pointer bytes only the step can make)
    keep = []; cargs = [a.make([], keep) for a in tbd_args()]
    assert L.rts_tbd_step_eval(*cargs) == 0
    made = {n: v for n, v, _ in keep}
    add("rts_tbd_extract_eval", [q(), Scalar("n_doppler", u32, N_D, [0]), rec_tbd(M), Array("merit", made["merit_out"], nan=5), Array("ptrs", made["ptr_out"]), Array("shifts", made["shifts_out"]),
                                 Scalar("n_frames", u32, 1, [0, 5]), rec_tbd_extract(M), Array("out", np.zeros(8, M.TBD_TRACK_DTYPE), out=True), Array("paths", np.zeros(2 * 4 * 8, np.uint32), out=True),
                                 Scalar("capacity", u32, 8), Out("n_out", u32)])
    add("rts_stft_eval", [q(), Array("cube", cube, nan=11), rec_stft(M), Array("out", np.zeros(4096), out=True), Out("n_frames_out", u32)])
    add("rts_align_eval", [q(), Array("cube", cube, nan=11), rec_align(M), Array("out", np.zeros(256), out=True)])
    add("rts_pga_eval", [q(), Array("cube", cube, nan=11), rec_pga(M), Array("phase_out", np.zeros(256), out=True), Array("rms_out", np.zeros(256), out=True)])
    add("rts_correct_eval", [q(), Array("cube", cube, out=True), rec_correct(M)])
    con = np.zeros(2, M.BEAT_CONTRIBUTION_DTYPE); con["rx"] = [0, 1]; con["re"] = [1.0, 0.5]; con["im"] = [0.0, -0.5]; con["delay"] = [3e-8, 5e-8]; con["doppler"] = [10.0, -10.0]
    add("rts_beat_eval", [q(), rec_beat(M), Array("c", con), Scalar("n", u32, 2), Scalar("pulse_index", u32, 1, [N_P]), Array("cube", cube, out=True)])
    add("rts_range_eval", [q(), Array("cube", cube, nan=11), rec_range(M), Array("out", np.zeros(4096), out=True)])
    add("rts_backproject_eval", [q(), Array("cube", cube, nan=11), rec_image(M), Array("out", np.zeros(2 * N_RX * 2 * 3), out=True)])
    add("rts_beamform_eval", [q(), Array("in", cube, nan=11), Scalar("n_rows_in", u32, N_P, [0]), rec_beam(M), Array("out", np.zeros(1024), out=True)])
    add("rts_covariance_eval", [q(), Array("in", cube, nan=11), Scalar("n_rows_in", u32, N_P, [0]), rec_cov(M), Array("out", np.zeros(2 * N_RX * N_RX), out=True)])
    add("rts_mvdr_eval", [Array("cov", hermitian(N_RX, 12), nan=0), Scalar("n_rx", u32, N_RX, [0]), rec_mvdr(M), Array("out", np.zeros(2 * 2 * N_RX), out=True)])
    add("rts_st_covariance_eval", [q(), Array("in", cube, nan=11), Scalar("n_rows_in", u32, N_P, [0]), rec_st_cov(M), Array("out", np.zeros(2 * 16 * N_RX * N_RX), out=True)])
    add("rts_st_apply_eval", [q(), Array("in", cube, nan=11), Scalar("n_rows_in", u32, N_P, [0]), rec_st_apply(M), Array("out", np.zeros(2048), out=True)])
    add("rts_eig_eval", [Array("cov", hermitian(3, 14), nan=0), Scalar("n", u32, 3, [0, 65]), Array("values_out", np.zeros(3), out=True), Array("vectors_out", np.zeros(18), out=True), Out("sweeps_out", u32)])
    vec = np.zeros((3, 3, 2)); vec[0, 0, 0] = vec[1, 1, 0] = vec[2, 2, 0] = 1.0
    add("rts_doa_scan_eval", [Array("vectors", vec, nan=3), Array("g", np.array([1.0, 0.5]), nan=1), Scalar("n", u32, 3, [0, 65]), Scalar("m", u32, 2, [0, 4]), Array("steering", rnd(15, 5, 3, 2), nan=2),
                              Scalar("n_dirs", u64, 5, [0]), Scalar("flags", u32, 0, [2]), Array("out", np.zeros(5), out=True)])
    add("rts_waveform_eval", [Record("w", M.RtsWaveform, dict(samples=rnd(16, 4, 2), n_samples=4, taps=2), bad=dict(n_samples=[0, 4097], taps=[0, 3, 66]), nan=dict(samples=3)),
                              Array("x", np.array([0.0, 1.5, 2.75])), Scalar("n", u32, 3), Array("out", np.zeros(6), out=True)])
    add("rts_noise_eval", [Scalar("seed", u64, 99), Array("index", np.array([0, 1, 1 << 40], np.uint64)), Scalar("n", u32, 3), Scalar("noise_power", dbl, 2.0, [-1.0, NAN, INF]), Array("out", np.zeros(6), out=True)])
    for kind in range(4):
        add("rts_window_make", [Scalar("kind", u32, kind, [4] if kind == 0 else []), Scalar("n", u32, 7, [0] if kind == 0 else []), Array("out", np.zeros(7), out=True, null=kind == 0)], tag="" if kind == 0 else "[kind %d]" % kind)
    add("rts_cfar_os_alpha", [Scalar("n_train", u32, 26, [0]), Scalar("rank", u32, 20, [0, 27]), Scalar("pfa", dbl, 1e-3, [0.0, 1.5, NAN]), Out("alpha", dbl)])
    add("rts_steering_make", [Array("positions", rnd(17, N_RX, 3), nan=4), Scalar("n_rx", u32, N_RX, [0]), Array("directions", np.array([[0.1, 0.0], [-0.2, 0.05]]), nan=1), Scalar("n_beams", u32, 2, [0]),
                              Scalar("wavelength", dbl, 0.03, [0.0, NAN]), Array("taper", np.array([1.0, 0.5]), nan=1), Array("weights_out", np.zeros(2 * 2 * N_RX), out=True)])
    add("rts_st_steering_make", [Array("spatial", rnd(18, 2, N_RX, 2), nan=1), Scalar("n_rx", u32, N_RX, [0]), Scalar("n_beams", u32, 2, [0]), Array("doppler", np.array([0.1, -0.25, 0.4]), nan=2),
                                 Scalar("n_doppler", u32, 3, [0]), Scalar("n_taps", u32, 2, [0, 17, 33]), Array("tap_taper", np.array([1.0, 0.7]), nan=0), Array("out", np.zeros(2 * 2 * 3 * 2 * N_RX), out=True)])
    for method in range(3):
        first = method == 2
        add("rts_doa_weights", [Scalar("method", u32, method, [3] if first else []), Array("values", np.array([3.0, 2.0, 0.5]), nan=1 if first else None, null=first), Scalar("n", u32, 3, [0, 65] if first else []),
                                Scalar("n_sources", u32, 1, [3] if first else []), Scalar("loading", dbl, 0.25, [-1.0, NAN] if first else []), Out("first", u32), Out("m", u32),
                                Array("g", np.zeros(64), out=True, null=first), Out("flags", u32)], pairs=first, tag="" if first else "[method %d]" % method)

    def unsorted(a):
        a[1] = 9.0

    def negative(a):
        a[2] = -1.0
    add("rts_source_count", [Array("values", np.array([3.0, 2.0, 0.5]), nan=1, alts=dict(unsorted=unsorted, negative=negative)), Scalar("n", u32, 3, [0, 65]), Scalar("K", u64, 100, [0]),
                             Scalar("criterion", u32, 1, [2]), Out("n_sources", u32)])
    return rows


# ---------------------------------------------------------------------------------------------- the handle part
def handle_rows(M):
    import torch
    from rts_amd import api
    L = M.lib()
    vp, u32, u64, dbl = C.c_void_p, C.c_uint32, C.c_uint64, C.c_double
    rows = []
    state = {}

    def dev(a):
        t = torch.from_numpy(np.ascontiguousarray(a)).to("cuda"); torch.cuda.synchronize(); return t

    def row(entry, case, rc, outs=()):
        rows.append({"entry": entry, "case": case, "rc": rc, "err": L.rts_last_error().decode(errors="replace") if rc else "", "out": [[n, sha(v)] for n, v in outs]})

    class Handle:
        name = "c"

        def mutations(self):
            return []

        def make(self, m, keep):
            return state["tr"].h

    class DevOut:
        """device_out of a call: NULL (library-owned); the mutations: misaligned, and on top of the cube the call reads"""
        def __init__(self, name="device_out", overlap=True):
            self.name, self.overlap = name, overlap

        def mutations(self):
            ms = [("%s misaligned" % self.name, self.name, ("ptr", state["scratch"].data_ptr() + 8))]
            return ms + ([("%s in place" % self.name, self.name, ("ptr", state["cube"].data_ptr()))] if self.overlap else [])

        def make(self, m, keep):
            m = dict(m)
            return vp(m["ptr"]) if "ptr" in m else None

    def get(entry, doubles):
        out = np.zeros(doubles)
        rc = getattr(L, entry)(state["tr"].h, out.ctypes.data, out.size)
        row(entry, "valid", rc, [("host_out", out)])
        return out

    # no cube: every entry point on a fresh handle
    tr = api.Tracer(8, 1); state["tr"] = tr
    state["scratch"] = dev(np.zeros(65536)); cube_h = complex_cube(21); state["cube"] = dev(cube_h)
    H, O = Handle(), DevOut
    wave = Record("w", M.RtsWaveform, dict(samples=rnd(16, 4, 2), n_samples=4, taps=2), bad=dict(n_samples=[0, 4097], taps=[0, 3, 66]), nan=dict(samples=3))
    calls = [("rts_cube_add_sources", [H, rec_source(M)]), ("rts_cube_detect", [H, rec_cfar(M), Scalar("device_map", vp, None), Scalar("n_doppler", u32, 0)]),
             ("rts_cube_detect_os", [H, rec_cfar_os(M), Scalar("device_map", vp, None), Scalar("n_doppler", u32, 0)]), ("rts_cube_plots", [H, rec_plot(M)]),
             ("rts_cube_tbd_step", [H, rec_tbd(M), Scalar("time", dbl, 1.0, [NAN]), Scalar("device_map", vp, None), Scalar("n_doppler", u32, 0)]),
             ("rts_cube_spectrogram", [H, rec_stft(M), O(overlap=False), Out("n_frames_out", u32)]), ("rts_cube_align", [H, rec_align(M), O(overlap=False)]),
             ("rts_cube_pga", [H, rec_pga(M), O(overlap=False)]), ("rts_cube_correct", [H, rec_correct(M)]),
             ("rts_cube_render_beat", [H, Scalar("pulse_index", u32, 1, [N_P]), rec_beat(M), Scalar("cspeed", dbl, 3e8, [0.0, NAN]), Scalar("carrier", dbl, 1e9, [-1.0])]),
             ("rts_cube_range_transform", [H, rec_range(M), O(overlap=False)]), ("rts_cube_backproject", [H, rec_image(M), O(overlap=False)]),
             ("rts_cube_beamform", [H, rec_beam(M), O()]), ("rts_cube_covariance", [H, rec_cov(M), O()]), ("rts_cube_st_covariance", [H, rec_st_cov(M), O()]),
             ("rts_cube_st_apply", [H, rec_st_apply(M), O()]), ("rts_cube_mvdr", [H, rec_mvdr(M, 0), O(overlap=False)]),
             ("rts_cube_eig", [H, Record("p", M.RtsEigParams, dict(n=0, device_cov=0), bad=dict(n=[5], device_cov=[BAD_PTR]), reserved=("reserved0", "reserved")), O("device_values", False), Scalar("device_vectors", vp, None)]),
             ("rts_cube_set_waveform", [H, wave]),
             ("rts_cube_render", [H, Scalar("pulse_index", u32, 1, [N_P]), Scalar("source", u32, 0, [2]), Scalar("flags", u32, 0, [2]), Scalar("cspeed", dbl, 3e8), Scalar("carrier", dbl, 1e9)]),
             ("rts_cube_compress", [H, Scalar("first_pulse", u32, 0, [N_P]), Scalar("n_pulses", u32, N_P, [N_P + 1])]),
             ("rts_cube_add_noise", [H, Scalar("first_pulse", u32, 0, [N_P]), Scalar("n_pulses", u32, N_P, [N_P + 1]), Scalar("noise_power", dbl, 0.5, [-1.0, NAN]), Scalar("seed", u64, 5)]),
             ("rts_cube_doppler", [H, Scalar("n_fft", u32, N_D, [3, 4, 8192]), Scalar("device_out", vp, None)])]
    for entry, args in calls:
        keep = []
        row(entry, "no cube", getattr(L, entry)(*[a.make([], keep) for a in args]))
    for entry in ("rts_cube_get", "rts_cube_doppler_get", "rts_cube_image_get", "rts_cube_spectrogram_get", "rts_cube_align_get", "rts_cube_range_get", "rts_cube_beam_get",
                  "rts_cube_covariance_get", "rts_cube_mvdr_get", "rts_cube_st_get", "rts_cube_doa_get"):
        out = np.zeros(8); row(entry, "no cube", getattr(L, entry)(tr.h, out.ctypes.data, out.size))
    # the cube; then every record's single and paired mutations: all but the bare call are refused before anything is launched
    tr.cube_attach(N_RX, N_P, N_B, 0.0, 1e-8, device_ptr=state["cube"].data_ptr())
    no_state = [("rts_cube_detect", "no map"), ("rts_cube_detect_os", "no map"), ("rts_cube_plots", "no list"), ("rts_cube_mvdr", "no covariance"), ("rts_cube_eig", "no covariance"),
                ("rts_cube_render", "no waveform"), ("rts_cube_compress", "no waveform")]
    for entry, case in no_state:
        keep = []; args = dict(calls)[entry]
        row(entry, case, getattr(L, entry)(*[a.make([], keep) for a in args]))
    n = u32(0); buf = np.zeros(8, M.DETECTION_DTYPE)
    row("rts_cube_detections_get", "no list", L.rts_cube_detections_get(tr.h, buf.ctypes.data, 8, C.byref(n)))
    doa = Record("p", M.RtsDoaScanParams, dict(n=0, first_vector=0, m=1, flags=0, n_dirs=5, g=np.array([1.0]), device_steering=0, device_vectors=0),
                 bad=dict(first_vector=[3], m=[0, 4], flags=[2], n_dirs=[0], device_vectors=[BAD_PTR]), nan=dict(g=0))
    keep = []; row("rts_cube_doa_scan", "no eigenvectors", L.rts_cube_doa_scan(tr.h, doa.make([], keep), None))
    bp = rec_beam(M); keep = []
    row("rts_cube_beamform", "no map (RTS_BEAM_FROM_MAP)", L.rts_cube_beamform(tr.h, bp.make([("set", ("source", 1))], keep), None))
    order = ["rts_cube_set_waveform", "rts_cube_doppler", "rts_cube_detect", "rts_cube_detect_os", "rts_cube_plots", "rts_cube_tbd_step", "rts_cube_spectrogram", "rts_cube_align", "rts_cube_pga",
             "rts_cube_range_transform", "rts_cube_backproject", "rts_cube_beamform", "rts_cube_covariance", "rts_cube_mvdr", "rts_cube_st_apply", "rts_cube_st_covariance", "rts_cube_eig",
             "rts_cube_add_noise", "rts_cube_compress", "rts_cube_add_sources", "rts_cube_correct"]
    for entry in order:                                  # (the products of one are the next one's state: map -> list -> plots, covariance -> weights, eigenpairs)
        rows.extend(rows_of(L, entry, dict(calls)[entry]))
    steer = dev(rnd(15, 5, 2 * N_RX, 2))
    doa.fields["device_steering"] = steer.data_ptr(); doa.bad["device_steering"] = [0, Named("misaligned", steer.data_ptr() + 8)]
    rows.extend(rows_of(L, "rts_cube_doa_scan", [H, doa, O(overlap=False)]))
    # render and beat render on the attached cube: their refusals only (every mutation is refused whatever the others are; a valid call needs a traced pulse)
    rows.extend(rows_of(L, "rts_cube_render", dict(calls)["rts_cube_render"], bare=False))
    rows.extend(rows_of(L, "rts_cube_render_beat", dict(calls)["rts_cube_render_beat"], bare=False))
    for entry, args in (("rts_cube_accumulate", [H, Scalar("pulse_index", u32, 0, [N_P]), Scalar("cspeed", dbl, 3e8), Scalar("carrier", dbl, 1e9)]), ("rts_cube_accumulate_paths", [H, Scalar("pulse_index", u32, 0, [N_P])])):
        rows.extend(rows_of(L, entry, args, bare=entry.endswith("paths")))      # (without an aggregation _paths is refused; a bare rts_cube_accumulate needs a traced pulse)
    # the tracker on the handle's plots: a step, its table through the getter at a capacity below it, a loaded table, the reset
    trk = np.zeros(2, M.TRACK_DTYPE); trk["id"] = [1, 2]; trk["rx"] = [0, 1]; trk["delay"] = [1e-7, 2e-7]; trk["doppler"] = [5.0, -5.0]; trk["p_dd"] = 1e-16; trk["p_ff"] = 100.0

    def nan_delay(a):
        a["delay"][0] = NAN
    tracks_get = lambda cap: [H, Array("out", np.zeros(max(cap, 1), M.TRACK_DTYPE), out=True, null=cap != 0), Scalar("capacity", u32, cap), Out("n_out", u32), Out("next_id_out", u64)]
    rows.extend(rows_of(L, "rts_cube_track", [H, rec_track(M), Scalar("time", dbl, 1.0, [NAN])]))
    rows.extend(rows_of(L, "rts_cube_tracks_get", tracks_get(4096), pairs=False, tag="[after a step]"))
    rows.extend(rows_of(L, "rts_cube_track_rounds", [H, Out("rounds", u32)], pairs=False))
    rows.extend(rows_of(L, "rts_cube_tracks_set", [H, Array("tracks", trk, alts=dict(nan=nan_delay)), Scalar("n", u32, 2, [65537]), Scalar("next_id", u64, 3), Scalar("time", dbl, 2.0, [NAN])]))
    for cap in (2, 1, 0):
        rows.extend(rows_of(L, "rts_cube_tracks_get", tracks_get(cap), pairs=False, tag="[2 loaded, capacity %d]" % cap))
    rows.extend(rows_of(L, "rts_cube_track", [H, rec_track(M), Scalar("time", dbl, 2.0)], pairs=False, tag="[T = 0 on a loaded table]", bare=True)[:1])
    row("rts_cube_tracks_reset", "valid", L.rts_cube_tracks_reset(tr.h))
    rows.extend(rows_of(L, "rts_cube_tracks_get", tracks_get(4), pairs=False, tag="[after the reset]"))
    # track-before-detect: the getters without an extraction, an extraction that finds more than it may store, its records and paths at capacities below them, the state's maps, the reset
    ex = rec_tbd_extract(M); ex.fields["threshold"] = -1.0; ex.fields["max_tracks"] = 3
    tbd_tracks = lambda cap: [H, Array("out", np.zeros(max(cap, 1), M.TBD_TRACK_DTYPE), out=True, null=cap != 0), Scalar("capacity", u32, cap), Out("n_out", u32)]
    tbd_paths = lambda cap: [H, Array("out", np.zeros(2 * 4 * max(cap, 1), np.uint32), out=True, null=cap != 0), Scalar("capacity_tracks", u32, cap)]
    tbd_maps = [("rts_cube_tbd_merit_get", [H, Array("host_out", np.zeros(N_RX * N_D * N_B), out=True), Scalar("capacity_doubles", u64, N_RX * N_D * N_B, [1])]),
                ("rts_cube_tbd_ring_get", [H, Array("ptr_out", np.zeros(4 * N_RX * N_D * N_B, np.uint8), out=True), Array("shifts_out", np.zeros(4 * N_D, np.int32), out=True), Scalar("capacity_frames", u32, 4, [0]), Out("n_frames_out", u32)]),
                ("rts_cube_tbd_info", [H, Array("shape_out", np.zeros(4, np.uint32), out=True, cast=C.POINTER(u32 * 4)), Out("frames_out", u64)])]
    rows.extend(rows_of(L, "rts_cube_tbd_tracks_get", tbd_tracks(8), pairs=False, tag="[no extraction]", bare=True)[:1])
    rows.extend(rows_of(L, "rts_cube_tbd_paths_get", tbd_paths(8), pairs=False, tag="[no extraction]", bare=True)[:1])
    rows.extend(rows_of(L, "rts_cube_tbd_extract", [H, ex]))
    for cap in (8, 2, 0):
        rows.extend(rows_of(L, "rts_cube_tbd_tracks_get", tbd_tracks(cap), pairs=False, tag="[capacity %d]" % cap))
        rows.extend(rows_of(L, "rts_cube_tbd_paths_get", tbd_paths(cap), pairs=False, tag="[capacity %d]" % cap))
    for entry, args in tbd_maps:
        rows.extend(rows_of(L, entry, args, pairs=False))
    row("rts_cube_tbd_reset", "valid", L.rts_cube_tbd_reset(tr.h))
    for entry, args in [("rts_cube_tbd_extract", [H, ex]), ("rts_cube_tbd_tracks_get", tbd_tracks(8)), ("rts_cube_tbd_paths_get", tbd_paths(8))] + tbd_maps:
        rows.extend(rows_of(L, entry, args, pairs=False, tag="[after the reset]", bare=True)[:1])
    # the eigenpairs and the phase table behind their getters: both outputs, one, none, a capacity below the product
    eig_n = 2 * N_RX                                       # (the handle's covariance is the stacked one: two taps)
    rows.extend(rows_of(L, "rts_cube_eig_get", [H, Array("values_out", np.zeros(eig_n), out=True), Array("vectors_out", np.zeros(2 * eig_n * eig_n), out=True), Scalar("capacity_values", u64, eig_n, [eig_n - 1]),
                                                Scalar("capacity_vector_doubles", u64, 2 * eig_n * eig_n, [1])]))
    rows.extend(rows_of(L, "rts_cube_pga_get", [H, Array("phase_out", np.zeros(N_RX * N_P), out=True), Array("rms_out", np.zeros(N_RX * 2), out=True), Scalar("capacity_phase", u64, N_RX * N_P, [1]),
                                                Scalar("capacity_rms", u64, N_RX * 2, [1])]))
    # rts_cube_attach's refusals, on a handle of their own (an accepted attach would end this handle's products)
    tr2 = api.Tracer(8, 1); state["tr"] = tr2
    rows.extend(rows_of(L, "rts_cube_attach", [H, cube_params(M), Scalar("device_ptr", vp, None)], bare=False, tag="[refusals]"))
    state["tr"] = tr; tr2.close()
    # what the valid calls left, through the getters (each synchronises)
    q = tr.cube().shape
    get("rts_cube_get", 2 * N_RX * N_P * N_B); get("rts_cube_doppler_get", 2 * N_RX * N_D * N_B); get("rts_cube_beam_get", 2 * 2 * N_P * N_B); get("rts_cube_covariance_get", 2 * 16 * N_RX * N_RX)
    get("rts_cube_mvdr_get", 2 * 2 * N_RX); get("rts_cube_st_get", 2 * 2 * (N_P - 1) * N_B); get("rts_cube_doa_get", 5); get("rts_cube_align_get", 4096); get("rts_cube_range_get", 4096)
    get("rts_cube_spectrogram_get", 4096); get("rts_cube_image_get", 2 * N_RX * 2 * 3)
    buf = np.zeros(4096, M.DETECTION_DTYPE); row("rts_cube_detections_get", "valid", L.rts_cube_detections_get(tr.h, buf.ctypes.data, 4096, C.byref(n)), [("out", buf), ("n", np.array([n.value]))])
    row("rts_cube_detections_get", "capacity 0", L.rts_cube_detections_get(tr.h, None, 0, C.byref(n)), [("n", np.array([n.value]))])
    pb = np.zeros(4096, M.PLOT_DTYPE); row("rts_cube_plots_get", "valid", L.rts_cube_plots_get(tr.h, pb.ctypes.data, 4096, C.byref(n)), [("out", pb), ("n", np.array([n.value]))])
    assert q == (N_RX, N_P, N_B)
    tr.close()
    return rows


def main(argv):
    if len(argv) >= 3 and argv[0] == "diff":
        a, b = (json.load(open(p)) for p in argv[1:3])
        key = lambda r: (r["entry"], r["case"])
        da, db = {key(r): r for r in a}, {key(r): r for r in b}
        bad = 0
        for k in sorted(set(da) | set(db)):
            if da.get(k) != db.get(k):
                bad += 1
                print("DIFFERS %s | %s\n   a: %s\n   b: %s" % (k[0], k[1], json.dumps(da.get(k)), json.dumps(db.get(k))))
        print("%d rows in a, %d in b, %d differ" % (len(a), len(b), bad))
        return 1 if bad else 0
    if len(argv) >= 2 and argv[0] == "run":
        from rts_amd import _lib as M
        rows = handle_rows(M) if "--handle" in argv else host_rows(M)
        with open(argv[-1], "w") as f:
            json.dump(rows, f, indent=0)
        print("%d rows (%d refused) from %s -> %s" % (len(rows), sum(1 for r in rows if r["rc"]), M.LIB_PATH, argv[-1]))
        return 0
    print(__doc__)
    return 2


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
