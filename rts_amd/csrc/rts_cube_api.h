// rts_cube_api.h -- what the entry points of the cube part of the C-ABI share (rts_cube_api.hip, rts_cube_detect_api.hip, rts_cube_array_api.hip): the argument checks that more
// than one of them applies, each forming the message of the entry point `who` from the rules of rts_cube_args.h; where a call reads
// from; how a product or a counted list comes home.  Internal: no kernels, nothing of this is exported.
#pragma once
#include <cmath>
#include <cstring>
#include "rts_internal.h"
#include "rts_cube_args.h"

#define NEED_CUBE(c, who, wording) do { if (!(c)->cube.set) { rts_set_error("%s: %s", (who), (wording)); return RTS_ERR_INVALID; } } while (0)

// ------------------------------------------------------------------------------------- spans, sizes
static inline int rts_pulses_check(const char* who, uint32_t first, uint32_t n, uint32_t rows, bool at_least_one)      // pulses first .. first + n inside the cube's rows; a product needs at least one
{
    if (rts_span_inside(first, n, rows, false, at_least_one)) return RTS_OK;
    if (at_least_one) rts_set_error("%s: first_pulse = %u, n_pulses = %u: at least one pulse, inside the cube's %u rows", who, first, n, rows);
    else rts_set_error("%s: pulses %u .. %u + %u outside the cube's %u", who, first, first, n, rows);
    return RTS_ERR_INVALID;
}

static inline int rts_taps_check(const char* who, uint32_t taps)      // the interpolator's support (rts_waveform.h): the nearest sample, or an even number of taps
{
    if (taps != 1u && (taps < 2u || taps > RTS_WAVEFORM_MAX_TAPS || (taps & 1u))) { rts_set_error("%s: taps = %u (1, or even in [2, %u])", who, taps, RTS_WAVEFORM_MAX_TAPS); return RTS_ERR_INVALID; }
    return RTS_OK;
}

static inline int rts_pulse_index_check(const char* who, uint32_t pulse_index, uint32_t rows)      // the row an impulse writer or the waveform render adds to
{
    if (pulse_index >= rows) { rts_set_error("%s: pulse %u >= %u", who, pulse_index, rows); return RTS_ERR_INVALID; }
    return RTS_OK;
}

// first .. first + n inside `total` bins or rows (n == 0: to the end, *count: how many that is); fmt: the entry point's sentence, which
// takes who, first, n and total ("%s: first_bin = %u, n_gate = %u: inside the cube's %u bins")
static inline int rts_gate_check(const char* who, const char* fmt, uint32_t first, uint32_t n, uint32_t total, uint32_t* count = nullptr)
{
    if (rts_span_inside(first, n, total, true, false, count)) return RTS_OK;
    rts_set_error(fmt, who, first, n, total);
    return RTS_ERR_INVALID;
}
static inline int rts_rows_check(const char* who, uint32_t first_row, uint32_t n_rows, uint32_t rows, uint32_t* count = nullptr)
{
    return rts_gate_check(who, "%s: first_row = %u, n_rows = %u: inside the source's %u rows", first_row, n_rows, rows, count);
}

// a transform length: a power of two in [lo, hi]
static inline int rts_fft_size_check(const char* who, uint32_t n_fft, uint32_t hi)
{
    if (!rts_pow2_in(n_fft, 2u, hi)) { rts_set_error("%s: n_fft = %u must be a power of two in [2, %u]", who, n_fft, hi); return RTS_ERR_INVALID; }
    return RTS_OK;
}

static inline int rts_window_finite_check(const char* who, const double* window, uint32_t n)      // (a null window is the rectangular one)
{
    if (window) for (uint32_t i = 0; i < n; i++) if (!std::isfinite(window[i])) { rts_set_error("%s: window[%u] is not finite", who, i); return RTS_ERR_INVALID; }
    return RTS_OK;
}

// the cube parameters an evaluator is given: n_rx and n_bins always, n_pulses and the time axis (dt, t0) where the evaluator reads them
static inline int rts_eval_cube_check(const char* who, const RtsCubeParams* q, bool pulses, bool time_axis)
{
    if (!q || q->n_rx == 0 || (pulses && q->n_pulses == 0) || q->n_bins == 0 || (time_axis && (!(q->dt > 0) || !std::isfinite(q->dt) || !std::isfinite(q->t0)))) {
        rts_set_error("%s: bad cube parameters", who); return RTS_ERR_INVALID; }
    return RTS_OK;
}

// ------------------------------------------------------------------------------------- where a beamformer-style call reads from (RTS_BEAM_FROM_CUBE / _MAP / _POINTER)
// The record's source fields, in two checks, because every record has reported the unknown source before its flags and limits and the
// n_rows_in / device_in rules after them, and a record with several wrong fields keeps reporting the one it reported
static inline int rts_source_known_check(const char* who, uint32_t source)
{
    if (source > RTS_BEAM_FROM_POINTER) {      // (rule 1 of rts_source_fields_rule)
        rts_set_error("%s: unknown source %u (RTS_BEAM_FROM_CUBE, _MAP, _POINTER)", who, source); return RTS_ERR_INVALID; }
    return RTS_OK;
}
static inline int rts_source_fields_check(const char* who, uint32_t source, uint32_t n_rows_in, const void* device_in)
{
    switch (rts_source_fields_rule(source, n_rows_in, device_in)) {
        case 0: return RTS_OK;
        case 1: return rts_source_known_check(who, source);      // (not reached where the record's first check has run)
        case 2: rts_set_error("%s: n_rows_in = %u without RTS_BEAM_FROM_POINTER", who, n_rows_in); break;
        case 3: rts_set_error("%s: device_in without RTS_BEAM_FROM_POINTER", who); break;
        default: rts_set_error("%s: n_rows_in = 0 with RTS_BEAM_FROM_POINTER", who); break;
    }
    return RTS_ERR_INVALID;
}
// an evaluator's array against the record that describes it
static inline int rts_source_rows_match_check(const char* who, uint32_t source, uint32_t n_rows_in, uint32_t n_rows_array)
{
    if (source == RTS_BEAM_FROM_POINTER && n_rows_in != n_rows_array) { rts_set_error("%s: the parameters' n_rows_in = %u, the array's %u", who, n_rows_in, n_rows_array); return RTS_ERR_INVALID; }
    return RTS_OK;
}
// the device source of a call and its rows: the cube, the LIBRARY-OWNED Doppler map (a caller-owned one may be gone), or the caller's pointer
static inline int rts_device_source(RtsContext* c, const char* who, uint32_t source, const void* device_in, uint32_t n_rows_in, const double** src, uint32_t* rows)
{
    *src = c->cube.p; *rows = c->cube.params.n_pulses;
    if (source == RTS_BEAM_FROM_MAP) {
        const RtsCubeProduct& m = c->cube.doppler.map;
        if (!m.valid || !m.own.p || m.p != m.own.p) { rts_set_error("%s: RTS_BEAM_FROM_MAP: no library-owned map (rts_cube_doppler with device_out NULL)", who); return RTS_ERR_INVALID; }
        *src = m.p; *rows = c->cube.doppler.n_fft;
    } else if (source == RTS_BEAM_FROM_POINTER) {
        if (!device_in) { rts_set_error("%s: null device_in with RTS_BEAM_FROM_POINTER", who); return RTS_ERR_INVALID; }
        *src = (const double*)device_in; *rows = n_rows_in;
    }
    if ((uintptr_t)*src & 15u) { rts_set_error("%s: %s is not 16-byte aligned", who, source == RTS_BEAM_FROM_POINTER ? "device_in" : "the source's device memory"); return RTS_ERR_INVALID; }
    return RTS_OK;
}
// the caller's output against each receiver's span of that source (cells cell0 .. cell1 of its rx_stride); fmt: the entry point's sentence,
// which takes who and the receiver (some add ": the transform is not in place")
static inline int rts_output_apart_check(const char* who, const char* fmt, const void* device_out, size_t out_doubles, const double* src, uint64_t rx_stride, uint64_t cell0, uint64_t cell1, uint32_t n_rx)
{
    uint32_t r = 0;
    if (device_out && rts_rx_spans_overlap(device_out, sizeof(double) * out_doubles, src, rx_stride, cell0, cell1, n_rx, &r)) { rts_set_error(fmt, who, r); return RTS_ERR_INVALID; }
    return RTS_OK;
}

// ------------------------------------------------------------------------------------- a matrix a call reads: the caller's device pointer, or the library-owned product of order own_n
// The entry point's three sentences: misaligned and none take who, other_n takes who, the record's order and the product's
static inline int rts_pointer_or_owned(const char* who, const void* device_ptr, const RtsCubeProduct& own, uint32_t own_n, const char* misaligned, const char* none, const char* other_n,
                                       const double** p, uint32_t* n)
{
    *p = (const double*)device_ptr;
    if (*p) {
        if ((uintptr_t)*p & 15u) { rts_set_error(misaligned, who); return RTS_ERR_INVALID; }
    } else {
        if (!own.valid) { rts_set_error(none, who); return RTS_ERR_INVALID; }
        if (*n != 0 && *n != own_n) { rts_set_error(other_n, who, *n, own_n); return RTS_ERR_INVALID; }
        *p = own.p; *n = own_n;
    }
    return RTS_OK;
}
// The same question for the map of a device detector or a track-before-detect step: the caller's (n_doppler rows, 16-byte aligned) or
// the handle's last Doppler map, caller-owned or not.  Beside the resolver and not through it: a caller map's row count is checked before its alignment
static inline int rts_cfar_map(RtsContext* c, const char* who, const void* device_map, const double** map, uint32_t* n_doppler)
{
    *map = (const double*)device_map;
    if (*map) {
        if (*n_doppler == 0) { rts_set_error("%s: n_doppler = 0 with a caller map", who); return RTS_ERR_INVALID; }
        if ((uintptr_t)*map & 15u) { rts_set_error("%s: device_map is not 16-byte aligned", who); return RTS_ERR_INVALID; }
    } else {
        if (!c->cube.doppler.map.valid) { rts_set_error("%s: no map (call rts_cube_doppler first, or pass device_map)", who); return RTS_ERR_INVALID; }
        *map = c->cube.doppler.map.p; *n_doppler = c->cube.doppler.n_fft;
    }
    return RTS_OK;
}

// ------------------------------------------------------------------------------------- what comes home
// `doubles` doubles at src -> the host, once the stream has produced them; have: they exist (the cube, or a valid product: its RECORDED place and size); none: the message when not
static inline int rts_cube_copy_out(RtsContext* c, const char* who, const char* none, bool have, const double* src, size_t doubles, double* host_out, uint64_t capacity_doubles)
{
    if (!c->cube.set || !have || !host_out) { rts_set_error("%s: %s", who, none); return RTS_ERR_INVALID; }
    if (capacity_doubles < doubles) { rts_set_error("%s: capacity too small", who); return RTS_ERR_CAPACITY; }
    RTS_HIP(hipStreamSynchronize(c->stream));
    RTS_HIP(hipMemcpy(host_out, src, sizeof(double) * doubles, hipMemcpyDeviceToHost));
    return RTS_OK;
}
static inline int rts_cube_copy_out(RtsContext* c, const char* who, const char* none, const RtsCubeProduct& m, double* host_out, uint64_t capacity_doubles)
{
    return rts_cube_copy_out(c, who, none, m.valid, m.p, m.doubles, host_out, capacity_doubles);
}

// the word a solve left behind its library-owned output (0: it succeeded), once the stream has run it
static inline int rts_status_word(RtsContext* c, const uint32_t* d_status, uint32_t* status)
{
    RTS_HIP(hipStreamSynchronize(c->stream));
    RTS_HIP(hipMemcpy(status, d_status, sizeof(uint32_t), hipMemcpyDeviceToHost));
    return RTS_OK;
}

// A counted list -> the host, once the stream has produced it: the total sits behind the scan at d_total, `max` records of
// record_bytes each are stored at d_list, and the first n = min(total, max, capacity) are copied (out may be null when capacity is 0)
static inline int rts_list_copy_out(RtsContext* c, const uint32_t* d_total, uint32_t max, const void* d_list, size_t record_bytes, void* out, uint32_t capacity, uint32_t* total, uint32_t* n)
{
    RTS_HIP(hipStreamSynchronize(c->stream));
    RTS_HIP(hipMemcpy(total, d_total, sizeof(uint32_t), hipMemcpyDeviceToHost));
    *n = rts_list_copied(*total, max, capacity);
    if (*n) RTS_HIP(hipMemcpy(out, d_list, record_bytes * *n, hipMemcpyDeviceToHost));
    return RTS_OK;
}
// ... and a list that did not fit: fmt, the entry point's sentence, takes who, n, total and the two limits, or the capacity alone
static inline int rts_list_fits_check(const char* who, const char* fmt, uint32_t n, uint32_t total, uint32_t max, uint32_t capacity)
{
    if (n >= total) return RTS_OK;
    rts_set_error(fmt, who, n, total, max, capacity);
    return RTS_ERR_CAPACITY;
}
static inline int rts_list_fits_check(const char* who, const char* fmt, uint32_t n, uint32_t total, uint32_t capacity)
{
    if (n >= total) return RTS_OK;
    rts_set_error(fmt, who, n, total, capacity);
    return RTS_ERR_CAPACITY;
}
