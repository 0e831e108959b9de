// rts_tbd.h -- the rules of track-before-detect by dynamic programming (include/rts_amd.h: RtsTbdParams, RtsTbdExtractParams,
// RtsTbdTrack), each written once and called by the kernels (rts_tbd.hip), the entry points (rts_cube_detect_api.hip) and the host
// evaluators (rts_tbd_step_eval, rts_tbd_extract_eval): the Doppler wrap and the shift table, the score, the window's first maximum
// and its code, the candidate rule, the walk back through the pointer maps, the record, the validation, and the evaluators
// themselves.  Every expression is written in the operand order of the header text and the units are built without contraction, so
// kernel and evaluator agree bit for bit.  Includes nothing of HIP: it compiles with any host compiler and is tested without a GPU
// (tests/test_tbd_host.py, tests/tbd/tbd_main.cpp).
#pragma once
#include <math.h>
#include <stdint.h>
#include <stddef.h>
#include "../../include/rts_amd.h"
#include "rts_cfar.h"             // RTS_HD, rts_cfar_local_max

#define RTS_TBD_TILE 1024u                    // range bins a workgroup of k_tbd_step takes (tests/test_gpu_tbd.py sizes its edge cases by it)
#define RTS_TBD_MAX_SHIFT 1073741824.0        // 2^30: a shift quotient beyond it is refused

RTS_HD bool rts_tbd_finite(double x) { return x - x == 0.0; }
RTS_HD uint32_t rts_tbd_codes(uint32_t Hd, uint32_t Hr) { return (2u * Hd + 1u) * (2u * Hr + 1u); }
RTS_HD uint32_t rts_tbd_max_tracks(const RtsTbdExtractParams& e) { return e.max_tracks ? e.max_tracks : RTS_TBD_MAX_TRACKS; }

// Doppler bin kd of nd as a signed bin in [-nd / 2, nd / 2), the way rts_cfar_record wraps it; the bin in hertz (0 without a pri)
RTS_HD double rts_tbd_bin(uint32_t kd, uint32_t nd)
{
    double w = (double)kd;
    if (w >= 0.5 * (double)nd) w -= (double)nd;
    return w;
}
RTS_HD double rts_tbd_hz(uint32_t kd, uint32_t nd, double pri) { return pri > 0.0 ? rts_tbd_bin(kd, nd) / ((double)nd * pri) : 0.0; }
// the shift of row kd: the quotient, whether a table may hold it, its entry
RTS_HD double rts_tbd_shift_quotient(uint32_t kd, uint32_t nd, double k, double pri, double T, double dt) { return ((k * rts_tbd_hz(kd, nd, pri)) * T) / dt; }
RTS_HD bool rts_tbd_shift_ok(double q) { return rts_tbd_finite(q) && q >= -RTS_TBD_MAX_SHIFT && q <= RTS_TBD_MAX_SHIFT; }
RTS_HD int32_t rts_tbd_shift(double q) { return (int32_t)rint(q); }

RTS_HD double rts_tbd_score(double re, double im, uint32_t mode, double scale)
{
    const double P = re * re + im * im;
    double x = P * scale;
    if (mode == RTS_TBD_AMPLITUDE) x = sqrt(x);
    return rts_tbd_finite(x) ? x : 0.0;
}

// The window's first maximum: at(dd, dr) is the previous merit at (wrap(kd + dd), r - s[kd] + dr), or 0 where that range index does
// not exist (0 never replaces the best, so this is "skipped").  Row by row in ascending dd, within a row in ascending dr, strictly
// greater replaces: the first maximum in ascending (dd, dr).
template <class At> RTS_HD void rts_tbd_best(int Hd, int Hr, At at, double* best, uint32_t* code)
{
    double b = 0.0; uint32_t c = RTS_TBD_NONE;
    for (int dd = -Hd; dd <= Hd; dd++)
        for (int dr = -Hr; dr <= Hr; dr++) {
            const double v = at(dd, dr);
            if (v > b) { b = v; c = (uint32_t)((dd + Hd) * (2 * Hr + 1) + (dr + Hr)); }
        }
    *best = b; *code = c;
}
RTS_HD double rts_tbd_merit(double x, double decay, double best) { return x + decay * best; }
RTS_HD uint32_t rts_tbd_row(uint32_t kd, int dd, uint32_t nd) { return (uint32_t)(((int64_t)kd + dd + (int64_t)nd) % (int64_t)nd); }

// The candidate rule for a cell of merit m; at(dk, dr) reads the merit map (Doppler wrapped by the caller, asked only for range
// neighbours that exist: left, right)
template <class At> RTS_HD bool rts_tbd_candidate(double m, double threshold, bool local_max, bool left, bool right, At at)
{
    if (!(m > threshold)) return false;
    return !local_max || rts_cfar_local_max(m, left, right, at);
}

// The walk back from end cell (kd, r): ptr(j, kd, r) is the pointer of the frame j back at that cell, shift(j, kd) its table's
// entry.  Writes the cells visited to path[2 j], path[2 j + 1] (j < max_cells <= depth) and 0xffffffff to the rest of the `depth`
// entries; returns the number of cells and the oldest one.
template <class Ptr, class Shift>
RTS_HD uint32_t rts_tbd_walk(uint32_t nd, uint32_t nb, uint32_t Hd, uint32_t Hr, uint32_t max_cells, uint32_t depth, uint32_t kd, uint32_t r, Ptr ptr, Shift shift,
                             uint32_t* path, uint32_t* first_kd, uint32_t* first_r)
{
    const uint32_t W = 2u * Hr + 1u, codes = rts_tbd_codes(Hd, Hr);
    uint32_t n = 0;
    for (;;) {
        path[2u * n] = kd; path[2u * n + 1u] = r; n++;
        if (n >= max_cells) break;
        const uint32_t c = ptr(n - 1u, kd, r);
        if (c >= codes) break;                                           // NONE (or no code of this window)
        const int dd = (int)(c / W) - (int)Hd, dr = (int)(c % W) - (int)Hr;
        const int64_t rp = ((int64_t)r - (int64_t)shift(n - 1u, kd)) + dr;
        if (rp < 0 || rp >= (int64_t)nb) break;
        kd = rts_tbd_row(kd, dd, nd); r = (uint32_t)rp;
    }
    *first_kd = kd; *first_r = r;
    for (uint32_t j = n; j < depth; j++) { path[2u * j] = 0xffffffffu; path[2u * j + 1u] = 0xffffffffu; }
    return n;
}

RTS_HD RtsTbdTrack rts_tbd_record(uint32_t rx, uint32_t kd, uint32_t r, uint32_t n_cells, uint32_t first_kd, uint32_t first_r, double merit,
                                  uint32_t nd, double t0, double dt, double pri)
{
    RtsTbdTrack o;
    o.rx = rx; o.doppler_bin = kd; o.range_bin = r; o.n_cells = n_cells; o.first_doppler_bin = first_kd; o.first_range_bin = first_r;
    o.merit = merit;
    o.delay = t0 + (double)r * dt;
    o.doppler = rts_tbd_hz(kd, nd, pri);
    return o;
}

// ---- validation.  The step's record on a map of nd x nb cells: 0, or the number of the rule it breaks (rts_cube_detect_api.hip words the message)
//   1 half_doppler  2 half_range  3 depth  4 score  5 flags  6 reserved  7 scale  8 decay  9 delay_rate_per_hz  10 pri
//   11 2 half_doppler + 1 > n_doppler  12 half_range >= n_bins
RTS_HD int rts_tbd_params_check(const RtsTbdParams* p, uint32_t nd, uint32_t nb)
{
    if (p->half_doppler > RTS_TBD_MAX_HALF_DOPPLER) return 1;
    if (p->half_range > RTS_TBD_MAX_HALF_RANGE) return 2;
    if (p->depth == 0u || p->depth > RTS_TBD_MAX_DEPTH) return 3;
    if (p->score > RTS_TBD_AMPLITUDE) return 4;
    if (p->flags) return 5;
    if (p->reserved0 || p->reserved[0] || p->reserved[1]) return 6;
    if (!rts_tbd_finite(p->scale) || !(p->scale > 0.0)) return 7;
    if (!(p->decay > 0.0) || !(p->decay <= 1.0)) return 8;
    if (!rts_tbd_finite(p->delay_rate_per_hz)) return 9;
    if (!rts_tbd_finite(p->pri) || !(p->pri >= 0.0)) return 10;
    if (2u * p->half_doppler + 1u > nd) return 11;
    if (p->half_range >= nb) return 12;
    return 0;
}
RTS_HD bool rts_tbd_interval_ok(double T) { return rts_tbd_finite(T) && T > 0.0; }
// the whole shift table of a later frame: 0, or 1 with *bad the first row whose quotient no table may hold
RTS_HD int rts_tbd_shifts_check(const RtsTbdParams* p, uint32_t nd, double T, double dt, uint32_t* bad)
{
    for (uint32_t kd = 0; kd < nd; kd++) if (!rts_tbd_shift_ok(rts_tbd_shift_quotient(kd, nd, p->delay_rate_per_hz, p->pri, T, dt))) { *bad = kd; return 1; }
    return 0;
}
// the extraction's record: 0, or  1 threshold  2 pri  3 flags  4 max_tracks  5 reserved
RTS_HD int rts_tbd_extract_check(const RtsTbdExtractParams* e)
{
    if (e->threshold != e->threshold) return 1;
    if (!rts_tbd_finite(e->pri) || !(e->pri >= 0.0)) return 2;
    if (e->flags & ~RTS_TBD_LOCAL_MAX) return 3;
    if (e->max_tracks > RTS_TBD_MAX_TRACKS) return 4;
    if (e->reserved[0] || e->reserved[1]) return 5;
    return 0;
}

// ---- host only from here.  Both on validated input.
// One step: map [n_rx][nd][nb] complex, merit_in (null: the first frame) -> merit_out, ptr_out [cells], shifts_out [nd]
static inline void rts_tbd_step_host(const RtsTbdParams* p, uint32_t n_rx, uint32_t nd, uint32_t nb, double dt, const double* map, const double* merit_in, double T,
                                     double* merit_out, uint8_t* ptr_out, int32_t* shifts_out)
{
    const int Hd = (int)p->half_doppler, Hr = (int)p->half_range;
    for (uint32_t kd = 0; kd < nd; kd++) shifts_out[kd] = merit_in ? rts_tbd_shift(rts_tbd_shift_quotient(kd, nd, p->delay_rate_per_hz, p->pri, T, dt)) : 0;
    for (uint32_t rx = 0; rx < n_rx; rx++)
        for (uint32_t kd = 0; kd < nd; kd++) {
            const size_t row = ((size_t)rx * nd + kd) * nb;
            const int64_t s = shifts_out[kd];
            for (uint32_t r = 0; r < nb; r++) {
                const double x = rts_tbd_score(map[2 * (row + r)], map[2 * (row + r) + 1], p->score, p->scale);
                if (!merit_in) { merit_out[row + r] = x; ptr_out[row + r] = (uint8_t)RTS_TBD_NONE; continue; }
                double best; uint32_t code;
                rts_tbd_best(Hd, Hr, [&](int dd, int dr) {
                    const int64_t rp = ((int64_t)r - s) + dr;
                    return rp < 0 || rp >= (int64_t)nb ? 0.0 : merit_in[((size_t)rx * nd + rts_tbd_row(kd, dd, nd)) * nb + (size_t)rp];
                }, &best, &code);
                merit_out[row + r] = rts_tbd_merit(x, p->decay, best); ptr_out[row + r] = (uint8_t)code;
            }
        }
}

// The extraction: merit, n_frames pointer maps and shift tables OLDEST FIRST.  Writes up to min(capacity, max_tracks) records and
// their paths ([depth][2] each) and returns the total.
static inline uint32_t rts_tbd_extract_host(const RtsTbdParams* p, const RtsTbdExtractParams* e, uint32_t n_rx, uint32_t nd, uint32_t nb, double t0, double dt,
                                            const double* merit, const uint8_t* ptrs, const int32_t* shifts, uint32_t n_frames, RtsTbdTrack* out, uint32_t* paths, uint32_t capacity)
{
    const size_t cells = (size_t)n_rx * nd * nb;
    const bool local_max = (e->flags & RTS_TBD_LOCAL_MAX) != 0u;
    const uint32_t room = capacity < rts_tbd_max_tracks(*e) ? capacity : rts_tbd_max_tracks(*e);
    uint32_t total = 0;
    for (uint32_t rx = 0; rx < n_rx; rx++)
        for (uint32_t kd = 0; kd < nd; kd++)
            for (uint32_t r = 0; r < nb; r++) {
                const double* m = merit + (size_t)rx * nd * nb;
                const double v = m[(size_t)kd * nb + r];
                if (!rts_tbd_candidate(v, e->threshold, local_max, r >= 1u, r + 1u < nb, [&](int dk, int dr) { return m[(size_t)rts_tbd_row(kd, dk, nd) * nb + (size_t)((int64_t)r + dr)]; })) continue;
                if (total < room) {
                    uint32_t fk, fr;
                    uint32_t* path = paths + (size_t)total * p->depth * 2u;
                    const uint32_t n = rts_tbd_walk(nd, nb, p->half_doppler, p->half_range, n_frames < p->depth ? n_frames : p->depth, p->depth, kd, r,
                        [&](uint32_t j, uint32_t k, uint32_t b) { return (uint32_t)ptrs[(size_t)(n_frames - 1u - j) * cells + ((size_t)rx * nd + k) * nb + b]; },
                        [&](uint32_t j, uint32_t k) { return shifts[(size_t)(n_frames - 1u - j) * nd + k]; }, path, &fk, &fr);
                    out[total] = rts_tbd_record(rx, kd, r, n, fk, fr, v, nd, t0, dt, e->pri);
                }
                total++;
            }
    return total;
}
