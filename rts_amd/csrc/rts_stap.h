// rts_stap.h -- space-time adaptive processing (include/rts_amd.h: RtsStCovParams, RtsStApplyParams): the stacked snapshot, the
// covariance and the tap filter over it, the steering product, the host evaluators and the host-only plan of the filter's launch,
// shared by the kernels (rts_adapt.hip: k_cube_cov's stacked form; rts_stap.hip: k_st_apply) and rts_st_covariance_eval /
// rts_st_apply_eval / rts_st_steering_make.  The terms and the partition are rts_adapt.h's and rts_beam.h's: fixed trees of IEEE
// basic operations, compiled with -ffp-contract=off.  Includes nothing of HIP: it compiles with any host compiler and is tested
// without a GPU (tests/test_stap_host.py, tests/stap/stap_main.cpp).
#pragma once
#include "rts_adapt.h"
#include "rts_beam.h"

// ---- the snapshot: x[d] = z[d % N][p + d / N][b], d = m N + rx (tap-major).  The element of x[d] inside a source of rx_stride
// elements per receiver and row_bins bins per row, relative to the element of (receiver 0, row p, bin b)
RTS_HD uint64_t rts_st_offset(uint32_t d, uint32_t n_rx, uint64_t rx_stride, uint32_t row_bins) { return (uint64_t)(d % n_rx) * rx_stride + (uint64_t)(d / n_rx) * row_bins; }

// out = t a = (tr ar - ti ai, tr ai + ti ar): the steering product temporal (x) spatial
RTS_HD void rts_st_steer_mul(double tr, double ti, double ar, double ai, double* o_re, double* o_im)
{
    *o_re = tr * ar - ti * ai; *o_im = tr * ai + ti * ar;
}

// ---- the stacked covariance on the host (validated by the caller): in [n_rx][n_rows_in][row_bins] interleaved -> out [D][D]
// interleaved, D = n_taps n_rx.  s: the training snapshots (s.n_rows START rows: the span's rows less n_taps - 1); plan:
// rts_cov_plan(D, s.n_rows, s.kept).  rts_cov_eval_host's tree with x in place of z
static inline void rts_st_cov_eval_host(uint32_t n_rx, uint32_t n_taps, uint32_t row_bins, const double* in, uint32_t n_rows_in, const RtsCovSet& s, const RtsCovPlan& plan, double* out)
{
    const uint64_t rx_stride = (uint64_t)n_rows_in * row_bins;
    const uint32_t D = n_rx * n_taps;
    const double Kd = (double)plan.K;
    for (uint32_t i = 0; i < D; i++) for (uint32_t j = 0; j <= i; j++) {
        const uint64_t oi = rts_st_offset(i, n_rx, rx_stride, row_bins), oj = rts_st_offset(j, n_rx, rx_stride, row_bins);
        double sr = 0.0, si = 0.0;
        for (uint32_t p = 0; p < plan.parts; p++) {
            const uint64_t c0 = rts_cov_part_begin(plan.tiles, plan.parts, p) * RTS_ADAPT_TILE, c1e = rts_cov_part_begin(plan.tiles, plan.parts, p + 1u) * RTS_ADAPT_TILE;
            const uint64_t c1 = c1e < plan.K ? c1e : plan.K;
            double pr = 0.0, pi = 0.0;
            for (uint64_t c = c0; c < c1; c++) {
                const uint64_t e = rts_cov_cell_index(s, row_bins, c);
                const double* a = in + 2 * (size_t)(oi + e); const double* b = in + 2 * (size_t)(oj + e);
                rts_adapt_add(c == c0, a[0], a[1], b[0], b[1], &pr, &pi);
            }
            if (p == 0u) { sr = pr; si = pi; } else { sr += pr; si += pi; }
        }
        sr = sr / Kd; si = si / Kd;
        if (i == j) { out[2 * ((size_t)i * D + i)] = sr; out[2 * ((size_t)i * D + i) + 1] = 0.0; }
        else { out[2 * ((size_t)i * D + j)] = sr; out[2 * ((size_t)i * D + j) + 1] = si; out[2 * ((size_t)j * D + i)] = sr; out[2 * ((size_t)j * D + i) + 1] = -si; }
    }
}

// ---- the plan of the filter's launch (host only), from the shape alone.  k_st_apply: a thread owns one bin, the RTS_ST_THREADS
// lanes of a workgroup (one wave) consecutive bins; it walks a strip of RTS_ST_STRIP output rows, loading the n_rx samples of input
// row q ONCE (in tiles of RTS_ST_RX_TILE receivers) and adding them into the n_taps outputs p = q - m still in flight, for a tile
// of filters whose running sums stay in registers: n_taps x tile complex128.  The tile shrinks as the taps grow, so that the sums
// fill at most 128 VGPRs (32 complex128) whatever n_taps; a workgroup holds one filter tile's weights [tile][D] in LDS.
// The workgroups: bin groups x strips x filter tiles, in this order in one grid dimension.  The tiles and the strips change which
// sums are in flight together, never the order of a sum: ascending d, the d = 0 term the start value.
#define RTS_ST_THREADS 64u
#define RTS_ST_STRIP 16u
#define RTS_ST_RX_TILE 8u
#define RTS_ST_FILTER_TILE(taps) ((taps) <= 2u ? 16u : (taps) <= 4u ? 8u : (taps) <= 8u ? 4u : 2u)
#define RTS_ST_MAX_GRID_X 2147483647u
struct RtsStApplyPlan { uint32_t D, out_rows, filter_tile, filter_tiles, strips, bin_groups, groups; uint64_t out_cells; size_t lds, out_doubles; bool supported; };
static inline RtsStApplyPlan rts_st_apply_plan(uint32_t n_rx, uint32_t n_taps, uint32_t n_filters, uint32_t n_rows, uint32_t n_bins, uint32_t flags)
{
    RtsStApplyPlan p;
    const bool shape = n_rx >= 1u && n_taps >= 1u && n_taps <= RTS_ST_MAX_TAPS && (uint64_t)n_taps * n_rx <= RTS_BEAM_MAX_RX && n_filters >= 1u &&
                       n_filters <= RTS_BEAM_MAX_BEAMS && (uint64_t)n_filters * n_taps * n_rx <= RTS_BEAM_MAX_WEIGHTS && n_rows >= n_taps && n_bins >= 1u;
    p.D = shape ? n_taps * n_rx : 0u;
    p.out_rows = shape ? n_rows - n_taps + 1u : 0u;
    p.filter_tile = RTS_ST_FILTER_TILE(n_taps);
    p.filter_tiles = (n_filters + p.filter_tile - 1u) / p.filter_tile;
    p.strips = (uint32_t)(((uint64_t)p.out_rows + RTS_ST_STRIP - 1u) / RTS_ST_STRIP);
    p.bin_groups = (uint32_t)(((uint64_t)n_bins + RTS_ST_THREADS - 1u) / RTS_ST_THREADS);
    p.out_cells = (uint64_t)p.out_rows * n_bins;
    const uint64_t per_tile = (uint64_t)p.bin_groups * p.strips;                 // (< 2^26 * 2^27: no overflow; times at most 1024 tiles neither)
    const uint64_t groups = per_tile * p.filter_tiles;
    p.supported = shape && groups >= 1u && groups <= RTS_ST_MAX_GRID_X;
    p.groups = p.supported ? (uint32_t)groups : 0u;
    p.lds = 16u * (size_t)p.filter_tile * p.D;
    p.out_doubles = (size_t)p.out_cells * n_filters * ((flags & RTS_BEAM_POWER) ? 1u : 2u);
    return p;
}

// ---- the filter on the host (validated by the caller): in [n_rx][n_rows_in][n_bins] interleaved, w [n_filters][D] interleaved,
// out [n_filters][n_rows - n_taps + 1][n_bins], complex or power.  Reads only rows first_row .. first_row + n_rows - 1
static inline void rts_st_apply_eval_host(uint32_t n_rx, uint32_t n_taps, uint32_t n_bins, const double* in, uint32_t n_rows_in, uint32_t first_row, uint32_t n_rows,
                                          uint32_t n_filters, const double* w, uint32_t flags, double* out)
{
    const uint32_t D = n_rx * n_taps, out_rows = n_rows - n_taps + 1u;
    const uint64_t rx_stride = (uint64_t)n_rows_in * n_bins;
    const size_t cells = (size_t)out_rows * n_bins, first = (size_t)first_row * n_bins;
    for (uint32_t f = 0; f < n_filters; f++) for (size_t c = 0; c < cells; c++) {
        double yr = 0.0, yi = 0.0;
        for (uint32_t d = 0; d < D; d++) {
            const double* z = in + 2 * ((size_t)rts_st_offset(d, n_rx, rx_stride, n_bins) + first + c);
            rts_beam_add(d == 0u, w[2 * ((size_t)f * D + d)], w[2 * ((size_t)f * D + d) + 1], z[0], z[1], &yr, &yi);
        }
        if (flags & RTS_BEAM_POWER) out[(size_t)f * cells + c] = rts_beam_power(yr, yi);
        else { out[2 * ((size_t)f * cells + c)] = yr; out[2 * ((size_t)f * cells + c) + 1] = yi; }
    }
}
