// rts_passive.h -- passive radar (include/rts_amd.h: RtsCancelParams, RtsXcorrParams): the lagged read of the reference channel, the
// terms and the partition of the Gram matrix and the cross vectors of batch ECA, the loading, the failed-block rule, the order of the
// subtraction, the tree of the reference cross-correlation, the parameter rules, the host-only plans of the launches and the two host
// evaluators, shared by the kernels (rts_passive.hip) and rts_cancel_eval / rts_xcorr_eval.  The factor, the substitutions and the
// pivot rule are rts_adapt.h's.  Fixed trees of IEEE basic operations and sqrt, compiled with -ffp-contract=off.  Includes nothing
// of HIP: it compiles with any host compiler and is tested without a GPU (tests/test_passive_host.py, tests/passive/passive_main.cpp).
//
// WHY BLOCKS.  Cancellation fits, per block of rows, one coefficient per lag to everything the reference explains in the surveillance
// rows.  An echo at lag k < K whose Doppler turns its phase by much less than one cycle over the block looks like a constant
// coefficient and is removed with the clutter; one that turns by a cycle or more averages out of b and stays.  So the filter is a
// notch of about one cycle per block duration around zero Doppler, over the lags 0 .. K - 1 only: rows_per_block chooses its width
// (short blocks: a wide notch that also follows clutter that drifts; the whole span: the narrowest one), and a target survives when
// its lag is at or beyond K or its Doppler is several cycles per block.
#pragma once
#include <math.h>
#include <stdint.h>
#include <stddef.h>
#include "../../include/rts_amd.h"
#include "rts_adapt.h"
#include "rts_cube_args.h"

// ---- the lagged read: x_k[n] = ref[n - k] of one row of interleaved samples, +0.0 for n < k (the render dropped what left the row)
RTS_HD void rts_passive_lag(const double* row, uint32_t n, uint32_t k, double* xr, double* xi)
{
    if (n < k) { *xr = 0.0; *xi = 0.0; } else { *xr = row[2 * (size_t)(n - k)]; *xi = row[2 * (size_t)(n - k) + 1]; }
}
// The terms are rts_adapt.h's a conj(b): G[i][j] += conj(x_i) x_j is rts_adapt_add(a = x_j, b = x_i), b_r[i] += conj(x_i) y is
// rts_adapt_add(a = y, b = x_i), z[l] += y[n + l] conj(ref[n]) is rts_adapt_add(a = y, b = ref).  A term whose lagged read is the
// zero above is formed and added like any other (the sums' tree does not depend on the lag).
// The subtraction's step y - c x is rts_adapt_sub_mul(l = c, u = x), k ascending.

// the receivers a call cancels: the mask, or with 0 every receiver but the reference
RTS_HD uint64_t rts_passive_mask(uint64_t rx_mask, uint32_t ref_rx, uint32_t n_rx)
{
    if (rx_mask) return rx_mask;
    const uint64_t all = n_rx >= 64u ? ~0ull : ((1ull << n_rx) - 1ull);
    return all & ~(1ull << ref_rx);
}
// the index of the lower triangle's entry (i, j <= i), row-major
RTS_HD uint32_t rts_passive_tri(uint32_t i, uint32_t j) { return i * (i + 1u) / 2u + j; }

// ---- the parameter rules.  Each returns 0, or the number of the rule that broke (rts_cube_api.hip words the messages)
// cancellation: 1 reserved fields; 2 n_rx above RTS_PASSIVE_MAX_RX; 3 ref_rx outside the cube; 4 n_taps outside 1 .. RTS_PASSIVE_MAX_TAPS;
// 5 the span: at least one pulse, inside the cube; 6 loading negative or not finite; 7 rx_mask names ref_rx; 8 rx_mask names a
// receiver the cube does not have; 9 more than RTS_PASSIVE_MAX_BLOCKS blocks
static inline int rts_cancel_rule(const RtsCancelParams* p, uint32_t n_rx, uint32_t n_pulses)
{
    if (p->reserved0 || p->reserved[0] || p->reserved[1]) return 1;
    if (n_rx > RTS_PASSIVE_MAX_RX) return 2;
    if (p->ref_rx >= n_rx) return 3;
    if (p->n_taps == 0u || p->n_taps > RTS_PASSIVE_MAX_TAPS) return 4;
    if (!rts_span_inside(p->first_pulse, p->n_pulses, n_pulses, false, true)) return 5;
    if (!(p->loading >= 0.0) || !(p->loading <= 1.7976931348623157e308)) return 6;
    if (p->rx_mask & (1ull << p->ref_rx)) return 7;
    if (n_rx < 64u && (p->rx_mask >> n_rx)) return 8;
    const uint32_t R = p->rows_per_block == 0u || p->rows_per_block > p->n_pulses ? p->n_pulses : p->rows_per_block;
    if ((p->n_pulses + R - 1u) / R > RTS_PASSIVE_MAX_BLOCKS) return 9;
    return 0;
}
// correlation: 1 reserved fields; 2 ref_rx outside the cube; 3 the span: at least one pulse, inside the cube; 4 n_lags outside
// 1 .. RTS_XCORR_MAX_LAGS; 5 first_lag above RTS_XCORR_MAX_FIRST_LAG; 6 n_bins above RTS_COMPRESS_MAX_BINS; 7 more than 65535 receivers or
// span rows (the launch grid)
static inline int rts_xcorr_rule(const RtsXcorrParams* p, uint32_t n_rx, uint32_t n_pulses, uint32_t n_bins)
{
    if (p->reserved0 || p->reserved[0] || p->reserved[1]) return 1;
    if (p->ref_rx >= n_rx) return 2;
    if (!rts_span_inside(p->first_pulse, p->n_pulses, n_pulses, false, true)) return 3;
    if (p->n_lags == 0u || p->n_lags > RTS_XCORR_MAX_LAGS) return 4;
    if (p->first_lag > RTS_XCORR_MAX_FIRST_LAG) return 5;
    if (n_bins > RTS_COMPRESS_MAX_BINS) return 6;
    if (n_rx > 65535u || p->n_pulses > 65535u) return 7;
    return 0;
}

// ---- the plan of the cancellation's launches (host only), from the shape alone.
// The span's rows are cut into n_blocks blocks of R rows (the last one shorter).  A row is cut into tpr = ceil(n_bins /
// RTS_PASSIVE_TILE) tiles of consecutive bins; the tiles of a block are numbered row-major (row, then tile of the row) and cut into
// parts as rts_adapt.h cuts the covariance's: a block of `tiles` tiles has parts = min(tiles, ppb), ppb = max(1, RTS_PASSIVE_MAX_PARTS
// / n_blocks), and part q owns the tiles floor(q tiles / parts) .. floor((q + 1) tiles / parts) - 1.  A part's sum runs over its
// cells in ascending order (tile, then bin), the first term the start value; the parts are summed in ascending q, part 0 the start
// value.  The same partition serves every entry of G and of every b_r.
//
// k_passive_gram: one workgroup per (block, part).  A tile of the reference row with its K - 1 bins of history is staged in LDS
// (RTS_PASSIVE_TILE + K - 1 complex128: at most 5 104 bytes) and serves all K (K + 1) / 2 entries: x_i of cell n is element
// n - i of it.  A thread owns one RTS_ADAPT_BLOCK x RTS_ADAPT_BLOCK block of entries (rts_adapt.h's cut of the lower triangle) and
// keeps their running sums in registers across the part's tiles.  The lanes of a wave hold neighbouring blocks of a block row: the
// x_i reads are one address (a broadcast), the x_j reads 32 bytes apart.
// k_passive_cross: one workgroup of RTS_PASSIVE_CROSS_RX waves per (block, part, group of that many cancelled receivers); lane i of
// a wave owns b_r[i].  k_passive_reduce: one thread per (block, entry).  k_passive_solve: one workgroup per block, as k_mvdr: thread
// i owns row i of the factor, then thread r solves receiver r's coefficients.  k_passive_apply: one workgroup per (row, tile,
// cancelled receiver), one thread per bin.
// The scratch of one part, and the reduced record of one block: [K (K + 1) / 2 entries of G | n_rx rows of K entries of b].
#define RTS_PASSIVE_WAVE 64u
#define RTS_PASSIVE_CROSS_RX 4u
#define RTS_PASSIVE_REDUCE_THREADS 256u
#define RTS_PASSIVE_REDUCE_BATCH 16u
#define RTS_PASSIVE_SOLVE_THREADS 64u
struct RtsCancelPlan {
    uint32_t K, n_rx, n_bins, rows, R, n_blocks, tpr, ppb, tri, stride, gram_blocks, gram_threads;
    size_t gram_lds, solve_lds, scratch_doubles, sums_doubles, coeff_doubles;
    bool supported;
};
static inline RtsCancelPlan rts_cancel_plan(uint32_t n_rx, uint32_t n_bins, uint32_t n_rows, uint32_t rows_per_block, uint32_t n_taps)
{
    RtsCancelPlan p;
    p.K = n_taps; p.n_rx = n_rx; p.n_bins = n_bins; p.rows = n_rows;
    p.R = rows_per_block == 0u || rows_per_block > n_rows ? n_rows : rows_per_block;
    p.supported = n_taps >= 1u && n_taps <= RTS_PASSIVE_MAX_TAPS && n_rx >= 1u && n_rx <= RTS_PASSIVE_MAX_RX && n_bins >= 1u && n_rows >= 1u;
    p.n_blocks = p.supported ? (n_rows + p.R - 1u) / p.R : 0u;
    if (p.n_blocks > RTS_PASSIVE_MAX_BLOCKS) p.supported = false;
    p.tpr = (uint32_t)(((uint64_t)n_bins + RTS_PASSIVE_TILE - 1u) / RTS_PASSIVE_TILE);
    p.ppb = !p.supported ? 0u : RTS_PASSIVE_MAX_PARTS / p.n_blocks ? RTS_PASSIVE_MAX_PARTS / p.n_blocks : 1u;
    p.tri = n_taps * (n_taps + 1u) / 2u;
    p.stride = p.tri + n_rx * n_taps;
    const uint32_t block_rows = (n_taps + RTS_ADAPT_BLOCK - 1u) / RTS_ADAPT_BLOCK;
    p.gram_blocks = block_rows * (block_rows + 1u) / 2u;
    p.gram_threads = (p.gram_blocks + RTS_PASSIVE_WAVE - 1u) / RTS_PASSIVE_WAVE * RTS_PASSIVE_WAVE;
    p.gram_lds = 16u * ((size_t)RTS_PASSIVE_TILE + n_taps - 1u);
    p.solve_lds = 16u * (size_t)n_taps * n_taps + 16u * (size_t)n_taps * RTS_PASSIVE_SOLVE_THREADS;
    p.scratch_doubles = 2u * (size_t)p.n_blocks * p.ppb * p.stride;
    p.sums_doubles = 2u * (size_t)p.n_blocks * p.stride;
    p.coeff_doubles = 2u * (size_t)n_rx * p.n_blocks * n_taps;
    return p;
}
// block b: its first row inside the span, its rows, its tiles and parts
RTS_HD uint32_t rts_cancel_block_rows(uint32_t rows, uint32_t R, uint32_t b) { const uint32_t r0 = b * R; return rows - r0 < R ? rows - r0 : R; }
RTS_HD uint32_t rts_cancel_block_parts(uint64_t tiles, uint32_t ppb) { return tiles < ppb ? (uint32_t)tiles : ppb; }

// ---- the plan of the correlation's launch (host only).  k_passive_xcorr: one workgroup of RTS_XCORR_THREADS per (group of that many
// lags, row, receiver), one thread per lag; the sum runs over n = 0 .. n_bins - 1 - l ascending, the first term the start value, an empty
// sum is (+0.0, +0.0).  The surveillance row passes through LDS in windows of RTS_XCORR_WINDOW + RTS_XCORR_THREADS samples (8 192
// bytes: many workgroups per CU), so neither n_bins nor n_lags is bounded by LDS; the window does not touch the tree.
#define RTS_XCORR_THREADS 256u
#define RTS_XCORR_WINDOW 256u
struct RtsXcorrPlan { uint32_t lag_groups; size_t lds, out_doubles; bool supported; };
static inline RtsXcorrPlan rts_xcorr_plan(uint32_t n_rx, uint32_t n_rows, uint32_t n_lags)
{
    RtsXcorrPlan p;
    p.supported = n_rx >= 1u && n_rx <= 65535u && n_rows >= 1u && n_rows <= 65535u && n_lags >= 1u && n_lags <= RTS_XCORR_MAX_LAGS;
    p.lag_groups = (n_lags + RTS_XCORR_THREADS - 1u) / RTS_XCORR_THREADS;
    p.lds = 16u * ((size_t)RTS_XCORR_WINDOW + RTS_XCORR_THREADS);
    p.out_doubles = 2u * (size_t)n_rx * n_rows * n_lags;
    return p;
}
// one output: y, ref: one row each of n_bins interleaved samples
RTS_HD void rts_xcorr_cell(const double* y, const double* ref, uint32_t n_bins, uint32_t l, double* zr, double* zi)
{
    double sr = 0.0, si = 0.0;
    if (l < n_bins) for (uint32_t n = 0; n < n_bins - l; n++) rts_adapt_add(n == 0u, y[2 * (size_t)(n + l)], y[2 * (size_t)(n + l) + 1], ref[2 * (size_t)n], ref[2 * (size_t)n + 1], &sr, &si);
    *zr = sr; *zi = si;
}

// ---- the evaluators (validated by the caller)
// one entry's sum over block b: other null: G's (i, j) of the reference rows; else b_r[i] with `other` the receiver's row 0 of the span
static inline void rts_cancel_sum_host(const RtsCancelPlan& plan, const double* ref, const double* other, uint32_t b, uint32_t i, uint32_t j, double* outr, double* outi)
{
    const uint32_t rb = rts_cancel_block_rows(plan.rows, plan.R, b);
    const uint64_t tiles = (uint64_t)rb * plan.tpr;
    const uint32_t parts = rts_cancel_block_parts(tiles, plan.ppb);
    double sr = 0.0, si = 0.0;
    for (uint32_t q = 0; q < parts; q++) {
        const uint64_t t0 = rts_cov_part_begin(tiles, parts, q), t1 = rts_cov_part_begin(tiles, parts, q + 1u);
        double pr = 0.0, pi = 0.0;
        for (uint64_t t = t0; t < t1; t++) {
            const size_t row = (size_t)b * plan.R + (size_t)(t / plan.tpr);
            const uint32_t n0 = (uint32_t)(t % plan.tpr) * RTS_PASSIVE_TILE, n1 = plan.n_bins - n0 < RTS_PASSIVE_TILE ? plan.n_bins : n0 + RTS_PASSIVE_TILE;
            const double* x = ref + 2 * row * plan.n_bins;
            for (uint32_t n = n0; n < n1; n++) {
                double ar, ai, br, bi;
                rts_passive_lag(x, n, i, &br, &bi);
                if (other) { ar = other[2 * (row * plan.n_bins + n)]; ai = other[2 * (row * plan.n_bins + n) + 1]; } else rts_passive_lag(x, n, j, &ar, &ai);
                rts_adapt_add(t == t0 && n == n0, ar, ai, br, bi, &pr, &pi);
            }
        }
        if (q == 0u) { sr = pr; si = pi; } else { sr += pr; si += pi; }
    }
    *outr = sr; *outi = si;
}
// doubles of work the evaluator needs
static inline size_t rts_cancel_work_doubles(uint32_t K) { return 2u * ((size_t)K * K + 2u * (size_t)K); }
// cube [n_rx][n_pulses][n_bins] interleaved, in place; coeffs [n_rx][n_blocks][K] interleaved (may be null); *n_failed: the failed blocks
static inline void rts_cancel_eval_host(const RtsCubeParams* q, double* cube, const RtsCancelParams* p, const RtsCancelPlan& plan, double* coeffs, uint32_t* n_failed, double* work)
{
    const uint32_t K = plan.K;
    const uint64_t mask = rts_passive_mask(p->rx_mask, p->ref_rx, q->n_rx);
    const size_t rx_stride = (size_t)q->n_pulses * q->n_bins;
    double* L = work; double* bv = work + 2 * (size_t)K * K; double* x = bv + 2 * (size_t)K;
    const double* ref = cube + 2 * ((size_t)p->ref_rx * rx_stride + (size_t)p->first_pulse * q->n_bins);
    uint32_t failed = 0u;
    if (coeffs) for (size_t e = 0; e < plan.coeff_doubles; e++) coeffs[e] = 0.0;
    for (uint32_t b = 0; b < plan.n_blocks; b++) {
        for (uint32_t i = 0; i < K; i++) for (uint32_t j = 0; j <= i; j++) {       // A = G + loading I, the lower triangle
            double gr, gi; rts_cancel_sum_host(plan, ref, nullptr, b, i, j, &gr, &gi);
            L[2 * ((size_t)i * K + j)] = i == j ? gr + p->loading : gr; L[2 * ((size_t)i * K + j) + 1] = gi;
        }
        if (rts_chol_factor_host(L, K) >= 0) { failed++; continue; }               // the failed block: unchanged, its coefficients 0
        const uint32_t rb = rts_cancel_block_rows(plan.rows, plan.R, b);
        for (uint32_t r = 0; r < q->n_rx; r++) {
            if (!((mask >> r) & 1ull)) continue;
            double* y = cube + 2 * ((size_t)r * rx_stride + (size_t)p->first_pulse * q->n_bins);
            for (uint32_t i = 0; i < K; i++) rts_cancel_sum_host(plan, ref, y, b, i, 0u, &bv[2 * i], &bv[2 * i + 1]);
            rts_chol_forward(L, K, K, bv, x, 1u);
            rts_chol_back(L, K, K, x, 1u);
            if (coeffs) for (uint32_t k = 0; k < 2u * K; k++) coeffs[2 * (((size_t)r * plan.n_blocks + b) * K) + k] = x[k];
            for (uint32_t row = b * plan.R; row < b * plan.R + rb; row++) {
                const double* xr = ref + 2 * (size_t)row * q->n_bins; double* yr = y + 2 * (size_t)row * q->n_bins;
                for (uint32_t n = 0; n < q->n_bins; n++) {
                    double ar = yr[2 * n], ai = yr[2 * n + 1];
                    for (uint32_t k = 0; k < K; k++) { double ur, ui; rts_passive_lag(xr, n, k, &ur, &ui); rts_adapt_sub_mul(x[2 * k], x[2 * k + 1], ur, ui, &ar, &ai); }
                    yr[2 * n] = ar; yr[2 * n + 1] = ai;
                }
            }
        }
    }
    *n_failed = failed;
}
// cube [n_rx][n_pulses][n_bins] interleaved -> out [n_rx][p->n_pulses][n_lags] interleaved
static inline void rts_xcorr_eval_host(const RtsCubeParams* q, const double* cube, const RtsXcorrParams* p, double* out)
{
    const size_t rx_stride = (size_t)q->n_pulses * q->n_bins;
    for (uint32_t r = 0; r < q->n_rx; r++) for (uint32_t row = 0; row < p->n_pulses; row++) {
        const double* y = cube + 2 * ((size_t)r * rx_stride + (size_t)(p->first_pulse + row) * q->n_bins);
        const double* ref = cube + 2 * ((size_t)p->ref_rx * rx_stride + (size_t)(p->first_pulse + row) * q->n_bins);
        double* z = out + 2 * (((size_t)r * p->n_pulses + row) * p->n_lags);
        for (uint32_t l = 0; l < p->n_lags; l++) rts_xcorr_cell(y, ref, q->n_bins, p->first_lag + l, &z[2 * l], &z[2 * l + 1]);
    }
}
