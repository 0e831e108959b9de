// rts_adapt.h -- adaptive (MVDR) beamforming (include/rts_amd.h: RtsCovParams, RtsMvdrParams): the term and the partition of the
// sample covariance, the Cholesky factor and the two substitutions of the weight solve, the host evaluators and the host-only plans
// of the launches, shared by the kernels (rts_adapt.hip: k_cube_cov, k_cube_cov_reduce, k_mvdr) and rts_covariance_eval /
// rts_mvdr_eval.  Fixed trees of IEEE basic operations and sqrt, compiled with -ffp-contract=off.  Includes nothing of HIP: it
// compiles with any host compiler and is tested without a GPU (tests/test_adapt_host.py, tests/adapt/adapt_main.cpp).
#pragma once
#include <math.h>
#include <stdint.h>
#include <stddef.h>
#include "../../include/rts_amd.h"

#ifndef RTS_HD
#define RTS_HD static inline          // (a host compiler; the library's units have rts_device_math.h's __host__ __device__ form)
#endif

// a conj(b) = (ar br + ai bi, ai br - ar bi): four multiplies, one add, one subtract.  The covariance's term (a = z_i, b = z_j) and
// the factor's L_ik conj(L_jk)
RTS_HD void rts_adapt_term(double ar, double ai, double br, double bi, double* tr, double* ti)
{
    *tr = ar * br + ai * bi; *ti = ai * br - ar * bi;
}
// the running sum of a part plus the term of its next cell; first: the term is the start value
RTS_HD void rts_adapt_add(bool first, double ar, double ai, double br, double bi, double* sr, double* si)
{
    double tr, ti; rts_adapt_term(ar, ai, br, bi, &tr, &ti);
    if (first) { *sr = tr; *si = ti; } else { *sr += tr; *si += ti; }
}
RTS_HD double rts_adapt_abs2(double re, double im) { return re * re + im * im; }
// x - l u = x - (lr ur - li ui, lr ui + li ur): the forward substitution's step
RTS_HD void rts_adapt_sub_mul(double lr, double li, double ur, double ui, double* xr, double* xi)
{
    *xr -= lr * ur - li * ui; *xi -= lr * ui + li * ur;
}
// x - conj(l) v = x - (lr vr + li vi, lr vi - li vr): the back substitution's step
RTS_HD void rts_adapt_sub_conj_mul(double lr, double li, double vr, double vi, double* xr, double* xi)
{
    *xr -= lr * vr + li * vi; *xi -= lr * vi - li * vr;
}
// x - a conj(b): the factor's step
RTS_HD void rts_adapt_sub_term(double ar, double ai, double br, double bi, double* xr, double* xi)
{
    double tr, ti; rts_adapt_term(ar, ai, br, bi, &tr, &ti);
    *xr -= tr; *xi -= ti;
}
// a pivot the factor goes on with: finite and > 0 (comparisons only, the same on host and device)
RTS_HD bool rts_adapt_pivot_ok(double d) { return d > 0.0 && d <= 1.7976931348623157e308; }

// ---- the training set: rows first_row .. + n_rows of every receiver, of each row the bins first_bin .. + n_bins without `skip_n`
// bins from the span's bin `skip_at` on.  kept = n_bins - skip_n bins per row; cell c is (row c / kept, kept bin c % kept)
struct RtsCovSet { uint32_t first_row, n_rows, first_bin, kept, skip_at, skip_n; };
RTS_HD uint32_t rts_cov_bin(const RtsCovSet& s, uint32_t k) { return s.first_bin + k + (k >= s.skip_at ? s.skip_n : 0u); }
// the cell's element index inside one receiver of a source of row_bins bins per row
RTS_HD uint64_t rts_cov_cell_index(const RtsCovSet& s, uint32_t row_bins, uint64_t c)
{
    const uint64_t row = c / s.kept; const uint32_t k = (uint32_t)(c - row * s.kept);
    return (s.first_row + row) * row_bins + rts_cov_bin(s, k);
}
// the tiles of part p: [first, end)
RTS_HD uint64_t rts_cov_part_begin(uint64_t tiles, uint32_t parts, uint32_t p) { return (uint64_t)p * tiles / parts; }

// ---- the plan of the covariance's launches (host only), from the shape alone.  k_cube_cov: one workgroup per part; a tile of
// RTS_ADAPT_TILE cells is staged in LDS as [rx][cell] complex128.  The lower triangle is cut into RTS_ADAPT_BLOCK x RTS_ADAPT_BLOCK
// blocks of entries, one thread per block (blocks on the diagonal form their upper entries too and store none of them).  The lanes
// of a wave hold neighbouring blocks of a block row: at one time they read the same cell of every RTS_ADAPT_BLOCK-th receiver.
// So the receivers' LDS rows are ordered by (rx % RTS_ADAPT_BLOCK, rx / RTS_ADAPT_BLOCK) and each row is padded by one element:
// those reads lie 16 bytes apart modulo the 256-byte bank row, no conflict; lanes that share a receiver read one address, a
// broadcast.  A workgroup holds the blocks rounded up to whole waves and at least one wave per RTS_ADAPT_STAGE receivers: a thread
// stages one cell of at most RTS_ADAPT_STAGE receivers per tile, which it loads into registers while the previous tile is summed.
// Whole waves are a multiple of the tile: in the staging a thread's cell never changes.  k_cube_cov_reduce: one thread per entry of
// the lower triangle.
#define RTS_ADAPT_BLOCK 2u
#define RTS_ADAPT_WAVE 64u
#define RTS_ADAPT_STAGE 8u
#define RTS_ADAPT_MAX_THREADS 576u      // 32 block rows at 64 receivers: 528 blocks, nine waves
#define RTS_ADAPT_REDUCE_THREADS 256u
#define RTS_ADAPT_REDUCE_BATCH 16u
#define RTS_ADAPT_MAX_TILES 4294967295ull
struct RtsCovPlan { uint64_t K, tiles; uint32_t parts, block_rows, blocks, threads, reduce_groups; size_t lds, scratch_bytes, out_doubles; bool supported; };
static inline RtsCovPlan rts_cov_plan(uint32_t n_rx, uint32_t n_rows, uint32_t kept)
{
    RtsCovPlan p;
    p.K = (uint64_t)n_rows * kept;
    p.tiles = (p.K + RTS_ADAPT_TILE - 1u) / RTS_ADAPT_TILE;
    p.supported = n_rx >= 1u && n_rx <= RTS_BEAM_MAX_RX && p.K >= 1u && p.tiles <= RTS_ADAPT_MAX_TILES;
    p.parts = !p.supported ? 0u : p.tiles < RTS_ADAPT_MAX_PARTS ? (uint32_t)p.tiles : RTS_ADAPT_MAX_PARTS;
    p.block_rows = (n_rx + RTS_ADAPT_BLOCK - 1u) / RTS_ADAPT_BLOCK;
    p.blocks = p.block_rows * (p.block_rows + 1u) / 2u;
    p.threads = (p.blocks + RTS_ADAPT_WAVE - 1u) / RTS_ADAPT_WAVE * RTS_ADAPT_WAVE;
    const uint32_t staging = (n_rx + RTS_ADAPT_STAGE - 1u) / RTS_ADAPT_STAGE * RTS_ADAPT_WAVE;
    if (p.threads < staging) p.threads = staging;
    p.reduce_groups = (n_rx * n_rx + RTS_ADAPT_REDUCE_THREADS - 1u) / RTS_ADAPT_REDUCE_THREADS;
    p.lds = 16u * (size_t)n_rx * (RTS_ADAPT_TILE + 1u);
    p.scratch_bytes = 16u * (size_t)p.parts * n_rx * n_rx;
    p.out_doubles = 2u * (size_t)n_rx * n_rx;
    return p;
}
static_assert(RTS_ADAPT_WAVE % RTS_ADAPT_TILE == 0u, "a workgroup of whole waves is a multiple of the tile");
// the LDS row of receiver r among n_rx
RTS_HD uint32_t rts_cov_lds_row(uint32_t r, uint32_t n_rx) { return (r % RTS_ADAPT_BLOCK) * ((n_rx + RTS_ADAPT_BLOCK - 1u) / RTS_ADAPT_BLOCK) + r / RTS_ADAPT_BLOCK; }
// block b of the lower triangle, row-major: (bi, bj <= bi) with b = bi (bi + 1) / 2 + bj.  Integers only (no square root): at most
// 32 steps
RTS_HD void rts_cov_block(uint32_t b, uint32_t* bi, uint32_t* bj)
{
    uint32_t i = 0u; while ((i + 1u) * (i + 2u) / 2u <= b) i++;
    *bi = i; *bj = b - i * (i + 1u) / 2u;
}

// ---- the plan of the solve (host only).  k_mvdr: ONE workgroup of RTS_MVDR_THREADS; A / L [n_rx][n_rx] in LDS and behind it the
// substitutions' vectors [n_rx][RTS_MVDR_THREADS] (a thread's own column: consecutive lanes 16 bytes apart).  Thread i owns row i of
// the factor; the beams are solved one per thread, in passes.
#define RTS_MVDR_THREADS 64u
struct RtsMvdrPlan { uint32_t passes; size_t lds, out_doubles; bool supported; };
static inline RtsMvdrPlan rts_mvdr_plan(uint32_t n_rx, uint32_t n_beams)
{
    RtsMvdrPlan p;
    p.supported = n_rx >= 1u && n_rx <= RTS_BEAM_MAX_RX && n_rx <= RTS_MVDR_THREADS && n_beams >= 1u && n_beams <= RTS_BEAM_MAX_BEAMS &&
                  (uint64_t)n_beams * n_rx <= RTS_BEAM_MAX_WEIGHTS;
    p.passes = (n_beams + RTS_MVDR_THREADS - 1u) / RTS_MVDR_THREADS;
    p.lds = 16u * (size_t)n_rx * n_rx + 16u * (size_t)n_rx * RTS_MVDR_THREADS;
    p.out_doubles = 2u * (size_t)n_beams * n_rx;
    return p;
}

// ---- the solve's pieces, on a factor L [n][n] interleaved with row stride ld elements (the kernel: LDS; the evaluator: a vector)
// the pivot of column j: A_jj less the squares of row j's factor entries left of it
RTS_HD double rts_mvdr_pivot(const double* L, uint32_t ld, uint32_t j)
{
    double d = L[2 * ((size_t)j * ld + j)];
    for (uint32_t k = 0; k < j; k++) d -= rts_adapt_abs2(L[2 * ((size_t)j * ld + k)], L[2 * ((size_t)j * ld + k) + 1]);
    return d;
}
// L_ij of a row i > j, in place of A_ij; ljj = sqrt(pivot)
RTS_HD void rts_mvdr_below(double* L, uint32_t ld, uint32_t i, uint32_t j, double ljj)
{
    double xr = L[2 * ((size_t)i * ld + j)], xi = L[2 * ((size_t)i * ld + j) + 1];
    for (uint32_t k = 0; k < j; k++)
        rts_adapt_sub_term(L[2 * ((size_t)i * ld + k)], L[2 * ((size_t)i * ld + k) + 1], L[2 * ((size_t)j * ld + k)], L[2 * ((size_t)j * ld + k) + 1], &xr, &xi);
    L[2 * ((size_t)i * ld + j)] = xr / ljj; L[2 * ((size_t)i * ld + j) + 1] = xi / ljj;
}
// the two substitutions on a factor, shared by the beams below and by rts_passive.h's coefficient solve.  x: the work vector [n],
// element k at x[2 k xs], x[2 k xs + 1]
// forward: x = L^-1 s, s [n] interleaved
RTS_HD void rts_chol_forward(const double* L, uint32_t ld, uint32_t n, const double* s, double* x, size_t xs)
{
    for (uint32_t i = 0; i < n; i++) {
        double xr = s[2 * i], xi = s[2 * i + 1];
        for (uint32_t k = 0; k < i; k++) rts_adapt_sub_mul(L[2 * ((size_t)i * ld + k)], L[2 * ((size_t)i * ld + k) + 1], x[2 * k * xs], x[2 * k * xs + 1], &xr, &xi);
        const double lii = L[2 * ((size_t)i * ld + i)];
        x[2 * i * xs] = xr / lii; x[2 * i * xs + 1] = xi / lii;
    }
}
// back: x = L^-H x, in place
RTS_HD void rts_chol_back(const double* L, uint32_t ld, uint32_t n, double* x, size_t xs)
{
    for (uint32_t i = n; i-- > 0u;) {
        double xr = x[2 * i * xs], xi = x[2 * i * xs + 1];
        for (uint32_t k = i + 1u; k < n; k++) rts_adapt_sub_conj_mul(L[2 * ((size_t)k * ld + i)], L[2 * ((size_t)k * ld + i) + 1], x[2 * k * xs], x[2 * k * xs + 1], &xr, &xi);
        const double lii = L[2 * ((size_t)i * ld + i)];
        x[2 * i * xs] = xr / lii; x[2 * i * xs + 1] = xi / lii;
    }
}
// one beam: s [n] interleaved -> w [n] interleaved; x: the beam's work vector
RTS_HD void rts_mvdr_beam(const double* L, uint32_t ld, uint32_t n, const double* s, double* x, size_t xs, double* w)
{
    rts_chol_forward(L, ld, n, s, x, xs);                // u = L^-1 s
    double den = rts_adapt_abs2(x[0], x[1]);
    for (uint32_t k = 1; k < n; k++) den += rts_adapt_abs2(x[2 * k * xs], x[2 * k * xs + 1]);
    rts_chol_back(L, ld, n, x, xs);                      // v = L^-H u
    for (uint32_t i = 0; i < n; i++) { w[2 * i] = x[2 * i * xs] / den; w[2 * i + 1] = x[2 * i * xs + 1] / den; }
}

// ---- the evaluators (validated by the caller)
// the covariance on the host: in [n_rx][n_rows_in][row_bins] interleaved -> out [n_rx][n_rx] interleaved
static inline void rts_cov_eval_host(uint32_t n_rx, uint32_t row_bins, const double* in, uint32_t n_rows_in, const RtsCovSet& s, const RtsCovPlan& plan, double* out)
{
    const size_t rx_stride = (size_t)n_rows_in * row_bins;
    const double Kd = (double)plan.K;
    for (uint32_t i = 0; i < n_rx; i++) for (uint32_t j = 0; j <= i; j++) {
        double sr = 0.0, si = 0.0;
        for (uint32_t p = 0; p < plan.parts; p++) {
            const uint64_t c0 = rts_cov_part_begin(plan.tiles, plan.parts, p) * RTS_ADAPT_TILE, c1e = rts_cov_part_begin(plan.tiles, plan.parts, p + 1u) * RTS_ADAPT_TILE;
            const uint64_t c1 = c1e < plan.K ? c1e : plan.K;
            double pr = 0.0, pi = 0.0;
            for (uint64_t c = c0; c < c1; c++) {
                const uint64_t e = rts_cov_cell_index(s, row_bins, c);
                const double* a = in + 2 * ((size_t)i * rx_stride + e); const double* b = in + 2 * ((size_t)j * rx_stride + e);
                rts_adapt_add(c == c0, a[0], a[1], b[0], b[1], &pr, &pi);
            }
            if (p == 0u) { sr = pr; si = pi; } else { sr += pr; si += pi; }
        }
        sr = sr / Kd; si = si / Kd;
        if (i == j) { out[2 * ((size_t)i * n_rx + i)] = sr; out[2 * ((size_t)i * n_rx + i) + 1] = 0.0; }
        else { out[2 * ((size_t)i * n_rx + j)] = sr; out[2 * ((size_t)i * n_rx + j) + 1] = si; out[2 * ((size_t)j * n_rx + i)] = sr; out[2 * ((size_t)j * n_rx + i) + 1] = -si; }
    }
}
// the column Cholesky of the lower triangle of A [n][n] in place, on the host.  Returns -1, or the column of the pivot that failed
static inline int rts_chol_factor_host(double* L, uint32_t n)
{
    for (uint32_t j = 0; j < n; j++) {
        const double d = rts_mvdr_pivot(L, n, j);
        if (!rts_adapt_pivot_ok(d)) return (int)j;
        const double ljj = sqrt(d);
        L[2 * ((size_t)j * n + j)] = ljj;
        for (uint32_t i = j + 1u; i < n; i++) rts_mvdr_below(L, n, i, j, ljj);
    }
    return -1;
}
// the solve on the host: cov [n][n], steering [n_beams][n] -> out [n_beams][n]; L: 2 n n doubles of work, x: 2 n.  Returns -1, or the
// column of the pivot that failed (out untouched)
static inline int rts_mvdr_eval_host(const double* cov, uint32_t n, uint32_t n_beams, const double* steering, double loading, double* L, double* x, double* out)
{
    for (uint32_t i = 0; i < n; i++) for (uint32_t j = 0; j <= i; j++) {       // A = R + loading I, the lower triangle
        const double re = cov[2 * ((size_t)i * n + j)];
        L[2 * ((size_t)i * n + j)] = i == j ? re + loading : re;
        L[2 * ((size_t)i * n + j) + 1] = i == j ? 0.0 : cov[2 * ((size_t)i * n + j) + 1];       // (the diagonal's imaginary part is never used)
    }
    const int bad = rts_chol_factor_host(L, n);
    if (bad >= 0) return bad;
    for (uint32_t b = 0; b < n_beams; b++) rts_mvdr_beam(L, n, n, steering + 2 * (size_t)b * n, x, 1u, out + 2 * (size_t)b * n);
    return -1;
}
