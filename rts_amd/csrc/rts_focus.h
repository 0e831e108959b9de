// rts_focus.h -- autofocus of the return cube (include/rts_amd.h: RtsAlignParams, RtsPgaParams, RtsCorrectParams): envelope range
// alignment against a global reference, phase-gradient autofocus and the in-place correction -- the arithmetic shared by the
// kernels (rts_focus.hip) and the host evaluators (rts_align_eval, rts_pga_eval, rts_correct_eval), and the host-only plans of the
// launches.  The transform is rts_stft.h's tree, the interpolator and the rotation are rts_image.h's.  Fixed trees of IEEE basic
// operations (alignment: bit-identical on host and device) plus sincospi / atan2 and the twiddles (PGA), compiled with
// -ffp-contract=off.  Includes nothing of HIP: it compiles with any host compiler and is tested without a GPU
// (tests/test_focus_host.py, tests/focus/focus_main.cpp).
#pragma once
#include <math.h>
#include <stdint.h>
#include <stddef.h>
#include "../../include/rts_amd.h"
#include "rts_stft.h"
#include "rts_image.h"

#ifndef RTS_HD
#define RTS_HD static inline          // (a host compiler; the library's units have rts_device_math.h's __host__ __device__ form)
#endif

#define RTS_FOCUS_MAX_RX 65535u              // the launch grid: receivers
#define RTS_FOCUS_MAX_GRID_X 2147483647u     // the launch grid: rows x workgroups per row
#define RTS_FOCUS_THREADS 256u

// ------------------------------------------------------------------------------------------------ range alignment
// the envelope of a sample
RTS_HD double rts_focus_envelope(double re, double im) { return sqrt(re * re + im * im); }
// R = (int64) floor(S + 0.5) of a shift of the table (finite, |S| <= RTS_ALIGN_MAX_LAG + 1/2: rts_align_pick)
RTS_HD int64_t rts_focus_round(double s) { return (int64_t)floor(s + 0.5); }
// env[i] of a row of n_bins envelopes, 0 outside the row
RTS_HD double rts_focus_env_at(const double* env, uint32_t n_bins, int64_t i) { return (i >= 0 && i < (int64_t)n_bins) ? env[i] : 0.0; }

// ref at bin n: sum_j e[j][n + R_j] -- ascending j from 0 inside chunks of RTS_ALIGN_PULSE_CHUNK pulses, the chunk sums added in
// ascending order, the first chunk's sum the start value.  env: [P][n_bins] (one receiver's rows), S: [P]
RTS_HD double rts_align_ref_at(const double* env, const double* S, uint32_t P, uint32_t n_bins, uint32_t n)
{
    double tot = 0.0;
    for (uint32_t j0 = 0; j0 < P; j0 += RTS_ALIGN_PULSE_CHUNK) {
        const uint32_t j1 = P - j0 < RTS_ALIGN_PULSE_CHUNK ? P : j0 + RTS_ALIGN_PULSE_CHUNK;
        double s = 0.0;
        for (uint32_t j = j0; j < j1; j++) s += rts_focus_env_at(env + (size_t)j * n_bins, n_bins, (int64_t)n + rts_focus_round(S[j]));
        if (j0 == 0) tot = s; else tot += s;
    }
    return tot;
}

// one block's sum of C(l): gate bins g0 .. g1 - 1 (ref is indexed by gate bin), each product rounded before it is added, from 0
RTS_HD double rts_align_block(const double* ref, const double* env_row, uint32_t n_bins, uint32_t first_bin, uint32_t g0, uint32_t g1, int32_t l)
{
    double s = 0.0;
    for (uint32_t g = g0; g < g1; g++) {
        const double pr = ref[g] * rts_focus_env_at(env_row, n_bins, (int64_t)first_bin + (int64_t)g + (int64_t)l);
        s += pr;
    }
    return s;
}

// the shift of a row from its correlation C[l + L], l in [-L, L]: l* by the scan 0, -1, +1, ... on a strict >, then the parabola
RTS_HD double rts_align_pick(const double* C, uint32_t L, uint32_t flags)
{
    int32_t best = 0;
    double bv = C[L];
    if (!(bv == bv)) bv = -INFINITY;                                 // (a NaN never wins)
    for (int32_t m = 1; m <= (int32_t)L; m++) {
        const double lo = C[(int32_t)L - m], hi = C[(int32_t)L + m];
        if (lo > bv) { bv = lo; best = -m; }
        if (hi > bv) { bv = hi; best = m; }
    }
    double delta = 0.0;
    const uint32_t ab = (uint32_t)(best < 0 ? -best : best);
    if (!(flags & RTS_ALIGN_INTEGER) && ab < L) {
        const double cm = C[(int32_t)L + best - 1], c0 = C[(int32_t)L + best], cp = C[(int32_t)L + best + 1];
        const double den = cm - 2.0 * c0 + cp;
        if (den < 0.0) {
            double d = 0.5 * (cm - cp) / den;
            if (d < -0.5) d = -0.5; else if (d > 0.5) d = 0.5; else if (!(d == d)) d = 0.0;
            delta = d;
        }
    }
    return (double)best + delta;
}

// ------------------------------------------------------------------------------------------------ phase: rotation, gradient, update
// (cs, sn) = (cos, sin)(2 pi phi) of a phase in cycles: f = phi - floor(phi), sincospi(2 f); a phase without a fraction gives (1, 0)
RTS_HD void rts_focus_rotation(double phi, double* cs, double* sn)
{
    const double f = phi - floor(phi);
    *sn = 0.0; *cs = 1.0;
    if (f >= 0.0 && f < 1.0) rts_image_sincospi(2.0 * f, sn, cs);
}
// v <- v (cs - j sn)
RTS_HD void rts_focus_unrotate(double cs, double sn, double* re, double* im)
{
    const double vr = *re, vi = *im;
    *re = vr * cs + vi * sn; *im = vi * cs - vr * sn;
}
// row k of the shifted spectrum is kept
RTS_HD bool rts_pga_keep(uint32_t k, uint32_t N, uint32_t W) { const uint32_t m = k < N - k ? k : N - k; return m <= W / 2u; }
// a = g conj(h)
RTS_HD void rts_pga_product(double gr, double gi, double hr, double hi, double* ar, double* ai) { *ar = gr * hr + gi * hi; *ai = gi * hr - gr * hi; }
// the phase step of a summed product, in cycles
RTS_HD double rts_pga_delta(double re, double im) { return (re == 0.0 && im == 0.0) ? 0.0 : atan2(im, re) / (2.0 * RTS_PI); }
// psi[N]: in the steps (psi[0] = 0), out the running sum less its mean and its least-squares line; returns the rms of the result
RTS_HD double rts_pga_update(uint32_t N, double* psi)
{
    double run = 0.0, sum = 0.0;
    for (uint32_t p = 0; p < N; p++) { run += psi[p]; psi[p] = run; sum += run; }
    const double mean = sum / (double)N, mid = ((double)N - 1.0) / 2.0;
    double sxy = 0.0, sxx = 0.0;
    for (uint32_t p = 0; p < N; p++) { const double x = (double)p - mid; sxy += x * psi[p]; sxx += x * x; }
    const double slope = sxy / sxx;
    double ss = 0.0;
    for (uint32_t p = 0; p < N; p++) { const double x = (double)p - mid; const double v = psi[p] - mean - slope * x; psi[p] = v; ss += v * v; }
    return sqrt(ss / (double)N);
}
// the window of the next iteration
RTS_HD uint32_t rts_pga_next_window(uint32_t W, uint32_t window_min) { const uint32_t h = W / 2u; return h > window_min ? h : window_min; }

// ------------------------------------------------------------------------------------------------ the plans of the launches (host only)
// Alignment.  The envelope of the rows goes to a scratch [n_rx][P][n_bins] once; per iteration one thread per (receiver, gate
// bin) forms ref, then one workgroup per (receiver, pulse) forms C: its lanes take (block, lag) pairs, lag fastest, pass by pass
// of blocks_per_pass blocks whose sums fit RTS_ALIGN_LDS_SUMS doubles of LDS; lane l adds its lag's block sums left to right.
#define RTS_ALIGN_LDS_SUMS 2048u
struct RtsAlignPlan { uint32_t n_gate, n_lags, n_blocks, blocks_per_pass; size_t env_doubles, ref_doubles, out_doubles; bool supported; };
static inline RtsAlignPlan rts_align_plan(uint32_t n_rx, uint32_t n_pulses, uint32_t n_bins, uint32_t n_gate, uint32_t max_lag)
{
    RtsAlignPlan p;
    p.n_gate = n_gate; p.n_lags = 2u * max_lag + 1u;
    p.n_blocks = (uint32_t)(((uint64_t)n_gate + RTS_ALIGN_BIN_BLOCK - 1u) / RTS_ALIGN_BIN_BLOCK);
    p.blocks_per_pass = RTS_ALIGN_LDS_SUMS / p.n_lags;
    p.env_doubles = (size_t)n_rx * n_pulses * n_bins; p.ref_doubles = (size_t)n_rx * n_gate; p.out_doubles = (size_t)n_rx * n_pulses;
    p.supported = n_rx <= RTS_FOCUS_MAX_RX && n_pulses <= RTS_FOCUS_MAX_GRID_X && max_lag <= RTS_ALIGN_MAX_LAG;      // (the grids: (n_pulses, n_rx) and (ceil(n_gate / 256), n_rx))
    return p;
}

// PGA.  One workgroup per (receiver, tile of RTS_PGA_BIN_TILE gate bins); its LDS holds TWO sets of N x BT complex128 columns (the
// spectrum, and the shifted, masked spectrum in bit-reversed order: the shift is no in-place permutation) and the N / 2 complex
// twiddles.  BT: the most columns, a power of two up to the tile, that fit the 160 KiB a workgroup may allocate: 8 up to N 512, 4 at
// 1024, 2 at 2048, 1 at 4096; the workgroup takes its tile in RTS_PGA_BIN_TILE / BT passes.  The grid is (tiles, n_rx).
#define RTS_PGA_LDS_MAX 163840u
static inline size_t rts_pga_lds_bytes(uint32_t N, uint32_t BT) { return 2u * (size_t)N * BT * 16u + (size_t)N * 8u; }
struct RtsPgaPlan { uint32_t logN, BT, passes, tiles, n_gate, window0, window_min; size_t lds, partial_doubles, out_doubles; bool supported; };
static inline RtsPgaPlan rts_pga_plan(uint32_t n_rx, uint32_t N, uint32_t n_gate, uint32_t n_iters, uint32_t window0, uint32_t window_min)
{
    RtsPgaPlan p;
    p.logN = rts_stft_log2(N);
    p.BT = RTS_PGA_BIN_TILE; while (p.BT > 1u && rts_pga_lds_bytes(N, p.BT) > RTS_PGA_LDS_MAX) p.BT >>= 1;
    p.lds = rts_pga_lds_bytes(N, p.BT);
    p.passes = RTS_PGA_BIN_TILE / p.BT;
    p.tiles = (uint32_t)(((uint64_t)n_gate + RTS_PGA_BIN_TILE - 1u) / RTS_PGA_BIN_TILE);
    p.n_gate = n_gate;
    p.window0 = window0 ? window0 : N / 2u; p.window_min = window_min ? window_min : 8u;
    p.partial_doubles = 2u * (size_t)n_rx * p.tiles * N;
    p.out_doubles = (size_t)n_rx * N + (size_t)n_rx * n_iters;
    p.supported = p.lds <= RTS_PGA_LDS_MAX && n_rx <= RTS_FOCUS_MAX_RX;
    return p;
}

// The correction.  One thread per (receiver, row, bin); the grid is (n_pulses * ceil(n_bins / 256), n_rx).
struct RtsCorrectPlan { uint32_t tiles; size_t scratch_doubles, table_doubles; bool supported; };
static inline RtsCorrectPlan rts_correct_plan(uint32_t n_rx, uint32_t n_pulses, uint32_t n_bins, bool shifts_host, bool phase_host, bool resample)
{
    RtsCorrectPlan p;
    p.tiles = (uint32_t)(((uint64_t)n_bins + RTS_FOCUS_THREADS - 1u) / RTS_FOCUS_THREADS);
    p.scratch_doubles = resample ? 2u * (size_t)n_rx * n_pulses * n_bins : 0;
    p.table_doubles = ((shifts_host ? 1u : 0u) + (phase_host ? 1u : 0u)) * (size_t)n_rx * n_pulses;
    p.supported = n_rx <= RTS_FOCUS_MAX_RX && (uint64_t)n_pulses * p.tiles <= RTS_FOCUS_MAX_GRID_X;
    return p;
}

// ------------------------------------------------------------------------------------------------ the host evaluators (validated by the caller)
// cube [n_rx][q->n_pulses][q->n_bins] interleaved; out: S [n_rx][P]; work: P n_bins + n_gate + n_lags doubles
static inline void rts_align_eval_host(const RtsCubeParams* q, const double* cube, const RtsAlignParams* p, const RtsAlignPlan& plan, double* out, double* work)
{
    const uint32_t P = p->n_pulses, nb = q->n_bins, G = plan.n_gate, L = p->max_lag;
    double* env = work; double* ref = env + (size_t)P * nb; double* C = ref + G;
    for (uint32_t r = 0; r < q->n_rx; r++) {
        const double* rows = cube + 2 * (((size_t)r * q->n_pulses + p->first_pulse) * nb);
        for (size_t i = 0; i < (size_t)P * nb; i++) env[i] = rts_focus_envelope(rows[2 * i], rows[2 * i + 1]);
        double* S = out + (size_t)r * P;
        for (uint32_t j = 0; j < P; j++) S[j] = 0.0;
        for (uint32_t it = 0; it < p->n_iters; it++) {
            for (uint32_t g = 0; g < G; g++) ref[g] = rts_align_ref_at(env, S, P, nb, p->first_bin + g);
            for (uint32_t j = 0; j < P; j++) {
                for (uint32_t li = 0; li < plan.n_lags; li++) {
                    double c = 0.0;
                    for (uint32_t b = 0; b < plan.n_blocks; b++) {
                        const uint32_t g0 = b * RTS_ALIGN_BIN_BLOCK, g1 = G - g0 < RTS_ALIGN_BIN_BLOCK ? G : g0 + RTS_ALIGN_BIN_BLOCK;
                        c += rts_align_block(ref, env + (size_t)j * nb, nb, p->first_bin, g0, g1, (int32_t)li - (int32_t)L);
                    }
                    C[li] = c;
                }
                S[j] = rts_align_pick(C, L, p->flags);
            }
        }
    }
}

// one gate column's gradient products a[N] (interleaved): col, col + 2 row_stride, ... are the column's N samples; rot: this
// receiver's N rotations (cs, sn); x, y: N complex each
static inline void rts_pga_column_host(const double* col, size_t row_stride, uint32_t N, uint32_t logN, const double* tw, const double* rot, uint32_t W, double* x, double* y, double* a)
{
    for (uint32_t i = 0; i < N; i++) {
        double re = col[2 * row_stride * i], im = col[2 * row_stride * i + 1];
        rts_focus_unrotate(rot[2 * i], rot[2 * i + 1], &re, &im);
        const uint32_t r = rts_stft_bitrev(i, logN);
        x[2 * r] = re; x[2 * r + 1] = im;
    }
    for (uint32_t s = 1; s <= logN; s++)
        for (uint32_t j = 0; j < N / 2u; j++) {
            uint32_t i0, i1, k; rts_stft_pair(j, s, N, &i0, &i1, &k);
            rts_stft_butterfly(tw[2 * k], tw[2 * k + 1], &x[2 * i0], &x[2 * i0 + 1], &x[2 * i1], &x[2 * i1 + 1]);
        }
    uint32_t ks = 0; double best = rts_stft_power(x[0], x[1]);
    for (uint32_t k = 1; k < N; k++) { const double pw = rts_stft_power(x[2 * k], x[2 * k + 1]); if (pw > best) { best = pw; ks = k; } }
    for (uint32_t k = 0; k < N; k++) {
        double re = 0.0, im = 0.0;
        if (rts_pga_keep(k, N, W)) { const uint32_t m = (k + ks) & (N - 1u); re = x[2 * m]; im = -x[2 * m + 1]; }
        const uint32_t r = rts_stft_bitrev(k, logN);
        y[2 * r] = re; y[2 * r + 1] = im;
    }
    for (uint32_t s = 1; s <= logN; s++)
        for (uint32_t j = 0; j < N / 2u; j++) {
            uint32_t i0, i1, k; rts_stft_pair(j, s, N, &i0, &i1, &k);
            rts_stft_butterfly(tw[2 * k], tw[2 * k + 1], &y[2 * i0], &y[2 * i0 + 1], &y[2 * i1], &y[2 * i1 + 1]);
        }
    a[0] = 0.0; a[1] = 0.0;
    for (uint32_t i = 1; i < N; i++) rts_pga_product(y[2 * i], -y[2 * i + 1], y[2 * i - 2], -y[2 * i - 1], &a[2 * i], &a[2 * i + 1]);
}

// phase [n_rx][N], rms [n_rx][n_iters]; work: 12 N doubles (x, y, a, the tile's sums, the sums: 2 N each; the twiddles N; psi N)
// plus 2 N for the rotations: 14 N
static inline void rts_pga_eval_host(const RtsCubeParams* q, const double* cube, const RtsPgaParams* p, const RtsPgaPlan& plan, double* phase, double* rms, double* work)
{
    const uint32_t N = p->n_pulses, G = plan.n_gate;
    double* x = work; double* y = x + 2 * (size_t)N; double* a = y + 2 * (size_t)N; double* ts = a + 2 * (size_t)N; double* A = ts + 2 * (size_t)N;
    double* tw = A + 2 * (size_t)N; double* psi = tw + N; double* rot = psi + N;
    rts_stft_twiddles_host(N, tw);
    for (uint32_t r = 0; r < q->n_rx; r++) {
        double* phi = phase + (size_t)r * N;
        for (uint32_t i = 0; i < N; i++) phi[i] = 0.0;
        uint32_t W = plan.window0;
        for (uint32_t it = 0; it < p->n_iters; it++) {
            for (uint32_t i = 0; i < N; i++) rts_focus_rotation(phi[i], &rot[2 * i], &rot[2 * i + 1]);
            for (uint32_t g = 0; g < G; g++) {
                const double* col = cube + 2 * ((((size_t)r * q->n_pulses + p->first_pulse) * q->n_bins) + p->first_bin + g);
                rts_pga_column_host(col, q->n_bins, N, plan.logN, tw, rot, W, x, y, a);
                const bool first_of_tile = g % RTS_PGA_BIN_TILE == 0, last_of_tile = g % RTS_PGA_BIN_TILE == RTS_PGA_BIN_TILE - 1u || g == G - 1u;
                for (uint32_t i = 0; i < 2 * N; i++) { if (first_of_tile) ts[i] = 0.0; ts[i] += a[i]; }
                if (last_of_tile) for (uint32_t i = 0; i < 2 * N; i++) { if (g < RTS_PGA_BIN_TILE) A[i] = ts[i]; else A[i] += ts[i]; }
            }
            psi[0] = 0.0;
            for (uint32_t i = 1; i < N; i++) psi[i] = rts_pga_delta(A[2 * i], A[2 * i + 1]);
            rms[(size_t)r * p->n_iters + it] = rts_pga_update(N, psi);
            for (uint32_t i = 0; i < N; i++) phi[i] += psi[i];
            W = rts_pga_next_window(W, plan.window_min);
        }
    }
}

// one corrected sample: bin n of a row (src: the row as it was), shift S or none, rotation (cs, sn) or none
RTS_HD void rts_correct_sample(const double* src, uint32_t n_bins, const RtsImageInterp ip, uint32_t n, bool has_shift, double S, bool has_phase, double cs, double sn, double* re, double* im)
{
    double vr, vi;
    if (has_shift) rts_image_sample(src, n_bins, ip, (double)n + S, &vr, &vi);
    else { vr = src[2 * (size_t)n]; vi = src[2 * (size_t)n + 1]; }
    if (has_phase) rts_focus_unrotate(cs, sn, &vr, &vi);
    *re = vr; *im = vi;
}

// the cube corrected in place; shifts, phase: [n_rx][P] or NULL; work: 2 n_bins doubles (a row as it was)
static inline void rts_correct_eval_host(const RtsCubeParams* q, double* cube, const RtsCorrectParams* p, const double* shifts, const double* phase, double* work)
{
    const RtsImageInterp ip = rts_image_interp_setup(p->taps);
    const uint32_t P = p->n_pulses, nb = q->n_bins;
    for (uint32_t r = 0; r < q->n_rx; r++)
        for (uint32_t j = 0; j < P; j++) {
            double* row = cube + 2 * (((size_t)r * q->n_pulses + p->first_pulse + j) * nb);
            for (size_t i = 0; i < 2 * (size_t)nb; i++) work[i] = row[i];
            double cs = 1.0, sn = 0.0;
            if (phase) rts_focus_rotation(phase[(size_t)r * P + j], &cs, &sn);
            const double S = shifts ? shifts[(size_t)r * P + j] : 0.0;
            for (uint32_t n = 0; n < nb; n++) rts_correct_sample(work, nb, ip, n, shifts != nullptr, S, phase != nullptr, cs, sn, &row[2 * (size_t)n], &row[2 * (size_t)n + 1]);
        }
}
