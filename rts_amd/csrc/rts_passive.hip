// rts_passive.hip -- passive radar on the device (include/rts_amd.h: rts_cube_cancel, rts_cube_xcorr): k_passive_gram,
// k_passive_cross, k_passive_reduce, k_passive_solve, k_passive_apply, k_passive_xcorr.  The arithmetic, the partition and the plans
// of the launches are rts_passive.h (and rts_adapt.h's factor and substitutions), shared with the host evaluators.  No atomics and no
// MFMA (its accumulation is fused; the trees here are uncontracted): identical bits from run to run and on the host.
#include <hip/hip_runtime.h>
#include "rts_internal.h"
#include "rts_passive.h"

struct RtsCancelArgs {
    double2* cube;                    // receiver 0, row 0, bin 0 of the attached cube
    uint64_t rx_stride;               // elements between two receivers
    uint64_t mask;                    // the receivers cancelled
    uint32_t ref_rx, first, rows, R, n_bins, K, n_rx, n_blocks, tpr, ppb, tri, stride, gram_blocks;
    double loading;
    double2* part;                    // [n_blocks][ppb][stride]
    double2* sums;                    // [n_blocks][stride]
    double2* coeff;                   // [n_rx][n_blocks][K]
    uint32_t* fail;                   // [n_blocks]
};

// the part a workgroup sums: block b, its part q -> the tiles [t0, t1) of the block; false: the block has fewer parts than q + 1
__device__ __forceinline__ bool rts_passive_part(const RtsCancelArgs& a, uint32_t slot, uint32_t* b, uint64_t* t0, uint64_t* t1)
{
    *b = slot / a.ppb; const uint32_t q = slot % a.ppb;
    const uint64_t tiles = (uint64_t)rts_cancel_block_rows(a.rows, a.R, *b) * a.tpr;
    const uint32_t parts = rts_cancel_block_parts(tiles, a.ppb);
    if (q >= parts) return false;
    *t0 = rts_cov_part_begin(tiles, parts, q); *t1 = rts_cov_part_begin(tiles, parts, q + 1u);
    return true;
}
// tile t of block b: its row of the cube and its bins [n0, n0 + nb)
__device__ __forceinline__ void rts_passive_tile(const RtsCancelArgs& a, uint32_t b, uint64_t t, uint64_t* row, uint32_t* n0, uint32_t* nb)
{
    *row = (uint64_t)a.first + (uint64_t)b * a.R + t / a.tpr;
    *n0 = (uint32_t)(t % a.tpr) * RTS_PASSIVE_TILE;
    *nb = a.n_bins - *n0 < RTS_PASSIVE_TILE ? a.n_bins - *n0 : RTS_PASSIVE_TILE;
}
// the reference's bins n0 - (K - 1) .. n0 + nb - 1 of one row -> s_x[0 .. nb + K - 1): element e is bin n0 + e - (K - 1), +0.0 before
// the row's start (rts_passive_lag's rule), so that x_k of bin n0 + cc is s_x[cc + K - 1 - k]
__device__ __forceinline__ void rts_passive_stage_ref(double2* s_x, const double2* __restrict__ ref_row, uint32_t n0, uint32_t nb, uint32_t K, uint32_t t, uint32_t nt)
{
    for (uint32_t e = t; e < nb + K - 1u; e += nt) {
        const uint32_t back = K - 1u - (e < K - 1u ? e : K - 1u);           // how far bin n0 + e - (K - 1) lies before n0 (0 from e = K - 1 on)
        double2 v = make_double2(0.0, 0.0);
        if (back <= n0) v = ref_row[n0 + e - (K - 1u)];
        s_x[e] = v;
    }
}

// The Gram matrix of the lagged copies of ONE row: per cell K (K + 1) / 2 terms of eight f64 operations against 16 bytes read.  One
// workgroup per (block, part); the tile of the reference in LDS serves every entry.  A thread owns an RTS_ADAPT_BLOCK x
// RTS_ADAPT_BLOCK block of entries and keeps the running sums in registers across the part's tiles.
__device__ __forceinline__ void rts_gram_cell(bool first, const double2* __restrict__ s_x, const uint32_t* oi, const uint32_t* oj, uint32_t cc, double2 (*acc)[RTS_ADAPT_BLOCK])
{
    double2 xi[RTS_ADAPT_BLOCK], xj[RTS_ADAPT_BLOCK];
#pragma unroll
    for (uint32_t k = 0; k < RTS_ADAPT_BLOCK; k++) { xi[k] = s_x[oi[k] + cc]; xj[k] = s_x[oj[k] + cc]; }
#pragma unroll
    for (uint32_t x = 0; x < RTS_ADAPT_BLOCK; x++)
#pragma unroll
        for (uint32_t y = 0; y < RTS_ADAPT_BLOCK; y++) rts_adapt_add(first, xj[y].x, xj[y].y, xi[x].x, xi[x].y, &acc[x][y].x, &acc[x][y].y);      // conj(x_i) x_j
}
__global__ void __launch_bounds__(576) k_passive_gram(const RtsCancelArgs a)
{
    extern __shared__ __attribute__((aligned(16))) double2 s_gram_x[];          // [RTS_PASSIVE_TILE + K - 1]
    const uint32_t t = threadIdx.x;
    uint32_t b; uint64_t t0, t1;
    if (!rts_passive_part(a, blockIdx.x, &b, &t0, &t1)) return;                  // (the whole workgroup)
    const bool active = t < a.gram_blocks;
    uint32_t bi = 0u, bj = 0u;
    if (active) rts_cov_block(t, &bi, &bj);
    uint32_t oi[RTS_ADAPT_BLOCK], oj[RTS_ADAPT_BLOCK];                           // K - 1 - lag (past the last lag: the last one again, sums nobody stores)
#pragma unroll
    for (uint32_t k = 0; k < RTS_ADAPT_BLOCK; k++) {
        const uint32_t i = bi * RTS_ADAPT_BLOCK + k, j = bj * RTS_ADAPT_BLOCK + k;
        oi[k] = a.K - 1u - (i < a.K ? i : a.K - 1u); oj[k] = a.K - 1u - (j < a.K ? j : a.K - 1u);
    }
    double2 acc[RTS_ADAPT_BLOCK][RTS_ADAPT_BLOCK];
#pragma unroll
    for (uint32_t k = 0; k < RTS_ADAPT_BLOCK * RTS_ADAPT_BLOCK; k++) acc[k / RTS_ADAPT_BLOCK][k % RTS_ADAPT_BLOCK] = make_double2(0.0, 0.0);
    const double2* __restrict__ ref = a.cube + (uint64_t)a.ref_rx * a.rx_stride;
    for (uint64_t tile = t0; tile < t1; tile++) {
        uint64_t row; uint32_t n0, nb;
        rts_passive_tile(a, b, tile, &row, &n0, &nb);
        __syncthreads();                                                          // (the previous tile's reads are done)
        rts_passive_stage_ref(s_gram_x, ref + row * a.n_bins, n0, nb, a.K, t, blockDim.x);
        __syncthreads();
        if (active) {
            uint32_t cc = 0u;
            if (tile == t0) { rts_gram_cell(true, s_gram_x, oi, oj, 0u, acc); cc = 1u; }      // the part's first cell: the start value
            for (; cc < nb; cc++) rts_gram_cell(false, s_gram_x, oi, oj, cc, acc);
        }
    }
    if (!active) return;
    double2* out = a.part + (size_t)blockIdx.x * a.stride;
#pragma unroll
    for (uint32_t x = 0; x < RTS_ADAPT_BLOCK; x++)
#pragma unroll
        for (uint32_t y = 0; y < RTS_ADAPT_BLOCK; y++) {
            const uint32_t i = bi * RTS_ADAPT_BLOCK + x, j = bj * RTS_ADAPT_BLOCK + y;
            if (i < a.K && j <= i) out[rts_passive_tri(i, j)] = acc[x][y];
        }
}

// the r-th set bit of mask (r below its population count)
__device__ __forceinline__ uint32_t rts_passive_nth(uint64_t mask, uint32_t r)
{
    for (uint32_t k = 0; k < r; k++) mask &= mask - 1ull;
    return (uint32_t)__builtin_ctzll(mask);
}

// The cross vectors: wave w of a workgroup owns cancelled receiver RTS_PASSIVE_CROSS_RX blockIdx.y + w, lane i its b_r[i].  The
// reference tile is shared by the waves; each stages its own receiver's tile.  y of a cell is one address for the wave (a
// broadcast), x_i consecutive 16-byte slots downwards: no bank conflict.
__global__ void __launch_bounds__(RTS_PASSIVE_CROSS_RX * RTS_PASSIVE_WAVE) k_passive_cross(const RtsCancelArgs a, uint32_t n_sel)
{
    extern __shared__ __attribute__((aligned(16))) double2 s_cross[];            // x [RTS_PASSIVE_TILE + K - 1], then y [RTS_PASSIVE_CROSS_RX][RTS_PASSIVE_TILE]
    const uint32_t t = threadIdx.x, w = t / RTS_PASSIVE_WAVE, i = t % RTS_PASSIVE_WAVE;
    uint32_t b; uint64_t t0, t1;
    if (!rts_passive_part(a, blockIdx.x, &b, &t0, &t1)) return;
    const uint32_t sel = blockIdx.y * RTS_PASSIVE_CROSS_RX + w;
    const bool have = sel < n_sel;                                               // (the wave's: it stages and sums, or only keeps the barriers)
    const uint32_t r = have ? rts_passive_nth(a.mask, sel) : 0u;
    const bool active = have && i < a.K;
    double2* s_x = s_cross; double2* s_y = s_cross + RTS_PASSIVE_TILE + a.K - 1u + (size_t)w * RTS_PASSIVE_TILE;
    const uint32_t oi = a.K - 1u - (i < a.K ? i : a.K - 1u);
    const double2* __restrict__ ref = a.cube + (uint64_t)a.ref_rx * a.rx_stride;
    const double2* __restrict__ y = a.cube + (uint64_t)r * a.rx_stride;
    double2 acc = make_double2(0.0, 0.0);
    for (uint64_t tile = t0; tile < t1; tile++) {
        uint64_t row; uint32_t n0, nb;
        rts_passive_tile(a, b, tile, &row, &n0, &nb);
        __syncthreads();
        rts_passive_stage_ref(s_x, ref + row * a.n_bins, n0, nb, a.K, t, blockDim.x);
        if (have) for (uint32_t e = i; e < nb; e += RTS_PASSIVE_WAVE) s_y[e] = y[row * a.n_bins + n0 + e];
        __syncthreads();
        if (active)
            for (uint32_t cc = 0; cc < nb; cc++) {
                const double2 yv = s_y[cc], xv = s_x[oi + cc];
                rts_adapt_add(tile == t0 && cc == 0u, yv.x, yv.y, xv.x, xv.y, &acc.x, &acc.y);      // conj(x_i) y
            }
    }
    if (active) a.part[(size_t)blockIdx.x * a.stride + a.tri + (size_t)r * a.K + i] = acc;
}

// one thread per (block, entry of its record): the parts' sums in ascending order, part 0 the start value; RTS_PASSIVE_REDUCE_BATCH
// loads in flight at once
__global__ void __launch_bounds__(RTS_PASSIVE_REDUCE_THREADS) k_passive_reduce(const RtsCancelArgs a)
{
    const uint64_t g = (uint64_t)blockIdx.x * RTS_PASSIVE_REDUCE_THREADS + threadIdx.x;
    if (g >= (uint64_t)a.n_blocks * a.stride) return;
    const uint32_t b = (uint32_t)(g / a.stride), e = (uint32_t)(g % a.stride);
    if (e >= a.tri && !((a.mask >> ((e - a.tri) / a.K)) & 1ull)) return;       // a receiver that is not cancelled: nobody wrote or reads its b
    const uint64_t tiles = (uint64_t)rts_cancel_block_rows(a.rows, a.R, b) * a.tpr;
    const uint32_t parts = rts_cancel_block_parts(tiles, a.ppb);
    const double2* __restrict__ part = a.part + (size_t)b * a.ppb * a.stride + e;
    double2 s = part[0];
    for (uint32_t q0 = 1; q0 < parts; q0 += RTS_PASSIVE_REDUCE_BATCH) {
        double2 v[RTS_PASSIVE_REDUCE_BATCH];
#pragma unroll
        for (uint32_t k = 0; k < RTS_PASSIVE_REDUCE_BATCH; k++) v[k] = part[(size_t)(q0 + k < parts ? q0 + k : parts - 1u) * a.stride];
#pragma unroll
        for (uint32_t k = 0; k < RTS_PASSIVE_REDUCE_BATCH; k++) if (q0 + k < parts) { s.x += v[k].x; s.y += v[k].y; }
    }
    a.sums[g] = s;
}

// One workgroup per block, k_mvdr's shape: A = G + loading I in LDS, thread i owns row i of the factor, column by column; then
// thread r solves receiver r's coefficients on its own column of the work vectors.  A failed pivot: every coefficient of the block
// is 0 and the block's word is the column + 1.
__global__ void __launch_bounds__(RTS_PASSIVE_SOLVE_THREADS) k_passive_solve(const RtsCancelArgs a)
{
    extern __shared__ __attribute__((aligned(16))) double2 s_solve[];            // L [K][K], then the work vectors [K][RTS_PASSIVE_SOLVE_THREADS]
    __shared__ uint32_t s_fail; __shared__ double s_ljj;
    const uint32_t t = threadIdx.x, K = a.K, b = blockIdx.x;
    const double2* __restrict__ rec = a.sums + (size_t)b * a.stride;
    double* L = (double*)s_solve;
    for (uint32_t e = t; e < K * K; e += RTS_PASSIVE_SOLVE_THREADS) {
        const uint32_t i = e / K, j = e % K;
        if (j > i) continue;
        double2 v = rec[rts_passive_tri(i, j)];
        if (i == j) v.x = v.x + a.loading;
        s_solve[e] = v;
    }
    if (t == 0u) s_fail = 0u;
    __syncthreads();
    uint32_t fail = 0u;
    for (uint32_t j = 0; j < K; j++) {
        if (t == j) {
            const double d = rts_mvdr_pivot(L, K, j);
            if (!rts_adapt_pivot_ok(d)) s_fail = j + 1u;
            else { const double ljj = sqrt(d); L[2 * ((size_t)j * K + j)] = ljj; s_ljj = ljj; }
        }
        __syncthreads();
        fail = s_fail;                                                            // (the same word for every thread: they leave together)
        if (fail) break;
        if (t > j && t < K) rts_mvdr_below(L, K, t, j, s_ljj);
        __syncthreads();
    }
    if (t == 0u) a.fail[b] = fail;
    double* x = (double*)(s_solve + (size_t)K * K + t);
    for (uint32_t r = t; r < a.n_rx; r += RTS_PASSIVE_SOLVE_THREADS) {
        double2* c = a.coeff + ((size_t)r * a.n_blocks + b) * K;
        if (fail || !((a.mask >> r) & 1ull)) { for (uint32_t k = 0; k < K; k++) c[k] = make_double2(0.0, 0.0); continue; }
        rts_chol_forward(L, K, K, (const double*)(rec + a.tri + (size_t)r * K), x, RTS_PASSIVE_SOLVE_THREADS);
        rts_chol_back(L, K, K, x, RTS_PASSIVE_SOLVE_THREADS);
        for (uint32_t k = 0; k < K; k++) c[k] = make_double2(x[2 * (size_t)k * RTS_PASSIVE_SOLVE_THREADS], x[2 * (size_t)k * RTS_PASSIVE_SOLVE_THREADS + 1]);
    }
}

// One workgroup per (row and tile, cancelled receiver), one thread per bin: y - c_0 x_0 - ... - c_{K-1} x_{K-1}, k ascending.  The
// rows of a failed block are left as they are.
__global__ void __launch_bounds__(RTS_PASSIVE_TILE) k_passive_apply(const RtsCancelArgs a)
{
    extern __shared__ __attribute__((aligned(16))) double2 s_apply[];            // x [RTS_PASSIVE_TILE + K - 1], then c [K]
    const uint32_t t = threadIdx.x, K = a.K;
    const uint32_t row = blockIdx.x / a.tpr, tile = blockIdx.x % a.tpr, b = row / a.R;
    if (a.fail[b]) return;                                                       // (the whole workgroup)
    const uint32_t r = rts_passive_nth(a.mask, blockIdx.y);
    const uint32_t n0 = tile * RTS_PASSIVE_TILE, nb = a.n_bins - n0 < RTS_PASSIVE_TILE ? a.n_bins - n0 : RTS_PASSIVE_TILE;
    double2* s_x = s_apply; double2* s_c = s_apply + RTS_PASSIVE_TILE + K - 1u;
    const size_t at = ((size_t)a.first + row) * a.n_bins;
    rts_passive_stage_ref(s_x, a.cube + (uint64_t)a.ref_rx * a.rx_stride + at, n0, nb, K, t, RTS_PASSIVE_TILE);
    if (t < K) s_c[t] = a.coeff[((size_t)r * a.n_blocks + b) * K + t];
    __syncthreads();
    if (t >= nb) return;
    double2* y = a.cube + (uint64_t)r * a.rx_stride + at + n0 + t;
    double2 v = *y;
    for (uint32_t k = 0; k < K; k++) { const double2 c = s_c[k], x = s_x[t + K - 1u - k]; rts_adapt_sub_mul(c.x, c.y, x.x, x.y, &v.x, &v.y); }
    *y = v;
}

int rts_cube_cancel_device(RtsContext* c, const RtsCancelParams& p, const RtsCancelPlan& plan, uint64_t mask)
{
    const RtsCubeParams& q = c->cube.params;
    RtsPassiveState& s = c->cube.passive;
    RtsCancelArgs a;
    a.cube = (double2*)c->cube.p; a.rx_stride = (uint64_t)q.n_pulses * q.n_bins; a.mask = mask;
    a.ref_rx = p.ref_rx; a.first = p.first_pulse; a.rows = plan.rows; a.R = plan.R; a.n_bins = q.n_bins; a.K = plan.K; a.n_rx = q.n_rx;
    a.n_blocks = plan.n_blocks; a.tpr = plan.tpr; a.ppb = plan.ppb; a.tri = plan.tri; a.stride = plan.stride; a.gram_blocks = plan.gram_blocks;
    a.loading = p.loading;
    a.part = (double2*)s.d_part.p; a.sums = (double2*)s.d_sums.p; a.coeff = (double2*)s.d_coeff.p; a.fail = s.d_fail.p;
    const uint32_t n_sel = (uint32_t)__builtin_popcountll(mask);
    const uint32_t slots = plan.n_blocks * plan.ppb;
    k_passive_gram<<<slots, plan.gram_threads, plan.gram_lds, c->stream>>>(a);
    RTS_HIP(hipGetLastError());
    if (n_sel) {
        const dim3 grid(slots, (n_sel + RTS_PASSIVE_CROSS_RX - 1u) / RTS_PASSIVE_CROSS_RX);
        k_passive_cross<<<grid, RTS_PASSIVE_CROSS_RX * RTS_PASSIVE_WAVE, plan.gram_lds + 16u * RTS_PASSIVE_CROSS_RX * RTS_PASSIVE_TILE, c->stream>>>(a, n_sel);
        RTS_HIP(hipGetLastError());
    }
    const uint64_t entries = (uint64_t)plan.n_blocks * plan.stride;
    k_passive_reduce<<<(unsigned)((entries + RTS_PASSIVE_REDUCE_THREADS - 1u) / RTS_PASSIVE_REDUCE_THREADS), RTS_PASSIVE_REDUCE_THREADS, 0, c->stream>>>(a);
    RTS_HIP(hipGetLastError());
    RTS_HIP(hipFuncSetAttribute((const void*)k_passive_solve, hipFuncAttributeMaxDynamicSharedMemorySize, (int)plan.solve_lds));
    k_passive_solve<<<plan.n_blocks, RTS_PASSIVE_SOLVE_THREADS, plan.solve_lds, c->stream>>>(a);
    RTS_HIP(hipGetLastError());
    if (n_sel) {
        const dim3 grid(plan.rows * plan.tpr, n_sel);
        k_passive_apply<<<grid, RTS_PASSIVE_TILE, plan.gram_lds + 16u * plan.K, c->stream>>>(a);
        RTS_HIP(hipGetLastError());
    }
    return RTS_OK;
}

// One workgroup per (group of RTS_XCORR_THREADS lags, row, receiver), thread t the lag first_lag + group RTS_XCORR_THREADS + t.  The
// surveillance row passes through LDS in windows: the samples n0 + l0 .. n0 + l0 + RTS_XCORR_WINDOW + RTS_XCORR_THREADS - 1, so
// that lag l0 + t of reference sample n0 + nn is element nn + t -- the lanes read consecutive 16-byte slots.  The reference sample
// is one address for the workgroup (a scalar load).  A thread stops where its lag leaves the row.
__global__ void __launch_bounds__(RTS_XCORR_THREADS) k_passive_xcorr(const double2* __restrict__ cube, double2* __restrict__ out, uint64_t rx_stride, uint32_t ref_rx, uint32_t first,
                                                                     uint32_t n_rows, uint32_t n_bins, uint32_t first_lag, uint32_t n_lags)
{
    __shared__ __attribute__((aligned(16))) double2 s_y[RTS_XCORR_WINDOW + RTS_XCORR_THREADS];
    const uint32_t t = threadIdx.x, row = blockIdx.y, r = blockIdx.z;
    const uint32_t l0 = first_lag + blockIdx.x * RTS_XCORR_THREADS, l = l0 + t;
    const double2* __restrict__ y = cube + (uint64_t)r * rx_stride + ((uint64_t)first + row) * n_bins;
    const double2* __restrict__ ref = cube + (uint64_t)ref_rx * rx_stride + ((uint64_t)first + row) * n_bins;
    const uint32_t group_end = l0 < n_bins ? n_bins - l0 : 0u;                   // reference samples the group's first lag sums: the most of the group
    const uint32_t my_end = l < n_bins ? n_bins - l : 0u;
    double2 acc = make_double2(0.0, 0.0);
    for (uint32_t n0 = 0; n0 < group_end; n0 += RTS_XCORR_WINDOW) {
        __syncthreads();
        for (uint32_t e = t; e < RTS_XCORR_WINDOW + RTS_XCORR_THREADS; e += RTS_XCORR_THREADS) {
            const uint64_t n = (uint64_t)n0 + l0 + e;
            s_y[e] = n < n_bins ? y[n] : make_double2(0.0, 0.0);
        }
        __syncthreads();
        const uint32_t lim = my_end > n0 ? (my_end - n0 < RTS_XCORR_WINDOW ? my_end - n0 : RTS_XCORR_WINDOW) : 0u;
        for (uint32_t nn = 0; nn < lim; nn++) {
            const double2 yv = s_y[nn + t], xv = ref[n0 + nn];
            rts_adapt_add(n0 + nn == 0u, yv.x, yv.y, xv.x, xv.y, &acc.x, &acc.y);
        }
    }
    if (blockIdx.x * RTS_XCORR_THREADS + t < n_lags) out[((size_t)r * n_rows + row) * n_lags + blockIdx.x * RTS_XCORR_THREADS + t] = acc;
}

int rts_cube_xcorr_device(RtsContext* c, const RtsXcorrParams& p, const RtsXcorrPlan& plan, double* out)
{
    const RtsCubeParams& q = c->cube.params;
    const dim3 grid(plan.lag_groups, p.n_pulses, q.n_rx);
    k_passive_xcorr<<<grid, RTS_XCORR_THREADS, 0, c->stream>>>((const double2*)c->cube.p, (double2*)out, (uint64_t)q.n_pulses * q.n_bins, p.ref_rx, p.first_pulse, p.n_pulses, q.n_bins,
                                                               p.first_lag, p.n_lags);
    RTS_HIP(hipGetLastError());
    return RTS_OK;
}
