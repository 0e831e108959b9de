// rts_adapt.hip -- adaptive (MVDR) beamforming on the device (include/rts_amd.h: rts_cube_covariance, rts_cube_mvdr): k_cube_cov,
// k_cube_cov_reduce, k_mvdr.  The arithmetic, the partition and the plans of the launches are rts_adapt.h, shared with the host
// evaluators.
#include <hip/hip_runtime.h>
#include "rts_internal.h"
#include "rts_adapt.h"
#include "rts_stap.h"

// The sample covariance is a rank-K update of the lower triangle of an n_rx x n_rx Hermitian matrix: per training cell
// n_rx (n_rx + 1) / 2 terms of four multiplies, an add and a subtract plus the two adds of the running sum, all f64 and uncontracted
// (the evaluator walks the same tree), against 16 n_rx bytes read: bound by f64 issue from about 8 receivers on.
// k_cube_cov: one workgroup per part of the tree.  It walks the part's tiles in ascending order; a tile is staged in LDS as
// [rx][cell], the lanes of a wave loading consecutive cells of one receiver (consecutive 16-byte elements but for the skipped bins
// and the row ends) into registers while the tile before is summed.  A thread owns one RTS_ADAPT_BLOCK x RTS_ADAPT_BLOCK block
// of entries (i, j <= i) and keeps their running sums in registers across all tiles of the part; per cell it reads the block's z_i and z_j from LDS, 16 bytes each (rts_adapt.h: the
// padded rows keep a wave's reads off each other's banks).  The part's partial [n_rx][n_rx] (lower triangle) is written with plain
// stores: no atomics.  k_cube_cov_reduce sums the partials in ascending part order, divides by K and writes both triangles.
struct RtsCovArgs {
    const double2* in;                // receiver 0, row 0, bin 0 of the source
    uint64_t rx_stride, K, tiles;     // elements between two receivers of the source; training cells; tiles
    RtsCovSet set;
    uint32_t row_bins, parts, n_rx, blocks;       // n_rx: the matrix's order (the stacked form: n_taps n_sp)
    uint32_t n_sp;                    // the stacked form (rts_stap.h): the source's receivers; row d of the matrix is receiver d % n_sp, d / n_sp rows on
    double2* part;                    // [parts][n_rx][n_rx]
    double2* out;                     // [n_rx][n_rx]
};

__device__ __forceinline__ void rts_cov_cell(bool first, const double2* __restrict__ s_z, const uint32_t* ri, const uint32_t* rj, uint32_t q, double2 (*acc)[RTS_ADAPT_BLOCK])
{
    double2 zi[RTS_ADAPT_BLOCK], zj[RTS_ADAPT_BLOCK];
#pragma unroll
    for (uint32_t a = 0; a < RTS_ADAPT_BLOCK; a++) { zi[a] = s_z[ri[a] + q]; zj[a] = s_z[rj[a] + q]; }
#pragma unroll
    for (uint32_t a = 0; a < RTS_ADAPT_BLOCK; a++)
#pragma unroll
        for (uint32_t b = 0; b < RTS_ADAPT_BLOCK; b++) rts_adapt_add(first, zi[a].x, zi[a].y, zj[b].x, zj[b].y, &acc[a][b].x, &acc[a][b].y);
}

// the staging of a tile, in two halves: the thread's cell of its receivers r_first, r_first + r_step, ... (at most RTS_ADAPT_STAGE:
// rts_adapt.h's plan) from memory into registers, and from the registers into the receivers' LDS rows
template <bool ST> __device__ __forceinline__ void rts_cov_fetch(double2* pre, const RtsCovArgs& a, bool any, uint64_t tile, uint32_t cc, uint32_t r_first, uint32_t r_step)
{
    const uint64_t c = tile * RTS_ADAPT_TILE + cc;
    const bool live = any && c < a.K;
    const double2* __restrict__ src = a.in + (live ? rts_cov_cell_index(a.set, a.row_bins, c) : 0u);
#pragma unroll
    for (uint32_t k = 0; k < RTS_ADAPT_STAGE; k++) {       // (every register gets a value: the array stays in registers)
        const uint32_t r = r_first + k * r_step;
        double2 v = make_double2(0.0, 0.0);
        if (live && r < a.n_rx) v = src[ST ? rts_st_offset(r, a.n_sp, a.rx_stride, a.row_bins) : (uint64_t)r * a.rx_stride];
        pre[k] = v;
    }
}
__device__ __forceinline__ void rts_cov_stage(const double2* pre, double2* s_z, const RtsCovArgs& a, uint64_t tile, uint32_t cc, uint32_t r_first, uint32_t r_step)
{
    if (tile * RTS_ADAPT_TILE + cc >= a.K) return;
#pragma unroll
    for (uint32_t k = 0; k < RTS_ADAPT_STAGE; k++) { const uint32_t r = r_first + k * r_step; if (r < a.n_rx) s_z[rts_cov_lds_row(r, a.n_rx) * (RTS_ADAPT_TILE + 1u) + cc] = pre[k]; }
}

// (five waves per SIMD: two workgroups of nine waves on a CU, one summing while the other stages)
// ST: the stacked snapshots of rts_stap.h in place of the receivers -- only the staging's addresses differ
template <bool ST> __global__ void __launch_bounds__(RTS_ADAPT_MAX_THREADS) __attribute__((amdgpu_waves_per_eu(5, 8))) k_cube_cov(const RtsCovArgs a)
{
    extern __shared__ __attribute__((aligned(16))) double2 s_cov_z[];            // [n_rx][RTS_ADAPT_TILE + 1], the rows in rts_cov_lds_row's order
    const uint32_t t = threadIdx.x, p = blockIdx.x, ld = RTS_ADAPT_TILE + 1u;
    const uint64_t tile0 = rts_cov_part_begin(a.tiles, a.parts, p), tile1 = rts_cov_part_begin(a.tiles, a.parts, p + 1u);
    const bool active = t < a.blocks;
    uint32_t bi = 0u, bj = 0u;
    if (active) rts_cov_block(t, &bi, &bj);
    // the LDS rows of the block's receivers (past the last receiver: the last one again, sums nobody stores)
    uint32_t ri[RTS_ADAPT_BLOCK], rj[RTS_ADAPT_BLOCK];
#pragma unroll
    for (uint32_t k = 0; k < RTS_ADAPT_BLOCK; k++) {
        const uint32_t i = bi * RTS_ADAPT_BLOCK + k, j = bj * RTS_ADAPT_BLOCK + k;
        ri[k] = rts_cov_lds_row(i < a.n_rx ? i : a.n_rx - 1u, a.n_rx) * ld; rj[k] = rts_cov_lds_row(j < a.n_rx ? j : a.n_rx - 1u, a.n_rx) * ld;
    }
    double2 acc[RTS_ADAPT_BLOCK][RTS_ADAPT_BLOCK];
#pragma unroll
    for (uint32_t k = 0; k < RTS_ADAPT_BLOCK * RTS_ADAPT_BLOCK; k++) acc[k / RTS_ADAPT_BLOCK][k % RTS_ADAPT_BLOCK] = make_double2(0.0, 0.0);
    const uint32_t cc = t % RTS_ADAPT_TILE, r_first = (uint32_t)__builtin_amdgcn_readfirstlane((int)(t / RTS_ADAPT_TILE)), r_step = blockDim.x / RTS_ADAPT_TILE;
    double2 pre[RTS_ADAPT_STAGE];                                                 // (r_first is the wave's: its receivers' addresses are scalar)
    rts_cov_fetch<ST>(pre, a, true, tile0, cc, r_first, r_step);
    for (uint64_t tile = tile0; tile < tile1; tile++) {
        __syncthreads();                                                          // (the previous tile's reads are done)
        rts_cov_stage(pre, s_cov_z, a, tile, cc, r_first, r_step);
        __syncthreads();
        rts_cov_fetch<ST>(pre, a, tile + 1u < tile1, tile + 1u, cc, r_first, r_step);                  // the next tile: in flight while this one is summed
        const uint64_t left = a.K - tile * RTS_ADAPT_TILE;
        const uint32_t ncell = left < RTS_ADAPT_TILE ? (uint32_t)left : RTS_ADAPT_TILE;
        if (active) {
            uint32_t q = 0u;
            if (tile == tile0) { rts_cov_cell(true, s_cov_z, ri, rj, 0u, acc); q = 1u; }     // the part's first cell: the start value
            for (; q < ncell; q++) rts_cov_cell(false, s_cov_z, ri, rj, q, acc);
        }
    }
    if (!active) return;
#pragma unroll
    for (uint32_t x = 0; x < RTS_ADAPT_BLOCK; x++)
#pragma unroll
        for (uint32_t y = 0; y < RTS_ADAPT_BLOCK; y++) {
            const uint32_t i = bi * RTS_ADAPT_BLOCK + x, j = bj * RTS_ADAPT_BLOCK + y;
            if (i < a.n_rx && j <= i) a.part[((size_t)p * a.n_rx + i) * a.n_rx + j] = acc[x][y];
        }
}

__global__ void __launch_bounds__(RTS_ADAPT_REDUCE_THREADS) k_cube_cov_reduce(const RtsCovArgs a)
{
    const uint32_t e = blockIdx.x * RTS_ADAPT_REDUCE_THREADS + threadIdx.x;
    if (e >= a.n_rx * a.n_rx) return;
    const uint32_t i = e / a.n_rx, j = e % a.n_rx;
    if (j > i) return;
    const double2* __restrict__ part = a.part + e;
    const size_t stride = (size_t)a.n_rx * a.n_rx;
    double2 s = part[0];
    // the loads of RTS_ADAPT_REDUCE_BATCH parts in flight at once, the adds in ascending order (one load's latency per part would be
    // the whole call's time)
    for (uint32_t p0 = 1; p0 < a.parts; p0 += RTS_ADAPT_REDUCE_BATCH) {
        double2 v[RTS_ADAPT_REDUCE_BATCH];
#pragma unroll
        for (uint32_t k = 0; k < RTS_ADAPT_REDUCE_BATCH; k++) v[k] = part[(size_t)(p0 + k < a.parts ? p0 + k : a.parts - 1u) * stride];
#pragma unroll
        for (uint32_t k = 0; k < RTS_ADAPT_REDUCE_BATCH; k++) if (p0 + k < a.parts) { s.x += v[k].x; s.y += v[k].y; }
    }
    const double Kd = (double)a.K;
    s.x = s.x / Kd; s.y = s.y / Kd;
    if (i == j) a.out[e] = make_double2(s.x, 0.0);
    else { a.out[e] = s; a.out[(size_t)j * a.n_rx + i] = make_double2(s.x, -s.y); }
}

// in: the source's receiver 0, row 0 (device); rx_stride: its n_rows_in n_bins; part: plan.scratch_bytes of scratch; n_taps 1: the
// receivers' covariance, set and plan over the cube's n_rx; more: the stacked one, set over the snapshots' start rows, plan over n_taps n_rx
int rts_cube_cov_device(RtsContext* c, const RtsCovSet& set, const RtsCovPlan& plan, uint32_t n_taps, const double* in, uint64_t rx_stride, double* part, double* out)
{
    RtsCovArgs a;
    a.in = (const double2*)in; a.rx_stride = rx_stride; a.K = plan.K; a.tiles = plan.tiles; a.set = set;
    a.row_bins = c->cube.params.n_bins; a.parts = plan.parts; a.n_sp = c->cube.params.n_rx; a.n_rx = a.n_sp * n_taps; a.blocks = plan.blocks;
    a.part = (double2*)part; a.out = (double2*)out;
    void (*k)(const RtsCovArgs) = n_taps > 1u ? k_cube_cov<true> : k_cube_cov<false>;
    RTS_HIP(hipFuncSetAttribute((const void*)k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)plan.lds));
    k<<<plan.parts, plan.threads, plan.lds, c->stream>>>(a);
    RTS_HIP(hipGetLastError());
    k_cube_cov_reduce<<<plan.reduce_groups, RTS_ADAPT_REDUCE_THREADS, 0, c->stream>>>(a);
    RTS_HIP(hipGetLastError());
    return RTS_OK;
}

// The solve is tiny next to the covariance (n_rx <= 64): ONE workgroup, correct and deterministic rather than clever.  A / L sits in
// LDS; thread i owns row i of the factor, column by column (the pivot's thread forms it and its square root, a barrier, the rows
// below form their entries, a barrier); then one thread per beam runs rts_adapt.h's substitutions on its own column of the work
// vectors, in passes of RTS_MVDR_THREADS beams.  A failed pivot: every weight NaN, the status word the column + 1 (0: solved).
struct RtsMvdrArgs { const double2* cov; const double2* s; double2* out; uint32_t* status; uint32_t n, n_beams, passes; double loading; };

__global__ void __launch_bounds__(RTS_MVDR_THREADS) k_mvdr(const RtsMvdrArgs a)
{
    extern __shared__ __attribute__((aligned(16))) double2 s_mvdr[];             // L [n][n], then the work vectors [n][RTS_MVDR_THREADS]
    __shared__ uint32_t s_fail; __shared__ double s_ljj;
    const uint32_t t = threadIdx.x, n = a.n;
    double* L = (double*)s_mvdr;
    for (uint32_t e = t; e < n * n; e += RTS_MVDR_THREADS) {
        const uint32_t i = e / n, j = e % n;
        if (j > i) continue;
        double2 v = a.cov[e];
        if (i == j) v.x = v.x + a.loading;
        s_mvdr[e] = v;
    }
    if (t == 0u) s_fail = 0u;
    __syncthreads();
    uint32_t fail = 0u;
    for (uint32_t j = 0; j < n; j++) {
        if (t == j) {
            const double d = rts_mvdr_pivot(L, n, j);
            if (!rts_adapt_pivot_ok(d)) s_fail = j + 1u;
            else { const double ljj = sqrt(d); L[2 * ((size_t)j * n + j)] = ljj; s_ljj = ljj; }
        }
        __syncthreads();
        fail = s_fail;                                                            // (the same word for every thread: they leave together)
        if (fail) break;
        if (t > j && t < n) rts_mvdr_below(L, n, t, j, s_ljj);
        __syncthreads();
    }
    if (t == 0u) *a.status = fail;
    if (fail) {
        const double nan = __builtin_nan("");
        for (uint32_t e = t; e < a.n_beams * n; e += RTS_MVDR_THREADS) a.out[e] = make_double2(nan, nan);
        return;
    }
    double* x = (double*)(s_mvdr + (size_t)n * n + t);
    for (uint32_t pass = 0; pass < a.passes; pass++) {
        const uint32_t b = pass * RTS_MVDR_THREADS + t;
        if (b < a.n_beams) rts_mvdr_beam(L, n, n, (const double*)(a.s + (size_t)b * n), x, RTS_MVDR_THREADS, (double*)(a.out + (size_t)b * n));
    }
}

// cov: [n_rx][n_rx] on the device; steering: the call's rows on the device (rts_cube_array_api.hip uploads them on the stream before this:
// RtsCubeState::adapt.mvdr_s); status: the word this call reports to
int rts_cube_mvdr_device(RtsContext* c, const RtsMvdrPlan& plan, uint32_t n_rx, uint32_t n_beams, double loading, const double* cov, const double* steering, uint32_t* status, double* out)
{
    RtsMvdrArgs a;
    a.cov = (const double2*)cov; a.s = (const double2*)steering; a.out = (double2*)out; a.status = status;
    a.n = n_rx; a.n_beams = n_beams; a.passes = plan.passes; a.loading = loading;
    RTS_HIP(hipFuncSetAttribute((const void*)k_mvdr, hipFuncAttributeMaxDynamicSharedMemorySize, (int)plan.lds));
    k_mvdr<<<1, RTS_MVDR_THREADS, plan.lds, c->stream>>>(a);
    RTS_HIP(hipGetLastError());
    return RTS_OK;
}
