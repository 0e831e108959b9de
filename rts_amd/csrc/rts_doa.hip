// rts_doa.hip -- direction finding on the device (include/rts_amd.h: rts_cube_eig, rts_cube_doa_scan): k_eig, k_doa_scan.
// The trees and the plans of the launches are rts_doa.h, shared with the host evaluators.
#include <hip/hip_runtime.h>
#include "rts_internal.h"
#include "rts_doa.h"

// The solve is tiny (n <= 64): ONE workgroup, correct and deterministic rather than clever.  X and V sit in LDS, row-major: the
// lanes of a round hold different columns, so at one time they read 16-byte elements of ONE row, apart by their columns -- no stride
// of a power of two.  RTS_EIG_LANES = 8 neighbouring threads own a slot of every round (rts_doa.h: rts_eig_pair_of).  Each of them
// forms the pair's three sums in full (the eight read one address at a time: a broadcast) and so the same rotation; after a barrier
// they rotate every eighth row of X and V each; a second barrier ends the round.  "Did anything rotate" is a word in LDS that every
// rotating thread sets and every thread reads after the sweep's last barrier.  Threads t < n own column t of the sweep's norms,
// of the eigenvalues and of the sort.
// What bounds it, measured (profiles/doa_bench.txt; 64 x 64, 9 sweeps and the one that finds nothing to rotate, 630 rounds): with a
// thread per pair on one wave a call took 12.3 ms, 41 000 cycles a round; reading the rows in batches of eight before using them
// 9.2 ms -- so not LDS latency alone: a pair is 16 f64 instructions per row for the sums and 40 for the two rotations, 3 584 for 64
// rows, 14 336 cycles of ONE SIMD's issue for the only wave.  Dealing the rotation's rows to eight lanes puts four waves on four
// SIMDs: 5.2 ms, 17 000 cycles a round for 1 344 instructions a lane, of which the sums, which every lane repeats, are three
// quarters; the rest is the chain of four square roots and six divisions and the two barriers (no counters taken).  Splitting the
// sums too would be a change of the tree (a fixed partition of the rows), not taken here.
struct RtsEigArgs { const double2* cov; double* values; double2* vectors; uint32_t* status; uint32_t n, rounds, slots; };

__global__ void __launch_bounds__(RTS_EIG_THREADS) k_eig(const RtsEigArgs a)
{
    extern __shared__ __attribute__((aligned(16))) double2 s_eig[];               // X [n][n], then V [n][n]
    __shared__ double s_col[RTS_BEAM_MAX_RX];                                     // the sweep's column norms; the eigenvalues
    __shared__ uint32_t s_bad, s_rot;
    const uint32_t t = threadIdx.x, n = a.n, slot = t / RTS_EIG_LANES, lane = t % RTS_EIG_LANES;
    double* X = (double*)s_eig; double* V = (double*)(s_eig + (size_t)n * n);
    if (t == 0u) s_bad = 0u;
    __syncthreads();
    for (uint32_t e = t; e < n * n; e += RTS_EIG_THREADS) {
        const uint32_t i = e / n, j = e % n;
        s_eig[(size_t)n * n + e] = make_double2(i == j ? 1.0 : 0.0, 0.0);
        if (j > i) continue;
        const double2 v = a.cov[e];
        if (i == j) { if (!rts_eig_finite(v.x)) s_bad = 1u; s_eig[e] = make_double2(v.x, 0.0); continue; }
        if (!rts_eig_finite(v.x) || !rts_eig_finite(v.y)) s_bad = 1u;
        s_eig[e] = v; s_eig[(size_t)j * n + i] = make_double2(v.x, -v.y);
    }
    __syncthreads();
    uint32_t status = s_bad ? 2u : 0u, sweeps = 0u;
    while (!status) {
        if (t < n) s_col[t] = rts_eig_norm2(X, n, n, t);
        if (t == 0u) s_rot = 0u;
        __syncthreads();
        double m2 = s_col[0];
        for (uint32_t col = 1; col < n; col++) { const double v = s_col[col]; if (v > m2) m2 = v; }
        const double floor2 = RTS_EIG_EPS2 * m2;
        for (uint32_t r = 0; r < a.rounds; r++) {
            uint32_t p = 0u, q = n; double c = 0.0, sr = 0.0, si = 0.0;
            if (slot < a.slots) rts_eig_pair_of(n, r, slot, &p, &q);
            const bool rotate = q < n && rts_eig_decide(X, n, n, p, q, floor2, &c, &sr, &si);
            __syncthreads();                                                      // (every lane of the pair has read the columns it is about to change)
            if (rotate) { rts_eig_rotate(X, V, n, n, p, q, c, sr, si, lane, RTS_EIG_LANES); s_rot = 1u; }
            __syncthreads();
        }
        const uint32_t rotated = s_rot;                                           // (the same word for every thread: they leave together)
        __syncthreads();                                                          // (read by all before the next sweep clears it)
        if (!rotated) break;
        sweeps++;
        if (sweeps == RTS_EIG_MAX_SWEEPS) status = 1u;
    }
    if (t == 0u) *a.status = status;
    if (status) {
        const double nan = __builtin_nan("");
        for (uint32_t e = t; e < n * n; e += RTS_EIG_THREADS) a.vectors[e] = make_double2(nan, nan);
        if (t < n) a.values[t] = nan;
        return;
    }
    if (t < n) s_col[t] = rts_eig_value(X, V, n, n, t);
    __syncthreads();
    if (t >= n) return;
    const uint32_t k = rts_eig_rank(s_col, n, t);
    a.values[k] = s_col[t];
    for (uint32_t i = 0; i < n; i++) a.vectors[(size_t)k * n + i] = s_eig[(size_t)n * n + (size_t)i * n + t];
}

// cov: [n][n] on the device; status: the word this call reports to
int rts_cube_eig_device(RtsContext* c, const RtsEigPlan& plan, uint32_t n, const double* cov, uint32_t* status, double* values, double* vectors)
{
    RtsEigArgs a;
    a.cov = (const double2*)cov; a.values = values; a.vectors = (double2*)vectors; a.status = status;
    a.n = n; a.rounds = plan.rounds; a.slots = plan.slots;
    RTS_HIP(hipFuncSetAttribute((const void*)k_eig, hipFuncAttributeMaxDynamicSharedMemorySize, (int)plan.lds));
    k_eig<<<1, RTS_EIG_THREADS, plan.lds, c->stream>>>(a);
    RTS_HIP(hipGetLastError());
    return RTS_OK;
}

// The scan is the beamformer's skinny complex f64 product with the beams folded away: q[dir] = sum_k g_k |sum_rx conj(v_k[rx]) a[rx][dir]|^2,
// per direction 16 n bytes in and 8 bytes out against 8 m n f64 operations -- bound by f64 issue from a few vectors on.  Thread t of
// workgroup g owns direction 256 g + t; the table is element-major, so every global access of a wave is 64 consecutive 16-byte
// elements.  The vectors [m][n] and g [m] are staged once per workgroup in LDS (at most 64 KiB + 512 B); every lane of a wave reads
// the same vector element at the same time, one 16-byte broadcast read per term and no bank conflict.
// Registers: the direction's elements of one tile (RTS_DOA_RX_TILE complex128 = 32 VGPRs) and the running y of one vector tile
// (RTS_DOA_VEC_TILE complex128 = 64 VGPRs); q lives across the vector tiles and takes g_k p_k in ascending k.  Up to one element
// tile the direction is loaded ONCE; with more, each vector tile walks the element tiles in ascending order and reads them again
// (1 / RTS_DOA_VEC_TILE of a re-read per vector).  A sum's order is the header's whatever the tiles.
// 114 VGPRs, no scratch (-Rpass-analysis=kernel-resource-usage: VGPRs 114, ScratchSize 0, 4 waves per SIMD).
struct RtsDoaArgs {
    const double2* a;                 // [n][n_dirs]
    const double2* v;                 // the first of the m vectors, [m][n] (device)
    const double* g;                  // [m] (device)
    uint64_t n_dirs;
    uint32_t n, m, rx_tiles, inverse;
    double* out;
};

__global__ void __launch_bounds__(RTS_DOA_THREADS) k_doa_scan(const RtsDoaArgs a)
{
    extern __shared__ __attribute__((aligned(16))) double2 s_doa_v[];            // [m][n], then g [m]
    const uint32_t t = threadIdx.x, nv = a.m * a.n;
    double* s_g = (double*)(s_doa_v + nv);
    for (uint32_t i = t; i < nv; i += RTS_DOA_THREADS) s_doa_v[i] = a.v[i];
    for (uint32_t i = t; i < a.m; i += RTS_DOA_THREADS) s_g[i] = a.g[i];
    __syncthreads();
    const uint64_t d = (uint64_t)blockIdx.x * RTS_DOA_THREADS + t;
    if (d >= a.n_dirs) return;
    const double2* __restrict__ in = a.a + d;
    double2 z[RTS_DOA_RX_TILE];
    const bool one = a.rx_tiles == 1u;
    if (one) {
#pragma unroll
        for (uint32_t r = 0; r < RTS_DOA_RX_TILE; r++) z[r] = r < a.n ? in[(uint64_t)r * a.n_dirs] : make_double2(0.0, 0.0);
    }
    double q = 0.0;
    for (uint32_t k0 = 0; k0 < a.m; k0 += RTS_DOA_VEC_TILE) {
        const uint32_t nk = a.m - k0 < RTS_DOA_VEC_TILE ? a.m - k0 : RTS_DOA_VEC_TILE;
        double2 y[RTS_DOA_VEC_TILE];
#pragma unroll
        for (uint32_t j = 0; j < RTS_DOA_VEC_TILE; j++) y[j] = make_double2(0.0, 0.0);
        for (uint32_t r0 = 0; r0 < a.n; r0 += RTS_DOA_RX_TILE) {
            const uint32_t live = a.n - r0 < RTS_DOA_RX_TILE ? a.n - r0 : RTS_DOA_RX_TILE;
            if (!one) {
#pragma unroll
                for (uint32_t r = 0; r < RTS_DOA_RX_TILE; r++) z[r] = r < live ? in[(uint64_t)(r0 + r) * a.n_dirs] : make_double2(0.0, 0.0);
            }
#pragma unroll
            for (uint32_t r = 0; r < RTS_DOA_RX_TILE; r++) {
                if (r < live) {
#pragma unroll
                    for (uint32_t j = 0; j < RTS_DOA_VEC_TILE; j++) {
                        const uint32_t k = k0 + (j < nk ? j : nk - 1u);      // (past the last vector: its elements again, a sum nobody uses)
                        const double2 w = s_doa_v[k * a.n + r0 + r];
                        rts_beam_add(r0 + r == 0u, w.x, w.y, z[r].x, z[r].y, &y[j].x, &y[j].y);
                    }
                }
            }
        }
#pragma unroll
        for (uint32_t j = 0; j < RTS_DOA_VEC_TILE; j++) {
            if (j < nk) {
                const double gp = s_g[k0 + j] * rts_beam_power(y[j].x, y[j].y);
                if (k0 + j == 0u) q = gp; else q += gp;
            }
        }
    }
    a.out[d] = a.inverse ? 1.0 / q : q;
}

// steering: [n][n_dirs] on the device; vectors: the first of the m rows of a table [.][n] on the device; g: [m] on the device
// (rts_cube_array_api.hip uploads it on the stream before this: RtsCubeState::doa.g)
int rts_cube_doa_scan_device(RtsContext* c, const RtsDoaScanPlan& plan, uint32_t n, uint32_t m, uint64_t n_dirs, uint32_t flags, const double* steering, const double* vectors,
                             const double* g, double* out)
{
    RtsDoaArgs a;
    a.a = (const double2*)steering; a.v = (const double2*)vectors; a.g = g; a.n_dirs = n_dirs;
    a.n = n; a.m = m; a.rx_tiles = plan.rx_tiles; a.inverse = (flags & RTS_DOA_INVERSE) ? 1u : 0u; a.out = out;
    RTS_HIP(hipFuncSetAttribute((const void*)k_doa_scan, hipFuncAttributeMaxDynamicSharedMemorySize, (int)plan.lds));
    k_doa_scan<<<plan.groups, RTS_DOA_THREADS, plan.lds, c->stream>>>(a);
    RTS_HIP(hipGetLastError());
    return RTS_OK;
}
