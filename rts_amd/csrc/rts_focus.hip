// rts_focus.hip -- autofocus of the return cube on the device (include/rts_amd.h: rts_cube_align, rts_cube_pga, rts_cube_correct):
//   * range alignment: the rows' envelopes once (k_focus_envelope), per iteration the reference (k_align_ref) and every row's
//     correlation, peak and parabola (k_align_corr) -- IEEE basic operations in rts_focus.h's order: the host evaluator's bits
//   * phase-gradient autofocus: per iteration the gate columns' gradient products summed per tile (k_pga_tile: rotate-on-load,
//     transform, peak, shift-and-window, inverse transform and products in LDS), the tile sums (k_pga_sum_tiles) and per receiver
//     the phase update (k_pga_update)
//   * the correction in place (k_focus_copy_rows, k_focus_correct)
// All on the handle's stream, none waits on the host.  The arithmetic and the launch plans are rts_focus.h.
//
// k_pga_tile's LDS: two column sets x[row][b], y[row][b] of 16-byte elements, row stride BT, and the twiddle table: rts_stft.hip's
// layout (b fastest; the load, the stages with 2^(s-1) * BT >= 16 and the products touch runs of at least 16 consecutive elements per
// 16 lanes: conflict-free for 128-bit accesses; the first 4 - log2 BT stages are 2-way).  The shift-and-window step reads row
// (k + k*[b]) mod N of column b -- k* differs from column to column, so its BT-element runs break up (up to BT-way on one step of
// 2 log2 N + 4) -- and writes bit-reversed rows like the load.  At N = 4096 (BT = 1) the two sets and the table fill the 160 KiB
// exactly: the peak search's scratch lives in y, which is idle until the shift.
#include <hip/hip_runtime.h>
#include "rts_internal.h"
#include "rts_focus.h"

// --------------------------------------------------------------------------- range alignment
// env[rx][j][bin] = |cube[rx][first_pulse + j][bin]|
__global__ void __launch_bounds__(RTS_FOCUS_THREADS) k_focus_envelope(const double2* __restrict__ cube, double* __restrict__ env, uint32_t n_rx, uint32_t n_pulses_cube, uint32_t n_bins,
                                                                       uint32_t first_pulse, uint32_t P)
{
    const size_t per_rx = (size_t)P * n_bins, total = per_rx * n_rx;
    for (size_t i = (size_t)blockIdx.x * RTS_FOCUS_THREADS + threadIdx.x; i < total; i += (size_t)gridDim.x * RTS_FOCUS_THREADS) {
        const size_t r = i / per_rx, k = i - r * per_rx;
        const double2 v = cube[(r * n_pulses_cube + first_pulse) * n_bins + k];
        env[i] = rts_focus_envelope(v.x, v.y);
    }
}

// ref[rx][g], g a gate bin: blockIdx.x = tile of 256 gate bins, blockIdx.y = receiver
__global__ void __launch_bounds__(RTS_FOCUS_THREADS) k_align_ref(const double* __restrict__ env, const double* __restrict__ S, double* __restrict__ ref, uint32_t P, uint32_t n_bins,
                                                                  uint32_t first_bin, uint32_t G)
{
    const uint32_t r = blockIdx.y, g = blockIdx.x * RTS_FOCUS_THREADS + threadIdx.x;
    if (g >= G) return;
    ref[(size_t)r * G + g] = rts_align_ref_at(env + (size_t)r * P * n_bins, S + (size_t)r * P, P, n_bins, first_bin + g);
}

// S[rx][j]: blockIdx.x = pulse, blockIdx.y = receiver.  Item (block bl of the pass, lag li), lag fastest: neighbouring lanes read
// neighbouring envelopes.  Lane li < n_lags adds its lag's block sums left to right across the passes; lane 0 picks the shift.
__global__ void __launch_bounds__(RTS_FOCUS_THREADS) k_align_corr(const double* __restrict__ env, const double* __restrict__ ref, double* __restrict__ S, uint32_t P, uint32_t n_bins,
                                                                   uint32_t first_bin, uint32_t G, uint32_t L, uint32_t flags, uint32_t n_blocks, uint32_t bpp)
{
    __shared__ double s_sum[RTS_ALIGN_LDS_SUMS];
    __shared__ double s_C[2u * RTS_ALIGN_MAX_LAG + 1u];
    const uint32_t t = threadIdx.x, j = blockIdx.x, r = blockIdx.y, n_lags = 2u * L + 1u;
    const double* env_row = env + ((size_t)r * P + j) * n_bins;
    const double* ref_rx = ref + (size_t)r * G;
    double c = 0.0;
    for (uint32_t b0 = 0; b0 < n_blocks; b0 += bpp) {
        const uint32_t nbp = n_blocks - b0 < bpp ? n_blocks - b0 : bpp;
        for (uint32_t item = t; item < nbp * n_lags; item += RTS_FOCUS_THREADS) {
            const uint32_t bl = item / n_lags, li = item - bl * n_lags;
            const uint32_t g0 = (b0 + bl) * RTS_ALIGN_BIN_BLOCK, g1 = G - g0 < RTS_ALIGN_BIN_BLOCK ? G : g0 + RTS_ALIGN_BIN_BLOCK;
            s_sum[item] = rts_align_block(ref_rx, env_row, n_bins, first_bin, g0, g1, (int32_t)li - (int32_t)L);
        }
        __syncthreads();
        if (t < n_lags) for (uint32_t bl = 0; bl < nbp; bl++) c += s_sum[bl * n_lags + t];
        __syncthreads();
    }
    if (t < n_lags) s_C[t] = c;
    __syncthreads();
    if (t == 0) S[(size_t)r * P + j] = rts_align_pick(s_C, L, flags);
}

static unsigned rts_focus_stride_grid(size_t total) { const size_t b = (total + RTS_FOCUS_THREADS - 1u) / RTS_FOCUS_THREADS; return (unsigned)(b < 1048576u ? (b ? b : 1u) : 1048576u); }

int rts_cube_align_device(RtsContext* c, const RtsAlignParams& p, const RtsAlignPlan& plan, double* out)
{
    const RtsCubeParams& q = c->cube.params;
    RTS_HIP(c->cube.focus.d_env.reserve(plan.env_doubles));
    RTS_HIP(c->cube.focus.d_ref.reserve(plan.ref_doubles));
    double* env = c->cube.focus.d_env.p; double* ref = c->cube.focus.d_ref.p;
    RTS_HIP(hipMemsetAsync(out, 0, sizeof(double) * plan.out_doubles, c->stream));
    k_focus_envelope<<<rts_focus_stride_grid(plan.env_doubles), RTS_FOCUS_THREADS, 0, c->stream>>>((const double2*)c->cube.p, env, q.n_rx, q.n_pulses, q.n_bins, p.first_pulse, p.n_pulses);
    RTS_HIP(hipGetLastError());
    const dim3 grid_ref((plan.n_gate + RTS_FOCUS_THREADS - 1u) / RTS_FOCUS_THREADS, q.n_rx), grid_corr(p.n_pulses, q.n_rx);
    for (uint32_t it = 0; it < p.n_iters; it++) {
        k_align_ref<<<grid_ref, RTS_FOCUS_THREADS, 0, c->stream>>>(env, out, ref, p.n_pulses, q.n_bins, p.first_bin, plan.n_gate);
        RTS_HIP(hipGetLastError());
        k_align_corr<<<grid_corr, RTS_FOCUS_THREADS, 0, c->stream>>>(env, ref, out, p.n_pulses, q.n_bins, p.first_bin, plan.n_gate, p.max_lag, p.flags, plan.n_blocks, plan.blocks_per_pass);
        RTS_HIP(hipGetLastError());
    }
    return RTS_OK;
}

// --------------------------------------------------------------------------- phase-gradient autofocus
struct RtsPgaArgs {
    const double2* cube; uint32_t n_pulses_cube, n_bins_cube;
    uint32_t first_pulse, first_bin, n_gate, N, logN, BT, passes, tiles, W;
    const double2* rot;               // [n_rx][N] (cos, sin)(2 pi phi)
    double2* partial;                 // [n_rx][tiles][N]
};

// the stages of rts_stft.h's tree on a column set in LDS (k_cube_stft's loop)
static __device__ __forceinline__ void rts_pga_stages(double2* x, const double2* tw, uint32_t N, uint32_t logN, uint32_t BT, uint32_t t)
{
    const uint32_t half = (N / 2u) * BT;
    for (uint32_t s = 1; s <= logN; s++) {
        for (uint32_t idx = t; idx < half; idx += RTS_FOCUS_THREADS) {
            const uint32_t j = idx / BT, b = idx - j * BT;
            uint32_t i0, i1, k; rts_stft_pair(j, s, N, &i0, &i1, &k);
            const double2 w = tw[k];
            double2 u = x[(size_t)i0 * BT + b], v = x[(size_t)i1 * BT + b];
            rts_stft_butterfly(w.x, w.y, &u.x, &u.y, &v.x, &v.y);
            x[(size_t)i0 * BT + b] = u; x[(size_t)i1 * BT + b] = v;
        }
        __syncthreads();
    }
}

// blockIdx.x = tile of RTS_PGA_BIN_TILE gate bins, blockIdx.y = receiver.  A pass takes BT gate bins from g0 = (tile * passes + pass) * BT.
// Element idx = row * BT + b has the same thread in every step; 256 is a multiple of BT, so a thread's elements share their column.
__global__ void __launch_bounds__(RTS_FOCUS_THREADS) k_pga_tile(const RtsPgaArgs a)
{
    extern __shared__ __attribute__((aligned(16))) double2 s_pga[];              // x [N][BT], y [N][BT], then [N/2] twiddles
    const uint32_t t = threadIdx.x, r = blockIdx.y, tile = blockIdx.x;
    const uint32_t N = a.N, BT = a.BT, total = N * BT;
    double2* x = s_pga; double2* y = s_pga + total; double2* tw = s_pga + 2 * (size_t)total;
    for (uint32_t k = t; k < N / 2; k += RTS_FOCUS_THREADS) { double sn, cs; rts_stft_twiddle(k, N, &cs, &sn); tw[k] = make_double2(cs, sn); }
    const double2* rows = a.cube + ((size_t)r * a.n_pulses_cube + a.first_pulse) * a.n_bins_cube + a.first_bin;
    const double2* rot = a.rot + (size_t)r * N;
    double2* part = a.partial + ((size_t)r * a.tiles + tile) * N;
    const uint32_t cnt = total < RTS_FOCUS_THREADS ? total : RTS_FOCUS_THREADS;      // the threads that hold elements
    double* s_v = (double*)y; uint32_t* s_k = (uint32_t*)(s_v + cnt);            // the peak search's candidates (y is idle until the shift)
    for (uint32_t pass = 0; pass < a.passes; pass++) {
        const uint32_t g0 = (tile * a.passes + pass) * BT;
        if (g0 >= a.n_gate) break;                                                // (uniform over the workgroup)
        const uint32_t nb = a.n_gate - g0 < BT ? a.n_gate - g0 : BT;
        if (pass) __syncthreads();                                                // (the previous pass's products have been summed)
        for (uint32_t idx = t; idx < total; idx += RTS_FOCUS_THREADS) {
            const uint32_t p = idx / BT, b = idx - p * BT;
            double2 v = make_double2(0.0, 0.0);
            if (b < nb) { v = rows[(size_t)p * a.n_bins_cube + g0 + b]; const double2 w = rot[p]; rts_focus_unrotate(w.x, w.y, &v.x, &v.y); }
            x[(size_t)rts_stft_bitrev(p, a.logN) * BT + b] = v;
        }
        __syncthreads();
        rts_pga_stages(x, tw, N, a.logN, BT, t);
        // k*[b]: the first maximum of the column's power.  A thread's own elements in ascending row, then its column's candidates
        uint32_t bk = 0xffffffffu; double bv = 0.0;
        for (uint32_t idx = t; idx < total; idx += RTS_FOCUS_THREADS) {
            const double2 v = x[idx]; const double pw = rts_stft_power(v.x, v.y);
            if (bk == 0xffffffffu || pw > bv) { bv = pw; bk = idx / BT; }
        }
        if (t < cnt) { s_v[t] = bv; s_k[t] = bk; }
        __syncthreads();
        uint32_t ks = 0xffffffffu; double kv = 0.0;
        for (uint32_t u = t % BT; u < cnt; u += BT) {
            const double v = s_v[u]; const uint32_t k = s_k[u];
            if (ks == 0xffffffffu || v > kv || (v == kv && k < ks)) { kv = v; ks = k; }
        }
        ks &= N - 1u;
        __syncthreads();                                                          // (the candidates have been read: y may be written)
        for (uint32_t idx = t; idx < total; idx += RTS_FOCUS_THREADS) {
            const uint32_t k = idx / BT, b = idx - k * BT;
            double2 v = make_double2(0.0, 0.0);
            if (rts_pga_keep(k, N, a.W)) { const double2 u = x[(size_t)((k + ks) & (N - 1u)) * BT + b]; v = make_double2(u.x, -u.y); }
            y[(size_t)rts_stft_bitrev(k, a.logN) * BT + b] = v;
        }
        __syncthreads();
        rts_pga_stages(y, tw, N, a.logN, BT, t);
        for (uint32_t idx = t; idx < total; idx += RTS_FOCUS_THREADS) {
            double2 pr = make_double2(0.0, 0.0);
            if (idx >= BT) { const double2 g = y[idx], h = y[idx - BT]; rts_pga_product(g.x, -g.y, h.x, -h.y, &pr.x, &pr.y); }
            x[idx] = pr;
        }
        __syncthreads();
        for (uint32_t p = t; p < N; p += RTS_FOCUS_THREADS) {
            double2 s = pass ? part[p] : make_double2(0.0, 0.0);                  // (this thread's own store of the previous pass)
            for (uint32_t b = 0; b < nb; b++) { const double2 v = x[(size_t)p * BT + b]; s.x += v.x; s.y += v.y; }
            part[p] = s;
        }
    }
}

// the tile sums of one (receiver, pulse) added in ascending tile order, the first one the start value
__global__ void __launch_bounds__(256) k_pga_sum_tiles(const double2* __restrict__ partial, double2* __restrict__ A, size_t n_rows, uint32_t N, uint32_t tiles)
{
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n_rows) return;
    const size_t r = i / N, p = i - r * N;
    const double2* src = partial + r * tiles * N + p;
    double2 s = src[0];
    for (uint32_t tl = 1; tl < tiles; tl++) { const double2 v = src[(size_t)tl * N]; s.x += v.x; s.y += v.y; }
    A[i] = s;
}

// phi = 0 and its rotations
__global__ void __launch_bounds__(256) k_pga_init(double* __restrict__ phi, double2* __restrict__ rot, size_t n)
{
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    phi[i] = 0.0;
    double cs, sn; rts_focus_rotation(0.0, &cs, &sn);
    rot[i] = make_double2(cs, sn);
}

// one workgroup per receiver: the steps from the summed products, their running sum less its mean and line (lane 0, left to
// right: the evaluator's order), the phase and its rotations for the next iteration, the iteration's rms
__global__ void __launch_bounds__(RTS_FOCUS_THREADS) k_pga_update(const double2* __restrict__ A, double* __restrict__ phi, double2* __restrict__ rot, double* __restrict__ rms,
                                                                   uint32_t N, uint32_t n_iters, uint32_t it)
{
    __shared__ double s_psi[RTS_PGA_MAX_PULSES];
    const uint32_t t = threadIdx.x, r = blockIdx.x;
    for (uint32_t p = t; p < N; p += RTS_FOCUS_THREADS) { const double2 v = A[(size_t)r * N + p]; s_psi[p] = p ? rts_pga_delta(v.x, v.y) : 0.0; }
    __syncthreads();
    if (t == 0) rms[(size_t)r * n_iters + it] = rts_pga_update(N, s_psi);
    __syncthreads();
    for (uint32_t p = t; p < N; p += RTS_FOCUS_THREADS) {
        const double v = phi[(size_t)r * N + p] + s_psi[p];
        phi[(size_t)r * N + p] = v;
        double cs, sn; rts_focus_rotation(v, &cs, &sn);
        rot[(size_t)r * N + p] = make_double2(cs, sn);
    }
}

// out: phase [n_rx][N], then rms [n_rx][n_iters]
int rts_cube_pga_device(RtsContext* c, const RtsPgaParams& p, const RtsPgaPlan& plan, double* out)
{
    const RtsCubeParams& q = c->cube.params;
    const uint32_t N = p.n_pulses;
    const size_t n_rows = (size_t)q.n_rx * N;
    RTS_HIP(c->cube.focus.d_pga_part.reserve(plan.partial_doubles));
    RTS_HIP(c->cube.focus.d_pga_sum.reserve(2 * n_rows));
    RTS_HIP(c->cube.focus.d_pga_rot.reserve(2 * n_rows));
    double* phi = out; double* rms = out + n_rows;
    double2* rot = (double2*)c->cube.focus.d_pga_rot.p;
    RtsPgaArgs a;
    a.cube = (const double2*)c->cube.p; a.n_pulses_cube = q.n_pulses; a.n_bins_cube = q.n_bins;
    a.first_pulse = p.first_pulse; a.first_bin = p.first_bin; a.n_gate = plan.n_gate; a.N = N; a.logN = plan.logN;
    a.BT = plan.BT; a.passes = plan.passes; a.tiles = plan.tiles; a.W = plan.window0;
    a.rot = rot; a.partial = (double2*)c->cube.focus.d_pga_part.p;
    const double2* A = plan.tiles > 1u ? (const double2*)c->cube.focus.d_pga_sum.p : a.partial;
    RTS_HIP(hipFuncSetAttribute((const void*)k_pga_tile, hipFuncAttributeMaxDynamicSharedMemorySize, (int)plan.lds));
    k_pga_init<<<(unsigned)((n_rows + 255) / 256), 256, 0, c->stream>>>(phi, rot, n_rows);
    RTS_HIP(hipGetLastError());
    const dim3 grid(plan.tiles, q.n_rx);
    for (uint32_t it = 0; it < p.n_iters; it++) {
        k_pga_tile<<<grid, RTS_FOCUS_THREADS, plan.lds, c->stream>>>(a);
        RTS_HIP(hipGetLastError());
        if (plan.tiles > 1u) {
            k_pga_sum_tiles<<<(unsigned)((n_rows + 255) / 256), 256, 0, c->stream>>>(a.partial, (double2*)c->cube.focus.d_pga_sum.p, n_rows, N, plan.tiles);
            RTS_HIP(hipGetLastError());
        }
        k_pga_update<<<q.n_rx, RTS_FOCUS_THREADS, 0, c->stream>>>(A, phi, rot, rms, N, p.n_iters, it);
        RTS_HIP(hipGetLastError());
        a.W = rts_pga_next_window(a.W, plan.window_min);
    }
    return RTS_OK;
}

// --------------------------------------------------------------------------- the correction
// scratch[rx][j][bin] = cube[rx][first_pulse + j][bin]
__global__ void __launch_bounds__(RTS_FOCUS_THREADS) k_focus_copy_rows(const double2* __restrict__ cube, double2* __restrict__ scratch, uint32_t n_rx, uint32_t n_pulses_cube, uint32_t n_bins,
                                                                        uint32_t first_pulse, uint32_t P)
{
    const size_t per_rx = (size_t)P * n_bins, total = per_rx * n_rx;
    for (size_t i = (size_t)blockIdx.x * RTS_FOCUS_THREADS + threadIdx.x; i < total; i += (size_t)gridDim.x * RTS_FOCUS_THREADS) {
        const size_t r = i / per_rx, k = i - r * per_rx;
        scratch[i] = cube[(r * n_pulses_cube + first_pulse) * n_bins + k];
    }
}

struct RtsCorrectArgs {
    double* cube; const double* rows;         // rows: the scratch copy [n_rx][P][n_bins] (with shifts), else unused
    uint32_t n_pulses_cube, n_bins, first_pulse, P, taps, tiles;
    const double* shifts; const double* phase;      // [n_rx][P] (device) or NULL
};

// blockIdx.x = row * tiles + tile of 256 bins, blockIdx.y = receiver.  With shifts the thread reads the row's copy; without, only
// the element it writes.
__global__ void __launch_bounds__(RTS_FOCUS_THREADS) k_focus_correct(const RtsCorrectArgs a)
{
    const uint32_t r = blockIdx.y, j = blockIdx.x / a.tiles, tile = blockIdx.x - j * a.tiles, n = tile * RTS_FOCUS_THREADS + threadIdx.x;
    if (n >= a.n_bins) return;
    double* row = a.cube + 2 * (((size_t)r * a.n_pulses_cube + a.first_pulse + j) * a.n_bins);
    const double* src = a.shifts ? a.rows + 2 * (((size_t)r * a.P + j) * a.n_bins) : row;
    const RtsImageInterp ip = rts_image_interp_setup(a.taps);
    double cs = 1.0, sn = 0.0;
    if (a.phase) rts_focus_rotation(a.phase[(size_t)r * a.P + j], &cs, &sn);
    const double S = a.shifts ? a.shifts[(size_t)r * a.P + j] : 0.0;
    double re, im;
    rts_correct_sample(src, a.n_bins, ip, n, a.shifts != nullptr, S, a.phase != nullptr, cs, sn, &re, &im);
    row[2 * (size_t)n] = re; row[2 * (size_t)n + 1] = im;
}

int rts_cube_correct_device(RtsContext* c, const RtsCorrectParams& p, const RtsCorrectPlan& plan, const double* shifts, const double* phase)
{
    const RtsCubeParams& q = c->cube.params;
    RtsCorrectArgs a;
    a.cube = c->cube.p; a.rows = nullptr;
    a.n_pulses_cube = q.n_pulses; a.n_bins = q.n_bins; a.first_pulse = p.first_pulse; a.P = p.n_pulses; a.taps = p.taps; a.tiles = plan.tiles;
    a.shifts = shifts; a.phase = phase;
    if (shifts) {
        RTS_HIP(c->cube.focus.d_rows.reserve(plan.scratch_doubles));
        a.rows = c->cube.focus.d_rows.p;
        k_focus_copy_rows<<<rts_focus_stride_grid(plan.scratch_doubles / 2), RTS_FOCUS_THREADS, 0, c->stream>>>((const double2*)c->cube.p, (double2*)c->cube.focus.d_rows.p, q.n_rx, q.n_pulses, q.n_bins,
                                                                                                                 p.first_pulse, p.n_pulses);
        RTS_HIP(hipGetLastError());
    }
    const dim3 grid(p.n_pulses * plan.tiles, q.n_rx);
    k_focus_correct<<<grid, RTS_FOCUS_THREADS, 0, c->stream>>>(a);
    RTS_HIP(hipGetLastError());
    return RTS_OK;
}
