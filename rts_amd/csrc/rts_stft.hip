// rts_stft.hip -- the slow-time transforms of the return cube on the device (include/rts_amd.h: rts_cube_doppler, rts_cube_spectrogram):
//   * the Doppler map: every pulse of a range bin, zero padded (k_cube_doppler)
//   * the tapered spectrogram: frames of a gate of bins (k_cube_stft, k_stft_sum_tiles)
// f64 butterflies in LDS, no MFMA: a workgroup holds a tile's N x BT complex128 columns and the twiddle table in LDS; the tree and
// the plans of the launches are rts_stft.h, shared with the host evaluators, so the two kernels' bins agree bit for bit.
//
// LDS layout: column set x[row][b], 16-byte elements, row stride BT (no padding: at n_fft 4096 the spectrogram's two columns and the
// table fill the 160 KiB exactly).  A thread owns element idx = row * BT + b with b fastest, so the load, every stage with
// 2^(s-1) * BT >= 16 and the store touch runs of at least 16 consecutive 16-byte elements per 16 lanes: conflict-free for the 128-bit
// LDS accesses, whose 16-lane groups cover 256 contiguous bytes.  Stage 1 at BT = 8 (and the first 4 - log2 BT stages below that)
// alternates BT-element runs of rows i0 and skips those of i1, which lands two runs of a lane group on the same banks (2-way); that
// is one stage of log2 N.
#include <hip/hip_runtime.h>
#include "rts_internal.h"
#include "rts_stft.h"

// --------------------------------------------------------------------------- the Doppler map
// out[rx][k][bin] = sum_{p < n_pulses} cube[rx][p][bin] e^{-2 pi j k p / N}, N a power of two >= n_pulses (zero padded).
// One block per (receiver, tile of BT consecutive range bins; rts_stft.h: rts_doppler_plan): every stage's N/2 x BT butterflies are
// dealt to the block's threads; rows of BT x 16 bytes are contiguous in the cube, so loads and stores are BT-bin segments.  A
// 1024-point f64 transform per (receiver, bin) is 5 120 butterflies; the whole C3 interval (4 x 1024 columns) is ~20 Mflop.
__global__ void __launch_bounds__(256) k_cube_doppler(const double* __restrict__ cube, double* __restrict__ out, uint32_t n_pulses, uint32_t n_bins, uint32_t N, uint32_t logN, uint32_t BT)
{
    extern __shared__ __attribute__((aligned(16))) double s_fft[];               // [N][BT] complex, then [N/2] complex twiddles
    double* x = s_fft; double* tw = s_fft + 2 * (size_t)N * BT;
    const uint32_t rx = blockIdx.y, bin0 = blockIdx.x * BT, t = threadIdx.x;
    for (uint32_t k = t; k < N / 2; k += blockDim.x) rts_stft_twiddle(k, N, &tw[2 * k], &tw[2 * k + 1]);
    for (uint32_t idx = t; idx < N * BT; idx += blockDim.x) {
        const uint32_t p = idx / BT, b = idx - p * BT, bin = bin0 + b;
        double re = 0.0, im = 0.0;
        if (p < n_pulses && bin < n_bins) { const double* src = cube + 2 * (((size_t)rx * n_pulses + p) * n_bins + bin); re = src[0]; im = src[1]; }
        const uint32_t pr = rts_stft_bitrev(p, logN);
        x[2 * ((size_t)pr * BT + b)] = re; x[2 * ((size_t)pr * BT + b) + 1] = im;
    }
    __syncthreads();
    for (uint32_t s = 1; s <= logN; s++) {
        for (uint32_t idx = t; idx < (N / 2) * BT; idx += blockDim.x) {
            const uint32_t j = idx / BT, b = idx - j * BT;
            __builtin_assume(j < 0x80000000u);       // (j < N / 2.  Said because the compiler bounds rts_stft_pair's j by its callers in this unit, and k_cube_stft's j has this bound)
            uint32_t i0, i1, k; rts_stft_pair(j, s, N, &i0, &i1, &k);
            double* a0 = x + 2 * ((size_t)i0 * BT + b); double* a1 = x + 2 * ((size_t)i1 * BT + b);
            rts_stft_butterfly(tw[2 * k], tw[2 * k + 1], &a0[0], &a0[1], &a1[0], &a1[1]);
        }
        __syncthreads();
    }
    for (uint32_t idx = t; idx < N * BT; idx += blockDim.x) {
        const uint32_t k = idx / BT, b = idx - k * BT, bin = bin0 + b;
        if (bin < n_bins) { double* dst = out + 2 * (((size_t)rx * N + k) * n_bins + bin); dst[0] = x[2 * ((size_t)k * BT + b)]; dst[1] = x[2 * ((size_t)k * BT + b) + 1]; }
    }
}

int rts_cube_doppler_device(RtsContext* c, uint32_t n_fft, double* out)
{
    const RtsCubeParams& q = c->cube.params;
    const RtsDopplerPlan plan = rts_doppler_plan(n_fft);
    RTS_HIP(hipFuncSetAttribute((const void*)k_cube_doppler, hipFuncAttributeMaxDynamicSharedMemorySize, (int)plan.lds));
    dim3 grid((q.n_bins + plan.BT - 1) / plan.BT, q.n_rx);
    k_cube_doppler<<<grid, 256, plan.lds, c->stream>>>(c->cube.p, out, q.n_pulses, q.n_bins, n_fft, plan.logN, plan.BT);
    RTS_HIP(hipGetLastError());
    return RTS_OK;
}

// --------------------------------------------------------------------------- the spectrogram
// a workgroup's N x BT elements dealt to its threads: at most 8192 / 256 each (rts_stft_plan: 1024 x 8, 2048 x 4, 4096 x 2) --
// N x BT is a power of two and its 16-byte elements fit the LDS beside the table, so it is below twice this many per thread
#define RTS_STFT_SUM_ITERS 32u
static_assert((RTS_STFT_LDS_MAX / 16u) / RTS_STFT_THREADS < 2u * RTS_STFT_SUM_ITERS, "elements per thread");

struct RtsStftArgs {
    const double2* cube; uint32_t n_pulses_cube, n_bins_cube;
    uint32_t first_pulse, window_len, hop, N, logN, first_bin, n_gate, BT, passes, tiles, n_frames, power, sum;
    const double* w;                  // [window_len] (device) or NULL: no multiply
    double* out; double* partial;     // partial: [n_rx][n_frames][tiles][N] (sum over more than one tile), else unused
};

// blockIdx.x = frame * tiles + tile, blockIdx.y = receiver.  A pass transforms BT gate bins from g0 = (tile * passes + pass) * BT.
// SUM: RTS_STFT_SUM_BINS (an instance of its own: its running sums are registers the other forms do not pay for).
template <bool SUM> __global__ void __launch_bounds__(RTS_STFT_THREADS) k_cube_stft(const RtsStftArgs a)
{
    extern __shared__ __attribute__((aligned(16))) double2 s_stft[];             // [N][BT] complex, then [N/2] complex twiddles
    double2* x = s_stft; double2* tw = s_stft + (size_t)a.N * a.BT;
    const uint32_t t = threadIdx.x, r = blockIdx.y, f = blockIdx.x / a.tiles, tile = blockIdx.x - f * a.tiles;
    const uint32_t N = a.N, BT = a.BT, total = N * BT;
    for (uint32_t k = t; k < N / 2; k += RTS_STFT_THREADS) { double sn, cs; rts_stft_twiddle(k, N, &cs, &sn); tw[k] = make_double2(cs, sn); }
    const double2* rows = a.cube + ((size_t)r * a.n_pulses_cube + a.first_pulse + (size_t)f * a.hop) * a.n_bins_cube + a.first_bin;
    const size_t rf = (size_t)r * a.n_frames + f;
    double acc[RTS_STFT_SUM_ITERS];                                              // RTS_STFT_SUM_BINS: the running sums of this thread's rows
    double* sums = SUM ? (a.tiles > 1u ? a.partial + (rf * a.tiles + tile) * N : a.out + rf * N) : nullptr;
    for (uint32_t pass = 0; pass < a.passes; pass++) {
        const uint32_t g0 = (tile * a.passes + pass) * BT;
        if (g0 >= a.n_gate) break;                                                // (uniform over the workgroup)
        const uint32_t nb = a.n_gate - g0 < BT ? a.n_gate - g0 : BT;
        if (pass) __syncthreads();                                                // (the previous pass's columns have been read)
        for (uint32_t idx = t; idx < total; idx += RTS_STFT_THREADS) {
            const uint32_t p = idx / BT, b = idx - p * BT;
            double2 v = make_double2(0.0, 0.0);
            if (p < a.window_len && b < nb) {
                v = rows[(size_t)p * a.n_bins_cube + g0 + b];
                if (a.w) rts_stft_taper(a.w[p], &v.x, &v.y);
            }
            x[(size_t)rts_stft_bitrev(p, a.logN) * BT + b] = v;
        }
        __syncthreads();
        for (uint32_t s = 1; s <= a.logN; s++) {
            for (uint32_t idx = t; idx < total / 2; idx += RTS_STFT_THREADS) {
                const uint32_t j = idx / BT, b = idx - j * BT;
                uint32_t i0, i1, k; rts_stft_pair(j, s, N, &i0, &i1, &k);
                const double2 w = tw[k];
                double2 u = x[(size_t)i0 * BT + b], v = x[(size_t)i1 * BT + b];
                rts_stft_butterfly(w.x, w.y, &u.x, &u.y, &v.x, &v.y);
                x[(size_t)i0 * BT + b] = u; x[(size_t)i1 * BT + b] = v;
            }
            __syncthreads();
        }
        if (SUM) {
            // every lane forms its element's power; the lane of column 0 adds its row's columns in ascending order onto the row's
            // running sum, which it keeps in a register from pass to pass (element idx has the same thread in every pass).  total
            // and 256 are multiples of BT and BT divides the wave, so a row's BT lanes sit side by side in one wave.
            const bool last = pass + 1u == a.passes || g0 + BT >= a.n_gate;
#pragma unroll
            for (uint32_t it = 0; it < RTS_STFT_SUM_ITERS; it++) {
                if (it * RTS_STFT_THREADS < total) {                              // (uniform)
                    const uint32_t idx = it * RTS_STFT_THREADS + t; const bool live = idx < total;
                    const uint32_t k = idx / BT, b = idx - k * BT;
                    double pw = 0.0;
                    if (live) { const double2 v = x[idx]; pw = rts_stft_power(v.x, v.y); }
                    double s = pass ? acc[it] + pw : pw;
                    for (uint32_t d = 1; d < BT; d++) { const double o = __shfl_down(pw, d); if (d < nb) s += o; }
                    acc[it] = s;
                    if (last && live && b == 0u) sums[k] = s;
                }
            }
        } else {
            for (uint32_t idx = t; idx < total; idx += RTS_STFT_THREADS) {
                const uint32_t k = idx / BT, b = idx - k * BT;
                if (b >= nb) continue;
                const double2 v = x[idx];
                const size_t o = (rf * N + k) * a.n_gate + g0 + b;
                if (a.power) a.out[o] = rts_stft_power(v.x, v.y); else ((double2*)a.out)[o] = v;
            }
        }
    }
}

// the tile sums of one (receiver, frame, row) added in ascending tile order, the first one the start value
__global__ void __launch_bounds__(256) k_stft_sum_tiles(const double* __restrict__ partial, double* __restrict__ out, size_t n_rows, uint32_t N, uint32_t tiles)
{
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n_rows) return;
    const size_t rf = i / N, k = i - rf * N;
    const double* src = partial + rf * tiles * N + k;
    double s = src[0];
    for (uint32_t tl = 1; tl < tiles; tl++) s += src[(size_t)tl * N];
    out[i] = s;
}

// window: the call's taper on the device (rts_cube_api.hip uploads it on the stream before this: RtsCubeState::stft.win) or NULL
int rts_cube_stft_device(RtsContext* c, const RtsStftParams& p, const RtsStftPlan& plan, const double* window, double* out)
{
    const RtsCubeParams& q = c->cube.params;
    RtsStftArgs a;
    a.cube = (const double2*)c->cube.p; a.n_pulses_cube = q.n_pulses; a.n_bins_cube = q.n_bins;
    a.first_pulse = p.first_pulse; a.window_len = p.window_len; a.hop = p.hop; a.N = p.n_fft; a.logN = plan.logN;
    a.first_bin = p.first_bin; a.n_gate = plan.n_gate; a.BT = plan.BT; a.passes = plan.passes; a.tiles = plan.tiles; a.n_frames = plan.n_frames;
    a.power = (p.flags & RTS_STFT_POWER) ? 1u : 0u; a.sum = (p.flags & RTS_STFT_SUM_BINS) ? 1u : 0u;
    a.w = window; a.out = out; a.partial = nullptr;
    if (plan.partial_doubles) { RTS_HIP(c->cube.stft.d_part.reserve(plan.partial_doubles)); a.partial = c->cube.stft.d_part.p; }
    dim3 grid(plan.n_frames * plan.tiles, q.n_rx);
    if (a.sum) {
        RTS_HIP(hipFuncSetAttribute((const void*)k_cube_stft<true>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)plan.lds));
        k_cube_stft<true><<<grid, RTS_STFT_THREADS, plan.lds, c->stream>>>(a);
    } else {
        RTS_HIP(hipFuncSetAttribute((const void*)k_cube_stft<false>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)plan.lds));
        k_cube_stft<false><<<grid, RTS_STFT_THREADS, plan.lds, c->stream>>>(a);
    }
    RTS_HIP(hipGetLastError());
    if (plan.partial_doubles) {
        const size_t n_rows = (size_t)q.n_rx * plan.n_frames * p.n_fft;
        k_stft_sum_tiles<<<(unsigned)((n_rows + 255) / 256), 256, 0, c->stream>>>(a.partial, out, n_rows, p.n_fft, plan.tiles);
        RTS_HIP(hipGetLastError());
    }
    return RTS_OK;
}
