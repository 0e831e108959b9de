// rts_beat.hip -- FMCW / stretch processing on the device (include/rts_amd.h: rts_cube_render_beat, rts_cube_range_transform):
//   * the dechirped beat render of a pulse's contributions into a row of the return cube (k_cube_beat, k_cube_beat_sum)
//   * the fast-time (range-axis) transform of the cube's rows (k_cube_range)
// The arithmetic and the plans of the launches are rts_beat.h (the transform's tree: rts_stft.h), shared with the host evaluators;
// what a received record contributes, the cell and the add are rts_cube_source.h, shared with the other writers (rts_render.hip).
#include <hip/hip_runtime.h>
#include "rts_internal.h"
#include "rts_beat.h"

// --------------------------------------------------------------------------- beat render (a gather)
// One workgroup of ONE wave per (receiver, tile of RTS_BEAT_TILE samples, part of the received set); lane t owns the strip of
// RTS_BEAT_STRIP samples at tile start + t * RTS_BEAT_STRIP: its sums are 32 doubles in registers, its sample times 16 more.  The
// part's records are scanned in chunks of 64: every lane reads one, keeps it if it belongs to this workgroup's receiver (and is its
// path's representative) and arrives no later than the tile's last sample, and forms its item (rts_beat.h: amplitude, delay, beat
// frequency, constant phase, the step's rotation) ONCE; the kept items are compacted into LDS in the set's order (ballot).  Every
// lane then walks the items in order -- all lanes read the same LDS address: a broadcast -- and its strip by rotation: per item one
// sincospi and 16 x (4 multiplies + 2 adds for the term, 2 adds for the sum, 4 + 2 for the rotation) in f64, which is what bounds
// the kernel: unlike the pulsed render every contribution reaches almost every sample.
// The finished sums cross a padded LDS tile (17 slots of 16 bytes per strip: lane t's 16-byte stores land on 16 different slots per
// 16 lanes) so that the workgroup's global accesses are coalesced: 64 consecutive samples per instruction, whether they are the
// atomic adds of a one-part render or the stores of a part's sums to scratch[part][rx][n].
struct RtsBeatArgs {
    RtsCubeSource src; uint32_t part_len; int doppler;
    double* cube; uint32_t n_pulses, n_bins, pulse; double t0, dt, S, T;
    double2* scratch;                 // more than one part: [parts][n_rx][n_bins]; else null: the sums are added to the cube
};
#define RTS_BEAT_PAD (RTS_BEAT_STRIP + 1u)

__global__ void __launch_bounds__(RTS_BEAT_THREADS) k_cube_beat(const RtsBeatArgs a, const unsigned long long* __restrict__ R_dev)
{
    __shared__ __attribute__((aligned(16))) RtsBeatItem s_item[RTS_BEAT_THREADS];
    __shared__ __attribute__((aligned(16))) double2 s_out[RTS_BEAT_THREADS * RTS_BEAT_PAD];
    const uint32_t lane = threadIdx.x, rx = blockIdx.y, part = blockIdx.z, n_rx = gridDim.y;
    uint32_t R = a.src.R;
    RTS_DEV_COUNT(R_dev, R, R = 0u);        // (renders nothing, but reaches the barriers and writes its part's zeros to scratch)
    const uint32_t tile0 = blockIdx.x * RTS_BEAT_TILE, n0 = tile0 + lane * RTS_BEAT_STRIP;
    const uint32_t tile_end = a.n_bins - tile0 < RTS_BEAT_TILE ? a.n_bins : tile0 + RTS_BEAT_TILE;      // (tile0 < n_bins: the grid's tiles)
    const double t_tile = rts_beat_time(a.t0, a.dt, tile_end - 1u);
    double t[RTS_BEAT_STRIP], acc[2 * RTS_BEAT_STRIP];
    double t_last = 0.0;
    bool live = n0 < a.n_bins;
    if (live) { t_last = rts_beat_strip_times(a.t0, a.dt, n0, a.n_bins, t); live = t[0] < a.T && t_last >= 0.0; }      // (a strip outside the oscillator's run passes no gate)
#pragma unroll
    for (uint32_t i = 0; i < 2 * RTS_BEAT_STRIP; i++) acc[i] = 0.0;
    const uint64_t begin64 = (uint64_t)part * a.part_len;
    const uint32_t begin = begin64 < R ? (uint32_t)begin64 : R;
    const uint32_t end = R - begin < a.part_len ? R : begin + a.part_len;
    for (uint32_t c0 = begin; c0 < end; c0 += RTS_BEAT_THREADS) {
        // ---- this chunk's contributions to the workgroup's tile, compacted in order
        const uint32_t i = c0 + lane;            // (c0 < end <= R < 2^32, lane < 64: wraps only past R, where the test below fails)
        bool keep = false; RtsBeatItem it;
        if (i >= c0 && i < end) {
            if (rts_cube_counts_for(a.src, a.src.paths != 0, i, (int32_t)rx)) {
                double delay, phase; rts_cube_timing(a.src, a.src.paths != 0, i, &delay, &phase);
                if (rts_beat_finite(delay) && delay <= t_tile) {
                    const PerRayData& r = a.src.rays[i];
                    double are, aim; rts_cube_amplitude(r.power, phase, &are, &aim);
                    it = rts_beat_item(are, aim, delay, a.doppler ? r.doppler : 0.0, a.S, a.dt);
                    keep = true;
                }
            }
        }
        const unsigned long long ball = __ballot(keep);
        const uint32_t before = (uint32_t)__popcll(ball & ((1ull << lane) - 1ull)), total = (uint32_t)__popcll(ball);
        __syncthreads();                          // (the previous chunk's items have been read)
        if (keep) s_item[before] = it;
        __syncthreads();
        if (live) for (uint32_t c = 0; c < total; c++) { const RtsBeatItem q = s_item[c]; rts_beat_strip(q, t, t_last, a.T, acc); }
    }
    // ---- the strip's sums -> the padded tile -> 64 consecutive samples per instruction
#pragma unroll
    for (uint32_t i = 0; i < RTS_BEAT_STRIP; i++) s_out[lane * RTS_BEAT_PAD + i] = make_double2(acc[2 * i], acc[2 * i + 1]);
    __syncthreads();
    for (uint32_t m = lane; m < RTS_BEAT_TILE; m += RTS_BEAT_THREADS) {
        const uint32_t n = tile0 + m;
        if (n >= a.n_bins) break;
        const double2 v = s_out[(m / RTS_BEAT_STRIP) * RTS_BEAT_PAD + (m % RTS_BEAT_STRIP)];
        if (a.scratch) a.scratch[((size_t)part * n_rx + rx) * a.n_bins + n] = v;
        else if (v.x != 0.0 || v.y != 0.0) rts_cube_add(rts_cube_cell(a.cube, a.n_pulses, a.n_bins, rx, a.pulse, n), v.x, v.y);
    }
}

// the parts' sums of one sample added in ascending part order, the first one the start value; then the one atomic add per component
__global__ void __launch_bounds__(256) k_cube_beat_sum(const double2* __restrict__ scratch, double* __restrict__ cube, uint32_t parts, uint32_t n_rx,
                                                       uint32_t n_pulses, uint32_t n_bins, uint32_t pulse)
{
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x, cells = (size_t)n_rx * n_bins;
    if (i >= cells) return;
    double2 s = scratch[i];
    for (uint32_t p = 1; p < parts; p++) { const double2 v = scratch[(size_t)p * cells + i]; s.x += v.x; s.y += v.y; }
    if (s.x != 0.0 || s.y != 0.0) {
        const size_t rx = i / n_bins, n = i - rx * n_bins;
        rts_cube_add(rts_cube_cell(cube, n_pulses, n_bins, rx, pulse, n), s.x, s.y);
    }
}

int rts_cube_beat_device(RtsContext* c, uint32_t pulse_index, const RtsBeatParams& p, const RtsBeatPlan& plan, double cspeed, double carrier, int64_t base)
{
    RtsBeatArgs a;
    a.src = rts_cube_source(c, p.source == RTS_RENDER_PATHS, cspeed, carrier, base);
    if (a.src.R == 0) return RTS_OK;
    const RtsCubeParams& q = c->cube.params;
    a.part_len = plan.part_len; a.doppler = (p.flags & RTS_RENDER_DOPPLER) ? 1 : 0;
    a.cube = c->cube.p; a.n_pulses = q.n_pulses; a.n_bins = q.n_bins; a.pulse = pulse_index; a.t0 = q.t0; a.dt = q.dt;
    a.S = p.slope; a.T = p.duration; a.scratch = nullptr;
    if (plan.scratch_doubles) { RTS_HIP(c->cube.fmcw.d_beat_part.reserve(plan.scratch_doubles)); a.scratch = (double2*)c->cube.fmcw.d_beat_part.p; }
    dim3 grid(plan.tiles, q.n_rx, plan.P);
    k_cube_beat<<<grid, RTS_BEAT_THREADS, 0, c->stream>>>(a, c->res.recv_dev);
    RTS_HIP(hipGetLastError());
    if (a.scratch) {
        const size_t cells = (size_t)q.n_rx * q.n_bins;
        k_cube_beat_sum<<<(unsigned)((cells + 255) / 256), 256, 0, c->stream>>>(a.scratch, c->cube.p, plan.P, q.n_rx, q.n_pulses, q.n_bins, pulse_index);
        RTS_HIP(hipGetLastError());
    }
    return RTS_OK;
}

// --------------------------------------------------------------------------- range transform
// One workgroup per RT consecutive rows (rts_beat.h: rts_range_plan).  LDS: x[r][i], RT rows of N complex128, then the N / 2 complex
// twiddles.  A row is contiguous in the cube and in the output, so consecutive lanes load consecutive samples and store consecutive
// bins: coalesced.  The butterflies are rts_stft.h's, each row on its own; a stage with half = 2^(s-1) < 16 has the 16 lanes of a
// 128-bit LDS access read runs of `half` elements 2 half apart, which lands two of them on the same slot (2-way, the first four of
// log2 N stages); from stage 5 on the runs are 16 consecutive elements: conflict-free.
struct RtsRangeFftArgs {
    const double2* cube; uint32_t n_pulses_cube, n_bins_cube;
    uint32_t first_pulse, n_pulses, first_bin, n_samples, N, logN, n_out, RT, reverse;
    uint64_t rows;
    const double* w;                  // [n_samples] (device) or NULL: no multiply
    double2* out;
};

__global__ void __launch_bounds__(RTS_RANGE_THREADS) k_cube_range(const RtsRangeFftArgs a)
{
    extern __shared__ __attribute__((aligned(16))) double2 s_range[];            // [RT][N] complex, then [N/2] complex twiddles
    const uint32_t t = threadIdx.x, N = a.N, total = N * a.RT;
    double2* x = s_range; double2* tw = s_range + total;
    for (uint32_t k = t; k < N / 2; k += RTS_RANGE_THREADS) { double sn, cs; rts_stft_twiddle(k, N, &cs, &sn); tw[k] = make_double2(cs, sn); }
    const uint64_t g0 = (uint64_t)blockIdx.x * a.RT;
    const uint32_t nr = a.rows - g0 < a.RT ? (uint32_t)(a.rows - g0) : a.RT;       // rows of this workgroup (g0 < rows: the grid)
    for (uint32_t idx = t; idx < total; idx += RTS_RANGE_THREADS) {
        const uint32_t r = idx >> a.logN, i = idx & (N - 1u);
        double2 v = make_double2(0.0, 0.0);
        if (r < nr && i < a.n_samples) {
            const uint64_t g = g0 + r, rx = g / a.n_pulses, j = g - rx * a.n_pulses;
            v = a.cube[(rx * a.n_pulses_cube + a.first_pulse + j) * a.n_bins_cube + a.first_bin + i];
            if (a.w) rts_stft_taper(a.w[i], &v.x, &v.y);
        }
        x[(r << a.logN) + rts_stft_bitrev(i, a.logN)] = v;
    }
    __syncthreads();
    for (uint32_t s = 1; s <= a.logN; s++) {
        for (uint32_t idx = t; idx < total / 2; idx += RTS_RANGE_THREADS) {
            const uint32_t r = idx >> (a.logN - 1u), j = idx & (N / 2 - 1u);
            uint32_t i0, i1, k; rts_stft_pair(j, s, N, &i0, &i1, &k);
            const double2 w = tw[k];
            double2* row = x + (r << a.logN);
            double2 u = row[i0], v = row[i1];
            rts_stft_butterfly(w.x, w.y, &u.x, &u.y, &v.x, &v.y);
            row[i0] = u; row[i1] = v;
        }
        __syncthreads();
    }
    const uint32_t n_store = nr * a.n_out;                                       // <= RT * N
    for (uint32_t idx = t; idx < n_store; idx += RTS_RANGE_THREADS) {
        const uint32_t r = idx / a.n_out, k = idx - r * a.n_out;
        const uint32_t src = a.reverse ? (N - k) & (N - 1u) : k;
        a.out[(g0 + r) * a.n_out + k] = x[(r << a.logN) + src];
    }
}

// window: the call's taper on the device (rts_cube_api.hip uploads it on the stream before this: RtsCubeState::fmcw.range_win) or NULL
int rts_cube_range_device(RtsContext* c, const RtsRangeParams& p, const RtsRangePlan& plan, const double* window, double* out)
{
    const RtsCubeParams& q = c->cube.params;
    RtsRangeFftArgs a;
    a.cube = (const double2*)c->cube.p; a.n_pulses_cube = q.n_pulses; a.n_bins_cube = q.n_bins;
    a.first_pulse = p.first_pulse; a.n_pulses = p.n_pulses; a.first_bin = p.first_bin; a.n_samples = plan.n_samples;
    a.N = p.n_fft; a.logN = plan.logN; a.n_out = plan.n_out; a.RT = plan.RT; a.reverse = (p.flags & RTS_RANGE_REVERSE) ? 1u : 0u;
    a.rows = plan.rows; a.w = window; a.out = (double2*)out;
    RTS_HIP(hipFuncSetAttribute((const void*)k_cube_range, hipFuncAttributeMaxDynamicSharedMemorySize, (int)plan.lds));
    k_cube_range<<<plan.groups, RTS_RANGE_THREADS, plan.lds, c->stream>>>(a);
    RTS_HIP(hipGetLastError());
    return RTS_OK;
}
