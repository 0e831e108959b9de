// rts_render.hip -- the writers of the cube: impulse, waveform render; range compression (include/rts_amd.h: RtsCubeParams, RtsWaveform):
//   * a pulse's contributions as impulses into the return cube, per received ray or per unique path (k_cube_accumulate)
//   * their render with the handle's transmit waveform (k_cube_render)
//   * range compression (matched filter) of the cube's rows in place (k_cube_compress)
// What a received record contributes, the cell and the add are rts_cube_source.h, shared with the beat render (rts_beat.hip).
#include <hip/hip_runtime.h>
#include "rts_internal.h"

// --------------------------------------------------------------------------- impulse cube
// one lane per received record, two f64 atomics into cube[rx][pulse][bin].  PATHS: per unique path, which needs the aggregation of
// the pulse (RtsCubeSource).  The fused end-of-pulse kernel (rts_post.hip: k_post_all) runs the same row.
template <bool PATHS>
__global__ void k_cube_accumulate(const RtsCubeSource s, double* __restrict__ cube, uint32_t n_rx, uint32_t n_pulses, uint32_t n_bins, uint32_t pulse, double t0, double dt,
                                  const unsigned long long* __restrict__ R_dev)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    uint32_t R = s.R;
    RTS_DEV_COUNT(R_dev, R, return);
    if (i >= R) return;
    rts_cube_impulse_row<PATHS>(s, i, cube, n_rx, n_pulses, n_bins, pulse, t0, dt);
}

template <bool PATHS> static int rts_cube_accumulate_launch(RtsContext* c, const RtsCubeSource& s, uint32_t pulse_index)
{
    if (s.R == 0) return RTS_OK;
    const RtsCubeParams& q = c->cube.params;
    k_cube_accumulate<PATHS><<<(unsigned)(((size_t)s.R + 255) / 256), 256, 0, c->stream>>>(s, c->cube.p, q.n_rx, q.n_pulses, q.n_bins, pulse_index, q.t0, q.dt, c->res.recv_dev);
    RTS_HIP(hipGetLastError());
    return RTS_OK;
}
int rts_cube_accumulate_device(RtsContext* c, uint32_t pulse_index, double cspeed, double carrier) { return rts_cube_accumulate_launch<false>(c, rts_cube_source(c, false, cspeed, carrier, 0), pulse_index); }
int rts_cube_accumulate_paths_device(RtsContext* c, uint32_t pulse_index, int64_t base) { return rts_cube_accumulate_launch<true>(c, rts_cube_source(c, true, 0.0, 0.0, base), pulse_index); }

// --------------------------------------------------------------------------- render (a gather)
// One block per (receiver, tile of RTS_RENDER_TILE output samples); thread t owns output sample n = tile start + t.  The waveform
// is staged in LDS.  The received set is scanned in chunks of RTS_RENDER_TILE records: every thread reads one, keeps it if it
// belongs to this block's receiver and its support reaches the tile, and the kept ones are compacted into LDS in the set's order
// (ballot + per-wave counts).  Their L weights h_L(q - phi) depend only on the fractional start phi: they are computed once per
// contribution and block, RTS_RENDER_SUB contributions at a time, into LDS.  Every thread then sums the contributions in order
// in registers; each finished sample goes to the cube with one atomic add per component.
#define RTS_RENDER_TILE 128
#define RTS_RENDER_SUB 32
struct RtsRenderArgs {
    RtsCubeSource src; int doppler;
    double* cube; uint32_t n_rx, n_pulses, n_bins, pulse; double t0, dt;
    const double* wave; uint32_t M, L;
};
struct RtsRenderItem { double are, aim, phi, d, f; int D; int pad; };

__global__ void __launch_bounds__(RTS_RENDER_TILE) k_cube_render(const RtsRenderArgs a, const unsigned long long* __restrict__ R_dev)
{
    extern __shared__ __attribute__((aligned(16))) double s_render[];      // [M] complex samples, then [RTS_RENDER_SUB][L] weights
    __shared__ RtsRenderItem s_item[RTS_RENDER_TILE];
    __shared__ uint32_t s_wave_n[RTS_RENDER_TILE / 64];
    double* sw = s_render; double* wts = s_render + 2 * (size_t)a.M;
    const uint32_t t = threadIdx.x, lane = t & 63u, wv = t >> 6, rx = blockIdx.y;
    const uint32_t M = a.M, L = a.L;
    const int q0 = rts_wave_q0(L);
    const int n = (int)(blockIdx.x * RTS_RENDER_TILE + t);
    const double n0 = (double)(blockIdx.x * RTS_RENDER_TILE);
    const double n1 = fmin(n0 + (double)(RTS_RENDER_TILE - 1), (double)a.n_bins - 1.0);       // last sample of the tile
    const double reach = (double)q0 + (double)(L - 1u) + (double)(M - 1u);                        // support of a start D: [D + q0, D + reach]
    uint32_t R = a.src.R;
    RTS_DEV_COUNT(R_dev, R, return);
    for (uint32_t i = t; i < 2 * M; i += RTS_RENDER_TILE) sw[i] = a.wave[i];
    double acc_r = 0.0, acc_i = 0.0;
    for (uint32_t c0 = 0; c0 < R; c0 += RTS_RENDER_TILE) {
        // ---- this chunk's contributions to the block's tile, compacted in order
        const uint32_t i = c0 + t;
        bool keep = false; RtsRenderItem it;
        if (i < R) {
            if (rts_cube_counts_for(a.src, a.src.paths != 0, i, (int32_t)rx)) {
                double delay, phase; rts_cube_timing(a.src, a.src.paths != 0, i, &delay, &phase);
                const double d = (delay - a.t0) / a.dt;
                const double Df = floor(d);
                if (Df + (double)q0 <= n1 && Df + reach >= n0) {          // (false for a non-finite start)
                    const PerRayData& r = a.src.rays[i];
                    rts_cube_amplitude(r.power, phase, &it.are, &it.aim);
                    it.phi = d - Df; it.d = d; it.f = r.doppler; it.D = (int)Df; it.pad = 0;
                    keep = true;
                }
            }
        }
        const unsigned long long ball = __ballot(keep);
        const uint32_t before = (uint32_t)__popcll(ball & ((1ull << lane) - 1ull));
        if (lane == 0) s_wave_n[wv] = (uint32_t)__popcll(ball);
        __syncthreads();
        uint32_t off = 0, total = 0;
        for (uint32_t w = 0; w < RTS_RENDER_TILE / 64; w++) { if (w < wv) off += s_wave_n[w]; total += s_wave_n[w]; }
        if (keep) s_item[off + before] = it;
        __syncthreads();
        // ---- in order, RTS_RENDER_SUB at a time: weights, then the sum
        for (uint32_t s0 = 0; s0 < total; s0 += RTS_RENDER_SUB) {
            const uint32_t ns = min((uint32_t)RTS_RENDER_SUB, total - s0);
            for (uint32_t k = t; k < ns * L; k += RTS_RENDER_TILE) {
                const uint32_t c = k / L, j = k - c * L;
                wts[k] = rts_wave_h((double)(q0 + (int)j) - s_item[s0 + c].phi, L);
            }
            __syncthreads();
            if ((uint32_t)n < a.n_bins) {
                for (uint32_t c = 0; c < ns; c++) {
                    const RtsRenderItem& q = s_item[s0 + c];
                    const int k = n - q.D - q0;                          // sample index of tap j: k - j
                    const int jlo = max(0, k - (int)M + 1), jhi = min((int)L - 1, k);
                    if (jlo > jhi) continue;
                    const double* w = wts + (size_t)c * L;
                    double er = 0.0, ei = 0.0;
                    for (int j = jlo; j <= jhi; j++) { const double h = w[j]; er += sw[2 * (k - j)] * h; ei += sw[2 * (k - j) + 1] * h; }
                    double vr = q.are * er - q.aim * ei, vi = q.are * ei + q.aim * er;      // a s(n - d)
                    if (a.doppler) {
                        double sn, cs; sincospi(2.0 * q.f * (((double)n - q.d) * a.dt), &sn, &cs);      // e^{j 2 pi f (n - d) dt}
                        const double tr = vr * cs - vi * sn; vi = vr * sn + vi * cs; vr = tr;
                    }
                    acc_r += vr; acc_i += vi;
                }
            }
            __syncthreads();
        }
    }
    if ((uint32_t)n < a.n_bins && (acc_r != 0.0 || acc_i != 0.0)) rts_cube_add(rts_cube_cell(a.cube, a.n_pulses, a.n_bins, rx, a.pulse, n), acc_r, acc_i);
}

int rts_cube_render_device(RtsContext* c, uint32_t pulse_index, bool paths, bool doppler, double cspeed, double carrier, int64_t base)
{
    RtsRenderArgs a;
    a.src = rts_cube_source(c, paths, cspeed, carrier, base); a.doppler = doppler ? 1 : 0;
    if (a.src.R == 0) return RTS_OK;
    const RtsCubeParams& q = c->cube.params;
    a.cube = c->cube.p; a.n_rx = q.n_rx; a.n_pulses = q.n_pulses; a.n_bins = q.n_bins; a.pulse = pulse_index; a.t0 = q.t0; a.dt = q.dt;
    a.wave = c->cube.wave.d.p; a.M = c->cube.wave.M; a.L = c->cube.wave.L;
    const size_t lds = sizeof(double) * (2 * (size_t)a.M + (size_t)RTS_RENDER_SUB * a.L);      // <= 64 KiB + 16 KiB
    RTS_HIP(hipFuncSetAttribute((const void*)k_cube_render, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    dim3 grid((q.n_bins + RTS_RENDER_TILE - 1) / RTS_RENDER_TILE, q.n_rx);
    k_cube_render<<<grid, RTS_RENDER_TILE, lds, c->stream>>>(a, c->res.recv_dev);
    RTS_HIP(hipGetLastError());
    return RTS_OK;
}

// --------------------------------------------------------------------------- range compression, in place
// z[n] = sum_m y[n + m] conj(s[m]).  One block per row (receiver, pulse): the whole row is read into LDS before any output is
// written, so the correlation can run in place; the waveform is read from memory (every lane reads the same sample: one
// broadcast load per m).  Thread t owns the outputs t + r * 256, r < RTS_COMPRESS_NR, of each pass: consecutive lanes read
// consecutive 16-byte LDS slots.
#define RTS_COMPRESS_THREADS 256
#define RTS_COMPRESS_NR 8
__global__ void __launch_bounds__(RTS_COMPRESS_THREADS) k_cube_compress(double* __restrict__ cube, const double* __restrict__ s, uint32_t M, uint32_t n_pulses,
                                                                        uint32_t first, uint32_t n_bins)
{
    extern __shared__ __attribute__((aligned(16))) double s_row[];            // [n_bins] complex
    const uint32_t t = threadIdx.x;
    double* row = cube + 2 * (((size_t)blockIdx.y * n_pulses + first + blockIdx.x) * n_bins);
    for (uint32_t i = t; i < n_bins; i += RTS_COMPRESS_THREADS) { s_row[2 * i] = row[2 * i]; s_row[2 * i + 1] = row[2 * i + 1]; }
    __syncthreads();
    for (uint32_t b0 = 0; b0 < n_bins; b0 += RTS_COMPRESS_THREADS * RTS_COMPRESS_NR) {
        double zr[RTS_COMPRESS_NR], zi[RTS_COMPRESS_NR];
        for (int r = 0; r < RTS_COMPRESS_NR; r++) { zr[r] = 0.0; zi[r] = 0.0; }
        const uint32_t mmax = min(M, n_bins - b0);
        for (uint32_t m = 0; m < mmax; m++) {
            const double sr = s[2 * m], si = s[2 * m + 1];
            for (int r = 0; r < RTS_COMPRESS_NR; r++) {
                const uint32_t j = b0 + t + (uint32_t)r * RTS_COMPRESS_THREADS + m;
                if (j < n_bins) { const double yr = s_row[2 * j], yi = s_row[2 * j + 1]; zr[r] += yr * sr + yi * si; zi[r] += yi * sr - yr * si; }
            }
        }
        for (int r = 0; r < RTS_COMPRESS_NR; r++) {
            const uint32_t nn = b0 + t + (uint32_t)r * RTS_COMPRESS_THREADS;
            if (nn < n_bins) { row[2 * nn] = zr[r]; row[2 * nn + 1] = zi[r]; }
        }
    }
}

int rts_cube_compress_device(RtsContext* c, uint32_t first_pulse, uint32_t n_pulses)
{
    const RtsCubeParams& q = c->cube.params;
    if (n_pulses == 0) return RTS_OK;
    const size_t lds = 16 * (size_t)q.n_bins;                                   // <= 128 KiB (RTS_COMPRESS_MAX_BINS)
    RTS_HIP(hipFuncSetAttribute((const void*)k_cube_compress, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    dim3 grid(n_pulses, q.n_rx);
    k_cube_compress<<<grid, RTS_COMPRESS_THREADS, lds, c->stream>>>(c->cube.p, c->cube.wave.d.p, c->cube.wave.M, q.n_pulses, first_pulse, q.n_bins);
    RTS_HIP(hipGetLastError());
    return RTS_OK;
}
