// rts_stap.hip -- the space-time tap filter on the device (include/rts_amd.h: rts_cube_st_apply): k_st_apply.
// The arithmetic and the plan of the launch are rts_stap.h, shared with the host evaluator.  (The stacked covariance is
// k_cube_cov's stacked form, rts_adapt.hip.)
#include <hip/hip_runtime.h>
#include "rts_internal.h"
#include "rts_stap.h"

// A skinny complex f64 product like the beamformer's, y[f][p][b] = sum_d conj(w[f][d]) x[d], bound by memory -- but the snapshots
// of neighbouring rows share n_taps - 1 of their n_taps rows: a cell-per-thread kernel reads every input element n_taps times.
// The sum's order (ascending d = m n_rx + rx) is what streaming the input rows in ascending order yields: a thread owns a bin (the
// 64 lanes of the wave consecutive bins: every global access is 64 consecutive 16-byte elements) and walks a strip of output rows;
// it loads input row q's n_rx samples once, in tiles of RTS_ST_RX_TILE receivers, and adds them with tap m's weights into output
// p = q - m, for every m: slot m of a ring of M running sums per filter.  After row q, slot M - 1 (output q - M + 1) is complete
// and stored, and the ring moves up by one slot (register moves with static indices: M is a template parameter; the moves are
// 1 / (2 n_rx) of the row's arithmetic).  A strip reads M - 1 rows behind its last output row, which the next strip reads again
// (the halo); the ring's slots of outputs outside the strip get no arithmetic (a branch of the whole wave per tap) and are never
// stored.  The strip is short (RTS_ST_STRIP = 16 rows): at 256 rows x 4 096 bins a strip of 32 leaves one wave per SIMD, and the
// halo's reads, which the neighbouring strip makes too, cost less than the idle SIMDs (profiles/stap_bench.txt).
// Registers: M x FT complex128 sums (FT = RTS_ST_FILTER_TILE(M): at most 32 sums, 128 VGPRs) and one receiver tile (32 VGPRs).
// A workgroup serves ONE filter tile, whose weights [FT][D] it stages in LDS; every lane reads the same weight at the same time,
// one 16-byte broadcast read per term and no bank conflict.  More filters than a tile: more workgroups, which read the input again.
struct RtsStArgs {
    const double2* in;                // receiver 0, row first_row, bin 0 of the source
    uint64_t rx_stride, out_cells;    // elements between two receivers of the source; out_rows n_bins
    const double2* w;                 // [n_filters][D] (device)
    uint32_t n_rx, n_filters, n_bins, out_rows, bin_groups, strips;
    void* out;
};

template <int M, bool POWER> __global__ void __launch_bounds__(RTS_ST_THREADS) k_st_apply(const RtsStArgs a)
{
    constexpr uint32_t FT = RTS_ST_FILTER_TILE((uint32_t)M);
    extern __shared__ __attribute__((aligned(16))) double2 s_st_w[];             // [FT][D], the tile's filters
    const uint32_t t = threadIdx.x, N = a.n_rx, D = (uint32_t)M * N;
    const uint32_t bg = blockIdx.x % a.bin_groups, rest = blockIdx.x / a.bin_groups, strip = rest % a.strips, f0 = rest / a.strips * FT;
    const uint32_t nf = a.n_filters - f0 < FT ? a.n_filters - f0 : FT;
    for (uint32_t i = t; i < nf * D; i += RTS_ST_THREADS) s_st_w[i] = a.w[(size_t)f0 * D + i];
    __syncthreads();
    const uint32_t b = bg * RTS_ST_THREADS + t;
    if (b >= a.n_bins) return;
    const uint32_t p0 = strip * RTS_ST_STRIP, p1 = a.out_rows - p0 < RTS_ST_STRIP ? a.out_rows : p0 + RTS_ST_STRIP;
    uint32_t wj[FT];                                                              // the LDS rows of the tile's filters (past the last: the last again, sums nobody stores)
#pragma unroll
    for (uint32_t j = 0; j < FT; j++) wj[j] = (j < nf ? j : nf - 1u) * D;
    double2 acc[M][FT];
#pragma unroll
    for (uint32_t k = 0; k < (uint32_t)M * FT; k++) acc[k / FT][k % FT] = make_double2(0.0, 0.0);
    const double2* __restrict__ in = a.in + b;
    for (uint32_t q = p0; q < p1 + (uint32_t)M - 1u; q++) {                       // (q <= out_rows + M - 2: the span's last row)
        const double2* __restrict__ row = in + (uint64_t)q * a.n_bins;
        for (uint32_t r0 = 0; r0 < N; r0 += RTS_ST_RX_TILE) {
            const uint32_t live = N - r0 < RTS_ST_RX_TILE ? N - r0 : RTS_ST_RX_TILE;
            double2 z[RTS_ST_RX_TILE];
#pragma unroll
            for (uint32_t r = 0; r < RTS_ST_RX_TILE; r++) z[r] = r < live ? row[(uint64_t)(r0 + r) * a.rx_stride] : make_double2(0.0, 0.0);
#pragma unroll
            for (uint32_t m = 0; m < (uint32_t)M; m++) {
                if (q < p0 + m || q >= p1 + m) continue;                           // output q - m is another strip's (the wave's branch: no arithmetic for it)
#pragma unroll
                for (uint32_t r = 0; r < RTS_ST_RX_TILE; r++) {
                    if (r < live) {
#pragma unroll
                        for (uint32_t j = 0; j < FT; j++) {
                            const double2 w = s_st_w[wj[j] + m * N + r0 + r];
                            rts_beam_add(m == 0u && r0 + r == 0u, w.x, w.y, z[r].x, z[r].y, &acc[m][j].x, &acc[m][j].y);
                        }
                    }
                }
            }
        }
        if (q >= p0 + (uint32_t)M - 1u) {                                         // output q - M + 1 has had its last row
            const uint64_t o = (uint64_t)(q - ((uint32_t)M - 1u)) * a.n_bins + b;
#pragma unroll
            for (uint32_t j = 0; j < FT; j++) {
                if (j < nf) {
                    const double2 y = acc[M - 1][j];
                    if (POWER) ((double*)a.out)[(uint64_t)(f0 + j) * a.out_cells + o] = rts_beam_power(y.x, y.y);
                    else ((double2*)a.out)[(uint64_t)(f0 + j) * a.out_cells + o] = y;
                }
            }
        }
#pragma unroll
        for (uint32_t m = (uint32_t)M - 1u; m > 0u; m--)
#pragma unroll
            for (uint32_t j = 0; j < FT; j++) acc[m][j] = acc[m - 1u][j];
    }
}

template <int M> static void rts_st_launch(const RtsStArgs& a, const RtsStApplyPlan& plan, bool power, hipStream_t stream)
{
    if (power) k_st_apply<M, true><<<plan.groups, RTS_ST_THREADS, plan.lds, stream>>>(a);
    else k_st_apply<M, false><<<plan.groups, RTS_ST_THREADS, plan.lds, stream>>>(a);
}

// in: the source's receiver 0, row first_row (device); rx_stride: its n_rows_in n_bins; weights: the call's table on the device
// (rts_cube_array_api.hip uploads it on the stream before this: RtsCubeState::stap.w)
int rts_cube_st_apply_device(RtsContext* c, const RtsStApplyParams& p, const RtsStApplyPlan& plan, const double* in, uint64_t rx_stride, const double* weights, void* out)
{
    RtsStArgs a;
    a.in = (const double2*)in; a.rx_stride = rx_stride; a.out_cells = plan.out_cells; a.w = (const double2*)weights;
    a.n_rx = c->cube.params.n_rx; a.n_filters = p.n_filters; a.n_bins = c->cube.params.n_bins; a.out_rows = plan.out_rows;
    a.bin_groups = plan.bin_groups; a.strips = plan.strips; a.out = out;
    const bool power = (p.flags & RTS_BEAM_POWER) != 0;
    switch (p.n_taps) {                                                           // (the plan's LDS is at most 16 KiB: no attribute to raise)
#define RTS_ST_CASE(m) case m: rts_st_launch<m>(a, plan, power, c->stream); break;
        RTS_ST_CASE(1) RTS_ST_CASE(2) RTS_ST_CASE(3) RTS_ST_CASE(4) RTS_ST_CASE(5) RTS_ST_CASE(6) RTS_ST_CASE(7) RTS_ST_CASE(8)
        RTS_ST_CASE(9) RTS_ST_CASE(10) RTS_ST_CASE(11) RTS_ST_CASE(12) RTS_ST_CASE(13) RTS_ST_CASE(14) RTS_ST_CASE(15) RTS_ST_CASE(16)
#undef RTS_ST_CASE
        default: rts_set_error("rts_cube_st_apply: n_taps = %u has no kernel", p.n_taps); return RTS_ERR_INVALID;
    }
    RTS_HIP(hipGetLastError());
    return RTS_OK;
}
