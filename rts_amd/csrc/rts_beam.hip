// rts_beam.hip -- receive-array beamforming on the device (include/rts_amd.h: rts_cube_beamform): k_cube_beam.
// The arithmetic and the plan of the launch are rts_beam.h, shared with the host evaluator.
#include <hip/hip_runtime.h>
#include "rts_internal.h"
#include "rts_beam.h"

// A skinny complex f64 matrix product, y[b][cell] = sum_rx conj(w[b][rx]) z[rx][cell], bound by memory: per cell 16 n_rx bytes in,
// 16 n_beams out.  The rows a call reads are contiguous per receiver and a beam's output is contiguous, so the cells (row, bin) are
// one flat index: thread t of workgroup g owns cell 256 g + t, and every global access of a wave is 64 consecutive 16-byte
// elements (the power forms: 8-byte), whatever n_bins.
// The weight table [n_beams][n_rx] is staged once per workgroup in LDS (at most 64 KiB); every lane of a wave reads the same
// weight at the same time, one 16-byte broadcast read per term and no bank conflict.
// Registers: the cell's samples of one receiver tile (RTS_BEAM_RX_TILE complex128 = 32 VGPRs) and the running sums of one beam tile
// (RTS_BEAM_BEAM_TILE complex128 = 64 VGPRs).  Up to one receiver tile the samples are loaded ONCE and serve every beam; with more,
// each beam tile walks the receiver tiles in ascending order and reads the samples again (from L2: 1 / RTS_BEAM_BEAM_TILE of a
// re-read per beam).  A sum's order is the header's whatever the tiles: ascending receivers, the first term the start value.
// RTS_BEAM_PEAK keeps rts_beam.h's streaming record per lane instead of storing the beams.
struct RtsBeamArgs {
    const double2* in;                // receiver 0, row first_row, bin 0 of the source
    uint64_t rx_stride, cells;        // elements between two receivers of the source; n_rows n_bins
    const double2* w;                 // [n_beams][n_rx] (device)
    uint32_t n_rx, n_beams, rx_tiles;
    void* out;
};
enum { RTS_BEAM_OUT_COMPLEX = 0, RTS_BEAM_OUT_POWER = 1, RTS_BEAM_OUT_PEAK = 2 };

__device__ __forceinline__ void rts_beam_load(double2* z, const double2* __restrict__ in, uint64_t rx_stride, uint32_t r0, uint32_t live)
{
#pragma unroll
    for (uint32_t r = 0; r < RTS_BEAM_RX_TILE; r++) z[r] = r < live ? in[(uint64_t)(r0 + r) * rx_stride] : make_double2(0.0, 0.0);
}

template <int MODE> __global__ void __launch_bounds__(RTS_BEAM_THREADS) k_cube_beam(const RtsBeamArgs a)
{
    extern __shared__ __attribute__((aligned(16))) double2 s_beam_w[];           // [n_beams][n_rx]
    const uint32_t t = threadIdx.x, nw = a.n_beams * a.n_rx;
    for (uint32_t i = t; i < nw; i += RTS_BEAM_THREADS) s_beam_w[i] = a.w[i];
    __syncthreads();
    const uint64_t c = (uint64_t)blockIdx.x * RTS_BEAM_THREADS + t;
    if (c >= a.cells) return;
    const double2* __restrict__ in = a.in + c;
    double2 z[RTS_BEAM_RX_TILE];
    const bool one = a.rx_tiles == 1u;
    if (one) rts_beam_load(z, in, a.rx_stride, 0u, a.n_rx);
    RtsBeamPeak pk = {0.0, 0.0, 0.0, 0.0, 0u, 0u};
    for (uint32_t b0 = 0; b0 < a.n_beams; b0 += RTS_BEAM_BEAM_TILE) {
        const uint32_t nb = a.n_beams - b0 < RTS_BEAM_BEAM_TILE ? a.n_beams - b0 : RTS_BEAM_BEAM_TILE;
        double2 y[RTS_BEAM_BEAM_TILE];
#pragma unroll
        for (uint32_t j = 0; j < RTS_BEAM_BEAM_TILE; j++) y[j] = make_double2(0.0, 0.0);
        for (uint32_t r0 = 0; r0 < a.n_rx; r0 += RTS_BEAM_RX_TILE) {
            const uint32_t live = a.n_rx - r0 < RTS_BEAM_RX_TILE ? a.n_rx - r0 : RTS_BEAM_RX_TILE;
            if (!one) rts_beam_load(z, in, a.rx_stride, r0, live);
#pragma unroll
            for (uint32_t r = 0; r < RTS_BEAM_RX_TILE; r++) {
                if (r < live) {
#pragma unroll
                    for (uint32_t j = 0; j < RTS_BEAM_BEAM_TILE; j++) {
                        const uint32_t b = b0 + (j < nb ? j : nb - 1u);      // (past the last beam: its weights again, a sum nobody stores)
                        const double2 w = s_beam_w[b * a.n_rx + r0 + r];
                        rts_beam_add(r0 + r == 0u, w.x, w.y, z[r].x, z[r].y, &y[j].x, &y[j].y);
                    }
                }
            }
        }
#pragma unroll
        for (uint32_t j = 0; j < RTS_BEAM_BEAM_TILE; j++) {
            if (j < nb) {
                const uint64_t o = (uint64_t)(b0 + j) * a.cells + c;
                if (MODE == RTS_BEAM_OUT_COMPLEX) ((double2*)a.out)[o] = y[j];
                else if (MODE == RTS_BEAM_OUT_POWER) ((double*)a.out)[o] = rts_beam_power(y[j].x, y[j].y);
                else rts_beam_peak_push(&pk, b0 + j, rts_beam_power(y[j].x, y[j].y));
            }
        }
    }
    if (MODE == RTS_BEAM_OUT_PEAK) {
        double2 v; rts_beam_peak_finish(&pk, a.n_beams, &v.x, &v.y);
        ((double2*)a.out)[c] = v;
    }
}

// in: the source's receiver 0, row first_row (device); rx_stride: its n_rows_in n_bins; weights: the call's table on the device
// (rts_cube_array_api.hip uploads it on the stream before this: RtsCubeState::beam.w)
int rts_cube_beam_device(RtsContext* c, const RtsBeamParams& p, const RtsBeamPlan& plan, const double* in, uint64_t rx_stride, const double* weights, void* out)
{
    RtsBeamArgs a;
    a.in = (const double2*)in; a.rx_stride = rx_stride; a.cells = plan.cells; a.w = (const double2*)weights;
    a.n_rx = c->cube.params.n_rx; a.n_beams = p.n_beams; a.rx_tiles = plan.rx_tiles; a.out = out;
    void (*k)(const RtsBeamArgs) = (p.flags & RTS_BEAM_PEAK) ? k_cube_beam<RTS_BEAM_OUT_PEAK> : (p.flags & RTS_BEAM_POWER) ? k_cube_beam<RTS_BEAM_OUT_POWER> : k_cube_beam<RTS_BEAM_OUT_COMPLEX>;
    RTS_HIP(hipFuncSetAttribute((const void*)k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)plan.lds));
    k<<<plan.groups, RTS_BEAM_THREADS, plan.lds, c->stream>>>(a);
    RTS_HIP(hipGetLastError());
    return RTS_OK;
}
