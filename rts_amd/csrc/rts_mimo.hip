// rts_mimo.hip -- MIMO radar on the device (include/rts_amd.h: rts_cube_bank): k_mimo_bank, the matched-filter bank.  The term, the
// order of a sum, the code multiply and the plan of the launch are rts_mimo.h, shared with the host evaluator.  No atomics and no
// MFMA (its accumulation is fused; the tree here is uncontracted): identical bits from run to run and on the host.
#include <hip/hip_runtime.h>
#include "rts_internal.h"
#include "rts_mimo.h"

struct RtsBankArgs {
    const double2* cube;              // receiver 0, row 0, bin 0 of the attached cube
    double2* out;                     // [n_waves n_rx][n_rows][n_bins]
    const double* tab;                // the staged table: the waveforms' samples, then the code table
    uint64_t rx_stride;               // elements between two receivers
    uint32_t n_rx, first, n_rows, n_bins, n_waves, tiles, S, code;      // code: the table holds one, at code_off
    uint64_t code_off;
    uint32_t M[RTS_BANK_MAX_WAVES], off[RTS_BANK_MAX_WAVES];
};

// One workgroup per (tile, row, receiver, group of G waveforms) -- rts_mimo.h: thread t owns J consecutive outputs of each of the
// group's waveforms; the row's samples are staged once, in J planes (sample i: plane i mod J, slot i / J), zeros beyond the row; the
// registers wa hold the samples J (t + q) .. J (t + q) + J - 1 of the tile, wb the next J.  At m = J q + c output j reads sample
// J (t + q) + c + j: wa[c + j], or wb[c + j - J].  Every index below is a constant after unrolling.  A waveform shorter than the
// group's longest, or missing from the last group, ends by the wave-uniform test m < Mw.
template <uint32_t G>
__global__ void __launch_bounds__(RTS_MIMO_THREADS) k_mimo_bank(const RtsBankArgs a)
{
    extern __shared__ __attribute__((aligned(16))) double2 s_y[];               // [J][S]
    constexpr uint32_t J = RTS_MIMO_J;
    const uint32_t t = threadIdx.x, S = a.S;
    uint32_t b = blockIdx.x;
    const uint32_t tile = b % a.tiles; b /= a.tiles;
    const uint32_t row = b % a.n_rows; b /= a.n_rows;
    const uint32_t r = b % a.n_rx, w0 = (b / a.n_rx) * G;
    uint32_t Mw[G], Mg = 0u; const double* sw[G];
#pragma unroll
    for (uint32_t w = 0; w < G; w++) {
        const bool have = w0 + w < a.n_waves;
        const uint32_t tw = have ? w0 + w : 0u;                                  // (no index beyond the tables, not even one that is not used)
        Mw[w] = have ? a.M[tw] : 0u; sw[w] = a.tab + a.off[tw];
        Mg = Mw[w] > Mg ? Mw[w] : Mg;
    }
    const uint32_t Q = (Mg + J - 1u) / J, U = RTS_MIMO_THREADS + Q, n0 = tile * RTS_BANK_TILE;      // (U <= S: the plan's Q is the set's)
    const double2* __restrict__ y = a.cube + (uint64_t)r * a.rx_stride + ((uint64_t)a.first + row) * a.n_bins;
    for (uint32_t e = t; e < J * U; e += RTS_MIMO_THREADS) {
        const uint64_t n = (uint64_t)n0 + e;
        s_y[(e % J) * S + e / J] = n < a.n_bins ? y[n] : make_double2(0.0, 0.0);
    }
    __syncthreads();
    double zr[G][J], zi[G][J];
#pragma unroll
    for (uint32_t w = 0; w < G; w++)
#pragma unroll
        for (uint32_t j = 0; j < J; j++) { zr[w][j] = 0.0; zi[w][j] = 0.0; }
    double2 wa[J], wb[J];
#pragma unroll
    for (uint32_t k = 0; k < J; k++) wa[k] = s_y[k * S + t];
    for (uint32_t q = 0; q < Q; q++) {
#pragma unroll
        for (uint32_t k = 0; k < J; k++) wb[k] = s_y[k * S + t + q + 1u];       // (t + q + 1 <= U - 1)
#pragma unroll
        for (uint32_t c = 0; c < J; c++) {
            const uint32_t m = J * q + c;
#pragma unroll
            for (uint32_t w = 0; w < G; w++) {
                if (m < Mw[w]) {
                    const double sr = sw[w][2 * m], si = sw[w][2 * m + 1];
#pragma unroll
                    for (uint32_t j = 0; j < J; j++) {
                        const double2 v = c + j < J ? wa[(c + j) % J] : wb[(c + j) % J];
                        rts_bank_term(v.x, v.y, sr, si, &zr[w][j], &zi[w][j]);
                    }
                }
            }
        }
#pragma unroll
        for (uint32_t k = 0; k < J; k++) wa[k] = wb[k];
    }
#pragma unroll
    for (uint32_t w = 0; w < G; w++) {
        if (w0 + w >= a.n_waves) continue;
        double cr = 0.0, ci = 0.0;
        if (a.code) { const double* c = a.tab + a.code_off + 2 * ((uint64_t)(w0 + w) * a.n_rows + row); cr = c[0]; ci = c[1]; }
        double2* z = a.out + (((uint64_t)(w0 + w) * a.n_rx + r) * a.n_rows + row) * a.n_bins;
#pragma unroll
        for (uint32_t j = 0; j < J; j++) {
            const uint64_t n = (uint64_t)n0 + J * t + j;
            if (n >= a.n_bins) continue;
            double2 v = make_double2(zr[w][j], zi[w][j]);
            if (a.code) rts_bank_code(cr, ci, zr[w][j], zi[w][j], &v.x, &v.y);
            z[n] = v;
        }
    }
}

template <uint32_t G>
static int rts_bank_launch(RtsContext* c, const RtsBankArgs& a, const RtsBankPlan& plan)
{
    RTS_HIP(hipFuncSetAttribute((const void*)k_mimo_bank<G>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)plan.lds));
    k_mimo_bank<G><<<plan.blocks, RTS_MIMO_THREADS, plan.lds, c->stream>>>(a);
    RTS_HIP(hipGetLastError());
    return RTS_OK;
}

int rts_cube_bank_device(RtsContext* c, const RtsBankParams& p, const RtsBankPlan& plan, const uint32_t* M, const double* tab, bool code, double* out)
{
    const RtsCubeParams& q = c->cube.params;
    RtsBankArgs a;
    a.cube = (const double2*)c->cube.p; a.out = (double2*)out; a.tab = tab; a.rx_stride = (uint64_t)q.n_pulses * q.n_bins;
    a.n_rx = q.n_rx; a.first = p.first_pulse; a.n_rows = p.n_pulses; a.n_bins = q.n_bins; a.n_waves = p.n_waves; a.tiles = plan.tiles; a.S = plan.S;
    a.code = code ? 1u : 0u; a.code_off = plan.code_off;
    for (uint32_t t = 0; t < RTS_BANK_MAX_WAVES; t++) { a.M[t] = t < p.n_waves ? M[t] : 0u; a.off[t] = plan.off[t]; }
    switch (plan.group) {
        case 4u: return rts_bank_launch<4u>(c, a, plan);
        case 2u: return rts_bank_launch<2u>(c, a, plan);
        default: return rts_bank_launch<1u>(c, a, plan);
    }
}
