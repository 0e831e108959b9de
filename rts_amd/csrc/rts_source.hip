// rts_source.hip -- clutter and jammer sources on the device (include/rts_amd.h: rts_cube_add_sources): k_cube_sources.
// The rules (pole, scale, draw, recursion, partials, tree) and the plan of the launch are rts_source.h, shared with the host evaluator.
#include <hip/hip_runtime.h>
#include "rts_internal.h"
#include "rts_source.h"

// The shape follows from the sum rule.  A wave owns ONE range bin for all pulses; lane j is partial j: it keeps the states c of the
// patches k = j + 64 i (i < NS) in registers (2 NS doubles) with their g s (NS doubles), walks the pulses, and per pulse
//   * turns each state by its pole (LDS, 16 bytes per lane and slot) and, only where g != 0, adds the draw, slot after slot through
//     ONE copy of the generator -- patches of rho = 1 never reach it, and a wave whose lanes all hold such patches branches around it;
//   * per receiver adds its patches' terms spatial (x) c in ascending k (the table is [n_rx][K] in LDS: consecutive lanes read
//     consecutive 16-byte entries) and combines the 64 partials by __shfl_down over 32, 16, 8, 4, 2, 1 lanes (rts_src_join: the
//     live mask of the call says which partials exist), RTS_SRC_RX_TILE receivers side by side; lane 0 puts the totals into the
//     workgroup's staging block.
// The RTS_SRC_WAVES waves of a workgroup take adjacent bins.  After stage_pulses pulses the workgroup adds the staged totals
// [pulse][rx][bin of the tile] to the cube: thread e takes bin e % 8 of row e / 8, so eight consecutive lanes read, add and write
// one 128-byte run of a cube row.  A bin of profile 0 (or beyond the cube) computes nothing and is skipped by the flush.
#define RTS_SRC_RX_TILE 4u
struct RtsSrcArgs {
    double2* cube;
    const double2* tab;               // spatial^T [n_rx][K] | pole [K] | (g, power) [K] | profile [n_bins] doubles (rts_src_table)
    uint32_t n_rx, n_pulses, n_bins, K, stage_pulses, has_profile;
    uint64_t seed, live;
};

template <int NS> __global__ void __launch_bounds__(RTS_SRC_THREADS) k_cube_sources(const RtsSrcArgs a)
{
    extern __shared__ __attribute__((aligned(16))) double2 s_src[];              // spatial^T [n_rx][K], pole [K], staging [stage_pulses][n_rx][TILE]
    __shared__ uint32_t s_on[RTS_SRC_WAVES];
    const uint32_t t = threadIdx.x, wave = t / RTS_SRC_LANES, lane = t % RTS_SRC_LANES, K = a.K, n_rx = a.n_rx;
    const double2* s_sp = s_src;
    const double2* s_pole = s_src + (size_t)n_rx * K;
    double2* s_out = s_src + (size_t)(n_rx + 1u) * K;
    for (uint32_t i = t; i < (n_rx + 1u) * K; i += RTS_SRC_THREADS) s_src[i] = a.tab[i];
    const double2* gp = a.tab + (size_t)(n_rx + 1u) * K;
    const double* prof = (const double*)(gp + K);
    const uint32_t bin0 = blockIdx.x * RTS_SRC_TILE, bin = bin0 + wave;
    double profile = 0.0;
    if (bin < a.n_bins) profile = a.has_profile ? prof[bin] : 1.0;
    const bool on = profile != 0.0;                                              // (wave-uniform)
    if (lane == 0u) s_on[wave] = on ? 1u : 0u;

    double cr[NS], ci[NS], gs[NS];
    uint32_t lv = 0u, dr = 0u;                                                   // bit i: slot i holds a patch that counts; ... whose g != 0
#pragma unroll
    for (int i = 0; i < NS; i++) { cr[i] = 0.0; ci[i] = 0.0; gs[i] = 0.0; }
    // (the slot loops that draw are NOT unrolled -- one copy of the generator, one draw in flight, and the slot's registers are
    // picked by a chain of compile-time indices under the wave-uniform i: unrolled, the sixteen draws of NS = 16 ran side by side
    // and spilled)
    if (on) {
        for (int i = 0; i < NS; i++) {
            const uint32_t k = lane + RTS_SRC_LANES * (uint32_t)i;
            if (k < K) {
                const double2 g = gp[k];
                if (rts_src_patch_live(g.y)) {
                    const double s = rts_src_scale(g.y, profile);
                    double wr, wi, c0r, c0i; rts_src_draw(a.seed, bin, 0u, k, &wr, &wi);
                    rts_src_first(s, wr, wi, &c0r, &c0i);
                    const double gsi = g.x * s;
#pragma unroll
                    for (int ii = 0; ii < NS; ii++) if (ii == i) { cr[ii] = c0r; ci[ii] = c0i; gs[ii] = gsi; }
                    lv |= 1u << i;
                    if (g.x != 0.0) dr |= 1u << i;
                }
            }
        }
    }
    __syncthreads();

    for (uint32_t p0 = 0; p0 < a.n_pulses; p0 += a.stage_pulses) {
        const uint32_t np = a.n_pulses - p0 < a.stage_pulses ? a.n_pulses - p0 : a.stage_pulses;
        if (on) {
            for (uint32_t pp = 0; pp < np; pp++) {
                const uint32_t pulse = p0 + pp;
                if (pulse) {
#pragma unroll
                    for (int i = 0; i < NS; i++) {
                        if ((lv >> i) & 1u) {
                            const double2 pole = s_pole[lane + RTS_SRC_LANES * (uint32_t)i];
                            rts_src_turn(pole.x, pole.y, &cr[i], &ci[i]);
                        }
                    }
                    if (__any(dr != 0u)) {                                       // (rho = 1 everywhere: the generator is never reached)
                        for (int i = 0; i < NS; i++) {
                            if ((dr >> i) & 1u) {
                                double wr, wi; rts_src_draw(a.seed, bin, pulse, lane + RTS_SRC_LANES * (uint32_t)i, &wr, &wi);
#pragma unroll
                                for (int ii = 0; ii < NS; ii++) if (ii == i) rts_src_innovate(gs[ii], wr, wi, &cr[ii], &ci[ii]);
                            }
                        }
                    }
                }
                // RTS_SRC_RX_TILE receivers at a time: their sums and their trees are independent, so the cross-lane moves of one hide
                // behind the others'.  A step of the tree that no partial reaches (live >> s == 0: fewer than s + 1 partials, e.g.
                // every step of a single jammer) is skipped whole -- it would change nothing.
                for (uint32_t rx0 = 0; rx0 < n_rx; rx0 += RTS_SRC_RX_TILE) {
                    double ar[RTS_SRC_RX_TILE], ai[RTS_SRC_RX_TILE];
#pragma unroll
                    for (uint32_t q = 0; q < RTS_SRC_RX_TILE; q++) {
                        const uint32_t rx = rx0 + q < n_rx ? rx0 + q : n_rx - 1u;      // (past the last receiver: its terms again, a total nobody stores)
                        ar[q] = 0.0; ai[q] = 0.0;
                        bool have = false;
#pragma unroll
                        for (int i = 0; i < NS; i++) {
                            if ((lv >> i) & 1u) {
                                const double2 sp = s_sp[(size_t)rx * K + lane + RTS_SRC_LANES * (uint32_t)i];
                                rts_src_term(have, sp.x, sp.y, cr[i], ci[i], &ar[q], &ai[q]);
                                have = true;
                            }
                        }
                    }
                    uint64_t live = a.live;
#pragma unroll
                    for (uint32_t s = RTS_SRC_LANES / 2u; s >= 1u; s >>= 1) {
                        if (live >> s) {                                             // (uniform: the mask is the call's)
#pragma unroll
                            for (uint32_t q = 0; q < RTS_SRC_RX_TILE; q++) {
                                const double br = __shfl_down(ar[q], s, RTS_SRC_LANES), bi = __shfl_down(ai[q], s, RTS_SRC_LANES);
                                if (lane < s) rts_src_join(live, lane, s, br, bi, &ar[q], &ai[q]);
                            }
                        }
                        live = rts_src_tree_next(live, s);
                    }
                    if (lane == 0u) {
#pragma unroll
                        for (uint32_t q = 0; q < RTS_SRC_RX_TILE; q++)
                            if (rx0 + q < n_rx) s_out[((size_t)pp * n_rx + rx0 + q) * RTS_SRC_TILE + wave] = make_double2(ar[q], ai[q]);
                    }
                }
            }
        }
        __syncthreads();
        const uint32_t n = np * n_rx * RTS_SRC_TILE;
        for (uint32_t e = t; e < n; e += RTS_SRC_THREADS) {
            const uint32_t w = e % RTS_SRC_TILE, row = e / RTS_SRC_TILE, pp = row / n_rx, rx = row % n_rx;
            if (s_on[w]) {                                                       // (a bin beyond the cube is off)
                const size_t at = ((size_t)rx * a.n_pulses + p0 + pp) * a.n_bins + bin0 + w;
                const double2 add = s_out[e];
                double2 v = a.cube[at];
                v.x = v.x + add.x; v.y = v.y + add.y;
                a.cube[at] = v;
            }
        }
        __syncthreads();
    }
}

// table: the call's table on the device (rts_cube_api.hip uploads it on the stream before this: RtsCubeState::source.tab); live: the
// partials that exist (rts_src_live_mask, not 0)
int rts_cube_sources_device(RtsContext* c, const RtsSrcPlan& plan, uint32_t K, bool has_profile, uint64_t seed, uint64_t live, const double* table)
{
    const RtsCubeParams& q = c->cube.params;
    RtsSrcArgs a;
    a.cube = (double2*)c->cube.p; a.tab = (const double2*)table;
    a.n_rx = q.n_rx; a.n_pulses = q.n_pulses; a.n_bins = q.n_bins; a.K = K; a.stage_pulses = plan.stage_pulses; a.has_profile = has_profile ? 1u : 0u;
    a.seed = seed; a.live = live;
    void (*k)(const RtsSrcArgs) = plan.slots == 1u ? k_cube_sources<1> : plan.slots == 2u ? k_cube_sources<2> : plan.slots == 4u ? k_cube_sources<4> :
                                  plan.slots == 8u ? k_cube_sources<8> : k_cube_sources<16>;
    RTS_HIP(hipFuncSetAttribute((const void*)k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)plan.lds));
    k<<<plan.groups, RTS_SRC_THREADS, plan.lds, c->stream>>>(a);
    RTS_HIP(hipGetLastError());
    return RTS_OK;
}
