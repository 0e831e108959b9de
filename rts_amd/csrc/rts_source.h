// rts_source.h -- clutter and jammer sources (include/rts_amd.h: RtsSourceParams): the pole and the gain of a patch, its scale on a
// bin, its draw, the recursion step, the complex product, the partials and their tree, the validation, the host evaluator and the
// host-only plan of the launch, each written once and shared by the kernel (rts_source.hip: k_cube_sources), the entry points
// (rts_cube_api.hip) and rts_sources_eval.  Fixed trees of IEEE basic operations in the operand order of the header text, compiled
// with -ffp-contract=off; the draw's log, cos and sin are the platform's (rts_noise.h).  Includes nothing of HIP: it compiles with
// any host compiler and is tested without a GPU (tests/test_source_host.py, tests/source/source_main.cpp).
#pragma once
#include <math.h>
#include <stdint.h>
#include <stddef.h>
#include "../../include/rts_amd.h"
#include "rts_beat.h"             // RTS_HD, RTS_PI, rts_beat_sincos_turns
#include "rts_noise.h"

#define RTS_SRC_LANES 64u                                         // the partials of the sum
#define RTS_SRC_MAX_SLOTS (RTS_SRC_MAX_PATCHES / RTS_SRC_LANES)   // patches of one partial, at most
#define RTS_SRC_SIGMA 0.70710678118654757                         // sqrt(0.5), correctly rounded: the draws have unit power

RTS_HD bool rts_src_finite(double x) { return x - x == 0.0; }

// a (x) b = (ar br - ai bi, ar bi + ai br)
RTS_HD void rts_src_mul(double ar, double ai, double br, double bi, double* re, double* im)
{
    *re = ar * br - ai * bi; *im = ar * bi + ai * br;
}

// s_kr, and w(k, r, p): Philox counter (bin, pulse, patch, 1)
RTS_HD double rts_src_scale(double power, double profile) { return sqrt(power * profile); }
RTS_HD void rts_src_draw(uint64_t seed, uint32_t bin, uint32_t pulse, uint32_t patch, double* wr, double* wi)
{
    rts_noise_sample4(seed, bin, pulse, patch, 1u, RTS_SRC_SIGMA, wr, wi);
}

// the recursion: c_0 = s w;  c_p = pole (x) c_p-1, then + (g s) w where g != 0
RTS_HD void rts_src_first(double s, double wr, double wi, double* cr, double* ci) { *cr = s * wr; *ci = s * wi; }
RTS_HD void rts_src_turn(double pr, double pi, double* cr, double* ci)
{
    double re, im; rts_src_mul(pr, pi, *cr, *ci, &re, &im);
    *cr = re; *ci = im;
}
RTS_HD void rts_src_innovate(double gs, double wr, double wi, double* cr, double* ci) { *cr = *cr + gs * wr; *ci = *ci + gs * wi; }

// a partial takes the term spatial (x) c of its next patch; have: it has a term already (else this one is the start value)
RTS_HD void rts_src_term(bool have, double sr, double si, double cr, double ci, double* ar, double* ai)
{
    double tr, ti; rts_src_mul(sr, si, cr, ci, &tr, &ti);
    if (have) { *ar = *ar + tr; *ai = *ai + ti; } else { *ar = tr; *ai = ti; }
}

// The tree over the 64 partials, steps s = 32, 16, 8, 4, 2, 1: partial j < s takes partial j + s.  live: bit j set where partial j
// exists; a partial that does not exist is left out, and where only j + s exists it becomes j.  The total ends in partial 0.
RTS_HD void rts_src_join(uint64_t live, uint32_t j, uint32_t s, double br, double bi, double* ar, double* ai)
{
    if (!((live >> (j + s)) & 1u)) return;
    if ((live >> j) & 1u) { *ar = *ar + br; *ai = *ai + bi; } else { *ar = br; *ai = bi; }
}
RTS_HD uint64_t rts_src_tree_next(uint64_t live, uint32_t s) { return (live | (live >> s)) & ((1ull << s) - 1ull); }

// patch k counts (power_k > 0; a patch of power 0 is skipped); the partials that exist
RTS_HD bool rts_src_patch_live(double power) { return power > 0.0; }
static inline uint64_t rts_src_live_mask(uint32_t K, const double* power)
{
    uint64_t live = 0;
    for (uint32_t k = 0; k < K; k++) if (rts_src_patch_live(power[k])) live |= 1ull << (k % RTS_SRC_LANES);
    return live;
}

// ---- host only from here.
// pole_k and g_k (rho NULL: 1)
static inline void rts_src_pole(double doppler, double rho, double* pr, double* pi, double* g)
{
    double s, c; rts_beat_sincos_turns(doppler, &s, &c);
    *pr = rho * c; *pi = rho * s;
    *g = sqrt(1.0 - rho * rho);
}

// validation of the record for a cube of n_rx receivers and n_bins bins: 0, or the number of the rule it breaks (rts_cube_api.hip
// words the message; *bad: the index of the entry for 10 .. 14)
//   1 n_patches  2 flags  3 reserved  4 null spatial  5 null power  6 null doppler  7 n_rx  8 n_patches * n_rx
//   10 spatial  11 power  12 doppler  13 rho  14 range_profile
static inline int rts_src_check(const RtsSourceParams* p, uint32_t n_rx, uint32_t n_bins, uint32_t* bad)
{
    if (p->n_patches == 0u || p->n_patches > RTS_SRC_MAX_PATCHES) return 1;
    if (p->flags) return 2;
    if (p->reserved[0] || p->reserved[1]) return 3;
    if (!p->spatial) return 4;
    if (!p->power) return 5;
    if (!p->doppler) return 6;
    if (n_rx > RTS_BEAM_MAX_RX) return 7;
    if ((uint64_t)p->n_patches * n_rx > RTS_SRC_MAX_TABLE) return 8;
    for (uint32_t i = 0; i < 2u * p->n_patches * n_rx; i++) if (!rts_src_finite(p->spatial[i])) { *bad = i / 2u; return 10; }
    for (uint32_t k = 0; k < p->n_patches; k++) if (!rts_src_finite(p->power[k]) || !(p->power[k] >= 0.0)) { *bad = k; return 11; }
    for (uint32_t k = 0; k < p->n_patches; k++) if (!rts_src_finite(p->doppler[k])) { *bad = k; return 12; }
    if (p->rho) for (uint32_t k = 0; k < p->n_patches; k++) if (!(p->rho[k] >= 0.0) || !(p->rho[k] <= 1.0)) { *bad = k; return 13; }
    if (p->range_profile) for (uint32_t r = 0; r < n_bins; r++) if (!rts_src_finite(p->range_profile[r]) || !(p->range_profile[r] >= 0.0)) { *bad = r; return 14; }
    return 0;
}

// ---- the plan of a launch, from the shape alone.  A wave owns ONE bin for all pulses: lane j keeps the states c of the patches
// k = j + 64 i (i < slots: 1, 2, 4, 8 or 16 register slots, the least that hold ceil(K / 64)) and is partial j of the sum.  A
// workgroup is RTS_SRC_WAVES waves on RTS_SRC_TILE = RTS_SRC_WAVES adjacent bins (128 bytes of a row); it keeps the spatial table
// (transposed, [n_rx][K]: consecutive lanes read consecutive entries) and the poles in LDS, stages the totals of stage_pulses pulses
// there ([stage_pulses][n_rx][RTS_SRC_TILE], at most RTS_SRC_STAGE_ROWS rows of 128 bytes) and then adds them to the cube, eight
// consecutive lanes on one 128-byte run.
// The table the call uploads, in doubles: spatial^T [n_rx][K][2] | pole [K][2] | (g, power) [K][2] | profile [n_bins] (if given).
#define RTS_SRC_WAVES 8u
#define RTS_SRC_TILE RTS_SRC_WAVES
#define RTS_SRC_THREADS (RTS_SRC_WAVES * RTS_SRC_LANES)
#define RTS_SRC_STAGE_ROWS 128u
#define RTS_SRC_STAGE_MAX_PULSES 16u
struct RtsSrcPlan { uint32_t groups, slots, stage_pulses; size_t lds, table_doubles; bool supported; };
static inline RtsSrcPlan rts_src_plan(uint32_t n_rx, uint32_t n_bins, uint32_t K, bool profile)
{
    RtsSrcPlan p;
    p.groups = (uint32_t)(((uint64_t)n_bins + RTS_SRC_TILE - 1u) / RTS_SRC_TILE);
    const uint32_t need = (K + RTS_SRC_LANES - 1u) / RTS_SRC_LANES;
    p.slots = 1u; while (p.slots < need) p.slots <<= 1;
    p.stage_pulses = n_rx ? RTS_SRC_STAGE_ROWS / n_rx : 1u;
    if (p.stage_pulses > RTS_SRC_STAGE_MAX_PULSES) p.stage_pulses = RTS_SRC_STAGE_MAX_PULSES;
    if (p.stage_pulses < 1u) p.stage_pulses = 1u;
    p.lds = 16u * ((size_t)K * n_rx + K + (size_t)p.stage_pulses * n_rx * RTS_SRC_TILE);
    p.table_doubles = 2u * ((size_t)K * n_rx + 2u * (size_t)K) + (profile ? n_bins : 0u);
    p.supported = n_rx >= 1u && n_rx <= RTS_BEAM_MAX_RX && K >= 1u && K <= RTS_SRC_MAX_PATCHES && (uint64_t)K * n_rx <= RTS_SRC_MAX_TABLE &&
                  p.slots <= RTS_SRC_MAX_SLOTS && p.groups >= 1u;
    return p;
}
// fills the table of the plan from a validated record
static inline void rts_src_table(const RtsSourceParams* p, uint32_t n_rx, uint32_t n_bins, double* tab)
{
    const uint32_t K = p->n_patches;
    double* sp = tab; double* pole = tab + 2u * (size_t)K * n_rx; double* gp = pole + 2u * (size_t)K; double* prof = gp + 2u * (size_t)K;
    for (uint32_t k = 0; k < K; k++) {
        for (uint32_t rx = 0; rx < n_rx; rx++) {
            sp[2u * ((size_t)rx * K + k)] = p->spatial[2u * ((size_t)k * n_rx + rx)];
            sp[2u * ((size_t)rx * K + k) + 1u] = p->spatial[2u * ((size_t)k * n_rx + rx) + 1u];
        }
        rts_src_pole(p->doppler[k], p->rho ? p->rho[k] : 1.0, &pole[2u * k], &pole[2u * k + 1u], &gp[2u * k]);
        gp[2u * k + 1u] = p->power[k];
    }
    if (p->range_profile) for (uint32_t r = 0; r < n_bins; r++) prof[r] = p->range_profile[r];
}

// ---- the evaluator (validated by the caller): adds to cube [n_rx][n_pulses][n_bins] interleaved.  work: rts_src_work_doubles(K)
// doubles -- pole [K][2], g [K], g s [K], c [K][2], the partials [64][2].
static inline size_t rts_src_work_doubles(uint32_t K) { return 6u * (size_t)K + 2u * RTS_SRC_LANES; }
static inline void rts_sources_eval_host(const RtsCubeParams* q, const RtsSourceParams* p, double* cube, double* work)
{
    const uint32_t K = p->n_patches, n_rx = q->n_rx, np = q->n_pulses, nb = q->n_bins;
    double* pole = work; double* g = pole + 2u * (size_t)K; double* gs = g + K; double* c = gs + K; double* part = c + 2u * (size_t)K;
    const uint64_t live0 = rts_src_live_mask(K, p->power);
    if (!live0) return;
    for (uint32_t r = 0; r < nb; r++) {
        const double profile = p->range_profile ? p->range_profile[r] : 1.0;
        if (profile == 0.0) continue;
        for (uint32_t k = 0; k < K; k++) {
            if (!rts_src_patch_live(p->power[k])) continue;
            double wr, wi;
            rts_src_pole(p->doppler[k], p->rho ? p->rho[k] : 1.0, &pole[2u * k], &pole[2u * k + 1u], &g[k]);
            const double s = rts_src_scale(p->power[k], profile);
            rts_src_draw(p->seed, r, 0u, k, &wr, &wi);
            rts_src_first(s, wr, wi, &c[2u * k], &c[2u * k + 1u]);
            gs[k] = g[k] * s;
        }
        for (uint32_t pl = 0; pl < np; pl++) {
            if (pl) for (uint32_t k = 0; k < K; k++) {
                if (!rts_src_patch_live(p->power[k])) continue;
                rts_src_turn(pole[2u * k], pole[2u * k + 1u], &c[2u * k], &c[2u * k + 1u]);
                if (g[k] != 0.0) {
                    double wr, wi; rts_src_draw(p->seed, r, pl, k, &wr, &wi);
                    rts_src_innovate(gs[k], wr, wi, &c[2u * k], &c[2u * k + 1u]);
                }
            }
            for (uint32_t rx = 0; rx < n_rx; rx++) {
                uint64_t have = 0;
                for (uint32_t k = 0; k < K; k++) {
                    if (!rts_src_patch_live(p->power[k])) continue;
                    const uint32_t j = k % RTS_SRC_LANES;
                    const double* sp = p->spatial + 2u * ((size_t)k * n_rx + rx);
                    rts_src_term((have >> j) & 1u, sp[0], sp[1], c[2u * k], c[2u * k + 1u], &part[2u * j], &part[2u * j + 1u]);
                    have |= 1ull << j;
                }
                uint64_t live = have;
                for (uint32_t s = RTS_SRC_LANES / 2u; s >= 1u; s >>= 1) {
                    for (uint32_t j = 0; j < s; j++) rts_src_join(live, j, s, part[2u * (j + s)], part[2u * (j + s) + 1u], &part[2u * j], &part[2u * j + 1u]);
                    live = rts_src_tree_next(live, s);
                }
                double* z = cube + 2u * (((size_t)rx * np + pl) * nb + r);
                z[0] = z[0] + part[0]; z[1] = z[1] + part[1];
            }
        }
    }
}
