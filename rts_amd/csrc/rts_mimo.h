// rts_mimo.h -- MIMO radar (include/rts_amd.h: RtsBankParams): the matched-filter bank that takes the transmitters of one cube apart --
// the term and the order of one output's sum, the slow-time code's multiply, the parameter rule, the host-only plan of the launch and
// the host evaluator, shared by the kernel (rts_mimo.hip) and rts_bank_eval.  The sum is k_cube_compress's tree (rts_render.hip): it
// starts at +0.0, runs over m ascending, forms no term beyond the row, and rounds every operation on its own (-ffp-contract=off).
// Includes nothing of HIP: it compiles with any host compiler and is tested without a GPU (tests/test_mimo_host.py,
// tests/mimo/mimo_main.cpp).
//
// The bank does not bound n_waves * n_rx: it writes as many virtual elements as the set and the cube give.  What can be ATTACHED
// afterwards and handed to the array families is bounded by their RTS_BEAM_MAX_RX (64): 16 waveforms on 4 receivers fill it.
#pragma once
#include <math.h>
#include <stdint.h>
#include <stddef.h>
#include "../../include/rts_amd.h"
#include "rts_cube_args.h"

#ifndef RTS_HD
#define RTS_HD static inline          // (a host compiler; the library's units have rts_device_math.h's __host__ __device__ form)
#endif

// ---- one term: z += y conj(s), the four products and the four sums each rounded on its own, in k_cube_compress's order
RTS_HD void rts_bank_term(double yr, double yi, double sr, double si, double* zr, double* zi)
{
    *zr += yr * sr + yi * si;
    *zi += yi * sr - yr * si;
}
// ---- the slow-time code: conj(c) z.  A zero entry gives zeros by this multiply, not by a skip
RTS_HD void rts_bank_code(double cr, double ci, double zr, double zi, double* outr, double* outi)
{
    *outr = cr * zr + ci * zi;
    *outi = cr * zi - ci * zr;
}
// ---- one output: bin n of one row y of n_bins interleaved samples against M interleaved waveform samples.  A term with
// n + m >= n_bins is not formed.
// (The kernel forms such terms on a +0.0 sample it staged itself and gets the same bits: the waveform is finite, so the products are
// zeros and their sum a zero; a running sum that started at +0.0 is never -0.0 -- x + y is -0.0 only when both are --, and adding a
// zero of either sign to anything but -0.0 leaves it as it is.)
RTS_HD void rts_bank_cell(const double* y, uint32_t n_bins, uint32_t n, const double* s, uint32_t M, double* zr, double* zi)
{
    double ar = 0.0, ai = 0.0;
    const uint32_t mm = M < n_bins - n ? M : n_bins - n;
    for (uint32_t m = 0; m < mm; m++) rts_bank_term(y[2 * (size_t)(n + m)], y[2 * (size_t)(n + m) + 1], s[2 * (size_t)m], s[2 * (size_t)m + 1], &ar, &ai);
    *zr = ar; *zi = ai;
}

// ---- the parameter rule, beside the waveforms' own (the RtsWaveform rule of rts_cube_set_waveform, applied to each by the entry
// points between 3 and 4).  0, or the number of the rule that broke: 1 reserved fields; 2 n_waves outside 1 .. RTS_BANK_MAX_WAVES;
// 3 null waveform array; 4 the span: at least one pulse, inside the cube
static inline int rts_bank_rule(const RtsBankParams* p, uint32_t n_pulses)
{
    if (p->reserved[0] || p->reserved[1]) return 1;
    if (p->n_waves == 0u || p->n_waves > RTS_BANK_MAX_WAVES) return 2;
    if (!p->waves) return 3;
    if (!rts_span_inside(p->first_pulse, p->n_pulses, n_pulses, false, true)) return 4;
    return 0;
}
// the code table [n_waves][n_rows] interleaved: the index of its first value that is not finite, or -1 (a null table has none)
static inline int64_t rts_bank_code_bad(const double* code, uint32_t n_waves, uint32_t n_rows)
{
    if (code) for (uint64_t i = 0; i < 2ull * n_waves * n_rows; i++) if (!(code[i] >= -1.7976931348623157e308 && code[i] <= 1.7976931348623157e308)) return (int64_t)i;
    return -1;
}

// ---- the plan of the launch (host only), from the shape and the waveforms' lengths alone.
// k_mimo_bank: one workgroup of RTS_MIMO_THREADS threads per (tile of RTS_BANK_TILE output bins, row, receiver, group of `group`
// consecutive waveforms).  Thread t owns the RTS_MIMO_J CONSECUTIVE outputs n0 + J t .. n0 + J t + J - 1 of every waveform of the
// group.  The workgroup stages the row's samples n0 .. n0 + J U - 1 (zeros beyond the row), U = RTS_MIMO_THREADS + ceil(max M / J),
// once, as J planes of S >= U slots: sample i sits in plane i mod J at slot i / J, so that the lanes of a wave, whose samples lie J
// apart, read consecutive 16-byte slots.  A thread keeps the J samples from its first output at m = J q in registers and reads the
// next J while it works: J reads serve J steps of m, each step J outputs of every waveform of the group -- 8 J `group` f64 operations
// per 16-byte LDS read, where k_cube_compress has 8.  The waveform's sample of a term is one address for the wave (a scalar load).
// The window and the grouping change which sums are in flight together, never the order of a sum.
// `group`: 4 waveforms per thread share one staging; while the grid then has fewer than RTS_MIMO_FILL_BLOCKS workgroups (four on
// each of 256 CUs) the group is halved, so that a small cube still fills the device.  LDS: 16 J S bytes, 73 984 at the longest
// waveform: it bounds neither n_bins nor n_waves.
#define RTS_MIMO_THREADS 128u
#define RTS_MIMO_J 4u
#define RTS_MIMO_MAX_GROUP 4u
#define RTS_MIMO_FILL_BLOCKS 1024u
#define RTS_MIMO_MAX_GRID 2147483647u
#if RTS_MIMO_THREADS * RTS_MIMO_J != RTS_BANK_TILE
#error "a workgroup's threads times their outputs is the tile"
#endif
struct RtsBankPlan {
    uint32_t tiles, group, groups, max_M, Q, S, blocks;
    uint32_t off[RTS_BANK_MAX_WAVES];      // where waveform t's samples begin in the staged table, in doubles
    size_t lds, out_doubles, tab_doubles, code_off;      // code_off: where the code table begins in the staged table (tab_doubles without one)
    bool supported;
};
// M[t]: the waveforms' lengths (each 1 .. RTS_WAVEFORM_MAX_SAMPLES); n_rows: the span's
static inline RtsBankPlan rts_bank_plan(uint32_t n_rx, uint32_t n_rows, uint32_t n_bins, uint32_t n_waves, const uint32_t* M, bool code)
{
    RtsBankPlan p;
    p.supported = n_rx >= 1u && n_rows >= 1u && n_bins >= 1u && n_waves >= 1u && n_waves <= RTS_BANK_MAX_WAVES;
    p.tiles = (uint32_t)(((uint64_t)n_bins + RTS_BANK_TILE - 1u) / RTS_BANK_TILE);
    p.max_M = 0u; p.tab_doubles = 0u;
    for (uint32_t t = 0; t < RTS_BANK_MAX_WAVES; t++) {
        p.off[t] = (uint32_t)p.tab_doubles;
        if (p.supported && t < n_waves) { if (M[t] > p.max_M) p.max_M = M[t]; p.tab_doubles += 2u * (size_t)M[t]; }
    }
    p.code_off = p.tab_doubles;
    if (p.supported && code) p.tab_doubles += 2u * (size_t)n_waves * n_rows;
    p.Q = (p.max_M + RTS_MIMO_J - 1u) / RTS_MIMO_J;
    p.S = (RTS_MIMO_THREADS + p.Q + 15u) / 16u * 16u + 4u;      // 4 mod 16: the staging's writes, J planes apart, fall on different banks
    p.lds = 16u * (size_t)RTS_MIMO_J * p.S;
    // the output's cells, V n_rows n_bins with V = n_waves n_rx, without a product that could wrap
    const uint64_t V = (uint64_t)n_waves * n_rx, row_cells = (uint64_t)n_rows * n_bins;
    if (p.supported && row_cells > RTS_BANK_MAX_CELLS / V) p.supported = false;
    p.out_doubles = p.supported ? 2u * (size_t)(V * row_cells) : 0u;
    // the grid: (tile, row, receiver, group) flattened
    p.group = RTS_MIMO_MAX_GROUP; p.groups = 0u; p.blocks = 0u;
    if (p.supported) {
        const uint64_t base = (uint64_t)p.tiles * n_rows * n_rx;      // (<= the output's cells / n_waves + rows: no wrap)
        while (p.group > 1u && base * ((n_waves + p.group - 1u) / p.group) < RTS_MIMO_FILL_BLOCKS) p.group /= 2u;
        p.groups = (n_waves + p.group - 1u) / p.group;
        if (base > RTS_MIMO_MAX_GRID / p.groups) p.supported = false; else p.blocks = (uint32_t)(base * p.groups);
    }
    return p;
}

// ---- the evaluator (validated by the caller): cube [n_rx][n_pulses][n_bins] interleaved -> out [n_waves n_rx][p->n_pulses][n_bins]
// interleaved, virtual element t n_rx + r; code [n_waves][p->n_pulses] interleaved or null.  Reads only the span's rows.
static inline void rts_bank_eval_host(const RtsCubeParams* q, const double* cube, const RtsBankParams* p, double* out)
{
    const size_t rx_stride = (size_t)q->n_pulses * q->n_bins;
    for (uint32_t t = 0; t < p->n_waves; t++) for (uint32_t r = 0; r < q->n_rx; r++) for (uint32_t row = 0; row < p->n_pulses; row++) {
        const double* y = cube + 2 * ((size_t)r * rx_stride + (size_t)(p->first_pulse + row) * q->n_bins);
        double* z = out + 2 * ((((size_t)t * q->n_rx + r) * p->n_pulses + row) * q->n_bins);
        const double* c = p->code ? p->code + 2 * ((size_t)t * p->n_pulses + row) : nullptr;
        for (uint32_t n = 0; n < q->n_bins; n++) {
            double zr, zi;
            rts_bank_cell(y, q->n_bins, n, p->waves[t].samples, p->waves[t].n_samples, &zr, &zi);
            if (c) rts_bank_code(c[0], c[1], zr, zi, &z[2 * (size_t)n], &z[2 * (size_t)n + 1]); else { z[2 * (size_t)n] = zr; z[2 * (size_t)n + 1] = zi; }
        }
    }
}
