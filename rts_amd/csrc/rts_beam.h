// rts_beam.h -- receive-array beamforming across the cube's receivers (include/rts_amd.h: RtsBeamParams): the term and the sum of a
// beam, the streaming peak over the beams of a cell, the host evaluator and the host-only plan of the launch, shared by the kernel
// (rts_beam.hip: k_cube_beam) and rts_beamform_eval.  Fixed trees of IEEE basic operations (the peak's offset: rts_cfar.h's
// log-parabola as it stands), compiled with -ffp-contract=off.  Includes nothing of HIP: it compiles with any host compiler and is
// tested without a GPU (tests/test_beam_host.py, tests/beam/beam_main.cpp).
#pragma once
#include <math.h>
#include <stdint.h>
#include <stddef.h>
#include "../../include/rts_amd.h"
#include "rts_cfar.h"

// conj(w) z = (wr zr + wi zi, wr zi - wi zr): four multiplies, one add, one subtract
RTS_HD void rts_beam_term(double wr, double wi, double zr, double zi, double* tr, double* ti)
{
    *tr = wr * zr + wi * zi; *ti = wr * zi - wi * zr;
}

// the sum so far plus the term of the next receiver; first: the term is the start value (receiver 0)
RTS_HD void rts_beam_add(bool first, double wr, double wi, double zr, double zi, double* yr, double* yi)
{
    double tr, ti; rts_beam_term(wr, wi, zr, zi, &tr, &ti);
    if (first) { *yr = tr; *yi = ti; } else { *yr += tr; *yi += ti; }
}

RTS_HD double rts_beam_power(double re, double im) { return re * re + im * im; }

// RTS_BEAM_PEAK of one cell, streaming: the beam powers are pushed in ascending beam order; held are the previous power, the best
// one (the FIRST beam that attains the largest power: a later beam replaces it only when strictly greater) and its two neighbours.
// No array of n_beams powers, so nothing is indexed.  With a NaN among the powers the reported beam is some beam, unspecified.
struct RtsBeamPeak { double prev, best, best_m, best_p; uint32_t b_best, next_is_neighbour; };
RTS_HD void rts_beam_peak_push(RtsBeamPeak* k, uint32_t b, double P)
{
    if (b == 0u) { k->best = P; k->best_m = 0.0; k->best_p = 0.0; k->b_best = 0u; k->next_is_neighbour = 1u; }
    else {
        if (k->next_is_neighbour) { k->best_p = P; k->next_is_neighbour = 0u; }
        if (P > k->best) { k->best_m = k->prev; k->best = P; k->best_p = 0.0; k->b_best = b; k->next_is_neighbour = 1u; }
    }
    k->prev = P;
}
// (P*, coordinate) after n_beams pushes: the offset is 0 at the first and the last beam (the beam axis does not wrap)
RTS_HD void rts_beam_peak_finish(const RtsBeamPeak* k, uint32_t n_beams, double* P, double* coordinate)
{
    const bool edge = k->b_best == 0u || k->b_best + 1u == n_beams;
    *P = k->best;
    *coordinate = (double)k->b_best + (edge ? 0.0 : rts_cfar_delta(k->best_m, k->best, k->best_p));
}

// ---- the plan of a launch (host only), from the shape alone.  The rows first_row .. first_row + n_rows - 1 of one receiver are
// contiguous in the input, and so is a beam's output: the call is a flat problem over cells = n_rows n_bins, one thread per cell,
// consecutive lanes on consecutive cells.  A workgroup of RTS_BEAM_THREADS threads stages the whole weight table (16 n_beams n_rx
// bytes, at most 64 KiB) in its LDS.  A thread keeps RTS_BEAM_RX_TILE receiver samples of its cell in registers and the running sums
// of RTS_BEAM_BEAM_TILE beams; with more receivers than one tile it walks the receiver tiles in ascending order per beam tile
// (the samples are read again from the caches), with at most one tile the samples are read once for all beams.  The tiles change
// which sums are in flight together, never the order of a sum: ascending receivers, the first term the start value.
#define RTS_BEAM_THREADS 256u
#define RTS_BEAM_RX_TILE 8u
#define RTS_BEAM_BEAM_TILE 16u
#define RTS_BEAM_MAX_GRID_X 2147483647u
struct RtsBeamPlan { uint32_t groups, rx_tiles, beam_tiles; uint64_t cells; size_t lds, out_doubles; bool supported; };
static inline RtsBeamPlan rts_beam_plan(uint32_t n_rx, uint32_t n_beams, uint32_t n_rows, uint32_t n_bins, uint32_t flags)
{
    RtsBeamPlan p;
    p.cells = (uint64_t)n_rows * n_bins;
    p.rx_tiles = (n_rx + RTS_BEAM_RX_TILE - 1u) / RTS_BEAM_RX_TILE;
    p.beam_tiles = (n_beams + RTS_BEAM_BEAM_TILE - 1u) / RTS_BEAM_BEAM_TILE;
    p.lds = 16u * (size_t)n_beams * n_rx;
    const uint64_t groups = (p.cells + RTS_BEAM_THREADS - 1u) / RTS_BEAM_THREADS;
    p.supported = n_rx >= 1u && n_rx <= RTS_BEAM_MAX_RX && n_beams >= 1u && n_beams <= RTS_BEAM_MAX_BEAMS &&
                  (uint64_t)n_beams * n_rx <= RTS_BEAM_MAX_WEIGHTS && groups >= 1u && groups <= RTS_BEAM_MAX_GRID_X;
    p.groups = p.supported ? (uint32_t)groups : 0u;
    p.out_doubles = (flags & RTS_BEAM_PEAK) ? 2u * (size_t)p.cells : (size_t)p.cells * n_beams * ((flags & RTS_BEAM_POWER) ? 1u : 2u);
    return p;
}

// the beamformer on the host (validated by the caller): in [n_rx][n_rows_in][n_bins] interleaved, w [n_beams][n_rx] interleaved, out in
// the layout of the flags.  Reads only rows first_row .. first_row + n_rows - 1 of every receiver.
static inline void rts_beam_eval_host(uint32_t n_rx, uint32_t n_bins, const double* in, uint32_t n_rows_in, uint32_t first_row, uint32_t n_rows,
                                      uint32_t n_beams, const double* w, uint32_t flags, double* out)
{
    const size_t cells = (size_t)n_rows * n_bins, rx_stride = (size_t)n_rows_in * n_bins, first = (size_t)first_row * n_bins;
    for (size_t c = 0; c < cells; c++) {
        RtsBeamPeak pk = {0.0, 0.0, 0.0, 0.0, 0u, 0u};
        for (uint32_t b = 0; b < n_beams; b++) {
            double yr = 0.0, yi = 0.0;
            for (uint32_t r = 0; r < n_rx; r++) {
                const double* z = in + 2 * ((size_t)r * rx_stride + first + c);
                rts_beam_add(r == 0u, w[2 * ((size_t)b * n_rx + r)], w[2 * ((size_t)b * n_rx + r) + 1], z[0], z[1], &yr, &yi);
            }
            if (flags & RTS_BEAM_PEAK) rts_beam_peak_push(&pk, b, rts_beam_power(yr, yi));
            else if (flags & RTS_BEAM_POWER) out[(size_t)b * cells + c] = rts_beam_power(yr, yi);
            else { out[2 * ((size_t)b * cells + c)] = yr; out[2 * ((size_t)b * cells + c) + 1] = yi; }
        }
        if (flags & RTS_BEAM_PEAK) rts_beam_peak_finish(&pk, n_beams, &out[2 * c], &out[2 * c + 1]);
    }
}
