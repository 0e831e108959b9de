// rts_cfar.h -- what every CFAR detector of include/rts_amd.h agrees on (rts_cube_detect, rts_cube_detect_os, rts_cfar_os_eval), each
// defined once: the window's geometry, the training count of a cell from its two range-edge distances, the 3 x 3 local-maximum rule,
// the log-parabola refinement and the RtsDetection record with its Doppler wrap.  The kernels (rts_detect.hip: k_cfar, k_cfar_os) and
// the host evaluator (rts_cfar_os.h) call these texts, so the edge rules and the record are one format, not three that happen to
// agree.  Includes nothing of HIP: it compiles with any host compiler and is tested without a GPU (tests/test_cfar_os_host.py,
// tests/cfar_os/cfar_os_main.cpp).
#pragma once
#include <math.h>
#include <stdint.h>
#include "../../include/rts_amd.h"

#ifndef RTS_HD
#define RTS_HD static inline          // (a host compiler; the library's units have rts_device_math.h's __host__ __device__ form)
#endif

// guard and training cells on each side of the cell under test, per axis; hr, hd: the halo a tile of the map is staged with (at least
// 1: the local-maximum rule and the refinement read the four neighbours whatever the window); rts_cfar_Or, _Od: the window's reach
struct RtsCfarWindow { int gr, gd, tr, td, hr, hd; };
RTS_HD int rts_cfar_Or(const RtsCfarWindow& w) { return w.gr + w.tr; }
RTS_HD int rts_cfar_Od(const RtsCfarWindow& w) { return w.gd + w.td; }
RTS_HD RtsCfarWindow rts_cfar_window(uint32_t gr, uint32_t gd, uint32_t tr, uint32_t td)
{
    RtsCfarWindow w;
    w.gr = (int)gr; w.gd = (int)gd; w.tr = (int)tr; w.td = (int)td;
    w.hr = rts_cfar_Or(w) > 1 ? rts_cfar_Or(w) : 1; w.hd = rts_cfar_Od(w) > 1 ? rts_cfar_Od(w) : 1;
    return w;
}

// training cells of a FULL window: the (2 (Gr + Tr) + 1) x (2 (Gd + Td) + 1) rectangle minus the guard rectangle
RTS_HD uint32_t rts_cfar_n0(uint32_t gr, uint32_t gd, uint32_t tr, uint32_t td)
{
    return (2u * (gr + tr) + 1u) * (2u * (gd + td) + 1u) - (2u * gr + 1u) * (2u * gd + 1u);
}

// training cells of a cell with edge_l bins to its left and edge_r to its right inside [0, n_bins) (Doppler wraps, range is truncated):
// outer columns (|dr| > Gr) hold 2 (Gd + Td) + 1 cells, inner columns and the cell's own hold the 2 Td rows outside the guard.
// *nl, *nr: the cells left (dr < 0) and right (dr > 0) of the cell's own column; returns the total, nl + nr + 2 Td.
RTS_HD int rts_cfar_count(const RtsCfarWindow& w, int edge_l, int edge_r, int* nl, int* nr)
{
    const int Or = rts_cfar_Or(w), Od = rts_cfar_Od(w);
    const int cl = edge_l < Or ? edge_l : Or, cr = edge_r < Or ? edge_r : Or;      // columns that exist on each side
    const int nlo = cl > w.gr ? cl - w.gr : 0, nli = cl < w.gr ? cl : w.gr;
    const int nro = cr > w.gr ? cr - w.gr : 0, nri = cr < w.gr ? cr : w.gr;
    *nl = nlo * (2 * Od + 1) + nli * 2 * w.td; *nr = nro * (2 * Od + 1) + nri * 2 * w.td;
    return *nl + *nr + 2 * w.td;
}
RTS_HD int rts_cfar_count(const RtsCfarWindow& w, int edge_l, int edge_r) { int nl, nr; return rts_cfar_count(w, edge_l, edge_r, &nl, &nr); }

// RTS_CFAR_LOCAL_MAX: P against its 3 x 3 neighbours at(dk, dr) -- strictly greater than those before it in flat (k, r) order (dk < 0,
// or dk = 0 and dr < 0), at least equal to those after, so a plateau of equal cells reports its first cell.  left, right: the range
// neighbour exists (range is truncated; the caller wraps Doppler in `at`, which is only asked for neighbours that exist).
template <class At> RTS_HD bool rts_cfar_local_max(double P, bool left, bool right, At at)
{
    bool peak = true;
    for (int dk = -1; dk <= 1; dk++)
        for (int dr = -1; dr <= 1; dr++) {
            if ((dk == 0 && dr == 0) || (dr < 0 && !left) || (dr > 0 && !right)) continue;
            const double q = at(dk, dr);
            if (dk < 0 || (dk == 0 && dr < 0)) peak = peak && P > q; else peak = peak && P >= q;
        }
    return peak;
}

// parabola through ln P of three samples: the vertex offset in [-0.5, 0.5], 0 when it is not a peak of positive powers
// (den < 0 leaves lm and lp finite -- a +inf among them makes den +inf or NaN -- so d is never NaN and a compare-and-select clamp would
// give the same values; fmin / fmax are v_min / v_max on the device, two VGPRs and one wave per SIMD of k_cfar<WRITE> cheaper)
RTS_HD double rts_cfar_delta(double pm, double p0, double pp)
{
    if (!(pm > 0.0) || !(p0 > 0.0) || !(pp > 0.0)) return 0.0;
    const double lm = log(pm), l0 = log(p0), lp = log(pp);
    const double den = lm - 2.0 * l0 + lp;
    if (!(den < 0.0)) return 0.0;
    const double d = 0.5 * (lm - lp) / den;
    return fmin(0.5, fmax(-0.5, d));
}

// The record of cell (rx, k, r) of a map of nd Doppler rows: n training cells, power P, the detector's noise estimate and threshold;
// p_rm, p_rp: the powers at r - 1, r + 1 (0 where the map ends), p_km, p_kp: at k - 1, k + 1 (wrapped).  Doppler bin k + offset is
// wrapped into [-nd / 2, nd / 2) before it becomes Hz.
RTS_HD RtsDetection rts_cfar_record(uint32_t rx, uint32_t k, uint32_t r, uint32_t n, double P, double noise, double thr,
                                    double p_rm, double p_rp, double p_km, double p_kp, uint32_t nd, double t0, double dt, double pri)
{
    const double dr_ = rts_cfar_delta(p_rm, P, p_rp);
    const double dd_ = rts_cfar_delta(p_km, P, p_kp);
    double w = (double)k + dd_;
    const double half = 0.5 * (double)nd;
    if (w >= half) w -= (double)nd; else if (w < -half) w += (double)nd;
    RtsDetection d;
    d.rx = rx; d.doppler_bin = k; d.range_bin = r; d.n_train = n;
    d.power = P; d.noise = noise; d.threshold = thr; d.range_offset = dr_; d.doppler_offset = dd_;
    d.delay = t0 + ((double)r + dr_) * dt;
    d.doppler = pri > 0.0 ? w / ((double)nd * pri) : 0.0;
    return d;
}
