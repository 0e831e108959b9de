// rts_image.h -- backprojection imaging of the return cube (include/rts_amd.h: RtsImageParams): the arithmetic of one pixel, shared
// by the kernel (rts_image.hip: k_backproject) and the host evaluator (rts_backproject_eval), and the host-only plan of the launch.
// Fixed trees of IEEE basic operations plus sinpi / sincospi / cos / sin, compiled with -ffp-contract=off.  Includes nothing of
// HIP: it compiles with any host compiler and is tested without a GPU (tests/test_image_host.py, tests/image/image_main.cpp).
#pragma once
#include <math.h>
#include <stdint.h>
#include <stddef.h>
#include "../../include/rts_amd.h"

#ifndef RTS_HD
#define RTS_HD static inline          // (a host compiler; the library's units have rts_device_math.h's __host__ __device__ form)
#endif
#ifndef RTS_PI
#define RTS_PI 3.14159265358979323846
#endif

// sin(pi x) for x in [0, 1) (the device's OCML sinpi; on the host the reflection about 1/2, exact, then libm's sin)
RTS_HD double rts_image_sinpi01(double x)
{
#ifdef __HIP_DEVICE_COMPILE__
    return sinpi(x);
#else
    if (x > 0.5) x = 1.0 - x;
    return sin(RTS_PI * x);
#endif
}

// (sin, cos)(pi t) for t in [0, 2) (the device's OCML sincospi; on the host an exact reduction to [-1/2, 1/2], then libm)
RTS_HD void rts_image_sincospi(double t, double* sn, double* cs)
{
#ifdef __HIP_DEVICE_COMPILE__
    sincospi(t, sn, cs);
#else
    double sgn = 1.0;
    if (t >= 1.0) { t -= 1.0; sgn = -1.0; }            // sin(pi (t + 1)) = -sin(pi t), likewise cos; exact
    double s, c;
    if (t > 0.5) { const double r = 1.0 - t; s = sin(RTS_PI * r); c = -cos(RTS_PI * r); }
    else { s = sin(RTS_PI * t); c = cos(RTS_PI * t); }
    if (t == 0.5) c = 0.0;
    *sn = sgn * s; *cs = sgn * c;
#endif
}

// what the interpolation of one image keeps per thread: the window's rotation from tap to tap
struct RtsImageInterp { uint32_t L; int hl; double cd, sd; };
RTS_HD RtsImageInterp rts_image_interp_setup(uint32_t taps)
{
    RtsImageInterp ip; ip.L = taps; ip.hl = (int)(taps / 2u);
    ip.cd = taps > 1u ? cos(2 * RTS_PI / (double)taps) : 1.0;
    ip.sd = taps > 1u ? sin(2 * RTS_PI / (double)taps) : 0.0;
    return ip;
}

// v = the row (n_bins complex samples, interleaved re / im) interpolated at d (in samples); reads row[2 m], row[2 m + 1] for
// 0 <= m < n_bins only
RTS_HD void rts_image_sample(const double* row, uint32_t n_bins, const RtsImageInterp ip, double d, double* re, double* im)
{
    double ar = 0.0, ai = 0.0;
    const double half = (double)ip.hl;
    if (ip.L == 1u) {
        const double e = d + 0.5;
        if (e >= 0.0 && e < (double)n_bins) {                       // (a NaN fails both)
            const uint32_t n = (uint32_t)floor(e);
            if (n < n_bins) { ar = row[2 * (size_t)n]; ai = row[2 * (size_t)n + 1]; }
        }
    } else if (d > -half - 1.0 && d < (double)n_bins + half + 1.0) {
        const double fl = floor(d);
        const double phi = d - fl;                                  // [0, 1), exact
        const int64_t i = (int64_t)fl;
        if (phi == 0.0) {
            if (i >= 0 && i < (int64_t)n_bins) { ar = row[2 * (size_t)i]; ai = row[2 * (size_t)i + 1]; }
        } else {
            const int64_t m0 = i - ip.hl + 1;                       // tap k reads sample m0 + k
            const int k_lo = m0 < 0 ? (int)(-m0) : 0;
            const int64_t last = (int64_t)n_bins - 1 - m0;
            const int k_hi = last < (int64_t)ip.L - 1 ? (int)last : (int)ip.L - 1;
            if (k_lo <= k_hi) {
                const double sp = rts_image_sinpi01(phi);
                const double u0 = phi + (double)(ip.hl - 1 - k_lo);
                const double a0 = 2 * RTS_PI * u0 / (double)ip.L;
                double C = cos(a0), S = sin(a0);
                for (int k = k_lo; k <= k_hi; k++) {
                    const int q = ip.hl - 1 - k;
                    const double u = phi + (double)q;
                    const double w = 0.42 + 0.5 * C + 0.08 * (2.0 * C * C - 1.0);
                    const double sinc = ((q & 1) ? -sp : sp) / (RTS_PI * u);
                    const double h = sinc * w;
                    const size_t m = (size_t)(m0 + k);
                    ar += row[2 * m] * h; ai += row[2 * m + 1] * h;
                    const double Cn = C * ip.cd + S * ip.sd, Sn = S * ip.cd - C * ip.sd;
                    C = Cn; S = Sn;
                }
            }
        }
    }
    *re = ar; *im = ai;
}

// pixel (ix, iy) of the grid
RTS_HD void rts_image_pixel(const double* origin, const double* step_x, const double* step_y, uint32_t ix, uint32_t iy, double* x)
{
    for (int c = 0; c < 3; c++) x[c] = origin[c] + (double)ix * step_x[c] + (double)iy * step_y[c];
}

// two-way delay of pixel x for a transmitter at tx and a receiver at rx
RTS_HD double rts_image_tau(const double* x, const double* tx, const double* rx, double cspeed)
{
    const double ax = x[0] - tx[0], ay = x[1] - tx[1], az = x[2] - tx[2];
    const double bx = x[0] - rx[0], by = x[1] - rx[1], bz = x[2] - rx[2];
    const double dT = sqrt(ax * ax + ay * ay + az * az);
    const double dR = sqrt(bx * bx + by * by + bz * bz);
    return (dT + dR) / cspeed;
}

// one pulse's term of one pixel
RTS_HD void rts_image_term(const double* row, uint32_t n_bins, const RtsImageInterp ip, double t0, double dt, double carrier, double cspeed,
                           double w, const double* x, const double* tx, const double* rx, double* re, double* im)
{
    const double tau = rts_image_tau(x, tx, rx, cspeed);
    const double d = (tau - t0) / dt;
    double vr, vi; rts_image_sample(row, n_bins, ip, d, &vr, &vi);
    const double c = carrier * tau;
    const double f = c - floor(c);
    double sn = 0.0, cs = 1.0;
    if (f >= 0.0 && f < 1.0) rts_image_sincospi(2.0 * f, &sn, &cs);      // (an overflowed c has no fraction: phase 0, v is 0 there anyway)
    const double a = w * vr, b = w * vi;
    *re = a * cs - b * sn; *im = a * sn + b * cs;
}

// ---- the plan of a launch (host only): tile shape, chunk count, whether the chunks are split over the grid, scratch size.
//   One thread per pixel of a tile of 256 pixels, 16 x 16 unless the image is narrower or lower than 16 (then as wide / high as the
//   image's next power of two, and the other side takes the rest).  Chunks of RTS_IMAGE_PULSE_CHUNK pulses: with enough tiles to
//   fill the device (tiles * n_rx >= split_below), or with a single chunk, every thread walks all chunks itself and writes the
//   image; otherwise each chunk is a workgroup of its own that writes its sum to scratch[chunk][rx][iy][ix] and a second kernel adds
//   them.  The per-pixel order of additions is the same either way.
#define RTS_IMAGE_TILE 256u
#define RTS_IMAGE_SPLIT_BELOW 1024u      // default split_below: four workgroups per compute unit of an MI355X
#define RTS_IMAGE_GRID_MAX 65535u
struct RtsImagePlan { uint32_t tw_log2, th_log2, tiles_x, tiles_y, n_chunks; bool split, supported; size_t scratch; };
static inline uint32_t rts_image_log2_ceil(uint32_t n) { uint32_t b = 0; while (b < 31 && (1u << b) < n) b++; return b; }
static inline RtsImagePlan rts_image_plan(uint32_t n_x, uint32_t n_y, uint32_t n_rx, uint32_t n_pulses, uint32_t split_below)
{
    RtsImagePlan p;
    p.tw_log2 = 4; p.th_log2 = 4;
    if (n_x < 16u) { p.tw_log2 = rts_image_log2_ceil(n_x); p.th_log2 = 8u - p.tw_log2; }
    else if (n_y < 16u) { p.th_log2 = rts_image_log2_ceil(n_y); p.tw_log2 = 8u - p.th_log2; }
    p.tiles_x = (n_x + (1u << p.tw_log2) - 1u) >> p.tw_log2;
    p.tiles_y = (n_y + (1u << p.th_log2) - 1u) >> p.th_log2;
    p.n_chunks = (uint32_t)(((uint64_t)n_pulses + RTS_IMAGE_PULSE_CHUNK - 1u) / RTS_IMAGE_PULSE_CHUNK);
    const uint64_t blocks = (uint64_t)p.tiles_x * p.tiles_y * n_rx;
    p.split = p.n_chunks > 1u && blocks < split_below;
    p.supported = n_rx <= RTS_IMAGE_GRID_MAX && p.n_chunks <= RTS_IMAGE_GRID_MAX && (uint64_t)p.tiles_x * p.tiles_y <= 0x7fffffffull;
    p.scratch = p.split ? (size_t)p.n_chunks * n_rx * n_y * n_x : 0;
    return p;
}

// the whole image on the host: cube [n_rx][n_pulses_cube][n_bins], out [n_rx][n_y][n_x], both interleaved re / im (validated by the caller)
static inline void rts_image_eval_host(const RtsCubeParams* q, const double* cube, const RtsImageParams* p, double* out)
{
    const RtsImageInterp ip = rts_image_interp_setup(p->taps);
    const uint32_t P = p->n_pulses;
    for (uint32_t r = 0; r < q->n_rx; r++)
        for (uint32_t iy = 0; iy < p->n_y; iy++)
            for (uint32_t ix = 0; ix < p->n_x; ix++) {
                double x[3]; rts_image_pixel(p->origin, p->step_x, p->step_y, ix, iy, x);
                double tr = 0.0, ti = 0.0;
                for (uint32_t j0 = 0; j0 < P; j0 += RTS_IMAGE_PULSE_CHUNK) {
                    const uint32_t j1 = P - j0 < RTS_IMAGE_PULSE_CHUNK ? P : j0 + RTS_IMAGE_PULSE_CHUNK;
                    double sr = 0.0, si = 0.0;
                    for (uint32_t j = j0; j < j1; j++) {
                        const double* row = cube + 2 * (((size_t)r * q->n_pulses + p->first_pulse + j) * q->n_bins);
                        double er, ei;
                        rts_image_term(row, q->n_bins, ip, q->t0, q->dt, p->carrier, p->cspeed, p->pulse_weight ? p->pulse_weight[j] : 1.0, x,
                                       p->tx_position + 3 * (size_t)j, p->rx_position + 3 * ((size_t)r * P + j), &er, &ei);
                        sr += er; si += ei;
                    }
                    if (j0 == 0) { tr = sr; ti = si; } else { tr += sr; ti += si; }
                }
                double* o = out + 2 * (((size_t)r * p->n_y + iy) * p->n_x + ix);
                if (p->flags & RTS_IMAGE_ACCUMULATE) { o[0] += tr; o[1] += ti; } else { o[0] = tr; o[1] = ti; }
            }
}
