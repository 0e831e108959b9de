// rts_waveform.h -- the transmit waveform's continuous envelope (include/rts_amd.h: RtsWaveform), evaluated on the host
// (rts_waveform_eval) and used by the render kernel (rts_render.hip: k_cube_render) through the SAME interpolation kernel h_L.
// Fixed trees of IEEE basic operations, compiled with -ffp-contract=off.
#pragma once
#include "rts_device_math.h"
#include "../../include/rts_amd.h"

// sin(pi x), exactly 0 at every integer x (the device's OCML sinpi; on the host a reduction to [-1/2, 1/2] by exact
// subtractions, then libm's sin)
RTS_HD double rts_sinpi(double x)
{
#ifdef __HIP_DEVICE_COMPILE__
    return sinpi(x);
#else
    double r = x - 2.0 * nearbyint(0.5 * x);                 // [-1, 1], exact
    if (r == nearbyint(r)) return 0.0;
    if (r > 0.5) r = 1.0 - r; else if (r < -0.5) r = -1.0 - r;      // sin(pi (1 - r)) = sin(pi r), exact subtractions
    return sin(RTS_PI * r);
#endif
}

// h_L(u): L = 1 sample-and-hold (1 on -1 < u <= 0), L even the Blackman-windowed sinc on |u| < L/2; h_L(0) = 1 exactly and, by
// sinpi, h_L(u) = 0 exactly at every other integer u
RTS_HD double rts_wave_h(double u, uint32_t L)
{
    if (L == 1u) return (u > -1.0 && u <= 0.0) ? 1.0 : 0.0;
    if (u == 0.0) return 1.0;
    const double half = 0.5 * (double)L;
    if (!(fabs(u) < half)) return 0.0;
    const double w = 0.42 + 0.5 * cos(2 * RTS_PI * u / (double)L) + 0.08 * cos(4 * RTS_PI * u / (double)L);
    return rts_sinpi(u) / (RTS_PI * u) * w;
}

// first tap of a contribution: its L weights are h_L(q - phi) for q = rts_wave_q0(L) .. rts_wave_q0(L) + L - 1, phi in [0, 1) the
// fractional part of its start; output sample n = floor(d) + k reads samples k - q
RTS_HD int rts_wave_q0(uint32_t L) { return L == 1u ? 0 : 1 - (int)(L / 2u); }

// s(x) = sum_m s[m] h_L(x - m) (s interleaved re / im, M samples); x outside the support, or not finite: 0
RTS_HD void rts_wave_eval(const double* s, uint32_t M, uint32_t L, double x, double* re, double* im)
{
    double ar = 0.0, ai = 0.0;
    const double half = 0.5 * (double)L;
    if (x > -half - 2.0 && x < (double)M + half + 2.0) {
        const int i = (int)floor(x), hl = (int)(L / 2u);
        const int lo = i - hl - 1 < 0 ? 0 : i - hl - 1, hi = i + hl + 1 > (int)M - 1 ? (int)M - 1 : i + hl + 1;
        for (int m = lo; m <= hi; m++) {
            const double h = rts_wave_h(x - (double)m, L);
            if (h != 0.0) { ar += s[2 * m] * h; ai += s[2 * m + 1] * h; }
        }
    }
    *re = ar; *im = ai;
}
