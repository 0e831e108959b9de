// rts_pattern.h -- tabulated antenna gain and RCS patterns (include/rts_amd.h: RtsPattern), evaluated on the host
// (rts_pattern_eval) and on the device (k_finalise_patterns, k_post_all) by the SAME functions.  Fixed trees of IEEE basic
// operations, compiled with -ffp-contract=off: a pattern's value is a function of its table and (u, v) only.
#pragma once
#include "rts_device_math.h"
#include "../../include/rts_amd.h"

#define RTS_TWO_PI 6.28318530717958647692

// One pattern as the evaluator reads it: the descriptor's numbers with pointers into wherever its tables live (the caller's
// arrays on the host; the handle's packed table buffer on the device).
struct RtsPatView {
    uint32_t kind, flags, n_u, n_v;
    double scale;
    const double* us; const double* uy;     // SEPARABLE: u samples / values
    const double* vs; const double* vy;     // SEPARABLE: v samples / values
    double u0, du, v0, dv;
    const double* grid;                     // GRID: [n_v][n_u]
};

// wrap(x) = x - 2 pi floor((x + pi) / 2 pi), in [-pi, pi)
RTS_HD double rts_wrap_pi(double x) { return x - RTS_TWO_PI * floor((x + RTS_PI) / RTS_TWO_PI); }

// piecewise-linear over strictly ascending s[0..n-1], clamped to the end values (a NaN abscissa reads the first value)
RTS_HD double rts_pat_lerp(const double* s, const double* y, uint32_t n, double x)
{
    if (n == 1u || !(x > s[0])) return y[0];
    if (x >= s[n - 1]) return y[n - 1];
    uint32_t lo = 0, hi = n - 1;                        // s[lo] <= x < s[hi]
    while (hi - lo > 1u) { const uint32_t mid = (lo + hi) >> 1; if (s[mid] <= x) lo = mid; else hi = mid; }
    const double t = (x - s[lo]) / (s[hi] - s[lo]);
    return y[lo] + t * (y[hi] - y[lo]);
}

// grid coordinate (x - x0) / dx clamped to [0, n - 1] (NaN: 0); cell i <= n - 2 and fraction t
RTS_HD void rts_pat_cell(double x, double x0, double dx, uint32_t n, uint32_t& i, double& t)
{
    double f = (x - x0) / dx;
    if (!(f >= 0.0)) f = 0.0;
    const double top = (double)(n - 1u);
    if (!(f <= top)) f = top;
    if (n < 2u) { i = 0; t = 0.0; return; }
    double fl = floor(f);
    if (fl > top - 1.0) fl = top - 1.0;
    i = (uint32_t)fl; t = f - fl;
}

RTS_HD double rts_pat_eval(const RtsPatView& p, double u, double v)
{
    if (p.kind == RTS_PATTERN_CONSTANT) return p.scale;
    if (p.kind == RTS_PATTERN_SEPARABLE) {
        const double uu = (p.flags & RTS_PATTERN_ABS_U) ? fabs(u) : u;
        const double vv = (p.flags & RTS_PATTERN_ABS_V) ? fabs(v) : v;
        return p.scale * rts_pat_lerp(p.us, p.uy, p.n_u, uu) * rts_pat_lerp(p.vs, p.vy, p.n_v, vv);
    }
    uint32_t i, j; double tu, tv;
    rts_pat_cell(u, p.u0, p.du, p.n_u, i, tu);
    rts_pat_cell(v, p.v0, p.dv, p.n_v, j, tv);
    const uint32_t i1 = p.n_u > 1u ? i + 1u : i, j1 = p.n_v > 1u ? j + 1u : j;
    const double* r0 = p.grid + (size_t)j * p.n_u; const double* r1 = p.grid + (size_t)j1 * p.n_u;
    const double a = r0[i] + tu * (r0[i1] - r0[i]);
    const double b = r1[i] + tu * (r1[i1] - r1[i]);
    return p.scale * (a + tv * (b - a));
}

// antenna angles of a pointing vector relative to a reference direction (ref_az, ref_el):
// u = wrap(atan2(y, x) - ref_az), v = asin(z / |vec|) - ref_el (asin term 0 for a zero vector)
RTS_HD void rts_pat_angles(dvec3 w, double ref_az, double ref_el, double& u, double& v)
{
    const double n = len3(w);
    const double az = atan2(w.y, w.x);
    double el = 0.0;
    if (n > 0.0) { double s = w.z / n; if (s > 1.0) s = 1.0; if (s < -1.0) s = -1.0; el = asin(s); }
    u = rts_wrap_pi(az - ref_az); v = el - ref_el;
}
