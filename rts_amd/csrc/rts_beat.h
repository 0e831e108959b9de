// rts_beat.h -- FMCW / stretch processing (include/rts_amd.h: RtsBeatParams, RtsRangeParams): the dechirped beat render's tree, shared
// by the kernel (rts_beat.hip: k_cube_beat) and the host evaluator (rts_beat_eval), the fast-time range transform's host evaluator
// (on the one transform tree, rts_stft.h) and the host-only plans of the three launches.  Fixed trees of IEEE basic
// operations plus sincospi, compiled with -ffp-contract=off.  Includes nothing of HIP: it compiles with any host compiler and is
// tested without a GPU (tests/test_beat_host.py, tests/beat/beat_main.cpp).
#pragma once
#include <math.h>
#include <stdint.h>
#include <stddef.h>
#include "../../include/rts_amd.h"
#include "rts_stft.h"

// (sin, cos)(2 pi psi) of a phase in turns: psi reduced by psi - floor(psi) to [0, 1], then one sincospi(2 .) (the device's OCML
// sincospi; on the host the exact reflections about 1 and 1/2, then libm)
RTS_HD void rts_beat_sincos_turns(double psi, double* sn, double* cs)
{
    const double u = 2.0 * (psi - floor(psi));
#ifdef __HIP_DEVICE_COMPILE__
    sincospi(u, sn, cs);
#else
    double t = u, sgn = 1.0;
    if (t >= 2.0) t -= 2.0;                              // (psi a hair below an integer: the difference rounds to 1)
    if (t >= 1.0) { t -= 1.0; sgn = -1.0; }              // sin(pi (t + 1)) = -sin(pi t), likewise cos; exact
    double s, c;
    if (t > 0.5) { const double r = 1.0 - t; s = sin(RTS_PI * r); c = -cos(RTS_PI * r); }
    else { s = sin(RTS_PI * t); c = cos(RTS_PI * t); }
    if (t == 0.5) c = 0.0;
    *sn = sgn * s; *cs = sgn * c;
#endif
}

RTS_HD bool rts_beat_finite(double x) { return x - x == 0.0; }

// what a contribution brings to every strip: amplitude, delay, beat frequency fb = f - S tau, the constant phase
// ph0 = S tau^2 / 2 - f tau (turns) and the rotation of one sample step, (sd, cd) = sincos of delta = fb dt -- once per contribution
struct RtsBeatItem { double are, aim, tau, fb, ph0, cd, sd, pad; };
RTS_HD RtsBeatItem rts_beat_item(double are, double aim, double tau, double f, double S, double dt)
{
    RtsBeatItem it;
    const double st = S * tau;
    it.are = are; it.aim = aim; it.tau = tau;
    it.fb = f - st;
    it.ph0 = (st * tau) * 0.5 - f * tau;
    rts_beat_sincos_turns(it.fb * dt, &it.sd, &it.cd);
    it.pad = 0.0;
    return it;
}

// the time of sample n, and the gate a sample passes: the echo has arrived and the local oscillator runs
RTS_HD double rts_beat_time(double t0, double dt, uint32_t n) { return t0 + (double)n * dt; }
RTS_HD bool rts_beat_gate(double tau, double t, double T) { return tau <= t && t >= 0.0 && t < T; }

// one contribution on one strip: t[i] the times of the strip's RTS_BEAT_STRIP samples (NaN beyond the row: no gate passes), t_last
// that of its last sample inside the row, acc[2 i], acc[2 i + 1] the strip's running sums.  A contribution that arrives after the
// strip adds nothing to it and is skipped whole.
RTS_HD void rts_beat_strip(const RtsBeatItem& it, const double* t, double t_last, double T, double* acc)
{
    if (!(it.tau <= t_last)) return;
    double s, c;
    rts_beat_sincos_turns(it.fb * t[0] + it.ph0, &s, &c);
#ifdef __HIP_DEVICE_COMPILE__
#pragma unroll
#endif
    for (uint32_t i = 0; i < RTS_BEAT_STRIP; i++) {
        const double tr = it.are * c - it.aim * s, ti = it.are * s + it.aim * c;
        if (rts_beat_gate(it.tau, t[i], T)) { acc[2 * i] += tr; acc[2 * i + 1] += ti; }
        const double cn = c * it.cd - s * it.sd, sn = s * it.cd + c * it.sd;
        c = cn; s = sn;
    }
}

// the times of the strip that starts at sample n0 (< n_bins); returns the time of its last sample inside the row
RTS_HD double rts_beat_strip_times(double t0, double dt, uint32_t n0, uint32_t n_bins, double* t)
{
    double t_last = 0.0;
#ifdef __HIP_DEVICE_COMPILE__
#pragma unroll
#endif
    for (uint32_t i = 0; i < RTS_BEAT_STRIP; i++) {
        if (n0 + i < n_bins) { t[i] = rts_beat_time(t0, dt, n0 + i); t_last = t[i]; }
        else t[i] = NAN;
    }
    return t_last;
}

// ---- the plan of a render (host only), from the size of the received set and the cube's shape alone.  One workgroup of one wave
// per (receiver, tile of RTS_BEAT_TILE samples, part); a thread owns one strip.  A set of up to RTS_BEAT_ONE_BELOW records (a group
// table) is ONE launch that adds to the cube itself.  A larger one is cut into P parts of consecutive records -- as many as bring
// the grid to RTS_BEAT_FILL workgroups (four one-wave workgroups on each of an MI355X's 256 compute units), no part shorter than
// RTS_BEAT_PART_MIN records, at most RTS_BEAT_MAX_PARTS -- whose sums go to scratch[part][rx][n] (complex128) and are added in
// ascending order by a second kernel.  force_parts != 0 (RTS_BEAT_PARTS, the tests): that many parts, as far as the set has records.
#define RTS_BEAT_THREADS 64u
#define RTS_BEAT_TILE (RTS_BEAT_THREADS * RTS_BEAT_STRIP)
#define RTS_BEAT_FILL 1024u
#define RTS_BEAT_PART_MIN 8u
#define RTS_BEAT_ONE_BELOW 64u
#define RTS_BEAT_MAX_RX 65535u
struct RtsBeatPlan { uint32_t tiles, P, part_len; size_t scratch_doubles; bool supported; };
static inline RtsBeatPlan rts_beat_plan(uint64_t R, uint32_t n_rx, uint32_t n_bins, uint32_t force_parts)
{
    RtsBeatPlan p;
    p.tiles = (uint32_t)(((uint64_t)n_bins + RTS_BEAT_TILE - 1u) / RTS_BEAT_TILE);
    uint64_t P = 1;
    if (force_parts) P = force_parts;
    else if (R > RTS_BEAT_ONE_BELOW) {
        const uint64_t groups = (uint64_t)p.tiles * n_rx;
        P = groups ? (RTS_BEAT_FILL + groups - 1u) / groups : 1u;
        if (P > R / RTS_BEAT_PART_MIN) P = R / RTS_BEAT_PART_MIN;
    }
    if (P > RTS_BEAT_MAX_PARTS) P = RTS_BEAT_MAX_PARTS;
    if (P > R) P = R;
    if (P < 1u) P = 1u;
    const uint64_t len = R ? (R + P - 1u) / P : 1u;
    p.part_len = (uint32_t)(len > 0xffffffffull ? 0xffffffffull : len);
    p.P = R ? (uint32_t)((R + len - 1u) / len) : 1u;          // (no empty part)
    p.scratch_doubles = p.P > 1u ? 2u * (size_t)p.P * n_rx * n_bins : 0u;
    p.supported = n_rx <= RTS_BEAT_MAX_RX && R <= 0xffffffffull;
    return p;
}

// the render on the host (validated by the caller): the contributions in order into a row of sums per receiver that starts at
// zero, then each sum that is not zero added to the cube once -- the kernel's order with P = 1.  work: 2 n_rx n_bins doubles.
static inline void rts_beat_eval_host(const RtsCubeParams* q, const RtsBeatParams* p, const RtsBeatContribution* c, uint32_t n, uint32_t pulse_index,
                                      double* cube, double* work)
{
    const uint32_t nb = q->n_bins;
    const bool dop = (p->flags & RTS_RENDER_DOPPLER) != 0;
    for (size_t i = 0; i < 2 * (size_t)q->n_rx * nb; i++) work[i] = 0.0;
    for (uint32_t k = 0; k < n; k++) {
        if (c[k].rx < 0 || (uint32_t)c[k].rx >= q->n_rx || !rts_beat_finite(c[k].delay)) continue;
        const RtsBeatItem it = rts_beat_item(c[k].re, c[k].im, c[k].delay, dop ? c[k].doppler : 0.0, p->slope, q->dt);
        double* row = work + 2 * (size_t)c[k].rx * nb;
        for (uint32_t n0 = 0; n0 < nb; n0 += RTS_BEAT_STRIP) {
            double t[RTS_BEAT_STRIP], acc[2 * RTS_BEAT_STRIP];
            const double t_last = rts_beat_strip_times(q->t0, q->dt, n0, nb, t);
            const uint32_t live = nb - n0 < RTS_BEAT_STRIP ? nb - n0 : RTS_BEAT_STRIP;
            for (uint32_t i = 0; i < 2 * RTS_BEAT_STRIP; i++) acc[i] = i < 2 * live ? row[2 * (size_t)n0 + i] : 0.0;
            rts_beat_strip(it, t, t_last, p->duration, acc);
            for (uint32_t i = 0; i < 2 * live; i++) row[2 * (size_t)n0 + i] = acc[i];
        }
    }
    for (uint32_t r = 0; r < q->n_rx; r++) {
        double* dst = cube + 2 * (((size_t)r * q->n_pulses + pulse_index) * nb);
        const double* src = work + 2 * (size_t)r * nb;
        for (uint32_t i = 0; i < nb; i++) if (src[2 * i] != 0.0 || src[2 * i + 1] != 0.0) { dst[2 * i] += src[2 * i]; dst[2 * i + 1] += src[2 * i + 1]; }
    }
}

// ---- the fast-time range transform.  The plan of a launch (host only): one workgroup of RTS_RANGE_THREADS threads holds RT whole
// rows of n_fft complex128 and the n_fft / 2 complex twiddles in LDS -- 96 KiB at n_fft 4096 with RT = 1, of the 160 KiB a workgroup
// may allocate.  RT: the most rows, a power of two up to RTS_RANGE_ROW_TILE, with RT n_fft <= RTS_RANGE_TILE_ELEMS (64 KiB of rows: two
// workgroups per compute unit, 16 elements per thread and pass).  The rows (receiver, pulse) are numbered rx n_pulses + j and dealt
// RT at a time: the grid is ceil(n_rx n_pulses / RT) workgroups.
#define RTS_RANGE_THREADS 256u
#define RTS_RANGE_ROW_TILE 16u
#define RTS_RANGE_TILE_ELEMS 4096u
#define RTS_RANGE_MAX_GRID_X 2147483647u
struct RtsRangePlan { uint32_t logN, RT, n_samples, n_out, groups; uint64_t rows; size_t lds, out_doubles; bool supported; };
static inline size_t rts_range_lds_bytes(uint32_t n_fft, uint32_t RT) { return (size_t)n_fft * RT * 16u + (size_t)n_fft * 8u; }
static inline RtsRangePlan rts_range_plan(uint32_t n_rx, uint32_t n_pulses, uint32_t n_samples, uint32_t n_fft, uint32_t n_out)
{
    RtsRangePlan p;
    p.logN = rts_stft_log2(n_fft);
    p.RT = RTS_RANGE_ROW_TILE; while (p.RT > 1u && (uint64_t)p.RT * n_fft > RTS_RANGE_TILE_ELEMS) p.RT >>= 1;
    p.lds = rts_range_lds_bytes(n_fft, p.RT);
    p.n_samples = n_samples; p.n_out = n_out ? n_out : n_fft;
    p.rows = (uint64_t)n_rx * n_pulses;
    const uint64_t groups = (p.rows + p.RT - 1u) / p.RT;
    p.supported = p.lds <= RTS_STFT_LDS_MAX && groups <= RTS_RANGE_MAX_GRID_X;
    p.groups = p.supported ? (uint32_t)groups : 0u;
    p.out_doubles = 2u * (size_t)p.rows * p.n_out;
    return p;
}

// the transform on the host (validated by the caller; plan from rts_range_plan): cube [n_rx][q->n_pulses][q->n_bins] interleaved, out
// complex [n_rx][p->n_pulses][n_out] interleaved, work: 3 n_fft doubles (the row, the twiddles).  Reads only the gate's samples of the
// span's rows and the window's n_samples values.
static inline void rts_range_eval_host(const RtsCubeParams* q, const double* cube, const RtsRangeParams* p, const RtsRangePlan& plan, double* out, double* work)
{
    const uint32_t N = p->n_fft;
    double* x = work; double* tw = work + 2 * (size_t)N;
    rts_stft_twiddles_host(N, tw);
    const bool rev = (p->flags & RTS_RANGE_REVERSE) != 0;
    for (uint32_t r = 0; r < q->n_rx; r++)
        for (uint32_t j = 0; j < p->n_pulses; j++) {
            const double* row = cube + 2 * (((size_t)r * q->n_pulses + p->first_pulse + j) * q->n_bins + p->first_bin);
            rts_stft_column_host(row, 1u, plan.n_samples, p->window, N, plan.logN, tw, x);
            double* o = out + 2 * (((size_t)r * p->n_pulses + j) * plan.n_out);
            for (uint32_t k = 0; k < plan.n_out; k++) {
                const uint32_t src = rev ? (N - k) & (N - 1u) : k;
                o[2 * k] = x[2 * src]; o[2 * k + 1] = x[2 * src + 1];
            }
        }
}
