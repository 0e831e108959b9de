// rts_cube_source.h -- what a received record brings to the return cube, once for every writer of the cube (rts_render.hip: the
// impulse kernels and the waveform render; rts_beat.hip: the beat render; rts_post.hip: the fused end-of-pulse kernel): which record
// counts, its delay and phase, its complex amplitude, and -- device only -- the cell it lands in and the add.  Fixed trees of IEEE
// basic operations, compiled with -ffp-contract=off.  Includes nothing of HIP but what __HIPCC__ / __HIP_DEVICE_COMPILE__ guard: it
// compiles with any host compiler and is tested without a GPU (tests/test_cube_source_host.py, tests/cube_source/cube_source_main.cpp).
#pragma once
#include <math.h>
#include <stdint.h>
#include <stddef.h>
#include "../../include/rts_prd.h"

#ifndef RTS_HD
#define RTS_HD static inline          // (a host compiler; the library's units have rts_device_math.h's __host__ __device__ form)
#endif
#ifndef RTS_PI
#define RTS_PI 3.14159265358979323846
#endif

// The received set a cube writer reads.  paths == 0: every received ray, with the per-ray delay and phase of the reference
// (cspeed, carrier).  paths != 0: one contribution per response the reference would emit for the pulse (ray_tracer.cpp:1290-1321)
// -- the representative ray of every (receiver, path) group, pm[i] == base + i, with the GROUP's power ((sum sqrt p / n)^2, in the
// record), mean delay and mean phase (aggregation.cu:88-93: delay[], phase[]); needs the aggregation of the pulse.
struct RtsCubeSource {
    const PerRayData* rays; const double* delay; const double* phase; const int32_t* pm; int64_t base;
    uint32_t R; int paths;
    double cspeed, carrier;
};

// The read of record i, the question and the answer apart (as ONE function that returns both, the waveform render needs four more
// registers and loses a wave per SIMD: profiles/cube_source_refactor.txt).  `paths`: s.paths, or the caller's constant.
// Does the record count: for receiver rx (rts_cube_counts_for), or for one of a cube's n_rx receivers (rts_cube_counts: for which);
// per path only the representative of its group does.
RTS_HD bool rts_cube_representative(const RtsCubeSource& s, const bool paths, const uint32_t i) { return !paths || (int64_t)s.pm[i] == s.base + (int64_t)i; }
RTS_HD bool rts_cube_counts_for(const RtsCubeSource& s, const bool paths, const uint32_t i, const int32_t rx) { return s.rays[i].received == rx && rts_cube_representative(s, paths, i); }
RTS_HD bool rts_cube_counts(const RtsCubeSource& s, const bool paths, const uint32_t i, const uint32_t n_rx, int32_t* rx)
{
    *rx = s.rays[i].received;
    return *rx >= 0 && (uint32_t)*rx < n_rx && rts_cube_representative(s, paths, i);
}
// With which delay and phase: the group's, or the per-ray terms in the reference's operand order
RTS_HD void rts_cube_timing(const RtsCubeSource& s, const bool paths, const uint32_t i, double* delay_out, double* phase_out)
{
    if (paths) { *delay_out = s.delay[i]; *phase_out = s.phase[i]; }
    else {
        const double delay = (s.rays[i].rayLength)/s.cspeed;                     // aggregation.cu:59
        const double phase = -fmod(delay*2*RTS_PI*s.carrier, 2*RTS_PI);          // aggregation.cu:60
        *delay_out = delay; *phase_out = phase;
    }
}

// a = sqrt(P) e^{j phase}
RTS_HD void rts_cube_amplitude(const double power, const double phase, double* re, double* im)
{
    const double amp = sqrt(power);
    double sn, cs;
#ifdef __HIP_DEVICE_COMPILE__
    sincos(phase, &sn, &cs);
#else
    sn = sin(phase); cs = cos(phase);
#endif
    *re = amp * cs; *im = amp * sn;
}

#ifdef __HIPCC__
// cube[rx][pulse][n] of an interleaved complex128 cube, and the add of every writer: one f64 atomic (global_atomic_add_f64) per component
// (rx and n in the caller's own types, an integer or a double that holds one: converted here, in the order of the expression)
template <typename RX, typename N>
__device__ __forceinline__ double* rts_cube_cell(double* cube, const uint32_t n_pulses, const uint32_t n_bins, const RX rx, const uint32_t pulse, const N n)
{
    return cube + 2 * (((size_t)rx * n_pulses + pulse) * n_bins + (size_t)n);
}
__device__ __forceinline__ void rts_cube_add(double* cell, const double re, const double im) { atomicAdd(cell, re); atomicAdd(cell + 1, im); }

// the impulse cube's row (k_cube_accumulate<PATHS>, rts_render.hip; the fused end-of-pulse kernel, rts_post.hip): record i of the set
// into bin floor((delay - t0) / dt) of its receiver's row of pulse `pulse`
template <bool PATHS>
__device__ __forceinline__ void rts_cube_impulse_row(const RtsCubeSource& s, const uint32_t i, double* cube, const uint32_t n_rx, const uint32_t n_pulses, const uint32_t n_bins,
                                                     const uint32_t pulse, const double t0, const double dt)
{
    int32_t rx;
    if (!rts_cube_counts(s, PATHS, i, n_rx, &rx)) return;
    double delay, phase; rts_cube_timing(s, PATHS, i, &delay, &phase);
    const double b = floor((delay - t0) / dt);
    if (!(b >= 0.0) || !(b < (double)n_bins)) return;
    // (rts_cube_amplitude and rts_cube_add written out: each product right before its add, the order in which the fused kernel has
    // always issued them -- its instructions are held fixed, profiles/cube_source_refactor.txt)
    const double amp = sqrt(s.rays[i].power);
    double sn, cs; sincos(phase, &sn, &cs);
    double* cell = rts_cube_cell(cube, n_pulses, n_bins, rx, pulse, b);
    atomicAdd(cell, amp * cs); atomicAdd(cell + 1, amp * sn);
}
#endif
