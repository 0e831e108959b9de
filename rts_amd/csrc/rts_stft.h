// rts_stft.h -- the slow-time transforms of the return cube: the radix-2 tree every transform of the library runs -- bit-reversed
// load, log2 N decimation-in-time stages, twiddles from one sincospi(-2 k / N) each -- shared by the kernels (rts_stft.hip:
// k_cube_doppler, k_cube_stft; rts_beat.hip: k_cube_range) and the host evaluators (rts_stft_eval, rts_range_eval); the host-only
// plans of the Doppler map's and the spectrogram's launches (include/rts_amd.h: rts_cube_doppler, RtsStftParams) and the windows.
// Fixed trees of IEEE basic operations, compiled with -ffp-contract=off.  Includes nothing of HIP: it compiles with any host
// compiler and is tested without a GPU (tests/test_stft_host.py, tests/stft/stft_main.cpp; tests/test_cube_source_host.py).
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

// tw_table[k] = (cos, sin)(pi (-2 k / N)), k < N / 2 (the device's OCML sincospi on the kernel's own argument; on the host the exact
// reflections sin(-pi u) = -sin(pi u), cos(-pi u) = cos(pi u), u = 2 k / N in [0, 1), about 1/2, then libm)
RTS_HD void rts_stft_twiddle(uint32_t k, uint32_t N, double* cs, double* sn)
{
#ifdef __HIP_DEVICE_COMPILE__
    sincospi(-2.0 * (double)k / (double)N, sn, cs);
#else
    const double u = 2.0 * (double)k / (double)N;
    double s, c;
    if (u > 0.5) { const double r = 1.0 - u; s = sin(RTS_PI * r); c = -cos(RTS_PI * r); }
    else { s = sin(RTS_PI * u); c = cos(RTS_PI * u); }
    if (u == 0.5) c = 0.0;
    *sn = -s; *cs = c;
#endif
}

// where sample p of a frame is stored: its index with the low logN bits reversed (1 <= logN <= 32)
RTS_HD uint32_t rts_stft_bitrev(uint32_t p, uint32_t logN)
{
    p = ((p >> 1) & 0x55555555u) | ((p & 0x55555555u) << 1);
    p = ((p >> 2) & 0x33333333u) | ((p & 0x33333333u) << 2);
    p = ((p >> 4) & 0x0f0f0f0fu) | ((p & 0x0f0f0f0fu) << 4);
    p = ((p >> 8) & 0x00ff00ffu) | ((p & 0x00ff00ffu) << 8);
    p = (p >> 16) | (p << 16);
    return p >> (32u - logN);
}

// butterfly j (< N / 2) of stage s (1 .. logN): the rows i0, i1 = i0 + 2^(s-1) it joins and the index of its twiddle in the table
RTS_HD void rts_stft_pair(uint32_t j, uint32_t s, uint32_t N, uint32_t* i0, uint32_t* i1, uint32_t* tw_index)
{
    const uint32_t half = 1u << (s - 1u), k = j & (half - 1u);
    *i0 = ((j >> (s - 1u)) << s) + k; *i1 = *i0 + half; *tw_index = k * (N >> s);
}

// (u, v) -> (u + t, u - t), t = tw v
RTS_HD void rts_stft_butterfly(double wr, double wi, double* ur, double* ui, double* vr, double* vi)
{
    const double xr = *vr, xi = *vi, tr = wr * xr - wi * xi, ti = wr * xi + wi * xr, ar = *ur, ai = *ui;
    *ur = ar + tr; *ui = ai + ti; *vr = ar - tr; *vi = ai - ti;
}

// a windowed sample
RTS_HD void rts_stft_taper(double w, double* re, double* im) { *re = w * *re; *im = w * *im; }

RTS_HD double rts_stft_power(double re, double im) { return re * re + im * im; }

// ---- the plans of the launches (host only).  log2 of a transform's size: the least logN <= 31 with 2^logN >= n_fft
static inline uint32_t rts_stft_log2(uint32_t n_fft) { uint32_t logN = 0; while (logN < 31u && (1u << logN) < n_fft) logN++; return logN; }
static inline size_t rts_stft_lds_bytes(uint32_t n_fft, uint32_t BT) { return (size_t)n_fft * BT * 16u + (size_t)n_fft * 8u; }

// The Doppler map (rts_cube_doppler: every pulse of the cube, no frames, gate or taper).  One workgroup per (receiver, tile of BT
// consecutive range bins); BT: the most columns, a power of two up to RTS_DOPPLER_BIN_TILE, whose N x BT complex128 fit 64 KiB.
#define RTS_DOPPLER_BIN_TILE 8u
#define RTS_DOPPLER_TILE_BYTES 65536u
struct RtsDopplerPlan { uint32_t logN, BT; size_t lds; };
static inline RtsDopplerPlan rts_doppler_plan(uint32_t n_fft)
{
    RtsDopplerPlan p;
    p.logN = rts_stft_log2(n_fft);
    p.BT = RTS_DOPPLER_BIN_TILE; while (p.BT > 1u && (size_t)n_fft * p.BT * 16u > RTS_DOPPLER_TILE_BYTES) p.BT >>= 1;
    p.lds = rts_stft_lds_bytes(n_fft, p.BT);
    return p;
}

// The spectrogram.  One workgroup per (receiver, frame, tile of gate bins); its LDS holds the tile's N x BT
// complex128 columns and the N / 2 complex twiddles.  BT: the most columns, a power of two up to RTS_STFT_BIN_TILE, that fit the
// 160 KiB a workgroup may allocate.  A workgroup takes BT gate bins; with RTS_STFT_SUM_BINS it takes a whole summation tile of
// RTS_STFT_BIN_TILE bins in RTS_STFT_BIN_TILE / BT passes.  The grid is (n_frames * tiles, n_rx).
#define RTS_STFT_LDS_MAX 163840u
#define RTS_STFT_THREADS 256u
struct RtsStftPlan { uint32_t logN, BT, passes, tiles, n_frames, n_gate; size_t lds, out_doubles, partial_doubles; bool supported; };
static inline RtsStftPlan rts_stft_plan(uint32_t n_rx, uint32_t n_pulses, uint32_t window_len, uint32_t hop, uint32_t n_fft, uint32_t n_gate, uint32_t flags)
{
    RtsStftPlan p;
    p.logN = rts_stft_log2(n_fft);
    p.BT = RTS_STFT_BIN_TILE; while (p.BT > 1u && rts_stft_lds_bytes(n_fft, p.BT) > RTS_STFT_LDS_MAX) p.BT >>= 1;
    p.lds = rts_stft_lds_bytes(n_fft, p.BT);
    const bool sum = (flags & RTS_STFT_SUM_BINS) != 0;
    p.passes = sum ? RTS_STFT_BIN_TILE / p.BT : 1u;
    const uint32_t per_group = sum ? RTS_STFT_BIN_TILE : p.BT;
    p.tiles = (uint32_t)(((uint64_t)n_gate + per_group - 1u) / per_group);
    p.n_frames = 1u + (n_pulses - window_len) / hop;
    p.n_gate = n_gate;
    p.supported = p.lds <= RTS_STFT_LDS_MAX && n_rx <= RTS_STFT_MAX_RX && (uint64_t)p.n_frames * p.tiles <= RTS_STFT_MAX_GRID_X;
    const size_t rows = (size_t)n_rx * p.n_frames * n_fft;
    p.out_doubles = sum ? rows : rows * n_gate * ((flags & RTS_STFT_POWER) ? 1u : 2u);
    p.partial_doubles = sum && p.tiles > 1u ? rows * p.tiles : 0;
    return p;
}

// the table of a transform: tw[2 k], tw[2 k + 1] = (cos, sin), k < N / 2
static inline void rts_stft_twiddles_host(uint32_t N, double* tw) { for (uint32_t k = 0; k < N / 2u; k++) rts_stft_twiddle(k, N, &tw[2 * k], &tw[2 * k + 1]); }

// one column on the host: x[N] complex (interleaved) <- the transform of the window_len samples at col, col + 2 row_stride, ...
// (reads exactly those samples), tapered by w unless it is NULL
static inline void rts_stft_column_host(const double* col, size_t row_stride, uint32_t window_len, const double* w, uint32_t N, uint32_t logN, const double* tw, double* x)
{
    for (uint32_t i = 0; i < N; i++) {
        double re = 0.0, im = 0.0;
        if (i < window_len) { re = col[2 * row_stride * i]; im = col[2 * row_stride * i + 1]; if (w) rts_stft_taper(w[i], &re, &im); }
        const uint32_t r = rts_stft_bitrev(i, logN);
        x[2 * r] = re; x[2 * r + 1] = im;
    }
    for (uint32_t s = 1; s <= logN; s++)
        for (uint32_t j = 0; j < N / 2u; j++) {
            uint32_t i0, i1, k; rts_stft_pair(j, s, N, &i0, &i1, &k);
            rts_stft_butterfly(tw[2 * k], tw[2 * k + 1], &x[2 * i0], &x[2 * i0 + 1], &x[2 * i1], &x[2 * i1 + 1]);
        }
}

// the whole spectrogram on the host (validated by the caller; plan from rts_stft_plan): cube [n_rx][q->n_pulses][q->n_bins] interleaved,
// out in the layout of the flags, work: 4 n_fft doubles (the column, the twiddles, a tile's sums)
static inline void rts_stft_eval_host(const RtsCubeParams* q, const double* cube, const RtsStftParams* p, const RtsStftPlan& plan, double* out, double* work)
{
    const uint32_t N = p->n_fft, G = plan.n_gate;
    double* x = work; double* tw = work + 2 * (size_t)N; double* ts = work + 3 * (size_t)N;
    rts_stft_twiddles_host(N, tw);
    const bool power = (p->flags & RTS_STFT_POWER) != 0, sum = (p->flags & RTS_STFT_SUM_BINS) != 0;
    for (uint32_t r = 0; r < q->n_rx; r++)
        for (uint32_t f = 0; f < plan.n_frames; f++) {
            const size_t row0 = (size_t)r * q->n_pulses + p->first_pulse + (size_t)f * p->hop;
            const size_t rf = (size_t)r * plan.n_frames + f;
            for (uint32_t g = 0; g < G; g++) {
                rts_stft_column_host(cube + 2 * (row0 * q->n_bins + p->first_bin + g), q->n_bins, p->window_len, p->window, N, plan.logN, tw, x);
                if (sum) {
                    const bool first_of_tile = g % RTS_STFT_BIN_TILE == 0, last_of_tile = g % RTS_STFT_BIN_TILE == RTS_STFT_BIN_TILE - 1u || g == G - 1u;
                    for (uint32_t k = 0; k < N; k++) { const double v = rts_stft_power(x[2 * k], x[2 * k + 1]); if (first_of_tile) ts[k] = v; else ts[k] += v; }
                    if (last_of_tile) for (uint32_t k = 0; k < N; k++) { double* o = out + rf * N + k; if (g < RTS_STFT_BIN_TILE) *o = ts[k]; else *o += ts[k]; }
                } else if (power) {
                    for (uint32_t k = 0; k < N; k++) out[(rf * N + k) * G + g] = rts_stft_power(x[2 * k], x[2 * k + 1]);
                } else {
                    for (uint32_t k = 0; k < N; k++) { double* o = out + 2 * ((rf * N + k) * G + g); o[0] = x[2 * k]; o[1] = x[2 * k + 1]; }
                }
            }
        }
}

// the symmetric windows of rts_window_make (kind < 4, n >= 1): the first half from the formula, the second its mirror
static inline void rts_stft_window_host(uint32_t kind, uint32_t n, double* out)
{
    static const double A[4][3] = {{1.0, 0.0, 0.0}, {0.5, 0.5, 0.0}, {0.54, 0.46, 0.0}, {0.42, 0.5, 0.08}};
    if (n == 1u) { out[0] = 1.0; return; }
    for (uint32_t i = 0; i < (n + 1u) / 2u; i++) {
        const double a = (double)i / (double)(n - 1u);
        const double v = kind == 0u ? 1.0 : A[kind][0] - A[kind][1] * cos(2 * RTS_PI * a) + A[kind][2] * cos(4 * RTS_PI * a);
        out[i] = v; out[n - 1u - i] = v;
    }
}
