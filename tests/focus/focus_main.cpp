// Driver of tests/test_focus_host.py: rts_amd/csrc/rts_focus.h alone (with rts_stft.h and rts_image.h, which it builds on), built
// with a plain host compiler (under AddressSanitizer + UndefinedBehaviorSanitizer where it has them).  One case per line on stdin,
// the results on stdout; the expectations live in the test.  The evaluators run on a heap cube of which ONLY the samples their
// definitions read are addressable -- the rows of the range (whole rows for the alignment and the correction, the gate's bins
// for the PGA) -- and everything else is poisoned, so a read or a write outside is a sanitizer report; outputs and work arrays
// are heap arrays of exactly their sizes.
#include "rts_focus.h"
#include <cstdio>
#include <cstring>
#include <vector>
#if defined(__SANITIZE_ADDRESS__) && defined(__has_include)
#if __has_include(<sanitizer/asan_interface.h>)
#include <sanitizer/asan_interface.h>
#define FOCUS_POISON(p, n) ASAN_POISON_MEMORY_REGION(p, n)
#define FOCUS_UNPOISON(p, n) ASAN_UNPOISON_MEMORY_REGION(p, n)
#endif
#endif
#ifndef FOCUS_POISON
#define FOCUS_POISON(p, n) ((void)(p), (void)(n))
#define FOCUS_UNPOISON(p, n) ((void)(p), (void)(n))
#endif

// the cube of the cases: y[r][p][b], a strong scatterer that walks one bin every 8 pulses on a pseudo-random floor
static double cube_re(uint32_t r, uint32_t p, uint32_t b, uint32_t nb)
{
    const uint32_t at = (nb / 2u + p / 8u) % nb;
    return (double)((r * 131u + p * 17u + b * 7u) % 23u) - 11.0 + 0.25 * (double)p + (b == at ? 200.0 : 0.0);
}
static double cube_im(uint32_t r, uint32_t p, uint32_t b) { return (double)((r * 5u + p * 3u + b * 11u) % 19u) - 9.0 - 0.5 * (double)b; }
static double* make_cube(const RtsCubeParams& q, int zero_row)
{
    const size_t cells = (size_t)q.n_rx * q.n_pulses * q.n_bins;
    double* cube = new double[2 * cells];
    for (uint32_t r = 0; r < q.n_rx; r++) for (uint32_t j = 0; j < q.n_pulses; j++) for (uint32_t b = 0; b < q.n_bins; b++) {
        const size_t c = ((size_t)r * q.n_pulses + j) * q.n_bins + b;
        const bool zero = zero_row >= 0 && j == (uint32_t)zero_row;
        cube[2 * c] = zero ? 0.0 : cube_re(r, j, b, q.n_bins); cube[2 * c + 1] = zero ? 0.0 : cube_im(r, j, b);
    }
    return cube;
}
// only bins first_bin .. first_bin + n_gate - 1 of rows first .. first + P - 1 stay addressable
static void poison_but(double* cube, const RtsCubeParams& q, uint32_t first, uint32_t P, uint32_t first_bin, uint32_t n_gate)
{
    const size_t cells = (size_t)q.n_rx * q.n_pulses * q.n_bins;
    FOCUS_POISON(cube, sizeof(double) * 2 * cells);
    for (uint32_t r = 0; r < q.n_rx; r++) for (uint32_t j = 0; j < P; j++)
        FOCUS_UNPOISON(cube + 2 * (((size_t)r * q.n_pulses + first + j) * q.n_bins + first_bin), sizeof(double) * 2 * n_gate);
}
static void print_all(const double* v, size_t n) { for (size_t i = 0; i < n; i++) printf("%.17g%c", v[i], i + 1 == n ? '\n' : ' '); }

int main()
{
    char name[32]; char line[1024];
    while (fgets(line, sizeof(line), stdin)) {
        double v[16] = {0}; int used = 0;
        if (sscanf(line, "%31s%n", name, &used) != 1) continue;
        int n = 0; for (const char* s = line + used; n < 16; n++) { int k = 0; if (sscanf(s, "%lf%n", &v[n], &k) != 1) break; s += k; }
        RtsCubeParams q; memset(&q, 0, sizeof(q)); q.n_rx = (uint32_t)v[0]; q.n_pulses = (uint32_t)v[1]; q.n_bins = (uint32_t)v[2]; q.dt = 1.0;
        if (!strcmp(name, "consts")) printf("%u %u %u %u %u %u %u %u %u %u\n", RTS_ALIGN_MAX_LAG, RTS_ALIGN_MAX_ITERS, RTS_ALIGN_PULSE_CHUNK, RTS_ALIGN_BIN_BLOCK, RTS_ALIGN_LDS_SUMS,
                                            RTS_PGA_MAX_PULSES, RTS_PGA_MAX_ITERS, RTS_PGA_BIN_TILE, RTS_PGA_LDS_MAX, RTS_FOCUS_MAX_RX);
        else if (!strcmp(name, "pgaplan") && n == 3) {        // n_rx, N, n_gate
            const RtsPgaPlan p = rts_pga_plan((uint32_t)v[0], (uint32_t)v[1], (uint32_t)v[2], 3u, 0u, 0u);
            printf("%u %u %u %u %zu %zu %zu %u %u %d\n", p.logN, p.BT, p.passes, p.tiles, p.lds, p.partial_doubles, p.out_doubles, p.window0, p.window_min, p.supported ? 1 : 0);
        }
        else if (!strcmp(name, "alignplan") && n == 5) {      // n_rx, n_pulses, n_bins, n_gate, max_lag
            const RtsAlignPlan p = rts_align_plan((uint32_t)v[0], (uint32_t)v[1], (uint32_t)v[2], (uint32_t)v[3], (uint32_t)v[4]);
            printf("%u %u %u %zu %zu %zu %d\n", p.n_lags, p.n_blocks, p.blocks_per_pass, p.env_doubles, p.ref_doubles, p.out_doubles, p.supported ? 1 : 0);
        }
        else if (!strcmp(name, "align") && n == 11) {         // n_rx rows n_bins first_pulse P first_bin n_gate max_lag n_iters flags zero_row
            RtsAlignParams p; memset(&p, 0, sizeof(p));
            p.first_pulse = (uint32_t)v[3]; p.n_pulses = (uint32_t)v[4]; p.first_bin = (uint32_t)v[5]; p.n_gate = (uint32_t)v[6];
            p.max_lag = (uint32_t)v[7]; p.n_iters = (uint32_t)v[8]; p.flags = (uint32_t)v[9];
            const RtsAlignPlan plan = rts_align_plan(q.n_rx, p.n_pulses, q.n_bins, p.n_gate, p.max_lag);
            double* cube = make_cube(q, (int)v[10]);
            poison_but(cube, q, p.first_pulse, p.n_pulses, 0, q.n_bins);
            double* out = new double[plan.out_doubles];
            double* work = new double[(size_t)p.n_pulses * q.n_bins + plan.n_gate + plan.n_lags];
            rts_align_eval_host(&q, cube, &p, plan, out, work);
            print_all(out, plan.out_doubles);
            FOCUS_UNPOISON(cube, sizeof(double) * 2 * (size_t)q.n_rx * q.n_pulses * q.n_bins);
            delete[] work; delete[] out; delete[] cube;
        }
        else if (!strcmp(name, "pga") && n == 10) {           // n_rx rows n_bins first_pulse N first_bin n_gate n_iters window0 window_min
            RtsPgaParams p; memset(&p, 0, sizeof(p));
            p.first_pulse = (uint32_t)v[3]; p.n_pulses = (uint32_t)v[4]; p.first_bin = (uint32_t)v[5]; p.n_gate = (uint32_t)v[6];
            p.n_iters = (uint32_t)v[7]; p.window0 = (uint32_t)v[8]; p.window_min = (uint32_t)v[9];
            const RtsPgaPlan plan = rts_pga_plan(q.n_rx, p.n_pulses, p.n_gate, p.n_iters, p.window0, p.window_min);
            double* cube = make_cube(q, -1);
            poison_but(cube, q, p.first_pulse, p.n_pulses, p.first_bin, p.n_gate);
            double* out = new double[plan.out_doubles];
            double* work = new double[14 * (size_t)p.n_pulses];
            rts_pga_eval_host(&q, cube, &p, plan, out, out + (size_t)q.n_rx * p.n_pulses, work);
            print_all(out, plan.out_doubles);
            FOCUS_UNPOISON(cube, sizeof(double) * 2 * (size_t)q.n_rx * q.n_pulses * q.n_bins);
            delete[] work; delete[] out; delete[] cube;
        }
        else if (!strcmp(name, "correct") && n == 7) {        // n_rx rows n_bins first_pulse P taps mode (1: shifts, 2: phase, 3: both)
            RtsCorrectParams p; memset(&p, 0, sizeof(p));
            p.first_pulse = (uint32_t)v[3]; p.n_pulses = (uint32_t)v[4]; p.taps = (uint32_t)v[5];
            const uint32_t mode = (uint32_t)v[6];
            const size_t rows = (size_t)q.n_rx * p.n_pulses;
            double* shifts = nullptr; double* phase = nullptr;
            if (mode & 1u) { shifts = new double[rows]; for (size_t i = 0; i < rows; i++) shifts[i] = ((double)((i * 3u) % 11u) - 5.0) * 0.5; }
            if (mode & 2u) { phase = new double[rows]; for (size_t i = 0; i < rows; i++) phase[i] = ((double)(i % 9u) - 4.0) * 0.375; }
            double* cube = make_cube(q, -1);
            poison_but(cube, q, p.first_pulse, p.n_pulses, 0, q.n_bins);
            double* work = new double[2 * (size_t)q.n_bins];
            rts_correct_eval_host(&q, cube, &p, shifts, phase, work);
            FOCUS_UNPOISON(cube, sizeof(double) * 2 * (size_t)q.n_rx * q.n_pulses * q.n_bins);
            print_all(cube, 2 * (size_t)q.n_rx * q.n_pulses * q.n_bins);
            delete[] work; delete[] cube; delete[] shifts; delete[] phase;
        }
        else { fprintf(stderr, "bad case: %s", line); return 2; }
    }
    return 0;
}
