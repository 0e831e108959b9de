// Driver of tests/test_beat_host.py: rts_amd/csrc/rts_beat.h alone, built with a plain host compiler (under AddressSanitizer +
// UndefinedBehaviorSanitizer where it has them).  One case per line on stdin, the results on stdout; the expectations live in the
// test.  "beat" runs the beat evaluator on heap arrays of exactly their sizes (contributions, cube, work).  "range" runs the range
// evaluator on a heap cube of which ONLY the samples the definition reads are addressable -- the gate's samples of the span's rows
// -- and everything else is poisoned, so a read of a row outside the span or of a sample outside the gate is a sanitizer report;
// the window and the output are heap arrays of exactly their sizes.
#include "rts_beat.h"
#include <cstdio>
#include <cstring>
#include <vector>
#if defined(__SANITIZE_ADDRESS__) && defined(__has_include)
#if __has_include(<sanitizer/asan_interface.h>)
#include <sanitizer/asan_interface.h>
#define BEAT_POISON(p, n) ASAN_POISON_MEMORY_REGION(p, n)
#define BEAT_UNPOISON(p, n) ASAN_UNPOISON_MEMORY_REGION(p, n)
#endif
#endif
#ifndef BEAT_POISON
#define BEAT_POISON(p, n) ((void)(p), (void)(n))
#define BEAT_UNPOISON(p, n) ((void)(p), (void)(n))
#endif

// the cube of the range cases: y[r][p][b] (tests/test_beat_host.py: main_cube)
static double cube_re(uint32_t r, uint32_t p, uint32_t b) { return (double)((r * 131u + p * 17u + b * 7u) % 23u) - 11.0 + 0.25 * (double)p; }
static double cube_im(uint32_t r, uint32_t p, uint32_t b) { return (double)((r * 5u + p * 3u + b * 11u) % 19u) - 9.0 - 0.5 * (double)b; }

// contribution k of the beat cases (tests/test_beat_host.py: main_contributions): receivers -1 .. n_rx, delays on and off the grid,
// before the row and beyond it, every 13th not finite
static RtsBeatContribution contribution(uint32_t k, uint32_t n_rx, uint32_t nb, double t0, double dt)
{
    RtsBeatContribution c; memset(&c, 0, sizeof(c));
    c.rx = (int32_t)(k % (n_rx + 2u)) - 1;
    c.re = ((double)((k * 7u) % 11u) - 5.0) / 4.0; c.im = ((double)((k * 3u) % 7u) - 3.0) / 4.0;
    c.delay = t0 + dt * ((double)((k * 37u) % (nb + 40u)) - 20.0 + 0.25 * (double)(k % 4u));
    if (k % 13u == 5u) c.delay = k % 2u ? INFINITY : (k % 4u ? NAN : -INFINITY);
    c.doppler = ((double)(k % 9u) - 4.0) * 2.5e5;
    return c;
}

int main()
{
    char name[32]; char line[1024];
    while (fgets(line, sizeof(line), stdin)) {
        double v[16] = {0}; int used = 0;
        if (sscanf(line, "%31s%n", name, &used) != 1) continue;
        int n = 0; for (const char* s = line + used; n < 16; n++) { int k = 0; if (sscanf(s, "%lf%n", &v[n], &k) != 1) break; s += k; }
        if (!strcmp(name, "consts"))
            printf("%u %u %u %u %u %u %u %u %u %u %u %u\n", RTS_BEAT_STRIP, RTS_BEAT_MAX_PARTS, RTS_BEAT_THREADS, RTS_BEAT_TILE, RTS_BEAT_FILL, RTS_BEAT_PART_MIN,
                   RTS_BEAT_ONE_BELOW, RTS_RANGE_MAX_FFT, RTS_RANGE_THREADS, RTS_RANGE_ROW_TILE, RTS_RANGE_TILE_ELEMS, RTS_RANGE_MAX_GRID_X);
        else if (!strcmp(name, "beatplan") && n == 4) {      // R, n_rx, n_bins, force_parts
            const RtsBeatPlan p = rts_beat_plan((uint64_t)v[0], (uint32_t)v[1], (uint32_t)v[2], (uint32_t)v[3]);
            printf("%u %u %u %zu %d\n", p.tiles, p.P, p.part_len, p.scratch_doubles, p.supported ? 1 : 0);
        }
        else if (!strcmp(name, "rangeplan") && n == 5) {     // n_rx, n_pulses, n_samples, n_fft, n_out
            const RtsRangePlan p = rts_range_plan((uint32_t)v[0], (uint32_t)v[1], (uint32_t)v[2], (uint32_t)v[3], (uint32_t)v[4]);
            printf("%u %u %u %u %u %llu %zu %zu %d\n", p.logN, p.RT, p.n_samples, p.n_out, p.groups, (unsigned long long)p.rows, p.lds, p.out_doubles, p.supported ? 1 : 0);
        }
        else if (!strcmp(name, "beat") && n == 10) {         // n_rx rows n_bins pulse n_contributions t0 dt slope duration doppler
            RtsCubeParams q; memset(&q, 0, sizeof(q)); q.n_rx = (uint32_t)v[0]; q.n_pulses = (uint32_t)v[1]; q.n_bins = (uint32_t)v[2]; q.t0 = v[5]; q.dt = v[6];
            RtsBeatParams p; memset(&p, 0, sizeof(p)); p.slope = v[7]; p.duration = v[8]; p.flags = v[9] != 0.0 ? RTS_RENDER_DOPPLER : 0u;
            const uint32_t pulse = (uint32_t)v[3], cnt = (uint32_t)v[4];
            RtsBeatContribution* c = new RtsBeatContribution[cnt];
            for (uint32_t k = 0; k < cnt; k++) c[k] = contribution(k, q.n_rx, q.n_bins, q.t0, q.dt);
            const size_t cells = (size_t)q.n_rx * q.n_pulses * q.n_bins;
            double* cube = new double[2 * cells];
            for (size_t i = 0; i < 2 * cells; i++) cube[i] = 0.0;
            double* work = new double[2 * (size_t)q.n_rx * q.n_bins];
            rts_beat_eval_host(&q, &p, c, cnt, pulse, cube, work);
            for (size_t i = 0; i < 2 * cells; i++) printf("%.17g%c", cube[i], i + 1 == 2 * cells ? '\n' : ' ');
            delete[] work; delete[] cube; delete[] c;
        }
        else if (!strcmp(name, "range") && n == 11) {        // n_rx rows n_bins first_pulse n_pulses first_bin n_samples n_fft n_out flags tapered
            RtsCubeParams q; memset(&q, 0, sizeof(q)); q.n_rx = (uint32_t)v[0]; q.n_pulses = (uint32_t)v[1]; q.n_bins = (uint32_t)v[2]; q.dt = 1.0;
            RtsRangeParams p; memset(&p, 0, sizeof(p));
            p.first_pulse = (uint32_t)v[3]; p.n_pulses = (uint32_t)v[4]; p.first_bin = (uint32_t)v[5]; p.n_samples = (uint32_t)v[6];
            p.n_fft = (uint32_t)v[7]; p.n_out = (uint32_t)v[8]; p.flags = (uint32_t)v[9];
            const uint32_t ns = p.n_samples ? p.n_samples : q.n_bins - p.first_bin;
            const RtsRangePlan plan = rts_range_plan(q.n_rx, p.n_pulses, ns, p.n_fft, p.n_out);
            const size_t cells = (size_t)q.n_rx * q.n_pulses * q.n_bins;
            double* cube = new double[2 * cells];
            for (uint32_t r = 0; r < q.n_rx; r++) for (uint32_t j = 0; j < q.n_pulses; j++) for (uint32_t b = 0; b < q.n_bins; b++) {
                const size_t c = ((size_t)r * q.n_pulses + j) * q.n_bins + b; cube[2 * c] = cube_re(r, j, b); cube[2 * c + 1] = cube_im(r, j, b); }
            BEAT_POISON(cube, sizeof(double) * 2 * cells);
            for (uint32_t r = 0; r < q.n_rx; r++) for (uint32_t j = 0; j < p.n_pulses; j++)
                BEAT_UNPOISON(cube + 2 * (((size_t)r * q.n_pulses + p.first_pulse + j) * q.n_bins + p.first_bin), sizeof(double) * 2 * ns);
            double* w = nullptr;
            if (v[10] != 0.0) { w = new double[ns]; for (uint32_t i = 0; i < ns; i++) w[i] = 0.5 + 0.25 * (double)i; }
            p.window = w;
            double* out = new double[plan.out_doubles];
            double* work = new double[3 * (size_t)p.n_fft];
            rts_range_eval_host(&q, cube, &p, plan, out, work);
            for (size_t i = 0; i < plan.out_doubles; i++) printf("%.17g%c", out[i], i + 1 == plan.out_doubles ? '\n' : ' ');
            BEAT_UNPOISON(cube, sizeof(double) * 2 * cells);
            delete[] work; delete[] out; delete[] w; delete[] cube;
        }
        else { fprintf(stderr, "bad case: %s", line); return 2; }
    }
    return 0;
}
