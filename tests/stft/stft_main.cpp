// Driver of tests/test_stft_host.py: rts_amd/csrc/rts_stft.h alone, built with a plain host compiler (under AddressSanitizer +
// UndefinedBehaviorSanitizer where it has them).  One case per line on stdin, the results on stdout; the expectations live in the
// test.  "eval" runs the host evaluator on a heap cube of which ONLY the samples the definition reads are addressable -- the rows
// of the whole frames inside [first_pulse, first_pulse + n_pulses), the bins of the gate -- and everything else is poisoned, so a
// read of a left-over pulse, of a pulse in a gap between frames or of a bin outside the gate is a sanitizer report; the window and
// the output are heap arrays of exactly their sizes.
#include "rts_stft.h"
#include <cstdio>
#include <cstring>
#include <vector>
#if defined(__SANITIZE_ADDRESS__) && defined(__has_include)
#if __has_include(<sanitizer/asan_interface.h>)
#include <sanitizer/asan_interface.h>
#define STFT_POISON(p, n) ASAN_POISON_MEMORY_REGION(p, n)
#define STFT_UNPOISON(p, n) ASAN_UNPOISON_MEMORY_REGION(p, n)
#endif
#endif
#ifndef STFT_POISON
#define STFT_POISON(p, n) ((void)(p), (void)(n))
#define STFT_UNPOISON(p, n) ((void)(p), (void)(n))
#endif

// the cube of the eval cases: y[r][p][b]
static double cube_re(uint32_t r, uint32_t p, uint32_t b) { return (double)((r * 131u + p * 17u + b * 7u) % 23u) - 11.0 + 0.25 * (double)p; }
static double cube_im(uint32_t r, uint32_t p, uint32_t b) { return (double)((r * 5u + p * 3u + b * 11u) % 19u) - 9.0 - 0.5 * (double)b; }

int main()
{
    char name[32]; char line[1024];
    while (fgets(line, sizeof(line), stdin)) {
        double v[16] = {0}; int used = 0;
        if (sscanf(line, "%31s%n", name, &used) != 1) continue;
        int n = 0; for (const char* s = line + used; n < 16; n++) { int k = 0; if (sscanf(s, "%lf%n", &v[n], &k) != 1) break; s += k; }
        if (!strcmp(name, "consts")) printf("%u %u %u %u %u %u\n", RTS_STFT_LDS_MAX, RTS_STFT_THREADS, RTS_STFT_MAX_FFT, RTS_STFT_BIN_TILE, RTS_STFT_MAX_RX, RTS_STFT_MAX_GRID_X);
        else if (!strcmp(name, "plan") && n == 7) {          // n_rx, n_pulses, window_len, hop, n_fft, n_gate, flags
            const RtsStftPlan p = rts_stft_plan((uint32_t)v[0], (uint32_t)v[1], (uint32_t)v[2], (uint32_t)v[3], (uint32_t)v[4], (uint32_t)v[5], (uint32_t)v[6]);
            printf("%u %u %u %u %u %zu %zu %zu %d\n", p.logN, p.BT, p.passes, p.tiles, p.n_frames, p.lds, p.out_doubles, p.partial_doubles, p.supported ? 1 : 0);
        }
        else if (!strcmp(name, "bitrev") && n == 2) printf("%u\n", rts_stft_bitrev((uint32_t)v[0], (uint32_t)v[1]));
        else if (!strcmp(name, "window") && n == 2) {        // kind, n
            const uint32_t cnt = (uint32_t)v[1];
            double* w = new double[cnt];
            rts_stft_window_host((uint32_t)v[0], cnt, w);
            for (uint32_t i = 0; i < cnt; i++) printf("%.17g%c", w[i], i + 1 == cnt ? '\n' : ' ');
            delete[] w;
        }
        else if (!strcmp(name, "eval") && n == 12) {         // n_rx rows n_bins first_pulse n_pulses window_len hop n_fft first_bin n_gate flags tapered
            RtsCubeParams q; memset(&q, 0, sizeof(q)); q.n_rx = (uint32_t)v[0]; q.n_pulses = (uint32_t)v[1]; q.n_bins = (uint32_t)v[2]; q.dt = 1.0;
            RtsStftParams p; memset(&p, 0, sizeof(p));
            p.first_pulse = (uint32_t)v[3]; p.n_pulses = (uint32_t)v[4]; p.window_len = (uint32_t)v[5]; p.hop = (uint32_t)v[6]; p.n_fft = (uint32_t)v[7];
            p.first_bin = (uint32_t)v[8]; p.n_bins = (uint32_t)v[9]; p.flags = (uint32_t)v[10];
            const RtsStftPlan plan = rts_stft_plan(q.n_rx, p.n_pulses, p.window_len, p.hop, p.n_fft, p.n_bins, p.flags);
            const size_t cells = (size_t)q.n_rx * q.n_pulses * q.n_bins;
            double* cube = new double[2 * cells];
            for (uint32_t r = 0; r < q.n_rx; r++) for (uint32_t j = 0; j < q.n_pulses; j++) for (uint32_t b = 0; b < q.n_bins; b++) {
                const size_t c = ((size_t)r * q.n_pulses + j) * q.n_bins + b; cube[2 * c] = cube_re(r, j, b); cube[2 * c + 1] = cube_im(r, j, b); }
            STFT_POISON(cube, sizeof(double) * 2 * cells);
            for (uint32_t r = 0; r < q.n_rx; r++) for (uint32_t f = 0; f < plan.n_frames; f++) for (uint32_t i = 0; i < p.window_len; i++)
                STFT_UNPOISON(cube + 2 * (((size_t)r * q.n_pulses + p.first_pulse + (size_t)f * p.hop + i) * q.n_bins + p.first_bin), sizeof(double) * 2 * p.n_bins);
            double* w = nullptr;
            if (v[11] != 0.0) { w = new double[p.window_len]; for (uint32_t i = 0; i < p.window_len; i++) w[i] = 0.5 + 0.25 * (double)i; }
            p.window = w;
            double* out = new double[plan.out_doubles];
            double* work = new double[4 * (size_t)p.n_fft];
            rts_stft_eval_host(&q, cube, &p, plan, out, work);
            printf("%u", plan.n_frames);
            for (size_t i = 0; i < plan.out_doubles; i++) printf(" %.17g", out[i]);
            printf("\n");
            STFT_UNPOISON(cube, sizeof(double) * 2 * cells);
            delete[] work; delete[] out; delete[] w; delete[] cube;
        }
        else { fprintf(stderr, "bad case: %s", line); return 2; }
    }
    return 0;
}
