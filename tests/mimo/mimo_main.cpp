// Driver of tests/test_mimo_host.py: rts_amd/csrc/rts_mimo.h alone, built with a plain host compiler (under AddressSanitizer +
// UndefinedBehaviorSanitizer where it has them).  One case per line on stdin, the results on stdout; the expectations live in the
// test.  "bank" runs the evaluator on a heap cube of which ONLY the span's rows are addressable -- the rows outside it are poisoned,
// so a read there is a sanitizer report; the waveforms, the code table and the output are heap arrays of exactly their sizes.
// "plan" and "rule" print the plan and the number of the rule.
#include "rts_mimo.h"
#include <cstdio>
#include <cstring>
#include <vector>
#if defined(__SANITIZE_ADDRESS__) && defined(__has_include)
#if __has_include(<sanitizer/asan_interface.h>)
#include <sanitizer/asan_interface.h>
#define MIMO_POISON(p, n) ASAN_POISON_MEMORY_REGION(p, n)
#define MIMO_UNPOISON(p, n) ASAN_UNPOISON_MEMORY_REGION(p, n)
#endif
#endif
#ifndef MIMO_POISON
#define MIMO_POISON(p, n) ((void)(p), (void)(n))
#define MIMO_UNPOISON(p, n) ((void)(p), (void)(n))
#endif

// the input of the bank cases (tests/test_mimo_host.py: main_input, main_wave, main_code): small dyadic values
static double in_re(uint32_t r, uint32_t p, uint32_t b) { return ((double)((r * 131u + p * 17u + b * 7u) % 23u) - 11.0) / 8.0 + 0.25 * (double)p; }
static double in_im(uint32_t r, uint32_t p, uint32_t b) { return ((double)((r * 5u + p * 3u + b * 11u) % 19u) - 9.0) / 16.0 - 0.03125 * (double)b; }
static double wave_re(uint32_t t, uint32_t m) { return ((double)((t * 37u + m * 13u) % 17u) - 8.0) / 4.0; }
static double wave_im(uint32_t t, uint32_t m) { return ((double)((t * 11u + m * 5u) % 13u) - 6.0) / 8.0; }
static double code_re(uint32_t t, uint32_t p) { return ((double)((t * 3u + p * 7u) % 5u) - 2.0) / 2.0; }
static double code_im(uint32_t t, uint32_t p) { return ((double)((t * 5u + p * 2u) % 7u) - 3.0) / 4.0; }

int main()
{
    char name[32]; static char line[65536];
    while (fgets(line, sizeof(line), stdin)) {
        std::vector<double> v; int used = 0;
        if (sscanf(line, "%31s%n", name, &used) != 1) continue;
        for (const char* s = line + used;;) { double x; int k = 0; if (sscanf(s, "%lf%n", &x, &k) != 1) break; v.push_back(x); s += k; }
        const size_t n = v.size();
        if (!strcmp(name, "plan") && n >= 5 && n == 5 + (size_t)v[3] && v[3] <= RTS_BANK_MAX_WAVES) {      // n_rx n_rows n_bins n_waves code M...
            uint32_t M[RTS_BANK_MAX_WAVES] = {0};
            for (uint32_t t = 0; t < (uint32_t)v[3]; t++) M[t] = (uint32_t)v[5 + t];
            const RtsBankPlan p = rts_bank_plan((uint32_t)v[0], (uint32_t)v[1], (uint32_t)v[2], (uint32_t)v[3], M, v[4] != 0.0);
            printf("%u %u %u %u %u %u %u %zu %zu %zu %zu %u %d\n", p.tiles, p.group, p.groups, p.max_M, p.Q, p.S, p.blocks, p.lds, p.out_doubles, p.tab_doubles, p.code_off,
                   p.off[(uint32_t)v[3] - 1u], p.supported ? 1 : 0);
        }
        else if (!strcmp(name, "rule") && n == 6) {          // n_pulses n_waves first n reserved null_waves
            RtsBankParams p; memset(&p, 0, sizeof(p));
            RtsWaveform w; memset(&w, 0, sizeof(w));
            p.waves = v[5] != 0.0 ? nullptr : &w; p.n_waves = (uint32_t)v[1]; p.first_pulse = (uint32_t)v[2]; p.n_pulses = (uint32_t)v[3]; p.reserved[1] = (uint64_t)v[4];
            printf("%d\n", rts_bank_rule(&p, (uint32_t)v[0]));
        }
        else if (!strcmp(name, "bank") && n >= 7 && n == 7 + (size_t)v[5]) {      // n_rx n_p N first count n_waves code M...
            RtsCubeParams q; memset(&q, 0, sizeof(q)); q.n_rx = (uint32_t)v[0]; q.n_pulses = (uint32_t)v[1]; q.n_bins = (uint32_t)v[2]; q.dt = 1.0;
            RtsBankParams p; memset(&p, 0, sizeof(p));
            p.first_pulse = (uint32_t)v[3]; p.n_pulses = (uint32_t)v[4]; p.n_waves = (uint32_t)v[5];
            std::vector<RtsWaveform> waves(p.n_waves); std::vector<double*> samples(p.n_waves); uint32_t M[RTS_BANK_MAX_WAVES] = {0};
            for (uint32_t t = 0; t < p.n_waves; t++) {
                M[t] = (uint32_t)v[7 + t];
                samples[t] = new double[2 * (size_t)M[t]];
                for (uint32_t m = 0; m < M[t]; m++) { samples[t][2 * m] = wave_re(t, m); samples[t][2 * m + 1] = wave_im(t, m); }
                memset(&waves[t], 0, sizeof(RtsWaveform)); waves[t].samples = samples[t]; waves[t].n_samples = M[t]; waves[t].taps = 1;
            }
            p.waves = waves.data();
            double* code = nullptr;
            if (v[6] != 0.0) {
                code = new double[2 * (size_t)p.n_waves * p.n_pulses];
                for (uint32_t t = 0; t < p.n_waves; t++) for (uint32_t r = 0; r < p.n_pulses; r++) { code[2 * ((size_t)t * p.n_pulses + r)] = code_re(t, r); code[2 * ((size_t)t * p.n_pulses + r) + 1] = code_im(t, r); }
            }
            p.code = code;
            if (rts_bank_rule(&p, q.n_pulses) || rts_bank_code_bad(code, p.n_waves, p.n_pulses) >= 0) { fprintf(stderr, "refused: %s", line); return 3; }
            const RtsBankPlan plan = rts_bank_plan(q.n_rx, p.n_pulses, q.n_bins, p.n_waves, M, code != nullptr);
            if (!plan.supported) { fprintf(stderr, "no plan: %s", line); return 3; }
            const size_t cells = (size_t)q.n_rx * q.n_pulses * q.n_bins;
            double* cube = new double[2 * cells];
            for (uint32_t r = 0; r < q.n_rx; r++) for (uint32_t row = 0; row < q.n_pulses; row++) for (uint32_t b = 0; b < q.n_bins; b++) {
                const size_t c = ((size_t)r * q.n_pulses + row) * q.n_bins + b; cube[2 * c] = in_re(r, row, b); cube[2 * c + 1] = in_im(r, row, b); }
            for (uint32_t r = 0; r < q.n_rx; r++) for (uint32_t row = 0; row < q.n_pulses; row++)
                if (row < p.first_pulse || row >= p.first_pulse + p.n_pulses) MIMO_POISON(cube + 2 * ((size_t)r * q.n_pulses + row) * q.n_bins, sizeof(double) * 2 * q.n_bins);
            double* out = new double[plan.out_doubles];
            rts_bank_eval_host(&q, cube, &p, out);
            for (size_t i = 0; i < plan.out_doubles; i++) printf("%a%c", out[i], i + 1 == plan.out_doubles ? '\n' : ' ');
            delete[] out;
            MIMO_UNPOISON(cube, sizeof(double) * 2 * cells); delete[] cube;
            delete[] code;
            for (uint32_t t = 0; t < p.n_waves; t++) delete[] samples[t];
        }
        else { fprintf(stderr, "bad case: %s", line); return 2; }
    }
    return 0;
}
