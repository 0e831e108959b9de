// Driver of tests/test_passive_host.py: rts_amd/csrc/rts_passive.h alone, built with a plain host compiler (under AddressSanitizer +
// UndefinedBehaviorSanitizer where it has them).  One case per line on stdin, the results on stdout; the expectations live in the
// test.  "cancel" and "xcorr" run the evaluators on a heap cube of which ONLY the span's rows are addressable -- the rows outside it
// are poisoned, so a read or a write there is a sanitizer report; coefficient, output and work arrays are heap arrays of exactly
// their sizes.  "cancelplan", "xcorrplan", "cancelrule" and "xcorrrule" print the plans and the numbers of the rules.
#include "rts_passive.h"
#include <cstdio>
#include <cstring>
#include <vector>
#if defined(__SANITIZE_ADDRESS__) && defined(__has_include)
#if __has_include(<sanitizer/asan_interface.h>)
#include <sanitizer/asan_interface.h>
#define PASSIVE_POISON(p, n) ASAN_POISON_MEMORY_REGION(p, n)
#define PASSIVE_UNPOISON(p, n) ASAN_UNPOISON_MEMORY_REGION(p, n)
#endif
#endif
#ifndef PASSIVE_POISON
#define PASSIVE_POISON(p, n) ((void)(p), (void)(n))
#define PASSIVE_UNPOISON(p, n) ((void)(p), (void)(n))
#endif

// the input of the cancel and xcorr cases (tests/test_passive_host.py: main_input)
static double in_re(uint32_t r, uint32_t p, uint32_t b) { return ((double)((r * 131u + p * 17u + b * 7u) % 23u) - 11.0) / 8.0 + 0.25 * (double)p; }
static double in_im(uint32_t r, uint32_t p, uint32_t b) { return ((double)((r * 5u + p * 3u + b * 11u) % 19u) - 9.0) / 16.0 - 0.03125 * (double)b; }

// a heap cube [n_rx][n_p][N] with the rows outside first .. first + count poisoned
static double* make_cube(uint32_t n_rx, uint32_t n_p, uint32_t N, uint32_t first, uint32_t count)
{
    double* cube = new double[2 * (size_t)n_rx * n_p * N];
    for (uint32_t r = 0; r < n_rx; r++) for (uint32_t p = 0; p < n_p; p++) for (uint32_t b = 0; b < N; b++) {
        const size_t c = ((size_t)r * n_p + p) * N + b; cube[2 * c] = in_re(r, p, b); cube[2 * c + 1] = in_im(r, p, b); }
    for (uint32_t r = 0; r < n_rx; r++) for (uint32_t p = 0; p < n_p; p++)
        if (p < first || p >= first + count) PASSIVE_POISON(cube + 2 * ((size_t)r * n_p + p) * N, sizeof(double) * 2 * N);
    return cube;
}
static void free_cube(double* cube, uint32_t n_rx, uint32_t n_p, uint32_t N)
{
    PASSIVE_UNPOISON(cube, sizeof(double) * 2 * (size_t)n_rx * n_p * N);
    delete[] cube;
}

int main()
{
    char name[32]; static char line[65536];
    while (fgets(line, sizeof(line), stdin)) {
        std::vector<double> v; int used = 0;
        if (sscanf(line, "%31s%n", name, &used) != 1) continue;
        for (const char* s = line + used;;) { double x; int k = 0; if (sscanf(s, "%lf%n", &x, &k) != 1) break; v.push_back(x); s += k; }
        const size_t n = v.size();
        if (!strcmp(name, "cancelplan") && n == 5) {         // n_rx n_bins n_rows rows_per_block K
            const RtsCancelPlan p = rts_cancel_plan((uint32_t)v[0], (uint32_t)v[1], (uint32_t)v[2], (uint32_t)v[3], (uint32_t)v[4]);
            printf("%u %u %u %u %u %u %u %u %u %zu %zu %zu %zu %zu %d\n", p.K, p.R, p.n_blocks, p.tpr, p.ppb, p.tri, p.stride, p.gram_blocks, p.gram_threads, p.gram_lds, p.solve_lds,
                   p.scratch_doubles, p.sums_doubles, p.coeff_doubles, p.supported ? 1 : 0);
        }
        else if (!strcmp(name, "xcorrplan") && n == 3) {     // n_rx n_rows n_lags
            const RtsXcorrPlan p = rts_xcorr_plan((uint32_t)v[0], (uint32_t)v[1], (uint32_t)v[2]);
            printf("%u %zu %zu %d\n", p.lag_groups, p.lds, p.out_doubles, p.supported ? 1 : 0);
        }
        else if (!strcmp(name, "cancelrule") && n == 10) {   // n_rx n_pulses ref_rx n_taps first n rows_per_block reserved rx_mask loading
            RtsCancelParams p; memset(&p, 0, sizeof(p));
            p.ref_rx = (uint32_t)v[2]; p.n_taps = (uint32_t)v[3]; p.first_pulse = (uint32_t)v[4]; p.n_pulses = (uint32_t)v[5]; p.rows_per_block = (uint32_t)v[6];
            p.reserved[1] = (uint64_t)v[7]; p.rx_mask = (uint64_t)v[8]; p.loading = v[9];
            printf("%d\n", rts_cancel_rule(&p, (uint32_t)v[0], (uint32_t)v[1]));
        }
        else if (!strcmp(name, "xcorrrule") && n == 9) {     // n_rx n_pulses n_bins ref_rx first n first_lag n_lags reserved
            RtsXcorrParams p; memset(&p, 0, sizeof(p));
            p.ref_rx = (uint32_t)v[3]; p.first_pulse = (uint32_t)v[4]; p.n_pulses = (uint32_t)v[5]; p.first_lag = (uint32_t)v[6]; p.n_lags = (uint32_t)v[7]; p.reserved0 = (uint32_t)v[8];
            printf("%d\n", rts_xcorr_rule(&p, (uint32_t)v[0], (uint32_t)v[1], (uint32_t)v[2]));
        }
        else if (!strcmp(name, "cancel") && n == 10) {       // n_rx n_p N ref_rx K first count rows_per_block rx_mask loading
            RtsCubeParams q; memset(&q, 0, sizeof(q)); q.n_rx = (uint32_t)v[0]; q.n_pulses = (uint32_t)v[1]; q.n_bins = (uint32_t)v[2]; q.dt = 1.0;
            RtsCancelParams p; memset(&p, 0, sizeof(p));
            p.ref_rx = (uint32_t)v[3]; p.n_taps = (uint32_t)v[4]; p.first_pulse = (uint32_t)v[5]; p.n_pulses = (uint32_t)v[6]; p.rows_per_block = (uint32_t)v[7];
            p.rx_mask = (uint64_t)v[8]; p.loading = v[9];
            if (rts_cancel_rule(&p, q.n_rx, q.n_pulses)) { fprintf(stderr, "refused: %s", line); return 3; }
            const RtsCancelPlan plan = rts_cancel_plan(q.n_rx, q.n_bins, p.n_pulses, p.rows_per_block, p.n_taps);
            double* cube = make_cube(q.n_rx, q.n_pulses, q.n_bins, p.first_pulse, p.n_pulses);
            double* coeffs = new double[plan.coeff_doubles]; double* work = new double[rts_cancel_work_doubles(plan.K)];
            uint32_t failed = 0;
            rts_cancel_eval_host(&q, cube, &p, plan, coeffs, &failed, work);
            printf("%u %u", plan.n_blocks, failed);
            for (size_t i = 0; i < plan.coeff_doubles; i++) printf(" %a", coeffs[i]);
            for (uint32_t r = 0; r < q.n_rx; r++) for (uint32_t row = 0; row < p.n_pulses; row++) for (uint32_t b = 0; b < 2 * q.n_bins; b++)
                printf(" %a", cube[2 * (((size_t)r * q.n_pulses + p.first_pulse + row) * q.n_bins) + b]);
            printf("\n");
            delete[] work; delete[] coeffs; free_cube(cube, q.n_rx, q.n_pulses, q.n_bins);
        }
        else if (!strcmp(name, "xcorr") && n == 8) {         // n_rx n_p N ref_rx first count first_lag n_lags
            RtsCubeParams q; memset(&q, 0, sizeof(q)); q.n_rx = (uint32_t)v[0]; q.n_pulses = (uint32_t)v[1]; q.n_bins = (uint32_t)v[2]; q.dt = 1.0;
            RtsXcorrParams p; memset(&p, 0, sizeof(p));
            p.ref_rx = (uint32_t)v[3]; p.first_pulse = (uint32_t)v[4]; p.n_pulses = (uint32_t)v[5]; p.first_lag = (uint32_t)v[6]; p.n_lags = (uint32_t)v[7];
            if (rts_xcorr_rule(&p, q.n_rx, q.n_pulses, q.n_bins)) { fprintf(stderr, "refused: %s", line); return 3; }
            const RtsXcorrPlan plan = rts_xcorr_plan(q.n_rx, p.n_pulses, p.n_lags);
            double* cube = make_cube(q.n_rx, q.n_pulses, q.n_bins, p.first_pulse, p.n_pulses);
            double* out = new double[plan.out_doubles];
            rts_xcorr_eval_host(&q, cube, &p, out);
            for (size_t i = 0; i < plan.out_doubles; i++) printf("%a%c", out[i], i + 1 == plan.out_doubles ? '\n' : ' ');
            delete[] out; free_cube(cube, q.n_rx, q.n_pulses, q.n_bins);
        }
        else { fprintf(stderr, "bad case: %s", line); return 2; }
    }
    return 0;
}
