// Driver of tests/test_adapt_host.py: rts_amd/csrc/rts_adapt.h alone, built with a plain host compiler (under AddressSanitizer +
// UndefinedBehaviorSanitizer where it has them).  One case per line on stdin, the results on stdout; the expectations live in the
// test.  "cov" runs the covariance's evaluator on a heap input of which ONLY the training cells are addressable -- everything else is
// poisoned, so a read of a row, a bin or a skipped bin outside the set is a sanitizer report; "mvdr" runs the solve on a heap
// covariance of which only the lower triangle and the diagonal's real parts are addressable.  Outputs and work arrays are heap
// arrays of exactly their sizes.  "covplan", "mvdrplan", "block" and "consts" print the plans and the constants they stand on.
#include "rts_adapt.h"
#include <cstdio>
#include <cstring>
#include <vector>
#if defined(__SANITIZE_ADDRESS__) && defined(__has_include)
#if __has_include(<sanitizer/asan_interface.h>)
#include <sanitizer/asan_interface.h>
#define ADAPT_POISON(p, n) ASAN_POISON_MEMORY_REGION(p, n)
#define ADAPT_UNPOISON(p, n) ASAN_UNPOISON_MEMORY_REGION(p, n)
#endif
#endif
#ifndef ADAPT_POISON
#define ADAPT_POISON(p, n) ((void)(p), (void)(n))
#define ADAPT_UNPOISON(p, n) ((void)(p), (void)(n))
#endif

// the input of the cov cases (tests/test_adapt_host.py: main_input), the covariance and the steering of the mvdr cases (main_cov, main_steering)
static double in_re(uint32_t r, uint32_t p, uint32_t b) { return (double)((r * 131u + p * 17u + b * 7u) % 23u) - 11.0 + 0.25 * (double)p; }
static double in_im(uint32_t r, uint32_t p, uint32_t b) { return (double)((r * 5u + p * 3u + b * 11u) % 19u) - 9.0 - 0.5 * (double)b; }
static double cov_re(uint32_t i, uint32_t j, uint32_t n) { return i == j ? (double)n + 0.25 * (double)i : ((double)((i * 7u + j * 3u) % 5u) - 2.0) / 8.0; }
static double cov_im(uint32_t i, uint32_t j) { return ((double)((i * 5u + j * 11u) % 7u) - 3.0) / 16.0; }
static double s_re(uint32_t b, uint32_t r) { return ((double)((b * 7u + r * 3u) % 11u) - 5.0) / 8.0; }
static double s_im(uint32_t b, uint32_t r) { return ((double)((b * 5u + r * 13u) % 9u) - 4.0) / 16.0 + 0.03125; }

int main()
{
    char name[32]; static char line[65536];
    while (fgets(line, sizeof(line), stdin)) {
        std::vector<double> v; int used = 0;
        if (sscanf(line, "%31s%n", name, &used) != 1) continue;
        for (const char* s = line + used;;) { double x; int k = 0; if (sscanf(s, "%lf%n", &x, &k) != 1) break; v.push_back(x); s += k; }
        const size_t n = v.size();
        if (!strcmp(name, "consts"))
            printf("%u %u %u %u %u %u %u %llu\n", RTS_ADAPT_TILE, RTS_ADAPT_MAX_PARTS, RTS_ADAPT_BLOCK, RTS_ADAPT_WAVE, RTS_ADAPT_MAX_THREADS, RTS_ADAPT_REDUCE_THREADS, RTS_MVDR_THREADS, RTS_ADAPT_MAX_TILES);
        else if (!strcmp(name, "covplan") && n == 3) {       // n_rx n_rows kept
            const RtsCovPlan p = rts_cov_plan((uint32_t)v[0], (uint32_t)v[1], (uint32_t)v[2]);
            printf("%llu %llu %u %u %u %u %u %zu %zu %zu %d\n", (unsigned long long)p.K, (unsigned long long)p.tiles, p.parts, p.block_rows, p.blocks, p.threads, p.reduce_groups,
                   p.lds, p.scratch_bytes, p.out_doubles, p.supported ? 1 : 0);
        }
        else if (!strcmp(name, "mvdrplan") && n == 2) {      // n_rx n_beams
            const RtsMvdrPlan p = rts_mvdr_plan((uint32_t)v[0], (uint32_t)v[1]);
            printf("%u %zu %zu %d\n", p.passes, p.lds, p.out_doubles, p.supported ? 1 : 0);
        }
        else if (!strcmp(name, "block") && n == 1) { uint32_t bi, bj; rts_cov_block((uint32_t)v[0], &bi, &bj); printf("%u %u\n", bi, bj); }
        else if (!strcmp(name, "parts") && n == 2) {         // tiles parts: the first tile of every part and the end
            for (uint32_t p = 0; p <= (uint32_t)v[1]; p++) printf("%llu%c", (unsigned long long)rts_cov_part_begin((uint64_t)v[0], (uint32_t)v[1], p), p == (uint32_t)v[1] ? '\n' : ' ');
        }
        else if (!strcmp(name, "cov") && n == 9) {           // n_rx n_rows_in n_bins first_row n_rows first_bin span skip_first skip_n (all resolved: no zeros that mean "to the last")
            const uint32_t n_rx = (uint32_t)v[0], rows_in = (uint32_t)v[1], nb = (uint32_t)v[2];
            RtsCovSet set; set.first_row = (uint32_t)v[3]; set.n_rows = (uint32_t)v[4]; set.first_bin = (uint32_t)v[5];
            const uint32_t span = (uint32_t)v[6], skip_first = (uint32_t)v[7]; set.skip_n = (uint32_t)v[8];
            set.kept = span - set.skip_n; set.skip_at = set.skip_n ? skip_first - set.first_bin : set.kept;
            const RtsCovPlan plan = rts_cov_plan(n_rx, set.n_rows, set.kept);
            const size_t cells_in = (size_t)n_rx * rows_in * nb;
            double* in = new double[2 * cells_in];
            for (uint32_t r = 0; r < n_rx; r++) for (uint32_t j = 0; j < rows_in; j++) for (uint32_t b = 0; b < nb; b++) {
                const size_t c = ((size_t)r * rows_in + j) * nb + b; in[2 * c] = in_re(r, j, b); in[2 * c + 1] = in_im(r, j, b); }
            ADAPT_POISON(in, sizeof(double) * 2 * cells_in);
            for (uint32_t r = 0; r < n_rx; r++) for (uint64_t c = 0; c < plan.K; c++)
                ADAPT_UNPOISON(in + 2 * ((size_t)r * rows_in * nb + rts_cov_cell_index(set, nb, c)), 2 * sizeof(double));
            double* out = new double[plan.out_doubles];
            rts_cov_eval_host(n_rx, nb, in, rows_in, set, plan, out);
            for (size_t i = 0; i < plan.out_doubles; i++) printf("%.17g%c", out[i], i + 1 == plan.out_doubles ? '\n' : ' ');
            ADAPT_UNPOISON(in, sizeof(double) * 2 * cells_in);
            delete[] out; delete[] in;
        }
        else if (!strcmp(name, "mvdr") && n == 4) {          // n_rx n_beams loading diagonal_scale (the diagonal is scaled: <= 0 fails a pivot)
            const uint32_t m = (uint32_t)v[0], beams = (uint32_t)v[1];
            double* cov = new double[2 * (size_t)m * m];
            for (uint32_t i = 0; i < m; i++) for (uint32_t j = 0; j < m; j++) {
                cov[2 * ((size_t)i * m + j)] = cov_re(i, j, m) * (i == j ? v[3] : 1.0); cov[2 * ((size_t)i * m + j) + 1] = cov_im(i, j); }
            ADAPT_POISON(cov, sizeof(double) * 2 * m * m);
            for (uint32_t i = 0; i < m; i++) { ADAPT_UNPOISON(cov + 2 * (size_t)i * m, sizeof(double) * 2 * i); ADAPT_UNPOISON(cov + 2 * ((size_t)i * m + i), sizeof(double)); }
            double* s = new double[2 * (size_t)beams * m];
            for (uint32_t b = 0; b < beams; b++) for (uint32_t r = 0; r < m; r++) { s[2 * ((size_t)b * m + r)] = s_re(b, r); s[2 * ((size_t)b * m + r) + 1] = s_im(b, r); }
            const RtsMvdrPlan plan = rts_mvdr_plan(m, beams);
            double* L = new double[2 * (size_t)m * m]; double* x = new double[2 * (size_t)m]; double* out = new double[plan.out_doubles];
            const int pivot = rts_mvdr_eval_host(cov, m, beams, s, v[2], L, x, out);
            if (pivot >= 0) printf("%d\n", pivot);
            else for (size_t i = 0; i < plan.out_doubles; i++) printf("%.17g%c", out[i], i + 1 == plan.out_doubles ? '\n' : ' ');
            ADAPT_UNPOISON(cov, sizeof(double) * 2 * m * m);
            delete[] out; delete[] x; delete[] L; delete[] s; delete[] cov;
        }
        else { fprintf(stderr, "bad case: %s", line); return 2; }
    }
    return 0;
}
