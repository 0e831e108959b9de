// Driver of tests/test_stap_host.py: rts_amd/csrc/rts_stap.h alone, built with a plain host compiler (under AddressSanitizer +
// UndefinedBehaviorSanitizer where it has them).  One case per line on stdin, the results on stdout; the expectations live in the
// test.  "stcov" runs the stacked covariance's evaluator on a heap input of which ONLY the elements of the training snapshots are
// addressable -- everything else is poisoned, so a read of a row, a bin or a skipped bin outside them is a sanitizer report;
// "stapply" runs the filter's evaluator on an input of which only the span's rows are addressable.  Outputs are heap arrays of
// exactly their sizes.  "applyplan" and "consts" print the filter's plan and the constants it stands on.
#include "rts_stap.h"
#include <cstdio>
#include <cstring>
#include <vector>
#if defined(__SANITIZE_ADDRESS__) && defined(__has_include)
#if __has_include(<sanitizer/asan_interface.h>)
#include <sanitizer/asan_interface.h>
#define STAP_POISON(p, n) ASAN_POISON_MEMORY_REGION(p, n)
#define STAP_UNPOISON(p, n) ASAN_UNPOISON_MEMORY_REGION(p, n)
#endif
#endif
#ifndef STAP_POISON
#define STAP_POISON(p, n) ((void)(p), (void)(n))
#define STAP_UNPOISON(p, n) ((void)(p), (void)(n))
#endif

// the input of the cases (tests/test_adapt_host.py: main_input) and the weights of the stapply cases (main_steering)
static double in_re(uint32_t r, uint32_t p, uint32_t b) { return (double)((r * 131u + p * 17u + b * 7u) % 23u) - 11.0 + 0.25 * (double)p; }
static double in_im(uint32_t r, uint32_t p, uint32_t b) { return (double)((r * 5u + p * 3u + b * 11u) % 19u) - 9.0 - 0.5 * (double)b; }
static double w_re(uint32_t f, uint32_t d) { return ((double)((f * 7u + d * 3u) % 11u) - 5.0) / 8.0; }
static double w_im(uint32_t f, uint32_t d) { return ((double)((f * 5u + d * 13u) % 9u) - 4.0) / 16.0 + 0.03125; }

static double* make_input(uint32_t n_rx, uint32_t rows_in, uint32_t nb)
{
    double* in = new double[2 * (size_t)n_rx * rows_in * nb];
    for (uint32_t r = 0; r < n_rx; r++) for (uint32_t j = 0; j < rows_in; j++) for (uint32_t b = 0; b < nb; b++) {
        const size_t c = ((size_t)r * rows_in + j) * nb + b; in[2 * c] = in_re(r, j, b); in[2 * c + 1] = in_im(r, j, b); }
    return in;
}

int main()
{
    char name[32]; static char line[65536];
    while (fgets(line, sizeof(line), stdin)) {
        std::vector<double> v; int used = 0;
        if (sscanf(line, "%31s%n", name, &used) != 1) continue;
        for (const char* s = line + used;;) { double x; int k = 0; if (sscanf(s, "%lf%n", &x, &k) != 1) break; v.push_back(x); s += k; }
        const size_t n = v.size();
        if (!strcmp(name, "consts"))
            printf("%u %u %u %u %u %u %u %u %u\n", RTS_ST_MAX_TAPS, RTS_ST_THREADS, RTS_ST_STRIP, RTS_ST_RX_TILE, RTS_ST_MAX_GRID_X, RTS_BEAM_MAX_RX, RTS_BEAM_MAX_BEAMS, RTS_BEAM_MAX_WEIGHTS, RTS_ADAPT_TILE);
        else if (!strcmp(name, "tile") && n == 1) printf("%u\n", RTS_ST_FILTER_TILE((uint32_t)v[0]));
        else if (!strcmp(name, "applyplan") && n == 6) {     // n_rx n_taps n_filters n_rows n_bins flags
            const RtsStApplyPlan p = rts_st_apply_plan((uint32_t)v[0], (uint32_t)v[1], (uint32_t)v[2], (uint32_t)v[3], (uint32_t)v[4], (uint32_t)v[5]);
            printf("%u %u %u %u %u %u %u %llu %zu %zu %d\n", p.D, p.out_rows, p.filter_tile, p.filter_tiles, p.strips, p.bin_groups, p.groups, (unsigned long long)p.out_cells,
                   p.lds, p.out_doubles, p.supported ? 1 : 0);
        }
        else if (!strcmp(name, "stcov") && n == 10) {        // n_rx n_taps n_rows_in n_bins first_row n_rows first_bin span skip_first skip_n (all resolved; n_rows: the span's rows)
            const uint32_t n_rx = (uint32_t)v[0], taps = (uint32_t)v[1], rows_in = (uint32_t)v[2], nb = (uint32_t)v[3];
            RtsCovSet set; set.first_row = (uint32_t)v[4]; set.n_rows = (uint32_t)v[5] - (taps - 1u); set.first_bin = (uint32_t)v[6];
            const uint32_t span = (uint32_t)v[7], skip_first = (uint32_t)v[8]; set.skip_n = (uint32_t)v[9];
            set.kept = span - set.skip_n; set.skip_at = set.skip_n ? skip_first - set.first_bin : set.kept;
            const uint32_t D = n_rx * taps;
            const RtsCovPlan plan = rts_cov_plan(D, set.n_rows, set.kept);
            const size_t cells_in = (size_t)n_rx * rows_in * nb;
            double* in = make_input(n_rx, rows_in, nb);
            STAP_POISON(in, sizeof(double) * 2 * cells_in);
            for (uint32_t d = 0; d < D; d++) for (uint64_t c = 0; c < plan.K; c++)
                STAP_UNPOISON(in + 2 * (rts_st_offset(d, n_rx, (uint64_t)rows_in * nb, nb) + rts_cov_cell_index(set, nb, c)), 2 * sizeof(double));
            double* out = new double[plan.out_doubles];
            rts_st_cov_eval_host(n_rx, taps, nb, in, rows_in, set, plan, out);
            for (size_t i = 0; i < plan.out_doubles; i++) printf("%.17g%c", out[i], i + 1 == plan.out_doubles ? '\n' : ' ');
            STAP_UNPOISON(in, sizeof(double) * 2 * cells_in);
            delete[] out; delete[] in;
        }
        else if (!strcmp(name, "stapply") && n == 8) {       // n_rx n_taps n_rows_in n_bins first_row n_rows n_filters flags
            const uint32_t n_rx = (uint32_t)v[0], taps = (uint32_t)v[1], rows_in = (uint32_t)v[2], nb = (uint32_t)v[3], first = (uint32_t)v[4], rows = (uint32_t)v[5];
            const uint32_t F = (uint32_t)v[6], flags = (uint32_t)v[7], D = n_rx * taps;
            const RtsStApplyPlan plan = rts_st_apply_plan(n_rx, taps, F, rows, nb, flags);
            if (!plan.supported) { fprintf(stderr, "unsupported: %s", line); return 2; }
            const size_t cells_in = (size_t)n_rx * rows_in * nb;
            double* in = make_input(n_rx, rows_in, nb);
            STAP_POISON(in, sizeof(double) * 2 * cells_in);
            for (uint32_t r = 0; r < n_rx; r++) STAP_UNPOISON(in + 2 * (((size_t)r * rows_in + first) * nb), sizeof(double) * 2 * (size_t)rows * nb);
            double* w = new double[2 * (size_t)F * D];
            for (uint32_t f = 0; f < F; f++) for (uint32_t d = 0; d < D; d++) { w[2 * ((size_t)f * D + d)] = w_re(f, d); w[2 * ((size_t)f * D + d) + 1] = w_im(f, d); }
            double* out = new double[plan.out_doubles];
            rts_st_apply_eval_host(n_rx, taps, nb, in, rows_in, first, rows, F, w, flags, out);
            for (size_t i = 0; i < plan.out_doubles; i++) printf("%.17g%c", out[i], i + 1 == plan.out_doubles ? '\n' : ' ');
            STAP_UNPOISON(in, sizeof(double) * 2 * cells_in);
            delete[] out; delete[] w; delete[] in;
        }
        else { fprintf(stderr, "bad case: %s", line); return 2; }
    }
    return 0;
}
