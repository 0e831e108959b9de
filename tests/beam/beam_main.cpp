// Driver of tests/test_beam_host.py: rts_amd/csrc/rts_beam.h and rts_cfar.h alone, built with a plain host compiler (under
// AddressSanitizer + UndefinedBehaviorSanitizer where it has them).  One case per line on stdin, the results on stdout; the
// expectations live in the test.  "beam" runs the evaluator on a heap input of which ONLY the rows the definition reads are
// addressable -- everything else is poisoned, so a read of a row outside the span is a sanitizer report; the weights and the output
// are heap arrays of exactly their sizes.  "peak" pushes a list of powers through the streaming peak; "delta" is rts_cfar.h's
// refinement; "plan" and "consts" print the launch plan and the constants it stands on.
#include "rts_beam.h"
#include "rts_cfar.h"
#include <cstdio>
#include <cstring>
#include <vector>
#if defined(__SANITIZE_ADDRESS__) && defined(__has_include)
#if __has_include(<sanitizer/asan_interface.h>)
#include <sanitizer/asan_interface.h>
#define BEAM_POISON(p, n) ASAN_POISON_MEMORY_REGION(p, n)
#define BEAM_UNPOISON(p, n) ASAN_UNPOISON_MEMORY_REGION(p, n)
#endif
#endif
#ifndef BEAM_POISON
#define BEAM_POISON(p, n) ((void)(p), (void)(n))
#define BEAM_UNPOISON(p, n) ((void)(p), (void)(n))
#endif

// the input and the weights of the beam cases (tests/test_beam_host.py: main_input, main_weights)
static double in_re(uint32_t r, uint32_t p, uint32_t b) { return (double)((r * 131u + p * 17u + b * 7u) % 23u) - 11.0 + 0.25 * (double)p; }
static double in_im(uint32_t r, uint32_t p, uint32_t b) { return (double)((r * 5u + p * 3u + b * 11u) % 19u) - 9.0 - 0.5 * (double)b; }
static double w_re(uint32_t b, uint32_t r) { return ((double)((b * 7u + r * 3u) % 11u) - 5.0) / 8.0; }
static double w_im(uint32_t b, uint32_t r) { return ((double)((b * 5u + r * 13u) % 9u) - 4.0) / 16.0; }

int main()
{
    char name[32]; static char line[65536];
    while (fgets(line, sizeof(line), stdin)) {
        std::vector<double> v; int used = 0;
        if (sscanf(line, "%31s%n", name, &used) != 1) continue;
        for (const char* s = line + used;;) { double x; int k = 0; if (sscanf(s, "%lf%n", &x, &k) != 1) break; v.push_back(x); s += k; }
        const size_t n = v.size();
        if (!strcmp(name, "consts"))
            printf("%u %u %u %u %u %u %u\n", RTS_BEAM_THREADS, RTS_BEAM_RX_TILE, RTS_BEAM_BEAM_TILE, RTS_BEAM_MAX_GRID_X, RTS_BEAM_MAX_RX, RTS_BEAM_MAX_BEAMS, RTS_BEAM_MAX_WEIGHTS);
        else if (!strcmp(name, "plan") && n == 5) {          // n_rx n_beams n_rows n_bins flags
            const RtsBeamPlan p = rts_beam_plan((uint32_t)v[0], (uint32_t)v[1], (uint32_t)v[2], (uint32_t)v[3], (uint32_t)v[4]);
            printf("%u %u %u %llu %zu %zu %d\n", p.groups, p.rx_tiles, p.beam_tiles, (unsigned long long)p.cells, p.lds, p.out_doubles, p.supported ? 1 : 0);
        }
        else if (!strcmp(name, "delta") && n == 3) printf("%.17g\n", rts_cfar_delta(v[0], v[1], v[2]));
        else if (!strcmp(name, "peak") && n >= 1) {          // the powers of one cell, in beam order
            double* P = new double[n];                       // (exactly n: the streaming record indexes nothing, the driver must not either)
            for (size_t i = 0; i < n; i++) P[i] = v[i];
            RtsBeamPeak pk = {0.0, 0.0, 0.0, 0.0, 0u, 0u};
            for (size_t i = 0; i < n; i++) rts_beam_peak_push(&pk, (uint32_t)i, P[i]);
            double best, coordinate; rts_beam_peak_finish(&pk, (uint32_t)n, &best, &coordinate);
            printf("%.17g %.17g\n", best, coordinate);
            delete[] P;
        }
        else if (!strcmp(name, "beam") && n == 7) {          // n_rx n_rows_in n_bins first_row n_rows n_beams flags
            const uint32_t n_rx = (uint32_t)v[0], rows_in = (uint32_t)v[1], nb = (uint32_t)v[2], first = (uint32_t)v[3], rows = (uint32_t)v[4], beams = (uint32_t)v[5], flags = (uint32_t)v[6];
            const size_t cells_in = (size_t)n_rx * rows_in * nb;
            double* in = new double[2 * cells_in];
            for (uint32_t r = 0; r < n_rx; r++) for (uint32_t j = 0; j < rows_in; j++) for (uint32_t b = 0; b < nb; b++) {
                const size_t c = ((size_t)r * rows_in + j) * nb + b; in[2 * c] = in_re(r, j, b); in[2 * c + 1] = in_im(r, j, b); }
            BEAM_POISON(in, sizeof(double) * 2 * cells_in);
            for (uint32_t r = 0; r < n_rx; r++) BEAM_UNPOISON(in + 2 * (((size_t)r * rows_in + first) * nb), sizeof(double) * 2 * (size_t)rows * nb);
            double* w = new double[2 * (size_t)beams * n_rx];
            for (uint32_t b = 0; b < beams; b++) for (uint32_t r = 0; r < n_rx; r++) { w[2 * ((size_t)b * n_rx + r)] = w_re(b, r); w[2 * ((size_t)b * n_rx + r) + 1] = w_im(b, r); }
            const RtsBeamPlan plan = rts_beam_plan(n_rx, beams, rows, nb, flags);
            double* out = new double[plan.out_doubles];
            rts_beam_eval_host(n_rx, nb, in, rows_in, first, rows, beams, w, flags, out);
            for (size_t i = 0; i < plan.out_doubles; i++) printf("%.17g%c", out[i], i + 1 == plan.out_doubles ? '\n' : ' ');
            BEAM_UNPOISON(in, sizeof(double) * 2 * cells_in);
            delete[] out; delete[] w; delete[] in;
        }
        else { fprintf(stderr, "bad case: %s", line); return 2; }
    }
    return 0;
}
