// Driver of tests/test_doa_host.py: rts_amd/csrc/rts_doa.h alone, built with a plain host compiler (under AddressSanitizer +
// UndefinedBehaviorSanitizer where it has them).  One case per line on stdin, the results on stdout; the expectations live in the
// test.  "eig" runs the solver on a heap matrix of which ONLY the lower triangle and the diagonal's real parts are addressable --
// everything else is poisoned, so a read of the upper triangle is a sanitizer report; "scan" runs the scan on a heap table of
// vectors of which only the rows first .. first + m - 1 are addressable.  Outputs and work arrays are heap arrays of exactly their
// sizes.  "eigplan", "scanplan", "pairs", "rank", "weights", "count" and "consts" print the plans, the pairing, the sort, the pure
// functions and the constants they stand on.
#include "rts_doa.h"
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#if defined(__SANITIZE_ADDRESS__) && defined(__has_include)
#if __has_include(<sanitizer/asan_interface.h>)
#include <sanitizer/asan_interface.h>
#define DOA_POISON(p, n) ASAN_POISON_MEMORY_REGION(p, n)
#define DOA_UNPOISON(p, n) ASAN_UNPOISON_MEMORY_REGION(p, n)
#endif
#endif
#ifndef DOA_POISON
#define DOA_POISON(p, n) ((void)(p), (void)(n))
#define DOA_UNPOISON(p, n) ((void)(p), (void)(n))
#endif

// the matrix of the eig cases (tests/test_doa_host.py: main_cov), the vectors and the table of the scan cases (main_vectors, main_table)
static double cov_re(uint32_t i, uint32_t j, uint32_t n) { return i == j ? (double)n + 0.25 * (double)i : ((double)((i * 7u + j * 3u) % 5u) - 2.0) / 8.0; }
static double cov_im(uint32_t i, uint32_t j) { return ((double)((i * 5u + j * 11u) % 7u) - 3.0) / 16.0; }
static double v_re(uint32_t k, uint32_t r) { return ((double)((k * 7u + r * 3u) % 11u) - 5.0) / 8.0; }
static double v_im(uint32_t k, uint32_t r) { return ((double)((k * 5u + r * 13u) % 9u) - 4.0) / 16.0 + 0.03125; }
static double a_re(uint32_t r, uint64_t d) { return ((double)((r * 3u + d * 5u) % 13u) - 6.0) / 4.0; }
static double a_im(uint32_t r, uint64_t d) { return ((double)((r * 11u + d * 7u) % 17u) - 8.0) / 8.0; }

int main()
{
    char name[32]; static char line[65536];
    while (fgets(line, sizeof(line), stdin)) {
        std::vector<double> v; std::vector<unsigned long long> u; int used = 0;
        if (sscanf(line, "%31s%n", name, &used) != 1) continue;
        for (const char* s = line + used;;) { double x; int k = 0; if (sscanf(s, "%lf%n", &x, &k) != 1) break; v.push_back(x); u.push_back(strtoull(s, nullptr, 10)); s += k; }
        const size_t n = v.size();
        if (!strcmp(name, "consts"))
            printf("%u %u %u %u %u %u %u\n", RTS_EIG_MAX_SWEEPS, RTS_EIG_THREADS, RTS_DOA_THREADS, RTS_DOA_RX_TILE, RTS_DOA_VEC_TILE, RTS_DOA_MAX_GRID_X, RTS_BEAM_MAX_RX);
        else if (!strcmp(name, "eigplan") && n == 1) {       // n
            const RtsEigPlan p = rts_eig_plan((uint32_t)v[0]);
            printf("%u %u %zu %zu %zu %d\n", p.rounds, p.slots, p.lds, p.value_doubles, p.vector_doubles, p.supported ? 1 : 0);
        }
        else if (!strcmp(name, "scanplan") && n == 3) {      // n m n_dirs (an integer up to 2^64 - 1)
            const RtsDoaScanPlan p = rts_doa_scan_plan((uint32_t)v[0], (uint32_t)v[1], (uint64_t)u[2]);
            printf("%u %u %u %zu %zu %d\n", p.groups, p.rx_tiles, p.vec_tiles, p.lds, p.out_doubles, p.supported ? 1 : 0);
        }
        else if (!strcmp(name, "pairs") && n == 1) {         // n: every (p, q) of a sweep, round by round, slot by slot; a bye as (n, n)
            const uint32_t m = (uint32_t)v[0]; const RtsEigPlan p = rts_eig_plan(m);
            printf("%u %u", p.rounds, p.slots);
            for (uint32_t r = 0; r < p.rounds; r++) for (uint32_t k = 0; k < p.slots; k++) {
                uint32_t a, b; rts_eig_pair_of(m, r, k, &a, &b);
                if (b >= m) printf(" %u %u", m, m); else printf(" %u %u", a, b);
            }
            printf("\n");
        }
        else if (!strcmp(name, "rank") && n >= 1) {          // the values: the rank of every column
            double* lam = new double[n];
            for (size_t i = 0; i < n; i++) lam[i] = v[i];
            for (size_t i = 0; i < n; i++) printf("%u%c", rts_eig_rank(lam, (uint32_t)n, (uint32_t)i), i + 1 == n ? '\n' : ' ');
            delete[] lam;
        }
        else if (!strcmp(name, "eig") && n == 2) {           // n diagonal_scale: status sweeps, then the values and the vectors
            const uint32_t m = (uint32_t)v[0]; const RtsEigPlan plan = rts_eig_plan(m);
            double* cov = new double[2 * (size_t)m * m];
            for (uint32_t i = 0; i < m; i++) for (uint32_t j = 0; j < m; j++) {
                cov[2 * ((size_t)i * m + j)] = cov_re(i, j, m) * (i == j ? v[1] : 1.0); cov[2 * ((size_t)i * m + j) + 1] = cov_im(i, j); }
            DOA_POISON(cov, sizeof(double) * 2 * m * m);
            for (uint32_t i = 0; i < m; i++) { DOA_UNPOISON(cov + 2 * (size_t)i * m, sizeof(double) * 2 * i); DOA_UNPOISON(cov + 2 * ((size_t)i * m + i), sizeof(double)); }
            double* X = new double[plan.vector_doubles]; double* V = new double[plan.vector_doubles]; double* lam = new double[m];
            double* values = new double[plan.value_doubles]; double* vectors = new double[plan.vector_doubles];
            uint32_t sweeps = 0;
            const uint32_t status = rts_eig_eval_host(cov, m, X, V, lam, values, vectors, &sweeps);
            printf("%u %u", status, sweeps);
            if (!status) { for (uint32_t i = 0; i < m; i++) printf(" %.17g", values[i]); for (size_t i = 0; i < plan.vector_doubles; i++) printf(" %.17g", vectors[i]); }
            printf("\n");
            DOA_UNPOISON(cov, sizeof(double) * 2 * m * m);
            delete[] vectors; delete[] values; delete[] lam; delete[] V; delete[] X; delete[] cov;
        }
        else if (!strcmp(name, "scan") && n == 6) {          // n rows first m n_dirs inverse: the table has `rows` vectors, g_k = 0.5 + k / 4
            const uint32_t m = (uint32_t)v[0], rows = (uint32_t)v[1], first = (uint32_t)v[2], cnt = (uint32_t)v[3]; const uint64_t nd = (uint64_t)u[4];
            const RtsDoaScanPlan plan = rts_doa_scan_plan(m, cnt, nd);
            double* tab = new double[2 * (size_t)rows * m];
            for (uint32_t k = 0; k < rows; k++) for (uint32_t r = 0; r < m; r++) { tab[2 * ((size_t)k * m + r)] = v_re(k, r); tab[2 * ((size_t)k * m + r) + 1] = v_im(k, r); }
            DOA_POISON(tab, sizeof(double) * 2 * rows * m);
            DOA_UNPOISON(tab + 2 * (size_t)first * m, sizeof(double) * 2 * cnt * m);
            double* g = new double[cnt];
            for (uint32_t k = 0; k < cnt; k++) g[k] = 0.5 + 0.25 * (double)k;
            double* a = new double[2 * (size_t)m * nd];
            for (uint32_t r = 0; r < m; r++) for (uint64_t d = 0; d < nd; d++) { a[2 * ((size_t)r * nd + d)] = a_re(r, d); a[2 * ((size_t)r * nd + d) + 1] = a_im(r, d); }
            double* out = new double[plan.out_doubles];
            rts_doa_scan_eval_host(tab + 2 * (size_t)first * m, g, m, cnt, a, nd, v[5] != 0.0 ? RTS_DOA_INVERSE : 0u, out);
            for (size_t i = 0; i < plan.out_doubles; i++) printf("%.17g%c", out[i], i + 1 == plan.out_doubles ? '\n' : ' ');
            DOA_UNPOISON(tab, sizeof(double) * 2 * rows * m);
            delete[] out; delete[] a; delete[] g; delete[] tab;
        }
        else if (!strcmp(name, "weights") && n >= 4) {       // method n_sources loading values...: the refusal, then first m flags g...
            const uint32_t m = (uint32_t)(n - 3);
            double* lam = new double[m]; double* g = new double[m];
            for (uint32_t i = 0; i < m; i++) lam[i] = v[3 + i];
            uint32_t first = 0, cnt = 0, flags = 0, bad = 0;
            const int rc = rts_doa_weights_host((uint32_t)v[0], lam, m, (uint32_t)v[1], v[2], &first, &cnt, g, &flags, &bad);
            printf("%d", rc);
            if (!rc) { printf(" %u %u %u", first, cnt, flags); for (uint32_t k = 0; k < cnt; k++) printf(" %.17g", g[k]); }
            printf("\n");
            delete[] g; delete[] lam;
        }
        else if (!strcmp(name, "count") && n >= 3) {         // K criterion values...
            const uint32_t m = (uint32_t)(n - 2);
            double* lam = new double[m];
            for (uint32_t i = 0; i < m; i++) lam[i] = v[2 + i];
            printf("%u\n", rts_source_count_host(lam, m, (uint64_t)u[0], (uint32_t)v[1]));
            delete[] lam;
        }
        else { fprintf(stderr, "bad case: %s", line); return 2; }
    }
    return 0;
}
