// Driver of tests/test_cfar_os_host.py: rts_amd/csrc/rts_cfar_os.h and the rts_cfar.h it includes alone, built with a plain host compiler (under AddressSanitizer +
// UndefinedBehaviorSanitizer where it has them).  One case per line on stdin, the results on stdout; the expectations live in the
// test.  Every array is a heap array of exactly its size, so a read or write past one is a sanitizer report: the keys of "select",
// the alpha table of "table" (N0 + 1 entries), and in "eval" the map, the key scratch (N0), the alpha table and the output
// (`capacity` records).
#include "rts_cfar_os.h"
#include <cstdio>
#include <cstring>
#include <vector>

// the map of the eval cases: z[rx][k][r]
static double map_re(uint32_t rx, uint32_t k, uint32_t r) { return (double)((rx * 131u + k * 17u + r * 7u) % 23u) - 11.0 + 0.25 * (double)k; }
static double map_im(uint32_t rx, uint32_t k, uint32_t r) { return (double)((rx * 5u + k * 3u + r * 11u) % 19u) - 9.0 - 0.5 * (double)(r % 5u); }

// The training count as the two detectors' kernels each wrote it before rts_cfar_count: the mean-level kernel's halves ...
static int imax(int a, int b) { return a > b ? a : b; }
static int imin(int a, int b) { return a < b ? a : b; }
static int former_half(int gr, int gd, int tr, int td, int edge)
{
    const int Or = gr + tr, Od = gd + td;
    const int no = imax(0, imin(Or, edge) - gr), ni = imin(gr, edge);
    return no * (2 * Od + 1) + ni * 2 * td;
}
// ... and the ordered-statistic header's total
static int former_total(int gr, int gd, int tr, int td, int edge_l, int edge_r)
{
    const int Or = gr + tr, Od = gd + td;
    const int cl = edge_l < Or ? edge_l : Or, cr = edge_r < Or ? edge_r : Or;
    const int nlo = cl > gr ? cl - gr : 0, nli = cl < gr ? cl : gr;
    const int nro = cr > gr ? cr - gr : 0, nri = cr < gr ? cr : gr;
    return (nlo + nro) * (2 * Od + 1) + (nli + nri + 1) * 2 * td;
}

int main()
{
    char name[32]; static char line[1 << 16];
    while (fgets(line, sizeof(line), stdin)) {
        int used = 0;
        if (sscanf(line, "%31s%n", name, &used) != 1) continue;
        std::vector<double> v;
        for (const char* s = line + used;;) { double x; int k = 0; if (sscanf(s, "%lf%n", &x, &k) != 1) break; v.push_back(x); s += k; }
        const size_t n = v.size();
        if (!strcmp(name, "n0") && n == 4) printf("%u\n", rts_cfar_n0((uint32_t)v[0], (uint32_t)v[1], (uint32_t)v[2], (uint32_t)v[3]));
        else if (!strcmp(name, "counts") && n == 5) {        // gr gd tr td n_bins: the training count of every range bin
            const int nb = (int)v[4];
            const RtsCfarWindow w = rts_cfar_window((uint32_t)v[0], (uint32_t)v[1], (uint32_t)v[2], (uint32_t)v[3]);
            for (int r = 0; r < nb; r++) printf("%d%c", rts_cfar_count(w, r, nb - 1 - r), r + 1 == nb ? '\n' : ' ');
        }
        else if (!strcmp(name, "halves") && n == 5) {        // gr gd tr td n_bins: "nl nr" of every range bin
            const int nb = (int)v[4];
            const RtsCfarWindow w = rts_cfar_window((uint32_t)v[0], (uint32_t)v[1], (uint32_t)v[2], (uint32_t)v[3]);
            for (int r = 0; r < nb; r++) { int nl, nr; rts_cfar_count(w, r, nb - 1 - r, &nl, &nr); printf("%d %d%c", nl, nr, r + 1 == nb ? '\n' : ' '); }
        }
        else if (!strcmp(name, "halves") && n == 1) {        // limit: every window of up to `limit` cells per field, every pair of edge distances up to
            const int lim = (int)v[0];                       // Or + 1 (beyond Or nothing changes): "checked mismatches" against the two former texts
            unsigned long long checked = 0, bad = 0;
            for (int gr = 0; gr <= lim; gr++) for (int gd = 0; gd <= lim; gd++) for (int tr = 0; tr <= lim; tr++) for (int td = 0; td <= lim; td++) {
                const RtsCfarWindow w = rts_cfar_window((uint32_t)gr, (uint32_t)gd, (uint32_t)tr, (uint32_t)td);
                for (int el = 0; el <= gr + tr + 1; el++) for (int er = 0; er <= gr + tr + 1; er++) {
                    int nl, nr; const int total = rts_cfar_count(w, el, er, &nl, &nr);
                    checked++;
                    if (nl != former_half(gr, gd, tr, td, el) || nr != former_half(gr, gd, tr, td, er) || total != former_total(gr, gd, tr, td, el, er) ||
                        total != nl + nr + 2 * td || total != rts_cfar_count(w, el, er)) bad++;
                }
            }
            printf("%llu %llu\n", checked, bad);
        }
        else if (!strcmp(name, "ranks") && n == 2) {         // rank N0: the rank of every N in 1 .. N0
            const uint32_t N0 = (uint32_t)v[1];
            for (uint32_t N = 1; N <= N0; N++) printf("%u%c", rts_cfar_os_rank((uint32_t)v[0], N, N0), N == N0 ? '\n' : ' ');
        }
        else if (!strcmp(name, "alpha") && n == 3) printf("%.17g\n", rts_cfar_os_alpha_solve((uint32_t)v[0], (uint32_t)v[1], v[2]));
        else if (!strcmp(name, "table") && n == 7) {         // gr gd tr td rank pfa n_bins: the N0 + 1 entries
            const uint32_t N0 = rts_cfar_n0((uint32_t)v[0], (uint32_t)v[1], (uint32_t)v[2], (uint32_t)v[3]);
            double* tab = new double[N0 + 1]();
            rts_cfar_os_alpha_table((uint32_t)v[0], (uint32_t)v[1], (uint32_t)v[2], (uint32_t)v[3], (uint32_t)v[4], v[5], (uint32_t)v[6], tab);
            for (uint32_t i = 0; i <= N0; i++) printf("%.17g%c", tab[i], i == N0 ? '\n' : ' ');
            delete[] tab;
        }
        else if (!strcmp(name, "select") && n >= 2) {        // k x_0 x_1 ...: the k-th smallest, through the keys and back
            const size_t cnt = n - 1;
            uint64_t* keys = new uint64_t[cnt];
            for (size_t i = 0; i < cnt; i++) keys[i] = rts_cfar_os_key(v[i + 1]);
            printf("%.17g\n", rts_cfar_os_unkey(rts_cfar_os_select(keys, cnt, (size_t)v[0])));
            delete[] keys;
        }
        else if (!strcmp(name, "eval") && n == 12) {         // n_rx n_doppler n_bins gr gd tr td rank flags pfa alpha capacity
            RtsCubeParams q; memset(&q, 0, sizeof(q)); q.n_rx = (uint32_t)v[0]; q.n_pulses = 1; q.n_bins = (uint32_t)v[2]; q.t0 = 0.0; q.dt = 1.0;
            const uint32_t nd = (uint32_t)v[1];
            RtsCfarOsParams p; memset(&p, 0, sizeof(p));
            p.guard_range = (uint32_t)v[3]; p.guard_doppler = (uint32_t)v[4]; p.train_range = (uint32_t)v[5]; p.train_doppler = (uint32_t)v[6];
            p.rank = (uint32_t)v[7]; p.flags = (uint32_t)v[8]; p.pfa = v[9]; p.alpha = v[10];
            const uint32_t capacity = (uint32_t)v[11];
            const uint32_t N0 = rts_cfar_n0(p.guard_range, p.guard_doppler, p.train_range, p.train_doppler);
            const size_t cells = (size_t)q.n_rx * nd * q.n_bins;
            double* map = new double[2 * cells];
            for (uint32_t rx = 0; rx < q.n_rx; rx++) for (uint32_t k = 0; k < nd; k++) for (uint32_t r = 0; r < q.n_bins; r++) {
                const size_t c = ((size_t)rx * nd + k) * q.n_bins + r; map[2 * c] = map_re(rx, k, r); map[2 * c + 1] = map_im(rx, k, r); }
            double* tab = nullptr;
            if (p.pfa != 0.0) { tab = new double[N0 + 1](); rts_cfar_os_alpha_table(p.guard_range, p.guard_doppler, p.train_range, p.train_doppler, p.rank, p.pfa, q.n_bins, tab); }
            uint64_t* keys = new uint64_t[N0];
            RtsDetection* out = new RtsDetection[capacity ? capacity : 1];
            const uint32_t total = rts_cfar_os_eval_host(&q, map, nd, &p, tab, keys, out, capacity);
            printf("%u", total);
            for (uint32_t i = 0; i < total && i < capacity; i++) printf(" %u %u %u %u %.17g %.17g", out[i].rx, out[i].doppler_bin, out[i].range_bin, out[i].n_train, out[i].power, out[i].noise);
            printf("\n");
            delete[] out; delete[] keys; delete[] tab; delete[] map;
        }
        else { fprintf(stderr, "bad case: %s", line); return 2; }
    }
    return 0;
}
