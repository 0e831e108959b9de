// rts_cfar_os.h -- the arithmetic of ordered-statistic CFAR (include/rts_amd.h: RtsCfarOsParams), shared by the kernel
// (rts_detect.hip: k_cfar_os), the launch (rts_cube_detect_os) and the host evaluator (rts_cfar_os_eval): the rank rule, the threshold
// factor of a false-alarm rate, the order-preserving 64-bit key of a power, a plain selection, and the evaluator itself.  The window,
// the training count, the local-maximum rule, the refinement and the record are every detector's: rts_cfar.h.  An order statistic has
// no summation order: kernel and evaluator agree on the noise estimate bit for bit.  Includes nothing of HIP: it compiles with any
// host compiler and is tested without a GPU (tests/test_cfar_os_host.py, tests/cfar_os/cfar_os_main.cpp).
#pragma once
#include <math.h>
#include <stdint.h>
#include <stddef.h>
#include <string.h>
#include "../../include/rts_amd.h"
#include "rts_cfar.h"

// the rank of a cell with N of the N0 training cells: ceil(rank N / N0), in [1, N] for rank in [1, N0] and N >= 1
RTS_HD uint32_t rts_cfar_os_rank(uint32_t rank, uint32_t N, uint32_t N0) { return (rank * N + N0 - 1u) / N0; }

// a power (>= 0, or +inf) <-> its 64-bit pattern: for non-negative doubles the patterns order as the values do
RTS_HD uint64_t rts_cfar_os_key(double p)
{
#ifdef __HIP_DEVICE_COMPILE__
    return (uint64_t)__double_as_longlong(p);
#else
    uint64_t k; memcpy(&k, &p, sizeof(k)); return k;
#endif
}
RTS_HD double rts_cfar_os_unkey(uint64_t k)
{
#ifdef __HIP_DEVICE_COMPILE__
    return __longlong_as_double((long long)k);
#else
    double p; memcpy(&p, &k, sizeof(p)); return p;
#endif
}

// ---- host only from here
// The k-th smallest (1-based, 1 <= k <= n) of the n keys at v, which it permutes: Hoare's FIND, partitioning around the value at the
// wanted place until that place is settled.  Keys are integers, so the order is total whatever the powers were.
static inline uint64_t rts_cfar_os_select(uint64_t* v, size_t n, size_t k)
{
    const int64_t want = (int64_t)k - 1;
    int64_t lo = 0, hi = (int64_t)n - 1;
    while (lo < hi) {
        const uint64_t x = v[want];
        int64_t i = lo, j = hi;
        do {
            while (v[i] < x) i++;
            while (x < v[j]) j--;
            if (i <= j) { const uint64_t t = v[i]; v[i] = v[j]; v[j] = t; i++; j--; }
        } while (i <= j);
        if (j < want) lo = i;
        if (want < i) hi = j;
    }
    return v[want];
}

// ln of the false-alarm law's reciprocal, sum_{i<k} ln(1 + alpha / (N - i)), and its derivative in alpha
static inline void rts_cfar_os_law(uint32_t N, uint32_t k, double alpha, double* f, double* df)
{
    double s = 0.0, d = 0.0;
    for (uint32_t i = 0; i < k; i++) { const double m = (double)(N - i); s += log1p(alpha / m); d += 1.0 / (m + alpha); }
    *f = s; *df = d;
}

// The threshold factor of the k-th of N training cells at false-alarm rate pfa: the root of prod_{i<k} (N - i) / (N - i + alpha) = pfa
// (square-law detected complex Gaussian noise).  Newton from 0 on g(alpha) = sum ln(1 + alpha / (N - i)) - ln(1 / pfa): g rises and is
// concave, so every tangent's root lies at or left of g's and the iterates climb to it; they stop when a step no longer raises alpha.
// 1 <= k <= N, 0 < pfa < 1 (the callers check).
static inline double rts_cfar_os_alpha_solve(uint32_t N, uint32_t k, double pfa)
{
    const double L = -log(pfa);
    double a = 0.0;
    for (int it = 0; it < 200; it++) {
        double f, df; rts_cfar_os_law(N, k, a, &f, &df);
        const double next = a + (L - f) / df;
        if (!(next > a)) break;
        a = next;
    }
    return a;
}

// The alphas of a map of n_bins range bins: tab[N] for every training count N that occurs (N depends on a cell's range bin alone, and
// only within Gr + Tr of an edge), each from rts_cfar_os_alpha_solve with the cell's own rank; entries that are already nonzero are kept
// (a caller's cache for one (window, rank, pfa)).  tab holds N0 + 1 doubles.  Returns how many entries it solved for.
static inline uint32_t rts_cfar_os_alpha_table(uint32_t gr, uint32_t gd, uint32_t tr, uint32_t td, uint32_t rank, double pfa, uint32_t n_bins, double* tab)
{
    const RtsCfarWindow w = rts_cfar_window(gr, gd, tr, td);
    const uint32_t N0 = rts_cfar_n0(gr, gd, tr, td), Or = (uint32_t)rts_cfar_Or(w);
    uint32_t solved = 0;
    for (uint32_t r = 0; r < n_bins; r++) {
        if (r > Or + 1u && n_bins - 1u - r > Or + 1u) { r = n_bins - 1u - (Or + 1u) - 1u; continue; }      // (the interior: one count)
        const uint32_t N = (uint32_t)rts_cfar_count(w, (int)r, (int)(n_bins - 1u - r));
        if (tab[N] == 0.0) { tab[N] = rts_cfar_os_alpha_solve(N, rts_cfar_os_rank(rank, N, N0), pfa); solved++; }
    }
    return solved;
}

// The whole detector on the host (validated by the caller): map [n_rx][n_doppler][n_bins] complex, interleaved; alpha_tab: N0 + 1
// alphas by training count (pfa) or NULL (p->alpha); keys: room for N0 values.  Writes up to `capacity` records in flat order and
// returns the total.
static inline uint32_t rts_cfar_os_eval_host(const RtsCubeParams* q, const double* map, uint32_t n_doppler, const RtsCfarOsParams* p, const double* alpha_tab,
                                             uint64_t* keys, RtsDetection* out, uint32_t capacity)
{
    const RtsCfarWindow w = rts_cfar_window(p->guard_range, p->guard_doppler, p->train_range, p->train_doppler);
    const int nd = (int)n_doppler, nb = (int)q->n_bins, Or = rts_cfar_Or(w), Od = rts_cfar_Od(w);
    const uint32_t N0 = rts_cfar_n0(p->guard_range, p->guard_doppler, p->train_range, p->train_doppler);
    const bool local_max = (p->flags & RTS_CFAR_LOCAL_MAX) != 0;
    uint32_t total = 0;
    for (uint32_t rx = 0; rx < q->n_rx; rx++) {
        const double* m = map + 2 * (size_t)rx * n_doppler * q->n_bins;
        const auto power = [m, nb](int k_, int r_) { const double* z = m + 2 * ((size_t)k_ * (size_t)nb + (size_t)r_); return z[0] * z[0] + z[1] * z[1]; };
        for (int k = 0; k < nd; k++)
            for (int r = 0; r < nb; r++) {
                size_t n = 0;                                                  // (counted, not rts_cfar_count: the tests compare the two)
                for (int dk = -Od; dk <= Od; dk++) {
                    int kk = (k + dk) % nd; if (kk < 0) kk += nd;
                    for (int dr = -Or; dr <= Or; dr++) {
                        if ((dk >= -w.gd && dk <= w.gd && dr >= -w.gr && dr <= w.gr) || r + dr < 0 || r + dr >= nb) continue;
                        keys[n++] = rts_cfar_os_key(power(kk, r + dr));
                    }
                }
                const uint32_t kth = rts_cfar_os_rank(p->rank, (uint32_t)n, N0);
                const double noise = rts_cfar_os_unkey(rts_cfar_os_select(keys, n, kth));
                const double alpha = alpha_tab ? alpha_tab[n] : p->alpha;
                const double thr = alpha * noise;
                const double P = power(k, r);
                bool det = P > thr;
                const int km = (k - 1 + nd) % nd, kp = (k + 1) % nd;
                if (det && local_max)
                    det = rts_cfar_local_max(P, r >= 1, r + 1 < nb, [&](int dk, int dr) { return power(dk < 0 ? km : dk > 0 ? kp : k, r + dr); });
                if (!det) continue;
                if (total < capacity)
                    out[total] = rts_cfar_record(rx, (uint32_t)k, (uint32_t)r, (uint32_t)n, P, noise, thr, r >= 1 ? power(k, r - 1) : 0.0,
                                                 r + 1 < nb ? power(k, r + 1) : 0.0, power(km, r), power(kp, r), n_doppler, q->t0, q->dt, p->pri);
                total++;
            }
    }
    return total;
}
