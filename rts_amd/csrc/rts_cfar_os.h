// rts_cfar_os.h -- the arithmetic of ordered-statistic CFAR (include/rts_amd.h: RtsCfarOsParams), shared by the kernel
// (rts_detect.hip: k_cfar_os), the launch (rts_cube_detect_os) and the host evaluator (rts_cfar_os_eval): the size of the window, the
// training count of a cell from its two range-edge distances, the rank rule, the threshold factor of a false-alarm rate, the
// order-preserving 64-bit key of a power, a plain selection, and the evaluator itself.  An order statistic has no summation order:
// kernel and evaluator agree on the noise estimate bit for bit.  Includes nothing of HIP: it compiles with any host compiler and is
// tested without a GPU (tests/test_cfar_os_host.py, tests/cfar_os/cfar_os_main.cpp).
#pragma once
#include <math.h>
#include <stdint.h>
#include <stddef.h>
#include <string.h>
#include "../../include/rts_amd.h"

#ifndef RTS_HD
#define RTS_HD static inline          // (a host compiler; the library's units have rts_device_math.h's __host__ __device__ form)
#endif

// training cells of a FULL window: the (2 (Gr + Tr) + 1) x (2 (Gd + Td) + 1) rectangle minus the guard rectangle
RTS_HD uint32_t rts_cfar_os_n0(uint32_t gr, uint32_t gd, uint32_t tr, uint32_t td)
{
    return (2u * (gr + tr) + 1u) * (2u * (gd + td) + 1u) - (2u * gr + 1u) * (2u * gd + 1u);
}

// training cells of a cell with edge_l bins to its left and edge_r to its right inside [0, n_bins) (Doppler wraps, range is truncated):
// outer columns (|dr| > Gr) hold 2 (Gd + Td) + 1 cells, inner columns and the cell's own hold the 2 Td rows outside the guard
RTS_HD int rts_cfar_os_count(int gr, int gd, int tr, int td, int edge_l, int edge_r)
{
    const int Or = gr + tr, Od = gd + td;
    const int cl = edge_l < Or ? edge_l : Or, cr = edge_r < Or ? edge_r : Or;      // columns that exist on each side
    const int nlo = cl > gr ? cl - gr : 0, nli = cl < gr ? cl : gr;
    const int nro = cr > gr ? cr - gr : 0, nri = cr < gr ? cr : gr;
    return (nlo + nro) * (2 * Od + 1) + (nli + nri + 1) * 2 * td;
}

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

// parabola through ln P of three samples: the vertex offset in [-0.5, 0.5], 0 when it is not a peak of positive powers
RTS_HD double rts_cfar_os_delta(double pm, double p0, double pp)
{
    if (!(pm > 0.0) || !(p0 > 0.0) || !(pp > 0.0)) return 0.0;
    const double lm = log(pm), l0 = log(p0), lp = log(pp);
    const double den = lm - 2.0 * l0 + lp;
    if (!(den < 0.0)) return 0.0;
    const double d = 0.5 * (lm - lp) / den;
    return d > 0.5 ? 0.5 : d < -0.5 ? -0.5 : d;
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
    const uint32_t N0 = rts_cfar_os_n0(gr, gd, tr, td), Or = gr + tr;
    uint32_t solved = 0;
    for (uint32_t r = 0; r < n_bins; r++) {
        if (r > Or + 1u && n_bins - 1u - r > Or + 1u) { r = n_bins - 1u - (Or + 1u) - 1u; continue; }      // (the interior: one count)
        const uint32_t N = (uint32_t)rts_cfar_os_count((int)gr, (int)gd, (int)tr, (int)td, (int)r, (int)(n_bins - 1u - r));
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
    const int gr = (int)p->guard_range, gd = (int)p->guard_doppler, tr = (int)p->train_range, td = (int)p->train_doppler, Or = gr + tr, Od = gd + td;
    const int nd = (int)n_doppler, nb = (int)q->n_bins;
    const uint32_t N0 = rts_cfar_os_n0(p->guard_range, p->guard_doppler, p->train_range, p->train_doppler);
    const bool local_max = (p->flags & RTS_CFAR_LOCAL_MAX) != 0;
    uint32_t total = 0;
    for (uint32_t rx = 0; rx < q->n_rx; rx++) {
        const double* m = map + 2 * (size_t)rx * n_doppler * q->n_bins;
        #define RTS_OS_P(k_, r_) (m[2 * ((size_t)(k_) * (size_t)nb + (size_t)(r_))] * m[2 * ((size_t)(k_) * (size_t)nb + (size_t)(r_))] + \
                                  m[2 * ((size_t)(k_) * (size_t)nb + (size_t)(r_)) + 1] * m[2 * ((size_t)(k_) * (size_t)nb + (size_t)(r_)) + 1])
        for (int k = 0; k < nd; k++)
            for (int r = 0; r < nb; r++) {
                size_t n = 0;
                for (int dk = -Od; dk <= Od; dk++) {
                    int kk = (k + dk) % nd; if (kk < 0) kk += nd;
                    for (int dr = -Or; dr <= Or; dr++) {
                        if ((dk >= -gd && dk <= gd && dr >= -gr && dr <= gr) || r + dr < 0 || r + dr >= nb) continue;
                        keys[n++] = rts_cfar_os_key(RTS_OS_P(kk, r + dr));
                    }
                }
                const uint32_t kth = rts_cfar_os_rank(p->rank, (uint32_t)n, N0);
                const double noise = rts_cfar_os_unkey(rts_cfar_os_select(keys, n, kth));
                const double alpha = alpha_tab ? alpha_tab[n] : p->alpha;
                const double thr = alpha * noise;
                const double P = RTS_OS_P(k, r);
                bool det = P > thr;
                const int km = (k - 1 + nd) % nd, kp = (k + 1) % nd;
                if (det && local_max) {
                    for (int dk = -1; dk <= 1 && det; dk++)
                        for (int dr = -1; dr <= 1; dr++) {
                            if ((dk == 0 && dr == 0) || r + dr < 0 || r + dr >= nb) continue;
                            const double v = RTS_OS_P(dk < 0 ? km : dk > 0 ? kp : k, r + dr);
                            if (dk < 0 || (dk == 0 && dr < 0)) det = det && P > v; else det = det && P >= v;
                        }
                }
                if (!det) continue;
                if (total < capacity) {
                    const double dr_ = rts_cfar_os_delta(r >= 1 ? RTS_OS_P(k, r - 1) : 0.0, P, r + 1 < nb ? RTS_OS_P(k, r + 1) : 0.0);
                    const double dd_ = rts_cfar_os_delta(RTS_OS_P(km, r), P, RTS_OS_P(kp, r));
                    double w = (double)k + dd_;
                    const double half = 0.5 * (double)nd;
                    if (w >= half) w -= (double)nd; else if (w < -half) w += (double)nd;
                    RtsDetection d;
                    d.rx = rx; d.doppler_bin = (uint32_t)k; d.range_bin = (uint32_t)r; d.n_train = (uint32_t)n;
                    d.power = P; d.noise = noise; d.threshold = thr; d.range_offset = dr_; d.doppler_offset = dd_;
                    d.delay = q->t0 + ((double)r + dr_) * q->dt;
                    d.doppler = p->pri > 0.0 ? w / ((double)nd * p->pri) : 0.0;
                    out[total] = d;
                }
                total++;
            }
        #undef RTS_OS_P
    }
    return total;
}
