// rts_doa.h -- direction finding (include/rts_amd.h: RtsEigParams, RtsDoaScanParams): the Hermitian eigensolver's tree (one-sided
// Jacobi, the round-robin pairing, the sort), the angular spectrum's tree, the spectra's weights, the source count, the host
// evaluators and the host-only plans of the launches, shared by the kernels (rts_doa.hip: k_eig, k_doa_scan) and rts_eig_eval /
// rts_doa_scan_eval / rts_doa_weights / rts_source_count.  Fixed trees of IEEE basic operations, sqrt and comparisons, compiled with
// -ffp-contract=off (rts_source_count apart: libm's log, host only, no device twin and no bit contract).  Includes nothing of HIP:
// it compiles with any host compiler and is tested without a GPU (tests/test_doa_host.py, tests/doa/doa_main.cpp).
//
// ---- the eigensolver's tree.  X [n][n] and V [n][n] complex128, row-major (element (i, col) at 2 (i ld + col)).  X = A: the lower
// triangle as read, the diagonal (re, +0.0), the upper triangle X[j][i] = (re, -im) of A[i][j] (i > j); V = I.  Nothing else of A
// is read.  A sweep: first m2 = the largest column norm squared, norm2(col) = the sum of (re re + im im) of X[i][col] over
// ascending i, the i = 0 term the start value, the maximum taken by `if (v > m2) m2 = v` over ascending col from norm2(0); floor2 =
// RTS_EIG_EPS2 m2.  Then the rounds r = 0 .. M - 2 of rts_eig_pair_of (M = n rounded up to even), and of each round the slots
// k = 0 .. M / 2 - 1; the pairs of a round are disjoint, so their order inside the round changes nothing.  A pair (p < q; q >= n is
// the bye of an odd n):
//     alpha = norm2(p);  beta = norm2(q);  gamma = the sum of conj(x_ip) x_iq = (pr qr + pi qi, pr qi - pi qr) (rts_beam_add) over
//     ascending i, the i = 0 term the start value;  g2 = gr gr + gi gi.
//     converged, no rotation:  g2 <= RTS_EIG_TOL2 (alpha beta), or alpha <= floor2, or beta <= floor2  (a column that holds only
//     the rounding noise of a null space: it passes the relative test for ever and means nothing).
//     g = sqrt(g2);  e = (gr / g, gi / g);  zeta = (beta - alpha) / (2.0 g);  az = zeta < 0 ? -zeta : zeta;
//     d = az + sqrt(1.0 + zeta zeta);  t = zeta < 0 ? -1.0 / d : 1.0 / d;  c = 1.0 / sqrt(1.0 + t t);  s = c t;
//     sr = s e.re;  si = s e.im;  and of X and then of V, every row i ascending, a = M[i][p], b = M[i][q]:
//         a' = (c ar - (sr br + si bi),  c ai - (sr bi - si br))        a' = c a - s conj(e) b
//         b' = ((sr ar - si ai) + c br,  (sr ai + si ar) + c bi)        b' = s e a + c b
// The solver: sweeps = 0; run a sweep; none of its pairs rotated: converged (status 0); otherwise sweeps = sweeps + 1 and, when
// sweeps == RTS_EIG_MAX_SWEEPS, status 1; else the next sweep.  `sweeps` counts the sweeps that rotated: the identity takes 0.
// RTS_EIG_TOL2 = 2^-100 (tol = 2^-50), RTS_EIG_EPS2 = 2^-104 (eps = 2^-52).  RTS_EIG_MAX_SWEEPS = 30: the evaluator needs at most
// 13 on the matrices of tests/test_doa_host.py (full-rank, barely full-rank and rank-deficient sample covariances up to 64 x 64).
// The eigenvalues: lambda(col) = the sum of (vr xr + vi xi), v = V[i][col], x = X[i][col], over ascending i, the i = 0 term the
// start value.  The order: rank(col) = the number of columns j with lambda(j) > lambda(col), or lambda(j) == lambda(col) and
// j < col: descending, ties by ascending column, a fixed permutation.  values[rank] = lambda(col), vectors[rank][i] = V[i][col]:
// ROW k = eigenvector k, no phase normalisation.  Before anything: an entry of the lower triangle (of the diagonal the real part)
// outside [-DBL_MAX, DBL_MAX] (comparisons: NaN fails them) is status 2.
// X = A V holds throughout and the columns of X end orthogonal: V diagonalises A^2.  For a positive semidefinite A (a covariance)
// these are A's eigenvectors; eigenvalues of equal magnitude and opposite sign would share a subspace of A^2.
//
// ---- the scan's tree.  Vectors v_k [n], k = 0 .. m - 1, weights g_k, direction a [n]:
//     y_k = the sum of conj(v_k[rx]) a[rx] (rts_beam_add: w = v_k[rx], z = a[rx]) over ascending rx, rx = 0 the start value;
//     p_k = rts_beam_power(y_k);  q = g_0 p_0, then q = q + g_k p_k for ascending k;  out = q, or with RTS_DOA_INVERSE 1.0 / q (the
//     IEEE quotient, no clamp: q = 0 gives +inf).
#pragma once
#include <math.h>
#include <stdint.h>
#include <stddef.h>
#include "../../include/rts_amd.h"
#include "rts_beam.h"

#define RTS_EIG_TOL2 7.8886090522101181e-31      // 2^-100
#define RTS_EIG_EPS2 4.9303806576313238e-32      // 2^-104
#define RTS_EIG_DBL_MAX 1.7976931348623157e308

RTS_HD bool rts_eig_finite(double x) { return x >= -RTS_EIG_DBL_MAX && x <= RTS_EIG_DBL_MAX; }

// ---- the pairing, a function of n alone (the circle method): M = n rounded up to even, rounds 0 .. M - 2, slots 0 .. M / 2 - 1.
// Slot 0 pairs M - 1 with r; slot k > 0 pairs (r + k) % (M - 1) with (r + M - 1 - k) % (M - 1).  p < q; q >= n: the bye
RTS_HD uint32_t rts_eig_even(uint32_t n) { return n + (n & 1u); }
RTS_HD void rts_eig_pair_of(uint32_t n, uint32_t r, uint32_t k, uint32_t* p, uint32_t* q)
{
    const uint32_t M = rts_eig_even(n);
    const uint32_t a = k == 0u ? M - 1u : (r + k) % (M - 1u), b = k == 0u ? r : (r + M - 1u - k) % (M - 1u);
    *p = a < b ? a : b; *q = a < b ? b : a;
}

RTS_HD double rts_eig_norm2(const double* X, uint32_t ld, uint32_t n, uint32_t col)
{
    double s = rts_beam_power(X[2 * (size_t)col], X[2 * (size_t)col + 1]);
    for (uint32_t i = 1; i < n; i++) s += rts_beam_power(X[2 * ((size_t)i * ld + col)], X[2 * ((size_t)i * ld + col) + 1]);
    return s;
}

// A pair walks its two columns twice, rows in batches of RTS_EIG_BATCH: the batch's elements are read first and used afterwards, so
// that on the device the reads of a batch are in flight together (one wave, LDS latency: rts_doa.hip).  The batches change which
// reads are in flight together, never a sum's order; past the last row a batch reads the last row again and uses nothing of it.
#define RTS_EIG_BATCH 8u
#if defined(__clang__)
#define RTS_EIG_UNROLL _Pragma("unroll")
#else
#define RTS_EIG_UNROLL
#endif
// alpha, beta and gamma of a pair in one walk: three independent sums over ascending i, each from its i = 0 term
RTS_HD void rts_eig_sums(const double* X, uint32_t ld, uint32_t n, uint32_t p, uint32_t q, double* alpha, double* beta, double* gr, double* gi)
{
    double a = 0.0, b = 0.0, yr = 0.0, yi = 0.0;
    for (uint32_t i0 = 0; i0 < n; i0 += RTS_EIG_BATCH) {
        double pr[RTS_EIG_BATCH], pi[RTS_EIG_BATCH], qr[RTS_EIG_BATCH], qi[RTS_EIG_BATCH];
        RTS_EIG_UNROLL
        for (uint32_t k = 0; k < RTS_EIG_BATCH; k++) {
            const size_t row = (size_t)(i0 + k < n ? i0 + k : n - 1u) * ld;
            pr[k] = X[2 * (row + p)]; pi[k] = X[2 * (row + p) + 1]; qr[k] = X[2 * (row + q)]; qi[k] = X[2 * (row + q) + 1];
        }
        RTS_EIG_UNROLL
        for (uint32_t k = 0; k < RTS_EIG_BATCH; k++) {
            if (i0 + k >= n) continue;
            const double ta = rts_beam_power(pr[k], pi[k]), tb = rts_beam_power(qr[k], qi[k]);
            if (i0 + k == 0u) { a = ta; b = tb; } else { a += ta; b += tb; }
            rts_beam_add(i0 + k == 0u, pr[k], pi[k], qr[k], qi[k], &yr, &yi);
        }
    }
    *alpha = a; *beta = b; *gr = yr; *gi = yi;
}

// the rows first, first + step, ... of X and of V under the pair's rotation.  A row's new elements depend on that row alone: the
// evaluator takes every row (0, 1), the kernel deals a pair's rows to RTS_EIG_LANES lanes -- the same bits
RTS_HD void rts_eig_rotate(double* X, double* V, uint32_t ld, uint32_t n, uint32_t p, uint32_t q, double c, double sr, double si, uint32_t first, uint32_t step)
{
    for (uint32_t i0 = first; i0 < n; i0 += RTS_EIG_BATCH * step) {
        double v[2][RTS_EIG_BATCH][4];                       // of X and of V: (ar, ai, br, bi) of the batch's rows
        RTS_EIG_UNROLL
        for (uint32_t k = 0; k < RTS_EIG_BATCH; k++) {
            const size_t row = (size_t)(i0 + k * step < n ? i0 + k * step : first) * ld;
            v[0][k][0] = X[2 * (row + p)]; v[0][k][1] = X[2 * (row + p) + 1]; v[0][k][2] = X[2 * (row + q)]; v[0][k][3] = X[2 * (row + q) + 1];
            v[1][k][0] = V[2 * (row + p)]; v[1][k][1] = V[2 * (row + p) + 1]; v[1][k][2] = V[2 * (row + q)]; v[1][k][3] = V[2 * (row + q) + 1];
        }
        RTS_EIG_UNROLL
        for (uint32_t k = 0; k < RTS_EIG_BATCH; k++) {
            if (i0 + k * step >= n) continue;
            const size_t row = (size_t)(i0 + k * step) * ld;
            RTS_EIG_UNROLL
            for (uint32_t w = 0; w < 2u; w++) {
                double* M = w ? V : X;
                const double ar = v[w][k][0], ai = v[w][k][1], br = v[w][k][2], bi = v[w][k][3];
                M[2 * (row + p)] = c * ar - (sr * br + si * bi); M[2 * (row + p) + 1] = c * ai - (sr * bi - si * br);
                M[2 * (row + q)] = (sr * ar - si * ai) + c * br; M[2 * (row + q) + 1] = (sr * ai + si * ar) + c * bi;
            }
        }
    }
}

// one pair of a round (p < q < n), first half: its sums and, when it is to rotate (true), the rotation (c, s e.re, s e.im)
RTS_HD bool rts_eig_decide(const double* X, uint32_t ld, uint32_t n, uint32_t p, uint32_t q, double floor2, double* c_out, double* sr, double* si)
{
    double alpha, beta, gr, gi;
    rts_eig_sums(X, ld, n, p, q, &alpha, &beta, &gr, &gi);
    const double g2 = gr * gr + gi * gi;
    if (g2 <= RTS_EIG_TOL2 * (alpha * beta) || alpha <= floor2 || beta <= floor2) return false;
    const double g = sqrt(g2), er = gr / g, ei = gi / g;
    const double zeta = (beta - alpha) / (2.0 * g), az = zeta < 0.0 ? -zeta : zeta;
    const double d = az + sqrt(1.0 + zeta * zeta), t = zeta < 0.0 ? -1.0 / d : 1.0 / d;
    const double c = 1.0 / sqrt(1.0 + t * t), s = c * t;
    *c_out = c; *sr = s * er; *si = s * ei;
    return true;
}

RTS_HD double rts_eig_value(const double* X, const double* V, uint32_t ld, uint32_t n, uint32_t col)
{
    double s = V[2 * (size_t)col] * X[2 * (size_t)col] + V[2 * (size_t)col + 1] * X[2 * (size_t)col + 1];
    for (uint32_t i = 1; i < n; i++) {
        const size_t e = 2 * ((size_t)i * ld + col);
        s += V[e] * X[e] + V[e + 1] * X[e + 1];
    }
    return s;
}
RTS_HD uint32_t rts_eig_rank(const double* lambda, uint32_t n, uint32_t col)
{
    uint32_t rank = 0u;
    for (uint32_t j = 0; j < n; j++) if (lambda[j] > lambda[col] || (lambda[j] == lambda[col] && j < col)) rank++;
    return rank;
}

// ---- the plan of the solve (host only).  k_eig: ONE workgroup of RTS_EIG_THREADS; X and V [n][n] in LDS (2 x 16 n n bytes: 128 KiB
// at 64).  RTS_EIG_LANES neighbouring threads own slot t / RTS_EIG_LANES of every round: each of them forms the pair's sums, whole
// (a pair's sums are not split across lanes, so the tree is the evaluator's whatever the launch), and they share the rotation's
// rows.  Thread t < n owns column t of the norms, the eigenvalues and the sort.
#define RTS_EIG_THREADS 256u
#define RTS_EIG_LANES 8u
struct RtsEigPlan { uint32_t rounds, slots; size_t lds, value_doubles, vector_doubles; bool supported; };
static inline RtsEigPlan rts_eig_plan(uint32_t n)
{
    RtsEigPlan p;
    p.supported = n >= 1u && n <= RTS_BEAM_MAX_RX && n <= RTS_EIG_THREADS && rts_eig_even(n) / 2u * RTS_EIG_LANES <= RTS_EIG_THREADS;
    p.rounds = p.supported ? rts_eig_even(n) - 1u : 0u;
    p.slots = p.supported ? rts_eig_even(n) / 2u : 0u;
    p.lds = 2u * 16u * (size_t)n * n;
    p.value_doubles = n; p.vector_doubles = 2u * (size_t)n * n;
    return p;
}

// ---- the solve on the host (validated by the caller): cov [n][n] interleaved; X, V: 2 n n doubles of work each; lambda: n.
// Returns the status; values [n] and vectors [n][n] are written only with status 0
static inline uint32_t rts_eig_eval_host(const double* cov, uint32_t n, double* X, double* V, double* lambda, double* values, double* vectors, uint32_t* sweeps_out)
{
    for (uint32_t i = 0; i < n; i++) for (uint32_t j = 0; j <= i; j++) {
        const double re = cov[2 * ((size_t)i * n + j)];
        if (!rts_eig_finite(re)) return 2u;
        if (i == j) { X[2 * ((size_t)i * n + i)] = re; X[2 * ((size_t)i * n + i) + 1] = 0.0; continue; }
        const double im = cov[2 * ((size_t)i * n + j) + 1];
        if (!rts_eig_finite(im)) return 2u;
        X[2 * ((size_t)i * n + j)] = re; X[2 * ((size_t)i * n + j) + 1] = im;
        X[2 * ((size_t)j * n + i)] = re; X[2 * ((size_t)j * n + i) + 1] = -im;
    }
    for (size_t e = 0; e < (size_t)n * n; e++) { V[2 * e] = e / n == e % n ? 1.0 : 0.0; V[2 * e + 1] = 0.0; }
    const RtsEigPlan plan = rts_eig_plan(n);
    uint32_t sweeps = 0u, status = 0u;
    for (;;) {
        double m2 = rts_eig_norm2(X, n, n, 0u);
        for (uint32_t col = 1; col < n; col++) { const double v = rts_eig_norm2(X, n, n, col); if (v > m2) m2 = v; }
        const double floor2 = RTS_EIG_EPS2 * m2;
        bool rotated = false;
        for (uint32_t r = 0; r < plan.rounds; r++) for (uint32_t k = 0; k < plan.slots; k++) {
            uint32_t p, q; rts_eig_pair_of(n, r, k, &p, &q);
            double c, sr, si;
            if (q < n && rts_eig_decide(X, n, n, p, q, floor2, &c, &sr, &si)) { rts_eig_rotate(X, V, n, n, p, q, c, sr, si, 0u, 1u); rotated = true; }
        }
        if (!rotated) break;
        sweeps++;
        if (sweeps == RTS_EIG_MAX_SWEEPS) { status = 1u; break; }
    }
    if (sweeps_out) *sweeps_out = sweeps;
    if (status) return status;
    for (uint32_t col = 0; col < n; col++) lambda[col] = rts_eig_value(X, V, n, n, col);
    for (uint32_t col = 0; col < n; col++) {
        const uint32_t k = rts_eig_rank(lambda, n, col);
        values[k] = lambda[col];
        for (uint32_t i = 0; i < n; i++) { vectors[2 * ((size_t)k * n + i)] = V[2 * ((size_t)i * n + col)]; vectors[2 * ((size_t)k * n + i) + 1] = V[2 * ((size_t)i * n + col) + 1]; }
    }
    return 0u;
}

// ---- the plan of the scan's launch (host only), from the shape alone.  k_doa_scan: one thread per direction, consecutive lanes on
// consecutive directions; the steering table is element-major [n][n_dirs], so every global access of a wave is 64 consecutive
// 16-byte elements.  A workgroup of RTS_DOA_THREADS stages the m vectors [m][n] and behind them g [m] in its LDS (at most 64 KiB +
// 512 B).  A thread keeps RTS_DOA_RX_TILE elements of its direction in registers and the running y of RTS_DOA_VEC_TILE vectors;
// with more elements than one tile it walks the element tiles in ascending order per vector tile (read again from the caches).
// The tiles change which sums are in flight together, never the order of a sum.
#define RTS_DOA_THREADS 256u
#define RTS_DOA_RX_TILE 8u
#define RTS_DOA_VEC_TILE 16u
#define RTS_DOA_MAX_GRID_X 2147483647u
struct RtsDoaScanPlan { uint32_t groups, rx_tiles, vec_tiles; size_t lds, out_doubles; bool supported; };
static inline RtsDoaScanPlan rts_doa_scan_plan(uint32_t n, uint32_t m, uint64_t n_dirs)
{
    RtsDoaScanPlan p;
    p.rx_tiles = (n + RTS_DOA_RX_TILE - 1u) / RTS_DOA_RX_TILE;
    p.vec_tiles = (m + RTS_DOA_VEC_TILE - 1u) / RTS_DOA_VEC_TILE;
    p.lds = 16u * (size_t)m * n + 8u * (size_t)m;
    const uint64_t groups = n_dirs / RTS_DOA_THREADS + (n_dirs % RTS_DOA_THREADS ? 1u : 0u);       // (no n_dirs + 255: it wraps at 2^64)
    p.supported = n >= 1u && n <= RTS_BEAM_MAX_RX && m >= 1u && m <= RTS_BEAM_MAX_RX && groups >= 1u && groups <= RTS_DOA_MAX_GRID_X;
    p.groups = p.supported ? (uint32_t)groups : 0u;
    p.out_doubles = p.supported ? (size_t)n_dirs : 0u;
    return p;
}

// one direction: v [m][n] interleaved, a: the direction's element rx at a[2 rx stride], a[2 rx stride + 1]
RTS_HD double rts_doa_direction(const double* v, const double* g, uint32_t n, uint32_t m, const double* a, size_t stride, uint32_t flags)
{
    double q = 0.0;
    for (uint32_t k = 0; k < m; k++) {
        double yr = 0.0, yi = 0.0;
        for (uint32_t rx = 0; rx < n; rx++) rts_beam_add(rx == 0u, v[2 * ((size_t)k * n + rx)], v[2 * ((size_t)k * n + rx) + 1], a[2 * rx * stride], a[2 * rx * stride + 1], &yr, &yi);
        const double gp = g[k] * rts_beam_power(yr, yi);
        if (k == 0u) q = gp; else q += gp;
    }
    return (flags & RTS_DOA_INVERSE) ? 1.0 / q : q;
}
// the scan on the host (validated by the caller): steering [n][n_dirs] interleaved -> out [n_dirs]
static inline void rts_doa_scan_eval_host(const double* v, const double* g, uint32_t n, uint32_t m, const double* steering, uint64_t n_dirs, uint32_t flags, double* out)
{
    for (uint64_t d = 0; d < n_dirs; d++) out[d] = rts_doa_direction(v, g, n, m, steering + 2 * d, (size_t)n_dirs, flags);
}

// ---- the spectra as (first vector, m, g[m], flags) of the scan, from the eigenvalues in the solver's order (host only).
// Returns 0, or the refusal: 1 unknown method, 2 loading negative or not finite, 3 a non-finite eigenvalue, 4 MUSIC with
// n_sources >= n, 5 Capon with a lambda_k + loading not > 0; *bad: the eigenvalue's index (3, 5)
static inline int rts_doa_weights_host(uint32_t method, const double* values, uint32_t n, uint32_t n_sources, double loading, uint32_t* first, uint32_t* m, double* g,
                                       uint32_t* flags, uint32_t* bad)
{
    if (method != RTS_DOA_BARTLETT && method != RTS_DOA_CAPON && method != RTS_DOA_MUSIC) return 1;
    if (!(loading >= 0.0) || !rts_eig_finite(loading)) return 2;
    for (uint32_t k = 0; k < n; k++) if (!rts_eig_finite(values[k])) { *bad = k; return 3; }
    if (method == RTS_DOA_MUSIC) {
        if (n_sources >= n) return 4;
        *first = n_sources; *m = n - n_sources; *flags = RTS_DOA_INVERSE;
        for (uint32_t k = 0; k < *m; k++) g[k] = 1.0;
        return 0;
    }
    if (method == RTS_DOA_CAPON) for (uint32_t k = 0; k < n; k++) if (!(values[k] + loading > 0.0)) { *bad = k; return 5; }
    *first = 0u; *m = n; *flags = method == RTS_DOA_CAPON ? RTS_DOA_INVERSE : 0u;
    for (uint32_t k = 0; k < n; k++) g[k] = method == RTS_DOA_CAPON ? 1.0 / (values[k] + loading) : values[k];
    return 0;
}

// ---- the number of sources (host only; Wax and Kailath's criteria) from the eigenvalues in descending order and the snapshot
// count K.  With the n - k smallest eigenvalues, L(k) = K (n - k) (log(their arithmetic mean) - the mean of their logs):
//     AIC(k) = 2 L(k) + 2 k (2 n - k);   MDL(k) = L(k) + 0.5 k (2 n - k) log K;   k = 0 .. n - 1, the first k of the smallest value.
// Every eigenvalue enters a logarithm: the caller refuses values not > 0
static inline uint32_t rts_source_count_host(const double* values, uint32_t n, uint64_t K, uint32_t criterion)
{
    uint32_t best = 0u; double best_v = 0.0, sum = 0.0, sum_log = 0.0;
    double crit[RTS_BEAM_MAX_RX];
    for (uint32_t k = n; k-- > 0u;) {                    // the n - k smallest: values[k .. n - 1], summed from the smallest up
        sum += values[k]; sum_log += log(values[k]);
        const double cnt = (double)(n - k), L = (double)K * cnt * (log(sum / cnt) - sum_log / cnt), pen = (double)k * (double)(2u * n - k);
        crit[k] = criterion == RTS_DOA_AIC ? 2.0 * L + 2.0 * pen : L + 0.5 * pen * log((double)K);
    }
    for (uint32_t k = 0; k < n; k++) if (k == 0u || crit[k] < best_v) { best = k; best_v = crit[k]; }
    return best;
}
