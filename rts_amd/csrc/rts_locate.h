// rts_locate.h -- the rules of multistatic localisation (include/rts_amd.h: RtsLocateParams, RtsTarget), each written once and called
// by the kernels (rts_locate.hip), the entry points (rts_cube_detect_api.hip) and the host evaluator (rts_locate_eval): the per-call
// constants, the screen, the closed form of a triple (min-norm solution, null vector, the two roots and their order), the completion,
// the Gauss-Newton refinement, velocity and cost, the order of the resolution, the validation, and the evaluator itself -- the serial
// pass over the triples and the serial greedy resolution (the kernels reach the same set by counts, a scan and rounds).  Every
// expression is written in the operand order of the header text and the units are built without contraction, so kernel and evaluator
// agree bit for bit.  Includes nothing of HIP: it compiles with any host compiler and is tested without a GPU
// (tests/test_locate_host.py, tests/locate/locate_main.cpp).
#pragma once
#include <math.h>
#include <stdint.h>
#include <stddef.h>
#include <algorithm>
#include <vector>
#include "../../include/rts_amd.h"
#include "rts_cfar.h"             // RTS_HD
#include "rts_cube_args.h"        // rts_device_list_rule

#define RTS_LOCATE_NONE 0xffffffffu

RTS_HD bool rts_locate_finite(double x) { return x - x == 0.0; }
RTS_HD double rts_locate_dot(const double* a, const double* b) { return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]; }
RTS_HD double rts_locate_norm(const double* a) { return sqrt(rts_locate_dot(a, a)); }
RTS_HD void rts_locate_cross(const double* a, const double* b, double* o)
{
    o[0] = a[1] * b[2] - a[2] * b[1]; o[1] = a[2] * b[0] - a[0] * b[2]; o[2] = a[0] * b[1] - a[1] * b[0];
}

// The constants of a call: the positions, d_a, |d_a|, |d_a|^2, D D^T, the anchor baselines (0-1, 0-2, 1-2), the cross products of D's
// columns and det D, and the scalars derived from the parameter record.  Doubles first: the record goes to the device as it stands.
struct RtsLocateGeo {
    double tx[3], s[RTS_LOCATE_MAX_RX][3];
    double d[3][3], dn[3], dd[3], G[3][3], base[3];
    double X12[3], X02[3], X01[3], detD;
    double sigma_r, lambda, sigma_f, gate, assoc, lo[3], hi[3];
    uint32_t n_rx, anchors[3], min_rx, n_iters, use_doppler, reserved;
};

// (host only: it reads the caller's rx_positions)
static inline RtsLocateGeo rts_locate_geo(const RtsLocateParams& p)
{
    RtsLocateGeo g;
    for (uint32_t m = 0; m < RTS_LOCATE_MAX_RX; m++) for (int c = 0; c < 3; c++) g.s[m][c] = m < p.n_rx ? p.rx_positions[3u * m + (uint32_t)c] : 0.0;
    for (int c = 0; c < 3; c++) { g.tx[c] = p.tx[c]; g.lo[c] = p.box_lo[c]; g.hi[c] = p.box_hi[c]; }
    for (int a = 0; a < 3; a++) {
        g.anchors[a] = p.anchors[a];
        for (int c = 0; c < 3; c++) g.d[a][c] = g.s[p.anchors[a]][c] - p.tx[c];
        g.dd[a] = rts_locate_dot(g.d[a], g.d[a]); g.dn[a] = sqrt(g.dd[a]);
    }
    for (int a = 0; a < 3; a++) for (int b = 0; b < 3; b++) g.G[a][b] = rts_locate_dot(g.d[a], g.d[b]);
    const int pair[3][2] = {{0, 1}, {0, 2}, {1, 2}};
    for (int q = 0; q < 3; q++) {
        double e[3];
        for (int c = 0; c < 3; c++) e[c] = g.s[p.anchors[pair[q][0]]][c] - g.s[p.anchors[pair[q][1]]][c];
        g.base[q] = rts_locate_norm(e);
    }
    double col[3][3];                                                    // the columns of D
    for (int c = 0; c < 3; c++) for (int a = 0; a < 3; a++) col[c][a] = g.d[a][c];
    rts_locate_cross(col[1], col[2], g.X12); rts_locate_cross(col[0], col[2], g.X02); rts_locate_cross(col[0], col[1], g.X01);
    g.detD = rts_locate_dot(col[2], g.X01);
    g.sigma_r = p.cspeed * p.sigma_delay; g.use_doppler = p.carrier > 0.0 ? 1u : 0u; g.lambda = g.use_doppler ? p.cspeed / p.carrier : 0.0;
    g.sigma_f = p.sigma_doppler; g.gate = p.gate; g.assoc = p.cspeed * p.assoc_delay;
    g.n_rx = p.n_rx; g.min_rx = p.min_receivers; g.n_iters = p.n_iters; g.reserved = 0u;
    return g;
}

// ---- the screen (2).  Written so that a NaN range sum -- a record that takes no part -- is screened out as well
RTS_HD bool rts_locate_screen_one(const RtsLocateGeo& g, int a, double R) { return R >= g.dn[a]; }
RTS_HD bool rts_locate_screen_pair(const RtsLocateGeo& g, int q, double Ra, double Rb) { return fabs(Ra - Rb) <= g.base[q]; }

// ---- Cholesky of a symmetric 3 x 3 given by its lower triangle A = {a00, a10, a11, a20, a21, a22}: false at a pivot that is not
// positive and finite; L in the same layout.  Then A^-1 b by the two triangular solves
RTS_HD bool rts_locate_pivot_ok(double p) { return p > 0.0 && rts_locate_finite(p); }
RTS_HD bool rts_locate_chol(const double* A, double* L)
{
    if (!rts_locate_pivot_ok(A[0])) return false;
    L[0] = sqrt(A[0]); L[1] = A[1] / L[0]; L[3] = A[3] / L[0];
    const double p1 = A[2] - L[1] * L[1];
    if (!rts_locate_pivot_ok(p1)) return false;
    L[2] = sqrt(p1); L[4] = (A[4] - L[3] * L[1]) / L[2];
    const double p2 = (A[5] - L[3] * L[3]) - L[4] * L[4];
    if (!rts_locate_pivot_ok(p2)) return false;
    L[5] = sqrt(p2);
    return true;
}
RTS_HD void rts_locate_chol_solve(const double* L, const double* b, double* y)
{
    const double z0 = b[0] / L[0], z1 = (b[1] - L[1] * z0) / L[2], z2 = ((b[2] - L[3] * z0) - L[4] * z1) / L[5];
    y[2] = z2 / L[5]; y[1] = (z1 - L[4] * y[2]) / L[2]; y[0] = ((z0 - L[1] * y[1]) - L[3] * y[2]) / L[0];
}

RTS_HD bool rts_locate_in_box(const RtsLocateGeo& g, const double* x)
{
    for (int c = 0; c < 3; c++) if (!rts_locate_finite(x[c]) || !(x[c] >= g.lo[c] && x[c] <= g.hi[c])) return false;
    return true;
}

// ---- the closed form of a screened triple (2): the positions of root 0 and root 1; bit q of the result: root q is kept
RTS_HD uint32_t rts_locate_solve(const RtsLocateGeo& g, const double* R, double x[2][3])
{
    double A[6], L[6], c[3], y[3], u0[3], n[3];
    A[0] = g.G[0][0] + R[0] * R[0]; A[1] = g.G[1][0] + R[1] * R[0]; A[2] = g.G[1][1] + R[1] * R[1];
    A[3] = g.G[2][0] + R[2] * R[0]; A[4] = g.G[2][1] + R[2] * R[1]; A[5] = g.G[2][2] + R[2] * R[2];
    if (!rts_locate_chol(A, L)) return 0u;
    for (int a = 0; a < 3; a++) c[a] = (g.dd[a] - R[a] * R[a]) / 2.0;
    rts_locate_chol_solve(L, c, y);
    for (int k = 0; k < 3; k++) u0[k] = (y[0] * g.d[0][k] + y[1] * g.d[1][k]) + y[2] * g.d[2][k];
    const double r0 = -((R[0] * y[0] + R[1] * y[1]) + R[2] * y[2]);
    n[0] = -rts_locate_dot(R, g.X12); n[1] = rts_locate_dot(R, g.X02); n[2] = -rts_locate_dot(R, g.X01);
    const double nr = -g.detD;
    const double qa = rts_locate_dot(n, n) - nr * nr, qb = rts_locate_dot(u0, n) - r0 * nr, qc = rts_locate_dot(u0, u0) - r0 * r0;
    const double disc = qb * qb - qa * qc;
    if (!(disc >= 0.0)) return 0u;
    const double sq = sqrt(disc), t = qb >= 0.0 ? -(qb + sq) : -(qb - sq);
    double l[2] = {t / qa, qc / t}, r[2];
    r[0] = r0 + l[0] * nr; r[1] = r0 + l[1] * nr;
    if (r[1] < r[0] || (r[1] == r[0] && l[1] < l[0])) { const double tl = l[0], tr = r[0]; l[0] = l[1]; r[0] = r[1]; l[1] = tl; r[1] = tr; }
    uint32_t kept = 0u;
    for (int q = 0; q < 2; q++) {
        for (int k = 0; k < 3; k++) x[q][k] = g.tx[k] + (u0[k] + l[q] * n[k]);
        if (!(r[q] > 0.0) || !rts_locate_finite(r[q])) continue;
        if (!(R[0] - r[q] > 0.0) || !(R[1] - r[q] > 0.0) || !(R[2] - r[q] > 0.0)) continue;
        if (rts_locate_in_box(g, x[q])) kept |= 1u << q;
    }
    return kept;
}

// ---- the records as the step sees them: per record its range sum (NaN: it takes no part), Doppler, power and list index, in segment
// order; seg[2 m], seg[2 m + 1]: where receiver m's segment begins and ends
struct RtsLocateList { const double* R; const double* f; const double* pw; const uint32_t* idx; const uint32_t* seg; };

RTS_HD double rts_locate_range_sum(double cspeed, double delay, double doppler, double power)
{
    return rts_locate_finite(delay) && rts_locate_finite(doppler) && rts_locate_finite(power) ? cspeed * delay : NAN;
}
RTS_HD bool rts_locate_is_anchor(const RtsLocateGeo& g, uint32_t m) { return m == g.anchors[0] || m == g.anchors[1] || m == g.anchors[2]; }

// row J_m = u_t + u_m at x and the range sum there
RTS_HD double rts_locate_row(const RtsLocateGeo& g, const double* x, uint32_t m, double* J)
{
    double a[3], b[3];
    for (int k = 0; k < 3; k++) { a[k] = x[k] - g.tx[k]; b[k] = x[k] - g.s[m][k]; }
    const double na = rts_locate_norm(a), nb = rts_locate_norm(b);
    for (int k = 0; k < 3; k++) J[k] = (a[k] / na) + (b[k] / nb);
    return na + nb;
}
// A = J^T J (lower triangle), gr = J^T rho and gf = J^T f at x over the receivers that have a record, in ascending order
RTS_HD void rts_locate_normal(const RtsLocateGeo& g, const RtsLocateList& z, const uint32_t* rec, const double* x, double* A, double* gr, double* gf)
{
    for (int k = 0; k < 6; k++) A[k] = 0.0;
    for (int k = 0; k < 3; k++) { gr[k] = 0.0; gf[k] = 0.0; }
    for (uint32_t m = 0; m < g.n_rx; m++) {
        if (rec[m] == RTS_LOCATE_NONE) continue;
        double J[3];
        const double rho = z.R[rec[m]] - rts_locate_row(g, x, m, J), f = z.f[rec[m]];
        A[0] = A[0] + J[0] * J[0]; A[1] = A[1] + J[1] * J[0]; A[2] = A[2] + J[1] * J[1];
        A[3] = A[3] + J[2] * J[0]; A[4] = A[4] + J[2] * J[1]; A[5] = A[5] + J[2] * J[2];
        for (int k = 0; k < 3; k++) { gr[k] = gr[k] + J[k] * rho; gf[k] = gf[k] + J[k] * f; }
    }
}

// ---- a kept root to a candidate (3, 4, 5): e3 the anchors' records (positions in z), x0 the root.  true: accepted, *out is the record
RTS_HD bool rts_locate_candidate(const RtsLocateGeo& g, const RtsLocateList& z, const uint32_t* e3, const double* x0, uint64_t index, RtsTarget* out)
{
    uint32_t rec[RTS_LOCATE_MAX_RX], K = 3u, flags = 0u;
    for (uint32_t m = 0; m < RTS_LOCATE_MAX_RX; m++) rec[m] = RTS_LOCATE_NONE;
    for (int a = 0; a < 3; a++) rec[g.anchors[a]] = e3[a];
    for (uint32_t m = 0; m < g.n_rx; m++) {
        if (rts_locate_is_anchor(g, m)) continue;
        double J[3];
        const double want = rts_locate_row(g, x0, m, J);
        uint32_t best = RTS_LOCATE_NONE; double bd = 0.0;
        for (uint32_t e = z.seg[2u * m]; e < z.seg[2u * m + 1u]; e++) {
            const double dist = fabs(z.R[e] - want);
            if (!(dist <= g.assoc)) continue;
            if (best == RTS_LOCATE_NONE || dist < bd) { best = e; bd = dist; }
        }
        rec[m] = best;
        if (best != RTS_LOCATE_NONE) K++;
    }
    if (K < g.min_rx) return false;
    double x[3] = {x0[0], x0[1], x0[2]}, A[6], L[6], gr[3], gf[3], y[3];
    for (uint32_t it = 0; it < g.n_iters; it++) {
        rts_locate_normal(g, z, rec, x, A, gr, gf);
        if (!rts_locate_chol(A, L)) { flags |= RTS_TARGET_UNREFINED; break; }
        rts_locate_chol_solve(L, gr, y);
        for (int k = 0; k < 3; k++) x[k] = x[k] + y[k];
    }
    if (!rts_locate_in_box(g, x)) return false;
    double v[3] = {0.0, 0.0, 0.0};
    if (g.use_doppler) {
        rts_locate_normal(g, z, rec, x, A, gr, gf);
        if (rts_locate_chol(A, L)) { rts_locate_chol_solve(L, gf, y); for (int k = 0; k < 3; k++) v[k] = -(g.lambda * y[k]); }
        else flags |= RTS_TARGET_UNREFINED;
    }
    double cost = 0.0, power = 0.0;
    const double vr = g.sigma_r * g.sigma_r, vf = g.sigma_f * g.sigma_f;
    for (uint32_t m = 0; m < g.n_rx; m++) {
        if (rec[m] == RTS_LOCATE_NONE) continue;
        double J[3];
        const double rho = z.R[rec[m]] - rts_locate_row(g, x, m, J);
        cost = cost + (rho * rho) / vr;
        power = power + z.pw[rec[m]];
    }
    if (g.use_doppler) for (uint32_t m = 0; m < g.n_rx; m++) {
        if (rec[m] == RTS_LOCATE_NONE) continue;
        double J[3];
        (void)rts_locate_row(g, x, m, J);
        const double e = z.f[rec[m]] + rts_locate_dot(J, v) / g.lambda;
        cost = cost + (e * e) / vf;
    }
    const uint32_t dof = g.use_doppler ? 2u * K - 6u : K - 3u;
    if (!(cost <= g.gate * (double)(dof > 1u ? dof : 1u))) return false;
    for (int k = 0; k < 3; k++) { out->pos[k] = x[k]; out->vel[k] = v[k]; }
    out->cost = cost + 0.0; out->power_sum = power; out->candidate = index; out->n_receivers = K; out->flags = flags;
    for (uint32_t m = 0; m < RTS_LOCATE_MAX_RX; m++) out->plot[m] = rec[m] == RTS_LOCATE_NONE ? RTS_LOCATE_NONE : z.idx[rec[m]];
    return true;
}

// One (i, j) pair of the anchors' first two segments against the third (P2 range sums at R2): the candidates it accepts, counted
// and -- with out -- written from out[0] while fewer than `room` are written.  i, j, k: positions inside the segments
RTS_HD uint32_t rts_locate_pair(const RtsLocateGeo& g, const RtsLocateList& z, uint32_t i, uint32_t j, const double* R2, uint32_t P1, uint32_t P2, RtsTarget* out, uint32_t room)
{
    const uint32_t e0 = z.seg[2u * g.anchors[0]] + i, e1 = z.seg[2u * g.anchors[1]] + j, first2 = z.seg[2u * g.anchors[2]];
    double R[3] = {z.R[e0], z.R[e1], 0.0};
    if (!rts_locate_screen_one(g, 0, R[0]) || !rts_locate_screen_one(g, 1, R[1]) || !rts_locate_screen_pair(g, 0, R[0], R[1])) return 0u;
    uint32_t n = 0u;
    for (uint32_t k = 0; k < P2; k++) {
        R[2] = R2[k];
        if (!rts_locate_screen_one(g, 2, R[2]) || !rts_locate_screen_pair(g, 1, R[0], R[2]) || !rts_locate_screen_pair(g, 2, R[1], R[2])) continue;
        double x[2][3];
        const uint32_t kept = rts_locate_solve(g, R, x);
        for (uint32_t q = 0; q < 2u; q++) {
            if (!(kept & (1u << q))) continue;
            const uint32_t e3[3] = {e0, e1, first2 + k};
            RtsTarget t;
            if (!rts_locate_candidate(g, z, e3, x[q], (((uint64_t)i * P1 + j) * P2 + k) * 2u + q, &t)) continue;
            if (out && n < room) out[n] = t;
            n++;
        }
    }
    return n;
}
RTS_HD uint32_t rts_locate_anchor_count(uint32_t lo, uint32_t hi) { return hi - lo < RTS_LOCATE_MAX_PER_RX ? hi - lo : RTS_LOCATE_MAX_PER_RX; }

// ---- the resolution's order (7): candidates compare by (16 - K, the bits of cost, position in the stored list); costs are not
// negative, so their bits order as unsigned integers the way the values do
RTS_HD uint32_t rts_locate_key_k(const RtsTarget& t) { return RTS_LOCATE_MAX_RX - (t.n_receivers < RTS_LOCATE_MAX_RX ? t.n_receivers : RTS_LOCATE_MAX_RX); }
RTS_HD uint64_t rts_locate_key_cost(const RtsTarget& t) { union { double d; uint64_t u; } b; b.d = t.cost; return b.u; }

RTS_HD uint32_t rts_locate_max_candidates(const RtsLocateParams& p) { return p.max_candidates ? p.max_candidates : RTS_LOCATE_DEFAULT_CANDIDATES; }
RTS_HD uint32_t rts_locate_max_targets(const RtsLocateParams& p) { return p.max_targets ? p.max_targets : RTS_LOCATE_DEFAULT_TARGETS; }

// ---- validation (host only, like the evaluator below).  The parameter record: 0, or the number of the rule it breaks (rts_cube_detect_api.hip words the message)
//   1 n_rx  2 rx_positions null  3 a position not finite  4 anchors  5 collinear baselines  6 cspeed  7 carrier  8 sigma_delay
//   9 sigma_doppler  10 gate  11 assoc_delay  12 box  13 min_receivers  14 n_iters  15 max_candidates  16 max_targets  17 source
//   18 n_list without device_list  19 n_list above its limit  20 device_list not 8-byte aligned  21 reserved  22 device_list with tracks
// the records a list of a source may hold: a caller's device list, the evaluator's host list
static inline uint32_t rts_locate_list_most(uint32_t source)
{
    return source == RTS_LOCATE_FROM_PLOTS ? RTS_LOCATE_MAX_LIST : source == RTS_LOCATE_FROM_TRACKS ? RTS_TRACK_MAX_TRACKS : RTS_LOCATE_MAX_CANDIDATES;
}
RTS_HD bool rts_locate_positive(double x) { return rts_locate_finite(x) && x > 0.0; }
static inline int rts_locate_params_check(const RtsLocateParams* p)
{
    if (p->n_rx < 3u || p->n_rx > RTS_LOCATE_MAX_RX) return 1;
    if (!p->rx_positions) return 2;
    for (int c = 0; c < 3; c++) if (!rts_locate_finite(p->tx[c])) return 3;
    for (uint32_t k = 0; k < 3u * p->n_rx; k++) if (!rts_locate_finite(p->rx_positions[k])) return 3;
    const uint32_t* a = p->anchors;
    if (a[0] >= p->n_rx || a[1] >= p->n_rx || a[2] >= p->n_rx || a[0] == a[1] || a[0] == a[2] || a[1] == a[2]) return 4;
    double e1[3], e2[3], x[3];
    for (int c = 0; c < 3; c++) { e1[c] = p->rx_positions[3u * a[1] + (uint32_t)c] - p->rx_positions[3u * a[0] + (uint32_t)c]; e2[c] = p->rx_positions[3u * a[2] + (uint32_t)c] - p->rx_positions[3u * a[0] + (uint32_t)c]; }
    rts_locate_cross(e1, e2, x);
    if (!(rts_locate_norm(x) > 1e-9 * (rts_locate_norm(e1) * rts_locate_norm(e2)))) return 5;
    if (!rts_locate_positive(p->cspeed)) return 6;
    if (!rts_locate_finite(p->carrier) || !(p->carrier >= 0.0)) return 7;
    if (!rts_locate_positive(p->sigma_delay)) return 8;
    if (!rts_locate_positive(p->sigma_doppler)) return 9;
    if (!rts_locate_positive(p->gate)) return 10;
    if (!rts_locate_positive(p->assoc_delay)) return 11;
    for (int c = 0; c < 3; c++) if (!rts_locate_finite(p->box_lo[c]) || !rts_locate_finite(p->box_hi[c]) || p->box_lo[c] > p->box_hi[c]) return 12;
    if (p->min_receivers < 3u || p->min_receivers > p->n_rx) return 13;
    if (p->n_iters > RTS_LOCATE_MAX_ITERS) return 14;
    if (p->max_candidates > RTS_LOCATE_MAX_CANDIDATES) return 15;
    if (p->max_targets > RTS_LOCATE_MAX_TARGETS) return 16;
    if (p->source > RTS_LOCATE_FROM_CANDIDATES) return 17;
    const int rule = rts_device_list_rule(p->device_list, p->n_list, rts_locate_list_most(p->source));
    if (rule) return 17 + rule;
    if (p->reserved[0] || p->reserved[1]) return 21;
    if (p->source == RTS_LOCATE_FROM_TRACKS && p->device_list) return 22;
    return 0;
}
// A host plot list: 0, or 1 with *bad the first record whose rx is below its predecessor's
static inline int rts_locate_plots_check(const RtsPlot* z, uint32_t n, uint32_t* bad)
{
    for (uint32_t j = 1; j < n; j++) if (z[j].rx < z[j - 1u].rx) { *bad = j; return 1; }
    return 0;
}
// A host candidate list: 0, or with *bad the record: 1 not above its predecessor's candidate index, 2 an index at or above
// RTS_LOCATE_MAX_INDEX, 3 n_receivers outside 1 .. RTS_LOCATE_MAX_RX, 4 a cost that is negative or NaN
static inline int rts_locate_candidates_check(const RtsTarget* t, uint32_t n, uint32_t* bad)
{
    for (uint32_t i = 0; i < n; i++) {
        *bad = i;
        if (i && !(t[i].candidate > t[i - 1u].candidate)) return 1;
        for (uint32_t m = 0; m < RTS_LOCATE_MAX_RX; m++) if (t[i].plot[m] != RTS_LOCATE_NONE && t[i].plot[m] >= RTS_LOCATE_MAX_INDEX) return 2;
        if (t[i].n_receivers == 0u || t[i].n_receivers > RTS_LOCATE_MAX_RX) return 3;
        if (!(t[i].cost >= 0.0)) return 4;
    }
    return 0;
}
// a track takes part
RTS_HD bool rts_locate_track_counts(uint32_t flags, uint32_t rx, uint32_t n_rx) { return (flags & RTS_TRACK_CONFIRMED) && !(flags & RTS_TRACK_COASTED) && rx < n_rx; }

// ---- host only from here
// The greedy pass (7) over n stored candidates: up to `capacity` targets to out in ascending candidate index; the total
static inline uint32_t rts_locate_resolve_host(const RtsTarget* cand, uint32_t n, uint32_t max_targets, RtsTarget* out, uint32_t capacity)
{
    std::vector<uint32_t> order(n);
    for (uint32_t i = 0; i < n; i++) order[i] = i;
    std::sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) {
        const uint32_t ka = rts_locate_key_k(cand[a]), kb = rts_locate_key_k(cand[b]);
        if (ka != kb) return ka < kb;
        const uint64_t ca = rts_locate_key_cost(cand[a]), cb = rts_locate_key_cost(cand[b]);
        return ca != cb ? ca < cb : a < b;
    });
    uint32_t top = 0;
    for (uint32_t i = 0; i < n; i++) for (uint32_t m = 0; m < RTS_LOCATE_MAX_RX; m++) if (cand[i].plot[m] != RTS_LOCATE_NONE && cand[i].plot[m] >= top) top = cand[i].plot[m] + 1u;
    std::vector<uint8_t> taken(top, 0), won(n, 0);
    for (uint32_t o = 0; o < n; o++) {
        const RtsTarget& t = cand[order[o]];
        bool is_free = true;
        for (uint32_t m = 0; m < RTS_LOCATE_MAX_RX; m++) if (t.plot[m] != RTS_LOCATE_NONE && taken[t.plot[m]]) is_free = false;
        if (!is_free) continue;
        for (uint32_t m = 0; m < RTS_LOCATE_MAX_RX; m++) if (t.plot[m] != RTS_LOCATE_NONE) taken[t.plot[m]] = 1;
        won[order[o]] = 1;
    }
    uint32_t total = 0;
    for (uint32_t i = 0; i < n; i++) {
        if (!won[i]) continue;
        if (total < capacity && total < max_targets) out[total] = cand[i];
        total++;
    }
    return total;
}

// The step on validated input.  list: RtsPlot[], RtsTrack[] or RtsTarget[] by p->source.  Writes up to `capacity` targets, returns
// the total; *cut: 1 when max_candidates cut the candidates, + 2 when an anchor's segment was cut
static inline uint32_t rts_locate_eval_host(const RtsLocateParams* p, const void* list, uint32_t n_list, RtsTarget* out, uint32_t capacity, uint32_t* cut)
{
    const uint32_t max_c = rts_locate_max_candidates(*p), max_t = rts_locate_max_targets(*p);
    *cut = 0u;
    if (p->source == RTS_LOCATE_FROM_CANDIDATES) {
        if (n_list > max_c) *cut |= 1u;
        return rts_locate_resolve_host((const RtsTarget*)list, n_list < max_c ? n_list : max_c, max_t, out, capacity);
    }
    const RtsLocateGeo g = rts_locate_geo(*p);
    std::vector<double> zR, zf, zp; std::vector<uint32_t> zi, seg(2u * RTS_LOCATE_MAX_RX, 0u);
    for (uint32_t m = 0; m < RTS_LOCATE_MAX_RX; m++) {                  // (rx does not decrease in a plot list; a table is walked per receiver)
        seg[2u * m] = (uint32_t)zR.size();
        for (uint32_t e = 0; e < n_list && m < p->n_rx; e++) {
            double delay, doppler, power;
            if (p->source == RTS_LOCATE_FROM_PLOTS) {
                const RtsPlot& r = ((const RtsPlot*)list)[e];
                if (r.rx != m) continue;
                delay = r.delay; doppler = r.doppler; power = r.power_sum;
            } else {
                const RtsTrack& r = ((const RtsTrack*)list)[e];
                if (r.rx != m || !rts_locate_track_counts(r.flags, r.rx, p->n_rx)) continue;
                delay = r.delay; doppler = r.doppler; power = r.power_sum;
            }
            zR.push_back(rts_locate_range_sum(p->cspeed, delay, doppler, power)); zf.push_back(doppler); zp.push_back(power); zi.push_back(e);
        }
        seg[2u * m + 1u] = (uint32_t)zR.size();
    }
    const RtsLocateList z = {zR.data(), zf.data(), zp.data(), zi.data(), seg.data()};
    uint32_t P[3];
    for (int a = 0; a < 3; a++) {
        const uint32_t lo = seg[2u * g.anchors[a]], hi = seg[2u * g.anchors[a] + 1u];
        P[a] = rts_locate_anchor_count(lo, hi);
        if (hi - lo > RTS_LOCATE_MAX_PER_RX) *cut |= 2u;
    }
    std::vector<RtsTarget> cand, some;
    uint64_t found = 0;
    const double* R2 = zR.data() + seg[2u * g.anchors[2]];
    for (uint32_t i = 0; i < P[0]; i++) for (uint32_t j = 0; j < P[1]; j++) {
        const uint32_t n = rts_locate_pair(g, z, i, j, R2, P[1], P[2], nullptr, 0u);
        if (n == 0u) continue;
        found += n;
        if (cand.size() >= max_c) continue;
        some.resize(n);
        rts_locate_pair(g, z, i, j, R2, P[1], P[2], some.data(), n);
        for (uint32_t q = 0; q < n && cand.size() < max_c; q++) cand.push_back(some[q]);
    }
    if (found > max_c) *cut |= 1u;
    return rts_locate_resolve_host(cand.data(), (uint32_t)cand.size(), max_t, out, capacity);
}
