// rts_track.h -- the rules of the tracker step (include/rts_amd.h: RtsTrackParams, RtsTrack), each written once and called by the
// kernels (rts_track.hip), the entry points (rts_cube_detect_api.hip) and the host evaluator (rts_tracks_eval): the Doppler wrap, the
// prediction with S and its determinant, the innovation and d2, the edge rule, the candidate list and its order, the update, the
// coast, the initiation, the lifecycle, the validation, and the evaluator itself -- the serial greedy pass over the sorted kept
// edges (the kernels reach the same matching by rounds).  Every expression is written in the operand order of the header text and
// the units are built without contraction, so kernel and evaluator agree bit for bit.  Includes nothing of HIP: it compiles with any
// host compiler and is tested without a GPU (tests/test_track_host.py, tests/track/track_main.cpp).
#pragma once
#include <math.h>
#include <stdint.h>
#include <stddef.h>
#include <algorithm>
#include <vector>
#include "../../include/rts_amd.h"
#include "rts_cfar.h"             // RTS_HD

#define RTS_TRACK_NONE 0xffffffffu
#define RTS_TRACK_FLAGS (RTS_TRACK_CONFIRMED | RTS_TRACK_COASTED | RTS_TRACK_NEW)

RTS_HD bool rts_track_finite(double x) { return x - x == 0.0; }      // (no isfinite overload question between host and device)

// x into [-period / 2, period / 2) when period > 0
RTS_HD double rts_track_wrap(double x, double period)
{
    if (!(period > 0.0)) return x;
    const double h = 0.5 * period;
    double r = x - period * floor((x + h) / period);
    if (r >= h) r -= period; else if (r < -h) r += period;
    return r;
}

// a track carried over the interval T: the predicted state and covariance, S (s_df = pdf) and its determinant
struct RtsTrackPred { double d, f, pdd, pdf, pff, s_dd, s_ff, det; };
RTS_HD RtsTrackPred rts_track_predict(const RtsTrack& t, const RtsTrackParams& p, double T)
{
    const double a = p.delay_rate_per_hz * T;
    RtsTrackPred r;
    r.d = t.delay + a * t.doppler; r.f = t.doppler;
    const double u = t.p_df + a * t.p_ff;
    r.pdd = ((t.p_dd + a * t.p_df) + a * u) + p.q * (((a * a) * T) / 3.0);
    r.pdf = u + p.q * ((a * T) / 2.0);
    r.pff = t.p_ff + p.q * T;
    r.s_dd = r.pdd + p.sigma_delay * p.sigma_delay;
    r.s_ff = r.pff + p.sigma_doppler * p.sigma_doppler;
    r.det = r.s_dd * r.s_ff - r.pdf * r.pdf;
    return r;
}

RTS_HD void rts_track_innovation(const RtsTrackPred& r, double z_d, double z_f, double period, double* v_d, double* v_f)
{
    *v_d = z_d - r.d; *v_f = rts_track_wrap(z_f - r.f, period);
}
RTS_HD double rts_track_d2(const RtsTrackPred& r, double v_d, double v_f)
{
    return ((((v_d * v_d) * r.s_ff) - ((2.0 * (v_d * v_f)) * r.pdf)) + ((v_f * v_f) * r.s_dd)) / r.det;
}
// The edge rule for a finite plot of the track's receiver: true with *d2 when 0 <= d2 <= gate (d2 + 0.0: a zero is +0, so the bits
// of an edge's d2 order as unsigned integers the way the values do)
RTS_HD bool rts_track_edge(const RtsTrackPred& r, double z_d, double z_f, double period, double gate, double* d2)
{
    double v_d, v_f; rts_track_innovation(r, z_d, z_f, period, &v_d, &v_f);
    const double x = rts_track_d2(r, v_d, v_f) + 0.0;
    *d2 = x;
    return x >= 0.0 && x <= gate;
}
RTS_HD bool rts_track_plot_finite(double z_d, double z_f) { return rts_track_finite(z_d) && rts_track_finite(z_f); }

// The candidate list of one track: up to K edges in ascending (d2, plot index), at d2[k * stride], j[k * stride].  Plots are offered
// in any order; the list ends as the K smallest of all that were offered.
RTS_HD bool rts_track_cand_before(double d2a, uint32_t ja, double d2b, uint32_t jb) { return d2a < d2b || (d2a == d2b && ja < jb); }
RTS_HD void rts_track_cand_insert(double* d2, uint32_t* j, size_t stride, uint32_t* n, uint32_t K, double x, uint32_t jx)
{
    uint32_t k = *n;
    if (k == K) { if (!rts_track_cand_before(x, jx, d2[(size_t)(K - 1u) * stride], j[(size_t)(K - 1u) * stride])) return; k = K - 1u; }
    else *n = k + 1u;
    for (; k > 0u && rts_track_cand_before(x, jx, d2[(size_t)(k - 1u) * stride], j[(size_t)(k - 1u) * stride]); k--) {
        d2[(size_t)k * stride] = d2[(size_t)(k - 1u) * stride]; j[(size_t)k * stride] = j[(size_t)(k - 1u) * stride];
    }
    d2[(size_t)k * stride] = x; j[(size_t)k * stride] = jx;
}

RTS_HD uint32_t rts_track_flags_after(uint32_t flags, uint32_t hits, uint32_t confirm_hits, uint32_t now)
{
    return (flags & RTS_TRACK_CONFIRMED) | (hits >= confirm_hits ? RTS_TRACK_CONFIRMED : 0u) | now;
}
// the track after a frame in which plot j (delay z_d, Doppler z_f, power_sum pw) was matched to it with distance d2
RTS_HD RtsTrack rts_track_update(const RtsTrack& t, const RtsTrackPred& r, const RtsTrackParams& p, uint32_t j, double z_d, double z_f, double pw, double d2)
{
    double v_d, v_f; rts_track_innovation(r, z_d, z_f, p.doppler_period, &v_d, &v_f);
    const double k_dd = ((r.pdd * r.s_ff) - (r.pdf * r.pdf)) / r.det, k_df = ((r.pdf * r.s_dd) - (r.pdd * r.pdf)) / r.det;
    const double k_fd = ((r.pdf * r.s_ff) - (r.pff * r.pdf)) / r.det, k_ff = ((r.pff * r.s_dd) - (r.pdf * r.pdf)) / r.det;
    RtsTrack o = t;
    o.delay = r.d + ((k_dd * v_d) + (k_df * v_f));
    o.doppler = rts_track_wrap(r.f + ((k_fd * v_d) + (k_ff * v_f)), p.doppler_period);
    o.p_dd = r.pdd - ((k_dd * r.pdd) + (k_df * r.pdf));
    o.p_df = r.pdf - ((k_dd * r.pdf) + (k_df * r.pff));
    o.p_ff = r.pff - ((k_fd * r.pdf) + (k_ff * r.pff));
    o.hits = t.hits + 1u; o.misses = 0u; o.age = t.age + 1u;
    o.flags = rts_track_flags_after(t.flags, o.hits, p.confirm_hits, 0u);
    o.plot_index = j; o.d2 = d2; o.power_sum = pw;
    return o;
}
// the track after a frame without a plot; *keep: it survives
RTS_HD RtsTrack rts_track_coast(const RtsTrack& t, const RtsTrackPred& r, const RtsTrackParams& p, bool* keep)
{
    RtsTrack o = t;
    o.delay = r.d; o.doppler = r.f; o.p_dd = r.pdd; o.p_df = r.pdf; o.p_ff = r.pff;
    o.misses = t.misses + 1u; o.age = t.age + 1u;
    o.flags = (t.flags & RTS_TRACK_CONFIRMED) | RTS_TRACK_COASTED;
    o.plot_index = RTS_TRACK_NONE; o.d2 = 0.0; o.power_sum = 0.0;
    *keep = !(o.misses > ((t.flags & RTS_TRACK_CONFIRMED) ? p.max_misses : p.tentative_misses));
    return o;
}
// the track that finite plot j starts
RTS_HD RtsTrack rts_track_start(const RtsTrackParams& p, uint64_t id, uint32_t j, uint32_t rx, double z_d, double z_f, double pw)
{
    RtsTrack o;
    o.id = id; o.rx = rx; o.hits = 1u; o.misses = 0u; o.age = 1u; o.plot_index = j;
    o.flags = rts_track_flags_after(0u, 1u, p.confirm_hits, RTS_TRACK_NEW);
    o.delay = z_d; o.doppler = rts_track_wrap(z_f, p.doppler_period);
    o.p_dd = p.sigma_delay * p.sigma_delay; o.p_df = 0.0; o.p_ff = p.sigma_doppler * p.sigma_doppler;
    o.d2 = 0.0; o.power_sum = pw;
    return o;
}
RTS_HD uint32_t rts_track_table_size(const RtsTrackParams& p) { return p.max_tracks ? p.max_tracks : RTS_TRACK_DEFAULT_TRACKS; }

// ---- validation.  The parameter record: 0, or the number of the rule it breaks (rts_cube_detect_api.hip words the message)
//   1 gate  2 sigma_delay  3 sigma_doppler  4 q  5 delay_rate_per_hz  6 doppler_period  7 confirm_hits  8 max_candidates  9 max_tracks
//   10 reserved  11 n_plots without device_plots  12 n_plots above RTS_TRACK_MAX_PLOTS  13 device_plots not 8-byte aligned
RTS_HD int rts_track_params_check(const RtsTrackParams* p)
{
    if (!rts_track_finite(p->gate) || !(p->gate > 0.0)) return 1;
    if (!rts_track_finite(p->sigma_delay) || !(p->sigma_delay > 0.0)) return 2;
    if (!rts_track_finite(p->sigma_doppler) || !(p->sigma_doppler > 0.0)) return 3;
    if (!rts_track_finite(p->q) || !(p->q >= 0.0)) return 4;
    if (!rts_track_finite(p->delay_rate_per_hz)) return 5;
    if (!rts_track_finite(p->doppler_period) || !(p->doppler_period >= 0.0)) return 6;
    if (p->confirm_hits == 0u) return 7;
    if (p->max_candidates == 0u || p->max_candidates > RTS_TRACK_MAX_CAND) return 8;
    if (p->max_tracks > RTS_TRACK_MAX_TRACKS) return 9;
    if (p->reserved[0] || p->reserved[1]) return 10;
    if (!p->device_plots && p->n_plots) return 11;
    if (p->n_plots > RTS_TRACK_MAX_PLOTS) return 12;
    if ((uintptr_t)p->device_plots & 7u) return 13;
    return 0;
}
RTS_HD bool rts_track_interval_ok(double T) { return rts_track_finite(T) && T > 0.0; }
// A host table: 0, or 1 (state or covariance not finite, p_dd or p_ff negative) or 2 (unknown flag bits) with *bad the record
RTS_HD int rts_track_table_check(const RtsTrack* t, uint32_t n, uint32_t* bad)
{
    for (uint32_t i = 0; i < n; i++) {
        *bad = i;
        if (!rts_track_finite(t[i].delay) || !rts_track_finite(t[i].doppler) || !rts_track_finite(t[i].p_dd) || !rts_track_finite(t[i].p_df) || !rts_track_finite(t[i].p_ff)
            || t[i].p_dd < 0.0 || t[i].p_ff < 0.0) return 1;
        if (t[i].flags & ~RTS_TRACK_FLAGS) return 2;
    }
    return 0;
}
// A host plot list: 0, or 1 with *bad the first record whose rx is below its predecessor's
RTS_HD int rts_track_plots_check(const RtsPlot* z, uint32_t n, uint32_t* bad)
{
    for (uint32_t j = 1; j < n; j++) if (z[j].rx < z[j - 1u].rx) { *bad = j; return 1; }
    return 0;
}

// ---- host only from here
// One step on validated input (n_in <= the table size).  Writes up to `capacity` records, returns the total and sets *next_id_out.
static inline uint32_t rts_tracks_eval_host(const RtsTrackParams* p, const RtsTrack* in, uint32_t n_in, uint64_t next_id, double T, const RtsPlot* z, uint32_t n_z,
                                            RtsTrack* out, uint32_t capacity, uint64_t* next_id_out)
{
    const uint32_t K = p->max_candidates, table = rts_track_table_size(*p);
    struct Edge { double d2; uint32_t i, j; };
    std::vector<RtsTrackPred> pred(n_in);
    std::vector<Edge> edges;
    std::vector<double> cd(K); std::vector<uint32_t> cj(K);
    for (uint32_t i = 0; i < n_in; i++) {
        pred[i] = rts_track_predict(in[i], *p, T);
        uint32_t n = 0, lo = 0, hi = n_z;                      // the receiver's part of the list (rx does not decrease)
        while (lo < hi) { const uint32_t mid = lo + (hi - lo) / 2u; if (z[mid].rx < in[i].rx) lo = mid + 1u; else hi = mid; }
        for (uint32_t j = lo; j < n_z && z[j].rx == in[i].rx; j++) {
            double d2;
            if (!rts_track_plot_finite(z[j].delay, z[j].doppler)) continue;
            if (rts_track_edge(pred[i], z[j].delay, z[j].doppler, p->doppler_period, p->gate, &d2)) rts_track_cand_insert(cd.data(), cj.data(), 1, &n, K, d2, j);
        }
        for (uint32_t k = 0; k < n; k++) edges.push_back(Edge{cd[k], i, cj[k]});
    }
    std::sort(edges.begin(), edges.end(), [](const Edge& a, const Edge& b) { return a.d2 != b.d2 ? a.d2 < b.d2 : a.i != b.i ? a.i < b.i : a.j < b.j; });
    std::vector<uint32_t> of_track(n_in, RTS_TRACK_NONE), of_plot(n_z, RTS_TRACK_NONE);
    std::vector<double> d2_of(n_in, 0.0);
    for (const Edge& e : edges) if (of_track[e.i] == RTS_TRACK_NONE && of_plot[e.j] == RTS_TRACK_NONE) { of_track[e.i] = e.j; of_plot[e.j] = e.i; d2_of[e.i] = e.d2; }
    uint32_t total = 0;
    for (uint32_t i = 0; i < n_in; i++) {
        bool keep = true;
        const uint32_t j = of_track[i];
        const RtsTrack o = j != RTS_TRACK_NONE ? rts_track_update(in[i], pred[i], *p, j, z[j].delay, z[j].doppler, z[j].power_sum, d2_of[i]) : rts_track_coast(in[i], pred[i], *p, &keep);
        if (!keep) continue;
        if (total < capacity) out[total] = o;
        total++;
    }
    const uint32_t survivors = total;
    for (uint32_t j = 0; j < n_z; j++) {
        if (of_plot[j] != RTS_TRACK_NONE || !rts_track_plot_finite(z[j].delay, z[j].doppler)) continue;
        if (total < capacity && total < table) out[total] = rts_track_start(*p, next_id + (total - survivors), j, z[j].rx, z[j].delay, z[j].doppler, z[j].power_sum);
        total++;
    }
    *next_id_out = next_id + ((total < table ? total : table) - survivors);
    return total;
}
