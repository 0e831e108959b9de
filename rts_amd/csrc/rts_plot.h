// rts_plot.h -- the rules of plot extraction (include/rts_amd.h: RtsPlotParams, RtsPlot), each written once and called by the kernels
// (rts_plot.hip), the launch (rts_cube_plots) and the host evaluator (rts_plots_eval): the flat key of a detection, the integer Doppler
// unwrap, the adjacency predicate, the neighbour enumeration as key intervals of the sorted list, the blocked order of the sums, the
// record from the sums and the root (with the single-cell rule), the validation, and the evaluator itself -- a plain union-find over
// the same neighbour enumeration.  The order of every sum is a pure function of the member count, so kernel and evaluator agree bit
// for bit.  Includes nothing of HIP: it compiles with any host compiler and is tested without a GPU (tests/test_plot_host.py,
// tests/plot/plot_main.cpp).
#pragma once
#include <math.h>
#include <stdint.h>
#include <stddef.h>
#include <vector>
#include "../../include/rts_amd.h"
#include "rts_cfar.h"

#define RTS_PLOT_BLOCK 64u          // members per block of the summation order

// the flat key of cell (rx, k, r) of a map of nd x nb cells per receiver: ascending keys are the detectors' list order
RTS_HD uint64_t rts_plot_key(uint32_t rx, uint32_t k, uint32_t r, uint32_t nd, uint32_t nb) { return ((uint64_t)rx * nd + k) * nb + r; }
RTS_HD uint64_t rts_plot_key(const RtsDetection& d, uint32_t nd, uint32_t nb) { return rts_plot_key(d.rx, d.doppler_bin, d.range_bin, nd, nb); }

// Doppler row k + dk of a circle of nd rows (dk may be negative and may exceed nd: the wrap is applied as it stands)
RTS_HD uint32_t rts_plot_row(uint32_t k, int64_t dk, uint32_t nd)
{
    const int64_t m = ((int64_t)k + dk) % (int64_t)nd;
    return (uint32_t)(m < 0 ? m + (int64_t)nd : m);
}

// k - k0 wrapped into [-nd / 2, nd / 2), in integer arithmetic (nd odd: -(nd - 1) / 2 .. (nd - 1) / 2).  A component wider than half
// the circle is mis-unwrapped: its far members come out on the wrong side of the root.  That is documented, not repaired.
RTS_HD int64_t rts_plot_unwrap(uint32_t k, uint32_t k0, uint32_t nd)
{
    int64_t d = (int64_t)k - (int64_t)k0;
    if (2 * d >= (int64_t)nd) d -= (int64_t)nd; else if (2 * d < -(int64_t)nd) d += (int64_t)nd;
    return d;
}

// two cells are adjacent: the same receiver, |r - r'| <= link_range, some dk with |dk| <= link_doppler and (k + dk) mod nd == k',
// and not the same cell.  Doppler wraps, range does not, receivers never join.
RTS_HD bool rts_plot_adjacent(uint32_t rx_a, uint32_t k_a, uint32_t r_a, uint32_t rx_b, uint32_t k_b, uint32_t r_b, uint32_t lr, uint32_t ld, uint32_t nd)
{
    if (rx_a != rx_b || (k_a == k_b && r_a == r_b)) return false;
    const uint32_t dr = r_a > r_b ? r_a - r_b : r_b - r_a;
    if (dr > lr) return false;
    const uint32_t up = k_b >= k_a ? k_b - k_a : k_b + nd - k_a, down = nd - up;      // steps from k_a to k_b upwards, downwards (nd when up is 0)
    return up <= ld || down <= ld;
}

// The neighbours of cell (rx, k, r) in Doppler row offset dk, |dk| <= link_doppler: the cells of row (k + dk) mod nd whose range bin
// lies in [r - link_range, r + link_range], cut at the map's edges -- an interval [*lo, *hi] of flat keys that a lower-bound binary
// search over the sorted list resolves.  The cell's own key lies inside the interval of dk = 0 (and of every dk that names its own
// row on a short map): the caller skips it.
RTS_HD void rts_plot_interval(uint32_t rx, uint32_t k, uint32_t r, int dk, uint32_t lr, uint32_t nd, uint32_t nb, uint64_t* lo, uint64_t* hi)
{
    const uint32_t kk = rts_plot_row(k, dk, nd);
    const uint32_t r_lo = r > lr ? r - lr : 0u;
    const uint64_t r_hi64 = (uint64_t)r + lr;
    const uint32_t r_hi = r_hi64 < (uint64_t)nb ? (uint32_t)r_hi64 : nb - 1u;
    *lo = rts_plot_key(rx, kk, r_lo, nd, nb); *hi = rts_plot_key(rx, kk, r_hi, nd, nb);
}

// the first index in [0, n) whose key is not below `want` (n when there is none); key(i) must ascend
template <class Key> RTS_HD uint32_t rts_plot_lower_bound(uint32_t n, uint64_t want, Key key)
{
    uint32_t lo = 0, hi = n;
    while (lo < hi) { const uint32_t mid = lo + (hi - lo) / 2u; if (key(mid) < want) lo = mid + 1u; else hi = mid; }
    return lo;
}

// Every neighbour j < i of list element i (adjacency is symmetric: each pair is met once, from its later cell): join(j) for each, in
// the order of the rows dk = -link_doppler .. link_doppler and ascending j within a row.  On a short map a row is named more than
// once and so is a neighbour; joining twice changes nothing.  key(j): the flat key of element j, j < i.
template <class Key, class Join> RTS_HD void rts_plot_neighbours(uint32_t i, uint32_t rx, uint32_t k, uint32_t r, uint32_t lr, uint32_t ld, uint32_t nd, uint32_t nb, Key key, Join join)
{
    for (int dk = -(int)ld; dk <= (int)ld; dk++) {
        uint64_t lo, hi; rts_plot_interval(rx, k, r, dk, lr, nd, nb, &lo, &hi);
        for (uint32_t j = rts_plot_lower_bound(i, lo, key); j < i && key(j) <= hi; j++) join(j);
    }
}

// ---- the sums.  Members are taken in ascending list index, added left to right (from 0) inside blocks of RTS_PLOT_BLOCK consecutive
// members, and the block sums are added left to right (from 0): rts_plot_member adds one member to its block's sums, rts_plot_fold one
// block to the total.  Each product is rounded before it is added (the units are built without contraction); dr^2 and dk^2 are formed
// first, in double, and are exact below 2^53.  The extent and the peak are order-free: minima, maxima and a maximum under a total order.
struct RtsPlotSums { double S, Sr, Sk, Srr, Skk, N; };
struct RtsPlotExtent { uint32_t r_min, r_max; int64_t dk_min, dk_max; uint32_t peak_index; double peak_power; };
RTS_HD RtsPlotSums rts_plot_sums_zero() { RtsPlotSums s; s.S = 0.0; s.Sr = 0.0; s.Sk = 0.0; s.Srr = 0.0; s.Skk = 0.0; s.N = 0.0; return s; }
RTS_HD RtsPlotExtent rts_plot_extent_none() { RtsPlotExtent e; e.r_min = 0xffffffffu; e.r_max = 0u; e.dk_min = INT64_MAX; e.dk_max = INT64_MIN; e.peak_index = 0xffffffffu; e.peak_power = 0.0; return e; }
// the peak of two: the larger power, ties to the lower index (an extent that has seen no member carries index 0xffffffff and loses)
RTS_HD bool rts_plot_peak_before(double pa, uint32_t ia, double pb, uint32_t ib) { return ib == 0xffffffffu || (ia != 0xffffffffu && (pa > pb || (pa == pb && ia < ib))); }
RTS_HD void rts_plot_extent_join(RtsPlotExtent& a, const RtsPlotExtent& b)
{
    if (b.r_min < a.r_min) a.r_min = b.r_min;
    if (b.r_max > a.r_max) a.r_max = b.r_max;
    if (b.dk_min < a.dk_min) a.dk_min = b.dk_min;
    if (b.dk_max > a.dk_max) a.dk_max = b.dk_max;
    if (!rts_plot_peak_before(a.peak_power, a.peak_index, b.peak_power, b.peak_index)) { a.peak_power = b.peak_power; a.peak_index = b.peak_index; }
}
// member `index` of the list, of the plot rooted at cell (k0, r0): into its block's sums and the extent
RTS_HD void rts_plot_member(const RtsDetection& d, uint32_t index, uint32_t k0, uint32_t r0, uint32_t nd, RtsPlotSums& b, RtsPlotExtent& e)
{
    const int64_t dri = (int64_t)d.range_bin - (int64_t)r0, dki = rts_plot_unwrap(d.doppler_bin, k0, nd);
    const double P = d.power, dr = (double)dri, dk = (double)dki;
    b.S += P; b.Sr += P * dr; b.Sk += P * dk; b.Srr += P * (dr * dr); b.Skk += P * (dk * dk); b.N += d.noise;
    RtsPlotExtent m; m.r_min = d.range_bin; m.r_max = d.range_bin; m.dk_min = dki; m.dk_max = dki; m.peak_index = index; m.peak_power = P;
    rts_plot_extent_join(e, m);
}
RTS_HD void rts_plot_fold(RtsPlotSums& t, const RtsPlotSums& b) { t.S += b.S; t.Sr += b.Sr; t.Sk += b.Sk; t.Srr += b.Srr; t.Skk += b.Skk; t.N += b.N; }

// block `blk` of a plot of `count` members: members blk RTS_PLOT_BLOCK .. of the plot, member(m) = the list index of its m-th member
template <class Member> RTS_HD RtsPlotSums rts_plot_block(const RtsDetection* list, uint32_t count, uint32_t blk, Member member, uint32_t k0, uint32_t r0, uint32_t nd, RtsPlotExtent& e)
{
    RtsPlotSums b = rts_plot_sums_zero();
    const uint32_t m0 = blk * RTS_PLOT_BLOCK, m1 = count - m0 < RTS_PLOT_BLOCK ? count : m0 + RTS_PLOT_BLOCK;
    for (uint32_t m = m0; m < m1; m++) { const uint32_t i = member(m); rts_plot_member(list[i], i, k0, r0, nd, b, e); }
    return b;
}
// the whole order, one block after the other (the host evaluator; one lane of the kernel for a plot it reduces alone)
template <class Member> RTS_HD RtsPlotSums rts_plot_reduce(const RtsDetection* list, uint32_t count, Member member, uint32_t k0, uint32_t r0, uint32_t nd, RtsPlotExtent& e)
{
    RtsPlotSums t = rts_plot_sums_zero();
    for (uint32_t blk = 0; blk * RTS_PLOT_BLOCK < count; blk++) rts_plot_fold(t, rts_plot_block(list, count, blk, member, k0, r0, nd, e));
    return t;
}

// The record of the plot rooted at list element first_index (`root`), of n_cells members with sums t and extent e.  A plot of one cell
// takes that detection's own refinement, and its delay and doppler are rts_cfar_record's expressions: the same bits.  S <= 0 (all
// powers zero): centroids at the root, spreads 0.
RTS_HD RtsPlot rts_plot_record(const RtsDetection& root, uint32_t first_index, uint32_t n_cells, const RtsPlotSums& t, const RtsPlotExtent& e,
                               uint32_t nd, double t0, double dt, double pri)
{
    const uint32_t k0 = root.doppler_bin, r0 = root.range_bin;
    RtsPlot p;
    p.rx = root.rx; p.n_cells = n_cells; p.first_index = first_index; p.peak_index = e.peak_index;
    p.range_min = e.r_min; p.range_max = e.r_max;
    p.doppler_lo = rts_plot_row(k0, e.dk_min, nd);
    const int64_t span = e.dk_max - e.dk_min + 1;
    p.doppler_span = span < (int64_t)nd ? (uint32_t)span : nd;
    p.power_sum = t.S; p.peak_power = e.peak_power; p.noise_sum = t.N;
    double rc, w, sr = 0.0, sk = 0.0;
    if (n_cells == 1u) { rc = (double)r0 + root.range_offset; w = (double)k0 + root.doppler_offset; }
    else if (!(t.S > 0.0)) { rc = (double)r0; w = (double)k0; }
    else {
        const double mr = t.Sr / t.S, mk = t.Sk / t.S;
        rc = (double)r0 + mr; w = (double)k0 + mk;
        sr = sqrt(fmax(0.0, t.Srr / t.S - mr * mr)); sk = sqrt(fmax(0.0, t.Skk / t.S - mk * mk));
    }
    const double half = 0.5 * (double)nd;
    if (w >= half) w -= (double)nd; else if (w < -half) w += (double)nd;
    p.range_centroid = rc; p.doppler_centroid = w; p.range_spread = sr; p.doppler_spread = sk;
    p.delay = t0 + rc * dt;
    p.doppler = pri > 0.0 ? w / ((double)nd * pri) : 0.0;
    return p;
}

// ---- validation.  The parameter record: 0, or the number of the rule it breaks (rts_cube_detect_api.hip words the message)
//   1 link_range  2 link_doppler  3 reserved  4 pri  5 device_list with n_doppler = 0  6 device_list not 8-byte aligned
//   7 n_list or n_doppler without device_list
RTS_HD int rts_plot_params_check(const RtsPlotParams* p)
{
    if (p->link_range > RTS_PLOT_MAX_LINK) return 1;
    if (p->link_doppler > RTS_PLOT_MAX_LINK) return 2;
    if (p->reserved[0] || p->reserved[1]) return 3;
    if (!(p->pri >= 0.0) || !(p->pri <= 1.7976931348623157e308)) return 4;
    if (p->device_list) { if (p->n_doppler == 0u) return 5; if ((uintptr_t)p->device_list & 7u) return 6; }
    else if (p->n_list || p->n_doppler) return 7;
    return 0;
}
// A host list: 0, or 1 (a bin outside the map of n_rx x nd x nb cells) or 2 (not in strictly ascending flat order) with *bad the record
RTS_HD int rts_plot_list_check(const RtsDetection* list, uint32_t n, uint32_t n_rx, uint32_t nd, uint32_t nb, uint32_t* bad)
{
    for (uint32_t i = 0; i < n; i++) {
        *bad = i;
        if (list[i].rx >= n_rx || list[i].doppler_bin >= nd || list[i].range_bin >= nb) return 1;
        if (i && rts_plot_key(list[i - 1], nd, nb) >= rts_plot_key(list[i], nd, nb)) return 2;
    }
    return 0;
}

// ---- host only from here
// The plots of a validated host list: a union-find whose roots are component minima (the smaller root always becomes the parent) over
// rts_plot_neighbours, the members of each component gathered in ascending index, the records through rts_plot_reduce and
// rts_plot_record.  Writes up to `capacity` records in ascending first_index and returns the total.
static inline uint32_t rts_plots_eval_host(const RtsCubeParams* q, const RtsDetection* list, uint32_t n, uint32_t nd, const RtsPlotParams* p, RtsPlot* out, uint32_t capacity)
{
    const uint32_t nb = q->n_bins, min_cells = p->min_cells ? p->min_cells : 1u;
    std::vector<uint32_t> parent(n), label(n), count(n, 0u), start((size_t)n + 1u, 0u), members(n);
    const auto key = [list, nd, nb](uint32_t j) { return rts_plot_key(list[j], nd, nb); };
    const auto find = [&parent](uint32_t x) { while (parent[x] != x) { parent[x] = parent[parent[x]]; x = parent[x]; } return x; };
    for (uint32_t i = 0; i < n; i++) {
        parent[i] = i;
        rts_plot_neighbours(i, list[i].rx, list[i].doppler_bin, list[i].range_bin, p->link_range, p->link_doppler, nd, nb, key,
                            [&](uint32_t j) { const uint32_t a = find(i), b = find(j); if (a < b) parent[b] = a; else parent[a] = b; });
    }
    for (uint32_t i = 0; i < n; i++) { label[i] = find(i); count[label[i]]++; }
    for (uint32_t i = 0; i < n; i++) start[i + 1u] = start[i] + count[i];
    std::vector<uint32_t> fill(start.begin(), start.end() - 1);
    for (uint32_t i = 0; i < n; i++) members[fill[label[i]]++] = i;
    uint32_t total = 0;
    for (uint32_t root = 0; root < n; root++) {
        if (count[root] < min_cells || count[root] == 0u) continue;
        if (total < capacity) {
            const uint32_t* mem = members.data() + start[root];
            RtsPlotExtent e = rts_plot_extent_none();
            const RtsPlotSums t = rts_plot_reduce(list, count[root], [mem](uint32_t m) { return mem[m]; }, list[root].doppler_bin, list[root].range_bin, nd, e);
            out[total] = rts_plot_record(list[root], root, count[root], t, e, nd, q->t0, q->dt, p->pri);
        }
        total++;
    }
    return total;
}
