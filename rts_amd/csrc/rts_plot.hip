// rts_plot.hip -- plot extraction on the device (include/rts_amd.h: rts_cube_plots): the connected components of a SPARSE, SORTED
// detection list by label equivalence, and one record per component.  Every rule -- key, adjacency, neighbour intervals, the order of
// the sums, the record -- is rts_plot.h, shared with the host evaluator rts_plots_eval.  Wave64; the launches are sized by the list's
// capacity and every kernel reads the count on the device, so the call never waits on the host.
//   1. k_plot_init     flat keys; parent[i] = i; the sort's identity values; the padding beyond the count
//   2. k_plot_link     one thread per detection: per Doppler row of the adjacency a lower-bound search over the keys of the elements
//                      BEFORE it and a walk along the interval; each neighbour found is united with it in the parent array
//   3. k_plot_flatten  parent[i] = the root of i = the smallest index of its component
//   4. radix sort of (label, index) by label: stable, so each component's members come together in ascending list index and the
//      components in ascending first_index
//   5. k_plot_flag     heads of the sorted runs, their lengths (a binary search for the run's end), the min_cells rule -> keep flags;
//      an exclusive scan of the flags gives every kept plot its output position and, in the extra last element, the total
//   6. k_plot_reduce   per kept plot the blocked sums in the fixed order and the record
// Why the labels do not depend on a race: parent[x] <= x always, and a union only ever writes a SMALLER index into a parent word
// (atomicMin), so the links form a forest whose every root is the minimum of its tree; a union that loses a race goes on with the
// value the word held, so no equivalence is dropped (rts_plot_unite).  When k_plot_link has ended every component is one tree, its
// root the component's minimum whatever the interleaving was; k_plot_flatten reads that root.  The parent array is in global memory: a
// default-length list is 65 536 x 4 B of parents, more than a workgroup's LDS, and the unions cross workgroups.
#include <cstring>
#include <hip/hip_runtime.h>
#include <rocprim/rocprim.hpp>
#include "rts_internal.h"

#define RTS_PLOT_THREADS 256
// a plot of more members than this is reduced by its wave together (a lane per 64-member block), a smaller one by one lane
#define RTS_PLOT_WAVE_ABOVE 64u

struct RtsPlotArgs {
    const RtsDetection* list; const uint32_t* n_dev; uint32_t n_cap, cap;      // cap = max(n_cap, 1): what the launches and the sort are sized by
    uint32_t nd, nb, lr, ld, min_cells, max_plots;
    double t0, dt, pri;
    uint64_t* key; uint32_t* parent; uint32_t* idx; uint32_t* lab_s; uint32_t* idx_s; uint32_t* len; uint32_t* flag; const uint32_t* off; RtsPlot* out;
};

// the list's length: the first min(n_cap, *n_dev) records count
__device__ __forceinline__ uint32_t rts_plot_n(const RtsPlotArgs& a)
{
    if (!a.n_dev) return a.n_cap;
    const uint32_t n = *a.n_dev;
    return n < a.n_cap ? n : a.n_cap;
}

// a parent word as another thread's union may just have left it (device scope: the unions cross workgroups and XCDs)
__device__ __forceinline__ uint32_t rts_plot_load(const uint32_t* parent, uint32_t x) { return __hip_atomic_load(parent + x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ uint32_t rts_plot_find(const uint32_t* parent, uint32_t x)
{
    for (uint32_t p = rts_plot_load(parent, x); p != x; p = rts_plot_load(parent, x)) x = p;      // (p < x: the walk descends and ends)
    return x;
}
// Unites the trees of a and b: the larger root is hung under the smaller with atomicMin.  When the word no longer held the root
// (another union was faster), the minimum now stands in it and the value it held, `old`, is still to be united with the smaller
// root: the loop goes on with it, so whoever wins, every pair that was asked for ends in one tree.
__device__ __forceinline__ void rts_plot_unite(uint32_t* parent, uint32_t a, uint32_t b)
{
    for (;;) {
        a = rts_plot_find(parent, a); b = rts_plot_find(parent, b);
        if (a == b) return;
        if (a < b) { const uint32_t t = a; a = b; b = t; }          // a: the larger root
        const uint32_t old = atomicMin(parent + a, b);
        if (old == a) return;
        a = old;
    }
}

__global__ void __launch_bounds__(RTS_PLOT_THREADS) k_plot_init(const RtsPlotArgs a)
{
    const uint32_t i = blockIdx.x * RTS_PLOT_THREADS + threadIdx.x;
    if (i >= a.cap) return;
    const uint32_t n = rts_plot_n(a);
    a.idx[i] = i;
    if (i < n) { a.key[i] = rts_plot_key(a.list[i], a.nd, a.nb); a.parent[i] = i; }
    else a.parent[i] = a.cap;                                        // (padding: sorts behind every label)
}

__global__ void __launch_bounds__(RTS_PLOT_THREADS) k_plot_link(const RtsPlotArgs a)
{
    const uint32_t i = blockIdx.x * RTS_PLOT_THREADS + threadIdx.x;
    if (i >= rts_plot_n(a)) return;
    const RtsDetection& d = a.list[i];
    const uint64_t* key = a.key; uint32_t* parent = a.parent;
    rts_plot_neighbours(i, d.rx, d.doppler_bin, d.range_bin, a.lr, a.ld, a.nd, a.nb, [key](uint32_t j) { return key[j]; },
                        [parent, i](uint32_t j) { rts_plot_unite(parent, i, j); });
}

// (other threads of this kernel write roots into words this one walks through: a walk that meets one only gets there sooner)
__global__ void __launch_bounds__(RTS_PLOT_THREADS) k_plot_flatten(const RtsPlotArgs a)
{
    const uint32_t i = blockIdx.x * RTS_PLOT_THREADS + threadIdx.x;
    if (i >= rts_plot_n(a)) return;
    const uint32_t root = rts_plot_find(a.parent, i);
    __hip_atomic_store(a.parent + i, root, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__global__ void __launch_bounds__(RTS_PLOT_THREADS) k_plot_flag(const RtsPlotArgs a)
{
    const uint32_t s = blockIdx.x * RTS_PLOT_THREADS + threadIdx.x;
    if (s == 0) a.flag[a.cap] = 0;                                  // the scan's extra element: its offset is the total
    if (s >= a.cap) return;
    const uint32_t n = rts_plot_n(a);
    uint32_t keep = 0, len = 0;
    if (s < n) {
        const uint32_t lab = a.lab_s[s];
        if (s == 0 || a.lab_s[s - 1] != lab) {                      // the head of a run: its end is the first sorted label above it
            const uint32_t* ls = a.lab_s;
            const uint32_t end = s + 1u + rts_plot_lower_bound(n - (s + 1u), (uint64_t)lab + 1u, [ls, s](uint32_t j) { return (uint64_t)ls[s + 1u + j]; });
            len = end - s;
            keep = len >= a.min_cells ? 1u : 0u;
        }
    }
    a.len[s] = len; a.flag[s] = keep;
}

__device__ __forceinline__ RtsPlotSums rts_plot_sums_lane(const RtsPlotSums& v, int j)
{
    RtsPlotSums o;
    o.S = __shfl(v.S, j); o.Sr = __shfl(v.Sr, j); o.Sk = __shfl(v.Sk, j); o.Srr = __shfl(v.Srr, j); o.Skk = __shfl(v.Skk, j); o.N = __shfl(v.N, j);
    return o;
}
__device__ __forceinline__ RtsPlotExtent rts_plot_extent_xor(const RtsPlotExtent& v, int m)
{
    RtsPlotExtent o;
    o.r_min = __shfl_xor(v.r_min, m); o.r_max = __shfl_xor(v.r_max, m);
    o.dk_min = (int64_t)__shfl_xor((long long)v.dk_min, m); o.dk_max = (int64_t)__shfl_xor((long long)v.dk_max, m);
    o.peak_index = __shfl_xor(v.peak_index, m); o.peak_power = __shfl_xor(v.peak_power, m);
    return o;
}

// One thread per sorted position; a wave covers 64 of them.  A kept head of at most RTS_PLOT_WAVE_ABOVE members is its lane's work
// (rts_plot_reduce, the evaluator's text).  The larger ones the wave takes one after the other, together: lane l forms the sums of
// blocks l, l + 64, .. (rts_plot_block), and after every 64 blocks the block sums are folded left to right -- every lane folds the
// same values, read lane by lane, so the order is the evaluator's.  Extent and peak are order-free: a butterfly at the end.
__global__ void __launch_bounds__(RTS_PLOT_THREADS) k_plot_reduce(const RtsPlotArgs a)
{
    const uint32_t s = blockIdx.x * RTS_PLOT_THREADS + threadIdx.x, lane = threadIdx.x & 63u;
    const bool keep = s < a.cap && a.flag[s] != 0u;
    const uint32_t len = keep ? a.len[s] : 0u, pos = keep ? a.off[s] : 0u;
    const bool write = keep && pos < a.max_plots;
    const uint32_t* idx_s = a.idx_s;
    if (write && len <= RTS_PLOT_WAVE_ABOVE) {
        const uint32_t root = idx_s[s];
        const RtsDetection& r = a.list[root];
        RtsPlotExtent e = rts_plot_extent_none();
        const RtsPlotSums t = rts_plot_reduce(a.list, len, [idx_s, s](uint32_t m) { return idx_s[s + m]; }, r.doppler_bin, r.range_bin, a.nd, e);
        a.out[pos] = rts_plot_record(r, root, len, t, e, a.nd, a.t0, a.dt, a.pri);
    }
    for (unsigned long long rest = __ballot(write && len > RTS_PLOT_WAVE_ABOVE); rest != 0ull; rest &= rest - 1ull) {
        const int src = __ffsll((long long)rest) - 1;
        const uint32_t s0 = s - lane + (uint32_t)src, L = __shfl(len, src), P = __shfl(pos, src);
        const uint32_t root = idx_s[s0];
        const RtsDetection& r = a.list[root];
        const uint32_t k0 = r.doppler_bin, r0 = r.range_bin, n_blocks = (L + RTS_PLOT_BLOCK - 1u) / RTS_PLOT_BLOCK;
        RtsPlotExtent e = rts_plot_extent_none();
        RtsPlotSums t = rts_plot_sums_zero();
        for (uint32_t b0 = 0; b0 < n_blocks; b0 += 64u) {             // (wave-uniform)
            RtsPlotSums blk = rts_plot_sums_zero();
            if (b0 + lane < n_blocks) blk = rts_plot_block(a.list, L, b0 + lane, [idx_s, s0](uint32_t m) { return idx_s[s0 + m]; }, k0, r0, a.nd, e);
            const int cnt = n_blocks - b0 < 64u ? (int)(n_blocks - b0) : 64;
            for (int j = 0; j < cnt; j++) rts_plot_fold(t, rts_plot_sums_lane(blk, j));
        }
        for (int m = 32; m >= 1; m >>= 1) rts_plot_extent_join(e, rts_plot_extent_xor(e, m));
        if ((int)lane == src) a.out[P] = rts_plot_record(r, root, L, t, e, a.nd, a.t0, a.dt, a.pri);
    }
}

int rts_cube_plots_device(RtsContext* c, const RtsPlotParams& p, const RtsDetection* list, const uint32_t* n_dev, uint32_t n_cap, uint32_t n_doppler, uint32_t max_plots)
{
    RtsPlotState& s = c->cube.plot;
    const RtsCubeParams& q = c->cube.params;
    const uint32_t cap = n_cap ? n_cap : 1u;
    RTS_HIP(s.d_key.reserve(cap)); RTS_HIP(s.d_parent.reserve(cap)); RTS_HIP(s.d_idx.reserve(cap)); RTS_HIP(s.d_lab_s.reserve(cap));
    RTS_HIP(s.d_idx_s.reserve(cap)); RTS_HIP(s.d_len.reserve(cap)); RTS_HIP(s.d_flag.reserve((size_t)cap + 1)); RTS_HIP(s.d_off.reserve((size_t)cap + 1));
    RTS_HIP(s.d_list.reserve(max_plots ? max_plots : 1u));
    unsigned bits = 1; while (bits < 32u && (cap >> bits) != 0u) bits++;      // labels and the padding value are at most cap
    size_t tmp_sort = 0, tmp_scan = 0;
    RTS_HIP(rocprim::radix_sort_pairs(nullptr, tmp_sort, s.d_parent.p, s.d_lab_s.p, s.d_idx.p, s.d_idx_s.p, (size_t)cap, 0u, bits, c->stream));
    RTS_HIP(rocprim::exclusive_scan(nullptr, tmp_scan, s.d_flag.p, s.d_off.p, 0u, (size_t)cap + 1, rocprim::plus<uint32_t>(), c->stream));
    RTS_HIP(s.d_tmp.reserve((tmp_sort > tmp_scan ? tmp_sort : tmp_scan) + 1));
    RtsPlotArgs a;
    a.list = list; a.n_dev = n_dev; a.n_cap = n_cap; a.cap = cap;
    a.nd = n_doppler; a.nb = q.n_bins; a.lr = p.link_range; a.ld = p.link_doppler; a.min_cells = p.min_cells ? p.min_cells : 1u; a.max_plots = max_plots;
    a.t0 = q.t0; a.dt = q.dt; a.pri = p.pri;
    a.key = s.d_key.p; a.parent = s.d_parent.p; a.idx = s.d_idx.p; a.lab_s = s.d_lab_s.p; a.idx_s = s.d_idx_s.p; a.len = s.d_len.p;
    a.flag = s.d_flag.p; a.off = s.d_off.p; a.out = s.d_list.p;
    const unsigned grid = (cap + RTS_PLOT_THREADS - 1) / RTS_PLOT_THREADS;
    k_plot_init<<<grid, RTS_PLOT_THREADS, 0, c->stream>>>(a);
    RTS_HIP(hipGetLastError());
    k_plot_link<<<grid, RTS_PLOT_THREADS, 0, c->stream>>>(a);
    RTS_HIP(hipGetLastError());
    k_plot_flatten<<<grid, RTS_PLOT_THREADS, 0, c->stream>>>(a);
    RTS_HIP(hipGetLastError());
    RTS_HIP(rocprim::radix_sort_pairs(s.d_tmp.p, tmp_sort, s.d_parent.p, s.d_lab_s.p, s.d_idx.p, s.d_idx_s.p, (size_t)cap, 0u, bits, c->stream));
    k_plot_flag<<<grid, RTS_PLOT_THREADS, 0, c->stream>>>(a);
    RTS_HIP(hipGetLastError());
    RTS_HIP(rocprim::exclusive_scan(s.d_tmp.p, tmp_scan, s.d_flag.p, s.d_off.p, 0u, (size_t)cap + 1, rocprim::plus<uint32_t>(), c->stream));
    k_plot_reduce<<<grid, RTS_PLOT_THREADS, 0, c->stream>>>(a);
    RTS_HIP(hipGetLastError());
    s.cap = cap; s.max = max_plots; s.valid = true;
    return RTS_OK;
}
