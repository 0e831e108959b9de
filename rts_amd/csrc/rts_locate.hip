// rts_locate.hip -- multistatic localisation on the device (include/rts_amd.h: rts_cube_locate): one frame of per-receiver records to
// targets.  Every rule -- the screen, the closed form, the completion, the refinement, velocity and cost, the resolution's order -- is
// rts_locate.h, shared with the host evaluator rts_locate_eval.  Wave64; the launches are sized by capacities and every kernel reads
// the counts on the device, so the call never waits on the host.
//   1. k_locate_plots         a thread per plot: the four fields the step reads, copied out of the 104-byte records (a record that
//      k_locate_track_flag    takes no part gets a NaN range sum); tracks instead: a flag per (receiver, table slot), an exclusive scan
//      k_locate_track_gather  over the [16][table] flags and a gather, which orders the copy by (rx, table index)
//   2. k_locate_segs          a thread per receiver: its segment of the copy (binary searches on rx)
//   3. k_locate_pairs<false>  a thread per (i, j) pair of the first two anchors' segments, a tile of 16 x 16 pairs per workgroup, the
//                             third anchor's range sums in LDS (8 KiB): the pair screen, then the k loop; per pair the number of
//                             candidates it accepts.  An exclusive scan over the pairs gives every pair its place in the list
//   4. k_locate_pairs<true>   the same walk for the pairs whose count is not zero: the candidates, in ascending candidate index
//   5. k_locate_resolve       ONE workgroup strides over the stored candidates in rounds of locally dominant candidates until none is
//                             live: the loop ends on the device
//   6. k_locate_write         winners -> an exclusive scan -> the targets in ascending candidate index; the counts
// Why the rounds give the greedy set.  The candidates are totally ordered by (16 - K, cost bits, position).  In a round every record
// holds the minimum over the LIVE candidates that name it -- a candidate is live until it wins or one of its records is taken -- and
// a live candidate wins when it holds the minimum at every record it names.  Such a candidate is smaller than every live candidate it
// conflicts with, so the greedy pass reaches it before any of them and finds its records free; and the smallest live candidate of all
// always wins, so every round with a live candidate takes at least one and the rounds end.  The minimum is taken in three order-free
// steps (atomicMin of 16 - K, of the cost's bits among those that hold the first, of the position among those that hold both).  Words
// other threads write with atomics are read and reset with agent-scope atomic loads and stores, never through a stale line of the L1.
#include <cstring>
#include <algorithm>
#include <hip/hip_runtime.h>
#include <rocprim/rocprim.hpp>
#include "rts_internal.h"

#define RTS_LOCATE_THREADS 256
#define RTS_LOCATE_TILE 16u
#define RTS_LOCATE_RESOLVE_THREADS 1024

struct RtsLocateArgs {
    const RtsLocateGeo* geo; double cspeed; uint32_t source, n_rx;
    const RtsPlot* plots; const uint32_t* n_dev; const RtsTrack* tracks; const RtsTrackMeta* tmeta;
    uint32_t rcap, acap;                                       // the records the copy may hold; the positions of an anchor's segment the pair launch covers
    double* zr; double* zf; double* zp; uint32_t* zi; uint32_t* zrx; uint32_t* seg; uint32_t* n;
    uint32_t* tflag; const uint32_t* toff;
    uint32_t* pcnt; const uint32_t* poff;
    RtsTarget* cand; const RtsTarget* cand_in; uint32_t ccap, n_in, icap;      // icap: the record indices the resolution's words cover
    uint32_t* state; uint32_t* taken; uint32_t* best_k; unsigned long long* best_c; uint32_t* best_i;
    uint32_t* win; const uint32_t* woff; RtsTarget* out; uint32_t tmax; RtsLocateMeta* meta;
};

__device__ __forceinline__ uint32_t rts_locate_ld(const uint32_t* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void rts_locate_st(uint32_t* p, uint32_t v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ unsigned long long rts_locate_ld(const unsigned long long* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void rts_locate_st(unsigned long long* p, unsigned long long v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

__global__ void __launch_bounds__(RTS_LOCATE_THREADS) k_locate_plots(const RtsLocateArgs a)
{
    const uint32_t e = blockIdx.x * RTS_LOCATE_THREADS + threadIdx.x;
    uint32_t n = a.rcap;
    if (a.n_dev) { const uint32_t have = *a.n_dev; if (have < n) n = have; }
    if (e == 0u) *a.n = n;
    if (e >= n) return;
    const RtsPlot& z = a.plots[e];
    a.zr[e] = rts_locate_range_sum(a.cspeed, z.delay, z.doppler, z.power_sum); a.zf[e] = z.doppler; a.zp[e] = z.power_sum; a.zi[e] = e; a.zrx[e] = z.rx;
}

// element m * rcap + i: track i takes part and stands at receiver m (element 16 rcap, the scan's extra one: 0)
__global__ void __launch_bounds__(RTS_LOCATE_THREADS) k_locate_track_flag(const RtsLocateArgs a)
{
    const uint32_t e = blockIdx.x * RTS_LOCATE_THREADS + threadIdx.x;
    if (e > RTS_LOCATE_MAX_RX * a.rcap) return;
    const uint32_t m = e / a.rcap, i = e % a.rcap, n = a.tmeta->n < a.rcap ? a.tmeta->n : a.rcap;
    uint32_t f = 0u;
    if (m < RTS_LOCATE_MAX_RX && i < n) { const RtsTrack& t = a.tracks[i]; f = t.rx == m && rts_locate_track_counts(t.flags, t.rx, a.n_rx) ? 1u : 0u; }
    a.tflag[e] = f;
}
__global__ void __launch_bounds__(RTS_LOCATE_THREADS) k_locate_track_gather(const RtsLocateArgs a)
{
    const uint32_t e = blockIdx.x * RTS_LOCATE_THREADS + threadIdx.x;
    if (e == 0u) *a.n = a.toff[RTS_LOCATE_MAX_RX * a.rcap];
    if (e >= RTS_LOCATE_MAX_RX * a.rcap || a.tflag[e] == 0u) return;
    const uint32_t m = e / a.rcap, i = e % a.rcap, pos = a.toff[e];         // (pos < rcap: a track is flagged at one receiver)
    const RtsTrack& t = a.tracks[i];
    a.zr[pos] = rts_locate_range_sum(a.cspeed, t.delay, t.doppler, t.power_sum); a.zf[pos] = t.doppler; a.zp[pos] = t.power_sum; a.zi[pos] = i; a.zrx[pos] = m;
}

__global__ void __launch_bounds__(64) k_locate_segs(const RtsLocateArgs a)
{
    const uint32_t m = threadIdx.x;
    if (m >= RTS_LOCATE_MAX_RX) return;
    const uint32_t n = *a.n;
    uint32_t b[2] = {0u, 0u};
    if (m < a.n_rx) for (uint32_t above = 0; above < 2u; above++) {
        uint32_t lo = 0, hi = n;
        while (lo < hi) { const uint32_t mid = lo + (hi - lo) / 2u; const uint32_t v = a.zrx[mid]; if (above ? v <= m : v < m) lo = mid + 1u; else hi = mid; }
        b[above] = lo;
    }
    a.seg[2u * m] = b[0]; a.seg[2u * m + 1u] = b[1];
}

// A thread per (i, j) pair, 16 x 16 pairs per workgroup; the third anchor's range sums in LDS.  Counting: pcnt[i acap + j] (the
// launch zeroed the array, so the pairs beyond the segments count 0).  Writing: the pair's candidates from cand[poff], while the
// list has room; a tile without a candidate returns before it stages anything.
template <bool WRITE> __global__ void __launch_bounds__(RTS_LOCATE_THREADS) k_locate_pairs(const RtsLocateArgs a)
{
    __shared__ double s_r2[RTS_LOCATE_MAX_PER_RX];
    const RtsLocateGeo& g = *a.geo;
    const RtsLocateList z = {a.zr, a.zf, a.zp, a.zi, a.seg};
    uint32_t P[3];
    for (int q = 0; q < 3; q++) P[q] = rts_locate_anchor_count(a.seg[2u * g.anchors[q]], a.seg[2u * g.anchors[q] + 1u]);
    const uint32_t i = blockIdx.y * RTS_LOCATE_TILE + threadIdx.x / RTS_LOCATE_TILE, j = blockIdx.x * RTS_LOCATE_TILE + threadIdx.x % RTS_LOCATE_TILE;
    if (blockIdx.y * RTS_LOCATE_TILE >= P[0] || blockIdx.x * RTS_LOCATE_TILE >= P[1]) return;      // (the whole workgroup)
    const bool mine = i < P[0] && j < P[1];
    const size_t at = (size_t)i * a.acap + j;
    uint32_t cnt = 0u;
    if (WRITE) {
        if (mine) cnt = a.pcnt[at];
        if (!__syncthreads_or(cnt != 0u)) return;
    }
    const uint32_t first2 = a.seg[2u * g.anchors[2]];
    for (uint32_t k = threadIdx.x; k < P[2]; k += RTS_LOCATE_THREADS) s_r2[k] = a.zr[first2 + k];
    __syncthreads();
    if (!mine) return;
    if (!WRITE) a.pcnt[at] = rts_locate_pair(g, z, i, j, s_r2, P[1], P[2], nullptr, 0u);
    else if (cnt != 0u) {
        const uint32_t pos = a.poff[at];
        if (pos < a.ccap) rts_locate_pair(g, z, i, j, s_r2, P[1], P[2], a.cand + pos, a.ccap - pos);
    }
}

__device__ __forceinline__ uint32_t rts_locate_stored(const RtsLocateArgs& a)
{
    if (a.source == RTS_LOCATE_FROM_CANDIDATES) return a.n_in < a.ccap ? a.n_in : a.ccap;
    const uint32_t total = a.poff[(size_t)a.acap * a.acap];
    return total < a.ccap ? total : a.ccap;
}

__global__ void __launch_bounds__(RTS_LOCATE_RESOLVE_THREADS) k_locate_resolve(const RtsLocateArgs a)
{
    __shared__ uint32_t s_active[2];
    const uint32_t nC = rts_locate_stored(a), tid = threadIdx.x;
    const RtsTarget* C = a.source == RTS_LOCATE_FROM_CANDIDATES ? a.cand_in : a.cand;
    if (tid < 2u) s_active[tid] = 0u;
    // every record a candidate names is free
    for (uint32_t c = tid; c < nC; c += RTS_LOCATE_RESOLVE_THREADS) {
        a.state[c] = 0u;
        for (uint32_t m = 0; m < RTS_LOCATE_MAX_RX; m++) { const uint32_t e = C[c].plot[m]; if (e < a.icap) rts_locate_st(a.taken + e, 0u); }
    }
    __syncthreads();
    uint32_t round = 0;
    for (;; round++) {
        // a live candidate with a taken record is out; the minima of the records the others name are reset ...
        for (uint32_t c = tid; c < nC; c += RTS_LOCATE_RESOLVE_THREADS) {
            if (a.state[c] != 0u) continue;
            bool out = false;
            for (uint32_t m = 0; m < RTS_LOCATE_MAX_RX; m++) { const uint32_t e = C[c].plot[m]; if (e < a.icap && rts_locate_ld(a.taken + e) != 0u) out = true; }
            if (out) { a.state[c] = 2u; continue; }
            for (uint32_t m = 0; m < RTS_LOCATE_MAX_RX; m++) {
                const uint32_t e = C[c].plot[m];
                if (e < a.icap) { rts_locate_st(a.best_k + e, 0xffffffffu); rts_locate_st(a.best_c + e, ~0ull); rts_locate_st(a.best_i + e, 0xffffffffu); }
            }
        }
        __syncthreads();
        if (tid == 0u) s_active[(round + 1u) & 1u] = 0u;                 // (last read before this round's first barrier)
        // ... every record takes the smallest 16 - K over the live candidates that name it ...
        for (uint32_t c = tid; c < nC; c += RTS_LOCATE_RESOLVE_THREADS) {
            if (a.state[c] != 0u) continue;
            const uint32_t kk = rts_locate_key_k(C[c]);
            for (uint32_t m = 0; m < RTS_LOCATE_MAX_RX; m++) { const uint32_t e = C[c].plot[m]; if (e < a.icap) atomicMin(a.best_k + e, kk); }
        }
        __syncthreads();
        // ... among those that hold it the smallest cost ...
        for (uint32_t c = tid; c < nC; c += RTS_LOCATE_RESOLVE_THREADS) {
            if (a.state[c] != 0u) continue;
            const uint32_t kk = rts_locate_key_k(C[c]); const unsigned long long cc = rts_locate_key_cost(C[c]);
            for (uint32_t m = 0; m < RTS_LOCATE_MAX_RX; m++) { const uint32_t e = C[c].plot[m]; if (e < a.icap && rts_locate_ld(a.best_k + e) == kk) atomicMin(a.best_c + e, cc); }
        }
        __syncthreads();
        // ... and among those that hold both the smallest position
        for (uint32_t c = tid; c < nC; c += RTS_LOCATE_RESOLVE_THREADS) {
            if (a.state[c] != 0u) continue;
            const uint32_t kk = rts_locate_key_k(C[c]); const unsigned long long cc = rts_locate_key_cost(C[c]);
            for (uint32_t m = 0; m < RTS_LOCATE_MAX_RX; m++) {
                const uint32_t e = C[c].plot[m];
                if (e < a.icap && rts_locate_ld(a.best_k + e) == kk && rts_locate_ld(a.best_c + e) == cc) atomicMin(a.best_i + e, c);
            }
        }
        __syncthreads();
        // a live candidate wins when every record it names holds it (the records are taken after the barrier)
        for (uint32_t c = tid; c < nC; c += RTS_LOCATE_RESOLVE_THREADS) {
            if (a.state[c] != 0u) continue;
            s_active[round & 1u] = 1u;
            const uint32_t kk = rts_locate_key_k(C[c]); const unsigned long long cc = rts_locate_key_cost(C[c]);
            bool wins = true;
            for (uint32_t m = 0; m < RTS_LOCATE_MAX_RX; m++) {
                const uint32_t e = C[c].plot[m];
                if (e < a.icap && !(rts_locate_ld(a.best_k + e) == kk && rts_locate_ld(a.best_c + e) == cc && rts_locate_ld(a.best_i + e) == c)) wins = false;
            }
            if (wins) a.state[c] = 3u;
        }
        __syncthreads();
        for (uint32_t c = tid; c < nC; c += RTS_LOCATE_RESOLVE_THREADS) {
            if (a.state[c] != 3u) continue;
            for (uint32_t m = 0; m < RTS_LOCATE_MAX_RX; m++) { const uint32_t e = C[c].plot[m]; if (e < a.icap) rts_locate_st(a.taken + e, 1u); }
            a.state[c] = 1u;
        }
        __syncthreads();
        if (s_active[round & 1u] == 0u) break;                           // (workgroup-uniform: written before the last barrier but one)
    }
    for (uint32_t c = tid; c <= a.ccap; c += RTS_LOCATE_RESOLVE_THREADS) a.win[c] = c < nC && a.state[c] == 1u ? 1u : 0u;      // (element ccap, the scan's extra one: 0)
    if (tid == 0u) a.meta->rounds = round;                               // rounds that found a live candidate
}

__global__ void __launch_bounds__(RTS_LOCATE_THREADS) k_locate_write(const RtsLocateArgs a)
{
    const uint32_t e = blockIdx.x * RTS_LOCATE_THREADS + threadIdx.x;
    if (e == 0u) {
        uint32_t cut = 0u;
        if (a.source != RTS_LOCATE_FROM_CANDIDATES) for (int q = 0; q < 3; q++) { const uint32_t m = a.geo->anchors[q]; if (a.seg[2u * m + 1u] - a.seg[2u * m] > RTS_LOCATE_MAX_PER_RX) cut = 1u; }
        a.meta->cand_total = a.source == RTS_LOCATE_FROM_CANDIDATES ? a.n_in : a.poff[(size_t)a.acap * a.acap];
        a.meta->cand_stored = rts_locate_stored(a); a.meta->targets_total = a.woff[a.ccap]; a.meta->seg_cut = cut;
        a.meta->reserved[0] = 0u; a.meta->reserved[1] = 0u; a.meta->reserved[2] = 0u;
    }
    if (e >= a.ccap || a.win[e] == 0u) return;
    const uint32_t pos = a.woff[e];
    if (pos < a.tmax) a.out[pos] = (a.source == RTS_LOCATE_FROM_CANDIDATES ? a.cand_in : a.cand)[e];
}

// geo: the call's constants on the device (null with RTS_LOCATE_FROM_CANDIDATES); list, n_dev, rcap: the source's records, where
// their count stands on the device (null: all rcap count) and how many there can be (plots: RtsPlot; tracks: the table cur and its
// RtsTrackMeta; candidates: RtsTarget)
int rts_cube_locate_device(RtsContext* c, const RtsLocateParams& p, const RtsLocateGeo* geo, const void* list, const void* n_dev, uint32_t rcap, uint32_t max_c, uint32_t max_t)
{
    RtsLocateState& s = c->cube.locate;
    const bool from_cand = p.source == RTS_LOCATE_FROM_CANDIDATES, from_tracks = p.source == RTS_LOCATE_FROM_TRACKS;
    const uint32_t rcap1 = from_cand ? 1u : (rcap ? rcap : 1u), acap = rcap1 < RTS_LOCATE_MAX_PER_RX ? rcap1 : RTS_LOCATE_MAX_PER_RX;
    const uint32_t icap = from_cand ? RTS_LOCATE_MAX_INDEX : rcap1;
    const size_t n_pairs = (size_t)acap * acap + 1, n_flags = from_tracks ? (size_t)RTS_LOCATE_MAX_RX * rcap1 + 1 : 1, n_win = (size_t)max_c + 1;
    RTS_HIP(s.d_zr.reserve(rcap1)); RTS_HIP(s.d_zf.reserve(rcap1)); RTS_HIP(s.d_zp.reserve(rcap1)); RTS_HIP(s.d_zi.reserve(rcap1)); RTS_HIP(s.d_zrx.reserve(rcap1));
    RTS_HIP(s.d_seg.reserve(2u * RTS_LOCATE_MAX_RX)); RTS_HIP(s.d_n.reserve(1)); RTS_HIP(s.d_tflag.reserve(n_flags)); RTS_HIP(s.d_toff.reserve(n_flags));
    RTS_HIP(s.d_pcnt.reserve(n_pairs)); RTS_HIP(s.d_poff.reserve(n_pairs)); RTS_HIP(s.d_cand.reserve(from_cand ? 1u : max_c)); RTS_HIP(s.d_state.reserve(max_c));
    RTS_HIP(s.d_taken.reserve(icap)); RTS_HIP(s.d_best_k.reserve(icap)); RTS_HIP(s.d_best_c.reserve(icap)); RTS_HIP(s.d_best_i.reserve(icap));
    RTS_HIP(s.d_win.reserve(n_win)); RTS_HIP(s.d_woff.reserve(n_win)); RTS_HIP(s.d_out.reserve(max_t)); RTS_HIP(s.d_meta.reserve(1));
    size_t tmp_pairs = 0, tmp_flags = 0, tmp_win = 0;
    RTS_HIP(rocprim::exclusive_scan(nullptr, tmp_pairs, s.d_pcnt.p, s.d_poff.p, 0u, n_pairs, rocprim::plus<uint32_t>(), c->stream));
    RTS_HIP(rocprim::exclusive_scan(nullptr, tmp_flags, s.d_tflag.p, s.d_toff.p, 0u, n_flags, rocprim::plus<uint32_t>(), c->stream));
    RTS_HIP(rocprim::exclusive_scan(nullptr, tmp_win, s.d_win.p, s.d_woff.p, 0u, n_win, rocprim::plus<uint32_t>(), c->stream));
    RTS_HIP(s.d_tmp.reserve(std::max(tmp_pairs, std::max(tmp_flags, tmp_win)) + 1));
    RtsLocateArgs a = {};
    a.geo = geo; a.cspeed = p.cspeed; a.source = p.source; a.n_rx = p.n_rx; a.rcap = rcap1; a.acap = acap;
    a.zr = s.d_zr.p; a.zf = s.d_zf.p; a.zp = s.d_zp.p; a.zi = s.d_zi.p; a.zrx = s.d_zrx.p; a.seg = s.d_seg.p; a.n = s.d_n.p;
    a.tflag = s.d_tflag.p; a.toff = s.d_toff.p; a.pcnt = s.d_pcnt.p; a.poff = s.d_poff.p;
    a.cand = s.d_cand.p; a.ccap = max_c; a.icap = icap; a.state = s.d_state.p; a.taken = s.d_taken.p; a.best_k = s.d_best_k.p;
    a.best_c = (unsigned long long*)s.d_best_c.p; a.best_i = s.d_best_i.p; a.win = s.d_win.p; a.woff = s.d_woff.p; a.out = s.d_out.p; a.tmax = max_t; a.meta = s.d_meta.p;
    if (from_cand) { a.cand_in = (const RtsTarget*)list; a.n_in = rcap; }
    else {
        if (from_tracks) {
            a.tracks = (const RtsTrack*)list; a.tmeta = (const RtsTrackMeta*)n_dev;
            const unsigned grid = (unsigned)((n_flags + RTS_LOCATE_THREADS - 1) / RTS_LOCATE_THREADS);
            k_locate_track_flag<<<grid, RTS_LOCATE_THREADS, 0, c->stream>>>(a);
            RTS_HIP(hipGetLastError());
            RTS_HIP(rocprim::exclusive_scan(s.d_tmp.p, tmp_flags, s.d_tflag.p, s.d_toff.p, 0u, n_flags, rocprim::plus<uint32_t>(), c->stream));
            k_locate_track_gather<<<grid, RTS_LOCATE_THREADS, 0, c->stream>>>(a);
            RTS_HIP(hipGetLastError());
        } else {
            a.plots = (const RtsPlot*)list; a.n_dev = (const uint32_t*)n_dev; if (rcap == 0u) a.n_dev = nullptr, a.rcap = 0u;
            k_locate_plots<<<(rcap1 + RTS_LOCATE_THREADS - 1) / RTS_LOCATE_THREADS, RTS_LOCATE_THREADS, 0, c->stream>>>(a);
            RTS_HIP(hipGetLastError());
            a.rcap = rcap1;
        }
        k_locate_segs<<<1, 64, 0, c->stream>>>(a);
        RTS_HIP(hipGetLastError());
        RTS_HIP(hipMemsetAsync(s.d_pcnt.p, 0, sizeof(uint32_t) * n_pairs, c->stream));
        const unsigned tiles = (acap + RTS_LOCATE_TILE - 1u) / RTS_LOCATE_TILE;
        k_locate_pairs<false><<<dim3(tiles, tiles), RTS_LOCATE_THREADS, 0, c->stream>>>(a);
        RTS_HIP(hipGetLastError());
        RTS_HIP(rocprim::exclusive_scan(s.d_tmp.p, tmp_pairs, s.d_pcnt.p, s.d_poff.p, 0u, n_pairs, rocprim::plus<uint32_t>(), c->stream));
        k_locate_pairs<true><<<dim3(tiles, tiles), RTS_LOCATE_THREADS, 0, c->stream>>>(a);
        RTS_HIP(hipGetLastError());
    }
    k_locate_resolve<<<1, RTS_LOCATE_RESOLVE_THREADS, 0, c->stream>>>(a);
    RTS_HIP(hipGetLastError());
    RTS_HIP(rocprim::exclusive_scan(s.d_tmp.p, tmp_win, s.d_win.p, s.d_woff.p, 0u, n_win, rocprim::plus<uint32_t>(), c->stream));
    k_locate_write<<<(unsigned)((n_win + RTS_LOCATE_THREADS - 1) / RTS_LOCATE_THREADS), RTS_LOCATE_THREADS, 0, c->stream>>>(a);
    RTS_HIP(hipGetLastError());
    return RTS_OK;
}
