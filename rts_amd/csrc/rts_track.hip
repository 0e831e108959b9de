// rts_track.hip -- the tracker step on the device (include/rts_amd.h: rts_cube_track): one frame of plots against the handle's track
// table.  Every rule -- prediction, d2, the edge, the candidate order, update, coast, start, lifecycle -- is rts_track.h, shared with
// the host evaluator rts_tracks_eval.  Wave64; the launches are sized by the table and the plot list's capacity and every kernel
// reads the counts on the device, so the call never waits on the host.
//   1. k_track_prep    a thread per track: the prediction, S and its determinant; a thread per plot: the four fields the step reads,
//                      copied out of the 104-byte records (the step does not refer to the plot buffers afterwards)
//   2. k_track_gate    a wave per track, 16 tracks per workgroup: the workgroup finds the part of the plot list its tracks'
//                      receivers span (binary searches on rx), stages it in LDS 256 plots at a time, and every wave tests the
//                      staged plots of its track's receiver 64 at a time with the full expression and keeps the K best in
//                      ascending (d2, plot index)
//   3. k_track_match   ONE workgroup strides over the tracks in rounds of locally dominant edges until no free track has a free
//                      candidate: the loop ends on the device
//   4. k_track_flag    survivors and unmatched finite plots -> flags; an exclusive scan over [tracks | plots | 1] gives every
//                      record its position: survivors in their order, then the new tracks in ascending plot index
//   5. k_track_write   update, coast and start into the OTHER table; the new count, total and next id
// Why the rounds give the greedy matching.  Edges are totally ordered by (d2, track, plot).  In a round every free plot holds the
// minimum (d2, track) over ALL kept edges to it from free tracks, and a free track is matched when its first free candidate's
// minimum is itself.  Such an edge is smaller than every other free edge at either end, so the greedy pass takes it before any of
// them; and the smallest free edge of all is always one, so every round matches at least one pair and the rounds end after at most
// min(tracks, plots).  The minimum is taken in two order-free steps: atomicMin on the bits of d2 (non-negative doubles order as
// unsigned integers), then atomicMin of the track index among the edges that hold that d2.  Words other threads write with atomics
// are read and reset with agent-scope atomic loads and stores, never through a stale line of the L1.
#include <cstring>
#include <hip/hip_runtime.h>
#include <rocprim/rocprim.hpp>
#include "rts_internal.h"

#define RTS_TRACK_THREADS 256
#define RTS_TRACK_MATCH_THREADS 1024

struct RtsTrackArgs {
    RtsTrackParams p; double T;
    const RtsPlot* list; const uint32_t* n_dev; uint32_t pcap, tcap;              // the list's capacity; the table's size
    const RtsTrack* in; RtsTrack* out; const RtsTrackMeta* meta_in; RtsTrackMeta* meta_out;
    RtsTrackPred* pred; double* zd; double* zf; double* pw; uint32_t* zrx;
    double* cd; uint32_t* cj; uint32_t* cn;                                       // candidates: entry k of track i at [k * tcap + i]
    uint32_t* of_track; uint32_t* of_plot; double* md2; unsigned long long* best_d; uint32_t* best_t; uint32_t* rounds;
    uint32_t* flag; const uint32_t* off;
};

__device__ __forceinline__ uint32_t rts_track_n_plots(const RtsTrackArgs& a)
{
    if (!a.n_dev) return a.pcap;
    const uint32_t n = *a.n_dev;
    return n < a.pcap ? n : a.pcap;
}
__device__ __forceinline__ uint32_t rts_track_n_tracks(const RtsTrackArgs& a) { const uint32_t n = a.meta_in->n; return n < a.tcap ? n : a.tcap; }

__device__ __forceinline__ uint32_t rts_track_ld(const uint32_t* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void rts_track_st(uint32_t* p, uint32_t v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ unsigned long long rts_track_ld(const unsigned long long* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void rts_track_st(unsigned long long* p, unsigned long long v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

__global__ void __launch_bounds__(RTS_TRACK_THREADS) k_track_prep(const RtsTrackArgs a)
{
    const uint32_t e = blockIdx.x * RTS_TRACK_THREADS + threadIdx.x;
    if (e < rts_track_n_tracks(a)) { a.pred[e] = rts_track_predict(a.in[e], a.p, a.T); a.cn[e] = 0u; a.of_track[e] = RTS_TRACK_NONE; a.md2[e] = 0.0; }
    if (e < rts_track_n_plots(a)) {
        const RtsPlot& z = a.list[e];
        a.zd[e] = z.delay; a.zf[e] = z.doppler; a.pw[e] = z.power_sum; a.zrx[e] = z.rx; a.of_plot[e] = RTS_TRACK_NONE;
    }
    if (e == 0u) *a.rounds = 0u;
}

// the first index in [0, n) with rx[index] >= want (above: > want); n when there is none
__device__ __forceinline__ uint32_t rts_track_bound(const uint32_t* rx, uint32_t n, uint32_t want, bool above)
{
    uint32_t lo = 0, hi = n;
    while (lo < hi) { const uint32_t mid = lo + (hi - lo) / 2u; const uint32_t v = rx[mid]; if (above ? v <= want : v < want) lo = mid + 1u; else hi = mid; }
    return lo;
}

// A WAVE per track.  A workgroup of four waves takes 16 consecutive tracks, four per wave, finds the part of the plot list their
// receivers span (binary searches on rx; the tracks of a table are in no receiver order, so this can be the whole list) and stages
// it in LDS 256 plots at a time; per staged chunk and track the wave tests 64 plots at a time, a lane each, with the full
// expression, and the gated ones enter the track's list one after the other in ascending plot index.  The list lives in the wave:
// lane k holds entry k; an insertion counts the entries before the new one (a ballot), shifts the rest up a lane and drops the
// last.  The list ends as the K smallest (d2, plot index) of all that were offered -- what rts_track_cand_insert leaves in the
// evaluator.  (A thread per track, 256 tracks per workgroup, each thread walking the staged plots alone, was measured and lost at
// every size: profiles/track_bench.txt.)
#define RTS_TRACK_WAVE_TRACKS 4u
#define RTS_TRACK_WAVE_BLOCK (RTS_TRACK_WAVE_TRACKS * (RTS_TRACK_THREADS / 64u))
__global__ void __launch_bounds__(RTS_TRACK_THREADS) k_track_gate(const RtsTrackArgs a)
{
    __shared__ double s_zd[RTS_TRACK_THREADS], s_zf[RTS_TRACK_THREADS];
    __shared__ uint32_t s_rx[RTS_TRACK_THREADS], s_span[2];
    const uint32_t nT = rts_track_n_tracks(a), nP = rts_track_n_plots(a), b0 = blockIdx.x * RTS_TRACK_WAVE_BLOCK;
    if (b0 >= nT) return;                                                // (the whole workgroup)
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6, K = a.p.max_candidates;
    if (threadIdx.x == 0) { s_span[0] = 0xffffffffu; s_span[1] = 0u; }
    __syncthreads();
    if (threadIdx.x < RTS_TRACK_WAVE_BLOCK && b0 + threadIdx.x < nT) {
        const uint32_t rx = a.in[b0 + threadIdx.x].rx;
        const uint32_t lo = rts_track_bound(a.zrx, nP, rx, false), hi = rts_track_bound(a.zrx, nP, rx, true);
        if (lo < hi) { atomicMin(&s_span[0], lo); atomicMax(&s_span[1], hi); }
    }
    __syncthreads();
    const uint32_t first = s_span[0], end = s_span[1];
    RtsTrackPred r[RTS_TRACK_WAVE_TRACKS]; uint32_t rx[RTS_TRACK_WAVE_TRACKS], n[RTS_TRACK_WAVE_TRACKS], e_j[RTS_TRACK_WAVE_TRACKS]; double e_d2[RTS_TRACK_WAVE_TRACKS];
    bool live[RTS_TRACK_WAVE_TRACKS];
#pragma unroll
    for (uint32_t q = 0; q < RTS_TRACK_WAVE_TRACKS; q++) {
        const uint32_t i = b0 + wave * RTS_TRACK_WAVE_TRACKS + q;
        live[q] = i < nT; n[q] = 0u; e_j[q] = 0u; e_d2[q] = 0.0; rx[q] = 0u; r[q] = RtsTrackPred{};
        if (live[q]) { r[q] = a.pred[i]; rx[q] = a.in[i].rx; }
    }
    for (uint32_t base = first; base < end; base += RTS_TRACK_THREADS) { // (workgroup-uniform)
        const uint32_t m = base + threadIdx.x;
        if (m < end) { s_zd[threadIdx.x] = a.zd[m]; s_zf[threadIdx.x] = a.zf[m]; s_rx[threadIdx.x] = a.zrx[m]; }
        __syncthreads();
        const uint32_t cnt = end - base < RTS_TRACK_THREADS ? end - base : RTS_TRACK_THREADS;
#pragma unroll
        for (uint32_t q = 0; q < RTS_TRACK_WAVE_TRACKS; q++) {
            if (!live[q]) continue;                                      // (wave-uniform)
            for (uint32_t sub = 0; sub < cnt; sub += 64u) {
                const uint32_t k = sub + lane;
                double d2 = 0.0;
                bool hit = false;
                if (k < cnt && s_rx[k] == rx[q] && rts_track_plot_finite(s_zd[k], s_zf[k])) hit = rts_track_edge(r[q], s_zd[k], s_zf[k], a.p.doppler_period, a.p.gate, &d2);
                for (unsigned long long rest = __ballot(hit); rest != 0ull; rest &= rest - 1ull) {
                    const int src = __ffsll((long long)rest) - 1;
                    const double x = __shfl(d2, src);
                    const uint32_t jx = base + sub + (uint32_t)src;
                    const uint32_t pos = (uint32_t)__popcll(__ballot(lane < n[q] && rts_track_cand_before(e_d2[q], e_j[q], x, jx)));
                    if (pos >= K) continue;                              // (wave-uniform)
                    const double up_d2 = __shfl_up(e_d2[q], 1); const uint32_t up_j = __shfl_up(e_j[q], 1);
                    if (lane == pos) { e_d2[q] = x; e_j[q] = jx; }
                    else if (lane > pos && lane <= n[q] && lane < K) { e_d2[q] = up_d2; e_j[q] = up_j; }
                    if (n[q] < K) n[q]++;
                }
            }
        }
        __syncthreads();
    }
#pragma unroll
    for (uint32_t q = 0; q < RTS_TRACK_WAVE_TRACKS; q++) {
        const uint32_t i = b0 + wave * RTS_TRACK_WAVE_TRACKS + q;
        if (!live[q]) continue;
        if (lane < n[q]) { a.cd[(size_t)lane * a.tcap + i] = e_d2[q]; a.cj[(size_t)lane * a.tcap + i] = e_j[q]; }
        if (lane == 0u) a.cn[i] = n[q];
    }
}

__global__ void __launch_bounds__(RTS_TRACK_MATCH_THREADS) k_track_match(const RtsTrackArgs a)
{
    __shared__ uint32_t s_active[2];
    const uint32_t nT = rts_track_n_tracks(a), tid = threadIdx.x;
    if (tid < 2u) s_active[tid] = 0u;
    __syncthreads();
    uint32_t round = 0;
    for (;; round++) {
        // the minima of the plots this round can reach are reset ...
        for (uint32_t i = tid; i < nT; i += RTS_TRACK_MATCH_THREADS) {
            if (a.of_track[i] != RTS_TRACK_NONE) continue;
            const uint32_t n = a.cn[i];
            for (uint32_t k = 0; k < n; k++) {
                const uint32_t j = a.cj[(size_t)k * a.tcap + i];
                if (rts_track_ld(a.of_plot + j) == RTS_TRACK_NONE) { rts_track_st(a.best_d + j, ~0ull); rts_track_st(a.best_t + j, RTS_TRACK_NONE); }
            }
        }
        __syncthreads();
        if (tid == 0u) s_active[(round + 1u) & 1u] = 0u;                 // (last read before this round's first barrier)
        // ... every free plot takes the smallest d2 over all kept edges from free tracks ...
        for (uint32_t i = tid; i < nT; i += RTS_TRACK_MATCH_THREADS) {
            if (a.of_track[i] != RTS_TRACK_NONE) continue;
            const uint32_t n = a.cn[i];
            for (uint32_t k = 0; k < n; k++) {
                const uint32_t j = a.cj[(size_t)k * a.tcap + i];
                if (rts_track_ld(a.of_plot + j) == RTS_TRACK_NONE) atomicMin(a.best_d + j, (unsigned long long)__double_as_longlong(a.cd[(size_t)k * a.tcap + i]));
            }
        }
        __syncthreads();
        // ... and among the edges that hold it the smallest track index
        for (uint32_t i = tid; i < nT; i += RTS_TRACK_MATCH_THREADS) {
            if (a.of_track[i] != RTS_TRACK_NONE) continue;
            const uint32_t n = a.cn[i];
            for (uint32_t k = 0; k < n; k++) {
                const uint32_t j = a.cj[(size_t)k * a.tcap + i];
                if (rts_track_ld(a.of_plot + j) == RTS_TRACK_NONE && rts_track_ld(a.best_d + j) == (unsigned long long)__double_as_longlong(a.cd[(size_t)k * a.tcap + i])) atomicMin(a.best_t + j, i);
            }
        }
        __syncthreads();
        // a free track is matched when its first free candidate's minimum is itself (the plot's word is written after the barrier:
        // this pass still reads which plots were free when the round began)
        for (uint32_t i = tid; i < nT; i += RTS_TRACK_MATCH_THREADS) {
            if (a.of_track[i] != RTS_TRACK_NONE) continue;
            const uint32_t n = a.cn[i];
            for (uint32_t k = 0; k < n; k++) {
                const uint32_t j = a.cj[(size_t)k * a.tcap + i];
                if (rts_track_ld(a.of_plot + j) != RTS_TRACK_NONE) continue;
                const double d2 = a.cd[(size_t)k * a.tcap + i];
                s_active[round & 1u] = 1u;
                if (rts_track_ld(a.best_d + j) == (unsigned long long)__double_as_longlong(d2) && rts_track_ld(a.best_t + j) == i) { a.of_track[i] = j; a.md2[i] = d2; }
                break;
            }
        }
        __syncthreads();
        for (uint32_t i = tid; i < nT; i += RTS_TRACK_MATCH_THREADS) {
            const uint32_t j = a.of_track[i];
            if (j != RTS_TRACK_NONE && rts_track_ld(a.of_plot + j) != i) rts_track_st(a.of_plot + j, i);
        }
        __syncthreads();
        if (s_active[round & 1u] == 0u) break;                           // (workgroup-uniform: written before the last barrier but one)
    }
    if (tid == 0u) *a.rounds = round;                                    // rounds that found a free edge
}

__global__ void __launch_bounds__(RTS_TRACK_THREADS) k_track_flag(const RtsTrackArgs a)
{
    const uint32_t e = blockIdx.x * RTS_TRACK_THREADS + threadIdx.x;
    if (e > a.tcap + a.pcap) return;
    uint32_t f = 0;
    if (e < a.tcap) {
        if (e < rts_track_n_tracks(a)) {
            const RtsTrack& t = a.in[e];
            f = a.of_track[e] != RTS_TRACK_NONE || !(t.misses + 1u > ((t.flags & RTS_TRACK_CONFIRMED) ? a.p.max_misses : a.p.tentative_misses)) ? 1u : 0u;
        }
    } else if (e < a.tcap + a.pcap) {
        const uint32_t j = e - a.tcap;
        if (j < rts_track_n_plots(a)) f = a.of_plot[j] == RTS_TRACK_NONE && rts_track_plot_finite(a.zd[j], a.zf[j]) ? 1u : 0u;
    }
    a.flag[e] = f;                                                       // (element tcap + pcap, the scan's extra one: 0)
}

__global__ void __launch_bounds__(RTS_TRACK_THREADS) k_track_write(const RtsTrackArgs a)
{
    const uint32_t e = blockIdx.x * RTS_TRACK_THREADS + threadIdx.x;
    const uint32_t survivors = a.off[a.tcap], total = a.off[a.tcap + a.pcap], stored = total < a.tcap ? total : a.tcap;
    if (e == 0u) { RtsTrackMeta m; m.next_id = a.meta_in->next_id + (stored - survivors); m.n = stored; m.total = total; m.rounds = *a.rounds; m.reserved = 0u; *a.meta_out = m; }
    if (e >= a.tcap + a.pcap || a.flag[e] == 0u) return;
    const uint32_t pos = a.off[e];
    if (pos >= a.tcap) return;
    if (e < a.tcap) {
        const uint32_t j = a.of_track[e];
        bool keep;
        a.out[pos] = j != RTS_TRACK_NONE ? rts_track_update(a.in[e], a.pred[e], a.p, j, a.zd[j], a.zf[j], a.pw[j], a.md2[e]) : rts_track_coast(a.in[e], a.pred[e], a.p, &keep);
    } else {
        const uint32_t j = e - a.tcap;
        a.out[pos] = rts_track_start(a.p, a.meta_in->next_id + (pos - survivors), j, a.zrx[j], a.zd[j], a.zf[j], a.pw[j]);
    }
}

// the table's buffers: both tables hold RTS_TRACK_MAX_TRACKS records from the start (a DevBuf that grows drops what it held)
int rts_cube_track_tables(RtsContext* c)
{
    RtsTrackState& s = c->cube.track;
    if (s.d_meta.p) return RTS_OK;
    RTS_HIP(s.d_tab[0].reserve(RTS_TRACK_MAX_TRACKS)); RTS_HIP(s.d_tab[1].reserve(RTS_TRACK_MAX_TRACKS));
    RTS_HIP(s.d_meta.reserve(2));
    RTS_HIP(hipMemsetAsync(s.d_meta.p, 0, 2 * sizeof(RtsTrackMeta), c->stream));
    s.cur = 0;
    return RTS_OK;
}

int rts_cube_track_device(RtsContext* c, const RtsTrackParams& p, double T, const RtsPlot* list, const uint32_t* n_dev, uint32_t pcap, uint32_t tcap)
{
    RtsTrackState& s = c->cube.track;
    RTS_TRY(rts_cube_track_tables(c));
    const uint32_t pcap1 = pcap ? pcap : 1u;
    const size_t n_scan = (size_t)tcap + pcap + 1;
    RTS_HIP(s.d_pred.reserve(tcap)); RTS_HIP(s.d_cd.reserve((size_t)tcap * RTS_TRACK_MAX_CAND)); RTS_HIP(s.d_cj.reserve((size_t)tcap * RTS_TRACK_MAX_CAND));
    RTS_HIP(s.d_cn.reserve(tcap)); RTS_HIP(s.d_of_track.reserve(tcap)); RTS_HIP(s.d_md2.reserve(tcap));
    RTS_HIP(s.d_zd.reserve(pcap1)); RTS_HIP(s.d_zf.reserve(pcap1)); RTS_HIP(s.d_pw.reserve(pcap1)); RTS_HIP(s.d_zrx.reserve(pcap1));
    RTS_HIP(s.d_of_plot.reserve(pcap1)); RTS_HIP(s.d_best_d.reserve(pcap1)); RTS_HIP(s.d_best_t.reserve(pcap1));
    RTS_HIP(s.d_flag.reserve(n_scan)); RTS_HIP(s.d_off.reserve(n_scan)); RTS_HIP(s.d_rounds.reserve(1));
    size_t tmp_scan = 0;
    RTS_HIP(rocprim::exclusive_scan(nullptr, tmp_scan, s.d_flag.p, s.d_off.p, 0u, n_scan, rocprim::plus<uint32_t>(), c->stream));
    RTS_HIP(s.d_tmp.reserve(tmp_scan + 1));
    RtsTrackArgs a;
    a.p = p; a.T = T; a.list = list; a.n_dev = n_dev; a.pcap = pcap; a.tcap = tcap;
    a.in = s.d_tab[s.cur].p; a.out = s.d_tab[s.cur ^ 1u].p; a.meta_in = s.d_meta.p + s.cur; a.meta_out = s.d_meta.p + (s.cur ^ 1u);
    a.pred = s.d_pred.p; a.zd = s.d_zd.p; a.zf = s.d_zf.p; a.pw = s.d_pw.p; a.zrx = s.d_zrx.p;
    a.cd = s.d_cd.p; a.cj = s.d_cj.p; a.cn = s.d_cn.p; a.of_track = s.d_of_track.p; a.of_plot = s.d_of_plot.p; a.md2 = s.d_md2.p;
    a.best_d = (unsigned long long*)s.d_best_d.p; a.best_t = s.d_best_t.p; a.rounds = s.d_rounds.p; a.flag = s.d_flag.p; a.off = s.d_off.p;
    const uint32_t widest = tcap > pcap1 ? tcap : pcap1;
    k_track_prep<<<(widest + RTS_TRACK_THREADS - 1) / RTS_TRACK_THREADS, RTS_TRACK_THREADS, 0, c->stream>>>(a);
    RTS_HIP(hipGetLastError());
    k_track_gate<<<(tcap + RTS_TRACK_WAVE_BLOCK - 1) / RTS_TRACK_WAVE_BLOCK, RTS_TRACK_THREADS, 0, c->stream>>>(a);
    RTS_HIP(hipGetLastError());
    k_track_match<<<1, RTS_TRACK_MATCH_THREADS, 0, c->stream>>>(a);
    RTS_HIP(hipGetLastError());
    const unsigned grid = (unsigned)((n_scan + RTS_TRACK_THREADS - 1) / RTS_TRACK_THREADS);
    k_track_flag<<<grid, RTS_TRACK_THREADS, 0, c->stream>>>(a);
    RTS_HIP(hipGetLastError());
    RTS_HIP(rocprim::exclusive_scan(s.d_tmp.p, tmp_scan, s.d_flag.p, s.d_off.p, 0u, n_scan, rocprim::plus<uint32_t>(), c->stream));
    k_track_write<<<grid, RTS_TRACK_THREADS, 0, c->stream>>>(a);
    RTS_HIP(hipGetLastError());
    s.cur ^= 1u;
    return RTS_OK;
}
