// rts_tbd.hip -- track-before-detect on the device (include/rts_amd.h: rts_cube_tbd_step, rts_cube_tbd_extract).  Every rule -- the
// shift, the score, the window's first maximum and its code, the candidate, the walk, the record -- is rts_tbd.h, shared with the
// host evaluators.  Wave64; nothing here waits on the host.
//   k_tbd_step        ONE pass, a workgroup per (rx, Doppler row kd, tile of RTS_TBD_TILE range bins).  It forms s[kd] itself (the
//                     arithmetic of the table is the header's; the workgroups of rx 0, tile 0 store the entry for the walk), stages
//                     the 2 Hd + 1 previous merit rows of its tile in LDS as f64, each displaced by -s[kd] and widened by Hr on both
//                     sides (zeros where the range axis ends: a zero never replaces the best), and every thread then takes cells
//                     tid, tid + 256, ..: the score from the map (one 16-byte load), the window out of LDS in ascending (dd, dr) --
//                     consecutive lanes read consecutive doubles, no bank conflicts -- merit and pointer out.  Per cell 16 B of map
//                     and 8 B of merit read, 8 B + 1 B written; the 2 Hd extra row reads of a tile are rows the workgroups of adjacent kd
//                     (adjacent block indices, so close in time, though as a rule on other XCDs) read too: cache at best, never
//                     relied on.  LDS: (2 Hd + 1)(TILE + 2 Hr) doubles,
//                     24.1 KiB at half (1, 2) -- six workgroups a CU -- and 57.6 KiB at (3, 15).
//                     The other shape -- a pass that leaves per cell of the previous map its first maximum over dr and that dr, and a
//                     second pass over dd at r - s[kd] -- writes and reads an intermediate of 9 B per cell, 18 B of traffic on a
//                     33-byte floor, to save LDS reads.  It was not built (profiles/tbd_bench.txt).
//   k_tbd_cand<false> a thread per cell, a wave per segment of 64 cells: the candidate rule, the segment's count (a ballot)
//   (exclusive scan of the counts, rocprim: element n_seg is the total)
//   k_tbd_cand<true>  the same rule again; a candidate's place is its segment's offset + its rank in the ballot -- ascending flat
//                     order, no atomics -- and the lane that holds it walks back through the ring (not hot: one thread per
//                     candidate) and writes record and path.
#include <cstring>
#include <hip/hip_runtime.h>
#include <rocprim/rocprim.hpp>
#include "rts_internal.h"

#define RTS_TBD_THREADS 256

struct RtsTbdStepArgs {
    const double* map; const double* prev; double* next; uint8_t* ptr; int32_t* shift;       // prev null: the first frame
    uint32_t n_rx, nd, nb, tiles; int Hd, Hr; uint32_t score;
    double scale, decay, k, pri, T, dt;
};

__global__ void __launch_bounds__(RTS_TBD_THREADS) k_tbd_step(const RtsTbdStepArgs a)
{
    extern __shared__ double s_prev[];                                   // [2 Hd + 1][TILE + 2 Hr]
    const uint32_t tid = threadIdx.x;
    const uint32_t kd = blockIdx.x % a.nd, tile = (blockIdx.x / a.nd) % a.tiles, rx = blockIdx.x / a.nd / a.tiles;
    const uint32_t r0 = tile * RTS_TBD_TILE, cnt = a.nb - r0 < RTS_TBD_TILE ? a.nb - r0 : RTS_TBD_TILE;
    const bool first = a.prev == nullptr;
    const int32_t s = first ? 0 : rts_tbd_shift(rts_tbd_shift_quotient(kd, a.nd, a.k, a.pri, a.T, a.dt));
    if (rx == 0u && tile == 0u && tid == 0u) a.shift[kd] = s;
    const uint32_t W = RTS_TBD_TILE + 2u * (uint32_t)a.Hr;
    if (!first) {
        const int64_t g0 = ((int64_t)r0 - (int64_t)s) - a.Hr;            // the range bin staged at column 0
        for (int dd = -a.Hd; dd <= a.Hd; dd++) {
            const double* row = a.prev + ((size_t)rx * a.nd + rts_tbd_row(kd, dd, a.nd)) * a.nb;
            double* dst = s_prev + (size_t)(dd + a.Hd) * W;
            for (uint32_t j = tid; j < cnt + 2u * (uint32_t)a.Hr; j += RTS_TBD_THREADS) {
                const int64_t g = g0 + j;
                dst[j] = g >= 0 && g < (int64_t)a.nb ? row[g] : 0.0;
            }
        }
        __syncthreads();
    }
    const size_t row = ((size_t)rx * a.nd + kd) * a.nb;
    const double2* map = (const double2*)a.map + row;
    for (uint32_t i = tid; i < cnt; i += RTS_TBD_THREADS) {
        const double2 z = map[r0 + i];
        const double x = rts_tbd_score(z.x, z.y, a.score, a.scale);
        double m = x; uint32_t code = RTS_TBD_NONE;
        if (!first) {
            const double* p0 = s_prev + (size_t)a.Hd * W + i + (uint32_t)a.Hr;      // the cell's column in the middle row
            double best;
            rts_tbd_best(a.Hd, a.Hr, [p0, W](int dd, int dr) { return p0[dd * (int)W + dr]; }, &best, &code);
            m = rts_tbd_merit(x, a.decay, best);
        }
        a.next[row + r0 + i] = m; a.ptr[row + r0 + i] = (uint8_t)code;
    }
}

struct RtsTbdExtArgs {
    const double* merit; const uint8_t* ring; const int32_t* shifts;                          // the ring's slots: [depth][cells], [depth][nd]
    uint32_t n_rx, nd, nb, cells, n_seg, depth, Hd, Hr, last, max_cells;                      // last: the slot of the newest frame
    double threshold, t0, dt, pri; uint32_t local_max, max_tracks;
    uint32_t* cnt; const uint32_t* off; RtsTbdTrack* out; uint32_t* paths;
};

template <bool WRITE> __global__ void __launch_bounds__(RTS_TBD_THREADS) k_tbd_cand(const RtsTbdExtArgs a)
{
    const uint32_t e = blockIdx.x * RTS_TBD_THREADS + threadIdx.x, lane = threadIdx.x & 63u, seg = e >> 6;
    if (seg > a.n_seg) return;                                           // (wave-uniform; segment n_seg is the scan's extra element: 0)
    bool cand = false;
    uint32_t rx = 0, kd = 0, r = 0; double v = 0.0;
    if (e < a.cells) {
        r = e % a.nb; kd = (e / a.nb) % a.nd; rx = e / a.nb / a.nd;
        const double* m = a.merit + (size_t)rx * a.nd * a.nb;
        v = m[(size_t)kd * a.nb + r];
        const uint32_t nd = a.nd, nb = a.nb;
        cand = rts_tbd_candidate(v, a.threshold, a.local_max != 0u, r >= 1u, r + 1u < nb,
                                 [m, kd, r, nd, nb](int dk, int dr) { return m[(size_t)rts_tbd_row(kd, dk, nd) * nb + (size_t)((int64_t)r + dr)]; });
    }
    const unsigned long long ball = __ballot(cand);
    if (!WRITE) { if (lane == 0u) a.cnt[seg] = (uint32_t)__popcll(ball); return; }
    if (!cand) return;
    const uint32_t pos = a.off[seg] + (uint32_t)__popcll(ball & ((1ull << lane) - 1ull));
    if (pos >= a.max_tracks) return;
    const uint8_t* ring = a.ring + ((size_t)rx * a.nd) * a.nb; const int32_t* shifts = a.shifts;
    const uint32_t depth = a.depth, last = a.last, nd = a.nd, nb = a.nb; const size_t cells = a.cells;
    uint32_t fk, fr;
    const uint32_t n = rts_tbd_walk(nd, nb, a.Hd, a.Hr, a.max_cells, depth, kd, r,
        [ring, depth, last, nb, cells](uint32_t j, uint32_t k, uint32_t b) { return (uint32_t)ring[(size_t)((last + depth - j) % depth) * cells + (size_t)k * nb + b]; },
        [shifts, depth, last, nd](uint32_t j, uint32_t k) { return shifts[(size_t)((last + depth - j) % depth) * nd + k]; },
        a.paths + (size_t)pos * depth * 2u, &fk, &fr);
    a.out[pos] = rts_tbd_record(rx, kd, r, n, fk, fr, v, nd, a.t0, a.dt, a.pri);
}

// One step of a validated call on a state whose buffers exist: map -> merit[cur ^ 1], the pointers and the shifts into ring slot `slot`
int rts_cube_tbd_step_device(RtsContext* c, const RtsTbdParams& p, const double* map, bool first, double T, double dt, uint32_t slot)
{
    RtsTbdState& s = c->cube.tbd;
    const size_t cells = (size_t)s.rx * s.nd * s.nb;
    RtsTbdStepArgs a;
    a.map = map; a.prev = first ? nullptr : s.d_merit[s.cur].p; a.next = s.d_merit[s.cur ^ 1u].p;
    a.ptr = s.d_ptr.p + (size_t)slot * cells; a.shift = s.d_shift.p + (size_t)slot * s.nd;
    a.n_rx = s.rx; a.nd = s.nd; a.nb = s.nb; a.tiles = (s.nb + RTS_TBD_TILE - 1u) / RTS_TBD_TILE;
    a.Hd = (int)p.half_doppler; a.Hr = (int)p.half_range; a.score = p.score;
    a.scale = p.scale; a.decay = p.decay; a.k = p.delay_rate_per_hz; a.pri = p.pri; a.T = T; a.dt = dt;
    const size_t lds = sizeof(double) * (2u * p.half_doppler + 1u) * (RTS_TBD_TILE + 2u * p.half_range);
    const uint64_t grid = (uint64_t)a.tiles * a.nd * a.n_rx;             // (cells <= RTS_TBD_MAX_CELLS: below 2^31)
    k_tbd_step<<<(unsigned)grid, RTS_TBD_THREADS, lds, c->stream>>>(a);
    RTS_HIP(hipGetLastError());
    s.cur ^= 1u;
    return RTS_OK;
}

int rts_cube_tbd_extract_device(RtsContext* c, const RtsTbdExtractParams& e, uint32_t max_tracks)
{
    RtsTbdState& s = c->cube.tbd;
    const uint32_t cells = s.rx * s.nd * s.nb, n_seg = (cells + 63u) / 64u;
    const size_t n_scan = (size_t)n_seg + 1;
    RTS_HIP(s.d_cnt.reserve(n_scan)); RTS_HIP(s.d_off.reserve(n_scan));
    RTS_HIP(s.d_out.reserve(max_tracks)); RTS_HIP(s.d_paths.reserve((size_t)max_tracks * s.depth * 2u));
    size_t tmp_scan = 0;
    RTS_HIP(rocprim::exclusive_scan(nullptr, tmp_scan, s.d_cnt.p, s.d_off.p, 0u, n_scan, rocprim::plus<uint32_t>(), c->stream));
    RTS_HIP(s.d_tmp.reserve(tmp_scan + 1));
    RtsTbdExtArgs a;
    a.merit = s.d_merit[s.cur].p; a.ring = s.d_ptr.p; a.shifts = s.d_shift.p;
    a.n_rx = s.rx; a.nd = s.nd; a.nb = s.nb; a.cells = cells; a.n_seg = n_seg; a.depth = s.depth; a.Hd = s.hd; a.Hr = s.hr;
    a.last = (uint32_t)((s.frames - 1u) % s.depth); a.max_cells = s.frames < s.depth ? (uint32_t)s.frames : s.depth;
    a.threshold = e.threshold; a.t0 = s.t0; a.dt = s.dt; a.pri = e.pri; a.local_max = e.flags & RTS_TBD_LOCAL_MAX; a.max_tracks = max_tracks;
    a.cnt = s.d_cnt.p; a.off = s.d_off.p; a.out = s.d_out.p; a.paths = s.d_paths.p;
    const unsigned grid = (unsigned)((n_scan * 64u + RTS_TBD_THREADS - 1) / RTS_TBD_THREADS);
    k_tbd_cand<false><<<grid, RTS_TBD_THREADS, 0, c->stream>>>(a);
    RTS_HIP(hipGetLastError());
    RTS_HIP(rocprim::exclusive_scan(s.d_tmp.p, tmp_scan, s.d_cnt.p, s.d_off.p, 0u, n_scan, rocprim::plus<uint32_t>(), c->stream));
    k_tbd_cand<true><<<grid, RTS_TBD_THREADS, 0, c->stream>>>(a);
    RTS_HIP(hipGetLastError());
    s.ext_nseg = n_seg; s.ext_max = max_tracks; s.ext_depth = s.depth; s.ext_valid = true;
    return RTS_OK;
}
