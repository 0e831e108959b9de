// rts_detect.hip -- the receiver end of the chain on the device (include/rts_amd.h: rts_cube_add_noise, rts_cube_detect, rts_cube_detect_os):
//   * receiver noise added to rows of the return cube (k_cube_noise; the generator is rts_noise.h, shared with rts_noise_eval)
//   * CFAR detection on a range-Doppler map and the compaction of its detections into one list in flat order: one frame (tiles,
//     staging, local maximum, segments, records; the rules every detector shares are rts_cfar.h) and two rules -- box sums and
//     CA / GO / SO (k_cfar), the k-th smallest training power (k_cfar_os; its arithmetic is rts_cfar_os.h, shared with rts_cfar_os_eval)
#include <cstring>
#include <hip/hip_runtime.h>
#include <rocprim/rocprim.hpp>
#include "rts_internal.h"

// --------------------------------------------------------------------------- receiver noise
// One thread per complex sample of the selected rows: a 16-byte load, the sample of its flat index added, a 16-byte store.  Rows
// first .. first + count - 1 of one receiver are contiguous, so blockIdx.y = receiver and x runs over count * n_bins samples.
#define RTS_NOISE_THREADS 256
__global__ void __launch_bounds__(RTS_NOISE_THREADS) k_cube_noise(double2* __restrict__ cube, uint32_t n_pulses, uint32_t n_bins, uint32_t first,
                                                                  uint64_t per_rx, double sigma, uint64_t seed)
{
    const uint64_t j = (uint64_t)blockIdx.x * RTS_NOISE_THREADS + threadIdx.x;
    if (j >= per_rx) return;
    const uint64_t i = ((uint64_t)blockIdx.y * n_pulses + first) * n_bins + j;          // flat index of the cube
    double re, im; rts_noise_sample(seed, i, sigma, &re, &im);
    double2 v = cube[i];
    v.x += re; v.y += im;
    cube[i] = v;
}

int rts_cube_noise_device(RtsContext* c, uint32_t first_pulse, uint32_t n_pulses, double sigma, uint64_t seed)
{
    const RtsCubeParams& q = c->cube.params;
    const uint64_t per_rx = (uint64_t)n_pulses * q.n_bins;
    if (per_rx == 0 || sigma == 0.0) return RTS_OK;
    dim3 grid((unsigned)((per_rx + RTS_NOISE_THREADS - 1) / RTS_NOISE_THREADS), q.n_rx);
    k_cube_noise<<<grid, RTS_NOISE_THREADS, 0, c->stream>>>((double2*)c->cube.p, q.n_pulses, q.n_bins, first_pulse, per_rx, sigma, seed);
    RTS_HIP(hipGetLastError());
    return RTS_OK;
}

// --------------------------------------------------------------------------- CFAR: the frame both detectors share
// One workgroup per tile of RTS_CFAR_TD Doppler rows x RTS_CFAR_TR range bins of one receiver, 256 threads.  P = |z|^2 of the tile and
// its halo (hd rows above and below, wrapped; hr columns left and right; rts_cfar.h) goes into LDS, one read of each cell of the map
// (16-byte loads, consecutive lanes along range).  Wave w owns rows w, w + 4, .. of the tile, lane l range bin r0 + l: a wave's ballot
// is one (rx, k, range tile) SEGMENT of the flat order, and mbcnt orders the detections within it.
// A detector's kernel runs twice: COUNT writes each segment's count; an exclusive scan over segments (in flat order) gives the offsets
// and, in the extra last element, the total; WRITE recomputes the tiles that hold a detection and writes each record at its offset.
// Nothing here asks which detector calls it: what differs between them (the value staged outside the map, the rule, its LDS) is a
// parameter or stays in the kernel.
#define RTS_CFAR_TD 16
#define RTS_CFAR_TR 64
#define RTS_CFAR_THREADS 256
struct RtsCfarFrame {
    const double2* map; uint32_t nd, nb, n_rt, local_max;
    RtsCfarWindow w;
    double pri, t0, dt;
    uint32_t* cnt; const uint32_t* off; RtsDetection* out; uint32_t max_det, n_seg;
};

struct RtsCfarTile { uint32_t t, lane, wv, rt, k0, rx, r0, rowsP, colsP; };      // the thread's place, its workgroup's tile, the staged rectangle
__device__ __forceinline__ RtsCfarTile rts_cfar_tile(const RtsCfarFrame& f)
{
    RtsCfarTile g;
    g.t = threadIdx.x; g.lane = g.t & 63u; g.wv = g.t >> 6;
    g.rt = blockIdx.x; g.k0 = blockIdx.y * RTS_CFAR_TD; g.rx = blockIdx.z; g.r0 = g.rt * RTS_CFAR_TR;
    g.rowsP = RTS_CFAR_TD + 2 * f.w.hd; g.colsP = RTS_CFAR_TR + 2 * f.w.hr;
    return g;
}

// the segment of Doppler row k of the tile, in flat order
__device__ __forceinline__ size_t rts_cfar_segment(const RtsCfarFrame& f, const RtsCfarTile& g, uint32_t k) { return ((size_t)g.rx * f.nd + k) * f.n_rt + g.rt; }

// P of the tile and its halo -> sP [rowsP][colsP], `outside` for cells outside [0, n_bins).  False (for the whole workgroup): a WRITE
// pass whose tile the COUNT pass found nothing in, which has nothing to stage.  Ends on a barrier: sP is complete.
template <bool WRITE>
__device__ __forceinline__ bool rts_cfar_stage(const RtsCfarFrame& f, const RtsCfarTile& g, double outside, double* sP)
{
    __shared__ uint32_t s_row[RTS_CFAR_TD + 2 * RTS_CFAR_MAX_HALF];      // Doppler row of the map behind each staged row (wrapped)
    if (WRITE) {
        bool any = false;
        if (g.t < RTS_CFAR_TD && g.k0 + g.t < f.nd) any = f.cnt[rts_cfar_segment(f, g, g.k0 + g.t)] != 0;
        if (!__syncthreads_or(any)) return false;
    } else if (g.t == 0 && (blockIdx.x | blockIdx.y | blockIdx.z) == 0) {
        f.cnt[f.n_seg] = 0;                          // the scan's extra element: its offset is the total
    }
    if (g.t < g.rowsP) { const int k = ((int)g.k0 - f.w.hd + (int)g.t) % (int)f.nd; s_row[g.t] = (uint32_t)(k < 0 ? k + (int)f.nd : k); }
    __syncthreads();
    const double2* mrx = f.map + (size_t)g.rx * f.nd * f.nb;
    for (uint32_t e = g.t; e < g.rowsP * g.colsP; e += RTS_CFAR_THREADS) {
        const uint32_t i = e / g.colsP, cc = e - i * g.colsP;
        const int r = (int)g.r0 - f.w.hr + (int)cc;
        double p = outside;
        if (r >= 0 && r < (int)f.nb) { const double2 z = mrx[(size_t)s_row[i] * f.nb + r]; p = z.x * z.x + z.y * z.y; }
        sP[e] = p;
    }
    __syncthreads();
    return true;
}

// RTS_CFAR_LOCAL_MAX for the cell at p0 of the staged tile, of power P, range bin r (rts_cfar.h; the staged rows already wrap)
__device__ __forceinline__ bool rts_cfar_tile_max(const RtsCfarFrame& f, const RtsCfarTile& g, const double* p0, double P, int r)
{
    const int colsP = (int)g.colsP;
    return rts_cfar_local_max(P, r >= 1, r + 1 < (int)f.nb, [p0, colsP](int dk, int dr) { return p0[dk * colsP + dr]; });
}

// A wave's row k of the tile, decided: ball = the ballot of det, seg its segment.  COUNT stores the segment's count; WRITE stores the
// lane's record at the segment's offset + its place in the ballot, unless max_detections cuts it.  n, noise, thr: the lane's
// training count, noise estimate and threshold; p0: its cell in the staged tile, of power P.
template <bool WRITE>
__device__ __forceinline__ void rts_cfar_emit(const RtsCfarFrame& f, const RtsCfarTile& g, size_t seg, unsigned long long ball, bool det,
                                              uint32_t k, int r, int n, const double* p0, double P, double noise, double thr)
{
    if (!WRITE) { if (g.lane == 0) f.cnt[seg] = (uint32_t)__popcll(ball); return; }
    if (!det) return;
    const uint32_t pos = f.off[seg] + (uint32_t)__popcll(ball & ((1ull << g.lane) - 1ull));
    if (pos >= f.max_det) return;
    f.out[pos] = rts_cfar_record(g.rx, k, (uint32_t)r, (uint32_t)n, P, noise, thr, r >= 1 ? p0[-1] : 0.0, r + 1 < (int)f.nb ? p0[1] : 0.0,
                                 p0[-(int)g.colsP], p0[g.colsP], f.nd, f.t0, f.dt, f.pri);
}

// The launch of either detector: the frame from the parameter record p (the fields RtsCfarParams and RtsCfarOsParams share), the
// buffers, COUNT, the scan, WRITE.  a: the kernel's arguments with the rule's own fields filled in; rule_rows: the rows of colsP
// doubles the rule keeps in LDS beside P.
template <class Params, class Args>
static int rts_cfar_launch(RtsContext* c, const char* who, const Params& p, const double* map, uint32_t n_doppler, uint32_t max_det, Args a,
                           void (*k_count)(Args), void (*k_write)(Args), uint32_t rule_rows)
{
    const RtsCubeParams& q = c->cube.params;
    RtsDetectState& s = c->cube.detect;
    RtsCfarFrame& f = a.f;
    f.map = (const double2*)map; f.nd = n_doppler; f.nb = q.n_bins; f.n_rt = (q.n_bins + RTS_CFAR_TR - 1) / RTS_CFAR_TR;
    f.w = rts_cfar_window(p.guard_range, p.guard_doppler, p.train_range, p.train_doppler);
    f.local_max = (p.flags & RTS_CFAR_LOCAL_MAX) ? 1u : 0u; f.pri = p.pri; f.t0 = q.t0; f.dt = q.dt;
    const size_t n_seg = (size_t)q.n_rx * n_doppler * f.n_rt;
    if (n_seg + 1 > 0xffffffffull) { rts_set_error("%s: %zu segments: the map is too large", who, n_seg); return RTS_ERR_INVALID; }
    f.n_seg = (uint32_t)n_seg; f.max_det = max_det;
    RTS_HIP(s.d_cnt.reserve(n_seg + 1)); RTS_HIP(s.d_off.reserve(n_seg + 1)); RTS_HIP(s.d_list.reserve(max_det));
    size_t tmp = 0;
    RTS_HIP(rocprim::exclusive_scan(nullptr, tmp, s.d_cnt.p, s.d_off.p, 0u, n_seg + 1, rocprim::plus<uint32_t>(), c->stream));
    RTS_HIP(s.d_tmp.reserve(tmp + 1));
    f.cnt = s.d_cnt.p; f.off = s.d_off.p; f.out = s.d_list.p;
    const size_t lds = sizeof(double) * (size_t)(RTS_CFAR_TD + 2 * f.w.hd + rule_rows) * (RTS_CFAR_TR + 2 * f.w.hr);      // P and the rule's rows: <= 60 KiB
    dim3 grid(f.n_rt, (n_doppler + RTS_CFAR_TD - 1) / RTS_CFAR_TD, q.n_rx);
    k_count<<<grid, RTS_CFAR_THREADS, lds, c->stream>>>(a);
    RTS_HIP(hipGetLastError());
    RTS_HIP(rocprim::exclusive_scan(s.d_tmp.p, tmp, s.d_cnt.p, s.d_off.p, 0u, n_seg + 1, rocprim::plus<uint32_t>(), c->stream));
    k_write<<<grid, RTS_CFAR_THREADS, lds, c->stream>>>(a);
    RTS_HIP(hipGetLastError());
    s.nseg = (uint32_t)n_seg; s.max = max_det; s.nd = n_doppler; s.valid = true;
    return RTS_OK;
}

// --------------------------------------------------------------------------- CFAR by the mean level (CA / GO / SO)
// The rule on the staged tile:
//   1. Column partial sums along Doppler for every tile row and staged column: strip = the 2 Td training rows (|dk| > Gd), full =
//      strip + the 2 Gd + 1 guard rows.  Direct sums of powers, never differences.  Cells outside [0, n_bins) are staged as 0.
//   2. Row sums per cell over the annulus as four disjoint rectangles -- outer columns (|dr| > Gr) from `full`, inner columns
//      (0 < |dr| <= Gr) and the CUT's own column from `strip`: left half (dr < 0), right half (dr > 0), centre (dr = 0).
struct RtsCfarArgs { RtsCfarFrame f; uint32_t mode; double pfa, alpha; };

template <bool WRITE>
__global__ void __launch_bounds__(RTS_CFAR_THREADS) k_cfar(const RtsCfarArgs a)
{
    extern __shared__ __attribute__((aligned(16))) double s_cfar[];      // P [rowsP][colsP], full [TD][colsP], strip [TD][colsP]
    const RtsCfarFrame& f = a.f;
    const RtsCfarTile g = rts_cfar_tile(f);
    const uint32_t t = g.t, lane = g.lane, wv = g.wv, k0 = g.k0, colsP = g.colsP;
    const int hr = f.w.hr, hd = f.w.hd, gr = f.w.gr, gd = f.w.gd, Or = rts_cfar_Or(f.w), Od = rts_cfar_Od(f.w);
    double* sP = s_cfar; double* sFull = sP + (size_t)g.rowsP * colsP; double* sStrip = sFull + (size_t)RTS_CFAR_TD * colsP;
    if (!rts_cfar_stage<WRITE>(f, g, 0.0, sP)) return;
    // 1. column sums along Doppler (tile row i is staged row i + hd)
    for (uint32_t e = t; e < RTS_CFAR_TD * colsP; e += RTS_CFAR_THREADS) {
        const uint32_t i = e / colsP, cc = e - i * colsP;
        const double* col = sP + (size_t)(i + hd) * colsP + cc;
        double strip = 0.0, guard = 0.0;
        for (int dk = -Od; dk < -gd; dk++) strip += col[dk * (int)colsP];
        for (int dk = gd + 1; dk <= Od; dk++) strip += col[dk * (int)colsP];
        for (int dk = -gd; dk <= gd; dk++) guard += col[dk * (int)colsP];
        sStrip[e] = strip; sFull[e] = strip + guard;
    }
    __syncthreads();
    // 2. per cell: row sums, threshold, rule, compaction
    const int r = (int)g.r0 + (int)lane;
    for (uint32_t i = wv; i < RTS_CFAR_TD; i += RTS_CFAR_THREADS / 64) {
        const uint32_t k = k0 + i;
        const bool valid = k < f.nd && r < (int)f.nb;
        const uint32_t cc = lane + (uint32_t)hr;
        const double* full = sFull + (size_t)i * colsP + cc; const double* strip = sStrip + (size_t)i * colsP + cc;
        double sl = 0.0, sr = 0.0;
        for (int dr = -Or; dr < -gr; dr++) sl += full[dr];
        for (int dr = -gr; dr < 0; dr++) sl += strip[dr];
        for (int dr = gr + 1; dr <= Or; dr++) sr += full[dr];
        for (int dr = 1; dr <= gr; dr++) sr += strip[dr];
        const double sc = strip[0];
        int nl, nr;
        const int n = rts_cfar_count(f.w, r, (int)f.nb - 1 - r, &nl, &nr);      // (lanes past the last bin: some count, never reported)
        double noise;
        if (a.mode == RTS_CFAR_CA) noise = (sl + sr + sc) / (double)n;
        else {
            const double ml = sl / (double)nl, mr = sr / (double)nr;
            if (nl == 0) noise = mr; else if (nr == 0) noise = ml;
            else noise = a.mode == RTS_CFAR_GO ? fmax(ml, mr) : fmin(ml, mr);
        }
        const double alpha = a.pfa > 0.0 ? (double)n * expm1(-log(a.pfa) / (double)n) : a.alpha;
        const double thr = alpha * noise;
        const double* p0 = sP + (size_t)(i + hd) * colsP + cc;
        const double P = p0[0];
        bool det = valid && P > thr;
        if (det && f.local_max) det = rts_cfar_tile_max(f, g, p0, P, r);
        const unsigned long long ball = __ballot(det);
        if (k >= f.nd) continue;                                        // (wave-uniform: k is the wave's row)
        rts_cfar_emit<WRITE>(f, g, rts_cfar_segment(f, g, k), ball, det, k, r, n, p0, P, noise, thr);
    }
}

int rts_cube_detect_device(RtsContext* c, const RtsCfarParams& p, const double* map, uint32_t n_doppler, uint32_t max_det)
{
    RtsCfarArgs a;
    a.mode = p.mode; a.pfa = p.pfa; a.alpha = p.alpha;
    return rts_cfar_launch(c, "rts_cube_detect", p, map, n_doppler, max_det, a, k_cfar<false>, k_cfar<true>, 2 * RTS_CFAR_TD);
}

// --------------------------------------------------------------------------- ordered-statistic CFAR
// The noise estimate is the k-th smallest of a cell's N training powers (rts_cfar_os.h) instead of their mean, so there are no box sums
// to share between cells and no LDS beside P:
//   1. Cells outside [0, n_bins) are staged as +inf: such a cell is never "below" anything.
//   2. The DECISION needs no selection.  fl(alpha x) does not fall when x rises, so P > alpha x_(k) holds exactly when at least k of the
//      training cells have alpha x_i < P: one multiply, compare and count per training cell, lane <-> range bin, so that consecutive
//      lanes read consecutive doubles of a staged row (8-byte LDS reads without bank conflicts).  Every loop bound is wave-uniform.
//   3. The RECORD needs x_(k) itself, and only the WRITE pass forms it -- it repeats step 2 for the rows of a tile that the COUNT pass
//      found a detection in, and no others -- per detected cell, the wave together: each lane takes up to 18 of
//      the <= 33 x 33 cells of the window's bounding rectangle as 64-bit keys (all ones for the guard and for cells outside the map),
//      and the k-th smallest key is built bit by bit from the top -- the largest t of which fewer than k keys lie below -- with one
//      ballot and population count per key register and bit, the high word first and then the low word of the keys that share it
//      (32-bit compares): 63 x 18 ballots per detection, 63 x 6 for a window of up to 384 cells, none on the common path.
struct RtsCfarOsArgs { RtsCfarFrame f; uint32_t rank, n0; const double* alpha_tab; double alpha; };
#define RTS_CFAR_OS_KEYS 18          // key registers per lane: 64 x 18 >= 33 x 33
#define RTS_CFAR_OS_KEYS_SMALL 6     // ... of which a window whose rectangle holds at most 64 x 6 cells fills only the first 6

// how many of the wave's keys k[0 .. R) (one per lane and register) lie below cand: a ballot and a population count per register
template <int R> __device__ __forceinline__ uint32_t rts_cfar_os_below(const uint32_t (&k)[RTS_CFAR_OS_KEYS], uint32_t cand)
{
    uint32_t c = 0;
#pragma unroll
    for (int j = 0; j < R; j++) c += (uint32_t)__popcll(__ballot(k[j] < cand));
    return c;
}

template <bool WRITE>
__global__ void __launch_bounds__(RTS_CFAR_THREADS) k_cfar_os(const RtsCfarOsArgs a)
{
    extern __shared__ __attribute__((aligned(16))) double s_os[];        // P [rowsP][colsP]
    const RtsCfarFrame& f = a.f;
    const RtsCfarTile g = rts_cfar_tile(f);
    const uint32_t lane = g.lane, wv = g.wv, k0 = g.k0, colsP = g.colsP;
    const int hr = f.w.hr, hd = f.w.hd, gr = f.w.gr, gd = f.w.gd, Or = rts_cfar_Or(f.w), Od = rts_cfar_Od(f.w);
    double* sP = s_os;
    if (!rts_cfar_stage<WRITE>(f, g, __builtin_huge_val(), sP)) return;
    // 2. per cell: the count of training cells below, the rule, compaction
    const int r = (int)g.r0 + (int)lane;
    const bool in_map = r < (int)f.nb;
    const int n = in_map ? rts_cfar_count(f.w, r, (int)f.nb - 1 - r) : 1;      // (lanes past the last bin: any count inside the table)
    const uint32_t kth = rts_cfar_os_rank(a.rank, (uint32_t)n, a.n0);
    const double alpha = a.alpha_tab ? a.alpha_tab[n] : a.alpha;
    for (uint32_t i = wv; i < RTS_CFAR_TD; i += RTS_CFAR_THREADS / 64) {
        const uint32_t k = k0 + i;
        if (k >= f.nd) continue;                                        // (wave-uniform: k is the wave's row)
        const size_t seg = rts_cfar_segment(f, g, k);
        if (WRITE && f.cnt[seg] == 0) continue;                         // (wave-uniform: the COUNT pass found nothing in this row of the tile)
        const double* p0 = sP + (size_t)(i + hd) * colsP + lane + (uint32_t)hr;
        const double P = p0[0];
        uint32_t below = 0;
        for (int dk = -Od; dk <= Od; dk++) {
            const double* row = p0 + dk * (int)colsP;
            if (dk >= -gd && dk <= gd) {
#pragma unroll 4
                for (int dr = -Or; dr < -gr; dr++) below += alpha * row[dr] < P ? 1u : 0u;
#pragma unroll 4
                for (int dr = gr + 1; dr <= Or; dr++) below += alpha * row[dr] < P ? 1u : 0u;
            } else {
#pragma unroll 8
                for (int dr = -Or; dr <= Or; dr++) below += alpha * row[dr] < P ? 1u : 0u;      // (unrolled: several LDS reads in flight per wait)
            }
        }
        bool det = in_map && below >= kth;
        if (det && f.local_max) det = rts_cfar_tile_max(f, g, p0, P, r);
        const unsigned long long ball = __ballot(det);
        // 3. the order statistic of every detected cell of the row (the loop and everything in it but `noise` is wave-uniform); the
        //    COUNT pass writes no record and skips it
        double noise = 0.0;
        const uint32_t W = 2u * (uint32_t)Or + 1u, rect = W * (2u * (uint32_t)Od + 1u);
        for (unsigned long long rest = WRITE ? ball : 0ull; rest != 0ull; rest &= rest - 1ull) {
            const int src = __ffsll((long long)rest) - 1, rs = (int)g.r0 + src;
            const double* c0 = sP + (size_t)(i + hd) * colsP + (uint32_t)src + (uint32_t)hr;
            uint32_t khi[RTS_CFAR_OS_KEYS], klo[RTS_CFAR_OS_KEYS];
#pragma unroll
            for (int j = 0; j < RTS_CFAR_OS_KEYS; j++) {
                const uint32_t e = (uint32_t)j * 64u + lane;
                uint64_t key = ~0ull;
                if (e < rect) {
                    const int dk = (int)(e / W) - Od, dr = (int)(e % W) - Or;
                    const bool guard = dk >= -gd && dk <= gd && dr >= -gr && dr <= gr;
                    if (!guard && rs + dr >= 0 && rs + dr < (int)f.nb) key = rts_cfar_os_key(c0[dk * (int)colsP + dr]);
                }
                khi[j] = (uint32_t)(key >> 32); klo[j] = (uint32_t)key;
            }
            const uint32_t ks = rts_cfar_os_rank(a.rank, (uint32_t)rts_cfar_count(f.w, rs, (int)f.nb - 1 - rs), a.n0);
            // the high word of the k-th smallest key (bit 31 is the sign: never set in a power's key) ...
            const bool small = rect <= 64u * RTS_CFAR_OS_KEYS_SMALL;      // (wave-uniform: the registers beyond hold no key)
            uint32_t hi = 0;
            for (int bit = 30; bit >= 0; bit--) {
                const uint32_t cand = hi | (1u << bit);
                const uint32_t c = small ? rts_cfar_os_below<RTS_CFAR_OS_KEYS_SMALL>(khi, cand) : rts_cfar_os_below<RTS_CFAR_OS_KEYS>(khi, cand);
                if (c < ks) hi = cand;
            }
            // ... then its low word: a key with a smaller high word is below every candidate (0: a candidate has a bit set), one with
            // a larger high word below none (all ones)
#pragma unroll
            for (int j = 0; j < RTS_CFAR_OS_KEYS; j++) klo[j] = khi[j] < hi ? 0u : khi[j] == hi ? klo[j] : 0xffffffffu;
            uint32_t lo = 0;
            for (int bit = 31; bit >= 0; bit--) {
                const uint32_t cand = lo | (1u << bit);
                const uint32_t c = small ? rts_cfar_os_below<RTS_CFAR_OS_KEYS_SMALL>(klo, cand) : rts_cfar_os_below<RTS_CFAR_OS_KEYS>(klo, cand);
                if (c < ks) lo = cand;
            }
            const uint64_t ans = (uint64_t)hi << 32 | lo;
            if ((int)lane == src) noise = rts_cfar_os_unkey(ans);
        }
        rts_cfar_emit<WRITE>(f, g, seg, ball, det, k, r, n, p0, P, noise, alpha * noise);
    }
}

int rts_cube_detect_os_device(RtsContext* c, const RtsCfarOsParams& p, const double* alpha_tab, const double* map, uint32_t n_doppler, uint32_t max_det)
{
    RtsCfarOsArgs a;
    a.rank = p.rank; a.n0 = rts_cfar_n0(p.guard_range, p.guard_doppler, p.train_range, p.train_doppler); a.alpha_tab = alpha_tab; a.alpha = p.alpha;
    return rts_cfar_launch(c, "rts_cube_detect_os", p, map, n_doppler, max_det, a, k_cfar_os<false>, k_cfar_os<true>, 0);
}
