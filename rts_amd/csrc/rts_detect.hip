// rts_detect.hip -- the receiver end of the chain on the device (include/rts_amd.h: rts_cube_add_noise, rts_cube_detect, rts_cube_detect_os):
//   * receiver noise added to rows of the return cube (k_cube_noise; the generator is rts_noise.h, shared with rts_noise_eval)
//   * CFAR detection on a range-Doppler map and the compaction of its detections into one list in flat order (k_cfar)
//   * ordered-statistic CFAR on the same map, into the same list (k_cfar_os; the arithmetic is rts_cfar_os.h, shared with rts_cfar_os_eval)
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

// --------------------------------------------------------------------------- CFAR
// One workgroup per tile of RTS_CFAR_TD Doppler rows x RTS_CFAR_TR range bins of one receiver, 256 threads.
//   1. P = |z|^2 of the tile and its halo (hd = max(Gd + Td, 1) rows above and below, wrapped; hr = max(Gr + Tr, 1) columns left and
//      right, 0 outside [0, n_bins)) into LDS, one read of each cell of the map (16-byte loads, consecutive lanes along range).
//   2. Column partial sums along Doppler for every tile row and staged column: strip = the 2 Td training rows (|dk| > Gd), full =
//      strip + the 2 Gd + 1 guard rows.  Direct sums of powers, never differences.
//   3. Row sums per cell over the annulus as four disjoint rectangles -- outer columns (|dr| > Gr) from `full`, inner columns
//      (0 < |dr| <= Gr) and the CUT's own column from `strip`: left half (dr < 0), right half (dr > 0), centre (dr = 0).
//   4. Wave w owns rows w, w + 4, .. of the tile, lane l range bin r0 + l: a wave's ballot is one (rx, k, range tile) SEGMENT of the
//      flat order, and mbcnt orders the detections within it.
// The kernel runs twice: COUNT writes each segment's count; an exclusive scan over segments (in flat order) gives the offsets and,
// in the extra last element, the total; WRITE recomputes the tiles that hold a detection and writes each record at its offset.
#define RTS_CFAR_TD 16
#define RTS_CFAR_TR 64
#define RTS_CFAR_THREADS 256
struct RtsCfarArgs {
    const double2* map; uint32_t nd, nb, n_rt;
    int gr, gd, tr, td, hr, hd;
    uint32_t mode, local_max; double pfa, alpha, pri, t0, dt;
    uint32_t* cnt; const uint32_t* off; RtsDetection* out; uint32_t max_det, n_seg;
};

// parabola through ln P of three samples: the vertex offset in [-0.5, 0.5], 0 when it is not a peak of positive powers
__device__ __forceinline__ double rts_cfar_delta(double pm, double p0, double pp)
{
    if (!(pm > 0.0) || !(p0 > 0.0) || !(pp > 0.0)) return 0.0;
    const double lm = log(pm), l0 = log(p0), lp = log(pp);
    const double den = lm - 2.0 * l0 + lp;
    if (!(den < 0.0)) return 0.0;
    const double d = 0.5 * (lm - lp) / den;
    return fmin(0.5, fmax(-0.5, d));
}

template <bool WRITE>
__global__ void __launch_bounds__(RTS_CFAR_THREADS) k_cfar(const RtsCfarArgs a)
{
    extern __shared__ __attribute__((aligned(16))) double s_cfar[];      // P [rowsP][colsP], full [TD][colsP], strip [TD][colsP]
    __shared__ uint32_t s_row[RTS_CFAR_TD + 2 * RTS_CFAR_MAX_HALF];      // Doppler row of the map behind each staged row (wrapped)
    const uint32_t t = threadIdx.x, lane = t & 63u, wv = t >> 6;
    const uint32_t rt = blockIdx.x, k0 = blockIdx.y * RTS_CFAR_TD, rx = blockIdx.z, r0 = rt * RTS_CFAR_TR;
    const int hr = a.hr, hd = a.hd, gr = a.gr, gd = a.gd, tr = a.tr, td = a.td;
    const int Or = gr + tr, Od = gd + td;
    const uint32_t rowsP = RTS_CFAR_TD + 2 * hd, colsP = RTS_CFAR_TR + 2 * hr;
    if (WRITE) {
        bool any = false;
        if (t < RTS_CFAR_TD && k0 + t < a.nd) any = a.cnt[((size_t)rx * a.nd + k0 + t) * a.n_rt + rt] != 0;
        if (!__syncthreads_or(any)) return;
    } else if (t == 0 && (blockIdx.x | blockIdx.y | blockIdx.z) == 0) {
        a.cnt[a.n_seg] = 0;                          // the scan's extra element: its offset is the total
    }
    double* sP = s_cfar; double* sFull = sP + (size_t)rowsP * colsP; double* sStrip = sFull + (size_t)RTS_CFAR_TD * colsP;
    if (t < rowsP) { const int k = ((int)k0 - hd + (int)t) % (int)a.nd; s_row[t] = (uint32_t)(k < 0 ? k + (int)a.nd : k); }
    __syncthreads();
    // 1. stage P
    const double2* mrx = a.map + (size_t)rx * a.nd * a.nb;
    for (uint32_t e = t; e < rowsP * colsP; e += RTS_CFAR_THREADS) {
        const uint32_t i = e / colsP, cc = e - i * colsP;
        const int r = (int)r0 - hr + (int)cc;
        double p = 0.0;
        if (r >= 0 && r < (int)a.nb) { const double2 z = mrx[(size_t)s_row[i] * a.nb + r]; p = z.x * z.x + z.y * z.y; }
        sP[e] = p;
    }
    __syncthreads();
    // 2. column sums along Doppler (tile row i is staged row i + hd)
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
    // 3. + 4. per cell: row sums, threshold, rule, compaction
    const int r = (int)r0 + (int)lane;
    const int edge_l = r, edge_r = (int)a.nb - 1 - r;              // cells to the range edges
    for (uint32_t i = wv; i < RTS_CFAR_TD; i += RTS_CFAR_THREADS / 64) {
        const uint32_t k = k0 + i;
        const bool valid = k < a.nd && r < (int)a.nb;
        const uint32_t cc = lane + (uint32_t)hr;
        const double* full = sFull + (size_t)i * colsP + cc; const double* strip = sStrip + (size_t)i * colsP + cc;
        double sl = 0.0, sr = 0.0;
        for (int dr = -Or; dr < -gr; dr++) sl += full[dr];
        for (int dr = -gr; dr < 0; dr++) sl += strip[dr];
        for (int dr = gr + 1; dr <= Or; dr++) sr += full[dr];
        for (int dr = 1; dr <= gr; dr++) sr += strip[dr];
        const double sc = strip[0];
        const int nlo = max(0, min(Or, edge_l) - gr), nli = min(gr, edge_l);
        const int nro = max(0, min(Or, edge_r) - gr), nri = min(gr, edge_r);
        const int nl = nlo * (2 * Od + 1) + nli * 2 * td, nr = nro * (2 * Od + 1) + nri * 2 * td;
        const int n = nl + nr + 2 * td;
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
        if (det && a.local_max) {
            for (int dk = -1; dk <= 1; dk++)
                for (int dr = -1; dr <= 1; dr++) {
                    if ((dk == 0 && dr == 0) || r + dr < 0 || r + dr >= (int)a.nb) continue;
                    const double q = p0[dk * (int)colsP + dr];
                    if (dk < 0 || (dk == 0 && dr < 0)) det = det && P > q; else det = det && P >= q;
                }
        }
        const unsigned long long ball = __ballot(det);
        if (k >= a.nd) continue;                                        // (wave-uniform: k is the wave's row)
        const size_t seg = ((size_t)rx * a.nd + k) * a.n_rt + rt;
        if (!WRITE) { if (lane == 0) a.cnt[seg] = (uint32_t)__popcll(ball); continue; }
        if (!det) continue;
        const uint32_t pos = a.off[seg] + (uint32_t)__popcll(ball & ((1ull << lane) - 1ull));
        if (pos >= a.max_det) continue;
        const double dr_ = rts_cfar_delta(r >= 1 ? p0[-1] : 0.0, P, r + 1 < (int)a.nb ? p0[1] : 0.0);
        const double dd_ = rts_cfar_delta(p0[-(int)colsP], P, p0[colsP]);
        double w = (double)k + dd_;
        const double half = 0.5 * (double)a.nd;
        if (w >= half) w -= (double)a.nd; else if (w < -half) w += (double)a.nd;
        RtsDetection d;
        d.rx = rx; d.doppler_bin = k; d.range_bin = (uint32_t)r; d.n_train = (uint32_t)n;
        d.power = P; d.noise = noise; d.threshold = thr; d.range_offset = dr_; d.doppler_offset = dd_;
        d.delay = a.t0 + ((double)r + dr_) * a.dt;
        d.doppler = a.pri > 0.0 ? w / ((double)a.nd * a.pri) : 0.0;
        a.out[pos] = d;
    }
}

int rts_cube_detect_device(RtsContext* c, const RtsCfarParams& p, const double* map, uint32_t n_doppler, uint32_t max_det)
{
    const RtsCubeParams& q = c->cube.params;
    RtsCfarArgs a;
    a.map = (const double2*)map; a.nd = n_doppler; a.nb = q.n_bins; a.n_rt = (q.n_bins + RTS_CFAR_TR - 1) / RTS_CFAR_TR;
    a.gr = (int)p.guard_range; a.gd = (int)p.guard_doppler; a.tr = (int)p.train_range; a.td = (int)p.train_doppler;
    a.hr = max(1, a.gr + a.tr); a.hd = max(1, a.gd + a.td);
    a.mode = p.mode; a.local_max = (p.flags & RTS_CFAR_LOCAL_MAX) ? 1u : 0u; a.pfa = p.pfa; a.alpha = p.alpha; a.pri = p.pri;
    a.t0 = q.t0; a.dt = q.dt;
    const size_t n_seg = (size_t)q.n_rx * n_doppler * a.n_rt;
    if (n_seg + 1 > 0xffffffffull) { rts_set_error("rts_cube_detect: %zu segments: the map is too large", n_seg); return RTS_ERR_INVALID; }
    a.n_seg = (uint32_t)n_seg; a.max_det = max_det;
    RTS_HIP(c->cube.d_det_cnt.reserve(n_seg + 1)); RTS_HIP(c->cube.d_det_off.reserve(n_seg + 1)); RTS_HIP(c->cube.d_det.reserve(max_det));
    size_t tmp = 0;
    RTS_HIP(rocprim::exclusive_scan(nullptr, tmp, c->cube.d_det_cnt.p, c->cube.d_det_off.p, 0u, n_seg + 1, rocprim::plus<uint32_t>(), c->stream));
    RTS_HIP(c->cube.d_det_tmp.reserve(tmp + 1));
    a.cnt = c->cube.d_det_cnt.p; a.off = c->cube.d_det_off.p; a.out = c->cube.d_det.p;
    const size_t lds = sizeof(double) * ((size_t)(RTS_CFAR_TD + 2 * a.hd) * (RTS_CFAR_TR + 2 * a.hr) + 2 * (size_t)RTS_CFAR_TD * (RTS_CFAR_TR + 2 * a.hr));      // <= 60 KiB
    dim3 grid(a.n_rt, (n_doppler + RTS_CFAR_TD - 1) / RTS_CFAR_TD, q.n_rx);
    k_cfar<false><<<grid, RTS_CFAR_THREADS, lds, c->stream>>>(a);
    RTS_HIP(hipGetLastError());
    RTS_HIP(rocprim::exclusive_scan(c->cube.d_det_tmp.p, tmp, c->cube.d_det_cnt.p, c->cube.d_det_off.p, 0u, n_seg + 1, rocprim::plus<uint32_t>(), c->stream));
    k_cfar<true><<<grid, RTS_CFAR_THREADS, lds, c->stream>>>(a);
    RTS_HIP(hipGetLastError());
    c->cube.det_nseg = (uint32_t)n_seg; c->cube.det_max = max_det; c->cube.det_valid = true;
    return RTS_OK;
}

// --------------------------------------------------------------------------- ordered-statistic CFAR
// The launch shape, the segments, the two passes and the scan between them are k_cfar's; the noise estimate is the k-th smallest of a
// cell's N training powers (rts_cfar_os.h) instead of their mean, so there are no box sums to share between cells:
//   1. P of the tile and its halo into LDS as in k_cfar, but +inf outside [0, n_bins): such a cell is never "below" anything.
//   2. The DECISION needs no selection.  fl(alpha x) does not fall when x rises, so P > alpha x_(k) holds exactly when at least k of the
//      training cells have alpha x_i < P: one multiply, compare and count per training cell, lane <-> range bin, so that consecutive
//      lanes read consecutive doubles of a staged row (8-byte LDS reads without bank conflicts).  Every loop bound is wave-uniform.
//   3. The RECORD needs x_(k) itself, and only the WRITE pass forms it -- it repeats step 2 for the rows of a tile that the COUNT pass
//      found a detection in, and no others -- per detected cell, the wave together: each lane takes up to 18 of
//      the <= 33 x 33 cells of the window's bounding rectangle as 64-bit keys (all ones for the guard and for cells outside the map),
//      and the k-th smallest key is built bit by bit from the top -- the largest t of which fewer than k keys lie below -- with one
//      ballot and population count per key register and bit, the high word first and then the low word of the keys that share it
//      (32-bit compares): 63 x 18 ballots per detection, 63 x 6 for a window of up to 384 cells, none on the common path.
struct RtsCfarOsArgs {
    const double2* map; uint32_t nd, nb, n_rt;
    int gr, gd, tr, td, hr, hd;
    uint32_t rank, n0, local_max; const double* alpha_tab; double alpha, pri, t0, dt;
    uint32_t* cnt; const uint32_t* off; RtsDetection* out; uint32_t max_det, n_seg;
};
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
    __shared__ uint32_t s_row[RTS_CFAR_TD + 2 * RTS_CFAR_MAX_HALF];      // Doppler row of the map behind each staged row (wrapped)
    const uint32_t t = threadIdx.x, lane = t & 63u, wv = t >> 6;
    const uint32_t rt = blockIdx.x, k0 = blockIdx.y * RTS_CFAR_TD, rx = blockIdx.z, r0 = rt * RTS_CFAR_TR;
    const int hr = a.hr, hd = a.hd, gr = a.gr, gd = a.gd, tr = a.tr, td = a.td;
    const int Or = gr + tr, Od = gd + td;
    const uint32_t rowsP = RTS_CFAR_TD + 2 * hd, colsP = RTS_CFAR_TR + 2 * hr;
    if (WRITE) {
        bool any = false;
        if (t < RTS_CFAR_TD && k0 + t < a.nd) any = a.cnt[((size_t)rx * a.nd + k0 + t) * a.n_rt + rt] != 0;
        if (!__syncthreads_or(any)) return;
    } else if (t == 0 && (blockIdx.x | blockIdx.y | blockIdx.z) == 0) {
        a.cnt[a.n_seg] = 0;                          // the scan's extra element: its offset is the total
    }
    double* sP = s_os;
    if (t < rowsP) { const int k = ((int)k0 - hd + (int)t) % (int)a.nd; s_row[t] = (uint32_t)(k < 0 ? k + (int)a.nd : k); }
    __syncthreads();
    // 1. stage P
    const double2* mrx = a.map + (size_t)rx * a.nd * a.nb;
    for (uint32_t e = t; e < rowsP * colsP; e += RTS_CFAR_THREADS) {
        const uint32_t i = e / colsP, cc = e - i * colsP;
        const int r = (int)r0 - hr + (int)cc;
        double p = __builtin_huge_val();
        if (r >= 0 && r < (int)a.nb) { const double2 z = mrx[(size_t)s_row[i] * a.nb + r]; p = z.x * z.x + z.y * z.y; }
        sP[e] = p;
    }
    __syncthreads();
    // 2. per cell: the count of training cells below, the rule, compaction
    const int r = (int)r0 + (int)lane;
    const bool in_map = r < (int)a.nb;
    const int n = in_map ? rts_cfar_os_count(gr, gd, tr, td, r, (int)a.nb - 1 - r) : 1;      // (lanes past the last bin: any count inside the table)
    const uint32_t kth = rts_cfar_os_rank(a.rank, (uint32_t)n, a.n0);
    const double alpha = a.alpha_tab ? a.alpha_tab[n] : a.alpha;
    for (uint32_t i = wv; i < RTS_CFAR_TD; i += RTS_CFAR_THREADS / 64) {
        const uint32_t k = k0 + i;
        if (k >= a.nd) continue;                                        // (wave-uniform: k is the wave's row)
        const size_t seg = ((size_t)rx * a.nd + k) * a.n_rt + rt;
        if (WRITE && a.cnt[seg] == 0) continue;                         // (wave-uniform: the COUNT pass found nothing in this row of the tile)
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
        if (det && a.local_max) {
            for (int dk = -1; dk <= 1; dk++)
                for (int dr = -1; dr <= 1; dr++) {
                    if ((dk == 0 && dr == 0) || r + dr < 0 || r + dr >= (int)a.nb) continue;
                    const double q = p0[dk * (int)colsP + dr];
                    if (dk < 0 || (dk == 0 && dr < 0)) det = det && P > q; else det = det && P >= q;
                }
        }
        const unsigned long long ball = __ballot(det);
        if (!WRITE) { if (lane == 0) a.cnt[seg] = (uint32_t)__popcll(ball); continue; }
        // 3. the order statistic of every detected cell of the row (the loop and everything in it but `noise` is wave-uniform)
        double noise = 0.0;
        const uint32_t W = 2u * (uint32_t)Or + 1u, rect = W * (2u * (uint32_t)Od + 1u);
        for (unsigned long long rest = ball; rest != 0ull; rest &= rest - 1ull) {
            const int src = __ffsll((long long)rest) - 1, rs = (int)r0 + src;
            const double* c0 = sP + (size_t)(i + hd) * colsP + (uint32_t)src + (uint32_t)hr;
            uint32_t khi[RTS_CFAR_OS_KEYS], klo[RTS_CFAR_OS_KEYS];
#pragma unroll
            for (int j = 0; j < RTS_CFAR_OS_KEYS; j++) {
                const uint32_t e = (uint32_t)j * 64u + lane;
                uint64_t key = ~0ull;
                if (e < rect) {
                    const int dk = (int)(e / W) - Od, dr = (int)(e % W) - Or;
                    const bool guard = dk >= -gd && dk <= gd && dr >= -gr && dr <= gr;
                    if (!guard && rs + dr >= 0 && rs + dr < (int)a.nb) key = rts_cfar_os_key(c0[dk * (int)colsP + dr]);
                }
                khi[j] = (uint32_t)(key >> 32); klo[j] = (uint32_t)key;
            }
            const uint32_t ks = rts_cfar_os_rank(a.rank, (uint32_t)rts_cfar_os_count(gr, gd, tr, td, rs, (int)a.nb - 1 - rs), a.n0);
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
        if (!det) continue;
        const uint32_t pos = a.off[seg] + (uint32_t)__popcll(ball & ((1ull << lane) - 1ull));
        if (pos >= a.max_det) continue;
        const double dr_ = rts_cfar_os_delta(r >= 1 ? p0[-1] : 0.0, P, r + 1 < (int)a.nb ? p0[1] : 0.0);
        const double dd_ = rts_cfar_os_delta(p0[-(int)colsP], P, p0[colsP]);
        double w = (double)k + dd_;
        const double half = 0.5 * (double)a.nd;
        if (w >= half) w -= (double)a.nd; else if (w < -half) w += (double)a.nd;
        RtsDetection d;
        d.rx = rx; d.doppler_bin = k; d.range_bin = (uint32_t)r; d.n_train = (uint32_t)n;
        d.power = P; d.noise = noise; d.threshold = alpha * noise; d.range_offset = dr_; d.doppler_offset = dd_;
        d.delay = a.t0 + ((double)r + dr_) * a.dt;
        d.doppler = a.pri > 0.0 ? w / ((double)a.nd * a.pri) : 0.0;
        a.out[pos] = d;
    }
}

int rts_cube_detect_os_device(RtsContext* c, const RtsCfarOsParams& p, const double* alpha_tab, const double* map, uint32_t n_doppler, uint32_t max_det)
{
    const RtsCubeParams& q = c->cube.params;
    RtsCfarOsArgs a;
    a.map = (const double2*)map; a.nd = n_doppler; a.nb = q.n_bins; a.n_rt = (q.n_bins + RTS_CFAR_TR - 1) / RTS_CFAR_TR;
    a.gr = (int)p.guard_range; a.gd = (int)p.guard_doppler; a.tr = (int)p.train_range; a.td = (int)p.train_doppler;
    a.hr = max(1, a.gr + a.tr); a.hd = max(1, a.gd + a.td);
    a.rank = p.rank; a.n0 = rts_cfar_os_n0(p.guard_range, p.guard_doppler, p.train_range, p.train_doppler);
    a.local_max = (p.flags & RTS_CFAR_LOCAL_MAX) ? 1u : 0u; a.alpha_tab = alpha_tab; a.alpha = p.alpha; a.pri = p.pri;
    a.t0 = q.t0; a.dt = q.dt;
    const size_t n_seg = (size_t)q.n_rx * n_doppler * a.n_rt;
    if (n_seg + 1 > 0xffffffffull) { rts_set_error("rts_cube_detect_os: %zu segments: the map is too large", n_seg); return RTS_ERR_INVALID; }
    a.n_seg = (uint32_t)n_seg; a.max_det = max_det;
    RTS_HIP(c->cube.d_det_cnt.reserve(n_seg + 1)); RTS_HIP(c->cube.d_det_off.reserve(n_seg + 1)); RTS_HIP(c->cube.d_det.reserve(max_det));
    size_t tmp = 0;
    RTS_HIP(rocprim::exclusive_scan(nullptr, tmp, c->cube.d_det_cnt.p, c->cube.d_det_off.p, 0u, n_seg + 1, rocprim::plus<uint32_t>(), c->stream));
    RTS_HIP(c->cube.d_det_tmp.reserve(tmp + 1));
    a.cnt = c->cube.d_det_cnt.p; a.off = c->cube.d_det_off.p; a.out = c->cube.d_det.p;
    const size_t lds = sizeof(double) * (size_t)(RTS_CFAR_TD + 2 * a.hd) * (RTS_CFAR_TR + 2 * a.hr);      // <= 36 KiB
    dim3 grid(a.n_rt, (n_doppler + RTS_CFAR_TD - 1) / RTS_CFAR_TD, q.n_rx);
    k_cfar_os<false><<<grid, RTS_CFAR_THREADS, lds, c->stream>>>(a);
    RTS_HIP(hipGetLastError());
    RTS_HIP(rocprim::exclusive_scan(c->cube.d_det_tmp.p, tmp, c->cube.d_det_cnt.p, c->cube.d_det_off.p, 0u, n_seg + 1, rocprim::plus<uint32_t>(), c->stream));
    k_cfar_os<true><<<grid, RTS_CFAR_THREADS, lds, c->stream>>>(a);
    RTS_HIP(hipGetLastError());
    c->cube.det_nseg = (uint32_t)n_seg; c->cube.det_max = max_det; c->cube.det_valid = true;
    return RTS_OK;
}
