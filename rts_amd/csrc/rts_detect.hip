// rts_detect.hip -- the receiver end of the chain on the device (include/rts_amd.h: rts_cube_add_noise, rts_cube_detect):
//   * receiver noise added to rows of the return cube (k_cube_noise; the generator is rts_noise.h, shared with rts_noise_eval)
//   * CFAR detection on a range-Doppler map and the compaction of its detections into one list in flat order (k_cfar)
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
