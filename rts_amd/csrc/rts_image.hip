// rts_image.hip -- backprojection imaging of the return cube on the device (include/rts_amd.h: rts_cube_backproject).  A gather in
// f64: one thread per pixel of a 256-pixel tile (neighbouring threads read neighbouring range bins of a row), per pulse two square
// roots, the interpolation of the row at the pixel's delay and the carrier phase -- the arithmetic is rts_image.h, shared with the
// host evaluator.  The tile, the receiver and (when the chunks are split, rts_image.h: rts_image_plan) the pulse chunk are on the grid.
#include <hip/hip_runtime.h>
#include "rts_internal.h"
#include "rts_image.h"

struct RtsImageArgs {
    const double* cube; uint32_t n_pulses_cube, n_bins, n_rx; double t0, dt;
    uint32_t n_x, n_y, taps, accumulate, first_pulse, n_pulses, n_chunks, split;
    uint32_t tiles_x, tw_log2;
    double origin[3], step_x[3], step_y[3], cspeed, carrier;
    const double* tx; const double* rx; const double* w;        // [P][3], [n_rx][P][3], [P] (device)
    double2* out; double2* scratch;
};

// blockIdx.x: tile (row-major over the tiles of the image), blockIdx.y: chunk (split) or 0, blockIdx.z: receiver.
// Per chunk the block stages the chunk's transmitter and receiver positions and weights in LDS, then every thread sums its pixel's
// terms of the chunk in ascending pulse order in registers.  Split: the chunk's sum goes to scratch[chunk][rx][iy][ix]
// (k_backproject_sum adds the chunks); otherwise the thread adds its chunk sums in ascending order itself and writes the pixel.
__global__ void __launch_bounds__(RTS_IMAGE_TILE) k_backproject(const RtsImageArgs a)
{
    __shared__ double s_tx[3 * RTS_IMAGE_PULSE_CHUNK], s_rx[3 * RTS_IMAGE_PULSE_CHUNK], s_w[RTS_IMAGE_PULSE_CHUNK];
    const uint32_t t = threadIdx.x, r = blockIdx.z;
    const uint32_t tile_y = blockIdx.x / a.tiles_x, tile_x = blockIdx.x - tile_y * a.tiles_x;
    const uint32_t th_log2 = 8u - a.tw_log2;
    const uint32_t ix = (tile_x << a.tw_log2) + (t & ((1u << a.tw_log2) - 1u)), iy = (tile_y << th_log2) + (t >> a.tw_log2);
    const bool active = ix < a.n_x && iy < a.n_y;
    double x[3]; rts_image_pixel(a.origin, a.step_x, a.step_y, ix, iy, x);
    const RtsImageInterp ip = rts_image_interp_setup(a.taps);
    const uint32_t c0 = a.split ? blockIdx.y : 0u, c1 = a.split ? c0 + 1u : a.n_chunks;
    const double* rows = a.cube + 2 * (((size_t)r * a.n_pulses_cube + a.first_pulse) * a.n_bins);
    double tr = 0.0, ti = 0.0;
    for (uint32_t c = c0; c < c1; c++) {
        const uint32_t j0 = c * RTS_IMAGE_PULSE_CHUNK;
        const uint32_t n = a.n_pulses - j0 < RTS_IMAGE_PULSE_CHUNK ? a.n_pulses - j0 : RTS_IMAGE_PULSE_CHUNK;
        if (c != c0) __syncthreads();
        if (t < 3u * n) { s_tx[t] = a.tx[3 * (size_t)j0 + t]; s_rx[t] = a.rx[3 * ((size_t)r * a.n_pulses + j0) + t]; }
        if (t < n) s_w[t] = a.w[j0 + t];
        __syncthreads();
        if (!active) continue;
        double sr = 0.0, si = 0.0;
        for (uint32_t j = 0; j < n; j++) {
            double er, ei;
            rts_image_term(rows + 2 * ((size_t)(j0 + j) * a.n_bins), a.n_bins, ip, a.t0, a.dt, a.carrier, a.cspeed, s_w[j], x, &s_tx[3 * j], &s_rx[3 * j], &er, &ei);
            sr += er; si += ei;
        }
        if (c == c0) { tr = sr; ti = si; } else { tr += sr; ti += si; }
    }
    if (!active) return;
    const size_t pix = ((size_t)r * a.n_y + iy) * a.n_x + ix;
    if (a.split) { a.scratch[(size_t)c0 * a.n_rx * a.n_y * a.n_x + pix] = make_double2(tr, ti); return; }
    double2 o = make_double2(tr, ti);
    if (a.accumulate) { const double2 p = a.out[pix]; o.x = p.x + tr; o.y = p.y + ti; }
    a.out[pix] = o;
}

// the chunk sums of one pixel added in ascending chunk order, the first one the start value
__global__ void __launch_bounds__(256) k_backproject_sum(const double2* __restrict__ scratch, double2* __restrict__ out, size_t n_pix, uint32_t n_chunks, uint32_t accumulate)
{
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n_pix) return;
    double2 s = scratch[i];
    for (uint32_t c = 1; c < n_chunks; c++) { const double2 v = scratch[(size_t)c * n_pix + i]; s.x += v.x; s.y += v.y; }
    if (accumulate) { const double2 p = out[i]; s.x = p.x + s.x; s.y = p.y + s.y; }
    out[i] = s;
}

// geo: the call's [tx | rx | w] block on the device (rts_cube_api.hip uploads it on the stream before this: RtsCubeState::image.geo)
int rts_cube_backproject_device(RtsContext* c, const RtsImageParams& p, const RtsImagePlan& plan, const double* geo, double* out)
{
    const RtsCubeParams& q = c->cube.params;
    RtsImageArgs a;
    a.cube = c->cube.p; a.n_pulses_cube = q.n_pulses; a.n_bins = q.n_bins; a.n_rx = q.n_rx; a.t0 = q.t0; a.dt = q.dt;
    a.n_x = p.n_x; a.n_y = p.n_y; a.taps = p.taps; a.accumulate = (p.flags & RTS_IMAGE_ACCUMULATE) ? 1u : 0u;
    a.first_pulse = p.first_pulse; a.n_pulses = p.n_pulses; a.n_chunks = plan.n_chunks; a.split = plan.split ? 1u : 0u;
    a.tiles_x = plan.tiles_x; a.tw_log2 = plan.tw_log2;
    for (int k = 0; k < 3; k++) { a.origin[k] = p.origin[k]; a.step_x[k] = p.step_x[k]; a.step_y[k] = p.step_y[k]; }
    a.cspeed = p.cspeed; a.carrier = p.carrier;
    a.tx = geo; a.rx = geo + 3 * (size_t)p.n_pulses; a.w = a.rx + 3 * (size_t)q.n_rx * p.n_pulses;
    a.out = (double2*)out; a.scratch = nullptr;
    if (plan.split) { RTS_HIP(c->cube.image.d_scratch.reserve(2 * plan.scratch)); a.scratch = (double2*)c->cube.image.d_scratch.p; }
    dim3 grid(plan.tiles_x * plan.tiles_y, plan.split ? plan.n_chunks : 1u, q.n_rx);
    k_backproject<<<grid, RTS_IMAGE_TILE, 0, c->stream>>>(a);
    RTS_HIP(hipGetLastError());
    if (plan.split) {
        const size_t n_pix = (size_t)q.n_rx * p.n_y * p.n_x;
        k_backproject_sum<<<(unsigned)((n_pix + 255) / 256), 256, 0, c->stream>>>(a.scratch, a.out, n_pix, plan.n_chunks, a.accumulate);
        RTS_HIP(hipGetLastError());
    }
    return RTS_OK;
}
