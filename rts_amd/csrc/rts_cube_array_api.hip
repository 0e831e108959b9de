// rts_cube_array_api.hip -- the cube part of the C-ABI of include/rts_amd.h, the receive array: beamforming and steering, covariance and MVDR, STAP, the
// eigensolver, the DOA scan, rts_doa_weights and rts_source_count, and the pure-host evaluators that go with them.  Host code only, no kernels: argument
// checks, the handle's cube state (RtsCubeState: beam, adapt, stap, doa; rts_cube_state.h), the calls of the launchers in the kernels' units.
#include <cmath>
#include <cstring>
#include <algorithm>
#include "rts_cube_api.h"

// ------------------------------------------------------------------------------------- receive-array beamforming
// (rts_amd.h: RtsBeamParams; the arithmetic and the launch plan are rts_beam.h, shared by the host export and the kernel, rts_beam.hip)
// the record, the limits and the weight table: what needs no source
static int rts_beam_check(const RtsBeamParams* p, uint32_t n_rx, const char* who)
{
    if (!p) { rts_set_error("%s: null parameters", who); return RTS_ERR_INVALID; }
    if (p->reserved[0] || p->reserved[1]) { rts_set_error("%s: reserved fields must be 0", who); return RTS_ERR_INVALID; }
    RTS_TRY(rts_source_known_check(who, p->source));
    if (p->flags & ~(RTS_BEAM_POWER | RTS_BEAM_PEAK)) { rts_set_error("%s: unknown flags 0x%x", who, p->flags); return RTS_ERR_INVALID; }
    if ((p->flags & RTS_BEAM_PEAK) && (p->flags & RTS_BEAM_POWER)) { rts_set_error("%s: flags: RTS_BEAM_PEAK excludes RTS_BEAM_POWER", who); return RTS_ERR_INVALID; }
    if (p->n_beams == 0 || p->n_beams > RTS_BEAM_MAX_BEAMS) { rts_set_error("%s: n_beams = %u (1 .. %u)", who, p->n_beams, RTS_BEAM_MAX_BEAMS); return RTS_ERR_INVALID; }
    if (n_rx > RTS_BEAM_MAX_RX) { rts_set_error("%s: n_rx = %u receivers: more than %u", who, n_rx, RTS_BEAM_MAX_RX); return RTS_ERR_INVALID; }
    if ((uint64_t)p->n_beams * n_rx > RTS_BEAM_MAX_WEIGHTS) { rts_set_error("%s: n_beams * n_rx = %u * %u weights: more than %u (the table sits in a workgroup's LDS)", who, p->n_beams, n_rx, RTS_BEAM_MAX_WEIGHTS); return RTS_ERR_INVALID; }
    if (!p->weights) { rts_set_error("%s: null weights", who); return RTS_ERR_INVALID; }
    for (uint32_t i = 0; i < 2 * p->n_beams * n_rx; i++) if (!std::isfinite(p->weights[i])) { rts_set_error("%s: weights[%u][%u] is not finite", who, i / 2 / n_rx, i / 2 % n_rx); return RTS_ERR_INVALID; }
    return rts_source_fields_check(who, p->source, p->n_rows_in, p->device_in);
}
// the span inside the source's rows, and the plan of its launch
static int rts_beam_rows_check(const RtsBeamParams* p, uint32_t rows, uint32_t n_rx, uint32_t n_bins, const char* who, RtsBeamPlan* plan)
{
    uint32_t n_rows = 0;
    RTS_TRY(rts_rows_check(who, p->first_row, p->n_rows, rows, &n_rows));
    *plan = rts_beam_plan(n_rx, p->n_beams, n_rows, n_bins, p->flags);
    if (!plan->supported) { rts_set_error("%s: %llu cells (n_rows * n_bins), %u per workgroup: more than %u workgroups (the launch grid)", who, (unsigned long long)plan->cells, RTS_BEAM_THREADS, RTS_BEAM_MAX_GRID_X); return RTS_ERR_INVALID; }
    return RTS_OK;
}

extern "C" int rts_beamform_eval(const RtsCubeParams* q, const double* in, uint32_t n_rows_in, const RtsBeamParams* p, double* out)
{
    RTS_TRY(rts_eval_cube_check("rts_beamform_eval", q, false, false));
    if (n_rows_in == 0) { rts_set_error("rts_beamform_eval: n_rows_in = 0"); return RTS_ERR_INVALID; }
    RTS_TRY(rts_beam_check(p, q->n_rx, "rts_beamform_eval"));
    RTS_TRY(rts_source_rows_match_check("rts_beamform_eval", p->source, p->n_rows_in, n_rows_in));
    RtsBeamPlan plan;
    RTS_TRY(rts_beam_rows_check(p, n_rows_in, q->n_rx, q->n_bins, "rts_beamform_eval", &plan));
    if (!in || !out) { rts_set_error("rts_beamform_eval: null input or output array"); return RTS_ERR_INVALID; }
    rts_beam_eval_host(q->n_rx, q->n_bins, in, n_rows_in, p->first_row, (uint32_t)(plan.cells / q->n_bins), p->n_beams, p->weights, p->flags, out);
    return RTS_OK;
}

extern "C" int rts_steering_make(const double* positions, uint32_t n_rx, const double* directions, uint32_t n_beams, double wavelength, const double* taper, double* weights_out)
{
    if (!positions || !directions || !weights_out) { rts_set_error("rts_steering_make: null positions, directions or output array"); return RTS_ERR_INVALID; }
    if (n_rx == 0 || n_beams == 0) { rts_set_error("rts_steering_make: n_rx = %u, n_beams = %u (each >= 1)", n_rx, n_beams); return RTS_ERR_INVALID; }
    if (!std::isfinite(wavelength) || !(wavelength > 0.0)) { rts_set_error("rts_steering_make: wavelength = %g (finite, > 0)", wavelength); return RTS_ERR_INVALID; }
    for (size_t i = 0; i < 3 * (size_t)n_rx; i++) if (!std::isfinite(positions[i])) { rts_set_error("rts_steering_make: position of receiver %zu is not finite", i / 3); return RTS_ERR_INVALID; }
    for (size_t i = 0; i < 2 * (size_t)n_beams; i++) if (!std::isfinite(directions[i])) { rts_set_error("rts_steering_make: direction of beam %zu is not finite", i / 2); return RTS_ERR_INVALID; }
    if (taper) for (uint32_t r = 0; r < n_rx; r++) if (!std::isfinite(taper[r])) { rts_set_error("rts_steering_make: taper[%u] is not finite", r); return RTS_ERR_INVALID; }
    for (uint32_t b = 0; b < n_beams; b++) {
        const double az = directions[2 * (size_t)b], el = directions[2 * (size_t)b + 1];
        const double ce = cos(el), ux = ce * cos(az), uy = ce * sin(az), uz = sin(el);
        for (uint32_t r = 0; r < n_rx; r++) {
            const double* pos = positions + 3 * (size_t)r;
            const double x = ((ux * pos[0] + uy * pos[1]) + uz * pos[2]) / wavelength;
            double s, cs; rts_beat_sincos_turns(x, &s, &cs);      // f = x - floor(x), the exact reflections, then libm: the host side of the transforms' twiddles
            double* w = weights_out + 2 * ((size_t)b * n_rx + r);
            if (taper) { w[0] = taper[r] * cs; w[1] = taper[r] * s; } else { w[0] = cs; w[1] = s; }
        }
    }
    return RTS_OK;
}

extern "C" int rts_cube_beamform(RtsHandle c, const RtsBeamParams* p, void* device_out)
{
    CHECK_HANDLE(c);
    NEED_CUBE(c, "rts_cube_beamform", "no cube (call rts_cube_attach first)");
    const RtsCubeParams& q = c->cube.params;
    RTS_TRY(rts_beam_check(p, q.n_rx, "rts_cube_beamform"));
    const double* src; uint32_t rows;
    RTS_TRY(rts_device_source(c, "rts_cube_beamform", p->source, p->device_in, p->n_rows_in, &src, &rows));
    RtsBeamPlan plan;
    RTS_TRY(rts_beam_rows_check(p, rows, q.n_rx, q.n_bins, "rts_cube_beamform", &plan));
    if ((uintptr_t)device_out & 15u) { rts_set_error("rts_cube_beamform: device_out is not 16-byte aligned"); return RTS_ERR_INVALID; }
    const uint64_t rx_stride = (uint64_t)rows * q.n_bins;
    const double* in = src + 2 * (size_t)p->first_row * q.n_bins;
    RTS_TRY(rts_output_apart_check("rts_cube_beamform", "%s: device_out overlaps the input the call reads (receiver %u): the transform is not in place", device_out, plan.out_doubles, in, rx_stride, 0u, plan.cells, q.n_rx));
    CHECK_CLOSED(c);
    double* out; RTS_HIP(c->cube.beam.out.place(device_out, plan.out_doubles, &out));
    // the weights -> pinned staging -> the device, on the stream (n_beams n_rx <= RTS_BEAM_MAX_WEIGHTS: one size for every call)
    RTS_HIP(c->cube.beam.w.upload(p->weights, 2 * (size_t)p->n_beams * q.n_rx, 2u * RTS_BEAM_MAX_WEIGHTS, c->stream));
    if (!device_out) c->cube.beam.out.record(out, plan.out_doubles);
    return rts_cube_beam_device(c, *p, plan, in, rx_stride, c->cube.beam.w.dev.p, out);
}

extern "C" int rts_cube_beam_get(RtsHandle c, double* host_out, uint64_t capacity_doubles)
{
    CHECK_HANDLE(c);
    return rts_cube_copy_out(c, "rts_cube_beam_get", "no library-owned beams (rts_cube_beamform with device_out NULL; the beams end at rts_cube_attach) / null output", c->cube.beam.out, host_out, capacity_doubles);
}

// ------------------------------------------------------------------------------------- adaptive (MVDR) beamforming
// (rts_amd.h: RtsCovParams, RtsMvdrParams; the trees and the launch plans are rts_adapt.h, shared by the host exports and the kernels, rts_adapt.hip)
// the record: what needs no source
static int rts_cov_check(const RtsCovParams* p, uint32_t n_rx, const char* who)
{
    if (!p) { rts_set_error("%s: null parameters", who); return RTS_ERR_INVALID; }
    if (p->reserved[0] || p->reserved[1]) { rts_set_error("%s: reserved fields must be 0", who); return RTS_ERR_INVALID; }
    RTS_TRY(rts_source_known_check(who, p->source));
    if (n_rx > RTS_BEAM_MAX_RX) { rts_set_error("%s: n_rx = %u receivers: more than %u", who, n_rx, RTS_BEAM_MAX_RX); return RTS_ERR_INVALID; }
    return rts_source_fields_check(who, p->source, p->n_rows_in, p->device_in);
}
// the training set inside the source's rows and bins, and the plan of its launches.  n_taps 1: the receivers' covariance; more: the
// stacked one (rts_stap.h) -- the span holds n_taps - 1 fewer start rows than rows, the matrix is of order n_taps n_rx
static int rts_cov_set_check(const RtsCovParams* p, uint32_t rows, uint32_t n_rx, uint32_t nb, const char* who, RtsCovSet* set, RtsCovPlan* plan, uint32_t n_taps = 1u)
{
    uint32_t span = 0;
    RTS_TRY(rts_rows_check(who, p->first_row, p->n_rows, rows, &set->n_rows));
    RTS_TRY(rts_gate_check(who, "%s: first_bin = %u, n_bins = %u: inside the source's %u bins", p->first_bin, p->n_bins, nb, &span));
    if (p->skip_n_bins == 0 && p->skip_first_bin != 0) { rts_set_error("%s: skip_first_bin = %u with skip_n_bins = 0", who, p->skip_first_bin); return RTS_ERR_INVALID; }
    if (p->skip_n_bins != 0 && (p->skip_first_bin < p->first_bin || p->skip_first_bin - p->first_bin >= span || p->skip_n_bins > span - (p->skip_first_bin - p->first_bin))) {
        rts_set_error("%s: skip_first_bin = %u, skip_n_bins = %u: inside the bins %u .. %u + %u", who, p->skip_first_bin, p->skip_n_bins, p->first_bin, p->first_bin, span); return RTS_ERR_INVALID; }
    if (p->skip_n_bins == span) { rts_set_error("%s: skip_n_bins = %u leaves no bin of the span's %u", who, p->skip_n_bins, span); return RTS_ERR_INVALID; }
    set->first_row = p->first_row; set->first_bin = p->first_bin;
    set->kept = span - p->skip_n_bins; set->skip_n = p->skip_n_bins; set->skip_at = p->skip_n_bins ? p->skip_first_bin - p->first_bin : set->kept;
    if (set->n_rows < n_taps) { rts_set_error("%s: n_rows = %u rows hold no snapshot of n_taps = %u", who, set->n_rows, n_taps); return RTS_ERR_INVALID; }
    set->n_rows -= n_taps - 1u;
    *plan = rts_cov_plan(n_rx * n_taps, set->n_rows, set->kept);
    if (!plan->supported) { rts_set_error("%s: %llu training cells (n_rows * kept bins) in tiles of %u: more than %llu tiles", who, (unsigned long long)plan->K, RTS_ADAPT_TILE, RTS_ADAPT_MAX_TILES); return RTS_ERR_INVALID; }
    return RTS_OK;
}

extern "C" int rts_covariance_eval(const RtsCubeParams* q, const double* in, uint32_t n_rows_in, const RtsCovParams* p, double* out)
{
    RTS_TRY(rts_eval_cube_check("rts_covariance_eval", q, false, false));
    if (n_rows_in == 0) { rts_set_error("rts_covariance_eval: n_rows_in = 0"); return RTS_ERR_INVALID; }
    RTS_TRY(rts_cov_check(p, q->n_rx, "rts_covariance_eval"));
    RTS_TRY(rts_source_rows_match_check("rts_covariance_eval", p->source, p->n_rows_in, n_rows_in));
    RtsCovSet set; RtsCovPlan plan;
    RTS_TRY(rts_cov_set_check(p, n_rows_in, q->n_rx, q->n_bins, "rts_covariance_eval", &set, &plan));
    if (!in || !out) { rts_set_error("rts_covariance_eval: null input or output array"); return RTS_ERR_INVALID; }
    rts_cov_eval_host(q->n_rx, q->n_bins, in, n_rows_in, set, plan, out);
    return RTS_OK;
}

extern "C" int rts_cube_covariance(RtsHandle c, const RtsCovParams* p, void* device_out)
{
    CHECK_HANDLE(c);
    NEED_CUBE(c, "rts_cube_covariance", "no cube (call rts_cube_attach first)");
    const RtsCubeParams& q = c->cube.params;
    RTS_TRY(rts_cov_check(p, q.n_rx, "rts_cube_covariance"));
    const double* src; uint32_t rows;
    RTS_TRY(rts_device_source(c, "rts_cube_covariance", p->source, p->device_in, p->n_rows_in, &src, &rows));
    RtsCovSet set; RtsCovPlan plan;
    RTS_TRY(rts_cov_set_check(p, rows, q.n_rx, q.n_bins, "rts_cube_covariance", &set, &plan));
    if ((uintptr_t)device_out & 15u) { rts_set_error("rts_cube_covariance: device_out is not 16-byte aligned"); return RTS_ERR_INVALID; }
    const uint64_t rx_stride = (uint64_t)rows * q.n_bins;
    // the output's bytes against each receiver's span of the input: its first training cell .. its last
    RTS_TRY(rts_output_apart_check("rts_cube_covariance", "%s: device_out overlaps the input the call reads (receiver %u)", device_out, plan.out_doubles, src, rx_stride, rts_cov_cell_index(set, q.n_bins, 0),
                                   rts_cov_cell_index(set, q.n_bins, plan.K - 1u) + 1u, q.n_rx));
    CHECK_CLOSED(c);
    double* out; RTS_HIP(c->cube.adapt.cov.place(device_out, plan.out_doubles, &out));
    RTS_HIP(c->cube.adapt.d_cov_part.reserve(plan.scratch_bytes / sizeof(double)));
    if (!device_out) { c->cube.adapt.cov.record(out, plan.out_doubles); c->cube.adapt.cov_n = q.n_rx; }
    return rts_cube_cov_device(c, set, plan, 1u, src, rx_stride, c->cube.adapt.d_cov_part.p, out);
}

extern "C" int rts_cube_covariance_get(RtsHandle c, double* host_out, uint64_t capacity_doubles)
{
    CHECK_HANDLE(c);
    return rts_cube_copy_out(c, "rts_cube_covariance_get", "no library-owned covariance (rts_cube_covariance with device_out NULL; a covariance ends at rts_cube_attach) / null output", c->cube.adapt.cov, host_out, capacity_doubles);
}

// the record, the limits and the steering rows of a solve over n_rx receivers
static int rts_mvdr_check(const RtsMvdrParams* p, uint32_t n_rx, const char* who, RtsMvdrPlan* plan)
{
    if (p->reserved[0] || p->reserved[1]) { rts_set_error("%s: reserved fields must be 0", who); return RTS_ERR_INVALID; }
    if (n_rx == 0 || n_rx > RTS_BEAM_MAX_RX) { rts_set_error("%s: n_rx = %u receivers (1 .. %u)", who, n_rx, RTS_BEAM_MAX_RX); return RTS_ERR_INVALID; }
    if (p->n_beams == 0 || p->n_beams > RTS_BEAM_MAX_BEAMS) { rts_set_error("%s: n_beams = %u (1 .. %u)", who, p->n_beams, RTS_BEAM_MAX_BEAMS); return RTS_ERR_INVALID; }
    if ((uint64_t)p->n_beams * n_rx > RTS_BEAM_MAX_WEIGHTS) { rts_set_error("%s: n_beams * n_rx = %u * %u weights: more than %u (a weight table of rts_cube_beamform)", who, p->n_beams, n_rx, RTS_BEAM_MAX_WEIGHTS); return RTS_ERR_INVALID; }
    if (!std::isfinite(p->loading) || p->loading < 0) { rts_set_error("%s: loading = %g (finite, >= 0)", who, p->loading); return RTS_ERR_INVALID; }
    if (!p->steering) { rts_set_error("%s: null steering", who); return RTS_ERR_INVALID; }
    for (uint32_t i = 0; i < 2 * p->n_beams * n_rx; i++) if (!std::isfinite(p->steering[i])) { rts_set_error("%s: steering[%u][%u] is not finite", who, i / 2 / n_rx, i / 2 % n_rx); return RTS_ERR_INVALID; }
    *plan = rts_mvdr_plan(n_rx, p->n_beams);
    if (!plan->supported) { rts_set_error("%s: n_rx = %u, n_beams = %u: beyond the solve's plan", who, n_rx, p->n_beams); return RTS_ERR_INVALID; }
    return RTS_OK;
}

extern "C" int rts_mvdr_eval(const double* cov, uint32_t n_rx, const RtsMvdrParams* p, double* out)
{
    if (!p) { rts_set_error("rts_mvdr_eval: null parameters"); return RTS_ERR_INVALID; }
    if (p->n_rx != n_rx) { rts_set_error("rts_mvdr_eval: the parameters' n_rx = %u, the array's %u", p->n_rx, n_rx); return RTS_ERR_INVALID; }
    RtsMvdrPlan plan;
    RTS_TRY(rts_mvdr_check(p, n_rx, "rts_mvdr_eval", &plan));
    if (!cov || !out) { rts_set_error("rts_mvdr_eval: null covariance or output array"); return RTS_ERR_INVALID; }
    std::vector<double> L(2 * (size_t)n_rx * n_rx), x(2 * (size_t)n_rx), w(plan.out_doubles);
    const int pivot = rts_mvdr_eval_host(cov, n_rx, p->n_beams, p->steering, p->loading, L.data(), x.data(), w.data());
    if (pivot >= 0) { rts_set_error("rts_mvdr_eval: the solve failed at pivot %d (not finite or not > 0: the covariance plus loading is not positive definite)", pivot); return RTS_ERR_INVALID; }
    memcpy(out, w.data(), sizeof(double) * plan.out_doubles);
    return RTS_OK;
}

extern "C" int rts_cube_mvdr(RtsHandle c, const RtsMvdrParams* p, void* device_out)
{
    CHECK_HANDLE(c);
    NEED_CUBE(c, "rts_cube_mvdr", "no cube (call rts_cube_attach first)");
    if (!p) { rts_set_error("rts_cube_mvdr: null parameters"); return RTS_ERR_INVALID; }
    const double* cov; uint32_t n_rx = p->n_rx;
    RTS_TRY(rts_pointer_or_owned("rts_cube_mvdr", p->device_cov, c->cube.adapt.cov, c->cube.adapt.cov_n, "%s: device_cov is not 16-byte aligned",
                                 "%s: no covariance (rts_cube_covariance with device_out NULL first, or pass device_cov)", "%s: n_rx = %u, the library-owned covariance's %u (or 0)", &cov, &n_rx));
    RtsMvdrPlan plan;
    RTS_TRY(rts_mvdr_check(p, n_rx, "rts_cube_mvdr", &plan));
    if ((uintptr_t)device_out & 15u) { rts_set_error("rts_cube_mvdr: device_out is not 16-byte aligned"); return RTS_ERR_INVALID; }
    if (device_out && rts_bytes_overlap(device_out, sizeof(double) * plan.out_doubles, cov, 16u * (size_t)n_rx * n_rx)) { rts_set_error("rts_cube_mvdr: device_out overlaps the covariance the call reads"); return RTS_ERR_INVALID; }
    CHECK_CLOSED(c);
    double* out; RTS_HIP(c->cube.adapt.mvdr.place(device_out, plan.out_doubles, &out));
    RTS_HIP(c->cube.adapt.d_mvdr_status.reserve(2));
    // the steering rows -> pinned staging -> the device, on the stream (n_beams n_rx <= RTS_BEAM_MAX_WEIGHTS: one size for every call)
    RTS_HIP(c->cube.adapt.mvdr_s.upload(p->steering, plan.out_doubles, 2u * RTS_BEAM_MAX_WEIGHTS, c->stream));
    if (!device_out) c->cube.adapt.mvdr.record(out, plan.out_doubles);
    return rts_cube_mvdr_device(c, plan, n_rx, p->n_beams, p->loading, cov, c->cube.adapt.mvdr_s.dev.p, c->cube.adapt.d_mvdr_status.p + (device_out ? 1 : 0), out);
}

extern "C" int rts_cube_mvdr_get(RtsHandle c, double* host_out, uint64_t capacity_doubles)
{
    CHECK_HANDLE(c);
    const RtsCubeProduct& m = c->cube.adapt.mvdr;
    if (!c->cube.set || !m.valid || !host_out) { rts_set_error("rts_cube_mvdr_get: no library-owned weights (rts_cube_mvdr with device_out NULL; the weights end at rts_cube_attach) / null output"); return RTS_ERR_INVALID; }
    if (capacity_doubles < m.doubles) { rts_set_error("rts_cube_mvdr_get: capacity too small"); return RTS_ERR_CAPACITY; }
    uint32_t status = 0;
    RTS_TRY(rts_status_word(c, c->cube.adapt.d_mvdr_status.p, &status));
    if (status) { rts_set_error("rts_cube_mvdr_get: the solve failed at pivot %u (not finite or not > 0: the covariance plus loading is not positive definite); every weight is NaN", status - 1u); return RTS_ERR_INVALID; }
    RTS_HIP(hipMemcpy(host_out, m.p, sizeof(double) * m.doubles, hipMemcpyDeviceToHost));
    return RTS_OK;
}

// ------------------------------------------------------------------------------------- space-time adaptive processing
// (rts_amd.h: RtsStCovParams, RtsStApplyParams; the snapshot, the evaluators and the filter's launch plan are rts_stap.h; the covariance's checks, tree,
// plan and kernels are the adaptive beamformer's, above, with n_taps; its library-owned result is the handle's `cov`, of order n_taps n_rx)
static int rts_st_taps_check(const char* who, uint32_t n_taps, uint32_t reserved0, uint32_t n_rx)
{
    if (reserved0) { rts_set_error("%s: reserved fields must be 0", who); return RTS_ERR_INVALID; }
    if (n_taps == 0 || n_taps > RTS_ST_MAX_TAPS) { rts_set_error("%s: n_taps = %u (1 .. %u)", who, n_taps, RTS_ST_MAX_TAPS); return RTS_ERR_INVALID; }
    if ((uint64_t)n_taps * n_rx > RTS_BEAM_MAX_RX) { rts_set_error("%s: n_taps * n_rx = %u * %u: a snapshot of more than %u entries", who, n_taps, n_rx, RTS_BEAM_MAX_RX); return RTS_ERR_INVALID; }
    return RTS_OK;
}
// the record's shared fields as the covariance's record
static RtsCovParams rts_st_cov_fields(const RtsStCovParams* p)
{
    RtsCovParams s = {};
    s.source = p->source; s.n_rows_in = p->n_rows_in; s.first_row = p->first_row; s.n_rows = p->n_rows; s.first_bin = p->first_bin; s.n_bins = p->n_bins;
    s.skip_first_bin = p->skip_first_bin; s.skip_n_bins = p->skip_n_bins; s.device_in = p->device_in; s.reserved[0] = p->reserved[0]; s.reserved[1] = p->reserved[1];
    return s;
}

extern "C" int rts_st_covariance_eval(const RtsCubeParams* q, const double* in, uint32_t n_rows_in, const RtsStCovParams* p, double* out)
{
    const char* who = "rts_st_covariance_eval";
    RTS_TRY(rts_eval_cube_check(who, q, false, false));
    if (n_rows_in == 0) { rts_set_error("%s: n_rows_in = 0", who); return RTS_ERR_INVALID; }
    if (!p) { rts_set_error("%s: null parameters", who); return RTS_ERR_INVALID; }
    const RtsCovParams s = rts_st_cov_fields(p);
    RTS_TRY(rts_cov_check(&s, q->n_rx, who));
    RTS_TRY(rts_st_taps_check(who, p->n_taps, p->reserved0, q->n_rx));
    RTS_TRY(rts_source_rows_match_check(who, p->source, p->n_rows_in, n_rows_in));
    RtsCovSet set; RtsCovPlan plan;
    RTS_TRY(rts_cov_set_check(&s, n_rows_in, q->n_rx, q->n_bins, who, &set, &plan, p->n_taps));
    if (!in || !out) { rts_set_error("%s: null input or output array", who); return RTS_ERR_INVALID; }
    rts_st_cov_eval_host(q->n_rx, p->n_taps, q->n_bins, in, n_rows_in, set, plan, out);
    return RTS_OK;
}

extern "C" int rts_cube_st_covariance(RtsHandle c, const RtsStCovParams* p, void* device_out)
{
    const char* who = "rts_cube_st_covariance";
    CHECK_HANDLE(c);
    NEED_CUBE(c, who, "no cube (call rts_cube_attach first)");
    if (!p) { rts_set_error("%s: null parameters", who); return RTS_ERR_INVALID; }
    const RtsCubeParams& q = c->cube.params;
    const RtsCovParams s = rts_st_cov_fields(p);
    RTS_TRY(rts_cov_check(&s, q.n_rx, who));
    RTS_TRY(rts_st_taps_check(who, p->n_taps, p->reserved0, q.n_rx));
    const double* src; uint32_t rows;
    RTS_TRY(rts_device_source(c, who, p->source, p->device_in, p->n_rows_in, &src, &rows));
    RtsCovSet set; RtsCovPlan plan;
    RTS_TRY(rts_cov_set_check(&s, rows, q.n_rx, q.n_bins, who, &set, &plan, p->n_taps));
    if ((uintptr_t)device_out & 15u) { rts_set_error("%s: device_out is not 16-byte aligned", who); return RTS_ERR_INVALID; }
    const uint64_t rx_stride = (uint64_t)rows * q.n_bins;
    // the output's bytes against each receiver's span of the input: the first snapshot's first cell .. the last one's last tap
    RTS_TRY(rts_output_apart_check(who, "%s: device_out overlaps the input the call reads (receiver %u)", device_out, plan.out_doubles, src, rx_stride, rts_cov_cell_index(set, q.n_bins, 0),
                                   rts_cov_cell_index(set, q.n_bins, plan.K - 1u) + (uint64_t)(p->n_taps - 1u) * q.n_bins + 1u, q.n_rx));
    CHECK_CLOSED(c);
    double* out; RTS_HIP(c->cube.adapt.cov.place(device_out, plan.out_doubles, &out));
    RTS_HIP(c->cube.adapt.d_cov_part.reserve(plan.scratch_bytes / sizeof(double)));
    if (!device_out) { c->cube.adapt.cov.record(out, plan.out_doubles); c->cube.adapt.cov_n = q.n_rx * p->n_taps; }
    return rts_cube_cov_device(c, set, plan, p->n_taps, src, rx_stride, c->cube.adapt.d_cov_part.p, out);
}

// the filter's record, limits and weight table: what needs no source
static int rts_st_apply_check(const RtsStApplyParams* p, uint32_t n_rx, const char* who)
{
    if (!p) { rts_set_error("%s: null parameters", who); return RTS_ERR_INVALID; }
    if (p->reserved[0] || p->reserved[1]) { rts_set_error("%s: reserved fields must be 0", who); return RTS_ERR_INVALID; }
    RTS_TRY(rts_source_known_check(who, p->source));
    if (p->flags & ~RTS_BEAM_POWER) { rts_set_error("%s: unknown flags 0x%x (RTS_BEAM_POWER)", who, p->flags); return RTS_ERR_INVALID; }
    RTS_TRY(rts_st_taps_check(who, p->n_taps, p->reserved0, n_rx));
    const uint32_t D = p->n_taps * n_rx;
    if (p->n_filters == 0 || p->n_filters > RTS_BEAM_MAX_BEAMS) { rts_set_error("%s: n_filters = %u (1 .. %u)", who, p->n_filters, RTS_BEAM_MAX_BEAMS); return RTS_ERR_INVALID; }
    if ((uint64_t)p->n_filters * D > RTS_BEAM_MAX_WEIGHTS) { rts_set_error("%s: n_filters * n_taps * n_rx = %u * %u weights: more than %u (a weight table of rts_cube_beamform)", who, p->n_filters, D, RTS_BEAM_MAX_WEIGHTS); return RTS_ERR_INVALID; }
    if (!p->weights) { rts_set_error("%s: null weights", who); return RTS_ERR_INVALID; }
    for (uint32_t i = 0; i < 2 * p->n_filters * D; i++) if (!std::isfinite(p->weights[i])) { rts_set_error("%s: weights[%u][%u] is not finite", who, i / 2 / D, i / 2 % D); return RTS_ERR_INVALID; }
    return rts_source_fields_check(who, p->source, p->n_rows_in, p->device_in);
}
// the span inside the source's rows, and the plan of its launch
static int rts_st_apply_rows_check(const RtsStApplyParams* p, uint32_t rows, uint32_t n_rx, uint32_t n_bins, const char* who, RtsStApplyPlan* plan)
{
    uint32_t n_rows = 0;
    RTS_TRY(rts_rows_check(who, p->first_row, p->n_rows, rows, &n_rows));
    if (n_rows < p->n_taps) { rts_set_error("%s: n_rows = %u rows hold no snapshot of n_taps = %u", who, n_rows, p->n_taps); return RTS_ERR_INVALID; }
    *plan = rts_st_apply_plan(n_rx, p->n_taps, p->n_filters, n_rows, n_bins, p->flags);
    if (!plan->supported) { rts_set_error("%s: n_rows = %u, n_bins = %u, n_filters = %u: more than %u workgroups (the launch grid)", who, n_rows, n_bins, p->n_filters, RTS_ST_MAX_GRID_X); return RTS_ERR_INVALID; }
    return RTS_OK;
}

extern "C" int rts_st_apply_eval(const RtsCubeParams* q, const double* in, uint32_t n_rows_in, const RtsStApplyParams* p, double* out)
{
    const char* who = "rts_st_apply_eval";
    RTS_TRY(rts_eval_cube_check(who, q, false, false));
    if (n_rows_in == 0) { rts_set_error("%s: n_rows_in = 0", who); return RTS_ERR_INVALID; }
    RTS_TRY(rts_st_apply_check(p, q->n_rx, who));
    RTS_TRY(rts_source_rows_match_check(who, p->source, p->n_rows_in, n_rows_in));
    RtsStApplyPlan plan;
    RTS_TRY(rts_st_apply_rows_check(p, n_rows_in, q->n_rx, q->n_bins, who, &plan));
    if (!in || !out) { rts_set_error("%s: null input or output array", who); return RTS_ERR_INVALID; }
    rts_st_apply_eval_host(q->n_rx, p->n_taps, q->n_bins, in, n_rows_in, p->first_row, plan.out_rows + p->n_taps - 1u, p->n_filters, p->weights, p->flags, out);
    return RTS_OK;
}

extern "C" int rts_st_steering_make(const double* spatial, uint32_t n_rx, uint32_t n_beams, const double* doppler, uint32_t n_doppler, uint32_t n_taps, const double* tap_taper, double* out)
{
    const char* who = "rts_st_steering_make";
    if (!spatial || !doppler || !out) { rts_set_error("%s: null spatial, doppler or output array", who); return RTS_ERR_INVALID; }
    if (n_rx == 0 || n_beams == 0 || n_doppler == 0) { rts_set_error("%s: n_rx = %u, n_beams = %u, n_doppler = %u (each >= 1)", who, n_rx, n_beams, n_doppler); return RTS_ERR_INVALID; }
    RTS_TRY(rts_st_taps_check(who, n_taps, 0u, n_rx));
    for (size_t i = 0; i < 2 * (size_t)n_beams * n_rx; i++) if (!std::isfinite(spatial[i])) { rts_set_error("%s: spatial[%zu][%zu] is not finite", who, i / 2 / n_rx, i / 2 % n_rx); return RTS_ERR_INVALID; }
    for (uint32_t k = 0; k < n_doppler; k++) if (!std::isfinite(doppler[k])) { rts_set_error("%s: doppler[%u] is not finite", who, k); return RTS_ERR_INVALID; }
    if (tap_taper) for (uint32_t m = 0; m < n_taps; m++) if (!std::isfinite(tap_taper[m])) { rts_set_error("%s: tap_taper[%u] is not finite", who, m); return RTS_ERR_INVALID; }
    const uint32_t D = n_taps * n_rx;
    for (uint32_t b = 0; b < n_beams; b++) for (uint32_t k = 0; k < n_doppler; k++) for (uint32_t m = 0; m < n_taps; m++) {
        double s, cs; rts_beat_sincos_turns(doppler[k] * (double)m, &s, &cs);      // (rts_steering_make's cosine and sine)
        const double tr = tap_taper ? tap_taper[m] * cs : cs, ti = tap_taper ? tap_taper[m] * s : s;
        for (uint32_t r = 0; r < n_rx; r++) {
            const double* a = spatial + 2 * ((size_t)b * n_rx + r);
            double* o = out + 2 * (((size_t)b * n_doppler + k) * D + (size_t)m * n_rx + r);
            rts_st_steer_mul(tr, ti, a[0], a[1], &o[0], &o[1]);
        }
    }
    return RTS_OK;
}

extern "C" int rts_cube_st_apply(RtsHandle c, const RtsStApplyParams* p, void* device_out)
{
    const char* who = "rts_cube_st_apply";
    CHECK_HANDLE(c);
    NEED_CUBE(c, who, "no cube (call rts_cube_attach first)");
    const RtsCubeParams& q = c->cube.params;
    RTS_TRY(rts_st_apply_check(p, q.n_rx, who));
    const double* src; uint32_t rows;
    RTS_TRY(rts_device_source(c, who, p->source, p->device_in, p->n_rows_in, &src, &rows));
    RtsStApplyPlan plan;
    RTS_TRY(rts_st_apply_rows_check(p, rows, q.n_rx, q.n_bins, who, &plan));
    if ((uintptr_t)device_out & 15u) { rts_set_error("%s: device_out is not 16-byte aligned", who); return RTS_ERR_INVALID; }
    const uint64_t rx_stride = (uint64_t)rows * q.n_bins;
    const double* in = src + 2 * (size_t)p->first_row * q.n_bins;
    RTS_TRY(rts_output_apart_check(who, "%s: device_out overlaps the input the call reads (receiver %u): the filter is not in place", device_out, plan.out_doubles, in, rx_stride, 0u,
                                   (uint64_t)(plan.out_rows + p->n_taps - 1u) * q.n_bins, q.n_rx));
    CHECK_CLOSED(c);
    double* out; RTS_HIP(c->cube.stap.out.place(device_out, plan.out_doubles, &out));
    // the weights -> pinned staging -> the device, on the stream (n_filters D <= RTS_BEAM_MAX_WEIGHTS: one size for every call)
    RTS_HIP(c->cube.stap.w.upload(p->weights, 2 * (size_t)p->n_filters * plan.D, 2u * RTS_BEAM_MAX_WEIGHTS, c->stream));
    if (!device_out) c->cube.stap.out.record(out, plan.out_doubles);
    return rts_cube_st_apply_device(c, *p, plan, in, rx_stride, c->cube.stap.w.dev.p, out);
}

extern "C" int rts_cube_st_get(RtsHandle c, double* host_out, uint64_t capacity_doubles)
{
    CHECK_HANDLE(c);
    return rts_cube_copy_out(c, "rts_cube_st_get", "no library-owned filter output (rts_cube_st_apply with device_out NULL; the output ends at rts_cube_attach) / null output", c->cube.stap.out, host_out, capacity_doubles);
}

// ------------------------------------------------------------------------------------- direction finding
// (rts_amd.h: RtsEigParams, RtsDoaScanParams; the trees and the launch plans are rts_doa.h, shared by the host exports and the kernels, rts_doa.hip)
extern "C" int rts_eig_eval(const double* cov, uint32_t n, double* values_out, double* vectors_out, uint32_t* sweeps_out)
{
    const RtsEigPlan plan = rts_eig_plan(n);
    if (!plan.supported) { rts_set_error("rts_eig_eval: n = %u (1 .. %u)", n, RTS_BEAM_MAX_RX); return RTS_ERR_INVALID; }
    if (!cov || !values_out || !vectors_out) { rts_set_error("rts_eig_eval: null covariance or output array"); return RTS_ERR_INVALID; }
    std::vector<double> X(plan.vector_doubles), V(plan.vector_doubles), lambda(n), values(n), vectors(plan.vector_doubles);
    uint32_t sweeps = 0;
    const uint32_t status = rts_eig_eval_host(cov, n, X.data(), V.data(), lambda.data(), values.data(), vectors.data(), &sweeps);
    if (status == 2u) { rts_set_error("rts_eig_eval: status 2: a non-finite entry in the covariance's lower triangle"); return RTS_ERR_INVALID; }
    if (status) { rts_set_error("rts_eig_eval: status 1: no convergence in %u sweeps", RTS_EIG_MAX_SWEEPS); return RTS_ERR_INVALID; }
    memcpy(values_out, values.data(), sizeof(double) * n);
    memcpy(vectors_out, vectors.data(), sizeof(double) * plan.vector_doubles);
    if (sweeps_out) *sweeps_out = sweeps;
    return RTS_OK;
}

extern "C" int rts_cube_eig(RtsHandle c, const RtsEigParams* p, void* device_values, void* device_vectors)
{
    const char* who = "rts_cube_eig";
    CHECK_HANDLE(c);
    NEED_CUBE(c, who, "no cube (call rts_cube_attach first)");
    if (!p) { rts_set_error("%s: null parameters", who); return RTS_ERR_INVALID; }
    if (p->reserved0 || p->reserved[0] || p->reserved[1]) { rts_set_error("%s: reserved fields must be 0", who); return RTS_ERR_INVALID; }
    const double* cov; uint32_t n = p->n;
    RTS_TRY(rts_pointer_or_owned(who, p->device_cov, c->cube.adapt.cov, c->cube.adapt.cov_n, "%s: device_cov is not 16-byte aligned",
                                 "%s: no covariance (rts_cube_covariance or rts_cube_st_covariance with device_out NULL first, or pass device_cov)", "%s: n = %u, the library-owned covariance's %u (or 0)", &cov, &n));
    const RtsEigPlan plan = rts_eig_plan(n);
    if (!plan.supported) { rts_set_error("%s: n = %u (1 .. %u)", who, n, RTS_BEAM_MAX_RX); return RTS_ERR_INVALID; }
    if (!device_values != !device_vectors) { rts_set_error("%s: device_values and device_vectors: both caller-owned or both NULL", who); return RTS_ERR_INVALID; }
    if ((uintptr_t)device_values & 7u) { rts_set_error("%s: device_values is not 8-byte aligned", who); return RTS_ERR_INVALID; }
    if ((uintptr_t)device_vectors & 15u) { rts_set_error("%s: device_vectors is not 16-byte aligned", who); return RTS_ERR_INVALID; }
    if (device_values) {
        const size_t nv = sizeof(double) * plan.value_doubles, nx = sizeof(double) * plan.vector_doubles;
        if (rts_bytes_overlap(device_values, nv, device_vectors, nx)) { rts_set_error("%s: device_values overlaps device_vectors", who); return RTS_ERR_INVALID; }
        if (rts_bytes_overlap(device_values, nv, cov, nx) || rts_bytes_overlap(device_vectors, nx, cov, nx)) { rts_set_error("%s: an output overlaps the covariance the call reads", who); return RTS_ERR_INVALID; }
    }
    CHECK_CLOSED(c);
    double* values; double* vectors;
    RTS_HIP(c->cube.doa.eig_val.place(device_values, plan.value_doubles, &values));
    RTS_HIP(c->cube.doa.eig_vec.place(device_vectors, plan.vector_doubles, &vectors));
    RTS_HIP(c->cube.doa.d_eig_status.reserve(2));
    if (!device_values) { c->cube.doa.eig_val.record(values, plan.value_doubles); c->cube.doa.eig_vec.record(vectors, plan.vector_doubles); c->cube.doa.eig_n = n; }
    return rts_cube_eig_device(c, plan, n, cov, c->cube.doa.d_eig_status.p + (device_values ? 1 : 0), values, vectors);
}

extern "C" int rts_cube_eig_get(RtsHandle c, double* values_out, double* vectors_out, uint64_t capacity_values, uint64_t capacity_vector_doubles)
{
    CHECK_HANDLE(c);
    const RtsCubeProduct& v = c->cube.doa.eig_val; const RtsCubeProduct& x = c->cube.doa.eig_vec;
    if (!c->cube.set || !v.valid || !x.valid || (!values_out && !vectors_out)) { rts_set_error("rts_cube_eig_get: no library-owned eigenpairs (rts_cube_eig with both outputs NULL; the eigenpairs end at rts_cube_attach) / null outputs"); return RTS_ERR_INVALID; }
    if ((values_out && capacity_values < v.doubles) || (vectors_out && capacity_vector_doubles < x.doubles)) { rts_set_error("rts_cube_eig_get: capacity too small"); return RTS_ERR_CAPACITY; }
    uint32_t status = 0;
    RTS_TRY(rts_status_word(c, c->cube.doa.d_eig_status.p, &status));
    if (status == 2u) { rts_set_error("rts_cube_eig_get: status 2: a non-finite entry in the covariance's lower triangle; every output is NaN"); return RTS_ERR_INVALID; }
    if (status) { rts_set_error("rts_cube_eig_get: status 1: no convergence in %u sweeps; every output is NaN", RTS_EIG_MAX_SWEEPS); return RTS_ERR_INVALID; }
    if (values_out) RTS_HIP(hipMemcpy(values_out, v.p, sizeof(double) * v.doubles, hipMemcpyDeviceToHost));
    if (vectors_out) RTS_HIP(hipMemcpy(vectors_out, x.p, sizeof(double) * x.doubles, hipMemcpyDeviceToHost));
    return RTS_OK;
}

// the record of a scan over vectors of n elements: what needs no device memory
static int rts_doa_scan_check(const char* who, uint32_t n, uint32_t first_vector, uint32_t m, uint32_t flags, uint64_t n_dirs, const double* g, RtsDoaScanPlan* plan)
{
    if (n == 0 || n > RTS_BEAM_MAX_RX) { rts_set_error("%s: n = %u (1 .. %u)", who, n, RTS_BEAM_MAX_RX); return RTS_ERR_INVALID; }
    if (flags & ~RTS_DOA_INVERSE) { rts_set_error("%s: unknown flags 0x%x", who, flags); return RTS_ERR_INVALID; }
    if (m == 0 || first_vector > n || m > n - first_vector) { rts_set_error("%s: first_vector = %u, m = %u: at least one vector, inside the table's %u rows", who, first_vector, m, n); return RTS_ERR_INVALID; }
    if (n_dirs == 0) { rts_set_error("%s: n_dirs = 0", who); return RTS_ERR_INVALID; }
    if (!g) { rts_set_error("%s: null g", who); return RTS_ERR_INVALID; }
    for (uint32_t k = 0; k < m; k++) if (!std::isfinite(g[k])) { rts_set_error("%s: g[%u] is not finite", who, k); return RTS_ERR_INVALID; }
    *plan = rts_doa_scan_plan(n, m, n_dirs);
    if (!plan->supported) { rts_set_error("%s: n_dirs = %llu directions, %u per workgroup: more than %u workgroups (the launch grid)", who, (unsigned long long)n_dirs, RTS_DOA_THREADS, RTS_DOA_MAX_GRID_X); return RTS_ERR_INVALID; }
    return RTS_OK;
}

extern "C" int rts_doa_scan_eval(const double* vectors, const double* g, uint32_t n, uint32_t m, const double* steering, uint64_t n_dirs, uint32_t flags, double* out)
{
    RtsDoaScanPlan plan;
    RTS_TRY(rts_doa_scan_check("rts_doa_scan_eval", n, 0u, m, flags, n_dirs, g, &plan));
    if (!vectors || !steering || !out) { rts_set_error("rts_doa_scan_eval: null vectors, steering or output array"); return RTS_ERR_INVALID; }
    rts_doa_scan_eval_host(vectors, g, n, m, steering, n_dirs, flags, out);
    return RTS_OK;
}

extern "C" int rts_cube_doa_scan(RtsHandle c, const RtsDoaScanParams* p, void* device_out)
{
    const char* who = "rts_cube_doa_scan";
    CHECK_HANDLE(c);
    NEED_CUBE(c, who, "no cube (call rts_cube_attach first)");
    if (!p) { rts_set_error("%s: null parameters", who); return RTS_ERR_INVALID; }
    if (p->reserved[0] || p->reserved[1]) { rts_set_error("%s: reserved fields must be 0", who); return RTS_ERR_INVALID; }
    const double* vec; uint32_t n = p->n;
    RTS_TRY(rts_pointer_or_owned(who, p->device_vectors, c->cube.doa.eig_vec, c->cube.doa.eig_n, "%s: device_vectors is not 16-byte aligned",
                                 "%s: no eigenvectors (rts_cube_eig with both outputs NULL first, or pass device_vectors)", "%s: n = %u, the library-owned eigenvectors' %u (or 0)", &vec, &n));
    RtsDoaScanPlan plan;
    RTS_TRY(rts_doa_scan_check(who, n, p->first_vector, p->m, p->flags, p->n_dirs, p->g, &plan));
    if (!p->device_steering) { rts_set_error("%s: null device_steering", who); return RTS_ERR_INVALID; }
    if ((uintptr_t)p->device_steering & 15u) { rts_set_error("%s: device_steering is not 16-byte aligned", who); return RTS_ERR_INVALID; }
    if ((uintptr_t)device_out & 7u) { rts_set_error("%s: device_out is not 8-byte aligned", who); return RTS_ERR_INVALID; }
    const double* rows = vec + 2 * (size_t)p->first_vector * n;
    if (device_out) {
        const size_t no = sizeof(double) * plan.out_doubles;
        if (rts_bytes_overlap(device_out, no, p->device_steering, 16u * (size_t)n * (size_t)p->n_dirs)) { rts_set_error("%s: device_out overlaps the steering table the call reads", who); return RTS_ERR_INVALID; }
        if (rts_bytes_overlap(device_out, no, rows, 16u * (size_t)p->m * n)) { rts_set_error("%s: device_out overlaps the vectors the call reads", who); return RTS_ERR_INVALID; }
    }
    CHECK_CLOSED(c);
    double* out; RTS_HIP(c->cube.doa.spectrum.place(device_out, plan.out_doubles, &out));
    // g -> pinned staging -> the device, on the stream (m <= RTS_BEAM_MAX_RX: one size for every call)
    RTS_HIP(c->cube.doa.g.upload(p->g, p->m, RTS_BEAM_MAX_RX, c->stream));
    if (!device_out) c->cube.doa.spectrum.record(out, plan.out_doubles);
    return rts_cube_doa_scan_device(c, plan, n, p->m, p->n_dirs, p->flags, (const double*)p->device_steering, rows, c->cube.doa.g.dev.p, out);
}

extern "C" int rts_cube_doa_get(RtsHandle c, double* host_out, uint64_t capacity_doubles)
{
    CHECK_HANDLE(c);
    return rts_cube_copy_out(c, "rts_cube_doa_get", "no library-owned spectrum (rts_cube_doa_scan with device_out NULL; the spectrum ends at rts_cube_attach) / null output", c->cube.doa.spectrum, host_out, capacity_doubles);
}

extern "C" int rts_doa_weights(uint32_t method, const double* values, uint32_t n, uint32_t n_sources, double loading, uint32_t* first, uint32_t* m, double* g, uint32_t* flags)
{
    if (!values || !first || !m || !g || !flags) { rts_set_error("rts_doa_weights: null eigenvalues or output"); return RTS_ERR_INVALID; }
    if (n == 0 || n > RTS_BEAM_MAX_RX) { rts_set_error("rts_doa_weights: n = %u (1 .. %u)", n, RTS_BEAM_MAX_RX); return RTS_ERR_INVALID; }
    uint32_t bad = 0, f = 0, mm = 0, fl = 0; double gg[RTS_BEAM_MAX_RX];
    switch (rts_doa_weights_host(method, values, n, n_sources, loading, &f, &mm, gg, &fl, &bad)) {
        case 0: break;
        case 1: rts_set_error("rts_doa_weights: unknown method %u (RTS_DOA_BARTLETT, _CAPON, _MUSIC)", method); return RTS_ERR_INVALID;
        case 2: rts_set_error("rts_doa_weights: loading = %g (finite, >= 0)", loading); return RTS_ERR_INVALID;
        case 3: rts_set_error("rts_doa_weights: values[%u] is not finite", bad); return RTS_ERR_INVALID;
        case 4: rts_set_error("rts_doa_weights: RTS_DOA_MUSIC: n_sources = %u leaves no noise subspace of n = %u", n_sources, n); return RTS_ERR_INVALID;
        default: rts_set_error("rts_doa_weights: RTS_DOA_CAPON: values[%u] + loading = %g is not > 0 (load more)", bad, values[bad] + loading); return RTS_ERR_INVALID;
    }
    *first = f; *m = mm; *flags = fl; memcpy(g, gg, sizeof(double) * mm);
    return RTS_OK;
}

extern "C" int rts_source_count(const double* values, uint32_t n, uint64_t K, uint32_t criterion, uint32_t* n_sources)
{
    if (!values || !n_sources) { rts_set_error("rts_source_count: null eigenvalues or output"); return RTS_ERR_INVALID; }
    if (n == 0 || n > RTS_BEAM_MAX_RX) { rts_set_error("rts_source_count: n = %u (1 .. %u)", n, RTS_BEAM_MAX_RX); return RTS_ERR_INVALID; }
    if (K == 0) { rts_set_error("rts_source_count: K = 0 snapshots"); return RTS_ERR_INVALID; }
    if (criterion != RTS_DOA_AIC && criterion != RTS_DOA_MDL) { rts_set_error("rts_source_count: unknown criterion %u (RTS_DOA_AIC, RTS_DOA_MDL)", criterion); return RTS_ERR_INVALID; }
    for (uint32_t k = 0; k < n; k++) {
        if (!std::isfinite(values[k]) || !(values[k] > 0.0)) { rts_set_error("rts_source_count: values[%u] = %g (finite, > 0: every eigenvalue enters a logarithm)", k, values[k]); return RTS_ERR_INVALID; }
        if (k && values[k] > values[k - 1u]) { rts_set_error("rts_source_count: values[%u] > values[%u]: not in descending order", k, k - 1u); return RTS_ERR_INVALID; }
    }
    *n_sources = rts_source_count_host(values, n, K, criterion);
    return RTS_OK;
}
