// rts_cube_api.hip -- the cube part of the C-ABI of include/rts_amd.h (rts_cube_reduce apart: rts_api.hip) and the pure-host evaluators that go with it.
// Host code only, no kernels: argument checks, the handle's cube state (RtsCubeState, rts_internal.h), the calls of the launchers in the kernels' units.
#include <cmath>
#include <cstring>
#include <algorithm>
#include "rts_cube_api.h"

// what a render reads and how (rts_cube_render's arguments, RtsBeatParams' fields); RTS_RENDER_PATHS reads the aggregation's results
static int rts_render_source_check(const char* who, uint32_t source, uint32_t flags)
{
    if (source != RTS_RENDER_RAYS && source != RTS_RENDER_PATHS) { rts_set_error("%s: unknown source %u (RTS_RENDER_RAYS, RTS_RENDER_PATHS)", who, source); return RTS_ERR_INVALID; }
    if (flags & ~RTS_RENDER_DOPPLER) { rts_set_error("%s: unknown flags 0x%x", who, flags); return RTS_ERR_INVALID; }
    return RTS_OK;
}
static int rts_render_paths_check(const RtsContext* c, const char* who)
{
    if (!c->res.agg_valid) { rts_set_error("%s: RTS_RENDER_PATHS needs rts_aggregate of this pulse first (the groups' power, delay and phase are its results)", who); return RTS_ERR_INVALID; }
    return RTS_OK;
}

// ------------------------------------------------------------------------------------- complex return cube
extern "C" int rts_cube_attach(RtsHandle c, const RtsCubeParams* p, void* device_ptr)
{
    CHECK_HANDLE(c);
    if (!p || p->n_rx == 0 || p->n_pulses == 0 || p->n_bins == 0 || !(p->dt > 0) || !std::isfinite(p->t0)) { rts_set_error("rts_cube_attach: bad parameters"); return RTS_ERR_INVALID; }
    const size_t doubles = 2 * (size_t)p->n_rx * p->n_pulses * p->n_bins;
    RTS_HIP(hipStreamSynchronize(c->stream));
    c->cube.params = *p;
    if (device_ptr) c->cube.p = (double*)device_ptr;        // caller-owned (and caller-zeroed) device memory
    else { RTS_HIP(c->cube.own.reserve(doubles)); c->cube.p = c->cube.own.p; RTS_HIP(hipMemset(c->cube.p, 0, sizeof(double) * doubles)); }
    c->cube.set = true;
    c->cube.end_products();
    return RTS_OK;
}

extern "C" int rts_cube_accumulate(RtsHandle c, uint32_t pulse_index, double cspeed, double carrier)
{
    CHECK_HANDLE(c);
    CHECK_CLOSED(c);
    NEED_CUBE(c, "rts_cube_accumulate", "call rts_cube_attach first");
    RTS_TRY(rts_pulse_index_check("rts_cube_accumulate", pulse_index, c->cube.params.n_pulses));
    return rts_cube_accumulate_device(c, pulse_index, cspeed, carrier);
}

extern "C" int rts_cube_accumulate_paths(RtsHandle c, uint32_t pulse_index)
{
    CHECK_HANDLE(c);
    CHECK_CLOSED(c);
    NEED_CUBE(c, "rts_cube_accumulate_paths", "call rts_cube_attach first");
    if (!c->res.agg_valid) { rts_set_error("rts_cube_accumulate_paths: call rts_aggregate for this pulse first (the groups' power, delay and phase are its results)"); return RTS_ERR_INVALID; }
    RTS_TRY(rts_pulse_index_check("rts_cube_accumulate_paths", pulse_index, c->cube.params.n_pulses));
    return rts_cube_accumulate_paths_device(c, pulse_index, c->res.agg_base_local);
}

extern "C" int rts_cube_doppler(RtsHandle c, uint32_t n_fft, void* device_out)
{
    CHECK_HANDLE(c);
    CHECK_CLOSED(c);
    NEED_CUBE(c, "rts_cube_doppler", "call rts_cube_attach first");
    if (!rts_pow2_in(n_fft, 2u, 4096u) || n_fft < c->cube.params.n_pulses) {
        rts_set_error("rts_cube_doppler: n_fft = %u must be a power of two in [max(2, n_pulses = %u), 4096]", n_fft, c->cube.params.n_pulses); return RTS_ERR_INVALID; }
    const size_t doubles = 2 * (size_t)c->cube.params.n_rx * n_fft * c->cube.params.n_bins;
    double* out; RTS_HIP(c->cube.doppler.place(device_out, doubles, &out));
    c->cube.doppler.record(out, doubles); c->cube.doppler_n = n_fft;       // (also when caller-owned: rts_cube_detect without a map takes it)
    return rts_cube_doppler_device(c, n_fft, out);
}

extern "C" int rts_cube_doppler_get(RtsHandle c, double* host_out, uint64_t capacity_doubles)
{
    CHECK_HANDLE(c);
    CHECK_CLOSED(c);
    return rts_cube_copy_out(c, "rts_cube_doppler_get", "no transform (rts_cube_doppler) / null output", c->cube.doppler, host_out, capacity_doubles);
}

extern "C" int rts_cube_get(RtsHandle c, double* host_out, uint64_t capacity_doubles)
{
    CHECK_HANDLE(c);
    CHECK_CLOSED(c);
    return rts_cube_copy_out(c, "rts_cube_get", "no cube / null output", true, c->cube.p, 2 * (size_t)c->cube.params.n_rx * c->cube.params.n_pulses * c->cube.params.n_bins, host_out, capacity_doubles);
}

// ------------------------------------------------------------------------------------- received signal: waveform render, range compression
// (rts_amd.h: RtsWaveform; the interpolator is rts_waveform.h, shared by the host export and the render kernel, rts_render.hip)
static int rts_waveform_check(const RtsWaveform* w, const char* who)
{
    if (!w) { rts_set_error("%s: null waveform", who); return RTS_ERR_INVALID; }
    if (w->reserved[0] || w->reserved[1]) { rts_set_error("%s: reserved fields must be 0", who); return RTS_ERR_INVALID; }
    if (w->n_samples == 0 || w->n_samples > RTS_WAVEFORM_MAX_SAMPLES) { rts_set_error("%s: %u samples (1 .. %u)", who, w->n_samples, RTS_WAVEFORM_MAX_SAMPLES); return RTS_ERR_INVALID; }
    RTS_TRY(rts_taps_check(who, w->taps));
    if (!w->samples) { rts_set_error("%s: null sample array", who); return RTS_ERR_INVALID; }
    for (uint32_t i = 0; i < 2 * w->n_samples; i++) if (!std::isfinite(w->samples[i])) { rts_set_error("%s: sample %u is not finite", who, i / 2); return RTS_ERR_INVALID; }
    return RTS_OK;
}

extern "C" int rts_waveform_eval(const RtsWaveform* w, const double* x, uint32_t n, double* out)
{
    RTS_TRY(rts_waveform_check(w, "rts_waveform_eval"));
    if (n && (!x || !out)) { rts_set_error("rts_waveform_eval: null point or output array"); return RTS_ERR_INVALID; }
    for (uint32_t i = 0; i < n; i++) rts_wave_eval(w->samples, w->n_samples, w->taps, x[i], &out[2 * (size_t)i], &out[2 * (size_t)i + 1]);
    return RTS_OK;
}

extern "C" int rts_cube_set_waveform(RtsHandle c, const RtsWaveform* w)
{
    CHECK_HANDLE(c);
    RTS_TRY(rts_waveform_check(w, "rts_cube_set_waveform"));
    // the handle's enqueued work may still read the previous waveform: a speculative chain is resolved, then the stream drained
    if (c->pulse.chained()) CHECK_CLOSED(c);      // (an OPEN pulse stays in flight: its render comes after the stream is drained below)
    RTS_HIP(hipStreamSynchronize(c->stream));
    RTS_HIP(c->cube.d_wave.reserve(2 * (size_t)w->n_samples));
    RTS_HIP(hipMemcpy(c->cube.d_wave.p, w->samples, sizeof(double) * 2 * w->n_samples, hipMemcpyHostToDevice));
    c->cube.wave_M = w->n_samples; c->cube.wave_L = w->taps; c->cube.wave_set = true;
    return RTS_OK;
}

extern "C" int rts_cube_render(RtsHandle c, uint32_t pulse_index, uint32_t source, uint32_t flags, double cspeed, double carrier)
{
    CHECK_HANDLE(c);
    RTS_TRY(rts_render_source_check("rts_cube_render", source, flags));
    CHECK_CLOSED(c);
    NEED_CUBE(c, "rts_cube_render", "call rts_cube_attach first");
    if (!c->cube.wave_set) { rts_set_error("rts_cube_render: no waveform (rts_cube_set_waveform)"); return RTS_ERR_INVALID; }
    RTS_TRY(rts_pulse_index_check("rts_cube_render", pulse_index, c->cube.params.n_pulses));
    const bool paths = source == RTS_RENDER_PATHS;
    if (paths) RTS_TRY(rts_render_paths_check(c, "rts_cube_render"));
    return rts_cube_render_device(c, pulse_index, paths, (flags & RTS_RENDER_DOPPLER) != 0, cspeed, carrier, c->res.agg_base_local);
}

extern "C" int rts_cube_compress(RtsHandle c, uint32_t first_pulse, uint32_t n_pulses)
{
    CHECK_HANDLE(c);
    CHECK_CLOSED(c);
    NEED_CUBE(c, "rts_cube_compress", "call rts_cube_attach first");
    if (!c->cube.wave_set) { rts_set_error("rts_cube_compress: no waveform (rts_cube_set_waveform)"); return RTS_ERR_INVALID; }
    const RtsCubeParams& q = c->cube.params;
    RTS_TRY(rts_pulses_check("rts_cube_compress", first_pulse, n_pulses, q.n_pulses, false));
    if (q.n_bins > RTS_COMPRESS_MAX_BINS) { rts_set_error("rts_cube_compress: %u range bins > %u (RTS_COMPRESS_MAX_BINS: one row of complex128 in a workgroup's LDS)", q.n_bins, RTS_COMPRESS_MAX_BINS); return RTS_ERR_INVALID; }
    return rts_cube_compress_device(c, first_pulse, n_pulses);
}

// ------------------------------------------------------------------------------------- receiver noise, CFAR detection
// (rts_amd.h; the generator is rts_noise.h, shared by the host export and the noise kernel; the kernels are in rts_detect.hip)
extern "C" int rts_noise_eval(uint64_t seed, const uint64_t* index, uint32_t n, double noise_power, double* out)
{
    if (!std::isfinite(noise_power) || noise_power < 0) { rts_set_error("rts_noise_eval: noise_power = %g (finite, >= 0)", noise_power); return RTS_ERR_INVALID; }
    if (n && (!index || !out)) { rts_set_error("rts_noise_eval: null index or output array"); return RTS_ERR_INVALID; }
    const double sigma = sqrt(noise_power / 2.0);
    for (uint32_t j = 0; j < n; j++) rts_noise_sample(seed, index[j], sigma, &out[2 * (size_t)j], &out[2 * (size_t)j + 1]);
    return RTS_OK;
}

extern "C" int rts_cube_add_noise(RtsHandle c, uint32_t first_pulse, uint32_t n_pulses, double noise_power, uint64_t seed)
{
    CHECK_HANDLE(c);
    if (!std::isfinite(noise_power) || noise_power < 0) { rts_set_error("rts_cube_add_noise: noise_power = %g (finite, >= 0)", noise_power); return RTS_ERR_INVALID; }
    CHECK_CLOSED(c);
    NEED_CUBE(c, "rts_cube_add_noise", "call rts_cube_attach first");
    const RtsCubeParams& q = c->cube.params;
    RTS_TRY(rts_pulses_check("rts_cube_add_noise", first_pulse, n_pulses, q.n_pulses, false));
    if ((uintptr_t)c->cube.p & 15u) { rts_set_error("rts_cube_add_noise: the cube's device memory is not 16-byte aligned"); return RTS_ERR_INVALID; }
    return rts_cube_noise_device(c, first_pulse, n_pulses, sqrt(noise_power / 2.0), seed);
}

// ------------------------------------------------------------------------------------- clutter and jammer sources
// (rts_amd.h: RtsSourceParams; the rules, the validation, the evaluator and the launch plan are rts_source.h, shared with the kernel, rts_source.hip)
static int rts_sources_check(const char* who, const RtsSourceParams* p, uint32_t n_rx, uint32_t n_bins)
{
    if (!p) { rts_set_error("%s: null parameters", who); return RTS_ERR_INVALID; }
    uint32_t bad = 0;
    switch (rts_src_check(p, n_rx, n_bins, &bad)) {
        case 0: return RTS_OK;
        case 1: rts_set_error("%s: n_patches = %u (1 .. %u, RTS_SRC_MAX_PATCHES)", who, p->n_patches, RTS_SRC_MAX_PATCHES); break;
        case 2: rts_set_error("%s: unknown flags 0x%x", who, p->flags); break;
        case 3: rts_set_error("%s: reserved fields must be 0", who); break;
        case 4: rts_set_error("%s: null spatial", who); break;
        case 5: rts_set_error("%s: null power", who); break;
        case 6: rts_set_error("%s: null doppler", who); break;
        case 7: rts_set_error("%s: n_rx = %u receivers: more than %u (RTS_BEAM_MAX_RX)", who, n_rx, RTS_BEAM_MAX_RX); break;
        case 8: rts_set_error("%s: n_patches * n_rx = %u * %u: more than %u (RTS_SRC_MAX_TABLE: the spatial table sits in a workgroup's LDS)", who, p->n_patches, n_rx, RTS_SRC_MAX_TABLE); break;
        case 10: rts_set_error("%s: spatial[%u][%u] is not finite", who, bad / n_rx, bad % n_rx); break;
        case 11: rts_set_error("%s: power[%u] = %g (finite, >= 0)", who, bad, p->power[bad]); break;
        case 12: rts_set_error("%s: doppler[%u] is not finite", who, bad); break;
        case 13: rts_set_error("%s: rho[%u] = %g outside [0, 1]", who, bad, p->rho[bad]); break;
        default: rts_set_error("%s: range_profile[%u] = %g (finite, >= 0)", who, bad, p->range_profile[bad]); break;
    }
    return RTS_ERR_INVALID;
}

extern "C" int rts_sources_eval(const RtsCubeParams* q, const RtsSourceParams* p, double* cube_inout)
{
    const char* who = "rts_sources_eval";
    RTS_TRY(rts_eval_cube_check(who, q, true, false));
    RTS_TRY(rts_sources_check(who, p, q->n_rx, q->n_bins));
    if (!cube_inout) { rts_set_error("%s: null array", who); return RTS_ERR_INVALID; }
    std::vector<double> work(rts_src_work_doubles(p->n_patches));
    rts_sources_eval_host(q, p, cube_inout, work.data());
    return RTS_OK;
}

extern "C" int rts_cube_add_sources(RtsHandle c, const RtsSourceParams* p)
{
    const char* who = "rts_cube_add_sources";
    CHECK_HANDLE(c);
    NEED_CUBE(c, who, "no cube (call rts_cube_attach first)");
    const RtsCubeParams& q = c->cube.params;
    RTS_TRY(rts_sources_check(who, p, q.n_rx, q.n_bins));
    if ((uintptr_t)c->cube.p & 15u) { rts_set_error("%s: the cube's device memory is not 16-byte aligned", who); return RTS_ERR_INVALID; }
    const RtsSrcPlan plan = rts_src_plan(q.n_rx, q.n_bins, p->n_patches, p->range_profile != nullptr);
    if (!plan.supported) { rts_set_error("%s: a cube of %u receivers x %u bins with %u patches has no launch plan", who, q.n_rx, q.n_bins, p->n_patches); return RTS_ERR_INVALID; }
    CHECK_CLOSED(c);
    const uint64_t live = rts_src_live_mask(p->n_patches, p->power);
    if (!live) return RTS_OK;                                   // every patch has power 0: nothing is written
    // the table -> pinned staging -> the device, on the stream; the staging grows to the largest table this cube's bins allow
    const size_t most = 2u * ((size_t)RTS_SRC_MAX_TABLE + 2u * RTS_SRC_MAX_PATCHES) + q.n_bins;
    double* tab = nullptr;
    RTS_HIP(c->cube.src_tab.begin(plan.table_doubles, most, most, &tab));
    rts_src_table(p, q.n_rx, q.n_bins, tab);
    RTS_HIP(c->cube.src_tab.send(plan.table_doubles, c->stream));
    return rts_cube_sources_device(c, plan, p->n_patches, p->range_profile != nullptr, p->seed, live, c->cube.src_tab.dev.p);
}

// The checks rts_cube_detect, rts_cube_detect_os and rts_cfar_os_eval share, in the order each of them applies them.
// flags, reserved fields and the window of either parameter record on a map of n_doppler x nb cells
template <class Params> static int rts_cfar_window_check(const char* who, const Params* p, uint32_t nb, uint32_t n_doppler)
{
    const uint32_t Gr = p->guard_range, Gd = p->guard_doppler, Tr = p->train_range, Td = p->train_doppler;
    if (p->flags & ~RTS_CFAR_LOCAL_MAX) { rts_set_error("%s: unknown flags 0x%x", who, p->flags); return RTS_ERR_INVALID; }
    if (p->reserved0 || p->reserved[0] || p->reserved[1]) { rts_set_error("%s: reserved fields must be 0", who); return RTS_ERR_INVALID; }
    if (Tr > RTS_CFAR_MAX_HALF || Td > RTS_CFAR_MAX_HALF || Gr > RTS_CFAR_MAX_HALF || Gd > RTS_CFAR_MAX_HALF) { rts_set_error("%s: guard_range, guard_doppler, train_range, train_doppler are at most %u each", who, RTS_CFAR_MAX_HALF); return RTS_ERR_INVALID; }
    if (Tr + Td == 0) { rts_set_error("%s: train_range + train_doppler = 0 (no training cells)", who); return RTS_ERR_INVALID; }
    if (Gr + Tr > RTS_CFAR_MAX_HALF) { rts_set_error("%s: guard_range + train_range = %u > %u", who, Gr + Tr, RTS_CFAR_MAX_HALF); return RTS_ERR_INVALID; }
    if (Gd + Td > RTS_CFAR_MAX_HALF) { rts_set_error("%s: guard_doppler + train_doppler = %u > %u", who, Gd + Td, RTS_CFAR_MAX_HALF); return RTS_ERR_INVALID; }
    if (2 * (Gd + Td) + 1 > n_doppler) { rts_set_error("%s: guard_doppler + train_doppler = %u: the window (%u rows) exceeds n_doppler = %u", who, Gd + Td, 2 * (Gd + Td) + 1, n_doppler); return RTS_ERR_INVALID; }
    if (Gr + Tr >= nb) { rts_set_error("%s: guard_range + train_range = %u >= n_bins = %u", who, Gr + Tr, nb); return RTS_ERR_INVALID; }
    return RTS_OK;
}

// exactly one of pfa and alpha, each in its range; pri.  Two checks, because rts_cube_detect has always reported its GO / SO rules
// between them, and a record with several wrong fields keeps reporting the one it reported
static int rts_cfar_level_check(const char* who, double pfa, double alpha)
{
    const bool has_pfa = pfa != 0.0, has_alpha = alpha != 0.0;
    if (has_pfa && !(pfa > 0.0 && pfa < 1.0)) { rts_set_error("%s: pfa = %g outside (0, 1)", who, pfa); return RTS_ERR_INVALID; }
    if (has_pfa == has_alpha) { rts_set_error("%s: give exactly one of pfa and alpha", who); return RTS_ERR_INVALID; }
    if (has_alpha && !(alpha > 0.0 && std::isfinite(alpha))) { rts_set_error("%s: alpha = %g (finite, > 0)", who, alpha); return RTS_ERR_INVALID; }
    return RTS_OK;
}
static int rts_cfar_pri_check(const char* who, double pri)
{
    if (!(pri >= 0.0) || !std::isfinite(pri)) { rts_set_error("%s: pri = %g (finite, >= 0)", who, pri); return RTS_ERR_INVALID; }
    return RTS_OK;
}

extern "C" int rts_cube_detect(RtsHandle c, const RtsCfarParams* p, const void* device_map, uint32_t n_doppler)
{
    CHECK_HANDLE(c);
    if (!p) { rts_set_error("rts_cube_detect: null parameters"); return RTS_ERR_INVALID; }
    CHECK_CLOSED(c);
    NEED_CUBE(c, "rts_cube_detect", "no cube (call rts_cube_attach first)");
    const double* map;
    RTS_TRY(rts_cfar_map(c, "rts_cube_detect", device_map, &map, &n_doppler));
    if (p->mode > RTS_CFAR_SO) { rts_set_error("rts_cube_detect: unknown mode %u (RTS_CFAR_CA, _GO, _SO)", p->mode); return RTS_ERR_INVALID; }
    RTS_TRY(rts_cfar_window_check("rts_cube_detect", p, c->cube.params.n_bins, n_doppler));
    RTS_TRY(rts_cfar_level_check("rts_cube_detect", p->pfa, p->alpha));
    if (p->mode != RTS_CFAR_CA && p->pfa != 0.0) { rts_set_error("rts_cube_detect: pfa is for mode RTS_CFAR_CA only (GO / SO take alpha)"); return RTS_ERR_INVALID; }
    if (p->mode != RTS_CFAR_CA && p->train_range == 0) { rts_set_error("rts_cube_detect: train_range = 0 with GO / SO (the halves are range halves)"); return RTS_ERR_INVALID; }
    RTS_TRY(rts_cfar_pri_check("rts_cube_detect", p->pri));
    c->cube.det_valid = false; c->cube.plot_valid = false;      // (plots index the list they were made from)
    return rts_cube_detect_device(c, *p, map, n_doppler, p->max_detections ? p->max_detections : RTS_CFAR_DEFAULT_MAX_DETECTIONS);
}

extern "C" int rts_cube_detections_get(RtsHandle c, RtsDetection* out, uint32_t capacity, uint32_t* n_out)
{
    CHECK_HANDLE(c);
    if (!n_out || (capacity && !out)) { rts_set_error("rts_cube_detections_get: null output"); return RTS_ERR_INVALID; }
    if (!c->cube.det_valid) { rts_set_error("rts_cube_detections_get: no detection list (rts_cube_detect, rts_cube_detect_os; a list ends at rts_cube_attach)"); return RTS_ERR_INVALID; }
    uint32_t n = 0;
    RTS_TRY(rts_list_copy_out(c, c->cube.d_det_off.p + c->cube.det_nseg, c->cube.det_max, c->cube.d_det.p, sizeof(RtsDetection), out, capacity, n_out, &n));
    return rts_list_fits_check("rts_cube_detections_get", "%s: %u of %u detections copied (max_detections %u, capacity %u)", n, *n_out, c->cube.det_max, capacity);
}

// ------------------------------------------------------------------------------------- ordered-statistic CFAR
// (rts_amd.h: RtsCfarOsParams; the arithmetic is rts_cfar_os.h, shared by the host exports and the kernel, rts_detect.hip; the checks of the
// fields it shares with RtsCfarParams are rts_cube_detect's, above)
static int rts_cfar_os_check(const RtsCfarOsParams* p, uint32_t nb, uint32_t n_doppler, const char* who)
{
    RTS_TRY(rts_cfar_window_check(who, p, nb, n_doppler));
    const uint32_t N0 = rts_cfar_n0(p->guard_range, p->guard_doppler, p->train_range, p->train_doppler);
    if (p->rank == 0 || p->rank > N0) { rts_set_error("%s: rank = %u outside [1, N0 = %u] (the training cells of a full window)", who, p->rank, N0); return RTS_ERR_INVALID; }
    RTS_TRY(rts_cfar_level_check(who, p->pfa, p->alpha));
    return rts_cfar_pri_check(who, p->pri);
}

extern "C" int rts_cfar_os_alpha(uint32_t n_train, uint32_t rank, double pfa, double* alpha)
{
    if (n_train == 0) { rts_set_error("rts_cfar_os_alpha: n_train = 0"); return RTS_ERR_INVALID; }
    if (rank == 0 || rank > n_train) { rts_set_error("rts_cfar_os_alpha: rank = %u outside [1, n_train = %u]", rank, n_train); return RTS_ERR_INVALID; }
    if (!(pfa > 0.0 && pfa < 1.0)) { rts_set_error("rts_cfar_os_alpha: pfa = %g outside (0, 1)", pfa); return RTS_ERR_INVALID; }
    if (!alpha) { rts_set_error("rts_cfar_os_alpha: null output"); return RTS_ERR_INVALID; }
    *alpha = rts_cfar_os_alpha_solve(n_train, rank, pfa);
    return RTS_OK;
}

extern "C" int rts_cfar_os_eval(const RtsCubeParams* q, const double* map, uint32_t n_doppler, const RtsCfarOsParams* p, RtsDetection* out, uint32_t capacity, uint32_t* n_out)
{
    RTS_TRY(rts_eval_cube_check("rts_cfar_os_eval", q, false, true));
    if (!p) { rts_set_error("rts_cfar_os_eval: null parameters"); return RTS_ERR_INVALID; }
    if (n_doppler == 0) { rts_set_error("rts_cfar_os_eval: n_doppler = 0"); return RTS_ERR_INVALID; }
    RTS_TRY(rts_cfar_os_check(p, q->n_bins, n_doppler, "rts_cfar_os_eval"));
    if (!map || !n_out || (capacity && !out)) { rts_set_error("rts_cfar_os_eval: null map or output"); return RTS_ERR_INVALID; }
    const uint32_t N0 = rts_cfar_n0(p->guard_range, p->guard_doppler, p->train_range, p->train_doppler);
    std::vector<double> tab; std::vector<uint64_t> keys(N0);
    if (p->pfa != 0.0) { tab.assign((size_t)N0 + 1, 0.0); rts_cfar_os_alpha_table(p->guard_range, p->guard_doppler, p->train_range, p->train_doppler, p->rank, p->pfa, q->n_bins, tab.data()); }
    const uint32_t total = rts_cfar_os_eval_host(q, map, n_doppler, p, tab.empty() ? nullptr : tab.data(), keys.data(), out, capacity);
    *n_out = total;
    return rts_list_fits_check("rts_cfar_os_eval", "%s: %u of %u detections written (capacity %u)", rts_list_copied(total, total, capacity), total, capacity);
}

extern "C" int rts_cube_detect_os(RtsHandle c, const RtsCfarOsParams* p, const void* device_map, uint32_t n_doppler)
{
    CHECK_HANDLE(c);
    if (!p) { rts_set_error("rts_cube_detect_os: null parameters"); return RTS_ERR_INVALID; }
    CHECK_CLOSED(c);
    NEED_CUBE(c, "rts_cube_detect_os", "no cube (call rts_cube_attach first)");
    const double* map;
    RTS_TRY(rts_cfar_map(c, "rts_cube_detect_os", device_map, &map, &n_doppler));
    const uint32_t nb = c->cube.params.n_bins;
    RTS_TRY(rts_cfar_os_check(p, nb, n_doppler, "rts_cube_detect_os"));
    c->cube.det_valid = false; c->cube.plot_valid = false;      // (plots index the list they were made from)
    // the alphas by training count -> pinned staging -> the device, on the stream (N0 + 1 <= RTS_CFAR_OS_MAX_TRAIN + 1: one size for every call);
    // a call that needs nothing the device table of the previous one lacks sends nothing
    const double* tab_dev = nullptr;
    if (p->pfa != 0.0) {
        RtsCubeState& s = c->cube;
        const uint32_t N0 = rts_cfar_n0(p->guard_range, p->guard_doppler, p->train_range, p->train_doppler);
        const uint32_t key[5] = {p->guard_range, p->guard_doppler, p->train_range, p->train_doppler, p->rank};
        if (s.os_tab.size() != (size_t)N0 + 1 || memcmp(key, s.os_tab_key, sizeof(key)) != 0 || s.os_tab_pfa != p->pfa) {
            s.os_tab.assign((size_t)N0 + 1, 0.0); memcpy(s.os_tab_key, key, sizeof(key)); s.os_tab_pfa = p->pfa; s.os_tab_sent = false;
        }
        if (rts_cfar_os_alpha_table(p->guard_range, p->guard_doppler, p->train_range, p->train_doppler, p->rank, p->pfa, nb, s.os_tab.data()) != 0) s.os_tab_sent = false;
        if (!s.os_tab_sent) {
            double* h = nullptr;
            RTS_HIP(s.os_alpha.begin(RTS_CFAR_OS_MAX_TRAIN + 1u, RTS_CFAR_OS_MAX_TRAIN + 1u, RTS_CFAR_OS_MAX_TRAIN + 1u, &h));
            memcpy(h, s.os_tab.data(), sizeof(double) * ((size_t)N0 + 1));
            RTS_HIP(s.os_alpha.send((size_t)N0 + 1, c->stream));
            s.os_tab_sent = true;
        }
        tab_dev = s.os_alpha.dev.p;
    }
    return rts_cube_detect_os_device(c, *p, tab_dev, map, n_doppler, p->max_detections ? p->max_detections : RTS_CFAR_DEFAULT_MAX_DETECTIONS);
}

// ------------------------------------------------------------------------------------- plot extraction
// (rts_amd.h: RtsPlotParams, RtsPlot; the rules and the host evaluator are rts_plot.h, shared with the kernels, rts_plot.hip)
#define RTS_PLOT_MAX_LIST 0x40000000u      // the kernels index the list, the sort and the scan (one element more) with 32 bits
static int rts_plot_check(const char* who, const RtsPlotParams* p)
{
    if (!p) { rts_set_error("%s: null parameters", who); return RTS_ERR_INVALID; }
    switch (rts_plot_params_check(p)) {
        case 0: return RTS_OK;
        case 1: rts_set_error("%s: link_range = %u > %u (RTS_PLOT_MAX_LINK)", who, p->link_range, RTS_PLOT_MAX_LINK); break;
        case 2: rts_set_error("%s: link_doppler = %u > %u (RTS_PLOT_MAX_LINK)", who, p->link_doppler, RTS_PLOT_MAX_LINK); break;
        case 3: rts_set_error("%s: reserved fields must be 0", who); break;
        case 4: rts_set_error("%s: pri = %g (finite, >= 0)", who, p->pri); break;
        case 5: rts_set_error("%s: n_doppler = 0 with a device_list", who); break;
        case 6: rts_set_error("%s: device_list is not 8-byte aligned", who); break;
        default: rts_set_error("%s: n_list = %u, n_doppler = %u without a device_list (both 0: the handle's list brings its own)", who, p->n_list, p->n_doppler); break;
    }
    return RTS_ERR_INVALID;
}

extern "C" int rts_plots_eval(const RtsCubeParams* q, const RtsDetection* list, uint32_t n_list, uint32_t n_doppler, const RtsPlotParams* p, RtsPlot* out, uint32_t capacity, uint32_t* n_out)
{
    const char* who = "rts_plots_eval";
    RTS_TRY(rts_eval_cube_check(who, q, false, true));
    RTS_TRY(rts_plot_check(who, p));
    if (n_doppler == 0) { rts_set_error("%s: n_doppler = 0", who); return RTS_ERR_INVALID; }
    if ((n_list && !list) || !n_out || (capacity && !out)) { rts_set_error("%s: null list or output", who); return RTS_ERR_INVALID; }
    if (n_list > RTS_PLOT_MAX_LIST) { rts_set_error("%s: n_list = %u > %u", who, n_list, RTS_PLOT_MAX_LIST); return RTS_ERR_INVALID; }
    uint32_t bad = 0;
    switch (rts_plot_list_check(list, n_list, q->n_rx, n_doppler, q->n_bins, &bad)) {
        case 0: break;
        case 1: rts_set_error("%s: list[%u]: (rx, doppler_bin, range_bin) = (%u, %u, %u) outside the map of %u x %u x %u cells", who, bad, list[bad].rx, list[bad].doppler_bin, list[bad].range_bin,
                              q->n_rx, n_doppler, q->n_bins); return RTS_ERR_INVALID;
        default: rts_set_error("%s: list[%u] is not above list[%u] in flat (rx, doppler_bin, range_bin) order", who, bad, bad - 1u); return RTS_ERR_INVALID;
    }
    const uint32_t total = rts_plots_eval_host(q, list, n_list, n_doppler, p, out, capacity);
    *n_out = total;
    return rts_list_fits_check(who, "%s: %u of %u plots written (capacity %u)", rts_list_copied(total, total, capacity), total, capacity);
}

extern "C" int rts_cube_plots(RtsHandle c, const RtsPlotParams* p)
{
    const char* who = "rts_cube_plots";
    CHECK_HANDLE(c);
    if (!p) { rts_set_error("%s: null parameters", who); return RTS_ERR_INVALID; }
    CHECK_CLOSED(c);
    NEED_CUBE(c, who, "no cube (call rts_cube_attach first)");
    RTS_TRY(rts_plot_check(who, p));
    RtsCubeState& s = c->cube;
    const RtsDetection* list = (const RtsDetection*)p->device_list;
    const uint32_t* n_dev = nullptr;
    uint32_t n_cap = p->n_list, nd = p->n_doppler;
    if (!list) {
        if (!s.det_valid) { rts_set_error("%s: no detection list (rts_cube_detect, rts_cube_detect_os; a list ends at rts_cube_attach) and no device_list", who); return RTS_ERR_INVALID; }
        list = s.d_det.p; n_dev = s.d_det_off.p + s.det_nseg; n_cap = s.det_max; nd = s.det_nd;
    }
    if (n_cap > RTS_PLOT_MAX_LIST) { rts_set_error("%s: a list of %u records > %u", who, n_cap, RTS_PLOT_MAX_LIST); return RTS_ERR_INVALID; }
    s.plot_valid = false; s.plot_own_list = p->device_list == nullptr;
    return rts_cube_plots_device(c, *p, list, n_dev, n_cap, nd, p->max_plots ? p->max_plots : n_cap);
}

extern "C" int rts_cube_plots_get(RtsHandle c, RtsPlot* out, uint32_t capacity, uint32_t* n_out)
{
    const char* who = "rts_cube_plots_get";
    CHECK_HANDLE(c);
    if (!n_out || (capacity && !out)) { rts_set_error("%s: null output", who); return RTS_ERR_INVALID; }
    RtsCubeState& s = c->cube;
    if (!s.plot_valid) { rts_set_error("%s: no plots (rts_cube_plots; plots end at rts_cube_detect, rts_cube_detect_os and rts_cube_attach)", who); return RTS_ERR_INVALID; }
    uint32_t total = 0, det_total = 0, n = 0;
    RTS_TRY(rts_list_copy_out(c, s.d_plot_off.p + s.plot_cap, s.plot_max, s.d_plot.p, sizeof(RtsPlot), out, capacity, &total, &n));
    if (s.plot_own_list) RTS_HIP(hipMemcpy(&det_total, s.d_det_off.p + s.det_nseg, sizeof(uint32_t), hipMemcpyDeviceToHost));
    *n_out = total;
    RTS_TRY(rts_list_fits_check(who, "%s: %u of %u plots copied (max_plots %u, capacity %u)", n, total, s.plot_max, capacity));
    if (s.plot_own_list && det_total > s.det_max) {
        rts_set_error("%s: the detection list was truncated (%u of %u detections stored): the %u plots describe the stored prefix", who, s.det_max, det_total, total); return RTS_ERR_CAPACITY; }
    return RTS_OK;
}

// ------------------------------------------------------------------------------------- tracking
// (rts_amd.h: RtsTrackParams, RtsTrack; the rules and the host evaluator are rts_track.h, shared with the kernels, rts_track.hip)
static int rts_track_check(const char* who, const RtsTrackParams* p)
{
    if (!p) { rts_set_error("%s: null parameters", who); return RTS_ERR_INVALID; }
    switch (rts_track_params_check(p)) {
        case 0: return RTS_OK;
        case 1: rts_set_error("%s: gate = %g (finite, > 0)", who, p->gate); break;
        case 2: rts_set_error("%s: sigma_delay = %g (finite, > 0)", who, p->sigma_delay); break;
        case 3: rts_set_error("%s: sigma_doppler = %g (finite, > 0)", who, p->sigma_doppler); break;
        case 4: rts_set_error("%s: q = %g (finite, >= 0)", who, p->q); break;
        case 5: rts_set_error("%s: delay_rate_per_hz = %g (finite)", who, p->delay_rate_per_hz); break;
        case 6: rts_set_error("%s: doppler_period = %g (finite, >= 0)", who, p->doppler_period); break;
        case 7: rts_set_error("%s: confirm_hits = 0", who); break;
        case 8: rts_set_error("%s: max_candidates = %u (1 .. %u, RTS_TRACK_MAX_CAND)", who, p->max_candidates, RTS_TRACK_MAX_CAND); break;
        case 9: rts_set_error("%s: max_tracks = %u > %u (RTS_TRACK_MAX_TRACKS)", who, p->max_tracks, RTS_TRACK_MAX_TRACKS); break;
        case 10: rts_set_error("%s: reserved fields must be 0", who); break;
        case 11: rts_set_error("%s: n_plots = %u without device_plots", who, p->n_plots); break;
        case 12: rts_set_error("%s: n_plots = %u > %u (RTS_TRACK_MAX_PLOTS)", who, p->n_plots, RTS_TRACK_MAX_PLOTS); break;
        default: rts_set_error("%s: device_plots is not 8-byte aligned", who); break;
    }
    return RTS_ERR_INVALID;
}
static int rts_track_table_refuse(const char* who, const RtsTrack* t, uint32_t n)
{
    uint32_t bad = 0;
    switch (rts_track_table_check(t, n, &bad)) {
        case 0: return RTS_OK;
        case 1: rts_set_error("%s: tracks[%u]: delay, doppler, p_dd, p_df, p_ff must be finite and p_dd, p_ff not negative", who, bad); break;
        default: rts_set_error("%s: tracks[%u]: unknown flags 0x%x", who, bad, t[bad].flags); break;
    }
    return RTS_ERR_INVALID;
}

extern "C" int rts_tracks_eval(const RtsTrackParams* p, const RtsTrack* in, uint32_t n_in, uint64_t next_id, double T, const RtsPlot* plots, uint32_t n_plots,
                               RtsTrack* out, uint32_t capacity, uint32_t* n_out, uint64_t* next_id_out)
{
    const char* who = "rts_tracks_eval";
    RTS_TRY(rts_track_check(who, p));
    if ((n_in && !in) || (n_plots && !plots) || !n_out || !next_id_out || (capacity && !out)) { rts_set_error("%s: null tracks, plots or output", who); return RTS_ERR_INVALID; }
    if (n_in > rts_track_table_size(*p)) { rts_set_error("%s: n_in = %u tracks > max_tracks = %u", who, n_in, rts_track_table_size(*p)); return RTS_ERR_INVALID; }
    if (n_plots > RTS_TRACK_MAX_PLOTS) { rts_set_error("%s: n_plots = %u > %u (RTS_TRACK_MAX_PLOTS)", who, n_plots, RTS_TRACK_MAX_PLOTS); return RTS_ERR_INVALID; }
    if (n_in && !rts_track_interval_ok(T)) { rts_set_error("%s: T = %g with tracks (positive, finite)", who, T); return RTS_ERR_INVALID; }
    RTS_TRY(rts_track_table_refuse(who, in, n_in));
    uint32_t bad = 0;
    if (rts_track_plots_check(plots, n_plots, &bad)) { rts_set_error("%s: plots[%u].rx = %u is below plots[%u].rx = %u (rx must not decrease)", who, bad, plots[bad].rx, bad - 1u, plots[bad - 1u].rx); return RTS_ERR_INVALID; }
    const uint32_t total = rts_tracks_eval_host(p, in, n_in, next_id, T, plots, n_plots, out, capacity, next_id_out);
    *n_out = total;
    const uint32_t table = rts_track_table_size(*p);
    return rts_list_fits_check(who, "%s: %u of %u tracks written (max_tracks %u, capacity %u)", rts_list_copied(total, table, capacity), total, table, capacity);
}

extern "C" int rts_cube_track(RtsHandle c, const RtsTrackParams* p, double time)
{
    const char* who = "rts_cube_track";
    CHECK_HANDLE(c);
    if (!p) { rts_set_error("%s: null parameters", who); return RTS_ERR_INVALID; }
    CHECK_CLOSED(c);
    RTS_TRY(rts_track_check(who, p));
    RtsCubeState& s = c->cube;
    const uint32_t table = rts_track_table_size(*p);
    if (s.trk_max && table != s.trk_max) { rts_set_error("%s: max_tracks = %u, the table was made with %u (rts_cube_tracks_reset first)", who, table, s.trk_max); return RTS_ERR_INVALID; }
    if (table < s.trk_loaded) { rts_set_error("%s: max_tracks = %u below the %u tracks loaded", who, table, s.trk_loaded); return RTS_ERR_INVALID; }
    if (!rts_track_finite(time)) { rts_set_error("%s: time = %g (finite)", who, time); return RTS_ERR_INVALID; }
    const double T = s.trk_live ? time - s.trk_time : 0.0;
    if (s.trk_live && !rts_track_interval_ok(T)) { rts_set_error("%s: T = time - the previous frame's = %g (positive, finite)", who, T); return RTS_ERR_INVALID; }
    const RtsPlot* list = (const RtsPlot*)p->device_plots;
    const uint32_t* n_dev = nullptr;
    uint32_t pcap = p->n_plots;
    if (!list) {
        if (!s.plot_valid) { rts_set_error("%s: no plots (rts_cube_plots; plots end at the detect calls and rts_cube_attach) and no device_plots", who); return RTS_ERR_INVALID; }
        list = s.d_plot.p; n_dev = s.d_plot_off.p + s.plot_cap; pcap = s.plot_max;
        if (pcap > RTS_TRACK_MAX_PLOTS) { rts_set_error("%s: a plot list of %u records > %u (RTS_TRACK_MAX_PLOTS)", who, pcap, RTS_TRACK_MAX_PLOTS); return RTS_ERR_INVALID; }
    }
    RTS_TRY(rts_cube_track_device(c, *p, T, list, n_dev, pcap, table));
    s.trk_max = table; s.trk_loaded = 0; s.trk_live = true; s.trk_time = time;
    return RTS_OK;
}

extern "C" int rts_cube_tracks_get(RtsHandle c, RtsTrack* out, uint32_t capacity, uint32_t* n_out, uint64_t* next_id_out)
{
    const char* who = "rts_cube_tracks_get";
    CHECK_HANDLE(c);
    if (!n_out || (capacity && !out)) { rts_set_error("%s: null output", who); return RTS_ERR_INVALID; }
    RtsCubeState& s = c->cube;
    RTS_TRY(rts_cube_track_tables(c));
    RTS_HIP(hipStreamSynchronize(c->stream));
    RtsTrackMeta m;
    RTS_HIP(hipMemcpy(&m, s.d_trk_meta.p + s.trk_cur, sizeof(m), hipMemcpyDeviceToHost));
    *n_out = m.total;
    if (next_id_out) *next_id_out = m.next_id;
    const uint32_t n = m.n < capacity ? m.n : capacity;
    if (n) RTS_HIP(hipMemcpy(out, s.d_trk[s.trk_cur].p, sizeof(RtsTrack) * n, hipMemcpyDeviceToHost));
    return rts_list_fits_check(who, "%s: %u of %u tracks copied (max_tracks %u, capacity %u)", n, m.total, s.trk_max, capacity);
}

// the rounds the matching of the last rts_cube_track took (tools/track_bench.py); synchronises
extern "C" int rts_cube_track_rounds(RtsHandle c, uint32_t* rounds)
{
    CHECK_HANDLE(c);
    if (!rounds) { rts_set_error("rts_cube_track_rounds: null output"); return RTS_ERR_INVALID; }
    RtsCubeState& s = c->cube;
    RTS_TRY(rts_cube_track_tables(c));
    RTS_HIP(hipStreamSynchronize(c->stream));
    RtsTrackMeta m;
    RTS_HIP(hipMemcpy(&m, s.d_trk_meta.p + s.trk_cur, sizeof(m), hipMemcpyDeviceToHost));
    *rounds = m.rounds;
    return RTS_OK;
}

static int rts_tracks_load(RtsContext* c, const RtsTrack* t, uint32_t n, const uint64_t* next_id)
{
    RtsCubeState& s = c->cube;
    RTS_TRY(rts_cube_track_tables(c));
    RTS_HIP(hipStreamSynchronize(c->stream));                 // (an enqueued step may still read and write both tables)
    RtsTrackMeta m;
    RTS_HIP(hipMemcpy(&m, s.d_trk_meta.p + s.trk_cur, sizeof(m), hipMemcpyDeviceToHost));
    m.n = n; m.total = n; m.rounds = 0; m.reserved = 0;
    if (next_id) m.next_id = *next_id;
    if (n) RTS_HIP(hipMemcpy(s.d_trk[s.trk_cur].p, t, sizeof(RtsTrack) * n, hipMemcpyHostToDevice));
    RTS_HIP(hipMemcpy(s.d_trk_meta.p + s.trk_cur, &m, sizeof(m), hipMemcpyHostToDevice));
    s.trk_max = 0; s.trk_loaded = n;
    return RTS_OK;
}

extern "C" int rts_cube_tracks_set(RtsHandle c, const RtsTrack* tracks, uint32_t n, uint64_t next_id, double time)
{
    const char* who = "rts_cube_tracks_set";
    CHECK_HANDLE(c);
    CHECK_CLOSED(c);
    if (n && !tracks) { rts_set_error("%s: null tracks", who); return RTS_ERR_INVALID; }
    if (n > RTS_TRACK_MAX_TRACKS) { rts_set_error("%s: n = %u > %u (RTS_TRACK_MAX_TRACKS)", who, n, RTS_TRACK_MAX_TRACKS); return RTS_ERR_INVALID; }
    if (n && !rts_track_finite(time)) { rts_set_error("%s: time = %g (finite)", who, time); return RTS_ERR_INVALID; }
    RTS_TRY(rts_track_table_refuse(who, tracks, n));
    RTS_TRY(rts_tracks_load(c, tracks, n, &next_id));
    c->cube.trk_live = n != 0u; c->cube.trk_time = time;
    return RTS_OK;
}

extern "C" int rts_cube_tracks_reset(RtsHandle c)
{
    CHECK_HANDLE(c);
    CHECK_CLOSED(c);
    RTS_TRY(rts_tracks_load(c, nullptr, 0, nullptr));
    c->cube.trk_live = false;
    return RTS_OK;
}

// ------------------------------------------------------------------------------------- track-before-detect
// (rts_amd.h: RtsTbdParams, RtsTbdExtractParams, RtsTbdTrack; the rules and the host evaluators are rts_tbd.h, shared with the kernels, rts_tbd.hip)
static int rts_tbd_check(const char* who, const RtsTbdParams* p, uint32_t nd, uint32_t nb)
{
    if (!p) { rts_set_error("%s: null parameters", who); return RTS_ERR_INVALID; }
    switch (rts_tbd_params_check(p, nd, nb)) {
        case 0: return RTS_OK;
        case 1: rts_set_error("%s: half_doppler = %u > %u (RTS_TBD_MAX_HALF_DOPPLER)", who, p->half_doppler, RTS_TBD_MAX_HALF_DOPPLER); break;
        case 2: rts_set_error("%s: half_range = %u > %u (RTS_TBD_MAX_HALF_RANGE)", who, p->half_range, RTS_TBD_MAX_HALF_RANGE); break;
        case 3: rts_set_error("%s: depth = %u (1 .. %u, RTS_TBD_MAX_DEPTH)", who, p->depth, RTS_TBD_MAX_DEPTH); break;
        case 4: rts_set_error("%s: unknown score %u (RTS_TBD_POWER, RTS_TBD_AMPLITUDE)", who, p->score); break;
        case 5: rts_set_error("%s: unknown flags 0x%x", who, p->flags); break;
        case 6: rts_set_error("%s: reserved fields must be 0", who); break;
        case 7: rts_set_error("%s: scale = %g (finite, > 0)", who, p->scale); break;
        case 8: rts_set_error("%s: decay = %g outside (0, 1]", who, p->decay); break;
        case 9: rts_set_error("%s: delay_rate_per_hz = %g (finite)", who, p->delay_rate_per_hz); break;
        case 10: rts_set_error("%s: pri = %g (finite, >= 0)", who, p->pri); break;
        case 11: rts_set_error("%s: half_doppler = %u: the window (%u rows) exceeds n_doppler = %u", who, p->half_doppler, 2u * p->half_doppler + 1u, nd); break;
        default: rts_set_error("%s: half_range = %u >= n_bins = %u", who, p->half_range, nb); break;
    }
    return RTS_ERR_INVALID;
}
static int rts_tbd_extract_refuse(const char* who, const RtsTbdExtractParams* e)
{
    if (!e) { rts_set_error("%s: null parameters", who); return RTS_ERR_INVALID; }
    switch (rts_tbd_extract_check(e)) {
        case 0: return RTS_OK;
        case 1: rts_set_error("%s: threshold is NaN", who); break;
        case 2: rts_set_error("%s: pri = %g (finite, >= 0)", who, e->pri); break;
        case 3: rts_set_error("%s: unknown flags 0x%x", who, e->flags); break;
        case 4: rts_set_error("%s: max_tracks = %u > %u (RTS_TBD_MAX_TRACKS)", who, e->max_tracks, RTS_TBD_MAX_TRACKS); break;
        default: rts_set_error("%s: reserved fields must be 0", who); break;
    }
    return RTS_ERR_INVALID;
}
// the shape of a map: what an evaluator is given, or what a step finds
static int rts_tbd_shape_check(const char* who, const RtsCubeParams* q, uint32_t nd)
{
    RTS_TRY(rts_eval_cube_check(who, q, false, true));
    const uint32_t n_rx = q->n_rx, nb = q->n_bins;
    if (nd == 0) { rts_set_error("%s: n_doppler = 0", who); return RTS_ERR_INVALID; }
    if ((uint64_t)n_rx * nd * nb > RTS_TBD_MAX_CELLS) { rts_set_error("%s: %u x %u x %u cells > %u (RTS_TBD_MAX_CELLS)", who, n_rx, nd, nb, RTS_TBD_MAX_CELLS); return RTS_ERR_INVALID; }
    return RTS_OK;
}
static int rts_tbd_shifts_refuse(const char* who, const RtsTbdParams* p, uint32_t nd, double T, double dt)
{
    if (!rts_tbd_interval_ok(T)) { rts_set_error("%s: T = time - the previous frame's = %g (positive, finite)", who, T); return RTS_ERR_INVALID; }
    uint32_t bad = 0;
    if (rts_tbd_shifts_check(p, nd, T, dt, &bad)) {
        rts_set_error("%s: the shift of Doppler row %u, ((delay_rate_per_hz f) T) / dt = %g, is not finite or beyond 2^30", who, bad, rts_tbd_shift_quotient(bad, nd, p->delay_rate_per_hz, p->pri, T, dt));
        return RTS_ERR_INVALID;
    }
    return RTS_OK;
}

extern "C" int rts_tbd_step_eval(const RtsCubeParams* q, const double* map, uint32_t n_doppler, const double* merit_in, const RtsTbdParams* p, double T,
                                 double* merit_out, uint8_t* ptr_out, int32_t* shifts_out)
{
    const char* who = "rts_tbd_step_eval";
    RTS_TRY(rts_tbd_shape_check(who, q, n_doppler));
    RTS_TRY(rts_tbd_check(who, p, n_doppler, q->n_bins));
    if (!map || !merit_out || !ptr_out || !shifts_out || merit_out == merit_in) { rts_set_error("%s: null map or output (merit_out must not be merit_in)", who); return RTS_ERR_INVALID; }
    if (merit_in) RTS_TRY(rts_tbd_shifts_refuse(who, p, n_doppler, T, q->dt));
    rts_tbd_step_host(p, q->n_rx, n_doppler, q->n_bins, q->dt, map, merit_in, T, merit_out, ptr_out, shifts_out);
    return RTS_OK;
}

extern "C" int rts_tbd_extract_eval(const RtsCubeParams* q, uint32_t n_doppler, const RtsTbdParams* p, const double* merit, const uint8_t* ptrs, const int32_t* shifts,
                                    uint32_t n_frames, const RtsTbdExtractParams* e, RtsTbdTrack* out, uint32_t* paths, uint32_t capacity, uint32_t* n_out)
{
    const char* who = "rts_tbd_extract_eval";
    RTS_TRY(rts_tbd_shape_check(who, q, n_doppler));
    RTS_TRY(rts_tbd_check(who, p, n_doppler, q->n_bins));
    RTS_TRY(rts_tbd_extract_refuse(who, e));
    if (n_frames == 0 || n_frames > p->depth) { rts_set_error("%s: n_frames = %u (1 .. depth = %u)", who, n_frames, p->depth); return RTS_ERR_INVALID; }
    if (!merit || !ptrs || !shifts || !n_out || (capacity && (!out || !paths))) { rts_set_error("%s: null merit, pointer maps, shift tables or output", who); return RTS_ERR_INVALID; }
    const uint32_t total = rts_tbd_extract_host(p, e, q->n_rx, n_doppler, q->n_bins, q->t0, q->dt, merit, ptrs, shifts, n_frames, out, paths, capacity);
    *n_out = total;
    return rts_list_fits_check(who, "%s: %u of %u tracks written (max_tracks %u, capacity %u)", rts_list_copied(total, rts_tbd_max_tracks(*e), capacity), total, rts_tbd_max_tracks(*e), capacity);
}

extern "C" int rts_cube_tbd_step(RtsHandle c, const RtsTbdParams* p, double time, const void* device_map, uint32_t n_doppler)
{
    const char* who = "rts_cube_tbd_step";
    CHECK_HANDLE(c);
    if (!p) { rts_set_error("%s: null parameters", who); return RTS_ERR_INVALID; }
    CHECK_CLOSED(c);
    NEED_CUBE(c, who, "no cube (call rts_cube_attach first)");
    const double* map;
    RTS_TRY(rts_cfar_map(c, who, device_map, &map, &n_doppler));
    RtsCubeState& s = c->cube;
    const RtsCubeParams& q = s.params;
    RTS_TRY(rts_tbd_shape_check(who, &q, n_doppler));
    RTS_TRY(rts_tbd_check(who, p, n_doppler, q.n_bins));
    if (!rts_tbd_finite(time)) { rts_set_error("%s: time = %g (finite)", who, time); return RTS_ERR_INVALID; }
    const bool first = s.tbd_frames == 0;
    double T = 0.0;
    if (!first) {
        if (q.n_rx != s.tbd_rx || n_doppler != s.tbd_nd || q.n_bins != s.tbd_nb) {
            rts_set_error("%s: a map of %u x %u x %u cells, the state has %u x %u x %u (rts_cube_tbd_reset first)", who, q.n_rx, n_doppler, q.n_bins, s.tbd_rx, s.tbd_nd, s.tbd_nb); return RTS_ERR_INVALID; }
        if (p->depth != s.tbd_depth || p->half_doppler != s.tbd_hd || p->half_range != s.tbd_hr) {
            rts_set_error("%s: depth, half_doppler, half_range = %u, %u, %u, the state was made with %u, %u, %u (rts_cube_tbd_reset first)", who, p->depth, p->half_doppler, p->half_range,
                          s.tbd_depth, s.tbd_hd, s.tbd_hr); return RTS_ERR_INVALID; }
        T = time - s.tbd_time;
        RTS_TRY(rts_tbd_shifts_refuse(who, p, n_doppler, T, q.dt));
    } else {
        // the state's buffers, of their final sizes (a DevBuf that grows drops what it held: they are made once per state)
        const size_t cells = (size_t)q.n_rx * n_doppler * q.n_bins;
        RTS_HIP(s.d_tbd_merit[0].reserve(cells)); RTS_HIP(s.d_tbd_merit[1].reserve(cells));
        RTS_HIP(s.d_tbd_ptr.reserve(cells * p->depth)); RTS_HIP(s.d_tbd_shift.reserve((size_t)n_doppler * p->depth));
        s.tbd_rx = q.n_rx; s.tbd_nd = n_doppler; s.tbd_nb = q.n_bins; s.tbd_depth = p->depth; s.tbd_hd = p->half_doppler; s.tbd_hr = p->half_range; s.tbd_cur = 0;
    }
    RTS_TRY(rts_cube_tbd_step_device(c, *p, map, first, T, q.dt, (uint32_t)(s.tbd_frames % s.tbd_depth)));
    s.tbd_frames++; s.tbd_time = time; s.tbd_t0 = q.t0; s.tbd_dt = q.dt;
    return RTS_OK;
}

#define NEED_TBD(c, who) do { if ((c)->cube.tbd_frames == 0) { rts_set_error("%s: no track-before-detect state (rts_cube_tbd_step; a state ends at rts_cube_tbd_reset)", (who)); return RTS_ERR_INVALID; } } while (0)

extern "C" int rts_cube_tbd_extract(RtsHandle c, const RtsTbdExtractParams* e)
{
    const char* who = "rts_cube_tbd_extract";
    CHECK_HANDLE(c);
    RTS_TRY(rts_tbd_extract_refuse(who, e));
    CHECK_CLOSED(c);
    NEED_TBD(c, who);
    c->cube.tbd_ext_valid = false;
    return rts_cube_tbd_extract_device(c, *e, rts_tbd_max_tracks(*e));
}

// the extraction's records or their paths (record_bytes each) -> the host: the total, and how many of the stored ones fit `capacity`
static int rts_tbd_extracted(RtsContext* c, const char* who, const void* d_list, size_t record_bytes, void* out, uint32_t capacity, uint32_t* total, uint32_t* n)
{
    RtsCubeState& s = c->cube;
    if (!s.tbd_ext_valid) { rts_set_error("%s: no extraction (rts_cube_tbd_extract; it ends at rts_cube_tbd_reset)", who); return RTS_ERR_INVALID; }
    return rts_list_copy_out(c, s.d_tbd_off.p + s.tbd_ext_nseg, s.tbd_ext_max, d_list, record_bytes, out, capacity, total, n);
}

extern "C" int rts_cube_tbd_tracks_get(RtsHandle c, RtsTbdTrack* out, uint32_t capacity, uint32_t* n_out)
{
    const char* who = "rts_cube_tbd_tracks_get";
    CHECK_HANDLE(c);
    if (!n_out || (capacity && !out)) { rts_set_error("%s: null output", who); return RTS_ERR_INVALID; }
    uint32_t total = 0, n = 0;
    RTS_TRY(rts_tbd_extracted(c, who, c->cube.d_tbd_out.p, sizeof(RtsTbdTrack), out, capacity, &total, &n));
    *n_out = total;
    return rts_list_fits_check(who, "%s: %u of %u tracks copied (max_tracks %u, capacity %u)", n, total, c->cube.tbd_ext_max, capacity);
}

extern "C" int rts_cube_tbd_paths_get(RtsHandle c, uint32_t* out, uint32_t capacity_tracks)
{
    const char* who = "rts_cube_tbd_paths_get";
    CHECK_HANDLE(c);
    if (capacity_tracks && !out) { rts_set_error("%s: null output", who); return RTS_ERR_INVALID; }
    uint32_t total = 0, n = 0;
    RTS_TRY(rts_tbd_extracted(c, who, c->cube.d_tbd_paths.p, sizeof(uint32_t) * 2u * c->cube.tbd_ext_depth, out, capacity_tracks, &total, &n));
    return rts_list_fits_check(who, "%s: the paths of %u of %u tracks copied (max_tracks %u, capacity %u)", n, total, c->cube.tbd_ext_max, capacity_tracks);
}

extern "C" int rts_cube_tbd_merit_get(RtsHandle c, double* host_out, uint64_t capacity_doubles)
{
    const char* who = "rts_cube_tbd_merit_get";
    CHECK_HANDLE(c);
    NEED_TBD(c, who);
    RtsCubeState& s = c->cube;
    const size_t cells = (size_t)s.tbd_rx * s.tbd_nd * s.tbd_nb;
    if (!host_out) { rts_set_error("%s: null output", who); return RTS_ERR_INVALID; }
    if (capacity_doubles < cells) { rts_set_error("%s: capacity too small", who); return RTS_ERR_CAPACITY; }
    RTS_HIP(hipStreamSynchronize(c->stream));
    RTS_HIP(hipMemcpy(host_out, s.d_tbd_merit[s.tbd_cur].p, sizeof(double) * cells, hipMemcpyDeviceToHost));
    return RTS_OK;
}

extern "C" int rts_cube_tbd_ring_get(RtsHandle c, uint8_t* ptr_out, int32_t* shifts_out, uint32_t capacity_frames, uint32_t* n_frames_out)
{
    const char* who = "rts_cube_tbd_ring_get";
    CHECK_HANDLE(c);
    NEED_TBD(c, who);
    RtsCubeState& s = c->cube;
    if (!n_frames_out || (capacity_frames && (!ptr_out || !shifts_out))) { rts_set_error("%s: null output", who); return RTS_ERR_INVALID; }
    const uint32_t have = s.tbd_frames < s.tbd_depth ? (uint32_t)s.tbd_frames : s.tbd_depth;
    *n_frames_out = have;
    if (capacity_frames < have) { rts_set_error("%s: %u frames stored, capacity %u", who, have, capacity_frames); return RTS_ERR_CAPACITY; }
    const size_t cells = (size_t)s.tbd_rx * s.tbd_nd * s.tbd_nb;
    RTS_HIP(hipStreamSynchronize(c->stream));
    for (uint32_t i = 0; i < have; i++) {                               // oldest first: frame frames - have + i
        const size_t slot = (size_t)((s.tbd_frames - have + i) % s.tbd_depth);
        RTS_HIP(hipMemcpy(ptr_out + (size_t)i * cells, s.d_tbd_ptr.p + slot * cells, cells, hipMemcpyDeviceToHost));
        RTS_HIP(hipMemcpy(shifts_out + (size_t)i * s.tbd_nd, s.d_tbd_shift.p + slot * s.tbd_nd, sizeof(int32_t) * s.tbd_nd, hipMemcpyDeviceToHost));
    }
    return RTS_OK;
}

extern "C" int rts_cube_tbd_info(RtsHandle c, uint32_t shape_out[4], uint64_t* frames_out)
{
    CHECK_HANDLE(c);
    if (!shape_out || !frames_out) { rts_set_error("rts_cube_tbd_info: null output"); return RTS_ERR_INVALID; }
    const RtsCubeState& s = c->cube;
    const bool have = s.tbd_frames != 0;
    shape_out[0] = have ? s.tbd_rx : 0u; shape_out[1] = have ? s.tbd_nd : 0u; shape_out[2] = have ? s.tbd_nb : 0u; shape_out[3] = have ? s.tbd_depth : 0u;
    *frames_out = s.tbd_frames;
    return RTS_OK;
}

extern "C" int rts_cube_tbd_reset(RtsHandle c)
{
    CHECK_HANDLE(c);
    c->cube.tbd_frames = 0; c->cube.tbd_ext_valid = false;      // (the buffers stay: work enqueued on them runs before the next state's, on the same stream)
    return RTS_OK;
}

// ------------------------------------------------------------------------------------- tapered slow-time spectrogram
// (rts_amd.h: RtsStftParams; the tree and the launch plan are rts_stft.h, shared by the host export and the kernel, rts_stft.hip)
static int rts_stft_check(const RtsStftParams* p, const RtsCubeParams& q, const char* who, RtsStftPlan* plan)
{
    if (!p) { rts_set_error("%s: null parameters", who); return RTS_ERR_INVALID; }
    if (p->reserved[0] || p->reserved[1]) { rts_set_error("%s: reserved fields must be 0", who); return RTS_ERR_INVALID; }
    if (p->flags & ~(RTS_STFT_POWER | RTS_STFT_SUM_BINS)) { rts_set_error("%s: unknown flags 0x%x", who, p->flags); return RTS_ERR_INVALID; }
    if ((p->flags & RTS_STFT_SUM_BINS) && !(p->flags & RTS_STFT_POWER)) { rts_set_error("%s: flags: RTS_STFT_SUM_BINS needs RTS_STFT_POWER", who); return RTS_ERR_INVALID; }
    RTS_TRY(rts_fft_size_check(who, p->n_fft, RTS_STFT_MAX_FFT));
    RTS_TRY(rts_pulses_check(who, p->first_pulse, p->n_pulses, q.n_pulses, true));
    if (p->window_len == 0 || p->window_len > p->n_fft || p->window_len > p->n_pulses) { rts_set_error("%s: window_len = %u (1 .. n_fft = %u, <= n_pulses = %u)", who, p->window_len, p->n_fft, p->n_pulses); return RTS_ERR_INVALID; }
    if (p->hop == 0) { rts_set_error("%s: hop = 0 (>= 1)", who); return RTS_ERR_INVALID; }
    uint32_t n_gate = 0;
    RTS_TRY(rts_gate_check(who, "%s: first_bin = %u, n_bins = %u: inside the cube's %u bins", p->first_bin, p->n_bins, q.n_bins, &n_gate));
    RTS_TRY(rts_window_finite_check(who, p->window, p->window_len));
    *plan = rts_stft_plan(q.n_rx, p->n_pulses, p->window_len, p->hop, p->n_fft, n_gate, p->flags);
    if (!plan->supported) {
        if (q.n_rx > RTS_STFT_MAX_RX) rts_set_error("%s: n_rx = %u receivers: more than %u (the launch grid)", who, q.n_rx, RTS_STFT_MAX_RX);
        else rts_set_error("%s: n_frames = %u frames x %u workgroups per frame (hop, n_bins): more than %u (the launch grid)", who, plan->n_frames, plan->tiles, RTS_STFT_MAX_GRID_X);
        return RTS_ERR_INVALID;
    }
    return RTS_OK;
}

extern "C" int rts_window_make(uint32_t kind, uint32_t n, double* out)
{
    if (n == 0) { rts_set_error("rts_window_make: n = 0"); return RTS_ERR_INVALID; }
    if (kind > RTS_WINDOW_BLACKMAN) { rts_set_error("rts_window_make: unknown kind %u", kind); return RTS_ERR_INVALID; }
    if (!out) { rts_set_error("rts_window_make: null output array"); return RTS_ERR_INVALID; }
    rts_stft_window_host(kind, n, out);
    return RTS_OK;
}

extern "C" int rts_stft_eval(const RtsCubeParams* q, const double* cube, const RtsStftParams* p, double* out, uint32_t* n_frames_out)
{
    RTS_TRY(rts_eval_cube_check("rts_stft_eval", q, true, false));
    RtsStftPlan plan;
    RTS_TRY(rts_stft_check(p, *q, "rts_stft_eval", &plan));
    if (!cube || !out) { rts_set_error("rts_stft_eval: null cube or output array"); return RTS_ERR_INVALID; }
    std::vector<double> work(4 * (size_t)p->n_fft);
    rts_stft_eval_host(q, cube, p, plan, out, work.data());
    if (n_frames_out) *n_frames_out = plan.n_frames;
    return RTS_OK;
}

extern "C" int rts_cube_spectrogram(RtsHandle c, const RtsStftParams* p, void* device_out, uint32_t* n_frames_out)
{
    CHECK_HANDLE(c);
    NEED_CUBE(c, "rts_cube_spectrogram", "no cube (call rts_cube_attach first)");
    const RtsCubeParams& q = c->cube.params;
    RtsStftPlan plan;
    RTS_TRY(rts_stft_check(p, q, "rts_cube_spectrogram", &plan));
    if ((uintptr_t)device_out & 15u) { rts_set_error("rts_cube_spectrogram: device_out is not 16-byte aligned"); return RTS_ERR_INVALID; }
    CHECK_CLOSED(c);
    double* out; RTS_HIP(c->cube.stft.place(device_out, plan.out_doubles, &out));
    // the window -> pinned staging -> the device, on the stream (window_len <= RTS_STFT_MAX_FFT: one size for every call)
    const double* win = nullptr;
    if (p->window) {
        RTS_HIP(c->cube.stft_win.upload(p->window, p->window_len, RTS_STFT_MAX_FFT, c->stream));
        win = c->cube.stft_win.dev.p;
    }
    if (!device_out) c->cube.stft.record(out, plan.out_doubles);
    if (n_frames_out) *n_frames_out = plan.n_frames;
    return rts_cube_stft_device(c, *p, plan, win, out);
}

extern "C" int rts_cube_spectrogram_get(RtsHandle c, double* host_out, uint64_t capacity_doubles)
{
    CHECK_HANDLE(c);
    return rts_cube_copy_out(c, "rts_cube_spectrogram_get", "no library-owned spectrogram (rts_cube_spectrogram with device_out NULL; a spectrogram ends at rts_cube_attach) / null output", c->cube.stft, host_out, capacity_doubles);
}

// ------------------------------------------------------------------------------------- autofocus: range alignment, phase-gradient autofocus, correction
// (rts_amd.h: RtsAlignParams, RtsPgaParams, RtsCorrectParams; the arithmetic and the launch plans are rts_focus.h, shared by the host exports and the kernels, rts_focus.hip)
static int rts_focus_gate_check(const char* who, uint32_t first_bin, uint32_t n_gate, uint32_t n_bins, uint32_t* gate)
{
    return rts_gate_check(who, "%s: first_bin = %u, n_gate = %u: inside the cube's %u bins", first_bin, n_gate, n_bins, gate);
}
static int rts_focus_rx_check(const char* who, uint32_t n_rx)
{
    if (n_rx > RTS_FOCUS_MAX_RX) { rts_set_error("%s: n_rx = %u receivers: more than %u (the launch grid)", who, n_rx, RTS_FOCUS_MAX_RX); return RTS_ERR_INVALID; }
    return RTS_OK;
}

static int rts_align_check(const RtsAlignParams* p, const RtsCubeParams& q, const char* who, RtsAlignPlan* plan)
{
    if (!p) { rts_set_error("%s: null parameters", who); return RTS_ERR_INVALID; }
    if (p->reserved0 || p->reserved[0] || p->reserved[1]) { rts_set_error("%s: reserved fields must be 0", who); return RTS_ERR_INVALID; }
    if (p->flags & ~RTS_ALIGN_INTEGER) { rts_set_error("%s: unknown flags 0x%x", who, p->flags); return RTS_ERR_INVALID; }
    RTS_TRY(rts_pulses_check(who, p->first_pulse, p->n_pulses, q.n_pulses, true));
    uint32_t gate = 0;
    RTS_TRY(rts_focus_gate_check(who, p->first_bin, p->n_gate, q.n_bins, &gate));
    if (p->max_lag > RTS_ALIGN_MAX_LAG) { rts_set_error("%s: max_lag = %u (0 .. %u)", who, p->max_lag, RTS_ALIGN_MAX_LAG); return RTS_ERR_INVALID; }
    if (p->n_iters == 0 || p->n_iters > RTS_ALIGN_MAX_ITERS) { rts_set_error("%s: n_iters = %u (1 .. %u)", who, p->n_iters, RTS_ALIGN_MAX_ITERS); return RTS_ERR_INVALID; }
    RTS_TRY(rts_focus_rx_check(who, q.n_rx));
    *plan = rts_align_plan(q.n_rx, p->n_pulses, q.n_bins, gate, p->max_lag);
    if (!plan->supported) { rts_set_error("%s: n_pulses = %u rows: more than %u (the launch grid)", who, p->n_pulses, RTS_FOCUS_MAX_GRID_X); return RTS_ERR_INVALID; }
    return RTS_OK;
}

static int rts_pga_check(const RtsPgaParams* p, const RtsCubeParams& q, const char* who, RtsPgaPlan* plan)
{
    if (!p) { rts_set_error("%s: null parameters", who); return RTS_ERR_INVALID; }
    if (p->reserved0 || p->reserved[0] || p->reserved[1]) { rts_set_error("%s: reserved fields must be 0", who); return RTS_ERR_INVALID; }
    if (!rts_pow2_in(p->n_pulses, 4u, RTS_PGA_MAX_PULSES)) {
        rts_set_error("%s: n_pulses = %u must be a power of two in [4, %u] (the radix-2 transform; no zero padding of a phase history)", who, p->n_pulses, RTS_PGA_MAX_PULSES); return RTS_ERR_INVALID; }
    RTS_TRY(rts_pulses_check(who, p->first_pulse, p->n_pulses, q.n_pulses, true));
    uint32_t gate = 0;
    RTS_TRY(rts_focus_gate_check(who, p->first_bin, p->n_gate, q.n_bins, &gate));
    if (p->n_iters == 0 || p->n_iters > RTS_PGA_MAX_ITERS) { rts_set_error("%s: n_iters = %u (1 .. %u)", who, p->n_iters, RTS_PGA_MAX_ITERS); return RTS_ERR_INVALID; }
    RTS_TRY(rts_focus_rx_check(who, q.n_rx));
    *plan = rts_pga_plan(q.n_rx, p->n_pulses, gate, p->n_iters, p->window0, p->window_min);
    if (!plan->supported) { rts_set_error("%s: n_pulses = %u: the columns do not fit the workgroup's memory", who, p->n_pulses); return RTS_ERR_INVALID; }
    return RTS_OK;
}

// handle: the USE flags are allowed (the evaluators have no tables)
static int rts_correct_check(const RtsCorrectParams* p, const RtsCubeParams& q, const char* who, bool handle, RtsCorrectPlan* plan)
{
    if (!p) { rts_set_error("%s: null parameters", who); return RTS_ERR_INVALID; }
    if (p->reserved[0] || p->reserved[1]) { rts_set_error("%s: reserved fields must be 0", who); return RTS_ERR_INVALID; }
    if (p->flags & ~(RTS_CORRECT_USE_ALIGN | RTS_CORRECT_USE_PGA)) { rts_set_error("%s: unknown flags 0x%x", who, p->flags); return RTS_ERR_INVALID; }
    if (p->flags && !handle) { rts_set_error("%s: flags = 0x%x: the evaluator has no tables (pass shifts / phase)", who, p->flags); return RTS_ERR_INVALID; }
    RTS_TRY(rts_pulses_check(who, p->first_pulse, p->n_pulses, q.n_pulses, true));
    RTS_TRY(rts_taps_check(who, p->taps));
    const bool use_s = (p->flags & RTS_CORRECT_USE_ALIGN) != 0, use_p = (p->flags & RTS_CORRECT_USE_PGA) != 0;
    if (use_s && p->shifts) { rts_set_error("%s: shifts together with RTS_CORRECT_USE_ALIGN", who); return RTS_ERR_INVALID; }
    if (use_p && p->phase) { rts_set_error("%s: phase together with RTS_CORRECT_USE_PGA", who); return RTS_ERR_INVALID; }
    if (!use_s && !use_p && !p->shifts && !p->phase) { rts_set_error("%s: neither shifts nor phase (arrays or flags)", who); return RTS_ERR_INVALID; }
    RTS_TRY(rts_focus_rx_check(who, q.n_rx));
    const size_t n = (size_t)q.n_rx * p->n_pulses;
    if (p->shifts) for (size_t i = 0; i < n; i++) if (!std::isfinite(p->shifts[i])) { rts_set_error("%s: shifts[%zu] is not finite", who, i); return RTS_ERR_INVALID; }
    if (p->phase) for (size_t i = 0; i < n; i++) if (!std::isfinite(p->phase[i])) { rts_set_error("%s: phase[%zu] is not finite", who, i); return RTS_ERR_INVALID; }
    *plan = rts_correct_plan(q.n_rx, p->n_pulses, q.n_bins, p->shifts != nullptr, p->phase != nullptr, use_s || p->shifts);
    if (!plan->supported) { rts_set_error("%s: n_pulses = %u rows x %u workgroups per row (n_bins): more than %u (the launch grid)", who, p->n_pulses, plan->tiles, RTS_FOCUS_MAX_GRID_X); return RTS_ERR_INVALID; }
    return RTS_OK;
}

extern "C" int rts_align_eval(const RtsCubeParams* q, const double* cube, const RtsAlignParams* p, double* out)
{
    RTS_TRY(rts_eval_cube_check("rts_align_eval", q, true, false));
    RtsAlignPlan plan;
    RTS_TRY(rts_align_check(p, *q, "rts_align_eval", &plan));
    if (!cube || !out) { rts_set_error("rts_align_eval: null cube or output array"); return RTS_ERR_INVALID; }
    std::vector<double> work((size_t)p->n_pulses * q->n_bins + plan.n_gate + plan.n_lags);
    rts_align_eval_host(q, cube, p, plan, out, work.data());
    return RTS_OK;
}

extern "C" int rts_pga_eval(const RtsCubeParams* q, const double* cube, const RtsPgaParams* p, double* phase_out, double* rms_out)
{
    RTS_TRY(rts_eval_cube_check("rts_pga_eval", q, true, false));
    RtsPgaPlan plan;
    RTS_TRY(rts_pga_check(p, *q, "rts_pga_eval", &plan));
    if (!cube || !phase_out || !rms_out) { rts_set_error("rts_pga_eval: null cube or output array"); return RTS_ERR_INVALID; }
    std::vector<double> work(14 * (size_t)p->n_pulses);
    rts_pga_eval_host(q, cube, p, plan, phase_out, rms_out, work.data());
    return RTS_OK;
}

extern "C" int rts_correct_eval(const RtsCubeParams* q, double* cube, const RtsCorrectParams* p)
{
    RTS_TRY(rts_eval_cube_check("rts_correct_eval", q, true, false));
    RtsCorrectPlan plan;
    RTS_TRY(rts_correct_check(p, *q, "rts_correct_eval", false, &plan));
    if (!cube) { rts_set_error("rts_correct_eval: null cube"); return RTS_ERR_INVALID; }
    std::vector<double> work(2 * (size_t)q->n_bins);
    rts_correct_eval_host(q, cube, p, p->shifts, p->phase, work.data());
    return RTS_OK;
}

extern "C" int rts_cube_align(RtsHandle c, const RtsAlignParams* p, void* device_out)
{
    const char* who = "rts_cube_align";
    CHECK_HANDLE(c);
    NEED_CUBE(c, who, "no cube (call rts_cube_attach first)");
    RtsAlignPlan plan;
    RTS_TRY(rts_align_check(p, c->cube.params, who, &plan));
    if ((uintptr_t)device_out & 7u) { rts_set_error("%s: device_out is not 8-byte aligned", who); return RTS_ERR_INVALID; }
    CHECK_CLOSED(c);
    double* out; RTS_HIP(c->cube.align.place(device_out, plan.out_doubles, &out));
    if (!device_out) { c->cube.align.record(out, plan.out_doubles); c->cube.align_first = p->first_pulse; c->cube.align_P = p->n_pulses; }
    return rts_cube_align_device(c, *p, plan, out);
}

extern "C" int rts_cube_align_get(RtsHandle c, double* host_out, uint64_t capacity_doubles)
{
    CHECK_HANDLE(c);
    return rts_cube_copy_out(c, "rts_cube_align_get", "no library-owned shift table (rts_cube_align with device_out NULL; a table ends at rts_cube_attach) / null output", c->cube.align, host_out, capacity_doubles);
}

extern "C" int rts_cube_pga(RtsHandle c, const RtsPgaParams* p, void* device_out)
{
    const char* who = "rts_cube_pga";
    CHECK_HANDLE(c);
    NEED_CUBE(c, who, "no cube (call rts_cube_attach first)");
    RtsPgaPlan plan;
    RTS_TRY(rts_pga_check(p, c->cube.params, who, &plan));
    if ((uintptr_t)device_out & 7u) { rts_set_error("%s: device_out is not 8-byte aligned", who); return RTS_ERR_INVALID; }
    CHECK_CLOSED(c);
    double* out; RTS_HIP(c->cube.pga.place(device_out, plan.out_doubles, &out));
    if (!device_out) { c->cube.pga.record(out, plan.out_doubles); c->cube.pga_first = p->first_pulse; c->cube.pga_P = p->n_pulses; c->cube.pga_iters = p->n_iters; }
    return rts_cube_pga_device(c, *p, plan, out);
}

extern "C" int rts_cube_pga_get(RtsHandle c, double* phase_out, double* rms_out, uint64_t capacity_phase, uint64_t capacity_rms)
{
    const char* who = "rts_cube_pga_get";
    CHECK_HANDLE(c);
    const RtsCubeState& s = c->cube;
    if (!s.set || !s.pga.valid) { rts_set_error("%s: no library-owned phase table (rts_cube_pga with device_out NULL; a table ends at rts_cube_attach)", who); return RTS_ERR_INVALID; }
    if (!phase_out && !rms_out) { rts_set_error("%s: null outputs", who); return RTS_ERR_INVALID; }
    const size_t n_phase = (size_t)s.params.n_rx * s.pga_P, n_rms = (size_t)s.params.n_rx * s.pga_iters;
    if ((phase_out && capacity_phase < n_phase) || (rms_out && capacity_rms < n_rms)) { rts_set_error("%s: capacity too small", who); return RTS_ERR_CAPACITY; }
    RTS_HIP(hipStreamSynchronize(c->stream));
    if (phase_out) RTS_HIP(hipMemcpy(phase_out, s.pga.p, sizeof(double) * n_phase, hipMemcpyDeviceToHost));
    if (rms_out) RTS_HIP(hipMemcpy(rms_out, s.pga.p + n_phase, sizeof(double) * n_rms, hipMemcpyDeviceToHost));
    return RTS_OK;
}

extern "C" int rts_cube_correct(RtsHandle c, const RtsCorrectParams* p)
{
    const char* who = "rts_cube_correct";
    CHECK_HANDLE(c);
    NEED_CUBE(c, who, "no cube (call rts_cube_attach first)");
    RtsCubeState& s = c->cube;
    RtsCorrectPlan plan;
    RTS_TRY(rts_correct_check(p, s.params, who, true, &plan));
    const double* shifts = nullptr; const double* phase = nullptr;
    if (p->flags & RTS_CORRECT_USE_ALIGN) {
        if (!s.align.valid || s.align_first != p->first_pulse || s.align_P != p->n_pulses) { rts_set_error("%s: RTS_CORRECT_USE_ALIGN: no library-owned shift table of rows %u .. %u + %u (rts_cube_align with device_out NULL)", who, p->first_pulse, p->first_pulse, p->n_pulses); return RTS_ERR_INVALID; }
        shifts = s.align.p;
    }
    if (p->flags & RTS_CORRECT_USE_PGA) {
        if (!s.pga.valid || s.pga_first != p->first_pulse || s.pga_P != p->n_pulses) { rts_set_error("%s: RTS_CORRECT_USE_PGA: no library-owned phase table of rows %u .. %u + %u (rts_cube_pga with device_out NULL)", who, p->first_pulse, p->first_pulse, p->n_pulses); return RTS_ERR_INVALID; }
        phase = s.pga.p;
    }
    CHECK_CLOSED(c);
    // the host tables -> pinned staging -> the device, on the stream
    if (plan.table_doubles) {
        double* h = nullptr;
        RTS_HIP(s.focus_tab.begin(plan.table_doubles, plan.table_doubles, plan.table_doubles, &h));
        const size_t n = (size_t)s.params.n_rx * p->n_pulses;
        size_t at = 0;
        if (p->shifts) { memcpy(h, p->shifts, sizeof(double) * n); at = n; }
        if (p->phase) memcpy(h + at, p->phase, sizeof(double) * n);
        RTS_HIP(s.focus_tab.send(plan.table_doubles, c->stream));
        if (p->shifts) shifts = s.focus_tab.dev.p;
        if (p->phase) phase = s.focus_tab.dev.p + at;
    }
    return rts_cube_correct_device(c, *p, plan, shifts, phase);
}

// ------------------------------------------------------------------------------------- FMCW: dechirped beat render, fast-time range transform
// (rts_amd.h: RtsBeatParams, RtsRangeParams; the trees and the launch plans are rts_beat.h / rts_stft.h, shared by the host exports and the kernels, rts_beat.hip)
static int rts_beat_check(const RtsBeatParams* p, const RtsCubeParams& q, uint32_t pulse_index, const char* who)
{
    if (!p) { rts_set_error("%s: null parameters", who); return RTS_ERR_INVALID; }
    if (!std::isfinite(p->slope) || p->slope == 0.0) { rts_set_error("%s: slope = %g (finite, != 0)", who, p->slope); return RTS_ERR_INVALID; }
    if (!std::isfinite(p->duration) || !(p->duration > 0.0)) { rts_set_error("%s: duration = %g (finite, > 0)", who, p->duration); return RTS_ERR_INVALID; }
    RTS_TRY(rts_render_source_check(who, p->source, p->flags));
    if (p->reserved[0] || p->reserved[1]) { rts_set_error("%s: reserved fields must be 0", who); return RTS_ERR_INVALID; }
    if (pulse_index >= q.n_pulses) { rts_set_error("%s: pulse_index = %u >= the cube's %u rows", who, pulse_index, q.n_pulses); return RTS_ERR_INVALID; }
    if (q.n_rx > RTS_BEAT_MAX_RX) { rts_set_error("%s: n_rx = %u receivers: more than %u (the launch grid)", who, q.n_rx, RTS_BEAT_MAX_RX); return RTS_ERR_INVALID; }
    return RTS_OK;
}

extern "C" int rts_beat_eval(const RtsCubeParams* q, const RtsBeatParams* p, const RtsBeatContribution* c, uint32_t n, uint32_t pulse_index, double* cube)
{
    RTS_TRY(rts_eval_cube_check("rts_beat_eval", q, true, true));
    RTS_TRY(rts_beat_check(p, *q, pulse_index, "rts_beat_eval"));
    if ((n && !c) || !cube) { rts_set_error("rts_beat_eval: null contribution array or cube"); return RTS_ERR_INVALID; }
    std::vector<double> work(2 * (size_t)q->n_rx * q->n_bins);
    rts_beat_eval_host(q, p, c, n, pulse_index, cube, work.data());
    return RTS_OK;
}

extern "C" int rts_cube_render_beat(RtsHandle c, uint32_t pulse_index, const RtsBeatParams* p, double cspeed, double carrier)
{
    CHECK_HANDLE(c);
    NEED_CUBE(c, "rts_cube_render_beat", "call rts_cube_attach first");
    RTS_TRY(rts_beat_check(p, c->cube.params, pulse_index, "rts_cube_render_beat"));
    const bool paths = p->source == RTS_RENDER_PATHS;
    if (!paths && (!std::isfinite(cspeed) || !(cspeed > 0.0))) { rts_set_error("rts_cube_render_beat: cspeed = %g (finite, > 0, with RTS_RENDER_RAYS)", cspeed); return RTS_ERR_INVALID; }
    if (!paths && (!std::isfinite(carrier) || carrier < 0.0)) { rts_set_error("rts_cube_render_beat: carrier = %g (finite, >= 0, with RTS_RENDER_RAYS)", carrier); return RTS_ERR_INVALID; }
    CHECK_CLOSED(c);
    if (paths) RTS_TRY(rts_render_paths_check(c, "rts_cube_render_beat"));
    const RtsBeatPlan plan = rts_beat_plan(c->res.n_recv, c->cube.params.n_rx, c->cube.params.n_bins, c->tune.beat_force_parts);
    if (!plan.supported) { rts_set_error("rts_cube_render_beat: %llu received rays: more than the launch takes", (unsigned long long)c->res.n_recv); return RTS_ERR_INVALID; }
    return rts_cube_beat_device(c, pulse_index, *p, plan, cspeed, carrier, c->res.agg_base_local);
}

static int rts_range_check(const RtsRangeParams* p, const RtsCubeParams& q, const char* who, RtsRangePlan* plan)
{
    if (!p) { rts_set_error("%s: null parameters", who); return RTS_ERR_INVALID; }
    if (p->reserved0 || p->reserved[0] || p->reserved[1]) { rts_set_error("%s: reserved fields must be 0", who); return RTS_ERR_INVALID; }
    if (p->flags & ~RTS_RANGE_REVERSE) { rts_set_error("%s: unknown flags 0x%x", who, p->flags); return RTS_ERR_INVALID; }
    RTS_TRY(rts_fft_size_check(who, p->n_fft, RTS_RANGE_MAX_FFT));
    RTS_TRY(rts_pulses_check(who, p->first_pulse, p->n_pulses, q.n_pulses, true));
    uint32_t n_samples = 0;
    RTS_TRY(rts_gate_check(who, "%s: first_bin = %u, n_samples = %u: inside the row's %u bins", p->first_bin, p->n_samples, q.n_bins, &n_samples));
    if (n_samples > p->n_fft) { rts_set_error("%s: n_samples = %u > n_fft = %u", who, n_samples, p->n_fft); return RTS_ERR_INVALID; }
    if (p->n_out > p->n_fft) { rts_set_error("%s: n_out = %u > n_fft = %u", who, p->n_out, p->n_fft); return RTS_ERR_INVALID; }
    RTS_TRY(rts_window_finite_check(who, p->window, n_samples));
    *plan = rts_range_plan(q.n_rx, p->n_pulses, n_samples, p->n_fft, p->n_out);
    if (!plan->supported) { rts_set_error("%s: n_rx = %u receivers x n_pulses = %u rows, %u per workgroup: more than %u workgroups (the launch grid)", who, q.n_rx, p->n_pulses, plan->RT, RTS_RANGE_MAX_GRID_X); return RTS_ERR_INVALID; }
    return RTS_OK;
}

extern "C" int rts_range_eval(const RtsCubeParams* q, const double* cube, const RtsRangeParams* p, double* out)
{
    RTS_TRY(rts_eval_cube_check("rts_range_eval", q, true, false));
    RtsRangePlan plan;
    RTS_TRY(rts_range_check(p, *q, "rts_range_eval", &plan));
    if (!cube || !out) { rts_set_error("rts_range_eval: null cube or output array"); return RTS_ERR_INVALID; }
    std::vector<double> work(3 * (size_t)p->n_fft);
    rts_range_eval_host(q, cube, p, plan, out, work.data());
    return RTS_OK;
}

extern "C" int rts_cube_range_transform(RtsHandle c, const RtsRangeParams* p, void* device_out)
{
    CHECK_HANDLE(c);
    NEED_CUBE(c, "rts_cube_range_transform", "no cube (call rts_cube_attach first)");
    const RtsCubeParams& q = c->cube.params;
    RtsRangePlan plan;
    RTS_TRY(rts_range_check(p, q, "rts_cube_range_transform", &plan));
    if ((uintptr_t)device_out & 15u) { rts_set_error("rts_cube_range_transform: device_out is not 16-byte aligned"); return RTS_ERR_INVALID; }
    if ((uintptr_t)c->cube.p & 15u) { rts_set_error("rts_cube_range_transform: the cube's device memory is not 16-byte aligned"); return RTS_ERR_INVALID; }
    CHECK_CLOSED(c);
    double* out; RTS_HIP(c->cube.range.place(device_out, plan.out_doubles, &out));
    // the window -> pinned staging -> the device, on the stream (n_samples <= RTS_RANGE_MAX_FFT: one size for every call)
    const double* win = nullptr;
    if (p->window) {
        RTS_HIP(c->cube.range_win.upload(p->window, plan.n_samples, RTS_RANGE_MAX_FFT, c->stream));
        win = c->cube.range_win.dev.p;
    }
    if (!device_out) c->cube.range.record(out, plan.out_doubles);
    return rts_cube_range_device(c, *p, plan, win, out);
}

extern "C" int rts_cube_range_get(RtsHandle c, double* host_out, uint64_t capacity_doubles)
{
    CHECK_HANDLE(c);
    return rts_cube_copy_out(c, "rts_cube_range_get", "no library-owned range map (rts_cube_range_transform with device_out NULL; a range map ends at rts_cube_attach) / null output", c->cube.range, host_out, capacity_doubles);
}

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
    double* out; RTS_HIP(c->cube.beam.place(device_out, plan.out_doubles, &out));
    // the weights -> pinned staging -> the device, on the stream (n_beams n_rx <= RTS_BEAM_MAX_WEIGHTS: one size for every call)
    RTS_HIP(c->cube.beam_w.upload(p->weights, 2 * (size_t)p->n_beams * q.n_rx, 2u * RTS_BEAM_MAX_WEIGHTS, c->stream));
    if (!device_out) c->cube.beam.record(out, plan.out_doubles);
    return rts_cube_beam_device(c, *p, plan, in, rx_stride, c->cube.beam_w.dev.p, out);
}

extern "C" int rts_cube_beam_get(RtsHandle c, double* host_out, uint64_t capacity_doubles)
{
    CHECK_HANDLE(c);
    return rts_cube_copy_out(c, "rts_cube_beam_get", "no library-owned beams (rts_cube_beamform with device_out NULL; the beams end at rts_cube_attach) / null output", c->cube.beam, host_out, capacity_doubles);
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
    double* out; RTS_HIP(c->cube.cov.place(device_out, plan.out_doubles, &out));
    RTS_HIP(c->cube.d_cov_part.reserve(plan.scratch_bytes / sizeof(double)));
    if (!device_out) { c->cube.cov.record(out, plan.out_doubles); c->cube.cov_n = q.n_rx; }
    return rts_cube_cov_device(c, set, plan, 1u, src, rx_stride, c->cube.d_cov_part.p, out);
}

extern "C" int rts_cube_covariance_get(RtsHandle c, double* host_out, uint64_t capacity_doubles)
{
    CHECK_HANDLE(c);
    return rts_cube_copy_out(c, "rts_cube_covariance_get", "no library-owned covariance (rts_cube_covariance with device_out NULL; a covariance ends at rts_cube_attach) / null output", c->cube.cov, host_out, capacity_doubles);
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
    RTS_TRY(rts_pointer_or_owned("rts_cube_mvdr", p->device_cov, c->cube.cov, c->cube.cov_n, "%s: device_cov is not 16-byte aligned",
                                 "%s: no covariance (rts_cube_covariance with device_out NULL first, or pass device_cov)", "%s: n_rx = %u, the library-owned covariance's %u (or 0)", &cov, &n_rx));
    RtsMvdrPlan plan;
    RTS_TRY(rts_mvdr_check(p, n_rx, "rts_cube_mvdr", &plan));
    if ((uintptr_t)device_out & 15u) { rts_set_error("rts_cube_mvdr: device_out is not 16-byte aligned"); return RTS_ERR_INVALID; }
    if (device_out && rts_bytes_overlap(device_out, sizeof(double) * plan.out_doubles, cov, 16u * (size_t)n_rx * n_rx)) { rts_set_error("rts_cube_mvdr: device_out overlaps the covariance the call reads"); return RTS_ERR_INVALID; }
    CHECK_CLOSED(c);
    double* out; RTS_HIP(c->cube.mvdr.place(device_out, plan.out_doubles, &out));
    RTS_HIP(c->cube.d_mvdr_status.reserve(2));
    // the steering rows -> pinned staging -> the device, on the stream (n_beams n_rx <= RTS_BEAM_MAX_WEIGHTS: one size for every call)
    RTS_HIP(c->cube.mvdr_s.upload(p->steering, plan.out_doubles, 2u * RTS_BEAM_MAX_WEIGHTS, c->stream));
    if (!device_out) c->cube.mvdr.record(out, plan.out_doubles);
    return rts_cube_mvdr_device(c, plan, n_rx, p->n_beams, p->loading, cov, c->cube.mvdr_s.dev.p, c->cube.d_mvdr_status.p + (device_out ? 1 : 0), out);
}

extern "C" int rts_cube_mvdr_get(RtsHandle c, double* host_out, uint64_t capacity_doubles)
{
    CHECK_HANDLE(c);
    const RtsCubeProduct& m = c->cube.mvdr;
    if (!c->cube.set || !m.valid || !host_out) { rts_set_error("rts_cube_mvdr_get: no library-owned weights (rts_cube_mvdr with device_out NULL; the weights end at rts_cube_attach) / null output"); return RTS_ERR_INVALID; }
    if (capacity_doubles < m.doubles) { rts_set_error("rts_cube_mvdr_get: capacity too small"); return RTS_ERR_CAPACITY; }
    uint32_t status = 0;
    RTS_TRY(rts_status_word(c, c->cube.d_mvdr_status.p, &status));
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
    double* out; RTS_HIP(c->cube.cov.place(device_out, plan.out_doubles, &out));
    RTS_HIP(c->cube.d_cov_part.reserve(plan.scratch_bytes / sizeof(double)));
    if (!device_out) { c->cube.cov.record(out, plan.out_doubles); c->cube.cov_n = q.n_rx * p->n_taps; }
    return rts_cube_cov_device(c, set, plan, p->n_taps, src, rx_stride, c->cube.d_cov_part.p, out);
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
    double* out; RTS_HIP(c->cube.st.place(device_out, plan.out_doubles, &out));
    // the weights -> pinned staging -> the device, on the stream (n_filters D <= RTS_BEAM_MAX_WEIGHTS: one size for every call)
    RTS_HIP(c->cube.st_w.upload(p->weights, 2 * (size_t)p->n_filters * plan.D, 2u * RTS_BEAM_MAX_WEIGHTS, c->stream));
    if (!device_out) c->cube.st.record(out, plan.out_doubles);
    return rts_cube_st_apply_device(c, *p, plan, in, rx_stride, c->cube.st_w.dev.p, out);
}

extern "C" int rts_cube_st_get(RtsHandle c, double* host_out, uint64_t capacity_doubles)
{
    CHECK_HANDLE(c);
    return rts_cube_copy_out(c, "rts_cube_st_get", "no library-owned filter output (rts_cube_st_apply with device_out NULL; the output ends at rts_cube_attach) / null output", c->cube.st, host_out, capacity_doubles);
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
    RTS_TRY(rts_pointer_or_owned(who, p->device_cov, c->cube.cov, c->cube.cov_n, "%s: device_cov is not 16-byte aligned",
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
    RTS_HIP(c->cube.eig_val.place(device_values, plan.value_doubles, &values));
    RTS_HIP(c->cube.eig_vec.place(device_vectors, plan.vector_doubles, &vectors));
    RTS_HIP(c->cube.d_eig_status.reserve(2));
    if (!device_values) { c->cube.eig_val.record(values, plan.value_doubles); c->cube.eig_vec.record(vectors, plan.vector_doubles); c->cube.eig_n = n; }
    return rts_cube_eig_device(c, plan, n, cov, c->cube.d_eig_status.p + (device_values ? 1 : 0), values, vectors);
}

extern "C" int rts_cube_eig_get(RtsHandle c, double* values_out, double* vectors_out, uint64_t capacity_values, uint64_t capacity_vector_doubles)
{
    CHECK_HANDLE(c);
    const RtsCubeProduct& v = c->cube.eig_val; const RtsCubeProduct& x = c->cube.eig_vec;
    if (!c->cube.set || !v.valid || !x.valid || (!values_out && !vectors_out)) { rts_set_error("rts_cube_eig_get: no library-owned eigenpairs (rts_cube_eig with both outputs NULL; the eigenpairs end at rts_cube_attach) / null outputs"); return RTS_ERR_INVALID; }
    if ((values_out && capacity_values < v.doubles) || (vectors_out && capacity_vector_doubles < x.doubles)) { rts_set_error("rts_cube_eig_get: capacity too small"); return RTS_ERR_CAPACITY; }
    uint32_t status = 0;
    RTS_TRY(rts_status_word(c, c->cube.d_eig_status.p, &status));
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
    RTS_TRY(rts_pointer_or_owned(who, p->device_vectors, c->cube.eig_vec, c->cube.eig_n, "%s: device_vectors is not 16-byte aligned",
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
    double* out; RTS_HIP(c->cube.doa.place(device_out, plan.out_doubles, &out));
    // g -> pinned staging -> the device, on the stream (m <= RTS_BEAM_MAX_RX: one size for every call)
    RTS_HIP(c->cube.doa_g.upload(p->g, p->m, RTS_BEAM_MAX_RX, c->stream));
    if (!device_out) c->cube.doa.record(out, plan.out_doubles);
    return rts_cube_doa_scan_device(c, plan, n, p->m, p->n_dirs, p->flags, (const double*)p->device_steering, rows, c->cube.doa_g.dev.p, out);
}

extern "C" int rts_cube_doa_get(RtsHandle c, double* host_out, uint64_t capacity_doubles)
{
    CHECK_HANDLE(c);
    return rts_cube_copy_out(c, "rts_cube_doa_get", "no library-owned spectrum (rts_cube_doa_scan with device_out NULL; the spectrum ends at rts_cube_attach) / null output", c->cube.doa, host_out, capacity_doubles);
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

// ------------------------------------------------------------------------------------- backprojection imaging
// (rts_amd.h: RtsImageParams; the arithmetic and the launch plan are rts_image.h, shared by the host export and the kernel, rts_image.hip)
static int rts_image_check(const RtsImageParams* p, const RtsCubeParams& q, const char* who)
{
    if (!p) { rts_set_error("%s: null parameters", who); return RTS_ERR_INVALID; }
    if (p->n_x == 0 || p->n_y == 0 || (uint64_t)p->n_x * p->n_y > RTS_IMAGE_MAX_PIXELS) { rts_set_error("%s: n_x = %u, n_y = %u (each >= 1, n_x * n_y <= %u)", who, p->n_x, p->n_y, RTS_IMAGE_MAX_PIXELS); return RTS_ERR_INVALID; }
    RTS_TRY(rts_taps_check(who, p->taps));
    if (p->flags & ~RTS_IMAGE_ACCUMULATE) { rts_set_error("%s: unknown flags 0x%x", who, p->flags); return RTS_ERR_INVALID; }
    if (p->reserved[0] || p->reserved[1]) { rts_set_error("%s: reserved fields must be 0", who); return RTS_ERR_INVALID; }
    RTS_TRY(rts_pulses_check(who, p->first_pulse, p->n_pulses, q.n_pulses, true));
    if (!std::isfinite(p->cspeed) || !(p->cspeed > 0.0)) { rts_set_error("%s: cspeed = %g (finite, > 0)", who, p->cspeed); return RTS_ERR_INVALID; }
    if (!std::isfinite(p->carrier) || p->carrier < 0.0) { rts_set_error("%s: carrier = %g (finite, >= 0)", who, p->carrier); return RTS_ERR_INVALID; }
    for (int k = 0; k < 3; k++) {
        if (!std::isfinite(p->origin[k])) { rts_set_error("%s: origin[%d] is not finite", who, k); return RTS_ERR_INVALID; }
        if (!std::isfinite(p->step_x[k])) { rts_set_error("%s: step_x[%d] is not finite", who, k); return RTS_ERR_INVALID; }
        if (!std::isfinite(p->step_y[k])) { rts_set_error("%s: step_y[%d] is not finite", who, k); return RTS_ERR_INVALID; }
    }
    if (!p->tx_position) { rts_set_error("%s: null tx_position", who); return RTS_ERR_INVALID; }
    if (!p->rx_position) { rts_set_error("%s: null rx_position", who); return RTS_ERR_INVALID; }
    for (size_t i = 0; i < 3 * (size_t)p->n_pulses; i++) if (!std::isfinite(p->tx_position[i])) { rts_set_error("%s: tx_position of pulse %zu is not finite", who, i / 3); return RTS_ERR_INVALID; }
    for (size_t i = 0; i < 3 * (size_t)q.n_rx * p->n_pulses; i++) if (!std::isfinite(p->rx_position[i])) { rts_set_error("%s: rx_position of receiver %zu, pulse %zu is not finite", who, i / 3 / p->n_pulses, i / 3 % p->n_pulses); return RTS_ERR_INVALID; }
    if (p->pulse_weight) for (uint32_t j = 0; j < p->n_pulses; j++) if (!std::isfinite(p->pulse_weight[j])) { rts_set_error("%s: pulse_weight[%u] is not finite", who, j); return RTS_ERR_INVALID; }
    if (!rts_image_plan(p->n_x, p->n_y, q.n_rx, p->n_pulses, 0u).supported) { rts_set_error("%s: n_rx = %u receivers / n_pulses = %u: more than %u receivers or chunks of %u pulses", who, q.n_rx, p->n_pulses, RTS_IMAGE_GRID_MAX, RTS_IMAGE_PULSE_CHUNK); return RTS_ERR_INVALID; }
    return RTS_OK;
}

extern "C" int rts_backproject_eval(const RtsCubeParams* q, const double* cube, const RtsImageParams* p, double* out)
{
    RTS_TRY(rts_eval_cube_check("rts_backproject_eval", q, true, true));
    RTS_TRY(rts_image_check(p, *q, "rts_backproject_eval"));
    if (!cube || !out) { rts_set_error("rts_backproject_eval: null cube or output array"); return RTS_ERR_INVALID; }
    rts_image_eval_host(q, cube, p, out);
    return RTS_OK;
}

extern "C" int rts_cube_backproject(RtsHandle c, const RtsImageParams* p, void* device_out)
{
    CHECK_HANDLE(c);
    NEED_CUBE(c, "rts_cube_backproject", "no cube (call rts_cube_attach first)");
    const RtsCubeParams& q = c->cube.params;
    RTS_TRY(rts_image_check(p, q, "rts_cube_backproject"));
    if ((uintptr_t)device_out & 15u) { rts_set_error("rts_cube_backproject: device_out is not 16-byte aligned"); return RTS_ERR_INVALID; }
    if ((p->flags & RTS_IMAGE_ACCUMULATE) && !device_out && !(c->cube.image.valid && c->cube.img_nx == p->n_x && c->cube.img_ny == p->n_y)) {
        rts_set_error("rts_cube_backproject: RTS_IMAGE_ACCUMULATE without device_out needs a library-owned image of the same n_x, n_y"); return RTS_ERR_INVALID; }
    CHECK_CLOSED(c);
    const RtsImagePlan plan = rts_image_plan(p->n_x, p->n_y, q.n_rx, p->n_pulses, c->tune.img_split_below);
    const size_t doubles = 2 * (size_t)q.n_rx * p->n_y * p->n_x;
    double* out; RTS_HIP(c->cube.image.place(device_out, doubles, &out));       // (accumulate: the shape is the same, so the buffer stays)
    // the geometry [tx | rx | w] -> pinned staging -> the device, on the stream
    const size_t P = p->n_pulses, n_geo = 3 * P + 3 * (size_t)q.n_rx * P + P;
    double* g = nullptr;
    RTS_HIP(c->cube.img_geo.begin(n_geo, std::max<size_t>(n_geo + n_geo / 2, 4096), n_geo, &g));
    memcpy(g, p->tx_position, sizeof(double) * 3 * P);
    memcpy(g + 3 * P, p->rx_position, sizeof(double) * 3 * q.n_rx * P);
    for (size_t j = 0; j < P; j++) g[3 * P + 3 * (size_t)q.n_rx * P + j] = p->pulse_weight ? p->pulse_weight[j] : 1.0;
    RTS_HIP(c->cube.img_geo.send(n_geo, c->stream));
    if (!device_out) { c->cube.image.record(out, doubles); c->cube.img_nx = p->n_x; c->cube.img_ny = p->n_y; }
    return rts_cube_backproject_device(c, *p, plan, c->cube.img_geo.dev.p, out);
}

extern "C" int rts_cube_image_get(RtsHandle c, double* host_out, uint64_t capacity_doubles)
{
    CHECK_HANDLE(c);
    return rts_cube_copy_out(c, "rts_cube_image_get", "no library-owned image (rts_cube_backproject with device_out NULL; an image ends at rts_cube_attach) / null output", c->cube.image, host_out, capacity_doubles);
}
