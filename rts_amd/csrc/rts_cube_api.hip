// rts_cube_api.hip -- the cube part of the C-ABI of include/rts_amd.h, first of three host units: the cube and the signal in it -- attach, accumulate,
// Doppler and get; waveform, render, compress; the MIMO matched-filter bank; passive cancellation and cross-correlation; noise; clutter and jammer sources; spectrogram; autofocus; FMCW; backprojection -- and the pure-host evaluators
// that go with them (rts_cube_reduce apart: rts_api.hip; the detection chain: rts_cube_detect_api.hip; the receive array: rts_cube_array_api.hip).
// Host code only, no kernels: argument checks, the handle's cube state (RtsCubeState, rts_cube_state.h), the calls of the launchers in the kernels' units.
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
    double* out; RTS_HIP(c->cube.doppler.map.place(device_out, doubles, &out));
    c->cube.doppler.map.record(out, doubles); c->cube.doppler.n_fft = n_fft;       // (also when caller-owned: rts_cube_detect without a map takes it)
    return rts_cube_doppler_device(c, n_fft, out);
}

extern "C" int rts_cube_doppler_get(RtsHandle c, double* host_out, uint64_t capacity_doubles)
{
    CHECK_HANDLE(c);
    CHECK_CLOSED(c);
    return rts_cube_copy_out(c, "rts_cube_doppler_get", "no transform (rts_cube_doppler) / null output", c->cube.doppler.map, host_out, capacity_doubles);
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
    RTS_HIP(c->cube.wave.d.reserve(2 * (size_t)w->n_samples));
    RTS_HIP(hipMemcpy(c->cube.wave.d.p, w->samples, sizeof(double) * 2 * w->n_samples, hipMemcpyHostToDevice));
    c->cube.wave.M = w->n_samples; c->cube.wave.L = w->taps; c->cube.wave.set = true;
    return RTS_OK;
}

extern "C" int rts_cube_render(RtsHandle c, uint32_t pulse_index, uint32_t source, uint32_t flags, double cspeed, double carrier)
{
    CHECK_HANDLE(c);
    RTS_TRY(rts_render_source_check("rts_cube_render", source, flags));
    CHECK_CLOSED(c);
    NEED_CUBE(c, "rts_cube_render", "call rts_cube_attach first");
    if (!c->cube.wave.set) { rts_set_error("rts_cube_render: no waveform (rts_cube_set_waveform)"); return RTS_ERR_INVALID; }
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
    if (!c->cube.wave.set) { rts_set_error("rts_cube_compress: no waveform (rts_cube_set_waveform)"); return RTS_ERR_INVALID; }
    const RtsCubeParams& q = c->cube.params;
    RTS_TRY(rts_pulses_check("rts_cube_compress", first_pulse, n_pulses, q.n_pulses, false));
    if (q.n_bins > RTS_COMPRESS_MAX_BINS) { rts_set_error("rts_cube_compress: %u range bins > %u (RTS_COMPRESS_MAX_BINS: one row of complex128 in a workgroup's LDS)", q.n_bins, RTS_COMPRESS_MAX_BINS); return RTS_ERR_INVALID; }
    return rts_cube_compress_device(c, first_pulse, n_pulses);
}

// ------------------------------------------------------------------------------------- MIMO radar: the matched-filter bank
// (rts_amd.h: RtsBankParams; the rule, the plan and the host evaluator are rts_mimo.h, shared with the kernel, rts_mimo.hip; each
// waveform passes rts_waveform_check, the one statement of the RtsWaveform rule)
static int rts_bank_check(const RtsBankParams* p, const RtsCubeParams& q, const char* who, uint32_t* M, RtsBankPlan* plan)
{
    if (!p) { rts_set_error("%s: null parameters", who); return RTS_ERR_INVALID; }
    const int rule = rts_bank_rule(p, q.n_pulses);
    if (rule == 1) { rts_set_error("%s: reserved fields must be 0", who); return RTS_ERR_INVALID; }
    if (rule == 2) { rts_set_error("%s: n_waves = %u (1 .. %u, RTS_BANK_MAX_WAVES)", who, p->n_waves, RTS_BANK_MAX_WAVES); return RTS_ERR_INVALID; }
    if (rule == 3) { rts_set_error("%s: null waves", who); return RTS_ERR_INVALID; }
    for (uint32_t t = 0; t < p->n_waves; t++) {
        char name[64]; snprintf(name, sizeof(name), "%s: waves[%u]", who, t);
        RTS_TRY(rts_waveform_check(&p->waves[t], name));
        M[t] = p->waves[t].n_samples;
    }
    if (rule == 4) return rts_pulses_check(who, p->first_pulse, p->n_pulses, q.n_pulses, true);
    const int64_t bad = rts_bank_code_bad(p->code, p->n_waves, p->n_pulses);
    if (bad >= 0) { rts_set_error("%s: code[%u][%u] is not finite", who, (uint32_t)(bad / 2 / p->n_pulses), (uint32_t)(bad / 2 % p->n_pulses)); return RTS_ERR_INVALID; }
    *plan = rts_bank_plan(q.n_rx, p->n_pulses, q.n_bins, p->n_waves, M, p->code != nullptr);
    if (!plan->supported) {
        rts_set_error("%s: an output of %u waveforms x %u receivers x %u rows x %u bins: more than %llu cells (RTS_BANK_MAX_CELLS) or than %u workgroups", who, p->n_waves, q.n_rx, p->n_pulses,
                      q.n_bins, (unsigned long long)RTS_BANK_MAX_CELLS, RTS_MIMO_MAX_GRID);
        return RTS_ERR_INVALID;
    }
    return RTS_OK;
}

extern "C" int rts_bank_eval(const RtsCubeParams* q, const double* cube, const RtsBankParams* p, double* out)
{
    const char* who = "rts_bank_eval";
    RTS_TRY(rts_eval_cube_check(who, q, true, false));
    uint32_t M[RTS_BANK_MAX_WAVES]; RtsBankPlan plan;
    RTS_TRY(rts_bank_check(p, *q, who, M, &plan));
    if (!cube || !out) { rts_set_error("%s: null cube or output array", who); return RTS_ERR_INVALID; }
    rts_bank_eval_host(q, cube, p, out);
    return RTS_OK;
}

extern "C" int rts_cube_bank(RtsHandle c, const RtsBankParams* p, void* device_out)
{
    const char* who = "rts_cube_bank";
    CHECK_HANDLE(c);
    NEED_CUBE(c, who, "no cube (call rts_cube_attach first)");
    const RtsCubeParams& q = c->cube.params;
    uint32_t M[RTS_BANK_MAX_WAVES]; RtsBankPlan plan;
    RTS_TRY(rts_bank_check(p, q, who, M, &plan));
    if ((uintptr_t)device_out & 15u) { rts_set_error("%s: device_out is not 16-byte aligned", who); return RTS_ERR_INVALID; }
    if ((uintptr_t)c->cube.p & 15u) { rts_set_error("%s: the cube's device memory is not 16-byte aligned", who); return RTS_ERR_INVALID; }
    RTS_TRY(rts_output_apart_check(who, "%s: device_out overlaps receiver %u of the cube: the bank is not in place", device_out, plan.out_doubles, c->cube.p, (uint64_t)q.n_pulses * q.n_bins,
                                   (uint64_t)p->first_pulse * q.n_bins, (uint64_t)(p->first_pulse + p->n_pulses) * q.n_bins, q.n_rx));
    CHECK_CLOSED(c);
    RtsMimoState& s = c->cube.mimo;
    double* out; RTS_HIP(s.out.place(device_out, plan.out_doubles, &out));
    // the waveforms' samples and the code table -> pinned staging -> the device, on the stream; a smaller set reuses both blocks
    double* h = nullptr;
    RTS_HIP(s.tab.begin(plan.tab_doubles, plan.tab_doubles, plan.tab_doubles, &h));
    for (uint32_t t = 0; t < p->n_waves; t++) memcpy(h + plan.off[t], p->waves[t].samples, sizeof(double) * 2 * M[t]);
    if (p->code) memcpy(h + plan.code_off, p->code, sizeof(double) * 2 * (size_t)p->n_waves * p->n_pulses);
    RTS_HIP(s.tab.send(plan.tab_doubles, c->stream));
    RTS_TRY(rts_cube_bank_device(c, *p, plan, M, s.tab.dev.p, p->code != nullptr, out));
    if (!device_out) s.out.record(out, plan.out_doubles);      // (once the launch is enqueued: a failed one leaves no product over unwritten memory)
    return RTS_OK;
}

extern "C" int rts_cube_bank_get(RtsHandle c, double* host_out, uint64_t capacity_doubles)
{
    CHECK_HANDLE(c);
    return rts_cube_copy_out(c, "rts_cube_bank_get", "no library-owned bank output (rts_cube_bank with device_out NULL; it ends at rts_cube_attach) / null output", c->cube.mimo.out, host_out, capacity_doubles);
}

// ------------------------------------------------------------------------------------- passive radar: reference-channel cancellation, cross-correlation
// (rts_amd.h: RtsCancelParams, RtsXcorrParams; the rules, the plans and the host evaluators are rts_passive.h, shared with the kernels, rts_passive.hip)
static int rts_cancel_check(const RtsCancelParams* p, const RtsCubeParams& q, const char* who, RtsCancelPlan* plan)
{
    if (!p) { rts_set_error("%s: null parameters", who); return RTS_ERR_INVALID; }
    switch (rts_cancel_rule(p, q.n_rx, q.n_pulses)) {
        case 0: break;
        case 1: rts_set_error("%s: reserved fields must be 0", who); return RTS_ERR_INVALID;
        case 2: rts_set_error("%s: n_rx = %u receivers: more than %u (RTS_PASSIVE_MAX_RX: the bits of rx_mask)", who, q.n_rx, RTS_PASSIVE_MAX_RX); return RTS_ERR_INVALID;
        case 3: rts_set_error("%s: ref_rx = %u >= the cube's %u receivers", who, p->ref_rx, q.n_rx); return RTS_ERR_INVALID;
        case 4: rts_set_error("%s: n_taps = %u (1 .. %u, RTS_PASSIVE_MAX_TAPS)", who, p->n_taps, RTS_PASSIVE_MAX_TAPS); return RTS_ERR_INVALID;
        case 5: return rts_pulses_check(who, p->first_pulse, p->n_pulses, q.n_pulses, true);
        case 6: rts_set_error("%s: loading = %g (finite, >= 0)", who, p->loading); return RTS_ERR_INVALID;
        case 7: rts_set_error("%s: rx_mask = 0x%llx names ref_rx = %u (the reference rows are never written)", who, (unsigned long long)p->rx_mask, p->ref_rx); return RTS_ERR_INVALID;
        case 8: rts_set_error("%s: rx_mask = 0x%llx names a receiver beyond the cube's %u", who, (unsigned long long)p->rx_mask, q.n_rx); return RTS_ERR_INVALID;
        default: rts_set_error("%s: n_pulses = %u in blocks of rows_per_block = %u: more than %u blocks (RTS_PASSIVE_MAX_BLOCKS)", who, p->n_pulses, p->rows_per_block, RTS_PASSIVE_MAX_BLOCKS); return RTS_ERR_INVALID;
    }
    *plan = rts_cancel_plan(q.n_rx, q.n_bins, p->n_pulses, p->rows_per_block, p->n_taps);
    if (!plan->supported) { rts_set_error("%s: a cube of %u receivers x %u bins with %u taps has no launch plan", who, q.n_rx, q.n_bins, p->n_taps); return RTS_ERR_INVALID; }
    return RTS_OK;
}

static int rts_xcorr_check(const RtsXcorrParams* p, const RtsCubeParams& q, const char* who, RtsXcorrPlan* plan)
{
    if (!p) { rts_set_error("%s: null parameters", who); return RTS_ERR_INVALID; }
    switch (rts_xcorr_rule(p, q.n_rx, q.n_pulses, q.n_bins)) {
        case 0: break;
        case 1: rts_set_error("%s: reserved fields must be 0", who); return RTS_ERR_INVALID;
        case 2: rts_set_error("%s: ref_rx = %u >= the cube's %u receivers", who, p->ref_rx, q.n_rx); return RTS_ERR_INVALID;
        case 3: return rts_pulses_check(who, p->first_pulse, p->n_pulses, q.n_pulses, true);
        case 4: rts_set_error("%s: n_lags = %u (1 .. %u, RTS_XCORR_MAX_LAGS)", who, p->n_lags, RTS_XCORR_MAX_LAGS); return RTS_ERR_INVALID;
        case 5: rts_set_error("%s: first_lag = %u (0 .. %u, RTS_XCORR_MAX_FIRST_LAG)", who, p->first_lag, RTS_XCORR_MAX_FIRST_LAG); return RTS_ERR_INVALID;
        case 6: rts_set_error("%s: %u range bins > %u (RTS_COMPRESS_MAX_BINS)", who, q.n_bins, RTS_COMPRESS_MAX_BINS); return RTS_ERR_INVALID;
        default: rts_set_error("%s: n_rx = %u receivers x n_pulses = %u rows: more than 65535 of either (the launch grid)", who, q.n_rx, p->n_pulses); return RTS_ERR_INVALID;
    }
    *plan = rts_xcorr_plan(q.n_rx, p->n_pulses, p->n_lags);
    if (!plan->supported) { rts_set_error("%s: %u receivers x %u rows x %u lags have no launch plan", who, q.n_rx, p->n_pulses, p->n_lags); return RTS_ERR_INVALID; }
    return RTS_OK;
}

extern "C" int rts_cancel_eval(const RtsCubeParams* q, double* cube_inout, const RtsCancelParams* p, double* coeffs_out, uint32_t* n_blocks_out, uint32_t* n_failed_out)
{
    const char* who = "rts_cancel_eval";
    RTS_TRY(rts_eval_cube_check(who, q, true, false));
    RtsCancelPlan plan;
    RTS_TRY(rts_cancel_check(p, *q, who, &plan));
    if (!cube_inout) { rts_set_error("%s: null cube", who); return RTS_ERR_INVALID; }
    std::vector<double> work(rts_cancel_work_doubles(plan.K));
    uint32_t failed = 0;
    rts_cancel_eval_host(q, cube_inout, p, plan, coeffs_out, &failed, work.data());
    if (n_blocks_out) *n_blocks_out = plan.n_blocks;
    if (n_failed_out) *n_failed_out = failed;
    return RTS_OK;
}

extern "C" int rts_xcorr_eval(const RtsCubeParams* q, const double* cube, const RtsXcorrParams* p, double* out)
{
    const char* who = "rts_xcorr_eval";
    RTS_TRY(rts_eval_cube_check(who, q, true, false));
    RtsXcorrPlan plan;
    RTS_TRY(rts_xcorr_check(p, *q, who, &plan));
    if (!cube || !out) { rts_set_error("%s: null cube or output array", who); return RTS_ERR_INVALID; }
    rts_xcorr_eval_host(q, cube, p, out);
    return RTS_OK;
}

extern "C" int rts_cube_cancel(RtsHandle c, const RtsCancelParams* p)
{
    const char* who = "rts_cube_cancel";
    CHECK_HANDLE(c);
    NEED_CUBE(c, who, "no cube (call rts_cube_attach first)");
    const RtsCubeParams& q = c->cube.params;
    RtsCancelPlan plan;
    RTS_TRY(rts_cancel_check(p, q, who, &plan));
    if ((uintptr_t)c->cube.p & 15u) { rts_set_error("%s: the cube's device memory is not 16-byte aligned", who); return RTS_ERR_INVALID; }
    CHECK_CLOSED(c);
    RtsPassiveState& s = c->cube.passive;
    // (mask, loading and shape are all the kernels read beside the cube: they travel as launch arguments, so this family has no staged upload)
    s.cancel_valid = false;                                    // a regrow frees what the record names; it is valid again once the launches are enqueued
    RTS_HIP(s.d_part.reserve(plan.scratch_doubles));
    RTS_HIP(s.d_sums.reserve(plan.sums_doubles));
    RTS_HIP(s.d_coeff.reserve(plan.coeff_doubles));
    RTS_HIP(s.d_fail.reserve(plan.n_blocks));
    RTS_TRY(rts_cube_cancel_device(c, *p, plan, rts_passive_mask(p->rx_mask, p->ref_rx, q.n_rx)));
    s.n_blocks = plan.n_blocks; s.n_taps = plan.K; s.n_rx = q.n_rx; s.cancel_valid = true;
    return RTS_OK;
}

extern "C" int rts_cube_cancel_info(RtsHandle c, uint32_t* n_blocks_out, uint32_t* n_failed_out)
{
    const char* who = "rts_cube_cancel_info";
    CHECK_HANDLE(c);
    const RtsPassiveState& s = c->cube.passive;
    if (!c->cube.set || !s.cancel_valid) { rts_set_error("%s: no cancellation (rts_cube_cancel; its record ends at rts_cube_attach)", who); return RTS_ERR_INVALID; }
    if (!n_blocks_out && !n_failed_out) { rts_set_error("%s: null outputs", who); return RTS_ERR_INVALID; }
    if (n_failed_out) {
        std::vector<uint32_t> fail(s.n_blocks);
        RTS_HIP(hipStreamSynchronize(c->stream));
        RTS_HIP(hipMemcpy(fail.data(), s.d_fail.p, sizeof(uint32_t) * s.n_blocks, hipMemcpyDeviceToHost));
        uint32_t n = 0; for (uint32_t f : fail) n += f != 0u;
        *n_failed_out = n;
    }
    if (n_blocks_out) *n_blocks_out = s.n_blocks;
    return RTS_OK;
}

extern "C" int rts_cube_cancel_coeffs_get(RtsHandle c, double* host_out, uint64_t capacity_doubles)
{
    CHECK_HANDLE(c);
    const RtsPassiveState& s = c->cube.passive;
    return rts_cube_copy_out(c, "rts_cube_cancel_coeffs_get", "no cancellation (rts_cube_cancel; its coefficients end at rts_cube_attach) / null output", s.cancel_valid, s.d_coeff.p,
                             2 * (size_t)s.n_rx * s.n_blocks * s.n_taps, host_out, capacity_doubles);
}

extern "C" int rts_cube_xcorr(RtsHandle c, const RtsXcorrParams* p, void* device_out)
{
    const char* who = "rts_cube_xcorr";
    CHECK_HANDLE(c);
    NEED_CUBE(c, who, "no cube (call rts_cube_attach first)");
    const RtsCubeParams& q = c->cube.params;
    RtsXcorrPlan plan;
    RTS_TRY(rts_xcorr_check(p, q, who, &plan));
    if ((uintptr_t)device_out & 15u) { rts_set_error("%s: device_out is not 16-byte aligned", who); return RTS_ERR_INVALID; }
    if ((uintptr_t)c->cube.p & 15u) { rts_set_error("%s: the cube's device memory is not 16-byte aligned", who); return RTS_ERR_INVALID; }
    const uint64_t rx_stride = (uint64_t)q.n_pulses * q.n_bins;
    RTS_TRY(rts_output_apart_check(who, "%s: device_out overlaps receiver %u of the cube: the correlation is not in place", device_out, plan.out_doubles, c->cube.p, rx_stride,
                                   (uint64_t)p->first_pulse * q.n_bins, (uint64_t)(p->first_pulse + p->n_pulses) * q.n_bins, q.n_rx));
    CHECK_CLOSED(c);
    double* out; RTS_HIP(c->cube.passive.xcorr.place(device_out, plan.out_doubles, &out));
    RTS_TRY(rts_cube_xcorr_device(c, *p, plan, out));
    if (!device_out) c->cube.passive.xcorr.record(out, plan.out_doubles);      // (once the launch is enqueued: a failed one leaves no product over unwritten memory)
    return RTS_OK;
}

extern "C" int rts_cube_xcorr_get(RtsHandle c, double* host_out, uint64_t capacity_doubles)
{
    CHECK_HANDLE(c);
    return rts_cube_copy_out(c, "rts_cube_xcorr_get", "no library-owned correlation (rts_cube_xcorr with device_out NULL; a correlation ends at rts_cube_attach) / null output", c->cube.passive.xcorr, host_out, capacity_doubles);
}

// ------------------------------------------------------------------------------------- receiver noise
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
    RTS_HIP(c->cube.source.tab.begin(plan.table_doubles, most, most, &tab));
    rts_src_table(p, q.n_rx, q.n_bins, tab);
    RTS_HIP(c->cube.source.tab.send(plan.table_doubles, c->stream));
    return rts_cube_sources_device(c, plan, p->n_patches, p->range_profile != nullptr, p->seed, live, c->cube.source.tab.dev.p);
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
    double* out; RTS_HIP(c->cube.stft.out.place(device_out, plan.out_doubles, &out));
    // the window -> pinned staging -> the device, on the stream (window_len <= RTS_STFT_MAX_FFT: one size for every call)
    const double* win = nullptr;
    if (p->window) {
        RTS_HIP(c->cube.stft.win.upload(p->window, p->window_len, RTS_STFT_MAX_FFT, c->stream));
        win = c->cube.stft.win.dev.p;
    }
    if (!device_out) c->cube.stft.out.record(out, plan.out_doubles);
    if (n_frames_out) *n_frames_out = plan.n_frames;
    return rts_cube_stft_device(c, *p, plan, win, out);
}

extern "C" int rts_cube_spectrogram_get(RtsHandle c, double* host_out, uint64_t capacity_doubles)
{
    CHECK_HANDLE(c);
    return rts_cube_copy_out(c, "rts_cube_spectrogram_get", "no library-owned spectrogram (rts_cube_spectrogram with device_out NULL; a spectrogram ends at rts_cube_attach) / null output", c->cube.stft.out, host_out, capacity_doubles);
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
    double* out; RTS_HIP(c->cube.focus.align.place(device_out, plan.out_doubles, &out));
    if (!device_out) { c->cube.focus.align.record(out, plan.out_doubles); c->cube.focus.align_first = p->first_pulse; c->cube.focus.align_P = p->n_pulses; }
    return rts_cube_align_device(c, *p, plan, out);
}

extern "C" int rts_cube_align_get(RtsHandle c, double* host_out, uint64_t capacity_doubles)
{
    CHECK_HANDLE(c);
    return rts_cube_copy_out(c, "rts_cube_align_get", "no library-owned shift table (rts_cube_align with device_out NULL; a table ends at rts_cube_attach) / null output", c->cube.focus.align, host_out, capacity_doubles);
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
    double* out; RTS_HIP(c->cube.focus.pga.place(device_out, plan.out_doubles, &out));
    if (!device_out) { c->cube.focus.pga.record(out, plan.out_doubles); c->cube.focus.pga_first = p->first_pulse; c->cube.focus.pga_P = p->n_pulses; c->cube.focus.pga_iters = p->n_iters; }
    return rts_cube_pga_device(c, *p, plan, out);
}

extern "C" int rts_cube_pga_get(RtsHandle c, double* phase_out, double* rms_out, uint64_t capacity_phase, uint64_t capacity_rms)
{
    const char* who = "rts_cube_pga_get";
    CHECK_HANDLE(c);
    const RtsCubeState& s = c->cube;
    if (!s.set || !s.focus.pga.valid) { rts_set_error("%s: no library-owned phase table (rts_cube_pga with device_out NULL; a table ends at rts_cube_attach)", who); return RTS_ERR_INVALID; }
    if (!phase_out && !rms_out) { rts_set_error("%s: null outputs", who); return RTS_ERR_INVALID; }
    const size_t n_phase = (size_t)s.params.n_rx * s.focus.pga_P, n_rms = (size_t)s.params.n_rx * s.focus.pga_iters;
    if ((phase_out && capacity_phase < n_phase) || (rms_out && capacity_rms < n_rms)) { rts_set_error("%s: capacity too small", who); return RTS_ERR_CAPACITY; }
    RTS_HIP(hipStreamSynchronize(c->stream));
    if (phase_out) RTS_HIP(hipMemcpy(phase_out, s.focus.pga.p, sizeof(double) * n_phase, hipMemcpyDeviceToHost));
    if (rms_out) RTS_HIP(hipMemcpy(rms_out, s.focus.pga.p + n_phase, sizeof(double) * n_rms, hipMemcpyDeviceToHost));
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
        if (!s.focus.align.valid || s.focus.align_first != p->first_pulse || s.focus.align_P != p->n_pulses) { rts_set_error("%s: RTS_CORRECT_USE_ALIGN: no library-owned shift table of rows %u .. %u + %u (rts_cube_align with device_out NULL)", who, p->first_pulse, p->first_pulse, p->n_pulses); return RTS_ERR_INVALID; }
        shifts = s.focus.align.p;
    }
    if (p->flags & RTS_CORRECT_USE_PGA) {
        if (!s.focus.pga.valid || s.focus.pga_first != p->first_pulse || s.focus.pga_P != p->n_pulses) { rts_set_error("%s: RTS_CORRECT_USE_PGA: no library-owned phase table of rows %u .. %u + %u (rts_cube_pga with device_out NULL)", who, p->first_pulse, p->first_pulse, p->n_pulses); return RTS_ERR_INVALID; }
        phase = s.focus.pga.p;
    }
    CHECK_CLOSED(c);
    // the host tables -> pinned staging -> the device, on the stream
    if (plan.table_doubles) {
        double* h = nullptr;
        RTS_HIP(s.focus.tab.begin(plan.table_doubles, plan.table_doubles, plan.table_doubles, &h));
        const size_t n = (size_t)s.params.n_rx * p->n_pulses;
        size_t at = 0;
        if (p->shifts) { memcpy(h, p->shifts, sizeof(double) * n); at = n; }
        if (p->phase) memcpy(h + at, p->phase, sizeof(double) * n);
        RTS_HIP(s.focus.tab.send(plan.table_doubles, c->stream));
        if (p->shifts) shifts = s.focus.tab.dev.p;
        if (p->phase) phase = s.focus.tab.dev.p + at;
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
    double* out; RTS_HIP(c->cube.fmcw.range.place(device_out, plan.out_doubles, &out));
    // the window -> pinned staging -> the device, on the stream (n_samples <= RTS_RANGE_MAX_FFT: one size for every call)
    const double* win = nullptr;
    if (p->window) {
        RTS_HIP(c->cube.fmcw.range_win.upload(p->window, plan.n_samples, RTS_RANGE_MAX_FFT, c->stream));
        win = c->cube.fmcw.range_win.dev.p;
    }
    if (!device_out) c->cube.fmcw.range.record(out, plan.out_doubles);
    return rts_cube_range_device(c, *p, plan, win, out);
}

extern "C" int rts_cube_range_get(RtsHandle c, double* host_out, uint64_t capacity_doubles)
{
    CHECK_HANDLE(c);
    return rts_cube_copy_out(c, "rts_cube_range_get", "no library-owned range map (rts_cube_range_transform with device_out NULL; a range map ends at rts_cube_attach) / null output", c->cube.fmcw.range, host_out, capacity_doubles);
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
    if ((p->flags & RTS_IMAGE_ACCUMULATE) && !device_out && !(c->cube.image.out.valid && c->cube.image.nx == p->n_x && c->cube.image.ny == p->n_y)) {
        rts_set_error("rts_cube_backproject: RTS_IMAGE_ACCUMULATE without device_out needs a library-owned image of the same n_x, n_y"); return RTS_ERR_INVALID; }
    CHECK_CLOSED(c);
    const RtsImagePlan plan = rts_image_plan(p->n_x, p->n_y, q.n_rx, p->n_pulses, c->tune.img_split_below);
    const size_t doubles = 2 * (size_t)q.n_rx * p->n_y * p->n_x;
    double* out; RTS_HIP(c->cube.image.out.place(device_out, doubles, &out));       // (accumulate: the shape is the same, so the buffer stays)
    // the geometry [tx | rx | w] -> pinned staging -> the device, on the stream
    const size_t P = p->n_pulses, n_geo = 3 * P + 3 * (size_t)q.n_rx * P + P;
    double* g = nullptr;
    RTS_HIP(c->cube.image.geo.begin(n_geo, std::max<size_t>(n_geo + n_geo / 2, 4096), n_geo, &g));
    memcpy(g, p->tx_position, sizeof(double) * 3 * P);
    memcpy(g + 3 * P, p->rx_position, sizeof(double) * 3 * q.n_rx * P);
    for (size_t j = 0; j < P; j++) g[3 * P + 3 * (size_t)q.n_rx * P + j] = p->pulse_weight ? p->pulse_weight[j] : 1.0;
    RTS_HIP(c->cube.image.geo.send(n_geo, c->stream));
    if (!device_out) { c->cube.image.out.record(out, doubles); c->cube.image.nx = p->n_x; c->cube.image.ny = p->n_y; }
    return rts_cube_backproject_device(c, *p, plan, c->cube.image.geo.dev.p, out);
}

extern "C" int rts_cube_image_get(RtsHandle c, double* host_out, uint64_t capacity_doubles)
{
    CHECK_HANDLE(c);
    return rts_cube_copy_out(c, "rts_cube_image_get", "no library-owned image (rts_cube_backproject with device_out NULL; an image ends at rts_cube_attach) / null output", c->cube.image.out, host_out, capacity_doubles);
}
