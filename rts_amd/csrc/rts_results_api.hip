// rts_results_api.hip -- what a pulse left, handed to the caller (C-ABI of include/rts_amd.h): its statistics, its received set and its aggregation.  Host code only, no
// kernels: every call settles the handle's pulse (CHECK_CLOSED), then reads the handle's record of results (RtsPulseResults, rts_internal.h) and its device buffers.
#include <cstring>
#include "rts_internal.h"

// n elements at src -> the caller's array, if the caller gave one
template <class T> static hipError_t rts_copy_home(T* dst, const T* src, size_t n) { return dst && n ? hipMemcpy(dst, src, sizeof(T) * n, hipMemcpyDeviceToHost) : hipSuccess; }

// The views' fall-back (no mirror of this set: not asked for, or larger than the mirror): n elements at src -> storage the handle keeps, *out
// pointing at it.  bit != 0: the array is read from the device ONCE per pulse (v_recv_have): pointers handed out earlier stay valid and keep their
// content -- the records as they were at the pulse's first call, i.e. AS RECEIVED when that call came before rts_finalise_values (a second
// call used to re-read records the finalisation had changed, and rts_aggregated_view's fallback overwrote them with group values).  bit 0: every call.
template <class T> static hipError_t rts_view_fill(RtsPulseResults& r, unsigned bit, std::vector<T>& v, const T* src, size_t n, const T** out)
{
    if (!(r.v_recv_have & bit)) { v.resize(n); const hipError_t e = hipMemcpy(v.data(), src, sizeof(T) * n, hipMemcpyDeviceToHost); if (e != hipSuccess) return e; r.v_recv_have |= bit; }
    if (out) *out = v.data();
    return hipSuccess;
}

extern "C" int rts_get_stats(RtsHandle c, RtsStats* out)
{
    if (!c || !out) { rts_set_error("rts_get_stats: null argument"); return RTS_ERR_INVALID; }
    CHECK_CLOSED(c);
    if (c->stats_pending) {                          // stage timers are resolved lazily: reading them drains the stream
        RTS_HIP(hipSetDevice(c->device));
        RTS_HIP(hipStreamSynchronize(c->stream));
        RtsStats& s = c->stats; float ms = 0;
        RTS_HIP(hipEventElapsedTime(&s.ms_scene, c->ev[0], c->ev[1]));
        RTS_HIP(hipEventElapsedTime(&s.ms_trace, c->ev[2], c->ev[3]));
        RTS_HIP(hipEventElapsedTime(&s.ms_compact, c->ev[4], c->ev[5]));
        s.ms_aggregate = 0;
        if (c->res.fin_timed || c->res.agg_timed) { RTS_HIP(hipEventElapsedTime(&ms, c->ev[6], c->ev[7])); s.ms_aggregate = ms; }
        c->stats_pending = false;
    }
    *out = c->stats; return RTS_OK;
}

// When the persistent blocks of the handle's last launch started and ended (a handle created with RTS_TIMELINE_BLOCKS=1; product builds): out[0..2] first / median / last
// block START, out[3..7] first / 10th percentile / median / 90th percentile / last block END, all in microseconds after the first start (the 100 MHz counter), out[8] the blocks.
// A launch is a BULK -- every block resident; the median end -- and a tail of the few tiles that are one ray's long chain of dependent steps.
// The summary comes home with the launch's counters, however the pulse was ended (rts_api.hip: rts_pulse_home).
extern "C" int rts_get_block_timeline(RtsHandle c, double* out, uint32_t n)
{
    if (!c || !out) { rts_set_error("rts_get_block_timeline: null argument"); return RTS_ERR_INVALID; }
    CHECK_CLOSED(c);
    if (!c->tune.timeline_blocks || c->tl_summary[8] == 0.0) { rts_set_error("rts_get_block_timeline: the handle records no block timeline (create it with RTS_TIMELINE_BLOCKS=1, product build) or has not traced yet"); return RTS_ERR_INVALID; }
    for (uint32_t k = 0; k < n && k < 9; k++) out[k] = c->tl_summary[k];
    return RTS_OK;
}

// Lane statistics of the last launch's walk (RTS_FLAG_COUNT_TRAVERSAL builds; zeros otherwise): out[0] lane-steps ISSUED (64 x the
// longest walk of every bounce round of every tile), out[1] of them issued to lanes that were in the round at all, out[2]
// walk steps actually taken.  1 - out[1]/out[0]: what lanes that left their tile early cost (re-packing rays between rounds could
// recover at most this); (out[1] - out[2])/out[0]: what waiting for the round's slowest lane costs.
// ... and the split VERDICT r4 #3 asked for: out[0..2] as rts_get_lane_stats, out[3] segments that walked at all, out[4] lane-steps issued to
// lanes that are in their tile's bounce round but never started a walk in it (a primary the pre-filter or every bounding sphere cleared, in a
// tile other lanes of which walk): out[4] / out[0] is what packing live launch indices of several tiles into dense waves could recover at most;
// (out[1] - out[2] - out[4]) / out[0] what waiting for the round's slowest WALKING lane costs.  n: capacity of out (<= 12 values are written).
static int rts_walk_counters(RtsContext* c, const char* who, uint64_t* out, uint32_t n)
{
    if (!c || !out) { rts_set_error("%s: null argument", who); return RTS_ERR_INVALID; }
    CHECK_CLOSED(c);
    const int src[12] = {8, 9, 10, 11, 15, 16, 17, 18, 19, 20, 21, 22};      // (out[5]: segments that skipped a target's walk above their triangle's horizon by the isotropic rule, out[11]: by an azimuth sector only; out[6], out[7]: the waves' walk iterations in bounce rounds >= 1, such rounds without any walk; out[8]: such rounds; out[9], out[10]: the walk iterations and the rounds of round 0 -- these five by each round's first lane, the three above by lane 0 of the wave)
    for (uint32_t k = 0; k < n && k < 12u; k++) out[k] = c->pin.p->cnt[src[k]];
    return RTS_OK;
}
extern "C" int rts_get_lane_stats(RtsHandle c, uint64_t* out3) { return rts_walk_counters(c, "rts_get_lane_stats", out3, 3); }
extern "C" int rts_get_walk_stats(RtsHandle c, uint64_t* out, uint32_t n) { return rts_walk_counters(c, "rts_get_walk_stats", out, n); }

extern "C" int rts_received_count(RtsHandle c, uint64_t* count)
{
    if (!c || !count) { rts_set_error("rts_received_count: null argument"); return RTS_ERR_INVALID; }
    CHECK_CLOSED(c);
    *count = c->res.n_recv; return RTS_OK;
}

extern "C" int rts_get_received(RtsHandle c, PerRayData* rays, int32_t* paths, double* rcs_angles, uint64_t* slots, uint64_t capacity)
{
    CHECK_HANDLE(c);
    CHECK_CLOSED(c);
    const uint64_t R = c->res.n_recv; const uint32_t D = c->depth;
    if (capacity < R) { rts_set_error("rts_get_received: capacity %llu < %llu received rays", (unsigned long long)capacity, (unsigned long long)R); return RTS_ERR_CAPACITY; }
    if (R == 0) return RTS_OK;
    RTS_HIP(hipStreamSynchronize(c->stream));
    RTS_HIP(rts_copy_home(rays, c->d_rx_rays.p, R)); RTS_HIP(rts_copy_home(paths, c->d_rx_paths.p, R * D));
    RTS_HIP(rts_copy_home(rcs_angles, c->d_rx_angles.p, 2 * R * D)); RTS_HIP(rts_copy_home(slots, c->d_rx_slots.p, R));
    return RTS_OK;
}

extern "C" int rts_get_all_rays(RtsHandle c, PerRayData* results, int32_t* targ_intersect, double* rcs_angle, int32_t* hit_prim, float* hit_t, uint64_t capacity)
{
    CHECK_HANDLE(c);
    CHECK_CLOSED(c);
    if (!(c->params.flags & RTS_FLAG_KEEP_ALL_RAYS)) { rts_set_error("rts_get_all_rays: handle was not created with RTS_FLAG_KEEP_ALL_RAYS"); return RTS_ERR_INVALID; }
    const uint64_t n1 = c->n_rays, n = n1 * c->last_args.rows; const uint32_t D = c->depth, H = rts_hit_rows(c->params.max_refl);
    if (capacity < n) { rts_set_error("rts_get_all_rays: capacity too small (%llu rows)", (unsigned long long)n); return RTS_ERR_CAPACITY; }
    if (n == 0) return RTS_OK;
    RTS_HIP(hipStreamSynchronize(c->stream));
    RTS_HIP(rts_copy_home(results, c->d_all_rays.p, n)); RTS_HIP(rts_copy_home(targ_intersect, c->d_all_paths.p, n * D)); RTS_HIP(rts_copy_home(rcs_angle, c->d_all_angles.p, 2 * n * D));
    RTS_HIP(rts_copy_home(hit_prim, c->d_hit_prim.p, n1 * H)); RTS_HIP(rts_copy_home(hit_t, c->d_hit_t.p, n1 * H));
    return RTS_OK;
}

extern "C" int rts_received_view(RtsHandle c, const PerRayData** rays, const int32_t** paths, const double** rcs_angles, const uint64_t** slots, uint64_t* count)
{
    CHECK_HANDLE(c);
    if (!count) { rts_set_error("rts_received_view: null count"); return RTS_ERR_INVALID; }
    CHECK_CLOSED(c);
    RtsPulseResults& r = c->res; const uint64_t R = r.n_recv; const uint32_t D = c->depth;
    *count = R;
    if (rays) *rays = nullptr; if (paths) *paths = nullptr; if (rcs_angles) *rcs_angles = nullptr; if (slots) *slots = nullptr;
    if (R == 0) return RTS_OK;
    RTS_HIP(rts_stream_wait(c, c->stream));
    const RtsHostMirror& m = r.mirror;
    if (m.recv_valid && R <= m.cap) {
        if (rays) *rays = (const PerRayData*)(m.buf.p + m.o_rays); if (paths) *paths = (const int32_t*)(m.buf.p + m.o_paths);
        if (rcs_angles) *rcs_angles = (const double*)(m.buf.p + m.o_angles); if (slots) *slots = (const uint64_t*)(m.buf.p + m.o_slots);
        return RTS_OK;
    }
    if (rays) RTS_HIP(rts_view_fill(r, 1u, r.v_rays, c->d_rx_rays.p, R, rays));
    if (paths && D) RTS_HIP(rts_view_fill(r, 2u, r.v_paths, c->d_rx_paths.p, R * D, paths));
    if (rcs_angles && D) RTS_HIP(rts_view_fill(r, 4u, r.v_angles, c->d_rx_angles.p, 2 * R * D, rcs_angles));
    if (slots) RTS_HIP(rts_view_fill(r, 8u, r.v_slots, c->d_rx_slots.p, R, slots));
    return RTS_OK;
}

// The per-received-ray update of ray_tracer.cpp:1219-1253 when the factors come from the simulator's callbacks: the caller has
// formed every received ray's final power and Doppler shift on the host (from rts_received_view's records); they replace the
// traced values on the device, in received order.  Enqueued (the values are copied out of the caller's arrays before the call
// returns); rts_aggregate follows.
extern "C" int rts_finalise_values(RtsHandle c, const double* power, const double* doppler, uint64_t count)
{
    CHECK_HANDLE(c);
    CHECK_CLOSED(c);
    if (count != c->res.n_recv) { rts_set_error("rts_finalise_values: %llu values for %llu received rays", (unsigned long long)count, (unsigned long long)c->res.n_recv); return RTS_ERR_INVALID; }
    if (count == 0) return RTS_OK;
    if (!power || !doppler) { rts_set_error("rts_finalise_values: null array"); return RTS_ERR_INVALID; }
    return rts_finalise_bracket(c, [&]() -> int {
        RtsHostMirror& m = c->res.mirror;
        if (!m.buf.p) RTS_TRY(rts_mirror_reserve(c, RTS_SMALL_CAP32));
        if (count <= m.cap) {
            // (the staging is free: what read it last -- this handle's previous pulse -- was waited for before this pulse was begun)
            memcpy(m.buf.p + m.o_vpower, power, sizeof(double) * count); memcpy(m.buf.p + m.o_vdoppler, doppler, sizeof(double) * count);
            return rts_post_set_values(c, (const double*)(m.buf.dev + m.o_vpower), (const double*)(m.buf.dev + m.o_vdoppler));
        }
        // a set beyond the mirror: blocking uploads into scratch the aggregation overwrites later
        RTS_HIP(c->d_delay.reserve(count)); RTS_HIP(c->d_phase.reserve(count));
        RTS_HIP(hipMemcpyAsync(c->d_delay.p, power, sizeof(double) * count, hipMemcpyHostToDevice, c->stream));
        RTS_HIP(hipMemcpyAsync(c->d_phase.p, doppler, sizeof(double) * count, hipMemcpyHostToDevice, c->stream));
        RTS_TRY(rts_post_set_values(c, c->d_delay.p, c->d_phase.p));
        RTS_HIP(hipStreamSynchronize(c->stream));
        return RTS_OK;
    });
}

// ------------------------------------------------------------------------------------- the aggregation
#define NEED_AGGREGATED(c, who) do { if (!(c)->res.agg_valid) { rts_set_error("%s: call rts_aggregate first", (who)); return RTS_ERR_INVALID; } } while (0)

// Per-ray outputs of the last rts_aggregate (what rs::kernel_wrapper leaves in h_rx_results_arr[].power / .doppler, h_delay_arr,
// h_phase_arr, h_pathMatch): pointers into the host mirror when the pulse was prefetched (the call waits for the handle's stream
// once), copies otherwise.  Valid until the handle's next rts_trace_pulse_begin.
extern "C" int rts_aggregated_view(RtsHandle c, const double** power, const double** doppler, const double** delay, const double** phase, const int32_t** path_match, uint64_t* count)
{
    CHECK_HANDLE(c);
    if (!count) { rts_set_error("rts_aggregated_view: null count"); return RTS_ERR_INVALID; }
    CHECK_CLOSED(c);
    NEED_AGGREGATED(c, "rts_aggregated_view");
    RtsPulseResults& r = c->res; const uint64_t R = r.n_recv;
    *count = R;
    if (power) *power = nullptr; if (doppler) *doppler = nullptr; if (delay) *delay = nullptr; if (phase) *phase = nullptr; if (path_match) *path_match = nullptr;
    if (R == 0) return RTS_OK;
    RTS_HIP(rts_stream_wait(c, c->stream));
    const RtsHostMirror& m = r.mirror;
    if (m.agg_valid && R <= m.cap) {
        if (power) *power = (const double*)(m.buf.p + m.o_apower); if (doppler) *doppler = (const double*)(m.buf.p + m.o_adoppler);
        if (delay) *delay = (const double*)(m.buf.p + m.o_adelay); if (phase) *phase = (const double*)(m.buf.p + m.o_aphase); if (path_match) *path_match = (const int32_t*)(m.buf.p + m.o_apm);
        return RTS_OK;
    }
    if (power || doppler) {
        RTS_HIP(rts_view_fill(r, 0u, r.v_agg_rays, c->d_rx_rays.p, R, (const PerRayData**)nullptr));      // (scratch of its own: rts_received_view's records stay as they were)
        r.v_apower.resize(R); r.v_adoppler.resize(R);
        for (uint64_t i = 0; i < R; i++) { r.v_apower[i] = r.v_agg_rays[i].power; r.v_adoppler[i] = r.v_agg_rays[i].doppler; }
        if (power) *power = r.v_apower.data(); if (doppler) *doppler = r.v_adoppler.data();
    }
    if (delay) RTS_HIP(rts_view_fill(r, 0u, r.v_adelay, c->d_delay.p, R, delay));
    if (phase) RTS_HIP(rts_view_fill(r, 0u, r.v_aphase, c->d_phase.p, R, phase));
    if (path_match) RTS_HIP(rts_view_fill(r, 0u, r.v_apm, c->d_pathmatch.p, R, path_match));
    return RTS_OK;
}

static int rts_groups_home(RtsContext* c, const char* who) { CHECK_CLOSED(c); NEED_AGGREGATED(c, who); return rts_aggregate_fetch(c, &c->res.groups); }      // the group table, read home if it is still on its way
extern "C" int rts_group_count(RtsHandle c, uint32_t* count)
{
    if (!c || !count) { rts_set_error("rts_group_count: null argument"); return RTS_ERR_INVALID; }
    RTS_TRY(rts_groups_home(c, "rts_group_count"));
    *count = (uint32_t)c->res.groups.size(); return RTS_OK;
}

extern "C" int rts_get_groups(RtsHandle c, RtsGroup* groups, uint32_t capacity)
{
    if (!c || (!groups && capacity)) { rts_set_error("rts_get_groups: null argument"); return RTS_ERR_INVALID; }
    RTS_TRY(rts_groups_home(c, "rts_get_groups"));
    if (capacity < c->res.groups.size()) { rts_set_error("rts_get_groups: capacity too small"); return RTS_ERR_CAPACITY; }
    if (!c->res.groups.empty()) memcpy(groups, c->res.groups.data(), sizeof(RtsGroup)*c->res.groups.size());
    return RTS_OK;
}

extern "C" int rts_get_aggregated(RtsHandle c, PerRayData* rays, double* delay, double* phase, int32_t* path_match, uint64_t capacity)
{
    CHECK_HANDLE(c);
    CHECK_CLOSED(c);
    NEED_AGGREGATED(c, "rts_get_aggregated");
    const uint64_t R = c->res.n_recv;
    if (capacity < R) { rts_set_error("rts_get_aggregated: capacity too small"); return RTS_ERR_CAPACITY; }
    if (R == 0) return RTS_OK;
    RTS_HIP(hipStreamSynchronize(c->stream));
    RTS_HIP(rts_copy_home(rays, c->d_rx_rays.p, R)); RTS_HIP(rts_copy_home(delay, c->d_delay.p, R));
    RTS_HIP(rts_copy_home(phase, c->d_phase.p, R)); RTS_HIP(rts_copy_home(path_match, c->d_pathmatch.p, R));
    return RTS_OK;
}
