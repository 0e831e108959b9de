// rts_cube_detect_api.hip -- the cube part of the C-ABI of include/rts_amd.h, the detection chain: both CFAR detectors and rts_cfar_os_alpha, plots, tracks, multistatic localisation,
// track-before-detect, and the pure-host evaluators that go with them.  Host code only, no kernels: argument checks, the handle's cube state (RtsCubeState:
// detect, plot, track, locate, tbd; rts_cube_state.h), the calls of the launchers in the kernels' units.
#include <cmath>
#include <cstring>
#include <algorithm>
#include "rts_cube_api.h"

// ------------------------------------------------------------------------------------- CFAR detection
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
    c->cube.detect.valid = false; c->cube.plot.valid = false;      // (plots index the list they were made from)
    return rts_cube_detect_device(c, *p, map, n_doppler, p->max_detections ? p->max_detections : RTS_CFAR_DEFAULT_MAX_DETECTIONS);
}

extern "C" int rts_cube_detections_get(RtsHandle c, RtsDetection* out, uint32_t capacity, uint32_t* n_out)
{
    CHECK_HANDLE(c);
    if (!n_out || (capacity && !out)) { rts_set_error("rts_cube_detections_get: null output"); return RTS_ERR_INVALID; }
    if (!c->cube.detect.valid) { rts_set_error("rts_cube_detections_get: no detection list (rts_cube_detect, rts_cube_detect_os; a list ends at rts_cube_attach)"); return RTS_ERR_INVALID; }
    uint32_t n = 0;
    RTS_TRY(rts_list_copy_out(c, c->cube.detect.d_off.p + c->cube.detect.nseg, c->cube.detect.max, c->cube.detect.d_list.p, sizeof(RtsDetection), out, capacity, n_out, &n));
    return rts_list_fits_check("rts_cube_detections_get", "%s: %u of %u detections copied (max_detections %u, capacity %u)", n, *n_out, c->cube.detect.max, capacity);
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
    c->cube.detect.valid = false; c->cube.plot.valid = false;      // (plots index the list they were made from)
    // the alphas by training count -> pinned staging -> the device, on the stream (N0 + 1 <= RTS_CFAR_OS_MAX_TRAIN + 1: one size for every call);
    // a call that needs nothing the device table of the previous one lacks sends nothing
    const double* tab_dev = nullptr;
    if (p->pfa != 0.0) {
        RtsCubeState& s = c->cube;
        const uint32_t N0 = rts_cfar_n0(p->guard_range, p->guard_doppler, p->train_range, p->train_doppler);
        const uint32_t key[5] = {p->guard_range, p->guard_doppler, p->train_range, p->train_doppler, p->rank};
        if (s.detect.os_tab.size() != (size_t)N0 + 1 || memcmp(key, s.detect.os_key, sizeof(key)) != 0 || s.detect.os_pfa != p->pfa) {
            s.detect.os_tab.assign((size_t)N0 + 1, 0.0); memcpy(s.detect.os_key, key, sizeof(key)); s.detect.os_pfa = p->pfa; s.detect.os_sent = false;
        }
        if (rts_cfar_os_alpha_table(p->guard_range, p->guard_doppler, p->train_range, p->train_doppler, p->rank, p->pfa, nb, s.detect.os_tab.data()) != 0) s.detect.os_sent = false;
        if (!s.detect.os_sent) {
            double* h = nullptr;
            RTS_HIP(s.detect.os_alpha.begin(RTS_CFAR_OS_MAX_TRAIN + 1u, RTS_CFAR_OS_MAX_TRAIN + 1u, RTS_CFAR_OS_MAX_TRAIN + 1u, &h));
            memcpy(h, s.detect.os_tab.data(), sizeof(double) * ((size_t)N0 + 1));
            RTS_HIP(s.detect.os_alpha.send((size_t)N0 + 1, c->stream));
            s.detect.os_sent = true;
        }
        tab_dev = s.detect.os_alpha.dev.p;
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
        if (!s.detect.valid) { rts_set_error("%s: no detection list (rts_cube_detect, rts_cube_detect_os; a list ends at rts_cube_attach) and no device_list", who); return RTS_ERR_INVALID; }
        list = s.detect.d_list.p; n_dev = s.detect.d_off.p + s.detect.nseg; n_cap = s.detect.max; nd = s.detect.nd;
    }
    if (n_cap > RTS_PLOT_MAX_LIST) { rts_set_error("%s: a list of %u records > %u", who, n_cap, RTS_PLOT_MAX_LIST); return RTS_ERR_INVALID; }
    s.plot.valid = false; s.plot.own_list = p->device_list == nullptr;
    return rts_cube_plots_device(c, *p, list, n_dev, n_cap, nd, p->max_plots ? p->max_plots : n_cap);
}

extern "C" int rts_cube_plots_get(RtsHandle c, RtsPlot* out, uint32_t capacity, uint32_t* n_out)
{
    const char* who = "rts_cube_plots_get";
    CHECK_HANDLE(c);
    if (!n_out || (capacity && !out)) { rts_set_error("%s: null output", who); return RTS_ERR_INVALID; }
    RtsCubeState& s = c->cube;
    if (!s.plot.valid) { rts_set_error("%s: no plots (rts_cube_plots; plots end at rts_cube_detect, rts_cube_detect_os and rts_cube_attach)", who); return RTS_ERR_INVALID; }
    uint32_t total = 0, det_total = 0, n = 0;
    RTS_TRY(rts_list_copy_out(c, s.plot.d_off.p + s.plot.cap, s.plot.max, s.plot.d_list.p, sizeof(RtsPlot), out, capacity, &total, &n));
    if (s.plot.own_list) RTS_HIP(hipMemcpy(&det_total, s.detect.d_off.p + s.detect.nseg, sizeof(uint32_t), hipMemcpyDeviceToHost));
    *n_out = total;
    RTS_TRY(rts_list_fits_check(who, "%s: %u of %u plots copied (max_plots %u, capacity %u)", n, total, s.plot.max, capacity));
    if (s.plot.own_list && det_total > s.detect.max) {
        rts_set_error("%s: the detection list was truncated (%u of %u detections stored): the %u plots describe the stored prefix", who, s.detect.max, det_total, total); return RTS_ERR_CAPACITY; }
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
    if (s.track.max && table != s.track.max) { rts_set_error("%s: max_tracks = %u, the table was made with %u (rts_cube_tracks_reset first)", who, table, s.track.max); return RTS_ERR_INVALID; }
    if (table < s.track.loaded) { rts_set_error("%s: max_tracks = %u below the %u tracks loaded", who, table, s.track.loaded); return RTS_ERR_INVALID; }
    if (!rts_track_finite(time)) { rts_set_error("%s: time = %g (finite)", who, time); return RTS_ERR_INVALID; }
    const double T = s.track.live ? time - s.track.time : 0.0;
    if (s.track.live && !rts_track_interval_ok(T)) { rts_set_error("%s: T = time - the previous frame's = %g (positive, finite)", who, T); return RTS_ERR_INVALID; }
    const RtsPlot* list = (const RtsPlot*)p->device_plots;
    const uint32_t* n_dev = nullptr;
    uint32_t pcap = p->n_plots;
    if (!list) {
        if (!s.plot.valid) { rts_set_error("%s: no plots (rts_cube_plots; plots end at the detect calls and rts_cube_attach) and no device_plots", who); return RTS_ERR_INVALID; }
        list = s.plot.d_list.p; n_dev = s.plot.d_off.p + s.plot.cap; pcap = s.plot.max;
        if (pcap > RTS_TRACK_MAX_PLOTS) { rts_set_error("%s: a plot list of %u records > %u (RTS_TRACK_MAX_PLOTS)", who, pcap, RTS_TRACK_MAX_PLOTS); return RTS_ERR_INVALID; }
    }
    RTS_TRY(rts_cube_track_device(c, *p, T, list, n_dev, pcap, table));
    s.track.max = table; s.track.loaded = 0; s.track.live = true; s.track.time = time;
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
    RTS_HIP(hipMemcpy(&m, s.track.d_meta.p + s.track.cur, sizeof(m), hipMemcpyDeviceToHost));
    *n_out = m.total;
    if (next_id_out) *next_id_out = m.next_id;
    const uint32_t n = m.n < capacity ? m.n : capacity;
    if (n) RTS_HIP(hipMemcpy(out, s.track.d_tab[s.track.cur].p, sizeof(RtsTrack) * n, hipMemcpyDeviceToHost));
    return rts_list_fits_check(who, "%s: %u of %u tracks copied (max_tracks %u, capacity %u)", n, m.total, s.track.max, capacity);
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
    RTS_HIP(hipMemcpy(&m, s.track.d_meta.p + s.track.cur, sizeof(m), hipMemcpyDeviceToHost));
    *rounds = m.rounds;
    return RTS_OK;
}

static int rts_tracks_load(RtsContext* c, const RtsTrack* t, uint32_t n, const uint64_t* next_id)
{
    RtsCubeState& s = c->cube;
    RTS_TRY(rts_cube_track_tables(c));
    RTS_HIP(hipStreamSynchronize(c->stream));                 // (an enqueued step may still read and write both tables)
    RtsTrackMeta m;
    RTS_HIP(hipMemcpy(&m, s.track.d_meta.p + s.track.cur, sizeof(m), hipMemcpyDeviceToHost));
    m.n = n; m.total = n; m.rounds = 0; m.reserved = 0;
    if (next_id) m.next_id = *next_id;
    if (n) RTS_HIP(hipMemcpy(s.track.d_tab[s.track.cur].p, t, sizeof(RtsTrack) * n, hipMemcpyHostToDevice));
    RTS_HIP(hipMemcpy(s.track.d_meta.p + s.track.cur, &m, sizeof(m), hipMemcpyHostToDevice));
    s.track.max = 0; s.track.loaded = n;
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
    c->cube.track.live = n != 0u; c->cube.track.time = time;
    return RTS_OK;
}

extern "C" int rts_cube_tracks_reset(RtsHandle c)
{
    CHECK_HANDLE(c);
    CHECK_CLOSED(c);
    RTS_TRY(rts_tracks_load(c, nullptr, 0, nullptr));
    c->cube.track.live = false;
    return RTS_OK;
}

// ------------------------------------------------------------------------------------- multistatic localisation
// (rts_amd.h: RtsLocateParams, RtsTarget; the rules and the host evaluator are rts_locate.h, shared with the kernels, rts_locate.hip)
static int rts_locate_check(const char* who, const RtsLocateParams* p)
{
    if (!p) { rts_set_error("%s: null parameters", who); return RTS_ERR_INVALID; }
    switch (rts_locate_params_check(p)) {
        case 0: return RTS_OK;
        case 1: rts_set_error("%s: n_rx = %u (3 .. %u, RTS_LOCATE_MAX_RX)", who, p->n_rx, RTS_LOCATE_MAX_RX); break;
        case 2: rts_set_error("%s: null rx_positions", who); break;
        case 3: rts_set_error("%s: tx and rx_positions must be finite", who); break;
        case 4: rts_set_error("%s: anchors = (%u, %u, %u): three distinct receivers below n_rx = %u", who, p->anchors[0], p->anchors[1], p->anchors[2], p->n_rx); break;
        case 5: rts_set_error("%s: anchors = (%u, %u, %u): their baselines are collinear", who, p->anchors[0], p->anchors[1], p->anchors[2]); break;
        case 6: rts_set_error("%s: cspeed = %g (finite, > 0)", who, p->cspeed); break;
        case 7: rts_set_error("%s: carrier = %g (finite, >= 0)", who, p->carrier); break;
        case 8: rts_set_error("%s: sigma_delay = %g (finite, > 0)", who, p->sigma_delay); break;
        case 9: rts_set_error("%s: sigma_doppler = %g (finite, > 0)", who, p->sigma_doppler); break;
        case 10: rts_set_error("%s: gate = %g (finite, > 0)", who, p->gate); break;
        case 11: rts_set_error("%s: assoc_delay = %g (finite, > 0)", who, p->assoc_delay); break;
        case 12: rts_set_error("%s: box_lo, box_hi must be finite with box_lo <= box_hi on every axis", who); break;
        case 13: rts_set_error("%s: min_receivers = %u (3 .. n_rx = %u)", who, p->min_receivers, p->n_rx); break;
        case 14: rts_set_error("%s: n_iters = %u > %u (RTS_LOCATE_MAX_ITERS)", who, p->n_iters, RTS_LOCATE_MAX_ITERS); break;
        case 15: rts_set_error("%s: max_candidates = %u > %u (RTS_LOCATE_MAX_CANDIDATES)", who, p->max_candidates, RTS_LOCATE_MAX_CANDIDATES); break;
        case 16: rts_set_error("%s: max_targets = %u > %u (RTS_LOCATE_MAX_TARGETS)", who, p->max_targets, RTS_LOCATE_MAX_TARGETS); break;
        case 17: rts_set_error("%s: unknown source %u (RTS_LOCATE_FROM_PLOTS, _TRACKS, _CANDIDATES)", who, p->source); break;
        case 18: rts_set_error("%s: n_list = %u without device_list", who, p->n_list); break;
        case 19: rts_set_error("%s: n_list = %u > %u, the source's limit", who, p->n_list, rts_locate_list_most(p->source)); break;
        case 20: rts_set_error("%s: device_list is not 8-byte aligned", who); break;
        case 21: rts_set_error("%s: reserved fields must be 0", who); break;
        default: rts_set_error("%s: device_list with RTS_LOCATE_FROM_TRACKS (the source is the handle's table)", who); break;
    }
    return RTS_ERR_INVALID;
}
// what every getter of a locate list says beyond the copy: the candidates or an anchor's segment were cut
static int rts_locate_cut_check(const char* who, bool cand_cut, bool seg_cut, uint32_t total)
{
    if (cand_cut) { rts_set_error("%s: max_candidates cut the accepted candidates: the %u targets resolve the stored prefix", who, total); return RTS_ERR_CAPACITY; }
    if (seg_cut) { rts_set_error("%s: an anchor's segment holds more than %u records (RTS_LOCATE_MAX_PER_RX): the %u targets use its first ones", who, RTS_LOCATE_MAX_PER_RX, total); return RTS_ERR_CAPACITY; }
    return RTS_OK;
}

extern "C" int rts_locate_eval(const RtsLocateParams* p, const void* list, uint32_t n_list, RtsTarget* out, uint32_t capacity, uint32_t* n_out)
{
    const char* who = "rts_locate_eval";
    RTS_TRY(rts_locate_check(who, p));
    if (!n_out || (capacity && !out)) { rts_set_error("%s: null output", who); return RTS_ERR_INVALID; }
    switch (rts_device_list_rule(list, n_list, rts_locate_list_most(p->source))) {      // (the rule of p->device_list, on the host list)
        case 0: break;
        case 1: rts_set_error("%s: null list with n_list = %u", who, n_list); return RTS_ERR_INVALID;
        case 2: rts_set_error("%s: n_list = %u > %u", who, n_list, rts_locate_list_most(p->source)); return RTS_ERR_INVALID;
        default: rts_set_error("%s: list is not 8-byte aligned", who); return RTS_ERR_INVALID;
    }
    uint32_t bad = 0;
    if (p->source == RTS_LOCATE_FROM_PLOTS && rts_locate_plots_check((const RtsPlot*)list, n_list, &bad)) {
        rts_set_error("%s: list[%u].rx is below list[%u].rx (rx must not decrease)", who, bad, bad - 1u); return RTS_ERR_INVALID; }
    if (p->source == RTS_LOCATE_FROM_CANDIDATES) switch (rts_locate_candidates_check((const RtsTarget*)list, n_list, &bad)) {
        case 0: break;
        case 1: rts_set_error("%s: list[%u].candidate is not above list[%u].candidate", who, bad, bad - 1u); return RTS_ERR_INVALID;
        case 2: rts_set_error("%s: list[%u] names an index >= %u (RTS_LOCATE_MAX_INDEX)", who, bad, RTS_LOCATE_MAX_INDEX); return RTS_ERR_INVALID;
        case 3: rts_set_error("%s: list[%u].n_receivers outside 1 .. %u", who, bad, RTS_LOCATE_MAX_RX); return RTS_ERR_INVALID;
        default: rts_set_error("%s: list[%u].cost is negative or NaN", who, bad); return RTS_ERR_INVALID;
    }
    uint32_t cut = 0;
    const uint32_t total = rts_locate_eval_host(p, list, n_list, out, capacity, &cut), max_t = rts_locate_max_targets(*p);
    *n_out = total;
    RTS_TRY(rts_list_fits_check(who, "%s: %u of %u targets written (max_targets %u, capacity %u)", rts_list_copied(total, max_t, capacity), total, max_t, capacity));
    return rts_locate_cut_check(who, (cut & 1u) != 0u, (cut & 2u) != 0u, total);
}

extern "C" int rts_cube_locate(RtsHandle c, const RtsLocateParams* p)
{
    const char* who = "rts_cube_locate";
    CHECK_HANDLE(c);
    RTS_TRY(rts_locate_check(who, p));
    CHECK_CLOSED(c);
    RtsCubeState& s = c->cube;
    const void* list = p->device_list; const void* n_dev = nullptr;
    uint32_t rcap = p->n_list;
    if (p->source == RTS_LOCATE_FROM_PLOTS && !list) {
        if (!s.plot.valid) { rts_set_error("%s: no plots (rts_cube_plots; plots end at the detect calls and rts_cube_attach) and no device_list", who); return RTS_ERR_INVALID; }
        list = s.plot.d_list.p; n_dev = s.plot.d_off.p + s.plot.cap; rcap = s.plot.max;
        if (rcap > RTS_LOCATE_MAX_LIST) { rts_set_error("%s: a plot list of %u records > %u (RTS_LOCATE_MAX_LIST)", who, rcap, RTS_LOCATE_MAX_LIST); return RTS_ERR_INVALID; }
    } else if (p->source == RTS_LOCATE_FROM_TRACKS) {
        RTS_TRY(rts_cube_track_tables(c));
        list = s.track.d_tab[s.track.cur].p; n_dev = s.track.d_meta.p + s.track.cur; rcap = s.track.max ? s.track.max : RTS_TRACK_MAX_TRACKS;
    } else if (p->source == RTS_LOCATE_FROM_CANDIDATES && !list) { rts_set_error("%s: RTS_LOCATE_FROM_CANDIDATES without device_list", who); return RTS_ERR_INVALID; }
    s.locate.valid = false;
    const RtsLocateGeo* geo = nullptr;
    if (p->source != RTS_LOCATE_FROM_CANDIDATES) {                      // the call's constants -> pinned staging -> the device, on the stream
        const RtsLocateGeo g = rts_locate_geo(*p);
        RTS_HIP(s.locate.geo.upload(&g, 1, 1, c->stream));
        geo = s.locate.geo.dev.p;
    }
    const uint32_t max_c = rts_locate_max_candidates(*p), max_t = rts_locate_max_targets(*p);
    RTS_TRY(rts_cube_locate_device(c, *p, geo, list, n_dev, rcap, max_c, max_t));
    s.locate.max_c = max_c; s.locate.max_t = max_t; s.locate.valid = true;
    return RTS_OK;
}

static int rts_locate_meta(RtsContext* c, const char* who, RtsLocateMeta* m)
{
    if (!c->cube.locate.valid) { rts_set_error("%s: no targets (rts_cube_locate)", who); return RTS_ERR_INVALID; }
    RTS_HIP(hipStreamSynchronize(c->stream));
    RTS_HIP(hipMemcpy(m, c->cube.locate.d_meta.p, sizeof(*m), hipMemcpyDeviceToHost));
    return RTS_OK;
}

extern "C" int rts_cube_targets_get(RtsHandle c, RtsTarget* out, uint32_t capacity, uint32_t* n_out)
{
    const char* who = "rts_cube_targets_get";
    CHECK_HANDLE(c);
    if (!n_out || (capacity && !out)) { rts_set_error("%s: null output", who); return RTS_ERR_INVALID; }
    RtsLocateState& s = c->cube.locate;
    RtsLocateMeta m;
    RTS_TRY(rts_locate_meta(c, who, &m));
    const uint32_t n = rts_list_copied(m.targets_total, s.max_t, capacity);
    if (n) RTS_HIP(hipMemcpy(out, s.d_out.p, sizeof(RtsTarget) * n, hipMemcpyDeviceToHost));
    *n_out = m.targets_total;
    RTS_TRY(rts_list_fits_check(who, "%s: %u of %u targets copied (max_targets %u, capacity %u)", n, m.targets_total, s.max_t, capacity));
    return rts_locate_cut_check(who, m.cand_total > s.max_c, m.seg_cut != 0u, m.targets_total);
}

// the rounds the resolution of the last rts_cube_locate took (tools/locate_bench.py); synchronises
extern "C" int rts_cube_locate_rounds(RtsHandle c, uint32_t* rounds)
{
    const char* who = "rts_cube_locate_rounds";
    CHECK_HANDLE(c);
    if (!rounds) { rts_set_error("%s: null output", who); return RTS_ERR_INVALID; }
    RtsLocateMeta m;
    RTS_TRY(rts_locate_meta(c, who, &m));
    *rounds = m.rounds;
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
    const bool first = s.tbd.frames == 0;
    double T = 0.0;
    if (!first) {
        if (q.n_rx != s.tbd.rx || n_doppler != s.tbd.nd || q.n_bins != s.tbd.nb) {
            rts_set_error("%s: a map of %u x %u x %u cells, the state has %u x %u x %u (rts_cube_tbd_reset first)", who, q.n_rx, n_doppler, q.n_bins, s.tbd.rx, s.tbd.nd, s.tbd.nb); return RTS_ERR_INVALID; }
        if (p->depth != s.tbd.depth || p->half_doppler != s.tbd.hd || p->half_range != s.tbd.hr) {
            rts_set_error("%s: depth, half_doppler, half_range = %u, %u, %u, the state was made with %u, %u, %u (rts_cube_tbd_reset first)", who, p->depth, p->half_doppler, p->half_range,
                          s.tbd.depth, s.tbd.hd, s.tbd.hr); return RTS_ERR_INVALID; }
        T = time - s.tbd.time;
        RTS_TRY(rts_tbd_shifts_refuse(who, p, n_doppler, T, q.dt));
    } else {
        // the state's buffers, of their final sizes (a DevBuf that grows drops what it held: they are made once per state)
        const size_t cells = (size_t)q.n_rx * n_doppler * q.n_bins;
        RTS_HIP(s.tbd.d_merit[0].reserve(cells)); RTS_HIP(s.tbd.d_merit[1].reserve(cells));
        RTS_HIP(s.tbd.d_ptr.reserve(cells * p->depth)); RTS_HIP(s.tbd.d_shift.reserve((size_t)n_doppler * p->depth));
        s.tbd.rx = q.n_rx; s.tbd.nd = n_doppler; s.tbd.nb = q.n_bins; s.tbd.depth = p->depth; s.tbd.hd = p->half_doppler; s.tbd.hr = p->half_range; s.tbd.cur = 0;
    }
    RTS_TRY(rts_cube_tbd_step_device(c, *p, map, first, T, q.dt, (uint32_t)(s.tbd.frames % s.tbd.depth)));
    s.tbd.frames++; s.tbd.time = time; s.tbd.t0 = q.t0; s.tbd.dt = q.dt;
    return RTS_OK;
}

#define NEED_TBD(c, who) do { if ((c)->cube.tbd.frames == 0) { rts_set_error("%s: no track-before-detect state (rts_cube_tbd_step; a state ends at rts_cube_tbd_reset)", (who)); return RTS_ERR_INVALID; } } while (0)

extern "C" int rts_cube_tbd_extract(RtsHandle c, const RtsTbdExtractParams* e)
{
    const char* who = "rts_cube_tbd_extract";
    CHECK_HANDLE(c);
    RTS_TRY(rts_tbd_extract_refuse(who, e));
    CHECK_CLOSED(c);
    NEED_TBD(c, who);
    c->cube.tbd.ext_valid = false;
    return rts_cube_tbd_extract_device(c, *e, rts_tbd_max_tracks(*e));
}

// the extraction's records or their paths (record_bytes each) -> the host: the total, and how many of the stored ones fit `capacity`
static int rts_tbd_extracted(RtsContext* c, const char* who, const void* d_list, size_t record_bytes, void* out, uint32_t capacity, uint32_t* total, uint32_t* n)
{
    RtsCubeState& s = c->cube;
    if (!s.tbd.ext_valid) { rts_set_error("%s: no extraction (rts_cube_tbd_extract; it ends at rts_cube_tbd_reset)", who); return RTS_ERR_INVALID; }
    return rts_list_copy_out(c, s.tbd.d_off.p + s.tbd.ext_nseg, s.tbd.ext_max, d_list, record_bytes, out, capacity, total, n);
}

extern "C" int rts_cube_tbd_tracks_get(RtsHandle c, RtsTbdTrack* out, uint32_t capacity, uint32_t* n_out)
{
    const char* who = "rts_cube_tbd_tracks_get";
    CHECK_HANDLE(c);
    if (!n_out || (capacity && !out)) { rts_set_error("%s: null output", who); return RTS_ERR_INVALID; }
    uint32_t total = 0, n = 0;
    RTS_TRY(rts_tbd_extracted(c, who, c->cube.tbd.d_out.p, sizeof(RtsTbdTrack), out, capacity, &total, &n));
    *n_out = total;
    return rts_list_fits_check(who, "%s: %u of %u tracks copied (max_tracks %u, capacity %u)", n, total, c->cube.tbd.ext_max, capacity);
}

extern "C" int rts_cube_tbd_paths_get(RtsHandle c, uint32_t* out, uint32_t capacity_tracks)
{
    const char* who = "rts_cube_tbd_paths_get";
    CHECK_HANDLE(c);
    if (capacity_tracks && !out) { rts_set_error("%s: null output", who); return RTS_ERR_INVALID; }
    uint32_t total = 0, n = 0;
    RTS_TRY(rts_tbd_extracted(c, who, c->cube.tbd.d_paths.p, sizeof(uint32_t) * 2u * c->cube.tbd.ext_depth, out, capacity_tracks, &total, &n));
    return rts_list_fits_check(who, "%s: the paths of %u of %u tracks copied (max_tracks %u, capacity %u)", n, total, c->cube.tbd.ext_max, capacity_tracks);
}

extern "C" int rts_cube_tbd_merit_get(RtsHandle c, double* host_out, uint64_t capacity_doubles)
{
    const char* who = "rts_cube_tbd_merit_get";
    CHECK_HANDLE(c);
    NEED_TBD(c, who);
    RtsCubeState& s = c->cube;
    const size_t cells = (size_t)s.tbd.rx * s.tbd.nd * s.tbd.nb;
    if (!host_out) { rts_set_error("%s: null output", who); return RTS_ERR_INVALID; }
    if (capacity_doubles < cells) { rts_set_error("%s: capacity too small", who); return RTS_ERR_CAPACITY; }
    RTS_HIP(hipStreamSynchronize(c->stream));
    RTS_HIP(hipMemcpy(host_out, s.tbd.d_merit[s.tbd.cur].p, sizeof(double) * cells, hipMemcpyDeviceToHost));
    return RTS_OK;
}

extern "C" int rts_cube_tbd_ring_get(RtsHandle c, uint8_t* ptr_out, int32_t* shifts_out, uint32_t capacity_frames, uint32_t* n_frames_out)
{
    const char* who = "rts_cube_tbd_ring_get";
    CHECK_HANDLE(c);
    NEED_TBD(c, who);
    RtsCubeState& s = c->cube;
    if (!n_frames_out || (capacity_frames && (!ptr_out || !shifts_out))) { rts_set_error("%s: null output", who); return RTS_ERR_INVALID; }
    const uint32_t have = s.tbd.frames < s.tbd.depth ? (uint32_t)s.tbd.frames : s.tbd.depth;
    *n_frames_out = have;
    if (capacity_frames < have) { rts_set_error("%s: %u frames stored, capacity %u", who, have, capacity_frames); return RTS_ERR_CAPACITY; }
    const size_t cells = (size_t)s.tbd.rx * s.tbd.nd * s.tbd.nb;
    RTS_HIP(hipStreamSynchronize(c->stream));
    for (uint32_t i = 0; i < have; i++) {                               // oldest first: frame frames - have + i
        const size_t slot = (size_t)((s.tbd.frames - have + i) % s.tbd.depth);
        RTS_HIP(hipMemcpy(ptr_out + (size_t)i * cells, s.tbd.d_ptr.p + slot * cells, cells, hipMemcpyDeviceToHost));
        RTS_HIP(hipMemcpy(shifts_out + (size_t)i * s.tbd.nd, s.tbd.d_shift.p + slot * s.tbd.nd, sizeof(int32_t) * s.tbd.nd, hipMemcpyDeviceToHost));
    }
    return RTS_OK;
}

extern "C" int rts_cube_tbd_info(RtsHandle c, uint32_t shape_out[4], uint64_t* frames_out)
{
    CHECK_HANDLE(c);
    if (!shape_out || !frames_out) { rts_set_error("rts_cube_tbd_info: null output"); return RTS_ERR_INVALID; }
    const RtsCubeState& s = c->cube;
    const bool have = s.tbd.frames != 0;
    shape_out[0] = have ? s.tbd.rx : 0u; shape_out[1] = have ? s.tbd.nd : 0u; shape_out[2] = have ? s.tbd.nb : 0u; shape_out[3] = have ? s.tbd.depth : 0u;
    *frames_out = s.tbd.frames;
    return RTS_OK;
}

extern "C" int rts_cube_tbd_reset(RtsHandle c)
{
    CHECK_HANDLE(c);
    c->cube.tbd.frames = 0; c->cube.tbd.ext_valid = false;      // (the buffers stay: work enqueued on them runs before the next state's, on the same stream)
    return RTS_OK;
}
