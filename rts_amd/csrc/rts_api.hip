// rts_api.hip -- host side of librts_amd.so: the C-ABI of include/rts_amd.h but for the scene (rts_scene.hip), the cube (rts_cube_api.hip, rts_cube_detect_api.hip, rts_cube_array_api.hip; rts_cube_reduce is here) and the accessors of a pulse's results (rts_results_api.hip).
//
// Mirrors the host driver rs::RTS of the reference (ray_tracer.cpp:507-1364) from the point
// where it owns device state: context set-up, per-pulse scene placement, launch, read-back,
// aggregation.  There is no CPU compute path: without a usable HIP device every compute
// entry point fails with RTS_ERR_NO_DEVICE.
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <cstdlib>
#include <dlfcn.h>
#include <algorithm>
#include <chrono>
#include <map>
#include <mutex>
#include <stdexcept>
#include <string>
#include "rts_internal.h"
#include "rts_raygen.h"
#include <atomic>

static thread_local char g_err[1024] = "";
void rts_set_error(const char* fmt, ...) { va_list ap; va_start(ap, fmt); vsnprintf(g_err, sizeof(g_err), fmt, ap); va_end(ap); }
extern "C" const char* rts_last_error(void) { return g_err; }
#include "rts_build_id.h"
extern "C" const char* rts_build_id(void) { return RTS_SOURCE_HASH; }

// One process (or one group of host threads) per GPU, ON THE GPU'S SOCKET: every kernel launch is a doorbell write and every
// completion a signal read across the fabric otherwise -- on the two-socket hosts of this pool a pipelined BASELINE configs[2]
// pulse took 0.68 ms instead of 0.63 ms when the scheduler happened to start the process on the other socket (the host side
// of rts_trace_pulse_begin alone 0.13 instead of 0.08 ms).  Restricts EVERY thread the process has at the time of the call
// (the runtime's helper threads included; threads created later inherit) to the CPUs of the device's NUMA node, within the
// set the process is allowed already.  *numa_node: the node, -1 when the platform does not say (nothing is changed then).
#include <dirent.h>
#include <sched.h>
extern "C" int rts_bind_host_to_device(int device, int* numa_node)
{
    if (numa_node) *numa_node = -1;
    char bdf[64] = {0};
    if (hipDeviceGetPCIBusId(bdf, (int)sizeof(bdf), device) != hipSuccess) { (void)hipGetLastError(); rts_set_error("rts_bind_host_to_device: no PCI address for device %d", device); return RTS_ERR_INVALID; }
    for (char* q = bdf; *q; q++) *q = (char)tolower((unsigned char)*q);
    char path[256]; snprintf(path, sizeof(path), "/sys/bus/pci/devices/%s/numa_node", bdf);
    int node = -1;
    if (FILE* f = fopen(path, "r")) { if (fscanf(f, "%d", &node) != 1) node = -1; fclose(f); }
    if (node < 0) return RTS_OK;
    snprintf(path, sizeof(path), "/sys/devices/system/node/node%d/cpulist", node);
    cpu_set_t want; CPU_ZERO(&want); int n_want = 0;
    if (FILE* f = fopen(path, "r")) {                                  // "64-127,192-255"
        int a = 0, b = 0; char sep = 0;
        while (fscanf(f, "%d", &a) == 1) {
            b = a;
            int ch = fgetc(f);
            if (ch == '-') { if (fscanf(f, "%d", &b) != 1) b = a; ch = fgetc(f); }
            for (int k = a; k <= b && k < CPU_SETSIZE; k++) { CPU_SET(k, &want); n_want++; }
            sep = (char)ch; if (sep != ',') break;
        }
        fclose(f);
    }
    if (n_want == 0) return RTS_OK;
    cpu_set_t have; CPU_ZERO(&have);
    if (sched_getaffinity(0, sizeof(have), &have) != 0) return RTS_OK;
    cpu_set_t both; CPU_AND(&both, &want, &have);
    if (CPU_COUNT(&both) == 0) return RTS_OK;                           // (the process is confined to the other socket: leave it)
    if (DIR* d = opendir("/proc/self/task")) {
        while (struct dirent* e = readdir(d)) { const int tid = atoi(e->d_name); if (tid > 0) (void)sched_setaffinity(tid, sizeof(both), &both); }
        closedir(d);
    } else (void)sched_setaffinity(0, sizeof(both), &both);
    if (numa_node) *numa_node = node;
    return RTS_OK;
}

extern int rts_fill_i32(hipStream_t st, int32_t* p, int32_t v, size_t n);

// The two waits of a pulse (its trace, its post-processing): a thread blocked in hipStreamSynchronize lets its core fall
// asleep, and every wake-up -- two per pulse, each in front of work the GPU is waiting for -- costs tens of microseconds on
// the hosts of this pool (the C++ adapter's loop ran 0.44 ms per pulse right after a second of host-side hierarchy build had
// kept the core awake, 0.72 ms otherwise).  RtsTuning::spin_wait (default on; RTS_SPIN_WAIT=0): poll the stream instead.
hipError_t rts_stream_wait(RtsContext* c, hipStream_t st)
{
    if (!c->tune.spin_wait) return hipStreamSynchronize(st);
    for (;;) {
        const hipError_t e = hipStreamQuery(st);
        if (e != hipErrorNotReady) return e;
        __builtin_ia32_pause();
    }
}
void rts_comm_cache_forget(RtsContext* c);

// The environment, as the readers of rts_tuning.h take it: the library looks at it nowhere else.
const char* rts_env(const char* name) { return getenv(name); }
// RTS_LAP, RTS_DEBUG_SYNC: read once per process, by whichever of the two is asked for first
static const RtsProcessTuning& rts_process_tuning() { static const RtsProcessTuning t = [] { RtsProcessTuning r; rts_tuning_read(&r, rts_env); return r; }(); return t; }

int rts_debug_stage(RtsContext* c, const char* name)
{
    if (!rts_process_tuning().debug_sync) return RTS_OK;
    fprintf(stderr, "[rts] stage %s ... ", name); fflush(stderr);
    hipError_t e = hipStreamSynchronize(c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->tstream);
    if (e != hipSuccess) { fprintf(stderr, "FAILED: %s\n", hipGetErrorString(e)); rts_set_error("stage %s: %s", name, hipGetErrorString(e)); return RTS_ERR_HIP; }
    fprintf(stderr, "ok\n"); fflush(stderr);
    return RTS_OK;
}

extern "C" int rts_device_count(int* n)
{
    if (!n) { rts_set_error("rts_device_count: null output"); return RTS_ERR_INVALID; }
    int k = 0; hipError_t e = hipGetDeviceCount(&k);
    if (e != hipSuccess) { *n = 0; rts_set_error("hipGetDeviceCount: %s", hipGetErrorString(e)); return RTS_ERR_NO_DEVICE; }
    *n = k; return RTS_OK;
}

void rts_hist_unref(RtsTileHist* h) { if (h && --h->refs == 0) delete h; }
void rts_gate_unref(RtsGate* g) { if (g && --g->refs == 0) { if (g->tstream) (void)hipStreamDestroy(g->tstream); delete g; } }

// The teardown of a handle, once.  After this body the members destroy themselves in reverse order of declaration: every DevBuf
// (hipFree), the pinned blocks pin, pin_rx and the mirror's (hipHostFree) and the staged uploads (pat_rx and the cube's, one per family that has a
// table to send: cube.detect.os_alpha, cube.image.geo, cube.stft.win ...: their event, then their blocks), in the order rts_cube_state.h's grouping gives.  That is safe because no work can read
// them any more: `stream` and `cstream` have been drained, the trace stream has been drained (it may live on with the other
// handles of the link group, but carries no work of this handle), and nothing is enqueued on a handle's behalf anywhere else.
RtsContext::~RtsContext()
{
    if (stream) (void)hipStreamSynchronize(stream);
    rts_scene_unref(scene); scene = nullptr;
    rts_hist_unref(hist); hist = nullptr;
    if (tstream) (void)hipStreamSynchronize(tstream);
    rts_gate_unref(gate); gate = nullptr;
    for (hipEvent_t e : ev) if (e) (void)hipEventDestroy(e);
    for (hipEvent_t e : ev_coop) if (e) (void)hipEventDestroy(e);
    if (cstream) { (void)hipStreamSynchronize(cstream); (void)hipStreamDestroy(cstream); }
    if (stream) (void)hipStreamDestroy(stream);
}

extern "C" int rts_create(const RtsParams* p, RtsHandle* out)
{
    if (!p || !out) { rts_set_error("rts_create: null argument"); return RTS_ERR_INVALID; }
    *out = nullptr;
    if (p->width == 0) { rts_set_error("rts_create: width must be >= 1"); return RTS_ERR_INVALID; }
    if ((uint64_t)p->width * p->width * p->width > 0xffffffffULL) {      // rayIndex is unsigned int, ray_tracer.cu:151
        rts_set_error("rts_create: W^3 must fit 32 bits (W <= 1625)"); return RTS_ERR_INVALID; }
    const uint32_t refr = p->max_refr > 0 ? 2u : 0u;                       // ">0 is forced to exactly 2", ray_tracer.cpp:604-605
    if (p->max_refl + refr > RTS_MAX_DEPTH) { rts_set_error("rts_create: max_refl + max_refr > %d", RTS_MAX_DEPTH); return RTS_ERR_UNSUPPORTED; }
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) { rts_set_error("rts_create: no HIP device (there is no CPU fallback)"); return RTS_ERR_NO_DEVICE; }
    if (p->device < 0 || p->device >= ndev) { rts_set_error("rts_create: device %d out of range (%d devices)", p->device, ndev); return RTS_ERR_INVALID; }
    RTS_HIP(hipSetDevice(p->device));
    RtsContext* c = new RtsContext();
    c->params = *p; c->params.max_refr = refr; c->depth = refr + p->max_refl; c->device = p->device;
    c->scene = new RtsScene(); c->scene->device = p->device;
    memset(&c->stats, 0, sizeof(c->stats));
    // two streams of different priority (=> different hardware queues): the long trace kernel on the low one, the many
    // short build/ordering/aggregation kernels on the high one so that they slot in while a trace kernel is running
    int prio_low = 0, prio_high = 0;
    (void)hipDeviceGetStreamPriorityRange(&prio_low, &prio_high);
    // every failure below: delete c (the destructor undoes whatever exists by then), set the error, return
    hipError_t e = hipStreamCreateWithPriority(&c->stream, hipStreamNonBlocking, prio_high);
    if (e != hipSuccess) { delete c; rts_set_error("hipStreamCreate: %s", hipGetErrorString(e)); return RTS_ERR_HIP; }
    c->gate = new RtsGate(); c->gate->refs = 1; c->gate->device = p->device;
    e = hipStreamCreateWithPriority(&c->gate->tstream, hipStreamNonBlocking, prio_low);
    if (e != hipSuccess) { delete c; rts_set_error("hipStreamCreate: %s", hipGetErrorString(e)); return RTS_ERR_HIP; }
    c->tstream = c->gate->tstream; c->tstream_now = c->tstream;
    for (int i = 0; i < 2; i++) { e = hipEventCreateWithFlags(&c->ev_coop[i], hipEventDisableTiming); if (e != hipSuccess) { delete c; rts_set_error("hipEventCreate: %s", hipGetErrorString(e)); return RTS_ERR_HIP; } }
    for (int i = 0; i < 9; i++) { e = hipEventCreate(&c->ev[i]); if (e != hipSuccess) { delete c; rts_set_error("hipEventCreate: %s", hipGetErrorString(e)); return RTS_ERR_HIP; } }
    e = c->pin.reserve(1, true);
    if (e != hipSuccess) { delete c; rts_set_error("hipHostMalloc / hipHostGetDevicePointer: %s", hipGetErrorString(e)); return RTS_ERR_HIP; }
    memset(c->pin.p, 0, sizeof(RtsPinned));
    hipDeviceProp_t prop; e = hipGetDeviceProperties(&prop, p->device);
    if (e != hipSuccess) { delete c; rts_set_error("hipGetDeviceProperties: %s", hipGetErrorString(e)); return RTS_ERR_HIP; }
    c->n_cu = prop.multiProcessorCount;
    rts_trace_preload();
    // experiment / test knobs, read ONCE PER HANDLE at creation (never per process: two handles of one process may differ): rts_tuning.h
    rts_tuning_read(&c->tune, rts_env);
    if (p->flags & RTS_FLAG_NO_PREFILTER) c->tune.use_pmask = false;
    c->hist = new RtsTileHist();
    *out = c;
    return RTS_OK;
}

// RTS_LAP=1: where the host side of rts_trace_pulse_begin spends its time, per section, summed per handle and printed by
// rts_destroy (stderr) -- the tool behind DESIGN.md's "what a slow run is"
struct RtsLapTimer {
    RtsContext* c; std::chrono::steady_clock::time_point t0; bool on;
    explicit RtsLapTimer(RtsContext* c_) : c(c_), on(rts_process_tuning().lap) { if (on) t0 = std::chrono::steady_clock::now(); }
    void lap(int k) { if (!on) return; const auto t1 = std::chrono::steady_clock::now(); c->lap_s[k] += std::chrono::duration<double>(t1 - t0).count(); c->lap_n[k]++; t0 = t1; }
};

// pulses begun and not yet ended or resolved, per device: a trace launch that will share the GPU with another pulse's kernels leaves block
// slots free for them (RtsTuning::grid_spare), a lone pulse takes the whole chip.  Moved by the transitions of RtsPulseState alone (rts_pulse_state.h).
static std::atomic<int> g_open_pulses[RTS_PULSE_SLOTS];
static std::mutex g_hist_mu;      // (re)allocation of a shared tile-cost history (RtsTileHist)

extern "C" int rts_destroy(RtsHandle c)
{
    if (!c) return RTS_OK;
    (void)hipSetDevice(c->device);
    (void)hipStreamSynchronize(c->stream);
    if (rts_process_tuning().lap && c->lap_n[0]) {
        static const char* names[8] = {"host prep", "upload + fill", "scene place", "buffers + tile order", "events + trace launch", "hipSetDevice", "resolve previous", ""};
        fprintf(stderr, "[rts lap] handle %p, %llu pulses begun, us per pulse:", (void*)c, (unsigned long long)c->lap_n[0]);
        for (int k = 0; k < 7; k++) fprintf(stderr, " %s %.1f |", names[k], c->lap_s[k] / (double)c->lap_n[0] * 1e6);
        fprintf(stderr, "\n");
    }
    c->pulse.abandon();
    rts_comm_cache_forget(c);
    delete c;
    return RTS_OK;
}

extern "C" int rts_link_handles(RtsHandle a, RtsHandle b)
{
    if (!a || !b || a == b) { rts_set_error("rts_link_handles: needs two distinct handles"); return RTS_ERR_INVALID; }
    if (a->device != b->device) { rts_set_error("rts_link_handles: handles live on different devices (%d, %d)", a->device, b->device); return RTS_ERR_INVALID; }
    if (a->gate == b->gate) return RTS_OK;
    if (a->gate->refs > 1 && b->gate->refs > 1) { rts_set_error("rts_link_handles: both handles already belong to (different) groups"); return RTS_ERR_INVALID; }
    if (a->pulse.open() || b->pulse.open()) { rts_set_error("rts_link_handles: a pulse is in flight"); return RTS_ERR_INVALID; }
    RtsContext* joiner = b->gate->refs == 1 ? b : a;     // the handle that is still alone adopts the other's trace stream
    RtsContext* host = joiner == b ? a : b;
    RTS_HIP(hipSetDevice(a->device));
    RTS_HIP(hipStreamSynchronize(joiner->tstream));
    rts_gate_unref(joiner->gate);      // (its only reference)
    joiner->gate = host->gate; joiner->gate->refs++; joiner->tstream = joiner->gate->tstream; joiner->tstream_now = joiner->tstream;
    return RTS_OK;
}

// The aggregation groups received rays by a packed (receiver, path) key of D x ceil(log2(targets + 1)) + ceil(log2(receivers))
// bits: one 64-bit sort when it fits, two or three stable passes when it does not (rts_post.hip: wide keys).  A configuration
// beyond 256 bits would be refused HERE, when the scene or the receivers are set, not in the middle of a pulse loop.
int check_key_width(uint32_t depth, uint32_t n_targets, uint32_t n_rx, const char* who)
{
    const RtsKeyPlan k = rts_key_plan_for(depth, n_targets, n_rx);
    if (!k.supported) {                               // (cannot happen within the other limits: 16 x 8 + 16 = 144 bits)
        rts_set_error("%s: %u targets x depth %u (max_refl + max_refr) with %u receivers needs a %u-bit (receiver, path) aggregation key; the limit is 256 bits",
                      who, n_targets, depth, n_rx, k.key_bits);
        return RTS_ERR_UNSUPPORTED;
    }
    return RTS_OK;
}

// ------------------------------------------------------------------------------------- receivers (the scene: rts_scene.hip)
extern "C" int rts_set_receivers(RtsHandle c, const RtsReceiverSphere* rx, uint32_t n_rx)
{
    CHECK_HANDLE(c);
    CHECK_CLOSED(c);
    if (n_rx && !rx) { rts_set_error("rts_set_receivers: null array"); return RTS_ERR_INVALID; }
    if (n_rx > 65535) { rts_set_error("rts_set_receivers: more than 65535 receivers"); return RTS_ERR_UNSUPPORTED; }
    RTS_TRY(check_key_width(c->depth, (uint32_t)c->scene->meshes.size(), n_rx, "rts_set_receivers"));
    std::vector<RtsRxDev> h(n_rx);
    for (uint32_t i = 0; i < n_rx; i++) {
        const RtsReceiverSphere& r = rx[i];
        const double vals[8] = { r.centre[0], r.centre[1], r.centre[2], r.radius, r.min_theta, r.max_theta, r.min_phi, r.max_phi };
        for (int k = 0; k < 8; k++) if (!std::isfinite(vals[k])) { rts_set_error("rts_set_receivers: receiver %u has a non-finite field", i); return RTS_ERR_INVALID; }
        // normalise_angle (ray_tracer.cu:53-57) walks in steps of 2 pi: keep the walk short
        if (std::fabs(r.min_theta) > 1e4 || std::fabs(r.max_theta) > 1e4 || std::fabs(r.min_phi) > 1e4 || std::fabs(r.max_phi) > 1e4) { rts_set_error("rts_set_receivers: receiver %u window angle magnitude > 1e4 rad", i); return RTS_ERR_INVALID; }
        h[i] = RtsRxDev{ r.centre[0], r.centre[1], r.centre[2], r.radius, r.min_theta, r.max_theta, r.min_phi, r.max_phi };
    }
    // A caller in a pulse loop sets the receivers before every pulse (the reference recomputes the capture spheres per pulse,
    // ray_tracer.cpp:894-918): an unchanged set costs nothing, a changed one is uploaded from pinned staging ON THE HANDLE'S
    // STREAM, ahead of the next trace -- no stream drain, no blocking copy (the handle has no pulse in flight here, so the
    // previous upload from the staging has long completed: its pulse was waited for).
    if (c->n_rx == n_rx && c->rx_host.size() == n_rx && (n_rx == 0 || memcmp(c->rx_host.data(), h.data(), sizeof(RtsRxDev) * n_rx) == 0)) return RTS_OK;
    if (n_rx <= 1024) {
        if (c->pin_rx.cap < n_rx) {
            if (c->pin_rx.p) RTS_HIP(hipStreamSynchronize(c->stream));
            RTS_HIP(c->pin_rx.reserve(std::max<uint32_t>(64u, n_rx), false));
        }
        if (c->d_rx.cap < (size_t)n_rx + 1) { RTS_HIP(hipStreamSynchronize(c->stream)); RTS_HIP(c->d_rx.reserve(n_rx + 1)); }
        if (n_rx) { memcpy(c->pin_rx.p, h.data(), sizeof(RtsRxDev) * n_rx); RTS_HIP(hipMemcpyAsync(c->d_rx.p, c->pin_rx.p, sizeof(RtsRxDev) * n_rx, hipMemcpyHostToDevice, c->stream)); }
    } else {
        RTS_HIP(hipStreamSynchronize(c->stream));
        RTS_HIP(c->d_rx.reserve(n_rx + 1));
        RTS_HIP(hipMemcpy(c->d_rx.p, h.data(), sizeof(RtsRxDev)*n_rx, hipMemcpyHostToDevice));
    }
    c->rx_host = h; c->n_rx = n_rx;
    return RTS_OK;
}

// ------------------------------------------------------------------------------------- launch constants
// sph_to_cart (ray_tracer.cu:132-139) and the launch-uniform part of ray_generation
// (ray_tracer.cu:155-156, 167-169 step factors, 173-175 Rot, 186-196 orth_vec and Rot1),
// evaluated once on the host in the reference's expression order.
static inline dvec3 host_sph_to_cart(double azi, double ele) { dvec3 c; c.x = std::cos(azi)*std::cos(ele); c.y = std::sin(azi)*std::cos(ele); c.z = std::sin(ele); return c; }

static void fill_launch_constants(RtsLaunchConsts& a, const RtsPulse& p, uint32_t W)
{
    const double spx = p.tx_span[0], spy = p.tx_span[1], spz = p.tx_span[2];
    const double dx = p.tx_dir[0], dy = p.tx_dir[1];
    a.ox = p.ray_origin[0]; a.oy = p.ray_origin[1]; a.oz = p.ray_origin[2];
    const dvec3 beamStart = host_sph_to_cart(-spx/2, -spy/2);
    const dvec3 beamEnd = host_sph_to_cart(spx/2, spy/2);
    a.bsx = beamStart.x; a.bsy = beamStart.y; a.bsz = beamStart.z;
    const dvec3 w1 = host_sph_to_cart(dx, dy);
    a.w1x = w1.x; a.w1y = w1.y; a.w1z = w1.z;
    a.stx = a.sty = a.stz = 0;
    if (W > 1) {
        a.stx = (((beamEnd.x*(1 + spz)) - beamStart.x)/(W - 1));
        a.sty = ((beamEnd.y - beamStart.y)/(W - 1));
        a.stz = ((beamEnd.z - beamStart.z)/(W - 1));
    }
    const double Rot[3][3] = {{std::cos(dx), -std::sin(dx), 0}, {std::sin(dx), std::cos(dx), 0}, {0, 0, 1}};
    for (int i = 0; i < 3; i++) for (int j = 0; j < 3; j++) a.rot[3*i + j] = Rot[i][j];
    dvec3 rotated; rotated.x = 0; rotated.y = 0; rotated.z = 0;
    rotated.x += Rot[0][1]; rotated.y += Rot[1][1]; rotated.z += Rot[2][1];
    const double on = std::sqrt(rotated.x*rotated.x + rotated.y*rotated.y + rotated.z*rotated.z);
    const dvec3 orth_vec = mk3(rotated.x/on, rotated.y/on, rotated.z/on);
    const double Rot1[3][3] = {
        {std::cos(dy) + orth_vec.x*orth_vec.x*(1 - std::cos(dy)), orth_vec.x*orth_vec.y*(1 - std::cos(dy)) + orth_vec.z*std::sin(dy), orth_vec.x*orth_vec.z*(1 - std::cos(dy)) - orth_vec.y*std::sin(dy)},
        {orth_vec.y*orth_vec.x*(1 - std::cos(dy)) - orth_vec.z*std::sin(dy), std::cos(dy) + orth_vec.y*orth_vec.y*(1 - std::cos(dy)), orth_vec.y*orth_vec.z*(1 - std::cos(dy)) + orth_vec.x*std::sin(dy)},
        {orth_vec.z*orth_vec.x*(1 - std::cos(dy)) + orth_vec.y*std::sin(dy), orth_vec.z*orth_vec.y*(1 - std::cos(dy)) - orth_vec.x*std::sin(dy), std::cos(dy) + orth_vec.z*orth_vec.z*(1 - std::cos(dy))}};
    for (int i = 0; i < 3; i++) for (int j = 0; j < 3; j++) a.rot1[3*i + j] = Rot1[i][j];
}

// Frame and extent of the primary-ray mask (RtsMaskFrame): b = direction of the beam's middle, (u, v) an orthonormal complement;
// the directions of a launch are the central projection of the (convex) lattice box, so the perspective coordinates of its
// eight corners bound those of every ray.
static void fill_mask_frame(RtsLaunchConsts& a, bool enable)
{
    RtsMaskFrame& f = a.mask; memset(&f, 0, sizeof(f));
    if (!enable || a.W < 2) return;
    dvec3 c[8]; dvec3 sum = mk3(0, 0, 0);
    for (int k = 0; k < 8; k++) {
        c[k] = rts_lattice_dir(a, (k & 1) ? a.W - 1 : 0, (k & 2) ? a.W - 1 : 0, (k & 4) ? a.W - 1 : 0);
        const double n = len3(c[k]); if (!(n > 0) || !std::isfinite(n)) return;
        c[k] = mk3(c[k].x / n, c[k].y / n, c[k].z / n); sum = add3(sum, c[k]);
    }
    const double sn = len3(sum); if (!(sn > 1e-6)) return;
    const dvec3 b = mk3(sum.x / sn, sum.y / sn, sum.z / sn);
    dvec3 ref = std::fabs(b.z) < 0.9 ? mk3(0, 0, 1) : mk3(1, 0, 0);
    dvec3 u = cross3(ref, b); const double un = len3(u); u = mk3(u.x / un, u.y / un, u.z / un);
    const dvec3 v = cross3(b, u);
    double u0 = 1e300, u1 = -1e300, v0 = 1e300, v1 = -1e300;
    for (int k = 0; k < 8; k++) {
        const double w = dot3(c[k], b); if (!(w > 0.5)) return;                  // beam wider than ~120 degrees: no mask
        const double uu = dot3(c[k], u) / w, vv = dot3(c[k], v) / w;
        u0 = std::min(u0, uu); u1 = std::max(u1, uu); v0 = std::min(v0, vv); v1 = std::max(v1, vv);
    }
    const double du = std::max(u1 - u0, 1e-9), dv = std::max(v1 - v0, 1e-9);
    u0 -= 0.002 * du; u1 += 0.002 * du; v0 -= 0.002 * dv; v1 += 0.002 * dv;   // rays exactly on the rim stay inside the bitmap
    f.bx = (float)b.x; f.by = (float)b.y; f.bz = (float)b.z; f.ux = (float)u.x; f.uy = (float)u.y; f.uz = (float)u.z; f.vx = (float)v.x; f.vy = (float)v.y; f.vz = (float)v.z;
    const double n_fit = std::floor(std::min(u1 - u0, v1 - v0) / RTS_MASK_MIN_CELL);
    if (!(n_fit >= 32.0)) return;                                                // beam narrower than 32 cells of the minimum size: no mask
    const uint32_t n = (uint32_t)std::min<double>(RTS_MASK_N, n_fit) & ~31u;     // whole 32-bit words per row
    f.u0 = (float)u0; f.v0 = (float)v0; f.inv_du = (float)(n / (u1 - u0)); f.inv_dv = (float)(n / (v1 - v0));
    f.n = n;
}

// Per-target placement constants of a pulse: inverse rotation, world bounds of the placed hierarchy, error slack.
static int fill_target_placement(const RtsContext* c, uint32_t t, RtsTargetDev& td)
{
    const RtsTargetMotion& m = c->motion[t]; const RtsBlasInfo& b = c->scene->blas[t];
    double R[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
    if (m.has_rotation) for (int k = 0; k < 9; k++) R[k] = m.rotation[k];
    for (int k = 0; k < 9; k++) if (!std::isfinite(R[k])) { rts_set_error("rts_trace_pulse: target %u has a non-finite rotation", t); return RTS_ERR_INVALID; }
    // the hierarchy is rigid: R must be a rotation up to rounding (the reference's are products of float-trig
    // axis rotations, ray_tracer.cpp:95-118, orthonormal to ~1e-7)
    double dev = 0;
    for (int i = 0; i < 3; i++) for (int j = 0; j < 3; j++) {
        double g = 0; for (int k = 0; k < 3; k++) g += R[3*k + i] * R[3*k + j];
        dev = std::max(dev, std::fabs(g - (i == j ? 1.0 : 0.0)));
    }
    if (!(dev < 1e-3)) { rts_set_error("rts_trace_pulse: target %u: rotation is not orthonormal (|R^T R - I| = %.3g); only rigid placements are supported", t, dev); return RTS_ERR_UNSUPPORTED; }
    const double det = R[0]*(R[4]*R[8] - R[5]*R[7]) - R[1]*(R[3]*R[8] - R[5]*R[6]) + R[2]*(R[3]*R[7] - R[4]*R[6]);
    const double id = 1.0 / det;
    td.rinv[0] = (R[4]*R[8] - R[5]*R[7]) * id; td.rinv[1] = (R[2]*R[7] - R[1]*R[8]) * id; td.rinv[2] = (R[1]*R[5] - R[2]*R[4]) * id;
    td.rinv[3] = (R[5]*R[6] - R[3]*R[8]) * id; td.rinv[4] = (R[0]*R[8] - R[2]*R[6]) * id; td.rinv[5] = (R[2]*R[3] - R[0]*R[5]) * id;
    td.rinv[6] = (R[3]*R[7] - R[4]*R[6]) * id; td.rinv[7] = (R[1]*R[6] - R[0]*R[7]) * id; td.rinv[8] = (R[0]*R[4] - R[1]*R[3]) * id;
    td.px = m.position[0]; td.py = m.position[1]; td.pz = m.position[2];
    td.root = b.root;
    // the horizon's tolerances (rts_horizon.hip); a placement that mirrors the mesh would swap the sides of every plane: no ray skips its walk then
    { const RtsHorizonMesh& hz = c->scene->hz[t]; td.hz_h0 = (float)hz.h0 * 1.000001f; td.hz_rho = det > 0.0 ? (float)hz.rho * 0.999999f : 0.0f; }      // (narrowed to the safe side each)
    // bounding sphere of the placed hierarchy: image of the local box centre, half diagonal stretched by the
    // rotation's deviation from orthonormality, padded by 1e-6 of the world scale
    double cl[3], half2 = 0, wc[3], wmax = 0;
    for (int i = 0; i < 3; i++) { cl[i] = 0.5 * b.lo[i] + 0.5 * b.hi[i]; const double h = 0.5 * (b.hi[i] - b.lo[i]); half2 += h * h; }
    for (int i = 0; i < 3; i++) { wc[i] = R[3*i]*cl[0] + R[3*i + 1]*cl[1] + R[3*i + 2]*cl[2] + m.position[i]; wmax = std::max(wmax, std::fabs(wc[i])); }
    double rad = std::sqrt(half2) * (1.0 + 2.0 * dev); wmax += rad;
    rad = rad * (1.0 + 1e-6) + wmax * 1e-6 + 1e-30;
    td.cx = wc[0]; td.cy = wc[1]; td.cz = wc[2]; td.r2 = rad * rad;
    // Extra origin slack of the target-space slab test.  What it has to cover is the one error that scales with the WORLD
    // coordinates: the exact test runs on vw = fl(fl(R v) + p), which is off the ideal R v + p by <= 2^-53 |vw| per
    // coordinate (one rounding of the final sum; the partial sums live at target scale), i.e. <= sqrt(3) 2^-53 wmax along a
    // target axis = 1.2e-9 m at Earth-centred coordinates (6.4e6 m).  Everything else -- the mapping R^-1 (o - p), o - p
    // itself (Sterbenz-exact or correctly rounded), the f32 narrowing of the mapped origin -- is relative to |o - p| and
    // is inside the 3e-7 |o'| of rts_slab_setup.  2^-49 wmax is that bound times 9.  (Round 1 used 4e-9 wmax: harmless
    // near the origin, but 2.6 cm on every slab plane of a mesh of 10-30 cm triangles at 6.4e6 m.)
    td.ew = (float)(wmax * c->tune.ew_rel) + 1.0e-30f;
    if (b.root < 0 || !std::isfinite(td.cx + td.cy + td.cz + td.r2)) td.root = -1;
    return RTS_OK;
}

// The shared tile-cost history holds n_hist records: left alone when it already does, else (re)allocated, zeroed and forgotten.
static int rts_hist_ensure(RtsContext* c, uint32_t n_hist)
{
    if (c->hist->n == n_hist) return RTS_OK;
    std::lock_guard<std::mutex> lk(g_hist_mu);      // (handles that share the history may be driven from different threads)
    RTS_HIP(hipDeviceSynchronize()); RTS_HIP(c->hist->d.reserve(n_hist)); RTS_HIP(hipMemset(c->hist->d.p, 0, sizeof(uint32_t) * n_hist));      // (blocking, once: the table may be shared with handles on other streams)
    c->hist->n = n_hist; c->hist->any = false; c->tile_cost_pending = false;
    return RTS_OK;
}

// The zero block and, behind it, room for the primary-ray mask; p_counters points at the block's 24 counters.
static int rts_zero_block_reserve(RtsContext* c)
{
    RTS_HIP(c->d_tile_ctr.reserve(RTS_ZERO_WORDS + RTS_MASK_WORDS + 64));
    c->p_counters = reinterpret_cast<unsigned long long*>(c->d_tile_ctr.p + RTS_OFF_COUNTERS);
    return RTS_OK;
}

// The eight per-pulse buffers hold at least the given element counts (rts_launch_plan.h: rts_launch_sizes).
static int rts_launch_buffers_reserve(RtsContext* c, const RtsLaunchSizes& s)
{
    RTS_HIP(c->d_recv.reserve(s.recv)); RTS_HIP(c->d_dir_hist.reserve(s.dir_hist)); RTS_HIP(c->d_child.reserve(s.child));
    RTS_HIP(c->d_stack_ovf.reserve(s.stack_ovf)); RTS_HIP(c->d_block_counters.reserve(s.block_counters));
    RTS_HIP(c->d_all.reserve(s.all)); RTS_HIP(c->d_hit_prim.reserve(s.hit_prim)); RTS_HIP(c->d_hit_t.reserve(s.hit_t));
    return RTS_OK;
}

// the cooperative kernel's rows of the per-thread slabs
static uint32_t rts_coop_threads(const RtsContext* c) { return c->tune.coop_frac > 0.0 ? c->tune.coop_grid_max * RTS_BLOCK : 0u; }

// Device buffers of a launch of up to n launch indices (grown, never shrunk).  Also the first touch of the big slabs:
// doing it before the first pulse keeps multi-GB hipMalloc calls out of a caller's timed or latency-critical region.
extern "C" int rts_reserve(RtsHandle c, uint64_t n_rays)
{
    CHECK_HANDLE(c);
    const uint64_t W3 = rts_lattice_size(c->params.width);
    const uint64_t n = std::min<uint64_t>(n_rays ? n_rays : W3, W3);
    if (n * rts_chains(c->params.max_refr) > 0xfffffff0ULL) { rts_set_error("rts_reserve: rays x chains exceeds 2^32"); return RTS_ERR_UNSUPPORTED; }
    // upper bounds of any launch's grid: threads of the child slab, threads of the overflow stack, blocks of both kernels
    const RtsLaunchSizes sz = rts_launch_sizes(n, (uint64_t)c->n_cu * 64 * RTS_BLOCK, (uint64_t)c->n_cu * 1024, rts_coop_threads(c), (uint64_t)c->n_cu * 64 + c->tune.coop_grid_max,
                                               c->params.max_refl, c->params.max_refr, (c->params.flags & RTS_FLAG_KEEP_ALL_RAYS) != 0);
    RTS_TRY(rts_launch_buffers_reserve(c, sz));
    RTS_TRY(rts_zero_block_reserve(c));
    const size_t n_tiles = (size_t)rts_wave_tiles(n);
    RTS_HIP(c->d_tile_cost.reserve(n_tiles)); RTS_HIP(c->d_tile_key.reserve(n_tiles)); RTS_HIP(c->d_tile_order.reserve(n_tiles));
    RTS_TRY(rts_hist_ensure(c, (uint32_t)rts_wave_tiles(W3)));
    // touch the two slabs the trace kernel writes sparsely, so that their pages exist before the first launch
    RTS_HIP(hipMemsetAsync(c->d_recv.p, 0, sizeof(RtsEndRecord) * sz.recv, c->stream));
    RTS_HIP(hipMemsetAsync(c->d_dir_hist.p, 0, sizeof(float) * c->d_dir_hist.cap, c->stream));
    RTS_HIP(hipStreamSynchronize(c->stream));
    return RTS_OK;
}

// ------------------------------------------------------------------------------------- launch
extern "C" int rts_trace_pulse(RtsHandle c, const RtsPulse* p)
{
    int rc = rts_trace_pulse_begin(c, p);
    return rc != RTS_OK ? rc : rts_trace_pulse_end(c);
}

// What the steps of rts_trace_pulse_begin hand on to each other: the resolved range, the ordinary kernel's grid and arguments.
struct RtsPulseLaunch {
    RtsRayRange r; uint32_t n = 0, grid = 0;
    bool moved = false, shared_gpu = false, keep_all = false, count_trav = false, pre_filter = false;
    RtsTraceArgs a;
    const char* tl_path = nullptr; size_t cnt_tl = 0;      // debug (RTS_TIMELINE): where this launch's timeline goes and its length
};

// The pulse's range arguments against the lattice and the handle's dealt list (rts_launch_plan.h: rts_ray_range); writes nothing.
static RtsRayRange pulse_ray_range(const RtsContext* c, const RtsPulse* p)
{
    const RtsRangeArgs q = {p->ray_first, p->ray_count, rts_lattice_size(c->params.width), p->interleave_tile, p->interleave_parts, p->interleave_part, RTS_INTERLEAVE_LIST,
                            c->il_list_tile, c->il_list_n, c->il_list_last, c->il_list_gen};
    return rts_ray_range(q);
}

// The failed check of a range as the caller reads it.
static int pulse_range_error(const RtsContext* c, const RtsPulse* p, const RtsRayRange& r)
{
    switch (r.err) {
    case RTS_RANGE_OK: return RTS_OK;
    case RTS_RANGE_LIST_TILE: rts_set_error("rts_trace_pulse: RTS_INTERLEAVE_LIST with tile %u, but the handle's tile list has %u tiles of %u launch indices (rts_set_tile_list)", p->interleave_tile, c->il_list_n, c->il_list_tile); break;
    case RTS_RANGE_BAD_INTERLEAVE: rts_set_error("rts_trace_pulse: bad interleave (tile %u, part %u of %u)", r.il_tile, r.il_part, r.il_parts); break;
    case RTS_RANGE_OUTSIDE: rts_set_error("rts_trace_pulse: ray range [%llu, +%llu) outside W^3 = %llu", (unsigned long long)r.first, (unsigned long long)r.span, (unsigned long long)rts_lattice_size(c->params.width)); break;
    case RTS_RANGE_LIST_BEYOND: rts_set_error("rts_trace_pulse: the handle's tile list names tile %u, the range has %llu tiles of %u launch indices", c->il_list_last, (unsigned long long)r.range_tiles, r.il_tile); break;
    }
    return RTS_ERR_INVALID;
}

// Forgets the previous pulse's results and notes the transmitter of this one (rts_finalise_patterns: its position and boresight).
static void pulse_reset_results(RtsContext* c, const RtsPulse* p)
{
    c->res.forget();
    for (int k = 0; k < 3; k++) c->pulse_org[k] = p->ray_origin[k];
    c->pulse_dir[0] = p->tx_dir[0]; c->pulse_dir[1] = p->tx_dir[1]; c->pulse_traced = true;
}

// Leaves the pulse's motion on the handle and says whether a target moved; if one did, the placements are in the pinned staging
// and bvh_valid is false until pulse_scene_place has enqueued them.
static int pulse_stage_motion(RtsContext* c, const RtsPulse* p, bool* moved_out)
{
    const uint32_t n_targets = (uint32_t)c->scene->meshes.size();
    bool moved = !c->bvh_valid;
    if (p->motion) {
        if (!c->motion_valid || memcmp(c->motion.data(), p->motion, sizeof(RtsTargetMotion)*n_targets) != 0) moved = true;
        if (n_targets) memcpy(c->motion.data(), p->motion, sizeof(RtsTargetMotion)*n_targets);
        c->motion_valid = true;
    } else if (!c->motion_valid) {
        for (auto& m : c->motion) memset(&m, 0, sizeof(m));
        c->motion_valid = true; moved = true;
    }
    c->stats.bvh_rebuilt = 0;
    *moved_out = moved;
    if (!moved) return RTS_OK;
    for (uint32_t t = 0; t < n_targets; t++) for (int k = 0; k < 3; k++)
        if (!std::isfinite(c->motion[t].position[k]) || !std::isfinite(c->motion[t].velocity[k])) { rts_set_error("rts_trace_pulse: target %u has a non-finite position/velocity", t); return RTS_ERR_INVALID; }
    if (n_targets > 256) { rts_set_error("rts_trace_pulse: more than 256 targets"); return RTS_ERR_UNSUPPORTED; }
    // pinned staging is safe to rewrite: every earlier upload precedes the previous launch's trace kernel, whose
    // completion the host already waited for (received-count readback)
    RtsTargetDev* td = c->pin.p->td;
    for (uint32_t t = 0; t < n_targets; t++) {
        td[t].reflCoeff = c->scene->meshes[t].refl_coeff; td[t].vx = c->motion[t].velocity[0]; td[t].vy = c->motion[t].velocity[1]; td[t].vz = c->motion[t].velocity[2];
        td[t].tri_base = c->scene->meshes[t].tri_base; td[t].perface_normals = c->scene->meshes[t].perface ? 1u : 0u; td[t].refrIndex = c->scene->meshes[t].refr_index;
        int rc = fill_target_placement(c, t, td[t]); if (rc != RTS_OK) { c->bvh_valid = false; c->motion_valid = false; return rc; }
        c->pin.p->motion[t] = c->motion[t];
    }
    c->bvh_valid = false;                                     // (until the upload and the placement kernels have been enqueued: an early return in between must not leave the device with the old placement)
    return RTS_OK;
}

// Leaves the pulse's launch constants in c->last_lc: ray generation, range and interleave, the division by W, the mask frame and
// the f32 constants of the pre-filter.
static void pulse_fill_constants(RtsContext* c, const RtsPulse& p, const RtsRayRange& r, bool pre_filter)
{
    const uint32_t W = c->params.width;
    RtsLaunchConsts& lc = c->last_lc; memset(&lc, 0, sizeof(lc));
    fill_launch_constants(lc, p, W);
    lc.ray_first = r.first; lc.W = W; lc.il_tile = r.il_tile; lc.il_parts = r.il_parts; lc.il_part = r.il_part; lc.il_list = r.il_list ? c->d_il_list.p : nullptr;
    const RtsDivMagic d = rts_div_magic(W); lc.w_magic = d.magic; lc.w_more = d.more;
    fill_mask_frame(lc, pre_filter && c->scene->n_prims > 0);
    for (int k = 0; k < 3; k++) { lc.f_bs[k] = (float)(&lc.bsx)[k]; lc.f_st[k] = (float)(&lc.stx)[k]; }
    for (int i = 0; i < 3; i++) for (int j = 0; j < 3; j++) lc.f_m[3 * i + j] = (float)(lc.rot1[3 * i] * lc.rot[j] + lc.rot1[3 * i + 1] * lc.rot[3 + j] + lc.rot1[3 * i + 2] * lc.rot[6 + j]);
}

static uint32_t* pulse_mask_words(const RtsContext* c) { return c->d_tile_ctr.p + RTS_ZERO_WORDS; }      // the primary-ray mask, behind the zero block

// Leaves enqueued: the pulse's parameters in ONE upload -- launch constants, and when a target moved the placements behind them --
// and ONE fill: the draw counters of both kernels, the order's head words and bins, the launch's 16 counters and, behind them,
// when this pulse has one, the primary-ray mask.
static int pulse_upload_and_fill(RtsContext* c, bool moved)
{
    const uint32_t n_targets = (uint32_t)c->scene->meshes.size(); const RtsMaskFrame& mask = c->last_lc.mask;
    c->pin.p->lc = c->last_lc;
    RTS_HIP(hipMemcpyAsync(c->d_params.p, &c->pin.p->lc, moved && n_targets ? offsetof(RtsPinned, td) + sizeof(RtsTargetDev) * n_targets : sizeof(RtsLaunchConsts), hipMemcpyHostToDevice, c->stream));
    RTS_TRY(rts_zero_block_reserve(c));
    RTS_HIP(hipMemsetAsync(c->d_tile_ctr.p, 0, sizeof(uint32_t) * (((RTS_ZERO_WORDS + (mask.n ? (size_t)mask.n * mask.n / 32u + 1u : 0u)) + 63u) & ~(size_t)63u), c->stream));      // (a whole number of 256-byte pieces: the runtime splits an odd-sized fill into two kernels)
    return RTS_OK;
}

// Leaves the placement (a target moved) and the primary-ray mask enqueued -- one pass over the leaves for both -- and bvh_valid true.
static int pulse_scene_place(RtsContext* c, bool moved)
{
    RTS_TRY(rts_scene_place(c, c->last_lc, moved, pulse_mask_words(c)));
    if (moved) { RTS_STAGE(c, "scene_place"); c->bvh_valid = true; c->stats.bvh_rebuilt = 1; }
    RTS_HIP(hipEventRecord(c->ev[1], c->stream));
    return RTS_OK;
}

// Leaves L.a filled from the handle (all but the tile order and the timeline) and the per-pulse buffers reserved; the keep-all hit
// records are cleared.
static int pulse_args_and_buffers(RtsContext* c, RtsPulseLaunch& L)
{
    RtsTraceArgs& a = L.a; memset(&a, 0, sizeof(a));
    const uint32_t n = L.n; const RtsLaunchConsts& lc = c->last_lc; hipStream_t st = c->stream;
    a.lc = c->p_lc;
    a.ray_first = L.r.first; a.n_rays = n; a.W = c->params.width; a.max_refl = c->params.max_refl; a.smooth = c->params.interpolate_smooth ? 1u : 0u;
    a.n_prims = c->scene->n_prims; a.n_targets = (uint32_t)c->scene->meshes.size(); a.n_rx = c->n_rx; a.keep_all = L.keep_all ? 1u : 0u;
    a.max_refr = c->params.max_refr; a.rows = a.max_refr ? c->params.max_refl + 3 : 1;      // (output rows per launch index: not rts_hit_rows)
    if ((uint64_t)n * rts_chains(a.max_refr) > 0xfffffff0ULL) { rts_set_error("rts_trace_pulse: rays x chains exceeds 2^32"); return RTS_ERR_UNSUPPORTED; }
    a.total_threads = L.grid * RTS_BLOCK;
    a.coop_spread = c->tune.coop_spread;
    a.coop_walk_steps_lo = std::min(c->tune.coop_walk_steps_lo, c->tune.coop_walk_steps);
    a.coop_walk_steps = c->tune.coop_walk_steps; a.coop_min_cost = c->tune.coop_walk_steps ? std::min<uint32_t>(c->tune.coop_floor, 1875u) : 0u;      // (nothing shorter than 50 us is looked at; RTS_COOP_STEPS=0: every tile is flagged)
    a.slab_threads = a.total_threads + rts_coop_threads(c);
    const RtsLaunchSizes sz = rts_launch_sizes(n, a.total_threads, a.total_threads, rts_coop_threads(c), (uint64_t)L.grid + c->tune.coop_grid_max, a.max_refl, a.max_refr, L.keep_all);
    RTS_TRY(rts_launch_buffers_reserve(c, sz));
    if (L.keep_all) {      // (the buffers' last element is spare)
        rts_fill_i32(st, c->d_hit_prim.p, -2, sz.hit_prim - 1);
        RTS_HIP(hipMemsetAsync(c->d_hit_t.p, 0, sizeof(float) * (sz.hit_t - 1), st));
    }
    a.pmask = lc.mask.n ? pulse_mask_words(c) : nullptr; a.pre_filter = L.pre_filter ? 1u : 0u;
    a.nodes4 = c->scene->d_nodes4.p; a.nodes4v = c->tune.node_versions ? c->scene->d_nodes4v.p : nullptr; a.stack_lds = c->tune.stack_lds; a.leaves = c->d_leaves.p; a.tri_nidx = c->scene->d_tri_nidx.p; a.normals = c->d_normals_world.p;
    a.targets = c->p_targets; a.rx = c->d_rx.p;
    a.recv_records = c->d_recv.p; a.all_records = c->d_all.p; a.counters = c->p_counters; a.block_counters = c->d_block_counters.p; a.dir_hist = c->d_dir_hist.p;
    a.hit_prim = c->d_hit_prim.p; a.hit_t = c->d_hit_t.p; a.stack_ovf = c->d_stack_ovf.p; a.child = c->d_child.p;
    a.rx_window_screen = c->tune.rx_window_screen ? 1u : 0u;
    a.horizon = (c->params.flags & RTS_FLAG_NO_HORIZON) ? 0u : (c->params.flags & RTS_FLAG_NO_HORIZON_SECTORS) ? 1u : 2u;
    a.coop_versions = c->tune.coop_versions ? 1u : 0u;
    a.tile_ctr = c->d_tile_ctr.p;
    return RTS_OK;
}

// Leaves the longest-tile-first order built from what this handle's earlier launches measured per global tile (rts_post.hip) and
// this launch's cost records cleared -- or, for a launch whose costs are not recorded (unaligned, or a single sweep), neither.
static int pulse_tile_order(RtsContext* c, RtsPulseLaunch& L)
{
    RtsTraceArgs& a = L.a;
    const RtsLaunchShape s = rts_launch_shape(L.n, L.r.first, L.r.il_tile, L.r.il_parts, L.r.il_part, rts_lattice_size(c->params.width));
    const uint32_t n_tiles = s.n_tiles, resident_waves = L.grid * (RTS_BLOCK / RTS_WTILE);
    a.batch_dead = s.aligned ? (uint32_t)c->tune.batch_dead : 0u;      // (a wave tile must be 64 CONSECUTIVE launch indices for the tile-level screen: rts_tile_maybe)
    if (!(c->tune.tile_lpt && s.aligned && n_tiles > resident_waves)) { c->tile_cost_pending = false; c->tile_last_valid = false; return RTS_OK; }
    RTS_TRY(rts_hist_ensure(c, s.n_hist));
    if (c->tile_cost_pending || c->hist->any) {
        c->coop_big_now = (L.r.il_parts > 1 && !L.shared_gpu && c->tune.coop_big_part > c->tune.coop_big) ? c->tune.coop_big_part : c->tune.coop_big;
        RTS_TRY(rts_tile_order_build(c, c->tile_cost_sig, c->tile_cost_pending, s.sig, n_tiles, resident_waves));
        a.tile_order = c->d_tile_order.p; a.tile_head = c->tune.coop_frac > 0.0 ? c->d_tile_ctr.p + RTS_OFF_HEAD + 2 : nullptr; a.tile_head_all = a.tile_head; c->hist->any = true;
        a.tile_live = c->d_tile_ctr.p + RTS_OFF_LIVE;      // (written by the order build)
    }
    const bool merged_all = c->tile_cost_pending && rts_wave_tiles(c->tile_cost_sig[0]) >= n_tiles && c->d_tile_cost.cap >= n_tiles;      // k_tile_merge read AND cleared the records
    RTS_HIP(c->d_tile_cost.reserve(n_tiles));
    if (!merged_all) RTS_HIP(hipMemsetAsync(c->d_tile_cost.p, 0, sizeof(uint32_t) * n_tiles, c->stream));
    a.tile_cost = c->d_tile_cost.p;
    c->tile_cost_pending = true; memcpy(c->tile_cost_sig, s.sig, sizeof(s.sig)); memcpy(c->tile_last_sig, s.sig, sizeof(s.sig)); c->tile_last_valid = true;
    return RTS_OK;
}

// Leaves the debug timeline of this launch zeroed and named in L.a: RTS_TIMELINE (counting build: blocks and tiles, dumped by
// pulse_timeline_dump) or RTS_TIMELINE_BLOCKS (product build: when every block started and ended, printed by rts_trace_pulse_end).
static int pulse_timelines(RtsContext* c, RtsPulseLaunch& L)
{
    const size_t blocks2 = (size_t)L.grid * 2;
    RtsLaunchTuning lt; if (L.count_trav) rts_tuning_read(&lt, rts_env);
    L.tl_path = lt.timeline;
    L.cnt_tl = blocks2 + 2 * (size_t)rts_wave_tiles(L.n);          // [grid][2] block ticks, [tiles] durations, [tiles] start ticks
    c->tl_blocks = 0;
    const size_t words = L.tl_path ? L.cnt_tl + 1 : (!L.count_trav && c->tune.timeline_blocks) ? blocks2 + 1 : 0;
    if (!words) return RTS_OK;
    RTS_HIP(c->d_timeline.reserve(words)); RTS_HIP(hipMemsetAsync(c->d_timeline.p, 0, sizeof(unsigned long long) * words, c->stream)); L.a.timeline = c->d_timeline.p;
    if (!L.tl_path) c->tl_blocks = L.grid;
    return RTS_OK;
}

// Leaves both trace kernels enqueued on the stream chosen for this pulse (c->tstream_now), bracketed by ev[2] / ev[3], and the
// handle's own stream waiting for them.
static int pulse_launch(RtsContext* c, RtsPulseLaunch& L)
{
    RtsTraceArgs& a = L.a; hipStream_t st = c->stream;
    RTS_STAGE(c, "pre-trace");
    // The trace kernel's stream: the handle's low-priority trace stream when other pulses share the GPU (their short kernels then get
    // in beside it), the handle's OWN stream when none does -- a pulse on its own is one dependent chain, and every hop between two
    // streams costs it 17-25 us of event hand-over (profiles/r04_inflight1_pulse_timeline.log: two hops per pulse)
    c->tstream_now = (c->tune.trace_own_stream && !L.shared_gpu && c->gate->refs.load() == 1) ? st : c->tstream;
    if (c->tstream_now != st) {
        RTS_HIP(hipEventRecord(c->ev[8], st));                   // scene + per-pulse buffers of this handle are ready
        RTS_HIP(hipStreamWaitEvent(c->tstream_now, c->ev[8], 0));
    }
    RTS_HIP(hipEventRecord(c->ev[2], c->tstream_now));
    // the cooperative kernel (tiles at the head of the cost order, one launch index per wave): its grid follows the head count
    // of the handle's previous order build (the count of THIS build is on the device; a grid too small or too large only costs
    // balance, every unit is drawn from a queue); it came home with that launch's counters
    // Whether there is a cooperative kernel at all is decided HERE, from that earlier count (both kernels must agree on
    // who traces the head of the order): no head last time -> none now, and the ordinary kernel traces every tile.
    unsigned coop_grid = 0;
    if (a.tile_head) {
        if (c->hist->head_hint_valid) c->n_head_hint = c->hist->head_hint;      // (the latest head count of ANY handle that shares the history)
        const bool grouped = a.nodes4v && a.coop_versions && !L.keep_all && !a.max_refr;      // (rts_trace_dispatch: the cooperative kernel that walks the octant versions holds 64 / RTS_COOP_GROUP rays per unit)
        coop_grid = rts_coop_grid(c->n_head_hint, grouped, c->tune.coop_grid_max);
        if (coop_grid == 0) a.tile_head = nullptr;
        c->last_args = a;
    }
    if (c->tune.debug_coop) fprintf(stderr, "[rts] launch: n_rays %u grid %u head hint %u coop grid %u walk-steps threshold %u min cost %u order %d\n", L.n, L.grid, c->n_head_hint, coop_grid, a.coop_walk_steps, a.coop_min_cost, a.tile_order ? 1 : 0);
    c->last_coop_grid = coop_grid;
    int rc = rts_trace_launch(c, a, L.count_trav, coop_grid);
    if (rc != RTS_OK) return rc;
    RTS_STAGE(c, "k_trace");
    RTS_HIP(hipEventRecord(c->ev[3], c->tstream_now));
    if (c->tstream_now != st) RTS_HIP(hipStreamWaitEvent(st, c->ev[3], 0));      // everything later on this handle's stream follows its trace
    return RTS_OK;
}

// debug (RTS_TIMELINE): waits for the launch and writes its block / tile timeline to the named file
static int pulse_timeline_dump(RtsContext* c, const RtsPulseLaunch& L)
{
    RTS_HIP(hipStreamSynchronize(c->stream));
    std::vector<unsigned long long> h(L.cnt_tl + 2);
    h[0] = L.grid; h[1] = rts_wave_tiles(L.n);
    RTS_HIP(hipMemcpy(h.data() + 2, c->d_timeline.p, sizeof(unsigned long long) * L.cnt_tl, hipMemcpyDeviceToHost));
    if (FILE* f = fopen(L.tl_path, "wb")) { fwrite(h.data(), sizeof(unsigned long long), h.size(), f); fclose(f); }
    return RTS_OK;
}

// Everything of a pulse up to and including the trace kernel, left in flight on the handle's stream.
// (the RtsLapTimer sections: rts_destroy's names[])
extern "C" int rts_trace_pulse_begin(RtsHandle c, const RtsPulse* p)
{
    if (!c) { rts_set_error("null handle"); return RTS_ERR_INVALID; }
    RtsLapTimer lt(c);
    CHECK_HANDLE(c);
    lt.lap(5);
    if (!p) { rts_set_error("rts_trace_pulse: null pulse"); return RTS_ERR_INVALID; }
    if (c->pulse.open()) { rts_set_error("rts_trace_pulse_begin: the previous pulse of this handle was begun but not ended"); return RTS_ERR_INVALID; }
    CHECK_CLOSED(c);
    lt.lap(6);
    RtsPulseLaunch L;
    L.r = pulse_ray_range(c, p);
    // (a dealt list that names a tile beyond the range is reported AFTER the motion is staged: a bad motion is the error of a call
    // that has both wrong, and the failed call leaves motion_valid and bvh_valid as staged)
    if (L.r.err != RTS_RANGE_OK && L.r.err != RTS_RANGE_LIST_BEYOND) return pulse_range_error(c, p, L.r);
    pulse_reset_results(c, p);
    RTS_HIP(hipEventRecord(c->ev[0], c->stream));
    RTS_TRY(pulse_stage_motion(c, p, &L.moved));
    if (L.r.err != RTS_RANGE_OK) return pulse_range_error(c, p, L.r);
    L.n = (uint32_t)L.r.count;
    c->ray_first = L.r.first; c->n_rays = L.n;
    L.keep_all = (c->params.flags & RTS_FLAG_KEEP_ALL_RAYS) != 0;
    L.count_trav = (c->params.flags & RTS_FLAG_COUNT_TRAVERSAL) != 0;
    // the trace kernel's blocks are persistent and four of them fill a CU's register file: a launch that shares the GPU leaves a few
    // block slots free so that the short kernels of the neighbouring pulses (other streams) are not locked out for the whole launch
    std::atomic<int>& open_here = rts_pulse_slot(g_open_pulses, c->device);
    L.shared_gpu = c->tune.grid_spare_forced || open_here.load() > 0;
    L.grid = rts_trace_grid(L.n, c->n_cu, c->tune.grid_mult, L.shared_gpu ? c->tune.grid_spare : 0);
    L.pre_filter = c->tune.use_pmask && !c->pre_dense;           // (a launch where most rays hit pays for the filter and skips nothing)
    pulse_fill_constants(c, *p, L.r, L.pre_filter);
    lt.lap(0);
    RTS_TRY(pulse_upload_and_fill(c, L.moved));
    lt.lap(1);
    RTS_TRY(pulse_scene_place(c, L.moved));
    lt.lap(2);
    RTS_TRY(pulse_args_and_buffers(c, L));
    RTS_TRY(pulse_tile_order(c, L));
    RTS_TRY(pulse_timelines(c, L));
    c->last_args = L.a;
    lt.lap(3);
    RTS_TRY(pulse_launch(c, L));
    lt.lap(4);
    // (the eight counters were written into the pinned block by k_sum_counters itself: no copy)
    c->pulse.begin(open_here);
    return L.tl_path ? pulse_timeline_dump(c, L) : RTS_OK;
}

// counters of a finished launch -> the handle's statistics and the hints its next launch uses
static void rts_pulse_account(RtsContext* c, const unsigned long long* cnt)
{
    const uint32_t n = c->n_rays;
    RtsStats& s = c->stats;
    s.rays = n; s.segments = cnt[1]; s.shaded = cnt[2]; s.received = cnt[0]; s.node_visits = cnt[3]; s.tri_tests = cnt[4]; s.stack_overflows = (uint32_t)cnt[5];
    s.n_prims = c->scene->n_prims; s.n_nodes = c->scene->n_nodes;
    s.walked_segments = cnt[11]; s.cost_records_dropped = (uint32_t)cnt[12];
    if (c->tune.debug_coop && (cnt[12] || cnt[14])) fprintf(stderr, "[rts] clocks: %llu cost records dropped; shader clock ran backwards on %llu tiles (XCC mask 0x%llx)\n", cnt[12], cnt[14] & 0x00ffffffffffffffULL, cnt[14] >> 56);
    s.coop_tiles = c->last_coop_grid ? (uint32_t)std::min<unsigned long long>(std::min<unsigned long long>(cnt[7], rts_wave_tiles(n)), 16384ull) : 0u;      // (the bounds k_trace applies to the order's head count)
    c->pre_dense = 2 * s.shaded > (uint64_t)n;                      // next launch of this handle: pre-filter only if most launch indices hit nothing
    s.ms_scene = s.ms_trace = s.ms_compact = s.ms_aggregate = 0;
    c->stats_pending = true;
    c->recv_hint = cnt[0]; c->recv_hint_valid = true;      // (the next pulse's choices -- speculate at all, one kernel or seven -- follow THIS pulse's count, not the handle's first)
}

// the counters of a finished launch, once the host has waited for its stream: the launch's own failures, then the received count and
// the order's head count (sizes the next cooperative grid of the handle and of those that share its history)
static int rts_counters_home(RtsContext* c, const unsigned long long* cnt)
{
    if (cnt[13]) { rts_set_error("rts_trace_pulse: %llu counter rows of the launch were never written by their blocks (counting build)", cnt[13]); return RTS_ERR_HIP; }
    if (cnt[6]) { rts_set_error("rts_trace_pulse: traversal stack overflow / malformed BVH guard tripped on %llu waves", cnt[6]); return RTS_ERR_HIP; }
    c->res.n_recv = cnt[0]; c->n_head_hint = (uint32_t)cnt[7]; c->hist->head_hint = c->n_head_hint; c->hist->head_hint_valid = true;
    return RTS_OK;
}

// RTS_TIMELINE_BLOCKS: the launch as a bulk (every block resident) and a tail (rts_get_block_timeline; profiles/r05h_batch_launch.log)
static void pulse_timeline_summary(RtsContext* c)
{
    std::vector<unsigned long long> h((size_t)c->tl_blocks * 2);
    (void)hipMemcpy(h.data(), c->d_timeline.p, sizeof(unsigned long long) * h.size(), hipMemcpyDeviceToHost);
    std::vector<unsigned long long> s0, s1; for (uint32_t i = 0; i < c->tl_blocks; i++) { s0.push_back(h[2 * i]); s1.push_back(h[2 * i + 1]); }
    std::sort(s0.begin(), s0.end()); std::sort(s1.begin(), s1.end());
    const size_t m = s0.size(); const unsigned long long t0 = s0[0];
    const size_t q[8] = {0, m / 2, m - 1, 0, m / 10, m / 2, m * 9 / 10, m - 1};
    for (int k = 0; k < 8; k++) c->tl_summary[k] = (double)((k < 3 ? s0[q[k]] : s1[q[k]]) - t0) / 100.0;      // us after the first block's start (100 MHz counter)
    c->tl_summary[8] = (double)m;
    if (c->tune.debug_coop) fprintf(stderr, "[rts] blocks of handle %p (us after the first start): start p50 %.1f max %.1f | end min %.1f p10 %.1f p50 %.1f p90 %.1f max %.1f\n", (void*)c,
                               c->tl_summary[1], c->tl_summary[2], c->tl_summary[3], c->tl_summary[4], c->tl_summary[5], c->tl_summary[6], c->tl_summary[7]);
}

// debug (RTS_DEBUG_COOP): what the head rule of this launch's order build saw (blocking read-backs)
static void pulse_debug_dump(RtsContext* c, const unsigned long long* cnt)
{
    unsigned long long sums[2] = {0, 0};
    (void)hipMemcpy(&sums[0], c->d_order_sum.p, sizeof(unsigned long long), hipMemcpyDeviceToHost);
    (void)hipMemcpy(&sums[1], c->d_tile_ctr.p + RTS_OFF_HEAD, sizeof(unsigned long long), hipMemcpyDeviceToHost);
    uint32_t live_w = 0; (void)hipMemcpy(&live_w, c->d_tile_ctr.p + RTS_OFF_LIVE, sizeof(uint32_t), hipMemcpyDeviceToHost);
    fprintf(stderr, "[rts] end: handle %p head count %llu coop grid %u | cost sum persisted %llu, this build's %llu | live word %u of %u tiles\n", (void*)c, cnt[7], c->last_coop_grid, sums[0], sums[1], live_w, (uint32_t)rts_wave_tiles(c->n_rays));
    if (c->tile_cost_pending && c->d_tile_cost.p) {          // the cost records this launch wrote (merged by the next order build)
        const uint32_t nt = (uint32_t)rts_wave_tiles(c->tile_cost_sig[0]);
        std::vector<uint32_t> h(nt);
        (void)hipMemcpy(h.data(), c->d_tile_cost.p, sizeof(uint32_t) * nt, hipMemcpyDeviceToHost);
        unsigned long long sum = 0, big = 0, flagged = 0; uint32_t mx = 0, shown = 0;
        for (uint32_t j = 0; j < nt; j++) { const uint32_t v = h[j] & 0x3fffffffu; sum += v; if (v > mx) mx = v; if (h[j] >> 31) flagged++; if (v > (1u << 26)) { big++; if (shown++ < 6) fprintf(stderr, "[rts]    tile %u record 0x%08x\n", j, h[j]); } }
        fprintf(stderr, "[rts]    records of this launch: sum %llu max %u, %llu above 2^26, %llu flagged LONG WALKS\n", sum, mx, big, flagged);
    }
}

// What every way of ending a pulse does once the host has waited for its stream: the launch's counters (its failures, the received count,
// the head count), the block timeline's summary, the statistics and the hints of the handle's next launch.
static int rts_pulse_home(RtsContext* c)
{
    const unsigned long long* cnt = c->pin.p->cnt;
    RTS_TRY(rts_counters_home(c, cnt));
    if (c->tl_blocks) pulse_timeline_summary(c);
    rts_pulse_account(c, cnt);
    return RTS_OK;
}

// ev[4] ... order + expand the received rays (and the keep-all buffers, and the host mirror when the pulse feeds it) ... ev[5]; left in flight on the stream
static int rts_post_received(RtsContext* c)
{
    RTS_HIP(hipEventRecord(c->ev[4], c->stream));
    RTS_TRY(rts_post_order_and_expand(c));
    if (c->params.flags & RTS_FLAG_KEEP_ALL_RAYS) { RTS_TRY(rts_post_expand_all(c)); }
    if (c->res.mirror.want) { RTS_TRY(rts_post_mirror_received(c)); }
    RTS_HIP(hipEventRecord(c->ev[5], c->stream));
    return RTS_OK;
}

// Waits for the pulse begun on this handle, then orders + expands its received rays (left in flight).
extern "C" int rts_trace_pulse_end(RtsHandle c)
{
    CHECK_HANDLE(c);
    if (!c->pulse.end()) { rts_set_error("rts_trace_pulse_end: no pulse in flight on this handle"); return RTS_ERR_INVALID; }
    RTS_HIP(rts_stream_wait(c, c->stream));         // the one host sync of the launch: the received count sizes what follows
    RTS_TRY(rts_pulse_home(c));
    if (c->tune.debug_coop && c->d_order_sum.p && c->d_tile_ctr.p) pulse_debug_dump(c, c->pin.p->cnt);
    c->res.agg_timed = false; c->res.fin_timed = false;
    return rts_post_received(c);
}

// ------------------------------------------------------------------------------------- finalise + aggregate
extern "C" int rts_finalise_uniform(RtsHandle c, const double* rcs_per_target, double wavelength, double gt, double gr, double carrier, double cspeed)
{
    CHECK_HANDLE(c);
    CHECK_CLOSED(c);
    std::vector<double> ones;
    if (!rcs_per_target) { ones.assign(c->scene->meshes.size() + 1, 1.0); rcs_per_target = ones.data(); }
    return rts_finalise_bracket(c, [&] { return rts_post_finalise(c, rcs_per_target, wavelength, gt, gr, carrier, cspeed); });
}

static int rts_aggregate_impl(RtsContext* c, double cspeed, double carrier, uint64_t recv_index_base)
{
    const uint64_t R = c->res.n_recv;
    c->res.agg_pending.valid = false;                                       // (an unread table of an earlier call is dropped)
    c->res.groups.clear(); c->res.recv_index_base = recv_index_base;
    if (R == 0) { c->res.agg_valid = true; return RTS_OK; }
    RTS_HIP(c->d_delay.reserve(R)); RTS_HIP(c->d_phase.reserve(R)); RTS_HIP(c->d_pathmatch.reserve(R));
    if (!c->res.fin_timed) RTS_HIP(hipEventRecord(c->ev[6], c->stream));
    c->res.agg_delay_in = false;                                            // (delay / phase sums start at zero: no fills)
    const int32_t max_path = (int32_t)c->scene->meshes.size() - 1, max_rx = c->n_rx ? (int32_t)c->n_rx - 1 : 0;
    const bool use_rows = recv_index_base == RTS_BASE_USE_ROWS;
    c->res.agg_base_local = use_rows ? 0 : (int64_t)recv_index_base;
    int rc = rts_aggregate_device(c, max_path, max_rx, c->d_rx_paths.p, R, c->depth, cspeed, carrier, use_rows ? 0 : recv_index_base, c->d_rx_rays.p,
                                  c->d_delay.p, c->d_phase.p, c->d_pathmatch.p, &c->res.groups, nullptr, nullptr, nullptr, INT32_MAX, use_rows ? c->d_rx_slots.p : nullptr);
    c->res.agg_delay_in = true;
    if (rc != RTS_OK) return rc;
    // (the rays' power / Doppler on the device are the group values now; the mirror still holds the set as it was received, and rts_received_view keeps serving it)
    if (c->res.mirror.want) { rc = rts_post_mirror_aggregated(c); if (rc != RTS_OK) return rc; }
    RTS_HIP(hipEventRecord(c->ev[7], c->stream));
    c->res.agg_timed = true; c->stats_pending = true;
    c->res.agg_valid = true;
    return RTS_OK;
}

extern "C" int rts_aggregate(RtsHandle c, double cspeed, double carrier, uint64_t recv_index_base)
{
    CHECK_HANDLE(c);
    CHECK_CLOSED(c);
    return rts_aggregate_impl(c, cspeed, carrier, recv_index_base);
}

// ------------------------------------------------------------------------------------- a pulse's post-processing without the host in it
// rts_trace_pulse_end_uniform = rts_trace_pulse_end + rts_finalise_uniform (+ rts_cube_accumulate) + rts_aggregate for a caller that
// needs no host callbacks between them ("device-side received count feeding the post kernels").  When the handle's
// previous pulse received no more than 3/4 of what the one-block ordering kernels take (4 096 rays with 32-bit sort keys, 2 048 with
// 64-bit ones) the whole chain is ENQUEUED behind the trace at once, sized for that capacity; its kernels read the received count the trace kernel left on the device and do nothing if it exceeds that
// capacity.  The count, the statistics and the group table come home with the first call that asks (rts_received_count,
// rts_get_stats, rts_group_count, ...; the handle's next rts_trace_pulse_begin at the latest): if the count did exceed the
// capacity the chain is run again then, the ordinary way.  Otherwise -- no history yet, KEEP_ALL, a large received set -- the
// call is the four calls it stands for.
static int rts_post_chain(RtsContext* c, bool ordered = false)      // ordered: rts_trace_pulse_end has ordered + expanded the received set already (its events ev[4] / ev[5] stand)
{
    const RtsSpecParams& q = c->spec;
    hipStream_t st = c->stream;
    const bool keep_all = (c->params.flags & RTS_FLAG_KEEP_ALL_RAYS) != 0;
    int rc = RTS_OK;
    // (one block does in 150 us what seven launches -- four of them many blocks wide -- do in 92 us + six launch gaps for BASELINE configs[2]'s
    // ~1 900 received rays; for a few hundred rays it is the other way round: sequential pulses, one kernel against seven, C3 1.025 / 0.980 ms,
    // C2 (400 rays) 0.339 / 0.354, configs[4] (100) 0.955 / 0.978, profiles/r04_post_one_ab.log -- so the choice follows the handle's last count)
    if (!ordered && q.mode == 0 && c->res.recv_dev && c->recv_hint_valid && c->recv_hint <= c->tune.post_one_max && c->tune.post_small && !keep_all && !c->res.mirror.want && c->res.n_recv <= c->spec_cap) {
        // the speculative chain as ONE kernel (rts_post.hip: k_post_all): sized for the capacity, the count from the device
        RTS_HIP(hipEventRecord(c->ev[4], st)); RTS_HIP(hipEventRecord(c->ev[5], st)); RTS_HIP(hipEventRecord(c->ev[6], st));
        c->res.agg_pending.valid = false; c->res.groups.clear();
        rc = rts_post_all_small(c, (uint32_t)c->res.n_recv, q, true); if (rc != RTS_OK) return rc;
        RTS_HIP(hipEventRecord(c->ev[7], st));
        c->res.fin_timed = true; c->res.agg_timed = true; c->stats_pending = true; c->res.agg_valid = true;
        return RTS_OK;
    }
    if (!ordered) { rc = rts_post_received(c); if (rc != RTS_OK) return rc; }
    if (q.mode == 1) return RTS_OK;                                     // rts_received_prefetch: the received set goes home, the caller finalises it
    RTS_HIP(hipEventRecord(c->ev[6], st));
    rc = q.fin ? rts_post_finalise_patterns(c, q) : rts_post_finalise(c, q.rcs.data(), q.wl, q.gt, q.gr, q.carrier, q.cspeed); if (rc != RTS_OK) return rc;
    c->res.fin_timed = true; c->res.agg_valid = false;
    if (q.cube_pulse >= 0) { rc = rts_cube_accumulate_device(c, (uint32_t)q.cube_pulse, q.cspeed, q.carrier); if (rc != RTS_OK) return rc; }
    rc = rts_aggregate_impl(c, q.cspeed, q.carrier, q.base);
    return rc;
}

static int rts_spec_resolve(RtsContext* c)      // the outcome of a chain that was enqueued on the device-side count (agg_timed / fin_timed stay as the chain set them)
{
    if (!c->pulse.resolve()) return RTS_OK;
    RTS_HIP(hipSetDevice(c->device));
    RTS_HIP(rts_stream_wait(c, c->stream));
    RTS_TRY(rts_pulse_home(c));
    if (c->res.n_recv > c->spec_cap) {                                      // more rays than the speculative chain was sized for: it did nothing; the ordinary chain now
        c->res.agg_pending.valid = false;
        return rts_post_chain(c);
    }
    if (c->res.n_recv == 0) { c->res.agg_pending.valid = false; c->res.groups.clear(); c->res.agg_valid = true; return RTS_OK; }
    c->res.agg_pending.R = (uint32_t)c->res.n_recv; c->res.agg_pending.spec = rts_agg_spec((uint32_t)c->res.n_recv);
    return RTS_OK;
}

// CHECK_CLOSED: OPEN -> ended, CHAINED -> resolved, IDLE -> nothing to do
int rts_pulse_settle(RtsContext* c) { return c->pulse.open() ? rts_trace_pulse_end(c) : c->pulse.chained() ? rts_spec_resolve(c) : RTS_OK; }

static int rts_trace_pulse_end_chain(RtsContext* c);
extern "C" int rts_trace_pulse_end_uniform(RtsHandle c, const double* rcs_per_target, double wavelength, double gt, double gr, double carrier, double cspeed,
                                           int32_t cube_pulse, uint64_t recv_index_base)
{
    CHECK_HANDLE(c);
    if (!c->pulse.open()) { rts_set_error("rts_trace_pulse_end_uniform: no pulse in flight on this handle"); return RTS_ERR_INVALID; }
    if (cube_pulse >= 0 && (!c->cube.set || (uint32_t)cube_pulse >= c->cube.params.n_pulses)) { rts_set_error("rts_trace_pulse_end_uniform: no cube attached, or pulse %d outside it", cube_pulse); return RTS_ERR_INVALID; }
    RtsSpecParams& q = c->spec;
    const size_t nt = c->scene->meshes.size();
    q.rcs.assign(nt + 1, 1.0); if (rcs_per_target) for (size_t t = 0; t < nt; t++) q.rcs[t] = rcs_per_target[t];
    q.wl = wavelength; q.gt = gt; q.gr = gr; q.carrier = carrier; q.cspeed = cspeed; q.cube_pulse = cube_pulse; q.base = recv_index_base; q.mode = 0; q.fin = 0;
    return rts_trace_pulse_end_chain(c);
}

// Is the open pulse's chain (c->spec), of capacity `cap` rays (0: it has none), enqueued behind the trace at once, on the device-side
// count?  When the handle's previous pulse received no more than 3/4 of the capacity.
static bool rts_speculates(const RtsContext* c, uint32_t cap)
{
    const bool keep_all = (c->params.flags & RTS_FLAG_KEEP_ALL_RAYS) != 0;
    return c->tune.post_small && c->tune.spec_enabled && cap > 0 && !keep_all && c->n_rays > 0 && c->recv_hint_valid && c->recv_hint <= ((uint64_t)cap * 3ull) / 4ull;
}
// ... and its enqueueing: the pulse is closed and awaits its resolution (rts_spec_resolve), the chain runs sized for the capacity
// with the count itself from the device (the handle's own stream already waits for the trace: rts_trace_pulse_begin)
static int rts_chain_on_device_count(RtsContext* c, uint32_t cap)
{
    c->spec_cap = cap;
    c->pulse.chain();                                                   // (the pulse stays counted on its device until it is resolved)
    c->res.agg_timed = false; c->res.fin_timed = false;
    c->res.n_recv = cap; c->res.recv_dev = c->p_counters;
    const int rc = rts_post_chain(c);
    c->res.recv_dev = nullptr; c->res.n_recv = 0;
    if (rc != RTS_OK) c->pulse.abandon();
    return rc;
}

// the rest of rts_trace_pulse_end_uniform / _patterns, once c->spec holds the pulse's post-processing parameters
static int rts_trace_pulse_end_chain(RtsContext* c)
{
    // the capacity of the chain: the smaller of its two one-block sorts -- none with a key beyond 64 bits (e.g. 16 bounces among >= 8
    // targets), sorted as two or three words by the GENERAL chain, whose kernels take the received count from the host (rts_post.hip:
    // only the one-block path reads it on the device): such a handle never speculates
    const uint32_t cap = rts_spec_cap(c->last_args.max_refr, rts_handle_key_plan(c));
    if (rts_speculates(c, cap)) return rts_chain_on_device_count(c, cap);
    RTS_TRY(rts_trace_pulse_end(c));
    return rts_post_chain(c, true);
}

// ------------------------------------------------------------------------------------- tabulated antenna gain and RCS patterns
// (rts_amd.h: RtsPattern; the evaluator is rts_pattern.h, shared by the host export and the finalisation kernels)
static bool pat_values_ok(const double* a, uint32_t n) { for (uint32_t i = 0; i < n; i++) if (!std::isfinite(a[i]) || a[i] < 0.0) return false; return true; }
static bool pat_ascending(const double* s, uint32_t n)
{
    for (uint32_t i = 0; i < n; i++) if (!std::isfinite(s[i]) || (i && !(s[i] > s[i - 1]))) return false;
    return true;
}
static int rts_pattern_check(const RtsPattern* p, const char* who, uint32_t index)
{
    if (!p) { rts_set_error("%s pattern %u: null descriptor", who, index); return RTS_ERR_INVALID; }
    if (p->reserved[0] || p->reserved[1]) { rts_set_error("%s pattern %u: reserved fields must be 0", who, index); return RTS_ERR_INVALID; }
    if (!std::isfinite(p->scale) || p->scale < 0.0) { rts_set_error("%s pattern %u: scale must be finite and >= 0", who, index); return RTS_ERR_INVALID; }
    if (p->kind == RTS_PATTERN_CONSTANT) {
        if (p->flags) { rts_set_error("%s pattern %u: a constant pattern takes no flags", who, index); return RTS_ERR_INVALID; }
        return RTS_OK;
    }
    if (p->kind != RTS_PATTERN_SEPARABLE && p->kind != RTS_PATTERN_GRID) { rts_set_error("%s pattern %u: unknown kind %u", who, index, p->kind); return RTS_ERR_INVALID; }
    if (p->n_u < 1 || p->n_v < 1 || p->n_u > RTS_PATTERN_MAX_AXIS || p->n_v > RTS_PATTERN_MAX_AXIS) { rts_set_error("%s pattern %u: %u x %u samples (1 .. %u per axis)", who, index, p->n_u, p->n_v, RTS_PATTERN_MAX_AXIS); return RTS_ERR_INVALID; }
    if (p->kind == RTS_PATTERN_SEPARABLE) {
        if (p->flags & ~(RTS_PATTERN_ABS_U | RTS_PATTERN_ABS_V)) { rts_set_error("%s pattern %u: unknown flags 0x%x", who, index, p->flags); return RTS_ERR_INVALID; }
        if (!p->u_samples || !p->u_values || !p->v_samples || !p->v_values) { rts_set_error("%s pattern %u: null sample or value array", who, index); return RTS_ERR_INVALID; }
        if (!pat_ascending(p->u_samples, p->n_u) || !pat_ascending(p->v_samples, p->n_v)) { rts_set_error("%s pattern %u: samples must be finite and strictly ascending", who, index); return RTS_ERR_INVALID; }
        if (!pat_values_ok(p->u_values, p->n_u) || !pat_values_ok(p->v_values, p->n_v)) { rts_set_error("%s pattern %u: values must be finite and >= 0", who, index); return RTS_ERR_INVALID; }
        return RTS_OK;
    }
    if (p->flags) { rts_set_error("%s pattern %u: a grid pattern takes no flags", who, index); return RTS_ERR_INVALID; }
    if ((uint64_t)p->n_u * p->n_v > RTS_PATTERN_MAX_GRID) { rts_set_error("%s pattern %u: grid of %u x %u samples exceeds %u", who, index, p->n_u, p->n_v, RTS_PATTERN_MAX_GRID); return RTS_ERR_INVALID; }
    if (!p->grid) { rts_set_error("%s pattern %u: null grid", who, index); return RTS_ERR_INVALID; }
    if (!std::isfinite(p->u0) || !std::isfinite(p->v0) || !std::isfinite(p->du) || !std::isfinite(p->dv) || !(p->du > 0.0) || !(p->dv > 0.0) ||
        !std::isfinite(p->u0 + (p->n_u - 1) * p->du) || !std::isfinite(p->v0 + (p->n_v - 1) * p->dv)) { rts_set_error("%s pattern %u: grid origin / spacing must be finite, du and dv > 0", who, index); return RTS_ERR_INVALID; }
    if (!pat_values_ok(p->grid, p->n_u * p->n_v)) { rts_set_error("%s pattern %u: grid values must be finite and >= 0", who, index); return RTS_ERR_INVALID; }
    return RTS_OK;
}
static RtsPatView pat_view(const RtsPattern& p)
{
    RtsPatView v; memset(&v, 0, sizeof(v));
    v.kind = p.kind; v.flags = p.flags; v.n_u = p.n_u; v.n_v = p.n_v; v.scale = p.scale;
    v.us = p.u_samples; v.uy = p.u_values; v.vs = p.v_samples; v.vy = p.v_values; v.u0 = p.u0; v.du = p.du; v.v0 = p.v0; v.dv = p.dv; v.grid = p.grid;
    return v;
}

extern "C" int rts_pattern_eval(const RtsPattern* p, const double* u, const double* v, uint32_t n, double* out)
{
    RTS_TRY(rts_pattern_check(p, "rts_pattern_eval:", 0));
    if (n && (!u || !v || !out)) { rts_set_error("rts_pattern_eval: null point or output array"); return RTS_ERR_INVALID; }
    const RtsPatView w = pat_view(*p);
    for (uint32_t i = 0; i < n; i++) out[i] = rts_pat_eval(w, u[i], v[i]);
    return RTS_OK;
}

extern "C" int rts_set_patterns(RtsHandle c, const RtsPattern* tx, const RtsPattern* rx, uint32_t n_rx, const RtsPattern* rcs, uint32_t n_targets)
{
    CHECK_HANDLE(c);
    if ((n_rx && !rx) || (n_targets && !rcs)) { rts_set_error("rts_set_patterns: null receiver or target pattern array"); return RTS_ERR_INVALID; }
    if (n_rx > (1u << 20) || n_targets > (1u << 20)) { rts_set_error("rts_set_patterns: %u receivers / %u targets", n_rx, n_targets); return RTS_ERR_INVALID; }
    std::vector<const RtsPattern*> all; all.reserve(1 + (size_t)n_rx + n_targets);
    all.push_back(tx); for (uint32_t k = 0; k < n_rx; k++) all.push_back(&rx[k]); for (uint32_t t = 0; t < n_targets; t++) all.push_back(&rcs[t]);
    RTS_TRY(rts_pattern_check(tx, "rts_set_patterns: transmitter", 0));
    for (uint32_t k = 0; k < n_rx; k++) RTS_TRY(rts_pattern_check(&rx[k], "rts_set_patterns: receiver", k));
    for (uint32_t t = 0; t < n_targets; t++) RTS_TRY(rts_pattern_check(&rcs[t], "rts_set_patterns: target", t));
    // ---- pack: [views | the tables' arrays], offsets first, device pointers once the buffer exists
    const size_t n_pat = all.size(), head = (n_pat * sizeof(RtsPatView) + 15) & ~(size_t)15;
    size_t n_dbl = 0;
    for (const RtsPattern* p : all)
        n_dbl += p->kind == RTS_PATTERN_SEPARABLE ? 2 * ((size_t)p->n_u + p->n_v) : p->kind == RTS_PATTERN_GRID ? (size_t)p->n_u * p->n_v : 0;
    const size_t bytes = head + n_dbl * sizeof(double);
    // the handle's enqueued work may still read the previous tables: a speculative chain is resolved (if it has to run again, it runs
    // with the tables it was enqueued for), then the stream drained
    if (c->pulse.chained()) CHECK_CLOSED(c);      // (an OPEN pulse stays in flight: it is finalised with the new tables)
    RTS_HIP(hipStreamSynchronize(c->stream));
    RTS_HIP(c->d_pat.reserve(bytes));
    std::vector<char> host(bytes);
    RtsPatView* views = reinterpret_cast<RtsPatView*>(host.data());
    double* dst = reinterpret_cast<double*>(host.data() + head);
    const double* dev = reinterpret_cast<const double*>(c->d_pat.p + head);
    size_t off = 0;
    for (size_t k = 0; k < n_pat; k++) {
        const RtsPattern& p = *all[k];
        RtsPatView v = pat_view(p);
        v.us = v.uy = v.vs = v.vy = v.grid = nullptr;
        if (p.kind == RTS_PATTERN_SEPARABLE) {
            memcpy(dst + off, p.u_samples, sizeof(double) * p.n_u); v.us = dev + off; off += p.n_u;
            memcpy(dst + off, p.u_values, sizeof(double) * p.n_u); v.uy = dev + off; off += p.n_u;
            memcpy(dst + off, p.v_samples, sizeof(double) * p.n_v); v.vs = dev + off; off += p.n_v;
            memcpy(dst + off, p.v_values, sizeof(double) * p.n_v); v.vy = dev + off; off += p.n_v;
        } else if (p.kind == RTS_PATTERN_GRID) {
            memcpy(dst + off, p.grid, sizeof(double) * p.n_u * p.n_v); v.grid = dev + off; off += (size_t)p.n_u * p.n_v;
        }
        views[k] = v;
    }
    RTS_HIP(hipMemcpy(c->d_pat.p, host.data(), bytes, hipMemcpyHostToDevice));
    c->pat_n_rx = n_rx; c->pat_n_targets = n_targets; c->pat_set = true;
    return RTS_OK;
}

// the pulse's pattern parameters -> q (checks of rts_finalise_patterns / rts_trace_pulse_end_patterns)
static int rts_pattern_pulse_params(RtsContext* c, const RtsPatternPulse* p, RtsSpecParams& q, const char* who)
{
    if (!p) { rts_set_error("%s: null pulse parameters", who); return RTS_ERR_INVALID; }
    if (!c->pat_set) { rts_set_error("%s: no patterns set (rts_set_patterns)", who); return RTS_ERR_INVALID; }
    if (c->pat_n_rx != c->n_rx) { rts_set_error("%s: patterns for %u receivers, the handle has %u", who, c->pat_n_rx, c->n_rx); return RTS_ERR_INVALID; }
    if ((size_t)c->pat_n_targets != c->scene->meshes.size()) { rts_set_error("%s: patterns for %u targets, the scene has %zu", who, c->pat_n_targets, c->scene->meshes.size()); return RTS_ERR_INVALID; }
    if (!c->pulse_traced) { rts_set_error("%s: the handle's received set is not a traced pulse's", who); return RTS_ERR_INVALID; }
    if (c->n_rx && (!p->rx_position || !p->rx_rotation)) { rts_set_error("%s: null receiver positions / rotations", who); return RTS_ERR_INVALID; }
    q.pat_rx.assign((size_t)c->n_rx * 8, 0.0);
    for (uint32_t k = 0; k < c->n_rx; k++) {
        for (int j = 0; j < 3; j++) q.pat_rx[(size_t)k * 8 + j] = p->rx_position[(size_t)k * 3 + j];
        for (int j = 0; j < 4; j++) q.pat_rx[(size_t)k * 8 + 3 + j] = p->rx_rotation[(size_t)k * 4 + j];
    }
    for (int j = 0; j < 3; j++) q.pat_org[j] = c->pulse_org[j];
    q.pat_dir[0] = c->pulse_dir[0]; q.pat_dir[1] = c->pulse_dir[1];
    q.wl = p->wavelength; q.carrier = p->carrier; q.cspeed = p->cspeed; q.fin = 1;
    return RTS_OK;
}

extern "C" int rts_finalise_patterns(RtsHandle c, const RtsPatternPulse* pulse)
{
    CHECK_HANDLE(c);
    CHECK_CLOSED(c);
    RtsSpecParams q;
    RTS_TRY(rts_pattern_pulse_params(c, pulse, q, "rts_finalise_patterns"));
    return rts_finalise_bracket(c, [&] { return rts_post_finalise_patterns(c, q); });
}

extern "C" int rts_trace_pulse_end_patterns(RtsHandle c, const RtsPatternPulse* pulse, int32_t cube_pulse, uint64_t recv_index_base)
{
    CHECK_HANDLE(c);
    if (!c->pulse.open()) { rts_set_error("rts_trace_pulse_end_patterns: no pulse in flight on this handle"); return RTS_ERR_INVALID; }
    if (cube_pulse >= 0 && (!c->cube.set || (uint32_t)cube_pulse >= c->cube.params.n_pulses)) { rts_set_error("rts_trace_pulse_end_patterns: no cube attached, or pulse %d outside it", cube_pulse); return RTS_ERR_INVALID; }
    RtsSpecParams& q = c->spec;
    RTS_TRY(rts_pattern_pulse_params(c, pulse, q, "rts_trace_pulse_end_patterns"));
    q.rcs.assign(c->scene->meshes.size() + 1, 1.0); q.gt = q.gr = 1.0;
    q.cube_pulse = cube_pulse; q.base = recv_index_base; q.mode = 0;
    return rts_trace_pulse_end_chain(c);
}

// ------------------------------------------------------------------------------------- the received set at home without copy calls
// rts_received_prefetch: for a caller that needs the received rays on the HOST (the simulator's RCS / gain callbacks,
// ray_tracer.cpp:1198-1256).  Behind the pulse's trace -- and, when the handle's previous pulse received few rays, without
// waiting for it: the kernels take the count from the device, like rts_trace_pulse_end_uniform's chain -- the received set is
// ordered, expanded and STORED BY A KERNEL into the handle's pinned host mirror; rts_received_view then waits once and hands out
// pointers into it.  No history yet, a large set, KEEP_ALL: the call only marks the pulse, and the ordinary (blocking)
// rts_trace_pulse_end that the first accessor runs feeds the mirror.
extern "C" int rts_received_prefetch(RtsHandle c)
{
    CHECK_HANDLE(c);
    if (!c->pulse.open()) { rts_set_error("rts_received_prefetch: no pulse in flight on this handle"); return RTS_ERR_INVALID; }
    const uint32_t cap = rts_small_cap(rts_recv_key64(c->last_args.max_refr));      // (the chain's only sort: the received rows')
    RTS_TRY(rts_mirror_reserve(c, cap));
    c->res.mirror.want = true;
    if (!rts_speculates(c, cap)) return RTS_OK;
    c->spec.mode = 1;
    return rts_chain_on_device_count(c, cap);
}

// ------------------------------------------------------------------------------------- several GPUs: the plan of an interval
// ---------------------------------------------------------------------------------------------------------------------
// Ray sharding dealt by last-seen cost (include/rts_amd.h: rts_tile_records_get / _set, rts_deal_tiles, rts_set_tile_list)
extern "C" int rts_set_tile_list(RtsHandle c, uint32_t tile, const uint32_t* tile_ids, uint32_t n_ids)
{
    CHECK_HANDLE(c);
    if (c->pulse.open()) { rts_set_error("rts_set_tile_list: a pulse of this handle is in flight"); return RTS_ERR_INVALID; }
    CHECK_CLOSED(c);
    // the cost records of the last launch are indexed through the list in force: into the history before it goes
    RTS_TRY(rts_tile_costs_flush(c));
    if (tile == 0) { c->il_list_n = 0; c->il_list_tile = 0; c->il_list_gen++; c->tile_last_valid = false; return RTS_OK; }      // no list any more
    if ((n_ids && !tile_ids) || tile % RTS_WTILE != 0) { rts_set_error("rts_set_tile_list: tile must be a positive multiple of %d launch indices (got %u)", RTS_WTILE, tile); return RTS_ERR_INVALID; }
    if (n_ids == 0) { c->il_list_n = 0; c->il_list_tile = tile; c->il_list_last = 0; c->il_list_gen++; c->tile_last_valid = false; return RTS_OK; }      // an EMPTY list: this worker was dealt nothing, its launches trace no launch index
    for (uint32_t k = 1; k < n_ids; k++) if (tile_ids[k] <= tile_ids[k - 1]) { rts_set_error("rts_set_tile_list: tile ids must be ascending and unique (entry %u: %u after %u)", k, tile_ids[k], tile_ids[k - 1]); return RTS_ERR_INVALID; }
    const uint64_t total = rts_lattice_size(c->params.width);
    if ((uint64_t)tile_ids[n_ids - 1] * tile >= total) { rts_set_error("rts_set_tile_list: tile %u of %u launch indices lies beyond W^3 = %llu", tile_ids[n_ids - 1], tile, (unsigned long long)total); return RTS_ERR_INVALID; }
    if ((uint64_t)n_ids * tile > 0xffffffffull) { rts_set_error("rts_set_tile_list: more than 2^32 launch indices"); return RTS_ERR_INVALID; }
    RTS_HIP(hipStreamSynchronize(c->stream));                      // (kernels still reading the old list through their launch constants: k_expand of the last pulse)
    RTS_HIP(c->d_il_list.reserve(n_ids));
    RTS_HIP(hipMemcpy(c->d_il_list.p, tile_ids, sizeof(uint32_t) * n_ids, hipMemcpyHostToDevice));
    c->il_list_n = n_ids; c->il_list_tile = tile; c->il_list_last = tile_ids[n_ids - 1]; c->il_list_gen++;
    c->tile_last_valid = false;
    return RTS_OK;
}

extern "C" int rts_tile_records_get(RtsHandle c, uint32_t* records, uint32_t n)
{
    CHECK_HANDLE(c);
    if (c->pulse.open()) { rts_set_error("rts_tile_records_get: a pulse of this handle is in flight"); return RTS_ERR_INVALID; }
    const uint64_t total = rts_lattice_size(c->params.width);
    if (!records || n != (uint32_t)rts_wave_tiles(total)) { rts_set_error("rts_tile_records_get: n must be ceil(W^3 / %d) = %llu", RTS_WTILE, (unsigned long long)rts_wave_tiles(total)); return RTS_ERR_INVALID; }
    RTS_TRY(rts_tile_costs_flush(c));
    RTS_HIP(c->d_rec_tmp.reserve(n));
    RTS_TRY(rts_tile_records_masked(c, c->d_rec_tmp.p, n));
    RTS_HIP(hipMemcpyAsync(records, c->d_rec_tmp.p, sizeof(uint32_t) * n, hipMemcpyDeviceToHost, c->stream));
    RTS_HIP(hipStreamSynchronize(c->stream));
    return RTS_OK;
}

extern "C" int rts_tile_records_set(RtsHandle c, const uint32_t* records, uint32_t n)
{
    CHECK_HANDLE(c);
    if (c->pulse.open()) { rts_set_error("rts_tile_records_set: a pulse of this handle is in flight"); return RTS_ERR_INVALID; }
    const uint64_t total = rts_lattice_size(c->params.width);
    if (!records || n != (uint32_t)rts_wave_tiles(total)) { rts_set_error("rts_tile_records_set: n must be ceil(W^3 / %d) = %llu", RTS_WTILE, (unsigned long long)rts_wave_tiles(total)); return RTS_ERR_INVALID; }
    RTS_HIP(hipStreamSynchronize(c->stream));
    RTS_HIP(c->hist->d.reserve(n));
    RTS_HIP(hipMemcpy(c->hist->d.p, records, sizeof(uint32_t) * n, hipMemcpyHostToDevice));
    c->hist->n = n; c->hist->any = true; c->tile_cost_pending = false; c->order_sum_valid = false;      // (records of the last launch not merged yet are superseded)
    return RTS_OK;
}

// Longest-first dealing of plan tiles to `parts` workers.  Deterministic: ties go to the lower tile number, then to the lower worker.
extern "C" int rts_deal_tiles(const uint32_t* records, uint32_t n_records, uint64_t total_rays, uint32_t tile, uint32_t parts, uint32_t* part_of_tile, uint64_t* cost_of_part)
{
    if (!records || !part_of_tile || parts == 0 || tile == 0 || tile % RTS_WTILE != 0 || total_rays == 0) { rts_set_error("rts_deal_tiles: bad arguments (tile must be a positive multiple of %d, parts >= 1)", RTS_WTILE); return RTS_ERR_INVALID; }
    if ((uint64_t)n_records != rts_wave_tiles(total_rays)) { rts_set_error("rts_deal_tiles: n_records must be ceil(total_rays / %d)", RTS_WTILE); return RTS_ERR_INVALID; }
    const uint64_t n_plan64 = (total_rays + tile - 1) / tile;
    if (n_plan64 > 0xffffffffull) { rts_set_error("rts_deal_tiles: too many tiles"); return RTS_ERR_INVALID; }
    const uint32_t n_plan = (uint32_t)n_plan64, per = tile / RTS_WTILE;
    std::vector<uint64_t> cost(n_plan); std::vector<uint32_t> n_long(n_plan, 0);
    for (uint32_t t = 0; t < n_plan; t++) {
        uint64_t v = 0; const uint64_t w0 = (uint64_t)t * per, w1 = std::min<uint64_t>(w0 + per, n_records);
        for (uint64_t w = w0; w < w1; w++) { v += records[w] & 0x3fffffffu; n_long[t] += (records[w] >> 30) ? 1u : 0u; }      // (LONG or LONGISH walks: what a part's head rule may hand to the cooperative kernel)
        cost[t] = v;                                               // 0: a tile nobody traced yet
    }
    std::vector<uint32_t> order, heads; order.reserve(n_plan);
    for (uint32_t t = 0; t < n_plan; t++) if (cost[t]) (n_long[t] ? heads : order).push_back(t);
    std::stable_sort(order.begin(), order.end(), [&](uint32_t x, uint32_t y) { return cost[x] > cost[y]; });
    std::stable_sort(heads.begin(), heads.end(), [&](uint32_t x, uint32_t y) { return cost[x] > cost[y]; });
    std::vector<std::pair<uint64_t, uint32_t>> heap(parts);
    for (uint32_t r = 0; r < parts; r++) heap[r] = {0, r};
    std::vector<uint64_t> n_of(parts, 0);
    // the tiles that hold LONG or LONGISH WALKS (bits 31 / 30 of a wave tile's record: the cooperative kernel's candidates) first, and by COUNT: a part's time follows the number of cooperative
    // tiles it holds more closely than their recorded cost (BASELINE configs[3] dealt by cost alone: 72 .. 239 of them per eighth, 0.77 .. 1.02 ms;
    // profiles/r05_c4_as_rank.log) -- longest first, each to the worker that holds the fewest of them so far (ties: the least cost)
    {
        std::vector<uint64_t> nl(parts, 0);
        for (uint32_t t : heads) {
            uint32_t best = 0;
            for (uint32_t r = 1; r < parts; r++) if (nl[r] < nl[best] || (nl[r] == nl[best] && heap[r].first < heap[best].first)) best = r;
            part_of_tile[t] = best; nl[best] += n_long[t]; heap[best].first += cost[t]; n_of[best]++;
        }
    }
    // the other tiles WITH a record: longest first, each to the worker with the least cost so far -- min-heap of (load, worker)
    auto cmp = [](const std::pair<uint64_t, uint32_t>& a, const std::pair<uint64_t, uint32_t>& b) { return a > b; };
    std::make_heap(heap.begin(), heap.end(), cmp);
    for (uint32_t k = 0; k < (uint32_t)order.size(); k++) {
        std::pop_heap(heap.begin(), heap.end(), cmp);
        std::pair<uint64_t, uint32_t>& top = heap.back();
        part_of_tile[order[k]] = top.second; top.first += cost[order[k]]; n_of[top.second]++;
        std::push_heap(heap.begin(), heap.end(), cmp);
    }
    std::vector<uint64_t> load(parts, 0);
    for (const auto& h : heap) load[h.second] = h.first;
    // the tiles WITHOUT a record (the first interval, a partial table, records a launch dropped): nothing is known about their cost, so their
    // COUNT is balanced -- in ascending tile order, each to the worker holding the fewest tiles so far (as cost-1 entries of the
    // heap above they all went to the lightest workers: 64 tiles, records {500, 100, 50}, three workers: 0 / ~6 / ~55 of the 61)
    for (uint32_t t = 0; t < n_plan; t++) {
        if (cost[t]) continue;
        uint32_t best = 0;
        for (uint32_t r = 1; r < parts; r++) if (n_of[r] < n_of[best]) best = r;
        part_of_tile[t] = best; n_of[best]++; load[best] += 1;
    }
    if (cost_of_part) for (uint32_t r = 0; r < parts; r++) cost_of_part[r] = load[r];
    return RTS_OK;
}

extern "C" int rts_plan_cpi(uint64_t total_rays, uint32_t n_pulses, uint32_t rank, uint32_t world, uint32_t mode, uint32_t min_items,
                            uint32_t tile, RtsPlanItem* out, uint32_t capacity, uint32_t* n_out)
{
    if (tile == 0) tile = RTS_PLAN_TILE;
    if (!n_out || world == 0 || rank >= world || mode > RTS_SHARD_PULSES_WHOLE) { rts_set_error("rts_plan_cpi: bad argument (rank %u of %u, mode %u)", rank, world, mode); return RTS_ERR_INVALID; }
    std::vector<RtsPlanItem> plan;
    auto item = [&](uint32_t pulse, uint32_t parts, uint32_t part) { RtsPlanItem it; memset(&it, 0, sizeof(it)); it.pulse = pulse; it.ray_first = 0; it.ray_count = total_rays;
                                                                     if (parts > 1) { it.interleave_tile = tile; it.interleave_parts = parts; it.interleave_part = part; } return it; };
    if (mode == RTS_SHARD_RAYS) {
        for (uint32_t k = 0; k < n_pulses; k++) plan.push_back(item(k, world, rank));
    } else if (mode == RTS_SHARD_PULSES_WHOLE && n_pulses >= world) {
        // whole pulses only, in contiguous runs (a handle's consecutive pulses are consecutive in time: its cost history fits): the first
        // n_pulses % world workers trace one pulse more.  A part of a pulse is a launch of another SHAPE -- its tile order starts from nothing,
        // and on a short interval that costs more than the imbalance of one pulse (profiles/r05d_as_rank_pulses_*.log)
        const uint32_t base = n_pulses / world, left = n_pulses - base * world;
        const uint32_t first = rank * base + std::min(rank, left), count = base + (rank < left ? 1u : 0u);
        for (uint32_t i = 0; i < count; i++) plan.push_back(item(first + i, 1, 0));
    } else {
        const uint32_t base = n_pulses / world, left = n_pulses - base * world;
        for (uint32_t i = 0; i < base; i++) plan.push_back(item(rank * base + i, 1, 0));
        if (left) {                                      // the left-over pulse this worker helps with, and who else does
            const uint32_t mine = (uint32_t)((uint64_t)rank * left / world);
            uint32_t group = 0, index = 0;
            for (uint32_t r = 0; r < world; r++) if ((uint32_t)((uint64_t)r * left / world) == mine) { if (r == rank) index = group; group++; }
            plan.push_back(item(base * world + mine, group, index));
        }
    }
    // refinement: the oldest item is split in two (every other one of its tiles each) until there are min_items
    while (!plan.empty() && plan.size() < min_items) {
        const RtsPlanItem it = plan.front();
        const uint32_t parts = it.interleave_parts > 1 ? it.interleave_parts : 1u, part = it.interleave_parts > 1 ? it.interleave_part : 0u;
        if (parts > 0x3fffffffu || rts_part_count(it.ray_count, tile, 2 * parts, part + parts) == 0) break;      // nothing left to split off
        plan.erase(plan.begin());
        plan.push_back(item(it.pulse, 2 * parts, part)); plan.push_back(item(it.pulse, 2 * parts, part + parts));
    }
    *n_out = (uint32_t)plan.size();
    if (out) { if (capacity < plan.size()) { rts_set_error("rts_plan_cpi: capacity %u < %zu items", capacity, plan.size()); return RTS_ERR_CAPACITY; }
               if (!plan.empty()) memcpy(out, plan.data(), sizeof(RtsPlanItem) * plan.size()); }
    return RTS_OK;
}

// ------------------------------------------------------------------------------------- several GPUs: sum of the return cubes
// RCCL is loaded on first use (dlopen): librts_amd.so has no link-time dependency on it, and a process that already holds
// a copy (torch.distributed) shares that one.
namespace {
typedef struct ncclComm* rccl_comm_t;
struct RcclApi {
    void* lib = nullptr; bool tried = false;
    int (*CommInitAll)(rccl_comm_t*, int, const int*) = nullptr;
    int (*CommDestroy)(rccl_comm_t) = nullptr;
    int (*AllReduce)(const void*, void*, size_t, int, int, rccl_comm_t, hipStream_t) = nullptr;
    int (*GroupStart)() = nullptr; int (*GroupEnd)() = nullptr;
    const char* (*GetErrorString)(int) = nullptr;
    bool load() {
        if (tried) return lib != nullptr;
        tried = true;
        const char* names[] = {"librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so.1", "/opt/rocm/lib/librccl.so"};
        for (const char* n : names) { lib = dlopen(n, RTLD_NOW | RTLD_LOCAL); if (lib) break; }
        if (!lib) return false;
        CommInitAll = (int (*)(rccl_comm_t*, int, const int*))dlsym(lib, "ncclCommInitAll");
        CommDestroy = (int (*)(rccl_comm_t))dlsym(lib, "ncclCommDestroy");
        AllReduce = (int (*)(const void*, void*, size_t, int, int, rccl_comm_t, hipStream_t))dlsym(lib, "ncclAllReduce");
        GroupStart = (int (*)())dlsym(lib, "ncclGroupStart"); GroupEnd = (int (*)())dlsym(lib, "ncclGroupEnd");
        GetErrorString = (const char* (*)(int))dlsym(lib, "ncclGetErrorString");
        if (!CommInitAll || !CommDestroy || !AllReduce || !GroupStart || !GroupEnd) { dlclose(lib); lib = nullptr; }
        return lib != nullptr;
    }
};
RcclApi g_rccl;
// Communicators are created once per set of devices and kept (ncclCommInitAll costs hundreds of milliseconds on eight GPUs, an
// all-reduce of a cube half a millisecond); an entry lives as long as one of the handles that used it (rts_destroy ->
// rts_comm_cache_forget).
struct CommEntry { std::vector<int> devs; std::vector<rccl_comm_t> comms; std::vector<RtsContext*> users; };
std::mutex g_comm_mu;
std::vector<CommEntry> g_comm_cache;
__global__ void k_add_f64(double* __restrict__ dst, const double* __restrict__ src, size_t n)
{
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) dst[i] += src[i];
}
// the communicators for the devices of `hs` (in handle order), created on first use; null on failure (*rc_out = RCCL's code)
const std::vector<rccl_comm_t>* comm_cache_get(RtsHandle* hs, uint32_t n, int* rc_out)
{
    std::vector<int> devs(n);
    for (uint32_t i = 0; i < n; i++) devs[i] = hs[i]->device;
    std::lock_guard<std::mutex> lk(g_comm_mu);
    CommEntry* e = nullptr;
    for (auto& x : g_comm_cache) if (x.devs == devs) { e = &x; break; }
    if (!e) {
        CommEntry ne; ne.devs = devs; ne.comms.assign(n, nullptr);
        const int rc = g_rccl.CommInitAll(ne.comms.data(), (int)n, devs.data());
        if (rc != 0) { *rc_out = rc; return nullptr; }
        g_comm_cache.push_back(std::move(ne)); e = &g_comm_cache.back();
    }
    for (uint32_t i = 0; i < n; i++) if (std::find(e->users.begin(), e->users.end(), hs[i]) == e->users.end()) e->users.push_back(hs[i]);
    *rc_out = 0;
    return &e->comms;
}
}  // namespace

// rts_destroy: the handle no longer keeps any communicator set alive; a set without users is destroyed
void rts_comm_cache_forget(RtsContext* c)
{
    std::lock_guard<std::mutex> lk(g_comm_mu);
    for (size_t k = 0; k < g_comm_cache.size();) {
        CommEntry& e = g_comm_cache[k];
        e.users.erase(std::remove(e.users.begin(), e.users.end(), c), e.users.end());
        if (e.users.empty()) { for (rccl_comm_t q : e.comms) if (q) (void)g_rccl.CommDestroy(q); g_comm_cache.erase(g_comm_cache.begin() + k); }
        else k++;
    }
}

// transport 0: RCCL when the handles sit on distinct devices and librccl loads, else peer copies; 1: RCCL or an error (with
// ONE handle: a one-rank communicator and all-reduce -- the identity, but the dlopen, the symbol table and the call sequence
// run, which is how the RCCL path is exercised on a single GPU); 2: peer copies.
extern "C" int rts_cube_reduce(RtsHandle* hs, uint32_t n, int transport)
{
    if (!hs || n == 0) { rts_set_error("rts_cube_reduce: no handles"); return RTS_ERR_INVALID; }
    for (uint32_t i = 0; i < n; i++) {
        if (!hs[i] || !hs[i]->cube.set) { rts_set_error("rts_cube_reduce: handle %u has no cube (rts_cube_attach)", i); return RTS_ERR_INVALID; }
        const RtsCubeParams &a = hs[0]->cube.params, &b = hs[i]->cube.params;
        if (a.n_rx != b.n_rx || a.n_pulses != b.n_pulses || a.n_bins != b.n_bins) { rts_set_error("rts_cube_reduce: handle %u has a cube of another shape", i); return RTS_ERR_INVALID; }
        for (uint32_t j = 0; j < i; j++) if (hs[j]->cube.p == hs[i]->cube.p) { rts_set_error("rts_cube_reduce: handles %u and %u share one cube buffer (nothing to add)", j, i); return RTS_ERR_INVALID; }
    }
    const size_t doubles = 2 * (size_t)hs[0]->cube.params.n_rx * hs[0]->cube.params.n_pulses * hs[0]->cube.params.n_bins;
    for (uint32_t i = 0; i < n; i++) { RtsContext* c = hs[i]; CHECK_CLOSED(c); RTS_HIP(hipSetDevice(c->device)); RTS_HIP(hipStreamSynchronize(c->stream)); }
    if (n == 1 && transport != 1) return RTS_OK;
    bool distinct = true;
    for (uint32_t i = 0; i < n; i++) for (uint32_t j = 0; j < i; j++) if (hs[i]->device == hs[j]->device) distinct = false;
    if (transport != 2 && distinct && g_rccl.load()) {
        // one communicator per device, all in this process; one all-reduce (sum, f64) on each handle's stream inside a group
        int rc = 0;
        const std::vector<rccl_comm_t>* comms = comm_cache_get(hs, n, &rc);
        if (comms) {
            // From here on there is no falling back: the all-reduce is in place, and after a failure part-way some cubes may
            // already hold partial sums -- adding them again over peer copies would count them twice.
            rc = g_rccl.GroupStart();
            for (uint32_t i = 0; i < n && rc == 0; i++) { (void)hipSetDevice(hs[i]->device); rc = g_rccl.AllReduce(hs[i]->cube.p, hs[i]->cube.p, doubles, 8 /* ncclFloat64 */, 0 /* ncclSum */, (*comms)[i], hs[i]->stream); }
            const int rc2 = g_rccl.GroupEnd(); if (rc == 0) rc = rc2;
            for (uint32_t i = 0; i < n; i++) { (void)hipSetDevice(hs[i]->device); (void)hipStreamSynchronize(hs[i]->stream); }
            if (rc == 0) return RTS_OK;
            rts_set_error("rts_cube_reduce: RCCL all-reduce failed (%s); the cubes may hold partial sums", g_rccl.GetErrorString ? g_rccl.GetErrorString(rc) : "?");
            return RTS_ERR_HIP;
        }
        if (transport == 1) { rts_set_error("rts_cube_reduce: ncclCommInitAll failed: %s", g_rccl.GetErrorString ? g_rccl.GetErrorString(rc) : "?"); return RTS_ERR_HIP; }
        // no communicator, nothing issued: peer copies
    } else if (transport == 1) { rts_set_error("rts_cube_reduce: RCCL requested but %s", distinct ? "librccl could not be loaded" : "two handles share a device"); return RTS_ERR_UNSUPPORTED; }
    if (n == 1) return RTS_OK;
    // peer copies: everything is added into handle 0's cube in handle order (bit-reproducible), then copied back out
    RtsContext* c0 = hs[0];
    RTS_HIP(hipSetDevice(c0->device));
    DevBuf<double> tmp; RTS_HIP(tmp.reserve(doubles));
    for (uint32_t i = 1; i < n; i++) {
        RTS_HIP(hipMemcpyPeerAsync(tmp.p, c0->device, hs[i]->cube.p, hs[i]->device, sizeof(double) * doubles, c0->stream));
        k_add_f64<<<(unsigned)((doubles + 255) / 256), 256, 0, c0->stream>>>(c0->cube.p, tmp.p, doubles);
        RTS_HIP(hipGetLastError());
    }
    RTS_HIP(hipStreamSynchronize(c0->stream));
    for (uint32_t i = 1; i < n; i++) RTS_HIP(hipMemcpyPeer(hs[i]->cube.p, hs[i]->device, c0->cube.p, c0->device, sizeof(double) * doubles));
    return RTS_OK;
}

// ------------------------------------------------------------------------------------- host-side group algebra
// Merge partial group tables (one per GPU): same (rx, path) => sums add, min_ray takes the minimum.
// Groups are combined in input order, output sorted by (rx, path) so the result does not depend
// on how many tables were concatenated beyond f64 rounding of the sums.
extern "C" int rts_merge_groups(const RtsGroup* in, uint32_t n_in, uint32_t depth, RtsGroup* out, uint32_t* n_out)
{
    if ((!in && n_in) || !n_out) { rts_set_error("rts_merge_groups: null argument"); return RTS_ERR_INVALID; }
    if (depth > RTS_MAX_DEPTH) { rts_set_error("rts_merge_groups: depth > %d", RTS_MAX_DEPTH); return RTS_ERR_INVALID; }
    typedef std::vector<int32_t> Key;
    std::map<Key, RtsGroup> m;
    for (uint32_t i = 0; i < n_in; i++) {
        Key k(1 + RTS_MAX_DEPTH); k[0] = in[i].rx; for (int d = 0; d < RTS_MAX_DEPTH; d++) k[1 + d] = in[i].path[d];
        auto it = m.find(k);
        if (it == m.end()) m.emplace(k, in[i]);
        else {
            RtsGroup& g = it->second;
            g.n += in[i].n; g.sum_sqrt_power += in[i].sum_sqrt_power; g.sum_delay += in[i].sum_delay; g.sum_phase += in[i].sum_phase; g.sum_doppler += in[i].sum_doppler;
            g.min_ray = std::min(g.min_ray, in[i].min_ray); g.direct = g.direct | in[i].direct;
        }
    }
    if (out) { if (*n_out < m.size()) { rts_set_error("rts_merge_groups: capacity too small"); *n_out = (uint32_t)m.size(); return RTS_ERR_CAPACITY; }
               uint32_t j = 0; for (auto& kv : m) out[j++] = kv.second; }
    *n_out = (uint32_t)m.size();
    return RTS_OK;
}

// Responses the reference would emit (ray_tracer.cpp:1290-1321) from a complete group table:
//   every non-direct group -> one response at its smallest ray, with the group means
//   (aggregation.cu:88-93); a receiver's direct group -> pathMatch = smallest ray of ANY group
//   at that receiver and sums over ALL its rays (aggregation.cu:56): emitted only if that
//   smallest ray is itself direct, otherwise it collapses onto the reflected group (quirk 9).
extern "C" int rts_groups_to_responses(const RtsGroup* groups, uint32_t n_groups, RtsResponse* out, uint32_t capacity, uint32_t* n_out)
{
    if ((!groups && n_groups) || !n_out) { rts_set_error("rts_groups_to_responses: null argument"); return RTS_ERR_INVALID; }
    struct Tot { double n = 0, sp = 0, dl = 0, ph = 0, dp = 0; uint64_t mn = ~0ULL; bool mn_direct = false; bool has_direct = false; };
    std::map<int32_t, Tot> tot;
    for (uint32_t i = 0; i < n_groups; i++) {
        Tot& t = tot[groups[i].rx];
        t.n += groups[i].n; t.sp += groups[i].sum_sqrt_power; t.dl += groups[i].sum_delay; t.ph += groups[i].sum_phase; t.dp += groups[i].sum_doppler;
        if (groups[i].min_ray < t.mn) { t.mn = groups[i].min_ray; t.mn_direct = groups[i].direct != 0; }
        if (groups[i].direct) t.has_direct = true;
    }
    std::vector<RtsResponse> r;
    for (uint32_t i = 0; i < n_groups; i++) {
        const RtsGroup& g = groups[i];
        RtsResponse q; q.rx = g.rx;
        if (!g.direct) {
            if (!(g.n > 0)) continue;
            double v = g.sum_sqrt_power / g.n;
            q.ray = g.min_ray; q.n = (uint32_t)g.n; q.power = v*v; q.delay = g.sum_delay / g.n; q.phase = g.sum_phase / g.n; q.doppler = g.sum_doppler / g.n;
            r.push_back(q);
        } else {
            const Tot& t = tot[g.rx];
            if (!t.mn_direct || !(t.n > 0)) continue;       // direct response lost (quirk 9) when a reflected ray has the smallest index
            double v = t.sp / t.n;
            q.ray = t.mn; q.n = (uint32_t)t.n; q.power = v*v; q.delay = t.dl / t.n; q.phase = t.ph / t.n; q.doppler = t.dp / t.n;
            r.push_back(q);
        }
    }
    std::sort(r.begin(), r.end(), [](const RtsResponse& a, const RtsResponse& b) { return a.ray < b.ray; });   // sort + unique of pathMatch (:1290-1292)
    *n_out = (uint32_t)r.size();
    if (out) { if (capacity < r.size()) { rts_set_error("rts_groups_to_responses: capacity too small"); return RTS_ERR_CAPACITY; }
               if (!r.empty()) memcpy(out, r.data(), sizeof(RtsResponse)*r.size()); }
    return RTS_OK;
}

// ------------------------------------------------------------------------------------- rs::kernel_wrapper
// Contexts of the handle-less entry points, one per device (the device current on the calling thread at the call), created on
// first use and kept for the life of the process.
static std::map<int, RtsContext*> g_wrapper_ctx;
static std::mutex g_wrapper_mutex;

static int wrapper_context(RtsContext** out)
{
    int cur = 0; if (hipGetDevice(&cur) != hipSuccess) cur = 0;
    std::lock_guard<std::mutex> lock(g_wrapper_mutex);
    auto it = g_wrapper_ctx.find(cur);
    if (it == g_wrapper_ctx.end()) {
        RtsParams p; memset(&p, 0, sizeof(p)); p.width = 1; p.max_refl = 1; p.device = cur;
        RtsContext* c = nullptr;
        RTS_TRY(rts_create(&p, &c));
        it = g_wrapper_ctx.emplace(cur, c).first;
    }
    *out = it->second;
    return RTS_OK;
}

extern "C" int rts_kernel_wrapper_on(RtsHandle h, PerRayData* h_rx_results_arr, int* h_rx_intersects_arr, unsigned int receivedRays,
                                     unsigned int depthTotal, unsigned int MaxThreads, unsigned int MaxBlocks, double cspeed,
                                     double carrier, double* h_npath_arr, double* h_power_arr, double* h_doppler_arr,
                                     double* h_delay_arr, double* h_phase_arr, int* h_pathMatch)
{
    (void)MaxThreads; (void)MaxBlocks;   // launch shapes are chosen by the library (aggregation.cu:142-160 picks them from these)
    if (receivedRays == 0) return RTS_OK;
    if (!h_rx_results_arr || (depthTotal && !h_rx_intersects_arr) || !h_delay_arr || !h_phase_arr || !h_pathMatch) { rts_set_error("rts_kernel_wrapper: null array"); return RTS_ERR_INVALID; }
    RtsContext* c = h;
    if (!c) RTS_TRY(wrapper_context(&c));
    else { CHECK_CLOSED(c); c->res.forget(); c->pulse_traced = false; }      // the handle's own received set is overwritten
    RTS_HIP(hipSetDevice(c->device));
    const size_t R = receivedRays, D = depthTotal;
    RTS_HIP(c->d_rx_rays.reserve(R)); RTS_HIP(c->d_rx_paths.reserve(R*D + 1)); RTS_HIP(c->d_delay.reserve(R)); RTS_HIP(c->d_phase.reserve(R)); RTS_HIP(c->d_pathmatch.reserve(R));
    RTS_HIP(c->d_rx_angles.reserve(3*R + 1));     // scratch: npath / power / doppler initial sums
    hipStream_t st = c->stream;
    RTS_HIP(hipMemcpyAsync(c->d_rx_rays.p, h_rx_results_arr, sizeof(PerRayData)*R, hipMemcpyHostToDevice, st));
    if (D) RTS_HIP(hipMemcpyAsync(c->d_rx_paths.p, h_rx_intersects_arr, sizeof(int)*R*D, hipMemcpyHostToDevice, st));
    RTS_HIP(hipMemcpyAsync(c->d_delay.p, h_delay_arr, sizeof(double)*R, hipMemcpyHostToDevice, st));
    RTS_HIP(hipMemcpyAsync(c->d_phase.p, h_phase_arr, sizeof(double)*R, hipMemcpyHostToDevice, st));
    RTS_HIP(hipMemcpyAsync(c->d_pathmatch.p, h_pathMatch, sizeof(int)*R, hipMemcpyHostToDevice, st));
    double* d_np = nullptr; double* d_pw = nullptr; double* d_dp = nullptr;
    if (h_npath_arr) { d_np = c->d_rx_angles.p; RTS_HIP(hipMemcpyAsync(d_np, h_npath_arr, sizeof(double)*R, hipMemcpyHostToDevice, st)); }
    if (h_power_arr) { d_pw = c->d_rx_angles.p + R; RTS_HIP(hipMemcpyAsync(d_pw, h_power_arr, sizeof(double)*R, hipMemcpyHostToDevice, st)); }
    if (h_doppler_arr) { d_dp = c->d_rx_angles.p + 2*R; RTS_HIP(hipMemcpyAsync(d_dp, h_doppler_arr, sizeof(double)*R, hipMemcpyHostToDevice, st)); }
    int32_t max_path = -1, max_rx = 0;
    for (size_t i = 0; i < R * D; i++) { if (h_rx_intersects_arr[i] < -1) { rts_set_error("rts_kernel_wrapper: path entry < -1"); return RTS_ERR_INVALID; } max_path = std::max(max_path, (int32_t)h_rx_intersects_arr[i]); }
    for (size_t i = 0; i < R; i++) { if (h_rx_results_arr[i].received < 0) { rts_set_error("rts_kernel_wrapper: ray %zu is not a received ray", i); return RTS_ERR_INVALID; } max_rx = std::max(max_rx, h_rx_results_arr[i].received); }
    int rc = rts_aggregate_device(c, max_path, max_rx, c->d_rx_paths.p, R, (uint32_t)D, cspeed, carrier, 0, c->d_rx_rays.p, c->d_delay.p, c->d_phase.p,
                                  c->d_pathmatch.p, nullptr, d_np, d_pw, d_dp, INT32_MIN /* use the caller's h_pathMatch */, nullptr);
    if (rc != RTS_OK) return rc;
    // copy back what the reference copies back (aggregation.cu:169-172)
    RTS_HIP(hipMemcpyAsync(h_rx_results_arr, c->d_rx_rays.p, sizeof(PerRayData)*R, hipMemcpyDeviceToHost, st));
    RTS_HIP(hipMemcpyAsync(h_delay_arr, c->d_delay.p, sizeof(double)*R, hipMemcpyDeviceToHost, st));
    RTS_HIP(hipMemcpyAsync(h_phase_arr, c->d_phase.p, sizeof(double)*R, hipMemcpyDeviceToHost, st));
    RTS_HIP(hipMemcpyAsync(h_pathMatch, c->d_pathmatch.p, sizeof(int)*R, hipMemcpyDeviceToHost, st));
    RTS_HIP(hipStreamSynchronize(st));
    return RTS_OK;
}

extern "C" int rts_kernel_wrapper(PerRayData* h_rx_results_arr, int* h_rx_intersects_arr, unsigned int receivedRays,
                                  unsigned int depthTotal, unsigned int MaxThreads, unsigned int MaxBlocks, double cspeed,
                                  double carrier, double* h_npath_arr, double* h_power_arr, double* h_doppler_arr,
                                  double* h_delay_arr, double* h_phase_arr, int* h_pathMatch)
{
    return rts_kernel_wrapper_on(nullptr, h_rx_results_arr, h_rx_intersects_arr, receivedRays, depthTotal, MaxThreads, MaxBlocks, cspeed, carrier,
                                 h_npath_arr, h_power_arr, h_doppler_arr, h_delay_arr, h_phase_arr, h_pathMatch);
}

// the C++ symbol the reference's caller links against (aggregation.cuh:19-22).  The reference prints and exit(1)s on a CUDA
// error (aggregation.cu:17-27); a library must not end the process, and carrying on with un-aggregated arrays would be worse:
// a failure is a C++ exception.
namespace rs {
void kernel_wrapper(PerRayData* h_rx_results_arr, int* h_rx_intersects_arr, unsigned int receivedRays, unsigned int depthTotal,
                    unsigned int MaxThreads, unsigned int MaxBlocks, double cspeed, double carrier, double* h_npath_arr,
                    double* h_power_arr, double* h_doppler_arr, double* h_delay_arr, double* h_phase_arr, int* h_pathMatch)
{
    int rc = rts_kernel_wrapper(h_rx_results_arr, h_rx_intersects_arr, receivedRays, depthTotal, MaxThreads, MaxBlocks, cspeed, carrier,
                                h_npath_arr, h_power_arr, h_doppler_arr, h_delay_arr, h_phase_arr, h_pathMatch);
    if (rc != RTS_OK) throw std::runtime_error(std::string("rs::kernel_wrapper: ") + rts_last_error());
}
}

// ------------------------------------------------------------------------------------- self test
__global__ void k_self_test_math(const float* y, const float* x, float* at, const double* a, const double* b, double* dv, double* sq, uint32_t n)
{
    uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    at[i] = rts_atan2f(y[i], x[i]);
    dv[i] = a[i] / b[i];
    sq[i] = sqrt(fabs(a[i]));
}

extern "C" int rts_self_test_math(RtsHandle c, const float* y, const float* x, float* atan2f_out, const double* a, const double* b,
                                  double* div_out, double* sqrt_out, uint32_t n)
{
    CHECK_HANDLE(c);
    if (n == 0) return RTS_OK;
    DevBuf<float> dy, dx, dat; DevBuf<double> da, db, ddv, dsq;
    RTS_HIP(dy.reserve(n)); RTS_HIP(dx.reserve(n)); RTS_HIP(dat.reserve(n));
    RTS_HIP(da.reserve(n)); RTS_HIP(db.reserve(n)); RTS_HIP(ddv.reserve(n)); RTS_HIP(dsq.reserve(n));
    RTS_HIP(hipMemcpy(dy.p, y, 4*n, hipMemcpyHostToDevice)); RTS_HIP(hipMemcpy(dx.p, x, 4*n, hipMemcpyHostToDevice));
    RTS_HIP(hipMemcpy(da.p, a, 8*n, hipMemcpyHostToDevice)); RTS_HIP(hipMemcpy(db.p, b, 8*n, hipMemcpyHostToDevice));
    k_self_test_math<<<(n + 255)/256, 256, 0, c->stream>>>(dy.p, dx.p, dat.p, da.p, db.p, ddv.p, dsq.p, n);
    RTS_HIP(hipGetLastError()); RTS_HIP(hipStreamSynchronize(c->stream));
    RTS_HIP(hipMemcpy(atan2f_out, dat.p, 4*n, hipMemcpyDeviceToHost)); RTS_HIP(hipMemcpy(div_out, ddv.p, 8*n, hipMemcpyDeviceToHost)); RTS_HIP(hipMemcpy(sqrt_out, dsq.p, 8*n, hipMemcpyDeviceToHost));
    return RTS_OK;
}
