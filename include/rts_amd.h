/* rts_amd.h -- C-ABI of the MI355X-native RTS hot path (librts_amd.so).
 *
 * Drop-in boundary for the ray-traced radar return path of ymartin101/RTS:
 *   ray launch -> closest triangle hit (static target-space BVH4, f64 triangle test) -> reflect shading ->
 *   receiver-sphere capture -> host/device finalisation -> per-receiver path aggregation.
 * Each entry point cites the reference interface it replaces (file:line in the reference
 * repository).  Plain pointers and sizes only: no HIP, torch or C++ types.
 *
 * Conventions
 *   - every function returns an int status (RTS_OK == 0); nothing ever exit()s or aborts
 *     (the reference aborts the process: RT_CHECK_ERROR, aggregation.cu:17-27);
 *     rts_last_error() returns a description of the last failure on the calling thread.
 *   - the library owns all device memory; the caller owns every host array it passes.
 *   - a handle is not thread-safe: one handle per host thread (and per GPU).
 *   - there is NO CPU fallback: every compute entry point fails with RTS_ERR_NO_DEVICE when
 *     no gfx950 device is usable.
 */
#ifndef RTS_AMD_H
#define RTS_AMD_H

#include <stdint.h>
#include "rts_prd.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct RtsContext* RtsHandle;

enum {
    RTS_OK = 0,
    RTS_ERR_INVALID = 1,      /* bad argument                                       */
    RTS_ERR_NO_DEVICE = 2,    /* no usable HIP device / kernels not loadable        */
    RTS_ERR_HIP = 3,          /* a HIP runtime call failed                          */
    RTS_ERR_UNSUPPORTED = 4,  /* feature outside the built scope    */
    RTS_ERR_CAPACITY = 5,     /* caller buffer too small                            */
    RTS_ERR_IO = 6            /* mesh file could not be read                        */
};

/* Launch-invariant parameters: rsParameters::GetRTSVariables() and friends
 * (ray_tracer.cpp:600-605, 645-648). */
typedef struct RtsParams {
    uint32_t width;              /* W: rays per lattice dimension, rayTotal = W^3 (rts_vars.x)          */
    uint32_t max_refl;           /* h_maxReflDepth (rts_vars.y)                                         */
    uint32_t max_refr;           /* h_maxRefrDepth (rts_vars.z); >0 is clamped to 2 as the reference:
                                    every output buffer then has max_refl + 3 rows per launch index,
                                    row = launch index + k * W^3 (ray_tracer.cpp:604-626)               */
    uint32_t interpolate_smooth; /* rsParameters::interpolate_smooth()                                  */
    int32_t device;              /* HIP device ordinal                                                  */
    uint32_t flags;              /* RTS_FLAG_*                                                          */
} RtsParams;

#define RTS_FLAG_KEEP_ALL_RAYS 1u /* also keep the full per-ray output buffers of the reference
                                     (dbuf_results / dbuf_targ_intersect / dbuf_rcs_angle for EVERY
                                     launch index) plus the per-segment hit trace -- parity/debug */
#define RTS_FLAG_DEVICE_BUILD 4u  /* (the default since round 3; kept for callers that set it) rts_set_scene builds the hierarchy ON THE
                                   * DEVICE: slab-split references, top-down binned SAH level by level, 4-wide collapse, compaction --
                                   * milliseconds for 10^5-10^6 triangles (the reference has OptiX rebuild its acceleration on the
                                   * device every pulse, ray_tracer.cpp:1126-1130; here once per scene) */
#define RTS_FLAG_HOST_BUILD 16u   /* build the hierarchy with the host SAH builder instead (rts_sah.cpp: seconds; a slightly better tree
                                   * on meshes with fans of sliver triangles) */
#define RTS_FLAG_NO_PREFILTER 8u   /* primary rays skip the conservative f32 pre-filter (direction mask over the placed triangles +
                                     widened receiver spheres) that lets rays which can meet nothing bypass the exact ray
                                     generation and the walk.  Results are identical either way (tested); the filter also switches
                                     itself off while more than half of a handle's launch indices hit.  RTS_PRIMARY_MASK=0 does the
                                     same from the environment. */
#define RTS_FLAG_NO_HORIZON 32u    /* bounce rays always walk the target they left.  By default a bounce ray that leaves its triangle above the
                                     triangle's horizon -- how high the rest of the same mesh rises over the triangle's plane, found once per
                                     scene (rts_get_horizon) -- provably misses that mesh and skips its walk.  Results are identical either
                                     way (tested); refracting launches never skip. */
#define RTS_FLAG_NO_HORIZON_SECTORS 64u /* the horizon by its isotropic rule only.  By default a bounce ray that the isotropic rule keeps walking is
                                     tested again against the horizon of the azimuth quadrant it leaves into (four values per side of a
                                     primitive, rts_get_horizon_sectors): a wing rises over a fuselage triangle's plane in one direction only.
                                     Results are identical either way (tested); for A/B runs, the tests and the fuzzer. */
#define RTS_FLAG_COUNT_TRAVERSAL 2u /* run the counting build of the trace kernel (node visits and
                                     triangle tests per segment, for the roofline accounting)        */

/* One target mesh in its own frame, i.e. after the t = 0 rotation of the mesh builders and
 * BEFORE the per-pulse displacement (ray_tracer.cpp:963-987).  Mirrors the per-instance
 * buffers dbuf_triangles / dbuf_triVertices / dbuf_normals and variables d_targReflCoeff /
 * d_targRefrIndex (ray_tracer.cpp:1043-1114).  n_normals > n_vertices selects the "rect"
 * per-face normal rule of triangle_mesh.cu:178-180. */
typedef struct RtsMesh {
    const uint32_t* triangles;   /* [n_triangles][3] vertex indices                     */
    const double* vertices;      /* [n_vertices][3]                                     */
    const double* normals;       /* [n_normals][3]                                      */
    uint32_t n_triangles, n_vertices, n_normals;
    uint32_t reserved;
    double refl_coeff;           /* Target::GetReflCoeff()                              */
    double refr_index;           /* Target::GetRefrIndex()                              */
} RtsMesh;

/* Per-pulse placement of one target: ray_tracer.cpp:941-948 (positions), :993-1007 (time
 * varying rotation applied to the t = 0 mesh), :1010-1014 (displacement), :1144-1145
 * (velocity = (pos(t + Ts) - pos(t)) / Ts). */
typedef struct RtsTargetMotion {
    double position[3];
    double velocity[3];
    double rotation[9];          /* row-major R_total = Rz*Ry*Rx, used only if has_rotation; must be a rotation
                                  * (|R^T R - I| < 1e-3): the hierarchy is rigid, else RTS_ERR_UNSUPPORTED   */
    int32_t has_rotation;
    int32_t reserved;
} RtsTargetMotion;

/* Receiver capture sphere: dbuf_sphCentre / sphRadius / min,maxTheta / min,maxPhi
 * (ray_tracer.cu:33-38), values as computed at ray_tracer.cpp:894-918. */
typedef struct RtsReceiverSphere {
    double centre[3];
    double radius;
    double min_theta, max_theta, min_phi, max_phi;
} RtsReceiverSphere;

/* One launch (one transmitter, one pulse): d_rayOrigin / d_txSpan / d_txDir
 * (ray_tracer.cu:41-43; ray_tracer.cpp:818,881-890).  ray_first/ray_count select a contiguous
 * range of the W^3 launch indices (multi-GPU sharding); ray_count == 0 means all. */
typedef struct RtsPulse {
    double ray_origin[3];
    double tx_span[3];           /* azimuth span, elevation span, launch range           */
    double tx_dir[2];            /* boresight azimuth, elevation                         */
    uint64_t ray_first;
    uint64_t ray_count;
    const RtsTargetMotion* motion; /* [n_targets]; NULL = keep the previous placement    */
    /* Interleaved sharding inside [ray_first, ray_first + ray_count): the range is cut into tiles of
     * interleave_tile launch indices and this launch traces tiles part, part + parts, part + 2 parts, ...
     * (parts <= 1: the whole range).  Rays that hit cluster in launch-index space, so ranks that share one
     * pulse balance far better with interleaved tiles than with contiguous sub-ranges.
     * interleave_parts == RTS_INTERLEAVE_LIST: the launch traces the tiles DEALT to the handle with rts_set_tile_list
     * (interleave_tile must be that list's tile size; interleave_part is ignored). */
    uint32_t interleave_tile, interleave_parts, interleave_part, reserved;
} RtsPulse;
#define RTS_INTERLEAVE_LIST 0xffffffffu

/* Per-pulse counters and stage timings (the reference prints four wall-clock timers,
 * ray_tracer.cpp:1158,1170,1332; aggregation.cu:166). */
typedef struct RtsStats {
    uint64_t rays;               /* launch indices traced in this call                  */
    uint64_t segments;           /* rtTrace calls: primary + bounce segments            */
    uint64_t shaded;             /* closest-hit invocations that passed the depth gate   */
    uint64_t received;           /* rays with received >= 0                             */
    uint64_t node_visits;        /* BVH nodes fetched   (RTS_FLAG_COUNT_TRAVERSAL only) */
    uint64_t tri_tests;          /* triangle tests      (RTS_FLAG_COUNT_TRAVERSAL only) */
    uint32_t n_prims, n_nodes;
    float ms_scene;              /* per-pulse scene placement (vertices, normals, leaves)*/
    float ms_trace;              /* trace kernel                                        */
    float ms_compact;            /* received-ray ordering + record expansion            */
    float ms_aggregate;          /* finalise + group-by                                 */
    uint32_t bvh_rebuilt;        /* 1 if a target moved and the scene was re-placed      */
    uint32_t stack_overflows;    /* traversal stack spills to global memory             */
    uint64_t walked_segments;    /* segments that entered a target's hierarchy at all -- the rest were cleared by the primary-ray
                                    pre-filter or by the targets' bounding spheres (RTS_FLAG_COUNT_TRAVERSAL only)              */
    uint32_t coop_tiles;         /* wave tiles of this launch traced as cooperative units (one launch index per wave)           */
    uint32_t cost_records_dropped;/* tiles whose duration read as nonsense and left no cost record (never, since the records are
                                    taken on the constant-rate counter; counted, not assumed)                                    */
} RtsStats;

/* One aggregated return: what ray_tracer.cpp:1301-1321 turns into an InterpPoint/Response. */
typedef struct RtsResponse {
    uint64_t ray;                /* index in the received list of the representative ray */
    int32_t rx;                  /* receiver index                                       */
    uint32_t n;                  /* rays aggregated                                      */
    double power, delay, doppler, phase;
} RtsResponse;

/* Partial sums of one (receiver, path) group -- the unit exchanged between GPUs. */
#define RTS_MAX_DEPTH 16
typedef struct RtsGroup {
    int32_t rx;
    uint32_t direct;             /* 1 if this is the direct-transmission group           */
    int32_t path[RTS_MAX_DEPTH]; /* target index per depth, -1 padded                    */
    uint64_t min_ray;            /* smallest received-list index in the group (global)   */
    double n, sum_sqrt_power, sum_delay, sum_phase, sum_doppler;
} RtsGroup;

/* ---------------------------------------------------------------- life cycle */
int rts_create(const RtsParams* params, RtsHandle* out);      /* rtContextCreate .. ray_tracer.cpp:532-800 */
int rts_destroy(RtsHandle h);                                 /* ray_tracer.cpp:1342-1360                  */
const char* rts_last_error(void);
/* 16 hex digits: SHA-256 (truncated) of the sources the library was built from (the .hip / .cpp / .h files of rts_amd/csrc + rts_amd.h + rts_prd.h,
 * in byte order of their names).  Profiles record it; bench.py refuses to price a run with counters of another build. */
const char* rts_build_id(void);
/* Restrict the calling process's threads to the CPUs of `device`'s NUMA node (one process per GPU, on the GPU's socket: kernel
 * launches and completion signals then stay on one socket -- 7 % of a pipelined pulse on a two-socket host).  Optional; call it
 * before creating handles, so that their pinned host blocks are allocated on that node too.  *numa_node (may be NULL): the node,
 * -1 if the platform does not report one (nothing is changed then). */
int rts_bind_host_to_device(int device, int* numa_node);
int rts_device_count(int* n);

/* ---------------------------------------------------------------- scene */
int rts_set_scene(RtsHandle h, const RtsMesh* meshes, uint32_t n_targets);          /* ray_tracer.cpp:1020-1117 */
int rts_set_receivers(RtsHandle h, const RtsReceiverSphere* rx, uint32_t n_rx);     /* ray_tracer.cpp:670-715,894-925 */
/* Several handles on one device (pulses in flight, rts_trace_pulse_begin/_end) can SHARE the immutable part of a scene:
 * dst gives up its own and reads src's meshes, hierarchy and leaf order (reference counted; the hierarchy is built once,
 * by the rts_set_scene of the handle that owns it).  Each handle still places, traces and post-processes into its own
 * per-pulse buffers.  A later rts_set_scene on any of the handles gives that handle a fresh scene of its own. */
int rts_share_scene(RtsHandle dst, RtsHandle src);
typedef struct RtsSceneInfo {
    uint32_t n_targets, n_prims, n_nodes, n_leaves;
    uint32_t handles_sharing;    /* handles that point at this scene                                         */
    uint32_t builder;            /* 0: host SAH (rts_sah.cpp), 1: device LBVH (rts_lbvh.hip)                 */
    double build_ms;             /* wall time of the hierarchy build inside rts_set_scene                    */
    uint64_t shared_device_bytes;/* device memory of the shared, immutable part                              */
    uint64_t handle_device_bytes;/* device memory of this handle's placement of it (leaf records, world-space
                                    vertices and normals); per-launch buffers (rts_reserve) not included       */
    uint64_t version_bytes;      /* of shared_device_bytes: the eight octant versions of the node records (0: the
                                    scene has none -- RTS_NODE_VERSIONS=0, or too large for them)               */
    uint64_t horizon_bytes;      /* of shared_device_bytes: the primitives' horizon, 2 x 4 bytes each (rts_get_horizon)    */
} RtsSceneInfo;
int rts_scene_info(RtsHandle h, RtsSceneInfo* out);
/* The isotropic horizon of the scene's primitives (per side the largest of its four azimuth sectors, below): out[n_prims][2] = (S+, S-) by global primitive id, S+ on the side
 * the normal (p0 - p2) x (p1 - p0) points to.  S = an upper bound of the sine of the elevation, over the triangle's plane, at which any
 * other point of the same mesh is seen from the triangle (0: nothing rises above the plane on that side; 1: the side is closed, or the
 * mesh's horizon is off -- a degenerate triangle, too large a mesh). */
int rts_get_horizon(RtsHandle h, float* out, uint32_t capacity_prims);
/* The horizon by azimuth sector, as the leaf records carry it: out[n_prims][2][4] bytes by global primitive id -- side (+, -), then the quadrant
 * of the departing ray's in-plane azimuth in the primitive's own frame u = e0 = p1 - p0, w = n x e0: sector = (a.u < 0 ? 1 : 0) | (a.w < 0 ? 2 : 0).
 * A byte b stands for b / 255, rounded up by the build; 0 is exactly 0, 255 closed.  rts_get_horizon returns, per side, the largest of the four
 * decoded: the isotropic S. */
int rts_get_horizon_sectors(RtsHandle h, uint8_t* out, uint32_t capacity_prims);

/* ---------------------------------------------------------------- launch
 * Replaces rtContextValidate/Compile/Launch3D (ray_tracer.cpp:1126-1165): places the targets,
 * re-places the scene on the device if any target moved (the hierarchy is static), traces ray_count launch indices and
 * leaves the received rays on the device, ordered by ascending launch index (the order of the
 * host scan at ray_tracer.cpp:1190).  Blocking. */
int rts_trace_pulse(RtsHandle h, const RtsPulse* pulse);

/* Pulse pipelining.  The reference runs its pulses strictly one after the other (the loop at ray_tracer.cpp:843:
 * acceleration rebuild -> rtContextLaunch3D -> host read-back -> aggregation, each blocking).  Pulses are independent,
 * so a caller may keep two (or more) handles holding the same scene, link them once, and alternate pulses between them:
 *     rts_trace_pulse_begin(hB, pulse k+1);   // enqueued, returns at once
 *     rts_trace_pulse_end(hA);                // pulse k: wait for its trace, order + expand its received rays
 *     ... rts_finalise_uniform / rts_cube_accumulate / rts_aggregate on hA ...
 * rts_trace_pulse == begin + end.  Trace kernels of linked handles execute one at a time in begin order (each has the
 * whole GPU, so rts_get_stats().ms_trace stays a single-kernel time); the scene placement of the next pulse and the
 * ordering / finalisation / aggregation of the previous one overlap with them on the handles' own HIP streams.
 * Linking is optional: un-linked handles also overlap their trace kernels (the tail of one launch -- a few slow tiles --
 * is filled by the next handle's blocks), which is faster; linking trades that for strictly serial, cleanly timed kernels.
 * Entry points that read a pulse's results end a begun pulse implicitly.  One host thread per link group. */
/* Optional: allocate (and touch) the device buffers of launches of up to n_rays launch indices now (0 = W^3) instead of
 * inside the first rts_trace_pulse; keeps multi-GB allocations out of a timed or latency-critical region. */
int rts_reserve(RtsHandle h, uint64_t n_rays);
int rts_trace_pulse_begin(RtsHandle h, const RtsPulse* pulse);
int rts_trace_pulse_end(RtsHandle h);
int rts_link_handles(RtsHandle a, RtsHandle b);               /* same device; groups grow by linking a member to a new handle */
int rts_get_stats(RtsHandle h, RtsStats* out);
/* Diagnostic (handles created with RTS_TIMELINE_BLOCKS=1; product builds): when the persistent blocks of the last launch started and ended -- out[0..2] first / median /
 * last block start, out[3..7] first / 10th percentile / median / 90th percentile / last block end, microseconds after the first start, out[8] the number of blocks. */
int rts_get_block_timeline(RtsHandle h, double* out, uint32_t n);

/* Received rays of the last pulse (ray_tracer.cpp:1186-1257 before the gain/RCS update):
 * rays[R], paths[R][D] (h_rx_intersects, D = max_refr + max_refl), rcs_angles[R][D][2],
 * slots[R] = global launch index.  Any output pointer may be NULL.  capacity in rays. */
/* Lane statistics of the last launch's traversal (counting build, RTS_FLAG_COUNT_TRAVERSAL): out3[0] walk iterations issued x 64
 * lanes, out3[1] the part issued to lanes that took part in their tile's bounce round, out3[2] walk steps actually taken. */
int rts_get_lane_stats(RtsHandle h, uint64_t* out3);
int rts_get_walk_stats(RtsHandle h, uint64_t* out, uint32_t n);   /* out[0..2] as rts_get_lane_stats; [3] segments that walked; [4] lane-steps issued to lanes that are in a bounce round but never started a walk in it; [5] bounce segments that skipped a target's walk above their triangle's horizon by the isotropic rule ([11]: by an azimuth sector only); [6] walk iterations of the waves in bounce rounds >= 1, [7] bounce rounds >= 1 in which the wave ran no walk at all, [8] bounce rounds >= 1, [9] walk iterations of the waves in round 0 (the primaries), [10] rounds 0 (counting builds; n <= 12) */
int rts_received_count(RtsHandle h, uint64_t* count);
int rts_get_received(RtsHandle h, struct PerRayData* rays, int32_t* paths, double* rcs_angles, uint64_t* slots,
                     uint64_t capacity);

/* The same without copy calls, for a caller in a pulse loop that needs the received rays on the HOST (the simulator's RCS and
 * antenna-gain callbacks of ray_tracer.cpp:1198-1256; include/rts_adapter.hpp):
 *     rts_trace_pulse_begin(h, pulse); rts_received_prefetch(h);       // enqueued, returns at once
 *     ... other handles' pulses ...
 *     rts_received_view(h, &rays, &paths, &angles, NULL, &R);          // ONE wait; pointers into the handle's pinned host mirror
 *     for i < R: power[i], doppler[i] = callbacks(rays[i], paths[i], angles[i])
 *     rts_finalise_values(h, power, doppler, R); rts_aggregate(h, c, fc, 0);      // enqueued
 *     ... other handles' pulses ...
 *     rts_aggregated_view(h, &power, &doppler, &delay, &phase, &path_match, &R);   // ONE wait; what rs::kernel_wrapper returns
 * rts_received_prefetch enqueues the ordering + expansion of the pulse's received rays behind its trace and has a kernel store
 * the result into mapped host memory -- without waiting for the trace when the handle's previous pulse received at most 3 072
 * rays (1 536 with refraction chains), otherwise it only marks the pulse and the first accessor's (blocking) rts_trace_pulse_end
 * feeds the mirror.  Either way the views equal rts_get_received / rts_get_aggregated bit for bit; sets beyond the mirror
 * (4 096 rays, or what the handle has seen) are served by copies.  View pointers stay valid until the handle's next
 * rts_trace_pulse_begin and keep their content: rts_received_view's records are the set as it was at the pulse's FIRST call of it --
 * AS RECEIVED when that call precedes rts_finalise_values (the adapter's order) -- whatever rts_finalise_values / rts_aggregate /
 * rts_aggregated_view do afterwards, also for sets beyond the mirror's capacity (served from copies made once per pulse). */
int rts_received_prefetch(RtsHandle h);
int rts_received_view(RtsHandle h, const struct PerRayData** rays, const int32_t** paths, const double** rcs_angles, const uint64_t** slots,
                      uint64_t* count);
int rts_finalise_values(RtsHandle h, const double* power, const double* doppler, uint64_t count);
int rts_aggregated_view(RtsHandle h, const double** power, const double** doppler, const double** delay, const double** phase,
                        const int32_t** path_match, uint64_t* count);

/* Full per-launch-index buffers (RTS_FLAG_KEEP_ALL_RAYS): results[n] / targ_intersect[n][D] /
 * rcs_angle[n][D][2] as mapped at ray_tracer.cpp:1180-1182, plus hit_prim[n][max_refl+1] (global
 * primitive id of the closest hit of each segment of the reflection chain, -1 = miss, -2 = not
 * traced) and hit_t[n][max_refl+1] (its f32 distance). */
int rts_get_all_rays(RtsHandle h, struct PerRayData* results, int32_t* targ_intersect, double* rcs_angle,
                     int32_t* hit_prim, float* hit_t, uint64_t capacity);

/* ---------------------------------------------------------------- finalise + aggregate on the device
 * rts_finalise_uniform: the per-received-ray update of ray_tracer.cpp:1219-1253 for the case
 * where RCS is a constant per target and the antenna gains are constants (isotropic antennas):
 *   power *= prod RCS[targ_k] ; power *= wavelength^2 * gt * gr ;
 *   doppler = carrier * ((1 + Vr/c) / (1 - Vr/c) - 1), Vr = doppler / 2.
 * With SOARS antenna / RCS callbacks use rts_get_received + rs::kernel_wrapper instead. */
int rts_finalise_uniform(RtsHandle h, const double* rcs_per_target, double wavelength, double gt, double gr,
                         double carrier, double cspeed);

/* One call instead of rts_trace_pulse_end + rts_finalise_uniform (+ rts_cube_accumulate when cube_pulse >= 0) + rts_aggregate, for a
 * caller that needs no host callbacks between them (ray_tracer.cpp:1180-1285 with constant RCS / gains).  When the handle's previous
 * pulse received few rays (at most 3 072 -- 1 536 with refraction chains or a (receiver, path) key beyond 31 bits) the whole chain is
 * enqueued behind the trace WITHOUT waiting for its received count -- the kernels take it from the device -- and the call returns
 * at once; the count, the statistics and the group table come home with the first call that asks for them (rts_received_count,
 * rts_get_stats, rts_group_count, rts_get_groups, rts_get_received, ...; the handle's next rts_trace_pulse_begin at the latest).  A
 * pulse that then turns out to have received more than the chain was sized for (4 096 / 2 048 rays) is post-processed again, the
 * ordinary way, at that point.  Results are those of the four calls, bit for bit.  (Measured on an MI355X with ROCm 7: the
 * submitting thread's wait for the trace disappears, the pulse rate does not change -- DESIGN.md section 5.) */
int rts_trace_pulse_end_uniform(RtsHandle h, const double* rcs_per_target, double wavelength, double gt, double gr,
                                double carrier, double cspeed, int32_t cube_pulse, uint64_t recv_index_base);

/* ---------------------------------------------------------------- tabulated antenna gain and RCS patterns
 * The per-received-ray update of ray_tracer.cpp:1198-1253 with the simulator's GetRCS / GetGain answered from tables on the
 * device instead of host callbacks.
 *
 * A pattern is a non-negative function of two angles (u, v), of one of three kinds:
 *   RTS_PATTERN_CONSTANT   scale, exactly (no arithmetic: the bits of the uniform path).
 *   RTS_PATTERN_SEPARABLE  scale * Lu(u') * Lv(v').  Lu, Lv piecewise-linear over strictly ascending sample abscissae (n >= 1),
 *                          clamped to the end values outside the sample range.  u' = |u| if RTS_PATTERN_ABS_U is set, else u;
 *                          likewise v' with RTS_PATTERN_ABS_V.
 *   RTS_PATTERN_GRID       scale * bilinear(grid, u, v).  grid row-major [n_v][n_u], samples at (u0 + i du, v0 + j dv),
 *                          du, dv > 0; coordinates clamped to the grid's range; interpolated in u on rows j and j+1, then in v.
 * A linear segment is y_i + t * (y_{i+1} - y_i), t = (x - s_i) / (s_{i+1} - s_i) (the library builds with -ffp-contract=off).
 * wrap(x) = x - 2 pi floor((x + pi) / 2 pi), in [-pi, pi).
 *
 * Antennas.  transvec / recvvec as ray_tracer.cpp:1204-1211: direct rays (reflDepth == 0 && refrDepth == 0) transvec =
 * origin - rx_pos, recvvec = rx_pos - origin (the reference's own sign); all others transvec = firstHitPoint - origin, recvvec =
 * prevHitPoint - rx_pos.  az = atan2(y, x), el = asin(z / |vec|) (0 for a zero vector); u = wrap(az - r_az), v = el - r_el (no
 * wrap on v).  Reference direction r: the transmitter's is the traced pulse's tx_dir (= GetRotation(time_t)), origin its
 * ray_origin; receiver k's is (az_k + az_rate_k * delay, el_k + el_rate_k * delay), delay = rayLength / cspeed -- the
 * GetRotation(delay + time_t) of :1234-1235 for a constant-rate rotation (az_k, el_k at the pulse time, rates in rad/s).
 * RCS.  At depth d with targ_d >= 0: target targ_d's pattern at u = wrap(x / 2), v = y / 2, (x, y) the ray's rcs_angle at d
 * (sums of the in- and out-azimuths and -elevations: the half sums are the bistatic bisector).  Another convention is folded
 * into the tables (e.g. the square root of a separable product is the product of the per-axis square roots).
 * Finalised ray, in the operand order of :1225-1247: power *= RCS_d in depth order, then power *= (wl*wl*Gt*Gr); Doppler as
 * rts_finalise_uniform.  With every pattern CONSTANT the result equals rts_finalise_uniform bit for bit.
 * Tables are for one wavelength: a caller whose carrier changes sets the patterns again. */
#define RTS_PATTERN_CONSTANT 0u
#define RTS_PATTERN_SEPARABLE 1u
#define RTS_PATTERN_GRID 2u
#define RTS_PATTERN_ABS_U 1u
#define RTS_PATTERN_ABS_V 2u
#define RTS_PATTERN_MAX_AXIS 65536u           /* samples per axis (separable n_u, n_v; grid n_u, n_v)   */
#define RTS_PATTERN_MAX_GRID 4194304u         /* grid n_u * n_v                                         */
typedef struct RtsPattern {
    uint32_t kind;               /* RTS_PATTERN_*                                                        */
    uint32_t flags;              /* RTS_PATTERN_ABS_U | RTS_PATTERN_ABS_V (SEPARABLE only; 0 otherwise)  */
    uint32_t n_u, n_v;           /* SEPARABLE: samples per axis; GRID: columns, rows; CONSTANT: unused   */
    double scale;                /* finite, >= 0                                                         */
    const double* u_samples;     /* SEPARABLE: [n_u] strictly ascending, finite                          */
    const double* u_values;      /* SEPARABLE: [n_u] finite, >= 0                                        */
    const double* v_samples;     /* SEPARABLE: [n_v]                                                     */
    const double* v_values;      /* SEPARABLE: [n_v]                                                     */
    double u0, du, v0, dv;       /* GRID: first sample and spacing per axis (finite, du, dv > 0)         */
    const double* grid;          /* GRID: [n_v][n_u] finite, >= 0                                        */
    uint64_t reserved[2];        /* 0                                                                    */
} RtsPattern;
/* Per-pulse parameters of the pattern finalisation. */
typedef struct RtsPatternPulse {
    double wavelength, carrier, cspeed;
    const double* rx_position;   /* [n_rx][3] receiver positions                                         */
    const double* rx_rotation;   /* [n_rx][4] az, el at the pulse time, az_rate, el_rate (rad/s)          */
} RtsPatternPulse;
/* Validates every table (finite values >= 0, ascending samples, size limits, known kind and flags) -- on failure
 * RTS_ERR_INVALID and the handle keeps its previous tables -- and packs them into one device buffer of the handle (the caller's
 * arrays are free on return).  Waits for the handle's enqueued work that may still read the previous tables.
 * tx: the transmitter; rx[n_rx] one per receiver (in rts_set_receivers order); rcs[n_targets] one per target. */
int rts_set_patterns(RtsHandle h, const RtsPattern* tx, const RtsPattern* rx, uint32_t n_rx, const RtsPattern* rcs,
                     uint32_t n_targets);
/* rts_finalise_uniform with the patterns: same place in the call sequence, same implicit end of a begun pulse.
 * RTS_ERR_INVALID when no patterns are set, when their n_rx / n_targets differ from the handle's receivers / scene, or when the
 * handle's received set is not a traced pulse's (e.g. after rts_kernel_wrapper_on). */
int rts_finalise_patterns(RtsHandle h, const RtsPatternPulse* pulse);
/* rts_trace_pulse_end_uniform with the pattern finalisation (same speculation, same results as the four calls). */
int rts_trace_pulse_end_patterns(RtsHandle h, const RtsPatternPulse* pulse, int32_t cube_pulse, uint64_t recv_index_base);
/* Pure host: validates *p and evaluates it at n points (u[i], v[i]) -> out[i].  No device needed. */
int rts_pattern_eval(const RtsPattern* p, const double* u, const double* v, uint32_t n, double* out);

/* rts_aggregate: myKernel1 + myKernel2 + unique paths (aggregation.cu:32-97,
 * ray_tracer.cpp:1283-1292) on the device-resident received set, as a sort/group-by.
 * recv_index_base offsets the received-list indices (multi-GPU with contiguous ranges: number of received
 * rays on lower ranks).  RTS_BASE_USE_ROWS makes RtsGroup.min_ray the GLOBAL BUFFER ROW (launch index + k W^3)
 * of the group's first ray instead: rows order rays exactly as received-list indices do, and they are comparable
 * across ranks whatever the sharding (interleaved tiles).
 * Rays are grouped by a packed (receiver, path) key of D x ceil(log2(targets + 1)) + ceil(log2(receivers)) bits,
 * D = max_refl + max_refr: one 64-bit radix sort when that fits 64 bits (every BASELINE configuration: C3 6 x 1 + 2,
 * C4 8 x 3 + 3), two or three stable passes over 64-bit words otherwise (e.g. 16 bounces in a scene of 100 targets: 115 bits). */
#define RTS_BASE_USE_ROWS 0xffffffffffffffffULL
int rts_aggregate(RtsHandle h, double cspeed, double carrier, uint64_t recv_index_base);
int rts_group_count(RtsHandle h, uint32_t* count);
int rts_get_groups(RtsHandle h, RtsGroup* groups, uint32_t capacity);
/* Per-ray aggregation outputs of the last rts_aggregate (what kernel_wrapper returns). */
int rts_get_aggregated(RtsHandle h, struct PerRayData* rays, double* delay, double* phase, int32_t* path_match,
                       uint64_t capacity);

/* Host-side: merge group tables (concatenated from several GPUs) and derive the responses
 * that ray_tracer.cpp:1290-1321 would emit.  Pure host code, no device needed. */
int rts_merge_groups(const RtsGroup* in, uint32_t n_in, uint32_t depth, RtsGroup* out, uint32_t* n_out);
int rts_groups_to_responses(const RtsGroup* groups, uint32_t n_groups, RtsResponse* out, uint32_t capacity,
                            uint32_t* n_out);

/* ---------------------------------------------------------------- complex return cube (derived product)
 * Not in the reference (SOARS' rsresponse renders the responses); the north star asks for "atomic complex
 * accumulation into per-receiver range-Doppler bins" with an RCCL reduce of the per-receiver return buffers.
 * cube[rx][pulse][bin] (complex128, interleaved re/im) += sqrt(power) * exp(j * phase) for every received,
 * finalised ray of the last pulse, with delay = rayLength / c, phase = -fmod(2 pi fc delay, 2 pi) (the phase
 * convention of aggregation.cu:59-60) and bin = floor((delay - t0) / dt); rays outside [0, n_bins) are dropped.
 * The storage may be caller-owned DEVICE memory (device_ptr != NULL, e.g. a torch tensor that is then
 * all-reduced over RCCL) or library-owned (device_ptr == NULL). */
typedef struct RtsCubeParams {
    uint32_t n_rx, n_pulses, n_bins, reserved;
    double t0, dt;
} RtsCubeParams;
int rts_cube_attach(RtsHandle h, const RtsCubeParams* params, void* device_ptr);
int rts_cube_accumulate(RtsHandle h, uint32_t pulse_index, double cspeed, double carrier);
int rts_cube_get(RtsHandle h, double* host_out, uint64_t capacity_doubles);
/* The same product per UNIQUE PATH instead of per received ray: one contribution per response the reference would emit for
 * the pulse (ray_tracer.cpp:1290-1321) -- sqrt(P_group) e^{j phase_group} at delay_group, the group values of
 * aggregation.cu:88-93 -- i.e. the reference's own (incoherent: mean of sqrt p, mean of wrapped phases) combination of
 * the rays of a path.  Needs rts_aggregate of the pulse on this handle.  rts_cube_accumulate is the COHERENT sum over the
 * rays (sum_i sqrt(p_i) e^{j phi_i}); the two differ by design, a caller uses one of them per cube. */
int rts_cube_accumulate_paths(RtsHandle h, uint32_t pulse_index);
/* Slow-time (Doppler) transform: for every receiver and range bin the n_fft-point DFT over the pulse axis, n_fft a power
 * of two with n_pulses <= n_fft <= 4096 (pulses beyond n_pulses count as zeros):
 *     out[rx][k][bin] = sum_p cube[rx][p][bin] e^{-2 pi j k p / n_fft}          (complex128, [n_rx][n_fft][n_bins])
 * device_out: caller-owned device memory of 2 n_rx n_fft n_bins doubles, or NULL: library-owned (rts_cube_doppler_get).
 * The map lives until the next rts_cube_doppler, rts_cube_attach or rts_destroy: after rts_cube_attach, rts_cube_doppler_get
 * returns RTS_ERR_INVALID and rts_cube_detect without a map of its own has none. */
int rts_cube_doppler(RtsHandle h, uint32_t n_fft, void* device_out);
int rts_cube_doppler_get(RtsHandle h, double* host_out, uint64_t capacity_doubles);

/* ---------------------------------------------------------------- received signal: waveform render and range compression
 * What SOARS does with the responses the reference hands it (ray_tracer.cpp:1311-1320): render them with the pulse's waveform.
 * A waveform is M complex baseband samples s[0..M-1] at the cube's sample interval dt, and an interpolation length L.  Its
 * continuous envelope at x (in samples) is
 *     s(x) = sum_{m=0}^{M-1} s[m] h_L(x - m)
 *   L = 1       sample-and-hold: h_1(u) = 1 for -1 < u <= 0, else 0 (sample m lands in output sample floor(d) + m: the bin of
 *               rts_cube_accumulate)
 *   L even, 2 .. 64   windowed sinc: h_L(u) = sinc(u) w(u) for |u| < L/2, else 0; sinc(u) = sinpi(u) / (pi u), h_L(0) = 1 exactly
 *               (so an on-grid delay reproduces the samples bit for bit); Blackman w(u) = 0.42 + 0.5 cos(2 pi u / L) + 0.08 cos(4 pi u / L)
 * Each contribution k -- amplitude a_k = sqrt(P_k) e^{j phi_k}, delay tau_k, Doppler frequency f_k, fractional start
 * d_k = (tau_k - t0) / dt -- adds to output sample n of the row (rx_k, pulse):
 *     y[n] += a_k s(n - d_k) e^{j 2 pi f_k (n - d_k) dt}          (f_k = 0 without RTS_RENDER_DOPPLER)
 * Samples outside [0, n_bins) are dropped.  The contributions are those of the two accumulations above:
 *   RTS_RENDER_RAYS   every received ray of the last pulse, as rts_cube_accumulate takes it: P its power, tau = rayLength / cspeed,
 *                     phi = -fmod(2 pi carrier tau, 2 pi), f its Doppler.  (After rts_aggregate -- and after the fused pulse ends,
 *                     which aggregate -- the rays carry their group's power and Doppler, aggregation.cu:88-93; render before it for
 *                     the finalised per-ray values.)
 *   RTS_RENDER_PATHS  the representative of each group of the pulse's rts_aggregate, as rts_cube_accumulate_paths takes it: the
 *                     group's power, delay, phase and Doppler.  cspeed and carrier are not used.
 * The render is a gather: per (receiver, tile of output samples) the contributions are summed in the received set's order,
 * then each sample is added to the cube with one atomic add -- handles that share a cube stay safe, and one handle's render
 * into a zeroed row is bit-reproducible.  Rendering is linear: rts_cube_reduce (and an all-reduce of caller-owned cubes) sums
 * rendered cubes as they are.
 * Range compression (matched filter), in place on the rows of the cube:
 *     z[n] = sum_{m=0}^{M-1} y[n + m] conj(s[m]),   y[j] = 0 for j >= n_bins
 * (an on-grid response at n0 peaks at z[n0] = a sum |s[m]|^2).  One workgroup holds a whole row in LDS: n_bins <= 8 192
 * (128 KiB of complex128 of the 160 KiB a gfx950 workgroup may allocate). */
#define RTS_RENDER_RAYS 0u
#define RTS_RENDER_PATHS 1u
#define RTS_RENDER_DOPPLER 1u
#define RTS_WAVEFORM_MAX_SAMPLES 4096u     /* the render stages the whole waveform in LDS: 64 KiB of complex128 */
#define RTS_WAVEFORM_MAX_TAPS 64u
#define RTS_COMPRESS_MAX_BINS 8192u
typedef struct RtsWaveform {
    const double* samples;       /* [n_samples] interleaved re / im, finite                         */
    uint32_t n_samples;          /* 1 .. RTS_WAVEFORM_MAX_SAMPLES                                   */
    uint32_t taps;               /* L: 1, or even in [2, RTS_WAVEFORM_MAX_TAPS]                     */
    uint64_t reserved[2];        /* 0                                                               */
} RtsWaveform;
/* Validates *w -- on failure RTS_ERR_INVALID and the handle keeps its previous waveform -- and copies it into a device buffer of
 * the handle (the caller's array is free on return).  Waits for the handle's enqueued work that may still read the previous one. */
int rts_cube_set_waveform(RtsHandle h, const RtsWaveform* w);
/* Renders the last pulse's contributions (source RTS_RENDER_RAYS / RTS_RENDER_PATHS; flags 0 or RTS_RENDER_DOPPLER) into row
 * pulse_index of every receiver of the attached cube, with the handle's waveform.  Works after every pulse end after which
 * rts_cube_accumulate works; RTS_RENDER_PATHS needs rts_aggregate of the pulse (or a fused pulse end, which aggregates). */
int rts_cube_render(RtsHandle h, uint32_t pulse_index, uint32_t source, uint32_t flags, double cspeed, double carrier);
/* Range-compresses rows first_pulse .. first_pulse + n_pulses - 1 of every receiver in place, with the handle's waveform. */
int rts_cube_compress(RtsHandle h, uint32_t first_pulse, uint32_t n_pulses);
/* Pure host: validates *w and evaluates its envelope s(x[i]) -> out[2 i], out[2 i + 1] (re, im); x outside the support or not
 * finite gives 0.  No device needed. */
int rts_waveform_eval(const RtsWaveform* w, const double* x, uint32_t n, double* out);

/* ---------------------------------------------------------------- receiver noise and CFAR detection on the range-Doppler map
 * Receiver noise: circular complex Gaussian samples with E|n|^2 = noise_power added to rows first_pulse .. first_pulse + n_pulses - 1
 * of every receiver of the attached cube.  Sample i -- the cube's flat index i = (rx n_pulses_cube + pulse) n_bins + bin -- is a
 * pure function of (seed, i), whatever the launch shape and however the rows are split across calls:
 *     Philox4x32-10 (multipliers 0xD2511F53, 0xCD9E8D57; Weyl constants 0x9E3779B9, 0xBB67AE85), counter (lo32(i), hi32(i), 0, 0),
 *     key (lo32(seed), hi32(seed)), output words x0..x3;
 *     a = (x0 << 32 | x1) >> 11, u1 = (a + 1) 2^-53 in (0, 1];  b = (x2 << 32 | x3) >> 11, u2 = b 2^-53;
 *     r = sqrt(-2 ln u1);  re += sqrt(noise_power / 2) r cos(2 pi u2),  im += sqrt(noise_power / 2) r sin(2 pi u2).
 * A plain read-add-write of the rows (no atomics), ordered on the handle's stream.  noise_power finite and >= 0; 0 is a no-op.
 *   * Add noise after the render and before rts_cube_compress: that is where thermal noise enters a receiver.
 *   * With several GPUs add it ONCE, on one handle, after rts_cube_reduce or the caller's all-reduce -- otherwise it is summed N times.
 * rts_noise_eval: pure host, the same generator (rts_noise.h): out[2 j], out[2 j + 1] = the noise sample of flat index index[j]. */
int rts_cube_add_noise(RtsHandle h, uint32_t first_pulse, uint32_t n_pulses, double noise_power, uint64_t seed);
int rts_noise_eval(uint64_t seed, const uint64_t* index, uint32_t n, double noise_power, double* out);

/* ---------------------------------------------------------------- clutter and jammer sources: correlated Gaussian patches
 * One call adds K = n_patches statistically independent patches to EVERY row of the attached cube.  One first-order complex
 * autoregression per patch and range bin covers ground clutter, clutter with internal motion and barrage jammers.  Patch k has
 *   spatial[k][rx]  its response on the receivers (complex128).  For a far-field patch this is its rts_steering_make row: a plane
 *                   wave's snapshot equals its steering row;
 *   power[k] >= 0   its mean power;
 *   doppler[k]      its Doppler in cycles per pulse;
 *   rho[k]          its pulse-to-pulse correlation in [0, 1] (NULL: all 1).  rho = 1 with the ridge's Doppler is ground clutter;
 *                   rho slightly below 1 is clutter with internal motion (a Lorentzian line of that width); rho = 0 is a noise
 *                   jammer, white in slow and fast time and of rank one across the receivers;
 * and range_profile[bin] >= 0 (NULL: all 1) scales the power per bin: range law, swath gate, jammer blanking.
 *     pole_k = rho_k (cos 2 pi f, sin 2 pi f),  f = doppler_k - floor(doppler_k)       on the host: the exact reflections about 1 and
 *                                                                                      1/2, then libm (rts_steering_make's rule)
 *     g_k    = sqrt(1 - rho_k rho_k)                                                   on the host
 *     s_kr   = sqrt(power_k * profile_r)                                               IEEE sqrt, the same bits on both sides
 *     w(k,r,p) = the generator of rts_cube_add_noise above with sqrt(noise_power / 2) = sqrt(0.5) (unit power), key
 *                (lo32(seed), hi32(seed)) and Philox counter (r, p, k, 1): the fourth word keeps these draws apart from
 *                rts_cube_add_noise's (counter (lo, hi, 0, 0)) under the same seed
 *     c_kr0  = s_kr w(k,r,0)                                                           (s wr, s wi)
 *     c_krp  = pole_k (x) c_kr,p-1 + (g_k * s_kr) w(k,r,p)                             a (x) b = (ar br - ai bi, ar bi + ai br);
 *              when g_k == 0 the second term is not formed and no draw is made
 *     cube[rx][p][r] += sum_k spatial[k][rx] (x) c_krp
 * Fixed trees of IEEE basic operations without contraction, apart from the draw's log, cos and sin (OCML on the device, libm on
 * the host: a few ulp).  The sum runs in ONE order, whatever the launch shape:
 *   * partial j (0 <= j < 64) adds the terms of the patches k = j, j + 64, j + 128, .. in ascending k; its first term is the start value;
 *   * the 64 partials then combine as j with j + 32 (j < 32), then + 16, + 8, + 4, + 2, + 1: partial j = partial j + partial (j + s);
 *   * a partial without a patch is left out of the tree, it is not added as zero: where only partial j + s exists it becomes partial j;
 *   * the total is added to the cube sample by one plain read-add-write.  No atomics -- the rule of rts_cube_add_noise.
 * The recursion always starts at pulse 0 of the cube and covers all n_pulses rows: there is no row range.  A bin with
 * profile_r == 0 is neither read nor written.  A patch with power_k == 0 is skipped: it brings no term to its partial (a partial
 * whose patches are all skipped is a partial without a patch) and makes no draw; with every patch skipped nothing is written.
 * By construction E|c_krp|^2 = power_k profile_r for every p, and E[c_krp conj(c_kr,p-1)] = pole_k power_k profile_r.
 *   * The bins are independent.  Added after rts_cube_compress a patch set is clutter at the range resolution; added before, the
 *     waveform's autocorrelation spreads it -- the right place for a jammer.
 *   * With several GPUs add it ONCE, on one handle, after rts_cube_reduce -- the rule of the noise.
 *   * Geometry that changes with range is several calls with different range_profile gates; calls with disjoint gates equal one
 *     call with their union, byte for byte.
 * Out of scope: range-correlated clutter, non-Gaussian (K-distributed) amplitude, deriving patch tables from a terrain mesh.
 * rts_cube_add_sources is enqueued on the handle's stream; the tables go through one staged upload and the caller's arrays are
 * free on return.  RTS_ERR_INVALID, naming the field, and the cube and the handle untouched: no cube attached; a NULL p, spatial,
 * power or doppler; flags or reserved fields not 0; n_patches 0 or above RTS_SRC_MAX_PATCHES; n_rx above RTS_BEAM_MAX_RX;
 * n_patches * n_rx above RTS_SRC_MAX_TABLE; an entry that is not finite; a negative power or profile; a rho outside [0, 1]; cube
 * memory that is not 16-byte aligned.
 * rts_sources_eval: pure host, the same rules (rts_source.h) on a host array [n_rx][n_pulses][n_bins] (interleaved re / im) that
 * it adds to in place, *q standing in for the attached cube; the same validation, and the array untouched when it refuses. */
#define RTS_SRC_MAX_PATCHES 1024u
#define RTS_SRC_MAX_TABLE   4096u   /* bounds n_patches * n_rx: the spatial table, 64 KiB of complex128, sits in LDS */
typedef struct RtsSourceParams {
    uint32_t n_patches, flags;        /* 1 .. RTS_SRC_MAX_PATCHES; flags 0 */
    const double* spatial;            /* host [n_patches][n_rx] interleaved re / im, finite */
    const double* power;              /* host [n_patches], finite, >= 0 */
    const double* doppler;            /* host [n_patches], finite, cycles per pulse */
    const double* rho;                /* host [n_patches] in [0, 1], or NULL: all 1 */
    const double* range_profile;      /* host [n_bins], finite, >= 0, or NULL: all 1 */
    uint64_t seed, reserved[2];
} RtsSourceParams;                    /* 72 bytes */
int rts_cube_add_sources(RtsHandle h, const RtsSourceParams* p);
int rts_sources_eval(const RtsCubeParams* q, const RtsSourceParams* p, double* cube_inout);

/* CFAR detection.  Input z[rx][k][r], complex128 [n_rx][n_doppler][n_bins] (n_rx, n_bins of the attached cube): the handle's last
 * rts_cube_doppler output (device_map NULL; n_doppler is then its n_fft and the argument is ignored) or a caller device pointer
 * (n_doppler >= 1 required, any value).  Cell power P = re re + im im.
 *   Window: the training cells of a cell under test (CUT) are the offsets (dk, dr) with |dk| <= Gd + Td, |dr| <= Gr + Tr, minus the
 *     guard rectangle |dk| <= Gd, |dr| <= Gr (which holds the CUT).  The Doppler axis is circular (the DFT is periodic) and wraps;
 *     the range axis is not: training cells outside [0, n_bins) are dropped, so their number N varies near the range edges.
 *   Noise: CA the mean of the N training cells; GO / SO the larger / smaller of the means of the cells with dr < 0 and with dr > 0
 *     (dr = 0 belongs to neither; a half that is empty at a range edge yields to the other).  Every estimate is a direct sum of
 *     the training powers -- never a difference of box sums -- so a cell 10^12 above the noise beside a CUT costs it no accuracy.
 *   Threshold alpha noise.  With pfa (CA only) each cell uses alpha = N (pfa^(-1/N) - 1), the exact CA threshold for square-law
 *     detection of complex Gaussian noise: the false-alarm rate is pfa at the range edges too.
 *   Detection: P > threshold; with RTS_CFAR_LOCAL_MAX also a 3 x 3 local maximum (Doppler wrapped, range truncated): strictly greater
 *     than each neighbour whose offset (dk, dr) is lexicographically below (0, 0), >= each one above it (one detection per plateau).
 *     The wrap is applied as it stands, also on a map too short for it: with n_doppler = 2 both Doppler offsets name the same row,
 *     and with n_doppler = 1 they name the cell's OWN row -- the neighbour (-1, 0) is then the cell itself, "strictly greater" never
 *     holds, and NO cell is reported.  That is the rule's consequence and it is kept (a one-row map has no Doppler axis to be a
 *     maximum along): detect on a single-row map without RTS_CFAR_LOCAL_MAX.
 *   Refinement: per axis a parabola through ln P of the two neighbours, delta = (ln P- - ln P+) / (2 (ln P- - 2 ln P0 + ln P+))
 *     clamped to [-0.5, 0.5]; 0 when a neighbour is missing (range edge), a power is <= 0 or the denominator is >= 0.
 *     delay = t0 + (range_bin + range_offset) dt; doppler = w / (n_doppler pri) with w = doppler_bin + doppler_offset wrapped into
 *     [-n_doppler / 2, n_doppler / 2) (0 when pri is 0).  Sign: with the cube's phase -2 pi fc tau and the transform's e^{-2 pi j k p / n},
 *     a CLOSING range (tau falling from pulse to pulse) gives a POSITIVE Doppler, fc |d tau / d pulse| / pri.
 *   Output: the list in ascending flat order (rx, doppler_bin, range_bin), bit-identical from run to run (the order comes from
 *     counts and a scan, never from atomics).  rts_cube_detect never waits on the host: it writes up to max_detections records and
 *     the total count to device buffers of the handle, which live until the next rts_cube_detect, rts_cube_attach or rts_destroy.
 *     rts_cube_detections_get synchronises, sets *n_out to the total and copies min(total, stored, capacity) records; it returns
 *     RTS_ERR_CAPACITY when that is fewer than the total, RTS_ERR_INVALID after an rts_cube_attach.
 *   RTS_ERR_INVALID, the message naming the field: no cube or no map; unknown mode or flags; nonzero reserved fields; Tr + Td = 0;
 *     Gr + Tr or Gd + Td > RTS_CFAR_MAX_HALF; 2 (Gd + Td) + 1 > n_doppler; Gr + Tr >= n_bins; pfa outside (0, 1); both or neither
 *     of pfa and alpha (alpha > 0 and finite); GO / SO with pfa or with Tr = 0; pri negative or not finite. */
#define RTS_CFAR_CA 0u          /* cell averaging                                    */
#define RTS_CFAR_GO 1u          /* greatest-of the two range halves                  */
#define RTS_CFAR_SO 2u          /* smallest-of                                       */
#define RTS_CFAR_LOCAL_MAX 1u   /* flag: report only 3x3 local maxima                */
#define RTS_CFAR_MAX_HALF 16u   /* guard + train per side, per axis                  */
typedef struct RtsCfarParams {
    uint32_t guard_range, guard_doppler, train_range, train_doppler;   /* cells on EACH side of the cell under test */
    uint32_t mode, flags;
    double pfa;              /* CA only: (0, 1) -> alpha per cell from its own training count; 0: use alpha   */
    double alpha;            /* > 0 when pfa == 0 (required for GO / SO)                                      */
    double pri;              /* pulse repetition interval for RtsDetection.doppler; 0: doppler = 0            */
    uint32_t max_detections; /* device list length; 0: 65 536                                                 */
    uint32_t reserved0; uint64_t reserved[2];                                         /* 0 */
} RtsCfarParams;
typedef struct RtsDetection {
    uint32_t rx, doppler_bin, range_bin, n_train;
    double power, noise, threshold;           /* |z|^2 of the cell, the noise estimate, alpha * noise     */
    double range_offset, doppler_offset;      /* sub-bin refinement, bins, in [-0.5, 0.5]                 */
    double delay, doppler;                    /* t0 + (range_bin + range_offset) dt;  Hz                  */
} RtsDetection;                               /* 72 bytes */
#define RTS_CFAR_DEFAULT_MAX_DETECTIONS 65536u
int rts_cube_detect(RtsHandle h, const RtsCfarParams* p, const void* device_map, uint32_t n_doppler);
int rts_cube_detections_get(RtsHandle h, RtsDetection* out, uint32_t capacity, uint32_t* n_out);

/* ---------------------------------------------------------------- ordered-statistic (OS) CFAR detection on the range-Doppler map
 * The detector above with the noise estimated by a RANK of the training powers instead of their mean: the estimate stays put until
 * k of a cell's N training cells are contaminated, so a strong return (another target, a multi-bounce path a few bins away, a
 * blade flash along Doppler) in a neighbour's window does not lift that neighbour's threshold by P / N and hide it.  Its own entry
 * point and parameter record: rts_cube_detect keeps refusing modes above RTS_CFAR_SO.  The arithmetic is rts_amd/csrc/rts_cfar_os.h,
 * shared by the kernel (rts_detect.hip) and the host evaluator; what it takes unchanged from rts_cube_detect is rts_amd/csrc/rts_cfar.h.
 *   Taken unchanged from rts_cube_detect: the input map (the handle's last rts_cube_doppler output, or a caller device pointer, 16-byte
 *     aligned, with n_doppler >= 1); the window (the training annulus |dk| <= Gd + Td, |dr| <= Gr + Tr minus the guard rectangle,
 *     Doppler wrapped, range truncated, so N varies near the range edges); RTS_CFAR_LOCAL_MAX, including its behaviour on one-row and
 *     two-row maps; the refinement, the delay and doppler fields and the Doppler sign; the output order, flat (rx, doppler_bin,
 *     range_bin), from counts and a scan, never from atomics; RtsDetection, max_detections, RTS_CFAR_DEFAULT_MAX_DETECTIONS.
 *     rts_cube_detect_os never waits on the host.  Its list shares the handle's detection buffers and is read with
 *     rts_cube_detections_get; a later rts_cube_detect, rts_cube_detect_os, rts_cube_attach or rts_destroy ends it.
 *   Window size and rank: a full window holds N0 = (2 (Gr + Tr) + 1) (2 (Gd + Td) + 1) - (2 Gr + 1) (2 Gd + 1) training cells
 *     (at most RTS_CFAR_OS_MAX_TRAIN) and `rank` = k0 in [1, N0] is the rank in a full window.  A cell with N training cells uses the
 *     rank k = (rank N + N0 - 1) / N0 in integer arithmetic, the ceiling of rank N / N0; it is at least 1 because N >= 1 under the
 *     validation rules.
 *   Noise, threshold, detection: noise is the k-th smallest (1-based) of the N training powers P = re re + im im; threshold =
 *     alpha noise, one multiply; a cell is detected when P > threshold (and, with RTS_CFAR_LOCAL_MAX, is a local maximum).
 *     RtsDetection.noise is that order statistic -- one of the map's own powers, bit for bit -- and n_train is N.  Powers are assumed
 *     finite or +inf; with a NaN in the map which cells are reported is unspecified, but nothing is read out of bounds.
 *   pfa: each cell uses alpha(N, k), the root of prod_{i=0}^{k-1} (N - i) / (N - i + alpha) = pfa, the exact OS false-alarm law for
 *     square-law detected complex Gaussian noise: the rate is pfa at the range edges too.  rts_cfar_os_alpha (pure host; n_train = N,
 *     rank = k) returns that root such that the product, re-evaluated at the returned alpha, is within 1e-11 relative of pfa
 *     (rounding alpha moves ln of the product by at most k 2^-53, about 1.2e-13; a checker evaluating k <= 1 088 factors adds about
 *     3 k 2^-53, about 3.6e-13; 1e-11 leaves a factor of 20 over the sum).  The device path and rts_cfar_os_eval take their alphas
 *     from this one function -- rts_cube_detect_os computes them on the host for the values of N that occur and passes them as a
 *     table -- so their thresholds are equal bit for bit.
 *   rts_cfar_os_eval: pure host, the same detector on a host map [n_rx][n_doppler][n_bins] (complex128, interleaved) with q (n_rx,
 *     n_bins, t0, dt; n_pulses is not used) in place of the attached cube: up to `capacity` records to out in the same order, the
 *     total to *n_out.  Integer fields, power, noise and threshold equal the device's bit for bit; the refinement fields to the
 *     rounding of log.
 *   RTS_ERR_INVALID, the message naming the field: everything rts_cube_detect refuses on the shared fields (no cube or no map;
 *     unknown flags; nonzero reserved fields; Tr + Td = 0; Gr + Tr or Gd + Td > RTS_CFAR_MAX_HALF; 2 (Gd + Td) + 1 > n_doppler;
 *     Gr + Tr >= n_bins; pfa outside (0, 1); both or neither of pfa and alpha (alpha > 0 and finite); pri negative or not finite);
 *     rank = 0 or rank > N0.  rts_cfar_os_alpha refuses n_train = 0, rank = 0, rank > n_train, pfa outside (0, 1) and a NULL output.
 *     rts_cfar_os_eval applies the same validation and also refuses NULL arguments (out may be NULL when capacity is 0); a refused
 *     call leaves out untouched.  It returns RTS_ERR_CAPACITY, with *n_out the total and the first `capacity` records written, when
 *     capacity is too small. */
#define RTS_CFAR_OS_MAX_TRAIN 1088u        /* (2*16+1)^2 - 1 */
typedef struct RtsCfarOsParams {
    uint32_t guard_range, guard_doppler, train_range, train_doppler;   /* cells on EACH side of the cell under test */
    uint32_t rank;           /* k0 in [1, N0]: the rank in a FULL window of N0 training cells                  */
    uint32_t flags;          /* RTS_CFAR_LOCAL_MAX                                                            */
    double pfa;              /* (0, 1) -> alpha per cell from its own training count and rank; 0: use alpha   */
    double alpha;            /* > 0 when pfa == 0                                                             */
    double pri;              /* pulse repetition interval for RtsDetection.doppler; 0: doppler = 0            */
    uint32_t max_detections; /* device list length; 0: 65 536                                                 */
    uint32_t reserved0; uint64_t reserved[2];                                         /* 0 */
} RtsCfarOsParams;                            /* 72 bytes */
int rts_cube_detect_os(RtsHandle h, const RtsCfarOsParams* p, const void* device_map, uint32_t n_doppler);
int rts_cfar_os_alpha(uint32_t n_train, uint32_t rank, double pfa, double* alpha);
int rts_cfar_os_eval(const RtsCubeParams* q, const double* map, uint32_t n_doppler, const RtsCfarOsParams* p,
                     RtsDetection* out, uint32_t capacity, uint32_t* n_out);

/* ---------------------------------------------------------------- plot extraction: detections clustered into target plots
 * The detectors above report CELLS; an extended body (a skin return and its multi-bounce paths, a blade flash along Doppler) crosses
 * the threshold in tens to thousands of them.  rts_cube_plots clusters a detection list into PLOTS -- the connected components of an
 * adjacency on the map -- on the device, and writes one record per plot: power-weighted centroid, extent, peak and summed power.
 * Detect WITHOUT RTS_CFAR_LOCAL_MAX, then extract plots.  The rules are rts_amd/csrc/rts_plot.h, shared by the kernels
 * (rts_plot.hip) and the host evaluator rts_plots_eval, which agree bit for bit.
 *   Input: a detection list in ascending flat order (rx, doppler_bin, range_bin) with no cell twice -- what both detectors write.
 *     device_list NULL: the handle's list, the first min(total, stored) records, with the n_doppler of the map it was detected on
 *     (the detect call records it).  Otherwise a caller-owned DEVICE array of n_list RtsDetection on a map of n_doppler rows and the
 *     attached cube's n_bins; it is taken as given: a list that breaks the ordering rule makes the plots unspecified, but nothing is
 *     read or written outside the list and the output buffers.  rts_plots_eval checks the ordering and the bin ranges and refuses a
 *     list that breaks them.
 *   Adjacency: two detections of the same rx are adjacent when |r - r'| <= link_range and an integer dk with |dk| <= link_doppler and
 *     (k + dk) mod n_doppler == k' exists, and they are not the same cell.  Doppler wraps, range does not, receivers never join.  As
 *     in the CFAR section the wrap is applied as it stands on short maps: with 2 link_doppler + 1 > n_doppler rows are simply named
 *     more than once.  link = (0, 0) makes every detection its own plot.  A plot is a connected component of this relation.
 *   Identity and order: a plot's first_index is the smallest list index among its cells (its ROOT); plots are written in ascending
 *     first_index.  Plots of fewer than min_cells cells are removed after the components are formed, so the survivors keep their
 *     relative order.  Output positions come from flags and a scan, never from atomics, and two runs on one list give the same bytes.
 *   Record: with the root at cell (k0, r0), member i has dr_i = r_i - r0 and dk_i = k_i - k0 wrapped into [-n_doppler / 2, n_doppler / 2)
 *     in integer arithmetic -- a component wider than half the Doppler circle is mis-unwrapped (its far members land on the wrong
 *     side of the root); that is a documented limit, not repaired.  With P_i the detection's power: S = sum P_i, S_r = sum P_i dr_i,
 *     S_k = sum P_i dk_i, S_rr = sum P_i dr_i^2, S_kk = sum P_i dk_i^2 (the square formed first), noise_sum = sum noise_i; each product
 *     is rounded before it is added (no contraction).  The ORDER of every sum is a pure function of the member count: members in
 *     ascending list index, added left to right from 0 inside blocks of 64 consecutive members, the block sums added left to right
 *     from 0.  Then
 *       range_centroid = (double)r0 + S_r / S;  doppler_centroid = w = (double)k0 + S_k / S wrapped into [-n_doppler / 2, n_doppler / 2)
 *       exactly as RtsDetection's w;  delay = t0 + range_centroid dt;  doppler = w / (n_doppler pri) (0 when pri is 0);
 *       range_spread, doppler_spread = sqrt(max(0, S_xx / S - (S_x / S)^2)), the power-weighted standard deviation in bins;
 *       range_min, range_max over the members;  doppler_lo = (k0 + min dk) mod n_doppler, doppler_span = min(n_doppler, max dk - min dk + 1):
 *       the Doppler extent is the circular interval doppler_lo .. doppler_lo + doppler_span - 1 mod n_doppler;
 *       peak_index = the member of largest power, ties to the lowest index;  power_sum = S.
 *     A plot of ONE cell takes that detection's own refinement: range_centroid = (double)r + range_offset, w from k + doppler_offset,
 *     both spreads 0, delay and doppler by the very expressions of RtsDetection -- so a RTS_CFAR_LOCAL_MAX list with link = (0, 0)
 *     passes through with delay and doppler equal to its detections' bit for bit.  S <= 0 (all powers zero): centroids at the root,
 *     spreads 0.
 *   Lifetime: rts_cube_plots never waits on the host: it sizes its launches by the list's capacity and reads the count on the device.
 *     The plots index the detection list and live until the next rts_cube_plots, rts_cube_detect, rts_cube_detect_os,
 *     rts_cube_attach or rts_destroy.  rts_cube_plots_get synchronises, sets *n_out to the total and copies min(total, stored,
 *     capacity) records.  It returns RTS_ERR_CAPACITY when fewer records were copied than the total, when max_plots cut the device
 *     list, and when the detection list the plots were made from was itself truncated (the plots then describe the stored prefix);
 *     RTS_ERR_INVALID when no plots exist.
 *   rts_plots_eval: pure host, the same plots of a host list on a map of q->n_rx x n_doppler x q->n_bins cells (q: n_rx, n_bins, t0,
 *     dt; n_pulses is not used): up to `capacity` records to out, the total to *n_out, RTS_ERR_CAPACITY when capacity is too small.
 *     Of p it uses link_range, link_doppler, min_cells and pri; the other fields are validated and otherwise ignored.
 *   RTS_ERR_INVALID, the message naming the field: no cube; no detection list and no device_list; link_range or link_doppler above
 *     RTS_PLOT_MAX_LINK; nonzero reserved fields; pri negative or not finite; device_list with n_doppler = 0 or not 8-byte aligned;
 *     n_list or n_doppler nonzero without device_list.  rts_plots_eval additionally refuses NULL arguments (out may be NULL when
 *     capacity is 0), n_doppler = 0, a list out of order and bins outside the map; a refused call leaves out untouched. */
#define RTS_PLOT_MAX_LINK 4u
typedef struct RtsPlotParams {
    uint32_t link_range, link_doppler;   /* 0 .. RTS_PLOT_MAX_LINK: reach of the adjacency, cells, per axis            */
    uint32_t min_cells;                  /* plots of fewer cells are dropped; 0 is taken as 1                          */
    uint32_t max_plots;                  /* device list length; 0: as many as the detection list can hold              */
    double pri;                          /* as RtsCfarParams.pri: for RtsPlot.doppler; 0: doppler = 0                   */
    const void* device_list;             /* NULL: the handle's detection list; else caller-owned DEVICE RtsDetection[] */
    uint32_t n_list, n_doppler;          /* with device_list: its length and the map's Doppler rows (>= 1); else 0      */
    uint64_t reserved[2];                /* 0 */
} RtsPlotParams;                                              /* 56 bytes */
typedef struct RtsPlot {
    uint32_t rx, n_cells, first_index, peak_index;            /* indices into the detection list                          */
    uint32_t range_min, range_max, doppler_lo, doppler_span;  /* extent; Doppler circular: doppler_lo .. +span-1 mod n    */
    double power_sum, peak_power, noise_sum;
    double range_centroid, doppler_centroid;                  /* bins; Doppler wrapped into [-n/2, n/2)                   */
    double range_spread, doppler_spread;                      /* power-weighted standard deviation, bins                  */
    double delay, doppler;                                    /* t0 + range_centroid dt;  Hz                              */
} RtsPlot;                                                    /* 104 bytes */
int rts_cube_plots(RtsHandle h, const RtsPlotParams* p);
int rts_cube_plots_get(RtsHandle h, RtsPlot* out, uint32_t capacity, uint32_t* n_out);
int rts_plots_eval(const RtsCubeParams* q, const RtsDetection* list, uint32_t n_list, uint32_t n_doppler,
                   const RtsPlotParams* p, RtsPlot* out, uint32_t capacity, uint32_t* n_out);   /* pure host */

/* ---------------------------------------------------------------- tracking: plots associated and filtered across coherent intervals
 * A plot belongs to one interval.  rts_cube_track advances a per-handle TRACK TABLE by one frame of plots, on the device and without
 * waiting on the host: per receiver a two-state Kalman filter in the plots' own coordinates (delay in seconds, Doppler in hertz),
 * gated global-nearest-neighbour association with a deterministic matching, a confirm / coast / delete lifecycle, and new tracks
 * from the plots nobody took.  The rules are rts_amd/csrc/rts_track.h, shared by the kernels (rts_track.hip) and the host evaluator
 * rts_tracks_eval, which agree bit for bit on every field.  All arithmetic is IEEE double, every product and quotient rounded on its
 * own (no contraction), in exactly the operand order written here; parentheses are evaluation order.
 *   Input: a plot list whose rx is non-decreasing -- what rts_cube_plots writes.  device_plots NULL: the handle's plots, the first
 *     min(total, stored) records, the count read on the device.  Otherwise a caller-owned DEVICE array of n_plots RtsPlot; it is taken
 *     as given: a list that breaks the rule makes the tracks unspecified, but nothing outside the list and the track buffers is
 *     touched.  Only rx, delay, doppler and power_sum are read.  A plot whose delay or doppler is not finite neither associates nor
 *     starts a track.  rts_tracks_eval refuses a list whose rx decreases.
 *   Time: T = time - the time of the previous frame (or of rts_cube_tracks_set).  The table HAS A TIME from the first rts_cube_track
 *     or an rts_cube_tracks_set of n > 0 tracks until rts_cube_tracks_reset or an rts_cube_tracks_set of none; while it has one, T
 *     must be positive and finite.  rts_tracks_eval takes T itself and asks the same when n_in > 0.
 *   Model, per track with state (d, f) and covariance (p_dd, p_df, p_ff), k = delay_rate_per_hz, a = k T.  A closing range gives a
 *     positive Doppler (the CFAR section), so the caller passes k = -1 / carrier; k = 0 decouples the axes.
 *       d- = d + a f;   f- = f
 *       u = p_df + a p_ff                                   (the off-diagonal after the first product F P)
 *       pdd- = ((p_dd + a p_df) + a u) + q (((a a) T) / 3)
 *       pdf- = u + q ((a T) / 2)
 *       pff- = p_ff + q T
 *       s_dd = pdd- + sigma_delay sigma_delay;   s_df = pdf-;   s_ff = pff- + sigma_doppler sigma_doppler
 *       det = s_dd s_ff - s_df s_df
 *   Innovation of plot (z_d, z_f):  v_d = z_d - d-;  v_f = wrap(z_f - f-).  wrap(x) with P = doppler_period > 0 and h = 0.5 P:
 *       r = x - P floor((x + h) / P);  then r - P if r >= h, r + P if r < -h (the rounding cases), so r lies in [-h, h).
 *     doppler_period = 0: wrap(x) = x.
 *       d2 = ((((v_d v_d) s_ff) - ((2 (v_d v_f)) s_df)) + ((v_f v_f) s_dd)) / det
 *   Gate: track i and plot j are an EDGE when they have the same rx, the plot is finite, and 0 <= d2 <= gate (a negative or NaN d2
 *     needs a covariance that is not positive semi-definite, which rts_cube_tracks_set refuses at its diagonal).  No cheaper
 *     pre-test stands in front of that expression.  Each track keeps its max_candidates (1 .. RTS_TRACK_MAX_CAND) edges of smallest
 *     (d2, plot index); the others are dropped BEFORE the matching.
 *   Matching: the greedy pass over the kept edges in ascending (d2, track index, plot index): an edge is taken when both its ends
 *     are free.  The device reaches the same matching by rounds of locally dominant edges (rts_track.hip) and ends the rounds itself.
 *   Update of a matched track, with K = P- S^-1:
 *       k_dd = ((pdd- s_ff) - (pdf- s_df)) / det;   k_df = ((pdf- s_dd) - (pdd- s_df)) / det
 *       k_fd = ((pdf- s_ff) - (pff- s_df)) / det;   k_ff = ((pff- s_dd) - (pdf- s_df)) / det
 *       d = d- + ((k_dd v_d) + (k_df v_f));   f = wrap(f- + ((k_fd v_d) + (k_ff v_f)))
 *       p_dd = pdd- - ((k_dd pdd-) + (k_df pdf-));  p_df = pdf- - ((k_dd pdf-) + (k_df pff-))  (once);  p_ff = pff- - ((k_fd pdf-) + (k_ff pff-))
 *     hits + 1, misses = 0, plot_index = j, d2 as above, power_sum the plot's.  RTS_TRACK_CONFIRMED is set once hits >=
 *     confirm_hits and stays set.
 *   An unmatched track COASTS: state and covariance become the prediction (d-, f-, pdd-, pdf-, pff-), misses + 1, RTS_TRACK_COASTED,
 *     plot_index = 0xffffffff, d2 = 0, power_sum = 0.  It is deleted when misses then exceeds max_misses (confirmed) or
 *     tentative_misses (not).  age + 1 in both cases; RTS_TRACK_COASTED and RTS_TRACK_NEW describe this frame only.
 *   Each finite plot no track took starts a track: state (delay, wrap(doppler)), covariance diag(sigma_delay sigma_delay,
 *     sigma_doppler sigma_doppler), hits 1, misses 0, age 1, RTS_TRACK_NEW (and RTS_TRACK_CONFIRMED when confirm_hits is 1),
 *     plot_index = j, d2 = 0, power_sum the plot's.
 *   Order and ids: the surviving tracks in their previous order, then the new ones in ascending plot index, with ids next_id,
 *     next_id + 1, .. in that order (uint64, per handle; rts_cube_tracks_reset does not rewind them).  Positions come from flags and
 *     a scan, never from atomics: two runs give the same bytes.  The table holds max_tracks records (0: RTS_TRACK_DEFAULT_TRACKS, at
 *     most RTS_TRACK_MAX_TRACKS): when it is full the survivors are kept, new tracks are stored in order until it is full, only
 *     stored tracks consume ids, and rts_cube_tracks_get returns RTS_ERR_CAPACITY.
 *   Lifetime: tracks span cubes.  They survive rts_cube_attach, the detect calls and rts_cube_plots, and end at
 *     rts_cube_tracks_reset and rts_destroy.  The step copies what it needs of the plots when it runs: the table does not refer to
 *     the plot buffers.  rts_cube_tracks_get synchronises, sets *n_out to the total (stored tracks plus the new ones a full table
 *     turned away) and *next_id_out, and copies min(stored, capacity) records; RTS_ERR_CAPACITY when that is fewer than the total.
 *     An empty table is 0 tracks, not an error.  rts_cube_tracks_set waits for the handle's stream and loads n tracks, next_id and
 *     the time they stand at; the next rts_cube_track chooses max_tracks anew (at least n).
 *   rts_tracks_eval: pure host, one step as a function: in[n_in], next_id and T to out (up to `capacity` records), *n_out (the
 *     total) and *next_id_out; the table it models holds p->max_tracks records.  device_plots and n_plots are validated and
 *     otherwise ignored.
 *   RTS_ERR_INVALID, the message naming the field, outputs and table untouched: gate, sigma_delay, sigma_doppler not finite or not
 *     positive; q negative or not finite; delay_rate_per_hz not finite; doppler_period negative or not finite; confirm_hits 0;
 *     max_candidates 0 or above RTS_TRACK_MAX_CAND; max_tracks above RTS_TRACK_MAX_TRACKS, changed since the previous
 *     rts_cube_track, or below the tracks loaded; no plots and no device_plots; n_plots without device_plots or above
 *     RTS_TRACK_MAX_PLOTS; device_plots not 8-byte aligned; nonzero reserved fields; T not positive and finite.
 *     rts_cube_tracks_set and rts_tracks_eval refuse a track whose state or covariance is not finite, whose p_dd or p_ff is
 *     negative, or whose flags hold unknown bits, and more tracks than the table holds. */
#define RTS_TRACK_MAX_CAND 16u
#define RTS_TRACK_MAX_TRACKS 65536u
#define RTS_TRACK_DEFAULT_TRACKS 16384u
#define RTS_TRACK_MAX_PLOTS 16777216u
#define RTS_TRACK_CONFIRMED 1u
#define RTS_TRACK_COASTED 2u      /* no plot this frame */
#define RTS_TRACK_NEW 4u          /* started this frame */
typedef struct RtsTrackParams {
    double gate;                         /* d2 <= gate associates (9.21: 99 % of a 2-degree-of-freedom chi-square)     */
    double sigma_delay, sigma_doppler;   /* measurement standard deviations, s and Hz, > 0                             */
    double q;                            /* Doppler random-walk intensity, Hz^2 / s, >= 0                              */
    double delay_rate_per_hz;            /* k: d(delay)/dt per hertz of Doppler; -1 / carrier by the library's signs   */
    double doppler_period;               /* Doppler is circular with this period (1 / pri); 0: not circular            */
    uint32_t confirm_hits;               /* >= 1                                                                       */
    uint32_t max_misses;                 /* a confirmed track is deleted when misses exceeds this                      */
    uint32_t tentative_misses;           /* ... a tentative one when misses exceeds this                               */
    uint32_t max_candidates;             /* 1 .. RTS_TRACK_MAX_CAND edges kept per track                               */
    uint32_t max_tracks;                 /* table size; 0: RTS_TRACK_DEFAULT_TRACKS                                    */
    uint32_t n_plots;                    /* with device_plots: its length; else 0                                      */
    const void* device_plots;            /* NULL: the handle's plots; else caller-owned DEVICE RtsPlot[]               */
    uint64_t reserved[2];                /* 0 */
} RtsTrackParams;                                             /* 96 bytes */
typedef struct RtsTrack {
    uint64_t id;
    uint32_t rx, flags;                                       /* RTS_TRACK_*                                              */
    uint32_t hits, misses, age, plot_index;                   /* plot_index: matched or initiating plot, 0xffffffff none  */
    double delay, doppler;                                    /* the state: s, Hz                                         */
    double p_dd, p_df, p_ff;                                  /* its covariance                                           */
    double d2, power_sum;                                     /* of this frame's match (0 when coasting)                  */
} RtsTrack;                                                   /* 88 bytes */
int rts_cube_track(RtsHandle h, const RtsTrackParams* p, double time);
int rts_cube_tracks_get(RtsHandle h, RtsTrack* out, uint32_t capacity, uint32_t* n_out, uint64_t* next_id_out);
int rts_cube_tracks_set(RtsHandle h, const RtsTrack* tracks, uint32_t n, uint64_t next_id, double time);
int rts_cube_tracks_reset(RtsHandle h);
int rts_cube_track_rounds(RtsHandle h, uint32_t* rounds);   /* diagnostic: rounds the last step's matching took; synchronises */
int rts_tracks_eval(const RtsTrackParams* p, const RtsTrack* in, uint32_t n_in, uint64_t next_id, double T,
                    const RtsPlot* plots, uint32_t n_plots, RtsTrack* out, uint32_t capacity, uint32_t* n_out,
                    uint64_t* next_id_out);                                                      /* pure host */

/* ---------------------------------------------------------------- multistatic localisation: the plots of several receivers to targets
 * Plots and tracks live in ONE receiver's coordinates.  A scene has one transmitter at tx and n_rx receivers at known positions
 * s_0 .. s_(n_rx-1); a target at x moving with v shows in receiver m at the bistatic delay (|x - tx| + |x - s_m|) / cspeed with the
 * Doppler -(1 / lambda) (u_t + u_m) . v, where u_t, u_m are the unit vectors from tx and s_m to x (a closing range gives a positive
 * Doppler, the sign of the CFAR section).  rts_cube_locate turns one frame of per-receiver records into TARGETS -- position,
 * velocity, the records they are made of -- on the device and without waiting on the host.  The rules are rts_amd/csrc/rts_locate.h,
 * shared by the kernels (rts_locate.hip) and the host evaluator rts_locate_eval, which agree bit for bit on every field.  All
 * arithmetic is IEEE double, every product, quotient and square root rounded on its own (no contraction), sums of three terms added
 * left to right, |a| = sqrt((a_x a_x + a_y a_y) + a_z a_z).
 *   Notation: R = cspeed delay (a record's range sum);  d_a = s_a - tx for the three ANCHOR receivers a = anchors[0 .. 2];
 *     sigma_R = cspeed sigma_delay;  lambda = cspeed / carrier (carrier = 0: no Doppler is used and every velocity is 0).
 *   Sources.  RTS_LOCATE_FROM_PLOTS: the handle's plots (device_list NULL: the first min(total, stored) records, the count read on
 *     the device) or a caller-owned DEVICE array of n_list RtsPlot whose rx does not decrease -- taken as given, as in rts_cube_track;
 *     rts_locate_eval refuses a list whose rx decreases.  Only rx, delay, doppler and power_sum are read.  RTS_LOCATE_FROM_TRACKS:
 *     the handle's track table (device_list must be NULL); only tracks that are RTS_TRACK_CONFIRMED and not RTS_TRACK_COASTED take
 *     part, through their delay, doppler and power_sum; the table is in no receiver order, so the step orders a copy by (rx, table
 *     index), and plot[] holds TABLE indices; rts_locate_eval takes a host RtsTrack[].  RTS_LOCATE_FROM_CANDIDATES: device_list is
 *     a DEVICE array of n_list RtsTarget, accepted candidates in ascending `candidate`; only the resolution (7) runs, on their
 *     n_receivers, cost and plot[] (every index below RTS_LOCATE_MAX_INDEX or 0xffffffff; an index names ONE record whatever receiver
 *     it stands at), and the other fields are copied.  It exists to hold the resolution to its definition on conflict graphs that no
 *     geometry produces on demand.  Records of a receiver >= n_rx are ignored.  A record whose delay, doppler or power_sum is not
 *     finite keeps its place in its segment but takes no part: it forms no triple and completes no candidate.
 *   1. Segments.  seg[m] is the records of receiver m in list order (tracks: in table order).  Of an anchor's segment the first
 *     P = min(size, RTS_LOCATE_MAX_PER_RX) records are used; a longer one makes rts_cube_targets_get return RTS_ERR_CAPACITY.
 *   2. Triples.  Every (i, j, k) in seg[a0] x seg[a1] x seg[a2] (positions inside the segments, below P_0, P_1, P_2):
 *     Screen: skipped when |R_a - R_b| > |s_a - s_b| for an anchor pair or R_a < |d_a| for an anchor: no point has those range sums.
 *     Equations in w = (u, r), u = x - tx, r = |u|:  d_a . u - R_a r = c_a = (|d_a|^2 - R_a R_a) / 2, a 3 x 4 system M w = c with
 *       M = [D | -R] (row a of D is d_a).
 *     Solve: M M^T = D D^T + R R^T is factored by Cholesky (lower, row by row: pivot p, l = sqrt(p), the entries below divided by l);
 *       a pivot that is not positive and finite gives no candidate.  y = (M M^T)^-1 c by the two triangular solves, w0 = M^T y:
 *       u0 = (y_0 d_0 + y_1 d_1) + y_2 d_2,  r0 = -((R_0 y_0 + R_1 y_1) + R_2 y_2).  The null vector n of M from its four 3 x 3
 *       cofactors, with X_pq the cross product of columns p and q of D:  n_x = -(R . X_12), n_y = R . X_02, n_z = -(R . X_01),
 *       n_r = -det D (det D = column 2 . X_01).  This never inverts D, so a transmitter and anchors in ONE PLANE -- the usual
 *       ground network, det D = 0 -- are solved too.  The roots of |u0 + l n_u|^2 = (r0 + l n_r)^2:  a = |n_u|^2 - n_r n_r,
 *       b = u0 . n_u - r0 n_r, q = |u0|^2 - r0 r0, disc = b b - a q; disc < 0 (or NaN) gives no candidate; t = -(b + sqrt(disc)) when
 *       b >= 0, else -(b - sqrt(disc)); l_A = t / a, l_B = q / t (the cancellation-free pair).  Each root has r = r0 + l n_r,
 *       u = u0 + l n_u, x = tx + u.  ROOT 0 is the one of smaller (r, l), root 1 the other (in a ground network both have the same
 *       r: mirror images in the plane).
 *     A root is kept when r > 0, R_a - r > 0 for the three anchors, x and r are finite, and box_lo <= x <= box_hi on every axis.
 *     The candidate index is ((i P_1 + j) P_2 + k) 2 + root, a uint64.
 *   3. Completion.  Every non-anchor receiver m in ascending order takes the participating record of seg[m] with the smallest
 *     |R - Rhat_m|, Rhat_m = |x0 - tx| + |x0 - s_m| at the root's x0, ties to the lowest position, and only when that distance is at
 *     most cspeed assoc_delay; otherwise m has no record.  K = 3 + the receivers that took one; K < min_receivers drops the candidate.
 *   4. Refinement.  n_iters Gauss-Newton steps on the K range sums, the receivers in ascending order: rows J_m = u_t + u_m (each
 *     component ((x - tx)_c / |x - tx|) + ((x - s_m)_c / |x - s_m|)), residuals rho_m = R_m - (|x - tx| + |x - s_m|), A = J^T J and
 *     g = J^T rho accumulated from 0 (each product rounded, then added), A factored as above, x + A^-1 g.  A pivot that is not positive
 *     and finite ends the refinement where x stands and sets RTS_TARGET_UNREFINED.  The final x must be finite and in the box.
 *   5. Velocity and cost at the final x (J, rho, A taken there anew).  carrier > 0: v = -lambda A^-1 J^T f with f_m the records'
 *     Dopplers, e_m = f_m + (J_m . v) / lambda; a pivot that fails here leaves v = 0 and e_m = f_m and sets RTS_TARGET_UNREFINED.
 *     Dopplers are taken as unambiguous: a stated limit.  cost = sum (rho_m rho_m) / (sigma_R sigma_R) + sum (e_m e_m) /
 *     (sigma_doppler sigma_doppler), the first sum from 0 over the receivers, then the second on top of it; dof = 2 K - 6.  carrier
 *     = 0: the second sum is absent and dof = K - 3.  The candidate is ACCEPTED when cost <= gate max(dof, 1).  power_sum: its
 *     records' power_sum added from 0 in receiver order.
 *   6. Capacity.  The accepted candidates are stored in ascending candidate index, at most max_candidates (0:
 *     RTS_LOCATE_DEFAULT_CANDIDATES, at most RTS_LOCATE_MAX_CANDIDATES); beyond that the stored prefix is resolved and
 *     rts_cube_targets_get returns RTS_ERR_CAPACITY.  Positions come from counts and a scan, never from atomics.
 *   7. Resolution.  The greedy pass over the accepted candidates in ascending (-K, cost, candidate index): a candidate becomes a
 *     TARGET when none of its records is taken, and then takes them.  The device reaches the same set by rounds of locally dominant
 *     candidates (rts_locate.hip) and ends the rounds itself.  Targets are written in ascending candidate index, at most max_targets
 *     (0: RTS_LOCATE_DEFAULT_TARGETS, at most RTS_LOCATE_MAX_TARGETS).  With exactly THREE receivers every feasible triple is a
 *     zero-cost candidate, so n targets give up to n^3 - n GHOSTS before the resolution and some survive it: inherent, not repaired
 *     -- use four receivers or more.
 *   Lifetime: the targets are NOT a product of the cube: the step copies what it needs of the records, and the targets survive
 *     rts_cube_attach, the detect calls, rts_cube_plots and rts_cube_track; they end at the next rts_cube_locate and at rts_destroy.
 *     rts_cube_targets_get synchronises, sets *n_out to the total and copies min(total, stored, capacity) records; RTS_ERR_CAPACITY
 *     when fewer were copied than the total, when max_candidates cut the candidates and when an anchor's segment was cut;
 *     RTS_ERR_INVALID before the first rts_cube_locate.  rx_positions is read during the call only (it goes through a staged upload).
 *   rts_locate_eval: pure host, the same targets of a host list of the source's record type (RtsPlot, RtsTrack or RtsTarget):
 *     up to `capacity` records to out, the total to *n_out, RTS_ERR_CAPACITY as above.  device_list and p->n_list are validated and
 *     otherwise ignored.
 *   RTS_ERR_INVALID, the message naming the field, outputs untouched: n_rx outside 3 .. RTS_LOCATE_MAX_RX; NULL rx_positions;
 *     anchors equal or >= n_rx; anchor baselines collinear, |(d_1 - d_0) x (d_2 - d_0)| <= 1e-9 |d_1 - d_0| |d_2 - d_0|; a position
 *     that is not finite; cspeed, sigma_delay, sigma_doppler, gate or assoc_delay not finite or not positive; carrier negative or not
 *     finite; a box bound that is not finite or box_lo > box_hi; min_receivers outside 3 .. n_rx; n_iters above RTS_LOCATE_MAX_ITERS;
 *     max_candidates or max_targets above their limits; an unknown source; no list for the source (no plots and no device_list;
 *     RTS_LOCATE_FROM_CANDIDATES without device_list; RTS_LOCATE_FROM_TRACKS with one); n_list without device_list or above
 *     RTS_LOCATE_MAX_LIST (candidates: RTS_LOCATE_MAX_CANDIDATES); device_list not 8-byte aligned; nonzero reserved fields.
 *     rts_locate_eval additionally refuses NULL arguments, a plot list whose rx decreases and a candidate list that is not in
 *     ascending `candidate`, names an index >= RTS_LOCATE_MAX_INDEX, has n_receivers outside 1 .. RTS_LOCATE_MAX_RX or a cost that
 *     is negative or NaN. */
#define RTS_LOCATE_MAX_RX 16u
#define RTS_LOCATE_MAX_PER_RX 1024u
#define RTS_LOCATE_MAX_ITERS 8u
#define RTS_LOCATE_DEFAULT_CANDIDATES 65536u
#define RTS_LOCATE_MAX_CANDIDATES 1048576u
#define RTS_LOCATE_DEFAULT_TARGETS 4096u
#define RTS_LOCATE_MAX_TARGETS 65536u
#define RTS_LOCATE_MAX_LIST 16777216u
#define RTS_LOCATE_MAX_INDEX 1048576u
#define RTS_LOCATE_FROM_PLOTS 0u
#define RTS_LOCATE_FROM_TRACKS 1u
#define RTS_LOCATE_FROM_CANDIDATES 2u
#define RTS_TARGET_UNREFINED 1u   /* a Gauss-Newton pivot failed: x is where the refinement stood */
typedef struct RtsLocateParams {
    double tx[3];                        /* the transmitter                                                             */
    const double* rx_positions;          /* HOST [n_rx][3], read during the call                                        */
    double cspeed, carrier;              /* carrier 0: no Doppler, velocity 0                                           */
    double sigma_delay, sigma_doppler;   /* measurement standard deviations, s and Hz, > 0                              */
    double gate;                         /* accepted when cost <= gate max(dof, 1)                                      */
    double assoc_delay;                  /* completion window, seconds, > 0                                             */
    double box_lo[3], box_hi[3];         /* the closed search volume                                                    */
    uint32_t n_rx;                       /* 3 .. RTS_LOCATE_MAX_RX                                                      */
    uint32_t anchors[3];                 /* three distinct receivers, not collinear                                     */
    uint32_t min_receivers;              /* 3 .. n_rx                                                                   */
    uint32_t n_iters;                    /* 0 .. RTS_LOCATE_MAX_ITERS Gauss-Newton steps                                */
    uint32_t max_candidates, max_targets;/* 0: the defaults                                                             */
    uint32_t source;                     /* RTS_LOCATE_FROM_*                                                           */
    uint32_t n_list;                     /* with device_list: its length; else 0                                        */
    const void* device_list;             /* NULL: the handle's plots / tracks; else caller-owned DEVICE records         */
    uint64_t reserved[2];                /* 0 */
} RtsLocateParams;                                            /* 192 bytes */
typedef struct RtsTarget {
    double pos[3], vel[3];                                    /* m, m / s                                                 */
    double cost, power_sum;
    uint64_t candidate;                                       /* the candidate index                                      */
    uint32_t n_receivers, flags;                              /* K; RTS_TARGET_*                                          */
    uint32_t plot[RTS_LOCATE_MAX_RX];                         /* per receiver the list index of its record, 0xffffffff none */
} RtsTarget;                                                  /* 144 bytes */
int rts_cube_locate(RtsHandle h, const RtsLocateParams* p);
int rts_cube_targets_get(RtsHandle h, RtsTarget* out, uint32_t capacity, uint32_t* n_out);
int rts_cube_locate_rounds(RtsHandle h, uint32_t* rounds);   /* diagnostic: rounds the last resolution took; synchronises */
int rts_locate_eval(const RtsLocateParams* p, const void* list, uint32_t n_list, RtsTarget* out, uint32_t capacity,
                    uint32_t* n_out);                                                            /* pure host */

/* ---------------------------------------------------------------- track-before-detect: dynamic programming over range-Doppler maps
 * Detect, plots and track are detect-BEFORE-track: a return reaches the tracker only when it crosses a CFAR threshold in one map.
 * rts_cube_tbd_step integrates the maps of successive intervals along every kinematically admissible cell path instead (Barniv;
 * Tonissen and Evans): a per-handle MERIT map takes each frame's score plus the best merit of a window of predecessor cells, a ring
 * of POINTER maps remembers which predecessor that was, and rts_cube_tbd_extract thresholds the accumulated merit once and reads the
 * paths back.  Both run on the device without waiting on the host.  The rules are rts_amd/csrc/rts_tbd.h, shared by the kernels
 * (rts_tbd.hip) and the host evaluators rts_tbd_step_eval and rts_tbd_extract_eval, which agree bit for bit.  All arithmetic is IEEE
 * double, every operation rounded on its own (no contraction); parentheses are evaluation order.
 *   State, per handle, of shape (n_rx, n_doppler, n_bins): the merit map, f64 [n_rx][n_doppler][n_bins]; a ring of `depth` pointer
 *     maps, uint8 in the same cell layout; per ring slot the shift table of its frame, int32 [n_doppler]; the frame count and the time
 *     of the last frame.  It survives rts_cube_attach and the detect, plot and track calls, and ends at rts_cube_tbd_reset and
 *     rts_destroy.  The shape and depth, half_doppler, half_range are fixed by the first step after a reset; a step that disagrees is
 *     RTS_ERR_INVALID and leaves the state untouched.
 *   Input of a step, as for rts_cube_detect: the handle's last rts_cube_doppler map (device_map NULL), or a caller's device pointer
 *     (16-byte aligned) with n_doppler >= 1; complex128 [n_rx][n_doppler][n_bins] with n_rx and n_bins of the attached cube.  Cell
 *     power P = re re + im im.
 *   Score: RTS_TBD_POWER x = P scale; RTS_TBD_AMPLITUDE x = sqrt(P scale).  scale > 0 and finite (the caller passes 1 / noise power).
 *     An x that is not finite counts as 0.
 *   Shift table of the frame: T = time - the previous frame's time, positive and finite from the second frame on, ignored on the
 *     first (whose table is all zeros).  w = kd wrapped into [-n_doppler / 2, n_doppler / 2) the way the CFAR section wraps it (kd -
 *     n_doppler when kd >= 0.5 n_doppler); f = w / (n_doppler pri), 0 when pri is 0;
 *       s[kd] = (int32) rint(((delay_rate_per_hz f) T) / dt)          (rint: to nearest, ties to even; dt of the attached cube)
 *     A quotient that is not finite or lies beyond +-2^30 is RTS_ERR_INVALID.  The sign convention is the tracker's: the caller
 *     passes delay_rate_per_hz = -1 / carrier.
 *   Recursion.  First frame: merit = x, every pointer RTS_TBD_NONE.  Later frames, for cell (rx, kd, r): best = 0, code = NONE; the
 *     offsets are visited in ascending (dd, dr), dd in [-Hd, Hd], dr in [-Hr, Hr]; the predecessor is cell (wrap(kd + dd),
 *     r - s[kd] + dr) of the previous merit map -- the Doppler index wraps, a range index outside [0, n_bins) is skipped -- and it
 *     replaces the best only when v > best: the FIRST maximum in that order wins, and a NaN or a merit that is not positive never
 *     does.  code = (dd + Hd)(2 Hr + 1) + (dr + Hr);  merit = x + (decay best), decay in (0, 1].  The pointer map goes into ring slot
 *     frame mod depth (frames count from 0); the merit map is replaced.
 *   Limits: Hd <= RTS_TBD_MAX_HALF_DOPPLER, Hr <= RTS_TBD_MAX_HALF_RANGE (a code is at most 216), 2 Hd + 1 <= n_doppler,
 *     Hr < n_bins, depth in 1 .. RTS_TBD_MAX_DEPTH, at most RTS_TBD_MAX_CELLS cells.
 *   Extraction: the candidates are the cells of the current merit map with merit > threshold; with RTS_TBD_LOCAL_MAX also 3 x 3 local
 *     maxima by the CFAR section's rule as it stands (strictly greater than the neighbours before the cell in flat order, >= those
 *     after; Doppler wrapped, range truncated) -- including its consequence on a ONE-ROW map, where the neighbour (-1, 0) is the cell
 *     itself and NO cell is a candidate: extract from a one-row state without RTS_TBD_LOCAL_MAX.  The list is in ascending flat order
 *     (rx, doppler_bin, range_bin), from counts and a scan, never from atomics: two runs give the same bytes.  Up to max_tracks
 *     records are stored (0: RTS_TBD_MAX_TRACKS, also the most); beyond that the total is kept and the get returns RTS_ERR_CAPACITY.
 *   Walk.  Each candidate is walked back through the ring.  At a cell (kd, r) of frame k with code c:
 *       dd = c / (2 Hr + 1) - Hd;  dr = c % (2 Hr + 1) - Hr;  the predecessor is (wrap(kd + dd), r - s_k[kd] + dr) in frame k - 1,
 *     s_k the shift table stored with frame k.  The walk stops at NONE or after min(frames, depth) cells.  (A byte that is no code of
 *     the window, or whose predecessor lies outside the range axis, ends the walk like NONE; a step never writes one.)
 *   RtsTbdTrack: the end cell (rx, doppler_bin, range_bin), n_cells visited, the OLDEST cell reached (first_doppler_bin,
 *     first_range_bin) -- paths merge going back, so cells around a target's end cell carry nearly the same merit and reach the same
 *     oldest cell: records that share it describe one target, and the caller merges them -- merit, delay = t0 + range_bin dt (t0, dt
 *     of the cube attached at the last step) and doppler = w / (n_doppler pri), 0 when pri is 0 (w of doppler_bin; pri of
 *     RtsTbdExtractParams).  Paths: uint32 [n][depth][2], entry j the (doppler_bin, range_bin) of the cell j frames back, j = 0 the
 *     end cell; entries beyond n_cells are 0xffffffff.
 *   Getters: rts_cube_tbd_tracks_get and rts_cube_tbd_paths_get synchronise and follow the capacity rule of rts_cube_tracks_get
 *     (*n_out the total; min(stored, capacity) records copied; RTS_ERR_CAPACITY when that is fewer than the total).
 *     rts_cube_tbd_merit_get copies the merit map; rts_cube_tbd_ring_get the stored pointer maps and shift tables, OLDEST FIRST,
 *     min(frames, depth) of them; rts_cube_tbd_info the state's shape (n_rx, n_doppler, n_bins, depth) and frame count (all 0 without
 *     a state).  rts_cube_tbd_reset ends the state and the extraction.
 *   Evaluators, pure host.  rts_tbd_step_eval: one step as a function -- map [n_rx][n_doppler][n_bins] (n_rx, n_bins, dt of q),
 *     merit_in (NULL: the first frame; T is then ignored) to merit_out (not merit_in), ptr_out [cells] and shifts_out [n_doppler].
 *     rts_tbd_extract_eval: merit, n_frames (1 .. depth) pointer maps [n_frames][cells] and shift tables [n_frames][n_doppler],
 *     OLDEST FIRST, to records and paths (up to `capacity` and max_tracks of them) and *n_out, the total; the walk stops after
 *     n_frames cells.
 *   RTS_ERR_INVALID, the message naming the field, outputs and state untouched: half_doppler, half_range, depth beyond their
 *     limits or changed since the first step; a window wider than the map; an unknown score; unknown flags; nonzero reserved fields;
 *     scale not positive and finite; decay outside (0, 1]; delay_rate_per_hz not finite; pri negative or not finite; time not
 *     finite; T not positive and finite; a shift quotient not finite or beyond +-2^30; a shape other than the state's; no map;
 *     threshold NaN; max_tracks above RTS_TBD_MAX_TRACKS; an extraction or a getter without a state. */
#define RTS_TBD_POWER 0u
#define RTS_TBD_AMPLITUDE 1u
#define RTS_TBD_LOCAL_MAX 1u             /* RtsTbdExtractParams.flags: only 3 x 3 local maxima of the merit map   */
#define RTS_TBD_NONE 0xffu               /* a pointer without a predecessor                                        */
#define RTS_TBD_MAX_HALF_DOPPLER 3u
#define RTS_TBD_MAX_HALF_RANGE 15u
#define RTS_TBD_MAX_DEPTH 64u
#define RTS_TBD_MAX_TRACKS 65536u
#define RTS_TBD_MAX_CELLS 0x40000000u
typedef struct RtsTbdParams {
    uint32_t half_doppler, half_range;   /* Hd, Hr: the transition window, cells on each side                      */
    uint32_t depth;                      /* pointer maps kept, 1 .. RTS_TBD_MAX_DEPTH                              */
    uint32_t score;                      /* RTS_TBD_POWER, RTS_TBD_AMPLITUDE                                       */
    uint32_t flags, reserved0;           /* 0 */
    double scale;                        /* > 0, finite: 1 / noise power                                           */
    double decay;                        /* (0, 1]: the weight of the best predecessor                             */
    double delay_rate_per_hz;            /* k: d(delay)/dt per hertz of Doppler; -1 / carrier by the library's signs */
    double pri;                          /* pulse repetition interval, >= 0; 0: no shift                           */
    uint64_t reserved[2];                /* 0 */
} RtsTbdParams;                                               /* 72 bytes */
typedef struct RtsTbdExtractParams {
    double threshold;                    /* merit > threshold is a candidate                                       */
    double pri;                          /* for RtsTbdTrack.doppler, >= 0; 0: doppler = 0                          */
    uint32_t flags;                      /* RTS_TBD_LOCAL_MAX                                                      */
    uint32_t max_tracks;                 /* records stored; 0: RTS_TBD_MAX_TRACKS                                  */
    uint64_t reserved[2];                /* 0 */
} RtsTbdExtractParams;                                        /* 40 bytes */
typedef struct RtsTbdTrack {
    uint32_t rx, doppler_bin, range_bin;                      /* the end cell, in the current merit map                   */
    uint32_t n_cells;                                         /* cells of the path, 1 .. min(frames, depth)               */
    uint32_t first_doppler_bin, first_range_bin;              /* the oldest cell reached                                  */
    double merit;
    double delay, doppler;                                    /* t0 + range_bin dt;  Hz                                   */
} RtsTbdTrack;                                                /* 48 bytes */
int rts_cube_tbd_step(RtsHandle h, const RtsTbdParams* p, double time, const void* device_map, uint32_t n_doppler);
int rts_cube_tbd_extract(RtsHandle h, const RtsTbdExtractParams* e);
int rts_cube_tbd_tracks_get(RtsHandle h, RtsTbdTrack* out, uint32_t capacity, uint32_t* n_out);
int rts_cube_tbd_paths_get(RtsHandle h, uint32_t* out, uint32_t capacity_tracks);
int rts_cube_tbd_merit_get(RtsHandle h, double* host_out, uint64_t capacity_doubles);
int rts_cube_tbd_ring_get(RtsHandle h, uint8_t* ptr_out, int32_t* shifts_out, uint32_t capacity_frames, uint32_t* n_frames_out);
int rts_cube_tbd_info(RtsHandle h, uint32_t shape_out[4], uint64_t* frames_out);
int rts_cube_tbd_reset(RtsHandle h);
int rts_tbd_step_eval(const RtsCubeParams* q, const double* map, uint32_t n_doppler, const double* merit_in, const RtsTbdParams* p,
                      double T, double* merit_out, uint8_t* ptr_out, int32_t* shifts_out);        /* pure host */
int rts_tbd_extract_eval(const RtsCubeParams* q, uint32_t n_doppler, const RtsTbdParams* p, const double* merit, const uint8_t* ptrs,
                         const int32_t* shifts, uint32_t n_frames, const RtsTbdExtractParams* e, RtsTbdTrack* out, uint32_t* paths,
                         uint32_t capacity, uint32_t* n_out);                                      /* pure host */

/* ---------------------------------------------------------------- tapered slow-time spectrogram (STFT) of the return cube
 * The short-time Fourier transform over the pulse axis, per range gate bin or summed over a gate: how Doppler changes INSIDE the
 * interval (rotor and blade flashes, tumbling bodies), where rts_cube_doppler's single rectangular DFT smears it into a band.  A
 * single frame whose window spans the interval is the TAPERED range-Doppler map: with all bins and complex output it has the layout
 * rts_cube_detect takes as device_map (n_doppler = n_fft), and with a NULL window, first_pulse 0 and window_len = n_pulses = the
 * cube's rows it equals rts_cube_doppler's output bit for bit.  Input: the attached cube y[rx][pulse][bin].  The arithmetic is
 * rts_amd/csrc/rts_stft.h, shared by the kernel (rts_stft.hip) and the host evaluator (the library builds with -ffp-contract=off:
 * the tree is the contract).
 *   Frames: only whole frames are formed, n_frames = 1 + (n_pulses - window_len) / hop (integer division); pulses left over at the
 *     end of the span are not read.  hop > window_len (gaps) and hop < window_len (overlap) are both legal.
 *   Frame input, for frame f, receiver r and gate bin g (cube bin first_bin + g; n_gate = n_bins, or the cube's n_bins - first_bin
 *     when n_bins == 0):
 *       x[i] = w[i] * y[r][first_pulse + f hop + i][first_bin + g]  for i < window_len, computed as (w re, w im);
 *       x[i] = 0                                                     for window_len <= i < n_fft;
 *     with window == NULL the samples are taken as they are, with no multiply at all.
 *   Transform: X[k] = sum_i x[i] e^{-2 pi j k i / n_fft}, by the one fixed tree of rts_cube_doppler's kernel: the samples stored at
 *     their bit-reversed index, then log2 n_fft radix-2 decimation-in-time stages; stage s = 1 .. log2 n_fft has half = 2^(s-1) and
 *     for every j < n_fft / 2, with k = j mod half, i0 = (j div half) 2^s + k, i1 = i0 + half, the butterfly
 *       (u, v) = (x[i0], x[i1]) -> (u + t, u - t),  t = tw v evaluated as (wr xr - wi xi, wr xi + wi xr),
 *       tw = tw_table[k (n_fft >> s)],  tw_table[m] = (cos, sin)(pi (-2 m / n_fft)) from one sincospi(-2.0 * m / n_fft), m < n_fft / 2.
 *   Output (row-major): complex128 [n_rx][n_frames][n_fft][n_gate];  with RTS_STFT_POWER f64 re re + im im of the same shape;  with
 *     RTS_STFT_POWER | RTS_STFT_SUM_BINS f64 [n_rx][n_frames][n_fft], the powers summed over the gate in ONE order whatever the launch
 *     shape: the gate is cut into tiles of RTS_STFT_BIN_TILE consecutive gate bins starting at gate bin 0; inside a tile the powers
 *     are added in ascending bin order, the first one the start value; then the tile sums are added in ascending tile order, the
 *     first again the start value.  No atomics: bit-identical from run to run.
 *   Axes: frame f is centred on pulse first_pulse + f hop + (window_len - 1) / 2.0.  Row k is Doppler k' / (n_fft pri), k' = k wrapped
 *     into [-n_fft / 2, n_fft / 2).  Sign as rts_cube_detect's: with the cube's phase -2 pi fc tau a CLOSING range (tau falling from
 *     pulse to pulse) gives a POSITIVE Doppler.
 * rts_cube_spectrogram is enqueued on the handle's stream and never waits for the device's earlier work (it waits only for the copy
 * of the PREVIOUS call's window out of the handle's pinned staging block); the caller's window array is free on return.  *n_frames_out
 * (may be NULL) is set on success.  device_out: caller-owned device memory of the output's size, 16-byte aligned, or NULL:
 * library-owned, alive until the next spectrogram of another size, rts_cube_attach or rts_destroy.  rts_cube_spectrogram_get
 * synchronises and copies the library-owned output (2 doubles per complex element); RTS_ERR_INVALID after an rts_cube_attach or with
 * no library-owned spectrogram, RTS_ERR_CAPACITY when capacity_doubles is too small.
 * Memory: the complex output is 16 n_rx n_frames n_fft n_gate bytes (the power form half of it); RTS_STFT_SUM_BINS writes
 * 8 n_rx n_frames n_fft bytes and, with more than one tile, keeps ceil(n_gate / 8) times that in a scratch buffer of the handle.
 * RTS_ERR_INVALID, the message naming the field: no cube attached; NULL p; nonzero reserved fields; unknown flags; RTS_STFT_SUM_BINS
 * without RTS_STFT_POWER; n_fft not a power of two in [2, RTS_STFT_MAX_FFT]; window_len 0, > n_fft or > n_pulses; hop 0; n_pulses 0
 * or first_pulse + n_pulses beyond the cube's rows; first_bin >= the cube's n_bins, or first_bin + n_bins beyond it; a non-finite
 * window value; a shape the launch grid cannot take: more than RTS_STFT_MAX_RX receivers (n_rx), or n_frames times the number of
 * workgroups per frame (ceil(n_gate / BT), BT = 8 up to n_fft 1024, 4 at 2048, 2 at 4096; ceil(n_gate / 8) with RTS_STFT_SUM_BINS)
 * above RTS_STFT_MAX_GRID_X.
 * rts_stft_eval: pure host, no device.  The same validation (q in place of the attached cube) and the same rts_stft.h functions on a
 * host cube [n_rx][q->n_pulses][q->n_bins] (interleaved re / im) -> out in the layout above.  A refused call leaves out untouched.
 * rts_window_make: pure host.  The symmetric windows w[i] = a0 - a1 cos(2 pi i / (n - 1)) + a2 cos(4 pi i / (n - 1)), i < n, with
 * (a0, a1, a2) = (1, 0, 0) RECT, (0.5, 0.5, 0) HANN, (0.54, 0.46, 0) HAMMING, (0.42, 0.5, 0.08) BLACKMAN; n == 1 gives 1.  The second
 * half mirrors the first (w[n - 1 - i] = w[i] exactly).  RTS_ERR_INVALID for n == 0, an unknown kind or a NULL out.  A window always
 * reaches the device as a host array copied by the call, so kernel and evaluator multiply by the same bits. */
#define RTS_STFT_POWER     1u   /* output re*re + im*im (real f64) instead of complex128            */
#define RTS_STFT_SUM_BINS  2u   /* needs RTS_STFT_POWER: one value per (rx, frame, k), summed over the gate */
#define RTS_STFT_MAX_FFT   4096u
#define RTS_STFT_BIN_TILE  8u   /* the summation order of RTS_STFT_SUM_BINS, see above             */
#define RTS_STFT_MAX_RX    65535u        /* the launch grid: receivers                               */
#define RTS_STFT_MAX_GRID_X 2147483647u  /* the launch grid: frames x workgroups per frame           */
typedef struct RtsStftParams {
    uint32_t first_pulse, n_pulses;   /* cube rows first_pulse .. first_pulse + n_pulses - 1                 */
    uint32_t window_len, hop;         /* pulses per frame (1 .. n_fft, <= n_pulses); pulses between frame starts (>= 1) */
    uint32_t n_fft;                   /* power of two in [2, RTS_STFT_MAX_FFT], >= window_len                */
    uint32_t first_bin, n_bins;       /* range gate; n_bins == 0: all bins from first_bin to the cube's last */
    uint32_t flags;
    const double* window;             /* [window_len] host, finite; NULL: rectangular (no multiply at all)   */
    uint64_t reserved[2];             /* 0 */
} RtsStftParams;
int rts_cube_spectrogram(RtsHandle h, const RtsStftParams* p, void* device_out, uint32_t* n_frames_out);
int rts_cube_spectrogram_get(RtsHandle h, double* host_out, uint64_t capacity_doubles);
int rts_stft_eval(const RtsCubeParams* q, const double* cube, const RtsStftParams* p, double* out, uint32_t* n_frames_out); /* pure host */
#define RTS_WINDOW_RECT 0u
#define RTS_WINDOW_HANN 1u
#define RTS_WINDOW_HAMMING 2u
#define RTS_WINDOW_BLACKMAN 3u
int rts_window_make(uint32_t kind, uint32_t n, double* out);   /* pure host */

/* ---------------------------------------------------------------- FMCW / stretch processing: dechirped beat render, fast-time range transform
 * The second class of radar: FMCW sets (automotive, altimeters, short-range surveillance) and pulsed LFM sets with stretch processing
 * never see the waveform at baseband.  They mix the echo with the running transmit chirp, sample the low-bandwidth BEAT signal and
 * take range from a fast-time FFT.  rts_cube_render_beat writes that beat signal into a row of the cube, rts_cube_range_transform
 * transforms rows along the range axis; everything downstream (noise, rts_cube_doppler, the CFARs, the spectrogram) then works
 * unchanged on the transformed cube.  The arithmetic is rts_amd/csrc/rts_beat.h (the transform's: rts_stft.h), shared by the kernels
 * (rts_beat.hip) and the host evaluators (the library builds with -ffp-contract=off: the tree is the contract).
 *
 * Beat render.  The contributions are exactly those of rts_cube_render for the chosen source: receiver rx_k, amplitude
 * a_k = sqrt(P_k) e^{j phi_k} (RTS_RENDER_RAYS: phi = -fmod(2 pi carrier tau, 2 pi); RTS_RENDER_PATHS: the group's phase), delay
 * tau_k, Doppler f_k (0 without RTS_RENDER_DOPPLER).  The call has rts_cube_render's place in the call sequence and its
 * preconditions, except that no waveform is needed.  With t_n = t0 + n dt (the cube's t0, dt; t = 0 is the start of the chirp) the
 * transmit baseband chirp is e^{j 2 pi S t^2 / 2}; the mixer forms rx conj(tx), so the cube's phase convention -2 pi fc tau and the
 * Doppler sign of rts_cube_doppler / rts_cube_detect carry over:
 *     y[rx_k][pulse][n] += a_k e^{j 2 pi psi_k(n)},   psi_k(n) = (f_k - S tau_k) t_n + S tau_k^2 / 2 - f_k tau_k     (turns)
 *         for the samples with tau_k <= t_n and 0 <= t_n < T;  nothing for a non-finite tau_k.
 * The beat frequency is f_k - S tau_k.  The caller keeps |S tau| dt < 1/2; aliasing is physics and is not refused.
 *   The tree: the row is cut into strips of RTS_BEAT_STRIP samples starting at multiples of it.  Per contribution, once:
 *       st = S tau;  fb = f - st;  ph0 = (st tau) 0.5 - f tau;  delta = fb dt;  (sd, cd) = sincospi(2 (delta - floor(delta))).
 *     Per contribution and strip whose last sample in the row has tau <= t (a later strip is skipped whole), with n0 its first sample:
 *       psi = fb t_n0 + ph0;  (s, c) = sincospi(2 (psi - floor(psi)));
 *       for i = 0 .. RTS_BEAT_STRIP - 1:  term = (are c - aim s, are s + aim c), added to the sample's sum only if sample n0 + i is in
 *       the row and passes the gate (tau <= t, t >= 0, t < T, t = t0 + (double)(n0 + i) dt);  then (c, s) <- (c cd - s sd, s cd + c sd).
 *     One sincospi per 16 samples instead of one per sample; the rotation's drift over 16 steps is a few ulp.
 *   Summation: a sample's sum starts at zero and takes the contributions in the received set's order; a sum that is not zero
 *     reaches the cube with ONE atomic add per component, so handles sharing a cube stay safe.  A large received set is cut into
 *     P <= RTS_BEAT_MAX_PARTS parts of consecutive records, each summed by workgroups of its own into a scratch buffer of the handle
 *     (16 P n_rx n_bins bytes at most); a second kernel adds the parts in ascending order, the first the start value, and does the
 *     atomic add.  P comes from a pure-host plan (rts_beat.h: rts_beat_plan) of the set's size and the cube's shape only, so a render
 *     into a zeroed row is bit-identical from run to run.  P is not part of the ABI; renders that differ in P differ in the last bits.
 *     (RTS_BEAT_PARTS = n in the environment of rts_create forces P = n as far as the set has records: the tests' switch.)
 *   The call is enqueued on the handle's stream and never waits on the host.
 *   RTS_ERR_INVALID, the message naming the field: no cube attached; NULL p; slope 0 or not finite; duration <= 0 or not finite; an
 *   unknown source or flags; nonzero reserved fields; pulse_index beyond the cube's rows; RTS_RENDER_RAYS with a cspeed that is not
 *   finite and > 0 or a carrier that is not finite and >= 0; RTS_RENDER_PATHS without rts_aggregate of the pulse; more than 65 535
 *   receivers (the launch grid).
 * rts_beat_eval: pure host, no device.  The same rts_beat.h functions on n contributions given as records (rx outside [0, n_rx) or
 * a non-finite delay: skipped), summed in order from zero and added to row pulse_index of a host cube
 * [n_rx][q->n_pulses][q->n_bins] (interleaved re / im) -- the kernel's order with P = 1.  The same validation of q and p (source is
 * checked and otherwise unused); a refused call leaves the cube untouched.
 *
 * Range transform.  Per row (rx, first_pulse + j), j < n_pulses, of the attached cube:
 *     x[i] = w[i] * y[first_bin + i]  for i < n_samples, computed as (w re, w im);   x[i] = 0  for n_samples <= i < n_fft;
 *     with window == NULL the samples are taken as they are, with no multiply at all;
 *     X = the transform of rts_stft.h as it stands (RtsStftParams above: bit-reversed load, radix-2 decimation-in-time stages,
 *     twiddles from one sincospi(-2 m / n_fft) each), X[k] = sum_i x[i] e^{-2 pi j k i / n_fft};
 *     out[rx][j][k] = X[k], or X[(n_fft - k) mod n_fft] with RTS_RANGE_REVERSE (the e^{+2 pi j k i / n_fft} transform), for k < n_out.
 *   Axis: an up-chirp (S > 0) has beat frequency -S tau and is transformed with RTS_RANGE_REVERSE, a down-chirp without it; bin k is
 *     then delay k / (|S| n_fft dt).  A caller attaches the output as a cube (rts_cube_attach with device_ptr, t0 = 0,
 *     dt = 1 / (|S| n_fft dt), n_bins = n_out) and runs rts_cube_doppler / rts_cube_detect* / rts_cube_spectrogram on it unchanged.
 *     Range-Doppler coupling: a Doppler f moves the apparent delay by -f / S.  It is inherent to the waveform and is not corrected.
 *   Output: complex128 [n_rx][n_pulses][n_out].  device_out: caller-owned device memory of that size, 16-byte aligned, or NULL:
 *     library-owned, alive until the next range transform of another size, rts_cube_attach or rts_destroy.  rts_cube_range_get
 *     synchronises and copies the library-owned output; RTS_ERR_INVALID after an rts_cube_attach or with no library-owned output,
 *     RTS_ERR_CAPACITY when capacity_doubles is too small.  The call is enqueued on the handle's stream and never waits for the
 *     device's earlier work (only for the copy of the PREVIOUS call's window out of the handle's pinned staging block); the
 *     caller's window array is free on return.
 *   RTS_ERR_INVALID, the message naming the field: no cube attached; NULL p; nonzero reserved fields; unknown flags; n_fft not a power
 *   of two in [2, RTS_RANGE_MAX_FFT]; first_bin >= the cube's n_bins or first_bin + n_samples beyond it; n_samples (after the default)
 *   > n_fft; n_out > n_fft; n_pulses 0 or first_pulse + n_pulses beyond the cube's rows; a non-finite window value; a device_out that
 *   is not 16-byte aligned; more than 2^31 - 1 workgroups (ceil(n_rx n_pulses / RT) with RT = min(16, 4096 / n_fft) rows each).
 * rts_range_eval: pure host, no device.  The same validation (q in place of the attached cube) and the same rts_stft.h functions on
 * a host cube [n_rx][q->n_pulses][q->n_bins] (interleaved re / im) -> out [n_rx][n_pulses][n_out].  A refused call leaves out untouched. */
#define RTS_BEAT_STRIP     16u     /* samples advanced by rotation from one sincospi (the summation tree, above) */
#define RTS_BEAT_MAX_PARTS 64u     /* most parts the received set is cut into (bounds the scratch)               */
typedef struct RtsBeatParams {
    double slope;            /* S, Hz/s: finite, != 0 (sign = up / down chirp)                      */
    double duration;         /* T, s: the local oscillator runs on 0 <= t < T; finite, > 0         */
    uint32_t source;         /* RTS_RENDER_RAYS / RTS_RENDER_PATHS (the contributions of rts_cube_render) */
    uint32_t flags;          /* 0 or RTS_RENDER_DOPPLER                                             */
    uint64_t reserved[2];    /* 0 */
} RtsBeatParams;
int rts_cube_render_beat(RtsHandle h, uint32_t pulse_index, const RtsBeatParams* p, double cspeed, double carrier);

typedef struct RtsBeatContribution { int32_t rx, reserved; double re, im, delay, doppler; } RtsBeatContribution;
/* pure host: adds the contributions into row pulse_index of a host cube [n_rx][q->n_pulses][q->n_bins] */
int rts_beat_eval(const RtsCubeParams* q, const RtsBeatParams* p, const RtsBeatContribution* c, uint32_t n,
                  uint32_t pulse_index, double* cube);

#define RTS_RANGE_REVERSE  1u      /* out[k] = X[(n_fft - k) mod n_fft]: the e^{+2 pi j k n / N} transform */
#define RTS_RANGE_MAX_FFT  4096u
typedef struct RtsRangeParams {
    uint32_t first_pulse, n_pulses;   /* cube rows first_pulse .. first_pulse + n_pulses - 1          */
    uint32_t first_bin, n_samples;    /* fast-time samples first_bin .. first_bin + n_samples - 1; n_samples 0: to the row's end */
    uint32_t n_fft;                   /* power of two in [2, RTS_RANGE_MAX_FFT], >= n_samples         */
    uint32_t n_out;                   /* bins kept, 1 .. n_fft; 0: n_fft                              */
    uint32_t flags, reserved0;
    const double* window;             /* [n_samples] host, finite; NULL: no multiply at all          */
    uint64_t reserved[2];
} RtsRangeParams;
int rts_cube_range_transform(RtsHandle h, const RtsRangeParams* p, void* device_out);  /* complex128 [n_rx][n_pulses][n_out] */
int rts_cube_range_get(RtsHandle h, double* host_out, uint64_t capacity_doubles);
int rts_range_eval(const RtsCubeParams* q, const double* cube, const RtsRangeParams* p, double* out);  /* pure host */

/* ---------------------------------------------------------------- receive-array beamforming across the cube's receivers
 * The third axis of the cube.  Every other product treats the receiver index as a loop index; this one combines the receivers of a
 * coherent cube into beams: the angle of a detection, and the array gain that makes a weak target detectable at all.  The arithmetic
 * is rts_amd/csrc/rts_beam.h, shared by the kernel (rts_beam.hip) and the host evaluator (the library builds with
 * -ffp-contract=off: the tree is the contract).  It holds no transcendental, so device and evaluator agree BIT FOR BIT.
 *   Input z[rx][row][bin], complex128; n_rx and n_bins are the attached cube's (a cube must be attached for every source):
 *     RTS_BEAM_FROM_CUBE     the attached cube, n_pulses rows;
 *     RTS_BEAM_FROM_MAP      the handle's last library-owned rts_cube_doppler map, n_fft rows;
 *     RTS_BEAM_FROM_POINTER  device_in, caller-owned device memory [n_rx][n_rows_in][n_bins], 16-byte aligned.
 *   Rows first_row .. first_row + n_rows - 1 of every receiver are read (n_rows 0: from first_row to the source's last row).
 *   Weights w[beam][rx], complex128 (interleaved re / im), on the host; the call copies them, kernel and evaluator multiply by the
 *   same bits.
 *     term(b, rx)    = conj(w[b][rx]) z[rx][row][bin] = (wr zr + wi zi, wr zi - wi zr)     four multiplies, one add, one subtract
 *     y[b][row][bin] = the sum of term(b, rx) over ascending rx; the rx = 0 term is the start value.
 *   Output, row-major:
 *     default          complex128 [n_beams][n_rows][n_bins]: the layout of a cube with n_rx = n_beams, which another handle attaches
 *                      (rts_cube_attach with device_ptr) to run rts_cube_doppler / rts_cube_detect* / rts_cube_spectrogram on beams;
 *     RTS_BEAM_POWER   f64 re re + im im, the same shape;
 *     RTS_BEAM_PEAK    f64 [n_rows][n_bins][2] = (P*, coordinate) and no per-beam output (it excludes RTS_BEAM_POWER): P* the
 *                      largest beam power of the cell, b* the LOWEST beam index that attains it,
 *                      coordinate = (double)b* + the log-parabola offset of the detection records (RtsDetection's range_offset rule)
 *                      through P[b* - 1], P[b*], P[b* + 1]; the offset is 0 when b* is the first or the last beam (the beam axis
 *                      does not wrap).  With a NaN among a cell's powers the reported beam is unspecified; nothing is read out of
 *                      bounds.
 *   No atomics: every output element is one plain store, bit-identical from run to run.
 *   device_out: caller-owned device memory of the output's size, 16-byte aligned, or NULL: library-owned, alive until the next
 *     beamform of another size, rts_cube_attach or rts_destroy.  rts_cube_beam_get synchronises and copies the library-owned
 *     output; RTS_ERR_INVALID after an rts_cube_attach or with no library-owned output, RTS_ERR_CAPACITY when capacity_doubles is
 *     too small.  The call is enqueued on the handle's stream and never waits for the device's earlier work (only for the copy of
 *     the PREVIOUS call's weights out of the handle's pinned staging block); the caller's weight array is free on return.
 *   RTS_ERR_INVALID, the message naming the field: no cube attached; NULL p or NULL weights; nonzero reserved fields; an unknown
 *   source or flags; RTS_BEAM_PEAK together with RTS_BEAM_POWER; n_beams 0 or above RTS_BEAM_MAX_BEAMS; n_rx above RTS_BEAM_MAX_RX;
 *   n_beams * n_rx above RTS_BEAM_MAX_WEIGHTS (64 KiB of complex128: the whole table sits in a workgroup's LDS); a non-finite
 *   weight; RTS_BEAM_FROM_MAP without a library-owned map; RTS_BEAM_FROM_POINTER with a NULL or misaligned device_in or with
 *   n_rows_in 0; n_rows_in or device_in set with another source; first_row or first_row + n_rows beyond the source's rows; a
 *   misaligned device_out; a caller-owned device_out whose bytes overlap the bytes of the input the call reads (the transform is not
 *   in place); a shape the launch grid cannot take (more than 2^31 - 1 workgroups of 256 cells).  A refused call leaves the
 *   handle's previous output and weights as they were.
 * rts_beamform_eval: pure host, no device.  The same rts_beam.h functions on a host array `in` [n_rx][n_rows_in][n_bins] (interleaved
 *   re / im), which stands for the source p names; q in place of the attached cube (n_rx, n_bins).  The same validation as far as it
 *   concerns no device memory: with RTS_BEAM_FROM_POINTER p->n_rows_in must equal the n_rows_in argument and p->device_in is not
 *   looked at.  NULL q, in or out, n_rx, n_bins or n_rows_in 0 are refused too.  A refused call leaves out untouched.
 * rts_steering_make: pure host.  Far-field steering weights in the cube's phase convention.  Direction b is (az, el) in radians,
 *   directions[2 b], directions[2 b + 1]; positions[3 rx ..] the element centres in metres:
 *     u = (cos el cos az, cos el sin az, sin el);  x = ((ux px + uy py) + uz pz) / wavelength;  f = x - floor(x);
 *     w[b][rx] = taper[rx] (cos 2 pi f + j sin 2 pi f), the cosine and sine by exact reflection into the first octants, then libm
 *     (the host side of the transforms' twiddles); a NULL taper means 1 and no multiply at all.
 *   The sign: the cube's phase is -2 pi fc tau; a plane wave from direction u reaches the element at p earlier by (u . p) / c, so its
 *   phase there is +2 pi (u . p) / lambda ahead, and y = sum conj(w) z peaks in the beam steered at u.
 *   RTS_ERR_INVALID for a NULL pointer (taper apart), n_rx or n_beams 0, a wavelength not finite and > 0, a non-finite position,
 *   direction or taper.
 * NOTE on geometry: the tracer ends a ray's length on the receiver's capture SPHERE, not at its centre.  Receivers of equal radius in
 *   the far field whose spheres are DISJOINT share that offset, so their relative phases are those of their centres.  Unequal radii
 *   or near-field geometry are the caller's to model; the beamformer itself is plain linear algebra on whatever cube it is given.
 * NOTE on dense arrays: a ray is delivered to ONE receiver only.  Where capture spheres overlap, the last capturing receiver of the
 *   list takes the ray and the ray's length accumulates the earlier spheres' entry distances (the reference's behaviour, quirk 4:
 *   tests/test_capture_branches.py).  So array elements closer than two radii cannot share a launch: of eight elements half a
 *   wavelength apart in one rts_set_receivers call the first seven receive nothing and the eighth every ray, with lengths that are
 *   not its own.  The recipe for a dense array is one launch per element -- rts_set_receivers with that element alone, then
 *   rts_cube_attach of a one-receiver cube at the element's slab (n_pulses * n_bins samples) of a shared [n_rx][n_pulses][n_bins]
 *   device buffer, then the pulses -- and a handle that attaches the whole buffer with n_rx elements for the array families.
 *   tests/test_array_chain_host.py shows both on the oracle, tests/test_gpu_array_chain.py the recipe on the device: the beams,
 *   the MVDR null, the angular spectra and the space-time filters of such a cube point where the sign rule above says. */
#define RTS_BEAM_FROM_CUBE    0u   /* rows of the attached cube                                                     */
#define RTS_BEAM_FROM_MAP     1u   /* the handle's last library-owned rts_cube_doppler map; rows = its n_fft       */
#define RTS_BEAM_FROM_POINTER 2u   /* device_in: complex128 [n_rx][n_rows_in][n_bins], 16-byte aligned              */
#define RTS_BEAM_POWER        1u   /* f64 re re + im im per beam                                                    */
#define RTS_BEAM_PEAK         2u   /* f64 (P*, coordinate) per cell, no per-beam output; excludes RTS_BEAM_POWER    */
#define RTS_BEAM_MAX_RX       64u
#define RTS_BEAM_MAX_BEAMS    1024u
#define RTS_BEAM_MAX_WEIGHTS  4096u  /* bounds n_beams * n_rx: 64 KiB of complex128                                 */
typedef struct RtsBeamParams {
    uint32_t n_beams, source;
    uint32_t first_row, n_rows;      /* n_rows 0: from first_row to the last row of the source                      */
    uint32_t n_rows_in, flags;       /* n_rows_in: POINTER only (0 otherwise); flags: RTS_BEAM_POWER | RTS_BEAM_PEAK */
    const double* weights;           /* host [n_beams][n_rx], interleaved re / im, finite                           */
    const void* device_in;           /* POINTER only                                                                */
    uint64_t reserved[2];            /* 0 */
} RtsBeamParams;
int rts_cube_beamform(RtsHandle h, const RtsBeamParams* p, void* device_out);
int rts_cube_beam_get(RtsHandle h, double* host_out, uint64_t capacity_doubles);
int rts_beamform_eval(const RtsCubeParams* q, const double* in, uint32_t n_rows_in, const RtsBeamParams* p, double* out); /* pure host */
int rts_steering_make(const double* positions, uint32_t n_rx, const double* directions, uint32_t n_beams,
                      double wavelength, const double* taper, double* weights_out);                                      /* pure host */

/* ---------------------------------------------------------------- adaptive (MVDR) beamforming: sample covariance and weight solve
 * Weights computed FROM THE DATA for rts_cube_beamform: the sample covariance R of the receivers over a set of training cells, and
 * the sample-matrix-inversion MVDR weights w = R^-1 s / (s^H R^-1 s) of steering rows s (rts_steering_make's layout).  Against a
 * strong directional interferer a conventional beam is limited by its sidelobes; these weights place a null on it.  The arithmetic
 * is rts_amd/csrc/rts_adapt.h, shared by the kernels (rts_adapt.hip) and the host evaluators (the library builds with
 * -ffp-contract=off: the trees are the contract).  They hold + - * / and sqrt only, so device and evaluators agree BIT FOR BIT.
 *
 * rts_cube_covariance.  Input z[rx][row][bin], complex128, from the beamformer's three sources under the beamformer's rules
 *   (RTS_BEAM_FROM_CUBE, _MAP, _POINTER; n_rows_in and device_in with _POINTER only; n_rx and n_bins are the attached cube's).
 *   Training cells: rows first_row .. first_row + n_rows - 1 (n_rows 0: to the source's last row), bins first_bin .. first_bin +
 *   n_bins - 1 (n_bins 0: to the last bin) WITHOUT the bins skip_first_bin .. skip_first_bin + skip_n_bins - 1 (the cells under test
 *   and their guard, so that a target does not null itself; skip_n_bins 0: none, and skip_first_bin must be 0 then).  The skipped
 *   interval lies inside the bin span and leaves at least one bin.  The cells are numbered row-major over the included bins,
 *   c = 0 .. K - 1.
 *     term(i, j, c) = z_i conj(z_j) = (ar br + ai bi, ai br - ar bi), a = z_i, b = z_j: four multiplies, one add, one subtract; j <= i.
 *     The cells are cut into tiles = ceil(K / RTS_ADAPT_TILE) tiles of consecutive cells and parts = min(RTS_ADAPT_MAX_PARTS, tiles)
 *     parts; part p owns the tiles floor(p tiles / parts) .. floor((p + 1) tiles / parts) - 1.  A part's sum runs over its cells in
 *     ascending c, the first term the start value; the parts are summed in ascending p, part 0 the start value; each component is
 *     then divided once by (double)K.  R[j][i] (j < i) is the exact conjugate (re, -im) of R[i][j]; the imaginary part of the
 *     diagonal is stored as +0.0.  The partition is a function of the shape alone, never of the device.
 *   Output complex128 [n_rx][n_rx], row-major, interleaved re / im.  No atomics: identical bits from run to run.
 * rts_cube_mvdr.  cov: device_cov (caller-owned device memory [n_rx][n_rx] complex128, 16-byte aligned, n_rx the record's) or, with
 *   device_cov NULL, the handle's last library-owned covariance (the record's n_rx is then 0 or that covariance's).  Only the lower
 *   triangle is read, and of the diagonal only the real part.  steering: host, complex128 [n_beams][n_rx], finite; copied by the call.
 *     1. A = R + loading I: one add per diagonal real part; loading >= 0 in the cube's power units (e.g. rts_cube_add_noise's
 *        noise_power).
 *     2. Column Cholesky A = L L^H, columns j ascending:
 *          d = A_jj, then d = d - (L_jk.re L_jk.re + L_jk.im L_jk.im) for k = 0 .. j - 1 ascending;  L_jj = sqrt(d);
 *          for i > j: x = A_ij, then x = x - L_ik conj(L_jk) (term's tree: a = L_ik, b = L_jk; re and im each one subtraction) for
 *          k = 0 .. j - 1 ascending;  L_ij = (x.re / L_jj, x.im / L_jj).
 *     3. Per beam b, s = steering[b]:
 *          forward, rows i ascending:  x = s_i, then x = x - L_ik u_k = x - (lr ur - li ui, lr ui + li ur) for k = 0 .. i - 1 ascending;
 *                                      u_i = (x.re / L_ii, x.im / L_ii);
 *          den = the sum of (u_k.re u_k.re + u_k.im u_k.im) over ascending k, the k = 0 term the start value;
 *          back, rows i descending:    x = u_i, then x = x - conj(L_ki) v_k = x - (lr vr + li vi, lr vi - li vr) for k = i + 1 .. n_rx - 1
 *                                      ascending;  v_i = (x.re / L_ii, x.im / L_ii);
 *          w[b][i] = (v_i.re / den, v_i.im / den).
 *     With the beamformer's y = sum conj(w) z the beam is distortionless: w^H s = 1.
 *     A pivot d that is not finite or not > 0 fails the solve at column j: EVERY weight of the output is NaN and a status word of the
 *     handle on the device records j; rts_cube_mvdr_get then returns RTS_ERR_INVALID naming the pivot (the handle stays usable).
 *   Output complex128 [n_beams][n_rx]: a weight table of rts_cube_beamform (n_rx <= RTS_BEAM_MAX_RX, n_beams <= RTS_BEAM_MAX_BEAMS,
 *   n_beams * n_rx <= RTS_BEAM_MAX_WEIGHTS), which the caller moves with rts_cube_mvdr_get -> RtsBeamParams.weights.
 * device_out of either call: caller-owned device memory of the output's size, 16-byte aligned, or NULL: library-owned, alive until
 *   the next call of another size, rts_cube_attach or rts_destroy; rts_cube_covariance_get / rts_cube_mvdr_get synchronise and copy
 *   the library-owned output (RTS_ERR_INVALID after an rts_cube_attach or with none, RTS_ERR_CAPACITY when capacity_doubles is too
 *   small).  A caller-owned output is not recorded.  The calls are enqueued on the handle's stream and never wait for the device's
 *   earlier work (rts_cube_mvdr: only for the copy of the PREVIOUS call's steering out of the handle's pinned staging block).
 * RTS_ERR_INVALID, the message naming the field: no cube attached; NULL p; nonzero reserved fields; an unknown source;
 *   RTS_BEAM_FROM_MAP without a library-owned map; RTS_BEAM_FROM_POINTER with a NULL or misaligned device_in or n_rows_in 0; n_rows_in
 *   or device_in with another source; rows or bins outside the source; a skipped interval outside the bin span, leaving no bin, or
 *   skip_first_bin set with skip_n_bins 0; n_rx above RTS_BEAM_MAX_RX; more than 2^32 - 1 tiles; a misaligned device_out; a
 *   device_out that overlaps the bytes the call reads; n_beams 0 or beyond the limits above; NULL or non-finite steering; a loading
 *   that is negative or not finite; neither device_cov nor a library-owned covariance; a misaligned device_cov; an n_rx that is 0
 *   with device_cov or differs from the library-owned covariance's.  A refused call leaves the handle's previous products as they
 *   were.
 * rts_covariance_eval / rts_mvdr_eval: pure host, no device: the same rts_adapt.h functions.  `in` [n_rx][n_rows_in][n_bins] stands for
 *   the source p names, q for the attached cube (n_rx, n_bins); as rts_beamform_eval, with RTS_BEAM_FROM_POINTER p->n_rows_in must
 *   equal the argument and device_in is not looked at.  rts_mvdr_eval reads cov [n_rx][n_rx] as the kernel does (device_cov is not
 *   looked at, p->n_rx must equal the argument); a failed solve returns RTS_ERR_INVALID naming the pivot.  A refused or failed call
 *   leaves out untouched. */
#define RTS_ADAPT_TILE       64u    /* training cells per tile of the covariance's tree                                 */
#define RTS_ADAPT_MAX_PARTS  512u   /* parts of the covariance's tree: the scratch is parts * n_rx^2 * 16 bytes (<= 32 MiB) */
typedef struct RtsCovParams {
    uint32_t source, n_rows_in;      /* RTS_BEAM_FROM_*; n_rows_in: POINTER only (0 otherwise)                       */
    uint32_t first_row, n_rows;      /* n_rows 0: from first_row to the last row of the source                      */
    uint32_t first_bin, n_bins;      /* n_bins 0: from first_bin to the last bin                                    */
    uint32_t skip_first_bin, skip_n_bins;  /* bins left out of the training set; skip_n_bins 0: none                */
    const void* device_in;           /* POINTER only                                                                */
    uint64_t reserved[2];            /* 0 */
} RtsCovParams;
typedef struct RtsMvdrParams {
    uint32_t n_beams, n_rx;          /* n_rx: with device_cov and in the evaluator; 0 or the covariance's otherwise  */
    double loading;                  /* >= 0, finite: added to the diagonal                                         */
    const double* steering;          /* host [n_beams][n_rx], interleaved re / im, finite                           */
    const void* device_cov;          /* complex128 [n_rx][n_rx], 16-byte aligned; NULL: the last library-owned covariance */
    uint64_t reserved[2];            /* 0 */
} RtsMvdrParams;
int rts_cube_covariance(RtsHandle h, const RtsCovParams* p, void* device_out);         /* complex128 [n_rx][n_rx] */
int rts_cube_covariance_get(RtsHandle h, double* host_out, uint64_t capacity_doubles);
int rts_covariance_eval(const RtsCubeParams* q, const double* in, uint32_t n_rows_in, const RtsCovParams* p, double* out);  /* pure host */
int rts_cube_mvdr(RtsHandle h, const RtsMvdrParams* p, void* device_out);              /* complex128 [n_beams][n_rx] */
int rts_cube_mvdr_get(RtsHandle h, double* host_out, uint64_t capacity_doubles);
int rts_mvdr_eval(const double* cov, uint32_t n_rx, const RtsMvdrParams* p, double* out);                                     /* pure host */

/* ---------------------------------------------------------------- space-time adaptive processing (STAP): stacked covariance, tap filter
 * The adaptive blocks above see ONE axis: the receivers of one cell.  On a moving platform the ground clutter is a ridge in the
 * angle-Doppler plane; a spatial null or a Doppler filter alone removes the target with it or leaves its sidelobes.  STAP applies the
 * same sample-matrix inversion to snapshots stacked over the receivers AND over n_taps consecutive rows (pulses).  The arithmetic is
 * rts_amd/csrc/rts_stap.h, shared by the kernels (rts_adapt.hip: the covariance; rts_stap.hip: the filter) and the host evaluators.
 * The trees hold + - * / only: device and evaluators agree BIT FOR BIT (the library builds with -ffp-contract=off).
 *   Input z[rx][row][bin], complex128, from the beamformer's three sources under the beamformer's rules.  N = the cube's n_rx,
 *   M = n_taps (1 .. RTS_ST_MAX_TAPS), D = M N <= RTS_BEAM_MAX_RX.  The snapshot at (row p, bin b) is
 *     x[d] = z[d % N][p + d / N][b],  d = m N + rx      tap-major: a steering vector is temporal (x) spatial.
 *   A span of n_rows rows (n_rows 0: from first_row to the source's last row) holds n_rows - M + 1 snapshot rows; n_rows < M is refused.
 * rts_cube_st_covariance.  Output complex128 [D][D].  Training snapshots: the start rows first_row .. first_row + n_rows - M, of each
 *   the bins rts_cube_covariance selects (span and skipped interval), numbered row-major c = 0 .. K - 1, K = (n_rows - M + 1) kept.
 *   The tree is rts_cube_covariance's with x in place of z: term(i, j <= i, c) = x_i conj(x_j), tiles of RTS_ADAPT_TILE cells,
 *   min(RTS_ADAPT_MAX_PARTS, tiles) parts, ascending sums, one division by (double)K, the exact conjugate in the upper triangle, +0.0
 *   on the diagonal's imaginary part, no atomics.  With n_taps = 1 the output is rts_cube_covariance's, bit for bit.
 *   A library-owned result (device_out NULL) becomes THE HANDLE'S LAST LIBRARY-OWNED COVARIANCE, of order D: rts_cube_mvdr with
 *   device_cov NULL solves it (steering rows of D entries, the record's n_rx 0 or D) and rts_cube_covariance_get copies it (2 D D
 *   doubles), through the code paths they have for rts_cube_covariance's.
 * rts_cube_st_apply.  Weights w[f][d], complex128 on the host [n_filters][D], copied by the call (n_filters <= RTS_BEAM_MAX_BEAMS,
 *   n_filters D <= RTS_BEAM_MAX_WEIGHTS).
 *     y[f][p][b] = the sum of conj(w[f][d]) x[d] (rts_cube_beamform's term) over ascending d; the d = 0 term is the start value.
 *   Output complex128 [n_filters][n_rows - M + 1][n_bins]: the layout of a cube with n_rx = n_filters and n_rows - M + 1 pulses, which
 *   another handle attaches (rts_cube_attach with device_ptr) for rts_cube_doppler / rts_cube_detect*; with the flag RTS_BEAM_POWER
 *   f64 re re + im im of the same shape.  No PEAK form.  Plain stores only: identical bits from run to run.  With n_taps = 1 the
 *   output is rts_cube_beamform's, bit for bit.  rts_cube_st_get copies a library-owned output, under rts_cube_beam_get's rules.
 * device_out, the stream and the staging of the weights: as rts_cube_covariance / rts_cube_beamform.
 * rts_st_steering_make: pure host.  spatial [n_beams][n_rx] (rts_steering_make's rows), doppler [n_doppler] in cycles per pulse,
 *   tap_taper [n_taps] real or NULL (1, and no multiply at all):
 *     x = f (double)m;  fr = x - floor(x);  t_m = tap_taper[m] (cos 2 pi fr + j sin 2 pi fr), cosine and sine as in rts_steering_make;
 *     out[beam n_doppler + k][m n_rx + rx] = t_m spatial[beam][rx] = (tr ar - ti ai, tr ai + ti ar).
 *   The sign: rts_cube_doppler is sum_p cube[p] e^(-2 pi j k p / n_fft); a scatterer at f cycles per pulse advances by e^(+2 pi j f)
 *   per pulse, and y = sum conj(w) x peaks in the filter steered at f.
 * rts_st_covariance_eval / rts_st_apply_eval: pure host, no device: the same rts_stap.h functions on `in` [n_rx][n_rows_in][n_bins],
 *   under rts_covariance_eval's / rts_beamform_eval's rules.  A refused call leaves out untouched.
 * RTS_ERR_INVALID, the message naming the field: everything rts_cube_covariance / rts_cube_beamform refuse for the fields they share
 *   (n_filters in n_beams' place), and: n_taps 0 or above RTS_ST_MAX_TAPS; n_taps * n_rx above RTS_BEAM_MAX_RX; n_rows (after the
 *   default) below n_taps; flags other than RTS_BEAM_POWER; nonzero reserved fields; a caller-owned output that overlaps the input the
 *   call reads; a shape the launch grid cannot take.  A refused call leaves the handle's previous products as they were. */
#define RTS_ST_MAX_TAPS      16u
typedef struct RtsStCovParams {
    uint32_t source, n_rows_in;      /* as RtsCovParams                                                              */
    uint32_t first_row, n_rows;      /* the span of rows the snapshots lie in; n_rows 0: to the source's last row    */
    uint32_t first_bin, n_bins;
    uint32_t skip_first_bin, skip_n_bins;
    uint32_t n_taps, reserved0;      /* 1 .. RTS_ST_MAX_TAPS; 0                                                      */
    const void* device_in;           /* POINTER only                                                                */
    uint64_t reserved[2];            /* 0 */
} RtsStCovParams;
typedef struct RtsStApplyParams {
    uint32_t n_filters, source;
    uint32_t first_row, n_rows;      /* n_rows 0: from first_row to the last row of the source                      */
    uint32_t n_rows_in, flags;       /* n_rows_in: POINTER only (0 otherwise); flags: RTS_BEAM_POWER                 */
    uint32_t n_taps, reserved0;      /* 1 .. RTS_ST_MAX_TAPS; 0                                                      */
    const double* weights;           /* host [n_filters][n_taps n_rx], interleaved re / im, finite                  */
    const void* device_in;           /* POINTER only                                                                */
    uint64_t reserved[2];            /* 0 */
} RtsStApplyParams;
int rts_cube_st_covariance(RtsHandle h, const RtsStCovParams* p, void* device_out);    /* complex128 [D][D], D = n_taps n_rx */
int rts_st_covariance_eval(const RtsCubeParams* q, const double* in, uint32_t n_rows_in, const RtsStCovParams* p, double* out);  /* pure host */
int rts_cube_st_apply(RtsHandle h, const RtsStApplyParams* p, void* device_out);       /* complex128 [n_filters][n_rows - n_taps + 1][n_bins] */
int rts_cube_st_get(RtsHandle h, double* host_out, uint64_t capacity_doubles);
int rts_st_apply_eval(const RtsCubeParams* q, const double* in, uint32_t n_rows_in, const RtsStApplyParams* p, double* out);     /* pure host */
int rts_st_steering_make(const double* spatial, uint32_t n_rx, uint32_t n_beams, const double* doppler, uint32_t n_doppler,
                         uint32_t n_taps, const double* tap_taper, double* out);                                                  /* pure host */

/* ---------------------------------------------------------------- direction finding: Hermitian eigensolver, angular spectrum scan
 * The beamformers above answer "what arrives from the directions I steer at"; the eigendecomposition of the covariance answers "how
 * many sources are there and where": MUSIC, Capon's and Bartlett's spectra, the source count (AIC / MDL), and whatever else stands
 * on eigenpairs (eigencanceler weights, principal components).  The arithmetic is rts_amd/csrc/rts_doa.h, shared by the kernels
 * (rts_doa.hip) and the host evaluators; + - * /, sqrt and comparisons only (the library builds with -ffp-contract=off): device and
 * evaluators agree BIT FOR BIT.  No atomics, plain stores only.
 *
 * rts_cube_eig.  cov: device_cov (caller-owned device memory [n][n] complex128, 16-byte aligned, n the record's) or, with device_cov
 *   NULL, the handle's last library-owned covariance -- rts_cube_covariance's of order n_rx or rts_cube_st_covariance's of order D
 *   (the record's n is then 0 or that order).  n <= RTS_BEAM_MAX_RX.  Only the lower triangle is read, and of the diagonal only the
 *   real part.  One-sided (Hestenes) Jacobi on X = A, V = I, both [n][n]:
 *     X[i][j] = A[i][j] (i > j), X[i][i] = (re A[i][i], +0.0), X[j][i] = (re, -im) of A[i][j].
 *     A sweep: m2 = the largest of norm2(col) = sum over ascending i of (re re + im im) of X[i][col] (the i = 0 term the start value),
 *     by `if (v > m2) m2 = v` over ascending col from norm2(0); floor2 = 2^-104 m2.  Then the rounds r = 0 .. M - 2 (M = n rounded up to
 *     even) of M / 2 disjoint column pairs: slot 0 pairs M - 1 with r, slot k > 0 pairs (r + k) % (M - 1) with
 *     (r + M - 1 - k) % (M - 1); p the smaller, q the larger; q >= n is the bye of an odd n.  A function of n alone.  Per pair:
 *       alpha = norm2(p);  beta = norm2(q);  gamma = sum over ascending i of conj(x_ip) x_iq = (pr qr + pi qi, pr qi - pi qr), the
 *       i = 0 term the start value;  g2 = gr gr + gi gi.
 *       No rotation when g2 <= 2^-100 (alpha beta), or alpha <= floor2, or beta <= floor2 (a column of a null space holds only
 *       rounding noise: it would pass the relative test for ever).  Otherwise
 *       g = sqrt(g2);  e = (gr / g, gi / g);  zeta = (beta - alpha) / (2.0 g);  d = |zeta| + sqrt(1.0 + zeta zeta);
 *       t = 1.0 / d, or -1.0 / d when zeta < 0;  c = 1.0 / sqrt(1.0 + t t);  s = c t;  sr = s e.re;  si = s e.im;  and every row i of X,
 *       then of V, with a = [i][p], b = [i][q]:
 *         a' = (c ar - (sr br + si bi), c ai - (sr bi - si br));   b' = ((sr ar - si ai) + c br, (sr ai + si ar) + c bi).
 *     The solver runs sweeps until one rotates nothing (status 0); after RTS_EIG_MAX_SWEEPS sweeps that each rotated it gives up
 *     (status 1).  An entry of the lower triangle outside [-DBL_MAX, DBL_MAX] (NaN included), checked before anything: status 2.
 *     lambda(col) = sum over ascending i of (vr xr + vi xi), v = V[i][col], x = X[i][col], the i = 0 term the start value.
 *     Order: descending lambda, ties by ascending column (rank(col) = the count of j with lambda(j) > lambda(col), or equal and
 *     j < col): fixed, never an unstable sort.  No phase normalisation.
 *   Output: device_values f64 [n] and device_vectors complex128 [n][n], ROW k = eigenvector k: a weight row of rts_cube_beamform.
 *     Both caller-owned (8- and 16-byte aligned) or both NULL: library-owned, THE HANDLE'S LAST LIBRARY-OWNED EIGENPAIRS.  With a
 *     status other than 0 EVERY output is NaN and a status word of the handle on the device records it; rts_cube_eig_get then returns
 *     RTS_ERR_INVALID naming the cause (the handle stays usable).  rts_cube_eig_get copies whichever of values_out (n doubles) and
 *     vectors_out (2 n n doubles) is not NULL.
 *   A is meant positive semidefinite (a covariance): V diagonalises A^2, so eigenvalues of equal magnitude and opposite sign would
 *   share a subspace.
 * rts_cube_doa_scan.  The angular spectrum of n_dirs directions through m vectors v_k [n] and weights g_k:
 *     y_k = sum over ascending rx of conj(v_k[rx]) a[rx] (rts_cube_beamform's term and sum: rx = 0 the start value);
 *     p_k = y.re y.re + y.im y.im;  q = g_0 p_0, then q = q + g_k p_k for ascending k;  out = q, or with RTS_DOA_INVERSE 1.0 / q: the
 *     IEEE quotient with no clamp, so q = 0 gives +inf.
 *   device_steering: caller-owned device memory, complex128 ELEMENT-MAJOR [n][n_dirs] (the cube's layout with the directions in the
 *   bins' place; rts_steering_make's rows transposed), 16-byte aligned.  The vectors are rows first_vector .. first_vector + m - 1 of
 *   device_vectors (complex128 [n][n], 16-byte aligned, n the record's) or, with device_vectors NULL, of the handle's last
 *   library-owned eigenvectors (n 0 or their order): MUSIC's noise subspace is a row range of the sorted table, nothing is copied.
 *   g: host [m], finite, copied by the call.  Output f64 [n_dirs], 8-byte aligned or NULL: library-owned, for rts_cube_doa_get.
 *   With m = 1 and g = 1 the output is rts_cube_beamform's RTS_BEAM_POWER of the table as a one-row cube, bit for bit.
 * rts_doa_weights: pure host.  (first, m, g[m], flags) of the scan for a spectrum, from the eigenvalues in the solver's order:
 *     RTS_DOA_BARTLETT  first 0, m n, g_k = lambda_k,                 flags 0                  a^H R a
 *     RTS_DOA_CAPON     first 0, m n, g_k = 1.0 / (lambda_k + loading), RTS_DOA_INVERSE        1 / (a^H (R + loading I)^-1 a)
 *     RTS_DOA_MUSIC     first n_sources, m n - n_sources, g_k = 1.0,  RTS_DOA_INVERSE          1 / |noise subspace^H a|^2
 *   g has room for n values.  Refused: NULL pointers; n 0 or above RTS_BEAM_MAX_RX; an unknown method; a loading that is negative or
 *   not finite; a non-finite eigenvalue; MUSIC with n_sources >= n; Capon with a lambda_k + loading not > 0.  n_sources is looked
 *   at by MUSIC only, loading is used by Capon only.
 * rts_source_count: pure host, libm's log, no device twin and no bit contract.  Eigenvalues in descending order, K snapshots; with
 *   the n - k smallest eigenvalues L(k) = K (n - k) (log(their arithmetic mean) - the mean of their logs),
 *     RTS_DOA_AIC: 2 L(k) + 2 k (2 n - k);  RTS_DOA_MDL: L(k) + 0.5 k (2 n - k) log K;  the first k in 0 .. n - 1 of the smallest value.
 *   Refused: NULL pointers; n 0 or above RTS_BEAM_MAX_RX; K 0; an unknown criterion; an eigenvalue that is not finite, not > 0
 *   (every one enters a logarithm: a rank-deficient covariance has no estimate) or larger than the one before it.
 * device outputs, the stream: as rts_cube_mvdr.  The calls are enqueued on the handle's stream and never wait for the device's
 *   earlier work (rts_cube_doa_scan: only for the copy of the PREVIOUS call's g out of the handle's pinned staging block).  The
 *   library-owned eigenpairs and spectrum end at rts_cube_attach; the getters synchronise and copy (RTS_ERR_INVALID with none,
 *   RTS_ERR_CAPACITY when a capacity is too small).  A caller-owned output is not recorded.
 * RTS_ERR_INVALID, the message naming the field: no cube attached; NULL p; nonzero reserved fields; neither device_cov nor a
 *   library-owned covariance; a misaligned device_cov; an n that is 0 or above RTS_BEAM_MAX_RX with device_cov, or differs from the
 *   library-owned covariance's; one of device_values / device_vectors NULL and the other not; a misaligned output; outputs that overlap
 *   each other or the bytes the call reads.  rts_cube_doa_scan: NULL or misaligned device_steering; n_dirs 0 or more than 2^31 - 1
 *   workgroups of 256 directions; m 0; first_vector + m above n; unknown flags; NULL g or a non-finite g_k; neither device_vectors nor
 *   library-owned eigenvectors; a misaligned device_vectors; an n that is 0 or above RTS_BEAM_MAX_RX with device_vectors, or differs
 *   from the library-owned eigenvectors'; a misaligned device_out; a device_out that overlaps the steering table or the vectors.  A
 *   refused call leaves the handle's previous products as they were.
 * rts_eig_eval / rts_doa_scan_eval: pure host, no device: the same rts_doa.h functions.  rts_eig_eval reads cov [n][n] as the kernel
 *   does; sweeps_out (or NULL): the sweeps that rotated (the identity: 0).  Status 1 or 2 returns RTS_ERR_INVALID naming the status.
 *   rts_doa_scan_eval: vectors [m][n] (the rows the scan uses), g [m], steering element-major [n][n_dirs].  A refused or failed
 *   call leaves the outputs untouched. */
#define RTS_EIG_MAX_SWEEPS   30u    /* sweeps that rotate before rts_cube_eig gives up (status 1)                       */
#define RTS_DOA_INVERSE      1u     /* out = 1.0 / q                                                                    */
#define RTS_DOA_BARTLETT     0u
#define RTS_DOA_CAPON        1u
#define RTS_DOA_MUSIC        2u
#define RTS_DOA_AIC          0u
#define RTS_DOA_MDL          1u
typedef struct RtsEigParams {
    uint32_t n, reserved0;           /* n: with device_cov; 0 or the covariance's order otherwise; reserved0: 0         */
    const void* device_cov;          /* complex128 [n][n], 16-byte aligned; NULL: the last library-owned covariance    */
    uint64_t reserved[2];            /* 0 */
} RtsEigParams;
typedef struct RtsDoaScanParams {
    uint32_t n, first_vector;        /* n: with device_vectors; 0 or the eigenvectors' order otherwise                 */
    uint32_t m, flags;               /* rows first_vector .. first_vector + m - 1; RTS_DOA_INVERSE                     */
    uint64_t n_dirs;
    const double* g;                 /* host [m], finite                                                            */
    const void* device_steering;     /* complex128 [n][n_dirs], 16-byte aligned                                     */
    const void* device_vectors;      /* complex128 [n][n], 16-byte aligned; NULL: the last library-owned eigenvectors */
    uint64_t reserved[2];            /* 0 */
} RtsDoaScanParams;
int rts_cube_eig(RtsHandle h, const RtsEigParams* p, void* device_values, void* device_vectors);     /* f64 [n], complex128 [n][n] */
int rts_cube_eig_get(RtsHandle h, double* values_out, double* vectors_out, uint64_t capacity_values, uint64_t capacity_vector_doubles);
int rts_eig_eval(const double* cov, uint32_t n, double* values_out, double* vectors_out, uint32_t* sweeps_out);              /* pure host */
int rts_cube_doa_scan(RtsHandle h, const RtsDoaScanParams* p, void* device_out);                      /* f64 [n_dirs] */
int rts_cube_doa_get(RtsHandle h, double* host_out, uint64_t capacity_doubles);
int rts_doa_scan_eval(const double* vectors, const double* g, uint32_t n, uint32_t m, const double* steering, uint64_t n_dirs,
                      uint32_t flags, double* out);                                                                            /* pure host */
int rts_doa_weights(uint32_t method, const double* values, uint32_t n, uint32_t n_sources, double loading,
                    uint32_t* first, uint32_t* m, double* g, uint32_t* flags);                                                 /* pure host */
int rts_source_count(const double* values, uint32_t n, uint64_t K, uint32_t criterion, uint32_t* n_sources);                  /* pure host */

/* ---------------------------------------------------------------- backprojection imaging (SAR / ISAR) of the return cube
 * A derived product like the cube itself: time-domain backprojection of a coherent interval onto a planar
 * pixel grid -- exact for any track, any bistatic geometry and any target motion, where the slow-time DFT focuses only while a
 * scatterer stays in its range bin.  Input: the attached cube y[rx][pulse][bin] -- range-compressed rows, or the impulse cube of
 * rts_cube_accumulate; t0, dt, n_bins, n_rx are the cube's.  The arithmetic below is rts_amd/csrc/rts_image.h, shared by the kernel
 * and the host evaluator (the library builds with -ffp-contract=off: the tree is the contract).
 *   Pixel (ix, iy) lies at x[c] = origin[c] + (double)ix * step_x[c] + (double)iy * step_y[c], evaluated left to right.
 *   For geometry index j in [0, n_pulses), cube row first_pulse + j and receiver r:
 *     dT  = sqrt(ax*ax + ay*ay + az*az),  a = x - tx_position[j]
 *     dR  = sqrt(bx*bx + by*by + bz*bz),  b = x - rx_position[r][j]
 *     tau = (dT + dR) / cspeed
 *     d   = (tau - t0) / dt
 *     v   = the row interpolated at d:
 *             taps even (2 .. RTS_WAVEFORM_MAX_TAPS): sum_m row[m] h_L(d - m), L = taps, the render's own h_L (RtsWaveform above), 0
 *               outside the row.  With i = floor(d), phi = d - i the L taps are m = i - L/2 + 1 + k, k = 0 .. L-1, summed in ascending
 *               m over those inside [0, n_bins); tap k sits at u = phi + (double)(L/2 - 1 - k), its sinc is (-1)^q sinpi(phi) / (pi u)
 *               (q = L/2 - 1 - k: ONE sinpi per sample) and its window 0.42 + 0.5 C + 0.08 (2 C C - 1) with C = cos(2 pi u / L) taken
 *               directly at the first tap summed and advanced from tap to tap by the rotation (C, S) <- (C cd + S sd, S cd - C sd),
 *               cd = cos(2 pi / L), sd = sin(2 pi / L).  phi = 0 gives row[i] bit for bit (0 outside the row).
 *             taps == 1: row[n], n = floor(d + 0.5); 0 if n is outside [0, n_bins)
 *             a d that is not finite gives 0.
 *     c   = carrier * tau;  f = c - floor(c);  (sn, cs) = sincospi(2 f)     -- undoes the cube's phase -fmod(2 pi fc tau, 2 pi)
 *     term = (w[j] * v) * (cs + j sn), re = a cs - b sn, im = a sn + b cs with (a, b) = (w re v, w im v);  w = pulse_weight, 1 when NULL
 *   image[r][iy][ix] = sum_j term, in ONE order whatever the launch shape: ascending j from 0 inside chunks of RTS_IMAGE_PULSE_CHUNK
 *   pulses, then the chunk sums added in ascending chunk order (the first chunk's sum is the start value) -- bit-identical from
 *   run to run, and a small image of many pulses still fills the GPU (one chunk per workgroup, a second kernel adds them; no atomics).
 *   With RTS_IMAGE_ACCUMULATE the finished sum is added to what the output holds (pulse-sharded GPUs: images are linear in the cube).
 * Geometry: stop-and-go, which is what a traced pulse records (rayLength / c at the pulse time).  All positions are given in the
 * image's frame: for SAR the world frame; for ISAR the caller moves the radar into the target's frame, p' = R_j^T (p - position_j)
 * with RtsTargetMotion's rotation and position of pulse j.
 * A COHERENT image needs a cube accumulated or rendered from rays (rts_cube_accumulate, RTS_RENDER_RAYS): the path products carry
 * the reference's mean of wrapped phases, which is not the phase of any delay.
 * rts_cube_backproject is ordered on the handle's stream and never waits for the device's earlier work (it waits only for the
 * copy of the PREVIOUS call's geometry out of the handle's pinned staging block); the caller's arrays are free on return.
 * device_out: caller-owned device memory of 2 n_rx n_y n_x doubles (16-byte aligned), or NULL: library-owned, alive until the next
 * backprojection of another size, rts_cube_attach or rts_destroy (the rule of the Doppler map).  rts_cube_image_get synchronises and
 * copies the library-owned image; RTS_ERR_INVALID after an rts_cube_attach.  RTS_IMAGE_ACCUMULATE with device_out NULL needs an
 * existing library-owned image of the same shape.
 * RTS_ERR_INVALID, the message naming the field: no cube attached; n_x or n_y zero or n_x n_y > RTS_IMAGE_MAX_PIXELS; taps not 1 and
 * not even in [2, RTS_WAVEFORM_MAX_TAPS]; unknown flags; nonzero reserved fields; n_pulses zero or first_pulse + n_pulses beyond the
 * cube's rows; cspeed not finite or <= 0; carrier not finite or negative; a non-finite position, origin, step or weight; a NULL
 * tx_position or rx_position; more than 65 535 receivers or chunks (the launch grid).
 * rts_backproject_eval: pure host, no device.  The same validation (q in place of the attached cube) and the same rts_image.h
 * functions on a host cube [n_rx][q->n_pulses][n_bins] (interleaved re / im) -> out [n_rx][n_y][n_x] (interleaved), added to
 * with RTS_IMAGE_ACCUMULATE.  A refused call leaves out untouched. */
#define RTS_IMAGE_ACCUMULATE 1u          /* add to the output instead of overwriting it */
#define RTS_IMAGE_PULSE_CHUNK 64u
#define RTS_IMAGE_MAX_PIXELS 16777216u   /* n_x * n_y */
typedef struct RtsImageParams {
    uint32_t n_x, n_y, taps, flags;
    uint32_t first_pulse, n_pulses;      /* cube rows first_pulse .. first_pulse + n_pulses - 1 */
    double origin[3], step_x[3], step_y[3];
    double cspeed, carrier;
    const double* tx_position;           /* [n_pulses][3]           host */
    const double* rx_position;           /* [n_rx][n_pulses][3]     host */
    const double* pulse_weight;          /* [n_pulses] or NULL      host */
    uint64_t reserved[2];                /* 0 */
} RtsImageParams;
int rts_cube_backproject(RtsHandle h, const RtsImageParams* p, void* device_out);   /* complex128 [n_rx][n_y][n_x]; NULL: library-owned */
int rts_cube_image_get(RtsHandle h, double* host_out, uint64_t capacity_doubles);
int rts_backproject_eval(const RtsCubeParams* q, const double* cube, const RtsImageParams* p, double* out);  /* pure host, no device */

/* ---------------------------------------------------------------- autofocus: range alignment, phase-gradient autofocus, correction
 * Motion compensation of a target whose motion is NOT known (rts_cube_doppler needs a scatterer that stays in its bin with a pure
 * tone for a phase history, rts_cube_backproject needs every pulse's positions): first the rows' range walk is estimated from their
 * envelopes and taken out, then the pulse-to-pulse phase error is estimated from the data and taken out.  Three operations, all
 * ordered on the handle's stream, none waits on the host.  "Rows" are cube rows first_pulse + j, j in [0, P), P = n_pulses; every
 * receiver is treated on its own.  The arithmetic is rts_amd/csrc/rts_focus.h, shared by the kernels and the host evaluators (the
 * library builds with -ffp-contract=off: the trees below are the contract).
 *
 * rts_cube_align: range shifts S, f64 [n_rx][P], in bins, against a GLOBAL reference (adjacent-pulse lags accumulate their errors
 *   into a drift; these do not).  The lag is absolute: max_lag L must cover the whole walk.
 *   Envelope e[j][n] = sqrt(re*re + im*im) over the whole row; a read outside [0, n_bins) gives 0.  The gate is bins first_bin ..
 *   first_bin + n_gate - 1 (n_gate 0: to the row's last bin).  S = 0, then n_iters times:
 *     R_j    = (int64) floor(S_j + 0.5)
 *     ref[n] = sum_j e[j][n + R_j] for every gate bin n: ascending j from 0 inside chunks of RTS_ALIGN_PULSE_CHUNK pulses, the chunk
 *              sums added in ascending order, the first chunk's sum the start value (the image's rule)
 *     C_j(l) = sum_{n in gate} ref[n] * e[j][n + l], l in [-L, L]: each product rounded before it is added; ascending n from 0.0
 *              inside blocks of RTS_ALIGN_BIN_BLOCK consecutive gate bins counted from the gate's first bin, the block sums added
 *              left to right from 0.0 (the plots' rule)
 *     l*     : scan l = 0, -1, +1, -2, +2, ..., -L, +L and replace only on a strict >: a NaN never wins, an all-zero row gives 0,
 *              ties go to the smaller |l| and then to the negative lag
 *     delta  : 0 with RTS_ALIGN_INTEGER or |l*| == L; else den = C(l*-1) - 2 C(l*) + C(l*+1) and, when den < 0,
 *              delta = 0.5 * (C(l*-1) - C(l*+1)) / den clamped to [-0.5, 0.5] (0 when den >= 0 or not a number)
 *     S_j    = (double)l* + delta
 *   IEEE basic operations in a fixed order: the device and rts_align_eval agree BIT FOR BIT.
 *   device_out: caller-owned device memory of n_rx P doubles (8-byte aligned), or NULL: library-owned, recorded as the handle's
 *   shift table (rts_cube_align_get synchronises and copies it; RTS_CORRECT_USE_ALIGN takes it on the device), alive until the next
 *   alignment of another size, rts_cube_attach or rts_destroy.  A caller-owned output is not recorded.
 *   Memory: the envelopes of the rows, 8 n_rx P n_bins bytes of handle-owned scratch.
 *   Regime: point-like scatterers well above the noise in the gate.  On an ungated row at 0 dB per-sample SNR the reference is
 *   mostly noise and the estimate is lost; gate the target.
 *
 * rts_cube_pga: the phase error phi, f64 [n_rx][P] in cycles, by phase-gradient autofocus; it does not change the cube.  N = P must be
 *   a power of two in [4, RTS_PGA_MAX_PULSES] (the transform is rts_stft.h's radix-2 tree; zero padding would put a step into the
 *   phase history).  phi = 0, W = window0 (0: N / 2); per iteration and gate column n:
 *     x[p] = y[p][n] * exp(-j 2 pi phi[p]): f = phi - floor(phi), (sn, cs) = sincospi(2 f) (the image's rotation), re = vr cs + vi sn,
 *            im = vi cs - vr sn -- always from the UNCHANGED cube: nothing accumulates in the data
 *     X    = the forward transform of rts_stft.h (bit-reversed load, rts_stft_pair / rts_stft_butterfly, the twiddle table)
 *     k*   = the first maximum of re*re + im*im in ascending k
 *     Y[k] = X[(k + k*) mod N] where min(k, N - k) <= W / 2 (integer division), else 0
 *     g    = conj(T(conj(Y))), T the same tree; no 1 / N
 *     a[p] = g[p] conj(g[p-1]), re = gr hr + gi hi, im = gi hr - gr hi, p >= 1; a[0] = 0
 *   A[p] = sum_n a_n[p]: ascending gate bins from 0.0 inside tiles of RTS_PGA_BIN_TILE consecutive gate bins, the tile sums added in
 *   ascending tile order, the first tile's sum the start value (RTS_STFT_SUM_BINS' scheme; no atomics).  Then per receiver:
 *     D[0] = 0, D[p] = atan2(Im A[p], Re A[p]) / (2 pi) (0 when both are 0);  psi = the running sum of D, left to right
 *     x_p = (double)p - (N - 1) / 2.0;  mean = sum psi / N;  slope = sum x_p psi_p / sum x_p x_p (sums left to right from 0.0)
 *     psi'_p = psi_p - mean - slope * x_p  -- the image neither rotates nor shifts in Doppler
 *     phi += psi';  rms[i] = sqrt(sum psi'^2 / N) in cycles;  W = max(window_min, W / 2)   (window_min 0: 8)
 *   Output: phi f64 [n_rx][P], then the convergence record rms f64 [n_rx][n_iters], n_rx (P + n_iters) doubles in all.  device_out:
 *   caller-owned (8-byte aligned), or NULL: library-owned, recorded as the handle's phase table (rts_cube_pga_get copies whichever of
 *   phase_out and rms_out is not NULL; RTS_CORRECT_USE_PGA takes it on the device).
 *   The twiddles, sincospi and atan2 are the device library's on the device and libm's on the host: the device and rts_pga_eval
 *   agree to a tolerance (tests/test_gpu_focus.py), not to the bit; a column whose two largest |X[k]|^2 tie may pick another k*.
 *   Run it on an ALIGNED cube, on a gate that holds the target: it needs a dominant scatterer per column that stays in its bin.
 *
 * rts_cube_correct: shifts and / or phases applied to the cube IN PLACE.  For each row and bin n:
 *     d = (double)n + S;  v = the old row interpolated at d (RtsImageParams above: taps, the same interpolator; S == 0 gives the row
 *     bit for bit);  then the rotation of rts_cube_pga's load by phi.
 *   Without shifts nothing is resampled (no copy is made: a thread reads only the element it writes), without phases nothing is
 *   rotated; with shifts the rows are copied to a handle-owned scratch first and the kernel reads the copy.  Rows outside the range
 *   are not touched.  shifts, phase: host arrays [n_rx][P] or NULL; they go through a staged upload and are free on return.
 *   RTS_CORRECT_USE_ALIGN / RTS_CORRECT_USE_PGA take the handle's library-owned tables on the device instead, without a host wait;
 *   the table must have been made for the same first_pulse and n_pulses.
 *   The Doppler map, the image and the other recorded products of the cube are NOT invalidated (nor are they by rts_cube_compress or
 *   rts_cube_add_sources): a product made before the correction is a product of the cube as it was.
 *
 * RTS_ERR_INVALID, the message naming the field, outputs untouched: no cube attached; NULL p; nonzero reserved fields; unknown flags;
 * n_pulses 0 or rows beyond the cube; a gate beyond the row; max_lag above RTS_ALIGN_MAX_LAG; n_iters outside [1, RTS_ALIGN_MAX_ITERS] /
 * [1, RTS_PGA_MAX_ITERS]; n_pulses of rts_cube_pga not a power of two in [4, RTS_PGA_MAX_PULSES]; taps not 1 and not even in [2,
 * RTS_WAVEFORM_MAX_TAPS]; a host shift or phase that is not finite; a flag together with the matching host pointer; neither shifts nor
 * phases; a flag without a valid table of the same rows; a device_out that is not 8-byte aligned; more than 65 535 receivers, or
 * rows x ceil(n_bins / 256) above 2^31 - 1 (the launch grids).  A cube that is not finite gives unspecified values, but nothing is
 * read or written outside the cube and the outputs.
 * rts_align_eval, rts_pga_eval, rts_correct_eval: pure host, no device; the same validation (q in place of the attached cube; the
 * USE flags are refused) and the same rts_focus.h functions on a host cube [n_rx][q->n_pulses][n_bins] (interleaved re / im), which
 * rts_correct_eval changes in place. */
#define RTS_ALIGN_INTEGER 1u             /* no sub-bin refinement */
#define RTS_ALIGN_MAX_LAG 64u
#define RTS_ALIGN_MAX_ITERS 8u
#define RTS_ALIGN_PULSE_CHUNK 64u        /* the summation order of ref, see above */
#define RTS_ALIGN_BIN_BLOCK 64u          /* the summation order of C, see above   */
typedef struct RtsAlignParams {
    uint32_t first_pulse, n_pulses;      /* cube rows first_pulse .. first_pulse + n_pulses - 1 */
    uint32_t first_bin, n_gate;          /* the gate; n_gate 0: to the row's last bin           */
    uint32_t max_lag, n_iters, flags, reserved0;
    uint64_t reserved[2];                /* 0 */
} RtsAlignParams;
#define RTS_PGA_MAX_PULSES 4096u
#define RTS_PGA_MAX_ITERS 16u
#define RTS_PGA_BIN_TILE 8u              /* the summation order of A, see above */
typedef struct RtsPgaParams {
    uint32_t first_pulse, n_pulses;      /* n_pulses: a power of two in [4, RTS_PGA_MAX_PULSES] */
    uint32_t first_bin, n_gate;          /* the gate; n_gate 0: to the row's last bin           */
    uint32_t n_iters, window0, window_min, reserved0;      /* window0 0: n_pulses / 2; window_min 0: 8 */
    uint64_t reserved[2];                /* 0 */
} RtsPgaParams;
#define RTS_CORRECT_USE_ALIGN 1u         /* shifts: the handle's library-owned table of rts_cube_align */
#define RTS_CORRECT_USE_PGA 2u           /* phases: the handle's library-owned table of rts_cube_pga   */
typedef struct RtsCorrectParams {
    uint32_t first_pulse, n_pulses, taps, flags;
    const double* shifts;                /* [n_rx][n_pulses] bins, or NULL    host */
    const double* phase;                 /* [n_rx][n_pulses] cycles, or NULL  host */
    uint64_t reserved[2];                /* 0 */
} RtsCorrectParams;
int rts_cube_align(RtsHandle h, const RtsAlignParams* p, void* device_out);          /* f64 [n_rx][n_pulses]; NULL: library-owned */
int rts_cube_align_get(RtsHandle h, double* host_out, uint64_t capacity_doubles);
int rts_cube_pga(RtsHandle h, const RtsPgaParams* p, void* device_out);              /* f64 [n_rx][n_pulses] phase, then [n_rx][n_iters] rms */
int rts_cube_pga_get(RtsHandle h, double* phase_out, double* rms_out, uint64_t capacity_phase, uint64_t capacity_rms);
int rts_cube_correct(RtsHandle h, const RtsCorrectParams* p);
int rts_align_eval(const RtsCubeParams* q, const double* cube, const RtsAlignParams* p, double* out);                          /* pure host */
int rts_pga_eval(const RtsCubeParams* q, const double* cube, const RtsPgaParams* p, double* phase_out, double* rms_out);      /* pure host */
int rts_correct_eval(const RtsCubeParams* q, double* cube, const RtsCorrectParams* p);                                        /* pure host */

/* ---------------------------------------------------------------- passive radar: reference-channel cancellation and cross-correlation
 * A passive receiver has no waveform of its own: a transmitter of opportunity sends a noise-like signal that differs in every
 * coherent row, one receiver (ref_rx, the reference channel) records it, the others (the surveillance channels) record its echoes
 * under the direct signal and the static clutter, 40 - 80 dB above them.  Two steps turn such a cube [n_rx][n_pulses][n_bins] --
 * rendered with a new waveform segment per pulse (rts_cube_set_waveform + rts_cube_render with RTS_RENDER_DOPPLER), the reference
 * row and any direct or clutter terms written by the caller into a caller-owned cube -- into the input of the existing chain:
 * rts_cube_cancel removes from the surveillance rows what the reference explains, rts_cube_xcorr correlates every row with the
 * reference row of the same pulse.  The output attached as a cube of n_bins = n_lags, t0 = first_lag * dt, then rts_cube_doppler:
 * that IS the cross-ambiguity function by the batches algorithm, and detection, plots, tracks and localisation follow unchanged.
 * The rows are independent batches: a read outside a row is 0.  The arithmetic is rts_amd/csrc/rts_passive.h, shared by the kernels
 * (rts_passive.hip) and the host evaluators; the trees hold + - * / and sqrt only and the library builds with -ffp-contract=off, so
 * device and evaluators agree BIT FOR BIT.
 *
 * rts_cube_cancel (batch ECA: a least-squares projection, in place on the surveillance rows; the reference rows are never written).
 *   K = n_taps; x_k[p][n] = ref[p][n - k], +0.0 for n < k.  The span first_pulse .. first_pulse + n_pulses - 1 is cut into blocks of
 *   rows_per_block consecutive rows (0, or more than n_pulses: the whole span is one block; the last block may be shorter),
 *   n_blocks = ceil(n_pulses / rows_per_block).  Per block, with the sums over the block's rows p and all bins n:
 *     G[i][j] = sum conj(x_i) x_j    (K x K Hermitian, the lower triangle j <= i is formed; shared by every receiver)
 *     b_r[i]  = sum conj(x_i) y_r    (per cancelled receiver r)
 *     term: a conj(b) = (ar br + ai bi, ai br - ar bi) with b = x_i and a = x_j or y_r; a term whose x is the +0.0 above is formed
 *       and added like any other.
 *     The sums' tree: a row is cut into ceil(n_bins / RTS_PASSIVE_TILE) tiles of consecutive bins; the block's tiles, numbered
 *       row-major, are cut into parts = min(tiles, max(1, RTS_PASSIVE_MAX_PARTS / n_blocks)) parts, part q owning the tiles
 *       floor(q tiles / parts) .. floor((q + 1) tiles / parts) - 1.  A part's sum runs over its cells in ascending order, the first
 *       term the start value; the parts are summed in ascending q, part 0 the start value.  A function of the shape alone.
 *     A = G + loading I (one add per diagonal real part; loading >= 0, finite, in the cube's power units times the block's cells),
 *       factored and solved as rts_cube_mvdr factors and solves (column Cholesky, forward then back substitution; no division by a
 *       norm): A c_r = b_r.
 *     y_r[p][n] <- y_r[p][n] - c_r[0] x_0[p][n] - ... - c_r[K-1] x_{K-1}[p][n], k ascending, each step
 *       y - c x = (yr - (cr xr - ci xi), yi - (cr xi + ci xr)).
 *   A FAILED BLOCK: a pivot that is not finite or not > 0 (fewer samples than taps with loading 0, an all-zero or a non-finite
 *     reference).  The block's rows stay as they are for every receiver, its coefficients are 0, and it is counted.
 *   rx_mask: bit r set: receiver r is cancelled; 0: every receiver but ref_rx.  The rows of the others stay bit-identical.
 *   The block length is the notch: coefficients estimated per block remove everything inside the K lags whose phase turns by less
 *     than about one cycle over the block, so rows_per_block rows give a Doppler notch of about 1 / (rows_per_block PRI) around 0.  A
 *     target survives at a lag >= K, or at a Doppler of several cycles per block.
 *   rts_cube_cancel_info: n_blocks and the failed blocks of the last call.  The failed blocks are counted from the blocks' pivot
 *   words on the device at every call: a stream synchronisation and a blocking copy of n_blocks words, a device round trip (pass
 *   n_failed_out NULL to skip it).  rts_cube_cancel_coeffs_get: the
 *   coefficients, complex128 [n_rx][n_blocks][K]; the slots of ref_rx and of receivers outside the mask hold zeros.  Both end at
 *   rts_cube_attach.  The other products of the cube are not invalidated (as with rts_cube_compress).
 * rts_cube_xcorr (out of place).  For every receiver r -- ref_rx too: its row is the reference's autocorrelation, by which a
 *   caller judges the waveform -- and every row p of the span:
 *     z[r][p][l - first_lag] = sum_{n = 0}^{n_bins - 1 - l} y_r[p][n + l] conj(ref[p][n]),   l = first_lag .. first_lag + n_lags - 1
 *   n ascending, the first term the start value, the term the one above with a = y, b = ref; a lag at or beyond n_bins gives
 *   (+0.0, +0.0).  Output complex128 [n_rx][n_pulses (the span's)][n_lags] into device_out (caller-owned device memory, 16-byte
 *   aligned, apart from the cube) or, with NULL, library-owned memory that rts_cube_xcorr_get copies; it ends at rts_cube_attach.
 *   Limits: n_bins <= RTS_COMPRESS_MAX_BINS, n_lags <= RTS_XCORR_MAX_LAGS, first_lag <= RTS_XCORR_MAX_FIRST_LAG, at most 65 535
 *   receivers and span rows.  The surveillance row passes through a workgroup's LDS in windows of 256 + 256 samples (8 KiB of the
 *   160 KiB a gfx950 workgroup may allocate), one thread per lag: LDS bounds neither n_bins nor n_lags.  The cancellation's workgroups
 *   hold a tile with its K - 1 samples of history (at most 319 complex128: 5 104 bytes) and, in the solve, the factor and the work
 *   vectors (16 K K + 1 024 K bytes: 128 KiB at K = 64).
 * The calls are enqueued on the handle's stream and never wait for the device's earlier work.
 * RTS_ERR_INVALID, the message naming the field: no cube attached; NULL p; a cube that is not 16-byte aligned.  rts_cube_cancel,
 *   rts_cancel_eval: (1) nonzero reserved fields; (2) more than RTS_PASSIVE_MAX_RX receivers; (3) ref_rx >= n_rx; (4) n_taps outside
 *   1 .. RTS_PASSIVE_MAX_TAPS; (5) a span of no pulse or outside the cube; (6) a loading that is negative or not finite; (7) ref_rx
 *   inside rx_mask; (8) rx_mask naming a receiver the cube does not have; (9) more than RTS_PASSIVE_MAX_BLOCKS blocks.
 *   rts_cube_xcorr, rts_xcorr_eval: (1) nonzero reserved fields; (2) ref_rx >= n_rx; (3) a span of no pulse or outside the cube;
 *   (4) n_lags outside 1 .. RTS_XCORR_MAX_LAGS; (5) first_lag above RTS_XCORR_MAX_FIRST_LAG; (6) n_bins above RTS_COMPRESS_MAX_BINS;
 *   (7) more than 65 535 receivers or span rows; and a misaligned device_out or one that overlaps the cube.  The getters: nothing to
 *   return (no call yet, or an rts_cube_attach since), a NULL output; RTS_ERR_CAPACITY when the capacity is too small.  A refused
 *   call leaves the cube and the handle's products as they were.
 * rts_cancel_eval / rts_xcorr_eval: pure host, no device: the same rts_passive.h functions on host arrays of the cube's layout, q its
 *   shape.  rts_cancel_eval works in place on cube_inout; coeffs_out ([n_rx][n_blocks][K] complex128), n_blocks_out and n_failed_out
 *   may each be NULL. */
#define RTS_PASSIVE_MAX_TAPS    64u      /* K                                                                                  */
#define RTS_PASSIVE_MAX_RX      64u      /* the bits of rx_mask                                                                */
#define RTS_PASSIVE_TILE        256u     /* bins per tile of the sums' tree                                                    */
#define RTS_PASSIVE_MAX_PARTS   512u     /* parts of all blocks together, while a block has at least one                       */
#define RTS_PASSIVE_MAX_BLOCKS  4096u    /* the parts' scratch is blocks * parts * (K (K + 1) / 2 + n_rx K) * 16 bytes         */
#define RTS_XCORR_MAX_LAGS      16384u
#define RTS_XCORR_MAX_FIRST_LAG 0x7fff0000u
typedef struct RtsCancelParams {
    uint32_t ref_rx, n_taps;         /* the reference channel; K: 1 .. RTS_PASSIVE_MAX_TAPS                          */
    uint32_t first_pulse, n_pulses;  /* the span: at least one pulse                                                 */
    uint32_t rows_per_block;         /* 0: the whole span is one block                                               */
    uint32_t reserved0;              /* 0 */
    uint64_t rx_mask;                /* the receivers cancelled; 0: all but ref_rx                                   */
    double loading;                  /* >= 0, finite: added to G's diagonal                                          */
    uint64_t reserved[2];            /* 0 */
} RtsCancelParams;                                            /* 56 bytes */
typedef struct RtsXcorrParams {
    uint32_t ref_rx, reserved0;      /* the reference channel; 0                                                     */
    uint32_t first_pulse, n_pulses;  /* the span: at least one pulse                                                 */
    uint32_t first_lag, n_lags;      /* lags first_lag .. first_lag + n_lags - 1                                     */
    uint64_t reserved[2];            /* 0 */
} RtsXcorrParams;                                             /* 40 bytes */
int rts_cube_cancel(RtsHandle h, const RtsCancelParams* p);
int rts_cube_cancel_info(RtsHandle h, uint32_t* n_blocks_out, uint32_t* n_failed_out);
int rts_cube_cancel_coeffs_get(RtsHandle h, double* host_out, uint64_t capacity_doubles);   /* complex128 [n_rx][n_blocks][K] */
int rts_cancel_eval(const RtsCubeParams* q, double* cube_inout, const RtsCancelParams* p, double* coeffs_out, uint32_t* n_blocks_out,
                    uint32_t* n_failed_out);                                                                                  /* pure host */
int rts_cube_xcorr(RtsHandle h, const RtsXcorrParams* p, void* device_out);                 /* complex128 [n_rx][n_pulses][n_lags] */
int rts_cube_xcorr_get(RtsHandle h, double* host_out, uint64_t capacity_doubles);
int rts_xcorr_eval(const RtsCubeParams* q, const double* cube, const RtsXcorrParams* p, double* out);                        /* pure host */

/* ---------------------------------------------------------------- MIMO radar: the matched-filter bank, to a virtual-array cube
 * Several transmitters, each with its own waveform, render into ONE cube (rts_cube_render adds; handles may share a cube).  The bank
 * takes them apart again: one matched filter per transmit waveform on every receive row.  Its output is a cube of n_waves * n_rx
 * VIRTUAL elements -- element t * n_rx + r is what receiver r heard of transmitter t, and for a far target it is the sample of a
 * physical element at rx_position[r] + tx_offset[t] -- which the array families (beamformer, covariance, MVDR, STAP, eigensolver,
 * angular scan) take as it stands once it is attached as a cube of n_waves * n_rx receivers.
 * For waveform t (samples s_t[0 .. M_t - 1]), receiver r, pulse p of the call's row range and bin n:
 *     z[n]                            = sum over m = 0 .. M_t - 1, ascending, of  y[r][p][n + m] (x) conj(s_t[m])
 *     out[t * n_rx + r][p - first][n] = conj(code[t][p - first]) (x) z[n]          (code NULL: z[n] itself, no multiply formed)
 *   The tree is rts_cube_compress's: the sums start at +0.0; a term with n + m >= n_bins is not formed; per term
 *   zr += yr sr + yi si and zi += yi sr - yr si, every operation rounded on its own (the library builds with -ffp-contract=off; no
 *   MFMA); the code multiply is (cr zr + ci zi, cr zi - ci zr).  The arithmetic is rts_amd/csrc/rts_mimo.h, shared by the kernel
 *   (rts_mimo.hip) and rts_bank_eval: device and evaluator agree BIT FOR BIT, whatever the kernel's tiling.
 *   Output: out of place, complex128 [n_waves * n_rx][n_pulses of the call][n_bins], into device_out (caller-owned device memory,
 *   16-byte aligned, apart from the rows the call reads) or, with NULL, library-owned memory that rts_cube_bank_get copies; that
 *   product ends at rts_cube_attach.  The cube is not changed.  Attaching the output ends the handle's products, so an output that is
 *   to be attached must be caller-owned.
 *   code: an optional HOST table [n_waves][n_pulses of the call] of complex128, the slow-time code of each transmitter (TDM: zeros and
 *   ones; DDMA: a phase ramp per transmitter), finite.  A zero entry gives a row of zeros by the same multiply, not by a skip.  The
 *   render side has no slow-time code: the caller renders transmitter t at pulse p with the waveform code[t][p] * s_t.
 *   waves: n_waves records (1 .. RTS_BANK_MAX_WAVES) that each pass rts_cube_set_waveform's rule; `taps` is validated and not
 *   used; the waveforms of one set may differ in length.  The samples and the code table are copied before the call returns.
 *   Limits: the output holds at most RTS_BANK_MAX_CELLS cells (its size is formed without a product that could wrap); the launch
 *   has at most 2^31 - 1 workgroups.  n_bins is NOT bounded by a workgroup's LDS (a workgroup stages RTS_BANK_TILE + max M - 1
 *   samples of a row, at most 73 984 bytes), nor is n_waves.  The bank does not bound n_waves * n_rx either; RTS_BEAM_MAX_RX
 *   bounds what the array families accept afterwards.
 *   Not here: FFT-based fast convolution (a different tree), the design of waveform sets, Doppler-tolerant banks.
 * The call is enqueued on the handle's stream and never waits for the device's earlier work.
 * RTS_ERR_INVALID, the message naming the field: no cube attached; NULL p; (1) nonzero reserved fields; (2) n_waves outside
 *   1 .. RTS_BANK_MAX_WAVES; (3) NULL waves; a waveform that rts_cube_set_waveform would refuse; (4) a span of no pulse or outside
 *   the cube; (5) a code entry that is not finite; (6) an output beyond RTS_BANK_MAX_CELLS cells or a launch beyond 2^31 - 1
 *   workgroups; a cube or a device_out that is not 16-byte aligned; a device_out that overlaps the rows the call reads.  The getter:
 *   nothing to return (no call with device_out NULL yet, or an rts_cube_attach since), a NULL output; RTS_ERR_CAPACITY when the
 *   capacity is too small.  A refused call leaves the output and the handle's products as they were.
 * rts_bank_eval: pure host, no device: the same rts_mimo.h functions on a host array of the cube's layout, q its shape. */
#define RTS_BANK_MAX_WAVES 16u
#define RTS_BANK_TILE      512u             /* output bins per workgroup                                                    */
#define RTS_BANK_MAX_CELLS 549755813888ull  /* 2^39 complex128 of output: what a flat launch of the beamformer may write    */
typedef struct RtsBankParams {
    const RtsWaveform* waves;        /* [n_waves]                                                                    */
    uint32_t n_waves;                /* 1 .. RTS_BANK_MAX_WAVES                                                      */
    const double* code;              /* NULL, or host [n_waves][n_pulses] interleaved re / im, finite                */
    uint32_t first_pulse, n_pulses;  /* the span: at least one pulse                                                 */
    uint64_t reserved[2];            /* 0 */
} RtsBankParams;                                              /* 48 bytes */
int rts_cube_bank(RtsHandle h, const RtsBankParams* p, void* device_out);                   /* complex128 [n_waves * n_rx][n_pulses][n_bins] */
int rts_cube_bank_get(RtsHandle h, double* host_out, uint64_t capacity_doubles);
int rts_bank_eval(const RtsCubeParams* q, const double* cube, const RtsBankParams* p, double* out);                          /* pure host */

/* ---------------------------------------------------------------- several GPUs (not in the reference: it is single-GPU)
 * Rays are independent (each launch index writes only its own rows, ray_tracer.cu:227-253) and so are pulses
 * (ray_tracer.cpp:843).  rts_plan_cpi deals the n_pulses x total_rays (pulse, launch index) pairs of one coherent
 * processing interval to `world` workers -- one handle set per GPU, in one process (rts_adapter.hpp) or one process per
 * GPU (bench.py) -- and returns worker `rank`'s share as RtsPulse-ready items:
 *   RTS_SHARD_PULSES  n_pulses / world whole pulses per worker; each of the n_pulses % world left-over pulses is shared by a
 *                     group of consecutive workers in interleaved tiles (RtsPulse.interleave_*)
 *   RTS_SHARD_RAYS    every pulse is split over all workers in interleaved tiles (work per worker independent of how
 *                     n_pulses divides by world)
 *   RTS_SHARD_PULSES_WHOLE  whole pulses only, contiguous runs, the first n_pulses % world workers one pulse more (a part of a pulse
 *                     is a launch of another shape whose schedule starts from nothing: on short intervals of small pulses that costs
 *                     more than one pulse of imbalance); with fewer pulses than workers: as RTS_SHARD_PULSES
 * min_items > 1 splits items further (part p of P -> parts p and p + P of 2 P) until the worker owns that many, so that
 * it can keep min_items pulses (or parts) in flight.  Parts of one pulse are merged again through their group tables
 * (rts_aggregate with RTS_BASE_USE_ROWS, rts_merge_groups) or through their received sets ordered by RtsResponse.ray /
 * slots.  Pure host code. */
typedef struct RtsPlanItem {
    uint32_t pulse;
    uint32_t interleave_tile, interleave_parts, interleave_part;   /* parts <= 1: the whole range */
    uint64_t ray_first, ray_count;
} RtsPlanItem;
#define RTS_SHARD_PULSES 0u
#define RTS_SHARD_RAYS 1u
#define RTS_SHARD_PULSES_WHOLE 2u
#define RTS_PLAN_TILE 4096u      /* default launch indices per interleaved tile (a multiple of 64 keeps the tile-cost history) */
int rts_plan_cpi(uint64_t total_rays, uint32_t n_pulses, uint32_t rank, uint32_t world, uint32_t mode, uint32_t min_items,
                 uint32_t tile /* launch indices per interleaved tile; 0 = RTS_PLAN_TILE */, RtsPlanItem* out, uint32_t capacity,
                 uint32_t* n_out);
/* Ray sharding BALANCED BY LAST-SEEN COST (instead of the static interleave): the tiles of a pulse are dealt to the workers
 * longest-first from what every tile cost the last time any worker traced it -- one exchange of a cost table per interval.
 * (The reference is single-GPU, ray_tracer.cpp:1165 is one rtContextLaunch1D over all W^3 indices; rays are independent,
 * ray_tracer.cu:227-253, so any partition of the launch indices gives the same rows.)
 *   rts_tile_records_get   the handle's cost records (one uint32 per 64 consecutive launch indices of the W^3 lattice, n =
 *                          ceil(W^3 / 64); bits 0-29 wave time in units of 64 shader clocks, bits 30-31 the walk-length flags of
 *                          the cooperative kernel's head rule) of the tiles its LAST launch traced, 0 for every other tile:
 *                          tables of workers that traced disjoint parts of a pulse merge with a plain sum (or max)
 *   rts_tile_records_set   replaces the handle's history with a merged table: its next launches order their tiles -- and pick
 *                          the cooperative kernel's head tiles -- from what ANY worker measured
 *   rts_deal_tiles         host code, deterministic (every worker computes the same map from the same table): first the plan tiles of `tile`
 *                          launch indices (a multiple of 64) that hold walk-length flags (the cooperative kernel's candidates), in descending
 *                          cost, each to the worker holding the fewest flagged wave tiles so far; then the others in descending cost, each to
 *                          the worker with the least cost so far; tiles without a record are then dealt by COUNT (ascending, each to the worker holding the fewest tiles).  part_of_tile[ceil(total_rays / tile)] <- worker
 *   rts_set_tile_list      the plan tiles (ascending, unique, < ceil(range / tile)) the handle's launches with
 *                          interleave_parts == RTS_INTERLEAVE_LIST trace; n_ids == 0 is an EMPTY list (a worker that was dealt nothing:
 *                          its launches trace no launch index and return empty sets); tile == 0 forgets the list */
int rts_tile_records_get(RtsHandle h, uint32_t* records, uint32_t n);
int rts_tile_records_set(RtsHandle h, const uint32_t* records, uint32_t n);
int rts_deal_tiles(const uint32_t* records, uint32_t n_records, uint64_t total_rays, uint32_t tile, uint32_t parts, uint32_t* part_of_tile, uint64_t* cost_of_part /* [parts] or NULL */);
int rts_set_tile_list(RtsHandle h, uint32_t tile, const uint32_t* tile_ids, uint32_t n_ids);
/* Sum of the complex return cubes of several handles (same RtsCubeParams; one handle per GPU, or several per GPU), left in
 * EVERY handle's cube: the "RCCL reduce over the per-receiver return buffers" of a multi-GPU interval when all GPUs belong
 * to one process.  transport 0: RCCL (ncclCommInitAll + ncclAllReduce, loaded on first use) when the handles sit on
 * distinct devices and librccl can be loaded, otherwise peer copies; 1: RCCL or fail; 2: peer copies (hipMemcpyPeer +
 * add, in handle order -- bit-reproducible). */
int rts_cube_reduce(RtsHandle* handles, uint32_t n_handles, int transport);

/* ---------------------------------------------------------------- the reference's inner C-like boundary
 * Same argument list and in/out behaviour as rs::kernel_wrapper (aggregation.cuh:19-22,
 * aggregation.cu:103-184); the C++ symbol rs::kernel_wrapper is exported by the library too
 * (include/rts_adapter.hpp).  Returns a status instead of exiting. */
int rts_kernel_wrapper(struct PerRayData* h_rx_results_arr, int* h_rx_intersects_arr, unsigned int receivedRays,
                       unsigned int depthTotal, unsigned int MaxThreads, unsigned int MaxBlocks, double cspeed,
                       double carrier, double* h_npath_arr, double* h_power_arr, double* h_doppler_arr,
                       double* h_delay_arr, double* h_phase_arr, int* h_pathMatch);
/* The same on the device and stream of a handle (NULL: a process-wide context of the calling thread's current device, one
 * per device, which is what rts_kernel_wrapper and rs::kernel_wrapper use).  The handle's own received set is overwritten.
 * rs::kernel_wrapper (void in the reference, which exit(1)s on error) throws std::runtime_error on failure. */
int rts_kernel_wrapper_on(RtsHandle h, struct PerRayData* h_rx_results_arr, int* h_rx_intersects_arr, unsigned int receivedRays,
                          unsigned int depthTotal, unsigned int MaxThreads, unsigned int MaxBlocks, double cspeed,
                          double carrier, double* h_npath_arr, double* h_power_arr, double* h_doppler_arr,
                          double* h_delay_arr, double* h_phase_arr, int* h_pathMatch);

/* ---------------------------------------------------------------- host scene helpers (ray_tracer.cpp:85-504, 894-918)
 * Two-call pattern for the variable-size builders: pass NULL outputs to obtain the sizes. */
int rts_vertex_rotation(double* vertices, uint32_t n, float yaw, float pitch, float roll);          /* :156-170 */
int rts_rotation_matrix(float yaw, float pitch, float roll, double* r9);                             /* :159-162 */
int rts_rect_mesh(float w, float h, float d, float yaw, float pitch, float roll, double* vertices24,
                  uint32_t* triangles36, double* normals36);                                         /* :226-297 */
int rts_sphere_mesh(uint32_t subdivisions, float radius, float yaw, float pitch, float roll, double* vertices,
                    uint32_t* n_vertices, uint32_t* triangles, uint32_t* n_triangles, double* normals); /* :300-426 */
int rts_file_mesh(const char* v_file, const char* n_file, float yaw, float pitch, float roll, double* vertices,
                  uint32_t* triangles, double* normals, uint32_t* n_triangles);                      /* :429-504 */
int rts_rx_sphere(const double* rx_position, double azimuth, double elevation, double radius, double theta_span,
                  double phi_span, RtsReceiverSphere* out);                                          /* :894-918 */

/* ---------------------------------------------------------------- introspection (tests)
 * The static target-space hierarchy built by rts_set_scene: nodes[RtsSceneInfo.n_nodes] as stored (128-byte records: lo x,y,z /
 * hi x,y,z planes of the four children as 6 x float[4], int32 child[4] (>= 0 node, < 0 ~leaf slot, 0x7fffffff unused),
 * int32 pad[4]); leaf_prim[*n_leaves] = global primitive id per leaf slot (primitives with a coordinate that is not finite, or not
 * below 3.0e38 in magnitude -- its padded f32 box would not be finite --, have none, whichever builder ran; a primitive whose box is mostly empty has several slots, each boxing a part of it -- "split references");
 * roots[n_targets] = root node per target (-1: no geometry).  Any output may be NULL (sizes: call with NULLs first). */
int rts_get_bvh(RtsHandle h, void* nodes128, uint32_t* leaf_prim, int32_t* roots, uint32_t node_capacity,
                uint32_t leaf_capacity, uint32_t* n_leaves);
/* The host SAH builder (rts_sah.cpp; RTS_FLAG_HOST_BUILD) on one mesh, without a device: nodes128 / leaf_prim as rts_get_bvh returns
 * them (leaf_prim[slot] = triangle index of the mesh).  Null outputs: sizes only.  Pure host code. */
int rts_build_hierarchy_host(const double* vertices, const uint32_t* triangles, uint32_t n_triangles, double split_budget, void* nodes128,
                             uint32_t node_capacity, uint32_t* leaf_prim, uint32_t leaf_capacity, uint32_t* n_nodes, uint32_t* n_leaves,
                             int32_t* root);
int rts_self_test_math(RtsHandle h, const float* y, const float* x, float* atan2f_out, const double* a,
                       const double* b, double* div_out, double* sqrt_out, uint32_t n);

#ifdef __cplusplus
}
#endif
#endif /* RTS_AMD_H */
