// rts_internal.h -- device-side data layout and the host context of librts_amd.so.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stddef.h>
#include <atomic>
#include <string>
#include <vector>
#include "../../include/rts_amd.h"
#include "rts_device_math.h"
#include "rts_pattern.h"
#include "rts_waveform.h"
#include "rts_noise.h"
#include "rts_image.h"            // the arithmetic of a backprojected pixel and the host-only plan of its launch
#include "rts_cube_source.h"      // what a received record brings to the cube: which counts, its delay, phase and amplitude, the cell and the add
#include "rts_stft.h"             // the radix-2 tree of the slow-time and fast-time transforms and the host-only plans of the Doppler map's and the spectrogram's launches
#include "rts_focus.h"            // autofocus: range alignment's reference, correlation and pick, the PGA's rotation, mask, products and update, the correction, their evaluators and the host-only plans of their launches
#include "rts_beat.h"             // the tree of the dechirped beat render, the range transform's evaluator and the host-only plans of their launches
#include "rts_beam.h"             // the beamformer's term, sum and streaming peak, its evaluator and the host-only plan of its launch
#include "rts_adapt.h"            // adaptive beamforming: the covariance's term and partition, the weight solve, their evaluators and the host-only plans of their launches
#include "rts_stap.h"             // space-time adaptive processing: the stacked snapshot, its covariance's and filter's evaluators, the host-only plan of the filter's launch
#include "rts_doa.h"              // direction finding: the eigensolver's and the angular scan's trees, the spectra's weights, the source count, their evaluators and the host-only plans of their launches
#include "rts_cfar_os.h"          // CFAR: what every detector shares (rts_cfar.h: window, training count, local maximum, refinement, record); OS: rank rule, alphas, the host evaluator
#include "rts_passive.h"          // passive radar: the lagged read, the Gram and cross sums' partition, the failed-block rule, the subtraction, the correlation's tree, the rules, the plans, the host evaluators
#include "rts_mimo.h"             // MIMO radar: the bank's term, its sum's order, the code multiply, the rule, the plan of the launch, the host evaluator
#include "rts_locate.h"           // multistatic localisation: the closed form of a triple, completion, refinement, cost, the resolution's order, the validation, the host evaluator
#include "rts_track.h"            // the tracker step: wrap, prediction, d2, the edge, the candidate order, update, coast, start, the validation, the host evaluator
#include "rts_tbd.h"              // track-before-detect: the shift table, the score, the window's first maximum, the candidate, the walk, the record, the validation, the host evaluators
#include "rts_source.h"           // clutter and jammer sources: pole, scale, draw, recursion, partials and tree, the validation, the host evaluator and the host-only plan of the launch
#include "rts_plot.h"             // plot extraction: key, unwrap, adjacency, neighbour intervals, the blocked sums, the record, the validation, the host evaluator
#include "rts_owned.h"            // DevBuf, PinBuf, StagedUpload: device and pinned host memory that frees itself
#include "rts_cube_state.h"       // RtsCubeProduct, RtsCubeState: the cube part of a handle, one record per family of entry points
#include "rts_launch_plan.h"      // RTS_BLOCK, RTS_WTILE, RTS_COOP_GROUP, RTS_STACK_OVF and the host arithmetic of a launch
#include "rts_post_plan.h"        // RTS_SMALL_CAP32 / 64, RTS_AGG_TILE and the host arithmetic of the post-processing
#include "rts_pulse_state.h"      // RtsPulseState: IDLE / OPEN / CHAINED, and the only code that moves the per-device count of open pulses
#include "rts_scene_host.h"       // RtsNode4, RtsBlasInfo, RtsMeshHost; the flattening of the caller's meshes, the host trees' concatenation, a mesh's bounds
#include "rts_tuning.h"           // RTS_STACK_LDS; RtsTuning, RtsSceneTuning: what the RTS_* environment switches fill, their table and its reader
static_assert(RtsTuning().img_split_below == RTS_IMAGE_SPLIT_BELOW, "the default of RTS_IMAGE_SPLIT_BELOW is rts_image.h's");

// ----------------------------------------------------------------------------- HBM layout
// (the BVH4 node of the static hierarchy, RtsNode4: rts_scene_host.h)

// Leaf record, 112 B (the bytes a lane at a node reads of its record: the same seven dwordx4 loads serve both), ONE PER
// PRIMITIVE and indexed by the global primitive id (the nodes' leaf children name primitives: k_children_to_prims, rts_scene.hip;
// only the ORDER in which k_leaves visits them follows the hierarchy's leaf slots, RtsScene::d_prim_order), refreshed every
// pulse: what the f64 intersection test needs of the triangle and
// what does not depend on the ray -- the first WORLD-space vertex, pre-gathered (the reference gathers through
// dbuf_triangles -> dbuf_triVertices per test, triangle_mesh.cu:147-154), and the test's ray-free terms e0 = p1 - p0,
// e1 = p0 - p2, n = e1 x e0 (triangle_mesh.cu:127-129), formed once per pulse by the placement kernel (k_leaves,
// rts_bvh.hip) with the helpers and in the order the test formed them per lane and per step: the same bits.  Plus the
// global primitive id and the target.
struct __attribute__((aligned(16))) RtsLeafTri {
    double p0x, p0y, p0z, e0x, e0y, e0z, e1x, e1y, e1z, nx, ny, nz;
    uint32_t prim;                  // global primitive id (targets concatenated in order)
    uint32_t targ;                  // target index
    uint32_t hz[2];                 // the primitive's horizon, side + and side -: four sector bytes each, byte k = S_k as k / 255 rounded up (rts_horizon.hip; 255: closed), copied by k_leaves from RtsScene::d_horizon
};
static_assert(sizeof(RtsLeafTri) == 112, "leaf size");
// The horizon's tolerances, relative to a mesh's extent E (the diagonal of its bounding box); the budget they belong to: DESIGN.md section 4
#define RTS_HZ_H0 9.5367431640625e-07        // 2^-20: heights up to h0 = RTS_HZ_H0 E count as "not above the plane"
#define RTS_HZ_RHO 0.00390625                 // 2^-8: the horizon holds for every origin within rho = RTS_HZ_RHO E of the triangle
#define RTS_HZ_DEGEN 9.5367431640625e-07      // 2^-20: a triangle whose smallest altitude is below RTS_HZ_DEGEN E switches its mesh's horizon off
#define RTS_HZ_EPS_AZ 0.015625                  // eps_az = 2^-6 rad: every azimuth sector's bound holds this far beyond the quadrant's two edges (rts_horizon.hip)
#define RTS_HZ_DECODE(b) ((double)(b) * (1.0 / 255.0))      // a sector byte's value; the build rounds up against this very expression
#define RTS_HZ_MARGIN 0.00390625f             // m_S = 2^-8: what the sine of a bounce ray's elevation must exceed S by (a placement may be off a rotation by 1e-3, rts_api.hip)
struct RtsHorizonMesh { double extent, h0, rho; };      // per mesh; rho = 0: its horizon is off
// the walk step decodes the record from the fetch's seven dwordx4 registers (rts_walk_step, rts_trace.hip): q0 = (p0x, p0y), q1 = (p0z, e0x),
// q2 = (e0y, e0z), q3 = (e1x, e1y), q4 = (e1z, nx), q5 = (ny, nz), q6 = (prim, targ, sectors of side +, of side -)
static_assert(offsetof(RtsLeafTri, p0x) == 0 && offsetof(RtsLeafTri, p0z) == 16 && offsetof(RtsLeafTri, e0y) == 32 && offsetof(RtsLeafTri, e1x) == 48 &&
              offsetof(RtsLeafTri, e1z) == 64 && offsetof(RtsLeafTri, ny) == 80 && offsetof(RtsLeafTri, prim) == 96 && offsetof(RtsLeafTri, targ) == 100,
              "leaf record offsets of the walk step's decode");

struct RtsTargetDev {               // per target, per pulse
    double reflCoeff;               // d_targReflCoeff
    double refrIndex;               // d_targRefrIndex
    double vx, vy, vz;              // dbuf_targ_vel[targ]
    uint32_t tri_base;              // first global primitive id
    uint32_t perface_normals;       // triangle_mesh.cu:178 (normals.size() > vertices.size())
    // placement of the target's static hierarchy for this pulse: local = rinv * (world - pos)
    double rinv[9];                 // inverse of the pulse's rotation (identity when the target does not rotate)
    double px, py, pz;
    double cx, cy, cz, r2;          // bounding sphere of the placed target (world space, radius^2, padded)
    float hz_h0, hz_rho;            // the horizon's tolerances for this target [m] (RtsHorizonMesh; hz_rho = 0: no bounce ray skips this target's walk)
    float ew;                       // extra origin slack of the target-space slab test [m]: covers the rounding of the world
                                    // vertices, of the exact test and of the world -> target mapping (~1e-12 of the world scale)
    int32_t root;                   // root node of the target's hierarchy, < 0: no (finite) geometry
};

struct RtsRxDev { double cx, cy, cz, radius, minTheta, maxTheta, minPhi, maxPhi; };

// End-of-ray record written by the trace kernel (received rays; every ray in KEEP_ALL mode).
struct __attribute__((aligned(16))) RtsEndRecord {
    double rayLength, power, doppler;
    double prevx, prevy, prevz;
    double firstx, firsty, firstz;
    uint64_t path_lo, path_hi;      // (targ + 1) per depth, 8 bits each, depth 0 in the low byte
    uint32_t slot;                  // local launch index (ray_first + slot = global index)
    int32_t received;
    uint32_t reflDepth;
    uint32_t pad;
};
static_assert(sizeof(RtsEndRecord) == 112, "end record size");
static_assert(sizeof(RtsDetection) == 72 && sizeof(RtsCfarParams) == 72 && sizeof(RtsCfarOsParams) == 72, "CFAR ABI sizes (rts_amd/_lib.py mirrors them)");
static_assert(sizeof(RtsPlot) == 104 && sizeof(RtsPlotParams) == 56, "plot ABI sizes (rts_amd/_lib.py mirrors them)");
static_assert(sizeof(RtsTrack) == 88 && sizeof(RtsTrackParams) == 96, "track ABI sizes (rts_amd/_lib.py mirrors them)");
static_assert(sizeof(RtsCancelParams) == 56 && sizeof(RtsXcorrParams) == 40, "passive ABI sizes (rts_amd/_lib.py mirrors them)");
static_assert(sizeof(RtsBankParams) == 48, "bank ABI size (rts_amd/_lib.py mirrors it)");
static_assert(sizeof(RtsTarget) == 144 && sizeof(RtsLocateParams) == 192, "locate ABI sizes (rts_amd/_lib.py mirrors them)");
static_assert(sizeof(RtsTbdParams) == 72 && sizeof(RtsTbdExtractParams) == 40 && sizeof(RtsTbdTrack) == 48, "track-before-detect ABI sizes (rts_amd/_lib.py mirrors them)");
static_assert(sizeof(RtsSourceParams) == 72, "source ABI size (rts_amd/_lib.py mirrors it)");
// RtsEndRecord::pad : bits 0-1 chain (output row = chain * n + slot), 2-3 refrDepth, 8-15 (target + 1) of chain 0's
// refraction (path prefill of rows >= 3), 16-17 children spawned

// State of a refracted child ray parked between chains (normal_shader.cu:191-256: the copy prd_refr).
struct __attribute__((aligned(16))) RtsChildState {
    double prevx, prevy, prevz, firstx, firsty, firstz;
    double rayLength, power, doppler, refx, refy;
    float dx, dy, dz;               // new_direction of refract(), exactly
    uint32_t refrDepth, refr_code, end, pad0, pad1;
};
static_assert(sizeof(RtsChildState) == 128, "child state size");

#ifndef RTS_TILE_CTRS
#define RTS_TILE_CTRS 64           // striped draw counters of the tile queue
#endif
#define RTS_TILE_BUCKETS 1024       // bins of the tiles' counting order (rts_post.hip: k_tile_bucket_*)
#define RTS_TILE_CTR_STRIDE 32     // ... one per 128-byte line: same-LINE atomics serialise in L2 (~10 ns each) whatever their address
// the cooperative kernel's per-XCD lists of head tiles (rts_trace.hip), each drawn through RTS_SEG_STRIPES counters of its own
#define RTS_XCD 8
#define RTS_SEG_STRIPES 8
#define RTS_TILE_CTRS_LAYOUT ((RTS_XCD + 1) * RTS_SEG_STRIPES + 8)       // counters reserved per kernel in the zero block (>= RTS_TILE_CTRS, >= RTS_XCD * RTS_SEG_STRIPES; 80: the layout's size since round 4, kept so that no offset behind it moves)
// the zero block: ONE fill per launch clears [draw counters of the ordinary kernel | of the cooperative kernel | head words: cost
// sum lo, hi, head count, pad | the launch's 24 u64 counters | the order's bins | the bins' reservation counters of the two-launch order build]
#define RTS_OFF_CTR_COOP (RTS_TILE_CTRS_LAYOUT * RTS_TILE_CTR_STRIDE)
#define RTS_OFF_HEAD (2 * RTS_TILE_CTRS_LAYOUT * RTS_TILE_CTR_STRIDE)
#define RTS_OFF_LIVE (RTS_OFF_HEAD + 4)       // 1 + the number of tiles at the front of this launch's order that cost more than a dead tile (0: unknown) -- written by the order build (rts_post.hip)
#define RTS_OFF_COUNTERS (RTS_OFF_HEAD + 8)
#define RTS_OFF_BINS (RTS_OFF_COUNTERS + 48)
#define RTS_OFF_TAKEN (RTS_OFF_BINS + RTS_TILE_BUCKETS)
#define RTS_ZERO_WORDS (RTS_OFF_TAKEN + RTS_TILE_BUCKETS)
#ifndef RTS_RX_LDS
#define RTS_RX_LDS 16               // receivers whose capture spheres the trace kernel keeps in LDS (the rest are read from memory)
#endif

// Launch constants of ray_generation (hoisted trig, ray_tracer.cu:155-203).  Device resident and
// read through a pointer: keeping these 30 doubles as by-value kernel arguments pinned ~60
// SGPRs for the whole kernel (SGPR spills to VGPR lanes).
// Primary-ray pre-filter and mask.  A primary ray that meets no triangle and no receiver sphere leaves NO trace in any output
// (not even with RTS_FLAG_KEEP_ALL_RAYS: its record is the initial payload, whatever its direction), and on C3 that is 84 % of
// the launch indices.  For those the exact f64 ray generation (two normalisations: a square root and three divisions each),
// the bounding-sphere tests, the target mapping, the root visits and the receiver quadratics buy nothing.  The trace kernel
// therefore first forms the direction in f32 (good to ~2e-6 rad) and asks two CONSERVATIVE questions -- is any triangle's
// projection near this direction (the mask below), can the ray come within a widened radius of a receiver sphere -- and only
// a ray that may hit something gets the exact treatment (everything a ray can be observed through is still computed exactly
// as before: the pre-filter can only say "certainly nothing").
// The mask: all primary rays of a launch start at the transmitter, so which of them CAN meet a triangle is a question
// about their direction alone.  Per pulse every placed triangle marks the cells of a 2-D bitmap over the beam -- perspective
// coordinates (p.u / p.b, p.v / p.b) of p = vertex - origin in a frame (b, u, v) around the boresight -- that the bounding
// rectangle of its projection touches (k_primary_mask, rts_bvh.hip); a primary ray whose own cell is clear skips the targets
// altogether (bounding spheres, target mapping, slab set-up, root visits: about half the instructions of a launch index that
// hits nothing -- 84 % of them on C3).  Conservative: a ray that hits a triangle has its direction inside the triangle's
// projection, hence inside the rectangle; the rectangle is widened by a cell, the ray's f32 coordinates are good to 1e-6 of the
// extent.  Disabled for the pulse (n = 0 / flag set) when a vertex is not in front of the transmitter, when a single triangle
// would cover more than RTS_MASK_MAX_CELLS cells, for W = 1 and for beams wider than ~120 degrees.  Cells are never finer than
// RTS_MASK_MIN_CELL (tangent units = radians): the f32 direction of the pre-filter must stay inside the one-cell margin.
#define RTS_MASK_MIN_CELL 1.0e-5
#define RTS_MASK_N 1024u
#define RTS_MASK_WORDS (RTS_MASK_N * RTS_MASK_N / 32u + 1u)      // the mask lives behind the handle's zero block (RTS_ZERO_WORDS): ONE fill per pulse clears both
#define RTS_MASK_MAX_CELLS 4096
struct RtsMaskFrame { float bx, by, bz, ux, uy, uz, vx, vy, vz; float u0, v0, inv_du, inv_dv; uint32_t n, pad0, pad1; };

struct RtsLaunchConsts {
    double ox, oy, oz;              // d_rayOrigin
    double bsx, bsy, bsz;           // beamStart
    double stx, sty, stz;           // lattice step per launch index
    double rot[9];                  // Rot  (azimuth)
    double rot1[9];                 // Rot1 (elevation about the rotated y axis)
    double w1x, w1y, w1z;           // direction for W == 1
    uint64_t ray_first;
    uint32_t W, pad;
    uint32_t w_magic, w_more;       // division by W (>= 2) without a divide: q = mulhi(magic, g); ((g - q) >> 1) + q >> more  (rts_launch_plan.h: rts_div_magic)
    uint32_t il_tile, il_parts, il_part, pad2;     // interleaved tiles (il_parts <= 1: contiguous)
    const uint32_t* il_list;        // != nullptr: local tile j of il_tile launch indices is tile il_list[j] of the range (rts_set_tile_list: tiles DEALT to this launch, ascending) instead of j * il_parts + il_part
    RtsMaskFrame mask;              // primary-ray mask frame (n = 0: no mask this launch)
    // f32 constants of the primary-ray PRE-FILTER (rts_trace.hip): beamStart, lattice step, and Rot1 * Rot in ONE matrix -- the two
    // normalisations between them (ray_tracer.cu:170, 182) only scale, so the direction is Rot1 Rot (bs + st l) up to its length
    float f_bs[3], f_st[3], f_m[9], f_pad;
};
static_assert(sizeof(RtsLaunchConsts) % 8 == 0, "launch constants are copied to LDS dword by dword");

struct RtsTraceArgs {
    const RtsLaunchConsts* lc;      // device copy of the launch constants
    uint64_t ray_first;
    uint32_t n_rays, W;
    uint32_t max_refl, smooth;
    uint32_t n_prims, n_targets, n_rx, keep_all;
    uint32_t max_refr, rows;        // 0 or 2; output rows per launch index (1 or max_refl + 3)
    RtsChildState* child;           // [2][grid threads] (refraction only)
    // scene
    const RtsNode4* nodes4;
    const RtsNode4* nodes4v;        // != null: the eight OCTANT VERSIONS of every node record, [node][octant] (k_node_versions, rts_scene.hip): the ordinary kernel walks these
    const RtsLeafTri* leaves;
    const uint32_t* tri_nidx;       // [n_prims][3] indices into normals
    const double* normals;          // world-space normals [.][3]
    const RtsTargetDev* targets;
    const RtsRxDev* rx;
    // outputs
    RtsEndRecord* recv_records;     // appended (unordered), capacity n_rays
    RtsEndRecord* all_records;      // [n_rays] (keep_all)
    unsigned long long* counters;   // [0] recv count (append atomic) [1] segments [2] shaded [3] node visits [4] tri tests [5] spills [6] hard overflow
    unsigned long long* block_counters;   // [grid][8] per-block partial sums of counters 1..6 (k_sum_counters)
    float* dir_hist;                // [max_refl][3][n_rays] reflected directions (f32)
    int32_t* hit_prim;              // [n_rays][max_refl+1] (keep_all)
    float* hit_t;                   // [n_rays][max_refl+1] (keep_all)
    int32_t* stack_ovf;             // [RTS_STACK_OVF][grid threads]
    uint32_t total_threads;         // threads of the ordinary kernel's grid
    uint32_t slab_threads;          // row length of the per-thread slabs (stack_ovf, child): total_threads + the cooperative kernel's threads
    const uint32_t* tile_order;     // [wave tiles] tile ids in descending order of the cost last seen by the handle (null: identity)
    uint32_t* tile_cost;            // [wave tiles] out: duration of the tile (units of 8/3 ticks of the 100 MHz counter = 64 shader clocks at 2.4 GHz, + 1)
    uint32_t* tile_ctr;             // the zero block: draw counters (element s * RTS_TILE_CTR_STRIDE; the cooperative kernel's at RTS_OFF_CTR_COOP), zero at launch
    uint32_t coop_spread;           // 1, 2, 4 or 8: XCD lists a head tile's 64 cooperative units are dealt to (rts_trace.hip)
    const uint32_t* tile_head;      // [1] number of tiles at the head of tile_order that are traced as 64 cooperative units (null: none)
    const uint32_t* tile_head_all;  // the same word whether or not this launch has a cooperative kernel (read back with the counters)
    const uint32_t* tile_live;      // != null: [1 + tiles at the front of tile_order that cost more than a dead tile last time] (0: unknown); the order behind them is drawn 64 tiles at a time, one LANE per tile (k_trace: dead-tile batches)
    uint32_t rx_window_screen;      // 1: the pre-filter also asks whether a crossing of a capture sphere can lie in the receiver's angular window (RTS_RX_WINDOW_SCREEN=0: only whether the sphere is reached)
    uint32_t coop_versions;         // 1: the cooperative kernel walks the octant versions too (product and counting builds of the plain chain; RTS_COOP_VERSIONS=0: the plain records and the sorted children)
    uint32_t batch_dead;            // 0: never batch; 1: batch the order's dead region (needs tile_live); 2: every position goes through the tile-level test first (RTS_DEAD_BATCH=all: tests)
    uint32_t coop_walk_steps_lo;    // ... bit 30 of the record: >= this many (LONGISH WALKS; the head rule asks more of such a tile's cost, rts_post.hip)
    uint32_t coop_min_cost, coop_walk_steps;   // a tile is flagged LONG WALKS (bit 31 of its cost record) if it took >= coop_min_cost units and >= coop_walk_steps walk iterations per bounce round
    unsigned long long* timeline;   // debug (RTS_TIMELINE, counting build): [grid][2] block start/end ticks, then [tiles] tile durations (100 MHz)
    uint32_t pre_filter;            // 1: primary rays go through the f32 pre-filter (needs the mask when there is geometry)
    const uint32_t* pmask;          // primary-ray mask: RTS_MASK_N^2 bits, then one word != 0 if the mask is void for this pulse (null: none)
    uint32_t stack_lds;             // LDS stack entries in use (RTS_STACK_LDS; smaller only to exercise the spill path in tests)
    uint32_t horizon;               // 2: a bounce ray that leaves its triangle above the triangle's horizon skips the walk of the target it left; 1: by the isotropic rule only (RTS_FLAG_NO_HORIZON_SECTORS); 0: never (RTS_FLAG_NO_HORIZON)
};

// ----------------------------------------------------------------------------- host context
// Pinned host staging (hipHostMalloc): every small per-pulse upload/readback goes through it, so the
// stream never has to be drained just to recycle a pageable temporary.
#define RTS_PIN_GROUPS 4096
static inline uint32_t rts_agg_spec(uint32_t R) { return R < RTS_PIN_GROUPS ? R : RTS_PIN_GROUPS; }      // groups of the table of R rays that come home in the pinned block (the rest on demand: rts_aggregate_fetch)
struct RtsPinned {
    // [lc | motion | td]: the per-pulse parameters, uploaded with ONE copy into RtsContext::d_params (same layout): the launch
    // constants alone when no target moved, else up to the last target's placement
    RtsLaunchConsts lc;
    RtsTargetMotion motion[256];
    RtsTargetDev td[256];
    unsigned long long cnt[24];
    uint32_t G, pad;
    double rcs[256];
    double gsum[5 * RTS_PIN_GROUPS]; uint64_t gkey[RTS_PIN_GROUPS]; uint64_t grow[RTS_PIN_GROUPS]; uint32_t gmin[RTS_PIN_GROUPS];
};

// Handles joined by rts_link_handles share one trace stream: their trace kernels execute one after the other, in the
// order the pulses were begun; the rest of each pulse (scene placement before, ordering / finalise /
// aggregation after) runs on the handle's own (high-priority) stream and overlaps with the other handles' trace kernels.
struct RtsGate { hipStream_t tstream = nullptr; std::atomic<int> refs{0}; int device = 0; };      // (handles may be driven from different threads)

// The immutable part of a scene -- meshes in their own frames, the static target-space hierarchy and its leaf order -- lives
// ONCE per device and is shared (reference counted) by every handle that was given it with rts_share_scene: handles that keep
// several pulses in flight place, trace and post-process into their own per-pulse buffers but read the same nodes.
struct RtsScene {
    std::atomic<int> refs{1}; int device = 0;
    std::vector<RtsMeshHost> meshes;
    uint32_t n_prims = 0, n_verts = 0, n_normals = 0;
    DevBuf<uint32_t> d_tri_vidx, d_tri_nidx, d_vert_targ, d_norm_targ, d_prim_targ;
    DevBuf<double> d_verts_local, d_normals_local;
    std::vector<RtsBlasInfo> blas; uint32_t n_nodes = 0, n_leaves = 0;
    DevBuf<RtsNode4> d_nodes4; DevBuf<uint32_t> d_leaf_prim;
    DevBuf<uint32_t> d_prim_order;  // [n_prims] the primitives by first appearance in d_leaf_prim (rts_prim_order.h): thread i of k_leaves handles primitive d_prim_order[i]
    DevBuf<RtsNode4> d_nodes4v;     // [n_nodes][8] octant versions of d_nodes4 (empty: none -- RTS_NODE_VERSIONS=0, or the scene too large for them)
    DevBuf<uint32_t> d_horizon;     // [n_prims][2] the primitives' horizon, side + and side - (four sector bytes each), by global primitive id (rts_horizon.hip); k_leaves copies it into the leaf records
    std::vector<RtsHorizonMesh> hz; // per mesh: extent and the horizon's tolerances
    double build_ms = 0; uint32_t builder = 0;     // how long the hierarchy build took, and where it ran (0 host SAH, 1 device LBVH)
    size_t device_bytes() const {
        return d_tri_vidx.cap * 4 + d_tri_nidx.cap * 4 + d_vert_targ.cap * 4 + d_norm_targ.cap * 4 + d_prim_targ.cap * 4 + d_verts_local.cap * 8 +
               d_normals_local.cap * 8 + (d_nodes4.cap + d_nodes4v.cap) * sizeof(RtsNode4) + d_leaf_prim.cap * 4 + d_prim_order.cap * 4 + d_horizon.cap * 4;
    }
};

// The tile-cost HISTORY (what every wave tile of the W^3 lattice cost the launch that traced it last: the cost order, the cooperative kernel's
// head and the dead part of the order are built from it, rts_post.hip) belongs to the handles that SHARE A SCENE on a device (round 5): they trace
// consecutive pulses of one interval, so what one of them measured is the best estimate the others have -- three handles in flight learn three times
// as fast, a handle's first launch finds the schedule its neighbours built, and a 20-pulse run is no longer mostly schedules settling.  Entries are
// single words replaced whole: a neighbour's merge racing with this handle's order build reads an old record or a new one, both valid estimates.
// (RTS_SHARE_HISTORY=0: every handle its own.)
struct RtsTileHist { std::atomic<int> refs{1}; DevBuf<uint32_t> d; uint32_t n = 0; bool any = false; uint32_t head_hint = 0; bool head_hint_valid = false; };

struct RtsSpecParams { std::vector<double> rcs; double wl = 0, gt = 0, gr = 0, carrier = 0, cspeed = 0; int32_t cube_pulse = -1; uint64_t base = 0;
                       int mode = 0;        // 0: the uniform chain (rts_trace_pulse_end_uniform); 1: order + expand + the received set to the host mirror (rts_received_prefetch)
                       int fin = 0;         // mode 0's finaliser: 0 uniform (rcs / gt / gr), 1 the handle's tabulated patterns (rts_trace_pulse_end_patterns) with:
                       std::vector<double> pat_rx; double pat_org[3] = {0, 0, 0}, pat_dir[2] = {0, 0};      // [n_rx][8] position, az, el, az_rate, el_rate, 0; the pulse's ray_origin and tx_dir
};
// Arguments of the pattern finaliser (rts_post.hip: finalise_row_patterns): the handle's packed tables -- views [tx | rx[n_rx] | rcs[n_targets]]
// followed by their arrays -- and the pulse's receiver rows, uploaded per pulse (rts_pattern_pulse_upload)
struct RtsPatArgs { const RtsPatView* pats; const double* rx; uint32_t n_rx, n_targets; double ox, oy, oz, tx_az, tx_el, wl, carrier, cspeed; };
// Host mirror of a pulse's received set and of its aggregation outputs (rts_received_prefetch, the C++ adapter's path): ONE pinned
// allocation that KERNELS write (k_mirror_rows, k_mirror_agg: only the rows that exist cross the bus, no copy calls) and read
// (k_set_values: the power / Doppler the simulator's callbacks produced).  cap rows of: PerRayData | path row | RCS-angle row | slot |
// aggregated power, doppler, delay, phase, pathMatch | values in: power, doppler.
struct RtsHostMirror {
    PinBuf<char> buf; uint32_t cap = 0, D = 0;       // buf.p / buf.dev: the block as the host / the kernels address it; cap: rows
    size_t o_rays = 0, o_paths = 0, o_angles = 0, o_slots = 0, o_apower = 0, o_adoppler = 0, o_adelay = 0, o_aphase = 0, o_apm = 0, o_vpower = 0, o_vdoppler = 0;
    bool recv_valid = false, agg_valid = false;      // the mirror holds the last pulse's received set / aggregation outputs (once the stream has drained)
    bool want = false;                               // this pulse's post-processing feeds the mirror (set by rts_received_prefetch, cleared by the next rts_trace_pulse_begin)
};
// rts_aggregate enqueues; the table is read (stream wait + pinned block -> RtsGroup records) by the first call that needs it
struct RtsAggPending { bool valid = false, rows = false; uint32_t R = 0, D = 0, spec = 0; RtsKeyPlan key = {}; uint64_t base = 0; double* gsum = nullptr; };

// What a pulse leaves for its accessors (rts_results_api.hip; the finalisers, the aggregation and the end-of-pulse chains of rts_api.hip; the
// launchers of rts_post.hip / rts_render.hip read n_recv / recv_dev).  The device buffers the results live in stay on the handle.
struct RtsPulseResults {
    uint64_t n_recv = 0;                // received rays (ordered, expanded: RtsContext::d_rx_*)
    const unsigned long long* recv_dev = nullptr;      // != nullptr while a chain is being enqueued on the device-side count: its kernels take the received count from here
    std::vector<RtsGroup> groups; bool agg_valid = false; uint64_t recv_index_base = 0;
    RtsAggPending agg_pending;          // the group table of the last rts_aggregate is still on its way (rts_aggregate_fetch reads it)
    bool agg_delay_in = true;           // rts_aggregate_device: the delay / phase arrays carry initial sums (rs::kernel_wrapper's in-out arguments); false: they start at zero
    int64_t agg_base_local = 0;         // pathMatch value of received ray i after rts_aggregate = agg_base_local + i
    RtsHostMirror mirror;               // rts_received_prefetch / rts_received_view / rts_finalise_values / rts_aggregated_view
    std::vector<PerRayData> v_rays; std::vector<int32_t> v_paths; std::vector<double> v_angles, v_apower, v_adoppler, v_adelay, v_aphase; std::vector<uint64_t> v_slots; std::vector<int32_t> v_apm;      // the views' fallback storage (sets beyond the mirror's capacity)
    std::vector<PerRayData> v_agg_rays; unsigned v_recv_have = 0;      // rts_aggregated_view's own scratch (never the received view's storage); bits: which of v_rays / v_paths / v_angles / v_slots hold THIS pulse's set already
    bool agg_timed = false, fin_timed = false;      // ev[6] / ev[7] bracket this pulse's finalisation / aggregation (rts_get_stats)
    // the previous results are gone: a new pulse begins (rts_trace_pulse_begin), or rts_kernel_wrapper_on overwrites the received set
    void forget() { agg_valid = false; agg_pending.valid = false; n_recv = 0; mirror.want = false; mirror.recv_valid = false; mirror.agg_valid = false; v_recv_have = 0; }
};
// What every kernel that takes recv_dev does first (R: the host's bound on the received count, which becomes the count).  Speculative
// post-processing: the count is the trace kernel's, on the device.  More than the caller's capacity: nothing is to be done, and
// `beyond` says how the kernel does nothing -- return, or what its barriers need.  A macro and not an inline function that returns
// a flag: the compiler folds such a flag into the bounds test that follows, and the kernels behind the trace keep their
// instructions (profiles/cube_source_refactor.txt).
#define RTS_DEV_COUNT(R_dev, R, beyond) do { if (R_dev) { const unsigned long long v_ = *(R_dev); if (v_ > (unsigned long long)(R)) { beyond; } else (R) = (uint32_t)v_; } } while (0)

struct RtsContext {
    RtsParams params;
    RtsTuning tune;                 // what the handle's RTS_* switches said at rts_create (rts_tuning.h); everything below is resources and state
    uint32_t depth = 0;             // D = max_refr + max_refl
    int device = 0;
    hipStream_t stream = nullptr;       // scene placement, ordering, finalise, aggregation (high priority: short kernels)
    hipStream_t tstream = nullptr;      // trace kernels (the link group's, see RtsGate)
    hipStream_t cstream = nullptr; hipEvent_t ev_coop[2] = {nullptr, nullptr};      // the cooperative trace kernel of a launch runs beside the ordinary one; stream created on first use (rts_trace.hip)
    uint32_t n_head_hint = 0;           // head count of the handle's previous order build (came home with that launch's counters)
    uint32_t last_coop_grid = 0;        // blocks of the cooperative kernel in the handle's last launch (0: none was launched)
    hipEvent_t ev[9] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
    // scene: the shared static part, and this handle's placement of it
    RtsScene* scene = nullptr;          // never null after rts_create
    DevBuf<double> d_verts_world, d_normals_world;
    std::vector<RtsTargetMotion> motion; bool motion_valid = false; bool bvh_valid = false;   // bvh_valid: scene placed for `motion`
    DevBuf<char> d_params;              // device image of RtsPinned's [lc | motion | td]
    RtsLaunchConsts* p_lc = nullptr; RtsTargetMotion* p_motion = nullptr; RtsTargetDev* p_targets = nullptr;     // ... and its parts
    // hierarchy: static nodes + leaf order (set_scene), leaf records refreshed per pulse
    DevBuf<RtsLeafTri> d_leaves; DevBuf<char> d_sort_tmp;
    // receivers
    DevBuf<RtsRxDev> d_rx; uint32_t n_rx = 0;
    // per pulse
    uint64_t ray_first = 0; uint32_t n_rays = 0;
    DevBuf<RtsEndRecord> d_recv, d_all; DevBuf<unsigned long long> d_block_counters, d_timeline; unsigned long long* p_counters = nullptr;      // (the 16 counters live behind the draw counters: one fill zeroes both)
    DevBuf<uint32_t> d_tile_cost, d_tile_key, d_tile_order, d_tile_ctr;
    RtsTileHist* hist = nullptr;        // never null after rts_create; shared with the handles of the same scene (rts_share_scene) unless tune.share_history is off
    double coop_big_now = 0.0;          // this launch's tune.coop_big: tune.coop_big_part when the launch is a part of a pulse on a GPU no other pulse shares
    bool tile_cost_pending = false; uint64_t tile_cost_sig[4] = {0, 0, 0, 0};   // this handle's last launch left cost records that are not merged into the history yet (rts_post.hip)
    // tiles DEALT to this handle (rts_set_tile_list: ray sharding balanced by last-seen cost instead of interleaved parts): ascending tile
    // numbers in units of il_list_tile launch indices; a pulse with interleave_parts == RTS_INTERLEAVE_LIST traces them
    DevBuf<uint32_t> d_il_list; uint32_t il_list_n = 0, il_list_tile = 0, il_list_gen = 0; uint32_t il_list_last = 0;
    uint64_t tile_last_sig[4] = {0, 0, 0, 0}; bool tile_last_valid = false; DevBuf<uint32_t> d_rec_tmp;      // shape of the last launch that recorded costs (rts_tile_records_get)
    DevBuf<float> d_dir_hist; DevBuf<uint32_t> d_pmask; bool pre_dense = false;
    DevBuf<int32_t> d_hit_prim; DevBuf<float> d_hit_t; DevBuf<int32_t> d_stack_ovf; DevBuf<RtsChildState> d_child;
    DevBuf<uint64_t> d_rk64, d_rk64_sorted;
    RtsTraceArgs last_args; RtsLaunchConsts last_lc;
    // received set (ordered, expanded; its count: res.n_recv)
    DevBuf<uint32_t> d_rk, d_rk_sorted, d_ri, d_ri_sorted;
    DevBuf<PerRayData> d_rx_rays; DevBuf<int32_t> d_rx_paths; DevBuf<double> d_rx_angles; DevBuf<uint64_t> d_rx_slots;
    DevBuf<PerRayData> d_all_rays; DevBuf<int32_t> d_all_paths; DevBuf<double> d_all_angles;
    // aggregation
    DevBuf<uint64_t> d_akeys, d_akeys_sorted; DevBuf<uint32_t> d_aidx, d_aidx_sorted; DevBuf<uint32_t> d_ghead, d_gid;
    DevBuf<double> d_gsum; DevBuf<uint32_t> d_gmin; DevBuf<uint64_t> d_gkey; DevBuf<uint32_t> d_gcount; DevBuf<uint64_t> d_grow; DevBuf<int32_t> d_gpath;
    DevBuf<double> d_delay, d_phase; DevBuf<int32_t> d_pathmatch; DevBuf<double> d_rcs;
    double tl_summary[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};      // tune.timeline_blocks: the last launch's percentiles (rts_get_block_timeline)
    uint32_t tl_blocks = 0;             // ... and the blocks whose start / end ticks this launch recorded
    bool order_sum_valid = false; DevBuf<unsigned long long> d_order_sum;      // the tile order in two launches when the previous launch had this launch's shape: d_order_sum holds that launch's cost sum (rts_post.hip: rts_tile_order_build)
    bool verts_world_valid = false;     // d_verts_world holds the current placement (the per-pulse scene update is one launch that writes the leaf records only: rts_scene_place)
    hipStream_t tstream_now = nullptr;  // the stream this pulse's trace kernel went to (rts_trace_pulse_begin; tune.trace_own_stream off: always the trace stream)
    uint32_t spec_cap = RTS_SMALL_CAP64;
    RtsSpecParams spec;                 // rts_trace_pulse_end_uniform: parameters of the chain, which may be enqueued on the device-side count (pulse.chained(); tune.spec_enabled off: never)
    uint64_t recv_hint = 0; bool recv_hint_valid = false;                    // received rays of the handle's previous pulse
    RtsPulseResults res;                // what the last pulse left for its accessors (rts_results_api.hip)
    PinBuf<RtsRxDev> pin_rx; std::vector<RtsRxDev> rx_host;      // receivers: last values set (an unchanged set is not uploaded again) and the pinned staging of the asynchronous upload
    RtsCubeState cube;                  // the complex return cube and what is derived from it, by family (rts_cube_state.h; the three rts_cube*_api.hip units)
    PinBuf<RtsPinned> pin;      // pinned host staging (one RtsPinned) and its address on the device (pin.dev): kernels write the small per-pulse read-backs (counters, group table) straight into it
    bool rcs_uploaded = false; DevBuf<double> d_rcsval; int n_cu = 0; bool stats_pending = false;
    RtsStats stats;
    // tabulated patterns (rts_set_patterns): one device buffer per handle, and the per-pulse receiver rows behind a staged upload
    DevBuf<char> d_pat; uint32_t pat_n_rx = 0, pat_n_targets = 0; bool pat_set = false;
    StagedUpload<double> pat_rx;
    double pulse_org[3] = {0, 0, 0}, pulse_dir[2] = {0, 0}; bool pulse_traced = false;      // the last traced pulse's ray_origin / tx_dir; false after rts_kernel_wrapper_on
    double lap_s[8] = {0, 0, 0, 0, 0, 0, 0, 0}; uint64_t lap_n[8] = {0, 0, 0, 0, 0, 0, 0, 0};      // RTS_LAP=1: host time per section of rts_trace_pulse_begin
    RtsGate* gate = nullptr;            // never null after rts_create
    RtsPulseState pulse;                // IDLE, OPEN (begun, the trace in flight) or CHAINED (its chain enqueued on the device-side count, awaiting rts_spec_resolve); counted on its device while not IDLE
    // Every raw handle above starts null and the destructor skips what is null: `delete c` is right for a handle that rts_create
    // left half built.  The body (rts_api.hip) drains the streams, drops the shared objects and destroys the events and streams; the
    // DevBuf / PinBuf / StagedUpload members free themselves after it.  The caller makes the handle's device current first.
    ~RtsContext();
};
// the (receiver, path) aggregation key of depth D among n_targets targets and n_rx receivers, and of the handle's own received sets
static inline RtsKeyPlan rts_key_plan_for(uint32_t D, uint32_t n_targets, uint32_t n_rx) { return rts_key_plan(D, (int64_t)n_targets - 1, (int64_t)(n_rx ? n_rx : 1u) - 1); }
static inline RtsKeyPlan rts_handle_key_plan(const RtsContext* c) { return rts_key_plan_for(c->depth, (uint32_t)c->scene->meshes.size(), c->n_rx); }
// the received set of the handle's pulse as a cube writer reads it (rts_cube_source.h; base: RtsPulseResults::agg_base_local)
static inline RtsCubeSource rts_cube_source(const RtsContext* c, bool paths, double cspeed, double carrier, int64_t base)
{
    RtsCubeSource s;
    s.rays = c->d_rx_rays.p; s.delay = c->d_delay.p; s.phase = c->d_phase.p; s.pm = c->d_pathmatch.p; s.base = base;
    s.R = (uint32_t)c->res.n_recv; s.paths = paths ? 1 : 0; s.cspeed = cspeed; s.carrier = carrier;
    return s;
}
void rts_scene_unref(RtsScene* s);          // drop one reference; the last one deletes the object (and with it its buffers)
void rts_hist_unref(RtsTileHist* h);
void rts_gate_unref(RtsGate* g);            // ... and destroys the group's trace stream

// implemented in the .hip units
int rts_sah_build(const double* verts, const uint32_t* tris, uint32_t n_tris, double split_budget, std::vector<RtsNode4>& nodes, std::vector<uint32_t>& leaf_prim, RtsBlasInfo& out);
int rts_lbvh_build_device(RtsContext* c, RtsScene* ns, const RtsSceneFlat& flat, const RtsSceneTuning& tune);
int rts_horizon_build(RtsContext* c, RtsScene* ns, const RtsSceneFlat& flat);      // rts_horizon.hip: ns->d_horizon, ns->hz (behind scene_finish)
int rts_scene_place(RtsContext* c, const RtsLaunchConsts& lc, bool place, uint32_t* pmask);      // placement kernels (place) + the primary-ray mask (lc.mask.n != 0)
int rts_tile_costs_flush(RtsContext* c);      // merge the cost records of the last launch into the history now (before its launch shape goes away)
int rts_tile_records_masked(RtsContext* c, uint32_t* d_out, uint32_t n);      // the history's records of the tiles the last launch traced, 0 elsewhere
int rts_tile_order_build(RtsContext* c, const uint64_t* prev_sig, bool prev_valid, const uint64_t* cur_sig, uint32_t n_tiles_cur, uint32_t resident_waves);
int rts_trace_launch(RtsContext* c, const RtsTraceArgs& a, bool count_traversal, unsigned coop_grid);
void rts_trace_preload();
int rts_post_order_and_expand(RtsContext* c);
int rts_mirror_reserve(RtsContext* c, uint32_t rows);
int rts_post_mirror_received(RtsContext* c);       // the ordered, expanded received set -> the host mirror (kernel stores, count from c->res.recv_dev when set)
int rts_post_mirror_aggregated(RtsContext* c);     // per-ray aggregation outputs -> the host mirror
int rts_post_set_values(RtsContext* c, const double* power, const double* doppler);      // power / Doppler of the received rays <- device-readable arrays (the mirror's values-in area)
int rts_post_expand_all(RtsContext* c);
int rts_post_all_small(RtsContext* c, uint32_t cap, const RtsSpecParams& sp, bool want_groups);      // the whole uniform post-processing of a small received set in ONE one-block kernel (count from the device)
int rts_cube_accumulate_device(RtsContext* c, uint32_t pulse_index, double cspeed, double carrier);      // rts_render.hip: the writers of the cube, range compression
int rts_cube_accumulate_paths_device(RtsContext* c, uint32_t pulse_index, int64_t base);
int rts_cube_render_device(RtsContext* c, uint32_t pulse_index, bool paths, bool doppler, double cspeed, double carrier, int64_t base);
int rts_cube_compress_device(RtsContext* c, uint32_t first_pulse, uint32_t n_pulses);
int rts_cube_noise_device(RtsContext* c, uint32_t first_pulse, uint32_t n_pulses, double sigma, uint64_t seed);          // rts_detect.hip
int rts_cube_detect_device(RtsContext* c, const RtsCfarParams& p, const double* map, uint32_t n_doppler, uint32_t max_det);
int rts_cube_detect_os_device(RtsContext* c, const RtsCfarOsParams& p, const double* alpha_tab, const double* map, uint32_t n_doppler, uint32_t max_det);      // alpha_tab: device, by training count (pfa), or null (p.alpha)
// rts_plot.hip.  list: n_cap records, of which the first min(n_cap, *n_dev) count (n_dev null: all n_cap)
int rts_cube_plots_device(RtsContext* c, const RtsPlotParams& p, const RtsDetection* list, const uint32_t* n_dev, uint32_t n_cap, uint32_t n_doppler, uint32_t max_plots);
// rts_track.hip.  list: pcap records, of which the first min(pcap, *n_dev) count (n_dev null: all); tcap: the table's size; T: the interval
int rts_cube_track_tables(RtsContext* c);      // the two tables and their meta records, zeroed on first use
int rts_cube_track_device(RtsContext* c, const RtsTrackParams& p, double T, const RtsPlot* list, const uint32_t* n_dev, uint32_t pcap, uint32_t tcap);
// rts_locate.hip.  geo: the call's constants on the device (null: candidates); list, n_dev, rcap: the source's records, their count on the device, their capacity
int rts_cube_locate_device(RtsContext* c, const RtsLocateParams& p, const RtsLocateGeo* geo, const void* list, const void* n_dev, uint32_t rcap, uint32_t max_c, uint32_t max_t);
// rts_tbd.hip.  Both on a validated call and a state whose buffers exist; the step writes merit map tbd_cur ^ 1 and ring slot `slot`
int rts_cube_tbd_step_device(RtsContext* c, const RtsTbdParams& p, const double* map, bool first, double T, double dt, uint32_t slot);
int rts_cube_tbd_extract_device(RtsContext* c, const RtsTbdExtractParams& e, uint32_t max_tracks);
int rts_cube_doppler_device(RtsContext* c, uint32_t n_fft, double* out);      // rts_stft.hip: the slow-time transforms
int rts_cube_stft_device(RtsContext* c, const RtsStftParams& p, const RtsStftPlan& plan, const double* window, double* out);
int rts_cube_align_device(RtsContext* c, const RtsAlignParams& p, const RtsAlignPlan& plan, double* out);      // rts_focus.hip: autofocus
int rts_cube_pga_device(RtsContext* c, const RtsPgaParams& p, const RtsPgaPlan& plan, double* out);      // out: phase [n_rx][N], then rms [n_rx][n_iters]
int rts_cube_correct_device(RtsContext* c, const RtsCorrectParams& p, const RtsCorrectPlan& plan, const double* shifts, const double* phase);      // the tables on the device, or null
int rts_cube_beat_device(RtsContext* c, uint32_t pulse_index, const RtsBeatParams& p, const RtsBeatPlan& plan, double cspeed, double carrier, int64_t base);      // rts_beat.hip
int rts_cube_range_device(RtsContext* c, const RtsRangeParams& p, const RtsRangePlan& plan, const double* window, double* out);
int rts_cube_sources_device(RtsContext* c, const RtsSrcPlan& plan, uint32_t K, bool has_profile, uint64_t seed, uint64_t live, const double* table);      // rts_source.hip
int rts_cube_beam_device(RtsContext* c, const RtsBeamParams& p, const RtsBeamPlan& plan, const double* in, uint64_t rx_stride, const double* weights, void* out);      // rts_beam.hip
int rts_cube_cov_device(RtsContext* c, const RtsCovSet& set, const RtsCovPlan& plan, uint32_t n_taps, const double* in, uint64_t rx_stride, double* part, double* out);      // rts_adapt.hip
int rts_cube_mvdr_device(RtsContext* c, const RtsMvdrPlan& plan, uint32_t n_rx, uint32_t n_beams, double loading, const double* cov, const double* steering, uint32_t* status, double* out);
// rts_passive.hip.  mask: the receivers cancelled (resolved); the state's buffers exist
int rts_cube_cancel_device(RtsContext* c, const RtsCancelParams& p, const RtsCancelPlan& plan, uint64_t mask);
int rts_cube_xcorr_device(RtsContext* c, const RtsXcorrParams& p, const RtsXcorrPlan& plan, double* out);
// rts_mimo.hip.  M: the waveforms' lengths; tab: the staged table on the device (plan.off, plan.code_off); code: it holds a code table
int rts_cube_bank_device(RtsContext* c, const RtsBankParams& p, const RtsBankPlan& plan, const uint32_t* M, const double* tab, bool code, double* out);
int rts_cube_st_apply_device(RtsContext* c, const RtsStApplyParams& p, const RtsStApplyPlan& plan, const double* in, uint64_t rx_stride, const double* weights, void* out);      // rts_stap.hip
int rts_cube_eig_device(RtsContext* c, const RtsEigPlan& plan, uint32_t n, const double* cov, uint32_t* status, double* values, double* vectors);      // rts_doa.hip
int rts_cube_doa_scan_device(RtsContext* c, const RtsDoaScanPlan& plan, uint32_t n, uint32_t m, uint64_t n_dirs, uint32_t flags, const double* steering, const double* vectors,
                             const double* g, double* out);
int rts_cube_backproject_device(RtsContext* c, const RtsImageParams& p, const RtsImagePlan& plan, const double* geo, double* out);      // rts_image.hip
int rts_post_finalise(RtsContext* c, const double* rcs_host, double wl, double gt, double gr, double carrier, double cspeed);
int rts_pattern_pulse_upload(RtsContext* c, const RtsSpecParams& q, RtsPatArgs* out);      // the pulse's receiver rows -> the device, on c->stream
int rts_post_finalise_patterns(RtsContext* c, const RtsSpecParams& q);                       // k_finalise_patterns on the received set (count from c->res.recv_dev when set)
hipError_t rts_stream_wait(RtsContext* c, hipStream_t st);
int rts_aggregate_fetch(RtsContext* c, std::vector<RtsGroup>* groups);      // second half of rts_aggregate_device when groups == &c->res.groups: no-op when nothing is pending
int rts_aggregate_device(RtsContext* c, int32_t max_path, int32_t max_rx, const int32_t* d_paths, uint64_t R, uint32_t D,
                         double cspeed, double carrier, uint64_t base, PerRayData* d_rays, double* d_delay,
                         double* d_phase, int32_t* d_pm, std::vector<RtsGroup>* groups, double* d_npath,
                         double* d_power_sum, double* d_doppler_sum, int32_t pm_init, const uint64_t* d_rows);
const char* rts_env(const char* name);      // the environment, for the readers of rts_tuning.h (rts_api.hip: the library looks at it nowhere else)
int check_key_width(uint32_t depth, uint32_t n_targets, uint32_t n_rx, const char* who);      // rts_api.hip: the aggregation key of a scene and a receiver set fits
int rts_attach_scene(RtsContext* c);        // rts_scene.hip: per-handle buffers sized by the scene the handle now points at
// RTS_DEBUG_SYNC=1: synchronise after every stage and name it on stderr, so that a device
// fault is attributed to the kernel that caused it
int rts_debug_stage(RtsContext* c, const char* name);
#define RTS_STAGE(c, name) do { int rc_ = rts_debug_stage((c), (name)); if (rc_ != RTS_OK) return rc_; } while (0)

#define RTS_HIP(call) do { hipError_t e_ = (call); if (e_ != hipSuccess) { \
    rts_set_error("%s failed: %s (%s:%d)", #call, hipGetErrorString(e_), __FILE__, __LINE__); return RTS_ERR_HIP; } } while (0)
// ... and the library's own status: what is not RTS_OK is the caller's return value (the callee has set the message)
#define RTS_TRY(expr) do { const int rc_ = (expr); if (rc_ != RTS_OK) return rc_; } while (0)

// every entry point that takes a handle (rts_api.hip, the three rts_cube*_api.hip units) makes its device current ...
#define CHECK_HANDLE(c) do { if (!(c)) { rts_set_error("null handle"); return RTS_ERR_INVALID; } RTS_HIP(hipSetDevice((c)->device)); } while (0)
// ... and those that consume a pulse's results, or replace what its enqueued work reads, settle the handle's pulse first: an OPEN one is
// ended (rts_trace_pulse_end), a CHAINED one resolved (rts_api.hip)
int rts_pulse_settle(RtsContext* c);
#define CHECK_CLOSED(c) do { int rc_ = rts_pulse_settle(c); if (rc_ != RTS_OK) return rc_; } while (0)

// What every finaliser of a received set does around its work: ev[6] / ev[7] bracket it for rts_get_stats, and the aggregation of the
// set as it was is no longer valid (the mirror keeps the set AS RECEIVED for the rest of the pulse: rts_received_view).
template <class Work> static inline int rts_finalise_bracket(RtsContext* c, Work work)
{
    RTS_HIP(hipEventRecord(c->ev[6], c->stream));
    RTS_TRY(work());
    RTS_HIP(hipEventRecord(c->ev[7], c->stream));
    c->res.fin_timed = true; c->stats_pending = true; c->res.agg_valid = false;
    return RTS_OK;
}
