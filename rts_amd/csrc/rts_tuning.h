// rts_tuning.h -- every RTS_* environment switch of the library: the records they fill, ONE table that says for each switch when
// it is read, by which rule and into which field, and one reader that walks the table.  No HIP, no handle, no allocation: it
// compiles with any host compiler and is tested without a GPU (tests/test_tuning_host.py).  What the switches were measured to do
// is in DESIGN.md ("The handle's tuning"); what an integrator needs of them in INTEGRATION.md ("Environment switches").
#pragma once
#include <math.h>
#include <stddef.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>
#include "../../include/rts_amd.h"      // RTS_BEAT_MAX_PARTS

#ifndef RTS_STACK_LDS
#define RTS_STACK_LDS 24            // traversal stack entries kept in LDS per lane
#endif

// ----------------------------------------------------------------------------- the records
// A handle's tuning: read ONCE PER HANDLE by rts_create (never per process: two handles of one process may differ) and never
// written again, but for RTS_FLAG_NO_PREFILTER, which clears use_pmask right after the read.  RtsContext::tune.
struct RtsTuning {
    // the trace launch
    bool use_pmask = true;              // the f32 pre-filter of primary rays and its mask
    int grid_mult = 4;                  // blocks of the trace kernel per compute unit
    int grid_spare = 160;               // block slots per 256 CUs a launch leaves free for the other open pulses of its device ...
    bool grid_spare_forced = false;     // ... and, once RTS_GRID_SPARE is set, of every launch
    bool tile_lpt = true;               // tiles are drawn in descending order of the cost last seen
    double ew_rel = 1.7763568394002505e-15;      // extra origin slack of the target-space slab test, relative to the world scale (2^-49)
    uint32_t stack_lds = RTS_STACK_LDS; // LDS stack entries in use
    bool rx_window_screen = true;       // the pre-filter also asks whether a crossing can lie in the receiver's angular window
    int batch_dead = 1;                 // dead-tile batches: 0 never, 1 the order's dead part, 2 every position is screened tile-wise first
    bool node_versions = true;          // the ordinary kernel walks the octant versions of the node records when the scene has them
    bool share_history = true;          // the tile-cost history is shared with the handles of the same scene (rts_share_scene)
    bool trace_own_stream = true;       // a lone handle's trace kernel goes to the handle's own stream
    bool spin_wait = true;              // the pulse's two host waits poll the stream instead of blocking (rts_stream_wait)
    // the cooperative kernel and the head of the tile order (rts_post.hip: RtsHeadRule)
    double coop_frac = 0.5;             // a tile costing more than this fraction of the launch's balanced time is traced as cooperative units (0: never)
    uint32_t coop_floor = 7500;         // ... and more than this many cost units (shader clocks >> 6; 7 500 = 0.2 ms of one wave)
    uint32_t coop_walk_steps = 1000;    // ... and whose bounce rounds took at least this many walk iterations each, on average: LONG WALKS (0: every tile above the floor)
    uint32_t coop_walk_steps_lo = 400;  // LONGISH WALKS: at least this many ...
    double coop_mid = 1.5;              // ... go to the head only if the tile cost more than this multiple of the balanced time (0: never)
    double coop_big = 0.0;              // ... or ANY tile costing more than this multiple of the balanced time, whatever its shape (0: off)
    double coop_big_part = 1.5;         // coop_big of a launch that is a PART of a pulse on a GPU no other pulse shares (0: off)
    uint32_t coop_spread = 1;           // XCD lists a head tile's 64 cooperative units are dealt to: 1, 2, 4 or 8
    uint32_t coop_grid_max = 1024;      // most blocks of the cooperative kernel
    bool coop_versions = true;          // the cooperative kernel walks the octant versions too
    // behind the trace
    bool post_small = true;             // received sets of up to 4096 rays are ordered / finished by single blocks
    uint64_t post_one_max = 1024;       // rts_trace_pulse_end_uniform is ONE kernel when the handle's previous pulse received at most this many rays
    uint32_t post_prio = 3;             // wave priority of k_post_all
    bool spec_enabled = true;           // rts_trace_pulse_end_uniform may enqueue its chain on the device-side received count
    // the cube
    uint32_t img_split_below = 1024;    // backprojection: workgroups below which the pulse chunks go on the grid (RTS_IMAGE_SPLIT_BELOW of rts_image.h)
    uint32_t beat_force_parts = 0;      // parts forced on the plan of a beat render (0: the plan's own)
    // debug
    bool timeline_blocks = false;       // product build: when every block started and ended (rts_get_block_timeline)
    bool debug_coop = false;            // one line per launch on stderr (grids, head hint, thresholds)
};

// Read once per rts_set_scene; device_build starts as the handle's flags say (RTS_FLAG_HOST_BUILD) before the read.
struct RtsSceneTuning {
    bool device_build = true;           // the hierarchy is built on the device (rts_lbvh.hip), else by the host builder (rts_sah.cpp)
    double split_budget = 2.0;          // extra references per triangle, on average, for triangles whose boxes are mostly empty
    bool build_fallback = true;         // a failed device build falls back to the host builder
    bool fail_device_build = false;     // tests: the device build is made to fail after it ran
    bool node_versions = true;          // the scene gets the octant versions of its node records (if they fit)
    bool version_key_centre = true;     // the versions order a node's children by their boxes' centres, else by their entry corners
    bool sah_tree = true;               // device builder: top-down binned SAH, else the Morton / Karras tree
    int crowd_rounds = 0;               // device builder: crowding rounds
    int ref_gain_rule = 1;              // device builder: a cut must pay (k_ref_count)
    bool debug_build = false;           // device builder: one line per crowding round on stderr
};

struct RtsProcessTuning {               // read once per process, at first use
    bool lap = false;                   // host time per section of rts_trace_pulse_begin, printed by rts_destroy
    bool debug_sync = false;            // synchronise after every stage and name it on stderr
};

struct RtsLaunchTuning {                // read per launch of a counting build
    const char* timeline = nullptr;     // file the launch's block and tile timeline is dumped to
};

// ----------------------------------------------------------------------------- the table
enum RtsSwitchScope { RTS_PER_HANDLE, RTS_PER_SCENE, RTS_PER_PROCESS, RTS_PER_LAUNCH };
// How a switch's text e becomes its field's value.  An unset switch leaves the field alone, whatever the kind.
enum RtsSwitchKind {
    RTS_SW_NOT_0,           // flag: e[0] != '0' ("", "yes": on; "00": off)
    RTS_SW_NONZERO,         // flag: atoi(e) != 0 ("", "yes": off; "00": off)
    RTS_SW_IS_1,            // flag: e[0] == '1'
    RTS_SW_PRESENT,         // flag: set at all, even to ""
    RTS_SW_NOT_WORD,        // flag: e is not `word`
    RTS_SW_INT_CLAMP,       // atoi(e) clamped to [lo, hi]
    RTS_SW_INT_INSIDE,      // atoi(e), kept only inside [lo, hi]
    RTS_SW_INT_ONE_OF,      // atoi(e), kept only if v is in 0 .. 31 and bit v of lo is set
    RTS_SW_REAL_FLOOR,      // atof(e), at least lo (not a number: lo)
    RTS_SW_REAL_INSIDE,     // atof(e), kept only if lo <= v <= hi
    RTS_SW_REAL_ABOVE,      // atof(e), kept only if v > lo
    RTS_SW_U64,             // strtoull(e, base 10)
    RTS_SW_PATH,            // e itself
    RTS_SW_DEAD_BATCH,      // "all": 2, else e[0] != '0'
    RTS_SW_GRID_SPARE,      // INT_CLAMP, and RtsTuning::grid_spare_forced is raised
    RTS_SW_ZERO_CLEARS      // an alias: atoi(e) == 0 writes 0 to the field of an earlier row, anything else changes nothing
};
enum RtsFieldType { RTS_F_BOOL, RTS_F_I32, RTS_F_U32, RTS_F_U64, RTS_F_F64, RTS_F_STR };
constexpr RtsFieldType rts_field_type(const bool*) { return RTS_F_BOOL; }
constexpr RtsFieldType rts_field_type(const int*) { return RTS_F_I32; }
constexpr RtsFieldType rts_field_type(const uint32_t*) { return RTS_F_U32; }
constexpr RtsFieldType rts_field_type(const uint64_t*) { return RTS_F_U64; }
constexpr RtsFieldType rts_field_type(const double*) { return RTS_F_F64; }
constexpr RtsFieldType rts_field_type(const char* const*) { return RTS_F_STR; }

struct RtsSwitch {
    const char* name; RtsSwitchScope scope; RtsSwitchKind kind; double lo, hi; const char* word;
    size_t field; RtsFieldType type;        // where in the scope's record, and what lives there
    const char* what;
};
#define RTS_FIELD(Record, member) offsetof(Record, member), rts_field_type((const decltype(Record::member)*)nullptr)
#define RTS_INT_MAX 2147483647.0

// One row per switch, in the order they are read.  The order matters once: RTS_COOP_SEG clears what RTS_COOP_STEPS set.
inline constexpr RtsSwitch RTS_SWITCHES[] = {
    {"RTS_PRIMARY_MASK", RTS_PER_HANDLE, RTS_SW_NOT_0, 0, 0, nullptr, RTS_FIELD(RtsTuning, use_pmask), "0: no pre-filter of primary rays (as RTS_FLAG_NO_PREFILTER); result-neutral, for A/B runs and tests"},
    {"RTS_GRID_MULT", RTS_PER_HANDLE, RTS_SW_INT_CLAMP, 1, RTS_INT_MAX, nullptr, RTS_FIELD(RtsTuning, grid_mult), "blocks of the trace kernel per compute unit"},
    {"RTS_GRID_SPARE", RTS_PER_HANDLE, RTS_SW_GRID_SPARE, 0, RTS_INT_MAX, nullptr, RTS_FIELD(RtsTuning, grid_spare), "block slots per 256 CUs a launch leaves free; set: every launch leaves them, not only one that shares its device"},
    {"RTS_TILE_LPT", RTS_PER_HANDLE, RTS_SW_NOT_0, 0, 0, nullptr, RTS_FIELD(RtsTuning, tile_lpt), "0: tiles in lattice order, no cost history, no cooperative kernel"},
    {"RTS_COOP_BIG_PART", RTS_PER_HANDLE, RTS_SW_REAL_INSIDE, 0, HUGE_VAL, nullptr, RTS_FIELD(RtsTuning, coop_big_part), "RTS_COOP_BIG of a launch that is a part of a pulse on an unshared GPU (0: off; DESIGN.md, the handle's tuning)"},
    {"RTS_COOP_FRAC", RTS_PER_HANDLE, RTS_SW_REAL_INSIDE, 0, HUGE_VAL, nullptr, RTS_FIELD(RtsTuning, coop_frac), "share of the balanced time above which a tile goes to the cooperative kernel (0: never; tests: 1e-12 puts every tile at the head)"},
    {"RTS_COOP_FLOOR", RTS_PER_HANDLE, RTS_SW_INT_CLAMP, 0, RTS_INT_MAX, nullptr, RTS_FIELD(RtsTuning, coop_floor), "cost units (64 shader clocks) below which no tile goes to the head"},
    {"RTS_DEBUG_COOP", RTS_PER_HANDLE, RTS_SW_PRESENT, 0, 0, nullptr, RTS_FIELD(RtsTuning, debug_coop), "one line per launch on stderr: grids, head hint, thresholds, clock anomalies"},
    {"RTS_SHARE_HISTORY", RTS_PER_HANDLE, RTS_SW_NOT_0, 0, 0, nullptr, RTS_FIELD(RtsTuning, share_history), "0: the handle keeps a tile-cost history of its own"},
    {"RTS_RX_WINDOW_SCREEN", RTS_PER_HANDLE, RTS_SW_NOT_0, 0, 0, nullptr, RTS_FIELD(RtsTuning, rx_window_screen), "0: the pre-filter only asks whether a capture sphere is reached (DESIGN.md §4, the receivers' window screen)"},
    {"RTS_TIMELINE_BLOCKS", RTS_PER_HANDLE, RTS_SW_NOT_0, 0, 0, nullptr, RTS_FIELD(RtsTuning, timeline_blocks), "product build: record when every block starts and ends (rts_get_block_timeline)"},
    {"RTS_COOP_VERSIONS", RTS_PER_HANDLE, RTS_SW_NOT_0, 0, 0, nullptr, RTS_FIELD(RtsTuning, coop_versions), "0: the cooperative kernel walks the plain node records"},
    {"RTS_DEAD_BATCH", RTS_PER_HANDLE, RTS_SW_DEAD_BATCH, 0, 0, "all", RTS_FIELD(RtsTuning, batch_dead), "dead-tile batches: 0 never, 1 the order's dead part, all: every position is screened tile-wise first (tests)"},
    {"RTS_WALK_VERSIONS", RTS_PER_HANDLE, RTS_SW_NOT_0, 0, 0, nullptr, RTS_FIELD(RtsTuning, node_versions), "0: the handle ignores the scene's octant versions (RTS_NODE_VERSIONS decides whether the scene has them)"},
    {"RTS_SPIN_WAIT", RTS_PER_HANDLE, RTS_SW_NONZERO, 0, 0, nullptr, RTS_FIELD(RtsTuning, spin_wait), "0: the pulse's two host waits block instead of polling"},
    {"RTS_TRACE_OWN_STREAM", RTS_PER_HANDLE, RTS_SW_NONZERO, 0, 0, nullptr, RTS_FIELD(RtsTuning, trace_own_stream), "0: the trace kernel always goes to the link group's trace stream"},
    {"RTS_SPECULATE", RTS_PER_HANDLE, RTS_SW_NONZERO, 0, 0, nullptr, RTS_FIELD(RtsTuning, spec_enabled), "0: rts_trace_pulse_end_uniform always waits for the received count"},
    {"RTS_POST_SMALL", RTS_PER_HANDLE, RTS_SW_NONZERO, 0, 0, nullptr, RTS_FIELD(RtsTuning, post_small), "0: the general post-processing chain for small received sets too"},
    {"RTS_POST_ONE_MAX", RTS_PER_HANDLE, RTS_SW_U64, 0, 0, nullptr, RTS_FIELD(RtsTuning, post_one_max), "most received rays (the handle's last count) for which the uniform pulse end is one kernel"},
    {"RTS_IMAGE_SPLIT_BELOW", RTS_PER_HANDLE, RTS_SW_INT_CLAMP, 0, 65536, nullptr, RTS_FIELD(RtsTuning, img_split_below), "backprojection: workgroups below which pulse chunks go on the grid (tests: 0 never, 65536 whenever there are two)"},
    {"RTS_BEAT_PARTS", RTS_PER_HANDLE, RTS_SW_INT_CLAMP, 0, RTS_BEAT_MAX_PARTS, nullptr, RTS_FIELD(RtsTuning, beat_force_parts), "tests: the parts of a beat render (0: the plan's own)"},
    {"RTS_POST_PRIO", RTS_PER_HANDLE, RTS_SW_INT_CLAMP, 0, 3, nullptr, RTS_FIELD(RtsTuning, post_prio), "wave priority of the one-kernel pulse end"},
    {"RTS_COOP_STEPS", RTS_PER_HANDLE, RTS_SW_INT_CLAMP, 0, RTS_INT_MAX, nullptr, RTS_FIELD(RtsTuning, coop_walk_steps), "walk iterations per bounce round that flag a tile LONG WALKS (0: every tile above the floor)"},
    {"RTS_COOP_STEPS_LO", RTS_PER_HANDLE, RTS_SW_INT_CLAMP, 0, RTS_INT_MAX, nullptr, RTS_FIELD(RtsTuning, coop_walk_steps_lo), "... that flag it LONGISH WALKS"},
    {"RTS_COOP_MID", RTS_PER_HANDLE, RTS_SW_REAL_FLOOR, 0, 0, nullptr, RTS_FIELD(RtsTuning, coop_mid), "multiple of the balanced time above which a longish tile goes to the head (0: never; DESIGN.md, the handle's tuning)"},
    {"RTS_COOP_SEG", RTS_PER_HANDLE, RTS_SW_ZERO_CLEARS, 0, 0, nullptr, RTS_FIELD(RtsTuning, coop_walk_steps), "the tests' old switch: 0 is RTS_COOP_STEPS=0, whatever RTS_COOP_STEPS says"},
    {"RTS_COOP_BIG", RTS_PER_HANDLE, RTS_SW_REAL_FLOOR, 0, 0, nullptr, RTS_FIELD(RtsTuning, coop_big), "multiple of the balanced time above which ANY tile goes to the head (0: off; DESIGN.md, the handle's tuning)"},
    {"RTS_COOP_SPREAD", RTS_PER_HANDLE, RTS_SW_INT_ONE_OF, (1 << 1) | (1 << 2) | (1 << 4) | (1 << 8), 0, nullptr, RTS_FIELD(RtsTuning, coop_spread), "XCD lists a head tile's cooperative units are dealt to: 1, 2, 4 or 8"},
    {"RTS_COOP_GRID", RTS_PER_HANDLE, RTS_SW_INT_CLAMP, 1, 4096, nullptr, RTS_FIELD(RtsTuning, coop_grid_max), "most blocks of the cooperative kernel"},
    {"RTS_EW_REL", RTS_PER_HANDLE, RTS_SW_REAL_ABOVE, 0, 0, nullptr, RTS_FIELD(RtsTuning, ew_rel), "origin slack of the slab test relative to the world scale (DESIGN.md §4, ew)"},
    {"RTS_STACK_LDS_DEBUG", RTS_PER_HANDLE, RTS_SW_INT_INSIDE, 1, RTS_STACK_LDS, nullptr, RTS_FIELD(RtsTuning, stack_lds), "tests: LDS stack entries in use, to force the spill path"},
    {"RTS_BUILDER", RTS_PER_SCENE, RTS_SW_NOT_WORD, 0, 0, "host", RTS_FIELD(RtsSceneTuning, device_build), "host: the host builder; anything else: the device builder, whatever RTS_FLAG_HOST_BUILD says"},
    {"RTS_SPLIT_BUDGET", RTS_PER_SCENE, RTS_SW_REAL_INSIDE, 0, 8, nullptr, RTS_FIELD(RtsSceneTuning, split_budget), "extra references per triangle where cutting pays (2 measured best for both builders)"},
    {"RTS_DEBUG_FAIL_DEVICE_BUILD", RTS_PER_SCENE, RTS_SW_PRESENT, 0, 0, nullptr, RTS_FIELD(RtsSceneTuning, fail_device_build), "tests: the device build fails after it ran"},
    {"RTS_DEVICE_BUILD_FALLBACK", RTS_PER_SCENE, RTS_SW_NOT_0, 0, 0, nullptr, RTS_FIELD(RtsSceneTuning, build_fallback), "0: a failed device build is an error instead of a host build"},
    {"RTS_NODE_VERSIONS", RTS_PER_SCENE, RTS_SW_NOT_0, 0, 0, nullptr, RTS_FIELD(RtsSceneTuning, node_versions), "0: the scene gets no octant versions of its node records"},
    {"RTS_VERSION_KEY", RTS_PER_SCENE, RTS_SW_NOT_WORD, 0, 0, "corner", RTS_FIELD(RtsSceneTuning, version_key_centre), "corner: the versions order children by entry corner, not by centre (profiles/r05a_versions_ab.log)"},
    {"RTS_DEVICE_TREE", RTS_PER_SCENE, RTS_SW_NOT_WORD, 0, 0, "lbvh", RTS_FIELD(RtsSceneTuning, sah_tree), "lbvh: the device builder's Morton / Karras tree instead of the binned SAH"},
    {"RTS_CROWD_ROUNDS", RTS_PER_SCENE, RTS_SW_INT_CLAMP, 0, 3, nullptr, RTS_FIELD(RtsSceneTuning, crowd_rounds), "device builder: crowding rounds (measured: no gain, twice the build time)"},
    {"RTS_REF_GAIN_RULE", RTS_PER_SCENE, RTS_SW_NONZERO, 0, 0, nullptr, RTS_FIELD(RtsSceneTuning, ref_gain_rule), "device builder, 0: a triangle is cut whether or not the cut pays"},
    {"RTS_DEBUG_BUILD", RTS_PER_SCENE, RTS_SW_PRESENT, 0, 0, nullptr, RTS_FIELD(RtsSceneTuning, debug_build), "device builder: one line per crowding round on stderr"},
    {"RTS_LAP", RTS_PER_PROCESS, RTS_SW_IS_1, 0, 0, nullptr, RTS_FIELD(RtsProcessTuning, lap), "1: host time per section of rts_trace_pulse_begin, printed by rts_destroy"},
    {"RTS_DEBUG_SYNC", RTS_PER_PROCESS, RTS_SW_IS_1, 0, 0, nullptr, RTS_FIELD(RtsProcessTuning, debug_sync), "1: synchronise after every stage and name it on stderr"},
    {"RTS_TIMELINE", RTS_PER_LAUNCH, RTS_SW_PATH, 0, 0, nullptr, RTS_FIELD(RtsLaunchTuning, timeline), "counting build: file the launch's block and tile timeline is dumped to"},
};
#define RTS_N_SWITCHES (sizeof(RTS_SWITCHES) / sizeof(RTS_SWITCHES[0]))
static_assert(RTS_N_SWITCHES == 44, "one row per switch");

// ----------------------------------------------------------------------------- the reader
typedef const char* (*RtsLookup)(const char* name);     // the environment (rts_api.hip: rts_env), or a test's map

inline void rts_tuning_store(void* record, const RtsSwitch& s, long long v)
{
    char* p = (char*)record + s.field;
    switch (s.type) {
    case RTS_F_BOOL: *(bool*)p = v != 0; break;
    case RTS_F_I32: *(int*)p = (int)v; break;
    case RTS_F_U32: *(uint32_t*)p = (uint32_t)v; break;
    default: break;
    }
}

// The switches of `scope` that `look` knows, applied in the table's order to that scope's record (which holds the defaults).
inline void rts_tuning_read(RtsSwitchScope scope, void* record, RtsLookup look)
{
    for (const RtsSwitch& s : RTS_SWITCHES) {
        if (s.scope != scope) continue;
        const char* e = look(s.name);
        if (!e) continue;
        char* p = (char*)record + s.field;
        switch (s.kind) {
        case RTS_SW_NOT_0: rts_tuning_store(record, s, e[0] != '0'); break;
        case RTS_SW_NONZERO: rts_tuning_store(record, s, atoi(e) != 0); break;
        case RTS_SW_IS_1: rts_tuning_store(record, s, e[0] == '1'); break;
        case RTS_SW_PRESENT: rts_tuning_store(record, s, 1); break;
        case RTS_SW_NOT_WORD: rts_tuning_store(record, s, strcmp(e, s.word) != 0); break;
        case RTS_SW_GRID_SPARE: ((RtsTuning*)record)->grid_spare_forced = true; [[fallthrough]];
        case RTS_SW_INT_CLAMP: { const int v = atoi(e); rts_tuning_store(record, s, v < s.lo ? (long long)s.lo : v > s.hi ? (long long)s.hi : v); break; }
        case RTS_SW_INT_INSIDE: { const int v = atoi(e); if (v >= s.lo && v <= s.hi) rts_tuning_store(record, s, v); break; }
        case RTS_SW_INT_ONE_OF: { const int v = atoi(e); if (v >= 0 && v < 32 && (((uint32_t)s.lo >> v) & 1u)) rts_tuning_store(record, s, v); break; }
        case RTS_SW_REAL_FLOOR: { const double v = atof(e); *(double*)p = s.lo < v ? v : s.lo; break; }
        case RTS_SW_REAL_INSIDE: { const double v = atof(e); if (v >= s.lo && v <= s.hi) *(double*)p = v; break; }
        case RTS_SW_REAL_ABOVE: { const double v = atof(e); if (v > s.lo) *(double*)p = v; break; }
        case RTS_SW_U64: *(uint64_t*)p = (uint64_t)strtoull(e, nullptr, 10); break;
        case RTS_SW_PATH: *(const char**)p = e; break;
        case RTS_SW_DEAD_BATCH: rts_tuning_store(record, s, strcmp(e, s.word) == 0 ? 2 : (e[0] != '0' ? 1 : 0)); break;
        case RTS_SW_ZERO_CLEARS: if (atoi(e) == 0) rts_tuning_store(record, s, 0); break;
        }
    }
}
inline void rts_tuning_read(RtsTuning* t, RtsLookup look) { rts_tuning_read(RTS_PER_HANDLE, t, look); }
inline void rts_tuning_read(RtsSceneTuning* t, RtsLookup look) { rts_tuning_read(RTS_PER_SCENE, t, look); }
inline void rts_tuning_read(RtsProcessTuning* t, RtsLookup look) { rts_tuning_read(RTS_PER_PROCESS, t, look); }
inline void rts_tuning_read(RtsLaunchTuning* t, RtsLookup look) { rts_tuning_read(RTS_PER_LAUNCH, t, look); }
