// rts_launch_plan.h -- the integer arithmetic of a pulse's launch, each formula written once: which launch indices a pulse
// traces, the division constants, the grids, the buffer sizes and the launch's shape.  No HIP, no handle, no allocation:
// plain structs returned by value, so it compiles with any host compiler and is tested without a GPU
// (tests/test_launch_plan_host.py).
#pragma once
#include <stdint.h>
#include <algorithm>

#ifndef RTS_BLOCK
#define RTS_BLOCK 256
#endif
#define RTS_WTILE 64               // work unit of the trace kernel: launch indices per wave tile
// lanes that share a ray in a unit of the cooperative kernel that walks the octant versions (rts_trace.hip: rts_walk_coop): 32 = two rays per wave (measured best: profiles/r05v_coop_group.log), 16 = four, 64 = one
#ifndef RTS_COOP_GROUP
#define RTS_COOP_GROUP 32
#endif
#define RTS_STACK_OVF 128           // further entries spilled to global memory (rare); a BVH4 node pushes up to 3 entries

inline uint64_t rts_wave_tiles(uint64_t n) { return (n + RTS_WTILE - 1) / RTS_WTILE; }      // wave tiles that hold n launch indices
inline uint64_t rts_lattice_size(uint32_t W) { return (uint64_t)W * W * W; }                // launch indices of a whole pulse
inline uint32_t rts_chains(uint32_t max_refr) { return max_refr ? 3u : 1u; }                // chains per launch index: the ray and, with refraction, its two children
inline uint32_t rts_hit_rows(uint32_t max_refl) { return max_refl + 1; }                    // hits recorded per launch index and chain (host side: the kernels index their planes with a.max_refl + 1 themselves)

// Launch indices of a range of `count` that fall into the tiles of interleaved part `part` of `parts` (tiles of `tile` indices,
// dealt round robin; parts <= 1: the whole range).
inline uint64_t rts_part_count(uint64_t count, uint32_t tile, uint32_t parts, uint32_t part)
{
    if (parts <= 1) return count;
    const uint64_t stride = (uint64_t)tile * parts, full = count / stride, rem = count % stride, lo = (uint64_t)part * tile;
    return full * tile + (rem > lo ? std::min<uint64_t>(rem - lo, tile) : 0);
}

// Branch-free division by W (libdivide's u32 scheme): g / W = (((g - t) >> 1) + t) >> more with t = mulhi(magic, g), exact for
// every 32-bit g (rts_raygen.h: rts_lattice_coords).  W < 2: {0, 0}, never used.
struct RtsDivMagic { uint32_t magic, more; };
inline RtsDivMagic rts_div_magic(uint32_t W)
{
    RtsDivMagic d = {0, 0};
    if (W < 2) return d;
    const uint32_t fl = 31u - (uint32_t)__builtin_clz(W);
    if ((W & (W - 1)) == 0) { d.magic = 0; d.more = fl - 1; }
    else {
        const uint64_t k2 = 1ULL << (32 + fl); uint64_t pm = k2 / W; const uint64_t rem = k2 - pm * W;
        pm += pm; const uint64_t tr = rem + rem;
        if (tr >= W || tr < rem) pm += 1;
        d.magic = (uint32_t)(1 + pm); d.more = fl;
    }
    return d;
}

// What a pulse asks for (ray_first, ray_count, interleave_*), the lattice size, and the handle's dealt tile list
// (rts_set_tile_list); list_mark is the interleave_parts value that selects that list (RTS_INTERLEAVE_LIST).
struct RtsRangeArgs {
    uint64_t ray_first, ray_count, total;
    uint32_t il_tile, il_parts, il_part, list_mark;
    uint32_t list_tile, list_n, list_last, list_gen;
};
enum RtsRangeError { RTS_RANGE_OK = 0, RTS_RANGE_LIST_TILE, RTS_RANGE_BAD_INTERLEAVE, RTS_RANGE_OUTSIDE, RTS_RANGE_LIST_BEYOND };
// The launch indices a pulse traces: `count` of them, drawn from the `span` indices from `first` on; il_* as the launch
// constants carry them (a dealt list: il_parts = list_mark, il_part = the list's generation).  The checks run in the order of
// the enum and the first that fails is returned; the fields resolved up to there are valid (range_tiles: tiles of il_tile
// indices in the span, for the list's last check).
struct RtsRayRange {
    RtsRangeError err;
    uint64_t first, span, count, range_tiles;
    uint32_t il_tile, il_parts, il_part;
    bool il_list;
};
inline RtsRayRange rts_ray_range(const RtsRangeArgs& q)
{
    RtsRayRange r = {RTS_RANGE_OK, q.ray_first, q.ray_count ? q.ray_count : (q.total > q.ray_first ? q.total - q.ray_first : 0), 0, 0, 0, 0, 0, q.il_parts == q.list_mark};
    if (r.il_list) {
        if (q.list_tile == 0 || q.il_tile != q.list_tile) { r.err = RTS_RANGE_LIST_TILE; return r; }
        r.il_tile = q.list_tile; r.il_parts = q.list_mark; r.il_part = q.list_gen;
    } else if (q.il_parts > 1) {
        r.il_tile = q.il_tile; r.il_parts = q.il_parts; r.il_part = q.il_part;
        if (r.il_tile == 0 || r.il_part >= r.il_parts) { r.err = RTS_RANGE_BAD_INTERLEAVE; return r; }
    }
    if (r.first > q.total || r.span > q.total - r.first) { r.err = RTS_RANGE_OUTSIDE; return r; }
    if (!r.il_list) { r.count = rts_part_count(r.span, r.il_tile, r.il_parts, r.il_part); return r; }
    // every listed tile is whole, except the last tile of the range when it is listed (the list is ascending: it is the last entry)
    r.range_tiles = (r.span + r.il_tile - 1) / r.il_tile;
    if (q.list_n == 0) return r;
    if (q.list_last >= r.range_tiles) { r.err = RTS_RANGE_LIST_BEYOND; return r; }
    r.count = (uint64_t)q.list_n * r.il_tile;
    if (q.list_last == r.range_tiles - 1) r.count -= r.range_tiles * r.il_tile - r.span;
    return r;
}

// Blocks of the ordinary trace kernel: one thread per launch index, capped at the resident set -- grid_mult blocks of 256 threads
// per CU (4 fill a CU's register file; the persistent waves draw tiles from a queue) less grid_spare block slots per 256 CUs, left
// free for the short kernels of the pulses that share the GPU (160 measured best with three pulses in flight: 0.709 vs 0.735
// ms/pulse at 64) -- and never 0.
inline uint32_t rts_trace_grid(uint32_t n, int n_cu, int grid_mult, int grid_spare)
{
    const uint32_t grid = (uint32_t)std::min<uint64_t>(((uint64_t)n + RTS_BLOCK - 1) / RTS_BLOCK, (uint64_t)std::max<int>((n_cu * grid_mult - grid_spare * n_cu / 256) * (256 / RTS_BLOCK), n_cu));
    return grid ? grid : 1;
}

// Blocks of the cooperative kernel for head_hint tiles at the head of the cost order, each traced as 64 units (RTS_COOP_GROUP
// when the units are grouped: 64 / RTS_COOP_GROUP rays per unit); four units per block, at least 16 blocks, at most
// coop_grid_max.  0: no head, no cooperative kernel this launch.
inline uint32_t rts_coop_grid(uint32_t head_hint, bool grouped, uint32_t coop_grid_max)
{
    const uint64_t units = (grouped ? (uint64_t)RTS_COOP_GROUP : 64ULL) * head_hint;
    return units == 0 ? 0u : (uint32_t)std::min<uint64_t>(coop_grid_max, std::max<uint64_t>(16, (units + 3) / 4));
}

// Element counts of the per-pulse buffers of a launch of n indices: `threads` of the ordinary kernel and coop_threads of the
// cooperative one own a row of the child slab, stack_threads + coop_threads a row of the overflow stack (a launch: its threads;
// rts_reserve: its bound of either), `blocks` (both kernels') a row of counters.  0: the launch has no such buffer.
struct RtsLaunchSizes { uint64_t recv, dir_hist, child, stack_ovf, block_counters, all, hit_prim, hit_t; };
inline RtsLaunchSizes rts_launch_sizes(uint64_t n, uint64_t threads, uint64_t stack_threads, uint64_t coop_threads, uint64_t blocks, uint32_t max_refl, uint32_t max_refr, bool keep_all)
{
    const uint64_t chains = rts_chains(max_refr), H = rts_hit_rows(max_refl);
    RtsLaunchSizes s;
    s.recv = n * chains + 1;
    s.dir_hist = (max_refr ? 3 * H : std::max<uint64_t>(max_refl, 1)) * 3 * n + 4;
    s.child = max_refr ? 2 * (threads + coop_threads) : 0;
    s.stack_ovf = (uint64_t)RTS_STACK_OVF * (stack_threads + coop_threads);
    s.block_counters = blocks * 8;
    s.all = keep_all ? n * chains + 1 : 0;
    s.hit_prim = s.hit_t = keep_all ? n * H + 1 : 0;
    return s;
}

// Shape of a launch: its signature (what a cost record of the launch is keyed by, rts_post.hip), whether its wave tiles are
// 64 CONSECUTIVE launch indices that line up with the history's (the tile-level screen and the cost records need that), its
// wave tiles and those of the whole lattice.
struct RtsLaunchShape { uint64_t sig[4]; bool aligned; uint32_t n_tiles, n_hist; };
inline RtsLaunchShape rts_launch_shape(uint32_t n, uint64_t first, uint32_t il_tile, uint32_t il_parts, uint32_t il_part, uint64_t total)
{
    RtsLaunchShape s = {{n, first, ((uint64_t)il_parts << 32) | il_tile, il_part},
                        first % RTS_WTILE == 0 && (il_parts <= 1 || il_tile % RTS_WTILE == 0),
                        (uint32_t)rts_wave_tiles(n), (uint32_t)rts_wave_tiles(total)};
    return s;
}
