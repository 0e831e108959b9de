// rts_post_plan.h -- the integer decisions of a pulse's post-processing (order, expand, finalise, aggregate: rts_post.hip and the
// end-of-pulse part of rts_api.hip), each written once: the width and packing of the (receiver, path) aggregation key, the sort
// bits of the received-row key, what the one-block sorts take and how many items per thread, the capacity of a chain enqueued on
// the device-side count, and where the aggregation's scratch buffers are sliced.  No HIP, no handle, no allocation: plain structs
// returned by value, so it compiles with any host compiler and is tested without a GPU (tests/test_post_plan_host.py).
#pragma once
#include <cstdint>
#include <cstddef>

#ifndef RTS_MAX_DEPTH
#define RTS_MAX_DEPTH 16              // include/rts_amd.h
#endif
#define RTS_SMALL_THREADS 256         // threads of the one-block ordering / finishing kernels (rts_post.hip: k_agg_order_small)
#define RTS_SMALL_CAP32 4096u         // received rays those kernels take with 32-bit sort keys ...
#define RTS_SMALL_CAP64 2048u         // ... and with 64-bit keys: the block's sort storage has to stay below the 40 KB of a free block slot
#define RTS_AGG_TILE 256              // rays per tile of the aggregation's fixed-shape sums (rts_post.hip: agg_tile_block)

// the smallest b >= 1 with 2^b >= n (64 for an n beyond 2^63)
inline uint32_t rts_bits_for(uint64_t n) { uint32_t b = 1; while (b < 64 && ((uint64_t)1 << b) < n) b++; return b; }

// ---- the aggregation key: equal keys <=> same receiver and identical path row (aggregation.cu:46-53)
//   key = rx << (D * B) | sum_k (path[k] + 1) << (k * B),   B bits per path entry (-1 .. max_path -> 0 .. max_path + 1; none at
//   D == 0), RXB for the receiver (0 .. max_rx).  Up to 64 bits it is one word; beyond (`wide`) the general chain sorts it as
//   n_words words and the later stages read a surrogate that keeps the receiver alone, at bit 32.  `shift`: where the receiver
//   sits in the word those stages read.  n_rx_tab: rows of the per-receiver totals.  supported: what rts_aggregate_device takes.
// The handle passes max_path = targets - 1 and max_rx = max(receivers, 1) - 1; rts_kernel_wrapper_on the largest entries of its
// caller's arrays.
struct RtsKeyPlan { uint32_t B, RXB, key_bits, shift, n_words, n_rx_tab; bool wide, supported; };
inline RtsKeyPlan rts_key_plan(uint32_t D, int64_t max_path, int64_t max_rx)
{
    RtsKeyPlan k;
    k.B = D ? rts_bits_for((uint64_t)(max_path + 2)) : 0u;
    k.RXB = rts_bits_for((uint64_t)(max_rx + 1));
    const uint64_t bits = (uint64_t)D * k.B + k.RXB;
    k.key_bits = bits > 0xffffffffu ? 0xffffffffu : (uint32_t)bits;
    k.wide = bits > 64;
    k.shift = k.wide ? 32u : D * k.B;               // (narrow: D * B <= 63, RXB >= 1)
    k.n_words = (uint32_t)((bits + 63u) / 64u);
    k.n_rx_tab = (uint32_t)max_rx + 1u;
    k.supported = D <= RTS_MAX_DEPTH && bits <= 256;
    return k;
}
// One-word keys as k_agg_keys and agg_order_block pack them (k_agg_keys_wide: the same fields across words); rts_aggregate_fetch
// decodes the groups' keys with the two functions below -- of a wide key's surrogate only the receiver.
inline uint64_t rts_key_encode(const RtsKeyPlan& k, uint32_t D, uint32_t rx, const int32_t* path)
{
    uint64_t key = (uint64_t)rx << k.shift;
    for (uint32_t c = 0; c < D; c++) key |= (uint64_t)(uint32_t)(path[c] + 1) << (c * k.B);
    return key;
}
inline uint32_t rts_key_rx(const RtsKeyPlan& k, uint64_t key) { return k.shift >= 64 ? 0u : (uint32_t)(key >> k.shift); }
inline int32_t rts_key_path(const RtsKeyPlan& k, uint64_t key, uint32_t c)
{
    const uint64_t pmask = k.shift >= 64 ? ~(uint64_t)0 : ((uint64_t)1 << k.shift) - 1;
    return (int32_t)(((key & pmask) >> (c * k.B)) & (((uint64_t)1 << k.B) - 1)) - 1;
}

// ---- the received-row key: row = chain * n_rays + launch slot (three chains with refraction: rts_launch_plan.h: rts_chains).
// Sort bits such that the padding key, 2^bits - 1, stays above every row; never more than 40.
inline uint32_t rts_recv_sort_bits(uint32_t n_rays, uint32_t max_refr)
{
    const uint64_t rows = (uint64_t)n_rays * (max_refr ? 3u : 1u);
    uint32_t bits = 1; while (bits < 40 && ((uint64_t)1 << bits) <= rows) bits++;
    return bits;
}

// ---- the one-block sorts: which key type, how many rays, how many items per thread
inline bool rts_recv_key64(uint32_t max_refr) { return max_refr != 0; }                  // refraction chains in the row key
inline bool rts_agg_key64(const RtsKeyPlan& k) { return k.key_bits >= 32u; }              // (a 32-bit sort leaves a bit for the padding key)
inline uint32_t rts_small_cap(bool key64) { return key64 ? RTS_SMALL_CAP64 : RTS_SMALL_CAP32; }
inline uint32_t rts_small_items(uint32_t cap) { return cap <= 4u * RTS_SMALL_THREADS ? 4u : cap <= 8u * RTS_SMALL_THREADS ? 8u : 16u; }
// Capacity of a post-processing chain enqueued on the device-side count (rts_trace_pulse_end_uniform): the smaller of its two
// sorts.  0, never: a wide key is sorted by the general chain, whose kernels take the count from the host.
inline uint32_t rts_spec_cap(uint32_t max_refr, const RtsKeyPlan& k)
{
    if (k.wide) return 0;
    const uint32_t a = rts_small_cap(rts_recv_key64(max_refr)), b = rts_small_cap(rts_agg_key64(k));
    return a < b ? a : b;
}

// ---- the aggregation's scratch for R rays and n_rx_tab receivers: element counts of the buffers, and the slices inside them
//   d_gcount (uint32):  gstart [R + 1] | .. | d_G, the group count, at o_G
//   d_gsum (double):    gsum [5 R] | tile_first [5 ntiles] at o_tile_first | tile_last [5 ntiles] at o_tile_last
//   d_rcs (double):     rxtot [5 n_rx_tab] | rxmin (uint32 [n_rx_tab]) at o_rxmin
// per_ray: the sort's keys and indices, head flags, group ids and the group table, one element per ray each.
struct RtsAggLayout { uint32_t ntiles; size_t per_ray, gcount, gsum, rcs, o_G, o_tile_first, o_tile_last, o_rxmin; };
inline RtsAggLayout rts_agg_layout(uint32_t R, uint32_t n_rx_tab)
{
    RtsAggLayout l;
    l.ntiles = (uint32_t)(((uint64_t)R + RTS_AGG_TILE - 1) / RTS_AGG_TILE);
    l.per_ray = R;
    l.gcount = (size_t)R + 4; l.o_G = (size_t)R + 2;
    l.gsum = 5 * ((size_t)R + 2 * (size_t)l.ntiles) + 16; l.o_tile_first = 5 * (size_t)R; l.o_tile_last = l.o_tile_first + 5 * (size_t)l.ntiles;
    l.rcs = 5 * (size_t)n_rx_tab + n_rx_tab + 8; l.o_rxmin = 5 * (size_t)n_rx_tab;
    return l;
}
