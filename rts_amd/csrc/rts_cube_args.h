// rts_cube_args.h -- the pure rules the cube entry points apply to their arguments (rts_cube_api.h words the messages): a span
// inside a total, a power of two in a range, two byte ranges against each other, an output against every receiver's span of
// the input, the source fields of a beamformer-style record, a caller's device list and its length.  Each returns the fact, or the number of the rule that broke.
// Host only, no HIP, no handle: tests/test_cube_args_host.py builds it alone (tests/cube_args/cube_args_main.cpp).
#pragma once
#include <cstddef>
#include <cstdint>
#include "../../include/rts_amd.h"

// first .. first + n inside [0, total): first < total and n <= total - first (no sum that could wrap).  n == 0 is "to the end"
// (zero_to_end) or a span of none; at_least_one refuses the latter.  count: what the span holds
static inline bool rts_span_inside(uint32_t first, uint32_t n, uint32_t total, bool zero_to_end, bool at_least_one, uint32_t* count = nullptr)
{
    if (first >= total || n > total - first) return false;
    const uint32_t have = n == 0 && zero_to_end ? total - first : n;
    if (at_least_one && have == 0) return false;
    if (count) *count = have;
    return true;
}

// v is a power of two in [lo, hi]
static inline bool rts_pow2_in(uint32_t v, uint32_t lo, uint32_t hi) { return v != 0 && v >= lo && v <= hi && (v & (v - 1u)) == 0u; }

// na bytes at a against nb bytes at b
static inline bool rts_bytes_overlap(const void* a, size_t na, const void* b, size_t nb)
{
    const uintptr_t a0 = (uintptr_t)a, a1 = a0 + na, b0 = (uintptr_t)b, b1 = b0 + nb;
    return a0 < b1 && b0 < a1;
}

// out_bytes bytes at out against what a call reads of n_rx receivers: of receiver r the cells cell0 .. cell1 (one past the last) of
// its rx_stride cells at src, a cell being one complex128.  *rx: the first receiver whose span the output overlaps
static inline bool rts_rx_spans_overlap(const void* out, size_t out_bytes, const void* src, uint64_t rx_stride, uint64_t cell0, uint64_t cell1, uint32_t n_rx, uint32_t* rx)
{
    for (uint32_t r = 0; r < n_rx; r++) {
        const uintptr_t i0 = (uintptr_t)src + 16u * (uintptr_t)(r * rx_stride + cell0);
        if (rts_bytes_overlap(out, out_bytes, (const void*)i0, 16u * (size_t)(cell1 - cell0))) { *rx = r; return true; }
    }
    return false;
}

// the source fields of a record that reads the cube, the Doppler map or the caller's pointer.  0: consistent; 1: unknown source;
// 2: n_rows_in without RTS_BEAM_FROM_POINTER; 3: device_in without it; 4: n_rows_in = 0 with it
static inline int rts_source_fields_rule(uint32_t source, uint32_t n_rows_in, const void* device_in)
{
    if (source > RTS_BEAM_FROM_POINTER) return 1;
    if (source != RTS_BEAM_FROM_POINTER && n_rows_in != 0) return 2;
    if (source != RTS_BEAM_FROM_POINTER && device_in) return 3;
    if (source == RTS_BEAM_FROM_POINTER && n_rows_in == 0) return 4;
    return 0;
}

// a counted list handed to the host: of `total` records found, `max` are stored, `capacity` fit the caller's array
static inline uint32_t rts_list_copied(uint32_t total, uint32_t max, uint32_t capacity)
{
    const uint32_t stored = total < max ? total : max;
    return stored < capacity ? stored : capacity;
}

// a caller-owned device list of n_list records of 8-byte alignment (null: the handle's own).  0: consistent; 1: n_list without a
// list; 2: n_list above `most`; 3: the list is not 8-byte aligned
static inline int rts_device_list_rule(const void* device_list, uint32_t n_list, uint32_t most)
{
    if (!device_list && n_list != 0) return 1;
    if (n_list > most) return 2;
    if ((uintptr_t)device_list & 7u) return 3;
    return 0;
}
