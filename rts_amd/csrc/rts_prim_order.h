// rts_prim_order.h -- the static order in which the per-pulse scene update (k_leaves, rts_bvh.hip) walks the primitives.
//
// The leaf records are indexed by primitive, but the block that rasterises its 256 triangles into the primary-ray mask wants
// them to be neighbours in space: the hierarchy's leaf slots are (the host builder numbers them depth-first, the device builder
// along its sorted references), the mesh's own numbering need not be.  The order is the primitives by their FIRST appearance in
// the leaf slots -- a triangle cut into several references has several slots, the later ones are dropped -- and behind them,
// ascending, every primitive no slot names (a triangle the device builder found no finite box for): the kernel visits each
// primitive exactly once whatever the builders keep.
// Host only, no HIP: tests/test_prim_order_host.py builds it alone.
#pragma once
#include <cstddef>
#include <cstdint>
#include <vector>

// (a slot that names no primitive of the scene -- >= n_prims -- is skipped)
static inline std::vector<uint32_t> rts_prim_order(const uint32_t* leaf_prim, size_t n_leaves, uint32_t n_prims)
{
    std::vector<uint32_t> order; order.reserve(n_prims);
    std::vector<uint8_t> seen(n_prims, 0);
    for (size_t s = 0; s < n_leaves; s++) {
        const uint32_t g = leaf_prim[s];
        if (g < n_prims && !seen[g]) { seen[g] = 1; order.push_back(g); }
    }
    for (uint32_t g = 0; g < n_prims; g++) if (!seen[g]) order.push_back(g);
    return order;
}
