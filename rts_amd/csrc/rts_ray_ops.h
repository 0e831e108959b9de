// rts_ray_ops.h -- the f64 triangle test of the trace kernel: a literal restatement of the cited reference lines
// (operand order matters: results are compared bit-for-bit with the CPU oracle).
#pragma once
#include "rts_internal.h"

struct TriHit { double t, beta, gamma; dvec3 n; bool ok; };

// The ray-free terms of the test (triangle_mesh.cu:127-129: e0 = p1 - p0, e1 = p0 - p2, n = cross(e1, e0)), formed ONCE per
// pulse where the placed vertices are in registers (k_leaves, rts_bvh.hip) and carried by the leaf record: same operands, same
// operations in the same order, contraction off -- the bits the test formed for itself at every step of every lane.
__device__ __forceinline__ void tri_terms(dvec3 p0, dvec3 p1, dvec3 p2, dvec3& e0, dvec3& e1, dvec3& n)
{
    e0 = sub3(p1, p0);
    e1 = sub3(p0, p2);
    n = cross3(e1, e0);
}

// intersect_triangle_doubles, triangle_mesh.cu:121-137 (tmin/tmax are the f32 ray constants).  Lines 127-129 -- the edges and
// the normal -- moved to the placement kernel (tri_terms above); the test starts at line 130, 1 / dot(n, d).
__device__ __forceinline__ TriHit tri_test(const RtsLeafTri& L, dvec3 o, dvec3 d, float tmin, float tmax)
{
    const dvec3 p0 = mk3(L.p0x, L.p0y, L.p0z);
    const dvec3 e0 = mk3(L.e0x, L.e0y, L.e0z);
    const dvec3 e1 = mk3(L.e1x, L.e1y, L.e1z);
    TriHit h;
    h.n = mk3(L.nx, L.ny, L.nz);
    const dvec3 e2 = scale3(1 / dot3(h.n, d), sub3(p0, o));
    const dvec3 i = cross3(d, e2);
    h.beta = dot3(i, e1);
    h.gamma = dot3(i, e0);
    h.t = dot3(h.n, e2);
    h.ok = (h.t < (double)tmax) & (h.t > (double)tmin) & (h.beta >= 0.0) & (h.gamma >= 0.0) & (h.beta + h.gamma <= 1);
    return h;
}
