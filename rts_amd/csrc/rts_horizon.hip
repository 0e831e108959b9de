// rts_horizon.hip -- the per-primitive HORIZON of a scene's meshes (once per scene, shared like d_prim_order): for every
// primitive T, in target space, two numbers S+(T), S-(T) in [0, 1], one per side of T's plane (+: the side the record's normal
// n = e1 x e0 points to).  A bounce ray that leaves T on a side at an elevation whose sine exceeds that side's S cannot meet
// T's own mesh again, and the trace kernel skips that target's walk for it (rts_shade, rts_trace.hip; the rule and its whole
// error budget: DESIGN.md section 4, "the horizon").
//
// What S bounds.  h(x) = the height of x above T's plane on the side in question.  With the mesh's extent E (the diagonal of its
// bounding box), h0 = RTS_HZ_H0 E and rho = RTS_HZ_RHO E:
//     S >= h(x) / |x - q|   for every point x of the SAME mesh's surface with h(x) > h0 and every q within rho of T (in space).
// The pair bound (conservative, not tight): for another primitive U of the mesh, hmax = the largest height of its three
// vertices (a triangle's heights are convex combinations of its vertices'), gap = |c_U - c_T| - r_U - r_T - rho with c, r the
// primitives' bounding spheres (centroid, farthest vertex): every x of U is at least gap from every q.  hmax <= h0: U contributes
// nothing.  Else gap <= 0: S = 1 (the side is closed: a concave edge, a touching part).  Else S = max(S, hmax / gap), at most 1.
// The work is quadratic and culled in two levels: blocks of RTS_HZ_BLOCK primitives in leaf order (neighbours in space) with a
// bounding sphere (C, R); a block contributes nothing to a side if hC + R <= h0 (wholly not above the plane) or if
// (hC + R) / (|C - c_T| - R - r_T - rho) does not exceed what the side already holds.
// Switched off for a mesh (every S = 1) when it holds a triangle that is degenerate or not finite -- smallest altitude
// 2 area / longest edge below RTS_HZ_DEGEN E: the f64 triangle test's own error is no longer small against tmin / 2 there --
// or when its share of the work, primitives x blocks of the scene, exceeds RTS_HZ_WORK_CAP.
#include <cmath>
#include "rts_internal.h"
#include "rts_ray_ops.h"

#define RTS_HZ_BLOCK 64u
#define RTS_HZ_WORK_CAP (1ull << 31)
#define RTS_HZ_SLICES 8u            // the blocks are dealt to this many threads per primitive (a primitive's 1 500 block tests are one dependent chain; the scene's primitives alone do not fill the device)

struct RtsHzPrim { double cx, cy, cz, r, nx, ny, nz, d; };      // bounding sphere; unit normal and plane offset (height of x = n . x - d)
struct RtsHzBlk { double cx, cy, cz, r; uint32_t tlo, thi; };  // bounding sphere of the block's primitives; the targets it holds

// per position i of the order: the primitive's sphere and plane, its vertices side by side; a degenerate one raises its mesh's flag
__global__ void k_hz_prims(const uint32_t* __restrict__ order, const uint32_t* __restrict__ tri_vidx, const double* __restrict__ verts, const uint32_t* __restrict__ prim_targ,
                           uint32_t n, const RtsHorizonMesh* __restrict__ mesh, uint32_t* __restrict__ mesh_off, RtsHzPrim* __restrict__ hp, double* __restrict__ pv)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint32_t g = order[i], t = prim_targ[g];
    double p[9];
    for (int k = 0; k < 3; k++) { const uint32_t v = tri_vidx[3 * (size_t)g + k]; for (int a = 0; a < 3; a++) p[3 * k + a] = verts[3 * (size_t)v + a]; }
    for (int k = 0; k < 9; k++) pv[(size_t)i * 9 + k] = p[k];
    dvec3 e0, e1, nn;
    tri_terms(mk3(p[0], p[1], p[2]), mk3(p[3], p[4], p[5]), mk3(p[6], p[7], p[8]), e0, e1, nn);      // the record's normal: e1 x e0, the same orientation
    const double nl = sqrt(nn.x * nn.x + nn.y * nn.y + nn.z * nn.z);
    const double l0 = sqrt(e0.x * e0.x + e0.y * e0.y + e0.z * e0.z), l1 = sqrt(e1.x * e1.x + e1.y * e1.y + e1.z * e1.z);
    const double e2x = p[6] - p[3], e2y = p[7] - p[4], e2z = p[8] - p[5], l2 = sqrt(e2x * e2x + e2y * e2y + e2z * e2z);
    const double longest = fmax(l0, fmax(l1, l2));
    const bool good = isfinite(nl) && isfinite(longest) && longest > 0.0 && nl / longest >= RTS_HZ_DEGEN * mesh[t].extent;
    if (!good) atomicOr(&mesh_off[t], 1u);
    RtsHzPrim q;
    q.cx = (p[0] + p[3] + p[6]) / 3.0; q.cy = (p[1] + p[4] + p[7]) / 3.0; q.cz = (p[2] + p[5] + p[8]) / 3.0;
    double r2 = 0.0;
    for (int k = 0; k < 3; k++) { const double dx = p[3 * k] - q.cx, dy = p[3 * k + 1] - q.cy, dz = p[3 * k + 2] - q.cz; r2 = fmax(r2, dx * dx + dy * dy + dz * dz); }
    q.r = sqrt(r2) * (1.0 + 1e-12);
    const double inv = good ? 1.0 / nl : 0.0;
    q.nx = nn.x * inv; q.ny = nn.y * inv; q.nz = nn.z * inv; q.d = q.nx * p[0] + q.ny * p[1] + q.nz * p[2];
    hp[i] = q;
}

// per block of RTS_HZ_BLOCK positions: a sphere around its primitives' spheres (centre: the mean of their centres), its targets' range
__global__ void k_hz_blocks(const uint32_t* __restrict__ order, const uint32_t* __restrict__ prim_targ, uint32_t n, uint32_t n_blocks, const RtsHzPrim* __restrict__ hp, RtsHzBlk* __restrict__ hb)
{
    const uint32_t b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= n_blocks) return;
    const uint32_t i0 = b * RTS_HZ_BLOCK, i1 = min(n, i0 + RTS_HZ_BLOCK);
    double cx = 0, cy = 0, cz = 0; uint32_t tlo = 0xffffffffu, thi = 0u;
    for (uint32_t i = i0; i < i1; i++) { cx += hp[i].cx; cy += hp[i].cy; cz += hp[i].cz; const uint32_t t = prim_targ[order[i]]; tlo = min(tlo, t); thi = max(thi, t); }
    const double m = 1.0 / (double)(i1 - i0); cx *= m; cy *= m; cz *= m;
    double r = 0.0;
    for (uint32_t i = i0; i < i1; i++) { const double dx = hp[i].cx - cx, dy = hp[i].cy - cy, dz = hp[i].cz - cz; r = fmax(r, sqrt(dx * dx + dy * dy + dz * dz) + hp[i].r); }
    RtsHzBlk o; o.cx = cx; o.cy = cy; o.cz = cz; o.r = isfinite(r) ? r * (1.0 + 1e-12) : INFINITY; o.tlo = tlo; o.thi = thi;      // (not finite: never culled)
    hb[b] = o;
}

// one side's share of a pair / block bound: what a height hmax at a distance of at least gap adds to s
__device__ __forceinline__ double hz_raise(double s, double hmax, double gap, double h0)
{
    if (!(hmax <= h0)) s = (gap > 0.0) ? fmax(s, fmin(1.0, hmax / gap)) : 1.0;      // (written so that a NaN closes the side)
    return s;
}

// thread (i, slice): primitive T = order[i] against the blocks b = slice, slice + RTS_HZ_SLICES, ..., then every primitive of the blocks that may raise one of
// its sides; the slices' results meet in an atomic maximum on the f32 bits (S >= 0: the bits order like the values; the array starts at zero)
__global__ void __launch_bounds__(256) k_hz_main(const uint32_t* __restrict__ order, const uint32_t* __restrict__ prim_targ, uint32_t n, uint32_t n_blocks, const RtsHorizonMesh* __restrict__ mesh,
                                                 const uint32_t* __restrict__ mesh_off, const RtsHzPrim* __restrict__ hp, const RtsHzBlk* __restrict__ hb, const double* __restrict__ pv,
                                                 uint32_t* __restrict__ horizon)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x, slice = blockIdx.y;
    if (i >= n) return;
    const uint32_t g = order[i], t = prim_targ[g];
    double sp = 0.0, sm = 0.0;
    if (mesh_off[t]) { sp = 1.0; sm = 1.0; }
    else {
        const RtsHzPrim T = hp[i];
        const double h0 = RTS_HZ_H0 * mesh[t].extent, rho = RTS_HZ_RHO * mesh[t].extent;
        for (uint32_t b = slice; b < n_blocks && !(sp >= 1.0 && sm >= 1.0); b += RTS_HZ_SLICES) {
            const RtsHzBlk B = hb[b];
            if (t < B.tlo || t > B.thi) continue;
            const double hc = T.nx * B.cx + T.ny * B.cy + T.nz * B.cz - T.d;
            const double dx = B.cx - T.cx, dy = B.cy - T.cy, dz = B.cz - T.cz;
            const double gap = sqrt(dx * dx + dy * dy + dz * dz) - B.r - T.r - rho;
            if (hz_raise(sp, hc + B.r, gap, h0) <= sp && hz_raise(sm, -hc + B.r, gap, h0) <= sm) continue;      // the block can raise neither side
            const uint32_t j0 = b * RTS_HZ_BLOCK, j1 = min(n, j0 + RTS_HZ_BLOCK);
            for (uint32_t j = j0; j < j1; j++) {
                if (j == i || prim_targ[order[j]] != t) continue;
                const RtsHzPrim U = hp[j];
                const double* u = pv + (size_t)j * 9;
                const double a0 = T.nx * u[0] + T.ny * u[1] + T.nz * u[2] - T.d, a1 = T.nx * u[3] + T.ny * u[4] + T.nz * u[5] - T.d, a2 = T.nx * u[6] + T.ny * u[7] + T.nz * u[8] - T.d;
                const double ex = U.cx - T.cx, ey = U.cy - T.cy, ez = U.cz - T.cz;
                const double pg = sqrt(ex * ex + ey * ey + ez * ez) - U.r - T.r - rho;
                sp = hz_raise(sp, fmax(a0, fmax(a1, a2)), pg, h0);
                sm = hz_raise(sm, fmax(-a0, fmax(-a1, -a2)), pg, h0);
            }
        }
    }
    // narrowed upwards: the f32 the leaf record carries is never below the f64 bound
    float fp = (float)sp, fm = (float)sm;
    if ((double)fp < sp) fp = __uint_as_float(__float_as_uint(fp) + 1u);
    if ((double)fm < sm) fm = __uint_as_float(__float_as_uint(fm) + 1u);
    atomicMax(&horizon[2 * (size_t)g], __float_as_uint(fminf(fp, 1.0f))); atomicMax(&horizon[2 * (size_t)g + 1], __float_as_uint(fminf(fm, 1.0f)));
}

// The scene's horizon: ns->d_horizon [n_prims][2] (S+, S-) and ns->hz[t] (extent, h0, rho of mesh t; rho = 0: the mesh is off).
// Called by rts_set_scene behind scene_finish (d_prim_order exists); the scratch arrays are freed on return.
int rts_horizon_build(RtsContext* c, RtsScene* ns, const RtsSceneFlat& flat)
{
    const uint32_t n = ns->n_prims, n_targets = (uint32_t)ns->meshes.size();
    ns->hz.assign(n_targets, RtsHorizonMesh{0.0, 0.0, 0.0});
    if (!n) return RTS_OK;
    const uint32_t n_blocks = (n + RTS_HZ_BLOCK - 1u) / RTS_HZ_BLOCK;
    std::vector<uint32_t> off(n_targets, 0u);
    for (uint32_t t = 0; t < n_targets; t++) {
        RtsBlasInfo b; rts_mesh_bounds(flat, t, &b);
        double e2 = 0; for (int a = 0; a < 3; a++) e2 += (b.hi[a] - b.lo[a]) * (b.hi[a] - b.lo[a]);
        const double E = std::sqrt(e2);
        ns->hz[t].extent = E; ns->hz[t].h0 = RTS_HZ_H0 * E; ns->hz[t].rho = RTS_HZ_RHO * E;
        if (!(E > 0.0) || !std::isfinite(E) || (unsigned long long)ns->meshes[t].n_tris * n_blocks > RTS_HZ_WORK_CAP) off[t] = 1u;
    }
    DevBuf<RtsHorizonMesh> d_mesh; DevBuf<uint32_t> d_off; DevBuf<RtsHzPrim> d_hp; DevBuf<RtsHzBlk> d_hb; DevBuf<double> d_pv;
    RTS_HIP(d_mesh.reserve(n_targets)); RTS_HIP(d_off.reserve(n_targets)); RTS_HIP(d_hp.reserve(n)); RTS_HIP(d_hb.reserve(n_blocks)); RTS_HIP(d_pv.reserve((size_t)n * 9));
    RTS_HIP(ns->d_horizon.reserve((size_t)n * 2));
    RTS_HIP(hipStreamSynchronize(c->stream));
    RTS_HIP(hipMemcpy(d_mesh.p, ns->hz.data(), sizeof(RtsHorizonMesh) * n_targets, hipMemcpyHostToDevice));
    RTS_HIP(hipMemcpy(d_off.p, off.data(), sizeof(uint32_t) * n_targets, hipMemcpyHostToDevice));
    k_hz_prims<<<(n + 255u) / 256u, 256, 0, c->stream>>>(ns->d_prim_order.p, ns->d_tri_vidx.p, ns->d_verts_local.p, ns->d_prim_targ.p, n, d_mesh.p, d_off.p, d_hp.p, d_pv.p);
    k_hz_blocks<<<(n_blocks + 255u) / 256u, 256, 0, c->stream>>>(ns->d_prim_order.p, ns->d_prim_targ.p, n, n_blocks, d_hp.p, d_hb.p);
    RTS_HIP(hipMemsetAsync(ns->d_horizon.p, 0, sizeof(float) * 2 * (size_t)n, c->stream));
    k_hz_main<<<dim3((n + 255u) / 256u, RTS_HZ_SLICES), 256, 0, c->stream>>>(ns->d_prim_order.p, ns->d_prim_targ.p, n, n_blocks, d_mesh.p, d_off.p, d_hp.p, d_hb.p, d_pv.p, reinterpret_cast<uint32_t*>(ns->d_horizon.p));
    RTS_HIP(hipGetLastError());
    RTS_HIP(hipMemcpyAsync(off.data(), d_off.p, sizeof(uint32_t) * n_targets, hipMemcpyDeviceToHost, c->stream));
    RTS_HIP(hipStreamSynchronize(c->stream));
    for (uint32_t t = 0; t < n_targets; t++) if (off[t]) ns->hz[t].rho = 0.0;      // (the trace kernel's rule asks 4 delta <= rho: never)
    return RTS_OK;
}

// the scene's horizon as the leaf records carry it: out[n_prims][2] = (S+, S-) by global primitive id
extern "C" int rts_get_horizon(RtsHandle c, float* out, uint32_t capacity_prims)
{
    CHECK_HANDLE(c);
    if (!out) { rts_set_error("rts_get_horizon: null argument"); return RTS_ERR_INVALID; }
    const RtsScene* sc = c->scene;
    if (capacity_prims < sc->n_prims) { rts_set_error("rts_get_horizon: capacity too small (%u primitives)", sc->n_prims); return RTS_ERR_CAPACITY; }
    RTS_HIP(hipStreamSynchronize(c->stream));
    if (sc->n_prims) RTS_HIP(hipMemcpy(out, sc->d_horizon.p, sizeof(float) * 2 * (size_t)sc->n_prims, hipMemcpyDeviceToHost));
    return RTS_OK;
}
