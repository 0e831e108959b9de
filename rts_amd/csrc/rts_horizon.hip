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
//
// BY AZIMUTH SECTOR.  A wing rises over a fuselage triangle's plane in one direction only, so each side carries FOUR values S_k, one per quadrant of the in-plane azimuth
// in T's own frame u = e0 / |e0|, w = n x u (n = e1 x e0, the record's normal): sector k = (a . u < 0 ? 1 : 0) | (a . w < 0 ? 2 : 0).  The contract, per sector, is the old one:
//     S_k >= h(x) / |x - q|   for every such x and q whenever the azimuth of (x - q), projected into T's plane, lies in quadrant k WIDENED by eps_az = RTS_HZ_EPS_AZ on both edges.
// eps_az = 2^-6 rad: a placement may be off a rotation by 1e-3 (fill_target_placement), which turns the placed frame against this one by no more than that; the rule's two sign
// tests are f64 dot products of vectors it reads from the placed record, wrong only within ~1e-15 rad of a boundary.  2^-6 is more than 15 x the sum.
// Which sectors another primitive or block U (sphere c_U, r_U) can reach from any q within rho of T (q in the sphere c_T, r_T + rho): x - q = P + v with P = c_U - c_T and
// |v| <= R = r_U + r_T + rho, so the in-plane coordinates of x - q lie in [P.u - R, P.u + R] x [P.w - R, P.w + R] (a box around the disc: no tighter than the contract) and
// the in-plane length is at most |P| + R.  A direction a is inside the widened quadrant (su, sw) exactly when su a.u >= -|a| sin eps_az and sw a.w >= -|a| sin eps_az, so U is
// attributed to every quadrant with su P.u + m >= 0 and sw P.w + m >= 0, m = R + (|P| + R) (eps_az + 1e-9) (sin x <= x; 1e-9 for the roundings of P.u, P.w) -- all four when
// |P| <= R.  A block is skipped only when it can raise none of the eight values.
// Storage: the eight values as BYTES, b = S rounded UP to a multiple of 1/255 (RTS_HZ_DECODE(b) >= S, checked with the decoder's own expression; 0 is exactly 0, 255 closed),
// in the two words per primitive that held S+ and S- as floats: word = side, byte k = sector k.  The slices' results meet in an atomic maximum on a scratch array of bytes-as-words.
#include <algorithm>
#include <cmath>
#include <vector>
#include "rts_internal.h"
#include "rts_ray_ops.h"

#define RTS_HZ_BLOCK 64u
#define RTS_HZ_WORK_CAP (1ull << 31)
#define RTS_HZ_SLICES 8u            // the blocks are dealt to this many threads per primitive (a primitive's 1 500 block tests are one dependent chain; the scene's primitives alone do not fill the device)

struct RtsHzPrim { double cx, cy, cz, r, nx, ny, nz, d, ux, uy, uz, wx, wy, wz; };      // bounding sphere; unit normal and plane offset (height of x = n . x - d); the in-plane frame u = e0 / |e0|, w = n x u
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
    const double iu = (good && l0 > 0.0) ? 1.0 / l0 : 0.0;      // (a mesh that is off never looks at its frames)
    q.ux = e0.x * iu; q.uy = e0.y * iu; q.uz = e0.z * iu;
    q.wx = q.ny * q.uz - q.nz * q.uy; q.wy = q.nz * q.ux - q.nx * q.uz; q.wz = q.nx * q.uy - q.ny * q.ux;
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

// the quadrants (bit k = sector k) that a sphere of radius R around the offset P (in-plane coordinates pu, pw; dist >= the in-plane length of P) can reach, each widened by
// RTS_HZ_EPS_AZ (the head of this file); written so that a NaN reaches all four
__device__ __forceinline__ uint32_t hz_reach(double pu, double pw, double dist, double R)
{
    const double m = R + (dist + R) * (RTS_HZ_EPS_AZ + 1e-9);
    const bool up = !(pu + m < 0.0), un = !(m - pu < 0.0), wp = !(pw + m < 0.0), wn = !(m - pw < 0.0);
    return (up && wp ? 1u : 0u) | (un && wp ? 2u : 0u) | (up && wn ? 4u : 0u) | (un && wn ? 8u : 0u);
}

// the byte a value s in [0, 1] is stored as: rounded UP against the decoder's own expression; 1, beyond and NaN: 255 (closed)
__device__ __forceinline__ uint32_t hz_encode(double s)
{
    if (!(s < 1.0)) return 255u;
    uint32_t b = s > 0.0 ? (uint32_t)ceil(s * 255.0) : 0u;
    if (b > 255u) b = 255u;
    while (b < 255u && RTS_HZ_DECODE(b) < s) b++;
    return b;
}

// thread (i, slice): primitive T = order[i] against the blocks b = slice, slice + RTS_HZ_SLICES, ..., then every primitive of the blocks that may raise one of
// its eight values (side x sector); the slices' results meet in an atomic maximum on the bytes, one word each (acc [n][8] by global primitive id: side * 4 + sector; starts at zero)
__global__ void __launch_bounds__(256) k_hz_main(const uint32_t* __restrict__ order, const uint32_t* __restrict__ prim_targ, uint32_t n, uint32_t n_blocks, const RtsHorizonMesh* __restrict__ mesh,
                                                 const uint32_t* __restrict__ mesh_off, const RtsHzPrim* __restrict__ hp, const RtsHzBlk* __restrict__ hb, const double* __restrict__ pv,
                                                 uint32_t* __restrict__ acc)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x, slice = blockIdx.y;
    if (i >= n) return;
    const uint32_t g = order[i], t = prim_targ[g];
    double s[8] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    if (mesh_off[t]) { for (int k = 0; k < 8; k++) s[k] = 1.0; }
    else {
        const RtsHzPrim T = hp[i];
        const double h0 = RTS_HZ_H0 * mesh[t].extent, rho = RTS_HZ_RHO * mesh[t].extent;
        for (uint32_t b = slice; b < n_blocks; b += RTS_HZ_SLICES) {
            bool closed = true;
            for (int k = 0; k < 8; k++) closed = closed && s[k] >= 1.0;
            if (closed) break;
            const RtsHzBlk B = hb[b];
            if (t < B.tlo || t > B.thi) continue;
            const double hc = T.nx * B.cx + T.ny * B.cy + T.nz * B.cz - T.d;
            const double dx = B.cx - T.cx, dy = B.cy - T.cy, dz = B.cz - T.cz;
            const double dist = sqrt(dx * dx + dy * dy + dz * dz), gap = dist - B.r - T.r - rho;
            const uint32_t reach = hz_reach(dx * T.ux + dy * T.uy + dz * T.uz, dx * T.wx + dy * T.wy + dz * T.wz, dist, B.r + T.r + rho);
            bool raises = false;                                     // the block can raise none of the eight values: skipped
            for (int k = 0; k < 4; k++) if (reach >> k & 1u) raises = raises || hz_raise(s[k], hc + B.r, gap, h0) > s[k] || hz_raise(s[4 + k], -hc + B.r, gap, h0) > s[4 + k];
            if (!raises) continue;
            const uint32_t j0 = b * RTS_HZ_BLOCK, j1 = min(n, j0 + RTS_HZ_BLOCK);
            for (uint32_t j = j0; j < j1; j++) {
                if (j == i || prim_targ[order[j]] != t) continue;
                const RtsHzPrim U = hp[j];
                const double* u = pv + (size_t)j * 9;
                const double a0 = T.nx * u[0] + T.ny * u[1] + T.nz * u[2] - T.d, a1 = T.nx * u[3] + T.ny * u[4] + T.nz * u[5] - T.d, a2 = T.nx * u[6] + T.ny * u[7] + T.nz * u[8] - T.d;
                const double ex = U.cx - T.cx, ey = U.cy - T.cy, ez = U.cz - T.cz;
                const double pd = sqrt(ex * ex + ey * ey + ez * ez), pg = pd - U.r - T.r - rho;
                const uint32_t pr = hz_reach(ex * T.ux + ey * T.uy + ez * T.uz, ex * T.wx + ey * T.wy + ez * T.wz, pd, U.r + T.r + rho);
                const double hp_ = fmax(a0, fmax(a1, a2)), hm_ = fmax(-a0, fmax(-a1, -a2));
                for (int k = 0; k < 4; k++) if (pr >> k & 1u) { s[k] = hz_raise(s[k], hp_, pg, h0); s[4 + k] = hz_raise(s[4 + k], hm_, pg, h0); }
            }
        }
    }
    for (int k = 0; k < 8; k++) { const uint32_t b = hz_encode(s[k]); if (b) atomicMax(&acc[8 * (size_t)g + k], b); }
}

// the eight bytes of a primitive into the two words the leaf record carries: word = side, byte k = sector k
__global__ void k_hz_pack(const uint32_t* __restrict__ acc, uint32_t n, uint32_t* __restrict__ horizon)
{
    const uint32_t g = blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= n) return;
    for (int side = 0; side < 2; side++) {
        const uint32_t* a = acc + 8 * (size_t)g + 4 * side;
        horizon[2 * (size_t)g + side] = (a[0] & 0xffu) | (a[1] & 0xffu) << 8 | (a[2] & 0xffu) << 16 | (a[3] & 0xffu) << 24;
    }
}

// The scene's horizon: ns->d_horizon [n_prims][2] (side +, side -: four sector bytes each) and ns->hz[t] (extent, h0, rho of mesh t; rho = 0: the mesh is off).
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
    DevBuf<RtsHorizonMesh> d_mesh; DevBuf<uint32_t> d_off; DevBuf<RtsHzPrim> d_hp; DevBuf<RtsHzBlk> d_hb; DevBuf<double> d_pv; DevBuf<uint32_t> d_acc;
    RTS_HIP(d_mesh.reserve(n_targets)); RTS_HIP(d_off.reserve(n_targets)); RTS_HIP(d_hp.reserve(n)); RTS_HIP(d_hb.reserve(n_blocks)); RTS_HIP(d_pv.reserve((size_t)n * 9)); RTS_HIP(d_acc.reserve((size_t)n * 8));
    RTS_HIP(ns->d_horizon.reserve((size_t)n * 2));
    RTS_HIP(hipStreamSynchronize(c->stream));
    RTS_HIP(hipMemcpy(d_mesh.p, ns->hz.data(), sizeof(RtsHorizonMesh) * n_targets, hipMemcpyHostToDevice));
    RTS_HIP(hipMemcpy(d_off.p, off.data(), sizeof(uint32_t) * n_targets, hipMemcpyHostToDevice));
    k_hz_prims<<<(n + 255u) / 256u, 256, 0, c->stream>>>(ns->d_prim_order.p, ns->d_tri_vidx.p, ns->d_verts_local.p, ns->d_prim_targ.p, n, d_mesh.p, d_off.p, d_hp.p, d_pv.p);
    k_hz_blocks<<<(n_blocks + 255u) / 256u, 256, 0, c->stream>>>(ns->d_prim_order.p, ns->d_prim_targ.p, n, n_blocks, d_hp.p, d_hb.p);
    RTS_HIP(hipMemsetAsync(d_acc.p, 0, sizeof(uint32_t) * 8 * (size_t)n, c->stream));
    k_hz_main<<<dim3((n + 255u) / 256u, RTS_HZ_SLICES), 256, 0, c->stream>>>(ns->d_prim_order.p, ns->d_prim_targ.p, n, n_blocks, d_mesh.p, d_off.p, d_hp.p, d_hb.p, d_pv.p, d_acc.p);
    k_hz_pack<<<(n + 255u) / 256u, 256, 0, c->stream>>>(d_acc.p, n, ns->d_horizon.p);
    RTS_HIP(hipGetLastError());
    RTS_HIP(hipMemcpyAsync(off.data(), d_off.p, sizeof(uint32_t) * n_targets, hipMemcpyDeviceToHost, c->stream));
    RTS_HIP(hipStreamSynchronize(c->stream));
    for (uint32_t t = 0; t < n_targets; t++) if (off[t]) ns->hz[t].rho = 0.0;      // (the trace kernel's rule asks 4 delta <= rho: never)
    return RTS_OK;
}

// the sector bytes of the scene's primitives, off the device: out[n_prims][2] words
static int hz_fetch(RtsContext* c, const char* who, const void* out, uint32_t capacity_prims, std::vector<uint32_t>& w)
{
    if (!out) { rts_set_error("%s: null argument", who); return RTS_ERR_INVALID; }
    const RtsScene* sc = c->scene;
    if (capacity_prims < sc->n_prims) { rts_set_error("%s: capacity too small (%u primitives)", who, sc->n_prims); return RTS_ERR_CAPACITY; }
    RTS_HIP(hipStreamSynchronize(c->stream));
    w.resize(2 * (size_t)sc->n_prims);
    if (sc->n_prims) RTS_HIP(hipMemcpy(w.data(), sc->d_horizon.p, sizeof(uint32_t) * 2 * (size_t)sc->n_prims, hipMemcpyDeviceToHost));
    return RTS_OK;
}

// the scene's ISOTROPIC horizon: out[n_prims][2] = (S+, S-) by global primitive id, per side the largest of its four decoded sectors -- the S the rule tests first
// (never below the decoded f64: narrowed upwards; 0 and 1 exact)
extern "C" int rts_get_horizon(RtsHandle c, float* out, uint32_t capacity_prims)
{
    CHECK_HANDLE(c);
    std::vector<uint32_t> w;
    RTS_TRY(hz_fetch(c, "rts_get_horizon", out, capacity_prims, w));
    for (size_t k = 0; k < w.size(); k++) {
        const uint32_t b = std::max(std::max(w[k] & 0xffu, w[k] >> 8 & 0xffu), std::max(w[k] >> 16 & 0xffu, w[k] >> 24));
        const double s = RTS_HZ_DECODE(b);
        float f = b == 255u ? 1.0f : (float)s;
        if ((double)f < s) f = std::nextafterf(f, 2.0f);
        out[k] = f;
    }
    return RTS_OK;
}

// the horizon as the leaf records carry it: out[n_prims][2][4] bytes by global primitive id, side (+, -) and sector; a byte b stands for b / 255 (RTS_HZ_DECODE)
extern "C" int rts_get_horizon_sectors(RtsHandle c, uint8_t* out, uint32_t capacity_prims)
{
    CHECK_HANDLE(c);
    std::vector<uint32_t> w;
    RTS_TRY(hz_fetch(c, "rts_get_horizon_sectors", out, capacity_prims, w));
    for (size_t k = 0; k < w.size(); k++) for (int j = 0; j < 4; j++) out[4 * k + j] = (uint8_t)(w[k] >> (8 * j) & 0xffu);
    return RTS_OK;
}
