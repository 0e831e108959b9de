// rts_scene_host.h -- the host arithmetic of rts_set_scene (rts_scene.hip): the caller's meshes flattened into the scene's global
// index arrays -- the only place that keeps a bad vertex or normal index from reaching a kernel --, one mesh's host-built tree
// appended to the scene's, and a mesh's f64 bounds for the device builder (rts_lbvh.hip).
// Host only, no HIP, no handle: tests/test_scene_host.py builds it alone (tests/scene_host/scene_host_main.cpp).
#pragma once
#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <vector>
#include "../../include/rts_amd.h"

void rts_set_error(const char* fmt, ...);

// BVH4 node, 128 B = one cache line, of the static target-space hierarchy (rts_sah.cpp): half the dependent fetch
// round-trips of a binary tree per ray.  SoA over the four children so that one dwordx4 load brings the same plane of
// all four (padded, f32, TARGET-SPACE) boxes.  Unused slots: empty box (never hit).
struct __attribute__((aligned(128))) RtsNode4 {
    float lox[4], loy[4], loz[4], hix[4], hiy[4], hiz[4];
    int32_t child[4];               // >= 0 -> node index, < 0 -> ~leaf slot, 0x7fffffff -> unused
    int32_t pad[4];
};
static_assert(sizeof(RtsNode4) == 128, "node4 size");

// One mesh's slice of the static hierarchy (host side).
struct RtsBlasInfo { int32_t root; uint32_t n_nodes, n_leaves, depth; double lo[3], hi[3], max_abs; };

struct RtsMeshHost {
    uint32_t n_tris, n_verts, n_normals;
    uint32_t tri_base, vert_base, normal_base;
    double refl_coeff, refr_index;
    bool perface;
};

// The scene as the device takes it: the meshes' slices and the targets concatenated in order.
struct RtsSceneFlat {
    std::vector<RtsMeshHost> meshes;
    std::vector<uint32_t> vidx, nidx;       // [n_tris][3] GLOBAL vertex / normal indices
    std::vector<uint32_t> ptarg, vtarg, ntarg;      // the target of every primitive, vertex, normal
    std::vector<double> verts, normals;     // [n_verts][3], [n_normals][3], each mesh in its own frame
    uint64_t n_tris = 0, n_verts = 0, n_normals = 0;
};

// Counts first (null arrays, the target and size limits: nothing of an array is read before they hold), then the arrays.
static inline int rts_scene_flatten(const RtsMesh* meshes, uint32_t n_targets, bool interpolate_smooth, RtsSceneFlat* out)
{
    if (n_targets && !meshes) { rts_set_error("rts_set_scene: null meshes"); return RTS_ERR_INVALID; }
    if (n_targets > 254) { rts_set_error("rts_set_scene: more than 254 targets"); return RTS_ERR_UNSUPPORTED; }
    std::vector<RtsMeshHost>& mh = out->meshes; mh.assign(n_targets, RtsMeshHost{});
    uint64_t nt = 0, nv = 0, nn = 0;
    for (uint32_t t = 0; t < n_targets; t++) {
        const RtsMesh& m = meshes[t];
        if ((m.n_triangles && !m.triangles) || (m.n_vertices && !m.vertices) || (m.n_normals && !m.normals)) { rts_set_error("rts_set_scene: target %u has null arrays", t); return RTS_ERR_INVALID; }
        mh[t].n_tris = m.n_triangles; mh[t].n_verts = m.n_vertices; mh[t].n_normals = m.n_normals;
        mh[t].tri_base = (uint32_t)nt; mh[t].vert_base = (uint32_t)nv; mh[t].normal_base = (uint32_t)nn;
        mh[t].refl_coeff = m.refl_coeff; mh[t].refr_index = m.refr_index;
        mh[t].perface = m.n_normals > m.n_vertices;                              // triangle_mesh.cu:178
        nt += m.n_triangles; nv += m.n_vertices; nn += m.n_normals;
        if (nt > 0x7ffffff0ULL || nv > 0x7ffffff0ULL || nn > 0x7ffffff0ULL) { rts_set_error("rts_set_scene: scene too large"); return RTS_ERR_UNSUPPORTED; }
    }
    out->n_tris = nt; out->n_verts = nv; out->n_normals = nn;
    std::vector<uint32_t>& vidx = out->vidx; std::vector<uint32_t>& nidx = out->nidx;
    vidx.assign(3*nt, 0); nidx.assign(3*nt, 0); out->vtarg.assign(nv, 0); out->ntarg.assign(nn, 0); out->ptarg.assign(nt, 0);
    out->verts.assign(3*nv, 0.0); out->normals.assign(3*nn, 0.0);
    for (uint32_t t = 0; t < n_targets; t++) {
        const RtsMesh& m = meshes[t]; const RtsMeshHost& h = mh[t];
        for (uint32_t i = 0; i < m.n_triangles; i++) {
            for (int k = 0; k < 3; k++) {
                uint32_t v = m.triangles[3*(size_t)i + k];
                if (v >= m.n_vertices) { rts_set_error("rts_set_scene: target %u triangle %u references vertex %u >= %u", t, i, v, m.n_vertices); return RTS_ERR_INVALID; }
                vidx[3*((size_t)h.tri_base + i) + k] = h.vert_base + v;
                // dbuf_normals is indexed by the vertex index (triangle_mesh.cu:170-172), or by the
                // primitive index for per-face ("rect") normals (:178-180)
                uint32_t ni = h.perface ? i : v;
                if (m.n_normals == 0) ni = 0; else if (ni >= m.n_normals) { rts_set_error("rts_set_scene: target %u normal index %u >= %u", t, ni, m.n_normals); return RTS_ERR_INVALID; }
                nidx[3*((size_t)h.tri_base + i) + k] = h.normal_base + ni;
            }
            out->ptarg[(size_t)h.tri_base + i] = t;
        }
        if (m.n_triangles && m.n_normals == 0 && interpolate_smooth) { rts_set_error("rts_set_scene: target %u has no normals but interpolate_smooth is set", t); return RTS_ERR_INVALID; }
        for (uint32_t i = 0; i < m.n_vertices; i++) { out->vtarg[(size_t)h.vert_base + i] = t; for (int k = 0; k < 3; k++) out->verts[3*((size_t)h.vert_base + i) + k] = m.vertices[3*(size_t)i + k]; }
        for (uint32_t i = 0; i < m.n_normals; i++) { out->ntarg[(size_t)h.normal_base + i] = t; for (int k = 0; k < 3; k++) out->normals[3*((size_t)h.normal_base + i) + k] = m.normals[3*(size_t)i + k]; }
    }
    return RTS_OK;
}

// One mesh's tree as the host builder leaves it (rts_sah_build: node and leaf-slot numbers of its own, leaf primitives local to
// the mesh) appended to the scene's: node children move by the nodes, ~slot children by the slots in front of it (an unused
// child stays), leaf primitives by tri_base, the root by the nodes.
static inline void rts_scene_append_tree(const std::vector<RtsNode4>& mesh_nodes, const std::vector<uint32_t>& mesh_leaf_prim, uint32_t tri_base,
                                         std::vector<RtsNode4>* nodes4, std::vector<uint32_t>* leaf_prim, RtsBlasInfo* blas)
{
    const int32_t node_base = (int32_t)nodes4->size(), leaf_base = (int32_t)leaf_prim->size();
    for (RtsNode4 nd : mesh_nodes) {
        for (int k = 0; k < 4; k++) { int32_t& ch = nd.child[k]; if (ch == 0x7fffffff) continue; if (ch >= 0) ch += node_base; else ch = ~(~ch + leaf_base); }
        nodes4->push_back(nd);
    }
    for (uint32_t lp : mesh_leaf_prim) leaf_prim->push_back(lp + tri_base);
    if (blas->root >= 0) blas->root += node_base;
}

// A coordinate a hierarchy can hold: finite AND far enough inside the f32 range for its padded, outward-rounded box to stay finite
// (load_tri of rts_lbvh.hip applies the same bound).  A triangle with any other coordinate gets no leaf from either builder: kept, the
// f32 boxes of its leaf and of every ancestor up to the root overflow to the "unused" sentinel and hide the valid triangles beside it.
static inline bool rts_coord_valid(double x) { return std::fabs(x) < 3.0e38; }

// The f64 bounds of mesh t over its valid triangles (for the per-pulse placement constants): lo / hi, zeros when it has none,
// and the largest magnitude among them.
static inline void rts_mesh_bounds(const RtsSceneFlat& f, uint32_t t, RtsBlasInfo* b)
{
    const RtsMeshHost& m = f.meshes[t];
    double lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
    uint32_t nv = 0;
    for (uint32_t i = 0; i < m.n_tris; i++) {
        bool finite = true;
        for (int k = 0; k < 3; k++) { const double* p = &f.verts[3 * (size_t)f.vidx[3 * ((size_t)m.tri_base + i) + k]]; finite = finite && rts_coord_valid(p[0]) && rts_coord_valid(p[1]) && rts_coord_valid(p[2]); }
        if (!finite) continue;
        nv++;
        for (int k = 0; k < 3; k++) { const double* p = &f.verts[3 * (size_t)f.vidx[3 * ((size_t)m.tri_base + i) + k]]; for (int a = 0; a < 3; a++) { lo[a] = std::min(lo[a], p[a]); hi[a] = std::max(hi[a], p[a]); } }
    }
    b->max_abs = 0;
    for (int a = 0; a < 3; a++) { b->lo[a] = nv ? lo[a] : 0; b->hi[a] = nv ? hi[a] : 0; b->max_abs = std::max(b->max_abs, std::max(std::fabs(b->lo[a]), std::fabs(b->hi[a]))); }
}
