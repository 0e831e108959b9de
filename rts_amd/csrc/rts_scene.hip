// rts_scene.hip -- the scene of a handle: rts_set_scene (flatten, upload, build, finish, swap), the two kernels that finish a
// hierarchy whichever builder made it, what a handle keeps per scene (rts_attach_scene), sharing (rts_share_scene) and
// introspection (rts_scene_info, rts_get_bvh).  The host arithmetic -- the flattening with its index checks, the concatenation of
// the host builder's trees -- is rts_scene_host.h; the builders are rts_lbvh.hip (device) and rts_sah.cpp (host).
#include <cstdio>
#include <cstring>
#include <algorithm>
#include <chrono>
#include <memory>
#include <thread>
#include "rts_internal.h"
#include "rts_prim_order.h"

__global__ void k_children_to_prims(RtsNode4* __restrict__ nodes, uint32_t n, const uint32_t* __restrict__ leaf_prim)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    for (int k = 0; k < 4; k++) { const int32_t ch = nodes[i].child[k]; nodes[i].pad[k] = ch; if (ch < 0) nodes[i].child[k] = ~(int32_t)leaf_prim[~ch]; }
}

// OCTANT VERSIONS of the node records (round 5; RtsScene::d_nodes4v, [node][octant]).  A ray's octant in a target's frame -- the
// signs of its direction there -- is fixed for a whole walk, and two things the node step used to work out per visit depend on
// nothing else: which plane of a child's slab the ray enters through (low when it runs towards +axis, high towards -axis: the
// role fetch formed six per-lane addresses for that) and a good front-to-back order of the four children (the step sorted the
// four entry distances: 5 compares + 20 selects).  Both are baked here, once per scene: version o of a node holds, per child
// slot, [entry planes x y z | exit planes x y z | child: ~primitive, or 8 x node + o = the child's record of the same octant], the slots in ascending order of the children's position along the
// octant's diagonal (key_mode 1, the default: the box's centre; 0: its entry corner), unused slots (degenerate box, never entered) last.
// The trace kernel reads the record of (node, octant) straight through and visits the open children in slot order.
// Eight times the node bytes (BASELINE configs[2]: 18 -> 145 MB, configs[3]: 185 MB -> 1.5 GB of 288 GB), of which a walk
// touches one version only.
__global__ void k_node_versions(const RtsNode4* __restrict__ nodes, uint32_t n, RtsNode4* __restrict__ out, int key_mode)
{
    const uint32_t g = blockIdx.x * blockDim.x + threadIdx.x;      // one thread per (node, octant)
    if (g >= n * 8u) return;
    const uint32_t i = g >> 3, o = g & 7u;
    const RtsNode4 nd = nodes[i];
    const bool mx = (o & 1u) != 0u, my = (o & 2u) != 0u, mz = (o & 4u) != 0u;      // the ray runs towards -x / -y / -z
    float key[4]; int ord[4];
    for (int k = 0; k < 4; k++) {
        const float ex = mx ? -nd.hix[k] : nd.lox[k], ey = my ? -nd.hiy[k] : nd.loy[k], ez = mz ? -nd.hiz[k] : nd.loz[k];      // entry corner, along the diagonal
        const float cx = 0.5f * (nd.lox[k] + nd.hix[k]), cy = 0.5f * (nd.loy[k] + nd.hiy[k]), cz = 0.5f * (nd.loz[k] + nd.hiz[k]);
        const float kc = key_mode == 1 ? ((mx ? -cx : cx) + (my ? -cy : cy) + (mz ? -cz : cz)) : (ex + ey + ez);
        key[k] = nd.child[k] == 0x7fffffff ? __builtin_inff() : kc;
        ord[k] = k;
    }
    for (int a = 1; a < 4; a++)                                     // stable insertion sort of four
        for (int b = a; b > 0 && key[ord[b]] < key[ord[b - 1]]; b--) { const int t = ord[b]; ord[b] = ord[b - 1]; ord[b - 1] = t; }
    RtsNode4 v;
    for (int j = 0; j < 4; j++) {
        const int k = ord[j];
        v.lox[j] = mx ? nd.hix[k] : nd.lox[k]; v.hix[j] = mx ? nd.lox[k] : nd.hix[k];      // lo* <- entry planes, hi* <- exit planes
        v.loy[j] = my ? nd.hiy[k] : nd.loy[k]; v.hiy[j] = my ? nd.loy[k] : nd.hiy[k];
        v.loz[j] = mz ? nd.hiz[k] : nd.loz[k]; v.hiz[j] = mz ? nd.loz[k] : nd.hiz[k];
        const int32_t ch = nd.child[k];
        v.child[j] = (ch >= 0 && ch != 0x7fffffff) ? (int32_t)(((uint32_t)ch << 3) | o) : ch;      // a node child: the index of ITS record of this octant (a walk never changes octant)
        v.pad[j] = nd.pad[k];
    }
    out[g] = v;
}

void rts_scene_unref(RtsScene* s) { if (s && --s->refs == 0) delete s; }

// ------------------------------------------------------------------------------------- rts_set_scene, step by step
// Every step works on the NEW scene object, which rts_set_scene holds until the swap: a step that fails leaves the handle's old scene alone.

// The flat arrays -> the new scene.  Blocking copies: each has landed before the first kernel that reads its target is enqueued on the handle's (non-blocking) stream -- the device builder's, k_children_to_prims behind the host builder's nodes.
static int scene_upload(RtsContext* c, RtsScene* ns, const RtsSceneFlat& f)
{
    const uint64_t nt = f.n_tris, nv = f.n_verts, nn = f.n_normals;
    RTS_HIP(hipStreamSynchronize(c->stream));
    RTS_HIP(ns->d_tri_vidx.reserve(3*nt + 1)); RTS_HIP(ns->d_tri_nidx.reserve(3*nt + 1)); RTS_HIP(ns->d_vert_targ.reserve(nv + 1)); RTS_HIP(ns->d_norm_targ.reserve(nn + 1));
    RTS_HIP(ns->d_prim_targ.reserve(nt + 1)); RTS_HIP(ns->d_verts_local.reserve(3*nv + 1)); RTS_HIP(ns->d_normals_local.reserve(3*nn + 1));
    if (nt) { RTS_HIP(hipMemcpy(ns->d_tri_vidx.p, f.vidx.data(), sizeof(uint32_t)*3*nt, hipMemcpyHostToDevice)); RTS_HIP(hipMemcpy(ns->d_tri_nidx.p, f.nidx.data(), sizeof(uint32_t)*3*nt, hipMemcpyHostToDevice));
              RTS_HIP(hipMemcpy(ns->d_prim_targ.p, f.ptarg.data(), sizeof(uint32_t)*nt, hipMemcpyHostToDevice)); }
    if (nv) { RTS_HIP(hipMemcpy(ns->d_vert_targ.p, f.vtarg.data(), sizeof(uint32_t)*nv, hipMemcpyHostToDevice)); RTS_HIP(hipMemcpy(ns->d_verts_local.p, f.verts.data(), sizeof(double)*3*nv, hipMemcpyHostToDevice)); }
    if (nn) { RTS_HIP(hipMemcpy(ns->d_norm_targ.p, f.ntarg.data(), sizeof(uint32_t)*nn, hipMemcpyHostToDevice)); RTS_HIP(hipMemcpy(ns->d_normals_local.p, f.normals.data(), sizeof(double)*3*nn, hipMemcpyHostToDevice)); }
    ns->meshes = f.meshes; ns->n_prims = (uint32_t)nt; ns->n_verts = (uint32_t)nv; ns->n_normals = (uint32_t)nn;
    return RTS_OK;
}

// The host builder: the meshes are independent, one host thread each (at most 16 at a time), results concatenated in target order.
static int scene_build_host(RtsScene* ns, const RtsMesh* meshes, double split_budget)
{
    const uint32_t n_targets = (uint32_t)ns->meshes.size();
    std::vector<RtsNode4> nodes4; std::vector<uint32_t> leaf_prim; std::vector<RtsBlasInfo> blas(n_targets);
    std::vector<std::vector<RtsNode4>> pn(n_targets); std::vector<std::vector<uint32_t>> pl(n_targets); std::vector<int> prc(n_targets, RTS_OK);
    for (uint32_t t0 = 0; t0 < n_targets; t0 += 16) {
        std::vector<std::thread> pool;
        for (uint32_t t = t0; t < std::min(n_targets, t0 + 16); t++)
            pool.emplace_back([&, t]() { prc[t] = rts_sah_build(meshes[t].vertices, meshes[t].triangles, meshes[t].n_triangles, split_budget, pn[t], pl[t], blas[t]); });
        for (auto& th : pool) th.join();
    }
    for (uint32_t t = 0; t < n_targets; t++) {
        if (prc[t] != RTS_OK) return prc[t];
        rts_scene_append_tree(pn[t], pl[t], ns->meshes[t].tri_base, &nodes4, &leaf_prim, &blas[t]);
    }
    RTS_HIP(ns->d_nodes4.reserve(nodes4.size() + 1)); RTS_HIP(ns->d_leaf_prim.reserve(leaf_prim.size() + 1));
    if (!nodes4.empty()) RTS_HIP(hipMemcpy(ns->d_nodes4.p, nodes4.data(), sizeof(RtsNode4)*nodes4.size(), hipMemcpyHostToDevice));
    if (!leaf_prim.empty()) RTS_HIP(hipMemcpy(ns->d_leaf_prim.p, leaf_prim.data(), sizeof(uint32_t)*leaf_prim.size(), hipMemcpyHostToDevice));
    ns->blas = blas; ns->n_nodes = (uint32_t)nodes4.size(); ns->n_leaves = (uint32_t)leaf_prim.size();
    ns->builder = 0;
    return RTS_OK;
}

// what a builder left in the new scene, dropped: the next builder starts from nothing
static void scene_drop_tree(RtsScene* ns) { ns->d_nodes4.release(); ns->d_leaf_prim.release(); ns->blas.clear(); ns->n_nodes = 0; ns->n_leaves = 0; }

// The static target-space hierarchy, one per mesh; leaf slots name GLOBAL primitive ids.  Two builders, same node format:
//   device (default) top-down binned SAH over split references, built on the GPU level by level (rts_lbvh.hip): milliseconds;
//          RTS_DEVICE_TREE=lbvh: the Morton / Karras tree of round 2 instead
//   host   RTS_BUILDER=host / RtsParams.flags & RTS_FLAG_HOST_BUILD: the same algorithm with a greedier reference splitter on
//          one host thread per mesh (rts_sah.cpp): ~1 s per 100 k triangles; traces a lone C3 pulse 7 % faster (its slowest
//          tile runs through the pole fans of the synthetic airframe), the pipelined benchmark, the dense control, spheres
//          and C4 within 1-4 %
// st.split_budget: extra references for triangles whose boxes are mostly empty (rts_sah.cpp, rts_lbvh.hip): an average triangle
// gets about 1 + budget references where cutting pays (2 measured best for both builders)
static int scene_build(RtsContext* c, RtsScene* ns, const RtsMesh* meshes, const RtsSceneFlat& f, const RtsSceneTuning& st)
{
    if (st.device_build) {
        // The device builder sizes its bins by the references of a level and closes within 256 levels or gives up: out of memory, or
        // a mesh it does not close on, must not fail the scene -- the host builder takes over (RTS_DEVICE_BUILD_FALLBACK=0:
        // the error is returned, for tests of the builder itself).
        int rc = rts_lbvh_build_device(c, ns, f, st);
        if (rc == RTS_OK && st.fail_device_build) { rts_set_error("rts_set_scene: device builder failure injected (RTS_DEBUG_FAIL_DEVICE_BUILD)"); rc = RTS_ERR_HIP; }      // tests: the fall-back below, with the builder's state to clean up
        if (rc == RTS_OK) { ns->builder = 1; return RTS_OK; }
        if (rc == RTS_ERR_INVALID || !st.build_fallback) return rc;
        (void)hipGetLastError();                                     // (a failed allocation leaves a sticky error code behind)
        fprintf(stderr, "[rts] device hierarchy build failed (%s): falling back to the host builder\n", rts_last_error());
        scene_drop_tree(ns);
    }
    return scene_build_host(ns, meshes, st.split_budget);
}

// What follows either builder: the nodes' leaf children from ~slot to ~primitive, the primitive order, the octant versions.
static int scene_finish(RtsContext* c, RtsScene* ns, const RtsSceneTuning& st)
{
    // Leaf records are kept per PRIMITIVE, not per leaf slot (a triangle cut into several references has several slots): the
    // nodes' leaf children are rewritten from ~slot to ~primitive here, once, whichever builder ran; the slot form is parked in
    // the record's unused words for rts_get_bvh.  A third of the per-pulse leaf refresh and of the leaf bytes on C3 (300 k slots
    // for 100 k triangles), and of the 240 MB per handle on BASELINE configs[3].
    if (ns->n_nodes) { k_children_to_prims<<<(ns->n_nodes + 255) / 256, 256, 0, c->stream>>>(ns->d_nodes4.p, ns->n_nodes, ns->d_leaf_prim.p); RTS_HIP(hipGetLastError()); RTS_HIP(hipStreamSynchronize(c->stream)); }
    // The order in which the per-pulse scene update visits the primitives (k_leaves, rts_bvh.hip): by first appearance in the leaf
    // slots, so that a block's 256 triangles are neighbours in space whatever the mesh's own numbering (rts_prim_order.h).  Once
    // per scene, whichever builder ran: one read-back of the slots, the de-duplication on the host.
    if (ns->n_prims) {
        std::vector<uint32_t> slots(ns->n_leaves);
        RTS_HIP(hipStreamSynchronize(c->stream));
        if (ns->n_leaves) RTS_HIP(hipMemcpy(slots.data(), ns->d_leaf_prim.p, sizeof(uint32_t) * ns->n_leaves, hipMemcpyDeviceToHost));
        const std::vector<uint32_t> order = rts_prim_order(slots.data(), slots.size(), ns->n_prims);
        RTS_HIP(ns->d_prim_order.reserve(order.size() + 1));
        RTS_HIP(hipMemcpy(ns->d_prim_order.p, order.data(), sizeof(uint32_t) * order.size(), hipMemcpyHostToDevice));
    }
    // the octant versions of the node records (k_node_versions): RTS_NODE_VERSIONS=0: none; they need 1 KB per node -- a scene whose
    // versions would not fit a quarter of the device's free memory goes without (the kernel then walks d_nodes4 as before)
    const bool want = st.node_versions;
    const int key_mode = st.version_key_centre ? 1 : 0;      // (measured, profiles/r05a_versions_ab.log: by centre the dense control visits 5.9 % more nodes than the sorted walk, by entry corner 9.6 %)
    size_t free_b = 0, total_b = 0; (void)hipMemGetInfo(&free_b, &total_b);
    const size_t need = (size_t)ns->n_nodes * 8 * sizeof(RtsNode4);
    if (want && ns->n_nodes && ns->n_nodes < (1u << 28) && need < free_b / 4) {
        if (ns->d_nodes4v.reserve((size_t)ns->n_nodes * 8) == hipSuccess) {
            k_node_versions<<<(ns->n_nodes * 8u + 255u) / 256u, 256, 0, c->stream>>>(ns->d_nodes4.p, ns->n_nodes, ns->d_nodes4v.p, key_mode);
            RTS_HIP(hipGetLastError()); RTS_HIP(hipStreamSynchronize(c->stream));
        } else (void)hipGetLastError();
    }
    return RTS_OK;
}

// Per-handle buffers sized by the scene the handle now points at; placement and tile history start afresh.
int rts_attach_scene(RtsContext* c)
{
    const RtsScene* sc = c->scene; const uint32_t n_targets = (uint32_t)sc->meshes.size();
    RTS_HIP(c->d_leaves.reserve((size_t)sc->n_prims + 1));      // one record per primitive (k_children_to_prims)
    RTS_HIP(c->d_verts_world.reserve(3*(size_t)sc->n_verts + 1)); RTS_HIP(c->d_normals_world.reserve(3*(size_t)sc->n_normals + 1));
    {   // device image of the pinned block's [lc | motion | td]
        const size_t span = offsetof(RtsPinned, cnt);
        RTS_HIP(c->d_params.reserve(span));
        c->p_lc = reinterpret_cast<RtsLaunchConsts*>(c->d_params.p + offsetof(RtsPinned, lc));
        c->p_motion = reinterpret_cast<RtsTargetMotion*>(c->d_params.p + offsetof(RtsPinned, motion));
        c->p_targets = reinterpret_cast<RtsTargetDev*>(c->d_params.p + offsetof(RtsPinned, td));
        c->rcs_uploaded = false;
    }
    c->verts_world_valid = false; c->order_sum_valid = false;
    if (c->hist->refs.load() > 1) { rts_hist_unref(c->hist); c->hist = new RtsTileHist(); }      // (a handle that leaves a shared scene leaves the shared history)
    c->motion.assign(n_targets, RtsTargetMotion{}); c->motion_valid = false; c->bvh_valid = false; c->hist->n = 0; c->hist->any = false; c->hist->head_hint_valid = false; c->tile_cost_pending = false; c->tile_last_valid = false;
    return RTS_OK;
}

// the new scene replaces the handle's (whose last reference deletes it)
static int scene_swap(RtsContext* c, RtsScene* ns)
{
    rts_scene_unref(c->scene);
    c->scene = ns;
    return rts_attach_scene(c);
}

extern "C" int rts_set_scene(RtsHandle c, const RtsMesh* meshes, uint32_t n_targets)
{
    CHECK_HANDLE(c);
    CHECK_CLOSED(c);
    RTS_TRY(check_key_width(c->depth, n_targets, c->n_rx, "rts_set_scene"));
    RtsSceneFlat flat;
    RTS_TRY(rts_scene_flatten(meshes, n_targets, c->params.interpolate_smooth, &flat));
    std::unique_ptr<RtsScene> ns(new RtsScene()); ns->device = c->device;      // swapped in at the end: every failure path below leaves the handle's old scene alone
    RTS_TRY(scene_upload(c, ns.get(), flat));
    const auto t_build0 = std::chrono::steady_clock::now();
    RtsSceneTuning st; st.device_build = (c->params.flags & RTS_FLAG_HOST_BUILD) == 0;
    rts_tuning_read(&st, rts_env);
    RTS_TRY(scene_build(c, ns.get(), meshes, flat, st));
    RTS_TRY(scene_finish(c, ns.get(), st));
    {   // the primitives' horizon (rts_horizon.hip): once per scene, like the order it is built along
        const auto t_hz0 = std::chrono::steady_clock::now();
        RTS_TRY(rts_horizon_build(c, ns.get(), flat));
        if (st.debug_build) fprintf(stderr, "[rts] horizon: %.2f ms\n", std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_hz0).count());
    }
    ns->build_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_build0).count();
    return scene_swap(c, ns.release());
}

// rts_share_scene: dst drops its own scene and uses src's (same device): the meshes, the hierarchy and its leaf order then
// exist once however many handles keep pulses in flight, and the hierarchy is built once.
extern "C" int rts_share_scene(RtsHandle dst, RtsHandle src)
{
    if (!dst || !src || dst == src) { rts_set_error("rts_share_scene: needs two distinct handles"); return RTS_ERR_INVALID; }
    if (dst->device != src->device) { rts_set_error("rts_share_scene: handles live on different devices (%d, %d)", dst->device, src->device); return RTS_ERR_INVALID; }
    if (dst->params.interpolate_smooth && !src->params.interpolate_smooth) {
        for (const RtsMeshHost& m : src->scene->meshes) if (m.n_tris && m.n_normals == 0) { rts_set_error("rts_share_scene: the scene has a mesh without normals but the receiving handle interpolates normals"); return RTS_ERR_INVALID; }
    }
    RtsContext* c = dst;
    CHECK_HANDLE(c);
    CHECK_CLOSED(c);
    RTS_HIP(hipStreamSynchronize(c->stream));
    if (dst->scene == src->scene) return RTS_OK;
    rts_scene_unref(dst->scene);
    dst->scene = src->scene; dst->scene->refs++;
    RTS_TRY(rts_attach_scene(dst));
    if (dst->tune.share_history && src->tune.share_history && dst->params.width == src->params.width) {      // ... and the tile-cost history of the scene's handles (RtsTileHist)
        rts_hist_unref(dst->hist);
        dst->hist = src->hist; dst->hist->refs++;
    }
    return RTS_OK;
}

extern "C" int rts_scene_info(RtsHandle c, RtsSceneInfo* out)
{
    if (!c || !out) { rts_set_error("rts_scene_info: null argument"); return RTS_ERR_INVALID; }
    const RtsScene* sc = c->scene;
    memset(out, 0, sizeof(*out));
    out->n_targets = (uint32_t)sc->meshes.size(); out->n_prims = sc->n_prims; out->n_nodes = sc->n_nodes; out->n_leaves = sc->n_leaves;
    out->handles_sharing = (uint32_t)sc->refs.load(); out->builder = sc->builder; out->build_ms = sc->build_ms;
    out->shared_device_bytes = sc->device_bytes(); out->version_bytes = sc->d_nodes4v.cap * sizeof(RtsNode4);
    out->horizon_bytes = sc->d_horizon.cap * sizeof(uint32_t);
    out->handle_device_bytes = c->d_leaves.cap * sizeof(RtsLeafTri) + c->d_verts_world.cap * 8 + c->d_normals_world.cap * 8 + c->d_params.cap;
    return RTS_OK;
}

// the hierarchy in the builders' form: leaf children as ~slot (k_children_to_prims parks them in pad[]), pad zero
extern "C" int rts_get_bvh(RtsHandle c, void* nodes128, uint32_t* leaf_prim, int32_t* roots, uint32_t node_capacity, uint32_t leaf_capacity, uint32_t* n_leaves)
{
    CHECK_HANDLE(c);
    if (n_leaves) *n_leaves = c->scene->n_leaves;
    if ((nodes128 && node_capacity < c->scene->n_nodes) || (leaf_prim && leaf_capacity < c->scene->n_leaves)) { rts_set_error("rts_get_bvh: capacity too small (%u nodes, %u leaves)", c->scene->n_nodes, c->scene->n_leaves); return RTS_ERR_CAPACITY; }
    RTS_HIP(hipStreamSynchronize(c->stream));
    if (nodes128 && c->scene->n_nodes) {
        RTS_HIP(hipMemcpy(nodes128, c->scene->d_nodes4.p, sizeof(RtsNode4)*c->scene->n_nodes, hipMemcpyDeviceToHost));
        RtsNode4* nd = static_cast<RtsNode4*>(nodes128);              // (the builders' form: leaf children as ~slot, see k_children_to_prims)
        for (uint32_t i = 0; i < c->scene->n_nodes; i++) for (int k = 0; k < 4; k++) { nd[i].child[k] = nd[i].pad[k]; nd[i].pad[k] = 0; }
    }
    if (leaf_prim && c->scene->n_leaves) RTS_HIP(hipMemcpy(leaf_prim, c->scene->d_leaf_prim.p, sizeof(uint32_t)*c->scene->n_leaves, hipMemcpyDeviceToHost));
    if (roots) for (size_t t = 0; t < c->scene->blas.size(); t++) roots[t] = c->scene->blas[t].root;
    return RTS_OK;
}
