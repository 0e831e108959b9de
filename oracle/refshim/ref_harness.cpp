// =====================================================================================
// ref_harness.cpp -- runs the reference's own device programs on the CPU.  TEST INFRASTRUCTURE ONLY.
//
// The reference's device sources are compiled unmodified as host C++ against the stand-in
// headers of this directory (rts_refshim.h) and driven through C entry points shaped like the
// oracle's (oracle/rts_oracle.cpp), so that one Python wrapper drives both and the tests can
// compare the oracle with the text it restates, bit for bit.
//
// Each source is included inside a namespace of its own: the three OptiX files declare the
// same variables (prd, ray, normal, dbuf_results ...) and each includes the unguarded
// ray_tracer.h, so each namespace has its own PerRayData (one layout, checked below).
//
// What the harness itself decides -- the part of OptiX that is not in the reference:
//   rtTrace            the brute force the project defines as "closest hit": every primitive of
//                      every target in global order through intersect(); a hit is kept when
//                      its f32 t is strictly smaller, so ties go to the lowest global id; then
//                      that target's closest_hit with its material variables, or miss
//   rtPayload          copied into the program's `prd` before a program runs and back after
//   nested rtTrace     payload, current ray, hit_t, the attribute `normal` and the material
//                      variables are saved and restored around the call
//   atan2f             of the miss program goes through a pointer: libm's by default, or the
//                      function installed with ref_set_atan2f (the oracle's orc_atan2f: "pinned")
//   kernel launches    a serial loop over blockIdx / threadIdx with the shape the reference's
//                      kernel_wrapper chooses (one block; a partial grid; the grid-stride arm)
// Not thread-safe: programs talk through namespace-scope variables, as they do through
// OptiX's variable scopes.
// =====================================================================================
#include "rts_refshim.h"

#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <sys/time.h>
#include <vector>

uint3 threadIdx, blockIdx;
dim3 blockDim, gridDim;

static float (*g_atan2f)(float, float) = ::atan2f;
static inline float refshim_atan2f(float y, float x) { return g_atan2f(y, x); }

namespace ref_tm {
#include "triangle_mesh.cu"
}
namespace ref_ns {
#include "normal_shader.cu"
}
#define atan2f(y, x) refshim_atan2f((y), (x))      // float parameters: the arguments are narrowed first, as in CUDA
namespace ref_rt {
#include "ray_tracer.cu"
}
#undef atan2f
namespace ref_ag {
#include "aggregation_kernels.cu"                   // written into oracle/_ref/ by the Makefile: the file up to its host section
}

typedef ref_rt::PerRayData PRD;
static_assert(sizeof(PRD) == 144 && alignof(PRD) == 16, "PerRayData layout");
static_assert(sizeof(ref_tm::PerRayData) == 144 && sizeof(ref_ns::PerRayData) == 144 && sizeof(ref_ag::PerRayData) == 144, "PerRayData layout");

// ------------------------------------------------------------------ scene and launch (the oracle's shapes)
struct RMesh {
    std::vector<uint3> tris; std::vector<double3> verts, normals;
    double reflCoeff, refrIndex;
};
struct RScene {
    std::vector<RMesh> meshes; std::vector<double3> vel;
    std::vector<double3> sphCentre; std::vector<double> sphRadius, minTheta, maxTheta, minPhi, maxPhi;
};
struct OPulse {                      // oracle/rts_oracle.cpp: OPulse
    double rayOrigin[3]; double txSpan[3]; double txDir[2];
    uint32_t width, maxRefl, maxRefr, interpolate_smooth;
};
struct Launch {
    RScene* sc; bool smooth;
    int* hit_prim; float* hit_t; unsigned hitCols; uint64_t rayIndex;
    uint64_t triTests, segments, shaded;
};
static Launch* g_launch = nullptr;

// ------------------------------------------------------------------ traversal state of one rtTrace
struct Trav {
    float tmin, tmax; bool found; unsigned targ, prim; float t; double3 normal;
    float pending; unsigned cur_targ, cur_prim;
};
static Trav* g_trav = nullptr;

bool rtPotentialIntersection(float t) { g_trav->pending = t; return (t > g_trav->tmin) && (t < g_trav->tmax); }
bool rtReportIntersection(unsigned int)
{
    Trav& tv = *g_trav;
    tv.tmax = tv.pending; tv.found = true; tv.t = tv.pending; tv.targ = tv.cur_targ; tv.prim = tv.cur_prim;
    tv.normal = ref_tm::normal;                      // the attribute as the intersection program left it
    return true;
}

static void bind_mesh(RMesh& m, bool smooth)
{
    ref_tm::dbuf_triangles.bind(m.tris.data(), m.tris.size());
    ref_tm::dbuf_triVertices.bind(m.verts.data(), m.verts.size());
    ref_tm::dbuf_normals.bind(m.normals.data(), m.normals.size());
    ref_tm::d_interpolate_smooth = smooth;
}

void refshim_trace(const optix::Ray& ray, void* payload, size_t payload_size)
{
    if (payload_size != sizeof(PRD)) { fprintf(stderr, "refshim: payload of %zu bytes\n", payload_size); abort(); }
    Launch& L = *g_launch;
    L.segments++;
    // everything a program of the CALLER may still read after this call returns
    const ref_tm::PerRayData s_tm_prd = ref_tm::prd; const optix::Ray s_tm_ray = ref_tm::ray; const double3 s_tm_normal = ref_tm::normal;
    const ref_ns::PerRayData s_ns_prd = ref_ns::prd; const optix::Ray s_ns_ray = ref_ns::ray; const double3 s_ns_normal = ref_ns::normal;
    const float s_hit_t = ref_ns::hit_t;
    const double s_refl = ref_ns::d_targReflCoeff, s_refr = ref_ns::d_targRefrIndex; const unsigned s_targ = ref_ns::d_targIndex;
    const ref_rt::PerRayData s_rt_prd = ref_rt::prd; const optix::Ray s_rt_ray = ref_rt::ray;
    Trav* const s_trav = g_trav;
    // the payload may BE one of those variables (a closest-hit program passes its own `prd` on): work on a copy, hand it back last
    PRD pay; memcpy(&pay, payload, sizeof(PRD));

    Trav tv; memset(&tv, 0, sizeof(tv));
    tv.tmin = ray.tmin; tv.tmax = ray.tmax; tv.found = false;
    g_trav = &tv;
    memcpy(&ref_tm::prd, &pay, sizeof(PRD)); ref_tm::ray = ray;
    for (unsigned ti = 0; ti < L.sc->meshes.size(); ti++) {
        RMesh& m = L.sc->meshes[ti];
        bind_mesh(m, L.smooth);
        for (unsigned pi = 0; pi < m.tris.size(); pi++) {
            tv.cur_targ = ti; tv.cur_prim = pi; L.triTests++;
            ref_tm::intersect((int)pi);
        }
    }
    // the oracle's debug record of the REFLECTION chain (a refracted payload has refrDepth >= 1): column = bounce number
    if (L.hit_prim && ref_tm::prd.refrDepth == 0 && ref_tm::prd.reflDepth < L.hitCols) {
        int gid = -1;
        if (tv.found) { gid = (int)tv.prim; for (unsigned k = 0; k < tv.targ; k++) gid += (int)L.sc->meshes[k].tris.size(); }
        L.hit_prim[L.rayIndex * L.hitCols + ref_tm::prd.reflDepth] = gid;
        L.hit_t[L.rayIndex * L.hitCols + ref_tm::prd.reflDepth] = tv.found ? tv.t : 0.0f;
    }
    if (tv.found) {
        const RMesh& m = L.sc->meshes[tv.targ];
        ref_ns::d_targReflCoeff = m.reflCoeff; ref_ns::d_targRefrIndex = m.refrIndex; ref_ns::d_targIndex = tv.targ;
        memcpy(&ref_ns::prd, &pay, sizeof(PRD)); ref_ns::ray = ray; ref_ns::hit_t = tv.t; ref_ns::normal = tv.normal;
        const unsigned before = ref_ns::prd.reflDepth;
        ref_ns::closest_hit();
        if (ref_ns::prd.reflDepth != before) L.shaded++;   // the shading body ran: it counts the bounce (normal_shader.cu:286)
        memcpy(&pay, &ref_ns::prd, sizeof(PRD));
    } else {
        memcpy(&ref_rt::prd, &pay, sizeof(PRD)); ref_rt::ray = ray;
        ref_rt::miss();
        memcpy(&pay, &ref_rt::prd, sizeof(PRD));
    }
    ref_tm::prd = s_tm_prd; ref_tm::ray = s_tm_ray; ref_tm::normal = s_tm_normal;
    ref_ns::prd = s_ns_prd; ref_ns::ray = s_ns_ray; ref_ns::normal = s_ns_normal; ref_ns::hit_t = s_hit_t;
    ref_ns::d_targReflCoeff = s_refl; ref_ns::d_targRefrIndex = s_refr; ref_ns::d_targIndex = s_targ;
    ref_rt::prd = s_rt_prd; ref_rt::ray = s_rt_ray;
    g_trav = s_trav;
    memcpy(payload, &pay, sizeof(PRD));
}

// =====================================================================================
//                                   extern "C" API (ctypes)
// =====================================================================================
extern "C" {

// fn == NULL: libm's atan2f; otherwise float fn(float y, float x), e.g. the oracle's orc_atan2f
void ref_set_atan2f(void* fn) { g_atan2f = fn ? (float (*)(float, float))fn : ::atan2f; }

void* ref_scene_create() { return new RScene(); }
void ref_scene_destroy(void* s) { delete (RScene*)s; }
void ref_scene_clear_meshes(void* s) { ((RScene*)s)->meshes.clear(); ((RScene*)s)->vel.clear(); }

void ref_scene_add_mesh(void* s, const uint32_t* tris, uint32_t ntris, const double* verts, uint32_t nverts,
                        const double* normals, uint32_t nnormals, double reflCoeff, double refrIndex, const double* vel)
{
    RScene* sc = (RScene*)s; RMesh m;
    m.tris.resize(ntris); for (uint32_t i = 0; i < ntris; i++) m.tris[i] = make_uint3(tris[3*i], tris[3*i+1], tris[3*i+2]);
    m.verts.resize(nverts); for (uint32_t i = 0; i < nverts; i++) m.verts[i] = make_double3(verts[3*i], verts[3*i+1], verts[3*i+2]);
    m.normals.resize(nnormals); for (uint32_t i = 0; i < nnormals; i++) m.normals[i] = make_double3(normals[3*i], normals[3*i+1], normals[3*i+2]);
    m.reflCoeff = reflCoeff; m.refrIndex = refrIndex;
    sc->meshes.push_back(std::move(m)); sc->vel.push_back(make_double3(vel[0], vel[1], vel[2]));
}

void ref_set_receivers(void* s, uint32_t n, const double* centre, const double* radius, const double* minTheta,
                       const double* maxTheta, const double* minPhi, const double* maxPhi)
{
    RScene* sc = (RScene*)s;
    sc->sphCentre.resize(n); sc->sphRadius.assign(radius, radius+n); sc->minTheta.assign(minTheta, minTheta+n);
    sc->maxTheta.assign(maxTheta, maxTheta+n); sc->minPhi.assign(minPhi, minPhi+n); sc->maxPhi.assign(maxPhi, maxPhi+n);
    for (uint32_t i = 0; i < n; i++) sc->sphCentre[i] = make_double3(centre[3*i], centre[3*i+1], centre[3*i+2]);
}

// rows per launch ray, as the host program sizes its buffers: 1 without refraction, maxRefl + 3 with
uint32_t ref_rows_per_ray(uint32_t maxRefl, uint32_t maxRefr) { return maxRefr == 2 ? (maxRefl + 1) + 1 + 1 : 1; }

// The arguments of orc_trace.  Only the full launch (ray_first = 0, ray_stride = 1, n_rays = W^3) exists in the reference;
// anything else returns 1.  use_bvh and n_threads are accepted and ignored (brute force, serial).
int ref_trace(void* s, const OPulse* p, uint64_t ray_first, uint64_t ray_stride, uint64_t n_rays, int use_bvh, int n_threads,
              PRD* results, int* targ_intersect, double* rcs_angle, int* hit_prim, float* hit_t, uint64_t* counters)
{
    (void)use_bvh; (void)n_threads;
    RScene* sc = (RScene*)s;
    const uint64_t W = p->width, W3 = W * W * W;
    if (ray_first != 0 || ray_stride != 1 || n_rays != W3 || W3 * ref_rows_per_ray(p->maxRefl, p->maxRefr) > 0xffffffffull) return 1;
    const unsigned D = p->maxRefr + p->maxRefl;
    const uint64_t rows = (uint64_t)ref_rows_per_ray(p->maxRefl, p->maxRefr) * W3;
    const unsigned hitCols = p->maxRefl + 1;
    // what the host program does before a launch: every output row reset, paths -1, angles -1e6
    for (uint64_t i = 0; i < rows; i++) {
        PRD& o = results[i]; memset(&o, 0, sizeof(o));
        o.refrIndex.x = 1; o.refrIndex.y = 1; o.received = -1; o.end = false;
    }
    for (uint64_t i = 0; i < rows * D; i++) { targ_intersect[i] = -1; rcs_angle[2*i] = -1000000; rcs_angle[2*i+1] = -1000000; }
    if (hit_prim) for (uint64_t i = 0; i < W3 * hitCols; i++) { hit_prim[i] = -2; hit_t[i] = 0.0f; }

    Launch L; memset(&L, 0, sizeof(L));
    L.sc = sc; L.smooth = p->interpolate_smooth != 0; L.hit_prim = hit_prim; L.hit_t = hit_t; L.hitCols = hitCols;
    g_launch = &L;

    const double3 origin = make_double3(p->rayOrigin[0], p->rayOrigin[1], p->rayOrigin[2]);
    // context variables of the ray generation and miss programs
    ref_rt::dbuf_results.bind(results, rows);
    ref_rt::dbuf_sphCentre.bind(sc->sphCentre.data(), sc->sphCentre.size());
    ref_rt::dbuf_sphRadius.bind(sc->sphRadius.data(), sc->sphRadius.size());
    ref_rt::dbuf_minTheta.bind(sc->minTheta.data(), sc->minTheta.size());
    ref_rt::dbuf_maxTheta.bind(sc->maxTheta.data(), sc->maxTheta.size());
    ref_rt::dbuf_minPhi.bind(sc->minPhi.data(), sc->minPhi.size());
    ref_rt::dbuf_maxPhi.bind(sc->maxPhi.data(), sc->maxPhi.size());
    ref_rt::d_width = (unsigned)W; ref_rt::d_rayOrigin = origin;
    ref_rt::d_txSpan = make_double3(p->txSpan[0], p->txSpan[1], p->txSpan[2]);
    ref_rt::d_txDir = make_double2(p->txDir[0], p->txDir[1]);
    ref_rt::d_rxsize = (unsigned)sc->sphCentre.size();
    ref_rt::d_maxRayTotal = (unsigned)rows;
    ref_rt::d_beamwidth_azi = 0; ref_rt::d_beamwidth_ele = 0;
    // context variables of the closest-hit program
    ref_ns::dbuf_results.bind((ref_ns::PerRayData*)results, rows);
    ref_ns::dbuf_targ_intersect.bind(targ_intersect, D, rows);
    ref_ns::dbuf_rcs_angle.bind((double2*)rcs_angle, D, rows);
    ref_ns::dbuf_targ_vel.bind(sc->vel.data(), sc->vel.size());
    ref_ns::d_rayOrigin = origin;
    ref_ns::d_maxReflDepth = p->maxRefl + 1; ref_ns::d_maxRefrDepth = p->maxRefr;
    ref_ns::d_width = (unsigned)W;

    for (unsigned z = 0; z < W; z++) for (unsigned y = 0; y < W; y++) for (unsigned x = 0; x < W; x++) {
        ref_rt::launchIndex = make_uint3(x, y, z); ref_ns::launchIndex = ref_rt::launchIndex;
        L.rayIndex = (uint64_t)z * W * W + (uint64_t)y * W + x;
        ref_rt::ray_generation();
    }
    if (counters) { counters[0] = 0; counters[1] = L.triTests; counters[2] = L.segments; counters[3] = L.shaded; }
    g_launch = nullptr;
    return 0;
}

// ---------------------------------------------------------------- the bound program on one triangle; returns validity
int ref_bound(const double* v0, const double* v1, const double* v2, float* out6)
{
    uint3 tri = make_uint3(0, 1, 2);
    double3 v[3] = { make_double3(v0[0], v0[1], v0[2]), make_double3(v1[0], v1[1], v1[2]), make_double3(v2[0], v2[1], v2[2]) };
    ref_tm::dbuf_triangles.bind(&tri, 1); ref_tm::dbuf_triVertices.bind(v, 3);
    ref_tm::bound(0, out6);
    return out6[0] <= out6[3] ? 1 : 0;               // an invalidated box has min > max
}
void ref_bound_n(uint64_t n, const double* v /* [n][3][3] */, float* out /* [n][6] */, int* valid)
{
    for (uint64_t i = 0; i < n; i++) valid[i] = ref_bound(v + 9*i, v + 9*i + 3, v + 9*i + 6, out + 6*i);
}

// ---------------------------------------------------------------- the intersection program on one ray and one triangle
// origin / dir: the payload's f64 prevHitPoint / rayDirection (what the triangle test reads); tmin / tmax: the ray's.
// normals [nnormals][3], nnormals >= 3; nnormals > 3 is the "more normals than vertices" rule.  Returns 1 on a reported hit.
int ref_intersect(const double* origin, const double* dir, float tmin, float tmax, const double* verts9, const double* normals,
                  uint32_t nnormals, int smooth, float* t_out, double* normal_out)
{
    RMesh m; m.tris.push_back(make_uint3(0, 1, 2));
    for (int k = 0; k < 3; k++) m.verts.push_back(make_double3(verts9[3*k], verts9[3*k+1], verts9[3*k+2]));
    for (uint32_t k = 0; k < nnormals; k++) m.normals.push_back(make_double3(normals[3*k], normals[3*k+1], normals[3*k+2]));
    bind_mesh(m, smooth != 0);
    memset(&ref_tm::prd, 0, sizeof(ref_tm::prd));
    ref_tm::prd.prevHitPoint = make_double3(origin[0], origin[1], origin[2]);
    ref_tm::prd.rayDirection = make_double3(dir[0], dir[1], dir[2]);
    ref_tm::ray = optix::make_Ray(make_float3((float)origin[0], (float)origin[1], (float)origin[2]),
                                  make_float3((float)dir[0], (float)dir[1], (float)dir[2]), 0, tmin, tmax);
    Trav tv; memset(&tv, 0, sizeof(tv)); tv.tmin = tmin; tv.tmax = tmax;
    Trav* const saved = g_trav; g_trav = &tv;
    ref_tm::intersect(0);
    g_trav = saved;
    *t_out = tv.found ? tv.t : 0.0f;
    normal_out[0] = tv.found ? tv.normal.x : 0.0; normal_out[1] = tv.found ? tv.normal.y : 0.0; normal_out[2] = tv.found ? tv.normal.z : 0.0;
    return tv.found ? 1 : 0;
}
void ref_intersect_n(uint64_t n, const double* origin, const double* dir, const float* tmin, const float* tmax, const double* verts9,
                     const double* normals /* [n][nnormals][3] */, uint32_t nnormals, int smooth, int* hit, float* t_out, double* normal_out)
{
    for (uint64_t i = 0; i < n; i++)
        hit[i] = ref_intersect(origin + 3*i, dir + 3*i, tmin[i], tmax[i], verts9 + 9*i, normals + 3*(size_t)nnormals*i, nnormals, smooth,
                               t_out + i, normal_out + 3*i);
}

// ---------------------------------------------------------------- the two aggregation kernels, launched serially
// launch shape as the reference's kernel_wrapper chooses it; shape_out[2] = (blocks, threads) if not NULL
void ref_aggregate(PRD* results_arr, int* targ_intersect_arr, unsigned receivedRays, unsigned depthTotal, unsigned MaxThreads,
                   unsigned MaxBlocks, double cspeed, double carrier, double* npath_arr, double* power_arr, double* doppler_arr,
                   double* delay_arr, double* phase_arr, int* pathMatch, unsigned* shape_out)
{
    unsigned blocks, threads;
    if (receivedRays <= MaxThreads) { blocks = 1; threads = receivedRays; }
    else if (receivedRays > MaxThreads * MaxBlocks) { blocks = MaxBlocks; threads = MaxThreads; }
    else { blocks = (receivedRays + (MaxThreads - 1)) / MaxThreads; threads = MaxThreads; }
    if (shape_out) { shape_out[0] = blocks; shape_out[1] = threads; }
    gridDim = dim3(); blockDim = dim3(); gridDim.x = blocks; blockDim.x = threads;
    blockIdx = make_uint3(0, 0, 0); threadIdx = make_uint3(0, 0, 0);
    ref_ag::PerRayData* res = (ref_ag::PerRayData*)results_arr;
    for (unsigned b = 0; b < blocks; b++) for (unsigned t = 0; t < threads; t++) {
        blockIdx.x = b; threadIdx.x = t;
        ref_ag::myKernel1(res, targ_intersect_arr, receivedRays, depthTotal, MaxThreads, MaxBlocks, npath_arr, power_arr, doppler_arr,
                          delay_arr, phase_arr, cspeed, carrier, pathMatch);
    }
    for (unsigned b = 0; b < blocks; b++) for (unsigned t = 0; t < threads; t++) {
        blockIdx.x = b; threadIdx.x = t;
        ref_ag::myKernel2(res, receivedRays, npath_arr, power_arr, doppler_arr, delay_arr, phase_arr);
    }
}

uint32_t ref_sizeof_prd() { return (uint32_t)sizeof(PRD); }

} // extern "C"
