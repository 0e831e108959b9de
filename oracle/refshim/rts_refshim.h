// =====================================================================================
// rts_refshim.h -- host stand-ins for the device API the reference's programs are written
// against (legacy OptiX rt* device API, CUDA vector types).  TEST INFRASTRUCTURE ONLY.
//
// With this directory on the include path the reference's device sources (triangle_mesh.cu,
// normal_shader.cu, ray_tracer.cu and the two kernels of aggregation.cu) compile UNMODIFIED as
// host C++17; ref_harness.cpp includes them and drives them.  Everything here is this
// project's own text, written from the published semantics DESIGN.md section 2 lists:
//   reflect(i, n)          = i - 2*n*dot(n, i)                                       (f32)
//   refract(r, i, n, ior)  : the sign of dot(i, n) picks eta = ior or 1/ior, total internal
//                            reflection gives r = 0 and false, else a normalised r    (f32)
//   normalize(v)           = v * (1 / sqrtf(dot(v, v)))                               (f32)
//   RT_DEFAULT_MAX         = 1e27f
//   rtPotentialIntersection(t) <=> tmin < t < current tmax, t narrowed to f32
//   optix::Aabb::invalidate(): min = +1e37f, max = -1e37f
// What is NOT here and stays restated, not pinned: the OptiX traversal (rtTrace is the brute
// force of ref_harness.cpp), CUDA's libm bits, the reference's host program.
// =====================================================================================
#ifndef RTS_REFSHIM_H
#define RTS_REFSHIM_H

#include <cfenv>
#include <cstddef>
#include <cstdio>
#include <cstdlib>
#include <math.h>      // the global ::sqrt, ::fabs, ::isinf ... the device code calls unqualified

// ------------------------------------------------------------------ function and program qualifiers
#define __device__
#define __global__
#define __host__
#define RT_PROGRAM
#define rtPrintf(...) ((void)0)
#define RT_DEFAULT_MAX 1e27f

// ------------------------------------------------------------------ CUDA vector types
struct float3 { float x, y, z; };
struct double2 { double x, y; } __attribute__((aligned(16)));
struct double3 { double x, y, z; };
struct uint2 { unsigned int x, y; };
struct uint3 { unsigned int x, y, z; };
struct dim3 { unsigned int x = 1, y = 1, z = 1; };

static inline float3 make_float3(float x, float y, float z) { float3 o; o.x = x; o.y = y; o.z = z; return o; }
static inline float3 make_float3(float s) { return make_float3(s, s, s); }
static inline double2 make_double2(double x, double y) { double2 o; o.x = x; o.y = y; return o; }
static inline double3 make_double3(double x, double y, double z) { double3 o; o.x = x; o.y = y; o.z = z; return o; }
static inline uint2 make_uint2(unsigned int x, unsigned int y) { uint2 o; o.x = x; o.y = y; return o; }
static inline uint3 make_uint3(unsigned int x, unsigned int y, unsigned int z) { uint3 o; o.x = x; o.y = y; o.z = z; return o; }

// kernel launch coordinates: set by the serial loop of ref_aggregate
extern uint3 threadIdx, blockIdx;
extern dim3 blockDim, gridDim;

// ------------------------------------------------------------------ directed f64 -> f32 conversions
// One conversion under the directed rounding mode; volatile keeps it where the mode is set.
static inline float refshim_d2f(double v, int mode)
{
    const int old = fegetround();
    fesetround(mode);
    volatile double in = v;
    volatile float out = (float)in;
    fesetround(old);
    return out;
}
static inline float __double2float_rd(double v) { return refshim_d2f(v, FE_DOWNWARD); }
static inline float __double2float_ru(double v) { return refshim_d2f(v, FE_UPWARD); }

// ------------------------------------------------------------------ namespace optix: Ray, Aabb, f32 vector maths
namespace optix {

struct Ray {
    float3 origin; float3 direction; unsigned int ray_type; float tmin; float tmax;
};
static inline Ray make_Ray(float3 origin, float3 direction, unsigned int ray_type, float tmin, float tmax)
{
    Ray r; r.origin = origin; r.direction = direction; r.ray_type = ray_type; r.tmin = tmin; r.tmax = tmax; return r;
}

struct Aabb {
    float3 m_min, m_max;
    void invalidate() { m_min = make_float3(1e37f); m_max = make_float3(-1e37f); }
};
static_assert(sizeof(Aabb) == 6 * sizeof(float), "a bound program's float[6] is read as an Aabb");

static inline float3 operator-(float3 a) { return make_float3(-a.x, -a.y, -a.z); }
static inline float3 operator-(float3 a, float3 b) { return make_float3(a.x - b.x, a.y - b.y, a.z - b.z); }
static inline float3 operator*(float3 a, float s) { return make_float3(a.x * s, a.y * s, a.z * s); }
static inline float3 operator*(float s, float3 a) { return make_float3(s * a.x, s * a.y, s * a.z); }
static inline float dot(float3 a, float3 b) { return a.x * b.x + a.y * b.y + a.z * b.z; }
static inline float3 normalize(float3 v) { const float invLen = 1.0f / sqrtf(dot(v, v)); return v * invLen; }
static inline float3 reflect(float3 i, float3 n) { return i - 2.0f * n * dot(n, i); }
static inline bool refract(float3& r, float3 i, float3 n, float ior)
{
    float3 nn = n;
    float negNdotV = dot(i, nn);
    float eta;
    if (negNdotV > 0.0f) { eta = ior; nn = -n; negNdotV = -negNdotV; }
    else { eta = 1.f / ior; }
    const float k = 1.f - eta * eta * (1.f - negNdotV * negNdotV);
    if (k < 0.0f) { r = make_float3(0.f); return false; }
    r = normalize(eta * i - (eta * negNdotV + sqrtf(k)) * nn);
    return true;
}

} // namespace optix

// ------------------------------------------------------------------ variables and buffers of the rt* API
// A declared variable is a plain variable of the namespace the program is included into; the
// harness sets it before it runs the program (semantic and annotation are dropped).
#define rtDeclareVariable(type, name, semantic, annotation) type name

struct rtObject { int unused; };

// rtBuffer<T, 1|2>: a non-owning view of an array the harness holds; [size_t] for one
// dimension, [uint2] (x = column, y = row) for two.  An index outside the buffer ends the run.
template <class T, int N> class rtBuffer {
    T* p_ = nullptr; size_t w_ = 0, h_ = 0;
    T& at(size_t i) const
    {
        if (i >= w_ * h_) { fprintf(stderr, "refshim: rtBuffer index %zu outside %zu x %zu\n", i, w_, h_); abort(); }
        return p_[i];
    }
public:
    void bind(T* p, size_t w, size_t h = 1) { p_ = p; w_ = w; h_ = h; }
    size_t size() const { return w_ * h_; }
    T& operator[](size_t i) const { static_assert(N == 1, "one index needs a 1-D buffer"); return at(i); }
    T& operator[](uint2 i) const
    {
        static_assert(N == 2, "a uint2 index needs a 2-D buffer");
        if (i.x >= w_) { fprintf(stderr, "refshim: rtBuffer column %u outside width %zu\n", i.x, w_); abort(); }
        return at((size_t)i.y * w_ + i.x);
    }
};

// ------------------------------------------------------------------ rt* device calls, served by ref_harness.cpp
bool rtPotentialIntersection(float t);
bool rtReportIntersection(unsigned int material);
void refshim_trace(const optix::Ray& ray, void* payload, size_t payload_size);
template <class P> static inline void rtTrace(rtObject, optix::Ray ray, P& payload) { refshim_trace(ray, &payload, sizeof(P)); }

#endif
