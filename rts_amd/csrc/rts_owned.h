// rts_owned.h -- the owning types of librts_amd.so: device memory (DevBuf), pinned host memory (PinBuf), and the pair of them
// behind an event that a small asynchronous upload goes through (StagedUpload).
//
// All free what they hold in their destructor and are move-only, so a struct that holds them (RtsContext, RtsScene,
// RtsTileHist, a function's temporaries) needs no release list of its own: `delete` or leaving the scope frees the buffers,
// members in reverse order of declaration.  hipFree waits for the device, so a buffer an enqueued kernel still reads is not
// freed under it; hipHostFree does not say so: the owner of a PinBuf synchronises the stream that reads it first.
//
// NO OBJECT OF THESE TYPES MAY HAVE STATIC STORAGE DURATION (nor a struct that holds one): its destructor would call HIP after
// the runtime has shut down.  The library has none; process-lifetime contexts are held by pointer and never deleted.
//
// Host code only, HIP's API header and the standard library only (tests/owned/owned_main.cpp builds it without the runtime).
#pragma once
#include <hip/hip_runtime_api.h>
#include <stddef.h>
#include <string.h>
#include <utility>

template <typename T> struct DevBuf {
    T* p = nullptr; size_t cap = 0;
    DevBuf() = default;
    DevBuf(const DevBuf&) = delete;
    DevBuf& operator=(const DevBuf&) = delete;
    DevBuf(DevBuf&& o) noexcept : p(o.p), cap(o.cap) { o.p = nullptr; o.cap = 0; }
    DevBuf& operator=(DevBuf&& o) noexcept { if (this != &o) { release(); p = o.p; cap = o.cap; o.p = nullptr; o.cap = 0; } return *this; }
    ~DevBuf() { release(); }
    hipError_t reserve(size_t n) {
        if (n <= cap) return hipSuccess;
        // hipFree is a device-wide synchronisation (it stalls the other handles' launches): grow geometrically, and give
        // the many small buffers sized by a pulse's received-ray count room to begin with
        size_t want = n + n / 8 + 16;
        if (want < 2 * cap) want = 2 * cap;
        if (sizeof(T) <= 144 && want < 65536) want = 65536;
        if (p) { (void)hipFree(p); p = nullptr; cap = 0; }
        hipError_t e = hipMalloc((void**)&p, want * sizeof(T));
        if (e == hipSuccess) cap = want;
        return e;
    }
    void release() { if (p) (void)hipFree(p); p = nullptr; cap = 0; }
};

// Pinned host staging (hipHostMalloc).  cap elements at p; dev: the same block as kernels address it, fetched only for the
// buffers that kernels write or read in place (want_dev, the same at every call for one buffer).  The caller chooses the size
// (no growth rule here: each staging block has its own) and, before a regrow, synchronises whatever stream may still read
// the old block.
template <typename T> struct PinBuf {
    T* p = nullptr; T* dev = nullptr; size_t cap = 0;
    PinBuf() = default;
    PinBuf(const PinBuf&) = delete;
    PinBuf& operator=(const PinBuf&) = delete;
    PinBuf(PinBuf&& o) noexcept : p(o.p), dev(o.dev), cap(o.cap) { o.p = nullptr; o.dev = nullptr; o.cap = 0; }
    PinBuf& operator=(PinBuf&& o) noexcept { if (this != &o) { release(); p = o.p; dev = o.dev; cap = o.cap; o.p = nullptr; o.dev = nullptr; o.cap = 0; } return *this; }
    ~PinBuf() { release(); }
    hipError_t reserve(size_t n, bool want_dev) {
        if (n <= cap) return hipSuccess;
        release();
        hipError_t e = hipHostMalloc((void**)&p, n * sizeof(T), hipHostMallocDefault);
        if (e != hipSuccess) { p = nullptr; return e; }
        if (want_dev) {
            void* dp = nullptr; e = hipHostGetDevicePointer(&dp, p, 0);
            if (e != hipSuccess) { release(); return e; }
            dev = static_cast<T*>(dp);
        }
        cap = n;
        return hipSuccess;
    }
    void release() { if (p) (void)hipHostFree(p); p = nullptr; dev = nullptr; cap = 0; }
};

// A small per-call upload that must not drain the stream: the caller's values -> a pinned staging block -> a device buffer, by an
// asynchronous copy on the stream whose later kernels read them.  The staging is rewritten only once the previous copy out of it
// has run (the event): the handle's earlier calls may still be in flight.
//   T* h; begin(need, grow_to, dev_need, &h);  fill h[0 .. n);  send(n, stream);  kernels on `stream` read dev.p
// begin waits for the previous send, makes room -- the pinned block is replaced by one of grow_to elements when it holds fewer than
// `need` (each site brings its own sizes, as with PinBuf), the device buffer holds dev_need -- and creates the event on first use.
// A begin without a send is allowed (nothing to upload this time).  The destructor destroys the event, then the members free
// themselves; like a PinBuf's owner, whoever destroys or move-assigns over a StagedUpload drains the stream it was sent on first.
template <typename T> struct StagedUpload {
    PinBuf<T> pin; DevBuf<T> dev; hipEvent_t ev = nullptr; bool armed = false;
    StagedUpload() = default;
    StagedUpload(const StagedUpload&) = delete;
    StagedUpload& operator=(const StagedUpload&) = delete;
    StagedUpload(StagedUpload&& o) noexcept : pin(std::move(o.pin)), dev(std::move(o.dev)), ev(o.ev), armed(o.armed) { o.ev = nullptr; o.armed = false; }
    StagedUpload& operator=(StagedUpload&& o) noexcept
    {
        if (this != &o) { drop_event(); pin = std::move(o.pin); dev = std::move(o.dev); ev = o.ev; armed = o.armed; o.ev = nullptr; o.armed = false; }
        return *this;
    }
    ~StagedUpload() { drop_event(); }
    hipError_t begin(size_t need, size_t grow_to, size_t dev_need, T** host)
    {
        hipError_t e;
        if (armed) { e = hipEventSynchronize(ev); if (e != hipSuccess) return e; armed = false; }
        if (pin.cap < need) { e = pin.reserve(grow_to, false); if (e != hipSuccess) return e; }
        if (!ev) { e = hipEventCreateWithFlags(&ev, hipEventDisableTiming); if (e != hipSuccess) { ev = nullptr; return e; } }
        e = dev.reserve(dev_need); if (e != hipSuccess) return e;
        *host = pin.p;
        return hipSuccess;
    }
    hipError_t send(size_t n, hipStream_t s)
    {
        hipError_t e = hipMemcpyAsync(dev.p, pin.p, n * sizeof(T), hipMemcpyHostToDevice, s); if (e != hipSuccess) return e;
        e = hipEventRecord(ev, s); if (e != hipSuccess) return e;
        armed = true;
        return hipSuccess;
    }
    // one array of n <= capacity elements, for the sites whose staging and device buffer have one size for every call
    hipError_t upload(const T* src, size_t n, size_t capacity, hipStream_t s)
    {
        T* h = nullptr;
        const hipError_t e = begin(capacity, capacity, capacity, &h); if (e != hipSuccess) return e;
        memcpy(h, src, n * sizeof(T));
        return send(n, s);
    }
    void drop_event() { if (ev) (void)hipEventDestroy(ev); ev = nullptr; armed = false; }
};
