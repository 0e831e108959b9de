// fake_hip.h -- stand-ins for the HIP calls that rts_amd/csrc/rts_owned.h makes, for host drivers that are built with a plain host compiler and linked
// WITHOUT the HIP runtime (tests/owned/owned_main.cpp, tests/cube_state/cube_state_main.cpp).  They log every call to g_log, keep the sets of live
// blocks and live events and can be told to fail their n-th call; the copy stand-in copies the bytes.  The tokens (ids count from 1 within a case):
//   M:<id>:<bytes> F:<id>        hipMalloc / hipFree of block <id>
//   HM:<id>:<bytes> HF:<id>      hipHostMalloc / hipHostFree
//   GP:<id>                      hipHostGetDevicePointer of block <id>
//   X:<call>                     a call that was told to fail;  BAD:<call> a free / query of an address that is not live
//   EC:<id> ES:<id> ER:<id> ED:<id>   hipEventCreateWithFlags / hipEventSynchronize / hipEventRecord / hipEventDestroy of event <id> (counted apart from the blocks)
//   CP:<dst id>:<src id>:<bytes> hipMemcpyAsync, host to device, on the case's stream (g_stream)
// One translation unit per program includes this header; fake_reset() starts a case.
#pragma once
#include <hip/hip_runtime_api.h>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <string>

static std::map<void*, int> g_live;      // address -> id
static std::map<void*, size_t> g_bytes;  // address -> size of the block
static std::map<void*, int> g_events;    // live events -> id
static int g_next_id = 1, g_next_event = 1;
static int g_fail_alloc = 0, g_fail_getptr = 0, g_fail_event = 0;      // fail the n-th allocation / device-address query / event creation from now (0: never)
static const hipStream_t g_stream = (hipStream_t)(void*)&g_next_id;    // the case's stream: never dereferenced
static std::string g_log;
static void logf(const char* tag, long long a, long long b = -1)
{
    char s[64]; if (b >= 0) snprintf(s, sizeof(s), "%s:%lld:%lld ", tag, a, b); else snprintf(s, sizeof(s), "%s:%lld ", tag, a);
    g_log += s;
}
static hipError_t fake_alloc(const char* tag, void** p, size_t bytes)
{
    if (g_fail_alloc && --g_fail_alloc == 0) { g_log += std::string("X:") + tag + " "; return hipErrorOutOfMemory; }      // (*p untouched)
    *p = malloc(bytes ? bytes : 1);
    g_live[*p] = g_next_id; g_bytes[*p] = bytes; logf(tag, g_next_id++, (long long)bytes);
    return hipSuccess;
}
static hipError_t fake_free(const char* tag, void* p)
{
    auto it = g_live.find(p);
    if (it == g_live.end()) { g_log += std::string("BAD:") + tag + " "; return hipErrorInvalidValue; }      // a second free of one address lands here
    logf(tag, it->second); g_live.erase(it); g_bytes.erase(p); free(p);
    return hipSuccess;
}
static void* dev_address(void* host) { return (char*)host + 1; }      // never dereferenced
extern "C" {
hipError_t hipMalloc(void** p, size_t bytes) { return fake_alloc("M", p, bytes); }
hipError_t hipFree(void* p) { return fake_free("F", p); }
hipError_t hipHostMalloc(void** p, size_t bytes, unsigned int flags) { if (flags != hipHostMallocDefault) g_log += "BAD:flags "; return fake_alloc("HM", p, bytes); }
hipError_t hipHostFree(void* p) { return fake_free("HF", p); }
hipError_t hipHostGetDevicePointer(void** dev, void* host, unsigned int flags)
{
    auto it = g_live.find(host);
    if (it == g_live.end() || flags != 0) { g_log += "BAD:GP "; return hipErrorInvalidValue; }
    if (g_fail_getptr && --g_fail_getptr == 0) { g_log += "X:GP "; return hipErrorInvalidValue; }
    logf("GP", it->second); *dev = dev_address(host);
    return hipSuccess;
}
hipError_t hipEventCreateWithFlags(hipEvent_t* e, unsigned flags)
{
    if (flags != hipEventDisableTiming) g_log += "BAD:flags ";
    if (g_fail_event && --g_fail_event == 0) { g_log += "X:EC "; return hipErrorOutOfMemory; }      // (*e untouched)
    *e = (hipEvent_t)malloc(1); g_events[(void*)*e] = g_next_event; logf("EC", g_next_event++);
    return hipSuccess;
}
static hipError_t event_call(const char* tag, hipEvent_t e)
{
    auto it = g_events.find((void*)e);
    if (it == g_events.end()) { g_log += std::string("BAD:") + tag + " "; return hipErrorInvalidHandle; }      // a null, dead or twice destroyed event
    logf(tag, it->second);
    return hipSuccess;
}
hipError_t hipEventSynchronize(hipEvent_t e) { return event_call("ES", e); }
hipError_t hipEventRecord(hipEvent_t e, hipStream_t s) { if (s != g_stream) g_log += "BAD:stream "; return event_call("ER", e); }
hipError_t hipEventDestroy(hipEvent_t e)
{
    const hipError_t r = event_call("ED", e);
    if (r == hipSuccess) { g_events.erase((void*)e); free((void*)e); }
    return r;
}
hipError_t hipMemcpyAsync(void* dst, const void* src, size_t bytes, hipMemcpyKind kind, hipStream_t s)
{
    auto d = g_live.find(dst), f = g_live.find(const_cast<void*>(src));
    if (d == g_live.end() || f == g_live.end() || kind != hipMemcpyHostToDevice || s != g_stream || bytes > g_bytes[d->first] || bytes > g_bytes[f->first]) { g_log += "BAD:CP "; return hipErrorInvalidValue; }
    char t[96]; snprintf(t, sizeof(t), "CP:%d:%d:%zu ", d->second, f->second, bytes); g_log += t;
    memcpy(dst, src, bytes);
    return hipSuccess;
}
}
static void fake_reset() { g_log.clear(); g_live.clear(); g_bytes.clear(); g_events.clear(); g_next_id = g_next_event = 1; g_fail_alloc = g_fail_getptr = g_fail_event = 0; }
// what a case leaves behind (blocks + events), then the stand-ins' own memory is given back
static size_t fake_live() { return g_live.size() + g_events.size(); }
static void fake_sweep() { for (auto& kv : g_live) free(kv.first); for (auto& kv : g_events) free(kv.first); }
