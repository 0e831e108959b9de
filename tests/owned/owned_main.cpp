// Driver of tests/test_owned_host.py: rts_amd/csrc/rts_owned.h alone, built with a plain host compiler and linked WITHOUT the HIP
// runtime -- the ten calls the header makes are the stand-ins below, which log every call, keep the sets of live blocks and live
// events and can be told to fail their n-th call; the copy stand-in copies the bytes.  One case per line on stdin (a name, then unsigned integers), one line of tokens on stdout:
//   M:<id>:<bytes> F:<id>        hipMalloc / hipFree of block <id> (ids count allocations from 1 within the case)
//   HM:<id>:<bytes> HF:<id>      hipHostMalloc / hipHostFree
//   GP:<id>                      hipHostGetDevicePointer of block <id>
//   X:<call>                     a call that was told to fail;  BAD:<call> a free / query of an address that is not live
//   S:<id>:<cap>:<dev>           a buffer's state: the block p names (0: null), cap, dev (0 null, 1 the device address of p, 2 any other)
//   E:<code>                     what reserve returned (0: hipSuccess);  LIVE:<n> blocks still allocated when the case's scope has ended
//   EC:<id> ES:<id> ER:<id> ED:<id>   hipEventCreateWithFlags / hipEventSynchronize / hipEventRecord / hipEventDestroy of event <id> (events count
//                                from 1 within the case, apart from the blocks); LIVE counts live blocks and live events
//   CP:<dst id>:<src id>:<bytes> hipMemcpyAsync, host to device, on the case's stream
//   U:<pinned id>:<cap>:<device id>:<cap>:<event id>:<armed>    a StagedUpload's state;  W:<id> the driver fills pinned block <id>;
//   EQ:<0|1>                     after a send: the bytes at the device block equal the bytes the driver wrote to staging
// The expectations live in the test.
#include "rts_owned.h"
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <string>
#include <type_traits>
#include <utility>

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

// a struct that holds owners as members and in an array can be moved and never copied
struct Holder { DevBuf<int> a[3]; DevBuf<double> b; PinBuf<char> c; };
static_assert(!std::is_copy_constructible<Holder>::value && !std::is_copy_assignable<Holder>::value, "owners must not be copyable");
static_assert(!std::is_copy_constructible<DevBuf<char>>::value && !std::is_copy_assignable<PinBuf<char>>::value, "owners must not be copyable");
static_assert(std::is_nothrow_move_constructible<Holder>::value && std::is_nothrow_move_assignable<Holder>::value, "owners move");
static_assert(!std::is_copy_constructible<StagedUpload<double>>::value && !std::is_copy_assignable<StagedUpload<double>>::value, "owners must not be copyable");
static_assert(std::is_nothrow_move_constructible<StagedUpload<double>>::value && std::is_nothrow_move_assignable<StagedUpload<double>>::value, "owners move");

template <size_t N> struct Elem { char b[N]; };
static bool g_want_dev = false;
template <typename T> static hipError_t grow(DevBuf<T>& b, size_t n) { return b.reserve(n); }
template <typename T> static hipError_t grow(PinBuf<T>& b, size_t n) { return b.reserve(n, g_want_dev); }
static int id_of(void* p) { if (!p) return 0; auto it = g_live.find(p); return it == g_live.end() ? -1 : it->second; }
template <typename T> static void state(const DevBuf<T>& b) { char s[64]; snprintf(s, sizeof(s), "S:%d:%zu:0 ", id_of(b.p), b.cap); g_log += s; }
template <typename T> static void state(const PinBuf<T>& b)
{
    char s[64]; snprintf(s, sizeof(s), "S:%d:%zu:%d ", id_of(b.p), b.cap, !b.dev ? 0 : ((void*)b.dev == dev_address(b.p) ? 1 : 2)); g_log += s;
}
template <typename B> static void assign(B& to, B& from) { to = std::move(from); }      // (a plain `b = std::move(b)` is a compiler warning)

// v[0 ..]: the case's numbers after the element size
template <typename B> static void run(const char* name, const unsigned long long* v, int n)
{
    if (!strcmp(name, "grow")) {                   // reserve(v[0]), reserve(v[1]), ...: state after each, then the scope ends
        B b; for (int i = 0; i < n; i++) { logf("E", (long long)grow(b, (size_t)v[i])); state(b); }
    } else if (!strcmp(name, "release")) {         // reserve(v[0]), release twice, reserve(v[1]), release twice
        B b; (void)grow(b, (size_t)v[0]); b.release(); state(b); b.release(); state(b); (void)grow(b, (size_t)v[1]); state(b); b.release(); b.release(); state(b);
    } else if (!strcmp(name, "fail")) {            // allocation number v[0] (and device-address query number v[1]) fails during reserve(v[2]), reserve(v[3]), ...
        B b; g_fail_alloc = (int)v[0]; g_fail_getptr = (int)v[1];
        for (int i = 2; i < n; i++) { logf("E", (long long)grow(b, (size_t)v[i]) != 0); state(b); }
    } else if (!strcmp(name, "movector")) {        // a(v[0]); B b(std::move(a))
        B a; (void)grow(a, (size_t)v[0]); B b(std::move(a)); state(a); state(b);
    } else if (!strcmp(name, "moveassign")) {      // a(v[0]), b(v[1]); b = std::move(a); then a is used again with v[2]
        B a, b; (void)grow(a, (size_t)v[0]); (void)grow(b, (size_t)v[1]); g_log += "| "; assign(b, a); state(a); state(b); (void)grow(a, (size_t)v[2]); state(a);
    } else if (!strcmp(name, "selfmove")) {
        B a; (void)grow(a, (size_t)v[0]); g_log += "| "; assign(a, a); state(a);
    } else if (!strcmp(name, "holder")) {          // owners in an array and as members, moved as a whole
        Holder h; (void)h.a[0].reserve((size_t)v[0]); (void)h.a[2].reserve((size_t)v[0]); (void)h.b.reserve((size_t)v[0]); (void)h.c.reserve((size_t)v[0], true);
        g_log += "| "; Holder k(std::move(h)); state(h.a[0]); state(h.c); state(k.a[0]); state(k.a[1]); state(k.c);
    } else g_log += "BAD:case ";
}

// ---- StagedUpload<double>.  A step is four numbers: begin(need, grow_to, dev_need), then -- when n != 0 -- the driver fills n elements
// of the staging with values of its own and calls send(n)
typedef StagedUpload<double> Staged;
static int event_id(hipEvent_t e) { if (!e) return 0; auto it = g_events.find((void*)e); return it == g_events.end() ? -1 : it->second; }
static void state(const Staged& u)
{
    char s[96]; snprintf(s, sizeof(s), "U:%d:%zu:%d:%zu:%d:%d ", id_of(u.pin.p), u.pin.cap, id_of(u.dev.p), u.dev.cap, event_id(u.ev), (int)u.armed); g_log += s;
}
static void step(Staged& u, const unsigned long long* q, double salt)
{
    double* h = nullptr;
    const hipError_t e = u.begin((size_t)q[0], (size_t)q[1], (size_t)q[2], &h);
    logf("E", (long long)(e != hipSuccess)); state(u);
    const size_t n = (size_t)q[3];
    if (e != hipSuccess || n == 0) return;
    if (h != u.pin.p) g_log += "BAD:host ";
    logf("W", id_of(h)); for (size_t i = 0; i < n; i++) h[i] = salt + (double)i;
    logf("E", (long long)(u.send(n, g_stream) != hipSuccess));
    bool eq = true; for (size_t i = 0; i < n; i++) eq = eq && u.dev.p[i] == salt + (double)i;      // (the stand-in's device block is host memory)
    logf("EQ", eq ? 1 : 0); state(u);
}
static void run_staged(const char* name, const unsigned long long* v, int n)
{
    if (!strcmp(name, "steps")) {                  // allocation number v[0] and event creation number v[1] fail (0: none); then the steps; then the scope ends
        Staged u; g_fail_alloc = (int)v[0]; g_fail_event = (int)v[1];
        for (int i = 2; i + 4 <= n; i += 4) step(u, v + i, 100.0 * i);
        g_log += "| ";
    } else if (!strcmp(name, "movector")) {        // a does the step; Staged b(std::move(a)); b does the same step again
        Staged a; step(a, v, 1.0); g_log += "| "; Staged b(std::move(a)); state(a); state(b); step(b, v, 2.0); g_log += "| ";
    } else if (!strcmp(name, "moveassign")) {      // a and b do a step each; b = std::move(a); a is used again
        Staged a, b; step(a, v, 1.0); step(b, v + 4, 2.0); g_log += "| "; assign(b, a); state(a); state(b); step(a, v, 3.0); g_log += "| ";
    } else if (!strcmp(name, "selfmove")) {
        Staged a; step(a, v, 1.0); g_log += "| "; assign(a, a); state(a); g_log += "| ";
    } else g_log += "BAD:case ";
}

int main()
{
    char name[32], kind[32]; char line[1024];
    while (fgets(line, sizeof(line), stdin)) {
        unsigned long long v[14] = {0}; int used = 0;
        if (sscanf(line, "%31s %31s%n", name, kind, &used) != 2) continue;
        int n = 0; for (const char* s = line + used; n < 14; n++) { int k = 0; if (sscanf(s, "%llu%n", &v[n], &k) != 1) break; s += k; }
        g_log.clear(); g_live.clear(); g_bytes.clear(); g_events.clear(); g_next_id = g_next_event = 1; g_fail_alloc = g_fail_getptr = g_fail_event = 0; g_want_dev = !strcmp(kind, "pindev");
        const bool pin = !strncmp(kind, "pin", 3);
        if (n < 1) { fprintf(stderr, "bad case: %s", line); return 2; }
        if (!strcmp(kind, "staged")) run_staged(name, v, n);
        else switch (v[0]) {                        // element size
        case 1: if (pin) run<PinBuf<Elem<1>>>(name, v + 1, n - 1); else run<DevBuf<Elem<1>>>(name, v + 1, n - 1); break;
        case 8: if (pin) run<PinBuf<Elem<8>>>(name, v + 1, n - 1); else run<DevBuf<Elem<8>>>(name, v + 1, n - 1); break;
        case 144: if (pin) run<PinBuf<Elem<144>>>(name, v + 1, n - 1); else run<DevBuf<Elem<144>>>(name, v + 1, n - 1); break;
        case 145: if (pin) run<PinBuf<Elem<145>>>(name, v + 1, n - 1); else run<DevBuf<Elem<145>>>(name, v + 1, n - 1); break;
        default: fprintf(stderr, "bad element size: %s", line); return 2;
        }
        printf("%sLIVE:%zu\n", g_log.c_str(), g_live.size() + g_events.size());
        for (auto& kv : g_live) free(kv.first);
        for (auto& kv : g_events) free(kv.first);
    }
    return 0;
}
