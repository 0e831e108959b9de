// Driver of tests/test_owned_host.py: rts_amd/csrc/rts_owned.h alone, built with a plain host compiler and linked WITHOUT the HIP
// runtime -- the ten calls the header makes are the stand-ins of fake_hip.h, which log every call, keep the sets of live blocks and live
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
#include "fake_hip.h"
#include <type_traits>
#include <utility>

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
        fake_reset(); g_want_dev = !strcmp(kind, "pindev");
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
        printf("%sLIVE:%zu\n", g_log.c_str(), fake_live());
        fake_sweep();
    }
    return 0;
}
