// Driver of tests/test_cube_state_host.py: rts_amd/csrc/rts_cube_state.h alone, built with a plain host compiler and linked WITHOUT the
// HIP runtime, on the stand-ins of tests/owned/fake_hip.h (whose tokens M: F: HM: HF: EC: ED: X: BAD: are described there).  No input;
// every case prints lines that begin with its name.  Its own tokens:
//   R:<p>:<doubles>:<valid>      a RtsCubeProduct's record; p: 0 null, 1 the product's own block, 2 the caller's pointer, 3 anything else
//   O:<p>                        what place() handed back through `out`, coded like p;  E:<0|1> whether it returned an error
//   C:<cap>                      the capacity of the product's own block;  LIVE:<n> blocks and events still alive after the case's scope
//   end_products prints one line `end_products product <name> <valid before> <valid after>` per RtsCubeProduct of RtsCubeState, one
//   `end_products list <name> <before> <after>` per counted list, and `end_products kept <0|1> ...`: what must not change, did not
// The expectations live in the test.
#include "rts_cube_state.h"
#include "../owned/fake_hip.h"
#include <type_traits>
#include <utility>

static_assert(!std::is_copy_constructible<RtsCubeState>::value && !std::is_copy_assignable<RtsCubeState>::value, "the cube state owns memory: no copies");
static_assert(std::is_nothrow_move_constructible<RtsCubeProduct>::value, "a product moves");

static double g_caller[4];      // "the caller's device memory": never dereferenced
static int code(const RtsCubeProduct& r, const double* p) { return !p ? 0 : p == r.own.p ? 1 : p == g_caller ? 2 : 3; }
static void rec(const RtsCubeProduct& r) { char s[64]; snprintf(s, sizeof(s), "R:%d:%zu:%d ", code(r, r.p), r.doubles, (int)r.valid); g_log += s; }
static void cap(const RtsCubeProduct& r) { char s[48]; snprintf(s, sizeof(s), "C:%zu ", r.own.cap); g_log += s; }
static void place(RtsCubeProduct& r, void* device_out, size_t n)
{
    double* out = (double*)(void*)&g_log;      // (anything but a value place() may hand back)
    const hipError_t e = r.place(device_out, n, &out);
    char s[32]; snprintf(s, sizeof(s), "E:%d O:%d ", (int)(e != hipSuccess), code(r, out)); g_log += s;
}
static void flush(const char* name) { printf("%s %s\n", name, g_log.c_str()); g_log.clear(); }
static void done(const char* name) { char s[32]; snprintf(s, sizeof(s), "LIVE:%zu", fake_live()); g_log += s; flush(name); fake_sweep(); }

// a library-owned product of 10 doubles, recorded: what the cases below start from
static void owned10(RtsCubeProduct& r) { double* out = nullptr; (void)r.place(nullptr, 10, &out); r.record(out, 10); g_log += "| "; }

static void product_cases()
{
    fake_reset();
    { RtsCubeProduct r; place(r, g_caller, 100); rec(r); cap(r); g_log += "| "; owned10(r); place(r, g_caller, 1u << 20); rec(r); cap(r); }      // a caller's pointer: never an allocation, the record untouched
    done("caller");
    fake_reset();
    { RtsCubeProduct r; owned10(r); cap(r); place(r, nullptr, 3); rec(r); place(r, nullptr, r.own.cap); rec(r); cap(r); }      // n <= own.cap, up to the capacity itself
    done("fits");
    fake_reset();
    { RtsCubeProduct r; owned10(r); g_fail_alloc = 1; place(r, nullptr, r.own.cap + 1); rec(r); cap(r); }      // the regrow's allocation fails: the old block is gone, and so is the record
    done("regrow_fails");
    fake_reset();
    { RtsCubeProduct r; owned10(r); const size_t n = r.own.cap + 1; place(r, nullptr, n); rec(r); r.record(r.own.p, n); rec(r); }      // ended until record()
    done("regrow");
    fake_reset();
    { RtsCubeProduct r; rec(r); r.record(g_caller, 7); rec(r); }      // record() alone: a caller-owned Doppler map
    done("record");
}

static void line(const char* kind, const char* name, bool before, bool after) { printf("end_products %s %s %d %d\n", kind, name, (int)before, (int)after); }
static void end_products_case()
{
    fake_reset();
    {
        RtsCubeState s;
        RtsCubeProduct* prod[] = {&s.doppler.map, &s.image.out, &s.stft.out, &s.fmcw.range, &s.beam.out, &s.adapt.cov, &s.adapt.mvdr, &s.stap.out,
                                  &s.doa.eig_val, &s.doa.eig_vec, &s.doa.spectrum, &s.focus.align, &s.focus.pga};
        const char* names[] = {"doppler.map", "image.out", "stft.out", "fmcw.range", "beam.out", "adapt.cov", "adapt.mvdr", "stap.out",
                               "doa.eig_val", "doa.eig_vec", "doa.spectrum", "focus.align", "focus.pga"};
        const int n = (int)(sizeof(prod) / sizeof(prod[0]));
        for (int i = 0; i < n; i++) prod[i]->record(g_caller, 4);
        s.set = true; s.params.n_rx = 3; s.params.n_pulses = 8; s.params.n_bins = 16; s.p = g_caller;
        s.detect.valid = true; s.plot.valid = true; s.plot.own_list = true;
        s.track.live = true; s.track.time = 2.5; s.track.cur = 1; s.track.max = 64;
        s.tbd.frames = 3; s.tbd.rx = 3; s.tbd.nd = 8; s.tbd.nb = 16; s.tbd.depth = 4; s.tbd.ext_valid = true;
        s.wave.set = true; s.wave.M = 5; s.wave.L = 2;
        s.detect.os_tab.assign(7, 1.5); s.detect.os_key[0] = 1; s.detect.os_key[4] = 9; s.detect.os_pfa = 1e-3; s.detect.os_sent = true;
        bool before[16]; for (int i = 0; i < n; i++) before[i] = prod[i]->valid;
        const bool det = s.detect.valid, plot = s.plot.valid;
        s.end_products();
        for (int i = 0; i < n; i++) line("product", names[i], before[i], prod[i]->valid);
        line("list", "detect", det, s.detect.valid); line("list", "plot", plot, s.plot.valid);
        printf("end_products kept %d %d %d %d %d %d\n",
               (int)(s.set && s.p == g_caller && s.params.n_rx == 3 && s.params.n_pulses == 8 && s.params.n_bins == 16),
               (int)(s.wave.set && s.wave.M == 5 && s.wave.L == 2),
               (int)(s.track.live && s.track.time == 2.5 && s.track.cur == 1 && s.track.max == 64),
               (int)(s.tbd.frames == 3 && s.tbd.rx == 3 && s.tbd.nd == 8 && s.tbd.nb == 16 && s.tbd.depth == 4 && s.tbd.ext_valid),
               (int)(s.detect.os_tab.size() == 7 && s.detect.os_tab[6] == 1.5 && s.detect.os_key[0] == 1 && s.detect.os_key[4] == 9 && s.detect.os_pfa == 1e-3 && s.detect.os_sent),
               (int)s.plot.own_list);
    }
    done("end_products");
}

// buffers, products and staged uploads (with their events) in several families; the state is moved, and both objects leave the scope
static void scope_case()
{
    fake_reset();
    {
        RtsCubeState a; double* out = nullptr; double* h = nullptr;
        (void)a.own.reserve(100); (void)a.wave.d.reserve(10); (void)a.doppler.map.place(nullptr, 10, &out); (void)a.detect.d_list.reserve(3);
        (void)a.detect.os_alpha.begin(4, 4, 4, &h); (void)a.track.d_tab[0].reserve(2); (void)a.track.d_tab[1].reserve(2); (void)a.tbd.d_merit[1].reserve(5);
        (void)a.image.geo.begin(4, 8, 4, &h); h[0] = 1.0; (void)a.image.geo.send(1, g_stream); (void)a.adapt.mvdr.place(nullptr, 6, &out); (void)a.doa.d_eig_status.reserve(2);
        (void)a.focus.tab.begin(2, 2, 2, &h); (void)a.focus.d_rows.reserve(9); (void)a.source.tab.begin(2, 2, 2, &h);
        g_log += "| ";
        RtsCubeState b(std::move(a));
        char s[64]; snprintf(s, sizeof(s), "MOVED:%d:%d ", (int)(!a.own.p && !a.wave.d.p && !a.doppler.map.own.p && !a.image.geo.ev && !a.focus.d_rows.p), (int)(b.own.p && b.image.geo.armed && b.focus.tab.ev)); g_log += s;
    }
    done("scope");
}

int main()
{
    product_cases();
    end_products_case();
    scope_case();
    return 0;
}
