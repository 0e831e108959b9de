// Driver of tests/test_mimo_state_host.py: the MIMO family's record of rts_amd/csrc/rts_cube_state.h (RtsMimoState), built with a plain
// host compiler and linked WITHOUT the HIP runtime, on the stand-ins of tests/owned/fake_hip.h -- the twin of
// tests/cube_state/cube_state_main.cpp and tests/passive/passive_state_main.cpp for the one product those drivers do not list.  No
// input; tokens as there.
//   end_products product mimo.out <valid before> <valid after>;  end_products kept <0|1>: the output's block and the staged table stay
//   reuse <0|1>: a second, smaller staged table allocates nothing
//   regrow <valid after a caller-owned place> <after a library-owned one that fits> <after a larger one> <after its record>: a regrow of
//     the library-owned output ends the record first
//   scope: the blocks made, MOVED, the frees
#include "rts_cube_state.h"
#include "../owned/fake_hip.h"
#include <type_traits>
#include <utility>

static_assert(std::is_same<RtsBankProduct, RtsCubeProduct>::value, "the bank's output is a product like the others");
static double g_caller[4];      // "the caller's device memory": never dereferenced

int main()
{
    fake_reset();
    {
        RtsCubeState s;
        s.set = true; s.p = g_caller;
        double* out = nullptr; double* h = nullptr;
        (void)s.mimo.out.place(nullptr, 10, &out); s.mimo.out.record(out, 10);
        (void)s.mimo.tab.begin(6, 6, 6, &h);
        { const size_t logged = g_log.size(); double* h2 = nullptr; (void)s.mimo.tab.begin(3, 3, 3, &h2); printf("reuse %d\n", (int)(h2 == h && g_log.size() == logged)); }      // a smaller set: no new block
        s.doppler.map.record(g_caller, 4);
        const bool b = s.mimo.out.valid, d = s.doppler.map.valid;
        s.end_products();
        printf("end_products product mimo.out %d %d\n", (int)b, (int)s.mimo.out.valid);
        printf("end_products product doppler.map %d %d\n", (int)d, (int)s.doppler.map.valid);
        printf("end_products kept %d\n", (int)(s.set && s.p == g_caller && s.mimo.out.own.p && s.mimo.out.p == s.mimo.out.own.p && s.mimo.out.doubles == 10 && s.mimo.tab.pin.p && s.mimo.tab.dev.p));
        // a caller-owned output leaves the record alone; a library-owned one that fits keeps it; a larger one ends it before the block is freed
        s.mimo.out.record(out, 10);
        double* o2 = nullptr;
        (void)s.mimo.out.place(g_caller, 1u << 20, &o2); const bool v0 = s.mimo.out.valid && o2 == g_caller;
        (void)s.mimo.out.place(nullptr, 8, &o2); const bool v1 = s.mimo.out.valid && o2 == out;
        (void)s.mimo.out.place(nullptr, s.mimo.out.own.cap + 1, &o2); const bool v2 = s.mimo.out.valid;
        s.mimo.out.record(o2, s.mimo.out.own.cap);
        printf("regrow %d %d %d %d\n", (int)v0, (int)v1, (int)v2, (int)(s.mimo.out.valid && s.mimo.out.p == s.mimo.out.own.p));
    }
    { char t[32]; snprintf(t, sizeof(t), "LIVE:%zu", fake_live()); printf("end_products %s%s\n", g_log.c_str(), t); g_log.clear(); fake_sweep(); }
    fake_reset();
    {
        RtsCubeState a; double* out = nullptr; double* h = nullptr;
        (void)a.mimo.out.place(nullptr, 7, &out); (void)a.mimo.tab.begin(5, 5, 5, &h);
        g_log += "| ";
        RtsCubeState b(std::move(a));
        char t[64]; snprintf(t, sizeof(t), "MOVED:%d:%d ", (int)(!a.mimo.out.own.p && !a.mimo.tab.pin.p && !a.mimo.tab.dev.p), (int)(b.mimo.out.own.p && b.mimo.tab.pin.p && b.mimo.tab.dev.p)); g_log += t;
    }
    { char t[32]; snprintf(t, sizeof(t), "LIVE:%zu", fake_live()); printf("scope %s%s\n", g_log.c_str(), t); g_log.clear(); fake_sweep(); }
    return 0;
}
