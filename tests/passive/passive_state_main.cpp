// Driver of tests/test_passive_state_host.py: the passive family's record of rts_amd/csrc/rts_cube_state.h (RtsPassiveState), built with a
// plain host compiler and linked WITHOUT the HIP runtime, on the stand-ins of tests/owned/fake_hip.h -- the twin of
// tests/cube_state/cube_state_main.cpp for the one product that driver does not list.  No input; tokens as there.
//   end_products product passive.xcorr <valid before> <valid after>;  end_products record passive.cancel <before> <after>
//   end_products kept <0|1>: the shape of the last cancellation and the buffers stay;  scope: the blocks made, MOVED, the frees
#include "rts_cube_state.h"
#include "../owned/fake_hip.h"
#include <type_traits>
#include <utility>

static_assert(std::is_same<RtsXcorrProduct, RtsCubeProduct>::value, "the correlation's output is a product like the others");
static double g_caller[4];      // "the caller's device memory": never dereferenced

int main()
{
    fake_reset();
    {
        RtsCubeState s;
        s.set = true; s.p = g_caller;
        double* out = nullptr;
        (void)s.passive.xcorr.place(nullptr, 10, &out); s.passive.xcorr.record(out, 10);
        (void)s.passive.d_coeff.reserve(6); (void)s.passive.d_fail.reserve(3);
        s.passive.n_blocks = 3; s.passive.n_taps = 2; s.passive.n_rx = 1; s.passive.cancel_valid = true;
        s.doppler.map.record(g_caller, 4);
        const bool x = s.passive.xcorr.valid, c = s.passive.cancel_valid, d = s.doppler.map.valid;
        s.end_products();
        printf("end_products product passive.xcorr %d %d\n", (int)x, (int)s.passive.xcorr.valid);
        printf("end_products record passive.cancel %d %d\n", (int)c, (int)s.passive.cancel_valid);
        printf("end_products product doppler.map %d %d\n", (int)d, (int)s.doppler.map.valid);
        printf("end_products kept %d\n", (int)(s.set && s.p == g_caller && s.passive.n_blocks == 3 && s.passive.n_taps == 2 && s.passive.n_rx == 1 && s.passive.d_coeff.p && s.passive.d_fail.p &&
                                                s.passive.xcorr.own.p && s.passive.xcorr.p == s.passive.xcorr.own.p && s.passive.xcorr.doubles == 10));
    }
    { char t[32]; snprintf(t, sizeof(t), "LIVE:%zu", fake_live()); printf("end_products %s%s\n", g_log.c_str(), t); g_log.clear(); fake_sweep(); }
    fake_reset();
    {
        RtsCubeState a; double* out = nullptr;
        (void)a.passive.d_part.reserve(5); (void)a.passive.d_sums.reserve(5); (void)a.passive.d_coeff.reserve(5); (void)a.passive.d_fail.reserve(2); (void)a.passive.xcorr.place(nullptr, 7, &out);
        g_log += "| ";
        RtsCubeState b(std::move(a));
        char t[64]; snprintf(t, sizeof(t), "MOVED:%d:%d ", (int)(!a.passive.d_part.p && !a.passive.d_fail.p && !a.passive.xcorr.own.p), (int)(b.passive.d_sums.p && b.passive.xcorr.own.p)); g_log += t;
    }
    { char t[32]; snprintf(t, sizeof(t), "LIVE:%zu", fake_live()); printf("scope %s%s\n", g_log.c_str(), t); g_log.clear(); fake_sweep(); }
    return 0;
}
