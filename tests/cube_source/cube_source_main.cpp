// Driver of tests/test_cube_source_host.py: rts_amd/csrc/rts_cube_source.h and the plans of rts_amd/csrc/rts_stft.h alone, built with
// a plain host compiler (under AddressSanitizer + UndefinedBehaviorSanitizer where it has them).  One case per line on stdin, the
// results on stdout; the expectations live in the test.  "read" takes a record set on its line and answers, per record, both forms
// of the question and the delay and phase as bit patterns.  The set's arrays are heap arrays of exactly their sizes, and a set read
// per ray has NO delay, phase or path-match array at all: a read of one is a sanitizer report.
#include "rts_cube_source.h"
#include "rts_stft.h"
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <iostream>

static unsigned long long bits(double x) { unsigned long long u; memcpy(&u, &x, sizeof(u)); return u; }

int main()
{
    std::string text;
    while (std::getline(std::cin, text)) {
        char name[32]; int used = 0;
        if (sscanf(text.c_str(), "%31s%n", name, &used) != 1) continue;
        const char* s = text.c_str() + used;
        auto next = [&](double* v) { char* e = nullptr; *v = strtod(s, &e); const bool ok = e != s; s = e; return ok; };
        if (!strcmp(name, "read")) {          // paths base n_rx rx cspeed carrier n, then n x (received rayLength power pm delay phase)
            double h[7]; for (double& x : h) if (!next(&x)) { fprintf(stderr, "bad case: %s\n", text.c_str()); return 2; }
            const bool paths = h[0] != 0.0; const uint32_t n_rx = (uint32_t)h[2], n = (uint32_t)h[6]; const int32_t rx_asked = (int32_t)h[3];
            PerRayData* rays = new PerRayData[n];
            double* delay = paths ? new double[n] : nullptr; double* phase = paths ? new double[n] : nullptr; int32_t* pm = paths ? new int32_t[n] : nullptr;
            for (uint32_t i = 0; i < n; i++) {
                double r[6]; for (double& x : r) if (!next(&x)) { fprintf(stderr, "bad record %u: %s\n", i, text.c_str()); return 2; }
                memset(&rays[i], 0, sizeof(PerRayData));
                rays[i].received = (int)r[0]; rays[i].rayLength = r[1]; rays[i].power = r[2];
                if (paths) { pm[i] = (int32_t)r[3]; delay[i] = r[4]; phase[i] = r[5]; }
            }
            RtsCubeSource src; src.rays = rays; src.delay = delay; src.phase = phase; src.pm = pm; src.base = (int64_t)h[1];
            src.R = n; src.paths = paths ? 1 : 0; src.cspeed = h[4]; src.carrier = h[5];
            for (uint32_t i = 0; i < n; i++) {
                int32_t own = -2; double d = 0.0, ph = 0.0, re = 0.0, im = 0.0;
                const bool asked = rts_cube_counts_for(src, paths, i, rx_asked), any = rts_cube_counts(src, paths, i, n_rx, &own);
                if (asked || any) { rts_cube_timing(src, paths, i, &d, &ph); rts_cube_amplitude(rays[i].power, ph, &re, &im); }
                printf("%d %d %d %llu %llu %.17g %.17g%c", asked ? 1 : 0, any ? 1 : 0, own, bits(d), bits(ph), re, im, i + 1 == n ? '\n' : ' ');
            }
            if (n == 0) printf("\n");
            delete[] pm; delete[] phase; delete[] delay; delete[] rays;
        }
        else if (!strcmp(name, "log2")) {     // n ...
            double v; bool first = true;
            while (next(&v)) { printf("%s%u", first ? "" : " ", rts_stft_log2((uint32_t)v)); first = false; }
            printf("\n");
        }
        else if (!strcmp(name, "dopplerplan")) {      // n_fft
            double v; if (!next(&v)) return 2;
            const RtsDopplerPlan p = rts_doppler_plan((uint32_t)v);
            printf("%u %u %zu\n", p.logN, p.BT, p.lds);
        }
        else { fprintf(stderr, "bad case: %s\n", text.c_str()); return 2; }
    }
    return 0;
}
