// Driver of tests/test_image_host.py: rts_amd/csrc/rts_image.h alone, built with a plain host compiler (under AddressSanitizer +
// UndefinedBehaviorSanitizer where it has them).  One case per line on stdin, one line of results on stdout; the expectations live
// in the test.  Every row is a heap array of EXACTLY n_bins complex samples, so a tap read outside the row is a sanitizer report.
#include "rts_image.h"
#include <cstdio>
#include <cstring>
#include <vector>

int main()
{
    char name[32]; char line[1024];
    while (fgets(line, sizeof(line), stdin)) {
        double v[8] = {0}; int used = 0;
        if (sscanf(line, "%31s%n", name, &used) != 1) continue;
        int n = 0; for (const char* s = line + used; n < 8; n++) { int k = 0; if (sscanf(s, "%lf%n", &v[n], &k) != 1) break; s += k; }
        if (!strcmp(name, "sample") && n == 3) {             // n_bins, taps, d: row[m] = (m + 1) + j (0.5 - m)
            const uint32_t nb = (uint32_t)v[0], taps = (uint32_t)v[1];
            double* row = new double[2 * (size_t)nb];
            for (uint32_t m = 0; m < nb; m++) { row[2 * m] = (double)m + 1.0; row[2 * m + 1] = 0.5 - (double)m; }
            double re, im; rts_image_sample(row, nb, rts_image_interp_setup(taps), v[2], &re, &im);
            delete[] row;
            printf("%.17g %.17g\n", re, im);
        }
        else if (!strcmp(name, "plan") && n == 5) {          // n_x, n_y, n_rx, n_pulses, split_below
            const RtsImagePlan p = rts_image_plan((uint32_t)v[0], (uint32_t)v[1], (uint32_t)v[2], (uint32_t)v[3], (uint32_t)v[4]);
            printf("%u %u %u %u %u %d %d %zu\n", p.tw_log2, p.th_log2, p.tiles_x, p.tiles_y, p.n_chunks, p.split ? 1 : 0, p.supported ? 1 : 0, p.scratch);
        }
        else if (!strcmp(name, "consts")) printf("%u %u %u %u\n", RTS_IMAGE_TILE, RTS_IMAGE_PULSE_CHUNK, RTS_IMAGE_MAX_PIXELS, RTS_IMAGE_GRID_MAX);
        else { fprintf(stderr, "bad case: %s", line); return 2; }
    }
    return 0;
}
