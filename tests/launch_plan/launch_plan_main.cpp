// Driver of tests/test_launch_plan_host.py: rts_amd/csrc/rts_launch_plan.h alone, built with a plain host compiler.
// One case per line on stdin (a name, then unsigned integers), one line of results on stdout; the expectations live in the test.
#include "rts_launch_plan.h"
#include <cstdio>
#include <cstring>
#include <cinttypes>

int main()
{
    char name[32]; char line[1024];
    while (fgets(line, sizeof(line), stdin)) {
        unsigned long long v[12] = {0}; int used = 0;
        if (sscanf(line, "%31s%n", name, &used) != 1) continue;
        int n = 0; for (const char* s = line + used; n < 12; n++) { int k = 0; if (sscanf(s, "%llu%n", &v[n], &k) != 1) break; s += k; }
        if (!strcmp(name, "consts")) printf("%d %d %d %d\n", RTS_WTILE, RTS_BLOCK, RTS_COOP_GROUP, RTS_STACK_OVF);
        else if (!strcmp(name, "small") && n == 3) printf("%" PRIu64 " %" PRIu64 " %u %u\n", rts_wave_tiles(v[0]), rts_lattice_size((uint32_t)v[1]), rts_chains((uint32_t)v[2]), rts_hit_rows((uint32_t)v[2]));
        else if (!strcmp(name, "magic") && n == 1) { const RtsDivMagic d = rts_div_magic((uint32_t)v[0]); printf("%u %u\n", d.magic, d.more); }
        else if (!strcmp(name, "part") && n == 4) printf("%" PRIu64 "\n", rts_part_count(v[0], (uint32_t)v[1], (uint32_t)v[2], (uint32_t)v[3]));
        else if (!strcmp(name, "range") && n == 11) {
            const RtsRangeArgs q = {v[0], v[1], v[2], (uint32_t)v[3], (uint32_t)v[4], (uint32_t)v[5], (uint32_t)v[6], (uint32_t)v[7], (uint32_t)v[8], (uint32_t)v[9], (uint32_t)v[10]};
            const RtsRayRange r = rts_ray_range(q);
            printf("%d %" PRIu64 " %" PRIu64 " %" PRIu64 " %" PRIu64 " %u %u %u %d\n", (int)r.err, r.first, r.span, r.count, r.range_tiles, r.il_tile, r.il_parts, r.il_part, r.il_list ? 1 : 0);
        }
        else if (!strcmp(name, "sizes") && n == 8) {
            const RtsLaunchSizes s = rts_launch_sizes(v[0], v[1], v[2], v[3], v[4], (uint32_t)v[5], (uint32_t)v[6], v[7] != 0);
            printf("%" PRIu64 " %" PRIu64 " %" PRIu64 " %" PRIu64 " %" PRIu64 " %" PRIu64 " %" PRIu64 " %" PRIu64 "\n", s.recv, s.dir_hist, s.child, s.stack_ovf, s.block_counters, s.all, s.hit_prim, s.hit_t);
        }
        else if (!strcmp(name, "grid") && n == 4) printf("%u\n", rts_trace_grid((uint32_t)v[0], (int)v[1], (int)v[2], (int)v[3]));
        else if (!strcmp(name, "coop") && n == 3) printf("%u\n", rts_coop_grid((uint32_t)v[0], v[1] != 0, (uint32_t)v[2]));
        else if (!strcmp(name, "shape") && n == 6) {
            const RtsLaunchShape s = rts_launch_shape((uint32_t)v[0], v[1], (uint32_t)v[2], (uint32_t)v[3], (uint32_t)v[4], v[5]);
            printf("%" PRIu64 " %" PRIu64 " %" PRIu64 " %" PRIu64 " %d %u %u\n", s.sig[0], s.sig[1], s.sig[2], s.sig[3], s.aligned ? 1 : 0, s.n_tiles, s.n_hist);
        }
        else { fprintf(stderr, "bad case: %s", line); return 2; }
    }
    return 0;
}
