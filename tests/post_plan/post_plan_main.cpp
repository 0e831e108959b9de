// Driver of tests/test_post_plan_host.py: rts_amd/csrc/rts_post_plan.h alone, built with a plain host compiler.
// One case per line on stdin (a name, then integers), one line of results on stdout; the expectations live in the test.
#include "rts_post_plan.h"
#include <cstdio>
#include <cstring>
#include <cinttypes>

int main()
{
    char name[32]; char line[1024];
    while (fgets(line, sizeof(line), stdin)) {
        long long v[24] = {0}; int used = 0;
        if (sscanf(line, "%31s%n", name, &used) != 1) continue;
        int n = 0; for (const char* s = line + used; n < 24; n++) { int k = 0; if (sscanf(s, "%lld%n", &v[n], &k) != 1) break; s += k; }
        if (!strcmp(name, "consts")) printf("%d %d %u %u %d\n", RTS_MAX_DEPTH, RTS_SMALL_THREADS, RTS_SMALL_CAP32, RTS_SMALL_CAP64, RTS_AGG_TILE);
        else if (!strcmp(name, "bits") && n == 1) printf("%u\n", rts_bits_for((uint64_t)v[0]));
        else if (!strcmp(name, "key") && n == 4) {          // D, max_path, max_rx, max_refr
            const RtsKeyPlan k = rts_key_plan((uint32_t)v[0], v[1], v[2]);
            printf("%u %u %u %u %u %u %d %d %u %d %u\n", k.B, k.RXB, k.key_bits, k.shift, k.n_words, k.n_rx_tab, k.wide ? 1 : 0, k.supported ? 1 : 0,
                   rts_small_cap(rts_agg_key64(k)), rts_agg_key64(k) ? 1 : 0, rts_spec_cap((uint32_t)v[3], k));
        }
        else if (!strcmp(name, "code") && n >= 4 && n == 4 + (int)v[0]) {      // D, max_path, max_rx, rx, path[D] -> the key, then the key decoded
            const uint32_t D = (uint32_t)v[0];
            const RtsKeyPlan k = rts_key_plan(D, v[1], v[2]);
            int32_t path[RTS_MAX_DEPTH]; for (uint32_t c = 0; c < D; c++) path[c] = (int32_t)v[4 + c];
            const uint64_t key = rts_key_encode(k, D, (uint32_t)v[3], path);
            printf("%" PRIu64 " %u", key, rts_key_rx(k, key));
            for (uint32_t c = 0; c < D; c++) printf(" %d", rts_key_path(k, key, c));
            printf("\n");
        }
        else if (!strcmp(name, "recv") && n == 2) printf("%u %d %u\n", rts_recv_sort_bits((uint32_t)v[0], (uint32_t)v[1]), rts_recv_key64((uint32_t)v[1]) ? 1 : 0, rts_small_cap(rts_recv_key64((uint32_t)v[1])));
        else if (!strcmp(name, "items") && n == 1) printf("%u\n", rts_small_items((uint32_t)v[0]));
        else if (!strcmp(name, "layout") && n == 2) {
            const RtsAggLayout l = rts_agg_layout((uint32_t)v[0], (uint32_t)v[1]);
            printf("%u %zu %zu %zu %zu %zu %zu %zu %zu\n", l.ntiles, l.per_ray, l.gcount, l.gsum, l.rcs, l.o_G, l.o_tile_first, l.o_tile_last, l.o_rxmin);
        }
        else { fprintf(stderr, "bad case: %s", line); return 2; }
    }
    return 0;
}
