// The stand-alone driver of rts_amd/csrc/rts_cube_args.h (tests/test_cube_args_host.py): one case per line of stdin, one answer per
// line of stdout.  Addresses are integers cast to pointers: the rules compare them and touch no memory.
//   span first n total zero_to_end at_least_one      -> ok count
//   pow2 v lo hi                                     -> ok
//   bytes a na b nb                                  -> overlap
//   rx out out_bytes src rx_stride cell0 cell1 n_rx  -> overlap receiver (receiver -1 without an overlap)
//   source source n_rows_in device_in                -> rule
//   copied total max capacity                        -> n
#include <cinttypes>
#include <cstdio>
#include <cstring>
#include "rts_cube_args.h"

int main()
{
    char cmd[16];
    while (scanf("%15s", cmd) == 1) {
        if (!strcmp(cmd, "span")) {
            uint32_t first, n, total, count = 0xdeadu; int zero_to_end, at_least_one;
            if (scanf("%" SCNu32 "%" SCNu32 "%" SCNu32 "%d%d", &first, &n, &total, &zero_to_end, &at_least_one) != 5) return 2;
            const bool ok = rts_span_inside(first, n, total, zero_to_end != 0, at_least_one != 0, &count);
            if (ok != rts_span_inside(first, n, total, zero_to_end != 0, at_least_one != 0)) return 3;      // (the count is optional)
            printf("%d %" PRIu32 "\n", ok ? 1 : 0, ok ? count : 0u);
        } else if (!strcmp(cmd, "pow2")) {
            uint32_t v, lo, hi;
            if (scanf("%" SCNu32 "%" SCNu32 "%" SCNu32, &v, &lo, &hi) != 3) return 2;
            printf("%d\n", rts_pow2_in(v, lo, hi) ? 1 : 0);
        } else if (!strcmp(cmd, "bytes")) {
            uint64_t a, na, b, nb;
            if (scanf("%" SCNu64 "%" SCNu64 "%" SCNu64 "%" SCNu64, &a, &na, &b, &nb) != 4) return 2;
            printf("%d\n", rts_bytes_overlap((const void*)(uintptr_t)a, (size_t)na, (const void*)(uintptr_t)b, (size_t)nb) ? 1 : 0);
        } else if (!strcmp(cmd, "rx")) {
            uint64_t out, out_bytes, src, stride, cell0, cell1; uint32_t n_rx, r = 0xdeadu;
            if (scanf("%" SCNu64 "%" SCNu64 "%" SCNu64 "%" SCNu64 "%" SCNu64 "%" SCNu64 "%" SCNu32, &out, &out_bytes, &src, &stride, &cell0, &cell1, &n_rx) != 7) return 2;
            const bool hit = rts_rx_spans_overlap((const void*)(uintptr_t)out, (size_t)out_bytes, (const void*)(uintptr_t)src, stride, cell0, cell1, n_rx, &r);
            printf("%d %ld\n", hit ? 1 : 0, hit ? (long)r : -1L);
        } else if (!strcmp(cmd, "source")) {
            uint32_t source, n_rows_in; int device_in;
            if (scanf("%" SCNu32 "%" SCNu32 "%d", &source, &n_rows_in, &device_in) != 3) return 2;
            printf("%d\n", rts_source_fields_rule(source, n_rows_in, device_in ? (const void*)(uintptr_t)4096u : nullptr));
        } else if (!strcmp(cmd, "copied")) {
            uint32_t total, max, capacity;
            if (scanf("%" SCNu32 "%" SCNu32 "%" SCNu32, &total, &max, &capacity) != 3) return 2;
            printf("%" PRIu32 "\n", rts_list_copied(total, max, capacity));
        } else return 2;
    }
    return 0;
}
