// Driver of tests/test_plot_host.py: rts_amd/csrc/rts_plot.h alone, built with a plain host compiler (under AddressSanitizer +
// UndefinedBehaviorSanitizer where it has them).  Cases on stdin, results on stdout; the expectations live in the test.  A case is
//     n_rx nd nb t0 dt  link_range link_doppler min_cells pri  capacity n   then n x (rx k r power noise range_offset doppler_offset)
// (doubles as C99 hexadecimal floats).  The list and the output are heap arrays of EXACTLY n and capacity records, so a read or a
// write beyond either is a sanitizer report.  Per case one line: the code of rts_plot_params_check, the code of rts_plot_list_check,
// the total, the number of pairs (i, j < i) on which the neighbour enumeration and the adjacency predicate disagree (lists of up to
// 8 192 records; the enumeration is what the union runs on, the predicate is the definition), then every field of the records written.
#include "rts_plot.h"
#include <cstdio>
#include <cstdlib>
#include <memory>
#include <vector>

int main()
{
    for (;;) {
        unsigned n_rx, nd, nb, lr, ld, min_cells, capacity, n;
        double t0, dt, pri;
        if (scanf("%u %u %u %la %la %u %u %u %la %u %u", &n_rx, &nd, &nb, &t0, &dt, &lr, &ld, &min_cells, &pri, &capacity, &n) != 11) break;
        std::unique_ptr<RtsDetection[]> list(new RtsDetection[n]);
        for (unsigned i = 0; i < n; i++) {
            RtsDetection& d = list[i];
            if (scanf("%u %u %u %la %la %la %la", &d.rx, &d.doppler_bin, &d.range_bin, &d.power, &d.noise, &d.range_offset, &d.doppler_offset) != 7) return 2;
            d.n_train = 0; d.threshold = 0.0; d.delay = 0.0; d.doppler = 0.0;
        }
        std::unique_ptr<RtsPlot[]> out(new RtsPlot[capacity]);
        RtsCubeParams q; q.n_rx = n_rx; q.n_pulses = 1; q.n_bins = nb; q.reserved = 0; q.t0 = t0; q.dt = dt;
        RtsPlotParams p; p.link_range = lr; p.link_doppler = ld; p.min_cells = min_cells; p.max_plots = 0; p.pri = pri; p.device_list = nullptr;
        p.n_list = 0; p.n_doppler = 0; p.reserved[0] = 0; p.reserved[1] = 0;
        uint32_t bad = 0;
        const int pc = rts_plot_params_check(&p), lc = pc ? 0 : rts_plot_list_check(list.get(), n, n_rx, nd, nb, &bad);
        uint32_t total = 0;
        if (!pc && !lc) total = rts_plots_eval_host(&q, list.get(), n, nd, &p, out.get(), capacity);
        unsigned long long wrong = 0;
        if (!pc && !lc && n <= 8192u) {
            std::vector<char> hit(n, 0);
            const RtsDetection* l = list.get();
            for (uint32_t i = 0; i < n; i++) {
                rts_plot_neighbours(i, l[i].rx, l[i].doppler_bin, l[i].range_bin, lr, ld, nd, nb, [l, nd, nb](uint32_t j) { return rts_plot_key(l[j], nd, nb); },
                                    [&hit](uint32_t j) { hit[j] = 1; });
                for (uint32_t j = 0; j < i; j++) {
                    const bool adj = rts_plot_adjacent(l[i].rx, l[i].doppler_bin, l[i].range_bin, l[j].rx, l[j].doppler_bin, l[j].range_bin, lr, ld, nd);
                    if (adj != (hit[j] != 0)) wrong++;
                    hit[j] = 0;
                }
            }
        }
        printf("%d %d %u %llu", pc, lc, total, wrong);
        for (uint32_t i = 0; i < total && i < capacity; i++) {
            const RtsPlot& r = out[i];
            printf(" %u %u %u %u %u %u %u %u %a %a %a %a %a %a %a %a %a", r.rx, r.n_cells, r.first_index, r.peak_index, r.range_min, r.range_max, r.doppler_lo, r.doppler_span,
                   r.power_sum, r.peak_power, r.noise_sum, r.range_centroid, r.doppler_centroid, r.range_spread, r.doppler_spread, r.delay, r.doppler);
        }
        printf("\n");
    }
    return 0;
}
