// locate_main.cpp -- rts_amd/csrc/rts_locate.h alone, without the library and without a GPU: built by tests/test_locate_host.py with g++
// under AddressSanitizer + UndefinedBehaviorSanitizer and run on its own.  Every list, receiver array and output is a heap array of
// exactly its size, so a read or write beyond what the step is given is an error here.
// stdin, per case (hex floats):
//   n_rx a0 a1 a2 min_receivers n_iters max_candidates max_targets source reserved capacity n_list
//   tx[3]  rx[n_rx][3]  cspeed carrier sigma_delay sigma_doppler gate assoc_delay  box_lo[3] box_hi[3]
//   n_list records: plots and tracks "rx flags delay doppler power_sum", candidates "candidate n_receivers cost plot[16]"
// stdout, per case: params_code list_code total cut clean n_written, then per written target
//   (cut: 1 max_candidates cut the candidates, + 2 an anchor's segment was cut)
//   candidate n_receivers flags plot[16] pos[3] vel[3] cost power_sum
#include <cstdio>
#include <cstring>
#include <memory>
#include "rts_locate.h"

static bool rd(double* x) { return scanf("%la", x) == 1; }
static bool ru(uint32_t* x) { unsigned long long v; if (scanf("%llu", &v) != 1) return false; *x = (uint32_t)v; return true; }

int main()
{
    for (;;) {
        RtsLocateParams p;
        memset(&p, 0, sizeof(p));
        uint32_t reserved = 0, capacity = 0, n_list = 0;
        if (!ru(&p.n_rx)) break;
        bool ok = ru(&p.anchors[0]) && ru(&p.anchors[1]) && ru(&p.anchors[2]) && ru(&p.min_receivers) && ru(&p.n_iters) && ru(&p.max_candidates) && ru(&p.max_targets)
            && ru(&p.source) && ru(&reserved) && ru(&capacity) && ru(&n_list);
        p.reserved[1] = reserved;
        for (int c = 0; c < 3; c++) ok = ok && rd(&p.tx[c]);
        const uint32_t n_pos = p.n_rx <= 64u ? p.n_rx : 0u;
        std::unique_ptr<double[]> rx(new double[3u * n_pos + (n_pos ? 0u : 1u)]);
        for (uint32_t k = 0; k < 3u * n_pos; k++) ok = ok && rd(&rx[k]);
        p.rx_positions = rx.get();
        ok = ok && rd(&p.cspeed) && rd(&p.carrier) && rd(&p.sigma_delay) && rd(&p.sigma_doppler) && rd(&p.gate) && rd(&p.assoc_delay);
        for (int c = 0; c < 3; c++) ok = ok && rd(&p.box_lo[c]);
        for (int c = 0; c < 3; c++) ok = ok && rd(&p.box_hi[c]);
        std::unique_ptr<RtsPlot[]> plots; std::unique_ptr<RtsTrack[]> tracks; std::unique_ptr<RtsTarget[]> cands;
        const void* list = nullptr;
        if (p.source == RTS_LOCATE_FROM_CANDIDATES) {
            cands.reset(new RtsTarget[n_list ? n_list : 1u]);
            for (uint32_t i = 0; i < n_list; i++) {
                RtsTarget& t = cands[i];
                memset(&t, 0, sizeof(t));
                unsigned long long cand = 0;
                ok = ok && scanf("%llu", &cand) == 1 && ru(&t.n_receivers) && rd(&t.cost);
                t.candidate = cand;
                for (uint32_t m = 0; m < RTS_LOCATE_MAX_RX; m++) ok = ok && ru(&t.plot[m]);
            }
            list = n_list ? cands.get() : nullptr;
        } else if (p.source == RTS_LOCATE_FROM_TRACKS) {
            tracks.reset(new RtsTrack[n_list ? n_list : 1u]);
            for (uint32_t i = 0; i < n_list; i++) {
                RtsTrack& t = tracks[i];
                memset(&t, 0, sizeof(t));
                ok = ok && ru(&t.rx) && ru(&t.flags) && rd(&t.delay) && rd(&t.doppler) && rd(&t.power_sum);
            }
            list = n_list ? tracks.get() : nullptr;
        } else {
            plots.reset(new RtsPlot[n_list ? n_list : 1u]);
            for (uint32_t i = 0; i < n_list; i++) {
                RtsPlot& z = plots[i];
                memset(&z, 0, sizeof(z));
                uint32_t flags = 0;
                ok = ok && ru(&z.rx) && ru(&flags) && rd(&z.delay) && rd(&z.doppler) && rd(&z.power_sum);
            }
            list = n_list ? plots.get() : nullptr;
        }
        if (!ok) { fprintf(stderr, "locate_main: malformed case\n"); return 2; }
        std::unique_ptr<RtsTarget[]> out(new RtsTarget[capacity ? capacity : 1u]);
        memset(out.get(), 0x5a, sizeof(RtsTarget) * (capacity ? capacity : 1u));
        const int code = rts_locate_params_check(&p);
        int list_code = 0;
        uint32_t bad = 0, total = 0, written = 0;
        uint32_t cut = 0;
        if (code == 0) {
            if (p.source == RTS_LOCATE_FROM_PLOTS) list_code = rts_locate_plots_check(plots.get(), n_list, &bad);
            if (p.source == RTS_LOCATE_FROM_CANDIDATES) list_code = rts_locate_candidates_check(cands.get(), n_list, &bad);
        }
        if (code == 0 && list_code == 0) {
            total = rts_locate_eval_host(&p, list, n_list, capacity ? out.get() : nullptr, capacity, &cut);
            written = rts_list_copied(total, rts_locate_max_targets(p), capacity);
        }
        bool clean = true;
        const unsigned char* raw = (const unsigned char*)out.get();
        for (size_t b = sizeof(RtsTarget) * written; b < sizeof(RtsTarget) * (capacity ? capacity : 1u); b++) if (raw[b] != 0x5a) clean = false;
        printf("%d %d %u %u %d %u", code, list_code, total, cut, clean ? 1 : 0, written);
        for (uint32_t i = 0; i < written; i++) {
            const RtsTarget& t = out[i];
            printf(" %llu %u %u", (unsigned long long)t.candidate, t.n_receivers, t.flags);
            for (uint32_t m = 0; m < RTS_LOCATE_MAX_RX; m++) printf(" %u", t.plot[m]);
            for (int c = 0; c < 3; c++) printf(" %a", t.pos[c]);
            for (int c = 0; c < 3; c++) printf(" %a", t.vel[c]);
            printf(" %a %a", t.cost, t.power_sum);
        }
        printf("\n");
    }
    return 0;
}
