// Driver of tests/test_track_host.py: rts_amd/csrc/rts_track.h alone, built with a plain host compiler (under AddressSanitizer +
// UndefinedBehaviorSanitizer where it has them).  Cases on stdin, results on stdout; the expectations live in the test.  A case is
//     gate sigma_delay sigma_doppler q delay_rate_per_hz doppler_period  confirm_hits max_misses tentative_misses max_candidates max_tracks
//     reserved  next_id T  capacity n_tracks n_plots
//     then n_tracks x (id rx flags hits misses age plot_index delay doppler p_dd p_df p_ff)  and  n_plots x (rx delay doppler power_sum)
// (doubles as C99 hexadecimal floats).  The table, the plot list and the output are heap arrays of EXACTLY n_tracks, n_plots and
// capacity records, so a read or a write beyond any of them is a sanitizer report; the output is filled with 0x5a first.  Per case one
// line: the code of rts_track_params_check, whether the interval passes rts_track_interval_ok, the codes of rts_track_table_check and
// rts_track_plots_check, the total, the next id, whether every output record beyond those written still holds its fill, then every
// field of the records written.  A refused case evaluates nothing.
#include "rts_track.h"
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>

int main()
{
    for (;;) {
        RtsTrackParams p;
        unsigned long long next_id, reserved;
        unsigned capacity, n_t, n_z;
        double T;
        if (scanf("%la %la %la %la %la %la %u %u %u %u %u %llu %llu %la %u %u %u", &p.gate, &p.sigma_delay, &p.sigma_doppler, &p.q, &p.delay_rate_per_hz, &p.doppler_period,
                  &p.confirm_hits, &p.max_misses, &p.tentative_misses, &p.max_candidates, &p.max_tracks, &reserved, &next_id, &T, &capacity, &n_t, &n_z) != 17) break;
        p.n_plots = 0; p.device_plots = nullptr; p.reserved[0] = 0; p.reserved[1] = reserved;
        std::unique_ptr<RtsTrack[]> in(new RtsTrack[n_t]);
        for (unsigned i = 0; i < n_t; i++) {
            RtsTrack& t = in[i];
            unsigned long long id;
            if (scanf("%llu %u %u %u %u %u %u %la %la %la %la %la", &id, &t.rx, &t.flags, &t.hits, &t.misses, &t.age, &t.plot_index, &t.delay, &t.doppler, &t.p_dd, &t.p_df, &t.p_ff) != 12) return 2;
            t.id = id; t.d2 = 0.0; t.power_sum = 0.0;
        }
        std::unique_ptr<RtsPlot[]> z(new RtsPlot[n_z]);
        for (unsigned j = 0; j < n_z; j++) {
            memset(&z[j], 0, sizeof(RtsPlot));
            if (scanf("%u %la %la %la", &z[j].rx, &z[j].delay, &z[j].doppler, &z[j].power_sum) != 4) return 2;
        }
        std::unique_ptr<RtsTrack[]> out(new RtsTrack[capacity]);
        memset((void*)out.get(), 0x5a, sizeof(RtsTrack) * capacity);
        uint32_t bad = 0;
        const int pc = rts_track_params_check(&p);
        const int ok = n_t == 0 || rts_track_interval_ok(T) ? 1 : 0;
        const int tc = rts_track_table_check(in.get(), n_t, &bad), zc = rts_track_plots_check(z.get(), n_z, &bad);
        uint32_t total = 0, written = 0;
        uint64_t nid = 0;
        if (!pc && ok && !tc && !zc && n_t <= rts_track_table_size(p)) {
            total = rts_tracks_eval_host(&p, in.get(), n_t, next_id, T, z.get(), n_z, out.get(), capacity, &nid);
            written = total < rts_track_table_size(p) ? total : rts_track_table_size(p);
            if (written > capacity) written = capacity;
        }
        int clean = 1;
        for (size_t b = sizeof(RtsTrack) * written; b < sizeof(RtsTrack) * capacity; b++) if (((const unsigned char*)out.get())[b] != 0x5a) clean = 0;
        printf("%d %d %d %d %u %llu %d", pc, ok, tc, zc, total, (unsigned long long)nid, clean);
        for (uint32_t i = 0; i < written; i++) {
            const RtsTrack& r = out[i];
            printf(" %llu %u %u %u %u %u %u %a %a %a %a %a %a %a", (unsigned long long)r.id, r.rx, r.flags, r.hits, r.misses, r.age, r.plot_index, r.delay, r.doppler, r.p_dd, r.p_df,
                   r.p_ff, r.d2, r.power_sum);
        }
        printf("\n");
    }
    return 0;
}
