// Driver of tests/test_source_host.py: rts_amd/csrc/rts_source.h alone, built with a plain host compiler (under AddressSanitizer +
// UndefinedBehaviorSanitizer where it has them).  Cases on stdin, results on stdout; the expectations live in the test.  A case is
//     n_rx n_pulses n_bins n_patches flags reserved seed has_rho has_profile prefill
//     then spatial (n_patches x n_rx x (re im)), power, doppler, rho (if has_rho), range_profile (if has_profile)
// (doubles as C99 hexadecimal floats).  The tables, the work array, the launch plan's table and the cube are heap arrays of EXACTLY
// their sizes, so a read or a write beyond any of them is a sanitizer report.  The cube starts as (prefill, -prefill) in every
// sample.  Per case one line: the code of rts_src_check and its index, the plan (groups slots stage_pulses lds table_doubles
// supported), the live mask, the sum of the plan's table (a read of every entry), then -- unless refused -- the cube.
#include "rts_source.h"
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>

static bool read_doubles(double* d, size_t n)
{
    for (size_t i = 0; i < n; i++) if (scanf("%la", &d[i]) != 1) return false;
    return true;
}

int main()
{
    for (;;) {
        unsigned n_rx, n_pulses, n_bins, K, flags, has_rho, has_profile;
        unsigned long long reserved, seed;
        double prefill;
        if (scanf("%u %u %u %u %u %llu %llu %u %u %la", &n_rx, &n_pulses, &n_bins, &K, &flags, &reserved, &seed, &has_rho, &has_profile, &prefill) != 10) break;
        std::unique_ptr<double[]> spatial(new double[2 * (size_t)K * n_rx]), power(new double[K]), doppler(new double[K]), rho(new double[has_rho ? K : 0]),
            profile(new double[has_profile ? n_bins : 0]);
        if (!read_doubles(spatial.get(), 2 * (size_t)K * n_rx) || !read_doubles(power.get(), K) || !read_doubles(doppler.get(), K)) return 2;
        if (has_rho && !read_doubles(rho.get(), K)) return 2;
        if (has_profile && !read_doubles(profile.get(), n_bins)) return 2;
        RtsSourceParams p;
        memset(&p, 0, sizeof(p));
        p.n_patches = K; p.flags = flags; p.reserved[1] = reserved; p.seed = seed;
        p.spatial = spatial.get(); p.power = power.get(); p.doppler = doppler.get();
        p.rho = has_rho ? rho.get() : nullptr; p.range_profile = has_profile ? profile.get() : nullptr;
        RtsCubeParams q;
        memset(&q, 0, sizeof(q));
        q.n_rx = n_rx; q.n_pulses = n_pulses; q.n_bins = n_bins; q.dt = 1.0;
        uint32_t bad = 0;
        const int code = rts_src_check(&p, n_rx, n_bins, &bad);
        const RtsSrcPlan plan = rts_src_plan(n_rx, n_bins, K, has_profile != 0);
        printf("%d %u %u %u %u %zu %zu %d", code, bad, plan.groups, plan.slots, plan.stage_pulses, plan.lds, plan.table_doubles, plan.supported ? 1 : 0);
        if (code) { printf("\n"); continue; }
        std::unique_ptr<double[]> tab(new double[plan.table_doubles]);
        rts_src_table(&p, n_rx, n_bins, tab.get());
        double sum = 0.0;
        for (size_t i = 0; i < plan.table_doubles; i++) sum += tab[i];
        printf(" %llu %a", (unsigned long long)rts_src_live_mask(K, p.power), sum);
        const size_t doubles = 2 * (size_t)n_rx * n_pulses * n_bins;
        std::unique_ptr<double[]> cube(new double[doubles]), work(new double[rts_src_work_doubles(K)]);
        for (size_t i = 0; i < doubles; i += 2) { cube[i] = prefill; cube[i + 1] = -prefill; }
        rts_sources_eval_host(&q, &p, cube.get(), work.get());
        for (size_t i = 0; i < doubles; i++) printf(" %a", cube[i]);
        printf("\n");
    }
    return 0;
}
