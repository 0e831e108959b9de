// Driver of tests/test_tuning_host.py: rts_amd/csrc/rts_tuning.h alone, built with a plain host compiler.
// One case per line on stdin: NAME=VALUE pairs separated by tabs (a value may be empty or hold spaces; "@host_build" stands for
// RTS_FLAG_HOST_BUILD in the handle's flags); the line "!table" asks for the table's rows instead.  The readers are served from
// that map; every field of every record is printed, one "record.field value" per line, and a line "." ends the case.  The
// expectations live in the test.
#include "rts_tuning.h"
#include <cinttypes>
#include <cstdio>
#include <map>
#include <string>

static std::map<std::string, std::string> g_env;
static const char* look(const char* name) { const auto it = g_env.find(name); return it == g_env.end() ? nullptr : it->second.c_str(); }

int main()
{
    static const char* scopes[] = {"handle", "scene", "process", "launch"};
    std::string line; int ch;
    for (;;) {
        line.clear();
        while ((ch = getchar()) != EOF && ch != '\n') line.push_back((char)ch);
        if (ch == EOF && line.empty()) break;
        if (line == "!table") {
            for (const RtsSwitch& s : RTS_SWITCHES) printf("%s %s\n", s.name, scopes[s.scope]);
            printf(".\n");
            continue;
        }
        g_env.clear(); bool host_build = false;
        for (size_t a = 0; a < line.size();) {
            size_t b = line.find('\t', a); if (b == std::string::npos) b = line.size();
            const std::string item = line.substr(a, b - a); a = b + 1;
            if (item == "@host_build") { host_build = true; continue; }
            const size_t eq = item.find('=');
            if (eq == std::string::npos) { fprintf(stderr, "bad item: %s\n", item.c_str()); return 2; }
            g_env[item.substr(0, eq)] = item.substr(eq + 1);
        }
        RtsTuning t; rts_tuning_read(&t, look);
        RtsSceneTuning s; s.device_build = !host_build; rts_tuning_read(&s, look);
        RtsProcessTuning p; rts_tuning_read(&p, look);
        RtsLaunchTuning l; rts_tuning_read(&l, look);
#define B(r, f) printf(#r "." #f " %d\n", r.f ? 1 : 0)
#define I(r, f) printf(#r "." #f " %lld\n", (long long)r.f)
#define U(r, f) printf(#r "." #f " %" PRIu64 "\n", (uint64_t)r.f)
#define D(r, f) printf(#r "." #f " %.17g\n", r.f)
        B(t, use_pmask); I(t, grid_mult); I(t, grid_spare); B(t, grid_spare_forced); B(t, tile_lpt); D(t, ew_rel); U(t, stack_lds);
        B(t, rx_window_screen); I(t, batch_dead); B(t, node_versions); B(t, share_history); B(t, trace_own_stream); B(t, spin_wait);
        D(t, coop_frac); U(t, coop_floor); U(t, coop_walk_steps); U(t, coop_walk_steps_lo); D(t, coop_mid); D(t, coop_big); D(t, coop_big_part);
        U(t, coop_spread); U(t, coop_grid_max); B(t, coop_versions); B(t, post_small); U(t, post_one_max); U(t, post_prio); B(t, spec_enabled);
        U(t, img_split_below); U(t, beat_force_parts); B(t, timeline_blocks); B(t, debug_coop);
        B(s, device_build); D(s, split_budget); B(s, build_fallback); B(s, fail_device_build); B(s, node_versions); B(s, version_key_centre);
        B(s, sah_tree); I(s, crowd_rounds); I(s, ref_gain_rule); B(s, debug_build);
        B(p, lap); B(p, debug_sync);
        printf("l.timeline %s\n", l.timeline ? l.timeline : "(null)");
        printf(".\n");
    }
    return 0;
}
