// Drives rts_amd/csrc/rts_pulse_state.h alone (tests/test_pulse_state_host.py): one case per input line, one output line per case.
//   walk D0 D1 D2 <step> ...   three handles on devices D0 D1 D2 over one array of counters; a step is a transition's letter (b begin,
//                              e end, c chain, r resolve, a abandon) and the handle's digit.  Per step: accepted, the three phases
//                              (0 IDLE, 1 OPEN, 2 CHAINED), the counts of the three devices' slots, the sum of all slots.
//   enum L                     every sequence of L steps over two handles on device 0, in ascending order of its base-10 number (digit =
//                              5 * handle + transition, b e c r a; first step first): one line per sequence, per step the packed
//                              accepted * 1000 + phase0 * 100 + phase1 * 10 + count of the slot.
#include <cstdio>
#include <cstring>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>
#include "rts_pulse_state.h"

static int phase(const RtsPulseState& s) { return s.idle() + s.open() + s.chained() != 1 ? -1 : s.open() ? 1 : s.chained() ? 2 : 0; }

static bool step(RtsPulseState& s, char op, std::atomic<int>* counters, int device)
{
    switch (op) {
    case 'b': return s.begin(rts_pulse_slot(counters, device));
    case 'e': return s.end();
    case 'c': return s.chain();
    case 'r': return s.resolve();
    case 'a': return s.abandon();
    }
    std::fprintf(stderr, "unknown transition %c\n", op); std::exit(2);
}

int main()
{
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream in(line); std::string cmd; in >> cmd;
        std::vector<std::atomic<int>> counters(RTS_PULSE_SLOTS);
        for (auto& c : counters) c.store(0);
        if (cmd == "walk") {
            int dev[3]; in >> dev[0] >> dev[1] >> dev[2];
            RtsPulseState h[3]; std::string t;
            while (in >> t) {
                const int k = t[1] - '0'; if (t.size() != 2 || k < 0 || k > 2) { std::fprintf(stderr, "bad step %s\n", t.c_str()); return 2; }
                const bool ok = step(h[k], t[0], counters.data(), dev[k]);
                int sum = 0; for (auto& c : counters) sum += c.load();
                std::printf("%d %d %d %d %d %d %d %d ", ok ? 1 : 0, phase(h[0]), phase(h[1]), phase(h[2]),
                            rts_pulse_slot(counters.data(), dev[0]).load(), rts_pulse_slot(counters.data(), dev[1]).load(), rts_pulse_slot(counters.data(), dev[2]).load(), sum);
            }
            std::printf("\n");
        } else if (cmd == "enum") {
            int L = 0; in >> L; if (L < 1 || L > 6) { std::fprintf(stderr, "enum 1 .. 6\n"); return 2; }
            long total = 1; for (int i = 0; i < L; i++) total *= 10;
            std::string out;
            for (long q = 0; q < total; q++) {
                RtsPulseState h[2]; long div = total;
                for (int i = 0; i < L; i++) {
                    div /= 10; const int d = (int)(q / div % 10);
                    const bool ok = step(h[d / 5], "becra"[d % 5], counters.data(), 0);
                    out += std::to_string((ok ? 1000 : 0) + phase(h[0]) * 100 + phase(h[1]) * 10 + counters[0].load()); out += i + 1 < L ? ' ' : '\n';
                }
                h[0].abandon(); h[1].abandon();
                if (counters[0].load() != 0) { std::fprintf(stderr, "sequence %ld left the count at %d\n", q, counters[0].load()); return 3; }
                if (out.size() > (1u << 20)) { std::fwrite(out.data(), 1, out.size(), stdout); out.clear(); }
            }
            std::fwrite(out.data(), 1, out.size(), stdout);
        } else { std::fprintf(stderr, "unknown case %s\n", cmd.c_str()); return 2; }
    }
    return 0;
}
