// Driver of tests/test_prim_order_host.py: rts_amd/csrc/rts_prim_order.h alone, no HIP.
// One case per input line: "n_prims slot slot ..." (the leaf slots' primitive ids); the answer is the order, one line per case.
#include <cstdio>
#include <iostream>
#include <sstream>
#include <string>
#include "rts_prim_order.h"

int main()
{
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream in(line);
        uint32_t n_prims = 0; in >> n_prims;
        std::vector<uint32_t> slots; uint32_t s;
        while (in >> s) slots.push_back(s);
        const std::vector<uint32_t> order = rts_prim_order(slots.data(), slots.size(), n_prims);
        for (size_t i = 0; i < order.size(); i++) printf(i ? " %u" : "%u", order[i]);
        printf("\n");
    }
    return 0;
}
