// flash_paged_varlen_plan_main.cpp — candle_birefnet_amd/csrc/brn_flash_paged_varlen_plan.h on its own, for
// tests/test_flash_attention_paged_varlen_cpu.py: compiled with the host compiler under -fsanitize=address,undefined (the header needs no
// HIP).  Every input line is "total_q G n_seqs cu[0] .. cu[n_seqs]"; the answer is one line: the plan's 2 * (n_seqs + 1) ints (the
// starts, then the tile prefix), then T_max and plan_ints.  The plan is written into a buffer of exactly plan_ints ints, so a write past
// it is the sanitizer's to report.
#include "brn_flash_paged_varlen_plan.h"

#include <cstdio>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

int main() {
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream in(line);
        int total_q, G, n_seqs;
        if (!(in >> total_q >> G >> n_seqs) || n_seqs < 1) return 2;
        std::vector<int> cu((size_t)n_seqs + 1);
        for (int& c : cu)
            if (!(in >> c)) return 2;
        std::vector<int> plan(brn::fa_pv_plan_ints(n_seqs));
        brn::flash_paged_varlen_plan_ref(cu.data(), n_seqs, total_q, G, plan.data());
        for (int v : plan) std::printf("%d ", v);
        std::printf("%lld %zu\n", brn::fa_pv_max_tiles(G, total_q, n_seqs), brn::fa_pv_plan_ints(n_seqs));
    }
    return 0;
}
