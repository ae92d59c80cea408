// The host-only plan of brn_flash_attention_varlen_forward (csrc/brn_flash_varlen_plan.h) as a stand-alone program for
// tests/test_flash_attention_varlen_cpu.py, which builds it with the host compiler under -fsanitize=address,undefined.
// stdin, one problem per line:  heads kv_heads window_left window_right n_seqs cu_q[0..n_seqs] cu_kv[0..n_seqs]
// stdout per problem:           "E <message>" when flash_varlen_check refuses it, otherwise "P <n_records>" and one line per record:
//                               q_start len_q kv_start len_kv q0 kt0 kt1
#include "brn_flash_varlen_plan.h"
#include <iostream>

int main() {
    int heads, kv_heads, wl, wr, n;
    while (std::cin >> heads >> kv_heads >> wl >> wr >> n) {
        std::vector<int> cq(n + 1), ckv(n + 1);
        for (int& x : cq) std::cin >> x;
        for (int& x : ckv) std::cin >> x;
        if (!std::cin) return 2;
        const std::string bad = brn::flash_varlen_check(cq.data(), ckv.data(), n, heads, kv_heads, wl, wr);
        if (!bad.empty()) {
            std::cout << "E " << bad << "\n";
            continue;
        }
        const std::vector<brn::FaVarlenRecord> recs = brn::flash_varlen_plan(cq.data(), ckv.data(), n, heads, kv_heads, wl, wr);
        std::cout << "P " << recs.size() << "\n";
        for (const brn::FaVarlenRecord& r : recs) {
            if (r.reserved != 0) return 3;
            std::cout << r.q_start << ' ' << r.len_q << ' ' << r.kv_start << ' ' << r.len_kv << ' ' << r.q0 << ' ' << r.kt0 << ' ' << r.kt1 << "\n";
        }
    }
    return 0;
}
