// brn_flash_paged_varlen_plan.h — what brn_flash_attention_paged_varlen_forward and brn_kv_cache_append_varlen need that needs no HIP:
// the rule that makes a device-resident cu_seqlens_q harmless, the tile count of a sequence, the bound the host sizes the grid with,
// and the layout of the device-side plan.  Included by brn_ops.cpp (the bound, the plan's size), by the kernels (the rule: the plan
// kernel of kernels/kv_cache.hip evaluates exactly these functions) and by the stand-alone program of
// tests/test_flash_attention_paged_varlen_cpu.py (flash_paged_varlen_plan_ref, the rule applied serially).  DESIGN.md 3.2m.
//
// The rule.  cu is [n_seqs + 1] int32 of UNVALIDATED device data; total_q is the capacity of the pack.
//   c_i = min(max(cu[i], 0), total_q)                 fa_pv_clamp
//   s_b = max over i <= b of c_i                      the running maximum: non-decreasing, 0 <= s_b <= total_q, whatever cu holds
//   sequence b owns tokens s_b .. s_{b+1} - 1         n_b = s_{b+1} - s_b >= 0; the sequences are disjoint and ordered
//   tiles_b = ceil(G * n_b / 64)                      fa_pv_tiles: tiles of 64 packed rows (fa_block_gqa's rows), never straddling sequences
// Tokens outside [s_0, s_{n_seqs}) are padding: no kernel writes anything for them.
// The plan, in plan_workspace: starts[0 .. n_seqs] = s_b, then tile_prefix[0 .. n_seqs] with tile_prefix[b] = sum of tiles_i over i < b
// (tile_prefix[n_seqs] = the real tile count T <= T_max).  2 * (n_seqs + 1) ints.
#pragma once
#include <cstddef>

namespace brn {

constexpr int FA_PV_ROWS = 64;                 // packed rows per tile (FA_BQ)
constexpr int FA_PV_MAX_SEQS = 65536;

constexpr int fa_pv_clamp(int c, int total_q) { return c < 0 ? 0 : (c > total_q ? total_q : c); }
constexpr int fa_pv_max(int a, int b) { return a > b ? a : b; }
// G * n < 2^31 is the entry's limit on G * total_q; the sum is formed in 64 bits all the same
constexpr int fa_pv_tiles(int G, int n) { return (int)(((long long)G * n + FA_PV_ROWS - 1) / FA_PV_ROWS); }

// T_max: every pack of at most total_q tokens in n_seqs sequences has sum_b ceil(G n_b / 64) <= (G * total_q + 63 * min(n_seqs, total_q)) / 64,
// since ceil(x / 64) <= (x + 63) / 64 and at most min(n_seqs, total_q) sequences are not empty
constexpr long long fa_pv_max_tiles(int G, int total_q, int n_seqs) {
    return ((long long)G * total_q + 63LL * (n_seqs < total_q ? n_seqs : total_q)) / FA_PV_ROWS;
}
constexpr size_t fa_pv_plan_ints(int n_seqs) { return 2 * ((size_t)n_seqs + 1); }
// where the two arrays of the plan start
constexpr size_t fa_pv_starts_at() { return 0; }
constexpr size_t fa_pv_tiles_at(int n_seqs) { return (size_t)n_seqs + 1; }

// the rule applied serially: what the plan kernel leaves in plan_workspace
inline void flash_paged_varlen_plan_ref(const int* cu, int n_seqs, int total_q, int G, int* plan) {
    int* starts = plan + fa_pv_starts_at();
    int* tiles = plan + fa_pv_tiles_at(n_seqs);
    int run = 0;
    for (int i = 0; i <= n_seqs; ++i) {
        run = fa_pv_max(run, fa_pv_clamp(cu[i], total_q));
        starts[i] = run;
    }
    tiles[0] = 0;
    for (int b = 0; b < n_seqs; ++b) tiles[b + 1] = tiles[b] + fa_pv_tiles(G, starts[b + 1] - starts[b]);
}

}  // namespace brn
