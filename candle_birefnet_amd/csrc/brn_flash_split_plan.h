// brn_flash_split_plan.h — the host side of brn_flash_attention_splitkv_forward that needs no HIP: how a call's K / V tiles are split
// between workgroups and how large its workspace is.  brn_flash_attention_splitkv_plan and the entry both call flash_split_plan, so what
// the plan reports is what the call does.  Every value is a function of the call's integer arguments; no device property is read.
// DESIGN.md 3.2h.
#pragma once
#include <algorithm>
#include <cstddef>

namespace brn {

constexpr int FA_SPLIT_TILE = 64;              // keys per K / V tile (FA_T), packed rows per workgroup (FA_BQ)
constexpr int FA_SPLIT_MAX = 1024;             // the largest kv_splits a caller may ask for
// the automatic rule (kv_splits == 0).  A launch whose base grid has fewer workgroups than FA_SPLIT_FILL_WGS counts as under-filled and
// is split until the grid reaches it, but never into splits of fewer than FA_SPLIT_MIN_TILES K / V tiles.  Both values come from the
// sweep of DESIGN.md 3.2h on an MI355X (256 CUs): two workgroups per CU is where the decode rows stop gaining (a grid of 256 is up to
// 27 % slower on the memory-bound 16 x 1 / 4096 row, a grid of 1024 at most 4 % faster), and a split of one tile loses to a split
// of two on the only row short enough to tell (1 x 1 / 4096).
constexpr int FA_SPLIT_FILL_WGS = 512;
constexpr int FA_SPLIT_MIN_TILES = 2;

struct FaSplitPlan {
    int S;                    // the splits the call really uses: no empty trailing split, S <= kv_splits
    int tps;                  // K / V tiles per split: split s owns tiles s * tps .. min((s + 1) * tps, nkt) - 1
    long long base;           // workgroups of the unsplit grid: batch * kv_heads * ceil(G * seq_q / 64); the launch has base * S
    size_t workspace_floats;  // S * R * (head_dim + 1), R = batch * heads * seq_q (not needed, and not touched, when S == 1)
};

// the splits the automatic rule asks for (before flash_split_plan normalises them)
inline int flash_split_auto(long long base, int nkt) {
    if (base >= FA_SPLIT_FILL_WGS) return 1;
    const long long want = (FA_SPLIT_FILL_WGS + base - 1) / base;
    const long long most = std::max(1, nkt / FA_SPLIT_MIN_TILES);
    return (int)std::min<long long>(std::min(want, most), FA_SPLIT_MAX);
}

// arguments already checked by the caller (every size >= 1, heads % kv_heads == 0, 0 <= kv_splits <= FA_SPLIT_MAX)
inline FaSplitPlan flash_split_plan(int batch, int seq_q, int seq_kv, int heads, int kv_heads, int head_dim, int kv_splits) {
    FaSplitPlan pl;
    const long long rows = (long long)(heads / kv_heads) * seq_q;
    pl.base = (long long)batch * kv_heads * ((rows + FA_SPLIT_TILE - 1) / FA_SPLIT_TILE);
    const int nkt = (seq_kv + FA_SPLIT_TILE - 1) / FA_SPLIT_TILE;
    const int ask = kv_splits ? kv_splits : flash_split_auto(pl.base, nkt);
    pl.tps = (nkt + ask - 1) / ask;
    pl.S = (nkt + pl.tps - 1) / pl.tps;
    const size_t R = (size_t)batch * heads * seq_q;
    pl.workspace_floats = (size_t)pl.S * R * ((size_t)head_dim + 1);
    return pl;
}

}  // namespace brn
