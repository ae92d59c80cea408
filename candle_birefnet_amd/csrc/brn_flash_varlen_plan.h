// brn_flash_varlen_plan.h — the host side of brn_flash_attention_varlen_forward that needs no HIP: the checks of the two cu_seqlens arrays
// and the table of workgroup records the kernels of kernels/flash_attention.hip read (form FA_VARLEN).  Included by brn_ops.cpp, by the
// kernels (for the record alone) and by the stand-alone program of tests/test_flash_attention_varlen_cpu.py.  DESIGN.md 3.2g.
#pragma once
#include <algorithm>
#include <cstdio>
#include <string>
#include <vector>

namespace brn {

constexpr int FA_VARLEN_ROWS = 64;       // packed rows per record (FA_BQ) and keys per K / V tile (FA_T)
constexpr int FA_VARLEN_MAX_LEN = 65536;

// One tile of 64 packed rows of one sequence; a workgroup per (record, K / V head).  Packed rows as in fa_block_gqa: the G * len_q rows of
// a K / V head's group, query-major (row r = query r / G of the group's head r % G).  32 bytes, read with wave-uniform loads.
struct FaVarlenRecord {
    int q_start, len_q;      // the sequence's rows of q / y: q_start .. q_start + len_q - 1
    int kv_start, len_kv;    // the sequence's rows of k / v
    int q0;                  // the tile's first packed row
    int kt0, kt1;            // the K / V tiles it walks: kt0 .. kt1 - 1
    int reserved;            // 0
};

// A window side of FA_VARLEN_MAX_LEN or more reaches past every sequence: it is the side at FA_VARLEN_MAX_LEN, bit for bit (lo stays 0
// because query + off <= len_kv - 1 < 65536, hi stays len_kv because off >= 0 with a window).  The entry clamps both sides with this
// before they reach the plan and the kernels, whose int arithmetic on query + off + window_right + 1 then stays below 2^18.
inline int fa_varlen_clamp_window(int w) { return std::min(w, FA_VARLEN_MAX_LEN); }

// a row's first visible key and its first excluded key after them: key j takes part exactly when lo <= j < hi (off = len_kv - len_q)
inline int fa_varlen_lo(int query, int off, int wl) { return wl < 0 ? 0 : std::max(0, query + off - wl); }
inline int fa_varlen_hi(int query, int off, int wr, int len_kv) { return wr < 0 ? len_kv : (int)std::min<long long>(len_kv, (long long)query + off + wr + 1); }

// Every limit on the content of cu_seqlens_q / cu_seqlens_kv (n_seqs + 1 ints each, n_seqs >= 1, heads % kv_heads == 0 checked by the
// caller): an empty string, or the message naming the first limit broken.  Nothing else reads the arrays before this passed.
inline std::string flash_varlen_check(const int* cu_q, const int* cu_kv, int n_seqs, int heads, int kv_heads, int wl, int wr) {
    char buf[256];
    if (cu_q[0] != 0 || cu_kv[0] != 0) {
        snprintf(buf, sizeof buf, "cu_seqlens_q[0] %d, cu_seqlens_kv[0] %d (cu_seqlens must start at 0)", cu_q[0], cu_kv[0]);
        return buf;
    }
    const long long G = heads / kv_heads;
    long long tiles = 0;
    for (int s = 0; s < n_seqs; ++s) {
        const long long lq = (long long)cu_q[s + 1] - cu_q[s], lkv = (long long)cu_kv[s + 1] - cu_kv[s];
        if (lq < 0 || lkv < 0) {
            snprintf(buf, sizeof buf, "sequence %d has a negative length (cu_seqlens must be non-decreasing)", s);
            return buf;
        }
        if (lq > FA_VARLEN_MAX_LEN || lkv > FA_VARLEN_MAX_LEN) {
            snprintf(buf, sizeof buf, "sequence %d: len_q %lld, len_kv %lld unsupported (every len_q, len_kv <= 65536)", s, lq, lkv);
            return buf;
        }
        if (lq >= 1 && lkv < 1) {
            snprintf(buf, sizeof buf, "sequence %d has queries and no keys (len_kv >= 1 wherever len_q >= 1)", s);
            return buf;
        }
        if (lq >= 1 && (wl >= 0 || wr >= 0) && lkv < lq) {
            snprintf(buf, sizeof buf, "sequence %d: a window requires len_kv >= len_q (len_q %lld, len_kv %lld)", s, lq, lkv);
            return buf;
        }
        if (G * lq > 0x7fffffffLL) {
            snprintf(buf, sizeof buf, "sequence %d: len_q %lld too large with G = %lld (G * len_q < 2^31)", s, lq, G);
            return buf;
        }
        tiles += (G * lq + FA_VARLEN_ROWS - 1) / FA_VARLEN_ROWS;
    }
    if (cu_q[n_seqs] < 1) return "no queries (total_q >= 1)";
    if (tiles * kv_heads > 0x7fffffffLL) {
        snprintf(buf, sizeof buf, "%lld tiles of 64 packed rows x kv_heads %d too large (packed-row tiles * kv_heads < 2^31)", tiles, kv_heads);
        return buf;
    }
    return std::string();
}

// The records of a call that passed flash_varlen_check, ordered by kt1 - kt0 descending (stable): the longest walks first, the launch
// ends on the short workgroups.  The bits do not depend on this order.
inline std::vector<FaVarlenRecord> flash_varlen_plan(const int* cu_q, const int* cu_kv, int n_seqs, int heads, int kv_heads, int wl, int wr) {
    wl = fa_varlen_clamp_window(wl); wr = fa_varlen_clamp_window(wr);
    const int G = heads / kv_heads;
    std::vector<FaVarlenRecord> recs;
    for (int s = 0; s < n_seqs; ++s) {
        const int lq = cu_q[s + 1] - cu_q[s], lkv = cu_kv[s + 1] - cu_kv[s], off = lkv - lq;
        const long long rows = (long long)G * lq;
        for (long long q0 = 0; q0 < rows; q0 += FA_VARLEN_ROWS) {
            const int qa = (int)(q0 / G), qb = (int)(std::min(q0 + FA_VARLEN_ROWS - 1, rows - 1) / G);   // the tile's first and last query
            FaVarlenRecord r{};
            r.q_start = cu_q[s]; r.len_q = lq; r.kv_start = cu_kv[s]; r.len_kv = lkv;
            r.q0 = (int)q0;
            r.kt0 = fa_varlen_lo(qa, off, wl) / FA_VARLEN_ROWS;                              // lo and hi do not fall along a tile
            r.kt1 = (fa_varlen_hi(qb, off, wr, lkv) + FA_VARLEN_ROWS - 1) / FA_VARLEN_ROWS;
            recs.push_back(r);
        }
    }
    std::stable_sort(recs.begin(), recs.end(), [](const FaVarlenRecord& a, const FaVarlenRecord& b) { return a.kt1 - a.kt0 > b.kt1 - b.kt0; });
    return recs;
}

}  // namespace brn
