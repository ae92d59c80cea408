// flash_attention.hip — q/k/v attention for long sequences (brn_flash_attention_forward, brn_flash_attention_bias_forward):
//   y[b,h] = softmax_rows( scale * (q[b,h] k[b,h]^T [+ bias[b % n_bias, h]])  [causal: key j takes part in query i's row exactly when j <= i] ) v[b,h]
// the plain flash_attention(&q, &k, &v, causal) of the reference's flash-attn dependency (examples/bench_flash_attn.rs:39-53), head_dim
// 32 / 64 / 128, 1 <= seq <= 65536, q and k/v of different lengths, in either the [batch, seq, heads, head_dim] or the
// [batch, heads, seq, head_dim] layout: the kernels take element strides (batch entry, head, sequence position; head_dim contiguous).
// It is the sibling of kernels/attention_bias.hip, which holds a whole score row of <= 144 keys in registers; here the row never exists.
//
// One workgroup = one (batch entry, head, tile of FA_BQ = 64 queries) = 4 waves; one wave = 16 queries.  K and V are walked in tiles of
// FA_T = 64 keys staged in LDS (single-buffered; the NEXT tile's global loads are issued into registers before the current tile is
// computed, so they fly under the MFMAs and are written to LDS after the barrier that ends the tile).  Per wave and tile, the MFMA
// formulation, tile map and LDS images of kernels/attention_mfma.h:
//   S^T[key][query] = K . Q^T            4 key sub-tiles of 16
//   online softmax                       scores * (scale * log2 e); excluded keys -> -3e38; tile maximum in-lane then across the 4 lane
//                                        groups (shfl_xor 16, 32); m_new = max(m, tile max); alpha = exp2(m - m_new) rescales the
//                                        running sum l and the O accumulators; numerators exp2(s - m_new); l += the lane's UNROUNDED
//                                        numerators (a lane's l is a partial sum over its keys: alpha is the same in the 4 lanes of
//                                        a query, so the 4 partials are added once, after the last tile)
//   O^T[d][query] += V^T . P^T
// m, l and O^T (head_dim / 16 accumulators of 4 registers) live in registers for the whole walk.  There is no split over keys between
// workgroups, no atomics, nothing shared between workgroups: an output row depends only on its own (batch entry, head), and the bits
// depend neither on `batch` nor on the grid.  Every loop bound is a function of the arguments.
// Ragged edges: K / V rows past seq_kv are ZEROS in LDS (their address is clamped to the last real row, the value replaced) and their
// scores are excluded; a pad query computes on the last real row and is never stored; every global address is clamped into the
// (batch entry, head) it belongs to.  Causal: tiles wholly above the workgroup's diagonal are not walked; in the others the keys after
// a lane's query are excluded.  Key 0 is visible to every query, so after the first tile every m is a real score: alpha never sees
// (-3e38) - (-3e38) with a non-zero l behind it, and exp2(excluded - m) is exactly 0 — an excluded key is in neither the maximum nor
// the sum.
// BIAS = true (a bias is given): the [seq_q, seq_kv] fp32 slab of the workgroup's (pattern, head) is streamed beside K and V.  A lane's
// 16 bias values of a tile (fa_load_bias) are issued with that tile's K / V global loads, held in registers under the MFMAs of the tile
// before, and become the initial accumulators of S^T = K . Q^T: the bias joins the unscaled fp32 scores at no instruction, and an
// all-zero bias gives the bits of BIAS = false.  A -inf entry excludes its key (exp2(-inf - m) = 0; it never raises m).  BIAS = false is
// the kernel as it was, instruction for instruction.  No additional LDS.  DESIGN.md 3.2d.
// GQA = true (brn_flash_attention_gqa_forward with kv_heads < heads, or a causal mask over a cache, seq_q < seq_kv): a group of
// G = heads / kv_heads query heads reads one K / V head, and the causal diagonal ends at the last key (key j <= query i + causal_off,
// causal_off = seq_kv - seq_q >= 0, so key 0 stays visible to every row).  One workgroup = one (batch entry, K / V head, tile of 64
// PACKED rows); packed row r of the group's G * seq_q is query r / G of query head (K / V head) * G + r % G (fa_block_gqa, fa_lane).
// Only what a row IS changes — a lane's q and y row, its bias slab and row, its limit; the wave's mask flag; the workgroup's nkt — the
// walk, the LDS images and the arithmetic are those of GQA = false, whose instantiations serve the two older entries as before.  A row's
// bits do not depend on which rows share its tile: a K / V tile wholly past a row's limit leaves alpha = exp2(m - m) = 1 and numerators
// exp2(-3e38 - m) = 0, so the results are those of the plain kernels on K / V repeated G times.  DESIGN.md 3.2f.
// FA_VARLEN (brn_flash_attention_varlen_forward): the third form of the packed-row kernels (FaForm; GQA = false / true above are FA_PLAIN /
// FA_PACKED).  One workgroup = one (record, K / V head); the record (brn_flash_varlen_plan.h, built and validated on the host) names the
// workgroup's sequence of a packed batch (q_start, len_q, kv_start, len_kv), its first packed row and the K / V tiles kt0 .. kt1 - 1 it
// walks.  seq_q, seq_kv and causal_off become the record's len_q, len_kv and off = len_kv - len_q (fa_params), the operand bases gain
// q_start * q_ss and kv_start * kv_ss in 64-bit arithmetic, and every clamp therefore clamps into the row's own sequence.  A row has two
// limits, lo = max(0, query + off - window_left) and hi = min(len_kv, query + off + window_right + 1) (-1: 0 / len_kv): keys outside
// lo .. hi - 1 are excluded (att_exclude4_window), and the wave's mask flag is two-sided (fa_tile_masks_window).  No bias.
// A lower limit breaks "key 0 is visible to every row".  What holds instead: every row sees its diagonal key query + off (the entry
// requires len_kv >= len_q with a window), and a row's visible keys are contiguous.  A row whose lo lies past the tile's kt0 first meets
// wholly excluded K / V tiles, while m is still ATT_NEG.  With ATT_NEG as the excluded score their numerators would be
// exp2(ATT_NEG - ATT_NEG) = 1 and l and O would collect garbage that only alpha = exp2(ATT_NEG - s) = 0 at the row's first real score s
// wipes, and only while that garbage is finite.  So this form excludes with -inf (att_exclude4_window), as a -inf bias entry does: the
// tile maximum is -inf, m stays ATT_NEG, alpha = exp2(0) = 1, the numerators are exp2(-inf - ATT_NEG) = 0 exactly, and l and O stay
// 0 + 0 . V until the row's own first tile; nothing needs wiping (alpha = 0 there multiplies zeros).  Tiles past a row's hi leave
// alpha = 1 and numerators exp2(-inf - m) = 0, as above.  So a row's bits depend on its sequence, query head and window alone, and equal
// those of the bias kernels on that sequence with the window written into the bias as -inf, also for large V.  DESIGN.md 3.2g.
// FA_SPLIT (brn_flash_attention_splitkv_forward): the fourth form.  One workgroup = one (batch entry, K / V head, tile of 64 packed rows,
// split s of S); the rows are those of FA_PACKED (fa_block_gqa on the workgroup's number / S, fa_lane unchanged) and the walk covers K / V
// tiles s tps .. min((s + 1) tps, the tile's causal nkt) - 1 (fa_block_split), started at kt_first as FA_VARLEN's.  A split
// other than the first does not hold key 0, so under the causal mask a row may meet wholly excluded tiles while m is still ATT_NEG: the
// form excludes with -inf exactly as FA_VARLEN does (att_exclude4_window with lo = 0), and such a tile leaves m = ATT_NEG, alpha = 1,
// l = 0, O = 0.  A workgroup whose range is empty (its tile's causal nkt ends before the split starts) decides so workgroup-uniformly
// before the first barrier, writes the empty markers of its real rows and returns.  fa_finish_split stores o * (1 / l) with the
// operations of fa_finish and m + log2(l) from lane group 0: into the workspace (O_part[s][r][d], lse2_part[s][r], r = (batch entry *
// heads + head) * seq_q + query, 64-bit offsets) when S > 1, straight into y (and lse = ln 2 * that) when S == 1; a row with l == 0 gets
// 0 and -inf, selected, never computed as 0 * inf.  flash_split_combine_kernel then merges the S partials of a row in the order
// s = 0 .. S - 1.  No atomics; a row's bits depend on its (batch entry, query head), seq_kv, the mask and tps alone.  DESIGN.md 3.2h.
// FA_PAGED (brn_flash_attention_paged_forward): the fifth form, FA_SPLIT with K / V in the pages of a pool and a length per batch entry that
// lives on the device.  The grid and the split are FA_SPLIT's at seq_kv = max_kv_len.  A workgroup reads its batch entry's kv_lens[b] (one
// scalar load), clamps it to 0 .. max_kv_len, and from there on IS an FA_SPLIT workgroup at seq_kv = len (fa_params): limit, causal_off =
// len - seq_q (it may be negative: rows with no visible key), the tile count and the empty decision all follow.  load_tile finds key t in
// row t % page_size of page block_table[b][t / page_size]: t is clamped to len - 1 BEFORE the table is indexed, so no entry at or past
// ceil(len / page_size) is read, the page number is clamped to 0 .. n_pages - 1 before it becomes an address, and a row at or past len is
// replaced by zeros as the other forms replace a row past seq_kv.  The table entries of tile kt + 2 are loaded (vector loads, a thread's
// own keys: NI entries in the f32 kernel, one per key pair in the 16-bit kernel) just before the K / V loads of tile kt + 1 are issued, so
// a tile's entries are in registers a whole tile before its loads need them and the table's latency is paid once, in the prologue.
// A row with no visible key at all (len 0, or causal with query + len - seq_q < 0) is empty in every split: fa_finish_split gives 0 / -inf
// as before, and flash_split_combine_kernel<true> selects y = 0, lse = -inf for it without forming -inf - -inf.  DESIGN.md 3.2i.
// KV (brn_flash_attention_paged_kv_forward): the type the pool is STORED in, a last template parameter of both kernels; float everywhere
// but in 12 FA_PAGED instantiations, where the pool holds __bf16 or _Float16.  The 16-bit kernel reads a pool of its own type with one
// 16-byte load per (key, 8 d) and carries the bits to LDS unconverted; the fp32 kernel reads either type and widens exactly as it writes
// LDS.  What reaches LDS is what KV = float puts there from the pool widened to fp32 ((E)(float)e == e), so a row carries those bits.
// The table-entry schedule, the clamps and the zero-select are FA_PAGED's; every instantiation with KV = float is the kernel it was,
// instruction for instruction.  DESIGN.md 3.2j.
// KV = fa_e4m3 (brn_flash_attention_paged_fp8_forward): the pool holds OCP e4m3fn BYTES with one fp32 scale per K / V head.  Both kernels
// read 8 bytes per (key, 8 d) with the 16-bit pools' staging maps and widen them in registers, exactly, to the type their LDS image
// holds (v_cvt_pk_f32_fp8, then the kernel's own cast: every e4m3 value is a bf16, an fp16 and an fp32 value), so LDS and everything
// after it see the fp32 pool of the widened bytes.  k_scale[g] joins the score scale once per workgroup (fl32(scale * k_scale[g]) where
// the other forms have scale), v_scale[g] multiplies a row's final y once: in fa_finish_split when S == 1, in
// flash_split_combine_kernel<true, true> when S > 1; partials and lse never see v_scale.  DESIGN.md 3.2k.
// FA_PAGED_VARLEN (brn_flash_attention_paged_varlen_forward): the sixth form, FA_PAGED with a workgroup's rows taken from a device-side
// plan instead of blockIdx arithmetic: a packed batch [total_q, heads, head_dim] of new tokens whose cu_seqlens_q lives on the device.
// paged_varlen_plan_kernel (kernels/kv_cache.hip; the rule: brn_flash_paged_varlen_plan.h) runs first on the stream and leaves the clamped
// starts s_b and the prefix of row tiles per sequence; the grid holds T_max * kv_heads * S workgroups, (row tile, K / V head, split).
// fa_params finds the tile's sequence by bisection of the prefix (scalar loads), returns before the first barrier when the tile is past
// the real count, and otherwise rewrites the arguments into those of an FA_PAGED workgroup of that sequence ALONE: batch 1, seq_q = n_b,
// seq_kv = len_b, causal_off = len_b - n_b, q / y based at token s_b, the table at the sequence's row.  The table schedule, the clamps,
// the zero-select, the staging, the scales and the walk are FA_PAGED's, untouched.  What a row IS stays n_b's business (fa_lane: masks,
// pad rows); WHERE it goes is total_q's: fa_finish_split<.., PV> stores y, lse and the partials at r = head * total_q + s_b + query of
// R = heads * total_q rows, the split entry's layout at batch 1, seq_q = total_q.  flash_split_combine_kernel<true, VS, PV> runs over
// those R rows and skips the tokens outside [s_0, s_n): padding rows are written by no kernel.  A sequence's bits are those of the FA_PAGED
// kernels called on it alone.  Every instantiation of the five older forms is the kernel it was, instruction for instruction.  DESIGN.md 3.2m.
#include "../brn_kernels.h"
#include "../brn_flash_varlen_plan.h"
#include "../brn_flash_paged_varlen_plan.h"
#include "attention_mfma.h"
#include <type_traits>

namespace brn {
namespace {

constexpr int FA_BQ = 64;            // queries per workgroup: 4 waves x 16
constexpr int FA_T = 64;             // keys per K / V tile
constexpr int FA_THREADS = 256;
static_assert(FA_BQ == FA_VARLEN_ROWS && FA_T == FA_VARLEN_ROWS, "the records of brn_flash_varlen_plan.h are tiles of FA_BQ rows and FA_T keys");
constexpr int FA_VT_LD = 72;         // 16-bit kernel: elements per LDS row of V^T (36 dwords: conflict-free 8-byte reads, 2-way 4-byte writes)

// the three forms of the kernels: a workgroup per (batch entry, head, 64 queries); per (batch entry, K / V head, 64 packed rows); per
// (record of a packed batch, K / V head), with a window; per (batch entry, K / V head, 64 packed rows, split over keys); the same over pages
// (FA_PAGED_VARLEN: FA_PAGED with the workgroup's rows taken from the device-side plan of a packed batch)
enum FaForm { FA_PLAIN = 0, FA_PACKED = 1, FA_VARLEN = 2, FA_SPLIT = 3, FA_PAGED = 4, FA_PAGED_VARLEN = 5 };
// the forms with K / V in the pages of a pool
constexpr bool fa_paged(FaForm f) { return f == FA_PAGED || f == FA_PAGED_VARLEN; }
// the forms whose walk is one split's range and whose finish is fa_finish_split (FA_PAGED: FA_SPLIT at the workgroup's own seq_kv, K / V in pages)
constexpr bool fa_splits(FaForm f) { return f == FA_SPLIT || fa_paged(f); }

// which (batch entry, head, query tile) this workgroup owns, where its operands start and how many K / V tiles it walks
struct FaBlock {
    const float* q; const float* k; const float* v; float* y;
    const float* bias;    // BIAS: the [seq_q, seq_kv] slab of this (bias pattern = batch entry % n_bias, head)
    int q0;               // first query of the tile (GQA: first packed row)
    int nkt;              // K / V tiles to walk: all of them, or (causal) those that reach the tile's last query; FA_VARLEN: one past the last (kt1)
    int kt0;              // FA_VARLEN, FA_SPLIT: the first K / V tile to walk (the other forms start at 0)
    int G, h0, rem;       // GQA: query heads per K / V head, the group's first query head, real rows after q0 (the tile's last real row is q0 + min(63, rem))
};
// GQA: the workgroup is (batch entry, K / V head, tile of 64 packed rows); q, y and bias point at the batch entry (pattern), the head is a
// lane's own (fa_lane); k and v at the K / V head
template <bool BIAS>
__device__ __forceinline__ FaBlock fa_block_gqa(const FlashAttentionParams& p, const unsigned wg) {   // wg: blockIdx.x; FA_SPLIT: blockIdx.x / S
    FaBlock r;
    r.G = p.heads / p.kv_heads;
    const int rows = r.G * p.seq_q;                      // < 2^31 (launch_flash_attention)
    const int nqt = (rows - 1) / FA_BQ + 1;
    // the grid order of fa_block, over (batch entry, K / V head): causal = longest tiles first
    int bh, qt;
    if (p.causal) {
        const unsigned nbh = (unsigned)(p.batch * p.kv_heads);
        qt = nqt - 1 - (int)(wg / nbh); bh = (int)(wg % nbh);
    } else {
        bh = (int)(wg / (unsigned)nqt); qt = (int)(wg - (unsigned)bh * (unsigned)nqt);
    }
    const int b = bh / p.kv_heads, kvh = bh - b * p.kv_heads;
    r.q = p.q + b * p.q_sb;
    r.y = p.y + b * p.q_sb;
    r.k = p.k + b * p.kv_sb + kvh * p.kv_sh;
    r.v = p.v + b * p.kv_sb + kvh * p.kv_sh;
    r.bias = nullptr;
    if constexpr (BIAS) r.bias = p.bias + (b % p.n_bias) * p.b_sp;
    r.h0 = kvh * r.G;
    r.q0 = qt * FA_BQ;
    r.rem = rows - 1 - r.q0;
    r.kt0 = 0;
    r.nkt = (p.seq_kv + FA_T - 1) / FA_T;
    // the tile's last real row holds its last query, whose last visible key is query + causal_off <= seq_kv - 1
    if (p.causal) r.nkt = min(r.nkt, ((r.q0 + min(FA_BQ - 1, r.rem)) / r.G + p.causal_off) / FA_T + 1);
    return r;
}
// FA_VARLEN: the workgroup is (record, K / V head); the record's sequence is the "batch entry", its own rows of q / y / k / v the only
// ones any address of the workgroup can reach (64-bit offsets: a pack may hold more than 2^31 elements)
__device__ __forceinline__ FaBlock fa_block_varlen(const FlashAttentionParams& p, const FaVarlenRecord& rec) {
    FaBlock r;
    r.G = p.heads / p.kv_heads;
    const int kvh = (int)(blockIdx.x % (unsigned)p.kv_heads);
    r.q = p.q + (long)rec.q_start * p.q_ss;
    r.y = p.y + (long)rec.q_start * p.q_ss;
    r.k = p.k + (long)rec.kv_start * p.kv_ss + kvh * p.kv_sh;
    r.v = p.v + (long)rec.kv_start * p.kv_ss + kvh * p.kv_sh;
    r.bias = nullptr;
    r.h0 = kvh * r.G;
    r.q0 = rec.q0;
    r.rem = r.G * rec.len_q - 1 - rec.q0;
    r.kt0 = rec.kt0;
    r.nkt = rec.kt1;
    return r;
}
// FA_SPLIT: the S splits of a (batch entry, K / V head, row tile) are neighbours in the grid; the tile is fa_block_gqa's, the walk the
// part of it that split s owns: K / V tiles s * tps .. min((s + 1) * tps, nkt) - 1, empty (kt0 >= nkt) where the causal nkt ends before
__device__ __forceinline__ FaBlock fa_block_split(const FlashAttentionParams& p) {
    const unsigned S = (unsigned)p.kv_splits, wg = blockIdx.x / S;
    FaBlock r = fa_block_gqa<false>(p, wg);
    r.kt0 = (int)(blockIdx.x - wg * S) * p.tiles_per_split;
    r.nkt = min(r.nkt, r.kt0 + p.tiles_per_split);
    return r;
}
// FA_PAGED_VARLEN: the workgroup is (row tile of the plan, K / V head, split); fa_params has turned the arguments into those of the tile's
// own sequence (q, y and the table based at it, batch 1, seq_q = n_b, seq_kv = len_b) and left the tile's first packed row in rec.q0.
// From there it is fa_block_gqa's tile and fa_block_split's range, restated without the grid arithmetic
__device__ __forceinline__ FaBlock fa_block_paged_varlen(const FlashAttentionParams& p, const FaVarlenRecord& rec) {
    const unsigned S = (unsigned)p.kv_splits, wg = blockIdx.x / S;
    const int kvh = (int)(wg % (unsigned)p.kv_heads);
    FaBlock r;
    r.G = p.heads / p.kv_heads;
    r.q = p.q; r.y = p.y;
    r.k = p.k + kvh * p.kv_sh;
    r.v = p.v + kvh * p.kv_sh;
    r.bias = nullptr;
    r.h0 = kvh * r.G;
    r.q0 = rec.q0;
    r.rem = r.G * p.seq_q - 1 - r.q0;
    r.nkt = (p.seq_kv + FA_T - 1) / FA_T;
    if (p.causal) r.nkt = min(r.nkt, ((r.q0 + min(FA_BQ - 1, r.rem)) / r.G + p.causal_off) / FA_T + 1);
    r.kt0 = (int)(blockIdx.x - wg * S) * p.tiles_per_split;
    r.nkt = min(r.nkt, r.kt0 + p.tiles_per_split);
    return r;
}
// FA_SPLIT: the workgroup's split and its batch entry (the grid order of fa_block_gqa, restated for the one value FaBlock does not keep)
struct FaSplit { int b, split; };
__device__ __forceinline__ FaSplit fa_split_of(const FlashAttentionParams& p) {
    const unsigned S = (unsigned)p.kv_splits, wg = blockIdx.x / S;
    const int nqt = (p.heads / p.kv_heads * p.seq_q - 1) / FA_BQ + 1;
    const int bh = p.causal ? (int)(wg % (unsigned)(p.batch * p.kv_heads)) : (int)(wg / (unsigned)nqt);
    return FaSplit{bh / p.kv_heads, (int)(blockIdx.x - wg * S)};
}
template <bool BIAS, FaForm FORM>
__device__ __forceinline__ FaBlock fa_block(const FlashAttentionParams& p) {
    if constexpr (fa_splits(FORM)) return fa_block_split(p);
    if constexpr (FORM == FA_PACKED) return fa_block_gqa<BIAS>(p, blockIdx.x);
    const int nqt = (p.seq_q + FA_BQ - 1) / FA_BQ;
    // not causal: the query tiles of a (batch entry, head) are neighbours in the grid (they walk the same K and V).  Causal: tile qt walks
    // qt + 1 K / V tiles, so the grid is ordered by query tile, last (longest) first: the launch ends on the short workgroups
    int bh, qt;
    if (p.causal) {
        const unsigned nbh = (unsigned)(p.batch * p.heads);
        qt = nqt - 1 - (int)(blockIdx.x / nbh); bh = (int)(blockIdx.x % nbh);
    } else {
        bh = (int)(blockIdx.x / (unsigned)nqt); qt = (int)(blockIdx.x - (unsigned)bh * (unsigned)nqt);
    }
    const int b = bh / p.heads, h = bh - b * p.heads;
    FaBlock r;
    r.q = p.q + b * p.q_sb + h * p.q_sh;
    r.y = p.y + b * p.q_sb + h * p.q_sh;
    r.k = p.k + b * p.kv_sb + h * p.kv_sh;
    r.v = p.v + b * p.kv_sb + h * p.kv_sh;
    r.bias = nullptr;
    if constexpr (BIAS) r.bias = p.bias + (b % p.n_bias) * p.b_sp + h * p.b_sh;
    r.q0 = qt * FA_BQ;
    r.nkt = (p.seq_kv + FA_T - 1) / FA_T;
    if (p.causal) r.nkt = min(r.nkt, min(r.q0 + FA_BQ - 1, p.seq_q - 1) / FA_T + 1);
    r.G = 1; r.h0 = h; r.rem = p.seq_q - 1 - r.q0;         // (not read)
    r.kt0 = 0;
    return r;
}

// What a lane's row of the workgroup's tile is.  Row = the query q0 + 16 wave + li of the workgroup's head; GQA: the PACKED row of that
// number among the G * seq_q rows of the K / V head's group, query-major: query = row / G, query head = h0 + row % G, so a wave's 16
// rows may straddle queries and heads, the K / V tile in LDS serves all G heads, and the causal diagonal of a tile spans 64 / G queries.
// A pad row (past the last real one) computes on the last real row and is never stored.
struct FaLane {
    const float* q;       // the row of q (head_dim floats)
    int yrow;             // where the row goes in y (fa_lane_y, after the walk): the UNCLAMPED query; GQA: the packed row, -1 for a pad row
    const float* bias;    // BIAS: the [seq_q, seq_kv] slab of the row's own head, and
    long brow;            //       the row's offset in it: query * seq_kv
    int limit;            // the row's first excluded key: seq_kv, or (causal) query + causal_off + 1
    int wave_row0;        // the first query of the wave's 16 rows (clamped; GQA: + causal_off): the wave's smallest limit - 1 under the causal mask (fa_tile_masks)
                          // FA_VARLEN: the wave's smallest limit itself (its first row's; fa_tile_masks_window)
    int lo, wave_lo;      // FA_VARLEN: the row's first visible key, and the wave's largest (its last row's)
};
template <FaForm FORM>
__device__ __forceinline__ FaLane fa_lane(const FlashAttentionParams& p, const FaBlock& blk, int wave, int li) {
    FaLane r;
    r.lo = 0; r.wave_lo = 0;
    if constexpr (FORM == FA_VARLEN) {
        // p.seq_q / p.seq_kv / p.causal_off: the record's len_q / len_kv / len_kv - len_q (fa_params).  Queries do not fall along
        // the packed rows, so neither do lo and hi: the wave's smallest hi is its first row's, its largest lo its last row's
        const int lr = wave * 16 + li;
        const int row = blk.q0 + min(lr, blk.rem);
        const int query = row / blk.G, head = blk.h0 + (row - query * blk.G);
        r.q = blk.q + (head * p.q_sh + query * p.q_ss);
        r.yrow = lr <= blk.rem ? row : -1;
        r.bias = nullptr; r.brow = 0;
        const int wl = p.window_left, wr = p.window_right;
        r.lo = wl < 0 ? 0 : max(0, query + p.causal_off - wl);
        r.limit = wr < 0 ? p.seq_kv : min(p.seq_kv, query + p.causal_off + wr + 1);
        const int qa = (blk.q0 + min(wave * 16, blk.rem)) / blk.G, qb = (blk.q0 + min(wave * 16 + 15, blk.rem)) / blk.G;
        r.wave_row0 = wr < 0 ? p.seq_kv : min(p.seq_kv, qa + p.causal_off + wr + 1);
        r.wave_lo = wl < 0 ? 0 : max(0, qb + p.causal_off - wl);
    } else if constexpr (FORM == FA_PACKED || fa_splits(FORM)) {              // (FA_SPLIT, FA_PAGED have no bias: blk.bias is null and never read)
        const int lr = wave * 16 + li;
        const int row = blk.q0 + min(lr, blk.rem);
        const int query = row / blk.G, head = blk.h0 + (row - query * blk.G);
        const long off = head * p.q_sh + query * p.q_ss;
        r.q = blk.q + off;
        r.yrow = lr <= blk.rem ? row : -1;
        r.bias = blk.bias + head * p.b_sh;
        r.brow = (long)query * p.seq_kv;
        r.limit = p.causal ? min(p.seq_kv, query + p.causal_off + 1) : p.seq_kv;
        r.wave_row0 = (blk.q0 + min(wave * 16, blk.rem)) / blk.G + p.causal_off;
    } else {
        const int query = blk.q0 + wave * 16 + li, qrow = min(query, p.seq_q - 1);
        r.q = blk.q + qrow * p.q_ss;
        r.yrow = query;
        r.bias = blk.bias;
        r.brow = (long)qrow * p.seq_kv;
        r.limit = p.causal ? min(p.seq_kv, qrow + 1) : p.seq_kv;
        r.wave_row0 = min(blk.q0 + wave * 16, p.seq_q - 1);
    }
    return r;
}
// the row of y, null for a pad row
template <FaForm FORM>
__device__ __forceinline__ float* fa_lane_y(const FlashAttentionParams& p, const FaBlock& blk, const FaLane& ln) {
    if constexpr (FORM != FA_PLAIN) {
        // (query and head are taken from the row a second time: one register across the walk, as the plain kernels have)
        const int row = max(ln.yrow, 0), query = row / blk.G, head = blk.h0 + (row - query * blk.G);
        return ln.yrow >= 0 ? blk.y + (head * p.q_sh + query * p.q_ss) : nullptr;
    } else return ln.yrow < p.seq_q ? blk.y + ln.yrow * p.q_ss : nullptr;
}

// The bias values a lane adds to its scores of the K / V tile at key0: for sub-tile s the 4 consecutive floats of keys
// key0 + 16 s + 4 g + 0..3 in row `row` (= the lane's clamped query * seq_kv, 64-bit) of the slab.  Every address stays inside the slab:
// seq_kv % 4 == 0 -> one 16-byte load per sub-tile, its first key clamped to seq_kv - 4 (the slab base is 16-byte aligned and row and
// key are multiples of 4, so the address is; a group of 4 is then wholly real or wholly past seq_kv); otherwise 4-byte loads with each
// key clamped to seq_kv - 1.  The choice is a function of seq_kv alone (wave-uniform).  What a clamped load returns belongs to an
// excluded key and is replaced before the maximum.  No address depends on a bias value.
// A/B switch (make EXTRA_CXXFLAGS=-DFA_BIAS_NONTEMPORAL=1): the 16-byte bias loads as non-temporal loads.  Every bias element is read once by
// one lane, so it has nothing to gain from the caches; DESIGN.md 3.2d has what the two builds measured.
#ifndef FA_FORCE_PACKED
#define FA_FORCE_PACKED 0
#endif
#ifndef FA_BIAS_NONTEMPORAL
#define FA_BIAS_NONTEMPORAL 0
#endif
__device__ __forceinline__ void fa_load_bias(f32x4 (&bv)[FA_T / 16], const float* slab, long row, int key0, int g, int seq_kv) {
    const float* rp = slab + row;
    if ((seq_kv & 3) == 0) {
#pragma unroll
        for (int s = 0; s < FA_T / 16; ++s) {
            const f32x4* src = reinterpret_cast<const f32x4*>(rp + min(key0 + s * 16 + g * 4, seq_kv - 4));
#if FA_BIAS_NONTEMPORAL
            bv[s] = __builtin_nontemporal_load(src);
#else
            bv[s] = *src;
#endif
        }
    } else {
#pragma unroll
        for (int s = 0; s < FA_T / 16; ++s) {
#pragma unroll
            for (int r = 0; r < 4; ++r) bv[s][r] = rp[min(key0 + s * 16 + g * 4 + r, seq_kv - 1)];
        }
    }
}

// One tile of the online softmax.  st: the lane's raw scores of keys key0 + 16 s + 4 g + r (s = sub-tile, r = register) of its query;
// limit: the lane's first excluded key (seq_kv, or query + 1 under the causal mask); mask: whether this tile can hold an excluded key
// for some lane of the wave (wave-uniform).  Leaves the numerators in st, updates m and l, returns alpha.
// WINDOW (FA_VARLEN): the keys before `lo` are excluded too (att_exclude4_window).
template <bool WINDOW = false>
__device__ __forceinline__ float fa_softmax_tile(f32x4 (&st)[FA_T / 16], float sc2, bool mask, int key0, int g, int limit, float& m, float& l, int lo = 0) {
    float mx = ATT_NEG;
#pragma unroll
    for (int s = 0; s < FA_T / 16; ++s) {
        att_scale4(st[s], sc2);
        if constexpr (WINDOW) {
            if (mask) att_exclude4_window(st[s], key0 + s * 16 + g * 4, lo, limit);
        } else if (mask) att_exclude4(st[s], key0 + s * 16 + g * 4, limit);
        mx = att_max4(mx, st[s]);
    }
    const float mn = fmaxf(m, att_group_max(mx));
    const float alpha = __builtin_amdgcn_exp2f(m - mn);
    float sum = 0.f;
#pragma unroll
    for (int s = 0; s < FA_T / 16; ++s) att_exp2_sum4(st[s], mn, sum);
    m = mn;
    l = l * alpha + sum;
    return alpha;
}
// whether the tile at key0 can hold an excluded key for a lane of this wave (rows: the wave's first query row, clamped)
__device__ __forceinline__ bool fa_tile_masks(const FlashAttentionParams& p, int key0, int wave_row0) {
    const int lim = p.causal ? min(p.seq_kv, wave_row0 + 1) : p.seq_kv;
    return key0 + FA_T > lim;
}
// FA_VARLEN, two-sided: the tile holds a key from the wave's smallest hi on, or one before the wave's largest lo
__device__ __forceinline__ bool fa_tile_masks_window(int key0, int wave_hi, int wave_lo) { return key0 + FA_T > wave_hi || key0 < wave_lo; }
// FA_VARLEN: the workgroup's record, and the arguments with the record's sequence in place of the call's: seq_q, seq_kv, causal_off
// (= off of the window; it may be negative where there is no window, and is then not read)
// FA_PAGED: the arguments with the workgroup's own sequence length in place of max_kv_len.  kv_lens[b] is unvalidated device data: it is
// clamped to 0 .. max_kv_len here and reaches nothing unclamped.  causal_off = len - seq_q may be negative (rows with no visible key)
template <FaForm FORM>
__device__ __forceinline__ FlashAttentionParams fa_params(const FlashAttentionParams& pa, FaVarlenRecord& rec) {
    if constexpr (FORM == FA_VARLEN) {
        rec = pa.plan[blockIdx.x / (unsigned)pa.kv_heads];           // wave-uniform
        FlashAttentionParams p = pa;
        p.seq_q = rec.len_q; p.seq_kv = rec.len_kv; p.causal_off = rec.len_kv - rec.len_q;
        return p;
    } else if constexpr (FORM == FA_PAGED) {
        FlashAttentionParams p = pa;
        p.seq_kv = min(max(pa.kv_lens[fa_split_of(pa).b], 0), pa.seq_kv);       // workgroup-uniform: one scalar load
        p.causal_off = pa.causal ? p.seq_kv - pa.seq_q : 0;
        return p;
    } else if constexpr (FORM == FA_PAGED_VARLEN) {
        // the workgroup's row tile (blockIdx.x / S / kv_heads) among the plan's: its sequence b is the one whose tile range holds it
        // (bisection of the prefix, workgroup-uniform scalar loads), its first packed row 64 * (tile - prefix[b]).  rec.len_q = 0 tells
        // the kernel that there is no such tile (the grid is sized by T_max) and it returns before its first barrier.  The plan is the
        // library's own, written by paged_varlen_plan_kernel just before; its values are clamped all the same before they bound a row
        FlashAttentionParams p = pa;
        const int n = pa.pv_n_seqs, total_q = pa.pv_total_q;
        const int* starts = pa.pv_plan + fa_pv_starts_at();
        const int* prefix = pa.pv_plan + fa_pv_tiles_at(n);
        const int tile = (int)(blockIdx.x / (unsigned)pa.kv_splits / (unsigned)pa.kv_heads);
        rec = FaVarlenRecord{};
        if (tile >= prefix[n]) return p;
        int lo = 0, hi = n;
        while (hi - lo > 1) {
            const int mid = (lo + hi) >> 1;
            if (prefix[mid] <= tile) lo = mid; else hi = mid;
        }
        const int b = lo;
        const int s_b = min(max(starts[b], 0), total_q), n_b = min(max(starts[b + 1] - s_b, 0), total_q - s_b);
        const long q0 = (long)(tile - prefix[b]) * FA_BQ;
        if (q0 < 0 || q0 >= (long)(pa.heads / pa.kv_heads) * n_b) return p;
        rec.q_start = s_b; rec.len_q = n_b; rec.q0 = (int)q0;
        p.batch = 1; p.seq_q = n_b; p.pv_row0 = s_b;
        p.q = pa.q + (long)s_b * pa.q_ss;
        p.y = pa.y + (long)s_b * pa.q_ss;
        p.block_table = pa.block_table + (long)b * pa.max_pages;
        p.seq_kv = min(max(pa.kv_lens[b], 0), pa.seq_kv);
        p.causal_off = pa.causal ? p.seq_kv - n_b : 0;
        return p;
    } else return pa;
}
// FA_PAGED: where key t (already clamped below the sequence's length) of the workgroup's batch entry lives: its table entry, and the
// offset of its row from the K / V head's base in the pool (64-bit), the page number clamped into the pool
struct FaPages { const int* table; long stride; int lg, mask, last; };
template <FaForm FORM>
__device__ __forceinline__ FaPages fa_pages_of(const FlashAttentionParams& p) {
    // (FA_PAGED_VARLEN: fa_params has based the table at the workgroup's sequence)
    if constexpr (FORM == FA_PAGED_VARLEN) return FaPages{p.block_table, p.page_stride, p.page_log2, (1 << p.page_log2) - 1, p.n_pages - 1};
    else return FaPages{p.block_table + (long)fa_split_of(p).b * p.max_pages, p.page_stride, p.page_log2, (1 << p.page_log2) - 1, p.n_pages - 1};
}
__device__ __forceinline__ int fa_page_entry(const FaPages& pg, int t) { return pg.table[t >> pg.lg]; }
__device__ __forceinline__ long fa_page_row(const FaPages& pg, int entry, int t, long kv_ss) {
    return (long)min(max(entry, 0), pg.last) * pg.stride + (long)(t & pg.mask) * kv_ss;
}
template <bool BIAS, FaForm FORM>
__device__ __forceinline__ FaBlock fa_block_of(const FlashAttentionParams& p, const FaVarlenRecord& rec) {
    if constexpr (FORM == FA_VARLEN) return fa_block_varlen(p, rec);
    else if constexpr (FORM == FA_PAGED_VARLEN) return fa_block_paged_varlen(p, rec);
    else return fa_block<BIAS, FORM>(p);
}
// the 4 partial sums of a query are added, and the query's row of y (null: a pad query) is stored
// BIAS: a row whose every visible key has a -inf bias never saw a real score (m is still ATT_NEG) and comes back NaN, also where excluded
// keys of its tiles left exp2(ATT_NEG - ATT_NEG) = 1 in l
template <int ND, bool BIAS>
__device__ __forceinline__ void fa_finish(float* yrow, int g, const f32x4 (&o)[ND], float l, float m) {
    float inv = 1.0f / att_group_sum(l);
    if constexpr (BIAS) inv = (m > ATT_NEG) ? inv : __builtin_nanf("");
    if (yrow) {
#pragma unroll
        for (int dt = 0; dt < ND; ++dt) att_store_o(yrow + g * 4, dt, o[dt], inv);
    }
}

// FA_SPLIT: the end of a split's walk.  o * (1 / l) with the operations of fa_finish (a partial carries the bits of the gqa entry on the
// split's keys), and m + log2(l) in the base-2 scaled-score domain from lane group 0.  A row that saw no key of the split (l == 0: only
// under the causal mask, or a workgroup with nothing to walk) stores 0 and -inf: inv is SELECTED to 0, 0 * inf is never computed.
// S > 1 (p.o_part): row r = (batch entry * heads + head) * seq_q + query of the workspace's O_part[split] and lse2_part[split], 64-bit
// offsets.  S == 1: the row of y, and lse[r] = ln 2 * (m + log2 l) where lse is wanted.
// VS (the fp8 pool): the S == 1 row of y is fl32(vs * fl32(o * inv)), vs = v_scale of the workgroup's K / V head; a partial is not scaled.
// PV (FA_PAGED_VARLEN): p.seq_q is the sequence's n_b and masks alone; a row's place is r = head * total_q + s_b + query among
// R = heads * total_q rows (the split entry's layout at batch 1, seq_q = total_q), the split the workgroup's own blockIdx.x % S
template <int D, bool VS = false, bool PV = false>
__device__ __forceinline__ void fa_finish_split(const FlashAttentionParams& p, const FaBlock& blk, const FaLane& ln, int g, const f32x4 (&o)[D / 16], float l, float m, float vs = 1.f) {
    const float lsum = att_group_sum(l);
    const bool empty = !(lsum > 0.f);
    const float inv = empty ? 0.f : 1.0f / lsum;
    const float lse2 = empty ? -__builtin_inff() : m + __builtin_amdgcn_logf(lsum);
    if (ln.yrow < 0) return;
    const int row = ln.yrow, query = row / blk.G, head = blk.h0 + (row - query * blk.G);
    const FaSplit sp = PV ? FaSplit{0, (int)(blockIdx.x % (unsigned)p.kv_splits)} : fa_split_of(p);
    const long r = PV ? (long)head * p.pv_total_q + p.pv_row0 + query : ((long)sp.b * p.heads + head) * p.seq_q + query;
    float* dst; float* ldst; float lv = lse2;
    if (p.o_part) {
        const long R = PV ? (long)p.heads * p.pv_total_q : (long)p.batch * p.heads * p.seq_q;
        dst = p.o_part + ((long)sp.split * R + r) * D;
        ldst = p.lse2_part + ((long)sp.split * R + r);
    } else {
        dst = blk.y + (head * p.q_sh + query * p.q_ss);
        ldst = p.lse ? p.lse + r : nullptr;
        lv = lse2 * 0.6931471805599453f;
    }
    if constexpr (VS) {
        if (!p.o_part) {
#pragma unroll
            for (int dt = 0; dt < D / 16; ++dt) *reinterpret_cast<f32x4*>(dst + g * 4 + dt * 16) = (o[dt] * inv) * vs;
            if (g == 0 && ldst) *ldst = lv;
            return;
        }
    }
#pragma unroll
    for (int dt = 0; dt < D / 16; ++dt) att_store_o(dst + g * 4, dt, o[dt], inv);
    if (g == 0 && ldst) *ldst = lv;
}

// ---- KV (brn_flash_attention_paged_kv_forward): the type the pool is stored in, float in every older form.  A 16-bit pool is read with
// 16-byte loads of 8 consecutive d of one key; offsets stay 64-bit and count elements.  fa_kv_base: the workgroup's K / V head in such a
// pool (FaBlock keeps float pointers: blk.k - p.k is the head's offset in elements, whatever an element is).  fa_widen is exact. ----
template <typename KV>
__device__ __forceinline__ const KV* fa_kv_base(const float* pool, const float* head) { return reinterpret_cast<const KV*>(pool) + (head - pool); }
template <typename KV>
__device__ __forceinline__ float fa_widen(KV e) {
    if constexpr (std::is_same<KV, __bf16>::value) return __builtin_bit_cast(float, (unsigned)__builtin_bit_cast(unsigned short, e) << 16);
    else return (float)e;
}
// ---- KV = fa_e4m3: a pool of OCP e4m3fn bytes (bias 7, max 448, no infinities, NaN = 0x7F / 0xFF), read 8 bytes = 8 d of one key at a
// time.  fa_fp8_widen8: the 8 bytes as fp32, exactly (v_cvt_pk_f32_fp8, two bytes each).  fa_fp8_heads: the workgroup's K / V head and
// its two scales (null = 1), two scalar loads; no address is formed from either value. ----
typedef unsigned char fa_e4m3;
__device__ __forceinline__ void fa_fp8_widen8(const vec8<fa_e4m3> b, f32x4& lo, f32x4& hi) {
    const vec2<unsigned> w = __builtin_bit_cast(vec2<unsigned>, b);
    const vec2<float> a0 = __builtin_amdgcn_cvt_pk_f32_fp8((int)w[0], false), a1 = __builtin_amdgcn_cvt_pk_f32_fp8((int)w[0], true);
    const vec2<float> a2 = __builtin_amdgcn_cvt_pk_f32_fp8((int)w[1], false), a3 = __builtin_amdgcn_cvt_pk_f32_fp8((int)w[1], true);
    lo = f32x4{a0[0], a0[1], a1[0], a1[1]};
    hi = f32x4{a2[0], a2[1], a3[0], a3[1]};
}
struct FaFp8Scales { float k, v; };
__device__ __forceinline__ FaFp8Scales fa_fp8_scales(const FlashAttentionParams& p, const FaBlock& blk) {
    const int kvh = blk.h0 / blk.G;                        // workgroup-uniform
    return FaFp8Scales{p.k_scale ? p.k_scale[kvh] : 1.f, p.v_scale ? p.v_scale[kvh] : 1.f};
}

// ---- fp32: v_mfma_f32_16x16x4_f32, an exact fmaf chain per score and per output ----
// LDS: Ks, Vs [64][D + 4] floats (D 128: 66 KB).  Staging item = (key, 4-wide d chunk), D / 16 items of K and of V per thread.
// KV = __bf16 / _Float16 (FA_PAGED only): staging item = (key, 8-wide d chunk), D / 32 items per thread, each ONE 16-byte load of K and of
// V; the elements stay 16-bit in registers under the MFMAs and are widened (exactly) as they are written to LDS, so Ks / Vs hold what
// the float pool widened on the host would have put there.  A thread's items are whole keys: one table entry per item, as for KV = float.
template <int D, bool BIAS, FaForm FORM, typename KV = float>
__global__ void __launch_bounds__(FA_THREADS) flash_attention_f32_kernel(const FlashAttentionParams pa) {
    constexpr bool KV16 = !std::is_same<KV, float>::value;             // a narrow pool: 16-bit elements, or (KV8) e4m3 bytes on the same map
    constexpr bool KV8 = std::is_same<KV, fa_e4m3>::value;
    static_assert(!KV16 || (fa_paged(FORM) && !BIAS), "16-bit and fp8 K / V storage exist for the paged forms alone");
    constexpr int LD = D + 4, NI = D / 16, ND = D / 16, NC = D / 32;
    constexpr int NI16 = D / 32;                           // KV16: items per thread
    __shared__ __attribute__((aligned(16))) float Ks[FA_T * LD];
    __shared__ __attribute__((aligned(16))) float Vs[FA_T * LD];
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int li = lane & 15, g = lane >> 4;
    FaVarlenRecord rec;
    const FlashAttentionParams p = fa_params<FORM>(pa, rec);
    if constexpr (FORM == FA_PAGED_VARLEN) {
        if (rec.len_q == 0) return;                        // past the plan's real tiles (workgroup-uniform, before the first barrier)
    }
    const FaBlock blk = fa_block_of<BIAS, FORM>(p, rec);
    const FaLane ln = fa_lane<FORM>(p, blk, wave, li);
    FaFp8Scales fs{1.f, 1.f};
    if constexpr (KV8) fs = fa_fp8_scales(p, blk);
    if constexpr (fa_splits(FORM)) {
        // nothing to walk (workgroup-uniform, before the first barrier): the empty markers of the real rows
        if (blk.kt0 >= blk.nkt) {
            f32x4 z[D / 16];
#pragma unroll
            for (int dt = 0; dt < D / 16; ++dt) z[dt] = f32x4{0.f, 0.f, 0.f, 0.f};
            fa_finish_split<D, KV8, FORM == FA_PAGED_VARLEN>(p, blk, ln, g, z, 0.f, ATT_NEG, fs.v);
            return;
        }
    }
    // Q fragment: chunk c of 32 d's -> d = 32 c + 8 g .. + 7 of the query's row (the MFMA k order is a permutation of d; K uses the same)
    f32x4 qv[2 * NC];
    {
        const float* qp = ln.q + g * 8;
#pragma unroll
        for (int c = 0; c < NC; ++c) {
            qv[2 * c] = *reinterpret_cast<const f32x4*>(qp + c * 32);
            qv[2 * c + 1] = *reinterpret_cast<const f32x4*>(qp + c * 32 + 4);
        }
    }
    f32x4 kr[NI], vr[NI];
    vec8<KV> kr16[NI16], vr16[NI16];                       // KV16: the tile in flight, as stored
    f32x4 bn[FA_T / 16];                                   // BIAS: the bias of the tile in kr / vr, loaded with it
    // FA_PAGED: the table entries of the thread's NI keys of a tile: pn as fetch_pages loads them, a tile ahead; pe those load_tile uses
    // (KV16: the thread's NI16 keys)
    FaPages pgs{};
    int pe[NI], pn[NI];
    auto fetch_pages = [&](int key0) {
        if constexpr (KV16) {
#pragma unroll
            for (int i = 0; i < NI16; ++i) pn[i] = fa_page_entry(pgs, min(key0 + (tid + i * FA_THREADS) / (D / 8), p.seq_kv - 1));
        } else {
#pragma unroll
            for (int i = 0; i < NI; ++i) pn[i] = fa_page_entry(pgs, min(key0 + (tid + i * FA_THREADS) / (D / 4), p.seq_kv - 1));
        }
    };
    auto use_pages = [&]() {
#pragma unroll
        for (int i = 0; i < (KV16 ? NI16 : NI); ++i) pe[i] = pn[i];
    };
    auto load_tile = [&](int key0) {
        if constexpr (KV16) {
            const KV* kb = fa_kv_base<KV>(p.k, blk.k);
            const KV* vb = fa_kv_base<KV>(p.v, blk.v);
#pragma unroll
            for (int i = 0; i < NI16; ++i) {
                const int idx = tid + i * FA_THREADS, t = key0 + idx / (D / 8), c8 = (idx % (D / 8)) * 8;
                const long src = fa_page_row(pgs, pe[i], min(t, p.seq_kv - 1), p.kv_ss) + c8;
                kr16[i] = *reinterpret_cast<const vec8<KV>*>(kb + src);
                vr16[i] = *reinterpret_cast<const vec8<KV>*>(vb + src);
                if (t >= p.seq_kv) {
#pragma unroll
                    for (int e = 0; e < 8; ++e) { kr16[i][e] = (KV)0.f; vr16[i][e] = (KV)0.f; }
                }
            }
            return;
        }
#pragma unroll
        for (int i = 0; i < NI; ++i) {
            const int idx = tid + i * FA_THREADS, t = key0 + idx / (D / 4), c4 = (idx % (D / 4)) * 4;
            long src;
            if constexpr (fa_paged(FORM)) src = fa_page_row(pgs, pe[i], min(t, p.seq_kv - 1), p.kv_ss) + c4;
            else src = min(t, p.seq_kv - 1) * p.kv_ss + c4;
            kr[i] = *reinterpret_cast<const f32x4*>(blk.k + src);
            vr[i] = *reinterpret_cast<const f32x4*>(blk.v + src);
            if (t >= p.seq_kv) { kr[i] = f32x4{0.f, 0.f, 0.f, 0.f}; vr[i] = kr[i]; }
        }
        if constexpr (BIAS) fa_load_bias(bn, ln.bias, ln.brow, key0, g, p.seq_kv);
    };
    f32x4 o[ND];
#pragma unroll
    for (int dt = 0; dt < ND; ++dt) o[dt] = f32x4{0.f, 0.f, 0.f, 0.f};
    float m = ATT_NEG, l = 0.f;
    const float sc2 = (KV8 ? p.scale * fs.k : p.scale) * ATT_LOG2E;

    const int kt_first = (FORM == FA_VARLEN || fa_splits(FORM)) ? blk.kt0 : 0;
    if constexpr (fa_paged(FORM)) { pgs = fa_pages_of<FORM>(p); fetch_pages(kt_first * FA_T); use_pages(); }
    load_tile(kt_first * FA_T);
    if constexpr (fa_paged(FORM)) fetch_pages((kt_first + 1) * FA_T);      // (a key past the sequence is clamped into it: a valid entry, not used)
    for (int kt = kt_first; kt < blk.nkt; ++kt) {
        __syncthreads();                                   // every wave is done reading the previous tile
        if constexpr (KV16) {
#pragma unroll
            for (int i = 0; i < NI16; ++i) {
                const int idx = tid + i * FA_THREADS, t = idx / (D / 8), c8 = (idx % (D / 8)) * 8;
#pragma unroll
                for (int hh = 0; hh < 2; ++hh) {
                    f32x4 kw, vw;
                    if constexpr (KV8) {
                        f32x4 k2[2], v2[2];
                        fa_fp8_widen8(kr16[i], k2[0], k2[1]);
                        fa_fp8_widen8(vr16[i], v2[0], v2[1]);
                        kw = k2[hh]; vw = v2[hh];
                    } else {
#pragma unroll
                        for (int e = 0; e < 4; ++e) { kw[e] = fa_widen<KV>(kr16[i][hh * 4 + e]); vw[e] = fa_widen<KV>(vr16[i][hh * 4 + e]); }
                    }
                    *reinterpret_cast<f32x4*>(Ks + t * LD + c8 + hh * 4) = kw;
                    *reinterpret_cast<f32x4*>(Vs + t * LD + c8 + hh * 4) = vw;
                }
            }
        } else {
#pragma unroll
            for (int i = 0; i < NI; ++i) {
                const int idx = tid + i * FA_THREADS, t = idx / (D / 4), c4 = (idx % (D / 4)) * 4;
                *reinterpret_cast<f32x4*>(Ks + t * LD + c4) = kr[i];
                *reinterpret_cast<f32x4*>(Vs + t * LD + c4) = vr[i];
            }
        }
        __syncthreads();
        // S^T = K . Q^T (BIAS: + bias, as the initial accumulator: it joins the unscaled scores, and an all-zero bias gives the bias-free bits)
        f32x4 st[FA_T / 16];
        if constexpr (BIAS) {
#pragma unroll
            for (int s = 0; s < FA_T / 16; ++s) st[s] = bn[s];
        }
        if (kt + 1 < blk.nkt) {
            if constexpr (fa_paged(FORM)) { use_pages(); fetch_pages((kt + 2) * FA_T); }   // tile kt + 2's entries go out ahead of tile kt + 1's K / V
            load_tile((kt + 1) * FA_T);
        }
#pragma unroll
        for (int s = 0; s < FA_T / 16; ++s) {
            f32x4 acc = {0.f, 0.f, 0.f, 0.f};
            if constexpr (BIAS) acc = st[s];
#pragma unroll
            for (int c = 0; c < NC; ++c) acc = att_score_f32(Ks + (s * 16 + li) * LD + c * 32 + g * 8, qv[2 * c], qv[2 * c + 1], acc);
            st[s] = acc;
        }
        float alpha;
        if constexpr (FORM == FA_VARLEN) alpha = fa_softmax_tile<true>(st, sc2, fa_tile_masks_window(kt * FA_T, ln.wave_row0, ln.wave_lo), kt * FA_T, g, ln.limit, m, l, ln.lo);
        else if constexpr (fa_splits(FORM)) alpha = fa_softmax_tile<true>(st, sc2, fa_tile_masks(p, kt * FA_T, ln.wave_row0), kt * FA_T, g, ln.limit, m, l, 0);
        else alpha = fa_softmax_tile(st, sc2, fa_tile_masks(p, kt * FA_T, ln.wave_row0), kt * FA_T, g, ln.limit, m, l);
#pragma unroll
        for (int dt = 0; dt < ND; ++dt) o[dt] *= alpha;
        // O^T += V^T . P^T
#pragma unroll
        for (int s = 0; s < FA_T / 16; ++s) {
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const float* vp = Vs + (s * 16 + g * 4 + r) * LD + li;
#pragma unroll
                for (int dt = 0; dt < ND; ++dt) o[dt] = att_pv_f32(vp, dt, st[s][r], o[dt]);
            }
        }
    }
    if constexpr (fa_splits(FORM)) fa_finish_split<D, KV8, FORM == FA_PAGED_VARLEN>(p, blk, ln, g, o, l, m, fs.v);
    else fa_finish<ND, BIAS>(fa_lane_y<FORM>(p, blk, ln), g, o, l, m);
}

// ---- 16-bit: q, k, v rounded to E (round to nearest even) as they are loaded; v_mfma_f32_16x16x32_{bf16,f16} with fp32 accumulation.
// Scores, m, l (of the UNROUNDED numerators) and O are fp32; the numerators are rounded to E for P . V.
// LDS: Kp[key][D] and Vt[d][72 keys] (kernels/attention_mfma.h): D 128 = 16 + 18 KB.
// Staging item = (key pair, 4-wide d chunk): thread -> (d chunk low 2 bits, key pair, d chunk high bits), so a quad of lanes reads 64
// contiguous bytes of a row and the 4-byte transposed V writes of a wave fall 2-way on the 32 banks.
// KV = E (FA_PAGED only; brn_flash_attention_paged_kv_forward): the pool already holds E.  Staging item = (key pair, 8-wide d chunk), the
// same thread map with 8 d where the float map has 4: ONE 16-byte load per key of K and of V, a quad of lanes still reads 64 contiguous
// bytes of a row, the K side goes to LDS as one 16-byte store of a whole att_k_chunk and the V side as 8 att_vt_store of the thread's
// key pair, no conversion anywhere.  Passes: D / 64; with D = 32 the 128 items fill half a pass, and waves 2 and 3 stage nothing
// (a wave-uniform branch; the tile is 4 KB of K and of V, and a map of single keys would turn the V^T stores into twice as many 2-byte
// ones).  What reaches LDS is what the float pool's cast puts there, since (E)(float)e == e: the bits of KV = float on the widened pool. ----
template <typename E, int D, bool BIAS, FaForm FORM, typename KV = float>
__global__ void __launch_bounds__(FA_THREADS) flash_attention_s16_kernel(const FlashAttentionParams pa) {
    constexpr bool F16 = std::is_same<E, _Float16>::value;
    constexpr bool KV16 = !std::is_same<KV, float>::value;             // a narrow pool: elements of E, or (KV8) e4m3 bytes on the same map
    constexpr bool KV8 = std::is_same<KV, fa_e4m3>::value;
    static_assert(!KV16 || (fa_paged(FORM) && !BIAS && (KV8 || std::is_same<KV, E>::value)), "narrow K / V storage: the paged forms, in the kernel's own type or e4m3");
    constexpr int NP16 = D == 128 ? 2 : 1;        // KV16: staging passes
    constexpr int NP = D / 32, ND = D / 16;       // staging passes = MFMA k steps of a score tile; d tiles of O^T
    typedef vec8<E> ex8;
    typedef vec4<E> ex4;
    __shared__ __attribute__((aligned(16))) E Kp[FA_T * D];
    __shared__ __attribute__((aligned(16))) E Vt[D * FA_VT_LD];
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int li = lane & 15, g = lane >> 4;
    FaVarlenRecord rec;
    const FlashAttentionParams p = fa_params<FORM>(pa, rec);
    if constexpr (FORM == FA_PAGED_VARLEN) {
        if (rec.len_q == 0) return;                        // past the plan's real tiles (workgroup-uniform, before the first barrier)
    }
    const FaBlock blk = fa_block_of<BIAS, FORM>(p, rec);
    const FaLane ln = fa_lane<FORM>(p, blk, wave, li);
    FaFp8Scales fs{1.f, 1.f};
    if constexpr (KV8) fs = fa_fp8_scales(p, blk);
    if constexpr (fa_splits(FORM)) {
        // nothing to walk (workgroup-uniform, before the first barrier): the empty markers of the real rows
        if (blk.kt0 >= blk.nkt) {
            f32x4 z[D / 16];
#pragma unroll
            for (int dt = 0; dt < D / 16; ++dt) z[dt] = f32x4{0.f, 0.f, 0.f, 0.f};
            fa_finish_split<D, KV8, FORM == FA_PAGED_VARLEN>(p, blk, ln, g, z, 0.f, ATT_NEG, fs.v);
            return;
        }
    }
    // Q fragment of MFMA k step c: d = 32 c + 8 g .. + 7 of the query's row
    ex8 qf[NP];
    {
        const float* qp = ln.q + g * 8;
#pragma unroll
        for (int c = 0; c < NP; ++c) qf[c] = att_round8<E>(*reinterpret_cast<const f32x4*>(qp + c * 32), *reinterpret_cast<const f32x4*>(qp + c * 32 + 4));
    }
    // staging: keys (2 tp, 2 tp + 1) of the tile, d = c4 .. c4 + 3 with c4 = 16 (hi + 2 pass) + 4 lo
    const int s_lo = tid & 3, s_tp = (tid >> 2) & 31, s_hi = tid >> 7;
    f32x4 kr[NP][2], vr[NP][2];
    typedef vec8<typename std::conditional<KV8, fa_e4m3, E>::type> kv8_t;
    kv8_t kr16[NP16][2], vr16[NP16][2];                    // KV16: the tile in flight, as stored
    const bool stages = D >= 64 || s_hi == 0;              // KV16, D = 32: the waves that hold items (wave-uniform)
    f32x4 bn[FA_T / 16];                                   // BIAS: the bias of the tile in kr / vr, loaded with it
    // FA_PAGED: the table entry of the thread's key pair of a tile: pn as fetch_pages loads it, a tile ahead; pe the one load_tile uses.
    // A page holds an even number of keys from an even key on, so the pair (and what a key past the sequence is clamped to) shares a page
    // (KV16: the thread still owns ONE key pair (2 tp, 2 tp + 1), now with 8 d of it.  A page holds at least 16 keys and starts at a
    // multiple of 16, 2 tp is even, so 2 tp and 2 tp + 1 lie on one page; a key at or past len is clamped to len - 1, which is 2 tp itself
    // when only 2 tp + 1 is past the end and the one key the entry was fetched for when both are: one entry per thread and tile serves)
    FaPages pgs{};
    int pe = 0, pn = 0;
    auto fetch_pages = [&](int key0) { pn = fa_page_entry(pgs, min(key0 + s_tp * 2, p.seq_kv - 1)); };
    auto use_pages = [&]() { pe = pn; };
    auto load_tile = [&](int key0) {
        if constexpr (KV16) {
            if (stages) {
                const KV* kb = fa_kv_base<KV>(p.k, blk.k);
                const KV* vb = fa_kv_base<KV>(p.v, blk.v);
#pragma unroll
                for (int ps = 0; ps < NP16; ++ps) {
                    const int c8 = (s_hi + 2 * ps) * 32 + s_lo * 8;
#pragma unroll
                    for (int u = 0; u < 2; ++u) {
                        const int t = key0 + s_tp * 2 + u;
                        const long src = fa_page_row(pgs, pe, min(t, p.seq_kv - 1), p.kv_ss) + c8;
                        kr16[ps][u] = *reinterpret_cast<const kv8_t*>(kb + src);
                        vr16[ps][u] = *reinterpret_cast<const kv8_t*>(vb + src);
                        if (t >= p.seq_kv) {
#pragma unroll
                            for (int e = 0; e < 8; ++e) { kr16[ps][u][e] = (KV)0.f; vr16[ps][u][e] = (KV)0.f; }
                        }
                    }
                }
            }
            return;
        }
#pragma unroll
        for (int ps = 0; ps < NP; ++ps) {
            const int c4 = (s_hi + 2 * ps) * 16 + s_lo * 4;
#pragma unroll
            for (int u = 0; u < 2; ++u) {
                const int t = key0 + s_tp * 2 + u;
                long src;
                if constexpr (fa_paged(FORM)) src = fa_page_row(pgs, pe, min(t, p.seq_kv - 1), p.kv_ss) + c4;
                else src = min(t, p.seq_kv - 1) * p.kv_ss + c4;
                kr[ps][u] = *reinterpret_cast<const f32x4*>(blk.k + src);
                vr[ps][u] = *reinterpret_cast<const f32x4*>(blk.v + src);
                if (t >= p.seq_kv) { kr[ps][u] = f32x4{0.f, 0.f, 0.f, 0.f}; vr[ps][u] = kr[ps][u]; }
            }
        }
        if constexpr (BIAS) fa_load_bias(bn, ln.bias, ln.brow, key0, g, p.seq_kv);
    };
    f32x4 o[ND];
#pragma unroll
    for (int dt = 0; dt < ND; ++dt) o[dt] = f32x4{0.f, 0.f, 0.f, 0.f};
    float m = ATT_NEG, l = 0.f;
    const float sc2 = (KV8 ? p.scale * fs.k : p.scale) * ATT_LOG2E;

    const int kt_first = (FORM == FA_VARLEN || fa_splits(FORM)) ? blk.kt0 : 0;
    if constexpr (fa_paged(FORM)) { pgs = fa_pages_of<FORM>(p); fetch_pages(kt_first * FA_T); use_pages(); }
    load_tile(kt_first * FA_T);
    if constexpr (fa_paged(FORM)) fetch_pages((kt_first + 1) * FA_T);      // (a key past the sequence is clamped into it: a valid entry, not used)
    for (int kt = kt_first; kt < blk.nkt; ++kt) {
        __syncthreads();                                   // every wave is done reading the previous tile
        if constexpr (KV16) {
            if (stages) {
#pragma unroll
                for (int ps = 0; ps < NP16; ++ps) {
                    const int c8 = (s_hi + 2 * ps) * 32 + s_lo * 8;
                    if constexpr (KV8) {
                        ex8 ke[2], ve[2];                      // the key pair's bytes widened exactly to E
#pragma unroll
                        for (int u = 0; u < 2; ++u) {
                            f32x4 a, b;
                            fa_fp8_widen8(kr16[ps][u], a, b); ke[u] = att_round8<E>(a, b);
                            fa_fp8_widen8(vr16[ps][u], a, b); ve[u] = att_round8<E>(a, b);
                        }
#pragma unroll
                        for (int u = 0; u < 2; ++u) {
                            const int t = s_tp * 2 + u;
                            *reinterpret_cast<ex8*>(att_k_chunk<D>(Kp + t * D, t, c8 >> 3)) = ke[u];
                        }
#pragma unroll
                        for (int e = 0; e < 8; ++e) att_vt_store(Vt + (c8 + e) * FA_VT_LD, s_tp, ve[0][e], ve[1][e]);
                    } else {
#pragma unroll
                        for (int u = 0; u < 2; ++u) {
                            const int t = s_tp * 2 + u;
                            *reinterpret_cast<ex8*>(att_k_chunk<D>(Kp + t * D, t, c8 >> 3)) = kr16[ps][u];
                        }
#pragma unroll
                        for (int e = 0; e < 8; ++e) att_vt_store(Vt + (c8 + e) * FA_VT_LD, s_tp, vr16[ps][0][e], vr16[ps][1][e]);
                    }
                }
            }
        } else {
#pragma unroll
            for (int ps = 0; ps < NP; ++ps) {
                const int c4 = (s_hi + 2 * ps) * 16 + s_lo * 4;
#pragma unroll
                for (int u = 0; u < 2; ++u) {
                    const int t = s_tp * 2 + u;
                    ex4 h;
#pragma unroll
                    for (int e = 0; e < 4; ++e) h[e] = (E)kr[ps][u][e];
                    *reinterpret_cast<ex4*>(att_k_chunk<D>(Kp + t * D, t, c4 >> 3) + (c4 & 4)) = h;
                }
#pragma unroll
                for (int e = 0; e < 4; ++e) att_vt_store(Vt + (c4 + e) * FA_VT_LD, s_tp, (E)vr[ps][0][e], (E)vr[ps][1][e]);
            }
        }
        __syncthreads();
        // S^T = K . Q^T (BIAS: + bias, as the initial accumulator: it joins the unscaled scores, and an all-zero bias gives the bias-free bits)
        f32x4 st[FA_T / 16];
        if constexpr (BIAS) {
#pragma unroll
            for (int s = 0; s < FA_T / 16; ++s) st[s] = bn[s];
        }
        if (kt + 1 < blk.nkt) {
            if constexpr (fa_paged(FORM)) { use_pages(); fetch_pages((kt + 2) * FA_T); }   // tile kt + 2's entries go out ahead of tile kt + 1's K / V
            load_tile((kt + 1) * FA_T);
        }
#pragma unroll
        for (int s = 0; s < FA_T / 16; ++s) {
            const int key = s * 16 + li;
            f32x4 acc = {0.f, 0.f, 0.f, 0.f};
            if constexpr (BIAS) acc = st[s];
#pragma unroll
            for (int c = 0; c < NP; ++c) acc = att_mfma<F16>(att_k_frag<D>(Kp + key * D, key, c * 4 + g), qf[c], acc);
            st[s] = acc;
        }
        float alpha;
        if constexpr (FORM == FA_VARLEN) alpha = fa_softmax_tile<true>(st, sc2, fa_tile_masks_window(kt * FA_T, ln.wave_row0, ln.wave_lo), kt * FA_T, g, ln.limit, m, l, ln.lo);
        else if constexpr (fa_splits(FORM)) alpha = fa_softmax_tile<true>(st, sc2, fa_tile_masks(p, kt * FA_T, ln.wave_row0), kt * FA_T, g, ln.limit, m, l, 0);
        else alpha = fa_softmax_tile(st, sc2, fa_tile_masks(p, kt * FA_T, ln.wave_row0), kt * FA_T, g, ln.limit, m, l);
#pragma unroll
        for (int dt = 0; dt < ND; ++dt) o[dt] *= alpha;
        // O^T += V^T . P^T: k step t = key sub-tiles (2t, 2t+1)
#pragma unroll
        for (int t = 0; t < FA_T / 32; ++t) {
            const ex8 pf = att_round8<E>(st[2 * t], st[2 * t + 1]);
#pragma unroll
            for (int dt = 0; dt < ND; ++dt) o[dt] = att_mfma<F16>(att_vt_frag(Vt + (dt * 16 + li) * FA_VT_LD + g * 4, t), pf, o[dt]);
        }
    }
    if constexpr (fa_splits(FORM)) fa_finish_split<D, KV8, FORM == FA_PAGED_VARLEN>(p, blk, ln, g, o, l, m, fs.v);
    else fa_finish<ND, BIAS>(fa_lane_y<FORM>(p, blk, ln), g, o, l, m);
}

// ---- FA_SPLIT, S > 1: the S partials of a row become the row.  One thread = (row r, 4 consecutive d): M = max_s lse2_part[s][r],
// w_s = exp2(lse2_part[s][r] - M), y = (sum_s w_s O_part[s][r]) / sum_s w_s with both sums in the order s = 0 .. S - 1,
// lse = ln 2 * (M + log2 sum_s w_s) from the thread of d = 0.  Split 0 holds key 0, which every row sees, so M is finite; an empty partial
// (-inf) has w = exp2(-inf) = 0 exactly and its O_part is 0.  y has q's strides; every offset into the workspace is 64-bit.
// A decode call has few rows and many splits, so the kernel is a chain of S load latencies unless the loads are issued together: the
// partials are fetched FA_COMBINE_CHUNK splits at a time (the index clamped to S - 1, the value of a clamped slot not used), and only
// the arithmetic runs one split after the other.
// PAGED = true (brn_flash_attention_paged_forward): a row may have no visible key in ANY split (its sequence is empty, or causal with
// query + len - seq_q < 0), so M may be -inf.  The weights are then taken against 0 instead of M (exp2(-inf - 0) = 0: -inf - -inf is never
// formed), and y = 0, lse = -inf are SELECTED for the row.  A row with a visible key has a finite M and goes through the operations of
// PAGED = false, which is the kernel of the split entry as it was. ----
constexpr int FA_COMBINE_THREADS = 256;
constexpr int FA_COMBINE_CHUNK = 8;
// VS (with PAGED; the fp8 pool): the row of y, after the select, is multiplied by v_scale of the row's K / V head; lse is not.
// PV (with PAGED; brn_flash_attention_paged_varlen_forward: batch 1, seq_q = total_q, row r = head * total_q + token): a token outside the
// plan's [s_0, s_n) is padding, no kernel wrote its partials, and its thread returns before it reads or writes anything of the row.
template <bool PAGED, bool VS = false, bool PV = false>
__global__ void __launch_bounds__(FA_COMBINE_THREADS) flash_split_combine_kernel(const FlashAttentionParams p) {
    const int D4 = p.head_dim / 4;
    const long R = (long)p.batch * p.heads * p.seq_q;
    const long idx = (long)blockIdx.x * FA_COMBINE_THREADS + threadIdx.x;
    if (idx >= R * D4) return;
    const long r = idx / D4;
    if constexpr (PV) {
        const int* starts = p.pv_plan + fa_pv_starts_at();
        const int token = (int)(r % p.seq_q);
        if (token < starts[0] || token >= starts[p.pv_n_seqs]) return;
    }
    const int d = (int)(idx - r * D4) * 4;
    const int S = p.kv_splits;
    float M = -__builtin_inff();
    for (int s0 = 0; s0 < S; s0 += FA_COMBINE_CHUNK) {
        float l2[FA_COMBINE_CHUNK];
#pragma unroll
        for (int j = 0; j < FA_COMBINE_CHUNK; ++j) l2[j] = p.lse2_part[(long)min(s0 + j, S - 1) * R + r];
#pragma unroll
        for (int j = 0; j < FA_COMBINE_CHUNK; ++j) M = fmaxf(M, l2[j]);          // (a clamped slot repeats split S - 1)
    }
    const bool none = PAGED && !(M > -__builtin_inff());
    if constexpr (PAGED) M = none ? 0.f : M;
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    float wsum = 0.f;
    for (int s0 = 0; s0 < S; s0 += FA_COMBINE_CHUNK) {
        float l2[FA_COMBINE_CHUNK];
        f32x4 ov[FA_COMBINE_CHUNK];
#pragma unroll
        for (int j = 0; j < FA_COMBINE_CHUNK; ++j) {
            const long sr = (long)min(s0 + j, S - 1) * R + r;
            l2[j] = p.lse2_part[sr];
            ov[j] = *reinterpret_cast<const f32x4*>(p.o_part + sr * p.head_dim + d);
        }
#pragma unroll
        for (int j = 0; j < FA_COMBINE_CHUNK; ++j) {
            if (s0 + j < S) {                                                      // wave-uniform
                const float w = __builtin_amdgcn_exp2f(l2[j] - M);
                acc += ov[j] * w;
                wsum += w;
            }
        }
    }
    const long bh = r / p.seq_q;
    const int query = (int)(r - bh * p.seq_q), b = (int)(bh / p.heads), head = (int)(bh - (long)b * p.heads);
    f32x4 yv = acc / wsum;
    float lv = (M + __builtin_amdgcn_logf(wsum)) * 0.6931471805599453f;
    if constexpr (PAGED) {
        if (none) { yv = f32x4{0.f, 0.f, 0.f, 0.f}; lv = -__builtin_inff(); }
    }
    if constexpr (VS) yv = yv * (p.v_scale ? p.v_scale[head / (p.heads / p.kv_heads)] : 1.f);
    *reinterpret_cast<f32x4*>(p.y + (b * p.q_sb + head * p.q_sh + query * p.q_ss + d)) = yv;
    if (d == 0 && p.lse) p.lse[r] = lv;
}

template <int D, bool BIAS, FaForm FORM>
void fa_launch(const FlashAttentionParams& p, dim3 grid, hipStream_t s) {
    const dim3 block(FA_THREADS);
    if (p.s16 == 0) hipLaunchKernelGGL((flash_attention_f32_kernel<D, BIAS, FORM>), grid, block, 0, s, p);
    else if (p.s16 == 1) hipLaunchKernelGGL((flash_attention_s16_kernel<__bf16, D, BIAS, FORM>), grid, block, 0, s, p);
    else hipLaunchKernelGGL((flash_attention_s16_kernel<_Float16, D, BIAS, FORM>), grid, block, 0, s, p);
}
// FA_PAGED over a 16-bit pool (p.kv_type 1 bf16 / 2 fp16; launch_flash_attention has refused every pairing but these): the fp32 kernel
// widening either type, or the 16-bit kernel of the pool's own type
template <int D>
void fa_launch_kv16(const FlashAttentionParams& p, dim3 grid, hipStream_t s) {
    const dim3 block(FA_THREADS);
    if (p.s16 == 0 && p.kv_type == 1) hipLaunchKernelGGL((flash_attention_f32_kernel<D, false, FA_PAGED, __bf16>), grid, block, 0, s, p);
    else if (p.s16 == 0) hipLaunchKernelGGL((flash_attention_f32_kernel<D, false, FA_PAGED, _Float16>), grid, block, 0, s, p);
    else if (p.s16 == 1) hipLaunchKernelGGL((flash_attention_s16_kernel<__bf16, D, false, FA_PAGED, __bf16>), grid, block, 0, s, p);
    else hipLaunchKernelGGL((flash_attention_s16_kernel<_Float16, D, false, FA_PAGED, _Float16>), grid, block, 0, s, p);
}
// FA_PAGED over an e4m3 pool (p.kv_type FA_KV_FP8): any compute mode reads it
template <int D>
void fa_launch_kv8(const FlashAttentionParams& p, dim3 grid, hipStream_t s) {
    const dim3 block(FA_THREADS);
    if (p.s16 == 0) hipLaunchKernelGGL((flash_attention_f32_kernel<D, false, FA_PAGED, fa_e4m3>), grid, block, 0, s, p);
    else if (p.s16 == 1) hipLaunchKernelGGL((flash_attention_s16_kernel<__bf16, D, false, FA_PAGED, fa_e4m3>), grid, block, 0, s, p);
    else hipLaunchKernelGGL((flash_attention_s16_kernel<_Float16, D, false, FA_PAGED, fa_e4m3>), grid, block, 0, s, p);
}
// FA_PAGED_VARLEN: the pool types and pairings of FA_PAGED (launch_flash_attention has refused every other)
template <int D>
void fa_launch_paged_varlen(const FlashAttentionParams& p, dim3 grid, hipStream_t s) {
    const dim3 block(FA_THREADS);
    constexpr FaForm F = FA_PAGED_VARLEN;
    if (p.kv_type == 0) fa_launch<D, false, F>(p, grid, s);
    else if (p.kv_type == FA_KV_FP8) {
        if (p.s16 == 0) hipLaunchKernelGGL((flash_attention_f32_kernel<D, false, F, fa_e4m3>), grid, block, 0, s, p);
        else if (p.s16 == 1) hipLaunchKernelGGL((flash_attention_s16_kernel<__bf16, D, false, F, fa_e4m3>), grid, block, 0, s, p);
        else hipLaunchKernelGGL((flash_attention_s16_kernel<_Float16, D, false, F, fa_e4m3>), grid, block, 0, s, p);
    } else if (p.s16 == 0 && p.kv_type == 1) hipLaunchKernelGGL((flash_attention_f32_kernel<D, false, F, __bf16>), grid, block, 0, s, p);
    else if (p.s16 == 0) hipLaunchKernelGGL((flash_attention_f32_kernel<D, false, F, _Float16>), grid, block, 0, s, p);
    else if (p.s16 == 1) hipLaunchKernelGGL((flash_attention_s16_kernel<__bf16, D, false, F, __bf16>), grid, block, 0, s, p);
    else hipLaunchKernelGGL((flash_attention_s16_kernel<_Float16, D, false, F, _Float16>), grid, block, 0, s, p);
}
template <int D>
void fa_launch(const FlashAttentionParams& p, FaForm form, dim3 grid, hipStream_t s) {
    if (form == FA_VARLEN) fa_launch<D, false, FA_VARLEN>(p, grid, s);
    else if (form == FA_PAGED_VARLEN) fa_launch_paged_varlen<D>(p, grid, s);
    else if (form == FA_PAGED && p.kv_type == FA_KV_FP8) fa_launch_kv8<D>(p, grid, s);
    else if (form == FA_PAGED && p.kv_type) fa_launch_kv16<D>(p, grid, s);
    else if (form == FA_PAGED) fa_launch<D, false, FA_PAGED>(p, grid, s);
    else if (form == FA_SPLIT) fa_launch<D, false, FA_SPLIT>(p, grid, s);
    else if (form == FA_PACKED) {
        if (p.bias) fa_launch<D, true, FA_PACKED>(p, grid, s);
        else fa_launch<D, false, FA_PACKED>(p, grid, s);
    } else {
        if (p.bias) fa_launch<D, true, FA_PLAIN>(p, grid, s);
        else fa_launch<D, false, FA_PLAIN>(p, grid, s);
    }
}

}  // namespace

hipError_t launch_flash_attention(const FlashAttentionParams& p, hipStream_t s) {
    // a 16-bit pool exists for the paged form alone, and a 16-bit kernel reads only a pool of its own type
    // (an e4m3 pool, FA_KV_FP8, is read by every kernel; the scale arrays exist with it alone)
    if (p.kv_type && (p.kv_type < 0 || p.kv_type > FA_KV_FP8 || !p.block_table || p.plan || (p.kv_type != FA_KV_FP8 && p.s16 && p.s16 != p.kv_type))) return hipErrorInvalidValue;
    if (p.kv_type != FA_KV_FP8 && (p.k_scale || p.v_scale)) return hipErrorInvalidValue;
    if (p.pv_plan) {
        // the packed paged batch: batch 1 and seq_q = pv_total_q lay out q, y, lse and the partials; the split is FA_PAGED's at
        // seq_kv = max_kv_len; the grid holds T_max row tiles (brn_flash_paged_varlen_plan.h), the plan kernel runs first on the stream
        const int G = p.kv_heads >= 1 && p.heads >= 1 && p.heads % p.kv_heads == 0 ? p.heads / p.kv_heads : 0;
        if (!(p.head_dim == 32 || p.head_dim == 64 || p.head_dim == 128) || G < 1 || p.batch != 1 || p.plan || p.bias || p.n_bias || p.causal_off || p.s16 < 0 || p.s16 > 2 ||
            !(p.scale > 0.f) || !p.pv_cu || p.pv_n_seqs < 1 || p.pv_n_seqs > FA_PV_MAX_SEQS || p.pv_total_q < 1 || p.seq_q != p.pv_total_q || (long)G * p.pv_total_q > 0x7fffffffL ||
            p.seq_kv < 1 || p.seq_kv > 65536 || !p.block_table || !p.kv_lens || p.page_log2 < 4 || p.page_log2 > 8 || p.n_pages < 1 || p.max_pages < 1 ||
            ((long)p.n_pages << p.page_log2) > 0x7fffffffL || ((long)p.max_pages << p.page_log2) < p.seq_kv || p.kv_sb != 0 || p.kv_sh != p.head_dim ||
            p.kv_ss != (long)p.kv_heads * p.head_dim || p.page_stride != (p.kv_ss << p.page_log2) || p.q_sh != p.head_dim || p.q_ss != (long)p.heads * p.head_dim)
            return hipErrorInvalidValue;
        const int nkt = (p.seq_kv + FA_T - 1) / FA_T, S = p.kv_splits, tps = p.tiles_per_split;
        const long nwg = fa_pv_max_tiles(G, p.pv_total_q, p.pv_n_seqs) * p.kv_heads * S;
        const long quads = (long)p.heads * p.pv_total_q * (p.head_dim / 4);
        if (S < 1 || tps < 1 || (long)(S - 1) * tps >= nkt || (long)S * tps < nkt || nwg < 1 || nwg > 0x7fffffffL || (S > 1) != (p.o_part != nullptr) ||
            (S > 1) != (p.lse2_part != nullptr) || (quads + FA_COMBINE_THREADS - 1) / FA_COMBINE_THREADS > 0x7fffffffL)
            return hipErrorInvalidValue;
        const hipError_t e = launch_paged_varlen_plan(p.pv_cu, p.pv_n_seqs, p.pv_total_q, G, p.pv_plan, s);
        if (e != hipSuccess) return e;
        const dim3 grid((unsigned)nwg);
        if (p.head_dim == 32) fa_launch<32>(p, FA_PAGED_VARLEN, grid, s);
        else if (p.head_dim == 64) fa_launch<64>(p, FA_PAGED_VARLEN, grid, s);
        else fa_launch<128>(p, FA_PAGED_VARLEN, grid, s);
        const dim3 cgrid((unsigned)((quads + FA_COMBINE_THREADS - 1) / FA_COMBINE_THREADS));
        if (S > 1 && p.kv_type == FA_KV_FP8) hipLaunchKernelGGL((flash_split_combine_kernel<true, true, true>), cgrid, dim3(FA_COMBINE_THREADS), 0, s, p);
        else if (S > 1) hipLaunchKernelGGL((flash_split_combine_kernel<true, false, true>), cgrid, dim3(FA_COMBINE_THREADS), 0, s, p);
        return hipGetLastError();
    }
    if (p.plan) {
        // the packed batch: the record table was built and every value in it checked by the entry (brn_flash_varlen_plan.h); what is
        // checked here is what the kernels assume of the other arguments
        if (!(p.head_dim == 32 || p.head_dim == 64 || p.head_dim == 128) || p.heads < 1 || p.kv_heads < 1 || p.kv_heads > p.heads ||
            p.heads % p.kv_heads || p.batch != 1 || p.causal || p.causal_off || p.bias || p.n_bias || p.s16 < 0 || p.s16 > 2 || !(p.scale > 0.f) ||
            p.n_records < 1 || p.window_left < -1 || p.window_right < -1 || p.window_left > FA_VARLEN_MAX_LEN || p.window_right > FA_VARLEN_MAX_LEN || (long)p.n_records * p.kv_heads > 0x7fffffffL)
            return hipErrorInvalidValue;
        const dim3 grid((unsigned)(p.n_records * p.kv_heads));
        if (p.head_dim == 32) fa_launch<32>(p, FA_VARLEN, grid, s);
        else if (p.head_dim == 64) fa_launch<64>(p, FA_VARLEN, grid, s);
        else fa_launch<128>(p, FA_VARLEN, grid, s);
        return hipGetLastError();
    }
    if (!(p.head_dim == 32 || p.head_dim == 64 || p.head_dim == 128) || p.seq_q < 1 || p.seq_kv < 1 || p.seq_q > 65536 || p.seq_kv > 65536 ||
        p.batch < 1 || p.heads < 1 || p.kv_heads < 1 || p.kv_heads > p.heads || p.heads % p.kv_heads ||
        p.causal_off != (p.causal && !p.block_table ? p.seq_kv - p.seq_q : 0) || p.causal_off < 0 || (p.block_table && !p.kv_splits) || p.s16 < 0 || p.s16 > 2 || !(p.scale > 0.f) ||
        p.n_bias < 0 || (p.bias == nullptr) != (p.n_bias == 0) || (p.n_bias > 0 && p.batch % p.n_bias))
        return hipErrorInvalidValue;
    if (p.kv_splits) {
        // the split over keys: S = kv_splits and tps = tiles_per_split as brn_flash_split_plan.h normalises them (no empty trailing split),
        // the partials in the workspace exactly when S > 1; no bias.  With a block table (the paged entry) seq_kv is max_kv_len, k and v are
        // the pool with a page's strides, and the per-sequence causal_off is the kernels' own (0 here)
        const bool paged = p.block_table != nullptr;
        if (paged && (!p.kv_lens || p.page_log2 < 4 || p.page_log2 > 8 || p.n_pages < 1 || p.max_pages < 1 || ((long)p.n_pages << p.page_log2) > 0x7fffffffL ||
                      ((long)p.max_pages << p.page_log2) < p.seq_kv || p.kv_sb != 0 || p.kv_sh != p.head_dim || p.kv_ss != (long)p.kv_heads * p.head_dim ||
                      p.page_stride != (p.kv_ss << p.page_log2)))
            return hipErrorInvalidValue;
        if (!paged && (p.kv_lens || p.page_stride || p.page_log2 || p.n_pages || p.max_pages)) return hipErrorInvalidValue;
        const int nkt = (p.seq_kv + FA_T - 1) / FA_T, S = p.kv_splits, tps = p.tiles_per_split;
        const long rows = (long)(p.heads / p.kv_heads) * p.seq_q;
        const long nwg = (long)p.batch * p.kv_heads * ((rows + FA_BQ - 1) / FA_BQ) * S;
        const long quads = (long)p.batch * p.heads * p.seq_q * (p.head_dim / 4);
        if (p.bias || S < 1 || tps < 1 || (long)(S - 1) * tps >= nkt || (long)S * tps < nkt || rows > 0x7fffffffL || nwg > 0x7fffffffL ||
            (S > 1) != (p.o_part != nullptr) || (S > 1) != (p.lse2_part != nullptr) || (quads + FA_COMBINE_THREADS - 1) / FA_COMBINE_THREADS > 0x7fffffffL)
            return hipErrorInvalidValue;
        const dim3 grid((unsigned)nwg);
        const FaForm form = paged ? FA_PAGED : FA_SPLIT;
        if (p.head_dim == 32) fa_launch<32>(p, form, grid, s);
        else if (p.head_dim == 64) fa_launch<64>(p, form, grid, s);
        else fa_launch<128>(p, form, grid, s);
        const dim3 cgrid((unsigned)((quads + FA_COMBINE_THREADS - 1) / FA_COMBINE_THREADS));
        if (S > 1 && p.kv_type == FA_KV_FP8) hipLaunchKernelGGL((flash_split_combine_kernel<true, true>), cgrid, dim3(FA_COMBINE_THREADS), 0, s, p);
        else if (S > 1 && paged) hipLaunchKernelGGL(flash_split_combine_kernel<true>, cgrid, dim3(FA_COMBINE_THREADS), 0, s, p);
        else if (S > 1) hipLaunchKernelGGL(flash_split_combine_kernel<false>, cgrid, dim3(FA_COMBINE_THREADS), 0, s, p);
        return hipGetLastError();
    }
    // one K / V head per query head and the diagonal at key = query: the kernels of the two older entries, a workgroup per (batch entry,
    // head, 64 queries).  Otherwise the packed-row kernels, a workgroup per (batch entry, K / V head, 64 packed rows)
    // A/B switch (make EXTRA_CXXFLAGS=-DFA_FORCE_PACKED=1): the packed-row kernels also where G == 1 and the diagonal is at key = query — the
    // same rows, grid order and addresses as the plain kernels, so the two builds differ by the kernels' code alone.  DESIGN.md 3.2f
    const FaForm gqa = (FA_FORCE_PACKED || p.kv_heads != p.heads || p.causal_off != 0) ? FA_PACKED : FA_PLAIN;
    const long rows = (long)(p.heads / p.kv_heads) * p.seq_q;
    if (rows > 0x7fffffffL) return hipErrorInvalidValue;
    const long nwg = (long)p.batch * p.kv_heads * ((rows + FA_BQ - 1) / FA_BQ);
    if (nwg > 0x7fffffffL) return hipErrorInvalidValue;
    const dim3 grid((unsigned)nwg);
    if (p.head_dim == 32) fa_launch<32>(p, gqa, grid, s);
    else if (p.head_dim == 64) fa_launch<64>(p, gqa, grid, s);
    else fa_launch<128>(p, gqa, grid, s);
    return hipGetLastError();
}

}  // namespace brn
