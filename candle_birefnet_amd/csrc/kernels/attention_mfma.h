// attention_mfma.h — the 16x16 MFMA attention formulation that kernels/window_attention.hip, kernels/attention_bias.hip and
// kernels/flash_attention.hip share, stated once.  Everything here is a device helper at the granularity of one 16-key tile or one
// MFMA k-step; geometry (sequence lengths, tile walks, biases, masks, launch shapes) belongs to the three files.  A kernel calls a
// helper only where its assembly stays what the spelled-out form gave (tools/isa_compare.py); the few places that spell a piece out
// say so in a comment, and a change to a helper here has to be made there too.
//
// All tiles are 16x16; lane = 16 g + li (li = lane & 15, lane group g = lane >> 4); C/D map: col = lane & 15, row = 4 (lane >> 4) + reg.
//   S^T[key][query] = K . Q^T   A = K (row = key li of the tile), B = Q^T (col = query li).  fp32: k-step 4, lane group g contracts
//                               d = 8g + s at step s (both operands use the same permutation, so a lane's 8 q or k values are 8
//                               consecutive floats of one row); 16-bit: k = 32, lane group g holds d = 8g .. 8g + 7 of a 32-wide chunk of
//                               the row.  A lane's 4 accumulator registers are keys 16 kt + 4g + 0..3 of ITS query (column li).
//   softmax over keys           = over the rows of S^T for a fixed column: in-lane over the tile registers, then across the 4 lane
//                               groups (shfl_xor 16, 32).
//   O^T[d][query] = V^T . P^T   B = P^T straight from the S^T accumulator registers, A = V^T with the same key permutation.  fp32:
//                               step r contracts key 4g + r.  16-bit: one MFMA contracts key tiles (2t, 2t+1): lane group g's k slots
//                               are keys 16 (2t) + 4g + 0..3 and 16 (2t+1) + 4g + 0..3 — exactly the keys whose P^T values the lane
//                               already holds — so P never leaves registers: no transpose, no LDS round trip.
//                               The lane ends with O^T[d = 16 dt + 4g + r][query li]: 4 consecutive outputs of its query's row.
// LDS images, fp32: Ks, Vs [key][D + 4] floats.  16-bit (E = __bf16 or _Float16):
//   Kp[key][D]     rows of D elements; the 16-byte chunk c (d = 8c .. 8c + 7) of row `key` is stored at c ^ att_kswz<D>(key):
//                  conflict-free ds_read_b128 of the A operand (row = key, chunk = 4 (k-step) + g)
//   Vt[d][keys]    V transposed, rows of an LD the file chooses: the A operand of O^T = V^T P^T is 8 keys of one d; written as key
//                  pairs (2tp, 2tp + 1), read as two 8-byte halves (tiles 2t and 2t + 1)
#pragma once
#include "split_planes.h"

namespace brn {

constexpr float ATT_LOG2E = 1.4426950408889634f;
constexpr float ATT_NEG = -3.0e38f;      // an excluded score: below every real one, and exp2(ATT_NEG - m) is exactly 0

template <typename E> using vec8 = E __attribute__((ext_vector_type(8)));
template <typename E> using vec4 = E __attribute__((ext_vector_type(4)));
template <typename E> using vec2 = E __attribute__((ext_vector_type(2)));

template <bool F16, typename V>
__device__ __forceinline__ f32x4 att_mfma(const V a, const V b, const f32x4 c) {
    if constexpr (F16) return __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(f16x8, a), __builtin_bit_cast(f16x8, b), c, 0, 0, 0);
    else return __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, a), __builtin_bit_cast(bf16x8, b), c, 0, 0, 0);
}

// ---- Kp: krow = Kp + key * D, the key's row ----
template <int D>
__device__ __forceinline__ int att_kswz(int key) {
    static_assert(D == 32 || D == 64 || D == 128, "rows of 4, 8 or 16 chunks");
    if constexpr (D == 32) return (0x78 >> (2 * ((key >> 2) & 3))) & 3;      // 4 chunks per row, 4 rows per bank cycle: perm[(key >> 2) & 3], perm = {0,2,3,1}
    else if constexpr (D == 64) return (key >> 1) & 7;                        // 8 chunks per row, 2 rows per bank cycle
    else return key & 15;                                                     // 16 chunks per row = one bank cycle
}
// where the 16-byte chunk c of the row is stored (a 4-wide store of d .. d + 3 goes to chunk d >> 3, + (d & 4))
template <int D, typename E>
__device__ __forceinline__ E* att_k_chunk(E* krow, int key, int c) { return krow + ((c ^ att_kswz<D>(key)) << 3); }
// A operand of S^T = K Q^T: chunk c of the row (16-bit k-step s of lane group g reads chunk 4 s + g)
template <int D, typename E>
__device__ __forceinline__ vec8<E> att_k_frag(const E* krow, int key, int c) { return *reinterpret_cast<const vec8<E>*>(att_k_chunk<D>(krow, key, c)); }

// ---- Vt: vrow = Vt + d * LD ----
// keys (2tp, 2tp + 1) of row d
template <typename E>
__device__ __forceinline__ void att_vt_store(E* vrow, int tp, E a, E b) {
    vec2<E> h;
    h[0] = a; h[1] = b;
    *reinterpret_cast<vec2<E>*>(vrow + tp * 2) = h;
}
// A operand of O^T = V^T P^T at k-step t (key tiles 2t, 2t + 1); vg = vrow + 4g; hi_tile = whether tile 2t + 1 exists in the image
// (the 10th of 9 does not: zeros)
template <typename E>
__device__ __forceinline__ vec8<E> att_vt_frag(const E* vg, int t, bool hi_tile = true) {
    const vec4<E> lo = *reinterpret_cast<const vec4<E>*>(vg + (2 * t) * 16);
    vec4<E> hi = {(E)0.f, (E)0.f, (E)0.f, (E)0.f};
    if (hi_tile) hi = *reinterpret_cast<const vec4<E>*>(vg + (hi_tile ? 2 * t + 1 : 0) * 16);
    vec8<E> vf;
#pragma unroll
    for (int e = 0; e < 4; ++e) { vf[e] = lo[e]; vf[4 + e] = hi[e]; }
    return vf;
}
// B operand of the same k-step before rounding: the lane's 8 softmax numerators, straight out of the S^T accumulators of an NT-tile row
template <int NT>
__device__ __forceinline__ void att_p_step(const f32x4 (&st)[NT], int t, float (&r)[8]) {
#pragma unroll
    for (int e = 0; e < 4; ++e) { r[e] = st[2 * t][e]; r[4 + e] = (2 * t + 1 < NT) ? st[(2 * t + 1 < NT) ? 2 * t + 1 : 0][e] : 0.f; }
}
// two accumulator tiles (or the two halves of a query's 8 d's) rounded to E, round to nearest even: a P fragment, a Q fragment
template <typename E>
__device__ __forceinline__ vec8<E> att_round8(const f32x4 a, const f32x4 b) {
    vec8<E> f;
#pragma unroll
    for (int e = 0; e < 4; ++e) { f[e] = (E)a[e]; f[4 + e] = (E)b[e]; }
    return f;
}

// ---- fp32: v_mfma_f32_16x16x4_f32, an exact fmaf chain per score and per output ----
// acc + the 8 products of one 32-wide chunk of a key row: kp = the key's row + 8g, (qa, qb) = the same 8 d's of the query
__device__ __forceinline__ f32x4 att_score_f32(const float* kp, const f32x4 qa, const f32x4 qb, f32x4 acc) {
    const f32x4 k0 = *reinterpret_cast<const f32x4*>(kp);
    const f32x4 k1 = *reinterpret_cast<const f32x4*>(kp + 4);
#pragma unroll
    for (int e = 0; e < 4; ++e) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(k0[e], qa[e], acc, 0, 0, 0);
#pragma unroll
    for (int e = 0; e < 4; ++e) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(k1[e], qb[e], acc, 0, 0, 0);
    return acc;
}
// one key of P . V into d tile dt: vp = Vs + key * LD + li, pr = the lane's numerator of that key
__device__ __forceinline__ f32x4 att_pv_f32(const float* vp, int dt, float pr, const f32x4 o) { return __builtin_amdgcn_mfma_f32_16x16x4f32(vp[dt * 16], pr, o, 0, 0, 0); }

// ---- softmax, per tile of 4 registers; the 4 lane groups of a query combine at the end ----
__device__ __forceinline__ float att_group_max(float mx) {
    mx = fmaxf(mx, __shfl_xor(mx, 16));
    return fmaxf(mx, __shfl_xor(mx, 32));
}
__device__ __forceinline__ float att_group_sum(float sum) {
    sum += __shfl_xor(sum, 16);
    return sum + __shfl_xor(sum, 32);
}
// scores -> exp2 units (sc2 = scale * ATT_LOG2E)
__device__ __forceinline__ void att_scale4(f32x4& s, float sc2) {
#pragma unroll
    for (int r = 0; r < 4; ++r) s[r] *= sc2;
}
// register r is key k0 + r: keys from `limit` on leave the softmax
__device__ __forceinline__ void att_exclude4(f32x4& s, int k0, int limit) {
#pragma unroll
    for (int r = 0; r < 4; ++r) s[r] = (k0 + r < limit) ? s[r] : ATT_NEG;
}
// the two-sided sibling (a window): keys before `lo` and keys from `hi` on leave the softmax.  They become -inf, not ATT_NEG: a row may
// meet wholly excluded tiles BEFORE its first real score, while m is still ATT_NEG, and exp2(-inf - ATT_NEG) is exactly 0 where
// exp2(ATT_NEG - ATT_NEG) would be 1 (what a -inf bias entry does; -inf never raises the maximum either)
__device__ __forceinline__ void att_exclude4_window(f32x4& s, int k0, int lo, int hi) {
#pragma unroll
    for (int r = 0; r < 4; ++r) s[r] = (k0 + r >= lo && k0 + r < hi) ? s[r] : -__builtin_inff();
}
__device__ __forceinline__ float att_max4(float mx, const f32x4 s) { return fmaxf(fmaxf(mx, fmaxf(s[0], s[1])), fmaxf(s[2], s[3])); }
// numerators exp2(s - m) in place, added to sum in register order
__device__ __forceinline__ void att_exp2_sum4(f32x4& s, float m, float& sum) {
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const float e = __builtin_amdgcn_exp2f(s[r] - m);
        s[r] = e;
        sum += e;
    }
}

// lane holds O^T[d = 16 dt + 4g + r][query]: one 16-byte store per d tile; yg = the query's row of y + 4g
__device__ __forceinline__ void att_store_o(float* yg, int dt, const f32x4 o, float inv) { *reinterpret_cast<f32x4*>(yg + dt * 16) = o * inv; }

}  // namespace brn
