// window_attention.hip — fused (shifted-)window attention for the Swin-L geometry (window 12x12 = 144 tokens,
// head_dim 32), exact fp32 on v_mfma_f32_16x16x4_f32.
//
// One workgroup = one (window, head).  It replaces, for that window/head, everything the reference does between
// the qkv Linear and the proj Linear (swin.rs:359-401 + 266-307):
//   pad_with_zeros (swin.rs:359-366)      -> a pad token's q/k/v is the qkv bias vector (LN output row == 0)
//   roll_2d(-shift) (swin.rs:371-377)     -> source position = (window position + shift) mod (Hp, Wp)
//   window_partition (swin.rs:446-459)    -> index math on load
//   q*scale, q@k^T, +bias, +mask, softmax_last_dim, @v (swin.rs:278-303)
//   transpose/reshape, window_reverse, roll_2d(+shift), narrow (swin.rs:306-307, 387-401) -> index math on store
// so none of the reference's ~8 full-tensor copies per block and no [B_,h,144,144] score tensor ever touch HBM.
//
// MFMA formulation, tile map and LDS images: kernels/attention_mfma.h (S^T = K . Q^T, softmax in-lane over 36 registers and across
// the 4 lane groups, O^T = V^T . P^T with P^T straight from the S^T accumulators).  What is particular here:
//   bias                        = this head's 529-entry table column in LDS, indexed arithmetically (no [h,144,144] tensor)
//   mask                        = the SW-MSA region ids of the window's tokens, compared per score
#include "../brn_kernels.h"
#include "attention_mfma.h"
#include "window_geometry.h"
#include "window_attention_select.h"
#include "window_attention_index.h"
#include <cstdlib>
#include <type_traits>

namespace brn {

constexpr int WS = 12;
constexpr int NTOK = 144;
constexpr int HD = 32;
constexpr int KV_LD = 36;          // floats per LDS row of K and V
constexpr int VT_LD = 148;         // 16-bit elements per LDS row of V^T (split and bf16 kernels)

// ---- what the three kernels share, each piece once.  Token helpers: WSZ = window side (7 only in the fp32 kernel) ----
// source row of window token t of window (wr, wc) of image b (roll + partition), -1 = pad token
template <int WSZ = WS>
__device__ __forceinline__ int att_tok_src(const WindowAttnParams& p, int b, int wr, int wc, int t) {
    const int ti = t / WSZ, tj = t - ti * WSZ;
    int sh = wr * WSZ + ti + p.shift, sw = wc * WSZ + tj + p.shift;   // shifted[i] = x[(i + shift) mod Hp] (swin.rs:412-444)
    if (sh >= p.Hp) sh -= p.Hp;
    if (sw >= p.Wp) sw -= p.Wp;
    return (sh < p.H && sw < p.W) ? (b * p.H + sh) * p.W + sw : -1;
}
// SW-MSA region id of window token t (h_slices / w_slices, swin.rs:608-629), by its position on the shifted, padded canvas
template <int WSZ = WS>
__device__ __forceinline__ int att_region(const WindowAttnParams& p, int wr, int wc, int t) {
    const int ti = t / WSZ, tj = t - ti * WSZ;
    const int ph = wr * WSZ + ti, pw = wc * WSZ + tj;
    const int fh = ph < p.Hp - WSZ ? 0 : (ph < p.Hp - p.shift ? 1 : 2);
    const int fw = pw < p.Wp - WSZ ? 0 : (pw < p.Wp - p.shift ? 1 : 2);
    return fh * 3 + fw;
}
// the shift mask (swin.rs:283-296) is non-zero only in the last row / column of windows; elsewhere it would add +0.0 to every score,
// which the result cannot see (a -0.0 score becomes +0.0; max and exp treat them alike)
template <int WSZ = WS>
__device__ __forceinline__ bool att_has_mask(const WindowAttnParams& p, int wr, int wc) {
    return p.shift > 0 && ((wr == p.Hp / WSZ - 1) | (wc == p.Wp / WSZ - 1));
}
// relative position index (swin.rs:182-184) of a (query, key) pair: att_qbase, att_qrev, att_koff, att_key0 (kernels/window_attention_index.h)
// v_max3_f32 spelled out: in the bf16 kernel fmaxf came with a canonicalising v_max x, x in front of every maximum (the scores are MFMA /
// fma results: never signalling; in the split kernel hipcc forms the same 18 v_max3_f32 per tile from fmaxf as well).  A maximum is exact,
// so for finite scores the grouping does not change the result; a NaN score still reaches the output through exp and the row sum
__device__ __forceinline__ float max3f(float a, float b, float c) {
    float r;
    asm("v_max3_f32 %0, %1, %2, %3" : "=v"(r) : "v"(a), "v"(b), "v"(c));
    return r;
}

// ---- split and bf16 kernels: 16-bit operands (E = __bf16 or _Float16), LDS images Kp[key][32 d] and Vt[d][VT_LD keys] of
// kernels/attention_mfma.h (the split kernel's row = plane * NTOK + key: NTOK % 16 == 0, so the plane does not change the swizzle) ----
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
// every global load goes out unconditionally from a clamped address: a pad token (src < 0) reads row 0 and is replaced afterwards
template <typename E>
__device__ __forceinline__ const E* att_row_ptr(const E* qkv, int src, int C3) { return qkv + (long)max(src, 0) * C3; }
// H (mode f32_half2): the two planes are fp16 planes of the scaled operands (kernels/split_planes.h, split_pair_h) — q (with its head_dim^-0.5), k
// and v scaled by 8, the un-normalised probabilities (in (0, 1]) by 2048 — on v_mfma_f32_16x16x32_f16; the scores and the output are
// un-scaled exactly.  ~2^-22 relative per product instead of 2^-16.
constexpr float ATT_H_QKV = 8.0f, ATT_H_P = 2048.0f;
// eight floats r (used up) -> NP plane fragments: bf16 (x ~ x_h + x_l [+ x_ll]), or with H the two fp16 planes of s x (bf16x8 = the 16-byte container)
template <int NP, bool H>
__device__ __forceinline__ void att_split8(float (&r)[8], const float s, bf16x8 (&out)[NP]) {
    if constexpr (H) {
        u32x4 hi, lo;
#pragma unroll
        for (int e = 0; e < 4; ++e) { unsigned a, b; split_pair_h(r[2 * e], r[2 * e + 1], s, a, b); hi[e] = a; lo[e] = b; }
        out[0] = __builtin_bit_cast(bf16x8, hi);
        out[1] = __builtin_bit_cast(bf16x8, lo);
    } else {
#pragma unroll
        for (int pl = 0; pl < NP; ++pl) {
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                const __bf16 h = (__bf16)r[e];
                out[pl][e] = h;
                r[e] -= (float)h;
            }
        }
    }
}
// acc + the NP (NP + 1) / 2 leading plane products of a . b, smallest first
template <int NP, bool H>
__device__ __forceinline__ f32x4 att_plane_mfma(const bf16x8 (&a)[NP], const bf16x8 (&b)[NP], f32x4 acc) {
    if constexpr (NP == 2) {
        acc = att_mfma<H>(a[1], b[0], acc);
        acc = att_mfma<H>(a[0], b[1], acc);
    }
    return att_mfma<H>(a[0], b[0], acc);
}
// lane group g's rows of the two d tiles of a query's output (o0 * inv: d = 4g .. 4g + 3 of the head, o1 * inv: 16 further) in the form the proj
// GEMM reads; FORMS = the forms the calling kernel can be asked for: planes by p.out_planes, else 16-bit elements E or fp32
enum : unsigned { ST_F32 = 1, ST_S16 = 2, ST_P2 = 4, ST_P3 = 8, ST_H2 = 16 };
template <unsigned FORMS, typename E = float>
__device__ __forceinline__ void att_store(const WindowAttnParams& p, int qsrc, int head, int g, const f32x4 o0, const f32x4 o1, const float inv) {
    const int C = p.C, col = head * HD + g * 4;
    if ((FORMS & ST_P3) && p.out_planes == 3) {           // mode f32_split3: the 3-plane P layout (rows 1.5x as long)
        float* orow = p.out + (long)qsrc * (C + C / 2);
        store_planes<3>(orow, col, o0 * inv), store_planes<3>(orow, col + 16, o1 * inv);
    } else if ((FORMS & ST_H2) && p.out_planes == 2) {    // mode f32_half2: two fp16 planes of out_h2 * out (rows as long as fp32 rows)
        float* orow = p.out + (long)qsrc * C;
        store_planes_h(orow, col, o0 * inv, p.out_h2), store_planes_h(orow, col + 16, o1 * inv, p.out_h2);
    } else if ((FORMS & ST_P2) && p.out_planes == 2) {    // the P layout: a head's 32 outputs are one K tile of the row
        float* orow = p.out + (long)qsrc * C;
        store_planes<2>(orow, col, o0 * inv), store_planes<2>(orow, col + 16, o1 * inv);
    } else if constexpr ((FORMS & ST_S16) != 0) {
        E* op = reinterpret_cast<E*>(p.out) + (long)qsrc * C + head * HD + g * 4;
        vec4<E> h0, h1;
#pragma unroll
        for (int e = 0; e < 4; ++e) { h0[e] = (E)(o0[e] * inv); h1[e] = (E)(o1[e] * inv); }
        *reinterpret_cast<vec4<E>*>(op) = h0, *reinterpret_cast<vec4<E>*>(op + 16) = h1;
    } else {
        float* op = p.out + (long)qsrc * C + head * HD + g * 4;
        *reinterpret_cast<f32x4*>(op) = o0 * inv, *reinterpret_cast<f32x4*>(op + 16) = o1 * inv;
    }
}

// Both kernels take TWO geometries (the full- and the half-scale map of a co-batched backbone pass, same C / heads / shift):
// blocks [0, nblk0) work on pa, the rest on pb — one launch, one ramp and one tail instead of two (the half-scale launch alone
// fills a fifth of the CU slots).  nblk0 = all blocks when there is only one map.  (The split and the bf16 kernel take a WindowOrder
// instead: the same two geometries, their windows in the order the launcher chose.)
// WSZ = window side: 12 (Swin-B / L, swin.rs:60,74) or 7 (Swin-T / S, swin.rs:32,46); head_dim is 32 in all four configurations.
// A window holds WSZ^2 tokens = NT16 key / query tiles of 16; the tail of the last tile (49 -> 64) is dummy: zero K / V rows, scores
// forced to -3e38 so that they leave the softmax, queries never stored.
// NWV = waves per workgroup: 3 (three query tiles each at window 12) or 9 (one query tile each: the workgroup lives a third as long on
// the same 41.5 KB of LDS = 3 workgroups per CU; at batch 1 a stage-2 launch is 1080 workgroups on 768 slots = two rounds whatever
// the wave count, so the round time is what counts)
// IOB = the qkv matrix and the output are bf16 (compute mode BRN_BF16 with a window the bf16 kernel below is not built for: window 7 of
// Swin-T / S): operands are widened on load — a pad token's q / k / v is the qkv bias rounded to bf16, what the qkv GEMM of that mode would
// have stored — the arithmetic stays the exact fp32 MFMA chain, the result is rounded once on store.
template <int IOB>
__device__ __forceinline__ f32x4 att_load4(const float* base, long off) {
    if constexpr (IOB != 0) {                   // 1: bf16 matrices, 2: fp16 matrices (compute mode BRN_F16)
        using E = std::conditional_t<IOB == 2, _Float16, __bf16>;
        typedef E ex4_ld __attribute__((ext_vector_type(4)));
        const ex4_ld h = *reinterpret_cast<const ex4_ld*>(reinterpret_cast<const E*>(base) + off);
        return f32x4{(float)h[0], (float)h[1], (float)h[2], (float)h[3]};
    } else return *reinterpret_cast<const f32x4*>(base + off);
}
template <int IOB>
__device__ __forceinline__ f32x4 att_bias4(const float* bias) {
    f32x4 v = *reinterpret_cast<const f32x4*>(bias);
    if constexpr (IOB != 0) {
        using E = std::conditional_t<IOB == 2, _Float16, __bf16>;
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = (float)(E)v[e];
    }
    return v;
}
template <int WSZ, int NWV = 3, int IOB = 0>
__global__ void __launch_bounds__(NWV * 64) window_attention_f32_kernel(const WindowAttnParams pa, const WindowAttnParams pb, const int nblk0) {
    constexpr int WS = WSZ, NTOK = WSZ * WSZ, NT16 = (NTOK + 15) / 16, NPADTOK = NT16 * 16;
    constexpr int NTHR = NWV * 64;
    const bool second = (int)blockIdx.x >= nblk0;
    const WindowAttnParams& p = second ? pb : pa;
    __shared__ __attribute__((aligned(16))) float Ks[NPADTOK * KV_LD];
    __shared__ __attribute__((aligned(16))) float Vs[NPADTOK * KV_LD];
    __shared__ int src_s[NPADTOK];   // source token offset (pixel index) or -1 for a pad token
    __shared__ int rid_s[NPADTOK];   // SW-MSA region id of the token (swin.rs:608-629)
    __shared__ float tab_s[(2 * WS - 1) * (2 * WS - 1)];   // this head's column of relative_position_bias_table

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int head = blockIdx.y;
    const int nWw = p.Wp / WS, nW = (p.Hp / WS) * nWw;
    const int bw = second ? (int)blockIdx.x - nblk0 : (int)blockIdx.x;
    const int b = bw / nW, w = bw - b * nW;      // window batch index is b*nW + w (swin.rs:456-458)
    const int wr = w / nWw, wc = w - wr * nWw;
    const int C = p.C, C3 = 3 * C;

    if (tid < NTOK) { src_s[tid] = att_tok_src<WS>(p, b, wr, wc, tid); rid_s[tid] = att_region<WS>(p, wr, wc, tid); }
    else if (tid < NPADTOK) { src_s[tid] = -1; rid_s[tid] = 0; }
    // window 12: the table is kept REVERSED and in log2 units (tab_s[j] = log2(e) * table[528 - j]): the 4 keys 16 kt + 4 g + {0..3} of
    // a lane lie in one window row (12 % 4 == 0), so their entries are 4 consecutive words — one index per key tile instead of
    // one per score — and the softmax runs on exp2.  Window 7 keeps the plain table and the per-score index.
    constexpr int TABN = (2 * WS - 1) * (2 * WS - 1);
    constexpr bool REV = WS == 12;
    for (int i = tid; i < TABN; i += NTHR) tab_s[i] = REV ? ATT_LOG2E * p.rel_table[head * TABN + (TABN - 1 - i)] : p.rel_table[head * TABN + i];
    const bool has_mask = att_has_mask<WS>(p, wr, wc);
    __syncthreads();

    // ---- stage K and V of this (window, head) into LDS: 144 rows x 8 float4 each ----
    for (int idx = tid; idx < NPADTOK * 8; idx += NTHR) {
        const int t = idx >> 3, c4 = (idx & 7) * 4;
        const int src = src_s[t];
        f32x4 kv, vv;
        if (src >= 0) { kv = att_load4<IOB>(p.qkv, (long)src * C3 + C + head * HD + c4); vv = att_load4<IOB>(p.qkv, (long)src * C3 + 2 * C + head * HD + c4); }
        else { kv = att_bias4<IOB>(p.qkv_bias + C + head * HD + c4); vv = att_bias4<IOB>(p.qkv_bias + 2 * C + head * HD + c4); }
        if (t >= NTOK) { kv = f32x4{0.f, 0.f, 0.f, 0.f}; vv = kv; }      // dummy tail of the last tile
        *reinterpret_cast<f32x4*>(Ks + t * KV_LD + c4) = kv;
        *reinterpret_cast<f32x4*>(Vs + t * KV_LD + c4) = vv;
    }
    __syncthreads();

    const int li = lane & 15, g = lane >> 4;

    // the Q fragment of the NEXT query tile is requested while this one is multiplied (8 registers; fetching all three up front
    // cost occupancy and was slower)
    auto load_q = [&](int qt, f32x4& q0, f32x4& q1) {
        const int qs = src_s[qt * 16 + li];
        if (qs >= 0) { q0 = att_load4<IOB>(p.qkv, (long)qs * C3 + head * HD + g * 8); q1 = att_load4<IOB>(p.qkv, (long)qs * C3 + head * HD + g * 8 + 4); }
        else { q0 = att_bias4<IOB>(p.qkv_bias + head * HD + g * 8); q1 = att_bias4<IOB>(p.qkv_bias + head * HD + g * 8 + 4); }
    };
    f32x4 qn0 = {0.f, 0.f, 0.f, 0.f}, qn1 = qn0;
    if (wave < NT16) load_q(wave, qn0, qn1);
    for (int qt = wave; qt < NT16; qt += NWV) {
        const int qtok = qt * 16 + li;
        const int qsrc = src_s[qtok];
        const int qrid = rid_s[qtok];
        const int qt_ = qtok < NTOK ? qtok : NTOK - 1;            // (dummy queries of the last tile compute on a valid row, never stored)
        const int qbase = att_qbase<WS>(qt_ / WS, qt_ % WS);
        // Q fragment: d = 8g .. 8g+7 of query row qtok, scaled before the product (swin.rs:278)
        const f32x4 qf0 = qn0 * p.scale, qf1 = qn1 * p.scale;
        if (qt + NWV < NT16) load_q(qt + NWV, qn0, qn1);
        // S^T = K . Q^T : 9 key tiles
        f32x4 st[NT16];
#pragma unroll
        for (int kt = 0; kt < NT16; ++kt) {
            st[kt] = att_score_f32(Ks + (kt * 16 + li) * KV_LD + g * 8, qf0, qf1, f32x4{0.f, 0.f, 0.f, 0.f});
            if (kt % 3 == 2) __builtin_amdgcn_sched_barrier(0);   // bound the scheduler's hoisting (register pressure)
        }
        // + relative position bias (swin.rs:284-285), + SW-MSA mask (swin.rs:288-297, value -100 swin.rs:651)
        float mx = ATT_NEG;
        if constexpr (REV) {
            const int qrev = att_qrev<WS>(qt_ / WS, qt_ % WS);
#pragma unroll
            for (int kt = 0; kt < NT16; ++kt) {
                const float* tb = tab_s + qrev + att_koff<WS>(att_key0(kt, g));
#pragma unroll
                for (int r = 0; r < 4; ++r) st[kt][r] = fmaf(st[kt][r], ATT_LOG2E, tb[r]);
            }
            if (has_mask) {
#pragma unroll
                for (int kt = 0; kt < NT16; ++kt) {
#pragma unroll
                    for (int r = 0; r < 4; ++r) st[kt][r] += (rid_s[kt * 16 + g * 4 + r] != qrid) ? -100.0f * ATT_LOG2E : 0.0f;
                }
            }
#pragma unroll
            for (int kt = 0; kt < NT16; ++kt) mx = fmaxf(fmaxf(mx, fmaxf(st[kt][0], st[kt][1])), fmaxf(st[kt][2], st[kt][3]));
        } else {
#pragma unroll
            for (int kt = 0; kt < NT16; ++kt) {
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int key = kt * 16 + g * 4 + r;
                    const int kk = key < NTOK ? key : 0;
                    float s = st[kt][r] + tab_s[max(0, qbase - kk - (WS - 1) * (kk / WS))];
                    if (p.shift > 0) s += (rid_s[key] != qrid) ? -100.0f : 0.0f;
                    if (NTOK % 16 != 0 && key >= NTOK) s = ATT_NEG;
                    st[kt][r] = s;
                    mx = fmaxf(mx, s);
                }
            }
        }
        mx = att_group_max(mx);
        float sum = 0.f;
#pragma unroll
        for (int kt = 0; kt < NT16; ++kt) {
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const float e = REV ? __builtin_amdgcn_exp2f(st[kt][r] - mx) : __expf(st[kt][r] - mx);
                st[kt][r] = e;
                sum += e;
            }
        }
        sum = att_group_sum(sum);
        // O^T = V^T . P^T : two d tiles
        f32x4 o0 = {0.f, 0.f, 0.f, 0.f}, o1 = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int kt = 0; kt < NT16; ++kt) {
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const float* vp = Vs + (kt * 16 + g * 4 + r) * KV_LD + li;
                o0 = att_pv_f32(vp, 0, st[kt][r], o0);
                o1 = att_pv_f32(vp, 1, st[kt][r], o1);
            }
            if (kt % 2 == 1) __builtin_amdgcn_sched_barrier(0);
        }
        // lane holds O^T[d = 16*dt + 4g + r][query = li]; softmax denominator applied here (swin.rs:300,303)
        if (qsrc >= 0 && qtok < NTOK) {
            const float inv = 1.0f / sum;
            att_store<ST_P3 | ST_H2 | (IOB != 0 ? ST_S16 : ST_F32), std::conditional_t<IOB == 2, _Float16, __bf16>>(p, qsrc, head, g, o0, o1, inv);
        }
    }
}

// =====================================================================================================================
// window_attention_split_kernel — the same fused window attention on the bf16 matrix cores (compute modes f32_split2 /
// bf16_operands).  q*scale, K, V and the softmax numerators P are split into NP bf16 terms (x ~ x_h + x_l) in registers /
// while staging, every product is the sum of the NP*(NP+1)/2 leading plane products on v_mfma_f32_16x16x32_bf16 (head_dim
// 32 = ONE MFMA k), accumulation, bias, mask and softmax stay fp32.  MFMA cycles per 16-query tile: 57 x 16 vs 144 x 32.
// LDS (40.2 KB -> 4 workgroups per CU instead of 3: the 864 workgroups of a Swin-L stage-2 launch fit one round):
//   Kp[pl][key][32 d]   bf16, 64-byte rows, 16-byte chunk c stored at c ^ perm[(key >> 2) & 3], perm = {0,2,3,1}
//                       (conflict-free ds_read_b128 of the A operand: row = key, k = d = 8g + j)
//   Vt[pl][d][148 keys] bf16 (V transposed): the A operand of O^T = V^T P^T needs 8 keys per lane for a fixed d; the k slots
//                       of an MFMA over key tiles (2t, 2t+1) are ordered so that lane group g contracts keys 16*(2t)+4g+0..3
//                       and 16*(2t+1)+4g+0..3 — exactly the keys whose P^T values the lane already holds in its S^T
//                       accumulators (C/D map row = 4g + reg) — so P never leaves registers.
// Queries: the REAL tokens of the window only, packed into 16-query tiles (kernels/window_geometry.h) — the reference crops a pad
// token's output row (swin.rs:387-401), and a query's result depends on its own lane group only, so the rows that are stored keep
// their bits.  Pad tokens stay KEYS.  A window on the padded border has fewer tiles (a corner window of the 32 x 32 map: 64 real
// queries = 4 tiles of 9); the launcher orders the windows so that those workgroups come last (WindowOrder).
// =====================================================================================================================
// which (window, head) a workgroup of the split / bf16 kernels works on: grid = (windows, heads or head groups), flattened x-major;
// ord.heads_inner puts the workgroups of one window next to each other and the windows in ord's order (most query tiles first)
struct AttBlock { WindowId win; int head; };
__device__ __forceinline__ AttBlock att_block(const WindowOrder& ord) {
    int flat = blockIdx.x, head = blockIdx.y;
    if (ord.heads_inner) {
        const int f = blockIdx.y * gridDim.x + blockIdx.x;
        flat = f / (int)gridDim.y;
        head = f - flat * (int)gridDim.y;
    }
    AttBlock r;
    r.win = order_window(ord, flat);
    r.head = head;
    return r;
}
// H (mode f32_half2): two fp16 planes on v_mfma_f32_16x16x32_f16 (ATT_H_QKV, att_split8)
template <int NP, bool H = false>
__global__ void __launch_bounds__(ATT_THREADS) __attribute__((amdgpu_waves_per_eu(3, 3))) window_attention_split_kernel(const WindowAttnParams pa, const WindowAttnParams pb, const WindowOrder ord) {
    static_assert(!H || NP == 2, "fp16 planes come in pairs");
    const AttBlock blk = att_block(ord);
    const bool second = blk.win.geom != 0;
    const WindowAttnParams& p = second ? pb : pa;
    __shared__ __attribute__((aligned(16))) __bf16 Kp[NP * NTOK * HD];
    __shared__ __attribute__((aligned(16))) __bf16 Vt[NP * HD * VT_LD];
    constexpr int TABN = (2 * WS - 1) * (2 * WS - 1);
    // the head's bias column REVERSED, in plain units: rev_s[j] = table[528 - j].  The 4 keys 16 kt + 4 g + {0..3} of a lane lie in one
    // window row, so their words are rev_s[qrev + koff + 0..3]: one address per key tile (kernels/window_attention_index.h; the largest
    // index a real query can form is 528)
    static_assert(WS % 4 == 0 && NTOK % 16 == 0, "the four keys of a lane's tile chunk lie in one window row");
    __shared__ float rev_s[TABN];
    __shared__ unsigned char rid_s[NTOK];
    __shared__ __attribute__((aligned(16))) float qb_s[HD];    // the head's q bias: what a pad query is (kept out of the loop's registers)

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int li = lane & 15, g = lane >> 4;
    const int head = blk.head;
    const int b = blk.win.b, wr = blk.win.wr, wc = blk.win.wc;
    const int C = p.C, C3 = 3 * C;
    // the query slots of this window: its real tokens only (a pad query's row is cropped, swin.rs:387-401; pad KEYS stay), wave-uniform
    const WindowReal wg = window_real(wr, wc, p.shift, p.H, p.W, p.Hp, p.Wp, ord.pack != 0);
    const int nq = wg.nq, ntile = window_tiles(wg);
    const bool has_mask = att_has_mask(p, wr, wc);
    auto tok_src = [&](int t) { return att_tok_src(p, b, wr, wc, t); };     // (kept a lambda: called directly, the helper compiled to other scalar code)

    // ---- every global load of the workgroup goes out FIRST, unconditionally, from clamped addresses (a pad token reads row 0 and is
    // replaced by the qkv bias afterwards, by a select): the K / V rows of the thread's three staging items = (token pair, 4-wide d chunk),
    // the bias chunks a pad token needs, the table words, the wave's first Q fragment.  The source rows are computed in registers: with
    // src_s built first and the loads inside the staging loop behind a lane-dependent pointer select, hipcc waited vmcnt(0) per
    // iteration and per query tile — six memory round trips one after the other in a workgroup that lives little longer than that. ----
    static_assert((NTOK / 2) * 8 == 3 * ATT_THREADS && ATT_THREADS % 8 == 0 && 3 * ATT_THREADS >= TABN, "three staging items and three table words per thread");
    const int c4 = (tid & 7) * 4;                                     // the same d chunk in all three items of a thread
    const float* kbp = p.qkv_bias + C + head * HD + c4;
    const f32x4 kbias = *reinterpret_cast<const f32x4*>(kbp);
    const f32x4 vbias = *reinterpret_cast<const f32x4*>(kbp + C);
    f32x4 kvr[3][2], vvr[3][2];
    int ssrc[3][2];
#pragma unroll
    for (int it = 0; it < 3; ++it) {
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            const int src = tok_src(((tid >> 3) + it * (ATT_THREADS / 8)) * 2 + u);
            ssrc[it][u] = src;
            const float* kp = att_row_ptr(p.qkv, src, C3) + C + head * HD + c4;
            kvr[it][u] = *reinterpret_cast<const f32x4*>(kp);
            vvr[it][u] = *reinterpret_cast<const f32x4*>(kp + C);
        }
    }
    float tbw[3];
#pragma unroll
    for (int j = 0; j < 3; ++j) tbw[j] = p.rel_table[head * TABN + min(tid + j * ATT_THREADS, TABN - 1)];
    const float* qbp = p.qkv_bias + head * HD + g * 8;
    const f32x4 qbias0 = *reinterpret_cast<const f32x4*>(qbp);
    const f32x4 qbias1 = *reinterpret_cast<const f32x4*>(qbp + 4);
    // the Q fragment of the NEXT query tile is requested while this one is multiplied (8 registers; all three up front cost occupancy)
    // (a slot past nq — the tail of the last tile, or a wave with no tile — reads the last real query's row and is never stored)
    int qsrc_n, qtok_n;
    f32x4 qn0, qn1;
    auto load_q = [&](int slot) {
        qtok_n = slot_token(wg, min(slot, nq - 1));
        qsrc_n = tok_src(qtok_n);
        const float* qp = att_row_ptr(p.qkv, qsrc_n, C3) + head * HD + g * 8;
        qn0 = *reinterpret_cast<const f32x4*>(qp);
        qn1 = *reinterpret_cast<const f32x4*>(qp + 4);
    };
    load_q(wave * 16 + li);

    if (tid < NTOK) rid_s[tid] = (unsigned char)att_region(p, wr, wc, tid);

    // ---- consume: K (row-major, swizzled) and V (transposed), split into planes; pad tokens take the qkv bias; the table ----
#pragma unroll
    for (int it = 0; it < 3; ++it) {
        const int tp = (tid >> 3) + it * (ATT_THREADS / 8);
        f32x4 kv[2], vv[2];
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            kv[u] = ssrc[it][u] < 0 ? kbias : kvr[it][u];
            vv[u] = ssrc[it][u] < 0 ? vbias : vvr[it][u];
        }
        // (4-wide K chunks and key PAIRS of V: not att_split8 — with it the fp16-plane kernel's store addresses compiled differently)
        if constexpr (H) {
#pragma unroll
            for (int u = 0; u < 2; ++u) {
                bf16x4 sp[2];
                split4h<false>(kv[u], 0xffffffffu, ATT_H_QKV, sp);
#pragma unroll
                for (int pl = 0; pl < 2; ++pl) *reinterpret_cast<bf16x4*>(att_k_chunk<HD>(Kp + (pl * NTOK + tp * 2 + u) * HD, tp * 2 + u, c4 >> 3) + (c4 & 4)) = sp[pl];
            }
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                unsigned hi, lo;
                split_pair_h(vv[0][e], vv[1][e], ATT_H_QKV, hi, lo);                          // keys (2tp, 2tp+1) of row d = c4+e
                *reinterpret_cast<unsigned*>(Vt + (c4 + e) * VT_LD + tp * 2) = hi;
                *reinterpret_cast<unsigned*>(Vt + (HD + c4 + e) * VT_LD + tp * 2) = lo;
            }
        } else {
#pragma unroll
            for (int u = 0; u < 2; ++u) {
                f32x4 r = kv[u];
#pragma unroll
                for (int pl = 0; pl < NP; ++pl) {
                    bf16x4 h;
#pragma unroll
                    for (int e = 0; e < 4; ++e) h[e] = (__bf16)r[e];
                    *reinterpret_cast<bf16x4*>(att_k_chunk<HD>(Kp + (pl * NTOK + tp * 2 + u) * HD, tp * 2 + u, c4 >> 3) + (c4 & 4)) = h;
                    if (pl + 1 < NP) {
#pragma unroll
                        for (int e = 0; e < 4; ++e) r[e] -= (float)h[e];
                    }
                }
            }
            f32x4 r0 = vv[0], r1 = vv[1];
#pragma unroll
            for (int pl = 0; pl < NP; ++pl) {
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const __bf16 h0 = (__bf16)r0[e], h1 = (__bf16)r1[e];
                    att_vt_store(Vt + (pl * HD + c4 + e) * VT_LD, tp, h0, h1);
                    if (pl + 1 < NP) { r0[e] -= (float)h0; r1[e] -= (float)h1; }
                }
            }
        }
    }
#pragma unroll
    for (int j = 0; j < 3; ++j)
        if (tid + j * ATT_THREADS < TABN) rev_s[TABN - 1 - (tid + j * ATT_THREADS)] = tbw[j];
    if (tid < 64 && li == 0) {
        *reinterpret_cast<f32x4*>(qb_s + g * 8) = qbias0;
        *reinterpret_cast<f32x4*>(qb_s + g * 8 + 4) = qbias1;
    }
    __syncthreads();

    // per key tile: the byte offset of att_koff(16 kt + 4 g), once per workgroup; added to an LDS address the compiler cannot take apart
    // (window_attention_bf16_kernel: with `rev_s + qrev + koff` it re-associates the array's base out of the sum, four VALU per key tile)
    typedef __attribute__((address_space(3))) const float lds_cfloat;
    unsigned koffb[9];
#pragma unroll
    for (int kt = 0; kt < 9; ++kt) koffb[kt] = (unsigned)att_koff(att_key0(kt, g)) * 4u;
    for (int qt = wave; qt < ntile; qt += 3) {
        const int slot = qt * 16 + li;
        const int qtok = qtok_n;                                     // a real token of the window, also for a slot past nq (load_q clamps)
        const int qsrc = qsrc_n;
        const int qrid = rid_s[qtok];
        const int qrev = att_qrev(qtok / WS, qtok % WS);
        // Q fragment (B operand of S^T = K Q^T): d = 8g .. 8g+7 of this lane's query, scaled (swin.rs:278), split
        bf16x8 qf[NP];
        {
            const f32x4 q0 = qsrc < 0 ? *reinterpret_cast<const f32x4*>(qb_s + g * 8) : qn0;
            const f32x4 q1 = qsrc < 0 ? *reinterpret_cast<const f32x4*>(qb_s + g * 8 + 4) : qn1;
            float r[8];
#pragma unroll
            for (int e = 0; e < 4; ++e) { r[e] = q0[e] * p.scale; r[4 + e] = q1[e] * p.scale; }
            if (qt + 3 < ntile) load_q(slot + 48);
            att_split8<NP, H>(r, ATT_H_QKV, qf);
        }
        f32x4 st[9];
#pragma unroll
        for (int kt = 0; kt < 9; ++kt) {
            bf16x8 kf[NP];
#pragma unroll
            for (int pl = 0; pl < NP; ++pl) kf[pl] = att_k_frag<HD>(Kp + (pl * NTOK + kt * 16 + li) * HD, kt * 16 + li, g);
            st[kt] = att_plane_mfma<NP, H>(kf, qf, f32x4{0.f, 0.f, 0.f, 0.f});
            if (kt % 3 == 2) __builtin_amdgcn_sched_barrier(0);
        }
        // + relative position bias (swin.rs:284-285), + SW-MSA mask (swin.rs:288-297, value -100 swin.rs:651): per score the same
        // operations on the same operands as with one table index per score
        unsigned tbq = (unsigned)(unsigned long)(lds_cfloat*)(rev_s + qrev);
        asm volatile("" : "+v"(tbq));
#pragma unroll
        for (int kt = 0; kt < 9; ++kt) {
            lds_cfloat* tb = (lds_cfloat*)(unsigned long)(tbq + koffb[kt]);
#pragma unroll
            for (int r = 0; r < 4; ++r) st[kt][r] = H ? fmaf(st[kt][r], 1.0f / (ATT_H_QKV * ATT_H_QKV), tb[r]) : st[kt][r] + tb[r];
        }
        if (has_mask) {                                              // (hipcc reads the four ids of a chunk as one word and compares its bytes)
#pragma unroll
            for (int kt = 0; kt < 9; ++kt) {
#pragma unroll
                for (int r = 0; r < 4; ++r) st[kt][r] += ((int)rid_s[att_key0(kt, g) + r] != qrid) ? -100.0f : 0.0f;
            }
        }
        float mx = ATT_NEG;
#pragma unroll
        for (int kt = 0; kt < 9; ++kt) mx = max3f(max3f(mx, st[kt][0], st[kt][1]), st[kt][2], st[kt][3]);
        mx = att_group_max(mx);
        float sum = 0.f;
#pragma unroll
        for (int kt = 0; kt < 9; ++kt) {
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const float e = __expf(st[kt][r] - mx);
                st[kt][r] = e;
                sum += e;
            }
        }
        sum = att_group_sum(sum);
        // O^T = V^T P^T: 5 k-steps of 32 keys (key tiles 2t, 2t+1; the 10th tile does not exist: zero operands)
        f32x4 o0 = {0.f, 0.f, 0.f, 0.f}, o1 = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int t = 0; t < 5; ++t) {
            float pr[8];
            att_p_step(st, t, pr);
            bf16x8 pf[NP];
            att_split8<NP, H>(pr, ATT_H_P, pf);
#pragma unroll
            for (int dt = 0; dt < 2; ++dt) {
                bf16x8 vf[NP];
#pragma unroll
                for (int pl = 0; pl < NP; ++pl) vf[pl] = att_vt_frag(Vt + (pl * HD + dt * 16 + li) * VT_LD + g * 4, t, 2 * t + 1 < 9);
                if (dt == 0) o0 = att_plane_mfma<NP, H>(vf, pf, o0);
                else o1 = att_plane_mfma<NP, H>(vf, pf, o1);
            }
            __builtin_amdgcn_sched_barrier(0);
        }
        if (qsrc >= 0 && slot < nq) {
            const float inv = (H ? 1.0f / (ATT_H_P * ATT_H_QKV) : 1.0f) / sum;
            att_store<ST_F32 | (H ? ST_H2 : ST_P2)>(p, qsrc, head, g, o0, o1, inv);
        }
    }
}

// =====================================================================================================================
// window_attention_bf16_kernel — compute mode BRN_BF16: qkv arrives as bf16 (the qkv GEMM's output), `out` leaves as bf16
// (the proj GEMM's input).  Same structure and LDS images as window_attention_split_kernel<1>; what changes is the staging
// (16-byte loads of 8 bf16, no split) and that q's scale is applied to the fp32 scores instead of to q (q is already
// rounded to bf16: scaling the accumulator avoids a second rounding; identical in real arithmetic, swin.rs:278).
// =====================================================================================================================
template <typename E>
__device__ __forceinline__ vec8<E> bias8_s16(const float* bp) {
    vec8<E> r;
#pragma unroll
    for (int e = 0; e < 8; ++e) r[e] = (E)bp[e];
    return r;
}

// Two heads per workgroup (6 waves: waves 0-2 head 2y, waves 3-5 head 2y + 1): a token's K (or V) rows of two adjacent heads are one
// 128-byte line, so the staging loads fetch whole lines (one head per workgroup used half of every line it touched).
// F16: qkv / out are fp16 matrices (compute mode BRN_F16): the same kernel on v_mfma_f32_16x16x32_f16
template <int ATT_BF16_HPW, bool F16 = false>
__global__ void __launch_bounds__(ATT_BF16_HPW * ATT_THREADS) __attribute__((amdgpu_waves_per_eu(5, 8))) window_attention_bf16_kernel(const WindowAttnParams pa, const WindowAttnParams pb, const WindowOrder ord) {
    using E = std::conditional_t<F16, _Float16, __bf16>;
    typedef vec8<E> ex8;
    const AttBlock blk = att_block(ord);
    const bool second = blk.win.geom != 0;
    const WindowAttnParams& p = second ? pb : pa;
    constexpr int TABN = (2 * WS - 1) * (2 * WS - 1);                 // 529
    __shared__ __attribute__((aligned(16))) E Kp_[ATT_BF16_HPW][NTOK * HD];
    __shared__ __attribute__((aligned(16))) E Vt_[ATT_BF16_HPW][HD * VT_LD];
    // a head's bias table REVERSED and in log2 units: rev[j] = log2(e) * table[528 - j].  The 4 keys 16 kt + 4 g + {0..3} of a lane
    // lie in one window row (12 % 4 == 0), so their table entries are 4 consecutive words of rev: one index per key tile
    // instead of one per score (the index arithmetic was most of the softmax's VALU work).
    __shared__ float rev_[ATT_BF16_HPW][TABN + 3];
    __shared__ __attribute__((aligned(4))) unsigned char rid_s[NTOK];

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int hp = wave / 3, wv = wave - 3 * hp;                      // head of the pair, wave within the head
    const int head0 = blk.head * ATT_BF16_HPW, head = head0 + hp;
    const int b = blk.win.b, wr = blk.win.wr, wc = blk.win.wc;
    const int C = p.C, C3 = 3 * C;
    // the query slots of this window: its real tokens only (window_attention_split_kernel), wave-uniform
    const WindowReal wg = window_real(wr, wc, p.shift, p.H, p.W, p.Hp, p.Wp, ord.pack != 0);
    const int nq = wg.nq, ntile = window_tiles(wg);
    const E* qkv = reinterpret_cast<const E*>(p.qkv);
    const int li = lane & 15, g = lane >> 4;
    const bool has_mask = att_has_mask(p, wr, wc);
    auto tok_src = [&](int t) { return att_tok_src(p, b, wr, wc, t); };
    E* Kp = Kp_[hp];
    E* Vt = Vt_[hp];
    const float* rev_s = rev_[hp];

    // ---- every global load of the workgroup goes out FIRST, unconditionally, from clamped addresses (a pad token reads row 0 and is
    // fixed up afterwards): the three Q fragments, the head's bias table, the K / V rows.  The first version loaded under lane-dependent
    // branches and in two dependent loops — hipcc waits vmcnt(0) at every join — and paid five HBM round trips one after the other
    // (3 table iterations, 2 staging iterations) in a kernel whose lifetime is little more than its memory latency. ----
    constexpr int NTHR = ATT_BF16_HPW * ATT_THREADS;
    constexpr int NITEM = (NTOK / 2) * 4 * ATT_BF16_HPW;                // (token pair, head of the pair, 8-wide d chunk)
    constexpr int NTAB = ATT_BF16_HPW * TABN;
    static_assert(2 * NTHR >= NITEM && 3 * NTHR >= NTAB, "two staging items and three table words per thread cover a head group");
    ex8 qf[3];
    int qsrc_[3];
#pragma unroll
    for (int u = 0; u < 3; ++u) {
        const int qs = tok_src(slot_token(wg, min((wv + 3 * u) * 16 + li, nq - 1)));     // (a slot past nq: the last real query's row, never stored)
        qsrc_[u] = qs;
        qf[u] = *reinterpret_cast<const ex8*>(att_row_ptr(qkv, qs, C3) + head * HD + g * 8);
    }
    float tbw[3];
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        const int i = min(tid + j * NTHR, NTAB - 1), hh = i / TABN, jj = i - hh * TABN;
        tbw[j] = p.rel_table[(head0 + hh) * TABN + (TABN - 1 - jj)];
    }
    ex8 kv[2][2], vv[2][2];
    int ssrc[2][2];
#pragma unroll
    for (int it = 0; it < 2; ++it) {
        const int idx = min(tid + it * NTHR, NITEM - 1);
        const int c8 = (idx & 3) * 8, hh = (idx >> 2) & (ATT_BF16_HPW - 1), tp = idx / (4 * ATT_BF16_HPW);
        const int hd = (head0 + hh) * HD;
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            const int src = tok_src(tp * 2 + u);
            ssrc[it][u] = src;
            const E* kp = att_row_ptr(qkv, src, C3) + C + hd + c8;
            kv[it][u] = *reinterpret_cast<const ex8*>(kp);
            vv[it][u] = *reinterpret_cast<const ex8*>(kp + C);
        }
    }
    if (tid < NTOK) rid_s[tid] = (unsigned char)att_region(p, wr, wc, tid);
    // ---- consume: table, K (row-major, chunk-swizzled), V (transposed); pad tokens take the qkv bias (swin.rs:359-366: their LayerNorm
    // output row is zero) in a second, divergent step that only the windows on the padded border execute ----
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        const int i = tid + j * NTHR;
        if (i < NTAB) { const int hh = i / TABN; rev_[hh][i - hh * TABN] = ATT_LOG2E * tbw[j]; }
    }
#pragma unroll
    for (int u = 0; u < 3; ++u)
        if (qsrc_[u] < 0) qf[u] = bias8_s16<E>(p.qkv_bias + head * HD + g * 8);
#pragma unroll
    for (int it = 0; it < 2; ++it) {
        const int idx = tid + it * NTHR;
        if (idx < NITEM) {
            const int c8 = (idx & 3) * 8, hh = (idx >> 2) & (ATT_BF16_HPW - 1), tp = idx / (4 * ATT_BF16_HPW);
            const int hd = (head0 + hh) * HD;
#pragma unroll
            for (int u = 0; u < 2; ++u) {
                if (ssrc[it][u] < 0) {
                    kv[it][u] = bias8_s16<E>(p.qkv_bias + C + hd + c8);
                    vv[it][u] = bias8_s16<E>(p.qkv_bias + 2 * C + hd + c8);
                }
            }
            // (att_k_chunk, spelled out: through the helper this kernel's staging addresses compiled to other vector code)
#pragma unroll
            for (int u = 0; u < 2; ++u) *reinterpret_cast<ex8*>(Kp_[hh] + (tp * 2 + u) * HD + (((c8 >> 3) ^ att_kswz<HD>(tp * 2 + u)) << 3)) = kv[it][u];
#pragma unroll
            for (int e = 0; e < 8; ++e) att_vt_store(Vt_[hh] + (c8 + e) * VT_LD, tp, vv[it][0][e], vv[it][1][e]);
        }
    }
    __syncthreads();

    const float scale2 = p.scale * ATT_LOG2E;
    ex8 ones8;
#pragma unroll
    for (int e = 0; e < 8; ++e) ones8[e] = (E)1.0f;
    // per key tile: koff = key0 + 11 (key0 / 12) for key0 = 16 kt + 4 g; the table word of (query, key0 + r) is rev[qrev + koff + r]
    // (byte offsets, one register per key tile, added to an LDS address the compiler cannot take apart: with `rev_s + qrev + koff[kt]`
    // it re-associated the array's constant base out of the sum and spent four VALU instructions per key tile on addresses: 94 of the
    // ~650 vector instructions of a query-tile triple)
    typedef __attribute__((address_space(3))) const float lds_cfloat;
    unsigned koffb[9];
#pragma unroll
    for (int kt = 0; kt < 9; ++kt) koffb[kt] = (unsigned)att_koff(att_key0(kt, g)) * 4u;
#pragma unroll
    for (int u = 0; u < 3; ++u) {
        const int qt = wv + 3 * u;
        if (qt >= ntile) break;                                       // wave-uniform: the window has fewer real queries
        const int slot = qt * 16 + li;
        const int qtok = slot_token(wg, min(slot, nq - 1));
        const int qsrc = qsrc_[u];
        const unsigned qrid4 = 0x01010101u * (unsigned)rid_s[qtok];
        const int qrev = att_qrev(qtok / WS, qtok % WS);
        f32x4 st[9];
#pragma unroll
        for (int kt = 0; kt < 9; ++kt) {
            st[kt] = att_mfma<F16>(att_k_frag<HD>(Kp + (kt * 16 + li) * HD, kt * 16 + li, g), qf[u], f32x4{0.f, 0.f, 0.f, 0.f});
            if (kt % 3 == 2) __builtin_amdgcn_sched_barrier(0);
        }
        float mx = ATT_NEG;
        unsigned tbq = (unsigned)(unsigned long)(lds_cfloat*)(rev_s + qrev);
        asm volatile("" : "+v"(tbq));
#pragma unroll
        for (int kt = 0; kt < 9; ++kt) {
            lds_cfloat* tb = (lds_cfloat*)(unsigned long)(tbq + koffb[kt]);
#pragma unroll
            for (int r = 0; r < 4; ++r) st[kt][r] = fmaf(st[kt][r], scale2, tb[r]);
        }
        if (has_mask) {
#pragma unroll
            for (int kt = 0; kt < 9; ++kt) {
                // byte r of x is 1 where key r lies in another region than the query, else 0: one byte-to-float conversion and one fma per
                // score, and the term added is exactly the reference's -100 (swin.rs:283-296, 651).  (region ids are 0 .. 8, so a byte of
                // the XOR is 0 .. 15: + 0x7f carries into bit 7 exactly when it is non-zero, and never into the next byte)
                const unsigned xr = *reinterpret_cast<const unsigned*>(rid_s + kt * 16 + g * 4) ^ qrid4;
                const unsigned x = ((xr + 0x7f7f7f7fu) >> 7) & 0x01010101u;
#pragma unroll
                for (int r = 0; r < 4; ++r) st[kt][r] = fmaf((float)((x >> (8 * r)) & 0xffu), -100.0f * ATT_LOG2E, st[kt][r]);
            }
        }
#pragma unroll
        for (int kt = 0; kt < 9; ++kt) mx = max3f(max3f(mx, st[kt][0], st[kt][1]), st[kt][2], st[kt][3]);
        mx = att_group_max(mx);
#pragma unroll
        for (int kt = 0; kt < 9; ++kt) {
#pragma unroll
            for (int r = 0; r < 4; ++r) st[kt][r] = __builtin_amdgcn_exp2f(st[kt][r] - mx);
        }
        // the row sums come out of the matrix pipe: a third "V" tile of ones makes every row of osum the sum over the keys of the
        // SAME bf16 weights the P V product uses (36 adds and two cross-lane steps per query tile less on the vector pipe)
        f32x4 o0 = {0.f, 0.f, 0.f, 0.f}, o1 = {0.f, 0.f, 0.f, 0.f}, osum = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int t = 0; t < 5; ++t) {
            float pr[8];
            att_p_step(st, t, pr);
            ex8 pf;
#pragma unroll
            for (int e = 0; e < 8; ++e) pf[e] = (E)pr[e];
#pragma unroll
            for (int dt = 0; dt < 2; ++dt) {
                const ex8 vf = att_vt_frag(Vt + (dt * 16 + li) * VT_LD + g * 4, t, 2 * t + 1 < 9);
                if (dt == 0) o0 = att_mfma<F16>(vf, pf, o0);
                else o1 = att_mfma<F16>(vf, pf, o1);
            }
            osum = att_mfma<F16>(ones8, pf, osum);
            __builtin_amdgcn_sched_barrier(0);
        }
        if (qsrc >= 0 && slot < nq) {
            const float inv = __builtin_amdgcn_rcpf(osum[0]);
            att_store<ST_S16, E>(p, qsrc, head, g, o0, o1, inv);
        }
    }
}

// which kernel, grid and block: select_window_attention (kernels/window_attention_select.h); here only the two process-wide switches and the launch
hipError_t launch_window_attention2(const WindowAttnParams& p, const WindowAttnParams* p2, hipStream_t s) {
    // BRN_ATT_HPW: two heads per workgroup of the bf16 kernel is the default — alone the launch is 6 % slower (3.25 against 3.05 ms per 8-image step),
    // but it reads whole 128-byte lines (one head touches half of every line it fetches: 8.5 GB read against 5.9 algorithmic), and with two sub-batch
    // streams sharing the HBM the step is 1.0 % faster (tools/ab_env.sh BRN_ATT_HPW "1 2"); BRN_ATT_HPW=1 selects one head
    static const int hpw = getenv("BRN_ATT_HPW") ? atoi(getenv("BRN_ATT_HPW")) : 2;
    static const int f32_waves = getenv("BRN_ATT_F32_WAVES") ? atoi(getenv("BRN_ATT_F32_WAVES")) : 9;
#ifdef BRN_DIAG_BUILD
    constexpr bool diag = true;
#else
    constexpr bool diag = false;
#endif
    const AttLaunch l = select_window_attention(p, p2, hpw, f32_waves, diag);
    if (l.kernel == ATT_INVALID) return hipErrorInvalidValue;
    const WindowAttnParams& q = p2 ? *p2 : p;
    // split / bf16 kernels: real queries only, windows with the most query tiles first (kernels/window_geometry.h; pack_q == 0: all 144
    // positions of every window in grid order, the form before).  A few integers computed here and passed by value: no table in memory
    WindowOrder ord;
    const WindowGeom geom[2] = {{p.B, p.H, p.W, p.Hp, p.Wp, p.shift}, {q.B, q.H, q.W, q.Hp, q.Wp, q.shift}};
    build_window_order(geom, p2 ? 2 : 1, (p.ws ? p.ws : WS) == WS && p.pack_q != 0, p.pack_q != 2, ord);
    const dim3 grid(l.grid_x, l.grid_y), block(l.block);
    switch (l.kernel) {
    case ATT_F32_W7: hipLaunchKernelGGL(window_attention_f32_kernel<7>, grid, block, 0, s, p, q, l.nblk0); break;
    case ATT_F32_W7_BF16: hipLaunchKernelGGL((window_attention_f32_kernel<7, 3, 1>), grid, block, 0, s, p, q, l.nblk0); break;
    case ATT_F32_W7_F16: hipLaunchKernelGGL((window_attention_f32_kernel<7, 3, 2>), grid, block, 0, s, p, q, l.nblk0); break;
    case ATT_F32_W12_9: hipLaunchKernelGGL((window_attention_f32_kernel<12, 9>), grid, block, 0, s, p, q, l.nblk0); break;
    case ATT_F32_W12_3: hipLaunchKernelGGL((window_attention_f32_kernel<12, 3>), grid, block, 0, s, p, q, l.nblk0); break;
    case ATT_SPLIT2: hipLaunchKernelGGL(window_attention_split_kernel<2>, grid, block, 0, s, p, q, ord); break;
    case ATT_SPLIT2_H: hipLaunchKernelGGL((window_attention_split_kernel<2, true>), grid, block, 0, s, p, q, ord); break;
#ifdef BRN_DIAG_BUILD
    case ATT_SPLIT1: hipLaunchKernelGGL(window_attention_split_kernel<1>, grid, block, 0, s, p, q, ord); break;
#endif
    case ATT_BF16_1: hipLaunchKernelGGL(window_attention_bf16_kernel<1>, grid, block, 0, s, p, q, ord); break;
    case ATT_BF16_2: hipLaunchKernelGGL(window_attention_bf16_kernel<2>, grid, block, 0, s, p, q, ord); break;
    case ATT_F16_1: hipLaunchKernelGGL((window_attention_bf16_kernel<1, true>), grid, block, 0, s, p, q, ord); break;
    case ATT_F16_2: hipLaunchKernelGGL((window_attention_bf16_kernel<2, true>), grid, block, 0, s, p, q, ord); break;
    default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}
hipError_t launch_window_attention(const WindowAttnParams& p, hipStream_t s) { return launch_window_attention2(p, nullptr, s); }

}  // namespace brn
