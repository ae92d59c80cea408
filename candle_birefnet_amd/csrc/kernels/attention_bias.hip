// attention_bias.hip — q/k/v attention with an additive (optionally repeating) bias for short sequences (N <= 144, head_dim 32):
//   y[b,h] = softmax_rows( scale * (q[b,h] k[b,h]^T + bias[b % n_bias, h]) ) v[b,h]
// the op candle's WindowAttention::forward hands to flash_attention_with_bias / flash_attention_with_repeating_bias (swin.rs:243, 252).
// It is the sibling of kernels/window_attention.hip for callers that bring their own q, k, v and bias: no window geometry, no
// relative-position table, no mask logic — the bias is a tensor that is read.
//
// One workgroup = one (batch entry, head); one wave = one 16-query tile, so a workgroup has ceil(N / 16) waves (1 .. 9).
// MFMA formulation, tile map and LDS images: kernels/attention_mfma.h.  What is particular here:
//   S^T[key][query] = bias^T + K . Q^T   the accumulator is LOADED from the bias tile (C operand): the bias is added before the scale, so
//                                        it costs no vector add; a lane's 4 registers are 4 consecutive keys of its query's bias row
//   softmax over keys                    exp2 with scale * log2(e) folded into one multiply; the row maximum is subtracted first
// Ragged N: N is rounded up to nt = ceil(N / 16) tiles inside the kernel.  K / V rows past N are ZEROS in LDS (never read from memory),
// their scores are forced to -3e38 after the scale so that they leave the row maximum and the row sum, a pad query computes on the
// last real row and is never stored, and every global address is clamped to the (batch entry, head) it belongs to.
// Nothing is shared between workgroups and there are no atomics: the result for a batch entry does not depend on `batch`.
#include "../brn_kernels.h"
#include "attention_mfma.h"
#include <type_traits>

namespace brn {
namespace {

constexpr int AB_HD = 32;            // head_dim
constexpr int AB_NMAX = 144;         // longest sequence: 9 tiles of 16
constexpr int AB_NT = 9;
constexpr int AB_KV_LD = 36;         // fp32 kernel: floats per LDS row of K and V
constexpr int AB_VT_LD = 148;        // 16-bit kernel: elements per LDS row of V^T

// which (batch entry, head) this workgroup owns and where its operands start
struct AbBlock {
    const float* q; const float* k; const float* v; const float* bias; float* y;   // bias: this (b % n_bias, head)'s [N][N] matrix or null
};
__device__ __forceinline__ AbBlock ab_block(const AttentionBiasParams& p) {
    const long bh = blockIdx.x;
    const long off = bh * p.N * AB_HD;
    AbBlock r;
    r.q = p.q + off; r.k = p.k + off; r.v = p.v + off; r.y = p.y + off;
    r.bias = nullptr;
    if (p.bias) {
        const int b = (int)(bh / p.heads), h = (int)(bh - (long)b * p.heads);
        r.bias = p.bias + ((long)(b % p.n_bias) * p.heads + h) * p.N * p.N;
    }
    return r;
}
// the 4 bias words of keys key0 .. key0 + 3 of one query's row (brow = that row), clamped to the row.  VEC: N % 4 == 0 and a 16-byte
// aligned tensor, so a group of 4 keys is either all real or all pad and one 16-byte load fetches it
template <bool VEC>
__device__ __forceinline__ f32x4 ab_bias4(const float* brow, int key0, int N) {
    if constexpr (VEC) return *reinterpret_cast<const f32x4*>(brow + min(key0, N - 4));
    else return f32x4{brow[min(key0, N - 1)], brow[min(key0 + 1, N - 1)], brow[min(key0 + 2, N - 1)], brow[min(key0 + 3, N - 1)]};
}
// the accumulators of S^T start as the bias tile (zeros without a bias); tiles past nt are never touched
template <bool VEC>
__device__ __forceinline__ void ab_load_bias(const float* bias, int qrow, int g, int N, int nt, f32x4 (&st)[AB_NT]) {
    const float* brow = bias ? bias + (long)qrow * N : nullptr;
#pragma unroll
    for (int kt = 0; kt < AB_NT; ++kt) {
        st[kt] = f32x4{0.f, 0.f, 0.f, 0.f};
        if (kt < nt && brow) st[kt] = ab_bias4<VEC>(brow, kt * 16 + g * 4, N);
    }
}
// scores -> un-normalised probabilities in place (exp2 units), returns the row sum.  Lane group g holds keys 16 kt + 4 g + r.
__device__ __forceinline__ float ab_softmax(f32x4 (&st)[AB_NT], int g, int N, int nt, float scale) {
    const float sc2 = scale * ATT_LOG2E;
    const int nlast = N - (nt - 1) * 16;            // real keys of the last tile: 1 .. 16
    float mx = ATT_NEG;
#pragma unroll
    for (int kt = 0; kt < AB_NT; ++kt) {
        if (kt < nt) {
            att_scale4(st[kt], sc2);
            // pad keys leave the softmax (att_exclude4(st[kt], g * 4, nlast), spelled out: through the helper the whole row loop compiled
            // to other code, with up to 6 VGPRs more)
            if (kt == nt - 1) {
#pragma unroll
                for (int r = 0; r < 4; ++r) st[kt][r] = (g * 4 + r < nlast) ? st[kt][r] : ATT_NEG;
            }
            mx = att_max4(mx, st[kt]);
        }
    }
    mx = att_group_max(mx);
    float sum = 0.f;
#pragma unroll
    for (int kt = 0; kt < AB_NT; ++kt) {
        if (kt < nt) att_exp2_sum4(st[kt], mx, sum);
    }
    return att_group_sum(sum);
}
// the two d tiles of a query's row of y
__device__ __forceinline__ void ab_store(float* y, int query, int g, const f32x4 o0, const f32x4 o1, const float inv) {
    float* yg = y + (long)query * AB_HD + g * 4;
    att_store_o(yg, 0, o0, inv);
    att_store_o(yg, 1, o1, inv);
}

// ---- fp32: v_mfma_f32_16x16x4_f32, an exact fmaf chain per score and per output ----
// LDS: Ks, Vs [144][36] floats = 41.5 KB.  Registers per wave: 36 score accumulators + 8 q + 8 k + 8 o.
template <bool BVEC>
__global__ void __launch_bounds__(AB_NT * 64) attention_bias_f32_kernel(const AttentionBiasParams p) {
    __shared__ __attribute__((aligned(16))) float Ks[AB_NMAX * AB_KV_LD];
    __shared__ __attribute__((aligned(16))) float Vs[AB_NMAX * AB_KV_LD];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, nthr = blockDim.x;
    const int li = lane & 15, g = lane >> 4;
    const int N = p.N, nt = (N + 15) >> 4;
    const AbBlock blk = ab_block(p);

    // the wave's own loads go out first: its Q fragment (d = 8g .. 8g+7 of query row qrow) and its bias tiles
    const int query = wave * 16 + li, qrow = min(query, N - 1);
    const float* qp = blk.q + (long)qrow * AB_HD + g * 8;
    const f32x4 q0 = *reinterpret_cast<const f32x4*>(qp), q1 = *reinterpret_cast<const f32x4*>(qp + 4);
    f32x4 st[AB_NT];
    ab_load_bias<BVEC>(blk.bias, qrow, g, N, nt, st);

    // ---- stage K and V of this (batch entry, head): nt * 16 rows x 8 float4, zeros past N ----
    for (int idx = tid; idx < nt * 16 * 8; idx += nthr) {
        const int t = idx >> 3, c4 = (idx & 7) * 4;
        const long src = (long)min(t, N - 1) * AB_HD + c4;
        f32x4 kv = *reinterpret_cast<const f32x4*>(blk.k + src), vv = *reinterpret_cast<const f32x4*>(blk.v + src);
        if (t >= N) { kv = f32x4{0.f, 0.f, 0.f, 0.f}; vv = kv; }
        *reinterpret_cast<f32x4*>(Ks + t * AB_KV_LD + c4) = kv;
        *reinterpret_cast<f32x4*>(Vs + t * AB_KV_LD + c4) = vv;
    }
    __syncthreads();
    if (wave >= nt) return;

    // S^T = bias^T + K . Q^T
#pragma unroll
    for (int kt = 0; kt < AB_NT; ++kt) {
        if (kt < nt) st[kt] = att_score_f32(Ks + (kt * 16 + li) * AB_KV_LD + g * 8, q0, q1, st[kt]);
        if (kt % 3 == 2) __builtin_amdgcn_sched_barrier(0);   // bound the scheduler's hoisting (register pressure)
    }
    const float sum = ab_softmax(st, g, N, nt, p.scale);
    // O^T = V^T . P^T : two d tiles
    f32x4 o0 = {0.f, 0.f, 0.f, 0.f}, o1 = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int kt = 0; kt < AB_NT; ++kt) {
        if (kt < nt) {
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const float* vp = Vs + (kt * 16 + g * 4 + r) * AB_KV_LD + li;
                o0 = att_pv_f32(vp, 0, st[kt][r], o0);
                o1 = att_pv_f32(vp, 1, st[kt][r], o1);
            }
        }
        if (kt % 2 == 1) __builtin_amdgcn_sched_barrier(0);
    }
    if (query < N) ab_store(blk.y, query, g, o0, o1, 1.0f / sum);
}

// ---- 16-bit: q, k, v rounded to E (round to nearest even) as they are loaded; v_mfma_f32_16x16x32_{bf16,f16} with fp32 accumulation.
// The bias, the scores, the row maximum and the row sum (of the UNROUNDED probabilities) are fp32; the probabilities are rounded to E for
// P . V.  LDS: Kp[key][32 d] and Vt[d][148 keys] (kernels/attention_mfma.h) = 18.2 KB.  Both images are zero-filled up to the even tile
// count, so a tile past nt contributes 0 x 0. ----
template <typename E, bool BVEC>
__global__ void __launch_bounds__(AB_NT * 64) attention_bias_s16_kernel(const AttentionBiasParams p) {
    constexpr bool F16 = std::is_same<E, _Float16>::value;
    typedef vec8<E> ex8;
    typedef vec4<E> ex4;
    __shared__ __attribute__((aligned(16))) E Kp[AB_NMAX * AB_HD];
    __shared__ __attribute__((aligned(16))) E Vt[AB_HD * AB_VT_LD];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, nthr = blockDim.x;
    const int li = lane & 15, g = lane >> 4;
    const int N = p.N, nt = (N + 15) >> 4;
    const AbBlock blk = ab_block(p);

    const int query = wave * 16 + li, qrow = min(query, N - 1);
    const float* qp = blk.q + (long)qrow * AB_HD + g * 8;
    const f32x4 q0 = *reinterpret_cast<const f32x4*>(qp), q1 = *reinterpret_cast<const f32x4*>(qp + 4);
    f32x4 st[AB_NT];
    ab_load_bias<BVEC>(blk.bias, qrow, g, N, nt, st);

    // ---- stage: item = (key pair tp, 4-wide d chunk); key tiles up to the even count (at most 9), zeros past N ----
    const int ktiles = min(AB_NT, (nt + 1) & ~1);
    for (int idx = tid; idx < ktiles * 8 * 8; idx += nthr) {
        const int tp = idx >> 3, c4 = (idx & 7) * 4;
        f32x4 kv[2], vv[2];
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            const int t = tp * 2 + u;
            const long src = (long)min(t, N - 1) * AB_HD + c4;
            kv[u] = *reinterpret_cast<const f32x4*>(blk.k + src);
            vv[u] = *reinterpret_cast<const f32x4*>(blk.v + src);
            if (t >= N) { kv[u] = f32x4{0.f, 0.f, 0.f, 0.f}; vv[u] = kv[u]; }
        }
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            const int t = tp * 2 + u;
            ex4 h;
#pragma unroll
            for (int e = 0; e < 4; ++e) h[e] = (E)kv[u][e];
            *reinterpret_cast<ex4*>(att_k_chunk<AB_HD>(Kp + t * AB_HD, t, c4 >> 3) + (c4 & 4)) = h;
        }
#pragma unroll
        for (int e = 0; e < 4; ++e) att_vt_store(Vt + (c4 + e) * AB_VT_LD, tp, (E)vv[0][e], (E)vv[1][e]);
    }
    __syncthreads();
    if (wave >= nt) return;

    const ex8 qf = att_round8<E>(q0, q1);
    // S^T = bias^T + K . Q^T: head_dim 32 is ONE MFMA k
#pragma unroll
    for (int kt = 0; kt < AB_NT; ++kt) {
        if (kt < nt) {
            const int key = kt * 16 + li;
            st[kt] = att_mfma<F16>(att_k_frag<AB_HD>(Kp + key * AB_HD, key, g), qf, st[kt]);
        }
    }
    const float sum = ab_softmax(st, g, N, nt, p.scale);
    // O^T = V^T . P^T: k-step t = key tiles (2t, 2t+1); the 10th tile does not exist
    f32x4 o0 = {0.f, 0.f, 0.f, 0.f}, o1 = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int t = 0; t < 5; ++t) {
        if (2 * t < nt) {
            const bool hi_tile = 2 * t + 1 < AB_NT;                  // compile-time per t after unrolling
            const bool hi_real = 2 * t + 1 < nt;
            // (att_p_step and att_round8 with a run-time tile count, spelled out: through a helper the tile tests compile to other scalar code)
            ex8 pf;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                pf[e] = (E)st[2 * t][e];
                pf[4 + e] = (E)((hi_tile && hi_real) ? st[hi_tile ? 2 * t + 1 : 0][e] : 0.f);
            }
#pragma unroll
            for (int dt = 0; dt < 2; ++dt) {
                const ex8 vf = att_vt_frag(Vt + (dt * 16 + li) * AB_VT_LD + g * 4, t, hi_tile);
                if (dt == 0) o0 = att_mfma<F16>(vf, pf, o0);
                else o1 = att_mfma<F16>(vf, pf, o1);
            }
        }
    }
    if (query < N) ab_store(blk.y, query, g, o0, o1, 1.0f / sum);
}

}  // namespace

hipError_t launch_attention_bias(const AttentionBiasParams& p, hipStream_t s) {
    if (p.N < 1 || p.N > AB_NMAX || p.batch < 1 || p.heads < 1 || (long)p.batch * p.heads > 0x7fffffffL || (p.bias && (p.n_bias < 1 || p.batch % p.n_bias)))
        return hipErrorInvalidValue;
    const int nt = (p.N + 15) / 16;
    const bool bvec = p.bias && p.N % 4 == 0 && (reinterpret_cast<uintptr_t>(p.bias) & 15) == 0;
    const dim3 grid((unsigned)((long)p.batch * p.heads)), block(nt * 64);
    if (p.s16 == 0) {
        if (bvec) hipLaunchKernelGGL(attention_bias_f32_kernel<true>, grid, block, 0, s, p);
        else hipLaunchKernelGGL(attention_bias_f32_kernel<false>, grid, block, 0, s, p);
    } else if (p.s16 == 1) {
        if (bvec) hipLaunchKernelGGL((attention_bias_s16_kernel<__bf16, true>), grid, block, 0, s, p);
        else hipLaunchKernelGGL((attention_bias_s16_kernel<__bf16, false>), grid, block, 0, s, p);
    } else if (p.s16 == 2) {
        if (bvec) hipLaunchKernelGGL((attention_bias_s16_kernel<_Float16, true>), grid, block, 0, s, p);
        else hipLaunchKernelGGL((attention_bias_s16_kernel<_Float16, false>), grid, block, 0, s, p);
    } else return hipErrorInvalidValue;
    return hipGetLastError();
}

}  // namespace brn
