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
#include "../brn_kernels.h"
#include "attention_mfma.h"
#include <type_traits>

namespace brn {
namespace {

constexpr int FA_BQ = 64;            // queries per workgroup: 4 waves x 16
constexpr int FA_T = 64;             // keys per K / V tile
constexpr int FA_THREADS = 256;
constexpr int FA_VT_LD = 72;         // 16-bit kernel: elements per LDS row of V^T (36 dwords: conflict-free 8-byte reads, 2-way 4-byte writes)

// which (batch entry, head, query tile) this workgroup owns, where its operands start and how many K / V tiles it walks
struct FaBlock {
    const float* q; const float* k; const float* v; float* y;
    const float* bias;    // BIAS: the [seq_q, seq_kv] slab of this (bias pattern = batch entry % n_bias, head)
    int q0;               // first query of the tile
    int nkt;              // K / V tiles to walk: all of them, or (causal) those that reach the tile's last query
};
template <bool BIAS>
__device__ __forceinline__ FaBlock fa_block(const FlashAttentionParams& p) {
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
    return r;
}

// The bias values a lane adds to its scores of the K / V tile at key0: for sub-tile s the 4 consecutive floats of keys
// key0 + 16 s + 4 g + 0..3 in row `row` (= the lane's clamped query * seq_kv, 64-bit) of the slab.  Every address stays inside the slab:
// seq_kv % 4 == 0 -> one 16-byte load per sub-tile, its first key clamped to seq_kv - 4 (the slab base is 16-byte aligned and row and
// key are multiples of 4, so the address is; a group of 4 is then wholly real or wholly past seq_kv); otherwise 4-byte loads with each
// key clamped to seq_kv - 1.  The choice is a function of seq_kv alone (wave-uniform).  What a clamped load returns belongs to an
// excluded key and is replaced before the maximum.  No address depends on a bias value.
// A/B switch (make EXTRA_CXXFLAGS=-DFA_BIAS_NONTEMPORAL=1): the 16-byte bias loads as non-temporal loads.  Every bias element is read once by
// one lane, so it has nothing to gain from the caches; DESIGN.md 3.2d has what the two builds measured.
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
__device__ __forceinline__ float fa_softmax_tile(f32x4 (&st)[FA_T / 16], float sc2, bool mask, int key0, int g, int limit, float& m, float& l) {
    float mx = ATT_NEG;
#pragma unroll
    for (int s = 0; s < FA_T / 16; ++s) {
        att_scale4(st[s], sc2);
        if (mask) att_exclude4(st[s], key0 + s * 16 + g * 4, limit);
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

// ---- fp32: v_mfma_f32_16x16x4_f32, an exact fmaf chain per score and per output ----
// LDS: Ks, Vs [64][D + 4] floats (D 128: 66 KB).  Staging item = (key, 4-wide d chunk), D / 16 items of K and of V per thread.
template <int D, bool BIAS>
__global__ void __launch_bounds__(FA_THREADS) flash_attention_f32_kernel(const FlashAttentionParams p) {
    constexpr int LD = D + 4, NI = D / 16, ND = D / 16, NC = D / 32;
    __shared__ __attribute__((aligned(16))) float Ks[FA_T * LD];
    __shared__ __attribute__((aligned(16))) float Vs[FA_T * LD];
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int li = lane & 15, g = lane >> 4;
    const FaBlock blk = fa_block<BIAS>(p);

    const int query = blk.q0 + wave * 16 + li, qrow = min(query, p.seq_q - 1);
    const int wave_row0 = min(blk.q0 + wave * 16, p.seq_q - 1);
    const int limit = p.causal ? min(p.seq_kv, qrow + 1) : p.seq_kv;
    const long brow = (long)qrow * p.seq_kv;       // BIAS: the query's row of the bias slab
    // Q fragment: chunk c of 32 d's -> d = 32 c + 8 g .. + 7 of the query's row (the MFMA k order is a permutation of d; K uses the same)
    f32x4 qv[2 * NC];
    {
        const float* qp = blk.q + qrow * p.q_ss + g * 8;
#pragma unroll
        for (int c = 0; c < NC; ++c) {
            qv[2 * c] = *reinterpret_cast<const f32x4*>(qp + c * 32);
            qv[2 * c + 1] = *reinterpret_cast<const f32x4*>(qp + c * 32 + 4);
        }
    }
    f32x4 kr[NI], vr[NI];
    f32x4 bn[FA_T / 16];                                   // BIAS: the bias of the tile in kr / vr, loaded with it
    auto load_tile = [&](int key0) {
#pragma unroll
        for (int i = 0; i < NI; ++i) {
            const int idx = tid + i * FA_THREADS, t = key0 + idx / (D / 4), c4 = (idx % (D / 4)) * 4;
            const long src = min(t, p.seq_kv - 1) * p.kv_ss + c4;
            kr[i] = *reinterpret_cast<const f32x4*>(blk.k + src);
            vr[i] = *reinterpret_cast<const f32x4*>(blk.v + src);
            if (t >= p.seq_kv) { kr[i] = f32x4{0.f, 0.f, 0.f, 0.f}; vr[i] = kr[i]; }
        }
        if constexpr (BIAS) fa_load_bias(bn, blk.bias, brow, key0, g, p.seq_kv);
    };
    f32x4 o[ND];
#pragma unroll
    for (int dt = 0; dt < ND; ++dt) o[dt] = f32x4{0.f, 0.f, 0.f, 0.f};
    float m = ATT_NEG, l = 0.f;
    const float sc2 = p.scale * ATT_LOG2E;

    load_tile(0);
    for (int kt = 0; kt < blk.nkt; ++kt) {
        __syncthreads();                                   // every wave is done reading the previous tile
#pragma unroll
        for (int i = 0; i < NI; ++i) {
            const int idx = tid + i * FA_THREADS, t = idx / (D / 4), c4 = (idx % (D / 4)) * 4;
            *reinterpret_cast<f32x4*>(Ks + t * LD + c4) = kr[i];
            *reinterpret_cast<f32x4*>(Vs + t * LD + c4) = vr[i];
        }
        __syncthreads();
        // S^T = K . Q^T (BIAS: + bias, as the initial accumulator: it joins the unscaled scores, and an all-zero bias gives the bias-free bits)
        f32x4 st[FA_T / 16];
        if constexpr (BIAS) {
#pragma unroll
            for (int s = 0; s < FA_T / 16; ++s) st[s] = bn[s];
        }
        if (kt + 1 < blk.nkt) load_tile((kt + 1) * FA_T);
#pragma unroll
        for (int s = 0; s < FA_T / 16; ++s) {
            f32x4 acc = {0.f, 0.f, 0.f, 0.f};
            if constexpr (BIAS) acc = st[s];
#pragma unroll
            for (int c = 0; c < NC; ++c) acc = att_score_f32(Ks + (s * 16 + li) * LD + c * 32 + g * 8, qv[2 * c], qv[2 * c + 1], acc);
            st[s] = acc;
        }
        const float alpha = fa_softmax_tile(st, sc2, fa_tile_masks(p, kt * FA_T, wave_row0), kt * FA_T, g, limit, m, l);
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
    fa_finish<ND, BIAS>(query < p.seq_q ? blk.y + query * p.q_ss : nullptr, g, o, l, m);
}

// ---- 16-bit: q, k, v rounded to E (round to nearest even) as they are loaded; v_mfma_f32_16x16x32_{bf16,f16} with fp32 accumulation.
// Scores, m, l (of the UNROUNDED numerators) and O are fp32; the numerators are rounded to E for P . V.
// LDS: Kp[key][D] and Vt[d][72 keys] (kernels/attention_mfma.h): D 128 = 16 + 18 KB.
// Staging item = (key pair, 4-wide d chunk): thread -> (d chunk low 2 bits, key pair, d chunk high bits), so a quad of lanes reads 64
// contiguous bytes of a row and the 4-byte transposed V writes of a wave fall 2-way on the 32 banks. ----
template <typename E, int D, bool BIAS>
__global__ void __launch_bounds__(FA_THREADS) flash_attention_s16_kernel(const FlashAttentionParams p) {
    constexpr bool F16 = std::is_same<E, _Float16>::value;
    constexpr int NP = D / 32, ND = D / 16;       // staging passes = MFMA k steps of a score tile; d tiles of O^T
    typedef vec8<E> ex8;
    typedef vec4<E> ex4;
    __shared__ __attribute__((aligned(16))) E Kp[FA_T * D];
    __shared__ __attribute__((aligned(16))) E Vt[D * FA_VT_LD];
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int li = lane & 15, g = lane >> 4;
    const FaBlock blk = fa_block<BIAS>(p);

    const int query = blk.q0 + wave * 16 + li, qrow = min(query, p.seq_q - 1);
    const int wave_row0 = min(blk.q0 + wave * 16, p.seq_q - 1);
    const int limit = p.causal ? min(p.seq_kv, qrow + 1) : p.seq_kv;
    const long brow = (long)qrow * p.seq_kv;       // BIAS: the query's row of the bias slab
    // Q fragment of MFMA k step c: d = 32 c + 8 g .. + 7 of the query's row
    ex8 qf[NP];
    {
        const float* qp = blk.q + qrow * p.q_ss + g * 8;
#pragma unroll
        for (int c = 0; c < NP; ++c) qf[c] = att_round8<E>(*reinterpret_cast<const f32x4*>(qp + c * 32), *reinterpret_cast<const f32x4*>(qp + c * 32 + 4));
    }
    // staging: keys (2 tp, 2 tp + 1) of the tile, d = c4 .. c4 + 3 with c4 = 16 (hi + 2 pass) + 4 lo
    const int s_lo = tid & 3, s_tp = (tid >> 2) & 31, s_hi = tid >> 7;
    f32x4 kr[NP][2], vr[NP][2];
    f32x4 bn[FA_T / 16];                                   // BIAS: the bias of the tile in kr / vr, loaded with it
    auto load_tile = [&](int key0) {
#pragma unroll
        for (int ps = 0; ps < NP; ++ps) {
            const int c4 = (s_hi + 2 * ps) * 16 + s_lo * 4;
#pragma unroll
            for (int u = 0; u < 2; ++u) {
                const int t = key0 + s_tp * 2 + u;
                const long src = min(t, p.seq_kv - 1) * p.kv_ss + c4;
                kr[ps][u] = *reinterpret_cast<const f32x4*>(blk.k + src);
                vr[ps][u] = *reinterpret_cast<const f32x4*>(blk.v + src);
                if (t >= p.seq_kv) { kr[ps][u] = f32x4{0.f, 0.f, 0.f, 0.f}; vr[ps][u] = kr[ps][u]; }
            }
        }
        if constexpr (BIAS) fa_load_bias(bn, blk.bias, brow, key0, g, p.seq_kv);
    };
    f32x4 o[ND];
#pragma unroll
    for (int dt = 0; dt < ND; ++dt) o[dt] = f32x4{0.f, 0.f, 0.f, 0.f};
    float m = ATT_NEG, l = 0.f;
    const float sc2 = p.scale * ATT_LOG2E;

    load_tile(0);
    for (int kt = 0; kt < blk.nkt; ++kt) {
        __syncthreads();                                   // every wave is done reading the previous tile
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
        __syncthreads();
        // S^T = K . Q^T (BIAS: + bias, as the initial accumulator: it joins the unscaled scores, and an all-zero bias gives the bias-free bits)
        f32x4 st[FA_T / 16];
        if constexpr (BIAS) {
#pragma unroll
            for (int s = 0; s < FA_T / 16; ++s) st[s] = bn[s];
        }
        if (kt + 1 < blk.nkt) load_tile((kt + 1) * FA_T);
#pragma unroll
        for (int s = 0; s < FA_T / 16; ++s) {
            const int key = s * 16 + li;
            f32x4 acc = {0.f, 0.f, 0.f, 0.f};
            if constexpr (BIAS) acc = st[s];
#pragma unroll
            for (int c = 0; c < NP; ++c) acc = att_mfma<F16>(att_k_frag<D>(Kp + key * D, key, c * 4 + g), qf[c], acc);
            st[s] = acc;
        }
        const float alpha = fa_softmax_tile(st, sc2, fa_tile_masks(p, kt * FA_T, wave_row0), kt * FA_T, g, limit, m, l);
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
    fa_finish<ND, BIAS>(query < p.seq_q ? blk.y + query * p.q_ss : nullptr, g, o, l, m);
}

template <int D, bool BIAS>
void fa_launch(const FlashAttentionParams& p, dim3 grid, hipStream_t s) {
    const dim3 block(FA_THREADS);
    if (p.s16 == 0) hipLaunchKernelGGL((flash_attention_f32_kernel<D, BIAS>), grid, block, 0, s, p);
    else if (p.s16 == 1) hipLaunchKernelGGL((flash_attention_s16_kernel<__bf16, D, BIAS>), grid, block, 0, s, p);
    else hipLaunchKernelGGL((flash_attention_s16_kernel<_Float16, D, BIAS>), grid, block, 0, s, p);
}
template <int D>
void fa_launch(const FlashAttentionParams& p, dim3 grid, hipStream_t s) {
    if (p.bias) fa_launch<D, true>(p, grid, s);
    else fa_launch<D, false>(p, grid, s);
}

}  // namespace

hipError_t launch_flash_attention(const FlashAttentionParams& p, hipStream_t s) {
    if (!(p.head_dim == 32 || p.head_dim == 64 || p.head_dim == 128) || p.seq_q < 1 || p.seq_kv < 1 || p.seq_q > 65536 || p.seq_kv > 65536 ||
        p.batch < 1 || p.heads < 1 || (p.causal && p.seq_q != p.seq_kv) || p.s16 < 0 || p.s16 > 2 || !(p.scale > 0.f) ||
        p.n_bias < 0 || (p.bias == nullptr) != (p.n_bias == 0) || (p.n_bias > 0 && p.batch % p.n_bias))
        return hipErrorInvalidValue;
    const long nwg = (long)p.batch * p.heads * ((p.seq_q + FA_BQ - 1) / FA_BQ);
    if (nwg > 0x7fffffffL) return hipErrorInvalidValue;
    const dim3 grid((unsigned)nwg);
    if (p.head_dim == 32) fa_launch<32>(p, grid, s);
    else if (p.head_dim == 64) fa_launch<64>(p, grid, s);
    else fa_launch<128>(p, grid, s);
    return hipGetLastError();
}

}  // namespace brn
