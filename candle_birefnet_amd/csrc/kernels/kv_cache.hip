// kv_cache.hip — brn_kv_cache_append: seq_new fp32 tokens per sequence go into the pages of a K / V pool (the pool of
// brn_flash_attention_paged_forward / brn_flash_attention_paged_kv_forward: [n_pages, page_size, kv_heads, head_dim] in fp32, bf16 or fp16),
// behind the keys each sequence already has, and the lengths move on.  Table and lengths are device data, as in the attention kernels.
//
// With L_b = min(max(kv_lens[b], 0), cap), cap = max_pages * page_size (< 2^31), token t of batch entry b is key pos = L_b + t of
// sequence b: row pos % page_size of page min(max(block_table[b][pos / page_size], 0), n_pages - 1).  A token with pos >= cap is dropped:
// its thread returns before it reads a table entry or forms an address.  No address depends on a device value except through these
// clamps: pos < cap bounds the table index by max_pages - 1 (clamped again where it is formed), the page clamp bounds the pool offset.
//
// kv_append_rows_kernel<KV>: bandwidth only.  One thread = 8 consecutive d of one (b, t, K / V head) row of K and of V: two 16-byte loads
// of k_new and of v_new, the cast (KV)x of the attention kernels (round to nearest even; fp16 overflow becomes +-inf, NaN stays NaN), one
// 16-byte store each (two for an fp32 pool).  Threads run d-fastest, then head, then token: a wave reads and writes whole rows.  Offsets
// are 64-bit, in elements.  kv_append_lens_kernel: one workgroup writes kv_lens_out[b] = min(L_b + seq_new, cap); it is launched AFTER the
// rows on the same stream, so kv_lens_out may be kv_lens itself.
//
// KV = kv_e4m3 (brn_kv_cache_append_fp8): the pool holds OCP e4m3fn bytes with one fp32 scale per K / V head (device data, null = 1).
// An element is stored in three steps: t = x / scale[h], the correctly rounded fp32 division; t clamped to +-448 by two compares and
// selects in plain C++, which keep a NaN; t rounded to nearest even by v_cvt_pk_fp8_f32.  Saturation is the clamp's, so it does not
// depend on what the instruction does on overflow; +-0 and underflow keep their sign; a NaN becomes a NaN byte.  The thread map is the
// same: 8 d per thread, one 8-byte store of K and of V.  No address depends on a scale.
//
// brn_rope_forward (rope_kernel) and the rope instantiation kv_append_rows_kernel<KV, true> (brn_kv_cache_append_rope / _rope_fp8) rotate
// pairs of a row by the caller's cos / sin table; RopeParams in brn_kernels.h states the rule.  The table row is min(position, n_pos - 1),
// the position device data, clamped like the lengths; the rotation is two rounded products and one rounded sum, never an fma (rope_pair).
//
// VARLEN (brn_kv_cache_append_varlen): the new tokens are a packed batch [total_q, kv_heads, head_dim] with cu_seqlens_q on the device.
// paged_varlen_plan_kernel (one workgroup, launched first; also the plan of brn_flash_attention_paged_varlen_forward) applies the rule of
// brn_flash_paged_varlen_plan.h: the clamped running maximum s_b, and the prefix of row tiles the attention kernels use.  The rows kernel
// keeps its thread map with the token in the place of (b, t): a token outside [s_0, s_n) is padding and returns; otherwise its sequence
// is the b with s_b <= token < s_{b+1}, found by bisection of the monotone starts, t = token - s_b, and everything from pos on is the
// plain append's.  kv_append_lens_varlen_kernel writes min(L_b + n_b, cap) afterwards.  DESIGN.md 3.2m.
#include "../brn_kernels.h"
#include "../brn_flash_paged_varlen_plan.h"
#include "attention_mfma.h"
#include <type_traits>

namespace brn {
namespace {

constexpr int KV_THREADS = 256;

template <typename KV>
__device__ __forceinline__ void kv_store8(KV* dst, const f32x4 a, const f32x4 b) {
    if constexpr (std::is_same<KV, float>::value) {
        *reinterpret_cast<f32x4*>(dst) = a;
        *reinterpret_cast<f32x4*>(dst + 4) = b;
    } else *reinterpret_cast<vec8<KV>*>(dst) = att_round8<KV>(a, b);
}

typedef unsigned char kv_e4m3;
__device__ __forceinline__ float kv_fp8_scaled(float x, float scale) {
    float t = x / scale;
    t = t > 448.f ? 448.f : t;             // (a NaN fails both compares and stays)
    t = t < -448.f ? -448.f : t;
    return t;
}
__device__ __forceinline__ void kv_store8_fp8(kv_e4m3* dst, const f32x4 a, const f32x4 b, float scale) {
    int lo = 0, hi = 0;
    lo = __builtin_amdgcn_cvt_pk_fp8_f32(kv_fp8_scaled(a[0], scale), kv_fp8_scaled(a[1], scale), lo, false);
    lo = __builtin_amdgcn_cvt_pk_fp8_f32(kv_fp8_scaled(a[2], scale), kv_fp8_scaled(a[3], scale), lo, true);
    hi = __builtin_amdgcn_cvt_pk_fp8_f32(kv_fp8_scaled(b[0], scale), kv_fp8_scaled(b[1], scale), hi, false);
    hi = __builtin_amdgcn_cvt_pk_fp8_f32(kv_fp8_scaled(b[2], scale), kv_fp8_scaled(b[3], scale), hi, true);
    *reinterpret_cast<vec2<int>*>(dst) = vec2<int>{lo, hi};
}

template <typename KV>
__device__ __forceinline__ void kv_put8(void* pages, long dst, const f32x4 a, const f32x4 b, const float* scale, int h) {
    if constexpr (std::is_same<KV, kv_e4m3>::value) kv_store8_fp8(static_cast<KV*>(pages) + dst, a, b, scale ? scale[h] : 1.f);
    else kv_store8(static_cast<KV*>(pages) + dst, a, b);
}

__device__ __forceinline__ f32x4 ld4(const float* p) { return *reinterpret_cast<const f32x4*>(p); }

// ---- the rotation (RopeParams in brn_kernels.h states the rule) ----
// one pair: two rounded products, then one rounded difference / sum (the rule is promised bit for bit).  The pragma keeps the four
// products out of an fma under hipcc's default -ffp-contract=fast-honor-pragmas and under on / off, which is every way the Makefile
// builds this file; an explicit -ffp-contract=fast would let the backend fuse in spite of it and must not be given to this file
__device__ __forceinline__ void rope_pair(float a, float b, float c, float s, float& ra, float& rb) {
#pragma clang fp contract(off)
    const float ac = a * c, bs = b * s, bc = b * c, as = a * s;
    ra = ac - bs;
    rb = bc + as;
}
// HALF: lo = x[8c .. 8c + 8), hi = x[8c + rot_dim / 2 ..), cs / sn = the table row's [8c .. 8c + 8)
__device__ __forceinline__ void rope_half8(f32x4& lo0, f32x4& lo1, f32x4& hi0, f32x4& hi1, const float* cs, const float* sn) {
    const f32x4 c0 = ld4(cs), c1 = ld4(cs + 4), s0 = ld4(sn), s1 = ld4(sn + 4);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        float a, b;
        rope_pair(lo0[j], hi0[j], c0[j], s0[j], a, b); lo0[j] = a; hi0[j] = b;
        rope_pair(lo1[j], hi1[j], c1[j], s1[j], a, b); lo1[j] = a; hi1[j] = b;
    }
}
// INTERLEAVED: x0, x1 = x[8c .. 8c + 8), cs / sn = the table row's [4c .. 4c + 4)
__device__ __forceinline__ void rope_inter8(f32x4& x0, f32x4& x1, const float* cs, const float* sn) {
    const f32x4 c = ld4(cs), s = ld4(sn);
    float a, b;
    rope_pair(x0[0], x0[1], c[0], s[0], a, b); x0[0] = a; x0[1] = b;
    rope_pair(x0[2], x0[3], c[1], s[1], a, b); x0[2] = a; x0[3] = b;
    rope_pair(x1[0], x1[1], c[2], s[2], a, b); x1[0] = a; x1[1] = b;
    rope_pair(x1[2], x1[3], c[3], s[3], a, b); x1[2] = a; x1[3] = b;
}

// ROPE (brn_kv_cache_append_rope / _rope_fp8): K is rotated at table row min(pos, rope_n_pos - 1) before the store; V and everything
// else is the plain append's.  The thread map stays one thread per 8 d of a row; for K in HALF style the thread of chunk c < rope_dim / 16
// also takes chunk c + rope_dim / 16 (both members of its pairs), the threads of those upper chunks touch V alone.  Every element of
// k_new is still read once and every pool element written once
template <typename KV, bool ROPE>
__global__ void __launch_bounds__(KV_THREADS) kv_append_rows_kernel(const KvAppendParams p) {
    const int C8 = p.head_dim >> 3;
    const long idx = (long)blockIdx.x * KV_THREADS + threadIdx.x;
    const long per_b = (long)p.seq_new * p.kv_heads * C8;
    if (idx >= per_b * p.batch) return;
    const int b = (int)(idx / per_b);
    const int r = (int)(idx - b * per_b);                          // < 65536 * kv_heads * 16 (launch_kv_cache_append: < 2^31)
    const int t = r / (p.kv_heads * C8), hc = r - t * (p.kv_heads * C8);
    const int h = hc / C8, c8 = (hc - h * C8) * 8;
    const long pos = (long)min(max(p.kv_lens[b], 0), p.cap) + t;
    if (pos >= p.cap) return;                                      // dropped: nothing read from the table, nothing written
    const int slot = min((int)(pos >> p.page_log2), p.max_pages - 1);
    const int page = min(max(p.block_table[(long)b * p.max_pages + slot], 0), p.n_pages - 1);
    const long dst = (long)page * p.page_stride + (pos & ((1 << p.page_log2) - 1)) * p.kv_ss + h * p.head_dim + c8;
    const long src = b * p.new_sb + t * p.new_ss + h * p.new_sh + c8;
    if constexpr (ROPE) {
        const int half = p.rope_dim >> 1;
        const float* cs = p.rope_cos + (long)min(pos, (long)p.rope_n_pos - 1) * half;
        const float* sn = p.rope_sin + (cs - p.rope_cos);
        if (p.rope_style == 0) {
            if (c8 < half) {
                f32x4 lo0 = ld4(p.k_new + src), lo1 = ld4(p.k_new + src + 4), hi0 = ld4(p.k_new + src + half), hi1 = ld4(p.k_new + src + half + 4);
                rope_half8(lo0, lo1, hi0, hi1, cs + c8, sn + c8);
                kv_put8<KV>(p.k_pages, dst, lo0, lo1, p.k_scale, h);
                kv_put8<KV>(p.k_pages, dst + half, hi0, hi1, p.k_scale, h);
            } else if (c8 >= p.rope_dim) kv_put8<KV>(p.k_pages, dst, ld4(p.k_new + src), ld4(p.k_new + src + 4), p.k_scale, h);
        } else {
            f32x4 k0 = ld4(p.k_new + src), k1 = ld4(p.k_new + src + 4);
            if (c8 < p.rope_dim) rope_inter8(k0, k1, cs + (c8 >> 1), sn + (c8 >> 1));
            kv_put8<KV>(p.k_pages, dst, k0, k1, p.k_scale, h);
        }
        kv_put8<KV>(p.v_pages, dst, ld4(p.v_new + src), ld4(p.v_new + src + 4), p.v_scale, h);
    } else {
        const f32x4 k0 = ld4(p.k_new + src), k1 = ld4(p.k_new + src + 4);
        const f32x4 v0 = ld4(p.v_new + src), v1 = ld4(p.v_new + src + 4);
        kv_put8<KV>(p.k_pages, dst, k0, k1, p.k_scale, h);
        kv_put8<KV>(p.v_pages, dst, v0, v1, p.v_scale, h);
    }
}

// the sequence of a packed token: the b in 0 .. n - 1 with starts[b] <= token < starts[b + 1] (starts non-decreasing, starts[0] <= token <
// starts[n] checked by the caller); empty sequences (equal starts) are stepped over
__device__ __forceinline__ int pv_sequence_of(const int* starts, int n, int token) {
    int lo = 0, hi = n;
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (starts[mid] <= token) lo = mid; else hi = mid;
    }
    return lo;
}
// VARLEN (brn_kv_cache_append_varlen): the plain append's thread map with the packed token in the place of (b, t); from pos on, its rule
template <typename KV>
__global__ void __launch_bounds__(KV_THREADS) kv_append_rows_varlen_kernel(const KvAppendParams p) {
    const int C8 = p.head_dim >> 3;
    const long idx = (long)blockIdx.x * KV_THREADS + threadIdx.x;
    const long per_t = (long)p.kv_heads * C8;
    if (idx >= per_t * p.pv_total_q) return;
    const int token = (int)(idx / per_t), hc = (int)(idx - token * per_t);
    const int h = hc / C8, c8 = (hc - h * C8) * 8;
    const int* starts = p.pv_plan + fa_pv_starts_at();
    if (token < starts[0] || token >= starts[p.pv_n_seqs]) return;     // padding: nothing read from the table, nothing written
    const int b = pv_sequence_of(starts, p.pv_n_seqs, token);
    const int t = token - min(max(starts[b], 0), token);               // (starts[b] <= token here; the clamp keeps t >= 0 whatever the plan holds)
    const long pos = (long)min(max(p.kv_lens[b], 0), p.cap) + t;
    if (pos >= p.cap) return;                                          // dropped: nothing read from the table, nothing written
    const int slot = min((int)(pos >> p.page_log2), p.max_pages - 1);
    const int page = min(max(p.block_table[(long)b * p.max_pages + slot], 0), p.n_pages - 1);
    const long dst = (long)page * p.page_stride + (pos & ((1 << p.page_log2) - 1)) * p.kv_ss + h * p.head_dim + c8;
    const long src = token * p.new_ss + h * p.new_sh + c8;
    const f32x4 k0 = ld4(p.k_new + src), k1 = ld4(p.k_new + src + 4);
    const f32x4 v0 = ld4(p.v_new + src), v1 = ld4(p.v_new + src + 4);
    kv_put8<KV>(p.k_pages, dst, k0, k1, p.k_scale, h);
    kv_put8<KV>(p.v_pages, dst, v0, v1, p.v_scale, h);
}

// brn_rope_forward: one thread = 8 consecutive d of a (b, t, head) row, two 16-byte loads and stores; in HALF style the thread of chunk
// c < rot_dim / 16 owns chunk c + rot_dim / 16 too, so a row has head_dim / 8 - rot_dim / 16 threads and both members of every pair are in
// one thread's registers before either is written: y may be x.  Chunks at or past rot_dim are copied.  Threads run d-fastest, then head,
// then token.  The table row comes from device data through a clamp
__global__ void __launch_bounds__(KV_THREADS) rope_kernel(const RopeParams p) {
    const int C8 = p.head_dim >> 3, R16 = p.rot_dim >> 4, half = p.rot_dim >> 1;
    const int W = p.style == 0 ? C8 - R16 : C8;
    const long idx = (long)blockIdx.x * KV_THREADS + threadIdx.x;
    const long per_b = (long)p.seq * p.heads * W;
    if (idx >= per_b * p.batch) return;
    const int b = (int)(idx / per_b);
    const int r = (int)(idx - b * per_b);                          // < seq * heads * head_dim / 8 (launch_rope: < 2^31)
    const int t = r / (p.heads * W), hw = r - t * (p.heads * W);
    const int h = hw / W, w = hw - h * W;
    const long P = p.positions ? max(p.positions[b], 0) : 0;
    const long row = min(P + t, (long)p.n_pos - 1);
    const float* cs = p.cos + row * half;
    const float* sn = p.sin + row * half;
    const long off = b * p.sb + t * p.ss + h * p.sh;
    if (p.style == 0 && w < R16) {
        const long o = off + w * 8;
        f32x4 lo0 = ld4(p.x + o), lo1 = ld4(p.x + o + 4), hi0 = ld4(p.x + o + half), hi1 = ld4(p.x + o + half + 4);
        rope_half8(lo0, lo1, hi0, hi1, cs + w * 8, sn + w * 8);
        *reinterpret_cast<f32x4*>(p.y + o) = lo0; *reinterpret_cast<f32x4*>(p.y + o + 4) = lo1;
        *reinterpret_cast<f32x4*>(p.y + o + half) = hi0; *reinterpret_cast<f32x4*>(p.y + o + half + 4) = hi1;
        return;
    }
    const int c8 = (p.style == 0 ? w + R16 : w) * 8;               // HALF: the chunks past rot_dim; INTERLEAVED: every chunk
    f32x4 x0 = ld4(p.x + off + c8), x1 = ld4(p.x + off + c8 + 4);
    if (p.style != 0 && c8 < p.rot_dim) rope_inter8(x0, x1, cs + (c8 >> 1), sn + (c8 >> 1));
    *reinterpret_cast<f32x4*>(p.y + off + c8) = x0; *reinterpret_cast<f32x4*>(p.y + off + c8 + 4) = x1;
}

__global__ void __launch_bounds__(KV_THREADS) kv_append_lens_kernel(const KvAppendParams p) {
    for (int b = threadIdx.x; b < p.batch; b += KV_THREADS)
        p.kv_lens_out[b] = (int)min((long)min(max(p.kv_lens[b], 0), p.cap) + p.seq_new, (long)p.cap);
}

// ---- the device-side plan of the packed paged entries: brn_flash_paged_varlen_plan.h states the rule, this kernel evaluates it with one
// workgroup.  Thread i owns a contiguous chunk of the n_seqs + 1 entries of cu: the chunk's clamped maximum, the running maximum of the
// chunks before it (LDS), then the starts of its chunk; the tile counts go the same way with a sum.  Every store is a lane's own. ----
constexpr int PV_THREADS = 256;
__global__ void __launch_bounds__(PV_THREADS) paged_varlen_plan_kernel(const int* cu, int n_seqs, int total_q, int G, int* plan) {
    __shared__ int cmax[PV_THREADS];
    __shared__ int csum[PV_THREADS];
    const int tid = threadIdx.x, n1 = n_seqs + 1;
    const int per = (n1 + PV_THREADS - 1) / PV_THREADS;
    const int i0 = min(tid * per, n1), i1 = min(i0 + per, n1);
    int* starts = plan + fa_pv_starts_at();
    int* tiles = plan + fa_pv_tiles_at(n_seqs);
    int mx = 0;
    for (int i = i0; i < i1; ++i) mx = fa_pv_max(mx, fa_pv_clamp(cu[i], total_q));
    cmax[tid] = mx;
    __syncthreads();
    int before = 0;
    for (int j = 0; j < tid; ++j) before = fa_pv_max(before, cmax[j]);
    // the starts of the chunk, and the tiles of its sequences: s_{i + 1} = max(s_i, c_{i + 1})
    int run = before, sum = 0;
    for (int i = i0; i < i1; ++i) {
        run = fa_pv_max(run, fa_pv_clamp(cu[i], total_q));
        starts[i] = run;
        if (i < n_seqs) sum += fa_pv_tiles(G, fa_pv_max(run, fa_pv_clamp(cu[i + 1], total_q)) - run);
    }
    csum[tid] = sum;
    __syncthreads();
    int acc = 0;
    for (int j = 0; j < tid; ++j) acc += csum[j];
    run = before;
    for (int i = i0; i < i1; ++i) {
        run = fa_pv_max(run, fa_pv_clamp(cu[i], total_q));
        tiles[i] = acc;
        if (i < n_seqs) acc += fa_pv_tiles(G, fa_pv_max(run, fa_pv_clamp(cu[i + 1], total_q)) - run);
    }
}

// VARLEN: kv_lens_out[b] = min(L_b + n_b, cap), n_b from the plan's starts; launched after the rows, so kv_lens_out may be kv_lens
__global__ void __launch_bounds__(KV_THREADS) kv_append_lens_varlen_kernel(const KvAppendParams p) {
    const int* starts = p.pv_plan + fa_pv_starts_at();
    for (int b = threadIdx.x; b < p.pv_n_seqs; b += KV_THREADS) {
        const int n = min(max(starts[b + 1] - starts[b], 0), p.pv_total_q);
        p.kv_lens_out[b] = (int)min((long)min(max(p.kv_lens[b], 0), p.cap) + n, (long)p.cap);
    }
}

// what both launchers ask of a table: the kernels index it with nothing but a clamped row and chunk offsets below rot_dim / 2
bool rope_table_ok(const float* cs, const float* sn, int n_pos, int rot_dim, int style, int head_dim) {
    return cs && sn && n_pos >= 1 && n_pos <= (1 << 24) && rot_dim >= 16 && rot_dim <= head_dim && rot_dim % 16 == 0 && (style == 0 || style == 1);
}

}  // namespace

hipError_t launch_paged_varlen_plan(const int* cu, int n_seqs, int total_q, int G, int* plan, hipStream_t s) {
    if (!cu || !plan || n_seqs < 1 || n_seqs > FA_PV_MAX_SEQS || total_q < 1 || G < 1 || (long)G * total_q > 0x7fffffffL) return hipErrorInvalidValue;
    hipLaunchKernelGGL(paged_varlen_plan_kernel, dim3(1), dim3(PV_THREADS), 0, s, cu, n_seqs, total_q, G, plan);
    return hipGetLastError();
}

hipError_t launch_kv_cache_append(const KvAppendParams& p, hipStream_t s) {
    const long cap = (long)p.max_pages << p.page_log2;
    if (p.pv_cu) {
        // the packed form: batch = pv_n_seqs sequences, the tokens [pv_total_q, kv_heads, head_dim]; no rope
        if (!(p.head_dim == 32 || p.head_dim == 64 || p.head_dim == 128) || p.kv_heads < 1 || p.batch != p.pv_n_seqs || p.pv_total_q < 1 || !p.pv_plan || p.rope_cos || p.rope_sin ||
            p.kv_type < 0 || p.kv_type > FA_KV_FP8 || (p.kv_type != FA_KV_FP8 && (p.k_scale || p.v_scale)) || !p.k_new || !p.v_new || !p.k_pages || !p.v_pages || !p.block_table || !p.kv_lens ||
            p.page_log2 < 4 || p.page_log2 > 8 || p.n_pages < 1 || p.max_pages < 1 || ((long)p.n_pages << p.page_log2) > 0x7fffffffL || cap > 0x7fffffffL || p.cap != cap ||
            p.kv_ss != (long)p.kv_heads * p.head_dim || p.page_stride != (p.kv_ss << p.page_log2))
            return hipErrorInvalidValue;
        const long blocks = ((long)p.pv_total_q * p.kv_heads * (p.head_dim / 8) + KV_THREADS - 1) / KV_THREADS;
        if (blocks > 0x7fffffffL) return hipErrorInvalidValue;
        const hipError_t e = launch_paged_varlen_plan(p.pv_cu, p.pv_n_seqs, p.pv_total_q, 1, p.pv_plan, s);
        if (e != hipSuccess) return e;
        const dim3 grid((unsigned)blocks), block(KV_THREADS);
        if (p.kv_type == 0) hipLaunchKernelGGL((kv_append_rows_varlen_kernel<float>), grid, block, 0, s, p);
        else if (p.kv_type == 1) hipLaunchKernelGGL((kv_append_rows_varlen_kernel<__bf16>), grid, block, 0, s, p);
        else if (p.kv_type == 2) hipLaunchKernelGGL((kv_append_rows_varlen_kernel<_Float16>), grid, block, 0, s, p);
        else hipLaunchKernelGGL((kv_append_rows_varlen_kernel<kv_e4m3>), grid, block, 0, s, p);
        if (p.kv_lens_out) hipLaunchKernelGGL(kv_append_lens_varlen_kernel, dim3(1), block, 0, s, p);
        return hipGetLastError();
    }
    if (!(p.head_dim == 32 || p.head_dim == 64 || p.head_dim == 128) || p.batch < 1 || p.kv_heads < 1 || p.seq_new < 1 || p.seq_new > 65536 ||
        p.kv_type < 0 || p.kv_type > FA_KV_FP8 || (p.kv_type != FA_KV_FP8 && (p.k_scale || p.v_scale)) || !p.k_new || !p.v_new || !p.k_pages || !p.v_pages || !p.block_table || !p.kv_lens || p.page_log2 < 4 ||
        p.page_log2 > 8 || p.n_pages < 1 || p.max_pages < 1 || ((long)p.n_pages << p.page_log2) > 0x7fffffffL || cap > 0x7fffffffL || p.cap != cap ||
        p.kv_ss != (long)p.kv_heads * p.head_dim || p.page_stride != (p.kv_ss << p.page_log2))
        return hipErrorInvalidValue;
    const long per_b = (long)p.seq_new * p.kv_heads * (p.head_dim / 8);
    const long blocks = (per_b * p.batch + KV_THREADS - 1) / KV_THREADS;
    if (per_b > 0x7fffffffL || blocks > 0x7fffffffL) return hipErrorInvalidValue;
    const dim3 grid((unsigned)blocks), block(KV_THREADS);
    if (p.rope_cos) {
        if (!rope_table_ok(p.rope_cos, p.rope_sin, p.rope_n_pos, p.rope_dim, p.rope_style, p.head_dim)) return hipErrorInvalidValue;
        if (p.kv_type == 0) hipLaunchKernelGGL((kv_append_rows_kernel<float, true>), grid, block, 0, s, p);
        else if (p.kv_type == 1) hipLaunchKernelGGL((kv_append_rows_kernel<__bf16, true>), grid, block, 0, s, p);
        else if (p.kv_type == 2) hipLaunchKernelGGL((kv_append_rows_kernel<_Float16, true>), grid, block, 0, s, p);
        else hipLaunchKernelGGL((kv_append_rows_kernel<kv_e4m3, true>), grid, block, 0, s, p);
    } else if (p.rope_sin) return hipErrorInvalidValue;
    else if (p.kv_type == 0) hipLaunchKernelGGL((kv_append_rows_kernel<float, false>), grid, block, 0, s, p);
    else if (p.kv_type == 1) hipLaunchKernelGGL((kv_append_rows_kernel<__bf16, false>), grid, block, 0, s, p);
    else if (p.kv_type == 2) hipLaunchKernelGGL((kv_append_rows_kernel<_Float16, false>), grid, block, 0, s, p);
    else hipLaunchKernelGGL((kv_append_rows_kernel<kv_e4m3, false>), grid, block, 0, s, p);
    if (p.kv_lens_out) hipLaunchKernelGGL(kv_append_lens_kernel, dim3(1), block, 0, s, p);
    return hipGetLastError();
}

hipError_t launch_rope(const RopeParams& p, hipStream_t s) {
    if (!(p.head_dim == 32 || p.head_dim == 64 || p.head_dim == 128) || p.batch < 1 || p.heads < 1 || p.seq < 1 || p.seq > 65536 || !p.x || !p.y ||
        !rope_table_ok(p.cos, p.sin, p.n_pos, p.rot_dim, p.style, p.head_dim))
        return hipErrorInvalidValue;
    const int W = p.head_dim / 8 - (p.style == 0 ? p.rot_dim / 16 : 0);
    const long per_b = (long)p.seq * p.heads * (p.head_dim / 8);
    if (per_b > 0x7fffffffL || per_b * p.batch > 0x7fffffffL) return hipErrorInvalidValue;
    const long blocks = ((long)p.batch * p.seq * p.heads * W + KV_THREADS - 1) / KV_THREADS;
    hipLaunchKernelGGL(rope_kernel, dim3((unsigned)blocks), dim3(KV_THREADS), 0, s, p);
    return hipGetLastError();
}

}  // namespace brn
