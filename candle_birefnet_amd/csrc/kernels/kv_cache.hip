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
#include "../brn_kernels.h"
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
    const f32x4 k0 = *reinterpret_cast<const f32x4*>(p.k_new + src), k1 = *reinterpret_cast<const f32x4*>(p.k_new + src + 4);
    const f32x4 v0 = *reinterpret_cast<const f32x4*>(p.v_new + src), v1 = *reinterpret_cast<const f32x4*>(p.v_new + src + 4);
    if constexpr (std::is_same<KV, kv_e4m3>::value) {
        kv_store8_fp8(static_cast<KV*>(p.k_pages) + dst, k0, k1, p.k_scale ? p.k_scale[h] : 1.f);
        kv_store8_fp8(static_cast<KV*>(p.v_pages) + dst, v0, v1, p.v_scale ? p.v_scale[h] : 1.f);
    } else {
        kv_store8(static_cast<KV*>(p.k_pages) + dst, k0, k1);
        kv_store8(static_cast<KV*>(p.v_pages) + dst, v0, v1);
    }
}

__global__ void __launch_bounds__(KV_THREADS) kv_append_lens_kernel(const KvAppendParams p) {
    for (int b = threadIdx.x; b < p.batch; b += KV_THREADS)
        p.kv_lens_out[b] = (int)min((long)min(max(p.kv_lens[b], 0), p.cap) + p.seq_new, (long)p.cap);
}

}  // namespace

hipError_t launch_kv_cache_append(const KvAppendParams& p, hipStream_t s) {
    const long cap = (long)p.max_pages << p.page_log2;
    if (!(p.head_dim == 32 || p.head_dim == 64 || p.head_dim == 128) || p.batch < 1 || p.kv_heads < 1 || p.seq_new < 1 || p.seq_new > 65536 ||
        p.kv_type < 0 || p.kv_type > FA_KV_FP8 || (p.kv_type != FA_KV_FP8 && (p.k_scale || p.v_scale)) || !p.k_new || !p.v_new || !p.k_pages || !p.v_pages || !p.block_table || !p.kv_lens || p.page_log2 < 4 ||
        p.page_log2 > 8 || p.n_pages < 1 || p.max_pages < 1 || ((long)p.n_pages << p.page_log2) > 0x7fffffffL || cap > 0x7fffffffL || p.cap != cap ||
        p.kv_ss != (long)p.kv_heads * p.head_dim || p.page_stride != (p.kv_ss << p.page_log2))
        return hipErrorInvalidValue;
    const long per_b = (long)p.seq_new * p.kv_heads * (p.head_dim / 8);
    const long blocks = (per_b * p.batch + KV_THREADS - 1) / KV_THREADS;
    if (per_b > 0x7fffffffL || blocks > 0x7fffffffL) return hipErrorInvalidValue;
    const dim3 grid((unsigned)blocks), block(KV_THREADS);
    if (p.kv_type == 0) hipLaunchKernelGGL(kv_append_rows_kernel<float>, grid, block, 0, s, p);
    else if (p.kv_type == 1) hipLaunchKernelGGL(kv_append_rows_kernel<__bf16>, grid, block, 0, s, p);
    else if (p.kv_type == 2) hipLaunchKernelGGL(kv_append_rows_kernel<_Float16>, grid, block, 0, s, p);
    else hipLaunchKernelGGL(kv_append_rows_kernel<kv_e4m3>, grid, block, 0, s, p);
    if (p.kv_lens_out) hipLaunchKernelGGL(kv_append_lens_kernel, dim3(1), block, 0, s, p);
    return hipGetLastError();
}

}  // namespace brn
