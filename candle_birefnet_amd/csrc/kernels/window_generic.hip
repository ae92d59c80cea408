// window_generic.hip — the index work of the generic window route (window sides other than 12 and 7; brn_window_generic.cpp): the three
// HBM-bound kernels around launch_flash_attention.  All of the roll / pad / partition / slot arithmetic is kernels/window_generic_geometry.h.
//   window_pack        qkv [B, H, W, 3C] (the qkv GEMM's output, natural token order, the mode's storage type)
//                      -> q, k, v [slots, heads, N, 32] fp32: roll(-shift), pad and window_partition (swin.rs:359-380) as index math; a pad
//                      token's q / k / v is the qkv bias (rounded to the storage type in the 16-bit modes, as the GEMM would write the row)
//   window_bias_build  rel_table [heads][(2 ws - 1)^2] -> bias [patterns, heads, N, N] fp32 = (relative-position bias (swin.rs:147-152,
//                      166-210) [+ the region mask of a border window, swin.rs:603-655]) / scale: the flash kernel adds its bias to the
//                      UNSCALED scores (swin.rs:231-241 pre-multiplies for the same reason)
//   window_scatter     y [slots, heads, N, 32] fp32 -> att [B, H, W, C] in the storage type, heads-major inside C (swin.rs:305-307): window
//                      reverse, roll(+shift) and crop (swin.rs:387-401)
// A thread row (threadIdx.y) owns one token (pack, scatter) or one bias row and does its index arithmetic once; threadIdx.x walks the
// row in 16-byte pieces.  Plain vector loads and stores, no LDS, nothing shared between threads.
#include "../brn_kernels.h"
#include "window_generic_geometry.h"

namespace brn {
namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));

// 16 bytes of storage type T (4 fp32 or 8 16-bit elements) <-> fp32 registers
template <class T> struct Vec16 { static constexpr int N = 16 / (int)sizeof(T); };
template <class T> __device__ __forceinline__ void ld16(const T* p, float (&v)[Vec16<T>::N]) {
    typedef T tv __attribute__((ext_vector_type(Vec16<T>::N)));
    const tv h = *reinterpret_cast<const tv*>(p);
#pragma unroll
    for (int e = 0; e < Vec16<T>::N; ++e) v[e] = (float)h[e];
}
template <class T> __device__ __forceinline__ void st16(T* p, const float (&v)[Vec16<T>::N]) {
    typedef T tv __attribute__((ext_vector_type(Vec16<T>::N)));
    tv h;
#pragma unroll
    for (int e = 0; e < Vec16<T>::N; ++e) h[e] = (T)v[e];
    *reinterpret_cast<tv*>(p) = h;
}
// n fp32 values (n = 4 or 8) as 16-byte accesses
template <int n> __device__ __forceinline__ void ldf(const float* p, float (&v)[n]) {
#pragma unroll
    for (int e = 0; e < n; e += 4) {
        const f32x4 t = *reinterpret_cast<const f32x4*>(p + e);
        v[e] = t[0]; v[e + 1] = t[1]; v[e + 2] = t[2]; v[e + 3] = t[3];
    }
}
template <int n> __device__ __forceinline__ void stf(float* p, const float (&v)[n]) {
#pragma unroll
    for (int e = 0; e < n; e += 4) {
        const f32x4 t = {v[e], v[e + 1], v[e + 2], v[e + 3]};
        *reinterpret_cast<f32x4*>(p + e) = t;
    }
}

// ntok = slots * N window positions; C % 32 == 0, so a 16-byte piece never leaves its head
template <class T>
__global__ void window_pack_kernel(WgenGeom g, const T* __restrict__ qkv, const float* __restrict__ qkv_bias, float* __restrict__ q, float* __restrict__ k,
                                   float* __restrict__ v, int C, int heads, long ntok) {
    constexpr int VEC = Vec16<T>::N;
    const long tok = (long)blockIdx.x * blockDim.y + threadIdx.y;
    if (tok >= ntok) return;
    const int N = wgen_tokens(g);
    const int slot = (int)(tok / N), t = (int)(tok - (long)slot * N), i = t / g.ws, j = t - i * g.ws;
    const WgenWindow w = wgen_slot_window(g, slot);
    const int src = wgen_src_token(g, w.b, w.wy, w.wx, i, j);
    const T* row = src >= 0 ? qkv + (long)src * 3 * C : nullptr;
    float* const dst[3] = {q, k, v};
#pragma unroll
    for (int which = 0; which < 3; ++which) {
        for (int c = threadIdx.x * VEC; c < C; c += blockDim.x * VEC) {
            float x[VEC];
            if (row) ld16<T>(row + which * C + c, x);
            else {
                ldf<VEC>(qkv_bias + which * C + c, x);
#pragma unroll
                for (int e = 0; e < VEC; ++e) x[e] = (float)(T)x[e];
            }
            stf<VEC>(dst[which] + (((long)slot * heads + (c >> 5)) * N + t) * 32 + (c & 31), x);
        }
    }
}

// ntok = B * H * W real tokens
template <class T>
__global__ void window_scatter_kernel(WgenGeom g, const float* __restrict__ y, T* __restrict__ att, int C, int heads, int ld, long ntok) {
    constexpr int VEC = Vec16<T>::N;
    const long tok = (long)blockIdx.x * blockDim.y + threadIdx.y;
    if (tok >= ntok) return;
    const int N = wgen_tokens(g), HW = g.H * g.W;
    const int b = (int)(tok / HW), r = (int)(tok - (long)b * HW), h = r / g.W, w = r - h * g.W;
    const WgenPlace p = wgen_dst_place(g, b, h, w);
    T* out = att + tok * ld;
    for (int c = threadIdx.x * VEC; c < C; c += blockDim.x * VEC) {
        float x[VEC];
        ldf<VEC>(y + (((long)p.slot * heads + (c >> 5)) * N + p.t) * 32 + (c & 31), x);
        st16<T>(out + c, x);
    }
}

// one thread = 4 consecutive keys of one (pattern, head, query) row; blockDim.x covers the whole row (N <= 1024)
__global__ void window_bias_build_kernel(WgenGeom g, const float* __restrict__ rel_table, float* __restrict__ bias, int heads, int n_plain, long nrows,
                                         float inv_scale) {
    const long row = (long)blockIdx.x * blockDim.y + threadIdx.y;
    const int k0 = threadIdx.x * 4, N = wgen_tokens(g);
    if (row >= nrows || k0 >= N) return;
    const int ws = g.ws, side = 2 * ws - 1;
    const int pat = (int)(row / ((long)heads * N)), r = (int)(row - (long)pat * heads * N), h = r / N, qt = r - h * N, qi = qt / ws, qj = qt - qi * ws;
    const bool masked = pat >= n_plain;
    const WgenWindow w = wgen_border_window(g, masked ? pat - n_plain : 0);
    const int rq = masked ? wgen_region(g, w.wy, w.wx, qi, qj) : 0;
    const float* tab = rel_table + (long)h * side * side;
    int ki = k0 / ws, kj = k0 - ki * ws;
    float val[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        if (k0 + e < N) {
            float x = tab[(qi - ki + ws - 1) * side + (qj - kj + ws - 1)];          // swin.rs:182-184
            if (masked && wgen_region(g, w.wy, w.wx, ki, kj) != rq) x += WGEN_MASK;
            val[e] = x * inv_scale;
        }
        if (++kj == ws) { kj = 0; ++ki; }
    }
    float* out = bias + row * N + k0;
    if ((N & 3) == 0) stf<4>(out, val);           // rows are 16-byte aligned exactly when N % 4 == 0
    else {
#pragma unroll
        for (int e = 0; e < 4; ++e) if (k0 + e < N) out[e] = val[e];
    }
}

// threadIdx.x pieces per row (a power of two, at most 256) and rows per 256-thread workgroup
static dim3 row_block(int pieces) {
    int tx = 1;
    while (tx < pieces && tx < 256) tx <<= 1;
    return dim3(tx, 256 / tx);
}
static bool grid_ok(long rows, const dim3& blk, dim3& grid) {
    const long nb = (rows + blk.y - 1) / blk.y;
    if (rows < 1 || nb > 0x7fffffffL) return false;
    grid = dim3((unsigned)nb);
    return true;
}
static bool geometry_ok(const WindowGenericParams& p) {
    if (!(p.B >= 1 && p.H >= 1 && p.W >= 1 && p.heads >= 1 && p.C == p.heads * 32 && p.ws >= WGEN_MIN_WS && p.ws <= WGEN_MAX_WS &&
          (p.shift == 0 || p.shift == p.ws / 2) && p.s16 >= 0 && p.s16 <= 2))
        return false;
    // token and slot numbers are ints (element offsets are 64-bit)
    return ((long)p.H + p.ws) * ((long)p.W + p.ws) * p.B <= 0x7fffffffL;
}

}  // namespace

hipError_t launch_window_pack(const WindowGenericParams& p, hipStream_t s) {
    if (!geometry_ok(p) || !p.qkv || !p.qkv_bias || !p.q || !p.k || !p.v) return hipErrorInvalidValue;
    const WgenGeom g = wgen_geom(p.B, p.H, p.W, p.ws, p.shift);
    const long ntok = (long)wgen_slots(g) * wgen_tokens(g);
    const dim3 blk = row_block(p.C / (p.s16 ? 8 : 4));
    dim3 grid;
    if (!grid_ok(ntok, blk, grid)) return hipErrorInvalidValue;
    if (p.s16 == 1) hipLaunchKernelGGL(window_pack_kernel<__bf16>, grid, blk, 0, s, g, reinterpret_cast<const __bf16*>(p.qkv), p.qkv_bias, p.q, p.k, p.v, p.C, p.heads, ntok);
    else if (p.s16 == 2) hipLaunchKernelGGL(window_pack_kernel<_Float16>, grid, blk, 0, s, g, reinterpret_cast<const _Float16*>(p.qkv), p.qkv_bias, p.q, p.k, p.v, p.C, p.heads, ntok);
    else hipLaunchKernelGGL(window_pack_kernel<float>, grid, blk, 0, s, g, p.qkv, p.qkv_bias, p.q, p.k, p.v, p.C, p.heads, ntok);
    return hipGetLastError();
}

hipError_t launch_window_scatter(const WindowGenericParams& p, hipStream_t s) {
    if (!geometry_ok(p) || !p.y || !p.att || p.ld_att < p.C || p.ld_att % (p.s16 ? 8 : 4)) return hipErrorInvalidValue;
    const WgenGeom g = wgen_geom(p.B, p.H, p.W, p.ws, p.shift);
    const long ntok = (long)p.B * p.H * p.W;
    const dim3 blk = row_block(p.C / (p.s16 ? 8 : 4));
    dim3 grid;
    if (!grid_ok(ntok, blk, grid)) return hipErrorInvalidValue;
    if (p.s16 == 1) hipLaunchKernelGGL(window_scatter_kernel<__bf16>, grid, blk, 0, s, g, p.y, reinterpret_cast<__bf16*>(p.att), p.C, p.heads, p.ld_att, ntok);
    else if (p.s16 == 2) hipLaunchKernelGGL(window_scatter_kernel<_Float16>, grid, blk, 0, s, g, p.y, reinterpret_cast<_Float16*>(p.att), p.C, p.heads, p.ld_att, ntok);
    else hipLaunchKernelGGL(window_scatter_kernel<float>, grid, blk, 0, s, g, p.y, p.att, p.C, p.heads, p.ld_att, ntok);
    return hipGetLastError();
}

hipError_t launch_window_bias_build(const WindowGenericParams& p, hipStream_t s) {
    if (!geometry_ok(p) || !p.rel_table || !p.bias || !(p.scale > 0.f)) return hipErrorInvalidValue;
    const WgenGeom g = wgen_geom(p.B, p.H, p.W, p.ws, p.shift);
    const int N = wgen_tokens(g);
    const long nrows = (long)wgen_bias_patterns(g) * p.heads * N;
    const dim3 blk = row_block((N + 3) / 4);
    dim3 grid;
    if (!grid_ok(nrows, blk, grid)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(window_bias_build_kernel, grid, blk, 0, s, g, p.rel_table, p.bias, p.heads, wgen_plain_patterns(g), nrows, 1.0f / p.scale);
    return hipGetLastError();
}

}  // namespace brn
