// deform_im2col.hip — the two kernels of brn_deform_conv2d_offsets_forward (host route: ../brn_deform_offsets.cpp; index math:
// deform_sample_geometry.h).  Both are HBM-bound data movement; the contraction that follows runs on the mode's existing GEMM kernels.
//
//   deform_om_pack_kernel   route 1 (fused): the caller's NCHW offset [B, 2 kh kw, Ho, Wo] and mask [B, kh kw, Ho, Wo] (one offset group)
//                           -> the fp32 map [B, Ho, Wo, ld] the gather loaders read (GemmParams::om): 2 kh kw offsets, kh kw multipliers
//                           (exactly 1.0f without a mask), zero pad columns.  A 32 x 32 transposition through LDS, both sides coalesced.
//   deform_im2col_kernel    route 2 (columns): the reference's Metal path taken literally (call_deformable_im2col, deform_conv.rs:101-215 /
//                           aspp.rs:58-165) — rows [m0, m0 + rows) of the column matrix [pixels][kh kw Cp], K = (tap, channel), in the
//                           storage type of the channels-last map it samples.  A lane owns one (pixel, tap, 16-byte channel chunk): mask x
//                           bilinear in fp32 (the arithmetic of gemm_f32_kernel's loader), rounded ONCE to the storage type (the rounding
//                           kernels/deform_bf16.hip applies to its A tile).  Consecutive lanes write consecutive 16-byte chunks: the stores
//                           of a wave are one contiguous kilobyte.  Pad channels [C, Cp) are written as zeros and never read.
//                           Offset groups: when C / G is a multiple of the chunk no chunk straddles a group and a lane does four 16-byte
//                           corner loads (VEC); otherwise every lane of the launch walks its chunk element by element (a group boundary
//                           may fall anywhere), the choice being a template argument, uniform over the launch.
// No address depends on an offset value except through deform_sample, whose indices are clamped into the image after a range test on the
// floats: NaN, infinite and huge offsets contribute 0.
#include <hip/hip_runtime.h>
#include "../brn_kernels.h"
#include "deform_sample_geometry.h"

namespace brn {

__global__ void __launch_bounds__(256) deform_om_pack_kernel(const float* __restrict__ offset, const float* __restrict__ mask, int taps, int HW,
                                                             int tiles_p, float* __restrict__ om, int ld) {
    __shared__ float tile[32][33];
    const int b = blockIdx.x / tiles_p, p0 = (blockIdx.x - b * tiles_p) * 32, c0 = blockIdx.y * 32;
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;   // 256 threads: 32 x 8
    for (int i = ty; i < 32; i += 8) {
        const int c = c0 + i, pq = p0 + tx;
        float v = 0.f;
        if (pq < HW) {
            if (c < 2 * taps) v = offset[((size_t)b * 2 * taps + c) * HW + pq];
            else if (c < 3 * taps) v = mask ? mask[((size_t)b * taps + (c - 2 * taps)) * HW + pq] : 1.0f;
        }
        tile[i][tx] = v;
    }
    __syncthreads();
    for (int i = ty; i < 32; i += 8) {
        const int pq = p0 + i, c = c0 + tx;
        if (pq < HW && c < ld) om[((size_t)b * HW + pq) * ld + c] = tile[tx][i];
    }
}

hipError_t launch_deform_om_pack(const DeformOffsetsParams& p, hipStream_t s) {
    const int taps = p.kh * p.kw, HW = p.Ho * p.Wo;
    if (p.G != 1 || !p.offset || !p.om || p.B < 1 || HW < 1 || taps < 1 || p.om_ld < 3 * taps) return hipErrorInvalidValue;
    const int tiles_p = (HW + 31) / 32;
    if ((long long)tiles_p * p.B > 0x7fffffffLL) return hipErrorInvalidValue;
    hipLaunchKernelGGL(deform_om_pack_kernel, dim3((unsigned)(tiles_p * p.B), (unsigned)((p.om_ld + 31) / 32)), dim3(256), 0, s, p.offset, p.mask, taps, HW,
                       tiles_p, p.om, p.om_ld);
    return hipGetLastError();
}

template <class T, bool VEC>
__global__ void __launch_bounds__(256) deform_im2col_kernel(const DeformOffsetsParams p) {
    constexpr int E = 16 / (int)sizeof(T);                  // channels of a 16-byte chunk
    typedef T vecT __attribute__((ext_vector_type(E)));
    const int taps = p.kh * p.kw, cpr = p.Cp / E, hw = p.Ho * p.Wo;
    const long long total = (long long)p.rows * taps * cpr;
    const bool narrow = total <= 0xffffffffLL;
    const T* __restrict__ x = reinterpret_cast<const T*>(p.x);
    T* __restrict__ col = reinterpret_cast<T*>(p.col);
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
        int cc, tap, ml;
        if (narrow) {                                         // uniform over the launch: 32-bit divisions (the 64-bit ones cost several times as much)
            const unsigned u = (unsigned)i, r = u / (unsigned)cpr;
            cc = (int)(u - r * (unsigned)cpr);
            ml = (int)(r / (unsigned)taps);
            tap = (int)(r - (unsigned)ml * (unsigned)taps);
        } else {
            const long long r = i / cpr;
            cc = (int)(i - r * cpr);
            ml = (int)(r / taps);
            tap = (int)(r - (long long)ml * taps);
        }
        const int m = p.m0 + ml;
        const int b = m / hw, rem = m - b * hw;
        const int oy = rem / p.Wo, ox = rem - oy * p.Wo;
        const int ky = tap / p.kw, kx = tap - ky * p.kw;
        const int c0 = cc * E;
        const float fy = (float)deform_tap_origin(oy, ky, p.stride_h, p.pad_h, p.dil_h);
        const float fx = (float)deform_tap_origin(ox, kx, p.stride_w, p.pad_w, p.dil_w);
        const float* offb = p.offset + (size_t)b * 2 * p.G * taps * hw + rem;
        const float* mskb = p.mask ? p.mask + (size_t)b * p.G * taps * hw + rem : nullptr;
        const T* xb = x + (size_t)b * p.H * p.W * p.ldx;
        float acc[E];
#pragma unroll
        for (int e = 0; e < E; ++e) acc[e] = 0.f;
        if (VEC) {
            if (c0 < p.C) {                                   // C % E == 0 here: a chunk is all real channels or all pad
                const int g = deform_group_of(c0, p.C, p.G);
                const int oc = deform_offset_channel(g, tap, taps);
                const float dy = offb[(size_t)oc * hw], dx = offb[(size_t)(oc + 1) * hw];
                const float mk = mskb ? mskb[(size_t)deform_mask_channel(g, tap, taps) * hw] : 1.0f;
                const DeformSample sp = deform_sample(fy + dy, fx + dx, p.H, p.W);
                if (sp.ok) {
#pragma unroll
                    for (int q = 0; q < 4; ++q) {
                        if (sp.ok & (1u << q)) {
                            const vecT v = *reinterpret_cast<const vecT*>(xb + (size_t)sp.idx[q] * p.ldx + c0);
#pragma unroll
                            for (int e = 0; e < E; ++e) acc[e] += sp.w[q] * (float)v[e];
                        }
                    }
#pragma unroll
                    for (int e = 0; e < E; ++e) acc[e] *= mk;
                }
            }
        } else {
            int g_cur = -1;
            float mk = 1.0f;
            DeformSample sp = deform_sample(-2.f, -2.f, p.H, p.W);      // (nothing sampled yet)
#pragma unroll
            for (int e = 0; e < E; ++e) {
                const int c = c0 + e;
                if (c >= p.C) break;
                const int g = deform_group_of(c, p.C, p.G);
                if (g != g_cur) {
                    g_cur = g;
                    const int oc = deform_offset_channel(g, tap, taps);
                    const float dy = offb[(size_t)oc * hw], dx = offb[(size_t)(oc + 1) * hw];
                    mk = mskb ? mskb[(size_t)deform_mask_channel(g, tap, taps) * hw] : 1.0f;
                    sp = deform_sample(fy + dy, fx + dx, p.H, p.W);
                }
                float a = 0.f;
#pragma unroll
                for (int q = 0; q < 4; ++q)
                    if (sp.ok & (1u << q)) a += sp.w[q] * (float)xb[(size_t)sp.idx[q] * p.ldx + c];
                acc[e] = sp.ok ? mk * a : 0.f;
            }
        }
        vecT o;
#pragma unroll
        for (int e = 0; e < E; ++e) o[e] = (T)acc[e];
        *reinterpret_cast<vecT*>(col + ((size_t)ml * taps + tap) * p.Cp + c0) = o;
    }
}

template <class T>
static hipError_t launch_im2col_t(const DeformOffsetsParams& p, hipStream_t s) {
    constexpr int E = 16 / (int)sizeof(T);
    const long long total = (long long)p.rows * p.kh * p.kw * (p.Cp / E);
    long long blocks = (total + 255) / 256;
    if (blocks > 2048) blocks = 2048;                        // 256 CUs x 8 workgroups; grid-stride beyond
    const bool vec = (p.C / p.G) % E == 0;
    if (vec) hipLaunchKernelGGL((deform_im2col_kernel<T, true>), dim3((unsigned)blocks), dim3(256), 0, s, p);
    else hipLaunchKernelGGL((deform_im2col_kernel<T, false>), dim3((unsigned)blocks), dim3(256), 0, s, p);
    return hipGetLastError();
}

hipError_t launch_deform_im2col(const DeformOffsetsParams& p, hipStream_t s) {
    if (!p.x || !p.col || !p.offset || p.B < 1 || p.C < 1 || p.H < 1 || p.W < 1 || p.kh < 1 || p.kw < 1 || p.G < 1 || p.C % p.G || p.Ho < 1 || p.Wo < 1 ||
        p.stride_h < 1 || p.stride_w < 1 || p.dil_h < 1 || p.dil_w < 1 || p.pad_h < 0 || p.pad_w < 0)
        return hipErrorInvalidValue;
    if (p.Cp < p.C || p.Cp % 32 || p.ldx < p.Cp || p.ldx % 8 || p.rows < 1 || p.m0 < 0 || (long long)p.m0 + p.rows > (long long)p.B * p.Ho * p.Wo)
        return hipErrorInvalidValue;
    if ((reinterpret_cast<uintptr_t>(p.x) | reinterpret_cast<uintptr_t>(p.col)) & 15) return hipErrorInvalidValue;
    if (p.s16 == 2) return launch_im2col_t<_Float16>(p, s);
    if (p.s16 == 1) return launch_im2col_t<__bf16>(p, s);
    if (p.s16 == 0) return launch_im2col_t<float>(p, s);
    return hipErrorInvalidValue;
}

}  // namespace brn
