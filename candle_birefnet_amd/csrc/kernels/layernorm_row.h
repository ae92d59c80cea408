// layernorm_row.h — one LayerNorm row on one wave64, the row kept in registers (two-pass mean / biased variance, eps inside the sqrt),
// float4 loads and stores: the row body of kernels/layernorm.hip, one copy for its three row sources.
// SRC: where the row comes from —
//   LN_SRC_ROWS    x + row * ldx
//   LN_SRC_MERGE   PatchMerging's 2x2 strided gather + concat (swin.rs:505-522) of x [B, H, W, Cin]
//   LN_SRC_SLICES  the raw split-K slices of the GEMM in front (GemmPlan::raw): v = 0; v += part[0] .. part[S-1]; v += bias; v += R — the
//                  operand order of splitk_reduce_kernel, so x keeps its bits — stored to x_out (which may alias R: a lane reads its chunk
//                  before it writes it) and normalised from the registers
#pragma once
#include "../brn_kernels.h"
#include "split_planes.h"

namespace brn {

constexpr int LN_MAX_V = 12;   // float4 per lane: C <= 64*4*12 = 3072
constexpr int LN_WAVES = 4;
constexpr int LN_MAX_BLOCKS = 2048;   // 8 workgroups per CU, grid-stride over rows
enum { LN_SRC_ROWS = 0, LN_SRC_MERGE = 1, LN_SRC_SLICES = 2 };

template <int SRC, int NV>
__device__ __forceinline__ void layernorm_row(const LayerNormParams& p, const long row, const int lane) {
    const int nv = p.C >> 2;   // float4 per row
    f32x4 v[NV];
    int h2 = 0, w2 = 0, bi = 0, Ho = 0, Wo = 0;
    if (SRC == LN_SRC_MERGE) {
        Ho = (p.H + 1) >> 1; Wo = (p.W + 1) >> 1;
        const int hw = Ho * Wo;
        bi = (int)(row / hw);
        const int rem = (int)(row - (long)bi * hw);
        h2 = rem / Wo; w2 = rem - h2 * Wo;
    }
    const int cin4 = p.Cin >> 2;
    const long slice_stride = (long)p.rows * p.C;
    float sum = 0.f;
#pragma unroll
    for (int i = 0; i < NV; ++i) {
        const int c4 = lane + i * 64;
        f32x4 t = {0.f, 0.f, 0.f, 0.f};
        if (c4 < nv) {
            if (SRC == LN_SRC_ROWS) {
                t = *reinterpret_cast<const f32x4*>(p.x + row * p.ldx + c4 * 4);
            } else if (SRC == LN_SRC_MERGE) {
                // concat order (even,even),(odd,even),(even,odd),(odd,odd) in (row,col) — swin.rs:509-519
                const int part = c4 / cin4, cc = c4 - part * cin4;
                const int y = 2 * h2 + (part & 1), x = 2 * w2 + (part >> 1);
                if (y < p.H && x < p.W)
                    t = *reinterpret_cast<const f32x4*>(p.x + (((long)bi * p.H + y) * p.W + x) * p.Cin + cc * 4);
            } else {
                const float* src = p.part + row * p.C + c4 * 4;
#pragma unroll 4
                for (int s = 0; s < p.slices; ++s) t = t + *reinterpret_cast<const f32x4*>(src + s * slice_stride);
                if (p.bias) t = t + *reinterpret_cast<const f32x4*>(p.bias + c4 * 4);
                if (p.R) t = t + *reinterpret_cast<const f32x4*>(p.R + row * p.ldr + p.r_coff + c4 * 4);
            }
            sum += (t[0] + t[1]) + (t[2] + t[3]);
        }
        v[i] = t;
    }
    if (SRC == LN_SRC_SLICES) {      // after every load of the row: x_out may be R
#pragma unroll
        for (int i = 0; i < NV; ++i) {
            const int c4 = lane + i * 64;
            if (c4 < nv) *reinterpret_cast<f32x4*>(p.x_out + row * p.ldxo + p.xo_coff + c4 * 4) = v[i];
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) sum += __shfl_xor(sum, o);
    const float mean = sum / (float)p.C;
    float sq = 0.f;
#pragma unroll
    for (int i = 0; i < NV; ++i) {
        if (lane + i * 64 < nv) {
            const f32x4 d = v[i] - mean;
            sq += (d[0] * d[0] + d[1] * d[1]) + (d[2] * d[2] + d[3] * d[3]);
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) sq += __shfl_xor(sq, o);
    const float rstd = 1.0f / sqrtf(sq / (float)p.C + p.eps);
    float* yrow = p.y + row * p.ldy + p.y_coff;
#pragma unroll
    for (int i = 0; i < NV; ++i) {
        const int c4 = lane + i * 64;
        if (c4 < nv) {
            const f32x4 gm = *reinterpret_cast<const f32x4*>(p.gamma + c4 * 4);
            const f32x4 bt = *reinterpret_cast<const f32x4*>(p.beta + c4 * 4);
            const f32x4 o = (v[i] - mean) * rstd * gm + bt;
            if (p.y_planes && p.y_h2 > 0.f) store_planes_h(p.y + row * p.ldy, p.y_coff + c4 * 4, o, p.y_h2);   // consumer = an fp16-pair GEMM (mode f32_half2)
            else if (p.y_planes) store_planes_n(p.y_planes, p.y + row * p.ldy, p.y_coff + c4 * 4, o);   // consumer = a split-bf16 GEMM (P layout)
            else if (p.y_bf16) {                 // compute mode BRN_BF16: the consumer GEMM reads bf16 (ldy / y_coff in bf16 elements)
                if (p.y_bf16 == 2) {             // compute mode BRN_F16: fp16
                    typedef _Float16 f16x4_ln __attribute__((ext_vector_type(4)));
                    f16x4_ln h;
#pragma unroll
                    for (int e = 0; e < 4; ++e) h[e] = (_Float16)o[e];
                    *reinterpret_cast<f16x4_ln*>(reinterpret_cast<_Float16*>(p.y) + row * p.ldy + p.y_coff + c4 * 4) = h;
                } else {
                bf16x4 h;
#pragma unroll
                for (int e = 0; e < 4; ++e) h[e] = (__bf16)o[e];
                *reinterpret_cast<bf16x4*>(reinterpret_cast<__bf16*>(p.y) + row * p.ldy + p.y_coff + c4 * 4) = h;
                }
            } else *reinterpret_cast<f32x4*>(yrow + c4 * 4) = o;
        }
    }
}

// what launch_layernorm refuses
inline bool layernorm_params_ok(const LayerNormParams& p) {
    if (p.C % 4 || p.C > 64 * 4 * LN_MAX_V || p.rows <= 0) return false;
    if (p.mode == 1 && (p.C != 4 * p.Cin || p.Cin % 4)) return false;
    if (p.y_bf16 && (p.y_planes || p.ldy % 4 || p.y_coff % 4)) return false;
    if (p.y_planes && (!(p.y_planes == 2 || p.y_planes == 3) || p.C % 32 || p.ldy % 16 || p.y_coff % 32)) return false;
    if (p.y_h2 > 0.f && p.y_planes != 2) return false;
    if (p.part && (p.slices < 1 || p.mode != 0 || !p.x_out || (p.ldxo | p.xo_coff) % 4 || (p.R && (p.ldr | p.r_coff) % 4))) return false;
    return true;
}
inline int layernorm_nv(const LayerNormParams& p) {       // the NV instantiation of a width: float4 per lane rounded up to 1, 2, 3, 6, 12
    const int nvl = (p.C / 4 + 63) / 64;
    return nvl <= 3 ? nvl : nvl <= 6 ? 6 : 12;
}

}  // namespace brn
