// gemm_probes.hip — probe kernels of the diag library (libbirefnet_hip_diag.so, include/birefnet_hip_diag.h): the inner loops of the
// split GEMMs (kernels/gemm_split.hip) and the matrix pipe in isolation.  Built by `make diag` only; the product library has none of them.
#include "../brn_kernels.h"
#include "gemm_common.h"

namespace brn {

// diagnostic: the consumer inner loop of the split kernels in isolation — fragments from LDS (ds_read_b128, conflict-free
// layout of the real kernel), NPAIR MFMAs per (i,j) sub-tile, no global memory, no barriers.  variant 0: reads of a k-step
// issued right before its MFMAs; variant 1: next k-step's fragments prefetched into a second register set.
template <int NP, int VARIANT>
__global__ void __launch_bounds__(256) lds_mfma_probe_kernel(int iters, float* sink) {
    constexpr int TM = 2, TN = 2, LD = 40;
    __shared__ __attribute__((aligned(16))) __bf16 smem[NP * 256 * LD];
    for (int i = threadIdx.x; i < NP * 256 * LD; i += 256) smem[i] = (__bf16)((float)((i * 7) & 15) * 0.0625f - 0.4f);
    __syncthreads();
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int wm = wave >> 1, wn = wave & 1;
    const __bf16* a_frag = smem + (wm * 64 + (lane & 31)) * LD + (lane >> 5) * 8;
    const __bf16* b_frag = smem + NP * 128 * LD + (wn * 64 + (lane & 31)) * LD + (lane >> 5) * 8;
    f32x16 acc[TM][TN];
    for (int i = 0; i < TM; ++i) for (int j = 0; j < TN; ++j) for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;
    auto rd = [&](int ks, bf16x8 (&af)[NP][TM], bf16x8 (&bf)[NP][TN]) {
#pragma unroll
        for (int pl = 0; pl < NP; ++pl) {
#pragma unroll
            for (int i = 0; i < TM; ++i) af[pl][i] = *reinterpret_cast<const bf16x8*>(a_frag + (pl * 128 + i * 32) * LD + ks * 16);
#pragma unroll
            for (int j = 0; j < TN; ++j) bf[pl][j] = *reinterpret_cast<const bf16x8*>(b_frag + (pl * 128 + j * 32) * LD + ks * 16);
        }
    };
    auto mm = [&](const bf16x8 (&af)[NP][TM], const bf16x8 (&bf)[NP][TN]) {
#pragma unroll
        for (int sum = NP - 1; sum >= 0; --sum)
#pragma unroll
            for (int pa = 0; pa < NP; ++pa) {
                const int pb = sum - pa;
                if (pb < 0 || pb >= NP) continue;
#pragma unroll
                for (int i = 0; i < TM; ++i)
#pragma unroll
                    for (int j = 0; j < TN; ++j)
                        acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af[pa][i], bf[pb][j], acc[i][j], 0, 0, 0);
            }
    };
    bf16x8 a0[NP][TM], b0[NP][TN], a1[NP][TM], b1[NP][TN];
    if (VARIANT == 0) {
        for (int it = 0; it < iters; ++it) {
            rd(0, a0, b0); mm(a0, b0);
            rd(1, a1, b1); mm(a1, b1);
            asm volatile("" ::: "memory");
        }
    } else {
        rd(0, a0, b0);
        for (int it = 0; it < iters; ++it) {
            rd(1, a1, b1); mm(a0, b0);
            rd(0, a0, b0); mm(a1, b1);
            asm volatile("" ::: "memory");
        }
    }
    float t = 0.f;
    for (int i = 0; i < TM; ++i) for (int j = 0; j < TN; ++j) for (int r = 0; r < 16; ++r) t += acc[i][j][r];
    if (t == 123.456f) sink[0] = t;
}
hipError_t launch_lds_mfma_probe(int blocks, int iters, int np, int variant, float* sink, hipStream_t s) {
#define BRN_P(NP_, V_) hipLaunchKernelGGL((lds_mfma_probe_kernel<NP_, V_>), dim3(blocks), dim3(256), 0, s, iters, sink)
    if (np == 1) { if (variant) BRN_P(1, 1); else BRN_P(1, 0); }
    else if (np == 2) { if (variant) BRN_P(2, 1); else BRN_P(2, 0); }
    else { if (variant) BRN_P(3, 1); else BRN_P(3, 0); }
#undef BRN_P
    return hipGetLastError();
}

// diagnostic: how MFMA and plain VALU work share a SIMD.  8 waves (two per SIMD) per workgroup.
//   mode 0: waves 0-3 MFMA only, waves 4-7 exit        mode 1: waves 4-7 VALU only, waves 0-3 exit
//   mode 2: waves 0-3 MFMA, waves 4-7 VALU (specialised) mode 3: every wave 1/2 of both, VALU interleaved between its MFMAs
//   mode 4: every wave 1/2 of both, VALU in one block after the MFMAs
template <int MODE>
__global__ void __launch_bounds__(512) mfma_valu_probe_kernel(int iters, float* sink) {
    const int wave = threadIdx.x >> 6;
    f32x16 acc[4];
    for (int i = 0; i < 4; ++i) for (int r = 0; r < 16; ++r) acc[i][r] = 0.f;
    bf16x8 a, b;
    for (int e = 0; e < 8; ++e) { a[e] = (__bf16)(0.01f * (threadIdx.x & 31) + e); b[e] = (__bf16)(0.5f - 0.03f * e); }
    float v[6];
    for (int e = 0; e < 6; ++e) v[e] = 1.0f + 0.001f * threadIdx.x + e;
    unsigned u[3] = {0, 0, 0};
#define BRN_MFMA(I) asm volatile("v_mfma_f32_32x32x16_bf16 %0, %1, %2, %0" : "+v"(acc[I]) : "v"(a), "v"(b))
    // the split's op mix per pair of elements: cvt_pk, shift, and, 2 sub, cvt_pk  (6 plain VALU)
#define BRN_VALU6(X, Y, U)                                                             \
    asm volatile("v_cvt_pk_bf16_f32 %0, %1, %2" : "=v"(U) : "v"(X), "v"(Y));          \
    asm volatile("v_lshlrev_b32 %0, 16, %1\n\tv_sub_f32 %0, %2, %0" : "=&v"(X) : "v"(U), "v"(X)); \
    asm volatile("v_and_b32 %0, 0xffff0000, %1\n\tv_sub_f32 %0, %2, %0" : "=&v"(Y) : "v"(U), "v"(Y)); \
    asm volatile("v_cvt_pk_bf16_f32 %0, %1, %2" : "=v"(U) : "v"(X), "v"(Y));
    if (MODE == 0 || MODE == 2) {
        if (wave < 4) {
            for (int it = 0; it < iters; ++it) {
#pragma unroll
                for (int m = 0; m < 24; ++m) BRN_MFMA(m & 3);
            }
        } else if (MODE == 2) {
            for (int it = 0; it < iters; ++it) {
#pragma unroll
                for (int g = 0; g < 12; ++g) { BRN_VALU6(v[(g % 3) * 2], v[(g % 3) * 2 + 1], u[g % 3]) }
            }
        }
    } else if (MODE == 1) {
        if (wave >= 4) {
            for (int it = 0; it < iters; ++it) {
#pragma unroll
                for (int g = 0; g < 12; ++g) { BRN_VALU6(v[(g % 3) * 2], v[(g % 3) * 2 + 1], u[g % 3]) }
            }
        }
    } else if (MODE >= 5) {
        // 5: waves 0-3 MFMA + fragment reads   6: waves 4-7 VALU + LDS stores   7: both   (the warp-specialised GEMM's K-tile shape)
        __shared__ __attribute__((aligned(16))) char lds[40960];
        const int lane = threadIdx.x & 63;
        if (wave < 4 && MODE != 6) {
            const unsigned ra = (unsigned)(size_t)lds + ((wave >> 1) * 64 + (lane & 31)) * 80 + (lane >> 5) * 16;
            f32x4 f[8];
            for (int it = 0; it < iters; ++it) {
#pragma unroll
                for (int ks = 0; ks < 2; ++ks) {
#pragma unroll
                    for (int q = 0; q < 8; ++q)
                        asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(f[q]) : "v"(ra), "n"(0) );
                    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
#pragma unroll
                    for (int m = 0; m < 12; ++m)
                        asm volatile("v_mfma_f32_32x32x16_bf16 %0, %1, %2, %0" : "+v"(acc[m & 3]) : "v"(f[m & 7]), "v"(f[(m + 3) & 7]));
                }
            }
            v[0] += f[0][0];
        } else if (wave >= 4 && MODE != 5) {
            const int pt = threadIdx.x - 256;
            const unsigned wa = (unsigned)(size_t)lds + (pt >> 3) * 80 + (pt & 7) * 8;
            const unsigned wb = (unsigned)(size_t)lds + 20480 + (pt >> 2) * 80 + (pt & 3) * 16;
            f32x4 w4 = {v[0], v[1], v[2], v[3]};
            for (int it = 0; it < iters; ++it) {
#pragma unroll
                for (int g = 0; g < 12; ++g) { BRN_VALU6(v[(g % 3) * 2], v[(g % 3) * 2 + 1], u[g % 3]) }
                unsigned long long d0 = ((unsigned long long)u[0] << 32) | u[1], d1 = ((unsigned long long)u[2] << 32) | u[0];
#pragma unroll
                for (int q = 0; q < 4; ++q)
                    asm volatile("ds_write2st64_b64 %0, %1, %2 offset0:%3 offset1:%4" :: "v"(wa), "v"(d0), "v"(d1), "n"(0), "n"(20) : "memory");
#pragma unroll
                for (int q = 0; q < 4; ++q)
                    asm volatile("ds_write_b128 %0, %1 offset:%2" :: "v"(wb), "v"(w4), "n"(0) : "memory");
                asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
            }
        }
    } else if (MODE == 3) {
        for (int it = 0; it < iters; ++it) {
#pragma unroll
            for (int m = 0; m < 12; ++m) {
                BRN_MFMA(m & 3);
                if (m & 1) { BRN_VALU6(v[(m % 3) * 2], v[(m % 3) * 2 + 1], u[m % 3]) }
            }
        }
    } else {
        for (int it = 0; it < iters; ++it) {
#pragma unroll
            for (int m = 0; m < 12; ++m) BRN_MFMA(m & 3);
#pragma unroll
            for (int g = 0; g < 6; ++g) { BRN_VALU6(v[(g % 3) * 2], v[(g % 3) * 2 + 1], u[g % 3]) }
        }
    }
#undef BRN_MFMA
#undef BRN_VALU6
    float t = v[0] + v[1] + v[2] + v[3] + v[4] + v[5] + (float)(u[0] ^ u[1] ^ u[2]);
    for (int i = 0; i < 4; ++i) for (int r = 0; r < 16; ++r) t += acc[i][r];
    if (t == 123.456f) sink[0] = t;
}
hipError_t launch_mfma_valu_probe(int blocks, int iters, int mode, float* sink, hipStream_t s) {
#define BRN_P(M_) hipLaunchKernelGGL((mfma_valu_probe_kernel<M_>), dim3(blocks), dim3(512), 0, s, iters, sink)
    switch (mode) { case 0: BRN_P(0); break; case 1: BRN_P(1); break; case 2: BRN_P(2); break; case 3: BRN_P(3); break; case 5: BRN_P(5); break; case 6: BRN_P(6); break; case 7: BRN_P(7); break; default: BRN_P(4); break; }
#undef BRN_P
    return hipGetLastError();
}

// diagnostic: back-to-back v_mfma_f32_32x32x2_f32 on register operands (4 independent accumulators per wave); lane 0 of
// each wave reports shader-clock / 100 MHz-realtime-clock ticks so the host can derive the sustained clock
__global__ void mfma_peak_kernel(int iters, float* sink, unsigned long long* clk) {
    f32x16 a0, a1, a2, a3;
    for (int r = 0; r < 16; ++r) { a0[r] = 0.f; a1[r] = 0.f; a2[r] = 0.f; a3[r] = 0.f; }
    float x = (float)(threadIdx.x & 7) * 0.125f - 0.4f, y = (float)(threadIdx.x & 3) * 0.25f - 0.3f;
    const unsigned long long t0 = __builtin_amdgcn_s_memtime(), r0 = __builtin_amdgcn_s_memrealtime();
    for (int i = 0; i < iters; ++i) {
        a0 = __builtin_amdgcn_mfma_f32_32x32x2f32(x, y, a0, 0, 0, 0);
        a1 = __builtin_amdgcn_mfma_f32_32x32x2f32(y, x, a1, 0, 0, 0);
        a2 = __builtin_amdgcn_mfma_f32_32x32x2f32(x, x, a2, 0, 0, 0);
        a3 = __builtin_amdgcn_mfma_f32_32x32x2f32(y, y, a3, 0, 0, 0);
    }
    const unsigned long long t1 = __builtin_amdgcn_s_memtime(), r1 = __builtin_amdgcn_s_memrealtime();
    float acc = 0.f;
    for (int r = 0; r < 16; ++r) acc += a0[r] + a1[r] + a2[r] + a3[r];
    if (acc == 123.456f) sink[0] = acc;
    if (threadIdx.x == 0 && blockIdx.x == 0) { clk[0] = t1 - t0; clk[1] = r1 - r0; }
}
__global__ void mfma_peak_bf16_kernel(int iters, float* sink, unsigned long long* clk, int nacc) {
    f32x16 a0, a1, a2, a3;
    for (int r = 0; r < 16; ++r) { a0[r] = 0.f; a1[r] = 0.f; a2[r] = 0.f; a3[r] = 0.f; }
    bf16x8 x, y;
    for (int j = 0; j < 8; ++j) { x[j] = (__bf16)((float)((threadIdx.x + j) & 7) * 0.125f - 0.4f); y[j] = (__bf16)((float)((threadIdx.x * 3 + j) & 3) * 0.25f - 0.3f); }
    const unsigned long long t0 = __builtin_amdgcn_s_memtime(), r0 = __builtin_amdgcn_s_memrealtime();
    if (nacc == 4) {
        for (int i = 0; i < iters; ++i) {
            a0 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(x, y, a0, 0, 0, 0);
            a1 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(y, x, a1, 0, 0, 0);
            a2 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(x, x, a2, 0, 0, 0);
            a3 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(y, y, a3, 0, 0, 0);
        }
    } else {
        for (int i = 0; i < iters; ++i) {
            a0 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(x, y, a0, 0, 0, 0);
            a0 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(y, x, a0, 0, 0, 0);
            a0 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(x, x, a0, 0, 0, 0);
            a0 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(y, y, a0, 0, 0, 0);
        }
    }
    const unsigned long long t1 = __builtin_amdgcn_s_memtime(), r1 = __builtin_amdgcn_s_memrealtime();
    float acc = 0.f;
    for (int r = 0; r < 16; ++r) acc += a0[r] + a1[r] + a2[r] + a3[r];
    if (acc == 123.456f) sink[0] = acc;
    if (threadIdx.x == 0 && blockIdx.x == 0) { clk[0] = t1 - t0; clk[1] = r1 - r0; }
}
hipError_t launch_mfma_peak_bf16(int blocks, int iters, float* sink, unsigned long long* clk, int nacc, hipStream_t s) {
    hipLaunchKernelGGL(mfma_peak_bf16_kernel, dim3(blocks), dim3(256), 0, s, iters, sink, clk, nacc);
    return hipGetLastError();
}
hipError_t launch_mfma_peak(int blocks, int iters, float* sink, unsigned long long* clk, hipStream_t s) {
    hipLaunchKernelGGL(mfma_peak_kernel, dim3(blocks), dim3(256), 0, s, iters, sink, clk);
    return hipGetLastError();
}

}  // namespace brn
