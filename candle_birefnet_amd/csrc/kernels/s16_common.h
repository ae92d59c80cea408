// s16_common.h — the 16-bit storage-type prelude of the kernel files that are compiled twice (Makefile): as is for compute mode BRN_BF16, and
// with -DBRN_S16_F16=1 for BRN_F16 — the same kernels with fp16 as the 16-bit storage / MFMA operand type (3 more mantissa bits at the same
// bytes and the same matrix rate), in namespace brn::hf.  Those files are gemm_bf16.hip, rows_bf16.hip and deform_bf16.hip.
//
// Namespaces: this header closes what it opens.  A .hip file puts its own code between BRN_S16_BEGIN and BRN_S16_END, which open and close
// namespace brn (bf16 build) or brn::hf (fp16 build) — the namespace everything below lives in.  What comes from gemm_common.h stays in brn.
#pragma once
#include "gemm_common.h"

#ifndef BRN_S16_F16
#define BRN_S16_F16 0
#endif
#if BRN_S16_F16
#define BRN_S16_BEGIN namespace brn { namespace hf {
#define BRN_S16_END }}
#define BRN_S16_SELF(FN) hf::FN      // (an unqualified call would also find the brn:: function of the same name through its brn::GemmParams argument)
#define BRN_MFMA_32X32X16(A, B, C) __builtin_amdgcn_mfma_f32_32x32x16_f16(A, B, C, 0, 0, 0)
#define BRN_MFMA_16X16X32(A, B, C) __builtin_amdgcn_mfma_f32_16x16x32_f16(A, B, C, 0, 0, 0)
#else
#define BRN_S16_BEGIN namespace brn {
#define BRN_S16_END }
#define BRN_S16_SELF(FN) FN
#define BRN_MFMA_32X32X16(A, B, C) __builtin_amdgcn_mfma_f32_32x32x16_bf16(A, B, C, 0, 0, 0)
#define BRN_MFMA_16X16X32(A, B, C) __builtin_amdgcn_mfma_f32_16x16x32_bf16(A, B, C, 0, 0, 0)
#endif

BRN_S16_BEGIN
#if BRN_S16_F16
typedef _Float16 s16_t;
#else
typedef __bf16 s16_t;
#endif
typedef s16_t s16x8 __attribute__((ext_vector_type(8)));

__device__ __forceinline__ unsigned pack_bf16x2(float lo, float hi) {      // v_cvt_pk_bf16_f32 / v_cvt_pk_f16_f32 (round to nearest even): lo in bits 0-15
    typedef s16_t s16x2 __attribute__((ext_vector_type(2)));
    const s16x2 t = {(s16_t)lo, (s16_t)hi};
    return __builtin_bit_cast(unsigned, t);
}
// the two 16-bit storage values packed in a dword, as fp32
__device__ __forceinline__ float s16_lo_f32(unsigned r) {
#if BRN_S16_F16
    typedef _Float16 h2 __attribute__((ext_vector_type(2)));
    return (float)__builtin_bit_cast(h2, r)[0];
#else
    return __builtin_bit_cast(float, r << 16);
#endif
}
__device__ __forceinline__ float s16_hi_f32(unsigned r) {
#if BRN_S16_F16
    typedef _Float16 h2 __attribute__((ext_vector_type(2)));
    return (float)__builtin_bit_cast(h2, r)[1];
#else
    return __builtin_bit_cast(float, r & 0xffff0000u);
#endif
}
__device__ __forceinline__ float bf16_bits_to_f32(unsigned short h) { return s16_lo_f32((unsigned)h); }

// byte offset of 16-byte chunk c (0..7) of tile row r (128-byte rows) in the swizzled image of a K-step-64 tile: rows 2p, 2p+1 share a
// 256-byte bank row whose sixteen 16-byte slots are permuted by p & 15 (conflict-free fragment reads)
__device__ __forceinline__ int swz_slot(int r, int c) { return (r >> 1) * 256 + (((((r & 1) << 3) | c) ^ ((r >> 1) & 15)) << 4); }

// LDS-DMA, 16 bytes per lane: 64-bit per-lane address / buffer resource + 32-bit lane offset + uniform offset
__device__ __forceinline__ void glds16(const void* gsrc, void* lds_dst) {
    __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)gsrc,
                                     (__attribute__((address_space(3))) void*)lds_dst, 16, 0, 0);
}
__device__ __forceinline__ void blds16(__amdgpu_buffer_rsrc_t rsrc, unsigned voff, int soff, void* lds_dst) {
    __builtin_amdgcn_raw_ptr_buffer_load_lds(rsrc, (__attribute__((address_space(3))) void*)lds_dst, 16, voff, soff, 0, 0);
}
template <int N> __device__ __forceinline__ void wait_vmcnt() { asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory"); }
BRN_S16_END
