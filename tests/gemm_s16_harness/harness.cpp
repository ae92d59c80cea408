// harness.cpp — test-only C entry points for launch_gemm_bf16 of both 16-bit builds (kernels/gemm_bf16.hip as is = namespace brn, and compiled
// with BRN_S16_F16=1 by gemm_f16.cpp beside this file = namespace brn::hf), so that the suite can force a tile, a split-K, the size of the
// persistent grid and every GemmParams field the 16-bit kernels read, with raw device pointers; for the tile planner; and for the weight
// layout of brn_pack.h.  tests/gemm_s16_harness.py builds the three files into one shared object.  No kernel code and no copies here.
#include "brn_pack.h"
#include "brn_kernels.h"

#define KH extern "C" __attribute__((visibility("default")))

// w: host fp32 [N][K] in the packed K order (dense: k; conv: (tap, channel)).  out: rows x ld 16-bit words, or null to ask for the sizes
// only.  conv_taps = kh kw and cinp = Cin for a channels-last conv, 0 for a Linear.  Returns 0, or 1 for arguments it refuses.
KH int kh_pack_s16(const float* w, int N, int K, int f16, int conv_taps, int cinp, uint16_t* out, int* rows, int* ld, int* chunk_major) {
    if (!w || N <= 0 || K <= 0 || conv_taps < 0 || cinp < 0) return 1;
    const std::vector<float> pk(w, w + (size_t)N * K);
    const brn::S16Storage st = brn::pack_s16_storage(pk, (size_t)K, f16 != 0, (size_t)conv_taps, (size_t)cinp);
    *rows = (int)st.rows; *ld = (int)st.ld; *chunk_major = st.chunk_major ? 1 : 0;
    if (out) std::copy(st.w.begin(), st.w.end(), out);
    return 0;
}

// the planner (host only; the two builds hold the same table)
KH void kh_plan_gemm_s16(int M, int N, int K, int f32_residual, int gelu, int* cfg, int* splitk) {
    const brn::GemmPlan pl = brn::plan_gemm_bf16(M, N, K, f32_residual != 0, gelu != 0);
    *cfg = pl.cfg; *splitk = pl.splitk;
}

// the GemmParams fields the 16-bit kernels read, in the struct's order, then the plan by name, the split-K scratch and the CU count the
// persistent grid is sized for (restored to 256 on the same thread); returns the hipError_t of launch_gemm_bf16 of the chosen build
KH int kh_launch_gemm_s16(int f16, const void* A, const void* Wp, void* C, int M, int N, int K, int mode, int lda, int a_coff, int Hin, int Win, int Cin,
                          int kh, int kw, int stride, int pad, int dil, int Hout, int Wout, const float* bias, const float* bbias, int bbias_rows,
                          const float* scale, const float* shift, int act, const void* R, int ldr, int r_coff, int ldc, int c_coff, int wp_rows,
                          int wp_ld, int k_chunk_major, int c_f32, int r_f32, int cfg, int splitk, float* ws, int launch_cus, void* stream) {
    brn::GemmParams p{};
    p.A = static_cast<const float*>(A); p.Wp = Wp; p.C = static_cast<float*>(C); p.M = M; p.N = N; p.K = K; p.mode = mode; p.lda = lda; p.a_coff = a_coff;
    p.Hin = Hin; p.Win = Win; p.Cin = Cin; p.kh = kh; p.kw = kw; p.stride = stride; p.pad = pad; p.dil = dil; p.Hout = Hout; p.Wout = Wout;
    p.bias = bias; p.bbias = bbias; p.bbias_rows = bbias_rows; p.scale = scale; p.shift = shift; p.act = act;
    p.R = static_cast<const float*>(R); p.ldr = ldr; p.r_coff = r_coff; p.ldc = ldc; p.c_coff = c_coff;
    p.planes = 1; p.wp_rows = wp_rows; p.wp_ld = wp_ld; p.k_chunk_major = k_chunk_major; p.c_f32 = c_f32; p.r_f32 = r_f32;
    const brn::GemmPlan plan{cfg, splitk, splitk > 1 ? (size_t)splitk * M * N : 0};
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    brn::set_launch_cus(launch_cus);
    const hipError_t e = f16 ? brn::hf::launch_gemm_bf16(p, plan, ws, s) : brn::launch_gemm_bf16(p, plan, ws, s);
    brn::set_launch_cus(256);
    return (int)e;
}
