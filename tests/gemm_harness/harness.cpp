// harness.cpp — test-only C entry points for brn::launch_gemm (kernels/gemm_f32.hip + kernels/gemm_split.hip), so that the suite can force a
// tile, a split-K and every GemmParams field with raw device pointers (tests/gemm_harness.py builds this file together with the two kernel
// files, taken from where they live, into one shared object), and for the weight layouts of brn_pack.h.  No kernel code and no copies here.
// With KH_HOST_ONLY defined only kh_pack_weights is compiled: pure host code, for the stand-alone program pack_main.cpp.
#include "brn_pack.h"

#define KH extern "C" __attribute__((visibility("default")))

// w: host fp32 [N][K], K % 32 == 0.  w_pad: [Npad][K] floats, Npad = N rounded up to 128, the rows >= N zero (GemmParams::W).  planes_out:
// [Npad][K / 32][np][32] 16-bit words (GemmParams::Wp) — np = planes bf16 planes of w_pad, or with half != 0 the fp16 pair of w_scale * w_pad
// (planes must be 2) — or null with planes == 0.  Returns w_scale (1 for bf16 planes), 0 for arguments it refuses.
KH float kh_pack_weights(const float* w, int N, int K, int planes, int half, float* w_pad, uint16_t* planes_out) {
    if (N <= 0 || K <= 0 || K % 32 || !(planes == 0 || planes == 2 || planes == 3) || (half && planes != 2)) return 0.f;
    const size_t npad = ((size_t)N + 127) / 128 * 128;
    std::vector<float> pk(npad * K, 0.f);
    std::copy(w, w + (size_t)N * K, pk.begin());
    std::copy(pk.begin(), pk.end(), w_pad);
    float w_scale = 1.f;
    if (planes) {
        const std::vector<uint16_t> pl = half ? brn::pack_half2_planes(pk, (size_t)K, &w_scale) : brn::pack_bf16_planes(pk, (size_t)K, planes);
        std::copy(pl.begin(), pl.end(), planes_out);
    }
    return w_scale;
}

#ifndef KH_HOST_ONLY
#include "brn_kernels.h"

// the fields of GemmParams in the struct's order (without the deformable loader's, the 16-bit storage modes' and the diagnostics), then the
// plan and the split-K scratch; returns the hipError_t of brn::launch_gemm
KH int kh_launch_gemm(const float* A, const float* W, float* C, int M, int N, int K, int mode, int lda, int a_coff, int Hin, int Win, int Cin,
                      int kh, int kw, int stride, int pad, int dil, int Hout, int Wout, int Kreal, const float* bias, const float* bbias,
                      int bbias_rows, const float* scale, const float* shift, int act, const float* R, int ldr, int r_coff, int ldc, int c_coff,
                      const void* Wp, int planes, int wp_rows, int a_planes, int c_planes, int h2, float a_scale, float out_scale, int c_bf16,
                      int cfg, int splitk, float* ws, void* stream) {
    brn::GemmParams p{};
    p.A = A; p.W = W; p.C = C; p.M = M; p.N = N; p.K = K; p.mode = mode; p.lda = lda; p.a_coff = a_coff;
    p.Hin = Hin; p.Win = Win; p.Cin = Cin; p.kh = kh; p.kw = kw; p.stride = stride; p.pad = pad; p.dil = dil; p.Hout = Hout; p.Wout = Wout;
    p.Kreal = Kreal;
    p.bias = bias; p.bbias = bbias; p.bbias_rows = bbias_rows; p.scale = scale; p.shift = shift; p.act = act;
    p.R = R; p.ldr = ldr; p.r_coff = r_coff; p.ldc = ldc; p.c_coff = c_coff;
    p.Wp = Wp; p.planes = planes; p.wp_rows = wp_rows;
    p.a_planes = a_planes; p.c_planes = c_planes;
    p.h2 = h2; p.a_scale = a_scale; p.out_scale = out_scale;
    p.c_bf16 = c_bf16;
    const brn::GemmPlan plan{cfg, splitk, splitk > 1 ? (size_t)splitk * M * N : 0};
    return (int)brn::launch_gemm(p, plan, ws, reinterpret_cast<hipStream_t>(stream));
}
#endif
