// harness.cpp — test-only C entry points for the GEMM -> LayerNorm pair with the split-K slices summed by the LayerNorm: brn::launch_gemm with
// GemmPlan::raw and brn::launch_layernorm with every LayerNormParams field (tests/gemm_ln_harness.py builds this file with
// kernels/gemm_f32.hip, gemm_split.hip and layernorm.hip, taken from where they live).  No kernel code here.
#include "brn_kernels.h"

#define KH extern "C" __attribute__((visibility("default")))

// kh_launch_gemm of tests/gemm_harness/harness.cpp with one more argument behind the stream: GemmPlan::raw
KH int kh_launch_gemm_raw(const float* A, const float* W, float* C, int M, int N, int K, int mode, int lda, int a_coff, int Hin, int Win, int Cin,
                          int kh, int kw, int stride, int pad, int dil, int Hout, int Wout, int Kreal, const float* bias, const float* bbias,
                          int bbias_rows, const float* scale, const float* shift, int act, const float* R, int ldr, int r_coff, int ldc, int c_coff,
                          const void* Wp, int planes, int wp_rows, int a_planes, int c_planes, int h2, float a_scale, float out_scale, int c_bf16,
                          int cfg, int splitk, float* ws, void* stream, int raw) {
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
    brn::GemmPlan plan{cfg, splitk, splitk > 1 ? (size_t)splitk * M * N : 0};
    plan.raw = raw;
    return (int)brn::launch_gemm(p, plan, ws, reinterpret_cast<hipStream_t>(stream));
}

// LayerNormParams field by field (tests/gemm_ln_harness.py mirrors this struct)
struct KhLayerNorm {
    const float* x; float* y; int rows, C; const float* gamma; const float* beta; float eps;
    int ldx, ldy, y_coff, mode, H, W, Cin, y_planes; float y_h2; int y_bf16;
    const float* part; int slices; const float* bias; const float* R; int ldr, r_coff; float* x_out; int ldxo, xo_coff;
};
static brn::LayerNormParams params_of(const KhLayerNorm& k) {
    brn::LayerNormParams p{};
    p.x = k.x; p.y = k.y; p.rows = k.rows; p.C = k.C; p.gamma = k.gamma; p.beta = k.beta; p.eps = k.eps;
    p.ldx = k.ldx; p.ldy = k.ldy; p.y_coff = k.y_coff; p.mode = k.mode; p.H = k.H; p.W = k.W; p.Cin = k.Cin;
    p.y_planes = k.y_planes; p.y_h2 = k.y_h2; p.y_bf16 = k.y_bf16;
    p.part = k.part; p.slices = k.slices; p.bias = k.bias; p.R = k.R; p.ldr = k.ldr; p.r_coff = k.r_coff;
    p.x_out = k.x_out; p.ldxo = k.ldxo; p.xo_coff = k.xo_coff;
    return p;
}
KH int kh_launch_layernorm_p(const KhLayerNorm* k, void* stream) { return (int)brn::launch_layernorm(params_of(*k), reinterpret_cast<hipStream_t>(stream)); }
