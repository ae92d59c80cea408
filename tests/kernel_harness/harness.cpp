// harness.cpp — test-only C entry points for the launchers of kernels/elementwise.hip and kernels/layernorm.hip, so that the
// suite can call each kernel with raw device pointers (tests/kernel_harness.py builds this file together with the two kernel
// files, taken from where they live, into one shared object).  One thin wrapper per launcher: `kh_<launcher>`; the hipError_t
// comes back as an int, the stream goes in as a void*.  No kernel code and no copies here.
#include "brn_kernels.h"

#define KH extern "C" __attribute__((visibility("default")))

static inline hipStream_t st(void* s) { return reinterpret_cast<hipStream_t>(s); }

KH int kh_launch_resize_nhwc(const float* x, int B, int Hin, int Win, int C, int ldx, int x_coff, float* y, int Hout, int Wout, int ldy,
                             int y_coff, void* s, int bf16, int accumulate) {
    return (int)brn::launch_resize_nhwc(x, B, Hin, Win, C, ldx, x_coff, y, Hout, Wout, ldy, y_coff, st(s), bf16, accumulate);
}
KH int kh_launch_resize_nchw(const float* x, int BC, int Hin, int Win, float* y, int Hout, int Wout, void* s) {
    return (int)brn::launch_resize_nchw(x, BC, Hin, Win, y, Hout, Wout, st(s));
}
KH int kh_launch_nchw_to_nhwc(const float* x, int B, int C, int H, int W, float* y, int ldy, int y_coff, void* s, int bf16) {
    return (int)brn::launch_nchw_to_nhwc(x, B, C, H, W, y, ldy, y_coff, st(s), bf16);
}
KH int kh_launch_nhwc_to_nchw(const float* x, int B, int C, int H, int W, int ldx, int x_coff, float* y, void* s, int bf16) {
    return (int)brn::launch_nhwc_to_nchw(x, B, C, H, W, ldx, x_coff, y, st(s), bf16);
}
KH int kh_launch_image2patches(const float* x, int B, int Cimg, int H, int W, int th, int tw, float* y, int ldy, int cpad, void* s, int bf16) {
    return (int)brn::launch_image2patches(x, B, Cimg, H, W, th, tw, y, ldy, cpad, st(s), bf16);
}
KH unsigned long long kh_gap_scratch_floats(int B, int HW, int C) { return (unsigned long long)brn::gap_scratch_floats(B, HW, C); }
KH int kh_launch_gap_nhwc(const float* x, int B, int HW, int C, int ldx, int x_coff, float* scratch, float* out, void* s, int bf16) {
    return (int)brn::launch_gap_nhwc(x, B, HW, C, ldx, x_coff, scratch, out, st(s), bf16);
}
KH int kh_launch_small_fc(const float* x, int B, int Cin, const float* w, int ldw, int w_off, int N, const float* scale, const float* shift,
                          int act, float* y, void* s) {
    return (int)brn::launch_small_fc(x, B, Cin, w, ldw, w_off, N, scale, shift, act, y, st(s));
}
KH int kh_launch_gdt_gate(float* p, int npix, int C, int ldp, int p_coff, const float* g, int ldg, const float* w, float bias, void* s, int bf16) {
    return (int)brn::launch_gdt_gate(p, npix, C, ldp, p_coff, g, ldg, w, bias, st(s), bf16);
}
KH int kh_launch_pixel_dot(const float* x, int npix, int C, int ldx, int x_coff, const float* w, float bias, float* y, void* s, int bf16) {
    return (int)brn::launch_pixel_dot(x, npix, C, ldx, x_coff, w, bias, y, st(s), bf16);
}
KH int kh_launch_final_head(const float* q, int B, int h, int w, const float* t, float bias, int H, int W, int apply_sigmoid, float* out, void* s) {
    return (int)brn::launch_final_head(q, B, h, w, t, bias, H, W, apply_sigmoid, out, st(s));
}
KH int kh_launch_head_stencil5x5(const float* img, int B, int H, int W, const float* k, const float* bias, float* y, void* s) {
    return (int)brn::launch_head_stencil5x5(img, B, H, W, k, bias, y, st(s));
}
KH int kh_launch_f32_to_bf16(const float* x, unsigned long long n, float* y_s16, void* s, int f16) {
    return (int)brn::launch_f32_to_bf16(x, (size_t)n, y_s16, st(s), f16);
}
KH int kh_launch_bf16_to_f32(const float* x_s16, unsigned long long n, float* y, void* s, int f16) {
    return (int)brn::launch_bf16_to_f32(x_s16, (size_t)n, y, st(s), f16);
}
KH int kh_launch_sigmoid(const float* x, unsigned long long n, float* y, void* s) { return (int)brn::launch_sigmoid(x, (size_t)n, y, st(s)); }
KH int kh_launch_mod_sigmoid2(float* x, unsigned long long rows, int ld, int c0, int c1, void* s) {
    return (int)brn::launch_mod_sigmoid2(x, (size_t)rows, ld, c0, c1, st(s));
}
// the fields of LayerNormParams, in the struct's order
KH int kh_launch_layernorm(const float* x, float* y, int rows, int C, const float* gamma, const float* beta, float eps, int ldx, int ldy,
                           int y_coff, int mode, int H, int W, int Cin, int y_planes, float y_h2, int y_bf16, void* s) {
    brn::LayerNormParams p{};
    p.x = x; p.y = y; p.rows = rows; p.C = C; p.gamma = gamma; p.beta = beta; p.eps = eps;
    p.ldx = ldx; p.ldy = ldy; p.y_coff = y_coff;
    p.mode = mode; p.H = H; p.W = W; p.Cin = Cin;
    p.y_planes = y_planes; p.y_h2 = y_h2; p.y_bf16 = y_bf16;
    return (int)brn::launch_layernorm(p, st(s));
}
