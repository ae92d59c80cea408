// graph_trace_stubs.cpp — every kernel-side symbol the forward graph (csrc/brn_graph*.cpp) links against, and the HIP runtime functions it
// calls, as stubs that log the call to stdout and touch nothing.  Linked with graph_trace_main.cpp into a host-only program
// (tests/test_graph_trace_cpu.py): the log is the sequence of launches the host code enqueues, with every argument, and two versions of the
// host code are equivalent iff their logs are equal.
//
// One line per call: the function, the stream (s<ordinal>), then the arguments in declaration order.  Struct arguments (GemmParams,
// LayerNormParams, WindowAttnParams) are printed field by field as name=value in declaration order; a field that is 0 / null is left out
// (GemmParams::bbias_rows: left out when 1, its value in all but one launch), so every field's value can be read off the line.  Pointers
// are symbolic (graph_trace.h): arena+<offset>, w<id>, img, out, null.
//
// The planners and eligibility tests are NOT the real ones (the test is about the host code, not kernel dispatch): they are small
// deterministic functions of their arguments, chosen so that at the traced shapes (B 1 / 2, 64 x 96 and 32 x 32 images) both outcomes of
// every eligibility test and a split-K scratch allocation occur:
//   plan_gemm(M, N, K, planes)            cfg = 0 (M >= 256) | 1 (M >= 64) | 2, + 3 when planes; split-K min(4, K / 2048) when K >= 4096 and M <= 128,
//                                         ws_floats = splitk * M * N
//   plan_gemm_bf16(M, N, K, f32res, gelu) cfg = (N >= 256 ? 2 : 0) + gelu; split-K 2 when K >= 4096, M <= 128 and not f32res, ws_floats = 2 * M * N
//   gemm_wstat_eligible(p)                K in {192, 384}, N % 192 == 0, M >= 128
//   gemm_wstat_ln_eligible(p)             K == 192, N == 192, M >= 128
//   gemm_rowln_eligible(p)                N in {768, 384}, M >= 64
//   deform_bf16_eligible(p)               M >= 4
//   patch_embed_ln_eligible(...)          Cin 3, N 192, k = stride = 4, H and W multiples of 4, H * W >= 1024
//   gap_scratch_floats(B, HW, C)          B * ceil(HW / 64) * C
// The brn::hf twins (compute mode f16) follow the same rules and log under hf::.
#include "graph_trace.h"
#include "brn_host.h"
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <string>

namespace trace {

static bool g_quiet = false;
static int g_next_event = 0;
void set_quiet(bool q) { g_quiet = q; }
void reset_events() { g_next_event = 0; }

static std::string sym(const void* p) {
    const uintptr_t a = reinterpret_cast<uintptr_t>(p);
    char b[64];
    auto in = [&](uintptr_t base, size_t len) { return a >= base && a - base < len; };
    auto named = [&](const char* n, uintptr_t base) { if (a == base) snprintf(b, sizeof b, "%s", n); else snprintf(b, sizeof b, "%s+%zu", n, (size_t)(a - base)); };
    if (!p) return "null";
    if (in(ARENA_BASE, ARENA_CAP)) snprintf(b, sizeof b, "arena+%zu", (size_t)(a - ARENA_BASE));
    else if (in(W_BASE, (size_t)1 << 36)) {
        const size_t id = (a - W_BASE) / W_STRIDE, off = (a - W_BASE) % W_STRIDE;
        if (off) snprintf(b, sizeof b, "w%zu+%zu", id, off); else snprintf(b, sizeof b, "w%zu", id);
    }
    else if (in(IMG_BASE, (size_t)1 << 36)) named("img", IMG_BASE);
    else if (in(OUT_BASE, (size_t)1 << 36)) named("out", OUT_BASE);
    else if (in(STREAM_BASE, 4096)) snprintf(b, sizeof b, "s%zu", (size_t)(a - STREAM_BASE) / 16);
    else if (in(FORK_BASE, 4096)) snprintf(b, sizeof b, "fork%zu", (size_t)(a - FORK_BASE) / 16);
    else if (in(JOIN_BASE, 4096)) snprintf(b, sizeof b, "join%zu", (size_t)(a - JOIN_BASE) / 16);
    else if (in(STAGE_BASE, 4096)) snprintf(b, sizeof b, "stage%zu", (size_t)(a - STAGE_BASE) / 16);
    else if (in(EV_BASE, (size_t)1 << 30)) snprintf(b, sizeof b, "ev%zu", (size_t)(a - EV_BASE) / 16);
    else snprintf(b, sizeof b, "?");           // a pointer from nowhere: never expected
    return b;
}

// a float in the fewest digits that read back as the same float
static std::string shortest(float v) {
    char b[32];
    snprintf(b, sizeof b, "%g", (double)v);
    if (strtof(b, nullptr) != v) snprintf(b, sizeof b, "%.9g", (double)v);
    return b;
}

// one log line under construction
struct Line {
    std::string s;
    Line(const char* fn, hipStream_t st) : s(fn) { s += ' '; s += sym(st); }
    explicit Line(const char* fn) : s(fn) {}
    Line& raw(const char* fmt, ...) {
        char b[128];
        va_list ap; va_start(ap, fmt); vsnprintf(b, sizeof b, fmt, ap); va_end(ap);
        s += ' '; s += b;
        return *this;
    }
    // positional arguments: always printed
    Line& i(long long v) { return raw("%lld", v); }
    Line& z(size_t v) { return raw("%zu", v); }
    Line& f(float v) { return raw("%s", shortest(v).c_str()); }
    Line& p(const void* v) { s += ' '; s += sym(v); return *this; }
    // struct fields: name=value, left out when 0 / null
    Line& i(const char* k, long long v) { return v ? raw("%s=%lld", k, v) : *this; }
    Line& f(const char* k, float v) { return v != 0.f ? raw("%s=%s", k, shortest(v).c_str()) : *this; }
    Line& p(const char* k, const void* v) { if (v) { s += ' '; s += k; s += '='; s += sym(v); } return *this; }
    hipError_t done() {
        if (!g_quiet) puts(s.c_str());
        return hipSuccess;
    }
};

static Line& gemm(Line& l, const brn::GemmParams& q) {
#define I(F) l.i(#F, q.F)
#define P(F) l.p(#F, q.F)
#define F(F_) l.f(#F_, q.F_)
    P(A); P(W); P(C); I(M); I(N); I(K); I(mode); I(lda); I(a_coff);
    I(Hin); I(Win); I(Cin); I(kh); I(kw); I(stride); I(pad); I(dil); I(Hout); I(Wout); I(Kreal);
    P(om); I(om_ld); I(om_mask_off); I(om_sigmoid);
    P(bias); P(bbias); if (q.bbias_rows != 1) l.raw("bbias_rows=%d", q.bbias_rows); P(scale); P(shift); I(act); P(R); I(ldr); I(r_coff); I(ldc); I(c_coff);
    P(Wp); I(planes); I(wp_rows); I(splitk); P(part); I(a_planes); I(c_planes); I(h2); F(a_scale); F(out_scale);
    I(wp_ld); I(k_chunk_major); I(c_f32); I(r_f32); I(a_bf16); I(c_bf16); P(trace); I(abl);
    return l;
}
static Line& layernorm(Line& l, const brn::LayerNormParams& q) {
    P(x); P(y); I(rows); I(C); P(gamma); P(beta); F(eps); I(ldx); I(ldy); I(y_coff); I(mode); I(H); I(W); I(Cin); I(y_planes); F(y_h2); I(y_bf16);
    return l;
}
static Line& attn(Line& l, const brn::WindowAttnParams& q) {
    P(qkv); P(qkv_bias); P(rel_table); P(out); I(B); I(H); I(W); I(C); I(heads); I(Hp); I(Wp); I(shift); F(scale); I(planes); I(out_planes);
    I(h2); F(out_h2); I(ws); I(io_bf16);
    return l;
}
#undef I
#undef P
#undef F
static Line& plan(Line& l, const brn::GemmPlan& pl, const float* ws) { return l.raw("plan=%d,%d,%zu", pl.cfg, pl.splitk, pl.ws_floats).p("ws", ws); }

// an eligibility query: the verdict, M N K, and a hash of every field (the launch that follows a `1` prints them in full)
static bool verdict(const char* fn, const brn::GemmParams& q, bool yes) {
    Line all(""); gemm(all, q);
    unsigned h = 2166136261u;
    for (char ch : all.s) h = (h ^ (unsigned char)ch) * 16777619u;
    if (!g_quiet) printf("%s M=%d N=%d K=%d #%08x -> %d\n", fn, q.M, q.N, q.K, h, yes ? 1 : 0);
    return yes;
}

}  // namespace trace

using trace::Line;

// ---- HIP runtime ----------------------------------------------------------------------------------------------------------------------
extern "C" {
hipError_t hipEventCreate(hipEvent_t* e) { *e = trace::event(trace::EV_BASE, trace::g_next_event++); return hipSuccess; }
hipError_t hipEventRecord(hipEvent_t e, hipStream_t s) { return Line("hipEventRecord", s).p(e).done(); }
hipError_t hipEventDestroy(hipEvent_t e) { return Line("hipEventDestroy").p(e).done(); }
hipError_t hipStreamWaitEvent(hipStream_t s, hipEvent_t e, unsigned flags) { return Line("hipStreamWaitEvent", s).p(e).i(flags).done(); }
hipError_t hipMemsetAsync(void* dst, int value, size_t bytes, hipStream_t s) { return Line("hipMemsetAsync", s).p(dst).i(value).z(bytes).done(); }
hipError_t hipFree(void* p) { return Line("hipFree").p(p).done(); }
hipError_t hipStreamDestroy(hipStream_t s) { return Line("hipStreamDestroy", s).done(); }
const char* hipGetErrorString(hipError_t) { return "stub"; }
}

namespace brn {

// ---- what the graph takes from brn_weights.cpp ---------------------------------------------------------------------------------------------
void fail(int code, const char* fmt, ...) {
    char buf[1024];
    va_list ap; va_start(ap, fmt); vsnprintf(buf, sizeof buf, fmt, ap); va_end(ap);
    throw Error(code, buf);
}
float half2_act_scale() { return 8.f; }     // the default of BRN_H2_ASCALE
DeviceOwner::~DeviceOwner() {}              // (Model owns one; nothing is ever uploaded here)

// ---- planners and eligibility tests (rules: head of this file) ----------------------------------------------------------------------------
static GemmPlan stub_plan_f32(int M, int N, int K, int planes) {
    GemmPlan pl{(M >= 256 ? 0 : M >= 64 ? 1 : 2) + (planes ? 3 : 0), 1, 0};
    if (K >= 4096 && M <= 128) { pl.splitk = K / 2048 < 4 ? K / 2048 : 4; pl.ws_floats = (size_t)pl.splitk * M * N; }
    return pl;
}
static GemmPlan stub_plan_s16(int M, int N, int K, bool f32res, bool gelu) {
    GemmPlan pl{(N >= 256 ? 2 : 0) + (gelu ? 1 : 0), 1, 0};
    if (K >= 4096 && M <= 128 && !f32res) { pl.splitk = 2; pl.ws_floats = (size_t)2 * M * N; }
    return pl;
}
GemmPlan plan_gemm(int M, int N, int K, int planes) { return stub_plan_f32(M, N, K, planes); }
size_t gap_scratch_floats(int B, int HW, int C) { return (size_t)B * ((HW + 63) / 64) * C; }
bool patch_embed_ln_eligible(int Cin, int N, int k, int stride, int H, int W, int ldw, int ldx) {
    const bool yes = Cin == 3 && N == 192 && k == 4 && stride == 4 && H % 4 == 0 && W % 4 == 0 && H * W >= 1024;
    if (!trace::g_quiet) printf("patch_embed_ln_eligible %d %d %d %d %d %d %d %d -> %d\n", Cin, N, k, stride, H, W, ldw, ldx, yes ? 1 : 0);
    return yes;
}

hipError_t launch_gemm(const GemmParams& p, const GemmPlan& pl, float* ws, hipStream_t s) { Line l("launch_gemm", s); return trace::plan(trace::gemm(l, p), pl, ws).done(); }

// the 16-bit kernels exist twice: namespace brn (bf16) and brn::hf (fp16)
#define S16_STUBS(PFX)                                                                                                                        \
    GemmPlan plan_gemm_bf16(int M, int N, int K, bool f32res, bool gelu) { return stub_plan_s16(M, N, K, f32res, gelu); }                      \
    hipError_t launch_gemm_bf16(const GemmParams& p, const GemmPlan& pl, float* ws, hipStream_t s) {                                          \
        Line l(PFX "launch_gemm_bf16", s); return trace::plan(trace::gemm(l, p), pl, ws).done();                                              \
    }                                                                                                                                         \
    bool gemm_wstat_eligible(const GemmParams& p) { return trace::verdict(PFX "gemm_wstat_eligible", p, (p.K == 192 || p.K == 384) && p.N % 192 == 0 && p.M >= 128); } \
    hipError_t launch_gemm_wstat(const GemmParams& p, hipStream_t s) { Line l(PFX "launch_gemm_wstat", s); return trace::gemm(l, p).done(); } \
    bool gemm_wstat_ln_eligible(const GemmParams& p) { return trace::verdict(PFX "gemm_wstat_ln_eligible", p, p.K == 192 && p.N == 192 && p.M >= 128); } \
    hipError_t launch_gemm_wstat_ln(const GemmParams& p, const float* gamma, const float* beta, float eps, void* y, int ldy, hipStream_t s) { \
        Line l(PFX "launch_gemm_wstat_ln", s); return trace::gemm(l, p).p(gamma).p(beta).f(eps).p(y).i(ldy).done();                          \
    }                                                                                                                                         \
    bool gemm_rowln_eligible(const GemmParams& p) { return trace::verdict(PFX "gemm_rowln_eligible", p, (p.N == 768 || p.N == 384) && p.M >= 64); } \
    hipError_t launch_gemm_rowln(const GemmParams& p, const float* gamma, const float* beta, float eps, void* y, int ldy, hipStream_t s) {    \
        Line l(PFX "launch_gemm_rowln", s); return trace::gemm(l, p).p(gamma).p(beta).f(eps).p(y).i(ldy).done();                             \
    }                                                                                                                                         \
    bool deform_bf16_eligible(const GemmParams& p) { return trace::verdict(PFX "deform_bf16_eligible", p, p.M >= 4); }                        \
    hipError_t launch_deform_bf16(const GemmParams& p, hipStream_t s) { Line l(PFX "launch_deform_bf16", s); return trace::gemm(l, p).done(); }
S16_STUBS("")
namespace hf {
S16_STUBS("hf::")
}
#undef S16_STUBS

// ---- the other launches ----------------------------------------------------------------------------------------------------------------
hipError_t launch_patch_embed_ln(const float* img, int B, int H, int W, const float* wgt, int ldw, const float* bias, const float* gamma, const float* beta,
                                 float eps, float* x, int ldx, hipStream_t s, const float* gamma1, const float* beta1, void* xn, int ldxn, int xn_f16) {
    return Line("launch_patch_embed_ln", s).p(img).i(B).i(H).i(W).p(wgt).i(ldw).p(bias).p(gamma).p(beta).f(eps).p(x).i(ldx).p(gamma1).p(beta1).p(xn).i(ldxn).i(xn_f16).done();
}
hipError_t launch_layernorm(const LayerNormParams& p, hipStream_t s) { Line l("launch_layernorm", s); return trace::layernorm(l, p).done(); }
hipError_t launch_window_attention2(const WindowAttnParams& p, const WindowAttnParams* p2, hipStream_t s) {
    Line l("launch_window_attention2", s);
    trace::attn(l, p);
    if (p2) { l.raw("|"); trace::attn(l, *p2); }
    return l.done();
}
hipError_t launch_resize_nhwc(const float* x, int B, int Hin, int Win, int C, int ldx, int x_coff, float* y, int Hout, int Wout, int ldy, int y_coff, hipStream_t s,
                              int bf16, int accumulate) {
    return Line("launch_resize_nhwc", s).p(x).i(B).i(Hin).i(Win).i(C).i(ldx).i(x_coff).p(y).i(Hout).i(Wout).i(ldy).i(y_coff).i(bf16).i(accumulate).done();
}
hipError_t launch_resize_nchw(const float* x, int BC, int Hin, int Win, float* y, int Hout, int Wout, hipStream_t s) {
    return Line("launch_resize_nchw", s).p(x).i(BC).i(Hin).i(Win).p(y).i(Hout).i(Wout).done();
}
hipError_t launch_image2patches(const float* x, int B, int Cimg, int H, int W, int th, int tw, float* y, int ldy, int cpad, hipStream_t s, int bf16) {
    return Line("launch_image2patches", s).p(x).i(B).i(Cimg).i(H).i(W).i(th).i(tw).p(y).i(ldy).i(cpad).i(bf16).done();
}
hipError_t launch_gap_nhwc(const float* x, int B, int HW, int C, int ldx, int x_coff, float* scratch, float* out, hipStream_t s, int bf16) {
    return Line("launch_gap_nhwc", s).p(x).i(B).i(HW).i(C).i(ldx).i(x_coff).p(scratch).p(out).i(bf16).done();
}
hipError_t launch_small_fc(const float* x, int B, int Cin, const float* w, int ldw, int w_off, int N, const float* scale, const float* shift, int act, float* y,
                           hipStream_t s) {
    return Line("launch_small_fc", s).p(x).i(B).i(Cin).p(w).i(ldw).i(w_off).i(N).p(scale).p(shift).i(act).p(y).done();
}
hipError_t launch_gdt_gate(float* p, int npix, int C, int ldp, int p_coff, const float* g, int ldg, const float* w, float bias, hipStream_t s, int bf16) {
    return Line("launch_gdt_gate", s).p(p).i(npix).i(C).i(ldp).i(p_coff).p(g).i(ldg).p(w).f(bias).i(bf16).done();
}
hipError_t launch_pixel_dot(const float* x, int npix, int C, int ldx, int x_coff, const float* w, float bias, float* y, hipStream_t s, int bf16) {
    return Line("launch_pixel_dot", s).p(x).i(npix).i(C).i(ldx).i(x_coff).p(w).f(bias).p(y).i(bf16).done();
}
hipError_t launch_final_head(const float* q, int B, int h, int w, const float* t, float bias, int H, int W, int apply_sigmoid, float* out, hipStream_t s) {
    return Line("launch_final_head", s).p(q).i(B).i(h).i(w).p(t).f(bias).i(H).i(W).i(apply_sigmoid).p(out).done();
}
hipError_t launch_head_stencil5x5(const float* img, int B, int H, int W, const float* k, const float* bias, float* y, hipStream_t s) {
    return Line("launch_head_stencil5x5", s).p(img).i(B).i(H).i(W).p(k).p(bias).p(y).done();
}
hipError_t launch_mod_sigmoid2(float* x, size_t rows, int ld, int c0, int c1, hipStream_t s) {
    return Line("launch_mod_sigmoid2", s).p(x).z(rows).i(ld).i(c0).i(c1).done();
}

}  // namespace brn
