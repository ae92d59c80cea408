// brn_graph.cpp — the primitives of the forward graph: the HBM arena, the environment switches, and the run_* pieces that turn a prepared
// weight and its operands into one launch of a gfx950 kernel (activations channels-last in the arena, every concatenation written in place
// into column windows of its consumer's input map).  Built from them: brn_graph_swin.cpp (backbone), brn_graph_model.cpp (the rest).
#include "brn_graph.h"

namespace brn {

// ---- arena ----------------------------------------------------------------------------------------------------------
float* Arena::alloc(size_t nfloats) {
    const size_t bytes = (nfloats * sizeof(float) + 255) & ~(size_t)255;
    const size_t off = top;
    top += bytes;
    if (top > peak) peak = top;
    if (dry) return reinterpret_cast<float*>(off);   // never dereferenced in a dry run
    if (top > cap) fail(BRN_ERR_OOM, "workspace arena overflow: need %zu bytes, have %zu", top, cap);
    return reinterpret_cast<float*>(base + off);
}

Map new_map(Ctx& c, int B, int H, int W, int C) { return Map(c.act_alloc((size_t)B * H * W * C), B, H, W, C); }   // fp32 map, or 16-bit in the 16-bit modes

const Switches& switches() {
    static const Switches sw = [] {
        Switches v;
#define BRN_X(field, name, dflt, doc) if (const char* e = getenv(name)) v.field = atoi(e);
        BRN_SWITCHES(BRN_X)
#undef BRN_X
        return v;
    }();
    return sw;
}

// ---- GEMM descriptors ---------------------------------------------------------------------------------------------------
static int conv_out_size(int in, int k, const GemmW& w) { return (in + 2 * w.pad - w.dil * (k - 1) - 1) / w.stride + 1; }
static void fill_geometry(GemmParams& p, const GemmW& w, int Hin, int Win, int Cin, int Hout, int Wout) {
    p.Hin = Hin; p.Win = Win; p.Cin = Cin; p.kh = w.kh; p.kw = w.kw; p.stride = w.stride; p.pad = w.pad; p.dil = w.dil;
    p.Hout = Hout; p.Wout = Wout; p.Kreal = w.Kreal;
}
static void fill_epilogue(GemmParams& p, const GemmW& w) { p.bias = w.bias; p.scale = w.scale; p.shift = w.shift; p.act = w.act; }
// the weights of the fp32 kernels: the fp32 matrix and, in the split modes, its planes
void fill_weights_f32(GemmParams& p, const GemmW& w) {
    p.W = w.w; p.Wp = w.wp; p.planes = w.planes; p.wp_rows = w.wp_rows;
    p.h2 = w.half;
    if (w.half) { p.a_scale = half2_act_scale(); p.out_scale = 1.f / (p.a_scale * w.w_scale); }
}
GemmParams dense_params(const GemmW& w, const GemmIO& io) {
    GemmParams p{};
    p.A = io.A; p.C = io.C; p.M = io.M; p.N = w.N; p.K = w.K; p.mode = GEMM_DENSE; p.lda = io.lda;
    fill_epilogue(p, w);
    p.bbias = io.bbias; p.bbias_rows = io.bbias_rows;
    p.R = io.R; p.ldr = io.ldr; p.r_coff = io.r_coff; p.ldc = io.ldc; p.c_coff = io.c_coff;
    return p;
}
// a conv over an image / a map of Hin x Win pixels (A, and for a channels-last map lda / a_coff, by the caller) into the window `out`
static GemmParams conv_params(const GemmW& w, const float* A, int Hin, int Win, int Cin, const Map& out, int Hout, int Wout) {
    GemmParams p{};
    p.A = A; p.C = out.p; p.M = out.B * Hout * Wout; p.N = w.N; p.K = w.K; p.mode = w.mode;
    fill_geometry(p, w, Hin, Win, Cin, Hout, Wout);
    fill_epilogue(p, w);
    p.bbias_rows = 1; p.ldc = out.ld; p.c_coff = out.coff;
    return p;
}
static GemmParams conv_params(const GemmW& w, const Map& in, const Map& out, int Hout, int Wout) {
    GemmParams p = conv_params(w, in.p, in.H, in.W, w.Cinp, out, Hout, Wout);
    p.lda = in.ld; p.a_coff = in.coff;
    return p;
}

// split-K scratch: released at once, dead as soon as the reduce pass has been enqueued (in-order stream).  false: a dry run, which ends here
static bool plan_scratch(Ctx& c, const GemmPlan& pl, float** ws) {
    const size_t mk = c.arena->mark();
    *ws = pl.ws_floats ? c.arena->alloc(pl.ws_floats) : nullptr;
    c.arena->release(mk);
    return !c.dry;
}
// algorithmic cost of a GEMM-shaped launch: a_elems elements of A, the weights, M x N results and as many residual elements, by element size
static Cost gemm_cost(const GemmW& w, int M, double a_elems, double a_size, double w_size, double c_size, double r_size = 0.0) {
    return {2.0 * M * (double)w.N * w.K, a_size * a_elems + w_size * (double)w.N * w.K + (c_size + r_size) * (double)M * w.N};
}

// bf16-storage mode: the same GEMM on kernels/gemm_bf16.hip (A bf16; C / R bf16 unless flagged fp32)
static void run_gemm_bf16(Ctx& c, const GemmW& w, GemmParams& p, int fam) {
    if (!w.wb) fail(BRN_ERR_INVALID_ARG, "bf16 mode: weight without a bf16 copy");
    const GemmPlan pl = S16F(c, plan_gemm_bf16)(p.M, p.N, p.K, p.c_f32 && p.R && p.r_f32, p.act == ACT_GELU_ERF);
    float* ws;
    if (!plan_scratch(c, pl, &ws)) return;
    p.Wp = w.wb; p.wp_rows = w.wb_rows; p.wp_ld = w.wb_ld; p.planes = 1;
    if (w.wf && w.mode == GEMM_DENSE && (switches().wstat & (p.K == 384 ? 2 : 1))) {   // short K, wide A: the weights stay in registers (gemm_wstat_bf16_kernel)
        GemmParams q = p;
        q.Wp = w.wf;
        if (S16F(c, gemm_wstat_eligible)(q)) {
            Bracket b(c, fam, gemm_cost(w, q.M, (double)q.M * q.K, 2.0, 2.0, 2.0), q.M, q.N, q.K);
            BRN_LAUNCH(S16F(c, launch_gemm_wstat)(q, c.stream));
            return;
        }
    }
    const double a_elems = p.mode == GEMM_DENSE ? (double)p.M * p.K : (double)p.M / ((double)p.Hout * p.Wout) * p.Hin * p.Win * p.Cin;
    Bracket b(c, fam, gemm_cost(w, p.M, a_elems, 2.0, 2.0, p.c_f32 ? 4.0 : 2.0, p.R ? (p.r_f32 ? 4.0 : 2.0) : 0.0), p.M, p.N, p.K);
    const hipError_t e = S16F(c, launch_gemm_bf16)(p, pl, ws, c.stream);
    if (e != hipSuccess)
        fail(BRN_ERR_HIP, "launch_gemm_bf16 (M %d, N %d, K %d, mode %d, Cin %d, %d x %d -> %d x %d, lda %d + %d, ldc %d + %d, tile cfg %d, split-K %d, chunk-major %d): %s",
             p.M, p.N, p.K, p.mode, p.Cin, p.Hin, p.Win, p.Hout, p.Wout, p.lda, p.a_coff, p.ldc, p.c_coff, pl.cfg, pl.splitk, p.k_chunk_major, hipGetErrorString(e));
}

void run_gemm(Ctx& c, const GemmW& w, const GemmIO& io) {
    GemmParams p = dense_params(w, io);
    if (p.bbias_rows < 1) p.bbias_rows = 1;
    if (c.bf16) {
        p.c_f32 = io.c_f32; p.r_f32 = io.r_f32;
        run_gemm_bf16(c, w, p, FAM_GEMM_DENSE);
        return;
    }
    fill_weights_f32(p, w);
    p.a_planes = io.a_planes; p.c_planes = io.c_planes;
    // A already split by its producer (P layout): the LDS-DMA plane kernel (kernels/gemm_planes.hip), when the shape allows — opt-in
    // (BRN_PLANES_KERNEL=1: measured 10-12 % SLOWER per forward at batch 1) and in the diag build only (make diag)
#ifdef BRN_DIAG_BUILD
    const bool planes_kernel = switches().planes_kernel && io.a_planes && gemm_planes_eligible(p);
    GemmPlan pl = planes_kernel ? plan_gemm_planes(p.M, w.N, w.K, w.planes, io.c_planes != 0) : plan_gemm(p.M, w.N, w.K, w.wp ? w.planes : 0);
#else
    constexpr bool planes_kernel = false;
    GemmPlan pl = plan_gemm(p.M, w.N, w.K, w.wp ? w.planes : 0);
#endif
    if (!planes_kernel && (io.a_planes || io.c_planes)) {
        // otherwise P operands exist only on the warp-specialised kernel; a P output cannot go through the split-K reduce pass
        if (!(w.wp && (w.planes == 2 || w.planes == 3))) fail(BRN_ERR_INVALID_ARG, "P activation layout outside the split modes");
        pl.cfg = 0;
        if (io.c_planes) { pl.splitk = 1; pl.ws_floats = 0; }
    }
    float* ws;
    if (!plan_scratch(c, pl, &ws)) return;
    Bracket b(c, FAM_GEMM_DENSE, gemm_cost(w, p.M, (double)p.M * w.K, 4.0, 4.0, 4.0, p.R ? 4.0 : 0.0), p.M, w.N, w.K);
#ifdef BRN_DIAG_BUILD
    if (planes_kernel) { BRN_LAUNCH(launch_gemm_planes(p, pl, ws, c.stream)); return; }
#endif
    BRN_LAUNCH(launch_gemm(p, pl, ws, c.stream));
}

bool deform_fused_sigmoid(const Ctx& c, const GemmW& w) {
    return c.bf16 && w.mode == GEMM_DEFORM_NHWC && w.wf && !switches().deform_f32 && w.Cinp % 64 == 0 && (w.N & 7) == 0 && w.act != ACT_GELU_ERF;
}

void run_conv(Ctx& c, const GemmW& w, const Map& in, const Map& out, const ConvOpts& o) {
    const int Hout = conv_out_size(in.H, w.kh, w), Wout = conv_out_size(in.W, w.kw, w);
    if (out.H != Hout || out.W != Wout || out.B != in.B || out.C != w.N)
        fail(BRN_ERR_INVALID_ARG, "conv output map [%d,%d,%d,%d] does not match expected [%d,%d,%d,%d]", out.B, out.H, out.W, out.C, in.B, Hout, Wout, w.N);
    if (in.C > w.Cinp || in.coff + w.Cinp > in.ld)
        fail(BRN_ERR_INVALID_ARG, "conv input window (C=%d coff=%d ld=%d) cannot supply %d channels", in.C, in.coff, in.ld, w.Cinp);
    if (w.mode == GEMM_DENSE) {
        run_gemm(c, w, GemmIO(c, in).to(out).f32(o.c_f32, 0));
        return;
    }
    const int M = out.B * Hout * Wout;
    if (c.bf16 && w.mode == GEMM_CONV_NHWC) {
        GemmParams p = conv_params(w, in, out, Hout, Wout);
        p.c_f32 = o.c_f32;
        p.k_chunk_major = w.wb_chunk_major;
        run_gemm_bf16(c, w, p, FAM_GEMM_CONV);
        return;
    }
    if (deform_fused_sigmoid(c, w) && !o.c_f32) {         // the gather on kernels/deform_bf16.hip (16-bit map in / out)
        if (!o.om) fail(BRN_ERR_INVALID_ARG, "deformable conv without an offset/modulator map");
        GemmParams p = conv_params(w, in, out, Hout, Wout);
        p.om = o.om; p.om_ld = o.om_ld; p.om_mask_off = o.om_mask_off; p.om_sigmoid = o.om_sigmoid;
        p.Wp = w.wf; p.planes = 1;
        if (S16F(c, deform_bf16_eligible)(p)) {
            if (c.dry) return;
            // algorithmic bytes: the sampled map once, the offset / modulator map, the weights, the result
            Cost cost = gemm_cost(w, M, (double)in.pixels() * w.Cinp, 2.0, 2.0, 2.0);
            cost.bytes += 4.0 * M * 3.0 * w.kh * w.kw;
            Bracket b(c, FAM_GEMM_DEFORM, cost, M, w.N, w.K);
            BRN_LAUNCH(S16F(c, launch_deform_bf16)(p, c.stream));
            return;
        }
        if (o.om_sigmoid) fail(BRN_ERR_INVALID_ARG, "deformable conv: raw modulator logits passed to a shape the bf16 gather kernel does not cover");
    } else if (o.om_sigmoid) fail(BRN_ERR_INVALID_ARG, "deformable conv: raw modulator logits outside the bf16 gather kernel");
    GemmPlan pl = plan_gemm(M, w.N, w.K, (w.wp && w.mode == GEMM_CONV_NHWC) ? w.planes : 0);
    if (c.bf16) { pl.splitk = 1; pl.ws_floats = 0; }     // (the fp32 split-K reduce pass has no bf16 output; deformable convs only)
    float* ws;
    if (!plan_scratch(c, pl, &ws)) return;
    GemmParams p = conv_params(w, in, out, Hout, Wout);
    p.om = o.om; p.om_ld = o.om_ld; p.om_mask_off = o.om_mask_off;
    fill_weights_f32(p, w);
    if (c.bf16) { p.a_bf16 = c.bf16; p.c_bf16 = o.c_f32 ? 0 : c.bf16; }   // deformable gather in bf16 mode: bf16 map in / out on the fp32-MFMA kernel
    if (w.mode == GEMM_DEFORM_NHWC && !o.om) fail(BRN_ERR_INVALID_ARG, "deformable conv without an offset/modulator map");
    Bracket b(c, w.mode == GEMM_DEFORM_NHWC ? FAM_GEMM_DEFORM : FAM_GEMM_CONV, gemm_cost(w, M, (double)in.pixels() * w.Cinp, 4.0, 4.0, 4.0), M, w.N, w.K);
    BRN_LAUNCH(launch_gemm(p, pl, ws, c.stream));
}

void run_conv_nchw(Ctx& c, const GemmW& w, const float* x, int B, int Hin, int Win, const Map& out, bool pad_to_stride) {
    int Hout = conv_out_size(Hin, w.kh, w), Wout = conv_out_size(Win, w.kw, w);
    // PatchEmbed (swin.rs:696-702) first pads the image with zeros on the right / bottom to a multiple of the patch: for a
    // k == stride, pad 0 conv that is the ceil-mode output size, and the gather loader already returns 0 beyond the border
    if (pad_to_stride && w.kh == w.stride && w.kw == w.stride && w.pad == 0 && w.dil == 1) { Hout = (Hin + w.stride - 1) / w.stride; Wout = (Win + w.stride - 1) / w.stride; }
    if (out.H != Hout || out.W != Wout || out.B != B || out.C != w.N)
        fail(BRN_ERR_INVALID_ARG, "conv(nchw) output map mismatch");
    const int M = B * Hout * Wout;
    const GemmPlan pl = plan_gemm(M, w.N, w.K);
    float* ws;
    if (!plan_scratch(c, pl, &ws)) return;
    GemmParams p = conv_params(w, x, Hin, Win, w.Cin, out, Hout, Wout);
    p.mode = GEMM_GATHER_NCHW;
    fill_weights_f32(p, w);
    Cost cost = gemm_cost(w, M, (double)B * w.Cin * Hin * Win, 4.0, 4.0, 4.0);
    cost.flop = 2.0 * M * (double)w.N * w.Kreal;
    Bracket b(c, FAM_GEMM_GATHER, cost, M, w.N, w.K);
    BRN_LAUNCH(launch_gemm(p, pl, ws, c.stream));
}

void run_layernorm(Ctx& c, const LNW& ln, const float* x, int rows, int ldx, const LnOut& out) {
    if (c.dry) return;
    LayerNormParams p{};
    p.x = x; p.y = out.y; p.rows = rows; p.C = ln.C; p.gamma = ln.g; p.beta = ln.b; p.eps = 1e-5f;
    p.ldx = ldx; p.ldy = out.ldy; p.y_coff = out.y_coff; p.mode = 0; p.y_planes = out.y_planes; p.y_bf16 = out.y_s16;
    p.y_h2 = out.y_planes == 2 ? c.h2_scale : 0.f;
    Bracket b(c, FAM_LAYERNORM, 0.0, (out.y_s16 ? 6.0 : 8.0) * rows * (double)ln.C, rows, ln.C, 0);
    BRN_LAUNCH(launch_layernorm(p, c.stream));
}

void run_resize(Ctx& c, const Map& in, const Map& out, bool accumulate) {
    if (in.C != out.C || in.B != out.B) fail(BRN_ERR_INVALID_ARG, "resize: channel/batch mismatch");
    if (c.dry) return;
    Bracket b(c, FAM_RESIZE, 0.0, (double)c.esz() * ((double)in.pixels() + (double)out.pixels() * (accumulate ? 2 : 1)) * in.C);
    BRN_LAUNCH(launch_resize_nhwc(in.p, in.B, in.H, in.W, in.C, in.ld, in.coff, out.p, out.H, out.W, out.ld, out.coff, c.stream, c.bf16, accumulate ? 1 : 0));
}

// (brn_host.h; no workspace is involved either way, so a dry run and a real run agree trivially)
bool linear_residual_ln(Ctx& c, const GemmW& w, const float* A, int M, int lda, float* x, const LNW& ln, float* y, int ldy, bool every_fused_kernel) {
    // gemm_rowln_bf16_kernel (N = 768 / 384) is built and tested but NOT used by the model by default (BRN_ROWLN: bit 0 = N 768, bit 1 = N 384):
    // its L2 -> LDS intake of W costs what the saved fp32 re-read of x is worth (-0.6 % end to end at c3)
    const int rowln_mask = every_fused_kernel ? 3 : switches().rowln;
    if (!c.bf16 || w.mode != GEMM_DENSE || ln.C != w.N || !ln.g || !ln.b) return false;
    GemmParams p = dense_params(w, GemmIO(A, M, lda).to(x, w.N).add(x, w.N));
    p.c_f32 = 1; p.r_f32 = 1;
    p.planes = 1;
    // wide stages: the workgroup owns 64 whole rows and W streams through LDS (gemm_rowln_bf16_kernel); else gemm_wstat_ln_bf16_kernel
    bool rowln = false;
    if (w.wb && (rowln_mask & (w.N == 768 ? 1 : w.N == 384 ? 2 : 0))) {
        p.Wp = w.wb; p.wp_rows = w.wb_rows; p.wp_ld = w.wb_ld;
        rowln = S16F(c, gemm_rowln_eligible)(p);
    }
    if (!rowln) {
        if (!switches().wstat_ln || !w.wf) return false;
        p.Wp = w.wf; p.wp_rows = 0; p.wp_ld = 0;
        if (!S16F(c, gemm_wstat_ln_eligible)(p)) return false;
    }
    if (c.dry) return true;
    Bracket b(c, FAM_GEMM_DENSE, gemm_cost(w, M, (double)M * w.K, 2.0, 2.0, 4.0 + 2.0, 4.0), M, w.N, w.K);      // x written, y written, x read
    if (rowln) BRN_LAUNCH(S16F(c, launch_gemm_rowln)(p, ln.g, ln.b, 1e-5f, y, ldy, c.stream));
    else BRN_LAUNCH(S16F(c, launch_gemm_wstat_ln)(p, ln.g, ln.b, 1e-5f, y, ldy, c.stream));
    return true;
}

}  // namespace brn
