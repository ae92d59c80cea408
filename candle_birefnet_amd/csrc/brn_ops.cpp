// brn_ops.cpp — the op-level entry points behind the extern "C" boundary (tests, the Rust shim): single layers and modules built from host
// weights per call, in the arithmetic brn_set_op_compute selected on the calling thread.  Weights are always host pointers; x / y /
// residual follow `loc`.
#include "brn_api_util.h"
#include "brn_flash_paged_varlen_plan.h"
#include "brn_flash_split_plan.h"
#include "brn_flash_varlen_plan.h"
#include "brn_graph.h"
#include "kernels/deform_sample_geometry.h"
#include <cmath>
#include <cstring>
#include <memory>

using namespace brn;

struct brn_swin { brn_config cfg; int device; DeviceOwner own; SwinW w; std::mutex mu; int bf16 = 0; };

namespace {

// brn_set_op_compute: thread-local by contract of the ABI (default BRN_F32).  Every entry reads it once and passes it down.
thread_local WeightBuild g_op;
inline int op_s16(WeightBuild wb, bool on = true) { return on && wb.planes == BUILD_BF16 ? (wb.f16 ? 2 : 1) : 0; }   // Ctx::bf16 of the entry's maps
// the q/k/v attention entries: in modes bf16 / f16 q, k, v are rounded to the 16-bit type as the kernel loads them; every other mode runs
// the exact fp32-MFMA kernel between its own GEMMs (as window-7 attention does)
inline int attention_op_s16() { return op_s16(g_op); }

// compute modes BRN_BF16 / BRN_F16 at op level: x is rounded to the 16-bit storage type at the edge, as the producing kernel of the
// model would have written it; what the entry returns stays fp32 at this boundary
const float* round_to_s16(Ctx& c, const float* dx, size_t n, bool f16) {
    float* xb = c.arena->alloc_bytes(n * 2);
    if (!c.dry) BRN_HIP(launch_f32_to_bf16(dx, n, xb, c.stream, f16));
    return xb;
}

// x [B][C][H][W] -> channels-last map X of Cp >= C channels (the pad channels zero) -> body(c, X, Y) -> y [B][O][Ho][Wo]
void through_nhwc(void* stream, int s16, const float* dx, int B, int C, int Cp, int H, int W, float* dy, int O, int Ho, int Wo,
                  const std::function<void(Ctx&, const Map&, const Map&)>& body) {
    with_arena((hipStream_t)stream, [&](Ctx& c) {
        Map X = new_map(c, B, H, W, Cp), Y = new_map(c, B, Ho, Wo, O);
        if (!c.dry) {
            if (Cp != C) BRN_HIP(hipMemsetAsync(X.p, 0, (size_t)B * H * W * Cp * c.esz(), c.stream));
            BRN_HIP(launch_nchw_to_nhwc(dx, B, C, H, W, X.p, X.ld, 0, c.stream, c.bf16));
        }
        body(c, X, Y);
        if (!c.dry) BRN_HIP(launch_nhwc_to_nchw(Y.p, B, O, Ho, Wo, Y.ld, 0, dy, c.stream, c.bf16));
    }, s16);
}

}  // namespace

extern "C" {

brn_status brn_set_op_compute(int dtype) {
    return guarded([&] {
        if (dtype == BRN_BF16_DEC_SPLIT2) fail(BRN_ERR_INVALID_ARG, "unsupported compute dtype %d", dtype);   // a mode of whole models only
        g_op = compute_mode(dtype).build;
    });
}

// ---- stand-alone SwinTransformer -----------------------------------------------------------------------------------------
brn_status brn_swin_create(const brn_config* cfg, const brn_named_tensor* weights, size_t n, const char* prefix, int device,
                           brn_swin** out) {
    return guarded([&] {
        if (!cfg || !weights || !out) fail(BRN_ERR_INVALID_ARG, "null argument");
        *out = nullptr;
        ensure_device(device);
        std::unique_ptr<brn_swin> h(new brn_swin());
        h->cfg = *cfg; h->device = device;
        WeightTable wt(weights, n);
        const WeightBuild wb = g_op;
        h->bf16 = op_s16(wb);
        build_swin_weights(wt, prefix ? prefix : "", *cfg, h->own, wb, h->w);
        *out = h.release();
    });
}
void brn_swin_destroy(brn_swin* s) {
    if (!s) return;
    (void)hipSetDevice(s->device);
    (void)hipDeviceSynchronize();
    delete s;
}
brn_status brn_swin_forward(brn_swin* s, const float* x, int B, int H, int W, brn_mem in_loc, float* const outs[4],
                            brn_mem out_loc, void* stream) {
    return guarded([&] {
        if (!s) fail(BRN_ERR_INVALID_ARG, "null handle");
        std::lock_guard<std::mutex> lk(s->mu);
        swin_entry(s->w, s->device, x, B, H, W, in_loc, outs, out_loc, stream, s->bf16);
    });
}

brn_status brn_linear_forward(const float* x, int M, int K, const float* w, const float* bias, int N, int act,
                              const float* residual, float* y, brn_mem loc, int device, void* stream) {
    return guarded([&] {
        if (!x || !w || !y || M < 1 || N < 1 || K < 1) fail(BRN_ERR_INVALID_ARG, "bad argument");
        ensure_device(device);
        DeviceOwner own;
        const WeightBuild wb = g_op;
        GemmW g = make_linear(own, wb, w, bias, N, K);
        g.act = act;
        Staging st(stream, loc);
        const float* dx = st.in(x, (size_t)M * K);
        const float* dr = residual ? st.in(residual, (size_t)M * N) : nullptr;
        float* dy = st.out(y, (size_t)M * N);
        const int s16 = op_s16(wb);            // then the product runs on kernels/gemm_bf16.hip; y (and the residual) stay fp32
        with_arena((hipStream_t)stream, [&](Ctx& c) {
            const float* a = s16 ? round_to_s16(c, dx, (size_t)M * K, wb.f16) : dx;
            run_gemm(c, g, GemmIO(a, M, K).to(dy, N).add(dr, N).f32(s16 ? 1 : 0, s16 ? 1 : 0));
        }, s16);
        st.finish();
    });
}

brn_status brn_linear_residual_layer_norm_forward(const float* x, int M, int K, const float* w, const float* bias, int N, const float* residual,
                                                  const float* gamma, const float* beta, float eps, float* x_out, float* y_out, brn_mem loc,
                                                  int device, void* stream) {
    return guarded([&] {
        if (!x || !w || !residual || !gamma || !beta || !x_out || !y_out || M < 1 || N < 1 || K < 1) fail(BRN_ERR_INVALID_ARG, "bad argument");
        if (N % 4 || N > 3072) fail(BRN_ERR_INVALID_ARG, "layer_norm width %d unsupported (multiple of 4, <= 3072)", N);
        if (eps != 1e-5f) fail(BRN_ERR_INVALID_ARG, "the fused projection + LayerNorm kernels are built for eps = 1e-5 (swin.rs:333-335)");
        ensure_device(device);
        DeviceOwner own;
        const WeightBuild wb = g_op;
        GemmW g = make_linear(own, wb, w, bias, N, K);
        LNW ln; ln.C = N; ln.g = own.upload(gamma, N); ln.b = own.upload(beta, N);
        Staging st(stream, loc);
        const float* dx = st.in(x, (size_t)M * K);
        const float* dr = st.in(residual, (size_t)M * N);
        float* dxo = st.out(x_out, (size_t)M * N);
        float* dyo = st.out(y_out, (size_t)M * N);
        const bool bf = wb.planes == BUILD_BF16;
        with_arena((hipStream_t)stream, [&](Ctx& c) {
            const float* a = bf ? round_to_s16(c, dx, (size_t)M * K, wb.f16) : dx;
            float* yb = bf ? c.arena->alloc_bytes((size_t)M * N * 2) : dyo;     // y produced as a 16-bit matrix and widened
            // the residual stream is updated in place inside the model: here x_out starts as a copy of the residual
            if (!c.dry) BRN_HIP(hipMemcpyAsync(dxo, dr, (size_t)M * N * sizeof(float), hipMemcpyDeviceToDevice, c.stream));
            if (!linear_residual_ln(c, g, a, M, K, dxo, ln, yb, N, true)) {
                // split modes: the GEMM's raw split-K slices summed by the LayerNorm, where the planner cuts (brn_gemm_ln.cpp)
                const GemmIO io = GemmIO(a, M, K).to(dxo, N).add(dxo, N).f32(bf ? 1 : 0, bf ? 1 : 0);
                const LnOut yo = LnOut(yb, N).s16(bf ? 1 : 0);
                if (!(g_gemm_ln_route && g_gemm_ln_route(c, g, io, ln, yo))) {
                    run_gemm(c, g, io);
                    run_layernorm(c, ln, dxo, M, N, yo);
                }
            }
            if (bf && !c.dry) BRN_HIP(launch_bf16_to_f32(yb, (size_t)M * N, dyo, c.stream, wb.f16));
        }, op_s16(wb));
        st.finish();
    });
}

brn_status brn_layer_norm_forward(const float* x, int rows, int C, const float* gamma, const float* beta, float eps, float* y,
                                  brn_mem loc, int device, void* stream) {
    return guarded([&] {
        if (!x || !gamma || !beta || !y || rows < 1) fail(BRN_ERR_INVALID_ARG, "bad argument");
        if (C % 4 || C > 3072) fail(BRN_ERR_INVALID_ARG, "layer_norm width %d unsupported (multiple of 4, <= 3072)", C);
        ensure_device(device);
        DeviceOwner own;
        LNW ln; ln.C = C; ln.g = own.upload(gamma, C); ln.b = own.upload(beta, C);
        Staging st(stream, loc);
        const float* dx = st.in(x, (size_t)rows * C);
        float* dy = st.out(y, (size_t)rows * C);
        LayerNormParams p{};
        p.x = dx; p.y = dy; p.rows = rows; p.C = C; p.gamma = ln.g; p.beta = ln.b; p.eps = eps; p.ldx = C; p.ldy = C;
        BRN_HIP(launch_layernorm(p, (hipStream_t)stream));
        BRN_HIP(hipStreamSynchronize((hipStream_t)stream));
        st.finish();
    });
}

brn_status brn_conv2d_forward(const float* x, int B, int C, int H, int W, const float* w, const float* bias, int O, int kh,
                              int kw, int stride, int pad, int dil, const float* bn_g, const float* bn_b, const float* bn_m,
                              const float* bn_v, float bn_eps, int act, float* y, brn_mem loc, int device, void* stream) {
    return guarded([&] {
        if (!x || !w || !y || B < 1 || C < 1 || O < 1 || kh < 1 || kw < 1 || stride < 1 || dil < 1 || pad < 0)
            fail(BRN_ERR_INVALID_ARG, "bad argument");
        const int Ho = (H + 2 * pad - dil * (kh - 1) - 1) / stride + 1, Wo = (W + 2 * pad - dil * (kw - 1) - 1) / stride + 1;
        if (Ho < 1 || Wo < 1) fail(BRN_ERR_INVALID_ARG, "empty conv output");
        ensure_device(device);
        DeviceOwner own;
        const WeightBuild wb = g_op;
        const bool nhwc = (C % 32) == 0;
        GemmW g = nhwc ? make_conv_nhwc(own, wb, w, nullptr, O, C, C, kh, kw, stride, pad, dil)
                       : make_conv_gather(own, w, nullptr, O, C, kh, kw, stride, pad, dil);
        if (bn_g) fold_bn(own, g, bias, bn_g, bn_b, bn_m, bn_v, bn_eps);
        else if (bias) g.bias = own.upload(bias, O);
        g.act = act;
        Staging st(stream, loc);
        const float* dx = st.in(x, (size_t)B * C * H * W);
        float* dy = st.out(y, (size_t)B * O * Ho * Wo);
        if (nhwc)            // bf16 mode (from 64 channels on): bf16 map in, bf16 map out, like inside the model
            through_nhwc(stream, op_s16(wb, C >= 64), dx, B, C, C, H, W, dy, O, Ho, Wo, [&](Ctx& c, const Map& X, const Map& Y) { run_conv(c, g, X, Y); });
        else
            with_arena((hipStream_t)stream, [&](Ctx& c) {
                Map Y = new_map(c, B, Ho, Wo, O);
                run_conv_nchw(c, g, dx, B, H, W, Y);
                if (!c.dry) BRN_HIP(launch_nhwc_to_nchw(Y.p, B, O, Ho, Wo, Y.ld, 0, dy, c.stream, c.bf16));
            });
        st.finish();
    });
}

brn_status brn_upsample_bilinear2d(const float* x, int B, int C, int H, int W, int oh, int ow, float* y, brn_mem loc,
                                   int device, void* stream) {
    return guarded([&] {
        if (!x || !y || B < 1 || C < 1 || H < 1 || W < 1 || oh < 1 || ow < 1) fail(BRN_ERR_INVALID_ARG, "bad argument");
        ensure_device(device);
        Staging st(stream, loc);
        const float* dx = st.in(x, (size_t)B * C * H * W);
        float* dy = st.out(y, (size_t)B * C * oh * ow);
        BRN_HIP(launch_resize_nchw(dx, B * C, H, W, dy, oh, ow, (hipStream_t)stream));
        BRN_HIP(hipStreamSynchronize((hipStream_t)stream));
        st.finish();
    });
}

brn_status brn_window_attention_forward(const float* x, int B, int H, int W, int C, int heads, int window_size, int shift,
                                        const float* qkv_w, const float* qkv_b, const float* proj_w, const float* proj_b,
                                        const float* rel_table, float* y, brn_mem loc, int device, void* stream) {
    return guarded([&] {
        if (!x || !qkv_w || !qkv_b || !proj_w || !proj_b || !rel_table || !y) fail(BRN_ERR_INVALID_ARG, "null argument");
        if (window_size < 2 || window_size > 32) fail(BRN_ERR_INVALID_ARG, "window attention: window_size %d unsupported (2 <= window_size <= 32)", window_size);
        if (!(shift == 0 || shift == window_size / 2))
            fail(BRN_ERR_INVALID_ARG, "window attention: shift %d unsupported (shift must be 0 or window_size / 2 = %d; 2 <= window_size <= 32)", shift, window_size / 2);
        if (B < 1 || H < 1 || W < 1 || heads < 1 || C != heads * 32) fail(BRN_ERR_INVALID_ARG, "window attention needs B, H, W >= 1 and head_dim 32 (C == heads * 32)");
        ensure_device(device);
        DeviceOwner own;
        // reuse the model's weight builder through a one-block table
        const int T = (2 * window_size - 1) * (2 * window_size - 1);
        SwinBlockW bk;
        bk.heads = heads;
        const WeightBuild wb = g_op;
        bk.qkv = make_linear(own, wb, qkv_w, qkv_b, 3 * C, C);
        bk.proj = make_linear(own, wb, proj_w, proj_b, C, C);
        {
            std::vector<float> tt((size_t)T * heads);
            for (int t = 0; t < T; ++t) for (int h = 0; h < heads; ++h) tt[(size_t)h * T + t] = rel_table[(size_t)t * heads + h];
            bk.rel_table = own.upload(tt);
        }
        Staging st(stream, loc);
        const float* dx = st.in(x, (size_t)B * H * W * C);
        float* dy = st.out(y, (size_t)B * H * W * C);
        // compute mode BRN_BF16 at op level: x is rounded to bf16 at the edge (inside the model LayerNorm writes it as bf16), qkv and
        // the attention output are bf16 matrices (window_attention_bf16_kernel), y = proj(...) stays fp32 like the residual stream
        const int s16 = op_s16(wb);
        with_arena((hipStream_t)stream, [&](Ctx& c) {
            const float* xn = s16 ? round_to_s16(c, dx, (size_t)B * H * W * C, wb.f16) : dx;
            swin_attention(c, bk, xn, B, H, W, C, shift, dy, nullptr, window_size);
        }, s16);
        st.finish();
    });
}

brn_status brn_attention_forward(const float* q, const float* k, const float* v, int batch, int heads, int N, int head_dim,
                                 const float* bias, int n_bias, float scale, float* y, brn_mem loc, int device, void* stream) {
    return guarded([&] {
        if (!q || !k || !v || !y) fail(BRN_ERR_INVALID_ARG, "attention: null q, k, v or y");
        if (head_dim != 32) fail(BRN_ERR_INVALID_ARG, "attention: head_dim %d unsupported (head_dim must be 32)", head_dim);
        if (N < 1 || N > 144) fail(BRN_ERR_INVALID_ARG, "attention: sequence length N = %d unsupported (1 <= N <= 144)", N);
        if (batch < 1 || heads < 1 || (long long)batch * heads > 0x7fffffffLL)
            fail(BRN_ERR_INVALID_ARG, "attention: batch %d, heads %d unsupported (batch >= 1, heads >= 1, batch * heads < 2^31)", batch, heads);
        if (n_bias < 0) fail(BRN_ERR_INVALID_ARG, "attention: n_bias %d is negative (n_bias >= 0)", n_bias);
        if ((bias == nullptr) != (n_bias == 0)) fail(BRN_ERR_INVALID_ARG, "attention: bias must be NULL exactly when n_bias == 0 (n_bias %d)", n_bias);
        if (n_bias > 0 && batch % n_bias) fail(BRN_ERR_INVALID_ARG, "attention: batch %d is not a multiple of n_bias %d (batch %% n_bias == 0)", batch, n_bias);
        if (!scale_arg_ok(scale)) fail(BRN_ERR_INVALID_ARG, "attention: scale must be finite and >= 0 (0 = head_dim^-0.5)");
        const size_t n = (size_t)batch * heads * N * head_dim, nb = (size_t)n_bias * heads * N * N;
        if (floats_overlap(q, n, y, n) || floats_overlap(k, n, y, n) || floats_overlap(v, n, y, n) || floats_overlap(bias, nb, y, n))
            fail(BRN_ERR_INVALID_ARG, "attention: y must not alias an input");
        if (loc == BRN_MEM_DEVICE && !all_aligned16({q, k, v, y})) fail(BRN_ERR_INVALID_ARG, "attention: device q, k, v and y must be 16-byte aligned");
        ensure_device(device);
        Staging st(stream, loc);
        AttentionBiasParams p{};
        p.q = st.in(q, n); p.k = st.in(k, n); p.v = st.in(v, n);
        p.bias = bias ? st.in(bias, nb) : nullptr;
        p.y = st.out(y, n);
        p.batch = batch; p.heads = heads; p.N = N; p.n_bias = n_bias;
        p.scale = scale_or_default(scale, head_dim);
        p.s16 = attention_op_s16();
        BRN_HIP(launch_attention_bias(p, (hipStream_t)stream));
        st.finish();
    });
}

// brn_flash_attention_forward, brn_flash_attention_bias_forward, brn_flash_attention_gqa_forward and brn_flash_attention_splitkv_forward
// (brn_flash_attention_paged_forward takes the size checks):
// one set of checks, one way to fill the kernels' arguments.  who = the message prefix; with_bias = an entry with a bias, whose bias /
// n_bias are checked (the bias-free entries pass null / 0); gqa = a grouped entry, whose kv_heads is checked (the other two pass heads)
// and whose causal mask ends at the last key.
// the sizes alone (what brn_flash_attention_splitkv_plan can check too)
static void flash_attention_check_sizes(const char* who, bool gqa, int batch, int seq_q, int seq_kv, int heads, int kv_heads, int head_dim) {
    if (!(head_dim == 32 || head_dim == 64 || head_dim == 128))
        fail(BRN_ERR_INVALID_ARG, "%s: head_dim %d unsupported (head_dim must be 32, 64 or 128)", who, head_dim);
    if (seq_q < 1 || seq_q > 65536 || seq_kv < 1 || seq_kv > 65536)
        fail(BRN_ERR_INVALID_ARG, "%s: seq_q %d, seq_kv %d unsupported (1 <= seq_q, seq_kv <= 65536)", who, seq_q, seq_kv);
    if (batch < 1 || heads < 1) fail(BRN_ERR_INVALID_ARG, "%s: batch %d, heads %d unsupported (batch >= 1, heads >= 1)", who, batch, heads);
    if (gqa) {
        if (kv_heads < 1 || kv_heads > heads || heads % kv_heads)
            fail(BRN_ERR_INVALID_ARG, "%s: kv_heads %d unsupported with heads %d (1 <= kv_heads <= heads, heads %% kv_heads == 0)", who, kv_heads, heads);
        // the grid: a workgroup per (batch entry, K / V head, 64 packed rows of the group's G * seq_q)
        const long long rows = (long long)(heads / kv_heads) * seq_q;
        if (rows > 0x7fffffffLL || (long long)batch * kv_heads * ((rows + 63) / 64) > 0x7fffffffLL)
            fail(BRN_ERR_INVALID_ARG, "%s: batch %d, heads %d, kv_heads %d, seq_q %d too large (G = heads / kv_heads, G * seq_q < 2^31, batch * kv_heads * ceil(G * seq_q / 64) < 2^31)",
                 who, batch, heads, kv_heads, seq_q);
    } else if ((long long)batch * heads * ((seq_q + 15) / 16) > 0x7fffffffLL)
        fail(BRN_ERR_INVALID_ARG, "%s: batch %d, heads %d, seq_q %d too large (batch * heads * ceil(seq_q / 16) < 2^31)", who, batch, heads, seq_q);
}
// every check of the three older entries, in their order; nothing here touches the device
static void flash_attention_check(const char* who, bool with_bias, bool gqa, const float* q, const float* k, const float* v, int batch, int seq_q,
                                  int seq_kv, int heads, int kv_heads, int head_dim, int layout, int causal, const float* bias, int n_bias,
                                  float scale, const float* y, brn_mem loc) {
    if (!q || !k || !v || !y) fail(BRN_ERR_INVALID_ARG, "%s: null q, k, v or y", who);
    flash_attention_check_sizes(who, gqa, batch, seq_q, seq_kv, heads, kv_heads, head_dim);
    if (layout != BRN_ATTN_BSHD && layout != BRN_ATTN_BHSD) fail(BRN_ERR_INVALID_ARG, "%s: layout %d unknown (layout must be 0 = BSHD or 1 = BHSD)", who, layout);
    if (causal != 0 && causal != 1) fail(BRN_ERR_INVALID_ARG, "%s: causal %d (causal must be 0 or 1)", who, causal);
    if (causal && gqa && seq_kv < seq_q) fail(BRN_ERR_INVALID_ARG, "%s: causal requires seq_kv >= seq_q (seq_q %d, seq_kv %d)", who, seq_q, seq_kv);
    if (causal && !gqa && seq_q != seq_kv) fail(BRN_ERR_INVALID_ARG, "%s: causal requires seq_q == seq_kv (seq_q %d, seq_kv %d)", who, seq_q, seq_kv);
    if (with_bias) {
        if (n_bias < 0) fail(BRN_ERR_INVALID_ARG, "%s: n_bias %d is negative (n_bias >= 0)", who, n_bias);
        if ((bias == nullptr) != (n_bias == 0)) fail(BRN_ERR_INVALID_ARG, "%s: bias must be NULL exactly when n_bias == 0 (n_bias %d)", who, n_bias);
        if (n_bias > 0 && batch % n_bias) fail(BRN_ERR_INVALID_ARG, "%s: batch %d is not a multiple of n_bias %d (batch %% n_bias == 0)", who, batch, n_bias);
    }
    if (!scale_arg_ok(scale)) fail(BRN_ERR_INVALID_ARG, "%s: scale must be finite and >= 0 (0 = head_dim^-0.5)", who);
    const size_t nq = (size_t)batch * heads * seq_q * head_dim, nkv = (size_t)batch * kv_heads * seq_kv * head_dim;
    const size_t nb = (size_t)n_bias * heads * seq_q * seq_kv;
    if (floats_overlap(q, nq, y, nq) || floats_overlap(k, nkv, y, nq) || floats_overlap(v, nkv, y, nq))
        fail(BRN_ERR_INVALID_ARG, "%s: y must not overlap an input", who);
    if (bias && floats_overlap(bias, nb, y, nq)) fail(BRN_ERR_INVALID_ARG, "%s: y must not overlap the bias", who);
    if (loc == BRN_MEM_DEVICE && !all_aligned16({q, k, v, y})) fail(BRN_ERR_INVALID_ARG, "%s: device q, k, v and y must be 16-byte aligned", who);
    if (loc == BRN_MEM_DEVICE && bias && !all_aligned16({bias})) fail(BRN_ERR_INVALID_ARG, "%s: device bias must be 16-byte aligned", who);
}
// the kernels' arguments of a checked call: operands through st, strides of the layout, mask, scale, arithmetic
static FlashAttentionParams flash_attention_params(Staging& st, const float* q, const float* k, const float* v, int batch, int seq_q, int seq_kv, int heads,
                                                   int kv_heads, int head_dim, int layout, int causal, const float* bias, int n_bias, float scale, float* y) {
    const size_t nq = (size_t)batch * heads * seq_q * head_dim, nkv = (size_t)batch * kv_heads * seq_kv * head_dim;
    const size_t nb = (size_t)n_bias * heads * seq_q * seq_kv;
    FlashAttentionParams p{};
    p.q = st.in(q, nq); p.k = st.in(k, nkv); p.v = st.in(v, nkv);
    if (bias) {
        p.bias = st.in(bias, nb); p.n_bias = n_bias;
        p.b_sh = (long)seq_q * seq_kv; p.b_sp = heads * p.b_sh;     // heads-major whatever the layout
    }
    p.y = st.out(y, nq);
    p.batch = batch; p.heads = heads; p.kv_heads = kv_heads; p.seq_q = seq_q; p.seq_kv = seq_kv; p.head_dim = head_dim;
    // one kernel for both layouts: element strides of (batch entry, head, sequence position); k and v have kv_heads heads
    const long d = head_dim;
    if (layout == BRN_ATTN_BSHD) {
        p.q_ss = heads * d; p.q_sh = d; p.q_sb = seq_q * p.q_ss;
        p.kv_ss = kv_heads * d; p.kv_sh = d; p.kv_sb = seq_kv * p.kv_ss;
    } else {
        p.q_ss = d; p.q_sh = seq_q * d; p.q_sb = heads * p.q_sh;
        p.kv_ss = d; p.kv_sh = seq_kv * d; p.kv_sb = kv_heads * p.kv_sh;
    }
    p.causal = causal;
    p.causal_off = causal ? seq_kv - seq_q : 0;
    p.scale = scale_or_default(scale, head_dim);
    p.s16 = attention_op_s16();
    return p;
}
static void flash_attention_body(const char* who, bool with_bias, bool gqa, const float* q, const float* k, const float* v, int batch, int seq_q,
                                 int seq_kv, int heads, int kv_heads, int head_dim, int layout, int causal, const float* bias, int n_bias,
                                 float scale, float* y, brn_mem loc, int device, void* stream) {
    flash_attention_check(who, with_bias, gqa, q, k, v, batch, seq_q, seq_kv, heads, kv_heads, head_dim, layout, causal, bias, n_bias, scale, y, loc);
    ensure_device(device);
    Staging st(stream, loc);
    const FlashAttentionParams p = flash_attention_params(st, q, k, v, batch, seq_q, seq_kv, heads, kv_heads, head_dim, layout, causal, bias, n_bias, scale, y);
    BRN_HIP(launch_flash_attention(p, (hipStream_t)stream));
    st.finish();
}

brn_status brn_flash_attention_forward(const float* q, const float* k, const float* v, int batch, int seq_q, int seq_kv, int heads, int head_dim,
                                       int layout, int causal, float scale, float* y, brn_mem loc, int device, void* stream) {
    return guarded([&] {
        flash_attention_body("flash attention", false, false, q, k, v, batch, seq_q, seq_kv, heads, heads, head_dim, layout, causal, nullptr, 0, scale, y, loc, device, stream);
    });
}

brn_status brn_flash_attention_bias_forward(const float* q, const float* k, const float* v, int batch, int seq_q, int seq_kv, int heads, int head_dim,
                                            int layout, int causal, const float* bias, int n_bias, float scale, float* y, brn_mem loc, int device,
                                            void* stream) {
    return guarded([&] {
        flash_attention_body("flash attention bias", true, false, q, k, v, batch, seq_q, seq_kv, heads, heads, head_dim, layout, causal, bias, n_bias, scale, y, loc, device, stream);
    });
}

brn_status brn_flash_attention_gqa_forward(const float* q, const float* k, const float* v, int batch, int seq_q, int seq_kv, int heads, int kv_heads,
                                           int head_dim, int layout, int causal, const float* bias, int n_bias, float scale, float* y, brn_mem loc,
                                           int device, void* stream) {
    return guarded([&] {
        flash_attention_body("flash attention gqa", true, true, q, k, v, batch, seq_q, seq_kv, heads, kv_heads, head_dim, layout, causal, bias, n_bias, scale, y, loc, device, stream);
    });
}

// The packed batch.  Everything the kernels read from the cu arrays reaches them through the record table of brn_flash_varlen_plan.h,
// built here from values that passed flash_varlen_check.  The table travels through a Staging temporary: the stream is synchronised
// before the call returns (also for device tensors), so the table and its host copy are free to go when it does.
brn_status brn_flash_attention_varlen_forward(const float* q, const float* k, const float* v, const int* cu_seqlens_q, const int* cu_seqlens_kv,
                                              int n_seqs, int heads, int kv_heads, int head_dim, int window_left, int window_right, float scale,
                                              float* y, brn_mem loc, int device, void* stream) {
    return guarded([&] {
        const char* who = "flash attention varlen";
        if (!q || !k || !v || !y) fail(BRN_ERR_INVALID_ARG, "%s: null q, k, v or y", who);
        if (!cu_seqlens_q || !cu_seqlens_kv) fail(BRN_ERR_INVALID_ARG, "%s: null cu_seqlens_q or cu_seqlens_kv", who);
        if (!(head_dim == 32 || head_dim == 64 || head_dim == 128))
            fail(BRN_ERR_INVALID_ARG, "%s: head_dim %d unsupported (head_dim must be 32, 64 or 128)", who, head_dim);
        if (heads < 1) fail(BRN_ERR_INVALID_ARG, "%s: heads %d unsupported (heads >= 1)", who, heads);
        if (kv_heads < 1 || kv_heads > heads || heads % kv_heads)
            fail(BRN_ERR_INVALID_ARG, "%s: kv_heads %d unsupported with heads %d (1 <= kv_heads <= heads, heads %% kv_heads == 0)", who, kv_heads, heads);
        if (n_seqs < 1) fail(BRN_ERR_INVALID_ARG, "%s: n_seqs %d unsupported (n_seqs >= 1)", who, n_seqs);
        if (window_left < -1 || window_right < -1)
            fail(BRN_ERR_INVALID_ARG, "%s: window (%d, %d) unsupported (window_left >= -1, window_right >= -1; -1 = unbounded)", who, window_left, window_right);
        if (!scale_arg_ok(scale)) fail(BRN_ERR_INVALID_ARG, "%s: scale must be finite and >= 0 (0 = head_dim^-0.5)", who);
        // a side that reaches past the longest sequence allowed is that side at 65536 (INT_MAX as "unbounded" included): clamped here,
        // before the plan and the kernels, whose int arithmetic on it then cannot wrap
        window_left = fa_varlen_clamp_window(window_left); window_right = fa_varlen_clamp_window(window_right);
        const std::string bad = flash_varlen_check(cu_seqlens_q, cu_seqlens_kv, n_seqs, heads, kv_heads, window_left, window_right);
        if (!bad.empty()) fail(BRN_ERR_INVALID_ARG, "%s: %s", who, bad.c_str());
        const size_t nq = (size_t)cu_seqlens_q[n_seqs] * heads * head_dim, nkv = (size_t)cu_seqlens_kv[n_seqs] * kv_heads * head_dim;
        if (floats_overlap(q, nq, y, nq) || floats_overlap(k, nkv, y, nq) || floats_overlap(v, nkv, y, nq))
            fail(BRN_ERR_INVALID_ARG, "%s: y must not overlap an input", who);
        if (loc == BRN_MEM_DEVICE && !all_aligned16({q, k, v, y})) fail(BRN_ERR_INVALID_ARG, "%s: device q, k, v and y must be 16-byte aligned", who);
        ensure_device(device);
        const std::vector<FaVarlenRecord> recs = flash_varlen_plan(cu_seqlens_q, cu_seqlens_kv, n_seqs, heads, kv_heads, window_left, window_right);
        Staging st(stream, loc);                 // after recs: its destructor synchronises the stream before recs goes
        FlashAttentionParams p{};
        p.q = st.in(q, nq); p.k = st.in(k, nkv); p.v = st.in(v, nkv);
        p.y = st.out(y, nq);
        static_assert(sizeof(FaVarlenRecord) == 8 * sizeof(float), "a record is 8 dwords");
        float* dplan = st.dalloc(recs.size() * 8);
        BRN_HIP(hipMemcpyAsync(dplan, recs.data(), recs.size() * sizeof(FaVarlenRecord), hipMemcpyHostToDevice, (hipStream_t)stream));
        p.plan = reinterpret_cast<const FaVarlenRecord*>(dplan);
        p.n_records = (int)recs.size();
        p.batch = 1; p.heads = heads; p.kv_heads = kv_heads; p.head_dim = head_dim;
        p.seq_q = p.seq_kv = 1;                  // each workgroup's own, from its record
        const long d = head_dim;
        p.q_ss = heads * d; p.q_sh = d; p.kv_ss = kv_heads * d; p.kv_sh = d;
        p.window_left = window_left; p.window_right = window_right;
        p.scale = scale_or_default(scale, head_dim);
        p.s16 = attention_op_s16();
        BRN_HIP(launch_flash_attention(p, (hipStream_t)stream));
        st.finish();
    });
}

// The split over keys.  brn_flash_split_plan.h decides S and tps for both entries below, from the integers alone; the checks the gqa entry
// makes without a bias are flash_attention_check's, under this entry's prefix.
static const char* const SPLITKV = "flash attention splitkv";
static void splitkv_check_splits(const char* who, int kv_splits) {
    if (kv_splits < 0 || kv_splits > FA_SPLIT_MAX)
        fail(BRN_ERR_INVALID_ARG, "%s: kv_splits %d unsupported (0 <= kv_splits <= %d; 0 = the library's rule)", who, kv_splits, FA_SPLIT_MAX);
}
static FaSplitPlan splitkv_plan_checked(const char* who, int batch, int seq_q, int seq_kv, int heads, int kv_heads, int head_dim, int kv_splits) {
    const FaSplitPlan pl = flash_split_plan(batch, seq_q, seq_kv, heads, kv_heads, head_dim, kv_splits);
    if (pl.base * pl.S > 0x7fffffffLL)
        fail(BRN_ERR_INVALID_ARG, "%s: %lld workgroups x %d splits too large (batch * kv_heads * ceil(G * seq_q / 64) * S < 2^31)", who, pl.base, pl.S);
    return pl;
}
brn_status brn_flash_attention_splitkv_plan(int batch, int seq_q, int seq_kv, int heads, int kv_heads, int head_dim, int kv_splits, int* splits_out,
                                            int* tiles_per_split_out, size_t* workspace_floats_out) {
    return guarded([&] {
        flash_attention_check_sizes(SPLITKV, true, batch, seq_q, seq_kv, heads, kv_heads, head_dim);
        splitkv_check_splits(SPLITKV, kv_splits);
        const FaSplitPlan pl = splitkv_plan_checked(SPLITKV, batch, seq_q, seq_kv, heads, kv_heads, head_dim, kv_splits);
        if (splits_out) *splits_out = pl.S;
        if (tiles_per_split_out) *tiles_per_split_out = pl.tps;
        if (workspace_floats_out) *workspace_floats_out = pl.workspace_floats;
    });
}

brn_status brn_flash_attention_splitkv_forward(const float* q, const float* k, const float* v, int batch, int seq_q, int seq_kv, int heads, int kv_heads,
                                               int head_dim, int layout, int causal, float scale, int kv_splits, float* y, float* lse, float* workspace,
                                               size_t workspace_floats, brn_mem loc, int device, void* stream) {
    return guarded([&] {
        const char* who = SPLITKV;
        // what the plan entry checks first (a buffer size below means something only once the sizes and the splits are sound), then
        // every check of the gqa entry without a bias
        flash_attention_check_sizes(who, true, batch, seq_q, seq_kv, heads, kv_heads, head_dim);
        splitkv_check_splits(SPLITKV, kv_splits);
        const FaSplitPlan pl = splitkv_plan_checked(SPLITKV, batch, seq_q, seq_kv, heads, kv_heads, head_dim, kv_splits);
        flash_attention_check(who, false, true, q, k, v, batch, seq_q, seq_kv, heads, kv_heads, head_dim, layout, causal, nullptr, 0, scale, y, loc);
        const size_t nq = (size_t)batch * heads * seq_q * head_dim, nkv = (size_t)batch * kv_heads * seq_kv * head_dim;
        const size_t R = (size_t)batch * heads * seq_q;
        // the partials are written, and only they: the workspace counts for what the call needs of it, nothing when S == 1
        const size_t need = pl.S > 1 ? pl.workspace_floats : 0;
        if (need && (!workspace || workspace_floats < need))
            fail(BRN_ERR_INVALID_ARG, "%s: workspace %s for %d splits (it must hold S * batch * heads * seq_q * (head_dim + 1) = %zu floats, workspace_floats %zu)",
                 who, workspace ? "too small" : "is NULL", pl.S, need, workspace_floats);
        float* const ws = need ? workspace : nullptr;
        const struct { const float* p; size_t n; const char* name; } outs[] = {{y, nq, "y"}, {lse, lse ? R : 0, "lse"}, {ws, need, "workspace"}};
        for (int a = 1; a < 3; ++a) {
            if (!outs[a].p) continue;
            if (floats_overlap(q, nq, outs[a].p, outs[a].n) || floats_overlap(k, nkv, outs[a].p, outs[a].n) || floats_overlap(v, nkv, outs[a].p, outs[a].n))
                fail(BRN_ERR_INVALID_ARG, "%s: %s must not overlap an input", who, outs[a].name);
            for (int b = 0; b < a; ++b)
                if (outs[b].p && floats_overlap(outs[b].p, outs[b].n, outs[a].p, outs[a].n))
                    fail(BRN_ERR_INVALID_ARG, "%s: %s and %s must not overlap", who, outs[b].name, outs[a].name);
        }
        if (loc == BRN_MEM_DEVICE && !all_aligned16({lse, ws})) fail(BRN_ERR_INVALID_ARG, "%s: device lse and workspace must be 16-byte aligned", who);
        ensure_device(device);
        Staging st(stream, loc);
        FlashAttentionParams p = flash_attention_params(st, q, k, v, batch, seq_q, seq_kv, heads, kv_heads, head_dim, layout, causal, nullptr, 0, scale, y);
        p.kv_splits = pl.S; p.tiles_per_split = pl.tps;
        if (lse) p.lse = st.out(lse, R);
        if (need) {
            p.o_part = st.out(ws, need);
            p.lse2_part = p.o_part + (size_t)pl.S * R * head_dim;
        }
        BRN_HIP(launch_flash_attention(p, (hipStream_t)stream));
        st.finish();
    });
}

// The split over keys with K / V in the pages of a pool and per-sequence lengths on the device.  The plan is the split entry's at
// seq_kv = max_kv_len.  block_table and kv_lens are never read on the host for BRN_MEM_DEVICE: nothing here depends on their content, and
// the call allocates nothing and does not synchronise (Staging has nothing to stage), so it may be captured into a graph.
// One body for brn_flash_attention_paged_forward (kv_type BRN_KV_F32) and brn_flash_attention_paged_kv_forward: the pool's element size is
// the only thing that differs on the host, so the overlap checks count bytes.  brn_flash_attention_paged_fp8_forward (fp8 = true: an
// e4m3fn pool of bytes, FA_KV_FP8 to the launcher, never a brn_kv_type) adds the two scale arrays, which are inputs like the table.
static const char* const KV_TYPE_NAME[3] = {"f32", "bf16", "f16"};
static size_t kv_type_bytes(int kv_type) { return kv_type == BRN_KV_F32 ? 4 : kv_type == FA_KV_FP8 ? 1 : 2; }
static void kv_type_check(const char* who, int kv_type) {
    if (kv_type != BRN_KV_F32 && kv_type != BRN_KV_BF16 && kv_type != BRN_KV_F16)
        fail(BRN_ERR_INVALID_ARG, "%s: kv_type %d unknown (kv_type must be 0 = f32, 1 = bf16 or 2 = f16)", who, kv_type);
}
// page_size 16 .. 256, a power of two; n_pages, max_pages >= 1; n_pages * page_size < 2^31 -> log2(page_size)
static int paged_pool_check(const char* who, int n_pages, int page_size, int max_pages) {
    int page_log2 = 0;
    while ((1 << page_log2) < page_size && page_log2 < 9) ++page_log2;
    if (page_size < 16 || page_size > 256 || (1 << page_log2) != page_size)
        fail(BRN_ERR_INVALID_ARG, "%s: page_size %d unsupported (page_size must be 16, 32, 64, 128 or 256)", who, page_size);
    if (n_pages < 1 || max_pages < 1) fail(BRN_ERR_INVALID_ARG, "%s: n_pages %d, max_pages %d unsupported (n_pages >= 1, max_pages >= 1)", who, n_pages, max_pages);
    if ((long long)n_pages * page_size > 0x7fffffffLL)
        fail(BRN_ERR_INVALID_ARG, "%s: n_pages %d of page_size %d too large (n_pages * page_size < 2^31)", who, n_pages, page_size);
    return page_log2;
}
static void flash_attention_paged_body(const char* who, const float* q, const void* k_pages, const void* v_pages, int kv_type, bool fp8, const float* k_scale,
                                       const float* v_scale, const int* block_table,
                                       const int* kv_lens, int batch, int seq_q, int max_kv_len, int heads, int kv_heads, int head_dim, int n_pages,
                                       int page_size, int max_pages, int layout, int causal, float scale, int kv_splits, float* y, float* lse,
                                       float* workspace, size_t workspace_floats, brn_mem loc, int device, void* stream) {
    if (!q || !k_pages || !v_pages || !y) fail(BRN_ERR_INVALID_ARG, "%s: null q, k_pages, v_pages or y", who);
    if (!block_table || !kv_lens) fail(BRN_ERR_INVALID_ARG, "%s: null block_table or kv_lens", who);
    if (fp8) kv_type = FA_KV_FP8;
    else kv_type_check(who, kv_type);
    const int s16 = attention_op_s16();
    if (!fp8 && kv_type != BRN_KV_F32 && s16 && s16 != kv_type)
        fail(BRN_ERR_INVALID_ARG, "%s: kv_type %s cannot be read in compute mode %s (a 16-bit compute mode reads a pool of its own type; the fp32-class modes read bf16 and f16 pools alike)",
             who, KV_TYPE_NAME[kv_type], KV_TYPE_NAME[s16]);
    const int page_log2 = paged_pool_check(who, n_pages, page_size, max_pages);
    if (max_kv_len < 1 || max_kv_len > 65536 || max_kv_len > (long long)max_pages * page_size)
        fail(BRN_ERR_INVALID_ARG, "%s: max_kv_len %d unsupported with max_pages %d of page_size %d (1 <= max_kv_len <= min(65536, max_pages * page_size))",
             who, max_kv_len, max_pages, page_size);
    // every limit of the split entry with max_kv_len in the place of seq_kv, but for its causal one (a per-sequence matter the kernels define)
    flash_attention_check_sizes(who, true, batch, seq_q, max_kv_len, heads, kv_heads, head_dim);
    splitkv_check_splits(who, kv_splits);
    const FaSplitPlan pl = splitkv_plan_checked(who, batch, seq_q, max_kv_len, heads, kv_heads, head_dim, kv_splits);
    if (layout != BRN_ATTN_BSHD && layout != BRN_ATTN_BHSD) fail(BRN_ERR_INVALID_ARG, "%s: layout %d unknown (layout must be 0 = BSHD or 1 = BHSD)", who, layout);
    if (causal != 0 && causal != 1) fail(BRN_ERR_INVALID_ARG, "%s: causal %d (causal must be 0 or 1)", who, causal);
    if (!scale_arg_ok(scale)) fail(BRN_ERR_INVALID_ARG, "%s: scale must be finite and >= 0 (0 = head_dim^-0.5)", who);
    const size_t nq = (size_t)batch * heads * seq_q * head_dim, npool = (size_t)n_pages * page_size * kv_heads * head_dim;
    const size_t pool_floats = npool * kv_type_bytes(kv_type) / 4;        // (npool is a multiple of 16 * 32)
    const size_t R = (size_t)batch * heads * seq_q, ntab = (size_t)batch * max_pages;
    const size_t need = pl.S > 1 ? pl.workspace_floats : 0;
    if (need && (!workspace || workspace_floats < need))
        fail(BRN_ERR_INVALID_ARG, "%s: workspace %s for %d splits (it must hold S * batch * heads * seq_q * (head_dim + 1) = %zu floats, workspace_floats %zu)",
             who, workspace ? "too small" : "is NULL", pl.S, need, workspace_floats);
    float* const ws = need ? workspace : nullptr;
    // sizes in bytes: the table and the lengths are ints, the pool's elements 4, 2 or 1 bytes (a null scale array overlaps nothing)
    const struct { const void* p; size_t n; } ins[] = {{q, nq * 4}, {k_pages, pool_floats * 4}, {v_pages, pool_floats * 4}, {block_table, ntab * 4}, {kv_lens, (size_t)batch * 4},
                                                       {k_scale, (size_t)kv_heads * 4}, {v_scale, (size_t)kv_heads * 4}};
    const struct { const float* p; size_t n; const char* name; } outs[] = {{y, nq * 4, "y"}, {lse, lse ? R * 4 : 0, "lse"}, {ws, need * 4, "workspace"}};
    for (int a = 0; a < 3; ++a) {
        if (!outs[a].p) continue;
        for (const auto& in : ins)
            if (bytes_overlap(in.p, in.n, outs[a].p, outs[a].n)) fail(BRN_ERR_INVALID_ARG, "%s: %s must not overlap an input", who, outs[a].name);
        for (int b = 0; b < a; ++b)
            if (outs[b].p && bytes_overlap(outs[b].p, outs[b].n, outs[a].p, outs[a].n))
                fail(BRN_ERR_INVALID_ARG, "%s: %s and %s must not overlap", who, outs[b].name, outs[a].name);
    }
    if (loc == BRN_MEM_DEVICE && !all_aligned16({q, k_pages, v_pages, y, lse, ws}))
        fail(BRN_ERR_INVALID_ARG, "%s: device q, k_pages, v_pages, y, lse and workspace must be 16-byte aligned", who);
    if (loc == BRN_MEM_DEVICE && ((reinterpret_cast<uintptr_t>(block_table) | reinterpret_cast<uintptr_t>(kv_lens)) & 3))
        fail(BRN_ERR_INVALID_ARG, "%s: device block_table and kv_lens must be 4-byte aligned", who);
    if (loc == BRN_MEM_DEVICE && ((reinterpret_cast<uintptr_t>(k_scale) | reinterpret_cast<uintptr_t>(v_scale)) & 3))
        fail(BRN_ERR_INVALID_ARG, "%s: device k_scale and v_scale must be 4-byte aligned", who);
    ensure_device(device);
    Staging st(stream, loc);
    FlashAttentionParams p{};
    if (k_scale) p.k_scale = st.in(k_scale, (size_t)kv_heads);
    if (v_scale) p.v_scale = st.in(v_scale, (size_t)kv_heads);
    p.q = st.in(q, nq); p.k = st.in(static_cast<const float*>(k_pages), pool_floats); p.v = st.in(static_cast<const float*>(v_pages), pool_floats);
    p.block_table = reinterpret_cast<const int*>(st.in(reinterpret_cast<const float*>(block_table), ntab));
    p.kv_lens = reinterpret_cast<const int*>(st.in(reinterpret_cast<const float*>(kv_lens), (size_t)batch));
    p.y = st.out(y, nq);
    p.batch = batch; p.heads = heads; p.kv_heads = kv_heads; p.seq_q = seq_q; p.seq_kv = max_kv_len; p.head_dim = head_dim;
    const long d = head_dim;
    if (layout == BRN_ATTN_BSHD) { p.q_ss = heads * d; p.q_sh = d; p.q_sb = seq_q * p.q_ss; }
    else { p.q_ss = d; p.q_sh = seq_q * d; p.q_sb = heads * p.q_sh; }
    // a key's row inside a page; the page comes from the table (no batch stride).  Strides count elements of the pool's type
    p.kv_ss = kv_heads * d; p.kv_sh = d; p.kv_sb = 0;
    p.page_stride = (long)page_size * p.kv_ss; p.page_log2 = page_log2; p.n_pages = n_pages; p.max_pages = max_pages;
    p.kv_type = kv_type;
    p.causal = causal; p.causal_off = 0;       // each workgroup's own: len_b - seq_q
    p.scale = scale_or_default(scale, head_dim);
    p.s16 = s16;
    p.kv_splits = pl.S; p.tiles_per_split = pl.tps;
    if (lse) p.lse = st.out(lse, R);
    if (need) {
        p.o_part = st.out(ws, need);
        p.lse2_part = p.o_part + (size_t)pl.S * R * head_dim;
    }
    BRN_HIP(launch_flash_attention(p, (hipStream_t)stream));
    st.finish();
}

brn_status brn_flash_attention_paged_forward(const float* q, const float* k_pages, const float* v_pages, const int* block_table, const int* kv_lens, int batch,
                                             int seq_q, int max_kv_len, int heads, int kv_heads, int head_dim, int n_pages, int page_size, int max_pages,
                                             int layout, int causal, float scale, int kv_splits, float* y, float* lse, float* workspace,
                                             size_t workspace_floats, brn_mem loc, int device, void* stream) {
    return guarded([&] {
        flash_attention_paged_body("flash attention paged", q, k_pages, v_pages, BRN_KV_F32, false, nullptr, nullptr, block_table, kv_lens, batch, seq_q, max_kv_len, heads, kv_heads, head_dim,
                                   n_pages, page_size, max_pages, layout, causal, scale, kv_splits, y, lse, workspace, workspace_floats, loc, device, stream);
    });
}

brn_status brn_flash_attention_paged_kv_forward(const float* q, const void* k_pages, const void* v_pages, int kv_type, const int* block_table,
                                                const int* kv_lens, int batch, int seq_q, int max_kv_len, int heads, int kv_heads, int head_dim,
                                                int n_pages, int page_size, int max_pages, int layout, int causal, float scale, int kv_splits, float* y,
                                                float* lse, float* workspace, size_t workspace_floats, brn_mem loc, int device, void* stream) {
    return guarded([&] {
        flash_attention_paged_body("flash attention paged kv", q, k_pages, v_pages, kv_type, false, nullptr, nullptr, block_table, kv_lens, batch, seq_q, max_kv_len, heads,
                                   kv_heads, head_dim, n_pages, page_size, max_pages, layout, causal, scale, kv_splits, y, lse, workspace, workspace_floats, loc, device, stream);
    });
}

brn_status brn_flash_attention_paged_fp8_forward(const float* q, const void* k_pages, const void* v_pages, const float* k_scale, const float* v_scale,
                                                 const int* block_table, const int* kv_lens, int batch, int seq_q, int max_kv_len, int heads, int kv_heads,
                                                 int head_dim, int n_pages, int page_size, int max_pages, int layout, int causal, float scale, int kv_splits,
                                                 float* y, float* lse, float* workspace, size_t workspace_floats, brn_mem loc, int device, void* stream) {
    return guarded([&] {
        flash_attention_paged_body("flash attention paged fp8", q, k_pages, v_pages, FA_KV_FP8, true, k_scale, v_scale, block_table, kv_lens, batch, seq_q, max_kv_len, heads,
                                   kv_heads, head_dim, n_pages, page_size, max_pages, layout, causal, scale, kv_splits, y, lse, workspace, workspace_floats, loc, device, stream);
    });
}

// seq_new tokens per sequence into the pool, behind the keys each sequence has (kernels/kv_cache.hip).  Like the paged attention entries it
// reads neither block_table nor kv_lens on the host for BRN_MEM_DEVICE, allocates nothing and does not synchronise.  BRN_MEM_HOST (a test
// convenience) stages the whole pool up and copies it back whole.
// The caller's rotary table of brn_rope_forward and the two rope appends: [n_pos, rot_dim / 2] fp32 each
struct RopeTable { const float* cos; const float* sin; int n_pos, rot_dim, style; };
static size_t rope_table_floats(const RopeTable& r) { return (size_t)r.n_pos * (r.rot_dim / 2); }
// (head_dim has been checked)
static void rope_table_check(const char* who, const RopeTable& r, int head_dim) {
    if (!r.cos || !r.sin) fail(BRN_ERR_INVALID_ARG, "%s: null cos or sin", who);
    if (r.rot_dim < 16 || r.rot_dim > head_dim || r.rot_dim % 16)
        fail(BRN_ERR_INVALID_ARG, "%s: rot_dim %d unsupported (rot_dim must be a multiple of 16 with 16 <= rot_dim <= head_dim = %d)", who, r.rot_dim, head_dim);
    if (r.style != BRN_ROPE_HALF && r.style != BRN_ROPE_INTERLEAVED) fail(BRN_ERR_INVALID_ARG, "%s: style %d unknown (style must be 0 = HALF or 1 = INTERLEAVED)", who, r.style);
    if (r.n_pos < 1 || r.n_pos > (1 << 24)) fail(BRN_ERR_INVALID_ARG, "%s: n_pos %d unsupported (1 <= n_pos <= 2^24)", who, r.n_pos);
}

// One body for brn_kv_cache_append and brn_kv_cache_append_fp8 (fp8 = true: an e4m3fn pool of bytes and the two scale arrays) and their
// rope forms (rope non-null: K is rotated by the table before the cast).
static void kv_cache_append_body(const char* who, const float* k_new, const float* v_new, int batch, int seq_new, int kv_heads, int head_dim, int layout, void* k_pages,
                                 void* v_pages, int kv_type, bool fp8, const float* k_scale, const float* v_scale, const int* block_table, const int* kv_lens,
                                 int* kv_lens_out, int n_pages, int page_size, int max_pages, brn_mem loc, int device, void* stream, const RopeTable* rope = nullptr) {
    {
        if (!k_new || !v_new || !k_pages || !v_pages) fail(BRN_ERR_INVALID_ARG, "%s: null k_new, v_new, k_pages or v_pages", who);
        if (!block_table || !kv_lens) fail(BRN_ERR_INVALID_ARG, "%s: null block_table or kv_lens", who);
        if (fp8) kv_type = FA_KV_FP8;
        else kv_type_check(who, kv_type);
        if (!(head_dim == 32 || head_dim == 64 || head_dim == 128))
            fail(BRN_ERR_INVALID_ARG, "%s: head_dim %d unsupported (head_dim must be 32, 64 or 128)", who, head_dim);
        if (rope) rope_table_check(who, *rope, head_dim);
        if (batch < 1 || kv_heads < 1) fail(BRN_ERR_INVALID_ARG, "%s: batch %d, kv_heads %d unsupported (batch >= 1, kv_heads >= 1)", who, batch, kv_heads);
        if (seq_new < 1 || seq_new > 65536) fail(BRN_ERR_INVALID_ARG, "%s: seq_new %d unsupported (1 <= seq_new <= 65536)", who, seq_new);
        if (layout != BRN_ATTN_BSHD && layout != BRN_ATTN_BHSD) fail(BRN_ERR_INVALID_ARG, "%s: layout %d unknown (layout must be 0 = BSHD or 1 = BHSD)", who, layout);
        const int page_log2 = paged_pool_check(who, n_pages, page_size, max_pages);
        if ((long long)max_pages * page_size > 0x7fffffffLL)
            fail(BRN_ERR_INVALID_ARG, "%s: max_pages %d of page_size %d too large (max_pages * page_size < 2^31)", who, max_pages, page_size);
        // the grid: a thread per 8 elements of a new row of K and of V
        const long long per_b = (long long)seq_new * kv_heads * (head_dim / 8);
        if (per_b > 0x7fffffffLL || (per_b * batch + 255) / 256 > 0x7fffffffLL)
            fail(BRN_ERR_INVALID_ARG, "%s: batch %d, seq_new %d, kv_heads %d too large (seq_new * kv_heads * head_dim / 8 < 2^31, batch * that / 256 < 2^31)", who, batch, seq_new, kv_heads);
        const size_t nnew = (size_t)batch * seq_new * kv_heads * head_dim, npool = (size_t)n_pages * page_size * kv_heads * head_dim;
        const size_t pool_floats = npool * kv_type_bytes(kv_type) / 4, ntab = (size_t)batch * max_pages;
        const struct { const void* p; size_t n; const char* name; } ins[] = {{k_new, nnew * 4, "k_new"}, {v_new, nnew * 4, "v_new"}, {block_table, ntab * 4, "block_table"},
                                                                             {kv_lens, (size_t)batch * 4, "kv_lens"}, {k_scale, (size_t)kv_heads * 4, "k_scale"},
                                                                             {v_scale, (size_t)kv_heads * 4, "v_scale"},
                                                                             {rope ? rope->cos : nullptr, rope ? rope_table_floats(*rope) * 4 : 0, "cos"},
                                                                             {rope ? rope->sin : nullptr, rope ? rope_table_floats(*rope) * 4 : 0, "sin"}};
        for (const auto& in : ins)
            if (bytes_overlap(in.p, in.n, k_pages, pool_floats * 4) || bytes_overlap(in.p, in.n, v_pages, pool_floats * 4))
                fail(BRN_ERR_INVALID_ARG, "%s: %s must not overlap the pool", who, in.name);
        if (bytes_overlap(k_pages, pool_floats * 4, v_pages, pool_floats * 4)) fail(BRN_ERR_INVALID_ARG, "%s: k_pages and v_pages must not overlap", who);
        if (kv_lens_out && kv_lens_out != kv_lens) {
            // kv_lens itself is the in-place form; any other overlap with an array the rows kernel reads or writes is refused
            for (const auto& in : ins)
                if (bytes_overlap(in.p, in.n, kv_lens_out, (size_t)batch * 4)) fail(BRN_ERR_INVALID_ARG, "%s: kv_lens_out must not overlap %s (kv_lens itself, the in-place form, excepted)", who, in.name);
            if (bytes_overlap(k_pages, pool_floats * 4, kv_lens_out, (size_t)batch * 4) || bytes_overlap(v_pages, pool_floats * 4, kv_lens_out, (size_t)batch * 4))
                fail(BRN_ERR_INVALID_ARG, "%s: kv_lens_out must not overlap the pool", who);
        }
        if (loc == BRN_MEM_DEVICE && !all_aligned16({k_new, v_new, k_pages, v_pages}))
            fail(BRN_ERR_INVALID_ARG, "%s: device k_new, v_new, k_pages and v_pages must be 16-byte aligned", who);
        if (loc == BRN_MEM_DEVICE && ((reinterpret_cast<uintptr_t>(block_table) | reinterpret_cast<uintptr_t>(kv_lens) | reinterpret_cast<uintptr_t>(kv_lens_out)) & 3))
            fail(BRN_ERR_INVALID_ARG, "%s: device block_table, kv_lens and kv_lens_out must be 4-byte aligned", who);
        if (loc == BRN_MEM_DEVICE && ((reinterpret_cast<uintptr_t>(k_scale) | reinterpret_cast<uintptr_t>(v_scale)) & 3))
            fail(BRN_ERR_INVALID_ARG, "%s: device k_scale and v_scale must be 4-byte aligned", who);
        if (rope && loc == BRN_MEM_DEVICE && !all_aligned16({rope->cos, rope->sin})) fail(BRN_ERR_INVALID_ARG, "%s: device cos and sin must be 16-byte aligned", who);
        ensure_device(device);
        Staging st(stream, loc);
        KvAppendParams p{};
        if (rope) {
            p.rope_cos = st.in(rope->cos, rope_table_floats(*rope)); p.rope_sin = st.in(rope->sin, rope_table_floats(*rope));
            p.rope_n_pos = rope->n_pos; p.rope_dim = rope->rot_dim; p.rope_style = rope->style;
        }
        if (k_scale) p.k_scale = st.in(k_scale, (size_t)kv_heads);
        if (v_scale) p.v_scale = st.in(v_scale, (size_t)kv_heads);
        p.k_new = st.in(k_new, nnew); p.v_new = st.in(v_new, nnew);
        if (loc == BRN_MEM_DEVICE) { p.k_pages = k_pages; p.v_pages = v_pages; }
        else {
            // the pool goes up whole and comes back whole
            float* pools[2] = {static_cast<float*>(k_pages), static_cast<float*>(v_pages)};
            void** dst[2] = {&p.k_pages, &p.v_pages};
            for (int a = 0; a < 2; ++a) {
                float* dpool = st.dalloc(pool_floats);
                BRN_HIP(hipMemcpyAsync(dpool, pools[a], pool_floats * 4, hipMemcpyHostToDevice, (hipStream_t)stream));
                st.outs.push_back({pools[a], dpool, pool_floats});
                *dst[a] = dpool;
            }
        }
        p.block_table = reinterpret_cast<const int*>(st.in(reinterpret_cast<const float*>(block_table), ntab));
        p.kv_lens = reinterpret_cast<const int*>(st.in(reinterpret_cast<const float*>(kv_lens), (size_t)batch));
        if (kv_lens_out) p.kv_lens_out = reinterpret_cast<int*>(st.out(reinterpret_cast<float*>(kv_lens_out), (size_t)batch));
        p.kv_type = kv_type;
        p.batch = batch; p.seq_new = seq_new; p.kv_heads = kv_heads; p.head_dim = head_dim;
        const long d = head_dim;
        if (layout == BRN_ATTN_BSHD) { p.new_ss = kv_heads * d; p.new_sh = d; p.new_sb = seq_new * p.new_ss; }
        else { p.new_ss = d; p.new_sh = seq_new * d; p.new_sb = kv_heads * p.new_sh; }
        p.kv_ss = kv_heads * d; p.page_stride = (long)page_size * p.kv_ss;
        p.page_log2 = page_log2; p.n_pages = n_pages; p.max_pages = max_pages; p.cap = max_pages * page_size;
        BRN_HIP(launch_kv_cache_append(p, (hipStream_t)stream));
        st.finish();
    }
}

brn_status brn_kv_cache_append(const float* k_new, const float* v_new, int batch, int seq_new, int kv_heads, int head_dim, int layout, void* k_pages,
                               void* v_pages, int kv_type, const int* block_table, const int* kv_lens, int* kv_lens_out, int n_pages, int page_size,
                               int max_pages, brn_mem loc, int device, void* stream) {
    return guarded([&] {
        kv_cache_append_body("kv cache append", k_new, v_new, batch, seq_new, kv_heads, head_dim, layout, k_pages, v_pages, kv_type, false, nullptr, nullptr, block_table,
                             kv_lens, kv_lens_out, n_pages, page_size, max_pages, loc, device, stream);
    });
}

brn_status brn_kv_cache_append_fp8(const float* k_new, const float* v_new, int batch, int seq_new, int kv_heads, int head_dim, int layout, void* k_pages,
                                   void* v_pages, const float* k_scale, const float* v_scale, const int* block_table, const int* kv_lens, int* kv_lens_out,
                                   int n_pages, int page_size, int max_pages, brn_mem loc, int device, void* stream) {
    return guarded([&] {
        kv_cache_append_body("kv cache append fp8", k_new, v_new, batch, seq_new, kv_heads, head_dim, layout, k_pages, v_pages, FA_KV_FP8, true, k_scale, v_scale, block_table,
                             kv_lens, kv_lens_out, n_pages, page_size, max_pages, loc, device, stream);
    });
}

brn_status brn_kv_cache_append_rope(const float* k_new, const float* v_new, int batch, int seq_new, int kv_heads, int head_dim, int layout, const float* cos,
                                    const float* sin, int n_pos, int rot_dim, int style, void* k_pages, void* v_pages, int kv_type, const int* block_table,
                                    const int* kv_lens, int* kv_lens_out, int n_pages, int page_size, int max_pages, brn_mem loc, int device, void* stream) {
    return guarded([&] {
        const RopeTable rope{cos, sin, n_pos, rot_dim, style};
        kv_cache_append_body("kv cache append rope", k_new, v_new, batch, seq_new, kv_heads, head_dim, layout, k_pages, v_pages, kv_type, false, nullptr, nullptr, block_table,
                             kv_lens, kv_lens_out, n_pages, page_size, max_pages, loc, device, stream, &rope);
    });
}

brn_status brn_kv_cache_append_rope_fp8(const float* k_new, const float* v_new, int batch, int seq_new, int kv_heads, int head_dim, int layout, const float* cos,
                                        const float* sin, int n_pos, int rot_dim, int style, void* k_pages, void* v_pages, const float* k_scale, const float* v_scale,
                                        const int* block_table, const int* kv_lens, int* kv_lens_out, int n_pages, int page_size, int max_pages, brn_mem loc,
                                        int device, void* stream) {
    return guarded([&] {
        const RopeTable rope{cos, sin, n_pos, rot_dim, style};
        kv_cache_append_body("kv cache append rope fp8", k_new, v_new, batch, seq_new, kv_heads, head_dim, layout, k_pages, v_pages, FA_KV_FP8, true, k_scale, v_scale,
                             block_table, kv_lens, kv_lens_out, n_pages, page_size, max_pages, loc, device, stream, &rope);
    });
}

// Rotary embedding of q (or of k at prefill) by the caller's table (kernels/kv_cache.hip, RopeParams).  positions is device data for
// BRN_MEM_DEVICE: never read on the host, clamped by the kernel; the call allocates nothing and does not synchronise.
brn_status brn_rope_forward(const float* x, int batch, int seq, int heads, int head_dim, int layout, const float* cos, const float* sin, int n_pos, int rot_dim,
                            int style, const int* positions, float* y, brn_mem loc, int device, void* stream) {
    return guarded([&] {
        const char* who = "rope";
        if (!x || !y) fail(BRN_ERR_INVALID_ARG, "%s: null x or y", who);
        if (!(head_dim == 32 || head_dim == 64 || head_dim == 128))
            fail(BRN_ERR_INVALID_ARG, "%s: head_dim %d unsupported (head_dim must be 32, 64 or 128)", who, head_dim);
        const RopeTable rope{cos, sin, n_pos, rot_dim, style};
        rope_table_check(who, rope, head_dim);
        if (batch < 1 || heads < 1) fail(BRN_ERR_INVALID_ARG, "%s: batch %d, heads %d unsupported (batch >= 1, heads >= 1)", who, batch, heads);
        if (seq < 1 || seq > 65536) fail(BRN_ERR_INVALID_ARG, "%s: seq %d unsupported (1 <= seq <= 65536)", who, seq);
        if (layout != BRN_ATTN_BSHD && layout != BRN_ATTN_BHSD) fail(BRN_ERR_INVALID_ARG, "%s: layout %d unknown (layout must be 0 = BSHD or 1 = BHSD)", who, layout);
        // the grid: a thread per 8 elements of a row at the most
        const long long per_b = (long long)seq * heads * (head_dim / 8);
        if (per_b > 0x7fffffffLL || per_b * batch > 0x7fffffffLL)
            fail(BRN_ERR_INVALID_ARG, "%s: batch %d, seq %d, heads %d too large (batch * seq * heads * head_dim / 8 < 2^31)", who, batch, seq, heads);
        const size_t n = (size_t)batch * seq * heads * head_dim, ntab = rope_table_floats(rope);
        if (y != x && bytes_overlap(x, n * 4, y, n * 4)) fail(BRN_ERR_INVALID_ARG, "%s: y must be x itself (in place) or not overlap x", who);
        const struct { const void* p; size_t n; const char* name; } ins[] = {{cos, ntab * 4, "cos"}, {sin, ntab * 4, "sin"}, {positions, (size_t)batch * 4, "positions"}};
        for (const auto& in : ins)
            if (bytes_overlap(in.p, in.n, y, n * 4)) fail(BRN_ERR_INVALID_ARG, "%s: %s must not overlap y", who, in.name);
        if (loc == BRN_MEM_DEVICE && !all_aligned16({x, y, cos, sin})) fail(BRN_ERR_INVALID_ARG, "%s: device x, y, cos and sin must be 16-byte aligned", who);
        if (loc == BRN_MEM_DEVICE && (reinterpret_cast<uintptr_t>(positions) & 3)) fail(BRN_ERR_INVALID_ARG, "%s: device positions must be 4-byte aligned", who);
        ensure_device(device);
        Staging st(stream, loc);
        RopeParams p{};
        p.x = st.in(x, n); p.y = st.out(y, n);
        p.cos = st.in(cos, ntab); p.sin = st.in(sin, ntab);
        if (positions) p.positions = reinterpret_cast<const int*>(st.in(reinterpret_cast<const float*>(positions), (size_t)batch));
        p.batch = batch; p.seq = seq; p.heads = heads; p.head_dim = head_dim;
        const long d = head_dim;
        if (layout == BRN_ATTN_BSHD) { p.ss = heads * d; p.sh = d; p.sb = seq * p.ss; }
        else { p.ss = d; p.sh = seq * d; p.sb = heads * p.sh; }
        p.n_pos = n_pos; p.rot_dim = rot_dim; p.style = style;
        BRN_HIP(launch_rope(p, (hipStream_t)stream));
        st.finish();
    });
}

// The packed batch over the paged pool: a mixed prefill / decode step in one call.  cu_seqlens_q is device data like the table and the
// lengths: never read on the host for BRN_MEM_DEVICE, made harmless by the rule of brn_flash_paged_varlen_plan.h, which a one-workgroup
// kernel evaluates into plan_workspace ahead of the main launch.  The host sizes the grid with T_max, the split with max_kv_len.  The calls
// allocate nothing and do not synchronise.  BRN_MEM_HOST (a test convenience) stages every output up as well as down, so that the rows
// no kernel writes (padding) come back as they went.
static const char* const PAGED_VARLEN = "flash attention paged varlen";
static const char* const APPEND_VARLEN = "kv cache append varlen";
static const char* const POOL_TYPE_NAME[4] = {"f32", "bf16", "f16", "e4m3"};
static void pool_type_check(const char* who, int pool_type, const float* k_scale, const float* v_scale) {
    if (pool_type < BRN_POOL_F32 || pool_type > BRN_POOL_E4M3)
        fail(BRN_ERR_INVALID_ARG, "%s: pool_type %d unknown (pool_type must be 0 = f32, 1 = bf16, 2 = f16 or 3 = e4m3)", who, pool_type);
    if (pool_type != BRN_POOL_E4M3 && (k_scale || v_scale))
        fail(BRN_ERR_INVALID_ARG, "%s: k_scale and v_scale must be NULL unless pool_type is 3 = e4m3 (pool_type %d = %s)", who, pool_type, POOL_TYPE_NAME[pool_type]);
}
// the sizes of a pack: 1 <= n_seqs <= 65536, total_q >= 1, G * total_q < 2^31 (G = 1 for the append)
static void pack_check(const char* who, int total_q, int n_seqs, int G) {
    if (n_seqs < 1 || n_seqs > FA_PV_MAX_SEQS) fail(BRN_ERR_INVALID_ARG, "%s: n_seqs %d unsupported (1 <= n_seqs <= 65536)", who, n_seqs);
    if (total_q < 1) fail(BRN_ERR_INVALID_ARG, "%s: total_q %d unsupported (total_q >= 1)", who, total_q);
    if ((long long)G * total_q > 0x7fffffffLL)
        fail(BRN_ERR_INVALID_ARG, "%s: total_q %d too large with G = heads / kv_heads = %d (G * total_q < 2^31)", who, total_q, G);
}
static void plan_workspace_check(const char* who, const int* plan_workspace, size_t plan_ints, int n_seqs) {
    const size_t need = fa_pv_plan_ints(n_seqs);
    if (!plan_workspace || plan_ints < need)
        fail(BRN_ERR_INVALID_ARG, "%s: plan_workspace %s (it must hold 2 * (n_seqs + 1) = %zu ints, plan_ints %zu)", who, plan_workspace ? "too small" : "is NULL", need, plan_ints);
    if (reinterpret_cast<uintptr_t>(plan_workspace) & 3) fail(BRN_ERR_INVALID_ARG, "%s: plan_workspace must be 4-byte aligned", who);
}
struct PvPlan { int S, tps; long long t_max; size_t workspace_floats, plan_ints; };
// every check the plan entry can make, and the split: nkt and the normalisation are flash_split_plan's, the base grid is T_max * kv_heads
static PvPlan paged_varlen_plan_checked(const char* who, int total_q, int n_seqs, int max_kv_len, int heads, int kv_heads, int head_dim, int kv_splits) {
    if (!(head_dim == 32 || head_dim == 64 || head_dim == 128))
        fail(BRN_ERR_INVALID_ARG, "%s: head_dim %d unsupported (head_dim must be 32, 64 or 128)", who, head_dim);
    if (heads < 1) fail(BRN_ERR_INVALID_ARG, "%s: heads %d unsupported (heads >= 1)", who, heads);
    if (kv_heads < 1 || kv_heads > heads || heads % kv_heads)
        fail(BRN_ERR_INVALID_ARG, "%s: kv_heads %d unsupported with heads %d (1 <= kv_heads <= heads, heads %% kv_heads == 0)", who, kv_heads, heads);
    const int G = heads / kv_heads;
    pack_check(who, total_q, n_seqs, G);
    if (max_kv_len < 1 || max_kv_len > 65536) fail(BRN_ERR_INVALID_ARG, "%s: max_kv_len %d unsupported (1 <= max_kv_len <= 65536)", who, max_kv_len);
    splitkv_check_splits(who, kv_splits);
    PvPlan pl;
    pl.t_max = fa_pv_max_tiles(G, total_q, n_seqs);
    const int nkt = (max_kv_len + FA_SPLIT_TILE - 1) / FA_SPLIT_TILE;
    const int ask = kv_splits ? kv_splits : flash_split_auto((long long)kv_heads * pl.t_max, nkt);
    pl.tps = (nkt + ask - 1) / ask;
    pl.S = (nkt + pl.tps - 1) / pl.tps;
    if (pl.t_max * kv_heads * pl.S > 0x7fffffffLL)
        fail(BRN_ERR_INVALID_ARG, "%s: %lld row tiles x kv_heads %d x %d splits too large (T_max * kv_heads * S < 2^31, T_max = (G * total_q + 63 * min(n_seqs, total_q)) / 64)",
             who, pl.t_max, kv_heads, pl.S);
    pl.workspace_floats = (size_t)pl.S * heads * total_q * ((size_t)head_dim + 1);
    pl.plan_ints = fa_pv_plan_ints(n_seqs);
    return pl;
}

brn_status brn_flash_attention_paged_varlen_plan(int total_q, int n_seqs, int max_kv_len, int heads, int kv_heads, int head_dim, int kv_splits,
                                                 int* splits_out, int* tiles_per_split_out, size_t* workspace_floats_out, size_t* plan_ints_out) {
    return guarded([&] {
        const PvPlan pl = paged_varlen_plan_checked(PAGED_VARLEN, total_q, n_seqs, max_kv_len, heads, kv_heads, head_dim, kv_splits);
        if (splits_out) *splits_out = pl.S;
        if (tiles_per_split_out) *tiles_per_split_out = pl.tps;
        if (workspace_floats_out) *workspace_floats_out = pl.workspace_floats;
        if (plan_ints_out) *plan_ints_out = pl.plan_ints;
    });
}

// BRN_MEM_HOST: an output that is only partly written goes up before it comes down
static float* stage_inout(Staging& st, float* p, size_t n, void* stream) {
    if (st.loc == BRN_MEM_DEVICE) return p;
    float* d = st.out(p, n);
    BRN_HIP(hipMemcpyAsync(d, p, n * sizeof(float), hipMemcpyHostToDevice, (hipStream_t)stream));
    return d;
}

brn_status brn_flash_attention_paged_varlen_forward(const float* q, const void* k_pages, const void* v_pages, int pool_type, const float* k_scale,
                                                    const float* v_scale, const int* block_table, const int* kv_lens, const int* cu_seqlens_q, int total_q,
                                                    int n_seqs, int max_kv_len, int heads, int kv_heads, int head_dim, int n_pages, int page_size, int max_pages,
                                                    int causal, float scale, int kv_splits, float* y, float* lse, float* workspace, size_t workspace_floats,
                                                    int* plan_workspace, size_t plan_ints, brn_mem loc, int device, void* stream) {
    return guarded([&] {
        const char* who = PAGED_VARLEN;
        if (!q || !k_pages || !v_pages || !y) fail(BRN_ERR_INVALID_ARG, "%s: null q, k_pages, v_pages or y", who);
        if (!block_table || !kv_lens || !cu_seqlens_q) fail(BRN_ERR_INVALID_ARG, "%s: null block_table, kv_lens or cu_seqlens_q", who);
        pool_type_check(who, pool_type, k_scale, v_scale);
        const int s16 = attention_op_s16();
        if ((pool_type == BRN_POOL_BF16 || pool_type == BRN_POOL_F16) && s16 && s16 != pool_type)
            fail(BRN_ERR_INVALID_ARG, "%s: pool_type %s cannot be read in compute mode %s (a 16-bit compute mode reads a pool of its own type or an e4m3 pool; the fp32-class modes read every pool)",
                 who, POOL_TYPE_NAME[pool_type], KV_TYPE_NAME[s16]);
        const int page_log2 = paged_pool_check(who, n_pages, page_size, max_pages);
        const PvPlan pl = paged_varlen_plan_checked(who, total_q, n_seqs, max_kv_len, heads, kv_heads, head_dim, kv_splits);
        if (max_kv_len > (long long)max_pages * page_size)
            fail(BRN_ERR_INVALID_ARG, "%s: max_kv_len %d unsupported with max_pages %d of page_size %d (1 <= max_kv_len <= min(65536, max_pages * page_size))",
                 who, max_kv_len, max_pages, page_size);
        if (causal != 0 && causal != 1) fail(BRN_ERR_INVALID_ARG, "%s: causal %d (causal must be 0 or 1)", who, causal);
        if (!scale_arg_ok(scale)) fail(BRN_ERR_INVALID_ARG, "%s: scale must be finite and >= 0 (0 = head_dim^-0.5)", who);
        const size_t nq = (size_t)total_q * heads * head_dim, npool = (size_t)n_pages * page_size * kv_heads * head_dim;
        const size_t pool_floats = npool * kv_type_bytes(pool_type) / 4;
        const size_t R = (size_t)heads * total_q, ntab = (size_t)n_seqs * max_pages;
        const size_t need = pl.S > 1 ? pl.workspace_floats : 0;
        if (need && (!workspace || workspace_floats < need))
            fail(BRN_ERR_INVALID_ARG, "%s: workspace %s for %d splits (it must hold S * heads * total_q * (head_dim + 1) = %zu floats, workspace_floats %zu)",
                 who, workspace ? "too small" : "is NULL", pl.S, need, workspace_floats);
        plan_workspace_check(who, plan_workspace, plan_ints, n_seqs);
        float* const ws = need ? workspace : nullptr;
        const struct { const void* p; size_t n; } ins[] = {{q, nq * 4}, {k_pages, pool_floats * 4}, {v_pages, pool_floats * 4}, {block_table, ntab * 4}, {kv_lens, (size_t)n_seqs * 4},
                                                           {cu_seqlens_q, ((size_t)n_seqs + 1) * 4}, {k_scale, (size_t)kv_heads * 4}, {v_scale, (size_t)kv_heads * 4}};
        const struct { const void* p; size_t n; const char* name; } outs[] = {{y, nq * 4, "y"}, {lse, lse ? R * 4 : 0, "lse"}, {ws, need * 4, "workspace"},
                                                                             {plan_workspace, pl.plan_ints * 4, "plan_workspace"}};
        for (int a = 0; a < 4; ++a) {
            if (!outs[a].p) continue;
            for (const auto& in : ins)
                if (bytes_overlap(in.p, in.n, outs[a].p, outs[a].n)) fail(BRN_ERR_INVALID_ARG, "%s: %s must not overlap an input", who, outs[a].name);
            for (int b = 0; b < a; ++b)
                if (outs[b].p && bytes_overlap(outs[b].p, outs[b].n, outs[a].p, outs[a].n))
                    fail(BRN_ERR_INVALID_ARG, "%s: %s and %s must not overlap", who, outs[b].name, outs[a].name);
        }
        if (loc == BRN_MEM_DEVICE && !all_aligned16({q, static_cast<const float*>(k_pages), static_cast<const float*>(v_pages), y, lse, ws}))
            fail(BRN_ERR_INVALID_ARG, "%s: device q, k_pages, v_pages, y, lse and workspace must be 16-byte aligned", who);
        if ((reinterpret_cast<uintptr_t>(block_table) | reinterpret_cast<uintptr_t>(kv_lens) | reinterpret_cast<uintptr_t>(cu_seqlens_q)) & 3)
            fail(BRN_ERR_INVALID_ARG, "%s: block_table, kv_lens and cu_seqlens_q must be 4-byte aligned", who);
        if (loc == BRN_MEM_DEVICE && ((reinterpret_cast<uintptr_t>(k_scale) | reinterpret_cast<uintptr_t>(v_scale)) & 3))
            fail(BRN_ERR_INVALID_ARG, "%s: device k_scale and v_scale must be 4-byte aligned", who);
        ensure_device(device);
        Staging st(stream, loc);
        FlashAttentionParams p{};
        if (k_scale) p.k_scale = st.in(k_scale, (size_t)kv_heads);
        if (v_scale) p.v_scale = st.in(v_scale, (size_t)kv_heads);
        p.q = st.in(q, nq); p.k = st.in(static_cast<const float*>(k_pages), pool_floats); p.v = st.in(static_cast<const float*>(v_pages), pool_floats);
        p.block_table = reinterpret_cast<const int*>(st.in(reinterpret_cast<const float*>(block_table), ntab));
        p.kv_lens = reinterpret_cast<const int*>(st.in(reinterpret_cast<const float*>(kv_lens), (size_t)n_seqs));
        p.pv_cu = reinterpret_cast<const int*>(st.in(reinterpret_cast<const float*>(cu_seqlens_q), (size_t)n_seqs + 1));
        p.pv_plan = loc == BRN_MEM_DEVICE ? plan_workspace : reinterpret_cast<int*>(st.dalloc(pl.plan_ints));
        p.pv_n_seqs = n_seqs; p.pv_total_q = total_q;
        p.y = stage_inout(st, y, nq, stream);
        // the layout of the split entry at batch 1, seq_q = total_q; each workgroup's own seq_q, seq_kv and causal_off come from the plan
        p.batch = 1; p.heads = heads; p.kv_heads = kv_heads; p.seq_q = total_q; p.seq_kv = max_kv_len; p.head_dim = head_dim;
        const long d = head_dim;
        p.q_ss = heads * d; p.q_sh = d; p.q_sb = total_q * p.q_ss;
        p.kv_ss = kv_heads * d; p.kv_sh = d; p.kv_sb = 0;
        p.page_stride = (long)page_size * p.kv_ss; p.page_log2 = page_log2; p.n_pages = n_pages; p.max_pages = max_pages;
        p.kv_type = pool_type;
        p.causal = causal; p.causal_off = 0;
        p.scale = scale_or_default(scale, head_dim);
        p.s16 = s16;
        p.kv_splits = pl.S; p.tiles_per_split = pl.tps;
        if (lse) p.lse = stage_inout(st, lse, R, stream);
        if (need) {
            p.o_part = stage_inout(st, ws, need, stream);
            p.lse2_part = p.o_part + (size_t)pl.S * R * head_dim;
        }
        BRN_HIP(launch_flash_attention(p, (hipStream_t)stream));
        st.finish();
    });
}

brn_status brn_kv_cache_append_varlen(const float* k_new, const float* v_new, const int* cu_seqlens_q, int total_q, int n_seqs, int kv_heads, int head_dim,
                                      void* k_pages, void* v_pages, int pool_type, const float* k_scale, const float* v_scale, const int* block_table,
                                      const int* kv_lens, int* kv_lens_out, int n_pages, int page_size, int max_pages, int* plan_workspace, size_t plan_ints,
                                      brn_mem loc, int device, void* stream) {
    return guarded([&] {
        const char* who = APPEND_VARLEN;
        if (!k_new || !v_new || !k_pages || !v_pages) fail(BRN_ERR_INVALID_ARG, "%s: null k_new, v_new, k_pages or v_pages", who);
        if (!block_table || !kv_lens || !cu_seqlens_q) fail(BRN_ERR_INVALID_ARG, "%s: null block_table, kv_lens or cu_seqlens_q", who);
        pool_type_check(who, pool_type, k_scale, v_scale);
        if (!(head_dim == 32 || head_dim == 64 || head_dim == 128))
            fail(BRN_ERR_INVALID_ARG, "%s: head_dim %d unsupported (head_dim must be 32, 64 or 128)", who, head_dim);
        if (kv_heads < 1) fail(BRN_ERR_INVALID_ARG, "%s: kv_heads %d unsupported (kv_heads >= 1)", who, kv_heads);
        pack_check(who, total_q, n_seqs, 1);
        const int page_log2 = paged_pool_check(who, n_pages, page_size, max_pages);
        if ((long long)max_pages * page_size > 0x7fffffffLL)
            fail(BRN_ERR_INVALID_ARG, "%s: max_pages %d of page_size %d too large (max_pages * page_size < 2^31)", who, max_pages, page_size);
        // the grid: a thread per 8 elements of a new row of K and of V
        if (((long long)total_q * kv_heads * (head_dim / 8) + 255) / 256 > 0x7fffffffLL)
            fail(BRN_ERR_INVALID_ARG, "%s: total_q %d, kv_heads %d too large (total_q * kv_heads * head_dim / 8 / 256 < 2^31)", who, total_q, kv_heads);
        plan_workspace_check(who, plan_workspace, plan_ints, n_seqs);
        const size_t nnew = (size_t)total_q * kv_heads * head_dim, npool = (size_t)n_pages * page_size * kv_heads * head_dim;
        const size_t pool_floats = npool * kv_type_bytes(pool_type) / 4, ntab = (size_t)n_seqs * max_pages, nplan = fa_pv_plan_ints(n_seqs);
        const struct { const void* p; size_t n; const char* name; } ins[] = {{k_new, nnew * 4, "k_new"}, {v_new, nnew * 4, "v_new"}, {block_table, ntab * 4, "block_table"},
                                                                             {kv_lens, (size_t)n_seqs * 4, "kv_lens"}, {cu_seqlens_q, ((size_t)n_seqs + 1) * 4, "cu_seqlens_q"},
                                                                             {k_scale, (size_t)kv_heads * 4, "k_scale"}, {v_scale, (size_t)kv_heads * 4, "v_scale"}};
        for (const auto& in : ins) {
            if (bytes_overlap(in.p, in.n, k_pages, pool_floats * 4) || bytes_overlap(in.p, in.n, v_pages, pool_floats * 4))
                fail(BRN_ERR_INVALID_ARG, "%s: %s must not overlap the pool", who, in.name);
            if (bytes_overlap(in.p, in.n, plan_workspace, nplan * 4)) fail(BRN_ERR_INVALID_ARG, "%s: plan_workspace must not overlap %s", who, in.name);
        }
        if (bytes_overlap(k_pages, pool_floats * 4, v_pages, pool_floats * 4)) fail(BRN_ERR_INVALID_ARG, "%s: k_pages and v_pages must not overlap", who);
        if (bytes_overlap(k_pages, pool_floats * 4, plan_workspace, nplan * 4) || bytes_overlap(v_pages, pool_floats * 4, plan_workspace, nplan * 4))
            fail(BRN_ERR_INVALID_ARG, "%s: plan_workspace must not overlap the pool", who);
        if (kv_lens_out && kv_lens_out != kv_lens) {
            for (const auto& in : ins)
                if (bytes_overlap(in.p, in.n, kv_lens_out, (size_t)n_seqs * 4)) fail(BRN_ERR_INVALID_ARG, "%s: kv_lens_out must not overlap %s (kv_lens itself, the in-place form, excepted)", who, in.name);
            if (bytes_overlap(k_pages, pool_floats * 4, kv_lens_out, (size_t)n_seqs * 4) || bytes_overlap(v_pages, pool_floats * 4, kv_lens_out, (size_t)n_seqs * 4))
                fail(BRN_ERR_INVALID_ARG, "%s: kv_lens_out must not overlap the pool", who);
        }
        if (kv_lens_out && bytes_overlap(kv_lens_out, (size_t)n_seqs * 4, plan_workspace, nplan * 4)) fail(BRN_ERR_INVALID_ARG, "%s: plan_workspace must not overlap kv_lens_out", who);
        if (loc == BRN_MEM_DEVICE && !all_aligned16({k_new, v_new, static_cast<const float*>(k_pages), static_cast<const float*>(v_pages)}))
            fail(BRN_ERR_INVALID_ARG, "%s: device k_new, v_new, k_pages and v_pages must be 16-byte aligned", who);
        if ((reinterpret_cast<uintptr_t>(block_table) | reinterpret_cast<uintptr_t>(kv_lens) | reinterpret_cast<uintptr_t>(kv_lens_out) | reinterpret_cast<uintptr_t>(cu_seqlens_q)) & 3)
            fail(BRN_ERR_INVALID_ARG, "%s: block_table, kv_lens, kv_lens_out and cu_seqlens_q must be 4-byte aligned", who);
        if (loc == BRN_MEM_DEVICE && ((reinterpret_cast<uintptr_t>(k_scale) | reinterpret_cast<uintptr_t>(v_scale)) & 3))
            fail(BRN_ERR_INVALID_ARG, "%s: device k_scale and v_scale must be 4-byte aligned", who);
        ensure_device(device);
        Staging st(stream, loc);
        KvAppendParams p{};
        if (k_scale) p.k_scale = st.in(k_scale, (size_t)kv_heads);
        if (v_scale) p.v_scale = st.in(v_scale, (size_t)kv_heads);
        p.k_new = st.in(k_new, nnew); p.v_new = st.in(v_new, nnew);
        p.k_pages = stage_inout(st, static_cast<float*>(k_pages), pool_floats, stream);       // BRN_MEM_HOST: the pool goes up whole and comes back whole
        p.v_pages = stage_inout(st, static_cast<float*>(v_pages), pool_floats, stream);
        p.block_table = reinterpret_cast<const int*>(st.in(reinterpret_cast<const float*>(block_table), ntab));
        p.kv_lens = reinterpret_cast<const int*>(st.in(reinterpret_cast<const float*>(kv_lens), (size_t)n_seqs));
        if (kv_lens_out) p.kv_lens_out = reinterpret_cast<int*>(st.out(reinterpret_cast<float*>(kv_lens_out), (size_t)n_seqs));
        p.pv_cu = reinterpret_cast<const int*>(st.in(reinterpret_cast<const float*>(cu_seqlens_q), (size_t)n_seqs + 1));
        p.pv_plan = loc == BRN_MEM_DEVICE ? plan_workspace : reinterpret_cast<int*>(st.dalloc(nplan));
        p.pv_n_seqs = n_seqs; p.pv_total_q = total_q;
        p.kv_type = pool_type;
        p.batch = n_seqs; p.seq_new = 0; p.kv_heads = kv_heads; p.head_dim = head_dim;
        const long d = head_dim;
        p.new_ss = kv_heads * d; p.new_sh = d; p.new_sb = 0;
        p.kv_ss = kv_heads * d; p.page_stride = (long)page_size * p.kv_ss;
        p.page_log2 = page_log2; p.n_pages = n_pages; p.max_pages = max_pages; p.cap = max_pages * page_size;
        BRN_HIP(launch_kv_cache_append(p, (hipStream_t)stream));
        st.finish();
    });
}

brn_status brn_patch_merging_forward(const float* x, int B, int H, int W, int C, const float* ng, const float* nb,
                                     const float* rw, float* y, brn_mem loc, int device, void* stream) {
    return guarded([&] {
        if (!x || !ng || !nb || !rw || !y || B < 1 || H < 1 || W < 1) fail(BRN_ERR_INVALID_ARG, "bad argument");
        if (C % 32 || 4 * C > 3072) fail(BRN_ERR_INVALID_ARG, "patch merging width %d unsupported", C);
        ensure_device(device);
        DeviceOwner own;
        LNW ln; ln.C = 4 * C; ln.g = own.upload(ng, 4 * C); ln.b = own.upload(nb, 4 * C);
        GemmW red = make_linear(own, WeightBuild{}, rw, nullptr, 2 * C, 4 * C);   // fp32 in every op mode
        const int Ho = (H + 1) / 2, Wo = (W + 1) / 2, M2 = B * Ho * Wo;
        Staging st(stream, loc);
        const float* dx = st.in(x, (size_t)B * H * W * C);
        float* dy = st.out(y, (size_t)M2 * 2 * C);
        with_arena((hipStream_t)stream, [&](Ctx& c) {
            float* pm = c.arena->alloc((size_t)M2 * 4 * C);
            if (!c.dry) {
                LayerNormParams p{};
                p.x = dx; p.y = pm; p.rows = M2; p.C = 4 * C; p.gamma = ln.g; p.beta = ln.b; p.eps = 1e-5f;
                p.ldy = 4 * C; p.mode = 1; p.H = H; p.W = W; p.Cin = C;
                BRN_HIP(launch_layernorm(p, c.stream));
            }
            run_gemm(c, red, GemmIO(pm, M2, 4 * C).to(dy, 2 * C));
        });
        st.finish();
    });
}

brn_status brn_aspp_deformable_forward(const brn_named_tensor* weights, size_t n, const char* prefix, int in_channels, int out_channels, int mode,
                                       const float* x, int B, int H, int W, float* y, brn_mem loc, int device, void* stream) {
    return guarded([&] {
        if (!weights || !x || !y || B < 1 || H < 1 || W < 1 || in_channels < 1 || out_channels < 0) fail(BRN_ERR_INVALID_ARG, "bad argument");
        if (mode != BRN_DEFORM_REFERENCE_CPU && mode != BRN_DEFORM_DEFORMABLE) fail(BRN_ERR_INVALID_ARG, "unknown deform mode %d", mode);
        ensure_device(device);
        DeviceOwner own;
        const WeightBuild wb = g_op;
        WeightTable wt(weights, n);
        ASPPW a;
        build_aspp_weights(wt, prefix ? prefix : "", mode, own, wb, a, in_channels, out_channels);
        Staging st(stream, loc);
        const float* dx = st.in(x, (size_t)B * a.ic * H * W);
        float* dy = st.out(y, (size_t)B * a.oc * H * W);
        through_nhwc(stream, op_s16(wb), dx, B, a.ic, a.icp, H, W, dy, a.oc, H, W, [&](Ctx& c, const Map& T, const Map& U) { aspp_forward(c, a, T, U, mode); });
        st.finish();
    });
}

brn_status brn_decblk_forward(const brn_named_tensor* weights, size_t n, const char* prefix, int cin, int cout, int inter, int use_aspp, int mode,
                              const float* x, int B, int H, int W, float* y, brn_mem loc, int device, void* stream) {
    return guarded([&] {
        if (!weights || !x || !y || B < 1 || H < 1 || W < 1 || cin < 1 || cout < 1 || inter < 0) fail(BRN_ERR_INVALID_ARG, "bad argument");
        if (mode != BRN_DEFORM_REFERENCE_CPU && mode != BRN_DEFORM_DEFORMABLE) fail(BRN_ERR_INVALID_ARG, "unknown deform mode %d", mode);
        ensure_device(device);
        DeviceOwner own;
        const WeightBuild wb = g_op;
        WeightTable wt(weights, n);
        DecBlkW blk;
        build_decblk_weights(wt, prefix ? prefix : "", cin, cout, mode, own, wb, blk, use_aspp != 0, inter > 0 ? inter : 64);
        const int cinp = blk.conv_in.Cinp;                   // in_channels rounded up to the kernels' channel granule (zero weights there)
        Staging st(stream, loc);
        const float* dx = st.in(x, (size_t)B * cin * H * W);
        float* dy = st.out(y, (size_t)B * cout * H * W);
        through_nhwc(stream, op_s16(wb), dx, B, cin, cinp, H, W, dy, cout, H, W, [&](Ctx& c, const Map& X, const Map& Y) { decblk_forward(c, blk, X, Y, mode); });
        st.finish();
    });
}

brn_status brn_deform_conv2d_forward(const float* x, int B, int C, int H, int W, const float* offset_w, const float* offset_b,
                                     const float* mod_w, const float* mod_b, const float* w, const float* bias, int O, int k,
                                     int stride, int pad, int mode, float* y, brn_mem loc, int device, void* stream) {
    return guarded([&] {
        if (!x || !offset_w || !offset_b || !mod_w || !mod_b || !w || !y || k < 1 || stride < 1 || pad < 0)
            fail(BRN_ERR_INVALID_ARG, "bad argument");
        if (mode == BRN_DEFORM_REFERENCE_CPU) {
            // deform_conv.rs:95-98: offsets and modulator are computed and discarded; the result is regular_conv(x)
            brn_status s = brn_conv2d_forward(x, B, C, H, W, w, bias, O, k, k, stride, pad, 1, nullptr, nullptr, nullptr,
                                              nullptr, 0.f, BRN_ACT_NONE, y, loc, device, stream);
            if (s != BRN_OK) fail(s, "%s", brn_last_error());
            return;
        }
        if (mode != BRN_DEFORM_DEFORMABLE) fail(BRN_ERR_INVALID_ARG, "unknown deform mode %d", mode);
        const int Ho = (H + 2 * pad - k) / stride + 1, Wo = (W + 2 * pad - k) / stride + 1, kk = k * k;
        ensure_device(device);
        DeviceOwner own;
        // compute mode BRN_BF16 at op level (brn_set_op_compute): bf16 map in / out as inside the model, offsets / modulator fp32, the
        // gather on kernels/deform_bf16.hip where the shape allows.  The plane modes (f32_split3 / f32_split2 / f32_half2) build both convs with
        // the op's planes, as the ASPP and decoder-block entries do: the offset / modulator conv and the gather run on the split kernels
        // (launch_gemm: deform_on_split).  Mode f32 and whatever those do not cover run the fp32-MFMA gather kernel.
        // Any in_channels (deform_conv.rs:29-36): the channels-last map is padded with zero channels to the kernels' granule (32; 64 for
        // the bf16 gather kernel), the weights with zero columns
        const bool bf = g_op.planes == BUILD_BF16 && (O % 8) == 0;
        const int Cp = (C + (bf ? 63 : 31)) / (bf ? 64 : 32) * (bf ? 64 : 32);
        const bool pl = g_op.planes == 2 || g_op.planes == 3 || g_op.planes == BUILD_HALF2;
        const WeightBuild wb = (bf || pl) ? g_op : WeightBuild{};
        std::vector<float> w3((size_t)3 * kk * C * kk), b3((size_t)3 * kk);
        memcpy(w3.data(), offset_w, (size_t)2 * kk * C * kk * sizeof(float));
        memcpy(w3.data() + (size_t)2 * kk * C * kk, mod_w, (size_t)kk * C * kk * sizeof(float));
        memcpy(b3.data(), offset_b, (size_t)2 * kk * sizeof(float));
        memcpy(b3.data() + 2 * kk, mod_b, (size_t)kk * sizeof(float));
        GemmW om = make_conv_nhwc(own, wb, w3.data(), b3.data(), 3 * kk, C, Cp, k, k, stride, pad, 1);
        om.mode = GEMM_CONV_NHWC;
        GemmW reg = make_conv_nhwc(own, wb, w, bias, O, C, Cp, k, k, stride, pad, 1);
        reg.mode = GEMM_DEFORM_NHWC;
        attach_deform_frags(own, wb, reg, w);
        Staging st(stream, loc);
        const float* dx = st.in(x, (size_t)B * C * H * W);
        float* dy = st.out(y, (size_t)B * O * Ho * Wo);
        through_nhwc(stream, op_s16(wb), dx, B, C, Cp, H, W, dy, O, Ho, Wo, [&](Ctx& c, const Map& X, const Map& Y) {
            const int ldom = (3 * kk + 3) / 4 * 4;
            const Map OM = Map(c.arena->alloc((size_t)B * Ho * Wo * ldom), B, Ho, Wo, ldom).window(0, 3 * kk);
            run_conv(c, om, X, OM, ConvOpts().f32());
            const bool fused_sig = deform_fused_sigmoid(c, reg);
            if (!c.dry && !fused_sig) BRN_HIP(launch_mod_sigmoid2(OM.p, (size_t)B * Ho * Wo, ldom, 2 * kk, 3 * kk, c.stream));
            run_conv(c, reg, X, Y, ConvOpts().offsets(OM, 2 * kk, fused_sig));
        });
        st.finish();
    });
}

// whether the product of the (positive) factors stays below 2^31, without overflowing on the way
static bool count_below_2_31(std::initializer_list<long long> factors) {
    long long n = 1;
    for (long long f : factors) {
        if (f < 1 || f > 0x7fffffffLL) return false;
        n *= f;
        if (n > 0x7fffffffLL) return false;
    }
    return true;
}

brn_status brn_deform_conv2d_offsets_forward(const float* x, int B, int C, int H, int W, const float* offset, const float* mask, const float* w,
                                             const float* bias, int O, int kh, int kw, int stride_h, int stride_w, int pad_h, int pad_w, int dil_h,
                                             int dil_w, int offset_groups, float* y, brn_mem loc, int device, void* stream) {
    return guarded([&] {
        const char* who = "deform conv offsets";
        const int G = offset_groups;
        // every refusal before the device
        if (!x || !offset || !w || !y) fail(BRN_ERR_INVALID_ARG, "%s: null x, offset, w or y (only mask and bias may be NULL)", who);
        if (B < 1 || C < 1 || H < 1 || W < 1 || O < 1 || kh < 1 || kw < 1)
            fail(BRN_ERR_INVALID_ARG, "%s: B %d, C %d, H %d, W %d, O %d, kh %d, kw %d unsupported (every size >= 1)", who, B, C, H, W, O, kh, kw);
        if (stride_h < 1 || stride_w < 1) fail(BRN_ERR_INVALID_ARG, "%s: stride (%d, %d) unsupported (stride_h, stride_w >= 1)", who, stride_h, stride_w);
        if (dil_h < 1 || dil_w < 1) fail(BRN_ERR_INVALID_ARG, "%s: dilation (%d, %d) unsupported (dil_h, dil_w >= 1)", who, dil_h, dil_w);
        if (pad_h < 0 || pad_w < 0) fail(BRN_ERR_INVALID_ARG, "%s: padding (%d, %d) unsupported (pad_h, pad_w >= 0)", who, pad_h, pad_w);
        if (G < 1 || C % G) fail(BRN_ERR_INVALID_ARG, "%s: offset_groups %d unsupported with C %d (offset_groups >= 1, C %% offset_groups == 0)", who, G, C);
        if ((long long)H + 2LL * pad_h > 0x7fffffffLL || (long long)W + 2LL * pad_w > 0x7fffffffLL)
            fail(BRN_ERR_INVALID_ARG, "%s: padded map too large (H + 2 pad_h, W + 2 pad_w < 2^31)", who);
        const long long Ho = deform_out_size(H, kh, stride_h, pad_h, dil_h), Wo = deform_out_size(W, kw, stride_w, pad_w, dil_w);
        if (Ho < 1 || Wo < 1)
            fail(BRN_ERR_INVALID_ARG, "%s: empty output, Ho %lld, Wo %lld (Ho, Wo >= 1: the dilated kernel must fit the padded map)", who, Ho, Wo);
        if (!count_below_2_31({B, Ho, Wo})) fail(BRN_ERR_INVALID_ARG, "%s: too many output pixels (B * Ho * Wo < 2^31)", who);
        if (!count_below_2_31({B, C, H, W})) fail(BRN_ERR_INVALID_ARG, "%s: x too large (B * C * H * W < 2^31 elements)", who);
        if (!count_below_2_31({B, 2, G, kh, kw, Ho, Wo})) fail(BRN_ERR_INVALID_ARG, "%s: offset too large (B * 2 * G * kh * kw * Ho * Wo < 2^31 elements)", who);
        if (!count_below_2_31({O, C, kh, kw}) || !count_below_2_31({kh, kw, (long long)C + 63}))
            fail(BRN_ERR_INVALID_ARG, "%s: w too large (O * C * kh * kw and kh * kw * (C + 63) < 2^31 elements)", who);
        if (!count_below_2_31({B, O, Ho, Wo})) fail(BRN_ERR_INVALID_ARG, "%s: y too large (B * O * Ho * Wo < 2^31 elements)", who);
        const int taps = kh * kw, ho = (int)Ho, wo = (int)Wo;
        const size_t nx = (size_t)B * C * H * W, noff = (size_t)B * 2 * G * taps * ho * wo, nmask = noff / 2, ny = (size_t)B * O * ho * wo;
        if (floats_overlap(x, nx, y, ny) || floats_overlap(offset, noff, y, ny) || floats_overlap(mask, nmask, y, ny) ||
            (loc == BRN_MEM_HOST && (floats_overlap(w, (size_t)O * C * taps, y, ny) || floats_overlap(bias, (size_t)O, y, ny))))
            fail(BRN_ERR_INVALID_ARG, "%s: y must not overlap an input", who);
        ensure_device(device);
        DeformOffsetsParams a{};
        a.B = B; a.C = C; a.H = H; a.W = W; a.kh = kh; a.kw = kw; a.stride_h = stride_h; a.stride_w = stride_w; a.pad_h = pad_h; a.pad_w = pad_w;
        a.dil_h = dil_h; a.dil_w = dil_w; a.G = G; a.Ho = ho; a.Wo = wo;
        DeviceOwner own;
        DeformOffsetsPlan plan = deform_offsets_prepare(own, g_op, a, w, bias, O);
        Staging st(stream, loc);
        const float* dx = st.in(x, nx);
        plan.geo.offset = st.in(offset, noff);
        plan.geo.mask = mask ? st.in(mask, nmask) : nullptr;
        float* dy = st.out(y, ny);
        through_nhwc(stream, plan.s16, dx, B, C, plan.Cp, H, W, dy, O, ho, wo, [&](Ctx& c, const Map& X, const Map& Y) { deform_offsets_route(c, plan, X, Y); });
        st.finish();
    });
}

}  // extern "C"
