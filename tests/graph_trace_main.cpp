// graph_trace_main.cpp — runs the forward graph (csrc/brn_graph*.cpp) on the CPU against the logging stubs of graph_trace_stubs.cpp and prints
// what it enqueues.  The models are descriptors only: every GemmW / LNW field the graph reads is filled as brn_weights.cpp fills it for the
// Swin-L channel plan (validate_config, brn_api.cpp), the pointers are fake (graph_trace.h), nothing is packed or uploaded.
#include "graph_trace.h"
#include "brn_host.h"
#include <cstdio>
#include <cstring>
#include <iterator>

using namespace brn;

namespace {

uintptr_t g_next_w = 0;
template <class T = float> T* fake_w() { return reinterpret_cast<T*>(trace::W_BASE + trace::W_STRIDE * g_next_w++); }

// ---- descriptors, as brn_weights.cpp sets them -------------------------------------------------------------------------------------------
// attach_planes (brn_weights.cpp:94-110) with pack_s16_storage's rows / ld / chunk-major rule (brn_pack.h:100-105); rows = roundup(N, 128)
void attach_planes(WeightBuild wb, GemmW& g) {
    const int rows = roundup(g.N, 128);
    if (wb.planes <= 0) return;
    if (wb.planes == BUILD_BF16) {
        const int taps = g.mode == GEMM_CONV_NHWC ? g.kh * g.kw : 0;
        g.wb = fake_w<void>(); g.wb_rows = roundup(rows, 256); g.wb_ld = roundup(g.K, 64);
        g.wb_chunk_major = taps > 0 && g.Cinp % 64 == 0 && g.Cinp > 64 && taps * g.Cinp == g.K;
    } else if (wb.planes == BUILD_HALF2) {
        g.wp = fake_w<void>(); g.planes = 2; g.wp_rows = rows; g.half = 1;
        g.w_scale = ldexpf(1.f, 12 + g.N % 3);          // (a power of two per tensor; the packer derives it from max |w|)
    } else {
        g.wp = fake_w<void>(); g.planes = wb.planes; g.wp_rows = rows;
    }
}
// attach_dense_frags (brn_weights.cpp:151-154)
void attach_dense_frags(WeightBuild wb, GemmW& g) {
    if (wb.planes != BUILD_BF16 || g.mode != GEMM_DENSE || (g.K != 192 && g.K != 384) || g.N < 192 || g.N % 192) return;
    g.wf = fake_w<void>();
}
// attach_deform_frags (brn_weights.cpp:147-150)
void attach_deform_frags(WeightBuild wb, GemmW& g) {
    if (wb.planes != BUILD_BF16 || g.Cinp % 64 || g.K != g.kh * g.kw * g.Cinp) return;
    g.wf = fake_w<void>();
}
// make_linear (brn_weights.cpp:113-124)
GemmW linear(WeightBuild wb, int N, int K, bool bias) {
    GemmW g;
    g.N = N; g.K = K; g.Kreal = K; g.Cin = K; g.Cinp = K; g.mode = GEMM_DENSE;
    g.w = fake_w();
    attach_planes(wb, g);
    attach_dense_frags(wb, g);
    if (bias) g.bias = fake_w();
    return g;
}
// make_conv_nhwc (brn_weights.cpp:126-144)
GemmW conv_nhwc(WeightBuild wb, int O, int Cin, int cinp, int k, int pad, bool bias) {
    GemmW g;
    g.N = O; g.K = k * k * cinp; g.Kreal = k * k * Cin; g.Cin = Cin; g.Cinp = cinp;
    g.kh = k; g.kw = k; g.stride = 1; g.pad = pad; g.dil = 1;
    g.mode = (k == 1 && pad == 0) ? GEMM_DENSE : GEMM_CONV_NHWC;
    g.w = fake_w();
    attach_planes(wb, g);
    if (g.mode == GEMM_DENSE && cinp == Cin) attach_dense_frags(wb, g);
    if (bias) g.bias = fake_w();
    return g;
}
// make_conv_gather (brn_weights.cpp:156-166)
GemmW conv_gather(int O, int Cin, int k, int stride) {
    GemmW g;
    g.N = O; g.Kreal = Cin * k * k; g.K = roundup(g.Kreal, 32); g.Cin = Cin; g.Cinp = Cin;
    g.kh = k; g.kw = k; g.stride = stride; g.pad = 0; g.dil = 1; g.mode = GEMM_GATHER_NCHW;
    g.w = fake_w(); g.bias = fake_w();
    return g;
}
// fold_bn (brn_weights.cpp:170-182)
void fold_bn(GemmW& g) { g.scale = fake_w(); g.shift = fake_w(); g.bias = nullptr; }
// conv_bn (brn_weights.cpp:259-272): always with a BN in the model
GemmW conv_bn(WeightBuild wb, int O, int Cin, int cinp, int k, int pad, int act) {
    GemmW g = conv_nhwc(wb, O, Cin, cinp, k, pad, false);
    fold_bn(g);
    g.act = act;
    return g;
}
LNW ln(int C) { LNW l; l.C = C; l.g = fake_w(); l.b = fake_w(); return l; }      // get_ln (brn_weights.cpp:193-199)

// build_swin_weights (brn_weights.cpp:207-256): Swin-L widths and heads, depths [2,2,2,2] (a shifted block in every stage)
void build_swin(WeightBuild wb, SwinW& out, int window = 12) {
    const int E = 192;
    out.embed_dim = E; out.window = window; out.patch = 4; out.in_ch = 3;
    out.patch_proj = conv_gather(E, 3, 4, 4);
    out.patch_norm = ln(E);
    for (int i = 0; i < 4; ++i) {
        SwinStageW& st = out.stages[i];
        const int C = E << i, heads = 6 << i, hidden = 4 * C;
        st.C = C; st.heads = heads;
        st.blocks.resize(2);
        for (SwinBlockW& bk : st.blocks) {
            bk.heads = heads;
            bk.norm1 = ln(C); bk.norm2 = ln(C);
            bk.qkv = linear(wb, 3 * C, C, true);
            bk.proj = linear(wb, C, C, true);
            bk.fc1 = linear(wb, hidden, C, true); bk.fc1.act = ACT_GELU_ERF;
            bk.fc2 = linear(wb, C, hidden, true);
            bk.rel_table = fake_w();
        }
        st.has_down = i < 3;
        if (st.has_down) { st.down_norm = ln(4 * C); st.reduction = linear(wb, 2 * C, 4 * C, false); }
        st.out_norm = ln(C);
    }
}
// build_aspp_weights (brn_weights.cpp:291-370)
void build_aspp(WeightBuild wb, int deform_mode, ASPPW& a, int IC) {
    const int OC = IC, PL = 256, ICP = roundup(IC, wb.planes == BUILD_BF16 ? 64 : 32);
    a.ic = IC; a.icp = ICP; a.oc = OC;
    const int ks[4] = {1, 1, 3, 7};
    for (int i = 0; i < 4; ++i) {
        const int k = ks[i], kk = k * k;
        DeformW& d = a.d[i];
        d.k = k;
        d.regular = conv_bn(wb, PL, IC, ICP, k, k / 2, ACT_RELU);
        if (deform_mode == BRN_DEFORM_DEFORMABLE) {
            d.regular.mode = GEMM_DEFORM_NHWC;
            attach_deform_frags(wb, d.regular);
            d.offmod = conv_nhwc(wb, roundup(3 * kk, 8), IC, ICP, k, k / 2, true);   // offmod.N = 3 k^2 rounded up to 8 (brn_weights.cpp:312-321)
        }
    }
    if (deform_mode == BRN_DEFORM_REFERENCE_CPU) {
        a.k1pair = linear(wb, 2 * PL, ICP, false);
        fold_bn(a.k1pair);
        a.k1pair.act = ACT_RELU;
    }
    a.gap_w = fake_w(); a.gap_scale = fake_w(); a.gap_shift = fake_w();
    a.conv1_full = fake_w();
    a.conv1_main = linear(wb, OC, 4 * PL, false);
    fold_bn(a.conv1_main);
    a.conv1_main.act = ACT_RELU;
}
// build_decblk_weights (brn_weights.cpp:274-288)
void build_decblk(WeightBuild wb, int cin, int cout, int deform_mode, DecBlkW& out) {
    const int IC = 64, gran = wb.planes == BUILD_BF16 ? 64 : 32;
    out.cin = cin; out.cout = cout; out.has_aspp = true; out.ic = IC; out.icp = roundup(IC, gran);
    out.conv_in = conv_bn(wb, IC, cin, roundup(cin, gran), 3, 1, ACT_RELU);
    out.conv_out = conv_bn(wb, cout, IC, out.icp, 3, 1, ACT_NONE);
    build_aspp(wb, deform_mode, out.aspp, IC);
}
// build_decoder_weights (brn_weights.cpp:373-484)
void build_decoder(WeightBuild wb, int deform_mode, DecoderW& out) {
    const int ipt_out[5] = {48, 96, 192, 384, 384}, ipt_in[5] = {3, 48, 192, 768, 3072};
    for (int i = 1; i < 5; ++i) {
        out.ipt[i].conv1 = conv_nhwc(wb, 64, ipt_in[i], roundup(ipt_in[i], 32), 3, 1, true);
        const int opad = (wb.planes == BUILD_BF16 && ipt_out[i] == 96) ? 128 : ipt_out[i];   // brn_weights.cpp:394-404
        out.ipt[i].conv_out = conv_nhwc(wb, opad, 64, 64, 3, 1, true);
    }
    const int dec_out[4] = {1536, 768, 384, 192}, dec_in[4] = {3072 + 384, 1536 + 384, 768 + 192, 384 + 96};
    for (int i = 0; i < 4; ++i) build_decblk(wb, dec_in[i], dec_out[i], deform_mode, out.dec[i]);
    for (int i = 0; i < 3; ++i) out.lat[i] = linear(wb, dec_out[i], dec_out[i], true);
    for (int i = 0; i < 3; ++i) {
        out.gdt[i] = conv_bn(wb, 16, dec_out[i], dec_out[i], 3, 1, ACT_RELU);
        out.gdt_attn_w[i] = fake_w(); out.gdt_attn_b[i] = 0.25f * (float)(i + 1);
    }
    out.out_w = fake_w(); out.out_b = -0.5f;
    out.head_k = fake_w(); out.head_b = fake_w();
}

// brn_model_create (brn_api.cpp:344-359): the compute modes as (backbone build, decoder build, Model::bf16, Model::dec_bf16)
struct Mode { const char* name; WeightBuild bb, dec; int bf16, dec_bf16; };
const Mode kModes[7] = {
    {"fp32", {0, false}, {0, false}, 0, 0},
    {"f32_split2", {2, false}, {2, false}, 0, 0},
    {"f32_half2", {BUILD_HALF2, false}, {BUILD_HALF2, false}, 0, 0},
    {"f32_split3", {3, false}, {3, false}, 0, 0},
    {"bf16", {BUILD_BF16, false}, {BUILD_BF16, false}, 1, 1},
    {"f16", {BUILD_BF16, true}, {BUILD_BF16, true}, 2, 2},
    {"bf16_dec_split2", {BUILD_BF16, false}, {2, false}, 1, 0},
};
void build_model(const Mode& md, int deform_mode, Model& m) {
    g_next_w = 0;
    memset(&m.cfg, 0, sizeof m.cfg);
    m.cfg.deform_mode = deform_mode;
    m.bf16 = md.bf16; m.dec_bf16 = md.dec_bf16;
    build_swin(md.bb, m.swin);
    build_decblk(md.dec, 5760, 3072, deform_mode, m.squeeze);       // squeeze_module.0: x4 channels -> lateral[3]
    build_decoder(md.dec, deform_mode, m.dec);
    m.has_decoder = true;
}

// ---- runs ----------------------------------------------------------------------------------------------------------------------------
float* const kImg = reinterpret_cast<float*>(trace::IMG_BASE);
float* const kOut = reinterpret_cast<float*>(trace::OUT_BASE);

Arena real_arena() { Arena a; a.base = reinterpret_cast<char*>(trace::ARENA_BASE); a.cap = trace::ARENA_CAP; return a; }
BranchSet branch_set() {
    BranchSet bs;
    for (int k = 0; k < BRN_AUX_STREAMS; ++k) { bs.stream[k] = trace::stream(1 + k); bs.fork_ev[k] = trace::event(trace::FORK_BASE, k); bs.join_ev[k] = trace::event(trace::JOIN_BASE, k); }
    return bs;
}

void run_dry(Model& m, int B, int H, int W) {
    trace::set_quiet(true);
    Arena a; a.dry = true;
    Ctx c{&a, nullptr, true, false, nullptr, nullptr, nullptr};
    c.bf16 = m.bf16;
    model_forward(m, c, nullptr, B, H, W, nullptr, 0);
    printf("dry: peak=%zu top=%zu\n", a.peak, a.top);
}
void run_branches(Model& m, int B, int H, int W) {
    trace::set_quiet(false);
    Arena a = real_arena();
    BranchSet bs = branch_set();
    Ctx c{&a, trace::stream(0), false, false, nullptr, nullptr, nullptr};
    c.bf16 = m.bf16; c.br = &bs; c.br_mask = ~0u;
    model_forward(m, c, kImg, B, H, W, kOut, 0);
    printf("branches: peak=%zu top=%zu pending=%u\n", a.peak, a.top, c.pending);
}
void run_profile(Model& m, int B, int H, int W) {
    trace::set_quiet(true);            // the records say what was launched, in order
    trace::reset_events();
    Arena a = real_arena();
    std::vector<LaunchRecord> records;
    std::vector<hipEvent_t> pool; size_t next = 0;
    for (int i = 0; i < 6; ++i) m.stage_ev[i] = trace::event(trace::STAGE_BASE, i);
    m.stage_ev_ok = true;
    Ctx c{&a, trace::stream(0), false, true, &records, &pool, &next};
    c.bf16 = m.bf16;
    model_forward(m, c, kImg, B, H, W, kOut, 1);
    m.stage_ev_ok = false;
    printf("profile: peak=%zu events=%zu records=%zu\n", a.peak, next, records.size());
    for (const LaunchRecord& r : records) printf("record fam=%d flop=%.17g bytes=%.17g M=%d N=%d K=%d region=%d\n", r.fam, r.flop, r.bytes, r.M, r.N, r.K, r.region);
}

// the forms brn_ops.cpp calls the graph pieces in
void run_op_forms() {
    trace::set_quiet(false);
    g_next_w = 0;
    float* const x = kImg;
    auto ctx = [](Arena& a, int bf16) { Ctx c{&a, trace::stream(0), false, false, nullptr, nullptr, nullptr}; c.bf16 = bf16; return c; };
    for (const Mode& md : {kModes[0], kModes[1], kModes[2], kModes[4], kModes[5]}) {
        printf("== ops %s\n", md.name);
        Arena a = real_arena();
        Ctx c = ctx(a, md.bf16);
        const WeightBuild wb = md.bb;
        // brn_window_attention_forward: window 12 shifted and window 7
        SwinBlockW bk;
        bk.heads = 6; bk.qkv = linear(wb, 576, 192, true); bk.proj = linear(wb, 192, 192, true); bk.rel_table = fake_w();
        swin_attention(c, bk, x, 1, 20, 30, 192, 6, kOut, nullptr, 12);
        swin_attention(c, bk, x, 2, 9, 5, 192, 3, kOut, nullptr, 7);
        // brn_linear_forward: residual, fp32 C / R in the 16-bit modes
        GemmW g = linear(wb, 200, 96, true);
        g.act = ACT_RELU;
        run_gemm(c, g, GemmIO(x, 77, 96).to(kOut, 200).add(x + 1000, 200).f32(md.bf16 ? 1 : 0, md.bf16 ? 1 : 0));
        // brn_linear_residual_layer_norm_forward: every fused kernel, and the two-launch fallback
        const int nk[4][3] = {{768, 3072, 100}, {384, 384, 100}, {192, 192, 480}, {384, 1536, 10}};      // N, K, M
        for (const int* s : nk) {
            GemmW gl = linear(wb, s[0], s[1], true);
            LNW l = ln(s[0]);
            const bool fused = linear_residual_ln(c, gl, x, s[2], s[1], kOut, l, kOut + 4096, s[0], true);
            printf("linear_residual_ln N=%d K=%d M=%d -> %d\n", s[0], s[1], s[2], fused ? 1 : 0);
            if (!fused) {
                run_gemm(c, gl, GemmIO(x, s[2], s[1]).to(kOut, s[0]).add(kOut, s[0]).f32(md.bf16 ? 1 : 0, md.bf16 ? 1 : 0));
                run_layernorm(c, l, kOut, s[2], s[0], LnOut(kOut + 4096, s[0]).s16(md.bf16 ? 1 : 0));
            }
        }
        // brn_conv2d_forward: channels-last (3 x 3 dilated, and 1 x 1 = dense) and the NCHW gather, with and without pad_to_stride
        {
            Map X = new_map(c, 2, 10, 14, 64), Y = new_map(c, 2, 10, 14, 40), Y1 = new_map(c, 2, 10, 14, 24);
            GemmW cv = conv_nhwc(wb, 40, 64, 64, 3, 1, true);
            run_conv(c, cv, X, Y);
            GemmW c1 = conv_nhwc(wb, 24, 64, 64, 1, 0, true);
            run_conv(c, c1, X, Y1);
        }
        if (!md.bf16) {
            GemmW pe = conv_gather(192, 3, 4, 4);
            Map T = new_map(c, 1, 8, 13, 192), U = new_map(c, 1, 7, 12, 192);
            run_conv_nchw(c, pe, x, 1, 30, 50, T, true);
            run_conv_nchw(c, pe, x, 1, 30, 50, U);
        }
        // brn_deform_conv2d_forward: offsets | modulator (fp32 out), 2 * sigmoid apart or fused, the gather; a 1 x 1 map the bf16 gather kernel
        // refuses (graph_trace_stubs.cpp) falls back to the fp32-MFMA one
        for (int side : {6, 1}) {
            const int Cp = md.bf16 ? 64 : 32;
            Map X = new_map(c, 1, side, side, Cp), Y = new_map(c, 1, side, side, 16);
            GemmW om = conv_nhwc(wb, 27, 20, Cp, 3, 1, true);
            om.mode = GEMM_CONV_NHWC;
            GemmW reg = conv_nhwc(wb, 16, 20, Cp, 3, 1, true);
            reg.mode = GEMM_DEFORM_NHWC;
            attach_deform_frags(wb, reg);
            const Map OM = Map(c.arena->alloc((size_t)side * side * 28), 1, side, side, 28).window(0, 27);
            run_conv(c, om, X, OM, ConvOpts().f32());
            const bool fused_sig = side > 1 && deform_fused_sigmoid(c, reg);
            printf("deform_fused_sigmoid -> %d\n", deform_fused_sigmoid(c, reg) ? 1 : 0);
            run_conv(c, reg, X, Y, ConvOpts().offsets(OM, 18, fused_sig));
        }
        printf("ops: peak=%zu top=%zu\n", a.peak, a.top);
    }
}

}  // namespace

int main() {
    try {
        const int deforms[2] = {BRN_DEFORM_REFERENCE_CPU, BRN_DEFORM_DEFORMABLE};
        for (size_t mi = 0; mi < std::size(kModes); ++mi)
            for (int dm : deforms) {
                Model m;
                build_model(kModes[mi], dm, m);
                printf("== model %s deform=%d B=1 64x96\n", kModes[mi].name, dm);
                run_dry(m, 1, 64, 96);
                run_branches(m, 1, 64, 96);
                // the profiled forward for four of the fourteen models (the size of the recorded log)
                const bool prof = (mi == 0 && dm == deforms[0]) || (mi == 2 && dm == deforms[1]) || (mi == 4 && dm == deforms[1]) || (mi == 6 && dm == deforms[0]);
                if (prof) run_profile(m, 1, 64, 96);
            }
        {
            Model m;
            build_model(kModes[4], BRN_DEFORM_DEFORMABLE, m);
            printf("== model bf16 deform=%d B=2 64x96\n", BRN_DEFORM_DEFORMABLE);
            run_dry(m, 2, 64, 96);
            run_branches(m, 2, 64, 96);
        }
        {
            // the half-scale image is too small for the fused PatchEmbed of the stubs: the two-kernel path beside an eligible full scale
            Model m;
            build_model(kModes[4], BRN_DEFORM_REFERENCE_CPU, m);
            printf("== model bf16 deform=%d B=1 32x32\n", BRN_DEFORM_REFERENCE_CPU);
            run_dry(m, 1, 32, 32);
            run_branches(m, 1, 32, 32);
        }
        run_op_forms();
    } catch (const Error& e) {
        printf("ERROR %d: %s\n", e.code, e.what());
        return 1;
    }
    return 0;
}
