// brn_graph_swin.cpp — SwinTransformer::forward (swin.rs:768-797) as launches of the run_* primitives (brn_graph.cpp): PatchEmbed, the
// blocks (window attention + MLP), PatchMerging, the stage output norms written into their consumers' windows.
#include "brn_graph.h"

namespace brn {

WindowGenericRoute g_window_generic_route = nullptr;    // set by brn_window_generic.cpp's registrar (brn_graph.h)
GemmLnRoute g_gemm_ln_route = nullptr;                  // set by brn_gemm_ln.cpp's registrar

void swin_stage_dims(int H, int W, int patch, int hs[4], int ws[4]) {
    int h = (H + patch - 1) / patch, w = (W + patch - 1) / patch;   // PatchEmbed pads to a multiple (swin.rs:696-702)
    for (int i = 0; i < 4; ++i) {
        hs[i] = h; ws[i] = w;
        h = (h + 1) / 2; w = (w + 1) / 2;                            // swin.rs:595
    }
}

// The attention half of a block for `nin` token sets that share the weights (the full- and half-scale backbone passes
// of birefnet.rs:416,426 are run as ONE pass over concatenated token rows: every per-token op sees M = M_full + M_half).
// ln2 / xn2: the block's norm2 and its output matrix — when the projection can take the LayerNorm into its epilogue
// (linear_residual_ln) it is done here and the function returns true.
static bool swin_attention_multi(Ctx& c, const SwinBlockW& blk, const float* xn, int B, int nin, const int* hs, const int* wsz, int C, int shift, float* y,
                                 const float* residual, int p2 = 0, int window = 12, const LNW* ln2 = nullptr, float* xn2 = nullptr, int ld_xn2 = 0) {
    const size_t mk = c.arena->mark();
    int M = 0;
    for (int k = 0; k < nin; ++k) M += B * hs[k] * wsz[k];
    float* qkv = c.act_alloc((size_t)M * 3 * C);                        // (bf16 in compute mode BRN_BF16, like att and xn)
    const int ldp = p2 ? C * p2 / 2 : C;                                // row stride (floats) of a P-layout [M][C] buffer
    float* att = c.act_alloc((size_t)M * ldp);
    run_gemm(c, blk.qkv, GemmIO(xn, M, ldp).to(qkv, 3 * C).planes(p2, 0));   // swin.rs:217 (pad rows are synthesised by the kernel)
    if (window != 12 && window != 7) {
        // no fused kernel for this window side: the generic route, map by map (it plans its own buffers, so it runs in a dry run too).
        // stage_pl needs window 12, so qkv and att are plain matrices here
        if (p2) fail(BRN_ERR_INVALID_ARG, "window_size %d: the generic window route takes no plane layout", window);
        if (!g_window_generic_route) fail(BRN_ERR_INVALID_ARG, "window_size %d needs the generic window route", window);
        size_t off = 0;
        for (int k = 0; k < nin; ++k) {
            g_window_generic_route(c, blk, c.at(qkv, off * 3 * C), c.at(att, off * C), B, hs[k], wsz[k], C, window, shift);
            off += (size_t)B * hs[k] * wsz[k];
        }
    } else if (!c.dry) {
        // one launch for all maps of the pass (full + half scale): fewer ramps and tails than one launch per geometry
        WindowAttnParams ps[2]{};
        size_t off = 0;
        double nwin = 0.0;
        for (int k = 0; k < nin; ++k) {
            WindowAttnParams& p = ps[k];
            p.qkv = c.at(qkv, off * 3 * C); p.qkv_bias = blk.qkv.bias; p.rel_table = blk.rel_table; p.out = c.at(att, off * ldp);
            p.io_bf16 = c.bf16;
            p.B = B; p.H = hs[k]; p.W = wsz[k]; p.C = C; p.heads = blk.heads;
            p.Hp = roundup(hs[k], window); p.Wp = roundup(wsz[k], window);   // swin.rs:359-360
            p.ws = window;
            p.shift = shift; p.scale = 1.0f / sqrtf(32.0f);          // head_dim^-0.5 (swin.rs:134)
            p.planes = (!c.bf16 && window == 12 && (blk.qkv.planes == 2 || blk.qkv.planes == 1)) ? blk.qkv.planes : 0;
            p.h2 = (p.planes == 2 && blk.qkv.half && switches().h2_att) ? 1 : 0;
            if (blk.qkv.half && !p.h2) p.planes = 0;        // BRN_H2_ATT=0: the fp32-MFMA kernel, like f32_split3
            p.pack_q = switches().att_pack_q;
            p.out_planes = p2;
            p.out_h2 = (p2 == 2 && blk.qkv.half) ? c.h2_scale : 0.f;
            nwin += (double)B * (p.Hp / window) * (p.Wp / window) * blk.heads;
            off += (size_t)B * hs[k] * wsz[k];
        }
        const double ntok = (double)window * window;
        Bracket b(c, FAM_ATTENTION, nwin * 2.0 * 2.0 * ntok * ntok * 32, (double)c.esz() * ((double)M * 4 * C), M, C, shift);
        BRN_LAUNCH(launch_window_attention2(ps[0], nin > 1 ? &ps[1] : nullptr, c.stream));
    }
    // swin.rs:310 (+ shortcut, swin.rs:406); the residual stream y / residual stays fp32 in every mode
    bool ln_done = false;
    if (ln2 && xn2 && !p2 && y == residual) ln_done = linear_residual_ln(c, blk.proj, att, M, ldp, y, *ln2, xn2, ld_xn2);
    // split modes: where the projection is cut along K, norm2 sums the slices (brn_gemm_ln.cpp)
    if (!ln_done && ln2 && xn2 && y == residual && g_gemm_ln_route)
        ln_done = g_gemm_ln_route(c, blk.proj, GemmIO(att, M, ldp).to(y, C).add(residual, C).planes(p2, 0).f32(c.bf16, c.bf16), *ln2, LnOut(xn2, ld_xn2).planes(p2).s16(c.bf16));
    if (!ln_done) run_gemm(c, blk.proj, GemmIO(att, M, ldp).to(y, C).add(residual, C).planes(p2, 0).f32(c.bf16, c.bf16));
    c.arena->release(mk);
    return ln_done;
}

void swin_attention(Ctx& c, const SwinBlockW& blk, const float* xn, int B, int H, int W, int C, int shift, float* y, const float* residual, int window) {
    swin_attention_multi(c, blk, xn, B, 1, &H, &W, C, shift, y, residual, 0, window);
}

void swin_forward_multi(Ctx& c, const SwinW& w, const SwinIn* ins, int nin, int B, bool outs_f32) {
    if (nin < 1 || nin > 2) fail(BRN_ERR_INVALID_ARG, "swin_forward_multi: 1 or 2 inputs");
    int hs[2][4], wsz[2][4];
    for (int k = 0; k < nin; ++k) swin_stage_dims(ins[k].H, ins[k].W, w.patch, hs[k], wsz[k]);
    auto rows = [&](int k, int i) { return B * hs[k][i] * wsz[k][i]; };
    auto total = [&](int i) { int m = 0; for (int k = 0; k < nin; ++k) m += rows(k, i); return m; };
    const size_t mk0 = c.arena->mark();
    const int E = w.embed_dim;
    // PatchEmbed (swin.rs:692-714): conv k4 s4 straight from the NCHW image (zero beyond the border = pad_with_zeros), LN
    float* x = c.arena->alloc((size_t)total(0) * E);
    // compute mode BRN_BF16, Swin-L geometry, image sides multiples of 4: conv + bias + LayerNorm in one kernel per image scale
    // (kernels/patch_embed.hip) — neither the conv output nor a second pass over it touches HBM
    const int pe_env = switches().patch_ln;     // 0: two kernels; 2: fused without the first block's norm1
    bool pe_fused = c.bf16 && pe_env != 0 && w.patch_proj.w && w.patch_proj.mode == GEMM_GATHER_NCHW && w.patch_proj.pad == 0 && w.patch_proj.dil == 1 &&
                    w.patch_proj.kh == w.patch_proj.kw && w.patch_norm.C == E && w.patch_norm.g && w.patch_norm.b;
    for (int k = 0; k < nin && pe_fused; ++k)
        pe_fused = patch_embed_ln_eligible(w.patch_proj.Cin, w.patch_proj.N, w.patch_proj.kh, w.patch_proj.stride, ins[k].H, ins[k].W, w.patch_proj.K, E);
    // ... and, while the row is in registers, the first block's norm1 of it (the bf16 operand of that block's qkv GEMM)
    float* xn0 = nullptr;
    if (pe_fused && pe_env != 2 && !w.stages[0].blocks.empty() && w.stages[0].C == E && w.stages[0].blocks[0].norm1.C == E && w.stages[0].blocks[0].norm1.g &&
        w.stages[0].blocks[0].norm1.b)
        xn0 = c.act_alloc((size_t)total(0) * E);
    if (pe_fused) {
        size_t off = 0;
        for (int k = 0; k < nin; ++k) {
            if (!c.dry) {
                const double M = (double)rows(k, 0);
                Bracket b(c, FAM_GEMM_GATHER, 2.0 * M * E * w.patch_proj.Kreal, 4.0 * ((double)B * 3 * ins[k].H * ins[k].W + M * E) + (xn0 ? 2.0 * M * E : 0.0), (int)M, E, w.patch_proj.K);
                const LNW* n1 = xn0 ? &w.stages[0].blocks[0].norm1 : nullptr;
                BRN_LAUNCH(launch_patch_embed_ln(ins[k].img, B, ins[k].H, ins[k].W, w.patch_proj.w, w.patch_proj.K, w.patch_proj.bias, w.patch_norm.g,
                                                 w.patch_norm.b, 1e-5f, x + off * E, E, c.stream, n1 ? n1->g : nullptr, n1 ? n1->b : nullptr,
                                                 xn0 ? c.at(xn0, off * E) : nullptr, E, c.bf16 == 2));
            }
            off += rows(k, 0);
        }
    } else {
        const size_t mk = c.arena->mark();
        float* t = c.arena->alloc((size_t)total(0) * E);
        size_t off = 0;
        for (int k = 0; k < nin; ++k) {
            run_conv_nchw(c, w.patch_proj, ins[k].img, B, ins[k].H, ins[k].W, Map(t + off * E, B, hs[k][0], wsz[k][0], E), true);
            off += rows(k, 0);
        }
        run_layernorm(c, w.patch_norm, t, total(0), E, LnOut(x, E));
        c.arena->release(mk);
    }
    // P layout (kernels/split_planes.h) of a stage's GEMM inputs in the split modes: 2 planes = the fp32 row size, 3 planes = 1.5x; 0 = plain matrices
    auto stage_planes = [&](const SwinStageW& sg) {
        if (sg.blocks.empty()) return 0;
        const SwinBlockW& b0 = sg.blocks[0];
        const int np = b0.qkv.planes;
        // (3 planes = rows 1.5x as long: measured 2 % SLOWER per forward in f32_split3 with the warp-specialised kernel, and the
        // LDS-DMA plane kernel, kernels/gemm_planes.hip, which needs P3 input, did not beat it at batch 1: 2 planes only by default)
#ifdef BRN_DIAG_BUILD
        const bool planes_on = switches().planes_kernel != 0;
#else
        constexpr bool planes_on = false;
#endif
        if (w.window == 12 && (np == 2 || (np == 3 && planes_on)) && b0.qkv.wp && b0.proj.wp && b0.fc1.wp && b0.fc2.wp && sg.C % 32 == 0 && b0.fc1.N % 32 == 0) return np;
        return 0;
    };
    float* xn_handoff = nullptr;       // the next stage's first norm1 matrix, and whether the reduction's LayerNorm wrote it
    bool handoff_done = false;
    for (int i = 0; i < 4; ++i) {
        const SwinStageW& st = w.stages[i];
        const int C = st.C, M = total(i);
        int hh[2], ww[2];
        for (int k = 0; k < nin; ++k) { hh[k] = hs[k][i]; ww[k] = wsz[k][i]; }
        float* xnext = nullptr;
        if (st.has_down) xnext = c.arena->alloc((size_t)total(i + 1) * 2 * C);
        // the PatchMerging reduction may write the next stage's first norm1 itself (g_gemm_ln_route): that matrix outlives this stage's mark
        float* xn_made = xn_handoff;
        xn_handoff = nullptr;
        int next_pl = 0;
        if (st.has_down && i + 1 < 4 && g_gemm_ln_route && !c.bf16 && !w.stages[i + 1].blocks.empty() && w.stages[i + 1].C == 2 * C) {
            next_pl = stage_planes(w.stages[i + 1]);
            xn_handoff = c.act_alloc((size_t)total(i + 1) * (next_pl ? 2 * C * next_pl / 2 : 2 * C));
        }
        const size_t mk = c.arena->mark();
        const int hidden = st.blocks.empty() ? 4 * C : st.blocks[0].fc1.N;
        const int stage_pl = stage_planes(st);
        const int ldx = stage_pl ? C * stage_pl / 2 : C, ldh = stage_pl ? hidden * stage_pl / 2 : hidden;
        c.h2_scale = (stage_pl == 2 && st.blocks[0].qkv.half) ? half2_act_scale() : 0.f;    // mode f32_half2: the P2 planes are fp16 planes of the scaled activations
        // compute mode BRN_BF16: x (the residual stream) stays fp32; every GEMM operand (xn, qkv, att, hid, pm) is bf16
        const int yb = c.bf16;
        // the next norm1 is already in xn: block 0's came out of the PatchEmbed kernel or of the reduction's LayerNorm, block j + 1's out of fc2's
        bool xn_ready = (i == 0 && xn0 && !stage_pl && ldx == C) || (xn_made && handoff_done);
        float* xn = (i == 0 && xn_ready) ? xn0 : xn_made ? xn_made : c.act_alloc((size_t)M * ldx);
        handoff_done = false;
        float* hid = c.act_alloc((size_t)M * ldh);
        for (size_t j = 0; j < st.blocks.size(); ++j) {
            const SwinBlockW& bk = st.blocks[j];
            const int shift = (j % 2 == 0) ? 0 : w.window / 2;                       // swin.rs:552
            // split modes: every GEMM input of the block is written by its producer in the P layout (the bf16 planes the GEMM
            // would split out while staging), so the GEMMs' staging waves only copy
            const int p2 = stage_pl;
            const LnOut xn_out = LnOut(xn, ldx).planes(p2).s16(yb);
            if (!xn_ready) run_layernorm(c, bk.norm1, x, M, C, xn_out);   // swin.rs:355
            xn_ready = false;
            const bool ln2_done = swin_attention_multi(c, bk, xn, B, nin, hh, ww, C, shift, x, x, p2, w.window, &bk.norm2, xn, ldx);   // x = shortcut + attn (swin.rs:406)
            if (!ln2_done) run_layernorm(c, bk.norm2, x, M, C, xn_out);               // swin.rs:407
            run_gemm(c, bk.fc1, GemmIO(xn, M, ldx).to(hid, ldh).planes(p2, p2));      // fc1 + gelu_erf (swin.rs:104-105)
            const GemmIO fc2_io = GemmIO(hid, M, ldh).to(x, C).add(x, C).planes(p2, 0).f32(yb, yb);     // x + fc2(...) (swin.rs:106,407)
            // ... with the next block's norm1 summing fc2's split-K slices where the route takes the pair (the last fc2 feeds the output norms)
            if (j + 1 < st.blocks.size() && g_gemm_ln_route) xn_ready = g_gemm_ln_route(c, bk.fc2, fc2_io, st.blocks[j + 1].norm1, xn_out);
            if (!xn_ready) run_gemm(c, bk.fc2, fc2_io);
        }
        // stage output = norm_i(x_out), pre-downsample (swin.rs:591,784-789); written into its consumer's window
        size_t off = 0, off2 = 0;
        float* pm = nullptr;
        const int pm_pl = (st.has_down && st.reduction.wp && (st.reduction.planes == 2 || (st.reduction.planes == 3 && stage_pl == 3)) && (4 * C) % 32 == 0) ? st.reduction.planes : 0;
        const int ldpm = pm_pl ? 4 * C * pm_pl / 2 : 4 * C;
        if (st.has_down) pm = c.act_alloc((size_t)total(i + 1) * ldpm);
        for (int k = 0; k < nin; ++k) {
            const Map& o = ins[k].outs[i];
            if (o.B != B || o.H != hh[k] || o.W != ww[k] || o.C != C) fail(BRN_ERR_INVALID_ARG, "swin output window %d has the wrong shape", i);
            run_layernorm(c, st.out_norm, x + off * C, rows(k, i), C, LnOut(o).s16(outs_f32 ? 0 : yb));
            if (st.has_down) {
                // PatchMerging (swin.rs:491-527): gather 2x2 + LN(4C) fused, then the bias-free reduction (below, once)
                const int M2 = rows(k, i + 1);
                if (!c.dry) {
                    LayerNormParams p{};
                    p.x = x + off * C; p.y = c.at(pm, off2 * ldpm); p.rows = M2; p.y_bf16 = yb; p.C = 4 * C; p.gamma = st.down_norm.g; p.beta = st.down_norm.b;
                    p.eps = 1e-5f; p.ldy = ldpm; p.y_coff = 0; p.mode = 1; p.H = hh[k]; p.W = ww[k]; p.Cin = C;
                    p.y_planes = pm_pl;                                            // P layout for the reduction GEMM
                    p.y_h2 = (pm_pl == 2 && st.reduction.half) ? half2_act_scale() : 0.f;
                    Bracket b(c, FAM_LAYERNORM, 0.0, 8.0 * M2 * 4.0 * C, M2, 4 * C, 1);
                    BRN_LAUNCH(launch_layernorm(p, c.stream));
                }
                off2 += M2;
            }
            off += rows(k, i);
        }
        if (st.has_down) {
            const GemmIO red_io = GemmIO(pm, total(i + 1), ldpm).to(xnext, 2 * C).planes(pm_pl, 0).f32(yb, 0);
            if (xn_handoff) {
                const SwinBlockW& nb = w.stages[i + 1].blocks[0];
                c.h2_scale = (next_pl == 2 && nb.qkv.half) ? half2_act_scale() : 0.f;
                handoff_done = g_gemm_ln_route(c, st.reduction, red_io, nb.norm1, LnOut(xn_handoff, next_pl ? 2 * C * next_pl / 2 : 2 * C).planes(next_pl));
            }
            if (!handoff_done) run_gemm(c, st.reduction, red_io);
        }
        c.h2_scale = 0.f;
        c.arena->release(mk);
        x = xnext;
    }
    c.arena->release(mk0);
}

}  // namespace brn
