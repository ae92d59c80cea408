// brn_graph_model.cpp — BiRefNet::forward_logits (birefnet.rs:412-461), BiRefNetDecoder::forward (birefnet.rs:278-376), BasicDecBlk /
// ASPPDeformable (decoder.rs:126-141, aspp.rs:303-333) as launches of the run_* primitives (brn_graph.cpp) on one stream and its branches.
#include "brn_graph.h"

namespace brn {

// ---- BasicDecBlk (decoder.rs:126-141) with ASPPDeformable (aspp.rs:303-333) ------------------------------------------------
void decblk_forward(Ctx& c, const DecBlkW& w, const Map& in, const Map& out, int deform_mode, int out_f32) {
    const size_t mk = c.arena->mark();
    // the maps between the convs carry w.icp channels: inter_channels rounded up to the channel granule (64 -> 64 in the model); a conv
    // writes its real output channels, so the pad channels of a fresh map are zeroed once
    auto inter_map = [&](int chans, int padded) {
        Map m_ = new_map(c, in.B, in.H, in.W, padded);
        if (padded != chans && !c.dry) BRN_HIP(hipMemsetAsync(m_.p, 0, m_.pixels() * (size_t)padded * c.esz(), c.stream));
        Map v = m_.window(0, chans);
        return std::make_pair(m_, v);
    };
    auto [t, t_out] = inter_map(w.ic, w.icp);
    run_conv(c, w.conv_in, in, t_out);                               // conv_in + bn_in + relu
    Map mid = t;
    if (w.has_aspp) {                                                // (else dec_att is None, decoder.rs:131-135)
        auto [u, u_out] = inter_map(w.aspp.oc, w.icp);               // (ASPPDeformable(inter, None): out_channels = inter_channels)
        aspp_forward(c, w.aspp, t, u_out, deform_mode);
        mid = u;
    }
    run_conv(c, w.conv_out, mid, out, ConvOpts().f32(out_f32));      // conv_out + bn_out (no ReLU)
    c.arena->release(mk);
}

void aspp_forward(Ctx& c, const ASPPW& a, const Map& t, const Map& u, int deform_mode) {
    if (t.C != a.icp || t.ld != a.icp || t.coff || u.C != a.oc || u.B != t.B || u.H != t.H || u.W != t.W)
        fail(BRN_ERR_INVALID_ARG, "ASPPDeformable(%d -> %d): input map [C %d, ld %d, coff %d] must be a whole map of %d channels, output map C %d", a.ic, a.oc, t.C,
             t.ld, t.coff, a.icp, u.C);
    const size_t mk = c.arena->mark();
    const int B = t.B, H = t.H, W = t.W, M = B * H * W, IC = a.icp, OC = a.oc;
    const int region0 = c.region;
    c.region = REGION_ASPP;
    Map cat = new_map(c, B, H, W, 1024);                             // [aspp1 | deform k1 | k3 | k7]; pooled branch -> bias
    float* g0 = c.arena->alloc((size_t)B * IC);
    float* g1 = c.arena->alloc((size_t)B * 256);
    float* gb = c.arena->alloc((size_t)B * OC);
    float* gscr = c.arena->alloc(gap_scratch_floats(B, H * W, IC));
    {
        // the branches only share their input t: each runs on its own stream (the 7 x 7 branch, the longest, stays on the main one)
        ArenaHold hold(*c.arena);
        {
            // pooled branch: mean over H then W (aspp.rs:314), 1x1 conv (no bias) + BN + ReLU, nearest-broadcast (aspp.rs:315-318)
            Branch br(c, 2);
            if (!c.dry) {
                Bracket b(c, FAM_ELEMENTWISE, 0.0, 4.0 * M * IC);
                BRN_LAUNCH(launch_gap_nhwc(t.p, B, H * W, IC, IC, 0, gscr, g0, c.stream, c.bf16));
                BRN_LAUNCH(launch_small_fc(g0, B, IC, a.gap_w, IC, 0, 256, a.gap_scale, a.gap_shift, ACT_RELU, g1, c.stream));
                BRN_LAUNCH(launch_small_fc(g1, B, 256, a.conv1_full, 1280, 1024, OC, nullptr, nullptr, ACT_NONE, gb, c.stream));
            }
        }
        if (deform_mode == BRN_DEFORM_REFERENCE_CPU) {
            { Branch br(c, 0); run_gemm(c, a.k1pair, GemmIO(c, t).to(cat)); }                 // aspp1 + aspp_deforms.0 (regular 1x1, BN, ReLU)
            { Branch br(c, 1); run_conv(c, a.d[2].regular, t, cat.window(512, 256)); }       // k3
            run_conv(c, a.d[3].regular, t, cat.window(768, 256));                             // k7
        } else {
            for (int i = 0; i < 4; ++i) {
                Branch br(c, i < 3 ? i : -1);
                const DeformW& d = a.d[i];
                const int kk = d.k * d.k, ldom = d.offmod.N;         // 3 k^2 rounded up to 8 (zero filters: build_aspp_weights)
                const Map om(c.arena->alloc((size_t)M * ldom), B, H, W, ldom);   // offsets / modulator stay fp32 in every mode
                run_conv(c, d.offmod, t, om, ConvOpts().f32());      // offset_conv | modulator_conv (aspp.rs:171,173)
                const bool fused_sig = deform_fused_sigmoid(c, d.regular);   // bf16 gather kernel: 2*sigmoid applied where the modulator is read
                if (!c.dry && !fused_sig) {
                    Bracket b(c, FAM_ELEMENTWISE, 0.0, 8.0 * M * kk);
                    BRN_LAUNCH(launch_mod_sigmoid2(om.p, (size_t)M, ldom, 2 * kk, 3 * kk, c.stream));   // 2*sigmoid (aspp.rs:174)
                }
                run_conv(c, d.regular, t, cat.window(256 * i, 256), ConvOpts().offsets(om, 2 * kk, fused_sig));
            }
        }
        join_branches(c, AUX_ASPP_MASK);
    }
    run_gemm(c, a.conv1_main, GemmIO(c, cat).to(u).image_bias(gb, H * W));   // conv1 + bn1 + relu (aspp.rs:329-331)
    c.region = region0;
    c.arena->release(mk);
}

// ---- decoder (birefnet.rs:278-376) ---------------------------------------------------------------------------------------
static void ipt_block(Ctx& c, const SimpleConvsW& w, const float* img, int B, int H, int W, int th, int tw, int cin, const Map& out) {
    const size_t mk = c.arena->mark();
    const int cinp = roundup(cin, 32);
    Map pt = new_map(c, B, th, tw, cinp);
    if (!c.dry) {
        Bracket b(c, FAM_ELEMENTWISE, 0.0, 8.0 * B * 3.0 * H * W);
        BRN_LAUNCH(launch_image2patches(img, B, 3, H, W, th, tw, pt.p, cinp, cinp, c.stream, c.bf16));   // birefnet.rs:288-300
    }
    Map mid = new_map(c, B, th, tw, 64);
    run_conv(c, w.conv1, pt, mid);        // no activation between the two convs (decoder.rs:52)
    run_conv(c, w.conv_out, mid, out);
    c.arena->release(mk);
}

static void gdt_gate(Ctx& c, const DecoderW& d, int i, const Map& p) {
    const size_t mk = c.arena->mark();
    Map g = new_map(c, p.B, p.H, p.W, 16);
    run_conv(c, d.gdt[i], p, g);                                      // conv3x3 -> 16, BN, ReLU (birefnet.rs:111-117)
    if (!c.dry) {
        Bracket b(c, FAM_ELEMENTWISE, 0.0, 8.0 * p.pixels() * p.C);
        BRN_LAUNCH(launch_gdt_gate(p.p, (int)p.pixels(), p.C, p.ld, p.coff, g.p, 16, d.gdt_attn_w[i], d.gdt_attn_b[i], c.stream, c.bf16));
    }
    c.arena->release(mk);
}

static DecMaps alloc_dec_maps(Ctx& c, const Model& m, int B, int H, int W) {
    const DecoderW& d = m.dec;
    DecMaps dm;
    dm.d3 = new_map(c, B, H / 16, W / 16, 1920);
    dm.d2 = new_map(c, B, H / 8, W / 8, 960);
    // (bf16-storage mode: 512 channels, the last 32 zeros written by ipt_blk2's padded conv_out: decoder_block1.conv_in runs chunk-major)
    const int d1pad = d.dec[3].conv_in.Cinp > 480 ? d.dec[3].conv_in.Cinp - 480 : 0;
    if (d.ipt[1].conv_out.N != 96 + d1pad) fail(BRN_ERR_INVALID_ARG, "ipt_blk2 / decoder_block1 channel padding mismatch");
    dm.d1 = new_map(c, B, H / 4, W / 4, 480 + d1pad);
    dm.d1.C = 480;
    return dm;
}
// ipt_blk5 .. ipt_blk2 (birefnet.rs:304-305,335-337,350-352,365-366): they read only the image and write the last channels of
// the concat maps, so they can run any time before the decoder block that reads the map
static void ipt_blocks(Ctx& c, const Model& m, const float* img, int B, int H, int W, const Map& d4, const DecMaps& dm) {
    const DecoderW& d = m.dec;
    ipt_block(c, d.ipt[4], img, B, H, W, H / 32, W / 32, 3072, d4.window(3072, 384));
    ipt_block(c, d.ipt[3], img, B, H, W, H / 16, W / 16, 768, dm.d3.window(1536, 384));   // ipt4_up is a same-size resize = identity
    ipt_block(c, d.ipt[2], img, B, H, W, H / 8, W / 8, 192, dm.d2.window(768, 192));
    ipt_block(c, d.ipt[1], img, B, H, W, H / 4, W / 4, 48, dm.d1.window(384, dm.d1.ld - 384));
}

// lateral_block4 / 3 / 2 (i = 0 / 1 / 2; 1x1 convs of the backbone maps, birefnet.rs:333,348,363) into [0:C) of the concat map `cat`:
// written there, or added to the up-sampled decoder map already there (accumulate)
static void lateral(Ctx& c, const DecoderW& d, int i, const Map& x, const Map& cat, bool accumulate) {
    const Map dst = cat.window(0, d.lat[i].N);
    GemmIO io = GemmIO(c, x).to(dst);
    if (accumulate) io.add(dst);
    run_gemm(c, d.lat[i], io);
}
// all three BEFORE the up-sampled decoder map is added (run_resize accumulates): they depend on the backbone only, so they can overlap the
// squeeze module and decoder_block4, whose launches fill a fraction of the chip.  fp32 maps only: (conv + bias) + resized and
// resized + (conv + bias) are the same fp32 sum, while on bf16 maps the stored conv result would be rounded once more.
static void lateral_blocks(Ctx& c, const Model& m, const Map& x1, const Map& x2, const Map& x3, const DecMaps& dm) {
    lateral(c, m.dec, 0, x3, dm.d3, false);
    lateral(c, m.dec, 1, x2, dm.d2, false);
    lateral(c, m.dec, 2, x1, dm.d1, false);
}

void decoder_forward(Ctx& c, const Model& m, const float* img, int B, int H, int W, const Map& x1, const Map& x2, const Map& x3,
                     const Map& d4, float* out, int apply_sigmoid, const DecMaps* pre) {
    const DecoderW& d = m.dec;
    const int dm = m.cfg.deform_mode;
    const int h1 = H / 4, w1 = W / 4;
    const size_t mk = c.arena->mark();
    const DecMaps maps = pre ? *pre : alloc_dec_maps(c, m, B, H, W);
    if (!pre) ipt_blocks(c, m, img, B, H, W, d4, maps);
    else join_branches(c, 1u << AUX_IPT);
    const bool lat_done = pre && pre->lat_done;
    // p1 is the last map of the chain and feeds a 192-term dot product per pixel (the head): in compute mode BRN_BF16 it is kept fp32
    // (BRN_P1_F32=0: bf16 like every other map) — its rounding is the one error of the decoder that nothing downstream averages
    const bool p1_f32 = c.bf16 && switches().p1_f32;
    // stage 4: cat(x4, ipt5) -> decoder_block4 -> gate (birefnet.rs:304-305, 323-329); stages 3, 2, 1 (birefnet.rs:332-344, 347-359,
    // 362-369): the previous stage's map up-sampled into [0:C) of the concat map, + lateral(x), -> decoder block (-> gate)
    const Map* xs[3] = {&x3, &x2, &x1};
    const Map* cats[4] = {&d4, &maps.d3, &maps.d2, &maps.d1};
    Map p;
    for (int i = 0; i < 4; ++i) {
        const Map& cat = *cats[i];
        const int C = d.dec[i].cout;
        if (i > 0) {
            if (i == 1 && lat_done) join_branches(c, 1u << AUX_LAT);
            run_resize(c, p, cat.window(0, p.C), lat_done);
            if (!lat_done) lateral(c, d, i - 1, *xs[i - 1], cat, true);
        }
        const bool last_f32 = i == 3 && p1_f32;
        p = last_f32 ? Map(c.arena->alloc(cat.pixels() * C), cat.B, cat.H, cat.W, C) : new_map(c, cat.B, cat.H, cat.W, C);
        decblk_forward(c, d.dec[i], cat, p, dm, last_f32 ? 1 : 0);
        if (i < 3) gdt_gate(c, d, i, p);
    }
    const Map& p1 = p;
    // head (birefnet.rs:372-375): q = <p1, w[0:192]> at 1/4 res; t = the whole ipt_blk1 branch (conv1 -> conv_out -> its
    // slice of conv_out1) as one composed 5x5 stencil on the image (brn_weights.cpp): no 64-channel 1024^2 map exists
    float* q = c.arena->alloc((size_t)B * h1 * w1);
    float* tl = c.arena->alloc((size_t)B * H * W);
    if (!c.dry) {
        Bracket b(c, FAM_ELEMENTWISE, 2.0 * B * H * (double)W * 75, 4.0 * B * H * (double)W * 5);
        BRN_LAUNCH(launch_pixel_dot(p1.p, B * h1 * w1, 192, p1.ld, p1.coff, d.out_w, 0.f, q, c.stream, p1_f32 ? 0 : c.bf16));
        BRN_LAUNCH(launch_head_stencil5x5(img, B, H, W, d.head_k, d.head_b, tl, c.stream));
        BRN_LAUNCH(launch_final_head(q, B, h1, w1, tl, d.out_b, H, W, apply_sigmoid, out, c.stream));
    }
    c.arena->release(mk);
}

// ---- BiRefNet::forward_logits (birefnet.rs:412-461) ----------------------------------------------------------------------------
void model_forward(Model& m, Ctx& c, const float* img, int B, int H, int W, float* out, int apply_sigmoid) {
    if (H % 32 || W % 32 || H < 32 || W < 32) fail(BRN_ERR_INVALID_ARG, "input %dx%d: H and W must be positive multiples of 32 (image2patches, birefnet.rs:288-300)", H, W);
    const bool prof = c.profile && !c.dry && m.stage_ev_ok;
    auto stamp = [&](int i) { if (prof) BRN_HIP(hipEventRecord(m.stage_ev[i], c.stream)); };
    // Ctx::bf16 says what the maps being allocated / the kernels being launched hold: the backbone's setting (m.bf16) inside
    // swin_forward_multi, the decoder side's (m.dec_bf16) everywhere else — the two differ only in the mixed mode BRN_BF16_DEC_SPLIT2
    struct Bf16Scope { Ctx& c; int old; Bf16Scope(Ctx& c_, int v) : c(c_), old(c_.bf16) { c.bf16 = v; } ~Bf16Scope() { c.bf16 = old; } };
    Bf16Scope dec_scope(c, m.dec_bf16);
    const size_t mk = c.arena->mark();
    const int h1 = H / 4, w1 = W / 4, h2 = H / 8, w2 = W / 8, h3 = H / 16, w3 = W / 16, h4 = H / 32, w4 = W / 32;
    // multi-scale concat targets (birefnet.rs:440-443) and the context concat (birefnet.rs:453): [x1|x2|x3|x4] at 1/32
    Map X1 = new_map(c, B, h1, w1, 384), X2 = new_map(c, B, h2, w2, 768), X3 = new_map(c, B, h3, w3, 1536);
    Map X4 = new_map(c, B, h4, w4, 5760), D4 = new_map(c, B, h4, w4, 3456);
    const DecMaps dmaps = alloc_dec_maps(c, m, B, H, W);
    stamp(0);
    {
        // the decoder's image-patch convolutions depend on nothing but the image: enqueued first, on an auxiliary stream, they fill
        // the CUs the batch-1 backbone leaves idle (their temporaries stay allocated: the branch is joined in decoder_forward)
        ArenaHold hold(*c.arena);
        Branch br(c, AUX_IPT);
        ipt_blocks(c, m, img, B, H, W, D4, dmaps);
    }
    {
        // both backbone passes (birefnet.rs:416 and :426) as one pass over concatenated token rows
        const size_t mk2 = c.arena->mark();
        const int Hh = H / 2, Wh = W / 2;
        float* half = c.arena->alloc((size_t)B * 3 * Hh * Wh);
        if (!c.dry) {
            Bracket b(c, FAM_RESIZE, 0.0, 4.0 * B * 3.0 * (H * (double)W + Hh * (double)Wh));
            BRN_LAUNCH(launch_resize_nchw(img, B * 3, H, W, half, Hh, Wh, c.stream));  // birefnet.rs:425
        }
        int hs[4], ws[4];
        swin_stage_dims(Hh, Wh, m.swin.patch, hs, ws);
        Map hm[4];
        for (int i = 0; i < 4; ++i) hm[i] = new_map(c, B, hs[i], ws[i], 192 << i);
        Map outs[4] = {X1.window(0, 192), X2.window(0, 384), X3.window(0, 768), X4.window(2688, 1536)};
        SwinIn ins[2] = {{img, H, W, outs}, {half, Hh, Wh, hm}};
        {
            Bf16Scope bb_scope(c, m.bf16);
            swin_forward_multi(c, m.swin, ins, 2, B, m.bf16 && !m.dec_bf16);
        }
        stamp(1);
        const Map half_dst[4] = {X1.window(192, 192), X2.window(384, 384), X3.window(768, 768), X4.window(4224, 1536)};
        for (int i = 0; i < 4; ++i) run_resize(c, hm[i], half_dst[i]);                // birefnet.rs:435-443
        c.arena->release(mk2);
        // context: x1, x2, x3 bilinearly DOWN-sampled to 1/32 (no antialias), birefnet.rs:450-453
        run_resize(c, X1, X4.window(0, 384));
        run_resize(c, X2, X4.window(384, 768));
        run_resize(c, X3, X4.window(1152, 1536));
    }
    DecMaps dmaps2 = dmaps;
    if (!c.bf16) {
        ArenaHold hold(*c.arena);
        Branch br(c, AUX_LAT);
        lateral_blocks(c, m, X1, X2, X3, dmaps2);
        dmaps2.lat_done = true;
    }
    stamp(2);
    decblk_forward(c, m.squeeze, X4, D4.window(0, 3072), m.cfg.deform_mode);          // birefnet.rs:457
    stamp(3);
    decoder_forward(c, m, img, B, H, W, X1, X2, X3, D4, out, apply_sigmoid, &dmaps2); // birefnet.rs:460
    stamp(4);
    join_branches(c, ~0u);                 // (every branch is joined where its result is read; nothing may outlive the forward)
    c.arena->release(mk);
}

Model::~Model() {
    auto mem = [](void* p) { if (p) (void)hipFree(p); };
    auto str = [](hipStream_t s) { if (s) (void)hipStreamDestroy(s); };
    auto ev = [](hipEvent_t e) { if (e) (void)hipEventDestroy(e); };
    mem(arena.base); mem(io.base);
    for (Side& sd : sides) { mem(sd.arena.base); str(sd.stream); ev(sd.join_ev); }
    ev(fork_ev);
    for (int k = 0; k < 2; ++k) { str(cu_stream[k]); ev(cu_join_ev[k]); }
    for (BranchSet& bs : branch_sets)
        for (int i = 0; i < BRN_AUX_STREAMS; ++i) { str(bs.stream[i]); ev(bs.fork_ev[i]); ev(bs.join_ev[i]); }
    for (hipEvent_t e : event_pool) (void)hipEventDestroy(e);
    if (stage_ev_ok) for (int i = 0; i < 6; ++i) (void)hipEventDestroy(stage_ev[i]);
    ev(done_ev);
}

}  // namespace brn
