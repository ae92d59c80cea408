// brn_weights.cpp — BiRefNet::new (birefnet.rs:389-409) on the device side: look the tensors up by their
// VarBuilder names, repack them for gemm_f32 (K-contiguous, channels-last tap order, rows padded
// to the tile), fold eval-mode BatchNorm into per-channel scale/shift, precompute the transposed relative-position
// bias per block (the analogue of WindowAttention::cached_bias, swin.rs:147-152), upload once.
#include "brn_host.h"
#include "brn_pack.h"
#include <cstdlib>
#include <cmath>
#include <cstring>
#include <cstdio>

namespace brn {

static thread_local std::string g_last_error;
void set_last_error(const std::string& s) { g_last_error = s; }
const char* last_error_cstr() { return g_last_error.c_str(); }

void fail(int code, const char* fmt, ...) {
    char buf[1024];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    throw Error(code, buf);
}

void ensure_device(int ordinal) {
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess || n <= 0) fail(BRN_ERR_NO_DEVICE, "no HIP device available (%s); this library has no CPU fallback",
                                        e != hipSuccess ? hipGetErrorString(e) : "device count 0");
    if (ordinal < 0 || ordinal >= n) fail(BRN_ERR_NO_DEVICE, "device ordinal %d out of range (have %d)", ordinal, n);
    BRN_HIP(hipSetDevice(ordinal));
}

// ---- device ownership -----------------------------------------------------------------------------------------
float* DeviceOwner::upload(const float* host, size_t n) {
    void* d = nullptr;
    hipError_t e = hipMalloc(&d, n * sizeof(float) + 16);
    if (e != hipSuccess) fail(BRN_ERR_OOM, "hipMalloc of %zu bytes failed: %s", n * sizeof(float), hipGetErrorString(e));
    ptrs.push_back(d);
    BRN_HIP(hipMemcpy(d, host, n * sizeof(float), hipMemcpyHostToDevice));
    return (float*)d;
}
DeviceOwner::~DeviceOwner() {
    for (void* p : ptrs) (void)hipFree(p);
}

// ---- weight table -----------------------------------------------------------------------------------------------
WeightTable::WeightTable(const brn_named_tensor* w, size_t n) {
    for (size_t i = 0; i < n; ++i)
        if (w[i].name) map[w[i].name] = &w[i];
}
const brn_named_tensor* WeightTable::get(const std::string& name, std::initializer_list<int64_t> shape) const {
    auto it = map.find(name);
    if (it == map.end()) fail(BRN_ERR_MISSING_TENSOR, "cannot find tensor %s", name.c_str());
    const brn_named_tensor* t = it->second;
    bool ok = t->ndim == (int)shape.size() && t->data != nullptr;
    if (ok) {
        int i = 0;
        for (int64_t d : shape) ok = ok && t->shape[i++] == d;
    }
    if (!ok) {
        std::string want, got;
        for (int64_t d : shape) want += (want.empty() ? "" : ", ") + std::to_string(d);
        for (int i = 0; i < t->ndim; ++i) got += (got.empty() ? "" : ", ") + std::to_string(t->shape[i]);
        fail(BRN_ERR_SHAPE, "shape mismatch for %s: expected [%s] got [%s]", name.c_str(), want.c_str(), got.c_str());
    }
    return t;
}

// one 16-bit buffer of a model (planes, bf16-storage matrix, fragments), with the same slack as the fp32 uploads
void* DeviceOwner::upload_u16(const std::vector<uint16_t>& v) {
    void* d = nullptr;
    hipError_t e = hipMalloc(&d, v.size() * 2 + 16);
    if (e != hipSuccess) fail(BRN_ERR_OOM, "hipMalloc of %zu bytes failed: %s", v.size() * 2, hipGetErrorString(e));
    ptrs.push_back(d);
    BRN_HIP(hipMemcpy(d, v.data(), v.size() * 2, hipMemcpyHostToDevice));
    return d;
}

float half2_act_scale() {
    const int k = switches().h2_ascale;                 // log2 of the scale
    return ldexpf(1.f, k < 0 ? 0 : (k > 8 ? 8 : k));
}

// the 16-bit copy of the packed fp32 matrix pk [rows][K] that mode wb computes with (layouts: brn_pack.h)
static void attach_planes(DeviceOwner& own, WeightBuild wb, GemmW& g, const std::vector<float>& pk, int rows) {
    const size_t K = (size_t)g.K;
    if (wb.planes <= 0) return;
    if (wb.planes == BUILD_BF16) {
        const size_t conv_taps = switches().conv_chunk_major && g.mode == GEMM_CONV_NHWC ? (size_t)g.kh * g.kw : 0;
        const S16Storage s = pack_s16_storage(pk, K, wb.f16, conv_taps, (size_t)g.Cinp);
        g.wb = own.upload_u16(s.w);
        g.wb_chunk_major = s.chunk_major ? 1 : 0; g.wb_rows = (int)s.rows; g.wb_ld = (int)s.ld;
    } else if (wb.planes == BUILD_HALF2) {
        g.wp = own.upload_u16(pack_half2_planes(pk, K, &g.w_scale));
        g.planes = 2; g.wp_rows = rows; g.half = 1;
    } else {
        g.wp = own.upload_u16(pack_bf16_planes(pk, K, wb.planes));
        g.planes = wb.planes; g.wp_rows = rows;
    }
}

// ---- repack helpers ------------------------------------------------------------------------------------------------
GemmW make_linear(DeviceOwner& own, WeightBuild wb, const float* w, const float* bias, int N, int K) {
    if (K % 32) fail(BRN_ERR_INVALID_ARG, "linear in_features %d must be a multiple of 32", K);
    GemmW g;
    g.N = N; g.K = K; g.Kreal = K; g.Cin = K; g.Cinp = K; g.mode = GEMM_DENSE;
    std::vector<float> pk((size_t)roundup(N, 128) * K, 0.f);
    memcpy(pk.data(), w, (size_t)N * K * sizeof(float));
    g.w = own.upload(pk);
    attach_planes(own, wb, g, pk, roundup(N, 128));
    attach_dense_frags(own, wb, g, w);
    if (bias) g.bias = own.upload(bias, N);
    return g;
}

GemmW make_conv_nhwc(DeviceOwner& own, WeightBuild wb, const float* w, const float* bias, int O, int Cin, int cinp, int kh, int kw,
                     int stride, int pad, int dil) {
    if (cinp % 32 || cinp < Cin) fail(BRN_ERR_INVALID_ARG, "padded channel count %d invalid for Cin %d", cinp, Cin);
    GemmW g;
    g.N = O; g.K = kh * kw * cinp; g.Kreal = kh * kw * Cin; g.Cin = Cin; g.Cinp = cinp;
    g.kh = kh; g.kw = kw; g.stride = stride; g.pad = pad; g.dil = dil;
    g.mode = (kh == 1 && kw == 1 && stride == 1 && pad == 0) ? GEMM_DENSE : GEMM_CONV_NHWC;
    std::vector<float> pk((size_t)roundup(O, 128) * g.K, 0.f);
    for (int o = 0; o < O; ++o)
        for (int ci = 0; ci < Cin; ++ci)
            for (int ky = 0; ky < kh; ++ky)
                for (int kx = 0; kx < kw; ++kx)
                    pk[(size_t)o * g.K + (size_t)(ky * kw + kx) * cinp + ci] = w[(((size_t)o * Cin + ci) * kh + ky) * kw + kx];
    g.w = own.upload(pk);
    attach_planes(own, wb, g, pk, roundup(O, 128));
    if (g.mode == GEMM_DENSE && cinp == Cin) attach_dense_frags(own, wb, g, w);      // 1x1 conv = Linear: [O][Cin] as stored
    if (bias) g.bias = own.upload(bias, O);
    return g;
}

// bf16-storage mode: the fragment-ordered copies (brn_pack.h) where the kernels that read them cover the shape
void attach_deform_frags(DeviceOwner& own, WeightBuild wb, GemmW& g, const float* w) {
    if (wb.planes != BUILD_BF16 || g.Cinp % 64 || g.K != g.kh * g.kw * g.Cinp) return;
    g.wf = own.upload_u16(pack_frags(w, g.N, roundup(g.N, 256), g.Cin, g.Cinp, g.kh * g.kw, wb.f16));
}
void attach_dense_frags(DeviceOwner& own, WeightBuild wb, GemmW& g, const float* w) {
    if (wb.planes != BUILD_BF16 || g.mode != GEMM_DENSE || (g.K != 192 && g.K != 384) || g.N < 192 || g.N % 192) return;
    g.wf = own.upload_u16(pack_frags(w, g.N, g.N, g.K, g.K, 1, wb.f16));
}

GemmW make_conv_gather(DeviceOwner& own, const float* w, const float* bias, int O, int Cin, int kh, int kw, int stride,
                       int pad, int dil) {
    GemmW g;
    g.N = O; g.Kreal = Cin * kh * kw; g.K = roundup(g.Kreal, 32); g.Cin = Cin; g.Cinp = Cin;
    g.kh = kh; g.kw = kw; g.stride = stride; g.pad = pad; g.dil = dil; g.mode = GEMM_GATHER_NCHW;
    std::vector<float> pk((size_t)roundup(O, 128) * g.K, 0.f);
    for (int o = 0; o < O; ++o) memcpy(&pk[(size_t)o * g.K], &w[(size_t)o * g.Kreal], (size_t)g.Kreal * sizeof(float));
    g.w = own.upload(pk);
    if (bias) g.bias = own.upload(bias, O);
    return g;
}

// eval-mode batch_norm after a conv (decoder.rs:128-129): y = ((acc + b) - mean) / sqrt(var + eps) * gamma + beta
//                                                        = acc * scale + shift
void fold_bn(DeviceOwner& own, GemmW& g, const float* conv_bias, const float* gamma, const float* beta,
             const float* mean, const float* var, float eps) {
    std::vector<float> sc(g.N), sh(g.N);
    for (int n = 0; n < g.N; ++n) {
        const double s = (double)gamma[n] / std::sqrt((double)var[n] + (double)eps);
        const double b = conv_bias ? (double)conv_bias[n] : 0.0;
        sc[n] = (float)s;
        sh[n] = (float)((b - (double)mean[n]) * s + (double)beta[n]);
    }
    g.scale = own.upload(sc);
    g.shift = own.upload(sh);
    g.bias = nullptr;
}

struct BNHost { const float *g, *b, *m, *v; };
static BNHost get_bn(const WeightTable& wt, const std::string& p, int C) {
    BNHost h;
    h.g = wt.get(p + ".weight", {C})->data;
    h.b = wt.get(p + ".bias", {C})->data;
    h.m = wt.get(p + ".running_mean", {C})->data;
    h.v = wt.get(p + ".running_var", {C})->data;
    return h;
}
static LNW get_ln(const WeightTable& wt, const std::string& p, int C, DeviceOwner& own) {
    LNW l;
    l.C = C;
    l.g = own.upload(wt.get(p + ".weight", {C})->data, C);
    l.b = own.upload(wt.get(p + ".bias", {C})->data, C);
    return l;
}
static GemmW get_linear(const WeightTable& wt, const std::string& p, int N, int K, bool bias, DeviceOwner& own, WeightBuild wb) {
    const float* w = wt.get(p + ".weight", {N, K})->data;
    const float* b = bias ? wt.get(p + ".bias", {N})->data : nullptr;
    return make_linear(own, wb, w, b, N, K);
}

// ---- Swin (swin.rs:725-764) -----------------------------------------------------------------------------------------
void build_swin_weights(const WeightTable& wt, const std::string& pre, const brn_config& cfg, DeviceOwner& own, WeightBuild wb, SwinW& out) {
    // 12 (Swin-B / L, swin.rs:60,74) and 7 (Swin-T / S, swin.rs:32,46) have fused attention kernels; every other side takes the generic route
    if (cfg.window_size < 2 || cfg.window_size > 32) fail(BRN_ERR_INVALID_ARG, "window_size %d unsupported (2 <= window_size <= 32)", cfg.window_size);
    if (cfg.patch_size < 1 || cfg.in_channels < 1) fail(BRN_ERR_INVALID_ARG, "bad patch_size/in_channels");
    out.embed_dim = cfg.embed_dim; out.window = cfg.window_size; out.patch = cfg.patch_size; out.in_ch = cfg.in_channels;
    const int E = cfg.embed_dim, P = cfg.patch_size, IC = cfg.in_channels;
    if (E % 32) fail(BRN_ERR_INVALID_ARG, "embed_dim %d must be a multiple of 32", E);
    {
        const float* w = wt.get(pre + "patch_embed.proj.weight", {E, IC, P, P})->data;
        const float* b = wt.get(pre + "patch_embed.proj.bias", {E})->data;
        out.patch_proj = make_conv_gather(own, w, b, E, IC, P, P, P, 0, 1);
        out.patch_norm = get_ln(wt, pre + "patch_embed.norm", E, own);
    }
    const int ws = cfg.window_size, T = (2 * ws - 1) * (2 * ws - 1);
    for (int i = 0; i < 4; ++i) {
        SwinStageW& st = out.stages[i];
        const int C = E << i, heads = cfg.num_heads[i];
        st.C = C; st.heads = heads;
        if (heads <= 0 || C != heads * 32)
            fail(BRN_ERR_INVALID_ARG, "stage %d: dim %d / heads %d: head_dim must be 32 (Swin-L geometry)", i, C, heads);
        const int hidden = (int)((double)C * (double)cfg.mlp_ratio);   // swin.rs:337
        const std::string lp = pre + "layers." + std::to_string(i) + ".";
        st.blocks.resize(cfg.depths[i]);
        for (int j = 0; j < cfg.depths[i]; ++j) {
            SwinBlockW& bk = st.blocks[j];
            const std::string bp = lp + "blocks." + std::to_string(j) + ".";
            bk.heads = heads;
            bk.norm1 = get_ln(wt, bp + "norm1", C, own);
            bk.norm2 = get_ln(wt, bp + "norm2", C, own);
            bk.qkv = get_linear(wt, bp + "attn.qkv", 3 * C, C, true, own, wb);
            bk.proj = get_linear(wt, bp + "attn.proj", C, C, true, own, wb);
            bk.fc1 = get_linear(wt, bp + "mlp.fc1", hidden, C, true, own, wb);
            bk.fc1.act = ACT_GELU_ERF;                                  // swin.rs:105
            bk.fc2 = get_linear(wt, bp + "mlp.fc2", C, hidden, true, own, wb);
            const float* table = wt.get(bp + "attn.relative_position_bias_table", {T, heads})->data;
            {   // [T][heads] -> [heads][T] so a workgroup reads its head's column contiguously; indexed in-kernel by
                // (qi-ki+ws-1)*(2ws-1) + (qj-kj+ws-1) (swin.rs:182-184)
                std::vector<float> tt((size_t)T * heads);
                for (int t = 0; t < T; ++t) for (int h = 0; h < heads; ++h) tt[(size_t)h * T + t] = table[(size_t)t * heads + h];
                bk.rel_table = own.upload(tt);
            }
        }
        st.has_down = i < 3;
        if (st.has_down) {
            st.down_norm = get_ln(wt, lp + "downsample.norm", 4 * C, own);
            st.reduction = get_linear(wt, lp + "downsample.reduction", 2 * C, 4 * C, false, own, wb);
        }
        st.out_norm = get_ln(wt, pre + "norm" + std::to_string(i), C, own);
    }
}

// ---- BasicDecBlk + ASPPDeformable (decoder.rs:86-124, aspp.rs:236-300) ---------------------------------------------------
static GemmW conv_bn(const WeightTable& wt, const std::string& conv, bool has_bias, const std::string& bn, int O, int Cin,
                     int cinp, int k, int pad, int act, DeviceOwner& own, WeightBuild wb) {
    const float* w = wt.get(conv + ".weight", {O, Cin, k, k})->data;
    const float* b = has_bias ? wt.get(conv + ".bias", {O})->data : nullptr;
    GemmW g = make_conv_nhwc(own, wb, w, nullptr, O, Cin, cinp, k, k, 1, pad, 1);
    if (!bn.empty()) {
        BNHost h = get_bn(wt, bn, O);
        fold_bn(own, g, b, h.g, h.b, h.m, h.v, 1e-5f);
    } else if (b) {
        g.bias = own.upload(b, O);
    }
    g.act = act;
    return g;
}

void build_decblk_weights(const WeightTable& wt, const std::string& p, int cin, int cout, int deform_mode, DeviceOwner& own,
                          WeightBuild wb, DecBlkW& out, bool use_aspp, int inter_channels) {
    const int IC = inter_channels;  // decoder.rs:94-98
    if (IC < 1) fail(BRN_ERR_INVALID_ARG, "decoder block inter_channels %d", IC);
    const int gran = wb.planes == BUILD_BF16 ? 64 : 32;
    out.cin = cin; out.cout = cout; out.has_aspp = use_aspp; out.ic = IC; out.icp = roundup(IC, gran);
    // The channels-last convs read whole 32-channel granules (64 in the bf16-storage mode, where e.g. decoder_block1's 480 is padded so
    // that the conv runs chunk-major): a channel count off the granule is padded with zero weights to the next multiple; the map then
    // carries that many channels, the pad ones zero (conv_in's pad OUTPUT channels have zero weights, scale and shift).  Every block of
    // the model has in_channels % 32 == 0 and inter_channels = 64.
    const int cin_pad = roundup(cin, gran);
    out.conv_in = conv_bn(wt, p + "conv_in", true, p + "bn_in", IC, cin, cin_pad, 3, 1, ACT_RELU, own, wb);
    out.conv_out = conv_bn(wt, p + "conv_out", true, p + "bn_out", cout, IC, out.icp, 3, 1, ACT_NONE, own, wb);   // no ReLU (decoder.rs:138-139)
    if (use_aspp) build_aspp_weights(wt, p + "dec_att.", deform_mode, own, wb, out.aspp, IC, 0);                    // decoder.rs:107-111
}

// ASPPDeformable::new (aspp.rs:236-300) under prefix `ap`: in_channels IC (64 inside the model's BasicDecBlk), out_channels OC
void build_aspp_weights(const WeightTable& wt, const std::string& ap, int deform_mode, DeviceOwner& own, WeightBuild wb, ASPPW& a, int in_channels, int out_channels) {
    const int IC = in_channels, OC = out_channels > 0 ? out_channels : in_channels, PL = 256;   // aspp.rs:242-243
    if (IC < 1) fail(BRN_ERR_INVALID_ARG, "ASPPDeformable in_channels %d", IC);
    const int ICP = roundup(IC, wb.planes == BUILD_BF16 ? 64 : 32);
    a.ic = IC; a.icp = ICP; a.oc = OC;
    const int ks[4] = {1, 1, 3, 7};
    const std::string mods[4] = {ap + "aspp1.", ap + "aspp_deforms.0.", ap + "aspp_deforms.1.", ap + "aspp_deforms.2."};
    for (int i = 0; i < 4; ++i) {
        const int k = ks[i], kk = k * k;
        DeformW& d = a.d[i];
        d.k = k;
        const std::string cp = mods[i] + "atrous_conv.";
        // all three convs must exist, as DeformConvASPP::new loads them (aspp.rs:39-45)
        const float* ow = wt.get(cp + "offset_conv.weight", {2 * kk, IC, k, k})->data;
        const float* ob = wt.get(cp + "offset_conv.bias", {2 * kk})->data;
        const float* mw = wt.get(cp + "modulator_conv.weight", {kk, IC, k, k})->data;
        const float* mb = wt.get(cp + "modulator_conv.bias", {kk})->data;
        d.regular = conv_bn(wt, cp + "regular_conv", false, mods[i] + "bn", PL, IC, ICP, k, k / 2, ACT_RELU, own, wb);
        if (deform_mode == BRN_DEFORM_DEFORMABLE) {
            d.regular.mode = GEMM_DEFORM_NHWC;
            attach_deform_frags(own, wb, d.regular, wt.get(cp + "regular_conv.weight", {PL, IC, k, k})->data);
            // offset_conv and modulator_conv stacked on N = 3 k^2, padded with zero filters to a multiple of 8 (3 / 27 / 147 -> 8 / 32 / 152): the
            // fp32 offset map then leaves the bf16 GEMM through its vector-store epilogue instead of the per-element one
            const int n3p = roundup(3 * kk, switches().offmod_pad8 ? 8 : 4);   // (A/B switch BRN_OFFMOD_PAD8: 0 = pad to 4 as before)
            std::vector<float> w3((size_t)n3p * IC * kk, 0.f), b3((size_t)n3p, 0.f);
            memcpy(w3.data(), ow, (size_t)2 * kk * IC * kk * sizeof(float));
            memcpy(w3.data() + (size_t)2 * kk * IC * kk, mw, (size_t)kk * IC * kk * sizeof(float));
            memcpy(b3.data(), ob, (size_t)2 * kk * sizeof(float));
            memcpy(b3.data() + 2 * kk, mb, (size_t)kk * sizeof(float));
            d.offmod = make_conv_nhwc(own, wb, w3.data(), b3.data(), n3p, IC, ICP, k, k, 1, k / 2, 1);
        }
    }
    if (deform_mode == BRN_DEFORM_REFERENCE_CPU) {
        // aspp1 and aspp_deforms.0 are both plain 1x1 IC->256 convs of the same input on the CPU path
        // (aspp.rs:183-185): one GEMM with N = 512 writes both concat slices (K = ICP: zero columns for the pad channels).
        const float* w0 = wt.get(mods[0] + "atrous_conv.regular_conv.weight", {PL, IC, 1, 1})->data;
        const float* w1 = wt.get(mods[1] + "atrous_conv.regular_conv.weight", {PL, IC, 1, 1})->data;
        std::vector<float> w2((size_t)2 * PL * ICP, 0.f);
        for (int n = 0; n < PL; ++n) {
            memcpy(&w2[(size_t)n * ICP], &w0[(size_t)n * IC], (size_t)IC * sizeof(float));
            memcpy(&w2[(size_t)(PL + n) * ICP], &w1[(size_t)n * IC], (size_t)IC * sizeof(float));
        }
        a.k1pair = make_linear(own, wb, w2.data(), nullptr, 2 * PL, ICP);
        BNHost h0 = get_bn(wt, mods[0] + "bn", PL), h1 = get_bn(wt, mods[1] + "bn", PL);
        std::vector<float> g(2 * PL), b(2 * PL), m(2 * PL), v(2 * PL);
        for (int n = 0; n < PL; ++n) {
            g[n] = h0.g[n]; b[n] = h0.b[n]; m[n] = h0.m[n]; v[n] = h0.v[n];
            g[PL + n] = h1.g[n]; b[PL + n] = h1.b[n]; m[PL + n] = h1.m[n]; v[PL + n] = h1.v[n];
        }
        fold_bn(own, a.k1pair, nullptr, g.data(), b.data(), m.data(), v.data(), 1e-5f);
        a.k1pair.act = ACT_RELU;
    }
    // global_avg_pool.1 (conv, no bias) + .2 (BN) (aspp.rs:271-278); rows padded to ICP like the pooled vector
    {
        const float* gw = wt.get(ap + "global_avg_pool.1.weight", {PL, IC, 1, 1})->data;
        std::vector<float> gp((size_t)PL * ICP, 0.f);
        for (int n = 0; n < PL; ++n) memcpy(&gp[(size_t)n * ICP], &gw[(size_t)n * IC], (size_t)IC * sizeof(float));
        a.gap_w = own.upload(gp);
        BNHost h = get_bn(wt, ap + "global_avg_pool.2", PL);
        std::vector<float> sc(PL), sh(PL);
        for (int n = 0; n < PL; ++n) {
            const double s = (double)h.g[n] / std::sqrt((double)h.v[n] + 1e-5);
            sc[n] = (float)s; sh[n] = (float)((0.0 - (double)h.m[n]) * s + (double)h.b[n]);
        }
        a.gap_scale = own.upload(sc); a.gap_shift = own.upload(sh);
    }
    // conv1 1x1 1280->OC no bias + bn1 + ReLU (aspp.rs:282-290, 329-331).  The first 1024 input channels are the four
    // spatial branches (a GEMM); the last 256 are the pooled branch, constant over the map -> a per-image bias.
    {
        const float* cw = wt.get(ap + "conv1.weight", {OC, 5 * PL, 1, 1})->data;
        a.conv1_full = own.upload(cw, (size_t)OC * 5 * PL);
        std::vector<float> mainw((size_t)OC * 4 * PL);
        for (int o = 0; o < OC; ++o) memcpy(&mainw[(size_t)o * 4 * PL], &cw[(size_t)o * 5 * PL], (size_t)4 * PL * sizeof(float));
        a.conv1_main = make_linear(own, wb, mainw.data(), nullptr, OC, 4 * PL);
        BNHost h = get_bn(wt, ap + "bn1", OC);
        fold_bn(own, a.conv1_main, nullptr, h.g, h.b, h.m, h.v, 1e-5f);
        a.conv1_main.act = ACT_RELU;
    }
}

// ---- BiRefNetDecoder::new (birefnet.rs:170-273) -------------------------------------------------------------------------
void build_decoder_weights(const WeightTable& wt, const std::string& p, const brn_config& cfg, DeviceOwner& own, WeightBuild wb, DecoderW& out) {
    int lat[4];
    brn_config_lateral_channels(&cfg, lat);                      // [384,768,1536,3072]
    const int ipt_out[5] = {48, 96, 192, 384, 384};              // birefnet.rs:180
    const int ipt_in[5] = {3, ipt_out[0], lat[0] / 2, lat[2] / 2, lat[3]};   // birefnet.rs:189-193
    // what image2patches really delivers at each scale (birefnet.rs:304-316): 3*g*g channels
    const int patch_ch[5] = {3, 48, 192, 768, 3072};
    for (int i = 0; i < 5; ++i)
        if (ipt_in[i] != patch_ch[i])
            fail(BRN_ERR_INVALID_ARG, "ipt_blk%d expects %d channels but image2patches yields %d: only the Swin-L channel plan "
                 "[192,384,768,1536] with mul_scl_ipt is self-consistent in the reference (birefnet.rs:189-193,304-316)",
                 i + 1, ipt_in[i], patch_ch[i]);
    // ipt_blk1 (conv1 3->64, conv_out 64->48, no activation) is composed with conv_out1's ipt slice into one stencil below
    for (int i = 1; i < 5; ++i) {
        const std::string ip = p + "ipt_blk" + std::to_string(i + 1) + ".";
        const int cin = ipt_in[i], cinp = roundup(cin, 32);
        const float* w = wt.get(ip + "conv1.weight", {64, cin, 3, 3})->data;
        const float* b = wt.get(ip + "conv1.bias", {64})->data;
        out.ipt[i].conv1 = make_conv_nhwc(own, wb, w, b, 64, cin, cinp, 3, 3, 1, 1, 1);
        const float* w2 = wt.get(ip + "conv_out.weight", {ipt_out[i], 64, 3, 3})->data;
        const float* b2 = wt.get(ip + "conv_out.bias", {ipt_out[i]})->data;
        // bf16-storage mode: the consumer of ipt_blk2 (decoder_block1.conv_in, 384 + 96 = 480 input channels) reads a map padded to 512
        // channels so that its K loop can run chunk-major (attach_planes); the 32 pad channels must hold zeros, and the cheapest writer
        // is this conv with 32 extra all-zero output channels (weights and bias zero: exact zeros, no activation follows)
        const int opad = (wb.planes == BUILD_BF16 && ipt_out[i] == 96) ? 128 : ipt_out[i];
        if (opad != ipt_out[i]) {
            std::vector<float> wz((size_t)opad * 64 * 9, 0.f), bz(opad, 0.f);
            memcpy(wz.data(), w2, (size_t)ipt_out[i] * 64 * 9 * sizeof(float));
            memcpy(bz.data(), b2, (size_t)ipt_out[i] * sizeof(float));
            out.ipt[i].conv_out = make_conv_nhwc(own, wb, wz.data(), bz.data(), opad, 64, 64, 3, 3, 1, 1, 1);
        } else
        out.ipt[i].conv_out = make_conv_nhwc(own, wb, w2, b2, ipt_out[i], 64, 64, 3, 3, 1, 1, 1);
    }
    const int dec_out[4] = {lat[2], lat[1], lat[0], lat[0] / 2};          // [1536,768,384,192] birefnet.rs:202
    const int dec_in[4] = {lat[3] + ipt_out[4], dec_out[0] + ipt_out[3], dec_out[1] + ipt_out[2], dec_out[2] + ipt_out[1]};
    const char* dnames[4] = {"decoder_block4.", "decoder_block3.", "decoder_block2.", "decoder_block1."};
    for (int i = 0; i < 4; ++i)
        build_decblk_weights(wt, p + dnames[i], dec_in[i], dec_out[i], cfg.deform_mode, own, wb, out.dec[i]);
    const char* lnames[3] = {"lateral_block4.conv", "lateral_block3.conv", "lateral_block2.conv"};
    const int lch[3] = {lat[2], lat[1], lat[0]};
    for (int i = 0; i < 3; ++i) {
        const float* w = wt.get(p + lnames[i] + ".weight", {lch[i], lch[i], 1, 1})->data;
        const float* b = wt.get(p + lnames[i] + ".bias", {lch[i]})->data;
        out.lat[i] = make_linear(own, wb, w, b, lch[i], lch[i]);
    }
    const char* sfx[3] = {"4", "3", "2"};
    for (int i = 0; i < 3; ++i) {
        const std::string gp = p + "gdt_convs_" + sfx[i];
        out.gdt[i] = conv_bn(wt, gp + ".0", true, gp + ".1", 16, dec_out[i], dec_out[i], 3, 1, ACT_RELU, own, wb);
        const std::string apn = p + "gdt_convs_attn_" + sfx[i] + ".0";
        out.gdt_attn_w[i] = own.upload(wt.get(apn + ".weight", {1, 16, 1, 1})->data, 16);
        out.gdt_attn_b[i] = wt.get(apn + ".bias", {1})->data[0];
        // loaded-but-unused heads must exist (birefnet.rs:230-232, 241-243)
        const std::string ppn = p + "gdt_convs_pred_" + sfx[i] + ".0";
        (void)wt.get(ppn + ".weight", {1, 16, 1, 1}); (void)wt.get(ppn + ".bias", {1});
        const std::string msn = p + "conv_ms_spvn_" + sfx[i];
        (void)wt.get(msn + ".weight", {1, dec_out[i], 1, 1}); (void)wt.get(msn + ".bias", {1});
    }
    // conv_out1.0: 1x1, 240 -> 1 (birefnet.rs:237-238).  w[0:192] acts on p1 (at 1/4 resolution, see final_head_kernel);
    // w[192:240] acts on ipt1 = ipt_blk1.conv_out(u) + b: composed here into one 3x3 64->1 stencil (fp64 accumulate).
    {
        const int fin = dec_out[3] + ipt_out[0];
        const float* ow = wt.get(p + "conv_out1.0.weight", {1, fin, 1, 1})->data;
        out.out_b = wt.get(p + "conv_out1.0.bias", {1})->data[0];
        out.out_w = own.upload(ow, fin);
        const float* w2 = wt.get(p + "ipt_blk1.conv_out.weight", {ipt_out[0], 64, 3, 3})->data;
        const float* b2 = wt.get(p + "ipt_blk1.conv_out.bias", {ipt_out[0]})->data;
        std::vector<float> tw(9 * 64);
        for (int t = 0; t < 9; ++t)
            for (int ci = 0; ci < 64; ++ci) {
                double s = 0.0;
                for (int o = 0; o < ipt_out[0]; ++o) s += (double)ow[dec_out[3] + o] * (double)w2[((size_t)o * 64 + ci) * 9 + t];
                tw[t * 64 + ci] = (float)s;
            }
        double tb = 0.0;
        for (int o = 0; o < ipt_out[0]; ++o) tb += (double)ow[dec_out[3] + o] * (double)b2[o];
        // One level further: ipt_blk1.conv1 (3x3, 3 -> 64, pad 1, bias b1) feeds that stencil with nothing in between
        // (SimpleConvs has no activation, decoder.rs:52), so t = stencil3x3(conv1(x)) is ONE 5x5, 3 -> 1 stencil on the image:
        //   t(p) = tb + sum_{d in D(p)} sum_ci tw[d][ci] * (b1[ci] + sum_e sum_c W1[ci][c][e] * x[c][p+d+e])
        // where D(p) = the taps d of the outer 3x3 whose centre p+d lies inside the image (the outer conv zero-pads conv1's
        // OUTPUT, it does not extend it): 3 x 3 border cases (first / inner / last row, same for columns), each with its own
        // composed kernel K[f = d+e][c] and bias.  x itself is zero-padded, as conv1 does.  fp64 accumulation on the host.
        const float* w1 = wt.get(p + "ipt_blk1.conv1.weight", {64, 3, 3, 3})->data;
        const float* b1 = wt.get(p + "ipt_blk1.conv1.bias", {64})->data;
        std::vector<float> hk(9 * 75), hb(9);
        for (int cy = 0; cy < 3; ++cy)
            for (int cx = 0; cx < 3; ++cx) {
                std::vector<double> K(75, 0.0);
                double bias = tb;
                for (int dy = -1; dy <= 1; ++dy) {
                    if ((cy == 0 && dy < 0) || (cy == 2 && dy > 0)) continue;
                    for (int dx = -1; dx <= 1; ++dx) {
                        if ((cx == 0 && dx < 0) || (cx == 2 && dx > 0)) continue;
                        const int t = (dy + 1) * 3 + (dx + 1);
                        for (int ci = 0; ci < 64; ++ci) {
                            const double a = tw[t * 64 + ci];
                            bias += a * (double)b1[ci];
                            for (int c = 0; c < 3; ++c)
                                for (int ey = -1; ey <= 1; ++ey)
                                    for (int ex = -1; ex <= 1; ++ex)
                                        K[((dy + ey + 2) * 5 + (dx + ex + 2)) * 3 + c] +=
                                            a * (double)w1[(((size_t)ci * 3 + c) * 3 + (ey + 1)) * 3 + (ex + 1)];
                        }
                    }
                }
                for (int i = 0; i < 75; ++i) hk[(cy * 3 + cx) * 75 + i] = (float)K[i];
                hb[cy * 3 + cx] = (float)bias;
            }
        out.head_k = own.upload(hk);
        out.head_b = own.upload(hb);
    }
}

}  // namespace brn
