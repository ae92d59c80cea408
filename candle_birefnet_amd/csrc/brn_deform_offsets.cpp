// brn_deform_offsets.cpp — the two routes of brn_deform_conv2d_offsets_forward (brn_ops.cpp, which checks the arguments and stages the
// buffers; nothing else reaches this file, the graph files least of all): a deformable convolution with torchvision deform_conv2d
// semantics whose offsets and mask are the CALLER's tensors (DeformConv2dConfig, deform_conv.rs:120-132), not the output of the
// layer's own two convs.  DESIGN.md 3.5b.
//
//   route 1, fused     one offset group and the same stride / pad / dilation on both axes: what the gather loaders of every mode read
//                      (gemm_f32_kernel's GEMM_DEFORM_NHWC loader, DeformLoader of gemm_split.hip, both kernels of deform_bf16.hip: all
//                      four take kh and kw apart and add tap * dil to the window origin).  deform_om_pack_kernel turns the NCHW offset /
//                      mask into the fp32 map [B, Ho, Wo, ld] of GemmParams::om (multipliers, no sigmoid: om_sigmoid = 0; 1.0f without a
//                      mask), then run_conv with a GEMM_DEFORM_NHWC weight built exactly as brn_deform_conv2d_forward builds it — with
//                      the layer's offsets as the tensor, the layer's bits.
//   route 2, columns   everything else (offset groups, per-axis stride / pad / dilation): deform_im2col_kernel writes rows of the column
//                      matrix [pixels][kh kw Cp] in the mode's storage type, the mode's dense GEMM multiplies them by the [O][kh kw Cp]
//                      weight (K order (tap, channel), bias in the epilogue).  The column buffer is bounded by BRN_DEFORM_COL_MB: the
//                      pixel range is walked in chunks of whole rows, a multiple of 64 each (the last one ragged), never fewer than 64.
// Every buffer comes from the arena, sized by the arguments alone: a dry run plans exactly what the real run takes.
#include "brn_api_util.h"
#include "brn_graph.h"
#include "kernels/deform_sample_geometry.h"

namespace brn {

bool deform_offsets_fused_eligible(const DeformOffsetsParams& a) {
    return a.G == 1 && a.stride_h == a.stride_w && a.pad_h == a.pad_w && a.dil_h == a.dil_w;
}

DeformOffsetsPlan deform_offsets_prepare(DeviceOwner& own, WeightBuild op, const DeformOffsetsParams& a, const float* w, const float* bias, int O) {
    DeformOffsetsPlan pl;
    pl.geo = a;
    pl.fused = deform_offsets_fused_eligible(a);
    const bool planes = op.planes == 2 || op.planes == 3 || op.planes == BUILD_HALF2;
    if (pl.fused) {
        // as brn_deform_conv2d_forward: the 16-bit gather kernel writes 8 output channels a lane, so other widths take the fp32 kernel on
        // fp32 maps; its channel granule is 64, the fp32-class loaders' 32
        const bool s16 = op.planes == BUILD_BF16 && (O % 8) == 0;
        pl.Cp = roundup(a.C, s16 ? 64 : 32);
        const WeightBuild wb = (s16 || planes) ? op : WeightBuild{};
        pl.g = make_conv_nhwc(own, wb, w, bias, O, a.C, pl.Cp, a.kh, a.kw, a.stride_h, a.pad_h, a.dil_h);
        pl.g.mode = GEMM_DEFORM_NHWC;
        attach_deform_frags(own, wb, pl.g, w);
        pl.s16 = s16 ? (op.f16 ? 2 : 1) : 0;
        return pl;
    }
    const bool s16 = op.planes == BUILD_BF16;
    pl.Cp = roundup(a.C, 32);
    const WeightBuild wb = (s16 || planes) ? op : WeightBuild{};
    const int taps = a.kh * a.kw, K = taps * pl.Cp;
    // make_conv_nhwc's K order, (tap, channel) with zero columns for the pad channels, but through make_linear: the 16-bit copy of a conv
    // weight may be chunk-major (BRN_CONV_CHUNK_MAJOR), and the dense GEMM reads K as the columns lie
    std::vector<float> pk((size_t)O * K, 0.f);
    for (int o = 0; o < O; ++o)
        for (int ci = 0; ci < a.C; ++ci)
            for (int t = 0; t < taps; ++t) pk[(size_t)o * K + (size_t)t * pl.Cp + ci] = w[((size_t)o * a.C + ci) * taps + t];
    pl.g = make_linear(own, wb, pk.data(), bias, O, K);
    pl.s16 = s16 ? (op.f16 ? 2 : 1) : 0;
    return pl;
}

// rows of the column matrix per chunk: what BRN_DEFORM_COL_MB holds, rounded down to a multiple of 64, at least 64
static int column_chunk_rows(size_t row_bytes) {
    const long long mb = switches().deform_col_mb;
    const long long rows = ((mb > 0 ? mb : 0) << 20) / (long long)row_bytes / 64 * 64;
    return rows < 64 ? 64 : (rows > 0x7fffffc0LL ? 0x7fffffc0 : (int)rows);
}

void deform_offsets_route(Ctx& c, const DeformOffsetsPlan& pl, const Map& X, const Map& Y) {
    const DeformOffsetsParams& a = pl.geo;
    const int taps = a.kh * a.kw, M = a.B * a.Ho * a.Wo;
    if (X.B != a.B || X.H != a.H || X.W != a.W || X.C != pl.Cp || X.coff || Y.B != a.B || Y.H != a.Ho || Y.W != a.Wo || Y.C != pl.g.N || Y.coff || Y.ld != pl.g.N)
        fail(BRN_ERR_INVALID_ARG, "deform conv offsets: maps do not match the plan");
    if (pl.fused) {
        const int ld = roundup(3 * taps, 4);
        float* om = c.arena->alloc((size_t)M * ld);
        if (!c.dry) {
            DeformOffsetsParams p = a;
            p.om = om; p.om_ld = ld;
            BRN_LAUNCH(launch_deform_om_pack(p, c.stream));
        }
        const Map OM = Map(om, a.B, a.Ho, a.Wo, ld).window(0, 3 * taps);
        run_conv(c, pl.g, X, Y, ConvOpts().offsets(OM, 2 * taps, false));
        return;
    }
    const int K = taps * pl.Cp;
    const int chunk = column_chunk_rows((size_t)K * c.esz());
    const int buf_rows = chunk < M ? chunk : M;
    const size_t mk = c.arena->mark();
    float* col = c.arena->alloc_bytes((size_t)buf_rows * K * c.esz());
    for (int m0 = 0; m0 < M; m0 += chunk) {
        const int rows = M - m0 < chunk ? M - m0 : chunk;
        if (!c.dry) {
            DeformOffsetsParams p = a;
            p.x = X.p; p.ldx = X.ld; p.Cp = pl.Cp; p.s16 = c.bf16;
            p.col = col; p.m0 = m0; p.rows = rows;
            BRN_LAUNCH(launch_deform_im2col(p, c.stream));
        }
        // the chunk's rows as a [1, 1, rows, K] map through the dense weight into the same rows of Y (in-order stream: the next chunk's
        // im2col overwrites `col` after this product has read it)
        run_conv(c, pl.g, Map(col, 1, 1, rows, K), Map(c.at(Y.p, (size_t)m0 * Y.ld), 1, 1, rows, pl.g.N));
    }
    c.arena->release(mk);
}

}  // namespace brn
