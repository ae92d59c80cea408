// conv_halo_geometry.h — which launches the halo-staged 3x3 conv kernel (gemm_conv_halo.h) takes, and how its workgroups tile the output map.
// Plain integer arithmetic on the fields of GemmParams (brn_kernels.h), no HIP header needed: the launcher and the kernel (kernels/gemm_split.hip)
// use it, and a stand-alone CPU check (tests/test_conv_halo_geometry_cpu.py) walks it.  P = GemmParams, or any struct with the same fields.
#pragma once

#if defined(__HIP__)
#define BRN_HALO_HD __host__ __device__
#else
#define BRN_HALO_HD
#endif

namespace brn {

// A workgroup's M tile is a block of HALO_TH x HALO_TW output pixels of ONE image (row r of the tile = pixel (r / TW, r % TW) of the block: a
// 16-row MFMA block is 16 consecutive x of one output row), its N tile 64 columns.  The input it needs per 32-channel chunk is the block's
// (TH + 2) x (TW + 2) halo.  Blocks may overhang the right and the bottom edge of the map; they never span two images.
constexpr int HALO_TH = 8, HALO_TW = 16, HALO_BM = HALO_TH * HALO_TW, HALO_BN = 64;
constexpr int HALO_H = HALO_TH + 2, HALO_W = HALO_TW + 2, HALO_PIXELS = HALO_H * HALO_W;
constexpr int HALO_CONV_MODE = 1;      // GEMM_CONV_NHWC (gemm_split.hip asserts the two agree)

struct ConvHaloTile { int b, y0, x0; };       // image and first output pixel of a block

BRN_HALO_HD inline int conv_halo_tiles_y(int H) { return (H + HALO_TH - 1) / HALO_TH; }
BRN_HALO_HD inline int conv_halo_tiles_x(int W) { return (W + HALO_TW - 1) / HALO_TW; }
// blocks of a batch of `images` H x W maps; block ids walk x fastest, then y, then the image
BRN_HALO_HD inline int conv_halo_tiles(int images, int H, int W) { return images * conv_halo_tiles_y(H) * conv_halo_tiles_x(W); }
BRN_HALO_HD inline ConvHaloTile conv_halo_tile(int H, int W, int tile) {
    const int tx = conv_halo_tiles_x(W), per_image = conv_halo_tiles_y(H) * tx;
    const int b = tile / per_image, r = tile - b * per_image;
    const int ty = r / tx;
    return ConvHaloTile{b, ty * HALO_TH, (r - ty * tx) * HALO_TW};
}
// tile row r in [0, HALO_BM) -> the GEMM row m = (b, y, x) it computes, or -1 where the block overhangs the map
BRN_HALO_HD inline int conv_halo_row(int H, int W, const ConvHaloTile& t, int r) {
    const int y = t.y0 + r / HALO_TW, x = t.x0 + r % HALO_TW;
    return (y < H && x < W) ? (t.b * H + y) * W + x : -1;
}
// split-K: slice s of S contracts the 32-channel chunks [s * per, min(chunks, (s + 1) * per)), per = ceil(chunks / S); trailing slices may be empty
BRN_HALO_HD inline int conv_halo_chunks_per_slice(int Cin, int splitk) { return (Cin / 32 + splitk - 1) / splitk; }

// 3x3, stride 1, dilation 1, pad 1 over a channels-last fp32 map, two operand planes, whole 32-channel chunks, whole images, and one image
// (A) and one 64-row weight panel (W planes) within the 32-bit byte offsets of a buffer resource.
template <class P>
inline bool conv_halo_eligible(const P& p) {
    const bool conv_two_planes = p.mode == HALO_CONV_MODE && p.planes == 2 && p.Wp != nullptr && !p.a_planes && !p.c_planes && !p.c_bf16;
    const bool three_by_three_same = p.kh == 3 && p.kw == 3 && p.stride == 1 && p.dil == 1 && p.pad == 1 && p.Hout == p.Hin && p.Wout == p.Win;
    if (!conv_two_planes || !three_by_three_same || p.Hin <= 0 || p.Win <= 0 || p.Cin <= 0) return false;
    const bool whole_chunks = p.Cin % 32 == 0 && p.K == 9 * p.Cin && ((p.lda | p.a_coff) & 3) == 0 && p.a_coff + p.Cin <= p.lda;
    const bool whole_images = p.M > 0 && p.M % (p.Hout * p.Wout) == 0;
    const bool offsets_fit = (double)p.Hin * p.Win * p.lda * 4.0 < 2147483648.0 && (double)HALO_BN * p.K * 4.0 < 2147483648.0;
    return whole_chunks && whole_images && offsets_fit && p.splitk >= 1;
}

}  // namespace brn
