// Stand-alone check of csrc/kernels/conv_halo_geometry.h (compiled and run by test_conv_halo_geometry_cpu.py under AddressSanitizer / UBSan):
// the tile <-> pixel map of the halo-staged conv kernel is a bijection onto [0, M), tiles never span two images and slices cover every channel
// chunk once; the predicate takes the model's twelve 3x3 launches of the two-plane modes and refuses what the kernel does not compute.
#include <cstdio>
#include <vector>

#include "kernels/conv_halo_geometry.h"

using namespace brn;

struct Params {      // the fields of GemmParams the header reads
    const void* Wp;
    int M, N, K, mode, lda, a_coff, Hin, Win, Cin, kh, kw, stride, pad, dil, Hout, Wout, planes, a_planes, c_planes, c_bf16, splitk;
};

static int failures = 0;
#define CHECK(cond, ...)                                  \
    do {                                                  \
        if (!(cond)) {                                    \
            ++failures;                                   \
            std::printf("FAILED %s: ", #cond);            \
            std::printf(__VA_ARGS__);                     \
            std::printf("\n");                            \
        }                                                 \
    } while (0)

static void check_map(int B, int H, int W) {
    const int M = B * H * W, tiles = conv_halo_tiles(B, H, W);
    std::vector<int> hits(M, 0);
    for (int t = 0; t < tiles; ++t) {
        const ConvHaloTile tl = conv_halo_tile(H, W, t);
        CHECK(tl.b >= 0 && tl.b < B && tl.y0 >= 0 && tl.y0 < H && tl.x0 >= 0 && tl.x0 < W && tl.y0 % HALO_TH == 0 && tl.x0 % HALO_TW == 0,
              "tile %d of %d x %d x %d starts at (%d, %d, %d)", t, B, H, W, tl.b, tl.y0, tl.x0);
        int inside = 0;
        for (int r = 0; r < HALO_BM; ++r) {
            const int m = conv_halo_row(H, W, tl, r);
            if (m < 0) continue;
            ++inside;
            CHECK(m < M && m / (H * W) == tl.b, "tile %d row %d -> m %d leaves image %d", t, r, m, tl.b);
            if (m >= 0 && m < M) ++hits[m];
            // a 16-row MFMA block is 16 consecutive x of one output row
            if (r % HALO_TW) { const int prev = conv_halo_row(H, W, tl, r - 1); CHECK(prev == m - 1, "tile %d rows %d, %d are not neighbours", t, r - 1, r); }
        }
        CHECK(inside > 0, "tile %d of %d x %d x %d is empty", t, B, H, W);
    }
    for (int m = 0; m < M; ++m) CHECK(hits[m] == 1, "%d x %d x %d: row %d computed %d times", B, H, W, m, hits[m]);
}

static void check_slices(int Cin, int S) {
    const int chunks = Cin / 32, per = conv_halo_chunks_per_slice(Cin, S);
    std::vector<int> hits(chunks, 0);
    for (int s = 0; s < S; ++s) {
        const int c0 = s * per, c1 = c0 + per < chunks ? c0 + per : chunks;
        for (int c = c0; c < c1; ++c) ++hits[c];
    }
    for (int c = 0; c < chunks; ++c) CHECK(hits[c] == 1, "Cin %d in %d slices: chunk %d contracted %d times", Cin, S, c, hits[c]);
}

static Params conv3x3(int M, int N, int K, int side, int splitk) {
    static const int w = 0;
    Params p{};
    p.Wp = &w;
    p.M = M; p.N = N; p.K = K; p.mode = HALO_CONV_MODE; p.Cin = K / 9; p.lda = p.Cin; p.a_coff = 0;
    p.Hin = p.Win = p.Hout = p.Wout = side;
    p.kh = p.kw = 3; p.stride = 1; p.pad = 1; p.dil = 1; p.planes = 2; p.splitk = splitk;
    return p;
}

int main() {
    static_assert(HALO_BM == 128 && HALO_PIXELS == 180, "8 x 16 pixels, a 10 x 18 halo");
    // the test geometries of conv_halo_cases.py and the model's five map sizes (1024^2 input: strides 4 .. 32, and the 16^2 map of a 512^2 input)
    const int maps[][3] = {{2, 11, 19}, {2, 5, 7}, {1, 9, 17}, {1, 16, 16}, {1, 32, 32}, {1, 64, 64}, {1, 128, 128}, {1, 256, 256}, {3, 8, 16}, {2, 1, 1}, {1, 17, 33}};
    for (const auto& g : maps) check_map(g[0], g[1], g[2]);
    const int cuts[][2] = {{96, 2}, {64, 3}, {64, 1}, {5760, 48}, {3456, 48}, {1920, 12}, {960, 3}, {480, 1}, {32, 64}};
    for (const auto& c : cuts) check_slices(c[0], c[1]);

    // the twelve launches of the flagship forward: decoder conv_in, gdt convs, ipt conv1 (M, N, K, map side, the plan's slices)
    const int model[][5] = {{1024, 64, 51840, 32, 48}, {1024, 64, 31104, 32, 48}, {4096, 64, 17280, 64, 12}, {16384, 64, 8640, 128, 3}, {65536, 64, 4320, 256, 1},
                            {1024, 16, 13824, 32, 48}, {4096, 16, 6912, 64, 12}, {16384, 16, 3456, 128, 3},
                            {1024, 64, 27648, 32, 48}, {4096, 64, 6912, 64, 12}, {16384, 64, 1728, 128, 3}, {65536, 64, 576, 256, 1}};
    for (const auto& m : model) {
        const Params p = conv3x3(m[0], m[1], m[2], m[3], m[4]);
        CHECK(conv_halo_eligible(p), "model launch %d x %d x %d refused", m[0], m[1], m[2]);
    }
    const Params ok = conv3x3(4096, 64, 6912, 64, 12);
    CHECK(conv_halo_eligible(ok), "the base of the refusals must be eligible");
    Params q = ok; q.stride = 2; q.Hout = q.Wout = 32; q.M = 1024;   CHECK(!conv_halo_eligible(q), "stride 2 accepted");
    q = ok; q.dil = 2; q.pad = 2;                                    CHECK(!conv_halo_eligible(q), "dilation 2 accepted");
    q = ok; q.kh = q.kw = 7; q.pad = 3; q.K = 49 * q.Cin;            CHECK(!conv_halo_eligible(q), "7 x 7 accepted");
    q = ok; q.Cin = 48; q.lda = 48; q.K = 9 * 48;                    CHECK(!conv_halo_eligible(q), "Cin %% 32 != 0 accepted");
    q = ok; q.planes = 3;                                            CHECK(!conv_halo_eligible(q), "three planes accepted");
    q = ok; q.mode = 0;                                              CHECK(!conv_halo_eligible(q), "a dense GEMM accepted");
    q = ok; q.Wp = nullptr;                                          CHECK(!conv_halo_eligible(q), "no weight planes accepted");
    q = ok; q.M = 4096 + 64;                                         CHECK(!conv_halo_eligible(q), "a partial image accepted");
    q = ok; q.a_coff = 2;                                            CHECK(!conv_halo_eligible(q), "an unaligned channel window accepted");
    q = ok; q.Hin = q.Win = q.Hout = q.Wout = 16384; q.M = 16384 * 16384; CHECK(!conv_halo_eligible(q), "a map beyond 32-bit byte offsets accepted");
    std::printf("%s\n", failures ? "failed" : "ok");
    return failures ? 1 : 0;
}
