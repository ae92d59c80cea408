// Stand-alone driver of the pure weight packers (candle_birefnet_amd/csrc/brn_pack.h) for tests/test_weight_pack_cpu.py:
//   weight_pack <packer> <in.f32> <out.u16> <ints...>     reads the fp32 matrix, writes what the packer returns
#include "brn_pack.h"
#include <cstdio>
#include <cstdlib>
#include <string>

int main(int argc, char** argv) {
    if (argc < 4) return 2;
    const std::string what = argv[1];
    auto arg = [&](int i) { return 4 + i < argc ? atoi(argv[4 + i]) : 0; };
    FILE* f = fopen(argv[2], "rb");
    if (!f) return 3;
    fseek(f, 0, SEEK_END);
    std::vector<float> in((size_t)ftell(f) / 4);
    fseek(f, 0, SEEK_SET);
    if (fread(in.data(), 4, in.size(), f) != in.size()) return 3;
    fclose(f);
    std::vector<uint16_t> out;
    if (what == "planes") out = brn::pack_bf16_planes(in, arg(0), arg(1));                    // K np
    else if (what == "half2") {                                                              // K; the scale's bits follow the planes
        float sc = 0.f;
        out = brn::pack_half2_planes(in, arg(0), &sc);
        uint16_t b[2];
        memcpy(b, &sc, 4);
        out.push_back(b[0]); out.push_back(b[1]);
    } else if (what == "s16") {                                                              // K f16 conv_taps cinp; rows, ld, chunk_major follow
        const brn::S16Storage s = brn::pack_s16_storage(in, arg(0), arg(1) != 0, arg(2), arg(3));
        out = s.w;
        out.push_back((uint16_t)s.rows); out.push_back((uint16_t)s.ld); out.push_back(s.chunk_major ? 1 : 0);
    } else if (what == "dense") out = brn::pack_frags(in.data(), arg(0), arg(0), arg(1), arg(1), 1, arg(2) != 0);   // N K f16: a Linear, rows as they are
    else if (what == "deform") out = brn::pack_frags(in.data(), arg(0), (arg(0) + 255) / 256 * 256, arg(1), arg(2), arg(3), arg(4) != 0);   // N Cin Cinp taps f16: a conv, rows to 256
    else return 2;
    f = fopen(argv[3], "wb");
    if (!f || fwrite(out.data(), 2, out.size(), f) != out.size()) return 4;
    fclose(f);
    return 0;
}
