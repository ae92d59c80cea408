// pack_main.cpp — kh_pack_weights of the GEMM harness as a stand-alone host program (tests/test_gemm_refs_cpu.py compiles it with the host
// compiler under AddressSanitizer / UBSan):  pack_main IN.f32 N K PLANES HALF OUT_PAD.f32 OUT_PLANES.u16  prints w_scale.
// The output buffers are sized exactly, so a write past what the entry point documents is caught.
#define KH_HOST_ONLY 1
#include "harness.cpp"
#include <cstdio>
#include <cstdlib>

static void dump(const char* path, const void* data, size_t bytes) {
    FILE* f = fopen(path, "wb");
    if (!f || (bytes && fwrite(data, 1, bytes, f) != bytes)) { fprintf(stderr, "cannot write %s\n", path); exit(2); }
    fclose(f);
}

int main(int argc, char** argv) {
    if (argc != 8) { fprintf(stderr, "usage: pack_main IN.f32 N K PLANES HALF OUT_PAD.f32 OUT_PLANES.u16\n"); return 2; }
    const int N = atoi(argv[2]), K = atoi(argv[3]), planes = atoi(argv[4]), half = atoi(argv[5]);
    std::vector<float> w((size_t)N * K);
    FILE* f = fopen(argv[1], "rb");
    if (!f || fread(w.data(), 4, w.size(), f) != w.size()) { fprintf(stderr, "cannot read %s\n", argv[1]); return 2; }
    fclose(f);
    const size_t npad = ((size_t)N + 127) / 128 * 128;
    std::vector<float> pad(npad * K);
    std::vector<uint16_t> pl(npad * K * planes);
    const float s = kh_pack_weights(w.data(), N, K, planes, half, pad.data(), planes ? pl.data() : nullptr);
    dump(argv[6], pad.data(), pad.size() * 4);
    dump(argv[7], pl.data(), pl.size() * 2);
    printf("%a\n", (double)s);
    return s > 0.f ? 0 : 1;
}
