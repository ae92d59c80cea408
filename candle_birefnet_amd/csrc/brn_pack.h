// brn_pack.h — the 16-bit weight layouts as pure host functions (no HIP): brn_weights.cpp uploads what they return, and
// tests/test_weight_pack_cpu.py checks them against a restatement of the layouts documented here.
#pragma once
#include <stdint.h>
#include <stddef.h>
#include <string.h>
#include <cmath>
#include <algorithm>
#include <vector>

namespace brn {

static inline uint16_t bf16_rne(float x) {            // round-to-nearest-even fp32 -> bf16 (finite inputs)
    uint32_t u;
    memcpy(&u, &x, 4);
    u += 0x7FFFu + ((u >> 16) & 1u);
    return (uint16_t)(u >> 16);
}
static inline float bf16_to_f32(uint16_t h) {
    uint32_t u = (uint32_t)h << 16;
    float f;
    memcpy(&f, &u, 4);
    return f;
}
static inline uint16_t f16_rne(float x) {             // round-to-nearest-even fp32 -> fp16 (finite inputs; |x| >= 65520 -> Inf)
    uint32_t u;
    memcpy(&u, &x, 4);
    const uint16_t sign = (uint16_t)((u >> 16) & 0x8000u);
    u &= 0x7fffffffu;
    if (u >= 0x47800000u) return sign | 0x7c00u;
    if (u < 0x38800000u) {                             // below 2^-14: a multiple of 2^-24 — the ulp of fp32 numbers in [0.5, 1)
        float f;
        memcpy(&f, &u, 4);
        f += 0.5f;
        uint32_t v;
        memcpy(&v, &f, 4);
        return sign | (uint16_t)(v - 0x3f000000u);
    }
    uint32_t v = u - 0x38000000u;
    v += 0xfffu + ((v >> 13) & 1u);
    return sign | (uint16_t)(v >> 13);
}
static inline float f16_to_f32(uint16_t h) {
    const uint32_t sign = (uint32_t)(h & 0x8000u) << 16, e = (h >> 10) & 31u, m = h & 0x3ffu;
    float f;
    if (e == 0) { f = (float)m * 5.9604644775390625e-08f; uint32_t u; memcpy(&u, &f, 4); u |= sign; memcpy(&f, &u, 4); return f; }
    const uint32_t u = sign | ((e == 31 ? 255u : e + 112u) << 23) | (m << 13);
    memcpy(&f, &u, 4);
    return f;
}
static inline uint16_t s16_rne(float x, bool f16) { return f16 ? f16_rne(x) : bf16_rne(x); }   // the 16-bit storage type of the build (BRN_BF16 / BRN_F16)

// error-free split of the packed fp32 matrix pk [rows][K] into np bf16 planes: plane p = RN_bf16(x - sum of the previous planes),
// stored interleaved per 32-deep K tile: [row][K/32][plane][32] (a (row, K tile) is np x 64 contiguous bytes)
static inline std::vector<uint16_t> pack_bf16_planes(const std::vector<float>& pk, size_t K, int np) {
    const size_t n = pk.size();
    std::vector<uint16_t> planes(n * np);
    for (size_t i = 0; i < n; ++i) {
        const size_t row = i / K, k = i - row * K;
        float r = pk[i];
        for (int p = 0; p < np; ++p) {
            const uint16_t h = bf16_rne(r);
            planes[(row * (K / 32) + k / 32) * (size_t)np * 32 + (size_t)p * 32 + (k & 31)] = h;
            r -= bf16_to_f32(h);
        }
    }
    return planes;
}

// mode f32_half2: hi = RN_f16(s w), lo = RN_f16(s w - hi), s = 2^k with max |w| s in (2^13, 2^14] — both planes of every weight that
// matters are normal fp16 numbers (hi + lo = s w up to 2^-22), and what falls below 2^-14 is 2^-38 of the largest weight.
// Same interleaving as pack_bf16_planes with two planes; *w_scale = s
static inline std::vector<uint16_t> pack_half2_planes(const std::vector<float>& pk, size_t K, float* w_scale) {
    const size_t n = pk.size();
    float mx = 0.f;
    for (size_t i = 0; i < n; ++i) mx = std::max(mx, fabsf(pk[i]));
    int k = 0;
    if (mx > 0.f && std::isfinite(mx)) { int ex; frexpf(mx, &ex); k = 14 - ex; }     // mx = f 2^ex, f in [0.5, 1): mx 2^k in [2^13, 2^14)
    k = std::max(-100, std::min(100, k));
    const float sc = ldexpf(1.f, k);
    std::vector<uint16_t> planes(n * 2);
    for (size_t i = 0; i < n; ++i) {
        const size_t row = i / K, kk = i - row * K;
        const float x = pk[i] * sc;
        const uint16_t h = f16_rne(x), l = f16_rne(x - f16_to_f32(h));
        const size_t o = (row * (K / 32) + kk / 32) * (size_t)64 + (kk & 31);
        planes[o] = h;
        planes[o + 32] = l;
    }
    *w_scale = sc;
    return planes;
}

// bf16-storage mode: W = RNE 16-bit of the packed matrix pk [rows][K] as [rows][ld], rows padded to 256, K to 64 (gemm_bf16.hip).
// Channels-last convs (conv_taps = kh kw > 0, K = conv_taps cinp) over more than one 64-channel chunk are stored chunk-major: K order
// (chunk, tap, channel in chunk) instead of pk's (tap, channel), so that the kh x kw taps of a chunk — which re-read the same input
// pixels — are consecutive K steps: the re-reads then hit L2 (tap-major order puts a whole Cin sweep of the tile's neighbourhood, > 4 MB
// for 32 concurrent tiles of the decoder's conv_in, between them)
struct S16Storage { std::vector<uint16_t> w; size_t rows = 0, ld = 0; bool chunk_major = false; };
static inline S16Storage pack_s16_storage(const std::vector<float>& pk, size_t K, bool f16, size_t conv_taps, size_t cinp) {
    S16Storage o;
    o.ld = (K + 63) / 64 * 64;
    const size_t nrows = pk.size() / K;
    o.rows = (nrows + 255) / 256 * 256;
    o.chunk_major = conv_taps > 0 && cinp % 64 == 0 && cinp > 64 && conv_taps * cinp == K;
    o.w.assign(o.rows * o.ld, 0);
    for (size_t r = 0; r < nrows; ++r)
        for (size_t k = 0; k < K; ++k) {
            size_t kd = k;
            if (o.chunk_major) { const size_t t = k / cinp, ci = k - t * cinp; kd = ((ci >> 6) * conv_taps + t) * 64 + (ci & 63); }
            o.w[r * o.ld + kd] = s16_rne(pk[r * K + k], f16);
        }
    return o;
}

// bf16-storage mode, the matrix in the order the MFMA consumes it: W[n][k] (k = (tap, ci), ci padded to Cinp; w is candle's [N][Cin][taps],
// a Linear's [N][K] with taps = 1) — fragment (n16 block, K step of 64, k32 half) is 1 KiB: lane l = 16 (k / 8 % 4) + n % 16 holds 8
// consecutive k — so a wave's fragment load is one contiguous read.  `rows` >= N rows are stored, the rest zero.  kernels/deform_bf16.hip
// reads convs with rows padded to 256, gemm_wstat_bf16_kernel Linears as they are.
static inline std::vector<uint16_t> pack_frags(const float* w, int N, int rows, int Cin, int Cinp, int taps, bool f16) {
    const int nk = taps * Cinp / 64;
    std::vector<uint16_t> wf((size_t)(rows / 16) * nk * 2 * 64 * 8, 0);
    for (int n = 0; n < N; ++n)
        for (int t = 0; t < taps; ++t)
            for (int ci = 0; ci < Cin; ++ci) {
                const int k = t * Cinp + ci;
                const int kt = k >> 6, s = (k >> 5) & 1, lane = ((k >> 3) & 3) * 16 + (n & 15), e = k & 7;
                wf[((((size_t)(n >> 4) * nk + kt) * 2 + s) * 64 + lane) * 8 + e] = s16_rne(w[((size_t)n * Cin + ci) * taps + t], f16);
            }
    return wf;
}

}  // namespace brn
