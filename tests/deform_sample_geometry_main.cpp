// Stand-alone check of candle_birefnet_amd/csrc/kernels/deform_sample_geometry.h (tests/test_deform_offsets_cpu.py compiles it with the
// host compiler under AddressSanitizer / UBSan): the header against brute force over small maps, sample points exactly on -1, H and W,
// and offsets of +-1e30, +-inf and NaN.  Prints "cases <n> samples <m>" and "ok"; exits 1 at the first mismatch.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <vector>
#include "kernels/deform_sample_geometry.h"

using namespace brn;

static long long n_cases = 0, n_samples = 0;

#define CHECK(cond, ...)                                      \
    do {                                                      \
        if (!(cond)) {                                        \
            std::printf("FAILED %s: ", #cond);                \
            std::printf(__VA_ARGS__);                         \
            std::printf("\n");                                \
            std::exit(1);                                     \
        }                                                     \
    } while (0)

// the bilinear footprint of (y, x) on an H x W map, written as a sum over every pixel (torchvision's rule: the point counts when it lies
// in (-1, H) x (-1, W); the corners are floor and floor + 1; a corner outside the image contributes nothing)
static std::vector<double> brute(double y, double x, int H, int W) {
    std::vector<double> f((size_t)H * W, 0.0);
    if (!(y > -1.0 && y < H && x > -1.0 && x < W)) return f;
    const double yf = std::floor(y), xf = std::floor(x);
    for (int py = 0; py < H; ++py)
        for (int px = 0; px < W; ++px) {
            double wy = 0.0, wx = 0.0;
            if (py == (int)yf) wy = 1.0 - (y - yf);
            else if (py == (int)yf + 1) wy = y - yf;
            if (px == (int)xf) wx = 1.0 - (x - xf);
            else if (px == (int)xf + 1) wx = x - xf;
            f[(size_t)py * W + px] = wy * wx;
        }
    return f;
}

static void check_point(float y, float x, int H, int W) {
    const DeformSample s = deform_sample(y, x, H, W);
    std::vector<double> got((size_t)H * W, 0.0);
    for (int c = 0; c < 4; ++c) {
        CHECK(s.idx[c] >= 0 && s.idx[c] < H * W, "corner %d index %d outside a %d x %d map (y %g, x %g)", c, s.idx[c], H, W, (double)y, (double)x);
        if (s.ok & (1u << c)) got[(size_t)s.idx[c]] += (double)s.w[c];
        else CHECK(s.w[c] == 0.f, "corner %d is not real but has weight %g (y %g, x %g)", c, (double)s.w[c], (double)y, (double)x);
    }
    const std::vector<double> want = brute((double)y, (double)x, H, W);
    for (int i = 0; i < H * W; ++i)
        CHECK(std::fabs(got[(size_t)i] - want[(size_t)i]) <= 1e-6, "pixel %d of %d x %d: %g, brute force %g (y %g, x %g)", i, H, W, got[(size_t)i], want[(size_t)i],
              (double)y, (double)x);
    ++n_samples;
}

static void check_dead(float y, float x, int H, int W) {
    const DeformSample s = deform_sample(y, x, H, W);
    CHECK(s.ok == 0u, "(y %g, x %g) on %d x %d must not count", (double)y, (double)x, H, W);
    for (int c = 0; c < 4; ++c) CHECK(s.w[c] == 0.f && s.idx[c] >= 0 && s.idx[c] < H * W, "corner %d of a dead sample: weight %g index %d", c, (double)s.w[c], s.idx[c]);
    ++n_samples;
}

int main() {
    // (a) samples on a quarter-step grid that reaches two pixels beyond every border, maps of 1 x 1 to 4 x 5
    for (int H = 1; H <= 4; ++H)
        for (int W = 1; W <= 5; ++W) {
            ++n_cases;
            for (int qy = -12; qy <= 4 * (H + 2); ++qy)
                for (int qx = -12; qx <= 4 * (W + 2); ++qx) check_point(0.25f * (float)qy, 0.25f * (float)qx, H, W);
            // irregular fractions too
            for (int i = 0; i < 64; ++i) check_point(-1.3f + 0.137f * (float)i, -1.1f + 0.093f * (float)i, H, W);
            // (b) exactly on the open ends of the range, and just inside them
            const float in = 0.5f;
            check_dead(-1.f, in, H, W); check_dead((float)H, in, H, W); check_dead(in, -1.f, H, W); check_dead(in, (float)W, H, W);
            check_point(std::nextafterf(-1.f, 0.f), 0.f, H, W); check_point(std::nextafterf((float)H, 0.f), 0.f, H, W);
            check_point(0.f, std::nextafterf(-1.f, 0.f), H, W); check_point(0.f, std::nextafterf((float)W, 0.f), H, W);
            // (c) coordinates no int can hold, and NaN: the range test on the floats ends them before any conversion
            const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
            const float bad[] = {1e30f, -1e30f, inf, -inf, nan, 3e9f, -3e9f};
            for (float v : bad) {
                // as the kernels form them: origin + offset
                check_dead(2.f + v, in, H, W); check_dead(in, 2.f + v, H, W); check_dead(2.f + v, 2.f + v, H, W);
            }
            check_dead(inf + -inf, in, H, W);
        }
    // (d) the output size against counting the positions where the dilated kernel fits the padded extent
    for (int in = 1; in <= 9; ++in)
        for (int k = 1; k <= 4; ++k)
            for (int stride = 1; stride <= 3; ++stride)
                for (int pad = 0; pad <= 3; ++pad)
                    for (int dil = 1; dil <= 3; ++dil) {
                        ++n_cases;
                        long long count = 0;
                        for (int o = 0; o < 64; ++o)
                            if ((long long)o * stride + (long long)dil * (k - 1) <= (long long)in + 2 * pad - 1) ++count;
                        CHECK(deform_out_size(in, k, stride, pad, dil) == count, "out size(in %d, k %d, stride %d, pad %d, dil %d) = %lld, counted %lld", in, k, stride,
                              pad, dil, deform_out_size(in, k, stride, pad, dil), count);
                        for (int o = 0; o < (int)count; ++o)
                            for (int t = 0; t < k; ++t) CHECK(deform_tap_origin(o, t, stride, pad, dil) == o * stride - pad + t * dil, "tap origin");
                    }
    CHECK(deform_out_size(2147483647, 1, 1, 1073741823, 1) == 2147483647LL + 2LL * 1073741823, "out size near the int range");
    CHECK(deform_out_size(3, 5, 2, 0, 1) == 0, "a kernel that does not fit gives no output");
    // (e) groups and channels: every (group, tap) owns two offset channels and one mask channel, all distinct and dense
    for (int G = 1; G <= 4; ++G)
        for (int cpg = 1; cpg <= 5; ++cpg)
            for (int taps = 1; taps <= 6; ++taps) {
                ++n_cases;
                const int C = G * cpg;
                std::vector<int> off_seen((size_t)2 * G * taps, 0), mask_seen((size_t)G * taps, 0);
                for (int c = 0; c < C; ++c) {
                    const int g = deform_group_of(c, C, G);
                    CHECK(g == c / cpg && g >= 0 && g < G, "group of channel %d of %d in %d groups: %d", c, C, G, g);
                }
                for (int g = 0; g < G; ++g)
                    for (int t = 0; t < taps; ++t) {
                        const int oc = deform_offset_channel(g, t, taps), mc = deform_mask_channel(g, t, taps);
                        CHECK(oc >= 0 && oc + 1 < 2 * G * taps && mc >= 0 && mc < G * taps, "channel range");
                        ++off_seen[(size_t)oc]; ++off_seen[(size_t)oc + 1]; ++mask_seen[(size_t)mc];
                    }
                for (int v : off_seen) CHECK(v == 1, "offset channels are not a bijection");
                for (int v : mask_seen) CHECK(v == 1, "mask channels are not a bijection");
            }
    std::printf("cases %lld samples %lld\nok\n", n_cases, n_samples);
    return 0;
}
