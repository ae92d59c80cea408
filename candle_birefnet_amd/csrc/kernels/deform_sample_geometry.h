// deform_sample_geometry.h — the index math of brn_deform_conv2d_offsets_forward (torchvision deform_conv2d semantics, SURVEY.md D1;
// the reference's DeformConv2dConfig, deform_conv.rs:101-215): kernels/deform_im2col.hip, its host route brn_deform_offsets.cpp, the entry's
// argument checks and a stand-alone CPU check (tests/test_deform_offsets_cpu.py) share it.  Plain arithmetic, no HIP header needed.
//
// Output pixel (oy, ox), tap t = ky kw + kx, offset group g sample the map at
//     y = oy stride_h - pad_h + ky dil_h + dy,   x = ox stride_w - pad_w + kx dil_w + dx
// with (dy, dx) = offset channels (2 (g kh kw + t), + 1).  The sample counts when y in (-1, H) and x in (-1, W); it is bilinear from
// (floor y, floor x), and a corner outside the image contributes zero.
//
// Order of operations in deform_sample: the range test is done on the FLOATS, before any float -> int conversion, and the integer clamps come
// after it.  A huge, infinite or NaN coordinate fails the test (every comparison with NaN is false) and never reaches a conversion, so it
// can neither steer an address nor be undefined behaviour on the host: such a sample contributes exactly 0.
#pragma once

#if defined(__HIPCC__)
#define BRN_DSG_HD __host__ __device__ __forceinline__
#else
#define BRN_DSG_HD inline
#endif

namespace brn {

// (in + 2 pad - dil (k - 1) - 1) / stride + 1 for in, k, stride, dil >= 1 and pad >= 0; 0 when the dilated kernel does not fit the padded
// extent (C division would round a negative numerator towards zero and answer 1).  64-bit: no intermediate overflows for int arguments
BRN_DSG_HD long long deform_out_size(int in, int k, int stride, int pad, int dil) {
    const long long num = (long long)in + 2LL * pad - (long long)dil * (k - 1) - 1;
    return num < 0 ? 0 : num / stride + 1;
}

// offset group of input channel c: G groups of C / G consecutive channels (C % G == 0)
BRN_DSG_HD int deform_group_of(int c, int C, int G) { return c / (C / G); }
// channel of the offset tensor [B, 2 G kh kw, Ho, Wo] that holds dy of (group, tap); dx is the next one
BRN_DSG_HD int deform_offset_channel(int g, int tap, int taps) { return 2 * (g * taps + tap); }
// channel of the mask tensor [B, G kh kw, Ho, Wo] of (group, tap)
BRN_DSG_HD int deform_mask_channel(int g, int tap, int taps) { return g * taps + tap; }
// the integer part of a sample coordinate: o stride - pad + k dil (the entry bounds in + 2 pad below 2^31, so this fits an int)
BRN_DSG_HD int deform_tap_origin(int o, int k, int stride, int pad, int dil) { return o * stride - pad + k * dil; }

// Four corners of one sample: pixel indices (row * W + column) CLAMPED into the image, the bilinear weights, and which corners are real.
// Order: (yl, xl), (yl, xh), (yh, xl), (yh, xh).  A corner that is not real has weight 0 and ok bit 0; its index points at a valid pixel
// whose value must not be used (select on ok, do not multiply: the pixel may hold a non-finite value)
struct DeformSample {
    int idx[4];
    float w[4];
    unsigned ok;       // bit c: corner c lies inside the image; 0 = the sample contributes nothing
};

BRN_DSG_HD DeformSample deform_sample(float y, float x, int H, int W) {
    DeformSample s;
    s.idx[0] = s.idx[1] = s.idx[2] = s.idx[3] = 0;
    s.w[0] = s.w[1] = s.w[2] = s.w[3] = 0.f;
    s.ok = 0u;
    // floats first: NaN, +-inf and anything beyond the map end here
    if (!(y > -1.f && y < (float)H && x > -1.f && x < (float)W)) return s;
    // y in (-1, H): floor(y) in [-1, H - 1], representable; the conversions are exact
    const float yf = __builtin_floorf(y), xf = __builtin_floorf(x);
    const int yl = (int)yf, xl = (int)xf;
    const float ly = y - yf, lx = x - xf, hy = 1.f - ly, hx = 1.f - lx;
    const bool yl_ok = yl >= 0, yh_ok = yl + 1 <= H - 1, xl_ok = xl >= 0, xh_ok = xl + 1 <= W - 1;
    // integer clamps, after the range test
    const int y0 = yl < 0 ? 0 : yl, y1 = yl + 1 > H - 1 ? H - 1 : yl + 1;
    const int x0 = xl < 0 ? 0 : xl, x1 = xl + 1 > W - 1 ? W - 1 : xl + 1;
    s.idx[0] = y0 * W + x0; s.idx[1] = y0 * W + x1; s.idx[2] = y1 * W + x0; s.idx[3] = y1 * W + x1;
    if (yl_ok && xl_ok) { s.w[0] = hy * hx; s.ok |= 1u; }
    if (yl_ok && xh_ok) { s.w[1] = hy * lx; s.ok |= 2u; }
    if (yh_ok && xl_ok) { s.w[2] = ly * hx; s.ok |= 4u; }
    if (yh_ok && xh_ok) { s.w[3] = ly * lx; s.ok |= 8u; }
    return s;
}

}  // namespace brn
