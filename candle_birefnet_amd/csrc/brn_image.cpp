// brn_image.cpp — image pre- and post-processing behind the extern "C" boundary (infer_image.rs:44-67, 84-110): the resampling axes,
// brn_preprocess_image, brn_postprocess_mask, brn_infer_images_u8.
#include "brn_api_util.h"
#include <cmath>
#include <algorithm>

using namespace brn;

namespace {

// One axis of image 0.25.9's resampler (imageops/sample.rs, horizontal_sample / vertical_sample): for every output index the
// first input index, the tap count and the normalised weights, computed in f32 in the crate's order of operations.
struct ResampleAxis {
    int in_n = 0, out_n = 0, max_taps = 0;
    std::vector<int> left, count;
    std::vector<float> w;      // [out_n][max_taps]
};
enum { FILTER_TRIANGLE = 0, FILTER_LANCZOS3 = 1 };

float sincf_image(float t) {
    const float a = t * 3.14159265358979323846f;     // f32::consts::PI
    return t == 0.0f ? 1.0f : sinf(a) / a;
}
float filter_kernel(int filter, float x) {
    if (filter == FILTER_TRIANGLE) return fabsf(x) < 1.0f ? 1.0f - fabsf(x) : 0.0f;
    return fabsf(x) < 3.0f ? sincf_image(x) * sincf_image(x / 3.0f) : 0.0f;
}
ResampleAxis make_axis(int in_n, int out_n, int filter) {
    ResampleAxis ax;
    ax.in_n = in_n; ax.out_n = out_n;
    const float support = filter == FILTER_TRIANGLE ? 1.0f : 3.0f;
    const float ratio = (float)in_n / (float)out_n;
    const float sratio = ratio < 1.0f ? 1.0f : ratio;
    const float src_support = support * sratio;
    ax.left.resize(out_n); ax.count.resize(out_n);
    std::vector<std::vector<float>> ws(out_n);
    for (int o = 0; o < out_n; ++o) {
        float inputx = ((float)o + 0.5f) * ratio;
        long l = (long)floorf(inputx - src_support);
        l = std::min<long>(std::max<long>(l, 0), (long)in_n - 1);
        long r = (long)ceilf(inputx + src_support);
        r = std::min<long>(std::max<long>(r, l + 1), (long)in_n);
        inputx = inputx - 0.5f;
        float sum = 0.0f;
        for (long i = l; i < r; ++i) {
            const float wv = filter_kernel(filter, ((float)i - inputx) / sratio);
            ws[o].push_back(wv);
            sum += wv;
        }
        for (float& v : ws[o]) v /= sum;
        ax.left[o] = (int)l; ax.count[o] = (int)(r - l);
        ax.max_taps = std::max(ax.max_taps, (int)(r - l));
    }
    ax.w.assign((size_t)out_n * ax.max_taps, 0.0f);
    for (int o = 0; o < out_n; ++o) std::copy(ws[o].begin(), ws[o].end(), ax.w.begin() + (size_t)o * ax.max_taps);
    return ax;
}
struct DevAxis { int* left; int* count; float* w; int max_taps; };
DevAxis upload_axis(DeviceOwner& own, const ResampleAxis& ax) {
    DevAxis d;
    d.left = reinterpret_cast<int*>(own.upload(reinterpret_cast<const float*>(ax.left.data()), ax.left.size()));
    d.count = reinterpret_cast<int*>(own.upload(reinterpret_cast<const float*>(ax.count.data()), ax.count.size()));
    d.w = own.upload(ax.w);
    d.max_taps = ax.max_taps;
    return d;
}
unsigned char* dev_bytes(DeviceOwner& own, size_t n) {
    std::vector<float> z((n + 3) / 4 + 4, 0.f);
    return reinterpret_cast<unsigned char*>(own.upload(z));
}

}  // namespace

extern "C" {

brn_status brn_preprocess_image(const unsigned char* pixels, int h, int w, int channels, int S, float* x_nchw, brn_mem out_loc,
                                int device, void* stream) {
    return guarded([&] {
        if (!pixels || !x_nchw) fail(BRN_ERR_INVALID_ARG, "null argument");
        if (h < 1 || w < 1 || S < 1 || !(channels == 3 || channels == 4))
            fail(BRN_ERR_INVALID_ARG, "preprocess: %dx%d image with %d channels to %d: need RGB8 or RGBA8 and positive sizes", h, w, channels, S);
        ensure_device(device);
        hipStream_t s = (hipStream_t)stream;
        DeviceOwner own;
        Staging so(stream, out_loc);
        float* dout = so.out(x_nchw, (size_t)3 * S * S);
        const ResampleAxis ay = make_axis(h, S, FILTER_TRIANGLE), ax = make_axis(w, S, FILTER_TRIANGLE);   // resize_exact(S, S, Triangle)
        const DevAxis dy = upload_axis(own, ay), dx = upload_axis(own, ax);
        unsigned char* din = dev_bytes(own, (size_t)h * w * channels);
        BRN_HIP(hipMemcpyAsync(din, pixels, (size_t)h * w * channels, hipMemcpyHostToDevice, s));
        std::vector<float> z((size_t)S * w * channels, 0.f);
        float* tmp = own.upload(z);                                    // the crate's intermediate Rgba32FImage (vertical pass first)
        const float mean[3] = {0.485f, 0.456f, 0.406f}, stdv[3] = {0.229f, 0.224f, 0.225f};    // infer_image.rs:53-54
        BRN_HIP(launch_resample_v_u8(din, h, w, channels, S, dy.left, dy.count, dy.w, dy.max_taps, tmp, s));
        BRN_HIP(launch_resample_h(tmp, S, w, channels, S, dx.left, dx.count, dx.w, dx.max_taps, nullptr, dout, mean, stdv, s));
        so.finish();
        BRN_HIP(hipStreamSynchronize(s));                               // `own` frees the temporaries when this scope ends
    });
}

brn_status brn_postprocess_mask(const float* logits, int S, brn_mem in_loc, int apply_sigmoid, int out_h, int out_w,
                                unsigned char* mask, int device, void* stream) {
    return guarded([&] {
        if (!logits || !mask) fail(BRN_ERR_INVALID_ARG, "null argument");
        if (S < 1 || out_h < 1 || out_w < 1) fail(BRN_ERR_INVALID_ARG, "postprocess: sizes must be positive");
        ensure_device(device);
        hipStream_t s = (hipStream_t)stream;
        DeviceOwner own;
        Staging si(stream, in_loc);
        const float* dl = si.in(logits, (size_t)S * S);
        unsigned char* m8 = dev_bytes(own, (size_t)S * S);
        BRN_HIP(launch_mask_u8(dl, (long)S * S, apply_sigmoid, m8, s));                       // infer_image.rs:84-99
        const ResampleAxis ay = make_axis(S, out_h, FILTER_LANCZOS3), ax = make_axis(S, out_w, FILTER_LANCZOS3);   // :103-108
        const DevAxis dy = upload_axis(own, ay), dx = upload_axis(own, ax);
        std::vector<float> z((size_t)out_h * S, 0.f);
        float* tmp = own.upload(z);
        unsigned char* dout = dev_bytes(own, (size_t)out_h * out_w);
        BRN_HIP(launch_resample_v_u8(m8, S, S, 1, out_h, dy.left, dy.count, dy.w, dy.max_taps, tmp, s));
        BRN_HIP(launch_resample_h(tmp, out_h, S, 1, out_w, dx.left, dx.count, dx.w, dx.max_taps, dout, nullptr, nullptr, nullptr, s));
        BRN_HIP(hipMemcpyAsync(mask, dout, (size_t)out_h * out_w, hipMemcpyDeviceToHost, s));
        BRN_HIP(hipStreamSynchronize(s));
    });
}

// examples/infer_image.rs:44-110 for a batch (see the header).  The staging pool: [raw images | vertical-pass temporaries (pre) |
// x batch | mask probabilities | u8 masks at S | vertical-pass temporaries (post) | u8 masks at the images' sizes]
brn_status brn_infer_images_u8(brn_model* mh, int n, const unsigned char* const* pixels, const int* heights, const int* widths, int channels, int S,
                               unsigned char* const* masks, void* stream) {
    return guarded([&] {
        if (!mh || !pixels || !heights || !widths || !masks || n < 1) fail(BRN_ERR_INVALID_ARG, "bad argument");
        if (!(channels == 3 || channels == 4) || S < 32 || S % 32) fail(BRN_ERR_INVALID_ARG, "infer_images: RGB8 / RGBA8 input and a model size that is a positive multiple of 32 (got %d channels, S = %d)", channels, S);
        Model& m = mh->m;
        if (m.decoder_only) fail(BRN_ERR_INVALID_ARG, "this handle holds only the decoder (brn_decoder_create)");
        for (int i = 0; i < n; ++i)
            if (!pixels[i] || !masks[i] || heights[i] < 1 || widths[i] < 1) fail(BRN_ERR_INVALID_ARG, "infer_images: image %d is null or empty", i);
        hipStream_t s = (hipStream_t)stream;
        std::lock_guard<std::mutex> io_lock(m.io_mu);      // the staging pool and the table cache belong to one call at a time
        auto al = [](size_t v) { return (v + 255) & ~(size_t)255; };
        std::vector<size_t> o_raw(n), o_tv(n), o_pv(n), o_out(n);
        size_t total = 0;
        for (int i = 0; i < n; ++i) { o_raw[i] = total; total += al((size_t)heights[i] * widths[i] * channels); }
        for (int i = 0; i < n; ++i) { o_tv[i] = total; total += al((size_t)S * widths[i] * channels * sizeof(float)); }
        const size_t o_x = total; total += al((size_t)n * 3 * S * S * sizeof(float));
        const size_t o_p = total; total += al((size_t)n * S * S * sizeof(float));
        const size_t o_m8 = total; total += al((size_t)n * S * S);
        for (int i = 0; i < n; ++i) { o_pv[i] = total; total += al((size_t)heights[i] * S * sizeof(float)); }
        for (int i = 0; i < n; ++i) { o_out[i] = total; total += al((size_t)heights[i] * widths[i]); }
        {
            std::lock_guard<std::mutex> lk(m.mu);
            BRN_HIP(hipSetDevice(m.device));
            if (total > m.io.cap) {
                if (m.io.base) { BRN_HIP(hipDeviceSynchronize()); (void)hipFree(m.io.base); m.io.base = nullptr; m.io.cap = 0; }
                void* d = nullptr;
                hipError_t e = hipMalloc(&d, total);
                if (e != hipSuccess) { (void)hipGetLastError(); fail(BRN_ERR_OOM, "hipMalloc of %zu bytes for the image staging failed: %s", total, hipGetErrorString(e)); }
                m.io.base = (char*)d; m.io.cap = total;
            }
        }
        // resampling tables, cached with the handle by (input size, output size, filter); uploaded once
        auto axis = [&](int in_n, int out_n, int filter) -> const Model::AxisDev& {
            std::lock_guard<std::mutex> lk(m.mu);
            for (const Model::AxisDev& a : m.axes) if (a.in_n == in_n && a.out_n == out_n && a.filter == filter) return a;
            const ResampleAxis ax = make_axis(in_n, out_n, filter);
            const DevAxis d = upload_axis(m.own, ax);
            m.axes.push_back({in_n, out_n, filter, d.max_taps, d.left, d.count, d.w});
            return m.axes.back();
        };
        char* base = m.io.base;
        float* x = reinterpret_cast<float*>(base + o_x);
        float* prob = reinterpret_cast<float*>(base + o_p);
        const float mean[3] = {0.485f, 0.456f, 0.406f}, stdv[3] = {0.229f, 0.224f, 0.225f};    // infer_image.rs:53-54
        for (int i = 0; i < n; ++i) {
            const int h = heights[i], w = widths[i];
            unsigned char* raw = reinterpret_cast<unsigned char*>(base + o_raw[i]);
            BRN_HIP(hipMemcpyAsync(raw, pixels[i], (size_t)h * w * channels, hipMemcpyHostToDevice, s));
            const Model::AxisDev ay = axis(h, S, FILTER_TRIANGLE), ax = axis(w, S, FILTER_TRIANGLE);          // resize_exact(S, S, Triangle)
            float* tv = reinterpret_cast<float*>(base + o_tv[i]);
            BRN_HIP(launch_resample_v_u8(raw, h, w, channels, S, ay.left, ay.count, ay.w, ay.max_taps, tv, s));
            BRN_HIP(launch_resample_h(tv, S, w, channels, S, ax.left, ax.count, ax.w, ax.max_taps, nullptr, x + (size_t)i * 3 * S * S, mean, stdv, s));
        }
        run_model(&m, x, n, S, S, BRN_MEM_DEVICE, prob, BRN_MEM_DEVICE, stream, 1);                           // forward(): sigmoid fused (birefnet.rs:466-469)
        unsigned char* m8 = reinterpret_cast<unsigned char*>(base + o_m8);
        BRN_HIP(launch_mask_u8(prob, (long)n * S * S, 0, m8, s));                                              // infer_image.rs:84-99
        for (int i = 0; i < n; ++i) {
            const int h = heights[i], w = widths[i];
            const Model::AxisDev ay = axis(S, h, FILTER_LANCZOS3), ax = axis(S, w, FILTER_LANCZOS3);          // :103-108
            float* pv = reinterpret_cast<float*>(base + o_pv[i]);
            unsigned char* dout = reinterpret_cast<unsigned char*>(base + o_out[i]);
            BRN_HIP(launch_resample_v_u8(m8 + (size_t)i * S * S, S, S, 1, h, ay.left, ay.count, ay.w, ay.max_taps, pv, s));
            BRN_HIP(launch_resample_h(pv, h, S, 1, w, ax.left, ax.count, ax.w, ax.max_taps, dout, nullptr, nullptr, nullptr, s));
            BRN_HIP(hipMemcpyAsync(masks[i], dout, (size_t)h * w, hipMemcpyDeviceToHost, s));
        }
        BRN_HIP(hipStreamSynchronize(s));
    });
}

}  // extern "C"
