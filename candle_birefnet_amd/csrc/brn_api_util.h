// brn_api_util.h — what the files behind the extern "C" boundary share (brn_api.cpp, brn_image.cpp, brn_ops.cpp): the exception
// barrier, per-call staging of caller buffers, a private arena for one graph fragment, the compute-mode table, the handles.
#pragma once
#include "brn_host.h"
#include <functional>

namespace brn {
const char* last_error_cstr();

// Exceptions stop here; every entry returns a status and leaves a thread-local message for brn_last_error().
template <class F>
static brn_status guarded(F&& f) {
    try {
        (void)hipGetLastError();              // an error another library (or an earlier failed call) left in this thread is not ours to report
        f();
        return BRN_OK;
    } catch (const Error& e) {
        set_last_error(e.what());
        return e.code;
    } catch (const std::bad_alloc&) {
        set_last_error("host allocation failed");
        return BRN_ERR_OOM;
    } catch (const std::exception& e) {
        set_last_error(e.what());
        return BRN_ERR_INVALID_ARG;
    }
}

// per-call staging of caller buffers: BRN_MEM_HOST buffers travel through temporary HBM allocations
struct Staging {
    hipStream_t s; brn_mem loc;
    std::vector<void*> tmp;
    struct Out { float* host; float* dev; size_t n; };
    std::vector<Out> outs;
    Staging(void* stream, brn_mem l) : s((hipStream_t)stream), loc(l) {}
    float* dalloc(size_t n) {
        void* d = nullptr;
        hipError_t e = hipMalloc(&d, n * sizeof(float) + 16);
        if (e != hipSuccess) fail(BRN_ERR_OOM, "hipMalloc of %zu bytes failed: %s", n * sizeof(float), hipGetErrorString(e));
        tmp.push_back(d);
        return (float*)d;
    }
    const float* in(const float* p, size_t n) {
        if (!p) fail(BRN_ERR_INVALID_ARG, "null input pointer");
        if (loc == BRN_MEM_DEVICE) return p;
        float* d = dalloc(n);
        BRN_HIP(hipMemcpyAsync(d, p, n * sizeof(float), hipMemcpyHostToDevice, s));
        return d;
    }
    float* out(float* p, size_t n) {
        if (!p) fail(BRN_ERR_INVALID_ARG, "null output pointer");
        if (loc == BRN_MEM_DEVICE) return p;
        float* d = dalloc(n);
        outs.push_back({p, d, n});
        return d;
    }
    void finish() {
        for (auto& o : outs) BRN_HIP(hipMemcpyAsync(o.host, o.dev, o.n * sizeof(float), hipMemcpyDeviceToHost, s));
        if (loc == BRN_MEM_HOST) BRN_HIP(hipStreamSynchronize(s));
    }
    ~Staging() {
        if (!tmp.empty()) (void)hipStreamSynchronize(s);
        for (void* p : tmp) (void)hipFree(p);
    }
};

// argument checks the q/k/v attention entries share (brn_ops.cpp); each entry words its own message
// whether the na floats at a (null: none) and the ny floats at y share a byte
inline bool floats_overlap(const float* a, size_t na, const float* y, size_t ny) {
    const uintptr_t a0 = reinterpret_cast<uintptr_t>(a), y0 = reinterpret_cast<uintptr_t>(y);
    return a && a0 < y0 + ny * sizeof(float) && y0 < a0 + na * sizeof(float);
}
// the same in bytes, for buffers whose element size varies (a K / V pool of brn_kv_type)
inline bool bytes_overlap(const void* a, size_t na, const void* y, size_t ny) {
    const uintptr_t a0 = reinterpret_cast<uintptr_t>(a), y0 = reinterpret_cast<uintptr_t>(y);
    return a && y && a0 < y0 + ny && y0 < a0 + na;
}
// device buffers are read and written with 16-byte accesses (host buffers are staged into allocations of the library's own)
inline bool all_aligned16(std::initializer_list<const void*> ptrs) {
    for (const void* p : ptrs)
        if (reinterpret_cast<uintptr_t>(p) & 15) return false;
    return true;
}
// a softmax scale argument is finite and >= 0; 0 selects head_dim^-0.5
inline bool scale_arg_ok(float scale) { return scale >= 0.f && std::isfinite(scale); }
inline float scale_or_default(float scale, int head_dim) { return scale > 0.f ? scale : 1.0f / sqrtf((float)head_dim); }

// run a graph fragment with a private arena: plan (dry), allocate, run
inline void with_arena(hipStream_t s, const std::function<void(Ctx&)>& fn, int bf16 = 0) {   // bf16: 0 fp32 maps, 1 bf16, 2 fp16 (Ctx::bf16)
    Arena a;
    a.dry = true;
    Ctx c{&a, s, true, false, nullptr, nullptr, nullptr};
    c.bf16 = bf16;
    fn(c);
    Arena real;
    real.cap = a.peak + 256;
    void* d = nullptr;
    hipError_t e = hipMalloc(&d, real.cap);
    if (e != hipSuccess) fail(BRN_ERR_OOM, "workspace hipMalloc of %zu bytes failed: %s", real.cap, hipGetErrorString(e));
    real.base = (char*)d;
    Ctx c2{&real, s, false, false, nullptr, nullptr, nullptr};
    c2.bf16 = bf16;
    try {
        fn(c2);
        BRN_HIP(hipStreamSynchronize(s));
    } catch (...) {
        (void)hipStreamSynchronize(s);
        (void)hipFree(d);
        throw;
    }
    (void)hipFree(d);
}

// what a brn_dtype means to the weight builders and to the activation maps (brn_api.cpp).  BRN_BF16_DEC_SPLIT2 maps to its backbone's
// arithmetic (BRN_BF16); what it means for a decoder, and whether an entry accepts it at all, is the caller's line
struct ComputeMode {
    WeightBuild build;
    int s16 = 0;                   // map storage: 0 fp32, 1 bf16, 2 fp16 (Ctx::bf16)
};
ComputeMode compute_mode(int dt);

// brn_api.cpp, also behind brn_infer_images_u8 and brn_swin_forward
void run_model(Model* m, const float* x, int B, int H, int W, brn_mem in_loc, float* out, brn_mem out_loc, void* stream, int apply_sigmoid);
void swin_entry(const SwinW& w, int device, const float* x, int B, int H, int W, brn_mem in_loc, float* const outs[4], brn_mem out_loc,
                void* stream, int bf16 = 0);

// brn_deform_offsets.cpp, behind brn_deform_conv2d_offsets_forward (brn_ops.cpp) alone: the weight of the route the geometry selects, then
// the route between the channels-last map X [B, H, W, Cp] and Y [B, Ho, Wo, O] (both in the storage type s16) inside the entry's arena
struct DeformOffsetsPlan {
    DeformOffsetsParams geo;       // geometry and the device pointers of offset / mask (x, col, om: filled by the route)
    bool fused = false;            // route 1 (gather loaders) or route 2 (column matrix + dense GEMM)
    int Cp = 0, s16 = 0;           // channels of X (granule-padded); storage type of X and Y (Ctx::bf16)
    GemmW g;                       // fused: a GEMM_DEFORM_NHWC conv weight; columns: the dense [O][kh kw Cp] weight
};
bool deform_offsets_fused_eligible(const DeformOffsetsParams& a);
DeformOffsetsPlan deform_offsets_prepare(DeviceOwner& own, WeightBuild op, const DeformOffsetsParams& a, const float* w, const float* bias, int O);
void deform_offsets_route(Ctx& c, const DeformOffsetsPlan& pl, const Map& X, const Map& Y);
}  // namespace brn

struct brn_model { brn::Model m; };
