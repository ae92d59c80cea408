// brn_api.cpp — the model behind the extern "C" boundary (include/birefnet_hip.h): handle and lifecycle, workspace planning, the
// forward and its profiling, the Swin / squeeze / decoder sub-forwards.  Image pre- and post-processing: brn_image.cpp; the op-level
// entry points: brn_ops.cpp.
#include "brn_api_util.h"
#include <cstring>
#include <cstdio>
#include <memory>
#include <cstdlib>

namespace brn {

// The one table from brn_dtype to arithmetic.  brn_model_create, brn_decoder_create and brn_set_op_compute start from it and state
// their differences themselves.
ComputeMode compute_mode(int dt) {
    ComputeMode m;
    if (dt == BRN_F32) m.build.planes = 0;
    else if (dt == BRN_F32_SPLIT3) m.build.planes = 3;
    else if (dt == BRN_F32_SPLIT2) m.build.planes = 2;
    else if (dt == BRN_F32_HALF2) m.build.planes = BUILD_HALF2;
#ifdef BRN_DIAG_BUILD
    else if (dt == BRN_BF16_OPERANDS) m.build.planes = 1;
#else
    else if (dt == BRN_BF16_OPERANDS) fail(BRN_ERR_INVALID_ARG, "compute dtype BRN_BF16_OPERANDS is superseded by BRN_BF16 and only built into libbirefnet_hip_diag.so");
#endif
    else if (dt == BRN_BF16 || dt == BRN_BF16_DEC_SPLIT2 || dt == BRN_F16) { m.build = {BUILD_BF16, dt == BRN_F16}; m.s16 = dt == BRN_F16 ? 2 : 1; }
    else fail(BRN_ERR_INVALID_ARG, "unsupported compute dtype %d", dt);
    return m;
}

// Size the workspace for a (B, H, W) request: a dry run of the forward with a counting arena.  Every request shape is planned
// on its own and the workspace only grows to the largest need seen (batch 16 at 512^2 followed by batch 1 at 2080^2 must not
// reserve batch 16 at 2080^2); a request that is <= a planned shape in every dimension fits without a new dry run.
static void plan_model(Model& m, int B, int H, int W) {
    if (m.arena.base)
        for (const Model::Planned& q : m.planned)
            if (B <= q.B && H <= q.H && W <= q.W) return;
    Arena dry;
    dry.dry = true;
    Ctx c{&dry, nullptr, true, false, nullptr, nullptr, nullptr};
    c.bf16 = m.bf16;
    model_forward(m, c, nullptr, B, H, W, nullptr, 0);
    size_t need = dry.peak + 4096;
    // staging for host-resident input / output of the full model
    need += ((size_t)B * 3 * H * W + (size_t)B * H * W) * sizeof(float) + 1024;
    if (!m.arena.base || need > m.arena.cap) {
        if (m.arena.base) { BRN_HIP(hipDeviceSynchronize()); (void)hipFree(m.arena.base); m.arena.base = nullptr; m.arena.cap = 0; m.planned.clear(); }
        void* d = nullptr;
        hipError_t e = hipMalloc(&d, need);
        if (e != hipSuccess) {
            (void)hipGetLastError();          // (the failed allocation must not be reported again by the next launch check)
            fail(BRN_ERR_OOM, "workspace hipMalloc of %zu bytes (B=%d, %dx%d) failed: %s", need, B, H, W, hipGetErrorString(e));
        }
        m.arena.base = (char*)d; m.arena.cap = need; m.arena.top = 0; m.arena.peak = 0; m.arena.dry = false;
    }
    if (m.planned.size() >= 16) m.planned.erase(m.planned.begin());
    m.planned.push_back({B, H, W});
    if (B > m.plan_B) m.plan_B = B;
    if (H > m.plan_H) m.plan_H = H;
    if (W > m.plan_W) m.plan_W = W;
}

static void collect_profile(Model& m, hipStream_t s) {
    BRN_HIP(hipStreamSynchronize(s));
    for (int f = 0; f < FAM_COUNT + REGION_COUNT; ++f) { m.fam_launches[f] = 0; m.fam_ms[f] = 0.f; m.fam_flop[f] = 0.0; m.fam_bytes[f] = 0.0; }
    // BRN_DUMP_LAUNCHES=<path>: one CSV row per launch of the last profiled forward (tuning aid)
    const char* dump = getenv("BRN_DUMP_LAUNCHES");
    FILE* df = dump ? fopen(dump, "w") : nullptr;
    if (df) fprintf(df, "family,M,N,K,ms,gflop,tflops,gbytes,region\n");
    for (auto& r : m.records) {
        float ms = 0.f;
        if (hipEventElapsedTime(&ms, r.e0, r.e1) != hipSuccess) ms = 0.f;
        if (df) fprintf(df, "%s,%d,%d,%d,%.4f,%.3f,%.2f,%.4f,%d\n", brn_kernel_family_name(r.fam), r.M, r.N, r.K, ms, r.flop / 1e9, ms > 0 ? r.flop / ms / 1e9 : 0.0, r.bytes / 1e9, r.region);
        m.fam_launches[r.fam]++; m.fam_ms[r.fam] += ms; m.fam_flop[r.fam] += r.flop; m.fam_bytes[r.fam] += r.bytes;
        if (r.region > REGION_NONE && r.region < REGION_COUNT) {
            const int g = FAM_COUNT + r.region;
            m.fam_launches[g]++; m.fam_ms[g] += ms; m.fam_flop[g] += r.flop; m.fam_bytes[g] += r.bytes;
        }
    }
    if (df) fclose(df);
    if (m.stage_ev_ok) {
        for (int i = 0; i < 4; ++i) (void)hipEventElapsedTime(&m.last_ms[i], m.stage_ev[i], m.stage_ev[i + 1]);
        (void)hipEventElapsedTime(&m.last_ms[4], m.stage_ev[0], m.stage_ev[4]);
    }
}

static void validate_config(const brn_config& c) {
    const int bc[4] = {192, 384, 768, 1536};
    for (int i = 0; i < 4; ++i)
        if (c.backbone_channels[i] != bc[i] || c.backbone_channels[i] != (c.embed_dim << i))
            fail(BRN_ERR_INVALID_ARG, "backbone_channels/embed_dim must be the Swin-L plan [192,384,768,1536]: the decoder's ipt blocks "
                 "hard-wire it (birefnet.rs:189-193)");
    if (!c.mul_scl_ipt || c.n_cxt != 3 || c.cxt[0] != 192 || c.cxt[1] != 384 || c.cxt[2] != 768)
        fail(BRN_ERR_INVALID_ARG, "only mul_scl_ipt=true with cxt=[192,384,768] is supported (the reference decoder's channel plan "
             "is inconsistent otherwise, birefnet.rs:176-207)");
    if (c.deform_mode != BRN_DEFORM_REFERENCE_CPU && c.deform_mode != BRN_DEFORM_DEFORMABLE)
        fail(BRN_ERR_INVALID_ARG, "unknown deform_mode %d", c.deform_mode);
    for (int i = 0; i < 4; ++i)
        if (c.depths[i] < 1 || c.depths[i] > 64) fail(BRN_ERR_INVALID_ARG, "depths[%d]=%d out of range", i, c.depths[i]);
}

static void run_model_locked(Model* m, const float* x, int B, int H, int W, brn_mem in_loc, float* out, brn_mem out_loc, void* stream, int apply_sigmoid);

// sub-batches a device-resident batch of B images runs as (BRN_SPLIT_STREAMS, default 2; at least two images per part)
static int sub_batch_parts(int B, int override_parts = 0) {
    const int want = override_parts > 0 ? override_parts : switches().split_streams;     // brn_model_set_streams beats the environment
    int parts = want < 1 ? 1 : (want > 8 ? 8 : want);
    if (parts > B / 2) parts = B / 2;
    return parts < 1 ? 1 : parts;
}
// streams, events and workspaces of parts 1 .. parts-1, each workspace as large as the main one (which plan_model sized for the
// largest part).  false = a workspace could not be allocated (the caller then runs the batch as one part); nothing is left half-made
static bool ensure_side_arenas(Model& m, int parts) {
    if ((int)m.sides.size() < parts - 1) m.sides.resize(parts - 1);
    for (int k = 0; k < parts - 1; ++k) {
        Model::Side& sd = m.sides[k];
        if (!sd.stream) {
            BRN_HIP(hipStreamCreateWithFlags(&sd.stream, hipStreamNonBlocking));
            BRN_HIP(hipEventCreateWithFlags(&sd.join_ev, hipEventDisableTiming));
        }
        if (sd.arena.base && sd.arena.cap >= m.arena.cap) continue;
        if (sd.arena.base) { BRN_HIP(hipDeviceSynchronize()); (void)hipFree(sd.arena.base); sd.arena.base = nullptr; sd.arena.cap = 0; }
        void* d = nullptr;
        const char* fault = getenv("BRN_FAULT_SIDE_ARENA");       // test hook: behave as if this allocation had failed
        hipError_t e = (fault && atoi(fault) != 0) ? hipErrorOutOfMemory : hipMalloc(&d, m.arena.cap);
        if (e != hipSuccess) {
            (void)hipGetLastError();                               // (must not be reported by the next launch check)
            return false;
        }
        sd.arena.base = (char*)d; sd.arena.cap = m.arena.cap;
    }
    return true;
}

void run_model(Model* m, const float* x, int B, int H, int W, brn_mem in_loc, float* out, brn_mem out_loc, void* stream, int apply_sigmoid) {
    if (!m || !x || !out) fail(BRN_ERR_INVALID_ARG, "null argument");
    if (B < 1) fail(BRN_ERR_INVALID_ARG, "batch must be >= 1");
    if (m->decoder_only) fail(BRN_ERR_INVALID_ARG, "this handle holds only the decoder (brn_decoder_create): forward_logits needs a whole model");
    std::lock_guard<std::mutex> lk(m->mu);
    try {
        run_model_locked(m, x, B, H, W, in_loc, out, out_loc, stream, apply_sigmoid);
    } catch (...) {
        // a forward that failed half-way may have work in flight on its sub-batch / branch streams that no event of the next call
        // orders against: drain the device before the workspace can be handed out again
        (void)hipDeviceSynchronize();
        throw;
    }
}

static void run_model_locked(Model* m, const float* x, int B, int H, int W, brn_mem in_loc, float* out, brn_mem out_loc, void* stream,
                             int apply_sigmoid) {
    BRN_HIP(hipSetDevice(m->device));
    hipStream_t s = (hipStream_t)stream;
    // a device-resident batch runs as `parts` sub-batches, each on its own stream with its own workspace (below): what has to fit a
    // workspace is then the LARGEST PART, and that is the shape the dry run plans (its GEMM plans — tiles, split-K scratch — are those of
    // the part, not of the whole batch); every workspace, the main one included, is sized to that peak
    int parts = sub_batch_parts(B, m->opt_parts);
    bool split = parts > 1 && !m->profiling && in_loc == BRN_MEM_DEVICE && out_loc == BRN_MEM_DEVICE;
    plan_model(*m, split ? (B + parts - 1) / parts : B, H, W);
    if (split && !ensure_side_arenas(*m, parts)) {
        // no memory for a second workspace: the batch runs as one part on one stream (planned as such) instead of failing
        split = false; parts = 1;
        plan_model(*m, B, H, W);
    }
    if (!m->done_ev) BRN_HIP(hipEventCreateWithFlags(&m->done_ev, hipEventDisableTiming));
    if (m->has_last && m->last_stream != s) BRN_HIP(hipStreamWaitEvent(s, m->done_ev, 0));   // previous forward still owns the arena
    m->arena.top = 0;
    const size_t n_in = (size_t)B * 3 * H * W, n_out = (size_t)B * H * W;
    const float* dx = x;
    float* dout = out;
    if (in_loc == BRN_MEM_HOST) {
        float* t = m->arena.alloc(n_in);
        BRN_HIP(hipMemcpyAsync(t, x, n_in * sizeof(float), hipMemcpyHostToDevice, s));
        dx = t;
    }
    if (out_loc == BRN_MEM_HOST) dout = m->arena.alloc(n_out);
    m->records.clear(); m->event_next = 0;
    if (m->profiling && !m->stage_ev_ok) {
        for (int i = 0; i < 6; ++i) BRN_HIP(hipEventCreate(&m->stage_ev[i]));
        m->stage_ev_ok = true;
    }
    // A batch as `parts` sub-batches on `parts` streams (images are independent units): the kernels of one part fill the CUs another
    // part's launch leaves idle in its last, partial round of tiles, and the write bursts of one part's epilogues fall into the K
    // loops of the others (measured at batch 8, 1024^2, bf16: +5.6 % with 2 parts).  BRN_SPLIT_STREAMS = number of
    // parts (default 2; 1 = one stream).  Each part has its own workspace; the results do not depend on how the host interleaves the
    // enqueues (same kernels, same plans per part, no atomics).  Profiled forwards run on one stream (per-launch events).
    // Independent branches of one forward (ASPP branches, the image-patch convolutions) go to auxiliary streams (brn_graph.h: Branch);
    // BRN_BRANCH_STREAMS (brn_host.h): by default on when the batch runs as ONE part (measured: +1.4 % at batch 1, 1024^2; with two
    // sub-batch streams the extra concurrency costs 2.5 % at batch 8).
    const int branches_env = m->opt_branches > -2 ? m->opt_branches : switches().branch_streams;    // brn_model_set_streams beats the environment
    bool branches_on = branches_env != 0;
    auto branch_set = [&](int k) -> BranchSet* {
        if (!branches_on || m->profiling) return nullptr;
        if ((int)m->branch_sets.size() <= k) m->branch_sets.resize(k + 1);
        BranchSet& bs = m->branch_sets[k];
        for (int i = 0; i < BRN_AUX_STREAMS; ++i) {
            if (bs.stream[i]) continue;
            BRN_HIP(hipStreamCreateWithFlags(&bs.stream[i], hipStreamNonBlocking));
            BRN_HIP(hipEventCreateWithFlags(&bs.fork_ev[i], hipEventDisableTiming));
            BRN_HIP(hipEventCreateWithFlags(&bs.join_ev[i], hipEventDisableTiming));
        }
        return &bs;
    };
    if (split) {
        if (branches_env < 0) branches_on = false;
        if (!m->fork_ev) BRN_HIP(hipEventCreateWithFlags(&m->fork_ev, hipEventDisableTiming));
        for (int k = 0; k < parts - 1; ++k) {
            Model::Side& sd = m->sides[k];
            sd.arena.top = 0; sd.arena.peak = 0; sd.arena.dry = false;
        }
        // BRN_CU_PARTITION (A/B switch, two parts only): each part's stream is confined to its own half of the chip by a CU mask (mask bit
        // i = CU i / 8 of XCD i % 8; 1 shares every L2, 2 does not).  The persistent GEMM grids are sized for the CUs of the mask (set_launch_cus).
        const int cu_part = switches().cu_partition;
        const bool masked = cu_part > 0 && parts == 2;
        if (masked && !m->cu_stream[0]) {
            for (int k = 0; k < 2; ++k) {
                uint32_t mask[8] = {0, 0, 0, 0, 0, 0, 0, 0};
                for (int i = 0; i < 256; ++i) {
                    const bool mine = cu_part == 2 ? ((i % 8 < 4) == (k == 0)) : ((i < 128) == (k == 0));
                    if (mine) mask[i >> 5] |= 1u << (i & 31);
                }
                BRN_HIP(hipExtStreamCreateWithCUMask(&m->cu_stream[k], 8, mask));
                BRN_HIP(hipEventCreateWithFlags(&m->cu_join_ev[k], hipEventDisableTiming));
            }
        }
        struct CusGuard { bool on; explicit CusGuard(bool o) : on(o) { if (on) set_launch_cus(128); } ~CusGuard() { if (on) set_launch_cus(256); } } cus_guard(masked);
        BRN_HIP(hipEventRecord(m->fork_ev, s));
        int b0 = 0;
        for (int k = 0; k < parts; ++k) {
            const int bk = B / parts + (k < B % parts ? 1 : 0);
            hipStream_t sk = masked ? m->cu_stream[k] : (k == 0 ? s : m->sides[k - 1].stream);
            if (k > 0 || masked) BRN_HIP(hipStreamWaitEvent(sk, m->fork_ev, 0));
            Ctx ck{k == 0 ? &m->arena : &m->sides[k - 1].arena, sk, false, false, nullptr, nullptr, nullptr};
            ck.bf16 = m->bf16;
            ck.br = branch_set(k);
            if (branches_env > 0) ck.br_mask = (unsigned)branches_env;
            model_forward(*m, ck, dx + (size_t)b0 * 3 * H * W, bk, H, W, dout + (size_t)b0 * H * W, apply_sigmoid);
            if (masked) BRN_HIP(hipEventRecord(m->cu_join_ev[k], sk));
            else if (k > 0) BRN_HIP(hipEventRecord(m->sides[k - 1].join_ev, sk));
            b0 += bk;
        }
        if (masked) { for (int k = 0; k < 2; ++k) BRN_HIP(hipStreamWaitEvent(s, m->cu_join_ev[k], 0)); }
        else for (int k = 1; k < parts; ++k) BRN_HIP(hipStreamWaitEvent(s, m->sides[k - 1].join_ev, 0));
        BRN_HIP(hipEventRecord(m->done_ev, s));
        m->last_stream = s; m->has_last = true;
        return;
    }
    Ctx c{&m->arena, s, false, m->profiling, &m->records, &m->event_pool, &m->event_next};
    c.bf16 = m->bf16;
    c.br = branch_set(0);
    if (branches_env > 0) c.br_mask = (unsigned)branches_env;
    model_forward(*m, c, dx, B, H, W, dout, apply_sigmoid);
    if (out_loc == BRN_MEM_HOST) {
        BRN_HIP(hipMemcpyAsync(out, dout, n_out * sizeof(float), hipMemcpyDeviceToHost, s));
        BRN_HIP(hipStreamSynchronize(s));
    }
    BRN_HIP(hipEventRecord(m->done_ev, s));
    m->last_stream = s; m->has_last = true;
    if (m->profiling) collect_profile(*m, s);
}

// ---- SwinTransformer::forward behind brn_model_backbone_forward and brn_swin_forward -------------------------------------------
static void swin_outputs_nchw(Ctx& c, const SwinW& w, const float* dx, int B, int H, int W, float* const douts[4]) {
    int hs[4], ws[4];
    swin_stage_dims(H, W, w.patch, hs, ws);
    Map hm[4];
    for (int i = 0; i < 4; ++i) hm[i] = new_map(c, B, hs[i], ws[i], w.embed_dim << i);
    const SwinIn in{dx, H, W, hm};
    swin_forward_multi(c, w, &in, 1, B);
    if (!c.dry)
        for (int i = 0; i < 4; ++i)     // NHWC -> NCHW: the permute(0,3,1,2) of swin.rs:786-788
            BRN_HIP(launch_nhwc_to_nchw(hm[i].p, B, hm[i].C, hs[i], ws[i], hm[i].ld, 0, douts[i], c.stream, c.bf16));
}

void swin_entry(const SwinW& w, int device, const float* x, int B, int H, int W, brn_mem in_loc, float* const outs[4], brn_mem out_loc,
                void* stream, int bf16) {
    if (!x || !outs) fail(BRN_ERR_INVALID_ARG, "null argument");
    if (B < 1 || H < 1 || W < 1) fail(BRN_ERR_INVALID_ARG, "bad input shape");
    BRN_HIP(hipSetDevice(device));
    Staging si(stream, in_loc), so(stream, out_loc);
    const float* dx = si.in(x, (size_t)B * 3 * H * W);
    int hs[4], ws[4];
    swin_stage_dims(H, W, w.patch, hs, ws);
    float* douts[4];
    for (int i = 0; i < 4; ++i) douts[i] = so.out(outs[i], (size_t)B * (w.embed_dim << i) * hs[i] * ws[i]);
    with_arena((hipStream_t)stream, [&](Ctx& c) { swin_outputs_nchw(c, w, dx, B, H, W, douts); }, bf16);
    so.finish();
}

}  // namespace brn

using namespace brn;

extern "C" {

int brn_abi_version(void) { return BRN_ABI_VERSION; }
const char* brn_last_error(void) { return last_error_cstr(); }
const char* brn_build_info(void) {
#define BRN_STR2(x) #x
#define BRN_STR(x) BRN_STR2(x)
    return "libbirefnet_hip gfx950 (CDNA4): compute modes f32 (fp32 MFMA), f32_split3 / f32_split2 (split-bf16 MFMA, fp32 storage), f32_half2 (fp16-pair MFMA, fp32 storage), bf16 / f16 (bf16 / fp16 storage + MFMA); HIP " BRN_STR(HIP_VERSION_MAJOR) "." BRN_STR(HIP_VERSION_MINOR) "." BRN_STR(HIP_VERSION_PATCH);
}
brn_status brn_device_count(int* n) {
    return guarded([&] {
        if (!n) fail(BRN_ERR_INVALID_ARG, "null argument");
        int k = 0;
        hipError_t e = hipGetDeviceCount(&k);
        *n = (e == hipSuccess) ? k : 0;
    });
}

void brn_config_default_swin_l(brn_config* c) {
    if (!c) return;
    memset(c, 0, sizeof *c);
    c->size_w = 1024; c->size_h = 1024;                       // birefnet.rs:35
    strncpy(c->backbone, "swin_v1_l", sizeof c->backbone - 1);  // birefnet.rs:36
    const int bc[4] = {192, 384, 768, 1536};                   // birefnet.rs:38
    const int dp[4] = {2, 2, 18, 2}, nh[4] = {6, 12, 24, 48};  // swin.rs:72-73
    for (int i = 0; i < 4; ++i) { c->backbone_channels[i] = bc[i]; c->depths[i] = dp[i]; c->num_heads[i] = nh[i]; }
    c->mul_scl_ipt = 1; c->ms_supervision = 1; c->dec_ipt = 1; c->use_aspp_deformable = 1;   // birefnet.rs:39-42
    c->cxt[0] = 192; c->cxt[1] = 384; c->cxt[2] = 768; c->n_cxt = 3;                          // birefnet.rs:43
    c->embed_dim = 192; c->window_size = 12; c->mlp_ratio = 4.0f; c->patch_size = 4; c->in_channels = 3;
    c->drop_path_rate = 0.2f;                                  // swin.rs:71-78
    c->deform_mode = BRN_DEFORM_REFERENCE_CPU;
}
void brn_config_lateral_channels(const brn_config* c, int out[4]) {
    const int mult = c->mul_scl_ipt ? 2 : 1;                   // birefnet.rs:51
    for (int i = 0; i < 4; ++i) out[i] = c->backbone_channels[i] * mult;
}
int brn_config_x4_channels(const brn_config* c) {
    const int mult = c->mul_scl_ipt ? 2 : 1;                   // birefnet.rs:57-60
    int s = c->backbone_channels[3] * mult;
    for (int i = 0; i < c->n_cxt; ++i) s += c->cxt[i] * mult;
    return s;
}

brn_status brn_model_create(const brn_config* cfg, const brn_named_tensor* weights, size_t n, int device, brn_dtype dt,
                            int max_batch, int max_h, int max_w, brn_model** out) {
    return guarded([&] {
        if (!cfg || !weights || !out) fail(BRN_ERR_INVALID_ARG, "null argument");
        const ComputeMode mode = compute_mode(dt);
        // the mixed mode: squeeze + decoder weights as two bf16 planes (mode f32_split2) on fp32 maps behind the bf16 backbone
        const bool mixed = dt == BRN_BF16_DEC_SPLIT2;
        const WeightBuild dec_build = mixed ? WeightBuild{2, false} : mode.build;
        *out = nullptr;
        ensure_device(device);
        validate_config(*cfg);
        std::unique_ptr<brn_model> h(new brn_model());
        Model& m = h->m;
        m.cfg = *cfg; m.device = device; m.bf16 = mode.s16; m.dec_bf16 = mixed ? 0 : mode.s16;
        WeightTable wt(weights, n);
        build_swin_weights(wt, "bb.", *cfg, m.own, mode.build, m.swin);                   // birefnet.rs:393
        int lat[4];
        brn_config_lateral_channels(cfg, lat);
        build_decblk_weights(wt, "squeeze_module.0.", brn_config_x4_channels(cfg), lat[3], cfg->deform_mode, m.own, dec_build, m.squeeze);   // birefnet.rs:397-399
        build_decoder_weights(wt, "decoder.", *cfg, m.own, dec_build, m.dec);             // birefnet.rs:401
        m.has_decoder = true;
        // (the batch the caller announces will run as sub_batch_parts(max_batch) parts when it is device-resident: plan the part;
        // a host-resident or profiled call of that batch re-plans for the whole batch when it comes)
        if (max_batch > 0 && max_h > 0 && max_w > 0) { const int pp = sub_batch_parts(max_batch, m.opt_parts); plan_model(m, (max_batch + pp - 1) / pp, max_h, max_w); }
        *out = h.release();
    });
}
brn_status brn_decoder_create(const brn_config* cfg, const brn_named_tensor* weights, size_t n, const char* prefix, int device, brn_dtype dt,
                              brn_model** out) {
    return guarded([&] {
        if (!cfg || !weights || !out) fail(BRN_ERR_INVALID_ARG, "null argument");
        if (dt == BRN_BF16_OPERANDS) fail(BRN_ERR_INVALID_ARG, "unsupported compute dtype %d", (int)dt);
        ComputeMode mode = compute_mode(dt);
        if (dt == BRN_BF16_DEC_SPLIT2) mode = {{2, false}, 0};          // (a decoder on its own in the mixed mode = mode f32_split2)
        *out = nullptr;
        ensure_device(device);
        validate_config(*cfg);
        std::unique_ptr<brn_model> h(new brn_model());
        Model& m = h->m;
        m.cfg = *cfg; m.device = device; m.bf16 = mode.s16; m.dec_bf16 = m.bf16;
        WeightTable wt(weights, n);
        build_decoder_weights(wt, prefix ? prefix : "", *cfg, m.own, mode.build, m.dec);   // birefnet.rs:170-273
        m.has_decoder = true; m.decoder_only = true;
        *out = h.release();
    });
}
brn_status brn_model_create_from_safetensors(const brn_config* cfg, const char* path, const char* prefix, int device, brn_dtype dt,
                                            int max_batch, int max_h, int max_w, brn_model** out) {
    brn_status st = guarded([&] {
        if (!cfg || !path || !out) fail(BRN_ERR_INVALID_ARG, "null argument");
        *out = nullptr;
    });
    if (st != BRN_OK) return st;
    SafetensorsFile f;
    std::vector<brn_named_tensor> named;
    st = guarded([&] { f.open(path); named = f.named(prefix); if (named.empty()) fail(BRN_ERR_MISSING_TENSOR, "no tensor under prefix '%s' in '%s'", prefix ? prefix : "", path); });
    if (st != BRN_OK) return st;
    return brn_model_create(cfg, named.data(), named.size(), device, dt, max_batch, max_h, max_w, out);   // copies; the mapping goes with f
}
void brn_model_destroy(brn_model* m) {
    if (!m) return;
    (void)hipSetDevice(m->m.device);
    (void)hipDeviceSynchronize();
    delete m;
}

brn_status brn_forward_logits(brn_model* m, const float* x, int B, int H, int W, brn_mem in_loc, float* out, brn_mem out_loc,
                              void* stream) {
    return guarded([&] { run_model(m ? &m->m : nullptr, x, B, H, W, in_loc, out, out_loc, stream, 0); });
}
brn_status brn_forward(brn_model* m, const float* x, int B, int H, int W, brn_mem in_loc, float* out, brn_mem out_loc,
                       void* stream) {
    return guarded([&] { run_model(m ? &m->m : nullptr, x, B, H, W, in_loc, out, out_loc, stream, 1); });
}

brn_status brn_model_set_streams(brn_model* m, int sub_batch_streams, int branch_stream_mask) {
    return guarded([&] {
        if (!m) fail(BRN_ERR_INVALID_ARG, "null model");
        if (sub_batch_streams < 0 || sub_batch_streams > 8 || branch_stream_mask < -1 || branch_stream_mask > 31)
            fail(BRN_ERR_INVALID_ARG, "sub_batch_streams in 0 .. 8 (0 = default), branch_stream_mask in -1 .. 31 (-1 = automatic)");
        std::lock_guard<std::mutex> lk(m->m.mu);
        m->m.opt_parts = sub_batch_streams;
        m->m.opt_branches = branch_stream_mask;
    });
}
brn_status brn_model_set_profiling(brn_model* m, int enable) {
    return guarded([&] {
        if (!m) fail(BRN_ERR_INVALID_ARG, "null model");
        std::lock_guard<std::mutex> lk(m->m.mu);
        m->m.profiling = enable != 0;
    });
}
brn_status brn_model_last_timings(brn_model* m, float ms[5]) {
    return guarded([&] {
        if (!m || !ms) fail(BRN_ERR_INVALID_ARG, "null argument");
        for (int i = 0; i < 5; ++i) ms[i] = m->m.last_ms[i];
    });
}
brn_status brn_model_last_kernel_stats(brn_model* m, int n, int* launches, float* ms, double* flop, double* bytes, int* n_out) {
    return guarded([&] {
        if (!m || !launches || !ms || !flop || !bytes) fail(BRN_ERR_INVALID_ARG, "null argument");
        const int rows = FAM_COUNT + REGION_COUNT;      // families, then regions (row FAM_COUNT + REGION_NONE stays zero)
        const int k = n < rows ? n : rows;
        for (int f = 0; f < k; ++f) {
            launches[f] = m->m.fam_launches[f]; ms[f] = m->m.fam_ms[f]; flop[f] = m->m.fam_flop[f]; bytes[f] = m->m.fam_bytes[f];
        }
        if (n_out) *n_out = rows;
    });
}
const char* brn_kernel_family_name(int f) {
    static const char* names[FAM_COUNT] = {"gemm_dense", "gemm_conv_nhwc", "gemm_gather_nchw", "gemm_deform_nhwc",
                                           "window_attention", "layernorm", "resize", "elementwise"};
    static const char* regions[REGION_COUNT] = {"region_none", "region_aspp"};
    if (f >= FAM_COUNT && f < FAM_COUNT + REGION_COUNT) return regions[f - FAM_COUNT];
    return (f >= 0 && f < FAM_COUNT) ? names[f] : "?";
}

// ---- pieces of the model used individually by bench_inference.rs -------------------------------------------------------
brn_status brn_model_backbone_forward(brn_model* m, const float* x, int B, int H, int W, brn_mem in_loc, float* const outs[4],
                                      brn_mem out_loc, void* stream) {
    return guarded([&] {
        if (!m) fail(BRN_ERR_INVALID_ARG, "null model");
        if (m->m.decoder_only) fail(BRN_ERR_INVALID_ARG, "this handle holds only the decoder (brn_decoder_create)");
        std::lock_guard<std::mutex> lk(m->m.mu);
        swin_entry(m->m.swin, m->m.device, x, B, H, W, in_loc, outs, out_loc, stream, m->m.bf16);
    });
}

brn_status brn_model_squeeze_forward(brn_model* m, const float* x4, int B, int h, int w, brn_mem in_loc, float* out,
                                     brn_mem out_loc, void* stream) {
    return guarded([&] {
        if (!m || !x4 || !out) fail(BRN_ERR_INVALID_ARG, "null argument");
        if (m->m.decoder_only) fail(BRN_ERR_INVALID_ARG, "this handle holds only the decoder (brn_decoder_create)");
        std::lock_guard<std::mutex> lk(m->m.mu);
        BRN_HIP(hipSetDevice(m->m.device));
        const int cin = m->m.squeeze.cin, cout = m->m.squeeze.cout;
        Staging si(stream, in_loc), so(stream, out_loc);
        const float* dx = si.in(x4, (size_t)B * cin * h * w);
        float* dy = so.out(out, (size_t)B * cout * h * w);
        with_arena((hipStream_t)stream, [&](Ctx& c) {
            Map X = new_map(c, B, h, w, cin), Y = new_map(c, B, h, w, cout);
            if (!c.dry) BRN_HIP(launch_nchw_to_nhwc(dx, B, cin, h, w, X.p, X.ld, 0, c.stream, c.bf16));
            decblk_forward(c, m->m.squeeze, X, Y, m->m.cfg.deform_mode);
            if (!c.dry) BRN_HIP(launch_nhwc_to_nchw(Y.p, B, cout, h, w, Y.ld, 0, dy, c.stream, c.bf16));
        }, m->m.dec_bf16);
        so.finish();
    });
}

brn_status brn_model_decoder_forward(brn_model* m, const float* x, const float* x1, const float* x2, const float* x3,
                                     const float* x4, int B, int H, int W, brn_mem in_loc, float* out, brn_mem out_loc,
                                     void* stream) {
    return guarded([&] {
        if (!m || !x || !x1 || !x2 || !x3 || !x4 || !out) fail(BRN_ERR_INVALID_ARG, "null argument");
        if (H % 32 || W % 32 || H < 32 || W < 32) fail(BRN_ERR_INVALID_ARG, "H and W must be positive multiples of 32");
        std::lock_guard<std::mutex> lk(m->m.mu);
        BRN_HIP(hipSetDevice(m->m.device));
        Staging si(stream, in_loc), so(stream, out_loc);
        const int hh[4] = {H / 4, H / 8, H / 16, H / 32}, ww[4] = {W / 4, W / 8, W / 16, W / 32};
        const int ch[4] = {384, 768, 1536, 3072};
        const float* src[4] = {x1, x2, x3, x4};
        const float* dsrc[4];
        for (int i = 0; i < 4; ++i) dsrc[i] = si.in(src[i], (size_t)B * ch[i] * hh[i] * ww[i]);
        const float* dx = si.in(x, (size_t)B * 3 * H * W);
        float* dy = so.out(out, (size_t)B * H * W);
        with_arena((hipStream_t)stream, [&](Ctx& c) {
            Map X1 = new_map(c, B, hh[0], ww[0], 384), X2 = new_map(c, B, hh[1], ww[1], 768), X3 = new_map(c, B, hh[2], ww[2], 1536);
            Map D4 = new_map(c, B, hh[3], ww[3], 3456);
            if (!c.dry) {
                BRN_HIP(launch_nchw_to_nhwc(dsrc[0], B, 384, hh[0], ww[0], X1.p, X1.ld, 0, c.stream, c.bf16));
                BRN_HIP(launch_nchw_to_nhwc(dsrc[1], B, 768, hh[1], ww[1], X2.p, X2.ld, 0, c.stream, c.bf16));
                BRN_HIP(launch_nchw_to_nhwc(dsrc[2], B, 1536, hh[2], ww[2], X3.p, X3.ld, 0, c.stream, c.bf16));
                BRN_HIP(launch_nchw_to_nhwc(dsrc[3], B, 3072, hh[3], ww[3], D4.p, D4.ld, 0, c.stream, c.bf16));
            }
            decoder_forward(c, m->m, dx, B, H, W, X1, X2, X3, D4, dy, 0);
        }, m->m.dec_bf16);
        so.finish();
    });
}

}  // extern "C"
