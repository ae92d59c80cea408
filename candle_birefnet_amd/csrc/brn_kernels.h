// brn_kernels.h — internal launch interface of the gfx950 kernels (not part of the C ABI).
// All activations are fp32, channels-last: a "map" is [B, H, W, ld] with the logical channels living in a
// column window [coff, coff+C) of the ld-wide rows, so concatenations are written in place (no cat copies).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace brn {

enum GemmMode {
    GEMM_DENSE = 0,       // A[m][k] = A + m*lda + k                         (Linear layers, 1x1 convs)
    GEMM_CONV_NHWC = 1,   // implicit im2col over a channels-last map, K = (ky,kx,ci), Cin % 32 == 0
    GEMM_GATHER_NCHW = 2, // implicit im2col over an NCHW image, K = (ci,ky,kx) (candle weight order), any Cin
    GEMM_DEFORM_NHWC = 3  // modulated deformable im2col (bilinear gather * mask), K = (ky,kx,ci), Cin % 32 == 0
};
enum Act { ACT_NONE = 0, ACT_RELU = 1, ACT_GELU_ERF = 2 };

struct GemmParams {
    const float* A;
    const float* W;       // [Npad][K] row-major, K contiguous, rows >= roundup(N, 128), K % 32 == 0, zero padded
    float* C;
    int M, N, K;
    int mode;
    int lda;              // dense: row stride; conv/deform: floats per pixel of the input map
    int a_coff;           // conv/deform: first channel of the input window
    // conv geometry (modes 1..3)
    int Hin, Win, Cin, kh, kw, stride, pad, dil, Hout, Wout;
    int Kreal;            // mode 2: Cin*kh*kw before padding to 32
    // deformable (mode 3): om = [B,Hout,Wout,om_ld] holding 2*kh*kw offsets (dy,dx interleaved, torchvision
    // order) then kh*kw modulator logits (already 2*sigmoid applied) starting at column om_mask_off
    const float* om; int om_ld; int om_mask_off;
    int om_sigmoid;       // deform_bf16 kernel only: the modulator columns hold raw logits, 2 * sigmoid (aspp.rs:173-174) is applied in the gather
    // epilogue:  v = acc (+ bias[n]) (+ bbias[m / bbias_rows][n]);  v = v*scale[n] + shift[n];  v = act(v);
    //            v += R[m*ldr + r_coff + n];  C[m*ldc + c_coff + n] = v
    const float* bias;
    const float* bbias; int bbias_rows;
    const float* scale; const float* shift;
    int act;
    const float* R; int ldr; int r_coff;
    int ldc; int c_coff;
    // split-bf16 path (planes = 0: fp32 MFMA path): Wp = W pre-split into `planes` bf16 planes [planes][wp_rows][K]
    const void* Wp; int planes; int wp_rows;
    // split-K (filled by launch_gemm from the plan): slices write raw partials to part[slice][M][N]
    int splitk; float* part;
    int a_planes, c_planes;   // 2: A is read / C is written in the P2 layout (kernels/split_planes.h); split-bf16 dense ws kernel only
    // mode f32_half2 (planes == 2 with fp16 planes, kernels/split_planes.h: split4h): Wp holds the fp16 planes of w_scale * W (a power of two per
    // tensor, GemmW::w_scale), A is split as the fp16 planes of a_scale * A while it is staged, and the accumulators are multiplied by
    // out_scale = 1 / (a_scale * w_scale) — exact — before the epilogue
    int h2; float a_scale, out_scale;
    // bf16-storage mode (kernels/gemm_bf16.hip): A, C, R are bf16 unless flagged; Wp is the plain [wp_rows][wp_ld] bf16 matrix
    int wp_ld;                // elements per W row (K rounded up to 64, zero padded)
    int k_chunk_major;        // bf16 implicit GEMM: W's K order is (64-channel chunk, tap, channel in chunk) instead of (tap, channel); Cin % 64 == 0
    int c_f32, r_f32;         // 1: C is written / R is read as fp32 (offset maps of the deformable mode, fp32 side outputs)
    int a_bf16, c_bf16;       // gemm_f32_kernel only (deformable gather in bf16 mode): A map read / C written as bf16
    unsigned long long* trace;   // diagnostics only: per-workgroup cycle stamps (gemm_split_ws_kernel), null in production
    int abl;   // diagnostics only (brn_gemm_microbench): 1 = no global loads in the K loop, 2 = no LDS staging, 4 = no fragment reads / MFMA
};

// cfg: 0 = 128x128, 1 = 128x64, 2 = 64x64 block tile.  raw = 1 (splitk > 1, fp32 C, no c_planes / c_bf16): launch_gemm leaves the raw slices
// part[s][M][N] in ws and launches no splitk_reduce_kernel — the consumer sums them (LayerNormParams::part)
struct GemmPlan { int cfg; int splitk; size_t ws_floats; int raw = 0; };
GemmPlan plan_gemm(int M, int N, int K, int planes = 0);   // planes: bf16 planes of the split modes (0 = fp32 kernels)
// the plan of a split-mode dense GEMM whose slices a LayerNorm sums (raw = 1), or splitk = 1: the pair does not beat GEMM + LayerNorm here
GemmPlan plan_gemm_ln(int M, int N, int K, int planes);
// ws: plan.ws_floats floats of scratch when plan.splitk > 1.  Returns the hipError_t of the launch(es).
hipError_t launch_gemm(const GemmParams& p, const GemmPlan& plan, float* ws, hipStream_t s);
// the split-bf16 path of launch_gemm (kernels/gemm_split.hip; p as launch_gemm validated it): dispatch over p.planes and the plan's tile.
// Plan configs 0 and 3..6 run on the warp-specialised 128x128 kernel, 1 and 2 on the 4-wave 128x64 / 64x64 tiles.
inline bool gemm_split_is_ws(int cfg) { return cfg == 6 || cfg == 0 || cfg == 3 || cfg == 4 || cfg == 5; }
hipError_t launch_gemm_split(const GemmParams& p, int cfg, hipStream_t s);

// CUs the persistent grids (gemm_bf16_kernel, gemm_wstat_*) are sized for on the calling host thread: 256 unless the launch stream carries a CU mask
int launch_cus();
void set_launch_cus(int n);
// bf16-storage mode: plan + launch (kernels/gemm_bf16.hip).  cfg: 0 = 128x128, 1 = 128x64, 2 = 256x256, 3 = 256x192 block tile
GemmPlan plan_gemm_bf16(int M, int N, int K, bool f32_residual = false, bool gelu = false);   // f32_residual: fp32 C with an fp32 residual (proj / fc2)
hipError_t launch_gemm_bf16(const GemmParams& p, const GemmPlan& plan, float* ws, hipStream_t s);

// bf16-storage mode, short-K dense GEMM with the weights resident in registers (kernels/rows_bf16.hip, gemm_wstat_bf16_kernel): Wp = the weights in
// MFMA fragment order (GemmW::wf, attach_dense_frags), K = 192 (64-row A tiles) or 384 (32-row tiles), N % 192 == 0, bf16 out, bias + activation only
bool gemm_wstat_eligible(const GemmParams& p);
hipError_t launch_gemm_wstat(const GemmParams& p, hipStream_t s);
// the same with N = K = 192, fp32 C + fp32 residual (in place or not) AND y = LayerNorm(C) gamma + beta written as a bf16 matrix
// (gemm_wstat_ln_bf16_kernel: the attention projection of a C = 192 stage with the block's norm2 in its epilogue)
// PatchEmbed for the Swin-L geometry as one kernel (kernels/patch_embed.hip): 4 x 4 stride-4 conv of the NCHW image (3 -> 192) + bias +
// LayerNorm, fp32, written into the residual stream x [B * H/4 * W/4][ldx]
bool patch_embed_ln_eligible(int Cin, int N, int k, int stride, int H, int W, int ldw, int ldx);
hipError_t launch_patch_embed_ln(const float* img, int B, int H, int W, const float* wgt, int ldw, const float* bias, const float* gamma,
                                 const float* beta, float eps, float* x, int ldx, hipStream_t s, const float* gamma1 = nullptr,
                                 const float* beta1 = nullptr, void* xn_bf16 = nullptr, int ldxn = 0, int xn_f16 = 0);   // (gamma1 / beta1 / xn: also LayerNorm(x) gamma1 + beta1 as a bf16 matrix)
bool gemm_wstat_ln_eligible(const GemmParams& p);
// the same fusion for N = 768 / 384 (any K % 32 == 0): gemm_rowln_bf16_kernel, a workgroup owns 64 whole rows, Wp = the plain [wp_rows][wp_ld] bf16 matrix
bool gemm_rowln_eligible(const GemmParams& p);
hipError_t launch_gemm_rowln(const GemmParams& p, const float* gamma, const float* beta, float eps, void* y_bf16, int ldy, hipStream_t s);
hipError_t launch_gemm_wstat_ln(const GemmParams& p, const float* gamma, const float* beta, float eps, void* y_bf16, int ldy, hipStream_t s);

// bf16-storage mode, modulated deformable conv (kernels/deform_bf16.hip): A = bf16 channels-last map, om = fp32 offsets | modulator,
// Wp = the weights in MFMA fragment order (GemmW::wf), C = bf16 window.  eligible(): shapes the kernel covers (else gemm_f32_kernel)
bool deform_bf16_eligible(const GemmParams& p);
hipError_t launch_deform_bf16(const GemmParams& p, hipStream_t s);

// split modes with A already in the P layout (kernels/gemm_planes.hip): LDS-DMA staged, persistent, no splitting wave
bool gemm_planes_eligible(const GemmParams& p);
GemmPlan plan_gemm_planes(int M, int N, int K, int planes, bool c_planes);
hipError_t launch_gemm_planes(const GemmParams& p, const GemmPlan& plan, float* ws, hipStream_t s);

// compute mode BRN_F16: the same kernels with fp16 as the 16-bit storage / MFMA operand type (kernels/gemm_bf16.hip, kernels/rows_bf16.hip and
// kernels/deform_bf16.hip compiled with -DBRN_S16_F16=1: kernels/s16_common.h).  Same contracts as the functions of the same name above.
namespace hf {
GemmPlan plan_gemm_bf16(int M, int N, int K, bool f32_residual = false, bool gelu = false);
hipError_t launch_gemm_bf16(const GemmParams& p, const GemmPlan& plan, float* ws, hipStream_t s);
bool gemm_wstat_eligible(const GemmParams& p);
hipError_t launch_gemm_wstat(const GemmParams& p, hipStream_t s);
bool gemm_wstat_ln_eligible(const GemmParams& p);
hipError_t launch_gemm_wstat_ln(const GemmParams& p, const float* gamma, const float* beta, float eps, void* y_bf16, int ldy, hipStream_t s);
bool gemm_rowln_eligible(const GemmParams& p);
hipError_t launch_gemm_rowln(const GemmParams& p, const float* gamma, const float* beta, float eps, void* y_bf16, int ldy, hipStream_t s);
bool deform_bf16_eligible(const GemmParams& p);
hipError_t launch_deform_bf16(const GemmParams& p, hipStream_t s);
}  // namespace hf

#ifdef BRN_DIAG_BUILD
hipError_t launch_mfma_valu_probe(int blocks, int iters, int mode, float* sink, hipStream_t s);
hipError_t launch_lds_mfma_probe(int blocks, int iters, int np, int variant, float* sink, hipStream_t s);
hipError_t launch_mfma_peak_bf16(int blocks, int iters, float* sink, unsigned long long* clk, int nacc, hipStream_t s);
hipError_t launch_mfma_peak(int blocks, int iters, float* sink, unsigned long long* clk, hipStream_t s);
#endif

struct LayerNormParams {
    const float* x; float* y;
    int rows, C;
    const float* gamma; const float* beta; float eps;
    int ldx;              // input row stride (mode 0)
    int ldy, y_coff;      // output row stride / column offset
    // mode 1: PatchMerging gather (swin.rs:505-522): row (b,i,j) of the merged map gathers the four tokens
    // (2i,2j),(2i+1,2j),(2i,2j+1),(2i+1,2j+1) of x [B,H,W,Cin], zero outside (odd H/W padding), C == 4*Cin
    int mode; int H, W, Cin;
    int y_planes;         // 2: write y in the P2 layout (kernels/split_planes.h) for a split-bf16 GEMM; 0: fp32
    float y_h2;           // > 0 (with y_planes == 2): the planes are the fp16 planes of y_h2 * y (mode f32_half2)
    int y_bf16;           // 1: y is a bf16 matrix (compute mode BRN_BF16; x stays fp32: the residual stream)
    // row source "sum of slices" (part != null; mode 0, x unused): the GEMM in front left its raw split-K slices part[s][rows][C]
    // (GemmPlan::raw) and the row is v = 0; v += part[0] .. part[slices - 1]; v += bias; v += R[row][r_coff ..] — splitk_reduce_kernel's
    // operand order — stored to x_out[row][xo_coff ..] (may alias R) and normalised from registers.  bias and R may each be null
    const float* part; int slices;
    const float* bias;
    const float* R; int ldr, r_coff;
    float* x_out; int ldxo, xo_coff;
};
hipError_t launch_layernorm(const LayerNormParams& p, hipStream_t s);

struct WindowAttnParams {
    const float* qkv;     // [B, H, W, 3C] natural token order (q | k | v, heads-major inside each, swin.rs:218)
    const float* qkv_bias;// [3C]  (q/k/v of a zero pad token)
    const float* rel_table;// relative_position_bias_table (swin.rs:138-141) transposed to [heads][(2*12-1)^2]; cached_bias (swin.rs:147-152) is never built
    float* out;           // [B, H, W, C]
    int B, H, W, C, heads;
    int Hp, Wp;           // padded canvas (multiples of 12)
    int shift;            // 0 or 6
    float scale;          // head_dim^-0.5
    int planes;           // 0: fp32 MFMA kernel (modes f32, f32_split3); 2 / 1: bf16-split kernel (f32_split2 / bf16_operands)
    int out_planes;       // 2: write `out` in the P2 layout (kernels/split_planes.h) for the proj GEMM; 0: fp32
    int h2;               // 1 (with planes == 2): the split kernel on fp16 planes (mode f32_half2)
    float out_h2;         // > 0 (with out_planes == 2, planes == 0 or h2): fp16 planes of out_h2 * out (mode f32_half2, written by the fp32-MFMA kernel)
    int ws;               // window side: 12 (0 = 12) or 7 (Swin-T / S: fp32 kernel only)
    int io_bf16;          // 1: qkv and out are bf16 matrices (compute mode BRN_BF16; qkv_bias / rel_table stay fp32)
    int pack_q;           // split / bf16 kernels at window 12 (BRN_ATT_PACK_Q): 1 = real queries only, windows with the most query tiles first;
                          // 2 = real queries only, grid order; 0 = all 144 positions of every window (kernels/window_geometry.h)
};
hipError_t launch_window_attention(const WindowAttnParams& p, hipStream_t s);
// two maps of the same stage in one launch (p2 may be null)
hipError_t launch_window_attention2(const WindowAttnParams& p, const WindowAttnParams* p2, hipStream_t s);

// q/k/v attention with an additive bias (kernels/attention_bias.hip; brn_attention_forward):
// y[b,h] = softmax_rows(scale * (q[b,h] k[b,h]^T + bias[b % n_bias, h])) v[b,h], head_dim 32, 1 <= N <= 144
struct AttentionBiasParams {
    const float* q; const float* k; const float* v;   // [batch, heads, N, 32], 16-byte aligned
    const float* bias;    // [n_bias, heads, N, N] or null (n_bias 0); added to the UNSCALED scores
    float* y;             // [batch, heads, N, 32]
    int batch, heads, N, n_bias;
    float scale;          // > 0 (the entry replaces 0 by head_dim^-0.5)
    int s16;              // 0: fp32 MFMA kernel; 1 / 2: q, k, v and the probabilities rounded to bf16 / fp16 on the 16-bit matrix instructions
};
hipError_t launch_attention_bias(const AttentionBiasParams& p, hipStream_t s);

// q/k/v attention for long sequences, online softmax over K / V tiles (kernels/flash_attention.hip; brn_flash_attention_forward and, with
// a bias, brn_flash_attention_bias_forward; with grouped K / V heads or a causal mask over a cache, brn_flash_attention_gqa_forward):
// y[b,h] = softmax_rows(scale * (q[b,h] k[b,h / G]^T [+ bias[b % n_bias, h]]) [causal: key j <= query i + causal_off]) v[b,h / G],
// G = heads / kv_heads, head_dim 32 / 64 / 128, 1 <= seq_q, seq_kv <= 65536; over a packed batch of sequences with a window mask,
// brn_flash_attention_varlen_forward (the fields after causal_off)
struct FaVarlenRecord;      // brn_flash_varlen_plan.h (host-only header)
struct FlashAttentionParams {
    const float* q; const float* k; const float* v;   // 16-byte aligned; head_dim contiguous
    float* y;             // q's shape and strides
    int batch, heads, seq_q, seq_kv, head_dim;
    long q_sb, q_sh, q_ss;       // element strides of q and y: batch entry, head, sequence position (multiples of head_dim)
    long kv_sb, kv_sh, kv_ss;    // element strides of k and v
    int causal;           // 1: key j takes part in query i's row exactly when j <= i (seq_q == seq_kv)
    float scale;          // > 0 (the entry replaces 0 by head_dim^-0.5)
    int s16;              // 0: fp32 MFMA kernel; 1 / 2: q, k, v and the softmax numerators rounded to bf16 / fp16 on the 16-bit matrix instructions
    // brn_flash_attention_bias_forward; all zero = no bias (the bias-free kernels)
    const float* bias;    // [n_bias, heads, seq_q, seq_kv] fp32, 16-byte aligned, added to the UNSCALED scores (-inf: the key is excluded); or null
    int n_bias;           // batch entry b reads pattern b % n_bias (batch % n_bias == 0); 0 exactly when bias is null
    long b_sp, b_sh;      // element strides of bias: pattern, head (heads-major whatever the layout of q / k / v)
    // brn_flash_attention_gqa_forward; kv_heads == heads and causal_off == 0 = the kernels of the two entries above, untouched
    int kv_heads;         // K / V heads (k, v strides are theirs): query head h reads K / V head h / (heads / kv_heads); heads % kv_heads == 0
    int causal_off;       // causal: seq_kv - seq_q >= 0, key j takes part in query i's row exactly when j <= i + causal_off; 0 when not causal
    // brn_flash_attention_varlen_forward; plan == null = the kernels of the three entries above, untouched.  With a plan: q, y
    // [total_q, heads, head_dim] and k, v [total_kv, kv_heads, head_dim] (batch 1, the strides of BSHD), no bias, causal 0; seq_q, seq_kv
    // and causal_off are each workgroup's own, from its record
    const FaVarlenRecord* plan;   // n_records records on the device (brn_flash_varlen_plan.h), every field validated on the host
    int n_records;                // the grid is n_records * kv_heads workgroups: workgroup w = (record w / kv_heads, K / V head w % kv_heads)
    int window_left, window_right;   // key j takes part in query i's row exactly when i + off - window_left <= j <= i + off + window_right,
                                     // off = len_kv - len_q of the row's sequence; -1 = unbounded on that side
    // brn_flash_attention_splitkv_forward; all zero = the kernels above, untouched.  With kv_splits >= 1: the packed-row kernels with the
    // walk of a workgroup cut into kv_splits ranges of K / V tiles, no bias, no plan (brn_flash_split_plan.h normalises both numbers)
    int kv_splits;                // S: workgroup w = (packed-row workgroup w / S, split w % S); (S - 1) * tiles_per_split < ceil(seq_kv / 64) <= S * tiles_per_split
    int tiles_per_split;          // split s walks K / V tiles s * tiles_per_split .. min((s + 1) * tiles_per_split, the row tile's nkt) - 1
    float* o_part;                // S > 1: [S][R][head_dim] normalised partial outputs, R = batch * heads * seq_q, row r = (b * heads + h) * seq_q + i; null when S == 1
    float* lse2_part;             // S > 1: [S][R] m + log2(l) of each partial (-inf: no visible key in the split); null when S == 1
    float* lse;                   // [R] ln sum_j exp(scale q . k_j) over the row's visible keys, or null = not wanted
    // brn_flash_attention_paged_forward; block_table == null = the kernels above, untouched.  With a table: the split form (kv_splits >= 1,
    // seq_kv = max_kv_len sizes the grid and the split) with K / V in pages: k, v [n_pages, page_size, kv_heads, head_dim] (kv_ss = kv_heads *
    // head_dim, kv_sh = head_dim, kv_sb = 0), each workgroup's seq_kv and causal_off its own sequence's, from kv_lens.  Both arrays hold
    // UNVALIDATED device data: a length is used as min(max(len, 0), seq_kv), a page number as min(max(page, 0), n_pages - 1)
    const int* block_table;       // [batch][max_pages]: key j of batch entry b is row j % page_size of page block_table[b][j / page_size]
    const int* kv_lens;           // [batch]
    long page_stride;             // elements between two pages: page_size * kv_heads * head_dim
    int page_log2;                // log2(page_size), 4 .. 8
    int n_pages, max_pages;       // max_pages * page_size >= seq_kv
    // brn_flash_attention_paged_kv_forward; 0 = the kernels above, untouched.  1 / 2 (with a table only): k and v point at a pool of bf16 /
    // fp16 elements (16-bit patterns; every stride and page_stride still counts ELEMENTS), read as stored by the 16-bit kernel of the same
    // type (s16 == kv_type) or widened exactly by the fp32 kernel (s16 == 0); any other pairing is refused.  Read by the launcher alone
    int kv_type;
    // brn_flash_attention_paged_fp8_forward: kv_type 3 (with a table only; any s16).  k and v point at a pool of OCP e4m3fn BYTES (strides
    // and page_stride still count elements), widened exactly to the kernel's own type as they are staged.  k_scale, v_scale: [kv_heads]
    // fp32 on the device, or null = all ones; device data like the table: read by the kernels alone, no address depends on them.  K / V
    // head g's workgroups run with scale * k_scale[g] in the place of scale, and a row's final y is multiplied by v_scale[g] once
    const float* k_scale; const float* v_scale;
    // brn_flash_attention_paged_varlen_forward; pv_plan == null = the kernels above, untouched.  With a plan: the paged form (any kv_type)
    // over a packed batch of new tokens.  batch = 1 and seq_q = pv_total_q describe q, y [total_q, heads, head_dim], lse [heads, total_q]
    // and the partials (row r = h * total_q + token); block_table is [pv_n_seqs][max_pages], kv_lens [pv_n_seqs].  pv_cu is UNVALIDATED
    // device data, read by the plan kernel alone, which writes pv_plan (brn_flash_paged_varlen_plan.h) ahead of the main launch; each
    // workgroup takes its sequence, seq_q = n_b, seq_kv = len_b, causal_off and its bases from the plan (fa_params).  pv_row0 is the
    // kernels' own: the workgroup's s_b
    const int* pv_cu;             // [pv_n_seqs + 1]
    int* pv_plan;                 // fa_pv_plan_ints(pv_n_seqs) ints
    int pv_n_seqs, pv_total_q, pv_row0;
};
constexpr int FA_KV_FP8 = 3;      // FlashAttentionParams::kv_type / KvAppendParams::kv_type of an e4m3fn pool (not a brn_kv_type: the public enum keeps its three values)
hipError_t launch_flash_attention(const FlashAttentionParams& p, hipStream_t s);

// brn_kv_cache_append (kernels/kv_cache.hip): token t of batch entry b becomes key min(max(kv_lens[b], 0), cap) + t of sequence b in the
// pool of the paged attention entries; keys at or past cap are dropped; kv_lens_out[b] = min(that length + seq_new, cap), written by a
// second launch (kv_lens_out may be kv_lens).  block_table and kv_lens hold UNVALIDATED device data, clamped as in FlashAttentionParams
struct KvAppendParams {
    const float* k_new; const float* v_new;   // fp32, 16-byte aligned, head_dim contiguous
    long new_sb, new_ss, new_sh;              // their element strides: batch entry, token, K / V head
    void* k_pages; void* v_pages;             // [n_pages, page_size, kv_heads, head_dim] of kv_type, 16-byte aligned
    int kv_type;                              // 0 fp32, 1 bf16, 2 fp16: the cast (E)x of the attention kernels, round to nearest even
    const int* block_table;                   // [batch][max_pages]
    const int* kv_lens;                       // [batch]
    int* kv_lens_out;                         // [batch], null = not wanted, or kv_lens itself
    int batch, seq_new, kv_heads, head_dim;
    long kv_ss, page_stride;                  // elements between two rows of a page (kv_heads * head_dim) and between two pages
    int page_log2, n_pages, max_pages;
    int cap;                                  // max_pages * page_size < 2^31
    // brn_kv_cache_append_fp8: kv_type FA_KV_FP8, an e4m3fn pool of bytes.  An element x of K head h is stored as the byte of
    // clamp(x / k_scale[h], +-448) rounded to nearest even (v_scale for V); [kv_heads] fp32 on the device, or null = all ones
    const float* k_scale; const float* v_scale;
    // brn_kv_cache_append_rope / _rope_fp8: rope_cos non-null selects the kernels' rope instantiation.  K token t of entry b is rotated
    // by the rule of RopeParams at table row min(L_b + t, rope_n_pos - 1), in fp32, before the cast; V is not.  Null: the plain append
    const float* rope_cos; const float* rope_sin;   // [rope_n_pos][rope_dim / 2] fp32, 16-byte aligned
    int rope_n_pos, rope_dim, rope_style;
    // brn_kv_cache_append_varlen: pv_cu non-null selects the packed form (no rope).  k_new, v_new are [pv_total_q, kv_heads, head_dim]
    // (new_ss / new_sh; new_sb and seq_new are not read), batch = pv_n_seqs.  The plan kernel turns pv_cu (UNVALIDATED device data) into
    // the starts s_b in pv_plan first; token s_b + t of sequence b becomes key L_b + t, kv_lens_out[b] = min(L_b + n_b, cap)
    const int* pv_cu;             // [pv_n_seqs + 1]
    int* pv_plan;                 // fa_pv_plan_ints(pv_n_seqs) ints
    int pv_n_seqs, pv_total_q;
};
hipError_t launch_kv_cache_append(const KvAppendParams& p, hipStream_t s);
// the device-side plan of the two packed paged entries (kernels/kv_cache.hip; the rule: brn_flash_paged_varlen_plan.h): one workgroup
// turns cu [n_seqs + 1] into plan's starts and tile prefix for groups of G query heads
hipError_t launch_paged_varlen_plan(const int* cu, int n_seqs, int total_q, int G, int* plan, hipStream_t s);

// brn_rope_forward (kernels/kv_cache.hip): y = x with the first rot_dim elements of every head row rotated in pairs by the caller's
// table.  Row p = min(max(positions[b], 0) + t, n_pos - 1) for token t of batch entry b (positions null = 0); pair i of rot_dim / 2 is
// (x[i], x[i + rot_dim / 2]) for style 0 (HALF) and (x[2i], x[2i + 1]) for style 1 (INTERLEAVED);
// a' = fl(fl(a cos[p][i]) - fl(b sin[p][i])), b' = fl(fl(b cos[p][i]) + fl(a sin[p][i])), never fused; d >= rot_dim is copied.
// positions holds UNVALIDATED device data: no address depends on it except through the clamp.  y may be x (the same strides)
struct RopeParams {
    const float* x; float* y;                 // fp32, 16-byte aligned, head_dim contiguous
    long sb, ss, sh;                          // element strides of both: batch entry, token, head
    const float* cos; const float* sin;       // [n_pos][rot_dim / 2] fp32, 16-byte aligned
    const int* positions;                     // [batch] or null
    int batch, seq, heads, head_dim;          // head_dim 32, 64 or 128; batch * seq * heads * head_dim / 8 < 2^31
    int n_pos, rot_dim, style;                // 1 <= n_pos <= 2^24; rot_dim a multiple of 16, 16 .. head_dim; style 0 or 1
};
hipError_t launch_rope(const RopeParams& p, hipStream_t s);

// the index kernels of the generic window route (kernels/window_generic.hip; geometry: kernels/window_generic_geometry.h), window sides
// 2 .. 32 other than the fused kernels' 12 and 7.  One struct for the three; each launcher reads the fields its kernel needs
struct WindowGenericParams {
    int B, H, W, C, heads;   // token map [B, H, W, C], C == heads * 32
    int ws, shift;           // window side; 0 or ws / 2
    int s16;                 // storage type of qkv and att: 0 fp32, 1 bf16, 2 fp16
    // window_pack: qkv [B, H, W, 3C] (storage type) -> q, k, v [slots, heads, ws^2, 32] fp32; pad positions from qkv_bias [3C]
    const float* qkv; const float* qkv_bias;
    float* q; float* k; float* v;
    // window_bias_build: rel_table [heads][(2 ws - 1)^2] -> bias [wgen_bias_patterns, heads, ws^2, ws^2] fp32, pre-divided by scale
    const float* rel_table; float* bias; float scale;
    // window_scatter: y [slots, heads, ws^2, 32] fp32 -> att [B, H, W, ld_att] (storage type), heads-major in the first C columns
    const float* y; float* att; int ld_att;
};
hipError_t launch_window_pack(const WindowGenericParams& p, hipStream_t s);
hipError_t launch_window_bias_build(const WindowGenericParams& p, hipStream_t s);
hipError_t launch_window_scatter(const WindowGenericParams& p, hipStream_t s);

// the two kernels of brn_deform_conv2d_offsets_forward (kernels/deform_im2col.hip; geometry: kernels/deform_sample_geometry.h; host route:
// brn_deform_offsets.cpp).  One struct for both; each launcher reads the fields its kernel needs
struct DeformOffsetsParams {
    int B, C, H, W;                  // the sampled map: C real channels
    int kh, kw, stride_h, stride_w, pad_h, pad_w, dil_h, dil_w;
    int G;                           // offset groups: channel c reads the offsets / mask of group c / (C / G)
    int Ho, Wo;
    const float* offset;             // [B, 2 G kh kw, Ho, Wo] fp32 (dy, dx interleaved per (group, tap))
    const float* mask;               // [B, G kh kw, Ho, Wo] fp32, or null = no modulation
    // deform_om_pack (G == 1): -> om [B, Ho, Wo, om_ld] fp32 = 2 kh kw offsets | kh kw multipliers (1.0f without a mask) | zero pad columns
    float* om; int om_ld;
    // deform_im2col: x [B, H, W, ldx] channels-last in the storage type s16 (0 fp32, 1 bf16, 2 fp16), Cp >= C channels a pixel (multiple of 32,
    // the pad channels are never read) -> col [rows][kh kw Cp] in the same type = rows [m0, m0 + rows) of the column matrix, K = (tap, channel)
    const float* x; int ldx, Cp, s16;
    float* col; int m0, rows;
};
hipError_t launch_deform_om_pack(const DeformOffsetsParams& p, hipStream_t s);
hipError_t launch_deform_im2col(const DeformOffsetsParams& p, hipStream_t s);

// ---- data movement / elementwise (HBM-bound) ------------------------------------------------------------
// bilinear, align_corners=true, channels-last window -> window; optional accumulate (y += )
hipError_t launch_resize_nhwc(const float* x, int B, int Hin, int Win, int C, int ldx, int x_coff,
                              float* y, int Hout, int Wout, int ldy, int y_coff, hipStream_t s, int bf16 = 0, int accumulate = 0);
// NCHW planar bilinear (the 3-channel image -> half scale), align_corners=true
hipError_t launch_resize_nchw(const float* x, int BC, int Hin, int Win, float* y, int Hout, int Wout, hipStream_t s);
// NCHW -> NHWC window and back
// (bf16 = 1: the channels-last side is a bf16 map, ld / coff in elements; the NCHW side is always fp32)
hipError_t launch_nchw_to_nhwc(const float* x, int B, int C, int H, int W, float* y, int ldy, int y_coff, hipStream_t s, int bf16 = 0);
hipError_t launch_nhwc_to_nchw(const float* x, int B, int C, int H, int W, int ldx, int x_coff, float* y, hipStream_t s, int bf16 = 0);
// image2patches (birefnet.rs:288-300): x NCHW [B,Cimg,H,W] -> y[b, th, tw, (c,gh,gw)] channels-last, ld = ldy
hipError_t launch_image2patches(const float* x, int B, int Cimg, int H, int W, int th, int tw,
                                float* y, int ldy, int cpad, hipStream_t s, int bf16 = 0);
// per-(b,c) mean over H*W of a channels-last window: out[b][c]   (aspp.rs:314)
size_t gap_scratch_floats(int B, int HW, int C);
hipError_t launch_gap_nhwc(const float* x, int B, int HW, int C, int ldx, int x_coff, float* scratch, float* out, hipStream_t s, int bf16 = 0);
// tiny dense layers on [B,Cin] vectors: y[b][n] = act((sum_k x[b][k] w[n*ldw + w_off + k]) * scale[n] + shift[n])
hipError_t launch_small_fc(const float* x, int B, int Cin, const float* w, int ldw, int w_off, int N,
                           const float* scale, const float* shift, int act, float* y, hipStream_t s);
// GDT gate (birefnet.rs:327-329): a = sigmoid(dot(g[pix][0:16], w) + b); p[pix][0:C] *= a
hipError_t launch_gdt_gate(float* p, int npix, int C, int ldp, int p_coff, const float* g, int ldg,
                           const float* w, float bias, hipStream_t s, int bf16 = 0);
// per-pixel dot: y[pix] = dot(x[pix][0:C], w) (+ bias)
hipError_t launch_pixel_dot(const float* x, int npix, int C, int ldx, int x_coff, const float* w, float bias,
                            float* y, hipStream_t s, int bf16 = 0);
// contiguous fp32 -> bf16 (round to nearest even)
hipError_t launch_f32_to_bf16(const float* x, size_t n, float* y_bf16, hipStream_t s, int f16 = 0);   // f16: fp16 instead (compute mode BRN_F16)
hipError_t launch_bf16_to_f32(const float* x_bf16, size_t n, float* y, hipStream_t s, int f16 = 0);
// final head (birefnet.rs:372-375 with conv_out1 commuted through the bilinear upsample):
// out[b][oy][ox] = bilinear(q [B,h,w] -> H,W) + t[b][oy][ox] (+bias); optional sigmoid
hipError_t launch_final_head(const float* q, int B, int h, int w, const float* t, float bias, int H, int W,
                             int apply_sigmoid, float* out, hipStream_t s);
// t = stencil5x5(x): the composed ipt_blk1 head on the NCHW image [B,3,H,W]; k = [9 border cases][5][5][3], bias = [9]
hipError_t launch_head_stencil5x5(const float* img, int B, int H, int W, const float* k, const float* bias, float* y, hipStream_t s);
// ---- image pre/post-processing (kernels/imageproc.hip; infer_image.rs:44-67,84-110) ----
hipError_t launch_resample_v_u8(const unsigned char* in, int h, int w, int C, int nh, const int* left, const int* count,
                                const float* wts, int max_taps, float* out, hipStream_t s);
// out_f32 != null: channels 0..2 as ((v/255) - mean[c]) / std[c] into NCHW [3][nh][nw]; else u8 [nh][nw][C]
hipError_t launch_resample_h(const float* in, int nh, int w, int C, int nw, const int* left, const int* count, const float* wts,
                             int max_taps, unsigned char* out_u8, float* out_f32, const float* mean, const float* stdv, hipStream_t s);
hipError_t launch_mask_u8(const float* logits, long n, int apply_sigmoid, unsigned char* out, hipStream_t s);
// y = sigmoid(x)
hipError_t launch_sigmoid(const float* x, size_t n, float* y, hipStream_t s);
// modulator epilogue for deformable mode: columns [c0,c1) of rows get 2/(1+exp(-x))   (aspp.rs:173-174)
hipError_t launch_mod_sigmoid2(float* x, size_t rows, int ld, int c0, int c1, hipStream_t s);

} // namespace brn
