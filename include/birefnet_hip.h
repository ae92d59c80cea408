/*
 * birefnet_hip.h — C ABI of libbirefnet_hip.so (MI355X / gfx950 native BiRefNet inference path).
 *
 * Every entry point is what the reference crate's FFI for the hot path would bind.  Citations are into
 * /root/reference (imperatormk/candle-birefnet); the Rust shim a maintainer would add is in INTEGRATION.md.
 *
 * Conventions
 *   - plain C: pointers + sizes, no C++/torch types.  All tensors are contiguous fp32.
 *   - brn_status: 0 = ok, non-zero = error; the message is available from brn_last_error() (thread-local).
 *     No exception or abort crosses the boundary (the one reference panic, swin.rs:352, is an error here).
 *   - brn_mem says where a caller buffer lives.  BRN_MEM_DEVICE pointers are HIP device pointers of the
 *     model's device; BRN_MEM_HOST buffers are staged through HBM by the library (H2D/D2H on `stream`).
 *   - `stream` is a hipStream_t passed as void* (NULL = the default stream).  Calls are asynchronous for
 *     BRN_MEM_DEVICE buffers and synchronous (stream-synchronised before return) for BRN_MEM_HOST output.
 *     A model handle owns ONE workspace: forwards on it are serialised on the host by a mutex and, when consecutive calls
 *     use different streams, on the GPU by an event (the later call's stream waits for the earlier forward's last kernel),
 *     so a handle may be driven from several threads / streams; for concurrent forwards use one handle per stream.
 *   - image tensors at this boundary are NCHW like candle's (infer_image.rs:67); the library's internal
 *     layout (NHWC) is not visible.
 *   - there is NO CPU fallback: every call needs a HIP device and fails with BRN_ERR_NO_DEVICE without one.
 */
#ifndef BIREFNET_HIP_H
#define BIREFNET_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define BRN_ABI_VERSION 1

typedef int brn_status;
enum {
    BRN_OK = 0,
    BRN_ERR_INVALID_ARG = 1,   /* bad shape / null pointer / unsupported config          */
    BRN_ERR_MISSING_TENSOR = 2,/* weight name absent (candle: Err from vb.get)            */
    BRN_ERR_SHAPE = 3,         /* weight present with the wrong shape                     */
    BRN_ERR_NO_DEVICE = 4,     /* no usable HIP device                                    */
    BRN_ERR_HIP = 5,           /* a HIP runtime call failed                               */
    BRN_ERR_OOM = 6            /* device workspace allocation failed                      */
};

typedef enum { BRN_MEM_HOST = 0, BRN_MEM_DEVICE = 1 } brn_mem;
/* Arithmetic of the contraction kernels.  In the BRN_F32* modes (and BRN_BF16_OPERANDS) everything else — LayerNorm, softmax, epilogues,
 * storage — is fp32 (the reference runs DType::F32, infer_image.rs:26):
 *   BRN_F32            fp32 operands on the fp32 matrix instruction (v_mfma_f32_32x32x2_f32), exact fmaf chain
 *   BRN_F32_SPLIT3     fp32 operands split error-free into 3 bf16 planes, 6 bf16 MFMAs per product, fp32 accumulate:
 *                      fp32-class accuracy (dropped terms < 2^-24 of a product) at 2.67x the fp32-MFMA rate
 *   BRN_F32_SPLIT2     2 planes, 3 MFMAs: ~2^-16 relative per product
 *   BRN_F32_HALF2      fp32 operands as TWO fp16 planes of the operand scaled by a power of two (weights: per tensor, so that the largest
 *                      lands in (2^13, 2^14]; activations: by 8), 3 fp16 MFMAs per product (hh, hl, lh), fp32 accumulate, the
 *                      accumulator un-scaled exactly: ~2^-22 relative per product — fp32-class accuracy at twice BRN_F32_SPLIT3's
 *                      matrix rate.  Range: a GEMM input activation of magnitude >= 8190 overflows fp16 and the logits come back
 *                      NaN (never silently wrong); BRN_F32_SPLIT3 has fp32's full range.  A deformable convolution's GEMM input is
 *                      modulator x bilinear sample, up to 2 |x|: there the ceiling on the sampled map is half that, 4095.  Beyond it the
 *                      result is non-finite as well (an offset that is itself NaN poisons its sample instead of dropping it).
 *   BRN_BF16_OPERANDS  operands rounded to bf16, fp32 accumulate, fp32 storage: superseded by BRN_BF16; the value is reserved, the
 *                      product library answers BRN_ERR_INVALID_ARG (only libbirefnet_hip_diag.so, `make diag`, still builds it)
 *   BRN_BF16           the bf16 throughput mode of BASELINE configs[2..4]: activations AND weights live in HBM as bf16,
 *                      bf16 MFMA with fp32 accumulation, fp32 statistics inside LayerNorm / softmax / GAP; x and the logits
 *                      stay fp32 at this boundary.  Parity is informational (error vs the fp32 oracle is reported).
 *   BRN_F16            the same graph and kernels as BRN_BF16 with fp16 as the 16-bit type: activations and weights live in HBM as fp16, fp16 MFMA
 *                      (the bf16 rate), fp32 accumulate / statistics / residual stream.  Same bytes and speed, 3 more mantissa bits: the error
 *                      against the fp32 oracle is ~8x smaller than BRN_BF16's (masks within 1e-3 of the reference's).
 *                      Range: a stored activation of magnitude >= 65520 becomes Inf (the logits NaN); BRN_BF16 has fp32's exponent range.
 *   BRN_BF16_DEC_SPLIT2  mixed: the Swin backbone (79 % of the FLOPs) as BRN_BF16, everything after it — multi-scale / context fusion,
 *                      squeeze module, decoder — as BRN_F32_SPLIT2 on fp32 maps.  The decoder's ~20 chained bf16 roundings are most of mode
 *                      BRN_BF16's error; this mode pays for removing them where they are cheapest. */
typedef enum { BRN_F32 = 0, BRN_F32_SPLIT3 = 1, BRN_F32_SPLIT2 = 2, BRN_BF16_OPERANDS = 3, BRN_BF16 = 4, BRN_BF16_DEC_SPLIT2 = 5, BRN_F32_HALF2 = 6, BRN_F16 = 7 } brn_dtype;

/* D1 of SURVEY.md §8: what DeformConvASPP::forward computes.
 * REFERENCE_CPU = aspp.rs:183-185 (offset/modulator discarded, regular_conv(x)) — the graded parity target.
 * DEFORMABLE    = aspp.rs:58-165 (Metal path: modulated deformable im2col + matmul).                     */
typedef enum { BRN_DEFORM_REFERENCE_CPU = 0, BRN_DEFORM_DEFORMABLE = 1 } brn_deform_mode;

/* activation selector of the op-level entry points */
typedef enum { BRN_ACT_NONE = 0, BRN_ACT_RELU = 1, BRN_ACT_GELU_ERF = 2 } brn_act;

/* Mirrors BiRefNetConfig (birefnet.rs:13-67) + SwinConfig (swin.rs:14-88), field for field,
 * decorative fields included.  BiRefNet::new ignores `backbone` and always builds swin_l (birefnet.rs:390-391);
 * here the swin_* fields are honoured so that reduced-depth models can be built for tests. */
typedef struct brn_config {
    int size_w, size_h;            /* BiRefNetConfig.size (never read in forward)                  */
    char backbone[32];             /* "swin_v1_l" (ignored, as in the reference)                   */
    int backbone_channels[4];      /* [192,384,768,1536]                                           */
    int mul_scl_ipt;               /* 1                                                            */
    int ms_supervision;            /* 1 (decorative)                                               */
    int dec_ipt;                   /* 1 (decorative: decoder always uses ipt blocks)               */
    int use_aspp_deformable;       /* 1                                                            */
    int cxt[3]; int n_cxt;         /* [192,384,768], 3                                             */
    /* SwinConfig */
    int embed_dim;                 /* 192 */
    int depths[4];                 /* [2,2,18,2] */
    int num_heads[4];              /* [6,12,24,48] */
    int window_size;               /* 12 */
    float mlp_ratio;               /* 4.0 */
    int patch_size;                /* 4 */
    int in_channels;               /* 3 */
    float drop_path_rate;          /* 0.2 (unused) */
    /* library-side switch (not in the reference config) */
    int deform_mode;               /* brn_deform_mode */
} brn_config;

/* One weight tensor as VarBuilder would hand it over (names: SURVEY.md App. A; shapes as in the safetensors). */
typedef struct brn_named_tensor {
    const char* name;
    const float* data;   /* host pointer, fp32, contiguous; the library copies, the caller keeps ownership */
    const int64_t* shape;
    int ndim;
} brn_named_tensor;

typedef struct brn_model brn_model;     /* BiRefNet (birefnet.rs:380-385) */
typedef struct brn_swin brn_swin;       /* stand-alone SwinTransformer (swin.rs:718-723) */

/* ---- library ------------------------------------------------------------------------------------------ */
int brn_abi_version(void);
const char* brn_last_error(void);               /* thread-local; wrapped into candle_core::Error::Msg by the shim */
brn_status brn_device_count(int* n);
const char* brn_build_info(void);               /* "gfx950 hipcc <ver> ..." */

/* ---- config ------------------------------------------------------------------------------------------- */
/* BiRefNetConfig::swin_l() / Default (birefnet.rs:32-46, 64-66) + SwinConfig::swin_l() (swin.rs:69-80). */
void brn_config_default_swin_l(brn_config* cfg);
/* BiRefNetConfig::lateral_channels (birefnet.rs:50-53) and x4_channels (birefnet.rs:56-61). */
void brn_config_lateral_channels(const brn_config* cfg, int out[4]);
int brn_config_x4_channels(const brn_config* cfg);

/* ---- model lifecycle: BiRefNet::new (birefnet.rs:389-409) --------------------------------------------- */
/* Weights are looked up by the names of SURVEY.md App. A below `prefix` ("" for a full checkpoint).
 * Missing name -> BRN_ERR_MISSING_TENSOR naming it; extra names are ignored.  The loaded-but-unused heads
 * (gdt_convs_pred_*, conv_ms_spvn_*; birefnet.rs:150-166) must be present, as in the reference.
 * max_batch/max_h/max_w size the HBM workspace (forward with larger inputs re-plans it). */
brn_status brn_model_create(const brn_config* cfg, const brn_named_tensor* weights, size_t n_weights,
                            int device_ordinal, brn_dtype compute_dtype,
                            int max_batch, int max_h, int max_w, brn_model** out);
/* VarBuilder::from_mmaped_safetensors(&[path], DType::F32, &device) + BiRefNet::new(config, vb) in one call
 * (infer_image.rs:35-40).  The file is memory-mapped and parsed natively (8-byte LE header length, JSON index, raw LE
 * tensors); F32 is read in place, F16 / BF16 are widened to fp32 as candle's VarBuilder does for DType::F32.  Tensor names
 * are looked up below `prefix` ("" or NULL for a full checkpoint).  Errors as brn_model_create, plus BRN_ERR_INVALID_ARG for
 * an unreadable or malformed file. */
brn_status brn_model_create_from_safetensors(const brn_config* cfg, const char* path, const char* prefix,
                                            int device_ordinal, brn_dtype compute_dtype,
                                            int max_batch, int max_h, int max_w, brn_model** out);
void brn_model_destroy(brn_model* m);

/* BiRefNet::forward_logits (birefnet.rs:412-461): x [B,3,H,W] -> logits [B,1,H,W] (pre-sigmoid).
 * H and W must be multiples of 32 (the decoder's image2patches, birefnet.rs:288-300, needs it). */
brn_status brn_forward_logits(brn_model* m, const float* x_nchw, int B, int H, int W, brn_mem in_loc,
                              float* logits_out, brn_mem out_loc, void* stream);
/* BiRefNet::forward (birefnet.rs:466-469): sigmoid(forward_logits). */
brn_status brn_forward(brn_model* m, const float* x_nchw, int B, int H, int W, brn_mem in_loc,
                       float* mask_out, brn_mem out_loc, void* stream);

/* Pub fields used individually by bench_inference.rs:34,77,83:
 * model.backbone.forward(x) -> 4 NCHW feature maps (swin.rs:768-797).  outs[i] is [B, C_i, ceil(H/4)/2^i, ...]. */
brn_status brn_model_backbone_forward(brn_model* m, const float* x_nchw, int B, int H, int W, brn_mem in_loc,
                                      float* const outs[4], brn_mem out_loc, void* stream);
/* model.squeeze_module.forward(x4) (birefnet.rs:86-94): [B,5760,h,w] -> [B,3072,h,w]. */
brn_status brn_model_squeeze_forward(brn_model* m, const float* x4_nchw, int B, int h, int w, brn_mem in_loc,
                                     float* out, brn_mem out_loc, void* stream);
/* model.decoder.forward(x, x1, x2, x3, x4) (birefnet.rs:278-376). x [B,3,H,W]; x1..x4 at H/4..H/32 with
 * 384/768/1536/3072 channels. */
brn_status brn_model_decoder_forward(brn_model* m, const float* x_nchw, const float* x1, const float* x2,
                                     const float* x3, const float* x4, int B, int H, int W, brn_mem in_loc,
                                     float* logits_out, brn_mem out_loc, void* stream);

/* BiRefNetDecoder::new(config, vb) on its own (birefnet.rs:170-273): a handle that holds ONLY the decoder's weights (names relative
 * to `prefix`, e.g. "decoder."; the loaded-but-unused heads of birefnet.rs:229-243 must be present, as in the reference).  Such a handle
 * serves brn_model_decoder_forward (and brn_model_destroy); every entry that needs the backbone or the squeeze module answers
 * BRN_ERR_INVALID_ARG on it. */
brn_status brn_decoder_create(const brn_config* cfg, const brn_named_tensor* weights, size_t n_weights, const char* prefix,
                              int device_ordinal, brn_dtype compute_dtype, brn_model** out);

/* How a forward is spread over HIP streams (it never changes what is computed per image; results for a given setting are repeatable bit
 * for bit).  sub_batch_streams: a device-resident batch of B >= 4 images runs as that many sub-batches (>= 2 images each) on as many
 * streams, forked from and joined to the caller's stream, each with its own workspace (0 = library default: 2, or BRN_SPLIT_STREAMS;
 * 1 = everything on the caller's stream).  branch_stream_mask: independent branches of one forward on auxiliary streams — bits 0-2 the
 * ASPP branches, 3 the image-patch convolutions, 4 the lateral convolutions; -1 = automatic (on when the batch runs as one part), 0 = off. */
brn_status brn_model_set_streams(brn_model* m, int sub_batch_streams, int branch_stream_mask);

/* Per-stage wall time of the last forward on this handle, measured with HIP events on the call's stream:
 * [0]=backbone full, [1]=backbone half+fusion, [2]=squeeze, [3]=decoder, [4]=total (ms).  Mirrors the timers of
 * bench_inference.rs:37-92.  Enabled by brn_model_set_profiling(m, 1) (adds event records + one sync). */
brn_status brn_model_set_profiling(brn_model* m, int enable);
brn_status brn_model_last_timings(brn_model* m, float ms[5]);
/* Per-kernel-family accounting of the last profiled forward: for family f (see brn_kernel_family_name)
 * launches[f], ms[f] (HIP-event time around each launch, summed), flop[f] (2*M*N*K of the launches) and bytes[f] (their
 * algorithmic operand + result bytes).  After the families come coarse graph regions counted a second time under their own
 * rows ("region_aspp" = every launch of the ASPPDeformable modules, aspp.rs:303-333; "region_none" stays zero).
 * n is the array capacity; returns the number of rows (families + regions) through *n_out. */
brn_status brn_model_last_kernel_stats(brn_model* m, int n, int* launches, float* ms, double* flop,
                                       double* bytes, int* n_out);
const char* brn_kernel_family_name(int f);

/* ---- stand-alone SwinTransformer: SwinTransformer::new / forward (swin.rs:725-797) -------------------- */
/* Any SwinConfig (swin_t / swin_s / swin_b / swin_l, or one of these with another window_size, 2 .. 32; head_dim 32) and any input size.
 * The handle is built for the arithmetic that brn_set_op_compute selected on the creating thread (default BRN_F32): window 12 uses the
 * mode's own attention kernel, window 7 the fp32-MFMA attention kernel in every mode (on bf16 matrices in mode BRN_BF16), every other
 * window_size the generic route of brn_window_attention_forward (pack, flash attention with bias, scatter).  The same range holds for
 * the window_size of brn_model_create, brn_model_create_from_safetensors and brn_decoder_create; outside it they answer
 * BRN_ERR_INVALID_ARG with a message naming window_size and the range. */
brn_status brn_swin_create(const brn_config* cfg /* swin_* fields */, const brn_named_tensor* weights,
                           size_t n_weights, const char* prefix, int device_ordinal, brn_swin** out);
void brn_swin_destroy(brn_swin* s);
brn_status brn_swin_forward(brn_swin* s, const float* x_nchw, int B, int H, int W, brn_mem in_loc,
                            float* const outs[4], brn_mem out_loc, void* stream);

/* ---- op-level entry points (the candle ops the reference calls; used by the parity tests) -------------- */
/* Selects the contraction arithmetic (brn_dtype) used by brn_linear_forward / brn_conv2d_forward on the calling thread
 * (default BRN_F32); models carry their own setting from brn_model_create. */
brn_status brn_set_op_compute(int dtype);
/* candle_nn::linear / linear_no_bias + optional gelu_erf + optional residual (swin.rs:98-107,130-131,406-407):
 * y[M,N] = act(x[M,K] @ w[N,K]^T + bias) (+ residual[M,N]).  bias/residual may be NULL. */
brn_status brn_linear_forward(const float* x, int M, int K, const float* w, const float* bias, int N,
                              int act, const float* residual, float* y, brn_mem loc, int device_ordinal,
                              void* stream);
/* The attention half's tail of a Swin block as the reference chains it (swin.rs:310 proj, :406 shortcut + attn, :407 norm2 — and the
 * same shape at the end of the MLP, :106-107 + the next block's norm1): x_out = x W^T + bias + residual, y_out = LayerNorm(x_out) gamma +
 * beta (eps inside the sqrt, biased variance).  x [M,K], w [N,K], residual / x_out / y_out [M,N], all fp32 at this boundary.  In compute
 * mode bf16 (brn_set_op_compute) x is rounded to bf16 at the edge and the pair runs as ONE row-owning kernel where the shape allows (N = 192,
 * 384, 768: gemm_wstat_ln_bf16_kernel / gemm_rowln_bf16_kernel; y_out is then a bf16-rounded matrix), otherwise as a GEMM and a LayerNorm launch. */
brn_status brn_linear_residual_layer_norm_forward(const float* x, int M, int K, const float* w, const float* bias, int N,
                                                  const float* residual, const float* gamma, const float* beta, float eps,
                                                  float* x_out, float* y_out, brn_mem loc, int device_ordinal, void* stream);

/* candle_nn::layer_norm(dim, eps) forward (swin.rs:333,335,486,680,754): rows of length C. */
brn_status brn_layer_norm_forward(const float* x, int rows, int C, const float* gamma, const float* beta,
                                  float eps, float* y, brn_mem loc, int device_ordinal, void* stream);
/* candle_nn::conv2d / conv2d_no_bias forward (decoder.rs:44-45,104,113; aspp.rs:39-45; swin.rs:677), NCHW,
 * optional eval-mode batch_norm (decoder.rs:105,129: (x-mean)/sqrt(var+eps)*gamma+beta) and activation fused.
 * bn = {gamma,beta,running_mean,running_var} each [O] or all NULL. */
brn_status brn_conv2d_forward(const float* x, int B, int C, int H, int W, const float* w, const float* bias,
                              int O, int kh, int kw, int stride, int pad, int dil,
                              const float* bn_gamma, const float* bn_beta, const float* bn_mean,
                              const float* bn_var, float bn_eps, int act,
                              float* y, brn_mem loc, int device_ordinal, void* stream);
/* Tensor::upsample_bilinear2d(h, w, align_corners=true) (birefnet.rs:332,425,435-438,450-452), NCHW. */
brn_status brn_upsample_bilinear2d(const float* x, int B, int C, int H, int W, int out_h, int out_w,
                                   float* y, brn_mem loc, int device_ordinal, void* stream);
/* The attention half of SwinTransformerBlock::forward between norm1 and the residual (swin.rs:356-403):
 * pad -> roll(-shift) -> window_partition -> WindowAttention::forward (qkv, q*scale, q@k^T + rel-pos bias
 * (+ SW-MSA mask), softmax, @v, proj) -> window_reverse -> roll(+shift) -> crop.
 * x [B,H,W,C] is the norm1 output; y [B,H,W,C].  rel_table is relative_position_bias_table [(2ws-1)^2, heads].
 * head_dim must be 32; 2 <= window_size <= 32; shift 0 or window_size / 2 (anything else is BRN_ERR_INVALID_ARG with a message naming
 * window_size and the range).
 * window_size 12 (Swin-B / L, swin.rs:55-80) runs the mode's own fused attention kernel and 7 (Swin-T / S, swin.rs:27-52) the fused
 * fp32-MFMA kernel, exactly as before the wider range existed.  Every other window_size takes the generic route: qkv GEMM -> pack (roll,
 * pad and partition as index math, q / k / v to [windows, heads, N, 32]) -> the kernel of brn_flash_attention_bias_forward with the
 * relative-position bias (+ the -100 region mask of swin.rs:603-655 for the windows of the last window row / column, the only ones whose
 * mask is not zero) pre-divided by the scale -> scatter (window reverse, roll back, crop) -> proj GEMM.  The reference's semantics hold
 * on that route: the map is padded after norm1, so a pad token's q / k / v is the qkv bias (rounded to the 16-bit type in BRN_BF16 /
 * BRN_F16) and it takes part as a key; shift 0 has no mask even on a padded canvas; a map smaller than the window is one padded window.
 * Its attention arithmetic is that of brn_flash_attention_bias_forward in the same compute mode: one exact fp32 kernel for BRN_F32 and
 * the three plane modes (so these differ only by their two GEMMs), the 16-bit kernel for BRN_BF16 / BRN_F16.  A repeated call repeats
 * its bits. */
brn_status brn_window_attention_forward(const float* x, int B, int H, int W, int C, int heads, int window_size,
                                        int shift, const float* qkv_w, const float* qkv_b,
                                        const float* proj_w, const float* proj_b, const float* rel_table,
                                        float* y, brn_mem loc, int device_ordinal, void* stream);
/* candle_mps_flash_attention::flash_attention_with_bias / flash_attention_with_repeating_bias as WindowAttention::forward
 * calls them (swin.rs:243, 252; examples/test_flash_bias.rs):
 *   y[b,h] = softmax_rows( scale * (q[b,h] k[b,h]^T + bias[b % n_bias, h]) ) v[b,h]
 * q, k, v, y: [batch, heads, N, head_dim] contiguous; bias: [n_bias, heads, N, N] contiguous or NULL (n_bias 0).
 * The bias is added to the UNSCALED scores, as MFA does; swin.rs:233-250 pre-multiplies it by 1/scale for that reason.
 * scale 0 = 1/sqrt(head_dim).  n_bias 1 = one bias for every batch entry (W-MSA);
 * n_bias = n_windows with batch % n_bias == 0 = the repeating form (SW-MSA, the index of swin.rs:291-294).
 * Limits (each violation is BRN_ERR_INVALID_ARG, checked before the device): head_dim == 32; 1 <= N <= 144; batch >= 1, heads >= 1
 * (batch * heads < 2^31); n_bias >= 0, bias NULL exactly when n_bias == 0, batch % n_bias == 0 when n_bias > 0; scale finite and >= 0;
 * q, k, v, y not NULL; y does not overlap an input; BRN_MEM_DEVICE q, k, v, y 16-byte aligned.  All five buffers live where `loc`
 * says; the stream and synchronisation conventions at the top of this header apply.
 * Arithmetic follows brn_set_op_compute on the calling thread.  BRN_F32: v_mfma_f32_16x16x4_f32, exact fmaf chains.  BRN_F32_SPLIT3 /
 * BRN_F32_SPLIT2 / BRN_F32_HALF2: the SAME fp32 kernel, bit-identical results (exact fp32 attention between the mode's own GEMMs, as
 * window-7 attention in those modes).  BRN_BF16 / BRN_F16: q, k, v are rounded to the 16-bit type at the edge (round to nearest
 * even), q k^T and P v run on the 16-bit matrix instructions with fp32 accumulation, and the softmax numerators are rounded to the
 * 16-bit type for P v; the bias, the scores, the row maximum, the row sum (taken from the unrounded numerators) and y stay fp32.
 * Softmax subtracts the row maximum first; the result for a batch entry does not depend on `batch`.
 * Not provided HERE, provided by brn_flash_attention_forward below (without a bias): the causal flag of the MFA calls (the reference
 * always passes false to these two); long sequences and head_dim 64 / 128 (the LLM shapes of examples/bench_flash_attn.rs:77-84); the
 * [batch, seq, heads, head_dim] layout of the bias-free flash_attention. */
brn_status brn_attention_forward(const float* q, const float* k, const float* v, int batch, int heads, int N, int head_dim,
                                 const float* bias, int n_bias, float scale,
                                 float* y, brn_mem loc, int device_ordinal, void* stream);
/* candle_mps_flash_attention::flash_attention(&q, &k, &v, causal), the third call of the reference's flash-attn dependency
 * (examples/bench_flash_attn.rs:39-53, sequences of 512 .. 8192, head_dim 64 / 128):
 *   y[b,h] = softmax_rows( scale * q[b,h] k[b,h]^T  [causal mask] ) v[b,h]
 * layout BRN_ATTN_BSHD: q, y [batch, seq_q, heads, head_dim] and k, v [batch, seq_kv, heads, head_dim] (flash_attention's layout);
 * layout BRN_ATTN_BHSD: [batch, heads, seq, head_dim] (brn_attention_forward's layout; bench_flash_attn.rs:19-21 before its transposes).
 * All four buffers are contiguous; one kernel serves both layouts through element strides.  scale 0 = 1/sqrt(head_dim).
 * causal 1: key j takes part in query i's row exactly when j <= i.  A masked key is left out of the row maximum and of the row sum (a
 * real exclusion, not an added -100); it requires seq_q == seq_kv.
 * Limits (each violation is BRN_ERR_INVALID_ARG with a message naming the limit, checked before the device): head_dim 32, 64 or 128;
 * 1 <= seq_q, seq_kv <= 65536; batch >= 1, heads >= 1; batch * heads * ceil(seq_q / 16) < 2^31; layout 0 or 1; causal 0 or 1; causal
 * requires seq_q == seq_kv; scale finite and >= 0; q, k, v, y not NULL; y overlaps no input; BRN_MEM_DEVICE q, k, v, y 16-byte aligned.
 * All four buffers live where `loc` says; the stream and synchronisation conventions at the top of this header apply.
 * The softmax is computed online: K and V are walked in tiles of 64 keys with a running row maximum, a running row sum and the output
 * accumulators in registers, rescaled whenever a tile raises the maximum; the [seq_q, seq_kv] score matrix never exists in memory.
 * Nothing is split over keys between workgroups and there are no atomics: an output row depends only on its own (batch entry, head),
 * its bits depend neither on `batch` nor on the launch grid, and a repeated call repeats its bits.
 * Arithmetic follows brn_set_op_compute on the calling thread, by the rule of brn_attention_forward.  BRN_BF16 / BRN_F16: q, k, v are
 * rounded to the 16-bit type at the edge (round to nearest even), q k^T and P v run on the 16-bit matrix instructions
 * (v_mfma_f32_16x16x32_{bf16,f16}) with fp32 accumulation, and the softmax numerators are rounded to the 16-bit type for P v; the
 * scores, the running maximum, the running sum (taken from the unrounded numerators) and y stay fp32.  Every other mode runs ONE exact
 * fp32 kernel (v_mfma_f32_16x16x4_f32): bit-identical results across BRN_F32, BRN_F32_SPLIT3, BRN_F32_SPLIT2 and BRN_F32_HALF2.
 * Not provided: a bias together with long sequences (brn_attention_forward has the bias, up to N = 144); a causal mask with
 * seq_q != seq_kv; head dims other than 32 / 64 / 128.  The bias together with long sequences is provided by
 * brn_flash_attention_bias_forward below. */
typedef enum { BRN_ATTN_BSHD = 0, BRN_ATTN_BHSD = 1 } brn_attn_layout;
brn_status brn_flash_attention_forward(const float* q, const float* k, const float* v,
                                       int batch, int seq_q, int seq_kv, int heads, int head_dim,
                                       int layout, int causal, float scale,
                                       float* y, brn_mem loc, int device_ordinal, void* stream);
/* flash_attention_with_bias / flash_attention_with_repeating_bias without the length limit of brn_attention_forward, and with their
 * causal flag: brn_flash_attention_forward plus an additive bias,
 *   y[b,h] = softmax_rows( scale * (q[b,h] k[b,h]^T + bias[b % n_bias, h])  [causal mask] ) v[b,h]
 * (Swin windows of 16 / 24 = N 256 / 576, relative-position or ALiBi-style biases on LLM shapes, key-padding masks).
 * bias: [n_bias, heads, seq_q, seq_kv] contiguous fp32, heads-major WHATEVER `layout` says for q / k / v / y (as MFA's bias is).  It is
 * added to the UNSCALED scores (the convention of brn_attention_forward and of swin.rs:231-233).  n_bias 1 = one bias for every batch
 * entry; n_bias > 1 with batch % n_bias == 0 = the repeating form; n_bias 0 with bias NULL runs the bias-free kernels and returns the
 * bits of brn_flash_attention_forward.  q, k, v, y, layout, causal, scale, loc, the stream rules and the arithmetic by
 * brn_set_op_compute are exactly those of brn_flash_attention_forward.  The bias stays fp32 in every mode: it joins the fp32 scores (as
 * the initial accumulator of q k^T) and is never rounded to the 16-bit type; an all-zero bias returns the bits of the bias-free entry.
 * A bias entry may be -inf: that key is excluded, it contributes exactly 0 to the row sum and to the output.  A row whose every visible
 * key is -inf comes back NaN.  +inf and NaN entries give unspecified values in their own row and nothing worse: no address depends on a
 * bias value.
 * Limits (each violation is BRN_ERR_INVALID_ARG with the prefix "flash attention bias:" and a message naming the limit, checked before
 * the device): every limit of brn_flash_attention_forward; n_bias >= 0; bias must be NULL exactly when n_bias == 0; batch % n_bias == 0;
 * y overlaps neither an input nor the bias; a BRN_MEM_DEVICE bias is 16-byte aligned.
 * The invariants of the bias-free entry hold: no split over keys, no atomics; an output row depends only on its own (batch entry, head)
 * and its bias pattern; the bits depend neither on `batch` nor on the launch grid, and a repeated call repeats its bits.
 * Not provided: a bias broadcast over heads; 16-bit bias storage; a causal mask with seq_q != seq_kv (brn_flash_attention_gqa_forward
 * below has it for seq_q < seq_kv, and K / V heads shared by a group of query heads). */
brn_status brn_flash_attention_bias_forward(const float* q, const float* k, const float* v,
                                            int batch, int seq_q, int seq_kv, int heads, int head_dim,
                                            int layout, int causal,
                                            const float* bias, int n_bias, float scale,
                                            float* y, brn_mem loc, int device_ordinal, void* stream);
/* brn_flash_attention_bias_forward for the attention of current decoders: a group of G = heads / kv_heads query heads shares one K / V
 * head (grouped-query attention; kv_heads 1 = multi-query), and the causal mask may lie over a K / V cache (seq_q < seq_kv: chunked
 * prefill, speculative or single-token decode):
 *   y[b,h] = softmax_rows( scale * (q[b,h] k[b, h / G]^T + bias[b % n_bias, h])  [causal mask] ) v[b, h / G]
 * q, y: [batch, seq_q, heads, head_dim] (BRN_ATTN_BSHD) or [batch, heads, seq_q, head_dim] (BRN_ATTN_BHSD); k, v: the same with seq_kv
 * and kv_heads.  Query head h reads K / V head h / G (the repeat_interleave(G) convention); K and V are never repeated in memory, and
 * a K / V tile is staged once for the G heads of its group.
 * bias: optional, [n_bias, heads, seq_q, seq_kv] fp32 indexed by QUERY head, with the rules of brn_flash_attention_bias_forward: added
 * to the unscaled scores, never rounded, -inf excludes a key, a row whose every visible key is -inf comes back NaN; n_bias 0 with bias
 * NULL selects the bias-free kernels.
 * causal 1: key j takes part in query i's row exactly when j <= i + (seq_kv - seq_q): the diagonal ends at the last key, so the last
 * query sees every key and query 0 sees keys 0 .. seq_kv - seq_q.  It requires seq_kv >= seq_q (every row sees key 0); with
 * seq_q == seq_kv it is the mask of the two entries above.  A masked key is a real exclusion, as there.
 * layout, scale, loc, the stream rules and the arithmetic by brn_set_op_compute are those of the two entries above: one exact fp32
 * kernel for BRN_F32 and the three plane modes, the 16-bit kernels for BRN_BF16 / BRN_F16.  No split over keys, no atomics; a row's
 * bits depend only on its own (batch entry, query head, bias pattern), neither on `batch` nor on the launch grid nor on which rows
 * share its workgroup; a repeated call repeats its bits.  The result carries the bits of brn_flash_attention_forward /
 * brn_flash_attention_bias_forward called on k, v repeated G times along heads (and, over a cache, with the causal mask written into the
 * bias as -inf).  With kv_heads == heads and seq_q == seq_kv (or causal 0) the call runs the kernels of those entries.
 * Limits (each violation is BRN_ERR_INVALID_ARG with the prefix "flash attention gqa:" and a message naming the limit, checked before
 * the device): every limit of brn_flash_attention_bias_forward except its causal one and its grid limit, which become: causal requires
 * seq_kv >= seq_q; G * seq_q < 2^31 and batch * kv_heads * ceil(G * seq_q / 64) < 2^31.  1 <= kv_heads <= heads and
 * heads % kv_heads == 0.
 * Not provided: a split over keys for single-token decode at long seq_kv (it contradicts the no-split invariant these entries promise:
 * a decode call is one workgroup per 64 / G .. 64 rows of a K / V head); sliding-window masks; variable-length batches; 16-bit tensors
 * at the boundary.  (Sliding-window masks and variable-length batches, without a bias and in the packed layout, are what
 * brn_flash_attention_varlen_forward below provides; the split over keys, as an entry with its own promise,
 * brn_flash_attention_splitkv_forward.) */
brn_status brn_flash_attention_gqa_forward(const float* q, const float* k, const float* v,
                                           int batch, int seq_q, int seq_kv, int heads, int kv_heads, int head_dim,
                                           int layout, int causal,
                                           const float* bias, int n_bias, float scale,
                                           float* y, brn_mem loc, int device_ordinal, void* stream);
/* brn_flash_attention_gqa_forward over a PACKED batch of sequences of unequal lengths, with a window mask:
 *   y[i,h] = softmax over the visible keys j of i's own sequence( scale * q[i,h] k[j, h / G]^T ) v[j, h / G]
 * q, y: [total_q, heads, head_dim]; k, v: [total_kv, kv_heads, head_dim]; contiguous fp32 where `loc` says (the packed "thd" layout: a
 * [batch, seq, heads, head_dim] tensor is the same memory with cu[b] = b * seq).
 * cu_seqlens_q, cu_seqlens_kv: n_seqs + 1 int32 values each, always HOST memory (like weights) whatever `loc` says.  Sequence s owns
 * rows cu[s] .. cu[s + 1] - 1; total_q = cu_seqlens_q[n_seqs], total_kv = cu_seqlens_kv[n_seqs].  Their content is validated on the host
 * before anything touches the device, and no address in a kernel depends on an unvalidated value.
 * The mask: with off = len_kv - len_q of the row's own sequence, key j of that sequence takes part in query i's row exactly when
 *   i + off - window_left <= j <= i + off + window_right;  -1 on a side = unbounded on that side.
 * (-1, -1) full attention; (-1, 0) the causal mask of the gqa entry, ending at the last key; (W - 1, 0) a causal sliding window of W
 * keys; (w, w) local bidirectional attention.  An excluded key is a real exclusion (in neither the maximum nor the sum), and a row
 * never sees a key of another sequence.  A sequence with len_q == 0 computes nothing, and its K / V rows are never read.
 * Grouping (query head h reads K / V head h / G, G = heads / kv_heads), scale (0 = 1/sqrt(head_dim)), the stream rules and the arithmetic
 * by brn_set_op_compute are those of brn_flash_attention_gqa_forward: one exact fp32 kernel for BRN_F32 and the three plane modes, the
 * 16-bit kernels for BRN_BF16 / BRN_F16.  No split over keys, no atomics; a row's bits depend only on its own sequence, query head and
 * window: not on n_seqs, not on the order of the sequences in the pack, not on the launch grid, not on which rows share its workgroup; a
 * repeated call repeats its bits.  A workgroup walks only the K / V tiles of 64 keys some row of it can see, so a window costs
 * O(len * window).  The result carries the bits of brn_flash_attention_gqa_forward on each sequence alone for (-1, -1) and (-1, 0), and
 * of brn_flash_attention_bias_forward on each sequence with k, v repeated G times and the window written into the bias as -inf.
 * The workgroup table derived from cu_seqlens is uploaded for the call through a temporary device allocation, so the call synchronises
 * the stream before it returns, also for BRN_MEM_DEVICE tensors; the cu arrays may be freed when it returns.  This is where its stream
 * rules differ from the gqa entry's: every call allocates and frees device memory (hipMalloc / hipFree, and hipFree waits for the
 * whole device, so work on other streams is synchronised too), and the call cannot be made while the stream is being captured into a
 * graph.
 * A window side of 65536 or more reaches past every sequence and is treated as 65536, with the bits of -1 on that side where -1 is
 * allowed (INT_MAX as "unbounded" is safe); it still counts as a window for the len_kv >= len_q rule.
 * Limits (each violation is BRN_ERR_INVALID_ARG with the prefix "flash attention varlen:" and a message naming the limit, checked
 * before the device): q, k, v, y, cu_seqlens_q, cu_seqlens_kv not NULL; head_dim 32, 64 or 128; heads >= 1, 1 <= kv_heads <= heads,
 * heads % kv_heads == 0; n_seqs >= 1; cu_seqlens must start at 0 and be non-decreasing; every len_q, len_kv <= 65536; total_q >= 1;
 * len_kv >= 1 wherever len_q >= 1; window_left >= -1, window_right >= -1; a window (either side >= 0) requires len_kv >= len_q for
 * every sequence with queries (every row then sees its diagonal key, and no row is empty); G * len_q < 2^31 and packed-row tiles *
 * kv_heads < 2^31 (tiles = the sum over sequences of ceil(G * len_q / 64)); scale finite and >= 0; y overlaps no input; BRN_MEM_DEVICE
 * q, k, v, y 16-byte aligned.
 * Not provided: a bias with packed sequences; the [batch, heads, seq, head_dim] layout; device-resident cu_seqlens; a split over keys;
 * 16-bit tensors at the boundary.  (The split over keys, for dense batches, is brn_flash_attention_splitkv_forward below.) */
brn_status brn_flash_attention_varlen_forward(const float* q, const float* k, const float* v,
                                              const int* cu_seqlens_q, const int* cu_seqlens_kv, int n_seqs,
                                              int heads, int kv_heads, int head_dim,
                                              int window_left, int window_right, float scale,
                                              float* y, brn_mem loc, int device_ordinal, void* stream);
/* brn_flash_attention_gqa_forward without a bias, with the K / V tiles of a call SPLIT between workgroups and the log-sum-exp of every
 * row: the entry for single-token or few-token decode over a long cache, where the gqa entry's grid of batch * kv_heads *
 * ceil(G * seq_q / 64) workgroups leaves most of the device idle, and for callers who merge attention over key ranges computed elsewhere.
 *   y[b,h] = softmax_rows( scale * q[b,h] k[b, h / G]^T  [causal mask] ) v[b, h / G],   lse[b,h,i] = ln sum_j exp(scale * q[b,h,i] . k[b, h / G, j])
 * q, k, v, y, layout, G = heads / kv_heads and scale (0 = head_dim^-0.5) are those of brn_flash_attention_gqa_forward; causal 1 ends the
 * mask at the last key and requires seq_kv >= seq_q.  lse: [batch, heads, seq_q] fp32, heads-major in either layout (like a bias), the sum
 * over the row's visible keys; NULL = not wanted.  Arithmetic by brn_set_op_compute: one exact fp32 kernel for BRN_F32 and the three
 * plane modes, the 16-bit kernels for BRN_BF16 / BRN_F16.
 * The split: nkt = ceil(seq_kv / 64) K / V tiles, tps = ceil(nkt / kv_splits), S = ceil(nkt / tps) (no empty trailing split, S <=
 * kv_splits); split s owns tiles s * tps .. min((s + 1) * tps, nkt) - 1, so the boundaries are tile boundaries and functions of seq_kv and
 * kv_splits alone.  kv_splits 0 lets the library choose, by a rule that is a pure function of the call's integer arguments (never of a
 * queried device property); brn_flash_attention_splitkv_plan returns the S, tps and workspace size a call will use, without a device,
 * and the explicit kv_splits = S repeats the bits.
 * workspace: where `loc` says, workspace_floats >= S * R * (head_dim + 1) floats with R = batch * heads * seq_q; NULL / 0 is allowed when
 * S == 1 (it is then not touched).  On return it holds the partials, and the layout is part of the contract:
 *   O_part[s][r][d] at float (s * R + r) * head_dim + d, then lse2_part[s][r] at float S * R * head_dim + s * R + r, r = (b * heads + h) * seq_q + i.
 * O_part[s][r] is the softmax-weighted V over the keys of split s alone, normalised; lse2_part[s][r] is m + log2(l) of that split in the
 * kernels' base-2 domain (scores times scale * log2 e).  A row with no visible key in split s (under the causal mask) gets O_part = 0
 * and lse2_part = -inf.  Floats past S * R * (head_dim + 1) are not touched.
 * The promise: no atomics; the partials of a row are combined in the fixed order s = 0 .. S - 1; a row's bits depend only on its own
 * (batch entry, query head), seq_kv, the mask and tps, neither on `batch` nor on the launch grid nor on which rows share its workgroup;
 * a repeated call repeats its bits; with S == 1 the result carries the bits of brn_flash_attention_gqa_forward.  With BRN_MEM_DEVICE the
 * call allocates nothing and does not synchronise the stream (unlike brn_flash_attention_varlen_forward, whose table upload does both):
 * it may be captured into a graph.
 * Limits (each violation is BRN_ERR_INVALID_ARG with the prefix "flash attention splitkv:" and a message naming the limit, checked before
 * the device): every limit of brn_flash_attention_gqa_forward without a bias; 0 <= kv_splits <= 1024; workspace not NULL and
 * workspace_floats large enough when S > 1 (the message names the float count needed); batch * kv_heads * ceil(G * seq_q / 64) * S < 2^31;
 * y, lse and workspace overlap neither each other nor an input; BRN_MEM_DEVICE pointers 16-byte aligned.
 * Not provided: a bias; packed or paged K / V; 16-bit tensors at the boundary; a split for the four older entries.  (Paged K / V with
 * per-sequence lengths on the device is brn_flash_attention_paged_forward below; a bf16 / fp16 K / V pool is
 * brn_flash_attention_paged_kv_forward, and writing new keys into a pool brn_kv_cache_append.) */
brn_status brn_flash_attention_splitkv_plan(int batch, int seq_q, int seq_kv, int heads, int kv_heads, int head_dim,
                                            int kv_splits, int* splits_out, int* tiles_per_split_out,
                                            size_t* workspace_floats_out);
brn_status brn_flash_attention_splitkv_forward(const float* q, const float* k, const float* v,
                                               int batch, int seq_q, int seq_kv, int heads, int kv_heads, int head_dim,
                                               int layout, int causal, float scale, int kv_splits,
                                               float* y, float* lse, float* workspace, size_t workspace_floats,
                                               brn_mem loc, int device_ordinal, void* stream);
/* brn_flash_attention_splitkv_forward over a PAGED K / V cache with per-sequence lengths that live on the device: the decode entry of a
 * serving batch, whose sequences have different lengths and keep their keys in fixed-size pages of a shared pool.
 *   y[b,h] = softmax over the visible keys j < len_b of batch entry b( scale * q[b,h] k_b[j, h / G]^T ) v_b[j, h / G],   lse as in the split entry
 * q, y, layout, G = heads / kv_heads, scale, lse ([batch, heads, seq_q], or NULL), workspace and kv_splits are exactly those of
 * brn_flash_attention_splitkv_forward.
 * k_pages, v_pages: [n_pages, page_size, kv_heads, head_dim] fp32, contiguous, where `loc` says; page_size 16, 32, 64, 128 or 256.  Offsets
 * into the pool are 64-bit: a pool may hold more than 2^31 floats.
 * block_table: [batch, max_pages] int32 where `loc` says.  Key j of batch entry b is row j % page_size of page block_table[b][j / page_size].
 * kv_lens: [batch] int32 where `loc` says; len_b = kv_lens[b] keys of batch entry b take part.  The kernels read both arrays as device
 * data: the host never reads them for BRN_MEM_DEVICE (for BRN_MEM_HOST they are staged like the float operands), so their values cannot
 * be validated before the launch and are made harmless instead:
 *   kv_lens[b] is used as min(max(kv_lens[b], 0), max_kv_len); a page number is used as min(max(page, 0), n_pages - 1);
 * no address in a kernel depends on either value other than through these clamps.  An out-of-range length therefore means max_kv_len (or
 * 0), an out-of-range page number means the last (or the first) page of the pool: a wrong result for that sequence, never an access
 * outside the pool or the table.  A table entry at or past ceil(len_b / page_size) of its sequence is never used to form an address, and
 * rows of a page at or past len_b are never read into the arithmetic: they, and every page no used entry names, may hold anything (NaN
 * included).
 * The mask: causal 0, the keys 0 .. len_b - 1; causal 1, key j takes part in query i's row exactly when j <= i + len_b - seq_q: the gqa
 * entry's mask, ending at the sequence's own last key.  len_b >= seq_q cannot be required of device data, so a row with no visible key
 * is defined: y = 0 (exact zeros) and lse = -inf, no NaN anywhere.  That covers len_b == 0 and causal rows with i + len_b - seq_q < 0.
 * The split and the workspace are brn_flash_attention_splitkv_plan(batch, seq_q, max_kv_len, heads, kv_heads, head_dim, kv_splits):
 * nkt = ceil(max_kv_len / 64), split s owns tiles s * tps .. min((s + 1) * tps, nkt) - 1 of every sequence; the grid and the split are
 * sized by max_kv_len, an upper bound the host knows, and a split that starts at or past a sequence's (causal) end writes the empty
 * markers O_part = 0 and lse2_part = -inf.  O_part / lse2_part keep the layout and meaning of the split entry; S == 1 writes y and lse
 * directly and touches no workspace.
 * The promise: no atomics; the partials of a row are combined in the fixed order s = 0 .. S - 1; a row's bits depend only on its own q
 * row, the keys and values of its sequence in logical order, len_b, the mask and tps: not on which physical pages hold the keys, not
 * on page_size, n_pages, max_pages, `batch`, the other sequences' lengths, the launch grid or which rows share its workgroup; a repeated
 * call repeats its bits.  With BRN_MEM_DEVICE the call allocates nothing, does not synchronise the stream and may be captured into a
 * graph; changing kv_lens, block_table and the pool contents between replays is the intended use.  For a sequence the split entry accepts
 * (len_b >= 1; causal: len_b >= seq_q) the row carries the bits of brn_flash_attention_splitkv_forward on that sequence's keys gathered
 * into a dense tensor with seq_kv = len_b, whenever both calls walk the same tile ranges (the same tps, or one split holding all of it).
 * Limits (each violation is BRN_ERR_INVALID_ARG with the prefix "flash attention paged:" and a message naming the limit, checked before
 * the device): every limit of brn_flash_attention_splitkv_forward with max_kv_len in the place of seq_kv, except that causal does not
 * require max_kv_len >= seq_q (a per-sequence matter, defined above); block_table and kv_lens not NULL; page_size 16, 32, 64, 128 or
 * 256; n_pages >= 1, max_pages >= 1, n_pages * page_size < 2^31; 1 <= max_kv_len <= min(65536, max_pages * page_size); y, lse and
 * workspace overlap neither each other nor any of the five inputs (sizes in bytes: the table and the lengths are ints); BRN_MEM_DEVICE
 * pointers 16-byte aligned, the two int arrays 4-byte aligned.
 * Not provided: a bias; a window; 16-bit or quantised pages (bf16 / fp16 pages are brn_flash_attention_paged_kv_forward below; quantised
 * ones nowhere); a K-transposed page layout; appending to the cache (brn_kv_cache_append below writes new keys into the pool). */
brn_status brn_flash_attention_paged_forward(const float* q, const float* k_pages, const float* v_pages,
                                             const int* block_table, const int* kv_lens,
                                             int batch, int seq_q, int max_kv_len, int heads, int kv_heads, int head_dim,
                                             int n_pages, int page_size, int max_pages,
                                             int layout, int causal, float scale, int kv_splits,
                                             float* y, float* lse, float* workspace, size_t workspace_floats,
                                             brn_mem loc, int device_ordinal, void* stream);
/* The element type of a K / V pool.  bf16 and fp16 pools hold the 16-bit patterns of their elements. */
typedef enum { BRN_KV_F32 = 0, BRN_KV_BF16 = 1, BRN_KV_F16 = 2 } brn_kv_type;
/* brn_flash_attention_paged_forward over a pool stored in fp32, bf16 or fp16: a decode call's cost is the K / V bytes it reads, and a
 * 16-bit pool holds twice the tokens and moves half the bytes.  Semantics, mask, clamps, plan, workspace layout, the defined empty row
 * (y = 0, lse = -inf), the promise (allocates nothing, does not synchronise, may be captured) and every limit are those of
 * brn_flash_attention_paged_forward; the arguments after kv_type are its arguments after v_pages, in its order.  What differs:
 * k_pages, v_pages: [n_pages, page_size, kv_heads, head_dim] of the type kv_type (a brn_kv_type) names, where `loc` says.  q, y, lse and
 * the workspace stay fp32.  BRN_KV_F32 runs brn_flash_attention_paged_forward's path and returns its bits.
 * Which arithmetic (brn_set_op_compute, as in every attention entry) reads which pool: BRN_BF16 reads a bf16 pool and BRN_F16 an f16 pool,
 * on the 16-bit kernels, and the elements go to the matrix instructions as stored, with no conversion; BRN_F32 and the three plane modes
 * read either 16-bit pool on the exact fp32 kernel, widening each element exactly.  A bf16 pool in mode BRN_F16, or the reverse, is
 * refused with a message that names both types: nothing is re-rounded silently.
 * The promise added: a row carries the bits of brn_flash_attention_paged_forward in the same compute mode on the pool widened to fp32
 * (y, lse and the partials in the workspace), because the 16-bit kernels round an fp32 pool to the type the 16-bit pool already holds.
 * Limits (each violation is BRN_ERR_INVALID_ARG with the prefix "flash attention paged kv:" and a message naming the limit, checked
 * before the device): every limit of brn_flash_attention_paged_forward; kv_type one of the three; the pairing of pool and compute mode
 * above; BRN_MEM_DEVICE k_pages / v_pages 16-byte aligned whatever the type; the overlap rules count bytes.
 * Not provided: fp8 / int8 or otherwise scaled pages (e4m3 pages with one scale per K / V head are brn_flash_attention_paged_fp8_forward
 * below; int8 nowhere); a K-transposed page layout; 16-bit q / y; 16-bit tensors for the dense, split and varlen entries; a window or a bias. */
brn_status brn_flash_attention_paged_kv_forward(const float* q, const void* k_pages, const void* v_pages, int kv_type,
                                                const int* block_table, const int* kv_lens,
                                                int batch, int seq_q, int max_kv_len, int heads, int kv_heads, int head_dim,
                                                int n_pages, int page_size, int max_pages,
                                                int layout, int causal, float scale, int kv_splits,
                                                float* y, float* lse, float* workspace, size_t workspace_floats,
                                                brn_mem loc, int device_ordinal, void* stream);
/* Appends seq_new new tokens to every sequence of a paged K / V cache (the pool, block table and lengths of the two paged attention
 * entries) and moves the lengths on, all on the device: an append with kv_lens_out = kv_lens followed by a paged attention call is one
 * whole decode step, and one captured graph.
 * k_new, v_new: fp32, [batch, seq_new, kv_heads, head_dim] (layout BRN_ATTN_BSHD) or [batch, kv_heads, seq_new, head_dim] (BRN_ATTN_BHSD).
 * k_pages, v_pages: the pool, [n_pages, page_size, kv_heads, head_dim] of kv_type (any brn_kv_type; BRN_KV_F32 is a plain scatter),
 * written in place.  block_table [batch, max_pages] and kv_lens [batch]: int32, read as device data and clamped, never trusted.
 * The rule: with cap = max_pages * page_size and L_b = min(max(kv_lens[b], 0), cap), token t of batch entry b becomes key L_b + t of
 * sequence b: row (L_b + t) % page_size of page min(max(block_table[b][(L_b + t) / page_size], 0), n_pages - 1).  A token whose position
 * is >= cap is dropped: nothing is written for it and no table entry is read for it.  No other row of the pool is written.
 * kv_lens_out: [batch] int32 or NULL; it receives min(L_b + seq_new, cap).  It may be kv_lens itself: the lengths are written by a launch
 * of their own after the rows, so the in-place form is well defined.  With NULL, kv_lens is left as it is.
 * Two sequences whose tables name the same page at a written position are the caller's error: the content of that page is then
 * unspecified, and nothing outside the pool is touched.
 * Conversion: the cast the attention kernels apply to an fp32 pool, round to nearest even.  An element appended to a 16-bit pool is bit for
 * bit what the fp32-pool kernel of that compute mode would have fed the matrix instructions, so append + attention over the 16-bit pool
 * gives the bits of brn_flash_attention_paged_forward in that mode on an fp32 pool of the unrounded keys.  A value beyond the fp16 range
 * becomes +-inf in an f16 pool, a NaN stays a NaN: documented, not trapped.
 * With BRN_MEM_DEVICE the call allocates nothing, does not synchronise the stream and may be captured.  BRN_MEM_HOST is a test
 * convenience: the WHOLE pool is staged to the device and copied back whole.
 * Limits (BRN_ERR_INVALID_ARG, prefix "kv cache append:", checked before the device): no NULL but kv_lens_out; kv_type one of the three;
 * head_dim 32, 64 or 128; batch >= 1, kv_heads >= 1; 1 <= seq_new <= 65536; layout 0 or 1; page_size 16, 32, 64, 128 or 256; n_pages >= 1,
 * max_pages >= 1, n_pages * page_size < 2^31, max_pages * page_size < 2^31; seq_new * kv_heads * head_dim / 8 < 2^31; k_new, v_new,
 * block_table and kv_lens do not overlap the pool, k_pages and v_pages not each other, kv_lens_out nothing but (wholly) kv_lens, sizes in
 * bytes; BRN_MEM_DEVICE k_new, v_new, k_pages, v_pages 16-byte aligned, the int arrays 4-byte aligned.
 * Not provided: a per-sequence number of new tokens (seq_new is one integer); copy-on-write or reference counting of shared pages;
 * scaled (fp8 / int8) pages (an e4m3 pool with per-head scales is written by brn_kv_cache_append_fp8 below). */
brn_status brn_kv_cache_append(const float* k_new, const float* v_new, int batch, int seq_new, int kv_heads, int head_dim, int layout,
                               void* k_pages, void* v_pages, int kv_type,
                               const int* block_table, const int* kv_lens, int* kv_lens_out,
                               int n_pages, int page_size, int max_pages,
                               brn_mem loc, int device_ordinal, void* stream);
/* brn_flash_attention_paged_forward over a pool stored in fp8 with one fp32 scale per K / V head: twice the tokens of a 16-bit pool in
 * the same memory and half its bytes on the rows that are bound by bytes.  Semantics, mask, clamps, plan, workspace layout, the defined
 * empty row (y = 0, lse = -inf), the promise (allocates nothing, does not synchronise, may be captured) and every limit are those of
 * brn_flash_attention_paged_forward; the arguments after kv_lens are its arguments after kv_lens, in its order.  What differs:
 * k_pages, v_pages: [n_pages, page_size, kv_heads, head_dim], one byte per element, OCP e4m3fn (the gfx950 format, not MI300's fnuz:
 * bias 7, largest value 448, no infinities, NaN = 0x7F / 0xFF), where `loc` says.  q, y, lse and the workspace stay fp32.
 * k_scale, v_scale: [kv_heads] fp32, where `loc` says; NULL means all ones.  Byte e of K head h stands for k_scale[h] * e4m3(e), byte e
 * of V head h for v_scale[h] * e4m3(e).  They are device data like the table and the lengths: the kernels read them, the host never does
 * for BRN_MEM_DEVICE, they may change between graph replays, and no address depends on them.  A scale that is not finite and positive
 * makes that head's results unspecified; it never causes an access outside the pool.
 * Every e4m3 value is a bf16, an fp16 and an fp32 value, so ONE fp8 pool is read by every compute mode (brn_set_op_compute): each byte is
 * widened exactly to the type the mode computes in, fp32 in the fp32-class modes, bf16 in BRN_BF16, fp16 in BRN_F16.
 * The promise added, for any finite positive scales, with s the call's resolved scale and g = h / G the K / V head of query head h: lse
 * and the partials in the workspace carry the bits of brn_flash_attention_paged_forward, in the same compute mode, on the fp32 pool that
 * holds the widened bytes, called with scale = fl32(s * k_scale[g]); y carries fl32(v_scale[g] * y of that call).  v_scale multiplies a
 * row's final y once, after normalisation; O_part / lse2_part are not scaled by it, and lse is the natural-log sum over the scaled scores.
 * Limits (each violation is BRN_ERR_INVALID_ARG with the prefix "flash attention paged fp8:" and a message naming the limit, checked
 * before the device): every limit of brn_flash_attention_paged_forward; BRN_MEM_DEVICE k_pages / v_pages 16-byte aligned, the two scale
 * arrays 4-byte aligned; the overlap rules count bytes and include the two scale arrays.
 * Not provided: computing scales (amax); per-page or per-token scales; e5m2; int8; fp8 q / y; the fp8 MFMA on the scores. */
brn_status brn_flash_attention_paged_fp8_forward(const float* q, const void* k_pages, const void* v_pages,
                                                 const float* k_scale, const float* v_scale,
                                                 const int* block_table, const int* kv_lens,
                                                 int batch, int seq_q, int max_kv_len, int heads, int kv_heads, int head_dim,
                                                 int n_pages, int page_size, int max_pages,
                                                 int layout, int causal, float scale, int kv_splits,
                                                 float* y, float* lse, float* workspace, size_t workspace_floats,
                                                 brn_mem loc, int device_ordinal, void* stream);
/* brn_kv_cache_append into the fp8 pool of brn_flash_attention_paged_fp8_forward.  The rule is brn_kv_cache_append's, unchanged: the
 * position rule, dropped positions, clamps, lengths written by a second launch, kv_lens_out in place; BRN_MEM_HOST stages the whole pool.
 * k_pages, v_pages: bytes of OCP e4m3fn; k_scale, v_scale: [kv_heads] fp32 where `loc` says, NULL = all ones, device data as above.
 * An element x of K head h is stored by three steps (V alike, with v_scale): t = x / k_scale[h], the correctly rounded fp32 division;
 * t clamped to +-448, a NaN kept; t rounded to nearest even into e4m3fn.  So a value beyond the range saturates to +-448 whatever the
 * conversion instruction does on overflow, +-0 and underflow keep their sign, and a NaN becomes a NaN byte (0x7F or 0xFF).
 * Limits (BRN_ERR_INVALID_ARG, prefix "kv cache append fp8:", checked before the device): every limit of brn_kv_cache_append but kv_type;
 * the scale arrays overlap neither the pool nor kv_lens_out, sizes in bytes; BRN_MEM_DEVICE scale arrays 4-byte aligned.
 * Not provided: computing scales (amax); per-page or per-token scales; e5m2; int8; a per-sequence number of new tokens. */
brn_status brn_kv_cache_append_fp8(const float* k_new, const float* v_new, int batch, int seq_new, int kv_heads, int head_dim, int layout,
                                   void* k_pages, void* v_pages, const float* k_scale, const float* v_scale,
                                   const int* block_table, const int* kv_lens, int* kv_lens_out,
                                   int n_pages, int page_size, int max_pages,
                                   brn_mem loc, int device_ordinal, void* stream);
/* Rotary position embedding: y = x with the first rot_dim elements of every head row rotated in pairs by the angles of the row's
 * position.  It is the step a decoder applies to q and to the new k before attention; with positions = kv_lens it rotates q at the
 * positions the new keys are about to take, on the device, so rope + brn_kv_cache_append_rope + paged attention is one captured graph.
 * x, y: fp32, [batch, seq, heads, head_dim] (layout BRN_ATTN_BSHD) or [batch, heads, seq, head_dim] (BRN_ATTN_BHSD).
 * The table: cos, sin are [n_pos, rot_dim / 2] fp32, contiguous, supplied by the caller, where `loc` says.  The library evaluates no sine
 * or cosine: every frequency-scaling scheme is a different table, and the result is promised bit for bit.
 * The rule, for a row x[0 .. head_dim) at table row p and i in 0 .. rot_dim / 2: style BRN_ROPE_HALF (NeoX / Llama) pairs a = x[i] with
 * b = x[i + rot_dim / 2], style BRN_ROPE_INTERLEAVED (GPT-J) pairs a = x[2i] with b = x[2i + 1]; the pair is written back to its two places as
 *   a' = fl(fl(a * cos[p][i]) - fl(b * sin[p][i])),   b' = fl(fl(b * cos[p][i]) + fl(a * sin[p][i])),
 * all in fp32: two rounded products, then one rounded difference or sum, never a fused multiply-add.  Elements d >= rot_dim are copied
 * with their bits (partial rotary), a NaN's payload included.
 * positions: [batch] int32 where `loc` says, or NULL = all 0.  They are device data and are clamped, never trusted: with
 * P_b = max(positions[b], 0), token t of batch entry b uses table row p = min(P_b + t, n_pos - 1), the sum formed without int32 overflow.
 * A position past the table reads the last row: a wrong rotation for that token, never a read outside the table.  No address depends on
 * a device value other than through this clamp.
 * y may be x itself, wholly (in place): both members of a pair are in one thread's registers before either is written.
 * With BRN_MEM_DEVICE the call allocates nothing, does not synchronise the stream and may be captured.
 * Limits (each violation is BRN_ERR_INVALID_ARG with the prefix "rope:" and a message naming the limit, checked before the device): x, y,
 * cos, sin not NULL; head_dim 32, 64 or 128; rot_dim a multiple of 16 with 16 <= rot_dim <= head_dim; style 0 or 1; 1 <= n_pos <= 2^24;
 * batch >= 1, heads >= 1; 1 <= seq <= 65536; layout 0 or 1; batch * seq * heads * head_dim / 8 < 2^31; y is x or does not overlap x; cos,
 * sin and positions do not overlap y, sizes in bytes; BRN_MEM_DEVICE x, y, cos, sin 16-byte aligned, positions 4-byte aligned.
 * Not provided: computing the table on the device; per-token position arrays (positions are P_b + t); rotating q inside the append
 * call; 16-bit x / y; rotation inside the attention kernels; a per-sequence seq_new. */
typedef enum { BRN_ROPE_HALF = 0, BRN_ROPE_INTERLEAVED = 1 } brn_rope_style;
brn_status brn_rope_forward(const float* x, int batch, int seq, int heads, int head_dim, int layout,
                            const float* cos, const float* sin, int n_pos, int rot_dim, int style,
                            const int* positions,
                            float* y, brn_mem loc, int device_ordinal, void* stream);
/* brn_kv_cache_append with the new keys rotated on their way into the pool: a key is read once, rotated in registers, rounded once and
 * written once.  It is brn_kv_cache_append in every respect (the arguments up to layout and from k_pages on are its arguments, in its
 * order) except that K token t of batch entry b is rotated by the rule of brn_rope_forward at P_b = L_b, the append's own clamped length:
 * table row min(L_b + t, n_pos - 1), the position the token takes in the cache.  The rotation is finished in fp32, then cast once.  V is
 * not rotated.  The position rule, the page clamp, dropped positions, kv_lens_out written by the later launch and the in-place form are
 * unchanged; cos, sin, n_pos, rot_dim and style are brn_rope_forward's.
 * The promise: for every pool type, the pool and kv_lens_out carry the bits of brn_kv_cache_append called on
 * k' = brn_rope_forward(k_new, positions = kv_lens).
 * Limits (BRN_ERR_INVALID_ARG, prefix "kv cache append rope:", checked before the device): every limit of brn_kv_cache_append; cos, sin
 * not NULL; rot_dim a multiple of 16 with 16 <= rot_dim <= head_dim; style 0 or 1; 1 <= n_pos <= 2^24; cos and sin overlap neither the
 * pool nor kv_lens_out, sizes in bytes; BRN_MEM_DEVICE cos, sin 16-byte aligned.
 * Not provided: computing the table on the device; per-token position arrays; rotating q inside the append call (brn_rope_forward with
 * positions = kv_lens, before the append); 16-bit k_new / v_new; rotation inside the attention kernels; a per-sequence seq_new. */
brn_status brn_kv_cache_append_rope(const float* k_new, const float* v_new, int batch, int seq_new, int kv_heads, int head_dim, int layout,
                                    const float* cos, const float* sin, int n_pos, int rot_dim, int style,
                                    void* k_pages, void* v_pages, int kv_type,
                                    const int* block_table, const int* kv_lens, int* kv_lens_out,
                                    int n_pages, int page_size, int max_pages,
                                    brn_mem loc, int device_ordinal, void* stream);
/* The same insertion into brn_kv_cache_append_fp8: K is rotated as above, in fp32, in front of the fp8 store's three steps (divide by the
 * head's scale, clamp to +-448, round to nearest even).  The pool and kv_lens_out carry the bits of brn_kv_cache_append_fp8 called on
 * k' = brn_rope_forward(k_new, positions = kv_lens).
 * Limits (BRN_ERR_INVALID_ARG, prefix "kv cache append rope fp8:", checked before the device): every limit of brn_kv_cache_append_fp8 and
 * the table limits of brn_kv_cache_append_rope.
 * Not provided: what brn_kv_cache_append_fp8 and brn_kv_cache_append_rope do not provide. */
brn_status brn_kv_cache_append_rope_fp8(const float* k_new, const float* v_new, int batch, int seq_new, int kv_heads, int head_dim, int layout,
                                        const float* cos, const float* sin, int n_pos, int rot_dim, int style,
                                        void* k_pages, void* v_pages, const float* k_scale, const float* v_scale,
                                        const int* block_table, const int* kv_lens, int* kv_lens_out,
                                        int n_pages, int page_size, int max_pages,
                                        brn_mem loc, int device_ordinal, void* stream);
/* The storage type of a K / V pool for the packed paged entries below: the three of brn_kv_type and the e4m3fn pool of the fp8 entries
 * in one argument.  (The older entries keep brn_kv_type and refuse 3.) */
typedef enum { BRN_POOL_F32 = 0, BRN_POOL_BF16 = 1, BRN_POOL_F16 = 2, BRN_POOL_E4M3 = 3 } brn_pool_type;
/* What brn_flash_attention_paged_varlen_forward and brn_kv_cache_append_varlen will use: host-only, a pure function of its integers,
 * like brn_flash_attention_splitkv_plan.  total_q is the CAPACITY of the pack in tokens, n_seqs its number of sequence slots.
 * With G = heads / kv_heads, T_max = (G * total_q + 63 * min(n_seqs, total_q)) / 64 bounds the row tiles of 64 packed rows of ANY pack of
 * at most total_q tokens in n_seqs sequences (sum_b ceil(G * n_b / 64) <= T_max: each of the at most min(n_seqs, total_q) sequences that
 * are not empty rounds up by less than one tile); the grid is sized by it.  nkt = ceil(max_kv_len / 64);
 * ask = kv_splits ? kv_splits : the automatic rule of brn_flash_attention_splitkv_plan on a base grid of kv_heads * T_max workgroups;
 * tps = ceil(nkt / ask), S = ceil(nkt / tps): tps depends on max_kv_len and kv_splits alone when kv_splits is given.
 * workspace_floats = S * R * (head_dim + 1), R = heads * total_q (not needed and not touched when S == 1).  plan_ints: the int32 count of
 * plan_workspace, the device-side plan both entries write before they use it; its inner layout is not part of the contract.  The
 * append entry needs the same plan_ints (it depends on n_seqs alone).  Any out pointer may be NULL.
 * Limits: those of brn_flash_attention_paged_varlen_forward that concern these integers, under its prefix. */
brn_status brn_flash_attention_paged_varlen_plan(int total_q, int n_seqs, int max_kv_len, int heads, int kv_heads, int head_dim, int kv_splits,
                                                 int* splits_out, int* tiles_per_split_out, size_t* workspace_floats_out, size_t* plan_ints_out);
/* Paged attention over a PACKED batch of new tokens: one call for a serving step that mixes decode sequences (one new token), prefill
 * chunks (hundreds, over a prefix already in the cache) and idle slots, with every per-sequence number on the device.
 * q, y: [total_q, heads, head_dim] fp32, packed like brn_flash_attention_varlen_forward's.  lse: [heads, total_q] fp32 or NULL, heads-major.
 * The pool, block_table [n_seqs, max_pages], kv_lens [n_seqs] and the scales are exactly those of brn_flash_attention_paged_kv_forward /
 * brn_flash_attention_paged_fp8_forward, pool_type (a brn_pool_type) naming the storage; k_scale and v_scale must be NULL unless
 * pool_type is BRN_POOL_E4M3.  The pairing of pool and compute mode is the kv entry's (a 16-bit mode reads a 16-bit pool of its own
 * type; every mode reads an fp32 or an e4m3 pool).
 * total_q is a capacity.  cu_seqlens_q: [n_seqs + 1] int32 where `loc` says, device data like the table and the lengths: never read by
 * the host for BRN_MEM_DEVICE, and made harmless instead of validated.  The clamp rule: with c_i = min(max(cu_seqlens_q[i], 0), total_q),
 * s_b is the running maximum of c_i over i <= b; sequence b owns tokens s_b .. s_{b+1} - 1, n_b = s_{b+1} - s_b.  The sequences are
 * therefore disjoint and ordered whatever the array holds.  The padding rule: tokens outside [s_0, s_{n_seqs}) are padding; their rows
 * of y, lse and the partials are not written by any kernel of the call, the combine included.
 * Sequence b, with len_b = min(max(kv_lens[b], 0), max_kv_len) (the length AFTER its new keys were appended): its rows are those of the
 * paged entry with seq_q = n_b.  causal 0: a row sees keys 0 .. len_b - 1.  causal 1: key j is visible to the sequence's query i exactly
 * when j <= i + len_b - n_b.  A row with no visible key gets y = 0 (exact zeros) and lse = -inf.  A sequence with n_b == 0 costs nothing,
 * and no table entry of it is read.
 * The split is that of brn_flash_attention_paged_varlen_plan.  Partials sit at row r = h * total_q + token of O_part[s] / lse2_part[s]:
 * the split entry's layout at batch 1, seq_q = total_q.  S == 1 touches no float workspace.  No atomics; the combine order is s = 0 .. S - 1.
 * The promise: a sequence's rows carry the bits of brn_flash_attention_paged_forward / _kv_forward / _fp8_forward in the same compute
 * mode, for y, lse and the partials of the splits that call has, where that call is made with batch = 1, seq_q = n_b, that sequence's
 * table row and length, the same max_kv_len and the same explicit kv_splits.  The bits depend on none of the other sequences, neither
 * on n_seqs nor on total_q, on no physical page and on no old workspace content.  With BRN_MEM_DEVICE the call allocates nothing, does
 * not synchronise the stream and may be captured; changing cu_seqlens_q, kv_lens, the table and the pool between replays is the
 * intended use.  (BRN_MEM_HOST, a test convenience, stages y, lse and the workspace up as well as down, so padding rows come back as they went.)
 * Limits (each violation is BRN_ERR_INVALID_ARG with the prefix "flash attention paged varlen:" and a message naming the limit, checked
 * before the device): no NULL but lse, the scales and (S == 1) workspace; pool_type one of the four, the scales and the pairing above;
 * head_dim 32, 64 or 128; heads >= 1, 1 <= kv_heads <= heads, heads % kv_heads == 0; 1 <= n_seqs <= 65536; total_q >= 1;
 * G * total_q < 2^31; T_max * kv_heads * S < 2^31; page_size 16, 32, 64, 128 or 256; n_pages >= 1, max_pages >= 1, n_pages * page_size
 * < 2^31; 1 <= max_kv_len <= min(65536, max_pages * page_size); 0 <= kv_splits <= 1024; causal 0 or 1; scale finite and >= 0; the
 * workspace large enough when S > 1; plan_workspace present, 4-byte aligned and of at least plan_ints ints (the message names the count);
 * y, lse, workspace and plan_workspace overlap neither each other nor any input, sizes in bytes; BRN_MEM_DEVICE float pointers and
 * pools 16-byte aligned, int and scale arrays 4-byte aligned.
 * Not provided: a window or a bias; fused rope (the recipe is below); the BHSD layout; 16-bit q / y; copy-on-write of shared pages. */
brn_status brn_flash_attention_paged_varlen_forward(const float* q, const void* k_pages, const void* v_pages, int pool_type,
                                                    const float* k_scale, const float* v_scale,
                                                    const int* block_table, const int* kv_lens, const int* cu_seqlens_q,
                                                    int total_q, int n_seqs, int max_kv_len, int heads, int kv_heads, int head_dim,
                                                    int n_pages, int page_size, int max_pages,
                                                    int causal, float scale, int kv_splits,
                                                    float* y, float* lse, float* workspace, size_t workspace_floats,
                                                    int* plan_workspace, size_t plan_ints,
                                                    brn_mem loc, int device_ordinal, void* stream);
/* brn_kv_cache_append / brn_kv_cache_append_fp8 for a packed batch: every sequence brings its own number of new tokens, known on the
 * device alone.  k_new, v_new: [total_q, kv_heads, head_dim] fp32.  cu_seqlens_q is read through the clamp rule above (running maximum
 * of the values clamped to 0 .. total_q).  Token t of sequence b (packed token s_b + t) becomes key L_b + t by the position rule of
 * brn_kv_cache_append: L_b = min(max(kv_lens[b], 0), cap), cap = max_pages * page_size, positions at or past cap dropped, the page
 * number clamped.  kv_lens_out[b] = min(L_b + n_b, cap), written by a later launch, so kv_lens_out may be kv_lens itself; NULL = not
 * wanted.  Padding tokens write nothing.  Conversion per pool_type is that of brn_kv_cache_append / brn_kv_cache_append_fp8 (scales NULL
 * unless BRN_POOL_E4M3).  plan_workspace / plan_ints: as above, from brn_flash_attention_paged_varlen_plan.
 * The promise: the pool and kv_lens_out carry the bits of the existing append entry of that pool type called per sequence with
 * batch = 1, seq_new = n_b.  With BRN_MEM_DEVICE the call allocates nothing, does not synchronise and may be captured.
 * No rope is fused.  The recipe: call brn_rope_forward with batch = total_q, seq = 1 and a per-token positions array (the position each
 * token takes in its sequence) on q and on k_new, then this append: the pool then holds the bits of brn_kv_cache_append_rope per sequence.
 * Limits (BRN_ERR_INVALID_ARG, prefix "kv cache append varlen:", checked before the device): no NULL but kv_lens_out and the scales;
 * pool_type one of the four, scales with BRN_POOL_E4M3 alone; head_dim 32, 64 or 128; kv_heads >= 1; 1 <= n_seqs <= 65536; total_q >= 1;
 * page_size 16, 32, 64, 128 or 256; n_pages >= 1, max_pages >= 1, n_pages * page_size < 2^31, max_pages * page_size < 2^31; plan_workspace
 * present, 4-byte aligned and of at least plan_ints ints; no input and not plan_workspace overlaps the pool, k_pages and v_pages not each
 * other, kv_lens_out nothing but (wholly) kv_lens, plan_workspace nothing, sizes in bytes; BRN_MEM_DEVICE k_new, v_new, k_pages, v_pages
 * 16-byte aligned, int and scale arrays 4-byte aligned.
 * Not provided: a window or a bias; fused rope; the BHSD layout; 16-bit k_new / v_new; copy-on-write of shared pages. */
brn_status brn_kv_cache_append_varlen(const float* k_new, const float* v_new, const int* cu_seqlens_q, int total_q, int n_seqs,
                                      int kv_heads, int head_dim, void* k_pages, void* v_pages, int pool_type,
                                      const float* k_scale, const float* v_scale,
                                      const int* block_table, const int* kv_lens, int* kv_lens_out,
                                      int n_pages, int page_size, int max_pages,
                                      int* plan_workspace, size_t plan_ints,
                                      brn_mem loc, int device_ordinal, void* stream);
/* PatchMerging::forward (swin.rs:491-527): x [B,H*W,C] -> [B, ceil(H/2)*ceil(W/2), 2C]. */
brn_status brn_patch_merging_forward(const float* x, int B, int H, int W, int C, const float* norm_g,
                                     const float* norm_b, const float* reduction_w, float* y, brn_mem loc,
                                     int device_ordinal, void* stream);
/* DeformableConv2d::forward (deform_conv.rs:82-99 / :101-215), NCHW.  mode = brn_deform_mode.  Runs in the arithmetic selected with
 * brn_set_op_compute, like brn_conv2d_forward: in BRN_F32_SPLIT3 / BRN_F32_SPLIT2 / BRN_F32_HALF2 the offset / modulator conv and the
 * modulated gather x weights both multiply that mode's planes (the gather itself — bilinear blend x modulator — is fp32).
 * offset_w [2k^2,C,k,k]+offset_b, mod_w [k^2,C,k,k]+mod_b, w [O,C,k,k], bias [O] or NULL. */
brn_status brn_deform_conv2d_forward(const float* x, int B, int C, int H, int W,
                                     const float* offset_w, const float* offset_b,
                                     const float* mod_w, const float* mod_b,
                                     const float* w, const float* bias, int O, int k, int stride, int pad,
                                     int mode, float* y, brn_mem loc, int device_ordinal, void* stream);
/* The deformable convolution itself, with the CALLER's offsets and mask: torchvision deform_conv2d semantics, the operation
 * the reference configures through DeformConv2dConfig::new (deform_conv.rs:120-132) and runs as call_deformable_im2col + matmul
 * (deform_conv.rs:101-215, aspp.rs:58-165).  brn_deform_conv2d_forward is the layer around it (offsets and modulator from its own two convs,
 * square kernel, one stride / pad, dilation 1, one offset group, always a mask); this entry takes every parameter of the config.
 *   x [B,C,H,W], offset [B, 2*G*kh*kw, Ho, Wo], mask [B, G*kh*kw, Ho, Wo] or NULL (no modulation: DCNv1, use_mask false), y [B,O,Ho,Wo]
 *   live where `loc` says; w [O,C,kh,kw] and bias [O] (or NULL) are host pointers.  G = offset_groups.
 *   Ho = (H + 2 pad_h - dil_h (kh - 1) - 1) / stride_h + 1, Wo likewise.
 *   Offset channel 2 (g kh kw + t) is dy and the next one dx of tap t = ky kw + kx; input channel c belongs to group c / (C / G).
 *   Output pixel (oy, ox) samples at (oy stride_h - pad_h + ky dil_h + dy, ox stride_w - pad_w + kx dil_w + dx): bilinear from the floor,
 *   zero unless the point lies in (-1, H) x (-1, W), corners outside the image contribute zero.  The mask is the multiplier itself (no
 *   sigmoid is applied).  An infinite, NaN or huge offset makes its sample contribute 0 or NaN and nothing else: no address depends on it.
 * Arithmetic by brn_set_op_compute, like brn_deform_conv2d_forward: the blend mask x bilinear is fp32 in every mode, the product with w
 * runs on the mode's matrix path (in BRN_BF16 / BRN_F16 x and w are rounded to the 16-bit type); offsets and mask stay fp32 in every mode.
 * Two routes, chosen by the geometry alone: with G == 1 and equal stride, pad and dilation on both axes the gather kernels the layer
 * uses (given the layer's offsets as a tensor and no mask where its modulator is 1, the layer's bits); everything else as a column
 * matrix (bounded by BRN_DEFORM_COL_MB MiB, walked in chunks of rows) times the mode's dense GEMM.
 * Limits (each violation is BRN_ERR_INVALID_ARG with the prefix "deform conv offsets:" and a message naming the limit, checked before
 * the device): x, offset, w, y non-NULL; every size, stride and dilation >= 1, pads >= 0; G >= 1 and C % G == 0; H + 2 pad_h and
 * W + 2 pad_w < 2^31; Ho, Wo >= 1; B * Ho * Wo and every buffer's element count < 2^31; y overlaps no input.
 * Not provided: weight groups (torchvision's `groups`; the reference multiplies the columns by one [O, C kh kw] weight, deform_conv.rs:101-215),
 * 16-bit tensors at the boundary, a backward pass. */
brn_status brn_deform_conv2d_offsets_forward(const float* x, int B, int C, int H, int W,
                                             const float* offset, const float* mask,
                                             const float* w, const float* bias, int O, int kh, int kw,
                                             int stride_h, int stride_w, int pad_h, int pad_w, int dil_h, int dil_w,
                                             int offset_groups,
                                             float* y, brn_mem loc, int device_ordinal, void* stream);

/* ASPPDeformable::new(in_channels, out_channels, vb.pp(prefix)) + forward (aspp.rs:236-333; BasicDecBlk builds it with
 * (64, None), decoder.rs:107-111): five branches on the map (aspp1 and aspp_deforms.{0,1,2} = DeformConvASPP k 1,1,3,7 -> 256, BN, ReLU;
 * global average pool -> 1x1 -> BN -> ReLU -> broadcast), concat 1280, conv1 1x1 (no bias) + bn1 + ReLU.  weights: the module's tensors
 * under `prefix` ("aspp1.atrous_conv.offset_conv.weight", ..., "conv1.weight", "bn1.*"; SURVEY.md App. A <ASPP>); mode =
 * brn_deform_mode; out_channels 0 = None = in_channels (aspp.rs:242).  x [B,in_channels,H,W] -> y [B,out_channels,H,W], NCHW; any widths. */
brn_status brn_aspp_deformable_forward(const brn_named_tensor* weights, size_t n_weights, const char* prefix, int in_channels,
                                       int out_channels, int mode, const float* x, int B, int H, int W, float* y, brn_mem loc,
                                       int device_ordinal, void* stream);

/* BasicDecBlk::new(in_channels, out_channels, &DecoderConfig, vb.pp(prefix)) + forward (decoder.rs:78-141), the block behind
 * SqueezeModule and decoder_block{4,3,2,1}: conv_in 3x3 (in_channels -> 64, bias) + bn_in + ReLU -> ASPPDeformable(64) (use_aspp != 0:
 * DecoderConfig::use_aspp_deformable, decoder.rs:107-111; 0 = dec_att is None) -> conv_out 3x3 (64 -> out_channels, bias) + bn_out (no
 * ReLU).  inter_channels: 64 (DecoderConfig::default(), what BiRefNet builds) or in_channels / 4 (inter_channels_adaptive,
 * decoder.rs:94-98); 0 = 64.
 * weights: "conv_in.weight|bias", "bn_in.*", "dec_att.<ASPP>", "conv_out.weight|bias", "bn_out.*" under `prefix` (SURVEY.md App. A
 * <DecBlk>); mode = brn_deform_mode.  x [B,in_channels,H,W] -> y [B,out_channels,H,W], NCHW; any widths (maps are padded to the
 * kernels' channel granule inside). */
brn_status brn_decblk_forward(const brn_named_tensor* weights, size_t n_weights, const char* prefix, int in_channels,
                              int out_channels, int inter_channels, int use_aspp, int mode, const float* x, int B, int H, int W,
                              float* y, brn_mem loc, int device_ordinal, void* stream);

/* ---- image pre/post-processing: the steps either side of forward_logits in examples/infer_image.rs ------ */
/* infer_image.rs:44-67.  `img.resize_exact(S, S, FilterType::Triangle)` -> `to_rgb8()` -> (v/255 - mean) / std with the
 * ImageNet constants of :53-54 -> x [3,S,S] fp32 (NCHW, one image).  pixels: host, interleaved RGB8 or RGBA8 (channels 3|4;
 * alpha is resampled like the crate does and then dropped by to_rgb8), row-major [h][w][channels].  The resampler restates
 * image 0.25.9 (Cargo.lock:1102; imageops/sample.rs: vertical pass into f32, horizontal pass with clamp + round-to-nearest
 * into u8, per-output weight tables normalised by their sum) — that crate is not vendored in the reference tree. */
brn_status brn_preprocess_image(const unsigned char* pixels, int h, int w, int channels, int S,
                                float* x_nchw_out, brn_mem out_loc, int device_ordinal, void* stream);
/* infer_image.rs:84-110.  logits [S,S] -> sigmoid (apply_sigmoid != 0; pass 0 for brn_forward's output) ->
 * `(v * 255.0).clamp(0.0, 255.0) as u8` -> `imageops::resize(&mask, out_w, out_h, FilterType::Lanczos3)` -> mask
 * [out_h][out_w] u8 on the host. */
brn_status brn_postprocess_mask(const float* logits, int S, brn_mem in_loc, int apply_sigmoid, int out_h, int out_w,
                                unsigned char* mask_out, int device_ordinal, void* stream);

/* examples/infer_image.rs:44-110 for a BATCH, end to end on the device: n images (host, RGB8 / RGBA8, each its own size) ->
 * resize_exact(S, S, Triangle) + ImageNet normalisation -> forward() (sigmoid fused) of the whole batch -> `as u8` -> resize back to each
 * image's own size (Lanczos3) -> n masks on the host (masks[i]: heights[i] x widths[i] bytes).  One call: the uploads, 4 small kernels
 * per image, ONE forward of batch n, the downloads; no allocation after the first call of a shape (the staging buffers and the
 * resampling tables live with the model handle and are reused), one stream synchronisation at the end.  Results are bit-identical to
 * brn_preprocess_image -> brn_forward -> brn_postprocess_mask image by image when the forward runs the same batch. */
brn_status brn_infer_images_u8(brn_model* m, int n, const unsigned char* const* pixels, const int* heights, const int* widths,
                               int channels, int S, unsigned char* const* masks, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* BIREFNET_HIP_H */
