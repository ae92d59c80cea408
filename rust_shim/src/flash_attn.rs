//! The three attention calls of the reference's `flash-attn` dependency over the library's two attention entry points: the narrow seam.
//!
//! `WindowAttention::forward` makes two of them behind its `flash-attn` feature (src/swin.rs:243, 252), served by `brn_attention_forward`
//! (N <= 144, head_dim 32, not causal: the Swin windows of 7 and 12) and by `brn_flash_attention_bias_forward` (everything else).
//! A `hip` feature beside `flash-attn` at swin.rs:226-258 keeps candle's `WindowAttention` (qkv, cached_bias, mask, proj) and swaps only
//! these calls:
//!
//!   #[cfg(feature = "hip")]
//!   use candle_birefnet_hip::flash_attn::{flash_attention_with_bias, flash_attention_with_repeating_bias};
//!
//! Same arguments, same pre-scaled bias (the bias is added to the UNSCALED scores, swin.rs:231-233), same `[batch, heads, N, head_dim]`
//! result.  Limits are the library's (include/birefnet_hip.h): head_dim 32 / 64 / 128, N up to 65536 (windows of 16 and 24 are N = 256
//! and 576), the `causal` flag honoured, -inf bias entries exclude their key; the bias is fp32, one slab per head (no broadcast over heads).
//! (A whole Swin block with such a window needs no seam: `crate::swin` and `brn_window_attention_forward` take window_size 2 ..= 32.)
//!
//! The third is the plain `flash_attention(&q, &k, &v, causal)` of examples/bench_flash_attn.rs:39-53 on `[batch, seq, heads, head_dim]`
//! tensors, served by `brn_flash_attention_forward`: head_dim 32 / 64 / 128, sequences up to 65536, q and k/v of different lengths, the
//! causal mask (which needs equal lengths), no bias.
use candle_core::{Result, Tensor};

use crate::hip_ffi as ffi;

/// y[b,h] = softmax(scale * (q k^T + bias[b % n_bias, h])) v, scale = head_dim^-0.5; tensors travel as host buffers
fn attention(q: &Tensor, k: &Tensor, v: &Tensor, bias: &Tensor, n_bias: usize, causal: bool) -> Result<Tensor> {
    let (batch, heads, n, head_dim) = q.dims4()?;
    if k.dims4()? != (batch, heads, n, head_dim) || v.dims4()? != (batch, heads, n, head_dim) {
        candle_core::bail!("q, k and v must share the shape [batch, heads, N, head_dim]")
    }
    let (nb, bh, bn0, bn1) = bias.dims4()?;
    if nb != n_bias || bh != heads || bn0 != n || bn1 != n {
        candle_core::bail!("bias must be [{n_bias}, {heads}, {n}, {n}], got {:?}", bias.dims())
    }
    let (qh, kh, vh, bhost) = (ffi::to_host(q)?, ffi::to_host(k)?, ffi::to_host(v)?, ffi::to_host(bias)?);
    let mut out = vec![0f32; batch * heads * n * head_dim];
    // the short op holds a whole score row in registers (the windows of 7 and 12); everything else walks K / V tiles with the bias beside them
    ffi::check(unsafe {
        if n <= 144 && head_dim == 32 && !causal {
            ffi::brn_attention_forward(qh.as_ptr(), kh.as_ptr(), vh.as_ptr(), batch as i32, heads as i32, n as i32, head_dim as i32, bhost.as_ptr(),
                                       n_bias as i32, 0.0, out.as_mut_ptr(), ffi::BRN_MEM_HOST, 0, std::ptr::null_mut())
        } else {
            ffi::brn_flash_attention_bias_forward(qh.as_ptr(), kh.as_ptr(), vh.as_ptr(), batch as i32, n as i32, n as i32, heads as i32,
                                                  head_dim as i32, ffi::BRN_ATTN_BHSD, causal as i32, bhost.as_ptr(), n_bias as i32, 0.0,
                                                  out.as_mut_ptr(), ffi::BRN_MEM_HOST, 0, std::ptr::null_mut())
        }
    })?;
    Tensor::from_vec(out, (batch, heads, n, head_dim), q.device())
}

/// `candle_mps_flash_attention::flash_attention_with_bias(&q, &k, &v, &scaled_bias, false)` (swin.rs:252): bias `[1 or batch, heads, N, N]`
pub fn flash_attention_with_bias(q: &Tensor, k: &Tensor, v: &Tensor, bias: &Tensor, causal: bool) -> Result<Tensor> {
    attention(q, k, v, bias, bias.dim(0)?, causal)
}

/// `candle_mps_flash_attention::flash_attention_with_repeating_bias(&q, &k, &v, &scaled_combined, n_windows, false)` (swin.rs:243): bias
/// `[n_windows, heads, N, N]`, batch entry b reads pattern b % n_windows (the window order of swin.rs:291-294)
pub fn flash_attention_with_repeating_bias(q: &Tensor, k: &Tensor, v: &Tensor, bias: &Tensor, n_windows: usize, causal: bool) -> Result<Tensor> {
    attention(q, k, v, bias, n_windows, causal)
}

/// `candle_mps_flash_attention::flash_attention(&q, &k, &v, causal)` (examples/bench_flash_attn.rs:45): q `[batch, seq_q, heads, head_dim]`,
/// k, v `[batch, seq_kv, heads, head_dim]` -> `[batch, seq_q, heads, head_dim]`; scale = head_dim^-0.5; tensors travel as host buffers
pub fn flash_attention(q: &Tensor, k: &Tensor, v: &Tensor, causal: bool) -> Result<Tensor> {
    let (batch, seq_q, heads, head_dim) = q.dims4()?;
    let (k_batch, seq_kv, k_heads, k_dim) = k.dims4()?;
    if (k_batch, k_heads, k_dim) != (batch, heads, head_dim) || v.dims4()? != (batch, seq_kv, heads, head_dim) {
        candle_core::bail!("q must be [batch, seq_q, heads, head_dim], k and v [batch, seq_kv, heads, head_dim]")
    }
    let (qh, kh, vh) = (ffi::to_host(q)?, ffi::to_host(k)?, ffi::to_host(v)?);
    let mut out = vec![0f32; batch * seq_q * heads * head_dim];
    ffi::check(unsafe {
        ffi::brn_flash_attention_forward(qh.as_ptr(), kh.as_ptr(), vh.as_ptr(), batch as i32, seq_q as i32, seq_kv as i32, heads as i32,
                                         head_dim as i32, ffi::BRN_ATTN_BSHD, causal as i32, 0.0, out.as_mut_ptr(), ffi::BRN_MEM_HOST, 0,
                                         std::ptr::null_mut())
    })?;
    Tensor::from_vec(out, (batch, seq_q, heads, head_dim), q.device())
}
