"""Op-level entry points of the C ABI (the candle ops the reference's hot path calls), used by the parity tests.
Weights are host arrays; activations may be numpy (host) or torch-on-GPU (device) tensors."""
import numpy as np

from . import _ffi
from . import tensors as T

_COMPUTE = {"f32": _ffi.BRN_F32, "f32_split3": _ffi.BRN_F32_SPLIT3, "f32_split2": _ffi.BRN_F32_SPLIT2, "f32_half2": _ffi.BRN_F32_HALF2, "bf16": _ffi.BRN_BF16, "f16": _ffi.BRN_F16}


def set_compute(mode: str):
    """contraction arithmetic of ops.linear / ops.conv2d on this thread (include/birefnet_hip.h brn_dtype)"""
    _ffi.check(_ffi.lib.brn_set_op_compute(_COMPUTE[mode]))


_ACT = {None: _ffi.BRN_ACT_NONE, "none": _ffi.BRN_ACT_NONE, "relu": _ffi.BRN_ACT_RELU, "gelu_erf": _ffi.BRN_ACT_GELU_ERF}


def linear(x, w, bias=None, act=None, residual=None, device=0):
    """candle_nn::linear(+gelu_erf)(+residual): x [M,K], w [N,K] -> [M,N]  (swin.rs:98-107,130-131)."""
    M, K = (int(v) for v in x.shape)
    N = int(w.shape[0])
    px, loc, keep, _ = T.as_arg(x)
    pr, rloc, rkeep, _ = T.as_arg(residual, (M, N)) if residual is not None else (None, loc, None, None)
    if residual is not None and rloc != loc:
        raise ValueError("x and residual must live on the same side")
    pw, kw = T.host_ptr(w)
    pb, kb = T.host_ptr(bias)
    y = T.alloc_like(keep, (M, N))
    _ffi.check(_ffi.lib.brn_linear_forward(px, M, K, pw, pb, N, _ACT[act], pr, T.ptr_of(y), loc, T.device_of(keep, device),
                                           T.stream_of(keep)))
    return y


def layer_norm(x, gamma, beta, eps=1e-5, device=0):
    """candle_nn::layer_norm forward over the last dim (swin.rs:333)."""
    C = int(x.shape[-1])
    rows = 1
    for v in x.shape[:-1]:
        rows *= int(v)
    px, loc, keep, _ = T.as_arg(x)
    pg, kg = T.host_ptr(gamma)
    pb, kb = T.host_ptr(beta)
    y = T.alloc_like(keep, tuple(x.shape))
    _ffi.check(_ffi.lib.brn_layer_norm_forward(px, rows, C, pg, pb, float(eps), T.ptr_of(y), loc, T.device_of(keep, device),
                                               T.stream_of(keep)))
    return y


def conv2d(x, w, bias=None, stride=1, padding=0, dilation=1, bn=None, bn_eps=1e-5, act=None, device=0):
    """candle_nn::conv2d (NCHW) with optional eval-mode batch_norm (gamma, beta, running_mean, running_var) + activation."""
    B, Cc, H, W = (int(v) for v in x.shape)
    O, Ci, kh, kw = (int(v) for v in w.shape)
    if Ci != Cc:
        raise ValueError("channel mismatch")
    Ho = (H + 2 * padding - dilation * (kh - 1) - 1) // stride + 1
    Wo = (W + 2 * padding - dilation * (kw - 1) - 1) // stride + 1
    px, loc, keep, _ = T.as_arg(x)
    pw, k1 = T.host_ptr(w)
    pb, k2 = T.host_ptr(bias)
    bnp = [T.host_ptr(a) for a in bn] if bn is not None else [(None, None)] * 4
    y = T.alloc_like(keep, (B, O, Ho, Wo))
    _ffi.check(_ffi.lib.brn_conv2d_forward(px, B, Cc, H, W, pw, pb, O, kh, kw, stride, padding, dilation, bnp[0][0], bnp[1][0],
                                           bnp[2][0], bnp[3][0], float(bn_eps), _ACT[act], T.ptr_of(y), loc,
                                           T.device_of(keep, device), T.stream_of(keep)))
    return y


def upsample_bilinear2d(x, out_h, out_w, device=0):
    """Tensor::upsample_bilinear2d(h, w, align_corners=true), NCHW (birefnet.rs:332)."""
    B, Cc, H, W = (int(v) for v in x.shape)
    px, loc, keep, _ = T.as_arg(x)
    y = T.alloc_like(keep, (B, Cc, out_h, out_w))
    _ffi.check(_ffi.lib.brn_upsample_bilinear2d(px, B, Cc, H, W, out_h, out_w, T.ptr_of(y), loc, T.device_of(keep, device),
                                                T.stream_of(keep)))
    return y


def window_attention(x, heads, shift, qkv_w, qkv_b, proj_w, proj_b, rel_table, window_size=12, device=0):
    """SwinTransformerBlock::forward between norm1 and the residual (swin.rs:356-403): x [B,H,W,C] -> [B,H,W,C]."""
    B, H, W, Cc = (int(v) for v in x.shape)
    px, loc, keep, _ = T.as_arg(x)
    hp = [T.host_ptr(a) for a in (qkv_w, qkv_b, proj_w, proj_b, rel_table)]
    y = T.alloc_like(keep, (B, H, W, Cc))
    _ffi.check(_ffi.lib.brn_window_attention_forward(px, B, H, W, Cc, heads, window_size, shift, *[h[0] for h in hp],
                                                     T.ptr_of(y), loc, T.device_of(keep, device), T.stream_of(keep)))
    return y


def attention(q, k, v, bias=None, n_bias=None, scale=None, device=0):
    """y[b,h] = softmax(scale * (q[b,h] k[b,h]^T + bias[b % n_bias, h])) v[b,h]: q, k, v [batch, heads, N, 32]; bias [n_bias, heads, N, N]
    (added to the UNSCALED scores) or None.  n_bias None = bias.shape[0]; scale None = head_dim^-0.5.  The limits are the library's
    (include/birefnet_hip.h brn_attention_forward): nothing is checked here."""
    batch, heads, N, hd = (int(s) for s in q.shape)
    pq, loc, keep, _ = T.as_arg(q)
    pk, kloc, kkeep, _ = T.as_arg(k, (batch, heads, N, hd))
    pv, vloc, vkeep, _ = T.as_arg(v, (batch, heads, N, hd))
    pb, bloc, bkeep, _ = T.as_arg(bias) if bias is not None else (None, loc, None, None)
    if not (kloc == vloc == bloc == loc):
        raise ValueError("q, k, v and bias must live on the same side")
    if n_bias is None:
        n_bias = int(bias.shape[0]) if bias is not None else 0
    y = T.alloc_like(keep, (batch, heads, N, hd))
    _ffi.check(_ffi.lib.brn_attention_forward(pq, pk, pv, batch, heads, N, hd, pb, int(n_bias), float(scale) if scale is not None else 0.0,
                                              T.ptr_of(y), loc, T.device_of(keep, device), T.stream_of(keep)))
    return y


def attention_with_bias(q, k, v, scaled_bias):
    """flash_attention_with_bias(&q, &k, &v, &scaled_bias, false) (swin.rs:252): scaled_bias [1 or batch, heads, N, N] is the bias
    already divided by the softmax scale (swin.rs:250).  N <= 144, head_dim 32; longer sequences, other head dims and the causal flag:
    flash_attention(..., layout="bhsd", bias=scaled_bias)."""
    return attention(q, k, v, scaled_bias)


def attention_with_repeating_bias(q, k, v, scaled_bias, n_windows):
    """flash_attention_with_repeating_bias(&q, &k, &v, &scaled_combined, n_windows, false) (swin.rs:243): scaled_bias
    [n_windows, heads, N, N], batch entry b reads pattern b % n_windows (swin.rs:291-294).  N <= 144, head_dim 32; the long form is
    flash_attention(..., layout="bhsd", bias=scaled_bias) with n_bias = scaled_bias.shape[0]."""
    return attention(q, k, v, scaled_bias, n_bias=int(n_windows))


_ATTN_LAYOUT = {"bshd": _ffi.BRN_ATTN_BSHD, "bhsd": _ffi.BRN_ATTN_BHSD}


def flash_attention(q, k, v, causal=False, scale=None, layout="bshd", device=0, bias=None):
    """flash_attention(&q, &k, &v, causal) (examples/bench_flash_attn.rs:39-53): y = softmax(scale * q k^T [causal: key j <= query i]) v per
    (batch entry, head).  layout "bshd": q [batch, seq_q, heads, head_dim], k, v [batch, seq_kv, heads, head_dim] (flash_attention's own);
    "bhsd": [batch, heads, seq, head_dim] (ops.attention's).  y has q's shape.  scale None = head_dim^-0.5.
    bias (a numpy array or a device tensor, like q): [n_bias, heads, seq_q, seq_kv] fp32, heads-major in either layout, added to the
    UNSCALED scores; batch entry b reads pattern b % n_bias; -inf excludes a key.  Without it brn_flash_attention_forward is called, with
    it brn_flash_attention_bias_forward.  The limits are the library's (include/birefnet_hip.h): nothing is checked here."""
    lay = _ATTN_LAYOUT[layout]
    if lay == _ffi.BRN_ATTN_BSHD:
        batch, seq_q, heads, hd = (int(s) for s in q.shape)
        seq_kv = int(k.shape[1])
        kv_shape = (batch, seq_kv, heads, hd)
    else:
        batch, heads, seq_q, hd = (int(s) for s in q.shape)
        seq_kv = int(k.shape[2])
        kv_shape = (batch, heads, seq_kv, hd)
    pq, loc, keep, _ = T.as_arg(q)
    pk, kloc, kkeep, _ = T.as_arg(k, kv_shape)
    pv, vloc, vkeep, _ = T.as_arg(v, kv_shape)
    if not (kloc == vloc == loc):
        raise ValueError("q, k and v must live on the same side")
    sc = float(scale) if scale is not None else 0.0
    if bias is None:
        y = T.alloc_like(keep, tuple(int(s) for s in q.shape))
        _ffi.check(_ffi.lib.brn_flash_attention_forward(pq, pk, pv, batch, seq_q, seq_kv, heads, hd, lay, int(bool(causal)), sc, T.ptr_of(y), loc,
                                                        T.device_of(keep, device), T.stream_of(keep)))
        return y
    n_bias = int(bias.shape[0])
    pb, bloc, bkeep, _ = T.as_arg(bias, (n_bias, heads, seq_q, seq_kv))
    if bloc != loc:
        raise ValueError("q, k, v and bias must live on the same side")
    y = T.alloc_like(keep, tuple(int(s) for s in q.shape))
    _ffi.check(_ffi.lib.brn_flash_attention_bias_forward(pq, pk, pv, batch, seq_q, seq_kv, heads, hd, lay, int(bool(causal)), pb, n_bias, sc,
                                                         T.ptr_of(y), loc, T.device_of(keep, device), T.stream_of(keep)))
    return y


def flash_attention_gqa(q, k, v, kv_heads=None, causal=False, scale=None, layout="bshd", bias=None, device=0):
    """brn_flash_attention_gqa_forward: flash_attention with K / V heads shared by groups of G = heads / kv_heads query heads (query head h
    reads K / V head h // G, the repeat_interleave(G) convention) and a causal mask that ends at the last key (key j <= query i +
    seq_kv - seq_q; seq_kv >= seq_q: attention over a K / V cache).  layout "bshd": q [batch, seq_q, heads, head_dim], k, v
    [batch, seq_kv, kv_heads, head_dim]; "bhsd": [batch, heads, seq_q, head_dim] and [batch, kv_heads, seq_kv, head_dim].  kv_heads None =
    taken from k's shape.  bias: as in flash_attention, [n_bias, heads, seq_q, seq_kv] fp32 indexed by QUERY head, or None.  y has q's
    shape.  The limits are the library's (include/birefnet_hip.h): nothing is checked here."""
    lay = _ATTN_LAYOUT[layout]
    seq_axis, head_axis = (1, 2) if lay == _ffi.BRN_ATTN_BSHD else (2, 1)
    batch, hd = int(q.shape[0]), int(q.shape[3])
    seq_q, heads, seq_kv = int(q.shape[seq_axis]), int(q.shape[head_axis]), int(k.shape[seq_axis])
    if kv_heads is None:
        kv_heads = int(k.shape[head_axis])
    kv_shape = (batch, seq_kv, kv_heads, hd) if lay == _ffi.BRN_ATTN_BSHD else (batch, kv_heads, seq_kv, hd)
    pq, loc, keep, _ = T.as_arg(q)
    pk, kloc, kkeep, _ = T.as_arg(k, kv_shape)
    pv, vloc, vkeep, _ = T.as_arg(v, kv_shape)
    n_bias = int(bias.shape[0]) if bias is not None else 0
    pb, bloc, bkeep, _ = T.as_arg(bias, (n_bias, heads, seq_q, seq_kv)) if bias is not None else (None, loc, None, None)
    if not (kloc == vloc == bloc == loc):
        raise ValueError("q, k, v and bias must live on the same side")
    y = T.alloc_like(keep, tuple(int(s) for s in q.shape))
    _ffi.check(_ffi.lib.brn_flash_attention_gqa_forward(pq, pk, pv, batch, seq_q, seq_kv, heads, int(kv_heads), hd, lay, int(bool(causal)), pb, n_bias,
                                                        float(scale) if scale is not None else 0.0, T.ptr_of(y), loc, T.device_of(keep, device),
                                                        T.stream_of(keep)))
    return y


def flash_attention_varlen(q, k, v, cu_seqlens_q, cu_seqlens_kv, window=(-1, -1), scale=None, kv_heads=None, device=0):
    """brn_flash_attention_varlen_forward: flash_attention_gqa over a packed batch.  q [total_q, heads, head_dim], k, v
    [total_kv, kv_heads, head_dim]; sequence s owns rows cu_seqlens[s] .. cu_seqlens[s + 1] - 1 of each.  cu_seqlens_q / cu_seqlens_kv:
    sequences or integer arrays of n_seqs + 1 offsets, converted to contiguous host int32 (they stay on the host whatever q is).
    window = (left, right): key j of a row's own sequence takes part in query i's row exactly when i + off - left <= j <= i + off + right,
    off = len_kv - len_q; -1 = unbounded.  (-1, -1) full, (-1, 0) causal, (W - 1, 0) a causal sliding window of W keys, (w, w) local.
    kv_heads None = taken from k's shape.  y has q's shape.  What only the wrapper can know is checked here, because the library would
    write or read past the tensors otherwise: the offsets fit int32, cu_seqlens_q[-1] == q.shape[0] and cu_seqlens_kv[-1] == k.shape[0].
    Every other limit is the library's (include/birefnet_hip.h)."""
    cq, ckv = (np.asarray(c.detach().cpu().numpy() if T._is_torch(c) else c).reshape(-1) for c in (cu_seqlens_q, cu_seqlens_kv))
    if cq.size != ckv.size or cq.size < 2:
        raise ValueError("cu_seqlens_q and cu_seqlens_kv must hold n_seqs + 1 offsets each, n_seqs >= 1")
    for c in (cq, ckv):
        if c.dtype.kind not in "iu" or int(c.min()) < -2 ** 31 or int(c.max()) >= 2 ** 31:
            raise ValueError("cu_seqlens must be integers that fit int32")
    cq, ckv = (np.ascontiguousarray(c, dtype=np.int32) for c in (cq, ckv))
    if int(cq[-1]) != int(q.shape[0]) or int(ckv[-1]) != int(k.shape[0]):
        raise ValueError(f"cu_seqlens_q[-1] {int(cq[-1])} / cu_seqlens_kv[-1] {int(ckv[-1])} must be the rows of q ({int(q.shape[0])}) / of k and v ({int(k.shape[0])})")
    window = tuple(min(int(w), 2 ** 31 - 1) for w in window)        # the library takes ints; anything this large is unbounded
    total_q, heads, hd = (int(s) for s in q.shape)
    if kv_heads is None:
        kv_heads = int(k.shape[1])
    kv_shape = (int(k.shape[0]), int(kv_heads), hd)
    pq, loc, keep, _ = T.as_arg(q)
    pk, kloc, kkeep, _ = T.as_arg(k, kv_shape)
    pv, vloc, vkeep, _ = T.as_arg(v, kv_shape)
    if not (kloc == vloc == loc):
        raise ValueError("q, k and v must live on the same side")
    y = T.alloc_like(keep, (total_q, heads, hd))
    _ffi.check(_ffi.lib.brn_flash_attention_varlen_forward(pq, pk, pv, cq.ctypes.data, ckv.ctypes.data, int(cq.size) - 1, heads, int(kv_heads), hd,
                                                           int(window[0]), int(window[1]), float(scale) if scale is not None else 0.0, T.ptr_of(y), loc,
                                                           T.device_of(keep, device), T.stream_of(keep)))
    return y


def flash_attention_splitkv_plan(batch, seq_q, seq_kv, heads, kv_heads, head_dim, kv_splits=0):
    """brn_flash_attention_splitkv_plan: (S, tiles_per_split, workspace_floats) a call with these integers will use; needs no device."""
    import ctypes as C
    S, tps, nws = C.c_int(0), C.c_int(0), C.c_size_t(0)
    _ffi.check(_ffi.lib.brn_flash_attention_splitkv_plan(int(batch), int(seq_q), int(seq_kv), int(heads), int(kv_heads), int(head_dim), int(kv_splits),
                                                         C.byref(S), C.byref(tps), C.byref(nws)))
    return S.value, tps.value, nws.value


def flash_attention_splitkv(q, k, v, kv_heads=None, causal=False, scale=None, layout="bshd", kv_splits=0, return_lse=False, return_partials=False,
                            device=0):
    """brn_flash_attention_splitkv_forward: flash_attention_gqa without a bias, the K / V tiles of a call split between workgroups
    (kv_splits; 0 = the library's rule) and combined in a fixed order.  Shapes, layout, kv_heads, causal and scale as in
    flash_attention_gqa.  The workspace is sized by brn_flash_attention_splitkv_plan and allocated beside q.  Returns y; with return_lse
    (y, lse [batch, heads, seq_q]); with return_partials additionally (O_part [S, R, head_dim], lse2_part [S, R]), views of the
    workspace, R = batch * heads * seq_q (heads-major rows); S == 1 leaves no partials and returns (None, None).  The limits are the
    library's (include/birefnet_hip.h): nothing is checked here."""
    lay = _ATTN_LAYOUT[layout]
    seq_axis, head_axis = (1, 2) if lay == _ffi.BRN_ATTN_BSHD else (2, 1)
    batch, hd = int(q.shape[0]), int(q.shape[3])
    seq_q, heads, seq_kv = int(q.shape[seq_axis]), int(q.shape[head_axis]), int(k.shape[seq_axis])
    if kv_heads is None:
        kv_heads = int(k.shape[head_axis])
    kv_shape = (batch, seq_kv, kv_heads, hd) if lay == _ffi.BRN_ATTN_BSHD else (batch, kv_heads, seq_kv, hd)
    pq, loc, keep, _ = T.as_arg(q)
    pk, kloc, kkeep, _ = T.as_arg(k, kv_shape)
    pv, vloc, vkeep, _ = T.as_arg(v, kv_shape)
    if not (kloc == vloc == loc):
        raise ValueError("q, k and v must live on the same side")
    S, _tps, nws = flash_attention_splitkv_plan(batch, seq_q, seq_kv, heads, kv_heads, hd, kv_splits)
    R = batch * heads * seq_q
    y = T.alloc_like(keep, tuple(int(s) for s in q.shape))
    lse = T.alloc_like(keep, (batch, heads, seq_q)) if return_lse else None
    ws = T.alloc_like(keep, (nws,)) if S > 1 else None
    _ffi.check(_ffi.lib.brn_flash_attention_splitkv_forward(pq, pk, pv, batch, seq_q, seq_kv, heads, int(kv_heads), hd, lay, int(bool(causal)),
                                                            float(scale) if scale is not None else 0.0, int(kv_splits), T.ptr_of(y),
                                                            T.ptr_of(lse) if lse is not None else None, T.ptr_of(ws) if ws is not None else None,
                                                            nws if ws is not None else 0, loc, T.device_of(keep, device), T.stream_of(keep)))
    out = (y,) + ((lse,) if return_lse else ())
    if return_partials:
        out += ((ws[:S * R * hd].reshape(S, R, hd), ws[S * R * hd:].reshape(S, R)) if ws is not None else (None, None),)
    return out[0] if len(out) == 1 else out


def _int32_arg(a, shape, what):
    """an int32 contiguous array / tensor of `shape` -> (pointer, loc, keepalive, host copy or None): a numpy input (or a CPU tensor) is
    converted and handed back for the range checks; a device tensor is never read back"""
    if T._is_torch(a):
        import torch
        if a.dtype != torch.int32:
            raise TypeError(f"{what} must be an int32 tensor")
        t = a.contiguous()
        if tuple(t.shape) != tuple(shape):
            raise ValueError(f"{what}: expected shape {tuple(shape)}, got {tuple(t.shape)}")
        if t.is_cuda:
            return t.data_ptr(), _ffi.BRN_MEM_DEVICE, t, None
        return t.data_ptr(), _ffi.BRN_MEM_HOST, t, t.numpy()
    h = np.asarray(a)
    if h.dtype.kind not in "iu" or (h.size and (int(h.min()) < -2 ** 31 or int(h.max()) >= 2 ** 31)):
        raise ValueError(f"{what} must be integers that fit int32")
    h = np.ascontiguousarray(h, dtype=np.int32)
    if tuple(h.shape) != tuple(shape):
        raise ValueError(f"{what}: expected shape {tuple(shape)}, got {tuple(h.shape)}")
    return h.ctypes.data, _ffi.BRN_MEM_HOST, h, h


_KV_TYPE = {None: _ffi.BRN_KV_F32, "f32": _ffi.BRN_KV_F32, "bf16": _ffi.BRN_KV_BF16, "f16": _ffi.BRN_KV_F16}


def _pool_arg(a, shape, kv_dtype, what):
    """a K / V pool of `kv_dtype` ("f32", "bf16", "f16") AS IT IS, never converted or copied (the append writes it in place) ->
    (pointer, loc, keepalive).  f32: float32 tensors / arrays.  bf16 / f16: torch.bfloat16 / torch.float16 tensors (host or device),
    np.float16 arrays for f16, np.uint16 arrays of bit patterns for either (numpy has no bf16).  "fp8" (the e4m3fn pool of the fp8
    entries): torch.uint8 or torch.float8_e4m3fn tensors, np.uint8 arrays of the bytes.  Anything else raises."""
    if tuple(int(s) for s in a.shape) != tuple(shape):
        raise ValueError(f"{what}: expected shape {tuple(shape)}, got {tuple(a.shape)}")
    if T._is_torch(a):
        import torch
        want = {"f32": (torch.float32,), "bf16": (torch.bfloat16,), "f16": (torch.float16,), "fp8": (torch.uint8, torch.float8_e4m3fn)}[kv_dtype]
        if a.dtype not in want:
            raise TypeError(f"{what}: kv_dtype {kv_dtype!r} needs a {' or '.join(str(w) for w in want)} tensor, got {a.dtype}")
        if not a.is_contiguous():
            raise ValueError(f"{what} must be contiguous")
        return a.data_ptr(), (_ffi.BRN_MEM_DEVICE if a.is_cuda else _ffi.BRN_MEM_HOST), a
    if not isinstance(a, np.ndarray):
        raise TypeError(f"{what} must be a torch tensor or a numpy array")
    ok = {"f32": (np.float32,), "bf16": (np.uint16,), "f16": (np.float16, np.uint16), "fp8": (np.uint8,)}[kv_dtype]
    if a.dtype not in [np.dtype(t) for t in ok]:
        raise TypeError(f"{what}: kv_dtype {kv_dtype!r} needs a numpy array of {' or '.join(np.dtype(t).name for t in ok)}, got {a.dtype}")
    if not a.flags.c_contiguous:
        raise ValueError(f"{what} must be contiguous")
    return a.ctypes.data, _ffi.BRN_MEM_HOST, a


def flash_attention_paged(q, k_pages, v_pages, block_table, kv_lens, max_kv_len=None, causal=False, scale=None, layout="bshd", kv_splits=0,
                          return_lse=False, return_partials=False, device=0, kv_dtype=None):
    """brn_flash_attention_paged_forward: flash_attention_splitkv over a paged K / V cache.  q as in flash_attention_splitkv (layout
    "bshd" [batch, seq_q, heads, head_dim] or "bhsd"); k_pages, v_pages [n_pages, page_size, kv_heads, head_dim] fp32; block_table
    [batch, max_pages] int32 (key j of batch entry b is row j % page_size of page block_table[b][j // page_size]); kv_lens [batch] int32;
    both on q's side.  max_kv_len sizes the grid and the split: None = max_pages * page_size capped at 65536.  The workspace is sized by
    flash_attention_splitkv_plan(batch, seq_q, max_kv_len, ...) and allocated beside q.  Returns as flash_attention_splitkv: y, with
    return_lse (y, lse), with return_partials additionally (O_part, lse2_part) or (None, None) when S == 1.  A row with no visible key
    comes back as zeros with lse -inf.
    For host (numpy / CPU tensor) inputs only, the wrapper refuses what only it can know cheaply: a length outside 0 .. max_kv_len and a
    USED table entry (one below ceil(len / page_size) of its sequence) outside 0 .. n_pages - 1.  Device tensors are not read back: the
    library clamps their values (include/birefnet_hip.h).  Every other limit is the library's.
    kv_dtype None: the above, exactly (whatever the pool is given as is converted to fp32).  "bf16" / "f16": brn_flash_attention_paged_kv_forward
    on a pool STORED in that type: torch.bfloat16 / torch.float16 tensors (host or device), np.float16 arrays for "f16", np.uint16 arrays
    of bit patterns for either; a pool of another dtype raises.  ("f32" is the new entry on an fp32 pool: the bits of None.)"""
    if kv_dtype not in _KV_TYPE:
        raise ValueError(f"kv_dtype {kv_dtype!r} unknown (None, 'f32', 'bf16' or 'f16')")
    return _flash_attention_paged(q, k_pages, v_pages, block_table, kv_lens, max_kv_len, causal, scale, layout, kv_splits, return_lse, return_partials, device, kv_dtype, None)


def flash_attention_paged_fp8(q, k_pages, v_pages, k_scale, v_scale, block_table, kv_lens, max_kv_len=None, causal=False, scale=None, layout="bshd", kv_splits=0,
                              return_lse=False, return_partials=False, device=0):
    """brn_flash_attention_paged_fp8_forward: flash_attention_paged over a pool STORED in fp8.  k_pages, v_pages
    [n_pages, page_size, kv_heads, head_dim] of OCP e4m3fn bytes, taken as they are: torch.uint8 or torch.float8_e4m3fn tensors (host or
    device), np.uint8 arrays on the host.  k_scale, v_scale: [kv_heads] fp32 on q's side, or None = all ones; byte e of K head h stands
    for k_scale[h] * e4m3(e), the same for V.  Everything else, the host-side checks included, is flash_attention_paged's.  One pool is
    read by every compute mode; lse and the partials carry the bits of flash_attention_paged on the widened bytes at
    scale * k_scale[h / G], y those bits times v_scale[h / G] (include/birefnet_hip.h)."""
    return _flash_attention_paged(q, k_pages, v_pages, block_table, kv_lens, max_kv_len, causal, scale, layout, kv_splits, return_lse, return_partials, device, "fp8",
                                  (k_scale, v_scale))


def _scale_arg(a, kv_heads, what):
    """a [kv_heads] fp32 scale array or None -> (pointer or None, loc or None, keepalive)"""
    if a is None:
        return None, None, None
    p, loc, keep, _ = T.as_arg(a, (kv_heads,))
    return p, loc, keep


def _flash_attention_paged(q, k_pages, v_pages, block_table, kv_lens, max_kv_len, causal, scale, layout, kv_splits, return_lse, return_partials, device, kv_dtype, scales):
    """the body of flash_attention_paged (scales None) and flash_attention_paged_fp8 (kv_dtype "fp8", scales = (k_scale, v_scale))"""
    lay = _ATTN_LAYOUT[layout]
    seq_axis, head_axis = (1, 2) if lay == _ffi.BRN_ATTN_BSHD else (2, 1)
    batch, hd = int(q.shape[0]), int(q.shape[3])
    seq_q, heads = int(q.shape[seq_axis]), int(q.shape[head_axis])
    n_pages, page_size, kv_heads = (int(s) for s in k_pages.shape[:3])
    if len(block_table.shape) != 2:
        raise ValueError("block_table must be [batch, max_pages]")
    max_pages = int(block_table.shape[1])
    if max_kv_len is None:
        max_kv_len = min(max_pages * page_size, 65536)
    max_kv_len = int(max_kv_len)
    pool_shape = (n_pages, page_size, kv_heads, hd)
    pq, loc, keep, _ = T.as_arg(q)
    if kv_dtype is None:
        pk, kloc, kkeep, _ = T.as_arg(k_pages, pool_shape)
        pv, vloc, vkeep, _ = T.as_arg(v_pages, pool_shape)
    else:
        pk, kloc, kkeep = _pool_arg(k_pages, pool_shape, kv_dtype, "k_pages")
        pv, vloc, vkeep = _pool_arg(v_pages, pool_shape, kv_dtype, "v_pages")
    pt, tloc, tkeep, th = _int32_arg(block_table, (batch, max_pages), "block_table")
    pl, lloc, lkeep, lh = _int32_arg(kv_lens, (batch,), "kv_lens")
    if not (kloc == vloc == tloc == lloc == loc):
        raise ValueError("q, k_pages, v_pages, block_table and kv_lens must live on the same side")
    if scales is not None:
        (pks, ksloc, kskeep), (pvs, vsloc, vskeep) = (_scale_arg(a, kv_heads, n) for a, n in zip(scales, ("k_scale", "v_scale")))
        if any(sl is not None and sl != loc for sl in (ksloc, vsloc)):
            raise ValueError("k_scale and v_scale must live on q's side")
    if lh is not None and th is not None:
        if lh.size and (int(lh.min()) < 0 or int(lh.max()) > max_kv_len):
            raise ValueError(f"kv_lens must lie in 0 .. max_kv_len = {max_kv_len}")
        used = np.arange(max_pages)[None, :] * page_size < lh[:, None]
        if used.any() and (int(th[used].min()) < 0 or int(th[used].max()) >= n_pages):
            raise ValueError(f"block_table entries in use must lie in 0 .. n_pages - 1 = {n_pages - 1}")
    S, _tps, nws = flash_attention_splitkv_plan(batch, seq_q, max_kv_len, heads, kv_heads, hd, kv_splits)
    R = batch * heads * seq_q
    y = T.alloc_like(keep, tuple(int(s) for s in q.shape))
    lse = T.alloc_like(keep, (batch, heads, seq_q)) if return_lse else None
    ws = T.alloc_like(keep, (nws,)) if S > 1 else None
    tail = (batch, seq_q, max_kv_len, heads, kv_heads, hd, n_pages, page_size, max_pages, lay, int(bool(causal)), float(scale) if scale is not None else 0.0,
            int(kv_splits), T.ptr_of(y), T.ptr_of(lse) if lse is not None else None, T.ptr_of(ws) if ws is not None else None,
            nws if ws is not None else 0, loc, T.device_of(keep, device), T.stream_of(keep))
    if kv_dtype is None:
        _ffi.check(_ffi.lib.brn_flash_attention_paged_forward(pq, pk, pv, pt, pl, *tail))
    elif scales is not None:
        _ffi.check(_ffi.lib.brn_flash_attention_paged_fp8_forward(pq, pk, pv, pks, pvs, pt, pl, *tail))
    else:
        _ffi.check(_ffi.lib.brn_flash_attention_paged_kv_forward(pq, pk, pv, _KV_TYPE[kv_dtype], pt, pl, *tail))
    out = (y,) + ((lse,) if return_lse else ())
    if return_partials:
        out += ((ws[:S * R * hd].reshape(S, R, hd), ws[S * R * hd:].reshape(S, R)) if ws is not None else (None, None),)
    return out[0] if len(out) == 1 else out


def kv_cache_append(k_new, v_new, k_pages, v_pages, block_table, kv_lens, kv_dtype=None, layout="bshd", update_lens=True, device=0):
    """brn_kv_cache_append: the seq_new tokens of k_new, v_new (fp32; layout "bshd" [batch, seq_new, kv_heads, head_dim] or "bhsd") go
    into the pool behind the keys each sequence has: token t of batch entry b becomes key L_b + t, L_b = kv_lens[b] clamped to
    0 .. max_pages * page_size; positions at or past that cap are dropped.  k_pages, v_pages [n_pages, page_size, kv_heads, head_dim]
    are written IN PLACE and therefore taken as they are: float32 for kv_dtype None / "f32"; for "bf16" / "f16" the dtypes
    flash_attention_paged(kv_dtype=...) accepts (the cast is the attention kernels', round to nearest even).  block_table
    [batch, max_pages] int32 and kv_lens [batch] int32, all on k_new's side.
    update_lens True: kv_lens (an int32 tensor / array, not a list) is updated in place and returned; False: the new lengths come back
    in a new array and kv_lens is left alone; None: no lengths are written and None is returned.
    For host inputs only, the wrapper refuses what flash_attention_paged refuses there: a length outside 0 .. max_pages * page_size and a
    table entry at a written position outside 0 .. n_pages - 1.  Device tensors are not read back: the library clamps their values."""
    if kv_dtype not in _KV_TYPE:
        raise ValueError(f"kv_dtype {kv_dtype!r} unknown (None, 'f32', 'bf16' or 'f16')")
    return _kv_cache_append(k_new, v_new, k_pages, v_pages, block_table, kv_lens, kv_dtype or "f32", layout, update_lens, device, None)


def kv_cache_append_fp8(k_new, v_new, k_pages, v_pages, k_scale, v_scale, block_table, kv_lens, layout="bshd", update_lens=True, device=0):
    """brn_kv_cache_append_fp8: kv_cache_append into the fp8 pool of flash_attention_paged_fp8 (torch.uint8 / torch.float8_e4m3fn
    tensors, np.uint8 arrays on the host; written in place).  k_scale, v_scale: [kv_heads] fp32 on k_new's side, or None = all ones.
    An element x of head h is stored as the e4m3fn byte of clamp(x / scale[h], -448, 448), rounded to nearest even; a NaN becomes a NaN
    byte.  The position rule, update_lens and the host-side checks are kv_cache_append's."""
    return _kv_cache_append(k_new, v_new, k_pages, v_pages, block_table, kv_lens, "fp8", layout, update_lens, device, (k_scale, v_scale))


_ROPE_STYLE = {"half": _ffi.BRN_ROPE_HALF, "interleaved": _ffi.BRN_ROPE_INTERLEAVED}


def rope_table(n_pos, rot_dim, theta=10000.0):
    """(cos, sin), each [n_pos, rot_dim / 2] float32: the angles p * theta^(-2 i / rot_dim) computed in float64 with numpy and rounded to
    fp32 once.  A convenience: the library takes any table (a scaled or interpolated one included) and promises its result for the
    table it is given, not for this one."""
    n_pos, rot_dim = int(n_pos), int(rot_dim)
    if n_pos < 1 or rot_dim < 2 or rot_dim % 2:
        raise ValueError("rope_table needs n_pos >= 1 and an even rot_dim >= 2")
    ang = np.arange(n_pos, dtype=np.float64)[:, None] * float(theta) ** (-np.arange(0, rot_dim, 2, dtype=np.float64) / rot_dim)[None, :]
    return np.cos(ang).astype(np.float32), np.sin(ang).astype(np.float32)


def _rope_table_arg(cos, sin, loc):
    """the two halves of a table on the side `loc` -> (cos pointer, sin pointer, n_pos, rot_dim, keepalives)"""
    if len(cos.shape) != 2:
        raise ValueError("cos and sin must be [n_pos, rot_dim / 2]")
    n_pos, half = int(cos.shape[0]), int(cos.shape[1])
    pc, cloc, ckeep, _ = T.as_arg(cos, (n_pos, half))
    ps, sloc, skeep, _ = T.as_arg(sin, (n_pos, half))
    if not (cloc == sloc == loc):
        raise ValueError("cos and sin must live on the side of the tensor they rotate")
    return pc, ps, n_pos, 2 * half, (ckeep, skeep)


def rope(x, cos, sin, positions=None, rot_dim=None, style="half", layout="bshd", out=None, device=0):
    """brn_rope_forward: x (fp32; layout "bshd" [batch, seq, heads, head_dim] or "bhsd") with the first rot_dim elements of every head
    row rotated in pairs; cos, sin [n_pos, rot_dim / 2] fp32 (rope_table makes the usual one), all on x's side.  Token t of batch entry b
    uses table row min(max(positions[b], 0) + t, n_pos - 1); positions [batch] int32 or None = all 0.  style "half" pairs x[i] with
    x[i + rot_dim / 2] (NeoX / Llama), "interleaved" pairs x[2i] with x[2i + 1] (GPT-J); a' = fl(fl(a cos) - fl(b sin)),
    b' = fl(fl(b cos) + fl(a sin)) in fp32, never fused; elements past rot_dim are copied.  rot_dim None: what the table says; a value
    must agree with it.  out: None = a new array beside x; x itself = in place; any other array of x's shape on x's side.
    For host inputs only, the wrapper refuses max(positions) + seq > n_pos (the library would clamp it to the last row).  Device
    tensors are not read back."""
    lay = _ATTN_LAYOUT[layout]
    seq_axis, head_axis = (1, 2) if lay == _ffi.BRN_ATTN_BSHD else (2, 1)
    shape = tuple(int(v) for v in x.shape)
    batch, hd, seq, heads = shape[0], shape[3], shape[seq_axis], shape[head_axis]
    px, loc, keep, _ = T.as_arg(x)
    pc, ps, n_pos, rd, rkeep = _rope_table_arg(cos, sin, loc)
    if rot_dim is not None and int(rot_dim) != rd:
        raise ValueError(f"rot_dim {rot_dim} does not agree with the table's {rd} (cos and sin are [n_pos, rot_dim / 2])")
    pp, ph = None, None
    if positions is not None:
        pp, ploc, pkeep, ph = _int32_arg(positions, (batch,), "positions")
        if ploc != loc:
            raise ValueError("positions must live on x's side")
    pmax = max(int(ph.max()), 0) if ph is not None and ph.size else 0
    if loc == _ffi.BRN_MEM_HOST and pmax + seq > n_pos:
        raise ValueError(f"max(positions) + seq = {pmax + seq} runs past the table (n_pos = {n_pos})")
    if out is None:
        y = T.alloc_like(keep, shape)
    elif out is x:
        if keep is not x and not (T._is_torch(x) and keep.data_ptr() == x.data_ptr()):
            raise TypeError("out=x needs x as a contiguous float32 tensor or array (it is written in place)")
        y = x
    else:
        if tuple(int(v) for v in out.shape) != shape:
            raise ValueError(f"out: expected shape {shape}, got {tuple(out.shape)}")
        py, yloc, ykeep, _ = T.as_arg(out)
        if yloc != loc or (ykeep is not out and not (T._is_torch(out) and ykeep.data_ptr() == out.data_ptr())):
            raise TypeError("out must be a contiguous float32 tensor or array on x's side (it is written in place)")
        y = out
    _ffi.check(_ffi.lib.brn_rope_forward(px, batch, seq, heads, hd, lay, pc, ps, n_pos, rd, _ROPE_STYLE[style], pp, T.ptr_of(y), loc,
                                         T.device_of(keep, device), T.stream_of(keep)))
    return y


def kv_cache_append_rope(k_new, v_new, cos, sin, k_pages, v_pages, block_table, kv_lens, kv_dtype=None, style="half", layout="bshd", update_lens=True, device=0):
    """brn_kv_cache_append_rope: kv_cache_append with K token t of batch entry b rotated by rope's rule at table row
    min(L_b + t, n_pos - 1), the position it takes in the cache, in fp32 before the cast; V is not rotated.  cos, sin: the table of rope
    on k_new's side (rot_dim is the table's).  The pool and the lengths carry the bits of kv_cache_append on
    rope(k_new, cos, sin, positions=kv_lens).  Everything else is kv_cache_append's.
    For host inputs only, the wrapper also refuses max(min(L_b + seq_new, cap)) > n_pos.  Device tensors are not read back."""
    if kv_dtype not in _KV_TYPE:
        raise ValueError(f"kv_dtype {kv_dtype!r} unknown (None, 'f32', 'bf16' or 'f16')")
    return _kv_cache_append(k_new, v_new, k_pages, v_pages, block_table, kv_lens, kv_dtype or "f32", layout, update_lens, device, None, (cos, sin, style))


def kv_cache_append_rope_fp8(k_new, v_new, cos, sin, k_pages, v_pages, k_scale, v_scale, block_table, kv_lens, style="half", layout="bshd", update_lens=True, device=0):
    """brn_kv_cache_append_rope_fp8: kv_cache_append_fp8 with K rotated as in kv_cache_append_rope, in fp32, in front of the fp8 store
    (divide by the head's scale, clamp to +-448, round to nearest even)."""
    return _kv_cache_append(k_new, v_new, k_pages, v_pages, block_table, kv_lens, "fp8", layout, update_lens, device, (k_scale, v_scale), (cos, sin, style))


def _kv_cache_append(k_new, v_new, k_pages, v_pages, block_table, kv_lens, kv_dtype, layout, update_lens, device, scales, rope=None):
    """the body of kv_cache_append (scales None) and kv_cache_append_fp8 (kv_dtype "fp8", scales = (k_scale, v_scale)); rope =
    (cos, sin, style): their rope forms"""
    lay = _ATTN_LAYOUT[layout]
    seq_axis, head_axis = (1, 2) if lay == _ffi.BRN_ATTN_BSHD else (2, 1)
    batch, hd = int(k_new.shape[0]), int(k_new.shape[3])
    seq_new, kv_heads = int(k_new.shape[seq_axis]), int(k_new.shape[head_axis])
    n_pages, page_size = int(k_pages.shape[0]), int(k_pages.shape[1])
    if len(block_table.shape) != 2:
        raise ValueError("block_table must be [batch, max_pages]")
    max_pages = int(block_table.shape[1])
    pool_shape = (n_pages, page_size, kv_heads, hd)
    pk, loc, keep, _ = T.as_arg(k_new)
    pv, vloc, vkeep, _ = T.as_arg(v_new, tuple(int(s) for s in k_new.shape))
    ppk, kloc, kkeep = _pool_arg(k_pages, pool_shape, kv_dtype, "k_pages")
    ppv, pvloc, pvkeep = _pool_arg(v_pages, pool_shape, kv_dtype, "v_pages")
    pt, tloc, tkeep, th = _int32_arg(block_table, (batch, max_pages), "block_table")
    pl, lloc, lkeep, lh = _int32_arg(kv_lens, (batch,), "kv_lens")
    if not (vloc == kloc == pvloc == tloc == lloc == loc):
        raise ValueError("k_new, v_new, k_pages, v_pages, block_table and kv_lens must live on the same side")
    if scales is not None:
        (pks, ksloc, kskeep), (pvs, vsloc, vskeep) = (_scale_arg(a, kv_heads, n) for a, n in zip(scales, ("k_scale", "v_scale")))
        if any(sl is not None and sl != loc for sl in (ksloc, vsloc)):
            raise ValueError("k_scale and v_scale must live on k_new's side")
    cap = max_pages * page_size
    if rope is not None:
        pc, ps, n_pos, rd, rkeep = _rope_table_arg(rope[0], rope[1], loc)    # (a name of its own: tkeep keeps block_table's copy alive)
        table = (pc, ps, n_pos, rd, _ROPE_STYLE[rope[2]])
        if lh is not None and lh.size and int(np.minimum(np.clip(lh, 0, cap).astype(np.int64) + seq_new, cap).max()) > n_pos:
            raise ValueError(f"max(min(L_b + seq_new, cap)) runs past the table (n_pos = {n_pos})")
    if lh is not None and th is not None:
        if lh.size and (int(lh.min()) < 0 or int(lh.max()) > cap):
            raise ValueError(f"kv_lens must lie in 0 .. max_pages * page_size = {cap}")
        slots = np.arange(max_pages)[None, :]
        written = (slots >= lh[:, None] // page_size) & (slots * page_size < np.minimum(lh[:, None] + seq_new, cap))
        if written.any() and (int(th[written].min()) < 0 or int(th[written].max()) >= n_pages):
            raise ValueError(f"block_table entries at written positions must lie in 0 .. n_pages - 1 = {n_pages - 1}")
    if update_lens is None:
        out, po = None, None
    elif update_lens:
        if lkeep is not kv_lens and not (T._is_torch(kv_lens) and lkeep.data_ptr() == kv_lens.data_ptr()):
            raise TypeError("update_lens=True needs kv_lens as a contiguous int32 tensor or array (it is written in place)")
        out, po = kv_lens, pl
    else:
        if T._is_torch(lkeep):
            import torch
            out = torch.empty_like(lkeep)
            po = out.data_ptr()
        else:
            out = np.empty(batch, np.int32)
            po = out.ctypes.data
    head = (pk, pv, batch, seq_new, kv_heads, hd, lay)
    tail = (pt, pl, po, n_pages, page_size, max_pages, loc, T.device_of(keep, device), T.stream_of(keep))
    if scales is not None:
        fn, pool = (_ffi.lib.brn_kv_cache_append_fp8 if rope is None else _ffi.lib.brn_kv_cache_append_rope_fp8), (ppk, ppv, pks, pvs)
    else:
        fn, pool = (_ffi.lib.brn_kv_cache_append if rope is None else _ffi.lib.brn_kv_cache_append_rope), (ppk, ppv, _KV_TYPE[kv_dtype])
    _ffi.check(fn(*head, *(table if rope is not None else ()), *pool, *tail))
    return out


_POOL_TYPE = {None: _ffi.BRN_POOL_F32, "bf16": _ffi.BRN_POOL_BF16, "f16": _ffi.BRN_POOL_F16, "e4m3": _ffi.BRN_POOL_E4M3}
_POOL_DTYPE = {None: "f32", "bf16": "bf16", "f16": "f16", "e4m3": "fp8"}          # what _pool_arg calls the storage


def flash_attention_paged_varlen_plan(total_q, n_seqs, max_kv_len, heads, kv_heads, head_dim, kv_splits=0):
    """brn_flash_attention_paged_varlen_plan: (S, tiles_per_split, workspace_floats, plan_ints) a packed paged call with these integers
    will use; needs no device."""
    import ctypes as C
    S, tps, nws, npl = C.c_int(0), C.c_int(0), C.c_size_t(0), C.c_size_t(0)
    _ffi.check(_ffi.lib.brn_flash_attention_paged_varlen_plan(int(total_q), int(n_seqs), int(max_kv_len), int(heads), int(kv_heads), int(head_dim), int(kv_splits),
                                                              C.byref(S), C.byref(tps), C.byref(nws), C.byref(npl)))
    return S.value, tps.value, nws.value, npl.value


def _int_buffer_like(keep, n):
    """n int32 beside `keep` (a device tensor, or anything on the host)"""
    if T._is_torch(keep):
        import torch
        return torch.empty(n, dtype=torch.int32, device=keep.device)
    return np.empty(n, np.int32)


def _packed_pool_args(kv_dtype, k_pages, v_pages, pool_shape, k_scale, v_scale, kv_heads):
    if kv_dtype not in _POOL_TYPE:
        raise ValueError(f"kv_dtype {kv_dtype!r} unknown (None, 'bf16', 'f16' or 'e4m3')")
    if kv_dtype != "e4m3" and (k_scale is not None or v_scale is not None):
        raise ValueError("k_scale and v_scale exist for kv_dtype 'e4m3' alone")
    pk, kloc, kkeep = _pool_arg(k_pages, pool_shape, _POOL_DTYPE[kv_dtype], "k_pages")
    pv, vloc, vkeep = _pool_arg(v_pages, pool_shape, _POOL_DTYPE[kv_dtype], "v_pages")
    (pks, ksloc, kskeep), (pvs, vsloc, vskeep) = (_scale_arg(a, kv_heads, n) for a, n in zip((k_scale, v_scale), ("k_scale", "v_scale")))
    return (pk, pv, pks, pvs), [kloc, vloc] + [sl for sl in (ksloc, vsloc) if sl is not None], (kkeep, vkeep, kskeep, vskeep)


def flash_attention_paged_varlen(q, k_pages, v_pages, block_table, kv_lens, cu_seqlens_q, max_kv_len=None, causal=False, scale=None, kv_splits=0,
                                 return_lse=False, return_partials=False, device=0, kv_dtype=None, k_scale=None, v_scale=None, out=None, lse_out=None,
                                 workspace=None, plan_workspace=None):
    """brn_flash_attention_paged_varlen_forward: flash_attention_paged over a PACKED batch of new tokens, one call for a mixed prefill /
    decode step.  q [total_q, heads, head_dim] fp32; cu_seqlens_q [n_seqs + 1] int32: sequence b owns tokens cu[b] .. cu[b + 1] - 1 (the
    library clamps it: running maximum of the values clamped to 0 .. total_q); tokens outside cu[0] .. cu[n_seqs] are padding and their
    rows of y, lse and the partials are not written.  block_table [n_seqs, max_pages] int32, kv_lens [n_seqs] int32 (the lengths AFTER the
    new keys were appended); the pool as flash_attention_paged takes it, STORED as kv_dtype says: None float32, "bf16", "f16", or "e4m3"
    (with k_scale, v_scale [kv_heads] fp32 or None).  All on q's side; nothing is read back or checked here.
    out / lse_out / workspace / plan_workspace: buffers to use instead of fresh ones (y [total_q, heads, head_dim]; lse [heads, total_q];
    workspace >= the plan's workspace_floats fp32; plan_workspace >= the plan's plan_ints int32).
    Returns as flash_attention_paged: y, with return_lse (y, lse [heads, total_q]), with return_partials additionally
    (O_part [S, heads * total_q, head_dim], lse2_part [S, heads * total_q]) or (None, None) when S == 1."""
    total_q, heads, hd = (int(s) for s in q.shape)
    n_pages, page_size, kv_heads = (int(s) for s in k_pages.shape[:3])
    if len(block_table.shape) != 2:
        raise ValueError("block_table must be [n_seqs, max_pages]")
    n_seqs, max_pages = int(block_table.shape[0]), int(block_table.shape[1])
    if max_kv_len is None:
        max_kv_len = min(max_pages * page_size, 65536)
    max_kv_len = int(max_kv_len)
    pq, loc, keep, _ = T.as_arg(q)
    (pk, pv, pks, pvs), locs, pkeep = _packed_pool_args(kv_dtype, k_pages, v_pages, (n_pages, page_size, kv_heads, hd), k_scale, v_scale, kv_heads)
    pt, tloc, tkeep, _ = _int32_arg(block_table, (n_seqs, max_pages), "block_table")
    pl, lloc, lkeep, _ = _int32_arg(kv_lens, (n_seqs,), "kv_lens")
    pc, cloc, ckeep, _ = _int32_arg(cu_seqlens_q, (n_seqs + 1,), "cu_seqlens_q")
    if any(l != loc for l in locs + [tloc, lloc, cloc]):
        raise ValueError("q, the pool, the scales, block_table, kv_lens and cu_seqlens_q must live on the same side")
    S, _tps, nws, npl = flash_attention_paged_varlen_plan(total_q, n_seqs, max_kv_len, heads, kv_heads, hd, kv_splits)
    R = heads * total_q
    y = out if out is not None else T.alloc_like(keep, (total_q, heads, hd))
    lse = lse_out if lse_out is not None else (T.alloc_like(keep, (heads, total_q)) if return_lse else None)
    ws = workspace if workspace is not None else (T.alloc_like(keep, (nws,)) if S > 1 else None)
    plan = plan_workspace if plan_workspace is not None else _int_buffer_like(keep, npl)
    _ffi.check(_ffi.lib.brn_flash_attention_paged_varlen_forward(
        pq, pk, pv, _POOL_TYPE[kv_dtype], pks, pvs, pt, pl, pc, total_q, n_seqs, max_kv_len, heads, kv_heads, hd, n_pages, page_size, max_pages, int(bool(causal)),
        float(scale) if scale is not None else 0.0, int(kv_splits), T.ptr_of(y), T.ptr_of(lse) if lse is not None else None, T.ptr_of(ws) if ws is not None else None,
        int(ws.numel() if T._is_torch(ws) else ws.size) if ws is not None else 0, T.ptr_of(plan), int(plan.numel() if T._is_torch(plan) else plan.size), loc,
        T.device_of(keep, device), T.stream_of(keep)))
    res = (y,) + ((lse,) if return_lse else ())
    if return_partials:
        res += ((ws[:S * R * hd].reshape(S, R, hd), ws[S * R * hd:S * R * (hd + 1)].reshape(S, R)) if S > 1 else (None, None),)
    return res[0] if len(res) == 1 else res


def kv_cache_append_varlen(k_new, v_new, cu_seqlens_q, k_pages, v_pages, block_table, kv_lens, kv_dtype=None, k_scale=None, v_scale=None, update_lens=True,
                           plan_workspace=None, device=0):
    """brn_kv_cache_append_varlen: kv_cache_append for a PACKED batch.  k_new, v_new [total_q, kv_heads, head_dim] fp32; cu_seqlens_q
    [n_seqs + 1] int32, clamped by the library as in flash_attention_paged_varlen; token t of sequence b becomes key L_b + t by
    kv_cache_append's rule, padding tokens write nothing.  The pool is written IN PLACE and taken as it is (kv_dtype None float32, "bf16",
    "f16", "e4m3" with k_scale / v_scale).  update_lens as in kv_cache_append: True writes kv_lens in place, False returns new lengths,
    None writes none.  Nothing is read back or checked here.  The rope recipe: rope(q, positions=...) and rope(k_new, positions=...) with
    batch = total_q, seq = 1 and a per-token positions array, then this call."""
    total_q, kv_heads, hd = (int(s) for s in k_new.shape)
    n_pages, page_size = int(k_pages.shape[0]), int(k_pages.shape[1])
    if len(block_table.shape) != 2:
        raise ValueError("block_table must be [n_seqs, max_pages]")
    n_seqs, max_pages = int(block_table.shape[0]), int(block_table.shape[1])
    pk, loc, keep, _ = T.as_arg(k_new)
    pv, vloc, vkeep, _ = T.as_arg(v_new, (total_q, kv_heads, hd))
    (ppk, ppv, pks, pvs), locs, pkeep = _packed_pool_args(kv_dtype, k_pages, v_pages, (n_pages, page_size, kv_heads, hd), k_scale, v_scale, kv_heads)
    pt, tloc, tkeep, _ = _int32_arg(block_table, (n_seqs, max_pages), "block_table")
    pl, lloc, lkeep, _ = _int32_arg(kv_lens, (n_seqs,), "kv_lens")
    pc, cloc, ckeep, _ = _int32_arg(cu_seqlens_q, (n_seqs + 1,), "cu_seqlens_q")
    if any(l != loc for l in locs + [vloc, tloc, lloc, cloc]):
        raise ValueError("k_new, v_new, the pool, the scales, block_table, kv_lens and cu_seqlens_q must live on the same side")
    if update_lens is None:
        out, po = None, None
    elif update_lens:
        if lkeep is not kv_lens and not (T._is_torch(kv_lens) and lkeep.data_ptr() == kv_lens.data_ptr()):
            raise TypeError("update_lens=True needs kv_lens as a contiguous int32 tensor or array (it is written in place)")
        out, po = kv_lens, pl
    else:
        out = _int_buffer_like(lkeep, n_seqs)
        po = T.ptr_of(out)
    # plan_ints depends on n_seqs alone: asked for at the smallest pack, so that no attention-side limit (T_max * kv_heads * S) refuses an append
    npl = flash_attention_paged_varlen_plan(1, n_seqs, 1, 1, 1, 32)[3]
    plan = plan_workspace if plan_workspace is not None else _int_buffer_like(keep, npl)
    _ffi.check(_ffi.lib.brn_kv_cache_append_varlen(pk, pv, pc, total_q, n_seqs, kv_heads, hd, ppk, ppv, _POOL_TYPE[kv_dtype], pks, pvs, pt, pl, po, n_pages, page_size,
                                                   max_pages, T.ptr_of(plan), int(plan.numel() if T._is_torch(plan) else plan.size), loc, T.device_of(keep, device),
                                                   T.stream_of(keep)))
    return out


def patch_merging(x, H, W, norm_g, norm_b, reduction_w, device=0):
    """PatchMerging::forward (swin.rs:491-527): x [B,H*W,C] -> [B, ceil(H/2)*ceil(W/2), 2C]."""
    B, L, Cc = (int(v) for v in x.shape)
    if L != H * W:
        raise ValueError("Input feature has wrong size")
    px, loc, keep, _ = T.as_arg(x)
    hp = [T.host_ptr(a) for a in (norm_g, norm_b, reduction_w)]
    y = T.alloc_like(keep, (B, ((H + 1) // 2) * ((W + 1) // 2), 2 * Cc))
    _ffi.check(_ffi.lib.brn_patch_merging_forward(px, B, H, W, Cc, *[h[0] for h in hp], T.ptr_of(y), loc,
                                                  T.device_of(keep, device), T.stream_of(keep)))
    return y


def _pair(v):
    return (int(v), int(v)) if isinstance(v, int) else (int(v[0]), int(v[1]))


def deform_conv2d(x, offset, weight, bias=None, stride=(1, 1), padding=(0, 0), dilation=(1, 1), mask=None, device=0):
    """torchvision.ops.deform_conv2d's signature over brn_deform_conv2d_offsets_forward (the reference's DeformConv2dConfig,
    deform_conv.rs:120-132): x [B,C,H,W], offset [B, 2*G*kh*kw, Ho, Wo] (the caller's, dy / dx interleaved per (group, tap)), weight
    [O,C,kh,kw], mask [B, G*kh*kw, Ho, Wo] or None (no modulation) -> [B,O,Ho,Wo].  stride / padding / dilation: an int or a (h, w) pair.
    The number of offset groups G is inferred from offset.shape[1].  The limits are the library's (include/birefnet_hip.h)."""
    B, Cc, H, W = (int(v) for v in x.shape)
    O, Ci, kh, kw = (int(v) for v in weight.shape)
    if Ci != Cc:
        raise ValueError("channel mismatch (weight groups are not provided)")
    (sh, sw), (ph, pw), (dh, dw) = _pair(stride), _pair(padding), _pair(dilation)
    oc = int(offset.shape[1])
    if oc < 2 * kh * kw or oc % (2 * kh * kw):
        raise ValueError(f"offset has {oc} channels: not a multiple of 2 * kh * kw = {2 * kh * kw}")
    G = oc // (2 * kh * kw)
    Ho, Wo = int(offset.shape[2]), int(offset.shape[3])
    px, loc, keep, _ = T.as_arg(x)
    po, oloc, okeep, _ = T.as_arg(offset, (B, oc, Ho, Wo))
    pm, mloc, mkeep, _ = T.as_arg(mask, (B, G * kh * kw, Ho, Wo)) if mask is not None else (None, loc, None, None)
    if not (oloc == mloc == loc):
        raise ValueError("x, offset and mask must live on the same side")
    if Ho != (H + 2 * ph - dh * (kh - 1) - 1) // sh + 1 or Wo != (W + 2 * pw - dw * (kw - 1) - 1) // sw + 1:
        raise ValueError(f"offset is {Ho} x {Wo}: not the output size of this geometry")
    pw_, k1 = T.host_ptr(weight)
    pb, k2 = T.host_ptr(bias)
    y = T.alloc_like(keep, (B, O, Ho, Wo))
    _ffi.check(_ffi.lib.brn_deform_conv2d_offsets_forward(px, B, Cc, H, W, po, pm, pw_, pb, O, kh, kw, sh, sw, ph, pw, dh, dw, G, T.ptr_of(y), loc,
                                                          T.device_of(keep, device), T.stream_of(keep)))
    return y


def aspp_deformable(x, tensors, mode="reference_cpu", prefix="", out_channels=None, device=0):
    """ASPPDeformable::new(in_channels, out_channels, vb.pp(prefix)) + forward (aspp.rs:236-333) on an NCHW map; `tensors`: name -> host
    array of the module's weights under `prefix` (SURVEY.md App. A <ASPP>; BasicDecBlk builds it with 64 -> 64).  mode: "reference_cpu"
    (aspp.rs:183-185) or "deformable" (aspp.rs:58-165).  out_channels None = in_channels (aspp.rs:242)."""
    from .birefnet import _named_array
    B, Cc, H, W = (int(v) for v in x.shape)
    oc = int(out_channels) if out_channels else Cc
    arr, keep_w = _named_array(tensors)
    px, loc, keep, _ = T.as_arg(x)
    y = T.alloc_like(keep, (B, oc, H, W))
    m = {"reference_cpu": _ffi.BRN_DEFORM_REFERENCE_CPU, "deformable": _ffi.BRN_DEFORM_DEFORMABLE}[mode]
    _ffi.check(_ffi.lib.brn_aspp_deformable_forward(arr, len(arr), prefix.encode(), Cc, oc, m, px, B, H, W, T.ptr_of(y), loc, T.device_of(keep, device),
                                                    T.stream_of(keep)))
    del keep_w
    return y


def decblk(x, tensors, out_channels, mode="reference_cpu", prefix="", use_aspp=True, inter_channels_adaptive=False, device=0):
    """BasicDecBlk::new(in_channels, out_channels, &DecoderConfig { use_aspp_deformable: use_aspp, inter_channels_adaptive }, vb.pp(prefix))
    + forward (decoder.rs:78-141) on an NCHW map [B,in_channels,H,W] -> [B,out_channels,H,W]; `tensors`: name -> host array of the
    block's weights under `prefix` (SURVEY.md App. A <DecBlk>).  inter_channels = 64, or in_channels // 4 when adaptive (decoder.rs:94-98)."""
    from .birefnet import _named_array
    B, Cc, H, W = (int(v) for v in x.shape)
    arr, keep_w = _named_array(tensors)
    px, loc, keep, _ = T.as_arg(x)
    y = T.alloc_like(keep, (B, int(out_channels), H, W))
    m = {"reference_cpu": _ffi.BRN_DEFORM_REFERENCE_CPU, "deformable": _ffi.BRN_DEFORM_DEFORMABLE}[mode]
    inter = Cc // 4 if inter_channels_adaptive else 64
    _ffi.check(_ffi.lib.brn_decblk_forward(arr, len(arr), prefix.encode(), Cc, int(out_channels), inter, int(bool(use_aspp)), m, px, B, H, W, T.ptr_of(y), loc,
                                           T.device_of(keep, device), T.stream_of(keep)))
    del keep_w
    return y


def linear_residual_layer_norm(x, w, bias, residual, gamma, beta, eps=1e-5, device=0):
    """x_out = x W^T + bias + residual; y_out = LayerNorm(x_out) gamma + beta — swin.rs:310 + :406 + :407 (and :106-107 + the next block's
    norm1) as one call; returns (x_out, y_out), both [M,N]."""
    M, K = (int(v) for v in x.shape)
    N = int(w.shape[0])
    px, loc, keep, _ = T.as_arg(x)
    pr, rloc, rkeep, _ = T.as_arg(residual, (M, N))
    if rloc != loc:
        raise ValueError("x and residual must live on the same side")
    (pw, kw), (pb, kb), (pg, kg), (pbt, kbt) = T.host_ptr(w), T.host_ptr(bias), T.host_ptr(gamma), T.host_ptr(beta)
    xo, yo = T.alloc_like(keep, (M, N)), T.alloc_like(keep, (M, N))
    _ffi.check(_ffi.lib.brn_linear_residual_layer_norm_forward(px, M, K, pw, pb, N, pr, pg, pbt, float(eps), T.ptr_of(xo), T.ptr_of(yo), loc,
                                                               T.device_of(keep, device), T.stream_of(keep)))
    return xo, yo
