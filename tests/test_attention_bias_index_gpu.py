"""window_attention_split_kernel (modes f32_half2, f32_split2) reads the relative position bias through one address per 16-key tile into the
head's reversed table column (csrc/kernels/window_attention_index.h).  Here every (query, key) pair's table word is made visible in the output:
the q rows of the qkv weight and the q bias are ZERO, so a real query's scores are exactly its 144 table words (+ the shift mask), and the
table holds distinct values spread over [-8, 8] — a wrong word for any pair moves that query's softmax weights, and the output, by O(1).
A second case keeps q random.  Geometries (window 12, 2 heads, head_dim 32): 24 x 24 (four whole windows) and 30 x 42 (padded border
windows: packed queries, clamped slots in the last tile), each at shift 0 and 6 (the mask on the last row / column of windows only).
Reference: fp64 numpy, written from swin.rs:147-152 (the bias gather) and swin.rs:266-307 (scale, q k^T, + bias, + mask, softmax, p v) with
the pad / roll / partition of swin.rs:356-401 around it.  Bound: the one tests/test_ops_gpu.py::test_window_attention_split_modes uses for
the mode (relative to max(1, max |ref|))."""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

WS, HEADS, HD = 12, 2, 32
C = HEADS * HD
TOL = {"f32_split2": 1e-4, "f32_half2": 2e-5}        # tests/test_ops_gpu.py::test_window_attention_split_modes
GEOMETRIES = [(24, 24, 0), (24, 24, 6), (30, 42, 0), (30, 42, 6)]


def _weights(zero_q):
    rng = np.random.default_rng(1234)
    w = {"qkv_w": (rng.standard_normal((3 * C, C)) * C ** -0.5).astype(np.float32), "qkv_b": (rng.standard_normal(3 * C) * 0.2).astype(np.float32),
         "proj_w": (rng.standard_normal((C, C)) * C ** -0.5).astype(np.float32), "proj_b": (rng.standard_normal(C) * 0.02).astype(np.float32)}
    if zero_q:
        w["qkv_w"][:C] = 0.0
        w["qkv_b"][:C] = 0.0
    # 529 x heads distinct values, evenly spread over [-8, 8], in random order
    n = (2 * WS - 1) ** 2 * HEADS
    w["table"] = rng.permutation(np.linspace(-8.0, 8.0, n)).astype(np.float32).reshape((2 * WS - 1) ** 2, HEADS)
    return w


def _rel_index():
    t = np.arange(WS * WS)
    ti, tj = t // WS, t % WS
    return (ti[:, None] - ti[None, :] + WS - 1) * (2 * WS - 1) + (tj[:, None] - tj[None, :] + WS - 1)        # swin.rs:182-184


def _reference(x, w, shift):
    x = x.astype(np.float64)
    B, H, W, _ = x.shape
    Hp, Wp = -(-H // WS) * WS, -(-W // WS) * WS
    xp = np.zeros((B, Hp, Wp, C))
    xp[:, :H, :W] = x                                                                                      # swin.rs:359-366
    if shift:
        xp = np.roll(xp, (-shift, -shift), axis=(1, 2))                                                    # swin.rs:371-377
    nWh, nWw = Hp // WS, Wp // WS
    xw = xp.reshape(B, nWh, WS, nWw, WS, C).transpose(0, 1, 3, 2, 4, 5).reshape(-1, WS * WS, C)            # swin.rs:446-459
    b_, n = xw.shape[0], WS * WS
    qkv = xw @ w["qkv_w"].astype(np.float64).T + w["qkv_b"].astype(np.float64)
    qkv = qkv.reshape(b_, n, 3, HEADS, HD).transpose(2, 0, 3, 1, 4)
    q, k, v = qkv[0] * HD ** -0.5, qkv[1], qkv[2]                                                          # swin.rs:278
    attn = q @ k.transpose(0, 1, 3, 2)                                                                     # swin.rs:281
    bias = w["table"].astype(np.float64)[_rel_index().reshape(-1)].reshape(n, n, HEADS).transpose(2, 0, 1)  # swin.rs:147-152
    attn = attn + bias[None]                                                                               # swin.rs:284-285
    if shift:
        img = np.zeros((Hp, Wp))
        cnt = 0
        for hs, he in ((0, Hp - WS), (Hp - WS, Hp - shift), (Hp - shift, Hp)):                             # swin.rs:608-629
            for ws_, we in ((0, Wp - WS), (Wp - WS, Wp - shift), (Wp - shift, Wp)):
                img[hs:he, ws_:we] = cnt
                cnt += 1
        ids = img.reshape(nWh, WS, nWw, WS).transpose(0, 2, 1, 3).reshape(-1, n)
        mask = np.where(ids[:, None, :] != ids[:, :, None], -100.0, 0.0)                                   # swin.rs:651
        nW = mask.shape[0]
        attn = (attn.reshape(b_ // nW, nW, HEADS, n, n) + mask[None, :, None]).reshape(b_, HEADS, n, n)     # swin.rs:288-297
    attn = np.exp(attn - attn.max(-1, keepdims=True))
    attn /= attn.sum(-1, keepdims=True)                                                                    # swin.rs:300
    o = (attn @ v).transpose(0, 2, 1, 3).reshape(b_, n, C)                                                 # swin.rs:303-307
    o = o @ w["proj_w"].astype(np.float64).T + w["proj_b"].astype(np.float64)
    o = o.reshape(B, nWh, nWw, WS, WS, C).transpose(0, 1, 3, 2, 4, 5).reshape(B, Hp, Wp, C)
    if shift:
        o = np.roll(o, (shift, shift), axis=(1, 2))
    return o[:, :H, :W]                                                                                    # swin.rs:387-401


@functools.lru_cache(maxsize=None)
def _case(H, W, shift, zero_q):
    """(x, weights, fp64 reference) of one case: computed once, shared by the modes, never written to"""
    x = np.random.default_rng(100 * H + W).standard_normal((1, H, W, C)).astype(np.float32)
    w = _weights(zero_q)
    ref = _reference(x, w, shift)
    for a in (x, ref, *w.values()):
        a.setflags(write=False)
    return x, w, ref


def _run(mode, x, w, shift):
    from candle_birefnet_amd import ops
    ops.set_compute(mode)
    try:
        return np.asarray(ops.window_attention(x, HEADS, shift, w["qkv_w"], w["qkv_b"], w["proj_w"], w["proj_b"], w["table"]))
    finally:
        ops.set_compute("f32")


def _check(mode, H, W, shift, zero_q):
    x, w, ref = _case(H, W, shift, zero_q)
    y = _run(mode, x, w, shift).astype(np.float64)
    scale = max(1.0, float(np.abs(ref).max()))
    err = float(np.abs(y - ref).max())
    print(f"{mode} {H}x{W} shift {shift} zero_q {int(zero_q)}: max abs err {err:.3e}, bound {TOL[mode] * scale:.3e} (scale {scale:.3g})")
    assert np.isfinite(y).all()
    assert err <= TOL[mode] * scale, f"max abs err {err:.3e} > {TOL[mode] * scale:.3e} (scale {scale:.3g})"


@pytest.mark.parametrize("mode", ["f32_half2", "f32_split2"])
@pytest.mark.parametrize("H,W,shift", GEOMETRIES)
def test_scores_are_the_table_words(gpu, mode, H, W, shift):
    """q = 0: softmax over the bias (and mask) alone — every (query, key) pair must have read its own table word"""
    _check(mode, H, W, shift, True)


@pytest.mark.parametrize("mode", ["f32_half2", "f32_split2"])
@pytest.mark.parametrize("H,W,shift", GEOMETRIES)
def test_random_q_with_spread_table(gpu, mode, H, W, shift):
    _check(mode, H, W, shift, False)


def test_a_wrong_word_would_show():
    """the premise of the q = 0 case, on the reference alone: exchanging two table entries moves the output far beyond the bounds"""
    x, w, ref = _case(24, 24, 0, True)
    w2 = {k: v.copy() for k, v in w.items()}
    w2["table"][[100, 101]] = w2["table"][[101, 100]]
    moved = float(np.abs(_reference(x, w2, 0) - ref).max())
    print(f"two table rows exchanged: reference moves by {moved:.3e}")
    assert moved > 100 * max(TOL.values()) * max(1.0, float(np.abs(ref).max()))
