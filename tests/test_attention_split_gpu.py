"""window_attention_split_kernel (compute modes f32_half2 and f32_split2) on the smallest geometries that reach each of its paths:
the up-front loads from clamped addresses, pad tokens patched from the qkv bias in the K / V rows and in the Q rows, the one-tile-ahead
Q fetch, the shift mask on edge windows only, and two geometries in one launch.  Same entry, same fp64 restatement and same bounds as
tests/test_ops_gpu.py::test_window_attention_split_modes."""
import functools

import numpy as np
import pytest
import torch

import torch_ref as R
from test_ops_gpu import _attn_weights, _close, rnd

pytestmark = pytest.mark.gpu

TOL = {"f32_split2": 1e-4, "f32_half2": 2e-5}      # tests/test_ops_gpu.py::test_window_attention_split_modes
MODEL_TOL = {"f32_split2": 1e-3, "f32_half2": 2e-4}   # tests/test_model_gpu.py::test_pieces_in_every_compute_mode

GEOMETRIES = [
    (1, 12, 12, 1, 0),      # one window, no pad token, no mask; token 143 is the last row of the qkv matrix
    (2, 30, 30, 3, 0),      # padded to 36: 3 x 3 windows, interior and edge windows in one launch, pad tokens in K / V and Q rows, odd head count
    (2, 30, 30, 3, 6),      # + the wrap of shifted sources and the mask on the last row / column of windows only
    (2, 12, 12, 2, 6),      # one (edge) window per image: the last real token of the last image is the very end of the qkv matrix
    (1, 4, 4, 1, 6),        # window token 0 has source (6, 6): a pad token first, clamped to row 0; 16 real tokens of 144
]


@functools.lru_cache(maxsize=None)
def _case(B, H, W, heads, shift):
    C = heads * 32
    w = _attn_weights(C, heads, seed=10)
    x = rnd(B, H, W, C, seed=99)
    ref = R.window_attention_block(torch.from_numpy(x).double(), w, "", heads, 12, shift, torch.float64).numpy()
    ref.setflags(write=False)
    return w, x, ref


def _run(mode, x, w, heads, shift):
    from candle_birefnet_amd import ops
    ops.set_compute(mode)
    try:
        return ops.window_attention(x, heads, shift, w["attn.qkv.weight"], w["attn.qkv.bias"], w["attn.proj.weight"], w["attn.proj.bias"],
                                    w["attn.relative_position_bias_table"])
    finally:
        ops.set_compute("f32")


@pytest.mark.parametrize("mode", ["f32_half2", "f32_split2"])
@pytest.mark.parametrize("B,H,W,heads,shift", GEOMETRIES)
def test_split_attention_paths(gpu, mode, B, H, W, heads, shift):
    """(the qkv matrix is the op's own arena allocation, directly followed by the attention output: a read past its end or before its
    start would show as a wrong value here, nothing is provoked)"""
    w, x, ref = _case(B, H, W, heads, shift)
    y = _run(mode, x, w, heads, shift)
    err = float(np.abs(np.asarray(y, np.float64) - ref).max())
    print(f"split attention {mode} B{B} {H}x{W} h{heads} s{shift}: max abs err {err:.2e}, |ref| max {np.abs(ref).max():.2f}")
    assert np.isfinite(y).all()
    _close(y, ref, tol=TOL[mode])
    y2 = _run(mode, x, w, heads, shift)
    np.testing.assert_array_equal(y, y2)        # the same call twice: the same bits


@functools.lru_cache(maxsize=None)
def _model_case():
    import candle_birefnet_amd as cb
    cfg = cb.BiRefNetConfig(deform_mode="reference_cpu")
    cfg.swin.depths = [2, 2, 2, 2]
    w = cb.synth_weights(cb.birefnet_weight_spec(cfg), seed=42)
    x = cb.synth_input(1, 160, 160)
    ref = R.forward_logits(x, w, cfg, torch.float64).numpy()
    ref.setflags(write=False)
    return cfg, w, x, ref


@pytest.mark.parametrize("mode", ["f32_half2", "f32_split2"])
def test_split_attention_two_geometries_in_one_launch(gpu, mode):
    """a 160 x 160 image (the decoder needs a multiple of 32): the co-batched backbone pass (swin_forward_multi) launches stage 0 on the
    40 x 40 map (padded to 48: 16 windows) and the 20 x 20 map (padded to 24: 4 windows) together, shifted and not.  The second geometry's workgroups must work on their own parameter
    block: computed from the first one's qkv rows and sizes the half-scale features — a quarter of the decoder's input — are wrong by
    their own magnitude, far beyond the mode's bound against the fp64 restatement."""
    import candle_birefnet_amd as cb
    cfg, w, x, ref = _model_case()
    m = cb.BiRefNet.new(cfg, cb.VarBuilder.from_tensors(w), compute=mode)
    try:
        y = np.asarray(m.forward_logits(x))
        y2 = np.asarray(m.forward_logits(x))
    finally:
        m.close()
    err = float(np.abs(y.astype(np.float64) - ref).max())
    print(f"two geometries {mode}: max abs err {err:.2e}, |ref| max {np.abs(ref).max():.2f}")
    assert np.isfinite(y).all()
    assert err <= MODEL_TOL[mode] * max(1.0, float(np.abs(ref).max()))
    np.testing.assert_array_equal(y, y2)
