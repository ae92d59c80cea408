"""brn_attention_forward on the GPU: the q/k/v attention with an additive / repeating bias that candle's WindowAttention hands to
flash_attention_with_bias / flash_attention_with_repeating_bias (swin.rs:243, 252; examples/test_flash_bias.rs), against
forward_standard (swin.rs:266-311, without the projection) in float64.

Bounds.  fp32 modes: the suite's fp32 figure, max |err| <= 3e-5 max(1, max |ref|) (tests/test_ops_gpu.py _close): products and sums
are fp32 fmaf chains.  16-bit modes: the reference takes q, k, v rounded to the 16-bit type, so the only rounding it lacks is that of
the softmax numerators before P v: each carries a relative error <= u / 2, which moves the normalised output by <= u / 2 max |v| through
the numerator (and by as much again through the denominator where the row sum is taken from the rounded values; this kernel sums the
unrounded ones) -> max |err| <= u max |v| + 3e-5 max(1, max |ref|), u = 2^-8 (bf16) or 2^-11 (fp16).
tests/test_attention_bias_cpu.py records that these inputs leave an emulation of that rounding inside u max |v|."""
import numpy as np
import pytest
import torch

import attention_bias_cases as A
import torch_ref as R

pytestmark = pytest.mark.gpu

F32_TOL = 3e-5


def _f32_bound(ref):
    return F32_TOL * max(1.0, float(np.abs(ref).max()))


def _s16_bound(ref, v, s16):
    return A.S16_ULP[s16] * float(np.abs(v).max()) + _f32_bound(ref)


def _run(shape, mode="f32", mask_value=-100.0):
    from candle_birefnet_amd import ops
    q, k, v, bias = A.make_inputs(shape, mask_value=mask_value)
    ops.set_compute(mode)
    try:
        return ops.attention(q, k, v, bias)
    finally:
        ops.set_compute("f32")


_F32 = {}


def _f32_result(shape):
    """mode f32's result of a case, computed once (the split modes are compared with it bit for bit)"""
    if shape not in _F32:
        _F32[shape] = _run(shape)
    return _F32[shape]


@pytest.mark.parametrize("shape", A.SHAPES)
def test_attention_f32_parity(gpu, shape):
    y = _f32_result(shape)
    ref = A.case_reference(shape)
    err = float(np.abs(np.asarray(y, np.float64) - ref).max())
    print(f"attention f32 {shape} qk std {A.QK_STD[shape]}: max abs err {err:.3e}, bound {_f32_bound(ref):.3e}")
    assert y.shape == ref.shape and np.isfinite(y).all()
    assert err <= _f32_bound(ref)


@pytest.mark.parametrize("mode", ["f32_split3", "f32_half2"])
@pytest.mark.parametrize("shape", A.SHAPES)
def test_attention_plane_modes_are_the_f32_kernel(gpu, shape, mode):
    """exact fp32 attention between the mode's own GEMMs: the same kernel, the same bits"""
    np.testing.assert_array_equal(_run(shape, mode), _f32_result(shape))


@pytest.mark.parametrize("s16", ["bf16", "f16"])
@pytest.mark.parametrize("shape", A.SHAPES)
def test_attention_s16_parity(gpu, shape, s16):
    y = _run(shape, s16)
    ref = A.case_reference(shape, s16)
    v = A.make_inputs(shape)[2]
    err = float(np.abs(np.asarray(y, np.float64) - ref).max())
    print(f"attention {s16} {shape} qk std {A.QK_STD[shape]}: max abs err {err:.3e}, bound {_s16_bound(ref, v, s16):.3e}")
    assert np.isfinite(y).all()
    assert err <= _s16_bound(ref, v, s16)


def test_attention_masked_entries_are_exact(gpu):
    """the lowered bias entries at -200 / scale instead of -100 / scale: exp(-100) is below half an ulp of the row's largest weight, so
    the fp32 result keeps every bit and the 16-bit results stay inside their bound of the -100 reference"""
    shape = (8, 6, 144, 8)
    ref, v = A.case_reference(shape), A.make_inputs(shape)[2]
    unmasked = A.case_reference(shape, mask_value=0.0)
    moved = float(np.abs(unmasked - ref).max())
    assert moved > 10 * _s16_bound(ref, v, "bf16"), "the inputs never reach the masked regime"
    assert float(np.abs(A.case_reference(shape, mask_value=-200.0) - ref).max()) < 1e-30
    y100, y200 = _f32_result(shape), _run(shape, mask_value=-200.0)
    assert np.isfinite(y200).all()
    np.testing.assert_array_equal(y200, y100)
    for s16 in ("bf16", "f16"):
        y = _run(shape, s16, mask_value=-200.0)
        err = float(np.abs(np.asarray(y, np.float64) - A.case_reference(shape, s16)).max())
        print(f"attention {s16}, mask -200: max abs err {err:.3e}, bound {_s16_bound(ref, v, s16):.3e}; removing the mask moves the reference by {moved:.3e}")
        assert np.isfinite(y).all() and err <= _s16_bound(ref, v, s16)


@pytest.mark.parametrize("mode", ["f32", "bf16"])
def test_attention_batch_independence(gpu, mode):
    """entry b of the 8-entry call equals the 1-entry call on entry b bit for bit, and a repeated call repeats its bits"""
    from candle_birefnet_amd import ops
    shape = (8, 6, 144, 1)
    q, k, v, bias = A.make_inputs(shape)
    ops.set_compute(mode)
    try:
        y = ops.attention(q, k, v, bias)
        y2 = ops.attention(q, k, v, bias)
        singles = [ops.attention(q[b:b + 1], k[b:b + 1], v[b:b + 1], bias) for b in range(shape[0])]
    finally:
        ops.set_compute("f32")
    np.testing.assert_array_equal(y, y2)
    for b in range(shape[0]):
        np.testing.assert_array_equal(y[b:b + 1], singles[b])


def _block_weights(C, heads, ws, seed):
    """_attn_weights of tests/test_ops_gpu.py for a window side ws"""
    rnd = lambda *s, seed, std: (np.random.default_rng(seed).standard_normal(s) * std).astype(np.float32)
    return {"attn.qkv.weight": rnd(3 * C, C, seed=seed, std=C ** -0.5), "attn.qkv.bias": rnd(3 * C, seed=seed + 1, std=0.2),
            "attn.proj.weight": rnd(C, C, seed=seed + 2, std=C ** -0.5), "attn.proj.bias": rnd(C, seed=seed + 3, std=0.02),
            "attn.relative_position_bias_table": rnd((2 * ws - 1) ** 2, heads, seed=seed + 4, std=0.5)}


@pytest.mark.parametrize("S,ws,shift", [(24, 12, 0), (24, 12, 6), (14, 7, 0), (14, 7, 3)])
def test_attention_agrees_with_the_fused_block(gpu, S, ws, shift):
    """candle's WindowAttention with only the flash call swapped (swin.rs:226-258) against brn_window_attention_forward: roll, window
    partition and the qkv Linear on the host side of the op, the relative-position gather (swin.rs:166-210) plus the -100 region mask
    (swin.rs:603-655) as the pre-scaled bias, the op, then proj, window reverse and un-roll.  Each path is within 3e-5 of the same
    float64 result, so they agree to 6e-5 max(1, max |ref|).  This pins b % n_bias to the model's window order."""
    from candle_birefnet_amd import ops
    B, heads = 2, 3
    C, N, nWs = heads * A.HD, ws * ws, S // ws
    nW = nWs * nWs
    w = _block_weights(C, heads, ws, seed=30)
    x = (np.random.default_rng(77).standard_normal((B, S, S, C))).astype(np.float32)
    fused = ops.window_attention(x, heads, shift, w["attn.qkv.weight"], w["attn.qkv.bias"], w["attn.proj.weight"], w["attn.proj.bias"],
                                 w["attn.relative_position_bias_table"], window_size=ws)
    xs = np.roll(x, (-shift, -shift), axis=(1, 2)) if shift else x
    xw = xs.reshape(B, nWs, ws, nWs, ws, C).transpose(0, 1, 3, 2, 4, 5).reshape(B * nW * N, C)
    qkv = ops.linear(np.ascontiguousarray(xw), w["attn.qkv.weight"], w["attn.qkv.bias"])
    qkv = qkv.reshape(B * nW, N, 3, heads, A.HD).transpose(2, 0, 3, 1, 4)
    q, k, v = (np.ascontiguousarray(qkv[i]) for i in range(3))
    table = torch.from_numpy(w["attn.relative_position_bias_table"]).double()
    bias = table[R.rel_index(ws).reshape(-1)].reshape(N, N, heads).permute(2, 0, 1).unsqueeze(0)        # [1, heads, N, N]
    if shift:
        bias = bias + R.attn_mask(S, S, ws, shift, torch.float64).unsqueeze(1)                         # [nW, heads, N, N]
    scaled_bias = (bias / A.SCALE).float().numpy()
    o = ops.attention_with_repeating_bias(q, k, v, scaled_bias, nW if shift else 1)
    o = np.ascontiguousarray(o.transpose(0, 2, 1, 3)).reshape(B * nW * N, C)
    o = ops.linear(o, w["attn.proj.weight"], w["attn.proj.bias"])
    o = o.reshape(B, nWs, nWs, ws, ws, C).transpose(0, 1, 3, 2, 4, 5).reshape(B, S, S, C)
    if shift:
        o = np.roll(o, (shift, shift), axis=(1, 2))
    err = float(np.abs(o.astype(np.float64) - fused.astype(np.float64)).max())
    bound = 2 * F32_TOL * max(1.0, float(np.abs(fused).max()))
    print(f"narrow seam vs fused block, {S}x{S} window {ws} shift {shift}: max abs diff {err:.3e}, bound {bound:.3e}")
    assert err <= bound


def test_attention_device_tensors(gpu):
    """q, k, v and the bias as torch tensors on the GPU: y comes back on the device with the bits of the host-buffer call"""
    from candle_birefnet_amd import ops
    shape = (4, 2, 17, 2)
    q, k, v, bias = A.make_inputs(shape)
    dq, dk, dv, db = (torch.from_numpy(np.array(a)).cuda() for a in (q, k, v, bias))
    y = ops.attention_with_repeating_bias(dq, dk, dv, db, shape[3])
    assert y.is_cuda and tuple(y.shape) == q.shape
    np.testing.assert_array_equal(y.cpu().numpy(), _f32_result(shape))


def test_attention_refusals_leave_no_stale_error(gpu):
    """every limit of the header is status 1 with a message naming it, and the valid call that follows succeeds"""
    from candle_birefnet_amd import _ffi, ops
    shape = (2, 4, 16, 1)
    q, k, v, bias = A.make_inputs(shape)
    for name, args, word in A.refusals():
        st, msg = A.raw_call(_ffi.lib, *args)
        assert st == 1 and word in msg, (name, st, msg)
        np.testing.assert_array_equal(ops.attention_with_bias(q, k, v, bias), _f32_result(shape))
