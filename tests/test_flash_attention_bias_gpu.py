"""brn_flash_attention_bias_forward on the GPU: flash_attention_with_bias / flash_attention_with_repeating_bias (swin.rs:243, 252) on
sequences of any length, with the causal flag, against float64 softmax(scale * (q k^T + bias[b % n_bias]) [causal exclusion]) v.

Bounds: the project's own, from tests/test_flash_attention_gpu.py.  fp32 modes: max |err| <= 3e-5 max(1, max |ref|).  16-bit modes: the
reference takes q, k, v rounded to the 16-bit type and the bias unrounded (the kernels never round it), so the only rounding it lacks is
that of the softmax numerators before P v -> max |err| <= u max |v| + 3e-5 max(1, max |ref|), u = 2^-8 (bf16) or 2^-11 (fp16).
tests/test_flash_attention_bias_cpu.py records that a numpy emulation of the tile-wise algorithm stays inside both on these inputs
(worst error / bound 0.08 in fp32, 0.22 in the 16-bit types) and that every case's with-bias and bias-free references differ by more
than 10 x the bound."""
import time

import numpy as np
import pytest
import torch

import flash_attention_bias_cases as B

pytestmark = pytest.mark.gpu


def _bound(ref, v, mode):
    return B.f32_bound(ref) if mode == "f32" else B.s16_bound(ref, v, mode)


def _call(q, k, v, bias, layout, causal=False, mode="f32", scale=None):
    from candle_birefnet_amd import ops
    ops.set_compute(mode)
    try:
        return ops.flash_attention(q, k, v, causal=bool(causal), scale=scale, layout=layout, bias=bias)
    finally:
        ops.set_compute("f32")


def _run(shape, mode="f32"):
    q, k, v, bias = B.make_inputs(shape)
    return _call(q, k, v, bias, B.LAYOUT[shape], shape[5], mode, B.case_scale(shape) or None)


_F32 = {}


def _f32_result(shape):
    """mode f32's result of a case, computed once (the other fp32-class modes are compared with it bit for bit)"""
    if shape not in _F32:
        _F32[shape] = _run(shape)
    return _F32[shape]


def _err(y, ref):
    return float(np.abs(np.asarray(y, np.float64) - ref).max())


@pytest.mark.parametrize("shape", B.SHAPES, ids=B.case_id)
def test_flash_attention_bias_f32_parity(gpu, shape):
    y = _f32_result(shape)
    ref = B.case_reference(shape)
    print(f"flash attention bias f32 {B.case_id(shape)}: max abs err {_err(y, ref):.3e}, bound {B.f32_bound(ref):.3e}")
    assert y.shape == ref.shape and np.isfinite(y).all()
    assert _err(y, ref) <= B.f32_bound(ref)


@pytest.mark.parametrize("mode", ["f32_split3", "f32_half2"])
@pytest.mark.parametrize("shape", B.SHAPES, ids=B.case_id)
def test_flash_attention_bias_plane_modes_are_the_f32_kernel(gpu, shape, mode):
    """one exact fp32 kernel behind every mode that is not bf16 / f16: the same bits"""
    np.testing.assert_array_equal(_run(shape, mode), _f32_result(shape))


@pytest.mark.parametrize("s16", ["bf16", "f16"])
@pytest.mark.parametrize("shape", B.SHAPES, ids=B.case_id)
def test_flash_attention_bias_s16_parity(gpu, shape, s16):
    y = _run(shape, s16)
    ref = B.case_reference(shape, s16)
    v = B.make_inputs(shape)[2]
    print(f"flash attention bias {s16} {B.case_id(shape)}: max abs err {_err(y, ref):.3e}, bound {B.s16_bound(ref, v, s16):.3e}")
    assert y.shape == ref.shape and np.isfinite(y).all()
    assert _err(y, ref) <= B.s16_bound(ref, v, s16)


@pytest.mark.parametrize("mode", ["f32", "bf16"])
@pytest.mark.parametrize("shape", [(2, 300, 300, 3, 64, 0), (2, 300, 300, 2, 64, 1)], ids=["300x300x3x64", "300x300x2x64-causal"])
def test_zero_bias_is_the_bias_free_op_bit_for_bit(gpu, shape, mode):
    """the bias is the initial accumulator of q k^T, so an all-zero bias leaves every bit of brn_flash_attention_forward's result; and
    bias NULL with n_bias 0 runs the bias-free kernels"""
    from candle_birefnet_amd import _ffi, ops
    batch, sq, skv, heads, hd, causal = shape
    rng = np.random.default_rng(11)
    q, k, v = (rng.standard_normal((batch, s, heads, hd)).astype(np.float32) for s in (sq, skv, skv))
    free = _call(q, k, v, None, "bshd", causal, mode)
    zero = _call(q, k, v, np.zeros((1, heads, sq, skv), np.float32), "bshd", causal, mode)
    np.testing.assert_array_equal(zero, free)
    y = np.full_like(q, np.nan)
    ops.set_compute(mode)
    try:
        st, msg = B.raw_call(_ffi.lib, q, k, v, batch, sq, skv, heads, hd, 0, causal, None, 0, 0.0, y)
    finally:
        ops.set_compute("f32")
    assert st == 0, msg
    np.testing.assert_array_equal(y, free)


@pytest.mark.parametrize("shape", [(2, 300, 300, 3, 64, 0, 1, "std"), (8, 256, 256, 3, 32, 0, 4, "swin16")], ids=B.case_id)
def test_the_bias_reaches_the_result(gpu, shape):
    """the result is the with-bias reference's and NOT the bias-free one's: the two references differ by more than 10 x the bound"""
    v = B.make_inputs(shape)[2]
    for mode in ("f32", "bf16", "f16"):
        s16 = None if mode == "f32" else mode
        ref, bare = B.case_reference(shape, s16), B.case_reference(shape, s16, with_bias=False)
        bound = _bound(ref, v, mode)
        y = _f32_result(shape) if s16 is None else _run(shape, mode)
        moved = _err(y, bare)
        print(f"{B.case_id(shape)} {mode}: differs from the bias-free reference by {moved:.3e}, bound {bound:.3e}")
        assert float(np.abs(bare - ref).max()) > 10 * bound, "the inputs never reach the biased regime"
        assert moved > 10 * bound and _err(y, ref) <= bound


@pytest.mark.parametrize("mode", ["f32", "bf16"])
def test_repeating_form_and_batch_independence(gpu, mode):
    """(4, 145, 145, 3, 32) over 2 patterns: entry b equals the batch-1, n_bias-1 call on bias[b % 2] bit for bit, and a repeated call
    repeats its bits"""
    shape = (4, 145, 145, 3, 32, 0, 2, "std")
    q, k, v, bias = B.make_inputs(shape)
    y = _f32_result(shape) if mode == "f32" else _run(shape, mode)
    np.testing.assert_array_equal(_run(shape, mode), y)
    for b in range(4):
        one = _call(q[b:b + 1], k[b:b + 1], v[b:b + 1], bias[b % 2:b % 2 + 1], B.LAYOUT[shape], mode=mode)
        np.testing.assert_array_equal(y[b:b + 1], one)


@pytest.mark.parametrize("mode", ["f32", "bf16"])
def test_layouts_agree(gpu, mode):
    """[batch, seq, heads, head_dim] and [batch, heads, seq, head_dim] q / k / v with the SAME (heads-major) bias array: the same bits
    after the host transpose (a square case and a cross case)"""
    for shape in ((2, 300, 300, 3, 64, 0, 1, "std"), (2, 5, 301, 2, 64, 0, 1, "std")):
        q, k, v, bias = B.make_inputs(shape)
        assert B.LAYOUT[shape] == "bshd"
        y = _call(q, k, v, bias, "bshd", mode=mode)
        qt, kt, vt = (np.ascontiguousarray(a.transpose(0, 2, 1, 3)) for a in (q, k, v))
        yt = _call(qt, kt, vt, bias, "bhsd", mode=mode)
        np.testing.assert_array_equal(yt.transpose(0, 2, 1, 3), y)


def test_minus_infinity_padding(gpu):
    """a -inf bias entry excludes its key: per pattern the result is, within the bound, that of the call on k, v and the bias truncated
    to the finite keys; every value is finite"""
    shape = (2, 70, 200, 2, 64, 0, 2, "pad")
    q, k, v, bias = B.make_inputs(shape)
    assert B.LAYOUT[shape] == "bshd"
    for mode in ("f32", "bf16", "f16"):
        y = _f32_result(shape) if mode == "f32" else _run(shape, mode)
        ref = B.case_reference(shape, None if mode == "f32" else mode)
        assert np.isfinite(y).all() and _err(y, ref) <= _bound(ref, v, mode)
        for pattern, first in enumerate(B.PAD_FROM):
            b = slice(pattern, pattern + 1)
            cut = _call(q[b], np.ascontiguousarray(k[b, :first]), np.ascontiguousarray(v[b, :first]), np.ascontiguousarray(bias[b, :, :, :first]), "bshd",
                        mode=mode)
            d = _err(y[b], cut.astype(np.float64))
            print(f"-inf padding {mode} pattern {pattern}: differs from the truncated call by {d:.3e}, bound {_bound(ref[b], v, mode):.3e}")
            assert d <= _bound(ref[b], v, mode)


def test_agrees_with_attention_forward(gpu):
    """brn_attention_forward at (8, 6, 144, 32) with a 4-pattern bias: each is within one bound of the same float64 result, so they
    agree within twice the bound — fp32, and bf16"""
    from candle_birefnet_amd import ops
    rng = np.random.default_rng(21)
    q, k, v = (rng.standard_normal((8, 6, 144, 32)).astype(np.float32) for _ in range(3))
    bias = (rng.standard_normal((4, 6, 144, 144)) * np.sqrt(32.0)).astype(np.float32)
    for mode in ("f32", "bf16"):
        ops.set_compute(mode)
        try:
            short = ops.attention_with_repeating_bias(q, k, v, bias, 4)
        finally:
            ops.set_compute("f32")
        y = _call(q, k, v, bias, "bhsd", mode=mode)
        ref = B.reference(*((B.round_s16(a, mode) for a in (q, k, v)) if mode != "f32" else (q, k, v)), bias)
        bound = _bound(ref, v, mode)
        diff = _err(y, short.astype(np.float64))
        print(f"flash bias vs short attention {mode}: max abs diff {diff:.3e}, bound {2 * bound:.3e}")
        assert _err(y, ref) <= bound and _err(short, ref) <= bound
        assert diff <= 2 * bound


@pytest.mark.parametrize("shape", [s for s in B.SHAPES if s[5]], ids=B.case_id)
def test_causal_row_zero_is_v0(gpu, shape):
    """query 0 sees key 0 alone, whatever its bias: its row is v[0], to the bound"""
    v = B.make_inputs(shape)[2]
    sel = (slice(None), 0) if B.LAYOUT[shape] == "bshd" else (slice(None), slice(None), 0)
    for mode in ("f32", "bf16", "f16"):
        y = _f32_result(shape) if mode == "f32" else _run(shape, mode)
        want = v[sel].astype(np.float64) if mode == "f32" else B.round_s16(v[sel], mode)
        assert _err(y[sel], want) <= _bound(want, v, mode), mode


def test_bias_offsets_past_2_31(gpu):
    """a fault of 32-bit index arithmetic on the bias shows only past 2^31 elements: 2112 heads x 1024 x 1024 = 2.21e9 bias floats
    (8.9 GB) on the device, q / k / v [1, 2112, 1024, 32], mode bf16.  The first and the last head must carry the bits of a one-head call
    on that head's slices (the bits do not depend on the grid), and the last 64 rows of the last head must meet the float64 reference."""
    from candle_birefnet_amd import ops
    heads, seq, hd = 2112, 1024, 32
    assert heads * seq * seq > 2 ** 31
    g = torch.Generator(device="cuda").manual_seed(6)
    q, k, v = (torch.randn(1, heads, seq, hd, device="cuda", generator=g) for _ in range(3))
    bias = torch.randn(1, heads, seq, seq, device="cuda", generator=g)
    ops.set_compute("bf16")
    try:
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        y = ops.flash_attention(q, k, v, layout="bhsd", bias=bias)
        torch.cuda.synchronize()
        print(f"bias offsets past 2^31: the {heads}-head call took {time.perf_counter() - t0:.3f} s")
        for h in (0, heads - 1):
            one = ops.flash_attention(*(a[:, h:h + 1].contiguous() for a in (q, k, v)), layout="bhsd", bias=bias[:, h:h + 1].contiguous())
            assert torch.equal(y[:, h:h + 1], one), h
    finally:
        ops.set_compute("f32")
    qs, ks, vs = (B.round_s16(a[:, -1:].cpu().numpy(), "bf16") for a in (q[:, :, -64:], k, v))
    ref = B.reference(qs, ks, vs, bias[:, -1:, -64:].cpu().numpy())
    assert _err(y[:, -1:, -64:].cpu().numpy(), ref) <= B.s16_bound(ref, vs, "bf16")


@pytest.mark.parametrize("shape", [(2, 17, 17, 3, 64, 0, 2, "std"), (1, 257, 257, 2, 128, 1, 1, "std")], ids=B.case_id)
def test_device_tensors(gpu, shape):
    """q, k, v and the bias as torch tensors on the GPU: y comes back on the device with the bits of the host-buffer call"""
    from candle_birefnet_amd import ops
    q, k, v, bias = B.make_inputs(shape)
    dq, dk, dv, db = (torch.from_numpy(np.array(a)).cuda() for a in (q, k, v, bias))
    y = ops.flash_attention(dq, dk, dv, causal=bool(shape[5]), layout=B.LAYOUT[shape], bias=db)
    assert y.is_cuda and tuple(y.shape) == q.shape
    np.testing.assert_array_equal(y.cpu().numpy(), _f32_result(shape))


def test_refusals_leave_no_stale_error(gpu):
    """every limit of the header is status 1 with a message naming it, and the valid call that follows succeeds with unchanged bits"""
    from candle_birefnet_amd import _ffi
    shape = (2, 17, 17, 3, 64, 0, 2, "std")
    for name, args, word in B.refusals():
        st, msg = B.raw_call(_ffi.lib, *args)
        assert st == 1 and msg.startswith("flash attention bias:") and word in msg, (name, st, msg)
        np.testing.assert_array_equal(_run(shape), _f32_result(shape))
