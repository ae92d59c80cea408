"""brn_flash_attention_forward on the GPU: the plain flash_attention(&q, &k, &v, causal) of examples/bench_flash_attn.rs:39-53 — long
sequences, head_dim 32 / 64 / 128, both layouts, the causal mask — against standard_attention (bench_flash_attn.rs:89-95) in float64.

Bounds: the project's own, from tests/test_attention_bias_gpu.py.  fp32 modes: max |err| <= 3e-5 max(1, max |ref|).  16-bit modes: the
reference takes q, k, v rounded to the 16-bit type, so the only rounding it lacks is that of the softmax numerators before P v: each
carries a relative error <= u / 2 — also when it is rounded relative to a running maximum and later multiplied by fp32 rescale factors —
which moves the normalised output by <= u / 2 max |v| through the numerator (the row sum is taken from the unrounded ones)
-> max |err| <= u max |v| + 3e-5 max(1, max |ref|), u = 2^-8 (bf16) or 2^-11 (fp16).
tests/test_flash_attention_cpu.py records that a numpy emulation of the tile-wise algorithm stays inside both on these inputs."""
import numpy as np
import pytest
import torch

import attention_bias_cases as AB
import flash_attention_cases as A

pytestmark = pytest.mark.gpu

F32_TOL = 3e-5


def _f32_bound(ref):
    return F32_TOL * max(1.0, float(np.abs(ref).max()))


def _s16_bound(ref, v, s16):
    return A.S16_ULP[s16] * float(np.abs(v).max()) + _f32_bound(ref)


def _call(q, k, v, layout, causal=False, mode="f32", scale=None):
    from candle_birefnet_amd import ops
    ops.set_compute(mode)
    try:
        return ops.flash_attention(q, k, v, causal=bool(causal), scale=scale, layout=layout)
    finally:
        ops.set_compute("f32")


def _run(shape, mode="f32"):
    return _call(*A.make_inputs(shape), shape[5], shape[6], mode, A.case_scale(shape) or None)


_F32 = {}


def _f32_result(shape):
    """mode f32's result of a case, computed once (the other fp32-class modes are compared with it bit for bit)"""
    if shape not in _F32:
        _F32[shape] = _run(shape)
    return _F32[shape]


@pytest.mark.parametrize("shape", A.SHAPES, ids=A.case_id)
def test_flash_attention_f32_parity(gpu, shape):
    y = _f32_result(shape)
    ref = A.case_reference(shape)
    err = float(np.abs(np.asarray(y, np.float64) - ref).max())
    print(f"flash attention f32 {A.case_id(shape)}: max abs err {err:.3e}, bound {_f32_bound(ref):.3e}")
    assert y.shape == ref.shape and np.isfinite(y).all()
    assert err <= _f32_bound(ref)


@pytest.mark.parametrize("mode", ["f32_split3", "f32_half2"])
@pytest.mark.parametrize("shape", A.SHAPES, ids=A.case_id)
def test_flash_attention_plane_modes_are_the_f32_kernel(gpu, shape, mode):
    """one exact fp32 kernel behind every mode that is not bf16 / f16: the same bits"""
    np.testing.assert_array_equal(_run(shape, mode), _f32_result(shape))


@pytest.mark.parametrize("s16", ["bf16", "f16"])
@pytest.mark.parametrize("shape", A.SHAPES, ids=A.case_id)
def test_flash_attention_s16_parity(gpu, shape, s16):
    y = _run(shape, s16)
    ref = A.case_reference(shape, s16)
    v = A.make_inputs(shape)[2]
    err = float(np.abs(np.asarray(y, np.float64) - ref).max())
    print(f"flash attention {s16} {A.case_id(shape)}: max abs err {err:.3e}, bound {_s16_bound(ref, v, s16):.3e}")
    assert y.shape == ref.shape and np.isfinite(y).all()
    assert err <= _s16_bound(ref, v, s16)


@pytest.mark.parametrize("mode", ["f32", "bf16"])
def test_flash_attention_layouts_agree(gpu, mode):
    """[batch, seq, heads, head_dim] and [batch, heads, seq, head_dim] go through one kernel on strides: the same bits after the host
    transpose (the second case is a cross shape, so that q's and k's strides differ)"""
    for shape in ((2, 300, 300, 3, 128, "bshd", 0), (2, 5, 300, 2, 64, "bshd", 0)):
        q, k, v = A.make_inputs(shape)
        y = _call(q, k, v, "bshd", mode=mode)
        qt, kt, vt = (np.ascontiguousarray(a.transpose(0, 2, 1, 3)) for a in (q, k, v))
        yt = _call(qt, kt, vt, "bhsd", mode=mode)
        np.testing.assert_array_equal(yt.transpose(0, 2, 1, 3), y)


@pytest.mark.parametrize("mode", ["f32", "bf16"])
@pytest.mark.parametrize("layout", ["bshd", "bhsd"])
def test_flash_attention_batch_independence(gpu, mode, layout):
    """entry b of a batch-4 call equals the batch-1 call on entry b bit for bit, and a repeated call repeats its bits"""
    rng = np.random.default_rng(77)
    shp = (4, 150, 3, 64) if layout == "bshd" else (4, 3, 150, 64)
    q, k, v = (rng.standard_normal(shp).astype(np.float32) for _ in range(3))
    y = _call(q, k, v, layout, True, mode)
    y2 = _call(q, k, v, layout, True, mode)
    np.testing.assert_array_equal(y, y2)
    for b in range(4):
        np.testing.assert_array_equal(y[b:b + 1], _call(q[b:b + 1], k[b:b + 1], v[b:b + 1], layout, True, mode))


@pytest.mark.parametrize("shape", [s for s in A.SHAPES if s[6]], ids=A.case_id)
def test_flash_attention_causal_row_zero_is_v0(gpu, shape):
    """query 0 sees key 0 alone: its row is v[0], to the bound"""
    q, k, v = A.make_inputs(shape)
    sel = (slice(None), 0) if shape[5] == "bshd" else (slice(None), slice(None), 0)
    for mode in ("f32", "bf16", "f16"):
        y = _f32_result(shape) if mode == "f32" else _run(shape, mode)
        want = v[sel] if mode == "f32" else A.round_s16(v[sel], mode)
        bound = _f32_bound(want) if mode == "f32" else _s16_bound(want, v, mode)
        assert float(np.abs(y[sel].astype(np.float64) - want).max()) <= bound, mode


def test_flash_attention_causal_reaches_the_masked_regime(gpu):
    """the causal result is the causal reference's and NOT the unmasked one's: the two references differ by more than 10x the bound"""
    shape = (2, 300, 300, 2, 64, "bshd", 1)
    v = A.make_inputs(shape)[2]
    for mode in ("f32", "bf16", "f16"):
        s16 = None if mode == "f32" else mode
        ref, unmasked = A.case_reference(shape, s16), A.case_reference(shape, s16, causal=0)
        bound = _f32_bound(ref) if s16 is None else _s16_bound(ref, v, s16)
        y = (_f32_result(shape) if s16 is None else _run(shape, mode)).astype(np.float64)
        moved = float(np.abs(y - unmasked).max())
        print(f"causal {mode}: differs from the non-causal reference by {moved:.3e}, bound {bound:.3e}")
        assert float(np.abs(unmasked - ref).max()) > 10 * bound, "the inputs never reach the masked regime"
        assert moved > 10 * bound and float(np.abs(y - ref).max()) <= bound


def test_flash_attention_agrees_with_attention_forward(gpu):
    """brn_attention_forward without a bias at (8, 6, 144, 32), BHSD: each is within one bound of the same float64 result, so they
    agree within twice the bound — fp32, and bf16"""
    from candle_birefnet_amd import ops
    ab = (8, 6, 144, 1)
    q, k, v, _ = AB.make_inputs(ab)
    for mode in ("f32", "bf16"):
        ops.set_compute(mode)
        try:
            short = ops.attention(q, k, v)
        finally:
            ops.set_compute("f32")
        y = _call(q, k, v, "bhsd", mode=mode)
        ref = A.reference(*((AB.round_s16(a, mode) for a in (q, k, v)) if mode != "f32" else (q, k, v)))
        bound = _f32_bound(ref) if mode == "f32" else _s16_bound(ref, v, mode)
        diff = float(np.abs(y.astype(np.float64) - short.astype(np.float64)).max())
        print(f"flash vs short attention {mode}: max abs diff {diff:.3e}, bound {2 * bound:.3e}")
        assert float(np.abs(y.astype(np.float64) - ref).max()) <= bound
        assert diff <= 2 * bound


def test_flash_attention_offsets_past_2_31(gpu):
    """a fault of 32-bit index arithmetic shows only past 2^31 elements: 272 heads x 65536 positions x 128 = 2.28e9 elements, once in q
    and y ([batch, heads, seq, head_dim], 16 keys) and once in k and v ([batch, seq, heads, head_dim], 16 queries), on device tensors.
    The first and the last head must carry the bits of a one-head call on that head alone (the bits do not depend on the grid), and the
    last rows of the last head must meet the float64 reference."""
    from candle_birefnet_amd import ops
    heads, seq, hd = 272, 65536, 128
    assert heads * seq * hd > 2 ** 31
    g = torch.Generator(device="cuda").manual_seed(5)
    q = torch.randn(1, heads, seq, hd, device="cuda", generator=g)
    k, v = (torch.randn(1, heads, 16, hd, device="cuda", generator=g) for _ in range(2))
    y = ops.flash_attention(q, k, v, layout="bhsd")
    for h in (0, heads - 1):
        one = ops.flash_attention(*(a[:, h:h + 1].contiguous() for a in (q, k, v)), layout="bhsd")
        assert torch.equal(y[:, h:h + 1], one), h
    ref = A.reference(*(a[:, -1:, -64:].cpu().numpy() for a in (q, k, v)))
    assert float(np.abs(y[:, -1:, -64:].cpu().numpy().astype(np.float64) - ref).max()) <= _f32_bound(ref)
    del q, y, one
    k, v = (torch.randn(1, seq, heads, hd, device="cuda", generator=g) for _ in range(2))
    q = torch.randn(1, 16, heads, hd, device="cuda", generator=g)
    y = ops.flash_attention(q, k, v, layout="bshd")
    for h in (0, heads - 1):
        qs, ks, vs = (a[:, :, h:h + 1].contiguous() for a in (q, k, v))
        assert torch.equal(y[:, :, h:h + 1], ops.flash_attention(qs, ks, vs, layout="bshd")), h
    ref = A.reference(*(a.cpu().numpy() for a in (qs, ks, vs)), layout="bshd")
    assert float(np.abs(y[:, :, -1:].cpu().numpy().astype(np.float64) - ref).max()) <= _f32_bound(ref)


@pytest.mark.parametrize("shape", [(2, 17, 17, 3, 64, "bshd", 0), (1, 257, 257, 2, 128, "bhsd", 1)], ids=A.case_id)
def test_flash_attention_device_tensors(gpu, shape):
    """q, k, v as torch tensors on the GPU: y comes back on the device with the bits of the host-buffer call"""
    from candle_birefnet_amd import ops
    q, k, v = A.make_inputs(shape)
    dq, dk, dv = (torch.from_numpy(np.array(a)).cuda() for a in (q, k, v))
    y = ops.flash_attention(dq, dk, dv, causal=bool(shape[6]), layout=shape[5])
    assert y.is_cuda and tuple(y.shape) == q.shape
    np.testing.assert_array_equal(y.cpu().numpy(), _f32_result(shape))


def test_flash_attention_refusals_leave_no_stale_error(gpu):
    """every limit of the header is status 1 with a message naming it, and the valid call that follows succeeds"""
    from candle_birefnet_amd import _ffi
    shape = (2, 17, 17, 3, 64, "bshd", 0)
    for name, args, word in A.refusals():
        st, msg = A.raw_call(_ffi.lib, *args)
        assert st == 1 and word in msg, (name, st, msg)
        np.testing.assert_array_equal(_run(shape), _f32_result(shape))
