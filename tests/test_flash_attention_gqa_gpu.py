"""brn_flash_attention_gqa_forward on the GPU: K / V heads shared by groups of query heads, and the causal mask over a K / V cache.

Both are index semantics, so the result is pinned BIT FOR BIT against the two older entries: a row's arithmetic does not depend on which
rows share its workgroup (a K / V tile that is wholly excluded for a row leaves alpha = 1 and numerators exactly 0 behind), a -inf bias
entry contributes exactly 0 and never raises the maximum, and a zero bias gives the bias-free bits (include/birefnet_hip.h).
Parity against float64 uses the bounds of tests/test_flash_attention_gpu.py unchanged (3e-5 max(1, max |ref|), plus u max |v| in the
16-bit modes on inputs rounded to the 16-bit type); tests/test_flash_attention_gqa_cpu.py records that the emulation of the packed-row walk
stays inside them on these inputs."""
import numpy as np
import pytest
import torch

import flash_attention_gqa_cases as GQ

pytestmark = pytest.mark.gpu

MODES = ["f32", "bf16", "f16"]


def _mode(mode, fn):
    from candle_birefnet_amd import ops
    ops.set_compute(mode)
    try:
        return fn(ops)
    finally:
        ops.set_compute("f32")


_GQA = {}


def _gqa(shape, mode="f32", layout="bhsd", causal=0, with_bias=False, kind="std1"):
    """the grouped entry on a case, as a BHSD array; computed once per argument set (read-only)"""
    key = (shape, mode, layout, causal, with_bias, kind)
    if key not in _GQA:
        q, k, v, bias = GQ.make_inputs(shape, kind)
        args = [GQ.in_layout(a, layout) for a in (q, k, v)]
        y = _mode(mode, lambda ops: ops.flash_attention_gqa(*args, causal=bool(causal), scale=GQ.kind_scale(kind), layout=layout,
                                                            bias=bias if with_bias else None))
        assert y.shape == args[0].shape
        _GQA[key] = GQ.to_bhsd(y, layout)
        _GQA[key].setflags(write=False)
    return _GQA[key]


def _old(shape, mode, layout, causal, bias, kind="std1"):
    """the older entries (brn_flash_attention_forward, or with a bias brn_flash_attention_bias_forward) on K / V repeated G times along
    heads, as a BHSD array"""
    q, k, v, _ = GQ.make_inputs(shape, kind)
    G = shape[3] // shape[4]
    args = [GQ.in_layout(a, layout) for a in (q, GQ.repeat_kv(k, G), GQ.repeat_kv(v, G))]
    y = _mode(mode, lambda ops: ops.flash_attention(*args, causal=bool(causal), scale=GQ.kind_scale(kind), layout=layout, bias=bias))
    return GQ.to_bhsd(y, layout)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("shape", GQ.GROUP_SHAPES, ids=GQ.shape_id)
def test_grouping_is_exact(gpu, shape, mode):
    """the bits of the older entries on materialised repeated K / V: both layouts, with and without a bias, not causal and (seq_q == seq_kv) causal"""
    bias = GQ.make_inputs(shape)[3]
    for layout in ("bshd", "bhsd"):
        for with_bias in (False, True):
            for causal in ((0, 1) if shape[1] == shape[2] else (0,)):
                y = _gqa(shape, mode, layout, causal, with_bias)
                assert np.isfinite(y).all()
                np.testing.assert_array_equal(y, _old(shape, mode, layout, causal, bias if with_bias else None), err_msg=f"{layout} bias {with_bias} causal {causal}")


@pytest.mark.parametrize("mode", ["f32", "bf16"])
@pytest.mark.parametrize("shape", GQ.CACHE_SHAPES, ids=GQ.shape_id)
def test_cached_causal_is_exact(gpu, shape, mode):
    """seq_q < seq_kv, causal: the bits of the bias entry, NOT causal, on repeated K / V with the mask written into the bias as -inf (over
    zeros, or over the caller's bias)"""
    bias = GQ.make_inputs(shape)[3]
    for layout in ("bshd", "bhsd"):
        for with_bias in (False, True):
            y = _gqa(shape, mode, layout, 1, with_bias)
            assert np.isfinite(y).all()
            np.testing.assert_array_equal(y, _old(shape, mode, layout, 0, GQ.mask_bias(shape, bias if with_bias else None)), err_msg=f"{layout} bias {with_bias}")


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("case", GQ.PARITY, ids=GQ.parity_id)
def test_parity_against_float64(gpu, case, mode):
    shape, kind, causal = case
    s16 = None if mode == "f32" else mode
    v = GQ.make_inputs(shape, kind)[2]
    for with_bias in (False, True):
        y = _gqa(shape, mode, "bhsd", causal, with_bias, kind)
        ref = GQ.case_reference(shape, kind, causal, s16, with_bias)
        bound = GQ.f32_bound(ref) if s16 is None else GQ.s16_bound(ref, v, s16)
        err = float(np.abs(np.asarray(y, np.float64) - ref).max())
        print(f"flash attention gqa {mode} {GQ.parity_id(case)} bias {int(with_bias)}: max abs err {err:.3e}, bound {bound:.3e}")
        assert y.shape == ref.shape and np.isfinite(y).all()
        assert err <= bound


def test_plane_modes_are_the_f32_kernel(gpu):
    """one exact fp32 kernel behind every mode that is not bf16 / f16: the same bits"""
    shape = (2, 17, 300, 6, 2, 32)
    for mode in ("f32_split3", "f32_split2", "f32_half2"):
        np.testing.assert_array_equal(_gqa(shape, mode, "bshd", 1, True), _gqa(shape, "f32", "bshd", 1, True))


@pytest.mark.parametrize("mode", ["f32", "bf16"])
@pytest.mark.parametrize("shape", [(2, 64, 64, 4, 4, 32), (2, 150, 150, 3, 3, 128)], ids=GQ.shape_id)
def test_degenerate_call_equals_the_older_entries(gpu, shape, mode):
    """kv_heads == heads and seq_q == seq_kv: the bits of brn_flash_attention_forward and, with a bias, of brn_flash_attention_bias_forward"""
    bias = GQ.make_inputs(shape)[3]
    for causal in (0, 1):
        for layout in ("bshd", "bhsd"):
            np.testing.assert_array_equal(_gqa(shape, mode, layout, causal, False), _old(shape, mode, layout, causal, None))
            np.testing.assert_array_equal(_gqa(shape, mode, layout, causal, True), _old(shape, mode, layout, causal, bias))


@pytest.mark.parametrize("shape", [(2, 17, 300, 6, 2, 32), (1, 100, 164, 4, 1, 128)], ids=GQ.shape_id)
def test_causal_row_zero_with_a_cache(gpu, shape):
    """query 0 of a cached causal call is the softmax over keys 0 .. seq_kv - seq_q alone: the non-causal call on those keys, to the fp32
    bound; the last query sees every key: the non-causal row, bit for bit"""
    q, k, v, _ = GQ.make_inputs(shape)
    n = shape[2] - shape[1] + 1
    y = _gqa(shape, "f32", "bhsd", 1)
    head = _mode("f32", lambda ops: ops.flash_attention_gqa(*(np.ascontiguousarray(a) for a in (q[:, :, :1], k[:, :, :n], v[:, :, :n])), layout="bhsd"))
    ref = GQ.reference(q[:, :, :1], k[:, :, :n], v[:, :, :n])
    assert float(np.abs(head.astype(np.float64) - ref).max()) <= GQ.f32_bound(ref)
    assert float(np.abs(y[:, :, :1].astype(np.float64) - ref).max()) <= GQ.f32_bound(ref)
    np.testing.assert_array_equal(y[:, :, -1], _gqa(shape, "f32", "bhsd", 0)[:, :, -1])


@pytest.mark.parametrize("mode", ["f32", "bf16"])
def test_batch_independence_repeatability_and_device_tensors(gpu, mode):
    """entry 1 of a batch-3 call equals the batch-1 call on that entry bit for bit; a repeated call repeats its bits; device tensors and
    host arrays give the same bits"""
    rng = np.random.default_rng(91)
    q = rng.standard_normal((3, 9, 12, 64)).astype(np.float32)                  # BSHD, G 4 over a cache of 200
    k, v = (rng.standard_normal((3, 200, 3, 64)).astype(np.float32) for _ in range(2))
    bias = (rng.standard_normal((1, 12, 9, 200)) * 8).astype(np.float32)
    call = lambda ops, *a: ops.flash_attention_gqa(*a[:3], causal=True, bias=a[3])
    y = _mode(mode, lambda ops: call(ops, q, k, v, bias))
    np.testing.assert_array_equal(_mode(mode, lambda ops: call(ops, q, k, v, bias)), y)
    np.testing.assert_array_equal(_mode(mode, lambda ops: call(ops, q[1:2], k[1:2], v[1:2], bias)), y[1:2])
    dev = [torch.from_numpy(a).cuda() for a in (q, k, v, bias)]
    yd = _mode(mode, lambda ops: call(ops, *dev))
    assert yd.is_cuda and tuple(yd.shape) == q.shape
    np.testing.assert_array_equal(yd.cpu().numpy(), y)


def test_offsets_past_2_31(gpu):
    """a fault of 32-bit index arithmetic in the per-lane row addresses shows only past 2^31 elements: 272 query heads x 65536 positions x
    128 = 2.28e9 elements in q and y ([batch, heads, seq, head_dim], G 136 over 2 K / V heads of 16 keys), then in k and v ([batch, seq,
    kv_heads, head_dim], 272 K / V heads under 544 query heads of 16 queries, causal over the cache), on device tensors.  The first and the
    last head must carry the bits of a one-head call on that head and its K / V head (grouping is exact), and the last rows of the last
    head must meet the float64 reference."""
    from candle_birefnet_amd import ops
    heads, seq, hd = 272, 65536, 128
    assert heads * seq * hd > 2 ** 31
    g = torch.Generator(device="cuda").manual_seed(6)
    q = torch.randn(1, heads, seq, hd, device="cuda", generator=g)
    k, v = (torch.randn(1, 2, 16, hd, device="cuda", generator=g) for _ in range(2))
    y = ops.flash_attention_gqa(q, k, v, layout="bhsd")
    for h in (0, heads - 1):
        kvh = h // (heads // 2)
        one = ops.flash_attention(q[:, h:h + 1].contiguous(), k[:, kvh:kvh + 1].contiguous(), v[:, kvh:kvh + 1].contiguous(), layout="bhsd")
        assert torch.equal(y[:, h:h + 1], one), h
    ref = GQ.reference(*(a.cpu().numpy() for a in (q[:, -1:, -64:], k[:, -1:], v[:, -1:])))
    assert float(np.abs(y[:, -1:, -64:].cpu().numpy().astype(np.float64) - ref).max()) <= GQ.f32_bound(ref)
    del q, y, one
    k, v = (torch.randn(1, seq, heads, hd, device="cuda", generator=g) for _ in range(2))
    q = torch.randn(1, 16, 2 * heads, hd, device="cuda", generator=g)
    y = ops.flash_attention_gqa(q, k, v, causal=True, layout="bshd")
    for h in (0, 2 * heads - 1):
        qs, ks, vs = q[:, :, h:h + 1].contiguous(), k[:, :, h // 2:h // 2 + 1].contiguous(), v[:, :, h // 2:h // 2 + 1].contiguous()
        assert torch.equal(y[:, :, h:h + 1], ops.flash_attention_gqa(qs, ks, vs, causal=True, layout="bshd")), h
    ref = GQ.reference(*(a.cpu().numpy().transpose(0, 2, 1, 3) for a in (qs, ks, vs)), causal=True).transpose(0, 2, 1, 3)
    assert float(np.abs(y[:, :, -1:].cpu().numpy().astype(np.float64) - ref).max()) <= GQ.f32_bound(ref)


def test_refusals_leave_no_stale_error(gpu):
    """every limit is status 1 with a message naming it, and the valid call that follows succeeds with the same bits as before"""
    from candle_birefnet_amd import _ffi
    shape = (2, 37, 37, 6, 2, 32)
    want = np.array(_gqa(shape, "f32", "bshd", 1, True))
    q, k, v, bias = GQ.make_inputs(shape)
    args = [GQ.in_layout(a, "bshd") for a in (q, k, v)]
    for name, a, word in GQ.refusals():
        st, msg = GQ.raw_call(_ffi.lib, *a)
        assert st == 1 and word in msg, (name, st, msg)
        y = _mode("f32", lambda ops: ops.flash_attention_gqa(*args, causal=True, bias=bias))
        np.testing.assert_array_equal(GQ.to_bhsd(y, "bshd"), want)
