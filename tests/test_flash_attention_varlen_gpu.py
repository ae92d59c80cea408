"""brn_flash_attention_varlen_forward on the GPU: packed batches of sequences of unequal lengths, and window masks.

Both are index semantics over the packed-row kernels, so the result is pinned BIT FOR BIT against the entries that exist: a uniform pack
is the gqa entry's batch; every sequence of a pack is the gqa entry on that sequence alone; a window is the bias entry on that sequence
with K / V repeated G times and the window written into a zero bias as -inf (a row's leading wholly excluded K / V tiles are wiped by
alpha = 0 at its first real score: kernels/flash_attention.hip).  Parity against float64 uses the bounds of
tests/test_flash_attention_gpu.py unchanged; tests/test_flash_attention_varlen_cpu.py records that the emulation of the walk stays inside
them on these inputs."""
import numpy as np
import pytest
import torch

import flash_attention_gqa_cases as GQ
import flash_attention_varlen_cases as VL

pytestmark = pytest.mark.gpu

MODES = ["f32", "bf16", "f16"]


def _mode(mode, fn):
    from candle_birefnet_amd import ops
    ops.set_compute(mode)
    try:
        return fn(ops)
    finally:
        ops.set_compute("f32")


_VARLEN = {}


def _varlen(name, window, mode="f32"):
    """the packed entry on a pack: y [total_q, heads, hd]; computed once per argument set (read-only)"""
    key = (name, window, mode)
    if key not in _VARLEN:
        q, k, v, cq, ckv = VL.make_pack(name)
        y = _mode(mode, lambda ops: ops.flash_attention_varlen(q, k, v, cq, ckv, window=window))
        assert y.shape == q.shape and y.dtype == np.float32
        y.setflags(write=False)
        _VARLEN[key] = y
    return _VARLEN[key]


def _gqa_alone(name, s, mode, causal):
    """the gqa entry on sequence s of a pack alone, BHSD"""
    q, k, v = VL.seq_inputs(name, s)
    return _mode(mode, lambda ops: ops.flash_attention_gqa(q, k, v, causal=causal, layout="bhsd"))


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("shape", [(2, 37, 37, 6, 2, 32), (2, 17, 300, 6, 2, 32)], ids=GQ.shape_id)
def test_uniform_pack_is_the_gqa_entry(gpu, shape, mode):
    """a [batch, seq, heads, head_dim] tensor is a pack with cu = b * seq: window (-1, -1) / (-1, 0) carry the bits of the gqa entry in
    BSHD, not causal / causal"""
    batch, sq, skv, heads, kv_heads, hd = shape
    q, k, v = (GQ.in_layout(a, "bshd") for a in GQ.make_inputs(shape)[:3])
    cq, ckv = np.arange(batch + 1) * sq, np.arange(batch + 1) * skv
    for window, causal in (((-1, -1), False), ((-1, 0), True)):
        y = _mode(mode, lambda ops: ops.flash_attention_varlen(q.reshape(batch * sq, heads, hd), k.reshape(batch * skv, kv_heads, hd),
                                                               v.reshape(batch * skv, kv_heads, hd), cq, ckv, window=window))
        want = _mode(mode, lambda ops: ops.flash_attention_gqa(q, k, v, causal=causal, layout="bshd"))
        assert y.shape == (batch * sq, heads, hd) and np.isfinite(y).all()
        np.testing.assert_array_equal(y.reshape(want.shape), want, err_msg=str(window))


@pytest.mark.parametrize("mode", ["f32", "bf16"])
@pytest.mark.parametrize("name", list(VL.PACKS))
def test_packing_is_exact(gpu, name, mode):
    """every sequence's slice of y is the gqa entry on that sequence alone, not causal for (-1, -1) and causal for (-1, 0)"""
    cq = VL.make_pack(name)[3]
    for window, causal in (((-1, -1), False), ((-1, 0), True)):
        y = _varlen(name, window, mode)
        assert np.isfinite(y).all()
        for s in VL.sequences(name):
            np.testing.assert_array_equal(VL.from_packed(y, cq, s), _gqa_alone(name, s, mode, causal), err_msg=f"{window} sequence {s}")


@pytest.mark.parametrize("mode", ["f32", "bf16"])
@pytest.mark.parametrize("name", list(VL.PACKS))
def test_windows_are_exact(gpu, name, mode):
    """every pack x window: each sequence's slice is the bias entry, NOT causal, on that sequence with K / V repeated G times and the
    window written into a zero bias as -inf; finite everywhere"""
    lens, heads, kv_heads, _ = VL.PACKS[name]
    cq = VL.make_pack(name)[3]
    for s in VL.sequences(name):
        q, k, v = VL.seq_inputs(name, s)
        kr, vr = GQ.repeat_kv(k, heads // kv_heads), GQ.repeat_kv(v, heads // kv_heads)
        for window in VL.WINDOWS:
            y = _varlen(name, window, mode)
            assert np.isfinite(y).all()
            bias = VL.mask_bias(heads, lens[s][0], lens[s][1], window)
            want = _mode(mode, lambda ops: ops.flash_attention(q, kr, vr, causal=False, layout="bhsd", bias=bias))
            np.testing.assert_array_equal(VL.from_packed(y, cq, s), want, err_msg=f"{window} sequence {s}")


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", list(VL.PACKS))
def test_parity_against_float64(gpu, name, mode):
    s16 = None if mode == "f32" else mode
    cq = VL.make_pack(name)[3]
    for window in VL.WINDOWS:
        y = _varlen(name, window, mode)
        assert np.isfinite(y).all()
        for s in VL.sequences(name):
            ref = VL.case_reference(name, s, window, s16)
            bound = VL.f32_bound(ref) if s16 is None else VL.s16_bound(ref, VL.seq_inputs(name, s)[2], s16)
            err = float(np.abs(VL.from_packed(y, cq, s).astype(np.float64) - ref).max())
            print(f"flash attention varlen {mode} pack {name} {VL.window_id(window)} sequence {s}: max abs err {err:.3e}, bound {bound:.3e}")
            assert err <= bound, (window, s)


@pytest.mark.parametrize("mode", ["f32", "bf16"])
def test_window_sides_past_every_sequence(gpu, mode):
    """a side of 65536 or more, INT_MAX as "unbounded" included, carries the bits of -1 on that side (the kernels' int arithmetic on
    query + off + window_right + 1 never sees it: the entry clamps)"""
    for name in ("A", "B"):
        for far, near in VL.FAR_WINDOWS:
            np.testing.assert_array_equal(_varlen(name, far, mode), _varlen(name, near, mode), err_msg=f"{name} {far}")


@pytest.mark.parametrize("mode", ["f32", "bf16"])
def test_large_v_in_leading_excluded_tiles(gpu, mode):
    """V rows of 1e37 in K / V tile 0, window (15, 0), one sequence of 150 at G = 1: queries 79 .. 127 share a workgroup that walks tile 0
    and see none of its keys.  64 numerators of 1 times 1e37 would overflow O before any alpha = 0 could wipe it; the excluded scores are
    -inf, the numerators 0, and the rows carry the bits of the bias entry with the window as a -inf bias"""
    q, k, v = VL.seq_inputs("D", 0)
    v = np.array(v)
    v[:, :, :64] = np.where(v[:, :, :64] < 0, np.float32(-1e37), np.float32(1e37))
    cu = np.array([0, 150])
    y = _mode(mode, lambda ops: ops.flash_attention_varlen(VL.to_packed(q), VL.to_packed(k), VL.to_packed(v), cu, cu, window=(15, 0)))
    want = _mode(mode, lambda ops: ops.flash_attention(q, k, v, causal=False, layout="bhsd", bias=VL.mask_bias(4, 150, 150, (15, 0))))
    assert np.isfinite(y).all() and float(np.abs(y[79:]).max()) < 10.0
    np.testing.assert_array_equal(VL.from_packed(y, cu, 0), want)


def test_plane_modes_are_the_f32_kernel(gpu):
    """one exact fp32 kernel behind every mode that is not bf16 / f16: the same bits"""
    for mode in ("f32_split3", "f32_split2", "f32_half2"):
        np.testing.assert_array_equal(_varlen("A", (15, 0), mode), _varlen("A", (15, 0), "f32"))


@pytest.mark.parametrize("mode", ["f32", "bf16"])
def test_order_independence_repeatability_and_device_tensors(gpu, mode):
    """reversing the order of the sequences in the pack gives each sequence the same bits (the record table is ordered differently, and
    every sequence starts elsewhere); a repeated call repeats its bits; device tensors and host arrays give the same bits"""
    for name, window in (("A", (20, 20)), ("B", (63, 0)), ("B", (-1, -1))):
        q, k, v, cq, ckv = VL.make_pack(name)
        y = _varlen(name, window, mode)
        np.testing.assert_array_equal(_mode(mode, lambda ops: ops.flash_attention_varlen(q, k, v, cq, ckv, window=window)), y)
        n = len(VL.PACKS[name][0])
        order = tuple(reversed(range(n)))
        qr, kr, vr, cqr, ckvr = VL.make_pack(name, order)
        yr = _mode(mode, lambda ops: ops.flash_attention_varlen(qr, kr, vr, cqr, ckvr, window=window))
        for pos, s in enumerate(order):
            np.testing.assert_array_equal(VL.from_packed(yr, cqr, pos), VL.from_packed(y, cq, s), err_msg=f"{name} {window} sequence {s}")
        dev = [torch.tensor(a, device="cuda") for a in (q, k, v)]
        yd = _mode(mode, lambda ops: ops.flash_attention_varlen(*dev, cq, ckv, window=window))
        assert yd.is_cuda and tuple(yd.shape) == q.shape
        np.testing.assert_array_equal(yd.cpu().numpy(), y)


def test_nothing_outside_y_is_written(gpu):
    """a raw call whose y points 64 rows into a larger sentinel-filled device buffer leaves both guard regions untouched; the K / V rows of
    pack B's entry with no queries may hold NaN without changing any output"""
    from candle_birefnet_amd import _ffi
    for name, window in (("A", (15, 0)), ("B", (-1, 5)), ("C", (-1, -1))):
        q, k, v, cq, ckv = VL.make_pack(name)
        _, heads, kv_heads, hd = VL.PACKS[name]
        total, row, guard = q.shape[0], heads * hd, 64 * heads * hd
        dq, dk, dv = (torch.tensor(a, device="cuda") for a in (q, k, v))
        buf = torch.full((2 * guard + total * row,), -777.0, device="cuda")
        st, msg = VL.raw_call(_ffi.lib, dq.data_ptr(), dk.data_ptr(), dv.data_ptr(), cq, ckv, len(cq) - 1, heads, kv_heads, hd, window[0], window[1], 0.0,
                              buf.data_ptr() + 4 * guard, 1)
        assert st == 0, msg
        torch.cuda.synchronize()
        out = buf.cpu().numpy()
        assert (out[:guard] == -777.0).all() and (out[guard + total * row:] == -777.0).all()
        np.testing.assert_array_equal(out[guard:guard + total * row].reshape(q.shape), _varlen(name, window))
    q, k, v, cq, ckv = VL.make_pack("B")
    k2, v2 = np.array(k), np.array(v)
    assert cq[2] == cq[1] and ckv[2] - ckv[1] == 9
    k2[ckv[1]:ckv[2]] = np.nan
    v2[ckv[1]:ckv[2]] = np.nan
    for window in ((-1, -1), (63, 0)):
        y = _mode("f32", lambda ops: ops.flash_attention_varlen(q, k2, v2, cq, ckv, window=window))
        np.testing.assert_array_equal(y, _varlen("B", window))


def test_refusals_leave_no_stale_error(gpu):
    """every limit is status 1 with a message naming it, and the valid call that follows succeeds with the same bits as before"""
    from candle_birefnet_amd import _ffi
    q, k, v, cq, ckv = VL.make_pack("A")
    want = np.array(_varlen("A", (15, 0)))
    for name, a, word in VL.refusals():
        st, msg = VL.raw_call(_ffi.lib, *a)
        assert st == 1 and msg.startswith("flash attention varlen: ") and word in msg, (name, st, msg)
        np.testing.assert_array_equal(_mode("f32", lambda ops: ops.flash_attention_varlen(q, k, v, cq, ckv, window=(15, 0))), want)


def test_offsets_past_2_31(gpu):
    """a fault of 32-bit index arithmetic in the sequence bases shows only past 2^31 elements: 266144 rows x 64 heads x 128 = 2.18e9 elements
    in q and y (four sequences of 65536 queries and one of 4000, which starts at element 2^31 exactly; G 32 over 2 K / V heads of 16 keys
    each), then in k and v (the same lengths as keys, 64 K / V heads under 128 query heads of 16 queries, causal over the cache), on device
    tensors.  The first and the last sequence must carry the bits of the gqa entry on that sequence alone."""
    from candle_birefnet_amd import ops
    long_lens, hd = [65536] * 4 + [4000], 128
    cu_long = np.concatenate([[0], np.cumsum(long_lens)])
    cu_short = np.arange(6) * 16
    assert cu_long[-1] * 64 * hd > 2 ** 31 and cu_long[-2] * 64 * hd == 2 ** 31
    g = torch.Generator(device="cuda").manual_seed(7)
    q = torch.randn(int(cu_long[-1]), 64, hd, device="cuda", generator=g)
    k, v = (torch.randn(int(cu_short[-1]), 2, hd, device="cuda", generator=g) for _ in range(2))
    y = ops.flash_attention_varlen(q, k, v, cu_long, cu_short)
    for s in (0, 4):
        one = ops.flash_attention_gqa(q[cu_long[s]:cu_long[s + 1]][None], k[cu_short[s]:cu_short[s + 1]][None], v[cu_short[s]:cu_short[s + 1]][None], layout="bshd")
        assert torch.equal(y[cu_long[s]:cu_long[s + 1]], one[0]), s
    del q, y, one
    k, v = (torch.randn(int(cu_long[-1]), 64, hd, device="cuda", generator=g) for _ in range(2))
    q = torch.randn(int(cu_short[-1]), 128, hd, device="cuda", generator=g)
    y = ops.flash_attention_varlen(q, k, v, cu_short, cu_long, window=(-1, 0))
    for s in (0, 4):
        one = ops.flash_attention_gqa(q[cu_short[s]:cu_short[s + 1]][None], k[cu_long[s]:cu_long[s + 1]][None], v[cu_long[s]:cu_long[s + 1]][None], causal=True,
                                      layout="bshd")
        assert torch.equal(y[cu_short[s]:cu_short[s + 1]], one[0]), s
    assert torch.isfinite(y).all()
