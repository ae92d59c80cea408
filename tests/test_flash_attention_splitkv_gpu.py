"""brn_flash_attention_splitkv_forward on the GPU: the K / V tiles of a call split between workgroups, the partials in the workspace, the
combine in a fixed order, and the log-sum-exp of every row.

What is index semantics is pinned BIT FOR BIT: one split is the gqa entry; a partial of a call that is not causal is the gqa entry on
the keys of its split; causal and not causal agree where every key is visible; kv_splits 0 is the explicit call with the plan's S.
Parity of y against float64 uses the bounds of tests/test_flash_attention_gqa_gpu.py unchanged, lse the same form
(3e-5 max(1, max |lse|)); tests/test_flash_attention_splitkv_cpu.py records that the emulation stays inside them on these inputs."""
import numpy as np
import pytest
import torch

import flash_attention_gqa_cases as GQ
import flash_attention_splitkv_cases as SK

pytestmark = pytest.mark.gpu

MODES = list(SK.MODES)
# test_result_is_the_combination_of_its_own_partials: the largest |y - combine64(own partials)| / max(1, max |y|), and the same for lse,
# allowed there: 4 x the larger of the figure measured in the emulation and the one measured on the GPU (its docstring has them)
COMBINE_TOL_Y = 4 * 9.63e-8
COMBINE_TOL_LSE = 4 * 1.05e-7


def _mode(mode, fn):
    from candle_birefnet_amd import ops
    ops.set_compute(mode)
    try:
        return fn(ops)
    finally:
        ops.set_compute("f32")


_RUN = {}


def _run(shape, kind, causal, ks, mode="f32", layout="bhsd"):
    """the entry on host arrays -> (y as BHSD, lse, O_part [S, R, D] or None, lse2_part [S, R] or None); computed once (read-only)"""
    key = (shape, kind, causal, ks, mode, layout)
    if key not in _RUN:
        q, k, v, _ = SK.make_inputs(shape, kind)
        args = [SK.in_layout(a, layout) for a in (q, k, v)]
        y, lse, (op, l2) = _mode(mode, lambda ops: ops.flash_attention_splitkv(*args, causal=bool(causal), scale=SK.kind_scale(kind), layout=layout,
                                                                                kv_splits=ks, return_lse=True, return_partials=True))
        assert y.shape == args[0].shape and lse.shape == (shape[0], shape[3], shape[1])
        out = (GQ.to_bhsd(y, layout), lse, op, l2)
        for a in out:
            if a is not None:
                a.setflags(write=False)
        _RUN[key] = out
    return _RUN[key]


def _gqa(q, k, v, mode, causal, kind="std1", layout="bhsd"):
    args = [SK.in_layout(a, layout) for a in (q, k, v)]
    return GQ.to_bhsd(_mode(mode, lambda ops: ops.flash_attention_gqa(*args, causal=bool(causal), scale=SK.kind_scale(kind), layout=layout)), layout)


def _check_lse(lse, shape, kind, causal, mode, what):
    ref = SK.case_reference(shape, kind, causal, None if mode == "f32" else mode)[1]
    err, bound = float(np.abs(np.asarray(lse, np.float64) - ref).max()), SK.lse_bound(ref)
    print(f"flash attention splitkv {mode} {what}: lse max abs err {err:.3e}, bound {bound:.3e}")
    assert np.isfinite(lse).all() and err <= bound


@pytest.mark.parametrize("mode", MODES)
def test_one_split_carries_the_gqa_bits(gpu, mode):
    """kv_splits 1, and the case whose S collapses to 1: the bits of ops.flash_attention_gqa in both layouts, causal and not, no
    partials; lse meets the float64 bound"""
    for shape, ks in (((2, 17, 300, 6, 2, 32), 1), ((2, 1, 300, 8, 2, 64), 1), ((1, 2, 65, 2, 1, 128), 1), (SK.COLLAPSED[0], SK.COLLAPSED[3])):
        q, k, v, _ = SK.make_inputs(shape)
        for layout in ("bshd", "bhsd"):
            for causal in (0, 1):
                y, lse, op, l2 = _run(shape, "std1", causal, ks, mode, layout)
                assert op is None and l2 is None
                np.testing.assert_array_equal(y, _gqa(q, k, v, mode, causal, layout=layout), err_msg=f"{shape} {layout} causal {causal}")
                _check_lse(lse, shape, "std1", causal, mode, f"{SK.shape_id(shape)} {layout} causal {causal} s{ks}")


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("case", [c for c in SK.CASES if not c[2] and SK.plan(c[0][2], c[3])[0] > 1], ids=SK.case_id)
def test_a_partial_is_the_gqa_entry_on_its_keys(gpu, case, mode):
    """not causal, S > 1: O_part[s] is bit for bit ops.flash_attention_gqa on k, v sliced to the keys of split s"""
    shape, kind, causal, ks = case
    q, k, v, _ = SK.make_inputs(shape, kind)
    S, tps = SK.plan(shape[2], ks)
    _, _, op, l2 = _run(*case, mode)
    assert op.shape == (S, shape[0] * shape[3] * shape[1], shape[5]) and l2.shape == op.shape[:2] and np.isfinite(l2).all()
    for s in range(S):
        keys = slice(s * tps * SK.T, min((s + 1) * tps * SK.T, shape[2]))
        want = _gqa(q, np.ascontiguousarray(k[:, :, keys]), np.ascontiguousarray(v[:, :, keys]), mode, 0, kind)
        np.testing.assert_array_equal(op[s].reshape(want.shape), want, err_msg=f"split {s}")


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("case", [c for c in SK.CASES if SK.plan(c[0][2], c[3])[0] > 1], ids=SK.case_id)
def test_result_is_the_combination_of_its_own_partials(gpu, case, mode):
    """y and lse against the float64 combination of the call's OWN returned partials: what the combine kernel adds on top of them.
    Measured as |difference| / max(1, max |reference|), the worst over every case with S > 1 and the modes f32 / bf16 / f16:
      y    emulation 8.92e-8, MI355X 9.63e-8        lse    emulation 1.05e-7, MI355X 9.80e-8
    (about one fp32 rounding of a value near the largest).  4 x the larger of the two is allowed, since the hardware's exp2 / log2 are not
    correctly rounded, capped by the 3e-5 of the parity bound.  DESIGN.md 3.2h."""
    y, lse, op, l2 = _run(*case, mode)
    y64, lse64 = SK.combine64(op, l2)
    y64, lse64 = y64.reshape(y.shape), lse64.reshape(lse.shape)
    ey = float(np.abs(y - y64).max()) / max(1.0, float(np.abs(y64).max()))
    el = float(np.abs(lse - lse64).max()) / max(1.0, float(np.abs(lse64).max()))
    print(f"flash attention splitkv {mode} {SK.case_id(case)}: combine y {ey:.3e}, lse {el:.3e} (relative to max(1, max |ref|))")
    assert np.isfinite(y).all() and np.isfinite(lse).all()
    assert ey <= min(COMBINE_TOL_Y, 3e-5) and el <= min(COMBINE_TOL_LSE, 3e-5)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("case", SK.CASES, ids=SK.case_id)
def test_parity_against_float64(gpu, case, mode):
    shape, kind, causal, ks = case
    v = SK.make_inputs(shape, kind)[2]
    y, lse, op, l2 = _run(*case, mode)
    ref, ref_lse = SK.case_reference(shape, kind, causal, None if mode == "f32" else mode)
    err, bound = float(np.abs(np.asarray(y, np.float64) - ref).max()), SK.y_bound(ref, v, mode)
    print(f"flash attention splitkv {mode} {SK.case_id(case)}: y max abs err {err:.3e}, bound {bound:.3e}")
    assert y.shape == ref.shape and np.isfinite(y).all()
    assert err <= bound
    _check_lse(lse, shape, kind, causal, mode, SK.case_id(case))
    if op is not None:
        empty = np.isneginf(l2)
        assert int(empty.sum()) == SK.empty_rows(case) and (op[empty] == 0).all() and np.isfinite(op).all() and not np.isnan(l2).any()


@pytest.mark.parametrize("mode", MODES)
def test_causal_changes_nothing_where_every_key_is_visible(gpu, mode):
    """seq_q == 1: the causal bits are the not-causal bits (y, lse and partials); seq_q > 1: the last query's row is the same under both"""
    a, b = (_run((2, 1, 300, 8, 2, 64), "std1", c, 3, mode) for c in (0, 1))
    for x, y in zip(a, b):
        np.testing.assert_array_equal(x, y)
    a, b = (_run((2, 7, 200, 16, 2, 64), "std1", c, 4, mode) for c in (0, 1))
    np.testing.assert_array_equal(a[0][:, :, -1], b[0][:, :, -1])
    np.testing.assert_array_equal(a[1][:, :, -1], b[1][:, :, -1])
    assert not np.array_equal(a[0][:, :, 0], b[0][:, :, 0])


@pytest.mark.parametrize("mode", MODES)
def test_automatic_split_is_the_explicit_one(gpu, mode):
    """kv_splits 0 carries the bits of the explicit call with the plan's S (and splits these shapes)"""
    from candle_birefnet_amd import ops
    for shape in ((3, 1, 1000, 5, 1, 128), (1, 130, 700, 4, 2, 32)):
        S, tps, _ = ops.flash_attention_splitkv_plan(*shape, 0)
        assert S > 1 and (S, tps) == SK.plan(shape[2], S)
        for x, y in zip(_run(shape, "std1", 1, 0, mode), _run(shape, "std1", 1, S, mode)):
            np.testing.assert_array_equal(x, y)


def _device_call(case, mode, fill, extra=64, sentinel=12345.0):
    """the raw entry on device tensors (BSHD) with a workspace of the plan's size + `extra` floats, every float of it `fill` first and the
    extra ones `sentinel`; -> (y, lse, workspace) as numpy"""
    import candle_birefnet_amd as cb
    shape, kind, causal, ks = case
    batch, seq_q, seq_kv, heads, kv_heads, hd = shape
    q, k, v = (torch.from_numpy(np.array(SK.in_layout(a, "bshd"))).cuda() for a in SK.make_inputs(shape, kind)[:3])
    S, _, need = cb.ops.flash_attention_splitkv_plan(*shape, ks)
    ws = torch.full((need + extra,), fill, dtype=torch.float32, device="cuda")
    ws[need:] = sentinel
    y = torch.full(q.shape, float("nan"), dtype=torch.float32, device="cuda")
    lse = torch.full((batch, heads, seq_q), float("nan"), dtype=torch.float32, device="cuda")

    def call(ops):
        st = cb._ffi.lib.brn_flash_attention_splitkv_forward(q.data_ptr(), k.data_ptr(), v.data_ptr(), batch, seq_q, seq_kv, heads, kv_heads, hd, 0, causal,
                                                             SK.kind_scale(kind) or 0.0, ks, y.data_ptr(), lse.data_ptr(), ws.data_ptr(), need, 1, 0,
                                                             torch.cuda.current_stream().cuda_stream)
        cb._ffi.check(st)
        torch.cuda.synchronize()
    _mode(mode, call)
    return y.cpu().numpy(), lse.cpu().numpy(), ws.cpu().numpy(), need


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("case", SK.EMPTY_CASES, ids=SK.case_id)
def test_workspace_is_written_before_it_is_read_and_not_past_its_size(gpu, case, mode):
    """the three cases with empty partials, on device tensors: a workspace pre-filled with NaN gives a finite result with the bits of a
    zero-filled one (every partial row, empty ones included, is written before the combine reads it), and the 64 floats past the stated
    size keep their sentinel"""
    y0, lse0, ws0, need = _device_call(case, mode, 0.0)
    y1, lse1, ws1, _ = _device_call(case, mode, float("nan"))
    assert np.isfinite(y1).all() and np.isfinite(lse1).all()
    np.testing.assert_array_equal(y1, y0)
    np.testing.assert_array_equal(lse1, lse0)
    np.testing.assert_array_equal(ws1[:need], ws0[:need])
    assert not np.isnan(ws1[:need]).any()
    assert (ws0[need:] == 12345.0).all() and (ws1[need:] == 12345.0).all() and ws1.size == need + 64
    # and device tensors carry the bits of host arrays
    yh, lseh, oph, l2h = _run(*case, mode, "bshd")
    np.testing.assert_array_equal(GQ.to_bhsd(y1, "bshd"), yh)
    np.testing.assert_array_equal(lse1, lseh)
    np.testing.assert_array_equal(ws1[:need], np.concatenate([oph.reshape(-1), l2h.reshape(-1)]))


@pytest.mark.parametrize("mode", MODES)
def test_batch_independence_and_repeatability(gpu, mode):
    """a batch entry computed alone carries the bits it has inside the batch (y, lse, partials); a repeated call repeats its bits"""
    shape, kind, causal, ks = (2, 17, 300, 6, 2, 32), "std1", 1, 3
    q, k, v, _ = SK.make_inputs(shape, kind)
    y, lse, op, l2 = _run(shape, kind, causal, ks, mode)
    S = op.shape[0]
    op, l2 = op.reshape(S, 2, -1, shape[5]), l2.reshape(S, 2, -1)
    for b in range(2):
        y1, lse1, (op1, l21) = _mode(mode, lambda ops: ops.flash_attention_splitkv(q[b:b + 1], k[b:b + 1], v[b:b + 1], causal=True, layout="bhsd", kv_splits=ks,
                                                                                    return_lse=True, return_partials=True))
        np.testing.assert_array_equal(y1[0], y[b])
        np.testing.assert_array_equal(lse1[0], lse[b])
        np.testing.assert_array_equal(op1, op[:, b])
        np.testing.assert_array_equal(l21, l2[:, b])
    again = _mode(mode, lambda ops: ops.flash_attention_splitkv(q, k, v, causal=True, layout="bhsd", kv_splits=ks, return_lse=True))
    np.testing.assert_array_equal(again[0], y)
    np.testing.assert_array_equal(again[1], lse)


def test_plane_modes_are_the_f32_kernel(gpu):
    """one exact fp32 kernel behind every mode that is not bf16 / f16: the same bits"""
    case = ((2, 17, 300, 6, 2, 32), "std1", 1, 3)
    for mode in ("f32_split3", "f32_split2", "f32_half2"):
        for x, y in zip(_run(*case, mode), _run(*case, "f32")):
            np.testing.assert_array_equal(x, y)


def test_a_refusal_leaves_the_next_call_alone(gpu):
    """each refusal is followed by a valid call that repeats its earlier bits"""
    import candle_birefnet_amd as cb
    shape, kind, causal, ks = (1, 2, 65, 2, 1, 128), "std1", 1, 2
    q, k, v, _ = SK.make_inputs(shape, kind)
    first = _run(shape, kind, causal, ks, "f32")
    for name, args, word in SK.refusals():
        st, msg = SK.raw_call(cb._ffi.lib, *args)
        assert st == 1 and msg.startswith("flash attention splitkv: ") and word in msg, (name, st, msg)
        y, lse = cb.ops.flash_attention_splitkv(q, k, v, causal=True, layout="bhsd", kv_splits=ks, return_lse=True)
        np.testing.assert_array_equal(y, first[0], err_msg=name)
        np.testing.assert_array_equal(lse, first[1], err_msg=name)
