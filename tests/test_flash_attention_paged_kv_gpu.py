"""brn_flash_attention_paged_kv_forward on the GPU: the paged entry over a pool STORED in bf16 / fp16.

The main statement is bit equality: in every (compute mode, pool type) pair the entry accepts, y, lse and the partials carry the bits of
brn_flash_attention_paged_forward in the same compute mode on the same pool widened to fp32 (the 16-bit kernels round an fp32 pool to
the type the 16-bit pool already holds, and the fp32 kernel widens exactly), whatever the loader's staging map is.  The cases, pools
(NaN wherever the entry must not read; the NaN pages stay NaN in 16 bits), reference and bounds are those of
tests/flash_attention_paged_cases.py, unchanged; the pool is PG.build_pool(case) rounded to the type with the suite's round_s16."""
import numpy as np
import pytest
import torch

import flash_attention_gqa_cases as GQ
import flash_attention_paged_cases as PG
import kv_cache_cases as KC

pytestmark = pytest.mark.gpu

PAIRS = list(KC.PAIRS)
PAIR_IDS = [f"{m}-on-{kv}" for m, kv in PAIRS]


def _mode(mode, fn):
    from candle_birefnet_amd import ops
    ops.set_compute(mode)
    try:
        return fn(ops)
    finally:
        ops.set_compute("f32")


_POOL, _RUN = {}, {}


def _pool(case, kv, page=None, shuffle=True):
    """(k bits, v bits, table, lens) of PG.build_pool rounded to kv (uint16, read-only); the NaN of the fp32 pool is NaN in 16 bits"""
    key = (case, kv, page, shuffle)
    if key not in _POOL:
        kp, vp, table, lens = PG.build_pool(case, page, shuffle)
        kb, vb = KC.to_bits(kp, kv), KC.to_bits(vp, kv)
        assert np.array_equal(np.isnan(KC.widen(kb, kv)), np.isnan(kp)) and np.isnan(kp).any()
        for a in (kb, vb):
            a.setflags(write=False)
        _POOL[key] = (kb, vb, table, lens)
    return _POOL[key]


def _call(ops, case, q, kp, vp, table, lens, layout, kv_dtype):
    _, _, _, kind, causal, ks = case
    y, lse, (op, l2) = ops.flash_attention_paged(q, kp, vp, table, lens, max_kv_len=PG.max_len(case), causal=bool(causal), scale=PG.kind_scale(kind), layout=layout,
                                                 kv_splits=ks, return_lse=True, return_partials=True, kv_dtype=kv_dtype)
    return y, lse, op, l2


def _run(case, mode, kv, layout="bhsd", page=None, shuffle=True, widened=False):
    """the new entry on the 16-bit pool (host arrays of bit patterns), or (widened) brn_flash_attention_paged_forward on that pool widened
    to fp32 -> (y as BHSD, lse, O_part or None, lse2_part or None); computed once (read-only)"""
    key = (case, mode, kv, layout, page, shuffle, widened)
    if key not in _RUN:
        q = PG.in_layout(PG.logical_inputs(case)[0], layout)
        kb, vb, table, lens = _pool(case, kv, page, shuffle)
        if widened:
            y, lse, op, l2 = _mode(mode, lambda ops: _call(ops, case, q, KC.widen(kb, kv), KC.widen(vb, kv), table, lens, layout, None))
        else:
            y, lse, op, l2 = _mode(mode, lambda ops: _call(ops, case, q, kb, vb, table, lens, layout, kv))
        assert y.shape == q.shape and lse.shape == (case[0][0], case[0][2], case[0][1])
        out = (GQ.to_bhsd(y, layout), lse, op, l2)
        for a in out:
            if a is not None:
                a.setflags(write=False)
        _RUN[key] = out
    return _RUN[key]


def _same_bits(got, want, what):
    for a, b, name in zip(got, want, ("y", "lse", "O_part", "lse2_part")):
        assert (a is None) == (b is None), (what, name)
        if a is not None:
            np.testing.assert_array_equal(a, b, err_msg=f"{name}: {what}")


@pytest.mark.parametrize("mode,kv", PAIRS, ids=PAIR_IDS)
@pytest.mark.parametrize("case", PG.CASES, ids=PG.case_id)
def test_bits_of_the_fp32_pool_entry_on_the_widened_pool(gpu, case, mode, kv):
    """y, lse, O_part and lse2_part, bit for bit, in every case and pair; both layouts for the first shape"""
    for layout in (("bhsd", "bshd") if case[0] == PG.FIRST[0] else ("bhsd",)):
        got, want = _run(case, mode, kv, layout), _run(case, mode, kv, layout, widened=True)
        assert (got[2] is None) == (PG.SK.plan(PG.max_len(case), case[5])[0] == 1)
        _same_bits(got, want, f"{PG.case_id(case)} {layout}")


@pytest.mark.parametrize("mode,kv", PAIRS, ids=PAIR_IDS)
def test_the_f32_pool_type_is_the_paged_entry(gpu, mode, kv):
    """BRN_KV_F32 through the new entry returns the bits of brn_flash_attention_paged_forward (one case per compute mode of the pairs)"""
    case = PG.FIRST
    _, _, _, kind, causal, ks = case
    q = PG.logical_inputs(case)[0]
    kp, vp, table, lens = PG.build_pool(case)
    want = _mode(mode, lambda ops: _call(ops, case, q, kp, vp, table, lens, "bhsd", None))
    got = _mode(mode, lambda ops: _call(ops, case, q, np.array(kp), np.array(vp), table, lens, "bhsd", "f32"))
    _same_bits(got, want, "kv_dtype f32")


@pytest.mark.parametrize("mode,kv", PAIRS, ids=PAIR_IDS)
def test_device_tensors_carry_the_bits_of_host_arrays(gpu, mode, kv):
    """torch.bfloat16 / torch.float16 tensors on the device (and, for f16, a numpy float16 array) against uint16 bit patterns on the host"""
    case = PG.FIRST
    kb, vb, table, lens = _pool(case, kv)
    q = PG.in_layout(PG.logical_inputs(case)[0], "bshd")
    tdt = torch.bfloat16 if kv == "bf16" else torch.float16
    dev = lambda a: torch.from_numpy(np.array(a)).cuda()
    kd, vd = (torch.from_numpy(np.array(a).view(np.int16)).view(tdt).cuda() for a in (kb, vb))
    y, lse, op, l2 = _mode(mode, lambda ops: _call(ops, case, dev(q), kd, vd, dev(table), dev(lens), "bshd", kv))
    torch.cuda.synchronize()
    got = (GQ.to_bhsd(y.cpu().numpy(), "bshd"), lse.cpu().numpy(), op.cpu().numpy(), l2.cpu().numpy())
    _same_bits(got, _run(case, mode, kv, "bshd"), "device tensors")
    if kv == "f16":
        host = _mode(mode, lambda ops: _call(ops, case, q, np.array(kb).view(np.float16), np.array(vb).view(np.float16), table, lens, "bshd", kv))
        _same_bits((GQ.to_bhsd(host[0], "bshd"),) + tuple(host[1:]), _run(case, mode, kv, "bshd"), "numpy float16")


@pytest.mark.parametrize("mode,kv", PAIRS, ids=PAIR_IDS)
def test_bits_do_not_depend_on_the_pages(gpu, mode, kv):
    """one logical batch in pages of 16, 64 and 256 keys, each with an identity and a shuffled table: one set of bits"""
    case = PG.FIRST[:4] + (1, 3)
    first = _run(case, mode, kv, page=16, shuffle=False)
    assert first[2] is not None
    for page in (16, 64, 256):
        for shuffle in (False, True):
            _same_bits(_run(case, mode, kv, page=page, shuffle=shuffle), first, f"page {page} shuffle {shuffle}")


@pytest.mark.parametrize("mode,kv", PAIRS, ids=PAIR_IDS)
@pytest.mark.parametrize("case", PG.CASES, ids=PG.case_id)
def test_nan_never_arrives(gpu, case, mode, kv):
    """every element of the pool the entry must not read is a 16-bit NaN: no output and no partial is NaN.  Implied by the bit equality,
    asserted on its own so that the message is clear"""
    y, lse, op, l2 = _run(case, mode, kv)
    assert not np.isnan(y).any(), "NaN from the pool reached y"
    assert not np.isnan(lse).any(), "NaN from the pool reached lse"
    assert op is None or not (np.isnan(op).any() or np.isnan(l2).any()), "NaN from the pool reached a partial"


@pytest.mark.parametrize("mode,kv", PAIRS, ids=PAIR_IDS)
@pytest.mark.parametrize("case", PG.CASES, ids=PG.case_id)
def test_parity_against_float64(gpu, case, mode, kv):
    """y within PG.y_bound and the finite lse within PG.lse_bound (both unchanged) of PG.reference on the pool's own values: k and v
    rounded to the pool's type, q rounded too in the 16-bit compute modes.  A row with no visible key is exactly 0 / -inf"""
    y, lse, op, l2 = _run(case, mode, kv)
    q, k, v = PG.logical_inputs(case)
    k16, v16 = (KC.widen(KC.to_bits(a, kv), kv) for a in (k, v))
    q_used = q if mode == "f32" else PG.round_s16(q, mode)
    ref, ref_lse = PG.reference(q_used, k16, v16, case[2], case[4], PG.kind_scale(case[3]))
    none = np.isneginf(ref_lse)
    assert int(none.sum()) == PG.all_empty_rows(case)
    assert (y[none] == 0).all() and np.isneginf(lse[none]).all() and np.isfinite(lse[~none]).all() and np.isfinite(y).all()
    err, bound = float(np.abs(np.asarray(y, np.float64) - ref).max()), PG.y_bound(ref, v16, mode)
    lerr, lbound = float(np.abs(np.asarray(lse[~none], np.float64) - ref_lse[~none]).max()), PG.lse_bound(ref_lse[~none])
    print(f"flash attention paged kv {mode} on {kv} {PG.case_id(case)}: y max abs err {err:.3e}, bound {bound:.3e}; lse {lerr:.3e}, bound {lbound:.3e}")
    assert err <= bound and lerr <= lbound
    if op is not None:
        empty = np.isneginf(l2)
        assert int(empty.sum()) == PG.empty_partial_rows(case) and (op[empty] == 0).all() and np.isfinite(op).all()


# ---- raw calls on device tensors ----
class _Dev:
    """a case on the device: q (BSHD), a 16-bit pool, the table, the lengths, and outputs / workspace allocated once"""

    def __init__(self, case, kv, pool=None, table=None, lens=None):
        import candle_birefnet_amd as cb
        (batch, seq_q, heads, kv_heads, hd), _, _, kind, causal, ks = case
        kb, vb, tb, ln = _pool(case, kv)
        self.kv = kv
        self.tdt = torch.bfloat16 if kv == "bf16" else torch.float16
        q = PG.in_layout(PG.logical_inputs(case)[0], "bshd")
        self.ints = (batch, seq_q, PG.max_len(case), heads, kv_heads, hd, kb.shape[0], kb.shape[1], tb.shape[1], 0, causal, PG.kind_scale(kind) or 0.0, ks)
        self.q = torch.from_numpy(np.array(q)).cuda()
        self.kp, self.vp = pool if pool is not None else (self.bits_to_device(a) for a in (kb, vb))
        self.table = torch.from_numpy(np.array(tb if table is None else table)).cuda()
        self.lens = torch.from_numpy(np.array(ln if lens is None else lens, dtype=np.int32)).cuda()
        self.S, _, self.need = cb.ops.flash_attention_splitkv_plan(batch, seq_q, PG.max_len(case), heads, kv_heads, hd, ks)
        self.ws = torch.zeros(self.need + 64, dtype=torch.float32, device="cuda")
        self.y = torch.empty(self.q.shape, dtype=torch.float32, device="cuda")
        self.lse = torch.empty((batch, heads, seq_q), dtype=torch.float32, device="cuda")

    def bits_to_device(self, bits):
        return torch.from_numpy(np.array(bits).view(np.int16)).view(self.tdt).cuda()

    def call(self, stream=None):
        import candle_birefnet_amd as cb
        st, msg = KC.raw_attend(cb._ffi.lib, self.q.data_ptr(), self.kp.data_ptr(), self.vp.data_ptr(), KC.KV_CODE[self.kv], self.table.data_ptr(), self.lens.data_ptr(),
                                *self.ints, self.y.data_ptr(), self.lse.data_ptr(), self.ws.data_ptr(), self.need, 1,
                                stream if stream is not None else torch.cuda.current_stream().cuda_stream)
        assert st == 0, msg

    def run(self, mode):
        self.y.fill_(float("nan"))
        self.lse.fill_(float("nan"))
        self.ws.fill_(float("nan"))
        self.ws[self.need:] = 12345.0
        _mode(mode, lambda ops: self.call())
        torch.cuda.synchronize()
        ws = self.ws.cpu().numpy()
        assert (ws[self.need:] == 12345.0).all(), "the workspace was written past its stated size"
        return self.y.cpu().numpy(), self.lse.cpu().numpy(), ws[:self.need]


@pytest.mark.parametrize("mode,kv", PAIRS, ids=PAIR_IDS)
def test_out_of_range_lengths_are_clamped(gpu, mode, kv):
    """kv_lens = max_kv_len + 1000 gives the bits of max_kv_len, kv_lens = -5 the bits of 0 (y = 0, lse = -inf)"""
    case = PG.FIRST[:2] + ((300, 300),) + PG.FIRST[3:]
    want = _Dev(case, kv, lens=(300, 0)).run(mode)
    got = _Dev(case, kv, lens=(1300, -5)).run(mode)
    assert np.isfinite(want[0]).all() and (want[0][1] == 0).all() and np.isneginf(want[1][1]).all() and np.isfinite(want[1][0]).all()
    for a, b in zip(got, want):
        np.testing.assert_array_equal(a, b)


@pytest.mark.parametrize("mode,kv", PAIRS, ids=PAIR_IDS)
def test_out_of_range_page_numbers_are_clamped(gpu, mode, kv):
    """As the page-clamp test of the fp32 entry: the pool is the MIDDLE of a larger device buffer whose margins (n_pages + 8 pages before
    and after, all NaN) cover every page number the test writes, so a missing clamp shows as NaN in a comparison, never as an access
    outside allocated memory.  The pool itself holds no NaN here (its poisoned elements are replaced by 0.5).  Table entries a sequence
    really uses are set to n_pages + 3 and -2; expected: the bits of the call with n_pages - 1 and 0 in those entries"""
    case = PG.FIRST
    kp, vp, table, lens = PG.build_pool(case)
    n_pages, margin = kp.shape[0], kp.shape[0] + 8
    probe = _Dev(case, kv)
    pools = []
    for a in (kp, vp):
        big = torch.full((n_pages + 2 * margin,) + a.shape[1:], float("nan"), dtype=probe.tdt, device="cuda")
        big[margin:margin + n_pages] = probe.bits_to_device(KC.to_bits(np.nan_to_num(a, nan=0.5), kv))
        pools.append(big)
    mid = tuple(b[margin:margin + n_pages] for b in pools)
    assert all(m.is_contiguous() and m.data_ptr() % 16 == 0 and m.data_ptr() == b.data_ptr() + 2 * margin * kp[0].size for m, b in zip(mid, pools))
    bad, good = table.copy(), table.copy()
    bad[0, 1], good[0, 1] = n_pages + 3, n_pages - 1          # sequence 0 (300 keys) uses entries 0 .. 18, sequence 1 (37 keys) 0 .. 2
    bad[0, 17], good[0, 17] = -2, 0
    bad[1, 2], good[1, 2] = -2, 0
    bad[1, 0], good[1, 0] = n_pages + 3, n_pages - 1
    want = _Dev(case, kv, pool=mid, table=good).run(mode)
    got = _Dev(case, kv, pool=mid, table=bad).run(mode)
    assert np.isfinite(want[0]).all() and np.isfinite(want[1]).all()
    for a, b in zip(got, want):
        np.testing.assert_array_equal(a, b)
    assert not np.array_equal(want[0], _Dev(case, kv, pool=mid).run(mode)[0])        # the entries are really used


def test_refusals_on_the_gpu_leave_the_next_call_alone(gpu):
    """kv_type 3, a bf16 pool in mode f16 and the reverse, a misaligned 16-bit pool: status 1 under the entry's prefix, and the valid call
    that follows repeats its earlier bits"""
    import candle_birefnet_amd as cb
    case = PG.FIFTH
    first = _run(case, "bf16", "bf16")
    picked = [r for r in KC.attend_refusals() if r[0] in ("kv_type 3", "a bf16 pool in mode f16", "an f16 pool in mode bf16", "misaligned device bf16 k_pages",
                                                         "misaligned device f16 v_pages")]
    assert len(picked) == 5
    q = PG.logical_inputs(case)[0]
    kb, vb, table, lens = _pool(case, "bf16")
    for name, args, word, mode in picked:
        st, msg = _mode(mode, lambda ops: KC.raw_attend(cb._ffi.lib, *args))
        assert st == 1 and msg.startswith("flash attention paged kv: ") and word in msg, (name, st, msg)
        again = _mode("bf16", lambda ops: _call(ops, case, q, kb, vb, table, lens, "bhsd", "bf16"))
        _same_bits(again, first, name)
