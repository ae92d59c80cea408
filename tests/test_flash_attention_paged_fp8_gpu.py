"""brn_flash_attention_paged_fp8_forward on the GPU: the paged entry over a pool of OCP e4m3fn bytes with one fp32 scale per K / V head.

The main statement is the contract's bits: in every compute mode lse, O_part and lse2_part carry the bits of
brn_flash_attention_paged_forward, in the same mode, on the fp32 pool WIDEN[bytes] called with scale = fl32(s * k_scale), and y is
fl32(v_scale * y of that call).  The pools are quantised on the CPU (kv_fp8_cases.quant), never by the append kernel; every byte the
entry must not read is 0xFF, a NaN.  Cases, reference and bounds are flash_attention_paged_cases', unchanged."""
import numpy as np
import pytest
import torch

import flash_attention_gqa_cases as GQ
import flash_attention_paged_cases as PG
import kv_fp8_cases as F8

pytestmark = pytest.mark.gpu
f32 = np.float32


def _mode(mode, fn):
    from candle_birefnet_amd import ops
    ops.set_compute(mode)
    try:
        return fn(ops)
    finally:
        ops.set_compute("f32")


def _kw(case, layout):
    return dict(max_kv_len=PG.max_len(case), causal=bool(case[4]), layout=layout, kv_splits=case[5], return_lse=True, return_partials=True)


def _fp8(ops, case, q, kb, vb, ks, vs, table, lens, layout="bhsd"):
    y, lse, (op, l2) = ops.flash_attention_paged_fp8(q, kb, vb, ks, vs, table, lens, scale=F8.case_scale(case), **_kw(case, layout))
    return y, lse, op, l2


def _fp32(ops, case, q, kf, vf, table, lens, scale, layout="bhsd"):
    y, lse, (op, l2) = ops.flash_attention_paged(q, kf, vf, table, lens, scale=float(scale), **_kw(case, layout))
    return y, lse, op, l2


_RUN = {}


def _run(case, mode, sk, layout="bhsd", page=None, shuffle=True, yardstick=False):
    """the fp8 entry on the CPU-quantised pool with the uniform scales SCALES[sk] (host arrays), or (yardstick) what the contract names:
    the fp32-pool entry on WIDEN[bytes] at fl32(s * k_scale), its y times v_scale in fp32 -> (y as BHSD, lse, O_part, lse2_part), once"""
    key = (case, mode, sk, layout, page, shuffle, yardstick)
    if key not in _RUN:
        _, ks, vs = F8.SCALES[sk]
        ksa, vsa = F8.scale_arrays(case[0][3], ks, vs)
        kb, vb, table, lens = F8.pool(case, ksa, vsa, page, shuffle)
        q = PG.in_layout(PG.logical_inputs(case)[0], layout)
        if yardstick:
            y, lse, op, l2 = _mode(mode, lambda ops: _fp32(ops, case, q, F8.WIDEN[kb], F8.WIDEN[vb], table, lens, f32(F8.case_scale(case)) * f32(ks), layout))
            y = (f32(vs) * y).astype(f32)
        else:
            y, lse, op, l2 = _mode(mode, lambda ops: _fp8(ops, case, q, np.array(kb), np.array(vb), ksa if sk else None, vsa if sk else None, table, lens, layout))
        assert y.shape == q.shape and y.dtype == f32
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


SK = list(range(len(F8.SCALES)))


# ---- 1. all 256 bytes ----
def _one_key_pool(rows):
    """two sequences of ONE key each, 8 K / V heads x 32: page 0 row 0 holds rows[0], page 2 row 0 rows[1] ([8, 32] bytes each); every
    other byte of the 4-page pool is UNREAD -> (pool bytes, table, lens)"""
    p = np.full((4, 16, 8, 32), F8.UNREAD, np.uint8)
    p[0, 0], p[2, 0] = rows
    return p, np.array([[0, 3], [2, 1]], np.int32), np.array([1, 1], np.int32)


ALL_BYTES = np.arange(256, dtype=np.uint8).reshape(8, 32)
FINITE_BYTES = np.where(np.isin(ALL_BYTES, F8.NAN_BYTES), 0, ALL_BYTES).astype(np.uint8)            # the two NaN bytes are replaced by 0


@pytest.mark.parametrize("mode", F8.MODES)
def test_all_256_bytes_through_v(gpu, mode):
    """len_b = 1: the softmax is exactly 1 and, with v_scale = 1, y IS the widened V row, in every mode: every byte's value, the
    subnormals included.  Bit for bit, but for the byte 0x80: its -0 is added to the accumulator's +0 and comes out as +0"""
    q = np.random.default_rng(5).standard_normal((2, 8, 1, 32)).astype(f32)
    vb, table, lens = _one_key_pool((FINITE_BYTES, FINITE_BYTES[::-1].copy()))
    kb, _, _ = _one_key_pool((np.full((8, 32), 0x38, np.uint8),) * 2)                                 # K = 1.0
    y = _mode(mode, lambda ops: ops.flash_attention_paged_fp8(q, kb, vb, None, None, table, lens, max_kv_len=16, scale=0.125, layout="bhsd", kv_splits=1))
    want = np.stack([F8.WIDEN[FINITE_BYTES], F8.WIDEN[FINITE_BYTES[::-1]]])[:, :, None, :]
    np.testing.assert_array_equal(y, want)
    not_neg0 = np.broadcast_to((np.stack([FINITE_BYTES, FINITE_BYTES[::-1]]) != 0x80)[:, :, None, :], y.shape)
    np.testing.assert_array_equal(y.view(np.uint32)[not_neg0], want.view(np.uint32)[not_neg0])
    assert int((~not_neg0).sum()) == 2 and (y[~not_neg0] == 0).all()


@pytest.mark.parametrize("mode", F8.MODES)
def test_all_256_bytes_through_k(gpu, mode):
    """the bytes in K, V = 1: lse = s * k_scale * q . k of the one key, the bits of the fp32-pool entry on the widened bytes"""
    q = np.random.default_rng(6).standard_normal((2, 8, 1, 32)).astype(f32)
    kb, table, lens = _one_key_pool((FINITE_BYTES, FINITE_BYTES[::-1].copy()))
    vb, _, _ = _one_key_pool((np.full((8, 32), 0x38, np.uint8),) * 2)
    ks = np.full(8, 0.0173, f32)
    kw = dict(max_kv_len=16, layout="bhsd", kv_splits=1, return_lse=True)
    y, lse = _mode(mode, lambda ops: ops.flash_attention_paged_fp8(q, kb, vb, ks, None, table, lens, scale=0.125, **kw))
    wy, wlse = _mode(mode, lambda ops: ops.flash_attention_paged(q, F8.WIDEN[kb], F8.WIDEN[vb], table, lens, scale=float(f32(0.125) * f32(0.0173)), **kw))
    np.testing.assert_array_equal(lse, wlse)
    np.testing.assert_array_equal(y, wy)
    assert np.isfinite(lse).all() and (y == 1).all() and np.abs(lse).max() > 0.5


# ---- 2. the contract's bits ----
@pytest.mark.parametrize("sk", SK, ids=F8.SCALE_IDS)
@pytest.mark.parametrize("mode", F8.MODES)
@pytest.mark.parametrize("case", PG.CASES, ids=PG.case_id)
def test_the_contracts_bits(gpu, case, mode, sk):
    """lse, O_part, lse2_part: the fp32-pool entry's on WIDEN[bytes] at fl32(s * k_scale); y: fl32(v_scale * its y).  Every case, mode
    and scale set; both layouts for the first shape"""
    for layout in (("bhsd", "bshd") if case[0] == PG.FIRST[0] else ("bhsd",)):
        got, want = _run(case, mode, sk, layout), _run(case, mode, sk, layout, yardstick=True)
        assert (got[2] is None) == (PG.SK.plan(PG.max_len(case), case[5])[0] == 1)
        _same_bits(got, want, f"{PG.case_id(case)} {layout}")


@pytest.mark.parametrize("mode", F8.MODES)
def test_scales_per_head_group_by_group(gpu, mode):
    """different scales per K / V head: every head group carries the bits of a kv_heads = 1 call of the fp32-pool entry on its slice of
    the widened pool at ITS scales (a row's bits do not depend on which rows share its launch)"""
    case = PG.FIRST
    (batch, seq_q, heads, kv_heads, hd), _, _, _, _, _ = case
    G = heads // kv_heads
    ks, vs = F8.per_head_scales(kv_heads)
    assert kv_heads > 1 and len(set(ks.tolist())) == kv_heads and len(set(vs.tolist())) == kv_heads
    kb, vb, table, lens = F8.pool(case, ks, vs)
    q = PG.logical_inputs(case)[0]
    y, lse, op, l2 = _mode(mode, lambda ops: _fp8(ops, case, q, np.array(kb), np.array(vb), ks, vs, table, lens))
    S = op.shape[0]
    op, l2 = op.reshape(S, batch, heads, seq_q, hd), l2.reshape(S, batch, heads, seq_q)
    for g in range(kv_heads):
        hs = slice(g * G, (g + 1) * G)
        sub = (case[0][:2] + (G, 1, hd),) + case[1:]
        kf, vf = (np.ascontiguousarray(F8.WIDEN[a[:, :, g:g + 1]]) for a in (kb, vb))
        wy, wlse, wop, wl2 = _mode(mode, lambda ops: _fp32(ops, sub, np.ascontiguousarray(q[:, hs]), kf, vf, table, lens, f32(F8.case_scale(case)) * ks[g]))
        np.testing.assert_array_equal(y[:, hs], (vs[g] * wy).astype(f32), err_msg=f"y of group {g}")
        np.testing.assert_array_equal(lse[:, hs], wlse, err_msg=f"lse of group {g}")
        np.testing.assert_array_equal(op[:, :, hs], wop.reshape(S, batch, G, seq_q, hd), err_msg=f"O_part of group {g}")
        np.testing.assert_array_equal(l2[:, :, hs], wl2.reshape(S, batch, G, seq_q), err_msg=f"lse2_part of group {g}")


# ---- 3. parity against float64 ----
@pytest.mark.parametrize("sk", SK, ids=F8.SCALE_IDS)
@pytest.mark.parametrize("mode", F8.MODES)
@pytest.mark.parametrize("case", PG.CASES, ids=PG.case_id)
def test_parity_against_float64(gpu, case, mode, sk):
    """y within PG.y_bound and the finite lse within PG.lse_bound (both unchanged) of PG.reference on the dequantised values
    scale * WIDEN[bytes]; q rounded in the 16-bit modes.  A row with no visible key is exactly 0 / -inf"""
    y, lse, op, l2 = _run(case, mode, sk)
    _, ks, vs = F8.SCALES[sk]
    ksa, vsa = F8.scale_arrays(case[0][3], ks, vs)
    q, k, v = PG.logical_inputs(case)
    # the logical k, v quantised as the pool's rows are: [batch, kv_heads, len, hd] -> bytes -> dequantised
    kd, vd = (np.swapaxes(F8.dequant(np.swapaxes(F8.quant(a, np.asarray(s, f32)[None, :, None, None]), 1, 2), s), 1, 2) for a, s in ((k, ksa), (v, vsa)))
    q_used = q if mode == "f32" else PG.round_s16(q, mode)
    ref, ref_lse = PG.reference(q_used, kd, vd, case[2], case[4], F8.case_scale(case))
    none = np.isneginf(ref_lse)
    assert int(none.sum()) == PG.all_empty_rows(case)
    assert (y[none] == 0).all() and np.isneginf(lse[none]).all() and np.isfinite(lse[~none]).all() and np.isfinite(y).all()
    err, bound = float(np.abs(np.asarray(y, np.float64) - ref).max()), PG.y_bound(ref, vd, mode)
    lerr, lbound = float(np.abs(np.asarray(lse[~none], np.float64) - ref_lse[~none]).max()), PG.lse_bound(ref_lse[~none])
    print(f"flash attention paged fp8 {mode} {F8.SCALE_IDS[sk]} {PG.case_id(case)}: y max abs err {err:.3e}, bound {bound:.3e}; lse {lerr:.3e}, bound {lbound:.3e}")
    assert err <= bound and lerr <= lbound
    if op is not None:
        empty = np.isneginf(l2)
        assert int(empty.sum()) == PG.empty_partial_rows(case) and (op[empty] == 0).all() and np.isfinite(op).all()


# ---- 4. pages, placement, device tensors, clamps ----
@pytest.mark.parametrize("mode", F8.MODES)
def test_bits_do_not_depend_on_the_pages(gpu, mode):
    """one logical batch in pages of 16 and 256 keys, each with an identity and a shuffled table: one set of bits"""
    case = PG.FIRST[:4] + (1, 3)
    first = _run(case, mode, 2, page=16, shuffle=False)
    assert first[2] is not None
    for page in (16, 256):
        for shuffle in (False, True):
            _same_bits(_run(case, mode, 2, page=page, shuffle=shuffle), first, f"page {page} shuffle {shuffle}")


@pytest.mark.parametrize("mode", F8.MODES)
def test_device_tensors_carry_the_bits_of_host_arrays(gpu, mode):
    """torch.uint8 and torch.float8_e4m3fn tensors on the device, scales on the device, against numpy bytes on the host"""
    case, sk = PG.FIRST, 2
    _, ks, vs = F8.SCALES[sk]
    ksa, vsa = F8.scale_arrays(case[0][3], ks, vs)
    kb, vb, table, lens = F8.pool(case, ksa, vsa)
    q = PG.in_layout(PG.logical_inputs(case)[0], "bshd")
    dev = lambda a: torch.from_numpy(np.array(a)).cuda()
    for view in (lambda t: t, lambda t: t.view(torch.float8_e4m3fn)):
        y, lse, op, l2 = _mode(mode, lambda ops: _fp8(ops, case, dev(q), view(dev(kb)), view(dev(vb)), dev(ksa), dev(vsa), dev(table), dev(lens), "bshd"))
        torch.cuda.synchronize()
        got = (GQ.to_bhsd(y.cpu().numpy(), "bshd"), lse.cpu().numpy(), op.cpu().numpy(), l2.cpu().numpy())
        _same_bits(got, _run(case, mode, sk, "bshd"), "device tensors")


class _Dev:
    """a case on the device: q (BSHD), an fp8 pool, scales, the table, the lengths, and outputs / workspace allocated once"""

    def __init__(self, case, sk=2, pool=None, table=None, lens=None):
        import candle_birefnet_amd as cb
        (batch, seq_q, heads, kv_heads, hd), _, _, _, causal, ks_ = case
        _, ks, vs = F8.SCALES[sk]
        ksa, vsa = F8.scale_arrays(kv_heads, ks, vs)
        kb, vb, tb, ln = F8.pool(case, ksa, vsa)
        q = PG.in_layout(PG.logical_inputs(case)[0], "bshd")
        self.ints = (batch, seq_q, PG.max_len(case), heads, kv_heads, hd, kb.shape[0], kb.shape[1], tb.shape[1], 0, causal, F8.case_scale(case), ks_)
        dev = lambda a, **kw: torch.from_numpy(np.array(a, **kw)).cuda()
        self.q = dev(q)
        self.kp, self.vp = pool if pool is not None else (dev(kb), dev(vb))
        self.ks, self.vs = dev(ksa), dev(vsa)
        self.table = dev(tb if table is None else table)
        self.lens = dev(ln if lens is None else lens, dtype=np.int32)
        self.S, _, self.need = cb.ops.flash_attention_splitkv_plan(batch, seq_q, PG.max_len(case), heads, kv_heads, hd, ks_)
        self.ws = torch.zeros(self.need + 64, dtype=torch.float32, device="cuda")
        self.y = torch.empty(self.q.shape, dtype=torch.float32, device="cuda")
        self.lse = torch.empty((batch, heads, seq_q), dtype=torch.float32, device="cuda")

    def call(self, stream=None):
        import candle_birefnet_amd as cb
        st, msg = F8.raw_attend(cb._ffi.lib, self.q.data_ptr(), self.kp.data_ptr(), self.vp.data_ptr(), self.ks.data_ptr(), self.vs.data_ptr(), self.table.data_ptr(),
                                self.lens.data_ptr(), *self.ints, self.y.data_ptr(), self.lse.data_ptr(), self.ws.data_ptr(), self.need, 1,
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


@pytest.mark.parametrize("mode", F8.MODES)
def test_out_of_range_lengths_are_clamped(gpu, mode):
    """kv_lens = max_kv_len + 1000 gives the bits of max_kv_len, kv_lens = -5 the bits of 0 (y = 0, lse = -inf)"""
    case = PG.FIRST[:2] + ((300, 300),) + PG.FIRST[3:]
    want = _Dev(case, lens=(300, 0)).run(mode)
    got = _Dev(case, lens=(1300, -5)).run(mode)
    assert np.isfinite(want[0]).all() and (want[0][1] == 0).all() and np.isneginf(want[1][1]).all() and np.isfinite(want[1][0]).all()
    for a, b in zip(got, want):
        np.testing.assert_array_equal(a, b)


@pytest.mark.parametrize("mode", F8.MODES)
def test_out_of_range_page_numbers_are_clamped(gpu, mode):
    """As the page-clamp test of the 16-bit entry: the pool is the MIDDLE of a larger device buffer whose margins (n_pages + 8 pages
    before and after, all 0xFF) cover every page number the test writes, so a missing clamp shows as NaN in a comparison, never as an
    access outside allocated memory.  The pool itself holds no NaN here (its unread bytes are replaced by 0x30 = 0.5).  Table entries a
    sequence really uses are set to n_pages + 3 and -2; expected: the bits of the call with n_pages - 1 and 0 in those entries"""
    case = PG.FIRST
    ksa, vsa = F8.scale_arrays(case[0][3], *F8.SCALES[2][1:])
    kb, vb, table, lens = F8.pool(case, ksa, vsa)
    n_pages, margin = kb.shape[0], kb.shape[0] + 8
    pools = []
    for a in (kb, vb):
        big = torch.full((n_pages + 2 * margin,) + a.shape[1:], F8.UNREAD, dtype=torch.uint8, device="cuda")
        big[margin:margin + n_pages] = torch.from_numpy(np.where(a == F8.UNREAD, 0x30, a).astype(np.uint8)).cuda()
        pools.append(big)
    mid = tuple(b[margin:margin + n_pages] for b in pools)
    assert all(m.is_contiguous() and m.data_ptr() % 16 == 0 and m.data_ptr() == b.data_ptr() + margin * kb[0].size for m, b in zip(mid, pools))
    bad, good = table.copy(), table.copy()
    bad[0, 1], good[0, 1] = n_pages + 3, n_pages - 1          # sequence 0 (300 keys) uses entries 0 .. 18, sequence 1 (37 keys) 0 .. 2
    bad[0, 17], good[0, 17] = -2, 0
    bad[1, 2], good[1, 2] = -2, 0
    bad[1, 0], good[1, 0] = n_pages + 3, n_pages - 1
    want = _Dev(case, pool=mid, table=good).run(mode)
    got = _Dev(case, pool=mid, table=bad).run(mode)
    assert np.isfinite(want[0]).all() and np.isfinite(want[1]).all()
    for a, b in zip(got, want):
        np.testing.assert_array_equal(a, b)
    assert not np.array_equal(want[0], _Dev(case, pool=mid).run(mode)[0])        # the entries are really used


# ---- 5. NaN never arrives ----
@pytest.mark.parametrize("sk", SK, ids=F8.SCALE_IDS)
@pytest.mark.parametrize("mode", F8.MODES)
@pytest.mark.parametrize("case", PG.CASES, ids=PG.case_id)
def test_nan_never_arrives(gpu, case, mode, sk):
    """every unread row and unused page of the pool is 0xFF: no output and no partial is NaN"""
    y, lse, op, l2 = _run(case, mode, sk)
    assert not np.isnan(y).any(), "NaN from the pool reached y"
    assert not np.isnan(lse).any(), "NaN from the pool reached lse"
    assert op is None or not (np.isnan(op).any() or np.isnan(l2).any()), "NaN from the pool reached a partial"


# ---- 6. append + attention, one graph ----
STEP = 3


class _Step(_Dev):
    """a decode state: the pool holds the first len_b - 3 keys of every sequence (quantised on the CPU at the start scales, every other
    byte UNREAD), lengths at len_b - 3, the last 3 keys of every sequence as fp32 tokens [batch, 3, kv_heads, hd]"""

    def __init__(self, case):
        super().__init__(case)
        (batch, _, _, kv_heads, hd), page, lens, _, _, _ = case
        _, k, v = PG.logical_inputs(case)
        _, _, table, _ = PG.build_pool(case)
        start = np.asarray(lens, np.int32) - STEP
        keep = np.zeros((self.ints[6], page), bool)
        for b in range(batch):
            pos = np.arange(start[b])
            keep[table[b, pos // page], pos % page] = True
        for t in (self.kp, self.vp):
            t[torch.from_numpy(~keep).cuda()] = F8.UNREAD
        self.tokens = tuple(torch.from_numpy(np.stack([a[b, :, lens[b] - STEP:lens[b]].transpose(1, 0, 2) for b in range(batch)]).astype(f32)).cuda() for a in (k, v))
        self.lens = torch.from_numpy(start).cuda()
        self.geo = (batch, kv_heads, hd, self.ints[6], page, table.shape[1])
        self.y.fill_(float("nan"))
        self.lse.fill_(float("nan"))

    def append(self, k_new, v_new, stream=None):
        import candle_birefnet_amd as cb
        batch, kv_heads, hd, n_pages, page, max_pages = self.geo
        st, msg = F8.raw_append(cb._ffi.lib, k_new.data_ptr(), v_new.data_ptr(), batch, int(k_new.shape[1]), kv_heads, hd, 0, self.kp.data_ptr(), self.vp.data_ptr(),
                                self.ks.data_ptr(), self.vs.data_ptr(), self.table.data_ptr(), self.lens.data_ptr(), self.lens.data_ptr(), n_pages, page, max_pages, 1,
                                stream if stream is not None else torch.cuda.current_stream().cuda_stream)
        assert st == 0, msg

    def results(self):
        torch.cuda.synchronize()
        return GQ.to_bhsd(self.y.cpu().numpy(), "bshd"), self.lse.cpu().numpy(), self.lens.cpu().numpy()


@pytest.mark.parametrize("mode", F8.MODES)
def test_one_graph_is_a_decode_step(gpu, mode):
    """On a side stream, brn_kv_cache_append_fp8 (one token per sequence, lengths in place) followed by the fp8 paged attention is
    captured into one graph.  Three replays, each after new q / k_new / v_new were copied into the captured input tensors and the two
    scale arrays were CHANGED in place, give the y, lse, lengths and pool bytes of the eager pair of calls on a second pool kept in step"""
    case = PG.FIRST
    lens = case[2]
    graph_side, eager_side = _Step(case), _Step(case)
    q = PG.logical_inputs(case)[0]
    k_in, v_in = (torch.zeros_like(t[:, :1]).contiguous() for t in graph_side.tokens)
    step_scales = [(ks * m, vs * n) for (ks, vs), m, n in zip([F8.per_head_scales(case[0][3])] * STEP, (1.0, 2.0, 0.75), (1.0, 0.5, 1.25))]

    def body(ops):
        eager_side.append(k_in, v_in)                           # warm: the library and its kernels are loaded before the capture
        eager_side.call()
        torch.cuda.synchronize()
        fresh = _Step(case)                                     # (the warm-up moved the eager side: start it again)
        eager_side.kp, eager_side.vp, eager_side.lens = fresh.kp, fresh.vp, fresh.lens
        side = torch.cuda.Stream()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            s = torch.cuda.current_stream().cuda_stream
            graph_side.append(k_in, v_in, stream=s)
            graph_side.call(stream=s)
        seen = []
        for step in range(STEP):
            tk, tv = (t[:, step:step + 1].contiguous() for t in graph_side.tokens)
            qn = torch.from_numpy(PG.in_layout(np.roll(q, step, axis=1), "bshd")).cuda()      # a new q each step: the heads rotate
            ksn, vsn = (torch.from_numpy(a.astype(f32)).cuda() for a in step_scales[step])
            for dst, src in ((k_in, tk), (v_in, tv), (graph_side.q, qn), (eager_side.q, qn), (graph_side.ks, ksn), (graph_side.vs, vsn), (eager_side.ks, ksn), (eager_side.vs, vsn)):
                dst.copy_(src)
            eager_side.append(tk, tv)
            eager_side.call()
            want = eager_side.results()
            graph_side.y.fill_(float("nan"))
            graph_side.lse.fill_(float("nan"))
            torch.cuda.synchronize()
            graph.replay()
            got = graph_side.results()
            for a, b, what in zip(got, want, ("y", "lse", "kv_lens")):
                np.testing.assert_array_equal(a, b, err_msg=f"{what} of replay {step}")
            assert got[2].tolist() == [L - STEP + step + 1 for L in lens] and np.isfinite(got[0]).all()
            seen.append(got[0])
        assert not np.array_equal(seen[0], seen[1]) and not np.array_equal(seen[1], seen[2])
        np.testing.assert_array_equal(graph_side.kp.cpu().numpy(), eager_side.kp.cpu().numpy())
        np.testing.assert_array_equal(graph_side.vp.cpu().numpy(), eager_side.vp.cpu().numpy())
    _mode(mode, body)


# ---- 7. refusals ----
def test_refusals_on_the_gpu_leave_the_next_call_alone(gpu):
    """status 1 under the entry's prefix, and the valid call that follows repeats its earlier bits"""
    import candle_birefnet_amd as cb
    case, sk = PG.FIFTH, 2
    first = _run(case, "bf16", sk)
    picked = [r for r in F8.attend_refusals() if r[0] in ("misaligned device fp8 k_pages", "misaligned device k_scale", "y is k_scale", "page_size 48",
                                                          "workspace overlaps the end of an fp8 v_pages (bytes)")]
    assert len(picked) == 5
    ksa, vsa = F8.scale_arrays(case[0][3], *F8.SCALES[sk][1:])
    kb, vb, table, lens = F8.pool(case, ksa, vsa)
    q = PG.logical_inputs(case)[0]
    for name, args, word in picked:
        st, msg = F8.raw_attend(cb._ffi.lib, *args)
        assert st == 1 and msg.startswith("flash attention paged fp8: ") and word in msg, (name, st, msg)
        again = _mode("bf16", lambda ops: _fp8(ops, case, q, np.array(kb), np.array(vb), ksa, vsa, table, lens))
        _same_bits(again, first, name)
