"""brn_flash_attention_paged_forward on the GPU: the split entry over a paged K / V cache with per-sequence lengths on the device.

What is index semantics is pinned BIT FOR BIT: a sequence carries the bits of brn_flash_attention_splitkv_forward on its keys gathered
into a dense tensor; the bits do not depend on the page size, on where the pages lie, on the batch or on the workspace's old content;
out-of-range device values give the bits of their clamped values; a graph replay gives the eager call's bits.  Parity against float64
uses the bounds of tests/test_flash_attention_splitkv_gpu.py unchanged; tests/test_flash_attention_paged_cpu.py records that the
emulation stays inside them on these inputs.  Every pool is filled with NaN wherever the entry must not read."""
import numpy as np
import pytest
import torch

import flash_attention_gqa_cases as GQ
import flash_attention_paged_cases as PG
import flash_attention_splitkv_cases as SK

pytestmark = pytest.mark.gpu

MODES = list(PG.MODES)


def _mode(mode, fn):
    from candle_birefnet_amd import ops
    ops.set_compute(mode)
    try:
        return fn(ops)
    finally:
        ops.set_compute("f32")


_RUN = {}


def _run(case, mode="f32", layout="bhsd", page=None, shuffle=True):
    """the entry on host arrays through the NaN-filled pool of the case -> (y as BHSD, lse, O_part [S, R, D] or None, lse2_part or None);
    computed once (read-only)"""
    key = (case, mode, layout, page, shuffle)
    if key not in _RUN:
        _, _, _, kind, causal, ks = case
        q = PG.in_layout(PG.logical_inputs(case)[0], layout)
        kp, vp, table, lens = PG.build_pool(case, page, shuffle)
        y, lse, (op, l2) = _mode(mode, lambda ops: ops.flash_attention_paged(q, kp, vp, table, lens, max_kv_len=PG.max_len(case), causal=bool(causal),
                                                                              scale=PG.kind_scale(kind), layout=layout, kv_splits=ks, return_lse=True,
                                                                              return_partials=True))
        assert y.shape == q.shape and lse.shape == (case[0][0], case[0][2], case[0][1])
        out = (GQ.to_bhsd(y, layout), lse, op, l2)
        for a in out:
            if a is not None:
                a.setflags(write=False)
        _RUN[key] = out
    return _RUN[key]


def _dense(case, b, mode, layout):
    """brn_flash_attention_splitkv_forward on sequence b alone: batch 1, seq_kv = len_b, the kv_splits of PG.dense_splits"""
    _, _, lens, kind, causal, _ = case
    q, k, v = PG.logical_inputs(case)
    args = [PG.in_layout(np.ascontiguousarray(a), layout) for a in (q[b:b + 1], k[b:b + 1, :, :lens[b]], v[b:b + 1, :, :lens[b]])]
    y, lse, (op, l2) = _mode(mode, lambda ops: ops.flash_attention_splitkv(*args, causal=bool(causal), scale=PG.kind_scale(kind), layout=layout,
                                                                            kv_splits=PG.dense_splits(case, b), return_lse=True, return_partials=True))
    return GQ.to_bhsd(y, layout), lse, op, l2


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("case", PG.CASES, ids=PG.case_id)
def test_a_sequence_carries_the_bits_of_the_split_entry_on_its_gathered_keys(gpu, case, mode):
    """every sequence the split entry accepts: y and lse of its rows, and its partials of the splits s < S_b the dense call has, bit for
    bit; its partials of the splits past its end exactly 0 / -inf.  Both layouts for the first shape"""
    (batch, seq_q, heads, _, hd), _, lens, _, _, ks = case
    S, _ = SK.plan(PG.max_len(case), ks)
    rows = heads * seq_q
    checked = 0
    for layout in (("bhsd", "bshd") if case[0] == PG.FIRST[0] else ("bhsd",)):
        y, lse, op, l2 = _run(case, mode, layout)
        assert (op is None) == (S == 1)
        for b in range(batch):
            if PG.dense_splits(case, b) is None:
                continue
            yd, lsed, opd, l2d = _dense(case, b, mode, layout)
            np.testing.assert_array_equal(y[b], yd[0], err_msg=f"y of sequence {b} {layout}")
            np.testing.assert_array_equal(lse[b], lsed[0], err_msg=f"lse of sequence {b} {layout}")
            checked += 1
            if op is None:
                continue
            opb, l2b = op.reshape(S, batch, rows, hd)[:, b], l2.reshape(S, batch, rows)[:, b]
            if opd is None:          # the dense call had one split: its y and lse ARE its partial (lse = ln 2 * lse2, one fp32 product)
                S_b = 1
                np.testing.assert_array_equal(opb[0], yd.reshape(rows, hd))
                np.testing.assert_array_equal(l2b[0] * np.float32(PG.LN2), lsed.reshape(rows))
            else:
                S_b = opd.shape[0]
                np.testing.assert_array_equal(opb[:S_b], opd)
                np.testing.assert_array_equal(l2b[:S_b], l2d)
            assert (opb[S_b:] == 0).all() and np.isneginf(l2b[S_b:]).all()
    assert checked > 0


@pytest.mark.parametrize("mode", MODES)
def test_bits_do_not_depend_on_the_pages(gpu, mode):
    """one logical batch in pages of 16, 64 and 256 keys, each with an identity and a shuffled table: one set of bits (y, lse, partials)"""
    case = PG.FIRST[:4] + (1, 3)
    first = _run(case, mode, page=16, shuffle=False)
    assert first[2] is not None
    for page in (16, 64, 256):
        for shuffle in (False, True):
            for a, b in zip(_run(case, mode, page=page, shuffle=shuffle), first):
                np.testing.assert_array_equal(a, b, err_msg=f"page {page} shuffle {shuffle}")


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("case", PG.CASES, ids=PG.case_id)
def test_nan_never_arrives(gpu, case, mode):
    """every float of the pool the entry must not read is NaN (unused pages, rows of a last page past len_b, the pages unused table
    entries name): no output and no partial is NaN.  Implied by the dense equivalence, asserted on its own so that the message is clear"""
    y, lse, op, l2 = _run(case, mode)
    assert not np.isnan(y).any(), "NaN from the pool reached y"
    assert not np.isnan(lse).any(), "NaN from the pool reached lse"
    assert op is None or not (np.isnan(op).any() or np.isnan(l2).any()), "NaN from the pool reached a partial"


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("case", PG.CASES, ids=PG.case_id)
def test_parity_against_float64(gpu, case, mode):
    """y within f32_bound / s16_bound and the finite lse within lse_bound of the float64 reference; a row no split has a key for is
    exactly 0 / -inf; the empty partials are 0 / -inf and as many as the mask says"""
    y, lse, op, l2 = _run(case, mode)
    v = PG.logical_inputs(case)[2]
    ref, ref_lse = PG.case_reference(case, None if mode == "f32" else mode)
    none = np.isneginf(ref_lse)
    assert int(none.sum()) == PG.all_empty_rows(case)
    assert (y[none] == 0).all() and np.isneginf(lse[none]).all() and np.isfinite(lse[~none]).all() and np.isfinite(y).all()
    err, bound = float(np.abs(np.asarray(y, np.float64) - ref).max()), PG.y_bound(ref, v, mode)
    lerr, lbound = float(np.abs(np.asarray(lse[~none], np.float64) - ref_lse[~none]).max()), PG.lse_bound(ref_lse[~none])
    print(f"flash attention paged {mode} {PG.case_id(case)}: y max abs err {err:.3e}, bound {bound:.3e}; lse {lerr:.3e}, bound {lbound:.3e}")
    assert err <= bound and lerr <= lbound
    if op is not None:
        empty = np.isneginf(l2)
        assert int(empty.sum()) == PG.empty_partial_rows(case) and (op[empty] == 0).all() and np.isfinite(op).all()


# ---- raw calls on device tensors ----
class _Dev:
    """a case on the device: q (BSHD), the pool, the table, the lengths, and outputs / workspace allocated once"""

    def __init__(self, case, pool=None, table=None, lens=None, extra=64):
        import candle_birefnet_amd as cb
        self.case = case
        (batch, seq_q, heads, kv_heads, hd), _, _, kind, causal, ks = case
        kp, vp, tb, ln = PG.build_pool(case)
        q = PG.in_layout(PG.logical_inputs(case)[0], "bshd")
        self.ints = (batch, seq_q, PG.max_len(case), heads, kv_heads, hd, kp.shape[0], kp.shape[1], tb.shape[1], 0, causal, PG.kind_scale(kind) or 0.0, ks)
        self.q = torch.from_numpy(np.array(q)).cuda()
        self.kp, self.vp = pool if pool is not None else (torch.from_numpy(np.array(a)).cuda() for a in (kp, vp))
        self.table = torch.from_numpy(np.array(tb if table is None else table)).cuda()
        self.lens = torch.from_numpy(np.array(ln if lens is None else lens, dtype=np.int32)).cuda()
        self.S, _, self.need = cb.ops.flash_attention_splitkv_plan(batch, seq_q, PG.max_len(case), heads, kv_heads, hd, ks)
        self.ws = torch.zeros(self.need + extra, dtype=torch.float32, device="cuda")
        self.y = torch.empty(self.q.shape, dtype=torch.float32, device="cuda")
        self.lse = torch.empty((batch, heads, seq_q), dtype=torch.float32, device="cuda")

    def call(self, stream=None, ws=True):
        """one raw library call on the current (or the given) stream; no synchronisation"""
        import candle_birefnet_amd as cb
        st, msg = PG.raw_call(cb._ffi.lib, self.q.data_ptr(), self.kp.data_ptr(), self.vp.data_ptr(), self.table.data_ptr(), self.lens.data_ptr(), *self.ints,
                              self.y.data_ptr(), self.lse.data_ptr(), self.ws.data_ptr() if ws else None, self.need if ws else 0, 1,
                              stream if stream is not None else torch.cuda.current_stream().cuda_stream)
        assert st == 0, msg

    def run(self, mode="f32", fill=None, sentinel=12345.0):
        """fill the outputs with NaN (and the workspace with `fill`, the floats past its stated size with `sentinel`), call, synchronise
        -> (y, lse, workspace) as numpy"""
        self.y.fill_(float("nan"))
        self.lse.fill_(float("nan"))
        if fill is not None:
            self.ws.fill_(fill)
            self.ws[self.need:] = sentinel
        _mode(mode, lambda ops: self.call())
        torch.cuda.synchronize()
        return self.y.cpu().numpy(), self.lse.cpu().numpy(), self.ws.cpu().numpy()


@pytest.mark.parametrize("mode", MODES)
def test_out_of_range_lengths_are_clamped(gpu, mode):
    """kv_lens = max_kv_len + 1000 gives the bits of max_kv_len, kv_lens = -5 the bits of 0 (y = 0, lse = -inf)"""
    case = PG.FIRST[:2] + ((300, 300),) + PG.FIRST[3:]
    want = _Dev(case, lens=(300, 0)).run(mode, 0.0)
    got = _Dev(case, lens=(1300, -5)).run(mode, 0.0)
    assert np.isfinite(want[0]).all() and (want[0][1] == 0).all() and np.isneginf(want[1][1]).all() and np.isfinite(want[1][0]).all()
    for a, b in zip(got, want):
        np.testing.assert_array_equal(a, b)


@pytest.mark.parametrize("mode", MODES)
def test_out_of_range_page_numbers_are_clamped(gpu, mode):
    """The pool is the MIDDLE of a larger device buffer whose margins (n_pages + 8 pages before and after, all NaN) cover every page
    number the test writes, so a missing clamp shows as NaN in a comparison, never as an access outside allocated memory.  The pool itself
    holds no NaN here (its poisoned floats are replaced by 0.5): the clamped pages are real ones.  Table entries a sequence really uses
    are set to n_pages + 3 and -2; expected: the bits of the call with n_pages - 1 and 0 in those entries"""
    case = PG.FIRST
    kp, vp, table, lens = PG.build_pool(case)
    n_pages, margin = kp.shape[0], kp.shape[0] + 8
    pools = []
    for a in (kp, vp):
        big = torch.full((n_pages + 2 * margin,) + a.shape[1:], float("nan"), dtype=torch.float32, device="cuda")
        big[margin:margin + n_pages] = torch.from_numpy(np.nan_to_num(a, nan=0.5)).cuda()
        pools.append(big)
    mid = tuple(b[margin:margin + n_pages] for b in pools)
    assert all(m.is_contiguous() and m.data_ptr() % 16 == 0 and m.data_ptr() == b.data_ptr() + 4 * margin * kp[0].size for m, b in zip(mid, pools))
    bad, good = table.copy(), table.copy()
    bad[0, 1], good[0, 1] = n_pages + 3, n_pages - 1          # sequence 0 (300 keys) uses entries 0 .. 18, sequence 1 (37 keys) 0 .. 2
    bad[0, 17], good[0, 17] = -2, 0
    bad[1, 2], good[1, 2] = -2, 0
    bad[1, 0], good[1, 0] = n_pages + 3, n_pages - 1
    want = _Dev(case, pool=mid, table=good).run(mode, 0.0)
    got = _Dev(case, pool=mid, table=bad).run(mode, 0.0)
    assert np.isfinite(want[0]).all() and np.isfinite(want[1]).all()
    for a, b in zip(got, want):
        np.testing.assert_array_equal(a, b)
    assert not np.array_equal(want[0], _Dev(case, pool=mid).run(mode, 0.0)[0])        # the entries are really used


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("case", (PG.FIRST, PG.THIRD, PG.FIFTH), ids=PG.case_id)
def test_workspace_is_written_before_it_is_read_and_not_past_its_size(gpu, case, mode):
    """a workspace pre-filled with NaN gives the bits of a zero-filled one (every partial row, empty ones included, is written before the
    combine reads it); the 64 floats past the stated size keep their sentinel; device tensors carry the bits of host arrays"""
    dev = _Dev(case)
    y0, lse0, ws0 = dev.run(mode, 0.0)
    y1, lse1, ws1 = dev.run(mode, float("nan"))
    need = dev.need
    np.testing.assert_array_equal(y1, y0)
    np.testing.assert_array_equal(lse1, lse0)
    np.testing.assert_array_equal(ws1[:need], ws0[:need])
    assert not np.isnan(y1).any() and not np.isnan(lse1).any() and not np.isnan(ws1[:need]).any()
    assert (ws0[need:] == 12345.0).all() and (ws1[need:] == 12345.0).all() and ws1.size == need + 64
    yh, lseh, oph, l2h = _run(case, mode, "bshd")
    np.testing.assert_array_equal(GQ.to_bhsd(y1, "bshd"), yh)
    np.testing.assert_array_equal(lse1, lseh)
    np.testing.assert_array_equal(ws1[:need], np.concatenate([oph.reshape(-1), l2h.reshape(-1)]))


def test_one_split_works_without_a_workspace(gpu):
    """S == 1 (the collapsed case, and kv_splits 1 over ragged lengths): a NULL workspace, y and lse written directly"""
    for case in (PG.COLLAPSED, PG.CASES[0]):
        dev = _Dev(case)
        assert dev.S == 1
        dev.y.fill_(float("nan"))
        dev.lse.fill_(float("nan"))
        dev.call(ws=False)
        torch.cuda.synchronize()
        yh, lseh, oph, _ = _run(case, "f32", "bshd")
        assert oph is None
        np.testing.assert_array_equal(GQ.to_bhsd(dev.y.cpu().numpy(), "bshd"), yh)
        np.testing.assert_array_equal(dev.lse.cpu().numpy(), lseh)


@pytest.mark.parametrize("mode", MODES)
def test_batch_independence_and_repeatability(gpu, mode):
    """a sequence computed alone (batch 1, the same max_kv_len and pool) carries the bits it has inside the batch (y, lse, partials); a
    repeated call repeats its bits"""
    case = next(c for c in PG.CASES if c[3] == "rising" and c[5] == 3)
    (batch, seq_q, heads, _, hd), _, _, kind, causal, ks = case
    q = PG.logical_inputs(case)[0]
    kp, vp, table, lens = PG.build_pool(case)
    y, lse, op, l2 = _run(case, mode)
    S = op.shape[0]
    op, l2 = op.reshape(S, batch, -1, hd), l2.reshape(S, batch, -1)
    kw = dict(max_kv_len=PG.max_len(case), causal=bool(causal), scale=PG.kind_scale(kind), layout="bhsd", kv_splits=ks, return_lse=True, return_partials=True)
    for b in range(batch):
        y1, lse1, (op1, l21) = _mode(mode, lambda ops: ops.flash_attention_paged(q[b:b + 1], kp, vp, table[b:b + 1], lens[b:b + 1], **kw))
        np.testing.assert_array_equal(y1[0], y[b])
        np.testing.assert_array_equal(lse1[0], lse[b])
        np.testing.assert_array_equal(op1, op[:, b])
        np.testing.assert_array_equal(l21, l2[:, b])
    again = _mode(mode, lambda ops: ops.flash_attention_paged(q, kp, vp, table, lens, **kw))
    np.testing.assert_array_equal(again[0], y)
    np.testing.assert_array_equal(again[1], lse)


def test_plane_modes_are_the_f32_kernel(gpu):
    """one exact fp32 kernel behind every mode that is not bf16 / f16: the same bits"""
    case = PG.FIFTH
    for mode in ("f32_split3", "f32_split2", "f32_half2"):
        for x, y in zip(_run(case, mode), _run(case, "f32")):
            np.testing.assert_array_equal(x, y)


def test_replayed_from_a_graph_while_lengths_and_table_change(gpu):
    """Raw library calls on preallocated device buffers, captured on a side stream into one graph (one branch).  Each replay gives the bits
    of the eager call on the same device state; between replays kv_lens and two table entries change on the device with ordinary tensor
    copies.  The entry allocates nothing and does not synchronise, or the capture would fail"""
    case = PG.FIRST[:2] + ((300, 300),) + PG.FIRST[3:]
    dev = _Dev(case)
    n_pages = dev.kp.shape[0]
    side = torch.cuda.Stream()
    graph = torch.cuda.CUDAGraph()
    dev.run()                                                  # warm: the library and its kernels are loaded before the capture
    with torch.cuda.graph(graph, stream=side):
        dev.call(stream=torch.cuda.current_stream().cuda_stream)
    t0 = dev.table.cpu().numpy()
    states = [((300, 37), t0), ((120, 300), t0)]
    t1 = t0.copy()
    t1[0, 0], t1[1, 0] = t0[1, 0], t0[0, 0]                   # two entries in use trade places: each sequence starts with the other's first 16 keys
    states.append(((300, 1), t1))
    seen = []
    for lens, table in states:
        dev.lens.copy_(torch.tensor(lens, dtype=torch.int32))
        dev.table.copy_(torch.from_numpy(table))
        assert int(dev.table.max()) < n_pages
        eager = dev.run()
        dev.y.fill_(float("nan"))
        dev.lse.fill_(float("nan"))
        dev.ws.fill_(float("nan"))
        torch.cuda.synchronize()
        graph.replay()
        torch.cuda.synchronize()
        got = (dev.y.cpu().numpy(), dev.lse.cpu().numpy())
        np.testing.assert_array_equal(got[0], eager[0], err_msg=f"replay with kv_lens {lens}")
        np.testing.assert_array_equal(got[1], eager[1], err_msg=f"replay with kv_lens {lens}")
        assert np.isfinite(got[0]).all()
        seen.append(got[0])
    assert not np.array_equal(seen[0], seen[1]) and not np.array_equal(seen[0][0], seen[2][0])


def test_a_refusal_leaves_the_next_call_alone(gpu):
    """each refusal is followed by a valid call that repeats its earlier bits"""
    import candle_birefnet_amd as cb
    case = PG.FIFTH
    _, _, _, kind, causal, ks = case
    q = PG.logical_inputs(case)[0]
    pool = PG.build_pool(case)
    first = _run(case, "f32")
    for name, args, word in PG.refusals():
        st, msg = PG.raw_call(cb._ffi.lib, *args)
        assert st == 1 and msg.startswith("flash attention paged: ") and word in msg, (name, st, msg)
        y, lse = cb.ops.flash_attention_paged(q, *pool, max_kv_len=PG.max_len(case), causal=bool(causal), layout="bhsd", kv_splits=ks, return_lse=True)
        np.testing.assert_array_equal(y, first[0], err_msg=name)
        np.testing.assert_array_equal(lse, first[1], err_msg=name)
