"""brn_flash_attention_paged_varlen_forward on the GPU: paged attention over a packed batch of new tokens with cu_seqlens_q on the device.

The main statement is the contract's bits: every sequence of a packed call carries, for y, lse and the partials, the bits of the EXISTING
paged entry of its pool type (brn_flash_attention_paged_forward / _kv_forward / _fp8_forward) called on that sequence alone with batch 1,
seq_q = n_b, the same max_kv_len and the same explicit kv_splits.  The per-sequence calls are made once (each on a pool of page size 16
that holds that sequence alone) and shared: a sequence's data does not depend on its place in a pack, so the same yardstick serves
either page size, either place of the pack, permuted packs and padded n_seqs / total_q.  y, lse and the workspace of every packed
call start as a sentinel; q's padding rows and everything of the pool no entry may read are NaN."""
import numpy as np
import pytest
import torch

import flash_attention_paged_cases as PG
import flash_attention_paged_varlen_cases as PV
import kv_cache_cases as KC

pytestmark = pytest.mark.gpu
f32 = np.float32
SENT = f32(-1234.5)                       # what a row no kernel writes must still hold (finite: "no NaN arrives" stays checkable)


def _mode(mode, fn):
    from candle_birefnet_amd import ops
    ops.set_compute(mode)
    try:
        return fn(ops)
    finally:
        ops.set_compute("f32")


def _packed(ops, cfg, q, pool_arrays, pool, cu, causal, ks, total_q=None):
    """one packed call on host arrays with sentinel-filled outputs -> (y [total_q, heads, hd], lse [heads, total_q], O_part
    [S, heads, total_q, hd] or None, lse2_part [S, heads, total_q] or None, the whole workspace)"""
    heads, kv_heads, hd = cfg
    kp, vp, ksc, vsc, table, lens = pool_arrays
    total_q = total_q or q.shape[0]
    S, _, nws, _ = ops.flash_attention_paged_varlen_plan(total_q, table.shape[0], PV.MAX_KV, heads, kv_heads, hd, ks)
    y, lse, ws = np.full((total_q, heads, hd), SENT, f32), np.full((heads, total_q), SENT, f32), np.full(nws + 64, SENT, f32)
    out = ops.flash_attention_paged_varlen(q, np.array(kp), np.array(vp), table, lens, cu, max_kv_len=PV.MAX_KV, causal=bool(causal), kv_splits=ks, return_lse=True,
                                           return_partials=True, kv_dtype=pool, k_scale=ksc, v_scale=vsc, out=y, lse_out=lse, workspace=ws)
    assert out[0] is y and out[1] is lse
    op, l2 = out[2]
    assert (op is None) == (S == 1)
    if S > 1:
        op, l2 = op.reshape(S, heads, total_q, hd), l2.reshape(S, heads, total_q)
        assert (ws[nws:] == SENT).all(), "the workspace past workspace_floats is untouched"
    else:
        assert (ws == SENT).all(), "S == 1 touches no float workspace"
    return y, lse, op, l2


_REF = {}


def _reference(cfg, mode, pool, causal, ks, n, L):
    """the existing paged entry of the pool type on the sequence (n, L) alone, in a page-16 pool that holds nothing else: batch 1,
    seq_q n, max_kv_len and kv_splits as in the packed call -> (y [n, heads, hd], lse [heads, n], O_part [S, heads, n, hd] or None,
    lse2_part [S, heads, n] or None), once"""
    key = (cfg, mode, pool, causal, ks, n, L)
    if key not in _REF:
        heads, _, hd = cfg
        kp, vp, ksc, vsc, table, lens = PV.typed_pool(cfg, ((n, L),), 16, pool)
        q = np.ascontiguousarray(PV.sequence(cfg, n, L)[0][None])
        kw = dict(max_kv_len=PV.MAX_KV, causal=bool(causal), layout="bshd", kv_splits=ks, return_lse=True, return_partials=True)
        tb, lb = table, lens

        def call(ops):
            if pool == "e4m3":
                return ops.flash_attention_paged_fp8(q, np.array(kp), np.array(vp), ksc, vsc, tb, lb, **kw)
            return ops.flash_attention_paged(q, np.array(kp), np.array(vp), tb, lb, kv_dtype=pool, **kw)
        y, lse, (op, l2) = _mode(mode, call)
        if op is not None:
            S = op.shape[0]
            op, l2 = op.reshape(S, heads, n, hd), l2.reshape(S, heads, n)
        _REF[key] = (y[0], lse[0], op, l2)
    return _REF[key]


def _check_sequences(got, cfg, mode, pool, causal, ks, pack, cu, what):
    """every sequence with n_b >= 1 against its yardstick, bit for bit -> how many were checked"""
    y, lse, op, l2 = got
    checked = 0
    for b, (n, L) in enumerate(pack):
        if n == 0:
            continue
        wy, wlse, wop, wl2 = _reference(cfg, mode, pool, causal, ks, n, L)
        rows = slice(int(cu[b]), int(cu[b]) + n)
        np.testing.assert_array_equal(y[rows].view(np.uint32), wy.view(np.uint32), err_msg=f"y of sequence {b} {(n, L)}: {what}")
        np.testing.assert_array_equal(lse[:, rows].view(np.uint32), wlse.view(np.uint32), err_msg=f"lse of sequence {b} {(n, L)}: {what}")
        assert (op is None) == (wop is None)
        if op is not None:
            assert op.shape[0] == wop.shape[0], "the splits that call has"
            np.testing.assert_array_equal(op[:, :, rows].view(np.uint32), wop.view(np.uint32), err_msg=f"O_part of sequence {b} {(n, L)}: {what}")
            np.testing.assert_array_equal(l2[:, :, rows].view(np.uint32), wl2.view(np.uint32), err_msg=f"lse2_part of sequence {b} {(n, L)}: {what}")
        checked += 1
    return checked


def _check_padding(got, cu, total_q, what):
    """rows outside [s_0, s_n) keep the sentinel in y, lse and the partials; the others hold no NaN and no sentinel"""
    y, lse, op, l2 = got
    pad = np.ones(total_q, bool)
    pad[int(cu[0]):int(cu[-1])] = False
    assert pad.sum() == total_q - (int(cu[-1]) - int(cu[0]))
    assert (y[pad] == SENT).all() and (lse[:, pad] == SENT).all(), what
    assert not np.isnan(y).any() and not np.isnan(lse).any() and not (y[~pad] == SENT).any() and not (lse[:, ~pad] == SENT).any(), what
    if op is not None:
        assert (op[:, :, pad] == SENT).all() and (l2[:, :, pad] == SENT).all(), what
        assert not np.isnan(op).any() and not np.isnan(l2).any() and not (op[:, :, ~pad] == SENT).any() and not (l2[:, :, ~pad] == SENT).any(), what


CASES = [(cfg, mode, pool) for cfg in PV.CONFIGS for mode in PV.MODES for pool in PV.pools_of(mode)]


@pytest.mark.parametrize("cfg,mode,pool", CASES, ids=[f"{PV.config_id(c)}-{m}-pool_{p or 'f32'}" for c, m, p in CASES])
def test_every_sequence_carries_the_bits_of_the_paged_entry_on_it_alone(gpu, cfg, mode, pool):
    """causal 0 / 1 x kv_splits 1 / 3 x page 16 / 64 x the pack at token 0 / 2: y, lse and the partials of every sequence with n_b >= 1,
    none skipped; the padding rows keep the sentinel; no NaN arrives although q's padding rows and the pool's unread parts are NaN; the
    first causal row of the last sequence is 0 / -inf"""
    want = sum(1 for n, _ in PV.PACK if n >= 1)
    for causal in PV.CAUSALS:
        for ks in PV.SPLITS:
            for page in PV.PAGES:
                for start in PV.CU0:
                    cu = PV.cu_of(PV.PACK, start)
                    q = PV.packed_q(cfg, PV.PACK, cu, PV.TOTAL_Q)
                    what = f"causal {causal} kv_splits {ks} page {page} cu[0] {start}"
                    got = _mode(mode, lambda ops: _packed(ops, cfg, q, PV.typed_pool(cfg, PV.PACK, page, pool), pool, cu, causal, ks))
                    assert _check_sequences(got, cfg, mode, pool, causal, ks, PV.PACK, cu, what) == want == 5
                    _check_padding(got, cu, PV.TOTAL_Q, what)
                    y, lse = got[:2]
                    first = int(cu[5])                                            # sequence (3, 2): query 0 sees key j <= 0 + 2 - 3
                    if causal:
                        assert (y[first] == 0).all() and np.isneginf(lse[:, first]).all() and np.isfinite(lse[:, first + 1:first + 3]).all(), what
                        assert int(np.isneginf(lse).sum()) == cfg[0], "no other row is empty"
                    else:
                        assert np.isfinite(lse[:, int(cu[0]):int(cu[-1])]).all(), what


@pytest.mark.parametrize("mode", PV.MODES)
def test_bits_do_not_depend_on_the_order_of_the_pack_on_n_seqs_or_on_total_q(gpu, mode):
    """the pack reversed and shuffled, idle slots added (n_seqs 6 -> 9), the capacity raised (total_q 64 -> 100, the pack behind 7
    padding tokens): every sequence still carries the bits of the same per-sequence call"""
    cfg, causal, ks = PV.CONFIGS[1], 1, 3
    pool = None if mode == "f32" else mode
    idle = ((0, 40), (0, 0), (0, 256))
    packs = (PV.PACK[::-1], tuple(PV.PACK[i] for i in (4, 0, 5, 2, 1, 3)), PV.PACK[:2] + idle[:1] + PV.PACK[2:] + idle[1:])
    for pack, total_q, start in ((packs[0], 64, 0), (packs[1], 64, 5), (packs[2], 64, 1), (packs[2], 100, 7), (PV.PACK, 59, 0)):
        cu = PV.cu_of(pack, start)
        q = PV.packed_q(cfg, pack, cu, total_q)
        for page in PV.PAGES:
            what = f"pack {pack} total_q {total_q} page {page}"
            got = _mode(mode, lambda ops: _packed(ops, cfg, q, PV.typed_pool(cfg, pack, page, pool), pool, cu, causal, ks))
            assert _check_sequences(got, cfg, mode, pool, causal, ks, pack, cu, what) == 5
            _check_padding(got, cu, total_q, what)


@pytest.mark.parametrize("mode,pool", (("f32", None), ("bf16", "bf16"), ("f16", "e4m3")))
def test_untrusted_device_values_give_the_bits_of_their_clamped_values(gpu, mode, pool):
    """a garbage cu_seqlens_q (negative, decreasing, beyond total_q), garbage kv_lens (negative, beyond max_kv_len) and garbage table
    entries (unused ones anything; used ones outside the pool) are ordinary defined inputs: the call returns the bits of the call on
    their clamped values, and those of the existing entry on each resulting sequence"""
    cfg, causal, ks, page = PV.CONFIGS[1], 1, 3, 16
    heads, kv_heads, hd = cfg
    pack = ((1, 130), (0, 77), (17, 256), (5, 200), (33, 97), (3, 0))                 # the lengths the garbage clamps to
    kp, vp, ksc, vsc, table, lens = PV.typed_pool(cfg, pack, page, pool)
    n_pages = kp.shape[0]
    q = np.random.default_rng(9).standard_normal((PV.TOTAL_Q, heads, hd)).astype(f32)
    bad_cu = np.array([-7, 1, -3, 18, 5, 56, 10 ** 9], np.int32)
    good_cu = PV.clamp_starts(bad_cu, PV.TOTAL_Q).astype(np.int32)
    assert good_cu.tolist() == [0, 1, 1, 18, 18, 56, 64]
    bad_lens = np.array([130, 77, 10 ** 9, 200, 97, -5], np.int32)
    assert np.clip(bad_lens, 0, PV.MAX_KV).tolist() == lens.tolist()
    bad_table, good_table = table.copy(), table.copy()
    for b, L in enumerate(lens):
        bad_table[b, (int(L) + page - 1) // page:] = (10 ** 9, -10 ** 9, 2 ** 31 - 1)[b % 3]          # never read
    bad_table[2, 3], good_table[2, 3] = -5, 0                                        # used entries: clamped into the pool
    bad_table[4, 1], good_table[4, 1] = n_pages + 9, n_pages - 1
    run = lambda t, l, c: _mode(mode, lambda ops: _packed(ops, cfg, q, (kp, vp, ksc, vsc, t, l), pool, c, causal, ks))
    got = run(bad_table, bad_lens, bad_cu)
    want = run(good_table, lens, good_cu)
    for a, b, name in zip(got, want, ("y", "lse", "O_part", "lse2_part")):
        np.testing.assert_array_equal(a, b, err_msg=name)
    assert not (got[0] == SENT).any(), "the clamped pack fills the capacity: no padding row"
    # the resulting sequences against the existing entry, each alone (the clamped table and lengths; the wrapper refuses the garbage)
    kw = dict(max_kv_len=PV.MAX_KV, causal=True, layout="bshd", kv_splits=ks, return_lse=True, return_partials=True)
    checked = 0
    for b in range(6):
        s, e = int(good_cu[b]), int(good_cu[b + 1])
        if e == s:
            continue
        qb, tb, lb = np.ascontiguousarray(q[None, s:e]), np.ascontiguousarray(good_table[b:b + 1]), np.ascontiguousarray(lens[b:b + 1])
        if pool == "e4m3":
            y, lse, (op, l2) = _mode(mode, lambda ops: ops.flash_attention_paged_fp8(qb, np.array(kp), np.array(vp), ksc, vsc, tb, lb, **kw))
        else:
            y, lse, (op, l2) = _mode(mode, lambda ops: ops.flash_attention_paged(qb, np.array(kp), np.array(vp), tb, lb, kv_dtype=pool, **kw))
        np.testing.assert_array_equal(got[0][s:e], y[0])
        np.testing.assert_array_equal(got[1][:, s:e], lse[0])
        np.testing.assert_array_equal(got[2][:, :, s:e], op.reshape(-1, heads, e - s, hd))
        np.testing.assert_array_equal(got[3][:, :, s:e], l2.reshape(-1, heads, e - s))
        checked += 1
    assert checked == 4
    assert (got[0][56:] == 0).all() and np.isneginf(got[1][:, 56:]).all(), "the sequence whose length clamps to 0: every row 0 / -inf"


@pytest.mark.parametrize("mode", PV.MODES)
def test_parity_against_float64(gpu, mode):
    """every sequence of the pack within the bounds of tests/test_flash_attention_splitkv_gpu.py (PG.y_bound, PG.lse_bound, unchanged) of
    the float64 reference on its own keys, over the fp32 pool; an empty row is exactly 0 / -inf"""
    cfg, ks = PV.CONFIGS[1], 3
    heads, kv_heads, hd = cfg
    s16 = None if mode == "f32" else mode
    cu = PV.cu_of(PV.PACK)
    q = PV.packed_q(cfg, PV.PACK, cu, PV.TOTAL_Q)
    for causal in PV.CAUSALS:
        y, lse, _, _ = _mode(mode, lambda ops: _packed(ops, cfg, q, PV.typed_pool(cfg, PV.PACK, 64, None), None, cu, causal, ks))
        for b, (n, L) in enumerate(PV.PACK):
            if n == 0:
                continue
            qs, k, v = (np.ascontiguousarray(a.transpose(1, 0, 2)[None]) for a in PV.sequence(cfg, n, L))      # BHSD, batch 1
            if s16:
                qs, k, v = (PG.round_s16(a, s16) for a in (qs, k, v))
            ref, ref_lse = PG.reference(qs, k, v, [L], causal)
            rows = slice(int(cu[b]), int(cu[b]) + n)
            gy, gl = y[rows].transpose(1, 0, 2)[None].astype(np.float64), lse[None, :, rows].astype(np.float64)
            none = np.isneginf(ref_lse)
            err, bound = float(np.abs(gy - ref).max()), PG.y_bound(ref, v, mode)
            lerr, lbound = float(np.abs(gl[~none] - ref_lse[~none]).max()), PG.lse_bound(ref_lse[~none])
            print(f"flash attention paged varlen {mode} causal {causal} sequence {(n, L)}: y max abs err {err:.3e}, bound {bound:.3e}; lse {lerr:.3e}, bound {lbound:.3e}")
            assert err <= bound and lerr <= lbound
            assert (gy[none] == 0).all() and np.isneginf(gl[none]).all() and int(none.sum()) == (heads if causal and (n, L) == (3, 2) else 0)


# ---- one captured graph is a mixed step: plan + append + attention ----
def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _dev_pool(bits, pool):
    """host pool (fp32 values, or uint16 bit patterns) -> the device tensor ops takes for it"""
    if pool is None:
        return _dev(bits)
    return _dev(bits.view(np.int16)).view(torch.bfloat16 if pool == "bf16" else torch.float16)


def _pool_bits(t, pool):
    return t.cpu().numpy() if pool is None else t.view(torch.int16).cpu().numpy().view(np.uint16)


class _Step:
    """the device buffers of one mixed step over capacity TOTAL_Q and 6 sequence slots"""

    def __init__(self, cfg, pool, n_pages, page, max_pages):
        heads, kv_heads, hd = cfg
        dt = torch.float32 if pool is None else torch.bfloat16 if pool == "bf16" else torch.float16
        self.cfg, self.pool = cfg, pool
        self.kp, self.vp = (torch.zeros(n_pages, page, kv_heads, hd, dtype=dt, device="cuda") for _ in range(2))
        self.table = torch.zeros(6, max_pages, dtype=torch.int32, device="cuda")
        self.lens = torch.zeros(6, dtype=torch.int32, device="cuda")
        self.cu = torch.zeros(7, dtype=torch.int32, device="cuda")
        self.q = torch.zeros(PV.TOTAL_Q, heads, hd, device="cuda")
        self.k_new, self.v_new = (torch.zeros(PV.TOTAL_Q, kv_heads, hd, device="cuda") for _ in range(2))
        self.y = torch.zeros(PV.TOTAL_Q, heads, hd, device="cuda")
        self.lse = torch.zeros(heads, PV.TOTAL_Q, device="cuda")
        from candle_birefnet_amd import ops
        _, _, nws, npl = ops.flash_attention_paged_varlen_plan(PV.TOTAL_Q, 6, PV.MAX_KV, heads, kv_heads, hd, 3)
        self.ws = torch.zeros(nws, device="cuda")
        self.plan = torch.zeros(npl, dtype=torch.int32, device="cuda")

    def load(self, pack, page):
        """the state BEFORE the step: the pool without each sequence's last n_b keys (NaN in their place), lengths len_b - n_b, and the
        step's inputs: those keys as packed new tokens, q, cu; outputs to the sentinel"""
        cfg, pool = self.cfg, self.pool
        kp, vp, table, lens = (a.copy() for a in PV.build_pool(cfg, pack, page))
        cu = PV.cu_of(pack)
        k_new, v_new = (np.full((PV.TOTAL_Q, cfg[1], cfg[2]), np.nan, f32) for _ in range(2))
        for b, (n, L) in enumerate(pack):
            _, k, v = PV.sequence(cfg, n, L)
            k_new[cu[b]:cu[b] + n], v_new[cu[b]:cu[b] + n] = k[L - n:], v[L - n:]
            for pos in range(L - n, L):
                kp[table[b, pos // page], pos % page] = np.nan
                vp[table[b, pos // page], pos % page] = np.nan
        if pool is not None:
            kp, vp = KC.to_bits(kp, pool), KC.to_bits(vp, pool)
        for dst, src in ((self.kp, _dev_pool(kp, pool)), (self.vp, _dev_pool(vp, pool)), (self.table, _dev(table)), (self.lens, _dev(lens - np.array([n for n, _ in pack], np.int32))),
                         (self.cu, _dev(cu)), (self.q, _dev(PV.packed_q(cfg, pack, cu, PV.TOTAL_Q))), (self.k_new, _dev(k_new)), (self.v_new, _dev(v_new))):
            dst.copy_(src)
        for t in (self.y, self.lse, self.ws):
            t.fill_(float(SENT))
        self.plan.fill_(-1)

    def step(self, ops):
        ops.kv_cache_append_varlen(self.k_new, self.v_new, self.cu, self.kp, self.vp, self.table, self.lens, kv_dtype=self.pool, update_lens=True, plan_workspace=self.plan)
        ops.flash_attention_paged_varlen(self.q, self.kp, self.vp, self.table, self.lens, self.cu, max_kv_len=PV.MAX_KV, causal=True, kv_splits=3, return_lse=True,
                                         kv_dtype=self.pool, out=self.y, lse_out=self.lse, workspace=self.ws, plan_workspace=self.plan)

    def results(self):
        torch.cuda.synchronize()
        return self.y.cpu().numpy(), self.lse.cpu().numpy(), self.lens.cpu().numpy(), _pool_bits(self.kp, self.pool), _pool_bits(self.vp, self.pool), self.ws.cpu().numpy()


# a step appends before it attends, so every sequence needs len_b >= n_b: the pack with its last sequence at (3, 3)
GRAPH_PACK = PV.PACK[:5] + ((3, 3),)
GRAPH_DECODE = tuple((1, L) for _, L in GRAPH_PACK)


@pytest.mark.parametrize("mode,pool", (("f32", None), ("bf16", "bf16")))
def test_one_graph_is_a_mixed_step_and_an_all_decode_step(gpu, mode, pool):
    """plan + append + attention captured once on a side stream; replayed for two contents of cu_seqlens_q / kv_lens / table / pool: the
    mixed pack, then six decode sequences.  Each replay gives the bits of the eager calls on a second set of buffers, the pool and the
    lengths of the finished step, and (y, lse) of the per-sequence yardstick"""
    from candle_birefnet_amd import ops
    cfg, page = PV.CONFIGS[1], 16
    n_pages, _, _, _ = PV.build_pool(cfg, GRAPH_PACK, page)[0].shape
    max_pages = PV.build_pool(cfg, GRAPH_PACK, page)[2].shape[1]
    assert PV.build_pool(cfg, GRAPH_DECODE, page)[0].shape[0] == n_pages
    graph_side, eager_side = (_Step(cfg, pool, n_pages, page, max_pages) for _ in range(2))
    # the yardsticks first: _reference sets the compute mode and sets it back to f32
    yardstick = {(n, L): _reference(cfg, mode, pool, 1, 3, n, L)[:2] for n, L in GRAPH_PACK + GRAPH_DECODE if n}
    ops.set_compute(mode)
    try:
        graph_side.load(GRAPH_PACK, page)
        graph_side.step(ops)                                     # warm-up outside the capture
        torch.cuda.synchronize()
        side = torch.cuda.Stream()
        graph = torch.cuda.CUDAGraph()
        graph_side.load(GRAPH_PACK, page)
        torch.cuda.synchronize()
        with torch.cuda.graph(graph, stream=side):
            graph_side.step(ops)
        seen = []
        for pack in (GRAPH_PACK, GRAPH_DECODE, GRAPH_PACK):
            graph_side.load(pack, page)
            eager_side.load(pack, page)
            eager_side.step(ops)
            want = eager_side.results()
            torch.cuda.synchronize()
            graph.replay()
            got = graph_side.results()
            for a, b, name in zip(got, want, ("y", "lse", "kv_lens", "k_pages", "v_pages", "workspace")):
                np.testing.assert_array_equal(a, b, err_msg=f"{name} of the replay against the eager calls, pack {pack}")
            assert got[2].tolist() == [L for _, L in pack]
            full = PV.typed_pool(cfg, pack, page, pool)
            same = lambda a, b: np.array_equal(a, b) if pool is not None else np.array_equal(a.view(np.uint32), b.view(np.uint32))
            assert same(got[3], full[0]) and same(got[4], full[1]), "the pool of the finished step, NaN rows included"
            cu = PV.cu_of(pack)
            y, lse = got[:2]
            for b, (n, L) in enumerate(pack):
                if n:
                    wy, wlse = yardstick[(n, L)]
                    np.testing.assert_array_equal(y[cu[b]:cu[b] + n], wy, err_msg=f"y of sequence {(n, L)} against the paged entry")
                    np.testing.assert_array_equal(lse[:, cu[b]:cu[b] + n], wlse)
            assert (y[cu[-1]:] == SENT).all() and (lse[:, cu[-1]:] == SENT).all()
            seen.append(y.copy())
        assert not np.array_equal(seen[0], seen[1]) and np.array_equal(seen[0], seen[2])
    finally:
        ops.set_compute("f32")
