"""brn_kv_cache_append on the GPU, alone and in front of brn_flash_attention_paged_kv_forward.

Pools start filled with a sentinel bit pattern (a NaN payload) and are compared on their raw bits: every row the rule of
kv_cache_cases.append_rule names holds the suite's own rounding (round_s16) of its token, a NaN token is a NaN, and every other row still
holds the sentinel.  Out-of-range device values are written into pools that are the middle of a larger buffer, so a missing clamp is a
failed comparison and never an access outside an allocation.  Append followed by attention over the 16-bit pool gives, bit for bit,
brn_flash_attention_paged_forward in the pool's compute mode on an fp32 pool of the UNROUNDED keys; captured into one graph, the pair
is a whole decode step."""
import numpy as np
import pytest
import torch

import flash_attention_gqa_cases as GQ
import flash_attention_paged_cases as PG
import kv_cache_cases as KC

pytestmark = pytest.mark.gpu

TORCH_DT = {"f32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16}
INT_DT = {"f32": (torch.int32, np.int32), "bf16": (torch.int16, np.int16), "f16": (torch.int16, np.int16)}


def _mode(mode, fn):
    from candle_birefnet_amd import ops
    ops.set_compute(mode)
    try:
        return fn(ops)
    finally:
        ops.set_compute("f32")


def _to_device(bits, kv):
    """bit patterns (uint16 / uint32) -> a device tensor of the pool's dtype holding them"""
    return torch.from_numpy(np.array(bits).view(INT_DT[kv][1])).view(TORCH_DT[kv]).cuda()


def _bits(t, kv):
    """a device tensor of the pool's dtype -> its bit patterns"""
    return t.view(INT_DT[kv][0]).cpu().numpy().view(KC.BITS[kv])


def _check_pool(got, want, nan, kv, what):
    """raw bits equal wherever the expected element is not a stored NaN token; there: is NaN"""
    np.testing.assert_array_equal(got[~nan], want[~nan], err_msg=what)
    assert np.isnan(KC.widen(got, kv)[nan]).all(), f"{what}: a NaN token is not a NaN in the pool"


@pytest.mark.parametrize("kv", KC.KV_TYPES)
@pytest.mark.parametrize("hd", KC.HEAD_DIMS)
@pytest.mark.parametrize("name", list(KC.APPEND_CASES))
def test_rows_lengths_and_everything_else(gpu, name, hd, kv):
    """every case, pool type and head_dim (both layouts where the case names two): the pool's bits after the call are the rule's on a
    sentinel pool, kv_lens_out is the rule's and kv_lens is unchanged.  The pool is the middle of a buffer with MARGIN sentinel pages on
    each side, wider than any page number a table holds: the margins keep the sentinel"""
    from candle_birefnet_amd import ops
    c = KC.APPEND_CASES[name]
    k, v = KC.new_tokens(name, hd)
    kw, vw, lens_want, knan, vnan = KC.expected_append(name, hd, kv)
    n_pages = KC.n_pages_of(c)
    table = torch.from_numpy(np.array(KC.table_of(name))).cuda()
    assert not c["bad"] or (int(table.min()) < 0 and int(table.max()) >= n_pages and KC.MARGIN >= max(-int(table.min()), int(table.max()) - n_pages + 1))
    for layout in c["layouts"]:
        big = [_to_device(KC.sentinel_pool(c, hd, kv, n_pages + 2 * KC.MARGIN), kv) for _ in range(2)]
        kp, vp = (b[KC.MARGIN:KC.MARGIN + n_pages] for b in big)
        assert kp.is_contiguous() and kp.data_ptr() % 16 == 0
        lens = torch.tensor(c["lens"], dtype=torch.int32, device="cuda")
        kn, vn = (torch.from_numpy(PG.in_layout(a.transpose(0, 2, 1, 3), layout) if layout == "bhsd" else np.array(a)).cuda() for a in (k, v))
        out = ops.kv_cache_append(kn, vn, kp, vp, table, lens, kv_dtype=None if kv == "f32" else kv, layout=layout, update_lens=False)
        torch.cuda.synchronize()
        _check_pool(_bits(kp, kv), kw, knan, kv, f"k_pages {layout}")
        _check_pool(_bits(vp, kv), vw, vnan, kv, f"v_pages {layout}")
        np.testing.assert_array_equal(out.cpu().numpy(), lens_want)
        np.testing.assert_array_equal(lens.cpu().numpy(), np.asarray(c["lens"], np.int32))
        for b in big:
            edge = _bits(b, kv)
            assert (edge[:KC.MARGIN] == KC.SENTINEL[kv]).all() and (edge[KC.MARGIN + n_pages:] == KC.SENTINEL[kv]).all(), "a margin was written"
    written = sum(len(KC.written_positions(c, b)) for b in range(c["batch"]))
    assert int((kw != KC.SENTINEL[kv]).any(axis=(2, 3)).sum()) == written


def test_what_the_cast_makes_of_ties_zeros_subnormals_overflow_and_nan(gpu):
    """the special values among the tokens, read back from where the rule puts them: ties go to even in both types, -0 keeps its sign, an
    f16 subnormal is kept, half the smallest f16 subnormal is 0, 70000 is +inf in f16 and finite in bf16, a NaN stays a NaN"""
    from candle_birefnet_amd import ops
    name, hd = "straddle", 32
    c = KC.APPEND_CASES[name]
    k, _ = KC.new_tokens(name, hd)
    n = KC.SPECIALS.size
    assert np.array_equal(k.reshape(-1)[:n].view(np.uint32), KC.SPECIALS.view(np.uint32)) and n <= hd
    want = {"bf16": [0x3F80, 0x3F82, 0xBF80, 0x3F80, 0x3F80, 0xBF80, 0x0000, 0x8000], "f16": [0x3C04, 0x3C0C, 0xBC04, 0x3C00, 0x3C02, 0xBC02, 0x0000, 0x8000]}
    L = c["lens"][0]
    table = KC.table_of(name)
    for kv in ("bf16", "f16"):
        kp, vp = (_to_device(KC.sentinel_pool(c, hd, kv), kv) for _ in range(2))
        kn, vn = (torch.from_numpy(np.array(a)).cuda() for a in KC.new_tokens(name, hd))
        ops.kv_cache_append(kn, vn, kp, vp, torch.from_numpy(np.array(table)).cuda(), torch.tensor(c["lens"], dtype=torch.int32, device="cuda"), kv_dtype=kv, update_lens=None)
        torch.cuda.synchronize()
        row = _bits(kp, kv)[table[0, L // c["page"]], L % c["page"], 0]           # token 0, head 0: the specials
        assert row[:8].tolist() == want[kv], (kv, [hex(x) for x in row[:8]])
        np.testing.assert_array_equal(row[:15], KC.to_bits(KC.SPECIALS[:15], kv))
        assert np.isnan(KC.widen(row[15:16], kv)).all() and row[16] == KC.to_bits(KC.SPECIALS[16:17], kv)[0]
        f = KC.widen(row, kv)
        if kv == "f16":
            assert 0 < row[8] < 0x0400 and row[10] == 0 and np.isposinf(f[11]) and np.isneginf(f[12]) and f[13] == 65504.0 and np.isposinf(f[14]) and np.isposinf(f[16])
        else:
            assert f[11] == 70144.0 and np.isfinite(f[16])


@pytest.mark.parametrize("kv", KC.KV_TYPES)
def test_lengths_separate_in_place_and_null(gpu, kv):
    """kv_lens_out separate from kv_lens (kv_lens unchanged), equal to kv_lens (updated in place, also across two calls in a row), and
    NULL (kv_lens unchanged): the pool's bits are the same in all three"""
    from candle_birefnet_amd import ops
    name, hd = "dropped", 32
    c = KC.APPEND_CASES[name]
    kw, vw, lens_want, knan, vnan = KC.expected_append(name, hd, kv)
    table = torch.from_numpy(np.array(KC.table_of(name))).cuda()
    kn, vn = (torch.from_numpy(np.array(a)).cuda() for a in KC.new_tokens(name, hd))
    kvd = None if kv == "f32" else kv
    for update in (False, True, None):
        kp, vp = (_to_device(KC.sentinel_pool(c, hd, kv), kv) for _ in range(2))
        lens = torch.tensor(c["lens"], dtype=torch.int32, device="cuda")
        out = ops.kv_cache_append(kn, vn, kp, vp, table, lens, kv_dtype=kvd, update_lens=update)
        torch.cuda.synchronize()
        _check_pool(_bits(kp, kv), kw, knan, kv, f"k_pages update_lens={update}")
        _check_pool(_bits(vp, kv), vw, vnan, kv, f"v_pages update_lens={update}")
        if update is None:
            assert out is None
        else:
            np.testing.assert_array_equal(out.cpu().numpy(), lens_want)
        assert (out is lens) == (update is True)
        np.testing.assert_array_equal(lens.cpu().numpy(), lens_want if update else np.asarray(c["lens"], np.int32))
        if update:
            # the lengths now stand at cap: a second step drops every token and leaves pool and lengths alone
            ops.kv_cache_append(kn, vn, kp, vp, table, lens, kv_dtype=kvd, update_lens=True)
            torch.cuda.synchronize()
            _check_pool(_bits(kp, kv), kw, knan, kv, "k_pages after a step at cap")
            assert lens.cpu().numpy().tolist() == [KC.cap_of(c)]


def test_host_arrays_carry_the_bits_of_device_tensors(gpu):
    """BRN_MEM_HOST (the pool staged up and copied back whole): numpy pools of bit patterns, written in place"""
    from candle_birefnet_amd import ops
    name, hd = "three_pages", 32
    c = KC.APPEND_CASES[name]
    k, v = KC.new_tokens(name, hd)
    for kv in KC.KV_TYPES:
        kw, vw, lens_want, knan, vnan = KC.expected_append(name, hd, kv)
        kp, vp = KC.sentinel_pool(c, hd, kv), KC.sentinel_pool(c, hd, kv)
        pools = (kp.view(np.float32), vp.view(np.float32)) if kv == "f32" else (kp, vp)
        lens = np.array(c["lens"], np.int32)
        out = ops.kv_cache_append(k, v, *pools, np.array(KC.table_of(name)), lens, kv_dtype=None if kv == "f32" else kv)
        assert out is lens
        _check_pool(kp, kw, knan, kv, "host k_pages")
        _check_pool(vp, vw, vnan, kv, "host v_pages")
        np.testing.assert_array_equal(lens, lens_want)


# ---- append, then attend ----
CASE128 = ((3, 1, 5, 1, 128), 64, (1000, 512, 3), "std1", 1, 4)      # the D 128 row of the paged cases with a sequence that starts empty
STEP = 3


class _Step:
    """A decode state on the device for a paged case: q (BSHD), a 16-bit pool that holds the first len_b - 3 keys of every sequence
    (rounded; every other element the sentinel NaN), the case's table, lengths at len_b - 3, the last 3 unrounded keys of every
    sequence as tokens [batch, 3, kv_heads, hd], outputs and workspace allocated once"""

    def __init__(self, case, kv):
        import candle_birefnet_amd as cb
        (batch, seq_q, heads, kv_heads, hd), page, lens, kind, causal, ks = case
        assert min(lens) >= STEP
        self.case, self.kv = case, kv
        q, k, v = PG.logical_inputs(case)
        kp, vp, table, _ = PG.build_pool(case)
        start = np.asarray(lens, np.int32) - STEP
        keep = np.zeros(kp.shape[:2], bool)
        for b in range(batch):
            pos = np.arange(start[b])
            keep[table[b, pos // page], pos % page] = True
        pools = []
        for a in (kp, vp):
            bits = KC.to_bits(a, kv)
            bits[~keep] = KC.SENTINEL[kv]
            pools.append(_to_device(bits, kv))
        self.kp, self.vp = pools
        self.tokens = tuple(torch.from_numpy(np.stack([a[b, :, lens[b] - STEP:lens[b]].transpose(1, 0, 2) for b in range(batch)]).astype(np.float32)).cuda() for a in (k, v))
        self.q = torch.from_numpy(np.array(PG.in_layout(q, "bshd"))).cuda()
        self.table = torch.from_numpy(np.array(table)).cuda()
        self.lens = torch.from_numpy(start).cuda()
        self.ints = (batch, seq_q, PG.max_len(case), heads, kv_heads, hd, kp.shape[0], page, table.shape[1], 0, causal, PG.kind_scale(kind) or 0.0, ks)
        self.geo = (batch, kv_heads, hd, kp.shape[0], page, table.shape[1])
        _, _, self.need = cb.ops.flash_attention_splitkv_plan(batch, seq_q, PG.max_len(case), heads, kv_heads, hd, ks)
        self.ws = torch.zeros(max(self.need, 4), dtype=torch.float32, device="cuda")
        self.y = torch.full(self.q.shape, float("nan"), dtype=torch.float32, device="cuda")
        self.lse = torch.full((batch, heads, seq_q), float("nan"), dtype=torch.float32, device="cuda")

    def append(self, k_new, v_new, stream=None):
        """raw brn_kv_cache_append of k_new, v_new [batch, seq_new, kv_heads, hd] (contiguous device tensors), lengths in place"""
        import candle_birefnet_amd as cb
        batch, kv_heads, hd, n_pages, page, max_pages = self.geo
        st, msg = KC.raw_append(cb._ffi.lib, k_new.data_ptr(), v_new.data_ptr(), batch, int(k_new.shape[1]), kv_heads, hd, 0, self.kp.data_ptr(), self.vp.data_ptr(),
                                KC.KV_CODE[self.kv], self.table.data_ptr(), self.lens.data_ptr(), self.lens.data_ptr(), n_pages, page, max_pages, 1,
                                stream if stream is not None else torch.cuda.current_stream().cuda_stream)
        assert st == 0, msg

    def attend(self, stream=None):
        import candle_birefnet_amd as cb
        st, msg = KC.raw_attend(cb._ffi.lib, self.q.data_ptr(), self.kp.data_ptr(), self.vp.data_ptr(), KC.KV_CODE[self.kv], self.table.data_ptr(), self.lens.data_ptr(),
                                *self.ints, self.y.data_ptr(), self.lse.data_ptr(), self.ws.data_ptr() if self.need else None, self.need, 1,
                                stream if stream is not None else torch.cuda.current_stream().cuda_stream)
        assert st == 0, msg

    def results(self):
        torch.cuda.synchronize()
        return GQ.to_bhsd(self.y.cpu().numpy(), "bshd"), self.lse.cpu().numpy(), self.lens.cpu().numpy()


@pytest.mark.parametrize("kv", ("bf16", "f16"))
@pytest.mark.parametrize("case,calls", ((PG.FIRST, 3), (PG.FIRST, 1), (CASE128, 1), (CASE128, 3)), ids=("first-3x1", "first-1x3", "d128-1x3", "d128-3x1"))
def test_append_then_attend_is_the_fp32_entry_on_the_unrounded_keys(gpu, case, calls, kv):
    """the pool holds len_b - 3 keys of each sequence; the last 3 arrive as fp32 tokens, in three calls of seq_new 1 or one call of 3;
    attention in mode E over the E pool then carries the bits of brn_flash_attention_paged_forward in mode E on the fp32 pool of the
    unrounded keys.  Before the append the result differs (the keys matter)"""
    _, _, lens, kind, causal, ks = case
    st = _Step(case, kv)

    def run(ops):
        st.attend()
        before = st.results()[0].copy()
        tk, tv = st.tokens
        for i in range(0, STEP, STEP // calls):
            st.append(tk[:, i:i + STEP // calls].contiguous(), tv[:, i:i + STEP // calls].contiguous())
        st.attend()
        return before
    before = _mode(kv, run)
    y, lse, lens_now = st.results()
    np.testing.assert_array_equal(lens_now, np.asarray(lens, np.int32))
    q = PG.logical_inputs(case)[0]
    want_y, want_lse = _mode(kv, lambda ops: ops.flash_attention_paged(q, *PG.build_pool(case), max_kv_len=PG.max_len(case), causal=bool(causal),
                                                                       scale=PG.kind_scale(kind), layout="bhsd", kv_splits=ks, return_lse=True))
    np.testing.assert_array_equal(y, want_y)
    np.testing.assert_array_equal(lse, want_lse)
    assert not np.isnan(y).any() and not np.array_equal(before, y)


@pytest.mark.parametrize("kv", ("bf16", "f16"))
def test_one_graph_is_a_decode_step(gpu, kv):
    """On a side stream, brn_kv_cache_append (one token per sequence, lengths in place) followed by the 16-bit paged attention is
    captured into one graph: one branch.  Three replays, each after new q / k_new / v_new were copied into the captured input tensors,
    give the y, lse and lengths of the eager pair of calls on a second pool kept in step"""
    case = PG.FIRST
    lens = case[2]
    graph_side, eager_side = _Step(case, kv), _Step(case, kv)
    q, k, v = PG.logical_inputs(case)
    batch = case[0][0]
    k_in, v_in = (torch.zeros_like(t[:, :1]).contiguous() for t in graph_side.tokens)

    def body(ops):
        eager_side.append(k_in, v_in)                           # warm: the library and its kernels are loaded before the capture
        eager_side.attend()
        torch.cuda.synchronize()
        fresh = _Step(case, kv)                                 # (the warm-up moved the eager side: start it again)
        eager_side.kp, eager_side.vp, eager_side.lens = fresh.kp, fresh.vp, fresh.lens
        side = torch.cuda.Stream()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            s = torch.cuda.current_stream().cuda_stream
            graph_side.append(k_in, v_in, stream=s)
            graph_side.attend(stream=s)
        seen = []
        for step in range(STEP):
            tk, tv = (t[:, step:step + 1].contiguous() for t in graph_side.tokens)
            qn = torch.from_numpy(PG.in_layout(np.roll(q, step, axis=1), "bshd")).cuda()      # a new q each step: the heads rotate
            for dst, src in ((k_in, tk), (v_in, tv), (graph_side.q, qn), (eager_side.q, qn)):
                dst.copy_(src)
            eager_side.append(tk, tv)
            eager_side.attend()
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
        np.testing.assert_array_equal(_bits(graph_side.kp, kv), _bits(eager_side.kp, kv))
        np.testing.assert_array_equal(_bits(graph_side.vp, kv), _bits(eager_side.vp, kv))
    _mode(kv, body)


def test_refusals_on_the_gpu_leave_the_pool_alone(gpu):
    """a refused append writes nothing: the pool keeps its sentinel and the lengths their values, and the valid call that follows works"""
    import candle_birefnet_amd as cb
    from candle_birefnet_amd import ops
    name, hd, kv = "straddle", 32, "bf16"
    c = KC.APPEND_CASES[name]
    kw, vw, lens_want, knan, vnan = KC.expected_append(name, hd, kv)
    kp, vp = (_to_device(KC.sentinel_pool(c, hd, kv), kv) for _ in range(2))
    kn, vn = (torch.from_numpy(np.array(a)).cuda() for a in KC.new_tokens(name, hd))
    table = torch.from_numpy(np.array(KC.table_of(name))).cuda()
    lens = torch.tensor(c["lens"], dtype=torch.int32, device="cuda")
    ok = (kn.data_ptr(), vn.data_ptr(), c["batch"], c["seq_new"], c["kv_heads"], hd, 0, kp.data_ptr(), vp.data_ptr(), 1, table.data_ptr(), lens.data_ptr(), lens.data_ptr(),
          KC.n_pages_of(c), c["page"], c["max_pages"], 1)
    sub = lambda i, v: ok[:i] + (v,) + ok[i + 1:]
    for args, word in ((sub(9, 3), "kv_type must be"), (sub(3, 0), "1 <= seq_new <= 65536"), (sub(8, kp.data_ptr()), "k_pages and v_pages must not overlap"),
                       (sub(0, kn.data_ptr() + 4), "16-byte aligned"), (sub(12, lens.data_ptr() + 2), "kv_lens_out must not overlap kv_lens"), (sub(0, kp.data_ptr()), "k_new must not overlap the pool")):
        st, msg = KC.raw_append(cb._ffi.lib, *args)
        assert st == 1 and msg.startswith("kv cache append: ") and word in msg, (st, msg)
    torch.cuda.synchronize()
    assert (_bits(kp, kv) == KC.SENTINEL[kv]).all() and (_bits(vp, kv) == KC.SENTINEL[kv]).all() and lens.cpu().numpy().tolist() == list(c["lens"])
    ops.kv_cache_append(kn, vn, kp, vp, table, lens, kv_dtype=kv)
    torch.cuda.synchronize()
    _check_pool(_bits(kp, kv), kw, knan, kv, "k_pages after the refusals")
    np.testing.assert_array_equal(lens.cpu().numpy(), lens_want)
