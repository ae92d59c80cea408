"""brn_rope_forward, brn_kv_cache_append_rope and brn_kv_cache_append_rope_fp8 on the GPU.

Everything is compared on raw bits with the numpy statement of the rule (rope_cases.rope_rule: two rounded fp32 products, one rounded
sum); where the rule's value is a NaN the device's must be a NaN.  Outputs are the middle of larger sentinel-filled buffers whose
margins must stay untouched, positions and lengths outside their range meet the clamps, and the fused appends are compared both with
the rule (through kv_cache_cases.append_rule / kv_fp8_cases.quant) and with the two-call form rope -> append.  One captured graph is a
whole rotary decode step."""
import numpy as np
import pytest
import torch

import flash_attention_gqa_cases as GQ
import flash_attention_paged_cases as PG
import kv_cache_cases as KC
import kv_fp8_cases as F8
import rope_cases as RC

pytestmark = pytest.mark.gpu

TORCH_DT = {"f32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16}
INT_DT = {"f32": (torch.int32, np.int32), "bf16": (torch.int16, np.int16), "f16": (torch.int16, np.int16)}
X_SENTINEL = 0x7FC00AB5            # fills every output before a call
MARGIN = 64                        # floats each side of y


def _dev(a):
    return torch.from_numpy(np.array(a)).cuda()


def _pool_to_device(bits, kv):
    return torch.from_numpy(np.array(bits).view(INT_DT[kv][1])).view(TORCH_DT[kv]).cuda()


def _bits(t, kv):
    return t.view(INT_DT[kv][0]).cpu().numpy().view(KC.BITS[kv])


def _check_pool(got, want, nan, kv, what):
    np.testing.assert_array_equal(got[~nan], want[~nan], err_msg=what)
    assert np.isnan(KC.widen(got, kv)[nan]).all(), f"{what}: a NaN token is not a NaN in the pool"


def _in_layout(a, layout):
    """a BSHD array -> contiguous in `layout`"""
    return np.ascontiguousarray(a.transpose(0, 2, 1, 3)) if layout == "bhsd" else np.ascontiguousarray(a)


def _tables(rd, n_pos=RC.N_POS):
    return tuple(_dev(a) for a in RC.table(rd, n_pos))


@pytest.mark.parametrize("style,hd,rd", RC.COMBOS, ids=RC.COMBO_IDS)
def test_forward_carries_the_bits_of_the_rule(gpu, style, hd, rd):
    """every style, rot_dim, head_dim and layout; positions NULL, in range, negative (clamped to 0), past the table (clamped to the last
    row) and at the int32 extremes; the tail d >= rot_dim bit-identical, NaN payload included.  y is the middle of a sentinel-filled
    buffer whose margins stay untouched; in place (y == x) gives the same bits"""
    from candle_birefnet_amd import ops
    cos, sin = RC.table(rd)
    dcos, dsin = _tables(rd)
    for name, (layouts, position_sets) in RC.FORWARD_CASES.items():
        c = KC.APPEND_CASES[name]
        x = RC.forward_input(name, hd)
        for positions in position_sets:
            pos = None if positions == "none" else positions
            want = RC.rope_rule(x, cos, sin, RC.table_rows(pos, c["batch"], c["seq_new"], RC.N_POS), style)
            dpos = None if pos is None else torch.tensor(pos, dtype=torch.int32, device="cuda")
            for layout in layouts:
                what = f"{name} {layout} positions {positions}"
                xl = _in_layout(x, layout)
                dx = _dev(xl)
                big = torch.from_numpy(np.full(x.size + 2 * MARGIN, X_SENTINEL, np.uint32).view(np.float32)).cuda()
                y = big[MARGIN:MARGIN + x.size].view(xl.shape)
                assert y.data_ptr() % 16 == 0
                out = ops.rope(dx, dcos, dsin, positions=dpos, rot_dim=rd, style=style, layout=layout, out=y)
                torch.cuda.synchronize()
                assert out is y
                got = y.cpu().numpy()
                wl = _in_layout(want, layout)
                RC.assert_bits(got, wl, what)
                np.testing.assert_array_equal(got[..., rd:].view(np.uint32), xl[..., rd:].view(np.uint32), err_msg=f"{what}: the tail")
                edge = big.cpu().numpy().view(np.uint32)
                assert (edge[:MARGIN] == X_SENTINEL).all() and (edge[MARGIN + x.size:] == X_SENTINEL).all(), f"{what}: a margin was written"
                np.testing.assert_array_equal(dx.cpu().numpy().view(np.uint32), xl.view(np.uint32), err_msg=f"{what}: x was written")
                # a new array, and in place
                fresh = ops.rope(dx, dcos, dsin, positions=dpos, style=style, layout=layout)
                same = ops.rope(dx, dcos, dsin, positions=dpos, style=style, layout=layout, out=dx)
                torch.cuda.synchronize()
                assert same is dx and fresh is not dx
                np.testing.assert_array_equal(fresh.cpu().numpy().view(np.uint32), got.view(np.uint32), err_msg=f"{what}: a new output")
                np.testing.assert_array_equal(dx.cpu().numpy().view(np.uint32), got.view(np.uint32), err_msg=f"{what}: in place")
            if rd < hd:
                assert want.reshape(-1).view(np.uint32)[-1] == RC.NAN_PAYLOAD
    # the rotation did something, and the position sets differ
    x = RC.forward_input("clamped_pages", hd)
    a, b = (RC.rope_rule(x, cos, sin, RC.table_rows(p, 2, 20, RC.N_POS), style) for p in ((3, 20), (30, 1000)))
    assert not np.array_equal(a, b, equal_nan=True) and not np.array_equal(a[..., :rd], x[..., :rd], equal_nan=True)


def test_host_arrays_carry_the_bits_of_device_tensors(gpu):
    """BRN_MEM_HOST: numpy in, numpy out, also in place"""
    from candle_birefnet_amd import ops
    name, hd, rd = "clamped_pages", 64, 32
    x = RC.forward_input(name, hd)
    cos, sin = RC.table(rd)
    for style in RC.STYLES:
        want = RC.rope_rule(x, cos, sin, RC.table_rows((3, 20), 2, 20, RC.N_POS), style)
        got = ops.rope(x, cos, sin, positions=np.array([3, 20], np.int32), style=style)
        RC.assert_bits(got, want, style)
        xin = np.array(x)
        assert ops.rope(xin, cos, sin, positions=[3, 20], style=style, out=xin) is xin
        RC.assert_bits(xin, want, f"{style} in place")


def _append_inputs(name, hd, layout, k, v):
    return tuple(_dev(PG.in_layout(a.transpose(0, 2, 1, 3), layout) if layout == "bhsd" else a) for a in (k, v))


@pytest.mark.parametrize("kv", KC.KV_TYPES)
@pytest.mark.parametrize("hd", KC.HEAD_DIMS)
@pytest.mark.parametrize("name", list(KC.APPEND_CASES))
def test_append_rope_rows_lengths_and_everything_else(gpu, name, hd, kv):
    """every append case, pool type and head_dim, both styles at every rot_dim (both layouts where the case names two): the pool's bits
    are KC.append_rule's on the rule-rotated K and the unrotated V, on a sentinel pool between MARGIN sentinel pages; kv_lens_out is the
    rule's and kv_lens is unchanged.  Separately the pool equals the bits of the two-call form: ops.rope on k_new at positions = kv_lens,
    then ops.kv_cache_append of the result"""
    from candle_birefnet_amd import ops
    c = KC.APPEND_CASES[name]
    k, v = KC.new_tokens(name, hd)
    _, vw, lens_want, _, vnan = KC.expected_append(name, hd, kv)
    n_pages = KC.n_pages_of(c)
    table_np, lens_np = KC.table_of(name), np.asarray(c["lens"], np.int32)
    table = _dev(table_np)
    kvd = None if kv == "f32" else kv
    none = np.zeros(vw.shape, bool)
    for style in RC.STYLES:
        for rd in RC.rot_dims(hd):
            kr = RC.rotated_k(name, k, rd, style)
            kw = KC.append_rule(KC.to_bits(kr, kv), KC.sentinel_pool(c, hd, kv), table_np, lens_np)[0]
            knan = KC.append_rule(np.isnan(kr), none, table_np, lens_np)[0]
            dcos, dsin = _tables(rd)
            for layout in c["layouts"]:
                what = f"{style} rot_dim {rd} {layout}"
                big = [_pool_to_device(KC.sentinel_pool(c, hd, kv, n_pages + 2 * KC.MARGIN), kv) for _ in range(2)]
                kp, vp = (b[KC.MARGIN:KC.MARGIN + n_pages] for b in big)
                lens = torch.tensor(c["lens"], dtype=torch.int32, device="cuda")
                kn, vn = _append_inputs(name, hd, layout, k, v)
                out = ops.kv_cache_append_rope(kn, vn, dcos, dsin, kp, vp, table, lens, kv_dtype=kvd, style=style, layout=layout, update_lens=False)
                torch.cuda.synchronize()
                _check_pool(_bits(kp, kv), kw, knan, kv, f"k_pages {what}")
                _check_pool(_bits(vp, kv), vw, vnan, kv, f"v_pages {what}")
                np.testing.assert_array_equal(out.cpu().numpy(), lens_want)
                np.testing.assert_array_equal(lens.cpu().numpy(), lens_np)
                for b in big:
                    edge = _bits(b, kv)
                    assert (edge[:KC.MARGIN] == KC.SENTINEL[kv]).all() and (edge[KC.MARGIN + n_pages:] == KC.SENTINEL[kv]).all(), f"{what}: a margin was written"
                # the two-call form on pools of its own
                kp2, vp2 = (_pool_to_device(KC.sentinel_pool(c, hd, kv), kv) for _ in range(2))
                k_rot = ops.rope(kn, dcos, dsin, positions=lens, style=style, layout=layout)
                out2 = ops.kv_cache_append(k_rot, vn, kp2, vp2, table, lens, kv_dtype=kvd, layout=layout, update_lens=False)
                torch.cuda.synchronize()
                two, one = _bits(kp2, kv), _bits(kp, kv)
                np.testing.assert_array_equal(one[~knan], two[~knan], err_msg=f"{what}: fused against rope + append")
                assert np.isnan(KC.widen(two, kv)[knan]).all()
                np.testing.assert_array_equal(_bits(vp2, kv), _bits(vp, kv))
                np.testing.assert_array_equal(out2.cpu().numpy(), lens_want)
    # the rotation reached the pool: the plain append's K differs wherever a row was written at a position other than 0
    if any(len(KC.written_positions(c, b)) and KC.written_positions(c, b)[-1] > 0 for b in range(c["batch"])):
        assert not np.array_equal(kw, KC.expected_append(name, hd, kv)[0])


@pytest.mark.parametrize("sk", range(len(F8.SCALES)), ids=F8.SCALE_IDS)
@pytest.mark.parametrize("hd", KC.HEAD_DIMS)
@pytest.mark.parametrize("name", list(KC.APPEND_CASES))
def test_append_rope_fp8_rows_lengths_and_everything_else(gpu, name, hd, sk):
    """the same for the fp8 entry with the tokens and scale sets of kv_fp8_cases: raw bytes against F8.quant of the rule-rotated K
    through KC.append_rule, a NaN byte wherever the rule's value is a NaN, and against rope + kv_cache_append_fp8"""
    from candle_birefnet_amd import ops
    c = KC.APPEND_CASES[name]
    sname, ks1, vs1 = F8.SCALES[sk]
    ks, vs = F8.per_head_scales(c["kv_heads"]) if sname == "odd" else F8.scale_arrays(c["kv_heads"], ks1, vs1)
    k, v = F8.new_tokens(name, hd, ks.tobytes(), vs.tobytes())
    _, vw, lens_want, _, vnan = F8.expected_append(name, hd, ks, vs)
    n_pages = KC.n_pages_of(c)
    table_np, lens_np = KC.table_of(name), np.asarray(c["lens"], np.int32)
    table = _dev(table_np)
    dks, dvs = (_dev(ks), _dev(vs)) if sk else (None, None)
    none = np.zeros(vw.shape, bool)

    def check(got, want, nan, what):
        np.testing.assert_array_equal(got[~nan], want[~nan], err_msg=what)
        assert ((got[nan] & 0x7F) == 0x7F).all(), f"{what}: a NaN token is not a NaN byte in the pool"

    for style in RC.STYLES:
        for rd in RC.rot_dims(hd):
            kq = F8.quant(RC.rotated_k(name, k, rd, style), ks[None, None, :, None])
            kw = KC.append_rule(kq, F8.sentinel_pool(c, hd), table_np, lens_np)[0]
            knan = KC.append_rule((kq & 0x7F) == 0x7F, none, table_np, lens_np)[0]
            dcos, dsin = _tables(rd)
            for layout in c["layouts"]:
                what = f"{style} rot_dim {rd} {layout}"
                big = [_dev(F8.sentinel_pool(c, hd, n_pages + 2 * KC.MARGIN)) for _ in range(2)]
                kp, vp = (b[KC.MARGIN:KC.MARGIN + n_pages] for b in big)
                lens = torch.tensor(c["lens"], dtype=torch.int32, device="cuda")
                kn, vn = _append_inputs(name, hd, layout, k, v)
                out = ops.kv_cache_append_rope_fp8(kn, vn, dcos, dsin, kp, vp, dks, dvs, table, lens, style=style, layout=layout, update_lens=False)
                torch.cuda.synchronize()
                check(kp.cpu().numpy(), kw, knan, f"k_pages {what}")
                check(vp.cpu().numpy(), vw, vnan, f"v_pages {what}")
                np.testing.assert_array_equal(out.cpu().numpy(), lens_want)
                np.testing.assert_array_equal(lens.cpu().numpy(), lens_np)
                for b in big:
                    edge = b.cpu().numpy()
                    assert (edge[:KC.MARGIN] == F8.UNREAD).all() and (edge[KC.MARGIN + n_pages:] == F8.UNREAD).all(), f"{what}: a margin was written"
                kp2, vp2 = (_dev(F8.sentinel_pool(c, hd)) for _ in range(2))
                k_rot = ops.rope(kn, dcos, dsin, positions=lens, style=style, layout=layout)
                ops.kv_cache_append_fp8(k_rot, vn, kp2, vp2, dks, dvs, table, lens, layout=layout, update_lens=False)
                torch.cuda.synchronize()
                check(kp.cpu().numpy(), kp2.cpu().numpy(), knan, f"{what}: fused against rope + append")
                np.testing.assert_array_equal(vp2.cpu().numpy(), vp.cpu().numpy())


def _expected(name, hd, kv, rd, style):
    """(k pool bits, its NaN mask, kv_lens_out) of the rule on a sentinel pool"""
    c = KC.APPEND_CASES[name]
    table_np, lens_np = KC.table_of(name), np.asarray(c["lens"], np.int32)
    kr = RC.rotated_k(name, KC.new_tokens(name, hd)[0], rd, style)
    kw, lens_want = KC.append_rule(KC.to_bits(kr, kv), KC.sentinel_pool(c, hd, kv), table_np, lens_np)
    return kw, KC.append_rule(np.isnan(kr), np.zeros(kw.shape, bool), table_np, lens_np)[0], lens_want


def test_lengths_in_place_and_host_pools(gpu):
    """update_lens True / None, and BRN_MEM_HOST numpy pools written in place, give the pool of the separate-lengths call"""
    from candle_birefnet_amd import ops
    name, hd, kv, rd, style = "dropped", 32, "f16", 16, "interleaved"
    c = KC.APPEND_CASES[name]
    k, v = KC.new_tokens(name, hd)
    kw, knan, lens_want = _expected(name, hd, kv, rd, style)
    dcos, dsin = _tables(rd)
    for update in (True, None):
        kp, vp = (_pool_to_device(KC.sentinel_pool(c, hd, kv), kv) for _ in range(2))
        lens = torch.tensor(c["lens"], dtype=torch.int32, device="cuda")
        out = ops.kv_cache_append_rope(_dev(k), _dev(v), dcos, dsin, kp, vp, _dev(KC.table_of(name)), lens, kv_dtype=kv, style=style, update_lens=update)
        torch.cuda.synchronize()
        _check_pool(_bits(kp, kv), kw, knan, kv, f"update_lens={update}")
        assert (out is lens) if update else (out is None)
        np.testing.assert_array_equal(lens.cpu().numpy(), lens_want if update else np.asarray(c["lens"], np.int32))
    name = "straddle"                                            # (host lengths must stay inside the table: 30 + 5 <= 40)
    c = KC.APPEND_CASES[name]
    k, v = KC.new_tokens(name, hd)
    kw, knan, lens_want = _expected(name, hd, kv, rd, style)
    kp, vp = KC.sentinel_pool(c, hd, kv), KC.sentinel_pool(c, hd, kv)
    lens = np.array(c["lens"], np.int32)
    assert ops.kv_cache_append_rope(k, v, *RC.table(rd), kp, vp, np.array(KC.table_of(name)), lens, kv_dtype=kv, style=style) is lens
    _check_pool(kp, kw, knan, kv, "host k_pages")
    np.testing.assert_array_equal(lens, lens_want)


def test_a_non_contiguous_device_table_gives_the_bits_of_the_contiguous_one(gpu):
    """block_table as a column slice of a wider int32 device tensor: the wrapper's contiguous copy must live until the launch.  With
    update_lens=False (a new lengths tensor is allocated between the copy and the call) both rope appends give the pool and the lengths
    of the call on the contiguous table, which are the rule's"""
    from candle_birefnet_amd import ops
    name, hd, rd, style = "three_pages", 32, 32, "half"
    c = KC.APPEND_CASES[name]
    k, v = KC.new_tokens(name, hd)
    table_np = np.array(KC.table_of(name))
    wide = torch.full((c["batch"], 2 * c["max_pages"] + 3), -77, dtype=torch.int32, device="cuda")
    wide[:, 1:1 + 2 * c["max_pages"]:2] = _dev(table_np)
    sliced = wide[:, 1:1 + 2 * c["max_pages"]:2]
    assert not sliced.is_contiguous() and np.array_equal(sliced.cpu().numpy(), table_np)
    dcos, dsin = _tables(rd)
    kn, vn = _dev(k), _dev(v)
    kw, knan, lens_want = _expected(name, hd, "bf16", rd, style)
    ks, vs = F8.per_head_scales(c["kv_heads"])
    dks, dvs = _dev(ks), _dev(vs)
    for rounds in range(3):                                    # (the allocator hands a freed block out again at once: a few rounds of the same call)
        got = {}
        for which, table in (("contiguous", _dev(table_np)), ("sliced", sliced)):
            lens = torch.tensor(c["lens"], dtype=torch.int32, device="cuda")
            kp, vp = (_pool_to_device(KC.sentinel_pool(c, hd, "bf16"), "bf16") for _ in range(2))
            out = ops.kv_cache_append_rope(kn, vn, dcos, dsin, kp, vp, table, lens, kv_dtype="bf16", style=style, update_lens=False)
            kp8, vp8 = (_dev(F8.sentinel_pool(c, hd)) for _ in range(2))
            out8 = ops.kv_cache_append_rope_fp8(kn, vn, dcos, dsin, kp8, vp8, dks, dvs, table, lens, style=style, update_lens=False)
            torch.cuda.synchronize()
            got[which] = (_bits(kp, "bf16"), _bits(vp, "bf16"), out.cpu().numpy(), kp8.cpu().numpy(), vp8.cpu().numpy(), out8.cpu().numpy())
            np.testing.assert_array_equal(lens.cpu().numpy(), np.asarray(c["lens"], np.int32))
        for a, b in zip(got["contiguous"], got["sliced"]):
            np.testing.assert_array_equal(a, b)
        _check_pool(got["sliced"][0], kw, knan, "bf16", "k_pages through the sliced table")
        np.testing.assert_array_equal(got["sliced"][2], lens_want)
        np.testing.assert_array_equal(got["sliced"][5], lens_want)
    assert (wide[:, ::2] == -77).all()


# ---- one graph is a rotary decode step ----
STEP = 3
GRAPH_N_POS = 320                 # the lengths of PG.FIRST end at 300 and 37


class _Step:
    """A decode state on the device for PG.FIRST (test_kv_cache_gpu's, restated for a rotary step): q (BSHD), a 16-bit pool that holds
    the first len_b - 3 keys of every sequence (every other element the sentinel NaN), the table, lengths at len_b - 3, outputs and
    workspace allocated once"""

    def __init__(self, case, kv):
        import candle_birefnet_amd as cb
        (batch, seq_q, heads, kv_heads, hd), page, lens, kind, causal, ks = case
        self.kv = kv
        q, _, _ = PG.logical_inputs(case)
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
            pools.append(_pool_to_device(bits, kv))
        self.kp, self.vp = pools
        self.q = _dev(PG.in_layout(q, "bshd"))
        self.table, self.lens = _dev(table), _dev(start)
        self.ints = (batch, seq_q, PG.max_len(case), heads, kv_heads, hd, kp.shape[0], page, table.shape[1], 0, causal, PG.kind_scale(kind) or 0.0, ks)
        self.geo = (batch, seq_q, heads, kv_heads, hd, kp.shape[0], page, table.shape[1])
        _, _, self.need = cb.ops.flash_attention_splitkv_plan(batch, seq_q, PG.max_len(case), heads, kv_heads, hd, ks)
        self.ws = torch.zeros(max(self.need, 4), dtype=torch.float32, device="cuda")
        self.y = torch.full(self.q.shape, float("nan"), dtype=torch.float32, device="cuda")
        self.lse = torch.full((batch, heads, seq_q), float("nan"), dtype=torch.float32, device="cuda")

    def step(self, k_new, v_new, cos, sin, rd, style, stream=None):
        """raw calls: rope on q in place at positions = kv_lens, append_rope with lengths in place, attention"""
        import candle_birefnet_amd as cb
        lib = cb._ffi.lib
        batch, seq_q, heads, kv_heads, hd, n_pages, page, max_pages = self.geo
        s = stream if stream is not None else torch.cuda.current_stream().cuda_stream
        code = RC.STYLE_CODE[style]
        st, msg = RC.raw_rope(lib, self.q.data_ptr(), batch, seq_q, heads, hd, 0, cos.data_ptr(), sin.data_ptr(), GRAPH_N_POS, rd, code, self.lens.data_ptr(), self.q.data_ptr(), 1, s)
        assert st == 0, msg
        st, msg = RC.raw_append_rope(lib, k_new.data_ptr(), v_new.data_ptr(), batch, int(k_new.shape[1]), kv_heads, hd, 0, cos.data_ptr(), sin.data_ptr(), GRAPH_N_POS, rd, code,
                                     self.kp.data_ptr(), self.vp.data_ptr(), KC.KV_CODE[self.kv], self.table.data_ptr(), self.lens.data_ptr(), self.lens.data_ptr(), n_pages, page,
                                     max_pages, 1, s)
        assert st == 0, msg
        st, msg = KC.raw_attend(lib, self.q.data_ptr(), self.kp.data_ptr(), self.vp.data_ptr(), KC.KV_CODE[self.kv], self.table.data_ptr(), self.lens.data_ptr(), *self.ints,
                                self.y.data_ptr(), self.lse.data_ptr(), self.ws.data_ptr() if self.need else None, self.need, 1, s)
        assert st == 0, msg

    def results(self):
        torch.cuda.synchronize()
        return GQ.to_bhsd(self.y.cpu().numpy(), "bshd"), self.lse.cpu().numpy(), self.lens.cpu().numpy()


@pytest.mark.parametrize("kv", ("bf16", "f16"))
def test_one_graph_is_a_rotary_decode_step(gpu, kv):
    """On a side stream, rope(q, positions = kv_lens) in place, brn_kv_cache_append_rope (one token per sequence, lengths in place) and
    the 16-bit paged attention are captured into one graph.  Three replays, each after new q / k_new / v_new were copied into the
    captured inputs, give the y, lse, lengths and pool bits of (a) the eager calls on a second pool kept in step and (b) the existing
    entries fed numpy-rotated q and k (ops.kv_cache_append + ops.flash_attention_paged) on a third.  y differs between replays and from
    the same step without rotation"""
    from candle_birefnet_amd import ops
    case = PG.FIRST
    (batch, seq_q, heads, kv_heads, hd), page, lens, kind, causal, ks = case
    rd, style = hd, "half"
    cos, sin = RC.table(rd, GRAPH_N_POS)
    dcos, dsin = _tables(rd, GRAPH_N_POS)
    q, k, v = PG.logical_inputs(case)
    tokens = tuple(np.stack([a[b, :, lens[b] - STEP:lens[b]].transpose(1, 0, 2) for b in range(batch)]).astype(np.float32) for a in (k, v))   # [batch, 3, kv_heads, hd]
    graph_side, eager_side, numpy_side, plain_side = (_Step(case, kv) for _ in range(4))
    k_in, v_in = (torch.zeros(batch, 1, kv_heads, hd, device="cuda") for _ in range(2))
    ops.set_compute(kv)
    try:
        warm = _Step(case, kv)                                  # the library and its kernels are loaded before the capture
        warm.step(k_in, v_in, dcos, dsin, rd, style)
        torch.cuda.synchronize()
        side = torch.cuda.Stream()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            graph_side.step(k_in, v_in, dcos, dsin, rd, style, stream=torch.cuda.current_stream().cuda_stream)
        attend = dict(max_kv_len=PG.max_len(case), causal=bool(causal), scale=PG.kind_scale(kind), layout="bshd", kv_splits=ks, return_lse=True, kv_dtype=kv)
        seen = []
        for step in range(STEP):
            tk, tv = (np.ascontiguousarray(t[:, step:step + 1]) for t in tokens)
            qn = np.ascontiguousarray(PG.in_layout(np.roll(q, step, axis=1), "bshd"))      # a new q each step: the heads rotate
            now = np.asarray(lens, np.int32) - STEP + step
            for dst, src in ((k_in, tk), (v_in, tv), (graph_side.q, qn), (eager_side.q, qn)):
                dst.copy_(_dev(src))
            eager_side.step(_dev(tk), _dev(tv), dcos, dsin, rd, style)
            want = eager_side.results()
            # the existing entries on inputs rotated in numpy at the positions the lengths name
            q_rot = RC.rope_rule(qn, cos, sin, RC.table_rows(now, batch, seq_q, GRAPH_N_POS), style)
            k_rot = RC.rope_rule(tk, cos, sin, RC.table_rows(now, batch, 1, GRAPH_N_POS), style)
            ops.kv_cache_append(_dev(k_rot), _dev(tv), numpy_side.kp, numpy_side.vp, numpy_side.table, numpy_side.lens, kv_dtype=kv)
            ny, nlse = ops.flash_attention_paged(_dev(q_rot), numpy_side.kp, numpy_side.vp, numpy_side.table, numpy_side.lens, **attend)
            # the same step without rotation
            ops.kv_cache_append(_dev(tk), _dev(tv), plain_side.kp, plain_side.vp, plain_side.table, plain_side.lens, kv_dtype=kv)
            py, _ = ops.flash_attention_paged(_dev(qn), plain_side.kp, plain_side.vp, plain_side.table, plain_side.lens, **attend)
            graph_side.y.fill_(float("nan"))
            graph_side.lse.fill_(float("nan"))
            torch.cuda.synchronize()
            graph.replay()
            got = graph_side.results()
            for a, b, what in zip(got, want, ("y", "lse", "kv_lens")):
                np.testing.assert_array_equal(a, b, err_msg=f"{what} of replay {step} against the eager calls")
            np.testing.assert_array_equal(got[0], GQ.to_bhsd(ny.cpu().numpy(), "bshd"), err_msg=f"y of replay {step} against the existing entries on numpy-rotated q and k")
            np.testing.assert_array_equal(got[1], nlse.cpu().numpy(), err_msg=f"lse of replay {step} against the existing entries")
            np.testing.assert_array_equal(got[2], numpy_side.lens.cpu().numpy())
            assert got[2].tolist() == [L - STEP + step + 1 for L in lens] and np.isfinite(got[0]).all()
            assert not np.array_equal(got[0], GQ.to_bhsd(py.cpu().numpy(), "bshd")), "the rotation does not matter"
            np.testing.assert_array_equal(graph_side.q.cpu().numpy().view(np.uint32), q_rot.view(np.uint32), err_msg="q rotated in place by the graph")
            seen.append(got[0])
        assert not np.array_equal(seen[0], seen[1]) and not np.array_equal(seen[1], seen[2])
        for other in (eager_side, numpy_side):
            np.testing.assert_array_equal(_bits(graph_side.kp, kv), _bits(other.kp, kv))
            np.testing.assert_array_equal(_bits(graph_side.vp, kv), _bits(other.vp, kv))
        assert not np.array_equal(_bits(graph_side.kp, kv), _bits(plain_side.kp, kv))
    finally:
        ops.set_compute("f32")


def test_refusals_on_the_gpu_leave_the_pool_alone(gpu):
    """a refused call writes nothing: the pool keeps its sentinel, the lengths their values and y its sentinel, and the valid calls that
    follow work"""
    import candle_birefnet_amd as cb
    from candle_birefnet_amd import ops
    lib = cb._ffi.lib
    name, hd, kv, rd, style = "straddle", 32, "bf16", 32, "half"
    c = KC.APPEND_CASES[name]
    k, v = KC.new_tokens(name, hd)
    table_np, lens_np = KC.table_of(name), np.asarray(c["lens"], np.int32)
    kr = RC.rotated_k(name, k, rd, style)
    kw, lens_want = KC.append_rule(KC.to_bits(kr, kv), KC.sentinel_pool(c, hd, kv), table_np, lens_np)
    knan = KC.append_rule(np.isnan(kr), np.zeros(kw.shape, bool), table_np, lens_np)[0]
    kp, vp = (_pool_to_device(KC.sentinel_pool(c, hd, kv), kv) for _ in range(2))
    kn, vn, table = _dev(k), _dev(v), _dev(table_np)
    dcos, dsin = _tables(rd)
    lens = torch.tensor(c["lens"], dtype=torch.int32, device="cuda")
    ok = (kn.data_ptr(), vn.data_ptr(), c["batch"], c["seq_new"], c["kv_heads"], hd, 0, dcos.data_ptr(), dsin.data_ptr(), RC.N_POS, rd, 0, kp.data_ptr(), vp.data_ptr(), 1,
          table.data_ptr(), lens.data_ptr(), lens.data_ptr(), KC.n_pages_of(c), c["page"], c["max_pages"], 1)
    sub = lambda i, val: ok[:i] + (val,) + ok[i + 1:]
    for args, word in ((sub(10, 24), "rot_dim must be"), (sub(11, 2), "style must be"), (sub(9, 0), "1 <= n_pos <= 2^24"), (sub(7, kp.data_ptr()), "cos must not overlap the pool"),
                       (sub(8, dsin.data_ptr() + 4), "cos and sin must be 16-byte aligned"), (sub(14, 3), "kv_type must be"), (sub(3, 0), "1 <= seq_new <= 65536"),
                       (sub(17, lens.data_ptr() + 2), "kv_lens_out must not overlap kv_lens")):
        st, msg = RC.raw_append_rope(lib, *args)
        assert st == 1 and msg.startswith("kv cache append rope: ") and word in msg, (st, msg)
    y = torch.from_numpy(np.full(k.size, X_SENTINEL, np.uint32).view(np.float32)).cuda()
    rok = (kn.data_ptr(), c["batch"], c["seq_new"], c["kv_heads"], hd, 0, dcos.data_ptr(), dsin.data_ptr(), RC.N_POS, rd, 0, lens.data_ptr(), y.data_ptr(), 1)
    rsub = lambda i, val: rok[:i] + (val,) + rok[i + 1:]
    for args, word in ((rsub(9, 48), "rot_dim must be"), (rsub(12, kn.data_ptr() + 64), "y must be x itself"), (rsub(6, y.data_ptr()), "cos must not overlap y"),
                       (rsub(11, lens.data_ptr() + 2), "positions must be 4-byte aligned"), (rsub(4, 96), "head_dim must be")):
        st, msg = RC.raw_rope(lib, *args)
        assert st == 1 and msg.startswith("rope: ") and word in msg, (st, msg)
    torch.cuda.synchronize()
    assert (_bits(kp, kv) == KC.SENTINEL[kv]).all() and (_bits(vp, kv) == KC.SENTINEL[kv]).all() and lens.cpu().numpy().tolist() == list(c["lens"])
    assert (y.cpu().numpy().view(np.uint32) == X_SENTINEL).all()
    np.testing.assert_array_equal(kn.cpu().numpy().view(np.uint32), k.view(np.uint32))
    got = ops.rope(kn, dcos, dsin, positions=lens, style=style)
    ops.kv_cache_append_rope(kn, vn, dcos, dsin, kp, vp, table, lens, kv_dtype=kv, style=style)
    torch.cuda.synchronize()
    RC.assert_bits(got.cpu().numpy(), kr, "rope after the refusals")
    _check_pool(_bits(kp, kv), kw, knan, kv, "k_pages after the refusals")
    np.testing.assert_array_equal(lens.cpu().numpy(), lens_want)
