"""brn_kv_cache_append_fp8 on the GPU, alone and in front of brn_flash_attention_paged_fp8_forward.

Pools start filled with 0xFF, margins included, and are compared on their raw bytes with the numpy / torch statement of the rule
(kv_fp8_cases.quant through kv_cache_cases.append_rule): x / scale in fp32, clamped to +-448 with NaN kept, rounded to nearest even into
e4m3fn.  Where the expected byte is a NaN the stored byte is checked as (byte & 0x7F) == 0x7F.  The tokens are KC.new_tokens with
KC.SPECIALS, plus the values that matter in e4m3 (ties, 448, 464, 465, 1e6, 2^-9, 2^-10, 1.5 * 2^-9, +-0), each times the head's scale."""
import numpy as np
import pytest
import torch

import flash_attention_paged_cases as PG
import kv_cache_cases as KC
import kv_fp8_cases as F8

pytestmark = pytest.mark.gpu
f32 = np.float32


def _scales(kv_heads, sk):
    """the scale set sk per head: uniform for ones / pow2, different per head for the third"""
    name, ks, vs = F8.SCALES[sk]
    return F8.per_head_scales(kv_heads) if name == "odd" else F8.scale_arrays(kv_heads, ks, vs)


def _dev(a):
    return torch.from_numpy(np.array(a)).cuda()


def _check_pool(got, want, nan, what):
    np.testing.assert_array_equal(got[~nan], want[~nan], err_msg=what)
    assert ((got[nan] & 0x7F) == 0x7F).all(), f"{what}: a NaN token is not a NaN byte in the pool"


@pytest.mark.parametrize("sk", range(len(F8.SCALES)), ids=F8.SCALE_IDS)
@pytest.mark.parametrize("hd", KC.HEAD_DIMS)
@pytest.mark.parametrize("name", list(KC.APPEND_CASES))
def test_rows_lengths_and_everything_else(gpu, name, hd, sk):
    """every case, head_dim and scale set (both layouts where the case names two): the pool's bytes after the call are the rule's on a
    pool of 0xFF, kv_lens_out is the rule's and kv_lens is unchanged; dropped positions write nothing.  The pool is the middle of a
    buffer with MARGIN pages of 0xFF on each side, wider than any page number a table holds: the margins keep their bytes"""
    from candle_birefnet_amd import ops
    c = KC.APPEND_CASES[name]
    ks, vs = _scales(c["kv_heads"], sk)
    k, v = F8.new_tokens(name, hd, ks.tobytes(), vs.tobytes())
    kw, vw, lens_want, knan, vnan = F8.expected_append(name, hd, ks, vs)
    n_pages = KC.n_pages_of(c)
    table = _dev(KC.table_of(name))
    for layout in c["layouts"]:
        big = [_dev(F8.sentinel_pool(c, hd, n_pages + 2 * KC.MARGIN)) for _ in range(2)]
        kp, vp = (b[KC.MARGIN:KC.MARGIN + n_pages] for b in big)
        assert kp.is_contiguous() and kp.data_ptr() % 16 == 0
        lens = torch.tensor(c["lens"], dtype=torch.int32, device="cuda")
        kn, vn = (_dev(PG.in_layout(a.transpose(0, 2, 1, 3), layout) if layout == "bhsd" else a) for a in (k, v))
        out = ops.kv_cache_append_fp8(kn, vn, kp, vp, _dev(ks) if sk else None, _dev(vs) if sk else None, table, lens, layout=layout, update_lens=False)
        torch.cuda.synchronize()
        _check_pool(kp.cpu().numpy(), kw, knan, f"k_pages {layout}")
        _check_pool(vp.cpu().numpy(), vw, vnan, f"v_pages {layout}")
        np.testing.assert_array_equal(out.cpu().numpy(), lens_want)
        np.testing.assert_array_equal(lens.cpu().numpy(), np.asarray(c["lens"], np.int32))
        for b in big:
            edge = b.cpu().numpy()
            assert (edge[:KC.MARGIN] == F8.UNREAD).all() and (edge[KC.MARGIN + n_pages:] == F8.UNREAD).all(), "a margin was written"
    # exactly the written rows changed (a written row holds at least one byte that is not 0xFF)
    written = sum(len(KC.written_positions(c, b)) for b in range(c["batch"]))
    assert int((kw != F8.UNREAD).any(axis=(2, 3)).sum()) == written


@pytest.mark.parametrize("sk", (0, 1), ids=F8.SCALE_IDS[:2])
def test_what_the_conversion_makes_of_the_specials(gpu, sk):
    """the special values, read back from where the rule puts them, against literal bytes: ties to even, saturation at 448 by the clamp
    (464, 465, 1e6 and KC's 70000 / 3e38), 2^-9 kept, 2^-10 a tie that goes to 0, 1.5 * 2^-9 a tie that goes up, -2^-10 to -0, +-0 keep
    their sign, a NaN becomes a NaN byte.  With the scales that are powers of two (x * s) / s is x, so the bytes are literal; the third
    scale set is compared with quant() in the test above"""
    from candle_birefnet_amd import ops
    name, hd = "straddle", 32
    c = KC.APPEND_CASES[name]
    ks, vs = _scales(c["kv_heads"], sk)
    k, v = F8.new_tokens(name, hd, ks.tobytes(), vs.tobytes())
    kp, vp = (_dev(F8.sentinel_pool(c, hd)) for _ in range(2))
    table = KC.table_of(name)
    ops.kv_cache_append_fp8(_dev(k), _dev(v), kp, vp, _dev(ks), _dev(vs), _dev(table), torch.tensor(c["lens"], dtype=torch.int32, device="cuda"), update_lens=None)
    torch.cuda.synchronize()
    L, n0, n = c["lens"][0], KC.SPECIALS.size, F8.FP8_SPECIALS.size
    for pool, h in ((kp, 0), (kp, 1), (vp, 1)):
        row = pool.cpu().numpy()[table[0, L // c["page"]], L % c["page"], h]           # token 0 of head h
        assert row[n0:n0 + n].tolist() == [0x38, 0x3A, 0xB8, 0x7E, 0x7E, 0x7E, 0x7E, 0xFE, 0x01, 0x00, 0x02, 0x80, 0x00, 0x80], (h, [hex(x) for x in row[n0:n0 + n]])
    if sk == 0:
        row = kp.cpu().numpy()[table[0, L // c["page"]], L % c["page"], 0]             # head 0 of k starts with KC.SPECIALS, unscaled
        np.testing.assert_array_equal(row[:15], F8.quant(KC.SPECIALS[:15], 1))
        assert row[6] == 0x00 and row[7] == 0x80 and row[11] == 0x7E and row[12] == 0xFE and (row[15] & 0x7F) == 0x7F and row[16] == 0x7E


def test_lengths_separate_in_place_and_null(gpu):
    """kv_lens_out separate from kv_lens, equal to kv_lens (in place, also across two calls in a row), and NULL: the same pool bytes"""
    from candle_birefnet_amd import ops
    name, hd, sk = "dropped", 32, 2
    c = KC.APPEND_CASES[name]
    ks, vs = _scales(c["kv_heads"], sk)
    kw, vw, lens_want, knan, vnan = F8.expected_append(name, hd, ks, vs)
    table = _dev(KC.table_of(name))
    kn, vn = (_dev(a) for a in F8.new_tokens(name, hd, ks.tobytes(), vs.tobytes()))
    ksd, vsd = _dev(ks), _dev(vs)
    for update in (False, True, None):
        kp, vp = (_dev(F8.sentinel_pool(c, hd)) for _ in range(2))
        lens = torch.tensor(c["lens"], dtype=torch.int32, device="cuda")
        out = ops.kv_cache_append_fp8(kn, vn, kp, vp, ksd, vsd, table, lens, update_lens=update)
        torch.cuda.synchronize()
        _check_pool(kp.cpu().numpy(), kw, knan, f"k_pages update_lens={update}")
        _check_pool(vp.cpu().numpy(), vw, vnan, f"v_pages update_lens={update}")
        if update is None:
            assert out is None
        else:
            np.testing.assert_array_equal(out.cpu().numpy(), lens_want)
        assert (out is lens) == (update is True)
        np.testing.assert_array_equal(lens.cpu().numpy(), lens_want if update else np.asarray(c["lens"], np.int32))
        if update:
            ops.kv_cache_append_fp8(kn, vn, kp, vp, ksd, vsd, table, lens, update_lens=True)      # at cap: every token dropped
            torch.cuda.synchronize()
            _check_pool(kp.cpu().numpy(), kw, knan, "k_pages after a step at cap")
            assert lens.cpu().numpy().tolist() == [KC.cap_of(c)]


def test_host_arrays_and_float8_tensors_carry_the_bytes_of_uint8_tensors(gpu):
    """BRN_MEM_HOST (the pool staged up and copied back whole) on numpy uint8 pools written in place, and torch.float8_e4m3fn pools on
    the device"""
    from candle_birefnet_amd import ops
    name, hd, sk = "three_pages", 32, 2
    c = KC.APPEND_CASES[name]
    ks, vs = _scales(c["kv_heads"], sk)
    k, v = F8.new_tokens(name, hd, ks.tobytes(), vs.tobytes())
    kw, vw, lens_want, knan, vnan = F8.expected_append(name, hd, ks, vs)
    kp, vp = F8.sentinel_pool(c, hd), F8.sentinel_pool(c, hd)
    lens = np.array(c["lens"], np.int32)
    out = ops.kv_cache_append_fp8(k, v, kp, vp, ks, vs, np.array(KC.table_of(name)), lens)
    assert out is lens
    _check_pool(kp, kw, knan, "host k_pages")
    _check_pool(vp, vw, vnan, "host v_pages")
    np.testing.assert_array_equal(lens, lens_want)
    kp8, vp8 = (_dev(F8.sentinel_pool(c, hd)).view(torch.float8_e4m3fn) for _ in range(2))
    ops.kv_cache_append_fp8(_dev(k), _dev(v), kp8, vp8, _dev(ks), _dev(vs), _dev(KC.table_of(name)), torch.tensor(c["lens"], dtype=torch.int32, device="cuda"))
    torch.cuda.synchronize()
    _check_pool(kp8.view(torch.uint8).cpu().numpy(), kw, knan, "float8 k_pages")
    _check_pool(vp8.view(torch.uint8).cpu().numpy(), vw, vnan, "float8 v_pages")


CASE128 = ((3, 1, 5, 1, 128), 64, (1000, 512, 3), "std1", 1, 4)      # the D 128 row of the paged cases with a sequence that starts empty


@pytest.mark.parametrize("mode", F8.MODES)
@pytest.mark.parametrize("case,calls", ((PG.FIRST, 3), (CASE128, 1)), ids=("first-3x1", "d128-1x3"))
def test_append_then_attend_is_attention_on_the_cpu_quantised_pool(gpu, case, calls, mode):
    """round trip: the pool holds len_b - 3 keys of each sequence quantised on the CPU; the last 3 arrive as fp32 tokens through the
    append (three calls of one token, or one of three).  Attention on that pool then carries the bits of the fp8 attention entry on the
    pool quantised WHOLLY on the CPU, and the two pools hold the same bytes wherever a key lives"""
    from candle_birefnet_amd import ops
    (batch, seq_q, heads, kv_heads, hd), page, lens, _, causal, ksplits = case
    ks, vs = F8.per_head_scales(kv_heads)
    kb, vb, table, _ = F8.pool(case, ks, vs)
    q, k, v = PG.logical_inputs(case)
    start = np.asarray(lens, np.int32) - 3
    assert min(lens) >= 3
    keep = np.zeros(kb.shape[:2], bool)
    for b in range(batch):
        pos = np.arange(start[b])
        keep[table[b, pos // page], pos % page] = True
    pools = []
    for a in (kb, vb):
        a = np.array(a)
        a[~keep] = F8.UNREAD
        pools.append(_dev(a))
    tokens = tuple(_dev(np.stack([a[b, :, lens[b] - 3:lens[b]].transpose(1, 0, 2) for b in range(batch)]).astype(f32)) for a in (k, v))
    dl, dt, dks, dvs = _dev(start), _dev(table), _dev(ks), _dev(vs)
    kw = dict(max_kv_len=PG.max_len(case), causal=bool(causal), scale=F8.case_scale(case), layout="bhsd", kv_splits=ksplits, return_lse=True)
    ops.set_compute(mode)
    try:
        for i in range(0, 3, 3 // calls):
            ops.kv_cache_append_fp8(tokens[0][:, i:i + 3 // calls].contiguous(), tokens[1][:, i:i + 3 // calls].contiguous(), *pools, dks, dvs, dt, dl)
        y, lse = ops.flash_attention_paged_fp8(_dev(q), *pools, dks, dvs, dt, dl, **kw)
        torch.cuda.synchronize()
        want_y, want_lse = ops.flash_attention_paged_fp8(q, np.array(kb), np.array(vb), ks, vs, table, np.asarray(lens, np.int32), **kw)
    finally:
        ops.set_compute("f32")
    np.testing.assert_array_equal(dl.cpu().numpy(), np.asarray(lens, np.int32))
    live = kb != F8.UNREAD
    np.testing.assert_array_equal(pools[0].cpu().numpy()[live], kb[live])
    np.testing.assert_array_equal(y.cpu().numpy(), want_y)
    np.testing.assert_array_equal(lse.cpu().numpy(), want_lse)
    assert not np.isnan(want_y).any()


def test_refusals_on_the_gpu_leave_the_pool_alone(gpu):
    """a refused append writes nothing: the pool keeps its 0xFF and the lengths their values, and the valid call that follows works"""
    import candle_birefnet_amd as cb
    from candle_birefnet_amd import ops
    name, hd, sk = "straddle", 32, 2
    c = KC.APPEND_CASES[name]
    ks, vs = _scales(c["kv_heads"], sk)
    kw, vw, lens_want, knan, vnan = F8.expected_append(name, hd, ks, vs)
    kp, vp = (_dev(F8.sentinel_pool(c, hd)) for _ in range(2))
    kn, vn = (_dev(a) for a in F8.new_tokens(name, hd, ks.tobytes(), vs.tobytes()))
    table, ksd, vsd = _dev(KC.table_of(name)), _dev(ks), _dev(vs)
    lens = torch.tensor(c["lens"], dtype=torch.int32, device="cuda")
    ok = (kn.data_ptr(), vn.data_ptr(), c["batch"], c["seq_new"], c["kv_heads"], hd, 0, kp.data_ptr(), vp.data_ptr(), ksd.data_ptr(), vsd.data_ptr(), table.data_ptr(),
          lens.data_ptr(), lens.data_ptr(), KC.n_pages_of(c), c["page"], c["max_pages"], 1)
    sub = lambda i, v: ok[:i] + (v,) + ok[i + 1:]
    for args, word in ((sub(3, 0), "1 <= seq_new <= 65536"), (sub(8, kp.data_ptr()), "k_pages and v_pages must not overlap"), (sub(0, kn.data_ptr() + 4), "16-byte aligned"),
                       (sub(9, ksd.data_ptr() + 2), "4-byte aligned"), (sub(10, kp.data_ptr() + 64), "v_scale must not overlap the pool"),
                       (sub(13, lens.data_ptr() + 2), "kv_lens_out must not overlap kv_lens")):
        st, msg = F8.raw_append(cb._ffi.lib, *args)
        assert st == 1 and msg.startswith("kv cache append fp8: ") and word in msg, (st, msg)
    torch.cuda.synchronize()
    assert (kp.cpu().numpy() == F8.UNREAD).all() and (vp.cpu().numpy() == F8.UNREAD).all() and lens.cpu().numpy().tolist() == list(c["lens"])
    ops.kv_cache_append_fp8(kn, vn, kp, vp, ksd, vsd, table, lens)
    torch.cuda.synchronize()
    _check_pool(kp.cpu().numpy(), kw, knan, "k_pages after the refusals")
    np.testing.assert_array_equal(lens.cpu().numpy(), lens_want)
