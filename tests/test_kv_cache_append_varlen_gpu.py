"""brn_kv_cache_append_varlen on the GPU: the append of a packed batch with cu_seqlens_q on the device.

The yardstick is the existing append entry of the pool type (brn_kv_cache_append / brn_kv_cache_append_fp8), called once per sequence
with batch 1 and seq_new = n_b on a second pool: the pool bytes and kv_lens_out must be the same, for fp32, bf16, fp16 and e4m3 pools.
Both pools start as the type's sentinel pattern, so every row that is not appended must still hold it; the padding tokens of the pack
are NaN and must arrive nowhere."""
import numpy as np
import pytest

import flash_attention_paged_varlen_cases as PV
import kv_cache_cases as KC
import kv_fp8_cases as F8

pytestmark = pytest.mark.gpu
f32 = np.float32
POOLS = (None, "bf16", "f16", "e4m3")
E4M3_SENTINEL = 0x5A
TOTAL_Q = 64
# (n_b, length BEFORE the append): a decode token, an idle slot, a fresh prefill over two pages, a chunk inside a page, a chunk across
# three pages of 16, a chunk across a page edge
PACK = ((1, 129), (0, 77), (17, 0), (5, 195), (33, 64), (3, 15))
CONFIGS = ((2, 32), (1, 128))                 # (kv_heads, head_dim)


def _sentinel_pool(shape, pool):
    if pool == "e4m3":
        return np.full(shape, E4M3_SENTINEL, np.uint8)
    kv = pool or "f32"
    return np.full(shape, KC.SENTINEL[kv], KC.BITS[kv])


def _as_pool(bits, pool):
    """what ops takes for the pool: float32 arrays for an fp32 pool (a view of the same memory), the bit patterns otherwise"""
    return bits.view(np.float32) if pool is None else bits


def _table(n_seqs, max_pages, seed):
    """distinct pages for every (sequence, slot), shuffled; 3 pages of the pool are named by nobody"""
    n_pages = n_seqs * max_pages + 3
    rng = np.random.default_rng(seed)
    return rng.permutation(n_pages)[:n_seqs * max_pages].reshape(n_seqs, max_pages).astype(np.int32), n_pages


def _tokens(total_q, kv_heads, hd, cu, seed):
    """k_new, v_new [total_q, kv_heads, hd]: standard normal x 3 with KC.SPECIALS at the start of every token of k; NaN in the padding"""
    rng = np.random.default_rng(seed)
    k, v = (rng.standard_normal((total_q, kv_heads, hd)).astype(f32) * 3 for _ in range(2))
    n = min(KC.SPECIALS.size, kv_heads * hd)
    finite = KC.SPECIALS[np.isfinite(KC.SPECIALS)][:n]
    k.reshape(total_q, -1)[::3, :finite.size] = finite
    k[:cu[0]] = v[:cu[0]] = np.nan
    k[cu[-1]:] = v[cu[-1]:] = np.nan
    return k, v


def _scales(pool, kv_heads):
    return F8.per_head_scales(kv_heads) if pool == "e4m3" else (None, None)


def _packed_append(ops, k, v, cu, kp, vp, pool, ks, vs, table, lens, update_lens=False):
    return ops.kv_cache_append_varlen(k, v, cu, _as_pool(kp, pool), _as_pool(vp, pool), table, lens, kv_dtype=pool, k_scale=ks, v_scale=vs, update_lens=update_lens)


def _per_sequence(ops, k, v, cu, kp, vp, pool, ks, vs, table, lens, cap):
    """the existing entry, one call per sequence with n_b >= 1 (batch 1, seq_new n_b); a sequence with n_b == 0 keeps its clamped length"""
    out = np.empty(len(lens), np.int32)
    calls = 0
    for b in range(len(lens)):
        s, e = int(cu[b]), int(cu[b + 1])
        if e == s:
            out[b] = min(max(int(lens[b]), 0), cap)
            continue
        kb, vb = np.ascontiguousarray(k[None, s:e]), np.ascontiguousarray(v[None, s:e])
        tb, lb = np.ascontiguousarray(table[b:b + 1]), np.ascontiguousarray(lens[b:b + 1])
        if pool == "e4m3":
            out[b] = ops.kv_cache_append_fp8(kb, vb, kp, vp, ks, vs, tb, lb, layout="bshd", update_lens=False)[0]
        else:
            out[b] = ops.kv_cache_append(kb, vb, _as_pool(kp, pool), _as_pool(vp, pool), tb, lb, kv_dtype=pool or "f32", layout="bshd", update_lens=False)[0]
        calls += 1
    return out, calls


def _rows_appended(lens, cu, cap):
    return sum(max(0, min(int(L) + int(cu[b + 1] - cu[b]), cap) - min(max(int(L), 0), cap)) for b, L in enumerate(lens))


@pytest.mark.parametrize("pool", POOLS, ids=[p or "f32" for p in POOLS])
@pytest.mark.parametrize("kv_heads,hd", CONFIGS)
def test_pool_and_lengths_carry_the_bits_of_the_per_sequence_appends(gpu, kv_heads, hd, pool):
    """page 16 and 64, the pack at token 0 and behind two padding tokens: the pool bytes and kv_lens_out of one packed call equal those
    of the existing entry called per sequence; every row not appended keeps the sentinel; no NaN of the padding arrives"""
    from candle_birefnet_amd import ops
    ks, vs = _scales(pool, kv_heads)
    lens = np.array([L for _, L in PACK], np.int32)
    for page in (16, 64):
        max_pages = 256 // page + 1
        cap = max_pages * page
        table, n_pages = _table(len(PACK), max_pages, 5 + page)
        for start in (0, 2):
            cu = PV.cu_of(PACK, start)
            k, v = _tokens(TOTAL_Q, kv_heads, hd, cu, 3 + hd)
            shape = (n_pages, page, kv_heads, hd)
            got_k, got_v, want_k, want_v = (_sentinel_pool(shape, pool) for _ in range(4))
            got_lens = _packed_append(ops, k, v, cu, got_k, got_v, pool, ks, vs, table, lens)
            want_lens, calls = _per_sequence(ops, k, v, cu, want_k, want_v, pool, ks, vs, table, lens, cap)
            assert calls == 5
            np.testing.assert_array_equal(got_k, want_k, err_msg=f"k_pages, page {page}, cu[0] {start}")
            np.testing.assert_array_equal(got_v, want_v, err_msg=f"v_pages, page {page}, cu[0] {start}")
            np.testing.assert_array_equal(got_lens, want_lens)
            assert got_lens.tolist() == [L + n for n, L in PACK] and lens.tolist() == [L for _, L in PACK], "kv_lens itself is left alone"
            sentinel = _sentinel_pool((), pool)
            untouched = (got_k.reshape(n_pages * page, -1) == sentinel).all(axis=1)
            assert int((~untouched).sum()) == _rows_appended(lens, cu, cap) == 59
            assert np.array_equal(untouched, (got_v.reshape(n_pages * page, -1) == sentinel).all(axis=1))
            if pool != "e4m3":
                kv = pool or "f32"
                assert not np.isnan(KC.widen(got_k.reshape(-1), kv)[np.repeat(~untouched, kv_heads * hd)]).any(), "a NaN of the padding tokens arrived"


@pytest.mark.parametrize("pool", (None, "f16", "e4m3"), ids=["f32", "f16", "e4m3"])
def test_lengths_in_place_tokens_dropped_at_cap_and_untrusted_values(gpu, pool):
    """cap = 3 pages of 16: a chunk that runs past cap loses its last tokens, a full sequence all of them, and kv_lens_out stops at cap;
    garbage lengths and a garbage cu_seqlens_q mean their clamped values; update_lens=True writes kv_lens itself (the in-place form)"""
    from candle_birefnet_amd import ops
    kv_heads, hd, page, max_pages = 2, 32, 16, 3
    cap = page * max_pages
    ks, vs = _scales(pool, kv_heads)
    table, n_pages = _table(5, max_pages, 17)
    bad_cu = np.array([-4, 5, 3, 8, 10 ** 9, 7], np.int32)                        # -> 0, 5, 5, 8, 20, 20 at total_q 20
    cu = PV.clamp_starts(bad_cu, 20).astype(np.int32)
    assert cu.tolist() == [0, 5, 5, 8, 20, 20]
    bad_lens = np.array([46, 20, 10 ** 9, -7, 30], np.int32)                      # -> 46, 20, 48, 0, 30
    lens = np.clip(bad_lens, 0, cap).astype(np.int32)
    k, v = _tokens(20, kv_heads, hd, cu, 23)
    shape = (n_pages, page, kv_heads, hd)
    got_k, got_v, want_k, want_v = (_sentinel_pool(shape, pool) for _ in range(4))
    in_place = bad_lens.copy()
    out = _packed_append(ops, k, v, bad_cu, got_k, got_v, pool, ks, vs, table, in_place, update_lens=True)
    assert out is in_place
    want_lens, calls = _per_sequence(ops, k, v, cu, want_k, want_v, pool, ks, vs, table, lens, cap)
    assert calls == 3
    np.testing.assert_array_equal(got_k, want_k)
    np.testing.assert_array_equal(got_v, want_v)
    np.testing.assert_array_equal(in_place, want_lens)
    assert in_place.tolist() == [48, 20, 48, 12, 30]
    sentinel = _sentinel_pool((), pool)
    assert int((~(got_k.reshape(n_pages * page, -1) == sentinel).all(axis=1)).sum()) == 2 + 0 + 12 == _rows_appended(lens, cu, cap), "3 + 3 tokens dropped at cap"


@pytest.mark.parametrize("pool", (None, "bf16"), ids=["f32", "bf16"])
@pytest.mark.parametrize("style", ("half", "interleaved"))
def test_rope_recipe_equals_the_rope_append_per_sequence(gpu, style, pool):
    """the documented recipe, brn_rope_forward with batch = total_q, seq = 1 and per-token positions L_b + t on k_new, then the packed
    append: the pool holds the bits of brn_kv_cache_append_rope called per sequence"""
    from candle_birefnet_amd import ops
    kv_heads, hd, page, rot = 2, 64, 16, 32
    max_pages = 256 // page + 1
    table, n_pages = _table(len(PACK), max_pages, 29)
    lens = np.array([L for _, L in PACK], np.int32)
    cu = PV.cu_of(PACK)
    k, v = _tokens(TOTAL_Q, kv_heads, hd, cu, 31)
    k[cu[-1]:] = v[cu[-1]:] = 0                                                   # (the padding rows go through rope: keep them quiet)
    cos, sin = ops.rope_table(300, rot)
    positions = np.zeros(TOTAL_Q, np.int32)
    for b, (n, L) in enumerate(PACK):
        positions[cu[b]:cu[b] + n] = L + np.arange(n)
    k_rot = ops.rope(k[:, None], cos, sin, positions=positions, style=style, layout="bshd")[:, 0]
    assert not np.array_equal(k_rot[:cu[-1]], k[:cu[-1]])
    shape = (n_pages, page, kv_heads, hd)
    got_k, got_v, want_k, want_v = (_sentinel_pool(shape, pool) for _ in range(4))
    got_lens = _packed_append(ops, np.ascontiguousarray(k_rot), v, cu, got_k, got_v, pool, None, None, table, lens)
    for b, (n, L) in enumerate(PACK):
        if n:
            s = int(cu[b])
            ops.kv_cache_append_rope(np.ascontiguousarray(k[None, s:s + n]), np.ascontiguousarray(v[None, s:s + n]), cos, sin, _as_pool(want_k, pool), _as_pool(want_v, pool),
                                     np.ascontiguousarray(table[b:b + 1]), np.ascontiguousarray(lens[b:b + 1]), kv_dtype=pool or "f32", style=style, layout="bshd", update_lens=False)
    np.testing.assert_array_equal(got_k, want_k)
    np.testing.assert_array_equal(got_v, want_v)
    assert got_lens.tolist() == [L + n for n, L in PACK]
