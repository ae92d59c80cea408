"""brn_flash_attention_paged_kv_forward and brn_kv_cache_append without a GPU: the symbols and their mirrors exist, the header states the
contracts, every refusal of both entries comes before the device check under its own prefix (the inherited limits too) and counts bytes,
the wrappers refuse a pool of the wrong dtype, and the numpy statement of the append rule (kv_cache_cases.append_rule) agrees with the
read-back of flash_attention_paged_cases.fetch_paged on every case of the GPU tests."""
import os
import re

import numpy as np
import pytest

import flash_attention_paged_cases as PG
import kv_cache_cases as KC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ATTEND, APPEND = "brn_flash_attention_paged_kv_forward", "brn_kv_cache_append"


def _header():
    return open(os.path.join(ROOT, "include", "birefnet_hip.h")).read()


def _comment(header, start, end):
    return " ".join(header[header.index(start):header.index(end)].replace("*", " ").split())


def _mode(mode, fn):
    from candle_birefnet_amd import ops
    ops.set_compute(mode)
    try:
        return fn()
    finally:
        ops.set_compute("f32")


def test_symbols_are_exported_declared_and_mirrored():
    import candle_birefnet_amd as cb
    header = _header()
    ffi = open(os.path.join(ROOT, "rust_shim", "src", "hip_ffi.rs")).read()
    readme = open(os.path.join(ROOT, "README.md")).read()
    for name in (ATTEND, APPEND):
        assert hasattr(cb._ffi.lib, name) and name in cb._ffi.DECLARED
        assert f"\nbrn_status {name}(" in header and f"pub fn {name}(" in ffi and name in readme
    assert re.search(r"typedef enum \{ BRN_KV_F32 = 0, BRN_KV_BF16 = 1, BRN_KV_F16 = 2 \} brn_kv_type;", header)
    assert (cb._ffi.BRN_KV_F32, cb._ffi.BRN_KV_BF16, cb._ffi.BRN_KV_F16) == (0, 1, 2)
    # the arguments after kv_type are the paged entry's after v_pages, in its order
    sig = lambda name: " ".join(re.search(r"\nbrn_status %s\((.*?)\);" % name, header, re.S).group(1).split())
    assert sig(ATTEND) == sig("brn_flash_attention_paged_forward").replace("const float* k_pages, const float* v_pages,", "const void* k_pages, const void* v_pages, int kv_type,")
    assert sig(APPEND) == ("const float* k_new, const float* v_new, int batch, int seq_new, int kv_heads, int head_dim, int layout, void* k_pages, void* v_pages, int kv_type, "
                           "const int* block_table, const int* kv_lens, int* kv_lens_out, int n_pages, int page_size, int max_pages, brn_mem loc, int device_ordinal, void* stream")
    assert header.index("\nbrn_status brn_flash_attention_paged_forward(") < header.index(f"\nbrn_status {ATTEND}(") < header.index(f"\nbrn_status {APPEND}(")
    assert callable(cb.ops.kv_cache_append) and f"{len(cb._ffi.DECLARED)} entry points" in readme
    assert "kernels/kv_cache.hip" in open(os.path.join(ROOT, "candle_birefnet_amd", "csrc", "Makefile")).read()


def test_header_states_both_contracts_and_what_is_not_provided():
    header = _header()
    text = _comment(header, "\nbrn_status brn_flash_attention_paged_forward(", f"\nbrn_status {ATTEND}(")
    for words in ("those of brn_flash_attention_paged_forward", "q, y, lse and the workspace stay fp32", "BRN_KV_F32 runs brn_flash_attention_paged_forward's path and returns its bits",
                  "BRN_BF16 reads a bf16 pool and BRN_F16 an f16 pool", "with no conversion", "widening each element exactly",
                  "refused with a message that names both types", "carries the bits of brn_flash_attention_paged_forward in the same compute mode on the pool widened to fp32",
                  '"flash attention paged kv:"', "kv_type one of the three", "16-byte aligned whatever the type", "the overlap rules count bytes"):
        assert words in text, words
    tail = text[text.rindex("Not provided:"):]
    for words in ("fp8 / int8 or otherwise scaled pages", "a K-transposed page layout", "16-bit q / y", "16-bit tensors for the dense, split and varlen entries", "a window or a bias"):
        assert words in tail, words
    text = _comment(header, f"\nbrn_status {ATTEND}(", f"\nbrn_status {APPEND}(")
    for words in ("L_b = min(max(kv_lens[b], 0), cap)", "cap = max_pages page_size", "row (L_b + t) % page_size of page min(max(block_table[b][(L_b + t) / page_size], 0), n_pages - 1)",
                  "is dropped: nothing is written for it and no table entry is read for it", "No other row of the pool is written", "min(L_b + seq_new, cap)",
                  "It may be kv_lens itself", "a launch of their own after the rows", "With NULL, kv_lens is left as it is", "the caller's error", "nothing outside the pool is touched",
                  "round to nearest even", "becomes +-inf in an f16 pool, a NaN stays a NaN", "allocates nothing, does not synchronise the stream and may be captured",
                  "a test convenience", "staged to the device and copied back whole", '"kv cache append:"', "1 <= seq_new <= 65536", "max_pages page_size < 2^31"):
        assert words in text, words
    tail = text[text.rindex("Not provided:"):]
    for words in ("a per-sequence number of new tokens", "copy-on-write or reference counting of shared pages"):
        assert words in tail, words
    # the two older entries point here
    paged = _comment(header, "\nbrn_status brn_flash_attention_splitkv_forward(", "\nbrn_status brn_flash_attention_paged_forward(")
    assert ATTEND in paged[paged.rindex("Not provided:"):] and APPEND in paged[paged.rindex("Not provided:"):]
    split = _comment(header, "\nbrn_status brn_flash_attention_varlen_forward(", "\nbrn_status brn_flash_attention_splitkv_plan(")
    assert ATTEND in split[split.rindex("Not provided:"):] and APPEND in split[split.rindex("Not provided:"):]


@pytest.mark.parametrize("name,args,word,mode", KC.attend_refusals(), ids=[r[0] for r in KC.attend_refusals()])
def test_attention_refusals_come_before_the_device_check(name, args, word, mode):
    """status 1 under the new entry's prefix with a message naming the limit, with or without a device: every inherited limit (the list of
    the paged entry with BRN_KV_F32 inserted) and every new one"""
    import candle_birefnet_amd as cb
    st, msg = _mode(mode, lambda: KC.raw_attend(cb._ffi.lib, *args))
    assert st == 1 and msg.startswith("flash attention paged kv: ") and word in msg, (name, st, msg)


def test_the_type_mismatch_names_both_types():
    import candle_birefnet_amd as cb
    for name, args, word, mode in KC.attend_refusals():
        if "cannot be read" in word:
            _, msg = _mode(mode, lambda: KC.raw_attend(cb._ffi.lib, *args))
            assert "bf16" in msg and " f16" in msg, msg


@pytest.mark.parametrize("name,args,word", KC.append_refusals(), ids=[r[0] for r in KC.append_refusals()])
def test_append_refusals_come_before_the_device_check(name, args, word):
    import candle_birefnet_amd as cb
    st, msg = KC.raw_append(cb._ffi.lib, *args)
    assert st == 1 and msg.startswith("kv cache append: ") and word in msg, (name, st, msg)


def test_overlap_checks_count_bytes():
    """a buffer that starts where a 16-bit pool ends lies inside the same pool counted as fp32: the call passes every check (without a
    device it reaches the device check; with one it runs).  kv_lens_out == kv_lens, the in-place form, passes too"""
    import candle_birefnet_amd as cb
    for name, args, mode in KC.attend_byte_counted_neighbours():
        st, msg = _mode(mode, lambda: KC.raw_attend(cb._ffi.lib, *args))
        assert st in (0, 4), (name, st, msg)
    for name, args in KC.append_byte_counted_neighbours():
        st, msg = KC.raw_append(cb._ffi.lib, *args)
        assert st in (0, 4), (name, st, msg)


def test_well_formed_calls_without_a_device_are_loud():
    import candle_birefnet_amd as cb
    if cb.device_count() > 0:
        pytest.skip("a GPU is present")
    q, kp, vp, y, lse, ws, table, lens = PG._refusal_buffers()
    for mode, kv in (("f32", 0),) + tuple((m, KC.KV_CODE[k]) for m, k in KC.PAIRS):
        st, msg = _mode(mode, lambda: KC.raw_attend(cb._ffi.lib, q, kp, vp, kv, table, lens, 2, 16, 200, 2, 1, 32, 20, 16, 13, 0, 0, 0.0, 2, y, lse, ws, 4224))
        assert st == 4 and "no CPU fallback" in msg, (mode, kv, st, msg)
    kn, vn, kp, vp, table, lens, lo = KC._append_buffers()
    for kv in (0, 1, 2):
        for out in (lo, lens, None):
            st, msg = KC.raw_append(cb._ffi.lib, kn, vn, 2, 4, 1, 32, 0, kp, vp, kv, table, lens, out, 20, 16, 13)
            assert st == 4 and "no CPU fallback" in msg, (kv, st, msg)


def test_wrappers_take_a_pool_as_it_is_or_refuse_it():
    """kv_dtype and the pool's dtype must agree (numpy: uint16 patterns for either type, float16 for f16); the append never converts or
    copies a pool; host lengths and written table entries out of range are refused as the paged wrapper refuses them"""
    import torch
    import candle_birefnet_amd as cb
    case = PG.FIRST
    q = PG.logical_inputs(case)[0]
    kp, vp, table, lens = PG.build_pool(case)
    attend = lambda k, v, kv: cb.ops.flash_attention_paged(q, k, v, table, lens, layout="bhsd", kv_splits=2, kv_dtype=kv)
    with pytest.raises(ValueError, match="kv_dtype"):
        attend(kp, vp, "fp8")
    for k, kv in ((kp, "bf16"), (kp.astype(np.float16), "bf16"), (torch.zeros(kp.shape, dtype=torch.float16), "bf16"), (torch.zeros(kp.shape, dtype=torch.bfloat16), "f16"),
                  (torch.zeros(kp.shape), "f16"), (np.zeros(kp.shape, np.int16), "f16")):
        with pytest.raises(TypeError, match="kv_dtype"):
            attend(k, k, kv)
    with pytest.raises(ValueError, match="expected shape"):
        attend(KC.to_bits(kp, "bf16")[:-1], KC.to_bits(vp, "bf16"), "bf16")
    c = KC.APPEND_CASES["straddle"]
    k, v = KC.new_tokens("straddle", 32)
    tab, ln = np.array(KC.table_of("straddle")), np.array(c["lens"], np.int32)
    pool = lambda kv: (KC.sentinel_pool(c, 32, kv), KC.sentinel_pool(c, 32, kv))
    append = lambda kpool, vpool, kv, t=tab, l=ln, **kw: cb.ops.kv_cache_append(k, v, kpool, vpool, t, l, kv_dtype=kv, **kw)
    with pytest.raises(TypeError, match="kv_dtype"):
        append(*pool("bf16"), None)                       # a uint16 pool is not an fp32 pool
    with pytest.raises(TypeError, match="kv_dtype"):
        append(*(p.view(np.float32) for p in pool("f32")), "f16")
    with pytest.raises(ValueError, match="contiguous"):
        append(*(np.concatenate([p, p], 3)[..., :32] for p in pool("bf16")), "bf16")
    with pytest.raises(ValueError, match="kv_lens must lie in 0 .. max_pages"):
        append(*pool("bf16"), "bf16", l=np.array([49], np.int32))
    for bad in (-1, KC.n_pages_of(c)):
        t = tab.copy()
        t[0, 2] = bad                                     # positions 30 .. 34: slots 1 and 2
        with pytest.raises(ValueError, match="block_table entries at written positions"):
            append(*pool("bf16"), "bf16", t=t)
    with pytest.raises(TypeError, match="in place"):
        append(*pool("bf16"), "bf16", l=[30])
    t = tab.copy()
    t[0, 0] = -9                                          # slot 0 is not written by this call: not checked
    if cb.device_count() == 0:
        with pytest.raises(cb.BrnError) as e:
            append(*pool("f16"), "f16", t=t)
        assert e.value.status == 4


@pytest.mark.parametrize("name", list(KC.APPEND_CASES))
def test_the_append_rule_agrees_with_the_read_back_of_the_paged_walk(name):
    """after the rule has run, PG.fetch_paged (the attention kernels' address rule) finds the new tokens at keys L_b .. of their sequence,
    kv_lens_out counts them, and every row the rule does not name still holds the sentinel.  Cases without out-of-range table entries
    only differ from the clamped one in that the clamp is the identity"""
    c = KC.APPEND_CASES[name]
    table = KC.table_of(name)
    for hd in KC.HEAD_DIMS:
        k, v = KC.new_tokens(name, hd)
        for kv in KC.KV_TYPES:
            kb, vb, lens_out, knan, vnan = KC.expected_append(name, hd, kv)
            fetch = PG.fetch_paged(kb, vb, table)
            named = np.zeros(kb.shape[:2], bool)
            for b in range(c["batch"]):
                pos = np.array(KC.written_positions(c, b), int)
                L = KC.clamp_len(c["lens"][b], KC.cap_of(c))
                assert lens_out[b] == min(L + c["seq_new"], KC.cap_of(c)) == (pos[-1] + 1 if pos.size else L)
                if not pos.size:
                    continue
                for h in range(c["kv_heads"]):
                    gk, gv = fetch(b, h, pos)
                    np.testing.assert_array_equal(gk, KC.to_bits(k[b, pos - L, h], kv))
                    np.testing.assert_array_equal(gv, KC.to_bits(v[b, pos - L, h], kv))
                named[np.clip(table[b, pos // c["page"]], 0, kb.shape[0] - 1), pos % c["page"]] = True
            assert int(named.sum()) == sum(len(KC.written_positions(c, b)) for b in range(c["batch"])), "two tokens share a row"
            assert (kb[~named] == KC.SENTINEL[kv]).all() and (vb[~named] == KC.SENTINEL[kv]).all()
            # a NaN token is a NaN in the pool, and the only NaN among the named rows
            for bits, nan in ((kb, knan), (vb, vnan)):
                assert not nan[~named].any() and np.array_equal(np.isnan(KC.widen(bits, kv))[named], nan[named])
        assert knan.any() or name in ("clamped_lens",), "the case stores a NaN token"


def test_storage_round_trips():
    """to_bits is round_s16 and widen is its exact inverse on what a pool can hold; the 16-bit kernels' cast of a widened element is the
    element ((E)(float)e == e), which is what the bit equality of the attention tests rests on"""
    x = np.concatenate([KC.SPECIALS, np.random.default_rng(5).standard_normal(4096).astype(np.float32) * 50])
    for kv in ("bf16", "f16"):
        bits = KC.to_bits(x, kv)
        w = KC.widen(bits, kv)
        ok = ~np.isnan(x)
        np.testing.assert_array_equal(w[ok].astype(np.float64), PG.round_s16(x, kv)[ok])
        np.testing.assert_array_equal(KC.to_bits(w, kv)[ok], bits[ok])
        assert np.isnan(w[~ok]).all()
    np.testing.assert_array_equal(KC.widen(KC.to_bits(x, "f32"), "f32").view(np.uint32), x.view(np.uint32))
