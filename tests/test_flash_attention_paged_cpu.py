"""brn_flash_attention_paged_forward without a GPU: the symbol and its mirrors exist, the header states the promise, the clamps, the
all-empty row, the limits and what is not provided, every refusal comes before the device check, the wrapper refuses what only it can
know, and the numpy emulation of the paged walk (flash_attention_paged_cases.emulate) stays inside the bounds the GPU tests use and
does not depend on where the pages lie."""
import os
import re

import numpy as np
import pytest

import flash_attention_paged_cases as PG
import flash_attention_splitkv_cases as SK

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "brn_flash_attention_paged_forward"


def _header():
    return open(os.path.join(ROOT, "include", "birefnet_hip.h")).read()


def _comment(header, start, end):
    return " ".join(header[header.index(start):header.index(end)].replace("*", " ").split())


def test_symbol_is_exported_declared_and_mirrored():
    import candle_birefnet_amd as cb
    assert hasattr(cb._ffi.lib, NAME) and NAME in cb._ffi.DECLARED
    header = _header()
    assert re.search(r"\nbrn_status brn_flash_attention_paged_forward\(const float\* q, const float\* k_pages, const float\* v_pages,"
                     r"\s+const int\* block_table, const int\* kv_lens,"
                     r"\s+int batch, int seq_q, int max_kv_len, int heads, int kv_heads, int head_dim,"
                     r"\s+int n_pages, int page_size, int max_pages,"
                     r"\s+int layout, int causal, float scale, int kv_splits,"
                     r"\s+float\* y, float\* lse, float\* workspace, size_t workspace_floats,"
                     r"\s+brn_mem loc, int device_ordinal, void\* stream\);", header)
    assert header.index("\nbrn_status brn_flash_attention_splitkv_forward(") < header.index(f"\nbrn_status {NAME}(") < header.index("\nbrn_status brn_patch_merging_forward(")
    assert callable(cb.ops.flash_attention_paged)
    ffi = open(os.path.join(ROOT, "rust_shim", "src", "hip_ffi.rs")).read()
    assert f"pub fn {NAME}(" in ffi
    readme = open(os.path.join(ROOT, "README.md")).read()
    assert NAME in readme and f"{len(cb._ffi.DECLARED)} entry points" in readme


def test_header_states_the_promise_the_clamps_the_empty_row_the_limits_and_what_is_not_provided():
    text = _comment(_header(), "\nbrn_status brn_flash_attention_splitkv_forward(", f"\nbrn_status {NAME}(")
    for words in ("no atomics", "fixed order s = 0 .. S - 1", "a repeated call repeats its bits",
                  "not on which physical pages hold the keys", "page_size, n_pages, max_pages, `batch`, the other sequences' lengths, the launch grid or which rows share its workgroup",
                  "allocates nothing, does not synchronise the stream and may be captured into a graph",
                  "changing kv_lens, block_table and the pool contents between replays is the intended use",
                  "carries the bits of brn_flash_attention_splitkv_forward on that sequence's keys gathered into a dense tensor with seq_kv = len_b",
                  "min(max(kv_lens[b], 0), max_kv_len)", "min(max(page, 0), n_pages - 1)", "no address in a kernel depends on either value other than through these clamps",
                  "An out-of-range length therefore means", "never an access outside the pool or the table",
                  "at or past ceil(len_b / page_size) of its sequence is never used to form an address", "at or past len_b are never read into the arithmetic",
                  "the host never reads them for BRN_MEM_DEVICE", "Offsets into the pool are 64-bit",
                  "j <= i + len_b - seq_q", "y = 0 (exact zeros) and lse = -inf, no NaN anywhere", "len_b == 0 and causal rows with i + len_b - seq_q < 0",
                  "brn_flash_attention_splitkv_plan(batch, seq_q, max_kv_len, heads, kv_heads, head_dim, kv_splits)", "O_part = 0 and lse2_part = -inf",
                  "S == 1 writes y and lse directly and touches no workspace",
                  '"flash attention paged:"', "causal does not require max_kv_len >= seq_q", "block_table and kv_lens not NULL", "page_size 16, 32, 64, 128 or 256",
                  "n_pages >= 1, max_pages >= 1, n_pages page_size < 2^31", "1 <= max_kv_len <= min(65536, max_pages page_size)",
                  "overlap neither each other nor any of the five inputs", "16-byte aligned, the two int arrays 4-byte aligned"):
        assert words in text, words
    tail = text[text.rindex("Not provided:"):]
    for words in ("a bias", "a window", "16-bit or quantised pages", "a K-transposed page layout", "appending to the cache"):
        assert words in tail, words


def test_the_split_entry_still_says_it_has_no_paged_form_and_points_here():
    text = _comment(_header(), "\nbrn_status brn_flash_attention_varlen_forward(", "\nbrn_status brn_flash_attention_splitkv_plan(")
    tail = text[text.rindex("Not provided:"):]
    assert "packed or paged K / V" in tail and NAME in tail


@pytest.mark.parametrize("name,args,word", PG.refusals(), ids=[r[0] for r in PG.refusals()])
def test_refusals_come_before_the_device_check(name, args, word):
    """status 1 with the entry's prefix and a message naming the limit, with or without a device.  The well-formed neighbour of every
    call is (q, kp, vp, table, lens, 2, 16, 200, 2, 1, 32, 20, 16, 13, 0, 0, 0.0, 2, y, lse, ws, 4224)"""
    import candle_birefnet_amd as cb
    st, msg = PG.raw_call(cb._ffi.lib, *args)
    assert st == 1 and msg.startswith("flash attention paged: ") and word in msg, (name, st, msg)


def test_well_formed_call_without_a_device_is_loud():
    """the neighbour of the refusals, and causal with max_kv_len < seq_q (no limit of this entry), reach the device check"""
    import candle_birefnet_amd as cb
    if cb.device_count() > 0:
        pytest.skip("a GPU is present")
    q, kp, vp, y, lse, ws, table, lens = PG._refusal_buffers()
    for ints in ((2, 16, 200, 2, 1, 32, 20, 16, 13, 0, 0, 0.0, 2), (2, 16, 8, 2, 1, 32, 20, 16, 13, 0, 1, 0.0, 1)):
        st, msg = PG.raw_call(cb._ffi.lib, q, kp, vp, table, lens, *ints, y, lse, ws, 4224)
        assert st == 4 and "no CPU fallback" in msg, (ints, st, msg)
    case = PG.FIRST
    qq = PG.logical_inputs(case)[0]
    with pytest.raises(cb.BrnError) as e:
        cb.ops.flash_attention_paged(qq, *PG.build_pool(case), causal=True, layout="bhsd", kv_splits=2, return_lse=True)
    assert e.value.status == 4 and "no CPU fallback" in str(e.value)


def test_wrapper_refuses_host_lengths_and_pages_out_of_range():
    """numpy inputs only: a length outside 0 .. max_kv_len, a USED table entry outside the pool, a wrong dtype or shape, mixed sides.
    An entry past a sequence's last page may hold anything."""
    import candle_birefnet_amd as cb
    case = PG.FIRST
    q = PG.logical_inputs(case)[0]
    kp, vp, table, lens = PG.build_pool(case)
    call = lambda t, l, **kw: cb.ops.flash_attention_paged(q, kp, vp, t, l, layout="bhsd", kv_splits=2, **kw)
    for bad_lens in (np.array([300, -1], np.int32), np.array([305, 37], np.int32)):
        with pytest.raises(ValueError, match="kv_lens must lie in 0 .. max_kv_len"):
            call(table, bad_lens, max_kv_len=300)
    with pytest.raises(ValueError, match="kv_lens must lie in 0 .. max_kv_len"):
        call(table, lens, max_kv_len=299)
    for bad in (-1, kp.shape[0]):
        t = table.copy()
        t[1, 2] = bad                                   # sequence 1 has 37 keys: pages 0, 1, 2
        with pytest.raises(ValueError, match="block_table entries in use"):
            call(t, lens)
    with pytest.raises(ValueError, match="fit int32"):
        call(table.astype(np.float32), lens)
    with pytest.raises(ValueError, match="expected shape"):
        call(table, lens[:1])
    t = table.copy()
    t[1, 3:] = -7                                       # past the last page of sequence 1: never used, not checked
    t[0, -1] = 10 ** 6
    if cb.device_count() == 0:
        with pytest.raises(cb.BrnError) as e:
            call(t, lens)
        assert e.value.status == 4


def test_empty_rows_of_the_cases():
    """the fifth case holds 16 + 8 rows no split has a key for (the empty sequence; queries 0 and 1 of the sequence of 2 keys); the
    first, third and fifth hold partial rows that see no key of their split (the fifth: 3 splits x 16 rows of the empty sequence, 8 + 16 +
    16 of the sequence of 2 keys, none of the long one)"""
    assert [PG.all_empty_rows(PG.FIFTH, b) for b in range(3)] == [0, 16, 8]
    assert [PG.all_empty_rows(c) for c in PG.CASES if c[0] != PG.FIFTH[0]] == [0] * (len(PG.CASES) - 1)
    assert [PG.empty_partial_rows(c) for c in (PG.FIRST, PG.THIRD, PG.FIFTH)] == [8, 216, 88]


def test_pool_builder_hides_nothing_and_poisons_the_rest():
    """the gathered keys are the logical ones; every float outside them is NaN; unused table entries name NaN pages; the pages are shuffled"""
    for case in (PG.FIRST, PG.FIFTH, PG.CASES[-1]):
        _, k, v = PG.logical_inputs(case)
        for page in (None, 16, 256):
            kp, vp, table, lens = PG.build_pool(case, page)
            ps = kp.shape[1]
            finite = 0
            for b, L in enumerate(lens):
                kb, vb = PG.gather(kp, vp, table, b, int(L))
                np.testing.assert_array_equal(kb[0], k[b, :, :L])
                np.testing.assert_array_equal(vb[0], v[b, :, :L])
                finite += int(L) * k.shape[1] * k.shape[3]
                assert np.isnan(kp[table[b, (int(L) + ps - 1) // ps:]]).all()
            assert int(np.isfinite(kp).sum()) == finite == int(np.isfinite(vp).sum())
            assert kp.shape[0] > sum((int(L) + ps - 1) // ps for L in lens) and table.shape[1] == PG.max_pages_of(case, page)
    used = PG.build_pool(PG.FIRST)[2][0, :19]
    assert not np.array_equal(used, np.sort(used)) and np.array_equal(PG.build_pool(PG.FIRST, shuffle=False)[2][0, :19], np.arange(19))


@pytest.mark.parametrize("case", PG.CASES, ids=PG.case_id)
def test_paged_emulation_stays_inside_the_bounds_and_ignores_the_pages(case):
    """the evidence behind the GPU parity bounds: the paged walk and the combine, in fp32, stay within f32_bound / s16_bound of the float64 y
    and within lse_bound of the float64 lse where it is finite; a row no split has a key for is exactly 0 / -inf; nothing is NaN although the
    pool is; empty partials are 0 / -inf and as many as the mask says; and the walk through the shuffled pool gives, bit for bit, the walk
    over the dense tensors"""
    shape, _, lens, kind, causal, ks = case
    v = PG.logical_inputs(case)[2]
    worst = {}
    for mode in PG.MODES:
        ref, ref_lse = PG.case_reference(case, None if mode == "f32" else mode)
        y, lse, o_part, l2_part = PG.case_emulation(case, mode)
        for a, b in zip(PG.case_emulation(case, mode, paged=True), (y, lse, o_part, l2_part)):
            np.testing.assert_array_equal(a, b)
        assert not any(np.isnan(a).any() for a in (y, lse, o_part, l2_part))
        none = np.isneginf(ref_lse)
        assert int(none.sum()) == PG.all_empty_rows(case)
        assert (y[none] == 0).all() and np.isneginf(lse[none]).all() and np.isfinite(lse[~none]).all() and np.isfinite(y).all()
        by, bl = PG.y_bound(ref, v, mode), PG.lse_bound(ref_lse[~none])
        ey = float(np.abs(y.astype(np.float64) - ref).max())
        el = float(np.abs(lse[~none].astype(np.float64) - ref_lse[~none]).max())
        worst[mode] = (ey / by, el / bl)
        assert ey <= by and el <= bl, (mode, ey, by, el, bl)
        empty = np.isneginf(l2_part)
        assert int(empty.sum()) == PG.empty_partial_rows(case) and (o_part[empty] == 0).all() and np.isfinite(l2_part[~empty]).all()
    print(f"{PG.case_id(case)}: worst error / bound (y, lse) " + ", ".join(f"{m} {a:.3f} {b:.3f}" for m, (a, b) in worst.items()))


def test_emulation_of_equal_lengths_is_the_split_emulation():
    """every sequence at max_kv_len: the paged emulation is flash_attention_splitkv_cases.emulate, bit for bit"""
    shape, kind, causal, ks = (2, 17, 300, 6, 2, 32), "std1", 1, 3
    q, k, v, _ = SK.make_inputs(shape, kind)
    want = SK.emulate(q, k, v, causal, None, ks)
    got = PG.emulate(q, PG.fetch_dense(k, v), (300, 300), 300, 2, causal, None, ks)
    for a, b in zip(got, want):
        np.testing.assert_array_equal(a, b)
