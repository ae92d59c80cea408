"""brn_flash_attention_splitkv_forward without a GPU: both symbols and their mirrors exist, the header states the promise, the workspace
layout, the limits and what is not provided, the argument checks come before the device check, brn_flash_attention_splitkv_plan keeps
its invariants over every small (tile count, kv_splits), and the numpy emulation of the split walk and the combine
(flash_attention_splitkv_cases.emulate) stays inside the bounds the GPU tests use."""
import os
import re

import numpy as np
import pytest

import flash_attention_gqa_cases as GQ
import flash_attention_splitkv_cases as SK

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FILL_WGS = 512       # FA_SPLIT_FILL_WGS of csrc/brn_flash_split_plan.h: the base grid from which the automatic rule stops splitting


def _header():
    return open(os.path.join(ROOT, "include", "birefnet_hip.h")).read()


def test_symbols_are_exported_declared_and_mirrored():
    import candle_birefnet_amd as cb
    for name in ("brn_flash_attention_splitkv_plan", "brn_flash_attention_splitkv_forward"):
        assert hasattr(cb._ffi.lib, name) and name in cb._ffi.DECLARED
    header = _header()
    assert re.search(r"\nbrn_status brn_flash_attention_splitkv_plan\(int batch, int seq_q, int seq_kv, int heads, int kv_heads, int head_dim,"
                     r"\s+int kv_splits, int\* splits_out, int\* tiles_per_split_out,\s+size_t\* workspace_floats_out\);", header)
    assert re.search(r"\nbrn_status brn_flash_attention_splitkv_forward\(const float\* q, const float\* k, const float\* v,"
                     r"\s+int batch, int seq_q, int seq_kv, int heads, int kv_heads, int head_dim,\s+int layout, int causal, float scale, int kv_splits,"
                     r"\s+float\* y, float\* lse, float\* workspace, size_t workspace_floats,\s+brn_mem loc, int device_ordinal, void\* stream\);", header)
    assert (header.index("\nbrn_status brn_flash_attention_varlen_forward(") < header.index("\nbrn_status brn_flash_attention_splitkv_plan(")
            < header.index("\nbrn_status brn_flash_attention_splitkv_forward("))
    assert callable(cb.ops.flash_attention_splitkv) and callable(cb.ops.flash_attention_splitkv_plan)
    ffi = open(os.path.join(ROOT, "rust_shim", "src", "hip_ffi.rs")).read()
    assert "pub fn brn_flash_attention_splitkv_plan(" in ffi and "pub fn brn_flash_attention_splitkv_forward(" in ffi


def test_header_states_the_promise_the_layout_the_limits_and_what_is_not_provided():
    header = _header()
    text = header[header.index("\nbrn_status brn_flash_attention_varlen_forward("):header.index("\nbrn_status brn_flash_attention_splitkv_plan(")]
    text = " ".join(text.replace("*", " ").split())
    for words in ("no atomics", "fixed order s = 0 .. S - 1", "neither on `batch` nor on the launch grid nor on which rows share its workgroup",
                  "a repeated call repeats its bits", "with S == 1 the result carries the bits of brn_flash_attention_gqa_forward",
                  "allocates nothing and does not synchronise the stream", "pure function of the call's integer arguments",
                  "O_part[s][r][d] at float (s R + r) head_dim + d", "lse2_part[s][r] at float S R head_dim + s R + r", "r = (b heads + h) seq_q + i",
                  "O_part = 0 and lse2_part = -inf", "are not touched",
                  '"flash attention splitkv:"', "0 <= kv_splits <= 1024", "batch kv_heads ceil(G seq_q / 64) S < 2^31", "16-byte aligned",
                  "overlap neither each other nor an input", "the message names the float count needed"):
        assert words in text, words
    tail = text[text.rindex("Not provided:"):]
    for words in ("a bias", "packed or paged K / V", "16-bit tensors at the boundary", "a split for the four older entries"):
        assert words in tail, words


def test_the_older_entries_still_say_they_do_not_split():
    header = _header()
    for a, b in (("brn_flash_attention_bias_forward", "brn_flash_attention_gqa_forward"), ("brn_flash_attention_gqa_forward", "brn_flash_attention_varlen_forward")):
        text = " ".join(header[header.index(f"\nbrn_status {a}("):header.index(f"\nbrn_status {b}(")].replace("*", " ").split())
        assert "a split over keys" in text[text.index("Not provided:"):]


@pytest.mark.parametrize("name,args,word", SK.refusals(), ids=[r[0] for r in SK.refusals()])
def test_refusals_come_before_the_device_check(name, args, word):
    """status 1 with the entry's prefix and a message naming the limit, with or without a device"""
    import candle_birefnet_amd as cb
    st, msg = SK.raw_call(cb._ffi.lib, *args)
    assert st == 1 and msg.startswith("flash attention splitkv: ") and word in msg, (name, st, msg)


def test_plan_refuses_what_the_entry_refuses():
    import candle_birefnet_amd as cb
    for args, word in (((2, 16, 200, 2, 1, 32, -1), "0 <= kv_splits <= 1024"), ((2, 16, 200, 2, 1, 32, 1025), "0 <= kv_splits <= 1024"),
                       ((2, 16, 200, 2, 1, 48, 2), "head_dim must be 32, 64 or 128"), ((2, 16, 200, 6, 4, 32, 2), "heads % kv_heads == 0"),
                       ((2, 16, 65537, 2, 1, 32, 2), "1 <= seq_q, seq_kv <= 65536"), ((32768, 1024, 65536, 64, 64, 32, 1024), "S < 2^31")):
        st, msg, *_ = SK.raw_plan(cb._ffi.lib, *args)
        assert st == 1 and msg.startswith("flash attention splitkv: ") and word in msg, (args, st, msg)


def test_well_formed_call_without_a_device_is_loud():
    import candle_birefnet_amd as cb
    if cb.device_count() > 0:
        pytest.skip("a GPU is present")
    q, k, v, _ = SK.make_inputs((2, 1, 300, 8, 2, 64))
    for layout, ks in (("bhsd", 1), ("bshd", 3), ("bshd", 0)):
        with pytest.raises(cb.BrnError) as e:
            cb.ops.flash_attention_splitkv(*(SK.in_layout(a, layout) for a in (q, k, v)), causal=True, layout=layout, kv_splits=ks, return_lse=True)
        assert e.value.status == 4 and "no CPU fallback" in str(e.value)


def test_plan_invariants_exhaustively():
    """nkt 1 .. 40 x kv_splits 1 .. 40 (seq_kv at both ends of its tile): S <= kv_splits, (S - 1) tps < nkt <= S tps (no empty trailing
    split), S == 1 for kv_splits == 1, the workspace formula; kv_splits 0 returns a value the explicit call accepts and reproduces"""
    import candle_birefnet_amd as cb
    lib = cb._ffi.lib
    batch, seq_q, heads, kv_heads, hd = 3, 2, 6, 2, 64
    R = batch * heads * seq_q
    for nkt in range(1, 41):
        for seq_kv in ((nkt - 1) * 64 + 1, nkt * 64):
            for ks in range(1, 41):
                st, msg, S, tps, n = SK.raw_plan(lib, batch, seq_q, seq_kv, heads, kv_heads, hd, ks)
                assert st == 0, msg
                assert (S, tps) == SK.plan(seq_kv, ks)
                assert 1 <= S <= ks and (S - 1) * tps < nkt <= S * tps
                assert ks != 1 or S == 1
                assert n == S * R * (hd + 1)
                assert SK.raw_plan(lib, batch, seq_q, seq_kv, heads, kv_heads, hd, S)[2:] == (S, tps, n)      # S is a fixed point
            st, msg, S0, tps0, n0 = SK.raw_plan(lib, batch, seq_q, seq_kv, heads, kv_heads, hd, 0)
            assert st == 0 and 1 <= S0 <= 1024 and (S0 - 1) * tps0 < nkt <= S0 * tps0 and n0 == S0 * R * (hd + 1)
            assert SK.raw_plan(lib, batch, seq_q, seq_kv, heads, kv_heads, hd, S0)[2:] == (S0, tps0, n0)


def test_automatic_rule_is_a_function_of_the_integers_and_stops_at_a_full_grid():
    """kv_splits 0: 1 once the base grid batch * kv_heads * ceil(G seq_q / 64) reaches the rule's threshold; below it the grid grows;
    outputs may be NULL"""
    import candle_birefnet_amd as cb
    lib = cb._ffi.lib
    for batch, seq_q, heads, kv_heads in ((FILL_WGS // 8, 1, 32, 8), (FILL_WGS, 1, 8, 1), (1, 64 * FILL_WGS, 1, 1), (4, 8 * FILL_WGS, 32, 8)):
        assert batch * kv_heads * ((heads // kv_heads * seq_q + 63) // 64) >= FILL_WGS
        assert SK.raw_plan(lib, batch, seq_q, 65536, heads, kv_heads, 128, 0)[2] == 1
    first = SK.raw_plan(lib, 1, 1, 32768, 32, 8, 128, 0)
    assert first[0] == 0 and first[2] > 1 and first == SK.raw_plan(lib, 1, 1, 32768, 32, 8, 128, 0)
    assert SK.raw_plan(lib, 1, 1, 64, 32, 8, 128, 0)[2] == 1              # one tile cannot be split
    assert lib.brn_flash_attention_splitkv_plan(1, 1, 4096, 32, 8, 128, 0, None, None, None) == 0


def test_empty_partial_rows_of_the_cases():
    """the three causal cases of the table hold 216, 304 and 2 real partial rows that see no key of their split"""
    assert [SK.empty_rows(c) for c in SK.EMPTY_CASES] == [216, 304, 2]


@pytest.mark.parametrize("case", SK.CASES, ids=SK.case_id)
def test_split_emulation_stays_inside_the_bounds(case):
    """the evidence behind the GPU parity bounds: the split walk and the combine, in fp32, stay within f32_bound / s16_bound of the float64
    y and within 3e-5 max(1, max |lse|) of the float64 lse; the result is finite everywhere; empty partials are 0 / -inf and as many as
    the mask says; with S == 1 the emulation is the one-walk emulation of the gqa cases, bit for bit"""
    shape, kind, causal, ks = case
    q, k, v, _ = SK.make_inputs(shape, kind)
    S, _ = SK.plan(shape[2], ks)
    worst = {}
    for mode in SK.MODES:
        s16 = None if mode == "f32" else mode
        ref, ref_lse = SK.case_reference(shape, kind, causal, s16)
        y, lse, o_part, l2_part = SK.case_emulation(case, mode)
        assert np.isfinite(y).all() and np.isfinite(lse).all() and not np.isnan(o_part).any() and not np.isnan(l2_part).any()
        ey, el = float(np.abs(y.astype(np.float64) - ref).max()), float(np.abs(lse.astype(np.float64) - ref_lse).max())
        by, bl = SK.y_bound(ref, v, mode), SK.lse_bound(ref_lse)
        worst[mode] = (ey / by, el / bl)
        assert ey <= by and el <= bl, (mode, ey, by, el, bl)
        empty = np.isneginf(l2_part)
        assert int(empty.sum()) == SK.empty_rows(case) and (o_part[empty] == 0).all() and np.isfinite(l2_part[~empty]).all()
        assert not empty[0].any()                                             # split 0 holds key 0, which every row sees
        if S == 1:
            qq, kk, vv = ((SK.round_s16(a, s16) for a in (q, k, v)) if s16 else (q, k, v))
            one = GQ.emulate(qq, kk, vv, None, causal, SK.kind_scale(kind), s16)
            assert np.array_equal(y, one)
    print(f"{SK.case_id(case)}: worst error / bound (y, lse) " + ", ".join(f"{m} {a:.3f} {b:.3f}" for m, (a, b) in worst.items()))


def test_kv_splits_1_emulation_is_the_gqa_emulation():
    """S == 1 by request, causal over a cache: the bits of the one-walk emulation"""
    shape = (2, 17, 300, 6, 2, 32)
    q, k, v, _ = SK.make_inputs(shape)
    for s16 in (None, "bf16"):
        qq, kk, vv = ((SK.round_s16(a, s16) for a in (q, k, v)) if s16 else (q, k, v))
        y, lse, _, l2 = SK.emulate(qq, kk, vv, 1, None, 1, s16)
        assert np.array_equal(y, GQ.emulate(qq, kk, vv, None, 1, None, s16)) and np.isfinite(l2).all()
        assert float(np.abs(lse - SK.reference_lse(qq, kk, True)).max()) <= SK.lse_bound(SK.reference_lse(qq, kk, True))


def test_combine64_of_exact_partials_is_the_reference():
    """what GPU test 3 leans on, in float64: exact partials over the splits' keys, merged by combine64, are the whole-row softmax"""
    shape = (1, 2, 65, 2, 1, 128)
    q, k, v, _ = SK.make_inputs(shape)
    ref, ref_lse = SK.case_reference(shape, "std1", 1)
    q64, k64, v64 = (np.asarray(a, np.float64) for a in (q, k, v))
    s = (q64 @ k64[:, [0, 0]].transpose(0, 1, 3, 2)) * 128 ** -0.5
    s = np.where(GQ.visible(2, 65), s, -np.inf)
    o_part, l2 = [], []
    for keys in (slice(0, 64), slice(64, 65)):
        with np.errstate(invalid="ignore", divide="ignore"):
            mx = s[..., keys].max(-1, keepdims=True)
            p = np.where(np.isneginf(mx), 0.0, np.exp(s[..., keys] - np.where(np.isneginf(mx), 0.0, mx)))
            l = p.sum(-1, keepdims=True)
            o_part.append(np.where(l > 0, (p @ v64[:, [0, 0]][:, :, keys]) / np.where(l > 0, l, 1.0), 0.0).reshape(-1, 128))
            l2.append(np.where(l > 0, (mx + np.log(np.where(l > 0, l, 1.0))) / np.log(2.0), -np.inf).reshape(-1))
    y, lse = SK.combine64(np.stack(o_part), np.stack(l2))
    np.testing.assert_allclose(y.reshape(ref.shape), ref, rtol=0, atol=1e-12)
    np.testing.assert_allclose(lse.reshape(ref_lse.shape), ref_lse, rtol=0, atol=1e-12)
