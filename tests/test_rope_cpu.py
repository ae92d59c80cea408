"""brn_rope_forward, brn_kv_cache_append_rope and brn_kv_cache_append_rope_fp8 without a GPU: the symbols and their mirrors exist, the
header states the rule, the clamps, the promise and what is not provided, every refusal of the three entries comes before the device
check under its own prefix (the inherited limits too) and counts bytes, the wrappers refuse what only they can know, and the numpy
statement of the rule (rope_cases.rope_rule) is what it claims to be: within three half-ulps of the exact rotation, a function of the
relative position only in the scores, and the same rotation in both styles up to the permutation between their pairings."""
import os
import re

import numpy as np
import pytest

import kv_cache_cases as KC
import kv_fp8_cases as F8
import rope_cases as RC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROPE, APPEND, APPEND8 = "brn_rope_forward", "brn_kv_cache_append_rope", "brn_kv_cache_append_rope_fp8"
PREFIX = {ROPE: "rope: ", APPEND: "kv cache append rope: ", APPEND8: "kv cache append rope fp8: "}


def _read(*parts):
    return open(os.path.join(ROOT, *parts)).read()


def _comment(header, start, end):
    return " ".join(header[header.index(start):header.index(end)].replace("*", " ").split())


def _sig(header, name):
    return " ".join(re.search(r"\nbrn_status %s\((.*?)\);" % name, header, re.S).group(1).split())


def test_symbols_are_exported_declared_and_mirrored():
    import candle_birefnet_amd as cb
    header, ffi, readme = _read("include", "birefnet_hip.h"), _read("rust_shim", "src", "hip_ffi.rs"), _read("README.md")
    for name in (ROPE, APPEND, APPEND8):
        assert hasattr(cb._ffi.lib, name) and name in cb._ffi.DECLARED
        assert f"\nbrn_status {name}(" in header and f"pub fn {name}(" in ffi and name in readme
    assert re.search(r"typedef enum \{ BRN_ROPE_HALF = 0, BRN_ROPE_INTERLEAVED = 1 \} brn_rope_style;", header)
    assert (cb._ffi.BRN_ROPE_HALF, cb._ffi.BRN_ROPE_INTERLEAVED) == (0, 1) and RC.STYLE_CODE == {"half": 0, "interleaved": 1}
    assert _sig(header, ROPE) == ("const float* x, int batch, int seq, int heads, int head_dim, int layout, const float* cos, const float* sin, int n_pos, int rot_dim, int style, "
                                  "const int* positions, float* y, brn_mem loc, int device_ordinal, void* stream")
    # the table goes in behind layout; everything else is the extended entry's, in its order
    table = "int layout, const float* cos, const float* sin, int n_pos, int rot_dim, int style,"
    assert _sig(header, APPEND) == _sig(header, "brn_kv_cache_append").replace("int layout,", table)
    assert _sig(header, APPEND8) == _sig(header, "brn_kv_cache_append_fp8").replace("int layout,", table)
    assert header.index("\nbrn_status brn_kv_cache_append_fp8(") < header.index(f"\nbrn_status {ROPE}(") < header.index(f"\nbrn_status {APPEND}(") < header.index(f"\nbrn_status {APPEND8}(")
    for fn in ("rope", "rope_table", "kv_cache_append_rope", "kv_cache_append_rope_fp8"):
        assert callable(getattr(cb.ops, fn))
    assert f"{len(cb._ffi.DECLARED)} entry points" in readme
    kernels = _read("candle_birefnet_amd", "csrc", "brn_kernels.h")
    assert "launch_rope" in kernels and "struct RopeParams" in kernels


def test_header_states_the_rule_the_clamps_the_promise_and_what_is_not_provided():
    header = _read("include", "birefnet_hip.h")
    text = _comment(header, "\nbrn_status brn_kv_cache_append_fp8(", f"\nbrn_status {ROPE}(")
    for words in ("[n_pos, rot_dim / 2] fp32, contiguous, supplied by the caller", "evaluates no sine or cosine", "BRN_ROPE_HALF (NeoX / Llama) pairs a = x[i] with b = x[i + rot_dim / 2]",
                  "BRN_ROPE_INTERLEAVED (GPT-J) pairs a = x[2i] with b = x[2i + 1]", "a' = fl(fl(a cos[p][i]) - fl(b sin[p][i]))", "b' = fl(fl(b cos[p][i]) + fl(a sin[p][i]))",
                  "never a fused multiply-add", "d >= rot_dim are copied with their bits", "NULL = all 0", "clamped, never trusted", "P_b = max(positions[b], 0)",
                  "p = min(P_b + t, n_pos - 1)", "without int32 overflow", "reads the last row", "never a read outside the table", "y may be x itself, wholly (in place)",
                  "allocates nothing, does not synchronise the stream and may be captured", '"rope:"', "rot_dim a multiple of 16 with 16 <= rot_dim <= head_dim", "1 <= n_pos <= 2^24",
                  "1 <= seq <= 65536", "batch seq heads head_dim / 8 < 2^31", "sizes in bytes", "16-byte aligned, positions 4-byte aligned"):
        assert words in text, words
    tail = text[text.rindex("Not provided:"):]
    for words in ("computing the table on the device", "per-token position arrays", "rotating q inside the append call", "16-bit x / y", "rotation inside the attention kernels",
                  "a per-sequence seq_new"):
        assert words in tail, words
    text = _comment(header, f"\nbrn_status {ROPE}(", f"\nbrn_status {APPEND}(")
    for words in ("read once, rotated in registers, rounded once and written once", "P_b = L_b, the append's own clamped length", "table row min(L_b + t, n_pos - 1)",
                  "finished in fp32, then cast once", "V is not rotated", "for every pool type", "carry the bits of brn_kv_cache_append called on k' = brn_rope_forward(k_new, positions = kv_lens)",
                  '"kv cache append rope:"', "every limit of brn_kv_cache_append", "overlap neither the pool nor kv_lens_out"):
        assert words in text, words
    assert "rotating q inside the append call" in text[text.rindex("Not provided:"):]
    text = _comment(header, f"\nbrn_status {APPEND}(", f"\nbrn_status {APPEND8}(")
    for words in ("in front of the fp8 store's three steps", "carry the bits of brn_kv_cache_append_fp8 called on k' = brn_rope_forward(k_new, positions = kv_lens)",
                  '"kv cache append rope fp8:"', "every limit of brn_kv_cache_append_fp8", "Not provided:"):
        assert words in text, words
    design = _read("DESIGN.md")
    assert "3.2l" in design and ROPE in design and APPEND in design


@pytest.mark.parametrize("name,args,word", RC.rope_refusals(), ids=[r[0] for r in RC.rope_refusals()])
def test_rope_refusals_come_before_the_device_check(name, args, word):
    import candle_birefnet_amd as cb
    st, msg = RC.raw_rope(cb._ffi.lib, *args)
    assert st == 1 and msg.startswith(PREFIX[ROPE]) and word in msg, (name, st, msg)


@pytest.mark.parametrize("name,args,word", RC.append_rope_refusals(), ids=[r[0] for r in RC.append_rope_refusals()])
def test_append_rope_refusals_come_before_the_device_check(name, args, word):
    """every inherited limit of brn_kv_cache_append under the new prefix, then the table's"""
    import candle_birefnet_amd as cb
    st, msg = RC.raw_append_rope(cb._ffi.lib, *args)
    assert st == 1 and msg.startswith(PREFIX[APPEND]) and word in msg, (name, st, msg)


@pytest.mark.parametrize("name,args,word", RC.append_rope_refusals(True), ids=[r[0] for r in RC.append_rope_refusals(True)])
def test_append_rope_fp8_refusals_come_before_the_device_check(name, args, word):
    import candle_birefnet_amd as cb
    st, msg = RC.raw_append_rope_fp8(cb._ffi.lib, *args)
    assert st == 1 and msg.startswith(PREFIX[APPEND8]) and word in msg, (name, st, msg)


def test_the_refusal_lists_hold_every_inherited_limit():
    assert len(RC.append_rope_refusals()) == len(KC.append_refusals()) + 14 and len(RC.append_rope_refusals(True)) == len(F8.append_refusals()) + 14
    assert [r[0] for r in RC.append_rope_refusals()][:len(KC.append_refusals())] == [r[0] for r in KC.append_refusals()]


def test_overlap_checks_count_bytes_and_in_place_passes():
    """a buffer that starts where another ends, y == x and kv_lens_out == kv_lens pass every check: without a device the call reaches
    the device check, with one it runs"""
    import candle_birefnet_amd as cb
    for name, args in RC.rope_neighbours():
        st, msg = RC.raw_rope(cb._ffi.lib, *args)
        assert st in (0, 4), (name, st, msg)
    for fp8, raw in ((False, RC.raw_append_rope), (True, RC.raw_append_rope_fp8)):
        for name, args in RC.append_rope_neighbours(fp8):
            st, msg = raw(cb._ffi.lib, *args)
            assert st in (0, 4), (name, st, msg)


def test_well_formed_calls_without_a_device_are_loud():
    import candle_birefnet_amd as cb
    if cb.device_count() > 0:
        pytest.skip("a GPU is present")
    for name, args in RC.rope_neighbours():
        st, msg = RC.raw_rope(cb._ffi.lib, *args)
        assert st == 4 and "no CPU fallback" in msg, (name, st, msg)
    for fp8, raw in ((False, RC.raw_append_rope), (True, RC.raw_append_rope_fp8)):
        for name, args in RC.append_rope_neighbours(fp8):
            st, msg = raw(cb._ffi.lib, *args)
            assert st == 4 and "no CPU fallback" in msg, (name, st, msg)


def test_wrappers_refuse_what_only_they_can_know():
    """host inputs: positions or lengths that run past the table, a rot_dim that contradicts the table, a table or out on the wrong
    side or of the wrong shape, an unknown style"""
    import candle_birefnet_amd as cb
    ops = cb.ops
    x = np.array(RC.forward_input("clamped_pages", 32))             # batch 2, seq 20
    cos, sin = RC.table(32)
    with pytest.raises(ValueError, match="runs past the table"):
        ops.rope(x, cos, sin, positions=np.array([3, 21], np.int32))
    with pytest.raises(ValueError, match="runs past the table"):
        ops.rope(x, cos[:19], sin[:19])
    with pytest.raises(ValueError, match="does not agree with the table"):
        ops.rope(x, cos, sin, rot_dim=16)
    with pytest.raises(ValueError, match="expected shape"):
        ops.rope(x, cos, sin[:, :8])
    with pytest.raises(KeyError):
        ops.rope(x, cos, sin, style="neox")
    with pytest.raises(ValueError, match="expected shape"):
        ops.rope(x, cos, sin, positions=np.zeros(3, np.int32))
    with pytest.raises(ValueError, match="out: expected shape"):
        ops.rope(x, cos, sin, out=np.zeros((2, 20, 2, 16), np.float32))
    with pytest.raises(TypeError, match="written in place"):
        ops.rope(x, cos, sin, out=np.zeros(x.shape, np.float64))
    with pytest.raises(TypeError, match="written in place"):
        xd = x.astype(np.float64)                                  # in place needs x itself as fp32: a converted copy would be written instead
        ops.rope(xd, cos, sin, out=xd)
    c = KC.APPEND_CASES["three_pages"]                               # lens (7, 0), seq_new 40: 47 > 40
    k, v = KC.new_tokens("three_pages", 32)
    pools = (KC.sentinel_pool(c, 32, "bf16"), KC.sentinel_pool(c, 32, "bf16"))
    tab, lens = np.array(KC.table_of("three_pages")), np.array(c["lens"], np.int32)
    with pytest.raises(ValueError, match="runs past the table"):
        ops.kv_cache_append_rope(k, v, cos, sin, *pools, tab, lens, kv_dtype="bf16")
    with pytest.raises(ValueError, match="runs past the table"):
        ops.kv_cache_append_rope_fp8(k, v, cos, sin, F8.sentinel_pool(c, 32), F8.sentinel_pool(c, 32), None, None, tab, lens)
    with pytest.raises(ValueError, match="kv_dtype"):
        ops.kv_cache_append_rope(k, v, cos, sin, *pools, tab, lens, kv_dtype="fp8")
    big = RC.table(32, 64)
    with pytest.raises(TypeError, match="kv_dtype"):
        ops.kv_cache_append_rope(k, v, *big, *pools, tab, lens, kv_dtype=None)       # a uint16 pool is not an fp32 pool
    with pytest.raises(ValueError, match="kv_lens must lie in 0 .. max_pages"):
        ops.kv_cache_append_rope(k, v, *big, *pools, tab, np.array([7, 65], np.int32), kv_dtype="bf16")
    if cb.device_count() == 0:
        with pytest.raises(cb.BrnError) as e:
            ops.kv_cache_append_rope(k, v, *big, *pools, tab, lens, kv_dtype="bf16")           # 47 <= 64: passes the wrapper
        assert e.value.status == 4
        with pytest.raises(cb.BrnError) as e:
            ops.rope(x, cos, sin, positions=np.array([3, 20], np.int32), out=x)
        assert e.value.status == 4


def test_rope_table_is_the_cases_table():
    import candle_birefnet_amd as cb
    for rd in (16, 64, 128):
        cos, sin = cb.ops.rope_table(RC.N_POS, rd, RC.THETA)
        want = RC.table(rd)
        assert cos.dtype == np.float32 and cos.shape == (RC.N_POS, rd // 2)
        np.testing.assert_array_equal(cos, want[0])
        np.testing.assert_array_equal(sin, want[1])
    assert (cb.ops.rope_table(3, 16)[0][0] == 1).all() and (cb.ops.rope_table(3, 16)[1][0] == 0).all()


@pytest.mark.parametrize("style,hd,rd", RC.COMBOS, ids=RC.COMBO_IDS)
def test_the_rule_is_within_three_half_ulps_of_the_exact_rotation(style, hd, rd):
    """|rule - exact| <= 3 * 2^-24 * (|a c| + |b s|) per element (two half-ulp products and a half-ulp sum, to first order), on the
    finite, normal-range tokens; the tail keeps its bits; the specials behave as IEEE says"""
    name = "three_pages"
    c = KC.APPEND_CASES[name]
    x = RC.forward_input(name, hd)
    cos, sin = RC.table(rd)
    rows = RC.table_rows((7, 0), c["batch"], c["seq_new"], RC.N_POS)
    got = RC.rope_rule(x, cos, sin, rows, style)
    ia, ib = RC.pair_index(rd, style)
    ea, eb, ma, mb = RC.rope_exact(x, cos, sin, rows, style)
    # where the bound is meant: finite operands whose products are far from the subnormal range and from overflow
    a, b = np.abs(x[..., ia].astype(np.float64)), np.abs(x[..., ib].astype(np.float64))
    ok = np.isfinite(a) & np.isfinite(b) & (np.maximum(a, b) < 1e30) & ((a == 0) | (a > 1e-20)) & ((b == 0) | (b > 1e-20))
    assert ok.mean() > 0.95
    for g, e, m in ((got[..., ia], ea, ma), (got[..., ib], eb, mb)):
        err = np.abs(g.astype(np.float64) - e)
        assert (err[ok] <= 3 * 2.0 ** -24 * m[ok]).all(), float((err[ok] / np.maximum(m[ok], 1e-300)).max() / 2.0 ** -24)
    np.testing.assert_array_equal(got[..., rd:].view(np.uint32), x[..., rd:].view(np.uint32))
    if rd < hd:
        assert got.reshape(-1).view(np.uint32)[-1] == RC.NAN_PAYLOAD
    # row 0 of the table is the identity in value: cos 1, sin 0 (a NaN spreads to its partner through NaN * 0, and the sign of a zero
    # may change: -0 - (-0) is +0)
    first = RC.rope_rule(x[:, :1], cos, sin, np.zeros((c["batch"], 1), np.int64), style)
    same = np.isfinite(first)
    assert (first[same] == x[:, :1][same]).all() and np.isnan(first[~same]).sum() >= np.isnan(x[:, :1]).sum() and np.isinf(first).sum() == 0
    assert np.isnan(got[..., :rd]).sum() >= 2, "the NaN among the tokens spreads to its partner"


@pytest.mark.parametrize("style", RC.STYLES)
def test_scores_depend_on_the_relative_position_only(style):
    """in float64 with an exact table: rot_m(q) . rot_n(k) == rot_{m + d}(q) . rot_{n + d}(k)"""
    rd = 32
    rng = np.random.default_rng(11)
    q, k = rng.standard_normal((1, 1, 4, rd)), rng.standard_normal((1, 1, 4, rd))
    ang = np.arange(64, dtype=np.float64)[:, None] * RC.THETA ** (-np.arange(0, rd, 2, dtype=np.float64) / rd)[None, :]
    cos, sin = np.cos(ang), np.sin(ang)

    def rot(x, p):
        ia, ib = RC.pair_index(rd, style)
        out = x.copy()
        out[..., ia] = x[..., ia] * cos[p] - x[..., ib] * sin[p]
        out[..., ib] = x[..., ib] * cos[p] + x[..., ia] * sin[p]
        return out
    ref = (rot(q, 3) * rot(k, 10)).sum(-1)
    for d in (1, 17, 50):
        np.testing.assert_allclose((rot(q, 3 + d) * rot(k, 10 + d)).sum(-1), ref, rtol=0, atol=1e-12)
    assert np.abs((rot(q, 3) * rot(k, 11)).sum(-1) - ref).max() > 1e-3
    # and the fp32 rule is that rotation
    c32, s32 = cos.astype(np.float32), sin.astype(np.float32)
    got = RC.rope_rule(q.astype(np.float32), c32, s32, np.array([[3]]), style)
    np.testing.assert_allclose(got, rot(q.astype(np.float32).astype(np.float64), 3), rtol=0, atol=1e-5)


@pytest.mark.parametrize("hd,rd", [(hd, rd) for hd in RC.HEAD_DIMS for rd in RC.rot_dims(hd)])
def test_the_two_styles_agree_under_the_permutation_between_their_pairings(hd, rd):
    name = "clamped_pages"
    c = KC.APPEND_CASES[name]
    x = RC.forward_input(name, hd)
    cos, sin = RC.table(rd)
    rows = RC.table_rows((3, 20), c["batch"], c["seq_new"], RC.N_POS)
    half = RC.rope_rule(x, cos, sin, rows, "half")
    inter = RC.rope_rule(RC.half_to_interleaved(x, rd), cos, sin, rows, "interleaved")
    RC.assert_bits(inter, RC.half_to_interleaved(half, rd))
    assert not np.array_equal(half[..., :rd], x[..., :rd], equal_nan=True)


def test_the_rotated_append_rule_keeps_the_append_rule():
    """the expected pools of the GPU tests: KC.append_rule on the rule-rotated K puts, at the keys of each sequence, the rotated tokens;
    V and the lengths are the plain append's"""
    for name in KC.APPEND_CASES:
        c = KC.APPEND_CASES[name]
        k, v = KC.new_tokens(name, 32)
        kr = RC.rotated_k(name, k, 16, "half")
        assert kr.shape == k.shape and np.array_equal(kr[..., 16:].view(np.uint32), k[..., 16:].view(np.uint32))
        table, lens = KC.table_of(name), np.asarray(c["lens"], np.int32)
        kb, lo = KC.append_rule(KC.to_bits(kr, "bf16"), KC.sentinel_pool(c, 32, "bf16"), table, lens)
        _, _, lens_want, _, _ = KC.expected_append(name, 32, "bf16")
        np.testing.assert_array_equal(lo, lens_want)
        for b in range(c["batch"]):
            L = KC.clamp_len(c["lens"][b], KC.cap_of(c))
            for pos in KC.written_positions(c, b):
                page = min(max(int(table[b, pos // c["page"]]), 0), kb.shape[0] - 1)
                want = KC.to_bits(kr[b, pos - L], "bf16")
                nan = np.isnan(kr[b, pos - L])
                np.testing.assert_array_equal(kb[page, pos % c["page"]][~nan], want[~nan])
