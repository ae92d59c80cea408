"""brn_flash_attention_gqa_forward without a GPU: the symbol and its mirrors exist, the argument checks come before the device check, the
packed-row map of the kernels (restated in numpy, flash_attention_gqa_cases.row_map) owns every (query, head) once and walks every visible
key, and the emulation of the tile walk with that map stays inside the bounds the GPU tests use."""
import itertools
import os
import re

import numpy as np
import pytest

import flash_attention_cases as A
import flash_attention_gqa_cases as GQ

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_symbol_is_exported_declared_and_mirrored():
    import candle_birefnet_amd as cb
    assert hasattr(cb._ffi.lib, "brn_flash_attention_gqa_forward") and "brn_flash_attention_gqa_forward" in cb._ffi.DECLARED
    header = open(os.path.join(ROOT, "include", "birefnet_hip.h")).read()
    assert re.search(r"\nbrn_status brn_flash_attention_gqa_forward\(const float\* q, const float\* k, const float\* v,"
                     r"\s+int batch, int seq_q, int seq_kv, int heads, int kv_heads, int head_dim,\s+int layout, int causal,"
                     r"\s+const float\* bias, int n_bias, float scale,\s+float\* y, brn_mem loc, int device_ordinal, void\* stream\);", header)
    assert header.index("\nbrn_status brn_flash_attention_bias_forward(") < header.index("\nbrn_status brn_flash_attention_gqa_forward(")
    assert callable(cb.ops.flash_attention_gqa)
    ffi = open(os.path.join(ROOT, "rust_shim", "src", "hip_ffi.rs")).read()
    assert "pub fn brn_flash_attention_gqa_forward(" in ffi


def test_header_states_what_is_not_provided():
    header = open(os.path.join(ROOT, "include", "birefnet_hip.h")).read()
    text = header[header.index("\nbrn_status brn_flash_attention_bias_forward("):header.index("\nbrn_status brn_flash_attention_gqa_forward(")]
    text = " ".join(text.replace("*", " ").split())
    tail = text[text.index("Not provided:"):]
    for words in ("a split over keys", "sliding-window masks", "variable-length batches", "16-bit tensors at the boundary"):
        assert words in tail, words
    for words in ('"flash attention gqa:"', "causal requires seq_kv >= seq_q", "heads % kv_heads == 0", "batch kv_heads ceil(G seq_q / 64) < 2^31"):
        assert words in text, words


@pytest.mark.parametrize("name,args,word", GQ.refusals(), ids=[r[0] for r in GQ.refusals()])
def test_refusals_come_before_the_device_check(name, args, word):
    """status 1 with the entry's prefix and a message naming the limit, with or without a device"""
    import candle_birefnet_amd as cb
    st, msg = GQ.raw_call(cb._ffi.lib, *args)
    assert st == 1 and msg.startswith("flash attention gqa: ") and word in msg, (name, st, msg)


def test_the_older_entries_keep_their_causal_refusal():
    """a causal call over a cache is still refused by the two older entries, in their own words"""
    import candle_birefnet_amd as cb
    import flash_attention_bias_cases as FB
    for mod in (A, FB):
        name, args, word = next(r for r in mod.refusals() if r[0] == "causal, seq_q != seq_kv")
        st, msg = mod.raw_call(cb._ffi.lib, *args)
        assert st == 1 and "causal requires seq_q == seq_kv" in msg, (st, msg)


def test_well_formed_call_without_a_device_is_loud():
    import candle_birefnet_amd as cb
    if cb.device_count() > 0:
        pytest.skip("a GPU is present")
    q, k, v, bias = GQ.make_inputs((2, 17, 300, 6, 2, 32))
    for layout, b in (("bhsd", None), ("bshd", bias)):
        with pytest.raises(cb.BrnError) as e:
            cb.ops.flash_attention_gqa(*(GQ.in_layout(a, layout) for a in (q, k, v)), causal=True, layout=layout, bias=b)
        assert e.value.status == 4 and "no CPU fallback" in str(e.value)


SMALL_G = (1, 2, 3, 5, 8, 16, 63, 64, 65, 80, 130)
SMALL_SQ = (1, 2, 3, 7, 16, 21, 22, 33, 64, 65, 100)


@pytest.mark.parametrize("causal", [0, 1])
def test_row_map_owns_every_row_once_and_walks_every_visible_key(causal):
    """exhaustively over small (G, seq_q, seq_kv - seq_q): every real (query, head) belongs to exactly one non-pad row of one tile; a pad
    row repeats the last real row; the tile's nkt K / V tiles reach every visible key of every row (and no tile is walked that no row of
    the workgroup can see, under the causal mask); a wave whose mask flag is off for a K / V tile has no lane with an excluded key in it"""
    for G, seq_q, extra in itertools.product(SMALL_G, SMALL_SQ, (0, 1, 63, 64, 65, 130)):
        seq_kv = seq_q + extra
        tiles = GQ.row_map(G, seq_q, seq_kv, causal)
        assert len(tiles) == (G * seq_q + GQ.BQ - 1) // GQ.BQ
        owned = np.zeros((seq_q, G), int)
        for t in tiles:
            real = ~t["pad"]
            np.add.at(owned, (t["query"][real], t["head"][real]), 1)
            assert real[0] and (t["query"] < seq_q).all() and (t["head"] < G).all()
            last = np.flatnonzero(real)[-1]
            assert (t["query"][~real] == t["query"][last]).all() and (t["head"][~real] == t["head"][last]).all()
            assert (np.diff(t["query"]) >= 0).all()                           # query-major: the limit does not fall along a tile
            want = GQ.visible(seq_q, seq_kv)[t["query"]].sum(-1) if causal else np.full(GQ.BQ, seq_kv)
            assert (t["limit"] == want).all() and (t["limit"] >= 1).all()     # key 0 is visible to every row
            assert t["nkt"] == (int(t["limit"].max()) + GQ.T - 1) // GQ.T     # reaches the last visible key, walks no tile beyond it
            for w in range(4):
                lim = t["limit"][16 * w:16 * w + 16]
                assert t["wave_lim"][w] == lim.min()
                for kt in range(t["nkt"]):
                    flagged = kt * GQ.T + GQ.T > t["wave_lim"][w]
                    assert flagged or (lim >= kt * GQ.T + GQ.T).all()
        assert (owned == 1).all(), (G, seq_q, seq_kv)


def test_causal_tiles_are_tight():
    """query-major packing: the rows of a tile span at most ceil(64 / G) + 1 queries, so its limits differ by no more than that"""
    for G, seq_q in itertools.product(SMALL_G, SMALL_SQ):
        for t in GQ.row_map(G, seq_q, seq_q + 70, 1):
            assert int(t["limit"].max() - t["limit"].min()) <= (GQ.BQ + G - 1) // G


@pytest.mark.parametrize("case", GQ.PARITY, ids=GQ.parity_id)
def test_packed_emulation_stays_inside_the_bounds(case):
    """the evidence behind the GPU parity bounds for the grouped cases: the kernels' walk over the packed rows, in fp32, stays within
    3e-5 max(1, max |ref|) of the float64 reference, and within u max |v| + that in the 16-bit types, with and without a bias"""
    shape, kind, causal = case
    q, k, v, bias = GQ.make_inputs(shape, kind)
    vmax = float(np.abs(v).max())
    worst = {}
    for s16 in (None, "bf16", "f16"):
        qq, kk, vv = ((GQ.round_s16(a, s16) for a in (q, k, v)) if s16 else (q, k, v))
        for with_bias in (False, True):
            ref = GQ.case_reference(shape, kind, causal, s16, with_bias)
            bound = GQ.s16_bound(ref, v, s16) if s16 else GQ.f32_bound(ref)
            y = GQ.emulate(qq, kk, vv, bias if with_bias else None, causal, GQ.kind_scale(kind), s16)
            err = float(np.abs(y.astype(np.float64) - ref).max())
            worst[s16 or "f32"] = max(worst.get(s16 or "f32", 0.0), err / bound)
            assert np.isfinite(y).all() and err <= bound, (s16, with_bias, err, bound, vmax)
    print(f"{GQ.parity_id(case)}: worst error / bound " + ", ".join(f"{k_} {w:.3f}" for k_, w in worst.items()))


def test_mask_bias_reference_is_the_causal_reference():
    """what the GPU test of the cached causal mask leans on, in float64: the older entries' reference on repeated K / V with the mask as a
    -inf bias is the grouped, bottom-right causal reference"""
    import flash_attention_bias_cases as FB
    for shape in GQ.CACHE_SHAPES:
        q, k, v, bias = GQ.make_inputs(shape)
        G = shape[3] // shape[4]
        for b in (None, bias):
            old = FB.reference(q, GQ.repeat_kv(k, G), GQ.repeat_kv(v, G), GQ.mask_bias(shape, b))
            np.testing.assert_allclose(old, GQ.reference(q, k, v, b, True), rtol=0, atol=1e-12)


def test_integer_kinds_are_exact_in_16_bits():
    for shape, kind, _ in GQ.PARITY:
        if not kind.startswith("std"):
            q, k, _, bias = GQ.make_inputs(shape, kind)
            for s16 in ("bf16", "f16"):
                assert np.array_equal(GQ.round_s16(q, s16), q) and np.array_equal(GQ.round_s16(k, s16), k)
