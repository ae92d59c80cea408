"""brn_flash_attention_paged_fp8_forward and brn_kv_cache_append_fp8 without a GPU: symbols, signatures, the header's contracts, every
refusal (status 1 under the entry's prefix, before the device check), the calls the byte count must let through, and the two older
entries, which still refuse kv_type 3."""
import os
import re

import numpy as np
import pytest

import flash_attention_paged_cases as PG
import kv_cache_cases as KC
import kv_fp8_cases as F8

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ATTEND, APPEND = "brn_flash_attention_paged_fp8_forward", "brn_kv_cache_append_fp8"


def _header():
    return open(os.path.join(ROOT, "include", "birefnet_hip.h")).read()


def _comment(header, start, end):
    return " ".join(header[header.index(start):header.index(end)].replace("*", " ").split())


def _sig(header, name):
    return " ".join(re.search(r"\nbrn_status %s\((.*?)\);" % name, header, re.S).group(1).split())


def test_symbols_are_exported_declared_and_mirrored():
    import candle_birefnet_amd as cb
    header = _header()
    ffi = open(os.path.join(ROOT, "rust_shim", "src", "hip_ffi.rs")).read()
    readme = open(os.path.join(ROOT, "README.md")).read()
    for name in (ATTEND, APPEND):
        assert hasattr(cb._ffi.lib, name) and name in cb._ffi.DECLARED
        assert f"\nbrn_status {name}(" in header and f"pub fn {name}(" in ffi and name in readme
    assert f"{len(cb._ffi.DECLARED)} entry points" in readme
    assert callable(cb.ops.flash_attention_paged_fp8) and callable(cb.ops.kv_cache_append_fp8)
    # brn_kv_type keeps its three values and its line
    assert re.search(r"typedef enum \{ BRN_KV_F32 = 0, BRN_KV_BF16 = 1, BRN_KV_F16 = 2 \} brn_kv_type;", header)


def test_signatures():
    header = _header()
    paged = _sig(header, "brn_flash_attention_paged_forward")
    assert _sig(header, ATTEND) == paged.replace("const float* k_pages, const float* v_pages,", "const void* k_pages, const void* v_pages, const float* k_scale, const float* v_scale,")
    # the tail after kv_lens is the paged entry's
    assert _sig(header, ATTEND).split("const int* kv_lens, ")[1] == paged.split("const int* kv_lens, ")[1]
    assert _sig(header, APPEND) == ("const float* k_new, const float* v_new, int batch, int seq_new, int kv_heads, int head_dim, int layout, void* k_pages, void* v_pages, "
                                    "const float* k_scale, const float* v_scale, const int* block_table, const int* kv_lens, int* kv_lens_out, int n_pages, int page_size, "
                                    "int max_pages, brn_mem loc, int device_ordinal, void* stream")
    assert _sig(header, APPEND) == _sig(header, "brn_kv_cache_append").replace("int kv_type,", "const float* k_scale, const float* v_scale,")
    assert header.index("\nbrn_status brn_kv_cache_append(") < header.index(f"\nbrn_status {ATTEND}(") < header.index(f"\nbrn_status {APPEND}(")


def test_header_states_the_format_the_scale_rule_the_prefixes_and_what_is_not_provided():
    header = _header()
    text = _comment(header, "\nbrn_status brn_kv_cache_append(", f"\nbrn_status {ATTEND}(")
    for words in ("OCP e4m3fn", "not MI300's fnuz", "bias 7, largest value 448, no infinities, NaN = 0x7F / 0xFF", "one byte per element",
                  "[kv_heads] fp32", "NULL means all ones", "Byte e of K head h stands for k_scale[h] e4m3(e)", "the host never does for BRN_MEM_DEVICE",
                  "may change between graph replays", "no address depends on them", "never causes an access outside the pool",
                  "widened exactly", "scale = fl32(s k_scale[g])", "y carries fl32(v_scale[g] y of that call)", "O_part / lse2_part are not scaled",
                  '"flash attention paged fp8:"', "the two scale arrays 4-byte aligned", "count bytes and include the two scale arrays"):
        assert words in text, words
    not_provided = ("computing scales (amax)", "per-page or per-token scales", "e5m2", "int8", "fp8 q / y", "the fp8 MFMA on the scores")
    tail = text[text.rindex("Not provided:"):]
    for words in not_provided:
        assert words in tail, words
    text = _comment(header, f"\nbrn_status {ATTEND}(", f"\nbrn_status {APPEND}(")
    for words in ("t = x / k_scale[h]", "correctly rounded fp32 division", "clamped to +-448, a NaN kept", "rounded to nearest even into e4m3fn",
                  "+-0 and underflow keep their sign", "a NaN becomes a NaN byte", '"kv cache append fp8:"', "BRN_MEM_HOST stages the whole pool"):
        assert words in text, words
    tail = text[text.rindex("Not provided:"):]
    for words in not_provided[:4]:
        assert words in tail, words


@pytest.mark.parametrize("name,args,word", F8.attend_refusals(), ids=[r[0] for r in F8.attend_refusals()])
def test_attention_refusals_come_before_the_device_check(name, args, word):
    import candle_birefnet_amd as cb
    st, msg = F8.raw_attend(cb._ffi.lib, *args)
    assert st == 1 and msg.startswith("flash attention paged fp8: ") and word in msg, (name, st, msg)


@pytest.mark.parametrize("name,args,word", F8.append_refusals(), ids=[r[0] for r in F8.append_refusals()])
def test_append_refusals_come_before_the_device_check(name, args, word):
    import candle_birefnet_amd as cb
    st, msg = F8.raw_append(cb._ffi.lib, *args)
    assert st == 1 and msg.startswith("kv cache append fp8: ") and word in msg, (name, st, msg)


def test_a_refusal_leaves_the_next_check_alone():
    """after each refusal the well-formed neighbour passes every check: without a device it reaches the device check (status 4, loud:
    no CPU fallback); with one it runs.  So do NULL scales and buffers that start where the one-byte pool ends"""
    import candle_birefnet_amd as cb
    lib = cb._ffi.lib
    good = F8.attend_neighbours()[0][1]
    for name, args, _ in F8.attend_refusals()[::6]:
        assert F8.raw_attend(lib, *args)[0] == 1, name
        st, msg = F8.raw_attend(lib, *good)
        assert st in (0, 4) and (st == 0 or "no CPU fallback" in msg), (name, st, msg)
    for name, args in F8.attend_neighbours():
        st, msg = F8.raw_attend(lib, *args)
        assert st in (0, 4), (name, st, msg)
    good = F8.append_neighbours()[0][1]
    for name, args, _ in F8.append_refusals()[::6]:
        assert F8.raw_append(lib, *args)[0] == 1, name
        st, msg = F8.raw_append(lib, *good)
        assert st in (0, 4) and (st == 0 or "no CPU fallback" in msg), (name, st, msg)
    for name, args in F8.append_neighbours():
        st, msg = F8.raw_append(lib, *args)
        assert st in (0, 4), (name, st, msg)


def test_every_compute_mode_accepts_the_fp8_pool():
    """no pairing restriction: the well-formed call passes every check in f32, bf16 and f16"""
    import candle_birefnet_amd as cb
    from candle_birefnet_amd import ops
    for mode in F8.MODES:
        ops.set_compute(mode)
        try:
            st, msg = F8.raw_attend(cb._ffi.lib, *F8.attend_neighbours()[0][1])
        finally:
            ops.set_compute("f32")
        assert st in (0, 4), (mode, st, msg)


def test_the_two_older_entries_still_refuse_kv_type_3():
    import candle_birefnet_amd as cb
    q, kp, vp, y, lse, ws, table, lens = PG._refusal_buffers()
    st, msg = KC.raw_attend(cb._ffi.lib, q, kp, vp, 3, table, lens, 2, 16, 200, 2, 1, 32, 20, 16, 13, 0, 0, 0.0, 2, y, lse, ws, 4224)
    assert st == 1 and msg == "flash attention paged kv: kv_type 3 unknown (kv_type must be 0 = f32, 1 = bf16 or 2 = f16)", (st, msg)
    kn, vn, kp, vp, table, lens, lo = KC._append_buffers()
    st, msg = KC.raw_append(cb._ffi.lib, kn, vn, 2, 4, 1, 32, 0, kp, vp, 3, table, lens, lo, 20, 16, 13)
    assert st == 1 and msg == "kv cache append: kv_type 3 unknown (kv_type must be 0 = f32, 1 = bf16 or 2 = f16)", (st, msg)


def test_the_wrappers_take_byte_pools_only():
    import torch
    from candle_birefnet_amd import ops
    q = np.zeros((1, 1, 2, 32), np.float32)
    table, lens = np.zeros((1, 1), np.int32), np.array([4], np.int32)
    for bad in (np.zeros((2, 16, 1, 32), np.float32), np.zeros((2, 16, 1, 32), np.uint16), torch.zeros((2, 16, 1, 32), dtype=torch.bfloat16)):
        with pytest.raises(TypeError, match="fp8"):
            ops.flash_attention_paged_fp8(q, bad, bad, None, None, table, lens)
        with pytest.raises(TypeError, match="fp8"):
            ops.kv_cache_append_fp8(np.zeros((1, 1, 1, 32), np.float32), np.zeros((1, 1, 1, 32), np.float32), bad, bad, None, None, table, lens)
    with pytest.raises(ValueError):
        ops.flash_attention_paged_fp8(q, np.zeros((2, 16, 1, 32), np.uint8), np.zeros((2, 16, 1, 32), np.uint8), np.ones(3, np.float32), None, table, lens)
