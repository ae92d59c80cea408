"""brn_flash_attention_paged_varlen_plan / _forward and brn_kv_cache_append_varlen without a GPU: the symbols and their mirrors exist,
the header states the clamp rule, the padding rule, the promise and the limits, every refusal comes before the device check under its
prefix, a well-formed call without a device is loud, the plan function equals its numpy restatement (T_max bounds every pack), and the
HIP-free plan header, compiled alone under the address and undefined-behaviour sanitizers, prints the starts and tiles the numpy
restatement predicts for well-formed and for garbage cu_seqlens_q."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import flash_attention_paged_varlen_cases as PV

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "candle_birefnet_amd", "csrc")
PLAN, ATTEND, APPEND = "brn_flash_attention_paged_varlen_plan", "brn_flash_attention_paged_varlen_forward", "brn_kv_cache_append_varlen"


def _header():
    return open(os.path.join(ROOT, "include", "birefnet_hip.h")).read()


def _comment(header, start, end):
    return " ".join(header[header.index(start):header.index(end)].replace("*", " ").split())


def test_symbols_are_exported_declared_and_mirrored():
    import candle_birefnet_amd as cb
    header = _header()
    ffi = open(os.path.join(ROOT, "rust_shim", "src", "hip_ffi.rs")).read()
    readme = open(os.path.join(ROOT, "README.md")).read()
    for name in (PLAN, ATTEND, APPEND):
        assert hasattr(cb._ffi.lib, name) and name in cb._ffi.DECLARED
        assert f"\nbrn_status {name}(" in header and f"pub fn {name}(" in ffi and name in readme
    assert f"{len(cb._ffi.DECLARED)} entry points" in readme
    # directly behind brn_kv_cache_append_rope_fp8, in the issue's order
    order = [header.index(f"\nbrn_status {n}(") for n in ("brn_kv_cache_append_rope_fp8", PLAN, ATTEND, APPEND, "brn_patch_merging_forward")]
    assert order == sorted(order)
    assert re.search(r"typedef enum \{ BRN_POOL_F32 = 0, BRN_POOL_BF16 = 1, BRN_POOL_F16 = 2, BRN_POOL_E4M3 = 3 \} brn_pool_type;", header)
    assert re.search(r"typedef enum \{ BRN_KV_F32 = 0, BRN_KV_BF16 = 1, BRN_KV_F16 = 2 \} brn_kv_type;", header), "brn_kv_type keeps its three values"
    assert (cb._ffi.BRN_POOL_F32, cb._ffi.BRN_POOL_BF16, cb._ffi.BRN_POOL_F16, cb._ffi.BRN_POOL_E4M3) == (0, 1, 2, 3)
    assert re.search(r"\nbrn_status brn_flash_attention_paged_varlen_forward\(const float\* q, const void\* k_pages, const void\* v_pages, int pool_type,"
                     r"\s+const float\* k_scale, const float\* v_scale,"
                     r"\s+const int\* block_table, const int\* kv_lens, const int\* cu_seqlens_q,"
                     r"\s+int total_q, int n_seqs, int max_kv_len, int heads, int kv_heads, int head_dim,"
                     r"\s+int n_pages, int page_size, int max_pages,"
                     r"\s+int causal, float scale, int kv_splits,"
                     r"\s+float\* y, float\* lse, float\* workspace, size_t workspace_floats,"
                     r"\s+int\* plan_workspace, size_t plan_ints,"
                     r"\s+brn_mem loc, int device_ordinal, void\* stream\);", header)
    assert re.search(r"\nbrn_status brn_kv_cache_append_varlen\(const float\* k_new, const float\* v_new, const int\* cu_seqlens_q, int total_q, int n_seqs,"
                     r"\s+int kv_heads, int head_dim, void\* k_pages, void\* v_pages, int pool_type,"
                     r"\s+const float\* k_scale, const float\* v_scale,"
                     r"\s+const int\* block_table, const int\* kv_lens, int\* kv_lens_out,"
                     r"\s+int n_pages, int page_size, int max_pages,"
                     r"\s+int\* plan_workspace, size_t plan_ints,"
                     r"\s+brn_mem loc, int device_ordinal, void\* stream\);", header)
    assert re.search(r"\nbrn_status brn_flash_attention_paged_varlen_plan\(int total_q, int n_seqs, int max_kv_len, int heads, int kv_heads, int head_dim, int kv_splits,"
                     r"\s+int\* splits_out, int\* tiles_per_split_out, size_t\* workspace_floats_out, size_t\* plan_ints_out\);", header)
    for fn in ("flash_attention_paged_varlen", "flash_attention_paged_varlen_plan", "kv_cache_append_varlen"):
        assert callable(getattr(cb.ops, fn))


def test_header_states_the_plan_the_clamp_rule_the_padding_rule_the_promise_and_the_limits():
    header = _header()
    plan = _comment(header, "\nbrn_status brn_kv_cache_append_rope_fp8(", f"\nbrn_status {PLAN}(")
    for words in ("host-only, a pure function of its integers", "T_max = (G total_q + 63 min(n_seqs, total_q)) / 64", "sum_b ceil(G n_b / 64) <= T_max",
                  "nkt = ceil(max_kv_len / 64)", "workspace_floats = S R (head_dim + 1), R = heads total_q", "its inner layout is not part of the contract"):
        assert words in plan, words
    text = _comment(header, f"\nbrn_status {PLAN}(", f"\nbrn_status {ATTEND}(")
    for words in ("[total_q, heads, head_dim] fp32", "lse: [heads, total_q] fp32 or NULL, heads-major", "k_scale and v_scale must be NULL unless pool_type is BRN_POOL_E4M3",
                  "total_q is a capacity", "never read by the host for BRN_MEM_DEVICE",
                  "c_i = min(max(cu_seqlens_q[i], 0), total_q)", "s_b is the running maximum of c_i over i <= b", "n_b = s_{b+1} - s_b",
                  "disjoint and ordered whatever the array holds",
                  "tokens outside [s_0, s_{n_seqs}) are padding", "not written by any kernel of the call, the combine included",
                  "len_b = min(max(kv_lens[b], 0), max_kv_len)", "j <= i + len_b - n_b", "y = 0 (exact zeros) and lse = -inf",
                  "A sequence with n_b == 0 costs nothing, and no table entry of it is read",
                  "r = h total_q + token", "S == 1 touches no float workspace", "No atomics; the combine order is s = 0 .. S - 1",
                  "carry the bits of brn_flash_attention_paged_forward / _kv_forward / _fp8_forward in the same compute mode",
                  "batch = 1, seq_q = n_b, that sequence's table row and length, the same max_kv_len and the same explicit kv_splits",
                  "none of the other sequences, neither on n_seqs nor on total_q, on no physical page and on no old workspace content",
                  "allocates nothing, does not synchronise the stream and may be captured",
                  "changing cu_seqlens_q, kv_lens, the table and the pool between replays is the intended use",
                  '"flash attention paged varlen:"', "1 <= n_seqs <= 65536", "total_q >= 1", "G total_q < 2^31",
                  "plan_workspace present, 4-byte aligned and of at least plan_ints ints (the message names the count)", "sizes in bytes"):
        assert words in text, words
    tail = text[text.rindex("Not provided:"):]
    for words in ("a window or a bias", "fused rope", "the BHSD layout", "16-bit q / y", "copy-on-write of shared pages"):
        assert words in tail, words
    text = _comment(header, f"\nbrn_status {ATTEND}(", f"\nbrn_status {APPEND}(")
    for words in ("[total_q, kv_heads, head_dim] fp32", "running maximum of the values clamped to 0 .. total_q", "becomes key L_b + t by the position rule of brn_kv_cache_append",
                  "kv_lens_out[b] = min(L_b + n_b, cap), written by a later launch, so kv_lens_out may be kv_lens itself", "Padding tokens write nothing",
                  "carry the bits of the existing append entry of that pool type called per sequence with batch = 1, seq_new = n_b",
                  "No rope is fused", "brn_rope_forward with batch = total_q, seq = 1 and a per-token positions array", "on q and on k_new, then this append",
                  '"kv cache append varlen:"', "1 <= n_seqs <= 65536", "total_q >= 1", "plan_workspace present, 4-byte aligned and of at least plan_ints ints"):
        assert words in text, words
    tail = text[text.rindex("Not provided:"):]
    for words in ("a window or a bias", "fused rope", "the BHSD layout", "copy-on-write of shared pages"):
        assert words in tail, words


def test_older_entries_keep_refusing_pool_type_3():
    """brn_pool_type is a new enum: the kv entries refuse 3 with their present message"""
    import candle_birefnet_amd as cb
    import flash_attention_paged_cases as PG
    import kv_cache_cases as KC
    q, kp, vp, y, lse, ws, table, lens = PG._refusal_buffers()
    st, msg = KC.raw_attend(cb._ffi.lib, q, kp, vp, 3, table, lens, 2, 16, 200, 2, 1, 32, 20, 16, 13, 0, 0, 0.0, 2, y, lse, ws, 4224)
    assert st == 1 and "kv_type 3 unknown (kv_type must be 0 = f32, 1 = bf16 or 2 = f16)" in msg, msg


@pytest.mark.parametrize("name,args,word", PV.attend_refusals(), ids=[r[0] for r in PV.attend_refusals()])
def test_attention_refusals_come_before_the_device_check(name, args, word):
    import candle_birefnet_amd as cb
    st, msg = PV.raw_attend(cb._ffi.lib, *args)
    assert st == 1 and msg.startswith("flash attention paged varlen: ") and word in msg, (name, st, msg)


@pytest.mark.parametrize("name,args,word", PV.append_refusals(), ids=[r[0] for r in PV.append_refusals()])
def test_append_refusals_come_before_the_device_check(name, args, word):
    import candle_birefnet_amd as cb
    st, msg = PV.raw_append(cb._ffi.lib, *args)
    assert st == 1 and msg.startswith("kv cache append varlen: ") and word in msg, (name, st, msg)


def test_pairing_of_pool_and_compute_mode_is_the_kv_entrys():
    """a 16-bit mode reads a 16-bit pool of its own type alone; fp32 and e4m3 pools go with every mode"""
    import candle_birefnet_amd as cb
    args = list(PV.attend_neighbour())
    for mode, pool_type, ok in (("bf16", 2, False), ("f16", 1, False), ("bf16", 1, True), ("f16", 2, True), ("f32", 1, True), ("f32", 2, True), ("bf16", 0, True),
                                ("f16", 3, True), ("f32_split3", 2, True)):
        args[3] = pool_type
        cb.ops.set_compute(mode)
        try:
            st, msg = PV.raw_attend(cb._ffi.lib, *args)
        finally:
            cb.ops.set_compute("f32")
        if not ok:
            assert st == 1 and msg.startswith("flash attention paged varlen: pool_type ") and "cannot be read in compute mode" in msg, (mode, pool_type, st, msg)
        else:
            assert not (st == 1 and "cannot be read" in msg), (mode, pool_type, st, msg)


def test_well_formed_calls_without_a_device_are_loud():
    """the neighbours of the refusals, and the byte-counted neighbours of the narrow pools, reach the device check"""
    import candle_birefnet_amd as cb
    if cb.device_count() > 0:
        pytest.skip("a GPU is present")
    for args in [PV.attend_neighbour()] + [a for _, a in PV.attend_byte_counted_neighbours()]:
        st, msg = PV.raw_attend(cb._ffi.lib, *args)
        assert st == 4 and "no CPU fallback" in msg, (st, msg)
    st, msg = PV.raw_append(cb._ffi.lib, *PV.append_neighbour())
    assert st == 4 and "no CPU fallback" in msg, (st, msg)
    # the in-place lengths form is well formed
    args = list(PV.append_neighbour())
    args[14] = args[13]
    st, msg = PV.raw_append(cb._ffi.lib, *args)
    assert st == 4 and "no CPU fallback" in msg, (st, msg)
    cfg = PV.CONFIGS[0]
    kp, vp, table, lens = PV.build_pool(cfg, PV.PACK, 16)
    cu = PV.cu_of(PV.PACK)
    with pytest.raises(cb.BrnError) as e:
        cb.ops.flash_attention_paged_varlen(PV.packed_q(cfg, PV.PACK, cu, PV.TOTAL_Q), kp, vp, table, lens, cu, max_kv_len=PV.MAX_KV, causal=True, kv_splits=3)
    assert e.value.status == 4 and "no CPU fallback" in str(e.value)


def test_plan_function_equals_the_numpy_restatement():
    import candle_birefnet_amd as cb
    rng = np.random.default_rng(3)
    problems = [(64, 6, 256, 4, 1, 64, ks) for ks in (0, 1, 3, 4, 1024)] + [(1, 1, 1, 1, 1, 32, 0), (543, 32, 4096, 32, 8, 128, 0), (32, 32, 4096, 32, 8, 128, 0),
                                                                            (5, 65536, 65536, 8, 8, 32, 0), (2 ** 20, 7, 65536, 128, 1, 128, 0)]
    for _ in range(200):
        kv_heads = int(rng.integers(1, 9))
        problems.append((int(rng.integers(1, 5000)), int(rng.integers(1, 300)), int(rng.integers(1, 65537)), kv_heads * int(rng.integers(1, 17)), kv_heads,
                         int(rng.choice([32, 64, 128])), int(rng.choice([0, 0, 1, 2, 3, 7, 64]))))
    for p in problems:
        st, msg, got = PV.raw_plan(cb._ffi.lib, *p)
        assert st == 0, (p, msg)
        assert got == PV.host_plan(*p), (p, got, PV.host_plan(*p))
        assert got == cb.ops.flash_attention_paged_varlen_plan(*p)
    # with kv_splits given, tps depends on max_kv_len and kv_splits alone
    assert len({PV.raw_plan(cb._ffi.lib, tq, n, 4096, 8, 2, 64, 5)[2][:2] for tq, n in ((1, 1), (64, 6), (5000, 300))}) == 1
    # the plan's refusals carry the attention entry's prefix
    st, msg, _ = PV.raw_plan(cb._ffi.lib, 64, 0, 256, 4, 1, 64, 0)
    assert st == 1 and msg.startswith("flash attention paged varlen: ") and "1 <= n_seqs <= 65536" in msg


def test_t_max_bounds_the_row_tiles_of_random_packs():
    """T_max >= sum_b ceil(G n_b / 64) for every pack of at most total_q tokens in n_seqs sequences, and is attained"""
    rng = np.random.default_rng(11)
    attained = False
    for _ in range(3000):
        G, n_seqs, total_q = int(rng.choice([1, 2, 3, 4, 8, 16, 80])), int(rng.integers(1, 40)), int(rng.integers(1, 400))
        cuts = np.sort(rng.integers(0, total_q + 1, n_seqs + 1))
        if rng.random() < 0.3:                                  # many sequences of one token: the worst rounding
            cuts = np.minimum(np.arange(n_seqs + 1), total_q)
        tiles = int(PV.tiles_of(cuts, G).sum())
        assert tiles <= PV.t_max(G, total_q, n_seqs), (G, n_seqs, total_q, cuts)
        attained |= tiles == PV.t_max(G, total_q, n_seqs)
    assert attained
    assert int(PV.tiles_of(PV.clamp_starts(PV.cu_of(PV.PACK), PV.TOTAL_Q), 4).sum()) == 8 <= PV.t_max(4, PV.TOTAL_Q, len(PV.PACK))


def _plan_problems():
    """(total_q, G, cu): the pack of the GPU tests in both places, permuted, and garbage: negative, decreasing, beyond total_q, all equal"""
    out = [(PV.TOTAL_Q, G, PV.cu_of(PV.PACK, s).tolist()) for G in (1, 4) for s in PV.CU0]
    out += [(PV.TOTAL_Q, 4, PV.cu_of(PV.PACK[::-1]).tolist()), (59, 1, PV.cu_of(PV.PACK).tolist()), (1, 1, [0, 1]), (1, 80, [0, 0, 0, 1, 1])]
    out += [(64, 4, [-7, 1, -3, 18, 5, 56, 10 ** 9]), (64, 2, [70, 3, 2, 1, 0]), (64, 3, [-2 ** 31, 2 ** 31 - 1]), (64, 1, [5, 5, 5, 5]), (10, 16, [9, 3, 10, 2, 11, -1]),
            (2 ** 20, 2047, [0, 2 ** 20, 5]), (300, 4, [0] + [-1] * 40 + [300])]
    rng = np.random.default_rng(5)
    for _ in range(40):
        n = int(rng.integers(1, 700))
        total_q = int(rng.integers(1, 2000))
        out.append((total_q, int(rng.integers(1, 20)), rng.integers(-50, total_q + 50, n + 1).tolist()))
    out.append((70000, 1, np.minimum(np.arange(65537), 70000).tolist()))             # the most sequences the entries accept
    return out


def test_plan_header_alone_under_the_sanitizers_prints_the_numpy_restatement(tmp_path):
    """brn_flash_paged_varlen_plan.h includes nothing of HIP: a stand-alone program of the host compiler, built with
    -fsanitize=address,undefined, prints starts and tile prefix as plan_ref predicts, for well-formed arrays and for garbage"""
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "paged_varlen_plan")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", CSRC,
                           os.path.join(ROOT, "tests", "flash_paged_varlen_plan_main.cpp"), "-o", exe])
    problems = _plan_problems()
    text = "\n".join(f"{tq} {G} {len(cu) - 1} " + " ".join(str(c) for c in cu) for tq, G, cu in problems) + "\n"
    r = subprocess.run([exe], input=text, stdout=subprocess.PIPE, stderr=subprocess.PIPE, universal_newlines=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    lines = r.stdout.splitlines()
    assert len(lines) == len(problems)
    for (tq, G, cu), line in zip(problems, lines):
        got = [int(v) for v in line.split()]
        n = len(cu) - 1
        want = PV.plan_ref(cu, tq, G)
        assert got[:-2] == want.tolist(), (tq, G, cu[:8])
        assert got[-2] == PV.t_max(G, tq, n) >= want[-1] and got[-1] == 2 * (n + 1)
        s = want[:n + 1]
        assert (np.diff(s) >= 0).all() and s[0] >= 0 and s[-1] <= tq, "the sequences are disjoint and ordered, inside the pack"


def test_the_pack_is_what_the_issue_names():
    cu = PV.cu_of(PV.PACK)
    assert cu.tolist() == [0, 1, 1, 18, 23, 56, 59] and PV.TOTAL_Q - cu[-1] == 5 and PV.cu_of(PV.PACK, 2)[-1] <= PV.TOTAL_Q
    assert PV.host_plan(PV.TOTAL_Q, 6, PV.MAX_KV, 4, 1, 64, 3)[:2] == (2, 2) and PV.host_plan(PV.TOTAL_Q, 6, PV.MAX_KV, 4, 1, 64, 1)[:2] == (1, 4)
    # the first causal row of the last sequence sees no key; no other row of the pack is empty
    import flash_attention_paged_cases as PG
    assert [int((PG.row_limits(n, L, 1) <= 0).sum()) for n, L in PV.PACK] == [0, 0, 0, 0, 0, 1]
    for cfg in PV.CONFIGS:
        for page in PV.PAGES:
            kp, vp, table, lens = PV.build_pool(cfg, PV.PACK, page)
            for b, (n, L) in enumerate(PV.PACK):
                _, k, v = PV.sequence(cfg, n, L)
                keys = np.arange(L)
                np.testing.assert_array_equal(kp[table[b, keys // page], keys % page], k)
                np.testing.assert_array_equal(vp[table[b, keys // page], keys % page], v)
                assert np.isnan(kp[table[b, (L + page - 1) // page:]]).all()
            assert int(np.isfinite(kp).sum()) == sum(L for _, L in PV.PACK) * cfg[1] * cfg[2]
