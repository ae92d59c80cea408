"""brn_flash_attention_varlen_forward without a GPU: the symbol and its mirrors exist, the argument checks come before the device check,
the host-only plan header (csrc/brn_flash_varlen_plan.h), compiled alone under the host sanitizers, prints the records its numpy
restatement (flash_attention_varlen_cases.plan) gives, those records own every (sequence, query, head) once and walk exactly the visible
keys, and the emulation of the walk stays inside the bounds the GPU tests use and equals the walk from tile 0 with the window as a -inf
bias."""
import itertools
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import flash_attention_bias_cases as FB
import flash_attention_gqa_cases as GQ
import flash_attention_varlen_cases as VL

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "candle_birefnet_amd", "csrc")
NAME = "brn_flash_attention_varlen_forward"


def test_symbol_is_exported_declared_and_mirrored():
    import candle_birefnet_amd as cb
    assert hasattr(cb._ffi.lib, NAME) and NAME in cb._ffi.DECLARED
    header = open(os.path.join(ROOT, "include", "birefnet_hip.h")).read()
    assert re.search(r"\nbrn_status brn_flash_attention_varlen_forward\(const float\* q, const float\* k, const float\* v,"
                     r"\s+const int\* cu_seqlens_q, const int\* cu_seqlens_kv, int n_seqs,\s+int heads, int kv_heads, int head_dim,"
                     r"\s+int window_left, int window_right, float scale,\s+float\* y, brn_mem loc, int device_ordinal, void\* stream\);", header)
    assert header.index("\nbrn_status brn_flash_attention_gqa_forward(") < header.index("\nbrn_status " + NAME + "(")
    assert callable(cb.ops.flash_attention_varlen)
    assert cb._ffi.lib.brn_abi_version() == 1
    ffi = open(os.path.join(ROOT, "rust_shim", "src", "hip_ffi.rs")).read()
    assert "pub fn brn_flash_attention_varlen_forward(" in ffi


def test_header_states_what_is_not_provided():
    header = open(os.path.join(ROOT, "include", "birefnet_hip.h")).read()
    text = header[header.index("\nbrn_status brn_flash_attention_gqa_forward("):header.index("\nbrn_status " + NAME + "(")]
    text = " ".join(text.replace("*", " ").split())
    tail = text[text.index("Not provided:"):]
    for words in ("a bias with packed sequences", "[batch, heads, seq, head_dim] layout", "device-resident cu_seqlens", "a split over keys",
                  "16-bit tensors at the boundary"):
        assert words in tail, words
    for words in ('"flash attention varlen:"', "always HOST memory", "a window (either side >= 0) requires len_kv >= len_q", "synchronises the stream"):
        assert words in text, words


@pytest.mark.parametrize("name,args,word", VL.refusals(), ids=[r[0] for r in VL.refusals()])
def test_refusals_come_before_the_device_check(name, args, word):
    """status 1 with the entry's prefix and a message naming the limit, with or without a device"""
    import candle_birefnet_amd as cb
    st, msg = VL.raw_call(cb._ffi.lib, *args)
    assert st == 1 and msg.startswith("flash attention varlen: ") and word in msg, (name, st, msg)


def test_well_formed_call_without_a_device_is_loud():
    import candle_birefnet_amd as cb
    if cb.device_count() > 0:
        pytest.skip("a GPU is present")
    q, k, v, cq, ckv = VL.make_pack("A")
    for window in ((-1, -1), (15, 0)):
        with pytest.raises(cb.BrnError) as e:
            cb.ops.flash_attention_varlen(q, k, v, cq, ckv, window=window)
        assert e.value.status == 4 and "no CPU fallback" in str(e.value)


# ---- the plan header, alone, under the host sanitizers ----
SMALL_G = (1, 2, 3, 5, 16, 64, 65, 80)
SMALL_LQ = (1, 2, 3, 7, 16, 22, 33, 64, 65, 100)
SMALL_EXTRA = (0, 1, 63, 64, 65, 130)
SMALL_WINDOWS = VL.WINDOWS + [(0, -1), (1, 1), (64, 64), (127, 0), (128, 0)] + [far for far, _ in VL.FAR_WINDOWS]


def _sweep():
    return list(itertools.product(SMALL_G, SMALL_LQ, SMALL_EXTRA, SMALL_WINDOWS))


def _problems():
    """(lens, heads, kv_heads, window) of every problem the program is given: the packs x windows, then the sweep as one-sequence packs"""
    probs = [(VL.PACKS[n][0], VL.PACKS[n][1], VL.PACKS[n][2], w) for n in VL.PACKS for w in VL.WINDOWS]
    return probs + [([(lq, lq + extra)], G, 1, w) for G, lq, extra, w in _sweep()]


@pytest.fixture(scope="module")
def planned(tmp_path_factory):
    """the records the compiled header prints for _problems(), one list of 7-tuples per problem"""
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path_factory.mktemp("varlen_plan") / "varlen_plan")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", CSRC,
                           os.path.join(ROOT, "tests", "flash_varlen_plan_main.cpp"), "-o", exe])
    lines = []
    for lens, heads, kv_heads, w in _problems():
        cq, ckv = VL.cu_of(lens)
        lines.append(" ".join(str(int(x)) for x in [heads, kv_heads, w[0], w[1], len(lens), *cq, *ckv]))
    # refused contents ride along: the checks run under the sanitizers too
    bad = ["2 1 -1 -1 2 0 16 8 0 16 32", "2 1 -1 0 2 0 16 33 0 16 32", "1 1 -1 -1 1 0 65537 0 16", "2 1 -1 -1 1 1 16 0 16"]
    r = subprocess.run([exe], input="\n".join(lines + bad) + "\n", stdout=subprocess.PIPE, stderr=subprocess.PIPE, universal_newlines=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    out = r.stdout.splitlines()
    got, at = [], 0
    for _ in lines:
        assert out[at].startswith("P "), out[at]
        n = int(out[at][2:])
        got.append([tuple(int(x) for x in ln.split()) for ln in out[at + 1:at + 1 + n]])
        at += 1 + n
    tail = out[at:]
    assert len(tail) == len(bad) and all(ln.startswith("E ") for ln in tail), tail
    for ln, word in zip(tail, ("non-decreasing", "a window requires len_kv >= len_q", "<= 65536", "must start at 0")):
        assert word in ln, ln
    return got


def test_plan_header_prints_the_records_of_the_numpy_restatement(planned):
    for (lens, heads, kv_heads, w), got in zip(_problems(), planned):
        assert got == VL.plan(lens, heads, kv_heads, w), (lens, heads, kv_heads, w)


def test_records_own_every_row_once_and_walk_exactly_the_visible_keys(planned):
    """on the sweep of small (G, len_q, len_kv - len_q, window): every real (query, head) belongs to exactly one non-pad row; a pad row
    repeats the last real row; kt0 .. kt1 reaches every visible key of every row and is tight on both ends; a wave whose mask flag is off
    for a tile has no lane with an excluded key in it; the records are in non-increasing kt1 - kt0"""
    n_packs = len(VL.PACKS) * len(VL.WINDOWS)
    for (G, lq, extra, w), recs in zip(_sweep(), planned[n_packs:]):
        lkv = lq + extra
        vis = VL.visible(lq, lkv, w)
        assert vis.any(-1).all()                                               # no row is empty: the diagonal key is visible
        first, last = vis.argmax(-1), lkv - 1 - vis[:, ::-1].argmax(-1)        # per query: first and last visible key
        assert (vis.sum(-1) == last - first + 1).all()                         # contiguous
        owned = np.zeros((lq, G), int)
        assert len(recs) == (G * lq + VL.BQ - 1) // VL.BQ
        walks = [r[6] - r[5] for r in recs]
        assert all(a >= b for a, b in zip(walks, walks[1:])) and min(walks) >= 1
        for rec in recs:
            assert rec[:4] == (0, lq, 0, lkv)
            t = VL.row_map(rec, G, w)
            real = ~t["pad"]
            np.add.at(owned, (t["query"][real], t["head"][real]), 1)
            assert real[0] and (t["query"] < lq).all() and (t["head"] < G).all()
            end = np.flatnonzero(real)[-1]
            assert (t["query"][~real] == t["query"][end]).all() and (t["head"][~real] == t["head"][end]).all()
            assert (np.diff(t["query"]) >= 0).all()
            assert (t["lo"] == first[t["query"]]).all() and (t["hi"] == last[t["query"]] + 1).all()
            kt0, kt1 = rec[5], rec[6]
            assert kt0 == int(t["lo"].min()) // VL.T and kt1 == (int(t["hi"].max()) + VL.T - 1) // VL.T      # reaches every visible key, tight
            for wv in range(4):
                lo, hi = t["lo"][16 * wv:16 * wv + 16], t["hi"][16 * wv:16 * wv + 16]
                assert t["wave_hi"][wv] == hi.min() and t["wave_lo"][wv] == lo.max()
                for kt in range(kt0, kt1):
                    if not VL.tile_flag(kt * VL.T, t["wave_hi"][wv], t["wave_lo"][wv]):
                        assert (lo <= kt * VL.T).all() and (hi >= kt * VL.T + VL.T).all()
        assert (owned == 1).all(), (G, lq, lkv, w)


def test_pack_records_are_sorted_and_cover_every_sequence(planned):
    at = 0
    for name in VL.PACKS:
        lens, heads, kv_heads, _ = VL.PACKS[name]
        G = heads // kv_heads
        cq, ckv = VL.cu_of(lens)
        for w in VL.WINDOWS:
            recs = planned[at]
            at += 1
            walks = [r[6] - r[5] for r in recs]
            assert all(a >= b for a, b in zip(walks, walks[1:]))
            for s, (lq, lkv) in enumerate(lens):
                mine = sorted(r[4] for r in recs if r[:4] == (int(cq[s]), lq, int(ckv[s]), lkv) and lq > 0)
                assert mine == list(range(0, G * lq, VL.BQ)), (name, w, s)
            assert all(r[1] > 0 for r in recs)                                 # the entry with no queries has no record


def test_far_window_sides_plan_like_unbounded_ones(planned):
    """a side that reaches past every sequence (INT_MAX included) gives the records of -1 on that side: the header clamps it to 65536
    before any int arithmetic, the numpy restatement computes in exact integers"""
    sweep = _sweep()
    n_packs = len(VL.PACKS) * len(VL.WINDOWS)
    at = {p: i for i, p in enumerate(sweep)}
    seen = 0
    for far, near in VL.FAR_WINDOWS:
        for (G, lq, extra, w), recs in zip(sweep, planned[n_packs:]):
            if w == far:
                assert recs == VL.plan([(lq, lq + extra)], G, 1, near), (G, lq, extra, far)
                if (G, lq, extra, near) in at:
                    assert recs == planned[n_packs + at[(G, lq, extra, near)]]
                seen += 1
    assert seen == len(VL.FAR_WINDOWS) * len(SMALL_G) * len(SMALL_LQ) * len(SMALL_EXTRA)


def test_wrapper_checks_cu_seqlens_against_the_tensors():
    """what the C ABI cannot know: offsets that do not end at the tensors' rows would make the library write or read past them; int64
    offsets that do not fit int32 would wrap; refused in the wrapper, before the library"""
    import candle_birefnet_amd as cb
    q, k, v, cq, ckv = VL.make_pack("A")
    big = np.array(cq, np.int64)
    big[-1] += 2 ** 32
    for bad_q, bad_kv, word in ((cq[:-1], ckv[:-1], "rows of q"), (cq, np.array(ckv) + np.arange(len(ckv)), "rows of q"), (big, ckv, "fit int32"),
                                (np.array(cq, np.float64), ckv, "fit int32"), (cq[:1], ckv[:1], "n_seqs >= 1"), (cq, ckv[:-1], "n_seqs + 1")):
        with pytest.raises(ValueError) as e:
            cb.ops.flash_attention_varlen(q, k, v, bad_q, bad_kv)
        assert word in str(e.value), (word, str(e.value))
    with pytest.raises(ValueError):
        cb.ops.flash_attention_varlen(q, k, v[:-1], cq, ckv)


# ---- the walk ----
@pytest.mark.parametrize("name", list(VL.PACKS))
def test_emulation_stays_inside_the_bounds_and_equals_the_bias_walk(name):
    """every pack x window x {f32, bf16, f16}: the emulated FA_VARLEN walk (tile skipping, a row's leading wholly excluded tiles included)
    stays inside the bounds of the GPU parity test, and is array-equal to the emulation of the walk from tile 0 with the window written
    into a zero bias as -inf (flash_attention_gqa_cases.emulate)"""
    heads = VL.PACKS[name][1]
    worst = {}
    for s in VL.sequences(name):
        q, k, v = VL.seq_inputs(name, s)
        lq, lkv = VL.PACKS[name][0][s]
        for w in VL.WINDOWS:
            bias = VL.mask_bias(heads, lq, lkv, w)
            for s16 in (None, "bf16", "f16"):
                qq, kk, vv = ((VL.round_s16(a, s16) for a in (q, k, v)) if s16 else (q, k, v))
                ref = VL.case_reference(name, s, w, s16)
                bound = VL.s16_bound(ref, v, s16) if s16 else VL.f32_bound(ref)
                y = VL.emulate(qq, kk, vv, w, None, s16)
                err = float(np.abs(y.astype(np.float64) - ref).max())
                worst[s16 or "f32"] = max(worst.get(s16 or "f32", 0.0), err / bound)
                assert np.isfinite(y).all() and err <= bound, (s, w, s16, err, bound)
                with np.errstate(over="ignore", invalid="ignore"):
                    np.testing.assert_array_equal(y, GQ.emulate(qq, kk, vv, bias, 0, None, s16), err_msg=f"{s} {w} {s16}")
    print(f"pack {name}: worst error / bound " + ", ".join(f"{k_} {w_:.3f}" for k_, w_ in worst.items()))


def test_mask_bias_reference_is_the_window_reference():
    """what the GPU test of the windows leans on, in float64: the bias entry's reference on repeated K / V with the window as a -inf bias
    is the window reference"""
    for name in VL.PACKS:
        heads, kv_heads = VL.PACKS[name][1:3]
        for s in VL.sequences(name):
            q, k, v = VL.seq_inputs(name, s)
            lq, lkv = VL.PACKS[name][0][s]
            for w in VL.WINDOWS:
                old = FB.reference(q, GQ.repeat_kv(k, heads // kv_heads), GQ.repeat_kv(v, heads // kv_heads), VL.mask_bias(heads, lq, lkv, w))
                np.testing.assert_allclose(old, VL.case_reference(name, s, w), rtol=0, atol=1e-12)


def test_common_windows_are_the_masks_of_the_gqa_entry():
    """(-1, -1) is no mask and (-1, 0) the causal mask that ends at the last key"""
    for lq, lkv in ((1, 1), (7, 200), (65, 66), (100, 164)):
        assert VL.visible(lq, lkv, (-1, -1)).all()
        assert np.array_equal(VL.visible(lq, lkv, (-1, 0)), GQ.visible(lq, lkv))
