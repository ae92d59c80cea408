"""brn_flash_attention_bias_forward without a GPU: the symbol and its mirrors exist, the argument checks come before the device check, the
committed inputs reach the regime each case is there for, and the numpy emulation of the tile-wise algorithm that stands behind the
bounds of tests/test_flash_attention_bias_gpu.py."""
import inspect
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import flash_attention_bias_cases as B

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_symbol_is_exported_declared_and_mirrored():
    import candle_birefnet_amd as cb
    assert hasattr(cb._ffi.lib, "brn_flash_attention_bias_forward") and "brn_flash_attention_bias_forward" in cb._ffi.DECLARED
    header = open(os.path.join(ROOT, "include", "birefnet_hip.h")).read()
    assert re.search(r"\nbrn_status brn_flash_attention_bias_forward\(const float\* q, const float\* k, const float\* v,\s+int batch, int seq_q, int seq_kv, int heads, int head_dim,"
                     r"\s+int layout, int causal,\s+const float\* bias, int n_bias, float scale,\s+float\* y, brn_mem loc, int device_ordinal, void\* stream\);", header)
    assert header.index("\nbrn_status brn_flash_attention_forward(") < header.index("\nbrn_status brn_flash_attention_bias_forward(")
    assert "bias" in inspect.signature(cb.ops.flash_attention).parameters
    assert inspect.signature(cb.ops.flash_attention).parameters["bias"].default is None
    shim = os.path.join(ROOT, "rust_shim", "src")
    assert "pub fn brn_flash_attention_bias_forward(" in open(os.path.join(shim, "hip_ffi.rs")).read()
    flash = open(os.path.join(shim, "flash_attn.rs")).read()
    # the two bias functions share one body: both must reach it, and it must hold both routes
    body = flash[flash.index("fn attention("):flash.index("pub fn flash_attention_with_bias(")]
    assert "ffi::brn_flash_attention_bias_forward(" in body and "ffi::brn_attention_forward(" in body and "ffi::BRN_ATTN_BHSD" in body
    assert "n <= 144 && head_dim == 32 && !causal" in body and "no causal mask" not in flash
    for name in ("flash_attention_with_bias", "flash_attention_with_repeating_bias"):
        fn = flash[flash.index(f"pub fn {name}("):]
        assert re.match(r"[^{]*\{\s*attention\(q, k, v, bias, .*, causal\)\s*\}", fn), name


def test_header_points_to_the_bias_entry():
    """the old 'Not provided' sentence of the bias-free entry still stands and now names the entry that provides the bias"""
    header = open(os.path.join(ROOT, "include", "birefnet_hip.h")).read()
    long = header[header.index("\nbrn_status brn_attention_forward("):header.index("\nbrn_status brn_flash_attention_forward(")]
    flat = " ".join(long.replace("*", " ").split())
    assert "Not provided: a bias together with long sequences" in flat
    assert flat.index("brn_flash_attention_bias_forward") > flat.index("Not provided: a bias together with long sequences")
    text = " ".join(header[header.index("\nbrn_status brn_flash_attention_forward("):header.index("\nbrn_status brn_flash_attention_bias_forward(")].replace("*", " ").split())
    for words in ("[n_bias, heads, seq_q, seq_kv]", "UNSCALED", "-inf", "comes back NaN", "batch % n_bias == 0", "no atomics"):
        assert words in text, words


@pytest.mark.parametrize("name,args,word", B.refusals(), ids=[r[0] for r in B.refusals()])
def test_refusals_come_before_the_device_check(name, args, word):
    """status 1 with the entry's prefix and a message naming the limit, with or without a device"""
    import candle_birefnet_amd as cb
    st, msg = B.raw_call(cb._ffi.lib, *args)
    assert st == 1 and msg.startswith("flash attention bias:") and word in msg, (name, st, msg)


def test_well_formed_call_without_a_device_is_loud():
    import candle_birefnet_amd as cb
    if cb.device_count() > 0:
        pytest.skip("a GPU is present")
    for shape in ((2, 17, 17, 3, 64, 0, 2, "std"), (2, 17, 17, 3, 64, 1, 1, "std")):
        q, k, v, bias = B.make_inputs(shape)
        with pytest.raises(cb.BrnError) as e:
            cb.ops.flash_attention(q, k, v, causal=bool(shape[5]), layout=B.LAYOUT[shape], bias=bias)
        assert e.value.status == 4 and "no CPU fallback" in str(e.value)
    q, k, v, _ = B.make_inputs((2, 17, 17, 3, 64, 0, 2, "std"))
    y = np.zeros_like(q)
    st, msg = B.raw_call(cb._ffi.lib, q, k, v, 2, 17, 17, 3, 64, 0, 0, None, 0, 0.0, y)         # bias NULL, n_bias 0: allowed
    assert st == 4, (st, msg)


def _emulate(q, k, v, bias, layout, causal, scale, tile, s16, placement):
    """The tile-wise algorithm of kernels/flash_attention.hip with the bias, in numpy, fp32 (np.float32) arithmetic throughout: K / V
    walked in tiles of `tile` keys; the bias tile joins the UNSCALED fp32 scores, either after the product ("add": (s + b) * sc2) or as
    the initial accumulator of the product ("acc": the kernels' choice — the products are added to it in k-steps of 4 (fp32) or 32
    (16-bit) head dims, as the matrix instructions do); times scale * log2(e) in one multiply; a running maximum m and a running sum l;
    O and l rescaled by exp2(m_old - m_new); numerators exp2(s - m_new), rounded to the 16-bit type for P v when s16 is given, l taken
    from the unrounded ones; excluded keys (causal) at -3e38.  q, k, v: already rounded to the 16-bit type when s16 is given."""
    f = np.float32
    q, k, v = (B.to_bhsd(np.asarray(a, f), layout) for a in (q, k, v))
    sq, skv, hd = q.shape[2], k.shape[2], q.shape[3]
    bias = np.asarray(bias, f)[np.arange(q.shape[0]) % bias.shape[0]]
    sc2 = f(f(scale if scale else f(1.0) / np.sqrt(f(hd))) * f(1.4426950408889634))
    m = np.full(q.shape[:3] + (1,), -3.0e38, f)
    l = np.zeros_like(m)
    o = np.zeros(q.shape, f)
    step = 32 if s16 else 4
    for k0 in range(0, skv, tile):
        kt = k[:, :, k0:k0 + tile].transpose(0, 1, 3, 2)
        bt = bias[..., k0:k0 + tile]
        if placement == "add":
            s = (q @ kt).astype(f) + bt
        else:
            s = bt.copy()
            for d0 in range(0, hd, step):
                s = s + (q[..., d0:d0 + step] @ kt[:, :, d0:d0 + step]).astype(f)
        with np.errstate(invalid="ignore"):
            s = s * sc2
        if causal:
            s = np.where((k0 + np.arange(s.shape[-1]))[None, :] <= np.arange(sq)[:, None], s, f(-3.0e38))
        mn = np.maximum(m, s.max(-1, keepdims=True))
        alpha = np.exp2(m - mn)
        p = np.exp2(s - mn)
        l = l * alpha + p.sum(-1, keepdims=True, dtype=f)
        pr = B.round_s16(p, s16).astype(f) if s16 else p
        o = o * alpha + (pr @ v[:, :, k0:k0 + tile]).astype(f)
        m = mn
    return np.ascontiguousarray(B.to_bhsd(o / l, layout))


@pytest.mark.parametrize("shape", B.SHAPES, ids=B.case_id)
def test_tilewise_emulation_stays_inside_the_bounds(shape):
    """The evidence behind the GPU bounds, re-established for the committed seeds: over tiles of 16, 64 and 128 keys and both placements
    of the bias add, the emulation stays within 3e-5 max(1, max |ref|) of the float64 reference in fp32 and within
    u max |v| + 3e-5 max(1, max |ref|) of the float64 reference on rounded q, k, v in the 16-bit types.  And the case can tell a kernel
    that drops the bias: its with-bias and bias-free references differ by more than 10 x the bound (seq 1 excepted: one key, weight 1)."""
    causal, scale, layout = shape[5], B.case_scale(shape), B.LAYOUT[shape]
    q, k, v, bias = B.make_inputs(shape)
    worst = {}
    for s16 in (None, "bf16", "f16"):
        ref = B.case_reference(shape, s16)
        qq, kk, vv = ((B.round_s16(a, s16) for a in (q, k, v)) if s16 else (q, k, v))
        bound = B.s16_bound(ref, v, s16) if s16 else B.f32_bound(ref)
        assert np.isfinite(ref).all()
        if shape[1:3] != (1, 1):
            moved = float(np.abs(B.case_reference(shape, s16, with_bias=False) - ref).max())
            assert moved > 10 * bound, (s16, moved, bound)
        for tile in (16, 64, 128):
            for placement in ("add", "acc"):
                y = _emulate(qq, kk, vv, bias, layout, causal, scale, tile, s16, placement)
                err = float(np.abs(y.astype(np.float64) - ref).max())
                worst[s16 or "f32"] = max(worst.get(s16 or "f32", 0.0), err / bound)
                assert np.isfinite(y).all() and err <= bound, (s16, tile, placement, err, bound)
    print(f"{B.case_id(shape)}: worst error / bound " + ", ".join(f"{k_} {w:.3f}" for k_, w in worst.items()))


def test_cases_reach_their_regimes():
    """The integer kinds survive the 16-bit rounding unchanged and have exact scores; 'large' has row maxima that overflow exp in fp32;
    'rising' ends with > 0.99 of its weight in the last K / V tile and its tile maxima rise, 'falling' keeps > 0.99 in the first; the swin kinds
    give their masked keys probabilities below 1e-30; 'pad' gives its -inf keys exactly 0."""
    seen = set()
    for shape in B.SHAPES:
        kind, skv = shape[7], shape[2]
        if kind == "std":
            continue
        seen.add(kind)
        q, k, v, bias = B.make_inputs(shape)
        p = B.probabilities(q, k, bias, B.LAYOUT[shape], shape[5], B.case_scale(shape))
        if kind in ("large", "rising", "falling"):
            for s16 in ("bf16", "f16"):
                assert np.array_equal(B.round_s16(q, s16), q) and np.array_equal(B.round_s16(k, s16), k)
            assert np.array_equal(bias, np.round(bias)) and float(np.abs(bias).max()) <= 2048      # integers fp32 adds exactly to integer scores
            qb, kb = (B.to_bhsd(np.asarray(a, np.float64), B.LAYOUT[shape]) for a in (q, k))
            s = (qb @ kb.transpose(0, 1, 3, 2) + bias.astype(np.float64)[np.arange(shape[0]) % shape[6]]) * 0.5
            last0 = (skv - 1) // B.T * B.T
            if kind == "large":
                assert np.array_equal(bias % 2, np.zeros_like(bias)) and np.array_equal(2 * s, np.round(2 * s))
                assert s.max(-1).min() > 40 and s.max() > 89          # exp(89) > FLT_MAX
            elif kind == "rising":
                assert p[..., last0:].sum(-1).min() > 0.99
                tile_max = [s[..., t0:t0 + B.T].max(-1) for t0 in range(0, skv, B.T)]
                assert all((b > a).all() for a, b in zip(tile_max, tile_max[1:]))
            else:
                assert p[..., :B.T].sum(-1).min() > 0.99
        elif kind.startswith("swin"):
            ws = int(kind[4:])
            _, masks = B.swin_bias(ws, shape[3], shape[4] ** -0.5, np.random.default_rng(0))
            masked = np.broadcast_to((masks < 0)[np.arange(shape[0]) % 4][:, None], p.shape)
            assert masked[1:4].any(axis=(1, 2, 3)).all() and not masked[0].any()        # pattern 0 has no mask, the others do
            assert float(p[masked].max()) < 1e-30
            assert abs(float(bias.min()) + 100.0 / shape[4] ** -0.5) < 3.0 / shape[4] ** -0.5          # -565.7 at head_dim 32
        else:
            assert kind == "pad"
            for pattern, first in enumerate(B.PAD_FROM):
                assert np.isneginf(bias[pattern, :, :, first:]).all() and np.isfinite(bias[pattern, :, :, :first]).all()
                assert (p[pattern::2, :, :, first:] == 0.0).all() and (p[pattern::2, :, :, :first] > 0.0).any()
    assert seen == {"swin16", "swin24", "large", "rising", "falling", "pad"}


def test_rust_shim_checker_is_green():
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "check_rust_shim.py")], capture_output=True, text=True)
    assert p.returncode == 0, p.stdout + p.stderr
