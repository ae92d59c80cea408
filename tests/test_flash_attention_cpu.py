"""brn_flash_attention_forward without a GPU: the symbol and its mirrors exist, the argument checks come before the device check, and
the numpy emulation of the tile-wise algorithm that stands behind the bounds of tests/test_flash_attention_gpu.py."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import flash_attention_cases as A

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32_TOL = 3e-5


def test_symbol_is_exported_declared_and_mirrored():
    import candle_birefnet_amd as cb
    assert hasattr(cb._ffi.lib, "brn_flash_attention_forward") and "brn_flash_attention_forward" in cb._ffi.DECLARED
    header = open(os.path.join(ROOT, "include", "birefnet_hip.h")).read()
    assert "typedef enum { BRN_ATTN_BSHD = 0, BRN_ATTN_BHSD = 1 } brn_attn_layout;" in header
    assert re.search(r"\nbrn_status brn_flash_attention_forward\(const float\* q, const float\* k, const float\* v,\s+int batch, int seq_q, int seq_kv, int heads, int head_dim,"
                     r"\s+int layout, int causal, float scale,\s+float\* y, brn_mem loc, int device_ordinal, void\* stream\);", header)
    assert (cb._ffi.BRN_ATTN_BSHD, cb._ffi.BRN_ATTN_BHSD) == (0, 1)
    assert callable(cb.ops.flash_attention)
    shim = os.path.join(ROOT, "rust_shim", "src")
    ffi = open(os.path.join(shim, "hip_ffi.rs")).read()
    assert "pub fn brn_flash_attention_forward(" in ffi and "pub const BRN_ATTN_BSHD: c_int = 0;" in ffi and "pub const BRN_ATTN_BHSD: c_int = 1;" in ffi
    flash = open(os.path.join(shim, "flash_attn.rs")).read()
    assert "pub fn flash_attention(q: &Tensor, k: &Tensor, v: &Tensor, causal: bool) -> Result<Tensor>" in flash
    assert "ffi::brn_flash_attention_forward(" in flash and "ffi::BRN_ATTN_BSHD" in flash


def test_header_points_from_the_short_entry_to_the_long_one():
    header = open(os.path.join(ROOT, "include", "birefnet_hip.h")).read()
    short = header[header.index("flash_attention_with_bias / flash_attention_with_repeating_bias"):header.index("\nbrn_status brn_attention_forward(")]
    assert "brn_flash_attention_forward" in short
    long = header[header.index("\nbrn_status brn_attention_forward("):header.index("\nbrn_status brn_flash_attention_forward(")]
    for words in ("a bias together with long sequences", "seq_q != seq_kv", "head dims other than 32 / 64 / 128"):
        assert words in " ".join(long.replace("*", " ").split()), words


@pytest.mark.parametrize("name,args,word", A.refusals(), ids=[r[0] for r in A.refusals()])
def test_refusals_come_before_the_device_check(name, args, word):
    """status 1 with a message naming the limit, with or without a device"""
    import candle_birefnet_amd as cb
    st, msg = A.raw_call(cb._ffi.lib, *args)
    assert st == 1 and word in msg, (name, st, msg)


def test_well_formed_call_without_a_device_is_loud():
    import candle_birefnet_amd as cb
    if cb.device_count() > 0:
        pytest.skip("a GPU is present")
    for shape in ((2, 17, 17, 3, 64, "bshd", 0), (2, 17, 17, 3, 64, "bhsd", 1)):
        q, k, v = A.make_inputs(shape)
        with pytest.raises(cb.BrnError) as e:
            cb.ops.flash_attention(q, k, v, causal=bool(shape[6]), layout=shape[5])
        assert e.value.status == 4 and "no CPU fallback" in str(e.value)


def _emulate(q, k, v, layout, causal, scale, tile, s16):
    """The tile-wise algorithm of kernels/flash_attention.hip in numpy, fp32 (np.float32) arithmetic throughout: K / V walked in tiles of
    `tile` keys; scores times scale * log2(e) in one multiply; a running maximum m and a running sum l; O and l rescaled by
    exp2(m_old - m_new); numerators exp2(s - m_new), rounded to the 16-bit type for P v when s16 is given, l taken from the unrounded
    ones; excluded keys (causal) simply absent.  q, k, v: already rounded to the 16-bit type when s16 is given."""
    f = np.float32
    q, k, v = (A.to_bhsd(np.asarray(a, f), layout) for a in (q, k, v))
    sq, skv, hd = q.shape[2], k.shape[2], q.shape[3]
    sc2 = f(f(scale if scale else f(1.0) / np.sqrt(f(hd))) * f(1.4426950408889634))
    m = np.full(q.shape[:3] + (1,), -3.0e38, f)
    l = np.zeros_like(m)
    o = np.zeros(q.shape, f)
    for k0 in range(0, skv, tile):
        s = (q @ k[:, :, k0:k0 + tile].transpose(0, 1, 3, 2)).astype(f) * sc2
        if causal:
            s = np.where((k0 + np.arange(s.shape[-1]))[None, :] <= np.arange(sq)[:, None], s, f(-3.0e38))
        mn = np.maximum(m, s.max(-1, keepdims=True))
        alpha = np.exp2(m - mn)
        p = np.exp2(s - mn)
        l = l * alpha + p.sum(-1, keepdims=True, dtype=f)
        pr = A.round_s16(p, s16).astype(f) if s16 else p
        o = o * alpha + (pr @ v[:, :, k0:k0 + tile]).astype(f)
        m = mn
    return np.ascontiguousarray(A.to_bhsd(o / l, layout))


SMALL = [s for s in A.SHAPES if s not in A.LARGEST]


@pytest.mark.parametrize("shape", SMALL, ids=A.case_id)
def test_tilewise_emulation_stays_inside_the_bounds(shape):
    """the evidence behind the GPU bounds: over tiles of 16, 64 and 128 keys the emulation stays within 3e-5 max(1, max |ref|) of the
    float64 reference in fp32, and within u max |v| + 3e-5 max(1, max |ref|) of the float64 reference on rounded q, k, v in the 16-bit
    types — a numerator rounded relative to a running maximum and later multiplied by fp32 rescale factors still carries u / 2.
    No case needed other inputs to stay inside."""
    causal, scale = shape[6], A.case_scale(shape)
    q, k, v = A.make_inputs(shape)
    vmax = float(np.abs(v).max())
    worst = {}
    for s16 in (None, "bf16", "f16"):
        ref = A.case_reference(shape, s16)
        qq, kk, vv = ((A.round_s16(a, s16) for a in (q, k, v)) if s16 else (q, k, v))
        bound = (A.S16_ULP[s16] * vmax if s16 else 0.0) + F32_TOL * max(1.0, float(np.abs(ref).max()))
        for tile in (16, 64, 128):
            y = _emulate(qq, kk, vv, shape[5], causal, scale, tile, s16)
            err = float(np.abs(y.astype(np.float64) - ref).max())
            worst[s16 or "f32"] = max(worst.get(s16 or "f32", 0.0), err / bound)
            assert np.isfinite(y).all() and err <= bound, (s16, tile, err, bound)
    print(f"{A.case_id(shape)}: worst error / bound " + ", ".join(f"{k_} {w:.3f}" for k_, w in worst.items()))


def test_integer_cases_have_exact_scores_and_reach_their_regimes():
    """q and k of the integer-valued cases survive the 16-bit rounding unchanged; 'large' has row maxima that overflow exp in fp32;
    'rising' ends with its weight in the last K / V tile, 'falling' keeps it in the first"""
    for shape in A.SHAPES:
        kind = A.KIND[shape]
        if kind.startswith("std"):
            continue
        q, k, v = A.make_inputs(shape)
        for s16 in ("bf16", "f16"):
            assert np.array_equal(A.round_s16(q, s16), q) and np.array_equal(A.round_s16(k, s16), k)
        qb, kb = (A.to_bhsd(np.asarray(a, np.float64), shape[5]) for a in (q, k))
        s = (qb @ kb.transpose(0, 1, 3, 2)) * 0.5
        p = np.exp(s - s.max(-1, keepdims=True))
        p /= p.sum(-1, keepdims=True)
        last0 = (shape[2] - 1) // A.T * A.T
        if kind == "large":
            assert s.max(-1).min() > 40 and s.max() > 89          # exp(89) > FLT_MAX
        elif kind == "rising":
            assert p[..., last0:].sum(-1).min() > 0.99                   # (the last tile is ragged: 44 of 64 keys)
            tile_max = [s[..., t0:t0 + A.T].max(-1) for t0 in range(0, shape[2], A.T)]
            assert all((b > a).all() for a, b in zip(tile_max, tile_max[1:]))
        else:
            assert p[..., :A.T].sum(-1).min() > 0.99


def test_rust_shim_checker_is_green():
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "check_rust_shim.py")], capture_output=True, text=True)
    assert p.returncode == 0, p.stdout + p.stderr
