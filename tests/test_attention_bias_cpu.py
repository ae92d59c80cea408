"""brn_attention_forward without a GPU: the symbol and its mirrors exist, the argument checks come before the device check, and the
numpy emulation behind the 16-bit bound of tests/test_attention_bias_gpu.py."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import attention_bias_cases as A

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_symbol_is_exported_declared_and_mirrored():
    import candle_birefnet_amd as cb
    assert hasattr(cb._ffi.lib, "brn_attention_forward") and "brn_attention_forward" in cb._ffi.DECLARED
    header = open(os.path.join(ROOT, "include", "birefnet_hip.h")).read()
    assert re.search(r"\nbrn_status brn_attention_forward\(const float\* q, const float\* k, const float\* v, int batch, int heads, int N, int head_dim,", header)
    for fn in ("attention", "attention_with_bias", "attention_with_repeating_bias"):
        assert callable(getattr(cb.ops, fn))
    shim = os.path.join(ROOT, "rust_shim", "src")
    assert "pub fn brn_attention_forward(" in open(os.path.join(shim, "hip_ffi.rs")).read()
    flash = open(os.path.join(shim, "flash_attn.rs")).read()
    assert "pub fn flash_attention_with_bias(q: &Tensor, k: &Tensor, v: &Tensor, bias: &Tensor, causal: bool) -> Result<Tensor>" in flash
    assert "pub fn flash_attention_with_repeating_bias(q: &Tensor, k: &Tensor, v: &Tensor, bias: &Tensor, n_windows: usize, causal: bool) -> Result<Tensor>" in flash
    assert "pub mod flash_attn;" in open(os.path.join(shim, "lib.rs")).read()


def test_refusals_come_before_the_device_check():
    """status 1 with a message naming the limit, with or without a device"""
    import candle_birefnet_amd as cb
    for name, args, word in A.refusals():
        st, msg = A.raw_call(cb._ffi.lib, *args)
        assert st == 1 and word in msg, (name, st, msg)


def test_well_formed_call_without_a_device_is_loud():
    import candle_birefnet_amd as cb
    if cb.device_count() > 0:
        pytest.skip("a GPU is present")
    q, k, v, bias = A.make_inputs((2, 4, 16, 1))
    for call in (lambda: cb.ops.attention(q, k, v, bias), lambda: cb.ops.attention(q, k, v), lambda: cb.ops.attention_with_repeating_bias(q, k, v, bias, 1)):
        with pytest.raises(cb.BrnError) as e:
            call()
        assert e.value.status == 4 and "no CPU fallback" in str(e.value)


@pytest.mark.parametrize("s16", ["bf16", "f16"])
@pytest.mark.parametrize("shape", [s for s in A.SHAPES if s not in A.LARGE_GRID])
def test_probability_rounding_stays_inside_the_s16_bound(shape, s16):
    """the one rounding the GPU test's 16-bit reference lacks, emulated: the softmax numerators (times 1 or 2048, the two scalings a
    kernel may round them at) rounded to the 16-bit type before P v, the row sum taken from the unrounded or from the rounded values.
    Over q / k of std 0.1, 1 and 3 the result stays within u max |v| of the reference, so the bound u max |v| + 3e-5 max(1, max |ref|)
    asks nothing of the kernel that the arithmetic it stands for does not deliver."""
    u = A.S16_ULP[s16]
    worst = 0.0
    for qk_std in (0.1, 1.0, 3.0):
        q, k, v, bias = A.make_inputs(shape, qk_std=qk_std)
        q, k, v = (A.round_s16(a, s16) for a in (q, k, v))
        p = np.exp(A.scores(q, k, bias, shape[3]))
        ref = (p / p.sum(-1, keepdims=True)) @ v
        vmax = float(np.abs(v).max())
        for pscale in (1.0, 2048.0):
            pr = A.round_s16(p * pscale, s16) / pscale
            for den in (p.sum(-1, keepdims=True), pr.sum(-1, keepdims=True)):
                err = float(np.abs((pr @ v) / den - ref).max())
                worst = max(worst, err / (u * vmax))
                assert err <= u * vmax, (qk_std, pscale, err, u * vmax)
    print(f"{s16} {shape}: worst error {worst:.3f} of u max |v|")


def test_rust_shim_checker_is_green():
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "check_rust_shim.py")], capture_output=True, text=True)
    assert p.returncode == 0, p.stdout + p.stderr
