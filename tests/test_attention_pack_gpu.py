"""Window attention over the real queries only (csrc/kernels/window_geometry.h; switch BRN_ATT_PACK_Q): window_attention_split_kernel
(compute modes f32_half2, f32_split2) and window_attention_bf16_kernel (bf16, f16; one and two heads per workgroup) on the smallest
geometries that reach each case of the packing — whole query tiles that disappear, pad columns (nothing disappears unless the queries are
packed), windows with fewer than 16 real queries, a partial last tile, corner windows with the wrap and the mask, and a map without a pad
token (grid order, all nine tiles).  Entry, fp64 restatement and bounds of tests/test_attention_split_gpu.py for the split modes, of
tests/test_ops_gpu.py::test_window_attention_bf16_mode for the 16-bit ones.  A pad query's row never reaches the output and a query's
result depends on its own lane group only, so the switch must not change a single bit: checked between child processes (the switch is
read once per process), op by op and on the logits of a model whose backbone launches two geometries at once."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

from test_attention_split_gpu import TOL, _case, _run
from test_ops_gpu import ATT_BF16_TOL, _att_bf16_reference, _attn_weights, rnd

pytestmark = pytest.mark.gpu

GEOMETRIES = [
    (2, 16, 24, 2, 0), (2, 16, 24, 2, 6),      # pad rows only: whole tiles disappear; two heads: the bf16 kernel's two-head form
    (2, 24, 16, 3, 0), (2, 24, 16, 3, 6),      # pad columns only: nothing disappears without packing; odd head count
    (1, 13, 13, 1, 0), (1, 13, 13, 1, 6),      # windows with 12 real tokens and with 1: a partial last tile, nq < 16
    (2, 30, 30, 3, 6),                         # corner, wrap and mask together
    (1, 24, 24, 2, 6),                         # no pad token: identity order, all nine tiles
]
MODES = ["f32_half2", "f32_split2", "bf16", "f16"]
MODEL_MODES = ["f32_half2", "bf16"]

_CHILD = r"""
import sys
import numpy as np
sys.path.insert(0, %(root)r); sys.path.insert(0, %(tests)r)
import candle_birefnet_amd as cb
import test_attention_pack_gpu as T
outs = {}
for g in T.GEOMETRIES:
    for mode in T.MODES:
        outs["op_%%s_%%s" %% (mode, "_".join(map(str, g)))] = np.asarray(T._op(mode, *g))
for mode in T.MODEL_MODES:
    outs["model_" + mode] = T._logits(mode)
np.savez(sys.argv[1], **outs)
"""


def _inputs(B, H, W, heads, shift):
    """the weights and the input of tests/test_attention_split_gpu.py::_case and of test_ops_gpu._att_bf16_reference"""
    return _attn_weights(heads * 32, heads, seed=10), rnd(B, H, W, heads * 32, seed=99)


def _op(mode, B, H, W, heads, shift):
    w, x = _inputs(B, H, W, heads, shift)
    return _run(mode, x, w, heads, shift)


@functools.lru_cache(maxsize=None)
def _model_inputs():
    import candle_birefnet_amd as cb
    cfg = cb.BiRefNetConfig(deform_mode="reference_cpu")
    cfg.swin.depths = [2, 2, 2, 2]
    return cfg, cb.synth_weights(cb.birefnet_weight_spec(cfg), seed=42), cb.synth_input(1, 160, 160)


def _logits(mode):
    """the 160 x 160 model of tests/test_attention_split_gpu.py::test_split_attention_two_geometries_in_one_launch"""
    import candle_birefnet_amd as cb
    cfg, w, x = _model_inputs()
    m = cb.BiRefNet.new(cfg, cb.VarBuilder.from_tensors(w), compute=mode)
    try:
        return np.asarray(m.forward_logits(x))
    finally:
        m.close()


@pytest.fixture(scope="module")
def switched(gpu, tmp_path_factory):
    """every op case and the model logits with BRN_ATT_PACK_Q=0 and =1, one child process each"""
    d = tmp_path_factory.mktemp("att_pack")
    code = _CHILD % {"root": os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests": os.path.dirname(os.path.abspath(__file__))}
    res = {}
    for v in ("0", "1"):
        out = str(d / f"pack{v}.npz")
        pr = subprocess.run([sys.executable, "-c", code, out], env=dict(os.environ, BRN_ATT_PACK_Q=v), capture_output=True, text=True, timeout=600)
        assert pr.returncode == 0, pr.stderr[-3000:]
        res[v] = np.load(out)
    assert sorted(res["0"].files) == sorted(res["1"].files) and len(res["0"].files) == len(GEOMETRIES) * len(MODES) + len(MODEL_MODES)
    return res


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("B,H,W,heads,shift", GEOMETRIES)
def test_packed_queries(gpu, switched, mode, B, H, W, heads, shift):
    y = _op(mode, B, H, W, heads, shift)
    assert np.isfinite(y).all()
    if mode in TOL:
        ref = _case(B, H, W, heads, shift)[2]
        scale = max(1.0, float(np.abs(ref).max()))
        bound = TOL[mode] * scale                                        # test_ops_gpu._close
    else:
        ref = _att_bf16_reference(B, H, W, heads, shift, s16=mode)[2]
        scale = float(np.abs(ref).max())
        bound = ATT_BF16_TOL * scale * (1.0 if mode == "bf16" else 0.125)
    err = float(np.abs(np.asarray(y, np.float64) - ref).max())
    print(f"packed attention {mode} B{B} {H}x{W} h{heads} s{shift}: max abs err {err:.2e}, bound {bound:.2e}, |ref| max {np.abs(ref).max():.2f}")
    assert err <= bound
    np.testing.assert_array_equal(y, _op(mode, B, H, W, heads, shift))          # the same call twice: the same bits
    key = "op_%s_%s" % (mode, "_".join(map(str, (B, H, W, heads, shift))))
    np.testing.assert_array_equal(switched["0"][key], switched["1"][key])      # all positions, grid order == real queries, long windows first
    np.testing.assert_array_equal(y, switched["1"][key])


@pytest.mark.parametrize("mode", MODEL_MODES)
def test_model_logits_bit_equal_between_switch_values(gpu, switched, mode):
    """two geometries in one launch (stage 0: the 40 x 40 and the 20 x 20 map, both padded), the reordered dispatch, the P2 output of
    mode f32_half2"""
    a, b = switched["0"]["model_" + mode], switched["1"]["model_" + mode]
    assert a.shape == (1, 1, 160, 160) and np.isfinite(a).all()
    np.testing.assert_array_equal(a, b)
