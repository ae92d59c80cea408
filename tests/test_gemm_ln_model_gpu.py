"""The GEMM -> LayerNorm route (brn_gemm_ln.cpp, switch BRN_GEMM_LN) inside whole models: the smallest full-depth golden model
(m96_d2222_ref_b2) in the three split modes, one child process per switch value (switches are read once per process).
 * BRN_GEMM_LN=2 (every eligible pair takes the route with two slices): within the 1e-4 of test_hip_model_goldens_and_oracle against the fp64
   golden, bit-identical when repeated (fixed summation order, no atomics), and different from BRN_GEMM_LN=0 in every mode — the route ran.
 * the default (the planner decides) and 0 (the GEMM, reduce and LayerNorm launches of before: no route) meet the same bound."""
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
TAG, MODES = "m96_d2222_ref_b2", ["f32_half2", "f32_split2", "f32_split3"]

CODE = (
    "import sys, numpy as np; sys.path.insert(0, %r); sys.path.insert(0, %r)\n"
    "import candle_birefnet_amd as cb, golden_cases as G\n"
    "cfg, w, x = G.model_case(%r)\n"
    "outs = {}\n"
    "for mode in %r:\n"
    "    m = cb.BiRefNet.new(cfg, cb.VarBuilder.from_tensors(w), compute=mode)\n"
    "    ys = [np.asarray(m.forward_logits(x)) for _ in range(3)]\n"
    "    assert all(np.array_equal(ys[0], y) for y in ys[1:]), mode\n"
    "    outs[mode] = ys[0]\n"
    "    m.close()\n"
    "np.savez(sys.argv[1], **outs)\n") % (os.path.dirname(HERE), HERE, TAG, MODES)


def test_route_in_whole_models(gpu, tmp_path):
    gold = np.load(os.path.join(HERE, "golden", "models_small.npz"))[TAG]
    res = {}
    for setting in ("0", "", "2"):
        out = str(tmp_path / f"gemm_ln{setting or 'default'}.npz")
        env = dict(os.environ)
        env.pop("BRN_GEMM_LN", None)
        if setting:
            env["BRN_GEMM_LN"] = setting
        pr = subprocess.run([sys.executable, "-c", CODE, out], env=env, capture_output=True, text=True, timeout=600)
        assert pr.returncode == 0, pr.stderr[-2000:]
        res[setting] = np.load(out)
    for mode in MODES:
        for setting in res:
            e = float(np.abs(res[setting][mode].astype(np.float64) - gold).max())
            print(f"{TAG} [{mode}] BRN_GEMM_LN={setting or 'default'}: max abs err vs golden(fp64) {e:.2e}")
            assert e < 1e-4, (mode, setting, e)
        d = float(np.abs(res["2"][mode] - res["0"][mode]).max())
        print(f"{TAG} [{mode}]: max |BRN_GEMM_LN=2 - BRN_GEMM_LN=0| {d:.2e}")
        assert d > 0.0, f"{mode}: the route changed no bit, so it did not run"
