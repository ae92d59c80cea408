"""brn_deform_conv2d_offsets_forward (ops.deform_conv2d) on the GPU: both routes — fused (one offset group, the same stride / pad / dilation
on both axes: the gather loaders of every mode behind deform_om_pack_kernel) and columns (everything else: deform_im2col_kernel + the
mode's dense GEMM) — against the fp64 restatement of tests/deform_offsets_cases.py.  Which route a case takes follows from its geometry
alone (csrc/brn_deform_offsets.cpp, deform_offsets_fused_eligible); test 4 pins the fused one to the layer's bits.

Bounds are the project's own for this arithmetic: mode f32 1e-4 max(1, max|ref|) (test_ops_gpu.py::test_deform_conv2d), the plane modes
the TOL table of test_deform_split_gpu.py, bf16 / f16 S16_ULP |ref| + (4e-3 | 5e-4) max|ref| against the exact-operand reference
(test_ops_gpu.py::test_deform_conv2d_bf16_mode)."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

import deform_offsets_cases as DC
from test_deform_split_gpu import S1, S3, TOL

PLANE_MODES = ["f32_split3", "f32_split2", "f32_half2"]
ALL_MODES = ["f32"] + PLANE_MODES + ["bf16", "f16"]
S16_ULP = {"bf16": 2.0 ** -8, "f16": 2.0 ** -11}
S16_ABS = {"bf16": 4e-3, "f16": 5e-4}


def check_mode_bound(y, ref, mode, what):
    """the mode's bound, with the measured figure printed before it is asserted"""
    y = np.asarray(y, np.float64)
    assert y.shape == ref.shape and np.isfinite(y).all(), what
    err = np.abs(y - ref)
    scale = np.abs(ref).max()
    if mode in S16_ULP:
        bound = S16_ULP[mode] * np.abs(ref) + S16_ABS[mode] * scale
        print(f"{what} [{mode}]: max abs err {err.max():.3e}, |ref| max {scale:.3f}, worst err / bound {(err / bound).max():.3f}")
        assert (err <= bound).all(), f"{what} [{mode}]: max abs err {err.max():.3e} (|ref| max {scale:.2f})"
    else:
        tol = 1e-4 if mode == "f32" else TOL[mode]
        rel = err.max() / max(1.0, scale)
        print(f"{what} [{mode}]: max err {rel:.3e} of max(1, max|ref| = {scale:.3f}) (tolerance {tol:.0e})")
        assert rel <= tol, f"{what} [{mode}]: {rel:.3e} > {tol:.0e}"


# ---- the cases: (B, C, G, kh, kw, stride, padding, dilation, H, W, O, mask) -------------------------------------------------------------
COL_A = (2, 8, 4, 3, 2, (2, 1), (1, 0), (1, 2), 9, 7, 5, True)         # C / G = 2: a 4-channel chunk straddles two groups (element path)
COL_B = (1, 3, 3, 1, 1, (1, 1), (0, 0), (1, 1), 5, 6, 1, False)        # one channel a group, 1 x 1, no mask, one output channel
COL_C = (3, 32, 1, 3, 1, (1, 1), (1, 0), (1, 1), 5, 7, 8, True)        # pad_h != pad_w; M = 105: a tile spans three images, the last is ragged
FUSED_DIL = (1, 64, 1, 3, 3, (1, 1), (2, 2), (2, 2), 12, 12, 256, False)
FUSED_7 = (1, 64, 1, 7, 7, (1, 1), (3, 3), (1, 1), 12, 12, 256, True)
FUSED_RECT = (2, 64, 1, 3, 5, (1, 1), (4, 4), (2, 2), 12, 12, 256, True)    # kh != kw AND dilation 2 through every mode's loader (test 5)
COL_MODES = (2, 64, 2, 3, 2, (2, 1), (1, 0), (1, 2), 13, 11, 40, True)      # the column route in every mode: vector chunks in fp32 and 16-bit


@functools.lru_cache(maxsize=None)
def _case(spec, seed=7):
    return DC.random_case(seed, *spec)


@functools.lru_cache(maxsize=None)
def _ref(spec, mode="f32"):
    return DC.reference(_case(spec), "f32" if mode not in S16_ULP else mode)


def test_routes_of_the_cases():
    """(CPU) the eligibility rule, restated: G == 1 and equal stride, pad, dilation on both axes"""
    fused = lambda s: s[2] == 1 and s[5][0] == s[5][1] and s[6][0] == s[6][1] and s[7][0] == s[7][1]
    assert [fused(s) for s in (COL_A, COL_B, COL_C, COL_MODES)] == [False] * 4
    assert [fused(s) for s in (FUSED_DIL, FUSED_7, FUSED_RECT)] == [True] * 3
    assert DC.out_hw(5, 7, 3, 1, 1, (1, 0), 1) == (5, 7) and 3 * 5 * 7 == 105


# ---- test 1: column route geometry, mode f32 ---------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("spec", [COL_A, COL_B, COL_C], ids=["A-groups-straddle", "B-1x1-nomask", "C-ragged-tiles"])
def test_column_route_geometry_f32(gpu, spec):
    check_mode_bound(DC.run_op(_case(spec), "f32"), _ref(spec), "f32", "columns")


# ---- test 2: fused route, mode f32 ---------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("spec", [FUSED_DIL, FUSED_7, FUSED_RECT], ids=["3x3-dil2-nomask", "7x7-mask", "3x5-dil2-mask"])
def test_fused_route_f32(gpu, spec):
    check_mode_bound(DC.run_op(_case(spec), "f32"), _ref(spec), "f32", "fused")


# ---- test 3: exact on integers -------------------------------------------------------------------------------------------------------
def _integer_case(B, C, G, k, H, W, O, pad=1):
    """x integer in [-4, 4], weights integer in [-2, 2], quarter-step offsets (one sample exactly on y = -1, one on y = H, one far outside),
    masks from {0.5, 1, 2}: samples are multiples of 1/32 below 8, so every plane, product and fp32 sum is exact in every fp32-class mode"""
    g = np.random.default_rng(5)
    taps = k * k
    Ho, Wo = DC.out_hw(H, W, k, k, 1, pad, 1)
    table = np.array([0.0, 0.5, -0.5, 1.25, -2.75, 0.25, 40.0, -0.75, 1.0, -1.5], np.float32)
    off = table[g.integers(0, len(table), (B, 2 * G * taps, Ho, Wo))]
    off[:, 0, 0, :] = -1.0 + pad                         # dy of (group 0, tap (0, 0)) in output row 0: exactly y = -1
    off[:, 2 * (taps - 1), Ho - 1, :] = H - ((Ho - 1) - pad + k - 1)      # dy of the last tap in the last row: exactly y = H
    mask = np.array([0.5, 1.0, 2.0], np.float32)[g.integers(0, 3, (B, G * taps, Ho, Wo))]
    c = dict(x=g.integers(-4, 5, (B, C, H, W)).astype(np.float32), offset=off, mask=mask, weight=g.integers(-2, 3, (O, C, k, k)).astype(np.float32),
             bias=None, stride=(1, 1), padding=(pad, pad), dilation=(1, 1))
    # every operand plane holds exactly these values
    assert np.array_equal(c["x"], np.round(c["x"])) and np.abs(c["x"]).max() <= 4
    assert np.array_equal(c["weight"], np.round(c["weight"])) and np.abs(c["weight"]).max() <= 2
    assert np.array_equal(off * 4, np.round(off * 4)) and set(np.unique(mask)) <= {0.5, 1.0, 2.0}
    assert C * taps * 8 * 2 * 32 < 2 ** 24               # |sample| <= 8, |w| <= 2, in units of 1/32: every partial sum is an integer below 2^24
    return c


@functools.lru_cache(maxsize=None)
def _integer_inputs(route):
    c = _integer_case(1, 64, 1 if route == "fused" else 2, 3, 16, 16, 256)
    ref = DC.reference(c)
    assert np.abs(ref).max() > 0
    return c, ref


@pytest.mark.gpu
@pytest.mark.parametrize("compute", ["f32"] + PLANE_MODES)
@pytest.mark.parametrize("route", ["fused", "columns"])
def test_exact_on_integers(gpu, route, compute):
    c, ref = _integer_inputs(route)
    y = np.asarray(DC.run_op(c, compute), np.float64)
    bad = int((y != ref).sum())
    assert bad == 0, f"{bad} of {ref.size} elements differ, max abs diff {np.abs(y - ref).max()}"


_CHILD = """
import sys, numpy as np
sys.path.insert(0, %r); sys.path.insert(0, %r)
import deform_offsets_cases as DC
from test_deform_offsets_gpu import _integer_case
c = _integer_case(2, 32, 2, 3, 32, 32, 24)
ref = DC.reference(c)
rows = (1 << 20) // (9 * 32 * 4) // 64 * 64
pixels = ref.shape[0] * ref.shape[2] * ref.shape[3]
assert pixels == 2048 and rows == 896 and -(-pixels // rows) == 3 and pixels %% rows, (pixels, rows)
for mode in ("f32", "f32_split3", "f32_split2", "f32_half2"):
    y = np.asarray(DC.run_op(c, mode), np.float64)
    bad = int((y != ref).sum())
    assert bad == 0, (mode, bad, float(np.abs(y - ref).max()))
print("exact in 3 chunks")
"""


@pytest.mark.gpu
def test_exact_on_integers_in_column_chunks(gpu):
    """BRN_DEFORM_COL_MB=1: 2048 pixels at 896 rows a chunk = three chunks, the last one ragged (256 rows).  A child process: the switch
    is read once per process."""
    here = os.path.dirname(os.path.abspath(__file__))
    pr = subprocess.run([sys.executable, "-c", _CHILD % (os.path.dirname(here), here)], env=dict(os.environ, BRN_DEFORM_COL_MB="1"), capture_output=True,
                        text=True, timeout=300)
    assert pr.returncode == 0 and "exact in 3 chunks" in pr.stdout, pr.stdout[-2000:] + pr.stderr[-2000:]


# ---- test 4: the seam with the layer -------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _seam_inputs(case):
    """a DeformableConv2d whose offset / modulator convs have all-zero weights: its internal map is the offset bias and 2 sigmoid(0) = 1"""
    B, C, H, W, O, k, s, p = case
    g = np.random.default_rng(21)
    taps = k * k
    Ho, Wo = DC.out_hw(H, W, k, k, s, p, 1)
    n = lambda *sh, std=1.0: (g.standard_normal(sh) * std).astype(np.float32)
    t = {"offset_conv.weight": np.zeros((2 * taps, C, k, k), np.float32), "offset_conv.bias": n(2 * taps, std=1.5),
         "modulator_conv.weight": np.zeros((taps, C, k, k), np.float32), "modulator_conv.bias": np.zeros(taps, np.float32),
         "regular_conv.weight": n(O, C, k, k, std=(C * taps) ** -0.5), "regular_conv.bias": n(O, std=0.1)}
    x = n(B, C, H, W)
    offset = np.ascontiguousarray(np.broadcast_to(t["offset_conv.bias"].reshape(1, -1, 1, 1), (B, 2 * taps, Ho, Wo)))
    c = dict(x=x, offset=offset, mask=None, weight=t["regular_conv.weight"], bias=t["regular_conv.bias"], stride=(s, s), padding=(p, p), dilation=(1, 1))
    return t, c


def _layer(case, t, x, compute):
    import candle_birefnet_amd as cb
    from candle_birefnet_amd import ops
    B, C, H, W, O, k, s, p = case
    layer = cb.DeformableConv2d.new(C, O, k, s, p, cb.VarBuilder.from_tensors(t), mode="deformable")
    ops.set_compute(compute)
    try:
        return np.asarray(layer.forward(x))
    finally:
        ops.set_compute("f32")


SEAM = [(S1, m) for m in ["f32"] + PLANE_MODES] + [(S3, m) for m in ["f32"] + PLANE_MODES] + [(S1, "bf16"), (S1, "f16")]


@pytest.mark.gpu
@pytest.mark.parametrize("case,compute", SEAM, ids=[f"{'S1' if c is S1 else 'S3'}-{m}" for c, m in SEAM])
def test_seam_with_the_layer(gpu, case, compute):
    """the layer's constants handed in as a tensor, no mask: the fused route returns the layer's bits; the same data as two offset groups
    with duplicated offsets goes through the column route and agrees with it within the mode's bound"""
    t, c = _seam_inputs(case)
    y_layer = _layer(case, t, c["x"], compute)
    y_op = np.asarray(DC.run_op(c, compute))
    assert y_op.shape == y_layer.shape and np.isfinite(y_op).all()
    assert y_op.tobytes() == y_layer.tobytes(), f"max abs diff {np.abs(y_op.astype(np.float64) - y_layer).max():.3e}"
    y_col = DC.run_op(c, compute, offset=np.tile(c["offset"], (1, 2, 1, 1)))
    check_mode_bound(y_col, y_op.astype(np.float64), compute, "columns vs fused")


# ---- test 5: every mode against the restatement -------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("compute", ALL_MODES)
@pytest.mark.parametrize("spec", [COL_MODES, FUSED_RECT], ids=["columns", "fused"])
def test_every_mode_against_the_restatement(gpu, spec, compute):
    check_mode_bound(DC.run_op(_case(spec), compute), _ref(spec, compute), compute, "fused" if spec is FUSED_RECT else "columns")


# ---- test 6: invariants ---------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("spec", [COL_A, FUSED_7], ids=["columns", "fused"])
def test_repeat_and_memory_side_give_the_same_bits(gpu, spec):
    import torch
    c = _case(spec)
    y1, y2 = np.asarray(DC.run_op(c, "f32")), np.asarray(DC.run_op(c, "f32"))
    assert y1.tobytes() == y2.tobytes()
    dev = {n: torch.from_numpy(c[n]).cuda() for n in ("x", "offset", "mask") if c[n] is not None}
    yd = DC.run_op(c, "f32", **dev)
    torch.cuda.synchronize()
    assert yd.is_cuda and yd.cpu().numpy().tobytes() == y1.tobytes()


@pytest.mark.gpu
def test_ops_infers_the_offset_groups(gpu):
    """offset.shape[1] / (2 kh kw) groups: four groups of which only the last one's offsets differ must move exactly that group's share"""
    c = dict(_case(COL_A))
    y4 = np.asarray(DC.run_op(c, "f32"), np.float64)
    check_mode_bound(y4, _ref(COL_A), "f32", "G = 4")
    taps = 6
    one = dict(c, offset=c["offset"][:, :2 * taps], mask=c["mask"][:, :taps])          # the first group's offsets for every channel: G = 1
    y1 = np.asarray(DC.run_op(one, "f32"), np.float64)
    ref1 = DC.restatement(one["x"], one["offset"], one["mask"], one["weight"], one["bias"], one["stride"], one["padding"], one["dilation"])
    check_mode_bound(y1, ref1, "f32", "G = 1")
    assert np.abs(y4 - y1).max() > 1e-2
