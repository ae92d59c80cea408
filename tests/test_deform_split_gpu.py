"""Deformable convs in the plane modes (f32_split3 / f32_split2 / f32_half2) run on the split kernels: the modulated-deformable A loader of
kernels/gemm_split.hip (DeformLoader), behind launch_gemm.  brn_deform_conv2d_forward builds its weights with the op's planes, so these
tests reach it through DeformableConv2d under ops.set_compute.

Cases are (B, C, H, W, O, k, stride, pad), the smallest that reach every path:
  S1  two K tiles per tap, full N tiles: the warp-specialised 128 x 128 kernel
  S2  M = 338 (a tile spans two images), K = 3136 on a small M: the split-K plan
  S3  three K tiles per tap, stride 2, no padding, a partial N tile: the 4-wave 64 x 64 kernel
  S4  one K tile, M = 105 (a 64-row tile spans three images, the last tile is ragged), N = 8
  S5  7 x 7 taps on a ragged map (test 3 only)"""
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import torch_ref as R

S1 = (1, 64, 16, 16, 256, 3, 1, 1)
S2 = (2, 64, 13, 13, 256, 7, 1, 3)
S3 = (1, 96, 17, 15, 40, 3, 2, 0)
S4 = (3, 32, 5, 7, 8, 1, 1, 0)
S5 = (1, 64, 20, 12, 256, 7, 1, 3)
PLANE_MODES = ["f32_split3", "f32_split2", "f32_half2"]
TOL = {"f32_split3": 2e-4, "f32_half2": 2e-4, "f32_split2": 5e-4}     # tools/deform_fuzz.py, relative to max(1, max |ref|)


def _rng(seed):
    return np.random.default_rng(seed)


def _out_hw(case):
    B, C, H, W, O, k, s, p = case
    return (H + 2 * p - k) // s + 1, (W + 2 * p - k) // s + 1


def _forward(case, t, x, compute, mode="deformable"):
    import candle_birefnet_amd as cb
    from candle_birefnet_amd import ops
    B, C, H, W, O, k, s, p = case
    layer = cb.DeformableConv2d.new(C, O, k, s, p, cb.VarBuilder.from_tensors(t), mode=mode)
    ops.set_compute(compute)
    try:
        return np.asarray(layer.forward(x))
    finally:
        ops.set_compute("f32")


def _conv(case, t, x, compute):
    from candle_birefnet_amd import ops
    B, C, H, W, O, k, s, p = case
    ops.set_compute(compute)
    try:
        return np.asarray(ops.conv2d(x, t["regular_conv.weight"], t["regular_conv.bias"], stride=s, padding=p))
    finally:
        ops.set_compute("f32")


def _ref_fp64(case, t, x):
    """the fp64 restatement with the offsets / modulator the layer's own convs produce (in fp64)"""
    B, C, H, W, O, k, s, p = case
    xt = torch.from_numpy(x).double()
    td = {n: torch.from_numpy(a).double() for n, a in t.items()}
    off = F.conv2d(xt, td["offset_conv.weight"], td["offset_conv.bias"], stride=s, padding=p)
    msk = 2.0 / (torch.exp(-F.conv2d(xt, td["modulator_conv.weight"], td["modulator_conv.bias"], stride=s, padding=p)) + 1.0)
    return R.deform_conv2d(xt, off, msk, td["regular_conv.weight"], td["regular_conv.bias"], s, p).numpy()


# ---- test 1: the mode's arithmetic --------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _zero_offset_inputs(case):
    B, C, H, W, O, k, s, p = case
    g = _rng(11)
    K = C * k * k
    t = {"offset_conv.weight": np.zeros((2 * k * k, C, k, k), np.float32), "offset_conv.bias": np.zeros(2 * k * k, np.float32),
         "modulator_conv.weight": np.zeros((k * k, C, k, k), np.float32), "modulator_conv.bias": np.zeros(k * k, np.float32),
         "regular_conv.weight": (g.standard_normal((O, C, k, k)) * K ** -0.5).astype(np.float32), "regular_conv.bias": np.zeros(O, np.float32)}
    return t, g.standard_normal((B, C, H, W)).astype(np.float32)


@pytest.mark.gpu
@pytest.mark.parametrize("case", [S1, S2, S3], ids=["S1", "S2", "S3"])
def test_deformable_conv_runs_in_the_modes_arithmetic(gpu, case):
    """Zero offsets and a modulator of exactly 1: every tap samples one pixel with weight 1, so the A operand is that of the plain conv bit
    for bit and the deformable conv must carry the plain conv's two-plane truncation (~2^-16 per product), not the fp32 kernel's reorder
    noise (~2^-24 per term): max|y_def - y_conv| <= max|y_conv - y_exact| / 8, with y_conv = ops.conv2d under f32_split2 and y_exact
    under f32.  On the fp32-MFMA gather kernel y_def sits beside y_exact and the bound fails (ratio 1).

    The deformable conv is launched with the plan of the mode's plain conv (same tile class, same split-K), so it sums every element in the
    same order: measured on MI355X max|y_def - y_conv| = 0 in all three cases against max|y_conv - y_exact| = 2.2e-5 / 1.8e-5 / 1.4e-5.
    (With another split-K than the conv's — 4 against 1 in S1 — the fp32 summation-order noise alone is 3.3e-6, a seventh of the truncation.)"""
    t, x = _zero_offset_inputs(case)
    y_def = _forward(case, t, x, "f32_split2").astype(np.float64)
    y_conv = _conv(case, t, x, "f32_split2").astype(np.float64)
    y_exact = _conv(case, t, x, "f32").astype(np.float64)
    d_mode = np.abs(y_def - y_conv).max()
    d_trunc = np.abs(y_conv - y_exact).max()
    print(f"max|y_def - y_conv| {d_mode:.3e}, max|y_conv - y_exact| {d_trunc:.3e}")
    assert d_trunc > 0.0
    assert d_mode <= d_trunc / 8


# ---- test 2: exact on integers ---------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _integer_inputs(case):
    """x integer in [-4, 4], weights integer in [-2, 2], constant quarter-step offsets (zero offset / modulator weights, the offsets are the
    offset conv's bias), modulator 2 sigmoid(0) = 1.  Samples are multiples of 1/16 below 4: every plane, product and fp32 sum is exact."""
    B, C, H, W, O, k, s, p = case
    Ho, Wo = _out_hw(case)
    g = _rng(5)
    kk = k * k
    table = [0.0, 0.5, -0.5, 1.25, -2.75, 0.25, 40.0, -0.75, 1.0, -1.5]         # 40: far outside every map here
    off = np.array([table[c % len(table)] for c in range(2 * kk)], np.float32)
    off[0] = -1.0 + p                                    # dy of tap (0, 0): output row 0 samples exactly y = -1 (contributes 0)
    if kk > 1:
        off[2 * (kk - 1)] = H - ((Ho - 1) * s - p + k - 1)   # dy of the last tap: the last output row samples exactly y = Hin (contributes 0)
    t = {"offset_conv.weight": np.zeros((2 * kk, C, k, k), np.float32), "offset_conv.bias": off,
         "modulator_conv.weight": np.zeros((kk, C, k, k), np.float32), "modulator_conv.bias": np.zeros(kk, np.float32),
         "regular_conv.weight": g.integers(-2, 3, (O, C, k, k)).astype(np.float32), "regular_conv.bias": np.zeros(O, np.float32)}
    x = g.integers(-4, 5, (B, C, H, W)).astype(np.float32)
    xt = torch.from_numpy(x).double()
    offm = torch.from_numpy(off).double().view(1, -1, 1, 1).expand(B, 2 * kk, Ho, Wo)
    ref = R.deform_conv2d(xt, offm, torch.ones(B, kk, Ho, Wo, dtype=torch.float64), torch.from_numpy(t["regular_conv.weight"]).double(),
                          torch.zeros(O, dtype=torch.float64), s, p).numpy()
    assert K_exact(case)
    return t, x, ref


def K_exact(case):
    B, C, H, W, O, k, s, p = case
    return C * k * k * 8 * 16 < 2 ** 24


@pytest.mark.parametrize("case", [S1, S2, S3, S4], ids=["S1", "S2", "S3", "S4"])
def test_integer_reference_agrees_with_oracle(case):
    """(CPU) the fp64 restatement and the oracle's deformable conv agree exactly on the integer inputs of the test below"""
    from oracle import oracle as ORC
    B, C, H, W, O, k, s, p = case
    t, x, ref = _integer_inputs(case)
    y = ORC.deform_conv2d(x, t["offset_conv.weight"], t["offset_conv.bias"], t["modulator_conv.weight"], t["modulator_conv.bias"],
                          t["regular_conv.weight"], t["regular_conv.bias"], k, s, p, 1)
    assert np.abs(ref).max() > 0
    assert np.array_equal(y.astype(np.float64), ref)


@pytest.mark.gpu
@pytest.mark.parametrize("compute", PLANE_MODES)
@pytest.mark.parametrize("case", [S1, S2, S3, S4], ids=["S1", "S2", "S3", "S4"])
def test_exact_on_integers(gpu, case, compute):
    """Quarter-step offsets (0, +-0.5, 1.25, -2.75, samples exactly on y = -1 and y = Hin, one far outside): the output equals the fp64
    restatement element for element, and three calls give the same bits."""
    t, x, ref = _integer_inputs(case)
    ys = [_forward(case, t, x, compute) for _ in range(3)]
    bad = int((ys[0].astype(np.float64) != ref).sum())
    assert bad == 0, f"{bad} of {ref.size} elements differ, max abs diff {np.abs(ys[0] - ref).max()}"
    assert ys[1].tobytes() == ys[0].tobytes() and ys[2].tobytes() == ys[0].tobytes()


# ---- test 3: random offsets against fp64 ---------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _random_inputs(case):
    """the weight recipe of test_ops_gpu.py::test_deform_conv2d: offsets of about 1.5 px, some samples leave the map"""
    B, C, H, W, O, k, s, p = case
    g = _rng(3)
    n = lambda *sh, std=1.0: (g.standard_normal(sh) * std).astype(np.float32)
    K = C * k * k
    t = {"offset_conv.weight": n(2 * k * k, C, k, k, std=1.5 * K ** -0.5), "offset_conv.bias": n(2 * k * k, std=0.3),
         "modulator_conv.weight": n(k * k, C, k, k, std=K ** -0.5), "modulator_conv.bias": n(k * k, std=0.1),
         "regular_conv.weight": n(O, C, k, k, std=K ** -0.5), "regular_conv.bias": n(O, std=0.1)}
    x = n(B, C, H, W)
    return t, x, _ref_fp64(case, t, x)


@pytest.mark.gpu
@pytest.mark.parametrize("compute", PLANE_MODES)
@pytest.mark.parametrize("case", [S1, S2, S3, S4, S5], ids=["S1", "S2", "S3", "S4", "S5"])
def test_random_offsets_vs_fp64(gpu, case, compute):
    t, x, ref = _random_inputs(case)
    y = _forward(case, t, x, compute).astype(np.float64)
    assert y.shape == ref.shape and np.isfinite(y).all()
    err = np.abs(y - ref).max() / max(1.0, np.abs(ref).max())
    print(f"{compute}: max err {err:.3e} (tolerance {TOL[compute]:.0e})")
    assert err <= TOL[compute]


# ---- test 4: f32_half2 beyond its range ------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_half2_is_never_silently_wrong(gpu):
    """One input pixel of 9000 (the modulated sample reaches the fp16 planes' ceiling with the mode's operand scale): every output element is
    either non-finite or within the mode's tolerance of the fp64 result."""
    case = S1
    t, x = _zero_offset_inputs(case)
    x = x.copy()
    x[0, 5, 7, 9] = 9000.0
    ref = _ref_fp64(case, t, x)
    y = _forward(case, t, x, "f32_half2").astype(np.float64)
    fin = np.isfinite(y)
    err = np.abs(np.where(fin, y, ref) - ref).max() / max(1.0, np.abs(ref).max())
    print(f"{int((~fin).sum())} of {y.size} non-finite, max err of the finite ones {err:.3e}")
    assert err <= TOL["f32_half2"]
