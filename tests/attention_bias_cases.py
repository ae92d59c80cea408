"""What tests/test_attention_bias_gpu.py and tests/test_attention_bias_cpu.py share: the case list of brn_attention_forward, its inputs,
the float64 reference (forward_standard of swin.rs:266-311 without the projection), the 16-bit rounding and the refusal list."""
import ctypes
import functools

import numpy as np
import torch

HD = 32
SCALE = HD ** -0.5
# (batch, heads, N, n_bias) -> std of q and k.  0.1, 1.0 and 3.0 each appear; the repeating cases (n_bias > 1) carry the mask regime
CASES = [
    ((2, 4, 16, 1), 1.0),        # test_flash_bias.rs
    ((8, 4, 49, 4), 3.0),        # test_flash_bias.rs
    ((8, 6, 144, 1), 1.0),       # Swin-L window, broadcast bias
    ((8, 6, 144, 8), 1.0),       # Swin-L window, repeating bias
    ((3, 3, 1, 1), 3.0),         # N = 1
    ((4, 2, 17, 2), 0.1),        # ragged N just above one tile
    ((2, 1, 143, 2), 3.0),       # ragged N just below the maximum
    ((1, 300, 16, 1), 0.1),      # many heads, batch 1
    ((176, 6, 144, 4), 1.0),     # more workgroups than one residency round on 256 CUs
    ((5, 2, 50, 0), 1.0),        # no bias
]
SHAPES = [c for c, _ in CASES]
QK_STD = dict(CASES)
LARGE_GRID = [(1, 300, 16, 1), (176, 6, 144, 4)]
S16_ULP = {"bf16": 2.0 ** -8, "f16": 2.0 ** -11}


@functools.lru_cache(maxsize=None)
def make_inputs(shape, qk_std=None, mask_value=-100.0):
    """standard-normal draws: q, k of std qk_std, v of std 1, bias of std 0.5 / scale; in the repeating cases ~30 % of the bias entries
    are lowered by a further |mask_value| / scale (the mask regime of swin.rs:636-650; mask_value 0 = no mask).  The same shape gives the
    same draws whatever qk_std and mask_value are.  The arrays are shared between tests: read-only."""
    batch, heads, N, n_bias = shape
    qk_std = QK_STD[shape] if qk_std is None else qk_std
    rng = np.random.default_rng(1000 + SHAPES.index(shape))
    q = (rng.standard_normal((batch, heads, N, HD)) * qk_std).astype(np.float32)
    k = (rng.standard_normal((batch, heads, N, HD)) * qk_std).astype(np.float32)
    v = rng.standard_normal((batch, heads, N, HD)).astype(np.float32)
    bias = None
    if n_bias > 0:
        b = rng.standard_normal((n_bias, heads, N, N)) * 0.5
        if n_bias > 1:
            b = b + np.where(rng.random((n_bias, heads, N, N)) < 0.3, mask_value, 0.0)
        bias = (b / SCALE).astype(np.float32)
        bias.setflags(write=False)
    for a in (q, k, v):
        a.setflags(write=False)
    return q, k, v, bias


def round_s16(a, s16="bf16"):
    """round-to-nearest-even fp32 -> bf16 or fp16 -> float64 (_bf16_round of tests/test_ops_gpu.py)"""
    return torch.from_numpy(np.array(a, np.float32)).to(torch.float16 if s16 == "f16" else torch.bfloat16).to(torch.float64).numpy()


def scores(q, k, bias, n_bias, scale=SCALE):
    """scale * (q k^T + bias[b % n_bias]) - row max, float64"""
    q, k = np.asarray(q, np.float64), np.asarray(k, np.float64)
    s = q @ k.transpose(0, 1, 3, 2)
    if bias is not None:
        s = s + np.asarray(bias, np.float64)[np.arange(q.shape[0]) % n_bias]
    s = s * scale
    return s - s.max(-1, keepdims=True)


def reference(q, k, v, bias, n_bias, scale=SCALE):
    """softmax(scale * (q k^T + bias[b % n_bias])) v in float64 (swin.rs:278-303 with the scale factored out, as swin.rs:233-252 does)"""
    p = np.exp(scores(q, k, bias, n_bias, scale))
    return (p / p.sum(-1, keepdims=True)) @ np.asarray(v, np.float64)


@functools.lru_cache(maxsize=None)
def case_reference(shape, s16=None, mask_value=-100.0):
    """the reference of a case, on q, k, v rounded to the 16-bit type when s16 is given; computed once, read-only"""
    q, k, v, bias = make_inputs(shape, mask_value=mask_value)
    if s16:
        q, k, v = (round_s16(a, s16) for a in (q, k, v))
    r = reference(q, k, v, bias, shape[3])
    r.setflags(write=False)
    return r


def raw_call(lib, q, k, v, batch, heads, N, head_dim, bias, n_bias, scale, y):
    """brn_attention_forward on host buffers with the integers exactly as given (the refusals need shapes the wrappers cannot express)"""
    ptr = lambda a: None if a is None else a.ctypes.data_as(ctypes.c_void_p)
    st = lib.brn_attention_forward(ptr(q), ptr(k), ptr(v), batch, heads, N, head_dim, ptr(bias), n_bias, scale, ptr(y), 0, 0, None)
    return st, (lib.brn_last_error() or b"").decode()


def refusals():
    """(name, arguments of raw_call after lib, word the message must contain): every limit of the header, on buffers large enough for
    whatever shape is named"""
    buf = lambda: np.zeros(8 * 2 * 145 * 64, np.float32)
    q, k, v, y, bias = buf(), buf(), buf(), buf(), np.zeros(4 * 2 * 145 * 145, np.float32)
    return [
        ("head_dim 64", (q, k, v, 2, 2, 16, 64, bias, 1, 0.0, y), "head_dim must be 32"),
        ("N 0", (q, k, v, 2, 2, 0, 32, bias, 1, 0.0, y), "1 <= N <= 144"),
        ("N 145", (q, k, v, 2, 2, 145, 32, bias, 1, 0.0, y), "1 <= N <= 144"),
        ("batch 6, n_bias 4", (q, k, v, 6, 2, 16, 32, bias, 4, 0.0, y), "batch % n_bias == 0"),
        ("bias with n_bias 0", (q, k, v, 2, 2, 16, 32, bias, 0, 0.0, y), "NULL exactly when n_bias == 0"),
        ("negative scale", (q, k, v, 2, 2, 16, 32, bias, 1, -0.5, y), "scale must be finite and >= 0"),
        ("y aliases q", (q, k, v, 2, 2, 16, 32, bias, 1, 0.0, q), "alias"),
    ]
