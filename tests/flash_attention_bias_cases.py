"""What tests/test_flash_attention_bias_gpu.py and tests/test_flash_attention_bias_cpu.py share: the case list of
brn_flash_attention_bias_forward, its seeded inputs, the float64 reference
    softmax(scale * (q k^T + bias[b % n_bias]) [causal exclusion]) v
(forward_standard of swin.rs:266-311 with the scale factored out as swin.rs:231-252 does, on sequences of any length), the refusal list
and a raw ctypes call.  The bias is [n_bias, heads, seq_q, seq_kv], heads-major in either layout of q / k / v, and is never rounded."""
import functools

import numpy as np

from flash_attention_cases import S16_ULP, T, round_s16, to_bhsd  # noqa: F401  (re-exported to the two test files)

# (batch, seq_q, seq_kv, heads, head_dim, causal, n_bias, kind) -> layout.  Kinds:
#   std      q, k, v standard normal; bias standard normal x sqrt(head_dim), the scale of q . k itself; scale head_dim^-0.5
#   swin16 / swin24   the bias swin.rs builds for a window of 16 / 24: a relative-position table [(2 ws - 1)^2, heads] (normal x 0.5)
#            gathered by the relative index, plus the shifted-window mask (0 where two positions share a region, -100 otherwise; the 4
#            patterns split the window at ws - ws / 2 along neither, one or both axes), all divided by scale (masked entries: -565.7)
#   large    q, k integers in [-4, 4], bias EVEN integers in [-120, 120], scale 0.5: every score exact in fp32, bf16 and fp16, and the row
#            maxima overflow exp unless the maximum is subtracted
#   rising / falling   q, k integers in [-2, 2], bias an integer in [-2, 2] +- 4 (j // 4), scale 0.5: the row maximum rises in every K / V
#            tile (the weight ends in the last one) or falls from the first — the rescale run is driven by the bias alone
#   pad      std, with bias[..., 130:] = -inf in pattern 0 and bias[..., 60:] = -inf in pattern 1 (inside the first K / V tile)
CASES = [
    ((2, 1, 1, 2, 32, 0, 1, "std"), "bhsd"),                 # seq 1
    ((2, 17, 17, 3, 64, 0, 2, "std"), "bshd"),               # ragged, seq_kv % 4 != 0 (4-byte loads), two patterns
    ((2, T - 1, T - 1, 2, 32, 0, 1, "std"), "bhsd"),         # around the K / V tile
    ((1, T, T, 2, 128, 0, 1, "std"), "bshd"),
    ((2, T + 1, T + 1, 2, 64, 0, 2, "std"), "bhsd"),
    ((4, 145, 145, 3, 32, 0, 2, "std"), "bhsd"),             # the first N beyond brn_attention_forward, batch 4 over 2 patterns
    ((2, 300, 300, 3, 64, 0, 1, "std"), "bshd"),             # several tiles, 16-byte loads (300 % 4 == 0), ragged last tile
    ((2, 300, 300, 2, 128, 0, 2, "std"), "bhsd"),
    ((2, 5, 301, 2, 64, 0, 1, "std"), "bshd"),               # cross shapes, both load paths
    ((2, 300, 7, 2, 64, 0, 2, "std"), "bhsd"),
    ((2, 17, 17, 3, 64, 1, 1, "std"), "bhsd"),               # causal + bias
    ((2, 300, 300, 2, 64, 1, 2, "std"), "bshd"),
    ((1, 257, 257, 2, 128, 1, 1, "std"), "bhsd"),
    ((8, 256, 256, 3, 32, 0, 4, "swin16"), "bhsd"),          # Swin windows 16 / 24
    ((4, 576, 576, 2, 32, 0, 4, "swin24"), "bshd"),
    ((2, 300, 300, 2, 64, 0, 1, "large"), "bhsd"),
    ((2, 40, 300, 2, 64, 0, 1, "rising"), "bshd"),
    ((2, 40, 300, 2, 64, 0, 1, "falling"), "bhsd"),
    ((2, 70, 200, 2, 64, 0, 2, "pad"), "bshd"),
]
SHAPES = [c for c, _ in CASES]
LAYOUT = dict(CASES)
SEED0 = 3007                   # about one seed in four leaves 'rising' below 0.99 of its weight in the last tile; this base does not
PAD_FROM = (130, 60)           # kind pad: the first -inf key of pattern 0 and of pattern 1


def case_id(shape):
    b, sq, skv, h, d, causal, nb, kind = shape
    return f"{b}x{sq}x{skv}x{h}x{d}-{LAYOUT[shape]}{'-causal' if causal else ''}-nb{nb}-{kind}"


def case_scale(shape):
    """the scale argument of the call: 0 = head_dim^-0.5"""
    return 0.0 if shape[7] in ("std", "swin16", "swin24", "pad") else 0.5


def swin_bias(ws, heads, scale, rng):
    """[4, heads, ws^2, ws^2]: (relative_position_bias_table[relative_position_index] + shifted-window mask) / scale, and the mask alone
    ([4, ws^2, ws^2], 0 / -100)"""
    table = rng.standard_normal(((2 * ws - 1) ** 2, heads)) * 0.5
    yy, xx = np.divmod(np.arange(ws * ws), ws)
    rel = (yy[:, None] - yy[None, :] + ws - 1) * (2 * ws - 1) + (xx[:, None] - xx[None, :] + ws - 1)
    rpb = table[rel].transpose(2, 0, 1)                                   # [heads, N, N]
    cut = ws - ws // 2
    masks = []
    for split_y, split_x in ((0, 0), (0, 1), (1, 0), (1, 1)):
        region = (yy >= cut) * 2 * split_y + (xx >= cut) * split_x
        masks.append(np.where(region[:, None] == region[None, :], 0.0, -100.0))
    masks = np.stack(masks)
    return (rpb[None] + masks[:, None]) / scale, masks


@functools.lru_cache(maxsize=None)
def make_inputs(shape):
    """q, k, v in the case's layout and the bias [n_bias, heads, seq_q, seq_kv] (fp32, contiguous).  Shared between tests: read-only."""
    batch, seq_q, seq_kv, heads, hd, causal, n_bias, kind = shape
    rng = np.random.default_rng(SEED0 + SHAPES.index(shape))
    v = rng.standard_normal((batch, heads, seq_kv, hd))
    if kind in ("std", "pad", "swin16", "swin24"):
        q = rng.standard_normal((batch, heads, seq_q, hd))
        k = rng.standard_normal((batch, heads, seq_kv, hd))
        if kind.startswith("swin"):
            bias, _ = swin_bias(int(kind[4:]), heads, hd ** -0.5, rng)
            assert bias.shape == (n_bias, heads, seq_q, seq_kv)
        else:
            bias = rng.standard_normal((n_bias, heads, seq_q, seq_kv)) * np.sqrt(hd)
        if kind == "pad":
            for pattern, first in enumerate(PAD_FROM):
                bias[pattern, :, :, first:] = -np.inf
    else:
        r = 4 if kind == "large" else 2
        q = rng.integers(-r, r + 1, (batch, heads, seq_q, hd)).astype(np.float64)
        k = rng.integers(-r, r + 1, (batch, heads, seq_kv, hd)).astype(np.float64)
        if kind == "large":
            bias = 2.0 * rng.integers(-60, 61, (n_bias, heads, seq_q, seq_kv))
        else:
            bias = rng.integers(-2, 3, (n_bias, heads, seq_q, seq_kv)) + (4.0 if kind == "rising" else -4.0) * (np.arange(seq_kv) // 4)
    out = []
    for a in (q, k, v):
        a = np.ascontiguousarray(to_bhsd(a, LAYOUT[shape]), dtype=np.float32)     # bhsd -> bshd is the same transpose
        a.setflags(write=False)
        out.append(a)
    bias = np.ascontiguousarray(bias, dtype=np.float32)
    bias.setflags(write=False)
    return tuple(out) + (bias,)


def probabilities(q, k, bias, layout="bhsd", causal=False, scale=None):
    """softmax(scale * (q k^T + bias[b % n_bias]) [causal]) in float64, [batch, heads, seq_q, seq_kv]; bias None = no bias"""
    q, k = (to_bhsd(np.asarray(a, np.float64), layout) for a in (q, k))
    scale = q.shape[-1] ** -0.5 if not scale else scale
    s = q @ k.transpose(0, 1, 3, 2)
    if bias is not None:
        s = s + np.asarray(bias, np.float64)[np.arange(q.shape[0]) % bias.shape[0]]
    s = s * scale
    if causal:
        s = np.where(np.arange(s.shape[-1])[None, :] <= np.arange(s.shape[-2])[:, None], s, -np.inf)
    p = np.exp(s - s.max(-1, keepdims=True))
    return p / p.sum(-1, keepdims=True)


def reference(q, k, v, bias, layout="bhsd", causal=False, scale=None):
    """the float64 result, in `layout`"""
    y = probabilities(q, k, bias, layout, causal, scale) @ to_bhsd(np.asarray(v, np.float64), layout)
    return np.ascontiguousarray(to_bhsd(y, layout))


@functools.lru_cache(maxsize=None)
def case_reference(shape, s16=None, with_bias=True):
    """the reference of a case, on q, k, v rounded to the 16-bit type when s16 is given (the bias is never rounded); with_bias False: the
    bias-free reference of the same q, k, v.  Computed once, read-only."""
    q, k, v, bias = make_inputs(shape)
    if s16:
        q, k, v = (round_s16(a, s16) for a in (q, k, v))
    r = reference(q, k, v, bias if with_bias else None, LAYOUT[shape], shape[5], case_scale(shape))
    r.setflags(write=False)
    return r


def f32_bound(ref, tol=3e-5):
    return tol * max(1.0, float(np.abs(ref).max()))


def s16_bound(ref, v, s16):
    return S16_ULP[s16] * float(np.abs(v).max()) + f32_bound(ref)


def raw_call(lib, q, k, v, batch, seq_q, seq_kv, heads, head_dim, layout, causal, bias, n_bias, scale, y, loc=0):
    """brn_flash_attention_bias_forward with the integers exactly as given; q, k, v, bias, y: numpy arrays, integers taken as addresses, or None"""
    ptr = lambda a: a if a is None or isinstance(a, int) else a.ctypes.data
    st = lib.brn_flash_attention_bias_forward(ptr(q), ptr(k), ptr(v), batch, seq_q, seq_kv, heads, head_dim, layout, causal, ptr(bias), n_bias, scale,
                                              ptr(y), loc, 0, None)
    return st, (lib.brn_last_error() or b"").decode()


@functools.lru_cache(maxsize=None)
def _refusal_buffers():
    return tuple(np.zeros(2 * 2 * 32 * 256, np.float32) for _ in range(5))


def refusals():
    """(name, arguments of raw_call after lib, words the message must contain): every limit of brn_flash_attention_forward with the same
    words (the list of tests/flash_attention_cases.py with a one-pattern bias put in), then the limits of the bias.  The buffers hold what
    the well-formed neighbours of each call would read; the refused calls read nothing."""
    q, k, v, y, bias = _refusal_buffers()
    a, ab = q.ctypes.data, bias.ctypes.data
    assert a % 16 == 0 and ab % 16 == 0
    b1 = (bias, 1)
    return [
        ("head_dim 48", (q, k, v, 2, 16, 16, 2, 48, 0, 0) + b1 + (0.0, y), "head_dim must be 32, 64 or 128"),
        ("head_dim 256", (q, k, v, 2, 16, 16, 2, 256, 0, 0) + b1 + (0.0, y), "head_dim must be 32, 64 or 128"),
        ("seq_q 0", (q, k, v, 2, 0, 16, 2, 32, 0, 0) + b1 + (0.0, y), "1 <= seq_q, seq_kv <= 65536"),
        ("seq_kv 0", (q, k, v, 2, 16, 0, 2, 32, 0, 0) + b1 + (0.0, y), "1 <= seq_q, seq_kv <= 65536"),
        ("seq_q 65537", (q, k, v, 1, 65537, 16, 1, 32, 0, 0) + b1 + (0.0, y), "1 <= seq_q, seq_kv <= 65536"),
        ("seq_kv 65537", (q, k, v, 1, 16, 65537, 1, 32, 0, 0) + b1 + (0.0, y), "1 <= seq_q, seq_kv <= 65536"),
        ("batch 0", (q, k, v, 0, 16, 16, 2, 32, 0, 0) + b1 + (0.0, y), "batch >= 1, heads >= 1"),
        ("heads 0", (q, k, v, 2, 16, 16, 0, 32, 0, 0) + b1 + (0.0, y), "batch >= 1, heads >= 1"),
        ("2^31 query tiles", (q, k, v, 32768, 65536, 16, 16, 32, 0, 0) + b1 + (0.0, y), "batch * heads * ceil(seq_q / 16) < 2^31"),
        ("layout 2", (q, k, v, 2, 16, 16, 2, 32, 2, 0) + b1 + (0.0, y), "layout must be 0"),
        ("causal 2", (q, k, v, 2, 16, 16, 2, 32, 0, 2) + b1 + (0.0, y), "causal must be 0 or 1"),
        ("causal, seq_q != seq_kv", (q, k, v, 2, 16, 17, 2, 32, 0, 1) + b1 + (0.0, y), "causal requires seq_q == seq_kv"),
        ("negative scale", (q, k, v, 2, 16, 16, 2, 32, 0, 0) + b1 + (-0.5, y), "scale must be finite and >= 0"),
        ("infinite scale", (q, k, v, 2, 16, 16, 2, 32, 0, 0) + b1 + (float("inf"), y), "scale must be finite and >= 0"),
        ("NaN scale", (q, k, v, 2, 16, 16, 2, 32, 0, 0) + b1 + (float("nan"), y), "scale must be finite and >= 0"),
        ("null q", (None, k, v, 2, 16, 16, 2, 32, 0, 0) + b1 + (0.0, y), "null q, k, v or y"),
        ("null y", (q, k, v, 2, 16, 16, 2, 32, 0, 0) + b1 + (0.0, None), "null q, k, v or y"),
        ("y is q", (q, k, v, 2, 16, 16, 2, 32, 0, 0) + b1 + (0.0, q), "overlap"),
        ("y overlaps the end of v", (q, k, v, 2, 16, 16, 2, 32, 0, 0) + b1 + (0.0, v.ctypes.data + 4 * (2 * 16 * 2 * 32 - 4)), "overlap"),
        ("misaligned device k", (q, a + 4096 + 4, v, 2, 16, 16, 2, 32, 0, 0) + b1 + (0.0, y, 1), "16-byte aligned"),
        ("n_bias -1", (q, k, v, 2, 16, 16, 2, 32, 0, 0, bias, -1, 0.0, y), "n_bias >= 0"),
        ("bias NULL, n_bias 1", (q, k, v, 2, 16, 16, 2, 32, 0, 0, None, 1, 0.0, y), "bias must be NULL exactly when n_bias == 0"),
        ("bias given, n_bias 0", (q, k, v, 2, 16, 16, 2, 32, 0, 0, bias, 0, 0.0, y), "bias must be NULL exactly when n_bias == 0"),
        ("batch 3, n_bias 2", (q, k, v, 3, 16, 16, 2, 32, 0, 0, bias, 2, 0.0, y), "batch % n_bias == 0"),
        ("y is the bias", (q, k, v, 2, 16, 16, 2, 32, 0, 0, bias, 1, 0.0, bias), "overlap"),
        ("y overlaps the end of the bias", (q, k, v, 2, 16, 16, 2, 32, 0, 0, bias, 1, 0.0, ab + 4 * (2 * 16 * 16 - 4)), "overlap"),
        ("misaligned device bias", (q, k, v, 2, 16, 16, 2, 32, 0, 0, ab + 4096 + 4, 1, 0.0, y, 1), "16-byte aligned"),
    ]
