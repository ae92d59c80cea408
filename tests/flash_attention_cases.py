"""What tests/test_flash_attention_gpu.py and tests/test_flash_attention_cpu.py share: the case list of brn_flash_attention_forward, its
seeded inputs, the float64 reference (standard_attention of examples/bench_flash_attn.rs:89-95 plus the causal exclusion, layout-aware),
the 16-bit rounding, the refusal list and a raw ctypes call.

T = 64 is the kernels' K / V tile (FA_T of kernels/flash_attention.hip); a workgroup owns 64 queries, a wave 16."""
import functools

import numpy as np
import torch

T = 64
# (batch, seq_q, seq_kv, heads, head_dim, layout, causal) -> kind.  "std1" / "std3": q, k standard normal times 1 / 3, v standard normal,
# scale head_dim^-0.5.  "large" / "rising" / "falling": INTEGER-valued q and k with scale 0.5 (every score exact in fp32, bf16 and fp16):
#   large    q, k integers in [-4, 4]: row maxima near 100, exp overflows fp32 unless the maximum is subtracted
#   rising   q, k integers in [-2, 2], q[..., 0] = 4, k[j, 0] = j // 4: the row maximum rises in every K / V tile, so the O and l rescale
#            runs every tile and the weight ends in the last tile
#   falling  k[j, 0] = -(j // 4): the first tile holds all the weight, later tiles add (almost) nothing
CASES = [
    ((3, 1, 1, 2, 32, "bhsd", 0), "std1"),              # seq 1
    ((2, 16, 16, 2, 32, "bshd", 0), "std1"),            # one query tile of a wave exactly
    ((2, 17, 17, 3, 64, "bshd", 0), "std1"),            # ragged just above it
    ((2, T - 1, T - 1, 2, 32, "bhsd", 0), "std1"),      # ragged around the K / V tile
    ((1, T, T, 2, 128, "bshd", 0), "std1"),
    ((2, T + 1, T + 1, 2, 64, "bhsd", 0), "std1"),
    ((2, 300, 300, 3, 32, "bshd", 0), "std1"),          # several K / V tiles, ragged last one, both layouts
    ((2, 300, 300, 3, 32, "bhsd", 0), "std3"),
    ((2, 300, 300, 3, 64, "bshd", 0), "std3"),
    ((2, 300, 300, 3, 64, "bhsd", 0), "std1"),
    ((2, 300, 300, 3, 128, "bshd", 0), "std1"),
    ((2, 300, 300, 3, 128, "bhsd", 0), "std3"),
    ((2, 5, 300, 2, 64, "bshd", 0), "std1"),            # cross shapes
    ((2, 300, 7, 2, 64, "bhsd", 0), "std1"),
    ((3, 1, 1, 2, 32, "bshd", 1), "std1"),              # causal
    ((2, 17, 17, 3, 64, "bhsd", 1), "std1"),
    ((2, 300, 300, 2, 64, "bshd", 1), "std1"),
    ((1, 257, 257, 2, 128, "bhsd", 1), "std1"),
    ((2, 300, 300, 2, 64, "bhsd", 0), "large"),
    ((2, 40, 300, 2, 64, "bshd", 0), "rising"),
    ((2, 40, 300, 2, 64, "bhsd", 0), "falling"),
    ((1, 512, 512, 32, 128, "bshd", 0), "std1"),        # the smallest shape of the reference bench (bench_flash_attn.rs:77)
    ((2, 1024, 1024, 8, 64, "bhsd", 0), "std1"),        # 16 x 64 query tiles of a wave = 256 workgroups (many residency rounds: the 2^31 test of test_flash_attention_gpu.py)
]
SHAPES = [c for c, _ in CASES]
KIND = dict(CASES)
LARGEST = [(1, 512, 512, 32, 128, "bshd", 0), (2, 1024, 1024, 8, 64, "bhsd", 0)]
S16_ULP = {"bf16": 2.0 ** -8, "f16": 2.0 ** -11}


def case_id(shape):
    b, sq, skv, h, d, layout, causal = shape
    return f"{b}x{sq}x{skv}x{h}x{d}-{layout}{'-causal' if causal else ''}-{KIND[shape]}"


def case_scale(shape):
    """the scale argument of the call: 0 = head_dim^-0.5"""
    return 0.0 if KIND[shape].startswith("std") else 0.5


def to_bhsd(a, layout):
    return a.transpose(0, 2, 1, 3) if layout == "bshd" else a


@functools.lru_cache(maxsize=None)
def make_inputs(shape):
    """q, k, v of a case in the case's layout (fp32, contiguous).  The arrays are shared between tests: read-only."""
    batch, seq_q, seq_kv, heads, hd, layout, causal = shape
    kind = KIND[shape]
    rng = np.random.default_rng(2000 + SHAPES.index(shape))
    v = rng.standard_normal((batch, heads, seq_kv, hd))
    if kind.startswith("std"):
        std = float(kind[3:])
        q = rng.standard_normal((batch, heads, seq_q, hd)) * std
        k = rng.standard_normal((batch, heads, seq_kv, hd)) * std
    else:
        r = 4 if kind == "large" else 2
        q = rng.integers(-r, r + 1, (batch, heads, seq_q, hd)).astype(np.float64)
        k = rng.integers(-r, r + 1, (batch, heads, seq_kv, hd)).astype(np.float64)
        if kind != "large":
            q[..., 0] = 4.0
            k[..., 0] = (np.arange(seq_kv) // 4) * (1.0 if kind == "rising" else -1.0)
    out = []
    for a in (q, k, v):
        a = np.ascontiguousarray(to_bhsd(a, layout), dtype=np.float32)     # bhsd -> bshd is the same transpose
        a.setflags(write=False)
        out.append(a)
    return tuple(out)


def round_s16(a, s16="bf16"):
    """round-to-nearest-even fp32 -> bf16 or fp16 -> float64 (_bf16_round of tests/test_ops_gpu.py)"""
    return torch.from_numpy(np.array(a, np.float32)).to(torch.float16 if s16 == "f16" else torch.bfloat16).to(torch.float64).numpy()


def reference(q, k, v, layout="bhsd", causal=False, scale=None):
    """softmax(scale q k^T) v in float64 (bench_flash_attn.rs:89-95); causal: key j takes part in query i's row exactly when j <= i.
    q, k, v and the result are in `layout`."""
    q, k, v = (to_bhsd(np.asarray(a, np.float64), layout) for a in (q, k, v))
    scale = q.shape[-1] ** -0.5 if not scale else scale
    s = (q @ k.transpose(0, 1, 3, 2)) * scale
    if causal:
        s = np.where(np.arange(s.shape[-1])[None, :] <= np.arange(s.shape[-2])[:, None], s, -np.inf)
    p = np.exp(s - s.max(-1, keepdims=True))
    y = (p / p.sum(-1, keepdims=True)) @ v
    return np.ascontiguousarray(to_bhsd(y, layout))


@functools.lru_cache(maxsize=None)
def case_reference(shape, s16=None, causal=None):
    """the reference of a case, on q, k, v rounded to the 16-bit type when s16 is given (causal: override the case's flag); computed once,
    read-only"""
    q, k, v = make_inputs(shape)
    if s16:
        q, k, v = (round_s16(a, s16) for a in (q, k, v))
    r = reference(q, k, v, shape[5], shape[6] if causal is None else causal, case_scale(shape))
    r.setflags(write=False)
    return r


def raw_call(lib, q, k, v, batch, seq_q, seq_kv, heads, head_dim, layout, causal, scale, y, loc=0):
    """brn_flash_attention_forward with the integers exactly as given (the refusals need arguments the wrapper cannot express); q, k, v, y:
    numpy arrays, integers taken as addresses, or None"""
    ptr = lambda a: a if a is None or isinstance(a, int) else a.ctypes.data
    st = lib.brn_flash_attention_forward(ptr(q), ptr(k), ptr(v), batch, seq_q, seq_kv, heads, head_dim, layout, causal, scale, ptr(y), loc, 0, None)
    return st, (lib.brn_last_error() or b"").decode()


@functools.lru_cache(maxsize=None)
def _refusal_buffers():
    return tuple(np.zeros(2 * 2 * 32 * 256, np.float32) for _ in range(4))


def refusals():
    """(name, arguments of raw_call after lib, words the message must contain): every limit of the header.  The buffers hold what the
    well-formed neighbours of each call would read; the refused calls read nothing."""
    q, k, v, y = _refusal_buffers()
    a = q.ctypes.data
    assert a % 16 == 0
    return [
        ("head_dim 48", (q, k, v, 2, 16, 16, 2, 48, 0, 0, 0.0, y), "head_dim must be 32, 64 or 128"),
        ("head_dim 256", (q, k, v, 2, 16, 16, 2, 256, 0, 0, 0.0, y), "head_dim must be 32, 64 or 128"),
        ("seq_q 0", (q, k, v, 2, 0, 16, 2, 32, 0, 0, 0.0, y), "1 <= seq_q, seq_kv <= 65536"),
        ("seq_kv 0", (q, k, v, 2, 16, 0, 2, 32, 0, 0, 0.0, y), "1 <= seq_q, seq_kv <= 65536"),
        ("seq_q 65537", (q, k, v, 1, 65537, 16, 1, 32, 0, 0, 0.0, y), "1 <= seq_q, seq_kv <= 65536"),
        ("seq_kv 65537", (q, k, v, 1, 16, 65537, 1, 32, 0, 0, 0.0, y), "1 <= seq_q, seq_kv <= 65536"),
        ("batch 0", (q, k, v, 0, 16, 16, 2, 32, 0, 0, 0.0, y), "batch >= 1, heads >= 1"),
        ("heads 0", (q, k, v, 2, 16, 16, 0, 32, 0, 0, 0.0, y), "batch >= 1, heads >= 1"),
        ("2^31 query tiles", (q, k, v, 32768, 65536, 16, 16, 32, 0, 0, 0.0, y), "batch * heads * ceil(seq_q / 16) < 2^31"),
        ("layout 2", (q, k, v, 2, 16, 16, 2, 32, 2, 0, 0.0, y), "layout must be 0"),
        ("causal 2", (q, k, v, 2, 16, 16, 2, 32, 0, 2, 0.0, y), "causal must be 0 or 1"),
        ("causal, seq_q != seq_kv", (q, k, v, 2, 16, 17, 2, 32, 0, 1, 0.0, y), "causal requires seq_q == seq_kv"),
        ("negative scale", (q, k, v, 2, 16, 16, 2, 32, 0, 0, -0.5, y), "scale must be finite and >= 0"),
        ("infinite scale", (q, k, v, 2, 16, 16, 2, 32, 0, 0, float("inf"), y), "scale must be finite and >= 0"),
        ("NaN scale", (q, k, v, 2, 16, 16, 2, 32, 0, 0, float("nan"), y), "scale must be finite and >= 0"),
        ("null q", (None, k, v, 2, 16, 16, 2, 32, 0, 0, 0.0, y), "null q, k, v or y"),
        ("null y", (q, k, v, 2, 16, 16, 2, 32, 0, 0, 0.0, None), "null q, k, v or y"),
        ("y is q", (q, k, v, 2, 16, 16, 2, 32, 0, 0, 0.0, q), "overlap"),
        ("y overlaps the end of v", (q, k, v, 2, 16, 16, 2, 32, 0, 0, 0.0, v.ctypes.data + 4 * (2 * 16 * 2 * 32 - 4)), "overlap"),
        ("misaligned device k", (q, a + 4096 + 4, v, 2, 16, 16, 2, 32, 0, 0, 0.0, y, 1), "16-byte aligned"),
    ]
