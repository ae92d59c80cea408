"""What tests/test_flash_attention_gqa_gpu.py and tests/test_flash_attention_gqa_cpu.py share: the case lists of
brn_flash_attention_gqa_forward, its seeded inputs, the repeat of K / V along heads that the older entries need, the causal mask over a
cache as a -inf bias, the float64 reference
    softmax(scale * (q[b,h] k[b, h // G]^T + bias[b % n_bias, h]) [key j <= query i + seq_kv - seq_q]) v[b, h // G],
the numpy emulation of the kernels' packed-row map and tile walk, the refusal list and a raw ctypes call.

Rounding, the bounds and the input kinds are those of flash_attention_cases / flash_attention_bias_cases."""
import functools

import numpy as np

from flash_attention_bias_cases import f32_bound, s16_bound  # noqa: F401  (re-exported to the two test files)
from flash_attention_cases import S16_ULP, T, round_s16, to_bhsd  # noqa: F401

BQ = 64          # packed rows per workgroup (FA_BQ of kernels/flash_attention.hip); T = 64 keys per K / V tile

# (batch, seq_q, seq_kv, heads, kv_heads, head_dim)
GROUP_SHAPES = [
    (2, 300, 300, 8, 2, 64),       # G 4, several tiles
    (2, 37, 37, 6, 2, 32),         # G 3: waves straddle heads and queries
    (3, 1, 300, 5, 1, 128),        # multi-query, one query
    (2, 7, 200, 16, 2, 64),        # G 8, ragged
    (1, 3, 70, 80, 1, 32),         # G 80 > 64: one tile lies inside one query
    (2, 64, 64, 4, 4, 32),         # G 1
]
CACHE_SHAPES = [
    (2, 1, 130, 4, 2, 64),         # single-token decode
    (2, 17, 300, 6, 2, 32),
    (1, 100, 164, 4, 1, 128),      # an offset of one K / V tile exactly
    (2, 65, 66, 4, 2, 64),
]
# parity against float64: (shape, kind, causal); kinds as in flash_attention_cases ("large" / "rising": integer q, k with scale 0.5)
PARITY = ([(s, "std1", 0) for s in GROUP_SHAPES] + [(s, "std1", 1) for s in GROUP_SHAPES if s[1] == s[2]] + [(s, "std1", 1) for s in CACHE_SHAPES]
          + [((2, 7, 200, 16, 2, 64), "large", 0), ((2, 17, 300, 6, 2, 32), "rising", 1)])


def shape_id(shape):
    return "x".join(str(v) for v in shape)


def parity_id(case):
    shape, kind, causal = case
    return f"{shape_id(shape)}-{kind}{'-causal' if causal else ''}"


def kind_scale(kind):
    """the scale argument of the call: None = head_dim^-0.5"""
    return None if kind.startswith("std") else 0.5


def n_bias_of(shape):
    return 2 if shape[0] % 2 == 0 else 1


@functools.lru_cache(maxsize=None)
def make_inputs(shape, kind="std1"):
    """q [batch, heads, seq_q, hd], k, v [batch, kv_heads, seq_kv, hd] and a bias [n_bias, heads, seq_q, seq_kv] (standard normal x
    sqrt(head_dim), the scale of q . k itself; even integers in the integer kinds, where every score stays exact), fp32, BHSD; in_layout()
    gives the other layout.  Shared between tests: read-only."""
    batch, seq_q, seq_kv, heads, kv_heads, hd = shape
    rng = np.random.default_rng(4100 + sum(v * 31 ** i for i, v in enumerate(shape)) % 100003 + len(kind))
    v = rng.standard_normal((batch, kv_heads, seq_kv, hd))
    nb = n_bias_of(shape)
    if kind.startswith("std"):
        std = float(kind[3:])
        q = rng.standard_normal((batch, heads, seq_q, hd)) * std
        k = rng.standard_normal((batch, kv_heads, seq_kv, hd)) * std
        bias = rng.standard_normal((nb, heads, seq_q, seq_kv)) * np.sqrt(hd)
    else:
        r = 4 if kind == "large" else 2
        q = rng.integers(-r, r + 1, (batch, heads, seq_q, hd)).astype(np.float64)
        k = rng.integers(-r, r + 1, (batch, kv_heads, seq_kv, hd)).astype(np.float64)
        if kind != "large":
            q[..., 0] = 4.0
            k[..., 0] = (np.arange(seq_kv) // 4) * (1.0 if kind == "rising" else -1.0)
        bias = 2.0 * rng.integers(-3, 4, (nb, heads, seq_q, seq_kv))
    out = []
    for a in (q, k, v, bias):
        a = np.ascontiguousarray(a, dtype=np.float32)
        a.setflags(write=False)
        out.append(a)
    return tuple(out)


def in_layout(a, layout):
    """a BHSD array in `layout`, contiguous (bhsd <-> bshd is the same transpose)"""
    return np.ascontiguousarray(to_bhsd(a, layout))


def repeat_kv(a, G):
    """k or v [batch, kv_heads, seq_kv, hd] (BHSD) materialised for the older entries: query head h reads K / V head h // G"""
    return np.ascontiguousarray(np.repeat(a, G, axis=1))


def visible(seq_q, seq_kv):
    """[seq_q, seq_kv] bool: key j takes part in query i's row under the causal mask that ends at the last key"""
    return np.arange(seq_kv)[None, :] <= np.arange(seq_q)[:, None] + (seq_kv - seq_q)


def mask_bias(shape, bias=None):
    """the causal mask as a bias of the older bias entry: 0 (or the caller's bias) where visible, -inf elsewhere; [n_bias, heads, seq_q, seq_kv]"""
    _, seq_q, seq_kv, heads, _, _ = shape
    base = np.zeros((1, heads, seq_q, seq_kv), np.float32) if bias is None else bias
    return np.ascontiguousarray(np.where(visible(seq_q, seq_kv), base, -np.inf).astype(np.float32))


def reference(q, k, v, bias=None, causal=False, scale=None):
    """the float64 result on BHSD arrays: grouped (k[:, h // G]) and bottom-right causal"""
    q, k, v = (np.asarray(a, np.float64) for a in (q, k, v))
    G = q.shape[1] // k.shape[1]
    group = np.arange(q.shape[1]) // G
    scale = q.shape[-1] ** -0.5 if not scale else scale
    s = q @ k[:, group].transpose(0, 1, 3, 2)
    if bias is not None:
        s = s + np.asarray(bias, np.float64)[np.arange(q.shape[0]) % bias.shape[0]]
    s = s * scale
    if causal:
        s = np.where(visible(q.shape[2], k.shape[2]), s, -np.inf)
    p = np.exp(s - s.max(-1, keepdims=True))
    return (p / p.sum(-1, keepdims=True)) @ v[:, group]


@functools.lru_cache(maxsize=None)
def case_reference(shape, kind, causal, s16=None, with_bias=False):
    """the reference of a case (BHSD), on q, k, v rounded to the 16-bit type when s16 is given (the bias is never rounded); computed once"""
    q, k, v, bias = make_inputs(shape, kind)
    if s16:
        q, k, v = (round_s16(a, s16) for a in (q, k, v))
    r = reference(q, k, v, bias if with_bias else None, causal, kind_scale(kind))
    r.setflags(write=False)
    return r


# ---- the packed-row map of kernels/flash_attention.hip (fa_block_gqa, fa_lane), restated in numpy ----
def row_map(G, seq_q, seq_kv, causal):
    """one dict per workgroup tile of a K / V head's G * seq_q packed rows: per lane row (64): query, head (within the group), limit (first
    excluded key), pad; per tile: nkt (K / V tiles walked); per wave (4): wave_lim, the limit fa_tile_masks derives from the wave's first row"""
    rows = G * seq_q
    off = seq_kv - seq_q if causal else 0
    tiles = []
    for q0 in range(0, rows, BQ):
        rem = rows - 1 - q0
        lr = np.arange(BQ)
        row = q0 + np.minimum(lr, rem)
        query, head = row // G, row % G
        limit = np.minimum(seq_kv, query + off + 1) if causal else np.full(BQ, seq_kv)
        nkt = (seq_kv + T - 1) // T
        if causal:
            nkt = min(nkt, ((q0 + min(BQ - 1, rem)) // G + off) // T + 1)
        wave_row0 = np.array([(q0 + min(16 * w, rem)) // G + off for w in range(4)])
        wave_lim = np.minimum(seq_kv, wave_row0 + 1) if causal else np.full(4, seq_kv)
        tiles.append({"query": query, "head": head, "limit": limit, "pad": lr > rem, "nkt": nkt, "wave_lim": wave_lim})
    return tiles


def emulate(q, k, v, bias, causal, scale, s16=None):
    """The kernels' walk in numpy, fp32 arithmetic throughout, on BHSD arrays (q, k, v already rounded when s16 is given): per (batch
    entry, K / V head) the packed rows of row_map in tiles of 64; K / V tiles 0 .. nkt - 1; scores (+ bias) times scale * log2(e); keys
    from the row's limit on (and past seq_kv) excluded with -3e38; running maximum m and sum l, O and l rescaled by exp2(m_old - m_new);
    numerators rounded to the 16-bit type for P v when s16 is given, l taken from the unrounded ones."""
    f = np.float32
    q, k, v = (np.asarray(a, f) for a in (q, k, v))
    batch, heads, seq_q, hd = q.shape
    kv_heads, seq_kv = k.shape[1], k.shape[2]
    G = heads // kv_heads
    sc2 = f(f(scale if scale else f(1.0) / np.sqrt(f(hd))) * f(1.4426950408889634))
    y = np.full(q.shape, np.nan, f)
    tiles = row_map(G, seq_q, seq_kv, causal)
    for b in range(batch):
        for kvh in range(kv_heads):
            for t in tiles:
                h, i = kvh * G + t["head"], t["query"]
                qt = q[b, h, i]                                     # [64, hd]
                m = np.full((BQ, 1), -3.0e38, f)
                l = np.zeros((BQ, 1), f)
                o = np.zeros((BQ, hd), f)
                for kt in range(t["nkt"]):
                    keys = np.arange(kt * T, min((kt + 1) * T, seq_kv))
                    s = (qt @ k[b, kvh, keys].T).astype(f)
                    if bias is not None:
                        s = s + bias[b % bias.shape[0]][h[:, None], i[:, None], keys[None, :]]
                    s = s * sc2
                    s = np.where(keys[None, :] < t["limit"][:, None], s, f(-3.0e38))
                    mn = np.maximum(m, s.max(-1, keepdims=True))
                    alpha = np.exp2(m - mn)
                    p = np.exp2(s - mn)
                    l = l * alpha + p.sum(-1, keepdims=True, dtype=f)
                    pr = round_s16(p, s16).astype(f) if s16 else p
                    o = o * alpha + (pr @ v[b, kvh, keys]).astype(f)
                    m = mn
                real = ~t["pad"]
                y[b, h[real], i[real]] = (o / l)[real]
    return y


# ---- refusals ----
def raw_call(lib, q, k, v, batch, seq_q, seq_kv, heads, kv_heads, head_dim, layout, causal, bias, n_bias, scale, y, loc=0):
    """brn_flash_attention_gqa_forward with the integers exactly as given; q, k, v, bias, y: numpy arrays, integers taken as addresses, or None"""
    ptr = lambda a: a if a is None or isinstance(a, int) else a.ctypes.data
    st = lib.brn_flash_attention_gqa_forward(ptr(q), ptr(k), ptr(v), batch, seq_q, seq_kv, heads, kv_heads, head_dim, layout, causal, ptr(bias), n_bias,
                                             scale, ptr(y), loc, 0, None)
    return st, (lib.brn_last_error() or b"").decode()


@functools.lru_cache(maxsize=None)
def _refusal_buffers():
    return tuple(np.zeros(2 * 2 * 32 * 256, np.float32) for _ in range(5))


def refusals():
    """(name, arguments of raw_call after lib, words the message must contain): the limits of the grouped entry, then those it inherits,
    under its own prefix.  The buffers hold what the well-formed neighbours of each call would read; the refused calls read nothing."""
    q, k, v, y, bias = _refusal_buffers()
    a, ab = q.ctypes.data, bias.ctypes.data
    assert a % 16 == 0 and ab % 16 == 0
    nb = (None, 0)
    b1 = (bias, 1)
    return [
        ("kv_heads 0", (q, k, v, 2, 16, 16, 2, 0, 32, 0, 0) + nb + (0.0, y), "1 <= kv_heads <= heads"),
        ("kv_heads -1", (q, k, v, 2, 16, 16, 2, -1, 32, 0, 0) + nb + (0.0, y), "1 <= kv_heads <= heads"),
        ("kv_heads > heads", (q, k, v, 2, 16, 16, 2, 4, 32, 0, 0) + nb + (0.0, y), "1 <= kv_heads <= heads"),
        ("heads % kv_heads != 0", (q, k, v, 2, 16, 16, 6, 4, 32, 0, 0) + nb + (0.0, y), "heads % kv_heads == 0"),
        ("causal, seq_kv < seq_q", (q, k, v, 2, 17, 16, 2, 1, 32, 0, 1) + nb + (0.0, y), "causal requires seq_kv >= seq_q"),
        ("2^31 tiles", (q, k, v, 32768, 65536, 16, 64, 64, 32, 0, 0) + nb + (0.0, y), "batch * kv_heads * ceil(G * seq_q / 64) < 2^31"),
        ("2^31 tiles, grouped", (q, k, v, 32768, 65536, 16, 128, 64, 32, 0, 0) + nb + (0.0, y), "batch * kv_heads * ceil(G * seq_q / 64) < 2^31"),
        ("2^31 packed rows", (q, k, v, 1, 65536, 16, 32768, 1, 32, 0, 0) + nb + (0.0, y), "G * seq_q < 2^31"),
        ("head_dim 48", (q, k, v, 2, 16, 16, 2, 1, 48, 0, 0) + nb + (0.0, y), "head_dim must be 32, 64 or 128"),
        ("seq_q 0", (q, k, v, 2, 0, 16, 2, 1, 32, 0, 0) + nb + (0.0, y), "1 <= seq_q, seq_kv <= 65536"),
        ("seq_kv 65537", (q, k, v, 1, 16, 65537, 2, 1, 32, 0, 0) + nb + (0.0, y), "1 <= seq_q, seq_kv <= 65536"),
        ("batch 0", (q, k, v, 0, 16, 16, 2, 1, 32, 0, 0) + nb + (0.0, y), "batch >= 1, heads >= 1"),
        ("heads 0", (q, k, v, 2, 16, 16, 0, 1, 32, 0, 0) + nb + (0.0, y), "batch >= 1, heads >= 1"),
        ("layout 2", (q, k, v, 2, 16, 16, 2, 1, 32, 2, 0) + nb + (0.0, y), "layout must be 0"),
        ("causal 2", (q, k, v, 2, 16, 16, 2, 1, 32, 0, 2) + nb + (0.0, y), "causal must be 0 or 1"),
        ("NaN scale", (q, k, v, 2, 16, 16, 2, 1, 32, 0, 0) + nb + (float("nan"), y), "scale must be finite and >= 0"),
        ("null k", (q, None, v, 2, 16, 16, 2, 1, 32, 0, 0) + nb + (0.0, y), "null q, k, v or y"),
        ("y is q", (q, k, v, 2, 16, 16, 2, 1, 32, 0, 0) + nb + (0.0, q), "overlap"),
        ("y overlaps the end of v (kv_heads 1)", (q, k, v, 2, 16, 16, 2, 1, 32, 0, 0) + nb + (0.0, v.ctypes.data + 4 * (2 * 16 * 1 * 32 - 4)), "overlap"),
        ("misaligned device v", (q, k, a + 4096 + 4, 2, 16, 16, 2, 1, 32, 0, 0) + nb + (0.0, y, 1), "16-byte aligned"),
        ("n_bias -1", (q, k, v, 2, 16, 16, 2, 1, 32, 0, 0, bias, -1, 0.0, y), "n_bias >= 0"),
        ("bias NULL, n_bias 1", (q, k, v, 2, 16, 16, 2, 1, 32, 0, 0, None, 1, 0.0, y), "bias must be NULL exactly when n_bias == 0"),
        ("bias given, n_bias 0", (q, k, v, 2, 16, 16, 2, 1, 32, 0, 0, bias, 0, 0.0, y), "bias must be NULL exactly when n_bias == 0"),
        ("batch 3, n_bias 2", (q, k, v, 3, 16, 16, 2, 1, 32, 0, 0, bias, 2, 0.0, y), "batch % n_bias == 0"),
        ("y is the bias", (q, k, v, 2, 16, 16, 2, 1, 32, 0, 0) + b1 + (0.0, bias), "overlap"),
        ("misaligned device bias", (q, k, v, 2, 16, 16, 2, 1, 32, 0, 0, ab + 4096 + 4, 1, 0.0, y, 1), "16-byte aligned"),
    ]
