"""What tests/test_flash_attention_splitkv_gpu.py and tests/test_flash_attention_splitkv_cpu.py share: the cases of
brn_flash_attention_splitkv_forward, the float64 reference of y and of
    lse[b,h,i] = ln sum_j exp(scale * q[b,h,i] . k[b, h // G, j])   over the row's visible keys,
the numpy emulation of the kernels' split walk and of the combine, the float64 combination of a call's own partials, the refusal list
and a raw ctypes call.

Inputs, rounding, the row map and the bounds of y are those of flash_attention_gqa_cases; the bound of lse has the form of f32_bound."""
import ctypes
import functools

import numpy as np

import flash_attention_gqa_cases as GQ
from flash_attention_gqa_cases import BQ, T, f32_bound, in_layout, kind_scale, make_inputs, round_s16, s16_bound, shape_id  # noqa: F401

LN2 = 0.6931471805599453
MODES = ("f32", "bf16", "f16")

# ((batch, seq_q, seq_kv, heads, kv_heads, head_dim), kind, causal, kv_splits): the smallest shapes at which each mechanism can go wrong
_TABLE = [
    ((2, 1, 300, 8, 2, 64), "std1", (0, 1), (2, 3, 5)),        # decode, ragged last tile, tps 3 / 2 / 1
    ((3, 1, 1000, 5, 1, 128), "std1", (1,), (4, 16)),          # multi-query, D 128
    ((1, 100, 110, 4, 1, 64), "std1", (1,), (2,)),             # rows of a walked tile with no key in split 1
    ((1, 130, 700, 4, 2, 32), "std1", (1,), (3, 11)),          # query tiles with different nkt; workgroups with nothing to walk
    ((1, 2, 65, 2, 1, 128), "std1", (1,), (2,)),               # one key in the last split, one row sees it
    ((2, 7, 200, 16, 2, 64), "std1", (1,), (4,)),              # G 8, ragged
    ((2, 7, 200, 16, 2, 64), "large", (0,), (2,)),
    ((1, 3, 70, 80, 1, 32), "std1", (0,), (2,)),               # G 80 > 64
    ((2, 17, 300, 6, 2, 32), "rising", (1,), (3, 5)),          # early splits whose weights underflow to exactly 0
    ((2, 17, 300, 6, 2, 32), "falling", (1,), (3, 5)),         # late splits whose weights underflow to exactly 0
    ((1, 1, 64, 4, 4, 32), "std1", (0,), (4,)),                # S collapses to 1
]
CASES = [(shape, kind, causal, ks) for shape, kind, causals, splits in _TABLE for causal in causals for ks in splits]
# the causal cases whose partials hold empty rows (a row with no visible key in a split), and how many real rows those are
EMPTY_CASES = [((1, 100, 110, 4, 1, 64), "std1", 1, 2), ((1, 130, 700, 4, 2, 32), "std1", 1, 11), ((1, 2, 65, 2, 1, 128), "std1", 1, 2)]
COLLAPSED = ((1, 1, 64, 4, 4, 32), "std1", 0, 4)


def case_id(case):
    shape, kind, causal, ks = case
    return f"{shape_id(shape)}-{kind}{'-causal' if causal else ''}-s{ks}"


def plan(seq_kv, kv_splits):
    """(S, tps) of an explicit kv_splits >= 1, as include/birefnet_hip.h states them"""
    nkt = (seq_kv + T - 1) // T
    tps = (nkt + kv_splits - 1) // kv_splits
    return (nkt + tps - 1) // tps, tps


def empty_rows(case):
    """how many (split, batch entry, head, query) partial rows of the case see no key: limit <= the split's first key"""
    shape, _, causal, ks = case
    batch, seq_q, seq_kv, heads, _, _ = shape
    S, tps = plan(seq_kv, ks)
    limit = np.arange(seq_q) + (seq_kv - seq_q) + 1 if causal else np.full(seq_q, seq_kv)
    return int(sum((limit <= s * tps * T).sum() for s in range(S))) * batch * heads


for _c in EMPTY_CASES:
    assert _c in CASES and empty_rows(_c) > 0, _c        # the coverage of the empty marker cannot vanish silently


# ---- float64 references ----
def reference_lse(q, k, causal=False, scale=None):
    """ln sum_j exp(scale q . k_j) over the visible keys, float64, BHSD arrays -> [batch, heads, seq_q]"""
    q, k = np.asarray(q, np.float64), np.asarray(k, np.float64)
    G = q.shape[1] // k.shape[1]
    scale = q.shape[-1] ** -0.5 if not scale else scale
    s = (q @ k[:, np.arange(q.shape[1]) // G].transpose(0, 1, 3, 2)) * scale
    if causal:
        s = np.where(GQ.visible(q.shape[2], k.shape[2]), s, -np.inf)
    mx = s.max(-1)
    return mx + np.log(np.exp(s - mx[..., None]).sum(-1))


@functools.lru_cache(maxsize=None)
def case_reference(shape, kind, causal, s16=None):
    """(y, lse) in float64 (BHSD / [batch, heads, seq_q]), on q, k, v rounded to the 16-bit type when s16 is given; computed once"""
    q, k, v, _ = make_inputs(shape, kind)
    if s16:
        q, k, v = (round_s16(a, s16) for a in (q, k, v))
    y = GQ.reference(q, k, v, None, causal, kind_scale(kind))
    lse = reference_lse(q, k, causal, kind_scale(kind))
    y.setflags(write=False)
    lse.setflags(write=False)
    return y, lse


def lse_bound(ref_lse, tol=3e-5):
    """the form of f32_bound: lse is an fp32 sum of exp2 / log2 results of the hardware in every mode"""
    return tol * max(1.0, float(np.abs(ref_lse).max()))


def y_bound(ref, v, mode):
    return f32_bound(ref) if mode == "f32" else s16_bound(ref, v, mode)


def combine64(o_part, lse2_part):
    """the float64 combination of partials [S, R, D], [S, R] -> (y [R, D], lse [R]): what a caller who merges them exactly would get"""
    o, l2 = np.asarray(o_part, np.float64), np.asarray(lse2_part, np.float64)
    M = l2.max(0)
    w = np.exp2(l2 - M)
    return (w[..., None] * o).sum(0) / w.sum(0)[:, None], (M + np.log2(w.sum(0))) * np.log(2.0)


# ---- the split walk and the combine of kernels/flash_attention.hip (FA_SPLIT, flash_split_combine_kernel), restated in numpy ----
def emulate(q, k, v, causal, scale, kv_splits, s16=None):
    """fp32 throughout, BHSD arrays (already rounded when s16 is given).  Per (batch entry, K / V head, tile of row_map, split s): K / V
    tiles s * tps .. min((s + 1) * tps, the tile's nkt) - 1, excluded keys -inf, numerators rounded to the 16-bit type for P v; the
    partial is o / l and m + log2(l), or 0 and -inf where l == 0 (also for a workgroup with nothing to walk).  Then the combine in the
    order s = 0 .. S - 1; S == 1 is the single partial itself.  Returns y [batch, heads, seq_q, hd], lse [batch, heads, seq_q],
    O_part [S, R, hd], lse2_part [S, R] (R rows heads-major)."""
    f = np.float32
    q, k, v = (np.asarray(a, f) for a in (q, k, v))
    batch, heads, seq_q, hd = q.shape
    kv_heads, seq_kv = k.shape[1], k.shape[2]
    G = heads // kv_heads
    S, tps = plan(seq_kv, kv_splits)
    sc2 = f(f(scale if scale else f(1.0) / np.sqrt(f(hd))) * f(1.4426950408889634))
    o_part = np.full((S, batch, heads, seq_q, hd), np.nan, f)
    l2_part = np.full((S, batch, heads, seq_q), np.nan, f)
    tiles = GQ.row_map(G, seq_q, seq_kv, causal)
    with np.errstate(divide="ignore", invalid="ignore"):
        for b in range(batch):
            for kvh in range(kv_heads):
                for t in tiles:
                    h, i = kvh * G + t["head"], t["query"]
                    qt = q[b, h, i]
                    real = ~t["pad"]
                    for s in range(S):
                        m = np.full((BQ, 1), -3.0e38, f)
                        l = np.zeros((BQ, 1), f)
                        o = np.zeros((BQ, hd), f)
                        for kt in range(s * tps, min((s + 1) * tps, t["nkt"])):
                            keys = np.arange(kt * T, min((kt + 1) * T, seq_kv))
                            sc = (qt @ k[b, kvh, keys].T).astype(f) * sc2
                            sc = np.where(keys[None, :] < t["limit"][:, None], sc, f(-np.inf))
                            mn = np.maximum(m, sc.max(-1, keepdims=True))
                            alpha = np.exp2(m - mn)
                            p = np.exp2(sc - mn)
                            l = l * alpha + p.sum(-1, keepdims=True, dtype=f)
                            pr = round_s16(p, s16).astype(f) if s16 else p
                            o = o * alpha + (pr @ v[b, kvh, keys]).astype(f)
                            m = mn
                        empty = l[:, 0] == 0
                        op = np.where(empty[:, None], f(0), o / l).astype(f)
                        l2 = np.where(empty, f(-np.inf), (m + np.log2(l))[:, 0]).astype(f)
                        o_part[s, b, h[real], i[real]] = op[real]
                        l2_part[s, b, h[real], i[real]] = l2[real]
        if S == 1:
            y, lse = o_part[0], (l2_part[0] * f(LN2)).astype(f)
        else:
            M = l2_part.max(0)
            acc = np.zeros(o_part.shape[1:], f)
            wsum = np.zeros(M.shape, f)
            for s in range(S):
                w = np.exp2(l2_part[s] - M).astype(f)
                acc = (acc + w[..., None] * o_part[s]).astype(f)
                wsum = (wsum + w).astype(f)
            y = (acc / wsum[..., None]).astype(f)
            lse = ((M + np.log2(wsum).astype(f)) * f(LN2)).astype(f)
    R = batch * heads * seq_q
    return y, lse, o_part.reshape(S, R, hd), l2_part.reshape(S, R)


@functools.lru_cache(maxsize=None)
def case_emulation(case, mode):
    shape, kind, causal, ks = case
    q, k, v, _ = make_inputs(shape, kind)
    s16 = None if mode == "f32" else mode
    if s16:
        q, k, v = (round_s16(a, s16) for a in (q, k, v))
    out = emulate(q, k, v, causal, kind_scale(kind), ks, s16)
    for a in out:
        a.setflags(write=False)
    return out


# ---- raw calls and refusals ----
def raw_plan(lib, batch, seq_q, seq_kv, heads, kv_heads, head_dim, kv_splits):
    """brn_flash_attention_splitkv_plan -> (status, message, S, tps, workspace_floats)"""
    S, tps, n = ctypes.c_int(-1), ctypes.c_int(-1), ctypes.c_size_t(0)
    st = lib.brn_flash_attention_splitkv_plan(batch, seq_q, seq_kv, heads, kv_heads, head_dim, kv_splits, ctypes.byref(S), ctypes.byref(tps), ctypes.byref(n))
    return st, (lib.brn_last_error() or b"").decode(), S.value, tps.value, n.value


def raw_call(lib, q, k, v, batch, seq_q, seq_kv, heads, kv_heads, head_dim, layout, causal, scale, kv_splits, y, lse, ws, ws_floats, loc=0):
    """brn_flash_attention_splitkv_forward with the integers exactly as given; q, k, v, y, lse, ws: numpy arrays, integers taken as
    addresses, or None"""
    ptr = lambda a: a if a is None or isinstance(a, int) else a.ctypes.data
    st = lib.brn_flash_attention_splitkv_forward(ptr(q), ptr(k), ptr(v), batch, seq_q, seq_kv, heads, kv_heads, head_dim, layout, causal, scale, kv_splits,
                                                 ptr(y), ptr(lse), ptr(ws), ws_floats, loc, 0, None)
    return st, (lib.brn_last_error() or b"").decode()


@functools.lru_cache(maxsize=None)
def _refusal_buffers():
    return tuple(np.zeros(2 * 2 * 32 * 256, np.float32) for _ in range(6))


def refusals():
    """(name, arguments of raw_call after lib, words the message must contain).  The well-formed neighbour of every call is
    (q, k, v, 2, 16, 200, 2, 1, 32, 0, 0, 0.0, 2, y, lse, ws, 4224): nkt 4, S 2, R 64, 2 * 64 * 33 = 4224 workspace floats.  The refused
    calls read nothing."""
    q, k, v, y, lse, ws = _refusal_buffers()
    a = q.ctypes.data
    assert a % 16 == 0
    tail = (y, lse, ws, 4224)
    return [
        ("kv_splits -1", (q, k, v, 2, 16, 200, 2, 1, 32, 0, 0, 0.0, -1) + tail, "0 <= kv_splits <= 1024"),
        ("kv_splits 1025", (q, k, v, 2, 16, 200, 2, 1, 32, 0, 0, 0.0, 1025) + tail, "0 <= kv_splits <= 1024"),
        ("workspace NULL, S 2", (q, k, v, 2, 16, 200, 2, 1, 32, 0, 0, 0.0, 2, y, lse, None, 0), "4224 floats"),
        ("workspace too small", (q, k, v, 2, 16, 200, 2, 1, 32, 0, 0, 0.0, 2, y, lse, ws, 4223), "4224 floats"),
        ("2^31 workgroups with the splits", (q, k, v, 32768, 1024, 65536, 64, 64, 32, 0, 0, 0.0, 1024) + tail, "S < 2^31"),
        ("lse is y", (q, k, v, 2, 16, 200, 2, 1, 32, 0, 0, 0.0, 2, y, y, ws, 4224), "overlap"),
        ("lse is k", (q, k, v, 2, 16, 200, 2, 1, 32, 0, 0, 0.0, 2, y, k, ws, 4224), "overlap"),
        ("workspace overlaps the end of y", (q, k, v, 2, 16, 200, 2, 1, 32, 0, 0, 0.0, 2, y, lse, y.ctypes.data + 4 * (2 * 16 * 2 * 32 - 4), 4224), "overlap"),
        ("workspace is v", (q, k, v, 2, 16, 200, 2, 1, 32, 0, 0, 0.0, 2, y, lse, v, 4224), "overlap"),
        ("workspace overlaps lse", (q, k, v, 2, 16, 200, 2, 1, 32, 0, 0, 0.0, 2, y, lse, lse.ctypes.data + 4 * 60, 4224), "overlap"),
        ("misaligned device lse", (q, k, v, 2, 16, 200, 2, 1, 32, 0, 0, 0.0, 2, y, lse.ctypes.data + 4096 + 4, ws, 4224, 1), "16-byte aligned"),
        ("misaligned device workspace", (q, k, v, 2, 16, 200, 2, 1, 32, 0, 0, 0.0, 2, y, lse, ws.ctypes.data + 4096 + 8, 4224, 1), "16-byte aligned"),
        # every bias-free limit of the gqa entry, under this entry's prefix
        ("kv_heads 0", (q, k, v, 2, 16, 200, 2, 0, 32, 0, 0, 0.0, 2) + tail, "1 <= kv_heads <= heads"),
        ("heads % kv_heads != 0", (q, k, v, 2, 16, 200, 6, 4, 32, 0, 0, 0.0, 2) + tail, "heads % kv_heads == 0"),
        ("causal, seq_kv < seq_q", (q, k, v, 2, 17, 16, 2, 1, 32, 0, 1, 0.0, 1) + tail, "causal requires seq_kv >= seq_q"),
        ("2^31 tiles", (q, k, v, 32768, 65536, 16, 64, 64, 32, 0, 0, 0.0, 1) + tail, "batch * kv_heads * ceil(G * seq_q / 64) < 2^31"),
        ("2^31 packed rows", (q, k, v, 1, 65536, 16, 32768, 1, 32, 0, 0, 0.0, 1) + tail, "G * seq_q < 2^31"),
        ("head_dim 48", (q, k, v, 2, 16, 200, 2, 1, 48, 0, 0, 0.0, 2) + tail, "head_dim must be 32, 64 or 128"),
        ("seq_q 0", (q, k, v, 2, 0, 200, 2, 1, 32, 0, 0, 0.0, 2) + tail, "1 <= seq_q, seq_kv <= 65536"),
        ("seq_kv 65537", (q, k, v, 1, 16, 65537, 2, 1, 32, 0, 0, 0.0, 2) + tail, "1 <= seq_q, seq_kv <= 65536"),
        ("batch 0", (q, k, v, 0, 16, 200, 2, 1, 32, 0, 0, 0.0, 2) + tail, "batch >= 1, heads >= 1"),
        ("layout 2", (q, k, v, 2, 16, 200, 2, 1, 32, 2, 0, 0.0, 2) + tail, "layout must be 0"),
        ("causal 2", (q, k, v, 2, 16, 200, 2, 1, 32, 0, 2, 0.0, 2) + tail, "causal must be 0 or 1"),
        ("NaN scale", (q, k, v, 2, 16, 200, 2, 1, 32, 0, 0, float("nan"), 2) + tail, "scale must be finite and >= 0"),
        ("null k", (q, None, v, 2, 16, 200, 2, 1, 32, 0, 0, 0.0, 2) + tail, "null q, k, v or y"),
        ("y is q", (q, k, v, 2, 16, 200, 2, 1, 32, 0, 0, 0.0, 2, q, lse, ws, 4224), "overlap"),
        ("misaligned device v", (q, k, a + 4096 + 4, 2, 16, 200, 2, 1, 32, 0, 0, 0.0, 2) + tail + (1,), "16-byte aligned"),
    ]
