"""What tests/test_flash_attention_varlen_gpu.py and tests/test_flash_attention_varlen_cpu.py share: the packs and windows of
brn_flash_attention_varlen_forward, the packed inputs (each sequence is a case of flash_attention_gqa_cases, seeded there), the window as a
visibility matrix and as a -inf bias, the float64 reference
    softmax over keys i + off - window_left <= j <= i + off + window_right of (scale * q[i,h] k[j, h // G]^T) v[j, h // G],  off = len_kv - len_q,
the numpy restatement of the record table (csrc/brn_flash_varlen_plan.h) and of the kernels' walk over it, the refusal list and a raw ctypes
call.

Inputs, rounding and the bounds are those of flash_attention_gqa_cases / flash_attention_bias_cases / flash_attention_cases."""
import functools

import numpy as np

import flash_attention_gqa_cases as GQ
from flash_attention_gqa_cases import BQ, T, f32_bound, round_s16, s16_bound  # noqa: F401  (re-exported to the two test files)

# name -> ([(len_q, len_kv), ...], heads, kv_heads, head_dim)
PACKS = {
    "A": ([(37, 37), (1, 130), (64, 64), (100, 164)], 6, 2, 32),
    "B": ([(300, 300), (0, 9), (7, 200), (65, 66)], 4, 1, 64),      # an entry with no queries
    "C": ([(3, 70), (1, 1), (17, 300)], 80, 1, 32),                 # G > 64: a tile lies inside one query
    "D": ([(150, 150), (64, 64)], 4, 4, 128),                       # G = 1
}
# (window_left, window_right); -1 = unbounded on that side
WINDOWS = [(-1, -1), (-1, 0), (0, 0), (15, 0), (63, 0), (64, 0), (100, 0), (20, 20), (-1, 5), (70, -1), (3, 130)]
# sides that reach past every sequence, INT_MAX included -> the window whose bits they must carry (the entry clamps a side to 65536)
INT_MAX = 2 ** 31 - 1
FAR_WINDOWS = [((3, INT_MAX), (3, -1)), ((INT_MAX, 0), (-1, 0)), ((65536, 70000), (-1, -1)), ((INT_MAX, INT_MAX), (-1, -1))]


def window_id(w):
    return f"w{w[0]}_{w[1]}".replace("-1", "x")


def cu_of(lens):
    """(cu_seqlens_q, cu_seqlens_kv) of a list of (len_q, len_kv), int32"""
    return (np.concatenate([[0], np.cumsum([l[0] for l in lens])]).astype(np.int32),
            np.concatenate([[0], np.cumsum([l[1] for l in lens])]).astype(np.int32))


def seq_shape(name, s):
    """sequence s of a pack as a shape of flash_attention_gqa_cases: (1, len_q, len_kv, heads, kv_heads, head_dim)"""
    lens, heads, kv_heads, hd = PACKS[name]
    return (1, lens[s][0], lens[s][1], heads, kv_heads, hd)


def seq_inputs(name, s):
    """q [1, heads, len_q, hd], k, v [1, kv_heads, len_kv, hd] of sequence s (BHSD, fp32, read-only): GQ.make_inputs of its shape"""
    return GQ.make_inputs(seq_shape(name, s))[:3]


def to_packed(a):
    """[1, heads, len, hd] (BHSD) -> [len, heads, hd], the rows of a sequence in the packed layout"""
    return np.ascontiguousarray(a[0].transpose(1, 0, 2))


def from_packed(y, cu, s):
    """sequence s of a packed [total, heads, hd] array as a BHSD array [1, heads, len, hd]"""
    return np.ascontiguousarray(np.asarray(y)[cu[s]:cu[s + 1]].transpose(1, 0, 2)[None])


@functools.lru_cache(maxsize=None)
def make_pack(name, order=None):
    """q [total_q, heads, hd], k, v [total_kv, kv_heads, hd], cu_seqlens_q, cu_seqlens_kv of a pack (order: a permutation of its sequences).
    Shared between tests: read-only."""
    lens = PACKS[name][0]
    order = tuple(range(len(lens))) if order is None else order
    parts = [seq_inputs(name, s) for s in order]
    out = [np.concatenate([to_packed(p[i]) for p in parts]) for i in range(3)] + list(cu_of([lens[s] for s in order]))
    for a in out:
        a.setflags(write=False)
    return tuple(out)


def visible(len_q, len_kv, window):
    """[len_q, len_kv] bool: key j takes part in query i's row"""
    wl, wr = window
    d = np.arange(len_kv)[None, :] - (np.arange(len_q)[:, None] + (len_kv - len_q))
    return ((d >= -wl) if wl >= 0 else np.ones_like(d, bool)) & ((d <= wr) if wr >= 0 else np.ones_like(d, bool))


def mask_bias(heads, len_q, len_kv, window):
    """the window as a bias of the bias entry: 0 where visible, -inf elsewhere; [1, heads, len_q, len_kv] fp32"""
    b = np.where(visible(len_q, len_kv, window), np.float32(0), np.float32(-np.inf)).astype(np.float32)
    return np.ascontiguousarray(np.broadcast_to(b, (1, heads, len_q, len_kv)))


def reference(q, k, v, window, scale=None):
    """the float64 result of one sequence on BHSD arrays: grouped (k[:, h // G]), the window as a real exclusion"""
    q, k, v = (np.asarray(a, np.float64) for a in (q, k, v))
    group = np.arange(q.shape[1]) // (q.shape[1] // k.shape[1])
    scale = q.shape[-1] ** -0.5 if not scale else scale
    s = (q @ k[:, group].transpose(0, 1, 3, 2)) * scale
    s = np.where(visible(q.shape[2], k.shape[2], window), s, -np.inf)
    p = np.exp(s - s.max(-1, keepdims=True))
    return (p / p.sum(-1, keepdims=True)) @ v[:, group]


@functools.lru_cache(maxsize=None)
def case_reference(name, s, window, s16=None):
    """the reference of sequence s of a pack (BHSD), on q, k, v rounded to the 16-bit type when s16 is given; computed once, read-only"""
    q, k, v = seq_inputs(name, s)
    if s16:
        q, k, v = (round_s16(a, s16) for a in (q, k, v))
    r = reference(q, k, v, window)
    r.setflags(write=False)
    return r


def sequences(name):
    """the indices of a pack's sequences that have queries"""
    return [s for s, (lq, _) in enumerate(PACKS[name][0]) if lq > 0]


# ---- the record table of csrc/brn_flash_varlen_plan.h and the rows of kernels/flash_attention.hip (FA_VARLEN), restated in numpy ----
def lo_of(query, off, wl):
    return np.zeros_like(query) if wl < 0 else np.maximum(0, query + off - wl)


def hi_of(query, off, wr, len_kv):
    return np.full_like(query, len_kv) if wr < 0 else np.minimum(len_kv, query + off + wr + 1)


def plan(lens, heads, kv_heads, window):
    """the records (q_start, len_q, kv_start, len_kv, q0, kt0, kt1), in the order of the table: kt1 - kt0 descending, stable"""
    G = heads // kv_heads
    wl, wr = window
    cq, ckv = cu_of(lens)
    recs = []
    for s, (lq, lkv) in enumerate(lens):
        rows, off = G * lq, lkv - lq
        for q0 in range(0, rows, BQ):
            qa, qb = np.array(q0 // G), np.array(min(q0 + BQ - 1, rows - 1) // G)
            recs.append((int(cq[s]), lq, int(ckv[s]), lkv, q0, int(lo_of(qa, off, wl)) // T, (int(hi_of(qb, off, wr, lkv)) + T - 1) // T))
    return sorted(recs, key=lambda r: -(r[6] - r[5]))              # sorted() is stable


def row_map(rec, G, window):
    """a record's 64 lane rows: query, head (within the group), lo, hi, pad; per wave (4): wave_hi (its first row's hi) and wave_lo (its
    last row's lo), what fa_tile_masks_window reads"""
    _, lq, _, lkv, q0, _, _ = rec
    wl, wr = window
    off, rem = lkv - lq, G * lq - 1 - q0
    lr = np.arange(BQ)
    row = q0 + np.minimum(lr, rem)
    query, head = row // G, row % G
    first = np.array([(q0 + min(16 * w, rem)) // G for w in range(4)])
    last = np.array([(q0 + min(16 * w + 15, rem)) // G for w in range(4)])
    return {"query": query, "head": head, "lo": lo_of(query, off, wl), "hi": hi_of(query, off, wr, lkv), "pad": lr > rem,
            "wave_hi": hi_of(first, off, wr, lkv), "wave_lo": lo_of(last, off, wl)}


def tile_flag(key0, wave_hi, wave_lo):
    """fa_tile_masks_window: whether the K / V tile at key0 can hold an excluded key for a lane of the wave"""
    return key0 + T > wave_hi or key0 < wave_lo


def emulate(q, k, v, window, scale=None, s16=None):
    """The FA_VARLEN walk of ONE sequence in numpy, fp32 arithmetic throughout, on BHSD arrays [1, heads, len_q, hd] / [1, kv_heads, len_kv,
    hd] (already rounded when s16 is given): per K / V head the records of the sequence; K / V tiles kt0 .. kt1 - 1 only; scores times
    scale * log2(e); keys outside lo .. hi - 1 (and past len_kv) excluded with -inf (att_exclude4_window), so a row whose lo lies past the
    record's first tile meets wholly excluded tiles first and keeps m = -3e38, numerators exp2(-inf + 3e38) = 0, l = 0 and O = 0 through
    them; running maximum m and sum l, O and l rescaled by exp2(m_old - m_new); numerators rounded to the 16-bit type for P v when s16 is given."""
    f = np.float32
    q, k, v = (np.asarray(a, f) for a in (q, k, v))
    _, heads, len_q, hd = q.shape
    kv_heads, len_kv = k.shape[1], k.shape[2]
    G = heads // kv_heads
    sc2 = f(f(scale if scale else f(1.0) / np.sqrt(f(hd))) * f(1.4426950408889634))
    y = np.full(q.shape, np.nan, f)
    with np.errstate(over="ignore", invalid="ignore"):
        for rec in plan([(len_q, len_kv)], heads, kv_heads, window):
            t = row_map(rec, G, window)
            for kvh in range(kv_heads):
                h, i = kvh * G + t["head"], t["query"]
                qt = q[0, h, i]
                m = np.full((BQ, 1), -3.0e38, f)
                l = np.zeros((BQ, 1), f)
                o = np.zeros((BQ, hd), f)
                for kt in range(rec[5], rec[6]):
                    keys = np.arange(kt * T, min((kt + 1) * T, len_kv))
                    s = (qt @ k[0, kvh, keys].T).astype(f) * sc2
                    s = np.where((keys[None, :] >= t["lo"][:, None]) & (keys[None, :] < t["hi"][:, None]), s, f(-np.inf))
                    mn = np.maximum(m, s.max(-1, keepdims=True))
                    alpha = np.exp2(m - mn)
                    p = np.exp2(s - mn)
                    l = l * alpha + p.sum(-1, keepdims=True, dtype=f)
                    pr = round_s16(p, s16).astype(f) if s16 else p
                    o = o * alpha + (pr @ v[0, kvh, keys]).astype(f)
                    m = mn
                real = ~t["pad"]
                y[0, h[real], i[real]] = (o / l)[real]
    return y


# ---- refusals ----
def raw_call(lib, q, k, v, cu_q, cu_kv, n_seqs, heads, kv_heads, head_dim, wl, wr, scale, y, loc=0):
    """brn_flash_attention_varlen_forward with the integers exactly as given; q, k, v, y, cu_q, cu_kv: numpy arrays, integers taken as
    addresses, or None"""
    ptr = lambda a: a if a is None or isinstance(a, int) else a.ctypes.data
    st = lib.brn_flash_attention_varlen_forward(ptr(q), ptr(k), ptr(v), ptr(cu_q), ptr(cu_kv), n_seqs, heads, kv_heads, head_dim, wl, wr, scale, ptr(y),
                                                loc, 0, None)
    return st, (lib.brn_last_error() or b"").decode()


@functools.lru_cache(maxsize=None)
def _refusal_buffers():
    return tuple(np.zeros(2 * 2 * 32 * 256, np.float32) for _ in range(4))


_CU = {}


def _cu(*vals):
    """an int32 array that lives as long as the module (the refusal list holds addresses of it)"""
    return _CU.setdefault(vals, np.array(vals, np.int32))


def refusals():
    """(name, arguments of raw_call after lib, words the message must contain): every limit of the header.  The buffers hold what the
    well-formed neighbours of each call would read; the refused calls read nothing but the cu arrays."""
    q, k, v, y = _refusal_buffers()
    a = q.ctypes.data
    assert a % 16 == 0
    c = _cu(0, 16, 32)
    ok = (c, c, 2, 2, 1, 32)                    # cu_q, cu_kv, n_seqs, heads, kv_heads, head_dim
    big = _cu(*(65536 * i for i in range(33)))
    return [
        ("null q", (None, k, v) + ok + (-1, -1, 0.0, y), "null q, k, v or y"),
        ("null y", (q, k, v) + ok + (-1, -1, 0.0, None), "null q, k, v or y"),
        ("null cu_seqlens_q", (q, k, v, None, c, 2, 2, 1, 32, -1, -1, 0.0, y), "null cu_seqlens_q or cu_seqlens_kv"),
        ("null cu_seqlens_kv", (q, k, v, c, None, 2, 2, 1, 32, -1, -1, 0.0, y), "null cu_seqlens_q or cu_seqlens_kv"),
        ("head_dim 48", (q, k, v, c, c, 2, 2, 1, 48, -1, -1, 0.0, y), "head_dim must be 32, 64 or 128"),
        ("heads 0", (q, k, v, c, c, 2, 0, 1, 32, -1, -1, 0.0, y), "heads >= 1"),
        ("kv_heads 0", (q, k, v, c, c, 2, 2, 0, 32, -1, -1, 0.0, y), "1 <= kv_heads <= heads"),
        ("kv_heads > heads", (q, k, v, c, c, 2, 2, 4, 32, -1, -1, 0.0, y), "1 <= kv_heads <= heads"),
        ("heads % kv_heads != 0", (q, k, v, c, c, 2, 6, 4, 32, -1, -1, 0.0, y), "heads % kv_heads == 0"),
        ("n_seqs 0", (q, k, v, c, c, 0, 2, 1, 32, -1, -1, 0.0, y), "n_seqs >= 1"),
        ("cu_q[0] != 0", (q, k, v, _cu(1, 16, 32), c, 2, 2, 1, 32, -1, -1, 0.0, y), "must start at 0"),
        ("cu_kv[0] != 0", (q, k, v, c, _cu(-1, 16, 32), 2, 2, 1, 32, -1, -1, 0.0, y), "must start at 0"),
        ("decreasing cu_q", (q, k, v, _cu(0, 16, 8), c, 2, 2, 1, 32, -1, -1, 0.0, y), "non-decreasing"),
        ("decreasing cu_kv", (q, k, v, c, _cu(0, 33, 32), 2, 2, 1, 32, -1, -1, 0.0, y), "non-decreasing"),
        ("len_q 65537", (q, k, v, _cu(0, 65537), _cu(0, 16), 1, 1, 1, 32, -1, -1, 0.0, y), "len_q, len_kv <= 65536"),
        ("len_kv 65537", (q, k, v, _cu(0, 16), _cu(0, 65537), 1, 1, 1, 32, -1, -1, 0.0, y), "len_q, len_kv <= 65536"),
        ("len_kv 0 with len_q 1", (q, k, v, _cu(0, 16, 17), _cu(0, 16, 16), 2, 2, 1, 32, -1, -1, 0.0, y), "len_kv >= 1 wherever len_q >= 1"),
        ("total_q 0", (q, k, v, _cu(0, 0, 0), c, 2, 2, 1, 32, -1, -1, 0.0, y), "total_q >= 1"),
        ("causal, len_kv < len_q", (q, k, v, _cu(0, 16, 33), c, 2, 2, 1, 32, -1, 0, 0.0, y), "a window requires len_kv >= len_q"),
        ("left window, len_kv < len_q", (q, k, v, _cu(0, 17, 32), c, 2, 2, 1, 32, 5, -1, 0.0, y), "a window requires len_kv >= len_q"),
        ("window_left -2", (q, k, v) + ok + (-2, 0, 0.0, y), "window_left >= -1"),
        ("window_right -2", (q, k, v) + ok + (0, -2, 0.0, y), "window_right >= -1"),
        ("2^31 packed rows", (q, k, v, _cu(0, 65536), _cu(0, 16), 1, 32768, 1, 32, -1, -1, 0.0, y), "G * len_q < 2^31"),
        ("2^31 workgroups", (q, k, v, big, big, 32, 65536, 65536, 32, -1, -1, 0.0, y), "packed-row tiles * kv_heads < 2^31"),
        ("negative scale", (q, k, v) + ok + (-1, -1, -0.5, y), "scale must be finite and >= 0"),
        ("NaN scale", (q, k, v) + ok + (-1, -1, float("nan"), y), "scale must be finite and >= 0"),
        ("infinite scale", (q, k, v) + ok + (-1, -1, float("inf"), y), "scale must be finite and >= 0"),
        ("y is q", (q, k, v) + ok + (-1, -1, 0.0, q), "overlap"),
        ("y overlaps the end of v", (q, k, v) + ok + (-1, -1, 0.0, v.ctypes.data + 4 * (32 * 1 * 32 - 4)), "overlap"),
        ("misaligned device k", (q, a + 4096 + 4, v) + ok + (-1, -1, 0.0, y, 1), "16-byte aligned"),
    ]
