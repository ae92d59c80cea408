"""What tests/test_flash_attention_paged_gpu.py and tests/test_flash_attention_paged_cpu.py share: the cases of
brn_flash_attention_paged_forward, the deterministic pool builder (shuffled pages, NaN wherever the entry must not read), the float64
reference with per-sequence lengths, the numpy emulation of the paged walk (flash_attention_splitkv_cases.emulate's arithmetic with the
limit and the tile count of each sequence, plus the row no split has a key for), the refusal list and a raw ctypes call.

Inputs, rounding, the row map and the bounds are those of flash_attention_gqa_cases / flash_attention_splitkv_cases, imported and not
edited: sequence b of a case is rows 0 .. len_b - 1 of batch entry b of make_inputs at seq_kv = max(kv_lens)."""
import ctypes
import functools

import numpy as np

import flash_attention_gqa_cases as GQ
import flash_attention_splitkv_cases as SK
from flash_attention_splitkv_cases import BQ, LN2, MODES, T, f32_bound, in_layout, kind_scale, lse_bound, round_s16, s16_bound, shape_id, y_bound  # noqa: F401

PAGE_SIZES = (16, 32, 64, 128, 256)

# ((batch, seq_q, heads, kv_heads, head_dim), page_size, kv_lens, kinds, causals, kv_splits): max_kv_len = max(kv_lens),
# max_pages = ceil(max_kv_len / page_size) + 1.  The smallest shapes at which each mechanism can go wrong
_TABLE = [
    ((2, 1, 8, 2, 64), 16, (300, 37), ("std1",), (0, 1), (1, 2, 3, 5)),     # 4 pages per tile, ragged last page and tile; the short sequence is empty in every split but the first
    ((3, 1, 5, 1, 128), 64, (1000, 512, 1), ("std1",), (1,), (4, 16)),      # page == tile, a full last page, a single key, multi-query
    ((1, 100, 4, 1, 64), 32, (110,), ("std1",), (1,), (2,)),                # rows of a walked tile with no key in split 1
    ((2, 7, 16, 2, 64), 128, (200, 129), ("std1",), (1,), (4,)),            # page larger than a tile, one key on the second page, G 8
    ((3, 4, 4, 2, 32), 256, (700, 0, 2), ("std1",), (1,), (3,)),            # an empty sequence; causal rows with len < seq_q
    ((1, 3, 80, 1, 32), 16, (70,), ("std1",), (0,), (2,)),                  # G 80 > 64
    ((2, 17, 6, 2, 32), 32, (300, 150), ("rising", "falling"), (1,), (3, 5)),   # splits whose weights underflow to exactly 0
    ((1, 1, 4, 4, 32), 64, (64,), ("std1",), (0,), (4,)),                   # S collapses to 1, no workspace
]
CASES = [(shape, page, lens, kind, causal, ks) for shape, page, lens, kinds, causals, splits in _TABLE for kind in kinds for causal in causals for ks in splits]
FIRST, THIRD, FIFTH = (next(c for c in CASES if c[0] == _TABLE[i][0] and c[5] > 1) for i in (0, 2, 4))     # (a split case of the row)
COLLAPSED = CASES[-1]


def case_id(case):
    shape, page, lens, kind, causal, ks = case
    return f"{shape_id(shape)}-p{page}-L{'_'.join(str(v) for v in lens)}-{kind}{'-causal' if causal else ''}-s{ks}"


def max_len(case):
    return max(case[2])


def max_pages_of(case, page=None):
    return (max_len(case) + (page or case[1]) - 1) // (page or case[1]) + 1


def full_shape(case):
    """the (batch, seq_q, seq_kv, heads, kv_heads, head_dim) of make_inputs that holds the case's logical q, k, v"""
    batch, seq_q, heads, kv_heads, hd = case[0]
    return (batch, seq_q, max_len(case), heads, kv_heads, hd)


def logical_inputs(case):
    """q [batch, heads, seq_q, hd], k, v [batch, kv_heads, max_len, hd] (BHSD, read-only); sequence b is k[b, :, :len_b]"""
    return GQ.make_inputs(full_shape(case), case[3])[:3]


def clamp_len(length, max_kv_len):
    return min(max(int(length), 0), max_kv_len)


def row_limits(seq_q, length, causal):
    """[seq_q] first excluded key of each query of a sequence of `length` keys (<= 0: the row sees nothing)"""
    return np.minimum(length, np.arange(seq_q) + (length - seq_q) + 1) if causal else np.full(seq_q, length)


def all_empty_rows(case, b=None):
    """how many (batch entry, head, query) rows of the case (of sequence b) see no key at all"""
    (batch, seq_q, heads, _, _), _, lens, _, causal, _ = case
    return sum(int((row_limits(seq_q, lens[i], causal) <= 0).sum()) * heads for i in (range(batch) if b is None else (b,)))


def empty_partial_rows(case):
    """how many (split, batch entry, head, query) partial rows see no key of their split: limit <= the split's first key"""
    (batch, seq_q, heads, _, _), _, lens, _, causal, ks = case
    S, tps = SK.plan(max_len(case), ks)
    return sum(int((row_limits(seq_q, lens[b], causal) <= s * tps * T).sum()) * heads for b in range(batch) for s in range(S))


def dense_splits(case, b):
    """kv_splits of the brn_flash_attention_splitkv_forward call on sequence b alone (seq_kv = len_b) that walks the tile ranges the paged
    call walks for it, or None where the split entry does not accept the sequence (len_b == 0; causal with len_b < seq_q)"""
    (_, seq_q, _, _, _), _, lens, _, causal, ks = case
    L = lens[b]
    if L < 1 or (causal and L < seq_q):
        return None
    _, tps = SK.plan(max_len(case), ks)
    nkt_b = (L + T - 1) // T
    if nkt_b <= tps:
        return 1
    ks_b = (nkt_b + tps - 1) // tps
    assert SK.plan(L, ks_b) == (ks_b, tps), (case_id(case), b, SK.plan(L, ks_b), tps)
    return ks_b


# coverage that must not vanish silently when a length or a split is edited
assert all_empty_rows(FIFTH, 1) > 0 and all_empty_rows(FIFTH, 2) > 0 and all_empty_rows(FIFTH, 0) == 0
assert all(empty_partial_rows(c) > 0 for c in (FIRST, THIRD, FIFTH))
assert SK.plan(max_len(COLLAPSED), COLLAPSED[5])[0] == 1
for _c in CASES:
    assert _c[1] in PAGE_SIZES
    for _b in range(_c[0][0]):
        dense_splits(_c, _b)               # asserts that every sequence the split entry accepts has a dense equivalent


# ---- the pool ----
@functools.lru_cache(maxsize=None)
def build_pool(case, page=None, shuffle=True, spare=5):
    """k_pages, v_pages [n_pages, page, kv_heads, hd], block_table [batch, max_pages] int32, kv_lens [batch] int32 of the case's logical
    batch (read-only).  Deterministic.  The used pages are a seeded permutation of the pool (shuffle) or 0, 1, 2, .. in sequence order
    (identity); the pool has `spare` pages more than are used, and EVERY float the entry must not read is NaN: the unused pages, the rows
    of a sequence's last page at or past len_b, and the table entries at or past a sequence's last page point at an unused (NaN) page."""
    page = page or case[1]
    batch, _, _, kv_heads, hd = case[0]
    lens = case[2]
    _, k, v = logical_inputs(case)
    need = [(L + page - 1) // page for L in lens]
    n_pages = sum(need) + spare
    rng = np.random.default_rng(977 + page + 13 * sum(lens))
    order = rng.permutation(n_pages) if shuffle else np.arange(n_pages)
    used, unused = order[:sum(need)], order[sum(need):]
    kp = np.full((n_pages, page, kv_heads, hd), np.nan, np.float32)
    vp = np.full((n_pages, page, kv_heads, hd), np.nan, np.float32)
    max_pages = max_pages_of(case, page)
    table = np.empty((batch, max_pages), np.int32)
    at = 0
    for b, L in enumerate(lens):
        table[b] = unused[(b + np.arange(max_pages)) % len(unused)]
        for j in range(need[b]):
            pg = int(used[at])
            at += 1
            table[b, j] = pg
            rows = min(page, L - j * page)
            kp[pg, :rows] = k[b, :, j * page:j * page + rows].transpose(1, 0, 2)
            vp[pg, :rows] = v[b, :, j * page:j * page + rows].transpose(1, 0, 2)
    out = (kp, vp, table, np.asarray(lens, np.int32))
    for a in out:
        a.setflags(write=False)
    return out


def gather(kp, vp, table, b, length):
    """sequence b's first `length` keys out of the pool -> k, v [1, kv_heads, length, hd] (BHSD)"""
    page = kp.shape[1]
    keys = np.arange(length)
    pg = table[b, keys // page]
    return tuple(np.ascontiguousarray(a[pg, keys % page].transpose(1, 0, 2)[None]) for a in (kp, vp))


# ---- float64 reference ----
def reference(q, k, v, lens, causal=False, scale=None):
    """(y [batch, heads, seq_q, hd], lse [batch, heads, seq_q]) in float64 on BHSD arrays, sequence b = k[b, :, :lens[b]]; a row with no
    visible key is y = 0, lse = -inf"""
    q, k, v = (np.asarray(a, np.float64) for a in (q, k, v))
    batch, heads, seq_q, hd = q.shape
    group = np.arange(heads) // (heads // k.shape[1])
    scale = hd ** -0.5 if not scale else scale
    y = np.zeros(q.shape)
    lse = np.full(q.shape[:3], -np.inf)
    for b in range(batch):
        L = int(lens[b])
        if L == 0:
            continue
        s = (q[b] @ k[b, group, :L].transpose(0, 2, 1)) * scale
        s = np.where(np.arange(L)[None, :] < row_limits(seq_q, L, causal)[:, None], s, -np.inf)
        mx = s.max(-1)
        seen = np.isfinite(mx)
        p = np.exp(s - np.where(seen, mx, 0.0)[..., None])
        l = np.where(seen, p.sum(-1), 1.0)
        y[b] = np.where(seen[..., None], (p @ v[b, group, :L]) / l[..., None], 0.0)
        lse[b] = np.where(seen, mx + np.log(l), -np.inf)
    return y, lse


@functools.lru_cache(maxsize=None)
def case_reference(case, s16=None):
    """(y, lse) of a case in float64, on q, k, v rounded to the 16-bit type when s16 is given; computed once"""
    q, k, v = logical_inputs(case)
    if s16:
        q, k, v = (round_s16(a, s16) for a in (q, k, v))
    out = reference(q, k, v, case[2], case[4], kind_scale(case[3]))
    for a in out:
        a.setflags(write=False)
    return out


# ---- the paged walk and the combine of kernels/flash_attention.hip (FA_PAGED, flash_split_combine_kernel<true>), restated in numpy ----
def emulate(q, fetch, lens, max_kv_len, kv_heads, causal, scale, kv_splits, s16=None):
    """SK.emulate's arithmetic with each sequence's own limit and tile count.  q [batch, heads, seq_q, hd] fp32 (already rounded when s16
    is given); fetch(b, kvh, keys) -> (k rows, v rows) [len(keys), hd] of sequence b (only keys below its clamped length are asked for).
    S and tps come from max_kv_len; split s of sequence b walks tiles s * tps .. min((s + 1) * tps, the row tile's nkt at len_b) - 1.
    The combine takes the weights against 0 where no split has a key and selects y = 0, lse = -inf there.  Returns y, lse, O_part
    [S, R, hd], lse2_part [S, R]."""
    f = np.float32
    q = np.asarray(q, f)
    batch, heads, seq_q, hd = q.shape
    G = heads // kv_heads
    S, tps = SK.plan(max_kv_len, kv_splits)
    sc2 = f(f(scale if scale else f(1.0) / np.sqrt(f(hd))) * f(1.4426950408889634))
    o_part = np.full((S, batch, heads, seq_q, hd), np.nan, f)
    l2_part = np.full((S, batch, heads, seq_q), np.nan, f)
    with np.errstate(divide="ignore", invalid="ignore"):
        for b in range(batch):
            L = clamp_len(lens[b], max_kv_len)
            for kvh in range(kv_heads):
                for t in GQ.row_map(G, seq_q, L, causal):
                    h, i = kvh * G + t["head"], t["query"]
                    qt = q[b, h, i]
                    real = ~t["pad"]
                    for s in range(S):
                        m = np.full((BQ, 1), -3.0e38, f)
                        l = np.zeros((BQ, 1), f)
                        o = np.zeros((BQ, hd), f)
                        for kt in range(s * tps, min((s + 1) * tps, t["nkt"])):
                            keys = np.arange(kt * T, min((kt + 1) * T, L))
                            kk, vv = (np.asarray(a, f) for a in fetch(b, kvh, keys))
                            sc = (qt @ kk.T).astype(f) * sc2
                            sc = np.where(keys[None, :] < t["limit"][:, None], sc, f(-np.inf))
                            mn = np.maximum(m, sc.max(-1, keepdims=True))
                            alpha = np.exp2(m - mn)
                            p = np.exp2(sc - mn)
                            l = l * alpha + p.sum(-1, keepdims=True, dtype=f)
                            pr = round_s16(p, s16).astype(f) if s16 else p
                            o = o * alpha + (pr @ vv).astype(f)
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
            none = np.isneginf(M)
            M = np.where(none, f(0), M)
            acc = np.zeros(o_part.shape[1:], f)
            wsum = np.zeros(M.shape, f)
            for s in range(S):
                w = np.exp2(l2_part[s] - M).astype(f)
                acc = (acc + w[..., None] * o_part[s]).astype(f)
                wsum = (wsum + w).astype(f)
            y = np.where(none[..., None], f(0), acc / wsum[..., None]).astype(f)
            lse = np.where(none, f(-np.inf), (M + np.log2(wsum).astype(f)) * f(LN2)).astype(f)
    R = batch * heads * seq_q
    return y, lse, o_part.reshape(S, R, hd), l2_part.reshape(S, R)


def fetch_dense(k, v):
    return lambda b, kvh, keys: (k[b, kvh, keys], v[b, kvh, keys])


def fetch_paged(kp, vp, table):
    """the kernels' address rule: row key % page_size of page clamp(block_table[b][key // page_size], 0, n_pages - 1)"""
    page, last = kp.shape[1], kp.shape[0] - 1
    return lambda b, kvh, keys: tuple(a[np.clip(table[b, keys // page], 0, last), keys % page, kvh] for a in (kp, vp))


@functools.lru_cache(maxsize=None)
def case_emulation(case, mode, paged=False):
    """the emulation of a case on its logical tensors, or (paged) through the shuffled NaN-filled pool of build_pool"""
    shape, _, lens, kind, causal, ks = case
    s16 = None if mode == "f32" else mode
    r = (lambda a: round_s16(a, s16)) if s16 else (lambda a: a)
    q, k, v = logical_inputs(case)
    if paged:
        kp, vp, table, _ = build_pool(case)
        fetch = fetch_paged(r(kp), r(vp), table)
    else:
        fetch = fetch_dense(r(k), r(v))
    out = emulate(r(q), fetch, lens, max_len(case), shape[3], causal, kind_scale(kind), ks, s16)
    for a in out:
        a.setflags(write=False)
    return out


# ---- raw calls and refusals ----
def raw_call(lib, q, kp, vp, table, lens, batch, seq_q, max_kv_len, heads, kv_heads, head_dim, n_pages, page_size, max_pages, layout, causal, scale,
             kv_splits, y, lse, ws, ws_floats, loc=0, stream=None):
    """brn_flash_attention_paged_forward with the integers exactly as given; the pointers: numpy arrays, integers taken as addresses, or None"""
    ptr = lambda a: a if a is None or isinstance(a, int) else a.ctypes.data
    st = lib.brn_flash_attention_paged_forward(ptr(q), ptr(kp), ptr(vp), ptr(table), ptr(lens), batch, seq_q, max_kv_len, heads, kv_heads, head_dim, n_pages,
                                               page_size, max_pages, layout, causal, scale, kv_splits, ptr(y), ptr(lse), ptr(ws), ws_floats, loc, 0, stream)
    return st, (lib.brn_last_error() or b"").decode()


@functools.lru_cache(maxsize=None)
def _refusal_buffers():
    return tuple(np.zeros(2 * 2 * 32 * 256, np.float32) for _ in range(6)) + (np.zeros(2 * 13, np.int32), np.full(2, 200, np.int32))


def refusals():
    """(name, arguments of raw_call after lib, words the message must contain).  The well-formed neighbour of every call is
    (q, kp, vp, table, lens, 2, 16, 200, 2, 1, 32, 20, 16, 13, 0, 0, 0.0, 2, y, lse, ws, 4224): batch 2, seq_q 16, max_kv_len 200, heads 2,
    kv_heads 1, head_dim 32, a pool of 20 pages of 16 keys, 13 table entries per sequence (208 >= 200), nkt 4, S 2, R 64,
    2 * 64 * 33 = 4224 workspace floats.  The refused calls read nothing."""
    q, kp, vp, y, lse, ws, table, lens = _refusal_buffers()
    a = q.ctypes.data
    assert a % 16 == 0 and table.ctypes.data % 4 == 0
    ins = (q, kp, vp, table, lens)
    tail = (y, lse, ws, 4224)
    ok = (2, 16, 200, 2, 1, 32, 20, 16, 13, 0, 0, 0.0, 2)

    def sub(**kw):
        names = ("batch", "seq_q", "max_kv_len", "heads", "kv_heads", "head_dim", "n_pages", "page_size", "max_pages", "layout", "causal", "scale", "kv_splits")
        assert set(kw) <= set(names)
        return tuple(kw.get(n, d) for n, d in zip(names, ok))

    return [
        ("null block_table", (q, kp, vp, None, lens) + ok + tail, "null block_table or kv_lens"),
        ("null kv_lens", (q, kp, vp, table, None) + ok + tail, "null block_table or kv_lens"),
        ("page_size 48", ins + sub(page_size=48) + tail, "page_size must be 16, 32, 64, 128 or 256"),
        ("page_size 8", ins + sub(page_size=8, max_pages=32) + tail, "page_size must be 16, 32, 64, 128 or 256"),
        ("page_size 512", ins + sub(page_size=512) + tail, "page_size must be 16, 32, 64, 128 or 256"),
        ("n_pages 0", ins + sub(n_pages=0) + tail, "n_pages >= 1, max_pages >= 1"),
        ("max_pages 0", ins + sub(max_pages=0) + tail, "n_pages >= 1, max_pages >= 1"),
        ("2^31 keys in the pool", ins + sub(n_pages=2 ** 23, page_size=256) + tail, "n_pages * page_size < 2^31"),
        ("max_kv_len 0", ins + sub(max_kv_len=0) + tail, "1 <= max_kv_len <= min(65536, max_pages * page_size)"),
        ("max_kv_len 65537", ins + sub(max_kv_len=65537, max_pages=5000) + tail, "1 <= max_kv_len <= min(65536, max_pages * page_size)"),
        ("max_kv_len past the table", ins + sub(max_kv_len=209) + tail, "1 <= max_kv_len <= min(65536, max_pages * page_size)"),
        ("kv_splits -1", ins + sub(kv_splits=-1) + tail, "0 <= kv_splits <= 1024"),
        ("kv_splits 1025", ins + sub(kv_splits=1025) + tail, "0 <= kv_splits <= 1024"),
        ("workspace NULL, S 2", ins + ok + (y, lse, None, 0), "4224 floats"),
        ("workspace too small", ins + ok + (y, lse, ws, 4223), "4224 floats"),
        ("2^31 workgroups with the splits", ins + (32768, 1024, 65536, 64, 64, 32, 20, 256, 256, 0, 0, 0.0, 1024) + tail, "S < 2^31"),
        ("lse is y", ins + ok + (y, y, ws, 4224), "overlap"),
        ("lse is k_pages", ins + ok + (y, kp, ws, 4224), "overlap"),
        ("y is the table", ins + ok + (table.ctypes.data, lse, ws, 4224), "overlap"),
        ("workspace is kv_lens", ins + ok + (y, lse, lens.ctypes.data, 4224), "overlap"),
        ("workspace overlaps the end of v_pages", ins + ok + (y, lse, vp.ctypes.data + 4 * (20 * 16 * 32 - 4), 4224), "overlap"),
        ("workspace overlaps lse", ins + ok + (y, lse, lse.ctypes.data + 4 * 60, 4224), "overlap"),
        ("misaligned device lse", ins + ok + (y, lse.ctypes.data + 4096 + 4, ws, 4224, 1), "16-byte aligned"),
        ("misaligned device workspace", ins + ok + (y, lse, ws.ctypes.data + 4096 + 8, 4224, 1), "16-byte aligned"),
        ("misaligned device v_pages", (q, kp, a + 4096 + 4, table, lens) + ok + tail + (1,), "16-byte aligned"),
        ("misaligned device block_table", (q, kp, vp, table.ctypes.data + 2, lens) + ok + tail + (1,), "4-byte aligned"),
        # every other limit of the split entry, under this entry's prefix
        ("kv_heads 0", ins + sub(kv_heads=0) + tail, "1 <= kv_heads <= heads"),
        ("heads % kv_heads != 0", ins + sub(heads=6, kv_heads=4) + tail, "heads % kv_heads == 0"),
        ("2^31 tiles", ins + (32768, 65536, 16, 64, 64, 32, 20, 16, 13, 0, 0, 0.0, 1) + tail, "batch * kv_heads * ceil(G * seq_q / 64) < 2^31"),
        ("2^31 packed rows", ins + (1, 65536, 16, 32768, 1, 32, 20, 16, 13, 0, 0, 0.0, 1) + tail, "G * seq_q < 2^31"),
        ("head_dim 48", ins + sub(head_dim=48) + tail, "head_dim must be 32, 64 or 128"),
        ("seq_q 0", ins + sub(seq_q=0) + tail, "1 <= seq_q, seq_kv <= 65536"),
        ("batch 0", ins + sub(batch=0) + tail, "batch >= 1, heads >= 1"),
        ("layout 2", ins + sub(layout=2) + tail, "layout must be 0"),
        ("causal 2", ins + sub(causal=2) + tail, "causal must be 0 or 1"),
        ("NaN scale", ins + sub(scale=float("nan")) + tail, "scale must be finite and >= 0"),
        ("null k_pages", (q, None, vp, table, lens) + ok + tail, "null q, k_pages, v_pages or y"),
        ("y is q", ins + ok + (q, lse, ws, 4224), "overlap"),
    ]
