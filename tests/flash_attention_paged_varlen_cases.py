"""What tests/test_flash_attention_paged_varlen_gpu.py, tests/test_kv_cache_append_varlen_gpu.py and
tests/test_flash_attention_paged_varlen_cpu.py share: the mixed prefill / decode pack of brn_flash_attention_paged_varlen_forward and
brn_kv_cache_append_varlen, its logical tensors, the pool builder in the style of flash_attention_paged_cases.build_pool (shuffled pages,
NaN wherever an entry must not read), the numpy restatement of the clamp rule and of the plan function, raw ctypes calls and the refusal
lists.

The yardstick of the GPU tests is the project's own: every sequence of a packed call must carry the bits of the existing paged entries
called on that sequence alone, so no tolerance is introduced here.  The float64 reference and its bounds are
flash_attention_paged_cases', imported and not edited."""
import functools

import numpy as np

import flash_attention_paged_cases as PG
import kv_cache_cases as KC
import kv_fp8_cases as F8

T = 64                                       # packed rows per row tile, keys per K / V tile
MODES = ("f32", "bf16", "f16")
# the pack, (n_b, len_b): len_b counts the keys AFTER the n_b new ones were appended
PACK = ((1, 130),      # decode
        (0, 77),       # idle slot
        (17, 17),      # fresh prefill; with G = 4 this is 68 packed rows, two tiles
        (5, 200),      # chunk over a long prefix
        (33, 97),      # chunk over a medium prefix
        (3, 2))        # first causal row empty (query 0 sees key j <= 0 + 2 - 3)
TOTAL_Q = 64                                 # 59 tokens, 5 padding tokens
MAX_KV = 256
PAGES = (16, 64)
CU0 = (0, 2)                                 # the pack starts at token 0, or behind two padding tokens
CONFIGS = ((4, 1, 32), (4, 1, 64), (4, 1, 128), (2, 2, 64))      # (heads, kv_heads, head_dim): every head_dim on the first pairing
CAUSALS = (0, 1)
SPLITS = (1, 3)                              # kv_splits 3 at nkt = 4: tps 2, S 2
assert sum(n for n, _ in PACK) == 59 and max(L for _, L in PACK) <= MAX_KV and PACK[2][0] * 4 > T


def pools_of(mode):
    """the pool types a compute mode is run over: fp32, its own 16-bit type (the fp32 kernel reads both), e4m3"""
    return (None, "bf16", "f16", "e4m3") if mode == "f32" else (None, mode, "e4m3")


def config_id(cfg):
    return f"h{cfg[0]}kv{cfg[1]}d{cfg[2]}"


def cu_of(pack, start=0):
    return np.concatenate([[start], start + np.cumsum([n for n, _ in pack])]).astype(np.int32)


# ---- the clamp rule and the plan function of include/birefnet_hip.h, restated ----
def clamp_starts(cu, total_q):
    """s_b: the running maximum of the values clamped to 0 .. total_q, in exact integers"""
    return np.maximum.accumulate(np.clip(np.asarray(cu, np.int64), 0, total_q))


def tiles_of(starts, G):
    """row tiles of 64 packed rows per sequence"""
    return (G * np.diff(starts) + T - 1) // T


def plan_ref(cu, total_q, G):
    """what the device-side plan holds: the starts, then the exclusive prefix of the tiles with the total at the end"""
    s = clamp_starts(cu, total_q)
    return np.concatenate([s, [0], np.cumsum(tiles_of(s, G))]).astype(np.int64)


def t_max(G, total_q, n_seqs):
    return (G * total_q + 63 * min(n_seqs, total_q)) // 64


def split_auto(base, nkt):
    """flash_split_auto of csrc/brn_flash_split_plan.h: fill 512 workgroups, no split below 2 tiles, at most 1024"""
    if base >= 512:
        return 1
    return min((512 + base - 1) // base, max(1, nkt // 2), 1024)


def host_plan(total_q, n_seqs, max_kv_len, heads, kv_heads, head_dim, kv_splits):
    """(S, tps, workspace_floats, plan_ints) as the header states them"""
    G = heads // kv_heads
    nkt = (max_kv_len + T - 1) // T
    ask = kv_splits if kv_splits else split_auto(kv_heads * t_max(G, total_q, n_seqs), nkt)
    tps = (nkt + ask - 1) // ask
    S = (nkt + tps - 1) // tps
    return S, tps, S * heads * total_q * (head_dim + 1), 2 * (n_seqs + 1)


# ---- logical tensors: a sequence's data depends on its (n_b, len_b) and the configuration alone, not on its place in a pack ----
@functools.lru_cache(maxsize=None)
def sequence(cfg, n, L):
    """q [n, heads, hd], k, v [L, kv_heads, hd] fp32 (read-only)"""
    heads, kv_heads, hd = cfg
    rng = np.random.default_rng(1000 * n + L + 7 * hd + heads)
    out = (rng.standard_normal((n, heads, hd)).astype(np.float32), rng.standard_normal((L, kv_heads, hd)).astype(np.float32),
           rng.standard_normal((L, kv_heads, hd)).astype(np.float32))
    for a in out:
        a.setflags(write=False)
    return out


def packed_q(cfg, pack, cu, total_q):
    """q [total_q, heads, hd]: each sequence's rows at cu[b]; every padding row NaN (no kernel may read it)"""
    q = np.full((total_q, cfg[0], cfg[2]), np.nan, np.float32)
    for b, (n, L) in enumerate(pack):
        q[cu[b]:cu[b] + n] = sequence(cfg, n, L)[0]
    return q


@functools.lru_cache(maxsize=None)
def build_pool(cfg, pack, page, max_kv_len=MAX_KV, spare=5):
    """k_pages, v_pages [n_pages, page, kv_heads, hd] fp32, block_table [n_seqs, max_pages] int32, kv_lens [n_seqs] int32 (read-only), in
    the style of PG.build_pool: the used pages are a seeded permutation of the pool, and EVERY float an entry must not read is NaN: the
    unused pages, the rows of a last page at or past len_b; table entries at or past a sequence's last page name unused pages."""
    _, kv_heads, hd = cfg
    need = [(L + page - 1) // page for _, L in pack]
    n_pages = sum(need) + spare
    rng = np.random.default_rng(311 + page + 17 * sum(L for _, L in pack) + len(pack))
    order = rng.permutation(n_pages)
    used, unused = order[:sum(need)], order[sum(need):]
    kp = np.full((n_pages, page, kv_heads, hd), np.nan, np.float32)
    vp = np.full((n_pages, page, kv_heads, hd), np.nan, np.float32)
    max_pages = (max_kv_len + page - 1) // page + 1
    table = np.empty((len(pack), max_pages), np.int32)
    at = 0
    for b, (n, L) in enumerate(pack):
        _, k, v = sequence(cfg, n, L)
        table[b] = unused[(b + np.arange(max_pages)) % len(unused)]
        for j in range(need[b]):
            pg = int(used[at])
            at += 1
            table[b, j] = pg
            rows = min(page, L - j * page)
            kp[pg, :rows] = k[j * page:j * page + rows]
            vp[pg, :rows] = v[j * page:j * page + rows]
    out = (kp, vp, table, np.asarray([L for _, L in pack], np.int32))
    for a in out:
        a.setflags(write=False)
    return out


def scales_of(kv_heads):
    """the non-trivial per-head scales of the e4m3 pools"""
    return F8.per_head_scales(kv_heads)


@functools.lru_cache(maxsize=None)
def typed_pool(cfg, pack, page, pool, max_kv_len=MAX_KV):
    """build_pool stored as `pool` says -> (k, v, k_scale, v_scale, table, lens): None fp32; "bf16" / "f16" uint16 bit patterns (a NaN
    stays a NaN); "e4m3" bytes at scales_of, F8.UNREAD wherever the fp32 pool holds NaN"""
    kp, vp, table, lens = build_pool(cfg, pack, page, max_kv_len)
    ks = vs = None
    if pool == "e4m3":
        ks, vs = scales_of(cfg[1])
        kp, vp = F8.quant_pool(kp, ks), F8.quant_pool(vp, vs)
    elif pool is not None:
        kp, vp = KC.to_bits(kp, pool), KC.to_bits(vp, pool)
    for a in (kp, vp):
        a.setflags(write=False)
    return kp, vp, ks, vs, table, lens


# ---- raw calls ----
_ptr = KC._ptr


def raw_plan(lib, total_q, n_seqs, max_kv_len, heads, kv_heads, head_dim, kv_splits):
    import ctypes
    S, tps, nws, npl = ctypes.c_int(-1), ctypes.c_int(-1), ctypes.c_size_t(0), ctypes.c_size_t(0)
    st = lib.brn_flash_attention_paged_varlen_plan(total_q, n_seqs, max_kv_len, heads, kv_heads, head_dim, kv_splits, ctypes.byref(S), ctypes.byref(tps),
                                                   ctypes.byref(nws), ctypes.byref(npl))
    return st, (lib.brn_last_error() or b"").decode(), (S.value, tps.value, nws.value, npl.value)


def raw_attend(lib, q, kp, vp, pool_type, ks, vs, table, lens, cu, total_q, n_seqs, max_kv_len, heads, kv_heads, head_dim, n_pages, page_size, max_pages, causal, scale,
               kv_splits, y, lse, ws, ws_floats, plan, plan_ints, loc=0, stream=None):
    """brn_flash_attention_paged_varlen_forward with the integers exactly as given; pointers: numpy arrays, integers taken as addresses, None"""
    st = lib.brn_flash_attention_paged_varlen_forward(_ptr(q), _ptr(kp), _ptr(vp), pool_type, _ptr(ks), _ptr(vs), _ptr(table), _ptr(lens), _ptr(cu), total_q, n_seqs,
                                                      max_kv_len, heads, kv_heads, head_dim, n_pages, page_size, max_pages, causal, scale, kv_splits, _ptr(y), _ptr(lse),
                                                      _ptr(ws), ws_floats, _ptr(plan), plan_ints, loc, 0, stream)
    return st, (lib.brn_last_error() or b"").decode()


def raw_append(lib, k_new, v_new, cu, total_q, n_seqs, kv_heads, head_dim, kp, vp, pool_type, ks, vs, table, lens, lens_out, n_pages, page_size, max_pages, plan,
               plan_ints, loc=0, stream=None):
    st = lib.brn_kv_cache_append_varlen(_ptr(k_new), _ptr(v_new), _ptr(cu), total_q, n_seqs, kv_heads, head_dim, _ptr(kp), _ptr(vp), pool_type, _ptr(ks), _ptr(vs),
                                        _ptr(table), _ptr(lens), _ptr(lens_out), n_pages, page_size, max_pages, _ptr(plan), plan_ints, loc, 0, stream)
    return st, (lib.brn_last_error() or b"").decode()


@functools.lru_cache(maxsize=None)
def _buffers():
    """q, kp, vp, y, lse, ws (floats), table, lens, cu, plan, lens_out (ints), ks, vs"""
    return (tuple(np.zeros(2 * 2 * 32 * 256, np.float32) for _ in range(6)) +
            (np.zeros(2 * 13, np.int32), np.full(2, 200, np.int32), np.array([0, 16, 32], np.int32), np.zeros(16, np.int32), np.zeros(2, np.int32)) +
            (np.ones(1, np.float32), np.ones(1, np.float32)))


# the well-formed neighbour of every refused attention call: a pack of 32 tokens in 2 sequences, max_kv_len 200, heads 2, kv_heads 1,
# head_dim 32, a pool of 20 pages of 16 keys, 13 table entries per sequence, nkt 4, kv_splits 2 -> S 2, R 64, 2 * 64 * 33 = 4224 workspace
# floats, 2 * 3 = 6 plan ints
ATTEND_OK = (32, 2, 200, 2, 1, 32, 20, 16, 13, 0, 0.0, 2)
ATTEND_NAMES = ("total_q", "n_seqs", "max_kv_len", "heads", "kv_heads", "head_dim", "n_pages", "page_size", "max_pages", "causal", "scale", "kv_splits")


def attend_neighbour():
    q, kp, vp, y, lse, ws, table, lens, cu, plan, _, _, _ = _buffers()
    return (q, kp, vp, 0, None, None, table, lens, cu) + ATTEND_OK + (y, lse, ws, 4224, plan, 6)


def attend_refusals():
    """(name, arguments of raw_attend after lib, words the message must contain).  The refused calls read nothing."""
    q, kp, vp, y, lse, ws, table, lens, cu, plan, _, ks, vs = _buffers()
    assert q.ctypes.data % 16 == 0 and table.ctypes.data % 4 == 0
    head = (q, kp, vp, 0, None, None, table, lens, cu)
    tail = (y, lse, ws, 4224, plan, 6)

    def sub(**kw):
        assert set(kw) <= set(ATTEND_NAMES)
        return tuple(kw.get(n, d) for n, d in zip(ATTEND_NAMES, ATTEND_OK))

    def ins(**kw):
        names = ("q", "kp", "vp", "pool_type", "ks", "vs", "table", "lens", "cu")
        assert set(kw) <= set(names)
        return tuple(kw.get(n, d) for n, d in zip(names, head))

    ok = ATTEND_OK
    return [
        ("null q", ins(q=None) + ok + tail, "null q, k_pages, v_pages or y"),
        ("null cu_seqlens_q", ins(cu=None) + ok + tail, "null block_table, kv_lens or cu_seqlens_q"),
        ("null kv_lens", ins(lens=None) + ok + tail, "null block_table, kv_lens or cu_seqlens_q"),
        ("pool_type 4", ins(pool_type=4) + ok + tail, "pool_type must be 0 = f32, 1 = bf16, 2 = f16 or 3 = e4m3"),
        ("pool_type -1", ins(pool_type=-1) + ok + tail, "pool_type must be 0 = f32, 1 = bf16, 2 = f16 or 3 = e4m3"),
        ("k_scale with an f32 pool", ins(ks=ks) + ok + tail, "k_scale and v_scale must be NULL unless pool_type is 3 = e4m3"),
        ("v_scale with a bf16 pool", ins(pool_type=1, vs=vs) + ok + tail, "k_scale and v_scale must be NULL unless pool_type is 3 = e4m3"),
        ("n_seqs 0", head + sub(n_seqs=0) + tail, "1 <= n_seqs <= 65536"),
        ("n_seqs 65537", head + sub(n_seqs=65537) + tail, "1 <= n_seqs <= 65536"),
        ("total_q 0", head + sub(total_q=0) + tail, "total_q >= 1"),
        ("2^31 packed rows", head + sub(total_q=2 ** 20, heads=2 ** 11) + tail, "G * total_q < 2^31"),
        ("2^31 workgroups", head + sub(total_q=2 ** 24, heads=64, kv_heads=64, max_kv_len=65536, max_pages=4096, kv_splits=1024) + tail, "T_max * kv_heads * S < 2^31"),
        ("head_dim 48", head + sub(head_dim=48) + tail, "head_dim must be 32, 64 or 128"),
        ("heads 0", head + sub(heads=0) + tail, "heads >= 1"),
        ("kv_heads 0", head + sub(kv_heads=0) + tail, "1 <= kv_heads <= heads"),
        ("heads % kv_heads != 0", head + sub(heads=6, kv_heads=4) + tail, "heads % kv_heads == 0"),
        ("page_size 48", head + sub(page_size=48) + tail, "page_size must be 16, 32, 64, 128 or 256"),
        ("n_pages 0", head + sub(n_pages=0) + tail, "n_pages >= 1, max_pages >= 1"),
        ("2^31 keys in the pool", head + sub(n_pages=2 ** 23, page_size=256) + tail, "n_pages * page_size < 2^31"),
        ("max_kv_len 0", head + sub(max_kv_len=0) + tail, "1 <= max_kv_len <= 65536"),
        ("max_kv_len 65537", head + sub(max_kv_len=65537, max_pages=5000) + tail, "1 <= max_kv_len <= 65536"),
        ("max_kv_len past the table", head + sub(max_kv_len=209) + tail, "1 <= max_kv_len <= min(65536, max_pages * page_size)"),
        ("kv_splits -1", head + sub(kv_splits=-1) + tail, "0 <= kv_splits <= 1024"),
        ("kv_splits 1025", head + sub(kv_splits=1025) + tail, "0 <= kv_splits <= 1024"),
        ("causal 2", head + sub(causal=2) + tail, "causal must be 0 or 1"),
        ("NaN scale", head + sub(scale=float("nan")) + tail, "scale must be finite and >= 0"),
        ("workspace NULL, S 2", head + ok + (y, lse, None, 0, plan, 6), "4224 floats"),
        ("workspace too small", head + ok + (y, lse, ws, 4223, plan, 6), "4224 floats"),
        ("plan_workspace NULL", head + ok + (y, lse, ws, 4224, None, 6), "6 ints"),
        ("plan_workspace too small", head + ok + (y, lse, ws, 4224, plan, 5), "6 ints"),
        ("plan_workspace misaligned", head + ok + (y, lse, ws, 4224, plan.ctypes.data + 2, 6), "plan_workspace must be 4-byte aligned"),
        ("lse is y", head + ok + (y, y, ws, 4224, plan, 6), "overlap"),
        ("y is q", head + ok + (q, lse, ws, 4224, plan, 6), "overlap"),
        ("lse is k_pages", head + ok + (y, kp, ws, 4224, plan, 6), "overlap"),
        ("workspace is cu_seqlens_q", head + ok + (y, lse, cu.ctypes.data, 4224, plan, 6), "overlap"),
        ("workspace overlaps the end of v_pages", head + ok + (y, lse, vp.ctypes.data + 4 * (20 * 16 * 32 - 4), 4224, plan, 6), "overlap"),
        ("plan_workspace is kv_lens", head + ok + (y, lse, ws, 4224, lens.ctypes.data, 6), "overlap"),
        ("plan_workspace inside y", head + ok + (y, lse, ws, 4224, y.ctypes.data + 64, 6), "overlap"),
        ("misaligned device lse", head + ok + (y, lse.ctypes.data + 4096 + 4, ws, 4224, plan, 6, 1), "16-byte aligned"),
        ("misaligned device v_pages", ins(vp=q.ctypes.data + 4096 + 4) + ok + tail + (1,), "16-byte aligned"),
        ("misaligned cu_seqlens_q", ins(cu=cu.ctypes.data + 2) + ok + tail + (1,), "4-byte aligned"),
    ]


def attend_byte_counted_neighbours():
    """narrow pools are counted in bytes: an output just behind the last BYTE of a bf16 / e4m3 pool is accepted (it reaches the device check)"""
    q, kp, vp, y, lse, ws, table, lens, cu, plan, _, ks, vs = _buffers()
    n = 20 * 16 * 32
    return [("lse behind a bf16 pool", (q, kp, vp, 1, None, None, table, lens, cu) + ATTEND_OK + (y, kp.ctypes.data + 2 * n, ws, 4224, plan, 6)),
            ("lse behind an e4m3 pool", (q, kp, vp, 3, ks, vs, table, lens, cu) + ATTEND_OK + (y, kp.ctypes.data + n, ws, 4224, plan, 6))]


# the well-formed neighbour of every refused append: 32 tokens in 2 sequences, kv_heads 1, head_dim 32, 20 pages of 16 keys, 13 entries each
APPEND_OK_TAIL = (20, 16, 13)


def append_neighbour():
    q, kp, vp, kn, vn, _, table, lens, cu, plan, lens_out, _, _ = _buffers()
    return (kn, vn, cu, 32, 2, 1, 32, kp, vp, 0, None, None, table, lens, lens_out) + APPEND_OK_TAIL + (plan, 6)


def append_refusals():
    q, kp, vp, kn, vn, _, table, lens, cu, plan, lens_out, ks, vs = _buffers()

    def call(**kw):
        names = ("k_new", "v_new", "cu", "total_q", "n_seqs", "kv_heads", "head_dim", "kp", "vp", "pool_type", "ks", "vs", "table", "lens", "lens_out", "n_pages",
                 "page_size", "max_pages", "plan", "plan_ints", "loc")
        assert set(kw) <= set(names)
        return tuple(kw.get(n, d) for n, d in zip(names, append_neighbour() + (0,)))

    return [
        ("null v_new", call(v_new=None), "null k_new, v_new, k_pages or v_pages"),
        ("null cu_seqlens_q", call(cu=None), "null block_table, kv_lens or cu_seqlens_q"),
        ("pool_type 4", call(pool_type=4), "pool_type must be 0 = f32, 1 = bf16, 2 = f16 or 3 = e4m3"),
        ("scales with an f16 pool", call(pool_type=2, ks=ks, vs=vs), "k_scale and v_scale must be NULL unless pool_type is 3 = e4m3"),
        ("head_dim 40", call(head_dim=40), "head_dim must be 32, 64 or 128"),
        ("kv_heads 0", call(kv_heads=0), "kv_heads >= 1"),
        ("n_seqs 0", call(n_seqs=0), "1 <= n_seqs <= 65536"),
        ("n_seqs 65537", call(n_seqs=65537), "1 <= n_seqs <= 65536"),
        ("total_q 0", call(total_q=0), "total_q >= 1"),
        ("page_size 24", call(page_size=24), "page_size must be 16, 32, 64, 128 or 256"),
        ("max_pages 0", call(max_pages=0), "n_pages >= 1, max_pages >= 1"),
        ("2^31 positions in the table", call(max_pages=2 ** 27), "max_pages * page_size < 2^31"),
        ("plan_workspace NULL", call(plan=None), "6 ints"),
        ("plan_workspace too small", call(plan_ints=5), "6 ints"),
        ("plan_workspace misaligned", call(plan=plan.ctypes.data + 1), "plan_workspace must be 4-byte aligned"),
        ("k_new inside the pool", call(k_new=kp.ctypes.data + 64), "k_new must not overlap the pool"),
        ("cu_seqlens_q inside the pool", call(cu=vp.ctypes.data + 128), "cu_seqlens_q must not overlap the pool"),
        ("k_pages is v_pages", call(vp=kp), "k_pages and v_pages must not overlap"),
        ("plan_workspace inside the pool", call(plan=kp.ctypes.data + 256), "plan_workspace must not overlap the pool"),
        ("plan_workspace is cu_seqlens_q", call(plan=cu.ctypes.data), "plan_workspace must not overlap cu_seqlens_q"),
        ("kv_lens_out overlaps the table", call(lens_out=table.ctypes.data + 8), "kv_lens_out must not overlap block_table"),
        ("kv_lens_out half over kv_lens", call(lens_out=lens.ctypes.data + 4), "kv_lens_out must not overlap kv_lens"),
        ("kv_lens_out is plan_workspace", call(lens_out=plan.ctypes.data), "plan_workspace must not overlap kv_lens_out"),
        ("misaligned device k_new", call(k_new=kn.ctypes.data + 4, loc=1), "16-byte aligned"),
        ("misaligned kv_lens_out", call(lens_out=lens_out.ctypes.data + 2, loc=1), "4-byte aligned"),
    ]
