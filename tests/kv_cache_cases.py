"""What tests/test_kv_cache_cpu.py, tests/test_kv_cache_gpu.py and tests/test_flash_attention_paged_kv_gpu.py share: the 16-bit storage
of a K / V pool (bit patterns, the suite's own rounding), the cases of brn_kv_cache_append with their deterministic inputs, the numpy
statement of the append rule, raw ctypes calls of the two entries and their refusal lists.

Rounding is flash_attention_cases.round_s16 (torch, round to nearest even); a bf16 bit pattern is its fp32 result shifted right by 16.
The pools of the attention tests are flash_attention_paged_cases.build_pool's, imported and not edited."""
import functools

import numpy as np

import flash_attention_paged_cases as PG
from flash_attention_paged_cases import round_s16

KV_TYPES = ("f32", "bf16", "f16")
KV_CODE = {"f32": 0, "bf16": 1, "f16": 2}
BITS = {"f32": np.uint32, "bf16": np.uint16, "f16": np.uint16}
# a NaN payload no conversion produces: what a row the rule does not name must still hold
SENTINEL = {"f32": 0x7FC00AB5, "bf16": 0x7FC5, "f16": 0x7E05}
# (compute mode, pool type) pairs the attention entry accepts and the tests run
PAIRS = (("bf16", "bf16"), ("f16", "f16"), ("f32", "bf16"), ("f32", "f16"))


def to_bits(a, kv):
    """fp32 values -> the bit patterns a pool of type kv stores for them (uint32 / uint16), round to nearest even"""
    a = np.ascontiguousarray(a, np.float32)
    if kv == "f32":
        return a.view(np.uint32).copy()
    r = round_s16(a, kv)
    if kv == "bf16":
        return (r.astype(np.float32).view(np.uint32) >> 16).astype(np.uint16)
    return r.astype(np.float16).view(np.uint16).copy()


def widen(bits, kv):
    """stored bit patterns -> the fp32 values they stand for, exactly"""
    bits = np.ascontiguousarray(bits)
    if kv == "f32":
        return bits.view(np.float32).copy()
    if kv == "bf16":
        return (bits.astype(np.uint32) << 16).view(np.float32)
    return bits.view(np.float16).astype(np.float32)


for _kv in KV_TYPES:
    assert np.isnan(widen(np.array([SENTINEL[_kv]], BITS[_kv]), _kv)).all()

# values every k_new / v_new holds among the ordinary ones: exact ties of both 16-bit types (to even, down and up), +-0, a value that is
# subnormal in f16, half the smallest f16 subnormal (a tie with 0), values past the f16 range, the largest finite f16 and its tie with
# inf, a NaN
SPECIALS = np.array([1 + 2.0 ** -8, 1 + 3 * 2.0 ** -8, -(1 + 2.0 ** -8), 1 + 2.0 ** -11, 1 + 3 * 2.0 ** -11, -(1 + 3 * 2.0 ** -11), 0.0, -0.0, 1e-5, -3e-6,
                     2.0 ** -25, 70000.0, -70000.0, 65504.0, 65520.0, np.nan, 3.0e38], np.float32)
assert to_bits(SPECIALS[:3], "bf16").tolist() == [0x3F80, 0x3F82, 0xBF80] and to_bits(SPECIALS[3:6], "f16").tolist() == [0x3C00, 0x3C02, 0xBC02]
assert to_bits(SPECIALS[6:8], "f16").tolist() == [0x0000, 0x8000] and 0 < to_bits(SPECIALS[8:9], "f16")[0] < 0x0400 and to_bits(SPECIALS[10:11], "f16")[0] == 0
assert to_bits(SPECIALS[11:15], "f16").tolist() == [0x7C00, 0xFC00, 0x7BFF, 0x7C00] and np.isnan(widen(to_bits(SPECIALS[15:16], "bf16"), "bf16")).all()


# ---- the cases of the append: name -> batch, seq_new, page, max_pages, kv_heads, lens, layouts, bad = {(b, slot): entry} ----
def _c(batch, seq_new, page, max_pages, kv_heads, lens, layouts=("bshd",), bad=None):
    return dict(batch=batch, seq_new=seq_new, page=page, max_pages=max_pages, kv_heads=kv_heads, lens=tuple(lens), layouts=layouts, bad=bad or {})


SPARE = 3                 # pages of the pool no table entry names
BAD_LOW, BAD_HIGH = -3, 7  # the out-of-range entries: -3, n_pages + 7
MARGIN = 8                 # sentinel pages each side of the pool in the clamped-pages case: more than any page number written
APPEND_CASES = {
    "page_edges": _c(3, 1, 16, 3, 2, (15, 16, 0)),                                  # last row of a page, first row of the next, an empty sequence
    "straddle": _c(1, 5, 16, 3, 2, (30,)),                                          # a step across a page boundary
    "three_pages": _c(2, 40, 16, 4, 3, (7, 0), layouts=("bshd", "bhsd")),           # three pages in one call, odd head count, both layouts
    "dropped": _c(1, 5, 16, 3, 2, (46,)),                                           # positions 48 .. 50 dropped, kv_lens_out 48
    "clamped_lens": _c(2, 3, 16, 3, 1, (-5, 1000)),                                 # -5 is 0; 1000 is cap = 48: every row dropped
    "clamped_pages": _c(2, 20, 16, 3, 2, (10, 0), bad={(0, 1): BAD_LOW, (1, 0): BAD_HIGH}),   # entries at written positions out of range
    "page256": _c(2, 1, 256, 2, 1, (255, 256)),                                     # the largest page: its last row, the next page's first
}
HEAD_DIMS = (32, 128)


def cap_of(c):
    return c["max_pages"] * c["page"]


def clamp_len(length, cap):
    return min(max(int(length), 0), cap)


def written_positions(c, b):
    """the positions of sequence b the call writes (those below cap)"""
    L = clamp_len(c["lens"][b], cap_of(c))
    return range(L, min(L + c["seq_new"], cap_of(c)))


def dropped_tokens(c):
    return sum(c["seq_new"] - len(written_positions(c, b)) for b in range(c["batch"]))


def n_pages_of(c):
    return c["batch"] * c["max_pages"] + SPARE


@functools.lru_cache(maxsize=None)
def table_of(name):
    """block_table [batch, max_pages] int32 (read-only): distinct pages for every (sequence, slot), a seeded permutation of the pool
    without its first and last page (what an out-of-range entry is clamped to, so that a clamped write shares its page with no other),
    with the case's out-of-range entries written over it"""
    c = APPEND_CASES[name]
    rng = np.random.default_rng(4242 + len(name) + c["page"])
    t = rng.permutation(np.arange(1, n_pages_of(c) - 1))[:c["batch"] * c["max_pages"]].reshape(c["batch"], c["max_pages"]).astype(np.int32)
    for (b, slot), v in c["bad"].items():
        t[b, slot] = v if v < 0 else n_pages_of(c) + v
    t.setflags(write=False)
    return t


@functools.lru_cache(maxsize=None)
def new_tokens(name, hd):
    """k_new, v_new [batch, seq_new, kv_heads, hd] fp32 (BSHD, read-only): standard normal x 3 with SPECIALS written over the start of k
    and (reversed) over the end of v"""
    c = APPEND_CASES[name]
    rng = np.random.default_rng(77 + hd + len(name) * 13 + c["seq_new"])
    k, v = (rng.standard_normal((c["batch"], c["seq_new"], c["kv_heads"], hd)).astype(np.float32) * 3 for _ in range(2))
    n = min(SPECIALS.size, k[0, 0].size)
    k.reshape(c["batch"], -1)[:, :n] = SPECIALS[:n]
    v.reshape(c["batch"], -1)[:, -n:] = SPECIALS[:n][::-1]
    for a in (k, v):
        a.setflags(write=False)
    return k, v


def sentinel_pool(c, hd, kv, pages=None):
    """[pages or n_pages, page, kv_heads, hd] of the type's sentinel bit pattern"""
    return np.full((pages or n_pages_of(c), c["page"], c["kv_heads"], hd), SENTINEL[kv], BITS[kv])


def append_rule(new_bits, pool_bits, table, lens, seq_new=None):
    """THE RULE, in numpy.  new_bits [batch, seq_new, kv_heads, hd] (BSHD) holds what is to be stored (bit patterns, or any array of the
    pool's dtype); returns (the pool after the append, kv_lens_out): token t of batch entry b goes to row (L_b + t) % page of page
    clamp(table[b][(L_b + t) // page], 0, n_pages - 1), L_b = min(max(lens[b], 0), cap), cap = max_pages * page; a position >= cap is
    dropped and reads no table entry; kv_lens_out[b] = min(L_b + seq_new, cap)"""
    n_pages, page = pool_bits.shape[:2]
    batch, max_pages = table.shape
    seq_new = new_bits.shape[1] if seq_new is None else seq_new
    cap = max_pages * page
    out = pool_bits.copy()
    lens_out = np.empty(batch, np.int32)
    for b in range(batch):
        L = clamp_len(lens[b], cap)
        for t in range(seq_new):
            pos = L + t
            if pos >= cap:
                continue
            out[min(max(int(table[b, pos // page]), 0), n_pages - 1), pos % page] = new_bits[b, t]
        lens_out[b] = min(L + seq_new, cap)
    return out, lens_out


def expected_append(name, hd, kv):
    """(k pool bits, v pool bits, kv_lens_out, k NaN mask, v NaN mask) of the case on sentinel pools; the masks mark the elements whose
    new value is a NaN (the stored pattern of a NaN is checked as "is NaN")"""
    c = APPEND_CASES[name]
    k, v = new_tokens(name, hd)
    table, lens = table_of(name), np.asarray(c["lens"], np.int32)
    kb, lo = append_rule(to_bits(k, kv), sentinel_pool(c, hd, kv), table, lens)
    vb, _ = append_rule(to_bits(v, kv), sentinel_pool(c, hd, kv), table, lens)
    none = np.zeros(kb.shape, bool)
    return kb, vb, lo, append_rule(np.isnan(k), none, table, lens)[0], append_rule(np.isnan(v), none, table, lens)[0]


# coverage that must not vanish silently when a case is edited
_C = APPEND_CASES
assert [clamp_len(L, cap_of(_C["page_edges"])) % 16 for L in _C["page_edges"]["lens"]] == [15, 0, 0] and 0 in _C["page_edges"]["lens"]
assert {p // 16 for p in written_positions(_C["straddle"], 0)} == {1, 2} and dropped_tokens(_C["straddle"]) == 0
assert len({p // 16 for p in written_positions(_C["three_pages"], 0)}) == 3 and _C["three_pages"]["kv_heads"] % 2 == 1 and len(_C["three_pages"]["layouts"]) == 2
assert list(written_positions(_C["dropped"], 0)) == [46, 47] and dropped_tokens(_C["dropped"]) == 3
assert [len(written_positions(_C["clamped_lens"], b)) for b in range(2)] == [3, 0] and min(_C["clamped_lens"]["lens"]) < 0 and max(_C["clamped_lens"]["lens"]) > cap_of(_C["clamped_lens"])
for (_b, _slot), _v in _C["clamped_pages"]["bad"].items():
    assert any(p // 16 == _slot for p in written_positions(_C["clamped_pages"], _b)), "an out-of-range entry must sit at a written position"
assert {v for v in _C["clamped_pages"]["bad"].values()} == {BAD_LOW, BAD_HIGH} and MARGIN > max(-BAD_LOW, BAD_HIGH)
assert _C["page256"]["page"] == 256 and [p % 256 for b in range(2) for p in written_positions(_C["page256"], b)] == [255, 0]
assert all(not c["bad"] or n == "clamped_pages" for n, c in _C.items())
for _n, _c_ in _C.items():
    _t = table_of(_n)
    _ok = [int(_t[b, s]) for b in range(_c_["batch"]) for s in range(_c_["max_pages"]) if (b, s) not in _c_["bad"]]
    assert len(set(_ok)) == len(_ok) and 0 < min(_ok) and max(_ok) < n_pages_of(_c_) - 1, "no two sequences share a page, none names the first or the last"


# ---- raw calls ----
def _ptr(a):
    return a if a is None or isinstance(a, int) else a.ctypes.data


def raw_attend(lib, q, kp, vp, kv_type, table, lens, batch, seq_q, max_kv_len, heads, kv_heads, head_dim, n_pages, page_size, max_pages, layout, causal, scale,
               kv_splits, y, lse, ws, ws_floats, loc=0, stream=None):
    """brn_flash_attention_paged_kv_forward with the integers exactly as given; the pointers: numpy arrays, integers taken as addresses, or None"""
    st = lib.brn_flash_attention_paged_kv_forward(_ptr(q), _ptr(kp), _ptr(vp), kv_type, _ptr(table), _ptr(lens), batch, seq_q, max_kv_len, heads, kv_heads, head_dim,
                                                  n_pages, page_size, max_pages, layout, causal, scale, kv_splits, _ptr(y), _ptr(lse), _ptr(ws), ws_floats, loc, 0, stream)
    return st, (lib.brn_last_error() or b"").decode()


def raw_append(lib, k_new, v_new, batch, seq_new, kv_heads, head_dim, layout, kp, vp, kv_type, table, lens, lens_out, n_pages, page_size, max_pages, loc=0, stream=None):
    """brn_kv_cache_append with the integers exactly as given"""
    st = lib.brn_kv_cache_append(_ptr(k_new), _ptr(v_new), batch, seq_new, kv_heads, head_dim, layout, _ptr(kp), _ptr(vp), kv_type, _ptr(table), _ptr(lens), _ptr(lens_out),
                                 n_pages, page_size, max_pages, loc, 0, stream)
    return st, (lib.brn_last_error() or b"").decode()


def attend_refusals():
    """(name, arguments of raw_attend after lib, words the message must contain, compute mode).  Every refusal of
    flash_attention_paged_cases.refusals() with kv_type BRN_KV_F32 inserted (the inherited limits, under the new prefix), then the new
    limits.  The refused calls read nothing."""
    out = [(name, args[:3] + (0,) + args[3:], word, "f32") for name, args, word in PG.refusals()]
    q, kp, vp, y, lse, ws, table, lens = PG._refusal_buffers()
    ok = (2, 16, 200, 2, 1, 32, 20, 16, 13, 0, 0, 0.0, 2)
    tail = (y, lse, ws, 4224)
    pool_bytes = 2 * 20 * 16 * 32                     # the pool of the well-formed call as bf16 / f16: 20 pages x 16 keys x 1 head x 32, 2 bytes each
    out += [
        ("kv_type 3", (q, kp, vp, 3, table, lens) + ok + tail, "kv_type must be 0 = f32, 1 = bf16 or 2 = f16", "f32"),
        ("kv_type -1", (q, kp, vp, -1, table, lens) + ok + tail, "kv_type must be 0 = f32, 1 = bf16 or 2 = f16", "f32"),
        ("a bf16 pool in mode f16", (q, kp, vp, 1, table, lens) + ok + tail, "kv_type bf16 cannot be read in compute mode f16", "f16"),
        ("an f16 pool in mode bf16", (q, kp, vp, 2, table, lens) + ok + tail, "kv_type f16 cannot be read in compute mode bf16", "bf16"),
        ("misaligned device bf16 k_pages", (q, kp.ctypes.data + 4096 + 2, vp, 1, table, lens) + ok + tail + (1,), "16-byte aligned", "bf16"),
        ("misaligned device f16 v_pages", (q, kp, vp.ctypes.data + 4096 + 8, 2, table, lens) + ok + tail + (1,), "16-byte aligned", "f32"),
        ("workspace overlaps the end of a bf16 v_pages (bytes)", (q, kp, vp, 1, table, lens) + ok + (y, lse, vp.ctypes.data + pool_bytes - 16, 4224), "overlap", "f32"),
        ("lse overlaps the end of an f16 k_pages (bytes)", (q, kp, vp, 2, table, lens) + ok + (y, kp.ctypes.data + pool_bytes - 4, ws, 4224), "overlap", "f16"),
    ]
    return out


def attend_byte_counted_neighbours():
    """calls the byte count must LET THROUGH: an output that starts where a 16-bit pool ends (inside where the same pool as fp32 would
    lie) -> (name, arguments, compute mode)"""
    q, kp, vp, y, lse, ws, table, lens = PG._refusal_buffers()
    ok = (2, 16, 200, 2, 1, 32, 20, 16, 13, 0, 0, 0.0, 2)
    pool_bytes = 2 * 20 * 16 * 32
    return [("workspace right behind a bf16 v_pages", (q, kp, vp, 1, table, lens) + ok + (y, lse, vp.ctypes.data + pool_bytes, 4224), "bf16"),
            ("lse right behind an f16 k_pages", (q, kp, vp, 2, table, lens) + ok + (y, kp.ctypes.data + pool_bytes, ws, 4224), "f32")]


@functools.lru_cache(maxsize=None)
def _append_buffers():
    # k_new, v_new: 2 x 4 x 1 x 32 floats used; pools: 20 x 16 x 1 x 32 elements used
    return tuple(np.zeros(20 * 16 * 32 + 64, np.float32) for _ in range(4)) + (np.zeros(2 * 13, np.int32), np.full(2, 5, np.int32), np.zeros(8, np.int32))


def append_refusals():
    """(name, arguments of raw_append after lib, words the message must contain).  The well-formed neighbour of every call is
    (k_new, v_new, 2, 4, 1, 32, 0, kp, vp, 1, table, lens, lens_out, 20, 16, 13): batch 2, seq_new 4, one K / V head of 32, BSHD, a bf16
    pool of 20 pages of 16 keys, 13 table entries per sequence.  The refused calls read nothing."""
    kn, vn, kp, vp, table, lens, lo = _append_buffers()
    assert kn.ctypes.data % 16 == 0 and kp.ctypes.data % 16 == 0
    ok = dict(batch=2, seq_new=4, kv_heads=1, head_dim=32, layout=0, kv_type=1, n_pages=20, page_size=16, max_pages=13)

    def call(k_new=kn, v_new=vn, k_pages=kp, v_pages=vp, block_table=table, kv_lens=lens, kv_lens_out=lo, loc=0, **kw):
        assert set(kw) <= set(ok)
        a = dict(ok, **kw)
        return (k_new, v_new, a["batch"], a["seq_new"], a["kv_heads"], a["head_dim"], a["layout"], k_pages, v_pages, a["kv_type"], block_table, kv_lens, kv_lens_out,
                a["n_pages"], a["page_size"], a["max_pages"], loc)

    new_bytes, pool16 = 4 * 2 * 4 * 32, 2 * 20 * 16 * 32
    return [
        ("null k_new", call(k_new=None), "null k_new, v_new, k_pages or v_pages"),
        ("null v_pages", call(v_pages=None), "null k_new, v_new, k_pages or v_pages"),
        ("null block_table", call(block_table=None), "null block_table or kv_lens"),
        ("null kv_lens", call(kv_lens=None), "null block_table or kv_lens"),
        ("kv_type 3", call(kv_type=3), "kv_type must be 0 = f32, 1 = bf16 or 2 = f16"),
        ("kv_type -1", call(kv_type=-1), "kv_type must be 0 = f32, 1 = bf16 or 2 = f16"),
        ("head_dim 48", call(head_dim=48), "head_dim must be 32, 64 or 128"),
        ("batch 0", call(batch=0), "batch >= 1, kv_heads >= 1"),
        ("kv_heads 0", call(kv_heads=0), "batch >= 1, kv_heads >= 1"),
        ("seq_new 0", call(seq_new=0), "1 <= seq_new <= 65536"),
        ("seq_new 65537", call(seq_new=65537), "1 <= seq_new <= 65536"),
        ("layout 2", call(layout=2), "layout must be 0"),
        ("page_size 48", call(page_size=48), "page_size must be 16, 32, 64, 128 or 256"),
        ("page_size 8", call(page_size=8), "page_size must be 16, 32, 64, 128 or 256"),
        ("page_size 512", call(page_size=512), "page_size must be 16, 32, 64, 128 or 256"),
        ("n_pages 0", call(n_pages=0), "n_pages >= 1, max_pages >= 1"),
        ("max_pages 0", call(max_pages=0), "n_pages >= 1, max_pages >= 1"),
        ("2^31 keys in the pool", call(n_pages=2 ** 23, page_size=256), "n_pages * page_size < 2^31"),
        ("2^31 keys in a table row", call(max_pages=2 ** 23, page_size=256), "max_pages * page_size < 2^31"),
        ("2^31 threads per batch entry", call(seq_new=65536, kv_heads=4096, head_dim=128), "seq_new * kv_heads * head_dim / 8 < 2^31"),
        ("k_new inside k_pages", call(k_new=kp.ctypes.data + 64), "k_new must not overlap the pool"),
        ("v_new overlaps the end of v_pages (bytes)", call(v_new=vp.ctypes.data + pool16 - 16), "v_new must not overlap the pool"),
        ("the table inside k_pages", call(block_table=kp.ctypes.data + 128), "block_table must not overlap the pool"),
        ("kv_lens inside v_pages", call(kv_lens=vp.ctypes.data), "kv_lens must not overlap the pool"),
        ("v_pages is k_pages", call(v_pages=kp), "k_pages and v_pages must not overlap"),
        ("v_pages overlaps the end of k_pages (bytes)", call(v_pages=kp.ctypes.data + pool16 - 32), "k_pages and v_pages must not overlap"),
        ("kv_lens_out half over kv_lens", call(kv_lens_out=lens.ctypes.data + 4), "kv_lens_out must not overlap kv_lens"),
        ("kv_lens_out inside the table", call(kv_lens_out=table.ctypes.data + 8), "kv_lens_out must not overlap block_table"),
        ("kv_lens_out inside k_new", call(kv_lens_out=kn.ctypes.data + new_bytes - 4), "kv_lens_out must not overlap k_new"),
        ("kv_lens_out inside k_pages", call(kv_lens_out=kp.ctypes.data + 16), "kv_lens_out must not overlap the pool"),
        ("misaligned device k_new", call(k_new=kn.ctypes.data + 4, loc=1), "16-byte aligned"),
        ("misaligned device 16-bit v_pages", call(v_pages=vp.ctypes.data + 2, loc=1), "16-byte aligned"),
        ("misaligned device kv_lens_out", call(kv_lens_out=lo.ctypes.data + 2, loc=1), "4-byte aligned"),
        ("misaligned device block_table", call(block_table=table.ctypes.data + 2, loc=1), "4-byte aligned"),
    ]


def append_byte_counted_neighbours():
    """calls the byte count must let through: v_new / kv_lens_out right behind a 16-bit pool -> (name, arguments)"""
    kn, vn, kp, vp, table, lens, lo = _append_buffers()
    pool16 = 2 * 20 * 16 * 32
    base = (2, 4, 1, 32, 0)
    return [("v_new right behind a bf16 v_pages", (kn, vp.ctypes.data + pool16) + base + (kp, vp, 1, table, lens, lo, 20, 16, 13)),
            ("kv_lens_out right behind an f16 k_pages", (kn, vn) + base + (kp, vp, 2, table, lens, kp.ctypes.data + pool16, 20, 16, 13)),
            ("kv_lens_out is kv_lens", (kn, vn) + base + (kp, vp, 1, table, lens, lens, 20, 16, 13))]
