"""What tests/test_rope_cpu.py and tests/test_rope_gpu.py share: the numpy statement of the rotary rule (rope_rule), its float64 form,
the tables, the cases with their deterministic inputs, raw ctypes calls of the three entries and their refusal lists.

THE RULE is written with np.float32 arrays: a product of two float32 arrays is one rounded float32 product and a sum one rounded sum, so
the rule is unfused by construction.  The tokens are kv_cache_cases.new_tokens (KC.SPECIALS among them: +-0, subnormals of f16, 70000, a
NaN); the append cases, pools and the append rule are kv_cache_cases', the fp8 store kv_fp8_cases'; both imported and not edited."""
import functools

import numpy as np

import kv_cache_cases as KC

STYLES = ("half", "interleaved")
STYLE_CODE = {"half": 0, "interleaved": 1}
HEAD_DIMS = (32, 64, 128)
N_POS, THETA = 40, 10000.0        # a small table: the 40-token case at kv_lens 7 and every past-the-table position set run past it
NAN_PAYLOAD = 0x7FC01234          # a NaN the tail must carry unchanged


def rot_dims(hd):
    return tuple(sorted({16, hd // 2, hd}))


COMBOS = [(style, hd, rd) for style in STYLES for hd in HEAD_DIMS for rd in rot_dims(hd)]
COMBO_IDS = [f"{s}-d{hd}-r{rd}" for s, hd, rd in COMBOS]


@functools.lru_cache(maxsize=None)
def table(rot_dim, n_pos=N_POS, theta=THETA):
    """(cos, sin) [n_pos, rot_dim / 2] fp32 (read-only): angles p * theta^(-2 i / rot_dim) in float64, rounded once"""
    ang = np.arange(n_pos, dtype=np.float64)[:, None] * theta ** (-np.arange(0, rot_dim, 2, dtype=np.float64) / rot_dim)[None, :]
    cs, sn = np.cos(ang).astype(np.float32), np.sin(ang).astype(np.float32)
    for a in (cs, sn):
        a.setflags(write=False)
    return cs, sn


def table_rows(positions, batch, seq, n_pos):
    """[batch, seq] table rows: p = min(max(positions[b], 0) + t, n_pos - 1), in Python integers (no int32 overflow); None = all 0"""
    pos = [0] * batch if positions is None else [max(int(v), 0) for v in positions]
    return np.array([[min(P + t, n_pos - 1) for t in range(seq)] for P in pos], np.int64)


def pair_index(rot_dim, style):
    """(index of a, index of b) of pair i = 0 .. rot_dim / 2"""
    i = np.arange(rot_dim // 2)
    return (i, i + rot_dim // 2) if style == "half" else (2 * i, 2 * i + 1)


def rope_rule(x, cos, sin, rows, style):
    """THE RULE.  x [batch, seq, heads, head_dim] fp32 (BSHD), rows [batch, seq] table rows -> the rotated array: for pair (a, b) of a row
    at table row p, a' = fl(fl(a c) - fl(b s)), b' = fl(fl(b c) + fl(a s)) with c = cos[p][i], s = sin[p][i]; d >= rot_dim keeps its bits"""
    x = np.ascontiguousarray(x, np.float32)
    cos, sin = np.asarray(cos), np.asarray(sin)
    assert cos.dtype == np.float32 and sin.dtype == np.float32
    ia, ib = pair_index(2 * cos.shape[1], style)
    c, s = cos[rows][:, :, None, :], sin[rows][:, :, None, :]
    a, b = x[..., ia], x[..., ib]
    out = x.copy()
    with np.errstate(invalid="ignore", over="ignore", under="ignore"):
        ac, bs, bc, as_ = a * c, b * s, b * c, a * s
        assert ac.dtype == np.float32
        out[..., ia] = ac - bs
        out[..., ib] = bc + as_
    return out


def rope_exact(x, cos, sin, rows, style):
    """the same rotation in float64 on the fp32 table -> (a', b', |a c| + |b s|, |b c| + |a s|) per pair, [batch, seq, heads, rot_dim / 2]"""
    x = np.asarray(x, np.float64)
    ia, ib = pair_index(2 * cos.shape[1], style)
    c, s = np.asarray(cos, np.float64)[rows][:, :, None, :], np.asarray(sin, np.float64)[rows][:, :, None, :]
    a, b = x[..., ia], x[..., ib]
    return a * c - b * s, b * c + a * s, np.abs(a * c) + np.abs(b * s), np.abs(b * c) + np.abs(a * s)


def half_to_interleaved(x, rot_dim):
    """the permutation of a row's first rot_dim elements that maps HALF's pairing onto INTERLEAVED's: pair i moves from
    (i, i + rot_dim / 2) to (2i, 2i + 1)"""
    out = np.array(x)
    ia, ib = pair_index(rot_dim, "half")
    ja, jb = pair_index(rot_dim, "interleaved")
    out[..., ja] = x[..., ia]
    out[..., jb] = x[..., ib]
    return out


# ---- brn_rope_forward: (append case whose tokens are the input, layouts, position sets); "none" = NULL ----
BIG = 2 ** 31 - 1
FORWARD_CASES = {
    "page_edges": (("bshd",), ("none", (0, 5, 39))),                                        # seq 1: the last row of the table exactly
    "clamped_pages": (("bshd", "bhsd"), ("none", (3, 20), (-7, 5), (30, 1000), (BIG, -BIG - 1))),  # seq 20: in range (20 + 19 = 39), negative, past the table, int32 extremes
    "three_pages": (("bshd", "bhsd"), ("none", (7, 0))),                                    # seq 40, heads 3: the first sequence runs past the table
}
for _n, (_l, _p) in FORWARD_CASES.items():
    _c = KC.APPEND_CASES[_n]
    assert _c["batch"] <= 3 and _c["seq_new"] <= 40 and _c["kv_heads"] <= 3
    assert all(p == "none" or len(p) == _c["batch"] for p in _p)
assert max(FORWARD_CASES["clamped_pages"][1][1]) + KC.APPEND_CASES["clamped_pages"]["seq_new"] == N_POS
assert any(KC.clamp_len(L, KC.cap_of(c)) + c["seq_new"] > N_POS for c in KC.APPEND_CASES.values() for L in c["lens"]), "an append case runs past the table"


@functools.lru_cache(maxsize=None)
def forward_input(name, hd):
    """x [batch, seq, heads, hd] fp32 (BSHD, read-only): the k of KC.new_tokens with a payload NaN as the last element of the last row"""
    x = np.array(KC.new_tokens(name, hd)[0])
    x.reshape(-1).view(np.uint32)[-1] = NAN_PAYLOAD
    x.setflags(write=False)
    return x


def assert_bits(got, want, what=""):
    """fp32 arrays equal bit for bit, except that where the expected value is a NaN the other must be a NaN (which NaN a rotation makes
    of a NaN is not part of the rule)"""
    got, want = np.ascontiguousarray(got, np.float32), np.ascontiguousarray(want, np.float32)
    assert got.shape == want.shape, what
    nan = np.isnan(want)
    np.testing.assert_array_equal(got.view(np.uint32)[~nan], want.view(np.uint32)[~nan], err_msg=what)
    assert np.isnan(got[nan]).all(), f"{what}: a NaN of the rule is not a NaN"


def rotated_k(name, k, rot_dim, style, n_pos=N_POS):
    """the rule applied to the k_new of append case `name` at P_b = L_b, the append's clamped length"""
    c = KC.APPEND_CASES[name]
    cos, sin = table(rot_dim, n_pos)
    rows = table_rows([KC.clamp_len(L, KC.cap_of(c)) for L in c["lens"]], c["batch"], c["seq_new"], n_pos)
    return rope_rule(k, cos, sin, rows, style)


# ---- raw calls ----
_ptr = KC._ptr


def raw_rope(lib, x, batch, seq, heads, head_dim, layout, cos, sin, n_pos, rot_dim, style, positions, y, loc=0, stream=None):
    """brn_rope_forward with the integers exactly as given; the pointers: numpy arrays, integers taken as addresses, or None"""
    st = lib.brn_rope_forward(_ptr(x), batch, seq, heads, head_dim, layout, _ptr(cos), _ptr(sin), n_pos, rot_dim, style, _ptr(positions), _ptr(y), loc, 0, stream)
    return st, (lib.brn_last_error() or b"").decode()


def raw_append_rope(lib, k_new, v_new, batch, seq_new, kv_heads, head_dim, layout, cos, sin, n_pos, rot_dim, style, kp, vp, kv_type, table_, lens, lens_out, n_pages, page_size,
                    max_pages, loc=0, stream=None):
    st = lib.brn_kv_cache_append_rope(_ptr(k_new), _ptr(v_new), batch, seq_new, kv_heads, head_dim, layout, _ptr(cos), _ptr(sin), n_pos, rot_dim, style, _ptr(kp), _ptr(vp),
                                      kv_type, _ptr(table_), _ptr(lens), _ptr(lens_out), n_pages, page_size, max_pages, loc, 0, stream)
    return st, (lib.brn_last_error() or b"").decode()


def raw_append_rope_fp8(lib, k_new, v_new, batch, seq_new, kv_heads, head_dim, layout, cos, sin, n_pos, rot_dim, style, kp, vp, ks, vs, table_, lens, lens_out, n_pages,
                        page_size, max_pages, loc=0, stream=None):
    st = lib.brn_kv_cache_append_rope_fp8(_ptr(k_new), _ptr(v_new), batch, seq_new, kv_heads, head_dim, layout, _ptr(cos), _ptr(sin), n_pos, rot_dim, style, _ptr(kp), _ptr(vp),
                                          _ptr(ks), _ptr(vs), _ptr(table_), _ptr(lens), _ptr(lens_out), n_pages, page_size, max_pages, loc, 0, stream)
    return st, (lib.brn_last_error() or b"").decode()


@functools.lru_cache(maxsize=None)
def _rope_buffers():
    # x, y: 2 x 4 x 2 x 32 floats used; cos, sin: 40 x 16 floats used; positions: 2 ints.  Each float buffer is large enough for any
    # well-formed neighbour below that starts behind another array inside it
    return tuple(np.zeros(4096, np.float32) for _ in range(4)) + (np.zeros(8, np.int32),)


X_BYTES, TAB_BYTES = 4 * 2 * 4 * 2 * 32, 4 * 40 * 16


def rope_refusals():
    """(name, arguments of raw_rope after lib, words the message must contain).  The well-formed neighbour of every call is
    (x, 2, 4, 2, 32, 0, cos, sin, 40, 32, 0, positions, y): batch 2, seq 4, 2 heads of 32, BSHD, a table of 40 rows for rot_dim 32, HALF.
    The refused calls read nothing."""
    x, y, cs, sn, pos = _rope_buffers()
    assert all(a.ctypes.data % 16 == 0 for a in (x, y, cs, sn))
    ok = dict(batch=2, seq=4, heads=2, head_dim=32, layout=0, n_pos=40, rot_dim=32, style=0)

    def call(x=x, y=y, cos=cs, sin=sn, positions=pos, loc=0, **kw):
        assert set(kw) <= set(ok)
        a = dict(ok, **kw)
        return (x, a["batch"], a["seq"], a["heads"], a["head_dim"], a["layout"], cos, sin, a["n_pos"], a["rot_dim"], a["style"], positions, y, loc)

    return [
        ("null x", call(x=None), "null x or y"),
        ("null y", call(y=None), "null x or y"),
        ("null cos", call(cos=None), "null cos or sin"),
        ("null sin", call(sin=None), "null cos or sin"),
        ("head_dim 48", call(head_dim=48), "head_dim must be 32, 64 or 128"),
        ("rot_dim 0", call(rot_dim=0), "rot_dim must be a multiple of 16 with 16 <= rot_dim <= head_dim"),
        ("rot_dim 8", call(rot_dim=8), "rot_dim must be a multiple of 16 with 16 <= rot_dim <= head_dim"),
        ("rot_dim 24", call(rot_dim=24), "rot_dim must be a multiple of 16 with 16 <= rot_dim <= head_dim"),
        ("rot_dim 48 > head_dim", call(rot_dim=48), "rot_dim must be a multiple of 16 with 16 <= rot_dim <= head_dim"),
        ("style 2", call(style=2), "style must be 0 = HALF or 1 = INTERLEAVED"),
        ("style -1", call(style=-1), "style must be 0 = HALF or 1 = INTERLEAVED"),
        ("n_pos 0", call(n_pos=0), "1 <= n_pos <= 2^24"),
        ("n_pos 2^24 + 1", call(n_pos=2 ** 24 + 1), "1 <= n_pos <= 2^24"),
        ("batch 0", call(batch=0), "batch >= 1, heads >= 1"),
        ("heads 0", call(heads=0), "batch >= 1, heads >= 1"),
        ("seq 0", call(seq=0), "1 <= seq <= 65536"),
        ("seq 65537", call(seq=65537), "1 <= seq <= 65536"),
        ("layout 2", call(layout=2), "layout must be 0"),
        ("2^31 chunks", call(batch=2, seq=65536, heads=1024, head_dim=128), "batch * seq * heads * head_dim / 8 < 2^31"),
        ("y half over x", call(y=x.ctypes.data + 64), "y must be x itself"),
        ("y overlaps the end of x (bytes)", call(y=x.ctypes.data + X_BYTES - 16), "y must be x itself"),
        ("cos inside y", call(cos=y.ctypes.data + 32), "cos must not overlap y"),
        ("sin overlaps the end of y (bytes)", call(sin=y.ctypes.data + X_BYTES - 16), "sin must not overlap y"),
        ("y overlaps the end of cos (bytes)", call(y=cs.ctypes.data + TAB_BYTES - 16), "cos must not overlap y"),
        ("positions inside y", call(positions=y.ctypes.data + 128), "positions must not overlap y"),
        ("misaligned device x", call(x=x.ctypes.data + 4, loc=1), "16-byte aligned"),
        ("misaligned device y", call(y=y.ctypes.data + 8, loc=1), "16-byte aligned"),
        ("misaligned device cos", call(cos=cs.ctypes.data + 4, loc=1), "16-byte aligned"),
        ("misaligned device sin", call(sin=sn.ctypes.data + 8, loc=1), "16-byte aligned"),
        ("misaligned device positions", call(positions=pos.ctypes.data + 2, loc=1), "positions must be 4-byte aligned"),
    ]


def rope_neighbours():
    """calls every check must LET THROUGH -> (name, arguments): in place, NULL positions, buffers that start where another ends (all
    inside the 16 KiB buffers)"""
    x, y, cs, sn, pos = _rope_buffers()
    base = (2, 4, 2, 32, 0)
    return [("the well-formed call", (x,) + base + (cs, sn, 40, 32, 0, pos, y)),
            ("in place", (x,) + base + (cs, sn, 40, 32, 0, pos, x)),
            ("NULL positions, interleaved, rot_dim 16", (x,) + base + (cs, sn, 40, 16, 1, None, y)),
            ("y right behind x", (x,) + base + (cs, sn, 40, 32, 0, pos, x.ctypes.data + X_BYTES)),
            ("y right behind cos", (x,) + base + (cs, sn, 40, 32, 0, pos, cs.ctypes.data + TAB_BYTES)),
            ("a table of one row", (x,) + base + (cs, sn, 1, 32, 0, pos, y))]


def _with_table(args, cos, sin, n_pos=40, rot_dim=32, style=0):
    """the arguments of KC.raw_append / F8.raw_append after lib -> those of the rope entry: the table goes in behind layout"""
    return args[:7] + (cos, sin, n_pos, rot_dim, style) + args[7:]


def append_rope_refusals(fp8=False):
    """(name, arguments of raw_append_rope / raw_append_rope_fp8 after lib, words the message must contain): every refusal of the entry
    it extends with a well-formed table put in (the inherited limits, under the new prefix), then the table's limits.  Well-formed
    neighbour: batch 2, seq_new 4, one K / V head of 32, 20 pages of 16 keys, 13 table entries per sequence, 40 table rows, rot_dim 32"""
    import kv_fp8_cases as F8
    _, _, cs, sn, _ = _rope_buffers()
    out = [(name, _with_table(a, cs, sn), word) for name, a, word in (F8.append_refusals() if fp8 else KC.append_refusals())]
    kn, vn, kp, vp, tab, lens, lo = KC._append_buffers()
    pool = (kp, vp) + (F8._scale_buffers() if fp8 else (1,))
    pool_bytes = 20 * 16 * 32 * (1 if fp8 else 2)

    def call(cos=cs, sin=sn, n_pos=40, rot_dim=32, style=0, head_dim=32, kv_lens_out=lo, loc=0):
        return (kn, vn, 2, 4, 1, head_dim, 0, cos, sin, n_pos, rot_dim, style) + pool + (tab, lens, kv_lens_out, 20, 16, 13, loc)

    out += [
        ("null cos", call(cos=None), "null cos or sin"),
        ("null sin", call(sin=None), "null cos or sin"),
        ("rot_dim 8", call(rot_dim=8), "rot_dim must be a multiple of 16 with 16 <= rot_dim <= head_dim"),
        ("rot_dim 40", call(rot_dim=40, head_dim=64), "rot_dim must be a multiple of 16 with 16 <= rot_dim <= head_dim"),
        ("rot_dim 64 > head_dim", call(rot_dim=64), "rot_dim must be a multiple of 16 with 16 <= rot_dim <= head_dim"),
        ("style 3", call(style=3), "style must be 0 = HALF or 1 = INTERLEAVED"),
        ("n_pos 0", call(n_pos=0), "1 <= n_pos <= 2^24"),
        ("n_pos 2^24 + 1", call(n_pos=2 ** 24 + 1), "1 <= n_pos <= 2^24"),
        ("cos inside k_pages", call(cos=kp.ctypes.data + 64), "cos must not overlap the pool"),
        ("sin overlaps the end of v_pages (bytes)", call(sin=vp.ctypes.data + pool_bytes - 16), "sin must not overlap the pool"),
        ("kv_lens_out inside cos", call(kv_lens_out=cs.ctypes.data + 16), "kv_lens_out must not overlap cos"),
        ("kv_lens_out at the end of sin (bytes)", call(kv_lens_out=sn.ctypes.data + TAB_BYTES - 8), "kv_lens_out must not overlap sin"),
        ("misaligned device cos", call(cos=cs.ctypes.data + 4, loc=1), "cos and sin must be 16-byte aligned"),
        ("misaligned device sin", call(sin=sn.ctypes.data + 8, loc=1), "cos and sin must be 16-byte aligned"),
    ]
    return out


def append_rope_neighbours(fp8=False):
    """calls every check must let through -> (name, arguments)"""
    import kv_fp8_cases as F8
    _, _, cs, sn, _ = _rope_buffers()
    kn, vn, kp, vp, tab, lens, lo = KC._append_buffers()
    pool = (kp, vp) + (F8._scale_buffers() if fp8 else (2,))
    pool_bytes = 20 * 16 * 32 * (1 if fp8 else 2)
    head = (kn, vn, 2, 4, 1, 32, 0)
    return [("the well-formed call", head + (cs, sn, 40, 32, 0) + pool + (tab, lens, lo, 20, 16, 13)),
            ("lengths in place, interleaved, rot_dim 16", head + (cs, sn, 40, 16, 1) + pool + (tab, lens, lens, 20, 16, 13)),
            ("sin right behind v_pages", head + (cs, vp.ctypes.data + pool_bytes, 40, 32, 0) + pool + (tab, lens, lo, 20, 16, 13)),
            ("kv_lens_out right behind cos", head + (cs, sn, 40, 32, 0) + pool + (tab, lens, cs.ctypes.data + TAB_BYTES, 20, 16, 13))]
