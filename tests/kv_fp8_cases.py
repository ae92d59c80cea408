"""What tests/test_kv_fp8_cpu.py, tests/test_flash_attention_paged_fp8_gpu.py and tests/test_kv_cache_append_fp8_gpu.py share: the numpy /
torch statement of the OCP e4m3fn format (WIDEN, quant), the scale sets, pools quantised ON THE CPU (0xFF wherever the entry must not
read), raw ctypes calls of the two fp8 entries and their refusal lists.

The cases, pools, reference and bounds are those of flash_attention_paged_cases (PG) and kv_cache_cases (KC), imported and not edited."""
import functools

import numpy as np
import torch

import flash_attention_paged_cases as PG
import kv_cache_cases as KC

# byte -> the fp32 value it stands for (0x7F and 0xFF: NaN)
WIDEN = torch.arange(256, dtype=torch.uint8).view(torch.float8_e4m3fn).float().numpy()
WIDEN.setflags(write=False)
NAN_BYTES = (0x7F, 0xFF)
NOT_NAN = np.array([i for i in range(256) if i not in NAN_BYTES])
UNREAD = 0xFF                   # what every byte the entries must not read holds: a NaN


def quant(x, scale):
    """THE RULE of the append, on the CPU: fp32 division (correctly rounded), clamp to +-448 with NaN kept, round to nearest even into
    e4m3fn -> bytes.  scale: a scalar, or an array that broadcasts against x"""
    x = np.ascontiguousarray(x, np.float32)
    with np.errstate(over="ignore"):                # (3e38 / 0.0173 is +inf, and is clamped)
        t = (x / np.asarray(scale, np.float32)).astype(np.float32)
    return torch.clamp(torch.from_numpy(np.ascontiguousarray(t)), -448, 448).to(torch.float8_e4m3fn).view(torch.uint8).numpy()


# the facts the tests rest on
assert np.isnan(WIDEN[list(NAN_BYTES)]).all() and np.isfinite(WIDEN[NOT_NAN]).all() and NOT_NAN.size == 254 and np.abs(WIDEN[NOT_NAN]).max() == 448.0
assert np.array_equal(WIDEN[NOT_NAN].astype(np.float16).astype(np.float32), WIDEN[NOT_NAN]), "every e4m3 value is an fp16 value"
assert np.array_equal(torch.from_numpy(WIDEN[NOT_NAN].copy()).to(torch.bfloat16).float().numpy(), WIDEN[NOT_NAN]), "every e4m3 value is a bf16 value"
assert np.array_equal(quant(WIDEN[NOT_NAN], 1), NOT_NAN.astype(np.uint8)), "quant is the inverse of WIDEN on every non-NaN byte (the sign of zero included)"
# round to nearest even, the ties at 0 / 2^-9 and at 464, saturation by the clamp, NaN
assert quant(np.array([2.0 ** -10, 1.5 * 2.0 ** -9, 1 + 2.0 ** -4, 1 + 3 * 2.0 ** -4, 464.0, 465.0, 1e6, -1e6, -0.0], np.float32), 1).tolist() == \
    [0x00, 0x02, 0x38, 0x3A, 0x7E, 0x7E, 0x7E, 0xFE, 0x80]
assert (quant(np.array([np.nan], np.float32), 1)[0] & 0x7F) == 0x7F

MODES = ("f32", "bf16", "f16")
# (name, k_scale, v_scale): ones, powers of two, neither
SCALES = (("ones", 1.0, 1.0), ("pow2", 2.0 ** -6, 2.0 ** -5), ("odd", 0.0173, 0.031))
SCALE_IDS = [s[0] for s in SCALES]


def scale_arrays(kv_heads, ks, vs):
    """uniform [kv_heads] fp32 arrays"""
    return np.full(kv_heads, ks, np.float32), np.full(kv_heads, vs, np.float32)


def per_head_scales(kv_heads):
    """different scales per K / V head, none a power of two"""
    h = np.arange(kv_heads, dtype=np.float32)
    return (np.float32(0.0173) * (1 + h)).astype(np.float32), (np.float32(0.031) / (1 + np.float32(0.5) * h)).astype(np.float32)


def case_scale(case):
    """the explicit scale s of a case: literal fp32 values, so that no host sqrt enters (0.125 is 64^-0.5)"""
    kind_s = PG.kind_scale(case[3])
    return float(np.float32(kind_s)) if kind_s else {32: float(np.float32(0.17677669)), 64: 0.125, 128: float(np.float32(0.088388346))}[case[0][4]]


def quant_pool(pool, scale):
    """an fp32 pool [n_pages, page, kv_heads, hd] of PG.build_pool (NaN wherever the entry must not read) -> its bytes at `scale`
    ([kv_heads]), UNREAD wherever the fp32 pool holds NaN"""
    b = quant(np.nan_to_num(pool, nan=0.0), np.asarray(scale, np.float32)[None, None, :, None])
    b[np.isnan(pool)] = UNREAD
    return b


@functools.lru_cache(maxsize=None)
def _pool_cached(case, page, shuffle, ks_bytes, vs_bytes):
    kp, vp, table, lens = PG.build_pool(case, page, shuffle)
    ks, vs = np.frombuffer(ks_bytes, np.float32), np.frombuffer(vs_bytes, np.float32)
    kb, vb = quant_pool(kp, ks), quant_pool(vp, vs)
    assert (kb[np.isnan(kp)] == UNREAD).all() and np.isnan(kp).any() and not np.isnan(WIDEN[kb[~np.isnan(kp)]]).any()
    for a in (kb, vb):
        a.setflags(write=False)
    return kb, vb, table, lens


def pool(case, ks, vs, page=None, shuffle=True):
    """(k bytes, v bytes, table, lens) of the case quantised on the CPU with the [kv_heads] scales ks, vs (read-only, computed once)"""
    return _pool_cached(case, page, shuffle, np.asarray(ks, np.float32).tobytes(), np.asarray(vs, np.float32).tobytes())


def dequant(b, scale):
    """bytes [..., kv_heads, hd] -> scale[h] * WIDEN[byte] in float64"""
    return np.asarray(scale, np.float64)[:, None] * WIDEN[b].astype(np.float64)


# ---- raw calls ----
_ptr = KC._ptr


def raw_attend(lib, q, kp, vp, ks, vs, table, lens, batch, seq_q, max_kv_len, heads, kv_heads, head_dim, n_pages, page_size, max_pages, layout, causal, scale,
               kv_splits, y, lse, ws, ws_floats, loc=0, stream=None):
    """brn_flash_attention_paged_fp8_forward with the integers exactly as given; the pointers: numpy arrays, integers taken as addresses, or None"""
    st = lib.brn_flash_attention_paged_fp8_forward(_ptr(q), _ptr(kp), _ptr(vp), _ptr(ks), _ptr(vs), _ptr(table), _ptr(lens), batch, seq_q, max_kv_len, heads, kv_heads,
                                                   head_dim, n_pages, page_size, max_pages, layout, causal, scale, kv_splits, _ptr(y), _ptr(lse), _ptr(ws), ws_floats, loc, 0, stream)
    return st, (lib.brn_last_error() or b"").decode()


def raw_append(lib, k_new, v_new, batch, seq_new, kv_heads, head_dim, layout, kp, vp, ks, vs, table, lens, lens_out, n_pages, page_size, max_pages, loc=0, stream=None):
    """brn_kv_cache_append_fp8 with the integers exactly as given"""
    st = lib.brn_kv_cache_append_fp8(_ptr(k_new), _ptr(v_new), batch, seq_new, kv_heads, head_dim, layout, _ptr(kp), _ptr(vp), _ptr(ks), _ptr(vs), _ptr(table), _ptr(lens),
                                     _ptr(lens_out), n_pages, page_size, max_pages, loc, 0, stream)
    return st, (lib.brn_last_error() or b"").decode()


@functools.lru_cache(maxsize=None)
def _scale_buffers():
    return np.ones(8, np.float32), np.ones(8, np.float32)


POOL_BYTES = 20 * 16 * 32           # the pool of the well-formed calls below as fp8: 20 pages x 16 keys x 1 head x 32, one byte each


def attend_refusals():
    """(name, arguments of raw_attend after lib, words the message must contain).  Every refusal of PG.refusals() with the two scale
    arrays inserted (the inherited limits, under the new prefix) except the one whose buffer lies behind the END of an fp32 pool, which is
    restated in bytes; then the new limits.  The refused calls read nothing."""
    ks, vs = _scale_buffers()
    out = [(name, args[:3] + (ks, vs) + args[3:], word) for name, args, word in PG.refusals() if name != "workspace overlaps the end of v_pages"]
    assert len(out) == len(PG.refusals()) - 1
    q, kp, vp, y, lse, ws, table, lens = PG._refusal_buffers()
    ok = (2, 16, 200, 2, 1, 32, 20, 16, 13, 0, 0, 0.0, 2)
    tail = (y, lse, ws, 4224)
    ins = (q, kp, vp, ks, vs, table, lens)
    out += [
        ("workspace overlaps the end of an fp8 v_pages (bytes)", ins + ok + (y, lse, vp.ctypes.data + POOL_BYTES - 16, 4224), "overlap"),
        ("lse overlaps the end of an fp8 k_pages (bytes)", ins + ok + (y, kp.ctypes.data + POOL_BYTES - 4, ws, 4224), "overlap"),
        ("y is k_scale", ins + ok + (ks.ctypes.data, lse, ws, 4224), "overlap"),
        ("workspace overlaps v_scale", (q, kp, vp, ks, ws.ctypes.data + 64, table, lens) + ok + tail, "overlap"),
        ("lse is v_scale with a NULL k_scale", (q, kp, vp, None, vs, table, lens) + ok + (y, vs.ctypes.data, ws, 4224), "overlap"),
        ("misaligned device fp8 k_pages", (q, kp.ctypes.data + 4096 + 8, vp, ks, vs, table, lens) + ok + tail + (1,), "16-byte aligned"),
        ("misaligned device k_scale", (q, kp, vp, ks.ctypes.data + 2, vs, table, lens) + ok + tail + (1,), "k_scale and v_scale must be 4-byte aligned"),
        ("misaligned device v_scale", (q, kp, vp, None, vs.ctypes.data + 1, table, lens) + ok + tail + (1,), "k_scale and v_scale must be 4-byte aligned"),
    ]
    return out


def attend_neighbours():
    """calls every check must LET THROUGH: NULL scales, and outputs that start where the fp8 pool ends -> (name, arguments)"""
    ks, vs = _scale_buffers()
    q, kp, vp, y, lse, ws, table, lens = PG._refusal_buffers()
    ok = (2, 16, 200, 2, 1, 32, 20, 16, 13, 0, 0, 0.0, 2)
    return [("the well-formed call", (q, kp, vp, ks, vs, table, lens) + ok + (y, lse, ws, 4224)),
            ("NULL scales", (q, kp, vp, None, None, table, lens) + ok + (y, lse, ws, 4224)),
            ("workspace right behind an fp8 v_pages", (q, kp, vp, ks, vs, table, lens) + ok + (y, lse, vp.ctypes.data + POOL_BYTES, 4224)),
            ("lse right behind an fp8 k_pages", (q, kp, vp, ks, None, table, lens) + ok + (y, kp.ctypes.data + POOL_BYTES, ws, 4224))]


def append_refusals():
    """(name, arguments of raw_append after lib, words the message must contain): KC.append_refusals() with the two scale arrays in the
    place of kv_type, without the kv_type ones and with those that count the bytes of a 16-bit pool restated for one byte per element;
    then the new limits"""
    ks, vs = _scale_buffers()
    out = [(name, a[:9] + (ks, vs) + a[10:], word) for name, a, word in KC.append_refusals() if "kv_type" not in name and "(bytes)" not in name]
    assert len(out) == len(KC.append_refusals()) - 4
    kn, vn, kp, vp, table, lens, lo = KC._append_buffers()
    base = (2, 4, 1, 32, 0)

    def call(k_new=kn, v_new=vn, k_pages=kp, v_pages=vp, k_scale=ks, v_scale=vs, kv_lens_out=lo, loc=0):
        return (k_new, v_new) + base + (k_pages, v_pages, k_scale, v_scale, table, lens, kv_lens_out, 20, 16, 13, loc)

    out += [
        ("v_new overlaps the end of an fp8 v_pages (bytes)", call(v_new=vp.ctypes.data + POOL_BYTES - 16), "v_new must not overlap the pool"),
        ("v_pages overlaps the end of an fp8 k_pages (bytes)", call(v_pages=kp.ctypes.data + POOL_BYTES - 32), "k_pages and v_pages must not overlap"),
        ("k_scale inside k_pages", call(k_scale=kp.ctypes.data + 256), "k_scale must not overlap the pool"),
        ("v_scale inside v_pages", call(v_scale=vp.ctypes.data + POOL_BYTES - 4), "v_scale must not overlap the pool"),
        ("kv_lens_out inside v_scale", call(kv_lens_out=vs.ctypes.data), "kv_lens_out must not overlap v_scale"),
        ("misaligned device k_scale", call(k_scale=ks.ctypes.data + 2, loc=1), "k_scale and v_scale must be 4-byte aligned"),
        ("misaligned device fp8 k_pages", call(k_pages=kp.ctypes.data + 8, loc=1), "16-byte aligned"),
    ]
    return out


def append_neighbours():
    """calls every check must let through -> (name, arguments)"""
    ks, vs = _scale_buffers()
    kn, vn, kp, vp, table, lens, lo = KC._append_buffers()
    base = (2, 4, 1, 32, 0)
    return [("the well-formed call", (kn, vn) + base + (kp, vp, ks, vs, table, lens, lo, 20, 16, 13)),
            ("NULL scales, lengths in place", (kn, vn) + base + (kp, vp, None, None, table, lens, lens, 20, 16, 13)),
            ("v_new right behind an fp8 v_pages", (kn, vp.ctypes.data + POOL_BYTES) + base + (kp, vp, ks, vs, table, lens, lo, 20, 16, 13)),
            ("kv_lens_out right behind an fp8 k_pages", (kn, vn) + base + (kp, vp, ks, vs, table, lens, kp.ctypes.data + POOL_BYTES, 20, 16, 13))]


# ---- the append's inputs: KC.new_tokens (KC.SPECIALS among them) plus the values that matter in e4m3, each times the head's scale ----
FP8_SPECIALS = np.array([1 + 2.0 ** -4, 1 + 3 * 2.0 ** -4, -(1 + 2.0 ** -4), 448.0, 464.0, 465.0, 1e6, -1e6, 2.0 ** -9, 2.0 ** -10, 1.5 * 2.0 ** -9, -(2.0 ** -10), 0.0, -0.0], np.float32)
assert FP8_SPECIALS.size + KC.SPECIALS.size <= 32
assert quant(FP8_SPECIALS, 1).tolist() == [0x38, 0x3A, 0xB8, 0x7E, 0x7E, 0x7E, 0x7E, 0xFE, 0x01, 0x00, 0x02, 0x80, 0x00, 0x80]
assert np.isnan(KC.SPECIALS).sum() == 1 and not np.signbit(KC.SPECIALS[np.isnan(KC.SPECIALS)]).any(), "the NaN among the inputs is positive"


@functools.lru_cache(maxsize=None)
def new_tokens(name, hd, ks_bytes, vs_bytes):
    """k_new, v_new [batch, seq_new, kv_heads, hd] fp32 (BSHD, read-only): KC.new_tokens with FP8_SPECIALS x the head's scale written
    behind KC.SPECIALS at the start of every head's first row of k and of v"""
    k, v = (np.array(a) for a in KC.new_tokens(name, hd))
    ks, vs = np.frombuffer(ks_bytes, np.float32), np.frombuffer(vs_bytes, np.float32)
    n0, n = KC.SPECIALS.size, FP8_SPECIALS.size
    for a, s in ((k, ks), (v, vs)):
        for h in range(a.shape[2]):
            a[:, 0, h, n0:n0 + n] = FP8_SPECIALS * s[h]
        a.setflags(write=False)
    return k, v


def sentinel_pool(c, hd, pages=None):
    return np.full((pages or KC.n_pages_of(c), c["page"], c["kv_heads"], hd), UNREAD, np.uint8)


def expected_append(name, hd, ks, vs):
    """(k pool bytes, v pool bytes, kv_lens_out, k NaN mask, v NaN mask) of the case on pools of UNREAD: KC.append_rule on quant()"""
    c = KC.APPEND_CASES[name]
    ks, vs = np.asarray(ks, np.float32), np.asarray(vs, np.float32)
    k, v = new_tokens(name, hd, ks.tobytes(), vs.tobytes())
    table, lens = KC.table_of(name), np.asarray(c["lens"], np.int32)
    kq, vq = quant(k, ks[None, None, :, None]), quant(v, vs[None, None, :, None])
    kb, lo = KC.append_rule(kq, sentinel_pool(c, hd), table, lens)
    vb, _ = KC.append_rule(vq, sentinel_pool(c, hd), table, lens)
    none = np.zeros(kb.shape, bool)
    return kb, vb, lo, KC.append_rule((kq & 0x7F) == 0x7F, none, table, lens)[0], KC.append_rule((vq & 0x7F) == 0x7F, none, table, lens)[0]
