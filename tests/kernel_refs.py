"""High-precision references for the kernel-harness tests (fp64 torch / numpy) and the emulation of the operand-plane formats of
kernels/split_planes.h.  Checked on the CPU by test_kernel_refs_cpu.py and test_gemm_refs_cpu.py."""
import numpy as np
import torch
import torch.nn.functional as F


def image2patches_nhwc(x, th, tw, cpad):
    """x [B,Cimg,H,W] -> [B,th,tw,cpad] float64: y[b][ty][tx][(c*gh + hg)*gw + wg] = x[b][c][hg*th + ty][wg*tw + tx], zero in [cout, cpad)"""
    x = np.asarray(x, np.float64)
    B, C, H, W = x.shape
    gh, gw = H // th, W // tw
    y = np.zeros((B, th, tw, cpad), np.float64)
    for c in range(C):
        for hg in range(gh):
            for wg in range(gw):
                y[..., (c * gh + hg) * gw + wg] = x[:, c, hg * th:(hg + 1) * th, wg * tw:(wg + 1) * tw]
    return y


def resize_nchw(x, oh, ow):
    """align-corners bilinear resize of [B,C,H,W], in fp64"""
    return F.interpolate(torch.as_tensor(np.asarray(x, np.float64)), size=(oh, ow), mode="bilinear", align_corners=True).numpy()


def resize_nhwc(x, oh, ow):
    """the same on a channels-last [B,H,W,C] array"""
    return resize_nchw(np.asarray(x, np.float64).transpose(0, 3, 1, 2), oh, ow).transpose(0, 2, 3, 1)


def head_stencil5x5(img, k, bias):
    """img [B,3,H,W], k [9][5][5][3] (case, fy, fx, channel), bias [9] -> [B,H,W]: the case of a pixel is 3*(0 first row | 2 last row | 1)
    + (0 first column | 2 last column | 1); taps outside the image are zero.  Nine zero-padded convolutions, one selected per pixel."""
    img = torch.as_tensor(np.asarray(img, np.float64))
    k = torch.as_tensor(np.asarray(k, np.float64)).reshape(9, 5, 5, 3)
    bias = torch.as_tensor(np.asarray(bias, np.float64))
    B, _, H, W = img.shape
    full = [F.conv2d(img, k[cs].permute(2, 0, 1)[None], bias[cs:cs + 1], padding=2)[:, 0] for cs in range(9)]
    assert H >= 2 and W >= 2                                     # (a row that is first and last has no case of its own: refused)
    ry, rx = torch.ones(H, dtype=torch.long), torch.ones(W, dtype=torch.long)
    ry[0], ry[H - 1], rx[0], rx[W - 1] = 0, 2, 0, 2
    case = ry[:, None] * 3 + rx[None, :]
    out = torch.zeros(B, H, W, dtype=torch.float64)
    for cs in range(9):
        out = torch.where((case == cs)[None], full[cs], out)
    return out.numpy()


def patch_merge_gather(x):
    """PatchMerging's input rows: x [B,H,W,Cin] -> [B*ceil(H/2)*ceil(W/2), 4*Cin], the four tokens (2i,2j), (2i+1,2j), (2i,2j+1), (2i+1,2j+1)
    concatenated in that order, zero outside the map (odd H / W)"""
    x = np.asarray(x)
    B, H, W, Cin = x.shape
    xp = np.zeros((B, H + (H & 1), W + (W & 1), Cin), x.dtype)
    xp[:, :H, :W] = x
    parts = [xp[:, 0::2, 0::2], xp[:, 1::2, 0::2], xp[:, 0::2, 1::2], xp[:, 1::2, 1::2]]
    return np.concatenate(parts, axis=-1).reshape(-1, 4 * Cin)


def layer_norm(x, gamma, beta, eps=1e-5):
    x = torch.as_tensor(np.asarray(x, np.float64))
    return F.layer_norm(x, (x.shape[-1],), torch.as_tensor(np.asarray(gamma, np.float64)), torch.as_tensor(np.asarray(beta, np.float64)), eps).numpy()


# ---- operand planes (kernels/split_planes.h) ----
# A row of K logical columns (K % 32 == 0) in the P layout: the 32-column tile kt occupies NP x 64 bytes, plane p at byte 64*NP*kt + 64*p,
# 2 bytes per element.  P2 / P3 hold bf16 planes, H2 is the P2 layout with the two fp16 planes of s*x.

def decode_planes(rows_u8, NP):
    """rows_u8 [rows, nbytes] uint8 (nbytes % (64*NP) == 0) -> uint16 bit patterns [NP, rows, K], K = nbytes / (2*NP)"""
    rows_u8 = np.ascontiguousarray(rows_u8, np.uint8)
    rows, nbytes = rows_u8.shape
    assert nbytes % (64 * NP) == 0
    t = rows_u8.view(np.uint16).reshape(rows, nbytes // (64 * NP), NP, 32)
    return np.ascontiguousarray(t.transpose(2, 0, 1, 3)).reshape(NP, rows, -1)


def encode_planes(planes_u16):
    """the inverse, written from store_planes<NP>: element `col` of plane `pl` goes to byte (col >> 5)*(64*NP) + (col & 31)*2 + 64*pl"""
    planes_u16 = np.asarray(planes_u16, np.uint16)
    NP, rows, K = planes_u16.shape
    assert K % 32 == 0
    out = np.zeros((rows, K * 2 * NP), np.uint8)
    for pl in range(NP):
        for col in range(K):
            o = (col >> 5) * (64 * NP) + (col & 31) * 2 + 64 * pl
            out[:, o] = planes_u16[pl, :, col] & 0xFF            # little endian
            out[:, o + 1] = planes_u16[pl, :, col] >> 8
    return out


def _bits16(t):
    return t.view(torch.int16).numpy().view(np.uint16)


def split_bf16(x, NP):
    """fp32 x -> (bits [NP, ...] uint16, values [NP, ...] float32): plane 0 = RNE_bf16(x), plane p+1 = RNE_bf16 of the exact fp32 remainder"""
    r = torch.as_tensor(np.asarray(x, np.float32)).clone()
    bits, vals = [], []
    for _ in range(NP):
        h = r.to(torch.bfloat16)
        bits.append(_bits16(h))
        vals.append(h.float().numpy())
        r = r - h.float()                                        # exact: the remainder of an RNE rounding fits the format it came from
    return np.stack(bits), np.stack(vals)


def split_h2(x, s):
    """fp32 x, s a power of two -> (bits [2, ...] uint16, values [2, ...] float32): hi = RNE_f16(s*x), lo = RNE_f16(s*x - hi)"""
    sx = torch.as_tensor(np.asarray(x, np.float32)) * np.float32(s)
    hi = sx.to(torch.float16)
    lo = (sx - hi.float()).to(torch.float16)
    return np.stack([_bits16(hi), _bits16(lo)]), np.stack([hi.float().numpy(), lo.float().numpy()])


def bf16_bits_to_f64(b):
    return (np.asarray(b, np.uint16).astype(np.uint32) << 16).view(np.float32).astype(np.float64)


def f16_bits_to_f64(b):
    return np.asarray(b, np.uint16).view(np.float16).astype(np.float64)


# ---- the GEMMs of kernels/gemm_f32.hip and kernels/gemm_split.hip ----
# The plane products a kernel keeps, as (A plane, W plane): three bf16 planes drop ml, lm, ll; two drop mm; the fp16 pair drops ll.
KEPT = {
    "bf16x3": ((0, 0), (0, 1), (1, 0), (0, 2), (2, 0), (1, 1)),
    "bf16x2": ((0, 0), (0, 1), (1, 0)),
    "h2": ((0, 0), (0, 1), (1, 0)),
}
ACT_NONE, ACT_RELU, ACT_GELU = 0, 1, 2


def gemm_planes_ref(a_planes, w_planes, kept, out_scale=1.0):
    """a_planes [NP, M, K], w_planes [NP, N, K] (plane VALUES) -> fp64 [M, N]: out_scale * the sum over `kept` of A_pa W_pb^T.  Every product
    of two 16-bit values is exact in fp64; out_scale is the power of two 1 / (a_scale w_scale) of the fp16 pair."""
    a, w = np.asarray(a_planes, np.float64), np.asarray(w_planes, np.float64)
    acc = np.zeros((a.shape[1], w.shape[1]), np.float64)
    for pa, pb in kept:
        acc += a[pa] @ w[pb].T
    return acc * float(out_scale)


def gemm_epilogue_ref(acc, bias=None, bbias=None, bbias_rows=0, scale=None, shift=None, act=ACT_NONE, R=None):
    """GemmParams' epilogue in fp64, in its documented order: bias[n], bbias[m / bbias_rows][n], scale and shift, activation, residual"""
    v = np.asarray(acc, np.float64).copy()
    if bias is not None:
        v += np.asarray(bias, np.float64)[None, :]
    if bbias is not None:
        v += np.asarray(bbias, np.float64)[np.arange(v.shape[0]) // bbias_rows]
    if scale is not None:
        v = v * np.asarray(scale, np.float64)[None, :] + np.asarray(shift, np.float64)[None, :]
    if act == ACT_RELU:
        v = np.maximum(v, 0.0)
    elif act == ACT_GELU:
        v = F.gelu(torch.from_numpy(v)).numpy()                       # erf form, fp64
    if R is not None:
        v += np.asarray(R, np.float64)
    return v


def im2col_nhwc(x, kh, kw, stride, pad, dil=1):
    """GEMM_CONV_NHWC's rows: x [B, H, W, C] -> ([B Hout Wout, kh kw C], Hout, Wout), K order (ky, kx, ci), zero outside the map"""
    x = np.asarray(x)
    B, H, W, C = x.shape
    Ho, Wo = (H + 2 * pad - dil * (kh - 1) - 1) // stride + 1, (W + 2 * pad - dil * (kw - 1) - 1) // stride + 1
    xp = np.zeros((B, H + 2 * pad, W + 2 * pad, C), x.dtype)
    xp[:, pad:pad + H, pad:pad + W] = x
    taps = [xp[:, ky * dil:ky * dil + (Ho - 1) * stride + 1:stride, kx * dil:kx * dil + (Wo - 1) * stride + 1:stride]
            for ky in range(kh) for kx in range(kw)]
    return np.stack(taps, axis=3).reshape(B * Ho * Wo, kh * kw * C), Ho, Wo


def im2col_nchw(x, kh, kw, stride, pad, kpad):
    """GEMM_GATHER_NCHW's rows: x [B, C, H, W] -> ([B Hout Wout, kpad], Hout, Wout), K order (ci, ky, kx), zero outside the map and in [C kh kw, kpad)"""
    x = np.asarray(x)
    cols, Ho, Wo = im2col_nhwc(x.transpose(0, 2, 3, 1), kh, kw, stride, pad)
    B, C = x.shape[:2]
    cols = cols.reshape(-1, kh * kw, C).transpose(0, 2, 1).reshape(B * Ho * Wo, C * kh * kw)
    out = np.zeros((cols.shape[0], kpad), x.dtype)
    out[:, :C * kh * kw] = cols
    return out, Ho, Wo


# Plane-exact data: sign * (1 + j 2^-9 + l 2^-18), j in {0, 1}, l in {0, j} ("bf16x3": the planes are 1, j 2^-9, l 2^-18 — an l without its j
# would sit in the MIDDLE plane), sign * (1 + j 2^-9) ("bf16x2", "f32") or sign * (1 + j 2^-12) ("h2": fp16 planes 1, j 2^-12 of the unscaled
# value).  Every kept plane product, and every product of two "f32" values, is then a multiple of UNIT[kind] (times the power-of-two operand
# scales), so any partial sum of them in any order is exact in fp32 as long as its magnitude stays below 2^24 UNIT: plane_exact_bound.
UNIT = {"f32": 2.0 ** -18, "bf16x3": 2.0 ** -18, "bf16x2": 2.0 ** -9, "h2": 2.0 ** -12}


def plane_exact_values(shape, kind, seed):
    g = np.random.default_rng(seed)
    sign = g.integers(0, 2, shape) * 2.0 - 1.0
    j = g.integers(0, 2, shape).astype(np.float64)
    l = g.integers(0, 2, shape) * j
    if kind == "h2":
        v = 1.0 + j * 2.0 ** -12
    elif kind == "bf16x3":
        v = 1.0 + j * 2.0 ** -9 + l * 2.0 ** -18
    else:
        v = 1.0 + j * 2.0 ** -9
    return (sign * v).astype(np.float32)


def keep_per_row(rows, cols, nkeep, seed):
    """a 0 / 1 mask [rows, cols] with exactly min(nkeep, cols) ones per row, at random columns"""
    g = np.random.default_rng(seed)
    order = np.argsort(g.random((rows, cols)), axis=1)
    return (order < min(nkeep, cols)).astype(np.float32)


def assert_plane_exact(a_rows, w, kind, addends=0.0, scale_max=1.0, scale_min=1.0, post=0.0):
    """The exactness condition of a plane-exact case, asserted on the CPU: a_rows [M, K] (the rows the kernel contracts: after im2col), w [N, K].
    max_mn sum_k |a||w| bounds every partial sum of kept products whatever the tile, ring depth or split-K.  The epilogue's operands are
    multiples of 1/4: bias and bbias (`addends` = the largest |bias| + |bbias|) keep the unit, a power-of-two scale multiplies value and unit
    (scale_min <= 1 <= scale_max), shift and residual (`post` = the largest |shift| + |R|) are added after it.  Returns the margin (< 1)."""
    sums = np.abs(np.asarray(a_rows, np.float64)) @ np.abs(np.asarray(w, np.float64)).T
    top = (sums.max() + addends) * scale_max + post
    limit = 2.0 ** 24 * UNIT[kind] * scale_min
    assert top < limit, f"not plane-exact: partial sums reach {top} >= 2^24 x {UNIT[kind] * scale_min}"
    return top / limit
