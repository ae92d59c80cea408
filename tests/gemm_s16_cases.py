"""The case table of test_gemm_s16_forms_gpu.py (launch_gemm_bf16 of kernels/gemm_bf16.hip, both storage types), each case's host data (exact
or Gaussian) and its fp64 reference.  Numpy / torch-on-CPU only: test_gemm_s16_refs_cpu.py asserts the conditions of every case without a GPU.

Exact data: A and W hold integers |x| <= 4 (exact in bf16 and fp16), bias / per-image bias / shift are multiples of 1/4 with |.| <= 1, scale is
in {+-1, +-0.5}, a 16-bit residual is a multiple of 1/4 with |.| <= 2 and an fp32 residual a multiple of 1/4 with |.| <= 64.  Every product and
every partial sum in any order is then an integer below 16 K < 2^24 and every epilogue step is exact in fp32: an fp32 C must equal the fp64
reference, a 16-bit C its round-to-nearest-even rounding.  GELU cases (no exact value) keep the activation's argument within |x| <= 6: their A
has two non-zeros of magnitude 1 per row and their W stays within |w| <= 2."""
import functools
import zlib
from dataclasses import dataclass

import numpy as np
import torch

import kernel_refs as KR

S16 = {"bf16": (0, torch.bfloat16), "f16": (1, torch.float16)}                # storage type -> (kh_launch_gemm_s16's f16, torch type)
MANT = {"bf16": (7, -126), "f16": (10, -14)}                                  # explicit mantissa bits, smallest normal exponent
TILES = {0: (128, 128), 1: (128, 64), 2: (256, 256), 3: (256, 192)}           # cfg -> (BM, BN); a dense K tail always runs 128 x 128
WG_PER_CU = {0: 2, 1: 3, 2: 1, 3: 1}
A_PAD, A_COFF = 48, 16       # a dense A sits in columns [16, 16 + K) of rows K + 48 wide; the other columns hold noise
MAP_PAD = 64                 # a conv input is a Cin-channel window of a map Cin + 64 channels wide; the other channels hold noise
C_ROWS_BEHIND = 2            # sentinel rows behind row M - 1 of every output
GELU_AS, GELU_S16OUT = 6.1e-7, 3.0e-6        # |error| for |x| <= 6 documented at gelu_erf_as / gelu_erf_bf16out (kernels/gemm_common.h)

# conv geometries: B, H, W, Cin, k (or (kh, kw)), pad, stride, dil, a_coff, chunk_major (None = as pack_s16_storage decides: Cin % 64 == 0 and Cin > 64)
CONVS = {
    "c64": (3, 10, 10, 64, 3, 1, 1, 1, 0, None),
    "c96": (3, 10, 10, 96, 3, 1, 1, 1, 0, None),            # K steps straddle taps; K = 864, K % 64 == 32: the c_ky < kh tail
    "c128cm": (3, 10, 10, 128, 3, 1, 1, 1, 0, None),        # chunk-major K order
    "c128tm": (3, 10, 10, 128, 3, 1, 1, 1, 0, False),       # the same weights tap-major
    "k7": (1, 12, 12, 64, 7, 3, 1, 1, 0, None),
    "s2": (2, 17, 15, 64, 3, 1, 2, 1, 0, None),
    "d2": (3, 10, 10, 64, 3, 2, 1, 2, 0, None),
    "ragged": (3, 9, 11, 64, 3, 1, 1, 1, 0, None),
    "b5": (5, 7, 7, 64, 3, 1, 1, 1, 0, None),               # 49 pixels per image: a 128-row tile spans four images, the 256-row tile all five
    "b6": (6, 7, 7, 64, 3, 1, 1, 1, 0, None),               # rows 0 .. 255 of the 256-row tile lie in six images
    "coff": (3, 10, 10, 64, 3, 1, 1, 1, 32, None),          # the window in the middle of the wider map
    "k3x5": (3, 10, 12, 64, (3, 5), 1, 1, 1, 0, None),      # kh != kw: tap -> (ky, kx) divides by kw
}


def conv_geometry(name):
    B, H, W, Cin, k, pad, stride, dil, coff, cm = CONVS[name]
    kh, kw = k if isinstance(k, tuple) else (k, k)
    Ho, Wo = (H + 2 * pad - dil * (kh - 1) - 1) // stride + 1, (W + 2 * pad - dil * (kw - 1) - 1) // stride + 1
    return dict(B=B, H=H, W=W, Cin=Cin, kh=kh, kw=kw, pad=pad, stride=stride, dil=dil, coff=coff, cm=cm, Ho=Ho, Wo=Wo, M=B * Ho * Wo, K=kh * kw * Cin)


@dataclass(frozen=True)
class Case:
    conv: str = ""           # "" = dense, else a key of CONVS (M and K are then the geometry's)
    M: int = 300
    N: int = 200
    K: int = 128
    cfg: int = 2
    splitk: int = 1
    cus: int = 256           # set_launch_cus: the persistent grid is cus x WG_PER_CU[cfg] workgroups at most
    c_f32: bool = False
    bias: bool = False
    bbias_rows: int = 0
    scale: bool = False
    act: int = KR.ACT_NONE
    R: str = ""              # "" | sep | inplace
    r_f32: bool = False
    r_pad: int = 16          # ldr = N + r_pad
    r_coff: int = 8
    c_pad: int = 16          # ldc = N + c_pad
    c_coff: int = 8
    positive: bool = False   # exact data without signs: sums around 4 K, so that integers above 2048 (exact ties in fp16) occur

    def __post_init__(self):
        if self.conv:
            g = conv_geometry(self.conv)
            object.__setattr__(self, "M", g["M"])
            object.__setattr__(self, "K", g["K"])

    @property
    def flavour(self):
        """the epilogue flavour launch_bf16_cfg picks (restated), 3 = the split-K reduce kernel"""
        if self.splitk > 1:
            return 3
        ldc = self.N + self.c_pad
        if self.N % 8 == 0 and not self.c_f32 and ldc % 8 == 0 and self.c_coff % 8 == 0 and (
                not self.R or (not self.r_f32 and self.ldr % 8 == 0 and self.rcoff % 8 == 0)):
            return 0
        if self.N % 8 == 0 and self.c_f32 and not self.bbias_rows and ldc % 4 == 0 and self.c_coff % 4 == 0 and (
                not self.R or (self.r_f32 and self.ldr % 4 == 0 and self.rcoff % 4 == 0)):
            return 2 if (self.conv and self.R) else 1
        return 2

    @property
    def ldr(self):
        return self.N + self.c_pad if self.R == "inplace" else self.N + self.r_pad

    @property
    def rcoff(self):
        return self.c_coff if self.R == "inplace" else self.r_coff

    @property
    def group(self):
        """the group whose Gaussian bound applies"""
        return {0: "flavour 1", 1: "flavour 1", 2: "flavour 2", 3: "split-K reduce"}[self.flavour]

    @property
    def gelu_abs(self):
        """the documented error of the GELU form this case's epilogue uses"""
        return GELU_S16OUT if self.flavour == 0 else GELU_AS

    @property
    def tile(self):
        return (128, 128) if (not self.conv and self.K % 64) else TILES[self.cfg]

    @property
    def id(self):
        s = f"{self.conv or 'dense'}-cfg{self.cfg}-sk{self.splitk}-{self.M}x{self.N}x{self.K}-{'f32' if self.c_f32 else 's16'}"
        for flag, on in [(f"cus{self.cus}", self.cus != 256), ("bias", self.bias), (f"bbias{self.bbias_rows}", self.bbias_rows), ("scale", self.scale),
                         ("relu", self.act == KR.ACT_RELU), ("gelu", self.act == KR.ACT_GELU),
                         (f"R{'32' if self.r_f32 else '16'}{self.R}+{self.r_pad}@{self.r_coff}", self.R),
                         (f"C+{self.c_pad}@{self.c_coff}", (self.c_pad, self.c_coff) != (16, 8)), ("pos", self.positive)]:
            if on:
                s += "-" + flag
        return s


RES = {0: dict(R="sep"), 1: dict(R="inplace", r_f32=True)}          # the residual a flavour-0 / flavour-1 launch takes


def _walk_cases():
    """launch_cus = 8: every workgroup walks three or more work items, full tiles followed by full and by ragged ones"""
    shapes = {2: (1300, 1000), 3: (1300, 904), 0: (700, 1096), 1: (700, 712)}
    combos = [(fl, res) for fl in (0, 1) for res in (False, True)]
    out = []
    for cfg, (M, N) in shapes.items():
        for ki, K in enumerate([64, 128, 192, 256]):                 # nt = 1, 2, 3, 4: each arm of the kstep chain is the last one once
            for ci, (fl, res) in enumerate(combos):
                if cfg != 2 and ci != (ki + cfg) % 4:                # the 256 x 256 tile takes the whole cross, the others a Latin square of it
                    continue
                out.append(Case(M=M, N=N, K=K, cfg=cfg, cus=8, c_f32=fl == 1, bias=True, **(RES[fl] if res else {})))
    # item counts that are no multiple of 8 (20, 25, 45, 66) and below 8 (6 each)
    for cfg, (M, N) in {2: (1100, 1000), 3: (1100, 904), 0: (600, 1096), 1: (700, 648)}.items():
        out.append(Case(M=M, N=N, K=192, cfg=cfg, cus=8, c_f32=cfg % 2 == 1, **RES[cfg % 2]))
    for cfg, (M, N) in {2: (300, 700), 3: (300, 520), 0: (300, 200), 1: (200, 136)}.items():
        out.append(Case(M=M, N=N, K=128, cfg=cfg, cus=8, c_f32=cfg % 2 == 0, **RES[1 - cfg % 2]))
    return out


WALK_MAIN = 28               # the first 28 walk cases are the ones whose workgroups must walk >= 3 items


def _tile_cases():
    out = []
    for conv in ["", "c64"]:
        for cfg in range(4):
            for N in [904 if cfg == 3 else 200, 130]:                # 2 x 192 rows > the 256 W rows packed for N = 200; N % 8 != 0: flavour 2
                out += [Case(conv=conv, N=N, cfg=cfg, c_f32=f32) for f32 in (False, True)]
    # integers above 256 / 2048: exact ties of the 16-bit conversion (K = 1024, unsigned data: sums around 4096)
    out += [Case(N=200, K=1024, cfg=2, positive=True), Case(N=136, K=1024, cfg=1, positive=True, bias=True)]
    return out


def _ktail_cases():
    """K % 64 == 32, dense: the 128 x 128 general-address form whatever cfg says (N = 136: 192 <= the 256 packed rows for cfg 3)"""
    return [Case(N=136, K=K, cfg=cfg, splitk=sk, c_f32=K == 96, bias=True) for K in (96, 160) for cfg in range(4) for sk in (1, 2)]


def _conv_cases():
    return [Case(conv=name, N=136, cfg=cfg, bias=True, act=KR.ACT_RELU) for name in CONVS for cfg in range(4)]


F32 = dict(c_f32=True)
ALL = dict(bias=True, scale=True, act=KR.ACT_RELU, R="sep")
EPILOGUES = [
    dict(bias=True), dict(bias=True, **F32), dict(bias=True, N=130),
    dict(bbias_rows=50), dict(bbias_rows=50, **F32),                                   # vectorised in flavour 0; forces flavour 2 with fp32 C
    dict(scale=True), dict(scale=True, **F32),
    dict(act=KR.ACT_RELU, bias=True), dict(act=KR.ACT_RELU, bias=True, **F32),
    dict(act=KR.ACT_GELU, bias=True), dict(act=KR.ACT_GELU, bias=True, **F32), dict(act=KR.ACT_GELU, bias=True, N=130),
    dict(R="sep"), dict(R="inplace"), dict(R="sep", r_f32=True, **F32), dict(R="inplace", r_f32=True, **F32),
    dict(R="sep", **F32), dict(R="sep", r_f32=True),                                   # residual and C of different types: flavour 2
    dict(c_pad=12, c_coff=4), dict(c_pad=12, c_coff=4, **F32), dict(c_pad=9, c_coff=3), dict(c_pad=9, c_coff=3, **F32),
    dict(R="sep", r_pad=12, r_coff=4), dict(R="sep", r_f32=True, r_pad=12, r_coff=4, **F32),
    dict(R="sep", r_pad=9, r_coff=5), dict(R="sep", r_f32=True, r_pad=9, r_coff=5, **F32),
    dict(bbias_rows=50, **ALL), dict(r_f32=True, **ALL, **F32), dict(bbias_rows=50, r_f32=True, **ALL, **F32),
    dict(conv="c64", bias=True, **F32), dict(conv="c64", bias=True, R="sep", r_f32=True, **F32),   # conv, fp32 C: flavour 1; with a residual flavour 2
]


def _epilogue_cases():
    return [Case(cfg=cfg, **e) for e in EPILOGUES for cfg in (2, 0)]


def _splitk_cases():
    """dense K = 320: five K steps in slices of 2, 2, 1 (split-K 3) and 2, 2, 1, 0 (split-K 4: the empty slice's partials are zero and still summed)"""
    out = []
    for sk in (3, 4):
        for f32 in (False, True):
            fields = [dict(), dict(bbias_rows=50, r_f32=f32, **ALL), dict(act=KR.ACT_GELU, bias=True), dict(R="inplace", r_f32=f32), dict(N=130, bias=True, scale=True)]
            out += [Case(K=320, splitk=sk, c_f32=f32, cfg=(2, 0, 1, 3)[(i + sk) % 4], **{"N": 136, **e}) for i, e in enumerate(fields)]
    out += [Case(conv="c64", N=136, splitk=3, cfg=cfg, bias=True, act=KR.ACT_RELU) for cfg in (1, 2)]
    # a slice that starts inside the tap list is the only place where (ky, kx) comes from a division (later taps are reached by increments):
    # kh != kw with slices starting at taps 5, 10 / 3, 6, 9, 12, and the chunk-major order with slices starting at taps 6 and 3 of chunks 0 and 1
    out += [Case(conv="k3x5", N=136, splitk=3, cfg=2), Case(conv="k3x5", N=136, splitk=5, cfg=1, c_f32=True), Case(conv="c128cm", N=136, splitk=3, cfg=0)]
    return out


WALK_CASES, TILE_CASES, KTAIL_CASES, CONV_CASES = _walk_cases(), _tile_cases(), _ktail_cases(), _conv_cases()
EPILOGUE_CASES, SPLITK_CASES = _epilogue_cases(), _splitk_cases()
ALL_CASES = WALK_CASES + TILE_CASES + KTAIL_CASES + CONV_CASES + EPILOGUE_CASES + SPLITK_CASES


# ---- the persistent walk of gemm_bf16_kernel, restated ----
def xcd_run_start(xcd, n):
    q, r = n >> 3, n & 7
    return xcd * (q + 1) if xcd < r else r * (q + 1) + (xcd - r) * q


def tile_coords(tile, tilesM, tilesN):
    per_group = tilesM * 8
    g, r = divmod(tile, per_group)
    gw = min(8, tilesN - g * 8)
    return r // gw, g * 8 + r % gw


def walk(case):
    """-> one list of work ids per workgroup, in the order the workgroup visits them"""
    BM, BN = case.tile
    cfg = 0 if case.tile == (128, 128) else case.cfg
    total = -(-case.M // BM) * -(-case.N // BN) * case.splitk
    grid = min(total, case.cus * WG_PER_CU[cfg])
    out = []
    for b in range(grid):
        xcd = b & 7
        cs = xcd_run_start(xcd, total)
        end = cs + (total >> 3) + (1 if xcd < (total & 7) else 0)
        step = (grid - xcd + 7) >> 3
        out.append(list(range(cs + (b >> 3), end, step)))
    return out, total


# ---- 16-bit number formats ----
def to_s16(x, s16):
    """RNE to the storage type -> (values as float64, bit patterns as uint16)"""
    t = torch.from_numpy(np.ascontiguousarray(x, np.float32)).to(S16[s16][1])
    return t.double().numpy(), t.view(torch.int16).numpy().view(np.uint16)


def ulp16(x, s16):
    """the spacing of the storage type's numbers at |x| (of its subnormals below the smallest normal)"""
    p, emin = MANT[s16]
    x = np.abs(np.asarray(x, np.float64))
    e = np.where(x == 0, emin, np.frexp(x)[1] - 1)                            # |x| in [2^e, 2^(e+1))
    return np.ldexp(1.0, np.maximum(e, emin) - p)


def floor16(x, s16):
    """the largest number of the storage type <= x (float64 in and out; |x| below the type's largest)"""
    u = ulp16(x, s16)
    return np.floor(np.asarray(x, np.float64) / u) * u


def ceil16(x, s16):
    return -floor16(-np.asarray(x, np.float64), s16)


def ties(ref, s16):
    """how many elements of ref lie exactly halfway between two neighbouring numbers of the storage type"""
    lo, hi = floor16(ref, s16), ceil16(ref, s16)
    return int(((lo != hi) & (ref - lo == hi - ref)).sum())


# ---- host data ----
def _seed(case, s16, exact):
    return zlib.crc32(f"{case.id}-{s16}-{exact}".encode())


def _quarters(g, shape, lim):
    return (g.integers(-4 * lim, 4 * lim + 1, shape) / 4.0).astype(np.float32)


def _values(case, exact, g, shape, w=False):
    if not exact:
        return g.standard_normal(shape).astype(np.float32)
    if case.act == KR.ACT_GELU:                                                # |acc| <= 2 x 1 x 2
        if w:
            return g.integers(-2, 3, shape).astype(np.float32)
        keep = KR.keep_per_row(int(np.prod(shape[:-1])), shape[-1], 2, int(g.integers(1 << 30))).reshape(shape)
        return (g.integers(0, 2, shape) * 2.0 - 1.0).astype(np.float32) * keep
    return g.integers(0 if case.positive else -4, 5, shape).astype(np.float32)


@functools.lru_cache(maxsize=4)
def host(case, s16, exact):
    """every host array of one run of `case` in storage type `s16`: a_host (fp32 values of the array to upload, noise included), geo (the launch's
    A fields), a_rows / w (the fp64 values of the rounded operands the GEMM contracts), the epilogue's operands, pre (the fp64 value the
    activation is applied to) and ref (the fp64 reference [M, N])"""
    g = np.random.default_rng(_seed(case, s16, exact))
    M, N, K = case.M, case.N, case.K
    if case.conv:
        c = conv_geometry(case.conv)
        ld = c["Cin"] + MAP_PAD
        win = to_s16(_values(case, exact, g, (c["B"], c["H"], c["W"], c["Cin"])), s16)[0]
        a_host = (g.standard_normal((c["B"], c["H"], c["W"], ld)) * 1e3).astype(np.float32)
        a_host[..., c["coff"]:c["coff"] + c["Cin"]] = win
        a_rows, Ho, Wo = KR.im2col_nhwc(win, c["kh"], c["kw"], c["stride"], c["pad"], c["dil"])
        assert (Ho, Wo) == (c["Ho"], c["Wo"]) and a_rows.shape == (M, K)
        geo = dict(mode=1, lda=ld, a_coff=c["coff"], Hin=c["H"], Win=c["W"], Cin=c["Cin"], kh=c["kh"], kw=c["kw"], stride=c["stride"], pad=c["pad"],
                   dil=c["dil"], Hout=Ho, Wout=Wo)
    else:
        a_rows = to_s16(_values(case, exact, g, (M, K)), s16)[0]
        a_host = (g.standard_normal((M, K + A_PAD)) * 1e3).astype(np.float32)
        a_host[:, A_COFF:A_COFF + K] = a_rows
        geo = dict(mode=0, lda=K + A_PAD, a_coff=A_COFF)
    w = _values(case, exact, g, (N, K), w=True)
    if not exact:
        w = (w / np.sqrt(K)).astype(np.float32)
    w = to_s16(w, s16)[0]
    h = dict(a_host=a_host, geo=geo, a_rows=a_rows, w=w, bias=None, bbias=None, scale=None, shift=None, R=None)
    if case.bias:
        h["bias"] = _quarters(g, N, 1) if exact else (g.standard_normal(N) * 0.5).astype(np.float32)
    if case.bbias_rows:
        nb = (M + case.bbias_rows - 1) // case.bbias_rows
        h["bbias"] = _quarters(g, (nb, N), 1) if exact else (g.standard_normal((nb, N)) * 0.5).astype(np.float32)
    if case.scale:
        h["scale"] = g.choice(np.array([1.0, -1.0, 0.5, -0.5], np.float32), N) if exact else (1 + g.standard_normal(N) * 0.1).astype(np.float32)
        h["shift"] = _quarters(g, N, 1) if exact else (g.standard_normal(N) * 0.1).astype(np.float32)
    if case.R:
        r = _quarters(g, (M, N), 64 if case.r_f32 else 2) if exact else g.standard_normal((M, N)).astype(np.float32)
        h["R"] = r.astype(np.float64) if case.r_f32 else to_s16(r, s16)[0]       # what the kernel reads: a 16-bit residual is rounded first
    acc = a_rows @ w.T
    h["pre"] = KR.gemm_epilogue_ref(acc, h["bias"], h["bbias"], case.bbias_rows, h["scale"], h["shift"])
    h["ref"] = KR.gemm_epilogue_ref(acc, h["bias"], h["bbias"], case.bbias_rows, h["scale"], h["shift"], case.act, h["R"])
    return h


def assert_exact(case, s16):
    """the exactness conditions of the exact run of `case`; returns the largest |partial sum| bound"""
    h = host(case, s16, True)
    a, w = h["a_rows"], h["w"]
    assert (a == np.round(a)).all() and (w == np.round(w)).all() and np.abs(a).max() <= 4 and np.abs(w).max() <= 4
    assert (to_s16(a, "bf16")[0] == a).all() and (to_s16(a, "f16")[0] == a).all()
    top = (np.abs(a) @ np.abs(w).T).max()
    assert top <= 16 * case.K < 2 ** 24
    for name, lim in [("bias", 1), ("bbias", 1), ("shift", 1), ("R", 64 if case.r_f32 else 2)]:
        if h[name] is not None:
            v = np.asarray(h[name], np.float64)
            assert (v * 4 == np.round(v * 4)).all() and np.abs(v).max() <= lim, name
    if h["scale"] is not None:
        assert set(np.abs(h["scale"]).tolist()) <= {1.0, 0.5}
    # every epilogue step stays a multiple of 1/8 far below 2^24 / 8: exact in fp32 in any order
    assert top + 2 + 1 + 64 < 2 ** 20
    if case.act == KR.ACT_GELU:
        assert np.abs(h["pre"]).max() <= 6
    else:
        assert (h["ref"].astype(np.float32).astype(np.float64) == h["ref"]).all()
    return top
