"""The case table of test_gemm_forms_gpu.py, each case's host data (plane-exact or Gaussian) and its fp64 reference.  Numpy only:
test_gemm_refs_cpu.py asserts the exactness condition of every case without a GPU.

Plane-exact data (kernel_refs.plane_exact_values): at most NNZ non-zeros per contracted row of A, W dense, the epilogue's operands multiples
of 1/4 and its scales powers of two, so that every kept plane product, every partial sum in any order and every epilogue step is exact in fp32
(kernel_refs.assert_plane_exact) and the kernel must return the fp64 reference bit for bit."""
import functools
import zlib
from dataclasses import dataclass

import numpy as np

import kernel_refs as KR

FORMS = {"f32": (0, 0), "bf16x2": (2, 0), "bf16x3": (3, 0), "h2": (2, 1)}          # form -> (GemmParams::planes, GemmParams::h2)
A_SCALE = 2.0 ** 10          # the fp16 pair's activation scale: |a_scale x| stays below 65504 for every |x| < 63
NNZ = 20                     # non-zeros per dense row of plane-exact A: 20 x 1.004 + the epilogue's addends < 32 = 2^24 x 2^-19
A_PAD, A_COFF = 48, 16       # a dense fp32 A sits in columns [16, 16 + K) of rows K + 48 wide; the other columns hold noise
P_PAD = 16                   # floats of noise behind a P-layout A row (lda % 16 == 0)
C_ROWS_BEHIND = 2            # sentinel rows behind row M - 1 of every output


@dataclass(frozen=True)
class Case:
    form: str
    mode: str = "dense"      # dense | conv (3x3, pad 1, Cin = 32 inside a 96-channel map) | gather4 (3 -> N, 4x4 stride 4) | gather3 (3 -> N, 3x3 pad 1)
    M: int = 300
    N: int = 200
    K: int = 96
    cfg: int = 2
    splitk: int = 1
    bias: bool = False
    bbias_rows: int = 0
    scale: bool = False
    act: int = KR.ACT_NONE
    R: str = ""              # "" | sep | inplace
    r_pad: int = 0           # ldr = N + r_pad
    r_coff: int = 0
    c_pad: int = 0           # ldc = N + c_pad (logical columns)
    c_coff: int = 0
    a_planes: bool = False
    c_planes: bool = False

    @property
    def planes(self):
        return FORMS[self.form][0]

    @property
    def h2(self):
        return FORMS[self.form][1]

    @property
    def family(self):
        """the kernel family whose tolerance applies"""
        if self.form == "f32":
            return "gemm_f32_kernel"
        if self.c_planes:
            return "P output"
        return "gemm_split_kernel" if self.cfg in (1, 2) else "gemm_split_ws_kernel"

    @property
    def id(self):
        s = f"{self.form}-{self.mode}-cfg{self.cfg}-sk{self.splitk}-{self.M}x{self.N}x{self.K}"
        for flag, on in [("bias", self.bias), (f"bbias{self.bbias_rows}", self.bbias_rows), ("scale", self.scale), ("relu", self.act == KR.ACT_RELU),
                         ("gelu", self.act == KR.ACT_GELU), (f"R{self.R}+{self.r_pad}@{self.r_coff}", self.R), (f"C+{self.c_pad}@{self.c_coff}", self.c_pad or self.c_coff),
                         ("Pin", self.a_planes), ("Pout", self.c_planes)]:
            if on:
                s += "-" + flag
        return s


CONV = dict(mode="conv", K=288)
GATHER4 = dict(mode="gather4", K=64)
GATHER3 = dict(mode="gather3", K=32)


def _nsk(cfg):
    """N = 200 and N = 130 (N % 4 = 2: scalar stores), split-K 1 and 3, paired one way on even plans and the other way on odd ones"""
    return [(200, 1), (130, 3)] if cfg % 2 == 0 else [(200, 3), (130, 1)]


def _tile_cases():
    out = []
    for cfg in range(6):                                     # gemm_f32_kernel: every tile launch_gemm knows, 3 (never planned) and the 8-wave 4 / 5 included
        for geo in [{}, CONV, GATHER4]:
            out += [Case("f32", cfg=cfg, N=n, splitk=sk, **geo) for n, sk in _nsk(cfg)]
    out.append(Case("f32", cfg=2, N=130, **GATHER3))         # the per-element loader of the NCHW gather
    for form in ["bf16x2", "bf16x3", "h2"]:
        for cfg in [1, 2, 0]:                                # gemm_split_kernel 128x64 / 64x64, gemm_split_ws_kernel with 32-deep stages
            for geo in [{}, CONV]:
                out += [Case(form, cfg=cfg, N=n, splitk=sk, **geo) for n, sk in _nsk(cfg)]
    # the 16-deep three-plane stage: more than 256 workgroups (17 x 16 tiles; 6 x 7 tiles x 7 slices)
    out += [Case("bf16x3", M=2100, N=2048, K=64, cfg=0), Case("bf16x3", M=700, N=896, K=224, cfg=0, splitk=7)]
    # the same stage on implicit-GEMM rows: 3 x 16 tiles x 6 slices of three 16-deep K tiles
    out.append(Case("bf16x3", cfg=0, N=2048, splitk=6, **CONV))
    # an empty last slice: 25 K tiles in 6 slices of 5
    out += [Case(form, M=64, N=64, K=800, cfg=cfg, splitk=6) for form, cfg in [("f32", 2), ("bf16x2", 2), ("bf16x2", 0), ("bf16x3", 0)]]
    return out


def _p_cases():
    out = []
    for form in ["bf16x2", "h2"]:
        out += [Case(form, cfg=0, N=192, a_planes=True), Case(form, cfg=0, N=128, splitk=3, a_planes=True)]
    for form in ["bf16x2", "bf16x3", "h2"]:
        out += [Case(form, cfg=0, N=192, c_planes=True, c_pad=64, c_coff=32),
                Case(form, cfg=0, N=128, c_planes=True, c_pad=64, c_coff=32, bias=True, a_planes=form != "bf16x3")]
    return out


EPILOGUES = [dict(bias=True), dict(bbias_rows=50), dict(scale=True), dict(act=KR.ACT_RELU, bias=True), dict(act=KR.ACT_GELU, bias=True),
             dict(R="sep", r_pad=24, r_coff=8), dict(R="inplace"), dict(c_pad=64, c_coff=32), dict(c_pad=9, c_coff=3),
             dict(R="sep", r_pad=8, r_coff=5), dict(bias=True, bbias_rows=50, scale=True, act=KR.ACT_RELU, R="sep", r_pad=8, r_coff=4, c_pad=8, c_coff=4)]


def _epilogue_cases():
    return [Case(form, cfg=cfg, splitk=sk, **e) for e in EPILOGUES for form, cfg in [("h2", 2), ("bf16x2", 0)] for sk in [1, 3]]


TILE_CASES, P_CASES, EPILOGUE_CASES = _tile_cases(), _p_cases(), _epilogue_cases()
ALL_CASES = TILE_CASES + P_CASES + EPILOGUE_CASES
CHAIN = dict(M=300, K1=96, N1=128, N2=192)       # GEMM -> P layout -> GEMM (fc1 -> fc2), two planes of either type


def _seed(case, exact):
    return zlib.crc32(f"{case.id}-{exact}".encode())


def _quarters(g, shape, lim):
    return (g.integers(-4 * lim, 4 * lim + 1, shape) / 4.0).astype(np.float32)


def w_scale_of(w):
    """pack_half2_planes' scale: the power of two that puts max |w| in [2^13, 2^14)"""
    return float(2.0 ** (14 - np.frexp(np.abs(w).max())[1]))


def split_planes(x, form, s):
    """(bits, values) of the operand planes of fp32 x in `form`; s = the fp16 pair's scale"""
    return KR.split_h2(x, s) if form == "h2" else KR.split_bf16(x, FORMS[form][0])


def contraction_ref(a_rows, w, form, a_given=None):
    """fp64 [M, N] of exactly what the kernels of `form` sum; a_given = the values of A's planes when it arrives in the P layout"""
    if form == "f32":
        return a_rows.astype(np.float64) @ w.astype(np.float64).T
    ws = w_scale_of(w)
    av = split_planes(a_rows, form, A_SCALE)[1] if a_given is None else a_given
    wv = split_planes(w, form, ws)[1]
    return KR.gemm_planes_ref(av, wv, KR.KEPT[form], 1.0 / (A_SCALE * ws) if form == "h2" else 1.0)


def plane_rows(x, form):
    """fp32 [rows, K] -> the P-layout bytes [rows, 2 NP K] of its planes"""
    return KR.encode_planes(split_planes(x, form, A_SCALE)[0])


def _operand_a(case, exact, g):
    """-> (a_host: the array to upload, a_off: floats from its start to GemmParams::A, geometry fields, a_rows [M, K]: what the GEMM contracts)"""
    kind = case.form
    M, K = case.M, case.K

    def values(shape, density=None):
        if not exact:
            return g.standard_normal(shape).astype(np.float32)
        v = KR.plane_exact_values(shape, kind, int(g.integers(1 << 30)))
        return v * (g.random(shape) < density).astype(np.float32)

    if case.mode == "dense":
        a_rows = values((M, K)) if not exact else KR.plane_exact_values((M, K), kind, int(g.integers(1 << 30))) * KR.keep_per_row(M, K, NNZ, int(g.integers(1 << 30)))
        if case.a_planes:
            NP = case.planes
            lda = K * NP // 2 + P_PAD
            host = np.full((M, lda * 4), 0x41, np.uint8)                       # (bf16 / fp16 words 0x4141: finite noise behind the row)
            host[:, :K * 2 * NP] = plane_rows(a_rows, case.form)
            return host, 0, dict(lda=lda), a_rows
        lda = K + A_PAD
        host = (g.standard_normal((M, lda)) * 1e3).astype(np.float32)
        host[:, A_COFF:A_COFF + K] = a_rows
        return host, A_COFF, dict(lda=lda), a_rows
    if case.mode == "conv":
        B, H, W, Cin, ld, coff = 3, 10, 10, 32, 96, 32
        win = values((B, H, W, Cin), 0.06)
        host = (g.standard_normal((B, H, W, ld)) * 1e3).astype(np.float32)
        host[..., coff:coff + Cin] = win
        a_rows, Ho, Wo = KR.im2col_nhwc(win, 3, 3, 1, 1)
        geo = dict(lda=ld, a_coff=coff, Hin=H, Win=W, Cin=Cin, kh=3, kw=3, stride=1, pad=1, dil=1, Hout=Ho, Wout=Wo, Kreal=9 * Cin)
    else:
        k, stride, pad, H = (4, 4, 0, 40) if case.mode == "gather4" else (3, 1, 1, 10)
        host = values((3, 3, H, H), 0.4)
        a_rows, Ho, Wo = KR.im2col_nchw(host, k, k, stride, pad, K)
        geo = dict(lda=0, Hin=H, Win=H, Cin=3, kh=k, kw=k, stride=stride, pad=pad, dil=1, Hout=Ho, Wout=Wo, Kreal=3 * k * k)
    assert a_rows.shape == (M, K), (a_rows.shape, M, K)
    return host, 0, geo, a_rows


@functools.lru_cache(maxsize=4)
def host(case, exact):
    """every host array of one run of `case`: the operands as uploaded, the epilogue's, and `ref`, the fp64 reference [M, N]"""
    g = np.random.default_rng(_seed(case, exact))
    M, N, K = case.M, case.N, case.K
    a_host, a_off, geo, a_rows = _operand_a(case, exact, g)
    if exact:
        w = KR.plane_exact_values((N, K), case.form, int(g.integers(1 << 30)))
    else:
        w = (g.standard_normal((N, K)) / np.sqrt(K)).astype(np.float32)
    if case.mode.startswith("gather"):
        w[:, geo["Kreal"]:] = 0.0                                              # W's K padding is zero (GemmParams::W)
    h = dict(a_host=a_host, a_off=a_off, geo=geo, a_rows=a_rows, w=w, bias=None, bbias=None, scale=None, shift=None, R=None)
    if case.bias:
        h["bias"] = _quarters(g, N, 1) if exact else (g.standard_normal(N) * 0.5).astype(np.float32)
    if case.bbias_rows:
        nb = (M + case.bbias_rows - 1) // case.bbias_rows
        h["bbias"] = _quarters(g, (nb, N), 1) if exact else (g.standard_normal((nb, N)) * 0.5).astype(np.float32)
    if case.scale:
        h["scale"] = g.choice(np.array([1.0, -1.0, 0.5, -0.5], np.float32), N) if exact else (1 + g.standard_normal(N) * 0.1).astype(np.float32)
        h["shift"] = _quarters(g, N, 1) if exact else (g.standard_normal(N) * 0.1).astype(np.float32)
    if case.R:
        h["R"] = _quarters(g, (M, N), 2) if exact else g.standard_normal((M, N)).astype(np.float32)
    a_given = split_planes(a_rows, case.form, A_SCALE)[1] if case.a_planes else None
    acc = contraction_ref(a_rows, w, case.form, a_given)
    h["ref"] = KR.gemm_epilogue_ref(acc, h["bias"], h["bbias"], case.bbias_rows, h["scale"], h["shift"], case.act, h["R"])
    return h


def exactness_margin(case):
    """asserts the exactness condition of the plane-exact run of `case`; returns how much of the bound it uses"""
    h = host(case, True)
    return KR.assert_plane_exact(h["a_rows"], h["w"], case.form, addends=float(case.bias) + float(bool(case.bbias_rows)),
                                 scale_min=0.5 if case.scale else 1.0, post=float(case.scale) + 2.0 * bool(case.R))


@functools.lru_cache(maxsize=None)
def chain_host(form, exact):
    """fc1 -> fc2: C1 = epilogue(A1 W1^T) written in the P layout, C2 = C1 W2^T.  Plane-exact: W1 is a signed selection (row n = +-1 at column
    n % K1), so C1 holds A1's plane-exact values again — with at most NNZ x ceil(N1 / K1) non-zeros per row — and both GEMMs are exact.
    Gaussian: GELU after fc1, as in a Swin MLP.  The reference of fc2 contracts the planes of the fp32-rounded reference of fc1."""
    M, K1, N1, N2 = CHAIN["M"], CHAIN["K1"], CHAIN["N1"], CHAIN["N2"]
    g = np.random.default_rng(zlib.crc32(f"chain-{form}-{exact}".encode()))
    if exact:
        a1 = KR.plane_exact_values((M, K1), form, 1) * KR.keep_per_row(M, K1, NNZ, 2)
        w1 = np.zeros((N1, K1), np.float32)
        w1[np.arange(N1), np.arange(N1) % K1] = g.integers(0, 2, N1) * 2.0 - 1.0
        w2 = KR.plane_exact_values((N2, N1), form, 3)
        act = KR.ACT_NONE
    else:
        a1 = g.standard_normal((M, K1)).astype(np.float32)
        w1 = (g.standard_normal((N1, K1)) / np.sqrt(K1)).astype(np.float32)
        w2 = (g.standard_normal((N2, N1)) / np.sqrt(N1)).astype(np.float32)
        act = KR.ACT_GELU
    c1 = KR.gemm_epilogue_ref(contraction_ref(a1, w1, form), act=act).astype(np.float32)
    c1_bits, c1_vals = split_planes(c1, form, A_SCALE)
    if exact:
        KR.assert_plane_exact(a1, w1, form)
        KR.assert_plane_exact(c1, w2, form)
    return dict(a1=a1, w1=w1, w2=w2, act=act, c1=c1, c1_bits=c1_bits, ref=contraction_ref(c1, w2, form, c1_vals))
