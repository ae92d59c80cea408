"""The case table of test_conv_halo_gpu.py (conv_halo_kernel, kernels/gemm_conv_halo.h: the halo-staged 3x3 implicit GEMM of the two-plane
modes), each case's host data (plane-exact or Gaussian) and its fp64 reference, in the style of gemm_cases.py.  Numpy only:
test_conv_halo_cases_cpu.py asserts the exactness condition of every case without a GPU.

The geometries are the smallest at which the kernel can still go wrong (a workgroup's tile is 8 x 16 output pixels of one image, a K step is
one tap of one 32-channel chunk, split-K slices are ranges of chunks):
    wide    B = 2, 11 x 19 map, Cin = 64 in columns [32, 96) of a 128-channel map: tiles overhang both edges, the image boundary falls inside
            M, and with two chunks the chunk-major K order differs from W's (tap, channel) order
    small   B = 2, 5 x 7 map, Cin = 32: narrower and lower than one tile
    uneven  9 x 17 map, Cin = 96, split-K 2: slices of two chunks and of one
    empty   9 x 17 map, Cin = 64, split-K 3: slices of one chunk, the third is empty and still writes zero partials
Plane-exact data is sparse: with DENSITY non-zeros per im2col row on average no row holds more than gemm_cases.NNZ (asserted), so every
partial sum in any order is exact."""
import functools
import zlib
from dataclasses import dataclass

import numpy as np

import gemm_cases as GC
import kernel_refs as KR

DENSITY = 6.0                # mean non-zeros per (interior) im2col row of plane-exact A

GEOMETRIES = {               # name -> B, H, W, Cin, floats per pixel, first channel of the window
    "wide": (2, 11, 19, 64, 128, 32),
    "small": (2, 5, 7, 32, 32, 0),
    "uneven": (1, 9, 17, 96, 96, 0),
    "empty": (1, 9, 17, 64, 64, 0),
}
SPLITK = {"wide": 1, "small": 1, "uneven": 2, "empty": 3}


@dataclass(frozen=True)
class Case:
    form: str                # h2 | bf16x2
    cfg: int                 # the plan's 4-wave tile: 1 (128 x 64) or 2 (64 x 64); both are routed to the halo kernel
    geo: str
    N: int
    bias: bool = False
    scale: bool = False
    act: int = KR.ACT_NONE
    R: bool = False          # a separate residual, ldr = N + 8, r_coff = 4
    c_pad: int = 0           # ldc = N + c_pad
    c_coff: int = 0

    @property
    def dims(self):
        return GEOMETRIES[self.geo]

    @property
    def M(self):
        B, H, W = self.dims[:3]
        return B * H * W

    @property
    def K(self):
        return 9 * self.dims[3]

    @property
    def splitk(self):
        return SPLITK[self.geo]

    @property
    def id(self):
        s = f"{self.form}-cfg{self.cfg}-{self.geo}-sk{self.splitk}-N{self.N}"
        for flag, on in [("bias", self.bias), ("scale", self.scale), ("relu", self.act == KR.ACT_RELU), ("R", self.R), (f"C+{self.c_pad}@{self.c_coff}", self.c_pad or self.c_coff)]:
            if on:
                s += "-" + flag
        return s


BSR = dict(bias=True, scale=True, act=KR.ACT_RELU)       # bias + scale / shift + ReLU
WIN = dict(c_pad=8, c_coff=4)                            # a column window of a wider output map
CASES = [
    Case("h2", 1, "wide", 64),
    Case("bf16x2", 2, "wide", 50, **BSR),
    Case("h2", 2, "wide", 16, **WIN),
    Case("bf16x2", 1, "wide", 64, R=True),
    Case("h2", 2, "small", 16),
    Case("bf16x2", 1, "small", 50, **BSR),
    Case("h2", 1, "uneven", 64, R=True),
    Case("bf16x2", 2, "uneven", 16, **WIN),
    Case("h2", 2, "empty", 50, **BSR),
    Case("bf16x2", 1, "empty", 64),
]


@functools.lru_cache(maxsize=4)
def host(case, exact):
    """every host array of one run of `case`: the map as uploaded, the im2col rows, the epilogue's operands and `ref`, the fp64 reference [M, N]"""
    g = np.random.default_rng(zlib.crc32(f"halo-{case.id}-{exact}".encode()))
    B, H, W, Cin, ld, coff = case.dims
    N, K = case.N, case.K
    if exact:
        win = KR.plane_exact_values((B, H, W, Cin), case.form, int(g.integers(1 << 30))) * (g.random((B, H, W, Cin)) < DENSITY / K).astype(np.float32)
        w = KR.plane_exact_values((N, K), case.form, int(g.integers(1 << 30)))
    else:
        win = g.standard_normal((B, H, W, Cin)).astype(np.float32)
        w = (g.standard_normal((N, K)) / np.sqrt(K)).astype(np.float32)
    a_host = (g.standard_normal((B, H, W, ld)) * 1e3).astype(np.float32)          # finite noise outside the window
    a_host[..., coff:coff + Cin] = win
    a_rows, Ho, Wo = KR.im2col_nhwc(win, 3, 3, 1, 1)
    assert (Ho, Wo) == (H, W) and a_rows.shape == (case.M, K)
    geo = dict(lda=ld, a_coff=coff, Hin=H, Win=W, Cin=Cin, kh=3, kw=3, stride=1, pad=1, dil=1, Hout=H, Wout=W, Kreal=K)
    h = dict(a_host=a_host, geo=geo, a_rows=a_rows, w=w, bias=None, scale=None, shift=None, R=None)
    if case.bias:
        h["bias"] = GC._quarters(g, N, 1) if exact else (g.standard_normal(N) * 0.5).astype(np.float32)
    if case.scale:
        h["scale"] = g.choice(np.array([1.0, -1.0, 0.5, -0.5], np.float32), N) if exact else (1 + g.standard_normal(N) * 0.1).astype(np.float32)
        h["shift"] = GC._quarters(g, N, 1) if exact else (g.standard_normal(N) * 0.1).astype(np.float32)
    if case.R:
        h["R"] = GC._quarters(g, (case.M, N), 2) if exact else g.standard_normal((case.M, N)).astype(np.float32)
    acc = GC.contraction_ref(a_rows, w, case.form)
    h["ref"] = KR.gemm_epilogue_ref(acc, h["bias"], None, 0, h["scale"], h["shift"], case.act, h["R"])
    return h


def exactness_margin(case):
    """asserts the exactness condition of the plane-exact run of `case`; returns how much of the bound it uses"""
    h = host(case, True)
    nnz = int((h["a_rows"] != 0).sum(1).max())
    assert 0 < nnz <= GC.NNZ, f"{nnz} non-zeros in an im2col row"
    return KR.assert_plane_exact(h["a_rows"], h["w"], case.form, addends=float(case.bias), scale_min=0.5 if case.scale else 1.0,
                                 post=float(case.scale) + 2.0 * case.R)
