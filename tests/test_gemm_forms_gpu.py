"""brn::launch_gemm (kernels/gemm_f32.hip, kernels/gemm_split.hip, the epilogue of kernels/gemm_common.h) through the GEMM harness, with the
tile, the split-K and every GemmParams field forced: each tile of the fp32 and the split kernels in each A mode, the 16-deep three-plane
stage, empty split-K slices, A and C in the P layouts, every epilogue field on a register-staged and on the warp-specialised kernel with and
without the split-K reduction, and the arguments launch_gemm refuses.  The cases, their data and references: gemm_cases.py.

Every case runs twice.  On plane-exact data every kept plane product, every partial sum in any order and every epilogue step is exact in
fp32 (asserted on the CPU: test_gemm_refs_cpu.py), so the result must equal the fp64 reference bit for bit whatever the tile, ring depth or
split-K (as numbers for fp32 outputs — the sign of a zero is not compared —, as bits for P-layout outputs).  GELU has no exact fp32 value: its
plane-exact run is held to the error documented at gelu_erf (gemm_common.h): 4.9e-7 + half an ulp of the result.  On Gaussian data the result
is compared with kernel_refs.gemm_planes_ref — the fp64 sum of exactly the plane products the kernel keeps (fp64 of the fp32 operands for the
fp32 kernel) — relative to max(1, max |ref|), under a bound of 3 x the largest error measured on an MI355X over the case list per kernel
family (the margin is for the fp32 accumulation order, which varies with tile and split-K), never above BOUND_CAP = 2e-5.

Measured on the MI355X (max over the cases of each family, the KH_MAXERR lines this file prints; bound = 3 x):
    gemm_f32_kernel        6.771e-07  (f32-conv-cfg3-sk1-300x130x288)               -> 2.03e-06
    gemm_split_kernel      5.455e-07  (bf16x3-conv-cfg1-sk1-300x130x288)            -> 1.64e-06
    gemm_split_ws_kernel   4.595e-07  (bf16x3-conv-cfg0-sk1-300x200x288)            -> 1.38e-06
    P output               6.466e-06  (bf16x2-dense-cfg0-sk1-300x192x96-C+64@32)    -> 1.94e-05
The P-output figure is the two-plane format itself: where the fp32 value differs from the reference in its last bits the middle plane can
round the other way, one ulp of it = 2^-17 of the value (three planes: 3.093e-07, the fp16 pair: 1.992e-07).  The fc1 -> fc2 chain hands its
intermediate over in that layout and is held to the same bound (measured 2.794e-06 with bf16 planes, 3.348e-07 with the fp16 pair).

Outputs, in-place residuals, separate residuals and split-K scratch are kernel_harness.Guarded: a write outside the buffer, outside the
column window or on rows >= M fails the test.  A's columns outside its window, and the bytes behind a P-layout row, hold finite noise."""
import numpy as np
import pytest
import torch

import gemm_cases as GC
import gemm_harness as GH
import kernel_refs as KR
from kernel_harness import SENT32, Guarded, dev, report

pytestmark = pytest.mark.gpu

BOUND_CAP = 2e-5
MEASURED = {"gemm_f32_kernel": 6.771e-07, "gemm_split_kernel": 5.455e-07, "gemm_split_ws_kernel": 4.595e-07, "P output": 6.466e-06}
TOL = {k: 3 * v for k, v in MEASURED.items()}
GELU_ABS, HALF_ULP = 4.9e-7, 2.0 ** -24

MODE = {"dense": GH.DENSE, "conv": GH.CONV_NHWC, "gather4": GH.GATHER_NCHW, "gather3": GH.GATHER_NCHW}
ids = lambda c: c.id                                                                                      # noqa: E731


def test_bounds_are_within_the_cap():
    assert all(0 < t <= BOUND_CAP for t in TOL.values()), TOL


class Run:
    """one prepared launch of a case: device operands, guarded outputs, the kh_launch_gemm fields"""

    def __init__(self, case, exact):
        self.case, self.exact = case, exact
        self.h = h = GC.host(case, exact)
        M, N, K = case.M, case.N, case.K
        planes, h2 = GC.FORMS[case.form]
        self.wp = wp = GH.pack_weights(h["w"], planes, h2)
        if h2:
            assert wp["w_scale"] == GC.w_scale_of(h["w"])
        self.a = torch.from_numpy(h["a_host"]).cuda()
        cw = planes if case.c_planes else 2                       # 16-bit words per logical column of C: a P3 row is 1.5 x as long
        self.ldc, lo, hi = (N + case.c_pad) * cw // 2, case.c_coff * cw // 2, (case.c_coff + N) * cw // 2
        self.C = Guarded((M + GC.C_ROWS_BEHIND, self.ldc), torch.float32)
        self.win = np.s_[:M, lo:hi]
        self.keep = [self.a]                                      # (tensors whose pointers the launch holds)
        f = dict(A=self.a.data_ptr() + 4 * h["a_off"], W=wp["W"], C=self.C.t, M=M, N=N, K=K, mode=MODE[case.mode], ldc=self.ldc, c_coff=case.c_coff,
                 Wp=wp["Wp"], planes=planes, wp_rows=wp["wp_rows"], a_planes=planes if case.a_planes else 0, c_planes=planes if case.c_planes else 0,
                 h2=h2, a_scale=GC.A_SCALE if h2 else 0.0, out_scale=1.0 / (GC.A_SCALE * wp["w_scale"]) if h2 else 0.0, act=case.act,
                 bbias_rows=case.bbias_rows, cfg=case.cfg, splitk=case.splitk, **h["geo"])
        for name in ["bias", "bbias", "scale", "shift"]:
            if h[name] is not None:
                f[name] = dev(h[name])
                self.keep.append(f[name])
        self.R = self.r_host = None
        if case.R == "sep":
            ldr = N + case.r_pad
            self.r_host = (np.random.default_rng(7).standard_normal((M, ldr)) * 1e3).astype(np.float32)
            self.r_host[:, case.r_coff:case.r_coff + N] = h["R"]
            self.R = Guarded((M, ldr), torch.float32)
            self.R.t.copy_(torch.from_numpy(self.r_host))
            f.update(R=self.R.t, ldr=ldr, r_coff=case.r_coff)
        elif case.R == "inplace":
            self.C.t[:M, lo:hi] = torch.from_numpy(h["R"]).cuda()
            f.update(R=self.C.t, ldr=self.ldc, r_coff=case.c_coff)
        self.ws = None
        if case.splitk > 1:
            self.ws = Guarded((case.splitk * M * N,), torch.float32)
            f["ws"] = self.ws.t
        self.fields = f

    def launch(self, **override):
        return GH.launch(**{**self.fields, **override})

    def check_buffers(self):
        case = self.case
        self.C.assert_untouched_outside(self.win)
        if self.R is not None:
            self.R.assert_guards()
            assert (self.R.bits() == self.r_host.view(np.int32)).all(), "the residual was written"
        if self.ws is not None:
            self.ws.assert_guards()
            part = self.ws.bits().reshape(case.splitk, case.M, case.N)
            assert (part != SENT32).all(), "a split-K partial was never written"
            if case.K == 800:                                     # slice 5 of 6 starts at K tile 25 of 25: empty, and still read by the reduction
                assert (part[5] == 0).all(), "the empty slice's partials are not zero"

    def compare(self):
        """the exact run's comparison, or the Gaussian run's error relative to max(1, max |ref|)"""
        case, ref = self.case, self.h["ref"]
        M = case.M
        ref32 = ref.astype(np.float32)
        if case.c_planes:
            raw = self.C.t[self.win].contiguous().view(torch.uint8).cpu().numpy()
            got_bits = KR.decode_planes(raw, case.planes)
            want_bits, want_vals = GC.split_planes(ref32, case.form, GC.A_SCALE)
            if self.exact:
                bad = np.argwhere(got_bits != want_bits)
                assert bad.size == 0, f"{len(bad)} plane words differ, first (plane, m, n) = {bad[0].tolist()}"
                return 0.0
            s = GC.A_SCALE if case.h2 else 1.0
            got = (KR.f16_bits_to_f64(got_bits) if case.h2 else KR.bf16_bits_to_f64(got_bits)).sum(0) / s
            want = want_vals.astype(np.float64).sum(0) / s
            return np.abs(got - want).max() / max(1.0, np.abs(want).max())
        got = self.C.t[self.win].cpu().numpy()
        assert got.shape == (M, case.N)
        if not self.exact:
            assert np.isfinite(got).all()
            return np.abs(got - ref).max() / max(1.0, np.abs(ref).max())
        if case.act == KR.ACT_GELU:
            bad = np.argwhere(~(np.abs(got - ref) <= GELU_ABS + HALF_ULP * np.abs(ref)))
        else:
            bad = np.argwhere(~(got == ref32))
        assert bad.size == 0, (f"{len(bad)} of {got.size} elements differ from the exact reference, first (m, n) = {bad[0].tolist()}: "
                               f"{got[tuple(bad[0])]!r} vs {ref32[tuple(bad[0])]!r}")
        return 0.0


def run_case(case, exact):
    r = Run(case, exact)
    rc = r.launch()
    assert rc == 0, f"launch_gemm returned hipError_t {rc}"
    r.check_buffers()
    return r.compare()


def both_runs(case):
    run_case(case, True)
    err = run_case(case, False)
    report(case.family.replace(" ", "_"), case.id, err)
    assert err <= TOL[case.family], f"{err:.3e} > {TOL[case.family]:.3e}"


@pytest.mark.parametrize("case", GC.TILE_CASES, ids=ids)
def test_tiles_and_kernels(case):
    both_runs(case)


@pytest.mark.parametrize("case", GC.P_CASES, ids=ids)
def test_p_layouts(case):
    both_runs(case)


@pytest.mark.parametrize("case", GC.EPILOGUE_CASES, ids=ids)
def test_epilogue_fields(case):
    both_runs(case)


@pytest.mark.parametrize("form", ["bf16x2", "h2"])
def test_chain_through_the_p_layout(form):
    """fc1 -> fc2: the first GEMM writes the P layout, the second reads it; both on the warp-specialised kernel"""
    M, K1, N1, N2 = (GC.CHAIN[k] for k in ["M", "K1", "N1", "N2"])
    planes, h2 = GC.FORMS[form]
    for exact in [True, False]:
        h = GC.chain_host(form, exact)
        w1, w2 = GH.pack_weights(h["w1"], planes, h2), GH.pack_weights(h["w2"], planes, h2)
        a1 = dev(h["a1"])
        c1, c2 = Guarded((M + 2, N1), torch.float32), Guarded((M + 2, N2), torch.float32)
        common = dict(M=M, mode=GH.DENSE, planes=planes, h2=h2, a_scale=GC.A_SCALE if h2 else 0.0, cfg=0, splitk=1)
        rc = GH.launch(A=a1, W=w1["W"], Wp=w1["Wp"], wp_rows=w1["wp_rows"], C=c1.t, N=N1, K=K1, lda=K1, ldc=N1, c_planes=planes, act=h["act"],
                       out_scale=1.0 / (GC.A_SCALE * w1["w_scale"]) if h2 else 0.0, **common)
        assert rc == 0
        rc = GH.launch(A=c1.t, W=w2["W"], Wp=w2["Wp"], wp_rows=w2["wp_rows"], C=c2.t, N=N2, K=N1, lda=N1, ldc=N2, a_planes=planes,
                       out_scale=1.0 / (GC.A_SCALE * w2["w_scale"]) if h2 else 0.0, **common)
        assert rc == 0
        c1.assert_untouched_outside(np.s_[:M])
        c2.assert_untouched_outside(np.s_[:M])
        got, ref = c2.t[:M].cpu().numpy(), h["ref"]
        if exact:
            mid = KR.decode_planes(c1.t[:M].contiguous().view(torch.uint8).cpu().numpy(), planes)
            assert (mid == h["c1_bits"]).all(), "the P-layout hand-over differs from the planes of the exact fc1 result"
            assert (got == ref.astype(np.float32)).all()
        else:
            err = np.abs(got - ref).max() / max(1.0, np.abs(ref).max())
            report("P_output", f"chain-{form}", err)
            assert err <= TOL["P output"], f"{err:.3e}"


REFUSALS = [
    ("K % 32", GC.Case("bf16x2", cfg=0), dict(K=80)),
    ("K % 32, fp32 kernel", GC.Case("f32", cfg=2), dict(K=80)),
    ("A in the P layout on a 4-wave tile", GC.Case("bf16x2", cfg=1, N=192, a_planes=True), {}),
    ("C in the P layout on a 4-wave tile", GC.Case("bf16x2", cfg=2, N=192, c_planes=True, c_pad=64, c_coff=32), {}),
    ("C in the P layout with split-K", GC.Case("bf16x2", cfg=0, N=192, c_planes=True, c_pad=64, c_coff=32, splitk=3), {}),
    ("C in the P layout with a residual", GC.Case("bf16x2", cfg=0, N=192, c_planes=True, c_pad=64, c_coff=32, R="sep"), {}),
    ("C in the P layout, N % 32", GC.Case("bf16x2", cfg=0, N=200, c_planes=True, c_pad=56, c_coff=32), {}),
    ("C in the P layout, c_coff % 32", GC.Case("bf16x2", cfg=0, N=192, c_planes=True, c_pad=64, c_coff=16), {}),
    ("C as the fp16 pair with split-K", GC.Case("h2", cfg=0, N=192, c_planes=True, c_pad=64, c_coff=32, splitk=3), {}),
    ("A in three planes", GC.Case("bf16x3", cfg=0, N=192, a_planes=True), {}),
    ("a 16-bit map with split-K", GC.Case("f32", cfg=2, splitk=3), dict(c_bf16=1)),
]


@pytest.mark.parametrize("why,case,override", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_refusals_never_launch(why, case, override):
    r = Run(case, True)
    assert r.launch(**override) == GH.INVALID_VALUE, why
    r.C.assert_untouched_outside(None)
    if r.ws is not None:
        r.ws.assert_untouched_outside(None)
