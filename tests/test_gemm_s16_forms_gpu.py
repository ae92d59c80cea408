"""launch_gemm_bf16 (kernels/gemm_bf16.hip: gemm_bf16_kernel, splitk_reduce_bf16_kernel) through the 16-bit GEMM harness, in both builds (bf16 =
namespace brn, fp16 = brn::hf), with the tile, the split-K, the epilogue flavour and the size of the persistent grid forced: the persistent walk
on a grid of 8 CUs (every workgroup walks three or more work items: the next item's first K step issued under the previous item's epilogue, the
counted vmcnt wait, K loops of 1 .. 4 steps), every tile at the default grid dense and as implicit GEMM, the dense K tail, the conv form's
geometries on all four tiles (a 256-row tile over five and over six images: 49 pixels each), every epilogue field on the 32 x 32 and the 16 x 16 accumulator layout in flavours 0, 1 and 2, split-K with an
empty slice through the reduce kernel (convs too: a slice that starts inside the tap list is where (ky, kx) comes from a division), and the arguments launch_gemm_bf16 refuses.  The cases, their data and references: gemm_s16_cases.py.

Every case runs twice.  On exact data (small integers; the conditions are asserted on the CPU: test_gemm_s16_refs_cpu.py) every product, every
partial sum in any order and every epilogue step is exact in fp32: an fp32 C must equal the fp64 reference as numbers, a 16-bit C its
round-to-nearest-even rounding bit for bit (the sign of a zero is not compared); integer results above 256 (bf16) / 2048 (fp16) are exact ties of
that conversion.  GELU has no exact value: an fp32 output is held to the error documented at gelu_erf_as (6.1e-7) + half an fp32 ulp, a 16-bit
output to the documented error of the form its flavour uses (gelu_erf_bf16out in flavour 0: 3.0e-6) + half a 16-bit ulp of the reference.

On Gaussian data (A ~ N(0, 1), W ~ N(0, 1 / K), rounded to the storage type) the reference is the fp64 product of the rounded operands and the
epilogue in fp64.  An fp32 C is compared relative to max(1, max |ref|) under 3 x the largest error measured on an MI355X over the cases of its
group (the margin is for the fp32 accumulation order), never above BOUND_CAP = 2e-5, the bound test_linear_bf16_mode holds the same comparison to:
    flavour 1 (fp32 C, vector stores)   3.940e-07  (f16-c64-cfg1-sk1-300x200x576-f32)                  -> 1.18e-06
    flavour 2 (per element)             3.402e-07  (f16-c64-cfg0-sk1-300x130x576-f32)                  -> 1.02e-06
    split-K reduce                      1.609e-07  (bf16-dense-cfg3-sk3-300x130x320-f32-bias-scale)    -> 4.83e-07
(the KH_MAXERR lines this file prints).
A 16-bit C must lie within half a 16-bit ulp of the reference + t, t = that bound x max(1, max |ref|) (+ the documented GELU error), and
between the 16-bit numbers below ref - t and above ref + t: it is the rounding of an fp32 value within t of the reference.  (Flavour 0 sums as
flavour 1 does and takes its bound.)  Nothing of the 16-bit comparison is measured on the code under test beyond those three figures.

C, a separate residual and the split-K scratch are kernel_harness.Guarded; C is a column window of wider rows with sentinel rows behind row
M - 1: a write outside the window or on rows >= M fails the test, and so does a scratch element never written.  A's columns outside its window
(dense) and the map's channels outside the conv's window hold large finite noise."""
import numpy as np
import pytest
import torch

import gemm_s16_cases as GC
import gemm_s16_harness as GH
import kernel_refs as KR
from kernel_harness import SENT32, Guarded, dev, report

pytestmark = pytest.mark.gpu

BOUND_CAP = 2e-5
MEASURED = {"flavour 1": 3.940e-07, "flavour 2": 3.402e-07, "split-K reduce": 1.609e-07}
TOL = {k: 3 * v for k, v in MEASURED.items()}
HALF_ULP32 = 2.0 ** -24

ids = lambda c: c.id                                                                                      # noqa: E731
S16 = ["bf16", "f16"]


def test_bounds_are_within_the_cap():
    assert all(0 < t <= BOUND_CAP for t in TOL.values()), TOL


class Run:
    """one prepared launch of a case in one storage type: device operands, guarded outputs, the kh_launch_gemm_s16 fields"""

    def __init__(self, case, s16, exact):
        self.case, self.s16, self.exact = case, s16, exact
        self.h = h = GC.host(case, s16, exact)
        f16, dt = GC.S16[s16]
        M, N = case.M, case.N
        self.a = dev(h["a_host"], dt)
        if case.conv:
            c = GC.conv_geometry(case.conv)
            wp = GH.pack(h["w"], f16, *((0, 0) if c["cm"] is False else (c["kh"] * c["kw"], c["Cin"])))
            assert wp["k_chunk_major"] == int(c["cm"] is None and c["Cin"] % 64 == 0 and c["Cin"] > 64)
        else:
            wp = GH.pack(h["w"], f16)
        self.c_dt = torch.float32 if case.c_f32 else dt
        self.ldc = N + case.c_pad
        self.C = Guarded((M + GC.C_ROWS_BEHIND, self.ldc), self.c_dt)
        self.win = np.s_[:M, case.c_coff:case.c_coff + N]
        self.keep = [self.a, wp["Wp"]]                                 # (tensors whose pointers the launch holds)
        f = dict(f16=f16, A=self.a, C=self.C.t, M=M, N=N, K=case.K, ldc=self.ldc, c_coff=case.c_coff, act=case.act, c_f32=int(case.c_f32),
                 r_f32=int(case.r_f32), bbias_rows=case.bbias_rows or 1, cfg=case.cfg, splitk=case.splitk, launch_cus=case.cus, **wp, **h["geo"])
        for name in ["bias", "bbias", "scale", "shift"]:
            if h[name] is not None:
                f[name] = dev(h[name])
                self.keep.append(f[name])
        self.R = self.r_bits = None
        r_dt = torch.float32 if case.r_f32 else dt
        if case.R == "sep":
            r_host = (np.random.default_rng(7).standard_normal((M, case.ldr)) * 1e3).astype(np.float32)
            r_host[:, case.r_coff:case.r_coff + N] = h["R"]
            self.R = Guarded((M, case.ldr), r_dt)
            self.R.t.copy_(dev(r_host, r_dt))
            self.r_bits = self.R.bits().copy()
            f.update(R=self.R.t, ldr=case.ldr, r_coff=case.r_coff)
        elif case.R == "inplace":
            assert r_dt == self.c_dt
            self.C.t[self.win] = dev(h["R"], r_dt)
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
            assert (self.R.bits() == self.r_bits).all(), "the residual was written"
        if self.ws is not None:
            self.ws.assert_guards()
            part = self.ws.bits().reshape(case.splitk, case.M, case.N)
            assert (part != SENT32).all(), "a split-K partial was never written"
            if case.splitk == 4 and case.K == 320:                     # slice 3 of 4 starts at K step 6 of 5: empty, and still read by the reduction
                assert (part[3] == 0).all(), "the empty slice's partials are not zero"

    def compare(self):
        """asserts the exact run's comparison; for a Gaussian run asserts the 16-bit conditions / returns the fp32 error relative to max(1, max |ref|)"""
        case, s16, ref = self.case, self.s16, self.h["ref"]
        got_t = self.C.t[self.win].contiguous()
        got = got_t.double().cpu().numpy()
        assert got.shape == (case.M, case.N)
        gelu = case.act == KR.ACT_GELU

        def none_bad(bad, what):
            bad = np.argwhere(bad)
            assert bad.size == 0, (f"{len(bad)} of {got.size} elements {what}, first (m, n) = {bad[0].tolist()}: "
                                   f"{got[tuple(bad[0])]!r} vs {ref[tuple(bad[0])]!r}")

        if self.exact:
            if gelu:
                half = HALF_ULP32 * np.abs(ref) if case.c_f32 else GC.ulp16(ref, s16) / 2
                none_bad(~(np.abs(got - ref) <= case.gelu_abs + half), "beyond the documented GELU error")
            elif case.c_f32:
                none_bad(~(got == ref), "differ from the exact reference")
            else:
                got_bits = got_t.view(torch.int16).cpu().numpy().view(np.uint16)
                want_bits = GC.to_s16(ref, s16)[1]
                none_bad((got_bits != want_bits) & ~((got == 0) & (ref == 0)), "are not the RNE rounding of the exact reference")
            return 0.0
        assert np.isfinite(got).all()
        top = max(1.0, np.abs(ref).max())
        if case.c_f32:
            return np.abs(got - ref).max() / top
        t = TOL[case.group] * top + (case.gelu_abs if gelu else 0.0)
        none_bad(~(np.abs(got - ref) <= GC.ulp16(ref, s16) / 2 + t), "beyond half a 16-bit ulp + the fp32 bound")
        none_bad(~((GC.floor16(ref - t, s16) <= got) & (got <= GC.ceil16(ref + t, s16))), "are no 16-bit neighbour of the reference")
        return None


def run_case(case, s16, exact):
    r = Run(case, s16, exact)
    rc = r.launch()
    assert rc == 0, f"launch_gemm_bf16 returned hipError_t {rc}"
    r.check_buffers()
    return r.compare()


def both_runs(case, s16):
    run_case(case, s16, True)
    err = run_case(case, s16, False)
    if err is not None:
        report(case.group.replace(" ", "_"), f"{s16}-{case.id}", err)
        assert err <= TOL[case.group], f"{err:.3e} > {TOL[case.group]:.3e}"


def cases(table):
    return pytest.mark.parametrize("case", table, ids=ids)


s16s = pytest.mark.parametrize("s16", S16)


@s16s
@cases(GC.WALK_CASES)
def test_persistent_walk(case, s16):
    both_runs(case, s16)


@s16s
@cases(GC.TILE_CASES)
def test_tiles_at_the_default_grid(case, s16):
    both_runs(case, s16)


@s16s
@cases(GC.KTAIL_CASES)
def test_dense_k_tail(case, s16):
    both_runs(case, s16)


@s16s
@cases(GC.CONV_CASES)
def test_conv_form(case, s16):
    both_runs(case, s16)


@s16s
@cases(GC.EPILOGUE_CASES)
def test_epilogue_fields(case, s16):
    both_runs(case, s16)


@s16s
@cases(GC.SPLITK_CASES)
def test_splitk_reduce(case, s16):
    both_runs(case, s16)


DENSE, CONV, CONV96 = GC.Case(cfg=0), GC.Case(conv="c64", N=136, cfg=0), GC.Case(conv="c96", N=136, cfg=0)
REFUSALS = [
    ("K % 32", DENSE, dict(K=80)),
    ("lda % 8", DENSE, dict(lda=128 + GC.A_PAD + 4)),
    ("a_coff % 8", DENSE, dict(a_coff=4)),
    ("wp_ld too short", DENSE, dict(wp_ld=64)),
    ("wp_ld % 8", DENSE, dict(wp_ld=132)),
    ("conv, Cin % 32", CONV, dict(Cin=80, K=720)),
    ("conv, Cin < 64", CONV, dict(Cin=32, K=288)),
    ("conv, K != kh kw Cin", CONV, dict(K=512)),
    ("chunk-major on a dense launch", DENSE, dict(k_chunk_major=1)),
    ("chunk-major with Cin % 64", CONV96, dict(k_chunk_major=1)),
    ("mode = GEMM_GATHER_NCHW", CONV, dict(mode=GH.GATHER_NCHW)),
    ("split-K without scratch", GC.Case(cfg=0, K=320, splitk=3), dict(ws=None)),
    ("cfg 3 at N = 512", GC.Case(N=512, cfg=3), {}),
    ("wp_rows below the tile's padding", GC.Case(cfg=2), dict(wp_rows=200)),
]


@s16s
@pytest.mark.parametrize("why,case,override", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_refusals_never_launch(why, case, override, s16):
    r = Run(case, s16, True)
    assert r.launch(**override) == GH.INVALID_VALUE, why
    r.C.assert_untouched_outside(None)
    if r.ws is not None:
        r.ws.assert_untouched_outside(None)
