"""conv_halo_kernel (kernels/gemm_conv_halo.h) through the GEMM harness: brn::launch_gemm with the plan forced to a 4-wave tile, which
launch_gemm_split routes to the halo-staged kernel for every 3x3 / stride 1 / pad 1 conv of the two-plane forms.  Cases, data and references:
conv_halo_cases.py (tiles that overhang both edges, a map smaller than a tile, two images in M, uneven and empty split-K slices, N = 64 / 16 /
50, bias + scale / shift + ReLU, a column window of the output, a separate residual; forms h2 and bf16x2 on plans 1 and 2).

Every case runs twice, as in test_gemm_forms_gpu.py.  On plane-exact data (exactness asserted on the CPU: test_conv_halo_cases_cpu.py) the
result must equal the fp64 reference bit for bit; with split-K so must every slice's partial sums, and those are the sums over the slice's
CHANNEL CHUNKS (all nine taps of channels [32 c0, 32 c1)), which only the chunk-major kernel produces.  On Gaussian data the result is
compared with the fp64 sum of exactly the plane products the kernel keeps, relative to max(1, max |ref|), under the bound of
test_gemm_forms_gpu.py's gemm_split_kernel family rule: 3 x the largest error measured on an MI355X over this case list, never above BOUND_CAP.

Measured on the MI355X (max over the cases, the KH_MAXERR lines this file prints; bound = 3 x):
    conv_halo_kernel       4.554e-07  (h2-cfg1-wide-sk1-N64)                        -> 1.37e-06

Outputs, residuals and split-K scratch are kernel_harness.Guarded: a write outside the buffer, outside the column window or on rows >= M
fails the test.  The map's channels outside the input window hold large finite noise."""
import numpy as np
import pytest
import torch

import conv_halo_cases as HC
import gemm_cases as GC
import gemm_harness as GH
import kernel_refs as KR
from kernel_harness import SENT32, Guarded, dev, report

pytestmark = pytest.mark.gpu

BOUND_CAP = 2e-5
MEASURED = 4.554e-07
TOL = 3 * MEASURED
R_PAD, R_COFF = 8, 4


def test_bound_is_within_the_cap():
    assert 0 < TOL <= BOUND_CAP


def slice_refs(case, h):
    """fp64 [S, M, N]: what slice s of the split-K scratch holds — the contraction over its channel chunks, all nine taps, before the epilogue
    (the fp16 pair's weight scale is that of the whole tensor)"""
    Cin, S = case.dims[3], case.splitk
    nch = Cin // 32
    per = (nch + S - 1) // S
    a, w = h["a_rows"].reshape(case.M, 9, Cin), h["w"].reshape(case.N, 9, Cin)
    ws = GC.w_scale_of(h["w"])
    out = np.zeros((S, case.M, case.N))
    for s in range(S):
        lo, hi = 32 * min(nch, s * per), 32 * min(nch, (s + 1) * per)
        if hi > lo:
            av = GC.split_planes(np.ascontiguousarray(a[:, :, lo:hi]).reshape(case.M, -1), case.form, GC.A_SCALE)[1]
            wv = GC.split_planes(np.ascontiguousarray(w[:, :, lo:hi]).reshape(case.N, -1), case.form, ws)[1]
            out[s] = KR.gemm_planes_ref(av, wv, KR.KEPT[case.form], 1.0 / (GC.A_SCALE * ws) if case.form == "h2" else 1.0)
    return out


def run_case(case, exact):
    h = HC.host(case, exact)
    M, N, K = case.M, case.N, case.K
    planes, h2 = GC.FORMS[case.form]
    wp = GH.pack_weights(h["w"], planes, h2)
    a = torch.from_numpy(h["a_host"]).cuda()
    ldc = N + case.c_pad
    C = Guarded((M + GC.C_ROWS_BEHIND, ldc), torch.float32)
    win = np.s_[:M, case.c_coff:case.c_coff + N]
    f = dict(A=a, W=wp["W"], C=C.t, M=M, N=N, K=K, mode=GH.CONV_NHWC, ldc=ldc, c_coff=case.c_coff, Wp=wp["Wp"], planes=planes, wp_rows=wp["wp_rows"],
             h2=h2, a_scale=GC.A_SCALE if h2 else 0.0, out_scale=1.0 / (GC.A_SCALE * wp["w_scale"]) if h2 else 0.0, act=case.act, cfg=case.cfg,
             splitk=case.splitk, **h["geo"])
    keep = [a]
    for name in ["bias", "scale", "shift"]:
        if h[name] is not None:
            f[name] = dev(h[name])
            keep.append(f[name])
    R = r_host = None
    if case.R:
        ldr = N + R_PAD
        r_host = (np.random.default_rng(7).standard_normal((M, ldr)) * 1e3).astype(np.float32)
        r_host[:, R_COFF:R_COFF + N] = h["R"]
        R = Guarded((M, ldr), torch.float32)
        R.t.copy_(torch.from_numpy(r_host))
        f.update(R=R.t, ldr=ldr, r_coff=R_COFF)
    ws = None
    if case.splitk > 1:
        ws = Guarded((case.splitk * M * N,), torch.float32)
        f["ws"] = ws.t
    rc = GH.launch(**f)
    assert rc == 0, f"launch_gemm returned hipError_t {rc}"

    C.assert_untouched_outside(win)
    if R is not None:
        R.assert_guards()
        assert (R.bits() == r_host.view(np.int32)).all(), "the residual was written"
    if ws is not None:
        ws.assert_guards()
        part = ws.bits().reshape(case.splitk, M, N)
        assert (part != SENT32).all(), "a split-K partial was never written"
        if exact:
            want = slice_refs(case, h).astype(np.float32)
            got_part = ws.t.cpu().numpy().reshape(case.splitk, M, N)
            assert (got_part == want).all(), "a slice's partial sums are not those of its channel chunks"
        if case.geo == "empty":
            assert (part[2] == 0).all(), "the empty slice's partials are not zero"
    got, ref = C.t[win].cpu().numpy(), h["ref"]
    assert got.shape == (M, N)
    if not exact:
        assert np.isfinite(got).all()
        return np.abs(got - ref).max() / max(1.0, np.abs(ref).max())
    ref32 = ref.astype(np.float32)
    bad = np.argwhere(~(got == ref32))
    assert bad.size == 0, (f"{len(bad)} of {got.size} elements differ from the exact reference, first (m, n) = {bad[0].tolist()}: "
                           f"{got[tuple(bad[0])]!r} vs {ref32[tuple(bad[0])]!r}")
    return 0.0


@pytest.mark.parametrize("case", HC.CASES, ids=lambda c: c.id)
def test_halo_conv(case):
    run_case(case, True)
    err = run_case(case, False)
    report("conv_halo_kernel", case.id, err)
    assert err <= TOL, f"{err:.3e} > {TOL:.3e}"


def test_same_call_twice_is_bit_identical():
    """no atomics, a fixed summation order: the Gaussian run of the split-K case repeated gives the same bits"""
    case = HC.CASES[6]
    assert case.splitk == 2
    h = HC.host(case, False)
    planes, h2 = GC.FORMS[case.form]
    wp = GH.pack_weights(h["w"], planes, h2)
    a = torch.from_numpy(h["a_host"]).cuda()
    outs = []
    for _ in range(2):
        C = torch.zeros((case.M, case.N), dtype=torch.float32, device="cuda")
        ws = torch.zeros((case.splitk * case.M * case.N,), dtype=torch.float32, device="cuda")
        rc = GH.launch(A=a, W=wp["W"], C=C, M=case.M, N=case.N, K=case.K, mode=GH.CONV_NHWC, ldc=case.N, Wp=wp["Wp"], planes=planes, wp_rows=wp["wp_rows"],
                       h2=h2, a_scale=GC.A_SCALE if h2 else 0.0, out_scale=1.0 / (GC.A_SCALE * wp["w_scale"]) if h2 else 0.0, cfg=case.cfg,
                       splitk=case.splitk, ws=ws, **h["geo"])
        assert rc == 0
        outs.append(C.cpu().numpy().view(np.int32))
    assert (outs[0] == outs[1]).all()
