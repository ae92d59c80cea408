"""GEMM -> LayerNorm with the split-K slices summed by the LayerNorm (GemmPlan::raw + LayerNormParams::part), through tests/gemm_ln_harness.

Pairs: M = 130 (a full and a ragged 128-row tile), N = 192 / 768 / 1536 (1, 3, 6 float4 per lane), K = 288 = 9 K tiles in S = 2 slices (5 + 4)
and S = 4 (3 + 3 + 3 + 0: the last slice has no K tile and contributes zeros), on the warp-specialised kernel, in the three operand forms of
the split modes: the fp16 pair (A in the P2 layout, y written as fp16 planes), two bf16 planes (P2 in, P2 out), three bf16 planes (fp32 in
and out).  Each with bias + residual in place, bias + separate residual, bias only, residual only, neither.  x_out sits in columns [4, 4 + N)
of rows N + 8 wide, y in columns [32, 32 + N) of rows N + 64 wide; every output is kernel_harness.Guarded.

 * The fused pair must equal launch_gemm with the same S (and its reduce pass) followed by launch_layernorm bit for bit, in x_out and in y:
   the LayerNorm sums in the reduce pass's operand order.
 * Against fp64 (the sum of the plane products the kernel keeps, + bias, + residual, LayerNorm) the pair is held to the bounds
   test_gemm_forms_gpu.py applies: x_out and an fp32 y to the warp-specialised kernel's, a P-layout y to "P output"; relative to
   max(1, max |ref|) like there.  The operands, their references and those bounds are that file's and gemm_cases.py's own."""
import functools

import numpy as np
import pytest
import torch

import gemm_cases as GC
import gemm_ln_harness as LH
import kernel_refs as KR
import test_gemm_forms_gpu as TG
from kernel_harness import SENT32, Guarded, dev, report, rnd

pytestmark = pytest.mark.gpu

M, K = 130, 288
Y_PAD, Y_COFF = 64, 32
EPILOGUES = [(True, "inplace"), (True, "sep"), (True, ""), (False, "sep"), (False, "")]
SHAPES = [(form, N, S) for form in ("h2", "bf16x2", "bf16x3") for N in (192, 768, 1536) for S in (2, 4)]


def case_of(form, N, S, bias, R):
    return GC.Case(form, M=M, N=N, K=K, cfg=0, splitk=S, bias=bias, R=R, r_pad=8 if R == "sep" else 0, r_coff=4 if R == "sep" else 0, c_pad=8, c_coff=4,
                   a_planes=form != "bf16x3")


def y_form(form):
    """(y_planes, y_h2) of the LayerNorm output that feeds a GEMM of `form`"""
    return {"h2": (2, GC.A_SCALE), "bf16x2": (2, 0.0), "bf16x3": (0, 0.0)}[form]


def ln_fields(case, y, gamma, beta):
    yp, yh = y_form(case.form)
    return dict(y=y.t, rows=M, C=case.N, gamma=gamma, beta=beta, ldy=case.N + Y_PAD, y_coff=Y_COFF, y_planes=yp, y_h2=yh)


@functools.lru_cache(maxsize=2)
def pair(form, N, S, bias, R):
    """both routes of one case -> (reference Run, its y, fused Run, its y, gamma, beta)"""
    case = case_of(form, N, S, bias, R)
    gamma, beta = 1.0 + 0.1 * rnd(N, seed=N + S), 0.1 * rnd(N, seed=N + S + 1)
    dg, db = dev(gamma), dev(beta)
    ref = TG.Run(case, False)
    assert LH.launch_gemm(**ref.fields) == 0
    y_ref = Guarded((M, N + Y_PAD), torch.float32)
    assert LH.launch_layernorm(LH.job(x=ref.C.t.data_ptr() + 4 * case.c_coff, ldx=ref.ldc, **ln_fields(case, y_ref, dg, db))) == 0
    fus = TG.Run(case, False)
    before = fus.C.bits().copy()
    assert LH.launch_gemm(raw=1, **fus.fields) == 0
    assert (fus.C.bits() == before).all(), "the raw-slice GEMM wrote C"
    y_fus = Guarded((M, N + Y_PAD), torch.float32)
    f = fus.fields
    j = LH.job(part=fus.ws.t, slices=S, bias=f.get("bias", 0), R=f.get("R", 0), ldr=f.get("ldr", 0), r_coff=f.get("r_coff", 0),
               x_out=fus.C.t, ldxo=fus.ldc, xo_coff=case.c_coff, **ln_fields(case, y_fus, dg, db))
    assert LH.launch_layernorm(j) == 0
    return ref, y_ref, fus, y_fus, gamma, beta


@pytest.mark.parametrize("form,N,S", SHAPES)
def test_fused_pair_equals_gemm_reduce_layernorm(form, N, S):
    for bias, R in EPILOGUES:
        ref, y_ref, fus, y_fus, _, _ = pair(form, N, S, bias, R)
        tag = f"bias {bias}, residual {R or 'none'}"
        for r in (ref, fus):
            r.check_buffers()                     # C outside its window, a separate residual, the scratch's guards; every slice element written
        part = fus.ws.bits().reshape(S, M, N)
        assert (part == ref.ws.bits().reshape(S, M, N)).all(), tag
        if S == 4:
            assert (part[3] == 0).all(), "the empty slice's partials are not zero"
        assert (fus.C.bits() == ref.C.bits()).all(), f"x_out differs ({tag})"
        for y in (y_ref, y_fus):
            y.assert_untouched_outside(np.s_[:, Y_COFF:Y_COFF + N])
        assert (y_fus.bits() == y_ref.bits()).all(), f"y differs ({tag})"
        assert (y_fus.bits()[:, Y_COFF:Y_COFF + N] != SENT32).all()


@pytest.mark.parametrize("form,N,S", SHAPES)
def test_fused_pair_against_fp64(form, N, S):
    worst_x = worst_y = 0.0
    for bias, R in EPILOGUES:
        _, _, fus, y_fus, gamma, beta = pair(form, N, S, bias, R)
        x64 = fus.h["ref"]
        worst_x = max(worst_x, fus.compare())
        y64 = KR.layer_norm(x64, gamma, beta)
        yp, yh = y_form(form)
        win = y_fus.t[:, Y_COFF:Y_COFF + N]
        if yp:
            bits = KR.decode_planes(win.contiguous().view(torch.uint8).cpu().numpy(), 2)
            got = (KR.f16_bits_to_f64(bits).sum(0) / yh) if yh else KR.bf16_bits_to_f64(bits).sum(0)
        else:
            got = win.double().cpu().numpy()
        assert np.isfinite(got).all()
        worst_y = max(worst_y, np.abs(got - y64).max() / max(1.0, np.abs(y64).max()))
    report("gemm_ln_x", f"{form}-{N}-sk{S}", worst_x)
    report("gemm_ln_y", f"{form}-{N}-sk{S}", worst_y)
    assert worst_x <= TG.TOL["gemm_split_ws_kernel"], f"{worst_x:.3e}"
    tol_y = TG.TOL["P output"] if y_form(form)[0] else TG.TOL["gemm_split_ws_kernel"]
    assert worst_y <= tol_y, f"{worst_y:.3e} > {tol_y:.3e}"


def test_refusals():
    case = case_of("bf16x2", 192, 2, True, "")
    r = TG.Run(case, False)
    before = r.C.bits().copy()
    f = dict(r.fields)
    assert LH.launch_gemm(raw=1, **{**f, "splitk": 1}) == LH.INVALID_VALUE
    assert LH.launch_gemm(raw=1, **{**f, "c_planes": 2, "ldc": 208, "c_coff": 0}) == LH.INVALID_VALUE
    assert LH.launch_gemm(raw=1, **{**f, "c_bf16": 1}) == LH.INVALID_VALUE
    assert (r.C.bits() == before).all() and (r.ws.bits() == SENT32).all(), "a refused launch wrote"
    y = Guarded((M, 192 + Y_PAD), torch.float32)
    g = dev(rnd(192))
    for slices in (0, -1):
        j = LH.job(part=r.ws.t, slices=slices, x_out=r.C.t, ldxo=r.ldc, xo_coff=4, **ln_fields(case, y, g, g))
        assert LH.launch_layernorm(j) == LH.INVALID_VALUE
    y.assert_untouched_outside(None)
    assert (r.C.bits() == before).all()
