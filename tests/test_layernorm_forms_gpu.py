"""kernels/layernorm.hip through the kernel harness: the fp32 output against an fp64 reference, then every other output form the launcher
accepts (bf16, fp16, the two- and three-plane P layouts, the fp16-pair planes of mode f32_half2) twice over: bit for bit against that
fp32 output pushed through the emulated format (kernel_refs.py), and directly against the fp64 reference at the bound the format allows
(one storage ulp, 2^-17 for two bf16 planes, nothing for three, 2^-21 for the fp16 pair; each on top of the fp32 term of
test_ops_gpu._close), so that no check rests on the kernel agreeing with itself.  Rows are wider than C on both sides and y_coff != 0."""
import functools

import numpy as np
import pytest
import torch

import kernel_refs as KR
from kernel_harness import Guarded, call, dev, report, rnd, run, windowed
from test_ops_gpu import S16_ULP, _close

pytestmark = pytest.mark.gpu

EPS, F32_TOL = 1e-5, 3e-5
# C reaches the five NV instantiations (1, 2, 3, 6, 12 float4 per lane), each with a full and a ragged last vector
DENSE = [(rows, C) for C in [4, 256, 260, 768, 772, 1540, 3072] for rows in [1, 5, 9]] + [(8200, 4)]    # 8200 rows: a second grid-stride row
MERGE = (2, 5, 3, 32)                                                                                    # B, H, W, Cin: odd H and W
CASES = [("dense", r, c) for r, c in DENSE] + [("merge",) + MERGE]
PLANE_CASES = [c for c in CASES if (c[2] if c[0] == "dense" else 4 * c[4]) % 32 == 0]
ids = lambda cs: ["-".join(map(str, c)) for c in cs]                                                      # noqa: E731


@functools.lru_cache(maxsize=None)
def _inputs(case):
    """(launcher arguments up to ldx, rows, C, fp64 reference) of a case; the operands stay on the device for every form"""
    if case[0] == "dense":
        _, rows, C = case
        ldx = C + 4
        xv = rnd(rows, C, seed=rows + C, std=3.0) + 0.5
        x, xe = windowed(xv, ldx, 0, torch.float32)
        geo = (0, 0, 0, 0)
    else:
        _, B, H, W, Cin = case
        C, ldx = 4 * Cin, 0
        xv = rnd(B, H, W, Cin, seed=11, std=3.0) + 0.5
        x, xe = dev(xv), KR.patch_merge_gather(xv.astype(np.float64))
        rows = xe.shape[0]
        geo = (1, H, W, Cin)
    g, b = 1 + rnd(C, seed=2, std=0.1), rnd(C, seed=3, std=0.1)
    return dict(x=x, g=dev(g), b=dev(b), rows=rows, C=C, ldx=ldx, geo=geo, ref=KR.layer_norm(xe, g, b, EPS))


def _launch(inp, y, ldy, y_coff, planes=0, h2=0.0, s16=0, fn=run):
    return fn("launch_layernorm", inp["x"], y, inp["rows"], inp["C"], inp["g"], inp["b"], EPS, inp["ldx"], ldy, y_coff, *inp["geo"], planes, h2, s16)


@functools.lru_cache(maxsize=None)
def _f32_output(case):
    inp = _inputs(case)
    C, ldy, coff = inp["C"], inp["C"] + 12, 8
    y = Guarded((inp["rows"], ldy), torch.float32)
    _launch(inp, y.t, ldy, coff)
    y.assert_untouched_outside(np.s_[:, coff:coff + C])
    return y.t[:, coff:coff + C].cpu().numpy()


def _bound(ref, rel):
    return rel * np.abs(ref) + F32_TOL * max(1.0, float(np.abs(ref).max()))


@pytest.mark.parametrize("case", CASES, ids=ids(CASES))
def test_layernorm_f32(gpu, case):
    y, ref = _f32_output(case), _inputs(case)["ref"]
    assert np.isfinite(y).all()
    report("layernorm", "f32", np.abs(y - ref).max())
    _close(y, ref)


@pytest.mark.parametrize("fname,flag,dt", [("bf16", 1, torch.bfloat16), ("f16", 2, torch.float16)], ids=["bf16", "f16"])
@pytest.mark.parametrize("case", CASES, ids=ids(CASES))
def test_layernorm_16bit(gpu, case, fname, flag, dt):
    inp, y32 = _inputs(case), _f32_output(case)
    C, ldy, coff = inp["C"], inp["C"] + 12, 8                    # in 16-bit elements
    y = Guarded((inp["rows"], ldy), dt)
    _launch(inp, y.t, ldy, coff, s16=flag)
    y.assert_untouched_outside(np.s_[:, coff:coff + C])
    got = y.t[:, coff:coff + C].cpu()
    want = torch.from_numpy(y32).to(dt)
    assert (got.view(torch.int16).numpy() == want.view(torch.int16).numpy()).all(), "not the RNE cast of the fp32 output"
    err = np.abs(got.double().numpy() - inp["ref"])
    report("layernorm", fname, err.max())
    assert (err <= _bound(inp["ref"], S16_ULP[fname])).all(), f"max abs err {err.max():.3e}"


def _plane_run(case, NP, h2=0.0):
    """run a plane form into rows that are two 32-column tiles wider than the window (y_coff = 32); returns (decoded planes [NP, rows, C]
    as uint16 bits, the fp32 output of the same case)"""
    inp, y32 = _inputs(case), _f32_output(case)
    C, coff = inp["C"], 32
    K = C + 64                                                   # logical columns of a row
    ldy = K * NP // 2                                            # floats: NP * 2 bytes per column
    y = Guarded((inp["rows"], ldy), torch.float32)
    _launch(inp, y.t, ldy, coff, planes=NP, h2=h2)
    y.assert_guards()
    planes = KR.decode_planes(y.t.cpu().numpy().view(np.uint8), NP)
    sent16 = np.uint16(0xFFC5), np.uint16(0xA5A5)                 # the halves of the fp32 sentinel
    outside = np.concatenate([planes[:, :, :coff], planes[:, :, coff + C:]], axis=2)
    assert np.isin(outside, sent16).all(), "columns outside the window were written"
    return planes[:, :, coff:coff + C], y32, inp["ref"]


@pytest.mark.parametrize("NP", [2, 3], ids=["P2", "P3"])
@pytest.mark.parametrize("case", PLANE_CASES, ids=ids(PLANE_CASES))
def test_layernorm_bf16_planes(gpu, case, NP):
    planes, y32, ref = _plane_run(case, NP)
    want, _ = KR.split_bf16(y32, NP)
    for p in range(NP):
        assert (planes[p] == want[p]).all(), f"plane {p} is not the emulated split of the fp32 output"
    total = KR.bf16_bits_to_f64(planes).sum(0)
    if NP == 3:
        assert (total == y32.astype(np.float64)).all(), "three planes do not sum back to the fp32 output"
    err = np.abs(total - ref)
    report("layernorm", f"P{NP}", err.max())
    assert (err <= _bound(ref, 2.0 ** -17 if NP == 2 else 0.0)).all(), f"max abs err {err.max():.3e}"


@pytest.mark.parametrize("s", [8.0, 0.5])
@pytest.mark.parametrize("case", PLANE_CASES, ids=ids(PLANE_CASES))
def test_layernorm_f16_pair_planes(gpu, case, s):
    planes, y32, ref = _plane_run(case, 2, h2=s)
    want, _ = KR.split_h2(y32, s)
    for p, name in enumerate(["hi", "lo"]):
        assert (planes[p] == want[p]).all(), f"the {name} plane is not the emulated fp16 pair of the fp32 output"
    err = np.abs(KR.f16_bits_to_f64(planes).sum(0) / s - ref)
    report("layernorm", f"H2(s={s:g})", err.max())
    assert (err <= _bound(ref, 2.0 ** -21)).all(), f"max abs err {err.max():.3e}"


def test_layernorm_refusals(gpu):
    inp = dict(_inputs(("dense", 5, 256)))
    y = Guarded((5, 512), torch.float32)

    def refused(C=256, ldy=320, coff=32, **kw):
        return _launch(dict(inp, C=C), y.t, ldy, coff, fn=call, **kw) != 0

    assert refused(C=6) and refused(C=3076) and refused(C=254)
    assert refused(C=48, planes=2) and refused(C=48, planes=3)            # planes need whole 32-column tiles
    assert refused(planes=1) and refused(planes=4)
    assert refused(planes=2, ldy=328) and refused(planes=2, coff=16)
    assert refused(h2=8.0) and refused(h2=8.0, planes=3)                  # the fp16 pair is a two-plane form
    assert refused(s16=1, planes=2) and refused(s16=2, planes=3)          # 16-bit output or planes, not both
    assert refused(s16=1, ldy=322) and refused(s16=1, coff=6)
    assert _launch(dict(inp, rows=0), y.t, 320, 32, fn=call) != 0
    merge = dict(_inputs(("merge",) + MERGE))
    assert _launch(dict(merge, C=96), y.t, 320, 32, fn=call) != 0         # C != 4 * Cin
    y.assert_untouched_outside(None)
