"""Every launcher of kernels/elementwise.hip, called directly through the kernel harness (kernel_harness.py) and held to an fp64 reference
on the exact operands: ragged sizes, every storage form, input and output windows inside wider rows, and sentinel bits around and
between everything a kernel may write.  Tolerances are the project's: test_ops_gpu._close (3e-5 of max(1, max|ref|)) for fp32 results,
1e-5 for the resizes (test_upsample_bilinear), one storage ulp (S16_ULP) on top for 16-bit outputs; data movement is bit-exact."""
import numpy as np
import pytest
import torch

import kernel_harness as KH
import kernel_refs as KR
from kernel_harness import FORMS, Guarded, bits_of, dev, report, rnd, run, call, windowed
from test_ops_gpu import S16_ULP

pytestmark = pytest.mark.gpu

F32_TOL, RESIZE_TOL = 3e-5, 1e-5
form = pytest.mark.parametrize("fname,flag,dt", FORMS, ids=[f[0] for f in FORMS])
S16 = [f for f in FORMS if f[1]]
form16 = pytest.mark.parametrize("fname,flag,dt", S16, ids=[f[0] for f in S16])


def check(kernel, fname, got, ref, tol=F32_TOL, out_s16=None, what=""):
    """got against the fp64 ref: tol * max(1, max|ref|), plus one ulp of the 16-bit storage type when the kernel's output is stored in one"""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    assert got.shape == ref.shape
    assert np.isfinite(got).all(), f"{kernel} {fname} {what}: non-finite output"
    err = np.abs(got - ref)
    report(kernel, fname, err.max() if err.size else 0.0)
    bound = tol * max(1.0, float(np.abs(ref).max())) + (S16_ULP[out_s16] * np.abs(ref) if out_s16 else 0.0)
    assert (err <= bound).all(), f"{kernel} {fname} {what}: max abs err {err.max():.3e}, bound {np.min(bound):.3e}.."


def s16(fname):
    return fname if fname != "f32" else None


# ---------------------------------------------------------------- resize_nhwc
RESIZE_SIZES = [(1, 1, 3, 5), (3, 5, 1, 1), (2, 3, 2, 3), (5, 7, 11, 13), (9, 6, 4, 5)]
# (C, ldx, x_coff, ldy, y_coff): all multiples of 8 -> the 16-byte kernel in the 16-bit forms; C = 12 or an offset of 4 -> the 4-wide kernel
RESIZE_WINDOWS = {"c8_wide16": (8, 24, 8, 16, 8), "c12": (12, 24, 4, 20, 4), "c8_coff4": (8, 16, 4, 12, 4)}


def _resize(flag, dt, xv, win, Hout, Wout, accumulate=0, y0=None):
    C, ldx, xc, ldy, yc = win
    B, Hin, Win, _ = xv.shape
    x, xe = windowed(xv, ldx, xc, dt)
    y = Guarded((B, Hout, Wout, ldy), dt)
    if y0 is not None:
        y.t[..., yc:yc + C] = dev(y0, dt)
    run("launch_resize_nhwc", x, B, Hin, Win, C, ldx, xc, y.t, Hout, Wout, ldy, yc, flag, accumulate)
    y.assert_untouched_outside(np.s_[..., yc:yc + C])
    return xe, y.t[..., yc:yc + C]


@form
@pytest.mark.parametrize("win", list(RESIZE_WINDOWS))
@pytest.mark.parametrize("Hin,Win,Hout,Wout", RESIZE_SIZES)
def test_resize_nhwc(gpu, fname, flag, dt, win, Hin, Win, Hout, Wout):
    w = RESIZE_WINDOWS[win]
    xv = rnd(2, Hin, Win, w[0], seed=1)
    xe, y = _resize(flag, dt, xv, w, Hout, Wout)
    if (Hin, Win) == (Hout, Wout):
        assert (bits_of(y) == bits_of(dev(xv, dt))).all(), "the identity resize is not a bit-exact copy"
    check("resize_nhwc", fname, y.double().cpu().numpy(), KR.resize_nhwc(xe, Hout, Wout), tol=RESIZE_TOL, out_s16=s16(fname), what=win)


@form16
@pytest.mark.parametrize("Hin,Win,Hout,Wout", RESIZE_SIZES)
def test_resize_nhwc_both_kernels_agree(gpu, fname, flag, dt, Hin, Win, Hout, Wout):
    xv = rnd(2, Hin, Win, 8, seed=2)
    _, wide = _resize(flag, dt, xv, RESIZE_WINDOWS["c8_wide16"], Hout, Wout)
    _, narrow = _resize(flag, dt, xv, RESIZE_WINDOWS["c8_coff4"], Hout, Wout)
    assert (bits_of(wide) == bits_of(narrow)).all(), "the 16-byte and the 4-wide kernel differ on the same data"


@pytest.mark.parametrize("win", list(RESIZE_WINDOWS))
@pytest.mark.parametrize("Hin,Win,Hout,Wout", RESIZE_SIZES)
def test_resize_nhwc_accumulate(gpu, win, Hin, Win, Hout, Wout):
    w = RESIZE_WINDOWS[win]
    xv, y0 = rnd(2, Hin, Win, w[0], seed=3), rnd(2, Hout, Wout, w[0], seed=4)
    xe, y = _resize(0, torch.float32, xv, w, Hout, Wout, accumulate=1, y0=y0)
    check("resize_nhwc+acc", "f32", y.double().cpu().numpy(), y0.astype(np.float64) + KR.resize_nhwc(xe, Hout, Wout), tol=RESIZE_TOL, what=win)


def test_resize_nhwc_refusals(gpu):
    x = dev(rnd(2, 3, 5, 24))
    for flag, dt in [(1, torch.bfloat16), (2, torch.float16)]:               # accumulate exists for fp32 maps only
        y = Guarded((2, 4, 4, 16), dt)
        assert call("launch_resize_nhwc", x, 2, 3, 5, 8, 24, 8, y.t, 4, 4, 16, 8, flag, 1) != 0
        y.assert_untouched_outside(None)
    y = Guarded((2, 4, 4, 16), torch.float32)
    for C, ldx, xc, ldy, yc in [(6, 24, 0, 16, 0), (8, 22, 0, 16, 0), (8, 24, 0, 14, 0), (8, 24, 2, 16, 0), (8, 24, 0, 16, 2)]:
        for flag in (0, 1, 2):
            assert call("launch_resize_nhwc", x, 2, 3, 5, C, ldx, xc, y.t, 4, 4, ldy, yc, flag, 0) != 0, (C, ldx, xc, ldy, yc)
    y.assert_untouched_outside(None)


# ---------------------------------------------------------------- nchw <-> nhwc
LAYOUT_C, LAYOUT_HW = [1, 31, 33, 100], [(1, 1), (31, 1), (3, 11), (7, 10)]      # HW = 1, 31, 33, 70


@form
def test_nchw_to_nhwc(gpu, fname, flag, dt):
    for C in LAYOUT_C:
        for H, W in LAYOUT_HW:
            xv = rnd(2, C, H, W, seed=C + H)
            ld, coff = C + 5, 3
            y = Guarded((2, H * W, ld), dt)
            run("launch_nchw_to_nhwc", dev(xv), 2, C, H, W, y.t, ld, coff, flag)
            y.assert_untouched_outside(np.s_[..., coff:coff + C])
            want = torch.from_numpy(xv).reshape(2, C, H * W).permute(0, 2, 1).to(dt)          # torch's RNE cast, on the CPU
            assert (bits_of(y.t[..., coff:coff + C]) == bits_of(want)).all(), (C, H, W)


@form
def test_nhwc_to_nchw(gpu, fname, flag, dt):
    for C in LAYOUT_C:
        for H, W in LAYOUT_HW:
            ld, coff = C + 5, 3
            x, _ = windowed(rnd(2, H * W, C, seed=C + W), ld, coff, dt)
            y = Guarded((2, C, H * W), torch.float32)
            run("launch_nhwc_to_nchw", x, 2, C, H, W, ld, coff, y.t, flag)
            y.assert_untouched_outside(np.s_[...])
            want = x[..., coff:coff + C].cpu().float().permute(0, 2, 1)
            assert (y.bits() == bits_of(want)).all(), (C, H, W)


def test_layout_round_trip_f32(gpu):
    for C in LAYOUT_C:
        for H, W in LAYOUT_HW:
            x = dev(rnd(2, C, H, W, seed=7))
            mid, back = Guarded((2, H * W, C + 3), torch.float32), Guarded((2, C, H, W), torch.float32)
            run("launch_nchw_to_nhwc", x, 2, C, H, W, mid.t, C + 3, 2, 0)
            run("launch_nhwc_to_nchw", mid.t, 2, C, H, W, C + 3, 2, back.t, 0)
            assert (back.bits() == bits_of(x)).all(), (C, H, W)


# ---------------------------------------------------------------- dtype converters
def _special_f32(n):
    """n fp32 values: random ones behind (as far as n allows) signed zeros, subnormals of both types, Inf, NaN, values that round up to the
    next binade, ties, and the 16-bit type's overflow edge"""
    x = rnd(n, seed=n, std=3.0)
    sp = np.array([-0.0, 0.0, 1e-40, -1e-45, 2.0 ** -130, 6e-8, -3e-6, np.inf, -np.inf, np.nan, 1.9999999, -3.9999998, 255.99999,
                   1.00390625, 1.01171875, 1.0009765625, 1.00048828125, 65519.0, 65520.0, -70000.0, 3.3e38, 3.4e38, 2.0 ** -24, 2.0 ** -25,
                   0.99999994], np.float32)
    x[:min(n, len(sp))] = sp[:n]
    return x


@pytest.mark.parametrize("f16,dt", [(0, torch.bfloat16), (1, torch.float16)], ids=["bf16", "f16"])
def test_f32_to_16bit(gpu, f16, dt):
    for n in [1, 255, 257, 70001]:
        x = _special_f32(n)
        y = Guarded((n,), dt)
        run("launch_f32_to_bf16", dev(x), n, y.t, f16)
        y.assert_untouched_outside(np.s_[...])
        want = torch.from_numpy(x).to(dt)
        nan = np.isnan(x)
        assert torch.isnan(y.t.cpu()[torch.from_numpy(nan)]).all(), "NaN did not stay NaN"
        assert (y.bits()[~nan] == bits_of(want)[~nan]).all(), n


@pytest.mark.parametrize("f16,dt", [(0, torch.bfloat16), (1, torch.float16)], ids=["bf16", "f16"])
def test_16bit_to_f32(gpu, f16, dt):
    for n in [1, 255, 257, 70001]:
        bits = np.random.default_rng(n).integers(-32768, 32768, n).astype(np.int16)       # every bit pattern class, NaNs included
        bits[:min(n, 6)] = np.array([0, -32768, 1, -32767, 0x7C00 if f16 else 0x7F80, 0x0400 if f16 else 0x0080], np.int16)[:n]
        x = torch.from_numpy(bits).view(dt)
        y = Guarded((n,), torch.float32)
        run("launch_bf16_to_f32", x.cuda(), n, y.t, f16)
        y.assert_untouched_outside(np.s_[...])
        want, got = x.float(), y.t.cpu()
        nan = torch.isnan(want)
        assert torch.isnan(got[nan]).all()
        assert (bits_of(got)[~nan.numpy()] == bits_of(want)[~nan.numpy()]).all(), n


# ---------------------------------------------------------------- image2patches
@form
@pytest.mark.parametrize("Cimg,H,W,th,tw,cpad,ld", [(3, 4, 144, 2, 72, 16, 24), (3, 32, 32, 4, 4, 192, 200), (3, 48, 48, 8, 8, 128, 136)])
def test_image2patches(gpu, fname, flag, dt, Cimg, H, W, th, tw, cpad, ld):
    xv = rnd(2, Cimg, H, W, seed=5)
    cout = Cimg * (H // th) * (W // tw)
    y = Guarded((2, th, tw, ld), dt)
    run("launch_image2patches", dev(xv), 2, Cimg, H, W, th, tw, y.t, ld, cpad, flag)
    y.assert_untouched_outside(np.s_[..., :cpad])
    want = torch.from_numpy(KR.image2patches_nhwc(xv, th, tw, cpad)).float().to(dt)          # fp32 -> fp64 -> fp32 is the identity
    got = bits_of(y.t[..., :cpad])
    assert (got[..., cout:] == 0).all(), "pad channels are not +0"
    assert (got == bits_of(want)).all()


def test_image2patches_refusals(gpu):
    y = Guarded((2, 2, 4, 24), torch.float32)
    x = dev(rnd(2, 3, 5, 8))
    assert call("launch_image2patches", x, 2, 3, 5, 8, 2, 4, y.t, 24, 16, 0) != 0        # H % th
    assert call("launch_image2patches", x, 2, 3, 5, 8, 5, 3, y.t, 24, 16, 0) != 0        # W % tw
    y.assert_untouched_outside(None)


# ---------------------------------------------------------------- global average pool
@form
def test_gap_nhwc(gpu, fname, flag, dt):
    for HW in [1, 15, 17, 128, 129, 643]:
        for C in [4, 64, 68, 132]:
            ld, coff = C + 8, 4
            x, xe = windowed(rnd(2, HW, C, seed=HW + C) + 0.25, ld, coff, dt)
            n = KH.lib().kh_gap_scratch_floats(2, HW, C)
            assert n == 2 * ((HW + 127) // 128) * C
            outs = []
            for _ in range(2):
                scratch, out = Guarded((n,), torch.float32), Guarded((2, C), torch.float32)
                run("launch_gap_nhwc", x, 2, HW, C, ld, coff, scratch.t, out.t, flag)
                scratch.assert_guards()                       # nothing past gap_scratch_floats floats
                out.assert_untouched_outside(np.s_[...])
                outs.append(out.bits())
            assert (outs[0] == outs[1]).all(), "two runs differ"
            check("gap_nhwc", fname, out.t.double().cpu().numpy(), xe.mean(axis=1), what=f"HW={HW} C={C}")


def test_gap_refusals(gpu):
    x, scratch, out = dev(rnd(2, 5, 16)), Guarded((64,), torch.float32), Guarded((2, 8), torch.float32)
    for C, ld, coff in [(6, 16, 0), (8, 14, 0), (8, 16, 2)]:
        assert call("launch_gap_nhwc", x, 2, 5, C, ld, coff, scratch.t, out.t, 0) != 0
    scratch.assert_untouched_outside(None)
    out.assert_untouched_outside(None)


# ---------------------------------------------------------------- small_fc
@pytest.mark.parametrize("act", [0, 1], ids=["none", "relu"])
@pytest.mark.parametrize("affine", [False, True], ids=["plain", "scale_shift"])
def test_small_fc(gpu, affine, act):
    for Cin in [1, 63, 65, 256]:
        for N in [1, 3, 5, 256]:
            ldw, w_off = Cin + 7, 3
            xv = rnd(2, Cin, seed=Cin)
            w, we = windowed(rnd(N, Cin, seed=N, std=Cin ** -0.5), ldw, w_off, torch.float32)
            sc, sh = 1 + rnd(N, seed=1, std=0.3), rnd(N, seed=2)
            y = Guarded((2, N), torch.float32)
            run("launch_small_fc", dev(xv), 2, Cin, w, ldw, w_off, N, dev(sc) if affine else None, dev(sh) if affine else None, act, y.t)
            y.assert_untouched_outside(np.s_[...])
            ref = xv.astype(np.float64) @ we.T
            if affine:
                ref = ref * sc.astype(np.float64) + sh.astype(np.float64)
            if act:
                ref = np.maximum(ref, 0)
            check("small_fc", "f32", y.t.double().cpu().numpy(), ref, what=f"Cin={Cin} N={N}")


# ---------------------------------------------------------------- GDT gate
@form
def test_gdt_gate(gpu, fname, flag, dt):
    for npix in [1, 3, 5, 37]:
        for C in [4, 256, 260]:
            ldp, coff, ldg = C + 8, 4, 20
            wv = rnd(16, seed=3, std=0.5)
            gv = rnd(npix, 16, seed=npix)
            sat = np.arange(npix) % 3                                   # 1: logit +100, 2: logit -100, 0: an ordinary one
            gv[sat == 1] = 100 * wv / (wv * wv).sum()
            gv[sat == 2] = -100 * wv / (wv * wv).sum()
            g, ge = windowed(gv, ldg, 0, dt)
            pv = rnd(npix, C, seed=C)
            p = Guarded((npix, ldp), dt)
            p.t[:, coff:coff + C] = dev(pv, dt)
            pe = p.t[:, coff:coff + C].double().cpu().numpy()
            before = bits_of(p.t[:, coff:coff + C])
            bias = 0.125
            run("launch_gdt_gate", p.t, npix, C, ldp, coff, g, ldg, dev(wv), bias, flag)
            p.assert_untouched_outside(np.s_[:, coff:coff + C])
            logit = ge[:, :16] @ wv.astype(np.float64) + bias
            assert (np.abs(logit[sat > 0]) > 95).all()
            got = p.t[:, coff:coff + C]
            check("gdt_gate", fname, got.double().cpu().numpy(), pe / (1 + np.exp(-logit))[:, None], out_s16=s16(fname), what=f"npix={npix} C={C}")
            assert (bits_of(got)[sat == 1] == before[sat == 1]).all(), "a saturated gate is not exactly 1"
            assert (got.double().cpu().numpy()[sat == 2] == 0).all(), "a closed gate is not exactly 0"


# ---------------------------------------------------------------- pixel_dot
@form
def test_pixel_dot(gpu, fname, flag, dt):
    for npix in [1, 15, 17, 1000]:
        for C in [4, 60, 68, 192]:
            ld, coff = C + 8, 4
            x, xe = windowed(rnd(npix, C, seed=npix + C), ld, coff, dt)
            wv = rnd(C, seed=C, std=C ** -0.5)
            y = Guarded((npix,), torch.float32)
            run("launch_pixel_dot", x, npix, C, ld, coff, dev(wv), -0.375, y.t, flag)
            y.assert_untouched_outside(np.s_[...])
            check("pixel_dot", fname, y.t.double().cpu().numpy(), xe @ wv.astype(np.float64) - 0.375, what=f"npix={npix} C={C}")


# ---------------------------------------------------------------- final head
@pytest.mark.parametrize("sig", [0, 1], ids=["logits", "sigmoid"])
@pytest.mark.parametrize("h,w,H,W", [(1, 1, 4, 4), (2, 3, 8, 12), (3, 2, 12, 8)])
def test_final_head(gpu, h, w, H, W, sig):
    qv, tv, bias = rnd(2, h, w, seed=1), rnd(2, H, W, seed=2), 0.3
    if sig:                                             # logits of +-100 and beyond exp's fp32 range: no NaN, exactly 0 / 1
        tv[0, 0, 0], tv[1, H - 1, W - 1], tv[0, 1, 1] = 100.0, -100.0, -90.0
    out = Guarded((2, H, W), torch.float32)
    run("launch_final_head", dev(qv), 2, h, w, dev(tv), bias, H, W, sig, out.t)
    out.assert_untouched_outside(np.s_[...])
    ref = KR.resize_nchw(qv[:, None], H, W)[:, 0] + tv.astype(np.float64) + bias
    if sig:
        ref = 1 / (1 + np.exp(-ref))
    check("final_head", "f32", out.t.double().cpu().numpy(), ref, what="sigmoid" if sig else "logits")


# ---------------------------------------------------------------- 5x5 head stencil
@pytest.mark.parametrize("H,W", [(2, 2), (2, 70), (5, 3), (9, 130)])
def test_head_stencil5x5(gpu, H, W):
    img, k, bias = rnd(2, 3, H, W, seed=1), rnd(9, 5, 5, 3, seed=2, std=0.2), rnd(9, seed=3)
    y = Guarded((2, H, W), torch.float32)
    run("launch_head_stencil5x5", dev(img), 2, H, W, dev(k), dev(bias), y.t)
    y.assert_untouched_outside(np.s_[...])
    check("head_stencil5x5", "f32", y.t.double().cpu().numpy(), KR.head_stencil5x5(img, k, bias), what=f"{H}x{W}")


def test_head_stencil5x5_refusals(gpu):
    y = Guarded((2, 8), torch.float32)
    img, k, bias = dev(rnd(2, 3, 1, 8)), dev(rnd(9, 75)), dev(rnd(9))
    assert call("launch_head_stencil5x5", img, 2, 1, 8, k, bias, y.t) != 0
    assert call("launch_head_stencil5x5", img, 2, 8, 1, k, bias, y.t) != 0
    y.assert_untouched_outside(None)


# ---------------------------------------------------------------- sigmoids
def _logits(rows, c0, c1, ld=27):
    """[rows, ld] with +-100, +-0 and the edges of exp's fp32 range inside columns [c0, c1) of the first and the last row"""
    x = rnd(rows, ld, seed=rows, std=3.0)
    sp = np.array([100.0, -100.0, 0.0, -0.0, 88.0, -88.0, 89.0, -104.0, 30.0], np.float32)
    x[0, c0:c1] = sp[:c1 - c0]
    x[rows - 1, c0:c1] = -sp[:c1 - c0][::-1] if rows > 1 else x[0, c0:c1]
    return x


@pytest.mark.parametrize("c0,c1", [(18, 27), (3, 5)])
@pytest.mark.parametrize("rows", [1, 7])
def test_mod_sigmoid2(gpu, rows, c0, c1):
    ld = 27
    xv = _logits(rows, c0, c1)
    x = Guarded((rows, ld), torch.float32)
    x.t[:, c0:c1] = dev(xv[:, c0:c1])
    run("launch_mod_sigmoid2", x.t, rows, ld, c0, c1)
    x.assert_untouched_outside(np.s_[:, c0:c1])
    check("mod_sigmoid2", "f32", x.t[:, c0:c1].double().cpu().numpy(), 2 / (1 + np.exp(-xv[:, c0:c1].astype(np.float64))))


@pytest.mark.parametrize("rows", [1, 7])
def test_sigmoid(gpu, rows):
    xv = _logits(rows, 0, 9)
    y = Guarded((rows * 27,), torch.float32)
    run("launch_sigmoid", dev(xv), rows * 27, y.t)
    y.assert_untouched_outside(np.s_[...])
    check("sigmoid", "f32", y.t.double().cpu().numpy(), 1 / (1 + np.exp(-xv.reshape(-1).astype(np.float64))))


# ---------------------------------------------------------------- resize_nchw (the one launcher that also has an op entry)
@pytest.mark.parametrize("Hin,Win,Hout,Wout", RESIZE_SIZES)
def test_resize_nchw(gpu, Hin, Win, Hout, Wout):
    xv = rnd(2, 3, Hin, Win, seed=8)
    y = Guarded((2, 3, Hout, Wout), torch.float32)
    run("launch_resize_nchw", dev(xv), 6, Hin, Win, y.t, Hout, Wout)
    y.assert_untouched_outside(np.s_[...])
    check("resize_nchw", "f32", y.t.double().cpu().numpy(), KR.resize_nchw(xv, Hout, Wout), tol=RESIZE_TOL)
