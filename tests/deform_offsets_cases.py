"""What the CPU and GPU tests of brn_deform_conv2d_offsets_forward (ops.deform_conv2d) share: an fp64 restatement of torchvision's
deform_conv2d with offset groups, per-axis stride / padding / dilation and an optional mask, written out from the entry's contract in
include/birefnet_hip.h (tests/torch_ref.py::deform_conv2d is the one-group, one-stride, dilation-1 special case), and the input recipes."""
import numpy as np
import torch


def pair(v):
    return (int(v), int(v)) if isinstance(v, int) else (int(v[0]), int(v[1]))


def out_hw(H, W, kh, kw, stride, padding, dilation):
    (sh, sw), (ph, pw), (dh, dw) = pair(stride), pair(padding), pair(dilation)
    return (H + 2 * ph - dh * (kh - 1) - 1) // sh + 1, (W + 2 * pw - dw * (kw - 1) - 1) // sw + 1


def restatement(x, offset, mask, weight, bias, stride=1, padding=0, dilation=1):
    """fp64.  x [B,C,H,W], offset [B, 2 G kh kw, Ho, Wo], mask [B, G kh kw, Ho, Wo] or None, weight [O,C,kh,kw], bias [O] or None."""
    d = torch.float64
    x, offset, weight = (torch.as_tensor(a).to(d) for a in (x, offset, weight))
    mask = None if mask is None else torch.as_tensor(mask).to(d)
    B, C, H, W = x.shape
    O, _, kh, kw = weight.shape
    taps = kh * kw
    G = offset.shape[1] // (2 * taps)
    assert offset.shape[1] == 2 * G * taps and C % G == 0
    cpg = C // G
    Ho, Wo = offset.shape[2], offset.shape[3]
    (sh, sw), (ph, pw), (dh, dw) = pair(stride), pair(padding), pair(dilation)
    assert (Ho, Wo) == out_hw(H, W, kh, kw, stride, padding, dilation)
    ys = torch.arange(Ho, dtype=d).view(1, Ho, 1) * sh - ph
    xs = torch.arange(Wo, dtype=d).view(1, 1, Wo) * sw - pw
    col = torch.zeros(B, C, taps, Ho, Wo, dtype=d)
    for g in range(G):
        xg = x[:, g * cpg:(g + 1) * cpg].reshape(B, cpg, H * W)
        for i in range(kh):
            for j in range(kw):
                t = i * kw + j
                py = ys + i * dh + offset[:, 2 * (g * taps + t)]
                px = xs + j * dw + offset[:, 2 * (g * taps + t) + 1]
                valid = (py > -1) & (py < H) & (px > -1) & (px < W)
                y0, x0 = torch.floor(py), torch.floor(px)
                ly, lx = py - y0, px - x0
                val = torch.zeros(B, cpg, Ho, Wo, dtype=d)
                for dy, wy in ((0, 1 - ly), (1, ly)):
                    for dx, wx in ((0, 1 - lx), (1, lx)):
                        yy, xx = (y0 + dy).long(), (x0 + dx).long()
                        ok = valid & (yy >= 0) & (yy <= H - 1) & (xx >= 0) & (xx <= W - 1)
                        idx = (yy.clamp(0, H - 1) * W + xx.clamp(0, W - 1)).view(B, 1, -1).expand(B, cpg, -1)
                        gat = torch.gather(xg, 2, idx).view(B, cpg, Ho, Wo)
                        val = val + gat * torch.where(ok, wy * wx, torch.zeros_like(wy)).unsqueeze(1)
                if mask is not None:
                    val = val * mask[:, g * taps + t].unsqueeze(1)
                col[:, g * cpg:(g + 1) * cpg, t] = val
    out = torch.einsum("bckhw,ock->bohw", col, weight.reshape(O, C, taps))
    if bias is not None:
        out = out + torch.as_tensor(bias).to(d).view(1, -1, 1, 1)
    return out.numpy()


def random_case(seed, B, C, G, kh, kw, stride, padding, dilation, H, W, O, use_mask, bias=True):
    """offsets of standard deviation 1.5 px with entries of 40.0 that leave every map; weights scaled to unit-variance outputs"""
    g = np.random.default_rng(seed)
    Ho, Wo = out_hw(H, W, kh, kw, stride, padding, dilation)
    assert Ho >= 1 and Wo >= 1
    n = lambda *sh, std=1.0: (g.standard_normal(sh) * std).astype(np.float32)
    offset = n(B, 2 * G * kh * kw, Ho, Wo, std=1.5)
    flat = offset.reshape(-1)
    flat[g.integers(0, flat.size, max(1, flat.size // 50))] = 40.0
    mask = (g.uniform(0.0, 2.0, (B, G * kh * kw, Ho, Wo)).astype(np.float32)) if use_mask else None
    K = C * kh * kw
    return dict(x=n(B, C, H, W), offset=offset, mask=mask, weight=n(O, C, kh, kw, std=K ** -0.5), bias=n(O, std=0.1) if bias else None,
                stride=pair(stride), padding=pair(padding), dilation=pair(dilation))


def round_to(a, mode):
    """a rounded to the 16-bit storage type of compute mode bf16 / f16 (round to nearest even), back in fp32"""
    t = torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32))
    return t.to(torch.bfloat16 if mode == "bf16" else torch.float16).to(torch.float32).numpy()


def reference(case, mode="f32"):
    """the restatement on the case; for the 16-bit modes on x and w rounded to the type (the exact-operand reference)"""
    x, w = case["x"], case["weight"]
    if mode in ("bf16", "f16"):
        x, w = round_to(x, mode), round_to(w, mode)
    return restatement(x, case["offset"], case["mask"], w, case["bias"], case["stride"], case["padding"], case["dilation"])


def run_op(case, compute="f32", **over):
    """ops.deform_conv2d on the case under ops.set_compute(compute); numpy in, numpy out unless over[...] replaces an argument"""
    from candle_birefnet_amd import ops
    a = dict(case)
    a.update(over)
    ops.set_compute(compute)
    try:
        return ops.deform_conv2d(a["x"], a["offset"], a["weight"], a["bias"], stride=a["stride"], padding=a["padding"], dilation=a["dilation"],
                                 mask=a["mask"])
    finally:
        ops.set_compute("f32")
