#!/usr/bin/env python3
"""Times ops.deform_conv2d (brn_deform_conv2d_offsets_forward) on device tensors with HIP events, in one process: 3 warm-up calls, then 10
timed calls (one event pair per call; the median and the fastest are printed).  One ASPP-sized shape — B 1, C 64, O 256, 7 x 7, pad 3,
256 x 256, with a mask — through the fused route (one offset group) and through the column route (two offset groups fed the same offsets:
the same arithmetic, as a column matrix of 65536 x 3136 elements + the mode's dense GEMM), in modes f32_half2 and bf16.
A size for the column route's overhead, not a benchmark: every call repacks and uploads the host weights and allocates its workspace, as
every op-level entry does, and both routes pay that alike.

  python tools/bench_deform_offsets.py"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

B, C, O, K, P, H, W = 1, 64, 256, 7, 3, 256, 256
WARMUP, TIMED = 3, 10


def bench(mode, groups):
    import numpy as np
    import torch
    from candle_birefnet_amd import ops
    g = torch.Generator(device="cuda").manual_seed(1)
    x = torch.randn(B, C, H, W, device="cuda", generator=g)
    off1 = torch.randn(B, 2 * K * K, H, W, device="cuda", generator=g) * 1.5
    msk1 = torch.rand(B, K * K, H, W, device="cuda", generator=g) * 2.0
    offset, mask = off1.repeat(1, groups, 1, 1).contiguous(), msk1.repeat(1, groups, 1, 1).contiguous()
    w = (np.random.default_rng(2).standard_normal((O, C, K, K)) * (C * K * K) ** -0.5).astype(np.float32)
    ops.set_compute(mode)
    try:
        for _ in range(WARMUP):
            ops.deform_conv2d(x, offset, w, None, padding=P, mask=mask)
        torch.cuda.synchronize()
        ms = []
        for _ in range(TIMED):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            y = ops.deform_conv2d(x, offset, w, None, padding=P, mask=mask)
            e1.record()
            e1.synchronize()
            ms.append(e0.elapsed_time(e1))
    finally:
        ops.set_compute("f32")
    assert bool(torch.isfinite(y).all())
    ms.sort()
    esz = 2 if mode in ("bf16", "f16") else 4
    col_mb = B * H * W * K * K * C * esz / 1e6
    print(f"{mode:10s} {'fused  ' if groups == 1 else 'columns'} (G = {groups}): median {ms[len(ms) // 2]:.3f} ms, fastest {ms[0]:.3f} ms per call"
          + (f"; column matrix {col_mb:.0f} MB written once and read once" if groups > 1 else ""), flush=True)
    return y


if __name__ == "__main__":
    import candle_birefnet_amd as cb
    if cb.device_count() < 1:
        sys.exit("no HIP device: nothing is measured")
    for mode in ("f32_half2", "bf16"):
        yf, yc = bench(mode, 1), bench(mode, 2)
        print(f"{mode:10s} max |columns - fused| = {float((yc - yf).abs().max()):.3e} on outputs of max magnitude {float(yf.abs().max()):.2f}", flush=True)
