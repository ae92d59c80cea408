#!/usr/bin/env python3
"""Times brn_attention_forward on device tensors with HIP events: 5 warm-up calls, then 20 timed calls (one event pair per call; the
median and the fastest are printed).  Shapes: the Swin-L stage-0 window batch of examples/bench_swin_attn.rs:16-20 /
bench_flash_attn.rs:64-67 with a broadcast bias, the shifted shape of test_flash_bias.rs:288-292 with one bias per window, and the
2904-head shape of bench_flash_attn.rs:74 without a bias; modes f32 and bf16.  FLOP = 4 batch heads N^2 32; bytes = q, k, v, y and
every bias matrix once (what the algorithm needs: with n_bias 484 the bias alone is 241 MB).

  python tools/bench_attention_op.py [--row 0|1|2] [--mode f32|bf16]"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

ROWS = [(484, 6, 144, 1), (484, 6, 144, 484), (1, 2904, 144, 0)]      # batch, heads, N, n_bias
WARMUP, TIMED = 5, 20


def bench(row, mode):
    import torch
    from candle_birefnet_amd import ops
    batch, heads, N, n_bias = row
    g = torch.Generator(device="cuda").manual_seed(1)
    q, k, v = (torch.randn(batch, heads, N, 32, device="cuda", generator=g) for _ in range(3))
    bias = torch.randn(n_bias, heads, N, N, device="cuda", generator=g) * (0.5 * 32 ** 0.5) if n_bias else None
    ops.set_compute(mode)
    try:
        for _ in range(WARMUP):
            ops.attention(q, k, v, bias)
        torch.cuda.synchronize()
        ms = []
        for _ in range(TIMED):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            y = ops.attention(q, k, v, bias)
            e1.record()
            e1.synchronize()
            ms.append(e0.elapsed_time(e1))
    finally:
        ops.set_compute("f32")
    assert bool(torch.isfinite(y).all())
    ms.sort()
    med, best = ms[len(ms) // 2], ms[0]
    flop = 4.0 * batch * heads * N * N * 32
    nbytes = 4.0 * (4 * batch * heads * N * 32 + n_bias * heads * N * N)
    print(f"{batch:4d} x {heads:4d} x {N} x 32  n_bias {n_bias:3d}  {mode:4s}: median {med:.4f} ms, fastest {best:.4f} ms per call, "
          f"{flop / med / 1e9:.2f} TF/s, {nbytes / med / 1e6:.0f} GB/s of algorithmic bytes ({nbytes / 1e6:.1f} MB)", flush=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--row", type=int, choices=range(len(ROWS)))
    ap.add_argument("--mode", choices=["f32", "bf16"])
    a = ap.parse_args()
    import candle_birefnet_amd as cb
    if cb.device_count() < 1:
        sys.exit("no HIP device: nothing is measured")
    for row in (ROWS if a.row is None else [ROWS[a.row]]):
        for mode in (["f32", "bf16"] if a.mode is None else [a.mode]):
            bench(row, mode)
