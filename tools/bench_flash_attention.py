#!/usr/bin/env python3
"""Times brn_flash_attention_forward on device tensors with HIP events: 5 warm-up calls, then 20 timed calls (one event pair per call; the
median and the fastest are reported).  Shapes: those of examples/bench_flash_attn.rs:70-84 (the two Swin-L window batches, the LLM
shapes 1 x 512 .. 8192 x 32 x 128 and 4 x 2048 x 8 x 64), in flash_attention's [batch, seq, heads, head_dim] layout, without and with
the causal mask; modes f32, bf16 and f16.  FLOP = 4 batch heads seq_q seq_kv head_dim, halved for causal.

Beside each non-causal row, in the same process and on the same values, the unfused "standard attention" of bench_flash_attn.rs:89-95
in torch — (q * scale) @ k^T, softmax over the last dim, @ v on [batch, heads, seq, head_dim] tensors — timed the same way; in the
16-bit modes torch gets tensors of that dtype.  It is the yardstick the reference example itself uses (it has no causal form).

  python tools/bench_flash_attention.py [--row N] [--mode f32|bf16|f16] [--json PATH]"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

ROWS = [(484, 144, 6, 32), (1, 144, 484 * 6, 32), (1, 512, 32, 128), (1, 1024, 32, 128), (1, 2048, 32, 128), (1, 4096, 32, 128),
        (1, 8192, 32, 128), (4, 2048, 8, 64)]                      # batch, seq, heads, head_dim
MODES = ["f32", "bf16", "f16"]
WARMUP, TIMED = 5, 20


def _time(fn):
    import torch
    for _ in range(WARMUP):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(TIMED):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        y = fn()
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    ms.sort()
    return ms[len(ms) // 2], ms[0], y


def standard_attention(q, k, v):
    """bench_flash_attn.rs:89-95"""
    import torch
    scale = 1.0 / (q.shape[-1] ** 0.5)
    attn = (q * scale) @ k.transpose(-2, -1)
    attn = torch.softmax(attn, dim=-1)
    return attn @ v


def bench(row, mode):
    import torch
    from candle_birefnet_amd import ops
    batch, seq, heads, hd = row
    g = torch.Generator(device="cuda").manual_seed(1)
    q, k, v = (torch.randn(batch, heads, seq, hd, device="cuda", generator=g) for _ in range(3))      # bench_flash_attn.rs:19-21
    qf, kf, vf = (a.transpose(1, 2).contiguous() for a in (q, k, v))                                    # bench_flash_attn.rs:40-42
    flop = 4.0 * batch * heads * seq * seq * hd
    out = []
    ops.set_compute(mode)
    try:
        for causal in (False, True):
            med, best, y = _time(lambda: ops.flash_attention(qf, kf, vf, causal=causal))
            assert bool(torch.isfinite(y).all())
            f = flop / 2 if causal else flop
            rec = {"batch": batch, "seq": seq, "heads": heads, "head_dim": hd, "mode": mode, "causal": int(causal), "ms_median": round(med, 4),
                   "ms_fastest": round(best, 4), "tflops": round(f / med / 1e9, 2), "torch_ms_median": None, "torch_tflops": None}
            if not causal:
                dt = {"f32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16}[mode]
                qt, kt, vt = (a.to(dt) for a in (q, k, v))
                tmed, _, yt = _time(lambda: standard_attention(qt, kt, vt))
                rec["torch_ms_median"], rec["torch_tflops"] = round(tmed, 4), round(f / tmed / 1e9, 2)
                rec["max_abs_diff_vs_torch"] = float((y.transpose(1, 2) - yt.float()).abs().max())
                del qt, kt, vt, yt
            out.append(rec)
            print(f"{batch:4d} x {seq:5d} x {heads:4d} x {hd:3d} {mode:4s} causal {int(causal)}: median {med:9.4f} ms, fastest {best:9.4f} ms, {rec['tflops']:7.2f} TF/s"
                  + (f"   | torch standard attention {rec['torch_ms_median']:9.4f} ms, {rec['torch_tflops']:7.2f} TF/s" if not causal else ""), flush=True)
    finally:
        ops.set_compute("f32")
    torch.cuda.empty_cache()
    return out


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--row", type=int, choices=range(len(ROWS)))
    ap.add_argument("--mode", choices=MODES)
    ap.add_argument("--json", help="write the records to this file")
    a = ap.parse_args()
    import candle_birefnet_amd as cb
    if cb.device_count() < 1:
        sys.exit("no HIP device: nothing is measured")
    recs = []
    for row in (ROWS if a.row is None else [ROWS[a.row]]):
        for mode in (MODES if a.mode is None else [a.mode]):
            recs += bench(row, mode)
    if a.json:
        with open(a.json, "w") as f:
            json.dump({"tool": "tools/bench_flash_attention.py", "warmup": WARMUP, "timed": TIMED, "rows": recs}, f, indent=1)
            f.write("\n")
