#!/usr/bin/env python3
"""Times brn_flash_attention_forward on device tensors with HIP events: 5 warm-up calls, then 20 timed calls (one event pair per call; the
median and the fastest are reported).  Shapes: those of examples/bench_flash_attn.rs:70-84 (the two Swin-L window batches, the LLM
shapes 1 x 512 .. 8192 x 32 x 128 and 4 x 2048 x 8 x 64), in flash_attention's [batch, seq, heads, head_dim] layout, without and with
the causal mask; modes f32, bf16 and f16.  FLOP = 4 batch heads seq_q seq_kv head_dim, halved for causal.

Beside each non-causal row, in the same process and on the same values, the unfused "standard attention" of bench_flash_attn.rs:89-95
in torch — (q * scale) @ k^T, softmax over the last dim, @ v on [batch, heads, seq, head_dim] tensors — timed the same way; in the
16-bit modes torch gets tensors of that dtype.  It is the yardstick the reference example itself uses (it has no causal form).

--bias times brn_flash_attention_bias_forward instead: per row, in the same process and on the same values, the bias-free call, the
call with one standard-normal x sqrt(head_dim) bias for every batch entry (n_bias = 1, [1, heads, seq, seq] fp32) and torch's unfused
attention with `+ bias` before the softmax (fp32 bias in every mode, as the fused call has it; non-causal rows only).  Two more rows, the
Swin windows of 16 and 24 ((64, 256, 6, 32) and (16, 576, 6, 32)), come with it; they and the window-12 row also get the repeating
form, n_bias = n_windows = batch.  Per record: ms with and without the bias, their difference, and that difference set against
bias bytes / 8 TB/s — the share of the HBM roof the bias stream reaches (non-causal: every bias byte is read exactly once).

--gqa times brn_flash_attention_gqa_forward beside the route it replaces, on the same values and in the same process, the two sides
ALTERNATING in 5 rounds of 3 warm-up + 10 timed calls each (median and fastest over the 50 calls of a side; spread = the lowest and the
highest of its 5 round medians).  Rows (batch, seq_q, seq_kv, heads, kv_heads, head_dim):
  seq_q == seq_kv   the grouped call, not causal and causal, against brn_flash_attention_forward on K / V materialised G times along heads
                    (the repeat itself is made once, outside the timed calls: the older route is not charged for it)
  seq_q <  seq_kv   the causal call over the cache against brn_flash_attention_bias_forward, not causal, on repeated K / V with the mask as
                    a [1, heads, seq_q, seq_kv] fp32 bias of 0 / -inf
Each record says whether the two sides returned the same bits.

--varlen times brn_flash_attention_varlen_forward in the same alternating style, on device tensors, in three groups of rows (--row 0 / 1 / 2):
  windows   causal sliding windows (W - 1, 0), W = 1024 and 4096, at seq 16384 with 32 / 8 heads of 128, beside the full causal call of the gqa
            entry on the same values (the window call walks at most ceil((W + 64 / G) / 64) + 1 K / V tiles per workgroup, the full causal call
            128 on average)
  ragged    a causal pack of 16 sequences of 128 .. 8192 positions in one call beside a loop of 16 gqa calls, one per sequence
  uniform   a [batch, seq, heads, head_dim] tensor as a pack with no window beside the gqa entry on it, with a "same bits" column; the packed
            call uploads its workgroup table through a temporary and synchronises the stream, which the event pair around it sees
The packed call's cu_seqlens are host arrays, as the entry requires.

--splitkv times brn_flash_attention_splitkv_forward in the same alternating style (all sides of a row take turns in each of the 5 rounds),
modes bf16 and f32, at 32 / 8 heads of 128: the decode rows 16 x 1 / 4096, 1 x 1 / 4096, 1 x 1 / 32768, 1 x 1 / 65536, the causal row
1 x 8 / 16384 and 64 x 1 / 4096, whose unsplit grid is already 512 workgroups.  Sides per row: brn_flash_attention_gqa_forward (the
baseline) and the new entry at kv_splits 1, 2, 4, 8, 16, 32, 64 and 0 (the library's rule); the timed new call includes the combine
launch.  Both sides are raw library calls on preallocated device tensors (y, lse and the workspace are allocated once per side, outside
the timed calls), so an event pair sees the library call and nothing of a wrapper.  Per record: the S each side really used, the best
explicit side, whether the rule's median lies inside that side's round spread, and whether the rule is slower than the gqa call beyond
the gqa call's round spread.  Without --json the records go to profiles/flash_attention_splitkv_bench.json.

--paged times brn_flash_attention_paged_forward beside brn_flash_attention_splitkv_forward on the same logical data, in the same
alternating style, modes bf16 and f32, at 32 / 8 heads of 128, kv_splits 0 on every side: 16 x 1 / 4096, 1 x 1 / 32768, 64 x 1 / 4096, the
causal 1 x 8 / 16384, and a ragged batch of 16 sequences whose lengths are spread evenly over 512 .. 4096 (max_kv_len 4096; its dense side
is the padded call at 4096, which computes more).  Sides: the split entry on the dense K / V, then the paged entry with pages of 16, 64
and 256 keys, each with an identity table (the pool IS the dense tensor's memory) and a shuffled one (a permuted copy).  The table and the
lengths are device tensors; raw library calls on preallocated outputs.  Per paged side: its time over the dense side's, whether its median
lies inside the dense side's round spread, and (equal lengths) whether it returned the dense call's bits.  Without --json the records go
to profiles/flash_attention_paged_bench.json.
--paged-kv16 times brn_flash_attention_paged_kv_forward on a bf16 / fp16 pool beside brn_flash_attention_paged_forward on the fp32 pool of
the same values (the yardstick: the older entry's kernels, never the code under test), in the same compute mode, on the rows of --paged at
page 64 with a shuffled table, for the pairs bf16 on bf16, f16 on f16 and f32 on bf16; then brn_kv_cache_append (64 x 1 and 16 x 512 new
tokens, lengths in place) beside a device-to-device copy of the bytes it writes.  Same protocol; --row picks an attention row, --mode a
pair by its compute mode.  Written to profiles/flash_attention_paged_kv16_bench.json.
--paged-fp8 times brn_flash_attention_paged_fp8_forward on an e4m3 pool (per-head scales on the device) beside
brn_flash_attention_paged_kv_forward on the bf16 / fp16 pool holding the widened bytes (the yardstick: the parent's kernels; bf16 in modes
bf16 and f32, f16 in mode f16), with brn_flash_attention_paged_forward on the fp32 pool for context, on the same rows, page 64, shuffled
table, modes bf16, f16 and f32; then brn_kv_cache_append_fp8 beside a device-to-device copy of the bytes it writes.  Same protocol.
Written to profiles/flash_attention_paged_fp8_bench.json.
--rope times, per pool type (bf16, f16, f32, fp8) at the append's two shapes, four sides alternating with the same protocol:
brn_kv_cache_append_rope (HALF, rot_dim = head_dim), brn_kv_cache_append alone, the two-call form (brn_rope_forward on k_new into a
buffer at positions = kv_lens, then brn_kv_cache_append of it) and a device-to-device copy of the bytes written.  Written to
profiles/flash_attention_rope_bench.json.
--paged-varlen times brn_flash_attention_paged_varlen_forward on a packed batch (a mixed step of 31 decode sequences and one 512-token
chunk; a pure decode step of 32 sequences; heads 32 / 8 x 128, page 64, bf16 pool and compute, causal, every length 4096) beside
brn_flash_attention_paged_kv_forward (the yardstick: the parent's kernels) called once per group of sequences with the same number of
new tokens, at kv_splits 0, 0, 1, 2, 4, 4: a row printed twice must repeat its result checksum.  Same protocol.  Written to
profiles/flash_attention_paged_varlen_bench.json.

  python tools/bench_flash_attention.py [--bias | --gqa | --varlen | --splitkv | --paged | --paged-kv16 | --paged-fp8 | --rope | --paged-varlen] [--row N] [--mode f32|bf16|f16] [--json PATH]"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

ROWS = [(484, 144, 6, 32), (1, 144, 484 * 6, 32), (1, 512, 32, 128), (1, 1024, 32, 128), (1, 2048, 32, 128), (1, 4096, 32, 128),
        (1, 8192, 32, 128), (4, 2048, 8, 64)]                      # batch, seq, heads, head_dim
BIAS_ROWS = ROWS + [(64, 256, 6, 32), (16, 576, 6, 32)]          # + Swin windows of 16 and 24 (Swin-384 / SwinV2 geometries)
SWIN_ROWS = [(484, 144, 6, 32), (64, 256, 6, 32), (16, 576, 6, 32)]
GQA_ROWS = [(1, 4096, 4096, 32, 8, 128), (4, 2048, 2048, 32, 8, 64), (1, 512, 4096, 32, 8, 128), (16, 1, 4096, 32, 8, 128)]
GQA_ROUNDS, GQA_WARMUP, GQA_TIMED = 5, 3, 10
VARLEN_WINDOW_ROW, VARLEN_WINDOWS = (1, 16384, 16384, 32, 8, 128), (1024, 4096)
VARLEN_RAGGED = ([128 * n for n in (1, 2, 3, 4, 6, 8, 12, 16, 24, 32, 48, 64, 64, 32, 8, 1)], 32, 8, 128)      # lengths, heads, kv_heads, head_dim
VARLEN_UNIFORM_ROWS = [(4, 4096, 4096, 32, 8, 128), (1, 4096, 4096, 32, 8, 128), (4, 2048, 2048, 32, 8, 64)]
VARLEN_GROUPS = ["windows", "ragged", "uniform"]
# (batch, seq_q, seq_kv, heads, kv_heads, head_dim, causal)
SPLITKV_ROWS = [(16, 1, 4096, 32, 8, 128, 0), (1, 1, 4096, 32, 8, 128, 0), (1, 1, 32768, 32, 8, 128, 0), (1, 1, 65536, 32, 8, 128, 0),
                (1, 8, 16384, 32, 8, 128, 1), (64, 1, 4096, 32, 8, 128, 0)]
SPLITKV_SPLITS = [1, 2, 4, 8, 16, 32, 64, 0]
SPLITKV_MODES = ["bf16", "f32"]
SPLITKV_JSON = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "flash_attention_splitkv_bench.json")
# (batch, seq_q, max_kv_len, heads, kv_heads, head_dim, causal, ragged): ragged = lengths spread evenly over 512 .. max_kv_len
PAGED_ROWS = [(16, 1, 4096, 32, 8, 128, 0, 0), (1, 1, 32768, 32, 8, 128, 0, 0), (64, 1, 4096, 32, 8, 128, 0, 0), (1, 8, 16384, 32, 8, 128, 1, 0),
              (16, 1, 4096, 32, 8, 128, 0, 1)]
PAGED_PAGES = [16, 64, 256]
# --paged-kv16: the rows above at page 64 with a shuffled table, per (compute mode, pool type) pair; then the append:
# (batch, seq_new, kv_heads, head_dim, page_size, pages per sequence): a decode step and a prefill chunk
PAGED_KV16_PAGE = 64
PAGED_KV16_PAIRS = [("bf16", "bf16"), ("f16", "f16"), ("f32", "bf16")]
KV_APPEND_ROWS = [(64, 1, 8, 128, 64, 64), (16, 512, 8, 128, 64, 64)]
KV_APPEND_TYPES = ["bf16", "f16", "f32"]
PAGED_KV16_JSON = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "flash_attention_paged_kv16_bench.json")
PAGED_FP8_JSON = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "flash_attention_paged_fp8_bench.json")
ROPE_JSON = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "flash_attention_rope_bench.json")
PAGED_VARLEN_JSON = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "flash_attention_paged_varlen_bench.json")
# brn_flash_attention_paged_varlen_forward: (name, [(n_b, len_b)], the existing calls that do the same work as (batch, seq_q) groups of the pack in order)
PAGED_VARLEN_ROWS = [("mixed: 31 decode + one 512-token chunk", [(1, 4096)] * 31 + [(512, 4096)], [(31, 1), (1, 512)]),
                     ("decode: 32 sequences", [(1, 4096)] * 32, [(32, 1)])]
PAGED_VARLEN_SHAPE = (32, 8, 128, 64)            # heads, kv_heads, head_dim, page
PAGED_JSON = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "flash_attention_paged_bench.json")
HBM_BYTES_PER_S = 8.0e12
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


def standard_attention_bias(q, k, v, bias):
    """standard_attention with the bias of swin.rs:278-303, on the unscaled scores: softmax(scale * (q k^T + bias)) v"""
    import torch
    scale = 1.0 / (q.shape[-1] ** 0.5)
    attn = ((q @ k.transpose(-2, -1)) + bias) * scale
    attn = torch.softmax(attn, dim=-1)
    return attn.to(v.dtype) @ v


def bench_bias(row, mode):
    import torch
    from candle_birefnet_amd import ops
    batch, seq, heads, hd = row
    g = torch.Generator(device="cuda").manual_seed(1)
    q, k, v = (torch.randn(batch, heads, seq, hd, device="cuda", generator=g) for _ in range(3))
    qf, kf, vf = (a.transpose(1, 2).contiguous() for a in (q, k, v))
    forms = [1] + ([batch] if row in SWIN_ROWS else [])
    flop = 4.0 * batch * heads * seq * seq * hd
    out = []
    ops.set_compute(mode)
    try:
        for causal in (False, True):
            free, _, _ = _time(lambda: ops.flash_attention(qf, kf, vf, causal=causal))
            for n_bias in forms:
                bias = torch.randn(n_bias, heads, seq, seq, device="cuda", generator=g) * hd ** 0.5
                med, best, y = _time(lambda: ops.flash_attention(qf, kf, vf, causal=causal, bias=bias))
                assert bool(torch.isfinite(y).all())
                f = flop / 2 if causal else flop
                nbytes = 4.0 * batch * heads * seq * seq               # every (batch entry, head) streams its own [seq, seq] slab once
                roof = nbytes / HBM_BYTES_PER_S * 1e3
                rec = {"batch": batch, "seq": seq, "heads": heads, "head_dim": hd, "mode": mode, "causal": int(causal), "n_bias": n_bias,
                       "ms_bias_median": round(med, 4), "ms_bias_fastest": round(best, 4), "ms_free_median": round(free, 4),
                       "ms_added": round(med - free, 4), "tflops_bias": round(f / med / 1e9, 2), "bias_stream_bytes": int(nbytes),
                       "bias_roof_ms": None, "hbm_roof_share": None, "torch_bias_ms_median": None, "fused_not_slower_than_torch": None}
                if not causal:
                    rec["bias_roof_ms"] = round(roof, 4)
                    rec["hbm_roof_share"] = round(roof / (med - free), 3) if med > free else None
                    dt = {"f32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16}[mode]
                    qt, kt, vt = (a.to(dt) for a in (q, k, v))
                    bt = bias if n_bias == 1 else bias.repeat(batch // n_bias, 1, 1, 1)
                    tmed, _, yt = _time(lambda: standard_attention_bias(qt, kt, vt, bt))
                    rec["torch_bias_ms_median"] = round(tmed, 4)
                    rec["fused_not_slower_than_torch"] = bool(med <= tmed)
                    rec["max_abs_diff_vs_torch"] = float((y.transpose(1, 2) - yt.float()).abs().max())
                    del qt, kt, vt, yt, bt
                out.append(rec)
                print(f"{batch:4d} x {seq:5d} x {heads:4d} x {hd:3d} {mode:4s} causal {int(causal)} n_bias {n_bias:3d}: bias {med:9.4f} ms, free {free:9.4f} ms, "
                      f"added {med - free:8.4f} ms" + (f" (bias bytes at 8 TB/s {roof:8.4f} ms)   | torch + bias {rec['torch_bias_ms_median']:9.4f} ms"
                                                      f"{'' if rec['fused_not_slower_than_torch'] else '   SLOWER THAN TORCH'}" if not causal else ""), flush=True)
                del bias, y
    finally:
        ops.set_compute("f32")
    torch.cuda.empty_cache()
    return out


def _time_alternating(fns):
    """the sides of a comparison, alternating: per side (median ms, fastest ms, lowest round median, highest round median, last result)"""
    import torch
    ms = [[] for _ in fns]
    meds = [[] for _ in fns]
    ys = [None] * len(fns)
    for _ in range(GQA_ROUNDS):
        for i, fn in enumerate(fns):
            for _ in range(GQA_WARMUP):
                fn()
            torch.cuda.synchronize()
            r = []
            for _ in range(GQA_TIMED):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                ys[i] = fn()
                e1.record()
                e1.synchronize()
                r.append(e0.elapsed_time(e1))
            ms[i] += r
            meds[i].append(sorted(r)[len(r) // 2])
    return [(sorted(m)[len(m) // 2], min(m), min(md), max(md), y) for m, md, y in zip(ms, meds, ys)]


def bench_gqa(row, mode):
    import torch
    from candle_birefnet_amd import ops
    batch, seq_q, seq_kv, heads, kv_heads, hd = row
    G = heads // kv_heads
    g = torch.Generator(device="cuda").manual_seed(1)
    q = torch.randn(batch, seq_q, heads, hd, device="cuda", generator=g)
    k, v = (torch.randn(batch, seq_kv, kv_heads, hd, device="cuda", generator=g) for _ in range(2))
    kr, vr = (a.repeat_interleave(G, dim=2).contiguous() for a in (k, v))
    out = []
    ops.set_compute(mode)
    try:
        for causal in ((False, True) if seq_q == seq_kv else (True,)):
            if seq_q == seq_kv:
                old_name, bias = "flash_attention on repeated K/V", None
                old = lambda: ops.flash_attention(q, kr, vr, causal=causal)
                flop = 4.0 * batch * heads * seq_q * seq_kv * hd / (2 if causal else 1)
            else:
                old_name = "flash_attention + -inf mask bias on repeated K/V"
                vis = torch.arange(seq_kv, device="cuda")[None, :] <= torch.arange(seq_q, device="cuda")[:, None] + (seq_kv - seq_q)
                bias = torch.where(vis, 0.0, float("-inf")).to(torch.float32).expand(1, heads, seq_q, seq_kv).contiguous()
                old = lambda: ops.flash_attention(q, kr, vr, causal=False, bias=bias)
                flop = 4.0 * batch * heads * hd * float(vis.sum())
            new = lambda: ops.flash_attention_gqa(q, k, v, causal=causal)
            (nm, nf, nlo, nhi, yn), (om, of, olo, ohi, yo) = _time_alternating([new, old])
            assert bool(torch.isfinite(yn).all())
            rec = {"batch": batch, "seq_q": seq_q, "seq_kv": seq_kv, "heads": heads, "kv_heads": kv_heads, "head_dim": hd, "mode": mode, "causal": int(causal),
                   "gqa_ms_median": round(nm, 4), "gqa_ms_fastest": round(nf, 4), "gqa_round_medians": [round(nlo, 4), round(nhi, 4)],
                   "gqa_tflops": round(flop / nm / 1e9, 2), "old_route": old_name, "old_ms_median": round(om, 4), "old_ms_fastest": round(of, 4),
                   "old_round_medians": [round(olo, 4), round(ohi, 4)], "same_bits": bool(torch.equal(yn, yo))}
            out.append(rec)
            print(f"{batch:3d} x {seq_q:5d} / {seq_kv:5d} x {heads:3d} / {kv_heads:2d} x {hd:3d} {mode:4s} causal {int(causal)}: gqa {nm:9.4f} ms [{nlo:.4f} .. {nhi:.4f}] "
                  f"{rec['gqa_tflops']:7.2f} TF/s | {old_name} {om:9.4f} ms [{olo:.4f} .. {ohi:.4f}] | same bits {rec['same_bits']}", flush=True)
            del bias
    finally:
        ops.set_compute("f32")
    torch.cuda.empty_cache()
    return out


def _side(prefix, t):
    med, fastest, lo, hi, _ = t
    return {prefix + "_ms_median": round(med, 4), prefix + "_ms_fastest": round(fastest, 4), prefix + "_round_medians": [round(lo, 4), round(hi, 4)]}


def bench_varlen(group, mode):
    import numpy as np
    import torch
    from candle_birefnet_amd import ops
    g = torch.Generator(device="cuda").manual_seed(1)
    out = []
    ops.set_compute(mode)
    try:
        if group == "windows":
            batch, seq, _, heads, kv_heads, hd = VARLEN_WINDOW_ROW
            q = torch.randn(batch, seq, heads, hd, device="cuda", generator=g)
            k, v = (torch.randn(batch, seq, kv_heads, hd, device="cuda", generator=g) for _ in range(2))
            qp, kp, vp = q.reshape(batch * seq, heads, hd), k.reshape(batch * seq, kv_heads, hd), v.reshape(batch * seq, kv_heads, hd)
            cu = np.arange(batch + 1) * seq
            full = lambda: ops.flash_attention_gqa(q, k, v, causal=True)
            for W in VARLEN_WINDOWS:
                win = lambda: ops.flash_attention_varlen(qp, kp, vp, cu, cu, window=(W - 1, 0))
                tw, tf = _time_alternating([win, full])
                assert bool(torch.isfinite(tw[4]).all())
                G = heads // kv_heads
                rec = {"group": group, "batch": batch, "seq": seq, "heads": heads, "kv_heads": kv_heads, "head_dim": hd, "mode": mode, "window": [W - 1, 0],
                       "tiles_per_workgroup_at_most": -(-(W + 64 // G) // 64) + 1, "full_causal_tiles_per_workgroup_mean": (seq // 64 + 1) / 2}
                rec.update(_side("window", tw))
                rec.update(_side("full_causal_gqa", tf))
                rec["full_over_window"] = round(tf[0] / tw[0], 2)
                # queries 0 .. W - 1 see keys 0 .. query under both masks
                rec["first_W_rows_same_bits"] = bool(torch.equal(tw[4][:W], tf[4].reshape(batch * seq, heads, hd)[:W]))
                out.append(rec)
                print(f"windows {mode:4s} W {W:5d}: window {tw[0]:9.4f} ms [{tw[2]:.4f} .. {tw[3]:.4f}] | full causal gqa {tf[0]:9.4f} ms [{tf[2]:.4f} .. {tf[3]:.4f}] | "
                      f"full / window {rec['full_over_window']:.2f} | first W rows same bits {rec['first_W_rows_same_bits']}", flush=True)
        elif group == "ragged":
            lens, heads, kv_heads, hd = VARLEN_RAGGED
            cu = np.concatenate([[0], np.cumsum(lens)])
            total = int(cu[-1])
            q = torch.randn(total, heads, hd, device="cuda", generator=g)
            k, v = (torch.randn(total, kv_heads, hd, device="cuda", generator=g) for _ in range(2))
            parts = [tuple(a[cu[s]:cu[s + 1]][None] for a in (q, k, v)) for s in range(len(lens))]
            pack = lambda: ops.flash_attention_varlen(q, k, v, cu, cu, window=(-1, 0))
            loop = lambda: [ops.flash_attention_gqa(*p, causal=True) for p in parts]
            tp, tl = _time_alternating([pack, loop])
            same = all(bool(torch.equal(tp[4][cu[s]:cu[s + 1]], tl[4][s][0])) for s in range(len(lens)))
            rec = {"group": group, "lengths": lens, "heads": heads, "kv_heads": kv_heads, "head_dim": hd, "mode": mode, "window": [-1, 0]}
            rec.update(_side("pack", tp))
            rec.update(_side("loop_of_gqa_calls", tl))
            rec["loop_over_pack"] = round(tl[0] / tp[0], 2)
            rec["same_bits"] = same
            out.append(rec)
            print(f"ragged  {mode:4s} {len(lens)} sequences, {total} rows: pack {tp[0]:9.4f} ms [{tp[2]:.4f} .. {tp[3]:.4f}] | loop of gqa calls {tl[0]:9.4f} ms "
                  f"[{tl[2]:.4f} .. {tl[3]:.4f}] | loop / pack {rec['loop_over_pack']:.2f} | same bits {same}", flush=True)
        else:
            for batch, seq_q, seq_kv, heads, kv_heads, hd in VARLEN_UNIFORM_ROWS:
                q = torch.randn(batch, seq_q, heads, hd, device="cuda", generator=g)
                k, v = (torch.randn(batch, seq_kv, kv_heads, hd, device="cuda", generator=g) for _ in range(2))
                qp, kp, vp = q.reshape(batch * seq_q, heads, hd), k.reshape(batch * seq_kv, kv_heads, hd), v.reshape(batch * seq_kv, kv_heads, hd)
                cq, ckv = np.arange(batch + 1) * seq_q, np.arange(batch + 1) * seq_kv
                pack = lambda: ops.flash_attention_varlen(qp, kp, vp, cq, ckv)
                gqa = lambda: ops.flash_attention_gqa(q, k, v)
                tp, tg = _time_alternating([pack, gqa])
                rec = {"group": group, "batch": batch, "seq_q": seq_q, "seq_kv": seq_kv, "heads": heads, "kv_heads": kv_heads, "head_dim": hd, "mode": mode,
                       "window": [-1, -1]}
                rec.update(_side("pack", tp))
                rec.update(_side("gqa", tg))
                rec["same_bits"] = bool(torch.equal(tp[4].reshape(tg[4].shape), tg[4]))
                rec["pack_median_inside_gqa_round_spread"] = bool(tg[2] <= tp[0] <= tg[3])
                out.append(rec)
                print(f"uniform {mode:4s} {batch} x {seq_q} / {seq_kv} x {heads} / {kv_heads} x {hd}: pack {tp[0]:9.4f} ms [{tp[2]:.4f} .. {tp[3]:.4f}] | gqa {tg[0]:9.4f} ms "
                      f"[{tg[2]:.4f} .. {tg[3]:.4f}] | same bits {rec['same_bits']} | inside the gqa spread {rec['pack_median_inside_gqa_round_spread']}", flush=True)
                del q, k, v, qp, kp, vp
    finally:
        ops.set_compute("f32")
    torch.cuda.empty_cache()
    return out


def bench_splitkv(row, mode):
    import torch
    import candle_birefnet_amd as cb
    from candle_birefnet_amd import ops
    lib = cb._ffi.lib
    batch, seq_q, seq_kv, heads, kv_heads, hd, causal = row
    g = torch.Generator(device="cuda").manual_seed(1)
    q = torch.randn(batch, seq_q, heads, hd, device="cuda", generator=g)
    k, v = (torch.randn(batch, seq_kv, kv_heads, hd, device="cuda", generator=g) for _ in range(2))
    stream = torch.cuda.current_stream().cuda_stream
    R = batch * heads * seq_q
    yg = torch.empty_like(q)

    def gqa():
        cb._ffi.check(lib.brn_flash_attention_gqa_forward(q.data_ptr(), k.data_ptr(), v.data_ptr(), batch, seq_q, seq_kv, heads, kv_heads, hd, 0, causal, None, 0, 0.0,
                                                          yg.data_ptr(), 1, 0, stream))
        return yg

    def split_side(ks):
        S, tps, need = ops.flash_attention_splitkv_plan(batch, seq_q, seq_kv, heads, kv_heads, hd, ks)
        y, lse, ws = torch.empty_like(q), torch.empty(R, device="cuda"), torch.empty(max(need, 4), device="cuda")

        def fn():
            cb._ffi.check(lib.brn_flash_attention_splitkv_forward(q.data_ptr(), k.data_ptr(), v.data_ptr(), batch, seq_q, seq_kv, heads, kv_heads, hd, 0, causal, 0.0,
                                                                  ks, y.data_ptr(), lse.data_ptr(), ws.data_ptr(), need, 1, 0, stream))
            return y
        return fn, S, tps

    out = []
    ops.set_compute(mode)
    try:
        sides = [split_side(ks) for ks in SPLITKV_SPLITS]
        t = _time_alternating([gqa] + [s[0] for s in sides])
        tg, ts = t[0], t[1:]
        assert all(bool(torch.isfinite(x[4]).all()) for x in t)
        G = heads // kv_heads
        rec = {"batch": batch, "seq_q": seq_q, "seq_kv": seq_kv, "heads": heads, "kv_heads": kv_heads, "head_dim": hd, "mode": mode, "causal": causal,
               "base_workgroups": batch * kv_heads * ((G * seq_q + 63) // 64), "kv_tiles": (seq_kv + 63) // 64}
        rec.update(_side("gqa", tg))
        rec["splitkv"] = []
        for ks, (_, S, tps), tt in zip(SPLITKV_SPLITS, sides, ts):
            e = {"kv_splits": ks, "S": S, "tiles_per_split": tps, "max_abs_diff_vs_gqa": float((tt[4] - tg[4]).abs().max())}
            e.update(_side("split", tt))
            rec["splitkv"].append(e)
        rec["kv_splits_1_same_bits_as_gqa"] = bool(torch.equal(ts[0][4], tg[4]))
        explicit = rec["splitkv"][:-1]
        best, auto = min(explicit, key=lambda e: e["split_ms_median"]), rec["splitkv"][-1]
        rec["best_explicit_kv_splits"] = best["kv_splits"]
        rec["auto_S"] = auto["S"]
        rec["auto_inside_best_round_spread"] = bool(auto["split_ms_median"] <= best["split_round_medians"][1])
        rec["auto_slower_than_gqa_beyond_spread"] = bool(auto["split_ms_median"] > tg[3])
        rec["gqa_over_auto"] = round(tg[0] / auto["split_ms_median"], 2)
        out.append(rec)
        print(f"{batch:3d} x {seq_q:2d} / {seq_kv:5d} x {heads} / {kv_heads} x {hd} {mode:4s} causal {causal}: gqa {tg[0]:8.4f} ms [{tg[2]:.4f} .. {tg[3]:.4f}] | "
              + " | ".join(f"s{e['kv_splits']}(S {e['S']}) {e['split_ms_median']:.4f} [{e['split_round_medians'][0]:.4f} .. {e['split_round_medians'][1]:.4f}]" for e in rec["splitkv"])
              + f" | best explicit {best['kv_splits']}, rule S {auto['S']}, inside its spread {rec['auto_inside_best_round_spread']}, gqa / rule {rec['gqa_over_auto']:.2f}, "
                f"kv_splits 1 same bits {rec['kv_splits_1_same_bits_as_gqa']}", flush=True)
    finally:
        ops.set_compute("f32")
    del q, k, v
    torch.cuda.empty_cache()
    return out


def bench_paged(row, mode):
    import torch
    import candle_birefnet_amd as cb
    from candle_birefnet_amd import ops
    lib = cb._ffi.lib
    batch, seq_q, seq_kv, heads, kv_heads, hd, causal, ragged = row
    g = torch.Generator(device="cuda").manual_seed(1)
    q = torch.randn(batch, seq_q, heads, hd, device="cuda", generator=g)
    k, v = (torch.randn(batch, seq_kv, kv_heads, hd, device="cuda", generator=g) for _ in range(2))
    lens_h = [512 + (seq_kv - 512) * b // (batch - 1) for b in range(batch)] if ragged else [seq_kv] * batch
    lens = torch.tensor(lens_h, dtype=torch.int32, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream
    R = batch * heads * seq_q
    S, tps, need = ops.flash_attention_splitkv_plan(batch, seq_q, seq_kv, heads, kv_heads, hd, 0)

    def outputs():
        return torch.empty_like(q), torch.empty(R, device="cuda"), torch.empty(max(need, 4), device="cuda")

    yd, lsed, wsd = outputs()

    def dense():
        cb._ffi.check(lib.brn_flash_attention_splitkv_forward(q.data_ptr(), k.data_ptr(), v.data_ptr(), batch, seq_q, seq_kv, heads, kv_heads, hd, 0, causal, 0.0,
                                                              0, yd.data_ptr(), lsed.data_ptr(), wsd.data_ptr(), need, 1, 0, stream))
        return yd

    def paged_side(page, shuffle):
        n_pages, max_pages = batch * seq_kv // page, seq_kv // page
        ident = torch.arange(n_pages, dtype=torch.int64, device="cuda")
        if shuffle:
            # physical page perm[j] holds logical page j
            perm = torch.randperm(n_pages, device="cuda", generator=g)
            kp, vp = (torch.empty_like(a).view(n_pages, page, kv_heads, hd).index_copy_(0, perm, a.view(n_pages, page, kv_heads, hd)) for a in (k, v))
            table = perm.to(torch.int32).view(batch, max_pages).contiguous()
        else:
            kp, vp, table = k, v, ident.to(torch.int32).view(batch, max_pages).contiguous()
        y, lse, ws = outputs()

        def fn():
            cb._ffi.check(lib.brn_flash_attention_paged_forward(q.data_ptr(), kp.data_ptr(), vp.data_ptr(), table.data_ptr(), lens.data_ptr(), batch, seq_q, seq_kv,
                                                                heads, kv_heads, hd, n_pages, page, max_pages, 0, causal, 0.0, 0, y.data_ptr(), lse.data_ptr(),
                                                                ws.data_ptr(), need, 1, 0, stream))
            return y
        return fn, (kp, vp, table)

    out = []
    ops.set_compute(mode)
    try:
        names = [(page, shuffle) for page in PAGED_PAGES for shuffle in (False, True)]
        sides = [paged_side(*n) for n in names]
        t = _time_alternating([dense] + [s[0] for s in sides])
        td, tp = t[0], t[1:]
        assert all(bool(torch.isfinite(x[4]).all()) for x in t)
        rec = {"batch": batch, "seq_q": seq_q, "max_kv_len": seq_kv, "kv_lens": "all max_kv_len" if not ragged else lens_h, "heads": heads, "kv_heads": kv_heads,
               "head_dim": hd, "mode": mode, "causal": causal, "S": S, "tiles_per_split": tps,
               "kv_bytes_read": 2 * 4 * sum(lens_h) * kv_heads * hd, "table_bytes": 4 * batch * (seq_kv // 16)}
        rec.update(_side("dense_split", td))
        rec["paged"] = []
        for (page, shuffle), tt in zip(names, tp):
            e = {"page_size": page, "table": "shuffled" if shuffle else "identity", "over_dense": round(tt[0] / td[0], 4),
                 "inside_dense_round_spread": bool(td[2] <= tt[0] <= td[3]), "faster_than_dense_spread": bool(tt[0] < td[2])}
            if not ragged:
                e["same_bits_as_dense"] = bool(torch.equal(tt[4], td[4]))
            e.update(_side("paged", tt))
            rec["paged"].append(e)
        out.append(rec)
        print(f"{batch:3d} x {seq_q:2d} / {seq_kv:5d}{' ragged' if ragged else ''} x {heads} / {kv_heads} x {hd} {mode:4s} causal {causal} S {S}: "
              f"dense split {td[0]:8.4f} ms [{td[2]:.4f} .. {td[3]:.4f}] | "
              + " | ".join(f"p{e['page_size']} {e['table'][:5]} {e['paged_ms_median']:.4f} [{e['paged_round_medians'][0]:.4f} .. {e['paged_round_medians'][1]:.4f}] x{e['over_dense']:.3f}"
                           + ("" if ragged else f" bits {e['same_bits_as_dense']}") for e in rec["paged"]), flush=True)
    finally:
        ops.set_compute("f32")
    del q, k, v, sides
    torch.cuda.empty_cache()
    return out


def bench_paged_kv16(row, pair):
    """brn_flash_attention_paged_kv_forward on a 16-bit pool beside brn_flash_attention_paged_forward (the yardstick, the parent's kernels)
    on the fp32 pool of the same logical data, in the same compute mode; page 64, shuffled table"""
    import torch
    import candle_birefnet_amd as cb
    from candle_birefnet_amd import ops
    lib = cb._ffi.lib
    mode, kv = pair
    batch, seq_q, seq_kv, heads, kv_heads, hd, causal, ragged = row
    page = PAGED_KV16_PAGE
    tdt = torch.bfloat16 if kv == "bf16" else torch.float16
    g = torch.Generator(device="cuda").manual_seed(1)
    q = torch.randn(batch, seq_q, heads, hd, device="cuda", generator=g)
    lens_h = [512 + (seq_kv - 512) * b // (batch - 1) for b in range(batch)] if ragged else [seq_kv] * batch
    lens = torch.tensor(lens_h, dtype=torch.int32, device="cuda")
    n_pages, max_pages = batch * seq_kv // page, seq_kv // page
    perm = torch.randperm(n_pages, device="cuda", generator=g)
    table = perm.to(torch.int32).view(batch, max_pages).contiguous()
    # the 16-bit pool, and the fp32 pool holding the same values: one logical cache, two storage types
    pools16 = [torch.randn(n_pages, page, kv_heads, hd, device="cuda", generator=g).to(tdt) for _ in range(2)]
    pools32 = [a.float() for a in pools16]
    stream = torch.cuda.current_stream().cuda_stream
    R = batch * heads * seq_q
    S, tps, need = ops.flash_attention_splitkv_plan(batch, seq_q, seq_kv, heads, kv_heads, hd, 0)
    outs = [(torch.empty_like(q), torch.empty(R, device="cuda"), torch.empty(max(need, 4), device="cuda")) for _ in range(2)]
    tail = (table.data_ptr(), lens.data_ptr(), batch, seq_q, seq_kv, heads, kv_heads, hd, n_pages, page, max_pages, 0, causal, 0.0, 0)

    def fp32_pool():
        y, lse, ws = outs[0]
        cb._ffi.check(lib.brn_flash_attention_paged_forward(q.data_ptr(), pools32[0].data_ptr(), pools32[1].data_ptr(), *tail, y.data_ptr(), lse.data_ptr(), ws.data_ptr(), need, 1, 0, stream))
        return y

    def kv16_pool():
        y, lse, ws = outs[1]
        cb._ffi.check(lib.brn_flash_attention_paged_kv_forward(q.data_ptr(), pools16[0].data_ptr(), pools16[1].data_ptr(), cb._ffi.BRN_KV_BF16 if kv == "bf16" else cb._ffi.BRN_KV_F16,
                                                               *tail, y.data_ptr(), lse.data_ptr(), ws.data_ptr(), need, 1, 0, stream))
        return y

    ops.set_compute(mode)
    try:
        t32, t16 = _time_alternating([fp32_pool, kv16_pool])
        assert bool(torch.isfinite(t32[4]).all()) and bool(torch.isfinite(t16[4]).all())
        keys = sum(lens_h) * kv_heads * hd
        rec = {"batch": batch, "seq_q": seq_q, "max_kv_len": seq_kv, "kv_lens": "all max_kv_len" if not ragged else lens_h, "heads": heads, "kv_heads": kv_heads,
               "head_dim": hd, "mode": mode, "kv_type": kv, "page_size": page, "table": "shuffled", "causal": causal, "S": S, "tiles_per_split": tps,
               "fp32_pool_kv_bytes": 2 * 4 * keys, "kv16_pool_kv_bytes": 2 * 2 * keys,
               "kv16_over_fp32": round(t16[0] / t32[0], 4), "kv16_below_lowest_fp32_round_median": bool(t16[0] < t32[2]),
               "same_bits": bool(torch.equal(t16[4], t32[4])),
               "fp32_pool_tb_per_s": round(2 * 4 * keys / (t32[0] * 1e-3) / 1e12, 3), "kv16_pool_tb_per_s": round(2 * 2 * keys / (t16[0] * 1e-3) / 1e12, 3)}
        rec.update(_side("fp32_pool", t32))
        rec.update(_side("kv16_pool", t16))
        print(f"{batch:3d} x {seq_q:2d} / {seq_kv:5d}{' ragged' if ragged else ''} x {heads} / {kv_heads} x {hd} {mode:4s} on {kv:4s} causal {causal} S {S}: "
              f"fp32 pool {t32[0]:8.4f} ms [{t32[2]:.4f} .. {t32[3]:.4f}] {rec['fp32_pool_tb_per_s']:.2f} TB/s | {kv} pool {t16[0]:8.4f} ms [{t16[2]:.4f} .. {t16[3]:.4f}] "
              f"{rec['kv16_pool_tb_per_s']:.2f} TB/s x{rec['kv16_over_fp32']:.3f} below the fp32 side's lowest round {rec['kv16_below_lowest_fp32_round_median']} bits {rec['same_bits']}", flush=True)
    finally:
        ops.set_compute("f32")
    del q, pools16, pools32, outs
    torch.cuda.empty_cache()
    return [rec]


def bench_paged_fp8(row, mode):
    """brn_flash_attention_paged_fp8_forward on an e4m3 pool beside brn_flash_attention_paged_kv_forward on the 16-bit pool of the widened
    bytes (the yardstick, the parent's kernels) and brn_flash_attention_paged_forward on the fp32 pool, in one compute mode; page 64,
    shuffled table"""
    import torch
    import candle_birefnet_amd as cb
    from candle_birefnet_amd import ops
    lib = cb._ffi.lib
    batch, seq_q, seq_kv, heads, kv_heads, hd, causal, ragged = row
    page = PAGED_KV16_PAGE
    kv = "f16" if mode == "f16" else "bf16"
    tdt = torch.float16 if kv == "f16" else torch.bfloat16
    g = torch.Generator(device="cuda").manual_seed(1)
    q = torch.randn(batch, seq_q, heads, hd, device="cuda", generator=g)
    lens_h = [512 + (seq_kv - 512) * b // (batch - 1) for b in range(batch)] if ragged else [seq_kv] * batch
    lens = torch.tensor(lens_h, dtype=torch.int32, device="cuda")
    n_pages, max_pages = batch * seq_kv // page, seq_kv // page
    perm = torch.randperm(n_pages, device="cuda", generator=g)
    table = perm.to(torch.int32).view(batch, max_pages).contiguous()
    # one logical cache, three storage types: standard normal values / 2^-6, clamped, as e4m3 bytes; the same values in 16 bits and in fp32
    pools8 = [(torch.randn(n_pages, page, kv_heads, hd, device="cuda", generator=g) * 64).clamp_(-448, 448).to(torch.float8_e4m3fn) for _ in range(2)]
    pools16 = [a.to(tdt) for a in pools8]
    pools32 = [a.float() for a in pools8]
    k_scale, v_scale = (torch.full((kv_heads,), 2.0 ** -6, device="cuda") for _ in range(2))
    stream = torch.cuda.current_stream().cuda_stream
    R = batch * heads * seq_q
    S, tps, need = ops.flash_attention_splitkv_plan(batch, seq_q, seq_kv, heads, kv_heads, hd, 0)
    outs = [(torch.empty_like(q), torch.empty(R, device="cuda"), torch.empty(max(need, 4), device="cuda")) for _ in range(3)]
    s = hd ** -0.5
    ints = (batch, seq_q, seq_kv, heads, kv_heads, hd, n_pages, page, max_pages, 0, causal)

    def fp8_pool():
        y, lse, ws = outs[0]
        cb._ffi.check(lib.brn_flash_attention_paged_fp8_forward(q.data_ptr(), pools8[0].data_ptr(), pools8[1].data_ptr(), k_scale.data_ptr(), v_scale.data_ptr(), table.data_ptr(),
                                                                lens.data_ptr(), *ints, s, 0, y.data_ptr(), lse.data_ptr(), ws.data_ptr(), need, 1, 0, stream))
        return y

    def kv16_pool():
        y, lse, ws = outs[1]
        cb._ffi.check(lib.brn_flash_attention_paged_kv_forward(q.data_ptr(), pools16[0].data_ptr(), pools16[1].data_ptr(), cb._ffi.BRN_KV_BF16 if kv == "bf16" else cb._ffi.BRN_KV_F16,
                                                               table.data_ptr(), lens.data_ptr(), *ints, s * 2.0 ** -6, 0, y.data_ptr(), lse.data_ptr(), ws.data_ptr(), need, 1, 0, stream))
        return y

    def fp32_pool():
        y, lse, ws = outs[2]
        cb._ffi.check(lib.brn_flash_attention_paged_forward(q.data_ptr(), pools32[0].data_ptr(), pools32[1].data_ptr(), table.data_ptr(), lens.data_ptr(), *ints, s * 2.0 ** -6, 0,
                                                            y.data_ptr(), lse.data_ptr(), ws.data_ptr(), need, 1, 0, stream))
        return y

    ops.set_compute(mode)
    try:
        t8, t16, t32 = _time_alternating([fp8_pool, kv16_pool, fp32_pool])
        assert all(bool(torch.isfinite(t[4]).all()) for t in (t8, t16, t32))
        keys = sum(lens_h) * kv_heads * hd
        tb = lambda nbytes, t: round(2 * nbytes * keys / (t[0] * 1e-3) / 1e12, 3)
        rec = {"batch": batch, "seq_q": seq_q, "max_kv_len": seq_kv, "kv_lens": "all max_kv_len" if not ragged else lens_h, "heads": heads, "kv_heads": kv_heads,
               "head_dim": hd, "mode": mode, "yardstick_kv_type": kv, "page_size": page, "table": "shuffled", "causal": causal, "S": S, "tiles_per_split": tps,
               "fp8_pool_kv_bytes": 2 * keys, "kv16_pool_kv_bytes": 4 * keys, "fp32_pool_kv_bytes": 8 * keys,
               "fp8_over_kv16": round(t8[0] / t16[0], 4), "fp8_over_fp32": round(t8[0] / t32[0], 4), "fp8_below_lowest_kv16_round_median": bool(t8[0] < t16[2]),
               # y = v_scale * the yardstick's y with v_scale a power of two: the same bits scaled exactly
               "same_bits_as_kv16_times_v_scale": bool(torch.equal(t8[4], t16[4] * 2.0 ** -6)),
               "fp8_pool_tb_per_s": tb(1, t8), "kv16_pool_tb_per_s": tb(2, t16), "fp32_pool_tb_per_s": tb(4, t32)}
        rec.update(_side("fp8_pool", t8))
        rec.update(_side("kv16_pool", t16))
        rec.update(_side("fp32_pool", t32))
        print(f"{batch:3d} x {seq_q:2d} / {seq_kv:5d}{' ragged' if ragged else ''} x {heads} / {kv_heads} x {hd} {mode:4s} causal {causal} S {S}: "
              f"fp8 pool {t8[0]:8.4f} ms [{t8[2]:.4f} .. {t8[3]:.4f}] {rec['fp8_pool_tb_per_s']:.2f} TB/s | {kv} pool {t16[0]:8.4f} ms [{t16[2]:.4f} .. {t16[3]:.4f}] "
              f"{rec['kv16_pool_tb_per_s']:.2f} TB/s | fp32 pool {t32[0]:8.4f} ms {rec['fp32_pool_tb_per_s']:.2f} TB/s | x{rec['fp8_over_kv16']:.3f} of 16-bit, "
              f"below its lowest round {rec['fp8_below_lowest_kv16_round_median']} bits {rec['same_bits_as_kv16_times_v_scale']}", flush=True)
    finally:
        ops.set_compute("f32")
    del q, pools8, pools16, pools32, outs
    torch.cuda.empty_cache()
    return [rec]


def bench_kv_append(row, kv):
    """brn_kv_cache_append (rows + lengths, in place; kv "fp8": brn_kv_cache_append_fp8 with per-head scales) beside a device-to-device
    copy of the bytes it writes, the bandwidth floor"""
    import torch
    import candle_birefnet_amd as cb
    lib = cb._ffi.lib
    batch, seq_new, kv_heads, hd, page, pages_per_seq = row
    tdt = {"f32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16, "fp8": torch.uint8}[kv]
    g = torch.Generator(device="cuda").manual_seed(2)
    k_new, v_new = (torch.randn(batch, seq_new, kv_heads, hd, device="cuda", generator=g) for _ in range(2))
    n_pages = batch * pages_per_seq
    kp, vp = (torch.zeros(n_pages, page, kv_heads, hd, device="cuda", dtype=tdt) for _ in range(2))
    table = torch.randperm(n_pages, device="cuda", generator=g).to(torch.int32).view(batch, pages_per_seq).contiguous()
    start = torch.full((batch,), page * pages_per_seq // 2 - 1, dtype=torch.int32, device="cuda")       # the first token lands on a page's last row
    lens = start.clone()
    stream = torch.cuda.current_stream().cuda_stream
    src, dst = (torch.empty(2 * batch * seq_new * kv_heads * hd, device="cuda", dtype=tdt) for _ in range(2))

    scales = [torch.full((kv_heads,), 0.0173, device="cuda") for _ in range(2)]

    def append():
        lens.copy_(start)
        if kv == "fp8":
            cb._ffi.check(lib.brn_kv_cache_append_fp8(k_new.data_ptr(), v_new.data_ptr(), batch, seq_new, kv_heads, hd, 0, kp.data_ptr(), vp.data_ptr(), scales[0].data_ptr(),
                                                      scales[1].data_ptr(), table.data_ptr(), lens.data_ptr(), lens.data_ptr(), n_pages, page, pages_per_seq, 1, 0, stream))
            return kp
        cb._ffi.check(lib.brn_kv_cache_append(k_new.data_ptr(), v_new.data_ptr(), batch, seq_new, kv_heads, hd, 0, kp.data_ptr(), vp.data_ptr(),
                                              {"f32": 0, "bf16": 1, "f16": 2}[kv], table.data_ptr(), lens.data_ptr(), lens.data_ptr(), n_pages, page, pages_per_seq, 1, 0, stream))
        return kp

    def copy():
        lens.copy_(start)
        dst.copy_(src)
        return dst

    ta, tc = _time_alternating([append, copy])
    rec = {"batch": batch, "seq_new": seq_new, "kv_heads": kv_heads, "head_dim": hd, "page_size": page, "kv_type": kv, "bytes_written": src.numel() * src.element_size(),
           "bytes_read": 2 * 4 * batch * seq_new * kv_heads * hd, "append_over_copy": round(ta[0] / tc[0], 3), "note": "both sides include one copy of the lengths (batch ints)"}
    rec.update(_side("append", ta))
    rec.update(_side("copy", tc))
    print(f"append {batch:3d} x {seq_new:3d} x {kv_heads} x {hd} -> {kv:4s}: {ta[0]:.4f} ms [{ta[2]:.4f} .. {ta[3]:.4f}] | copy of {rec['bytes_written']} bytes {tc[0]:.4f} ms "
          f"[{tc[2]:.4f} .. {tc[3]:.4f}] x{rec['append_over_copy']:.2f}", flush=True)
    return [rec]


def bench_rope(row, kv):
    """brn_kv_cache_append_rope (kv "fp8": _rope_fp8) beside the plain append, the two-call form rope(k_new) -> append and a
    device-to-device copy of the bytes written; all sides rewind the lengths first"""
    import torch
    import candle_birefnet_amd as cb
    from candle_birefnet_amd import ops
    lib = cb._ffi.lib
    batch, seq_new, kv_heads, hd, page, pages_per_seq = row
    tdt = {"f32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16, "fp8": torch.uint8}[kv]
    g = torch.Generator(device="cuda").manual_seed(2)
    k_new, v_new = (torch.randn(batch, seq_new, kv_heads, hd, device="cuda", generator=g) for _ in range(2))
    k_rot = torch.empty_like(k_new)
    n_pages = batch * pages_per_seq
    kp, vp = (torch.zeros(n_pages, page, kv_heads, hd, device="cuda", dtype=tdt) for _ in range(2))
    table = torch.randperm(n_pages, device="cuda", generator=g).to(torch.int32).view(batch, pages_per_seq).contiguous()
    start = torch.full((batch,), page * pages_per_seq // 2 - 1, dtype=torch.int32, device="cuda")
    lens = start.clone()
    n_pos = page * pages_per_seq
    cos, sin = (torch.from_numpy(a).cuda() for a in ops.rope_table(n_pos, hd))
    stream = torch.cuda.current_stream().cuda_stream
    src, dst = (torch.empty(2 * batch * seq_new * kv_heads * hd, device="cuda", dtype=tdt) for _ in range(2))
    scales = [torch.full((kv_heads,), 0.0173, device="cuda") for _ in range(2)]
    head = (batch, seq_new, kv_heads, hd, 0)
    rope_args = (cos.data_ptr(), sin.data_ptr(), n_pos, hd, 0)
    pool = (kp.data_ptr(), vp.data_ptr()) + ((scales[0].data_ptr(), scales[1].data_ptr()) if kv == "fp8" else ({"f32": 0, "bf16": 1, "f16": 2}[kv],))
    tail = (table.data_ptr(), lens.data_ptr(), lens.data_ptr(), n_pages, page, pages_per_seq, 1, 0, stream)
    plain_fn, rope_fn = (lib.brn_kv_cache_append_fp8, lib.brn_kv_cache_append_rope_fp8) if kv == "fp8" else (lib.brn_kv_cache_append, lib.brn_kv_cache_append_rope)

    def fused():
        lens.copy_(start)
        cb._ffi.check(rope_fn(k_new.data_ptr(), v_new.data_ptr(), *head, *rope_args, *pool, *tail))
        return kp

    def plain():
        lens.copy_(start)
        cb._ffi.check(plain_fn(k_new.data_ptr(), v_new.data_ptr(), *head, *pool, *tail))
        return kp

    def two_calls():
        lens.copy_(start)
        cb._ffi.check(lib.brn_rope_forward(k_new.data_ptr(), *head, *rope_args, lens.data_ptr(), k_rot.data_ptr(), 1, 0, stream))
        cb._ffi.check(plain_fn(k_rot.data_ptr(), v_new.data_ptr(), *head, *pool, *tail))
        return kp

    def copy():
        lens.copy_(start)
        dst.copy_(src)
        return dst

    two_calls()
    want = kp.clone()
    kp.zero_()
    fused()
    torch.cuda.synchronize()
    bits_equal = bool(torch.equal(kp.view(torch.uint8), want.view(torch.uint8)))
    tf, tp, t2, tc = _time_alternating([fused, plain, two_calls, copy])
    written = src.numel() * src.element_size()
    read = 2 * 4 * batch * seq_new * kv_heads * hd
    rec = {"batch": batch, "seq_new": seq_new, "kv_heads": kv_heads, "head_dim": hd, "page_size": page, "kv_type": kv, "style": "half", "rot_dim": hd, "bytes_written": written,
           "bytes_read": read, "fused_bits_equal_two_calls": bits_equal, "fused_over_plain": round(tf[0] / tp[0], 3), "two_calls_over_plain": round(t2[0] / tp[0], 3),
           "fused_over_copy": round(tf[0] / tc[0], 3), "fused_bytes_per_s": round((read + written) / (tf[0] * 1e-3), 0), "plain_bytes_per_s": round((read + written) / (tp[0] * 1e-3), 0),
           "two_calls_bytes_per_s": round((read + written + read) / (t2[0] * 1e-3), 0), "copy_bytes_per_s": round(2 * written / (tc[0] * 1e-3), 0),
           "note": "every side includes one copy of the lengths (batch ints); bytes per second count reads + writes (the two-call form moves k_new three times)"}
    for name, t in (("append_rope", tf), ("append", tp), ("rope_then_append", t2), ("copy", tc)):
        rec.update(_side(name, t))
    print(f"rope {batch:3d} x {seq_new:3d} x {kv_heads} x {hd} -> {kv:4s}: fused {tf[0]:.4f} ms [{tf[2]:.4f} .. {tf[3]:.4f}] | append {tp[0]:.4f} [{tp[2]:.4f} .. {tp[3]:.4f}] | "
          f"rope + append {t2[0]:.4f} [{t2[2]:.4f} .. {t2[3]:.4f}] | copy {tc[0]:.4f} [{tc[2]:.4f} .. {tc[3]:.4f}] | bits equal {bits_equal}", flush=True)
    return [rec]


def bench_paged_varlen(row, kv_splits=0):
    """brn_flash_attention_paged_varlen_forward on a packed batch beside the existing entry (brn_flash_attention_paged_kv_forward, the
    parent's kernels) on the same work: one call per group of sequences with the same number of new tokens.  bf16 pool, bf16 compute,
    causal, page 64, shuffled table; every record also says whether the packed rows equal the existing entry's, bit for bit"""
    import torch
    import candle_birefnet_amd as cb
    from candle_birefnet_amd import ops
    lib = cb._ffi.lib
    name, pack, groups = row
    heads, kv_heads, hd, page = PAGED_VARLEN_SHAPE
    n_seqs, total_q, max_kv = len(pack), sum(n for n, _ in pack), max(L for _, L in pack)
    max_pages = (max_kv + page - 1) // page
    n_pages = n_seqs * max_pages
    g = torch.Generator(device="cuda").manual_seed(1)
    q = torch.randn(total_q, heads, hd, device="cuda", generator=g)
    pools = [torch.randn(n_pages, page, kv_heads, hd, device="cuda", generator=g).to(torch.bfloat16) for _ in range(2)]
    table = torch.randperm(n_pages, device="cuda", generator=g).to(torch.int32).view(n_seqs, max_pages).contiguous()
    lens = torch.tensor([L for _, L in pack], dtype=torch.int32, device="cuda")
    cu_h = [0]
    for n, _ in pack:
        cu_h.append(cu_h[-1] + n)
    cu = torch.tensor(cu_h, dtype=torch.int32, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream
    S, tps, need, npl = ops.flash_attention_paged_varlen_plan(total_q, n_seqs, max_kv, heads, kv_heads, hd, kv_splits)
    y, lse, ws, plan = torch.empty_like(q), torch.empty(heads * total_q, device="cuda"), torch.empty(max(need, 4), device="cuda"), torch.empty(npl, dtype=torch.int32, device="cuda")

    def packed():
        cb._ffi.check(lib.brn_flash_attention_paged_varlen_forward(q.data_ptr(), pools[0].data_ptr(), pools[1].data_ptr(), cb._ffi.BRN_POOL_BF16, None, None, table.data_ptr(),
                                                                   lens.data_ptr(), cu.data_ptr(), total_q, n_seqs, max_kv, heads, kv_heads, hd, n_pages, page, max_pages, 1, 0.0,
                                                                   kv_splits, y.data_ptr(), lse.data_ptr(), ws.data_ptr(), need, plan.data_ptr(), npl, 1, 0, stream))
        return y

    # the existing entry: the groups' rows of q, table and lens are contiguous slices of the pack's
    calls, at, seq_at = [], 0, 0
    for batch, seq_q in groups:
        assert all(n == seq_q for n, _ in pack[seq_at:seq_at + batch])
        gS, _, gneed = ops.flash_attention_splitkv_plan(batch, seq_q, max_kv, heads, kv_heads, hd, kv_splits)
        gy = torch.empty(batch, seq_q, heads, hd, device="cuda")
        calls.append((q[at:at + batch * seq_q], table[seq_at:seq_at + batch], lens[seq_at:seq_at + batch], batch, seq_q, gy, torch.empty(batch * heads * seq_q, device="cuda"),
                      torch.empty(max(gneed, 4), device="cuda"), gneed, gS))
        at += batch * seq_q
        seq_at += batch

    def existing():
        for gq, gt, gl, batch, seq_q, gy, glse, gws, gneed, _ in calls:
            cb._ffi.check(lib.brn_flash_attention_paged_kv_forward(gq.data_ptr(), pools[0].data_ptr(), pools[1].data_ptr(), cb._ffi.BRN_KV_BF16, gt.data_ptr(), gl.data_ptr(), batch,
                                                                   seq_q, max_kv, heads, kv_heads, hd, n_pages, page, max_pages, 0, 1, 0.0, kv_splits, gy.data_ptr(), glse.data_ptr(),
                                                                   gws.data_ptr(), gneed, 1, 0, stream))
        return torch.cat([c[5].reshape(-1, heads, hd) for c in calls])

    ops.set_compute("bf16")
    try:
        te, tp = _time_alternating([existing, packed])
        same = bool(torch.equal(te[4], tp[4])) if all(c[9] == S for c in calls) or kv_splits else None      # the bits are promised at the same explicit kv_splits
        keys = sum(L for _, L in pack) * kv_heads * hd
        rec = {"row": name, "total_q": total_q, "n_seqs": n_seqs, "max_kv_len": max_kv, "heads": heads, "kv_heads": kv_heads, "head_dim": hd, "mode": "bf16", "pool": "bf16",
               "page_size": page, "table": "shuffled", "causal": 1, "kv_splits": kv_splits, "S": S, "tiles_per_split": tps, "existing_calls": [(c[3], c[4], c[9]) for c in calls],
               "packed_over_existing": round(tp[0] / te[0], 4), "packed_below_highest_existing_round_median": bool(tp[0] < te[3]), "same_bits": same,
               "kv_bytes": 2 * 2 * keys, "packed_y_sha1": __import__("hashlib").sha1(tp[4].cpu().numpy().tobytes()).hexdigest()[:16]}
        rec.update(_side("existing", te))
        rec.update(_side("packed", tp))
        print(f"{name}, kv_splits {kv_splits}: existing {len(calls)} call(s) (S {[c[9] for c in calls]}) {te[0]:8.4f} ms [{te[2]:.4f} .. {te[3]:.4f}] | packed (S {S}) {tp[0]:8.4f} ms "
              f"[{tp[2]:.4f} .. {tp[3]:.4f}] x{rec['packed_over_existing']:.3f} bits {same} y {rec['packed_y_sha1']}", flush=True)
    finally:
        ops.set_compute("f32")
    del q, pools, calls
    torch.cuda.empty_cache()
    return [rec]


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--bias", action="store_true", help="time brn_flash_attention_bias_forward beside the bias-free call and torch + bias")
    ap.add_argument("--gqa", action="store_true", help="time brn_flash_attention_gqa_forward beside the older entries on repeated K / V (and a -inf mask bias)")
    ap.add_argument("--varlen", action="store_true", help="time brn_flash_attention_varlen_forward: windows, a ragged pack, a uniform pack, beside the gqa entry")
    ap.add_argument("--splitkv", action="store_true", help="time brn_flash_attention_splitkv_forward at kv_splits 1 .. 64 and 0 beside the gqa entry")
    ap.add_argument("--paged", action="store_true", help="time brn_flash_attention_paged_forward (pages of 16 / 64 / 256, identity and shuffled tables) beside the split entry")
    ap.add_argument("--paged-kv16", action="store_true", help="time brn_flash_attention_paged_kv_forward on 16-bit pools beside the fp32-pool entry, and brn_kv_cache_append beside a copy")
    ap.add_argument("--paged-fp8", action="store_true", help="time brn_flash_attention_paged_fp8_forward on an e4m3 pool beside the 16-bit-pool and fp32-pool entries, and brn_kv_cache_append_fp8 beside a copy")
    ap.add_argument("--rope", action="store_true", help="time brn_kv_cache_append_rope beside the plain append, rope + append in two calls, and a copy")
    ap.add_argument("--paged-varlen", action="store_true", help="time brn_flash_attention_paged_varlen_forward (a mixed prefill / decode step, a pure decode step) beside the existing paged entry called per group; every row is printed twice")
    ap.add_argument("--row", type=int, choices=range(len(BIAS_ROWS)))
    ap.add_argument("--mode", choices=MODES)
    ap.add_argument("--json", help="write the records to this file")
    a = ap.parse_args()
    import candle_birefnet_amd as cb
    if cb.device_count() < 1:
        sys.exit("no HIP device: nothing is measured")
    recs = []
    if a.bias + a.gqa + a.varlen + a.splitkv + a.paged + a.paged_kv16 + a.paged_fp8 + a.rope + a.paged_varlen > 1:
        sys.exit("--bias, --gqa, --varlen, --splitkv, --paged, --paged-kv16, --paged-fp8, --rope and --paged-varlen are separate tables: one at a time")
    if a.paged_varlen:
        for row in (PAGED_VARLEN_ROWS if a.row is None else [PAGED_VARLEN_ROWS[a.row]] if a.row < len(PAGED_VARLEN_ROWS) else sys.exit(f"--row {a.row}: only {len(PAGED_VARLEN_ROWS)} rows in this table")):
            for ks in (0, 0, 1, 2, 4, 4):            # the automatic rule and kv_splits 4 twice: a repeated row must repeat its result
                recs += bench_paged_varlen(row, ks)
        with open(a.json or PAGED_VARLEN_JSON, "w") as f:
            json.dump({"tool": "tools/bench_flash_attention.py --paged-varlen", "warmup": GQA_WARMUP, "timed": GQA_ROUNDS * GQA_TIMED, "rows": recs}, f, indent=1)
            f.write("\n")
        sys.exit(0)
    if a.rope:
        for row in (KV_APPEND_ROWS if a.row is None else [KV_APPEND_ROWS[a.row]] if a.row < len(KV_APPEND_ROWS) else sys.exit(f"--row {a.row}: only {len(KV_APPEND_ROWS)} rows in this table")):
            for kv in KV_APPEND_TYPES + ["fp8"]:
                recs += bench_rope(row, kv)
        with open(a.json or ROPE_JSON, "w") as f:
            json.dump({"tool": "tools/bench_flash_attention.py --rope", "warmup": GQA_WARMUP, "timed": GQA_ROUNDS * GQA_TIMED, "rows": recs}, f, indent=1)
            f.write("\n")
        sys.exit(0)
    if a.paged_fp8:
        for row in (PAGED_ROWS if a.row is None else [PAGED_ROWS[a.row]] if a.row < len(PAGED_ROWS) else sys.exit(f"--row {a.row}: only {len(PAGED_ROWS)} rows in this table")):
            for mode in (["bf16", "f16", "f32"] if a.mode is None else [a.mode]):
                recs += bench_paged_fp8(row, mode)
        appends = []
        if a.row is None:
            for row in KV_APPEND_ROWS:
                appends += bench_kv_append(row, "fp8")
        with open(a.json or PAGED_FP8_JSON, "w") as f:
            json.dump({"tool": "tools/bench_flash_attention.py --paged-fp8", "warmup": GQA_WARMUP, "timed": GQA_ROUNDS * GQA_TIMED, "rows": recs, "append": appends}, f, indent=1)
            f.write("\n")
        sys.exit(0)
    if a.paged_kv16:
        for row in (PAGED_ROWS if a.row is None else [PAGED_ROWS[a.row]] if a.row < len(PAGED_ROWS) else sys.exit(f"--row {a.row}: only {len(PAGED_ROWS)} rows in this table")):
            for pair in PAGED_KV16_PAIRS:
                if a.mode is None or pair[0] == a.mode:
                    recs += bench_paged_kv16(row, pair)
        appends = []
        if a.row is None:
            for row in KV_APPEND_ROWS:
                for kv in KV_APPEND_TYPES:
                    appends += bench_kv_append(row, kv)
        with open(a.json or PAGED_KV16_JSON, "w") as f:
            json.dump({"tool": "tools/bench_flash_attention.py --paged-kv16", "warmup": GQA_WARMUP, "timed": GQA_ROUNDS * GQA_TIMED, "rows": recs, "append": appends}, f, indent=1)
            f.write("\n")
        sys.exit(0)
    rows = BIAS_ROWS if a.bias else GQA_ROWS if a.gqa else VARLEN_GROUPS if a.varlen else SPLITKV_ROWS if a.splitkv else PAGED_ROWS if a.paged else ROWS
    if a.row is not None and a.row >= len(rows):
        sys.exit(f"--row {a.row}: only {len(rows)} rows in this table")
    for row in (rows if a.row is None else [rows[a.row]]):
        for mode in ((SPLITKV_MODES if a.splitkv or a.paged else MODES) if a.mode is None else [a.mode]):
            recs += (bench_bias(row, mode) if a.bias else bench_gqa(row, mode) if a.gqa else bench_varlen(row, mode) if a.varlen else
                     bench_splitkv(row, mode) if a.splitkv else bench_paged(row, mode) if a.paged else bench(row, mode))
    if a.splitkv and not a.json:
        a.json = SPLITKV_JSON
    if a.paged and not a.json:
        a.json = PAGED_JSON
    if a.json:
        with open(a.json, "w") as f:
            alternating = a.gqa or a.varlen or a.splitkv or a.paged
            json.dump({"tool": "tools/bench_flash_attention.py" + (" --bias" if a.bias else " --gqa" if a.gqa else " --varlen" if a.varlen else " --splitkv" if a.splitkv else
                                                                     " --paged" if a.paged else ""),
                       "warmup": GQA_WARMUP if alternating else WARMUP, "timed": GQA_ROUNDS * GQA_TIMED if alternating else TIMED, "rows": recs}, f, indent=1)
            f.write("\n")
