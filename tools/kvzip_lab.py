#!/usr/bin/env python3
"""kvp_kvzip_score CALL times on the GPU (hipEvent medians over warmed-up windows of 0.25 s of back-to-back calls) at the Llama-3.1-8B
geometry of one KVzip chunk -- B 1, Hq 32, Hkv 8, D 128, bf16, chunk 2048, Lq = chunk + the prompt's length, sink 4, the chunk in the
middle of a 128k cache -- next to

  * a torch restatement of the expression the reference evaluates per layer and chunk (kvzip_press.py:312-354: RoPE, the concatenated
    [sink | chunk | repeat] keys, the stored softmax of [Hkv, G, Lq, sink + chunk + Lq], the causal mask added to it, the slice, the amax),
    written for this tool, on the same GPU in the same process, the two taking turns;
  * the modelled floor: the FLOP of both passes (QK^T over the keys below the causal diagonal, then over the chunk again) at the bf16
    matrix peak (16 x the 157.3 TFLOPS float32 matrix rate).

Also recorded: the peak transient device memory of one call of each (torch.cuda.max_memory_allocated over the call, minus what was
allocated before it) and the worst relative difference between the two results (the baseline rounds its logits and its softmax to bf16:
a sanity comparison only).

    python tools/kvzip_lab.py [--reps 7] [--out profiles/kvzip_lab.json]
"""
import argparse
import json
import math
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
BF16_MATRIX_PEAK = 16 * 157.3e12   # FLOP / s


def timed(fns, reps, warmup=2, window_s=0.25):
    """median / min milliseconds per CALL of each function of ``fns`` (the ctypes call and the allocations included).  A timed window is
    as many back-to-back calls between a pair of events as fill ``window_s`` seconds (sized from the warm-up calls), the functions taking
    turns from window to window."""
    import torch

    def window(fn, calls):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(calls):
            fn()
        b.record()
        b.synchronize()
        return a.elapsed_time(b) / calls

    calls = []
    for fn in fns:
        for _ in range(warmup):
            ms = window(fn, 1)
        calls.append(max(1, int(window_s * 1e3 / ms + 0.5)))
    times = [[] for _ in fns]
    for _ in range(reps):
        for i, fn in enumerate(fns):
            times[i].append(window(fn, calls[i]))
    return [dict(median_ms=statistics.median(x), min_ms=min(x), max_ms=max(x), windows=reps, calls_per_window=c) for x, c in zip(times, calls)]


def peak_transient_bytes(fn):
    import torch

    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    out = fn()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - before
    del out
    return int(peak)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7, help="timed windows of 0.25 s per function")
    ap.add_argument("--context", type=int, default=131072)
    ap.add_argument("--chunk", type=int, default=2048)
    ap.add_argument("--prompt", type=int, default=22, help="tokens of the repeat prompt in front of the chunk (prompt + 8 of the previous chunk + template)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch

    from kvpress_amd import _native

    assert torch.cuda.is_available(), "kvzip_lab needs a GPU"
    dev, dt = "cuda", torch.bfloat16
    B, Hq, Hkv, D, sink = 1, 32, 8, 128, 4
    G, Lq, C = Hq // Hkv, args.chunk + args.prompt, args.context
    start = (C // 2) // args.chunk * args.chunk
    end, S = start + args.chunk, C + Lq
    gen = torch.Generator(device=dev).manual_seed(0)
    keys = torch.randn((B, Hkv, S, D), device=dev, generator=gen).to(dt)
    q_pre = torch.randn((B, Lq, Hq, D), device=dev, generator=gen).to(dt).transpose(1, 2)     # q_proj's layout
    pos = torch.arange(C, S, device=dev, dtype=torch.float32)
    inv = 1.0 / (500000.0 ** (torch.arange(0, D, 2, device=dev, dtype=torch.float32) / D))
    ang = torch.cat([pos[:, None] * inv, pos[:, None] * inv], dim=-1)[None]
    cos, sin = ang.cos().to(dt), ang.sin().to(dt)

    def library():
        return _native.kvzip_score(q_pre, cos, sin, keys, sink, start, end)

    def torch_expression():
        half = D // 2
        rot = torch.cat((-q_pre[..., half:], q_pre[..., :half]), dim=-1)
        q = (q_pre * cos.unsqueeze(1) + rot * sin.unsqueeze(1)).reshape(B, Hkv, G, Lq, D)
        sub = torch.cat([keys[:, :, :sink], keys[:, :, start:end], keys[:, :, S - Lq:]], dim=2)
        w = torch.matmul(q, sub.unsqueeze(2).transpose(-2, -1).contiguous()) / math.sqrt(D)
        causal = torch.full((Lq, Lq), torch.finfo(w.dtype).min, device=dev, dtype=w.dtype).triu(1)
        w[..., -Lq:] += causal
        w = torch.softmax(w, dim=-1)
        return w[..., sink:sink + (end - start)].amax(dim=(-3, -2)).float()

    got, ref = library(), torch_expression()
    diff = float(((got - ref).abs() / ref.abs().clamp_min(1e-30)).max())
    mem_lib, mem_torch = peak_transient_bytes(library), peak_transient_bytes(torch_expression)
    r_lib, r_torch = timed([library, torch_expression], args.reps)
    n = end - start
    flop = 2.0 * D * Hq * (Lq * (sink + n) + Lq * (Lq + 1) / 2 + Lq * n)      # pass 1 below the diagonal + pass 2 over the chunk
    r_lib.update(flop=flop, floor_ms=flop / BF16_MATRIX_PEAK * 1e3, achieved_tflops=flop / (r_lib["median_ms"] * 1e-3) / 1e12,
                 peak_transient_bytes=mem_lib)
    r_lib["floor_over_call_time"] = r_lib["floor_ms"] / r_lib["median_ms"]   # of the bf16 matrix peak, from the CALL time
    r_torch.update(peak_transient_bytes=mem_torch)
    out = {"geometry": dict(B=B, Hq=Hq, Hkv=Hkv, D=D, dtype="bf16", context=C, chunk=args.chunk, Lq=Lq, sink=sink, start=start),
           "device": torch.cuda.get_device_name(0), "kernel": r_lib, "torch_expression": r_torch,
           "torch_over_kernel": r_torch["median_ms"] / r_lib["median_ms"], "max_rel_diff_to_bf16_baseline": diff}
    line = json.dumps(out)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
