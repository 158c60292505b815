#!/usr/bin/env python3
"""kvp_vwl1norm_rescale CALL times on the GPU (hipEvent medians over warmed-up windows of 0.25 s of back-to-back calls), Llama-3.1-8B
geometry (B 1, Hq 32, Hkv 8, D 128, hidden 4096, bf16) at S = 32768 and S = 131072, next to

  * the plain per-head torch expression the reference evaluates, ``(V_h @ Wo_h).abs().sum(-1)`` for every query head, mean over the
    group (criticalkv_press.py:57-76), on the same GPU in the same process, the two taking turns;
  * the modelled floor 2 * S * D * hidden * Hq FLOP at the bf16 matrix peak (16 x the 157.3 TFLOPS float32 matrix rate).

    python tools/critical_lab.py [--reps 7] [--out profiles/critical_lab.json]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
BF16_MATRIX_PEAK = 16 * 157.3e12   # FLOP / s


def timed(fns, reps, warmup=2, window_s=0.25):
    """median / min milliseconds per CALL of each function of ``fns`` (a call through the Python binding: the ctypes call and the
    allocation of the output included, not a kernel time).  A timed window is as many back-to-back calls between a pair of events as
    fill ``window_s`` seconds (sized from the warm-up calls), the functions taking turns from window to window."""
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7, help="timed windows of 0.25 s per function and size")
    ap.add_argument("--sizes", default="32768,131072")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch

    from kvpress_amd import _native

    assert torch.cuda.is_available(), "critical_lab needs a GPU"
    dev, dt = "cuda", torch.bfloat16
    B, Hq, Hkv, D, hidden = 1, 32, 8, 128, 4096
    G = Hq // Hkv
    gen = torch.Generator(device=dev).manual_seed(0)
    wo = (torch.randn((hidden, Hq * D), device=dev, generator=gen) / 64).to(dt)
    out = {"geometry": dict(B=B, Hq=Hq, Hkv=Hkv, D=D, hidden=hidden, dtype="bf16"), "device": torch.cuda.get_device_name(0)}
    for S in [int(x) for x in args.sizes.split(",")]:
        values = torch.randn((B, Hkv, S, D), device=dev, generator=gen).to(dt)
        wo_heads = wo.t().reshape(Hq, D, hidden)   # criticalkv_press.py:61-62

        def torch_per_head():
            heads = [(values[:, h // G] @ wo_heads[h]).abs().sum(-1) for h in range(Hq)]
            return torch.stack(heads, dim=1).view(B, Hkv, G, S).mean(dim=2)

        ref = torch_per_head().float()
        got = _native.vwl1norm(values, wo, Hq)
        # the baseline rounds every [S, hidden] product and its sum to bf16: a sanity comparison only
        out_of_line = float(((got - ref).abs() / ref).max())
        r_lib, r_torch = timed([lambda: _native.vwl1norm(values, wo, Hq), torch_per_head], args.reps)
        flop = 2.0 * B * S * D * hidden * Hq
        r_lib.update(flop=flop, floor_ms=flop / BF16_MATRIX_PEAK * 1e3, achieved_tflops=flop / (r_lib["median_ms"] * 1e-3) / 1e12)
        r_lib["floor_over_call_time"] = r_lib["floor_ms"] / r_lib["median_ms"]   # of the bf16 matrix peak, from the CALL time
        out[f"S{S}"] = dict(kernel=r_lib, torch_per_head=r_torch, torch_over_kernel=r_torch["median_ms"] / r_lib["median_ms"],
                            max_rel_diff_to_bf16_baseline=out_of_line)
        del values, ref, got
    line = json.dumps(out)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
