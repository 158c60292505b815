#!/usr/bin/env python3
"""kvp_kvzap_score CALL times on the GPU (hipEvent medians over warmed-up windows of 0.25 s of back-to-back calls) at the Llama-3.1-8B
geometry of one KVzap layer -- B 1, hidden 4096, hidden_dim 512, 8 kv heads, bf16 -- for a 32k and a 128k prefill and for one decoding
step (S = 1), next to

  * a torch restatement of the expression the reference evaluates per layer and forward (kvzap_press.py:79-81 with the mlp body :38-45:
    F.linear -> gelu -> F.linear -> transpose), written for this tool, on the same GPU in the same process, the two taking turns;
  * the modelled floor of the prefill sizes: the FLOP of both layers at the bf16 matrix peak (16 x the 157.3 TFLOPS float32 matrix rate).

Also recorded: the peak transient device memory of one call of each (torch.cuda.max_memory_allocated over the call, minus what was
allocated before it, the result included) and the worst difference between the two results in units of the contract's scale (the
baseline rounds its activations and its result to bf16: a sanity comparison only).  ``--linear`` adds the linear surrogate.

    python tools/kvzap_lab.py [--reps 7] [--out profiles/kvzap_lab.json]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from kvzip_lab import BF16_MATRIX_PEAK, peak_transient_bytes, timed  # noqa: E402  (the same timing and memory probes)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7, help="timed windows of 0.25 s per function")
    ap.add_argument("--sizes", type=int, nargs="+", default=[32768, 131072, 1])
    ap.add_argument("--linear", action="store_true", help="also time the linear surrogate")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    import torch.nn.functional as F

    from kvpress_amd import _native

    assert torch.cuda.is_available(), "kvzap_lab needs a GPU"
    dev, dt = "cuda", torch.bfloat16
    B, K, N, Hout = 1, 4096, 512, 8
    gen = torch.Generator(device=dev).manual_seed(0)

    def uniform(*shape, fan_in):
        return ((torch.rand(shape, device=dev, generator=gen) * 2 - 1) / fan_in ** 0.5).to(dt)

    w1, b1, w2, b2 = uniform(N, K, fan_in=K), uniform(N, fan_in=K), uniform(Hout, N, fan_in=N), uniform(Hout, fan_in=N)
    wl, bl = uniform(Hout, K, fan_in=K), uniform(Hout, fan_in=K)
    results = []
    for model in ["mlp"] + (["linear"] if args.linear else []):
        for S in args.sizes:
            x = torch.randn((B, S, K), device=dev, generator=gen).to(dt)
            if model == "mlp":
                def library():
                    return _native.kvzap_score(x, w1, b1, w2, b2)

                def torch_expression():
                    return F.linear(F.gelu(F.linear(x, w1, b1)), w2, b2).transpose(1, 2)
                flop = 2.0 * B * S * (K * N + N * Hout)
                scale = (x.float().abs() @ w1.float().abs().t() + b1.float().abs()) @ w2.float().abs().t() + b2.float().abs()
            else:
                def library():
                    return _native.kvzap_score(x, wl, bl)

                def torch_expression():
                    return F.linear(x, wl, bl).transpose(1, 2)
                flop = 2.0 * B * S * K * Hout
                scale = x.float().abs() @ wl.float().abs().t() + bl.float().abs()
            got, ref = library(), torch_expression()
            diff = float(((got - ref.float()).abs() / scale.transpose(1, 2)).max())
            del scale
            mem_lib, mem_torch = peak_transient_bytes(library), peak_transient_bytes(torch_expression)
            r_lib, r_torch = timed([library, torch_expression], args.reps)
            r_lib.update(flop=flop, floor_ms=flop / BF16_MATRIX_PEAK * 1e3, achieved_tflops=flop / (r_lib["median_ms"] * 1e-3) / 1e12,
                         peak_transient_bytes=mem_lib)
            r_lib["fraction_of_bf16_matrix_peak"] = r_lib["floor_ms"] / r_lib["median_ms"]   # from the CALL time
            r_torch.update(peak_transient_bytes=mem_torch, achieved_tflops=flop / (r_torch["median_ms"] * 1e-3) / 1e12)
            results.append(dict(model=model, S=S, kernel=r_lib, torch_expression=r_torch, torch_over_kernel=r_torch["median_ms"] / r_lib["median_ms"],
                                max_diff_to_bf16_baseline_over_scale=diff))
            del x, got, ref
    out = {"geometry": dict(B=B, K=K, N=N, Hout=Hout, dtype="bf16"), "device": torch.cuda.get_device_name(0), "results": results}
    line = json.dumps(out)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
