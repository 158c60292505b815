#!/usr/bin/env python3
"""kvp_fastkvzip_score CALL times on the GPU (hipEvent medians over warmed-up windows of 0.25 s of back-to-back calls) at the Qwen3-8B
geometry of one FastKVzip gate -- B 1, hidden 4096, 8 kv heads, 4 query heads each, output_dim 16, 16 sink keys, bf16 -- for a 32k and a
128k prefill, next to

  * a torch restatement of what the gate evaluates per layer (fastkvzip_press.py:54-71 and the protected positions of :240-247: two
    F.linear, two RMSNorms, two batched matmuls, exp, sum, mean), written for this tool, on the same GPU in the same process, the two
    taking turns;
  * the vendor GEMM alone: one F.linear of the hidden states with the 640 stacked weight rows;
  * the modelled floor: the FLOP of both projections at the bf16 matrix peak.

Also recorded: the peak transient device memory of one call of each (the result included), the worst difference between the two results,
and the library's call time forced onto each of its two geometries (KVP_FASTKVZIP_GEO: 1 = 512 weight rows a workgroup in K tiles of 64,
two groups of 4 heads here; 2 = 640 rows in K tiles of 32, all 8 heads in one group) and onto groups of 2 heads and of 1 head (KVP_FASTKVZIP_HEADS).

    python tools/fastkvzip_lab.py [--reps 7] [--out profiles/fastkvzip_lab.json]
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
    ap.add_argument("--sizes", type=int, nargs="+", default=[32768, 131072])
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    import torch.nn.functional as F

    from kvpress_amd import _native

    assert torch.cuda.is_available(), "fastkvzip_lab needs a GPU"
    dev, dt = "cuda", torch.bfloat16
    B, K, Hkv, G, D, J, eps, n_sink, window = 1, 4096, 8, 4, 16, 16, 1e-6, 4, 4096
    gen = torch.Generator(device=dev).manual_seed(0)

    def uniform(*shape):
        return ((torch.rand(shape, device=dev, generator=gen) * 2 - 1) / K ** 0.5).to(dt)

    wq, bq, wk = uniform(Hkv * G * D, K), uniform(Hkv * G * D), uniform(Hkv * D, K)
    b = (0.5 * torch.randn((Hkv, G), device=dev, generator=gen)).to(dt)
    gq, gk = (0.5 + torch.rand(D, device=dev, generator=gen) for _ in range(2))
    kb = 0.5 * torch.randn((Hkv, J, D), device=dev, generator=gen)
    w_all = torch.cat([wq, wk])

    def rmsnorm(v, g):
        f = v.float()
        return g * (f * torch.rsqrt(f.pow(2).mean(-1, keepdim=True) + eps)).to(v.dtype)

    results = []
    for S in args.sizes:
        x = torch.randn((B, S, K), device=dev, generator=gen).to(dt)
        tail = int(S * 0.02) if S < 32000 else window

        def library():
            return _native.fastkvzip_score(x, wq, bq, wk, b, gq, gk, kb, eps, n_sink, tail)

        def torch_expression():
            h = x[0]
            q = rmsnorm(F.linear(h, wq, bq).view(S, Hkv, G, D), gq).permute(1, 0, 3, 2)        # [Hkv, S, D, G] float32
            k = rmsnorm(F.linear(h, wk).view(S, Hkv, 1, D), gk).permute(1, 0, 2, 3)            # [Hkv, S, 1, D]
            logit = torch.matmul(k, q) / D ** 0.5 + b.float()[:, None, None, :]
            base = torch.matmul(kb[:, None], q) / D ** 0.5                                     # [Hkv, S, J, G]
            score = (1 / (1 + torch.exp(base - logit).sum(2))).mean(-1)[None]
            score[..., :n_sink] = 1.0
            score[..., S - tail:] = 1.0
            return score

        def vendor_gemm():
            return F.linear(x[0], w_all)

        flop = 2.0 * B * S * K * Hkv * (G + 1) * D
        got, ref = library(), torch_expression()
        diff = float((got - ref).abs().max())
        del got, ref
        mem_lib, mem_torch = peak_transient_bytes(library), peak_transient_bytes(torch_expression)
        r_lib, r_torch, r_gemm = timed([library, torch_expression, vendor_gemm], args.reps)
        r_lib.update(flop=flop, floor_ms=flop / BF16_MATRIX_PEAK * 1e3, achieved_tflops=flop / (r_lib["median_ms"] * 1e-3) / 1e12,
                     peak_transient_bytes=mem_lib)
        r_lib["fraction_of_bf16_matrix_peak"] = r_lib["floor_ms"] / r_lib["median_ms"]   # from the CALL time
        r_torch.update(peak_transient_bytes=mem_torch)
        r_gemm.update(achieved_tflops=flop / (r_gemm["median_ms"] * 1e-3) / 1e12)
        other = {}
        for name, env in (("rows512_ktile64_heads4", dict(KVP_FASTKVZIP_GEO="1")), ("rows640_ktile32_heads8", dict(KVP_FASTKVZIP_GEO="2")),
                          ("rows512_ktile64_heads2", dict(KVP_FASTKVZIP_GEO="1", KVP_FASTKVZIP_HEADS="2")),
                          ("rows512_ktile64_heads1", dict(KVP_FASTKVZIP_GEO="1", KVP_FASTKVZIP_HEADS="1"))):
            os.environ.update(env)
            _native.tuning_reload()
            other[name] = timed([library], args.reps)[0]["median_ms"]
            for k in env:
                del os.environ[k]
        _native.tuning_reload()
        results.append(dict(S=S, kernel=r_lib, torch_expression=r_torch, vendor_gemm=r_gemm, torch_over_kernel=r_torch["median_ms"] / r_lib["median_ms"],
                            kernel_over_vendor_gemm=r_lib["median_ms"] / r_gemm["median_ms"], median_ms_by_geometry=other,
                            max_abs_diff_to_bf16_baseline=diff))
        del x
    out = {"geometry": dict(B=B, K=K, Hkv=Hkv, G=G, D=D, J=J, dtype="bf16"), "device": torch.cuda.get_device_name(0),
           "results": results}
    line = json.dumps(out)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
