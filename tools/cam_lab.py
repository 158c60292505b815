#!/usr/bin/env python3
"""CAMPress timings on the GPU (hipEvent medians over warmed-up repeats of batches of calls), Llama-3.1-8B geometry (H_kv 8, G 4, D 128, bf16, B 1):

  * the per-step attention accumulate (kvp_cam_attn_accumulate) at S = 2560 and S = 131072;
  * one compression 2560 -> 2048 with 512 merge candidates and merge_budget 32 (CAMPress(KnormPress).compress), against
    DecodingPress(KnormPress).compress -- plain eviction -- at the same shape;

each next to its modelled byte floor (bytes the algorithm must move / 6.29 TB/s, the copy ceiling DESIGN.md section 5 uses).

    python tools/cam_lab.py [--reps 30] [--out profiles/cam_lab.json]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
COPY_CEILING = 6.29e12   # bytes / s


def timed(fns, reps, inner=20, warmup=3):
    """median / min microseconds per call of each function of ``fns``: ``inner`` back-to-back calls between a pair of events (so the
    events see the device's time per call, not one launch's host path), the functions taking turns from repeat to repeat"""
    import torch

    def batch(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(inner):
            fn()
        b.record()
        b.synchronize()
        return a.elapsed_time(b) * 1e3 / inner

    for _ in range(warmup):
        for fn in fns:
            batch(fn)
    times = [[] for _ in fns]
    for _ in range(reps):
        for i, fn in enumerate(fns):
            times[i].append(batch(fn))
    return [dict(median_us=statistics.median(x), min_us=min(x), reps=reps, calls_per_rep=inner) for x in times]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch

    import kvpress_amd as P
    from kvpress_amd import _native

    assert torch.cuda.is_available(), "cam_lab needs a GPU"
    dev, dt = "cuda", torch.bfloat16
    B, H, G, D = 1, 8, 4, 128
    gen = torch.Generator(device=dev).manual_seed(0)
    out = {"geometry": dict(B=B, Hkv=H, G=G, D=D, dtype="bf16"), "device": torch.cuda.get_device_name(0)}

    for S in (2560, 131072):
        keys = torch.randn((B, H, S, D), device=dev, generator=gen).to(dt)
        q = torch.randn((B, H * G, 1, D), device=dev, generator=gen).to(dt)
        cos = torch.rand((1, 1, D), device=dev, generator=gen).to(dt)
        sin = torch.rand((1, 1, D), device=dev, generator=gen).to(dt)
        running = torch.zeros((B, H, S + 512), device=dev)
        r, = timed([lambda: _native.cam_attn_accumulate_(q, cos, sin, keys, running, S - 1)], args.reps, inner=20 if S < 10000 else 5)
        # K once, the logits written and read once, the running sum read and written
        nbytes = B * H * S * D * 2 + 2 * B * H * G * S * 4 + 2 * B * H * S * 4
        r.update(bytes=nbytes, floor_us=nbytes / COPY_CEILING * 1e6)
        r["floor_over_median"] = r["floor_us"] / r["median_us"]
        out[f"accumulate_S{S}"] = r
        del keys, running

    S, T, M, m = 2560, 2048, 512, 32
    keys = torch.randn((B, H, S, D), device=dev, generator=gen).to(dt)
    values = torch.randn((B, H, S, D), device=dev, generator=gen).to(dt)
    running = torch.rand((B, H, S), device=dev, generator=gen)

    class _M(torch.nn.Module):
        layer_idx, head_dim = 0, D

    module = _M()
    cam = P.CAMPress(base_press=P.KnormPress(), compression_interval=M, target_size=T, merge_budget=m)

    def cam_compress():
        cam.layer_step_counts[0] = M
        return cam.compress(module, None, keys, values, running, {})

    dec = P.DecodingPress(base_press=P.KnormPress(), compression_interval=M, target_size=T)
    r_cam, r_dec = timed([cam_compress, lambda: dec.compress(module, None, keys, values, None, {})], args.reps)   # taking turns
    # K for the norms, T rows of K and V read and written, A' and the candidates' values (each read by up to m rows, from cache: once)
    nbytes = B * H * (S * D * 2 + 4 * T * D * 2 + M * D * 2 + 2 * T * 4)
    r_cam.update(bytes=nbytes, floor_us=nbytes / COPY_CEILING * 1e6)
    r_cam["floor_over_median"] = r_cam["floor_us"] / r_cam["median_us"]
    out["compress_cam_2560_2048"] = r_cam
    out["compress_decoding_knorm_2560_2048"] = r_dec
    out["cam_over_plain_eviction"] = r_cam["median_us"] / r_dec["median_us"]
    # the plan and the merge-prune on their own
    kept = _native.topk_select(running[:, :1], T)[:, 0]
    sel = _native.topk_select(running[:, :1], T + M)[:, 0]
    out["merge_plan"], = timed([lambda: _native.cam_merge_plan(kept, sel, running, S, m, n_cand=M)], args.reps)
    cand, start, prob = _native.cam_merge_plan(kept, sel, running, S, m, n_cand=M)
    mask = torch.bernoulli(prob)
    out["merge_prune"], = timed([lambda: _native.cam_merge_prune(keys, values, running, kept, cand, start, mask, m)], args.reps)
    line = json.dumps(out)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
