#!/usr/bin/env python3
"""MergingPress timings on one GPU (Llama-3.1-8B layer geometry: H_kv 8, Hq 32, D 128, bf16, ratio 0.5), one JSON line:

    python tools/merging_bench.py [--seqs 32768,131072] [--iters 5] [--out profiles/merging_bench.json]

Per sequence length: ms per layer of MergingPress(SnapKVPress(.5)).compress next to SnapKVPress(.5).compress, the merge alone
(kvp_merge_values after the select and the gather), its kernels (hipEvent timing through the library's per-kernel profiler), the
argmax kernel's share of the 2.5 PFLOP/s dense bf16 MFMA rate (2 * n_evict * n_kept * D * H FLOPs), and at 32k a plain-PyTorch
restatement of the reference's merge() on the same GPU.
"""
import argparse
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))

import torch  # noqa: E402

PEAK_BF16 = 2.5e15


def torch_merge(keys, values, indices):
    """merging_press.py:99-177 in eager PyTorch (threshold 0, fraction 1)"""
    bsz, num_heads, seq_len, head_dim = keys.shape
    n_kept = indices.shape[2]
    n_evict = seq_len - n_kept
    evict_mask = torch.ones(bsz, num_heads, seq_len, device=keys.device, dtype=torch.bool)
    evict_mask.scatter_(2, indices, False)
    evict_idx = evict_mask.nonzero(as_tuple=False)[:, 2].reshape(bsz, num_heads, n_evict)
    keep_idx = indices.unsqueeze(-1).expand(-1, -1, -1, head_dim)
    evict_idx = evict_idx.unsqueeze(-1).expand(-1, -1, -1, head_dim)
    kept_keys = keys.gather(2, keep_idx).float()
    evict_keys = keys.gather(2, evict_idx).float()
    kept_values = values.gather(2, keep_idx)
    evict_values = values.gather(2, evict_idx)
    kept_keys = kept_keys / kept_keys.norm(dim=-1, keepdim=True).clamp(min=1e-6)
    evict_keys = evict_keys / evict_keys.norm(dim=-1, keepdim=True).clamp(min=1e-6)
    max_sim, target = (evict_keys @ kept_keys.transpose(-2, -1)).max(dim=-1)
    merge_ok = max_sim >= 0.0
    weights = max_sim.clamp(min=0) * merge_ok.float()
    target_norm = kept_values.float().norm(dim=-1).gather(2, target)
    evict_norm = evict_values.float().norm(dim=-1)
    weights = weights * evict_norm / (evict_norm + target_norm + 1e-6)
    target = target.unsqueeze(-1).expand(-1, -1, -1, head_dim)
    weights = weights.unsqueeze(-1)
    value_accum = torch.zeros(bsz, num_heads, n_kept, head_dim, device=keys.device, dtype=torch.float32)
    value_accum.scatter_add_(2, target, weights * evict_values.float())
    weight_accum = torch.zeros(bsz, num_heads, n_kept, device=keys.device, dtype=torch.float32)
    weight_accum.scatter_add_(2, target[..., 0], weights[..., 0])
    kept_values = torch.where((weight_accum > 0).unsqueeze(-1),
                              ((kept_values.float() + value_accum) / (1.0 + weight_accum).unsqueeze(-1)).to(values.dtype), kept_values)
    result_values = values.clone()
    result_values.scatter_(2, keep_idx, kept_values)
    return keys, result_values


def timed(fn, iters):
    fn()
    torch.cuda.synchronize()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(iters)]
    for a, b in ev:
        a.record()
        fn()
        b.record()
    torch.cuda.synchronize()
    t = sorted(a.elapsed_time(b) for a, b in ev)
    return t[len(t) // 2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seqs", default="32768,131072")
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    import _inputs
    from kvpress_amd import MergingPress, SnapKVPress, _native

    H, G, D, ratio, hsz = 8, 4, 128, 0.5, 4096
    res = {"metric": "merging_press_ms_per_layer", "geometry": dict(H_kv=H, Hq=H * G, D=D, hidden=hsz, dtype="bf16", ratio=ratio), "seqs": {}}
    for S in [int(x) for x in a.seqs.split(",")]:
        gen = torch.Generator().manual_seed(7)
        s = dict(B=1, H=H, G=G, Hq=H * G, S=S, D=D, hsz=hsz, dtype="bf16", seed=7,
                 wq=(torch.randn((H * G * D, hsz), generator=gen) / 64).numpy(), hidden=torch.randn((1, S, hsz), generator=gen).numpy())
        att, rot, hidden, pe = _inputs.build_llama_attention(s, torch.bfloat16, "cuda")
        keys = torch.randn((1, H, S, D), device="cuda", dtype=torch.bfloat16)
        values = torch.randn((1, H, S, D), device="cuda", dtype=torch.bfloat16)
        kw = {"position_embeddings": pe}
        inner = SnapKVPress(ratio)
        merging = MergingPress(SnapKVPress(ratio))
        with torch.no_grad():
            t_inner = timed(lambda: inner.compress(att, hidden, keys, values, None, kw), a.iters)
            t_press = timed(lambda: merging.compress(att, hidden, keys, values, None, kw), a.iters)
            scores = inner.score(att, hidden, keys, values, None, kw)
            n = int(S * (1 - ratio))
            idx = _native.topk_select(scores, n)
            k_out, v_out = _native.gather_kv(keys, values, idx)
            v_keep = v_out.clone()
            t_both = timed(lambda: (v_out.copy_(v_keep), _native.merge_values_(keys, values, idx, k_out, v_out, 0.0, 1.0)), a.iters)
            t_copy = timed(lambda: v_out.copy_(v_keep), a.iters)
            _native.prof_enable(True)
            _native.merge_values_(keys, values, idx, k_out, v_out, 0.0, 1.0)
            torch.cuda.synchronize()
            kern = {}
            for name, ms in _native.prof_records():
                kern[name] = kern.get(name, 0.0) + ms
            _native.prof_enable(False)
        t_argmax = sum(v for k_, v in kern.items() if k_.startswith("merge_argmax"))
        flops = 2.0 * (S - n) * n * D * H
        row = dict(snapkv_compress_ms=round(t_inner, 3), merging_snapkv_compress_ms=round(t_press, 3), merge_only_ms=round(t_both - t_copy, 3),
                   kernels_ms={k_: round(v, 3) for k_, v in kern.items()}, argmax_ms=round(t_argmax, 3), argmax_tflop=round(flops / 1e12, 2),
                   argmax_frac_of_peak=round(flops / (t_argmax * 1e-3) / PEAK_BF16, 3) if t_argmax else None)
        if S <= 32768:
            with torch.no_grad():
                row["torch_merge_ms"] = round(timed(lambda: torch_merge(keys, values, idx.long()), a.iters), 3)
        res["seqs"][str(S)] = row
        del att, hidden, keys, values, scores, k_out, v_out, v_keep
        torch.cuda.empty_cache()
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
