#!/usr/bin/env python3
"""ms per layer at 128k (Llama-3.1-8B attention geometry, bf16) of NonCausalAttnPress / LeverageScorePress / CompactorPress.score:
the model's projections (torch), the library's part (the rest of score()), and a plain-PyTorch restatement of the reference's
scorers on the same GPU (written here; its chunked attention materialises [B, Hq, S/chunk, chunk, chunk] like the reference's).

    python tools/compactor_bench.py [--seq 131072] [--iters 5] [--torch-seq 32768]
Per-kernel times: run it under `rocprofv3 --kernel-trace --stats -- python tools/compactor_bench.py`.
"""
import argparse
import json
import math
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def timed(fn, iters):
    import torch

    fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    ts = []
    for _ in range(iters):
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1))
    return sorted(ts)[len(ts) // 2]


def torch_ncattn(q, k, v, cos, sin, chunk):
    import torch
    import torch.nn.functional as F

    h = q.shape[-1] // 2
    q = q * cos[:, None] + torch.cat((-q[..., h:], q[..., :h]), -1) * sin[:, None]
    B, Hq, S, D = q.shape
    G = Hq // k.shape[1]
    k = k.repeat_interleave(G, 1)
    S_pad = math.ceil(S / chunk) * chunk
    if S_pad != S:
        q = F.pad(q, (0, 0, 0, S_pad - S))
        k = F.pad(k, (0, 0, 0, S_pad - S))
    n = S_pad // chunk
    a = torch.softmax((q.view(B, Hq, n, chunk, D) @ k.view(B, Hq, n, chunk, D).transpose(-1, -2)).float(), -1).sum(-2)
    a = a.view(B, -1, G, S_pad)[..., :S].mean(2) * v.norm(dim=-1)
    s = F.avg_pool1d(a, 3, 1, 1)
    return (s - s.mean()) / s.std().clamp_min(1e-6)


def torch_leverage(kpre, phi):
    import torch

    X = ((kpre - kpre.mean(-2, keepdim=True)) @ phi).float()
    G = X.transpose(-1, -2) @ X
    L = torch.linalg.cholesky(0.5 * (G + G.transpose(-1, -2)) + 1e-2 * torch.eye(G.shape[-1], device=G.device))
    s = (X * torch.cholesky_solve(X.transpose(-1, -2), L).transpose(-1, -2)).sum(-1).clamp_min(0)
    return (s - s.mean()) / s.std().clamp_min(1e-6)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seq", type=int, default=131072)
    ap.add_argument("--torch-seq", type=int, default=32768)
    ap.add_argument("--iters", type=int, default=5)
    a = ap.parse_args()
    import torch
    from transformers import LlamaConfig
    from transformers.models.llama.modeling_llama import LlamaAttention, LlamaRotaryEmbedding

    import kvpress_amd as P
    from kvpress_amd import _native
    from kvpress_amd.utils import get_prerope_key_states, get_prerope_query_states

    dev, dt = "cuda:0", torch.bfloat16
    res = {"seq": a.seq, "geometry": "Hq 32, Hkv 8, D 128, hidden 4096, bf16", "ms_per_layer": {}}
    for S, full in ((a.seq, True), (a.torch_seq, False)):
        cfg = LlamaConfig(hidden_size=4096, num_attention_heads=32, num_key_value_heads=8, head_dim=128, num_hidden_layers=1,
                          intermediate_size=32, vocab_size=32, max_position_embeddings=S)
        torch.manual_seed(0)
        att = LlamaAttention(cfg, layer_idx=0).to(dev, dt)
        rot = LlamaRotaryEmbedding(cfg).to(dev)
        hidden = torch.randn(1, S, 4096, device=dev, dtype=dt)
        cos, sin = rot(hidden, torch.arange(S, device=dev)[None])
        keys = torch.randn(1, 8, S, 128, device=dev, dtype=dt)
        values = torch.randn(1, 8, S, 128, device=dev, dtype=dt)
        kw = {"position_embeddings": (cos, sin)}
        r = {}
        with torch.no_grad():
            q = get_prerope_query_states(att, hidden)
            kp = get_prerope_key_states(att, hidden)
            phi = torch.randn(1, 8, 128, 48, device=dev, dtype=dt) / math.sqrt(48)
            r["q_proj"] = timed(lambda: get_prerope_query_states(att, hidden), a.iters)
            r["k_proj"] = timed(lambda: get_prerope_key_states(att, hidden), a.iters)
            r["lib_noncausal"] = timed(lambda: _native.ncattn_score(q, cos, sin, keys, values, 256), a.iters)
            r["lib_leverage"] = timed(lambda: _native.leverage_score(kp, phi), a.iters)
            if full:
                r["press_noncausal"] = timed(lambda: P.NonCausalAttnPress(0.5).score(att, hidden, keys, values, None, kw), a.iters)
                r["press_leverage"] = timed(lambda: P.LeverageScorePress(0.5).score(att, hidden, keys, values, None, kw), a.iters)
                r["press_compactor"] = timed(lambda: P.CompactorPress(0.5).score(att, hidden, keys, values, None, kw), a.iters)
                r["compress_compactor"] = timed(lambda: P.CompactorPress(0.5).compress(att, hidden, keys, values, None, kw), a.iters)
            else:
                r["torch_noncausal"] = timed(lambda: torch_ncattn(q, keys, values, cos, sin, 256), a.iters)
                r["torch_leverage"] = timed(lambda: torch_leverage(kp, phi), a.iters)
        res["ms_per_layer"][str(S)] = {k: round(v, 4) for k, v in r.items()}
        del q, kp, hidden, keys, values, att
        torch.cuda.empty_cache()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
