"""Float64 numpy restatement of the three CAMPress kernels (include/kvpress_hip.h: kvp_cam_attn_accumulate, kvp_cam_merge_plan,
kvp_cam_merge_prune; kvpress/presses/cam_press.py:124-361) and of the press's ranking.  Test infrastructure only."""
from __future__ import annotations

import numpy as np

import _inputs


def rope_last_query(q_pre, cos, sin, dtype: str) -> np.ndarray:
    """q * cos + rotate_half(q) * sin of the newest token's query [B,Hq,1,D] with torch's own ops in the model dtype (every product and
    the sum rounded to it, cam_press.py:341-344), as float64."""
    import torch

    dt = _inputs.torch_dtype(dtype)
    q = torch.from_numpy(np.asarray(q_pre, np.float32)).to(dt)
    c = torch.from_numpy(np.asarray(cos, np.float32)).to(dt)[:, None]
    s = torch.from_numpy(np.asarray(sin, np.float32)).to(dt)[:, None]
    half = q.shape[-1] // 2
    rot = torch.cat((-q[..., half:], q[..., :half]), dim=-1)
    return ((q * c) + (rot * s)).double().numpy()


def attention_row(q_rot, keys, n_kv_heads: int) -> np.ndarray:
    """mean over the query heads of a kv head of softmax_s(q . k_s / sqrt(D)) over ALL keys: [B,Hkv,S] (cam_press.py:346-361)."""
    q = np.asarray(q_rot, np.float64)[:, :, 0]                     # [B,Hq,D]
    k = np.asarray(keys, np.float64)                               # [B,Hkv,S,D]
    B, Hq, D = q.shape
    G = Hq // n_kv_heads
    logits = np.einsum("bhgd,bhsd->bhgs", q.reshape(B, n_kv_heads, G, D), k) / np.sqrt(D)
    logits -= logits.max(-1, keepdims=True)
    p = np.exp(logits)
    p /= p.sum(-1, keepdims=True)
    return p.mean(2)


def group_mean(attn_row, n_kv_heads: int) -> np.ndarray:
    a = np.asarray(attn_row, np.float64)                           # [B,Hq,S]
    B, Hq, S = a.shape
    return a.reshape(B, n_kv_heads, Hq // n_kv_heads, S).mean(2)


def accumulate(running, s_prev: int, a) -> np.ndarray:
    """running[s] = (s < s_prev ? running[s] : 0) + a[s] for s < S; whatever lies beyond s_prev in ``running`` is ignored"""
    S = a.shape[-1]
    out = np.zeros(a.shape, np.float64)
    out[..., :s_prev] = np.asarray(running)[..., :s_prev]
    return out + a


def rank(mean_scores, T: int, M: int):
    """kept = ranks [0, T), candidates = ranks [T, T + M) of the total order (score descending, position ascending); both returned in
    ascending position, int32 [B,T] / [B,M]"""
    order = np.argsort(-np.asarray(mean_scores, np.float64), axis=-1, kind="stable")
    return np.sort(order[:, :T], axis=-1).astype(np.int32), np.sort(order[:, T:T + M], axis=-1).astype(np.int32)


def plan(kept, cand, A, merge_budget: int):
    """start, budget int64 [B,M]; prob float64 [B,H,M] (cam_press.py:159-183)"""
    kept, cand, A = np.asarray(kept, np.int64), np.asarray(cand, np.int64), np.asarray(A, np.float64)
    B, T = kept.shape
    M = cand.shape[1]
    H = A.shape[1]
    start = np.stack([np.searchsorted(kept[b], cand[b], side="right") for b in range(B)]) if M else np.zeros((B, 0), np.int64)
    budget = np.minimum(merge_budget, T - start)
    prob = np.zeros((B, H, M))
    with np.errstate(divide="ignore", invalid="ignore"):
        for b in range(B):
            for i in range(M):
                w = kept[b, start[b, i]:start[b, i] + budget[b, i]]
                mean = A[b][:, w].sum(-1) / max(int(budget[b, i]), 1)
                prob[b, :, i] = A[b, :, cand[b, i]] / mean
    prob = np.where(np.isnan(prob), 0.0, prob)
    prob = np.where(np.isinf(prob), 1.0, prob)
    return start, budget, np.clip(prob, 0.0, 1.0)


def merge_prune(keys, values, A, kept, cand, mask, merge_budget: int, dtype: str):
    """dict: k [B,H,T,D], v (float64 sums rounded once to ``dtype``), v64 (unrounded), a [B,H,T], merged bool [B,H,T] (rows with at least
    one contributor whose mask is not zero) -- cam_press.py:188-213"""
    keys, values, A = np.asarray(keys), np.asarray(values, np.float64), np.asarray(A)
    kept64, cand64 = np.asarray(kept, np.int64), np.asarray(cand, np.int64)
    B, H, S, D = keys.shape
    T, M = kept64.shape[1], cand64.shape[1]
    start, budget, _ = plan(kept64, cand64, np.zeros((B, H, S)), merge_budget)
    ix = kept64[:, None, :, None].repeat(H, 1).repeat(D, 3)
    k_out = np.take_along_axis(keys, ix, 2)
    v64 = np.take_along_axis(values, ix, 2).copy()
    a_out = np.take_along_axis(A, kept64[:, None, :].repeat(H, 1), 2)
    merged = np.zeros((B, H, T), bool)
    mask = np.asarray(mask, np.float64)
    for b in range(B):
        for i in range(M):
            s0, n = int(start[b, i]), int(budget[b, i])
            if n < 1:
                continue
            for h in range(H):
                if mask[b, h, i] != 0:
                    v64[b, h, s0:s0 + n] += (mask[b, h, i] / n) * values[b, h, cand64[b, i]]
                    merged[b, h, s0:s0 + n] = True
    return dict(k=k_out, v=_inputs.round_to(v64.astype(np.float32), dtype) if dtype != "f32" else v64.astype(np.float32), v64=v64, a=a_out,
                merged=merged, start=start, budget=budget)
