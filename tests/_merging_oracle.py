"""float64 numpy restatement of MergingPress.merge (kvpress/presses/merging_press.py:99-177) over kept indices in any order.

``merge`` returns the evicted positions, the nearest survivor (index into the kept list, ties to the lowest index) and its cosine, the
gates and the merged V' (the kept rows of ``values`` in kept-list order; merged rows rounded to the dtype).  ``target`` / ``max_sim`` can
be supplied (a kernel's own argmax): the gates are then evaluated on those float32 numbers with float32 quantile arithmetic, as the
kernel does, and only the weights and sums run in float64."""
from __future__ import annotations

import numpy as np

import _inputs

EPS = 1e-6


def evicted_positions(kept: np.ndarray, S: int) -> np.ndarray:
    """[B, H, S - n_kept] ascending complement of the kept set (evict_mask.nonzero(), :124-127)."""
    B, H, nk = kept.shape
    mask = np.ones((B, H, S), dtype=bool)
    np.put_along_axis(mask, kept.astype(np.int64), False, axis=2)
    return np.nonzero(mask)[2].reshape(B, H, S - nk)


def similarities(keys: np.ndarray, kept: np.ndarray, ev: np.ndarray, b: int, h: int) -> np.ndarray:
    """float64 cosine similarities [n_evict, n_kept] of one head (the reference's normalise-then-matmul, :131-139)."""
    k = keys[b, h].astype(np.float64)
    kk, ke = k[kept[b, h]], k[ev[b, h]]
    kk = kk / np.maximum(np.linalg.norm(kk, axis=-1, keepdims=True), EPS)
    ke = ke / np.maximum(np.linalg.norm(ke, axis=-1, keepdims=True), EPS)
    return ke @ kk.T


def aten_quantile(x: np.ndarray, q: float) -> np.ndarray:
    """torch.quantile(x, q, dim=-1) with ATen's arithmetic: float32 rank q * (n - 1), floor / ceil order statistics, lerp with the
    weight < 0.5 branch split (a -inf lower statistic gives NaN for weights < 0.5 and -inf above: the reference's behaviour)."""
    n = x.shape[-1]
    qf = np.float32(q)
    rank = np.float32(qf * np.float32(n - 1))
    lo, hi = int(np.floor(rank)), int(np.ceil(rank))
    w = x.dtype.type(np.float32(rank - np.float32(lo)))
    s = np.sort(x, axis=-1)
    a, c = s[..., lo], s[..., hi]
    with np.errstate(invalid="ignore", over="ignore"):
        d = c - a
        return np.where(abs(w) < 0.5, a + w * d, c - d * (x.dtype.type(1) - w))


def merge(keys, values, kept, threshold: float, fraction: float, dtype: str, target=None, max_sim=None) -> dict:
    keys = np.asarray(keys, dtype=np.float32)
    values = np.asarray(values, dtype=np.float32)
    kept = np.asarray(kept).astype(np.int64)
    B, H, S, D = keys.shape
    nk = kept.shape[-1]
    ne = S - nk
    v_kept = np.take_along_axis(values, kept[..., None].repeat(D, -1), axis=2)
    out = dict(evicted=np.zeros((B, H, ne), np.int64), target=np.zeros((B, H, ne), np.int64), max_sim=np.zeros((B, H, ne)),
               ok=np.zeros((B, H, ne), bool), weights=np.zeros((B, H, ne)), v=v_kept.copy(), merged=np.zeros((B, H, nk), bool))
    if ne == 0 or nk == 0:
        return out
    ev = evicted_positions(kept, S)
    out["evicted"] = ev
    if target is None:
        ms = np.zeros((B, H, ne))
        tg = np.zeros((B, H, ne), np.int64)
        for b in range(B):
            for h in range(H):
                sim = similarities(keys, kept, ev, b, h)
                tg[b, h] = sim.argmax(-1)          # first occurrence of the maximum
                ms[b, h] = sim[np.arange(ne), tg[b, h]]
        gdt = np.float64
    else:
        tg = np.asarray(target).astype(np.int64)
        ms = np.asarray(max_sim, dtype=np.float32)
        gdt = np.float32
    ok = ms >= np.float32(threshold)
    if fraction < 1.0 and ok.any():
        masked = np.where(ok, ms, -np.inf).astype(gdt)
        thr = aten_quantile(masked, 1.0 - fraction)[..., None]
        with np.errstate(invalid="ignore"):
            ok = ok & (ms >= thr)
    v64 = values.astype(np.float64)
    en = np.linalg.norm(np.take_along_axis(v64, ev[..., None].repeat(D, -1), axis=2), axis=-1)
    tn = np.take_along_axis(np.linalg.norm(v_kept.astype(np.float64), axis=-1), tg, axis=2)
    w = np.maximum(ms.astype(np.float64), 0.0) * ok * en / (en + tn + EPS)
    acc = np.zeros((B, H, nk, D))
    wsum = np.zeros((B, H, nk))
    for b in range(B):
        for h in range(H):
            ve = v64[b, h, ev[b, h]]
            np.add.at(acc[b, h], tg[b, h], w[b, h][:, None] * ve)     # ascending evicted position, as scatter_add_
            np.add.at(wsum[b, h], tg[b, h], w[b, h])
    merged = wsum > 0
    new = _inputs.round_to(((v_kept + acc) / (1.0 + wsum)[..., None]).astype(np.float32), dtype)
    out.update(target=tg, max_sim=ms, ok=ok, weights=w, merged=merged, v=np.where(merged[..., None], new, v_kept))
    return out
