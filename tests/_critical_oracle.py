"""float64 numpy restatement of CriticalKVPress / CriticalAdaKVPress (kvpress/presses/criticalkv_press.py:57-194): the projected L1 norm,
the rescale with float32's behaviour at the top of the range, both two-stage selections and this package's per-element batch rule.
Test infrastructure only.

Ties.  torch.topk leaves the choice among near-equal scores open and the reference computes in float32, so every selection here also
reports its BAND: the positions within ``rel`` (1e-3) of that selection's threshold.  Kept sets, masks and filled entries are compared
outside the union of the bands (sets_equal_outside); oracle/gen_golden_critical.py asserts that the bands of the fixtures are small."""
from __future__ import annotations

import numpy as np

FMAX = float(np.finfo(np.float32).max)
REL = 1e-3


def vwl1norm(values: np.ndarray, wo: np.ndarray, num_heads: int) -> np.ndarray:
    """norm[b,k,s] = (1/G) sum_g sum_c |sum_d v[b,k,s,d] wo[c, (k G + g) D + d]|  (:57-76), float64"""
    v = np.asarray(values, np.float64)
    B, H, S, D = v.shape
    G = num_heads // H
    w = np.asarray(wo, np.float64).reshape(wo.shape[0], num_heads, D)
    out = np.zeros((B, H, S))
    for h in range(H):
        for g in range(G):
            out[:, h] += np.abs(v[:, h] @ w[:, h * G + g].T).sum(-1)
    return out / G


def rescale(scores: np.ndarray, norm: np.ndarray, eps: float) -> np.ndarray:
    """(scores + eps) * norm as float32 evaluates it where that matters (:87): fmax + eps == fmax, and a product beyond fmax is +inf"""
    s = np.asarray(scores, np.float64)
    with np.errstate(over="ignore", invalid="ignore"):
        x = np.where(s >= FMAX, FMAX, s + eps) * np.asarray(norm, np.float64)
    return np.where(x > FMAX, np.inf, x)


def _topk(row: np.ndarray, k: int) -> np.ndarray:
    """positions of the k largest entries, ties to the lowest position (the library's rule)"""
    return np.argsort(-row, kind="stable")[:k]


def _band(row: np.ndarray, k: int, rel: float = REL) -> np.ndarray:
    """positions within rel of the threshold of the top-k selection of row (none if the selection takes nothing or everything)"""
    if k <= 0 or k >= row.size:
        return np.zeros(row.size, bool)
    t = np.sort(row)[::-1][k - 1]
    if not np.isfinite(t) or t >= FMAX:   # (a threshold among the protected entries: filling one of them again changes nothing)
        return np.zeros(row.size, bool)
    with np.errstate(invalid="ignore"):
        return np.abs(row - t) <= rel * abs(t)


def critical_scores(inner: np.ndarray, norm: np.ndarray, ratio: float, fsr: float, eps: float):
    """CriticalKVPress.score (:78-92): (final scores float64 [B,H,S], band bool [B,H,S] of the stage-1 selection)"""
    inner = np.asarray(inner, np.float64)
    B, H, S = inner.shape
    k1 = int((1 - ratio) * S * fsr)
    final = rescale(inner, norm, eps)
    band = np.zeros(inner.shape, bool)
    for b in range(B):
        for h in range(H):
            final[b, h, _topk(inner[b, h], k1)] = FMAX
            band[b, h] = _band(inner[b, h], k1)
    return final, band


def kept_positions(final: np.ndarray, n_kept: int):
    """ScorerPress.compress on the final scores: (sorted kept positions int32 [B,H,n], band bool [B,H,S])"""
    B, H, S = final.shape
    pos = np.zeros((B, H, n_kept), np.int32)
    band = np.zeros(final.shape, bool)
    for b in range(B):
        for h in range(H):
            pos[b, h] = np.sort(_topk(final[b, h], n_kept))
            band[b, h] = _band(final[b, h], n_kept)
    return pos, band


def stage1_budgets(budgets: np.ndarray, fsr: float) -> np.ndarray:
    """(head_budgets * first_stage_ratio).to(int64) in torch's float32 arithmetic (:167): 90 * 0.7 is 63 there, 62 in float64"""
    return (np.asarray(budgets).astype(np.float32) * np.float32(fsr)).astype(np.int64)


def critical_ada(inner: np.ndarray, norm: np.ndarray, ratio: float, alpha: float, fsr: float, eps: float) -> dict:
    """CriticalAdaKVPress.compress (:137-194), every batch element on its own (this package's rule; the reference's for B = 1).
    Returns budgets int64 [B,H], masked: sorted flat indices head * S + position int64 [B, n_pruned], final float64 [B,H,S], band bool
    [B,H,S] (the union over all selections), band_max (the largest band of a single per-head selection), budget_band (positions within
    rel of the threshold of the flattened budget selection, the threshold itself included) and budget_gap [B]: the relative gap there."""
    s_all = np.asarray(inner, np.float64).copy()
    B, H, S = s_all.shape
    n_kept = int(S * (1 - ratio))
    n_safe = int(n_kept * alpha)
    n_pruned = H * (S - n_kept)
    out = dict(budgets=np.zeros((B, H), np.int64), masked=np.zeros((B, n_pruned), np.int64), final=np.zeros((B, H, S)),
               band=np.zeros((B, H, S), bool), band_max=0, budget_band=0, budget_gap=np.full(B, np.inf))

    def mark(band_row, sel):
        band_row |= sel
        out["band_max"] = max(out["band_max"], int(sel.sum()))

    for b in range(B):
        s, band = s_all[b], out["band"][b]
        for h in range(H):
            mark(band[h], _band(s[h], n_safe))
            s[h, _topk(s[h], n_safe)] = FMAX
        flat = s.reshape(-1)
        k = n_kept * H
        budgets = np.bincount(_topk(flat, k) // S, minlength=H).astype(np.int64)
        if 0 < k < flat.size:
            srt = np.sort(flat)[::-1]
            out["budget_gap"][b] = abs(srt[k - 1] - srt[k]) / max(abs(srt[k - 1]), 1e-300)
            out["budget_band"] = max(out["budget_band"], int(_band(flat, k).sum()))
        b1 = stage1_budgets(budgets, fsr)
        for h in range(H):
            mark(band[h], _band(s[h], int(b1[h])))
            s[h, _topk(s[h], int(b1[h]))] = FMAX
        s = rescale(s, norm[b], eps)
        for h in range(H):
            mark(band[h], _band(s[h], int(budgets[h])))
            s[h, _topk(s[h], int(budgets[h]))] = FMAX
        flat = s.reshape(-1)
        band |= _band(-flat, n_pruned).reshape(H, S)
        out["masked"][b] = np.sort(_topk(-flat, n_pruned))
        out["budgets"][b], out["final"][b] = budgets, s
    return out


def sets_equal_outside(a, b, band_flat) -> bool:
    """two index sets of one row are the same size and agree on every position outside the band"""
    a, b = np.asarray(a).ravel(), np.asarray(b).ravel()
    free = ~np.asarray(band_flat).ravel()
    return a.size == b.size and set(a[free[a]].tolist()) == set(b[free[b]].tolist())
