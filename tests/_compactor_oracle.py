"""Float64 numpy restatement of the Compactor family's scorers (reference non_causal_attention_press.py:47-122,
leverage_press.py:47-110, compactor_press.py:87-122), with the model dtype's roundings where the reference's torch ops round
(RoPE per op, the matmul outputs, the key mean, ||v||).  The sketch Phi is an argument (the reference draws it with torch.randn)."""
from __future__ import annotations

import math

import numpy as np

from _inputs import round_to


def _r(x, dtype):
    return round_to(np.asarray(x, dtype=np.float32), dtype).astype(np.float64)


def rope(q, cos, sin, dtype):
    """q * cos + rotate_half(q) * sin with each op rounded to ``dtype``; q [B,H,S,D], cos/sin [Bc,S,D]."""
    q = np.asarray(q, np.float32)
    h = q.shape[-1] // 2
    rh = np.concatenate([-q[..., h:], q[..., :h]], axis=-1)
    c, s = np.asarray(cos, np.float32)[:, None], np.asarray(sin, np.float32)[:, None]
    return _r(_r(q * c, dtype) + _r(rh * s, dtype), dtype)


def zscore(x):
    x = np.asarray(x, np.float64)
    return (x - x.mean()) / max(x.std(ddof=1), 1e-6)


def ncattn_colsums(q_rot, k, chunk, dtype):
    """non_causal_chunked_attn (:47-93) on RoPE'd queries [B,Hq,S,D] and keys [B,Hkv,S,D]: [B,Hq,S]."""
    B, Hq, S, D = q_rot.shape
    G = Hq // k.shape[1]
    kk = np.repeat(np.asarray(k, np.float64), G, axis=1)
    S_pad = math.ceil(S / chunk) * chunk
    qp = np.zeros((B, Hq, S_pad, D)); qp[:, :, :S] = q_rot
    kp = np.zeros((B, Hq, S_pad, D)); kp[:, :, :S] = kk
    n = S_pad // chunk
    dots = np.einsum("bhcid,bhcjd->bhcij", qp.reshape(B, Hq, n, chunk, D), kp.reshape(B, Hq, n, chunk, D))
    dots = _r(dots, dtype)
    if S_pad != S:   # the last chunk's padded rows / columns (:70-88)
        inval = np.arange((S // chunk) * chunk, S_pad) >= S
        last = dots[:, :, -1]
        last[:, :, inval, :] = 0.0
        last[:, :, :, inval] = float(_r(np.array([-1e-9]), dtype)[0])
    dots = dots - dots.max(-1, keepdims=True)
    p = np.exp(dots)
    p /= p.sum(-1, keepdims=True)
    return p.sum(-2).reshape(B, Hq, S_pad)[..., :S]


def ncattn_raw(q_pre, cos, sin, k, v, chunk, dtype):
    """NonCausalAttnPress.score (:95-122) before the z-score: [B,Hkv,S]."""
    q_rot = rope(q_pre, cos, sin, dtype)
    A = ncattn_colsums(q_rot, k, chunk, dtype)
    B, Hq, S = A.shape
    Hkv = k.shape[1]
    A = A.reshape(B, Hkv, Hq // Hkv, S).mean(2)
    vn = _r(np.sqrt((np.asarray(v, np.float64) ** 2).sum(-1)), dtype)
    x = A * vn
    xp = np.pad(x, ((0, 0), (0, 0), (1, 1)))
    return (xp[..., :-2] + xp[..., 1:-1] + xp[..., 2:]) / 3.0


def chol_with_jitter(G, jitter=1e-2, max_tries=5):
    cur = float(jitter)
    for _ in range(max_tries):
        try:
            return np.linalg.cholesky(G + cur * np.eye(G.shape[-1]))
        except np.linalg.LinAlgError:
            cur = max(1e-8, (1e-2 if cur == 0.0 else 10.0 * cur))
    raise RuntimeError(f"Cholesky failed after {max_tries} tries.")


def leverage_raw(k_pre, phi, dtype):
    """compute_leverage_scores (:59-110) with the sketch phi [B,H,D,k]: [B,H,S]."""
    k_pre = np.asarray(k_pre, np.float32)
    B, H, S, D = k_pre.shape
    out = np.zeros((B, H, S))
    for b in range(B):
        for h in range(H):
            kk = k_pre[b, h].astype(np.float64)
            mu = _r(kk.mean(0), dtype)
            X = _r(kk - mu, dtype)
            X = _r(X @ np.asarray(phi[b, h], np.float64), dtype)
            G = X.T @ X
            L = chol_with_jitter(0.5 * (G + G.T))
            Y = np.linalg.solve(L, X.T)
            out[b, h] = np.maximum((Y * Y).sum(0), 0.0)
    return out


def compactor_combine(z_lev, z_attn, left, right, blending):
    s = blending * np.asarray(z_lev, np.float64) + np.asarray(z_attn, np.float64)
    return np.pad(s, ((0, 0), (0, 0), (left, right)), constant_values=s.max())


def n_kept(S, ratio):
    return int(S * (1 - ratio))


def kept_sets_equal_up_to_ties(got_scores, want_scores, n, tol):
    """Every row: the tokens whose reference score clears the n-th largest by more than tol are kept, those below it by more than
    tol are not (the band in between may go either way)."""
    g = np.argsort(-got_scores, axis=-1, kind="stable")[..., :n]
    for r in np.ndindex(*want_scores.shape[:-1]):
        w = want_scores[r]
        thr = np.sort(w)[::-1][n - 1]
        kept = np.zeros(w.shape[-1], bool); kept[g[r]] = True
        if not (kept[w > thr + tol].all() and not kept[w < thr - tol].any()):
            return False
    return True
