"""float64 restatement of FastKVzip's gate (kvpress/presses/fastkvzip_press.py:54-71), of the protected positions of :240-247 and of
the selection (compress_post, :251-287), with a first-order ERROR BOUND per score for an evaluation whose products accumulate in float32
and whose every later step is float32 (include/kvpress_hip.h: kvp_fastkvzip_score).  Test infrastructure only.

The bound (derivation: DESIGN.md section 2), u = 2^-24, c = K + 2 (0 for exact inputs, whose projections carry no error):
    projected entry p_i:       e_i  = c u (|W| |x| + |bias|)_i
    RMSNorm n = g p / r:       en_i = |g_i| (e_i / r + |p_i| sum_j |p_j| e_j / (D r^3)) + (D/2 + 5) u |n_i|        r = sqrt(mean p^2 + eps)
    logit l = <k,q>/sqrt D + b: el  = (sum_d ek_d |q_d| + |k_d| eq_d + (D + 2) u |k_d q_d|) / sqrt D + u |l|
    base_j = <kb_j,q>/sqrt D:  eb_j = (sum_d |kb_jd| eq_d + (D + 2) u |kb_jd q_d|) / sqrt D
    s = 1 / (1 + sum_j E_j), E_j = exp(base_j - l):
                               es   = s^2 sum_j E_j (eb_j + el + u |base_j - l| + (2 + J) u) + 2 u s
    score = mean_g s_g:        bound = mean_g es_g + G u score
The contract is |library - float64| <= 2 bound (the factor 2 is the project's margin, as in the KVzap contract)."""
import numpy as np

U = 2.0 ** -24


def _project(x, w, bias, c, perturb):
    """(p, e) [B, S, rows]: x w^T + bias and c u (|x| |w|^T + |bias|); perturb = (b, s, row, k, factor): the products w[row, k] * x[b, s, k]
    count `factor` times (0: dropped, 2: doubled); s and row are an index or a slice (slice(None): every token / every row)"""
    p = x @ w.T
    if perturb is not None:
        b, s, row, k, factor = perturb
        hit = np.zeros(p.shape[1:])
        hit[s, row] = 1.0
        p[b] += (factor - 1.0) * np.outer(x[b, :, k], w[:, k]) * hit
    e = c * U * (np.abs(x) @ np.abs(w).T)
    if bias is not None:
        p, e = p + bias, e + c * U * np.abs(bias)
    return p, e


def _rmsnorm(p, e, g, eps):
    D = p.shape[-1]
    r = np.sqrt((p * p).mean(-1, keepdims=True) + eps)
    n = g * p / r
    en = np.abs(g) * (e / r + np.abs(p) * (np.abs(p) * e).sum(-1, keepdims=True) / (D * r ** 3)) + (D / 2 + 5) * U * np.abs(n)
    return n, en


def fastkvzip_score(x, wq, bq, wk, b, gq, gk, kb, eps, k_term=True, perturb_q=None, perturb_k=None):
    """(score, bound), float64 [B, Hkv, S] each, from the hidden states x [B,S,K] and one layer's gate: wq [Hkv*G*D, K], bq, wk [Hkv*D, K],
    b [Hkv, G], gq, gk [D], kb [Hkv, J, D].  No protected positions (see `protect`).  k_term False: the projections are exact."""
    x, wq, bq, wk, b, gq, gk, kb = (np.asarray(a, np.float64) for a in (x, wq, bq, wk, b, gq, gk, kb))
    B, S, K = x.shape
    Hkv, G = b.shape
    D, J = gq.shape[0], kb.shape[1]
    c = (K + 2.0) if k_term else 0.0
    sd = np.sqrt(float(D))
    pq, eq = _project(x, wq, bq, c, perturb_q)
    pk, ek = _project(x, wk, None, c, perturb_k)
    q, eq = _rmsnorm(pq.reshape(B, S, Hkv, G, D), eq.reshape(B, S, Hkv, G, D), gq, eps)
    k, ek = _rmsnorm(pk.reshape(B, S, Hkv, D), ek.reshape(B, S, Hkv, D), gk, eps)
    aq, ak, akb = np.abs(q), np.abs(k), np.abs(kb)

    logit = np.einsum("bshd,bshgd->bshg", k, q) / sd + b
    el = (np.einsum("bshd,bshgd->bshg", ek, aq) + np.einsum("bshd,bshgd->bshg", ak, eq)
          + (D + 2) * U * np.einsum("bshd,bshgd->bshg", ak, aq)) / sd + U * np.abs(logit)
    base = np.einsum("hjd,bshgd->bshgj", kb, q) / sd
    eb = (np.einsum("hjd,bshgd->bshgj", akb, eq) + (D + 2) * U * np.einsum("hjd,bshgd->bshgj", akb, aq)) / sd
    z = base - logit[..., None]
    E = np.exp(z)
    s = 1.0 / (1.0 + E.sum(-1))
    es = s * s * (E * (eb + el[..., None] + U * np.abs(z) + (2 + J) * U)).sum(-1) + 2 * U * s
    score = s.mean(-1)
    bound = es.mean(-1) + G * U * score
    return score.transpose(0, 2, 1), bound.transpose(0, 2, 1)


def protect(score, head, tail):
    """a copy with the first `head` and the last `tail` positions set to 1 (either may exceed the length)"""
    out = np.array(score, copy=True)
    S = out.shape[-1]
    out[..., :min(head, S)] = 1.0
    out[..., S - min(tail, S):] = 1.0
    return out


def protected_counts(ctx_len, n_sink=4, window_size=4096, window_ratio=0.02):
    """(head, tail) of fastkvzip_press.py:240-247, the quirk included: a window of 0 tokens protects EVERY position"""
    window = int(ctx_len * window_ratio) if ctx_len < 32000 else window_size
    return n_sink, (ctx_len if window == 0 else window)


def worst_ratio(got, ref, bound):
    """max |got - ref| / (2 bound)"""
    return float((np.abs(np.asarray(got, np.float64) - ref) / (2.0 * bound)).max())


def compress_post(score_val, compression_ratio, layerwise):
    """per layer the SET of masked (batch, head, position) and n_pruned (:251-287); ties are broken arbitrarily, as torch.topk's are"""
    score_val = np.asarray(score_val)
    L, B, H, S = score_val.shape
    if layerwise:
        n_pruned = [int(B * H * S * compression_ratio)] * L
    else:
        order = np.argsort(score_val.reshape(-1), kind="stable")[:int(score_val.size * compression_ratio)]
        n_pruned = np.bincount(order // (B * H * S), minlength=L).tolist()
    sets = []
    for l in range(L):
        flat = score_val[l].reshape(B, H * S)
        idx = np.argsort(flat, axis=1, kind="stable")[:, :n_pruned[l]]
        sets.append({(bb, int(i) // S, int(i) % S) for bb in range(B) for i in idx[bb]})
    return sets, n_pruned


def boundary_gaps(score_val, compression_ratio, layerwise):
    """the gaps between the neighbouring sorted scores at every selection boundary (the cross-layer one unless layerwise, then each
    layer's): a selection is decided by the scores alone where every gap exceeds twice the scores' error"""
    score_val = np.asarray(score_val, np.float64)
    L, B, H, S = score_val.shape
    gaps = []

    def gap(sorted_scores, n):
        if 0 < n < len(sorted_scores):
            gaps.append(float(sorted_scores[n] - sorted_scores[n - 1]))

    if not layerwise:
        gap(np.sort(score_val.reshape(-1)), int(score_val.size * compression_ratio))
    _, n_pruned = compress_post(score_val, compression_ratio, layerwise)
    for l in range(L):
        for bb in range(B):
            gap(np.sort(score_val[l, bb].reshape(-1)), n_pruned[l])
    return gaps
