"""float64 numpy restatement of KVzip's scorer (include/kvpress_hip.h: kvp_kvzip_score; kvpress/presses/kvzip_press.py:312-354) and of
its selection (compress_post, :360-394).  Test infrastructure only."""
import numpy as np

BAND = 1e-3   # relative distance to a selection threshold inside which the reference and this package may disagree


def rotate_half(x):
    h = x.shape[-1] // 2
    return np.concatenate([-x[..., h:], x[..., :h]], axis=-1)


def rope(q, cos, sin):
    """q [B,Hq,Lq,D], cos / sin [1 or B, Lq, D], float64 throughout"""
    q = np.asarray(q, np.float64)
    return q * np.asarray(cos, np.float64)[:, None] + rotate_half(q) * np.asarray(sin, np.float64)[:, None]


def kvzip_score(q_rot, keys, sink, start, end, row_scale=None, col_scale=None):
    """q_rot: RoPE'd queries [B,Hq,Lq,D]; keys [B,Hkv,S,D] whose last Lq rows belong to the repeated tokens.  Row t sees
    [0, sink) u [start, end) u {S - Lq + u : u <= t}; returns max over (g, t) of softmax * row_scale[t] * col_scale[hG+g, j], [B,Hkv,end-start]"""
    q = np.asarray(q_rot, np.float64)
    k = np.asarray(keys, np.float64)
    B, Hq, Lq, D = q.shape
    Hkv, S = k.shape[1], k.shape[2]
    G, ctx = Hq // Hkv, end - start
    assert 0 <= sink <= start < end <= S - Lq
    ks = np.concatenate([k[:, :, :sink], k[:, :, start:end], k[:, :, S - Lq:]], axis=2)
    logits = np.einsum("bhgtd,bhnd->bhgtn", q.reshape(B, Hkv, G, Lq, D), ks) / np.sqrt(D)
    u = np.arange(Lq)
    logits[..., sink + ctx:] = np.where(u[None, :] <= u[:, None], logits[..., sink + ctx:], -np.inf)
    logits -= logits.max(axis=-1, keepdims=True)
    p = np.exp(logits)
    p = (p / p.sum(axis=-1, keepdims=True))[..., sink:sink + ctx]
    if row_scale is not None:
        p = p * np.asarray(row_scale, np.float64)[:, None, None, :, None]
    if col_scale is not None:
        p = p * np.asarray(col_scale, np.float64).reshape(B, Hkv, G, 1, ctx)
    return p.max(axis=(2, 3))


def plus_scales(hidden, values_chunk, wo, num_heads):
    """KVzip+ (:336-348): 1 / ||h_t|| [B,Lq] and ||V_j Wo_{h,g}||_2 [B,Hq,ctx]; hidden [B,Lq,hidden], values_chunk [B,Hkv,ctx,D],
    wo = o_proj.weight [hidden, Hq*D]"""
    h, v, wo = np.asarray(hidden, np.float64), np.asarray(values_chunk, np.float64), np.asarray(wo, np.float64)
    B, Hkv, ctx, D = v.shape
    G = num_heads // Hkv
    w = wo.T.reshape(Hkv, G, D, -1)
    col = np.linalg.norm(np.einsum("bhtd,hgdj->bhgtj", v, w), axis=-1)
    return 1.0 / np.linalg.norm(h, axis=-1), col.reshape(B, Hkv * G, ctx)


def _bottom(flat, n):
    """indices of the n smallest (ties: the lowest index), ascending; the band around the threshold (the n-th smallest value); the threshold"""
    order = np.argsort(flat, kind="stable")
    if n == 0:
        return np.zeros(0, np.int64), np.zeros(flat.shape, bool), -np.inf
    thr = flat[order[n - 1]]
    with np.errstate(invalid="ignore"):
        band = (np.abs(flat - thr) <= BAND * np.abs(thr)) | (flat == thr)
    return np.sort(order[:n]), band, thr


def compress_post(score_val, compression_ratio, layerwise):
    """score_val [L,1,H,C] -> dict: `counts` [L] (n_pruned_layers); per layer `pruned` (flat indices head * C + position, ascending), `bands`
    (the flat indices within BAND of that layer's threshold `thr`[l]); `global_band` [L, H*C] and `global_thr`: the same for the cross-layer
    threshold (layerwise: empty, -inf)"""
    sv = np.asarray(score_val, np.float64)
    L, B, H, C = sv.shape
    assert B == 1
    per_layer = B * H * C
    global_band, global_thr = np.zeros((L, per_layer), bool), -np.inf
    if layerwise:
        counts = np.full(L, int(per_layer * compression_ratio), np.int64)
    else:
        idx, band, global_thr = _bottom(sv.reshape(-1), int(sv.size * compression_ratio))
        counts = np.bincount(idx // per_layer, minlength=L).astype(np.int64)
        global_band = band.reshape(L, per_layer)
    pruned, bands, thr = [], [], []
    for l in range(L):
        i, b, t = _bottom(sv[l].reshape(-1), int(counts[l]))
        pruned.append(i)
        bands.append(b)
        thr.append(t)
    return dict(counts=counts, pruned=pruned, bands=bands, thr=thr, global_band=global_band, global_thr=global_thr)


def sets_equal_outside(a, b, band):
    """do the index sets a and b agree on every index outside `band` (a boolean mask over the indices)?"""
    diff = np.setxor1d(np.asarray(a, np.int64), np.asarray(b, np.int64))
    return bool(band[diff].all()) if diff.size else True


def rel_err(got, ref):
    """the score contract's error measure: |got - ref| / (|ref| + 1e-3 * row maximum) -- 1e-3 relative plus
    1e-6 x the row maximum is `rel_err <= 1e-3`.  Where the reference is infinite (KVzip+ on a zero hidden state: 1 / ||h|| = inf) the
    same infinity is required, and the row maximum is taken over the finite entries."""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    fin = np.isfinite(ref)
    if not np.array_equal(got[~fin], ref[~fin]):
        return float("inf")
    rowmax = np.abs(np.where(fin, ref, 0.0)).max(axis=-1, keepdims=True)
    err = np.abs(np.where(fin, got, 0.0) - np.where(fin, ref, 0.0)) / (np.abs(np.where(fin, ref, 1.0)) + 1e-3 * rowmax + np.finfo(np.float64).tiny)
    return float(err.max())
