"""Inputs for which float32 arithmetic is exact, for the long reductions (numpy only; test infrastructure).

The 1e-3 score contract on i.i.d. Gaussian inputs cannot see a reduction that loses, doubles or misplaces ONE of its
n terms: the result moves by about 1 / n and n is in the thousands.  Two families of inputs can:

  census   every term is an exactly representable number whose partial sums stay integers below 2^24 (small integers; all-zero logits,
           so that a softmax is exactly uniform).  The result is a count: 1 / n_visible, sum of integers / G.
  impulse  everything is zero except one element at a structural position (a tile, chunk or mask boundary, a ragged tail) that weighs
           about as much as all the others together, so its loss or duplication moves the result by orders of magnitude more than the bound.

Every family has a builder of the inputs (exact in the case's dtype), a closed-form reference with a ``mutant=`` argument, and the
case tables both test files share (tests/test_exact_inputs_host.py on the CPU, tests/test_gpu_exact_reductions.py on the GPU).  The
closed forms are used on the CPU only: to cross-check the oracle and to prove, with the mutants, that one miscounted element would
have failed the GPU test.  The GPU tests compare with the project's oracles, not with these.

Mutants (None: the correct result):
  ("drop", m)      element m is missing from the sum          ("double", m)   element m is counted twice
  (name, +1 / -1)  a boundary moved by one: "causal" (SnapKV's visibility rule), "hidden" (vwl1norm's Wo rows), "n_sink" (ea_score),
                   "S" (the last element of the sequence), "s_prev" (CAM's running sum)
"""
from __future__ import annotations

import math

import numpy as np

import _inputs

TIGHT = 1e-5          # relative, for results that pass through exp2 / log2: at most 40 float32 roundings (2.4e-6) and a 1-ulp hardware exp2 /
                      # log2 on arguments with |log2| <= 17 (about 1.4e-6)
LIMIT = 1 << 24       # integers below it are exact in float32


def is_exact(x: np.ndarray, dtype: str) -> bool:
    x = np.asarray(x, np.float32)
    return bool(np.array_equal(_inputs.round_to(x, dtype), x))


def groups(items, n):
    """items in lists of n, the last one filled up by repeating its last item (one launch carries n positions)"""
    items = list(items)
    out = [items[i:i + n] for i in range(0, len(items), n)]
    out[-1] = out[-1] + [out[-1][-1]] * (n - len(out[-1]))
    return out


def impulse_product(n_keys: int, D: int) -> tuple:
    """(alpha, beta): powers of two, alpha * beta the largest power of two with alpha * beta / sqrt(D) <= ln(n_keys): the heavy key weighs
    between sqrt(n) and n light keys, so both its own miscount and a light key's move the normaliser visibly, and |logit * log2(e)| <= 17"""
    p = max(0, math.floor(math.log2(math.log(max(n_keys, 3)) * math.sqrt(D))))
    assert (2.0 ** p) / math.sqrt(D) * math.log2(math.e) <= 17.0
    return 2.0 ** ((p + 1) // 2), 2.0 ** (p // 2)


def _softmax_weights(ell: np.ndarray) -> np.ndarray:
    ell = np.asarray(ell, np.float64)
    return np.exp(ell - ell.max(-1, keepdims=True))


# =====================================================================================================================================
# A. SnapKV / FINCH window passes
# =====================================================================================================================================
# (W, S, G, D, ks, dtype, B, H)
SNAP_CENSUS = [
    (64, 3000, 4, 128, 5, "bf16", 2, 2),      # hand-scheduled
    (64, 4160, 4, 128, 5, "bf16", 1, 1),      # one-tile workgroups, many partials
    (64, 20000, 4, 128, 5, "bf16", 2, 2),     # also under KVP_SK_SLOTS = 8 and 64
    (64, 3000, 5, 128, 5, "f16", 2, 2),       # compiler-scheduled; two group-blocks
    (33, 2100, 1, 64, 3, "bf16", 2, 2),
    (130, 5000, 13, 96, 3, "bf16", 2, 2),
    (200, 2500, 4, 256, 5, "f16", 2, 2),
    (200, 253, 7, 128, 5, "bf16", 2, 2),      # S < Wp
    (65, 66, 4, 64, 1, "bf16", 2, 2),         # S < Wp
    (1, 5000, 2, 128, 1, "bf16", 2, 2),
    (64, 1500, 2, 128, 5, "f32", 2, 2),       # generic kernels
    (7, 300, 4, 6, 5, "f32", 2, 2),           # generic kernels
]
SNAP_FINCH = [SNAP_CENSUS[0], SNAP_CENSUS[3], SNAP_CENSUS[7]]
SNAP_SLOTS = {2: (8, 64)}                     # index into SNAP_CENSUS -> the KVP_SK_SLOTS values it also runs under
SNAP_IMPULSE = [
    (64, 3000, 4, 128, 5, "bf16", 2, 2),
    (64, 3000, 8, 64, 5, "f16", 2, 2),
    (100, 4200, 4, 256, 5, "bf16", 2, 2),
    (33, 2100, 1, 96, 3, "bf16", 2, 2),
    (64, 1500, 2, 128, 5, "f32", 2, 2),
    # added to the specified table: at S = 20 000 the census moves by 1 / n = 5e-5 only (5 x TIGHT), so the walks, partials and the combine at
    # that length (and under KVP_SK_SLOTS) get an impulse case, whose heavy key moves the result by per cents
    (64, 20000, 4, 128, 5, "bf16", 2, 2),
]
SNAP_IMPULSE_LONG = 5                         # index of the added case: only the mutants that touch the heavy key reach 10 x TIGHT there


def snap_census(W, S, G, D, ks, dtype, B, H, seed=0):
    """q = 0 (every window row uniform over its visible keys), random keys (they cannot matter)"""
    rs = np.random.RandomState(seed + W + S + G + D)
    q = np.zeros((B, H * G, W, D), np.float32)
    k = _inputs.round_to(rs.standard_normal((B, H, S, D)).astype(np.float32), dtype)
    return q, k


def snap_padded_window(W):
    return (W + 63) // 64 * 64


def snap_impulse_positions(W, S):
    """t*: sub-tile and tile edges, the edges of the padded and the real window, and positions inside the window (only rows w >= j may see
    S - W + j)"""
    Wp = snap_padded_window(W)
    mid, last = (S - W) // 256, (S - W) // 128
    t = [0, 31, 32, 127, 128, 128 * mid - 1, 128 * mid, 128 * last - 1, 128 * last, S - Wp - 1, S - Wp, S - W - 1]
    t += [S - W + j for j in (0, 1, W // 2, W - 1)]
    return sorted({x for x in t if 0 <= x < S})


def snap_impulse(W, S, G, D, ks, dtype, tstar, seed=0):
    """every window row of every head alpha e_0; keys zero except k[b, h, t*[b][h], 0] = beta.  tstar: [B][H]"""
    tstar = np.asarray(tstar)
    B, H = tstar.shape
    alpha, beta = impulse_product(S, D)
    q = np.zeros((B, H * G, W, D), np.float32)
    q[..., 0] = alpha
    k = np.zeros((B, H, S, D), np.float32)
    for b in range(B):
        for h in range(H):
            k[b, h, tstar[b, h], 0] = beta
    assert is_exact(q, dtype) and is_exact(k, dtype)
    return q, k


def snap_logits(q, k):
    """[B,H,S] float64: the logits of every window row of every head of a kv head (the builders give all of them the same query)"""
    q, k = np.asarray(q, np.float64), np.asarray(k, np.float64)
    B, Hq, W, D = q.shape
    H = k.shape[1]
    assert (q == q[:, :, :1]).all() and (q.reshape(B, H, Hq // H, W, D) == q.reshape(B, H, Hq // H, W, D)[:, :, :1]).all()
    return np.einsum("bhd,bhsd->bhs", q.reshape(B, H, Hq // H, W, D)[:, :, 0, 0], k) / math.sqrt(D)


def snap_attention_closed(ell, W, mutant=None):
    """[B,H,W,S-W] float64: the window attention of any head of the kv head.  Row w sees the keys t <= S - W + w."""
    ell = np.asarray(ell, np.float64)
    S = ell.shape[-1]
    wt = _softmax_weights(ell)
    csum = np.cumsum(wt, -1)
    shift = mutant[1] if mutant is not None and mutant[0] == "causal" else 0
    last = np.clip(S - W + np.arange(W) + shift, 0, S - 1)                      # the last key row w sees
    Z = csum[..., last]                                                        # [B,H,W]
    if mutant is not None and mutant[0] in ("drop", "double"):
        m = np.broadcast_to(np.asarray(mutant[1]), ell.shape[:-1])             # a position per (b, h), or one for all
        wm = np.take_along_axis(wt, m[..., None], -1)                          # [B,H,1]
        sees = m[..., None] <= last                                            # [B,H,W]
        Z = Z + np.where(sees, wm if mutant[0] == "double" else -wm, 0.0)
    return wt[..., None, :S - W] / Z[..., None]


def _pool(s, ks):
    pad = ks // 2
    sp = np.pad(s, [(0, 0)] * (s.ndim - 1) + [(pad, pad)])
    return sum(sp[..., j:j + s.shape[-1]] for j in range(ks)) / ks


def snap_closed(ell, W, ks, mutant=None, finch=None):
    """[B,H,S] float32 as oracle.snapkv_score gives it (finch = None) or oracle.finch_score(normalize_scores=finch)"""
    attn = snap_attention_closed(ell, W, mutant)
    S = np.asarray(ell).shape[-1]
    if finch:
        attn = attn * np.arange(S - W, S, dtype=np.float64)[:, None]
    sc = attn.mean(-2)
    if finch is None:
        sc = _pool(sc, ks)
    fill = float(np.float32(sc.max())) + 1.0
    return np.concatenate([sc, np.full(sc.shape[:-1] + (W,), fill)], -1).astype(np.float32)


# =====================================================================================================================================
# B. ExpectedAttention
# =====================================================================================================================================
def qstats_plan(Sq, nbh):
    """(nchunk, rows) as ea_mfma.hip's qstats_plan: the rows of one float32 partial"""
    cap = min(32, max(1, 512 // max(1, nbh)))
    nc = min(cap, max(1, (Sq + 4095) // 4096))
    nc = max(nc, min(32, (Sq + 16383) // 16384))
    r = ((Sq + nc - 1) // nc + 63) // 64 * 64
    return (Sq + r - 1) // r, r


# (dtype, D, B, Hq, Sq, layout, rows)   layout: "q_proj" = [B, Sq, Hq * D] seen as [B, Hq, Sq, D]; rows: the chunk length qstats_plan gives
EA_QSTATS = [
    ("bf16", 128, 1, 3, 10000, "q_proj", 3392),        # matrix cores; 3 heads -> 3 chunks of 3392 rows
    ("f16", 64, 2, 2, 4500, "q_proj", 2304),           # matrix cores, pairs of heads: 2 "heads" of 128 -> 2 chunks of 2304 rows
    ("f16", 64, 2, 2, 4500, "contiguous", 2304),       # matrix cores, zero-padded to 128: 4 heads -> 2 chunks of 2304
    ("bf16", 96, 1, 3, 5000, "contiguous", 2560),      # matrix cores, zero-padded: 2 chunks of 2560
    ("bf16", 256, 1, 2, 4200, "contiguous", 2112),     # matrix cores, six pairs of quarters per head: 2 chunks of 2112
    ("f32", 128, 1, 2, 4500, "contiguous", 2304),      # generic (the plan of the matrix-core path: positions only)
    ("bf16", 128, 1, 2, 4095, "contiguous", 4096),     # generic: below 4096 rows
    ("bf16", 128, 2, 3, 257, "contiguous", 320),       # generic
]


def ea_qstats_rows(dtype, D, B, Hq, Sq, layout):
    nbh = B * Hq // 2 if (D == 64 and layout == "q_proj") else B * Hq * 6 if D == 256 else B * Hq
    return qstats_plan(Sq, nbh)[1]


def ea_structural_rows(Sq, rows):
    return sorted({r for r in (0, 15, 16, 63, 64, rows - 1, rows, Sq - 17, Sq - 16, Sq - 1) if 0 <= r < Sq})


def _strip_pairs(D):
    n = D // 32
    pairs = [(a, b) for a in range(n) for b in range(a + 1, n)]
    return sorted(pairs, key=lambda p: (p[0] // 2 == p[1] // 2, p))            # different 64-dimension strips first


def ea_qstats_inputs(dtype, D, B, Hq, Sq, layout, rows, seed=0):
    """census: integers in [-2, 3] (non-zero mean); impulse: the structural rows are zero except +64 / -64 on a pair of dimensions in
    different 32-dimension strips (different 64-dimension strips first), another pair for every head and row.  Returns q [B,Hq,Sq,D]
    float32 and the structural rows."""
    rs = np.random.RandomState(seed + D + Sq)
    q = rs.randint(-2, 4, size=(B, Hq, Sq, D)).astype(np.float32)
    srows = ea_structural_rows(Sq, rows)
    pairs = _strip_pairs(D)
    for b in range(B):
        for h in range(Hq):
            for m, r in enumerate(srows):
                sa, sb = pairs[(m + 3 * h + b) % len(pairs)]
                q[b, h, r] = 0.0
                q[b, h, r, 32 * sa + (5 * m + h) % 32] = 64.0
                q[b, h, r, 32 * sb + (11 * m + 3 * h + 1) % 32] = -64.0
    assert is_exact(q, dtype)
    return q, srows


def ea_qstats_moments(q):
    """(sum x [B,Hq,D], sum x x^T [B,Hq,D,D]) as float64 holding exact integers"""
    x = np.asarray(q, np.float64)
    return x.sum(2), np.einsum("bhsi,bhsj->bhij", x, x)


def ea_qstats_closed(q, mutant=None, moments=None):
    """(mu, cov) float64 from the integer raw moments.  Mutants: ("drop2" / "double2", m) row m in the second moments only (the syrk and
    the column sums are separate instructions), ("drop1" / "double1", m) in the column sums only, ("S", -1) the last row missing from both,
    ("S", +1) the last row read again for the row past the end."""
    x = np.asarray(q, np.float64)
    n = x.shape[2]
    s1, s2 = moments if moments is not None else ea_qstats_moments(x)
    if mutant is not None:
        kind, m = mutant
        if kind == "S":
            kind, m = ("drop" if m < 0 else "double"), n - 1
            row = x[:, :, m]
            sg = -1.0 if kind == "drop" else 1.0
            s1 = s1 + sg * row
            s2 = s2 + sg * row[..., :, None] * row[..., None, :]
        else:
            row = x[:, :, m]
            sg = -1.0 if kind.startswith("drop") else 1.0
            if kind.endswith("1"):
                s1 = s1 + sg * row
            else:
                s2 = s2 + sg * row[..., :, None] * row[..., None, :]
    mu = s1 / n
    return mu, s2 / n - mu[..., :, None] * mu[..., None, :]


def ea_qstats_errors(mu, cov, mu_w, cov_w):
    """the GPU test's metric: (max |d mu| / max |mu|, max |d cov_ij| / sqrt(cov_ii cov_jj))"""
    mu_w, cov_w = np.asarray(mu_w, np.float64), np.asarray(cov_w, np.float64)
    d = np.sqrt(np.einsum("bhii->bhi", cov_w))
    return (float(np.abs(mu - mu_w).max() / np.abs(mu_w).max()),
            float((np.abs(cov - cov_w) / (d[..., :, None] * d[..., None, :])).max()))


# (S, G, D, n_sink, dtype, B, H)
EA_SCORE = [
    (4100, 4, 128, 4, "bf16", 2, 2),
    (9001, 8, 128, 7, "f16", 1, 2),
    (6000, 2, 64, 0, "bf16", 2, 2),
    (6000, 4, 96, 4, "bf16", 1, 2),
    (1000, 3, 128, 1, "bf16", 2, 2),
    (4500, 3, 128, 4, "bf16", 1, 2),          # G = 3: the three-kernel path
]


def ea_onehot_values(B, H, S, D, dtype, rs):
    """value rows with one non-zero entry 2^k: the norm is exactly 2^k"""
    v = np.zeros((B, H, S, D), np.float32)
    d = rs.randint(0, D, size=(B, H, S))
    e = rs.randint(-3, 4, size=(B, H, S))
    np.put_along_axis(v, d[..., None], (2.0 ** e)[..., None].astype(np.float32), -1)
    assert is_exact(v, dtype)
    return v


def ea_score_census(S, G, D, n_sink, dtype, B, H, seed=0):
    """mu = 0, random keys (they cannot matter), one-hot values: every scored key gets 1 / (S - n_sink), times its value norm"""
    rs = np.random.RandomState(seed + S + G + D)
    k = _inputs.round_to(rs.standard_normal((B, H, S, D)).astype(np.float32), dtype)
    return k, ea_onehot_values(B, H, S, D, dtype, rs), np.zeros((B, H * G, D), np.float32)


def ea_score_positions(S, n_sink):
    return sorted({t for t in (n_sink - 1, n_sink, 127, 128, 4095, 4096, S - 1) if 0 <= t < S})


def ea_score_impulse(S, G, D, n_sink, dtype, tstar, seed=0):
    """mu = alpha e_0 for every head; keys zero except k[b, h, t*[b][h], 0] = beta; one-hot values"""
    tstar = np.asarray(tstar)
    B, H = tstar.shape
    alpha, beta = impulse_product(S - n_sink, D)
    mu = np.zeros((B, H * G, D), np.float32)
    mu[..., 0] = alpha
    k = np.zeros((B, H, S, D), np.float32)
    for b in range(B):
        for h in range(H):
            k[b, h, tstar[b, h], 0] = beta
    assert is_exact(k, dtype) and is_exact(mu, "bf16")
    return k, ea_onehot_values(B, H, S, D, dtype, np.random.RandomState(seed + S)), mu


def ea_score_logits(k, mu):
    """[B,H,S] float64 (cov = 0 or None; the builders give every head of a kv head the same mu)"""
    k, mu = np.asarray(k, np.float64), np.asarray(mu, np.float64)
    B, H, S, D = k.shape
    mg = mu.reshape(B, H, -1, D)
    assert (mg == mg[:, :, :1]).all()
    return np.einsum("bhd,bhsd->bhs", mg[:, :, 0], k) / math.sqrt(D)


def ea_score_closed(ell, v, n_sink, use_vnorm, eps=0.0, mutant=None):
    """[B,H,S] float32 as oracle.ea_score.  Mutants: drop / double key m in the normaliser, ("n_sink", d): the normaliser starts at
    n_sink + d, ("S", -1): it ends one key early."""
    ell = np.asarray(ell, np.float64)
    full = np.exp(ell - ell[..., n_sink:].max(-1, keepdims=True))              # all keys, on the scale of the scored ones
    wt = full[..., n_sink:]
    Z = wt.sum(-1, keepdims=True)
    if mutant is not None:
        kind, m = mutant
        if kind in ("drop", "double"):
            m = np.broadcast_to(np.asarray(m), ell.shape[:-1])
            wm = np.take_along_axis(full, m[..., None], -1)
            Z = Z + (wm if kind == "double" else -wm)
        elif kind == "n_sink":
            Z = full[..., max(n_sink + m, 0):].sum(-1, keepdims=True)
        elif kind == "S":
            assert m == -1
            Z = Z - full[..., -1:]
        else:
            raise ValueError(mutant)
    sc = wt / Z
    if use_vnorm:
        vv = np.asarray(v, np.float64)[:, :, n_sink:]
        sc = (sc + eps) * np.sqrt((vv * vv).sum(-1))
    fill = float(np.float32(sc.max())) + 1.0
    return np.concatenate([np.full(sc.shape[:-1] + (n_sink,), fill), sc], -1).astype(np.float32)


# =====================================================================================================================================
# C. vwl1norm
# =====================================================================================================================================
VWL1_HIDDEN = (1, 24, 31, 32, 33, 63, 64, 65, 127, 128, 129, 320, 328)
VWL1_S, VWL1_HKV = 70, 2


def vwl1_census_cases(D):
    """(hidden, G, dtype) for the matrix-core head sizes 64, 96, 128, 256: every hidden with every D; G in {1, 3, 4, 8} and both 16-bit
    dtypes cycle so that every (G, dtype), (hidden, G) neighbourhood and (D, G, dtype) occurs"""
    di = (64, 96, 128, 256).index(D)
    return [(hid, (1, 3, 4, 8)[(i + di) % 4], ("bf16", "f16")[(i // 4 + di) % 2]) for i, hid in enumerate(VWL1_HIDDEN)]


VWL1_GENERIC = [(129, 4, "f32", 16), (328, 3, "f32", 16), (33, 8, "bf16", 16), (320, 1, "bf16", 16)]      # (hidden, G, dtype, D)


def vwl1_tile(D):
    return 64 if D == 256 else 128             # Wo rows per tile (vwl1.hip: Geo::WT)


def vwl1_census(hidden, G, dtype, D, seed=0, S=VWL1_S, Hkv=VWL1_HKV, B=1):
    """integers in [-2, 2]: every dot product and every abs-sum is an integer below 2^24; float32 scores of both signs"""
    rs = np.random.RandomState(seed + hidden * 7 + G + D)
    v = rs.randint(-2, 3, size=(B, Hkv, S, D)).astype(np.float32)
    wo = rs.randint(-2, 3, size=(hidden, Hkv * G * D)).astype(np.float32)
    sc = (3.0 * rs.standard_normal((B, Hkv, S))).astype(np.float32)
    assert 4 * D * hidden * G < LIMIT
    return v, wo, sc


def vwl1_row_sums(v, wo, G):
    """[B,Hkv,S,hidden] float64 holding exact integers: sum_g |sum_d v w| of every Wo row"""
    v = np.asarray(v, np.float64)
    B, H, S, D = v.shape
    w = np.asarray(wo, np.float64).reshape(wo.shape[0], H, G, D)
    return np.abs(np.einsum("bhsd,chgd->bhsgc", v, w)).sum(3)


def vwl1_closed(v, wo, G, mutant=None):
    """norm [B,Hkv,S] float64.  Mutants: drop / double Wo row m; ("hidden", -1) the last row masked away, ("hidden", +1) the row past the end
    -- requested clamped to the last one -- not masked"""
    rows = vwl1_row_sums(v, wo, G)
    total = rows.sum(-1)
    if mutant is not None:
        kind, m = mutant
        if kind == "hidden":
            kind, m = ("drop" if m < 0 else "double"), rows.shape[-1] - 1
        total = total + (rows[..., m] if kind == "double" else -rows[..., m])
    return total / G


def vwl1_rescale_expected(sc, norm32, eps):
    """float32 (sc + eps) * norm in that order, every step rounded"""
    return np.float32(np.float32(np.asarray(sc, np.float32) + np.float32(eps)) * np.asarray(norm32, np.float32))


# (hidden, G, dtype, D)
VWL1_IMPULSE = [(328, 4, "bf16", 128), (328, 4, "f16", 256), (129, 8, "bf16", 64), (320, 3, "f16", 96), (33, 1, "bf16", 128),
                (129, 4, "f32", 16)]


def vwl1_impulse_rows(hidden, D):
    WT = vwl1_tile(D)
    return sorted({c for c in (0, 31, 32, WT - 1, WT, hidden - 2, hidden - 1) if 0 <= c < hidden})


def vwl1_impulse(hidden, G, dtype, D, seed=0, S=VWL1_S, Hkv=VWL1_HKV, B=1):
    """wo zero except, in every kv head's column block, one power of two per selected row (row c_m, head g_m, dimension d_m); random v.
    Returns v, wo and the entries [(c, g, d, w)]."""
    rs = np.random.RandomState(seed + hidden + D)
    v = _inputs.round_to(rs.standard_normal((B, Hkv, S, D)).astype(np.float32), dtype)
    wo = np.zeros((hidden, Hkv * G * D), np.float32)
    entries = []
    for m, c in enumerate(vwl1_impulse_rows(hidden, D)):
        g, d, w = m % G, (37 * m + 5) % D, 2.0 ** ((m % 5) - 2) * (-1.0) ** m
        entries.append((c, g, d, w))
        for h in range(Hkv):
            wo[c, (h * G + g) * D + d] = w
    assert is_exact(wo, dtype)
    return v, wo, entries


def vwl1_impulse_closed(v, entries, G, mutant=None):
    """(1 / G) sum_m |v[s, d_m]| |w_m|, float64"""
    v = np.asarray(v, np.float64)
    terms = np.stack([np.abs(v[..., d]) * abs(w) for (_, _, d, w) in entries], -1)
    total = terms.sum(-1)
    if mutant is not None:
        kind, m = mutant
        if kind == "hidden":
            kind, m = ("drop" if m < 0 else "double"), len(entries) - 1          # the last selected row is hidden - 1
        total = total + (terms[..., m] if kind == "double" else -terms[..., m])
    return total / G


# =====================================================================================================================================
# D. CAM step attention
# =====================================================================================================================================
# (S, G, D, dtype, B, H)
CAM_CASES = [
    (257, 1, 6, "f32", 2, 2),
    (4097, 4, 128, "bf16", 2, 2),
    (4097, 9, 64, "f16", 2, 2),
    (20000, 16, 256, "bf16", 1, 2),
    (4097, 4, 8, "bf16", 2, 2),
]
CAM_SWAP = (4097, 4, 128, "bf16", 2, 2)      # the case that also runs with cos = 0, sin = 1 (a signed permutation)


def cam_chunk(R, S):
    """keys per pass-1 workgroup as cam.hip's cam_chunk (R = B * Hkv).  It is NOT a constant 1024: about 1024 workgroups over all rows,
    whole 64-key groups, at most 256 chunks per row -- 64 keys at S = 4097 and R = 4, 128 at S = 20 000"""
    c = max((S * R + 1023) // 1024, (S + 255) // 256)
    return max(64, (c + 63) // 64 * 64)


def cam_positions(S, chunk):
    last = (S - 1) // chunk * chunk
    return sorted({t for t in (0, 255, 256, chunk - 1, chunk, 1023, 1024, last - 1, last, S - 1) if 0 <= t < S})


def cam_rotary(D, swap=False):
    one, zero = np.ones((1, 1, D), np.float32), np.zeros((1, 1, D), np.float32)
    return (zero, one) if swap else (one, zero)


def cam_census(S, G, D, dtype, B, H, seed=0):
    rs = np.random.RandomState(seed + S + G + D)
    return np.zeros((B, H * G, 1, D), np.float32), _inputs.round_to(rs.standard_normal((B, H, S, D)).astype(np.float32), dtype)


def cam_impulse(S, G, D, dtype, tstar, swap=False):
    """the newest query alpha e_0 before the rotation for every head; keys zero except beta at t* on the dimension the rotated query
    lands on (0 for the identity table; D / 2 for cos = 0, sin = 1, where q_rot = rotate_half(q))"""
    tstar = np.asarray(tstar)
    B, H = tstar.shape
    alpha, beta = impulse_product(S, D)
    q = np.zeros((B, H * G, 1, D), np.float32)
    q[..., 0] = alpha
    k = np.zeros((B, H, S, D), np.float32)
    for b in range(B):
        for h in range(H):
            k[b, h, tstar[b, h], D // 2 if swap else 0] = beta
    assert is_exact(q, dtype) and is_exact(k, dtype)
    return q, k


def cam_logits(q, k, swap=False):
    q, k = np.asarray(q, np.float64), np.asarray(k, np.float64)
    B, Hq, _, D = q.shape
    H = k.shape[1]
    qg = q[:, :, 0].reshape(B, H, Hq // H, D)
    assert (qg == qg[:, :, :1]).all()
    q0 = qg[:, :, 0]
    if swap:
        q0 = np.concatenate([-q0[..., D // 2:], q0[..., :D // 2]], -1)
    return np.einsum("bhd,bhsd->bhs", q0, k) / math.sqrt(D)


def cam_prev(B, H, cap, seed=7):
    return np.random.RandomState(seed).gamma(0.5, 1.0, size=(B, H, cap)).astype(np.float32) + np.float32(0.125)


def cam_closed(ell, prev, s_prev, mutant=None):
    """running[:S] float64 after the step.  Mutants: drop / double key m in the normaliser, ("S", -1) the last key missing from it,
    ("s_prev", d) the boundary between kept and stale running sums moved by d"""
    ell = np.asarray(ell, np.float64)
    S = ell.shape[-1]
    wt = _softmax_weights(ell)
    Z = wt.sum(-1, keepdims=True)
    sp = s_prev
    if mutant is not None:
        kind, m = mutant
        if kind in ("drop", "double"):
            m = np.broadcast_to(np.asarray(m), ell.shape[:-1])
            wm = np.take_along_axis(wt, m[..., None], -1)
            Z = Z + (wm if kind == "double" else -wm)
        elif kind == "S":
            Z = Z - wt[..., -1:]
        elif kind == "s_prev":
            sp = min(max(s_prev + m, 0), S)
        else:
            raise ValueError(mutant)
    out = wt / Z
    out[..., :sp] += np.asarray(prev, np.float64)[..., :sp]
    return out


def rel_err(got, want):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    return float((np.abs(got - want) / np.maximum(np.abs(want), 1e-300)).max())
