"""The exact-input cases of tests/_exact_inputs.py, checked on the CPU (no GPU needed):

  a. the closed form equals the float64 oracle: 1e-12 relative wherever the oracle hands out float64 (window attention, query statistics,
     vwl1norm, CAM's attention row); where it rounds its result to float32 (snapkv_score, finch_score, ea_score) to that rounding, 1.2e-7;
  b. the inputs are what makes float32 exact: integers whose sums stay below 2^24, or logits that are 0 except one single product;
  c. sensitivity: every mutant of the closed form moves at least one compared output by at least 10 x the GPU test's tolerance, in the
     GPU test's own metric -- the new GPU tests would fail on a kernel that miscounts ONE element.  Census cases are held to every
     mutant.  Impulse cases are held to the mutants in which the heavy element is the miscounted one: next to a heavy key of e^L <= n
     light keys a miscounted LIGHT key moves the normaliser by 0.5 / n .. 1 / n only, which is the census's business.  At S = 20 000
     the census itself moves by 1 / n = 5e-5, 5 x TIGHT: asserted as such (>= 4 x), and an impulse case at that length carries the 10 x;
  d. the gap: the same drop-one mutant on the i.i.d. inputs of test_ea_qstats_mfma_multichunk and of
     test_snapkv_any_window_on_the_mfma_path[64-3000-4-5] stays inside those tests' tolerances.

The oracles are per (batch, kv head) independent, so the cases run here with B = 1 and at most two kv heads."""
import numpy as np
import pytest

import _cam_oracle as CAMO
import _critical_oracle as CO
import _exact_inputs as X
import _inputs
from oracle import kvpress_oracle as O

TIGHT = X.TIGHT
F32 = 1.2e-7        # the oracle's own rounding of its result to float32
NEED = 10 * TIGHT


def rows_err(got, want, sl=slice(None)):
    """the GPU tests' relative error, worst per (b, h) row"""
    got, want = np.asarray(got, np.float64)[..., sl], np.asarray(want, np.float64)[..., sl]
    return (np.abs(got - want) / np.maximum(np.abs(want), 1e-300)).max(-1)


# ---- A. SnapKV / FINCH -------------------------------------------------------------------------------------------------------------
def _snap_check_a(q, k, W, ks, finch_modes=()):
    ell = X.snap_logits(q, k)
    G = q.shape[1] // k.shape[1]
    attn = np.repeat(X.snap_attention_closed(ell, W), G, axis=1)
    assert X.rel_err(attn, O.snapkv_window_attention(q, k)) <= 1e-12
    want = O.snapkv_score(q, k, ks)
    got = X.snap_closed(ell, W, ks)
    assert X.rel_err(got, want) <= F32
    for mode in finch_modes:
        assert X.rel_err(X.snap_closed(ell, W, 1, finch=mode), O.finch_score(q, k, mode)) <= F32
    return ell, got


@pytest.mark.parametrize("case", X.SNAP_CENSUS, ids=lambda c: "-".join(map(str, c[:6])))
def test_snap_census(case):
    W, S, G, D, ks, dtype, _, _ = case
    q, k = X.snap_census(W, S, G, D, ks, dtype, 1, 1)
    assert not q.any() and X.is_exact(k, dtype)                                                   # b: every logit is exactly 0
    finch = case in X.SNAP_FINCH
    ell, ref = _snap_check_a(q, k, W, ks, (True, False) if finch else ())                         # a
    need = NEED if S <= 10000 else 4 * TIGHT                                                      # c
    if S > 10000:
        assert any(c[1] == S for c in X.SNAP_IMPULSE)
    # (W = 1: the only window row sees all S keys, there is no key a rule moved by +1 could add)
    for mutant in [("drop", 0), ("drop", S - W - 1), ("double", (S - W) // 2), ("causal", -1)] + ([("causal", 1)] if W > 1 else []):
        moved = rows_err(X.snap_closed(ell, W, ks, mutant), ref, slice(0, S - W)).min()
        assert moved >= need, (case, mutant, moved)
        if finch:
            moved = rows_err(X.snap_closed(ell, W, 1, mutant, finch=True), X.snap_closed(ell, W, 1, finch=True), slice(0, S - W)).min()
            assert moved >= need, (case, mutant, "finch", moved)


def snap_impulse_mutants(W, S, t):
    """the mutants that miscount the heavy key at t"""
    out = [("drop", t), ("double", t)]
    if t >= S - W:
        out.append(("causal", -1))            # row t - (S - W) loses it
        if t > S - W:
            out.append(("causal", 1))         # the row before gains it
    return out


@pytest.mark.parametrize("case", X.SNAP_IMPULSE, ids=lambda c: "-".join(map(str, c[:6])))
def test_snap_impulse(case):
    W, S, G, D, ks, dtype, _, _ = case
    G = min(G, 2)                                                 # (the heads of a kv head are copies of each other: two are enough here)
    alpha, beta = X.impulse_product(S, D)
    assert alpha * beta / np.sqrt(D) <= np.log(S) < 2 * alpha * beta / np.sqrt(D)
    for t in X.snap_impulse_positions(W, S):
        q, k = X.snap_impulse(W, S, G, D, ks, dtype, [[t]])
        assert np.count_nonzero(q) == q[..., 0].size and np.count_nonzero(k) == 1                # b: one non-zero product per logit
        ell, ref = _snap_check_a(q, k, W, ks)                                                     # a
        for mutant in snap_impulse_mutants(W, S, t):                                              # c
            moved = rows_err(X.snap_closed(ell, W, ks, mutant), ref, slice(0, S - W)).min()
            assert moved >= NEED, (case, t, mutant, moved)


def test_snap_gap_on_gaussian_inputs():
    """d: test_snapkv_any_window_on_the_mfma_path at (W, S, G, ks) = (64, 3000, 4, 5), D = 128, with ONE key missing from the normaliser of
    every row that sees it, for every 97th key in turn: the typical lost key moves the scores by less than RTOL = 1e-3 and the present test
    passes (a key with one of the largest logits can reach 1e-3: the Gaussian inputs see some lost keys, by luck, and not most)"""
    W, S, G, ks, D = 64, 3000, 4, 5, 128
    rs = np.random.RandomState(W * 131 + S + G + D)
    B, H = 2, 2
    q = _inputs.round_to((rs.standard_normal((B, H * G, W, D)) * 1.5).astype(np.float32), "bf16")
    k = rs.standard_normal((B, H, S, D)).astype(np.float32)
    k[1, :, : S // 3] *= 3.0
    k = _inputs.round_to(k, "bf16")
    attn = O.snapkv_window_attention(q, k)
    want = O._snapkv_from_window_attn(attn, H, W, ks, np.float64)[..., :-W]
    moved = []
    for m in range(0, S - W, 97):
        mutated = O._snapkv_from_window_attn(attn / (1.0 - attn[..., m:m + 1]), H, W, ks, np.float64)[..., :-W]
        moved.append(rows_err(mutated, want))                          # [B,H]: every kv head has lost its own key m
    moved = np.stack(moved)
    print(f"SnapKV, Gaussian inputs, one key missing from the normaliser: scores of its kv head move by {np.median(moved):.3g} (median), "
          f"{moved.max():.3g} (largest); {100 * (moved <= 1e-3).mean():.0f}% of the lost keys stay inside RTOL 1e-3")
    assert moved.min() > 0 and np.median(moved) <= 1e-3 and (moved <= 1e-3).mean() >= 0.5


# ---- B. ExpectedAttention ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", X.EA_QSTATS, ids=lambda c: "-".join(map(str, c)))
def test_ea_qstats(case):
    dtype, D, B, Hq, Sq, layout, rows = case
    assert rows == X.ea_qstats_rows(dtype, D, B, Hq, Sq, layout)
    q, srows = X.ea_qstats_inputs(dtype, D, 1, min(Hq, 2), Sq, layout, rows)
    s1, s2 = X.ea_qstats_moments(q)
    # b: integers; |sum x_i x_j| over any subset of rows <= sqrt(sum x_i^2 sum x_j^2) <= the largest diagonal entry
    assert np.array_equal(q, np.round(q)) and np.einsum("bhii->bhi", s2).max() < X.LIMIT and np.abs(s1).max() < X.LIMIT
    for b in range(q.shape[0]):
        for h in range(q.shape[1]):
            pairs = {tuple(np.flatnonzero(q[b, h, r])) for r in srows}
            assert all(len(p) == 2 and p[0] // 32 != p[1] // 32 for p in pairs) and len(pairs) >= min(len(srows), 3)
    mu_w, cov_w = O.ea_query_stats(q, True)
    mu, cov = X.ea_qstats_closed(q, moments=(s1, s2))
    assert max(X.ea_qstats_errors(mu, cov, mu_w, cov_w)) <= 1e-12                                  # a
    ordinary = next(r for r in range(100, Sq) if r not in srows)
    mutants = [(kind, r) for r in srows + [ordinary] for kind in ("drop2", "double2", "drop1", "double1")] + [("S", -1), ("S", 1)]
    for mutant in mutants:                                                                         # c
        moved = max(X.ea_qstats_errors(*X.ea_qstats_closed(q, mutant, (s1, s2)), mu, cov))
        assert moved >= NEED, (case, mutant, moved)


def test_ea_qstats_gap_on_gaussian_inputs():
    """d: test_ea_qstats_mfma_multichunk's inputs with the last row missing from the oracle's (centred) second moments only: inside that
    test's bounds (1e-3 at most, 1e-4 on average).  The test owes what it does see to its large means: the matrix-core kernel accumulates
    RAW moments, and a row x lost there is x x^T / n, which at |mean| = 10 sigma is far outside (printed); on queries with small means
    the two are the same and neither shows."""
    rs = np.random.RandomState(7)
    B, Hq, Sq, D = 1, 3, 10000, 128
    q = rs.standard_normal((B, Hq, Sq, D)).astype(np.float32) * np.exp(0.5 * rs.standard_normal((1, Hq, 1, D))).astype(np.float32)
    q += rs.standard_normal((1, Hq, 1, D)).astype(np.float32) * 3.0
    q[:, :, :, ::17] *= 6.0
    q = _inputs.round_to(q, "bf16")
    mu_w, cov_w = O.ea_query_stats(q, True)
    d = np.sqrt(np.einsum("bhii->bhi", cov_w))
    scale = d[..., :, None] * d[..., None, :]
    last = q[:, :, -1].astype(np.float64)
    c = last - mu_w
    err = np.abs(c[..., :, None] * c[..., None, :] / Sq) / scale
    raw = np.abs(last[..., :, None] * last[..., None, :] / Sq) / scale
    print(f"EA query statistics, Gaussian inputs, last row missing from the second moments: centred {err.max():.3g} at most, {err.mean():.3g} "
          f"on average; raw {raw.max():.3g} at most, {raw.mean():.3g} on average")
    assert 0 < err.max() <= 1e-3 and err.mean() <= 1e-4


def ea_score_mutants(S, n_sink, t):
    out = [("drop", t), ("double", t)] if t >= n_sink else []
    if t == n_sink:
        out.append(("n_sink", 1))
    if t == n_sink - 1:
        out.append(("n_sink", -1))
    if t == S - 1:
        out.append(("S", -1))
    return out


@pytest.mark.parametrize("case", X.EA_SCORE, ids=lambda c: "-".join(map(str, c[:5])))
def test_ea_score(case):
    S, G, D, ns, dtype, _, _ = case
    B, H, G = 1, 2, min(G, 2)                                     # (the heads of a kv head are copies of each other: two are enough here)
    # census
    k, v, mu = X.ea_score_census(S, G, D, ns, dtype, B, H)
    norms = np.sqrt((v.astype(np.float64) ** 2).sum(-1))
    assert not mu.any() and (np.count_nonzero(v, axis=-1) == 1).all() and np.array_equal(np.log2(norms), np.round(np.log2(norms)))   # b
    ell = X.ea_score_logits(k, mu)
    for use_vnorm in (True, False):
        ref = X.ea_score_closed(ell, v, ns, use_vnorm)
        for cov in (None, np.zeros((B, H * G, D, D), np.float32)) if use_vnorm else (None,):
            assert X.rel_err(ref, O.ea_score(k, v, mu, cov, ns, use_vnorm, 0.0)) <= F32           # a
        if not use_vnorm:
            assert np.array_equal(ref[..., ns:], np.full((B, H, S - ns), np.float32(1.0 / (S - ns))))
        mutants = [("drop", ns + 5), ("double", S - 1), ("n_sink", 1), ("S", -1)] + ([("n_sink", -1)] if ns else [])
        for mutant in mutants:                                                                     # c
            moved = rows_err(X.ea_score_closed(ell, v, ns, use_vnorm, mutant=mutant), ref, slice(ns, None)).min()
            assert moved >= NEED, (case, mutant, moved)
    # impulse
    for pos in X.groups(X.ea_score_positions(S, ns), H):
        k, v, mu = X.ea_score_impulse(S, G, D, ns, dtype, [pos])
        assert np.count_nonzero(k) == H and np.count_nonzero(mu) == H * G                         # b
        ell = X.ea_score_logits(k, mu)
        ref = X.ea_score_closed(ell, v, ns, True)
        assert X.rel_err(ref, O.ea_score(k, v, mu, None, ns, True, 0.0)) <= F32                   # a
        for h, t in enumerate(pos):
            for mutant in ea_score_mutants(S, ns, t):                                              # c
                moved = rows_err(X.ea_score_closed(ell, v, ns, True, mutant=mutant), ref, slice(ns, None))[0, h]
                assert moved >= NEED, (case, t, mutant, moved)


# ---- C. vwl1norm -------------------------------------------------------------------------------------------------------------------
def _ulps(a, b):
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    return np.abs(a.view(np.int32).astype(np.int64) - b.view(np.int32).astype(np.int64))


def _vwl1_cases():
    return [(hid, G, dt, D) for D in (64, 96, 128, 256) for hid, G, dt in X.vwl1_census_cases(D)] + X.VWL1_GENERIC


def test_vwl1_census_sweep_covers_every_value():
    cases = _vwl1_cases()
    assert {c[0] for c in cases} == set(X.VWL1_HIDDEN) and {c[1] for c in cases} == {1, 3, 4, 8}
    for D in (64, 96, 128, 256):
        mine = [c for c in cases if c[3] == D]
        assert {c[0] for c in mine} == set(X.VWL1_HIDDEN) and {(c[1], c[2]) for c in mine} == {(g, d) for g in (1, 3, 4, 8) for d in ("bf16", "f16")}
    assert ("f32", 16) in {c[2:] for c in cases} and ("bf16", 16) in {c[2:] for c in cases}


def test_vwl1_census():
    for hidden, G, dtype, D in _vwl1_cases():
        v, wo, sc = X.vwl1_census(hidden, G, dtype, D)
        assert X.is_exact(v, dtype) and X.is_exact(wo, dtype) and np.array_equal(v, np.round(v)) and np.array_equal(wo, np.round(wo))
        rows = X.vwl1_row_sums(v, wo, G)
        assert rows.sum(-1).max() < X.LIMIT and np.array_equal(rows, np.round(rows))              # b
        ref = X.vwl1_closed(v, wo, G)
        assert X.rel_err(ref, CO.vwl1norm(v, wo, X.VWL1_HKV * G)) <= 1e-12                         # a
        ref32 = ref.astype(np.float32)
        if G != 3:
            assert np.array_equal(ref32.astype(np.float64), ref)                                  # an integer over a power of two
        # c: the GPU test asks for the same bits (G = 3: 1 ulp); every mutant is off by more than 10 ulps somewhere
        for mutant in [("drop", 0), ("drop", hidden // 2), ("double", hidden - 1), ("hidden", -1), ("hidden", 1)]:
            mut32 = X.vwl1_closed(v, wo, G, mutant).astype(np.float32)
            assert _ulps(mut32, ref32).max() > 10, (hidden, G, dtype, D, mutant)
            assert _ulps(X.vwl1_rescale_expected(sc, mut32, 1e-4), X.vwl1_rescale_expected(sc, ref32, 1e-4)).max() > 10


@pytest.mark.parametrize("case", X.VWL1_IMPULSE, ids=lambda c: "-".join(map(str, c)))
def test_vwl1_impulse(case):
    hidden, G, dtype, D = case
    v, wo, entries = X.vwl1_impulse(hidden, G, dtype, D)
    assert X.is_exact(v, dtype) and (np.count_nonzero(wo, axis=1) <= X.VWL1_HKV).all()             # b: one product per (row, kv head)
    assert [e[0] for e in entries] == X.vwl1_impulse_rows(hidden, D) and entries[-1][0] == hidden - 1
    ref = X.vwl1_impulse_closed(v, entries, G)
    assert X.rel_err(ref, CO.vwl1norm(v, wo, X.VWL1_HKV * G)) <= 1e-12                             # a
    mutants = [(kind, m) for m in range(len(entries)) for kind in ("drop", "double")] + [("hidden", -1), ("hidden", 1)]
    for mutant in mutants:                                                                         # c: the GPU test's bound is 1e-6
        assert rows_err(X.vwl1_impulse_closed(v, entries, G, mutant), ref).min() >= 10 * 1e-6, (case, mutant)


# ---- D. CAM step attention ---------------------------------------------------------------------------------------------------------
def _cam_oracle(q, cos, sin, k, prev, s_prev, dtype):
    return CAMO.accumulate(prev, s_prev, CAMO.attention_row(CAMO.rope_last_query(q, cos[0], sin[0], dtype), k, k.shape[1]))


@pytest.mark.parametrize("case", X.CAM_CASES, ids=lambda c: "-".join(map(str, c[:4])))
def test_cam(case):
    S, G, D, dtype, Bc, Hc = case
    B, H, G = 1, 2, min(G, 2)                                     # (the heads of a kv head are copies of each other: two are enough here)
    chunk = X.cam_chunk(Bc * Hc, S)
    assert chunk % 64 == 0 and (S + chunk - 1) // chunk <= 256
    prev = X.cam_prev(B, H, S + 37)
    cos, sin = X.cam_rotary(D)
    # census
    q, k = X.cam_census(S, G, D, dtype, B, H)
    assert not q.any()                                                                             # b
    ell = X.cam_logits(q, k)
    need = NEED if S <= 10000 else 4 * TIGHT
    for s_prev in (0, S - 3):
        ref = X.cam_closed(ell, prev, s_prev)
        assert X.rel_err(ref, _cam_oracle(q, cos, sin, k, prev, s_prev, dtype)) <= 1e-12            # a
        assert np.allclose(ref[..., s_prev:], 1.0 / S, rtol=1e-15)
        mutants = [("drop", 0), ("double", S // 2), ("S", -1), ("s_prev", 1)] + ([("s_prev", -1)] if s_prev else [])
        for mutant in mutants:                                                                     # c
            moved = rows_err(X.cam_closed(ell, prev, s_prev, mutant), ref).min()
            assert moved >= need, (case, s_prev, mutant, moved)
    # impulse
    for swap in ((False, True) if case == X.CAM_SWAP else (False,)):
        cos, sin = X.cam_rotary(D, swap)
        for pos in X.groups(X.cam_positions(S, chunk), H):
            q, k = X.cam_impulse(S, G, D, dtype, [pos], swap)
            assert np.count_nonzero(k) == H and np.count_nonzero(q) == H * G                       # b
            ell = X.cam_logits(q, k, swap)
            assert ell.max() > 0
            ref = X.cam_closed(ell, prev, 0)
            assert X.rel_err(ref, _cam_oracle(q, cos, sin, k, prev, 0, dtype)) <= 1e-12             # a
            for h, t in enumerate(pos):
                for mutant in [("drop", t), ("double", t)] + ([("S", -1)] if t == S - 1 else []):  # c
                    moved = rows_err(X.cam_closed(ell, prev, 0, mutant), ref)[0, h]
                    assert moved >= NEED, (case, t, mutant, moved)
