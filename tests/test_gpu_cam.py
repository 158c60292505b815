"""CAMPress on the GPU: the three kernels against the float64 oracle (tests/_cam_oracle.py) over the smallest shapes that can go wrong, the
press against the reference's fixtures (tests/golden/cam_*.npz), the hook through the pipeline and one 128k-key step."""
import numpy as np
import pytest
import torch

import _cam_inputs as CI
import _cam_oracle as O
import _inputs
from _cam_pipeline import check_cam_pipeline
from _support import golden, merged_tol, ref_tol, torch_dtype

pytestmark = pytest.mark.gpu

DEV = "cuda"


def _score_contract(got, want):
    """1e-3 relative, plus 1e-6 of the row maximum for entries that far below it.  Returns the worst ratio."""
    tol = 1e-3 * np.abs(want) + 1e-6 * np.abs(want).max(-1, keepdims=True)
    err = np.abs(got - want)
    assert (err <= tol).all(), float((err / np.maximum(tol, 1e-300)).max())
    return float((err / np.maximum(np.abs(want), 1e-300))[np.abs(want) > 1e-3 * np.abs(want).max(-1, keepdims=True)].max(initial=0.0))


# ---- (a) attention accumulate ----------------------------------------------------------------------------------------------------------
def _step_inputs(B, H, G, S, D, dt, seed, pad_s=5, pad_d=0):
    """q_pre [B,Hq,1,D], cos / sin [1,1,D], and K as a [B,H,S,D] view of a larger cache (pad_s rows before and after, pad_d unused columns)"""
    rs = np.random.RandomState(seed)
    q = _inputs.round_to(rs.standard_normal((B, H * G, 1, D)).astype(np.float32) * 1.5, dt)
    k = _inputs.round_to(rs.standard_normal((B, H, S, D)).astype(np.float32), dt)
    ang = rs.uniform(0, 6.28, size=(1, 1, D // 2)).astype(np.float32)
    cos = _inputs.round_to(np.concatenate([np.cos(ang), np.cos(ang)], -1), dt)
    sin = _inputs.round_to(np.concatenate([np.sin(ang), np.sin(ang)], -1), dt)
    big = torch.zeros((B, H, S + 2 * pad_s, D + pad_d), dtype=torch_dtype(dt), device=DEV)
    view = big[:, :, pad_s:pad_s + S, :D]
    view.copy_(torch.from_numpy(k).to(torch_dtype(dt)))
    return q, cos, sin, k, view


ACC_CASES = [(1, 1, 6, "f32"), (2, 2, 64, "bf16"), (63, 4, 80, "f16"), (257, 8, 96, "bf16"), (4097, 16, 128, "bf16"), (257, 4, 256, "f16"),
             (4097, 2, 128, "f32"), (63, 16, 64, "f16"), (257, 1, 256, "f32"), (4097, 4, 6, "bf16"), (2, 8, 80, "f32"), (63, 2, 96, "f32"),
             (257, 16, 256, "bf16"), (4097, 8, 64, "f16"), (1, 4, 128, "bf16"),
             (257, 16, 6, "f32"), (63, 8, 6, "bf16"),          # the generic path with 8 and 16 query heads per kv head
             (257, 9, 128, "bf16"), (63, 13, 64, "f16"),       # an uneven split of the group over two workgroups: 5 + 4, 7 + 6 heads
             (257, 4, 8, "bf16"), (63, 8, 16, "f16")]          # one and two 16-byte pieces per row: 1 and 2 lanes per key


@pytest.mark.parametrize("S,G,D,dt", ACC_CASES)
def test_attn_accumulate_against_oracle(S, G, D, dt):
    """Worst relative error measured over the sweep, entries above 1e-3 of their row maximum: 1.23e-6."""
    from kvpress_amd import _native

    B, H, cap = 2, 2, S + 37
    q, cos, sin, k, kview = _step_inputs(B, H, G, S, D, dt, 100 + S + G + D)
    a = O.attention_row(O.rope_last_query(q, cos[0], sin[0], dt), k, H)
    np.testing.assert_allclose(a.sum(-1), 1.0, atol=1e-12)
    qt, ct, st = (torch.from_numpy(x).to(DEV, torch_dtype(dt)) for x in (q, cos, sin))
    rs = np.random.RandomState(7)
    prev = rs.gamma(0.5, 1.0, size=(B, H, cap)).astype(np.float32)
    worst = 0.0
    for s_prev in sorted({0, max(S - 1, 0), max(S - 3, 0)}):
        running = torch.from_numpy(prev).to(DEV)
        running[..., s_prev:] = float("nan")                                       # the stale tail counts as zero
        r0 = running.clone()
        _native.cam_attn_accumulate_(qt, ct, st, kview, running, s_prev)
        torch.cuda.synchronize()
        got = running.cpu().numpy()
        worst = max(worst, _score_contract(got[..., :S], O.accumulate(prev, s_prev, a)))
        assert torch.equal(running[..., S:].view(torch.int32), r0[..., S:].view(torch.int32))      # nothing beyond S is written
        if s_prev == 0:
            np.testing.assert_allclose(got[..., :S].sum(-1, dtype=np.float64), 1.0, atol=1e-4)
            again = torch.full_like(running, float("nan"))
            _native.cam_attn_accumulate_(qt, ct, st, kview, again, 0)
            assert torch.equal(again[..., :S], running[..., :S])                                     # bit-identical from run to run
    print(f"accumulate S={S} G={G} D={D} {dt}: worst relative error {worst:.3g}")


def test_attn_accumulate_unaligned_rows_take_the_generic_path():
    """bf16, D = 64, but a row stride of 68 elements: not 16-byte aligned"""
    from kvpress_amd import _native

    B, H, G, S, D, dt = 2, 2, 4, 257, 64, "bf16"
    q, cos, sin, k, kview = _step_inputs(B, H, G, S, D, dt, 5, pad_d=4)
    assert kview.stride(2) == 68
    running = torch.full((B, H, S), float("nan"), device=DEV)
    _native.cam_attn_accumulate_(*(torch.from_numpy(x).to(DEV, torch_dtype(dt)) for x in (q, cos, sin)), kview, running, 0)
    _score_contract(running.cpu().numpy(), O.attention_row(O.rope_last_query(q, cos[0], sin[0], dt), k, H))


def test_running_sum_after_n_steps():
    """n decoding steps without a compression: every row sums to n"""
    from kvpress_amd import _native

    B, H, G, D, dt, S0, n = 2, 2, 4, 128, "bf16", 300, 4
    q, cos, sin, k, _ = _step_inputs(B, H, G, S0 + n, D, dt, 11)
    keys = torch.from_numpy(k).to(DEV, torch_dtype(dt))
    running = torch.full((B, H, 512), float("nan"), device=DEV)
    want = np.zeros((B, H, S0 + n))
    for i in range(n):
        S = S0 + i + 1
        qi = _inputs.round_to(q * (1 + 0.1 * i), dt)
        _native.cam_attn_accumulate_(*(torch.from_numpy(x).to(DEV, torch_dtype(dt)) for x in (qi, cos, sin)), keys[:, :, :S], running, S - 1 if i else 0)
        want[..., :S] += O.attention_row(O.rope_last_query(qi, cos[0], sin[0], dt), k[:, :, :S], H)
    got = running.cpu().numpy()[..., :S0 + n]
    np.testing.assert_allclose(got.sum(-1, dtype=np.float64), float(n), atol=1e-4)
    _score_contract(got, want)


@pytest.mark.parametrize("S,G,dt", [(1, 1, "f32"), (63, 4, "bf16"), (4097, 16, "f16"), (257, 2, "f32")])
def test_attn_accumulate_row_mode(S, G, dt):
    """the eager attention row, [B,Hq,S] as the last query row of [B,Hq,Q,S] (strided)"""
    from kvpress_amd import _native

    B, H, Q = 2, 2, 3
    rs = np.random.RandomState(S + G)
    w = rs.gamma(0.3, 1.0, size=(B, H * G, Q, S))
    w = _inputs.round_to((w / w.sum(-1, keepdims=True)).astype(np.float32), dt)
    attn = torch.from_numpy(w).to(DEV, torch_dtype(dt))
    prev = rs.gamma(0.5, 1.0, size=(B, H, S + 9)).astype(np.float32)
    for s_prev in sorted({0, max(S - 1, 0), max(S - 3, 0)}):
        running = torch.from_numpy(prev).to(DEV)
        running[..., s_prev:] = float("nan")
        _native.cam_attn_accumulate_row_(attn[:, :, -1, :], running, s_prev)
        got = running.cpu().numpy()
        _score_contract(got[..., :S], O.accumulate(prev, s_prev, O.group_mean(w[:, :, -1], H)))
        assert np.isnan(got[..., S:]).all()


# ---- (b) plan and (c) merge-prune ------------------------------------------------------------------------------------------------------
def _lists(B, S, T, M, seed, layout="random"):
    """ascending kept [B,T] and candidates [B,M], disjoint"""
    rs = np.random.RandomState(seed)
    kept, cand = np.zeros((B, T), np.int32), np.zeros((B, M), np.int32)
    for b in range(B):
        if layout == "random":
            perm = rs.permutation(S)
            kept[b], cand[b] = np.sort(perm[:T]), np.sort(perm[T:T + M])
        elif layout == "after":          # every candidate after the last kept token: budget 0
            kept[b], cand[b] = np.arange(T), T + np.sort(rs.permutation(S - T)[:M])
        elif layout == "before":         # every candidate before the first kept token
            kept[b], cand[b] = S - T + np.arange(T), np.sort(rs.permutation(S - T)[:M])
        elif layout == "between":        # all candidates between two neighbouring kept tokens
            g = T // 2
            kept[b] = np.concatenate([np.arange(g), S - (T - g) + np.arange(T - g)])
            cand[b] = g + np.sort(rs.permutation(S - T)[:M])
    return kept, cand


def _running(B, H, S, seed, cap_extra=3):
    rs = np.random.RandomState(seed)
    a = rs.gamma(0.5, 1.0, size=(B, H, S + cap_extra)).astype(np.float32)
    return a, torch.from_numpy(a).to(DEV)[..., :S]        # a [B,H,S] view of a longer buffer


@pytest.mark.parametrize("S,T,M,m,layout", [(9, 8, 1, 32, "random"), (300, 200, 100, 8, "random"), (300, 17, 60, 32, "random"), (300, 200, 50, 5, "after"),
                                            (300, 200, 50, 5, "before"), (1500, 1000, 500, 32, "between"), (64, 1, 63, 1, "random")])
def test_merge_plan_against_oracle(S, T, M, m, layout):
    from kvpress_amd import _native

    B, H = 2, 3
    kept, cand = _lists(B, S, T, M, S + T + M, layout)
    a, run = _running(B, H, S, 3)
    a[:, 1] = 0.0                                           # 0 / 0 -> NaN -> 0
    a[0, 2][kept[0]] = 0.0                                  # x / 0 -> inf -> 1
    run = torch.from_numpy(a).to(DEV)[..., :S]
    kt, ct = torch.from_numpy(kept).to(DEV), torch.from_numpy(cand).to(DEV)
    c1, start, prob = _native.cam_merge_plan(kt, ct, run, S, m)
    sel = torch.from_numpy(np.sort(np.concatenate([kept, cand], -1), -1)).to(DEV)
    c2, start2, prob2 = _native.cam_merge_plan(kt, sel, run, S, m, n_cand=M)       # the candidates found from the superset
    torch.cuda.synchronize()
    o_start, o_budget, o_prob = O.plan(kept, cand, a[..., :S], m)
    np.testing.assert_array_equal(start.cpu().numpy(), o_start)
    np.testing.assert_array_equal(np.minimum(m, T - start.cpu().numpy()), o_budget)
    for c in (c1, c2):
        np.testing.assert_array_equal(c.cpu().numpy(), cand)
    assert torch.equal(start, start2) and torch.equal(prob, prob2)
    got = prob.cpu().numpy()
    _score_contract(got, o_prob)
    assert (got[:, 1] == 0).all()
    has_window = o_budget[0] > 0
    assert (got[0, 2][has_window & (a[0, 2][cand[0]] > 0)] == 1).all()


PRUNE_CASES = [  # S, T, M, m, layout, D, dt, mask
    (9, 8, 1, 32, "random", 64, "bf16", "rand"),            # S = T + 1
    (40, 30, 10, 4, "random", 6, "f32", "rand"),            # steps > S - T is the caller's clip: M = S - T
    (300, 17, 60, 32, "random", 128, "bf16", "rand"),       # m > T: every window clipped
    (300, 200, 50, 5, "after", 80, "f16", "ones"),          # budget 0: nothing merges
    (300, 200, 50, 5, "before", 96, "bf16", "ones"),
    (1500, 1000, 500, 32, "between", 128, "bf16", "ones"),  # 500 contributors per row
    (1500, 1000, 500, 32, "between", 256, "f16", "rand"),
    (300, 200, 100, 8, "random", 128, "f16", "zeros"),
    (300, 200, 100, 8, "random", 256, "f32", "ones"),
    (257, 129, 100, 3, "random", 80, "f32", "rand"),
    (300, 200, 100, 8, "random", 64, "bf16", "frac"),       # a mask that is not 0 / 1
]


@pytest.mark.parametrize("S,T,M,m,layout,D,dt,mk", PRUNE_CASES)
def test_merge_prune_against_oracle(S, T, M, m, layout, D, dt, mk):
    from kvpress_amd import _native

    B, H = 2, 2
    rs = np.random.RandomState(S + T + D)
    k = _inputs.round_to(rs.standard_normal((B, H, S, D)).astype(np.float32), dt)
    v = _inputs.round_to(rs.standard_normal((B, H, S, D)).astype(np.float32), dt)
    kept, cand = _lists(B, S, T, M, S + M, layout)
    a, run = _running(B, H, S, 4)
    mask = {"rand": (rs.uniform(size=(B, H, M)) < 0.5), "ones": np.ones((B, H, M)), "zeros": np.zeros((B, H, M)),
            "frac": rs.uniform(size=(B, H, M))}[mk].astype(np.float32)
    big_k = torch.zeros((B, H, S + 10, D), dtype=torch_dtype(dt), device=DEV)      # strided cache views
    big_v = torch.zeros_like(big_k)
    keys, values = big_k[:, :, 4:4 + S], big_v[:, :, 4:4 + S]
    keys.copy_(torch.from_numpy(k).to(torch_dtype(dt)))
    values.copy_(torch.from_numpy(v).to(torch_dtype(dt)))
    k0, v0, r0 = big_k.clone(), big_v.clone(), run.clone()
    kt, ct, mt = torch.from_numpy(kept).to(DEV), torch.from_numpy(cand).to(DEV), torch.from_numpy(mask).to(DEV)
    _, start, _ = _native.cam_merge_plan(kt, ct, run, S, m)
    ko, vo, ao = _native.cam_merge_prune(keys, values, run, kt, ct, start, mt, m)
    ko2, vo2, ao2 = _native.cam_merge_prune(keys, values, run, kt, ct, start, mt, m)
    torch.cuda.synchronize()
    assert torch.equal(big_k, k0) and torch.equal(big_v, v0) and torch.equal(run, r0)                    # the inputs are not written
    assert torch.equal(ko, ko2) and torch.equal(ao, ao2) and torch.equal(vo.view(torch.uint8), vo2.view(torch.uint8))
    o = O.merge_prune(k, v, a[..., :S], kept, cand, mask, m, dt)
    np.testing.assert_array_equal(ko.float().cpu().numpy(), o["k"])
    np.testing.assert_array_equal(ao.cpu().numpy(), o["a"])
    got = vo.float().cpu().numpy()
    np.testing.assert_array_equal(got[~o["merged"]], o["v"][~o["merged"]])                                # bit-exact without contributors
    ref = o["v"][o["merged"]]
    err = np.abs(got[o["merged"]] - ref)
    assert (err <= merged_tol(ref, dt)).all(), float(err.max(initial=0.0))
    if layout == "after" or mk == "zeros":
        assert not o["merged"].any()
    if layout == "between":
        assert o["merged"].any(-1).all() and (o["budget"] == min(m, T - T // 2)).all()


# ---- against the reference ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(CI.CASES))
def test_compress_against_reference_fixtures(name):
    """the whole compress() on the float32 module with the reference's mask replayed: its kept set (K', A') exactly, its V' to ref_tol"""
    import kvpress_amd as P

    s, g = CI.make_case(name), golden(name)
    module, hidden, kw = CI.module_and_step(s, torch.float32, DEV)
    keys, values, running = (torch.from_numpy(s[n]).to(DEV) for n in ("keys", "values", "running"))
    k0, v0 = keys.clone(), values.clone()
    press = P.CAMPress(base_press=P.KnormPress(), compression_interval=s["steps"], target_size=s["T"], merge_budget=s["m"])
    press.layer_step_counts[0] = s["steps"]
    press._running_attn_sum[0] = running
    probs = []

    def replay(prob):
        probs.append(prob)
        return torch.from_numpy(g["o32_mask"]).to(DEV)
    press._draw_merge_mask = replay
    with torch.no_grad():
        k2, v2 = press.compress(module, hidden, keys, values, running, kw)
    torch.cuda.synchronize()
    assert torch.equal(keys, k0) and torch.equal(values, v0)
    np.testing.assert_array_equal(k2.cpu().numpy(), g["o32_k"])
    np.testing.assert_array_equal(press._running_attn_sum[0].cpu().numpy(), g["o32_a"])
    assert (np.abs(probs[0].cpu().numpy() - g["o32_prob"]) <= 1e-3 * g["o32_prob"] + 1e-6).all()
    err = np.abs(v2.cpu().numpy() - g["o32_v"])
    assert (err <= ref_tol(g["o32_v"], "f32")).all(), float(err.max())


@pytest.mark.parametrize("name", list(CI.CASES))
def test_kernels_against_native_dtype_fixtures(name):
    """the reference's run in the model dtype, on its own kept set, candidates and mask: K', A' and the rows nothing is merged into are its
    bits (its merged rows round every product and every scatter_add_ step to the dtype: DESIGN.md section 2, deviation 2)"""
    from kvpress_amd import _native

    s, g = CI.make_case(name), golden(name)
    dt = s["dtype"]
    keys, values = (torch.from_numpy(s[n]).to(DEV, torch_dtype(dt)) for n in ("keys", "values"))
    running = torch.from_numpy(s["running"]).to(DEV)
    kt, ct, mt = (torch.from_numpy(g[f"nat_{n}"]).to(DEV) for n in ("kept", "cand", "mask"))
    _, start, _ = _native.cam_merge_plan(kt, ct, running, s["S"], s["m"])
    ko, vo, ao = _native.cam_merge_prune(keys, values, running, kt, ct, start, mt, s["m"])
    torch.cuda.synchronize()
    np.testing.assert_array_equal(ko.float().cpu().numpy(), g["nat_k"])
    np.testing.assert_array_equal(ao.cpu().numpy(), g["nat_a"])
    o = O.merge_prune(s["keys"], s["values"], s["running"], g["nat_kept"], g["nat_cand"], g["nat_mask"], s["m"], dt)
    np.testing.assert_array_equal(vo.float().cpu().numpy()[~o["merged"]], g["nat_v"][~o["merged"]])


@pytest.mark.parametrize("name", list(CI.CASES))
def test_step_attention_against_reference_fixtures(name):
    from kvpress_amd import _native
    from kvpress_amd.utils import get_prerope_query_states

    s, g = CI.make_case(name), golden(name)
    module, hidden, kw = CI.module_and_step(s, torch.float32, DEV)
    keys = torch.from_numpy(s["keys"]).to(DEV)
    cos, sin = kw["position_embeddings"]
    running = torch.full((s["B"], s["H"], s["S"]), float("nan"), device=DEV)
    with torch.no_grad():
        _native.cam_attn_accumulate_(get_prerope_query_states(module, hidden), cos, sin, keys, running, 0)
    _score_contract(running.cpu().numpy(), g["o32_attn"].astype(np.float64))


# ---- the hook ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype,eager", [(torch.float32, False), (torch.bfloat16, False), (torch.float32, True)])
def test_cam_pipeline_gpu(dtype, eager):
    check_cam_pipeline("cuda:0", dtype, eager)


def test_llama8b_128k_step():
    """one decoding step over 128k keys (H_kv 8, G 4, D 128, bf16; 1024-key chunks, many sweeps per workgroup) into a stale (NaN) running
    sum: no memory beyond the workspace, and at 512 sampled keys per kv head -- the largest entries of the row among them -- the
    attention itself matches a chunked float64 softmax to the score contract, its tolerance taken from the attention row's own maximum"""
    from kvpress_amd import _native

    B, H, G, S, D = 1, 8, 4, 131072, 128
    gen = torch.Generator(device=DEV).manual_seed(0)
    keys = torch.randn((B, H, S, D), device=DEV, generator=gen).to(torch.bfloat16)
    q = (2.0 * torch.randn((B, H * G, 1, D), device=DEV, generator=gen)).to(torch.bfloat16)
    ang = torch.rand((1, 1, D // 2), device=DEV, generator=gen) * 6.28
    cos, sin = (torch.cat([f(ang), f(ang)], -1).to(torch.bfloat16) for f in (torch.cos, torch.sin))
    running = torch.full((B, H, S + 512), float("nan"), device=DEV)
    ws_bytes = _native.lib().kvp_cam_attn_workspace_bytes(B, H * G, H, S)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    _native.cam_attn_accumulate_(q, cos, sin, keys, running, 0)
    torch.cuda.synchronize()
    extra = torch.cuda.max_memory_allocated() - base
    assert extra <= ws_bytes + (2 << 20), (extra, ws_bytes)
    half = D // 2
    q_rot = (q * cos[:, None]) + (torch.cat((-q[..., half:], q[..., :half]), -1) * sin[:, None])       # torch's own bf16 ops
    rs = np.random.RandomState(1)
    for h in range(H):
        logits = torch.empty((G, S), dtype=torch.float64, device=DEV)
        for c0 in range(0, S, 16384):
            logits[:, c0:c0 + 16384] = q_rot[0, h * G:(h + 1) * G, 0].double() @ keys[0, h, c0:c0 + 16384].double().T / D ** 0.5
        a = torch.softmax(logits, -1).mean(0)
        pos = torch.cat([torch.from_numpy(rs.choice(S, 448, replace=False)).to(DEV), a.topk(63).indices, torch.tensor([S - 1], device=DEV)])
        got, want = running[0, h, pos].double(), a[pos]
        err = (got - want).abs()
        assert (err <= 1e-3 * want + 1e-6 * a.max()).all(), float((err / (1e-3 * want + 1e-6 * a.max())).max())
        torch.testing.assert_close(running[0, h, :S].double().sum(), torch.ones((), dtype=torch.float64, device=DEV), atol=1e-4, rtol=0)
    assert torch.isnan(running[..., S:]).all()
