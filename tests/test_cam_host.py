"""CAMPress without a GPU: the float64 oracle (tests/_cam_oracle.py) against the reference's fixtures (tests/golden/cam_*.npz), the
press's host logic over oracle-backed stand-ins of its three library calls, the package surface and the C ABI's argument checks."""
import ctypes

import numpy as np
import pytest
import torch

import _cam_inputs as CI
import _cam_oracle as O
import _inputs
from _cam_pipeline import check_cam_pipeline
from _support import cache_sizes, dtype_name, golden, ref_tol, tiny_pipeline


# ---- the oracle reproduces the reference ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(CI.CASES))
def test_oracle_reproduces_the_reference_compress(name):
    """Worst oracle-vs-reference difference of the float32 run over the three fixtures: prob 5.2e-8, V' 4.8e-7 absolute."""
    s, g = CI.make_case(name), golden(name)
    mean = -np.linalg.norm(s["keys"].astype(np.float64), axis=-1).mean(1)          # KnormPress, head mean
    M = min(s["steps"], s["S"] - s["T"])
    kept, cand = O.rank(mean, s["T"], M)
    np.testing.assert_array_equal(kept, g["o32_kept"])
    np.testing.assert_array_equal(cand, g["o32_cand"])
    start, budget, prob = O.plan(kept, cand, s["running"], s["m"])
    err = np.abs(prob - g["o32_prob"]).max(initial=0.0)
    print(f"{name}: prob max abs err {err:.3g}")
    assert err <= 2e-5
    for run, dt in (("o32", "f32"), ("nat", s["dtype"])):
        o = O.merge_prune(s["keys"], s["values"], s["running"], g[f"{run}_kept"], g[f"{run}_cand"], g[f"{run}_mask"], s["m"], dt)
        np.testing.assert_array_equal(o["k"], g[f"{run}_k"])
        np.testing.assert_array_equal(o["a"], g[f"{run}_a"])
        np.testing.assert_array_equal(o["v"][~o["merged"]], g[f"{run}_v"][~o["merged"]])
        if run == "o32":
            verr = np.abs(o["v"] - g["o32_v"])
            print(f"{name}: V' max abs err {verr.max():.3g}")
            assert (verr <= ref_tol(g["o32_v"], dt)).all(), float(verr.max())
    if s["zero_head"] is not None:
        assert (prob[:, s["zero_head"]] == 0).all()                                  # 0 / 0 -> NaN -> 0


@pytest.mark.parametrize("name", list(CI.CASES))
def test_oracle_reproduces_the_reference_step_attention(name):
    """Worst over the fixtures: 1.6e-8 absolute."""
    s, g = CI.make_case(name), golden(name)
    module, hidden, kw = CI.module_and_step(s, torch.float32)
    from kvpress_amd.utils import get_prerope_query_states

    with torch.no_grad():
        q_pre = get_prerope_query_states(module, hidden)
    cos, sin = kw["position_embeddings"]
    a = O.attention_row(O.rope_last_query(q_pre.numpy(), cos.numpy(), sin.numpy(), "f32"), s["keys"], s["H"])
    err = np.abs(a - g["o32_attn"]).max()
    print(f"{name}: attention max abs err {err:.3g}")
    assert err <= 2e-5
    np.testing.assert_allclose(a.sum(-1), 1.0, atol=1e-12)


# ---- the press's host logic ------------------------------------------------------------------------------------------------------------
@pytest.fixture
def fake_cam(fake_native, monkeypatch):
    """fake_native plus oracle-backed stand-ins for the three CAM entry points"""
    calls = {"q": 0, "row": 0, "plan": 0, "prune": 0}

    def _store(running, s_prev, a):
        S = a.shape[-1]
        running[..., :S] = torch.from_numpy(O.accumulate(running.numpy(), s_prev, a)).float()
        return running

    def cam_attn_accumulate_(q_pre, cos, sin, keys, running, s_prev):
        calls["q"] += 1
        assert q_pre.shape[2] == 1 and cos.shape[-2] == 1 and running.shape[-1] >= keys.shape[2]
        q = O.rope_last_query(q_pre.float().numpy(), cos.float().numpy(), sin.float().numpy(), dtype_name(keys.dtype))
        return _store(running, s_prev, O.attention_row(q, keys.float().numpy(), keys.shape[1]))

    def cam_attn_accumulate_row_(attn_row, running, s_prev):
        calls["row"] += 1
        return _store(running, s_prev, O.group_mean(attn_row.float().numpy(), running.shape[1]))

    def cam_merge_plan(kept, sel, running, S, merge_budget, n_cand=None):
        calls["plan"] += 1
        k, sl = kept.numpy(), sel.numpy()
        M = sl.shape[1] if n_cand is None else n_cand
        cand = sl if sl.shape[1] == M else np.stack([np.setdiff1d(sl[b], k[b]) for b in range(k.shape[0])]).reshape(k.shape[0], M)
        start, _, prob = O.plan(k, cand, running.numpy()[..., :S], merge_budget)
        return torch.from_numpy(cand.astype(np.int32)), torch.from_numpy(start.astype(np.int32)), torch.from_numpy(prob.astype(np.float32))

    def cam_merge_prune(keys, values, running, kept, cand, start, mask, merge_budget):
        calls["prune"] += 1
        o = O.merge_prune(keys.float().numpy(), values.float().numpy(), running.numpy(), kept.numpy(), cand.numpy(), mask.numpy(), merge_budget,
                          dtype_name(keys.dtype))
        np.testing.assert_array_equal(o["start"], start.numpy())
        return (torch.from_numpy(o["k"]).to(keys.dtype), torch.from_numpy(o["v"]).to(keys.dtype), torch.from_numpy(o["a"].astype(np.float32)))

    for fn in (cam_attn_accumulate_, cam_attn_accumulate_row_, cam_merge_plan, cam_merge_prune):
        monkeypatch.setattr(fake_native, fn.__name__, fn)
    fake_native.cam_calls = calls
    return fake_native


def test_cam_pipeline_cpu(fake_cam):
    check_cam_pipeline("cpu", None)
    assert fake_cam.cam_calls["q"] and fake_cam.cam_calls["plan"] == fake_cam.cam_calls["prune"] > 0


def test_cam_pipeline_eager_row_cpu(fake_cam):
    """with eager attention the layer returns its weights: their last row is accumulated, no query is projected"""
    from transformers import DynamicCache

    import kvpress_amd as P

    pipe = tiny_pipeline("cpu", None, eager=True)
    press = P.CAMPress(base_press=P.KnormPress(), compression_interval=4, target_size=32)
    cache = DynamicCache()
    pipe(_inputs.tiny_context(60), question="w1 w2", press=press, cache=cache, max_new_tokens=10)
    assert all(32 <= n <= 35 for n in cache_sizes(cache))
    assert fake_cam.cam_calls["row"] > 0 and fake_cam.cam_calls["q"] == 0


@pytest.mark.parametrize("name", list(CI.CASES))
def test_compress_replays_the_reference(fake_cam, name):
    """compress() called the way oracle/gen_golden_cam.py calls the reference's, its mask replayed: the reference's kept set, K', V', A'"""
    import kvpress_amd as P

    s, g = CI.make_case(name), golden(name)
    module, hidden, kw = CI.module_and_step(s, torch.float32)
    keys, values, running = (torch.from_numpy(s[n]) for n in ("keys", "values", "running"))
    k0, v0, r0 = keys.clone(), values.clone(), running.clone()
    press = P.CAMPress(base_press=P.KnormPress(), compression_interval=s["steps"], target_size=s["T"], merge_budget=s["m"])
    press.layer_step_counts[0] = s["steps"]
    press._running_attn_sum[0] = running
    seen = []

    def replay(prob):
        seen.append(prob)
        return torch.from_numpy(g["o32_mask"])
    press._draw_merge_mask = replay
    with torch.no_grad():
        k2, v2 = press.compress(module, hidden, keys, values, running, kw)
    assert torch.equal(keys, k0) and torch.equal(values, v0) and torch.equal(running, r0)        # deviation 4: nothing is written
    np.testing.assert_allclose(seen[0].numpy(), g["o32_prob"], atol=2e-5)
    np.testing.assert_array_equal(k2.numpy(), g["o32_k"])
    np.testing.assert_array_equal(press._running_attn_sum[0].numpy(), g["o32_a"])
    err = np.abs(v2.numpy() - g["o32_v"])
    assert (err <= ref_tol(g["o32_v"], "f32")).all(), float(err.max())
    # at or below the target: the inputs come back
    press.target_size = s["S"]
    assert press.compress(module, hidden, keys, values, running, kw) == (keys, values)


# ---- surface ---------------------------------------------------------------------------------------------------------------------------
def test_import_surface():
    import kvpress_amd as P

    assert "CAMPress" in P.__all__ and P.CAMPress.__name__ == "CAMPress" and "CAMPress" not in P._NOT_BUILT
    assert issubclass(P.CAMPress, P.DecodingPress)
    press = P.CAMPress(base_press=P.KnormPress())
    assert (press.compression_interval, press.target_size, press.hidden_states_buffer_size, press.merge_budget) == (512, 2048, 256, 32)
    for bad in (0, -3):
        with pytest.raises(AssertionError):
            P.CAMPress(base_press=P.KnormPress(), merge_budget=bad)
    with pytest.raises(AssertionError):
        P.CAMPress(base_press=P.ChunkPress(P.KnormPress()))


def test_chain_switches_the_prefill_press_to_score_order():
    import kvpress_amd as P
    from kvpress_amd.presses.scorer_press import resolve_chain_kept_order

    first = P.KnormPress(0.5)
    assert resolve_chain_kept_order(first, [P.CAMPress(base_press=P.KnormPress())], "test") == "switched"
    assert first.kept_order == "score"
    assert resolve_chain_kept_order(P.KnormPress(0.5), [P.DecodingPress(base_press=P.KnormPress())], "test") is None


def test_c_abi_rejects_bad_arguments():
    """before any HIP call, in the style of tests/test_capi_symbols.py::test_version_and_errors"""
    from kvpress_amd import _native, build

    build.build()
    lib = _native.lib()
    # plan(kept, sel, n_sel, attn, a_sb, a_sh, B, H, S, T, M, merge_budget, cand, start, prob, stream)
    assert lib.kvp_cam_merge_plan(None, None, 2, None, 0, 0, 1, 2, 10, 11, 2, 4, None, None, None, None) == -1     # T > S
    assert b"bad shape" in lib.kvp_last_error()
    assert lib.kvp_cam_merge_plan(None, None, 4, None, 0, 0, 1, 2, 10, 8, 4, 4, None, None, None, None) == -1      # T + M > S
    assert b"bad shape" in lib.kvp_last_error()
    for budget in (0, -1):
        assert lib.kvp_cam_merge_plan(None, None, 2, None, 0, 0, 1, 2, 10, 8, 2, budget, None, None, None, None) == -1
        assert b"merge_budget" in lib.kvp_last_error()
    assert lib.kvp_cam_merge_plan(None, None, 3, None, 0, 0, 1, 2, 10, 8, 2, 4, None, None, None, None) == -1      # neither M nor T + M
    assert b"n_sel" in lib.kvp_last_error()
    assert lib.kvp_cam_merge_plan(None, None, 2, None, 0, 0, 1, 2, 10, 8, 2, 4, None, None, None, None) == -1
    assert b"null pointer" in lib.kvp_last_error()
    assert lib.kvp_cam_merge_plan(None, None, 0, None, 0, 0, 1, 2, 10, 8, 0, 4, None, None, None, None) == 0       # no candidate: nothing to do
    # prune(k.., v.., attn.., kept, cand, start, mask, dtype, B, H, S, T, M, D, merge_budget, k_out, v_out, attn_out, stream)
    prune = lambda dtype, S, T, M, D, budget: lib.kvp_cam_merge_prune(None, 0, 0, 0, None, 0, 0, 0, None, 0, 0, None, None, None, None, dtype,
                                                                       1, 2, S, T, M, D, budget, None, None, None, None)
    assert prune(7, 10, 8, 2, 64, 4) == -1 and b"dtype" in lib.kvp_last_error()
    assert prune(2, 10, 11, 0, 64, 4) == -1 and b"bad shape" in lib.kvp_last_error()
    assert prune(2, 10, 8, 2, 64, 0) == -1 and b"merge_budget" in lib.kvp_last_error()
    assert prune(2, 10, 8, 2, 257, 4) == -1 and b"head size" in lib.kvp_last_error()
    assert prune(2, 10, 8, 2, 64, 4) == -1 and b"null pointer" in lib.kvp_last_error()
    # accumulate(q.., cos, sin, cs.., k.., dtype, B, Hq, Hkv, S, D, running, r_sb, r_sh, cap, S_prev, ws, ws_bytes, stream)
    acc = lambda dtype, Hq, Hkv, S, D, cap, prev: lib.kvp_cam_attn_accumulate(None, 0, 0, 0, None, None, 0, 0, None, 0, 0, 0, dtype, 1, Hq, Hkv, S,
                                                                               D, None, 0, cap, cap, prev, None, 0, None)
    assert acc(5, 4, 2, 10, 64, 16, 9) == -1 and b"dtype" in lib.kvp_last_error()
    assert acc(2, 5, 2, 10, 64, 16, 9) == -1 and b"bad shape" in lib.kvp_last_error()
    assert acc(2, 4, 2, 10, 7, 16, 9) == -1 and b"head size" in lib.kvp_last_error()
    assert acc(2, 34, 2, 10, 64, 16, 9) == -1 and b"16 query heads" in lib.kvp_last_error()
    assert acc(2, 4, 2, 10, 64, 9, 9) == -1 and b"running sum" in lib.kvp_last_error()        # cap < S
    assert acc(2, 4, 2, 10, 64, 16, 11) == -1 and b"running sum" in lib.kvp_last_error()      # S_prev > S
    assert acc(2, 4, 2, 10, 64, 16, 9) == -1 and b"null pointer" in lib.kvp_last_error()
    assert lib.kvp_cam_attn_accumulate_row(None, 0, 0, 9, 1, 4, 2, 10, None, 0, 16, 16, 9, None) == -1 and b"dtype" in lib.kvp_last_error()
    assert lib.kvp_cam_attn_accumulate_row(None, 0, 0, 2, 1, 4, 2, 10, None, 0, 16, 16, 9, None) == -1 and b"null pointer" in lib.kvp_last_error()
    # Llama-3.1-8B at 128k keys: the logits of one step, 4 bytes per query head and key, and little else
    ws = lib.kvp_cam_attn_workspace_bytes(1, 32, 8, 131072)
    assert 32 * 131072 * 4 <= ws < 32 * 131072 * 4 + (1 << 20)
    assert lib.kvp_cam_attn_workspace_bytes(1, 5, 2, 10) == 0
