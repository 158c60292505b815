"""MergingPress on the GPU: kvp_merge_values against the float64 oracle over a shape sweep, the press against the reference's fixtures
(tests/golden/mrg_*.npz), the tie and NaN-quantile edge cases, determinism, no side effects and the 128k Llama-3.1-8B geometry."""
import numpy as np
import pytest
import torch

import _inputs
import _merging_inputs as MI
import _merging_oracle as O
from _support import golden, kept_positions, merged_tol, ref_tol, torch_dtype

pytestmark = pytest.mark.gpu

DEV = "cuda"


def _run_kernel(keys, values, kept, thr, frac):
    """K' / V' gathered by the library, then merged; returns (K', V', target, max_sim)"""
    from kvpress_amd import _native

    B, H, S, D = keys.shape
    n = kept.shape[-1]
    k_out, v_out = _native.gather_kv(keys, values, kept)
    tg = torch.full((B, H, S - n), -7, dtype=torch.int32, device=keys.device)
    ms = torch.full((B, H, S - n), float("nan"), dtype=torch.float32, device=keys.device)
    _native.merge_values_(keys, values, kept, k_out, v_out, thr, frac, target=tg, max_sim=ms)
    torch.cuda.synchronize()
    return k_out, v_out, tg, ms


def _check_against_oracle(keys_np, values_np, kept_np, thr, frac, dt, k_out, v_out, tg, ms):
    B, H, S, D = keys_np.shape
    n = kept_np.shape[-1]
    kept64 = kept_np.astype(np.int64)
    np.testing.assert_array_equal(k_out.float().cpu().numpy(), np.take_along_axis(keys_np, kept64[..., None].repeat(D, -1), 2))
    tg, ms = tg.cpu().numpy(), ms.cpu().numpy()
    ev = O.evicted_positions(kept_np, S)
    # targets, tie-tolerant: the chosen survivor is a maximum to 1e-5, and the oracle's own where the runner-up is further away
    for b in range(B):
        for h in range(H):
            sim = O.similarities(keys_np, kept_np, ev, b, h)
            best = sim.max(-1)
            chosen = sim[np.arange(S - n), tg[b, h]]
            assert (chosen >= best - 1e-5).all(), (b, h, float((best - chosen).max()))
            np.testing.assert_allclose(ms[b, h], best, atol=1e-5)
            part = np.partition(sim, -2, axis=-1)[:, -2] if n > 1 else np.full(S - n, -np.inf)
            clear = best - part > 1e-5
            np.testing.assert_array_equal(tg[b, h][clear], sim.argmax(-1)[clear])
    o = O.merge(keys_np, values_np, kept_np, thr, frac, dt, target=tg, max_sim=ms)
    got = v_out.float().cpu().numpy()
    base = np.take_along_axis(values_np, kept64[..., None].repeat(D, -1), 2)
    untouched = ~o["merged"]
    np.testing.assert_array_equal(got[untouched], base[untouched])             # rows without contributions are bit-exact
    ref = o["v"][o["merged"]]
    err = np.abs(got[o["merged"]] - ref)
    assert (err <= merged_tol(ref, dt)).all(), float(err.max())
    return o


def _rand_case(B, H, S, D, dt, ratio, seed):
    rs = np.random.RandomState(seed)
    k = rs.standard_normal((B, H, S, D)).astype(np.float32)
    # a shared direction per head so that similarities spread over [0, 1] and the threshold / fraction gates bite
    k = _inputs.round_to(k + 1.5 * rs.standard_normal((1, H, 1, D)).astype(np.float32), dt)
    v = _inputs.round_to(rs.standard_normal((B, H, S, D)).astype(np.float32), dt)
    n = int(S * (1 - ratio))
    sc = rs.standard_normal((B, H, S)).astype(np.float32)
    kept = np.ascontiguousarray(np.argsort(-sc, axis=-1, kind="stable")[..., :n]).astype(np.int32)
    return k, v, kept


SWEEP = []
for i, (B, H, S, D, dt) in enumerate([(1, 1, 1, 64, "bf16"), (1, 8, 2, 128, "bf16"), (2, 1, 63, 96, "f16"), (1, 8, 257, 128, "bf16"),
                                      (2, 8, 1000, 64, "f16"), (1, 8, 4097, 128, "bf16"), (2, 1, 257, 256, "bf16"), (1, 8, 1000, 80, "bf16"),
                                      (2, 8, 257, 128, "f32"), (1, 1, 4097, 256, "f16"), (1, 8, 1000, 256, "f32"), (2, 8, 63, 80, "f32")]):
    for j, (ratio, thr, frac) in enumerate([(0.1, 0.0, 1.0), (0.5, 0.3, 0.75), (0.9, 0.0, 0.3)]):
        SWEEP.append((B, H, S, D, dt, ratio, thr, frac, 1000 + 10 * i + j))


@pytest.mark.parametrize("B,H,S,D,dt,ratio,thr,frac,seed", SWEEP)
def test_kernel_against_oracle(B, H, S, D, dt, ratio, thr, frac, seed):
    k, v, kept = _rand_case(B, H, S, D, dt, ratio, seed)
    n = kept.shape[-1]
    keys = torch.from_numpy(k).to(DEV, torch_dtype(dt))
    values = torch.from_numpy(v).to(DEV, torch_dtype(dt))
    kept_t = torch.from_numpy(kept).to(DEV)
    k0, v0 = keys.clone(), values.clone()
    k_out, v_out, tg, ms = _run_kernel(keys, values, kept_t, thr, frac)
    assert torch.equal(keys, k0) and torch.equal(values, v0)
    if n == 0 or n == S:
        np.testing.assert_array_equal(v_out.float().cpu().numpy(), np.take_along_axis(v, kept.astype(np.int64)[..., None].repeat(D, -1), 2))
        return
    _check_against_oracle(k, v, kept, thr, frac, dt, k_out, v_out, tg, ms)


def test_strided_cache_views():
    """keys / values as views of a larger cache (the head stride is not S * D) give the same result"""
    k, v, kept = _rand_case(1, 4, 700, 128, "bf16", 0.5, 77)
    big_k = torch.zeros((1, 4, 900, 128), dtype=torch.bfloat16, device=DEV)
    big_v = torch.zeros_like(big_k)
    big_k[:, :, 100:800] = torch.from_numpy(k).to(DEV, torch.bfloat16)
    big_v[:, :, 100:800] = torch.from_numpy(v).to(DEV, torch.bfloat16)
    out = _run_kernel(big_k[:, :, 100:800], big_v[:, :, 100:800], torch.from_numpy(kept).to(DEV), 0.0, 1.0)
    _check_against_oracle(k, v, kept, 0.0, 1.0, "bf16", *out)


@pytest.mark.parametrize("run", ["o32", "nat"])
@pytest.mark.parametrize("name", list(MI.CASES))
def test_merge_against_reference_fixtures(name, run):
    """the kernel on the reference's own kept indices (its descending-score order) gives the reference's targets and V'"""
    s, g = MI.make_case(name), golden(name)
    tdt = torch.float32 if run == "o32" else torch_dtype(s["dtype"])
    dt = "f32" if run == "o32" else s["dtype"]
    kept = g[f"{run}_kept"]
    keys = torch.from_numpy(s["keys"]).to(DEV, tdt)
    values = torch.from_numpy(s["values"]).to(DEV, tdt)
    _, v_out, tg, ms = _run_kernel(keys, values, torch.from_numpy(kept).to(DEV), s["thr"], s["frac"])
    if 0 < kept.shape[-1] < s["S"]:
        ev = O.evicted_positions(kept, s["S"])
        for b in range(s["B"]):
            for h in range(s["H"]):
                sim = O.similarities(s["keys"], kept, ev, b, h)
                mine = sim[np.arange(ev.shape[-1]), tg.cpu().numpy()[b, h]]
                theirs = sim[np.arange(ev.shape[-1]), g[f"{run}_target"][b, h]]
                assert (np.abs(mine - theirs) <= 1e-5).all()
        np.testing.assert_allclose(ms.cpu().numpy(), g[f"{run}_max_sim"], atol=1e-5)
    ref_v = g[f"{run}_v"]
    err = np.abs(v_out.float().cpu().numpy() - ref_v)
    assert (err <= ref_tol(ref_v, dt)).all(), float(err.max(initial=0.0))


@pytest.mark.parametrize("order", ["position", "score"])
@pytest.mark.parametrize("name", [n for n in MI.CASES if MI.CASES[n]["data"] != "dup"])   # identical keys: Knorm ties between positions
def test_press_against_reference_fixtures(name, order):
    """the whole press in float32 (scores, hence kept sets, as the reference's; in a 16-bit model the reference's scores are rounded
    to the dtype and tie); "score" order reproduces the reference's tensor order"""
    run = "o32"
    import kvpress_amd as P

    s, g = MI.make_case(name), golden(name)
    tdt = torch.float32 if run == "o32" else torch_dtype(s["dtype"])
    dt = "f32" if run == "o32" else s["dtype"]
    module, hidden, kw = MI.module_and_kwargs(s, tdt, DEV)
    keys = torch.from_numpy(s["keys"]).to(DEV, tdt)
    values = torch.from_numpy(s["values"]).to(DEV, tdt)
    k0, v0 = keys.clone(), values.clone()
    inner = MI.inner_press(s, P)
    inner.kept_order = order
    press = P.MergingPress(inner, similarity_threshold=s["thr"], merge_fraction=s["frac"])
    with torch.no_grad():
        k2, v2 = press.compress(module, hidden, keys, values, None, kw)
    torch.cuda.synchronize()
    assert torch.equal(keys, k0) and torch.equal(values, v0)
    kept, ref_v = g[f"{run}_kept"], g[f"{run}_v"]
    D = s["D"]
    got_k, got = k2.float().cpu().numpy(), v2.float().cpu().numpy()
    if order == "position" or s["press"] == "snapkv":
        # SnapKV's window tokens all score max + 1: their order among themselves is torch.topk's choice, so compare by position
        perm = np.argsort(kept, axis=-1, kind="stable")
        kept = np.take_along_axis(kept, perm, -1)
        ref_v = np.take_along_axis(ref_v, perm[..., None].repeat(D, -1), 2)
        if order == "score":
            mine = np.argsort(kept_positions(got_k, s["keys"]), axis=-1, kind="stable")
            got_k = np.take_along_axis(got_k, mine[..., None].repeat(D, -1), 2)
            got = np.take_along_axis(got, mine[..., None].repeat(D, -1), 2)
    assert got.shape == ref_v.shape
    np.testing.assert_array_equal(got_k, np.take_along_axis(s["keys"], kept.astype(np.int64)[..., None].repeat(D, -1), 2))
    err = np.abs(got - ref_v)
    assert (err <= ref_tol(ref_v, dt)).all(), float(err.max(initial=0.0))


def test_duplicate_keys_tie_to_the_lowest_kept_index():
    s, g = MI.make_case("mrg_knorm_dup_s96_d64"), golden("mrg_knorm_dup_s96_d64")
    keys = torch.from_numpy(s["keys"]).to(DEV, torch.bfloat16)
    values = torch.from_numpy(s["values"]).to(DEV, torch.bfloat16)
    for kept in (g["o32_kept"], np.ascontiguousarray(np.sort(g["o32_kept"], axis=-1))):
        _, v_out, tg, ms = _run_kernel(keys, values, torch.from_numpy(kept).to(DEV), 0.0, 1.0)
        ev = O.evicted_positions(kept, s["S"])
        for h in range(s["H"]):
            sim = O.similarities(s["keys"], kept, ev, 0, h)
            np.testing.assert_array_equal(tg.cpu().numpy()[0, h], sim.argmax(-1))
    np.testing.assert_array_equal(_run_kernel(keys, values, torch.from_numpy(g["nat_kept"]).to(DEV), 0.0, 1.0)[2].cpu().numpy(),
                                  g["nat_target"])


def test_nan_quantile_row_merges_nothing():
    s, g = MI.make_case("mrg_knorm_nanq_s200_d128"), golden("mrg_knorm_nanq_s200_d128")
    kept = g["nat_kept"]
    keys = torch.from_numpy(s["keys"]).to(DEV, torch.bfloat16)
    values = torch.from_numpy(s["values"]).to(DEV, torch.bfloat16)
    _, v_out, tg, ms = _run_kernel(keys, values, torch.from_numpy(kept).to(DEV), s["thr"], s["frac"])
    base = np.take_along_axis(s["values"], kept.astype(np.int64)[..., None].repeat(s["D"], -1), 2)
    got = v_out.float().cpu().numpy()
    np.testing.assert_array_equal(got[0, 1], base[0, 1])      # head 1: NaN quantile, nothing merges
    assert not np.array_equal(got[0, 0], base[0, 0])          # head 0 merges


def test_deterministic():
    k, v, kept = _rand_case(2, 8, 4097, 128, "bf16", 0.5, 5)
    keys = torch.from_numpy(k).to(DEV, torch.bfloat16)
    values = torch.from_numpy(v).to(DEV, torch.bfloat16)
    kept_t = torch.from_numpy(kept).to(DEV)
    a = _run_kernel(keys, values, kept_t, 0.0, 0.75)
    b = _run_kernel(keys, values, kept_t, 0.0, 0.75)
    for x, y in zip(a, b):
        assert torch.equal(x.contiguous().view(torch.uint8), y.contiguous().view(torch.uint8))


def test_llama8b_128k_geometry():
    """H_kv 8, D 128, bf16, 128k tokens, ratio 0.5: completes, at most 64 MiB beyond the outputs, 256 sampled rows match float64"""
    from kvpress_amd import KnormPress, MergingPress, _native

    B, H, S, D = 1, 8, 131072, 128
    g = torch.Generator(device=DEV).manual_seed(0)
    keys = (torch.randn((B, H, S, D), device=DEV, generator=g) + 1.5 * torch.randn((1, H, 1, D), device=DEV, generator=g)).to(torch.bfloat16)
    values = torch.randn((B, H, S, D), device=DEV, generator=g).to(torch.bfloat16)
    press = MergingPress(KnormPress(0.5))
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    k2, v2 = press.compress(None, None, keys, values, None, {})
    torch.cuda.synchronize()
    extra = torch.cuda.max_memory_allocated() - base - (k2.numel() + v2.numel()) * 2
    assert extra < 64 << 20, extra / 2 ** 20
    n = S // 2
    kept = _native.topk_select(_native.rownorm_score(keys, -1.0), n)
    tg = torch.empty((B, H, S - n), dtype=torch.int32, device=DEV)
    ms = torch.empty((B, H, S - n), dtype=torch.float32, device=DEV)
    k_out, v_out = _native.gather_kv(keys, values, kept)
    _native.merge_values_(keys, values, kept, k_out, v_out, 0.0, 1.0, target=tg, max_sim=ms)
    torch.cuda.synchronize()
    assert torch.equal(v_out, v2)
    # 256 sampled evicted rows against a chunked float64 check over the kept keys K'
    mask = torch.ones((B, H, S), dtype=torch.bool, device=DEV)
    mask.scatter_(2, kept.long(), False)
    ev = mask.nonzero()[:, 2].view(B, H, S - n)
    rs = np.random.RandomState(3)
    for h in range(H):
        kk = k_out[0, h].double()
        kk = kk / kk.norm(dim=-1, keepdim=True).clamp_min(1e-6)
        rows = torch.from_numpy(rs.choice(S - n, 32, replace=False)).to(DEV)
        ke = keys[0, h, ev[0, h, rows]].double()
        ke = ke / ke.norm(dim=-1, keepdim=True).clamp_min(1e-6)
        best = torch.full((32,), -2.0, dtype=torch.float64, device=DEV)
        for c0 in range(0, n, 16384):
            best = torch.maximum(best, (ke @ kk[c0:c0 + 16384].T).max(-1).values)
        chosen = (ke * kk[tg[0, h, rows].long()]).sum(-1)
        assert (chosen >= best - 1e-5).all()
        torch.testing.assert_close(ms[0, h, rows].double(), best, atol=1e-5, rtol=0)
