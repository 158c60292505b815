"""MergingPress without a GPU: the float64 oracle against the reference's own outputs (tests/golden/mrg_*.npz), the press's host logic
with the library calls replaced by the oracle, the import surface, the chain's kept order and the C ABI's argument checks."""
import ctypes

import numpy as np
import pytest
import torch

import _inputs
import _merging_inputs as MI
import _merging_oracle as O
from _support import dtype_name, golden, kept_positions


def _nat_inputs(s, run):
    """the keys / values a run saw, as float32 arrays (the case's arrays are already rounded to its dtype)"""
    return s["keys"], s["values"]


@pytest.mark.parametrize("run", ["o32", "nat"])
@pytest.mark.parametrize("name", list(MI.CASES))
def test_oracle_reproduces_reference_goldens(name, run):
    s, g = MI.make_case(name), golden(name)
    keys, values = _nat_inputs(s, run)
    kept = g[f"{run}_kept"]
    dt = "f32" if run == "o32" else s["dtype"]
    o = O.merge(keys, values, kept, s["thr"], s["frac"], dt)
    S, n = s["S"], kept.shape[-1]
    if 0 < n < S:
        # the reference's float32 cosines against float64: the same nearest survivor wherever the runner-up is not within 2e-5
        np.testing.assert_allclose(o["max_sim"], g[f"{run}_max_sim"], atol=2e-5)
        diff = o["target"] != g[f"{run}_target"]
        for b, h, e in zip(*np.nonzero(diff)):
            sim = O.similarities(keys, kept, o["evicted"], b, h)[e]
            assert sim[g[f"{run}_target"][b, h, e]] >= sim.max() - 2e-5
    ref_v = g[f"{run}_v"]
    assert o["v"].shape == ref_v.shape
    scale = max(1.0, float(np.abs(ref_v).max(initial=0.0)))
    ulp = {"f32": 2e-5, "f16": 2 ** -10, "bf16": 2 ** -7}[dt]
    # float32 sums in the reference, float64 here, both rounded to the dtype: at most one unit in the last place apart, else 2e-5
    np.testing.assert_allclose(o["v"], ref_v, atol=2e-5 * scale, rtol=ulp)


def test_fixtures_cover_the_edge_cases():
    """the NaN-quantile row merges nothing, the duplicate keys tie, n_kept == 0 returns empty tensors"""
    s, g = MI.make_case("mrg_knorm_nanq_s200_d128"), golden("mrg_knorm_nanq_s200_d128")
    o = O.merge(s["keys"], s["values"], g["o32_kept"], s["thr"], s["frac"], "f32")
    assert o["merged"][0, 0].any() and not o["merged"][0, 1].any()
    masked = np.where(o["max_sim"] >= np.float32(s["thr"]), o["max_sim"], -np.inf)
    assert np.isnan(O.aten_quantile(masked, 1 - s["frac"])[0, 1])
    np.testing.assert_array_equal(g["o32_v"][0, 1], np.take_along_axis(s["values"][0, 1], g["o32_kept"][0, 1][:, None].astype(np.int64), 0))
    s, g = MI.make_case("mrg_knorm_dup_s96_d64"), golden("mrg_knorm_dup_s96_d64")
    ev = O.evicted_positions(g["o32_kept"], s["S"])
    ties = 0
    for h in range(s["H"]):
        sim = O.similarities(s["keys"], g["o32_kept"], ev, 0, h)
        best = sim.max(-1, keepdims=True)
        ties += int(((sim >= best - 1e-12).sum(-1) > 1).sum())
        np.testing.assert_array_equal(g["o32_target"][0, h], sim.argmax(-1))   # the lowest index among the tied
    assert ties > 0
    g = golden("mrg_knorm_nkept0_s20_d64")
    assert g["o32_v"].shape[2] == 0 and g["o32_kept"].shape[2] == 0


def test_aten_quantile_matches_torch():
    x = np.array([[-np.inf] * 3 + [0.5, 0.7, 0.9], [0.1, 0.4, -np.inf, 0.3, 0.2, 0.8]], dtype=np.float32)
    for q in (0.0, 0.1, 0.2, 0.39, 0.4, 0.41, 0.5, 0.55, 0.7, 1.0):
        np.testing.assert_array_equal(O.aten_quantile(x, q), torch.from_numpy(x).quantile(q, dim=-1).numpy())


def test_import_surface_and_asserts():
    import kvpress_amd as P
    from kvpress_amd import KnormPress, MergingPress

    assert "MergingPress" in P.__all__ and P.MergingPress is MergingPress
    with pytest.raises(AssertionError, match="MergingPress requires a ScorerPress, got NoneType"):
        MergingPress()
    with pytest.raises(AssertionError, match="MergingPress requires a ScorerPress, got ComposedPress"):
        MergingPress(P.ComposedPress([KnormPress(0.5)]))
    with pytest.raises(AssertionError):
        MergingPress(KnormPress(0.5), similarity_threshold=1.5)
    with pytest.raises(AssertionError):
        MergingPress(KnormPress(0.5), similarity_threshold=-0.1)
    with pytest.raises(AssertionError, match=r"merge_fraction must be in \(0, 1\]"):
        MergingPress(KnormPress(0.5), merge_fraction=0.0)
    p = MergingPress(KnormPress(0.25))
    assert p.compression_ratio == 0.25
    p.compression_ratio = 0.5
    assert p.press.compression_ratio == 0.5
    assert (p.similarity_threshold, p.merge_fraction) == (0.0, 1.0)


def test_post_init_from_model_forwards():
    from kvpress_amd import KnormPress, MergingPress

    seen = []

    class Inner(KnormPress):
        def post_init_from_model(self, model):
            seen.append(model)

    MergingPress(Inner(0.5)).post_init_from_model("m")
    assert seen == ["m"]


@pytest.fixture(scope="module")
def lib():
    from kvpress_amd import _native
    from kvpress_amd import build as B

    B.build()
    return _native.lib()


@pytest.fixture
def oracle_merge(monkeypatch, fake_native):
    """fake_native's select / gather plus a merge_values_ backed by the oracle (CPU tensors), recording its calls"""
    from kvpress_amd import _native

    calls = []

    def merge_values_(keys, values, kept_idx, k_out, v_out, threshold, fraction, target=None, max_sim=None):
        calls.append((tuple(keys.shape), tuple(kept_idx.shape), threshold, fraction))
        o = O.merge(keys.float().numpy(), values.float().numpy(), kept_idx.numpy(), threshold, fraction, dtype_name(v_out.dtype))
        v_out.copy_(torch.from_numpy(o["v"]).to(v_out.dtype))
        return v_out

    monkeypatch.setattr(_native, "merge_values_", merge_values_)
    return calls


@pytest.mark.parametrize("name", ["mrg_knorm_b2_s333_d128", "mrg_snapkv_s300_d64_g4", "mrg_keydiff_s157_d256_f32", "mrg_knorm_nanq_s200_d128",
                                  "mrg_knorm_nkept0_s20_d64"])
@pytest.mark.parametrize("order", ["position", "score"])
def test_compress_on_host_matches_reference(name, order, oracle_merge):
    import kvpress_amd as P

    s, g = MI.make_case(name), golden(name)
    module, hidden, kw = MI.module_and_kwargs(s, torch.float32)
    keys = torch.from_numpy(s["keys"])
    values = torch.from_numpy(s["values"])
    k0, v0 = keys.clone(), values.clone()
    inner = MI.inner_press(s, P)
    inner.kept_order = order
    press = P.MergingPress(inner, similarity_threshold=s["thr"], merge_fraction=s["frac"])
    with torch.no_grad():
        k2, v2 = press.compress(module, hidden, keys, values, None, kw)
    assert torch.equal(keys, k0) and torch.equal(values, v0)
    kept = g["o32_kept"]
    ref_v = g["o32_v"]
    n = kept.shape[-1]
    assert len(oracle_merge) == (1 if 0 < n < s["S"] else 0)
    if order == "position" or s["press"] == "snapkv":
        # SnapKV's window tokens all score max + 1: their order among themselves is torch.topk's choice, so compare by position
        perm = np.argsort(kept, axis=-1, kind="stable")
        kept = np.take_along_axis(kept, perm, -1)
        ref_v = np.take_along_axis(ref_v, perm[..., None].repeat(s["D"], -1), 2)
        if order == "score":
            mine = np.argsort(kept_positions(k2.numpy(), s["keys"]), axis=-1, kind="stable")
            k2 = torch.from_numpy(np.take_along_axis(k2.numpy(), mine[..., None].repeat(s["D"], -1), 2))
            v2 = torch.from_numpy(np.take_along_axis(v2.numpy(), mine[..., None].repeat(s["D"], -1), 2))
    np.testing.assert_array_equal(k2.numpy(), np.take_along_axis(s["keys"], kept[..., None].astype(np.int64).repeat(s["D"], -1), 2))
    np.testing.assert_allclose(v2.numpy(), ref_v, atol=2e-5 * max(1.0, float(np.abs(ref_v).max(initial=0.0))), rtol=2e-5)


def test_chain_switches_inner_press_to_score_order():
    from kvpress_amd import ComposedPress, KnormPress, MergingPress, StreamingLLMPress
    from kvpress_amd.presses.scorer_press import resolve_chain_kept_order

    inner = KnormPress(0.5)
    chain = ComposedPress([MergingPress(inner), StreamingLLMPress(0.25)])
    chain._check_kept_order()     # what its first hook call does
    assert inner.kept_order == "score"
    assert chain.presses[0].press is inner
    inner2 = KnormPress(0.5)
    assert resolve_chain_kept_order(MergingPress(inner2), [StreamingLLMPress(0.25)], "test") == "switched"
    assert inner2.kept_order == "score"


def test_capi_argument_checks(lib):
    f = lib.kvp_merge_values
    args = [None, 0, 0, 0, None, 0, 0, 0, None, None, None]
    rc = f(*args, 7, 1, 1, 10, 5, 64, ctypes.c_double(0.0), ctypes.c_double(1.0), None, 0, None, None, None)
    assert rc == -1 and b"dtype" in lib.kvp_last_error()
    rc = f(*args, 2, 1, 1, 10, 11, 64, ctypes.c_double(0.0), ctypes.c_double(1.0), None, 0, None, None, None)
    assert rc == -1 and b"bad shape" in lib.kvp_last_error()
    rc = f(*args, 2, 1, 1, 10, 5, 64, ctypes.c_double(0.0), ctypes.c_double(0.0), None, 0, None, None, None)
    assert rc == -1 and b"merge_fraction" in lib.kvp_last_error()
    rc = f(*args, 2, 1, 1, 10, 5, 512, ctypes.c_double(0.0), ctypes.c_double(1.0), None, 0, None, None, None)
    assert rc == -1 and b"head size" in lib.kvp_last_error()
    rc = f(*args, 2, 1, 1, 10, 5, 64, ctypes.c_double(0.0), ctypes.c_double(1.0), None, 0, None, None, None)
    assert rc == -1 and b"null pointer" in lib.kvp_last_error()
    # n_kept == 0 or n_kept == S: nothing to merge (merging_press.py:120-121), no pointer is touched
    assert f(*args, 2, 1, 1, 10, 0, 64, ctypes.c_double(0.0), ctypes.c_double(1.0), None, 0, None, None, None) == 0
    assert f(*args, 2, 1, 1, 10, 10, 64, ctypes.c_double(0.0), ctypes.c_double(1.0), None, 0, None, None, None) == 0


def test_workspace_is_linear_in_tokens(lib):
    """O(B*H*S): Llama-3.1-8B at 128k needs ~32 MiB, never anything of size n_evict x n_kept"""
    n = lib.kvp_merge_workspace_bytes(1, 8, 131072, 65536, 128)
    assert 0 < n <= 40 << 20
    assert lib.kvp_merge_workspace_bytes(1, 8, 2 * 131072, 131072, 128) <= 2 * n + 4096
    assert lib.kvp_merge_workspace_bytes(0, 8, 100, 50, 128) == 0
