"""CriticalKVPress / CriticalAdaKVPress without a GPU: the package surface, the classes' fields, assertions and warning next to the
reference's (kvpress/presses/criticalkv_press.py), the argument checks of the new C-ABI entries, the float64 oracle
(tests/_critical_oracle.py) against the REAL reference's outputs (tests/golden/crit_*.npz, tools/gen_golden_critical.py), and the host
logic of both presses over oracle-backed entry points against the same fixtures."""
import dataclasses
import logging
import os

import numpy as np
import pytest
import torch

import _critical_inputs as CI
import _critical_oracle as CO
import _inputs

GOLD = os.path.join(os.path.dirname(__file__), "golden")
FMAX = np.finfo(np.float32).max


def gold(name):
    return np.load(os.path.join(GOLD, f"{name}.npz"))


@pytest.fixture(scope="module")
def lib():
    from kvpress_amd import build as B

    B.build()
    from kvpress_amd import _native

    return _native.lib()


# ---- surface ------------------------------------------------------------------------------------------------------------------------
def test_package_surface():
    import kvpress_amd as P
    from kvpress_amd.presses import criticalkv_press as M

    assert "CriticalAdaKVPress" in P.__all__ and "CriticalAdaKVPress" not in P._NOT_BUILT and P.CriticalAdaKVPress is M.CriticalAdaKVPress
    assert "CriticalKVPress" not in P.__all__
    with pytest.raises(AttributeError, match="outside the hot-path scope") as e:
        P.CriticalKVPress
    assert "kvpress_amd.presses.criticalkv_press.CriticalKVPress" in str(e.value)
    assert issubclass(M.CriticalKVPress, P.ScorerPress) and issubclass(M.CriticalAdaKVPress, P.BasePress)
    assert not issubclass(M.CriticalAdaKVPress, P.ScorerPress)


def test_fields_and_defaults_are_the_references():
    """criticalkv_press.py:37 (CriticalKVPress.__init__) and :118-121 (the dataclass fields of CriticalAdaKVPress)"""
    import inspect

    import kvpress_amd as P
    from kvpress_amd.presses.criticalkv_press import CriticalAdaKVPress, CriticalKVPress

    sig = inspect.signature(CriticalKVPress.__init__)
    assert [(n, p.default) for n, p in list(sig.parameters.items())[1:]] == [("press", inspect.Parameter.empty), ("epsilon", 1e-4),
                                                                               ("first_stage_ratio", 0.5)]
    assert [(f.name, f.default) for f in dataclasses.fields(CriticalAdaKVPress)] == [("press", None), ("alpha_safeguard", 0.20), ("epsilon", 1e-4),
                                                                                      ("first_stage_ratio", 0.5)]
    inner = P.KnormPress(0.25)
    for press in (CriticalKVPress(inner), CriticalAdaKVPress(inner)):
        assert press.compression_ratio == 0.25           # the property delegates to the wrapped press, both ways
        press.compression_ratio = 0.5
        assert inner.compression_ratio == 0.5
        inner.compression_ratio = 0.25
        assert (press.epsilon, press.first_stage_ratio) == (1e-4, 0.5)
    assert callable(CriticalKVPress.vwl1norm) and isinstance(inspect.getattr_static(CriticalKVPress, "vwl1norm"), staticmethod)

    class Recorder(P.KnormPress):
        def post_init_from_model(self, model):
            self.seen = model

    for cls in (CriticalKVPress, CriticalAdaKVPress):
        r = Recorder(0.5)
        cls(r).post_init_from_model("model")
        assert r.seen == "model"


def test_assertions_and_warning(caplog):
    import kvpress_amd as P
    from kvpress_amd.presses.criticalkv_press import CriticalAdaKVPress, CriticalKVPress

    for cls in (CriticalKVPress, CriticalAdaKVPress):
        with pytest.raises(AssertionError, match="requires a ScorerPress"):
            cls(P.AdaKVPress(P.KnormPress(0.5)))
    with pytest.raises(AssertionError, match="requires a ScorerPress"):
        CriticalAdaKVPress()
    for alpha in (-0.1, 1.5):
        with pytest.raises(AssertionError, match="alpha_safeguard"):
            CriticalAdaKVPress(P.KnormPress(0.5), alpha_safeguard=alpha)
    for cls in (CriticalKVPress, CriticalAdaKVPress):
        caplog.clear()
        with caplog.at_level(logging.WARNING, logger="kvpress_amd.presses.criticalkv_press"):
            cls(P.ExpectedAttentionPress(0.5, use_vnorm=False))
            assert not caplog.records
            cls(P.ExpectedAttentionPress(0.5))
        assert len(caplog.records) == 1 and f"use_vnorm should be disabled for {cls.__name__}" in caplog.records[0].getMessage()


def test_ratio_zero_and_no_cpu_fallback():
    import kvpress_amd as P
    from kvpress_amd._native import KvpressHipError
    from kvpress_amd.presses.criticalkv_press import CriticalAdaKVPress, CriticalKVPress

    k, v = torch.zeros(1, 2, 16, 8), torch.ones(1, 2, 16, 8)
    for cls in (CriticalKVPress, CriticalAdaKVPress):
        k0, v0 = cls(P.KnormPress(0.0)).compress(None, None, k, v, None, {})
        assert k0 is k and v0 is v
    s = CI.make_case("crit_knorm_s257_d16")
    att, _, hidden, pe = _inputs.build_llama_attention(s, torch.float32)
    att.config._attn_implementation = "sdpa"
    keys, values = torch.from_numpy(s["keys"]), torch.from_numpy(s["values"])
    for cls in (CriticalKVPress, CriticalAdaKVPress):
        with pytest.raises(KvpressHipError):
            cls(P.KnormPress(0.5)).compress(att, hidden, keys, values, None, {"position_embeddings": pe})
    from kvpress_amd import _native

    with pytest.raises(KvpressHipError):
        _native.vwl1norm(values, att.o_proj.weight, s["Hq"])
    with pytest.raises(KvpressHipError):
        _native.vwl1norm_rescale_(torch.zeros(1, 2, s["S"]), values, att.o_proj.weight, s["Hq"], 1e-4)
    with pytest.raises(KvpressHipError):
        _native.scores_fill_prefix_(torch.zeros(2, 8), torch.zeros(2, 3, dtype=torch.int32), torch.zeros(2, dtype=torch.int32), 1.0)


# ---- C ABI ----------------------------------------------------------------------------------------------------------------------------
def test_capi_argument_errors_come_before_any_hip_call(lib):
    def rescale(dtype=2, Hq=4, Hkv=2, hidden=64, values=None, wo=None, out=None):
        return lib.kvp_vwl1norm_rescale(values, 0, 0, 0, dtype, wo, 64, 1, Hq, Hkv, 10, 16, hidden, None, 0, 1e-4, out, None, 0, None)

    assert rescale(dtype=7) == -1 and b"bad dtype" in lib.kvp_last_error()
    assert rescale(Hq=5) == -1 and b"Hq % Hkv != 0" in lib.kvp_last_error()
    assert rescale(Hkv=0) == -1 and b"Hq % Hkv != 0" in lib.kvp_last_error()
    for hidden in (0, -4):
        assert rescale(hidden=hidden) == -1 and b"hidden must be positive" in lib.kvp_last_error()
    assert rescale() == -1 and b"null pointer" in lib.kvp_last_error()
    assert lib.kvp_scores_fill_prefix(None, 2, 8, 8, None, 3, None, 1.0, None) == -1 and b"null pointer" in lib.kvp_last_error()
    assert lib.kvp_scores_fill_prefix(None, 2, 8, 4, None, 3, None, 1.0, None) == -1 and b"bad shape" in lib.kvp_last_error()
    assert lib.kvp_scores_fill_prefix(None, 0, 8, 8, None, 3, None, 1.0, None) == 0      # nothing to do


def test_workspace_is_nowhere_near_the_references_temporary(lib):
    """the reference's per-head [S, hidden] temporary alone is 1 GiB at this geometry (criticalkv_press.py:69)"""
    assert lib.kvp_vwl1norm_workspace_bytes(1, 32, 8, 131072, 128, 4096) < 32 << 20


# ---- the oracle against the reference's outputs -----------------------------------------------------------------------------------------
def _wo(s):
    att, _, _, _ = _inputs.build_llama_attention(s, torch.float32)
    return CI.wo_of(att)


def check_scores(got, ref, band, what):
    """final scores against the reference's: the protected entries (float32 max) at the same places outside the band, the others within
    2e-5 relative where finite, infinities at the same places"""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    free = ~band
    assert np.array_equal((got == FMAX) & free, (ref == FMAX) & free), f"{what}: protected entries differ outside the band"
    assert np.array_equal(np.isinf(got) & free, np.isinf(ref) & free), f"{what}: infinities differ"
    m = free & np.isfinite(ref) & np.isfinite(got)
    err = np.abs(got[m] - ref[m]) / np.maximum(np.abs(ref[m]), 1e-30)
    assert err.max() <= 2e-5, f"{what}: scores differ by {err.max():.3g} relative"


@pytest.mark.parametrize("name", list(CI.CASES))
def test_oracle_matches_reference(name):
    s, g = CI.make_case(name), gold(name)
    norm = CO.vwl1norm(s["values"], _wo(s), s["Hq"])
    err = np.abs(norm - g["norm"]) / np.abs(g["norm"])
    print(f"{name}: oracle norm vs the reference's float32 norm: {err.max():.3g} relative")
    assert err.max() <= 2e-5
    # the native 16-bit run of the reference rounds every product row to the dtype: a sanity band only
    assert np.abs(g["nat_norm"] - norm).max() / np.abs(norm).max() < 0.05
    inner = g["inner"]
    for i, r in enumerate(s["ratios"]):
        n_kept = int(s["S"] * (1 - r))
        final, band1 = CO.critical_scores(inner, norm, r, s["fsr"], CI.EPSILON)
        check_scores(final, g[f"crit_scores_{i}"], band1, f"{name} r={r}")
        # the reference's run on the 16-bit module rounds the inner scores, every product row, the norm and the result to the dtype
        nat = g[f"nat_crit_scores_{i}"].astype(np.float64)
        m = np.isfinite(nat) & np.isfinite(final) & (final < 1e30) & (nat < 1e30)      # neither protected nor overflowed
        m &= np.abs(final) > 1e-3 * np.abs(final[m]).max()
        dev16 = np.abs(nat[m] - final[m]) / np.abs(final[m])
        print(f"{name} r={r}: the reference's 16-bit scores vs the oracle: median {np.median(dev16):.3g}, worst {dev16.max():.3g} relative")
        assert np.median(dev16) < 0.02 and dev16.max() < 0.05     # (a handful of roundings at 2^-8 / 2^-11 each)
        pos, band2 = CO.kept_positions(final, n_kept)
        for h in range(s["H"]):
            assert CO.sets_equal_outside(pos[0, h], g[f"crit_pos_{i}"][0, h], band1[0, h] | band2[0, h]), f"{name} r={r} head {h}: kept positions"
        a = CO.critical_ada(inner, norm, r, s["alpha"], s["fsr"], CI.EPSILON)
        assert np.array_equal(a["budgets"][0], g[f"ada_budgets_{i}"]), f"{name} r={r}: budgets"
        assert CO.sets_equal_outside(a["masked"][0], g[f"ada_masked_{i}"], a["band"][0]), f"{name} r={r}: masked positions"


# ---- the presses' host logic over oracle-backed entry points ---------------------------------------------------------------------------
@pytest.fixture
def fake_critical(fake_native, monkeypatch):
    def norm32(values, wo, num_heads):
        return torch.from_numpy(CO.vwl1norm(values.float().numpy(), wo.detach().float().numpy(), num_heads).astype(np.float32))

    def vwl1norm_rescale_(scores, values, wo, num_heads, eps):
        return scores.add_(eps).mul_(norm32(values, wo, num_heads))

    def scores_fill_prefix_(scores, idx, counts, value):
        S = scores.shape[-1]
        rows, ir, cnt = scores.view(-1, S), idx.reshape(-1, idx.shape[-1]).long(), counts.reshape(-1).tolist()
        for r in range(rows.shape[0]):
            rows[r, ir[r, :cnt[r]]] = value
        return scores

    for name, fn in dict(vwl1norm=norm32, vwl1norm_rescale_=vwl1norm_rescale_, scores_fill_prefix_=scores_fill_prefix_).items():
        monkeypatch.setattr(fake_native, name, fn)
    return fake_native


def run_presses_against_fixture(name, dev, dtype=torch.float32):
    """both presses on the case's float32 module against the reference's outputs; shared with tests/test_gpu_critical.py"""
    import kvpress_amd as P
    from kvpress_amd import _native
    from kvpress_amd.presses.criticalkv_press import CriticalAdaKVPress, CriticalKVPress

    s, g = CI.make_case(name), gold(name)
    att, _, hidden, pe = _inputs.build_llama_attention(s, dtype, dev)
    att.config._attn_implementation = "sdpa"
    keys, values = torch.from_numpy(s["keys"]).to(dev, dtype), torch.from_numpy(s["values"]).to(dev, dtype)
    kw = {"position_embeddings": pe}
    S, H = s["S"], s["H"]
    with torch.no_grad():
        norm = CriticalKVPress.vwl1norm(values, att).cpu().numpy()
        assert norm.dtype == np.float32
        assert (np.abs(norm - g["norm"]) / np.abs(g["norm"])).max() <= 2e-5
        for i, r in enumerate(s["ratios"]):
            n_kept = int(S * (1 - r))
            ref_final, band1 = CO.critical_scores(g["inner"], g["norm"], r, s["fsr"], CI.EPSILON)
            _, band2 = CO.kept_positions(ref_final, n_kept)
            p = CriticalKVPress(CI.inner_press(P, s, r), epsilon=CI.EPSILON, first_stage_ratio=s["fsr"])
            sc = p.score(att, hidden, keys, values, None, kw)
            assert sc.dtype == torch.float32 and tuple(sc.shape) == (1, H, S)
            check_scores(sc.cpu().numpy(), g[f"crit_scores_{i}"], band1, f"{name} r={r}")
            ko, vo = p.compress(att, hidden, keys, values, None, kw)
            assert tuple(ko.shape) == (1, H, n_kept, s["D"]) == tuple(vo.shape)
            # the kept rows as positions: K rows are distinct, so each kept row is found again in the cache
            pos = _native_positions(ko, keys)
            for h in range(H):
                assert CO.sets_equal_outside(pos[0, h], g[f"crit_pos_{i}"][0, h], band1[0, h] | band2[0, h]), f"{name} r={r} head {h}: kept positions"

            a = CO.critical_ada(g["inner"], g["norm"], r, s["alpha"], s["fsr"], CI.EPSILON)
            ada = CriticalAdaKVPress(CI.inner_press(P, s, r), alpha_safeguard=s["alpha"], epsilon=CI.EPSILON, first_stage_ratio=s["fsr"])
            before = keys.clone()
            safeguarded = ada.press.score(att, hidden, keys, values, None, kw).float().clone()
            n_safe = int(n_kept * s["alpha"])
            if n_safe:
                _native.scores_fill_at_(safeguarded, _native.topk_select(safeguarded, n_safe), float(FMAX))
            assert np.array_equal(ada.head_budgets(safeguarded, n_kept).cpu().numpy()[0], g[f"ada_budgets_{i}"]), f"{name} r={r}: budgets"
            ko, vo = ada.compress(att, hidden, keys, values, None, kw)
            assert ko is keys and vo is values and torch.equal(keys, before)       # nothing is removed from the cache
            bi, hi, si = att.masked_key_indices
            n_pruned = H * (S - n_kept)
            assert bi.shape == hi.shape == si.shape == (n_pruned,) and bi.dtype == torch.int64 and int(bi.max()) == 0
            flat = (hi * S + si).cpu().numpy()
            assert np.array_equal(flat, np.sort(flat)) and len(set(flat.tolist())) == n_pruned
            assert CO.sets_equal_outside(flat, g[f"ada_masked_{i}"], a["band"][0]), f"{name} r={r}: masked positions"


def _native_positions(k_out: torch.Tensor, keys: torch.Tensor) -> np.ndarray:
    """positions [B,H,n] of the gathered rows k_out [B,H,n,D] in keys [B,H,S,D] (rows are distinct), sorted"""
    ko, k = k_out.float().cpu().numpy(), keys.float().cpu().numpy()
    B, H, n, _ = ko.shape
    pos = np.zeros((B, H, n), np.int64)
    for b in range(B):
        for h in range(H):
            eq = (ko[b, h][:, None, :] == k[b, h][None, :, :]).all(-1)
            assert (eq.sum(1) == 1).all()
            pos[b, h] = np.sort(eq.argmax(1))
    return pos


@pytest.mark.parametrize("name", list(CI.CASES))
def test_presses_host_logic_matches_reference(name, fake_critical):
    run_presses_against_fixture(name, "cpu")


def run_stage1_truncation(dev, monkeypatch):
    """CriticalAdaKVPress on scores built so that the head budgets are (90, 110), first_stage_ratio 0.7: stage 1 protects 63 entries of
    head 0 -- 90 * 0.7 as a float32 product is 63.0 (criticalkv_press.py:167: an int64 tensor times a Python float), as a Python float
    62.99999999999999, which truncates to 62.  Shared with tests/test_gpu_critical.py."""
    import kvpress_amd as P
    from kvpress_amd import _native

    assert int(90 * 0.7) == 62
    s = CI.make_case("crit_knorm_s257_d16")
    S, H = 200, s["H"]
    att, _, hidden, pe = _inputs.build_llama_attention(s, torch.float32, dev)
    att.config._attn_implementation = "sdpa"
    rs = np.random.RandomState(9)
    keys = torch.from_numpy(rs.standard_normal((1, H, S, s["D"])).astype(np.float32)).to(dev)
    values = torch.from_numpy(rs.standard_normal((1, H, S, s["D"])).astype(np.float32)).to(dev)
    sc = (rs.permutation(H * S).reshape(1, H, S) * 1e-3).astype(np.float32)            # distinct, all below 1
    for h, budget in enumerate((90, 110)):                                             # the n_kept * H = 200 largest of the flattened row
        sc[0, h, rs.choice(S, budget, replace=False)] += 10.0

    class GivenScores(P.ScorerPress):
        def score(self, module, hidden_states, keys, values, attentions, kwargs):
            return torch.from_numpy(sc).to(keys.device)

    calls, fill = [], _native.scores_fill_prefix_

    def spy(scores, idx, counts, value):
        out = fill(scores, idx, counts, value)
        calls.append((counts.reshape(-1).tolist(), (out == value).sum(-1).reshape(-1).tolist()))
        return out

    monkeypatch.setattr(_native, "scores_fill_prefix_", spy)
    press = P.CriticalAdaKVPress(GivenScores(0.5), alpha_safeguard=0.0, first_stage_ratio=0.7)
    with torch.no_grad():
        press.compress(att, hidden[:, :S], keys, values, None, {"position_embeddings": pe})
    assert len(calls) == 2
    assert calls[0] == ([63, 77], [63, 77]), calls[0]       # stage 1: counts handed to the library, entries at float32 max afterwards
    assert calls[1][0] == [90, 110]                         # stage 2: the head budgets themselves
    _, hi, _ = att.masked_key_indices
    assert torch.bincount(hi.cpu(), minlength=H).tolist() == [S - 90, S - 110]


def test_stage1_budgets_are_truncated_from_a_float32_product(fake_critical, monkeypatch):
    run_stage1_truncation("cpu", monkeypatch)


def test_ada_batch_elements_are_treated_alone(fake_critical):
    """the defined deviation: budgets per batch element (the reference adds them up over the batch and fails, :163-164, :176)"""
    import kvpress_amd as P
    from kvpress_amd.presses.criticalkv_press import CriticalAdaKVPress

    s = CI.make_case("crit_knorm_s257_d16")
    att, _, hidden, pe = _inputs.build_llama_attention(s, torch.float32)
    att.config._attn_implementation = "sdpa"
    rs = np.random.RandomState(5)
    keys = torch.from_numpy(np.concatenate([s["keys"], 3.0 * rs.standard_normal(s["keys"].shape).astype(np.float32)]))
    values = torch.from_numpy(np.concatenate([s["values"], rs.standard_normal(s["values"].shape).astype(np.float32)]))
    press = CriticalAdaKVPress(P.KnormPress(0.5), alpha_safeguard=0.2, first_stage_ratio=0.3)
    with torch.no_grad():
        press.compress(att, hidden.expand(2, -1, -1), keys, values, None, {"position_embeddings": pe})
        bi, hi, si = att.masked_key_indices
        both = [(hi[bi == b] * s["S"] + si[bi == b]).tolist() for b in range(2)]
        for b in range(2):
            press.compress(att, hidden, keys[b:b + 1], values[b:b + 1], None, {"position_embeddings": pe})
            _, hi1, si1 = att.masked_key_indices
            assert (hi1 * s["S"] + si1).tolist() == both[b]
    assert both[0] != both[1]
