"""CriticalKVPress / CriticalAdaKVPress without a GPU: the package surface, the classes' fields, assertions and warning next to the
reference's (kvpress/presses/criticalkv_press.py), the argument checks of the new C-ABI entries, the float64 oracle
(tests/_critical_oracle.py) against the REAL reference's outputs (tests/golden/crit_*.npz, oracle/gen_golden_critical.py), and the host
logic of both presses over oracle-backed entry points against the same fixtures."""
import dataclasses
import logging

import numpy as np
import pytest
import torch

import _critical_inputs as CI
import _critical_oracle as CO
import _inputs
from _critical_checks import check_scores, run_presses_against_fixture, run_stage1_truncation
from _support import golden


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


@pytest.mark.parametrize("name", list(CI.CASES))
def test_oracle_matches_reference(name):
    s, g = CI.make_case(name), golden(name)
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


@pytest.mark.parametrize("name", list(CI.CASES))
def test_presses_host_logic_matches_reference(name, fake_critical):
    run_presses_against_fixture(name, "cpu")


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
