"""Compactor family without a GPU: the float64 oracle against the reference's own outputs (tests/golden/cpt_*.npz), the presses' host
logic with the library calls replaced by the oracle, the import surface, the C ABI's argument checks and workspace sizes."""
import ctypes

import numpy as np
import pytest
import torch

import _compactor_inputs as CI
import _compactor_oracle as O
from _support import golden


def _o32_inputs(s):
    from kvpress_amd.utils import get_prerope_key_states, get_prerope_query_states

    att, hidden, (cos, sin) = CI.build_attention(s, torch.float32)
    keys = CI.post_rope_keys(att, hidden, (cos, sin))
    with torch.no_grad():
        q = get_prerope_query_states(att, hidden)
        kpre = get_prerope_key_states(att, hidden)
    return att, hidden, (cos, sin), q.numpy(), kpre.numpy(), keys.numpy(), s["values"]


@pytest.mark.parametrize("name", list(CI.CASES))
def test_oracle_reproduces_reference_goldens(name):
    s, g = CI.make_case(name), golden(name)
    att, hidden, (cos, sin), q, kpre, keys, values = _o32_inputs(s)
    # the reference runs in float32, the oracle in float64: measured <= 9e-6 relative on these cases
    nc = O.ncattn_raw(q, cos.numpy(), sin.numpy(), keys, values, s["chunk"], "f32")
    np.testing.assert_allclose(nc, g["o32_nc_raw"], rtol=2e-5, atol=0)
    np.testing.assert_allclose(O.zscore(nc), g["o32_nc_z"], atol=3e-5 * np.abs(g["o32_nc_z"]).max())
    lev = O.leverage_raw(kpre, CI.phi_from_draw(g["o32_lev_phi_draw"], s["sketch"], torch.float32), "f32")
    np.testing.assert_allclose(lev, g["o32_lev_raw"], rtol=2e-5, atol=0)
    np.testing.assert_allclose(O.zscore(lev), g["o32_lev_z"], atol=3e-5 * np.abs(g["o32_lev_z"]).max())
    for ratio in CI.RATIOS:
        tag = f"o32_cpt_r{int(ratio * 100)}"
        left, right = s["sinks"]
        S = s["S"]
        inner = slice(left, S - right)
        ncz = O.zscore(O.ncattn_raw(q[:, :, inner], cos.numpy()[:, inner], sin.numpy()[:, inner], keys[:, :, inner], values[:, :, inner],
                                    s["chunk"], "f32"))
        lz = O.zscore(O.leverage_raw(kpre[:, :, inner], CI.phi_from_draw(g[tag + "_phi_draw"], s["sketch"], torch.float32), "f32"))
        sc = O.compactor_combine(lz, ncz, left, right, ratio)
        np.testing.assert_allclose(sc, g[tag + "_scores"], atol=5e-5 * np.abs(g[tag + "_scores"]).max())
        assert O.kept_sets_equal_up_to_ties(sc, g[tag + "_scores"], O.n_kept(S, ratio), 1e-4 * np.abs(sc).max())


@pytest.fixture
def oracle_native(monkeypatch):
    """kvpress_amd._native's Compactor calls replaced by the oracle (CPU tensors in and out), recording their arguments."""
    from kvpress_amd import _native

    calls = []

    def nc(q, cos, sin, keys, values, chunk):
        calls.append(("nc", tuple(keys.shape), chunk))
        raw = O.ncattn_raw(q.float().numpy(), cos.float().numpy(), sin.float().numpy(), keys.float().numpy(), values.float().numpy(), chunk, "f32")
        return torch.from_numpy(O.zscore(raw)).float()

    def lev(kpre, phi, return_raw=False):
        calls.append(("lev", tuple(kpre.shape), tuple(phi.shape)))
        raw = O.leverage_raw(kpre.float().numpy(), phi.float().numpy(), "f32")
        z = torch.from_numpy(O.zscore(raw)).float()
        return (z, torch.from_numpy(raw).float()) if return_raw else z

    def comb(zl, za, left, right, blending):
        calls.append(("comb", left, right, blending))
        return torch.from_numpy(O.compactor_combine(zl.numpy(), za.numpy(), left, right, blending)).float()

    monkeypatch.setattr(_native, "ncattn_score", nc)
    monkeypatch.setattr(_native, "leverage_score", lev)
    monkeypatch.setattr(_native, "compactor_combine", comb)
    return calls


@pytest.mark.parametrize("name", ["cpt_s200_c256_d128_g8", "cpt_b2_s333_c64_d96_g4"])
def test_compactor_host_logic_matches_reference(name, oracle_native):
    import kvpress_amd as P

    s, g = CI.make_case(name), golden(name)
    att, hidden, pe, *_ = _o32_inputs(s)
    keys = torch.from_numpy(CI.post_rope_keys(att, hidden, pe).numpy())
    values = torch.from_numpy(s["values"])
    for ratio in CI.RATIOS:
        tag = f"o32_cpt_r{int(ratio * 100)}"
        p = P.CompactorPress(ratio, sink_size_start=s["sinks"][0], sink_size_end=s["sinks"][1], chunk_size=s["chunk"],
                             sketch_dimension=s["sketch"])
        draw = torch.from_numpy(g[tag + "_phi_draw"])
        orig = torch.randn
        try:
            torch.randn = lambda *a, **kw: draw   # the reference's draw: the press scales it by 1 / sqrt(k) itself
            with torch.no_grad():
                sc = p.score(att, hidden, keys, values, None, {"position_embeddings": pe})
        finally:
            torch.randn = orig
        assert sc.shape == (s["B"], s["H"], s["S"])
        np.testing.assert_allclose(sc.numpy(), g[tag + "_scores"], atol=5e-5 * np.abs(g[tag + "_scores"]).max())
        left, right = s["sinks"]
        assert ("comb", left, right, ratio) in oracle_native
        assert ("nc", (s["B"], s["H"], s["S"] - left - right, s["D"]), s["chunk"]) in oracle_native
        if left:
            assert (sc[..., :left] == sc.max()).all() and (sc[..., s["S"] - right:] == sc.max()).all()


def test_blending_default_and_setattr_propagation(oracle_native):
    import kvpress_amd as P

    p = P.CompactorPress(0.3, sink_size_start=0, sink_size_end=0)
    assert p._leverage_press.compression_ratio == 0.3 and p._non_causal_press.chunk_size == 256 and p._leverage_press.sketch_dimension == 48
    p.compression_ratio = 0.6
    p.chunk_size = 64
    p.sketch_dimension = 32
    assert p._leverage_press.compression_ratio == 0.6 and p._non_causal_press.compression_ratio == 0.6
    assert p._non_causal_press.chunk_size == 64 and p._leverage_press.sketch_dimension == 32
    s = CI.make_case("cpt_s256_c128_d64_g4")
    att, hidden, pe, *_ = _o32_inputs(s)
    keys = CI.post_rope_keys(att, hidden, pe)
    values = torch.from_numpy(s["values"])
    with torch.no_grad():
        p.score(att, hidden, keys, values, None, {"position_embeddings": pe})
        assert oracle_native[-1] == ("comb", 0, 0, 0.6)          # blending defaults to compression_ratio
        p.blending = 0.1
        p.score(att, hidden, keys, values, None, {"position_embeddings": pe})
        assert oracle_native[-1] == ("comb", 0, 0, 0.1)
        p.blending, p.compression_ratio = None, None
        p.score(att, hidden, keys, values, None, {"position_embeddings": pe})
        assert oracle_native[-1] == ("comb", 0, 0, 0.35)         # ... and to 0.35 without one
    assert ("nc", (1, 2, 256, 64), 64) in oracle_native


def test_prefill_only(oracle_native):
    import kvpress_amd as P

    s = CI.make_case("cpt_s256_c128_d64_g4")
    att, hidden, pe, *_ = _o32_inputs(s)
    keys = CI.post_rope_keys(att, hidden, pe)
    values = torch.from_numpy(s["values"])
    for p in (P.CompactorPress(0.5), P.LeverageScorePress(0.5), P.NonCausalAttnPress(0.5)):
        with pytest.raises(AssertionError, match="prefill"):
            p.score(att, hidden[:, -1:], keys, values, None, {"position_embeddings": pe})


def test_package_surface():
    import kvpress_amd as P
    from kvpress_amd import CompactorPress, LeverageScorePress, NonCausalAttnPress  # noqa: F401

    assert {"CompactorPress", "LeverageScorePress", "NonCausalAttnPress"} <= set(P.__all__)
    assert P.CompactorPress.__name__ == "CompactorPress"
    with pytest.raises(AttributeError, match="outside the hot-path scope"):
        P.CriticalKVPress
    assert callable(P.LeverageScorePress.chol_with_jitter) and callable(P.LeverageScorePress.compute_leverage_scores)
    L = P.LeverageScorePress.chol_with_jitter(torch.eye(3) * 2, jitter=1e-2)
    assert torch.allclose(L @ L.T, torch.eye(3) * 2.01)


def test_capi_checks_and_workspace_sizes():
    from kvpress_amd import _native

    lib = _native.lib()
    # Llama-3.1-8B geometry at 128k: a few MiB, never of order Hq * S * chunk (32 * 131072 * 256 * 4 bytes = 4 GiB)
    assert lib.kvp_ncattn_workspace_bytes(1, 8, 131072) < 16 << 20
    assert lib.kvp_leverage_workspace_bytes(1, 8, 131072, 128, 48) < 16 << 20
    assert lib.kvp_leverage_workspace_bytes(1, 8, 131072, 128, 256) < 32 << 20
    assert lib.kvp_compactor_combine_workspace_bytes() <= 4096
    rc = lib.kvp_ncattn_score(None, 0, 0, 0, None, None, 0, 0, None, 0, 0, 0, None, 0, 0, 0, 2, 1, 4, 2, 100, 128, 256, None, None, None, 0, None)
    assert rc == -1 and b"null pointer" in lib.kvp_last_error()
    p = ctypes.c_void_p(16)
    rc = lib.kvp_ncattn_score(p, 0, 0, 0, p, p, 0, 0, p, 0, 0, 0, p, 0, 0, 0, 2, 1, 4, 2, 100, 128, 0, None, p, p, 1 << 30, None)
    assert rc == -1 and b"chunk_size" in lib.kvp_last_error()
    rc = lib.kvp_ncattn_score(p, 0, 0, 0, p, p, 0, 0, p, 0, 0, 0, p, 0, 0, 0, 2, 1, 6, 4, 100, 128, 256, None, p, p, 1 << 30, None)
    assert rc == -1 and b"Hq % Hkv" in lib.kvp_last_error()
    rc = lib.kvp_ncattn_score(p, 0, 0, 0, p, p, 0, 0, p, 0, 0, 0, p, 0, 0, 0, 7, 1, 4, 2, 100, 128, 256, None, p, p, 1 << 30, None)
    assert rc == -1 and b"dtype" in lib.kvp_last_error()
    rc = lib.kvp_leverage_score(p, 0, 0, 0, p, 0, 0, 0, 2, 1, 2, 100, 128, 257, None, p, p, 1 << 30, None)
    assert rc == -1 and b"sketch_dimension" in lib.kvp_last_error()
    rc = lib.kvp_leverage_score(p, 0, 0, 0, None, 0, 0, 0, 2, 1, 2, 100, 128, 48, None, p, p, 1 << 30, None)
    assert rc == -1 and b"null pointer" in lib.kvp_last_error()
    rc = lib.kvp_compactor_combine(None, None, 1, 1, 10, 0, 0, ctypes.c_float(0.5), None, None, 0, None)
    assert rc == -1 and b"null pointer" in lib.kvp_last_error()
