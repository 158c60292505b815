"""Compactor family on the MI355X: the kernels against the float64 oracle over a shape sweep (MFMA and generic paths), the presses'
compress() against the reference's own outputs (tests/golden/cpt_*.npz) with the recorded sketch injected, run-to-run bit identity,
and a 128k Llama-3.1-8B-geometry CompactorPress."""
import os

import numpy as np
import pytest
import torch

import _compactor_inputs as CI
import _compactor_oracle as O
from _inputs import round_to, torch_dtype
from _support import golden

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _nc_inputs(B, Hkv, G, S, D, dt, seed):
    rs = np.random.RandomState(seed)
    q = round_to(rs.standard_normal((B, Hkv * G, S, D)).astype(np.float32) * 0.5, dt)
    k = round_to(rs.standard_normal((B, Hkv, S, D)).astype(np.float32) * 0.5, dt)
    v = round_to(rs.standard_normal((B, Hkv, S, D)).astype(np.float32), dt)
    ang = np.arange(S)[:, None] * (10000.0 ** (-np.arange(D // 2) / (D // 2)))[None]
    ang = np.concatenate([ang, ang], -1)[None]
    return q, k, v, round_to(np.cos(ang).astype(np.float32), dt), round_to(np.sin(ang).astype(np.float32), dt)


NC_SWEEP = [  # (B, Hkv, G, S, D, chunk, dtype)
    (1, 2, 4, 127, 128, 128, "bf16"), (1, 2, 4, 128, 128, 128, "bf16"), (1, 2, 4, 129, 128, 128, "bf16"),
    (2, 2, 4, 1000, 128, 256, "bf16"), (1, 1, 8, 4097, 128, 256, "bf16"), (1, 2, 1, 1000, 64, 128, "f16"),
    (2, 1, 4, 255, 64, 256, "f16"), (1, 2, 4, 1000, 96, 64, "bf16"), (1, 1, 4, 513, 256, 512, "bf16"),
    (1, 2, 16, 300, 128, 512, "bf16"), (1, 2, 4, 300, 256, 256, "f16"),
    (1, 2, 4, 300, 128, 128, "f32"), (1, 2, 2, 301, 64, 100, "bf16"), (1, 1, 3, 77, 48, 32, "f16"),
]


@pytest.mark.parametrize("B,Hkv,G,S,D,chunk,dt", NC_SWEEP)
def test_ncattn_kernel_vs_oracle(B, Hkv, G, S, D, chunk, dt):
    from kvpress_amd import _native

    q, k, v, cos, sin = _nc_inputs(B, Hkv, G, S, D, dt, seed=S + D + chunk)
    want = O.ncattn_raw(q, cos, sin, k, v, chunk, dt)
    tdt = torch_dtype(dt)
    T = lambda a: torch.from_numpy(a).to(DEV, tdt)   # noqa: E731
    z, raw = _native.ncattn_score(T(q), T(cos), T(sin), T(k), T(v), chunk, return_raw=True)
    z2 = _native.ncattn_score(T(q), T(cos), T(sin), T(k), T(v), chunk)
    torch.cuda.synchronize()
    raw, z = raw.cpu().numpy(), z.cpu().numpy()
    assert np.array_equal(z, z2.cpu().numpy()), "not run-to-run identical"
    # every element: raw <= 1e-3 relative, z-scores <= 1e-3 * max|z| (worst measured over this sweep: 2.2e-4 and 1.7e-4, bf16 logits
    # that round to the neighbouring 16-bit number after the kernel's and the oracle's different summation orders)
    rel = np.abs(raw - want) / np.abs(want)
    assert rel.max() <= 1e-3, rel.max()
    wz = O.zscore(want)
    assert np.abs(z - wz).max() <= 1e-3 * np.abs(wz).max(), np.abs(z - wz).max() / np.abs(wz).max()


def test_ncattn_generic_path_matches_mfma():
    """the same bf16 shape through both kernels (KVP_NCATTN_GENERIC=1 forces the generic one)"""
    from kvpress_amd import _native

    q, k, v, cos, sin = _nc_inputs(1, 2, 4, 700, 128, "bf16", seed=3)
    T = lambda a: torch.from_numpy(a).to(DEV, torch.bfloat16)   # noqa: E731
    want = O.ncattn_raw(q, cos, sin, k, v, 256, "bf16")
    _, a = _native.ncattn_score(T(q), T(cos), T(sin), T(k), T(v), 256, return_raw=True)
    os.environ["KVP_NCATTN_GENERIC"] = "1"
    try:
        _native.tuning_reload()
        _, b = _native.ncattn_score(T(q), T(cos), T(sin), T(k), T(v), 256, return_raw=True)
    finally:
        del os.environ["KVP_NCATTN_GENERIC"]
        _native.tuning_reload()
    a, b = a.cpu().numpy(), b.cpu().numpy()
    assert (np.abs(a - want) / np.abs(want)).max() <= 1e-3 and (np.abs(b - want) / np.abs(want)).max() <= 1e-3
    assert np.abs(a - b).max() <= 1e-4 * np.abs(want).max()


@pytest.mark.parametrize("B,H,S,D,ks,dt", [(1, 2, 300, 128, 48, "bf16"), (2, 2, 1000, 64, 64, "f16"), (1, 1, 4097, 128, 48, "f32"),
                                           (1, 2, 257, 96, 256, "f32"), (1, 1, 100, 256, 7, "bf16"), (1, 1, 50, 64, 1, "f32")])
def test_leverage_kernel_vs_oracle(B, H, S, D, ks, dt):
    from kvpress_amd import _native

    rs = np.random.RandomState(S + ks)
    k = round_to(rs.standard_normal((B, H, S, D)).astype(np.float32), dt)
    phi = round_to((rs.standard_normal((B, H, D, ks)) / np.sqrt(ks)).astype(np.float32), dt)
    want = O.leverage_raw(k, phi, dt)
    tdt = torch_dtype(dt)
    z, raw = _native.leverage_score(torch.from_numpy(k).to(DEV, tdt), torch.from_numpy(phi).to(DEV, tdt), return_raw=True)
    z2 = _native.leverage_score(torch.from_numpy(k).to(DEV, tdt), torch.from_numpy(phi).to(DEV, tdt))
    raw, z = raw.cpu().numpy(), z.cpu().numpy()
    assert np.array_equal(z, z2.cpu().numpy())
    # worst measured: 1.4e-3 raw / 2.1e-3 max|z| on the f16 case (D 64, sketch 64), where a few sketch values x land on the
    # neighbouring f16 number after the kernel's float32 and the oracle's float64 dot products; <= 2.2e-5 on every other case
    rel = np.abs(raw - want) / np.abs(want)
    assert np.quantile(rel, 0.999) <= 1e-3 and rel.max() <= 3e-3, (np.quantile(rel, 0.999), rel.max())
    wz = O.zscore(want)
    dz = np.abs(z - wz) / np.abs(wz).max()
    assert np.quantile(dz, 0.99) <= 1e-3 and dz.max() <= 3e-3, (np.quantile(dz, 0.99), dz.max())


def test_leverage_cholesky_failure_is_loud():
    """leverage_press.py:56 raises RuntimeError when the factorisation fails after five jitters: keys with a NaN make every pivot
    NaN, and the library says so through kvp_last_error instead of returning scores"""
    from kvpress_amd import _native

    k = torch.randn(1, 2, 64, 64, device=DEV)
    k[0, 1, 5, 3] = float("nan")
    phi = torch.randn(1, 2, 64, 48, device=DEV) / np.sqrt(48)
    with pytest.raises(_native.KvpressHipError, match="Cholesky failed after 5 tries"):
        _native.leverage_score(k, phi)
    _native.leverage_score(torch.randn(1, 2, 64, 64, device=DEV), phi)   # the next call is unaffected


@pytest.mark.parametrize("name", list(CI.CASES))
def test_compactor_compress_vs_reference_o32(name):
    """CompactorPress.compress() on the float32 module with the reference's recorded sketch: scores within the reference's own float32
    noise, kept sets equal up to ties (the sink pads tie with the argmax in the reference itself)."""
    import kvpress_amd as P

    s, g = CI.make_case(name), golden(name)
    att, hidden, pe = CI.build_attention(s, torch.float32, DEV)
    keys = CI.post_rope_keys(att, hidden, pe)
    values = torch.from_numpy(s["values"]).to(DEV)
    for ratio in CI.RATIOS:
        tag = f"o32_cpt_r{int(ratio * 100)}"
        p = P.CompactorPress(ratio, sink_size_start=s["sinks"][0], sink_size_end=s["sinks"][1], chunk_size=s["chunk"],
                             sketch_dimension=s["sketch"])
        draw = torch.from_numpy(g[tag + "_phi_draw"]).to(DEV)
        orig = torch.randn
        try:
            torch.randn = lambda *a, **kw: draw   # noqa: B023  (the reference's draw; the press scales it by 1 / sqrt(k))
            with torch.no_grad():
                sc = p.score(att, hidden, keys, values, None, {"position_embeddings": pe}).cpu().numpy()
                ko, vo = p.compress(att, hidden, keys, values, None, {"position_embeddings": pe})
        finally:
            torch.randn = orig
        want = g[tag + "_scores"]
        # worst measured 3.5e-6 * max|score|: the library against the reference's float32 run
        assert np.abs(sc - want).max() <= 2e-5 * np.abs(want).max(), np.abs(sc - want).max() / np.abs(want).max()
        n = O.n_kept(s["S"], ratio)
        assert O.kept_sets_equal_up_to_ties(sc, want, n, 1e-4 * np.abs(want).max())
        assert ko.shape == (s["B"], s["H"], n, s["D"]) and vo.shape == ko.shape


@pytest.mark.parametrize("name", list(CI.CASES))
def test_noncausal_native_dtype_vs_reference(name):
    """the native-dtype (bf16) module: the reference's own z-scores of NonCausalAttnPress"""
    import kvpress_amd as P

    s, g = CI.make_case(name), golden(name)
    dt = torch_dtype(s["dtype"])
    att, hidden, pe = CI.build_attention(s, dt, DEV)
    keys = CI.post_rope_keys(att, hidden, pe)
    values = torch.from_numpy(s["values"]).to(DEV, dt)
    with torch.no_grad():
        z = P.NonCausalAttnPress(0.5, chunk_size=s["chunk"]).score(att, hidden, keys, values, None, {"position_embeddings": pe})
    want = g["nat_nc_z"]
    # bf16 logits: the GEMM library and the kernel sum in different orders, so a few logits round to the neighbouring bf16 number
    # (worst measured on the fixtures: 6e-4 * max|z|, 99th percentile 7e-5)
    d = np.abs(z.cpu().numpy() - want) / np.abs(want).max()
    assert np.quantile(d, 0.99) <= 2e-4 and d.max() <= 2e-3, (np.quantile(d, 0.99), d.max())


@pytest.mark.parametrize("H", [1, 2])
def test_compactor_single_token_middle(H):
    """13 tokens with the default sinks (8, 4) leave ONE token between them.  Its z-scores are the std of B * H values: NaN for one
    head (torch's std of a single element), and then every score is NaN as in the reference (the pad value is the NaN max);
    finite for two heads, equal to the oracle's"""
    import kvpress_amd as P

    s = CI.make_case("cpt_s256_c128_d64_g4", S=13, H=H, dtype="f32")
    att, hidden, pe = CI.build_attention(s, torch.float32, DEV)
    keys = CI.post_rope_keys(att, hidden, pe)
    values = torch.from_numpy(s["values"]).to(DEV)
    with torch.no_grad():
        sc = P.CompactorPress(0.5).score(att, hidden, keys, values, None, {"position_embeddings": pe}).cpu().numpy()
    assert sc.shape == (1, H, 13)
    if H == 1:
        assert np.isnan(sc).all()
        return
    with torch.no_grad():
        from kvpress_amd.utils import get_prerope_query_states
        q = get_prerope_query_states(att, hidden).cpu().numpy()
    cos, sin = pe[0].cpu().numpy(), pe[1].cpu().numpy()
    ncz = O.zscore(O.ncattn_raw(q[:, :, 8:9], cos[:, 8:9], sin[:, 8:9], keys.cpu().numpy()[:, :, 8:9], s["values"][:, :, 8:9], 256, "f32"))
    # leverage of a single token: x = 0 after centring, raw 0 on both heads, z = 0 / 0 -> NaN ... unless the std is clamped: 0 / 1e-6 = 0
    lz = np.zeros_like(ncz)
    want = O.compactor_combine(lz, ncz, 8, 4, 0.5)
    assert np.isfinite(sc).all() and np.abs(sc - want).max() <= 1e-5, (sc, want)


@pytest.mark.parametrize("cls,kw", [("CompactorPress", dict(compression_ratio=0.5, sink_size_start=0, sink_size_end=0)),
                                    ("CompactorPress", dict(compression_ratio=0.2, sink_size_start=8, sink_size_end=4)),
                                    ("LeverageScorePress", dict(compression_ratio=0.5, sketch_dimension=48)),
                                    ("LeverageScorePress", dict(compression_ratio=0.5, sketch_dimension=64)),
                                    ("NonCausalAttnPress", dict(compression_ratio=0.5, chunk_size=128)),
                                    ("NonCausalAttnPress", dict(compression_ratio=0.5, chunk_size=256))])
def test_reference_compactor_suite_on_tiny_llama(cls, kw):
    """the reference's tests/presses/test_compactor_press.py shape check: 30 tokens through the hook, cache length int(S * (1 - ratio))"""
    import kvpress_amd as P
    from transformers import DynamicCache

    import _inputs

    model = _inputs.make_tiny_llama(seed=0, device=DEV)
    press = getattr(P, cls)(**kw)
    ids = torch.randint(3, 64, (1, 30), device=DEV, generator=torch.Generator(DEV).manual_seed(0))
    with torch.no_grad(), press(model):
        cache = DynamicCache()
        model(ids, past_key_values=cache)
    n = int(30 * (1 - kw["compression_ratio"]))
    assert all(layer.keys.shape[2] == n for layer in cache.layers)


def test_compactor_128k_llama8b_geometry():
    """CompactorPress(0.5).compress() at 128k tokens, Llama-3.1-8B attention geometry (Hq 32, Hkv 8, D 128, hidden 4096), bf16: completes
    without any allocation of order Hq * S * chunk (4 GiB)"""
    import kvpress_amd as P
    from transformers import LlamaConfig
    from transformers.models.llama.modeling_llama import LlamaAttention, LlamaRotaryEmbedding

    S = 131072
    cfg = LlamaConfig(hidden_size=4096, num_attention_heads=32, num_key_value_heads=8, head_dim=128, num_hidden_layers=1,
                      intermediate_size=32, vocab_size=32, max_position_embeddings=S)
    torch.manual_seed(0)
    att = LlamaAttention(cfg, layer_idx=0).to(DEV, torch.bfloat16)
    rot = LlamaRotaryEmbedding(cfg).to(DEV)
    hidden = torch.randn(1, S, 4096, device=DEV, dtype=torch.bfloat16)
    cos, sin = rot(hidden, torch.arange(S, device=DEV)[None])
    keys = torch.randn(1, 8, S, 128, device=DEV, dtype=torch.bfloat16)
    values = torch.randn(1, 8, S, 128, device=DEV, dtype=torch.bfloat16)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    with torch.no_grad():
        ko, vo = P.CompactorPress(0.5).compress(att, hidden, keys, values, None, {"position_embeddings": (cos, sin)})
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    assert ko.shape == (1, 8, S // 2, 128)
    assert torch.isfinite(ko.float()).all()
    # q_proj output (1 GiB) + k_proj + outputs + a few MiB of workspaces; the reference's temporaries alone are ~ 10 GiB
    assert peak < 3 << 30, peak
