"""CriticalKVPress / CriticalAdaKVPress on the GPU: kvp_vwl1norm_rescale (matrix-core and generic path) and kvp_scores_fill_prefix against
the float64 oracle (tests/_critical_oracle.py), both presses against the REAL reference's outputs (tests/golden/crit_*.npz), the
per-element batch rule, determinism, the Llama-3.1-8B geometry at 128k tokens and a tiny model end to end."""
import numpy as np
import pytest
import torch

import _critical_inputs as CI
import _critical_oracle as CO
import _inputs
from _critical_checks import run_presses_against_fixture, run_stage1_truncation
from _support import torch_dtype

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FMAX = float(np.finfo(np.float32).max)


def make_inputs(S, D, hidden, G, Hkv, B, dtype, seed):
    """values [B,Hkv,S,D] and wo [hidden, Hq*D], exact in `dtype`, and float32 scores of both signs (Knorm's are negative)"""
    rs = np.random.RandomState(seed)
    v = _inputs.round_to(rs.standard_normal((B, Hkv, S, D)).astype(np.float32), dtype)
    wo = _inputs.round_to((rs.standard_normal((hidden, Hkv * G * D)) / np.sqrt(Hkv * G * D)).astype(np.float32), dtype)
    sc = (3.0 * rs.standard_normal((B, Hkv, S))).astype(np.float32)
    return v, wo, sc


# S, D, hidden, G, Hkv, B, dtype, mode -- every value of the issue's sweep at least once.  The Wo tile is 128 rows for D <= 128 and 64 rows
# for D = 256: hidden = 320 ends in a partial tile for D <= 128 only (320 = 5 * 64), so D = 256 has cases of its own, hidden = 328
# (a partial last tile) and 24 (less than one 32-row sub-tile), in both 16-bit dtypes; S = 63 / 257 / 1000 are no multiple of the
# 256- (D = 256: 128-) token tile; D = 16 and float32 take the generic kernel
SWEEP = [
    (1, 128, 128, 1, 1, 1, "bf16", "norm"),
    (63, 64, 320, 4, 2, 1, "f16", "rescale"),
    (257, 96, 320, 8, 1, 2, "bf16", "alias"),
    (1000, 128, 1024, 4, 2, 1, "bf16", "rescale"),
    (257, 256, 320, 1, 2, 2, "f16", "norm"),
    (1000, 16, 128, 4, 1, 1, "f32", "rescale"),
    (63, 16, 320, 8, 2, 2, "bf16", "alias"),
    (257, 128, 1024, 4, 1, 1, "f32", "norm"),
    (1000, 64, 1024, 8, 1, 2, "bf16", "norm"),
    (1000, 256, 128, 4, 2, 1, "bf16", "rescale"),
    (63, 96, 128, 1, 1, 1, "f16", "norm"),
    (257, 128, 320, 8, 2, 1, "f16", "alias"),
    (257, 256, 328, 4, 1, 1, "bf16", "norm"),
    (63, 256, 328, 1, 2, 1, "f16", "rescale"),
    (257, 256, 24, 4, 2, 1, "f16", "alias"),
    (63, 256, 24, 8, 1, 2, "bf16", "norm"),
    (63, 128, 24, 4, 1, 1, "bf16", "rescale"),
]


def run_kernel(v, wo, sc, Hq, mode, eps=1e-4):
    from kvpress_amd import _native

    if mode == "norm":
        return _native.vwl1norm(v, wo, Hq)
    if mode == "alias":      # out aliases scores_in
        s = sc.clone()
        out = _native.vwl1norm_rescale_(s, v, wo, Hq, eps)
        assert out.data_ptr() == s.data_ptr()
        return out
    # scores_in and out apart, through the C entry itself
    out = torch.full_like(sc, float("nan"))
    B, Hkv, S, D = v.shape
    _native._call("kvp_vwl1norm_rescale", *_native._tensor(v), _native._DTYPES[v.dtype], *_native._tensor(wo, 1), B, Hq, Hkv, S, D, wo.shape[0],
                  sc.data_ptr(), S, float(eps), out.data_ptr(), None, 0, _native._stream(v))
    return out


@pytest.mark.parametrize("S,D,hidden,G,Hkv,B,dtype,mode", SWEEP)
def test_vwl1norm_kernel_against_float64(S, D, hidden, G, Hkv, B, dtype, mode):
    """the section 2 contract: 1e-3 relative against float64 (the products of 16-bit inputs are exact in float32, so what is measured
    is the float32 accumulation: expected near 1e-6)"""
    v, wo, sc = make_inputs(S, D, hidden, G, Hkv, B, dtype, seed=S + D + hidden)
    ref = CO.vwl1norm(v, wo, Hkv * G)
    if mode != "norm":
        ref = (sc.astype(np.float64) + np.float64(np.float32(1e-4))) * ref
    got = run_kernel(torch.from_numpy(v).to(DEV, torch_dtype(dtype)), torch.from_numpy(wo).to(DEV, torch_dtype(dtype)), torch.from_numpy(sc).to(DEV), Hkv * G, mode)
    assert got.dtype == torch.float32 and tuple(got.shape) == (B, Hkv, S)
    got = got.cpu().numpy().astype(np.float64)
    ok = np.abs(sc + 1e-4) > 1e-3 if mode != "norm" else np.ones(ref.shape, bool)   # (away from the cancellation of scores + eps)
    err = (np.abs(got - ref) / np.abs(ref))[ok].max()
    print(f"vwl1norm S={S} D={D} hidden={hidden} G={G} Hkv={Hkv} B={B} {dtype} {mode}: worst relative error {err:.3g}")
    assert np.isfinite(got).all() and err <= 1e-3


@pytest.mark.parametrize("dtype,D", [("bf16", 128), ("f32", 16)])
def test_strided_inputs_give_the_same_bits(dtype, D):
    """values as a slice of a larger cache, wo as a row-strided view: bit-identical to the contiguous copies"""
    from kvpress_amd import _native

    S, hidden, G, Hkv, B = 300, 320, 4, 2, 2
    v, wo, _ = make_inputs(S, D, hidden, G, Hkv, B, dtype, seed=7)
    big = torch.zeros(B, Hkv, S + 24, D + 8, dtype=torch_dtype(dtype), device=DEV)
    big[:, :, 8:8 + S, :D] = torch.from_numpy(v).to(DEV, torch_dtype(dtype))
    vs = big[:, :, 8:8 + S, :D]
    wbig = torch.zeros(hidden, Hkv * G * D + 64, dtype=torch_dtype(dtype), device=DEV)
    wbig[:, :Hkv * G * D] = torch.from_numpy(wo).to(DEV, torch_dtype(dtype))
    ws = wbig[:, :Hkv * G * D]
    assert not vs.is_contiguous() and not ws.is_contiguous()
    ref = _native.vwl1norm(vs.contiguous(), ws.contiguous(), Hkv * G)
    assert torch.equal(_native.vwl1norm(vs, ws.contiguous(), Hkv * G), ref)
    assert torch.equal(_native.vwl1norm(vs.contiguous(), ws, Hkv * G), ref)
    assert (big[:, :, :8] == 0).all() and (big[..., D:] == 0).all()


@pytest.mark.parametrize("dtype,D", [("bf16", 64), ("f32", 16)])
def test_zero_value_row(dtype, D):
    """a zero value row has norm 0, and a protected (float32 max) entry there rescales to 0: it loses its protection, as in the reference"""
    from kvpress_amd import _native

    S, hidden, G, Hkv = 70, 128, 2, 2
    v, wo, sc = make_inputs(S, D, hidden, G, Hkv, 1, dtype, seed=3)
    v[0, 1, 7] = 0.0
    sc[0, 1, 7] = sc[0, 0, 9] = FMAX
    norm_ref = CO.vwl1norm(v, wo, Hkv * G)
    vt, wt = torch.from_numpy(v).to(DEV, torch_dtype(dtype)), torch.from_numpy(wo).to(DEV, torch_dtype(dtype))
    norm = _native.vwl1norm(vt, wt, Hkv * G).cpu().numpy()
    assert norm[0, 1, 7] == 0.0 and (np.delete(norm.ravel(), S + 7) > 0).all()
    out = _native.vwl1norm_rescale_(torch.from_numpy(sc).to(DEV), vt, wt, Hkv * G, 1e-4).cpu().numpy()
    ref = CO.rescale(sc, norm_ref, 1e-4)
    assert out[0, 1, 7] == 0.0 == ref[0, 1, 7]
    assert np.isinf(ref[0, 0, 9]) == np.isinf(out[0, 0, 9]) and (np.isinf(out[0, 0, 9]) or abs(out[0, 0, 9] / ref[0, 0, 9] - 1) < 1e-3)


def test_scores_fill_prefix():
    from kvpress_amd import _native

    R, S, n = 5, 300, 40
    g = torch.Generator().manual_seed(1)
    scores = torch.randn(R, S, generator=g)
    idx = torch.stack([torch.randperm(S, generator=g)[:n] for _ in range(R)]).to(torch.int32)
    counts = torch.tensor([0, n, 7, 1, 39], dtype=torch.int32)
    want = scores.clone()
    for r in range(R):
        want[r, idx[r, :counts[r]].long()] = FMAX
    got = _native.scores_fill_prefix_(scores.clone().to(DEV), idx.to(DEV), counts.to(DEV), FMAX).cpu()
    assert torch.equal(got.view(torch.int32), want.view(torch.int32))    # entries outside the prefixes keep their bits
    got3 = _native.scores_fill_prefix_(scores.clone().view(1, R, S).to(DEV), idx.view(1, R, n).to(DEV), counts.view(1, R).to(DEV), FMAX).cpu()
    assert torch.equal(got3.view(R, S), want)
    assert torch.equal(_native.scores_fill_prefix_(scores.clone().to(DEV), idx[:, :0].to(DEV), counts.to(DEV) * 0, 1.0).cpu(), scores)


@pytest.mark.parametrize("name", list(CI.CASES))
def test_presses_match_reference_f32_module(name):
    run_presses_against_fixture(name, DEV)


def _native_inner_scores(s, press, att, hidden, pe):
    """the wrapped press's scores on the 16-bit module as the oracle gives them from the same rounded inputs (SnapKV: from the window
    queries the module produced, rounded to the dtype)"""
    from oracle import kvpress_oracle as O

    if s["kind"] == "knorm":
        return O.knorm_score(s["keys"])
    q = press.compute_window_queries(att, hidden, s["W"], pe)
    return O.snapkv_score(q.float().cpu().numpy(), s["keys"], s["ks"])


@pytest.mark.parametrize("name", list(CI.CASES))
def test_native_16bit_module_against_oracle(name):
    """the case's 16-bit module: float32 norm, CriticalKV scores (1e-3) and CriticalAdaKV budgets and masks against the oracle on the same
    rounded inputs"""
    import kvpress_amd as P
    from kvpress_amd.presses.criticalkv_press import CriticalKVPress

    s = CI.make_case(name)
    dt = torch_dtype(s["dtype"])
    att, _, hidden, pe = _inputs.build_llama_attention(s, dt, DEV)
    att.config._attn_implementation = "sdpa"
    keys, values = torch.from_numpy(s["keys"]).to(DEV, dt), torch.from_numpy(s["values"]).to(DEV, dt)
    kw = {"position_embeddings": pe}
    norm_ref = CO.vwl1norm(s["values"], CI.wo_of(att), s["Hq"])
    S, H = s["S"], s["H"]
    with torch.no_grad():
        norm = CriticalKVPress.vwl1norm(values, att)
        assert norm.dtype == torch.float32
        assert (np.abs(norm.cpu().numpy() - norm_ref) / norm_ref).max() <= 1e-3
        for r in s["ratios"]:
            inner_press = CI.inner_press(P, s, r)
            inner = _native_inner_scores(s, inner_press, att, hidden, pe)
            sc = CriticalKVPress(inner_press, epsilon=CI.EPSILON, first_stage_ratio=s["fsr"]).score(att, hidden, keys, values, None, kw)
            assert sc.dtype == torch.float32
            sc = sc.cpu().numpy()
            ref, band = CO.critical_scores(inner, norm_ref, r, s["fsr"], CI.EPSILON)
            free = ~band
            assert np.array_equal((sc == FMAX) & free, (ref == FMAX) & free)
            m = free & np.isfinite(ref) & (ref != FMAX) & (np.abs(inner + CI.EPSILON) > 1e-2 * np.abs(inner))   # (no cancellation in scores + eps)
            err = (np.abs(sc[m] - ref[m]) / np.abs(ref[m])).max()
            print(f"{name} r={r}: CriticalKV scores on the {s['dtype']} module vs the oracle: worst {err:.3g} relative")
            assert err <= 1e-3

            a = CO.critical_ada(inner, norm_ref, r, s["alpha"], s["fsr"], CI.EPSILON)
            ada = P.CriticalAdaKVPress(inner_press, alpha_safeguard=s["alpha"], epsilon=CI.EPSILON, first_stage_ratio=s["fsr"])
            ada.compress(att, hidden, keys, values, None, kw)
            _, hi, si = att.masked_key_indices
            flat = (hi * S + si).cpu().numpy()
            n_kept = int(S * (1 - r))
            assert flat.size == H * (S - n_kept) == len(set(flat.tolist()))
            # budgets: kept entries per head.  They are the oracle's unless other scores lie within the band of the flattened budget
            # threshold; each such score can move one unit of budget between two heads
            budgets = S - np.bincount(flat // S, minlength=H)
            moved = int(np.abs(budgets - a["budgets"][0]).sum())
            assert moved <= 2 * (a["budget_band"] - 1), (budgets, a["budgets"][0], a["budget_band"])
            free = ~a["band"][0].ravel()
            differ = set(flat[free[flat]].tolist()) ^ set(a["masked"][0][free[a["masked"][0]]].tolist())
            assert len(differ) <= 2 * moved, f"{name} r={r}: {len(differ)} masked positions differ outside the bands (budgets moved by {moved})"


def test_stage1_budgets_are_truncated_from_a_float32_product_gpu(monkeypatch):
    run_stage1_truncation(DEV, monkeypatch)


def _ada_flat(press, att, hidden, keys, values, pe, S):
    press.compress(att, hidden, keys, values, None, {"position_embeddings": pe})
    bi, hi, si = att.masked_key_indices
    return [(hi[bi == b] * S + si[bi == b]).tolist() for b in range(keys.shape[0])]


def test_ada_batch_of_two_equals_the_elements_alone():
    """the defined deviation: budgets per batch element; matrix-core path (bf16, D = 64)"""
    import kvpress_amd as P

    s = CI.make_case("crit_knorm_s300_d64_g4")
    att, _, hidden, pe = _inputs.build_llama_attention(s, torch.bfloat16, DEV)
    att.config._attn_implementation = "sdpa"
    rs = np.random.RandomState(5)
    keys = torch.from_numpy(np.concatenate([s["keys"], 3.0 * rs.standard_normal(s["keys"].shape).astype(np.float32)])).to(DEV, torch.bfloat16)
    values = torch.from_numpy(np.concatenate([s["values"], rs.standard_normal(s["values"].shape).astype(np.float32)])).to(DEV, torch.bfloat16)
    press = P.CriticalAdaKVPress(P.KnormPress(0.5), alpha_safeguard=0.2, first_stage_ratio=0.3)
    with torch.no_grad():
        both = _ada_flat(press, att, hidden.expand(2, -1, -1), keys, values, pe, s["S"])
        for b in range(2):
            assert _ada_flat(press, att, hidden, keys[b:b + 1], values[b:b + 1], pe, s["S"])[0] == both[b]
    assert both[0] != both[1] and len(both[0]) == s["H"] * (s["S"] - int(s["S"] * 0.5))


def test_two_runs_are_bit_identical():
    import kvpress_amd as P
    from kvpress_amd import _native

    v, wo, sc = make_inputs(1000, 128, 1024, 4, 2, 2, "bf16", seed=11)
    vt, wt = torch.from_numpy(v).to(DEV, torch.bfloat16), torch.from_numpy(wo).to(DEV, torch.bfloat16)
    a, b = _native.vwl1norm(vt, wt, 8), _native.vwl1norm(vt, wt, 8)
    assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    s = CI.make_case("crit_knorm_s300_d64_g4")
    att, _, hidden, pe = _inputs.build_llama_attention(s, torch.bfloat16, DEV)
    att.config._attn_implementation = "sdpa"
    keys, values = torch.from_numpy(s["keys"]).to(DEV, torch.bfloat16), torch.from_numpy(s["values"]).to(DEV, torch.bfloat16)
    press = P.CriticalAdaKVPress(P.KnormPress(0.4))
    with torch.no_grad():
        assert _ada_flat(press, att, hidden, keys, values, pe, s["S"]) == _ada_flat(press, att, hidden, keys, values, pe, s["S"])


def test_llama8b_geometry_128k():
    """B 1, Hq 32, Hkv 8, D 128, hidden 4096, bf16, S = 131072: completes, allocates less than 64 MiB beyond inputs and output (the
    reference's per-head temporary is 1 GiB), and 256 sampled tokens match a float64 evaluation to 1e-3"""
    from kvpress_amd import _native

    S, Hq, Hkv, D, hidden = 131072, 32, 8, 128, 4096
    g = torch.Generator(DEV).manual_seed(0)
    values = torch.randn(1, Hkv, S, D, device=DEV, dtype=torch.bfloat16, generator=g)
    wo = (torch.randn(hidden, Hq * D, device=DEV, generator=g) / 64).to(torch.bfloat16)
    scores = torch.randn(1, Hkv, S, device=DEV, generator=g)
    sc0 = scores.clone()
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    out = _native.vwl1norm_rescale_(scores, values, wo, Hq, 1e-4)
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    assert peak < 64 << 20, peak
    assert torch.isfinite(out).all()
    tok = torch.randint(0, S, (256,), device=DEV, generator=g)
    tok[:2] = torch.tensor([0, S - 1], device=DEV)
    w64 = wo.double().view(hidden, Hq, D)
    G = Hq // Hkv
    worst = 0.0
    for k in range(Hkv):
        v64 = values[0, k, tok].double()                                             # [256, D]
        norm = torch.einsum("td,cgd->tgc", v64, w64[:, k * G:(k + 1) * G]).abs().sum((1, 2)) / G
        ref = (sc0[0, k, tok].double() + float(np.float32(1e-4))) * norm
        ok = (sc0[0, k, tok] + 1e-4).abs() > 1e-3
        worst = max(worst, float(((out[0, k, tok].double() - ref).abs() / ref.abs())[ok].max()))
    print(f"128k Llama-3.1-8B geometry: worst relative error of 256 sampled tokens x 8 heads {worst:.3g}")
    assert worst <= 1e-3


def test_tiny_llama_end_to_end():
    """a tiny Llama under `with CriticalAdaKVPress(SnapKVPress(0.5))(model)` generates; every layer carries H * (S - n_kept) masked triples"""
    import kvpress_amd as P
    from transformers import DynamicCache

    model = _inputs.make_tiny_llama(seed=0, device=DEV)
    press = P.CriticalAdaKVPress(P.SnapKVPress(0.5, window_size=8, kernel_size=5))
    S = 60
    ids = torch.randint(3, 64, (1, S), device=DEV, generator=torch.Generator(DEV).manual_seed(0))
    with torch.no_grad(), press(model):
        cache = DynamicCache()
        nxt = model(ids, past_key_values=cache).logits[:, -1].argmax(-1, keepdim=True)
        H = model.config.num_key_value_heads
        for layer in model.model.layers:
            bi, hi, si = layer.self_attn.masked_key_indices
            assert bi.numel() == hi.numel() == si.numel() == H * (S - int(S * 0.5))
            assert int(si.max()) < S and int(hi.max()) < H
        assert all(layer.keys.shape[2] == S for layer in cache.layers)      # nothing leaves the cache: the pruned keys are masked
        new = []
        for _ in range(4):                                                  # greedy decoding over the masked cache
            logits = model(nxt, past_key_values=cache).logits[:, -1]
            assert torch.isfinite(logits).all()
            nxt = logits.argmax(-1, keepdim=True)
            new.append(int(nxt))
    assert len(new) == 4 and cache.get_seq_length() == S + 4
