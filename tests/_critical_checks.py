"""CriticalKVPress / CriticalAdaKVPress against the reference's outputs (tests/golden/crit_*.npz): the check bodies shared by
tests/test_critical_host.py (CPU, oracle-backed entry points) and tests/test_gpu_critical.py (the HIP kernels)."""
import numpy as np
import torch

import _critical_inputs as CI
import _critical_oracle as CO
import _inputs
from _support import golden, kept_positions

FMAX = np.finfo(np.float32).max


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


def run_presses_against_fixture(name, dev, dtype=torch.float32):
    """both presses on the case's float32 module against the reference's outputs"""
    import kvpress_amd as P
    from kvpress_amd import _native
    from kvpress_amd.presses.criticalkv_press import CriticalAdaKVPress, CriticalKVPress

    s, g = CI.make_case(name), golden(name)
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
            pos = np.sort(kept_positions(ko, keys), -1)
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


def run_stage1_truncation(dev, monkeypatch):
    """CriticalAdaKVPress on scores built so that the head budgets are (90, 110), first_stage_ratio 0.7: stage 1 protects 63 entries of
    head 0 -- 90 * 0.7 as a float32 product is 63.0 (criticalkv_press.py:167: an int64 tensor times a Python float), as a Python float
    62.99999999999999, which truncates to 62."""
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
