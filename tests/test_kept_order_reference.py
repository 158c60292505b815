"""Reference-exact tensor mode: ``press.kept_order = "score"`` must reproduce the K' / V' TENSORS the reference's
``ScorerPress.compress`` returns (kvpress/presses/scorer_press.py:95-100: rows in `scores.topk(n_kept)` order, descending score).

Fixtures: tests/golden/order_*.npz, outputs of the REAL reference's compress() (oracle/gen_golden_order.py).  What "equal" can
mean is set by the reference itself: where two neighbouring kept scores are EQUAL (SnapKV's W window columns and
ExpectedAttention's sinks all hold the pad constant max + 1) torch.topk's order is unspecified, and where they differ by less than
an implementation's float32 score error the order is not defined either.  So the kept ranks are cut into runs at every gap
larger than the scorer's margin; inside a run the SET of rows must match, and every run of length one -- the general case --
must match the reference's tensor rows bit for bit.  Cases whose every gap exceeds the margin are compared with torch.equal on the
whole tensor.  The GPU test runs the kernels; the CPU test runs the same check through the oracle-backed stand-in (host logic)."""

import numpy as np
import pytest
import torch

import _inputs
from _support import golden

ORDER_CASES = ["kn_readme", "kn_tiny_d6", "kn_d96_bf16", "sk_257_A", "sk_257_B", "sk_f16_d64", "ea_257_A", "ea_nocov"]
# relative score margin below which the order of two neighbours is not considered defined (>= 4 x the measured kernel-vs-reference
# float32 score error of DESIGN.md §2: Knorm / SnapKV ~4e-7, ExpectedAttention < 1e-4)
MARGIN = {"knorm": 2e-6, "snapkv": 4e-6, "ea": 4e-4}
# ... when the press runs on a bf16 / f16 MODULE (as users run it) the window / all-token queries themselves differ from the
# float32 run's by the model's own rounding of q, cos and sin (3e-4 flat data, 4.5e-3 structured keys; bound 6e-3)
MARGIN_NATIVE = {"knorm": 2e-6, "snapkv": 1.2e-2, "ea": 1.2e-2}
WHOLE_TENSOR = {("kn_readme", 0), ("kn_readme", 1), ("kn_tiny_d6", 1), ("kn_tiny_d6", 2)}   # every gap of these exceeds the margin


def _press(P, s, ratio):
    if s["kind"] == "knorm":
        p = P.KnormPress(compression_ratio=ratio)
    elif s["kind"] == "snapkv":
        p = P.SnapKVPress(compression_ratio=ratio, window_size=s["W"], kernel_size=s["ks"])
    else:
        p = P.ExpectedAttentionPress(compression_ratio=ratio, n_future_positions=s["n_future"], n_sink=s["n_sink"],
                                     use_covariance=s["use_covariance"], use_vnorm=s["use_vnorm"], epsilon=s["epsilon"])
    p.kept_order = "score"
    return p


def _load_rows(fx, key, dt):
    a = fx[key]
    if a.dtype == np.uint16:
        return torch.from_numpy(a.view(np.int16).copy()).view(dt)
    return torch.from_numpy(a).to(dt)


def check_case(name, device, native, force_f32=False):
    import kvpress_amd as P

    s = _inputs.make_case(name)
    dt = torch.float32 if force_f32 else _inputs.torch_dtype(s["dtype"])   # (the numpy stand-in of the host test has no bf16)
    fx = golden(f"order_{name}")
    att, rot, hidden, pe = _inputs.build_llama_attention(s, dt, device)
    keys = torch.from_numpy(s["keys"]).to(device=device, dtype=dt)
    values = torch.from_numpy(s["values"]).to(device=device, dtype=dt)
    kwargs = {"position_embeddings": pe}
    margin = (MARGIN if dt == torch.float32 else MARGIN_NATIVE)[s["kind"]]
    stats = []
    for i, r in enumerate(fx["ratios"]):
        press = _press(P, s, float(r))
        with torch.no_grad():
            ko, vo = press.compress(att, hidden, keys, values, None, kwargs)
            sc = press.score(att, hidden, keys, values, None, kwargs)
        idx_ref = torch.from_numpy(fx[f"idx_{i}"]).long()
        val = torch.from_numpy(fx[f"val_{i}"]).double()
        case_dt = _inputs.torch_dtype(s["dtype"])
        ko_ref, vo_ref = _load_rows(fx, f"ko_{i}", case_dt).to(dt), _load_rows(fx, f"vo_{i}", case_dt).to(dt)
        B, H, n = idx_ref.shape
        assert tuple(ko.shape) == tuple(ko_ref.shape) == (B, H, n, s["D"]) and ko.dtype == dt and ko.is_contiguous()
        ours = native.topk_select(sc, n, native.ORDER_SCORE).long().cpu()
        e = ours.to(device).unsqueeze(-1).expand(-1, -1, -1, s["D"])
        assert torch.equal(ko, keys.gather(2, e)) and torch.equal(vo, values.gather(2, e)), "compress() must store the rows in ORDER_SCORE order"
        ko_c, vo_c = ko.cpu(), vo.cpu()
        # boundaries between rank j and j + 1 (j = n - 1: against the best dropped score)
        gap = (val[..., :-1] - val[..., 1:]) / val[..., :-1].abs().clamp_min(1e-300)
        cut = (gap > margin) | ~torch.isfinite(val[..., 1:])
        exact_rows = total_rows = 0
        for b in range(B):
            for h in range(H):
                c = cut[b, h]
                start = 0
                for j in range(n):
                    if not (c[j] or j == n - 1):
                        continue
                    run = slice(start, j + 1)
                    closed = bool(c[j])   # an open last run: which of its members is kept at all is within the margin
                    if closed:
                        assert set(ours[b, h, run].tolist()) == set(idx_ref[b, h, run].tolist()), (name, float(r), b, h, start, j)
                        if j + 1 - start == 1:
                            assert torch.equal(ko_c[b, h, j], ko_ref[b, h, j]) and torch.equal(vo_c[b, h, j], vo_ref[b, h, j])
                            exact_rows += 1
                    start = j + 1
                total_rows += n
        if (name, i) in WHOLE_TENSOR and (dt == torch.float32 or s["kind"] == "knorm"):
            assert torch.equal(ko_c, ko_ref) and torch.equal(vo_c, vo_ref), f"{name} ratio {r}: whole-tensor equality with the reference"
            assert exact_rows == total_rows
        stats.append((float(r), exact_rows, total_rows))
    return stats


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["float32", "native"])
@pytest.mark.parametrize("name", ORDER_CASES)
def test_kept_order_score_equals_reference_tensors_gpu(name, mode):
    """mode float32: module and tensors in float32, like the reference run that made the fixture (the tight margins);
    native: the case's own bf16 / f16 module and tensors (the kernels of the fast paths; the queries differ by the model's rounding)."""
    from kvpress_amd import _native

    stats = check_case(name, "cuda:0", _native, force_f32=(mode == "float32"))
    print(name, mode, [(r, f"{a}/{t} rows pinned bit for bit") for r, a, t in stats])
    assert any(a > 0 for _, a, _ in stats), stats


@pytest.mark.parametrize("name", ["kn_readme", "kn_tiny_d6", "sk_257_A", "ea_257_A"])
def test_kept_order_score_equals_reference_tensors_host(name, fake_native):
    """The same check on the CPU with the oracle-backed stand-in for the kernels: pins the press-level plumbing of kept_order
    (and this file's run logic) where no GPU exists."""
    stats = check_case(name, "cpu", fake_native, force_f32=True)
    assert any(a > 0 for _, a, _ in stats), stats


# ---- chains (round 6): ComposedPress / PrefillDecodingPress switch the earlier press to the reference's order by themselves -----------
CHAINS = {
    "chain_kn_stream": ("kn_tiny_d6", 0.25, lambda P, s: P.StreamingLLMPress(compression_ratio=0.5, n_sink=3)),
    "chain_kn_snap": ("sk_257_A", 0.25, lambda P, s: P.SnapKVPress(compression_ratio=0.5, window_size=s["W"], kernel_size=s["ks"])),
}


def _sorted_rows(t):
    """rows of [n, D] in lexicographic order (the data is random: rows are distinct)"""
    rows = [tuple(r) for r in t.double().tolist()]
    return sorted(rows)


def check_chain(cname, device, explicit_position=False):
    """p1.compress -> p2.compress the way composed_press.py:56-62 chains the hooks, against the REAL reference's final K' / V'
    (tests/golden/order_chain_*.npz, oracle/gen_golden_order.py chains).  Returns the number of (batch, head) rows whose kept SET equals
    the reference's."""
    import kvpress_amd as P

    case, r1, mk2 = CHAINS[cname]
    s = _inputs.make_case(case)
    fx = golden(f"order_{cname}")
    dt = torch.float32
    att, rot, hidden, pe = _inputs.build_llama_attention(s, dt, device)
    keys = torch.from_numpy(s["keys"]).to(device=device, dtype=dt)
    values = torch.from_numpy(s["values"]).to(device=device, dtype=dt)
    kwargs = {"position_embeddings": pe}
    p1, p2 = P.KnormPress(compression_ratio=r1), mk2(P, s)
    if explicit_position:
        p1.kept_order = "position"
    chain = P.ComposedPress([p1, p2])
    chain._check_kept_order()                      # what the chain's first hook call does
    assert p1.kept_order == ("position" if explicit_position else "score")
    with torch.no_grad():
        k1, v1 = p1.compress(att, hidden, keys, values, None, kwargs)
        k2, v2 = p2.compress(att, hidden, k1, v1, None, kwargs)
    case_dt = _inputs.torch_dtype(s["dtype"])
    ko_ref, vo_ref = _load_rows(fx, "ko", case_dt).to(dt), _load_rows(fx, "vo", case_dt).to(dt)
    assert tuple(k2.shape) == tuple(ko_ref.shape)
    k2, v2 = k2.cpu(), v2.cpu()
    same = 0
    B, H = k2.shape[:2]
    for b in range(B):
        for h in range(H):
            same += int(_sorted_rows(k2[b, h]) == _sorted_rows(ko_ref[b, h]) and _sorted_rows(v2[b, h]) == _sorted_rows(vo_ref[b, h]))
    return same, B * H, float(fx["gap2"].min())


@pytest.mark.parametrize("cname", list(CHAINS))
def test_chain_equals_reference_host(cname, fake_native):
    same, total, gap = check_chain(cname, "cpu")
    assert same == total, (cname, same, total, gap)


def test_chain_with_explicit_position_order_differs_from_reference_host(fake_native):
    """the control: pinned to position order, the sinks / recent tokens of the second stage are other tokens than the reference's"""
    same, total, _ = check_chain("chain_kn_stream", "cpu", explicit_position=True)
    assert same < total


@pytest.mark.gpu
@pytest.mark.parametrize("cname", list(CHAINS))
def test_chain_equals_reference_gpu(cname):
    same, total, gap = check_chain(cname, "cuda:0")
    assert same == total, (cname, same, total, gap)
