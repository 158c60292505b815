"""FastKVzipPress without a GPU: the package surface and the classes next to the reference's (kvpress/presses/fastkvzip_press.py), the
argument checks of the new C-ABI entry, the float64 oracle (tests/_fastkvzip_oracle.py) against the REAL reference's outputs
(tests/golden/fastkvzip_flow_*.npz, oracle/gen_golden_fastkvzip.py), the sensitivity of the exact-input case the GPU test uses, and the
press's host logic with ``_native.fastkvzip_score`` replaced by the oracle."""
import dataclasses

import numpy as np
import pytest
import torch

import _fastkvzip_checks as FC
import _fastkvzip_inputs as FI
import _fastkvzip_oracle as FO
import _inputs
from _support import golden


@pytest.fixture(scope="module")
def lib():
    from kvpress_amd import build as B

    B.build()
    from kvpress_amd import _native

    return _native.lib()


# ---- surface --------------------------------------------------------------------------------------------------------------------------
def test_package_surface():
    import kvpress_amd as P
    from kvpress_amd import FastKVzipPress
    from kvpress_amd.presses import fastkvzip_press

    assert "FastKVzipPress" in P.__all__ and "FastKVzipPress" not in P._NOT_BUILT and FastKVzipPress is fastkvzip_press.FastKVzipPress
    assert issubclass(FastKVzipPress, P.BasePress) and not issubclass(FastKVzipPress, P.ScorerPress)
    for name in ("FastKVzipGate", "load_fastkvzip", "get_gate_id", "get_gate_weight"):
        assert hasattr(fastkvzip_press, name)


def test_fields_and_defaults_are_the_references():
    """fastkvzip_press.py:160-168"""
    from kvpress_amd import FastKVzipPress

    fields = {f.name: f for f in dataclasses.fields(FastKVzipPress)}
    assert list(fields) == ["compression_ratio", "layerwise", "n_sink", "window_size", "window_ratio", "gates", "score_val"]
    assert [fields[n].default for n in fields] == [0.0, False, 4, 4096, 0.02, None, None]
    assert not fields["gates"].init and not fields["score_val"].init
    press = FastKVzipPress(0.3, True)
    assert (press.compression_ratio, press.layerwise, press.gates, press.score_val) == (0.3, True, None, None)


def test_gate_has_the_references_state_dict():
    """fastkvzip_press.py:28-50: keys, shapes and dtypes (projections and b in the gate's dtype, norm weights and k_base float32); the
    fixture's state dict loads with strict=True"""
    from kvpress_amd.presses.fastkvzip_press import FastKVzipGate

    gate = FastKVzipGate(3, 24, 2, 4, torch.bfloat16)
    sd = gate.state_dict()
    assert sorted(sd) == sorted(FI.GATE_KEYS)
    assert {k: (tuple(v.shape), v.dtype) for k, v in sd.items()} == {
        "q_proj.weight": ((128, 24), torch.bfloat16), "q_proj.bias": ((128,), torch.bfloat16), "k_proj.weight": ((32, 24), torch.bfloat16),
        "q_norm.weight": ((16,), torch.float32), "k_norm.weight": ((16,), torch.float32), "k_base": ((2, 1, 16, 16), torch.float32),
        "b": ((2, 1, 4), torch.bfloat16)}
    assert (gate.index, gate.output_dim, gate.nhead, gate.ngroup, gate.sink, gate.d, gate.q_norm.variance_epsilon) == (3, 16, 2, 4, 16, 4.0, 1e-6)
    assert bool((sd["q_norm.weight"] == 1).all()) and bool((sd["k_base"] == 0).all()) and bool((sd["b"] == 0).all())
    with pytest.raises(NotImplementedError):
        gate(torch.zeros(1, 3, 24))
    g = golden("fastkvzip_flow_120_r02")
    gates = FI.load_gates(g, _inputs.make_tiny_llama(dtype=torch.float32).config)           # strict=True inside
    assert len(gates) == 2 and np.array_equal(gates[1].k_base.detach().numpy(), g["gate1/k_base"])


def test_no_hub_access_when_gates_are_assigned(monkeypatch):
    """fastkvzip_press.py:174: the gates are loaded only when there are none; the loader's name and its hub call are the reference's"""
    import huggingface_hub

    from kvpress_amd.presses import fastkvzip_press as M

    asked = []
    monkeypatch.setattr(huggingface_hub, "hf_hub_download", lambda **kw: asked.append(kw) or (_ for _ in ()).throw(OSError("no network")))
    monkeypatch.setattr(M, "get_gate_id", lambda model_name: "qwen3-8b/q4_dim16_sink16.pt")
    model = _inputs.make_tiny_llama(dtype=torch.float32)
    press = M.FastKVzipPress(0.5)
    sentinel = press.gates = [object(), object()]
    press.post_init_from_model(model)
    assert press.gates is sentinel and asked == []
    press.gates = None
    model.config.name_or_path = "Qwen/Qwen3-8B"
    with pytest.raises(RuntimeError, match="no published FastKVzip gates"):
        press.post_init_from_model(model)
    assert asked == [dict(repo_id="Jang-Hyun/Fast-KVzip", filename="qwen3-8b/q4_dim16_sink16.pt", repo_type="model")]


# ---- C ABI ----------------------------------------------------------------------------------------------------------------------------
P0 = 1 << 12     # a well-aligned non-null address that is never dereferenced: every check below fails before a launch


def test_capi_argument_errors_come_before_any_hip_call(lib):
    def score(dtype=2, B=1, S=4, K=32, Hkv=2, G=2, D=16, J=4, eps=1e-6, head=0, tail=0, x=P0, wq=P0, bq=P0, wk=P0, b=P0, gq=P0, gk=P0, kb=P0, out=P0):
        return lib.kvp_fastkvzip_score(x, 0, 0, dtype, wq, bq, wk, b, gq, gk, kb, B, S, K, Hkv, G, D, J, eps, head, tail, out, 0, 0, 0, None, 0, None)

    assert score(dtype=7) == -1 and b"bad dtype" in lib.kvp_last_error()
    for kw in (dict(D=0), dict(D=65), dict(D=-16)):
        assert score(**kw) == -1 and b"bad output_dim" in lib.kvp_last_error(), kw
    for kw in (dict(B=0), dict(S=-1), dict(K=0), dict(Hkv=0), dict(G=0), dict(J=-1), dict(S=1 << 31), dict(G=512, D=64)):
        assert score(**kw) == -1 and b"bad shape" in lib.kvp_last_error(), kw
    for kw in (dict(head=-1), dict(tail=-1)):
        assert score(**kw) == -1 and b"bad protected counts" in lib.kvp_last_error(), kw
    assert score(eps=-1.0) == -1 and b"bad eps" in lib.kvp_last_error()
    for name in ("x", "wq", "bq", "wk", "b", "gq", "gk", "out"):
        assert score(**{name: None}) == -1 and b"null pointer" in lib.kvp_last_error(), name
    assert score(kb=None) == -1 and b"k_base" in lib.kvp_last_error()
    assert score(S=0, x=None, out=None) == 0                                                              # nothing to do


def test_workspace_holds_nothing_of_extent_s_times_columns(lib):
    """Qwen3-8B, 128k tokens: the reference's logit_base [Hkv, S, 16, G] alone is 268 MB in float32; here every path keeps its
    intermediates in its workgroups' LDS"""
    assert lib.kvp_fastkvzip_score_workspace_bytes(2, 1, 131072, 4096, 8, 4, 16, 16) < 4 << 20
    assert lib.kvp_fastkvzip_score_workspace_bytes(0, 2, 1, 24, 2, 2, 16, 16) < 4 << 20


def test_no_cpu_fallback():
    from kvpress_amd import _native
    from kvpress_amd._native import KvpressHipError

    s = FI.score_case(("f32", 1, 3, 24, 2, 2, 4))
    t = {n: torch.from_numpy(np.asarray(s[n])) for n in ("x", "wq", "bq", "wk", "b", "gq", "gk", "kb")}
    with pytest.raises(KvpressHipError):
        _native.fastkvzip_score(t["x"], t["wq"], t["bq"], t["wk"], t["b"], t["gq"], t["gk"], t["kb"], FI.EPS)


# ---- the oracle -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(FI.FLOW))
def test_oracle_matches_the_references_scores_and_selection(name):
    """the float64 oracle on the hidden states the reference's gates received against the float32 score_val the reference stacked: inside
    2 x bound, protected positions exactly 1.0; and the selection from the oracle's scores leaves the reference's masked sets (the
    fixture's boundary gaps are 10 x the contract bound -- asserted here again, from the oracle's side)"""
    spec, g = FI.FLOW[name], golden(name)
    head, tail = FO.protected_counts(spec["tokens"])
    ours, worst, bmax = [], 0.0, 0.0
    for l in range(2):
        ref, bound = FO.fastkvzip_score(g[f"hidden_{l}"], *FI.gate_arrays(g, l), FI.EPS)
        ours.append(FO.protect(ref, head, tail))
        worst, bmax = max(worst, FO.worst_ratio(g["score_val"][l], ours[l], bound)), max(bmax, float(bound.max()))
        assert np.array_equal(g["score_val"][l] == 1.0, ours[l] == 1.0)
    print(f"{name}: the reference's float32 scores vs the oracle: worst {worst:.3g} of 2 x bound (largest bound {bmax:.3g})")
    assert worst <= 1.0
    ours = np.stack(ours)
    if spec["tokens"] < 50:
        assert (ours == 1.0).all() and (g["score_val"] == 1.0).all() and int(g["n_pruned"].sum()) == int(ours.size * spec["compression_ratio"])
        return
    assert min(FO.boundary_gaps(ours, spec["compression_ratio"], spec["layerwise"])) >= 10 * 2 * bmax
    sets, n_pruned = FO.compress_post(ours, spec["compression_ratio"], spec["layerwise"])
    assert n_pruned == g["n_pruned"].tolist()
    for l in range(2):
        assert sets[l] == FC.triples_set(g[f"masked_{l}"]), (name, l)
    assert (ours == 1.0).sum() == 2 * 2 * (head + tail) and not any(p < head or p >= spec["tokens"] - tail for s in sets for _, _, p in s)


def test_restatement_against_plain_torch():
    """the oracle against the lines of fastkvzip_press.py:54-71 written out in float64 torch, B = 2, odd sizes"""
    s = FI.score_case(("f32", 2, 11, 40, 3, 5, 7, 8))
    x, wq, bq, wk, b, gq, gk, kb = (torch.from_numpy(np.asarray(s[n], np.float64)) for n in ("x", "wq", "bq", "wk", "b", "gq", "gk", "kb"))

    def norm(v, g):
        return g * v * torch.rsqrt(v.pow(2).mean(-1, keepdim=True) + s["eps"])

    for i in range(2):
        q = norm((x[i] @ wq.T + bq).view(11, 3, 5, 8), gq).transpose(0, 1).transpose(-1, -2)      # head x seq x dim x group
        k = norm((x[i] @ wk.T).view(11, 3, 1, 8), gk).transpose(0, 1)                              # head x seq x 1 x dim
        logit = torch.matmul(k, q) / np.sqrt(8.0) + b[:, None, None, :]
        base = torch.matmul(kb[:, None], q) / np.sqrt(8.0)
        want = (1 / (1 + torch.exp(base - logit).sum(2, keepdim=True))).mean(-1).squeeze(-1)
        got, bound = FO.fastkvzip_score(*FI.oracle_args(s))
        assert np.allclose(got[i], want.numpy(), rtol=0, atol=1e-14) and (bound > 0).all()
    assert (FO.fastkvzip_score(*FI.oracle_args(FI.score_case(("f32", 1, 3, 24, 2, 2, 0))))[0] == 1.0).all()      # J = 0


EXACT_CASE = ("bf16", 1, FI.TILE + 1, 4096, 8, 4, 16)


def _moved(s, args, ref, tol, proj, t, row, k, factor):
    """max over the scores of |score with the perturbed product(s) - score| / tolerance"""
    return float((np.abs(FO.fastkvzip_score(*args, k_term=False, **{f"perturb_{proj}": (0, t, row, k, factor)})[0] - ref) / tol).max())


def test_exact_input_case_is_sensitive_to_a_lost_or_doubled_element():
    """The GPU test compares exact-input cases at the bound WITHOUT its K term.  Here the oracle drops or doubles element k of the
    reduction -- in one weight row for every token (a fragment of a weight row lost), and in one token's row for every weight row (a
    fragment of a token row lost) -- and some score must move by more than 10 x that tolerance, at the largest K, where one element weighs
    least.  Sampled: 6 random k plus the edges of the 16-byte chunks, k-steps and K tiles, each with a random row / token."""
    s = FI.exact_case(EXACT_CASE)
    for name in ("x", "wq", "wk"):
        assert set(np.unique(np.abs(s[name]))) == {1.0, 2.0}
    assert np.array_equal(s["bq"], np.round(s["bq"])) and np.abs(s["bq"]).max() <= 3
    args = FI.oracle_args(s)
    ref, bound = FO.fastkvzip_score(*args, k_term=False)
    tol = 2 * bound
    assert tol.max() < 1e-5
    rs = np.random.RandomState(5)
    S, K, H, G = s["S"], s["K"], s["Hkv"], s["G"]
    ks = sorted(set(rs.randint(K, size=6).tolist() + [0, 7, 8, 16, 63, 64, K - 65, K - 1]))
    every = slice(None)
    worst = np.inf
    for proj, rows in (("q", H * G * 16), ("k", H * 16)):
        for k in ks:
            for factor in (0.0, 2.0):
                worst = min(worst, _moved(s, args, ref, tol, proj, every, rs.randint(rows), k, factor),
                            _moved(s, args, ref, tol, proj, rs.randint(S), every, k, factor))
    print(f"exact case {EXACT_CASE}: a lost or doubled element of a row moves some score by at least {worst:.3g} x the tolerance")
    assert worst > 10.0


# (case, products sampled per projection, the share of them that must move their score by more than 10 x the tolerance)
SINGLE_PRODUCT = [(("bf16", 1, FI.TILE + 1, 32, 8, 4, 16), 100, 0.9), (("f16", 1, 2 * FI.TILE + 3, 96, 8, 8, 16), 100, 0.5), (EXACT_CASE, 30, 0.5)]


@pytest.mark.parametrize("case,n,share", SINGLE_PRODUCT, ids=lambda v: FI.case_id(v) if isinstance(v, tuple) else str(v))
def test_exact_input_cases_are_sensitive_to_a_single_product(case, n, share):
    """A SINGLE dropped or doubled product (one token, one row, one k) reaches exactly one score: the projected value moves by 1 .. 4, the
    RMSNorm divides it by r ~ 2.5 sqrt(K) (14 at K 32, 160 at K 4096) and keeps only its part orthogonal to the vector, and the score's
    derivative s (1 - s) / (4 G) times the matching element of the other vector can be arbitrarily small for a particular (token, row): NO
    gate gives EVERY single product 10 x the tolerance (the smallest seen is 0.1 x), so "any" is asserted as a stated share of a seeded
    sample instead.  At K 32, where one product weighs most, at least 9 in 10 must move their score by more than 10 x the tolerance
    (measured 0.98, median 350 x); at K 96 with G 8 and at K 4096 the median must (measured shares 0.87 and 0.77, medians 115 x and 31 x
    -- the 1 / sqrt(K) of r: 350 sqrt(32 / 4096) = 31).  With at least 129 x 640 products in a case, a kernel that loses products at
    even a few positions is seen at most of them; what a single stray product can hide under is stated, not assumed away."""
    s = FI.exact_case(case)
    args = FI.oracle_args(s)
    ref, bound = FO.fastkvzip_score(*args, k_term=False)
    tol = 2 * bound
    rs = np.random.RandomState(5)
    single = []
    for proj, rows in (("q", s["Hkv"] * s["G"] * 16), ("k", s["Hkv"] * 16)):
        for _ in range(n):
            t, row, k = rs.randint(s["S"]), rs.randint(rows), rs.randint(s["K"])
            single += [_moved(s, args, ref, tol, proj, t, row, k, factor) for factor in (0.0, 2.0)]
    single = np.array(single)
    got = float((single > 10.0).mean())
    print(f"exact case {FI.case_id(case)}: a single product moves its score by {single.min():.3g} .. {single.max():.3g} x the tolerance "
          f"(median {np.median(single):.3g}); {got:.3f} of {single.size} by more than 10 x (required: {share})")
    assert got >= share


# ---- the press's host logic over an oracle-backed entry point -----------------------------------------------------------------------------
@pytest.fixture
def fake_fastkvzip(fake_native, monkeypatch):
    calls = []

    def fastkvzip_score(hidden_states, wq, bq, wk, b, gq, gk, k_base, eps, protect_head=0, protect_tail=0, out=None):
        for t in (wq, bq, wk, b):
            assert t.dtype == hidden_states.dtype and t.is_contiguous()
        for t in (gq, gk, k_base):
            assert t.dtype == torch.float32 and t.is_contiguous()
        assert k_base.dim() == 3 and b.dim() == 2
        arrays = [t.detach().double().numpy() for t in (hidden_states, wq, bq, wk, b, gq, gk, k_base)]
        res = torch.from_numpy(FO.protect(FO.fastkvzip_score(*arrays, eps)[0], protect_head, protect_tail).astype(np.float32))
        calls.append((tuple(hidden_states.shape), protect_head, protect_tail, None if out is None else tuple(out.shape)))
        if out is None:
            return res
        out.copy_(res)
        return out

    monkeypatch.setattr(fake_native, "fastkvzip_score", fastkvzip_score)
    fake_native.fastkvzip_calls = calls
    yield fake_native
    del fake_native.fastkvzip_calls


@pytest.mark.parametrize("name", list(FI.FLOW))
def test_press_host_logic_matches_reference(name, fake_fastkvzip):
    rec = FC.check_flow_against_fixture(name, "cpu")
    n = rec["spec"]["tokens"]
    head, tail = FO.protected_counts(n)
    # one call per layer, straight into the layer's slice of the table; the gates' tensors packed once per layer
    assert fake_fastkvzip.fastkvzip_calls == [((1, n, 24), head, tail, (1, 2, n))] * 2
    assert len(rec["press"]._packed_layers) == 2 and rec["press"].score_val.shape == (2, 1, 2, n)


def test_a_batch_of_two_and_a_second_prefill(fake_fastkvzip):
    """B = 2 (the reference's gate cannot): one row per batch element, equal to the two single runs; decoding steps are not scored; the
    table is allocated anew by the next prefill"""
    from transformers import DynamicCache

    from kvpress_amd import FastKVzipPress

    g = golden("fastkvzip_flow_56_r02")
    model = _inputs.make_tiny_llama(dtype=torch.float32)
    press = FastKVzipPress(compression_ratio=0.25)
    press.gates = FI.load_gates(g, model.config)
    ids = torch.cat([torch.from_numpy(g["ids"]), torch.from_numpy(FI.flow_ids(99, 56))])
    cache = DynamicCache()
    with torch.no_grad(), press(model):
        model.model(input_ids=ids, past_key_values=cache)
        model.model(input_ids=ids[:, :1], past_key_values=cache)            # a decoding step inside the context: passes through
    assert len(fake_fastkvzip.fastkvzip_calls) == 2 and press.score_val.shape == (2, 2, 2, 56)
    assert np.abs(press.score_val[:, :1].numpy() - g["score_val"]).max() < 1e-5
    for layer in model.model.layers:
        bi, hi, si = layer.self_attn.masked_key_indices
        assert bi.tolist() == [0] * (len(bi) // 2) + [1] * (len(bi) // 2) and int(si.min()) >= 4 and int(si.max()) < 55
    first = press.score_val
    with torch.no_grad(), press(model):
        model.model(input_ids=ids[:1, :50], past_key_values=DynamicCache())
    assert press.score_val is not first and press.score_val.shape == (2, 1, 2, 50)


def test_ratio_zero_masks_nothing(fake_fastkvzip):
    from transformers import DynamicCache

    from kvpress_amd import FastKVzipPress

    g = golden("fastkvzip_flow_56_r02")
    model = _inputs.make_tiny_llama(dtype=torch.float32)
    for layer in model.model.layers:
        layer.self_attn.masked_key_indices = None
    press = FastKVzipPress()
    press.gates = FI.load_gates(g, model.config)
    with torch.no_grad(), press(model):
        model.model(input_ids=torch.from_numpy(g["ids"]), past_key_values=DynamicCache())
    assert press.score_val.shape == (2, 1, 2, 56) and all(layer.self_attn.masked_key_indices is None for layer in model.model.layers)
