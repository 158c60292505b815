"""KVzapPress and DMSPress without a GPU: the package surface and the classes next to the reference's (kvpress/presses/kvzap_press.py,
dms_press.py), the argument checks of the new C-ABI entries, the float64 oracle (tests/_kvzap_oracle.py) against the REAL reference's
outputs (tests/golden/kvzap_*.npz, oracle/gen_golden_kvzap.py), and the presses' host logic with ``_native.kvzap_score`` /
``_native.threshold_select`` replaced by the oracle."""
import ctypes
import dataclasses
from contextlib import contextmanager
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import _inputs
import _kvzap_checks as ZC
import _kvzap_inputs as ZI
import _kvzap_oracle as ZO
from _support import golden, tiny_pipeline


@pytest.fixture(scope="module")
def lib():
    from kvpress_amd import build as B

    B.build()
    from kvpress_amd import _native

    return _native.lib()


# ---- surface --------------------------------------------------------------------------------------------------------------------------
def test_package_surface():
    import kvpress_amd as P
    from kvpress_amd.presses import dms_press, kvzap_press

    assert "KVzapPress" in P.__all__ and "KVzapPress" not in P._NOT_BUILT and P.KVzapPress is kvzap_press.KVzapPress
    assert issubclass(P.KVzapPress, P.ScorerPress)
    assert "DMSPress" not in P.__all__
    with pytest.raises(AttributeError, match="outside the hot-path scope") as e:
        P.DMSPress
    assert "kvpress_amd.presses.dms_press.DMSPress" in str(e.value)
    assert issubclass(dms_press.DMSPress, P.BasePress) and not issubclass(dms_press.DMSPress, P.ScorerPress)


def test_fields_and_defaults_are_the_references():
    """kvzap_press.py:61-62 and dms_press.py:48-53, :58-67"""
    import kvpress_amd as P
    from kvpress_amd.presses.dms_press import DMSPress
    from kvpress_amd.presses.kvzap_press import KVzapConfig, KVzapModel, KVzapPress

    fields = {f.name: f for f in dataclasses.fields(KVzapPress)}
    assert list(fields) == ["compression_ratio", "model_type", "kvzap_model_name"]
    assert fields["model_type"].default == "mlp" and fields["kvzap_model_name"].default is None and not fields["kvzap_model_name"].init
    assert KVzapPress.kvzap_model is None and "kvzap_model" not in fields
    assert KVzapConfig.model_type == "kvzap" and KVzapModel.config_class is KVzapConfig
    cfg = KVzapConfig(input_dim=24, output_dim=2, n_modules=3, hidden_dim=8)
    assert (cfg.input_dim, cfg.output_dim, cfg.hidden_dim, cfg.n_modules) == (24, 2, 8, 3)
    mlp, lin = KVzapModel(cfg), KVzapModel(KVzapConfig(input_dim=24, output_dim=2, n_modules=3))
    assert sorted(mlp.state_dict()) == sorted(f"layers.{i}.{j}.{p}" for i in range(3) for j in (0, 2) for p in ("weight", "bias"))
    assert sorted(lin.state_dict()) == sorted(f"layers.{i}.{p}" for i in range(3) for p in ("weight", "bias"))
    assert isinstance(mlp.layers[0][1], torch.nn.GELU) and mlp.layers[0][1].approximate == "none"
    assert mlp(torch.zeros(5, 3, 24)).shape == (5, 3, 2)

    fields = {f.name: f for f in dataclasses.fields(DMSPress)}
    assert list(fields) == ["press", "threshold", "sliding_window_size", "decoding", "scores_buffer", "compression_ratios"]
    assert (fields["threshold"].default, fields["sliding_window_size"].default, fields["decoding"].default) == (None, 128, False)
    assert not fields["scores_buffer"].init and not fields["compression_ratios"].init
    press = DMSPress(P.KnormPress(0.0), threshold=-4)
    assert press.scores_buffer == {} and press.compression_ratios == {} and "scores_buffer" not in repr(press)
    with pytest.raises(AttributeError, match="compression ratio cannot be set for DMSPress"):
        press.compression_ratio = 0.5
    with pytest.raises(AssertionError, match="Forward pass must be run"):
        press.compression_ratio
    press.compression_ratios.update({0: 0.25, 1: 0.75})
    assert press.compression_ratio == 0.5


def test_surrogate_is_injected_or_loaded_by_name(monkeypatch, tmp_path):
    """kvzap_press.py:64-68: the hub is asked under the reference's name when there is no model or the served model changed; an assigned
    model is kept.  A saved checkpoint loads with from_pretrained."""
    from kvpress_amd.presses.kvzap_press import KVzapConfig, KVzapModel, KVzapPress

    model = _inputs.make_tiny_llama(dtype=torch.float32)
    sur = KVzapModel(KVzapConfig(input_dim=24, output_dim=2, n_modules=2, hidden_dim=8))
    # a checkpoint directory as the hub serves it (config.json + model.safetensors), written by hand
    import json

    from safetensors.torch import save_file

    (tmp_path / "config.json").write_text(json.dumps(dict(model_type="kvzap", input_dim=24, output_dim=2, n_modules=2, hidden_dim=8)))
    save_file({k: v.contiguous() for k, v in sur.state_dict().items()}, str(tmp_path / "model.safetensors"), metadata={"format": "pt"})
    back = KVzapModel.from_pretrained(tmp_path)
    assert all(torch.equal(a, b) for a, b in zip(sur.state_dict().values(), back.state_dict().values())) and back.config.hidden_dim == 8

    asked = []
    monkeypatch.setattr(KVzapModel, "from_pretrained", classmethod(lambda cls, name, *a, **kw: asked.append(name) or sur))
    press = KVzapPress(model_type="linear")
    model.config.name_or_path = "meta-llama/Llama-3.1-8B-Instruct"
    press.post_init_from_model(model)
    press.post_init_from_model(model)
    assert asked == ["nvidia/KVzap-linear-Llama-3.1-8B-Instruct"] and press.kvzap_model is sur and press.kvzap_model_name == asked[0]
    model.config.name_or_path = "Qwen/Qwen3-8B"
    press.post_init_from_model(model)
    assert asked[1:] == ["nvidia/KVzap-linear-Qwen3-8B"]
    injected = KVzapPress()
    injected.kvzap_model = back
    injected.post_init_from_model(model)
    assert injected.kvzap_model is back and len(asked) == 2 and KVzapPress.kvzap_model is None


# ---- C ABI ----------------------------------------------------------------------------------------------------------------------------
P0 = 1 << 12     # a well-aligned non-null address that is never dereferenced: every check below fails before a launch


def test_capi_argument_errors_come_before_any_hip_call(lib):
    def score(dtype=2, B=1, S=4, K=32, N=32, Hout=2, x=P0, w1=P0, b1=P0, w2=P0, b2=P0, out=P0, ws=None, ws_bytes=0):
        return lib.kvp_kvzap_score(x, 0, 0, dtype, w1, b1, w2, b2, B, S, K, N, Hout, out, 0, 0, 0, ws, ws_bytes, None)

    assert score(dtype=7) == -1 and b"bad dtype" in lib.kvp_last_error()
    for kw in (dict(B=0), dict(S=-1), dict(K=0), dict(K=-32), dict(N=-1), dict(Hout=0), dict(Hout=257), dict(S=1 << 31)):
        assert score(**kw) == -1 and b"bad shape" in lib.kvp_last_error(), kw
    for kw in (dict(x=None), dict(w1=None), dict(b1=None), dict(out=None)):
        assert score(**kw) == -1 and b"null pointer" in lib.kvp_last_error(), kw
    for kw in (dict(w2=None), dict(b2=None)):
        assert score(**kw) == -1 and b"second layer" in lib.kvp_last_error(), kw
    assert score(N=0, w2=None, b2=None) == -3 and b"workspace too small" in lib.kvp_last_error()     # the linear model needs no second layer
    assert score() == -3 and b"workspace too small" in lib.kvp_last_error()                            # 4 rows: the few-rows path's partials
    assert score(ws=P0, ws_bytes=16) == -3 and b"workspace too small" in lib.kvp_last_error()
    assert score(S=0, x=None, out=None) == 0                                                              # nothing to do

    total = ctypes.c_int64(-7)

    def count(B=1, H=2, n=10, scores=P0, ws=None, ws_bytes=0, tot=ctypes.byref(total)):
        return lib.kvp_threshold_count(scores, 0, 0, 0, B, H, n, 0.5, ws, ws_bytes, tot, None)

    def select(B=1, H=2, n=10, scores=P0, ws=None, ws_bytes=0, tot=3, out=P0):
        return lib.kvp_threshold_select(scores, 0, 0, 0, B, H, n, 0.5, 0, ws, ws_bytes, tot, out, out, out, None)

    for fn in (count, select):
        for kw in (dict(B=-1), dict(H=-1), dict(n=-1), dict(B=1 << 30, H=1 << 30)):
            assert fn(**kw) == -1 and b"bad shape" in lib.kvp_last_error(), (fn.__name__, kw)
        assert fn(scores=None) == -1 and b"null pointer" in lib.kvp_last_error()
        assert fn() == -3 and b"workspace too small" in lib.kvp_last_error()
    assert count(tot=None) == -1 and b"null pointer" in lib.kvp_last_error()
    assert count(n=0, scores=None) == 0 and total.value == 0
    assert select(out=None) == -1 and b"null pointer" in lib.kvp_last_error()
    for tot in (-1, 21):
        assert select(tot=tot) == -1 and b"bad total" in lib.kvp_last_error()
    assert select(tot=0, scores=None, out=None) == 0


def test_workspaces_hold_nothing_of_extent_s_times_hidden(lib):
    """Llama-3.1-8B, 128k tokens: the reference's two [S, 512] transients are 2 x 128 MiB in bf16; here nothing at all.  A decoding
    step: the float32 partials of 8 outputs per slice of 4 hidden columns"""
    assert lib.kvp_kvzap_score_workspace_bytes(2, 1, 131072, 4096, 512, 8) == 0
    assert lib.kvp_kvzap_score_workspace_bytes(2, 1, 1, 4096, 512, 8) == 128 * 8 * 4
    assert 0 < lib.kvp_kvzap_score_workspace_bytes(2, 2, 8, 4096, 0, 8) <= 64 << 10
    assert 0 < lib.kvp_threshold_select_workspace_bytes(1, 8, 131072) <= 16 << 10
    assert lib.kvp_threshold_select_workspace_bytes(2, 2, 1) <= 1024


def test_no_cpu_fallback():
    from kvpress_amd import _native
    from kvpress_amd._native import KvpressHipError

    s = ZI.score_case(0, 1, 3, 24, 8, 2, "f32")
    with pytest.raises(KvpressHipError):
        _native.kvzap_score(*(torch.from_numpy(s[n]) for n in ("x", "w1", "b1", "w2", "b2")))
    with pytest.raises(KvpressHipError):
        _native.threshold_select(torch.zeros(1, 2, 5), 0.5, 0)


# ---- the oracle -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(ZI.FIXTURES))
def test_oracle_matches_the_references_scores(name):
    """the float64 oracle on the hidden states the reference's scorer received against the float32 scores it returned: the reference's
    own float32 evaluation obeys the contract bound at K = 24 too"""
    spec, g = ZI.FIXTURES[name], golden(name)
    factor, worst, n = ZI.bound(24, spec["hidden_dim"] or 0), 0.0, 0
    for l in range(2):
        for t in range(1 + ZI.DECODE_TOKENS):
            ref, scale = ZO.kvzap_score(g[f"hidden_{l}_{t}"], *ZI.layer_weights(g, spec, l))
            got = g[f"scores_{l}_{t}"]
            assert got.shape == ref.shape == (ZI.BATCH, 2, ZI.PROMPT_TOKENS if t == 0 else 1)
            worst = max(worst, ZO.worst_ratio(got, ref, scale, factor))
            assert float((np.abs(ref - float(g["threshold"])) / scale).min()) >= 10 * factor       # the fixture's threshold condition
            n += got.size
    print(f"{name}: the reference's float32 scores vs the oracle over {n} entries: worst {worst:.3g} of the bound {factor:.3g} x scale")
    assert worst <= 1.0


@pytest.mark.parametrize("name", list(ZI.FIXTURES))
def test_dms_oracle_replays_the_reference(name):
    """tests/_kvzap_oracle.py's step-by-step DMS fed with the reference's scores leaves the reference's triples and ratios"""
    g = golden(name)
    for l in range(2):
        dms = ZO.Dms(float(g["threshold"]), ZI.WINDOW)
        for t in range(1 + ZI.DECODE_TOKENS):
            dms.step(g[f"scores_{l}_{t}"], prefilling=t == 0)
            theirs = g[f"masked_{l}_{t}"]
            ours = np.zeros((3, 0), np.int64) if dms.masked is None else np.stack(dms.masked)
            assert np.array_equal(ours, theirs), (name, l, t)      # order included: both are torch.where's, step after step
            assert dms.ratio == g["ratios"][l, t] and dms.buffer.shape[-1] == ZI.WINDOW
    frac = g["ratios"][:, -1]
    assert ((0.15 < frac) & (frac < 0.6)).all(), frac


def test_threshold_select_oracle():
    sc = np.array([[[0.1, np.nan, -1.0, 0.5], [0.6, 0.4, np.inf, -np.inf]]], np.float32)
    b, h, p = ZO.threshold_select(sc, 0.5, shift=10)
    assert (b.tolist(), h.tolist(), p.tolist()) == ([0, 0, 0, 0], [0, 0, 1, 1], [10, 12, 11, 13])
    tb, th, tp = torch.where(torch.from_numpy(sc) < 0.5)
    assert np.array_equal(tb.numpy(), b) and np.array_equal(th.numpy(), h) and np.array_equal(tp.numpy() + 10, p)


# ---- the presses' host logic over oracle-backed entry points ---------------------------------------------------------------------------
@pytest.fixture
def fake_kvzap(fake_native, monkeypatch):
    calls = []

    def kvzap_score(hidden_states, w1, b1, w2=None, b2=None, out=None):
        for t in (w1, b1) + (() if w2 is None else (w2, b2)):
            assert t.dtype == hidden_states.dtype and t.is_contiguous()
        arrays = [None if t is None else t.detach().double().numpy() for t in (hidden_states, w1, b1, w2, b2)]
        res = torch.from_numpy(ZO.kvzap_score(*arrays)[0].astype(np.float32))
        calls.append(("score", tuple(hidden_states.shape), w2 is not None))
        if out is None:
            return res
        out.copy_(res)
        return out

    def threshold_select(scores, threshold, shift=0):
        assert scores.dtype == torch.float32 and scores.dim() == 3
        calls.append(("select", tuple(scores.shape), int(shift)))
        return [torch.from_numpy(a) for a in ZO.threshold_select(scores.numpy(), threshold, shift)]

    monkeypatch.setattr(fake_native, "kvzap_score", kvzap_score)
    monkeypatch.setattr(fake_native, "threshold_select", threshold_select)
    fake_native.kvzap_calls = calls
    yield fake_native
    del fake_native.kvzap_calls


@pytest.mark.parametrize("name", list(ZI.FIXTURES))
def test_press_host_logic_matches_reference(name, fake_kvzap):
    rec = ZC.check_flow_against_fixture(name, "cpu")
    calls = fake_kvzap.kvzap_calls
    # per layer: one score per forward; the prefill evicts 70 - 16 positions with shift 0, step t one position with shift 54 + t
    scores = [c for c in calls if c[0] == "score"]
    assert scores == [("score", (ZI.BATCH, ZI.PROMPT_TOKENS if t == 0 else 1, 24), rec["spec"]["hidden_dim"] is not None)
                      for t in range(1 + ZI.DECODE_TOKENS) for _ in range(2)]
    selects = [c for c in calls if c[0] == "select"]
    assert selects == [("select", (ZI.BATCH, 2, 54 if t == 0 else 1), 0 if t == 0 else 53 + t) for t in range(1 + ZI.DECODE_TOKENS) for _ in range(2)]
    # the surrogate's weights were packed once per layer
    packs = rec["press"].press._packed_layers
    assert len(packs) == 2 and all(len(v) == 4 for v in packs.values())


def test_sliding_window_zero(fake_kvzap):
    """nothing is protected: every scored position is decided at once and the buffer stays empty"""
    rec = ZC.run_flow("kvzap_mlp", "cpu", sliding_window_size=0)
    for l in range(2):
        dms = ZO.Dms(float(rec["fixture"]["threshold"]), 0)
        for t in range(1 + ZI.DECODE_TOKENS):
            dms.step(rec["scores"][l, t], prefilling=t == 0)
            assert rec["buffer_len"][l, t] == 0
            assert ZO.triples_set(dms.masked) == ZO.triples_set(rec["masked"][l, t]) and rec["ratios"][l, t] == dms.ratio
        assert max(rec["masked"][l, ZI.DECODE_TOKENS][2]) >= ZI.PROMPT_TOKENS        # decoded tokens are evicted too


def test_prefill_only_mode_leaves_decoding_alone(fake_kvzap):
    rec = ZC.run_flow("kvzap_linear", "cpu", decoding=False)
    g = rec["fixture"]
    assert len([c for c in fake_kvzap.kvzap_calls if c[0] == "score"]) == 2          # the two layers' prefill
    for l in range(2):
        for t in range(1 + ZI.DECODE_TOKENS):
            assert ZO.triples_set(rec["masked"][l, t]) == ZO.triples_set(g[f"masked_{l}_0"])
            assert rec["buffer_len"][l, t] == ZI.WINDOW and rec["ratios"][l, t] == g["ratios"][l, 0]


def test_a_new_prefill_forgets_the_last_context(fake_kvzap):
    from transformers import DynamicCache

    rec = ZC.run_flow("kvzap_linear", "cpu")
    press, model = rec["press"], rec["model"]
    ids = torch.from_numpy(rec["fixture"]["prompt_ids"])[:, :10]
    with torch.no_grad(), press(model):
        model.model(input_ids=ids, past_key_values=DynamicCache())
    assert {l: b.shape[-1] for l, b in press.scores_buffer.items()} == {0: 10, 1: 10} and press.compression_ratios == {0: 0, 1: 0}
    assert all(layer.self_attn.masked_key_indices is None for layer in model.model.layers)


def test_kvzap_alone_is_a_scorer_press(fake_kvzap):
    """under ScorerPress.compress: int(S * (1 - r)) rows per head, the best-scored ones"""
    from kvpress_amd.presses.kvzap_press import KVzapPress

    spec, g = ZI.FIXTURES["kvzap_mlp"], golden("kvzap_mlp")
    llama = _inputs.make_tiny_llama(dtype=torch.float32)
    press = KVzapPress(compression_ratio=0.3)
    press.kvzap_model = ZI.load_surrogate(spec, g, llama.config)
    hidden = torch.from_numpy(g["hidden_1_0"])[:, :50]
    rs = np.random.RandomState(3)
    keys, values = (torch.from_numpy(rs.standard_normal((ZI.BATCH, 2, 50, 6)).astype(np.float32)) for _ in range(2))
    ko, vo = press.compress(SimpleNamespace(layer_idx=1), hidden, keys, values, None, {})
    assert ko.shape == vo.shape == (ZI.BATCH, 2, int(50 * (1 - 0.3)), 6)
    scores = press.score(SimpleNamespace(layer_idx=1), hidden, keys, values, None, {})
    assert scores.dtype == torch.float32 and np.allclose(scores.numpy(), g["scores_1_0"][..., :50], atol=1e-5)
    kept = scores.topk(35, dim=-1).indices.sort(dim=-1).values
    assert torch.equal(ko, keys.gather(2, kept[..., None].expand(-1, -1, -1, 6)))


@pytest.mark.parametrize("decoding", [False, True])
def test_pipeline_enters_the_press_for_decoding_iff_asked(decoding, fake_kvzap):
    """kvpress/pipeline.py:231-232"""
    from kvpress_amd.presses.dms_press import DMSPress
    from kvpress_amd.presses.kvzap_press import KVzapPress

    entered = []

    class Counting(DMSPress):
        @contextmanager
        def __call__(self, model):
            entered.append(len(self.scores_buffer))
            with DMSPress.__call__(self, model):
                yield

    pipe = tiny_pipeline("cpu", dtype=torch.float32)
    spec, g = ZI.FIXTURES["kvzap_linear"], golden("kvzap_linear")
    scorer = KVzapPress(model_type="linear")
    scorer.kvzap_model = ZI.load_surrogate(spec, g, pipe.model.config)
    press = Counting(scorer, threshold=float(g["threshold"]), sliding_window_size=4, decoding=decoding)
    res = pipe(_inputs.tiny_context(40), question="w1 w2", press=press, max_new_tokens=3)
    assert isinstance(res["answer"], str)
    assert entered == ([0, 2] if decoding else [0])
    scored = [c for c in fake_kvzap.kvzap_calls if c[0] == "score"]
    assert (len(scored) > 2) == decoding and len(scored) >= 2          # the two layers' prefill; the question and the answer only when asked
