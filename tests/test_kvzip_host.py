"""KVzipPress without a GPU: the package surface and the class next to the reference's (kvpress/presses/kvzip_press.py), the argument
checks of the new C-ABI entry, the float64 oracle (tests/_kvzip_oracle.py) against the REAL reference's outputs (tests/golden/kvzip_*.npz,
oracle/gen_golden_kvzip.py), and the press's host logic with ``_native.kvzip_score`` replaced by the oracle."""
import dataclasses
import functools
import logging

import numpy as np
import pytest
import torch

import _inputs
import _kvzip_inputs as KI
import _kvzip_oracle as KO
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
    from kvpress_amd.presses import kvzip_press as M

    assert "KVzipPress" not in P.__all__
    with pytest.raises(AttributeError, match="outside the hot-path scope") as e:
        P.KVzipPress
    assert "kvpress_amd.presses.kvzip_press.KVzipPress" in str(e.value)
    assert issubclass(M.KVzipPress, P.BasePress) and not issubclass(M.KVzipPress, P.ScorerPress)


def test_fields_assertion_and_warning(caplog):
    """kvzip_press.py:50-53 (the dataclass fields), :56 (the assertion), :57-62 (the warning)"""
    from kvpress_amd.presses.kvzip_press import KVzipPress

    assert [(f.name, f.default) for f in dataclasses.fields(KVzipPress)] == [("compression_ratio", 0.0), ("layerwise", False), ("n_sink", 4),
                                                                              ("kvzip_plus_normalization", False)]
    assert KVzipPress.tokenizer is None
    for r in (-0.1, 1.0):
        with pytest.raises(AssertionError, match="Compression ratio must be between 0 and 1"):
            KVzipPress(compression_ratio=r)
    with caplog.at_level(logging.WARNING, logger="kvpress_amd.presses.kvzip_press"):
        press = KVzipPress(0.3)
    assert len(caplog.records) == 1 and "requires multiple forward passes" in caplog.records[0].getMessage()
    assert (press.context_length, press.prefix_length, press.start_idx, press.end_idx, press.score_val) == (0, 0, 0, 0, None)
    import inspect

    sig = inspect.signature(KVzipPress.prepare)
    assert [(n, p.default) for n, p in list(sig.parameters.items())[3:]] == [("chunk_size", 2048), ("prev_postfix_size", 8)]
    assert list(inspect.signature(KVzipPress._chunk_fn).parameters) == ["self", "ctx_ids", "chunk_size"]


def test_composed_press_refuses_it():
    import kvpress_amd as P
    from kvpress_amd.presses.kvzip_press import KVzipPress

    with pytest.raises(AssertionError, match="ComposedPress cannot contains AdaKVPress or KVzipPress"):
        P.ComposedPress([P.KnormPress(0.5), KVzipPress(0.5)])


def test_chunk_fn():
    from kvpress_amd.presses.kvzip_press import KVzipPress

    press = KVzipPress(0.5)
    ids = torch.arange(150)[None]
    assert [c.shape[1] for c in press._chunk_fn(ids, 64)] == [64, 64, 22]
    assert [c.shape[1] for c in press._chunk_fn(ids[:, :128], 64)] == [64, 64]
    assert [c.shape[1] for c in press._chunk_fn(ids[:, :64], 64)] == [64] and press._chunk_fn(ids[:, :10], 64)[0] is not None
    assert torch.equal(torch.cat(press._chunk_fn(ids, 64), dim=1), ids)


# ---- C ABI ----------------------------------------------------------------------------------------------------------------------------
def test_capi_argument_errors_come_before_any_hip_call(lib):
    def score(dtype=2, Hq=4, Hkv=2, S=200, Lq=50, D=16, sink=4, start=10, end=100, stride=150, ptr=None):
        return lib.kvp_kvzip_score(ptr, 0, 0, 0, ptr, ptr, 0, 0, ptr, 0, 0, 0, dtype, 1, Hq, Hkv, S, Lq, D, sink, start, end, None, None, ptr,
                                   stride, None, 0, None)

    assert score(dtype=7) == -1 and b"bad dtype" in lib.kvp_last_error()
    assert score(Hq=5) == -1 and b"Hq % Hkv != 0" in lib.kvp_last_error()
    for kw in (dict(D=7), dict(Lq=0), dict(S=50), dict(S=1 << 31)):
        assert score(**kw) == -1 and b"bad shape" in lib.kvp_last_error(), kw
    for kw in (dict(sink=-1), dict(sink=11), dict(start=100), dict(end=151)):
        assert score(**kw) == -1 and b"sink <= start < end <= S - Lq" in lib.kvp_last_error(), kw
    assert score(stride=89) == -1 and b"out_stride" in lib.kvp_last_error()
    assert score() == -1 and b"null pointer" in lib.kvp_last_error()
    assert score(ptr=1 << 12) == -3 and b"workspace too small" in lib.kvp_last_error()      # (checked before any launch)


def test_workspace_is_nowhere_near_the_references_temporary(lib):
    """Llama-3.1-8B, one 2048-token chunk: the reference's softmax alone is 8 * 4 * 2070 * 4122 * 2 bytes = 0.55 GB (kvzip_press.py:330-332);
    here the rotated queries (17 MB) and a few floats per row"""
    ws = lib.kvp_kvzip_score_workspace_bytes(2, 1, 32, 8, 2070, 128, 4, 2048)
    assert 16 << 20 < ws < 24 << 20
    assert lib.kvp_kvzip_score_workspace_bytes(0, 1, 4, 2, 70, 6, 0, 64) < 64 << 10
    assert lib.kvp_kvzip_score_workspace_bytes(2, 1, 5, 2, 70, 6, 0, 64) == 0               # not a shape


def test_no_cpu_fallback():
    from kvpress_amd import _native
    from kvpress_amd._native import KvpressHipError

    s = KI.kernel_case("f32_d6_generic")
    with pytest.raises(KvpressHipError):
        _native.kvzip_score(*(torch.from_numpy(s[n]) for n in ("q", "cos", "sin", "keys")), s["sink"], s["start"], s["end"])


# ---- the oracle -----------------------------------------------------------------------------------------------------------------------
def test_oracle_closed_forms():
    """the exact inputs of tests/test_gpu_kvzip.py on the oracle itself: census, heavy key in / outside the chunk, heavy row"""
    shape = (2, 2, 70, 6, 4, 9, 64, 22, "f32")
    Hkv, G, Lq, D, sink, start, n, tail, _ = shape

    def run(s):
        return KO.kvzip_score(KO.rope(s["q"], s["cos"], s["sin"]), s["keys"], s["sink"], s["start"], s["end"], s["row_scale"], s["col_scale"])

    s, _ = KI.exact_case(*shape)
    assert np.allclose(run(s), 1.0 / (sink + n + 1), rtol=1e-13)
    for mutant_sink in (sink - 1, sink + 1):     # a dropped or doubled key moves the census by 1 / count: far above 1e-5
        assert abs((sink + n + 1) / (mutant_sink + n + 1) - 1) > 1e-3
    s["row_scale"] = np.zeros((1, Lq), np.float32)
    s["row_scale"][0, 33] = 1.0
    assert np.allclose(run(s), 1.0 / (sink + n + 34), rtol=1e-13)
    s, lam = KI.exact_case(*shape, heavy_key=(1, start + 5))
    got, e = run(s), np.exp(lam)
    assert np.isclose(got[0, 1, 5], e / (sink + n + e), rtol=1e-13) and np.allclose(got[0, 0], 1.0 / (sink + n + 1), rtol=1e-13)
    assert np.allclose(np.delete(got[0, 1], 5), 1.0 / (sink + n + e), rtol=1e-13)
    for p in (sink, start - 1, start + n, start + n + tail + 1):
        s, _ = KI.exact_case(*shape, heavy_key=(1, p))
        assert np.allclose(run(s), 1.0 / (sink + n + 1), rtol=1e-13), p
    s, lam = KI.exact_case(*shape, heavy_key=(1, start + 32), heavy_row=(3, 69))
    got, e = run(s), np.exp(lam)
    assert np.isclose(got[0, 1, 32], e / (sink + n + 69 + e), rtol=1e-13) and np.allclose(np.delete(got[0, 1], 32), 1.0 / (sink + n + 1), rtol=1e-13)


# ---- the press over the oracle-backed entry point against the reference's outputs ---------------------------------------------------------
@pytest.fixture
def fake_kvzip(fake_native, monkeypatch):
    calls = []

    def kvzip_score(q_pre, cos, sin, keys, sink, start, end, row_scale=None, col_scale=None, out=None):
        q_rot = KO.rope(q_pre.detach().double().numpy(), cos.double().numpy(), sin.double().numpy())
        rs, cs = (None if x is None else x.double().numpy() for x in (row_scale, col_scale))
        res = torch.from_numpy(KO.kvzip_score(q_rot, keys.detach().double().numpy(), sink, start, end, rs, cs).astype(np.float32))
        calls.append(dict(sink=sink, start=start, end=end, Lq=q_pre.shape[2], S=keys.shape[2], scales=row_scale is not None and col_scale is not None))
        if out is None:
            return res
        out.copy_(res)
        return out

    monkeypatch.setattr(fake_native, "kvzip_score", kvzip_score)
    fake_native.kvzip_calls = calls
    yield fake_native
    del fake_native.kvzip_calls


def run_press(spec, ids=None, model=None, cache=None, **overrides):
    """the press on the tiny float32 Llama as oracle/gen_golden_kvzip.py runs the reference's; returns what compress_post saw and left"""
    from transformers import DynamicCache

    from kvpress_amd.presses.kvzip_press import KVzipPress

    model = model or _inputs.make_tiny_llama(dtype=torch.float32)
    press = KVzipPress(**{**spec["press"], **overrides})
    press.tokenizer = _inputs.make_tiny_tokenizer()
    seen = {"press": press, "model": model}
    prepare, compress_post = functools.partial(press.prepare, chunk_size=KI.CHUNK), press.compress_post

    def recording_prepare(m, tok):
        seen["pairs"] = prepare(m, tok)
        return seen["pairs"]

    def recording_compress_post(m):
        seen["score_val"] = press.score_val.detach().clone()
        seen["lengths"] = [layer.keys.shape[2] for layer in press._cache.layers]
        return compress_post(m)

    press.prepare, press.compress_post = recording_prepare, recording_compress_post
    ids = torch.from_numpy(KI.context_ids(spec["seed"])) if ids is None else ids
    seen["cache"] = cache = cache or DynamicCache()
    with torch.no_grad(), press(model):
        model.model(input_ids=ids, past_key_values=cache)
    seen["masked"] = [layer.self_attn.masked_key_indices for layer in model.model.layers]
    return seen


@pytest.mark.parametrize("name", list(KI.FIXTURES))
def test_press_host_logic_matches_reference(name, fake_kvzip):
    spec, g = KI.FIXTURES[name], golden(name)
    seen = run_press(spec)
    # chunking and the prompts of the first and the later chunks
    assert len(seen["pairs"]) == int(g["n_pairs"]) == 3
    for i, (a, r) in enumerate(seen["pairs"]):
        assert np.array_equal(a.numpy(), g[f"prefill_{i}"]) and np.array_equal(r.numpy(), g[f"repeat_{i}"]), i
        assert r.dtype == torch.long
    assert [p[0].shape[1] for p in seen["pairs"]] == [64, 64, 22]
    assert torch.equal(seen["pairs"][1][1][:, -64 - 8:-64], seen["pairs"][0][0][:, -8:])     # "starting with" the previous chunk's tail
    # one call per layer and chunk: sink = min(n_sink, start) -- 0 for the first chunk --, the chunk's columns, the whole cache's keys
    calls = fake_kvzip.kvzip_calls
    assert len(calls) == 2 * 3
    for c, (i, (a, r)) in zip(calls, [(i, p) for i, p in enumerate(seen["pairs"]) for _ in range(2)]):
        assert (c["sink"], c["start"], c["end"]) == (0 if i == 0 else 4, 64 * i, 64 * i + a.shape[1])
        assert (c["Lq"], c["S"]) == (r.shape[1], KI.CONTEXT_TOKENS + r.shape[1])               # every layer was cut back after the chunk before
        assert c["scales"] == bool(spec["press"].get("kvzip_plus_normalization"))
    assert seen["lengths"] == [KI.CONTEXT_TOKENS] * 2 and [l.keys.shape[2] for l in seen["cache"].layers] == [KI.CONTEXT_TOKENS] * 2
    # the oracle's scores against the reference's float32 scores: both sum <= 237 float32 terms per row (2e-5 = 170 float32 roundings)
    sv, ref = seen["score_val"].numpy(), g["score_val"]
    assert sv.dtype == np.float32 and sv.shape == ref.shape == (2, 1, 2, KI.CONTEXT_TOKENS)
    fin = np.isfinite(ref)                       # (KVzip+ on the zero hidden states of the prompt: +inf in both)
    assert np.array_equal(sv[~fin], ref[~fin])
    err = float(np.abs(sv[fin] / ref[fin] - 1).max())
    print(f"{name}: oracle score_val vs the reference's float32 score_val: {err:.3g} relative")
    assert err <= 2e-5
    # the selection: counts exact, sets equal outside the bands
    L, _, H, C = ref.shape
    o = KO.compress_post(ref, spec["press"]["compression_ratio"], spec["press"].get("layerwise", False))
    assert list(o["counts"]) == list(g["n_pruned_layers"])
    for l in range(L):
        band = o["bands"][l] | o["global_band"][l]
        theirs = g[f"masked_head_{l}"].astype(np.int64) * C + g[f"masked_seq_{l}"]
        assert KO.sets_equal_outside(o["pruned"][l], theirs, band), f"{name} layer {l}: the oracle's selection"
        b, h, p = seen["masked"][l]
        assert len(h) == int(g["n_pruned_layers"][l]) and not b.any() and h.dtype == torch.int64
        assert KO.sets_equal_outside(h.numpy() * C + p.numpy(), theirs, band), f"{name} layer {l}: the press's selection"
    # the state is gone
    press = seen["press"]
    assert press.score_val is None and press._cache is None and press._context_ids is None and press.context_length == 0


def test_sink_columns_and_float32_table(fake_kvzip):
    """score_val is float32 whatever the model's dtype, [..., :n_sink] = 1 before the chunks are scored (kvzip_press.py:248)"""
    from kvpress_amd.presses.kvzip_press import KVzipPress

    press = KVzipPress(0.5, n_sink=3)
    press._context_ids, press.context_length = torch.zeros((1, 20), dtype=torch.long), 20
    press._suffix_ids = torch.zeros((1, 0), dtype=torch.long)      # no chat template: "\n" holds no word
    model = _inputs.make_tiny_llama(dtype=torch.bfloat16)
    pairs = press.prepare(model, _inputs.make_tiny_tokenizer(), chunk_size=8, prev_postfix_size=2)
    assert press.score_val.dtype == torch.float32 and press.score_val.shape == (2, 1, 2, 20)
    assert bool((press.score_val[..., :3] == 1).all()) and bool((press.score_val[..., 3:] == 0).all())
    assert [a.shape[1] for a, _ in pairs] == [8, 8, 4] and pairs[1][1].shape[1] == pairs[0][1].shape[1] + 5 + 2   # the later prompt: 5 more words, then the previous tail


def test_ratio_zero_does_nothing(fake_kvzip):
    seen = run_press(KI.FIXTURES["kvzip_global"], compression_ratio=0.0)
    assert not fake_kvzip.kvzip_calls and "pairs" not in seen and seen["masked"] == [None, None]
    assert all(not layer.self_attn._forward_hooks for layer in seen["model"].model.layers)


def test_state_is_reset_after_an_exception(fake_kvzip, monkeypatch):
    from transformers import DynamicCache

    from kvpress_amd.presses.kvzip_press import KVzipPress

    model = _inputs.make_tiny_llama(dtype=torch.float32)
    original = model.model.forward
    press = KVzipPress(0.5)
    press.tokenizer = _inputs.make_tiny_tokenizer()
    ids = torch.from_numpy(KI.context_ids(0))
    with pytest.raises(RuntimeError, match="inside the with"):
        with torch.no_grad(), press(model):
            model.model(input_ids=ids, past_key_values=DynamicCache())
            assert press._context_ids is ids
            raise RuntimeError("inside the with")
    assert model.model.forward == original and press._context_ids is None and press._cache is None and not fake_kvzip.kvzip_calls

    # and after one in the middle of the reconstruction: the hooks are gone too
    def failing(*a, **kw):
        raise RuntimeError("in the scorer")

    monkeypatch.setattr(fake_kvzip, "kvzip_score", failing)
    with pytest.raises(RuntimeError, match="in the scorer"):
        run_press(KI.FIXTURES["kvzip_global"], model=model)
    assert all(not layer.self_attn._forward_hooks for layer in model.model.layers)
    assert model.model.forward == original


def test_batch_and_eager_are_refused(fake_kvzip):
    spec = KI.FIXTURES["kvzip_global"]
    with pytest.raises(AssertionError, match="batch size of 1"):
        run_press(spec, ids=torch.from_numpy(KI.context_ids(0)).repeat(2, 1))
    model = _inputs.make_tiny_llama(dtype=torch.float32)
    model.config._attn_implementation = "eager"
    with pytest.raises(AssertionError, match="eager mode not supported"):
        run_press(spec, model=model)


def test_tokenizer_default_is_the_hub(monkeypatch):
    """without the class attribute the reference's call is made (kvzip_press.py:96)"""
    import transformers

    from kvpress_amd.presses.kvzip_press import KVzipPress

    asked = []

    def from_pretrained(name, *a, **kw):
        asked.append(name)
        return _inputs.make_tiny_tokenizer()

    monkeypatch.setattr(transformers.AutoTokenizer, "from_pretrained", staticmethod(from_pretrained))
    model = _inputs.make_tiny_llama(dtype=torch.float32)
    model.config.name_or_path = "somewhere/tiny"
    with KVzipPress(0.0)(model):
        pass
    assert asked == ["somewhere/tiny"]


# ---- compile-time budgets of the new kernels (tests/test_build_resources.py's audit, per kernel) ------------------------------------------
def test_kernel_register_and_lds_budgets():
    """no kernel of kvzip.hip spills or uses scratch; the matrix-core kernels keep two waves per SIMD and the 64 KiB of static LDS a launch
    gets without raising the limit (two double-buffered 128-row tiles)"""
    import os
    import re
    import subprocess

    from kvpress_amd import build as B

    src = os.path.join(B.CSRC, "kvzip.hip")
    r = subprocess.run([B._hipcc(), *B.flags_for(src), "-c", src, "-o", os.devnull, "-Rpass-analysis=kernel-resource-usage"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    kernels, name = {}, None
    for line in r.stderr.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            name = m.group(1)
            kernels[name] = {}
        for key in ("ScratchSize [bytes/lane]", "VGPRs Spill", "SGPRs Spill", "LDS Size [bytes/block]", "Occupancy [waves/SIMD]"):
            m = re.search(r"\s" + re.escape(key) + r": (\d+)", line)
            if m:
                kernels[name][key] = int(m.group(1))
    mfma = {n: k for n, k in kernels.items() if "kvzip_mfma_kernel" in n}
    assert len(mfma) == 2 * 4 * 2 and len(kernels) >= len(mfma) + 3 + 6 + 2       # dtype x D x pass; rope, generic passes, combine, merge
    for n, k in kernels.items():
        assert k["ScratchSize [bytes/lane]"] == 0 and k["VGPRs Spill"] == 0 and k["SGPRs Spill"] == 0, (n, k)
    for n, k in mfma.items():
        assert k["LDS Size [bytes/block]"] <= 64 * 1024 and k["Occupancy [waves/SIMD]"] >= 2, (n, k)
