"""The DMSPress(KVzapPress) flow of the fixtures (tests/golden/kvzap_*.npz), shared by the host test (oracle-backed entry points, CPU) and
the GPU test (the library): the same model, ids and surrogate weights as oracle/gen_golden_kvzap.py used for the REAL reference."""
import numpy as np
import torch

import _inputs
import _kvzap_inputs as ZI
import _kvzap_oracle as ZO
from _support import golden


def run_flow(name, device, **press_kw):
    """prefill + the teacher-forced decoding steps under this package's DMSPress(KVzapPress); returns what every step left behind:
    scores[(l, t)], hidden[(l, t)], masked[(l, t)] (None or three int64 arrays), ratios [L, steps], buffer_len[(l, t)]"""
    from transformers import DynamicCache

    from kvpress_amd.presses.dms_press import DMSPress
    from kvpress_amd.presses.kvzap_press import KVzapPress

    spec, g = ZI.FIXTURES[name], golden(name)
    model = _inputs.make_tiny_llama(dtype=torch.float32, device=device)
    scorer = KVzapPress(model_type=spec["model_type"])
    scorer.kvzap_model = ZI.load_surrogate(spec, g, model.config)
    kw = dict(threshold=float(g["threshold"]), sliding_window_size=ZI.WINDOW, decoding=True)
    kw.update(press_kw)
    press = DMSPress(scorer, **kw)
    L, steps = model.config.num_hidden_layers, 1 + ZI.DECODE_TOKENS
    rec = dict(scores={}, hidden={}, masked={}, buffer_len={}, ratios=np.full((L, steps), np.nan), press=press, model=model, fixture=g, spec=spec)
    score, step = scorer.score, [0]

    def recording_score(module, hidden_states, keys, values, attentions, kwargs):
        out = score(module, hidden_states, keys, values, attentions, kwargs)
        assert out.dtype == torch.float32 and tuple(out.shape) == (ZI.BATCH, 2, hidden_states.shape[1])
        rec["scores"][int(module.layer_idx), step[0]] = out.detach().cpu().numpy().copy()
        rec["hidden"][int(module.layer_idx), step[0]] = hidden_states.detach().float().cpu().numpy().copy()
        return out

    scorer.score = recording_score

    def after_step():
        for l, layer in enumerate(model.model.layers):
            m = getattr(layer.self_attn, "masked_key_indices", None)
            if m is not None:
                assert len(m) == 3 and all(t.dtype == torch.int64 and t.device.type == torch.device(device).type for t in m)
                m = tuple(t.cpu().numpy() for t in m)
            rec["masked"][l, step[0]] = m
            if l in press.compression_ratios:
                rec["ratios"][l, step[0]] = press.compression_ratios[l]
            if l in press.scores_buffer:
                rec["buffer_len"][l, step[0]] = press.scores_buffer[l].shape[-1]
        step[0] += 1

    prompt, decode = (torch.from_numpy(g[n]).to(device) for n in ("prompt_ids", "decode_ids"))
    cache = DynamicCache()
    with torch.no_grad(), press(model):
        model.model(input_ids=prompt, past_key_values=cache)
        after_step()
        for t in range(ZI.DECODE_TOKENS):
            model.model(input_ids=decode[:, t:t + 1], past_key_values=cache)
            after_step()
    assert [layer.keys.shape[2] for layer in cache.layers] == [ZI.PROMPT_TOKENS + ZI.DECODE_TOKENS] * L     # nothing leaves the cache
    return rec


def check_flow_against_fixture(name, device):
    """masked triples as SETS equal to the reference's at every step and layer (the fixture's threshold has no reference score within
    10 x the contract bound), compression ratios equal, the window never longer than sliding_window_size, the scores inside the contract"""
    rec = run_flow(name, device)
    g, spec = rec["fixture"], rec["spec"]
    L, steps = rec["ratios"].shape
    factor, worst = ZI.bound(24, spec["hidden_dim"] or 0), 0.0
    for l in range(L):
        for t in range(steps):
            ref, scale = ZO.kvzap_score(rec["hidden"][l, t], *ZI.layer_weights(g, spec, l))
            worst = max(worst, ZO.worst_ratio(rec["scores"][l, t], ref, scale, factor))
            theirs = g[f"masked_{l}_{t}"]
            ours = rec["masked"][l, t]
            assert ZO.triples_set(theirs) == (set() if ours is None else ZO.triples_set(ours)), f"{name}: layer {l} step {t}: masked sets differ"
            assert ours is None or len(ours[0]) == theirs.shape[1], f"{name}: layer {l} step {t}: a triple is listed twice"
            assert rec["buffer_len"][l, t] <= ZI.WINDOW
    print(f"{name} on {device}: worst score error {worst:.3g} of the contract bound 2 (K + N + 4) u scale")
    assert worst <= 1.0
    assert np.array_equal(rec["ratios"], g["ratios"]), (rec["ratios"], g["ratios"])
    assert rec["press"].compression_ratio == g["ratios"][:, -1].mean()
    return rec
