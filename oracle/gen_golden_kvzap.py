#!/usr/bin/env python3
"""Reference outputs of DMSPress(KVzapPress): runs the REAL reference (NVIDIA/kvpress, put on the path by oracle/gen_golden.py's shims) on
the host CPU over the tiny float32 Llama of tests/_inputs.py with a seeded surrogate (tests/_kvzap_inputs.py) and writes
tests/golden/kvzap_*.npz -- one fixture for the mlp (hidden_dim 32), one for the linear model.

    PYTHONDONTWRITEBYTECODE=1 python oracle/gen_golden_kvzap.py [case ...]

The surrogate is injected through a subclass, as the reference's own tests/default_presses.py:45-55 does (no hub).  transformers 5.x
passes no ``cache_position`` to the attention layers, which the reference's hook reads (dms_press.py:73-74): the forward pre-hook of
oracle/gen_golden_pipeline.py re-creates it.  B = 2, 70 prompt tokens through ``model.model`` under the press, then 6 TEACHER-FORCED
single-token forwards (the ids are part of the inputs, so the trajectory cannot fork), sliding_window_size 16, decoding=True.

Per fixture: ``prompt_ids`` [2,70], ``decode_ids`` [2,6], ``threshold``; the surrogate's state dict (``weight/<name>``); per layer l and
step t (0 = the prefill): ``scores_<l>_<t>`` float32 [2,2,q_len] as the wrapped press returned them, ``hidden_<l>_<t>`` the hidden states
it received, ``masked_<l>_<t>`` int64 [3,n] the layer's masked triples after the step (n = 0: None) and ``ratios`` [L, steps].

Threshold condition (on the inputs; a cap, not a measurement).  The prefill's scores do not depend on the threshold (nothing is masked
before the first decoding step), so the candidates are the midpoints of the gaps between neighbouring sorted prefill scores around
their 0.3, 0.5 and 0.7 quantiles.  Each candidate is run; its margin is the minimum of |score - threshold| / scale over EVERY entry
scored in that run (scale: tests/_kvzap_oracle.py).  The fixture keeps the candidate with the largest margin and asserts that it is at
least 10 x the contract bound 2 (K + N + 4) u: the reference alone has no entry in the band, so masked sets must be EQUAL."""
import sys

import gen_golden  # (next to this script) the generators' shared opening and closing


def main(argv):
    gen_golden.setup()
    import numpy as np
    import torch
    from kvpress.presses.dms_press import DMSPress  # the reference
    from kvpress.presses.kvzap_press import KVzapConfig, KVzapModel, KVzapPress
    from transformers import DynamicCache

    import _inputs
    import _kvzap_inputs as ZI
    import _kvzap_oracle as ZO

    def inject_cache_position(module, args, kwargs):
        cache = kwargs["past_key_values"]
        past = cache.get_seq_length(module.layer_idx)
        q_len = kwargs["hidden_states"].shape[1]
        kwargs["cache_position"] = torch.arange(past, past + q_len)
        return args, kwargs

    for name in argv or list(ZI.FIXTURES):
        spec = ZI.FIXTURES[name]
        model = _inputs.make_tiny_llama(dtype=torch.float32)
        for layer in model.model.layers:
            layer.self_attn.register_forward_pre_hook(inject_cache_position, with_kwargs=True)
        surrogate = ZI.make_surrogate(KVzapConfig, KVzapModel, spec, model.config)
        prompt, decode = (torch.from_numpy(a) for a in ZI.fixture_ids(spec["seed"]))
        K, N = model.config.hidden_size, spec["hidden_dim"] or 0
        L = model.config.num_hidden_layers

        class SeededKVzapPress(KVzapPress):
            def post_init_from_model(self, model_):
                self.kvzap_model = surrogate

        def run(threshold):
            scorer = SeededKVzapPress(model_type=spec["model_type"])
            press = DMSPress(scorer, threshold=threshold, sliding_window_size=ZI.WINDOW, decoding=True)
            rec = {"scores": {}, "hidden": {}, "masked": {}, "ratios": np.zeros((L, 1 + ZI.DECODE_TOKENS))}
            score, step = scorer.score, [0]

            def recording_score(module, hidden_states, keys, values, attentions, kwargs):
                out = score(module, hidden_states, keys, values, attentions, kwargs)
                rec["scores"][module.layer_idx, step[0]] = out.detach().clone().numpy()
                rec["hidden"][module.layer_idx, step[0]] = hidden_states.detach().clone().numpy()
                return out

            scorer.score = recording_score

            def after_step():
                for l, layer in enumerate(model.model.layers):
                    m = layer.self_attn.masked_key_indices
                    rec["masked"][l, step[0]] = np.zeros((3, 0), np.int64) if m is None else np.stack([t.numpy().astype(np.int64) for t in m])
                    rec["ratios"][l, step[0]] = press.compression_ratios[l]
                step[0] += 1

            cache = DynamicCache()
            with torch.no_grad(), press(model):
                model.model(input_ids=prompt, past_key_values=cache)
                after_step()
                for t in range(ZI.DECODE_TOKENS):
                    model.model(input_ids=decode[:, t:t + 1], past_key_values=cache)
                    after_step()
            assert [layer.keys.shape[2] for layer in cache.layers] == [ZI.PROMPT_TOKENS + ZI.DECODE_TOKENS] * L
            margin = np.inf
            for (l, t), sc in rec["scores"].items():
                _, scale = ZO.kvzap_score(rec["hidden"][l, t], *ZI.layer_weights(weights, spec, l))
                margin = min(margin, float((np.abs(sc.astype(np.float64) - threshold) / scale).min()))
            return rec, margin

        weights = {f"weight/{k}": v.detach().numpy() for k, v in surrogate.state_dict().items()}
        first, _ = run(0.0)
        pre = np.sort(np.concatenate([first["scores"][l, 0].ravel() for l in range(L)]).astype(np.float64))
        best = None
        for q in (0.3, 0.5, 0.7):
            i0 = int(q * len(pre))
            for i in range(max(i0 - 8, 0), min(i0 + 8, len(pre) - 1)):
                thr = float(np.float32(0.5 * (pre[i] + pre[i + 1])))
                rec, margin = run(thr)
                if best is None or margin > best[1]:
                    best = (thr, margin, rec, q)
        thr, margin, rec, q = best
        need = 10 * ZI.bound(K, N)
        assert margin >= need, f"{name}: the best margin {margin:.3g} of scale is below 10 x the contract bound {need:.3g}"
        fractions = [rec["ratios"][l, -1] for l in range(L)]
        print(f"{name}: threshold {thr!r} (near the {q} quantile), margin {margin:.3g} of scale (10 x bound = {need:.3g}), "
              f"masked fractions after the last step {fractions}")
        out = dict(prompt_ids=prompt.numpy(), decode_ids=decode.numpy(), threshold=np.float64(thr), margin=np.float64(margin),
                   ratios=rec["ratios"], **weights)
        for (l, t), sc in rec["scores"].items():
            out[f"scores_{l}_{t}"], out[f"hidden_{l}_{t}"], out[f"masked_{l}_{t}"] = sc, rec["hidden"][l, t], rec["masked"][l, t]
        gen_golden.save(name, out)


if __name__ == "__main__":
    main(sys.argv[1:])
