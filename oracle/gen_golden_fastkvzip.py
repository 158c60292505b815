#!/usr/bin/env python3
"""Reference outputs of FastKVzipPress: runs the REAL reference (NVIDIA/kvpress, put on the path by oracle/gen_golden.py's shims) on the
host CPU and writes two kinds of fixture.

    PYTHONDONTWRITEBYTECODE=1 python oracle/gen_golden_fastkvzip.py [name ...]

(a) tests/golden/fastkvzip_flow_*.npz (tests/_fastkvzip_inputs.py: FLOW).  The real press on the tiny float32 Llama of tests/_inputs.py,
seeded gates injected through a subclass as the reference's own tests/default_presses.py:58-71 does (no hub).  transformers 5.x passes no
``cache_position`` to the attention layers, which the reference's hook reads (fastkvzip_press.py:226): the forward pre-hook of
oracle/gen_golden_kvzap.py re-creates it.  Per fixture: ``ids`` [1, tokens], ``seed``, the gates' state dicts (``gate<l>/<key>``),
``score_val`` [L, 1, Hkv, tokens] as compress_post stacked it, per layer ``hidden_<l>`` (the hidden states the gate received), ``masked_<l>``
int64 [3, n] and ``n_pruned`` [L].

Condition on (a) (on the inputs; a cap, not a measurement).  torch.topk's choice among equal scores is unspecified, and layer 0's gate
sees the normed embeddings, so equal token ids give bit-equal scores there.  The generator therefore takes the gaps between neighbouring
sorted scores at the cross-layer boundary and at each layer's boundary (tests/_fastkvzip_oracle.py: boundary_gaps) and asserts that every
one is at least 10 x the contract bound 2 x max(bound); where it is not, it tries the next seed.  With that, masked SETS must equal the
reference's.  The 40-token fixture pins the scores only: a window of 0 tokens sets every score to 1.0 (:247) and everything ties.

(b) tests/golden/fastkvzip_cases.npz.  For every bf16 / f16 kernel case of tests/_fastkvzip_inputs.py the reference's own gate on the CPU
in that dtype (one batch element at a time: its forward squeezes batch 0), and its max abs error against the float64 oracle as one number
per case: the library, which keeps float32 where the reference rounds to 16 bits twice, must not be the less accurate of the two."""
import sys

import gen_golden  # (next to this script) the generators' shared opening and closing


def main(argv):
    gen_golden.setup()
    import numpy as np
    import torch
    from kvpress.presses.fastkvzip_press import FastKVzipGate, FastKVzipPress  # the reference
    from transformers import DynamicCache

    import _fastkvzip_inputs as FI
    import _fastkvzip_oracle as FO
    import _inputs

    def inject_cache_position(module, args, kwargs):
        cache = kwargs["past_key_values"]
        past = cache.get_seq_length(module.layer_idx)
        q_len = kwargs["hidden_states"].shape[1]
        kwargs["cache_position"] = torch.arange(past, past + q_len)
        return args, kwargs

    def run_flow(spec, seed):
        model = _inputs.make_tiny_llama(dtype=torch.float32)
        hidden = {}

        def pre_hook(module, args, kwargs):
            hidden[int(module.layer_idx)] = kwargs["hidden_states"].detach().clone().numpy()
            return inject_cache_position(module, args, kwargs)

        for layer in model.model.layers:
            layer.self_attn.register_forward_pre_hook(pre_hook, with_kwargs=True)
        gates = FI.make_gates(FastKVzipGate, seed, model.config)
        state = FI.gates_state(gates)

        class SeededFastKVzipPress(FastKVzipPress):
            def post_init_from_model(self, model_):
                self.gates = gates

        press = SeededFastKVzipPress(compression_ratio=spec["compression_ratio"], layerwise=spec["layerwise"])
        ids = torch.from_numpy(FI.flow_ids(seed, spec["tokens"]))
        with torch.no_grad(), press(model):
            model.model(input_ids=ids, past_key_values=DynamicCache())
        score_val = press.score_val.detach().numpy()
        L = model.config.num_hidden_layers
        masked = [np.stack([t.numpy().astype(np.int64) for t in layer.self_attn.masked_key_indices]) for layer in model.model.layers]
        # the contract bound of these scores, from the hidden states the gates received
        bound = max(float(FO.fastkvzip_score(hidden[l], *FI.gate_arrays(state, l), FI.EPS)[1].max()) for l in range(L))
        out = dict(ids=ids.numpy(), seed=np.int64(seed), score_val=score_val, n_pruned=np.array([m.shape[1] for m in masked], np.int64), **state)
        out.update({f"masked_{l}": m for l, m in enumerate(masked)})
        out.update({f"hidden_{l}": hidden[l] for l in range(L)})
        return out, bound

    names = argv or list(FI.FLOW) + [FI.REFERENCE_ERROR_FIXTURE]
    for name in names:
        if name == FI.REFERENCE_ERROR_FIXTURE:
            continue
        spec = FI.FLOW[name]
        for seed in range(spec["seed"], spec["seed"] + 400, 10):     # (the specs' seeds are 1 apart: the searches never meet)
            out, bound = run_flow(spec, seed)
            if (out["score_val"] == 1.0).all():
                assert spec["tokens"] < 50, name
                print(f"{name}: seed {seed}: every score is 1.0 (a window of 0 tokens), scores pinned only")
                break
            gaps = FO.boundary_gaps(out["score_val"], spec["compression_ratio"], spec["layerwise"])
            need = 10 * 2 * bound
            if min(gaps) >= need:
                out["min_gap"] = np.float64(min(gaps))
                print(f"{name}: seed {seed}: boundary gaps {['%.3g' % g for g in gaps]} >= 10 x the contract bound = {need:.3g}; n_pruned {out['n_pruned'].tolist()}")
                break
            print(f"{name}: seed {seed} skipped: smallest boundary gap {min(gaps):.3g} < {need:.3g}")
        else:
            raise AssertionError(f"{name}: no seed with boundary gaps of 10 x the contract bound")
        head, tail = FO.protected_counts(spec["tokens"])
        assert (out["score_val"] == 1.0).sum() >= out["score_val"][..., 0].size * min(head + tail, spec["tokens"]) and out["score_val"].dtype == np.float32
        gen_golden.save(name, out)

    if FI.REFERENCE_ERROR_FIXTURE in names:
        errors = {}
        for case in FI.MFMA_CASES + FI.GENERIC_CASES:
            if case[0] == "f32":
                continue
            s = FI.score_case(case)
            dt = _inputs.torch_dtype(case[0])
            gate = FastKVzipGate(0, s["K"], s["Hkv"], s["G"], dt, s["D"], s["J"])
            gate.load_state_dict({"q_proj.weight": torch.from_numpy(s["wq"]).to(dt), "q_proj.bias": torch.from_numpy(s["bq"]).to(dt),
                                  "k_proj.weight": torch.from_numpy(s["wk"]).to(dt), "q_norm.weight": torch.from_numpy(s["gq"]),
                                  "k_norm.weight": torch.from_numpy(s["gk"]), "k_base": torch.from_numpy(s["kb"])[:, None],
                                  "b": torch.from_numpy(s["b"]).to(dt)[:, None]})
            assert gate.q_norm.variance_epsilon == FI.EPS
            with torch.no_grad():
                got = torch.cat([gate(torch.from_numpy(s["x"][i:i + 1]).to(dt)) for i in range(s["B"])]).double().numpy()
            ref, bound = FO.fastkvzip_score(*FI.oracle_args(s))
            errors[FI.case_id(case)] = np.float64(np.abs(got - ref).max())
            print(f"{FI.case_id(case)}: the reference's {case[0]} gate is {errors[FI.case_id(case)]:.3g} from float64 (contract bound {2 * bound.max():.3g})")
        gen_golden.save(FI.REFERENCE_ERROR_FIXTURE, errors)


if __name__ == "__main__":
    main(sys.argv[1:])
