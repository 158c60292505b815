"""The FastKVzipPress flow of the fixtures (tests/golden/fastkvzip_flow_*.npz), shared by the host test (oracle-backed entry points, CPU)
and the GPU test (the library): the same model, ids and gate weights as oracle/gen_golden_fastkvzip.py used for the REAL reference."""
import numpy as np
import torch

import _fastkvzip_inputs as FI
import _fastkvzip_oracle as FO
import _inputs
from _support import golden


def triples_set(triples):
    return set(zip(*(np.asarray(t).tolist() for t in triples)))


def run_flow(name, device):
    """the prefill under this package's FastKVzipPress with the fixture's gates; returns the press, the model, the fixture, score_val and
    per layer the masked triples"""
    from transformers import DynamicCache

    from kvpress_amd.presses.fastkvzip_press import FastKVzipPress

    spec, g = FI.FLOW[name], golden(name)
    model = _inputs.make_tiny_llama(dtype=torch.float32, device=device)
    press = FastKVzipPress(compression_ratio=spec["compression_ratio"], layerwise=spec["layerwise"])
    press.gates = [gate.to(device) for gate in FI.load_gates(g, model.config)]
    with torch.no_grad(), press(model):
        model.model(input_ids=torch.from_numpy(g["ids"]).to(device), past_key_values=DynamicCache())
    if device != "cpu":
        torch.cuda.synchronize()
    masked = []
    for layer in model.model.layers:
        m = layer.self_attn.masked_key_indices
        assert len(m) == 3 and all(t.dtype == torch.int64 and t.device.type == torch.device(device).type for t in m)
        masked.append(tuple(t.cpu().numpy() for t in m))
    return dict(press=press, model=model, fixture=g, spec=spec, score_val=press.score_val.detach().cpu().numpy(), masked=masked)


def check_flow_against_fixture(name, device):
    """score_val within 2 x bound of the float64 oracle on the reference's hidden states AND within 2 x bound of the reference's own
    scores, protected positions exactly 1.0, masked SETS and n_pruned per layer equal to the reference's
    (the fixture's boundary gaps are 10 x the contract bound).  The 40-token fixture: every score 1.0, nothing else is decided."""
    rec = run_flow(name, device)
    g, spec, sv = rec["fixture"], rec["spec"], rec["score_val"]
    L = len(rec["masked"])
    assert sv.dtype == np.float32 and sv.shape == g["score_val"].shape == (L, 1, 2, spec["tokens"])
    head, tail = FO.protected_counts(spec["tokens"])
    worst = 0.0
    for l in range(L):
        ref, bound = FO.fastkvzip_score(g[f"hidden_{l}"], *FI.gate_arrays(g, l), FI.EPS)
        prot = FO.protect(ref, head, tail)
        assert np.array_equal(sv[l] == 1.0, prot == 1.0) or spec["tokens"] < 50
        worst = max(worst, FO.worst_ratio(sv[l], prot, bound), FO.worst_ratio(sv[l], g["score_val"][l].astype(np.float64), bound))
    print(f"{name} on {device}: worst score error {worst:.3g} of the contract bound 2 x bound")
    assert worst <= 1.0
    if spec["tokens"] < 50:
        assert (sv == 1.0).all() and (g["score_val"] == 1.0).all()
        assert [len(m[0]) for m in rec["masked"]] == g["n_pruned"].tolist() or sum(len(m[0]) for m in rec["masked"]) == int(g["n_pruned"].sum())
        return rec
    for l in range(L):
        assert len(rec["masked"][l][0]) == int(g["n_pruned"][l]), f"{name}: layer {l}: n_pruned differs"
        assert triples_set(rec["masked"][l]) == triples_set(g[f"masked_{l}"]), f"{name}: layer {l}: masked sets differ"
        assert len(triples_set(rec["masked"][l])) == int(g["n_pruned"][l]), f"{name}: layer {l}: a triple is listed twice"
    return rec
