#!/usr/bin/env python3
"""Reference outputs of KVzipPress: runs the REAL reference (NVIDIA/kvpress, put on the path by oracle/gen_golden.py's shims) on the host
CPU over the tiny float32 Llama of tests/_inputs.py and the seeded contexts of tests/_kvzip_inputs.py and writes
tests/golden/kvzip_*.npz.

    PYTHONDONTWRITEBYTECODE=1 python oracle/gen_golden_kvzip.py [case ...]

AutoTokenizer.from_pretrained is patched to return the in-memory word-level tokenizer (no hub), `prepare` is bound to
chunk_size = 64 (150 context tokens: 3 chunks, the last one partial).  Per case: `context_ids` [1,150]; the chunk pairs the reference
prepared (`n_pairs`, `prefill_<i>`, `repeat_<i>`); `score_val` [L,1,H,150] as compress_post saw it; `n_pruned_layers` [L]; the masked
triples of every layer (`masked_head_<l>`, `masked_seq_<l>`; the batch index is 0).

Band condition (on the inputs, checked here): at most 1 % of a layer's pruned entries lie within 1e-3 relative of that layer's selection
threshold, and at most 1 % of all pruned entries within 1e-3 of the cross-layer threshold.  The context's seed is chosen so that the
reference alone meets it -- where it can be met at all.  On this model it cannot for layer 0: the tokenizer knows none of the prompt's
words, every one becomes <unk> = id 0 = the model's pad id, whose embedding row is zero, so the first rows of every repeated input have
all-zero queries in layer 0, their attention is exactly uniform and, with the fewest visible keys, they win every column's maximum: the
reference's layer-0 scores are the census 1 / (sink + chunk + 1), bit-equal over a whole chunk (64, 64 and 22 columns x 2 heads: three
values in all), whatever the context.  A threshold inside such a group is an exact tie of the reference's own float32 scores, not
a near miss.  Entries BIT-EQUAL to a threshold are therefore counted apart (`tied_at_threshold` [L], `tied_at_global_threshold`): the
1 % condition holds for the entries that are within 1e-3 of a threshold WITHOUT being equal to it, in every layer, and literally (ties
included) wherever a threshold is not tied.  Which members of a tied group are pruned is torch.topk's choice in the reference and the lowest
positions' here; the counts do not depend on it (a group lies within one layer).  With KVzip+ the same zero rows have ||h|| = 0: the
reference's layer-0 scores are all +inf, nothing of layer 0 is pruned and all of layer 1 is.
"""
import functools
import sys

import gen_golden  # (next to this script) the generators' shared opening and closing


def main(argv):
    gen_golden.setup()
    import numpy as np
    import torch
    from kvpress.presses import kvzip_press as R  # the reference
    from transformers import DynamicCache

    import _inputs
    import _kvzip_inputs as KI
    import _kvzip_oracle as KO

    tokenizer = _inputs.make_tiny_tokenizer()
    R.AutoTokenizer.from_pretrained = staticmethod(lambda *a, **kw: tokenizer)
    # an empty text (the tokenizer has no chat template and "\n" holds no word) must still give integer ids
    encode = tokenizer.encode

    def encode_long(text, **kw):
        ids = encode(text, **kw)
        return ids.reshape(1, -1).to(torch.long) if torch.is_tensor(ids) else ids

    tokenizer.encode = encode_long

    for name in argv or list(KI.FIXTURES):
        spec = KI.FIXTURES[name]
        torch.manual_seed(0)
        model = _inputs.make_tiny_llama(dtype=torch.float32)
        ids = torch.from_numpy(KI.context_ids(spec["seed"]))
        press = R.KVzipPress(**spec["press"])
        seen = {}
        prepare = functools.partial(R.KVzipPress.prepare, press, chunk_size=KI.CHUNK)

        def recording_prepare(model_, tokenizer_):
            seen["pairs"] = prepare(model_, tokenizer_)
            return seen["pairs"]

        compress_post = press.compress_post

        def recording_compress_post(model_):
            seen["score_val"] = press.score_val.detach().clone()
            return compress_post(model_)

        press.prepare, press.compress_post = recording_prepare, recording_compress_post
        cache = DynamicCache()
        with torch.no_grad(), press(model):
            model.model(input_ids=ids, past_key_values=cache)
        assert [layer.keys.shape[2] for layer in cache.layers] == [KI.CONTEXT_TOKENS] * 2, "the cache was not cut back to the context"

        sv = seen["score_val"].float().numpy()
        L, _, H, C = sv.shape
        out = dict(context_ids=ids.numpy(), score_val=sv, n_pairs=np.int64(len(seen["pairs"])))
        for i, (a, r) in enumerate(seen["pairs"]):
            out[f"prefill_{i}"], out[f"repeat_{i}"] = a.numpy().astype(np.int64), r.numpy().astype(np.int64)
        counts = []
        for l, layer in enumerate(model.model.layers):
            b, h, s = layer.self_attn.masked_key_indices
            assert int(b.abs().sum()) == 0
            out[f"masked_head_{l}"], out[f"masked_seq_{l}"] = h.numpy().astype(np.int32), s.numpy().astype(np.int32)
            counts.append(len(h))
        out["n_pruned_layers"] = np.asarray(counts, np.int64)

        # the band condition, and the oracle's selection next to the reference's
        o = KO.compress_post(sv, spec["press"]["compression_ratio"], spec["press"].get("layerwise", False))
        assert list(o["counts"]) == counts, (list(o["counts"]), counts)
        flat = sv.reshape(L, -1).astype(np.float64)
        refs = [out[f"masked_head_{l}"].astype(np.int64) * C + out[f"masked_seq_{l}"] for l in range(L)]
        tied, near = [], []
        for l in range(L):
            tied.append(int((flat[l] == o["thr"][l]).sum()) if counts[l] else 0)
            near.append(int((o["bands"][l] & (flat[l] != o["thr"][l]))[refs[l]].sum()) + min(tied[l], 1))
            assert tied[l] > 1 or near[l] <= 0.01 * max(counts[l], 1), f"{name} layer {l}: {near[l]} of {counts[l]} pruned entries within 1e-3 of the layer's threshold"
            assert near[l] - 1 <= 0.01 * max(counts[l], 1), f"{name} layer {l}: {near[l] - 1} pruned entries near the tied threshold"
            assert KO.sets_equal_outside(o["pruned"][l], refs[l], o["bands"][l] | o["global_band"][l]), f"{name} layer {l}: the oracle's selection differs outside the bands"
        gtied = int((flat == o["global_thr"]).sum())
        gnear = int(sum((o["global_band"][l] & (flat[l] != o["global_thr"]))[refs[l]].sum() for l in range(L))) + min(gtied, 1)
        assert gnear - (gtied > 1) <= 0.01 * sum(counts), f"{name}: {gnear} of {sum(counts)} pruned entries within 1e-3 of the global threshold"
        out["tied_at_threshold"], out["tied_at_global_threshold"] = np.asarray(tied, np.int64), np.int64(gtied)
        print(f"{name}: n_pruned_layers {counts}; pruned entries within 1e-3 of the layer thresholds {near} (bit-equal to them: {tied}), of the "
              f"global threshold {gnear} (bit-equal: {gtied})")
        gen_golden.save(name, out)


if __name__ == "__main__":
    main(sys.argv[1:])
