#!/usr/bin/env python3
"""Reference outputs of MergingPress: runs the REAL reference (NVIDIA/kvpress, put on the path by oracle/gen_golden.py's shims, as the
oracle/gen_golden*.py scripts do) on the host CPU over the seeded inputs of tests/_merging_inputs.py and writes tests/golden/mrg_*.npz.

    PYTHONDONTWRITEBYTECODE=1 python oracle/gen_golden_merging.py [case ...]

Per case and run ("o32": module and tensors in float32; "nat": the case's model dtype): the kept indices in the reference's order
(descending score, `*_kept`), the nearest survivor and its cosine as the reference's merge() computed them (`*_target`, `*_max_sim`:
recorded from its `.max(dim=-1)` call while compress() runs) and the compressed V' it returns (`*_v`, float32).
"""
import sys

import gen_golden  # (next to this script) the generators' shared opening and closing


def main(argv):
    gen_golden.setup()
    import numpy as np
    import torch
    import kvpress  # the reference
    from kvpress import MergingPress

    import _inputs
    import _merging_inputs as MI

    class MaxRecorder:
        """records the (values, indices) of every Tensor.max(dim=-1) call: merge() makes exactly one (:139)"""

        def __init__(self):
            self.seen = []
            self.orig = torch.Tensor.max

        def __enter__(self):
            rec = self

            def mx(t, *a, **kw):
                r = rec.orig(t, *a, **kw)
                if kw.get("dim") == -1 and not a:
                    rec.seen.append((r.values.detach().clone(), r.indices.detach().clone()))
                return r
            torch.Tensor.max = mx
            return self

        def __exit__(self, *exc):
            torch.Tensor.max = self.orig

    for name in argv or list(MI.CASES):
        s = MI.make_case(name)
        out = {}
        for run, dt in (("o32", torch.float32), ("nat", _inputs.torch_dtype(s["dtype"]))):
            torch.manual_seed(s["seed"])
            module, hidden, kw = MI.module_and_kwargs(s, dt)
            keys = torch.from_numpy(s["keys"]).to(dt)
            values = torch.from_numpy(s["values"]).to(dt)
            press = MergingPress(MI.inner_press(s, kvpress), similarity_threshold=s["thr"], merge_fraction=s["frac"])
            with torch.no_grad():
                scores = press.press.score(module, hidden, keys, values, None, kw)
                n = int(s["S"] * (1 - s["ratio"]))
                kept = scores.topk(n, dim=-1).indices
                with MaxRecorder() as r:
                    k2, v2 = press.compress(module, hidden, keys, values, None, kw)
            assert len(r.seen) == (1 if 0 < n < s["S"] else 0), len(r.seen)
            out[f"{run}_kept"] = kept.numpy().astype(np.int32)
            if r.seen:
                out[f"{run}_max_sim"] = r.seen[0][0].float().numpy()
                out[f"{run}_target"] = r.seen[0][1].numpy().astype(np.int32)
            out[f"{run}_v"] = v2.float().numpy()
        gen_golden.save(name, out)


if __name__ == "__main__":
    main(sys.argv[1:])
