#!/usr/bin/env python3
"""Reference outputs of CriticalKVPress / CriticalAdaKVPress: runs the REAL reference (NVIDIA/kvpress, put on the path by
oracle/gen_golden.py's shims) on the host CPU over the seeded inputs of tests/_critical_inputs.py and writes tests/golden/crit_*.npz.

    PYTHONDONTWRITEBYTECODE=1 python oracle/gen_golden_critical.py [case ...]

Per case, from the run with module and tensors in float32: `norm` (CriticalKVPress.vwl1norm, [B,H,S]) and `inner` (the wrapped press's
scores); per ratio i `crit_scores_<i>` (CriticalKVPress.score) and `crit_pos_<i>` (the positions its compress() keeps, sorted, int32
[B,H,n]); `ada_budgets_<i>` (the head budgets, the result of the reference's scatter_add_ at :164) and `ada_masked_<i>` (sorted flat
indices head * S + position of module.masked_key_indices, B = 1).  From the run on the native 16-bit module: `nat_norm` and
`nat_crit_scores_<i>`, stored as float32.

The comparisons of tests/test_critical_host.py and tests/test_gpu_critical.py are exact outside the bands of tests/_critical_oracle.py;
asserted here, on the reference's own numbers: per head and selection at most 1 % of the positions lie in its band, and the flattened budget selection
has a relative gap above 1e-4 at its threshold (the budgets then compare exactly).
"""
import sys

import gen_golden  # (next to this script) the generators' shared opening and closing


def main(argv):
    gen_golden.setup()
    import numpy as np
    import torch
    import kvpress as R   # the reference

    import _critical_inputs as CI
    import _critical_oracle as CO
    import _inputs

    class BudgetRecorder:
        """records the result of every Tensor.scatter_add_ while compress() runs (the head budgets, :163-164)"""

        def __enter__(self):
            self.seen, self.orig = [], torch.Tensor.scatter_add_
            rec = self

            def fn(t, *a, **kw):
                r = rec.orig(t, *a, **kw)
                rec.seen.append(r.detach().clone())
                return r
            torch.Tensor.scatter_add_ = fn
            return self

        def __exit__(self, *exc):
            torch.Tensor.scatter_add_ = self.orig

    for name in argv or list(CI.CASES):
        s = CI.make_case(name)
        assert s["B"] == 1, "the reference's CriticalAdaKVPress fails for B > 1"
        S, H = s["S"], s["H"]
        out = {"ratios": np.asarray(s["ratios"], dtype=np.float64)}
        for run, dt in (("f32", torch.float32), ("nat", _inputs.torch_dtype(s["dtype"]))):
            att, rot, hidden, pe = _inputs.build_llama_attention(s, dt)
            att.config._attn_implementation = "sdpa"
            keys = torch.from_numpy(s["keys"]).to(dt)
            values = torch.from_numpy(s["values"]).to(dt)
            kw = {"position_embeddings": pe}
            with torch.no_grad():
                norm = R.CriticalKVPress.vwl1norm(values, att)
                if run == "nat":
                    out["nat_norm"] = norm.float().numpy()
                    for i, r in enumerate(s["ratios"]):
                        p = R.CriticalKVPress(CI.inner_press(R, s, r), epsilon=CI.EPSILON, first_stage_ratio=s["fsr"])
                        out[f"nat_crit_scores_{i}"] = p.score(att, hidden, keys, values, None, kw).float().numpy()
                    continue
                out["norm"] = norm.numpy()
                inner = CI.inner_press(R, s, s["ratios"][0]).score(att, hidden, keys, values, None, kw).numpy()
                out["inner"] = inner
                for i, r in enumerate(s["ratios"]):
                    n_kept = int(S * (1 - r))
                    p = R.CriticalKVPress(CI.inner_press(R, s, r), epsilon=CI.EPSILON, first_stage_ratio=s["fsr"])
                    sc = p.score(att, hidden, keys, values, None, kw)
                    ko, _ = p.compress(att, hidden, keys, values, None, kw)
                    assert ko.shape[2] == n_kept
                    out[f"crit_scores_{i}"] = sc.numpy()
                    out[f"crit_pos_{i}"] = sc.topk(n_kept, dim=-1).indices.sort(dim=-1).values.numpy().astype(np.int32)
                    for h in range(H):   # the two selections of a head: stage 1 on the inner scores, the final top-k
                        for row, k in ((inner[0, h], int((1 - r) * S * s["fsr"])), (sc.numpy()[0, h], n_kept)):
                            nb = int(CO._band(row.astype(np.float64), k).sum())
                            assert nb <= 0.01 * S, f"{name} r={r} head {h}: {nb} of {S} positions within 1e-3 of a CriticalKV threshold"

                    p = R.CriticalAdaKVPress(CI.inner_press(R, s, r), alpha_safeguard=s["alpha"], epsilon=CI.EPSILON, first_stage_ratio=s["fsr"])
                    with BudgetRecorder() as rec:
                        p.compress(att, hidden, keys, values, None, kw)
                    assert len(rec.seen) == 1 and int(rec.seen[0].sum()) == n_kept * H
                    bi, hi, si = att.masked_key_indices
                    assert int(bi.max()) == 0 and hi.numel() == H * (S - n_kept)
                    out[f"ada_budgets_{i}"] = rec.seen[0].numpy().astype(np.int64)
                    out[f"ada_masked_{i}"] = np.sort((hi * S + si).numpy()).astype(np.int32)
                    a = CO.critical_ada(inner, norm.numpy(), r, s["alpha"], s["fsr"], CI.EPSILON)
                    assert a["band_max"] <= 0.01 * S, f"{name} r={r}: {a['band_max']} of {S} positions within 1e-3 of a CriticalAdaKV threshold"
                    assert a["budget_gap"].min() > 1e-4, f"{name} r={r}: budget threshold gap {a['budget_gap']}"
        gen_golden.save(name, out)


if __name__ == "__main__":
    main(sys.argv[1:])
