#!/usr/bin/env python3
"""Reference outputs of CAMPress: runs the REAL reference (NVIDIA/kvpress, put on the path by oracle/gen_golden.py's shims) on the host CPU
over the seeded inputs of tests/_cam_inputs.py and writes tests/golden/cam_*.npz.

    PYTHONDONTWRITEBYTECODE=1 python oracle/gen_golden_cam.py [case ...]

Per case and run ("o32": module and tensors in float32; "nat": the case's model dtype), from one direct call of compress() with the
layer's step count and running attention sum preset: the kept and the merge-candidate positions (the two arguments of its
torch.searchsorted call), the merge probabilities and the mask (input and output of its torch.bernoulli call), K', V' and the pruned
running sum A' (`*_kept`, `*_cand`, `*_prob`, `*_mask`, `*_k`, `*_v`, `*_a`); and the per-step attention of the newest token from its
two static methods (`*_attn`, [B,Hkv,S]).
"""
import sys

import gen_golden  # (next to this script) the generators' shared opening and closing


def main(argv):
    gen_golden.setup()
    import numpy as np
    import torch
    from kvpress import CAMPress, KnormPress  # the reference

    import _cam_inputs as CI
    import _inputs

    class Recorder:
        """records the arguments and the result of every call of torch.<name> while compress() runs"""

        def __init__(self, name):
            self.name, self.seen, self.orig = name, [], getattr(torch, name)

        def __enter__(self):
            def fn(*a, **kw):
                r = self.orig(*a, **kw)
                self.seen.append(([x.detach().clone() for x in a if torch.is_tensor(x)], r.detach().clone()))
                return r
            setattr(torch, self.name, fn)
            return self

        def __exit__(self, *exc):
            setattr(torch, self.name, self.orig)

    for name in argv or list(CI.CASES):
        s = CI.make_case(name)
        out = {}
        for run, dt in (("o32", torch.float32), ("nat", _inputs.torch_dtype(s["dtype"]))):
            torch.manual_seed(s["seed"])
            module, hidden, kw = CI.module_and_step(s, dt)
            keys = torch.from_numpy(s["keys"]).to(dt)
            values = torch.from_numpy(s["values"]).to(dt)
            running = torch.from_numpy(s["running"]).to(dt)
            with torch.no_grad():
                attn = CAMPress._compute_current_token_attention(module, hidden, keys, kw)
                out[f"{run}_attn"] = CAMPress._aggregate_attention_per_kv_head(attn, s["H"]).squeeze(2).float().numpy()
                press = CAMPress(base_press=KnormPress(), compression_interval=s["steps"], target_size=s["T"], merge_budget=s["m"])
                press.layer_step_counts[0] = s["steps"]
                press._running_attn_sum[0] = running.clone()
                if run == "o32":   # the kept sets compare exactly only without ties among the head-mean scores
                    mean = press.base_press.score(module, hidden, keys, values, None, kw).mean(dim=1)
                    assert all(len(np.unique(r)) == r.size for r in mean.numpy()), f"{name}: tied head-mean scores"
                with Recorder("searchsorted") as ss, Recorder("bernoulli") as bn:
                    k2, v2 = press.compress(module, hidden, keys.clone(), values.clone(), running.clone(), kw)   # (it writes into values)
            assert len(ss.seen) == 1 and len(bn.seen) == 1, (len(ss.seen), len(bn.seen))
            out[f"{run}_kept"] = ss.seen[0][0][0].numpy().astype(np.int32)
            out[f"{run}_cand"] = ss.seen[0][0][1].numpy().astype(np.int32)
            out[f"{run}_prob"] = bn.seen[0][0][0].float().numpy()
            out[f"{run}_mask"] = bn.seen[0][1].float().numpy()
            out[f"{run}_k"] = k2.float().numpy()
            out[f"{run}_v"] = v2.float().numpy()
            out[f"{run}_a"] = press._running_attn_sum[0].float().numpy()
        gen_golden.save(name, out)


if __name__ == "__main__":
    main(sys.argv[1:])
