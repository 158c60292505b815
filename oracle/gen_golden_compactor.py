#!/usr/bin/env python3
"""Reference outputs of the Compactor family (NonCausalAttnPress, LeverageScorePress, CompactorPress): runs the REAL reference
(NVIDIA/kvpress, put on the path by oracle/gen_golden.py's shims, as the oracle/gen_golden*.py scripts do) on the host CPU over the seeded inputs of
tests/_compactor_inputs.py and writes tests/golden/cpt_*.npz.

    PYTHONDONTWRITEBYTECODE=1 python oracle/gen_golden_compactor.py [case ...]

Per case and run ("o32": module and tensors in float32; "nat": the case's model dtype): the sketch the reference drew (recorded by
wrapping torch.randn: the raw draw `*_phi_draw`, BEFORE the reference's `* (1 / sqrt(k))`; tests/_compactor_inputs.phi_from_draw
applies that scaling exactly as leverage_press.py:68-75 does, and a test that injects the draw as torch.randn's result reproduces Phi), the raw and z-scored scores of NonCausalAttn and Leverage, CompactorPress's scores and the positions its
compress() keeps per ratio.
"""
import sys

import gen_golden  # (next to this script) the generators' shared opening and closing


def main(argv):
    gen_golden.setup()
    import numpy as np
    import torch
    import torch.nn.functional as F
    from kvpress import CompactorPress, LeverageScorePress, NonCausalAttnPress  # the reference
    from kvpress.utils import get_prerope_key_states, get_prerope_query_states
    from transformers.models.llama.modeling_llama import repeat_kv, rotate_half

    import _compactor_inputs as CI
    import _inputs

    class Recorder:
        def __init__(self):
            self.drawn = []
            self.orig = torch.randn

        def __enter__(self):
            def randn(*a, **kw):
                t = self.orig(*a, **kw)
                self.drawn.append(t.detach().clone())
                return t
            torch.randn = randn
            return self

        def __exit__(self, *exc):
            torch.randn = self.orig

    for name in argv or list(CI.CASES):
        s = CI.make_case(name)
        out = {}
        for run, dt in (("o32", torch.float32), ("nat", _inputs.torch_dtype(s["dtype"]))):
            torch.manual_seed(s["seed"])
            att, hidden, (cos, sin) = CI.build_attention(s, dt)
            keys = CI.post_rope_keys(att, hidden, (cos, sin))
            values = torch.from_numpy(s["values"]).to(dt)
            kw = {"position_embeddings": (cos, sin)}
            with torch.no_grad():
                # NonCausalAttnPress: raw (the reference's lines :109-120 around its own non_causal_chunked_attn) and z-scored
                q = get_prerope_query_states(att, hidden)
                qr = (q * cos.unsqueeze(1)) + (rotate_half(q) * sin.unsqueeze(1))
                G = q.shape[1] // values.shape[1]
                A = NonCausalAttnPress.non_causal_chunked_attn(qr, repeat_kv(keys, G), s["chunk"])
                A = A.view(A.shape[0], values.shape[1], -1, A.shape[-1]).mean(dim=-2)
                raw = F.avg_pool1d(A * values.norm(dim=-1), kernel_size=3, padding=1, stride=1)
                nc = NonCausalAttnPress(0.5, chunk_size=s["chunk"])
                out[f"{run}_nc_raw"] = raw.float().numpy()
                out[f"{run}_nc_z"] = nc.score(att, hidden, keys, values, None, kw).float().numpy()
                # LeverageScorePress
                kpre = get_prerope_key_states(att, hidden)
                with Recorder() as r:
                    lraw = LeverageScorePress.compute_leverage_scores(kpre, s["sketch"])
                # the raw draw (Phi = draw * (1 / sqrt(k)) in the draw's dtype: _compactor_inputs.phi_from_draw)
                out[f"{run}_lev_phi_draw"] = r.drawn[0].float().numpy()
                out[f"{run}_lev_raw"] = lraw.float().numpy()
                out[f"{run}_lev_z"] = ((lraw - lraw.mean()) / lraw.std().clamp_min(1e-6)).float().numpy()
                # CompactorPress: scores and kept positions
                for ratio in CI.RATIOS:
                    p = CompactorPress(ratio, sink_size_start=s["sinks"][0], sink_size_end=s["sinks"][1], chunk_size=s["chunk"],
                                       sketch_dimension=s["sketch"])
                    with Recorder() as r:
                        sc = p.score(att, hidden, keys, values, None, kw)
                    tag = f"{run}_cpt_r{int(ratio * 100)}"
                    out[tag + "_phi_draw"] = r.drawn[0].float().numpy()
                    out[tag + "_scores"] = sc.float().numpy()
                    n = int(s["S"] * (1 - ratio))
                    out[tag + "_kept"] = np.sort(sc.float().topk(n, dim=-1).indices.numpy(), axis=-1).astype(np.int32)
        gen_golden.save(name, out)


if __name__ == "__main__":
    main(sys.argv[1:])
