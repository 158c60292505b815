#!/usr/bin/env python3
"""Generate tests/golden/torch_path_pinned.json: the record() (digests) of the REAL reference's ``press.score()`` (float32 and
native dtype), ``compress()`` lengths and top-k indices of the float32 scores, for the cases of
tests/test_oracle_golden.py::test_torch_path_is_the_reference_op_for_op, on the pinned CPU backend of oracle/torch_path_pinned.py
(the same backend the test runs oracle/torch_path.py on, so that bit-for-bit equality means the same ops in the same order on any
machine).  Needs the reference package where gen_golden.py imports it (and its shims); test infrastructure only.

    PYTHONDONTWRITEBYTECODE=1 python oracle/gen_golden_torch_path.py
"""
import json
import os
import sys

import gen_golden  # (next to this script) the generators' shared opening and closing
import torch_path_pinned as TPP


def cases():
    import _inputs

    return [n for n in _inputs.CASES if _inputs.spec(n)["kind"] in ("knorm", "snapkv", "ea")
            and _inputs.spec(n)["use_covariance"] and _inputs.spec(n)["use_vnorm"] and _inputs.spec(n)["epsilon"] == 0.0]


def main():
    TPP.pin()
    gen_golden.setup()
    import numpy as np
    import torch
    from kvpress import ExpectedAttentionPress, KnormPress, SnapKVPress  # the reference

    import _inputs

    out = {}
    for name in cases():
        s = _inputs.make_case(name)

        def make_press(ratio):
            if s["kind"] == "knorm":
                return KnormPress(compression_ratio=ratio)
            if s["kind"] == "snapkv":
                return SnapKVPress(compression_ratio=ratio, window_size=s["W"], kernel_size=s["ks"])
            return ExpectedAttentionPress(compression_ratio=ratio, n_future_positions=s["n_future"], n_sink=s["n_sink"],
                                          use_covariance=s["use_covariance"], use_vnorm=s["use_vnorm"], epsilon=s["epsilon"])

        for mode, dt in (("f32", torch.float32), ("nat", _inputs.torch_dtype(s["dtype"]))):
            att, rot, hidden, pe = _inputs.build_llama_attention(s, dt)
            keys, values = torch.from_numpy(s["keys"]).to(dt), torch.from_numpy(s["values"]).to(dt)
            kwargs = {"position_embeddings": pe}
            with torch.no_grad():
                sc = make_press(0.5).score(att, hidden, keys, values, None, kwargs)
                out[TPP.key(name, f"scores_{mode}")] = sc.float().numpy()
                if mode == "f32":
                    for i, r in enumerate(s["ratios"]):
                        ko, vo = make_press(r).compress(att, hidden, keys, values, None, kwargs)
                        n = ko.shape[2]
                        out[TPP.key(name, f"nkept_{i}")] = np.int64(n)
                        out[TPP.key(name, f"idx_f32_{i}")] = sc.topk(n, dim=-1).indices.sort(dim=-1).values.numpy().astype(np.int32)
    path = os.path.join(gen_golden.GOLDEN, "torch_path_pinned.json")
    with open(path, "w") as f:   # one entry per line
        f.write("{\n" + ",\n".join(f"{json.dumps(k)}: {json.dumps(v)}" for k, v in TPP.record(out).items()) + "\n}\n")
    print(f"{len(cases())} cases: wrote {os.path.getsize(path)} bytes to {path}")


if __name__ == "__main__":
    if not TPP.pinned():
        sys.exit(TPP.run_pinned(os.path.abspath(__file__), sys.argv[1:]))
    main()
