#!/usr/bin/env python3
"""oracle/torch_path.py on a pinned CPU backend, for its bit-for-bit check against the REAL reference
(tests/test_oracle_golden.py::test_torch_path_is_the_reference_op_for_op).

The bits of a CPU matmul, reduction or softmax depend on the machine: MKL's and oneDNN's code path for the processor at hand,
ATen's vector width, the number of threads.  Scores of the reference taken on one machine are therefore not the bits the same
ops give on another.  Both sides of the check run on one backend that is the same everywhere: PINNED_ENV in the environment of
a fresh process (MKL and ATen read it when they load: MKL's conditional bitwise reproducibility on its generic code path,
ATen's scalar kernels), oneDNN off and one thread (pin()).  oracle/gen_golden_torch_path.py runs the reference that way and
keeps the record() of its arrays (SHA-256 of dtype, shape and bytes: equal digests are equal bits) in
tests/golden/torch_path_pinned.json; this script runs the restatement that way:

    python oracle/torch_path_pinned.py OUT.npz CASE [CASE ...]

Test infrastructure only (see oracle/kvpress_oracle.py header).
"""
import os
import subprocess
import sys

PINNED_ENV = {"MKL_CBWR": "COMPATIBLE,STRICT", "ATEN_CPU_CAPABILITY": "default", "OMP_NUM_THREADS": "1", "MKL_NUM_THREADS": "1"}


def pinned() -> bool:
    return all(os.environ.get(k) == v for k, v in PINNED_ENV.items())


def run_pinned(script: str, argv) -> int:
    """run `script argv` in a fresh process with PINNED_ENV (the variables only act before torch loads)"""
    return subprocess.run([sys.executable, script, *argv], env={**os.environ, **PINNED_ENV}).returncode


def pin():
    """the in-process half of the pinned backend; the process must have started with PINNED_ENV"""
    import torch

    assert pinned(), f"start this process with {PINNED_ENV} (they act only before torch loads)"
    torch.backends.mkldnn.enabled = False
    torch.set_num_threads(1)


def key(name: str, field: str) -> str:
    return f"{name}__{field}"


def record(arrays) -> dict:
    """{key: {"sha256", "shape", "sum"}} of arrays: the digest pins every bit (dtype, shape and bytes); the float64 sum only helps
    to read a mismatch"""
    import hashlib

    import numpy as np

    out = {}
    for k in sorted(arrays):
        a = np.ascontiguousarray(arrays[k])
        h = hashlib.sha256(f"{a.dtype.str}{a.shape}".encode())
        h.update(a.tobytes())
        out[k] = {"sha256": h.hexdigest(), "shape": list(a.shape), "sum": float(a.astype(np.float64).sum())}
    return out


def main(out: str, names) -> None:
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path[:0] = [repo, os.path.join(repo, "tests")]
    pin()
    import numpy as np
    import torch

    import _inputs
    from oracle import torch_path as TP

    res = {}
    for name in names:
        s = _inputs.make_case(name)
        for mode, dt in (("f32", torch.float32), ("nat", _inputs.torch_dtype(s["dtype"]))):
            att, rot, hidden, pe = _inputs.build_llama_attention(s, dt)
            keys, values = torch.from_numpy(s["keys"]).to(dt), torch.from_numpy(s["values"]).to(dt)
            kw = {"position_embeddings": pe}
            with torch.no_grad():
                if s["kind"] == "knorm":
                    sc = TP.knorm_score(att, hidden, keys, values, kw)
                elif s["kind"] == "snapkv":
                    sc = TP.snapkv_score(att, hidden, keys, values, kw, W=s["W"], ks=s["ks"])
                else:
                    sc = TP.ea_score(att, hidden, keys, values, kw, n_future=s["n_future"], n_sink=s["n_sink"])
                res[key(name, f"scores_{mode}")] = sc.float().numpy()
                if mode == "f32":
                    for i, r in enumerate(s["ratios"]):
                        ko, vo, idx = TP.torch_compress(lambda *a: sc, r, att, hidden, keys, values, kw)
                        res[key(name, f"nkept_{i}")] = np.int64(ko.shape[2])
                        res[key(name, f"idx_f32_{i}")] = np.sort(idx.numpy(), -1).astype(np.int32)
    np.savez(out, **res)


if __name__ == "__main__":
    if not pinned():
        sys.exit(run_pinned(os.path.abspath(__file__), sys.argv[1:]))
    main(sys.argv[1], sys.argv[2:])
