"""What more than one test module needs: fixture loading, dtype names, the merge tolerances, kept positions recovered from K' and the
tiny-Llama pipeline.  Plain functions and constants; the per-family inputs and oracles stay in tests/_X_inputs.py / _X_oracle.py."""
import os

import numpy as np

import _inputs
from _inputs import torch_dtype  # noqa: F401  ("f32" / "f16" / "bf16" -> torch.dtype; defined next to the cases that name dtypes)

GOLDEN_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
ULP = {"f32": 2.0 ** -23, "f16": 2.0 ** -10, "bf16": 2.0 ** -7}


def golden_path(name_with_suffix):
    return os.path.join(GOLDEN_DIR, name_with_suffix)


def golden(name):
    """the arrays of tests/golden/<name>.npz"""
    return dict(np.load(golden_path(name + ".npz")))


def dtype_name(dtype):
    """torch.dtype -> "f32" / "f16" / "bf16" (the inverse of torch_dtype)"""
    return next(n for n in ULP if torch_dtype(n) == dtype)


def merged_tol(ref, dt):
    """one unit in the last place of the dtype (a float32 model: a few float32 ulps, the sums run in float32 vs float64)"""
    if dt == "f32":
        return 64 * ULP[dt] * np.abs(ref) + 1e-7
    return ULP[dt] * np.maximum(np.abs(ref), 2.0 ** -14) * 1.0001


def ref_tol(ref_v, dt):
    # the reference's V' up to one unit in the last place of the dtype (its float32 cosines and sums run in another order: where
    # v' + sum(w v) cancels, that leaves a few 1e-7 absolute)
    return merged_tol(ref_v, dt) + 2e-6 * max(1.0, float(np.abs(ref_v).max(initial=0.0)))


def _float32_array(x):
    return np.ascontiguousarray(x if isinstance(x, np.ndarray) else x.detach().float().cpu().numpy(), dtype=np.float32)


def kept_positions(k_out, keys):
    """int64 [B,H,n]: the cache position of every row of K' [B,H,n,D] in keys [B,H,S,D], in K' order (numpy arrays or torch tensors).
    Rows match byte-wise, and every row of K' has to match exactly one cache row."""
    ko, k = _float32_array(k_out), _float32_array(keys)
    B, H, n, _ = ko.shape
    pos = np.zeros((B, H, n), np.int64)
    for b in range(B):
        for h in range(H):
            lut = {}
            for s in range(k.shape[2]):
                lut.setdefault(k[b, h, s].tobytes(), []).append(s)
            hits = [lut.get(r.tobytes(), []) for r in ko[b, h]]
            assert all(len(m) == 1 for m in hits), f"batch {b} head {h}: a row of K' matches {sorted({len(m) for m in hits})} cache rows"
            pos[b, h] = [m[0] for m in hits]
    return pos


def tiny_pipeline(device="cpu", dtype=None, eager=False):
    """the kv-press pipeline over the tiny random-init Llama"""
    from transformers import pipeline

    import kvpress_amd  # noqa: F401  (registers the task)

    model = _inputs.make_tiny_llama(dtype=dtype, device=device)
    if eager:
        model.config._attn_implementation = "eager"
    return pipeline("kv-press-text-generation", model=model, tokenizer=_inputs.make_tiny_tokenizer(), device=device)


def cache_sizes(cache):
    return [layer.keys.shape[2] for layer in cache.layers]
