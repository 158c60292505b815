"""Seeded inputs of the CriticalKV fixtures (tests/golden/crit_*.npz, oracle/gen_golden_critical.py): a cache, hidden states and q_proj
from _inputs.make_case, and the attention layer of _inputs.build_llama_attention, whose o_proj is seeded there.  Every number is exact
in the case's 16-bit dtype, so the reference's float32 run and its native run see the same inputs."""
from __future__ import annotations

import _inputs

# name -> case (fields as _inputs.CASES) + alpha: CriticalAdaKVPress.alpha_safeguard, fsr: first_stage_ratio of both presses.
# B = 1: the reference's CriticalAdaKVPress fails for larger batches (criticalkv_press.py:163-164, :176).
CASES = {
    "crit_knorm_s257_d16": dict(kind="knorm", B=1, H=2, G=2, S=257, D=16, dtype="bf16", data="B", seed=912, alpha=0.2, fsr=0.5, ratios=(0.3, 0.5)),
    "crit_snapkv_s700_d16": dict(kind="snapkv", B=1, H=2, G=2, S=700, D=16, dtype="f16", data="B", seed=902, W=8, ks=5, alpha=0.2, fsr=0.5,
                                 ratios=(0.5,)),
    # another first_stage_ratio and alpha; D = 64: the matrix-core path on a 16-bit module
    "crit_knorm_s300_d64_g4": dict(kind="knorm", B=1, H=2, G=4, S=300, D=64, dtype="bf16", data="B", seed=906, alpha=0.5, fsr=0.7, ratios=(0.4,)),
}
EPSILON = 1e-4   # the reference's default


def make_case(name: str) -> dict:
    _inputs.CASES[name] = {k: v for k, v in CASES[name].items() if k not in ("alpha", "fsr")}
    try:
        s = _inputs.make_case(name)
    finally:
        del _inputs.CASES[name]
    s["alpha"], s["fsr"] = CASES[name]["alpha"], CASES[name]["fsr"]
    return s


def inner_press(ns, s: dict, ratio: float):
    """the wrapped scorer of a case from namespace ``ns`` (the reference package or this one)"""
    if s["kind"] == "knorm":
        return ns.KnormPress(compression_ratio=ratio)
    return ns.SnapKVPress(compression_ratio=ratio, window_size=s["W"], kernel_size=s["ks"])


def wo_of(module):
    """o_proj.weight [hidden, Hq * D] of the seeded layer as float32 numpy"""
    return module.o_proj.weight.detach().float().cpu().numpy()
