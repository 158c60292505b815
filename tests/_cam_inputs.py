"""Seeded inputs of the CAMPress fixtures (tests/golden/cam_*.npz, oracle/gen_golden_cam.py): the cache of _merging_inputs, an attention
layer with q_proj and rotary tables from _inputs.build_llama_attention, and a running attention sum (rounded to the case's dtype, so
the float32 run and the native run of the reference see the same numbers)."""
from __future__ import annotations

import math

import numpy as np

import _inputs
import _merging_inputs as MI

# name -> case.  T: target_size; steps: decoding steps since the last compression (the number of merge candidates, clipped to S - T);
# m: merge_budget; G = Hq / H; zero_head: that kv head's running sum is all zero (every probability is 0 / 0 -> 0).
CASES = {
    "cam_b2_s160_d64_g2": dict(B=2, H=2, G=2, S=160, D=64, dtype="bf16", T=96, steps=40, m=8, zero_head=None, seed=701),
    "cam_s97_d128_g4": dict(B=1, H=2, G=4, S=97, D=128, dtype="f16", T=64, steps=50, m=32, zero_head=None, seed=702),      # steps > S - T
    "cam_s70_d6_f32": dict(B=1, H=2, G=2, S=70, D=6, dtype="f32", T=40, steps=10, m=100, zero_head=1, seed=703),           # m > T
}


def make_case(name: str) -> dict:
    s = dict(CASES[name], name=name, press="knorm", data="A")
    s["keys"], s["values"] = MI.make_keys_values(s["B"], s["H"], s["S"], s["D"], s["dtype"], "A", s["seed"])
    rs = np.random.RandomState(s["seed"] + 1000)
    s["Hq"] = s["H"] * s["G"]
    s["hsz"] = hsz = 64
    s["hidden"] = _inputs.round_to(rs.standard_normal((s["B"], s["S"], hsz)).astype(np.float32), s["dtype"])
    s["wq"] = _inputs.round_to((rs.standard_normal((s["Hq"] * s["D"], hsz)) / math.sqrt(hsz)).astype(np.float32), s["dtype"])
    # what a few hundred decoding steps leave: positive, a few large entries
    a = rs.gamma(0.5, 1.0, size=(s["B"], s["H"], s["S"])).astype(np.float32)
    if s["zero_head"] is not None:
        a[:, s["zero_head"]] = 0.0
    s["running"] = _inputs.round_to(a, s["dtype"])
    return s


def module_and_step(s: dict, dtype, device="cpu"):
    """(attention module, hidden states of the newest token [B,1,hsz], kwargs with its rotary row) of a decoding step at position S - 1"""
    att, rot, hidden, (cos, sin) = _inputs.build_llama_attention(s, dtype, device)
    return att, hidden[:, -1:], {"position_embeddings": (cos[:, -1:], sin[:, -1:])}
