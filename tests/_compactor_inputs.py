"""Seeded inputs of the Compactor-family fixtures (tests/golden/cpt_*.npz, oracle/gen_golden_compactor.py): the attention layer of
_inputs.build_llama_attention with its k_proj seeded as well (that helper leaves it to torch's init)."""
from __future__ import annotations

import math

import numpy as np

import _inputs

# name -> geometry.  G = Hq / H.  sinks = (sink_size_start, sink_size_end) of CompactorPress.
CASES = {
    "cpt_s256_c128_d64_g4": dict(B=1, H=2, G=4, S=256, D=64, chunk=128, sketch=48, sinks=(0, 0), dtype="bf16", seed=501),
    "cpt_s300_c128_d128_g1": dict(B=1, H=2, G=1, S=300, D=128, chunk=128, sketch=64, sinks=(1, 1), dtype="f16", seed=502),
    "cpt_s200_c256_d128_g8": dict(B=1, H=1, G=8, S=200, D=128, chunk=256, sketch=48, sinks=(8, 4), dtype="bf16", seed=503),
    "cpt_b2_s333_c64_d96_g4": dict(B=2, H=2, G=4, S=333, D=96, chunk=64, sketch=48, sinks=(8, 4), dtype="bf16", seed=504),
    "cpt_s257_c256_d256_g4_f32": dict(B=1, H=2, G=4, S=257, D=256, chunk=256, sketch=64, sinks=(1, 1), dtype="f32", seed=505),
}
RATIOS = (0.25, 0.5)


def make_case(name: str, **override) -> dict:
    s = dict(CASES[name], name=name)
    s.update(override)
    rs = np.random.RandomState(s["seed"])
    Hq, D = s["H"] * s["G"], s["D"]
    s["Hq"] = Hq
    s["hsz"] = hsz = 64 if D < 128 else 128
    s["hidden"] = _inputs.round_to(rs.standard_normal((s["B"], s["S"], hsz)).astype(np.float32), s["dtype"])
    s["wq"] = _inputs.round_to((rs.standard_normal((Hq * D, hsz)) / math.sqrt(hsz)).astype(np.float32), s["dtype"])
    s["wk"] = _inputs.round_to((rs.standard_normal((s["H"] * D, hsz)) / math.sqrt(hsz)).astype(np.float32), s["dtype"])
    s["values"] = _inputs.round_to(rs.standard_normal((s["B"], s["H"], s["S"], D)).astype(np.float32), s["dtype"])
    return s


def build_attention(s: dict, dtype, device="cpu"):
    """build_llama_attention + the seeded k_proj; returns (module, hidden, (cos, sin))."""
    import torch

    att, rot, hidden, pe = _inputs.build_llama_attention(s, dtype, device)
    with torch.no_grad():
        att.k_proj.weight.copy_(torch.from_numpy(s["wk"]).to(device=device, dtype=dtype))
    return att, hidden, pe


def post_rope_keys(att, hidden, pe):
    """The cache's keys: k_proj + RoPE as LlamaAttention.forward computes them."""
    import torch
    from transformers.models.llama.modeling_llama import apply_rotary_pos_emb

    B, S, _ = hidden.shape
    with torch.no_grad():
        k = att.k_proj(hidden).view(B, S, -1, att.head_dim).transpose(1, 2)
        q = att.q_proj(hidden).view(B, S, -1, att.head_dim).transpose(1, 2)
        _, k = apply_rotary_pos_emb(q, k, *pe)
    return k


def phi_from_draw(draw, sketch: int, dtype):
    """The reference's Phi from its raw torch.randn draw (leverage_press.py:68-75): ``draw * (1 / sqrt(k))`` in the draw's dtype
    (the fixtures' ``*_phi_draw`` arrays are that draw; float32 arrays hold bf16 / f16 draws exactly).  numpy float32 array out."""
    import torch

    t = torch.as_tensor(draw).to(dtype) * (1 / math.sqrt(sketch))
    return t.float().numpy()
