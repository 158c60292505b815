"""Seeded inputs of the MergingPress fixtures (tests/golden/mrg_*.npz, oracle/gen_golden_merging.py): cache keys / values drawn with
numpy's frozen RandomState (rounded to the case's dtype, so both runs see the same numbers) and, for SnapKV, the attention layer of
_inputs.build_llama_attention."""
from __future__ import annotations

import math

import numpy as np

import _inputs

# name -> case.  press: the inner ScorerPress (knorm | snapkv | keydiff); G = Hq / H; data: "A" N(0, 1) keys, "dup" keys that are
# power-of-two multiples of a few directions (exact cosine ties), "zero" one all-zero key per head and some all-zero values,
# "nanq" head 0 clustered (every similarity passes), the other heads random (every one fails: a NaN quantile row).
CASES = {
    "mrg_knorm_b2_s333_d128": dict(press="knorm", B=2, H=2, G=1, S=333, D=128, dtype="bf16", data="A", ratio=0.5, thr=0.0, frac=1.0, seed=601),
    "mrg_snapkv_s300_d64_g4": dict(press="snapkv", B=1, H=2, G=4, S=300, D=64, dtype="f16", data="A", ratio=0.6, thr=0.1, frac=0.75, seed=602),
    "mrg_keydiff_s157_d256_f32": dict(press="keydiff", B=1, H=2, G=1, S=157, D=256, dtype="f32", data="zero", ratio=0.3, thr=0.0, frac=0.3,
                                      seed=603),
    "mrg_knorm_dup_s96_d64": dict(press="knorm", B=1, H=2, G=1, S=96, D=64, dtype="bf16", data="dup", ratio=0.5, thr=0.0, frac=1.0, seed=604),
    "mrg_knorm_nanq_s200_d128": dict(press="knorm", B=1, H=2, G=1, S=200, D=128, dtype="bf16", data="nanq", ratio=0.5, thr=0.3, frac=0.3,
                                     seed=605),
    "mrg_snapkv_b2_s333_d128_g2": dict(press="snapkv", B=2, H=2, G=2, S=333, D=128, dtype="bf16", data="A", ratio=0.25, thr=0.0, frac=1.0,
                                       seed=606),
    "mrg_knorm_nkept0_s20_d64": dict(press="knorm", B=1, H=2, G=1, S=20, D=64, dtype="bf16", data="A", ratio=0.96, thr=0.0, frac=1.0, seed=607),
}


def make_keys_values(B, H, S, D, dtype, data, seed):
    rs = np.random.RandomState(seed)
    k = rs.standard_normal((B, H, S, D)).astype(np.float32)
    v = rs.standard_normal((B, H, S, D)).astype(np.float32)
    if data == "dup":
        dirs = _inputs.round_to(rs.standard_normal((B, H, 6, D)).astype(np.float32), dtype)
        pick = rs.randint(0, 6, size=(B, H, S))
        scale = 2.0 ** rs.randint(-2, 3, size=(B, H, S, 1))
        k = np.take_along_axis(dirs, pick[..., None].repeat(D, -1), axis=2) * scale.astype(np.float32)
    elif data == "zero":
        for b in range(B):
            for h in range(H):
                k[b, h, rs.randint(0, S)] = 0.0
        v[:, :, rs.randint(0, S, size=S // 8)] = 0.0
    elif data == "nanq":
        base = rs.standard_normal((B, 1, 1, D)).astype(np.float32)
        k[:, :1] = base + 0.3 * k[:, :1]
    return _inputs.round_to(k, dtype), _inputs.round_to(v, dtype)


def make_case(name: str, **override) -> dict:
    s = dict(CASES[name], name=name)
    s.update(override)
    s["keys"], s["values"] = make_keys_values(s["B"], s["H"], s["S"], s["D"], s["dtype"], s["data"], s["seed"])
    if s["press"] == "snapkv":
        rs = np.random.RandomState(s["seed"] + 1000)
        s["Hq"] = s["H"] * s["G"]
        s["hsz"] = hsz = 64
        s["hidden"] = _inputs.round_to(rs.standard_normal((s["B"], s["S"], hsz)).astype(np.float32), s["dtype"])
        s["wq"] = _inputs.round_to((rs.standard_normal((s["Hq"] * s["D"], hsz)) / math.sqrt(hsz)).astype(np.float32), s["dtype"])
    return s


def inner_press(s: dict, lib):
    """The case's inner ScorerPress from ``lib`` (the reference's kvpress or kvpress_amd)."""
    if s["press"] == "knorm":
        return lib.KnormPress(s["ratio"])
    if s["press"] == "snapkv":
        return lib.SnapKVPress(s["ratio"], window_size=32, kernel_size=5)
    return lib.KeyDiffPress(s["ratio"])


def module_and_kwargs(s: dict, dtype, device="cpu"):
    """(module, hidden_states, kwargs) that the inner press's score() is called with."""
    import torch

    if s["press"] == "snapkv":
        att, rot, hidden, pe = _inputs.build_llama_attention(s, dtype, device)
        return att, hidden, {"position_embeddings": pe}

    class _M(torch.nn.Module):
        pass

    m = _M()
    m.head_dim = s["D"]
    m.layer_idx = 0
    return m, torch.zeros((s["B"], s["S"], 8), dtype=dtype, device=device), {}
