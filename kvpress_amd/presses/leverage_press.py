"""LeverageScorePress (kvpress/presses/leverage_press.py:15-110) on kvp_leverage_score."""
from __future__ import annotations

import math
from dataclasses import dataclass

import torch
from torch import nn

from kvpress_amd import _native
from kvpress_amd.presses.scorer_press import ScorerPress
from kvpress_amd.utils import get_prerope_key_states


@dataclass
class LeverageScorePress(ScorerPress):
    """Approximate leverage scores of the pre-RoPE keys under a right Gaussian sketch (Compactor, Chari & Van Durme 2025,
    https://arxiv.org/abs/2507.08143), z-scored over the whole [B, H_kv, S] tensor.  Prefill only.

    Parameters
    ----------
    compression_ratio : float, default=0.0
    sketch_dimension : int, default=48
        Size of the Gaussian sketch (1 .. 256 in the library).
    """

    compression_ratio: float = 0.0
    sketch_dimension: int = 48

    @staticmethod
    def chol_with_jitter(G: torch.Tensor, jitter: float = 0.0, max_tries: int = 5):
        """Cholesky factorisation with adaptive jitter (leverage_press.py:47-56): a torch helper on a k x k matrix, kept for the
        reference's public signature; the press itself factorises inside kvp_leverage_score (float64, same schedule)."""
        identity = torch.eye(G.shape[-1], device=G.device, dtype=G.dtype)
        cur = float(jitter)
        for _ in range(max_tries):
            L, info = torch.linalg.cholesky_ex(G + cur * identity, upper=False)
            if bool((info == 0).all()):
                return L
            cur = max(1e-8, (1e-2 if cur == 0.0 else 10.0 * cur))
        raise RuntimeError(f"Cholesky failed after {max_tries} tries.")

    @staticmethod
    def draw_sketch(key_states: torch.Tensor, sketch_dimension: int) -> torch.Tensor:
        """Phi [B, H, D, k], drawn exactly as leverage_press.py:68-75 draws it (same call, shape, dtype, device, scale): the random
        stream stays the reference's."""
        d, k = key_states.shape[-1], sketch_dimension
        return torch.randn(key_states.shape[0], key_states.shape[1], d, k, device=key_states.device,
                           dtype=key_states.dtype) * (1 / math.sqrt(k))

    @staticmethod
    def compute_leverage_scores(key_states: torch.Tensor, sketch_dimension: int) -> torch.Tensor:
        """Raw leverage scores [B, H, S] float32 of the pre-RoPE keys (leverage_press.py:59-110 before the z-score)."""
        phi = LeverageScorePress.draw_sketch(key_states, sketch_dimension)
        return _native.leverage_score(key_states, phi, return_raw=True)[1]

    def score(self, module: nn.Module, hidden_states: torch.Tensor, keys: torch.Tensor, values: torch.Tensor,
              attentions: torch.Tensor, kwargs) -> torch.Tensor:
        n_queries = hidden_states.shape[-2]
        assert keys.shape[-2] == n_queries, "LeverageScorePress only supports prefill "
        pre_rope_keys = get_prerope_key_states(module, hidden_states)   # the model's k_proj (a torch call)
        phi = self.draw_sketch(pre_rope_keys, self.sketch_dimension)
        return _native.leverage_score(pre_rope_keys, phi)
