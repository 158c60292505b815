"""NonCausalAttnPress (kvpress/presses/non_causal_attention_press.py:16-122) on kvp_ncattn_score."""
from __future__ import annotations

from dataclasses import dataclass

import torch
from torch import nn

from kvpress_amd import _native
from kvpress_amd.presses.scorer_press import ScorerPress
from kvpress_amd.utils import get_prerope_query_states


@dataclass
class NonCausalAttnPress(ScorerPress):
    """Non-causal, chunked attention scorer of Compactor (Chari & Van Durme 2025, https://arxiv.org/abs/2507.08143): every query of a
    chunk of ``chunk_size`` tokens attends to every key of the chunk; a key's score is the attention it receives, averaged over the
    query-head group, times ||v||, smoothed with avg_pool1d(3) and z-scored over the whole [B, H_kv, S] tensor.  Prefill only.

    Parameters
    ----------
    compression_ratio : float, default=0.0
    chunk_size : int, default=256
        Chunk size of the non-causal attention.
    """

    compression_ratio: float = 0.0
    chunk_size: int = 256

    def score(self, module: nn.Module, hidden_states: torch.Tensor, keys: torch.Tensor, values: torch.Tensor,
              attentions: torch.Tensor, kwargs) -> torch.Tensor:
        n_queries = hidden_states.shape[-2]
        assert keys.shape[-2] == n_queries, "NonCausalAttnPress only supports prefill"
        assert self.chunk_size > 0, "chunk_size must be positive"
        cos, sin = kwargs["position_embeddings"]
        # q_proj is the model's own nn.Linear (a torch call); RoPE, the chunked attention, ||v||, pooling and the z-score: the library
        q = get_prerope_query_states(module, hidden_states)   # (B, Hq, S, D)
        q_len = q.shape[-2]
        return _native.ncattn_score(q, cos[:, -q_len:], sin[:, -q_len:], keys, values, self.chunk_size)
