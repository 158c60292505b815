"""CompactorPress (kvpress/presses/compactor_press.py:16-122): LeverageScorePress + NonCausalAttnPress blended by kvp_compactor_combine."""
from __future__ import annotations

from dataclasses import dataclass
from typing import Optional

import torch
from torch import nn

from kvpress_amd import _native
from kvpress_amd.presses.leverage_press import LeverageScorePress
from kvpress_amd.presses.non_causal_attention_press import NonCausalAttnPress
from kvpress_amd.presses.scorer_press import ScorerPress


@dataclass
class CompactorPress(ScorerPress):
    """Compactor (Chari & Van Durme 2025, https://arxiv.org/abs/2507.08143): ``blending`` x the leverage z-scores of the pre-RoPE keys
    plus the non-causal chunked attention z-scores; the first ``sink_size_start`` and last ``sink_size_end`` tokens are always kept
    (padded with the maximum score).  Prefill only.

    Parameters
    ----------
    compression_ratio : float, default=0.0
    sink_size_start : int, default=8
    sink_size_end : int, default=4
    chunk_size : int, default=256
        Chunk size of the non-causal attention.
    sketch_dimension : int, default=48
        Size of the Gaussian sketch.
    blending : Optional[float], default=None
        Weight of the leverage scores; ``None`` means ``compression_ratio`` (0.35 if that is ``None``).
    """

    compression_ratio: float = 0.0
    sink_size_start: int = 8
    sink_size_end: int = 4
    chunk_size: int = 256
    sketch_dimension: int = 48
    blending: Optional[float] = None

    _leverage_press: Optional[LeverageScorePress] = None
    _non_causal_press: Optional[NonCausalAttnPress] = None

    def __post_init__(self):
        super().__post_init__()
        self._leverage_press = LeverageScorePress(compression_ratio=self.compression_ratio, sketch_dimension=self.sketch_dimension)
        self._non_causal_press = NonCausalAttnPress(compression_ratio=self.compression_ratio, chunk_size=self.chunk_size)

    def __setattr__(self, name, value):
        # compactor_press.py:76-87: the inner presses follow the wrapper's settings
        object.__setattr__(self, name, value)
        if name == "compression_ratio":
            if "_leverage_press" in self.__dict__:
                self._leverage_press.compression_ratio = value
            if "_non_causal_press" in self.__dict__:
                self._non_causal_press.compression_ratio = value
        if name == "sketch_dimension":
            if "_leverage_press" in self.__dict__:
                self._leverage_press.sketch_dimension = value
        if name == "chunk_size":
            if "_non_causal_press" in self.__dict__:
                self._non_causal_press.chunk_size = value

    def score(self, module: nn.Module, hidden_states: torch.Tensor, keys: torch.Tensor, values: torch.Tensor,
              attentions: torch.Tensor, kwargs) -> torch.Tensor:
        n_queries = hidden_states.shape[-2]
        assert keys.shape[-2] == n_queries, "CompactorPress only supports prefill at the moment"
        left_keep = min(self.sink_size_start, n_queries)
        right_keep = min(self.sink_size_end, max(0, n_queries - left_keep))
        start_idx, end_idx = left_keep, (None if right_keep == 0 else -right_keep)

        hs = hidden_states[:, start_idx:end_idx]
        keys = keys[..., start_idx:end_idx, :]
        values = values[..., start_idx:end_idx, :]
        cos, sin = kwargs["position_embeddings"]
        sliced_kwargs = {"position_embeddings": (cos[..., start_idx:end_idx, :], sin[..., start_idx:end_idx, :])}

        l_scores = self._leverage_press.score(module, hs, keys, values, attentions, sliced_kwargs)
        attn_scores = self._non_causal_press.score(module, hs, keys, values, attentions, sliced_kwargs)
        assert attn_scores.shape == l_scores.shape, "CompactorPress only supports prefill at the moment"
        blending = self.blending if self.blending is not None else self.compression_ratio
        blending = 0.35 if blending is None else blending
        return _native.compactor_combine(l_scores, attn_scores, left_keep, right_keep, blending)
