"""MergingPress (kvpress/presses/merging_press.py:17-177): any ScorerPress's select + gather, with every evicted token's value folded into
its most cosine-similar survivor by kvp_merge_values (include/kvpress_hip.h) instead of being dropped."""
from __future__ import annotations

from dataclasses import dataclass

import torch
from torch import nn

from kvpress_amd import _native
from kvpress_amd.presses.base_press import BasePress
from kvpress_amd.presses.scorer_press import ScorerPress


@dataclass
class MergingPress(BasePress):
    """Merge-on-evict wrapper for any :class:`ScorerPress` (Token Merging, Bolya et al. 2023; D2O, Wan et al. 2024).

    Each evicted token's value is blended into the value of the kept token whose key is most cosine-similar, weighted by the
    similarity and the relative value norms; keys are kept unchanged.  The survivors are stored in the inner press's ``kept_order``.

    Parameters
    ----------
    press : ScorerPress
        Underlying scorer that decides which tokens survive.
    similarity_threshold : float, default=0.0
        Minimum cosine similarity for a merge to proceed.
    merge_fraction : float, default=1.0
        Fraction of evicted tokens (ranked by similarity) that are merged.
    """

    press: ScorerPress = None  # type: ignore[assignment]
    similarity_threshold: float = 0.0
    merge_fraction: float = 1.0

    def __post_init__(self):
        assert isinstance(self.press, ScorerPress), (
            f"MergingPress requires a ScorerPress, got {type(self.press).__name__}"
        )
        assert 0.0 <= self.similarity_threshold <= 1.0
        assert 0.0 < self.merge_fraction <= 1.0, "merge_fraction must be in (0, 1]"

    def post_init_from_model(self, model):
        self.press.post_init_from_model(model)

    @property
    def compression_ratio(self) -> float:
        return self.press.compression_ratio

    @compression_ratio.setter
    def compression_ratio(self, value: float) -> None:
        self.press.compression_ratio = value

    def compress(self, module: nn.Module, hidden_states: torch.Tensor, keys: torch.Tensor, values: torch.Tensor,
                 attentions: torch.Tensor, kwargs: dict) -> tuple[torch.Tensor, torch.Tensor]:
        """merging_press.py:64-97: score, select ``int(k_len * (1 - ratio))`` (the reference's own count, not the inner press's
        n_kept()), gather, then merge the evicted values into V' in place."""
        if self.press.compression_ratio == 0:
            return keys, values

        scores = self.press.score(module, hidden_states, keys, values, attentions, kwargs)
        k_len = keys.shape[2]
        n_kept = int(k_len * (1 - self.press.compression_ratio))
        indices = _native.topk_select(scores, n_kept, self.press.library_order())   # int32 [B, H, n_kept]
        k_out, v_out = _native.gather_kv(keys, values, indices)               # new contiguous tensors: the inputs stay untouched
        if 0 < n_kept < k_len:                                                # merging_press.py:120-121
            _native.merge_values_(keys, values, indices, k_out, v_out, self.similarity_threshold, self.merge_fraction)
        return k_out, v_out
