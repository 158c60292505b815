"""CriticalKVPress / CriticalAdaKVPress (kvpress/presses/criticalkv_press.py:17-194): two-stage selection with the scores of any
ScorerPress rescaled by the L1 norm of every value row pushed through the output projection (https://arxiv.org/abs/2502.03805).

On the library: the wrapped press's ``score`` -> ``kvp_topk_select`` (stage 1) -> ``kvp_vwl1norm_rescale`` (the reference's
``vwl1norm`` :57-76 and ``(scores + epsilon) * norm`` :87 in one kernel: nothing of size [S, hidden] is stored) -> the protection of
the stage-1 survivors with float32 max (``kvp_scores_fill_at`` / ``kvp_scores_fill_prefix``).  CriticalAdaKVPress adds AdaKV's
head-wise budgets; K and V stay in the cache and the pruned triples go to ``module.masked_key_indices`` (kvpress_amd.attention_patch).

Defined deviation: CriticalAdaKVPress computes the head budgets per batch element, so every element is treated
as the reference treats it alone; the reference adds the budgets of all batch elements into one vector (:163-164) and fails for B > 1."""
from __future__ import annotations

import logging
from dataclasses import dataclass

import torch
from torch import nn

from kvpress_amd import _native
from kvpress_amd.attention_patch import patch_attention_functions
from kvpress_amd.presses.base_press import BasePress
from kvpress_amd.presses.expected_attention_press import ExpectedAttentionPress
from kvpress_amd.presses.scorer_press import ScorerPress

logger = logging.getLogger(__name__)
_FMAX = torch.finfo(torch.float32).max


def _float32_scores(press, module, hidden_states, keys, values, attentions, kwargs) -> torch.Tensor:
    """the wrapped press's scores as a float32 tensor this press may write to"""
    scores = press.score(module, hidden_states, keys, values, attentions, kwargs)
    scores = scores.to(torch.float32).contiguous()
    if scores.data_ptr() in (keys.data_ptr(), values.data_ptr()):
        scores = scores.clone()
    return scores


def _rescale_(scores: torch.Tensor, values: torch.Tensor, module: nn.Module, epsilon: float) -> torch.Tensor:
    """scores <- (scores + epsilon) * vwl1norm(values, module) (:86-87, :174-175); an o_proj bias is ignored, as in the reference"""
    return _native.vwl1norm_rescale_(scores, values, module.o_proj.weight, module.config.num_attention_heads, epsilon)


class CriticalKVPress(ScorerPress):
    """CriticalKV (https://arxiv.org/abs/2502.03805): two-stage compression with output projection weighting.

    Parameters
    ----------
    press : ScorerPress
        Base scoring method to enhance with output projection weighting.
    epsilon : float, default=1e-4
        Small value for numerical stability in score rescaling.
    first_stage_ratio : float, default=0.5
        Fraction of the budget selected in the first stage (on the wrapped press's scores alone).
    """

    def __init__(self, press: ScorerPress, epsilon: float = 1e-4, first_stage_ratio: float = 0.5):
        self.press = press
        self.epsilon = epsilon
        self.first_stage_ratio = first_stage_ratio

        assert isinstance(self.press, ScorerPress), "CriticalKVPress requires a ScorerPress as input"
        if isinstance(self.press, ExpectedAttentionPress) and self.press.use_vnorm:
            logger.warning("use_vnorm should be disabled for CriticalKVPress")

    def post_init_from_model(self, model):
        self.press.post_init_from_model(model)

    @property
    def compression_ratio(self):
        return self.press.compression_ratio

    @compression_ratio.setter
    def compression_ratio(self, value):
        self.press.compression_ratio = value

    @staticmethod
    def vwl1norm(values: torch.Tensor, module: nn.Module) -> torch.Tensor:
        """float32 [B, num_kv_heads, k_len] (:57-76)"""
        return _native.vwl1norm(values, module.o_proj.weight, module.config.num_attention_heads)

    def score(self, module: nn.Module, hidden_states: torch.Tensor, keys: torch.Tensor, values: torch.Tensor,
              attentions: torch.Tensor, kwargs) -> torch.Tensor:
        scores = _float32_scores(self.press, module, hidden_states, keys, values, attentions, kwargs)
        k_len = keys.shape[2]
        selection_budget = int((1 - self.compression_ratio) * k_len * self.first_stage_ratio)   # :82
        top_k_index = _native.topk_select(scores, selection_budget)                              # :83
        _rescale_(scores, values, module, self.epsilon)                                          # :86-87
        return _native.scores_fill_at_(scores, top_k_index, _FMAX)                               # :90


@dataclass
class CriticalAdaKVPress(BasePress):
    """CriticalAdaKV (https://arxiv.org/abs/2502.03805): CriticalKV's two stages with AdaKV's head-wise budgets.

    Parameters
    ----------
    press : ScorerPress
        The underlying scoring method used to evaluate token importance.
    alpha_safeguard : float, default=0.20
        Minimum fraction of KV pairs that each head must retain (see AdaKVPress).
    epsilon : float, default=1e-4
        Small value for numerical stability in score rescaling.
    first_stage_ratio : float, default=0.5
        Fraction of every head's budget selected in the first stage.
    """

    press: ScorerPress = None
    alpha_safeguard: float = 0.20
    epsilon: float = 1e-4
    first_stage_ratio: float = 0.5

    def __post_init__(self):
        assert 0 <= self.alpha_safeguard <= 1, "alpha_safeguard should be in 0, 1]"
        assert isinstance(self.press, ScorerPress), "CriticalAdaKVPress requires a ScorerPress as input"
        if isinstance(self.press, ExpectedAttentionPress) and self.press.use_vnorm:
            logger.warning("use_vnorm should be disabled for CriticalAdaKVPress")
        patch_attention_functions()

    def post_init_from_model(self, model):
        self.press.post_init_from_model(model)

    @property
    def compression_ratio(self):
        return self.press.compression_ratio

    @compression_ratio.setter
    def compression_ratio(self, value):
        self.press.compression_ratio = value

    def head_budgets(self, scores: torch.Tensor, n_kept: int) -> torch.Tensor:
        """int64 [B, H]: per batch element, how many of the ``n_kept * H`` largest scores of the flattened row lie in each head (:159-164)"""
        bsz, num_kv, k_len = scores.shape
        top = _native.topk_select(scores.view(bsz, num_kv * k_len), n_kept * num_kv).to(torch.int64)
        budgets = torch.zeros((bsz, num_kv), dtype=torch.int64, device=scores.device)
        return budgets.scatter_add_(1, top // k_len, torch.ones_like(top))

    def compress(self, module: nn.Module, hidden_states: torch.Tensor, keys: torch.Tensor, values: torch.Tensor,
                 attentions: torch.Tensor, kwargs: dict) -> tuple[torch.Tensor, torch.Tensor]:
        if self.compression_ratio == 0:
            return keys, values
        assert module.config._attn_implementation != "eager", "eager mode not supported"

        scores = _float32_scores(self.press, module, hidden_states, keys, values, attentions, kwargs)
        bsz, num_kv, k_len = scores.shape

        n_kept = int(k_len * (1 - self.compression_ratio))          # ScorerPress definition
        n_safe = int(n_kept * self.alpha_safeguard)                 # :150
        if n_safe:
            _native.scores_fill_at_(scores, _native.topk_select(scores, n_safe), _FMAX)

        budgets = self.head_budgets(scores, n_kept)
        # :167 in torch's float32 arithmetic (int64 tensor * Python float), as the reference evaluates it
        budgets_1st = (budgets * self.first_stage_ratio).to(torch.int64)
        # the one device -> host read of the layer: the selects need the largest budget of each stage (the reference's .tolist(), :167)
        k_1st, k_2nd = torch.stack((budgets_1st.max(), budgets.max())).tolist()

        # stage 1 (:168-171): every head protects its own prefix of the score-ordered selection
        top = _native.topk_select(scores, k_1st, _native.ORDER_SCORE)
        _native.scores_fill_prefix_(scores, top, budgets_1st, _FMAX)
        # stage 2 (:174-179)
        _rescale_(scores, values, module, self.epsilon)
        top = _native.topk_select(scores, k_2nd, _native.ORDER_SCORE)
        _native.scores_fill_prefix_(scores, top, budgets, _FMAX)

        n_pruned = num_kv * (k_len - n_kept)                        # :186
        flat = _native.topk_select(scores.view(bsz, num_kv * k_len), n_pruned, _native.ORDER_POSITION | _native.TOPK_SMALLEST)
        flat = flat.to(torch.int64).flatten()
        batch_indices = torch.arange(bsz, device=flat.device).repeat_interleave(n_pruned)
        module.masked_key_indices = (batch_indices, flat // k_len, flat % k_len)
        return keys, values
