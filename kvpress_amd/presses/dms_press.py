"""DMSPress (kvpress/presses/dms_press.py:15-130): wraps a ScorerPress and evicts every KV pair whose score falls below a threshold once
the pair has left a sliding window of recent tokens -- the dense-prefill inference scheme of Dynamic Memory Sparsification
(https://arxiv.org/abs/2506.05345) without its trained evictors.  The compression ratio is a result, not a setting, and the press
works during prefill and, with ``decoding=True``, for every generated token.

On the library: the wrapped press's ``score`` on the last ``q_len`` keys (``kvp_kvzap_score`` for KVzapPress), the scores of the window
kept as a float32 torch tensor, and ``kvp_threshold_count`` / ``kvp_threshold_select`` for what left the window (the reference's
``torch.where(scores < threshold)`` and its shift, :106-112).  K and V stay in the cache; the evicted (batch, head, position)
triples are appended to ``module.masked_key_indices`` and masked while decoding by kvpress_amd.attention_patch.

Host-side difference: prefill is told from decoding by this package's ``is_prefilling`` (tensor shapes; transformers 5.x passes no
``cache_position``) and the number of processed tokens is the layer's cache length (DMSPress never shortens the cache)."""
from __future__ import annotations

from dataclasses import dataclass, field
from typing import Optional

import torch
import torch.nn as nn

from kvpress_amd import _native
from kvpress_amd.attention_patch import patch_attention_functions
from kvpress_amd.presses.base_press import BasePress, is_prefilling
from kvpress_amd.presses.scorer_press import ScorerPress
from kvpress_amd.utils import _is_quantized, extract_keys_and_values


@dataclass
class DMSPress(BasePress):
    """Threshold eviction behind a sliding window.

    Parameters
    ----------
    press : ScorerPress
        Scores the new tokens of every forward.
    threshold : float, optional
        Tokens with a score below it are evicted.
    sliding_window_size : int, default=128
        Number of recent tokens protected from eviction.
    decoding : bool, default=False
        Also compress while decoding.
    """

    press: ScorerPress
    threshold: Optional[float] = None
    sliding_window_size: int = 128
    decoding: bool = False
    scores_buffer: dict[int, torch.Tensor] = field(default_factory=dict, init=False, repr=False)
    compression_ratios: dict[int, float] = field(default_factory=dict, init=False, repr=False)

    def __post_init__(self):
        patch_attention_functions()

    def post_init_from_model(self, model):
        self.press.post_init_from_model(model)

    @property
    def compression_ratio(self):
        """the mean over the layers of the fraction of masked (batch, head, position) entries; known once a forward has run"""
        assert len(self.compression_ratios) > 0, "Forward pass must be run to compute the compression ratio"
        return sum(self.compression_ratios.values()) / len(self.compression_ratios)

    @compression_ratio.setter
    def compression_ratio(self, value):
        """a result of the threshold and the input, not a setting"""
        raise AttributeError(f"compression ratio cannot be set for {type(self).__name__}")

    def forward_hook(self, module: nn.Module, input: list[torch.Tensor], kwargs: dict, output: list):
        hidden_states = kwargs["hidden_states"]
        cache = kwargs["past_key_values"]
        q_len = hidden_states.shape[1]
        layer_idx = int(module.layer_idx)
        cache_layer = cache.layers[layer_idx]
        kv_len = cache.get_seq_length(layer_idx) if _is_quantized(cache) else cache_layer.keys.shape[2]
        prefilling = is_prefilling(kv_len, q_len, kwargs, cache_layer)

        # a new context: forget the last one's window and ratios (dms_press.py:80-82)
        if prefilling and layer_idx == 0:
            self.scores_buffer.clear()
            self.compression_ratios.clear()
        if not prefilling and not self.decoding:
            return output

        keys, values = extract_keys_and_values(cache, layer_idx)
        cache_len = keys.shape[2]   # every processed token is still in the cache: the reference's cache_position[-1] + 1 (:73)
        scores = self.press.score(module, hidden_states, keys[:, :, -q_len:], values[:, :, -q_len:], None, kwargs)
        if scores.dtype != torch.float32:
            scores = scores.to(torch.float32)

        if prefilling:
            buffer = scores
        else:
            buffer = torch.cat([self.scores_buffer[layer_idx], scores], dim=-1)

        # what left the window is decided now (:99-120)
        n_to_evict = buffer.shape[-1] - self.sliding_window_size
        if n_to_evict > 0:
            shift = cache_len - n_to_evict - self.sliding_window_size
            new_masked = _native.threshold_select(buffer[..., :n_to_evict], self.threshold, shift)
            buffer = buffer[..., n_to_evict:]
            if len(new_masked[0]) > 0:
                masked = getattr(module, "masked_key_indices", None)
                if masked is None:
                    module.masked_key_indices = new_masked
                else:
                    module.masked_key_indices = [torch.cat([i, new_i]) for i, new_i in zip(masked, new_masked)]
        self.scores_buffer[layer_idx] = buffer

        masked = getattr(module, "masked_key_indices", None)
        if masked is not None:
            bsz, num_key_value_heads = keys.shape[:2]
            self.compression_ratios[layer_idx] = len(masked[0]) / (bsz * num_key_value_heads * cache_len)
        else:
            self.compression_ratios[layer_idx] = 0
        return output
