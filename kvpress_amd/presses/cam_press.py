"""CAMPress (kvpress/presses/cam_press.py:24-361): Cache Merging (CaM, https://openreview.net/forum?id=LCTmppB165) while the model decodes.

A DecodingPress whose compression does not simply drop the evicted tokens: the best-scored of them (as many as there were decoding
steps since the last compression) spread their value over the ``merge_budget`` kept tokens that follow them in the cache, each with
probability clamp(A_i / mean(A over that window), 0, 1), A being the attention every cached token has received from the decoded tokens
so far.  Three library calls carry it (include/kvpress_hip.h): kvp_cam_attn_accumulate at every decoding step of every layer,
kvp_cam_merge_plan and kvp_cam_merge_prune at a compression.

Defined deviations: A and the merge probabilities are float32; the merged values are summed in float32 and rounded
once; score ties follow the library's rule (score descending, position ascending) for the kept set AND the candidates; the cache
tensors handed to ``compress`` are never written."""
from __future__ import annotations

from dataclasses import dataclass

import torch
from torch import nn

from kvpress_amd import _native
from kvpress_amd.presses.base_press import is_prefilling
from kvpress_amd.presses.decoding_press import DecodingPress, _kv_len, _write_back
from kvpress_amd.utils import extract_keys_and_values, get_prerope_query_states


@dataclass
class CAMPress(DecodingPress):
    """Parameters
    ----------
    base_press : ScorerPress
        Scores the tokens when a compression is due.
    compression_interval : int, default=512
        Decoding steps between two compressions of a layer (1: the original per-step CaM).
    target_size : int, default=2048
        Tokens a layer keeps after a compression.
    hidden_states_buffer_size : int, default=256
        Hidden states kept per layer between compressions.
    merge_budget : int, default=32
        Kept tokens, in cache order after the evicted one, that share its value.
    """

    merge_budget: int = 32

    def __post_init__(self):
        super().__post_init__()
        assert self.merge_budget > 0, "merge_budget must be positive"

    def reset(self):
        super().reset()
        # layer -> the attention received so far, float32 [B, Hkv, S]: a view of _attn_buffer[layer], whose capacity grows in steps
        self._running_attn_sum: dict[int, torch.Tensor] = {}
        self._attn_buffer: dict[int, torch.Tensor] = {}

    def _running_buffer(self, layer_idx: int, B: int, H: int, S: int, device) -> tuple[torch.Tensor, int]:
        """The layer's buffer with room for S tokens and the number of leading entries that hold its running sum."""
        run = self._running_attn_sum.get(layer_idx)
        buf = self._attn_buffer.get(layer_idx)
        s_prev = 0 if run is None else run.shape[-1]
        assert s_prev <= S, f"the cache of layer {layer_idx} shrank from {s_prev} to {S} tokens outside this press"
        if buf is None or buf.shape[-1] < S or run is None or run.data_ptr() != buf.data_ptr():
            step = max(256, self.compression_interval)
            buf = torch.empty((B, H, -(-S // step) * step), dtype=torch.float32, device=device)
            if s_prev:
                buf[..., :s_prev].copy_(run)      # after a compression: A' moves into a buffer with room for the next interval
            self._attn_buffer[layer_idx] = buf
        return buf, s_prev

    def _draw_merge_mask(self, prob: torch.Tensor) -> torch.Tensor:
        return torch.bernoulli(prob)              # cam_press.py:186

    def compress(self, module: nn.Module, hidden_states: torch.Tensor, keys: torch.Tensor, values: torch.Tensor,
                 attentions: torch.Tensor, kwargs: dict) -> tuple[torch.Tensor, torch.Tensor]:
        """``attentions`` is the layer's running attention sum [B, Hkv, S] (cam_press.py:124-215)."""
        layer_idx = int(module.layer_idx)
        S, T = keys.shape[2], self.target_size
        if S <= T:
            return keys, values
        saved = self.base_press.compression_ratio
        self.base_press.compression_ratio = self._find_target_compression_ratio(S, T)
        try:
            scores = self.base_press.score(module, hidden_states, keys, values, None, kwargs)
        finally:
            self.base_press.compression_ratio = saved
        scores = _native.scores_head_mean_(scores if scores.dtype == torch.float32 else scores.float())[:, :1]   # :142
        M = min(int(self.layer_step_counts[layer_idx]), S - T)                                                  # :149-150
        # ranks [0, T) of the library's total order are kept, ranks [T, T + M) are merged; both selects come back in ascending position
        kept = _native.topk_select(scores, T, _native.ORDER_POSITION)[:, 0]
        sel = _native.topk_select(scores, T + M, _native.ORDER_POSITION)[:, 0] if M else kept
        running = attentions.to(torch.float32)
        cand, start, prob = _native.cam_merge_plan(kept, sel, running, S, self.merge_budget, n_cand=M)
        mask = self._draw_merge_mask(prob)
        keys, values, self._running_attn_sum[layer_idx] = _native.cam_merge_prune(keys, values, running, kept, cand, start, mask,
                                                                                   self.merge_budget)
        return keys, values

    def forward_hook(self, module: nn.Module, input: list[torch.Tensor], kwargs: dict, output: list):
        hidden_states = kwargs["hidden_states"]
        cache = kwargs["past_key_values"]
        q_len = hidden_states.shape[1]
        layer_idx = int(module.layer_idx)
        cache_layer = cache.layers[layer_idx]
        if is_prefilling(_kv_len(cache, layer_idx), q_len, kwargs, cache_layer):
            # a (possibly new) sequence starts: nothing of an earlier one may be added to (cam_press.py:242-249)
            self._running_attn_sum.pop(layer_idx, None)
            self._attn_buffer.pop(layer_idx, None)
            self.hidden_states_buffer[layer_idx] = []
            self.layer_step_counts[layer_idx] = 0
            return output

        self.hidden_states_buffer[layer_idx].append(hidden_states.detach().clone())
        keys, values = extract_keys_and_values(cache, layer_idx)
        B, H, S, _ = keys.shape
        running, s_prev = self._running_buffer(layer_idx, B, H, S, keys.device)
        attentions = output[1] if isinstance(output, (tuple, list)) and len(output) > 1 and output[1] is not None else None
        if attentions is not None:
            _native.cam_attn_accumulate_row_(attentions[:, :, -1, :], running, s_prev)                 # :259-263
        else:
            q_pre = get_prerope_query_states(module, hidden_states[:, -1:])                            # :338-344
            cos, sin = kwargs["position_embeddings"]
            _native.cam_attn_accumulate_(q_pre, cos[:, -1:], sin[:, -1:], keys, running, s_prev)
        self._running_attn_sum[layer_idx] = running[..., :S]
        self.layer_step_counts[layer_idx] += 1

        if (self.layer_step_counts[layer_idx] >= self.compression_interval and S > self.target_size) or q_len >= self.target_size:
            buffered = torch.cat(self.hidden_states_buffer[layer_idx], dim=1)
            keys, values = self.compress(module, buffered, keys, values, self._running_attn_sum[layer_idx], kwargs)
            _write_back(cache, cache_layer, keys, values)
            self.layer_step_counts[layer_idx] = 0
            self.hidden_states_buffer[layer_idx] = []      # buffer and cache must describe the same tokens

        n = self.hidden_states_buffer_size
        self.hidden_states_buffer[layer_idx] = self.hidden_states_buffer[layer_idx][-n:] if n > 0 else []
        return output
