"""KVzipPress (kvpress/presses/kvzip_press.py:22-394): query-agnostic compression by context reconstruction
(https://arxiv.org/abs/2505.23416).  After the ordinary prefill the model is asked, chunk by chunk, to repeat the context; the
importance of a cached KV pair is the largest attention any repeated token of any query head of its group pays to it.

On the library: per layer and chunk one ``kvp_kvzip_score`` call (the reference's key concatenation, the stored softmax of
``[Hkv, G, q_len, sink + chunk + q_len]``, its causal mask, slice and amax, :312-354, without any tensor of that extent), written
straight into the chunk's columns of the score table; ``compress_post`` selects each layer's cross-head bottom-k with
``kvp_topk_select(KVP_TOPK_SMALLEST)`` as AdaKVPress does.  K and V stay in the cache and the pruned triples go to
``module.masked_key_indices`` (kvpress_amd.attention_patch).  ``q_proj`` and the KVzip+ scales (``1 / ||h_t||`` per row and
``||V_j Wo_{h,g}||_2`` per chunk column) stay torch calls in the hook.

Defined deviation: ``score_val`` is float32 whatever the model's dtype; the reference keeps the model dtype
(:245), where thousands of scores tie."""
from __future__ import annotations

import logging
from contextlib import contextmanager
from dataclasses import dataclass
from types import MethodType
from typing import Generator, List

import torch
from torch import nn

from kvpress_amd import _native
from kvpress_amd.attention_patch import patch_attention_functions
from kvpress_amd.presses.base_press import SUPPORTED_MODEL_NAMES, BasePress
from kvpress_amd.utils import _is_quantized, extract_keys_and_values, get_prerope_query_states

logger = logging.getLogger(__name__)


def mask_lowest_scores(model, score_val: torch.Tensor, compression_ratio: float, layerwise: bool) -> None:
    """``compress_post`` of KVzipPress (:360-394) and of FastKVzipPress (fastkvzip_press.py:251-287), which share it line for line: from
    the score table [L, B, Hkv, S] the cross-layer budget, then each layer's bottom-k across heads into ``module.masked_key_indices``."""
    if compression_ratio > 0:
        n_layer, bsz, num_key_value_heads, ctx_len = score_val.shape

        if layerwise:
            n_pruned_layers = [int(bsz * num_key_value_heads * ctx_len * compression_ratio)] * n_layer
        else:   # once per context: a torch expression
            n_pruned_indices = int(score_val.numel() * compression_ratio)
            pruned_indices = torch.topk(-score_val.reshape(-1), n_pruned_indices).indices
            n_tokens_per_layer = bsz * num_key_value_heads * ctx_len
            n_pruned_layers = torch.bincount(pruned_indices // n_tokens_per_layer, minlength=n_layer).tolist()

        for layer in model.model.layers:
            module = layer.self_attn
            layer_idx = int(module.layer_idx)
            assert module.config._attn_implementation != "eager", "eager mode not supported"

            scores = score_val[layer_idx]
            n_pruned = int(n_pruned_layers[layer_idx])
            flat = _native.topk_select(scores.view(bsz, num_key_value_heads * ctx_len), n_pruned,
                                       _native.ORDER_POSITION | _native.TOPK_SMALLEST)
            flat = flat.to(torch.int64).flatten()
            batch_indices = torch.arange(bsz, device=flat.device).repeat_interleave(n_pruned)
            module.masked_key_indices = (batch_indices, flat // ctx_len, flat % ctx_len)


@dataclass
class KVzipPress(BasePress):
    """KVzip (https://arxiv.org/abs/2505.23416).

    Parameters
    ----------
    compression_ratio : float, default=0.0
        Fraction of key-value pairs to remove during compression.
    layerwise : bool, default=False
        Uniform compression ratio across layers; when False the overall ratio is kept and every layer gets its own.
    n_sink : int, default=4
        Number of initial tokens to preserve as attention sinks.
    kvzip_plus_normalization : bool, default=False
        KVzip+ normalisation of the attention (rows by 1 / ||h||, columns by ||Wo V||).

    ``tokenizer`` (a plain class attribute, not a field): when set it is used instead of
    ``AutoTokenizer.from_pretrained(model.config.name_or_path)``.
    """

    compression_ratio: float = 0.0
    layerwise: bool = False
    n_sink: int = 4
    kvzip_plus_normalization: bool = False

    tokenizer = None

    def __post_init__(self):
        assert 0 <= self.compression_ratio < 1, "Compression ratio must be between 0 and 1"
        logger.warning(
            "KVzipPress requires multiple forward passes for chunked context reconstruction, "
            "resulting in a computational overhead of 2–3 times the initial prefilling cost. "
            "This significantly increases the overall prefilling time compared to other compression methods, "
            "which is inherent to the KVzip algorithm design."
        )
        patch_attention_functions()
        self._reset_internal_parameters()

    def _reset_internal_parameters(self):
        self.context_length = 0
        self.prefix_length = 0

        self._suffix_ids = None
        self._context_ids = None
        self._cache = None

        self.score_val = None
        self.start_idx = 0
        self.end_idx = 0

    @contextmanager
    def __call__(self, model) -> Generator:
        """The initial prefill runs inside the ``with``; on the way out the context is reconstructed chunk by chunk under the press's
        own hook, scored and compressed (:78-147)."""
        if type(model).__name__ not in SUPPORTED_MODEL_NAMES:
            logger.warning(f"Model {type(model)} not tested, supported models: {SUPPORTED_MODEL_NAMES}")
        if any(c.__name__ == "Gemma3PreTrainedModel" for c in type(model).__mro__):
            raise ValueError("KVzipPress is not supported for Gemma3ForCausalLM")

        self.post_init_from_model(model)

        tokenizer = self.tokenizer
        if tokenizer is None:
            from transformers import AutoTokenizer

            tokenizer = AutoTokenizer.from_pretrained(model.config.name_or_path)

        # the part of the chat template that follows the user's text (:99-113)
        if tokenizer.chat_template is None:
            prefix_text = ""
            suffix_text = "\n"
        else:
            dummy_context = "dummy context"
            separator = "\n" + "#" * len(dummy_context)
            temp_context = tokenizer.apply_chat_template([{"role": "user", "content": dummy_context + separator}],
                                                         add_generation_prompt=True, tokenize=False, enable_thinking=False)
            context, suffix_text = temp_context.split(separator)
            prefix_text = context.split(dummy_context)[0]
        self.prefix_length = self._encode(tokenizer, prefix_text).shape[-1]
        self._suffix_ids = self._encode(tokenizer, suffix_text)

        # catch the context ids and the cache of the prefill (:120-127)
        original_forward = model.model.forward

        def wrapped_forward(model_self, *args, **kwargs):
            assert kwargs["input_ids"].shape[0] == 1, "KVzipPress only supports a batch size of 1"
            self._context_ids = kwargs["input_ids"]
            self._cache = kwargs["past_key_values"]
            return original_forward(*args, **kwargs)

        model.model.forward = MethodType(wrapped_forward, model.model)

        hooks = []
        try:
            try:
                yield
            finally:
                model.model.forward = original_forward

            if self.compression_ratio > 0 and self._context_ids is not None:
                for layer in model.model.layers:
                    layer.self_attn.rotary_emb = model.model.rotary_emb
                    hooks.append(layer.self_attn.register_forward_hook(self.forward_hook, with_kwargs=True))
                self._perform_kvzip_compression(model, tokenizer)
        finally:
            for hook in hooks:
                hook.remove()
            self._reset_internal_parameters()
        _native.async_error_check()   # as BasePress.__call__: reached only when nothing raised

    @staticmethod
    def _encode(tokenizer, text: str) -> torch.Tensor:
        """int64 [1, n] (an empty text gives [1, 0], whatever dtype the tokenizer returns for it)"""
        return tokenizer.encode(text, return_tensors="pt", add_special_tokens=False).reshape(1, -1).to(torch.long)

    def forward_hook(self, module: nn.Module, input: list[torch.Tensor], kwargs: dict, output: list):
        """During the reconstruction forwards: score the current chunk, then cut the layer back to the prefilled context (:149-177)."""
        hidden_states = kwargs["hidden_states"]
        cache = kwargs.get("past_key_values", None) or kwargs.get("past_key_value", None)
        cache_layer = cache.layers[module.layer_idx]

        keys, values = extract_keys_and_values(cache, module.layer_idx)
        keys, values = self.score_kvzip(module, hidden_states, keys, values, output[1] if len(output) > 1 else None, kwargs)

        if _is_quantized(cache):
            cache_layer._quantized_keys = cache_layer._quantize(keys, axis=cache_layer.axis_key)
            cache_layer._quantized_values = cache_layer._quantize(values, axis=cache_layer.axis_value)
            cache_layer.keys = torch.zeros(0, dtype=keys.dtype, device=keys.device)
            cache_layer.values = torch.zeros(0, dtype=keys.dtype, device=keys.device)
            cache_layer.cumulative_length = keys.shape[2]
        else:
            cache_layer.keys = keys
            cache_layer.values = values
        return output

    def _perform_kvzip_compression(self, model, tokenizer):
        """One model forward per (chunk, repeat prompt) pair on top of the prefilled cache, then the selection (:179-202)."""
        self.context_length = self._context_ids.shape[1]
        chunked_context_pairs = self.prepare(model, tokenizer)

        self.start_idx = self.prefix_length
        for prefill_ids, repeat_ids in chunked_context_pairs:
            self.end_idx = self.start_idx + prefill_ids.shape[1]
            model(input_ids=repeat_ids.to(model.device), past_key_values=self._cache, logits_to_keep=1)
            self.start_idx = self.end_idx

        self.compress_post(model)

    def _chunk_fn(self, ctx_ids: torch.Tensor, chunk_size: int) -> List[torch.Tensor]:
        """Chunk input tokens (:204-223)"""
        ctx_len = ctx_ids.shape[1]
        if ctx_len <= chunk_size:
            return [ctx_ids]
        chunks = [ctx_ids[:, i * chunk_size:(i + 1) * chunk_size] for i in range((ctx_len - 1) // chunk_size + 1)]
        return [c for c in chunks if c.shape[1] > 0]

    def prepare(self, model, tokenizer, chunk_size: int = 2048, prev_postfix_size=8) -> List[tuple[torch.Tensor, torch.Tensor]]:
        """The score table and the (chunk ids, repeat-prompt ids) pairs (:225-264)."""
        ctx_ids = self._context_ids[:, self.prefix_length:].to("cpu")

        # float32 whatever the model's dtype; batch size 1 only
        self.score_val = torch.zeros((model.config.num_hidden_layers, 1, model.config.num_key_value_heads, self.context_length),
                                     dtype=torch.float32, device=model.device)
        self.score_val[..., : self.n_sink] = 1.0

        chunked_context_pairs = []
        chunked_input_ids = self._chunk_fn(ctx_ids, chunk_size)
        for i, a_ids in enumerate(chunked_input_ids):
            if i == 0:
                q_ids = self._encode(tokenizer, "\n\nRepeat the previous context exactly.")
            else:
                q_ids = self._encode(tokenizer, "\n\nRepeat the part of the previous context exactly, starting with")
                q_ids = torch.cat([q_ids, chunked_input_ids[i - 1][:, -prev_postfix_size:]], dim=1)
            chunked_context_pairs.append((a_ids, torch.cat([q_ids, self._suffix_ids, a_ids], dim=1)))
        return chunked_context_pairs

    def score_kvzip(self, module: nn.Module, hidden_states: torch.Tensor, keys: torch.Tensor, values: torch.Tensor,
                    attentions: torch.Tensor, kwargs) -> tuple[torch.Tensor, torch.Tensor]:
        """The chunk's maximum cross-attention scores into ``self.score_val`` (:287-354); returns K and V cut back to the prefilled
        context (:357)."""
        bsz, q_len, _ = hidden_states.shape
        assert bsz == 1, "KVzipPress only supports a batch size of 1"
        queries = get_prerope_query_states(module, hidden_states)
        cos, sin = kwargs["position_embeddings"]

        sink = min(self.n_sink, self.start_idx)
        row_scale = col_scale = None
        if self.kvzip_plus_normalization:
            row_scale, col_scale = self._plus_scales(module, hidden_states, values[:, :, self.start_idx:self.end_idx])
        layer_idx = int(module.layer_idx)
        _native.kvzip_score(queries, cos, sin, keys, sink, self.start_idx, self.end_idx, row_scale, col_scale,
                            out=self.score_val[layer_idx][..., self.start_idx:self.end_idx])
        return keys[:, :, : self.context_length], values[:, :, : self.context_length]

    @staticmethod
    def _plus_scales(module: nn.Module, hidden_states: torch.Tensor, values_chunk: torch.Tensor):
        """KVzip+ (:336-348) for the chunk's columns only, in float32: 1 / ||h_t|| [B, q_len] and ||V_j Wo_{h,g}||_2 [B, Hq, ctx]"""
        num_kv = values_chunk.shape[1]
        groups = module.config.num_attention_heads // num_kv
        row_scale = 1.0 / torch.norm(hidden_states.float(), dim=-1)
        wo = module.o_proj.weight.float().t().reshape(num_kv, groups, module.head_dim, -1)   # [Hkv, G, D, hidden]
        v = values_chunk.float()
        # one group member at a time: the transient is [B, Hkv, ctx, hidden]
        col = torch.stack([torch.einsum("bhtd,hdj->bhtj", v, wo[:, g]).norm(dim=-1) for g in range(groups)], dim=2)
        return row_scale, col.reshape(v.shape[0], num_kv * groups, v.shape[2])

    def compress_post(self, model):
        """The (head, position) pairs every layer masks (:360-394): the cross-layer budget, then each layer's bottom-k across heads."""
        mask_lowest_scores(model, self.score_val, self.compression_ratio, self.layerwise)
