"""KVzapPress (kvpress/presses/kvzap_press.py:14-82): a per-layer surrogate -- linear, or a two-layer MLP with an erf GELU -- predicts
KVzip's score of every KV pair from the hidden states the attention layer receives (https://arxiv.org/abs/2601.07891).  It works during
prefill and during decoding and is meant to be used through DMSPress (kvpress_amd.presses.dms_press).

On the library: one ``kvp_kvzap_score`` call per layer and forward -- both linear layers, the GELU and the transpose of :79-81, with
nothing of extent ``S x hidden_dim`` stored.  The surrogate's weights are packed once per layer, device and dtype (the reference's
``kvzap_module.to(device, dtype)`` of :80).

``KVzapConfig`` / ``KVzapModel`` keep the reference's names, config fields and ``layers`` structure, so the published checkpoints
``nvidia/KVzap-{linear,mlp}-<model>`` load with ``from_pretrained``.  ``kvzap_model`` is a plain class attribute: a model assigned to it
(tests, offline use) is kept, and the hub is asked only when there is none or the served model's name changed.

Defined deviation: the scores are float32 whatever the model's dtype; the reference returns the model dtype."""
from __future__ import annotations

from dataclasses import dataclass, field
from typing import Literal, Optional

import torch
import torch.nn as nn
from transformers import PretrainedConfig, PreTrainedModel

from kvpress_amd import _native
from kvpress_amd.presses.scorer_press import ScorerPress


class KVzapConfig(PretrainedConfig):
    model_type = "kvzap"
    # the dimensions are required, as in the reference: transformers 5.x must not build a default instance to diff against when it
    # prints or saves the config (from_pretrained does both)
    has_no_defaults_at_init = True

    def __init__(self, *, input_dim: int, output_dim: int, n_modules: int, hidden_dim: Optional[int] = None, **kwargs):
        super().__init__(**kwargs)
        self.input_dim = input_dim
        self.output_dim = output_dim
        self.hidden_dim = hidden_dim
        self.n_modules = n_modules


class KVzapModel(PreTrainedModel):
    config_class = KVzapConfig  # type: ignore[assignment]

    def __init__(self, config):
        super().__init__(config)
        self.all_tied_weights_keys = {}
        if config.hidden_dim is None:      # linear model (kvzap_press.py:33-35)
            self.layers = nn.ModuleList([nn.Linear(config.input_dim, config.output_dim) for _ in range(config.n_modules)])
        else:                              # two-layer MLP (kvzap_press.py:38-45)
            self.layers = nn.ModuleList(
                nn.Sequential(nn.Linear(config.input_dim, config.hidden_dim), nn.GELU(), nn.Linear(config.hidden_dim, config.output_dim))
                for _ in range(config.n_modules))

    def forward(self, x):
        """x [batch, n_modules, input_dim] -> [batch, n_modules, output_dim]: layer i on slice i (the training-time form; the press
        calls one layer at a time)"""
        outs = [layer(x[:, i]) for i, layer in enumerate(self.layers)]
        return torch.stack(outs, dim=1)


@dataclass
class KVzapPress(ScorerPress):
    """KVzap: a fast approximation of KVzip for prefilling and decoding; ``model_type`` is "linear" or "mlp"."""

    model_type: Literal["linear", "mlp"] = "mlp"
    kvzap_model_name: Optional[str] = field(default=None, init=False)

    kvzap_model = None   # a KVzapModel; assign one to skip the hub

    def post_init_from_model(self, model):
        kvzap_model_name = f"nvidia/KVzap-{self.model_type}-{model.config.name_or_path.split('/')[-1]}"
        # an assigned model (kvzap_model_name still None) is kept; one this method loaded is replaced when the served model changes
        if self.kvzap_model is None or (self.kvzap_model_name is not None and kvzap_model_name != self.kvzap_model_name):
            self.kvzap_model_name = kvzap_model_name
            self.kvzap_model = KVzapModel.from_pretrained(self.kvzap_model_name)

    def _packed(self, layer_idx: int, device: torch.device, dtype: torch.dtype) -> tuple:
        """(w1, b1, w2, b2) of one layer, contiguous on ``device`` in ``dtype`` (w2 = b2 = None for the linear model); built once"""
        cache = self.__dict__.setdefault("_packed_layers", {})
        key = (id(self.kvzap_model), layer_idx, device, dtype)
        hit = cache.get(key)
        if hit is None:
            if cache and next(iter(cache))[0] != key[0]:     # another model was assigned: its packs are dead
                cache.clear()
            layer = self.kvzap_model.layers[layer_idx]
            linears = [layer] if isinstance(layer, nn.Linear) else [layer[0], layer[2]]
            packed = [t.detach().to(device=device, dtype=dtype).contiguous() for lin in linears for t in (lin.weight, lin.bias)]
            hit = cache[key] = tuple(packed) if len(packed) == 4 else (packed[0], packed[1], None, None)
        return hit

    def score(self, module: nn.Module, hidden_states: torch.Tensor, keys: torch.Tensor, values: torch.Tensor,
              attentions: torch.Tensor, kwargs: dict) -> torch.Tensor:
        """float32 [B, Hkv, q_len]: the surrogate of layer ``module.layer_idx`` on the hidden states (kvzap_press.py:79-82)"""
        assert self.kvzap_model is not None, "KVzapPress has no surrogate model: assign kvzap_model or enter the press with a model"
        w1, b1, w2, b2 = self._packed(int(module.layer_idx), hidden_states.device, hidden_states.dtype)
        return _native.kvzap_score(hidden_states, w1, b1, w2, b2)
