"""FastKVzipPress (kvpress/presses/fastkvzip_press.py:23-287): a small per-layer gate predicts KVzip's importance score of every KV pair
from the hidden states the attention layer receives, in the one ordinary prefill and with no reconstruction pass
(https://arxiv.org/abs/2601.17668).

On the library: one ``kvp_fastkvzip_score`` call per layer -- both projections, the two RMSNorms, the logits against the key and the
sink keys, the exps, the group mean and the protected positions of :240-247 -- written straight into the layer's slice of one
``[L, B, Hkv, S]`` score table, with nothing of extent ``S x columns`` stored (the reference keeps ``q`` [S, Hkv*G*16] and ``logit_base``
[Hkv, S, 16, G] in float32).  ``compress_post`` is KVzipPress's (kvpress_amd.presses.kvzip_press.mask_lowest_scores): K and V stay in the
cache and the pruned triples go to ``module.masked_key_indices`` (kvpress_amd.attention_patch).

``FastKVzipGate`` keeps the reference's constructor and state-dict keys and dtypes, so the published gates (``Jang-Hyun/Fast-KVzip``) load
with ``load_state_dict``; here it is a parameter container -- the press never calls a torch forward.  ``load_fastkvzip``, ``get_gate_id``
and ``get_gate_weight`` keep the reference's names; the hub is asked only when ``press.gates`` is None.

Defined deviations: the scores are float32 whatever the gate's dtype and everything after the products is float32
(the reference rounds the projections and the normalised vectors to the gate's dtype); a batch of more than one sequence works, one row
per batch element (the reference's gate squeezes batch 0)."""
from __future__ import annotations

import logging
import math
import re
from contextlib import contextmanager
from dataclasses import dataclass, field
from typing import Generator

import torch
from torch import nn

from kvpress_amd import _native
from kvpress_amd.attention_patch import patch_attention_functions
from kvpress_amd.presses.base_press import SUPPORTED_MODEL_NAMES, BasePress, _language_model, is_prefilling
from kvpress_amd.presses.kvzip_press import mask_lowest_scores
from kvpress_amd.utils import _is_quantized

logger = logging.getLogger(__name__)


class _GateNorm(nn.Module):
    """the parameters of the reference's Qwen3RMSNorm(output_dim): a float32 ``weight`` of ones and ``variance_epsilon``"""

    def __init__(self, dim: int, eps: float = 1e-6):
        super().__init__()
        self.weight = nn.Parameter(torch.ones(dim))
        self.variance_epsilon = eps


class FastKVzipGate(nn.Module):
    """Fast KVzip gate (fastkvzip_press.py:23-52): the parameters of one layer.  The scores are computed by ``kvp_fastkvzip_score``."""

    def __init__(self, index: int, input_dim: int, nhead: int, ngroup: int, dtype: torch.dtype, output_dim: int = 16, sink: int = 16):
        super().__init__()
        self.index = index
        self.output_dim = output_dim
        self.nhead = nhead
        self.ngroup = ngroup
        self.sink = sink

        self.q_proj = nn.Linear(input_dim, nhead * ngroup * output_dim, bias=True, dtype=dtype)
        self.k_proj = nn.Linear(input_dim, nhead * output_dim, bias=False, dtype=dtype)
        self.q_norm = _GateNorm(output_dim)
        self.k_norm = _GateNorm(output_dim)
        self.k_base = nn.Parameter(torch.zeros([nhead, 1, sink, output_dim]))
        self.b = nn.Parameter(torch.zeros([nhead, 1, ngroup], dtype=dtype))

        self.d = math.sqrt(self.output_dim)

    def forward(self, hidden_states: torch.Tensor):
        raise NotImplementedError("FastKVzipGate holds parameters only: FastKVzipPress scores with kvp_fastkvzip_score")

    def extra_repr(self):
        return f"index={self.index}, output_dim={self.output_dim}, nhead={self.nhead}, ngroup={self.ngroup}, sink={self.sink}"


GATE_REPO = "Jang-Hyun/Fast-KVzip"     # the hub repository of the published gates: <model name, lower case>/q<G>_dim16_sink16.pt


def get_gate_id(model_name: str) -> str:
    """The file of the published gates of a model inside GATE_REPO; the group size G comes from the model's config."""
    from transformers import AutoConfig

    config = AutoConfig.from_pretrained(model_name)
    config = getattr(config, "text_config", config)
    group = config.num_attention_heads // config.num_key_value_heads
    return f"{model_name.rsplit('/', 1)[-1].lower()}/q{group}_dim16_sink16.pt"


def get_gate_weight(model_name: str):
    """(the per-layer state dicts of a model's published gates, their gate id), fetched from the hub"""
    from huggingface_hub import hf_hub_download

    gate_id = get_gate_id(model_name)
    checkpoint = torch.load(hf_hub_download(repo_id=GATE_REPO, filename=gate_id, repo_type="model"), weights_only=False)
    return checkpoint["module"], gate_id


def load_fastkvzip(model_name: str = "Qwen/Qwen3-8B", device: str = "cuda") -> list:
    """One FastKVzipGate per layer holding a model's published gates.  The geometry is read off the first layer's tensors (q_proj.weight
    is [Hkv * G * D, hidden], k_proj.weight [Hkv * D, hidden], q_norm.weight [D]) and the number of sink keys off the file name."""
    assert model_name, "load_fastkvzip needs the served model's name"
    layers, gate_id = get_gate_weight(model_name)
    wq, wk, dim = layers[0]["q_proj.weight"], layers[0]["k_proj.weight"], layers[0]["q_norm.weight"].shape[-1]
    sink = re.search(r"sink(\d+)", gate_id)
    gates = []
    for index, state in enumerate(layers):
        gate = FastKVzipGate(index, wq.shape[1], wk.shape[0] // dim, wq.shape[0] // wk.shape[0], wq.dtype, dim, int(sink.group(1)) if sink else 0)
        gate.load_state_dict(state)
        gates.append(gate.to(device))
    logger.info(f"FastKVzip gates {gate_id}: {len(gates)} layers")
    return gates


@dataclass
class FastKVzipPress(BasePress):
    """Fast KVzip (https://arxiv.org/abs/2601.17668): KV importance from gates trained on KVzip's scores.

    Parameters
    ----------
    compression_ratio : float, default=0.0
        Fraction of key-value pairs to remove during compression.
    layerwise : bool, default=False
        Uniform compression ratio across layers; when False the overall ratio is kept and every layer gets its own.
    n_sink : int, default=4
        Number of initial tokens to preserve as attention sinks.
    window_size : int, default=4096
        Number of last tokens retained for contexts of 32000 tokens and more.
    window_ratio : float, default=0.02
        Fraction of the context length retained at its end for shorter contexts.
    """

    compression_ratio: float = 0.0
    layerwise: bool = False

    n_sink: int = 4
    window_size: int = 4096
    window_ratio: float = 0.02

    gates: list[nn.Module] | None = field(init=False, default=None)
    score_val: list[torch.Tensor] | torch.Tensor | None = field(init=False, default=None)

    def __post_init__(self):
        patch_attention_functions()

    def post_init_from_model(self, model):
        """Assigned gates are kept; with none, the served model's published gates are fetched."""
        if self.gates is not None:
            return
        name = model.config.name_or_path
        try:
            self.gates = load_fastkvzip(model_name=name, device=model.device)
        except Exception as e:
            raise RuntimeError(f"no published FastKVzip gates could be loaded for {name!r} (https://huggingface.co/{GATE_REPO}); "
                               "assign press.gates to use gates of your own") from e

    @contextmanager
    def __call__(self, model) -> Generator:
        """The prefill runs inside the ``with`` and every layer's hook scores it; on the way out the lowest scores are masked
        (fastkvzip_press.py:184-213)."""
        if type(model).__name__ not in SUPPORTED_MODEL_NAMES:
            logger.warning(f"Model {type(model)} not tested, supported models: {SUPPORTED_MODEL_NAMES}")
        if any(c.__name__ == "Gemma3PreTrainedModel" for c in type(model).__mro__):
            # the reference skips the sliding layers and then cannot stack their missing scores (:199-204, :256)
            raise ValueError("FastKVzipPress is not supported for Gemma3")

        self.post_init_from_model(model)
        hooks = []
        try:
            self.score_val = None   # reset every prefilling; allocated by the first hooked layer
            self._n_layers = len(model.model.layers)
            language_model = _language_model(model)
            for layer in language_model.layers:
                if hasattr(language_model, "rotary_emb"):
                    layer.self_attn.rotary_emb = language_model.rotary_emb
                hooks.append(layer.self_attn.register_forward_hook(self.forward_hook, with_kwargs=True))
            yield

            self.compress_post(model)
        finally:
            for hook in hooks:
                hook.remove()
        _native.async_error_check()   # as BasePress.__call__: reached only when nothing raised

    def forward_hook(self, module: nn.Module, input: list[torch.Tensor], kwargs: dict, output: list):
        """Score the layer during the prefill; later forwards pass through (fastkvzip_press.py:215-230)."""
        hidden_states = kwargs["hidden_states"]
        q_len = hidden_states.shape[1]
        cache = kwargs.get("past_key_values", None) or kwargs.get("past_key_value", None)
        cache_layer = cache.layers[module.layer_idx]
        kv_len = cache.get_seq_length(module.layer_idx) if _is_quantized(cache) else cache_layer.keys.shape[2]
        if not is_prefilling(kv_len, q_len, kwargs, cache_layer):
            return output

        self._score_fast(module, hidden_states)
        return output

    def _packed(self, layer_idx: int, device: torch.device, dtype: torch.dtype) -> tuple:
        """(wq, bq, wk, b, gq, gk, k_base, eps) of one layer as the library takes them: the projections and ``b`` contiguous on ``device`` in
        ``dtype``, the norm weights and ``k_base`` [Hkv, J, D] in float32; built once per (gates, layer, device, dtype)"""
        cache = self.__dict__.setdefault("_packed_layers", {})
        key = (id(self.gates), layer_idx, device, dtype)
        hit = cache.get(key)
        if hit is None:
            if cache and next(iter(cache))[0] != key[0]:     # other gates were assigned: their packs are dead
                cache.clear()
            gate = self.gates[layer_idx]
            nhead, ngroup, dim = gate.nhead, gate.ngroup, gate.output_dim

            def cast(t, dt, *shape):
                return t.detach().to(device=device, dtype=dt).reshape(*shape).contiguous()

            hit = cache[key] = (cast(gate.q_proj.weight, dtype, nhead * ngroup * dim, -1), cast(gate.q_proj.bias, dtype, -1),
                                cast(gate.k_proj.weight, dtype, nhead * dim, -1), cast(gate.b, dtype, nhead, ngroup),
                                cast(gate.q_norm.weight, torch.float32, dim), cast(gate.k_norm.weight, torch.float32, dim),
                                cast(gate.k_base, torch.float32, nhead, -1, dim), float(gate.q_norm.variance_epsilon))
        return hit

    def _score_fast(self, module: nn.Module, hidden_states: torch.Tensor):
        """The layer's scores into its slice of the score table (fastkvzip_press.py:232-249)."""
        layer_idx = int(module.layer_idx)
        bsz, ctx_len, _ = hidden_states.shape
        wq, bq, wk, b, gq, gk, k_base, eps = self._packed(layer_idx, hidden_states.device, hidden_states.dtype)
        if self.score_val is None:   # float32 whatever the model's dtype
            self.score_val = torch.empty((self._n_layers, bsz, b.shape[0], ctx_len), dtype=torch.float32, device=hidden_states.device)

        window_size = int(ctx_len * self.window_ratio) if ctx_len < 32000 else self.window_size
        # `scores[:, :, -window_size:] = 1.0` with window_size == 0 sets EVERY score (contexts under 50 tokens at the default ratio)
        protect_tail = ctx_len if window_size == 0 else window_size
        _native.fastkvzip_score(hidden_states, wq, bq, wk, b, gq, gk, k_base, eps, max(int(self.n_sink), 0), protect_tail,
                                out=self.score_val[layer_idx])

    def compress_post(self, model):
        """The (head, position) pairs every layer masks (fastkvzip_press.py:251-287): KVzipPress's selection."""
        if self.score_val is not None:   # (None: no prefill ran inside the `with`)
            mask_lowest_scores(model, self.score_val, self.compression_ratio, self.layerwise)
