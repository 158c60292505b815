"""kvpress_amd: MI355X-native score -> top-k -> gather hot path of NVIDIA/kvpress.

The public API mirrors the reference's (same class names, dataclass fields and method signatures): BasePress / ScorerPress,
the three core scorers (KnormPress, SnapKVPress, ExpectedAttentionPress), the scorers and wrappers of SURVEY.md §8(f) that build on the
same kernels (see __all__) and the "kv-press-text-generation" pipeline, registered on import like the
reference's.  Everything below ``compress()`` runs in hand-written HIP kernels (gfx950) reached through the C ABI of
include/kvpress_hip.h; there is no CPU or pure-PyTorch fallback.
"""
from kvpress_amd.presses.adakv_press import AdaKVPress
from kvpress_amd.presses.base_press import BasePress
from kvpress_amd.presses.cam_press import CAMPress
from kvpress_amd.presses.chunk_press import ChunkPress
from kvpress_amd.presses.compactor_press import CompactorPress
from kvpress_amd.presses.composed_press import ComposedPress
from kvpress_amd.presses.criticalkv_press import CriticalAdaKVPress
from kvpress_amd.presses.cur_press import CURPress
from kvpress_amd.presses.decoding_press import CompressionRatioDecodingPress, DecodingPress, PrefillDecodingPress
from kvpress_amd.presses.expected_attention_press import ExpectedAttentionPress
from kvpress_amd.presses.fastkvzip_press import FastKVzipPress
from kvpress_amd.presses.finch_press import FinchPress
from kvpress_amd.presses.key_rerotation_press import KeyRerotationPress
from kvpress_amd.presses.keydiff_press import KeyDiffPress
from kvpress_amd.presses.knorm_press import KnormPress
from kvpress_amd.presses.kvzap_press import KVzapPress
from kvpress_amd.presses.leverage_press import LeverageScorePress
from kvpress_amd.presses.merging_press import MergingPress
from kvpress_amd.presses.non_causal_attention_press import NonCausalAttnPress
from kvpress_amd.presses.per_layer_compression_press import PerLayerCompressionPress
from kvpress_amd.presses.pyramidkv_press import PyramidKVPress
from kvpress_amd.presses.qfilter_press import QFilterPress
from kvpress_amd.presses.random_press import RandomPress
from kvpress_amd.presses.scorer_press import ScorerPress
from kvpress_amd.presses.snapkv_press import SnapKVPress
from kvpress_amd.presses.streaming_llm_press import StreamingLLMPress
from kvpress_amd.presses.tova_press import TOVAPress

__version__ = "0.1.0"
# the path (a), the scorers that reuse its kernels (f-2), the selection wrappers (f-3), the decode-time step (f-4), the
# pipeline (f-1); plus four tiny host-only presses the reference's own test fixtures for those rows are built from (Composed, PerLayer,
# Random, StreamingLLM); plus the Compactor family (NonCausalAttn, LeverageScore, Compactor), MergingPress, CAMPress, CriticalAdaKVPress, KVzapPress and FastKVzipPress.  Presses outside that scope that still have kernels here live in kvpress_amd.contrib.
__all__ = ["BasePress", "ScorerPress", "KnormPress", "SnapKVPress", "ExpectedAttentionPress", "PyramidKVPress", "TOVAPress", "KeyDiffPress", "QFilterPress",
           "CURPress", "FinchPress", "ChunkPress", "KeyRerotationPress", "AdaKVPress", "DecodingPress", "CompressionRatioDecodingPress", "PrefillDecodingPress",
           "ComposedPress", "PerLayerCompressionPress", "RandomPress", "StreamingLLMPress", "KVPressTextGenerationPipeline",
           "NonCausalAttnPress", "LeverageScorePress", "CompactorPress", "MergingPress", "CAMPress", "CriticalAdaKVPress", "KVzapPress", "FastKVzipPress"]


# The reference exports every press at top level (kvpress/__init__.py:7-49).  The five out-of-scope presses that exist here resolve
# lazily to kvpress_amd.contrib (so `from kvpress_amd import ThinKPress` works like `from kvpress import ThinKPress` without the hot-path
# package importing its contrib sub-package); the reference's other presses are NOT part of this package and say so.
_CONTRIB = ("BlockPress", "ChunkKVPress", "LagKVPress", "ObservedAttentionPress", "ThinKPress")
_NOT_BUILT = ("CapPress", "CriticalKVPress", "DMSPress", "DuoAttentionPress",
              "ExpectedAttentionStatsPress", "KVComposePress", "KVzipPress", "LUKVPress",
              "RestoreKVPress", "SimLayerKVPress")


def __getattr__(name):
    if name in _CONTRIB:
        import importlib

        return getattr(importlib.import_module("kvpress_amd.contrib"), name)
    if name == "SUPPORTED_MODELS":     # kvpress/presses/base_press.py:26-33 (model classes; here the names are matched, resolved on demand)
        import transformers

        from kvpress_amd.presses.base_press import SUPPORTED_MODEL_NAMES

        return tuple(getattr(transformers, n) for n in SUPPORTED_MODEL_NAMES)
    if name == "CriticalKVPress":      # built, but the top-level name stays refused for now
        raise AttributeError("kvpress_amd has no top-level CriticalKVPress: the name is still listed outside the hot-path scope of this "
                             "package (DESIGN.md section 9); the class lives at kvpress_amd.presses.criticalkv_press.CriticalKVPress")
    if name == "KVzipPress":           # built, the top-level name likewise still refused
        raise AttributeError("kvpress_amd has no top-level KVzipPress: the name is still listed outside the hot-path scope of this "
                             "package (DESIGN.md section 9); the class lives at kvpress_amd.presses.kvzip_press.KVzipPress")
    if name == "DMSPress":             # built (it drives KVzapPress), the top-level name likewise still refused
        raise AttributeError("kvpress_amd has no top-level DMSPress: the name is still listed outside the hot-path scope of this "
                             "package (DESIGN.md section 9); the class lives at kvpress_amd.presses.dms_press.DMSPress")
    if name in _NOT_BUILT:
        raise AttributeError(f"kvpress_amd has no {name}: it is outside the hot-path scope of this package (SURVEY.md section 8, DESIGN.md "
                             f"section 9); use NVIDIA/kvpress's {name}")
    raise AttributeError(f"module 'kvpress_amd' has no attribute {name!r}")


def __dir__():
    return sorted(list(globals()) + list(_CONTRIB))


# importing the package registers the "kv-press-text-generation" task, as `import kvpress` does (kvpress/__init__.py, pipeline.py:326-331)
from kvpress_amd.pipeline import KVPressTextGenerationPipeline  # noqa: E402
