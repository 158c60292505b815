"""The reference's behavioural tests of the decoding presses (tests/test_decoding_compression.py of the reference) re-created for CAMPress on
the tiny random-init Llama through the pipeline; shared by tests/test_cam_host.py (CPU, oracle-backed entry points) and
tests/test_gpu_cam.py (the HIP kernels)."""
import torch

import _inputs
from _support import cache_sizes, tiny_pipeline
from kvpress_amd.utils import extract_keys_and_values


def _watched(press, cam):
    """after every call of the hook the layer's running sum is as long as its cache"""
    inner = cam.forward_hook
    seen = []

    def hook(module, input, kwargs, output):
        out = inner(module, input, kwargs, output)
        n = extract_keys_and_values(kwargs["past_key_values"], module.layer_idx)[0].shape[2]     # (a QuantizedCache: its quantised part)
        if int(module.layer_idx) in cam._running_attn_sum:
            run = cam._running_attn_sum[int(module.layer_idx)]
            assert run.dtype == torch.float32 and run.shape[-1] == n, (run.shape, n)
            seen.append(n)
        return out

    cam.forward_hook = hook
    return seen


def check_cam_pipeline(device, dtype, eager=False):
    """the reference's behavioural tests (tests/test_decoding_compression.py) with CAMPress; shared with tests/test_gpu_cam.py"""
    from transformers import DynamicCache

    import kvpress_amd as P

    pipe = tiny_pipeline(device, dtype, eager)
    for target, interval, budget in ((32, 4, 32), (64, 3, 2), (128, 5, 200)):
        press = P.CAMPress(base_press=P.KnormPress(compression_ratio=0.5), compression_interval=interval, target_size=target, merge_budget=budget)
        seen = _watched(press, press)
        cache = DynamicCache()
        res = pipe(_inputs.tiny_context(100 if target < 128 else 140), question="w1 w2 w3", press=press, cache=cache, max_new_tokens=20)
        assert isinstance(res["answer"], str) and seen
        assert all(target <= n <= target + interval - 1 for n in cache_sizes(cache)), (target, cache_sizes(cache))
        assert press._running_attn_sum == {} and press._attn_buffer == {}        # the context manager's exit resets
    # the cache is below the target: steps are counted, nothing is compressed
    press = P.CAMPress(base_press=P.KnormPress(), compression_interval=2, target_size=400)
    cache = DynamicCache()
    pipe(_inputs.tiny_context(50), question="w6", press=press, cache=cache, max_new_tokens=6)
    assert all(n > 50 for n in cache_sizes(cache))
    # a QuantizedCache: the merged keys / values are re-quantised into the layer (DecodingPress's write-back).  As in the reference the
    # press sees the quantised part only, which grows by the residual buffer's 8 tokens at a time.
    press = P.CAMPress(base_press=P.KnormPress(), compression_interval=3, target_size=40, merge_budget=4)
    seen = _watched(press, press)
    cache = _inputs.make_fixed_point_cache(pipe.model.config)
    pipe(_inputs.tiny_context(70), question="w2 w5", press=press, cache=cache, max_new_tokens=10)
    lens = [cache.get_seq_length(i) for i in range(len(cache.layers))]
    assert seen and all(40 <= n <= 40 + 8 + 3 - 1 for n in lens), lens
    cam = P.CAMPress(base_press=P.KnormPress(), compression_interval=3, target_size=48, merge_budget=4)
    combined = P.PrefillDecodingPress(prefilling_press=P.KnormPress(compression_ratio=0.6), decoding_press=cam)
    seen = _watched(combined, cam)
    cache = DynamicCache()
    pipe(_inputs.tiny_context(130), question="w4 w5", press=combined, cache=cache, max_new_tokens=15)
    assert seen and all(48 <= n <= 48 + 3 - 1 for n in cache_sizes(cache)), cache_sizes(cache)
    assert combined.prefilling_press.kept_order == "score"                     # CAM's windows are neighbours in CACHE order
    # one press object, two sequences of different length: nothing of the first is added to in the second
    press = P.CAMPress(base_press=P.KnormPress(), compression_interval=3, target_size=40, merge_budget=8)
    outs = []
    for n_ctx in (60, 75, 60):
        cache = DynamicCache()
        torch.manual_seed(0)                                                     # the Bernoulli draws
        outs.append((pipe(_inputs.tiny_context(n_ctx), question="w3", press=press, cache=cache, max_new_tokens=9)["answer"], cache_sizes(cache)))
    assert outs[0] == outs[2]
