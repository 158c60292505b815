"""ctypes binding of libkvpress_hip.so (include/kvpress_hip.h) for torch tensors on a HIP device.

There is deliberately NO fallback: if the shared library is missing, or a tensor is not on a
GPU, the call raises.  PyTorch is used for device memory (outputs / workspaces come from the
caching allocator, so they are stream-ordered) and for the current stream only.
"""
from __future__ import annotations

import ctypes
import os
import threading
from ctypes import c_char_p, c_double, c_float, c_int, c_int32, c_int64, c_size_t, c_void_p
from typing import Optional

import torch  # must be imported before the .so so that it binds to torch's libamdhip64.so.7

_HERE = os.path.dirname(os.path.abspath(__file__))
# KVPRESS_HIP_LIB: an alternative build of the same library (kernel labs under tools/); unset in production
LIB_PATH = os.environ.get("KVPRESS_HIP_LIB") or os.path.join(_HERE, "lib", "libkvpress_hip.so")
CONTRIB_LIB_PATH = os.path.join(os.path.dirname(LIB_PATH), "libkvpress_hip_contrib.so")

KVP_F32, KVP_F16, KVP_BF16 = 0, 1, 2
KVP_EASYNC = -5
ORDER_POSITION, ORDER_SCORE = 0, 1
TOPK_WS_CLEAN, TOPK_SMALLEST = 0x100, 0x200
CUR_LEVERAGE = {"key": 0, "value": 1, "kv_avg": 2, "kv_product": 3}
_DTYPES = {torch.float32: KVP_F32, torch.float16: KVP_F16, torch.bfloat16: KVP_BF16}
_TOPK_WS: dict = {}   # (thread, kind of use, device index, stream, call shape...) -> zero-initialised, self-cleaning workspace (_clean_ws)
_TOPK_WS_LOCK = threading.Lock()
_WS_BYTES: dict = {}  # (kvp_*_workspace_bytes, shape...) -> its answer (_ws_bytes)

# ---- loading and the signature tables -----------------------------------------------------------------------------------------------
# name -> (restype, argtypes); mirrors include/kvpress_hip.h line by line (tests/test_capi_symbols.py::test_binding_covers_header holds
# every entry against its prototype: return type, arity, order and type of the parameters)
_I64 = c_int64
SIGNATURES = {
    "kvp_version": (c_int, []),
    "kvp_last_error": (c_char_p, []),
    "kvp_async_error_check": (c_int, []),
    "kvp_rownorm_score": (c_int, [c_void_p, c_int, _I64, _I64, _I64, _I64, _I64, _I64, _I64, c_float, c_void_p, c_void_p]),
    "kvp_rowdot_score": (c_int, [c_void_p, c_int, _I64, _I64, _I64, _I64, _I64, _I64, _I64, c_void_p, _I64, c_float, c_void_p, c_void_p]),
    "kvp_knorm_compress_workspace_bytes": (c_size_t, [_I64] * 4),
    "kvp_knorm_compress": (c_int, [c_void_p, _I64, _I64, _I64, c_void_p, _I64, _I64, _I64, c_int, _I64, _I64, _I64, _I64, _I64,
                                   c_void_p, c_void_p, c_void_p, c_size_t, c_int, c_void_p]),
    "kvp_snapkv_compress_workspace_bytes": (c_size_t, [_I64] * 7),
    "kvp_snapkv_compress_rope": (c_int, [c_void_p, _I64, _I64, _I64, c_void_p, c_void_p, _I64, _I64, c_void_p, _I64, _I64, _I64,
                                         c_void_p, _I64, _I64, _I64, c_int, _I64, _I64, _I64, _I64, _I64, _I64, c_int, _I64,
                                         c_void_p, c_void_p, c_void_p, c_size_t, c_int, c_void_p]),
    "kvp_cur_workspace_bytes": (c_size_t, [_I64] * 3),
    "kvp_cur_score": (c_int, [c_void_p, _I64, _I64, _I64, c_void_p, _I64, _I64, _I64, c_int, _I64, _I64, _I64, _I64, c_int, _I64, _I64,
                              c_void_p, c_void_p, c_size_t, c_void_p]),
    "kvp_keydiff_workspace_bytes": (c_size_t, [_I64] * 4),
    "kvp_keydiff_score": (c_int, [c_void_p, c_int, _I64, _I64, _I64, _I64, _I64, _I64, _I64, c_void_p, c_void_p, c_size_t, c_void_p]),
    "kvp_scores_head_mean": (c_int, [c_void_p, _I64, _I64, _I64, _I64, _I64, c_void_p]),
    "kvp_snapkv_workspace_bytes": (c_size_t, [_I64] * 6),
    "kvp_snapkv_score": (c_int, [c_void_p, _I64, _I64, _I64, c_void_p, _I64, _I64, _I64, c_int,
                                 _I64, _I64, _I64, _I64, _I64, _I64, c_int, c_void_p, c_void_p, c_size_t, c_void_p]),
    "kvp_snapkv_score_rope": (c_int, [c_void_p, _I64, _I64, _I64, c_void_p, c_void_p, _I64, _I64, c_void_p, _I64, _I64, _I64, c_int,
                                      _I64, _I64, _I64, _I64, _I64, _I64, c_int, c_void_p, c_void_p, c_size_t, c_void_p]),
    "kvp_finch_score": (c_int, [c_void_p, _I64, _I64, _I64, c_void_p, c_void_p, _I64, _I64, c_void_p, _I64, _I64, _I64, c_int,
                                _I64, _I64, _I64, _I64, _I64, _I64, c_int, c_void_p, c_void_p, c_size_t, c_void_p]),
    "kvp_snapkv_qproj_rope": (c_int, [c_void_p, _I64, _I64, c_void_p, c_void_p, c_void_p, _I64, _I64, c_int, _I64, _I64, _I64, _I64, _I64,
                                      c_void_p, c_void_p]),
    "kvp_snapkv_score_hidden": (c_int, [c_void_p, _I64, _I64, c_void_p, _I64, c_void_p, c_void_p, _I64, _I64, c_void_p, _I64, _I64, _I64,
                                        c_int, _I64, _I64, _I64, _I64, _I64, _I64, c_int, c_void_p, c_void_p, c_size_t, c_void_p]),
    "kvp_snapkv_compress_hidden": (c_int, [c_void_p, _I64, _I64, c_void_p, _I64, c_void_p, c_void_p, _I64, _I64, c_void_p, _I64, _I64, _I64,
                                           c_void_p, _I64, _I64, _I64, c_int, _I64, _I64, _I64, _I64, _I64, _I64, c_int, _I64,
                                           c_void_p, c_void_p, c_void_p, c_size_t, c_int, c_void_p]),
    "kvp_snapkv_score_from_attn": (c_int, [c_void_p, _I64, _I64, _I64, c_int, _I64, _I64, _I64, _I64, _I64, c_int,
                                           c_void_p, c_void_p, c_size_t, c_void_p]),
    "kvp_ea_qstats_workspace_bytes": (c_size_t, [_I64] * 4),
    "kvp_ea_qstats": (c_int, [c_void_p, _I64, _I64, _I64, c_int, _I64, _I64, _I64, _I64, c_void_p, c_void_p,
                              c_void_p, c_size_t, c_void_p]),
    "kvp_ea_score_workspace_bytes": (c_size_t, [_I64] * 5),
    "kvp_ea_score": (c_int, [c_void_p, _I64, _I64, _I64, c_void_p, _I64, _I64, _I64, c_int, c_void_p, c_void_p,
                             _I64, _I64, _I64, _I64, _I64, _I64, c_int, c_float, c_void_p, c_void_p, c_size_t, c_void_p]),
    "kvp_topk_workspace_bytes": (c_size_t, [_I64] * 3),
    "kvp_topk_order_workspace_bytes": (c_size_t, [_I64] * 3),
    "kvp_topk_select": (c_int, [c_void_p, _I64, _I64, _I64, _I64, c_int, c_void_p, c_void_p, c_size_t, c_void_p]),
    "kvp_topk_segmented_workspace_bytes": (c_size_t, [_I64] * 4),
    "kvp_topk_select_segmented": (c_int, [c_void_p, _I64, _I64, _I64, _I64, _I64, c_int, c_void_p, c_void_p, c_size_t, c_void_p]),
    "kvp_scores_fill_at": (c_int, [c_void_p, _I64, _I64, _I64, c_void_p, _I64, c_float, c_void_p]),
    "kvp_rerotate_keys": (c_int, [c_void_p, c_int, _I64, _I64, _I64, _I64, c_void_p, c_void_p, c_void_p]),
    "kvp_gather_kv": (c_int, [c_void_p, _I64, _I64, _I64, c_void_p, _I64, _I64, _I64, c_int, _I64, _I64, _I64, _I64,
                              c_void_p, _I64, c_void_p, c_void_p, c_void_p]),
    "kvp_gather_kv_rerotate": (c_int, [c_void_p, _I64, _I64, _I64, c_void_p, _I64, _I64, _I64, c_int, _I64, _I64, _I64, _I64,
                                       c_void_p, _I64, c_void_p, c_void_p, c_void_p, c_void_p]),
    "kvp_ncattn_workspace_bytes": (c_size_t, [_I64] * 3),
    "kvp_ncattn_score": (c_int, [c_void_p, _I64, _I64, _I64, c_void_p, c_void_p, _I64, _I64, c_void_p, _I64, _I64, _I64, c_void_p, _I64, _I64,
                                 _I64, c_int, _I64, _I64, _I64, _I64, _I64, _I64, c_void_p, c_void_p, c_void_p, c_size_t, c_void_p]),
    "kvp_leverage_workspace_bytes": (c_size_t, [_I64] * 5),
    "kvp_leverage_score": (c_int, [c_void_p, _I64, _I64, _I64, c_void_p, _I64, _I64, _I64, c_int, _I64, _I64, _I64, _I64, _I64,
                                   c_void_p, c_void_p, c_void_p, c_size_t, c_void_p]),
    "kvp_leverage_status": (c_int, [c_void_p, _I64, _I64, _I64, _I64, _I64, c_void_p]),
    "kvp_compactor_combine_workspace_bytes": (c_size_t, []),
    "kvp_compactor_combine": (c_int, [c_void_p, c_void_p, _I64, _I64, _I64, _I64, _I64, c_float, c_void_p, c_void_p, c_size_t, c_void_p]),
    "kvp_merge_workspace_bytes": (c_size_t, [_I64] * 5),
    "kvp_merge_values": (c_int, [c_void_p, _I64, _I64, _I64, c_void_p, _I64, _I64, _I64, c_void_p, c_void_p, c_void_p, c_int, _I64, _I64, _I64,
                                 _I64, _I64, c_double, c_double, c_void_p, c_size_t, c_void_p, c_void_p, c_void_p]),
    "kvp_cam_attn_workspace_bytes": (c_size_t, [_I64] * 4),
    "kvp_cam_attn_accumulate": (c_int, [c_void_p, _I64, _I64, _I64, c_void_p, c_void_p, _I64, _I64, c_void_p, _I64, _I64, _I64, c_int,
                                        _I64, _I64, _I64, _I64, _I64, c_void_p, _I64, _I64, _I64, _I64, c_void_p, c_size_t, c_void_p]),
    "kvp_cam_attn_accumulate_row": (c_int, [c_void_p, _I64, _I64, c_int, _I64, _I64, _I64, _I64, c_void_p, _I64, _I64, _I64, _I64, c_void_p]),
    "kvp_cam_merge_plan": (c_int, [c_void_p, c_void_p, _I64, c_void_p, _I64, _I64, _I64, _I64, _I64, _I64, _I64, _I64, c_void_p, c_void_p,
                                   c_void_p, c_void_p]),
    "kvp_cam_merge_prune": (c_int, [c_void_p, _I64, _I64, _I64, c_void_p, _I64, _I64, _I64, c_void_p, _I64, _I64, c_void_p, c_void_p, c_void_p,
                                    c_void_p, c_int, _I64, _I64, _I64, _I64, _I64, _I64, _I64, c_void_p, c_void_p, c_void_p, c_void_p]),
    "kvp_vwl1norm_workspace_bytes": (c_size_t, [_I64] * 6),
    "kvp_vwl1norm_rescale": (c_int, [c_void_p, _I64, _I64, _I64, c_int, c_void_p, _I64, _I64, _I64, _I64, _I64, _I64, _I64, c_void_p, _I64,
                                     c_float, c_void_p, c_void_p, c_size_t, c_void_p]),
    "kvp_scores_fill_prefix": (c_int, [c_void_p, _I64, _I64, _I64, c_void_p, _I64, c_void_p, c_float, c_void_p]),
    "kvp_kvzip_score_workspace_bytes": (c_size_t, [c_int] + [_I64] * 7),
    "kvp_kvzip_score": (c_int, [c_void_p, _I64, _I64, _I64, c_void_p, c_void_p, _I64, _I64, c_void_p, _I64, _I64, _I64, c_int, _I64, _I64, _I64,
                                _I64, _I64, _I64, _I64, _I64, _I64, c_void_p, c_void_p, c_void_p, _I64, c_void_p, c_size_t, c_void_p]),
    "kvp_kvzap_score_workspace_bytes": (c_size_t, [c_int] + [_I64] * 5),
    "kvp_kvzap_score": (c_int, [c_void_p, _I64, _I64, c_int, c_void_p, c_void_p, c_void_p, c_void_p, _I64, _I64, _I64, _I64, _I64,
                                c_void_p, _I64, _I64, _I64, c_void_p, c_size_t, c_void_p]),
    "kvp_threshold_select_workspace_bytes": (c_size_t, [_I64] * 3),
    "kvp_threshold_count": (c_int, [c_void_p, _I64, _I64, _I64, _I64, _I64, _I64, c_float, c_void_p, c_size_t, ctypes.POINTER(c_int64), c_void_p]),
    "kvp_threshold_select": (c_int, [c_void_p, _I64, _I64, _I64, _I64, _I64, _I64, c_float, _I64, c_void_p, c_size_t, _I64,
                                     c_void_p, c_void_p, c_void_p, c_void_p]),
    "kvp_fastkvzip_score_workspace_bytes": (c_size_t, [c_int] + [_I64] * 7),
    "kvp_fastkvzip_score": (c_int, [c_void_p, _I64, _I64, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                    _I64, _I64, _I64, _I64, _I64, _I64, _I64, c_float, _I64, _I64, c_void_p, _I64, _I64, _I64,
                                    c_void_p, c_size_t, c_void_p]),
}
# include/kvpress_hip_lab.h: measurement / test aids of the same library (bench.py, tools/, the select's residency tests)
LAB_SIGNATURES = {
    "kvp_prof_enable": (c_int, [c_int]),
    "kvp_prof_count": (c_int, []),
    "kvp_prof_get": (c_int, [c_int, ctypes.POINTER(c_char_p), ctypes.POINTER(c_float)]),
    "kvp_clock_probe": (c_int, [c_void_p, c_int, c_void_p]),
    "kvp_occupy_cus": (c_int, [c_int, c_int, c_int, c_int, c_void_p]),
    "kvp_tuning_reload": (c_int, []),
}
# include/kvpress_hip_extra.h: kernels of the presses outside SURVEY section 8 (kvpress_amd.contrib), their own shared library
CONTRIB_SIGNATURES = {
    "kvp_observed_attention_score": (c_int, [c_void_p, _I64, _I64, _I64, c_int, _I64, _I64, _I64, _I64, _I64, c_void_p, c_void_p]),
    "kvp_lagkv_score": (c_int, [c_void_p, _I64, _I64, _I64, c_void_p, _I64, _I64, _I64, c_int, _I64, _I64, _I64, _I64, _I64, _I64, c_int,
                                c_void_p, c_void_p]),
    "kvp_think_workspace_bytes": (c_size_t, [_I64] * 4),
    "kvp_think_channel_scores": (c_int, [c_void_p, _I64, _I64, _I64, c_void_p, _I64, _I64, _I64, c_int, _I64, _I64, _I64, _I64, _I64, _I64,
                                         c_void_p, c_void_p, c_size_t, c_void_p]),
    "kvp_zero_channels": (c_int, [c_void_p, _I64, _I64, _I64, c_int, _I64, _I64, _I64, _I64, c_void_p, _I64, c_void_p]),
}

_lib = None
_contrib_lib = None


class KvpressHipError(RuntimeError):
    pass


def lib() -> ctypes.CDLL:
    """Load libkvpress_hip.so (once).  Raises if it has not been built: there is no fallback."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise KvpressHipError(
                f"{LIB_PATH} not found: build it with `python -m kvpress_amd.build` (hipcc, gfx950). "
                "kvpress_amd has no CPU / pure-PyTorch fallback.")
        handle = ctypes.CDLL(LIB_PATH)
        for name, (res, args) in {**SIGNATURES, **LAB_SIGNATURES}.items():
            fn = getattr(handle, name)  # AttributeError if the ABI is incomplete
            fn.restype, fn.argtypes = res, args
        _lib = handle
    return _lib


def contrib_lib() -> ctypes.CDLL:
    """Load libkvpress_hip_contrib.so (once): LagKV / ThinK / ObservedAttention kernels (kvpress_amd.contrib).  It resolves the
    error / launch plumbing against libkvpress_hip.so, which is loaded first."""
    global _contrib_lib
    if _contrib_lib is None:
        lib()
        if not os.path.exists(CONTRIB_LIB_PATH):
            raise KvpressHipError(f"{CONTRIB_LIB_PATH} not found: build it with `python -m kvpress_amd.build` (hipcc, gfx950).")
        handle = ctypes.CDLL(CONTRIB_LIB_PATH)
        for name, (res, args) in CONTRIB_SIGNATURES.items():
            fn = getattr(handle, name)
            fn.restype, fn.argtypes = res, args
        _contrib_lib = handle
    return _contrib_lib


# ---- marshalling and workspace helpers ------------------------------------------------------------------------------------------------
def _check(rc: int, what: str):
    if rc != 0:
        msg = lib().kvp_last_error()
        if rc == KVP_EASYNC:
            # a kernel of an EARLIER call reported at run time that its result is invalid (the cluster select's barrier timed out:
            # include/kvpress_hip.h).  Its workspace -- whichever it was -- is dirty: no cached "clean" workspace survives.
            with _TOPK_WS_LOCK:
                _TOPK_WS.clear()
        raise KvpressHipError(f"{what} failed ({rc}): {msg.decode() if msg else ''}")


def _call(name: str, *args, contrib: bool = False, what: Optional[str] = None, clean_ws: Optional[torch.Tensor] = None):
    """Call the entry point ``name`` of the library (``contrib``: of the contrib library); a non-zero return code raises KvpressHipError under that same name (``what``:
    under another).  ``clean_ws`` is the cached self-cleaning workspace the call used: a failed call may leave dirty histograms
    behind, so it leaves the cache before the error is raised and is never reused as "clean"."""
    rc = getattr(contrib_lib() if contrib else lib(), name)(*args)
    if rc != 0:
        if clean_ws is not None:
            _drop_ws(clean_ws)
        _check(rc, what or name)


def async_error_check() -> None:
    """Raise KvpressHipError if a kernel has reported an asynchronous failure since the last check (no synchronisation: call it
    after a stream sync to cover everything enqueued so far).  No-op when the library has not been loaded."""
    if _lib is not None:
        _call("kvp_async_error_check")


def _dev(t: torch.Tensor):
    if not t.is_cuda:
        raise KvpressHipError(
            f"kvpress_amd kernels need tensors on a HIP device, got {t.device} (no CPU fallback exists)")
    if t.dtype not in _DTYPES:
        raise KvpressHipError(f"unsupported dtype {t.dtype} (float32 / float16 / bfloat16)")
    return t


def _rows(t: torch.Tensor) -> torch.Tensor:
    """_dev + a [..., D] view whose last dim is contiguous (sliced cache views pass through untouched)."""
    if not t.is_cuda or t.dtype not in _DTYPES:
        _dev(t)   # raises
    return t if (t.shape[-1] == 1 or t.stride(-1) == 1) else t.contiguous()


def _p(t: Optional[torch.Tensor]):
    return t.data_ptr() if t is not None else None   # (ints / None: ctypes converts them for a c_void_p parameter)


def _tensor(t: torch.Tensor, n: int = 3) -> tuple:
    """The argument group of a tensor: its pointer and the element strides of its first ``n`` dims; 0 for size-1 dims (torch reports
    arbitrary strides there)."""
    shape, stride = t.shape, t.stride()
    if n == 3:   # (spelled out: a third of the cost of the general form, on every call of the decode regime)
        return (t.data_ptr(), 0 if shape[0] == 1 else stride[0], 0 if shape[1] == 1 else stride[1], 0 if shape[2] == 1 else stride[2])
    return (t.data_ptr(), *[0 if shape[i] == 1 else stride[i] for i in range(n)])


def _kv(keys: torch.Tensor, values: torch.Tensor, same: bool = True):
    """The keys / values prelude: both on a device in a supported dtype with a contiguous last dim and (``same``) of one dtype and
    shape.  Returns them and B, H, S, D of the keys."""
    keys, values = _rows(keys), _rows(values)
    if same:
        assert keys.dtype == values.dtype and keys.shape == values.shape
    return (keys, values, *keys.shape)


def _queries(q: torch.Tensor, keys: torch.Tensor):
    """Window queries [B,Hq,W,D] for prepared keys [B,Hkv,S,D]: in the keys' dtype, last dim contiguous.  Returns them and
    B, Hq, Hkv, S, W, D."""
    q = _rows(q)
    if q.dtype != keys.dtype:
        q = q.to(keys.dtype)
    B, Hq, W, D = q.shape
    Bk, Hkv, S, Dk = keys.shape
    assert B == Bk and D == Dk and Hq % Hkv == 0, (q.shape, keys.shape)
    return q, B, Hq, Hkv, S, W, D


def _rotary(cos: torch.Tensor, sin: torch.Tensor, dt: torch.dtype, window: Optional[tuple] = None):
    """The rotary tables as the library takes them: dtype ``dt``, contiguous last dim, equal strides.  With ``window = (B, W, D)`` they
    are the window's, [1 or B, W, D], and a table with ONE row is broadcast over the window (stride 0), which is what the
    reference's ``cos[:, -W:].unsqueeze(1)`` does when a decoding step hands over the current position only (DecodingPress with a
    window scorer)."""
    cos, sin = _rows(cos.to(dt)), _rows(sin.to(dt))
    if window is not None:
        B, W, D = window
        assert cos.shape == sin.shape and cos.shape[-1] == D and cos.shape[0] in (1, B) and cos.shape[-2] in (1, W), (cos.shape, (B, W, D))
    if sin.stride() != cos.stride():
        sin, cos = sin.contiguous(), cos.contiguous()
    if window is not None and cos.shape[-2] == 1 and W > 1:
        cos, sin = cos.expand(-1, W, -1), sin.expand(-1, W, -1)
    return cos, sin


def _tables(cos: torch.Tensor, sin: torch.Tensor) -> tuple:
    """The argument group of _rotary's tables: both pointers and their common strides."""
    shape, stride = cos.shape, cos.stride()
    return (cos.data_ptr(), sin.data_ptr(), 0 if shape[0] == 1 else stride[0], 0 if shape[1] == 1 else stride[1])


def _stream(t: torch.Tensor):
    return torch.cuda.current_stream(t.device).cuda_stream   # (an int: ctypes converts it for a c_void_p parameter)


class _on_device:
    """``with _on_device(dev)`` only when ``dev`` is not already current: the context manager costs several microseconds
    per call, which is a tenth of a whole decode-regime compress (tools/host_overhead_probe.py)."""
    __slots__ = ("ctx",)

    def __init__(self, dev):
        self.ctx = None if dev.index is None or torch.cuda.current_device() == dev.index else torch.cuda.device(dev)

    def __enter__(self):
        if self.ctx is not None:
            self.ctx.__enter__()

    def __exit__(self, *exc):
        if self.ctx is not None:
            return self.ctx.__exit__(*exc)
        return False


def _ws(nbytes: int, like: torch.Tensor) -> torch.Tensor:
    return torch.empty(max(int(nbytes), 256), dtype=torch.uint8, device=like.device)


def _scratch(name: str, like: torch.Tensor, *shape, contrib: bool = False) -> torch.Tensor:
    """A fresh scratch workspace of ``name(*shape)`` bytes (``name``: the *_workspace_bytes companion of the entry) on like's device."""
    return _ws(getattr(contrib_lib() if contrib else lib(), name)(*shape), like)


def _ws_bytes(fn_name: str, *shape) -> int:
    """kvp_*_workspace_bytes(shape), remembered per shape (a ctypes call per compress is measurable in the decode regime)."""
    key = (fn_name,) + shape
    n = _WS_BYTES.get(key)
    if n is None:
        if len(_WS_BYTES) > 256:
            _WS_BYTES.clear()
        n = _WS_BYTES[key] = int(getattr(lib(), fn_name)(*shape))
    return n


def _clean_ws(kind: str, shape: tuple, nbytes: int, device, stream_handle: int) -> torch.Tensor:
    """The zero-filled-once workspace of a select or a fused compress, one per (calling thread, kind of use, device, stream, call
    shape): the calls leave its histogram region clean, so it is passed with KVP_TOPK_WS_CLEAN from then on.  Two Python threads
    never share one, even on the same stream."""
    key = (threading.get_ident(), kind, device.index, stream_handle) + shape
    with _TOPK_WS_LOCK:
        ws = _TOPK_WS.get(key)
        if ws is None:
            if len(_TOPK_WS) > 64:
                _TOPK_WS.clear()
            ws = torch.zeros(max(int(nbytes), 256), dtype=torch.uint8, device=device)
            _TOPK_WS[key] = ws
    return ws


def _drop_ws(ws: torch.Tensor):
    with _TOPK_WS_LOCK:
        for key in [k for k, v in _TOPK_WS.items() if v is ws]:
            del _TOPK_WS[key]


def _fused_compress(name: str, kind: str, shape: tuple, keys: torch.Tensor, Hkv: int, n: int, order: int, run: bool, *args):
    """The second half of the fused compress wrappers: (K', V') [B,Hkv,n,D] in the keys' dtype, the clean workspace of ``shape`` (which
    is also what kvp_<kind>_compress_workspace_bytes takes), then ``name(*args, n, K', V', workspace, flags, stream)`` if ``run``."""
    ko = torch.empty((keys.shape[0], Hkv, n, keys.shape[3]), dtype=keys.dtype, device=keys.device)
    vo = torch.empty_like(ko)
    if run:
        with _on_device(keys.device):
            st = _stream(keys)
            ws = _clean_ws(kind, shape, _ws_bytes("kvp_" + kind + "_compress_workspace_bytes", *shape), keys.device, st)
            _call(name, *args, n, _p(ko), _p(vo), _p(ws), ws.numel(), TOPK_WS_CLEAN | (int(order) & ORDER_SCORE), st, clean_ws=ws)
    return ko, vo


# ---- product wrappers, in the order of include/kvpress_hip.h --------------------------------------------------------------------------
def rownorm_score(x: torch.Tensor, scale: float) -> torch.Tensor:
    """out[b,h,s] = scale * ||x[b,h,s,:]||_2, float32 [B,H,S]."""
    x = _rows(x)
    B, H, S, D = x.shape
    ptr, *strides = _tensor(x)
    out = torch.empty((B, H, S), dtype=torch.float32, device=x.device)
    with _on_device(x.device):
        _call("kvp_rownorm_score", ptr, _DTYPES[x.dtype], B, H, S, D, *strides, float(scale), _p(out), _stream(x))
    return out


def rowdot_score(x: torch.Tensor, filt: torch.Tensor, scale: float) -> torch.Tensor:
    """out[b,h,s] = scale * <x[b,h,s,:], filt[h,:]>, float32 [B,H,S]; filt [H,D] in x's dtype (qfilter_press.py:79-82)."""
    x = _rows(x)
    B, H, S, D = x.shape
    filt = _dev(filt)
    assert tuple(filt.shape) == (H, D), (filt.shape, x.shape)
    if filt.dtype != x.dtype or filt.device != x.device:
        filt = filt.to(device=x.device, dtype=x.dtype)
    if filt.stride(-1) != 1:
        filt = filt.contiguous()
    ptr, *strides = _tensor(x)
    out = torch.empty((B, H, S), dtype=torch.float32, device=x.device)
    with _on_device(x.device):
        _call("kvp_rowdot_score", ptr, _DTYPES[x.dtype], B, H, S, D, *strides, *_tensor(filt, 1), float(scale), _p(out), _stream(x))
    return out


def snapkv_score(q_win: torch.Tensor, keys: torch.Tensor, kernel_size: int) -> torch.Tensor:
    """SnapKV scores [B,Hkv,S] float32 from RoPE'd window queries [B,Hq,W,D] and keys [B,Hkv,S,D]."""
    keys = _rows(keys)
    q_win, B, Hq, Hkv, S, W, D = _queries(q_win, keys)
    scores = torch.empty((B, Hkv, S), dtype=torch.float32, device=keys.device)
    with _on_device(keys.device):
        ws = _scratch("kvp_snapkv_workspace_bytes", keys, B, Hq, Hkv, S, W, D)
        _call("kvp_snapkv_score", *_tensor(q_win), *_tensor(keys), _DTYPES[keys.dtype], B, Hq, Hkv, S, W, D, int(kernel_size),
              _p(scores), _p(ws), ws.numel(), _stream(keys))
    return scores


def snapkv_score_rope(q_pre: torch.Tensor, cos: torch.Tensor, sin: torch.Tensor, keys: torch.Tensor,
                      kernel_size: int, _finch_normalize=None) -> torch.Tensor:
    """SnapKV scores from the PRE-RoPE window queries [B,Hq,W,D] and the window's cos/sin [1 or B, W, D]:
    the RoPE (q*cos + rotate_half(q)*sin, rounded like torch does in the model dtype) runs in the library."""
    keys = _rows(keys)
    q_pre, B, Hq, Hkv, S, W, D = _queries(q_pre, keys)
    cos, sin = _rotary(cos, sin, keys.dtype, (B, W, D))
    scores = torch.empty((B, Hkv, S), dtype=torch.float32, device=keys.device)
    with _on_device(keys.device):
        ws = _scratch("kvp_snapkv_workspace_bytes", keys, B, Hq, Hkv, S, W, D)
        name, last = (("kvp_snapkv_score_rope", int(kernel_size)) if _finch_normalize is None
                      else ("kvp_finch_score", int(_finch_normalize)))
        _call(name, *_tensor(q_pre), *_tables(cos, sin), *_tensor(keys), _DTYPES[keys.dtype], B, Hq, Hkv, S, W, D, last,
              _p(scores), _p(ws), ws.numel(), _stream(keys))
    return scores


def finch_score(q_pre: torch.Tensor, cos: torch.Tensor, sin: torch.Tensor, keys: torch.Tensor, normalize_scores: bool) -> torch.Tensor:
    """FINCH scores (finch_press.py:56-83) from the PRE-RoPE window queries [B,Hq,W,D] (any W) and the window's cos/sin."""
    return snapkv_score_rope(q_pre, cos, sin, keys, 1, _finch_normalize=bool(normalize_scores))


def snapkv_score_from_attn(attn_win: torch.Tensor, num_kv_heads: int, k_len: int, kernel_size: int) -> torch.Tensor:
    """Same from given attention weights: attn_win = attentions[..., -W:, :-W]  [B,Hq,W,S-W]."""
    attn_win = _rows(attn_win)
    B, Hq, W, Sm = attn_win.shape
    S = int(k_len)
    assert Sm == S - W, (attn_win.shape, S)
    scores = torch.empty((B, num_kv_heads, S), dtype=torch.float32, device=attn_win.device)
    with _on_device(attn_win.device):
        ws = _scratch("kvp_snapkv_workspace_bytes", attn_win, B, Hq, num_kv_heads, S, W, 1)
        _call("kvp_snapkv_score_from_attn", *_tensor(attn_win), _DTYPES[attn_win.dtype], B, Hq, num_kv_heads, S, W, int(kernel_size),
              _p(scores), _p(ws), ws.numel(), _stream(attn_win))
    return scores


def ea_qstats(q: torch.Tensor, use_covariance: bool = True):
    """mu [B,Hq,D], cov [B,Hq,D,D] (float32) of the queries q [B,Hq,Sq,D]."""
    q = _rows(q)
    B, Hq, Sq, D = q.shape
    mu = torch.empty((B, Hq, D), dtype=torch.float32, device=q.device)
    cov = torch.empty((B, Hq, D, D), dtype=torch.float32, device=q.device) if use_covariance else None
    with _on_device(q.device):
        ws = _scratch("kvp_ea_qstats_workspace_bytes", q, B, Hq, Sq, D)
        _call("kvp_ea_qstats", *_tensor(q), _DTYPES[q.dtype], B, Hq, Sq, D, _p(mu), _p(cov), _p(ws), ws.numel(), _stream(q))
    return mu, cov


def ea_score(keys: torch.Tensor, values: torch.Tensor, mu: torch.Tensor, cov: Optional[torch.Tensor], n_sink: int,
             use_vnorm: bool, epsilon: float) -> torch.Tensor:
    """ExpectedAttention scores [B,Hkv,S] float32 (post-RoPE mu/cov float32 contiguous)."""
    keys, values, B, Hkv, S, D = _kv(keys, values)
    mu = mu.to(torch.float32).contiguous()
    cov = cov.to(torch.float32).contiguous() if cov is not None else None
    Hq = mu.shape[1]
    assert mu.shape == (B, Hq, D) and (cov is None or cov.shape == (B, Hq, D, D))
    scores = torch.empty((B, Hkv, S), dtype=torch.float32, device=keys.device)
    with _on_device(keys.device):
        ws = _scratch("kvp_ea_score_workspace_bytes", keys, B, Hq, Hkv, S, D)
        _call("kvp_ea_score", *_tensor(keys), *_tensor(values), _DTYPES[keys.dtype], _p(mu), _p(cov), B, Hq, Hkv, S, D, int(n_sink),
              int(bool(use_vnorm)), float(epsilon), _p(scores), _p(ws), ws.numel(), _stream(keys))
    return scores


def topk_select(scores: torch.Tensor, k: int, order: int = ORDER_POSITION) -> torch.Tensor:
    """Indices (int32 [..., k]) of the k largest scores per row of float32 scores[..., S]; ties -> lowest position.
    ``order | TOPK_SMALLEST`` selects the k smallest instead."""
    if not scores.is_cuda:
        raise KvpressHipError(f"kvpress_amd kernels need tensors on a HIP device, got {scores.device}")
    s = scores.to(torch.float32)
    if s.stride(-1) != 1:
        s = s.contiguous()
    S = s.shape[-1]
    lead = s.shape[:-1]
    s2 = s.reshape(-1, S)  # a view whenever possible
    if s2.stride(-1) != 1 or (s2.shape[0] > 1 and s2.stride(0) < S):
        s2 = s2.contiguous()
    R = s2.shape[0]
    idx = torch.empty((R, k), dtype=torch.int32, device=s.device)
    if R and k:
        with _on_device(s.device):
            st = _stream(s)
            if (int(order) & 0xFF) == ORDER_SCORE:
                # descending-score order: the select's self-cleaning region first, then the sort's tiles and samples (never read before
                # they are written)
                ws = _clean_ws("order", (R, S, int(k)), lib().kvp_topk_order_workspace_bytes(R, S, k), s.device, st)
            else:
                # the layout (hence the clean region) depends on R and S only
                ws = _clean_ws("topk", (R, S), lib().kvp_topk_workspace_bytes(R, S, k), s.device, st)
            _call("kvp_topk_select", _p(s2), R, S, s2.stride(0) if R > 1 else S, int(k), int(order) | TOPK_WS_CLEAN, _p(idx),
                  _p(ws), ws.numel(), st, clean_ws=ws)
    return idx.reshape(*lead, k)


def _gather(name: str, keys: torch.Tensor, values: torch.Tensor, idx: torch.Tensor, *extra):
    keys, values, B, H, S, D = _kv(keys, values)
    idx = idx.to(torch.int32).contiguous()
    n = idx.shape[-1]
    assert idx.shape == (B, H, n)
    ko = torch.empty((B, H, n, D), dtype=keys.dtype, device=keys.device)
    vo = torch.empty((B, H, n, D), dtype=values.dtype, device=values.device)
    if B * H * n:
        with _on_device(keys.device):
            _call(name, *_tensor(keys), *_tensor(values), _DTYPES[keys.dtype], B, H, S, D, _p(idx), n, *extra, _p(ko), _p(vo), _stream(keys))
    return ko, vo


def gather_kv(keys: torch.Tensor, values: torch.Tensor, idx: torch.Tensor):
    """K'[b,h,j] = K[b,h,idx[b,h,j]] (and V'), contiguous [B,H,n,D] in the input dtype."""
    return _gather("kvp_gather_kv", keys, values, idx)


def scores_fill_at_(scores: torch.Tensor, idx: torch.Tensor, value: float) -> torch.Tensor:
    """In place: scores[..., idx[..., j]] = value (float32 scores [..., S] contiguous, int32 idx [..., n])."""
    assert scores.dtype == torch.float32 and scores.is_contiguous() and scores.is_cuda
    S = scores.shape[-1]
    idx = idx.to(torch.int32).contiguous()
    n = idx.shape[-1]
    R = scores.numel() // S if S else 0
    assert idx.numel() == R * n
    with _on_device(scores.device):
        _call("kvp_scores_fill_at", _p(scores), R, S, S, _p(idx), n, float(value), _stream(scores))
    return scores


def topk_select_segmented(scores: torch.Tensor, seg_len: int, k: int, pos_base: int = 0) -> torch.Tensor:
    """Per-chunk top-k: scores float32 [..., nseg * seg_len]; returns int32 [..., nseg * k] row positions (+ pos_base),
    chunk after chunk (ascending)."""
    if not scores.is_cuda:
        raise KvpressHipError(f"kvpress_amd kernels need tensors on a HIP device, got {scores.device}")
    s = scores.to(torch.float32).contiguous()
    L = s.shape[-1]
    assert L % seg_len == 0, (L, seg_len)
    nseg = L // seg_len
    lead = s.shape[:-1]
    s2 = s.reshape(-1, L)
    R = s2.shape[0]
    idx = torch.empty((R, nseg * k), dtype=torch.int32, device=s.device)
    if R and k:
        with _on_device(s.device):
            st = _stream(s)
            # chunks of up to 32768 scores are selected by one workgroup each (topk_row_kernel): no workspace at all.  (Round 6: a fresh
            # zero-filled 33 MB workspace per call was 11 us of ChunkPress's 128k step -- profiles/r06_rocprofv3_kernel_stats_chunk_snapkv128k.csv)
            ws = None if seg_len <= 32768 else _clean_ws(
                "seg", (R, nseg, int(seg_len)), lib().kvp_topk_segmented_workspace_bytes(R, nseg, seg_len, k), s.device, st)
            _call("kvp_topk_select_segmented", _p(s2), R, nseg, int(seg_len), int(k), int(pos_base), TOPK_WS_CLEAN if ws is not None else 0,
                  _p(idx), _p(ws), ws.numel() if ws is not None else 0, st, clean_ws=ws)
    return idx.reshape(*lead, nseg * k)


def rerotate_keys_(keys_kept: torch.Tensor, idx: torch.Tensor, inv_freq: torch.Tensor) -> torch.Tensor:
    """In place: re-rotate gathered keys [B,H,n,D] (kept at ascending positions idx [B,H,n]) to positions 0..n-1."""
    _dev(keys_kept)
    assert keys_kept.is_contiguous()
    B, H, n, D = keys_kept.shape
    idx = idx.to(torch.int32).contiguous()
    assert idx.shape == (B, H, n)
    inv = inv_freq.to(device=keys_kept.device, dtype=torch.float32).contiguous()
    assert inv.numel() == D // 2
    with _on_device(keys_kept.device):
        _call("kvp_rerotate_keys", _p(keys_kept), _DTYPES[keys_kept.dtype], B, H, n, D, _p(idx), _p(inv), _stream(keys_kept))
    return keys_kept


def gather_kv_rerotate(keys: torch.Tensor, values: torch.Tensor, idx: torch.Tensor, inv_freq: torch.Tensor):
    """gather_kv + rerotate_keys_ in one pass: K'[b,h,j] = K[b,h,idx[b,h,j]] re-rotated from position idx[b,h,j] to position j, V' the
    plain gather (same bits as the two calls)."""
    inv = inv_freq.to(device=keys.device, dtype=torch.float32).contiguous()
    assert inv.numel() == keys.shape[3] // 2
    return _gather("kvp_gather_kv_rerotate", keys, values, idx, _p(inv))


def knorm_compress(keys: torch.Tensor, values: torch.Tensor, n_kept: int, order: int = ORDER_POSITION):
    """KnormPress.compress in one library call: (K', V') contiguous [B,H,n_kept,D]; order = ORDER_SCORE stores the rows in descending
    score order (the reference's layout)."""
    keys, values, B, H, S, D = _kv(keys, values)
    n = int(n_kept)
    return _fused_compress("kvp_knorm_compress", "knorm", (B, H, S, n), keys, H, n, order, bool(n and B and H),
                           *_tensor(keys), *_tensor(values), _DTYPES[keys.dtype], B, H, S, D)


def snapkv_compress_rope(q_pre: torch.Tensor, cos: torch.Tensor, sin: torch.Tensor, keys: torch.Tensor, values: torch.Tensor,
                         kernel_size: int, n_kept: int, order: int = ORDER_POSITION):
    """SnapKVPress.compress (attentions=None) in one library call from the pre-RoPE window queries; order = ORDER_SCORE stores the rows
    in descending score order (window tokens first: the reference's layout)."""
    keys, values, _, _, _, _ = _kv(keys, values)
    q_pre, B, Hq, Hkv, S, W, D = _queries(q_pre, keys)
    cos, sin = _rotary(cos, sin, keys.dtype, (B, W, D))
    n = int(n_kept)
    return _fused_compress("kvp_snapkv_compress_rope", "snapkv", (B, Hq, Hkv, S, W, D, n), keys, Hkv, n, order, bool(n),
                           *_tensor(q_pre), *_tables(cos, sin), *_tensor(keys), *_tensor(values), _DTYPES[keys.dtype],
                           B, Hq, Hkv, S, W, D, int(kernel_size))


def keydiff_score(keys: torch.Tensor) -> torch.Tensor:
    """KeyDiff scores [B,H,S] float32: -cos(k, mean of the normalised keys of the head)."""
    keys = _rows(keys)
    B, H, S, D = keys.shape
    ptr, *strides = _tensor(keys)
    scores = torch.empty((B, H, S), dtype=torch.float32, device=keys.device)
    with _on_device(keys.device):
        ws = _scratch("kvp_keydiff_workspace_bytes", keys, B, H, S, D)
        _call("kvp_keydiff_score", ptr, _DTYPES[keys.dtype], B, H, S, D, *strides, _p(scores), _p(ws), ws.numel(), _stream(keys))
    return scores


def cur_score(keys: torch.Tensor, values: torch.Tensor, leverage_type: str, local_window_size: int, num_sinks: int) -> torch.Tensor:
    """CUR leverage scores [B,H,S] float32 (local_window_size 0 = no local approximation)."""
    keys, values, B, H, S, D = _kv(keys, values, same=False)
    assert keys.dtype == values.dtype and keys.shape[:3] == values.shape[:3] and keys.shape[3] == values.shape[3]
    if leverage_type not in CUR_LEVERAGE:
        raise ValueError("Unknown leverage type: choose from 'kv_avg', 'key', 'value' or 'kv_product'")
    scores = torch.empty((B, H, S), dtype=torch.float32, device=keys.device)
    with _on_device(keys.device):
        ws = _scratch("kvp_cur_workspace_bytes", keys, B, H, S)
        _call("kvp_cur_score", *_tensor(keys), *_tensor(values), _DTYPES[keys.dtype], B, H, S, D, CUR_LEVERAGE[leverage_type],
              int(local_window_size), int(num_sinks), _p(scores), _p(ws), ws.numel(), _stream(keys))
    return scores


def scores_head_mean_(scores: torch.Tensor) -> torch.Tensor:
    """In place: every head's scores <- the mean over heads (scores float32 [B,H,S], last dim contiguous)."""
    assert scores.dtype == torch.float32 and scores.dim() == 3 and scores.stride(2) == 1
    _dev(scores)
    B, H, S = scores.shape
    ptr, *strides = _tensor(scores, 2)
    with _on_device(scores.device):
        _call("kvp_scores_head_mean", ptr, B, H, S, *strides, _stream(scores))
    return scores


def _hidden(hidden_win, wq, cos, sin, dt):
    """The window's hidden states, the q_proj weight and the rotary tables as the library's own projection takes them."""
    hidden_win = _dev(hidden_win)
    assert hidden_win.dtype == dt and wq.dtype == dt and hidden_win.stride(-1) == 1 and wq.is_contiguous()
    return (hidden_win, *_rotary(cos, sin, dt))


def _hidden_keys(hidden_win, wq, cos, sin, keys):
    """_hidden for prepared keys [B,Hkv,S,D]: the three tensors, then B, Hq, Hkv, S, W, D and the hidden size K."""
    hidden_win, cos, sin = _hidden(hidden_win, wq, cos, sin, keys.dtype)
    B, W, K = hidden_win.shape
    Bk, Hkv, S, D = keys.shape
    Hq = wq.shape[0] // D
    assert B == Bk and Hq % Hkv == 0
    return hidden_win, cos, sin, B, Hq, Hkv, S, W, D, K


def snapkv_qproj_rope(hidden_win: torch.Tensor, wq: torch.Tensor, cos: torch.Tensor, sin: torch.Tensor, head_dim: int = 128) -> torch.Tensor:
    """RoPE'd window queries [B, Hq, W, D] from hidden_states[:, -W:] and q_proj.weight (bf16 / f16, W = 64, D = 128)."""
    dt = hidden_win.dtype
    hidden_win, cos, sin = _hidden(hidden_win, wq, cos, sin, dt)
    B, W, K = hidden_win.shape
    Hq = wq.shape[0] // head_dim
    out = torch.empty((B, Hq, W, head_dim), dtype=dt, device=hidden_win.device)
    with _on_device(hidden_win.device):
        _call("kvp_snapkv_qproj_rope", *_tensor(hidden_win, 2), _p(wq), *_tables(cos, sin), _DTYPES[dt], B, Hq, W, head_dim, K,
              _p(out), _stream(hidden_win))
    return out


def snapkv_score_hidden(hidden_win: torch.Tensor, wq: torch.Tensor, cos: torch.Tensor, sin: torch.Tensor, keys: torch.Tensor,
                        kernel_size: int) -> torch.Tensor:
    """SnapKV scores [B,Hkv,S] float32 from the window's hidden states and the q_proj weight (projection + RoPE in the library)."""
    keys = _rows(keys)
    hidden_win, cos, sin, B, Hq, Hkv, S, W, D, K = _hidden_keys(hidden_win, wq, cos, sin, keys)
    scores = torch.empty((B, Hkv, S), dtype=torch.float32, device=keys.device)
    with _on_device(keys.device):
        ws = _scratch("kvp_snapkv_workspace_bytes", keys, B, Hq, Hkv, S, W, D)
        _call("kvp_snapkv_score_hidden", *_tensor(hidden_win, 2), _p(wq), K, *_tables(cos, sin), *_tensor(keys), _DTYPES[keys.dtype],
              B, Hq, Hkv, S, W, D, int(kernel_size), _p(scores), _p(ws), ws.numel(), _stream(keys))
    return scores


def snapkv_compress_hidden(hidden_win: torch.Tensor, wq: torch.Tensor, cos: torch.Tensor, sin: torch.Tensor, keys: torch.Tensor,
                           values: torch.Tensor, kernel_size: int, n_kept: int, order: int = ORDER_POSITION):
    """SnapKVPress.compress (attentions=None) in one library call from the window's hidden states (order: see snapkv_compress_rope)."""
    keys, values, _, _, _, _ = _kv(keys, values)
    hidden_win, cos, sin, B, Hq, Hkv, S, W, D, K = _hidden_keys(hidden_win, wq, cos, sin, keys)
    n = int(n_kept)
    return _fused_compress("kvp_snapkv_compress_hidden", "snapkv", (B, Hq, Hkv, S, W, D, n), keys, Hkv, n, order, bool(n),
                           *_tensor(hidden_win, 2), _p(wq), K, *_tables(cos, sin), *_tensor(keys), *_tensor(values), _DTYPES[keys.dtype],
                           B, Hq, Hkv, S, W, D, int(kernel_size))


# the Compactor family (non_causal_attention_press.py, leverage_press.py, compactor_press.py)
def ncattn_score(q_pre: torch.Tensor, cos: torch.Tensor, sin: torch.Tensor, keys: torch.Tensor, values: torch.Tensor, chunk_size: int,
                 return_raw: bool = False):
    """NonCausalAttnPress scores (non_causal_attention_press.py:95-122): z-scores [B,Hkv,S] float32 from the PRE-RoPE queries
    [B,Hq,S,D], the rotary tables of the same S positions [1 or B, S, D], keys and values [B,Hkv,S,D]; with ``return_raw`` also the
    scores before the z-score."""
    keys, values, _, Hkv, _, _ = _kv(keys, values, same=False)
    q_pre = _rows(q_pre)
    dt = keys.dtype
    if q_pre.dtype != dt:
        q_pre = q_pre.to(dt)
    if values.dtype != dt:
        values = values.to(dt)
    B, Hq, S, D = q_pre.shape
    assert keys.shape == (B, Hkv, S, D) and tuple(values.shape[:3]) == (B, Hkv, S) and values.shape[3] == D, (q_pre.shape, keys.shape, values.shape)
    if Hq % Hkv != 0:
        raise KvpressHipError(f"kvp_ncattn_score: Hq % Hkv != 0 ({Hq}, {Hkv})")
    cos, sin = _rotary(cos, sin, dt)
    assert cos.shape == sin.shape and cos.shape[-1] == D and cos.shape[-2] == S and cos.shape[0] in (1, B), (cos.shape, q_pre.shape)
    raw = torch.empty((B, Hkv, S), dtype=torch.float32, device=keys.device) if return_raw else None
    z = torch.empty((B, Hkv, S), dtype=torch.float32, device=keys.device)
    with _on_device(keys.device):
        ws = _scratch("kvp_ncattn_workspace_bytes", keys, B, Hkv, S)
        _call("kvp_ncattn_score", *_tensor(q_pre), *_tables(cos, sin), *_tensor(keys), *_tensor(values), _DTYPES[dt], B, Hq, Hkv, S, D,
              int(chunk_size), _p(raw), _p(z), _p(ws), ws.numel(), _stream(keys))
    return (z, raw) if return_raw else z


def leverage_score(keys_pre: torch.Tensor, phi: torch.Tensor, return_raw: bool = False):
    """LeverageScorePress scores (leverage_press.py:59-110): z-scores [B,H,S] float32 from the PRE-RoPE keys [B,H,S,D] and the
    Gaussian sketch phi [B,H,D,k] (drawn by the caller, leverage_press.py:68-75).  Synchronises the stream to check the Cholesky
    factorisation, as the reference does; raises KvpressHipError("... Cholesky failed after 5 tries ...") like its RuntimeError."""
    k, phi = _rows(keys_pre), _rows(phi)
    if phi.dtype != k.dtype:
        phi = phi.to(k.dtype)
    B, H, S, D = k.shape
    assert tuple(phi.shape[:3]) == (B, H, D), (phi.shape, k.shape)
    ks = phi.shape[3]
    raw = torch.empty((B, H, S), dtype=torch.float32, device=k.device) if return_raw else None
    z = torch.empty((B, H, S), dtype=torch.float32, device=k.device)
    with _on_device(k.device):
        ws = _scratch("kvp_leverage_workspace_bytes", k, B, H, S, D, ks)
        _call("kvp_leverage_score", *_tensor(k), *_tensor(phi), _DTYPES[k.dtype], B, H, S, D, ks, _p(raw), _p(z), _p(ws), ws.numel(), _stream(k))
        _call("kvp_leverage_status", _p(ws), B, H, S, D, ks, _stream(k), what="kvp_leverage_score")
    return (z, raw) if return_raw else z


def compactor_combine(z_lev: torch.Tensor, z_attn: torch.Tensor, sink_start: int, sink_end: int, blending: float) -> torch.Tensor:
    """blending * z_lev + z_attn, padded with sink_start / sink_end positions holding the global max (compactor_press.py:119-122)."""
    z_lev = _dev(z_lev).contiguous()
    z_attn = _dev(z_attn).contiguous()
    assert z_lev.shape == z_attn.shape and z_lev.dtype == torch.float32 and z_attn.dtype == torch.float32, (z_lev.shape, z_attn.shape)
    B, H, Si = z_lev.shape
    out = torch.empty((B, H, Si + sink_start + sink_end), dtype=torch.float32, device=z_lev.device)
    with _on_device(z_lev.device):
        ws = _scratch("kvp_compactor_combine_workspace_bytes", z_lev)
        _call("kvp_compactor_combine", _p(z_lev), _p(z_attn), B, H, Si, int(sink_start), int(sink_end), float(blending), _p(out), _p(ws),
              ws.numel(), _stream(z_lev))
    return out


# MergingPress (merging_press.py:99-177)
def merge_values_(keys: torch.Tensor, values: torch.Tensor, kept_idx: torch.Tensor, k_out: torch.Tensor, v_out: torch.Tensor,
                  threshold: float, fraction: float, target: Optional[torch.Tensor] = None, max_sim: Optional[torch.Tensor] = None):
    """MergingPress.merge after the select and the gather: folds every evicted token's value (keys / values [B,H,S,D], evicted = not in
    the int32 kept_idx [B,H,n_kept]) into its most cosine-similar kept row, IN PLACE in v_out (the contiguous gathered V'; k_out is the
    gathered K').  ``target`` (int32) / ``max_sim`` (float32) [B,H,S-n_kept], if given, receive the argmax and its cosine.  Returns v_out."""
    keys, values, B, H, S, D = _kv(keys, values, same=False)
    dt = keys.dtype
    assert values.dtype == dt and tuple(values.shape) == (B, H, S, D), (keys.shape, values.shape)
    n = kept_idx.shape[-1]
    assert tuple(kept_idx.shape) == (B, H, n) and kept_idx.dtype == torch.int32 and kept_idx.is_contiguous(), (kept_idx.shape, kept_idx.dtype)
    for t in (k_out, v_out):
        assert t.dtype == dt and tuple(t.shape) == (B, H, n, D) and t.is_contiguous() and t.device == keys.device, (t.shape, t.dtype)
    for t, tdt in ((target, torch.int32), (max_sim, torch.float32)):
        if t is not None:
            assert t.dtype == tdt and tuple(t.shape) == (B, H, S - n) and t.is_contiguous(), (t.shape, t.dtype)
    if n == 0 or n == S:
        return v_out
    with _on_device(keys.device):
        ws = _scratch("kvp_merge_workspace_bytes", keys, B, H, S, n, D)
        _call("kvp_merge_values", *_tensor(keys), *_tensor(values), _p(kept_idx), _p(k_out), _p(v_out), _DTYPES[dt], B, H, S, n, D,
              float(threshold), float(fraction), _p(ws), ws.numel(), _p(target), _p(max_sim), _stream(keys))
    return v_out


# CAMPress (cam_press.py:124-361)
def _cam_running(running: torch.Tensor, B: int, Hkv: int, S: int, s_prev: int):
    assert running.dtype == torch.float32 and running.is_cuda and running.dim() == 3 and running.stride(2) == 1, (running.shape, running.dtype)
    assert tuple(running.shape[:2]) == (B, Hkv) and running.shape[2] >= S and 0 <= s_prev <= S, (running.shape, (B, Hkv, S), s_prev)
    return (*_tensor(running, 2), running.shape[2], int(s_prev))


def cam_attn_accumulate_(q_pre: torch.Tensor, cos: torch.Tensor, sin: torch.Tensor, keys: torch.Tensor, running: torch.Tensor,
                         s_prev: int) -> torch.Tensor:
    """In place: running[b,h,s] = (s < s_prev ? running[b,h,s] : 0) + the newest token's attention over all S keys, averaged over the
    query heads of kv head h (cam_press.py:258-283, 326-361).  q_pre: its PRE-RoPE query [B,Hq,1,D]; cos / sin: its row [1 or B, 1, D];
    keys [B,Hkv,S,D]; running: float32 [B,Hkv,cap >= S]."""
    keys = _rows(keys)
    q_pre, B, Hq, Hkv, S, W, D = _queries(q_pre, keys)
    assert W == 1, q_pre.shape
    cos, sin = _rotary(cos, sin, keys.dtype, (B, 1, D))
    with _on_device(keys.device):
        ws = _ws(_ws_bytes("kvp_cam_attn_workspace_bytes", B, Hq, Hkv, S), keys)
        _call("kvp_cam_attn_accumulate", *_tensor(q_pre), *_tables(cos, sin), *_tensor(keys), _DTYPES[keys.dtype], B, Hq, Hkv, S, D,
              *_cam_running(running, B, Hkv, S, s_prev), _p(ws), ws.numel(), _stream(keys))
    return running


def cam_attn_accumulate_row_(attn_row: torch.Tensor, running: torch.Tensor, s_prev: int) -> torch.Tensor:
    """The same from the attention row the layer returned: attn_row [B,Hq,S] (the last query row of the weights, cam_press.py:259-263)."""
    attn_row = _rows(attn_row)
    B, Hq, S = attn_row.shape
    Hkv = running.shape[1]
    with _on_device(attn_row.device):
        _call("kvp_cam_attn_accumulate_row", *_tensor(attn_row, 2), _DTYPES[attn_row.dtype], B, Hq, Hkv, S,
              *_cam_running(running, B, Hkv, S, s_prev), _stream(attn_row))
    return running


def _cam_lists(kept: torch.Tensor, cand: torch.Tensor, running: torch.Tensor, S: int):
    B, T = kept.shape
    M = cand.shape[1]
    for t in (kept, cand):
        assert t.dtype == torch.int32 and t.is_contiguous() and t.is_cuda and t.shape[0] == B, (t.shape, t.dtype)
    assert running.dtype == torch.float32 and running.dim() == 3 and running.stride(2) == 1 and running.shape[0] == B and running.shape[2] >= S
    return B, running.shape[1], T, M


def cam_merge_plan(kept: torch.Tensor, sel: torch.Tensor, running: torch.Tensor, S: int, merge_budget: int, n_cand: Optional[int] = None):
    """(cand, start int32 [B,M], prob float32 [B,H,M]) of the M merge candidates against the kept positions [B,T] and the running
    attention sum [B,H,>=S] (cam_press.py:144-183).  ``sel`` (int32, ascending) holds the candidates themselves, [B,M], or -- with
    ``n_cand = M`` -- kept and candidates together, [B,T+M]: the library then finds the candidates."""
    B, H, T, N = _cam_lists(kept, sel, running, S)
    M = N if n_cand is None else int(n_cand)
    assert N in (M, T + M), (N, T, M)
    cand = torch.empty((B, M), dtype=torch.int32, device=kept.device)
    start = torch.empty((B, M), dtype=torch.int32, device=kept.device)
    prob = torch.empty((B, H, M), dtype=torch.float32, device=kept.device)
    with _on_device(kept.device):
        _call("kvp_cam_merge_plan", _p(kept), _p(sel), N, *_tensor(running, 2), B, H, int(S), T, M, int(merge_budget), _p(cand), _p(start),
              _p(prob), _stream(kept))
    return cand, start, prob


def cam_merge_prune(keys: torch.Tensor, values: torch.Tensor, running: torch.Tensor, kept: torch.Tensor, cand: torch.Tensor,
                    start: torch.Tensor, mask: torch.Tensor, merge_budget: int):
    """(K', V' [B,H,T,D], A' float32 [B,H,T]): the gathers at the kept positions, V' with the masked candidates' values spread over
    their windows (cam_press.py:188-213).  New tensors: keys, values and running are not written."""
    keys, values, B, H, S, D = _kv(keys, values)
    Bk, Hr, T, M = _cam_lists(kept, cand, running, S)
    assert (Bk, Hr) == (B, H) and tuple(start.shape) == (B, M) and start.dtype == torch.int32 and start.is_contiguous()
    mask = mask.to(torch.float32).contiguous()
    assert tuple(mask.shape) == (B, H, M), (mask.shape, (B, H, M))
    ko = torch.empty((B, H, T, D), dtype=keys.dtype, device=keys.device)
    vo = torch.empty_like(ko)
    ao = torch.empty((B, H, T), dtype=torch.float32, device=keys.device)
    with _on_device(keys.device):
        _call("kvp_cam_merge_prune", *_tensor(keys), *_tensor(values), *_tensor(running, 2), _p(kept), _p(cand), _p(start), _p(mask),
              _DTYPES[keys.dtype], B, H, S, T, M, D, int(merge_budget), _p(ko), _p(vo), _p(ao), _stream(keys))
    return ko, vo, ao


# CriticalKVPress / CriticalAdaKVPress (criticalkv_press.py:57-92, :137-194)
def _vwl1(values: torch.Tensor, wo: torch.Tensor, num_heads: int, scores: Optional[torch.Tensor], eps: float, out: torch.Tensor):
    values = _rows(values)
    B, Hkv, S, D = values.shape
    wo = _dev(wo)
    Hq = int(num_heads)
    if Hq % Hkv != 0:
        raise KvpressHipError(f"kvp_vwl1norm_rescale: Hq % Hkv != 0 ({Hq}, {Hkv})")
    assert wo.dim() == 2 and wo.shape[1] == Hq * D, (wo.shape, Hq, D)
    if wo.dtype != values.dtype or wo.device != values.device:
        wo = wo.to(device=values.device, dtype=values.dtype)
    if wo.stride(1) != 1:
        wo = wo.contiguous()
    with _on_device(values.device):
        nws = _ws_bytes("kvp_vwl1norm_workspace_bytes", B, Hq, Hkv, S, D, wo.shape[0])   # 0 today: no allocation
        ws = _ws(nws, values) if nws else None
        _call("kvp_vwl1norm_rescale", *_tensor(values), _DTYPES[values.dtype], *_tensor(wo, 1), B, Hq, Hkv, S, D, wo.shape[0],
              _p(scores), S, float(eps), _p(out), _p(ws), nws, _stream(values))
    return out


def vwl1norm(values: torch.Tensor, wo: torch.Tensor, num_heads: int) -> torch.Tensor:
    """CriticalKVPress.vwl1norm (criticalkv_press.py:57-76): float32 [B,Hkv,S], the L1 norm of every value row [B,Hkv,S,D] pushed through
    o_proj.weight ``wo`` [hidden, num_heads * D] (a row-strided view passes through), averaged over the query heads of its kv head.
    ``wo`` is read in place when it has the values' dtype and device (a model's own cache: always); otherwise -- a float32 cache over a
    bf16 module -- the whole weight is converted and copied on EVERY call."""
    B, Hkv, S, _ = values.shape
    return _vwl1(values, wo, num_heads, None, 0.0, torch.empty((B, Hkv, S), dtype=torch.float32, device=values.device))


def vwl1norm_rescale_(scores: torch.Tensor, values: torch.Tensor, wo: torch.Tensor, num_heads: int, eps: float) -> torch.Tensor:
    """In place: scores <- (scores + eps) * vwl1norm(values, wo, num_heads) in float32, in that order (criticalkv_press.py:87);
    scores float32 [B,Hkv,S] contiguous."""
    _dev(scores), _dev(values)
    assert scores.dtype == torch.float32 and scores.is_contiguous() and tuple(scores.shape) == tuple(values.shape[:3]), (
        scores.shape, scores.dtype, values.shape)
    return _vwl1(values, wo, num_heads, scores, eps, scores)


def scores_fill_prefix_(scores: torch.Tensor, idx: torch.Tensor, counts: torch.Tensor, value: float) -> torch.Tensor:
    """In place: scores[r, idx[r, j]] = value for j < counts[r] (criticalkv_press.py:169-171, :177-179): float32 scores [..., S]
    contiguous, int32 idx [..., n] (the rows of an ORDER_SCORE select), counts one integer per row on the device."""
    _dev(scores)
    assert scores.dtype == torch.float32 and scores.is_contiguous()
    S = scores.shape[-1]
    idx = idx.to(torch.int32).contiguous()
    n = idx.shape[-1]
    R = scores.numel() // S if S else 0
    counts = counts.to(device=scores.device, dtype=torch.int32).contiguous()
    assert idx.numel() == R * n and counts.numel() == R, (idx.shape, counts.shape, scores.shape)
    with _on_device(scores.device):
        _call("kvp_scores_fill_prefix", _p(scores), R, S, S, _p(idx), n, _p(counts), float(value), _stream(scores))
    return scores


# KVzipPress (kvzip_press.py:312-354)
def kvzip_score(q_pre: torch.Tensor, cos: torch.Tensor, sin: torch.Tensor, keys: torch.Tensor, sink: int, start: int, end: int,
                row_scale: Optional[torch.Tensor] = None, col_scale: Optional[torch.Tensor] = None,
                out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """KVzip's maximum cross-attention of the chunk ``[start, end)``: float32 [B,Hkv,end-start] from the PRE-RoPE queries [B,Hq,Lq,D] of
    the repeated tokens, their cos / sin [1 or B, Lq, D] and the layer's keys [B,Hkv,S,D] as the cache holds them after that forward (the
    last Lq rows are the repeated tokens' keys; a strided view passes through).  ``row_scale`` [B,Lq] and ``col_scale`` [B,Hq,end-start]
    (non-negative) multiply the probabilities before the maximum.  ``out``: a float32 view [B,Hkv,end-start] with a contiguous last
    dim and rows ``out.stride(1)`` apart (a slice of the press's score table) that is written in place."""
    keys = _rows(keys)
    q_pre, B, Hq, Hkv, S, Lq, D = _queries(q_pre, keys)
    cos, sin = _rotary(cos, sin, keys.dtype, (B, Lq, D))
    sink, start, end = int(sink), int(start), int(end)
    n = end - start

    def scale(t, shape):
        if t is None:
            return None
        assert tuple(t.shape) == shape, (t.shape, shape)
        return _dev(t.to(device=keys.device, dtype=torch.float32)).contiguous()

    row_scale, col_scale = scale(row_scale, (B, Lq)), scale(col_scale, (B, Hq, n))
    if out is None:
        out = torch.empty((B, Hkv, max(n, 0)), dtype=torch.float32, device=keys.device)
    assert out.dtype == torch.float32 and out.device == keys.device and tuple(out.shape) == (B, Hkv, n), (out.shape, out.dtype, (B, Hkv, n))
    row_stride = out.stride(1) if Hkv > 1 else (out.stride(0) if B > 1 else n)
    assert (n <= 1 or out.stride(2) == 1) and (B == 1 or out.stride(0) == Hkv * row_stride), out.stride()
    with _on_device(keys.device):
        nws = _ws_bytes("kvp_kvzip_score_workspace_bytes", _DTYPES[keys.dtype], B, Hq, Hkv, Lq, D, sink, n)
        ws = _ws(nws, keys)
        _call("kvp_kvzip_score", *_tensor(q_pre), *_tables(cos, sin), *_tensor(keys), _DTYPES[keys.dtype], B, Hq, Hkv, S, Lq, D, sink, start, end,
              _p(row_scale), _p(col_scale), _p(out), row_stride, _p(ws), ws.numel(), _stream(keys))
    return out


def kvzap_score(hidden_states: torch.Tensor, w1: torch.Tensor, b1: torch.Tensor, w2: Optional[torch.Tensor] = None,
                b2: Optional[torch.Tensor] = None, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """KVzap's surrogate scores (kvzap_press.py:79-81): float32 [B,Hout,S] from the hidden states [B,S,K] (rows contiguous, any strides
    over B and S) and one layer of the surrogate, contiguous and in the hidden states' dtype: ``w1`` [N,K], ``b1`` [N], ``w2`` [Hout,N],
    ``b2`` [Hout] for the mlp; ``w1`` [Hout,K], ``b1`` [Hout] and no second layer for the linear model.  ``out``: a float32 [B,Hout,S]
    tensor of any strides that is written in place."""
    x = _rows(hidden_states)
    B, S, K = x.shape
    mlp = w2 is not None
    for t in (w1, b1) + ((w2, b2) if mlp else ()):
        assert t is not None and t.dtype == x.dtype and t.device == x.device and t.is_contiguous(), "surrogate weights: contiguous, in the hidden states' dtype, on their device"
    N, Hout = (w1.shape[0], w2.shape[0]) if mlp else (0, w1.shape[0])
    assert w1.shape[1] == K and b1.numel() == w1.shape[0] and (not mlp or (w2.shape[1] == N and b2.numel() == Hout)), (x.shape, w1.shape, b1.shape)
    if out is None:
        out = torch.empty((B, Hout, S), dtype=torch.float32, device=x.device)
    assert out.dtype == torch.float32 and out.device == x.device and tuple(out.shape) == (B, Hout, S), (out.shape, out.dtype, (B, Hout, S))
    with _on_device(x.device):
        ws = _ws(_ws_bytes("kvp_kvzap_score_workspace_bytes", _DTYPES[x.dtype], B, S, K, N, Hout), x)
        _call("kvp_kvzap_score", *_tensor(x, 2), _DTYPES[x.dtype], _p(w1), _p(b1), _p(w2), _p(b2), B, S, K, N, Hout, *_tensor(out),
              _p(ws), ws.numel(), _stream(x))
    return out


def threshold_select(scores: torch.Tensor, threshold: float, shift: int = 0) -> list:
    """``list(torch.where(scores < threshold))`` with ``shift`` added to the positions (dms_press.py:106-112): three int64 tensors
    (batch, head, position + shift) in row-major order for float32 scores [B,H,n] of any strides.  A NaN is not below the threshold.
    Waits for the stream once, to size the result, as torch.where does."""
    if not scores.is_cuda:
        raise KvpressHipError(f"kvpress_amd kernels need tensors on a HIP device, got {scores.device} (no CPU fallback exists)")
    assert scores.dtype == torch.float32 and scores.dim() == 3, (scores.dtype, scores.shape)
    B, H, n = scores.shape
    total = c_int64(0)
    with _on_device(scores.device):
        st = _stream(scores)
        ws = _ws(_ws_bytes("kvp_threshold_select_workspace_bytes", B, H, n), scores)
        _call("kvp_threshold_count", *_tensor(scores), B, H, n, float(threshold), _p(ws), ws.numel(), ctypes.byref(total), st)
        out = [torch.empty(total.value, dtype=torch.int64, device=scores.device) for _ in range(3)]
        if total.value:
            _call("kvp_threshold_select", *_tensor(scores), B, H, n, float(threshold), int(shift), _p(ws), ws.numel(), total.value,
                  _p(out[0]), _p(out[1]), _p(out[2]), st)
    return out


def fastkvzip_score(hidden_states: torch.Tensor, wq: torch.Tensor, bq: torch.Tensor, wk: torch.Tensor, b: torch.Tensor, gq: torch.Tensor,
                    gk: torch.Tensor, k_base: torch.Tensor, eps: float, protect_head: int = 0, protect_tail: int = 0,
                    out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """FastKVzip's gate scores (fastkvzip_press.py:54-71, :240-247): float32 [B,Hkv,S] from the hidden states [B,S,K] (rows contiguous,
    any strides over B and S) and one layer's gate: ``wq`` [Hkv*G*D,K], ``bq`` [Hkv*G*D], ``wk`` [Hkv*D,K] and ``b`` [Hkv,G] contiguous in
    the hidden states' dtype; the norm weights ``gq``, ``gk`` [D] and ``k_base`` [Hkv,J,D] contiguous float32.  The first
    ``protect_head`` and the last ``protect_tail`` positions are written as exactly 1.0.  ``out``: a float32 [B,Hkv,S] tensor of any
    strides (a layer's slice of the press's score table) that is written in place."""
    x = _rows(hidden_states)
    B, S, K = x.shape
    for t in (wq, bq, wk, b):
        assert t.dtype == x.dtype and t.device == x.device and t.is_contiguous(), "gate projections and b: contiguous, in the hidden states' dtype, on their device"
    for t in (gq, gk, k_base):
        assert t.dtype == torch.float32 and t.device == x.device and t.is_contiguous(), "norm weights and k_base: contiguous float32 on the hidden states' device"
    Hkv, G = b.shape
    D = gq.numel()
    J = k_base.shape[1]
    assert wq.shape == (Hkv * G * D, K) and bq.numel() == Hkv * G * D and wk.shape == (Hkv * D, K) and gk.numel() == D and \
        tuple(k_base.shape) == (Hkv, J, D), (x.shape, wq.shape, bq.shape, wk.shape, b.shape, gq.shape, gk.shape, k_base.shape)
    if out is None:
        out = torch.empty((B, Hkv, S), dtype=torch.float32, device=x.device)
    assert out.dtype == torch.float32 and out.device == x.device and tuple(out.shape) == (B, Hkv, S), (out.shape, out.dtype, (B, Hkv, S))
    with _on_device(x.device):
        ws = _ws(_ws_bytes("kvp_fastkvzip_score_workspace_bytes", _DTYPES[x.dtype], B, S, K, Hkv, G, D, J), x)
        _call("kvp_fastkvzip_score", *_tensor(x, 2), _DTYPES[x.dtype], _p(wq), _p(bq), _p(wk), _p(b), _p(gq), _p(gk), _p(k_base), B, S, K, Hkv, G,
              D, J, float(eps), int(protect_head), int(protect_tail), *_tensor(out), _p(ws), ws.numel(), _stream(x))
    return out


# ---- the q_proj eligibility logic ---------------------------------------------------------------------------------------------------
# The window q_proj + RoPE of the SnapKV-type presses run in the library (qproj.hip) for a plain bias-free bf16 / f16 nn.Linear
# (qproj_rope_eligible): inside bench.py's loop the step is 3-4 us shorter than with the model's own GEMM + the RoPE launch
# (round 4, two boxes, alternating runs: profiles/r04_qproj_lab.txt; rounds 1-2 had measured parity in isolation and kept it off).
# The library sums the eight k-step partials in a fixed order where the GEMM library has its own: 0.01 % of the projected values
# round to the neighbouring 16-bit number (tests/test_gpu_parity.py::test_qproj_rope_kernel_vs_torch).  KVP_LIBRARY_QPROJ=0 (or
# this attribute) keeps the model's own q_proj -- bit-identical queries to the reference's on the same GPU; quantised, LoRA-wrapped,
# biased or q_norm'ed projections always do.
USE_LIBRARY_QPROJ = os.environ.get("KVP_LIBRARY_QPROJ", "1") != "0"


def qproj_rope_supported(module, hidden_states: torch.Tensor, window: int) -> bool:
    """Should the press project the window in the library?  USE_LIBRARY_QPROJ, qproj_rope_eligible, and at most TWO batch elements: the
    kernel streams the q_proj weight once per batch element (its grid is (columns, batch); the second element's slices come from the
    L2s / memory-side cache), a GEMM over all B x 64 rows reads it once.  Measured on the cold weight (profiles/r06_qproj_batch_lab.txt):
    B = 1 22.2 us against GEMM 22.7 + RoPE launch ~5; B = 2 26.7 against 24.3 + 5; B = 4 45.2 against 23.6 + 5 -- so up to two.
    (ChunkPress hands the wrapped press its 128 chunks as a batch of 128 windows: 1239 against 195 us.)"""
    return USE_LIBRARY_QPROJ and hidden_states.shape[0] <= 2 and qproj_rope_eligible(module, hidden_states, window)


_QP_ELIGIBLE: dict = {}   # (id(module), weight data_ptr, weight version, dtype, window) -> the module-side half of the answer


def qproj_rope_eligible(module, hidden_states: torch.Tensor, window: int) -> bool:
    """True if the window's q_proj + RoPE can run in the library (qproj.hip): a plain bias-free ``nn.Linear`` q_proj in
    bf16 / f16 (not a quantised or LoRA-wrapped subclass), no per-head q_norm, window 64, head_dim 128, hidden % 256 == 0."""
    lin = module.__dict__.get("_modules", {}).get("q_proj")
    if type(lin) is torch.nn.Linear and hidden_states.is_cuda and hidden_states.stride(-1) == 1:
        w = lin._parameters.get("weight")
        if _linear_is_hooked(lin):   # (never remembered: hooks come and go)
            return False
        if type(w) in (torch.Tensor, torch.nn.Parameter):   # (the module-side checks are remembered per weight tensor: they cost more than the rest of the call's Python)
            key = (id(module), w.data_ptr(), w._version, hidden_states.dtype, window, lin._parameters.get("bias") is None,
                   "q_norm" in module.__dict__["_modules"])
            hit = _QP_ELIGIBLE.get(key)
            if hit is not None:
                return hit
            ok = _qproj_rope_eligible_slow(module, hidden_states, window)
            if len(_QP_ELIGIBLE) > 512:
                _QP_ELIGIBLE.clear()
            _QP_ELIGIBLE[key] = ok
            return ok
    return _qproj_rope_eligible_slow(module, hidden_states, window)


def _linear_is_hooked(lin) -> bool:
    """The library reads ``q_proj.weight`` directly instead of CALLING q_proj: anything that rides on the call -- forward (pre-)hooks of
    steering / tracing tools, accelerate's ``_hf_hook`` (offloading, device alignment) -- would be skipped, so such a module keeps
    the model's own call."""
    return bool(lin._forward_hooks) or bool(lin._forward_pre_hooks) or hasattr(lin, "_hf_hook")


def _qproj_rope_eligible_slow(module, hidden_states: torch.Tensor, window: int) -> bool:
    lin = getattr(module, "q_proj", None)
    if type(lin) is not torch.nn.Linear or lin.bias is not None or hasattr(module, "q_norm") or _linear_is_hooked(lin):
        return False
    w = lin.weight
    if type(w) not in (torch.Tensor, torch.nn.Parameter):   # tensor subclasses (torchao-quantised, DTensor-sharded ...) keep the nn.Linear type and
        return False                                        # report the plain dtype, but their data_ptr() is not the [out, in] matrix
    return (hidden_states.is_cuda and w.is_cuda and w.dtype == hidden_states.dtype and w.dtype in (torch.bfloat16, torch.float16)
            and w.is_contiguous() and window == 64 and getattr(module, "head_dim", 0) == 128 and w.shape[1] % 256 == 0
            and hidden_states.stride(-1) == 1 and w.shape[0] == module.config.num_attention_heads * 128)


# ---- contrib wrappers: include/kvpress_hip_extra.h, libkvpress_hip_contrib.so ----------------------------------------------------------
def observed_attention_score(attentions: torch.Tensor, num_kv_heads: int) -> torch.Tensor:
    """Average attention weight every key receives (observed_attention_press.py:42-48): attentions [B,Hq,Sq,S] -> [B,Hkv,S] float32."""
    a = _rows(attentions)
    B, Hq, Sq, S = a.shape
    assert Hq % num_kv_heads == 0, (a.shape, num_kv_heads)
    out = torch.empty((B, num_kv_heads, S), dtype=torch.float32, device=a.device)
    with _on_device(a.device):
        _call("kvp_observed_attention_score", *_tensor(a), _DTYPES[a.dtype], B, Hq, num_kv_heads, Sq, S, _p(out), _stream(a),
              contrib=True)
    return out


def lagkv_score(keys: torch.Tensor, values: torch.Tensor, n_sink: int, lag_size: int, cross_scoring: bool) -> torch.Tensor:
    """LagKV scores [B,H,S] float32 (lagkv_press.py:56-97) for S >= n_sink + 2 * lag_size."""
    keys, values, B, H, S, D = _kv(keys, values)
    out = torch.empty((B, H, S), dtype=torch.float32, device=keys.device)
    with _on_device(keys.device):
        _call("kvp_lagkv_score", *_tensor(keys), *_tensor(values), _DTYPES[keys.dtype], B, H, S, D, int(n_sink), int(lag_size),
              int(bool(cross_scoring)), _p(out), _stream(keys), contrib=True)
    return out


def think_channel_scores(q_win: torch.Tensor, keys: torch.Tensor) -> torch.Tensor:
    """ThinK's per-channel scores [B,Hkv,D] float32 (think_press.py:72-76) from the RoPE'd window queries [B,Hq,W,D] and keys."""
    keys = _rows(keys)
    q_win, B, Hq, Hkv, S, W, D = _queries(q_win, keys)
    out = torch.empty((B, Hkv, D), dtype=torch.float32, device=keys.device)
    with _on_device(keys.device):
        ws = _scratch("kvp_think_workspace_bytes", keys, B, Hkv, S, D, contrib=True)
        _call("kvp_think_channel_scores", *_tensor(q_win), *_tensor(keys), _DTYPES[keys.dtype], B, Hq, Hkv, S, W, D, _p(out), _p(ws), ws.numel(),
              _stream(keys), contrib=True)
    return out


def zero_channels_(x: torch.Tensor, idx: torch.Tensor) -> torch.Tensor:
    """x[b,h,:,idx[b,h,j]] = 0 in place (think_press.py:81-82); x [B,H,S,D] with a contiguous last dim, idx [B,H,n] int32."""
    assert x.is_cuda and x.stride(-1) == 1, "zero_channels_ works in place on a device tensor with contiguous rows"
    B, H, S, D = x.shape
    assert idx.is_cuda and idx.device == x.device and tuple(idx.shape[:2]) == (B, H), (idx.shape, x.shape)
    idx = idx.to(torch.int32).contiguous()
    with _on_device(x.device):
        _call("kvp_zero_channels", *_tensor(x), _DTYPES[x.dtype], B, H, S, D, _p(idx), idx.shape[2], _stream(x), contrib=True)
    return x


# ---- lab aids: include/kvpress_hip_lab.h (bench.py, tools/, the select's residency tests) -----------------------------------------------
def clock_probe(device=None, spin_us: int = 20) -> torch.Tensor:
    """Enqueue a shader-clock probe on the current stream; returns a 1-element float32 device tensor (MHz) that is valid
    once the stream has run it."""
    dev = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
    out = torch.zeros(1, dtype=torch.float32, device=dev)
    with _on_device(dev):
        _call("kvp_clock_probe", _p(out), int(spin_us), _stream(out))
    return out


def occupy_cus(blocks: int, threads: int, lds_bytes: int, spin_us: int, stream=None) -> None:
    """TEST AID: enqueue `blocks` workgroups that hold `threads` threads + `lds_bytes` of LDS for `spin_us` microseconds on
    `stream` (default: the current one)."""
    st = stream if stream is not None else torch.cuda.current_stream()
    _call("kvp_occupy_cus", int(blocks), int(threads), int(lds_bytes), int(spin_us), c_void_p(st.cuda_stream))


def prof_enable(on: bool) -> None:
    """Turn the library's per-kernel HIP-event timing on/off (clears previous records)."""
    _call("kvp_prof_enable", int(bool(on)))


def prof_records():
    """[(kernel name, milliseconds)] recorded since prof_enable(True); synchronises on each event."""
    out = []
    name, ms = c_char_p(), c_float()
    for i in range(lib().kvp_prof_count()):
        _call("kvp_prof_get", i, ctypes.byref(name), ctypes.byref(ms))
        out.append((name.value.decode(), float(ms.value)))
    return out


def tuning_reload() -> None:
    """Make the library re-read its KVP_* tuning variables (they are read from the environment once and cached)."""
    _call("kvp_tuning_reload")
