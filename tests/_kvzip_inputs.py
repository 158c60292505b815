"""Seeded inputs of the KVzip tests: the kernel cases of tests/test_gpu_kvzip.py (random and exact inputs) and the tiny-Llama contexts of
the fixtures tests/golden/kvzip_*.npz (oracle/gen_golden_kvzip.py).  Test infrastructure only."""
import numpy as np

import _inputs

# ---- fixtures: the REAL reference on the tiny float32 Llama (2 layers, 2 kv heads, head_dim 6) -------------------------------------------
CHUNK = 64          # prepare(chunk_size=...): 150 context tokens = 3 chunks, the last one partial (22)
CONTEXT_TOKENS = 150
# seed of the context: the first of 17 700 tried with which the reference alone meets the band condition of oracle/gen_golden_kvzip.py (layer 1
# of the tiny model spreads its 300 scores over a few per cent: a threshold has a neighbour within 1e-3 for all but a few contexts)
FIXTURES = {
    "kvzip_global": dict(seed=17653, press=dict(compression_ratio=0.5, layerwise=False)),
    "kvzip_layerwise": dict(seed=17653, press=dict(compression_ratio=0.5, layerwise=True)),
    "kvzip_plus": dict(seed=17653, press=dict(compression_ratio=0.5, layerwise=False, kvzip_plus_normalization=True)),
}


def context_words(seed):
    """CONTEXT_TOKENS - 1 word indices: the pipeline puts the bos token in front of the context (the tokenizer has no chat template)"""
    return np.random.default_rng(1000 + seed).integers(0, len(_inputs.TINY_WORDS), CONTEXT_TOKENS - 1)


def context_text(seed):
    return " ".join(_inputs.TINY_WORDS[i] for i in context_words(seed))


def context_ids(seed):
    """int64 [1, CONTEXT_TOKENS]: what the pipeline's preprocess makes of context_text(seed) -- <s> = 1, then w_i = 3 + i"""
    return np.concatenate([[1], 3 + context_words(seed)]).astype(np.int64)[None]


# ---- kernel inputs -------------------------------------------------------------------------------------------------------------------------
def make_kernel_case(seed, B, Hkv, G, Lq, D, ctx_len, sink, start, end, dtype, scales=False, spread=1.0):
    """q_pre [B,Hq,Lq,D], cos / sin [1,Lq,D], keys [B,Hkv,ctx_len + Lq,D] rounded to `dtype` ("f32" / "f16" / "bf16"); with `scales`
    row_scale [B,Lq] and col_scale [B,Hq,end-start] (positive float32)"""
    rng = np.random.default_rng(seed)
    Hq, S = Hkv * G, ctx_len + Lq
    q = _inputs.round_to(spread * rng.standard_normal((B, Hq, Lq, D)).astype(np.float32), dtype)
    k = _inputs.round_to(rng.standard_normal((B, Hkv, S, D)).astype(np.float32), dtype)
    pos = np.arange(ctx_len, S, dtype=np.float64)[:, None]
    inv = 1.0 / (10000.0 ** (np.arange(0, D, 2, dtype=np.float64) / D))
    ang = np.concatenate([pos * inv, pos * inv], axis=-1)[None]
    cos, sin = _inputs.round_to(np.cos(ang).astype(np.float32), dtype), _inputs.round_to(np.sin(ang).astype(np.float32), dtype)
    out = dict(q=q, keys=k, cos=cos, sin=sin, sink=sink, start=start, end=end, dtype=dtype, row_scale=None, col_scale=None)
    if scales:
        out["row_scale"] = rng.uniform(0.5, 2.0, (B, Lq)).astype(np.float32)
        out["col_scale"] = rng.uniform(0.5, 2.0, (B, Hq, end - start)).astype(np.float32)
    return out


def unit_rope(Lq, D):
    """cos = 1, sin = 0: the rotation is the identity (exact-input cases place their own rows)"""
    return np.ones((1, Lq, D), np.float32), np.zeros((1, Lq, D), np.float32)


# name -> make_kernel_case arguments (B, Hkv, G, Lq, D, sink, start, n = end - start, tail = S - Lq - end, dtype, scales, strided).  The
# smallest shapes at which a path can go wrong: Lq = 77 and n = 100 are no multiple of a 32-row block; start is no multiple of any tile;
# Lq = 20 is shorter than one block, 129 one streamed tile plus 1, 300 more than one owned tile at D <= 128 (256 rows: the key splits of
# its first row tile end below the last one's, so empty splits occur); n = 300 more than one key tile; f32 / D = 6 and a key view with
# unaligned rows take the generic kernels.
def _k(B=1, Hkv=2, G=4, Lq=77, D=128, sink=4, start=13, n=100, tail=37, dtype="bf16", scales=False, strided=False):
    return dict(B=B, Hkv=Hkv, G=G, Lq=Lq, D=D, sink=sink, start=start, n=n, tail=tail, dtype=dtype, scales=scales, strided=strided)


KERNEL_CASES = {
    "bf16_d128": _k(),
    "f16_d128_scales": _k(dtype="f16", sink=0, tail=0, scales=True),
    "bf16_d128_first_chunk": _k(sink=0, start=0, scales=True),
    "f16_d128_sink_touches_chunk": _k(dtype="f16", sink=4, start=4, tail=0),
    "bf16_d64": _k(D=64, scales=True),
    "f16_d96": _k(D=96, dtype="f16"),
    "bf16_d256": _k(D=256, Hkv=1, scales=True),
    "bf16_g1": _k(G=1, tail=0),
    "f16_g16": _k(G=16, Hkv=1, dtype="f16", scales=True),
    "bf16_strided_keys": _k(strided=True),
    "bf16_lq20": _k(Lq=20),
    "bf16_lq129": _k(Lq=129, scales=True),
    "f16_lq300_n300": _k(Lq=300, n=300, dtype="f16", Hkv=1, scales=True),
    "bf16_d256_lq129_n130": _k(D=256, Lq=129, n=130, Hkv=1, G=2),
    "bf16_batch2": _k(B=2, Lq=40, n=50, scales=True),
    "f32_d6_generic": _k(D=6, G=2, dtype="f32"),
    "f32_d6_generic_scales": _k(D=6, G=2, dtype="f32", scales=True, sink=0, tail=0),
    "bf16_unaligned_rows_generic": _k(Lq=20, n=30, strided="unaligned", scales=True),
}


def kernel_case(name):
    c = KERNEL_CASES[name]
    end = c["start"] + c["n"]
    seed = sorted(KERNEL_CASES).index(name)
    s = make_kernel_case(seed, c["B"], c["Hkv"], c["G"], c["Lq"], c["D"], end + c["tail"], c["sink"], c["start"], end, c["dtype"], c["scales"])
    s["strided"] = c["strided"]
    return s


# ---- exact inputs: closed forms that do not depend on the order of any sum (tests/test_gpu_exact_reductions.py's manner) ------------------
def exact_case(Hkv, G, Lq, D, sink, start, n, tail, dtype, heavy_key=None, heavy_row=None):
    """All-zero queries and keys (the census: every probability is a reciprocal count) except: `heavy_key` (kv head, cache position): that
    key is b * e_0; `heavy_row` (query head, row): that query is a * e_0, and with heavy_key alone EVERY query is a * e_0.  The rotation is the
    identity.  a = b = 8 (exact in every dtype; lam = 5.7 at D = 128), 2 below D = 64 (lam = 1.6 at D = 6), so that e^lam stays far from
    the ends of the float32 range.  Returns the case and lam = a * b / sqrt(D), the one non-zero logit."""
    a = b = 8.0 if D >= 64 else 2.0
    Hq, end = Hkv * G, start + n
    S = end + tail + Lq
    q, k = np.zeros((1, Hq, Lq, D), np.float32), np.zeros((1, Hkv, S, D), np.float32)
    if heavy_key is not None:
        k[0, heavy_key[0], heavy_key[1], 0] = b
    if heavy_row is not None:
        q[0, heavy_row[0], heavy_row[1], 0] = a
    elif heavy_key is not None:
        q[..., 0] = a
    cos, sin = unit_rope(Lq, D)
    return dict(q=q, keys=k, cos=cos, sin=sin, sink=sink, start=start, end=end, dtype=dtype, row_scale=None, col_scale=None, strided=False), a * b / np.sqrt(D)
