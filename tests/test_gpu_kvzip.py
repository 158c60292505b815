"""KVzipPress on the GPU: kvp_kvzip_score (matrix-core and generic path) against the float64 oracle (tests/_kvzip_oracle.py) on random and
on exact inputs, run-to-run reproducibility, and the press through the pipeline on the tiny Llama against the REAL reference's outputs
(tests/golden/kvzip_*.npz, oracle/gen_golden_kvzip.py).

Score contract: 1e-3 relative + 1e-6 x the row maximum.  Exact inputs: 1e-5 relative, as for the other reductions
that go through exp2 / log2 (tests/test_gpu_exact_reductions.py)."""
import functools

import numpy as np
import pytest
import torch

import _inputs
import _kvzip_inputs as KI
import _kvzip_oracle as KO
from _support import golden, tiny_pipeline, torch_dtype

pytestmark = pytest.mark.gpu
DEV = "cuda"
EXACT = 1e-5


def _rotate_half(x):
    h = x.shape[-1] // 2
    return torch.cat((-x[..., h:], x[..., :h]), dim=-1)


def _device_args(s):
    dt = torch_dtype(s["dtype"])
    q, cos, sin = (torch.from_numpy(s[n]).to(DEV, dt) for n in ("q", "cos", "sin"))
    keys = torch.from_numpy(s["keys"]).to(DEV, dt)
    if s.get("strided") is True:          # every second row of a buffer twice as long, behind an offset: strides, not a copy
        buf = torch.zeros((keys.shape[0], keys.shape[1], 2 * keys.shape[2] + 3, keys.shape[3]), device=DEV, dtype=dt)
        buf[:, :, 3::2] = keys
        keys = buf[:, :, 3::2]
    elif s.get("strided") == "unaligned":   # rows D + 1 elements apart: no 16-byte alignment
        buf = torch.zeros((*keys.shape[:3], keys.shape[3] + 1), device=DEV, dtype=dt)
        buf[..., :-1] = keys
        keys = buf[..., :-1]
    rs, cs = (None if s[n] is None else torch.from_numpy(s[n]).to(DEV) for n in ("row_scale", "col_scale"))
    return q, cos, sin, keys, s["sink"], s["start"], s["end"], rs, cs


def run_kernel(s):
    from kvpress_amd import _native

    out = _native.kvzip_score(*_device_args(s))
    torch.cuda.synchronize()
    return out.cpu().numpy()


def oracle(s):
    """the float64 oracle on the SAME rotated queries: torch's own ops on the CPU in the model dtype round q * cos + rotate_half(q) * sin
    exactly as the library does (every product and the sum to the dtype)"""
    dt = torch_dtype(s["dtype"])
    q, cos, sin = (torch.from_numpy(s[n]).to(dt) for n in ("q", "cos", "sin"))
    q_rot = q * cos.unsqueeze(1) + _rotate_half(q) * sin.unsqueeze(1)
    return KO.kvzip_score(q_rot.double().numpy(), s["keys"], s["sink"], s["start"], s["end"], s["row_scale"], s["col_scale"])


@pytest.mark.parametrize("name", list(KI.KERNEL_CASES))
def test_kernel_against_float64(name):
    s = KI.kernel_case(name)
    got, ref = run_kernel(s), oracle(s)
    assert got.shape == ref.shape and np.isfinite(got).all()
    err = KO.rel_err(got, ref)
    print(f"kvzip_score {name}: worst error {err:.3g} (contract 1e-3: relative + 1e-6 x the row maximum)")
    assert err <= 1e-3


def test_out_view_is_written_in_place_and_nothing_else():
    """the press hands over score_val[layer][..., start:end]: rows `context_length` apart; the columns outside keep their bits"""
    from kvpress_amd import _native

    s = KI.kernel_case("bf16_d128")
    args = _device_args(s)
    table = torch.full((1, 2, s["end"] + 37), -7.0, device=DEV)
    view = table[..., s["start"]:s["end"]]
    assert _native.kvzip_score(*args, out=view) is view
    ref = _native.kvzip_score(*args)
    assert torch.equal(view, ref)
    table[..., s["start"]:s["end"]] = -7.0
    assert bool((table == -7.0).all())


def test_two_runs_give_the_same_bits():
    for name in ("f16_lq300_n300", "bf16_d256", "f32_d6_generic_scales"):
        s = KI.kernel_case(name)
        a, b = run_kernel(s), run_kernel(s)
        assert a.tobytes() == b.tobytes(), name


# ---- exact inputs ------------------------------------------------------------------------------------------------------------------------
# (Hkv, G, Lq, D, sink, start, n, tail, dtype): matrix cores at one and at several owned / streamed tiles, D = 256's split rows, generic
EXACT_SHAPES = [(2, 2, 77, 128, 4, 13, 100, 37, "bf16"), (1, 2, 300, 128, 4, 13, 300, 0, "f16"), (1, 2, 129, 256, 0, 5, 130, 3, "bf16"),
                (1, 2, 300, 64, 4, 4, 100, 37, "bf16"), (2, 2, 70, 6, 4, 9, 64, 22, "f32")]
_ids = lambda p: "-".join(map(str, p))


def _rel(got, ref):
    return float(np.abs(got / ref - 1.0).max())


@pytest.mark.parametrize("shape", EXACT_SHAPES, ids=_ids)
def test_census(shape):
    """all-zero queries: every probability is a reciprocal count; the maximum over the rows is row 0's, 1 / (sink + n + 1), in EVERY column.
    A key counted twice, a dropped sink key or an off-by-one of the causal boundary moves it.  With the row scale a unit impulse at row
    t the answer is that row's 1 / (sink + n + t + 1): every row's count is checked, the rows at block, tile and split edges included."""
    Hkv, G, Lq, D, sink, start, n, tail, dtype = shape
    s, _ = KI.exact_case(*shape)
    rng = np.random.default_rng(7)
    s["keys"] = _inputs.round_to(rng.standard_normal(s["keys"].shape).astype(np.float32), dtype)   # zero queries: the keys do not matter
    got = run_kernel(s)
    err = _rel(got, 1.0 / (sink + n + 1))
    print(f"census {shape}: {err:.3g}")
    assert err <= EXACT
    for t in sorted({0, 1, 31, 32, 63, 64, 127, 128, 255, 256, Lq - 1} & set(range(Lq))):
        s["row_scale"] = np.zeros((1, Lq), np.float32)
        s["row_scale"][0, t] = 1.0
        err = _rel(run_kernel(s), 1.0 / (sink + n + t + 1))
        assert err <= EXACT, (shape, t, err)


@pytest.mark.parametrize("shape", EXACT_SHAPES, ids=_ids)
def test_heavy_key(shape):
    """one key b * e_0 under queries a * e_0: its logit is lam, every other 0.  In the chunk (first column, last column, block and tile edges)
    it takes e^lam / (sink + n + e^lam) and leaves 1 / (sink + n + e^lam) to the other columns of its kv head; among the sink keys it lowers
    every column alike; at a position no row sees, and among the repeated keys (row 0 does not see it), it must raise nothing."""
    Hkv, G, Lq, D, sink, start, n, tail, dtype = shape
    end, S = start + n, start + n + tail + Lq
    h = Hkv - 1
    uniform = 1.0 / (sink + n + 1)
    for j in sorted({0, 31, 32, 127, 128, 255, 256, n - 1} & set(range(n))):
        s, lam = KI.exact_case(*shape, heavy_key=(h, start + j))
        got, e = run_kernel(s), np.exp(lam)
        ref = np.full((1, Hkv, n), uniform)
        ref[0, h] = 1.0 / (sink + n + e)
        ref[0, h, j] = e / (sink + n + e)
        assert _rel(got, ref) <= EXACT, (shape, "column", j, _rel(got, ref))
    outside = [p for p in (sink, start - 1, end, S - Lq - 1) if sink <= p < start or end <= p < S - Lq] + [S - Lq + 1, S - 1]
    for p in outside:
        s, _ = KI.exact_case(*shape, heavy_key=(h, p))
        assert _rel(run_kernel(s), uniform) <= EXACT, (shape, "outside", p)
    if sink:
        s, lam = KI.exact_case(*shape, heavy_key=(h, sink - 1))
        ref = np.full((1, Hkv, n), uniform)
        ref[0, h] = 1.0 / (sink + n + np.exp(lam))
        assert _rel(run_kernel(s), ref) <= EXACT, (shape, "sink")


@pytest.mark.parametrize("shape", EXACT_SHAPES, ids=_ids)
def test_heavy_row(shape):
    """one query row a * e_0 (first row, last row, the rows at block, tile and row-split edges) against one key b * e_0 in the chunk: that row
    alone lifts the key's column to e^lam / (sink + n + t + e^lam); every other column keeps row 0's 1 / (sink + n + 1)."""
    Hkv, G, Lq, D, sink, start, n, tail, dtype = shape
    j0, uniform = n // 2, 1.0 / (sink + n + 1)
    for hq in (0, Hkv * G - 1):
        for t in sorted({0, 31, 32, 63, 64, 127, 128, 255, 256, Lq - 1} & set(range(Lq))):
            s, lam = KI.exact_case(*shape, heavy_key=(hq // G, start + j0), heavy_row=(hq, t))
            e = np.exp(lam)
            ref = np.full((1, Hkv, n), uniform)
            ref[0, hq // G, j0] = max(e / (sink + n + t + e), uniform)
            got = run_kernel(s)
            assert _rel(got, ref) <= EXACT, (shape, hq, t, _rel(got, ref))


# ---- the press through the pipeline against the reference's outputs --------------------------------------------------------------------
@pytest.mark.parametrize("name", list(KI.FIXTURES))
def test_press_through_the_pipeline_matches_reference(name):
    from kvpress_amd.presses.kvzip_press import KVzipPress

    spec, g = KI.FIXTURES[name], golden(name)
    pipe = tiny_pipeline(DEV, torch.float32)
    press = KVzipPress(**spec["press"])
    press.tokenizer = pipe.tokenizer
    press.prepare = functools.partial(press.prepare, chunk_size=KI.CHUNK)
    seen = {}
    compress_post = press.compress_post

    def recording_compress_post(model):
        seen["ids"] = press._context_ids.cpu().numpy()
        seen["score_val"] = press.score_val.detach().cpu().numpy()
        compress_post(model)
        seen["masked"] = [tuple(x.cpu().numpy() for x in layer.self_attn.masked_key_indices) for layer in model.model.layers]

    press.compress_post = recording_compress_post
    out = pipe(KI.context_text(spec["seed"]), question="w1 w2", press=press, max_new_tokens=4)
    assert isinstance(out["answer"], str)
    assert np.array_equal(seen["ids"], g["context_ids"])
    sv, ref = seen["score_val"], g["score_val"]
    err = KO.rel_err(sv, ref)
    print(f"{name}: score_val on the GPU vs the reference's: worst {err:.3g}")
    assert sv.dtype == np.float32 and sv.shape == ref.shape and err <= 1e-3
    L, _, H, C = ref.shape
    o = KO.compress_post(ref, spec["press"]["compression_ratio"], spec["press"].get("layerwise", False))
    for l, layer in enumerate(pipe.model.model.layers):
        b, h, p = seen["masked"][l]
        assert len(h) == int(g["n_pruned_layers"][l]) and not b.any()
        mine, theirs = h.astype(np.int64) * C + p, g[f"masked_head_{l}"].astype(np.int64) * C + g[f"masked_seq_{l}"]
        assert KO.sets_equal_outside(mine, theirs, o["bands"][l] | o["global_band"][l]), f"{name} layer {l}"
        # the answer was generated with the masks in place: they are still on the modules
        assert layer.self_attn.masked_key_indices is not None and len(layer.self_attn.masked_key_indices[1]) == len(h)
