"""KVzapPress / DMSPress on the GPU: kvp_kvzap_score (matrix-core, few-rows, linear and generic paths) against the float64 oracle
(tests/_kvzap_oracle.py) on random and on exact inputs, strides, run-to-run reproducibility, kvp_threshold_count / _select against numpy,
and the DMS flow against the REAL reference's outputs (tests/golden/kvzap_*.npz) and, on the matrix-core path, against the oracle.

Score contract: |out - ref| <= 2 (K + N + 4) u scale, u = 2^-24, scale = |b2| + sum_j |W2_j| (|b1_j| + sum_k |x_k| |W1_jk|).
Exact inputs: 1e-5 relative, as in tests/test_gpu_exact_reductions.py."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import _kvzap_checks as ZC
import _kvzap_inputs as ZI
import _kvzap_oracle as ZO
from _support import torch_dtype

pytestmark = pytest.mark.gpu
DEV = "cuda"
EXACT = 1e-5
TILE = 128      # tokens per workgroup of the matrix-core kernel for N <= 512 (64 for N <= 1024)
PATH_TILE, PATH_ROWS, PATH_GENERIC = 1, 2, 3      # KVP_KVZAP_PATH


def _dev(s, strided=False):
    """(x, w1, b1, w2, b2) on the device in the case's dtype; strided: x is every second row of a longer buffer behind an offset"""
    dt = torch_dtype(s["dtype"])
    x, w1, b1, w2, b2 = (None if s[n] is None else torch.from_numpy(s[n]).to(DEV, dt) for n in ("x", "w1", "b1", "w2", "b2"))
    if strided == "unaligned":      # rows K + 1 elements apart: no 16-byte alignment
        buf = torch.zeros((*x.shape[:2], x.shape[2] + 1), device=DEV, dtype=dt)
        buf[..., :-1] = x
        x = buf[..., :-1]
    elif strided:
        buf = torch.zeros((x.shape[0] + 1, 2 * x.shape[1] + 3, x.shape[2]), device=DEV, dtype=dt)
        buf[1:, 3::2] = x
        x = buf[1:, 3::2]
        assert not x.is_contiguous()
    return x, w1, b1, w2, b2


def run_kernel(s, strided=False, out=None):
    from kvpress_amd import _native

    res = _native.kvzap_score(*_dev(s, strided), out=out)
    torch.cuda.synchronize()
    return res.cpu().numpy()


def check_against_oracle(s, got, what):
    ref, scale = ZO.kvzap_score(s["x"], s["w1"], s["b1"], s["w2"], s["b2"])
    assert got.shape == ref.shape == (s["B"], s["Hout"], s["S"]) and got.dtype == np.float32 and np.isfinite(got).all()
    ratio = ZO.worst_ratio(got, ref, scale, ZI.bound(s["K"], s["N"]))
    print(f"kvzap_score {what}: worst error {ratio:.3g} of the contract bound 2 (K + N + 4) u scale = {ZI.bound(s['K'], s['N']):.3g} scale")
    assert ratio <= 1.0
    return ratio


# (dtype, B, S, K, N, Hout); N = 0: the linear model.  S walks 1, 3, 16, 17, 63, 64, 65, T - 1, T, T + 1, 2 T + 3 over a thinned product of
# K in {32, 96, 4096}, N in {32, 96, 512}, Hout in {1, 2, 8}, B in {1, 2}; K = 4096 with N = 512 at S <= 2 T + 3 only
SCORE_CASES = [
    ("bf16", 1, 1, 4096, 512, 8), ("f16", 2, 3, 32, 32, 1), ("bf16", 1, 16, 96, 96, 2), ("f16", 2, 8, 4096, 512, 8),
    ("bf16", 1, 17, 4096, 512, 8), ("bf16", 2, 16, 96, 96, 2), ("f16", 2, 63, 96, 32, 2), ("bf16", 1, 64, 32, 96, 8),
    ("f16", 1, 65, 96, 512, 1), ("bf16", 1, TILE - 1, 4096, 512, 8), ("f16", 1, TILE, 4096, 512, 8), ("bf16", 2, TILE + 1, 32, 512, 2),
    ("bf16", 1, 2 * TILE + 3, 4096, 512, 8), ("f16", 2, 2 * TILE + 3, 96, 96, 1),
    # N above 512: the 64-token geometry (19 and 32 column blocks), around its own tile
    ("bf16", 1, 63, 64, 608, 2), ("f16", 1, 64, 96, 1024, 8), ("bf16", 2, 65, 32, 1024, 1), ("bf16", 1, 2 * 64 + 3, 4096, 544, 8),
    # the generic path: float32, K = 24 (the tiny Llama), N = 40
    ("f32", 1, 17, 24, 40, 2), ("f32", 2, 65, 32, 32, 8), ("bf16", 1, 65, 24, 40, 2), ("f16", 1, TILE + 1, 96, 40, 1), ("f32", 1, 1, 4096, 512, 8),
    ("bf16", 1, 3, 96, 40, 2),      # few rows, N no multiple of 32
    # the linear model
    ("bf16", 1, 1, 4096, 0, 8), ("f16", 2, 3, 96, 0, 2), ("bf16", 2, 8, 32, 0, 1), ("bf16", 1, 17, 4096, 0, 8), ("f16", 1, TILE, 32, 0, 1),
    ("bf16", 2, TILE + 1, 96, 0, 8), ("bf16", 1, 2 * TILE + 3, 4096, 0, 8), ("f16", 1, 63, 96, 0, 2), ("f32", 1, 65, 24, 0, 2), ("f32", 2, 16, 96, 0, 8),
]


@pytest.mark.parametrize("case", SCORE_CASES, ids=lambda c: "-".join(map(str, c)))
def test_score_against_float64(case):
    s = ZI.score_case(sum(case[1:]), *case[1:], case[0])
    check_against_oracle(s, run_kernel(s), str(case))


def test_empty_sequence_writes_nothing():
    from kvpress_amd import _native

    s = ZI.score_case(1, 2, 5, 96, 32, 2, "bf16")
    x, w1, b1, w2, b2 = _dev(s)
    out = _native.kvzap_score(x[:, :0], w1, b1, w2, b2)
    torch.cuda.synchronize()
    assert out.shape == (2, 2, 0)


@pytest.mark.parametrize("case", [("bf16", 2, TILE + 5, 96, 96, 2), ("f16", 2, 5, 4096, 512, 8), ("bf16", 2, 70, 96, 0, 8), ("f32", 2, 33, 24, 40, 2)],
                         ids=lambda c: "-".join(map(str, c)))
def test_strided_inputs_and_output_give_the_same_bits(case):
    """hidden states that are every second row of a longer buffer, and an output that is a transposed slice of a wider table: bit-equal
    to the contiguous call, and nothing outside the view is written"""
    s = ZI.score_case(9, *case[1:], case[0])
    plain = run_kernel(s)
    assert run_kernel(s, strided=True).tobytes() == plain.tobytes()
    table = torch.full((s["B"], s["S"] + 4, s["Hout"] + 3), -7.0, device=DEV)
    view = table[:, 2:-2, 1:1 + s["Hout"]].transpose(1, 2)         # [B, Hout, S] with strides (.., 1, Hout + 3)
    assert run_kernel(s, strided=True, out=view).tobytes() == plain.tobytes()
    table[:, 2:-2, 1:1 + s["Hout"]] = -7.0
    assert bool((table == -7.0).all())


@pytest.mark.parametrize("case", [("bf16", 2, TILE + 5, 96, 96, 2), ("f16", 1, 3, 4096, 512, 8), ("bf16", 2, 70, 96, 0, 8)], ids=lambda c: "-".join(map(str, c)))
def test_unaligned_rows_are_served_by_the_generic_kernel(case, knobs):
    """16-bit hidden states whose rows are not 16-byte aligned: the fast paths refuse them; same bits as the generic kernel on the
    aligned copy, inside the contract"""
    s = ZI.score_case(13, *case[1:], case[0])
    got = run_kernel(s, strided="unaligned")
    check_against_oracle(s, got, f"{case}, rows K + 1 elements apart")
    knobs(KVP_KVZAP_PATH=PATH_GENERIC)
    assert run_kernel(s).tobytes() == got.tobytes()


def test_two_runs_give_the_same_bits():
    for case in (("bf16", 1, 2 * TILE + 3, 4096, 512, 8), ("f16", 2, 4, 4096, 512, 8), ("bf16", 1, 1, 4096, 0, 8), ("bf16", 2, 300, 96, 0, 2),
                 ("f32", 1, 65, 24, 40, 2)):
        s = ZI.score_case(4, *case[1:], case[0])
        a, b = run_kernel(s), run_kernel(s)
        assert a.tobytes() == b.tobytes(), case


@pytest.mark.parametrize("case", [("bf16", 1, 1, 4096, 512, 8), ("f16", 2, 8, 96, 96, 2), ("bf16", 1, 16, 32, 1024, 1), ("bf16", 2, 3, 4096, 0, 8)],
                         ids=lambda c: "-".join(map(str, c)))
def test_few_rows_path_and_tile_path_agree(case, knobs):
    """up to 16 rows are served by both; each meets the contract, so they differ by at most twice the bound (and a generic run too)"""
    s = ZI.score_case(21, *case[1:], case[0])
    ref, scale = ZO.kvzap_score(s["x"], s["w1"], s["b1"], s["w2"], s["b2"])
    got = {}
    for name, path in (("few-rows", PATH_ROWS), ("tile", PATH_TILE), ("generic", PATH_GENERIC)):
        knobs(KVP_KVZAP_PATH=path)
        got[name] = run_kernel(s)
        check_against_oracle(s, got[name], f"{case} forced onto the {name} path")
    knobs(KVP_KVZAP_PATH=None)
    assert run_kernel(s).tobytes() == got["few-rows"].tobytes()          # what such a shape takes by default
    assert ZO.worst_ratio(got["tile"], got["few-rows"].astype(np.float64), scale, 2 * ZI.bound(s["K"], s["N"])) <= 1.0


# (dtype, B, S, K, N, Hout) at tile-boundary K and N: K = 32 (half a K tile), 64, 96 (one and a half), 4096; N = 32, 512, 544 (the other geometry)
EXACT_CASES = [("bf16", 1, TILE + 1, 32, 32, 2), ("f16", 2, TILE + 1, 64, 512, 8), ("bf16", 1, TILE + 1, 96, 544, 2), ("bf16", 1, 2 * TILE + 3, 4096, 512, 8),
               ("bf16", 1, 64 + 1, 4096, 1024, 8), ("f16", 2, 3, 96, 512, 8), ("bf16", 1, 1, 4096, 512, 8), ("f32", 1, 5, 24, 40, 2),
               ("bf16", 1, TILE + 1, 4096, 0, 8), ("f16", 2, 2, 4096, 0, 8), ("bf16", 1, 37, 96, 0, 1), ("f16", 1, 1, 544, 0, 2), ("f32", 1, 5, 24, 0, 2)]


@pytest.mark.parametrize("case", EXACT_CASES, ids=lambda c: "-".join(map(str, c)))
def test_exact_inputs_no_element_lost_or_doubled(case):
    """integer data, every partial sum exact: the linear model gives the exact sum, the mlp with a one-hot W2 gelu(integer) + b2; a lost
    or doubled element would move the result by at least 1 in sums of at most 4 K"""
    s = ZI.exact_case(*case[1:], case[0])
    got = run_kernel(s)
    x, w1 = s["x"].astype(np.float64), s["w1"].astype(np.float64)
    pre = np.einsum("bsk,jk->bjs", x, w1) + s["b1"][None, :, None]
    if s["N"]:
        assert pre.min() >= s["K"] - 3                                     # gelu(z) = z here
        want = pre[:, s["pick"]] + s["b2"][None, :, None]
    else:
        want = pre
    err = float((np.abs(got - want) / np.maximum(np.abs(want), 1.0)).max())
    print(f"kvzap_score exact {case}: {err:.3g} relative")
    assert 1.0 / (4 * s["K"] + 8) > 5 * EXACT                              # one element is well above the tolerance
    assert err <= EXACT


# ---- kvp_threshold_count / kvp_threshold_select -----------------------------------------------------------------------------------------
def _select(scores, threshold, shift=0):
    from kvpress_amd import _native

    out = _native.threshold_select(scores, threshold, shift)
    torch.cuda.synchronize()
    assert len(out) == 3 and all(t.dtype == torch.int64 and t.is_cuda for t in out)
    return [t.cpu().numpy() for t in out]


@pytest.mark.parametrize("rows", [(1, 1), (2, 8)], ids=["BH1", "BH16"])
@pytest.mark.parametrize("n", [1, 2, 255, 256, 257, 2047, 2048, 2049, 70001])
def test_threshold_select_matches_numpy(n, rows):
    B, H = rows
    sc = np.random.RandomState(n + B).standard_normal((B, H, n)).astype(np.float32)
    for thr, shift in ((0.0, 0), (-0.7, 123), (9.0, 0), (-9.0, 5)):         # about half, a quarter, all below, none below
        want = ZO.threshold_select(sc, thr, shift)
        got = _select(torch.from_numpy(sc).to(DEV), thr, shift)
        assert all(np.array_equal(g, w) for g, w in zip(got, want)), (n, rows, thr)     # order included
    assert len(ZO.threshold_select(sc, 9.0)[0]) == sc.size and len(ZO.threshold_select(sc, -9.0)[0]) == 0


def test_threshold_select_nan_views_and_ties():
    sc = np.random.RandomState(0).standard_normal((2, 3, 5000)).astype(np.float32)
    sc[0, 1, 7] = sc[1, 2, 4999] = np.nan                                  # a NaN compares false: kept
    sc[1, 0, 100:200] = 0.25                                               # equal to the threshold: not below it
    dev = torch.from_numpy(sc).to(DEV)
    want = ZO.threshold_select(sc, 0.25)
    assert all(np.array_equal(g, w) for g, w in zip(_select(dev, 0.25), want))
    assert not any((b, h, p) in ZO.triples_set(want) for b, h, p in ((0, 1, 7), (1, 2, 4999), (1, 0, 150)))
    # a [..., :n] view of the buffer (rows 5000 apart), as DMSPress hands it over, and a view strided in every dimension
    for n in (1, 72, 4097):
        assert all(np.array_equal(g, w) for g, w in zip(_select(dev[..., :n], 0.25, 11), ZO.threshold_select(sc[..., :n], 0.25, 11))), n
    view = dev.transpose(0, 1)[:, :, 3::2]
    assert all(np.array_equal(g, w) for g, w in zip(_select(view, -0.5), ZO.threshold_select(sc.transpose(1, 0, 2)[:, :, 3::2], -0.5)))
    assert all(len(t) == 0 for t in _select(dev[..., :0], 0.25))


# ---- the flow ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(ZI.FIXTURES))
def test_dms_flow_matches_reference(name):
    """the fixtures' flow with the float32 tiny Llama on the GPU (hidden size 24: the generic path): masked sets and ratios equal the
    reference's"""
    ZC.check_flow_against_fixture(name, DEV)


@pytest.mark.parametrize("model_type", ["mlp", "linear"])
def test_dms_flow_on_the_matrix_core_path(model_type):
    """synthetic bf16 hidden states (K = 128, N = 64) through the press's hook on a stub attention module: 200 prompt rows (matrix-core /
    linear kernel), then 5 single-row steps (few-rows path).  The threshold is the midpoint of the widest gap among the central fifth of
    the ORACLE's scores, and that half gap must exceed the contract bound -- so the sets are equal."""
    from transformers import DynamicCache

    from kvpress_amd.presses.dms_press import DMSPress
    from kvpress_amd.presses.kvzap_press import KVzapConfig, KVzapModel, KVzapPress

    B, H, K, N, S0, steps, D = 2, 2, 128, 64 if model_type == "mlp" else 0, 200, 5, 8
    torch.manual_seed(5)
    surrogate = KVzapModel(KVzapConfig(input_dim=K, output_dim=H, hidden_dim=N or None, n_modules=1)).eval()
    hidden = torch.randn(B, S0 + steps, K).to(torch.bfloat16)
    lin = [surrogate.layers[0]] if N == 0 else [surrogate.layers[0][0], surrogate.layers[0][2]]
    w = [t.detach().to(torch.bfloat16).double().numpy() for l in lin for t in (l.weight, l.bias)] + [None, None] * (N == 0)
    ref, scale = ZO.kvzap_score(hidden.double().numpy(), *w[:4])                          # [B, H, 205]
    flat = np.sort(ref.ravel())
    lo, hi = int(0.4 * flat.size), int(0.6 * flat.size)
    i = lo + int(np.argmax(np.diff(flat[lo:hi + 1])))
    thr = float(np.float32(0.5 * (flat[i] + flat[i + 1])))
    margin = float((np.abs(ref - thr) / scale).min())
    print(f"{model_type}: threshold {thr:.6g}, nearest oracle score {margin:.3g} of scale away (bound {ZI.bound(K, N):.3g})")
    assert margin >= 2 * ZI.bound(K, N)

    scorer = KVzapPress(model_type=model_type)
    scorer.kvzap_model = surrogate
    press = DMSPress(scorer, threshold=thr, decoding=True)
    module, cache, dms = SimpleNamespace(layer_idx=0, masked_key_indices=None), DynamicCache(), ZO.Dms(thr, 128)
    pos = 0
    for t, q_len in enumerate([S0] + [1] * steps):
        h = hidden[:, pos:pos + q_len].to(DEV)
        kv = torch.zeros(B, H, q_len, D, device=DEV, dtype=torch.bfloat16)
        cache.update(kv, kv, 0)
        press.forward_hook(module, [], {"hidden_states": h, "past_key_values": cache}, [None])
        dms.step(ref[..., pos:pos + q_len], prefilling=t == 0)
        pos += q_len
        torch.cuda.synchronize()
        ours = module.masked_key_indices
        assert ours is not None and ZO.triples_set(tuple(x.cpu().numpy() for x in ours)) == ZO.triples_set(dms.masked), (model_type, t)
        assert len(ours[0]) == len(dms.masked[0]) and press.compression_ratios[0] == dms.ratio
        assert press.scores_buffer[0].shape[-1] == 128 and press.scores_buffer[0].is_cuda
    assert 0.05 < dms.ratio < 0.5
