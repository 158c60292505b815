"""FastKVzipPress on the GPU: kvp_fastkvzip_score (matrix-core and generic paths) against the float64 oracle and its error bound
(tests/_fastkvzip_oracle.py) on random and on exact inputs, protected positions, strides, run-to-run reproducibility, path agreement, and
the press's flow against the REAL reference's outputs (tests/golden/fastkvzip_flow_*.npz) and, on the matrix-core path, against the oracle.

Score contract: |out - float64| <= 2 bound, the bound per score from the oracle; for 16-bit cases the library must
also be no further from float64 than the reference's own gate in that dtype was (tests/golden/fastkvzip_cases.npz).  Exact inputs: the
bound without its K term."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import _fastkvzip_checks as FC
import _fastkvzip_inputs as FI
import _fastkvzip_oracle as FO
import _inputs
from _support import golden, tiny_pipeline, torch_dtype

pytestmark = pytest.mark.gpu
DEV = "cuda"
T = FI.TILE
PATH_TILE, PATH_GENERIC = 1, 3      # KVP_FASTKVZIP_PATH
GEO_ROWS512, GEO_ROWS640 = 1, 2     # KVP_FASTKVZIP_GEO


def _dev(s, strided=False):
    """(x, wq, bq, wk, b, gq, gk, kb) on the device: the first five in the case's dtype, the rest float32; strided: x is every second row
    of a longer buffer behind an offset; "unaligned": rows K + 1 elements apart"""
    dt = torch_dtype(s["dtype"])
    x, wq, bq, wk, b = (torch.from_numpy(s[n]).to(DEV, dt) for n in ("x", "wq", "bq", "wk", "b"))
    gq, gk, kb = (torch.from_numpy(s[n]).to(DEV) for n in ("gq", "gk", "kb"))
    if strided == "unaligned":
        buf = torch.zeros((*x.shape[:2], x.shape[2] + 1), device=DEV, dtype=dt)
        buf[..., :-1] = x
        x = buf[..., :-1]
    elif strided:
        buf = torch.zeros((x.shape[0] + 1, 2 * x.shape[1] + 3, x.shape[2]), device=DEV, dtype=dt)
        buf[1:, 3::2] = x
        x = buf[1:, 3::2]
        assert not x.is_contiguous()
    return x, wq, bq, wk, b, gq, gk, kb


def run_kernel(s, strided=False, out=None, head=0, tail=0, kernels=False):
    """the scores; kernels: also the names of the kernels the call launched (the library's per-kernel records)"""
    from kvpress_amd import _native

    args = _dev(s, strided)
    if kernels:
        _native.prof_enable(True)
    try:
        res = _native.fastkvzip_score(*args, s["eps"], head, tail, out=out)
        torch.cuda.synchronize()
        names = [n for n, _ in _native.prof_records()] if kernels else None
    finally:
        if kernels:
            _native.prof_enable(False)
    return (res.cpu().numpy(), names) if kernels else res.cpu().numpy()


_ORACLE = {}


def oracle(s, case):
    """(score, bound) of FI.score_case(case), computed once per module"""
    if case not in _ORACLE:
        _ORACLE[case] = FO.fastkvzip_score(*FI.oracle_args(s))
    return _ORACLE[case]


def check_against_oracle(s, got, what, ref_bound):
    ref, bound = ref_bound
    assert got.shape == ref.shape == (s["B"], s["Hkv"], s["S"]) and got.dtype == np.float32 and np.isfinite(got).all()
    ratio = FO.worst_ratio(got, ref, bound)
    print(f"fastkvzip_score {what}: worst error {ratio:.3g} of the contract 2 x bound (largest bound {bound.max():.3g}, "
          f"largest error {np.abs(got - ref).max():.3g})")
    assert ratio <= 1.0
    return ratio


@pytest.mark.parametrize("case", FI.MFMA_CASES + FI.GENERIC_CASES, ids=FI.case_id)
def test_score_against_float64(case):
    s = FI.score_case(case)
    got, names = run_kernel(s, kernels=True)
    assert names == ["fastkvzip_mfma" if case in FI.MFMA_CASES else "fastkvzip_generic"]      # no quiet change of path
    check_against_oracle(s, got, FI.case_id(case), oracle(s, case))
    if case[0] != "f32":     # never the less accurate of the two: the reference's own gate in this dtype, on the CPU
        theirs = float(golden(FI.REFERENCE_ERROR_FIXTURE)[FI.case_id(case)])
        ours = float(np.abs(got - oracle(s, case)[0]).max())
        print(f"    the reference's {case[0]} gate: {theirs:.3g} from float64; the library: {ours:.3g}")
        assert ours <= theirs


def test_empty_sequence_writes_nothing():
    from kvpress_amd import _native

    s = FI.score_case(("bf16", 2, 5, 96, 2, 2, 4))
    t = _dev(s)
    out = torch.full((2, 2, 0), -7.0, device=DEV)
    res = _native.fastkvzip_score(t[0][:, :0], *t[1:], s["eps"], 4, 2, out=out)
    torch.cuda.synchronize()
    assert res.shape == (2, 2, 0)


EXACT_CASES = [("bf16", 1, T + 1, 32, 8, 4, 16), ("f16", 1, 2 * T + 3, 96, 8, 8, 16), ("bf16", 1, T + 1, 4096, 8, 4, 16), ("bf16", 1, 2 * T + 3, 4096, 2, 2, 4),
               ("f16", 2, T + 1, 96, 8, 3, 16), ("bf16", 1, 2 * T + 3, 32, 1, 1, 16), ("f32", 1, 5, 24, 2, 2, 16), ("f32", 1, 3, 4096, 1, 2, 4)]


@pytest.mark.parametrize("case", EXACT_CASES, ids=FI.case_id)
def test_exact_inputs_no_element_lost_or_doubled(case):
    """integer x, Wq, Wk in +-{1, 2} and integer bq: every projected value is exact in any order, so the comparison runs at the bound
    WITHOUT its K term -- a lost or doubled element of a row cannot hide under it (tests/test_fastkvzip_host.py shows it would move some
    score by more than 10 x this tolerance)"""
    s = FI.exact_case(case)
    check_against_oracle(s, run_kernel(s), f"exact {FI.case_id(case)}", FO.fastkvzip_score(*FI.oracle_args(s), k_term=False))


PROTECT_CASE = ("bf16", 2, 2 * T + 3, 32, 2, 2, 16)


@pytest.mark.parametrize("tail", [0, 1, T + 1, 2 * T + 3])
@pytest.mark.parametrize("head", [0, 4, 2 * T + 10])
def test_protected_positions_are_exactly_one(head, tail):
    s = FI.score_case(PROTECT_CASE)
    S = s["S"]
    plain = run_kernel(s)
    assert not (plain == 1.0).any()
    got = run_kernel(s, head=head, tail=tail)
    prot = np.zeros(S, bool)
    prot[:min(head, S)] = True
    prot[S - min(tail, S):] = True
    assert (got[..., prot] == 1.0).all() and got[..., ~prot].tobytes() == plain[..., ~prot].tobytes()
    if head == 4 and tail == T + 1:      # the generic path fills the same positions
        s32 = FI.score_case(("f32", 2, 2 * T + 3, 24, 2, 2, 16))
        g32, p32 = run_kernel(s32, head=head, tail=tail), run_kernel(s32)
        assert (g32[..., prot] == 1.0).all() and g32[..., ~prot].tobytes() == p32[..., ~prot].tobytes()


@pytest.mark.parametrize("case", [("bf16", 2, T + 5, 96, 8, 4, 16), ("f16", 2, 5, 4096, 2, 2, 4), ("f32", 2, 33, 24, 2, 2, 16)], ids=FI.case_id)
def test_strided_inputs_and_a_table_slice_give_the_same_bits(case):
    """hidden states that are every second row of a longer buffer, and an output that is layer 1's slice of an [L, B, Hkv, S] table (and
    a transposed slice of a wider one): bit-equal to the contiguous call, and nothing outside the slice is written"""
    s = FI.score_case(case, seed=9)
    plain = run_kernel(s, head=4, tail=2)
    assert run_kernel(s, strided=True, head=4, tail=2).tobytes() == plain.tobytes()
    table = torch.full((3, s["B"], s["Hkv"], s["S"]), -7.0, device=DEV)
    assert run_kernel(s, strided=True, out=table[1], head=4, tail=2).tobytes() == plain.tobytes()
    assert bool((table[0] == -7.0).all()) and bool((table[2] == -7.0).all()) and table[1].cpu().numpy().tobytes() == plain.tobytes()
    wide = torch.full((s["B"], s["S"] + 4, s["Hkv"] + 3), -7.0, device=DEV)
    view = wide[:, 2:-2, 1:1 + s["Hkv"]].transpose(1, 2)         # [B, Hkv, S] with strides (.., 1, Hkv + 3)
    assert run_kernel(s, out=view, head=4, tail=2).tobytes() == plain.tobytes()
    wide[:, 2:-2, 1:1 + s["Hkv"]] = -7.0
    assert bool((wide == -7.0).all())


@pytest.mark.parametrize("case", [("bf16", 2, T + 5, 96, 8, 4, 16), ("f16", 1, 3, 4096, 2, 2, 4)], ids=FI.case_id)
def test_unaligned_rows_are_served_by_the_generic_kernel(case, knobs):
    """16-bit hidden states whose rows are not 16-byte aligned: the matrix-core path refuses them; same bits as the generic kernel on
    the aligned copy, inside the contract"""
    s = FI.score_case(case, seed=13)
    got = run_kernel(s, strided="unaligned")
    check_against_oracle(s, got, f"{FI.case_id(case)}, rows K + 1 elements apart", FO.fastkvzip_score(*FI.oracle_args(s)))
    knobs(KVP_FASTKVZIP_PATH=PATH_GENERIC)
    assert run_kernel(s).tobytes() == got.tobytes()


def test_two_runs_give_the_same_bits():
    for case in (("bf16", 1, 2 * T + 3, 4096, 8, 4, 16), ("f16", 2, T + 1, 96, 8, 8, 16), ("f32", 1, 65, 24, 2, 2, 16)):
        s = FI.score_case(case, seed=4)
        a, b = run_kernel(s), run_kernel(s)
        assert a.tobytes() == b.tobytes(), case


@pytest.mark.parametrize("case", [("bf16", 1, T + 1, 96, 8, 4, 16), ("f16", 2, 5, 4096, 8, 8, 16), ("bf16", 1, 2 * T + 3, 32, 1, 1, 0)], ids=FI.case_id)
def test_matrix_core_and_generic_paths_agree(case, knobs):
    """each meets the contract and they agree within 2 x bound; the scores depend neither on how the heads are grouped nor on the
    geometry of the matrix-core kernel (bit-equal: the k order of a vector's products is the same)"""
    s = FI.score_case(case, seed=21)
    ref_bound = FO.fastkvzip_score(*FI.oracle_args(s))
    got = {}
    for name, path in (("matrix-core", PATH_TILE), ("generic", PATH_GENERIC)):
        knobs(KVP_FASTKVZIP_PATH=path)
        got[name] = run_kernel(s)
        check_against_oracle(s, got[name], f"{FI.case_id(case)} forced onto the {name} path", ref_bound)
    knobs(KVP_FASTKVZIP_PATH=None)
    assert run_kernel(s).tobytes() == got["matrix-core"].tobytes()          # what such a shape takes by default
    assert got["matrix-core"].tobytes() != got["generic"].tobytes() or s["J"] == 0      # (two kernels did run)
    assert float((np.abs(got["matrix-core"].astype(np.float64) - got["generic"]) / (2.0 * ref_bound[1])).max()) <= 1.0
    knobs(KVP_FASTKVZIP_HEADS=1)
    assert run_kernel(s).tobytes() == got["matrix-core"].tobytes()
    for geo in (GEO_ROWS512, GEO_ROWS640):
        knobs(KVP_FASTKVZIP_HEADS=None, KVP_FASTKVZIP_GEO=geo)
        assert run_kernel(s).tobytes() == got["matrix-core"].tobytes(), geo


@pytest.mark.parametrize("geo", [1, 2], ids=["rows512", "rows640"])
@pytest.mark.parametrize("case", [("bf16", 1, T + 1, 4096, 8, 4, 16), ("f16", 2, 2 * T + 3, 96, 8, 8, 16), ("bf16", 2, T - 1, 32, 8, 3, 16)], ids=FI.case_id)
def test_both_geometries_against_float64(case, geo, knobs):
    """the dispatch picks a geometry by shape; here each is forced: 512 weight rows a workgroup ((8, 4): two head groups of 4, (8, 8):
    3 + 3 + 2, (8, 3): one group) and 640 rows ((8, 4): one group, (8, 8): two of 4, (8, 3): one)"""
    knobs(KVP_FASTKVZIP_GEO=geo)
    s = FI.score_case(case)
    got, names = run_kernel(s, kernels=True)
    assert names == ["fastkvzip_mfma"]
    check_against_oracle(s, got, f"{FI.case_id(case)} on geometry {geo}", oracle(s, case))


# ---- the flow ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(FI.FLOW))
def test_flow_matches_reference(name):
    """the fixtures' flow with the float32 tiny Llama on the GPU (hidden size 24: the generic path): score_val within the contract of the
    reference's, masked sets and n_pruned per layer equal; the 40-token prompt: all ones"""
    FC.check_flow_against_fixture(name, DEV)


@pytest.mark.parametrize("layerwise", [False, True])
def test_flow_on_the_matrix_core_path(layerwise):
    """synthetic bf16 hidden states (K = 64, Hkv 2, G 4) through the press's hook on stub attention modules, 2 layers of 200 tokens, then
    compress_post at a ratio whose boundaries lie in gaps of the ORACLE's scores above twice the contract bound, so the masked sets are equal"""
    from transformers import DynamicCache

    from kvpress_amd import FastKVzipPress
    from kvpress_amd.presses.fastkvzip_press import FastKVzipGate

    L, B, S, K, H, G = 2, 1, 200, 64, 2, 4
    cfg = SimpleNamespace(num_hidden_layers=L, hidden_size=K, num_key_value_heads=H, num_attention_heads=H * G, _attn_implementation="sdpa")
    gates = [g.to(DEV) for g in FI.make_gates(FastKVzipGate, 31, cfg, dtype=torch.bfloat16)]
    state = FI.gates_state(gates)
    torch.manual_seed(6)
    hidden = torch.randn(L, B, S, K).to(torch.bfloat16)
    head, tail = FO.protected_counts(S)
    ref, bmax = [], 0.0
    for l in range(L):
        sc, bound = FO.fastkvzip_score(hidden[l].double().numpy(), *FI.gate_arrays(state, l), FI.EPS)
        ref.append(FO.protect(sc, head, tail))
        bmax = max(bmax, float(bound.max()))
    ref = np.stack(ref)
    # the ratio: the first of 0.300, 0.305 .. whose selection boundaries all lie in gaps of the oracle's scores wider than that
    ratio = next((r for r in np.arange(0.3, 0.5, 0.005) if min(FO.boundary_gaps(ref, r, layerwise)) >= 2 * 2 * bmax), None)
    assert ratio is not None
    print(f"layerwise={layerwise}: ratio {ratio:.3f}, boundary gaps {['%.3g' % g for g in FO.boundary_gaps(ref, ratio, layerwise)]}, contract bound {2 * bmax:.3g}")

    press = FastKVzipPress(compression_ratio=ratio, layerwise=layerwise)
    press.gates = gates
    press._n_layers = L
    modules = [SimpleNamespace(layer_idx=l, masked_key_indices=None, config=cfg) for l in range(L)]
    cache = DynamicCache()
    for l, module in enumerate(modules):
        kv = torch.zeros(B, H, S, 8, device=DEV, dtype=torch.bfloat16)
        cache.update(kv, kv, l)
        press.forward_hook(module, [], {"hidden_states": hidden[l].to(DEV), "past_key_values": cache}, [None])
    press.compress_post(SimpleNamespace(model=SimpleNamespace(layers=[SimpleNamespace(self_attn=m) for m in modules])))
    torch.cuda.synchronize()
    sv = press.score_val.cpu().numpy()
    assert sv.dtype == np.float32 and np.array_equal(sv == 1.0, ref == 1.0)
    assert float((np.abs(sv - ref) / (2 * bmax)).max()) <= 1.0
    sets, n_pruned = FO.compress_post(ref, ratio, layerwise)
    for l, module in enumerate(modules):
        ours = tuple(t.cpu().numpy() for t in module.masked_key_indices)
        assert len(ours[0]) == n_pruned[l] and FC.triples_set(ours) == sets[l], (layerwise, l)


def test_pipeline_under_the_press():
    """one kv-press-text-generation call: an answer comes back and every layer is left with masked indices"""
    from kvpress_amd import FastKVzipPress

    pipe = tiny_pipeline(DEV, dtype=torch.float32)
    press = FastKVzipPress(compression_ratio=0.5)
    press.gates = [g.to(DEV) for g in FI.load_gates(golden("fastkvzip_flow_120_r02"), pipe.model.config)]
    res = pipe(_inputs.tiny_context(150), question="w1 w2", press=press, max_new_tokens=3)
    assert isinstance(res["answer"], str)
    n = press.score_val.shape[-1]
    total = 0
    for layer in pipe.model.model.layers:
        m = layer.self_attn.masked_key_indices
        assert m is not None and len(m) == 3 and len(m[0]) > 0 and int(m[2].max()) < n - int(n * 0.02) and int(m[2].min()) >= 4
        total += len(m[0])
    assert total == int(press.score_val.numel() * 0.5)
