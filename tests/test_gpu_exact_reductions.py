"""The long reductions on inputs for which float32 arithmetic is exact (tests/_exact_inputs.py): the kernel has to equal the float64 oracle
up to a handful of final roundings, so ONE element that is lost, counted twice or on the wrong side of a boundary sticks out -- which the
1e-3 contract on Gaussian inputs cannot see (1 / n with n in the thousands).  tests/test_exact_inputs_host.py proves on the CPU that
every such mutant of every case moves the compared outputs by at least 10 x the bound used here.

The reference is the project's oracle on the same inputs (oracle/kvpress_oracle.py, tests/_critical_oracle.py, tests/_cam_oracle.py).
Bounds: TIGHT = 1e-5 relative where the result passes through exp2 / log2 (at most 40 float32 roundings, 2.4e-6, and a 1-ulp hardware
exp2 / log2 on arguments with |log2| <= 17, 1.4e-6); bit equality with the float32-rounded oracle where it is an integer over a power of
two.  Every test prints its worst error; the figures measured on an MI355X are in DESIGN.md section 2."""
import numpy as np
import pytest
import torch

import _cam_oracle as CAMO
import _critical_oracle as CO
import _exact_inputs as X
import _inputs
from oracle import kvpress_oracle as O

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TIGHT = X.TIGHT


def native():
    from kvpress_amd import _native

    return _native


def dev(x, dtype):
    return torch.from_numpy(np.ascontiguousarray(x)).to(device=DEV, dtype=_inputs.torch_dtype(dtype))


def case_id(c):
    return "-".join(map(str, c))


def check_rel(got, want, bound, what):
    got = np.asarray(got, np.float64)
    assert got.shape == want.shape and np.isfinite(got).all(), what
    err = X.rel_err(got, want)
    assert err <= bound, f"{what}: relative error {err:.3g} > {bound:g}"
    return err


# ---- A. SnapKV / FINCH window passes -------------------------------------------------------------------------------------------------
def check_snap(got, want, W, what):
    got = got.cpu().numpy()
    err = check_rel(got[..., :-W], np.asarray(want[..., :-W], np.float64), TIGHT, what)
    assert np.all(got[..., -W:] == np.float32(got[..., :-W].max()) + np.float32(1.0)), what      # the pad columns: max + 1
    return err


def identity_tables(W, D, dtype):
    return torch.ones((1, W, D), device=DEV, dtype=_inputs.torch_dtype(dtype)), torch.zeros((1, W, D), device=DEV, dtype=_inputs.torch_dtype(dtype))


@pytest.mark.parametrize("case", X.SNAP_CENSUS, ids=case_id)
def test_snapkv_census(case, knobs):
    """q = 0: every window row is uniform over the keys it sees, every score is the pooled (1 / W) sum_w 1 / n_w.  Measured: 5.2e-7 at most."""
    W, S, G, D, ks, dtype, B, H = case
    N = native()
    q, k = X.snap_census(*case)
    qt, kt = dev(q, dtype), dev(k, dtype)
    want = O.snapkv_score(q, k, ks)
    worst = check_snap(N.snapkv_score(qt, kt, ks), want, W, f"snapkv census {case}")
    for slots in X.SNAP_SLOTS.get(X.SNAP_CENSUS.index(case), ()):
        knobs(KVP_SK_SLOTS=slots)
        worst = max(worst, check_snap(N.snapkv_score(qt, kt, ks), want, W, f"snapkv census {case} KVP_SK_SLOTS={slots}"))
        knobs(KVP_SK_SLOTS=None)
    if case in X.SNAP_FINCH:
        cos, sin = identity_tables(W, D, dtype)
        for mode in (True, False):
            got = N.finch_score(qt, cos, sin, kt, mode)
            worst = max(worst, check_snap(got, O.finch_score(q, k, mode), W, f"finch census {case} normalize_scores={mode}"))
    print(f"snapkv census {case}: worst relative error {worst:.3g}")


@pytest.mark.parametrize("case", X.SNAP_IMPULSE, ids=case_id)
def test_snapkv_impulse(case, knobs):
    """every window row alpha e_0, one key beta e_0 at t*, another t* for every (b, kv head): tile and sub-tile edges, the edges of the padded
    and the real window, and inside the window, where only the rows w >= j may see key S - W + j.  Measured: 6.5e-7 at most."""
    W, S, G, D, ks, dtype, B, H = case
    N = native()
    worst = 0.0
    all_slots = (None, 8, 64) if X.SNAP_IMPULSE.index(case) == X.SNAP_IMPULSE_LONG else (None,)
    for pos in X.groups(X.snap_impulse_positions(W, S), B * H):
        q, k = X.snap_impulse(W, S, G, D, ks, dtype, np.reshape(pos, (B, H)))
        qt, kt, want = dev(q, dtype), dev(k, dtype), O.snapkv_score(q, k, ks)
        for slots in all_slots:
            knobs(KVP_SK_SLOTS=slots)
            worst = max(worst, check_snap(N.snapkv_score(qt, kt, ks), want, W, f"snapkv impulse {case} t* = {pos} KVP_SK_SLOTS={slots}"))
    print(f"snapkv impulse {case}: worst relative error {worst:.3g}")


# ---- B. ExpectedAttention ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", X.EA_QSTATS, ids=case_id)
def test_ea_qstats_exact(case):
    """integers in [-2, 3] (every raw moment of a chunk an integer below 2^24) and, at the first and last rows of the k-steps, tiles, chunks
    and of the ragged tail, +64 / -64 on a pair of dimensions in different strips.  Measured: mu 1.6e-7; covariance 1.5e-7 on the matrix cores, 8.6e-6 in the
    generic kernel at Sq = 257 (it accumulates CENTRED products, which are not exact: Sq float32 roundings next to a 4096-sized term)."""
    dtype, D, B, Hq, Sq, layout, rows = case
    N = native()
    q, _ = X.ea_qstats_inputs(*case)
    mu_w, cov_w = O.ea_query_stats(q, True)
    qt = dev(q.transpose(0, 2, 1, 3), dtype).transpose(1, 2) if layout == "q_proj" else dev(q, dtype)
    assert (qt.stride(1) == D) == (layout == "q_proj")
    mu, cov = N.ea_qstats(qt, True)
    e_mu, e_cov = X.ea_qstats_errors(mu.cpu().numpy().astype(np.float64), cov.cpu().numpy().astype(np.float64), mu_w, cov_w)
    mu2, cov2 = N.ea_qstats(qt, False)
    e_mu2 = float(np.abs(mu2.cpu().numpy() - mu_w).max() / np.abs(mu_w).max())
    print(f"ea_qstats {case}: mu {e_mu:.3g} (without covariance {e_mu2:.3g}) of max |mu|, covariance {e_cov:.3g} of sqrt(cov_ii cov_jj)")
    assert e_mu <= TIGHT and e_cov <= TIGHT and cov2 is None and e_mu2 <= TIGHT


def check_ea(got, want, ns, what):
    got = got.cpu().numpy()
    err = check_rel(got[..., ns:], np.asarray(want[..., ns:], np.float64), TIGHT, what)
    assert np.all(got[..., :ns] == np.float32(got[..., ns:].max()) + np.float32(1.0)), what      # the sinks: max + 1
    return err


@pytest.mark.parametrize("case", X.EA_SCORE, ids=case_id)
def test_ea_score_exact(case, knobs):
    """census: mu = 0, cov zero or None, epsilon = 0, one-hot values of norm 2^k -- every scored key gets 2^k / (S - n_sink); impulse:
    mu = alpha e_0 and one heavy key on either side of the sinks, of the 128- and 4096-key edges and at the end.  Measured: 6.1e-7 at most."""
    S, G, D, ns, dtype, B, H = case
    N = native()
    worst = 0.0
    all_fused = (None, 0) if D == 128 else (None,)
    k, v, mu = X.ea_score_census(*case)
    kt, vt, mut = dev(k, dtype), dev(v, dtype), dev(mu, "f32")
    zero_cov = torch.zeros((B, H * G, D, D), device=DEV)
    for use_vnorm in (True, False):
        want = O.ea_score(k, v, mu, None, ns, use_vnorm, 0.0)
        for fused in all_fused:
            knobs(KVP_EA_FUSED_FINALIZE=fused)
            for cov in (None, zero_cov) if use_vnorm else (None,):
                got = N.ea_score(kt, vt, mut, cov, ns, use_vnorm, 0.0)
                what = f"ea_score census {case} vnorm={use_vnorm} cov={'None' if cov is None else 0} KVP_EA_FUSED_FINALIZE={fused}"
                worst = max(worst, check_ea(got, want, ns, what))
    for pos in X.groups(X.ea_score_positions(S, ns), B * H):
        k, v, mu = X.ea_score_impulse(S, G, D, ns, dtype, np.reshape(pos, (B, H)))
        kt, vt, mut, want = dev(k, dtype), dev(v, dtype), dev(mu, "f32"), O.ea_score(k, v, mu, None, ns, True, 0.0)
        for fused in all_fused:
            knobs(KVP_EA_FUSED_FINALIZE=fused)
            got = N.ea_score(kt, vt, mut, None, ns, True, 0.0)
            worst = max(worst, check_ea(got, want, ns, f"ea_score impulse {case} t* = {pos} KVP_EA_FUSED_FINALIZE={fused}"))
    print(f"ea_score {case}: worst relative error {worst:.3g}")


# ---- C. vwl1norm ---------------------------------------------------------------------------------------------------------------------
def vwl1_run(v, wo, sc, Hq, mode, eps=1e-4):
    N = native()
    if mode == "norm":
        return N.vwl1norm(v, wo, Hq)
    if mode == "alias":
        s = sc.clone()
        out = N.vwl1norm_rescale_(s, v, wo, Hq, eps)
        assert out.data_ptr() == s.data_ptr()
        return out
    out = torch.full_like(sc, float("nan"))                     # scores_in and out apart, through the C entry itself
    B, Hkv, S, D = v.shape
    N._call("kvp_vwl1norm_rescale", *N._tensor(v), N._DTYPES[v.dtype], *N._tensor(wo, 1), B, Hq, Hkv, S, D, wo.shape[0],
            sc.data_ptr(), S, float(eps), out.data_ptr(), None, 0, N._stream(v))
    return out


def ulps(a, b):
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    return int(np.abs(a.view(np.int32).astype(np.int64) - b.view(np.int32).astype(np.int64)).max())


@pytest.mark.parametrize("D", [64, 96, 128, 256, 16])
def test_vwl1norm_census(D):
    """v and wo integers in [-2, 2]: every dot product and abs-sum an integer below 2^24.  The norm has the bits of the float32-rounded
    oracle (G = 3: within 1 ulp), the rescale those of float32 (sc + eps) * norm.  hidden from 1 to 328 on either side of the 32-row sub-tile
    and of the 64- / 128-row tile; D = 16: the generic kernel.  Measured: 0 ulps everywhere."""
    cases = X.VWL1_GENERIC if D == 16 else [c + (D,) for c in X.vwl1_census_cases(D)]
    worst = 0
    for hidden, G, dtype, _ in cases:
        v, wo, sc = X.vwl1_census(hidden, G, dtype, D)
        want = CO.vwl1norm(v, wo, X.VWL1_HKV * G).astype(np.float32)
        vt, wt, st = dev(v, dtype), dev(wo, dtype), dev(sc, "f32")
        norm = vwl1_run(vt, wt, st, X.VWL1_HKV * G, "norm").cpu().numpy()
        what = f"vwl1norm census hidden={hidden} G={G} {dtype} D={D}"
        u = ulps(norm, want)
        worst = max(worst, u)
        assert u <= (1 if G == 3 else 0), f"{what}: norm {u} ulps from the oracle"
        for mode in ("rescale", "alias"):                       # from the kernel's own norm: the rescale itself must be exact
            got = vwl1_run(vt, wt, st, X.VWL1_HKV * G, mode).cpu().numpy()
            assert np.array_equal(got.view(np.int32), X.vwl1_rescale_expected(sc, norm, 1e-4).view(np.int32)), f"{what} {mode}"
    print(f"vwl1norm census D={D}: {len(cases)} shapes, norm at most {worst} ulps from the float32-rounded oracle, rescale bit-exact")


@pytest.mark.parametrize("case", X.VWL1_IMPULSE, ids=case_id)
def test_vwl1norm_impulse(case):
    """wo zero except one power of two in each of the rows 0, 31, 32, WT - 1, WT, hidden - 2, hidden - 1 (rows past hidden are requested
    clamped to the last one: an unmasked tail would count it again).  Measured: 1.0e-7 at most."""
    hidden, G, dtype, D = case
    v, wo, _ = X.vwl1_impulse(*case)
    want = CO.vwl1norm(v, wo, X.VWL1_HKV * G)
    got = native().vwl1norm(dev(v, dtype), dev(wo, dtype), X.VWL1_HKV * G).cpu().numpy()
    err = check_rel(got, want, 1e-6, f"vwl1norm impulse {case}")
    print(f"vwl1norm impulse {case}: worst relative error {err:.3g}")


# ---- D. CAM step attention -----------------------------------------------------------------------------------------------------------
def cam_step(q, cos, sin, k, dtype, prev, s_prev, S):
    """the step on a running sum whose stale tail (from s_prev on) is NaN; checks that nothing beyond S is written"""
    running = torch.from_numpy(prev.copy()).to(DEV)
    running[..., s_prev:] = float("nan")
    r0 = running.clone()
    native().cam_attn_accumulate_(dev(q, dtype), dev(cos, dtype), dev(sin, dtype), dev(k, dtype), running, s_prev)
    torch.cuda.synchronize()
    assert torch.equal(running[..., S:].view(torch.int32), r0[..., S:].view(torch.int32))
    return running.cpu().numpy()[..., :S]


@pytest.mark.parametrize("case", X.CAM_CASES, ids=case_id)
def test_cam_attn_exact(case):
    """identity rotary table (one case also with cos = 0, sin = 1, a signed permutation).  Census: q = 0, running[:S] = prev[:s_prev] + 1 / S.
    Impulse: one heavy key at the first and last key of a 256-key block, of a pass-1 chunk (cam_chunk: 64 or 128 keys here, not 1024), of
    the last chunk and of the row.  Measured: 5.9e-7 at most."""
    S, G, D, dtype, B, H = case
    chunk = X.cam_chunk(B * H, S)
    prev = X.cam_prev(B, H, S + 37)
    worst = 0.0
    cos, sin = X.cam_rotary(D)
    q, k = X.cam_census(*case)
    a = CAMO.attention_row(CAMO.rope_last_query(q, cos[0], sin[0], dtype), k, H)
    for s_prev in (0, S - 3):
        got = cam_step(q, cos, sin, k, dtype, prev, s_prev, S)
        worst = max(worst, check_rel(got, CAMO.accumulate(prev, s_prev, a), TIGHT, f"cam census {case} s_prev={s_prev}"))
    for swap in (False, True) if case == X.CAM_SWAP else (False,):
        cos, sin = X.cam_rotary(D, swap)
        for pos in X.groups(X.cam_positions(S, chunk), B * H):
            q, k = X.cam_impulse(S, G, D, dtype, np.reshape(pos, (B, H)), swap)
            a = CAMO.attention_row(CAMO.rope_last_query(q, cos[0], sin[0], dtype), k, H)
            assert a.max() > 1.0 / S                                # the heavy key is on the dimension the rotated query lands on
            got = cam_step(q, cos, sin, k, dtype, prev, 0, S)
            worst = max(worst, check_rel(got, CAMO.accumulate(prev, 0, a), TIGHT, f"cam impulse {case} swap={swap} t* = {pos}"))
    print(f"cam_attn_accumulate {case}: chunk {chunk}, worst relative error {worst:.3g}")
