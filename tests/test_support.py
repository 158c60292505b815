"""tests/_support.py itself: the shared tolerances pinned numerically (an edit of the one definition has to be deliberate), kept positions
recovered from K', the dtype names and the fixture loader."""
import numpy as np
import pytest
import torch

from _support import ULP, dtype_name, golden, golden_path, kept_positions, merged_tol, ref_tol, torch_dtype

REF = np.array([0.0, 2.0 ** -20, 1.0, -3.5])
# merged_tol: float32 64 ulps relative + 1e-7; 16-bit one ulp of max(|ref|, 2^-14), times 1.0001
MERGED = {
    "f32": [1e-7, 2.0 ** -37 + 1e-7, 2.0 ** -17 + 1e-7, 3.5 * 2.0 ** -17 + 1e-7],
    "f16": [2.0 ** -24 * 1.0001, 2.0 ** -24 * 1.0001, 2.0 ** -10 * 1.0001, 3.5 * 2.0 ** -10 * 1.0001],
    "bf16": [2.0 ** -21 * 1.0001, 2.0 ** -21 * 1.0001, 2.0 ** -7 * 1.0001, 3.5 * 2.0 ** -7 * 1.0001],
}


@pytest.mark.parametrize("dt", ["f32", "f16", "bf16"])
def test_tolerances_are_pinned(dt):
    assert ULP == {"f32": 2.0 ** -23, "f16": 2.0 ** -10, "bf16": 2.0 ** -7}
    np.testing.assert_allclose(merged_tol(REF, dt), MERGED[dt], rtol=1e-13, atol=0)
    # ref_tol: + 2e-6 * max(1, max |ref|) = 7e-6 here, 2e-6 for values below 1, and an empty array has maximum 0
    np.testing.assert_allclose(ref_tol(REF, dt), np.array(MERGED[dt]) + 7e-6, rtol=1e-13, atol=0)
    np.testing.assert_allclose(ref_tol(REF[:2], dt), np.array(MERGED[dt][:2]) + 2e-6, rtol=1e-13, atol=0)
    assert ref_tol(np.zeros((1, 2, 0, 4)), dt).shape == (1, 2, 0, 4)


def _cache():
    return np.random.RandomState(0).standard_normal((1, 2, 7, 4)).astype(np.float32)


def test_kept_positions_returns_the_permutation():
    keys = _cache()
    perm = np.stack([np.random.RandomState(h + 1).permutation(7)[:5] for h in range(2)])[None]       # [1,2,5], unsorted
    k_out = np.take_along_axis(keys, perm[..., None].repeat(4, -1), 2)
    pos = kept_positions(k_out, keys)
    assert pos.dtype == np.int64 and np.array_equal(pos, perm)
    # torch tensors, 16-bit included: the rows still match byte-wise
    kt = torch.from_numpy(keys).to(torch.bfloat16)
    assert np.array_equal(kept_positions(kt.gather(2, torch.from_numpy(perm)[..., None].expand(-1, -1, -1, 4)), kt), perm)


def test_kept_positions_rejects_rows_that_repeat_or_are_missing():
    keys = _cache()
    keys[0, 1, 5] = keys[0, 1, 2]
    with pytest.raises(AssertionError):
        kept_positions(keys[:, :, [0, 2, 3]], keys)                   # head 1: row 2 is in the cache twice
    assert np.array_equal(kept_positions(keys[:, :1, [0, 2, 3]], keys[:, :1]), [[[0, 2, 3]]])
    with pytest.raises(AssertionError):
        kept_positions(keys[:, :1, :3] + 1.0, keys[:, :1])           # rows that are not in the cache at all


def test_dtype_names_round_trip():
    for name, dt in (("f32", torch.float32), ("f16", torch.float16), ("bf16", torch.bfloat16)):
        assert torch_dtype(name) is dt and dtype_name(dt) == name == dtype_name(torch_dtype(name))
    import _inputs

    assert _inputs.torch_dtype is torch_dtype


def test_golden_loads_the_whole_fixture():
    g = golden("kn_readme")
    with np.load(golden_path("kn_readme.npz")) as f:
        assert isinstance(g, dict) and sorted(g) == sorted(f.files)
        assert all(np.array_equal(g[k], f[k]) for k in f.files)
