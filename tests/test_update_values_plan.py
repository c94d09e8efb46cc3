"""CFS_HIP_FLAG_KEEP_VALUE_MAP on the host, without a GPU: the values and the value maps of the host builder
(cfs_plan.hpp) come from the positions with col <= row of the caller's array and from nowhere else -- what
include/cfs_hip.h promises ("only entries with col <= row are read"; for a mirrored shard "the lower entries
(c, i) they mirror") and what cfs_hip_sym_update_values_* pours through later.

The caller's array is rand_matrices.exact_values: an integer that depends on the POSITION at every col <= row,
NaN at every col > row.  cfs_hip_sym_plan_check_* compares bit patterns (memcmp), so NaN serves as the poison as
it stands -- no finite stand-in was needed: a stored value or a map entry taken from an upper position holds the
bits of NaN where the check expects the bits of an integer, and the check counts it."""
import numpy as np
import pytest

import cfs_spmv_amd as cfs
from cfs_spmv_amd import synth
from rand_matrices import exact_matrix, exact_values

FLAG_NO_REORDER, FLAG_CLUSTER, FLAG_HYB = 8, 16, 128
STAND_INS = [("Flan_1565", 0.05), ("ldoor", 0.1), ("pdb1HYS", 0.3)]
WHOLE = {"natural": FLAG_NO_REORDER, "clustered": FLAG_CLUSTER, "hyb": FLAG_HYB, "clustered+hyb": FLAG_CLUSTER | FLAG_HYB}
# (a mirrored shard finds the lower entry through Builder::src_at in natural order and through build_plan's
# lower_value_pos in clustered order: both orders are forced once)
SHARDS = {"mirrored": 0, "mirrored+natural": FLAG_NO_REORDER, "mirrored+clustered": FLAG_CLUSTER, "mirrored+hyb": FLAG_HYB,
          "mirrored+clustered+hyb": FLAG_CLUSTER | FLAG_HYB, "exchange": cfs.FLAG_SHARD_EXCHANGE}
DTYPES = pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])

_CACHE = {}


def _matrix(name, scale):
    if (name, scale) not in _CACHE:
        n, rp, ci, _, low = synth.generate(name, scale)
        _CACHE[name, scale] = (n, rp, ci, low)
    return _CACHE[name, scale]


def test_the_poisoned_array_is_what_it_claims():
    """NaN exactly above the diagonal; the same (min, max) pair would hold different numbers in the two triangles"""
    n, rp, ci, low = _matrix("pdb1HYS", 0.3)
    va, vb = exact_values(n, rp, ci, 1), exact_values(n, rp, ci, 2)
    rows = np.repeat(np.arange(n), np.diff(rp))
    assert np.array_equal(np.isnan(va), ci > rows) and int((ci < rows).sum()) == low
    fin = ~np.isnan(va)
    assert np.all(np.abs(va[fin]) >= 1) and np.all(np.abs(va[fin]) <= 1021) and np.array_equal(va[fin], np.rint(va[fin]))
    assert (va[fin] != vb[fin]).mean() > 0.9 and (va[fin] < 0).any() and (va[fin] > 0).any()
    assert np.array_equal(exact_values(n, rp, ci, 1, np.float32)[fin].astype(np.float64), va[fin])
    A = exact_matrix(n, rp, ci, va)
    assert (A != A.T).nnz == 0 and A.nnz == 2 * low + int((ci == rows).sum())


@DTYPES
@pytest.mark.parametrize("form", list(WHOLE))
@pytest.mark.parametrize("name,scale", STAND_INS)
def test_whole_matrix_builds_read_the_lower_triangle_only(name, scale, form, dtype):
    n, rp, ci, low = _matrix(name, scale)
    va = exact_values(n, rp, ci, 3, dtype)
    rep = cfs.plan_check(n, rp, ci, va, options=cfs.make_options(flags=WHOLE[form] | cfs.FLAG_KEEP_VALUE_MAP))
    assert rep["mismatches"] == 0, rep
    assert rep["decoded"] == rep["nnz_low"] == low
    if name == "ldoor" and form == "hyb":
        assert rep["far_entries"] > 0  # (the far sections and their map are under test)


@DTYPES
@pytest.mark.parametrize("form", list(SHARDS))
@pytest.mark.parametrize("name,scale", STAND_INS)
def test_shards_read_the_lower_triangle_only(name, scale, form, dtype):
    """3 ranks.  A mirrored shard stores the entries (i, c >= row_end) of its rows one-sided, with the value of the
    lower entry (c, i) of the rank above: the position above the diagonal in its own row holds NaN here"""
    n, rp, ci, low = _matrix(name, scale)
    va = exact_values(n, rp, ci, 4, dtype)
    rs = cfs.balanced_splits(n, rp, ci, 3)
    flags = SHARDS[form]
    tot = mirrored = 0
    for r in range(3):
        rep = cfs.plan_check(n, rp, ci, va, 3, r, rs, options=cfs.make_options(flags=flags | cfs.FLAG_KEEP_VALUE_MAP))
        assert rep["mismatches"] == 0, (r, rep)
        assert rep["decoded"] == rep["nnz_low"] + rep["mirror_entries"]
        tot += rep["nnz_low"]
        mirrored += rep["mirror_entries"]
        if form == "exchange":
            assert rep["mirror_entries"] == 0 and (rep["remote_vals"] > 0) == (r > 0)
    assert tot == low
    assert (mirrored > 0) == (form != "exchange")  # (the one-sided entries exist where they are claimed to be checked)
