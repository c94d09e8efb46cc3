"""rand_matrices.sym_confinement_case, the matrix of tests/test_gpu_sym_confinement.py, without a GPU:
its `expect` against the numpy statement of the contract, the sites it is built for, the schedule's
own decode check on it, and the reference's SSS path on the poisoned x."""
import numpy as np
import pytest

import cfs_spmv_amd as cfs
import rand_matrices as rm

NO_REORDER, NO_CALIBRATE, HYB = 8, 32, 128
POISONS = (np.nan, np.inf, -np.inf)


@pytest.fixture(scope="module")
def case():
    n, rp, ci, special, expect = rm.sym_confinement_case(np.random.default_rng(0))
    va, x = rm.sym_int_values(np.random.default_rng(1), n, rp, ci)
    return n, rp, ci, special, expect, va, x, expect.sites


def test_expect_is_what_the_numpy_reference_gives_for_each_poison(case):
    """one column at a time and all at once: the non-finite rows of sym_reference are expect[j], and
    every other row is the integer product"""
    n, rp, ci, special, expect, va, x, _ = case
    exact = rm.sym_int_product(n, rp, ci, va, x)
    assert np.array_equal(rm.sym_reference(n, rp, ci, va, x), exact)
    assert np.abs(exact).max() < 2 ** 24 and np.abs(va).max() <= 8 and np.abs(x).max() <= 8 and np.all(va != 0)
    for poison in POISONS:
        for cols in [[j] for j in special] + [special]:
            xp = x.copy()
            xp[cols] = poison
            y = rm.sym_reference(n, rp, ci, va, xp)
            want = np.unique(np.concatenate([expect[int(j)] for j in cols]))
            assert np.array_equal(np.flatnonzero(~np.isfinite(y)), want), (poison, cols)
            fin = np.isfinite(y)
            assert np.array_equal(y[fin], exact[fin])
            if np.isinf(poison):  # never +Inf and -Inf in one row: a NaN only where 0 * Inf stands for a missing diagonal
                nan = np.flatnonzero(np.isnan(y))
                assert set(nan) <= {int(j) for j in cols} and all(j not in ci[rp[j]:rp[j + 1]] for j in nan)


def test_every_site_is_there(case):
    n, rp, ci, special, expect, va, x, site = case
    f = rm.sym_row_features(n, rp, ci, special, expect)
    low = lambda i: (lambda c: c[c < i])(ci[rp[i]:rp[i + 1]])
    assert site["col0"] == 0 and site["last"] == n - 1 and {0, n - 1} <= set(special)
    assert any("packet" in t for t in f.values()) and any("leftover" in t for t in f.values())
    assert "packet" in f[site["band"]]
    assert {"no_diag_self", "no_diag_ref"} <= f[site["nodiag"]]
    assert all(j in ci[rp[j]:rp[j + 1]] for j in special if j != site["nodiag"])  # ... the others store theirs
    for j in site["lonely"]:
        assert f[j] == {"no_lower"} and list(expect[j]) == [j]
    # the sibling chain: three rows with the same first column; the last has three packets, the others two,
    # whose eight columns open the long row's; the special column is the ninth of the long row only
    r = int(np.flatnonzero(np.array([low(i).size == 12 and site["sibling"] in low(i) for i in expect[site["sibling"]]]))[0])
    r = int(expect[site["sibling"]][r])
    a, b, c = low(r - 2), low(r - 1), low(r)
    assert (a.size, b.size, c.size) == (8, 9, 12) and np.array_equal(a, c[:8]) and np.array_equal(b[:8], c[:8])
    assert c[8] == site["sibling"] and site["sibling"] not in a and site["sibling"] not in b
    # long rows: more than 32 packets, so split wherever the tile's rows average fewer than 16
    assert "late" in f[site["long_col"]]
    assert low(site["long_row"]).size >= 160 and site["long_row"] in special
    # the hub run: every row but the lonely ones holds exactly the 16 columns up to the hub; a lonely row
    # every 37 rows, so any 64 consecutive rows of the run hold one
    run = expect[site["hub"]][expect[site["hub"]] > site["hub"]]
    lonely = np.array(site["lonely"])
    assert np.array_equal(np.sort(np.concatenate([run, lonely])), site["hub"] + 1 + np.arange(rm.SYM_CONFINE_RUN))
    assert np.diff(lonely).max() == 37 and lonely[0] - site["hub"] <= 37 and site["hub"] + rm.SYM_CONFINE_RUN - lonely[-1] <= 37
    assert all(np.array_equal(low(i), np.arange(site["hub"] - 15, site["hub"] + 1)) for i in run[::97])
    # first quarter <- last quarter
    assert (expect[site["far_once"]] > 3 * n // 4).sum() == 1 and site["far_once"] < n // 4
    assert (expect[site["far_node"]] > 3 * n // 4).sum() == 5
    assert site["sender"] > 3 * n // 4 and (expect[site["sender"]] < n // 4).sum() == 1


@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
def test_schedules_of_the_case_decode_to_the_input(case, dtype):
    n, rp, ci, special, expect, va, x, site = case
    va = va.astype(dtype)
    low = int((np.repeat(np.arange(n), np.diff(rp)) > ci).sum())  # entries of the strict lower triangle
    for block, slots, flags in ((256, 768, NO_REORDER), (512, 1536, NO_REORDER | HYB), (1024, 0, 0), (512, 0, 16)):
        rep = cfs.plan_check(n, rp, ci, va, options=cfs.make_options(slots, 0, block, flags | NO_CALIBRATE))
        assert rep["mismatches"] == 0 and rep["decoded"] == rep["nnz_low"] == low, rep
        if flags & HYB:
            assert rep["far_entries"] > 0
    for splits in ([0, n // 2, n], [0, n // 3, 2 * n // 3, n]):
        rs, nr = np.array(splits, np.int32), len(splits) - 1
        for xflag in (0, cfs.FLAG_SHARD_EXCHANGE):
            tot, mirror, remote = 0, 0, 0
            for rank in range(nr):
                rep = cfs.plan_check(n, rp, ci, va, nr, rank, rs, options=cfs.make_options(1536, 0, 512, NO_REORDER | NO_CALIBRATE | xflag))
                assert rep["mismatches"] == 0 and rep["decoded"] == rep["nnz_low"] + rep["mirror_entries"], rep
                tot += rep["nnz_low"]
                mirror += rep["mirror_entries"]
                remote += rep["remote_vals"]
                # first-quarter columns held by rows of the last quarter: the last rank sends its sums for
                # them (exchange form); mirrored, the first rank keeps the images of those entries
                if xflag and rank == nr - 1:
                    assert rep["remote_vals"] > 0, rep
                if not xflag and rank == 0:
                    assert rep["mirror_entries"] > 0, rep
            assert tot == low
            assert (remote > 0 and mirror == 0) if xflag else (mirror > 0 and remote == 0)


@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
def test_reference_sss_path_has_the_same_non_finite_rows(case, dtype):
    """oracle.SymOracle (the reference's SSS kernel, one thread) on the poisoned x: its non-finite
    rows are the contract's, for every poison, and the finite rows are the integer product."""
    from oracle import oracle
    n, rp, ci, special, expect, va, x, _ = case
    va, x = va.astype(dtype), x.astype(dtype)
    exact = rm.sym_int_product(n, rp, ci, va, x)
    o = oracle.SymOracle(n, rp, ci, va, 1)
    for poison in POISONS:
        xp = x.copy()
        xp[special] = poison
        y = o.spmv(xp)
        ref = rm.sym_reference(n, rp, ci, va, xp)
        assert np.array_equal(np.flatnonzero(~np.isfinite(y)), np.flatnonzero(~np.isfinite(ref))), poison
        fin = np.isfinite(ref)
        assert np.array_equal(y[fin], exact[fin])
        assert np.array_equal(np.isnan(y), np.isnan(ref)) and np.array_equal(np.sign(y[~fin & ~np.isnan(ref)]), np.sign(ref[~fin & ~np.isnan(ref)]))
    o.close()


@pytest.mark.parametrize("dof", [1, 2, 4])
def test_fixed_number_of_unknowns_per_node(dof):
    """dof = k: every node outside the designed sites has k unknowns; same guarantees"""
    n, rp, ci, special, expect = rm.sym_confinement_case(np.random.default_rng(dof), dof=dof)
    va, x = rm.sym_int_values(np.random.default_rng(2), n, rp, ci)
    assert set(expect.sites) == {"col0", "band", "nodiag", "sibling", "long_col", "long_row", "hub", "lonely",
                                 "far_once", "far_node", "sender", "last"}
    xp = x.copy()
    xp[special] = np.inf
    y = rm.sym_reference(n, rp, ci, va, xp)
    assert np.array_equal(np.flatnonzero(~np.isfinite(y)), np.unique(np.concatenate(list(expect.values()))))
    rep = cfs.plan_check(n, rp, ci, va, options=cfs.make_options(768, 0, 256, NO_REORDER | NO_CALIBRATE | HYB))
    assert rep["mismatches"] == 0 and rep["far_entries"] > 0
