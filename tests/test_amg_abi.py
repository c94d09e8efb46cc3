"""The aggregation multigrid entry points without a GPU, by the method of test_pcg_cheb_abi.py: the header declares
them, the library exports them, the ctypes binding declares them; the argument checks of cfs_hip_amg_create_* answer
before anything touches a device, in the documented order; and one level of the set-up, cfs_hip_debug_amg_coarsen
(host only), against what it is documented to compute:

  agg is a partition onto 0 .. nc - 1 with aggregates of at most 2^passes rows, numbered by their first row, each
  connected in the graph of A;  w = 1 / sqrt(a_ii) to 2 ulp;  the coarse matrix is P^T A P with P = diag(w) Q, Q the
  0/1 map of agg.  The reference sums w_i a_ij w_j, with the RETURNED w, over the contributions of every coarse entry
  in np.longdouble.  The library computes each term with two roundings ((w_i a_ij) w_j; w itself carries a third against
  1 / sqrt(a_ii), which the reference shares) and adds the k terms of an entry in k - 1 roundings, each on a partial
  sum of modulus at most S = sum |terms|: an entry may differ by (k + 4) 2^-53 S.

  Invariance: the weights make B = W A W, and so the matching and the coarse matrix, independent of a symmetric
  scaling of A -- the coarse matrix of D A D equals that of A within the same bound, with the same aggregates.

  lap2d(40, 33) with 2 passes: 330 aggregates of 4 (a numpy model of the algorithm gave exactly 330 / 1320 before
  the library did), asserted as nc <= 0.30 n.

  The rule itself: _model_coarsen restates the text of include/cfs_hip.h in plain Python, and cfs.coarsen must give
  its aggregates, weights, pattern and coarse values in every bit (6 matrices and an isotropic Laplacian, where ties
  between free neighbours really occur; 1, 2, 3 passes).  What the reading of the caller's CSR promises: entries above
  the diagonal ignored, unsorted rows sorted, duplicates summed -- a CSR disturbed in all three ways coarsens to the
  same bits."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import cfs_spmv_amd as cfs
from cfs_spmv_amd import _lib
from test_gpu_cg_steps import _matrix
from test_gpu_lobpcg import scaled
from test_gpu_lobpcg_steps import lap2d

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("cfs_hip_amg_create_f64", "cfs_hip_amg_create_f32", "cfs_hip_amg_destroy", "cfs_hip_amg_info",
       "cfs_hip_amg_level_aggregates", "cfs_hip_amg_level_matrix", "cfs_hip_amg_coarse_inverse", "cfs_hip_amg_apply",
       "cfs_hip_sym_pcg_amg", "cfs_hip_debug_amg_coarsen")
LD = np.longdouble
U = 2.0 ** -53
MATRICES = ("lap2d40x33", "lap2d40x33-scaled", "rand63", "rand1026", "rand1", "rand2")
_CACHE = {}


def matrix(name):
    """(n, rowptr, colind, values) in fp64, both triangles; computed once, shared, unchanged"""
    if name not in _CACHE:
        if name.endswith("-scaled"):
            m = scaled(*matrix(name[:-7]))
        elif name.startswith("lap2d"):
            m = lap2d(*(int(v) for v in name[5:].split("x")))
        else:
            m = _matrix(name)
        n, rp, ci, va = m
        _CACHE[name] = (n, np.asarray(rp, np.int32), np.asarray(ci, np.int32), np.asarray(va, np.float64))
    return _CACHE[name]


def test_the_symbols_are_declared_exported_and_bound():
    text = open(os.path.join(ROOT, "include", "cfs_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    lib = cfs.load()
    raw = C.CDLL(cfs.lib_path())
    for name in NEW:
        assert re.search(r"\bint\s+" + name + r"\s*\(", code), f"{name} is not declared in cfs_hip.h"
        assert name in _lib.SYMBOLS
        getattr(raw, name)  # dlsym
    assert re.search(r"#define\s+CFS_HIP_ABI_VERSION\s+4\b", code) and lib.cfs_hip_abi_version() == 4
    assert re.search(r"#define\s+CFS_HIP_AMG_MAX_LEVELS\s+16\b", code) and re.search(r"#define\s+CFS_HIP_AMG_MAX_COARSE\s+1024\b", code)
    assert re.search(r"typedef\s+struct\s+cfs_hip_amg_s\s*\*\s*cfs_hip_amg_t\s*;", code)
    assert re.search(r"int\s+passes\s*;\s*int\s+degree\s*;\s*int\s+coarse_max\s*;\s*int\s+reserved_\s*;\s*double\s+ratio\s*;", code)
    vp, ip, dp, i, d, ll = C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_double), C.c_int, C.c_double, C.c_longlong
    for suf in ("f64", "f32"):
        assert getattr(lib, "cfs_hip_amg_create_" + suf).argtypes == [vp, i, vp, vp, vp, C.POINTER(_lib.AmgOptions), C.POINTER(vp)]
    assert lib.cfs_hip_amg_apply.argtypes == [vp, vp, vp, vp]
    assert lib.cfs_hip_sym_pcg_amg.argtypes == [vp, vp, vp, vp, d, i, i, ip, dp, vp]
    assert lib.cfs_hip_debug_amg_coarsen.argtypes == [i, vp, vp, vp, i, vp, vp, ip, vp, vp, vp, ll, C.POINTER(ll)]
    assert C.sizeof(_lib.AmgOptions) == 24 and (_lib.AMG_MAX_LEVELS, _lib.AMG_MAX_COARSE) == (16, 1024)
    # the Python mirror
    for name in ("amg", "pcg_amg"):
        assert callable(getattr(cfs.SymMatrix, name))
    for name in ("info", "aggregates", "level_matrix", "coarse_inverse", "apply", "close"):
        assert callable(getattr(cfs.Amg, name))
    from cfs_spmv_amd import solver
    assert callable(solver.pcg_amg) and callable(solver.pcg_amg_native) and callable(cfs.coarsen)


def test_argument_checks_answer_before_any_device_work():
    lib = cfs.load()
    bound = lib.cfs_hip_runtime_bound()
    n, rp, ci, va = matrix("rand63")
    # (a non-null handle that is never dereferenced: every check below comes before the handle is looked at)
    fake = C.c_void_p(0x1000)

    def create(h=fake, rowptr=rp, colind=ci, values=va, out=True, suf="f64", **kw):
        a = C.c_void_p(0x7)
        o = dict(passes=0, degree=0, coarse_max=0, ratio=0.0)
        o.update(kw)
        opt = _lib.AmgOptions(o["passes"], o["degree"], o["coarse_max"], 0, o["ratio"])
        v = None if values is None else values.astype(np.float64 if suf == "f64" else np.float32)
        rc = getattr(lib, "cfs_hip_amg_create_" + suf)(h, n, None if rowptr is None else rowptr.ctypes.data,
                                                       None if colind is None else colind.ctypes.data,
                                                       None if v is None else v.ctypes.data, C.byref(opt),
                                                       C.byref(a) if out else None)
        assert not out or a.value is None  # *out = NULL on every error
        return rc, lib.cfs_hip_last_error()

    everything_bad = dict(passes=9, degree=9, ratio=np.nan, coarse_max=5000)
    for suf in ("f64", "f32"):
        for kw in (dict(h=None), dict(rowptr=None), dict(colind=None), dict(values=None), dict(out=False)):
            rc, msg = create(suf=suf, **kw, **everything_bad)  # (null comes first: the options are bad as well)
            assert rc == _lib.ERR_ARG and b"null" in msg, (kw, msg)
        # the order: passes, degree, ratio, coarse_max -- every later one is bad as well
        order = [("passes", (-1, 4, 9), b"passes"), ("degree", (-1, 5, 17), b"degree"),
                 ("ratio", (1.0, 0.5, -4.0, np.inf, np.nan), b"ratio"), ("coarse_max", (-1, 1025, 5000), b"coarse_max")]
        for k, (field, values, word) in enumerate(order):
            later = {f: everything_bad[f] for f, _, _ in order[k + 1:]}
            for v in values:
                rc, msg = create(suf=suf, **{field: v}, **later)
                assert rc == _lib.ERR_ARG and word in msg, (field, v, msg)
    # the host-only entry
    agg, w = np.zeros(n, np.int32), np.zeros(n)
    crp, cci, cva = np.zeros(n + 1, np.int32), np.zeros(len(ci), np.int32), np.zeros(len(ci))
    nc, nnz = C.c_int(), C.c_longlong()
    args = [n, rp.ctypes.data, ci.ctypes.data, va.ctypes.data, 2, agg.ctypes.data, w.ctypes.data, C.byref(nc), crp.ctypes.data,
            cci.ctypes.data, cva.ctypes.data, len(ci), C.byref(nnz)]
    for k in (1, 5, 6, 7, 8, 12):
        bad = list(args)
        bad[k] = None
        assert lib.cfs_hip_debug_amg_coarsen(*bad) == _lib.ERR_ARG and b"null" in lib.cfs_hip_last_error(), k
    for passes in (0, 4, -1):
        bad = list(args)
        bad[4] = passes
        assert lib.cfs_hip_debug_amg_coarsen(*bad) == _lib.ERR_ARG and b"passes" in lib.cfs_hip_last_error()
    bad = list(args)
    bad[11] = 3  # too little room: what is needed comes back
    assert lib.cfs_hip_debug_amg_coarsen(*bad) == _lib.ERR_ARG and 3 < nnz.value <= len(ci)
    assert lib.cfs_hip_debug_amg_coarsen(*args) == 0
    assert lib.cfs_hip_amg_destroy(None) == 0
    assert lib.cfs_hip_runtime_bound() == bound  # nothing above initialised the runtime


def _reference(n, rp, ci, va, agg, w, nc):
    """{(I, J): (sum of w_i a_ij w_j, sum of their moduli, their number)} over I >= J, in long double"""
    rows = np.repeat(np.arange(n), np.diff(rp))
    I, J = agg[rows], agg[ci]
    keep = I >= J
    term = (w.astype(LD)[rows] * va.astype(LD) * w.astype(LD)[ci])[keep]
    key = I[keep].astype(np.int64) * nc + J[keep]
    uniq, inv = np.unique(key, return_inverse=True)
    s, sa, k = np.zeros(len(uniq), LD), np.zeros(len(uniq), LD), np.zeros(len(uniq), np.int64)
    np.add.at(s, inv, term)
    np.add.at(sa, inv, np.abs(term))
    np.add.at(k, inv, 1)
    return uniq, s, sa, k


@pytest.mark.parametrize("passes", (1, 2, 3))
@pytest.mark.parametrize("name", MATRICES)
def test_one_level_of_the_set_up(name, passes):
    import scipy.sparse as sp
    from scipy.sparse.csgraph import connected_components
    n, rp, ci, va = matrix(name)
    agg, w, (nc, crp, cci, cva) = cfs.coarsen(n, rp, ci, va, passes)
    # a partition onto 0 .. nc - 1, numbered in order of creation (by first row), at most 2^passes rows each
    assert agg.min() == 0 and agg.max() == nc - 1
    sizes = np.bincount(agg, minlength=nc)
    assert sizes.min() >= 1 and sizes.max() <= 2 ** passes
    first = np.full(nc, n)
    np.minimum.at(first, agg, np.arange(n))
    assert np.all(np.diff(first) > 0)
    # every aggregate is connected in the graph of A: the edges inside aggregates alone leave exactly nc components
    rows = np.repeat(np.arange(n), np.diff(rp))
    inside = (agg[rows] == agg[ci]) & (va != 0)
    G = sp.csr_matrix((np.ones(int(inside.sum())), (rows[inside], ci[inside])), shape=(n, n))
    ncomp, label = connected_components(G, directed=False)
    assert ncomp == nc and len(set(zip(label.tolist(), agg.tolist()))) == nc
    # the weights
    diag = sp.csr_matrix((va, ci, rp), shape=(n, n)).diagonal()
    want = 1 / np.sqrt(diag)
    assert np.all(np.abs(w - want) <= 2 * np.spacing(want))
    # the coarse matrix: lower triangle + diagonal, columns ascending, P^T A P entry by entry
    assert len(crp) == nc + 1 and crp[0] == 0 and crp[-1] == len(cci) == len(cva) and np.all(np.diff(crp) >= 1)
    crow = np.repeat(np.arange(nc), np.diff(crp))
    assert np.all(cci <= crow) and np.all(cci[crp[1:] - 1] == np.arange(nc))
    key = crow.astype(np.int64) * nc + cci
    assert np.all(np.diff(key) > 0)
    uniq, s, sa, k = _reference(n, rp, ci, va, agg, w, nc)
    assert np.array_equal(key, uniq)  # the same pattern
    err = np.abs(cva.astype(LD) - s)
    allowed = (k + 4) * LD(U) * sa
    worst = float(np.max(err / np.maximum(allowed, LD(1e-300))))
    print(f"amg-coarsen {name} passes={passes}: n={n} nc={nc} nnz={len(cva)} largest aggregate {sizes.max()} "
          f"singletons {int((sizes == 1).sum())} worst error / allowed {worst:.3f}")
    assert np.all(err <= allowed), worst
    assert len(cva) <= int((ci <= rows).sum())  # never more stored entries than the input
    if name == "lap2d40x33" and passes == 2:
        assert nc <= 0.30 * n, (nc, n)


@pytest.mark.parametrize("passes", (1, 2, 3))
def test_the_hierarchy_is_invariant_under_a_symmetric_scaling(passes):
    """the coarse matrix of D A D, D = diag(10^uniform(-1, 1)), against that of A: the same aggregates, every entry
    within the bound of the test above"""
    n, rp, ci, va = matrix("lap2d40x33")
    ns, rps, cis, vas = matrix("lap2d40x33-scaled")
    assert ns == n and np.array_equal(rps, rp) and np.array_equal(cis, ci) and not np.allclose(vas, va)
    agg, w, (nc, crp, cci, cva) = cfs.coarsen(n, rp, ci, va, passes)
    aggs, ws, (ncs, crps, ccis, cvas) = cfs.coarsen(n, rps, cis, vas, passes)
    assert ncs == nc and np.array_equal(aggs, agg) and np.array_equal(crps, crp) and np.array_equal(ccis, cci)
    assert not np.allclose(ws, w)
    _, _, sa, k = _reference(n, rp, ci, va, agg, w, nc)
    err = np.abs(cvas.astype(LD) - cva.astype(LD))
    allowed = (k + 4) * LD(U) * sa
    print(f"amg-coarsen invariance passes={passes}: nc={nc} worst difference / allowed {float(np.max(err / allowed)):.3f}")
    assert np.all(err <= allowed)


@pytest.mark.parametrize("value", (0.0, -1.5, np.nan, np.inf, None))
def test_a_diagonal_that_is_not_positive_is_refused(value):
    """zero, negative, not finite, or missing (None): CFS_HIP_ERR_ARG in the words of the Jacobi refusal"""
    n, rp, ci, va = matrix("rand63")
    rows = np.repeat(np.arange(n), np.diff(rp))
    k = int(np.flatnonzero((rows == ci) & (rows == 40))[0])
    if value is None:
        keep = np.arange(len(ci)) != k
        rp2 = rp.copy()
        rp2[41:] -= 1
        rp, ci, va = rp2, ci[keep], va[keep]
    else:
        va = va.copy()
        va[k] = value
    with pytest.raises(_lib.CfsHipError, match="positive diagonal, 1 of 63") as e:
        cfs.coarsen(n, rp, ci, va, 2)
    assert e.value.code == _lib.ERR_ARG


# ---- the set-up restated from the text of cfs_hip.h, and what the reading of the caller's CSR promises ----------------
def _model_coarsen(n, rp, ci, va, passes, ties=None):
    """One level as include/cfs_hip.h words it, in plain Python floats (IEEE double, sqrt and division correctly
    rounded) on dictionaries {row: {column: value}} -- a restatement of the rules, not of the library's loops:
      w_i = 1 / sqrt(a_ii);  b_ij = (w_i a_ij) w_j from the entries with col <= row, mirrored
      per pass: the rows ascending; an unmatched row takes the unmatched neighbour with the largest
      |b_ij| / sqrt(b_ii b_jj) > 0, the columns ascending and the comparison strict (a tie keeps the smallest j);
      aggregates numbered as they are made;  then C = Q^T B Q: the entries with J <= I, each the sum of its
      contributions in ascending (row, column) order, and the upper triangle their mirror.
    Returns what cfs.coarsen returns.  The CSR must have no duplicate entries.  ties (a list): receives (pass, row) of
    every row that had two or more unmatched neighbours of the same, largest strength -- where the tie rule decided."""
    import math
    rp, ci, va = rp.tolist(), ci.tolist(), va.tolist()
    diag = {ci[k]: va[k] for i in range(n) for k in range(rp[i], rp[i + 1]) if ci[k] == i}
    w = [1.0 / math.sqrt(diag[i]) for i in range(n)]
    B = {i: {} for i in range(n)}
    for i in range(n):
        for k in range(rp[i], rp[i + 1]):
            if ci[k] <= i:
                assert ci[k] not in B[i]
                B[i][ci[k]] = B[ci[k]][i] = (w[i] * va[k]) * w[ci[k]]
    agg = list(range(n))
    for p in range(passes):
        q, made = {}, 0
        for i in sorted(B):
            if i in q:
                continue
            best, sbest, tied = None, 0.0, False
            for j in sorted(B[i]):
                if j != i and j not in q:
                    s = abs(B[i][j]) / math.sqrt(B[i][i] * B[j][j])
                    if s > sbest:
                        best, sbest, tied = j, s, False
                    elif s == sbest and best is not None:
                        tied = True
            if tied and ties is not None:
                ties.append((p, i))
            q[i] = made
            if best is not None:
                q[best] = made
            made += 1
        Cm = {I: {} for I in range(made)}
        for i in sorted(B):
            for j in sorted(B[i]):
                I, J = q[i], q[j]
                if J <= I:
                    Cm[I][J] = Cm[I][J] + B[i][j] if J in Cm[I] else B[i][j]
        for I in sorted(Cm):
            for J in Cm[I]:
                Cm[J][I] = Cm[I][J]
        agg, B = [q[a] for a in agg], Cm
    nc = len(B)
    low = [[(J, B[I][J]) for J in sorted(B[I]) if J <= I] for I in range(nc)]
    crp = np.cumsum([0] + [len(r) for r in low]).astype(np.int32)
    return (np.array(agg, np.int32), np.array(w, np.float64),
            (nc, crp, np.array([J for r in low for J, _ in r], np.int32), np.array([v for r in low for _, v in r], np.float64)))


def _same_level(got, want):
    """agg, w, the pattern and the coarse values: equal in every bit"""
    (agg, w, (nc, crp, cci, cva)), (agg2, w2, (nc2, crp2, cci2, cva2)) = got, want
    return (nc == nc2 and np.array_equal(agg, agg2) and np.array_equal(w.view(np.uint8), w2.view(np.uint8)) and
            np.array_equal(crp, crp2) and np.array_equal(cci, cci2) and cva.dtype == cva2.dtype == np.float64 and
            np.array_equal(cva.view(np.uint8), cva2.view(np.uint8)))


def _iso2d(nx, ny):
    """kron(I, T_nx) + kron(T_ny, I), T = tridiag(-1, 2, -1): the five-point Laplacian, every coupling equally strong"""
    import scipy.sparse as sp
    T = lambda n: sp.diags([-np.ones(n - 1), 2 * np.ones(n), -np.ones(n - 1)], [-1, 0, 1])
    A = (sp.kron(sp.identity(ny), T(nx)) + sp.kron(T(ny), sp.identity(nx))).tocsr()
    A.sort_indices()
    return A.shape[0], A.indptr.astype(np.int32), A.indices.astype(np.int32), A.data.astype(np.float64)


@pytest.mark.parametrize("passes", (1, 2, 3))
@pytest.mark.parametrize("name", MATRICES + ("iso2d13x11",))
def test_the_set_up_is_the_documented_one_bit_for_bit(name, passes):
    """cfs.coarsen against _model_coarsen: the same aggregates, weights, pattern and coarse VALUES in every bit -- the
    matching rule (strongest neighbour, ties to the smallest j) and the order of every sum are the documented ones, not
    merely some valid partition with its own P^T A P.
    Where the tie rule decides: the rows of lap2d have two equally strong neighbours, i - 1 and i + 1, but i - 1 is
    always matched already when row i has its turn, and the same holds on its coarse grids: the model counts NO row of
    lap2d40x33, in any pass, at which two free neighbours tie (the count is printed) -- a matching that broke ties
    towards the largest j passes every lap2d and rand case.  In the isotropic iso2d13x11 a row whose right and lower
    neighbours are both free has a tie between them (the strengths are exactly 1/4: w = 1/2 and b_ij = -1/4 are
    exact): 60 of its 143 rows in the first pass.  That is asserted, so that a change of the matrix cannot silently
    empty the case."""
    n, rp, ci, va = _iso2d(13, 11) if name.startswith("iso2d") else matrix(name)
    ties = []
    got, want = cfs.coarsen(n, rp, ci, va, passes), _model_coarsen(n, rp, ci, va, passes, ties)
    sizes = np.bincount(np.bincount(want[0]), minlength=2 ** passes + 1)[1:]
    per_pass = [sum(1 for p, _ in ties if p == k) for k in range(passes)]
    print(f"amg-model {name} passes={passes}: n={n} nc={want[2][0]} aggregates of 1 .. {2 ** passes} rows: "
          + "/".join(str(int(s)) for s in sizes) + f"; rows where a tie was broken, per pass: {per_pass}")
    assert int(sizes.sum()) == want[2][0] and int((sizes * np.arange(1, len(sizes) + 1)).sum()) == n
    if name == "iso2d13x11":
        assert per_pass[0] >= n // 4, per_pass
    assert np.array_equal(got[0], want[0]), "the aggregates differ from the documented matching"
    assert _same_level(got, want)


def _disturbed(n, rp, ci, va, seed):
    """the same matrix as amg_lower has to read it: every entry above the diagonal replaced by a random value, about
    half of those with col <= row split into two equal halves (v / 2 + v / 2 is exact), every row's columns shuffled"""
    rng = np.random.default_rng(seed)
    nrp, nci, nva = [0], [], []
    for i in range(n):
        cols, vals = [], []
        for k in range(rp[i], rp[i + 1]):
            j, v = int(ci[k]), float(va[k])
            if j > i:
                cols.append(j), vals.append(float(rng.uniform(-5, 5)))
            elif rng.random() < 0.5:
                assert v / 2 + v / 2 == v
                cols += [j, j]
                vals += [v / 2, v / 2]
            else:
                cols.append(j), vals.append(v)
        order = rng.permutation(len(cols))
        nci += [cols[k] for k in order]
        nva += [vals[k] for k in order]
        nrp.append(len(nci))
    return np.array(nrp, np.int32), np.array(nci, np.int32), np.array(nva, np.float64)


@pytest.mark.parametrize("passes", (1, 2, 3))
@pytest.mark.parametrize("name", ("rand63", "rand1026", "lap2d40x33-scaled"))
def test_entries_above_the_diagonal_duplicates_and_unsorted_rows(name, passes):
    """what the reading of the caller's CSR promises: entries with col > row are ignored, rows need not be sorted,
    duplicates are summed -- cfs.coarsen of the disturbed CSR equals that of the clean one in every bit"""
    n, rp, ci, va = matrix(name)
    rp2, ci2, va2 = _disturbed(n, rp, ci, va, seed=n + passes)
    rows, rows2 = np.repeat(np.arange(n), np.diff(rp)), np.repeat(np.arange(n), np.diff(rp2))
    # the disturbance is there: more entries, other values above the diagonal, rows that are not ascending
    assert len(ci2) > len(ci) + int((ci <= rows).sum()) // 4
    assert not np.array_equal(np.sort(va2[ci2 > rows2]), np.sort(va[ci > rows]))
    assert int(((np.diff(ci2) < 0) & (np.diff(rows2) == 0)).sum()) > n // 4
    assert _same_level(cfs.coarsen(n, rp2, ci2, va2, passes), cfs.coarsen(n, rp, ci, va, passes))
