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
  the library did), asserted as nc <= 0.30 n."""
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
