"""The locally dominant matching and the entry points of the device set-up without a GPU, by the method of
test_amg_abi.py: the header declares the new symbols, the library exports them, the ctypes binding declares them; the
argument checks of cfs_hip_amg_create_dominant_* and cfs_hip_amg_create_device_* answer before anything touches a
device, in the order and words of cfs_hip_amg_create_*; and one level of the host set-up with the new matching,
cfs_hip_debug_amg_coarsen_dominant, against the rule as include/cfs_hip.h words it.

  _model restates the text of the header in plain Python floats on dictionaries, with its own copy of the hash h:
  candidate edges with s > 0, the total order (larger s, even smaller endpoint, smaller h, smaller (lo, hi)), synchronous
  rounds until one forms no pair or 64 have run, aggregates numbered by smallest member, then Q^T B Q summed in
  ascending (row, column) order.  cfs.coarsen(matching="dominant") must give its aggregates, weights, pattern and coarse
  values in every bit, and its round counts.  The same model with the rounds replaced by ONE sequential pass over the
  sorted edges (take an edge when both ends are free) must give the same again wherever the cap was not reached.

  The cap: a chain of 200 rows whose strength grows strictly along it forms exactly one pair per round, from its far
  end: 64 rounds, 64 pairs, 72 singletons, where the sorted pass pairs all 200 rows."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

import cfs_spmv_amd as cfs
from cfs_spmv_amd import _lib
from test_amg_abi import MATRICES, U, LD, _disturbed, _iso2d, _reference, _same_level, matrix

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("cfs_hip_amg_create_dominant_f64", "cfs_hip_amg_create_dominant_f32", "cfs_hip_amg_create_device_f64",
       "cfs_hip_amg_create_device_f32", "cfs_hip_amg_setup_info", "cfs_hip_debug_amg_coarsen_dominant")
CASES = MATRICES + ("iso2d13x11",)
CAP = 64
_MODEL = {}


def get(name):
    if name == "chain200":
        return chain(200)
    return _iso2d(13, 11) if name.startswith("iso2d") else matrix(name)


def chain(n):
    """off-diagonals -0.001 k between rows k - 1 and k, every diagonal entry the sum of the moduli of its off-diagonals
    plus 1: the strength grows strictly along the chain"""
    import scipy.sparse as sp
    off = -0.001 * np.arange(1, n)
    d = np.ones(n)
    d[:-1] += np.abs(off)
    d[1:] += np.abs(off)
    A = sp.diags([off, d, off], [-1, 0, 1]).tocsr()
    A.sort_indices()
    return n, A.indptr.astype(np.int32), A.indices.astype(np.int32), A.data.astype(np.float64)


def _h(lo, hi):
    m = 0xFFFFFFFF
    x = ((lo * 0x9E3779B1) & m) ^ ((hi * 0x85EBCA77) & m)
    x ^= x >> 15
    x = (x * 0x2C1B3C6D) & m
    x ^= x >> 12
    x = (x * 0x297A2D39) & m
    x ^= x >> 15
    return x


def _order(s, i, j):
    """the place of the edge (i, j) of strength s in the total order: smaller comes first"""
    lo, hi = min(i, j), max(i, j)
    return (-s, lo & 1, _h(lo, hi), lo, hi)


def _model(n, rp, ci, va, passes, sequential=False):
    """One level as the header words it.  sequential: every pass by one pass over the sorted edges instead of rounds.
    Returns (what cfs.coarsen returns, the rounds of every pass, the number of rows at which an edge won against
    another of exactly the same strength -- where the parity or the hash decided)"""
    rp, ci, va = rp.tolist(), ci.tolist(), va.tolist()
    diag = {ci[k]: va[k] for i in range(n) for k in range(rp[i], rp[i + 1]) if ci[k] == i}
    w = [1.0 / math.sqrt(diag[i]) for i in range(n)]
    B = {i: {} for i in range(n)}
    for i in range(n):
        for k in range(rp[i], rp[i + 1]):
            if ci[k] <= i:
                assert ci[k] not in B[i]
                B[i][ci[k]] = B[ci[k]][i] = (w[i] * va[k]) * w[ci[k]]
    agg, rounds, decided = list(range(n)), [], 0
    for _ in range(passes):
        strength = lambda i, j: abs(B[i][j]) / math.sqrt(B[i][i] * B[j][j])
        mate = {}
        if sequential:
            edges = sorted(_order(strength(i, j), i, j) for i in B for j in B[i] if j < i and strength(i, j) > 0)
            for _, _, _, lo, hi in edges:
                if lo not in mate and hi not in mate:
                    mate[lo], mate[hi] = hi, lo
            rounds.append(0)
        else:
            r = 0
            while r < CAP:
                r += 1
                to = {}
                for i in B:
                    if i in mate:
                        continue
                    cand = sorted(_order(strength(i, j), i, j) + (j,) for j in B[i]
                                  if j != i and j not in mate and strength(i, j) > 0)
                    if cand:
                        to[i] = cand[0][-1]
                        decided += len(cand) > 1 and cand[0][0] == cand[1][0]
                pairs = [(i, j) for i, j in to.items() if i < j and to.get(j) == i]
                for i, j in pairs:
                    mate[i], mate[j] = j, i
                if not pairs:
                    break
            rounds.append(r)
        q, made = {}, 0
        for i in sorted(B):  # numbered by smallest member, ascending
            if i not in q:
                q[i] = made
                if i in mate:
                    q[mate[i]] = made
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
    level = (np.array(agg, np.int32), np.array(w, np.float64),
             (nc, crp, np.array([J for r in low for J, _ in r], np.int32), np.array([v for r in low for _, v in r], np.float64)))
    return level, rounds, decided


def model(name, passes, sequential=False):
    """computed once, shared, unchanged"""
    key = (name, passes, sequential)
    if key not in _MODEL:
        _MODEL[key] = _model(*get(name), passes, sequential)
    return _MODEL[key]


def test_the_symbols_are_declared_exported_and_bound():
    text = open(os.path.join(ROOT, "include", "cfs_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    lib = cfs.load()
    raw = C.CDLL(cfs.lib_path())
    for name in NEW:
        assert re.search(r"\bint\s+" + name + r"\s*\(", code), f"{name} is not declared in cfs_hip.h"
        assert name in _lib.SYMBOLS
        getattr(raw, name)  # dlsym
    assert re.search(r"#define\s+CFS_HIP_AMG_MATCH_ROUNDS\s+64\b", code) and _lib.AMG_MATCH_ROUNDS == CAP
    assert re.search(r"#define\s+CFS_HIP_AMG_MATCHING_GREEDY\s+0\b", code) and re.search(r"#define\s+CFS_HIP_AMG_MATCHING_DOMINANT\s+1\b", code)
    assert (_lib.AMG_MATCHING_GREEDY, _lib.AMG_MATCHING_DOMINANT) == (0, 1)
    # the constants of the hash stand in the header as the model has them
    for const in ("0x9E3779B1u", "0x85EBCA77u", "0x2C1B3C6Du", "0x297A2D39u"):
        assert const in text
    vp, ip, dp, i, ll = C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_double), C.c_int, C.c_longlong
    for suf in ("f64", "f32"):
        for kind in ("dominant_", "device_"):
            assert getattr(lib, "cfs_hip_amg_create_" + kind + suf).argtypes == [vp, i, vp, vp, vp, C.POINTER(_lib.AmgOptions), C.POINTER(vp)]
    assert lib.cfs_hip_amg_setup_info.argtypes == [vp, ip, ip, ip, dp, C.POINTER(ll)]
    assert lib.cfs_hip_debug_amg_coarsen_dominant.argtypes == [i, vp, vp, vp, i, vp, vp, ip, vp, vp, vp, ll, C.POINTER(ll), ip]
    assert callable(cfs.Amg.setup_info)
    import inspect
    for f in (cfs.SymMatrix.amg, cfs.Amg.__init__):
        par = inspect.signature(f).parameters
        assert par["matching"].default == "greedy" and par["setup"].default == "host"
    assert inspect.signature(cfs.coarsen).parameters["matching"].default == "greedy"


def test_argument_checks_answer_before_any_device_work():
    """both new create families: null first, then passes, degree, ratio, coarse_max, each in the words of
    cfs_hip_amg_create_* (the same message from the same code), *out = NULL on every error"""
    lib = cfs.load()
    bound = lib.cfs_hip_runtime_bound()
    n, rp, ci, va = matrix("rand63")
    fake = C.c_void_p(0x1000)  # (never dereferenced: every check below comes before the handle is looked at)

    def create(kind, h=fake, rowptr=rp, colind=ci, values=va, out=True, suf="f64", **kw):
        a = C.c_void_p(0x7)
        o = dict(passes=0, degree=0, coarse_max=0, ratio=0.0)
        o.update(kw)
        opt = _lib.AmgOptions(o["passes"], o["degree"], o["coarse_max"], 0, o["ratio"])
        v = None if values is None else values.astype(np.float64 if suf == "f64" else np.float32)
        rc = getattr(lib, "cfs_hip_amg_create_" + kind + suf)(h, n, None if rowptr is None else rowptr.ctypes.data,
                                                              None if colind is None else colind.ctypes.data,
                                                              None if v is None else v.ctypes.data, C.byref(opt),
                                                              C.byref(a) if out else None)
        assert not out or a.value is None
        return rc, lib.cfs_hip_last_error()

    everything_bad = dict(passes=9, degree=9, ratio=np.nan, coarse_max=5000)
    order = [("passes", (-1, 4, 9), b"passes"), ("degree", (-1, 5, 17), b"degree"),
             ("ratio", (1.0, 0.5, -4.0, np.inf, np.nan), b"ratio"), ("coarse_max", (-1, 1025, 5000), b"coarse_max")]
    for kind in ("dominant_", "device_"):
        for suf in ("f64", "f32"):
            for kw in (dict(h=None), dict(rowptr=None), dict(colind=None), dict(values=None), dict(out=False)):
                rc, msg = create(kind, suf=suf, **kw, **everything_bad)
                assert rc == _lib.ERR_ARG and b"null" in msg, (kind, kw, msg)
            for k, (field, values, word) in enumerate(order):
                later = {f: everything_bad[f] for f, _, _ in order[k + 1:]}
                for v in values:
                    rc, msg = create(kind, suf=suf, **{field: v}, **later)
                    assert rc == _lib.ERR_ARG and word in msg, (kind, field, v, msg)
                    assert (rc, msg) == create("", suf=suf, **{field: v}, **later)  # the words of cfs_hip_amg_create_*
    # the host-only entry
    agg, w = np.zeros(n, np.int32), np.zeros(n)
    crp, cci, cva = np.zeros(n + 1, np.int32), np.zeros(len(ci), np.int32), np.zeros(len(ci))
    nc, nnz, rounds = C.c_int(), C.c_longlong(), (C.c_int * 3)()
    args = [n, rp.ctypes.data, ci.ctypes.data, va.ctypes.data, 2, agg.ctypes.data, w.ctypes.data, C.byref(nc), crp.ctypes.data,
            cci.ctypes.data, cva.ctypes.data, len(ci), C.byref(nnz), rounds]
    for k in (1, 5, 6, 7, 8, 12, 13):
        bad = list(args)
        bad[k] = None
        assert lib.cfs_hip_debug_amg_coarsen_dominant(*bad) == _lib.ERR_ARG and b"null" in lib.cfs_hip_last_error(), k
    for passes in (0, 4, -1):
        bad = list(args)
        bad[4] = passes
        assert lib.cfs_hip_debug_amg_coarsen_dominant(*bad) == _lib.ERR_ARG and b"passes" in lib.cfs_hip_last_error()
    assert lib.cfs_hip_debug_amg_coarsen_dominant(*args) == 0 and rounds[0] >= 1 and rounds[1] >= 1 and rounds[2] == 0
    assert lib.cfs_hip_amg_setup_info(None, None, None, None, None, None) == _lib.ERR_ARG
    with pytest.raises(ValueError):
        cfs.coarsen(n, rp, ci, va, 2, matching="heavy")
    assert lib.cfs_hip_runtime_bound() == bound  # nothing above initialised the runtime


def test_the_python_arguments_are_checked_before_the_library_is_asked():
    """setup="device" with the greedy matching does not exist, nor a refreshable dominant hierarchy, nor other words"""
    n, rp, ci, va = matrix("rand63")

    class NoHandle:  # (the ValueError comes before the matrix is looked at)
        pass

    for kw in (dict(setup="device"), dict(setup="device", matching="greedy"), dict(matching="dominant", refreshable=True),
               dict(matching="other"), dict(setup="gpu", matching="dominant")):
        with pytest.raises(ValueError):
            cfs.Amg(NoHandle(), rp, ci, va, **kw)


@pytest.mark.parametrize("passes", (1, 2, 3))
@pytest.mark.parametrize("name", CASES)
def test_the_matching_is_the_documented_one_bit_for_bit(name, passes):
    """cfs.coarsen(matching="dominant") against the rounds model: aggregates, weights, pattern, coarse values in every
    bit, and the rounds of every pass"""
    n, rp, ci, va = get(name)
    rounds = []
    got = cfs.coarsen(n, rp, ci, va, passes, matching="dominant", rounds=rounds)
    want, wrounds, decided = model(name, passes)
    sizes = np.bincount(np.bincount(want[0]), minlength=2 ** passes + 1)[1:]
    print(f"amg-dominant {name} passes={passes}: n={n} nc={want[2][0]} aggregates of 1 .. {2 ** passes} rows: "
          + "/".join(str(int(s)) for s in sizes) + f"; rounds {wrounds}; rows where parity or hash decided: {decided}")
    assert rounds == wrounds and max(wrounds) < CAP
    assert np.array_equal(got[0], want[0]), "the aggregates differ from the documented matching"
    assert _same_level(got, want)
    # numbered by smallest member, at most 2^passes rows each
    first = np.full(got[2][0], n)
    np.minimum.at(first, got[0], np.arange(n))
    assert np.all(np.diff(first) > 0) and np.bincount(got[0]).max() <= 2 ** passes


def test_the_cases_exercise_the_rounds_and_the_tie_keys():
    """counted by the model: a case that needs at least 3 rounds, and one where an edge wins against another of exactly
    the same strength -- on the isotropic grid every coupling is exactly 1/4, so parity and hash decide everywhere"""
    _, rounds_iso, decided_iso = model("iso2d13x11", 1)
    _, rounds_rand, _ = model("rand1026", 1)
    print(f"amg-dominant rounds: iso2d13x11 {rounds_iso} (rows decided by parity or hash: {decided_iso}), rand1026 {rounds_rand}")
    assert max(rounds_iso + rounds_rand) >= 3
    assert decided_iso >= 143 // 4


@pytest.mark.parametrize("passes", (1, 2, 3))
@pytest.mark.parametrize("name", CASES)
def test_below_the_cap_the_rounds_give_the_sequential_pass_over_the_sorted_edges(name, passes):
    n, rp, ci, va = get(name)
    want, _, _ = model(name, passes, sequential=True)
    assert _same_level(cfs.coarsen(n, rp, ci, va, passes, matching="dominant"), want)


def test_the_cap_of_64_rounds():
    n, rp, ci, va = chain(200)
    rows = np.repeat(np.arange(n), np.diff(rp))
    w = 1 / np.sqrt(va[rows == ci])
    s = np.abs(va[ci == rows - 1]) * w[1:] * w[:-1]
    assert len(s) == 199 and np.all(np.diff(s) > 0)  # the strength grows strictly along the chain
    rounds = []
    got = cfs.coarsen(n, rp, ci, va, 1, matching="dominant", rounds=rounds)
    want, wrounds, _ = model("chain200", 1)
    seq, _, _ = model("chain200", 1, sequential=True)
    assert rounds == wrounds == [CAP]
    assert _same_level(got, want)
    sizes = np.bincount(got[0])
    assert int((sizes == 1).sum()) == 72 and int((sizes == 2).sum()) == 64
    assert int((np.bincount(seq[0]) == 1).sum()) == 0 and not np.array_equal(got[0], seq[0])


@pytest.mark.parametrize("passes", (1, 2, 3))
def test_an_exactly_scaled_matrix_has_the_same_aggregates(passes):
    """D A D with D powers of two: the same aggregates, the coarse matrix within the bound of test_amg_abi.py"""
    n, rp, ci, va = matrix("rand1026")
    rows = np.repeat(np.arange(n), np.diff(rp))
    d = 2.0 ** np.random.default_rng(7).integers(-20, 21, n)
    vas = d[rows] * va * d[ci]
    agg, w, (nc, crp, cci, cva) = cfs.coarsen(n, rp, ci, va, passes, matching="dominant")
    aggs, ws, (ncs, crps, ccis, cvas) = cfs.coarsen(n, rp, ci, vas, passes, matching="dominant")
    assert ncs == nc and np.array_equal(aggs, agg) and np.array_equal(crps, crp) and np.array_equal(ccis, cci)
    assert not np.allclose(ws, w)
    _, _, sa, k = _reference(n, rp, ci, va, agg, w, nc)
    assert np.all(np.abs(cvas.astype(LD) - cva.astype(LD)) <= (k + 4) * LD(U) * sa)


@pytest.mark.parametrize("passes", (1, 2, 3))
@pytest.mark.parametrize("name", ("rand63", "rand1026", "lap2d40x33-scaled"))
def test_a_disturbed_csr_coarsens_to_the_same_bits(name, passes):
    n, rp, ci, va = matrix(name)
    rp2, ci2, va2 = _disturbed(n, rp, ci, va, seed=n + passes)
    assert _same_level(cfs.coarsen(n, rp2, ci2, va2, passes, matching="dominant"), cfs.coarsen(n, rp, ci, va, passes, matching="dominant"))


@pytest.mark.parametrize("passes", (1, 2, 3))
@pytest.mark.parametrize("name", CASES)
def test_the_greedy_matching_is_the_old_call(name, passes):
    n, rp, ci, va = get(name)
    old = cfs.coarsen(n, rp, ci, va, passes)
    assert _same_level(cfs.coarsen(n, rp, ci, va, passes, matching="greedy"), old)
