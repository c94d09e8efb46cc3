"""The refresh of a multigrid hierarchy without a GPU, by the method of test_amg_abi.py: the new entry points are
declared, exported and bound and refuse null arguments before any device work; and one level of a refresh,
cfs_hip_debug_amg_recoarsen (host only: the lists of cfs_hip_amg_create_refreshable_*, evaluated in the order the
kernels add), against a FROZEN MODEL -- _model_coarsen of test_amg_abi.py with the matching of every round replaced by
the q recorded from a run on the values at create, the same dictionaries and the same order of sums.

  The model itself is checked first, against code that existed before: with values_new = values_at_create it must
  reproduce cfs.coarsen in every bit.
  New values: every diagonal entry times 1 + uniform(0, 1), default_rng(7) -- the matrix stays positive definite, the
  strengths |b_ij| / sqrt(b_ii b_jj) do not change but b_ij themselves (and hence ties and the coarse strengths) do.
  On rand63 and rand1026 a fresh matching on these values differs from the frozen one at every pass count; that is
  asserted (and the number of rows that change aggregate printed), so the cases cannot silently stop telling a refresh
  from a re-match.
  The same through _disturbed: junk above the diagonal, entries split into duplicates, rows shuffled -- the lists must
  read exactly what amg_lower reads; and through disturbed3, whose splits are three UNEQUAL parts, so that the order in
  which the duplicates are added shows in the sum: it must be amg_lower's.
  Scaling: cfs.recoarsen(lap2d40x33, lap2d40x33-scaled) equals cfs.coarsen(lap2d40x33-scaled) in every bit (the
  aggregates coincide: the existing invariance test asserts it)."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

import cfs_spmv_amd as cfs
from cfs_spmv_amd import _lib
from test_amg_abi import _disturbed, _iso2d, _same_level, matrix

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("cfs_hip_amg_create_refreshable_f64", "cfs_hip_amg_create_refreshable_f32", "cfs_hip_amg_update_values_f64",
       "cfs_hip_amg_update_values_f32", "cfs_hip_amg_refresh_info", "cfs_hip_debug_amg_refresh_split",
       "cfs_hip_debug_amg_recoarsen")
CASES = ("rand63", "rand1026", "lap2d40x33", "iso2d13x11", "rand1", "rand2")
# rows that change aggregate when the new values are matched afresh, at 1, 2, 3 passes (counted with the model)
MOVED = {"rand63": (47, 35, 39), "rand1026": (835, 858, 955)}


def _case(name):
    return _iso2d(13, 11) if name.startswith("iso2d") else matrix(name)


def new_values(n, rp, ci, va, seed=7):
    """every diagonal entry times 1 + uniform(0, 1)"""
    f = 1.0 + np.random.default_rng(seed).uniform(0.0, 1.0, n)
    rows = np.repeat(np.arange(n), np.diff(rp))
    out = va.copy()
    d = rows == ci
    out[d] *= f[rows[d]]
    return out


def model_frozen(n, rp, ci, va, passes, qs=None):
    """_model_coarsen of test_amg_abi.py, word for word, except that with qs (a list of {row: aggregate} per round) the
    matching of every round is TAKEN from it instead of made.  Returns (what cfs.coarsen returns, the qs used)."""
    rp, ci, va = rp.tolist(), ci.tolist(), va.tolist()
    diag = {ci[k]: va[k] for i in range(n) for k in range(rp[i], rp[i + 1]) if ci[k] == i}
    w = [1.0 / math.sqrt(diag[i]) for i in range(n)]
    B = {i: {} for i in range(n)}
    for i in range(n):
        for k in range(rp[i], rp[i + 1]):
            if ci[k] <= i:
                assert ci[k] not in B[i]
                B[i][ci[k]] = B[ci[k]][i] = (w[i] * va[k]) * w[ci[k]]
    agg, used = list(range(n)), []
    for p in range(passes):
        if qs is not None:
            q = qs[p]
            made = max(q.values()) + 1
        else:
            q, made = {}, 0
            for i in sorted(B):
                if i in q:
                    continue
                best, sbest = None, 0.0
                for j in sorted(B[i]):
                    if j != i and j not in q:
                        s = abs(B[i][j]) / math.sqrt(B[i][i] * B[j][j])
                        if s > sbest:
                            best, sbest = j, s
                q[i] = made
                if best is not None:
                    q[best] = made
                made += 1
        used.append(q)
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
            (nc, crp, np.array([J for r in low for J, _ in r], np.int32), np.array([v for r in low for _, v in r], np.float64))), used


def bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a.view(np.uint8), b.view(np.uint8))


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
    vp, ip, dp, i, ll = C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_double), C.c_int, C.c_longlong
    for suf in ("f64", "f32"):
        assert getattr(lib, "cfs_hip_amg_create_refreshable_" + suf).argtypes == [vp, i, vp, vp, vp, C.POINTER(_lib.AmgOptions),
                                                                                 C.POINTER(vp)]
        assert getattr(lib, "cfs_hip_amg_update_values_" + suf).argtypes == [vp, vp, ll]
    assert lib.cfs_hip_amg_refresh_info.argtypes == [vp, C.POINTER(ll), ip, dp]
    assert lib.cfs_hip_debug_amg_recoarsen.argtypes == [i, vp, vp, vp, vp, i, vp, vp, ll, C.POINTER(ll)]
    assert C.sizeof(_lib.AmgOptions) == 24  # the layout of the options did not change
    for name in ("update_values", "refresh_info"):
        assert callable(getattr(cfs.Amg, name))
    assert callable(cfs.recoarsen)
    import inspect
    assert inspect.signature(cfs.SymMatrix.amg).parameters["refreshable"].default is False
    assert inspect.signature(cfs.Amg.__init__).parameters["refreshable"].default is False


def test_null_arguments_are_refused_before_any_device_work():
    lib = cfs.load()
    bound = lib.cfs_hip_runtime_bound()
    n, rp, ci, va = matrix("rand63")
    fake = C.c_void_p(0x1000)  # (never dereferenced: null comes first)
    opt = _lib.AmgOptions(0, 0, 0, 0, 0.0)
    for suf, dt in (("f64", np.float64), ("f32", np.float32)):
        v = va.astype(dt)
        create = getattr(lib, "cfs_hip_amg_create_refreshable_" + suf)
        for k in (0, 2, 3, 4, 6):
            a = C.c_void_p(0x7)
            args = [fake, n, rp.ctypes.data, ci.ctypes.data, v.ctypes.data, C.byref(opt), C.byref(a)]
            args[k] = None
            assert create(*args) == _lib.ERR_ARG and b"null" in lib.cfs_hip_last_error(), (suf, k)
            assert k == 6 or a.value is None
        update = getattr(lib, "cfs_hip_amg_update_values_" + suf)
        assert update(None, v.ctypes.data, len(v)) == _lib.ERR_ARG and b"null" in lib.cfs_hip_last_error()
        assert update(fake, None, len(v)) == _lib.ERR_ARG and b"null" in lib.cfs_hip_last_error()
    mb, cnt, sec = C.c_longlong(), C.c_int(), C.c_double()
    assert lib.cfs_hip_amg_refresh_info(None, C.byref(mb), C.byref(cnt), C.byref(sec)) == _lib.ERR_ARG
    # the host-only entry
    w, cva, nnz = np.zeros(n), np.zeros(len(ci)), C.c_longlong()
    args = [n, rp.ctypes.data, ci.ctypes.data, va.ctypes.data, va.ctypes.data, 2, w.ctypes.data, cva.ctypes.data, len(ci), C.byref(nnz)]
    for k in (1, 2, 3, 4, 6, 9):
        bad = list(args)
        bad[k] = None
        assert lib.cfs_hip_debug_amg_recoarsen(*bad) == _lib.ERR_ARG and b"null" in lib.cfs_hip_last_error(), k
    for passes in (0, 4, -1):
        bad = list(args)
        bad[5] = passes
        assert lib.cfs_hip_debug_amg_recoarsen(*bad) == _lib.ERR_ARG and b"passes" in lib.cfs_hip_last_error()
    bad = list(args)
    bad[8] = 3  # too little room: what is needed comes back
    assert lib.cfs_hip_debug_amg_recoarsen(*bad) == _lib.ERR_ARG and 3 < nnz.value <= len(ci)
    assert lib.cfs_hip_debug_amg_recoarsen(*args) == 0
    assert lib.cfs_hip_runtime_bound() == bound  # nothing above initialised the runtime


@pytest.mark.parametrize("passes", (1, 2, 3))
@pytest.mark.parametrize("name", CASES)
def test_the_frozen_model_with_unchanged_values_is_the_set_up(name, passes):
    """the model against code that was there before: its own matching, and the matching handed back to it frozen, both
    give cfs.coarsen in every bit"""
    n, rp, ci, va = _case(name)
    got = cfs.coarsen(n, rp, ci, va, passes)
    free, qs = model_frozen(n, rp, ci, va, passes)
    frozen, _ = model_frozen(n, rp, ci, va, passes, qs)
    assert _same_level(got, free) and _same_level(got, frozen)


@pytest.mark.parametrize("passes", (1, 2, 3))
@pytest.mark.parametrize("name", CASES)
def test_recoarsen_is_the_frozen_model_bit_for_bit(name, passes):
    n, rp, ci, va = _case(name)
    vb = new_values(n, rp, ci, va)
    old, qs = model_frozen(n, rp, ci, va, passes)
    want, _ = model_frozen(n, rp, ci, vb, passes, qs)
    fresh, _ = model_frozen(n, rp, ci, vb, passes)
    moved = int((fresh[0] != old[0]).sum())
    print(f"amg-recoarsen {name} passes={passes}: n={n} nc={old[2][0]}; a fresh matching on the new values moves {moved} rows")
    assert np.array_equal(want[0], old[0]) and np.array_equal(want[2][1], old[2][1]) and np.array_equal(want[2][2], old[2][2])
    if name in ("rand63", "rand1026"):
        assert moved == MOVED[name][passes - 1], "the case no longer tells a refresh from a re-match as it did"
        assert not bits(fresh[2][3], want[2][3])
    w, cva = cfs.recoarsen(n, rp, ci, va, vb, passes)
    assert bits(w, want[1]), "w differs from the frozen model"
    assert bits(cva, want[2][3]), "the coarse values differ from the frozen model"
    # and with the values unchanged: the set-up itself
    w0, cva0 = cfs.recoarsen(n, rp, ci, va, va, passes)
    assert bits(w0, old[1]) and bits(cva0, old[2][3])


@pytest.mark.parametrize("passes", (1, 2, 3))
@pytest.mark.parametrize("name", ("rand63", "rand1026"))
def test_recoarsen_reads_the_callers_csr_as_amg_lower_does(name, passes):
    """both arrays through _disturbed with one seed (the same pattern and shuffle: its draws do not depend on the
    values): junk above the diagonal, duplicates (v / 2 + v / 2, exact), unsorted rows"""
    n, rp, ci, va = matrix(name)
    vb = new_values(n, rp, ci, va)
    rp2, ci2, va2 = _disturbed(n, rp, ci, va, seed=n + passes)
    rp3, ci3, vb2 = _disturbed(n, rp, ci, vb, seed=n + passes)
    assert np.array_equal(rp2, rp3) and np.array_equal(ci2, ci3) and len(ci2) > len(ci)
    _, qs = model_frozen(n, rp, ci, va, passes)
    want, _ = model_frozen(n, rp, ci, vb, passes, qs)
    w, cva = cfs.recoarsen(n, rp2, ci2, va2, vb2, passes)
    assert bits(w, want[1]) and bits(cva, want[2][3])
    w1, cva1 = cfs.recoarsen(n, rp, ci, va, vb, passes)
    assert bits(w, w1) and bits(cva, cva1)


def disturbed3(n, rp, ci, arrays, seed):
    """_disturbed with splits whose ORDER shows: about half of the entries with col <= row become three unequal parts
    v f1, v f2, v - v f1 - v f2 (f drawn from (0.1, 0.4)), entries above the diagonal junk, every row shuffled; the same
    pattern, shuffle and fractions for every array of `arrays`.  Returns (rowptr, colind, [disturbed values], [clean
    values], reordered): clean = the arrays in the pattern given with every split entry replaced by the sum of its parts
    in the order they stand in the shuffled row, first + second, then + third -- what amg_lower has to compute;
    reordered = the entries of the first array whose parts give another fp64 number when added from the back."""
    rng = np.random.default_rng(seed)
    nrp, nci, out, clean, reordered = [0], [], [[] for _ in arrays], [np.array(v, np.float64) for v in arrays], 0
    for i in range(n):
        cols, vals, src = [], [[] for _ in arrays], []
        for k in range(rp[i], rp[i + 1]):
            j = int(ci[k])
            if j > i:
                junk = float(rng.uniform(-5, 5))
                cols.append(j), src.append(-1)
                for v in vals:
                    v.append(junk)
            elif rng.random() < 0.5:
                f1, f2 = (float(f) for f in rng.uniform(0.1, 0.4, 2))
                cols += [j, j, j]
                src += [k, k, k]
                for v, a in zip(vals, arrays):
                    x = float(a[k])
                    v += [x * f1, x * f2, x - x * f1 - x * f2]
            else:
                cols.append(j), src.append(k)
                for v, a in zip(vals, arrays):
                    v.append(float(a[k]))
        order = rng.permutation(len(cols))
        nci += [cols[t] for t in order]
        for m, v in enumerate(vals):
            row = [v[t] for t in order]
            out[m] += row
            parts = {}
            for t, x in zip(order, row):
                if src[t] >= 0:
                    parts.setdefault(src[t], []).append(x)
            for k, ps in parts.items():
                acc = ps[0]
                for x in ps[1:]:
                    acc = acc + x
                clean[m][k] = acc
                if m == 0 and len(ps) == 3 and (ps[2] + ps[1]) + ps[0] != acc:
                    reordered += 1
        nrp.append(len(nci))
    return np.array(nrp, np.int32), np.array(nci, np.int32), [np.array(v, np.float64) for v in out], clean, reordered


@pytest.mark.parametrize("passes", (1, 2, 3))
@pytest.mark.parametrize("name", ("rand63", "rand1026"))
def test_duplicates_are_summed_in_the_order_amg_lower_reads_them(name, passes):
    """three unequal parts per split entry: their sum depends on the order (asserted: for many entries the sum from the
    back is another number), and the lists must add them as amg_lower does -- in the order they stand in the row"""
    n, rp, ci, va = matrix(name)
    vb = new_values(n, rp, ci, va)
    rp2, ci2, (va2, vb2), (ca, cb), reordered = disturbed3(n, rp, ci, [va, vb], seed=n + passes)
    assert len(ci2) > len(ci) and reordered > n // 8, reordered
    assert _same_level(cfs.coarsen(n, rp2, ci2, va2, passes), cfs.coarsen(n, rp, ci, ca, passes))  # (amg_lower itself)
    _, qs = model_frozen(n, rp, ci, ca, passes)
    want, _ = model_frozen(n, rp, ci, cb, passes, qs)
    w, cva = cfs.recoarsen(n, rp2, ci2, va2, vb2, passes)
    assert bits(w, want[1]) and bits(cva, want[2][3])


@pytest.mark.parametrize("passes", (1, 2, 3))
def test_recoarsen_onto_scaled_values_is_the_set_up_of_the_scaled_matrix(passes):
    n, rp, ci, va = matrix("lap2d40x33")
    _, _, _, vs = matrix("lap2d40x33-scaled")
    agg, _, _ = cfs.coarsen(n, rp, ci, va, passes)
    aggs, ws, (_, _, _, cvas) = cfs.coarsen(n, rp, ci, vs, passes)
    assert np.array_equal(agg, aggs)  # (otherwise the case shows nothing)
    w, cva = cfs.recoarsen(n, rp, ci, va, vs, passes)
    assert bits(w, ws) and bits(cva, cvas)


def test_a_diagonal_that_is_not_positive_is_refused():
    n, rp, ci, va = matrix("rand63")
    rows = np.repeat(np.arange(n), np.diff(rp))
    k = int(np.flatnonzero((rows == ci) & (rows == 40))[0])
    for value in (0.0, -1.5, np.nan, np.inf):
        vb = va.copy()
        vb[k] = value
        with pytest.raises(_lib.CfsHipError, match="positive diagonal, 1 of 63") as e:
            cfs.recoarsen(n, rp, ci, va, vb, 2)
        assert e.value.code == _lib.ERR_ARG
