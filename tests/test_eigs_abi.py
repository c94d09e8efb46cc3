"""cfs_hip_sym_eigs, cfs_hip_sym_debug_lanczos, cfs_hip_debug_symeig and cfs_hip_debug_eigs_combine without a GPU: the header declares them with the
documented signatures, the library exports them, the ctypes bindings' argument types match the declarations, the
Python mirror is there, the argument checks that need no device answer before anything touches one -- and the small
dense eigensolver of the restart, which runs on the host, against numpy.linalg.eigh.

The entry points are additions: CFS_HIP_ABI_VERSION stays where the library's other tests pin it, and callers detect
them by their symbols, as they do for the other solver entry points.

cfs_hip_debug_symeig: with r = max_i ||T s_i - w_i s_i||inf and o = max |S^T S - I|, the library is allowed 8 x numpy's
own r and o on the same T plus 8 * 2^-53 * ||T||inf, and eigenvalue i may differ from numpy's by the sum of the two
residual 2-norms of pair i (each residual bounds the distance of its w_i to a true eigenvalue; the vectors have unit
norm to rounding).  That pairs the eigenvalues by index only where the gaps of the spectrum exceed the sum, which the
test asserts from numpy's spectrum for the matrices with distinct eigenvalues."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

import cfs_spmv_amd as cfs
from cfs_spmv_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIGNATURES = {
    "cfs_hip_sym_eigs": ["cfs_hip_sym_t h", "int k", "int which", "int ncv", "double tol", "int max_restarts",
                         "const void *v0_dev", "double *eigenvalues", "void *vectors_dev", "long long ld",
                         "double *residuals", "int *nconv", "int *restarts", "int *products", "void *stream"],
    "cfs_hip_sym_debug_lanczos": ["cfs_hip_sym_t h", "const void *v0_dev", "int steps", "void *basis_dev", "long long ld",
                                  "double *alpha", "double *beta", "int *done", "void *stream"],
    "cfs_hip_debug_symeig": ["int m", "const double *a", "double *w", "double *s"],
    "cfs_hip_debug_eigs_combine": ["void *out_dev", "long long ldo", "const void *basis_dev", "long long ld", "long long n", "int m",
                                   "int nout", "const double *s", "int value_bytes", "void *stream"],
}


def _header():
    text = open(os.path.join(ROOT, "include", "cfs_hip.h")).read()
    return re.sub(r"/\*.*?\*/", "", text, flags=re.S)


@pytest.mark.parametrize("name", list(SIGNATURES))
def test_the_symbols_are_declared_exported_and_bound(name):
    code = _header()
    m = re.search(r"\bint\s+" + name + r"\s*\((.*?)\)\s*;", code, flags=re.S)
    assert m, f"{name} is not declared in cfs_hip.h"
    params = [" ".join(p.split()) for p in m.group(1).split(",")]
    assert params == SIGNATURES[name]
    # appended behind cfs_hip_sym_minres
    assert code.index("cfs_hip_sym_minres") < m.start()
    assert name in _lib.SYMBOLS
    getattr(C.CDLL(cfs.lib_path()), name)  # dlsym
    lib = cfs.load()
    assert int(re.search(r"#define\s+CFS_HIP_ABI_VERSION\s+(\d+)\b", code).group(1)) == 4
    assert lib.cfs_hip_abi_version() == 4
    vp, ip, dp = C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_double)
    ctype = {"cfs_hip_sym_t": vp, "void *": vp, "const void *": vp, "int": C.c_int, "double": C.c_double, "int *": ip,
             "double *": dp, "const double *": dp, "long long": C.c_longlong}
    declared = [ctype[re.sub(r"\w+$", "", p).strip()] for p in params]
    assert getattr(lib, name).argtypes == declared


def test_the_constants():
    code = _header()
    for name, value in (("LARGEST", 0), ("SMALLEST", 1), ("MAGNITUDE", 2), ("MAX_NCV", 128)):
        assert int(re.search(r"#define\s+CFS_HIP_EIGS_" + name + r"\s+(\d+)\b", code).group(1)) == value
        assert getattr(_lib, "EIGS_" + name) == value


def test_the_python_mirror():
    from cfs_spmv_amd import solver
    p = inspect.signature(cfs.SymMatrix.eigs).parameters
    assert list(p) == ["self", "k", "which", "ncv", "tol", "max_restarts", "v0", "vectors", "stream"]
    assert [p[k].default for k in list(p)[1:]] == [6, "LA", None, 1e-10, 100, None, True, None]
    for f in (solver.eigs, solver.eigs_native):
        p = inspect.signature(f).parameters
        assert list(p)[:2] == ["A", "k"] and p["which"].default == "LA" and p["ncv"].default is None
        assert p["tol"].default == 1e-10 and p["max_restarts"].default == 100


def _call(lib, h, k=4, which=_lib.EIGS_LARGEST, ncv=20, tol=1e-8, max_restarts=10, v0=None, w=True, x=None, ld=0):
    vals = (C.c_double * 128)(*([7.0] * 128))
    nconv, restarts, products = C.c_int(7), C.c_int(7), C.c_int(7)
    rc = lib.cfs_hip_sym_eigs(h, k, which, ncv, tol, max_restarts, v0, vals if w else None, x, ld, None, C.byref(nconv),
                              C.byref(restarts), C.byref(products), None)
    return rc, (nconv.value, restarts.value, products.value), list(vals)


def test_null_arguments_are_refused_first():
    lib = cfs.load()
    bound = lib.cfs_hip_runtime_bound()
    h = C.c_void_p(0x1000)
    for which in (0, 1, 2, 3, -1):
        for k in (4, 0, -1):
            for hh, w in ((None, True), (h, False), (None, False)):
                rc, counters, vals = _call(lib, hh, k=k, which=which, w=w)
                assert rc == _lib.ERR_ARG and b"null" in lib.cfs_hip_last_error(), (which, k, hh, w)
                assert counters == (7, 7, 7) and vals == [7.0] * 128
    a, b, d = (C.c_double * 4)(), (C.c_double * 4)(), C.c_int(7)
    for args in ((None, None, 3, h, 16, a, b, C.byref(d)), (h, None, 3, None, 16, a, b, C.byref(d)),
                 (h, None, 3, h, 16, None, b, C.byref(d)), (h, None, 3, h, 16, a, None, C.byref(d)), (h, None, 3, h, 16, a, b, None)):
        assert lib.cfs_hip_sym_debug_lanczos(*args, None) == _lib.ERR_ARG and b"null" in lib.cfs_hip_last_error()
    assert d.value == 7
    # cfs_hip_debug_eigs_combine: the null check comes before every other one (m, nout, value_bytes, ld are bad too)
    s = (C.c_double * 4)()
    for out, basis, sp in ((None, h, s), (h, None, s), (h, h, None), (None, None, None)):
        assert lib.cfs_hip_debug_eigs_combine(out, 3, basis, 3, 16, 0, 5, sp, 3, None) == _lib.ERR_ARG
        assert b"null" in lib.cfs_hip_last_error()
    assert lib.cfs_hip_runtime_bound() == bound  # nothing above initialised the runtime


def test_checks_that_need_no_device_answer_before_the_handle_is_looked_at():
    lib = cfs.load()
    bound = lib.cfs_hip_runtime_bound()
    # (a non-null handle that is never dereferenced: the checks of the other arguments come first)
    h = C.c_void_p(0x1000)

    def refused(word, **kw):
        rc, counters, vals = _call(lib, h, **kw)
        msg = lib.cfs_hip_last_error()
        assert rc == _lib.ERR_ARG and word in msg, (kw, rc, msg)
        assert counters == (0, 0, 0) and vals == [7.0] * 128, kw  # the counters zeroed, nothing else written
        return msg
    # in the documented order: every later argument is bad as well
    bad = dict(k=0, tol=-1.0, max_restarts=-1, v0=C.c_void_p(0x3008))
    refused(b"unknown which", which=3, **bad)
    refused(b"unknown which", which=-1, **bad)
    del bad["k"]
    for k, ncv in ((0, 20), (-1, 20), (20, 20), (21, 20), (4, -1), (4, 129), (128, 0), (1, 1)):
        refused(b"k / ncv", k=k, ncv=ncv, **bad)
    del bad["tol"], bad["max_restarts"]
    for kw in (dict(tol=-1e-3), dict(tol=float("nan")), dict(max_restarts=-1)):
        refused(b"tolerance", **kw, **bad)
    refused(b"16-byte aligned", v0=C.c_void_p(0x3008))
    refused(b"16-byte aligned", x=C.c_void_p(0x4004), ld=1 << 20)
    a, b, d = (C.c_double * 4)(), (C.c_double * 4)(), C.c_int(7)
    for steps in (0, -1, 129):
        assert lib.cfs_hip_sym_debug_lanczos(h, None, steps, C.c_void_p(0x4000), 16, a, b, C.byref(d), None) == _lib.ERR_ARG
        assert b"steps" in lib.cfs_hip_last_error() and d.value == 0
    assert lib.cfs_hip_sym_debug_lanczos(h, None, 3, C.c_void_p(0x4008), 16, a, b, C.byref(d), None) == _lib.ERR_ARG
    assert b"16-byte aligned" in lib.cfs_hip_last_error()
    assert lib.cfs_hip_runtime_bound() == bound  # nothing above initialised the runtime


def test_the_restart_kernel_entry_point_refuses_before_any_device_work():
    """cfs_hip_debug_eigs_combine with pointers that are never dereferenced, in the documented order: every later argument
    is bad as well"""
    lib = cfs.load()
    bound = lib.cfs_hip_runtime_bound()
    s = (C.c_double * (128 * 128))()
    good = dict(out=0x100000, ldo=64, basis=0x100000, ld=64, n=60, m=20, nout=12, vb=8)

    def refused(word, **kw):
        a = dict(good, **kw)
        rc = lib.cfs_hip_debug_eigs_combine(C.c_void_p(a["out"]), a["ldo"], C.c_void_p(a["basis"]), a["ld"], a["n"], a["m"], a["nout"],
                                            s, a["vb"], None)
        msg = lib.cfs_hip_last_error()
        assert rc == _lib.ERR_ARG and word in msg, (kw, rc, msg)
    later = dict(vb=3, out=0x100008, ld=59)
    for m, nout in ((0, 0), (0, 1), (-1, 1), (129, 1), (129, 129), (20, 0), (20, -1), (20, 21), (128, 129), (1, 2)):
        refused(b"m / nout", m=m, nout=nout, **later)
    del later["vb"]
    for vb in (0, 1, 2, 3, 5, 16, -8):
        refused(b"value_bytes", vb=vb, **later)
    del later["out"]
    for kw in (dict(out=0x200008), dict(basis=0x100004), dict(out=0x200001, basis=0x100001), dict(out=0x100008, basis=0x100008)):
        refused(b"16-byte aligned", **kw, **later)
    del later["ld"]
    for kw in (dict(ld=59), dict(ldo=59), dict(out=0x200000, ldo=59), dict(ld=61), dict(ldo=63), dict(n=0), dict(n=-1), dict(n=65),
               dict(vb=4, ld=62), dict(vb=4, ldo=66), dict(ld=1 << 60, ldo=1 << 60), dict(ld=0, ldo=0, n=0)):
        refused(b"bad ld", **kw)
    # the in-place restart is out == basis AND ldo == ld; every other overlap of [first byte, row n - 1 of the last column]
    vb, ld, n, m, nout = 8, 64, 60, 20, 12
    base, span_b, span_o = 0x100000, ((m - 1) * ld + n) * vb, ((nout - 1) * ld + n) * vb
    for kw in (dict(ldo=66),                                     # the same start, another stride
               dict(out=base + ld * vb),                         # shifted by a column
               dict(out=base + 16), dict(out=base - 16),         # shifted by two rows
               dict(out=base + span_b - 16),                     # out begins on the basis's last two rows
               dict(out=base - span_o + 16),                     # out ends on the basis's first two rows
               dict(out=base - 0x80000, ldo=0x8000),             # out's wide columns straddle the whole basis
               dict(out=base + (m - 1) * ld * vb)):              # out begins at the basis's last column
        refused(b"overlap", **kw)
    assert span_b % 16 == 0 and span_o % 16 == 0
    assert lib.cfs_hip_runtime_bound() == bound  # nothing above initialised the runtime


# ---- cfs_hip_debug_symeig ----------------------------------------------------------------------------------------
def _symeig(T):
    m = T.shape[0]
    a = np.ascontiguousarray(T, np.float64)
    w, s = np.zeros(m), np.zeros((m, m))
    dp = C.POINTER(C.c_double)
    _lib.check(cfs.load().cfs_hip_debug_symeig(m, a.ctypes.data_as(dp), w.ctypes.data_as(dp), s.ctypes.data_as(dp)))
    return w, s


def tridiagonal(m, seed):
    """diagonal i + uniform(-0.25, 0.25), off-diagonal uniform(0.05, 0.2): by Gershgorin the eigenvalues lie in disjoint
    intervals around 0 .. m - 1, at least 0.1 apart"""
    rng = np.random.default_rng(seed)
    T = np.diag(np.arange(m) + rng.uniform(-0.25, 0.25, m))
    e = rng.uniform(0.05, 0.2, max(m - 1, 0))
    return T + np.diag(e, 1) + np.diag(e, -1)


def arrow(m, l, seed):
    """the projected matrix after a restart: l kept Ritz values on the diagonal, their arrow in row / column l, a
    tridiagonal tail.  Diagonal 2 i + noise, arrow entries of geometrically falling size (the converged pairs' are
    tiny), so the eigenvalues stay well apart"""
    rng = np.random.default_rng(seed)
    T = np.diag(2.0 * np.arange(m) + rng.uniform(-0.25, 0.25, m))
    T[:l, l] = T[l, :l] = rng.uniform(0.5, 1.0, l) * 0.5 ** np.arange(l)[::-1] * rng.choice([-1, 1], l)
    for i in range(l, m - 1):
        T[i, i + 1] = T[i + 1, i] = rng.uniform(0.05, 0.5)
    return T


CASES = [(f"tridiagonal{m}", lambda m=m: tridiagonal(m, m), True) for m in (1, 2, 3, 20, 128)] + \
        [(f"arrow{m}_{l}", lambda m=m, l=l: arrow(m, l, m), True) for m, l in ((20, 12), (128, 66))] + \
        [("repeated", lambda: np.diag([3.0, -1.0, 3.0, 0.0, -1.0, 3.0, 0.0, 5.0]), False)]


def _quality(T, w, s):
    """(r, o, the residual 2-norm of every pair over the norm of its vector), evaluated in long double so that the
    figures are those of the pairs and not of this evaluation"""
    T, w, s = (x.astype(np.longdouble) for x in (T, w, s))
    R = T @ s - s * w
    norms = np.sqrt(np.sum(R * R, axis=0)) / np.sqrt(np.sum(s * s, axis=0))
    return float(np.max(np.abs(R))), float(np.max(np.abs(s.T @ s - np.eye(len(w))))), norms.astype(np.float64)


@pytest.mark.parametrize("name,make,distinct", CASES, ids=[c[0] for c in CASES])
def test_symeig_against_numpy(name, make, distinct):
    T = make()
    m = T.shape[0]
    assert np.array_equal(T, T.T)
    wn, sn = np.linalg.eigh(T)
    w, s = _symeig(T)
    rn, on, res_n = _quality(T, wn, sn)
    r, o, res = _quality(T, w, s)
    slack = 8 * 2.0 ** -53 * float(np.max(np.sum(np.abs(T), axis=1)))
    print(f"symeig {name}: residual {r:.3e} (numpy {rn:.3e}), orthogonality {o:.3e} (numpy {on:.3e}), slack {slack:.3e}, "
          f"max |w - numpy| {np.max(np.abs(w - wn)):.3e}")
    assert np.all(np.diff(w) >= 0), "ascending"
    assert r <= 8 * rn + slack and o <= 8 * on + slack
    bound = res + res_n
    if distinct and m > 1:
        # the gaps exceed the bound, so eigenvalue i of one is eigenvalue i of the other
        assert np.min(np.diff(wn)) > np.max(bound[:-1] + bound[1:])
    assert np.all(np.abs(w - wn) <= bound + slack * (not distinct))


def test_symeig_reads_the_upper_triangle_of_a_row_major_matrix_and_returns_columns():
    T = arrow(7, 3, 1)
    w, s = _symeig(np.triu(T))  # the lower triangle is not looked at
    wn = np.linalg.eigvalsh(T)
    assert np.max(np.abs(w - wn)) <= 1e-13 * np.max(np.abs(wn))
    assert np.max(np.abs(T @ s[:, 2] - w[2] * s[:, 2])) <= 1e-13 * np.max(np.abs(wn))


def test_symeig_refuses_bad_sizes():
    lib = cfs.load()
    dp = C.POINTER(C.c_double)
    a = np.zeros((130, 130))
    w, s = np.full(130, 7.0), np.full((130, 130), 7.0)
    for m in (0, -1, 129):
        assert lib.cfs_hip_debug_symeig(m, a.ctypes.data_as(dp), w.ctypes.data_as(dp), s.ctypes.data_as(dp)) == _lib.ERR_ARG
    assert np.all(w == 7.0) and np.all(s == 7.0)
    assert lib.cfs_hip_debug_symeig(3, None, w.ctypes.data_as(dp), s.ctypes.data_as(dp)) == _lib.ERR_ARG
