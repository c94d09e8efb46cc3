"""cfs_hip_sym_lobpcg and its developer entry points without a GPU: the header declares them with the documented
signatures, the library exports them, the ctypes bindings' argument types match the declarations, the Python mirror is
there, the argument checks that need no device answer before anything touches one -- and the Rayleigh-Ritz step of the
iteration (cfs_hip_debug_lobpcg_rr), which runs on the host, against scipy.linalg.eigh(H, G).

The entry points are additions: CFS_HIP_ABI_VERSION stays where the library's other tests pin it, and callers detect
them by their symbols, as they do for the other solver entry points.

cfs_hip_debug_lobpcg_rr: G = S^T S and H = S^T A S of a random S in R^(200 x m) and a fixed SPD A.  Both sides' pairs
(theta_i, c_i) are evaluated in long double (_quality).  The library is allowed 8 x scipy's own figures for |C^T G C - I|
and for the off-diagonal of C^T H C, plus 8 * 2^-53 * ||H||inf, and theta_i may differ from scipy's by the sum of the two
sides' residual norms of pair i.  The norm is ||H c - theta G c|| in the G^-1 norm: with c^T G c = 1 to rounding it bounds
the distance of theta to an eigenvalue of the pencil (H, G), and _quality evaluates exactly that, through a Cholesky
factor of G written out in long double.  That pairs the eigenvalues by index only where the gaps exceed the sum, which
the test asserts from scipy's spectrum."""
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
    "cfs_hip_sym_lobpcg": ["cfs_hip_sym_t h", "int k", "int block_rows", "double tol", "double scale", "int maxiter",
                           "const void *x0_dev", "long long ld0", "double *eigenvalues", "void *vectors_dev", "long long ld",
                           "double *residuals", "int *nconv", "int *iterations", "int *products", "void *stream"],
    "cfs_hip_debug_lobpcg_rr": ["int m", "const double *g", "const double *hh", "int k", "double drop", "double *theta",
                                "double *c", "int *rank"],
    "cfs_hip_debug_gram": ["const void *s_dev", "const void *t_dev", "long long ld", "long long n", "int m", "int value_bytes",
                           "double *g", "double *hh", "void *stream"],
    "cfs_hip_sym_debug_lobpcg": ["cfs_hip_sym_t h", "int k", "int block_rows", "const void *x0_dev", "long long ld0", "int iters",
                                 "double *theta", "void *vectors_dev", "long long ld", "double *resnorms", "void *stream"],
    "cfs_hip_debug_lobpcg_update": ["void *s_dev", "long long ld", "long long n", "int k", "int m", "const double *c",
                                    "int value_bytes", "void *stream"],
    "cfs_hip_debug_gram_cols": ["const void *s_dev", "const void *t_dev", "long long ld", "long long n", "int m", "const int *idx",
                                "int full_h", "int value_bytes", "double *g", "double *hh", "void *stream"],
    "cfs_hip_debug_lobpcg_update_cols": ["void *s_dev", "void *as_dev", "long long ld", "long long n", "int k", "int m",
                                         "const int *idx", "int with_p", "const double *c", "int value_bytes", "void *stream"],
    "cfs_hip_sym_debug_lobpcg_residual": ["cfs_hip_sym_t h", "int block_rows", "const void *x_dev", "const void *ax_dev", "void *w_dev",
                                          "long long ld", "int k", "const double *theta", "unsigned active", "double *sums",
                                          "void *stream"],
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
    # appended behind cfs_hip_debug_symeig
    assert code.index("cfs_hip_debug_symeig") < m.start()
    assert name in _lib.SYMBOLS
    getattr(C.CDLL(cfs.lib_path()), name)  # dlsym
    lib = cfs.load()
    assert int(re.search(r"#define\s+CFS_HIP_ABI_VERSION\s+(\d+)\b", code).group(1)) == 4
    assert lib.cfs_hip_abi_version() == 4
    vp, ip, dp = C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_double)
    ctype = {"cfs_hip_sym_t": vp, "void *": vp, "const void *": vp, "int": C.c_int, "double": C.c_double, "int *": ip,
             "double *": dp, "const double *": dp, "long long": C.c_longlong, "const int *": ip, "unsigned": C.c_uint}
    declared = [ctype[re.sub(r"\w+$", "", p).strip()] for p in params]
    assert getattr(lib, name).argtypes == declared


def test_the_constant():
    assert int(re.search(r"#define\s+CFS_HIP_LOBPCG_MAX_K\s+(\d+)\b", _header()).group(1)) == 16 == _lib.LOBPCG_MAX_K


def test_the_python_mirror():
    from cfs_spmv_amd import solver
    p = inspect.signature(cfs.SymMatrix.lobpcg).parameters
    assert list(p) == ["self", "k", "precond", "block", "tol", "scale", "maxiter", "x0", "stream"]
    assert [p[k].default for k in list(p)[1:]] == [6, "jacobi", 3, 1e-10, None, 500, None, None]
    for f in (solver.lobpcg, solver.lobpcg_native):
        p = inspect.signature(f).parameters
        assert list(p)[:2] == ["A", "k"] and p["precond"].default == "jacobi" and p["block"].default == 3
        assert p["tol"].default == 1e-10 and p["scale"].default is None and p["maxiter"].default == 500


def _call(lib, h, k=4, block_rows=1, tol=1e-8, scale=1.0, maxiter=10, x0=None, ld0=0, w=True, x=C.c_void_p(0x4000), ld=1 << 20):
    vals = (C.c_double * 16)(*([7.0] * 16))
    res = (C.c_double * 16)(*([7.0] * 16))
    nconv, iterations, products = C.c_int(7), C.c_int(7), C.c_int(7)
    rc = lib.cfs_hip_sym_lobpcg(h, k, block_rows, tol, scale, maxiter, x0, ld0, vals if w else None, x, ld, res, C.byref(nconv),
                                C.byref(iterations), C.byref(products), None)
    return rc, (nconv.value, iterations.value, products.value), list(vals) + list(res)


def test_null_arguments_are_refused_first():
    lib = cfs.load()
    bound = lib.cfs_hip_runtime_bound()
    h = C.c_void_p(0x1000)
    for k in (4, 0, 17):
        for block_rows in (1, 5, -1):
            for hh, w, x in ((None, True, h), (h, False, h), (h, True, None), (None, False, None)):
                rc, counters, out = _call(lib, hh, k=k, block_rows=block_rows, tol=-1.0, w=w, x=x)
                assert rc == _lib.ERR_ARG and b"null" in lib.cfs_hip_last_error(), (k, block_rows, hh, w, x)
                assert counters == (7, 7, 7) and out == [7.0] * 32
    t, r = (C.c_double * 16)(*([7.0] * 16)), (C.c_double * 16)(*([7.0] * 16))
    for args in ((None, 4, 1, None, 0, 2, t, h, 1 << 20, r), (h, 4, 1, None, 0, 2, None, h, 1 << 20, r),
                 (h, 4, 1, None, 0, 2, t, None, 1 << 20, r), (h, 4, 1, None, 0, 2, t, h, 1 << 20, None)):
        assert lib.cfs_hip_sym_debug_lobpcg(*args, None) == _lib.ERR_ARG and b"null" in lib.cfs_hip_last_error()
    g = (C.c_double * 4)()
    assert lib.cfs_hip_debug_gram(None, h, 16, 16, 2, 8, g, g, None) == _lib.ERR_ARG and b"null" in lib.cfs_hip_last_error()
    assert lib.cfs_hip_debug_gram(h, h, 16, 16, 2, 8, None, g, None) == _lib.ERR_ARG and b"null" in lib.cfs_hip_last_error()
    assert lib.cfs_hip_debug_lobpcg_update(None, 16, 16, 1, 2, g, 8, None) == _lib.ERR_ARG and b"null" in lib.cfs_hip_last_error()
    assert list(t) == [7.0] * 16 and list(r) == [7.0] * 16
    assert lib.cfs_hip_runtime_bound() == bound  # nothing above initialised the runtime


def test_checks_that_need_no_device_answer_before_the_handle_is_looked_at():
    lib = cfs.load()
    bound = lib.cfs_hip_runtime_bound()
    # (a non-null handle that is never dereferenced: the checks of the other arguments come first)
    h = C.c_void_p(0x1000)

    def refused(word, **kw):
        rc, counters, out = _call(lib, h, **kw)
        msg = lib.cfs_hip_last_error()
        assert rc == _lib.ERR_ARG and word in msg, (kw, rc, msg)
        assert counters == (0, 0, 0) and out == [7.0] * 32, kw  # the counters zeroed, nothing else written
        return msg
    # in the documented order: every later argument is bad as well
    bad = dict(block_rows=5, tol=-1.0, scale=0.0, maxiter=-1, x0=C.c_void_p(0x3008))
    for k in (0, -1, 17, 1 << 20):
        refused(b"bad k", k=k, **bad)
    del bad["block_rows"]
    for block_rows in (5, 7, 8, -1, 12):
        refused(b"block_rows", block_rows=block_rows, **bad)
    del bad["tol"], bad["scale"], bad["maxiter"]
    for kw in (dict(tol=-1e-3), dict(tol=float("nan")), dict(scale=0.0), dict(scale=-1.0), dict(scale=float("inf")),
               dict(scale=float("nan")), dict(maxiter=-1)):
        refused(b"tolerance", **kw, **bad)
    refused(b"16-byte aligned", x0=C.c_void_p(0x3008), ld0=1 << 20)
    refused(b"16-byte aligned", x=C.c_void_p(0x4004))
    t, r = (C.c_double * 16)(*([7.0] * 16)), (C.c_double * 16)(*([7.0] * 16))
    for k, block_rows, iters, x, word in ((0, 1, 2, 0x4000, b"bad k"), (17, 1, 2, 0x4000, b"bad k"), (4, 5, 2, 0x4000, b"block_rows"),
                                          (4, 1, -1, 0x4000, b"tolerance"), (4, 1, 2, 0x4008, b"16-byte aligned")):
        assert lib.cfs_hip_sym_debug_lobpcg(h, k, block_rows, None, 0, iters, t, C.c_void_p(x), 1 << 20, r, None) == _lib.ERR_ARG
        assert word in lib.cfs_hip_last_error()
    assert list(t) == [7.0] * 16 and list(r) == [7.0] * 16
    # the two kernel-level entry points: sizes, then alignment, before a pointer is classified
    g = (C.c_double * 4)()
    p = C.c_void_p(0x4000)
    for m in (0, -1, 49):
        assert lib.cfs_hip_debug_gram(p, p, 16, 16, m, 8, g, g, None) == _lib.ERR_ARG and b"m must lie" in lib.cfs_hip_last_error()
    for ld, n, vb, s in ((16, 16, 2, p), (15, 16, 8, p), (17, 17, 8, p), (16, 0, 8, p), (16, 16, 8, C.c_void_p(0x4008))):
        assert lib.cfs_hip_debug_gram(s, p, ld, n, 2, vb, g, g, None) == _lib.ERR_ARG
        assert lib.cfs_hip_debug_lobpcg_update(s, ld, n, 1, 2, g, vb, None) == _lib.ERR_ARG
    for k, m in ((0, 1), (17, 3), (2, 7), (2, 0)):
        assert lib.cfs_hip_debug_lobpcg_update(p, 16, 16, k, m, g, 8, None) == _lib.ERR_ARG and b"3 k" in lib.cfs_hip_last_error()
    assert lib.cfs_hip_runtime_bound() == bound  # nothing above initialised the runtime


def test_the_kernel_forms_refuse_in_the_documented_order():
    """cfs_hip_debug_gram_cols, cfs_hip_debug_lobpcg_update_cols, cfs_hip_sym_debug_lobpcg_residual: a null pointer, the
    sizes (an index out of range among them), value_bytes, alignment and ld, each with every later argument bad as well,
    before a pointer is classified or the handle is looked at; nothing is written"""
    lib = cfs.load()
    bound = lib.cfs_hip_runtime_bound()
    g, hh = (C.c_double * 9)(*([7.0] * 9)), (C.c_double * 9)(*([7.0] * 9))
    p, odd = C.c_void_p(0x4000), C.c_void_p(0x4008)
    ints = lambda *v: (C.c_int * len(v))(*v)
    ok = ints(0, 2, 5)

    def refused(f, word, *args):
        assert f(*args, None) == _lib.ERR_ARG, (f.__name__, args)
        assert word in lib.cfs_hip_last_error(), (f.__name__, args, lib.cfs_hip_last_error())
    gram = lib.cfs_hip_debug_gram_cols
    for s, t, idx, a, b in ((None, p, ok, g, hh), (p, None, ok, g, hh), (p, p, None, g, hh), (p, p, ok, None, hh), (p, p, ok, g, None)):
        refused(gram, b"null", s, t, 15, 16, 49, idx, 2, 3, a, b)
    for m in (0, -1, 49):
        refused(gram, b"m must lie", odd, p, 15, 16, m, ints(48, 0, 0), 2, 3, g, hh)
    for idx in (ints(0, 48, 1), ints(0, 1, -1), ints(1 << 20, 0, 0)):
        refused(gram, b"is not a column", odd, p, 15, 16, 3, idx, 2, 3, g, hh)
    for full_h in (2, -1):
        refused(gram, b"full_h", odd, p, 15, 16, 3, ok, full_h, 3, g, hh)
    refused(gram, b"value_bytes", odd, p, 15, 16, 3, ok, 0, 3, g, hh)
    for s, t, ld, n in ((odd, p, 16, 16), (p, odd, 16, 16), (p, p, 15, 16), (p, p, 17, 17), (p, p, 16, 0), (p, p, 1 << 60, 16)):
        refused(gram, b"multiples of 16 bytes", s, t, ld, n, 3, ok, 0, 8, g, hh)
    assert list(g) == [7.0] * 9 and list(hh) == [7.0] * 9

    upd = lib.cfs_hip_debug_lobpcg_update_cols
    for s, idx, c in ((None, ok, g), (p, None, g), (p, ok, None)):
        refused(upd, b"null", s, odd, 15, 16, 0, 3, idx, 2, c, 3)
    for k, m in ((0, 1), (17, 3), (2, 7), (2, 0)):
        refused(upd, b"3 k", odd, odd, 15, 16, k, m, ints(48, 0, 0), 2, g, 3)
    for k, idx in ((1, ints(0, 3, 1)), (2, ints(0, 6, 1)), (16, ints(48, 0, 0)), (2, ints(0, 1, -1))):
        refused(upd, b"is not a column", odd, odd, 15, 16, k, 3, idx, 2, g, 3)
    for with_p in (2, -1):
        refused(upd, b"with_p", odd, odd, 15, 16, 2, 3, ok, with_p, g, 3)
    refused(upd, b"value_bytes", odd, odd, 15, 16, 2, 3, ok, 1, g, 3)
    for s, a, ld, n in ((odd, None, 16, 16), (p, odd, 16, 16), (p, None, 15, 16), (p, None, 17, 17), (p, None, 16, 0), (p, p, 1 << 60, 16)):
        refused(upd, b"multiples of 16 bytes", s, a, ld, n, 2, 3, ok, 1, g, 8)
    for a in (0x4000, 0x4000 + 8 * (5 * 16 + 14), 0x4000 - 8 * (5 * 16 + 14)):  # (a block: 5 ld + n = 96 values of 8 bytes)
        refused(upd, b"overlap", p, C.c_void_p(a), 16, 16, 2, 3, ok, 1, g, 8)

    res = lib.cfs_hip_sym_debug_lobpcg_residual
    h = C.c_void_p(0x1000)  # (never dereferenced: the checks of the other arguments come first)
    th, sums = (C.c_double * 16)(*([0.5] * 16)), (C.c_double * 32)(*([7.0] * 32))
    for hh_, x, ax, w, t, s in ((None, p, p, p, th, sums), (h, None, p, p, th, sums), (h, p, None, p, th, sums), (h, p, p, None, th, sums),
                                (h, p, p, p, None, sums), (h, p, p, p, th, None)):
        refused(res, b"null", hh_, 5, x, ax, w, 1, 0, t, 1, s)
    for k in (0, -1, 17):
        refused(res, b"bad k", h, 5, odd, p, p, 1, k, th, 1 << 20, sums)
    for block_rows in (5, 7, 8, -1, 12):
        refused(res, b"block_rows", h, block_rows, odd, p, p, 1, 4, th, 1 << 4, sums)
    for k, active in ((4, 1 << 4), (4, 0xffffffff), (1, 2), (15, 1 << 15), (16, 1 << 16)):
        refused(res, b"active", h, 1, odd, p, p, 1, k, th, active, sums)
    for x, ax, w in ((odd, p, p), (p, odd, p), (p, p, odd)):
        refused(res, b"16-byte aligned", h, 1, x, ax, w, 1, 4, th, 0xf, sums)
    assert list(sums) == [7.0] * 32
    assert lib.cfs_hip_runtime_bound() == bound  # nothing above initialised the runtime


# ---- cfs_hip_debug_lobpcg_rr --------------------------------------------------------------------------------------
DROP = 64 * 2.0 ** -53
N = 200


def _rr(G, H, k, drop=DROP):
    m = G.shape[0]
    g, hh = np.ascontiguousarray(G, np.float64), np.ascontiguousarray(H, np.float64)
    theta, c, rank = np.full(k, 7.0), np.full((m, k), 7.0), C.c_int(-1)
    dp = C.POINTER(C.c_double)
    _lib.check(cfs.load().cfs_hip_debug_lobpcg_rr(m, g.ctypes.data_as(dp), hh.ctypes.data_as(dp), k, drop, theta.ctypes.data_as(dp),
                                                  c.ctypes.data_as(dp), C.byref(rank)))
    return theta, c, rank.value


def _spd():
    """a fixed SPD A: Q diag(1 .. 50, spaced geometrically) Q^T with Q from the QR of a seeded Gaussian"""
    rng = np.random.default_rng(12345)
    Q = np.linalg.qr(rng.standard_normal((N, N)))[0]
    A = (Q * np.geomspace(1.0, 50.0, N)) @ Q.T
    return 0.5 * (A + A.T)


def _pencil(m, seed=None):
    S = np.random.default_rng(m if seed is None else seed).standard_normal((N, m))
    return S, S.T @ S, S.T @ _spd() @ S


def _quality(G, H, theta, Cm):
    """(max |C^T G C - I|, max off-diagonal |C^T H C|, per pair ||L^-1 (H c - theta G c)||_2 with G = L L^T), in long
    double, G and H symmetrised from their upper triangles as the library reads them"""
    ld = np.longdouble
    G, H = (np.triu(M) + np.triu(M, 1).T for M in (G.astype(ld), H.astype(ld)))
    Cm, theta = Cm.astype(ld), theta.astype(ld)
    k = Cm.shape[1]
    o = float(np.max(np.abs(Cm.T @ G @ Cm - np.eye(k))))
    T = Cm.T @ H @ Cm
    off = float(np.max(np.abs(T - np.diag(np.diag(T))))) if k > 1 else 0.0
    R = H @ Cm - (G @ Cm) * theta
    # ||L^-1 r||^2 = r^T G^-1 r; solved in long double by Cholesky written out (numpy has no long-double solver)
    m = G.shape[0]
    L = np.zeros((m, m), ld)
    for j in range(m):
        L[j, j] = np.sqrt(G[j, j] - np.dot(L[j, :j], L[j, :j]))
        for i in range(j + 1, m):
            L[i, j] = (G[i, j] - np.dot(L[i, :j], L[j, :j])) / L[j, j]
    Y = np.zeros_like(R)
    for i in range(m):
        Y[i] = (R[i] - L[i, :i] @ Y[:i]) / L[i, i]
    return o, off, np.sqrt(np.sum(Y * Y, axis=0)).astype(np.float64)


@pytest.mark.parametrize("m", [1, 2, 3, 12, 48])
def test_rr_against_scipy(m):
    import scipy.linalg
    S, G, H = _pencil(m)
    k = min(m, 16)
    ws, Vs = scipy.linalg.eigh(H, G)
    theta, Cm, rank = _rr(G, H, k)
    assert rank == m and np.all(np.diff(theta) >= 0), "all columns kept, ascending"
    on, offn, res_n = _quality(G, H, ws[:k], Vs[:, :k])
    o, off, res = _quality(G, H, theta, Cm)
    slack = 8 * 2.0 ** -53 * float(np.max(np.sum(np.abs(H), axis=1)))
    print(f"lobpcg_rr m={m}: |C^T G C - I| {o:.3e} (scipy {on:.3e}), off-diagonal of C^T H C {off:.3e} (scipy {offn:.3e}), slack "
          f"{slack:.3e}, max |theta - scipy| {np.max(np.abs(theta - ws[:k])):.3e}, residuals {np.max(res):.3e} (scipy {np.max(res_n):.3e})")
    assert o <= 8 * on + slack and off <= 8 * offn + slack
    bound = res + res_n
    if m > 1:  # the gaps exceed the bound, so eigenvalue i of one is eigenvalue i of the other
        assert np.min(np.diff(ws)) > np.max(bound) * 2
    assert np.all(np.abs(theta - ws[:k]) <= bound)


@pytest.mark.parametrize("kind", ["duplicated", "zero"])
@pytest.mark.parametrize("m", [3, 12, 48])
def test_rr_drops_a_dependent_column(m, kind):
    """column m - 2 a copy of column 0, or zero: rank m - 1, and theta the spectrum of the pencil on the reduced space
    (S without that column), within the same bound; every output finite, the dropped zero column's row of C zero"""
    import scipy.linalg
    S = _pencil(m)[0].copy()
    j = m - 2
    S[:, j] = S[:, 0] if kind == "duplicated" else 0.0
    A = _spd()
    G, H = S.T @ S, S.T @ A @ S
    k = min(m - 1, 16)
    theta, Cm, rank = _rr(G, H, k)
    assert rank == m - 1
    assert np.all(np.isfinite(theta)) and np.all(np.isfinite(Cm))
    if kind == "zero":
        assert not Cm[j].any()
    keep = [i for i in range(m) if i != j]
    Gr, Hr = G[np.ix_(keep, keep)], H[np.ix_(keep, keep)]
    ws, Vs = scipy.linalg.eigh(Hr, Gr)
    # the library's pairs restated on the reduced basis: a copy's coefficient is added to the original's
    Cr = Cm[keep].copy()
    if kind == "duplicated":
        Cr[0] += Cm[j]
    o, off, res = _quality(Gr, Hr, theta, Cr)
    on, offn, res_n = _quality(Gr, Hr, ws[:k], Vs[:, :k])
    slack = 8 * 2.0 ** -53 * float(np.max(np.sum(np.abs(H), axis=1)))
    print(f"lobpcg_rr m={m} {kind}: |C^T G C - I| {o:.3e} (scipy {on:.3e}), off-diagonal {off:.3e} (scipy {offn:.3e}), "
          f"max |theta - scipy| {np.max(np.abs(theta - ws[:k])):.3e}, residuals {np.max(res):.3e} (scipy {np.max(res_n):.3e})")
    assert o <= 8 * on + slack and off <= 8 * offn + slack
    assert np.all(np.abs(theta - ws[:k]) <= res + res_n)


def test_rr_reads_the_upper_triangles_and_zero_fills_beyond_the_rank():
    S, G, H = _pencil(5)
    a = _rr(G, H, 3)
    b = _rr(np.triu(G), np.triu(H), 3)  # the lower triangles are not looked at
    assert all(np.array_equal(x, y) for x, y in zip(a[:2], b[:2])) and a[2] == b[2] == 5
    S[:, 1] = S[:, 3] = 0.0
    theta, Cm, rank = _rr(S.T @ S, S.T @ _spd() @ S, 4)
    assert rank == 3 and theta[3] == 0.0 and not Cm[:, 3].any() and Cm[:, :3].any(axis=0).all()
    # a matrix of zeros: rank 0, zero outputs
    theta, Cm, rank = _rr(np.zeros((4, 4)), np.zeros((4, 4)), 2)
    assert rank == 0 and not theta.any() and not Cm.any()


def test_rr_refuses_bad_sizes():
    lib = cfs.load()
    dp = C.POINTER(C.c_double)
    g = np.eye(50)
    theta, c, rank = np.full(50, 7.0), np.full((50, 50), 7.0), C.c_int(7)
    args = lambda m, k, drop=DROP: (m, g.ctypes.data_as(dp), g.ctypes.data_as(dp), k, drop, theta.ctypes.data_as(dp),
                                    c.ctypes.data_as(dp), C.byref(rank))
    for m, k in ((0, 1), (-1, 1), (49, 4), (12, 0), (12, -1), (48, 17), (3, 4)):
        assert lib.cfs_hip_debug_lobpcg_rr(*args(m, k)) == _lib.ERR_ARG, (m, k)
    for drop in (-1.0, 1.0, float("nan")):
        assert lib.cfs_hip_debug_lobpcg_rr(*args(4, 2, drop)) == _lib.ERR_ARG
    assert np.all(theta == 7.0) and np.all(c == 7.0) and rank.value == 7
    assert lib.cfs_hip_debug_lobpcg_rr(3, None, g.ctypes.data_as(dp), 1, DROP, theta.ctypes.data_as(dp), c.ctypes.data_as(dp),
                                       C.byref(rank)) == _lib.ERR_ARG
    nan = np.eye(3)
    nan[0, 1] = np.nan
    assert lib.cfs_hip_debug_lobpcg_rr(3, nan.ctypes.data_as(dp), g.ctypes.data_as(dp), 1, DROP, theta.ctypes.data_as(dp),
                                       c.ctypes.data_as(dp), C.byref(rank)) == _lib.ERR_INTERNAL
