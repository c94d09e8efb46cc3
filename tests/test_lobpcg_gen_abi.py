"""The pencil forms of LOBPCG -- cfs_hip_sym_lobpcg_gen, _lobpcg_gen_amg, _debug_lobpcg_gen, cfs_hip_debug_gram3_cols,
cfs_hip_debug_lobpcg_update3_cols, cfs_hip_sym_debug_lobpcg_residual_gen -- without a GPU, by the method of
test_lobpcg_abi.py: the header declares them with the documented signatures, the library exports them, the ctypes
bindings' argument types match the declarations, the null-pointer refusals and the checks that need no device answer
before a handle is dereferenced or the runtime initialised, and the Python mirror raises its ValueErrors before any
device work.

The entry points are additions: CFS_HIP_ABI_VERSION stays at 4 and callers detect them by their symbols."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

import cfs_spmv_amd as cfs
from cfs_spmv_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_TAIL = ["const void *x0_dev", "long long ld0", "double *eigenvalues", "void *vectors_dev", "long long ld", "double *residuals",
         "int *nconv", "int *iterations", "int *products", "int *b_products", "void *stream"]
SIGNATURES = {
    "cfs_hip_sym_lobpcg_gen": ["cfs_hip_sym_t h", "cfs_hip_sym_t hb", "int k", "int block_rows", "double tol", "double scale",
                               "int maxiter"] + _TAIL,
    "cfs_hip_sym_lobpcg_gen_amg": ["cfs_hip_sym_t h", "cfs_hip_sym_t hb", "cfs_hip_amg_t a", "int k", "double tol", "double scale",
                                   "int maxiter"] + _TAIL,
    "cfs_hip_sym_debug_lobpcg_gen": ["cfs_hip_sym_t h", "cfs_hip_sym_t hb", "int k", "int block_rows", "const void *x0_dev",
                                     "long long ld0", "int iters", "double *theta", "void *vectors_dev", "long long ld",
                                     "double *resnorms", "void *stream"],
    "cfs_hip_debug_gram3_cols": ["const void *s_dev", "const void *as_dev", "const void *bs_dev", "long long ld", "long long n", "int m",
                                 "const int *idx", "int value_bytes", "double *g", "double *hh", "void *stream"],
    "cfs_hip_debug_lobpcg_update3_cols": ["void *s_dev", "void *as_dev", "void *bs_dev", "long long ld", "long long n", "int k", "int m",
                                          "const int *idx", "int with_p", "const double *c", "int value_bytes", "void *stream"],
    "cfs_hip_sym_debug_lobpcg_residual_gen": ["cfs_hip_sym_t h", "int block_rows", "const void *x_dev", "const void *ax_dev",
                                              "const void *bx_dev", "void *w_dev", "long long ld", "int k", "const double *theta",
                                              "unsigned active", "double *sums", "void *stream"],
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
    assert name in _lib.SYMBOLS
    getattr(C.CDLL(cfs.lib_path()), name)  # dlsym
    lib = cfs.load()
    assert int(re.search(r"#define\s+CFS_HIP_ABI_VERSION\s+(\d+)\b", code).group(1)) == 4
    assert lib.cfs_hip_abi_version() == 4
    vp, ip, dp = C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_double)
    ctype = {"cfs_hip_sym_t": vp, "cfs_hip_amg_t": vp, "void *": vp, "const void *": vp, "int": C.c_int, "double": C.c_double,
             "int *": ip, "double *": dp, "const double *": dp, "long long": C.c_longlong, "const int *": ip, "unsigned": C.c_uint}
    declared = [ctype[re.sub(r"\w+$", "", p).strip()] for p in params]
    assert getattr(lib, name).argtypes == declared


def test_the_python_mirror():
    from cfs_spmv_amd import solver
    # SymMatrix.lobpcg keeps the argument list test_lobpcg_abi.py pins; the pencil is a method of its own with B in front
    p = inspect.signature(cfs.SymMatrix.lobpcg).parameters
    q = inspect.signature(cfs.SymMatrix.lobpcg_gen).parameters
    assert list(q) == ["self", "B"] + list(p)[1:] and q["B"].default is inspect.Parameter.empty
    assert [q[k].default for k in list(q)[2:]] == [p[k].default for k in list(p)[1:]]
    for f in (solver.lobpcg, solver.lobpcg_native, cfs.SymMatrix.debug_lobpcg):
        p = inspect.signature(f).parameters
        assert list(p)[-1] == "B" and p["B"].default is None


def _shell(n, dtype):
    """a SymMatrix that holds no handle: n and dtype are all the ValueErrors look at"""
    A = object.__new__(cfs.SymMatrix)
    A.n, A.dtype = n, np.dtype(dtype)
    return A


def test_the_value_errors_come_before_any_device_work():
    from cfs_spmv_amd import solver
    lib = cfs.load()
    bound = lib.cfs_hip_runtime_bound()
    A = _shell(240, np.float64)
    calls = [lambda B: A.lobpcg_gen(B, k=4, scale=1.0), lambda B: A.debug_lobpcg(4, 1, 2, B=B), lambda B: solver.lobpcg(A, 4, scale=1.0, B=B),
             lambda B: solver.lobpcg_native(A, 4, scale=1.0, B=B), lambda B: solver.lobpcg(A, 4, iters=2, B=B)]
    for call in calls:
        for B in (np.ones(240), 1.0, "M", [1.0] * 240):
            with pytest.raises(ValueError, match="B must be a SymMatrix"):
                call(B)
        with pytest.raises(ValueError, match="the n and the dtype of A"):
            call(_shell(239, np.float64))
        with pytest.raises(ValueError, match="the n and the dtype of A"):
            call(_shell(240, np.float32))
    assert lib.cfs_hip_runtime_bound() == bound  # nothing above initialised the runtime


def _gen(lib, h, hb, k=4, block_rows=1, tol=1e-8, scale=1.0, maxiter=10, x0=None, ld0=0, w=True, x=C.c_void_p(0x4000), ld=1 << 20, a=False):
    vals = (C.c_double * 16)(*([7.0] * 16))
    res = (C.c_double * 16)(*([7.0] * 16))
    cnt = [C.c_int(7) for _ in range(4)]
    tail = (tol, scale, maxiter, x0, ld0, vals if w else None, x, ld, res, *(C.byref(c) for c in cnt), None)
    if a is False:
        rc = lib.cfs_hip_sym_lobpcg_gen(h, hb, k, block_rows, *tail)
    else:
        rc = lib.cfs_hip_sym_lobpcg_gen_amg(h, hb, a, k, *tail)
    return rc, tuple(c.value for c in cnt), list(vals) + list(res)


def test_null_arguments_are_refused_first():
    lib = cfs.load()
    bound = lib.cfs_hip_runtime_bound()
    h = C.c_void_p(0x1000)
    for k in (4, 0, 17):
        for block_rows in (1, 5):
            for hh, hb, w, x in ((None, h, True, h), (h, None, True, h), (h, h, False, h), (h, h, True, None), (None, None, False, None)):
                rc, counters, out = _gen(lib, hh, hb, k=k, block_rows=block_rows, tol=-1.0, w=w, x=x)
                assert rc == _lib.ERR_ARG and b"null" in lib.cfs_hip_last_error(), (k, block_rows, hh, hb, w, x)
                assert counters == (7, 7, 7, 7) and out == [7.0] * 32
        for hh, hb, a, w, x in ((None, h, h, True, h), (h, None, h, True, h), (h, h, None, True, h), (h, h, h, False, h), (h, h, h, True, None)):
            rc, counters, out = _gen(lib, hh, hb, k=k, tol=-1.0, w=w, x=x, a=a)
            assert rc == _lib.ERR_ARG and b"null" in lib.cfs_hip_last_error(), (k, hh, hb, a, w, x)
            assert counters == (7, 7, 7, 7) and out == [7.0] * 32
    t, r = (C.c_double * 16)(*([7.0] * 16)), (C.c_double * 16)(*([7.0] * 16))
    for args in ((None, h, 4, 1, None, 0, 2, t, h, 1 << 20, r), (h, None, 4, 1, None, 0, 2, t, h, 1 << 20, r),
                 (h, h, 4, 1, None, 0, 2, None, h, 1 << 20, r), (h, h, 4, 1, None, 0, 2, t, None, 1 << 20, r),
                 (h, h, 4, 1, None, 0, 2, t, h, 1 << 20, None)):
        assert lib.cfs_hip_sym_debug_lobpcg_gen(*args, None) == _lib.ERR_ARG and b"null" in lib.cfs_hip_last_error()
    assert list(t) == [7.0] * 16 and list(r) == [7.0] * 16
    g, hh_ = (C.c_double * 9)(*([7.0] * 9)), (C.c_double * 9)(*([7.0] * 9))
    p = C.c_void_p(0x4000)
    ok = (C.c_int * 3)(0, 2, 5)
    for s, a, b, idx, gg, hg in ((None, p, p, ok, g, hh_), (p, None, p, ok, g, hh_), (p, p, None, ok, g, hh_), (p, p, p, None, g, hh_),
                                 (p, p, p, ok, None, hh_), (p, p, p, ok, g, None)):
        assert lib.cfs_hip_debug_gram3_cols(s, a, b, 15, 16, 49, idx, 3, gg, hg, None) == _lib.ERR_ARG
        assert b"null" in lib.cfs_hip_last_error()
    for s, a, b, idx, c in ((None, p, p, ok, g), (p, None, p, ok, g), (p, p, None, ok, g), (p, p, p, None, g), (p, p, p, ok, None)):
        assert lib.cfs_hip_debug_lobpcg_update3_cols(s, a, b, 15, 16, 0, 3, idx, 2, c, 3, None) == _lib.ERR_ARG
        assert b"null" in lib.cfs_hip_last_error()
    th, sums = (C.c_double * 16)(*([0.5] * 16)), (C.c_double * 32)(*([7.0] * 32))
    for hh2, x, ax, bx, w, t2, s2 in ((None, p, p, p, p, th, sums), (h, None, p, p, p, th, sums), (h, p, None, p, p, th, sums),
                                      (h, p, p, None, p, th, sums), (h, p, p, p, None, th, sums), (h, p, p, p, p, None, sums),
                                      (h, p, p, p, p, th, None)):
        assert lib.cfs_hip_sym_debug_lobpcg_residual_gen(hh2, 5, x, ax, bx, w, 1, 0, t2, 1, s2, None) == _lib.ERR_ARG
        assert b"null" in lib.cfs_hip_last_error()
    assert list(g) == [7.0] * 9 and list(hh_) == [7.0] * 9 and list(sums) == [7.0] * 32
    assert lib.cfs_hip_runtime_bound() == bound  # nothing above initialised the runtime


def test_checks_that_need_no_device_answer_before_the_handles_are_looked_at():
    """the order of cfs_hip_sym_lobpcg: every later argument is bad as well; the counters zeroed, nothing else written"""
    lib = cfs.load()
    bound = lib.cfs_hip_runtime_bound()
    h, hb, a = C.c_void_p(0x1000), C.c_void_p(0x2000), C.c_void_p(0x3000)  # (never dereferenced)

    def refused(word, **kw):
        rc, counters, out = _gen(lib, h, hb, **kw)
        msg = lib.cfs_hip_last_error()
        assert rc == _lib.ERR_ARG and word in msg, (kw, rc, msg)
        assert counters == (0, 0, 0, 0) and out == [7.0] * 32, kw
    for amg in (False, a):
        bad = dict(block_rows=5, tol=-1.0, scale=0.0, maxiter=-1, x0=C.c_void_p(0x3008), a=amg)
        for k in (0, -1, 17, 1 << 20):
            refused(b"bad k", k=k, **bad)
        del bad["block_rows"]
        if amg is False:
            for block_rows in (5, 7, 8, -1, 12):
                refused(b"block_rows", block_rows=block_rows, **bad)
        del bad["tol"], bad["scale"], bad["maxiter"]
        for kw in (dict(tol=-1e-3), dict(tol=float("nan")), dict(scale=0.0), dict(scale=-1.0), dict(scale=float("inf")),
                   dict(scale=float("nan")), dict(maxiter=-1)):
            refused(b"tolerance", **kw, **bad)
        refused(b"16-byte aligned", x0=C.c_void_p(0x3008), ld0=1 << 20, a=amg)
        refused(b"16-byte aligned", x=C.c_void_p(0x4004), a=amg)
    t, r = (C.c_double * 16)(*([7.0] * 16)), (C.c_double * 16)(*([7.0] * 16))
    for k, block_rows, iters, x, word in ((0, 1, 2, 0x4000, b"bad k"), (17, 1, 2, 0x4000, b"bad k"), (4, 5, 2, 0x4000, b"block_rows"),
                                          (4, 1, -1, 0x4000, b"tolerance"), (4, 1, 2, 0x4008, b"16-byte aligned")):
        assert lib.cfs_hip_sym_debug_lobpcg_gen(h, hb, k, block_rows, None, 0, iters, t, C.c_void_p(x), 1 << 20, r, None) == _lib.ERR_ARG
        assert word in lib.cfs_hip_last_error()
    assert list(t) == [7.0] * 16 and list(r) == [7.0] * 16
    assert lib.cfs_hip_runtime_bound() == bound  # nothing above initialised the runtime


def test_the_kernel_forms_refuse_in_the_documented_order():
    """the sizes (an index out of range among them), value_bytes, alignment and ld, an overlap -- each with every later
    argument bad as well, before a pointer is classified or the handle is looked at; nothing is written"""
    lib = cfs.load()
    bound = lib.cfs_hip_runtime_bound()
    g, hh = (C.c_double * 9)(*([7.0] * 9)), (C.c_double * 9)(*([7.0] * 9))
    p, odd = C.c_void_p(0x4000), C.c_void_p(0x4008)
    ints = lambda *v: (C.c_int * len(v))(*v)
    ok = ints(0, 2, 5)

    def refused(f, word, *args):
        assert f(*args, None) == _lib.ERR_ARG, (f.__name__, args)
        assert word in lib.cfs_hip_last_error(), (f.__name__, args, lib.cfs_hip_last_error())
    gram = lib.cfs_hip_debug_gram3_cols
    for m in (0, -1, 49):
        refused(gram, b"m must lie", odd, p, p, 15, 16, m, ints(48, 0, 0), 3, g, hh)
    for idx in (ints(0, 48, 1), ints(0, 1, -1), ints(1 << 20, 0, 0)):
        refused(gram, b"is not a column", odd, p, p, 15, 16, 3, idx, 3, g, hh)
    refused(gram, b"value_bytes", odd, p, p, 15, 16, 3, ok, 3, g, hh)
    for s, a, b, ld, n in ((odd, p, p, 16, 16), (p, odd, p, 16, 16), (p, p, odd, 16, 16), (p, p, p, 15, 16), (p, p, p, 17, 17),
                           (p, p, p, 16, 0), (p, p, p, 1 << 60, 16)):
        refused(gram, b"multiples of 16 bytes", s, a, b, ld, n, 3, ok, 8, g, hh)
    assert list(g) == [7.0] * 9 and list(hh) == [7.0] * 9

    upd = lib.cfs_hip_debug_lobpcg_update3_cols
    far, far2 = C.c_void_p(0x40000), C.c_void_p(0x80000)
    for k, m in ((0, 1), (17, 3), (2, 7), (2, 0)):
        refused(upd, b"3 k", odd, odd, odd, 15, 16, k, m, ints(48, 0, 0), 2, g, 3)
    for k, idx in ((1, ints(0, 3, 1)), (2, ints(0, 6, 1)), (16, ints(48, 0, 0)), (2, ints(0, 1, -1))):
        refused(upd, b"is not a column", odd, odd, odd, 15, 16, k, 3, idx, 2, g, 3)
    for with_p in (2, -1):
        refused(upd, b"with_p", odd, odd, odd, 15, 16, 2, 3, ok, with_p, g, 3)
    refused(upd, b"value_bytes", odd, odd, odd, 15, 16, 2, 3, ok, 1, g, 3)
    for s, a, b, ld, n in ((odd, far, far2, 16, 16), (p, odd, far2, 16, 16), (p, far, odd, 16, 16), (p, far, far2, 15, 16),
                           (p, far, far2, 17, 17), (p, far, far2, 16, 0), (p, p, p, 1 << 60, 16)):
        refused(upd, b"multiples of 16 bytes", s, a, b, ld, n, 2, 3, ok, 1, g, 8)
    edge = 8 * (5 * 16 + 14)  # (a block: 5 ld + n = 96 values of 8 bytes)
    for a, b in ((0x4000, 0x80000), (0x40000, 0x4000), (0x40000, 0x40000 + edge), (0x4000 + edge, 0x80000), (0x40000, 0x4000 - edge)):
        refused(upd, b"overlap", p, C.c_void_p(a), C.c_void_p(b), 16, 16, 2, 3, ok, 1, g, 8)

    res = lib.cfs_hip_sym_debug_lobpcg_residual_gen
    h = C.c_void_p(0x1000)  # (never dereferenced: the checks of the other arguments come first)
    th, sums = (C.c_double * 16)(*([0.5] * 16)), (C.c_double * 32)(*([7.0] * 32))
    for k in (0, -1, 17):
        refused(res, b"bad k", h, 5, odd, p, p, p, 1, k, th, 1 << 20, sums)
    for block_rows in (5, 7, 8, -1, 12):
        refused(res, b"block_rows", h, block_rows, odd, p, p, p, 1, 4, th, 1 << 4, sums)
    for k, active in ((4, 1 << 4), (4, 0xffffffff), (1, 2), (15, 1 << 15), (16, 1 << 16)):
        refused(res, b"active", h, 1, odd, p, p, p, 1, k, th, active, sums)
    for x, ax, bx, w in ((odd, p, p, p), (p, odd, p, p), (p, p, odd, p), (p, p, p, odd)):
        refused(res, b"16-byte aligned", h, 1, x, ax, bx, w, 1, 4, th, 0xf, sums)
    assert list(sums) == [7.0] * 32
    assert lib.cfs_hip_runtime_bound() == bound  # nothing above initialised the runtime
