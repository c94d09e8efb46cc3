"""cfs_hip_amg_apply_cols, cfs_hip_sym_lobpcg_amg and their companions without a GPU, by the method of
test_lobpcg_abi.py: the header declares them with the documented signatures, the library exports them, the ctypes
bindings' argument types match the declarations, the Python mirror is there and raises its ValueErrors before any device
work, and the argument checks that need no device answer before a handle is dereferenced or the runtime initialised.

The entry points are additions: CFS_HIP_ABI_VERSION stays at 4 and callers detect them by their symbols.

SymMatrix.lobpcg keeps the signature test_lobpcg_abi.py pins: the hierarchy is passed as `precond` itself there, and by
name -- precond="amg", amg=G -- through solver.lobpcg and solver.lobpcg_native."""
import ctypes as C
import inspect
import os
import re

import pytest

import cfs_spmv_amd as cfs
from cfs_spmv_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIGNATURES = {
    "cfs_hip_amg_apply_cols": ["cfs_hip_amg_t a", "void *z_dev", "const void *r_dev", "long long ld", "int ncols", "unsigned active",
                               "void *stream"],
    "cfs_hip_amg_column_cycles": ["cfs_hip_amg_t a", "long long *cycles"],
    "cfs_hip_sym_lobpcg_amg": ["cfs_hip_sym_t h", "cfs_hip_amg_t a", "int k", "double tol", "double scale", "int maxiter",
                               "const void *x0_dev", "long long ld0", "double *eigenvalues", "void *vectors_dev", "long long ld",
                               "double *residuals", "int *nconv", "int *iterations", "int *products", "void *stream"],
    "cfs_hip_sym_debug_lobpcg_amg": ["cfs_hip_sym_t h", "cfs_hip_amg_t a", "int k", "const void *x0_dev", "long long ld0", "int iters",
                                     "double *theta", "void *vectors_dev", "long long ld", "double *resnorms", "void *stream"],
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
             "int *": ip, "double *": dp, "long long": C.c_longlong, "unsigned": C.c_uint, "long long *": C.POINTER(C.c_longlong)}
    declared = [ctype[re.sub(r"\w+$", "", p).strip()] for p in params]
    assert getattr(lib, name).argtypes == declared


def test_the_python_mirror():
    from cfs_spmv_amd import solver
    for f in (solver.lobpcg, solver.lobpcg_native):
        p = inspect.signature(f).parameters
        assert list(p)[:2] == ["A", "k"] and p["amg"].default is None and p["precond"].default == "jacobi"
    p = inspect.signature(cfs.Amg.apply).parameters
    assert list(p) == ["self", "z", "r", "active", "stream"] and p["active"].default is None and p["stream"].default is None
    assert p["active"].kind is p["stream"].kind is inspect.Parameter.KEYWORD_ONLY  # (a positional stream cannot become the mask)
    assert callable(cfs.SymMatrix.debug_lobpcg_amg) and callable(cfs.Amg.column_cycles)


class _NoDevice:
    """stands in for a SymMatrix / an Amg where the arguments are refused before either is used"""
    dtype = None

    def __getattr__(self, name):
        raise AssertionError(f"{name} was asked for: the arguments should have been refused first")


def test_the_value_errors_come_before_any_device_work():
    from cfs_spmv_amd import solver
    lib = cfs.load()
    bound = lib.cfs_hip_runtime_bound()
    A, G = _NoDevice(), _NoDevice()
    for f in (solver.lobpcg, solver.lobpcg_native):
        with pytest.raises(ValueError, match="needs amg="):
            f(A, 4, precond="amg")
        for precond in ("jacobi", "none", "block_jacobi"):
            with pytest.raises(ValueError, match='goes with precond="amg"'):
                f(A, 4, precond=precond, amg=G)
    # the method has no argument for the hierarchy: the name alone is refused, and says where the hierarchy goes
    with pytest.raises(ValueError, match="needs the hierarchy"):
        cfs.SymMatrix.lobpcg(A, k=4, precond="amg", scale=1.0)
    assert lib.cfs_hip_runtime_bound() == bound  # nothing above initialised the runtime


def _solve(lib, h, a, k=4, tol=1e-8, scale=1.0, maxiter=10, x0=None, ld0=0, w=True, x=C.c_void_p(0x4000), ld=1 << 20):
    vals = (C.c_double * 16)(*([7.0] * 16))
    res = (C.c_double * 16)(*([7.0] * 16))
    nconv, iterations, products = C.c_int(7), C.c_int(7), C.c_int(7)
    rc = lib.cfs_hip_sym_lobpcg_amg(h, a, k, tol, scale, maxiter, x0, ld0, vals if w else None, x, ld, res, C.byref(nconv),
                                    C.byref(iterations), C.byref(products), None)
    return rc, (nconv.value, iterations.value, products.value), list(vals) + list(res)


def test_null_arguments_are_refused_first():
    lib = cfs.load()
    bound = lib.cfs_hip_runtime_bound()
    h = C.c_void_p(0x1000)
    for k in (4, 0, 17):
        for hh, a, w, x in ((None, h, True, h), (h, None, True, h), (h, h, False, h), (h, h, True, None), (None, None, False, None)):
            rc, counters, out = _solve(lib, hh, a, k=k, tol=-1.0, w=w, x=x)
            assert rc == _lib.ERR_ARG and b"null" in lib.cfs_hip_last_error(), (k, hh, a, w, x)
            assert counters == (7, 7, 7) and out == [7.0] * 32
    t, r = (C.c_double * 16)(*([7.0] * 16)), (C.c_double * 16)(*([7.0] * 16))
    for args in ((None, h, 4, None, 0, 2, t, h, 1 << 20, r), (h, None, 4, None, 0, 2, t, h, 1 << 20, r),
                 (h, h, 4, None, 0, 2, None, h, 1 << 20, r), (h, h, 4, None, 0, 2, t, None, 1 << 20, r),
                 (h, h, 4, None, 0, 2, t, h, 1 << 20, None)):
        assert lib.cfs_hip_sym_debug_lobpcg_amg(*args, None) == _lib.ERR_ARG and b"null" in lib.cfs_hip_last_error()
    assert list(t) == [7.0] * 16 and list(r) == [7.0] * 16
    p = C.c_void_p(0x4000)
    for a, z, rr in ((None, p, p), (h, None, p), (h, p, None)):
        assert lib.cfs_hip_amg_apply_cols(a, z, rr, 16, 17, 1 << 20, None) == _lib.ERR_ARG and b"null" in lib.cfs_hip_last_error()
    cyc = C.c_longlong(7)
    assert lib.cfs_hip_amg_column_cycles(None, C.byref(cyc)) == _lib.ERR_ARG and cyc.value == 7
    assert lib.cfs_hip_amg_column_cycles(h, None) == _lib.ERR_ARG
    assert lib.cfs_hip_runtime_bound() == bound  # nothing above initialised the runtime


def test_checks_that_need_no_device_answer_before_the_handles_are_looked_at():
    lib = cfs.load()
    bound = lib.cfs_hip_runtime_bound()
    # (non-null handles that are never dereferenced: the checks of the other arguments come first)
    h, a = C.c_void_p(0x1000), C.c_void_p(0x2000)

    def refused(word, **kw):
        rc, counters, out = _solve(lib, h, a, **kw)
        msg = lib.cfs_hip_last_error()
        assert rc == _lib.ERR_ARG and word in msg, (kw, rc, msg)
        assert counters == (0, 0, 0) and out == [7.0] * 32, kw  # the counters zeroed, nothing else written
    # in the order of cfs_hip_sym_lobpcg: every later argument is bad as well
    bad = dict(tol=-1.0, scale=0.0, maxiter=-1, x0=C.c_void_p(0x3008))
    for k in (0, -1, 17, 1 << 20):
        refused(b"bad k", k=k, **bad)
    del bad["tol"], bad["scale"], bad["maxiter"]
    for kw in (dict(tol=-1e-3), dict(tol=float("nan")), dict(scale=0.0), dict(scale=-1.0), dict(scale=float("inf")),
               dict(scale=float("nan")), dict(maxiter=-1)):
        refused(b"tolerance", **kw, **bad)
    refused(b"16-byte aligned", x0=C.c_void_p(0x3008), ld0=1 << 20)
    refused(b"16-byte aligned", x=C.c_void_p(0x4004))
    t, r = (C.c_double * 16)(*([7.0] * 16)), (C.c_double * 16)(*([7.0] * 16))
    for k, iters, x, word in ((0, 2, 0x4000, b"bad k"), (17, 2, 0x4000, b"bad k"), (4, -1, 0x4000, b"tolerance"),
                              (4, 2, 0x4008, b"16-byte aligned")):
        assert lib.cfs_hip_sym_debug_lobpcg_amg(h, a, k, None, 0, iters, t, C.c_void_p(x), 1 << 20, r, None) == _lib.ERR_ARG
        assert word in lib.cfs_hip_last_error()
    assert list(t) == [7.0] * 16 and list(r) == [7.0] * 16
    # the blocked cycle: ncols, the mask, the alignment of the pointers -- before the hierarchy is read
    p, odd = C.c_void_p(0x4000), C.c_void_p(0x4008)
    for ncols in (0, -1, 17, 1 << 20):
        assert lib.cfs_hip_amg_apply_cols(a, odd, p, 0, ncols, 0xffffffff, None) == _lib.ERR_ARG
        assert b"ncols" in lib.cfs_hip_last_error()
    for ncols, active in ((4, 1 << 4), (4, 0xffffffff), (1, 2), (15, 1 << 15), (16, 1 << 16), (16, 1 << 31)):
        assert lib.cfs_hip_amg_apply_cols(a, odd, p, 0, ncols, active, None) == _lib.ERR_ARG
        assert b"active" in lib.cfs_hip_last_error()
    for z, rr in ((odd, p), (p, odd)):
        assert lib.cfs_hip_amg_apply_cols(a, z, rr, 0, 4, 0xf, None) == _lib.ERR_ARG
        assert b"16-byte aligned" in lib.cfs_hip_last_error()
    assert lib.cfs_hip_runtime_bound() == bound  # nothing above initialised the runtime
