"""cfs_hip_sym_minres without a GPU: the header declares it with the documented signature, the library exports
it, the ctypes binding's argument types match the declaration, the Python mirror is there, and the argument
checks that need no device answer before anything touches one.

The entry point is an addition: CFS_HIP_ABI_VERSION stays where the library's other tests pin it, and callers
detect the entry point by its symbol, as they do for the other solver entry points."""
import ctypes as C
import inspect
import os
import re

import cfs_spmv_amd as cfs
from cfs_spmv_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "cfs_hip_sym_minres"
SIGNATURE = ["cfs_hip_sym_t h", "void *u_dev", "const void *b_dev", "int precond", "double shift", "double tol",
             "int maxiter", "int check_every", "int *iterations", "double *relres", "void *stream"]
PRECONDS = (_lib.PRECOND_NONE, _lib.PRECOND_JACOBI, 2, -1)


def test_the_symbol_is_declared_exported_and_bound():
    text = open(os.path.join(ROOT, "include", "cfs_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    m = re.search(r"\bint\s+" + NAME + r"\s*\((.*?)\)\s*;", code, flags=re.S)
    assert m, f"{NAME} is not declared in cfs_hip.h"
    params = [" ".join(p.split()) for p in m.group(1).split(",")]
    assert params == SIGNATURE
    # appended behind cfs_hip_sym_pcg_mixed
    assert code.index("cfs_hip_sym_pcg_mixed") < m.start()
    assert NAME in _lib.SYMBOLS
    getattr(C.CDLL(cfs.lib_path()), NAME)  # dlsym
    lib = cfs.load()
    assert int(re.search(r"#define\s+CFS_HIP_ABI_VERSION\s+(\d+)\b", code).group(1)) == 4
    assert lib.cfs_hip_abi_version() == 4
    vp, ip, dp = C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_double)
    ctype = {"cfs_hip_sym_t": vp, "void *": vp, "const void *": vp, "int": C.c_int, "double": C.c_double, "int *": ip,
             "double *": dp}
    declared = [ctype[re.sub(r"\w+$", "", p).strip()] for p in params]
    assert getattr(lib, NAME).argtypes == declared
    assert declared == [vp, vp, vp, C.c_int, C.c_double, C.c_double, C.c_int, C.c_int, ip, dp, vp]


def test_the_python_mirror():
    from cfs_spmv_amd import solver
    assert callable(cfs.SymMatrix.minres) and callable(solver.minres) and callable(solver.minres_native)
    p = inspect.signature(cfs.SymMatrix.minres).parameters
    assert list(p) == ["self", "u", "b", "precond", "shift", "tol", "maxiter", "check_every", "stream"]
    assert [p[k].default for k in ("precond", "shift", "tol", "maxiter", "check_every", "stream")] == \
        ["none", 0.0, 1e-10, 1000, 8, None]
    for f in (solver.minres, solver.minres_native):
        p = inspect.signature(f).parameters
        assert list(p)[:2] == ["A", "b"] and p["precond"].default == "none" and p["shift"].default == 0.0


def _call(lib, h, u, b, precond=_lib.PRECOND_NONE, shift=0.0, tol=1e-8, maxiter=10):
    it, res = C.c_int(7), C.c_double(7.0)
    rc = getattr(lib, NAME)(h, u, b, precond, shift, tol, maxiter, 8, C.byref(it), C.byref(res), None)
    return rc, it.value, res.value


def test_null_arguments_are_refused_first():
    lib = cfs.load()
    bound = lib.cfs_hip_runtime_bound()
    h, u, b = C.c_void_p(0x1000), C.c_void_p(0x3000), C.c_void_p(0x4000)
    for precond in PRECONDS:
        for args in ((None, u, b), (h, None, b), (h, u, None), (None, None, None)):
            assert _call(lib, *args, precond=precond)[0] == _lib.ERR_ARG, (precond, args)
            assert b"null" in lib.cfs_hip_last_error(), (precond, args)
    assert lib.cfs_hip_runtime_bound() == bound  # nothing above initialised the runtime


def test_checks_that_need_no_device_answer_before_the_handle_is_looked_at():
    lib = cfs.load()
    bound = lib.cfs_hip_runtime_bound()
    # (a non-null handle that is never dereferenced: the checks of the other arguments come first)
    h, u, b = C.c_void_p(0x1000), C.c_void_p(0x3000), C.c_void_p(0x4000)
    refused = (_lib.ERR_ARG, 0, 0.0)
    for precond in (2, -1, 7):
        assert _call(lib, h, u, b, precond=precond) == refused and b"unknown preconditioner" in lib.cfs_hip_last_error()
    assert _call(lib, h, u, u) == refused and b"different vectors" in lib.cfs_hip_last_error()
    for uu, bb in ((C.c_void_p(0x3008), b), (u, C.c_void_p(0x4004))):
        assert _call(lib, h, uu, bb) == refused and b"16-byte aligned" in lib.cfs_hip_last_error()
    for kw in (dict(tol=-1e-3), dict(tol=float("nan")), dict(maxiter=-1)):
        assert _call(lib, h, u, b, **kw) == refused and b"tolerance" in lib.cfs_hip_last_error(), kw
    for shift in (float("nan"), float("inf"), -float("inf")):
        for precond in (_lib.PRECOND_NONE, _lib.PRECOND_JACOBI):
            assert _call(lib, h, u, b, precond=precond, shift=shift) == refused, (shift, precond)
            assert b"shift" in lib.cfs_hip_last_error()
    assert lib.cfs_hip_runtime_bound() == bound  # nothing above initialised the runtime
