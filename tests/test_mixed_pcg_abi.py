"""cfs_hip_sym_pcg_mixed without a GPU: the header declares it with the documented signature, the library
exports it, the ctypes binding's argument types match the declaration, the Python mirror is there, and the
argument checks that need no device answer before anything touches one.

The entry point is an addition: CFS_HIP_ABI_VERSION stays where the library's other tests pin it, and callers
detect the entry point by its symbol, as they do for the other solver entry points."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

import cfs_spmv_amd as cfs
from cfs_spmv_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "cfs_hip_sym_pcg_mixed"
SIGNATURE = ["cfs_hip_sym_t h64", "cfs_hip_sym_t h32", "void *u_dev", "const void *b_dev", "int block_rows", "double tol",
             "double delta", "int maxiter", "int check_every", "int *iterations", "int *replacements", "double *relres",
             "void *stream"]


def test_the_symbol_is_declared_exported_and_bound():
    text = open(os.path.join(ROOT, "include", "cfs_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    m = re.search(r"\bint\s+" + NAME + r"\s*\((.*?)\)\s*;", code, flags=re.S)
    assert m, f"{NAME} is not declared in cfs_hip.h"
    params = [" ".join(p.split()) for p in m.group(1).split(",")]
    assert params == SIGNATURE
    assert NAME in _lib.SYMBOLS
    getattr(C.CDLL(cfs.lib_path()), NAME)  # dlsym
    lib = cfs.load()
    version = int(re.search(r"#define\s+CFS_HIP_ABI_VERSION\s+(\d+)\b", code).group(1))
    assert lib.cfs_hip_abi_version() == version
    vp, ip, dp = C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_double)
    ctype = {"cfs_hip_sym_t": vp, "void *": vp, "const void *": vp, "int": C.c_int, "double": C.c_double, "int *": ip,
             "double *": dp}
    declared = [ctype[re.sub(r"\w+$", "", p).strip()] for p in params]
    assert getattr(lib, NAME).argtypes == declared
    assert declared == [vp, vp, vp, vp, C.c_int, C.c_double, C.c_double, C.c_int, C.c_int, ip, ip, dp, vp]


def test_the_python_mirror():
    from cfs_spmv_amd import solver
    assert callable(cfs.MixedSym.pcg) and callable(cfs.MixedSym.close) and callable(cfs.MixedSym.from_handles)
    sig = inspect.signature(cfs.MixedSym.pcg).parameters
    assert [sig[k].default for k in ("precond", "block", "delta", "check_every")] == ["jacobi", 3, 0.1, 8]
    for f in (solver.pcg_mixed, solver.pcg_mixed_native):
        p = inspect.signature(f).parameters
        assert p["delta"].default == 0.1 and p["precond"].default == "jacobi" and p["block"].default == 3
    rp, ci = np.array([0, 1, 2], np.int32), np.array([0, 1], np.int32)
    for values in (np.ones(2, np.float32), np.ones(2, np.int64), np.ones(2, np.complex128)):
        with pytest.raises(TypeError, match="float64"):  # (refused before a handle is built)
            cfs.MixedSym(2, rp, ci, values)


def test_checks_that_need_no_device_answer_first():
    lib = cfs.load()
    bound = lib.cfs_hip_runtime_bound()
    # (non-null handles that are never dereferenced: the checks of the other arguments come first)
    h64, h32, u, b = C.c_void_p(0x1000), C.c_void_p(0x2000), C.c_void_p(0x3000), C.c_void_p(0x4000)

    def call(h64, h32, u, b, block_rows=1, delta=0.1):
        it, rep, res = C.c_int(7), C.c_int(7), C.c_double(7.0)
        rc = getattr(lib, NAME)(h64, h32, u, b, block_rows, 1e-8, delta, 10, 8, C.byref(it), C.byref(rep), C.byref(res), None)
        return rc, it.value, rep.value, res.value
    for args in ((None, h32, u, b), (h64, None, u, b), (h64, h32, None, b), (h64, h32, u, None), (None, None, None, None)):
        assert call(*args)[0] == _lib.ERR_ARG and b"null" in lib.cfs_hip_last_error(), args
    for block_rows in (5, 7, -1, 8):
        assert call(h64, h32, u, b, block_rows=block_rows) == (_lib.ERR_ARG, 0, 0, 0.0)
        assert b"block_rows" in lib.cfs_hip_last_error()
    for delta in (-0.5, 1.0, 2.0, float("nan"), float("inf")):
        assert call(h64, h32, u, b, delta=delta) == (_lib.ERR_ARG, 0, 0, 0.0), delta
        assert b"delta" in lib.cfs_hip_last_error()
    assert call(h64, h32, u, u) == (_lib.ERR_ARG, 0, 0, 0.0) and b"different vectors" in lib.cfs_hip_last_error()
    assert lib.cfs_hip_runtime_bound() == bound  # nothing above initialised the runtime
