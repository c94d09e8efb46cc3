"""cfs_hip_sym_pcg and cfs_hip_sym_diagonal_async without a GPU: the library exports them, the ctypes
binding declares them, and their argument checks answer before anything touches a device."""
import ctypes as C
import os
import re

import cfs_spmv_amd as cfs
from cfs_spmv_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("cfs_hip_sym_pcg", "cfs_hip_sym_diagonal_async")


def test_both_symbols_are_declared_exported_and_bound():
    text = open(os.path.join(ROOT, "include", "cfs_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    lib = cfs.load()
    raw = C.CDLL(cfs.lib_path())
    for name in NEW:
        assert re.search(r"\bint\s+" + name + r"\s*\(", code), f"{name} is not declared in cfs_hip.h"
        assert name in _lib.SYMBOLS
        getattr(raw, name)  # dlsym
    assert re.search(r"#define\s+CFS_HIP_PRECOND_NONE\s+0\b", code) and re.search(r"#define\s+CFS_HIP_PRECOND_JACOBI\s+1\b", code)
    assert (_lib.PRECOND_NONE, _lib.PRECOND_JACOBI) == (0, 1)
    assert lib.cfs_hip_abi_version() == 4
    vp, ip = C.c_void_p, C.POINTER(C.c_int)
    assert lib.cfs_hip_sym_diagonal_async.argtypes == [vp, vp, vp]
    assert lib.cfs_hip_sym_pcg.argtypes == [vp, vp, vp, C.c_int, C.c_double, C.c_int, C.c_int, ip,
                                            C.POINTER(C.c_double), vp]
    # the Python mirror
    for name in ("diagonal", "pcg"):
        assert callable(getattr(cfs.SymMatrix, name))
    from cfs_spmv_amd import solver
    assert callable(solver.pcg) and callable(solver.pcg_native)


def test_null_arguments_are_refused_before_any_device_work():
    lib = cfs.load()
    bound = lib.cfs_hip_runtime_bound()
    it, res = C.c_int(7), C.c_double(7.0)
    # (a non-null handle that is never dereferenced: the null check of the vectors comes first)
    fake = C.c_void_p(0x1000)
    vec = C.c_void_p(0x2000)
    for precond in (_lib.PRECOND_NONE, _lib.PRECOND_JACOBI, 5):
        for h, u, b in ((None, vec, vec), (fake, None, vec), (fake, vec, None), (None, None, None)):
            rc = lib.cfs_hip_sym_pcg(h, u, b, precond, 1e-8, 10, 8, C.byref(it), C.byref(res), None)
            assert rc == _lib.ERR_ARG, (precond, h, u, b, rc)
            assert b"null" in lib.cfs_hip_last_error()
    for h, d in ((None, vec), (fake, None), (None, None)):
        assert lib.cfs_hip_sym_diagonal_async(h, d, None) == _lib.ERR_ARG
        assert b"null" in lib.cfs_hip_last_error()
    assert lib.cfs_hip_runtime_bound() == bound  # nothing above initialised the runtime
