"""cfs_hip_sym_block_diagonal_async, cfs_hip_sym_pcg_block and cfs_hip_sym_block_inverse_async without a
GPU: the library exports them, the ctypes binding declares them, the ABI version has not moved, and
their argument checks answer before anything touches a device."""
import ctypes as C
import os
import re

import cfs_spmv_amd as cfs
from cfs_spmv_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("cfs_hip_sym_block_diagonal_async", "cfs_hip_sym_pcg_block", "cfs_hip_sym_block_inverse_async")
BAD_BLOCK_ROWS = (0, 5, 7, -1)


def test_the_three_symbols_are_declared_exported_and_bound():
    text = open(os.path.join(ROOT, "include", "cfs_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    lib = cfs.load()
    raw = C.CDLL(cfs.lib_path())
    for name in NEW:
        assert re.search(r"\bint\s+" + name + r"\s*\(", code), f"{name} is not declared in cfs_hip.h"
        assert name in _lib.SYMBOLS
        getattr(raw, name)  # dlsym
    assert re.search(r"#define\s+CFS_HIP_ABI_VERSION\s+4\b", code)
    assert lib.cfs_hip_abi_version() == 4
    vp, ip = C.c_void_p, C.POINTER(C.c_int)
    assert lib.cfs_hip_sym_block_diagonal_async.argtypes == [vp, C.c_int, vp, vp]
    assert lib.cfs_hip_sym_block_inverse_async.argtypes == [vp, C.c_int, vp, vp]
    assert lib.cfs_hip_sym_pcg_block.argtypes == [vp, vp, vp, C.c_int, C.c_double, C.c_int, C.c_int, ip,
                                                  C.POINTER(C.c_double), vp]
    # the Python mirror
    for name in ("block_diagonal", "block_inverse", "pcg"):
        assert callable(getattr(cfs.SymMatrix, name))
    import inspect
    from cfs_spmv_amd import solver
    for f in (cfs.SymMatrix.pcg, solver.pcg, solver.pcg_native):
        assert inspect.signature(f).parameters["block"].default == 3


def test_null_handles_and_unknown_block_sizes_are_refused_before_any_device_work():
    lib = cfs.load()
    bound = lib.cfs_hip_runtime_bound()
    # (a non-null handle that is never dereferenced: the checks of the other arguments come first)
    fake, vec, other = C.c_void_p(0x1000), C.c_void_p(0x2000), C.c_void_p(0x3000)
    for gather in (lib.cfs_hip_sym_block_diagonal_async, lib.cfs_hip_sym_block_inverse_async):
        for bs in (1, 2, 3, 4, 6) + BAD_BLOCK_ROWS:
            for h, out in ((None, vec), (fake, None), (None, None)):
                assert gather(h, bs, out, None) == _lib.ERR_ARG, (bs, h, out)
                assert b"null" in lib.cfs_hip_last_error()
        for bs in BAD_BLOCK_ROWS:
            assert gather(fake, bs, vec, None) == _lib.ERR_ARG, bs
            assert b"block_rows" in lib.cfs_hip_last_error()
    for bs in (1, 2, 3, 4, 6) + BAD_BLOCK_ROWS:
        for h, u, b in ((None, vec, other), (fake, None, other), (fake, vec, None), (None, None, None)):
            it, res = C.c_int(7), C.c_double(7.0)
            rc = lib.cfs_hip_sym_pcg_block(h, u, b, bs, 1e-8, 10, 8, C.byref(it), C.byref(res), None)
            assert rc == _lib.ERR_ARG, (bs, h, u, b, rc)
            assert b"null" in lib.cfs_hip_last_error()
    for bs in BAD_BLOCK_ROWS:
        it, res = C.c_int(7), C.c_double(7.0)
        rc = lib.cfs_hip_sym_pcg_block(fake, vec, other, bs, 1e-8, 10, 8, C.byref(it), C.byref(res), None)
        assert rc == _lib.ERR_ARG and b"block_rows" in lib.cfs_hip_last_error(), bs
        assert it.value == 0 and res.value == 0.0
    assert lib.cfs_hip_runtime_bound() == bound  # nothing above initialised the runtime
