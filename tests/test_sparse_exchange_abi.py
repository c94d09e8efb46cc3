"""The packed all-to-all of the native exchange (cfs_hip_comm_alltoallv) and the selectable exchange form
of a multi-device handle (cfs_hip_sym_multi_set_exchange, cfs_hip_sym_multi_exchange_info) without a
GPU: the library exports them, the header declares them, the ctypes binding lists them, and their
argument checks answer before anything touches a device."""
import ctypes as C
import os
import re

import cfs_spmv_amd as cfs
from cfs_spmv_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("cfs_hip_comm_alltoallv", "cfs_hip_sym_multi_set_exchange", "cfs_hip_sym_multi_exchange_info")


def test_the_three_symbols_are_declared_exported_and_bound():
    text = open(os.path.join(ROOT, "include", "cfs_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    lib = cfs.load()
    raw = C.CDLL(cfs.lib_path())
    for name in NEW:
        assert re.search(r"\bint\s+" + name + r"\s*\(", code), f"{name} is not declared in cfs_hip.h"
        assert name in _lib.SYMBOLS
        getattr(raw, name)  # dlsym
    assert re.search(r"#define\s+CFS_HIP_EXCHANGE_REDUCE_SCATTER\s+0\b", code)
    assert re.search(r"#define\s+CFS_HIP_EXCHANGE_SPARSE\s+1\b", code)
    assert (_lib.EXCHANGE_REDUCE_SCATTER, _lib.EXCHANGE_SPARSE) == (0, 1)
    assert (cfs.EXCHANGE_REDUCE_SCATTER, cfs.EXCHANGE_SPARSE) == (0, 1)
    assert lib.cfs_hip_abi_version() == 4
    assert re.search(r"#define\s+CFS_HIP_ABI_VERSION\s+4\b", code)
    vp, ip, i64p = C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_int64)
    assert lib.cfs_hip_comm_alltoallv.argtypes == [vp, vp, vp, vp, C.c_int, vp]
    assert lib.cfs_hip_sym_multi_set_exchange.argtypes == [vp, C.c_int]
    assert lib.cfs_hip_sym_multi_exchange_info.argtypes == [vp, ip, i64p, i64p]
    for name in ("set_exchange", "exchange_info"):
        assert callable(getattr(cfs.SymMatrix, name))


def test_alltoallv_refuses_a_null_communicator_and_bad_value_sizes():
    lib = cfs.load()
    bound = lib.cfs_hip_runtime_bound()
    one = (C.c_void_p * 1)(0x1000)
    counts = (C.c_int64 * 1)(0)
    rc = lib.cfs_hip_comm_alltoallv(None, one, one, counts, 8, one)
    assert rc == _lib.ERR_ARG
    assert b"bad argument" in lib.cfs_hip_last_error()
    # (a communicator that is never dereferenced: the checks of the other arguments come first)
    fake = C.c_void_p(0x1000)
    for send, recv, cnt, vb, st in ((None, one, counts, 8, one), (one, None, counts, 8, one), (one, one, None, 8, one),
                                    (one, one, counts, 8, None), (one, one, counts, 2, one), (one, one, counts, 16, one)):
        assert lib.cfs_hip_comm_alltoallv(fake, send, recv, cnt, vb, st) == _lib.ERR_ARG
        assert b"bad argument" in lib.cfs_hip_last_error()
    assert lib.cfs_hip_runtime_bound() == bound  # nothing above initialised the runtime


def test_the_handle_entry_points_refuse_a_null_handle():
    lib = cfs.load()
    bound = lib.cfs_hip_runtime_bound()
    form, vals, nbytes = C.c_int(7), C.c_int64(7), C.c_int64(7)
    for f in (_lib.EXCHANGE_REDUCE_SCATTER, _lib.EXCHANGE_SPARSE, 5):
        assert lib.cfs_hip_sym_multi_set_exchange(None, f) == _lib.ERR_ARG
        assert b"null handle" in lib.cfs_hip_last_error()
    lib.cfs_hip_comm_alltoallv(None, None, None, None, 8, None)  # another message in between
    assert lib.cfs_hip_sym_multi_exchange_info(None, C.byref(form), C.byref(vals), C.byref(nbytes)) == _lib.ERR_ARG
    assert b"null handle" in lib.cfs_hip_last_error()
    assert (form.value, vals.value, nbytes.value) == (7, 7, 7)  # outputs untouched
    assert lib.cfs_hip_runtime_bound() == bound
