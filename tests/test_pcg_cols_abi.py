"""cfs_hip_sym_pcg_cols and cfs_hip_sym_pcg_amg_cols without a GPU, by the method of test_lobpcg_amg_abi.py: the header
declares them with the documented signatures, the library exports them, the ctypes bindings' argument types match the
declarations, the Python mirror is there and raises its ValueErrors before any device work, and the argument checks that
need no device answer, in the documented order, before a handle is dereferenced or the runtime initialised.

The entry points are additions: CFS_HIP_ABI_VERSION stays at 4 and callers detect them by their symbols.  SymMatrix.pcg,
SymMatrix.pcg_amg and the functions of solver.py keep their signatures."""
import ctypes as C
import inspect
import os
import re

import pytest

import cfs_spmv_amd as cfs
from cfs_spmv_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIGNATURES = {
    "cfs_hip_sym_pcg_cols": ["cfs_hip_sym_t h", "void *u_dev", "const void *b_dev", "long long ld", "int ncols", "int block_rows",
                             "double tol", "int maxiter", "int check_every", "int *iterations", "double *relres", "void *stream"],
    "cfs_hip_sym_pcg_amg_cols": ["cfs_hip_sym_t h", "cfs_hip_amg_t a", "void *u_dev", "const void *b_dev", "long long ld", "int ncols",
                                 "double tol", "int maxiter", "int check_every", "int *iterations", "double *relres", "void *stream"],
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
             "int *": ip, "double *": dp, "long long": C.c_longlong}
    declared = [ctype[re.sub(r"\w+$", "", p).strip()] for p in params]
    assert getattr(lib, name).argtypes == declared


def test_the_documented_order_of_the_refusals_is_in_the_header():
    text = " ".join(open(os.path.join(ROOT, "include", "cfs_hip.h")).read().split()).replace(" * ", " ")  # (the comment's margin)
    doc = text[text.index("PRECONDITIONED CG ON A BLOCK OF RIGHT-HAND SIDES"):text.index("int cfs_hip_sym_pcg_cols(")]
    assert "bits of the one-column entry" in doc
    doc = doc[doc.index("Refusals"):]
    words = ["a null pointer", "ncols outside 1 .. CFS_HIP_LOBPCG_MAX_K", "not 16-byte aligned", "ld < n", "blocks overlap", "tol < 0",
             "block_rows that is not", "CFS_HIP_ERR_UNSUPPORTED for a shard", "a host pointer", "not positive (definite)"]
    at = [doc.index(w) for w in words]
    assert at == sorted(at), list(zip(words, at))
    doc = text[text.index("int cfs_hip_sym_pcg_cols("):text.index("int cfs_hip_sym_pcg_amg_cols(")]
    doc = doc[doc.index("Refusals as for cfs_hip_sym_pcg_cols"):]
    at = [doc.index(w) for w in ("CFS_HIP_ERR_UNSUPPORTED", "created on another handle", "last refresh failed", "a host pointer")]
    assert at == sorted(at), at


def test_the_python_mirror():
    from cfs_spmv_amd import solver
    p = inspect.signature(cfs.SymMatrix.pcg_cols).parameters
    assert list(p) == ["self", "U", "B", "precond", "block", "tol", "maxiter", "check_every", "stream"]
    assert (p["precond"].default, p["block"].default, p["tol"].default, p["maxiter"].default, p["check_every"].default,
            p["stream"].default) == ("jacobi", 3, 1e-10, 1000, 8, None)
    for f in (solver.pcg_cols, solver.pcg_cols_native):
        q = inspect.signature(f).parameters
        assert list(q)[:2] == ["A", "B"] and q["amg"].default is None and q["precond"].default == "jacobi" and q["block"].default == 3
    # what was there before keeps its signature
    assert list(inspect.signature(cfs.SymMatrix.pcg).parameters) == ["self", "u", "b", "precond", "tol", "maxiter", "check_every", "stream",
                                                                     "block"]
    assert list(inspect.signature(cfs.SymMatrix.pcg_amg).parameters) == ["self", "u", "b", "amg", "tol", "maxiter", "check_every", "stream"]
    assert list(inspect.signature(solver.pcg_amg_native).parameters) == ["A", "b", "amg", "tol", "maxiter", "x0", "check_every"]


class _NoDevice:
    """stands in for a SymMatrix / an Amg where the arguments are refused before either is used"""
    dtype = None

    def __getattr__(self, name):
        raise AssertionError(f"{name} was asked for: the arguments should have been refused first")


def test_the_value_errors_come_before_any_device_work():
    import torch
    from cfs_spmv_amd import solver
    lib = cfs.load()
    bound = lib.cfs_hip_runtime_bound()
    A, G = _NoDevice(), _NoDevice()
    B = torch.zeros((6, 4), dtype=torch.float64)
    for f in (solver.pcg_cols, solver.pcg_cols_native):
        with pytest.raises(ValueError, match="needs amg="):
            f(A, B, precond="amg")
        for precond in ("jacobi", "none", "block_jacobi"):
            with pytest.raises(ValueError, match='goes with precond="amg"'):
                f(A, B, precond=precond, amg=G)
    cols = lambda n, k, ld, dt=torch.float64: torch.as_strided(torch.zeros(k * ld, dtype=dt), (n, k), (1, ld))
    U = cols(6, 4, 8)
    for bad in (cols(6, 3, 8), cols(5, 4, 8), cols(6, 4, 8, torch.float32), torch.zeros(6, dtype=torch.float64)):
        with pytest.raises(ValueError, match="2-D blocks of the same shape and type"):
            cfs.SymMatrix.pcg_cols(A, U, bad)
    with pytest.raises(ValueError, match="2-D blocks"):
        cfs.SymMatrix.pcg_cols(A, U[:, 0], U[:, 1])
    for bad in (cols(6, 4, 10), torch.zeros((6, 4), dtype=torch.float64)):  # another ld; row-major
        with pytest.raises(ValueError, match="stored by columns"):
            cfs.SymMatrix.pcg_cols(A, U, bad)
        with pytest.raises(ValueError, match="stored by columns"):
            cfs.SymMatrix.pcg_cols(A, bad, U)
    with pytest.raises(ValueError, match="needs the hierarchy"):
        cfs.SymMatrix.pcg_cols(A, U, cols(6, 4, 8), precond="amg")
    with pytest.raises(ValueError, match="unknown preconditioner"):
        cfs.SymMatrix.pcg_cols(A, U, cols(6, 4, 8), precond="ssor")
    assert lib.cfs_hip_runtime_bound() == bound  # nothing above initialised the runtime


def _call(lib, amg, h, a, u, b, ld=1 << 20, ncols=4, block_rows=1, tol=1e-8, maxiter=10, with_out=True):
    it = (C.c_int * 17)(*([7] * 17))
    res = (C.c_double * 17)(*([7.0] * 17))
    outs = (it, res) if with_out else (None, None)
    if amg:
        rc = lib.cfs_hip_sym_pcg_amg_cols(h, a, u, b, ld, ncols, tol, maxiter, 8, *outs, None)
    else:
        rc = lib.cfs_hip_sym_pcg_cols(h, u, b, ld, ncols, block_rows, tol, maxiter, 8, *outs, None)
    return rc, list(it), list(res)


@pytest.mark.parametrize("amg", (False, True), ids=("pcg_cols", "pcg_amg_cols"))
def test_the_refusals_that_need_no_device_come_in_the_documented_order(amg):
    lib = cfs.load()
    bound = lib.cfs_hip_runtime_bound()
    # (non-null handles that are never dereferenced: the checks below come before the handle is read)
    h, a, p, q, odd = C.c_void_p(0x1000), C.c_void_p(0x2000), C.c_void_p(0x4000), C.c_void_p(0x8000), C.c_void_p(0x4008)
    # 1. a null pointer first: every later argument is bad as well, and nothing is written
    nulls = [(None, a, p, q), (h, a, None, q), (h, a, p, None), (None, None, None, None)] + ([(h, None, p, q)] if amg else [])
    for hh, aa, u, b in nulls:
        for ncols in (4, 0, 17):
            rc, it, res = _call(lib, amg, hh, aa, u, b, ld=-1, ncols=ncols, block_rows=5, tol=-1.0, maxiter=-1)
            assert rc == _lib.ERR_ARG and b"null" in lib.cfs_hip_last_error(), (hh, aa, u, b, ncols)
            assert it == [7] * 17 and res == [7.0] * 17
    # 2. ncols, with misaligned pointers, a bad ld, tolerance and block_rows behind it; *iterations = 0
    for ncols in (0, -1, 17, 1 << 20):
        rc, it, res = _call(lib, amg, h, a, odd, odd, ld=-1, ncols=ncols, block_rows=5, tol=-1.0, maxiter=-1)
        assert rc == _lib.ERR_ARG and b"ncols" in lib.cfs_hip_last_error(), ncols
        assert it == [0] + [7] * 16 and res == [0.0] + [7.0] * 16
        assert _call(lib, amg, h, a, odd, odd, ld=-1, ncols=ncols, with_out=False)[0] == _lib.ERR_ARG  # (either may be NULL)
    # 3. the alignment of the pointers, with everything behind it bad; the outputs of every column zeroed
    for u, b in ((odd, q), (p, odd), (odd, odd)):
        for ncols in (1, 9, 16):
            rc, it, res = _call(lib, amg, h, a, u, b, ld=-1, ncols=ncols, block_rows=5, tol=-1.0, maxiter=-1)
            assert rc == _lib.ERR_ARG and b"16-byte aligned" in lib.cfs_hip_last_error(), (u, b, ncols)
            assert it == [0] * ncols + [7] * (17 - ncols) and res == [0.0] * ncols + [7.0] * (17 - ncols)
    assert lib.cfs_hip_runtime_bound() == bound  # nothing above initialised the runtime
