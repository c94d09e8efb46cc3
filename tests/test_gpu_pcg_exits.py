"""The exit paths of the PCG entry points that share one host driver (cfs_solver::Pcg in cfs_solver.hpp):
cfs_hip_sym_cg, _pcg (Jacobi), _pcg_block (3), _pcg_cheb (degree 3 on Jacobi, estimated bounds) and _pcg_amg, in fp64
and fp32, on one seeded symmetric positive definite matrix of n = 257 rows (rand257 of test_gpu_cg_steps.py, scaled as
in test_gpu_pcg_steps.py): a tail behind the 16-byte part of the vectors, a trailing partial node block, less than one
grid trip.  One table, so that a solver added to it is held to the same exits:

  done at the first look (tol = 1e30), and maxiter = 0:  no iteration, the bytes of u untouched, relres the
      long-double ||b - A u0|| / ||b|| within the bound of the siblings' test_iteration_count_and_reported_residual
      (_true_relres of test_gpu_cg_steps.py)
  b = 0 and u0 = 0:                                      no iteration, relres == 0.0, u untouched
  a diagonal entry of 0 (the entry points that build M^-1 in the call):  CFS_HIP_ERR_ARG, u untouched
      (cfs_hip_amg_create_* refuses such a matrix: test_gpu_amg_steps.py)
  maxiter = 1 .. 4 on a deterministic handle:            the same bytes of u at check_every = 1 and 16
"""
import functools

import numpy as np
import pytest

from test_gpu_cg_steps import DET, DTYPES, _matrix, _rhs, _torch_first, _true_relres  # noqa: F401 (_torch_first: autouse)
from test_gpu_pcg_steps import scaled

pytestmark = pytest.mark.gpu

NAME = "rand257"


def _cg(A, G, u, b, **kw):
    return A.cg(u, b, **kw)


def _jacobi(A, G, u, b, **kw):
    return A.pcg(u, b, precond="jacobi", **kw)


def _block3(A, G, u, b, **kw):
    return A.pcg(u, b, precond="block_jacobi", block=3, **kw)


def _cheb3(A, G, u, b, **kw):
    return A.pcg_cheb(u, b, base="jacobi", degree=3, **kw)[:2]


def _amg(A, G, u, b, **kw):
    return A.pcg_amg(u, b, G, **kw)


# (the entry point, whether it builds its M^-1 -- and may refuse it -- inside the call)
ENTRIES = {"cg": (_cg, False), "pcg_jacobi": (_jacobi, True), "pcg_block3": (_block3, True), "pcg_cheb3": (_cheb3, True),
           "pcg_amg": (_amg, False)}
EACH = pytest.mark.parametrize("entry", list(ENTRIES))


@functools.lru_cache(maxsize=None)
def _case(dtype):
    """(n, rp, ci, va in the value type, b): computed once, shared, unchanged"""
    n, rp, ci, va = _matrix(NAME)
    assert n == 257
    return n, rp, ci, scaled(n, rp, ci, va, dtype), _rhs(n, dtype)


@pytest.fixture(scope="module")
def handles():
    """handles(dtype) -> (a deterministic handle, its hierarchy with more than the dense level): made once per value
    type, closed behind the module's last test"""
    made = {}

    def get(dtype):
        import cfs_spmv_amd as cfs
        if dtype not in made:
            n, rp, ci, va, _ = _case(dtype)
            D = cfs.SymMatrix(n, rp, ci, va, options=cfs.make_options(flags=DET))
            assert D.kernel_variant()["det"] == 1
            G = D.amg(rp, ci, va, coarse_max=64)
            assert G.info()["levels"] >= 2
            made[dtype] = (D, G)
        return made[dtype]
    yield get
    for D, G in made.values():
        G.close()
        D.close()


def _solve(entry, A, G, b, x0, **kw):
    """(the bytes of u afterwards, iterations, relres)"""
    import torch
    u = torch.from_numpy(x0).cuda()
    it, res = ENTRIES[entry][0](A, G, u, torch.from_numpy(b).cuda(), **kw)
    torch.cuda.synchronize()
    return u.cpu().numpy().view(np.uint8), it, res


@DTYPES
@EACH
@pytest.mark.parametrize("how", ["tol", "maxiter"])
def test_nothing_to_do_leaves_u_and_reports_its_residual(how, entry, dtype, handles):
    n, rp, ci, va, b = _case(dtype)
    A, G = handles(dtype)
    x0 = np.random.default_rng(4).uniform(-1, 1, n).astype(dtype)
    kw = dict(tol=1e30, maxiter=50) if how == "tol" else dict(tol=1e-8, maxiter=0)
    u, it, res = _solve(entry, A, G, b, x0, **kw)
    true, slack = _true_relres(n, rp, ci, va, b, x0, dtype)
    print(f"pcg-exits {np.dtype(dtype).name} {entry} {how}: iterations {it}, reported {res:.6e}, long double {true:.6e}, slack {slack:.3e}")
    assert it == 0
    assert np.array_equal(u, x0.view(np.uint8))
    assert abs(res - true) <= slack, (res, true, slack)


@DTYPES
@EACH
def test_zero_right_hand_side_and_zero_guess(entry, dtype, handles):
    n = _case(dtype)[0]
    A, G = handles(dtype)
    zero = np.zeros(n, dtype)
    u, it, res = _solve(entry, A, G, zero, zero, tol=1e-8, maxiter=50)
    assert it == 0 and res == 0.0
    assert np.array_equal(u, zero.view(np.uint8))


@DTYPES
@pytest.mark.parametrize("entry", [e for e in ENTRIES if ENTRIES[e][1]])
def test_a_zero_on_the_diagonal_is_refused_before_u_is_written(entry, dtype):
    import torch
    import cfs_spmv_amd as cfs
    from cfs_spmv_amd import _lib
    n, rp, ci, va, b = _case(dtype)
    rows = np.repeat(np.arange(n), np.diff(rp))
    va = va.copy()
    va[int(np.flatnonzero((rows == ci) & (rows == 100))[0])] = 0
    A = cfs.SymMatrix(n, rp, ci, va)
    x0 = np.random.default_rng(5).uniform(-1, 1, n).astype(dtype)
    for check_every in (1, 8):
        u = torch.from_numpy(x0).cuda()
        with pytest.raises(_lib.CfsHipError) as e:
            ENTRIES[entry][0](A, None, u, torch.from_numpy(b).cuda(), tol=1e-8, maxiter=50, check_every=check_every)
        assert e.value.code == _lib.ERR_ARG, e.value
        torch.cuda.synchronize()
        assert np.array_equal(u.cpu().numpy().view(np.uint8), x0.view(np.uint8))
    A.close()


@DTYPES
@EACH
def test_the_window_between_two_looks_does_not_change_the_bytes(entry, dtype, handles):
    n, rp, ci, va, b = _case(dtype)
    A, G = handles(dtype)
    x0 = np.zeros(n, dtype)
    for k in (1, 2, 3, 4):
        u1, it1, res1 = _solve(entry, A, G, b, x0, tol=0.0, maxiter=k, check_every=1)
        u16, it16, res16 = _solve(entry, A, G, b, x0, tol=0.0, maxiter=k, check_every=16)
        assert it1 == it16 == k, (k, it1, it16)
        assert np.array_equal(u1, u16) and res1 == res16, (k, res1, res16)
        assert not np.array_equal(u1, x0.view(np.uint8))
