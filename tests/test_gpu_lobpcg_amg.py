"""cfs_hip_sym_lobpcg_amg on the GPU: LOBPCG with one column-blocked multigrid cycle per iteration as M^-1.

The spectrum is held to the rules of test_gpu_lobpcg.py, unchanged (its _check): nconv == k; r_i <= 2 tol lmax, r_i
recomputed in long double from the returned pairs; |theta_i - lambda_i| <= r_i + 16 u lmax BY INDEX against a dense or
shift-invert reference; the library's residuals within 4 u lmax + 1e-3 r_i.  Tolerances per value type are that file's.

  lap2d16x15, coarse_max 16 (levels 240 / 60 / 15), k = 4 and k = 16;  lap2d40x33 and lap2d40x33-scaled (fp64 only, as
  there), coarse_max 64;  rand257, coarse_max 40, the five-fold eigenvalue;  rand3, k = 1, a dense-only hierarchy:
  M^-1 = A^-1 up to rounding, so the solve must end within 3 iterations;  rotated_node_laplacian(3, 12, 11), block = 3,
  fp64 (its gaps are below what _check asks of fp32), and rotated_node_laplacian(2, 6, 5), block = 2, in both types.

Native against the model.  theta and the residual norms of cfs_hip_sym_debug_lobpcg_amg after iters = 0, 1, 3 on a
deterministic handle against a restatement of the same iterations in long double (test_gpu_lobpcg_steps.py's, with
W_i = Hierarchy.cycle((V)R_i) in long double); solver.lobpcg(precond="amg", iters=...), which forms W by the one-column
cfs_hip_amg_apply, is measured the same way in both value types and the native loop is allowed 4 x the larger of the two:
the allowance of that file's debug comparison.

The preconditioner has something to do.  lap2d40x33 and lap2d40x33-scaled, fp64, tol 1e-10, k = 4, the default start
block: the multigrid run takes at most half the iterations of precond="jacobi" in the same test run, and fewer products
than k x iterations (soft locking, and so a mask with holes, was exercised).  A numpy model of the iteration gave 86
against 352 and 46 against 330 iterations, and 184 products against 4 x 86 = 344.

Measured on the MI355X (iterations / products of the multigrid solve; fp64 at tol 1e-10, fp32 at 1e-4, lap2d(40,33) fp32
at 5e-5):

  lap2d(16,15) k=4   f64 34 / 111   f32 13 / 50        (Jacobi, test_gpu_lobpcg.py: 108 / 356 and 44 / 145)
  lap2d(16,15) k=16  f64 34 / 352   f32 15 / 166
  lap2d(40,33)       f64 84 / 186   f32 17 / 62        (Jacobi, same run: 352 / 871)
  lap2d(40,33) scaled f64 45 / 128                      (Jacobi, same run: 330 / 734)
  rand257            f64 32 / 128   f32 12 / 51
  rand3 k=1          f64 2 / 4      f32 2 / 4
  rotated_node_laplacian(3,12,11) block=3  f64 30 / 98
  rotated_node_laplacian(2,6,5) block=2    f64 31 / 87    f32 9 / 36
  debug entry against the long-double iterations, lap2d(16,15) k=4, iters 0 / 1 / 3 (model f64, model f32, native f64, native f32):
    8.998e-16, 7.623e-09, 1.500e-15, 7.623e-09;  1.850e-15, 5.186e-08, 2.467e-15, 5.186e-08;  1.606e-15, 6.278e-08, 1.092e-15, 6.278e-08
  host-driven and native loop, lap2d(16,15): 34 iterations, 111 products, 111 cycles each in f64; 13, 50, 50 in f32
"""
import ctypes as C
import functools

import numpy as np
import pytest

from test_amg_block_abi import rotated_node_laplacian
from test_gpu_amg_steps import Hierarchy
from test_gpu_cg_steps import DET, DTYPES, UNIT
from test_gpu_lobpcg import TOL, TOL_LAP40, _case, _check, _residuals, _torch_first  # noqa: F401
from test_gpu_lobpcg_steps import LD, _deviation, _round

pytestmark = pytest.mark.gpu


def _solve(A, G, **kw):
    import torch
    w, X, info = A.lobpcg(precond=G, **kw)
    torch.cuda.synchronize()
    return w, np.ascontiguousarray(X.cpu().numpy()), info


@functools.lru_cache(maxsize=None)
def _node_case(dtype, k=4, shape=(3, 12, 11)):
    """_case() for rotated_node_laplacian(*shape); computed once, shared, unchanged"""
    import scipy.sparse as sp
    n, rp, ci, va = rotated_node_laplacian(*shape)
    va = np.asarray(va).astype(dtype)
    lam = np.linalg.eigvalsh(sp.csr_matrix((va.astype(np.float64), ci, rp), shape=(n, n)).toarray())
    lmax = float(np.max(np.abs(lam)))
    lam = lam[:k + 1].copy()
    for x in (va, lam):
        x.setflags(write=False)
    return n, rp, ci, va, lam, lmax


# ---- the spectrum -----------------------------------------------------------------------------------------------
@DTYPES
@pytest.mark.parametrize("k", [4, 16])
def test_lap2d_16_15(k, dtype):
    """levels 240 / 60 / 15"""
    import cfs_spmv_amd as cfs
    case = _case("lap2d16x15", dtype, k=k)
    A = cfs.SymMatrix(*case[:4])
    G = A.amg(*case[1:4], coarse_max=16)
    assert tuple(G.info()["n"]) == (240, 60, 15)
    w, X, info = _check("lap2d(16,15) amg", case, dtype, A, TOL[dtype], k=k, precond=G)
    assert info["cycles"] > 0
    G.close()
    A.close()


@DTYPES
def test_lap2d_40_33(dtype):
    import cfs_spmv_amd as cfs
    case = _case("lap2d40x33", dtype)
    A = cfs.SymMatrix(*case[:4])
    G = A.amg(*case[1:4], coarse_max=64)
    _check("lap2d(40,33) amg", case, dtype, A, TOL_LAP40[dtype], precond=G, maxiter=1000)
    G.close()
    A.close()


def test_lap2d_40_33_scaled():
    """rows of mixed scale, fp64: the weights of the hierarchy make it invariant under the scaling"""
    import cfs_spmv_amd as cfs
    case = _case("lap2d40x33-scaled", np.float64)
    A = cfs.SymMatrix(*case[:4])
    G = A.amg(*case[1:4], coarse_max=64)
    _check("lap2d(40,33) scaled amg", case, np.float64, A, 1e-10, precond=G, maxiter=1000)
    G.close()
    A.close()


@DTYPES
def test_rand257_the_five_fold_eigenvalue(dtype):
    import cfs_spmv_amd as cfs
    case = _case("rand257", dtype)
    A = cfs.SymMatrix(*case[:4])
    G = A.amg(*case[1:4], coarse_max=40)
    _check("rand257 amg", case, dtype, A, TOL[dtype], precond=G)
    G.close()
    A.close()


@DTYPES
def test_rand3_a_dense_only_hierarchy_ends_within_three_iterations(dtype):
    import cfs_spmv_amd as cfs
    case = _case("rand3", dtype, k=1)
    A = cfs.SymMatrix(*case[:4])
    G = A.amg(*case[1:4], coarse_max=512)
    assert tuple(G.info()["kind"]) == (2,), "dense only"
    w, X, info = _check("rand3 amg", case, dtype, A, TOL[dtype], k=1, precond=G)
    assert info["iterations"] <= 3, info
    G.close()
    A.close()


def test_the_node_block_form():
    """fp64 only: the low gaps of this matrix are 3.5e-6 lmax (lmax 4741 over eigenvalues of 0.2 .. 0.44), below the
    4 tol lmax = 4e-4 lmax that _check's rule of a well chosen case asks of fp32 at its tolerance of 1e-4 -- at that
    tolerance the allowed residual, 0.47, exceeds the eigenvalues themselves and nothing can be paired by index"""
    import cfs_spmv_amd as cfs
    dtype = np.float64
    case = _node_case(dtype)
    A = cfs.SymMatrix(*case[:4])
    G = A.amg(*case[1:4], coarse_max=32, block=3)
    assert G.info()["block"] == 3 and G.info()["levels"] >= 2
    _check("rotated_node_laplacian(3,12,11) amg", case, dtype, A, TOL[dtype], precond=G)
    G.close()
    A.close()


@DTYPES
def test_the_node_block_form_in_both_value_types(dtype):
    """rotated_node_laplacian(2, 6, 5) with block = 2, n = 60: its low gaps are 6.7e-4 lmax and more (lmax 154), above
    the 4 tol lmax that _check asks of fp32 at tol 1e-4, so the node-block solve is held end to end in fp32 as well"""
    import cfs_spmv_amd as cfs
    case = _node_case(dtype, shape=(2, 6, 5))
    A = cfs.SymMatrix(*case[:4])
    G = A.amg(*case[1:4], coarse_max=8, block=2)
    assert G.info()["block"] == 2 and G.info()["levels"] >= 2
    _check("rotated_node_laplacian(2,6,5) amg", case, dtype, A, TOL[dtype], precond=G)
    G.close()
    A.close()


# ---- native against the model ---------------------------------------------------------------------------------------
def _reference_iterations(n, rp, ci, va, dtype, k, H, x0, iters):
    """test_gpu_lobpcg_steps.reference_iterations with W_i = the long-double cycle of H on the stored (V)R_i"""
    from oracle import oracle
    from cfs_spmv_amd.solver import lobpcg_rr
    S, AS = np.zeros((3 * k, n), LD), np.zeros((3 * k, n), LD)
    S[:k] = x0.T.astype(LD)

    def product(c):
        AS[c] = _round(oracle.csr_spmv_ldx(n, rp, ci, va, S[c]), dtype)

    def rayleigh_ritz(cols):
        Sa, ASa = S[cols], AS[cols]
        theta, Cm, rank = lobpcg_rr(Sa @ Sa.T, Sa @ ASa.T, k, 64 * UNIT[dtype])
        assert rank == k or len(cols) > k
        Cm = Cm.astype(LD)
        Cp = Cm.copy()
        Cp[:k] = 0
        X, AX = _round(Cm.T @ Sa, dtype), _round(Cm.T @ ASa, dtype)
        if len(cols) > k:
            S[2 * k:], AS[2 * k:] = _round(Cp.T @ Sa, dtype), _round(Cp.T @ ASa, dtype)
        S[:k], AS[:k] = X, AX
        return theta.astype(LD)

    def residual(theta):
        R = AS[:k] - theta[:, None] * S[:k]
        for i in range(k):
            S[k + i] = _round(H.cycle(_round(R[i], dtype)), dtype)
        return np.sqrt(np.sum(R * R, axis=1)) / np.sqrt(np.sum(S[:k] * S[:k], axis=1))

    for c in range(k):
        product(c)
    theta = rayleigh_ritz(list(range(k)))
    res = residual(theta)
    for it in range(iters):
        for i in range(k):
            product(k + i)
        theta = rayleigh_ritz(list(range(2 * k if it == 0 else 3 * k)))
        res = residual(theta)
    return theta.astype(np.float64), res.astype(np.float64)


@functools.lru_cache(maxsize=None)
def _iteration_case(iters):
    """per value type: (the native loop's deviation from the long-double iterations, the model's, the reference)"""
    import torch
    import cfs_spmv_amd as cfs
    from cfs_spmv_amd import solver
    k, out = 4, {}
    for dtype in (np.float64, np.float32):
        n, rp, ci, va = _case("lap2d16x15", dtype)[:4]
        A = cfs.SymMatrix(n, rp, ci, va, options=cfs.make_options(flags=DET))
        G = A.amg(rp, ci, va, coarse_max=16)
        H = Hierarchy(G, n, rp, ci, va, 1)
        ref = _reference_iterations(n, rp, ci, va, dtype, k, H, solver.default_x0(n, k, dtype), iters)
        theta, X, res = A.debug_lobpcg_amg(G, k, iters)
        torch.cuda.synchronize()
        theta2, X2, res2 = A.debug_lobpcg_amg(G, k, iters)
        torch.cuda.synchronize()
        assert X.shape == (n, k) and bool(torch.all(torch.isfinite(X)))
        assert np.array_equal(theta.view(np.uint8), theta2.view(np.uint8)) and bool(torch.equal(X, X2))
        wm, Xm, im = solver.lobpcg(A, k, precond="amg", amg=G, iters=iters)
        assert im["cycles"] == k * (iters + 1)
        G.close()
        A.close()
        out[dtype] = (_deviation(theta, res, ref), _deviation(wm, im["residuals"], ref), ref)
    return out


@DTYPES
@pytest.mark.parametrize("iters", [0, 1, 3])
def test_iterations_against_the_long_double_recurrence_and_the_model(iters, dtype):
    case = _iteration_case(iters)
    native, model = case[dtype][0], max(case[np.float64][1], case[np.float32][1])
    print(f"lobpcg-amg-steps lap2d16x15 k=4 iters={iters}: model f64 {case[np.float64][1]:.3e}, model f32 {case[np.float32][1]:.3e}, "
          f"native f64 {case[np.float64][0]:.3e}, native f32 {case[np.float32][0]:.3e}")
    ref = case[dtype][2]
    assert np.all(np.isfinite(ref[0])) and np.all(np.diff(ref[0]) >= 0)
    assert native <= 4 * model, f"lap2d16x15 {np.dtype(dtype).name}: deviation {native:.3e}, allowed 4 x {model:.3e}"


@DTYPES
def test_host_driven_and_native_loops_agree(dtype):
    """solver.lobpcg(precond="amg") against solver.lobpcg_native(precond="amg") on lap2d(16, 15): theta within the sum of
    the two runs' residuals, the comparison test_gpu_lobpcg.py makes between the two loops"""
    import torch
    import cfs_spmv_amd as cfs
    from cfs_spmv_amd.solver import lobpcg, lobpcg_native
    n, rp, ci, va, lam, lmax = _case("lap2d16x15", dtype)
    A = cfs.SymMatrix(n, rp, ci, va)
    G = A.amg(rp, ci, va, coarse_max=16)
    w1, X1, i1 = lobpcg(A, 4, precond="amg", amg=G, tol=TOL[dtype], scale=lmax)
    w2, X2, i2 = lobpcg_native(A, 4, precond="amg", amg=G, tol=TOL[dtype], scale=lmax)
    torch.cuda.synchronize()
    G.close()
    A.close()
    print(f"lobpcg-amg {np.dtype(dtype).name} lap2d(16,15): host-driven {w1} ({i1['iterations']} iterations, {i1['products']} products, "
          f"{i1['cycles']} cycles), native {w2} ({i2['iterations']} iterations, {i2['products']} products, {i2['cycles']} cycles)")
    assert i1["nconv"] == i2["nconv"] == 4 and X1.shape == X2.shape == (n, 4)
    assert np.all(np.abs(w1 - w2) <= i1["residuals"] + i2["residuals"])


# ---- the preconditioner has something to do -------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["lap2d40x33", "lap2d40x33-scaled"])
def test_half_the_iterations_of_jacobi_and_soft_locking(name):
    """fp64, tol 1e-10, k = 4, the default start block.  Measured on the MI355X (iterations / products):
      lap2d40x33:         jacobi 352 / 871,  amg  84 / 186 (186 cycles; k x iterations = 336)
      lap2d40x33-scaled:  jacobi 330 / 734,  amg  45 / 128 (128 cycles; k x iterations = 180)"""
    import torch
    import cfs_spmv_amd as cfs
    n, rp, ci, va, lam, lmax = _case(name, np.float64)
    A = cfs.SymMatrix(n, rp, ci, va)
    G = A.amg(rp, ci, va, coarse_max=64)
    wj, Xj, ij = A.lobpcg(k=4, precond="jacobi", tol=1e-10, scale=lmax, maxiter=1000)
    wa, Xa, ia = _solve(A, G, k=4, tol=1e-10, scale=lmax, maxiter=1000)
    torch.cuda.synchronize()
    G.close()
    A.close()
    print(f"lobpcg-amg f64 {name}: jacobi {ij['iterations']} iterations / {ij['products']} products, amg {ia['iterations']} / "
          f"{ia['products']} ({ia['cycles']} cycles)")
    assert ij["nconv"] == ia["nconv"] == 4
    assert 2 * ia["iterations"] <= ij["iterations"], (ia["iterations"], ij["iterations"])
    assert ia["products"] < 4 * ia["iterations"], "soft locking never dropped a pair"


# ---- reproducibility, refresh, refusals -----------------------------------------------------------------------------
@DTYPES
def test_a_deterministic_handle_is_bit_reproducible(dtype):
    import cfs_spmv_amd as cfs
    n, rp, ci, va, lam, lmax = _case("lap2d40x33", dtype)
    D = cfs.SymMatrix(n, rp, ci, va, options=cfs.make_options(flags=DET))
    assert D.kernel_variant()["det"] == 1
    G = D.amg(rp, ci, va, coarse_max=64)
    kw = dict(k=4, tol=TOL_LAP40[dtype], scale=lmax, maxiter=30)
    w1, X1, i1 = _solve(D, G, **kw)
    w2, X2, i2 = _solve(D, G, **kw)
    G.close()
    D.close()
    assert np.all(np.isfinite(w1)) and np.all(np.diff(w1) >= 0) and i1["iterations"] > 0
    assert np.array_equal(w1.view(np.uint8), w2.view(np.uint8)) and np.array_equal(X1.view(np.uint8), X2.view(np.uint8))
    assert (i1["nconv"], i1["iterations"], i1["products"], i1["cycles"]) == (i2["nconv"], i2["iterations"], i2["products"], i2["cycles"])
    assert np.array_equal(i1["residuals"].view(np.uint8), i2["residuals"].view(np.uint8))


@DTYPES
def test_a_refreshable_hierarchy_follows_update_values(dtype):
    """new values poured into the handle and into the hierarchy: the spectrum asserted is that of the NEW matrix"""
    import scipy.sparse as sp
    import cfs_spmv_amd as cfs
    n, rp, ci, va, lam, lmax = _case("lap2d16x15", dtype)
    rows = np.repeat(np.arange(n), np.diff(rp))
    s = 1.0 + 0.5 * np.cos(0.37 * np.arange(n)) ** 2
    vb = (s[rows] * np.asarray(va, np.float64) * s[ci]).astype(dtype)
    lamb = np.linalg.eigvalsh(sp.csr_matrix((vb.astype(np.float64), ci, rp), shape=(n, n)).toarray())
    new = (n, rp, ci, vb, lamb[:5].copy(), float(np.max(np.abs(lamb))))
    assert np.min(np.abs(new[4][:4] - lam[:4])) > 1e-3 * lmax, "the new spectrum is another one"
    A = cfs.SymMatrix(n, rp, ci, va, options=cfs.make_options(flags=cfs.FLAG_KEEP_VALUE_MAP))
    G = A.amg(rp, ci, va, coarse_max=16, refreshable=True)
    _check("lap2d(16,15) amg, as created", (n, rp, ci, va, lam, lmax), dtype, A, TOL[dtype], precond=G)
    A.update_values(vb)
    G.update_values(vb)
    assert G.refresh_info()["refreshes"] == 1
    _check("lap2d(16,15) amg, new values", new, dtype, A, TOL[dtype], precond=G)
    G.close()
    A.close()


@DTYPES
def test_refusals_leave_the_vectors_untouched(dtype):
    import torch
    import cfs_spmv_amd as cfs
    from cfs_spmv_amd import _lib
    lib = cfs.load()
    n, rp, ci, va, lam, lmax = _case("rand257", dtype)
    other = np.float32 if dtype == np.float64 else np.float64
    A, A2, Ao = cfs.SymMatrix(n, rp, ci, va), cfs.SymMatrix(n, rp, ci, va), cfs.SymMatrix(n, rp, ci, np.asarray(va).astype(other))
    G, Go = A.amg(rp, ci, va, coarse_max=40, refreshable=True), Ao.amg(rp, ci, np.asarray(va).astype(other), coarse_max=40)
    tdt = torch.float64 if dtype == np.float64 else torch.float32
    per = 16 // np.dtype(dtype).itemsize
    ld = -(-n // per) * per
    X = torch.full((4 * ld,), -777.25, dtype=tdt, device="cuda")
    w, res = (C.c_double * 4)(*([7.0] * 4)), (C.c_double * 4)(*([7.0] * 4))
    cnt = [C.c_int(7) for _ in range(3)]

    def refused(code, word, h=A, a=G, k=4, debug=False):
        if debug:
            rc = lib.cfs_hip_sym_debug_lobpcg_amg(h._h, a._a if a is not None else None, k, None, 0, 2, w, X.data_ptr(), ld, res, None)
        else:
            rc = lib.cfs_hip_sym_lobpcg_amg(h._h, a._a if a is not None else None, k, 1e-6, 1.0, 5, None, 0, w, X.data_ptr(), ld, res,
                                            *(C.byref(c) for c in cnt), None)
        assert rc == code and word in lib.cfs_hip_last_error(), (word, rc, lib.cfs_hip_last_error())
        torch.cuda.synchronize()
        assert bool(torch.all(X == -777.25)) and list(w) == [7.0] * 4 and list(res) == [7.0] * 4
    for debug in (False, True):
        refused(_lib.ERR_ARG, b"null", a=None, debug=debug)
        refused(_lib.ERR_ARG, b"another handle", h=A2, debug=debug)
        refused(_lib.ERR_ARG, b"value type", a=Go, debug=debug)
        refused(_lib.ERR_ARG, b"bad k", k=0, debug=debug)
        refused(_lib.ERR_ARG, b"bad k", k=17, debug=debug)
    # 3 k > n
    m, rp3, ci3, va3 = _case("rand3", dtype, k=1)[:4]
    B = cfs.SymMatrix(m, rp3, ci3, va3)
    GB = B.amg(rp3, ci3, va3, coarse_max=1)
    refused(_lib.ERR_ARG, b"bad k", h=B, a=GB, k=2)
    GB.close()
    B.close()
    # a shard, and a multi-device handle
    S = cfs.SymMatrix(n, rp, ci, va, row_splits=np.array([0, n // 2, n], np.int32), rank=1)
    refused(_lib.ERR_UNSUPPORTED, b"shard", h=S)
    S.close()
    if torch.cuda.device_count() >= 2:
        M = cfs.SymMatrix(n, rp, ci, va, ngpus=2)
        refused(_lib.ERR_UNSUPPORTED, b"multi-device", h=M)
        M.close()
    # a hierarchy whose last refresh failed
    rows = np.repeat(np.arange(n), np.diff(rp))
    zero = np.array(va)
    zero[int(np.flatnonzero((rows == ci) & (rows == 40))[0])] = 0.0
    with pytest.raises(_lib.CfsHipError):
        G.update_values(zero)
    refused(_lib.ERR_ARG, b"the last refresh failed")
    refused(_lib.ERR_ARG, b"the last refresh failed", debug=True)
    G.update_values(np.array(va))
    wv, Xv, info = A.lobpcg(k=4, precond=G, tol=TOL[dtype], scale=lmax)
    assert info["nconv"] == 4
    with pytest.raises(ValueError, match="another matrix"):
        A2.lobpcg(k=4, precond=G, scale=lmax)
    for Z in (G, Go):
        Z.close()
    for Z in (A, A2, Ao):
        Z.close()
