"""cfs_hip_sym_lobpcg, the whole solver: LOBPCG on the GPU against a reference spectrum -- dense numpy.linalg.eigvalsh for
n <= 1026, scipy.sparse.linalg.eigsh(A64, k + 1, sigma=0) above (each of its eigenvalues re-evaluated as the long-double
Rayleigh quotient of its own vector, the _case idea of test_gpu_eigs.py) -- of the matrix as the library holds it (the
values rounded to the value type).  lap2d(nx, ny) = 1 kron(I, T_nx) + 0.37 kron(T_ny, I), T = tridiag(-1, 2, -1);
"scaled" is D A D with D = 10^uniform(-1, 1), seed n.  k = 4 and the library's own start block unless a case says
otherwise; `scale` is lmax of the reference, so the stopping rule is the one the assertions are written in.

With r_i = ||A x_i - theta_i x_i||_2 / ||x_i||_2 recomputed HERE in long double from the returned x_i and theta_i:

    nconv == k;   r_i <= 2 tol lmax;   |theta_i - lambda_i| <= r_i + 16 u lmax   (u = 2^-53 / 2^-24);
    the library's residuals within 4 u lmax + 1e-3 r_i of r_i

The factor 2 covers the rounding of the product the solver's own confirm step recomputes AX with.  Comparing with lambda_i
BY INDEX is what catches a solver that skips an eigenvalue; the test first asserts from the reference spectrum that
lambda_1 .. lambda_{k+1} are pairwise either apart by more than 4 tol lmax or equal to within 16 u lmax.  The second
case is rand257: its five rows that hold only a diagonal entry make 1.0 a five-fold eigenvalue, the whole wanted end, for
which every index names the same number and the comparison by index stays exact; no tolerance makes a gap of 0 exceed
4 tol lmax.  tol per case: fp64 1e-10 throughout; fp32 5e-5 on lap2d(40, 33) (gaps 3.5e-4 lmax) and 1e-4 elsewhere
(gaps at least 7.5e-4 lmax); the scaled lap2d(40, 33) has gaps of 5e-7 lmax, below what fp32 resolves: fp64 only.

Measured on the MI355X (value type, case: iterations, products, nconv, r = max r_i / (tol lmax), dtheta = max |theta_i -
lambda_i| / lmax, and how far the library's residuals are from r_i):

  f64 lap2d(16,15) n=240 k=4 none: iterations 108, products 356, nconv 4, max r/(tol lmax) 0.900, max |theta - lambda|/lmax 6.29e-16, library residuals off by 2.57e-18 lmax
  f32 lap2d(16,15) n=240 k=4 none: iterations 44, products 145, nconv 4, max r/(tol lmax) 0.994, max |theta - lambda|/lmax 9.70e-08, library residuals off by 1.17e-09 lmax
  f64 lap2d(16,15) n=240 k=4 jacobi: iterations 108, products 356, nconv 4, max r/(tol lmax) 0.900, max |theta - lambda|/lmax 4.38e-15, library residuals off by 3.81e-18 lmax
  f32 lap2d(16,15) n=240 k=4 jacobi: iterations 44, products 145, nconv 4, max r/(tol lmax) 0.993, max |theta - lambda|/lmax 8.97e-08, library residuals off by 2.45e-09 lmax
  f64 lap2d(16,15) n=240 k=4 block3: iterations 74, products 243, nconv 4, max r/(tol lmax) 0.872, max |theta - lambda|/lmax 1.33e-15, library residuals off by 2.62e-18 lmax
  f32 lap2d(16,15) n=240 k=4 block3: iterations 29, products 100, nconv 4, max r/(tol lmax) 0.842, max |theta - lambda|/lmax 6.20e-08, library residuals off by 8.99e-10 lmax
  f64 lap2d(40,33) n=1320 k=4 jacobi: iterations 352, products 871, nconv 4, max r/(tol lmax) 0.944, max |theta - lambda|/lmax 4.06e-17, library residuals off by 1.78e-18 lmax
  f32 lap2d(40,33) n=1320 k=4 jacobi: iterations 110, products 358, nconv 4, max r/(tol lmax) 0.991, max |theta - lambda|/lmax 2.97e-07, library residuals off by 3.75e-10 lmax
  f64 lap2d(40,33) scaled n=1320 k=4 jacobi: iterations 330, products 734, nconv 4, max r/(tol lmax) 0.902, max |theta - lambda|/lmax 1.04e-18, library residuals off by 2.41e-20 lmax
  f64 rand257 n=257 k=4 jacobi: iterations 44, products 178, nconv 4, max r/(tol lmax) 0.740, max |theta - lambda|/lmax 1.18e-16, library residuals off by 4.36e-24 lmax
  f32 rand257 n=257 k=4 jacobi: iterations 16, products 64, nconv 4, max r/(tol lmax) 0.875, max |theta - lambda|/lmax 7.18e-08, library residuals off by 1.45e-12 lmax
  f64 band20001 n=20001 k=4 jacobi: iterations 308, products 644, nconv 4, max r/(tol lmax) 0.989, max |theta - lambda|/lmax 1.91e-16, library residuals off by 2.24e-19 lmax
  f32 band20001 n=20001 k=4 jacobi: iterations 77, products 217, nconv 4, max r/(tol lmax) 0.911, max |theta - lambda|/lmax 2.33e-07, library residuals off by 3.69e-11 lmax
  f64 rand3 n=3 k=1 jacobi: iterations 2, products 4, nconv 1, max r/(tol lmax) 0.000, max |theta - lambda|/lmax 1.75e-16, library residuals off by 7.50e-18 lmax
  f64 lap2d(16,15) n=240 k=16 jacobi: iterations 98, products 811, nconv 16, max r/(tol lmax) 0.890, max |theta - lambda|/lmax 1.59e-15, library residuals off by 5.09e-18 lmax
  f32 rand3 n=3 k=1 jacobi: iterations 2, products 4, nconv 1, max r/(tol lmax) 0.000, max |theta - lambda|/lmax 1.40e-08, library residuals off by 6.86e-10 lmax
  f32 lap2d(16,15) n=240 k=16 jacobi: iterations 37, products 352, nconv 16, max r/(tol lmax) 0.935, max |theta - lambda|/lmax 9.94e-08, library residuals off by 1.73e-09 lmax
  f64 band600001 n=600001 k=2 jacobi: iterations 264, products 498, nconv 2, max r/(tol lmax) 0.931, max |theta - lambda|/lmax 3.74e-16, library residuals off by 7.73e-20 lmax
  f32 band600001 n=600001 k=2 jacobi: iterations 97, products 176, nconv 2, max r/(tol lmax) 0.985, max |theta - lambda|/lmax 3.27e-07, library residuals off by 1.11e-11 lmax
  f64 band20001 (two shards) n=20001 k=4 none: iterations 225, products 611, nconv 4, max r/(tol lmax) 0.936, max |theta - lambda|/lmax 3.35e-16, library residuals off by 3.54e-19 lmax
  f32 band20001 (two shards) n=20001 k=4 none: iterations 74, products 231, nconv 4, max r/(tol lmax) 0.891, max |theta - lambda|/lmax 2.51e-07, library residuals off by 7.06e-11 lmax
  f64 band20001 (two shards) n=20001 k=4 jacobi: iterations 308, products 644, nconv 4, max r/(tol lmax) 0.989, max |theta - lambda|/lmax 3.11e-16, library residuals off by 2.38e-19 lmax
  f32 band20001 (two shards) n=20001 k=4 jacobi: iterations 77, products 217, nconv 4, max r/(tol lmax) 0.910, max |theta - lambda|/lmax 1.99e-07, library residuals off by 4.50e-11 lmax
  f64 lap2d(16,15), x0 with a repeated column n=240 k=4 jacobi: iterations 129, products 400, nconv 4, max r/(tol lmax) 0.981, max |theta - lambda|/lmax 1.36e-15, library residuals off by 2.35e-18 lmax
  f32 lap2d(16,15), x0 with a repeated column n=240 k=4 jacobi: iterations 49, products 160, nconv 4, max r/(tol lmax) 0.920, max |theta - lambda|/lmax 7.19e-08, library residuals off by 1.00e-09 lmax

and, from the other tests:

  f64 lap2d(40,33) scaled, maxiter 200: none nconv 0, iterations 200, products 808; jacobi nconv 3, iterations 200, products 604
  f64 Flan_1565@0.01 (deterministic): theta [1.65893712 2.07328502 2.35829972 2.562277  ], iterations 10, nconv 0
  f32 Flan_1565@0.01 (deterministic): theta [1.65893706 2.07328506 2.35829984 2.56227698], iterations 10, nconv 0
  f64 lap2d(16,15): host-driven [0.04827269 0.09038295 0.14927443 0.15876629] (108 iterations, 356 products), native [0.04827269 0.09038295 0.14927443 0.15876629] (108 iterations, 356 products)
  f32 lap2d(16,15): host-driven [0.04827271 0.09038313 0.14927455 0.15876683] (44 iterations, 145 products), native [0.04827271 0.09038311 0.14927455 0.15876678] (44 iterations, 145 products)
"""
import ctypes as C
import functools

import numpy as np
import pytest

from test_gpu_cg_steps import DET, DTYPES, UNIT, _matrix
from test_gpu_kernel_variants import PLAN_KNOBS
from test_gpu_lobpcg_steps import matrix

pytestmark = pytest.mark.gpu

TOL = {np.float64: 1e-10, np.float32: 1e-4}
TOL_LAP40 = {np.float64: 1e-10, np.float32: 5e-5}


@pytest.fixture(autouse=True)
def _torch_first(monkeypatch):
    """torch brings a HIP runtime of its own: it has to initialise before libcfs_hip.so's"""
    import torch
    torch.cuda.init()
    torch.cuda.set_device(0)
    for k in PLAN_KNOBS:
        monkeypatch.delenv(k, raising=False)
    yield


def scaled(n, rp, ci, va):
    import scipy.sparse as sp
    A = sp.csr_matrix((np.asarray(va, np.float64), ci, rp), shape=(n, n))
    D = sp.diags(10.0 ** np.random.default_rng(n).uniform(-1, 1, n))
    A = (D @ A @ D).tocsr()
    A.sort_indices()
    return n, A.indptr.astype(np.int32), A.indices.astype(np.int32), A.data


@functools.lru_cache(maxsize=None)
def _case(name, dtype, k=4):
    """(n, rp, ci, va in the value type, the k + 1 smallest reference eigenvalues (fewer when n says so), lmax); a name
    ending in "-scaled" is the scaled matrix.  Computed once, shared, unchanged"""
    import scipy.sparse as sp
    import scipy.sparse.linalg as spl
    n, rp, ci, va = scaled(*matrix(name[:-7])) if name.endswith("-scaled") else matrix(name)
    va = np.asarray(va).astype(dtype)
    A64 = sp.csr_matrix((va.astype(np.float64), ci, rp), shape=(n, n))
    if n <= 1026:
        lam = np.linalg.eigvalsh(A64.toarray())
        lmax = float(np.max(np.abs(lam)))
        lam = lam[:k + 1].copy()
    else:
        from oracle import oracle
        lam, Q = spl.eigsh(A64.tocsc(), k + 1, sigma=0, which="LM")
        for i in range(k + 1):
            x = Q[:, i].astype(np.longdouble)
            lam[i] = float(np.dot(x, oracle.csr_spmv_ldx(n, rp, ci, va, x)) / np.dot(x, x))
        lam = np.sort(lam)
        lmax = float(np.max(np.abs(spl.eigsh(A64, 1, which="LM", tol=1e-9, return_eigenvectors=False))))
    for x in (rp, ci, va, lam):
        x.setflags(write=False)
    return n, rp, ci, va, lam, lmax


def _residuals(n, rp, ci, va, w, X):
    """r_i in long double from the returned pairs (X: (n, k) numpy)"""
    from oracle import oracle
    out = []
    for i in range(len(w)):
        x = X[:, i].astype(np.longdouble)
        d = oracle.csr_spmv_ldx(n, rp, ci, va, x) - np.longdouble(w[i]) * x
        out.append(float(np.sqrt(np.dot(d, d)) / np.sqrt(np.dot(x, x))))
    return np.array(out)


def _solve(A, **kw):
    import torch
    w, X, info = A.lobpcg(**kw)
    torch.cuda.synchronize()
    return w, np.ascontiguousarray(X.cpu().numpy()), info


def _kw(precond):
    return dict(precond="block_jacobi", block=3) if precond == "block3" else dict(precond=precond)


def _check(label, case, dtype, A, tol, k=4, precond="jacobi", maxiter=500, x0=None):
    n, rp, ci, va, lam, lmax = case
    u = UNIT[dtype]
    gaps = np.diff(lam)
    assert len(lam) == min(k + 1, n) and np.all((gaps > 4 * tol * lmax) | (gaps <= 16 * u * lmax)), f"{label}: badly chosen case, gaps {gaps}"
    w, X, info = _solve(A, k=k, tol=tol, scale=lmax, maxiter=maxiter, x0=x0, **_kw(precond))
    assert w.shape == (k,) and w.dtype == np.float64 and X.shape == (n, k)
    r = _residuals(n, rp, ci, va, w, X)
    print(f"lobpcg {np.dtype(dtype).name} {label} n={n} k={k} {precond}: iterations {info['iterations']}, products "
          f"{info['products']}, nconv {info['nconv']}, max r/(tol lmax) {np.max(r) / (tol * lmax):.3f}, "
          f"max |theta - lambda|/lmax {np.max(np.abs(w - lam[:k])) / lmax:.2e}, library residuals off by "
          f"{np.max(np.abs(info['residuals'] - r)) / lmax:.2e} lmax")
    errors = []
    if info["nconv"] != k:
        errors.append(f"nconv = {info['nconv']}")
    if not np.all(np.diff(w) >= 0):
        errors.append(f"theta not ascending: {w}")
    for i in range(k):
        if not r[i] <= 2 * tol * lmax:
            errors.append(f"r_{i} = {r[i]:.3e} > 2 tol lmax = {2 * tol * lmax:.3e}")
        if not abs(w[i] - lam[i]) <= r[i] + 16 * u * lmax:
            errors.append(f"theta_{i} = {w[i]!r}, lambda_{i} = {lam[i]!r}: apart by more than r_i + 16 u lmax = {r[i] + 16 * u * lmax:.3e}")
        if not abs(info["residuals"][i] - r[i]) <= 4 * u * lmax + 1e-3 * r[i]:
            errors.append(f"residuals[{i}] = {info['residuals'][i]:.3e}, recomputed {r[i]:.3e}")
    assert not errors, f"{label} {np.dtype(dtype).name}: " + "; ".join(errors)
    return w, X, info


@DTYPES
@pytest.mark.parametrize("precond", ["none", "jacobi", "block3"])
def test_lap2d_16_15(precond, dtype):
    import cfs_spmv_amd as cfs
    case = _case("lap2d16x15", dtype)
    A = cfs.SymMatrix(*case[:4])
    _check("lap2d(16,15)", case, dtype, A, TOL[dtype], precond=precond)
    A.close()


@DTYPES
def test_lap2d_40_33(dtype):
    import cfs_spmv_amd as cfs
    case = _case("lap2d40x33", dtype)
    A = cfs.SymMatrix(*case[:4])
    _check("lap2d(40,33)", case, dtype, A, TOL_LAP40[dtype], maxiter=1000)
    A.close()


def test_lap2d_40_33_scaled_with_jacobi():
    """rows of mixed scale, fp64 (the low gaps are 5e-7 lmax): the case the preconditioner exists for"""
    import cfs_spmv_amd as cfs
    case = _case("lap2d40x33-scaled", np.float64)
    A = cfs.SymMatrix(*case[:4])
    _check("lap2d(40,33) scaled", case, np.float64, A, 1e-10, maxiter=1000)
    A.close()


@DTYPES
@pytest.mark.parametrize("name", ["rand257", "band20001"])
def test_dominant_matrices(name, dtype):
    import cfs_spmv_amd as cfs
    case = _case(name, dtype)
    A = cfs.SymMatrix(*case[:4])
    _check(name, case, dtype, A, TOL[dtype])
    A.close()


@DTYPES
def test_the_edges_of_k(dtype):
    """k = 1 on n = 3, the 3 k <= n edge; k = 16 on lap2d(16, 15), the cap: 48 columns in S"""
    import cfs_spmv_amd as cfs
    case = _case("rand3", dtype, k=1)
    A = cfs.SymMatrix(*case[:4])
    _check("rand3", case, dtype, A, TOL[dtype], k=1)
    A.close()
    case = _case("lap2d16x15", dtype, k=16)
    A = cfs.SymMatrix(*case[:4])
    _check("lap2d(16,15)", case, dtype, A, TOL[dtype], k=16)
    A.close()


@DTYPES
def test_beyond_one_grid_stride_sweep(dtype):
    """band600001, k = 2: n lies beyond one sweep of the vector kernels' grid and has an odd tail"""
    import cfs_spmv_amd as cfs
    case = _case("band600001", dtype, k=2)
    A = cfs.SymMatrix(*case[:4])
    _check("band600001", case, dtype, A, TOL[dtype], k=2)
    A.close()


@DTYPES
@pytest.mark.parametrize("precond", ["none", "jacobi"])
def test_through_a_two_shard_handle(precond, dtype):
    import cfs_spmv_amd as cfs
    from cfs_spmv_amd import _lib
    case = _case("band20001", dtype)
    M = cfs.SymMatrix(*case[:4], ngpus=2)
    _check("band20001 (two shards)", case, dtype, M, TOL[dtype], precond=precond)
    with pytest.raises(_lib.CfsHipError) as e:
        M.lobpcg(k=4, precond="block_jacobi", block=3, scale=case[5])
    assert e.value.code == _lib.ERR_UNSUPPORTED
    M.close()


def test_the_scaled_case_without_and_with_the_preconditioner():
    """lap2d(40, 33) scaled, fp64, maxiter = 200: without a preconditioner the call returns 0 with nconv < k and finite
    outputs; Jacobi issues fewer products than that run, at the same maxiter"""
    import cfs_spmv_amd as cfs
    n, rp, ci, va, lam, lmax = _case("lap2d40x33-scaled", np.float64)
    A = cfs.SymMatrix(n, rp, ci, va)
    w0, X0, i0 = _solve(A, k=4, precond="none", tol=1e-10, scale=lmax, maxiter=200)
    w1, X1, i1 = _solve(A, k=4, precond="jacobi", tol=1e-10, scale=lmax, maxiter=200)
    A.close()
    print(f"lobpcg f64 lap2d(40,33) scaled, maxiter 200: none nconv {i0['nconv']}, iterations {i0['iterations']}, products "
          f"{i0['products']}; jacobi nconv {i1['nconv']}, iterations {i1['iterations']}, products {i1['products']}")
    assert i0["nconv"] < 4 and i0["iterations"] == 200
    assert np.all(np.isfinite(w0)) and np.all(np.isfinite(X0)) and np.all(np.isfinite(i0["residuals"])) and np.all(np.diff(w0) >= 0)
    assert i1["products"] < i0["products"]


@DTYPES
def test_a_deterministic_handle_is_bit_reproducible(dtype):
    """Flan_1565@0.01, block Jacobi on the node blocks, maxiter = 10: two runs bit-equal in theta, X, residuals, counters"""
    import cfs_spmv_amd as cfs
    n, rp, ci, va = _matrix("Flan_1565@0.01")
    D = cfs.SymMatrix(n, rp, ci, va.astype(dtype), options=cfs.make_options(flags=DET))
    assert D.kernel_variant()["det"] == 1
    kw = dict(k=4, precond="block_jacobi", block=3, tol=TOL[dtype], scale=1.0, maxiter=10)
    w1, X1, i1 = _solve(D, **kw)
    w2, X2, i2 = _solve(D, **kw)
    D.close()
    print(f"lobpcg {np.dtype(dtype).name} Flan_1565@0.01 (deterministic): theta {w1}, iterations {i1['iterations']}, nconv {i1['nconv']}")
    assert np.all(np.isfinite(w1)) and np.all(np.diff(w1) >= 0) and i1["iterations"] == 10
    assert np.array_equal(w1.view(np.uint8), w2.view(np.uint8)) and np.array_equal(X1.view(np.uint8), X2.view(np.uint8))
    assert (i1["nconv"], i1["iterations"], i1["products"]) == (i2["nconv"], i2["iterations"], i2["products"])
    assert np.array_equal(i1["residuals"].view(np.uint8), i2["residuals"].view(np.uint8))


@DTYPES
def test_a_start_block_with_two_identical_columns(dtype):
    """the drop rule keeps the first Rayleigh-Ritz step regular; the dependent column is replaced and the solve converges"""
    import torch
    import cfs_spmv_amd as cfs
    from cfs_spmv_amd.solver import default_x0
    case = _case("lap2d16x15", dtype)
    x0 = default_x0(case[0], 4, dtype)
    x0[:, 2] = x0[:, 0]
    A = cfs.SymMatrix(*case[:4])
    _check("lap2d(16,15), x0 with a repeated column", case, dtype, A, TOL[dtype], x0=torch.from_numpy(x0).cuda())
    A.close()


@DTYPES
def test_error_paths(dtype):
    import scipy.sparse as sp
    import torch
    import cfs_spmv_amd as cfs
    from cfs_spmv_amd import _lib
    n, rp, ci, va = _case("rand257", dtype)[:4]

    def refused(M, code, word, **kw):
        with pytest.raises(_lib.CfsHipError, match=word) as e:
            M.lobpcg(**dict(dict(k=4, tol=1e-6, scale=1.0, maxiter=5), **kw))
        assert e.value.code == code, (kw, e.value)
    A = cfs.SymMatrix(n, rp, ci, va)
    refused(A, _lib.ERR_ARG, "bad k", k=17)
    refused(A, _lib.ERR_ARG, "bad k", k=0)
    refused(A, _lib.ERR_ARG, "block_rows", precond="block_jacobi", block=5)
    refused(A, _lib.ERR_ARG, "tolerance", scale=0.0)
    with pytest.raises(ValueError):
        A.lobpcg(k=2, precond="ilu", scale=1.0)
    # a host pointer, 16-byte aligned, as x0 and as the vectors: straight through the C entry point
    lib = cfs.load()
    per = 16 // np.dtype(dtype).itemsize
    ld = -(-n // per) * per
    host = np.zeros(4 * ld + 8, dtype)
    host = host[(-host.ctypes.data % 16) // host.itemsize:][:4 * ld]
    dev = torch.zeros(4 * ld, dtype=torch.float64 if dtype == np.float64 else torch.float32, device="cuda")
    w = (C.c_double * 4)()
    cnt = [C.c_int(7) for _ in range(3)]
    for x0p, xp in ((host.ctypes.data, dev.data_ptr()), (None, host.ctypes.data)):
        rc = lib.cfs_hip_sym_lobpcg(A._h, 4, 1, 1e-6, 1.0, 5, x0p, ld, w, xp, ld, None, *(C.byref(c) for c in cnt), None)
        assert rc == _lib.ERR_ARG and b"device pointer" in lib.cfs_hip_last_error()
        assert [c.value for c in cnt] == [0, 0, 0] and not host.any() and not bool(dev.any())
    A.close()
    # 3 k > n
    m, rp2, ci2, va2 = _matrix("rand5")
    B = cfs.SymMatrix(m, rp2, ci2, va2.astype(dtype))
    refused(B, _lib.ERR_ARG, "bad k", k=2)
    B.close()
    # a shard
    S = cfs.SymMatrix(n, rp, ci, va, row_splits=np.array([0, n // 2, n], np.int32), rank=1)
    refused(S, _lib.ERR_UNSUPPORTED, "shard")
    S.close()
    # a diagonal entry that is zero, or NaN, with Jacobi; an indefinite 3 x 3 block with block Jacobi: nothing written
    M = sp.lil_matrix(sp.csr_matrix((va.astype(np.float64), ci, rp), shape=(n, n)))
    for bad, kw, word in ((0.0, dict(precond="jacobi"), "positive diagonal"), (np.nan, dict(precond="jacobi"), "positive diagonal"),
                          (None, dict(precond="block_jacobi", block=3), "positive definite")):
        Mb = M.copy()
        if bad is None:
            Mb[30, 31] = Mb[31, 30] = 4.0 * max(Mb[30, 30], Mb[31, 31])  # a 2 x 2 minor with a negative determinant
        else:
            Mb[100, 100] = bad
        Mb = Mb.tocsr()
        Mb.sort_indices()
        Z = cfs.SymMatrix(n, Mb.indptr.astype(np.int32), Mb.indices.astype(np.int32), Mb.data.astype(dtype))
        refused(Z, _lib.ERR_ARG, word, **kw)
        if bad == 0.0:  # without the preconditioner the matrix is as good as any
            assert Z.lobpcg(k=2, precond="none", tol=1e-3, scale=1.0, maxiter=3)[2]["iterations"] <= 3
        Z.close()


@DTYPES
def test_host_driven_and_native_loops_agree(dtype):
    """solver.lobpcg (torch-driven) against solver.lobpcg_native on lap2d(16, 15) with Jacobi: theta within the sum of the
    two runs' residuals"""
    import torch
    import cfs_spmv_amd as cfs
    from cfs_spmv_amd.solver import lobpcg, lobpcg_native
    n, rp, ci, va, lam, lmax = _case("lap2d16x15", dtype)
    A = cfs.SymMatrix(n, rp, ci, va)
    w1, X1, i1 = lobpcg(A, 4, tol=TOL[dtype], scale=lmax)
    w2, X2, i2 = lobpcg_native(A, 4, tol=TOL[dtype], scale=lmax)
    torch.cuda.synchronize()
    A.close()
    print(f"lobpcg {np.dtype(dtype).name} lap2d(16,15): host-driven {w1} ({i1['iterations']} iterations, {i1['products']} products), "
          f"native {w2} ({i2['iterations']} iterations, {i2['products']} products)")
    assert i1["nconv"] == i2["nconv"] == 4 and X1.shape == X2.shape == (n, 4)
    assert np.all(np.abs(w1 - w2) <= i1["residuals"] + i2["residuals"])
