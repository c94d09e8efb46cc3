"""cfs_hip_sym_lobpcg_gen, the whole solver for the pencil A x = lambda B x, on the GPU, in the structure of
test_gpu_lobpcg.py.  A = lap2d(nx, ny) of the tests; B = M_ny kron M_nx with M = tridiag(1, 4, 1) / 6, the consistent mass
matrix of linear elements, or its lumped form diag(B 1).  The reference is scipy.linalg.eigh(A64, B64) of the matrices as
the library holds them (the values rounded to the value type); lmax = lambda_max(A), bmin = lambda_min(B) (0.115 for
(16, 15), 0.112 for (40, 33), 0.694 lumped).  band20001 runs with a seeded diagonal B = diag(uniform(0.5, 2)); its
reference is scipy.sparse.linalg.eigsh(A, k + 1, M=B, sigma=0), each value re-evaluated as the long-double Rayleigh
quotient x^T A x / x^T B x of its own vector.

With r_i = ||A x_i - theta_i B x_i||_2 / ||x_i||_2 recomputed HERE in long double with the oracle's product:

    nconv == k;   r_i <= 2 tol lmax;   |theta_i - lambda_i| <= r_i / bmin + 16 u lambda_max(A, B);
    the library's residuals within 4 u lmax + 1e-3 r_i of r_i

The third is the residual bound of a pencil: ||r||_{B^-1} / ||x||_B <= ||r||_2 / (bmin ||x||_2).  The test first asserts
from the reference that lambda_1 .. lambda_{k+1} are apart by more than 4 tol lmax / bmin, so that comparing BY INDEX
catches a solver that skips an eigenvalue.  Gaps: lap2d(16,15) k = 4 2.8e-3 lmax, k = 16 3.8e-4 lmax, lap2d(40,33) 3.3e-4
lmax, lumped 2.0e-3 lmax.  tol: fp64 1e-10, fp32 5e-5.

X is B-orthonormal: max |X^T B X - I| in long double is at most 8 x the same figure of the host model
solver.lobpcg(A, k, B=B) on the same case, plus 16 u_V; the host model is the reference there, not the native code.

Measured on the MI355X (products with A = products with B in every run):

  f64 lap2d(16,15) n=240 k=4 none: iterations 131, products 387, max r/(tol lmax) 0.974, max |theta - lambda|/lmax 1.94e-15
  f32 lap2d(16,15) n=240 k=4 none: iterations 52, products 163, max r/(tol lmax) 0.966, max |theta - lambda|/lmax 2.19e-08
  f64 lap2d(16,15) n=240 k=4 jacobi: iterations 131, products 387, max r/(tol lmax) 0.974, max |theta - lambda|/lmax 1.94e-15, library residuals off by 2.17e-18 lmax
  f32 lap2d(16,15) n=240 k=4 jacobi: iterations 52, products 163, max r/(tol lmax) 0.967, max |theta - lambda|/lmax 2.22e-08, library residuals off by 1.16e-09 lmax
  f64 lap2d(16,15) n=240 k=4 block3: iterations 88, products 253, max r/(tol lmax) 0.676, max |theta - lambda|/lmax 1.95e-15
  f32 lap2d(16,15) n=240 k=4 block3: iterations 31, products 105, max r/(tol lmax) 0.949, max |theta - lambda|/lmax 3.14e-08
  f64 lap2d(16,15) n=240 k=16 jacobi: iterations 95, products 802, nconv 16, max r/(tol lmax) 0.863, max |theta - lambda|/lmax 1.96e-15
  f64 lap2d(40,33) n=1320 k=4 jacobi: iterations 497, products 995, max r/(tol lmax) 0.968, max |theta - lambda|/lmax 2.12e-15
  f64 lap2d(40,33) n=1320 k=4 multigrid: iterations 51, products 131, cycles 131, max r/(tol lmax) 0.628
  f64 lap2d(16,15) lumped n=240 k=4 jacobi: iterations 128, products 394, max r/(tol lmax) 0.906, max |theta - lambda|/lmax 1.28e-15
  f32 lap2d(16,15) lumped n=240 k=4 jacobi: iterations 53, products 167, max r/(tol lmax) 0.757, max |theta - lambda|/lmax 2.02e-08
  f64 band20001 diagonal B n=20001 k=4 jacobi: iterations 161, products 510, max r/(tol lmax) 0.991, max |theta - lambda|/lmax 9.57e-17
  f32 band20001 diagonal B n=20001 k=4 jacobi: iterations 61, products 206, max r/(tol lmax) 0.987, max |theta - lambda|/lmax 2.78e-08
  max |X^T B X - I|: f64 native 3.42e-15, host model 1.50e-15 (16 u_V 1.78e-15); f32 native 1.74e-07, host model 1.66e-07 (16 u_V 9.54e-07)
  B = I: theta and the iteration count (108 fp64, 48 fp32) of the standard solver; B = A: |theta - 1| <= 6.7e-16, 0 iterations
  host-driven and native: 131 iterations and 387 + 387 products each in fp64, 52 and 163 + 163 in fp32, theta equal to 8 digits
  Flan_1565@0.01 with its lumped mass (deterministic), 10 iterations: theta 1.3808688 1.68501544 2.22811585 2.35550869, two runs bit-equal"""
import ctypes as C
import functools

import numpy as np
import pytest

from test_gpu_cg_steps import DET, DTYPES, UNIT, _matrix
from test_gpu_kernel_variants import PLAN_KNOBS
from test_gpu_lobpcg_steps import matrix

pytestmark = pytest.mark.gpu

LD = np.longdouble
TOL = {np.float64: 1e-10, np.float32: 5e-5}


@pytest.fixture(autouse=True)
def _torch_first(monkeypatch):
    """torch brings a HIP runtime of its own: it has to initialise before libcfs_hip.so's"""
    import torch
    torch.cuda.init()
    torch.cuda.set_device(0)
    for k in PLAN_KNOBS:
        monkeypatch.delenv(k, raising=False)
    yield


def _csr(M, dtype):
    M = M.tocsr()
    M.sort_indices()
    return M.shape[0], M.indptr.astype(np.int32), M.indices.astype(np.int32), M.data.astype(dtype)


def mass(nx, ny, kind):
    """M_ny kron M_nx, M = tridiag(1, 4, 1) / 6 ("consistent"), or diag of its row sums ("lumped"), as scipy CSR"""
    import scipy.sparse as sp
    M = lambda n: sp.diags([np.ones(n - 1), 4 * np.ones(n), np.ones(n - 1)], [-1, 0, 1]) / 6.0
    B = sp.kron(M(ny), M(nx)).tocsr()
    return sp.diags(np.asarray(B.sum(axis=1)).ravel()).tocsr() if kind == "lumped" else B


@functools.lru_cache(maxsize=None)
def _case(name, dtype, k=4, kind="consistent"):
    """dict(A, B: (n, rp, ci, va in the value type), lam: the k + 1 smallest reference eigenvalues, lmax, bmin, pmax =
    lambda_max(A, B)).  kind: "consistent" / "lumped" (lap2d only), "diag" (a seeded diagonal), "identity", "minus".
    Computed once, shared, unchanged"""
    import scipy.linalg
    import scipy.sparse as sp
    import scipy.sparse.linalg as spl
    n, rp, ci, va = matrix(name)
    va = np.asarray(va).astype(dtype)
    if kind in ("consistent", "lumped"):
        Bm = mass(*(int(x) for x in name[5:].split("x")), kind)
    elif kind == "diag":
        Bm = sp.diags(np.random.default_rng(n).uniform(0.5, 2.0, n)).tocsr()
    else:
        Bm = sp.identity(n, format="csr") * (1.0 if kind == "identity" else -1.0)
    Bc = _csr(Bm, dtype)
    A64 = sp.csr_matrix((va.astype(np.float64), ci, rp), shape=(n, n))
    B64 = sp.csr_matrix((Bc[3].astype(np.float64), Bc[2], Bc[1]), shape=(n, n))
    out = dict(A=(n, rp, ci, va), B=Bc)
    if kind == "minus":
        return out
    if n <= 1400:
        lamA = np.linalg.eigvalsh(A64.toarray())
        lam = scipy.linalg.eigh(A64.toarray(), B64.toarray(), eigvals_only=True)
        out.update(lmax=float(np.max(np.abs(lamA))), bmin=float(np.linalg.eigvalsh(B64.toarray())[0]), pmax=float(np.max(np.abs(lam))),
                   lam=lam[:k + 1].copy())
    else:
        from oracle import oracle
        lam, Q = spl.eigsh(A64.tocsc(), k + 1, M=B64.tocsc(), sigma=0, which="LM")
        for i in range(k + 1):
            x = Q[:, i].astype(LD)
            lam[i] = float(np.dot(x, oracle.csr_spmv_ldx(n, rp, ci, va, x)) / np.dot(x, oracle.csr_spmv_ldx(*Bc, x)))
        out.update(lam=np.sort(lam), lmax=float(np.max(np.abs(spl.eigsh(A64, 1, which="LM", tol=1e-9, return_eigenvectors=False)))),
                   bmin=float(np.min(B64.diagonal())),
                   pmax=float(np.max(np.abs(spl.eigsh(A64, 1, M=B64.tocsc(), which="LM", tol=1e-9, return_eigenvectors=False)))))
    for x in (rp, ci, va, *Bc[1:], out["lam"]):
        x.setflags(write=False)
    return out


def _residuals(case, w, X):
    """r_i in long double from the returned pairs (X: (n, k) numpy)"""
    from oracle import oracle
    out = []
    for i in range(len(w)):
        x = X[:, i].astype(LD)
        d = oracle.csr_spmv_ldx(*case["A"], x) - LD(w[i]) * oracle.csr_spmv_ldx(*case["B"], x)
        out.append(float(np.sqrt(np.dot(d, d)) / np.sqrt(np.dot(x, x))))
    return np.array(out)


def _b_orthonormality(case, X):
    """max |X^T B X - I| in long double"""
    from oracle import oracle
    Xl = X.astype(LD)
    BX = np.stack([oracle.csr_spmv_ldx(*case["B"], Xl[:, i].copy()) for i in range(X.shape[1])], axis=1)
    return float(np.max(np.abs(Xl.T @ BX - np.eye(X.shape[1]))))


def _solve(A, **kw):
    import torch
    B = kw.pop("B", None)  # (SymMatrix.lobpcg keeps its argument list: the pencil is lobpcg_gen(B, ...))
    w, X, info = A.lobpcg(**kw) if B is None else A.lobpcg_gen(B, **kw)
    torch.cuda.synchronize()
    return w, np.ascontiguousarray(X.cpu().numpy()), info


def _kw(precond):
    return dict(precond="block_jacobi", block=3) if precond == "block3" else dict(precond=precond)


def _handles(case, options=None):
    import cfs_spmv_amd as cfs
    kw = {} if options is None else dict(options=options)
    return cfs.SymMatrix(*case["A"], **kw), cfs.SymMatrix(*case["B"], **kw)


def _check(label, case, dtype, A, B, tol, k=4, precond="jacobi", maxiter=500):
    n, lam, lmax, bmin, pmax = case["A"][0], case["lam"], case["lmax"], case["bmin"], case["pmax"]
    u = UNIT[dtype]
    gaps = np.diff(lam)
    assert len(lam) == k + 1 and np.all(gaps > 4 * tol * lmax / bmin), f"{label}: badly chosen case, gaps {gaps / lmax} lmax"
    w, X, info = _solve(A, k=k, tol=tol, scale=lmax, maxiter=maxiter, B=B, **(_kw(precond) if isinstance(precond, str) else dict(precond=precond)))
    assert w.shape == (k,) and w.dtype == np.float64 and X.shape == (n, k)
    r = _residuals(case, w, X)
    pname = precond if isinstance(precond, str) else "amg"
    print(f"lobpcg_gen {np.dtype(dtype).name} {label} n={n} k={k} {pname}: iterations {info['iterations']}, products {info['products']}, "
          f"b_products {info['b_products']}, nconv {info['nconv']}, max r/(tol lmax) {np.max(r) / (tol * lmax):.3f}, "
          f"max |theta - lambda|/lmax {np.max(np.abs(w - lam[:k])) / lmax:.2e}, library residuals off by "
          f"{np.max(np.abs(info['residuals'] - r)) / lmax:.2e} lmax")
    errors = []
    if info["nconv"] != k:
        errors.append(f"nconv = {info['nconv']}")
    if info["b_products"] != info["products"]:
        errors.append(f"products {info['products']}, b_products {info['b_products']}: every column gets one product of each")
    if not np.all(np.diff(w) >= 0):
        errors.append(f"theta not ascending: {w}")
    for i in range(k):
        if not r[i] <= 2 * tol * lmax:
            errors.append(f"r_{i} = {r[i]:.3e} > 2 tol lmax = {2 * tol * lmax:.3e}")
        if not abs(w[i] - lam[i]) <= r[i] / bmin + 16 * u * pmax:
            errors.append(f"theta_{i} = {w[i]!r}, lambda_{i} = {lam[i]!r}: apart by more than r_i / bmin + 16 u lambda_max(A, B) = "
                          f"{r[i] / bmin + 16 * u * pmax:.3e}")
        if not abs(info["residuals"][i] - r[i]) <= 4 * u * lmax + 1e-3 * r[i]:
            errors.append(f"residuals[{i}] = {info['residuals'][i]:.3e}, recomputed {r[i]:.3e}")
    assert not errors, f"{label} {np.dtype(dtype).name}: " + "; ".join(errors)
    return w, X, info


@DTYPES
@pytest.mark.parametrize("precond", ["none", "jacobi", "block3"])
def test_lap2d_16_15_with_the_consistent_mass(precond, dtype):
    case = _case("lap2d16x15", dtype)
    A, B = _handles(case)
    _check("lap2d(16,15)", case, dtype, A, B, TOL[dtype], precond=precond)
    A.close(), B.close()


def test_lap2d_16_15_at_the_cap_of_k():
    """k = 16: 48 columns in each of the three blocks, a row of the Gram tile at its widest"""
    case = _case("lap2d16x15", np.float64, k=16)
    A, B = _handles(case)
    _check("lap2d(16,15)", case, np.float64, A, B, 1e-10, k=16)
    A.close(), B.close()


def test_lap2d_40_33_with_the_consistent_mass():
    case = _case("lap2d40x33", np.float64)
    A, B = _handles(case)
    _check("lap2d(40,33)", case, np.float64, A, B, 1e-10, maxiter=1000)
    A.close(), B.close()


@DTYPES
def test_lap2d_16_15_with_the_lumped_mass(dtype):
    case = _case("lap2d16x15", dtype, kind="lumped")
    A, B = _handles(case)
    _check("lap2d(16,15) lumped", case, dtype, A, B, TOL[dtype])
    A.close(), B.close()


@DTYPES
def test_band20001_with_a_seeded_diagonal_b(dtype):
    case = _case("band20001", dtype, kind="diag")
    A, B = _handles(case)
    _check("band20001 diagonal B", case, dtype, A, B, TOL[dtype])
    A.close(), B.close()


@DTYPES
def test_the_vectors_are_b_orthonormal(dtype):
    """against the host model on the same case: 8 x its figure plus 16 u_V"""
    from cfs_spmv_amd.solver import lobpcg
    case = _case("lap2d16x15", dtype)
    A, B = _handles(case)
    kw = dict(tol=TOL[dtype], scale=case["lmax"])
    w, X, info = _solve(A, k=4, B=B, **kw)
    wm, Xm, im = lobpcg(A, 4, B=B, **kw)
    A.close(), B.close()
    got, model = _b_orthonormality(case, X), _b_orthonormality(case, np.ascontiguousarray(Xm.cpu().numpy()))
    print(f"lobpcg_gen {np.dtype(dtype).name} lap2d(16,15): max |X^T B X - I| native {got:.3e}, host model {model:.3e}, "
          f"16 u_V {16 * UNIT[dtype]:.3e}")
    assert info["nconv"] == im["nconv"] == 4
    assert got <= 8 * model + 16 * UNIT[dtype]


def test_multigrid_takes_fewer_iterations_than_jacobi():
    """A.lobpcg_gen(B, k=4, precond=G) on lap2d(40, 33), fp64: the same assertions, and fewer iterations than the Jacobi run"""
    case = _case("lap2d40x33", np.float64)
    A, B = _handles(case)
    G = A.amg(*case["A"][1:])
    wj, Xj, ij = _check("lap2d(40,33)", case, np.float64, A, B, 1e-10, maxiter=1000)
    wg, Xg, ig = _check("lap2d(40,33)", case, np.float64, A, B, 1e-10, precond=G, maxiter=1000)
    G.close(), A.close(), B.close()
    print(f"lobpcg_gen f64 lap2d(40,33): jacobi {ij['iterations']} iterations, multigrid {ig['iterations']} iterations, {ig['cycles']} cycles")
    assert ig["iterations"] < ij["iterations"] and ig["cycles"] > 0


@DTYPES
def test_b_the_identity_agrees_with_the_standard_solver(dtype):
    case = _case("lap2d16x15", dtype, kind="identity")
    A, B = _handles(case)
    kw = dict(k=4, tol=TOL[dtype], scale=case["lmax"])
    w1, X1, i1 = _solve(A, B=B, **kw)
    w0, X0, i0 = _solve(A, **kw)
    A.close(), B.close()
    print(f"lobpcg_gen {np.dtype(dtype).name} lap2d(16,15), B = I: {w1} ({i1['iterations']} iterations), standard {w0} ({i0['iterations']})")
    assert i1["nconv"] == i0["nconv"] == 4 and "b_products" not in i0 and i1["b_products"] == i1["products"]
    assert np.all(np.abs(w1 - w0) <= i1["residuals"] + i0["residuals"])


@DTYPES
def test_b_the_handle_of_a_itself(dtype):
    """hb == h: every theta is 1 within 16 u"""
    case = _case("lap2d16x15", dtype, kind="identity")
    A, B = _handles(case)
    B.close()
    w, X, info = _solve(A, k=4, tol=TOL[dtype], scale=case["lmax"], B=A)
    A.close()
    print(f"lobpcg_gen {np.dtype(dtype).name} lap2d(16,15), B = A: theta - 1 = {w - 1.0}, iterations {info['iterations']}")
    assert info["nconv"] == 4 and np.all(np.abs(w - 1.0) <= 16 * UNIT[dtype])


@DTYPES
def test_host_driven_and_native_loops_agree(dtype):
    """solver.lobpcg(B=B) (torch-driven) against solver.lobpcg_native(B=B) on lap2d(16, 15) with Jacobi: theta within the sum
    of the two runs' residuals over bmin"""
    import torch
    from cfs_spmv_amd.solver import lobpcg, lobpcg_native
    case = _case("lap2d16x15", dtype)
    A, B = _handles(case)
    w1, X1, i1 = lobpcg(A, 4, tol=TOL[dtype], scale=case["lmax"], B=B)
    w2, X2, i2 = lobpcg_native(A, 4, tol=TOL[dtype], scale=case["lmax"], B=B)
    torch.cuda.synchronize()
    A.close(), B.close()
    print(f"lobpcg_gen {np.dtype(dtype).name} lap2d(16,15): host-driven {w1} ({i1['iterations']} iterations, {i1['products']} + "
          f"{i1['b_products']} products), native {w2} ({i2['iterations']} iterations, {i2['products']} + {i2['b_products']} products)")
    assert i1["nconv"] == i2["nconv"] == 4 and X1.shape == X2.shape == (case["A"][0], 4)
    assert np.all(np.abs(w1 - w2) <= (i1["residuals"] + i2["residuals"]) / case["bmin"])


@DTYPES
def test_two_deterministic_handles_are_bit_reproducible(dtype):
    """Flan_1565@0.01 and its lumped mass diag(|A| 1) / mean, block Jacobi on the node blocks, maxiter = 10: two runs bit-equal
    in theta, X, residuals and all four counters"""
    import scipy.sparse as sp
    import cfs_spmv_amd as cfs
    n, rp, ci, va = _matrix("Flan_1565@0.01")
    d = np.asarray(abs(sp.csr_matrix((np.asarray(va, np.float64), ci, rp), shape=(n, n))).sum(axis=1)).ravel()
    opt = cfs.make_options(flags=DET)
    D = cfs.SymMatrix(n, rp, ci, va.astype(dtype), options=opt)
    M = cfs.SymMatrix(*_csr(sp.diags(d / d.mean()), dtype), options=opt)
    assert D.kernel_variant()["det"] == 1 and M.kernel_variant()["det"] == 1
    kw = dict(k=4, precond="block_jacobi", block=3, tol=TOL[dtype], scale=1.0, maxiter=10, B=M)
    w1, X1, i1 = _solve(D, **kw)
    w2, X2, i2 = _solve(D, **kw)
    D.close(), M.close()
    print(f"lobpcg_gen {np.dtype(dtype).name} Flan_1565@0.01 (deterministic): theta {w1}, iterations {i1['iterations']}, nconv {i1['nconv']}")
    assert np.all(np.isfinite(w1)) and np.all(np.diff(w1) >= 0) and i1["iterations"] == 10
    assert np.array_equal(w1.view(np.uint8), w2.view(np.uint8)) and np.array_equal(X1.view(np.uint8), X2.view(np.uint8))
    cnt = lambda i: (i["nconv"], i["iterations"], i["products"], i["b_products"])
    assert cnt(i1) == cnt(i2) and i1["b_products"] > 0
    assert np.array_equal(i1["residuals"].view(np.uint8), i2["residuals"].view(np.uint8))


@DTYPES
def test_refusals(dtype):
    """each refusal with its code and word, through the C entry point where Python would raise first: nothing is written
    and the four counters are zero"""
    import torch
    import cfs_spmv_amd as cfs
    from cfs_spmv_amd import _lib
    lib = cfs.load()
    case = _case("lap2d16x15", dtype)
    n, rp, ci, va = case["A"]
    other = np.float32 if dtype == np.float64 else np.float64
    per = 16 // np.dtype(dtype).itemsize
    ld, k = -(-n // per) * per, 4
    dev = torch.zeros(k * ld, dtype=torch.float64 if dtype == np.float64 else torch.float32, device="cuda")

    def refused(h, hb, code, word, amg=None):
        w, res = (C.c_double * k)(*([7.0] * k)), (C.c_double * k)(*([7.0] * k))
        cnt = [C.c_int(7) for _ in range(4)]
        tail = (1e-6, 1.0, 5, None, ld, w, dev.data_ptr(), ld, res, *(C.byref(c) for c in cnt), None)
        rc = lib.cfs_hip_sym_lobpcg_gen_amg(h, hb, amg, k, *tail) if amg is not None else lib.cfs_hip_sym_lobpcg_gen(h, hb, k, 1, *tail)
        torch.cuda.synchronize()
        assert rc == code and word in lib.cfs_hip_last_error(), (rc, lib.cfs_hip_last_error(), word)
        assert [c.value for c in cnt] == [0, 0, 0, 0] and list(w) == [7.0] * k and list(res) == [7.0] * k and not bool(dev.any())
    A, B = _handles(case)
    # B of another n, of another value type: CFS_HIP_ERR_ARG where the handles are first read
    Bn = cfs.SymMatrix(*_case("rand257", dtype, kind="identity")["B"])
    refused(A._h, Bn._h, _lib.ERR_ARG, b"B must have the n")
    Bn.close()
    Bt = cfs.SymMatrix(*_case("lap2d16x15", other)["B"])
    refused(A._h, Bt._h, _lib.ERR_ARG, b"B must have the n")
    with pytest.raises(ValueError):  # (Python says so before any device work)
        A.lobpcg_gen(Bt, k=k, scale=1.0)
    Bt.close()
    # a shard or a multi-device handle on either side: CFS_HIP_ERR_UNSUPPORTED
    splits = np.array([0, n // 2, n], np.int32)
    Sa, Sb = cfs.SymMatrix(n, rp, ci, va, row_splits=splits, rank=1), cfs.SymMatrix(*case["B"], row_splits=splits, rank=1)
    refused(Sa._h, B._h, _lib.ERR_UNSUPPORTED, b"shard")
    refused(A._h, Sb._h, _lib.ERR_UNSUPPORTED, b"shard")
    Sa.close(), Sb.close()
    Ma, Mb = cfs.SymMatrix(n, rp, ci, va, ngpus=2), cfs.SymMatrix(*case["B"], ngpus=2)
    refused(Ma._h, B._h, _lib.ERR_UNSUPPORTED, b"multi-device")
    refused(A._h, Mb._h, _lib.ERR_UNSUPPORTED, b"multi-device")
    Ma.close(), Mb.close()
    # B = -I: every G_jj is negative, the start block has rank 0 in the B inner product after the two refills
    Bneg = cfs.SymMatrix(*_case("lap2d16x15", dtype, kind="minus")["B"])
    refused(A._h, Bneg._h, _lib.ERR_ARG, b"positive definite")
    G = A.amg(rp, ci, va)
    refused(A._h, Bneg._h, _lib.ERR_ARG, b"positive definite", amg=G._a)
    with pytest.raises(_lib.CfsHipError, match="positive definite") as e:
        A.lobpcg_gen(Bneg, k=k, scale=1.0)
    assert e.value.code == _lib.ERR_ARG
    with pytest.raises(_lib.CfsHipError, match="positive definite"):
        A.debug_lobpcg(k, 1, 2, B=Bneg)
    G.close(), Bneg.close()
    # the refusals of cfs_hip_sym_lobpcg, through Python
    for kw, word in ((dict(k=17), "bad k"), (dict(precond="block_jacobi", block=5), "block_rows"), (dict(scale=0.0), "tolerance")):
        with pytest.raises(_lib.CfsHipError, match=word) as e:
            A.lobpcg_gen(B, **dict(dict(k=k, tol=1e-6, scale=1.0, maxiter=5), **kw))
        assert e.value.code == _lib.ERR_ARG
    A.close(), B.close()
