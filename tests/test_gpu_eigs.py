"""cfs_hip_sym_eigs, the whole solver: thick-restart Lanczos on the GPU against a reference spectrum -- dense
numpy.linalg.eigh for n <= 1026, scipy.sparse.linalg.eigsh(A64, k, which, tol=0) above (in both, each eigenvalue
re-evaluated as the long-double Rayleigh quotient of its own vector, see _case) -- of the matrix as the library
holds it (the values rounded to the value type).  fp64 runs with tol 1e-10, fp32 with tol 1e-4; k = 4 and ncv = 20
unless a case says otherwise; the start vector is default_rng(n).uniform(-1, 1, n).

spiked(M, k, sign): with w the largest absolute row sum of M, sign * w * (1 + i) is added to the diagonal of row
(i (n - 1)) // (k - 1), i = 0 .. k - 1 -- k eigenvalues separated from each other and from the rest by about w, which
converge in 0-1 restarts.  The plain dominant(...) / banded_spd matrices need more (fp64: 4-5 restarts on rand257 /
rand1023, 19 on band20001; fp32: 2-3 and 11): they are the cases that exercise the restart.

With r_i = ||A x_i - theta_i x_i||_2 / ||x_i||_2 recomputed HERE in long double from the returned x_i and theta_i, and
lmax the largest |lambda| of the reference:

    nconv == k;   r_i <= 2 tol lmax;   |theta_i - lambda_i| <= r_i + 16 u lmax   (u = 2^-53 / 2^-24)

The factor 2 covers the O(sqrt(ncv) u ||A||) between the Lanczos estimate the solver stops on and the true residual of
the rounded vector -- below 1 % of tol at these tolerances.  Comparing with lambda_i BY INDEX is what catches a solver
that returns an interior eigenvalue; the test first asserts from the reference spectrum that the gaps of the wanted
eigenvalues exceed 4 tol lmax.  The library's own `residuals` must agree with r_i within 4 u lmax + 1e-3 r_i (the
product it recomputes them from is rounded to the value type), and products = ncv + restarts (ncv - l) + k with
l = k + (ncv - k) / 2.

Wide bases (test_wide_bases_and_many_pairs): ncv up to CFS_HIP_EIGS_MAX_NCV = 128 and k up to 100 on the plain rand1023 and
rand257, where l = 84, 53, 96 and 114 columns are kept per restart; on the CPU model the cases take 2 / 2, 10 / 8, 3 / 2 and
9 / 8 restarts (fp64 / fp32), and the smallest wanted gap over 4 tol lmax is 4.3e6 / 4.3, 4.3e6 / 4.3, 1.16e6 / 1.16 and
1.11e6 / 1.11 -- narrow in fp32 but above 1, from the reference spectrum alone.

Measured on the MI355X (value type, case: restarts, products, nconv, r = max r_i / (tol lmax), dtheta = max |theta_i -
lambda_i| / lmax, and how far the library's residuals are from r_i):

  f64 rand257 LA n=257 k=4 ncv=20 LA: restarts 0, products 24, nconv 4, r 0.000, dtheta 4.58e-16, residuals off by 4.42e-17 lmax
  f32 rand257 LA n=257 k=4 ncv=20 LA: restarts 0, products 24, nconv 4, r 0.000, dtheta 1.89e-08, residuals off by 3.91e-08 lmax
  f64 rand257 SA n=257 k=4 ncv=20 SA: restarts 0, products 24, nconv 4, r 0.000, dtheta 3.94e-16, residuals off by 2.55e-17 lmax
  f32 rand257 SA n=257 k=4 ncv=20 SA: restarts 0, products 24, nconv 4, r 0.000, dtheta 3.64e-08, residuals off by 1.76e-08 lmax
  f64 rand257 plain n=257 k=4 ncv=20 LA: restarts 4, products 56, nconv 4, r 0.005, dtheta 1.22e-15, residuals off by 2.02e-17 lmax
  f32 rand257 plain n=257 k=4 ncv=20 LA: restarts 2, products 40, nconv 4, r 0.082, dtheta 2.33e-08, residuals off by 2.49e-08 lmax
  f64 rand1023 LA n=1023 k=4 ncv=20 LA: restarts 0, products 24, nconv 4, r 0.000, dtheta 7.89e-16, residuals off by 1.08e-17 lmax
  f32 rand1023 LA n=1023 k=4 ncv=20 LA: restarts 0, products 24, nconv 4, r 0.001, dtheta 5.55e-08, residuals off by 4.14e-08 lmax
  f64 rand1023 SA n=1023 k=4 ncv=20 SA: restarts 0, products 24, nconv 4, r 0.028, dtheta 1.08e-15, residuals off by 3.16e-17 lmax
  f32 rand1023 SA n=1023 k=4 ncv=20 SA: restarts 0, products 24, nconv 4, r 0.000, dtheta 3.57e-08, residuals off by 3.98e-08 lmax
  f64 rand1023 plain n=1023 k=4 ncv=20 LA: restarts 5, products 64, nconv 4, r 0.473, dtheta 2.35e-15, residuals off by 4.83e-17 lmax
  f32 rand1023 plain n=1023 k=4 ncv=20 LA: restarts 3, products 48, nconv 4, r 0.023, dtheta 2.35e-08, residuals off by 4.58e-08 lmax
  f64 band20001 LA n=20001 k=4 ncv=20 LA: restarts 1, products 32, nconv 4, r 0.000, dtheta 3.57e-17, residuals off by 1.05e-17 lmax
  f32 band20001 LA n=20001 k=4 ncv=20 LA: restarts 0, products 24, nconv 4, r 0.000, dtheta 4.29e-08, residuals off by 1.37e-08 lmax
  f64 band20001 SA n=20001 k=4 ncv=20 SA: restarts 0, products 24, nconv 4, r 0.010, dtheta 1.57e-16, residuals off by 6.76e-17 lmax
  f32 band20001 SA n=20001 k=4 ncv=20 SA: restarts 0, products 24, nconv 4, r 0.000, dtheta 1.73e-08, residuals off by 5.05e-09 lmax
  f64 band20001 plain n=20001 k=4 ncv=20 LA: restarts 19, products 176, nconv 4, r 0.431, dtheta 1.91e-16, residuals off by 5.23e-17 lmax
  f32 band20001 plain n=20001 k=4 ncv=20 LA: restarts 11, products 112, nconv 4, r 0.178, dtheta 2.22e-09, residuals off by 2.91e-08 lmax
  f64 rand1023 SA-spiked n=1023 k=4 ncv=20 LM: restarts 3, products 48, nconv 4, r 0.004, dtheta 1.08e-15, residuals off by 3.16e-17 lmax
  f32 rand1023 SA-spiked n=1023 k=4 ncv=20 LM: restarts 0, products 24, nconv 4, r 0.934, dtheta 1.61e-07, residuals off by 3.98e-08 lmax
  f64 rand2 n=2 k=1 ncv=2 LA: restarts 0, products 3, nconv 1, r 0.000, dtheta 0.00e+00, residuals off by 1.81e-16 lmax
  f64 rand65 n=65 k=4 ncv=65 LA: restarts 0, products 69, nconv 4, r 0.000, dtheta 8.07e-16, residuals off by 8.05e-17 lmax
  f32 rand2 n=2 k=1 ncv=2 LA: restarts 0, products 3, nconv 1, r 0.001, dtheta 3.08e-08, residuals off by 2.24e-08 lmax
  f32 rand65 n=65 k=4 ncv=65 LA: restarts 0, products 69, nconv 4, r 0.001, dtheta 2.52e-08, residuals off by 1.75e-08 lmax
  f64 band600001 LA n=600001 k=2 ncv=8 LA: restarts 5, products 25, nconv 2, r 0.118, dtheta 1.25e-16, residuals off by 6.07e-19 lmax
  f32 band600001 LA n=600001 k=2 ncv=8 LA: restarts 2, products 16, nconv 2, r 0.040, dtheta 1.61e-08, residuals off by 3.09e-08 lmax
  f64 band20001 plain (two shards) n=20001 k=4 ncv=20 LA: restarts 19, products 176, nconv 4, r 0.431, dtheta 1.91e-16, residuals off by 5.23e-18 lmax
  f32 band20001 plain (two shards) n=20001 k=4 ncv=20 LA: restarts 11, products 112, nconv 4, r 0.178, dtheta 5.43e-09, residuals off by 3.10e-08 lmax
  f64 rand1023 plain n=1023 k=40 ncv=128 LA: restarts 2, products 256, nconv 40, r 0.000, dtheta 5.89e-16, residuals off by 3.28e-17 lmax
  f32 rand1023 plain n=1023 k=40 ncv=128 LA: restarts 2, products 256, nconv 40, r 0.001, dtheta 2.35e-08, residuals off by 4.41e-08 lmax
  f64 rand1023 plain n=1023 k=40 ncv=67 LA: restarts 10, products 247, nconv 40, r 0.224, dtheta 5.89e-16, residuals off by 7.13e-17 lmax
  f32 rand1023 plain n=1023 k=40 ncv=67 LA: restarts 8, products 219, nconv 40, r 0.222, dtheta 2.36e-08, residuals off by 4.19e-08 lmax
  f64 rand257 plain n=257 k=64 ncv=128 LA: restarts 3, products 288, nconv 64, r 0.000, dtheta 4.73e-16, residuals off by 6.02e-17 lmax
  f32 rand257 plain n=257 k=64 ncv=128 LA: restarts 2, products 256, nconv 64, r 0.364, dtheta 1.41e-08, residuals off by 4.11e-08 lmax
  f64 rand257 plain n=257 k=100 ncv=128 LA: restarts 9, products 354, nconv 100, r 0.003, dtheta 7.43e-16, residuals off by 6.02e-17 lmax
  f32 rand257 plain n=257 k=100 ncv=128 LA: restarts 8, products 340, nconv 100, r 0.001, dtheta 1.41e-08, residuals off by 4.11e-08 lmax

(against numpy.linalg.eigvalsh's own values, the reference before the wide cases, the fp64 dtheta of these four were 6.59e-15,
6.95e-15, 2.70e-15 and 2.70e-15 -- above the 16 u = 1.78e-15 of the check, with the SAME theta bits from runs of different
ncv: the error was eigvalsh's, see _case)

and, from the other tests:

  f64 Flan_1565@0.01 (deterministic): theta [55.83123707 55.6165941  55.18076045 54.59034505], restarts 3, nconv 0
  f32 Flan_1565@0.01 (deterministic): theta [55.83123707 55.61659409 55.18076043 54.5903451 ], restarts 3, nconv 0
  f64 band20001 tol=0: r after one restart [0.00173845 0.0987018  0.14109276 0.18494614], after two [4.05702323e-05 1.04333924e-02 4.44162703e-02 8.52379429e-02]
  f32 band20001 tol=0: r after one restart [0.00173844 0.09870176 0.14109274 0.18494613], after two [4.05740763e-05 1.04334026e-02 4.44162399e-02 8.52378863e-02]
  f64 rand1023 LA: host-driven [108.00682035  82.71047214  57.5341871   40.13856879] (0 restarts), native [108.00682035  82.71047214  57.5341871   40.13856879] (0 restarts)
  f32 rand1023 LA: host-driven [108.00682283  82.71047633  57.53418396  40.1385675 ] (0 restarts), native [108.00682283  82.71047633  57.53418396  40.1385675 ] (0 restarts)
"""
import functools

import numpy as np
import pytest

from test_gpu_cg_steps import DET, DTYPES, UNIT, _matrix
from test_gpu_kernel_variants import PLAN_KNOBS
from test_gpu_lanczos_steps import BLOCK3, decoupled

pytestmark = pytest.mark.gpu

TOL = {np.float64: 1e-10, np.float32: 1e-4}


@pytest.fixture(autouse=True)
def _torch_first(monkeypatch):
    """torch brings a HIP runtime of its own: it has to initialise before libcfs_hip.so's"""
    import torch
    torch.cuda.init()
    torch.cuda.set_device(0)
    for k in PLAN_KNOBS:
        monkeypatch.delenv(k, raising=False)
    yield


def spiked(n, rp, ci, va, k, sign):
    import scipy.sparse as sp
    A = sp.csr_matrix((np.asarray(va, np.float64), ci, rp), shape=(n, n))
    w = float(abs(A).sum(axis=1).max())
    d = np.zeros(n)
    for i in range(k):
        d[(i * (n - 1)) // (k - 1)] += sign * w * (1 + i)
    A = (A + sp.diags(d)).tocsr()
    A.sort_indices()
    return n, A.indptr.astype(np.int32), A.indices.astype(np.int32), A.data


def _sorted(lam, which):
    if which == "SA":
        return np.sort(lam)
    if which == "LA":
        return np.sort(lam)[::-1]
    return lam[np.argsort(-np.abs(lam), kind="stable")]


@functools.lru_cache(maxsize=None)
def _case(name, kind, dtype, k=4, which=None):
    """(n, rp, ci, va in the value type, v0, the k reference eigenvalues in the order of `which`, lmax): kind "plain", or
    "LA" / "SA" for the matrix spiked at that end; computed once, shared, unchanged"""
    import scipy.sparse as sp
    import scipy.sparse.linalg as spl
    n, rp, ci, va = _matrix(name)
    if kind != "plain":
        n, rp, ci, va = spiked(n, rp, ci, va, k, 1 if kind == "LA" else -1)
    which = which or ("LA" if kind == "plain" else kind)
    va = np.asarray(va).astype(dtype)
    A64 = sp.csr_matrix((va.astype(np.float64), ci, rp), shape=(n, n))
    if n <= 1026:
        # eigvalsh's own eigenvalues are off by up to 57 u lmax inside the spectrum of rand1023 (24 u lmax on rand257) and
        # differ between machines, more than the 16 u lmax of the check; the top four, all that was compared before the
        # wide cases, are not.  As below: each is replaced by the Rayleigh quotient of eigh's vector in long double
        # (eigh's residuals are below 1e-13: within r^2 / gap of the eigenvalue, far below u lmax)
        from oracle import oracle
        lam, Q = np.linalg.eigh(A64.toarray())
        lmax = float(np.max(np.abs(lam)))
        pick = {"SA": np.argsort(lam, kind="stable"), "LA": np.argsort(lam, kind="stable")[::-1],
                "LM": np.argsort(-np.abs(lam), kind="stable")}[which][:k]
        lam = lam[pick]
        for i, j in enumerate(pick):
            x = Q[:, j].astype(np.longdouble)
            lam[i] = float(np.dot(x, oracle.csr_spmv_ldx(n, rp, ci, va, x)) / np.dot(x, x))
    else:
        # eigsh's own eigenvalues are off by up to 2.4e-14 (13 ulp) on band20001 and differ between machines, more than
        # the 16 u lmax of the check: each is replaced by the Rayleigh quotient of eigsh's vector in long double, which
        # is within r^2 / gap of the eigenvalue that vector belongs to (r, its residual, is below 1e-13 here)
        from oracle import oracle
        lam, Q = spl.eigsh(A64, k, which=which, tol=0)
        for i in range(k):
            x = Q[:, i].astype(np.longdouble)
            lam[i] = float(np.dot(x, oracle.csr_spmv_ldx(n, rp, ci, va, x)) / np.dot(x, x))
        lam = _sorted(lam, which)
        lmax = float(np.max(np.abs(spl.eigsh(A64, 1, which="LM", tol=0, return_eigenvectors=False))))
    v0 = np.random.default_rng(n).uniform(-1, 1, n).astype(dtype)
    for x in (rp, ci, va, v0, lam):
        x.setflags(write=False)
    return n, rp, ci, va, v0, lam, lmax


def _residuals(n, rp, ci, va, w, X):
    """r_i in long double from the returned pairs (X: (n, k) numpy)"""
    from oracle import oracle
    out = []
    for i in range(len(w)):
        x = X[:, i].astype(np.longdouble)
        d = oracle.csr_spmv_ldx(n, rp, ci, va, x) - np.longdouble(w[i]) * x
        out.append(float(np.sqrt(np.dot(d, d)) / np.sqrt(np.dot(x, x))))
    return np.array(out)


def _solve(A, v0, **kw):
    import torch
    w, X, info = A.eigs(v0=torch.from_numpy(np.array(v0)).cuda() if v0 is not None else None, **kw)
    torch.cuda.synchronize()
    return w, (np.ascontiguousarray(X.cpu().numpy()) if X is not None else None), info


def _check(label, case, dtype, A, k=4, ncv=20, which="LA", plain=False):
    n, rp, ci, va, v0, lam, lmax = case
    tol, u = TOL[dtype], UNIT[dtype]
    gaps = np.abs(np.diff(lam))
    assert len(lam) == k and (k == 1 or np.min(gaps) > 4 * tol * lmax), f"{label}: badly chosen case, gaps {gaps}"
    w, X, info = _solve(A, v0, k=k, which=which, ncv=ncv, tol=tol)
    assert w.shape == (k,) and w.dtype == np.float64 and X.shape == (n, k)
    r = _residuals(n, rp, ci, va, w, X)
    print(f"eigs {np.dtype(dtype).name} {label} n={n} k={k} ncv={ncv} {which}: restarts {info['restarts']}, products "
          f"{info['products']}, nconv {info['nconv']}, max r/(tol lmax) {np.max(r) / (tol * lmax):.3f}, "
          f"max |theta - lambda|/lmax {np.max(np.abs(w - lam)) / lmax:.2e}, library residuals off by "
          f"{np.max(np.abs(info['residuals'] - r)) / lmax:.2e} lmax")
    errors = []
    if info["nconv"] != k:
        errors.append(f"nconv = {info['nconv']}")
    for i in range(k):
        if not r[i] <= 2 * tol * lmax:
            errors.append(f"r_{i} = {r[i]:.3e} > 2 tol lmax = {2 * tol * lmax:.3e}")
        if not abs(w[i] - lam[i]) <= r[i] + 16 * u * lmax:
            errors.append(f"theta_{i} = {w[i]!r}, lambda_{i} = {lam[i]!r}: apart by more than r_i + 16 u lmax = {r[i] + 16 * u * lmax:.3e}")
        if not abs(info["residuals"][i] - r[i]) <= 4 * u * lmax + 1e-3 * r[i]:
            errors.append(f"residuals[{i}] = {info['residuals'][i]:.3e}, recomputed {r[i]:.3e}")
    l = k + (ncv - k) // 2
    if info["products"] != ncv + info["restarts"] * (ncv - l) + k:
        errors.append(f"products = {info['products']} with {info['restarts']} restarts")
    if plain and not info["restarts"] >= 1:
        errors.append("no restart was needed: the restart kernel did not run")
    assert not errors, f"{label} {np.dtype(dtype).name}: " + "; ".join(errors)
    return w, X, info


@DTYPES
@pytest.mark.parametrize("kind", ["LA", "SA", "plain"])
@pytest.mark.parametrize("name", ["rand257", "rand1023", "band20001"])
def test_extreme_pairs(name, kind, dtype):
    import cfs_spmv_amd as cfs
    case = _case(name, kind, dtype)
    A = cfs.SymMatrix(*case[:4])
    _check(f"{name} {kind}", case, dtype, A, which="LA" if kind == "plain" else kind, plain=kind == "plain")
    A.close()


# (name, k, ncv): l = k + (ncv - k) / 2 kept columns = 84; 53 (m = 67 odd); 96; 114 (residual slots up to 199)
WIDE = [("rand1023", 40, 128), ("rand1023", 40, 67), ("rand257", 64, 128), ("rand257", 100, 128)]


@DTYPES
@pytest.mark.parametrize("name,k,ncv", WIDE)
def test_wide_bases_and_many_pairs(name, k, ncv, dtype):
    """the restart at deep bases: V S with more than 64 / 32 kept columns (the second chunk of eigs_combine_kernel's column
    loop), the arrow of the projected matrix in row l up to 114, k up to 100 returned columns and closing residuals.  Every
    case restarts at least once (`plain`); the checks are _check's own"""
    import cfs_spmv_amd as cfs
    case = _case(name, "plain", dtype, k=k)
    A = cfs.SymMatrix(*case[:4])
    _check(f"{name} plain", case, dtype, A, k=k, ncv=ncv, plain=True)
    A.close()


def _pair_invariants(n, rp, ci, va, w, X, lmax):
    """(max |X^T X - I|, max_i |theta_i - x_i^T A x_i / x_i^T x_i| / lmax) in long double from the returned pairs"""
    from oracle import oracle
    Xl = X.astype(np.longdouble)
    orth = float(np.max(np.abs(Xl.T @ Xl - np.eye(X.shape[1], dtype=np.longdouble))))
    rq = 0.0
    for i in range(X.shape[1]):
        x = Xl[:, i]
        rq = max(rq, abs(float(np.longdouble(w[i]) - np.dot(x, oracle.csr_spmv_ldx(n, rp, ci, va, x)) / np.dot(x, x))))
    return orth, rq / lmax


@DTYPES
def test_the_end_of_the_range(dtype):
    """rand257, k = 127 = CFS_HIP_EIGS_MAX_NCV - 1, ncv = 128, tol = 0, max_restarts = 2: l = 127, every restart keeps 127 of
    128 columns and adds one product.  No convergence is claimed (127 of 257 eigenvalues do not converge in two restarts,
    and nothing is compared with the spectrum): return code 0, the counters, finite outputs in descending order, the
    library's residuals against the long-double recomputation for all 127 pairs (the closing residual slots up to 253),
    and two invariants of the returned pairs in long double,

        o = max |X^T X - I|        q = max_i |theta_i - x_i^T A x_i / x_i^T x_i| / lmax

    each allowed 4 x the same quantity of solver.eigs, the host-driven model, run here on the same handle with the same
    arguments, + 16 u.  Measured on the MI355X (native / model):

      f64: nconv 0, o = 5.100e-15 / 3.288e-15, q = 4.626e-16 / 6.113e-16, residuals off by 6.02e-17 lmax
      f32: nconv 0, o = 8.649e-08 / 8.649e-08, q = 1.406e-08 / 1.406e-08, residuals off by 4.11e-08 lmax
    """
    import torch
    import cfs_spmv_amd as cfs
    from cfs_spmv_amd import solver
    k, ncv = 127, 128
    n, rp, ci, va, v0, lam, lmax = _case("rand257", "plain", dtype, k=k)
    u = UNIT[dtype]
    A = cfs.SymMatrix(n, rp, ci, va)
    w, X, info = _solve(A, v0, k=k, which="LA", ncv=ncv, tol=0.0, max_restarts=2)  # (a return code other than 0 raises)
    wm, Xm, im = solver.eigs(A, k, which="LA", ncv=ncv, tol=0.0, max_restarts=2, v0=torch.from_numpy(np.array(v0)).cuda())
    torch.cuda.synchronize()
    Xm = np.ascontiguousarray(Xm.cpu().numpy())
    A.close()
    assert info["restarts"] == 2 and info["products"] == 128 + 2 + 127
    assert im["restarts"] == 2 and im["products"] == info["products"], "the model ran the same iteration"
    assert w.shape == (k,) and X.shape == (n, k)
    assert np.all(np.isfinite(w)) and np.all(np.isfinite(X)) and np.all(np.isfinite(info["residuals"]))
    assert np.all(np.diff(w) <= 0), "descending"
    r = _residuals(n, rp, ci, va, w, X)
    off = np.abs(info["residuals"] - r)
    assert np.all(off <= 4 * u * lmax + 1e-3 * r), f"residuals off by up to {np.max(off) / lmax:.2e} lmax, at pair {int(np.argmax(off))}"
    o, q = _pair_invariants(n, rp, ci, va, w, X, lmax)
    om, qm = _pair_invariants(n, rp, ci, va, wm, Xm, lmax)
    print(f"eigs {np.dtype(dtype).name} rand257 k=127 ncv=128 two restarts: nconv {info['nconv']} (model {im['nconv']}), "
          f"|X^T X - I| {o:.3e} / {om:.3e}, |theta - rq| / lmax {q:.3e} / {qm:.3e}, residuals off by {np.max(off) / lmax:.2e} lmax")
    assert o <= 4 * om + 16 * u, f"|X^T X - I| = {o:.3e}, allowed 4 x {om:.3e} + 16 u"
    assert q <= 4 * qm + 16 * u, f"|theta - rq| / lmax = {q:.3e}, allowed 4 x {qm:.3e} + 16 u"


@DTYPES
def test_largest_magnitude_at_the_negative_end(dtype):
    """the SA-spiked rand1023: its largest |lambda| are three negative spikes and then the top of the positive end"""
    import cfs_spmv_amd as cfs
    case = _case("rand1023", "SA", dtype, which="LM")
    assert np.all(case[5][:3] < 0) and case[5][3] > 0 and np.all(np.diff(np.abs(case[5])) < 0)
    A = cfs.SymMatrix(*case[:4])
    _check("rand1023 SA-spiked", case, dtype, A, which="LM")
    A.close()


@DTYPES
def test_the_smallest_sizes(dtype):
    """rand2 with k = 1, ncv = 2 = n; rand65 with ncv = n: the basis spans the whole space"""
    import cfs_spmv_amd as cfs
    case = _case("rand2", "plain", dtype, k=1)
    A = cfs.SymMatrix(*case[:4])
    _check("rand2", case, dtype, A, k=1, ncv=2)
    A.close()
    case = _case("rand65", "plain", dtype)
    A = cfs.SymMatrix(*case[:4])
    _check("rand65", case, dtype, A, ncv=65)
    A.close()


@DTYPES
def test_beyond_one_grid_stride_sweep(dtype):
    """spiked band600001, LA, k = 2, ncv = 8: n lies beyond one sweep of the vector kernels' grid and has an odd tail"""
    import cfs_spmv_amd as cfs
    case = _case("band600001", "LA", dtype, k=2)
    A = cfs.SymMatrix(*case[:4])
    _check("band600001 LA", case, dtype, A, k=2, ncv=8)
    A.close()


@DTYPES
def test_through_a_two_shard_handle(dtype):
    import cfs_spmv_amd as cfs
    case = _case("band20001", "plain", dtype)
    M = cfs.SymMatrix(*case[:4], ngpus=2)
    _check("band20001 plain (two shards)", case, dtype, M, plain=True)
    M.close()


@DTYPES
def test_a_deterministic_handle_is_bit_reproducible(dtype):
    """Flan_1565@0.01, LA: two runs bit-equal in theta and X, and the values-only call returns the same theta bits"""
    import cfs_spmv_amd as cfs
    n, rp, ci, va = _matrix("Flan_1565@0.01")
    va = va.astype(dtype)
    v0 = np.random.default_rng(n).uniform(-1, 1, n).astype(dtype)
    D = cfs.SymMatrix(n, rp, ci, va, options=cfs.make_options(flags=DET))
    assert D.kernel_variant()["det"] == 1
    kw = dict(k=4, which="LA", ncv=20, tol=TOL[dtype], max_restarts=3)
    w1, X1, i1 = _solve(D, v0, **kw)
    w2, X2, i2 = _solve(D, v0, **kw)
    w3, X3, i3 = _solve(D, v0, vectors=False, **kw)
    D.close()
    print(f"eigs {np.dtype(dtype).name} Flan_1565@0.01 (deterministic): theta {w1}, restarts {i1['restarts']}, nconv {i1['nconv']}")
    assert np.all(np.isfinite(w1)) and np.all(np.diff(w1) <= 0)
    assert np.array_equal(w1.view(np.uint8), w2.view(np.uint8)) and np.array_equal(X1.view(np.uint8), X2.view(np.uint8))
    assert (i1["nconv"], i1["restarts"], i1["products"]) == (i2["nconv"], i2["restarts"], i2["products"])
    assert np.array_equal(i1["residuals"].view(np.uint8), i2["residuals"].view(np.uint8))
    assert X3 is None and np.array_equal(w1.view(np.uint8), w3.view(np.uint8))
    assert (i3["nconv"], i3["restarts"]) == (i1["nconv"], i1["restarts"]) and i3["products"] == i1["products"] - 4
    # without vectors the residuals are the Lanczos estimates: what nconv was counted from
    lmax_ritz = abs(w1[0])
    assert np.all(i3["residuals"][:i3["nconv"]] <= TOL[dtype] * lmax_ritz * (1 + 1e-12))


@DTYPES
def test_an_unreachable_tolerance(dtype):
    """tol = 0 and max_restarts = 2 on the plain band20001: returns 0 with nconv < k and finite outputs, and no pair is
    worse than after one restart (within 4 u lmax, what the residual of a vector stored in the value type can resolve)"""
    import cfs_spmv_amd as cfs
    n, rp, ci, va, v0, lam, lmax = _case("band20001", "plain", dtype)
    A = cfs.SymMatrix(n, rp, ci, va)
    w2, X2, i2 = _solve(A, v0, k=4, which="LA", ncv=20, tol=0.0, max_restarts=2)
    w1, X1, i1 = _solve(A, v0, k=4, which="LA", ncv=20, tol=0.0, max_restarts=1)
    A.close()
    assert i2["nconv"] < 4 and i2["restarts"] == 2 and i1["restarts"] == 1
    assert np.all(np.isfinite(w2)) and np.all(np.isfinite(X2)) and np.all(np.isfinite(i2["residuals"]))
    r2, r1 = _residuals(n, rp, ci, va, w2, X2), _residuals(n, rp, ci, va, w1, X1)
    print(f"eigs {np.dtype(dtype).name} band20001 tol=0: r after one restart {r1}, after two {r2}")
    assert np.all(r2 <= r1 + 4 * UNIT[dtype] * lmax)


@DTYPES
def test_breakdown(dtype):
    """the block [[2, 1, 0], [1, 2, 1], [0, 1, 2]] cut off from the rest of rand257, v0 = e_0: the Krylov space is the block's,
    exactly -- a breakdown at step 3, the Ritz pairs of T_3 are the block's eigenpairs 2 - sqrt 2, 2, 2 + sqrt 2"""
    import cfs_spmv_amd as cfs
    n, rp, ci, va = decoupled("rand257", [0, 1, 2], BLOCK3)
    va = va.astype(dtype)
    A = cfs.SymMatrix(n, rp, ci, va)
    e = np.zeros(n, dtype)
    e[0] = 1
    u = UNIT[dtype]
    w, X, info = _solve(A, e, k=2, which="SA", ncv=20, tol=TOL[dtype])
    assert info["nconv"] == 2 and info["restarts"] == 0 and info["products"] == 3 + 2
    assert np.max(np.abs(w - np.array([2 - np.sqrt(2), 2.0]))) <= 16 * u * (2 + np.sqrt(2))
    assert not X[3:].any() and np.max(_residuals(n, rp, ci, va, w, X)) <= 16 * u * (2 + np.sqrt(2))
    w, X, info = _solve(A, e, k=4, which="SA", ncv=20, tol=TOL[dtype])
    A.close()
    assert info["nconv"] == 3 and info["restarts"] == 0 and info["products"] == 3 + 3
    assert np.max(np.abs(w[:3] - np.array([2 - np.sqrt(2), 2.0, 2 + np.sqrt(2)]))) <= 16 * u * (2 + np.sqrt(2))
    # the remaining outputs are zero-filled
    assert w[3] == 0.0 and info["residuals"][3] == 0.0 and not X[:, 3].any() and X[:, :3].any(axis=0).all()


@DTYPES
def test_error_paths(dtype):
    import torch
    import cfs_spmv_amd as cfs
    from cfs_spmv_amd import _lib
    n, rp, ci, va, v0 = _case("rand257", "plain", dtype)[:5]
    A = cfs.SymMatrix(n, rp, ci, va)

    def refused(code, word, **kw):
        with pytest.raises(_lib.CfsHipError, match=word) as e:
            A.eigs(**dict(dict(k=4, ncv=20, tol=1e-6, v0=torch.from_numpy(np.array(v0)).cuda()), **kw))
        assert e.value.code == code, (kw, e.value)
    refused(_lib.ERR_ARG, "start vector", v0=torch.zeros(n, dtype=torch.float64 if dtype == np.float64 else torch.float32, device="cuda"))
    nan = v0.copy()
    nan[n // 2] = np.nan
    refused(_lib.ERR_ARG, "start vector", v0=torch.from_numpy(nan).cuda())
    refused(_lib.ERR_ARG, "k / ncv", ncv=129)
    host = np.zeros(n + 8, dtype)
    host = host[(-host.ctypes.data % 16) // host.itemsize:][:n]  # a host pointer, 16-byte aligned
    refused(_lib.ERR_ARG, "device pointer", v0=host)
    with pytest.raises(ValueError):
        A.eigs(k=2, which="BE")
    A.close()
    # ncv > n on a small matrix
    m, rp2, ci2, va2 = _matrix("rand5")
    B = cfs.SymMatrix(m, rp2, ci2, va2.astype(dtype))
    with pytest.raises(_lib.CfsHipError, match="k / ncv") as e:
        B.eigs(k=2, ncv=6)
    assert e.value.code == _lib.ERR_ARG
    w, X, info = B.eigs(k=2, tol=TOL[dtype])  # the default ncv = min(n, max(2 k + 1, 20)) = n, the library's start vector
    assert info["nconv"] == 2
    B.close()
    S = cfs.SymMatrix(n, rp, ci, va, row_splits=np.array([0, n // 2, n], np.int32), rank=1)
    with pytest.raises(_lib.CfsHipError) as e:
        S.eigs(k=4, ncv=20)
    assert e.value.code == _lib.ERR_UNSUPPORTED
    S.close()


@DTYPES
def test_host_driven_and_native_loops_agree(dtype):
    """solver.eigs (torch-driven) against solver.eigs_native on the LA-spiked rand1023: theta within the sum of the two
    runs' residuals"""
    import torch
    import cfs_spmv_amd as cfs
    from cfs_spmv_amd.solver import eigs, eigs_native
    n, rp, ci, va, v0, lam, lmax = _case("rand1023", "LA", dtype)
    A = cfs.SymMatrix(n, rp, ci, va)
    v0d = torch.from_numpy(np.array(v0)).cuda()
    w1, X1, i1 = eigs(A, 4, which="LA", ncv=20, tol=TOL[dtype], v0=v0d)
    w2, X2, i2 = eigs_native(A, 4, which="LA", ncv=20, tol=TOL[dtype], v0=v0d)
    torch.cuda.synchronize()
    A.close()
    print(f"eigs {np.dtype(dtype).name} rand1023 LA: host-driven {w1} ({i1['restarts']} restarts), native {w2} ({i2['restarts']} restarts)")
    assert i1["nconv"] == i2["nconv"] == 4 and X1.shape == X2.shape == (n, 4)
    assert np.all(np.abs(w1 - w2) <= i1["residuals"] + i2["residuals"])
