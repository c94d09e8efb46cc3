"""cfs_hip_sym_pcg_cheb, cfs_hip_sym_cheb_apply and cfs_hip_sym_precond_lmax step by step, by the method of
test_gpu_pcg_steps.py: what the kernels of csrc/cfs_solver_cheb.hpp (and, for p . q and the direction step of
the outer iteration, cg_dot_kernel and cg_direction_kernel<V, 0, P_RZ0, OneColumn> of csrc/cfs_solver.hpp)
compute against the same recurrences in np.longdouble on the CPU, the product as long-double row sums of the
CSR (oracle.csr_spmv_ldx).

    z = P_m r:   z_1 = d_1 = (1/theta) M^-1 r;   t = A z_j;  d_{j+1} = c1_j d_j + c2_j M^-1 (r - t);  z_{j+1} = z_j + d_{j+1}
    PCG:         r = b - A u;  z = P_m r;  p = z;  rz = r.z
                 q = A p;  alpha = rz / p.q;  u += alpha p;  r -= alpha q;  z = P_m r;  rz' = r.z;  rr' = r.r
                 beta = rz' / rz;  p = z + beta p
    power:       t = A v;  w = M^-1 t;  est = (w.t) / (v.t);  v = w / sqrt(w.w)

theta, c1_j, c2_j are the fp64 numbers the host passes to the kernels (solver.cheb_coeffs, bit for bit those of
cfs_hip_debug_cheb_coeffs: test_pcg_cheb_abi.py), converted exactly: they define the operator.  M^-1 is 1, dinv =
1 / a_ii of the diagonal rounded to the value type, or the inverse node blocks the library stores
(A.block_inverse(3), converted exactly, as test_gpu_block_pcg_steps.py does).

Tolerance, as everywhere in this suite: each recurrence is run a second time on the CPU in the working precision
with the kernels' rounding rules -- z, d, t, w, v and the products stored in the value type; every update computed
in fp64 from the stored operands and rounded once; M^-1 (r - t) formed in fp64 from (double)r_i - (double)t_i;
dinv_i = (V)(1.0 / (double)a_ii); dots accumulated in fp64 over the stored values, r.r from the unrounded update.
d is that run's deviation from the long-double run; the GPU, which differs from it only in the order of the
additions inside the products and the dots, is allowed 4 d + 16 u (u = 2^-53 / 2^-24).  A case whose d exceeds
D_LIMIT (1e-6 / 1e-2) is badly chosen and fails.  Neither the reference nor d involves the library.

The bounds are passed explicitly wherever a recurrence is pinned: lmax = the Gershgorin bound ||M^-1 A||inf computed
on the host, lmin = lmax / 30, so that these tests do not rest on the power method.  (On the symmetrically scaled
matrices that bound is loose -- D^-1 A keeps its spectrum under the scaling, its row sums do not: 112 against a
lambda_max of 1.3 on pwtk@0.05 -- which suits a test of the arithmetic: every case is well inside the margin.)

Measured on the MI355X (d / the GPU's deviation):

  cheb_apply  f64 pwtk@0.05 jacobi m=5          1.2e-16/1.3e-16    symmetry 1.1e-18
  cheb_apply  f32 pwtk@0.05 jacobi m=5          6.8e-08/6.8e-08    symmetry 5.1e-10
  cheb_apply  f64 rotated3 block_jacobi m=5     1.1e-14/1.1e-14    symmetry 5.2e-18
  cheb_apply  f32 rotated3 block_jacobi m=5     7.4e-06/3.0e-06    symmetry 4.1e-09
  iterates    f64 band20001 (two shards) m=3 k=10   3.7e-16/5.3e-16
  iterates    f32 band20001 (two shards) m=3 k=10   2.1e-07/2.4e-07
  estimate    f64 rand1026 block_jacobi         1.2e-16/2.1e-17    est 1.5327 <= lambda_max 1.5935
  lap2d(40, 33): Jacobi PCG 172 iterations, degree 4 with the default bounds (0.0712, 2.137) 48; lmax = half the
  Gershgorin bound (98.3): 165 iterations, converged; lmax = half the estimate (0.971): 200 iterations, relres 8.9
  reported, 8.9 in long double.
"""
import ctypes as C

import numpy as np
import pytest

from test_gpu_block_pcg_steps import rotated_node_blocks
from test_gpu_cg_steps import DET, DTYPES, _true_relres
from test_gpu_kernel_variants import PLAN_KNOBS
from test_gpu_lanczos_steps import default_v0
from test_gpu_lobpcg_steps import lap2d
from test_gpu_pcg_steps import D_LIMIT, KS, UNIT, _deviation, _matrix, _rhs, scaled

pytestmark = pytest.mark.gpu

LD = np.longdouble
RAND = [f"rand{n}" for n in (1, 2, 3, 5, 63, 64, 65, 255, 257, 1023, 1026)]
APPLY_MATRICES = RAND + ["pwtk@0.05"]
DEGREES = (1, 2, 3, 5)
BASES = {"none": 0, "jacobi": 1, "block_jacobi": 3}


@pytest.fixture(autouse=True)
def _torch_first(monkeypatch):
    """torch brings a HIP runtime of its own: it has to initialise before libcfs_hip.so's"""
    import torch
    torch.cuda.init()
    torch.cuda.set_device(0)
    for k in PLAN_KNOBS + ("CFS_HIP_CG_GRAPH",):
        monkeypatch.delenv(k, raising=False)
    yield


# ---- the CPU side -------------------------------------------------------------------------------------
class Problem:
    """a matrix in the value type, its product and its base preconditioner M^-1 in long double (dtype None) and in
    the working precision; minv: the (nb, bs, bs) inverse blocks for base "block_jacobi" """

    def __init__(self, n, rp, ci, va, base, minv=None):
        import scipy.sparse as sp
        self.n, self.rp, self.ci, self.va, self.base, self.minv = n, rp, ci, va, base, minv
        self.dtype = va.dtype.type
        self.A = sp.csr_matrix((va, ci.copy(), rp.copy()), shape=(n, n))
        self.diag = self.A.diagonal().astype(va.dtype)

    def prec(self, dtype):
        return (LD, LD) if dtype is None else (dtype, np.float64)

    def mv(self, x, dtype):
        from oracle import oracle
        if dtype is None:
            return oracle.csr_spmv_ldx(self.n, self.rp, self.ci, self.va, x)
        return (self.A @ x).astype(dtype)

    def apply(self, x, dtype):
        """M^-1 x for x in the scalar precision S"""
        S = self.prec(dtype)[1]
        if self.base == "none":
            return x
        if self.base == "jacobi":
            if dtype is None:
                return x * (1 / self.diag.astype(LD))
            return x * (1.0 / self.diag.astype(np.float64)).astype(dtype).astype(S)
        nb, bs, _ = self.minv.shape
        M = self.minv.astype(S)
        xp = np.zeros(nb * bs, S)
        xp[:self.n] = x
        xb = xp.reshape(nb, bs)
        z = np.zeros((nb, bs), S)
        for j in range(bs):  # (ascending j, as the kernels)
            z += M[:, :, j] * xb[:, j:j + 1]
        return z.reshape(-1)[:self.n]

    def minv_sparse(self):
        """M^-1 as stored, in fp64"""
        import scipy.sparse as sp
        if self.base == "none":
            return sp.identity(self.n, format="csr")
        if self.base == "jacobi":
            return sp.diags((1.0 / self.diag.astype(np.float64)).astype(self.dtype).astype(np.float64)).tocsr()
        nb = self.minv.shape[0]
        B = sp.bsr_matrix((self.minv.astype(np.float64), np.arange(nb), np.arange(nb + 1))).tocsr()
        return B[:self.n, :self.n]

    def gershgorin(self):
        """||M^-1 A||inf >= lambda_max(M^-1 A)"""
        P = (self.minv_sparse() @ self.A.astype(np.float64)).tocsr()
        return float(np.max(np.abs(P).sum(axis=1)))

    def bounds(self):
        lmax = self.gershgorin()
        return lmax / 30.0, lmax


def coeffs(degree, lmin, lmax):
    from cfs_spmv_amd.solver import cheb_coeffs
    theta, pairs = cheb_coeffs(degree, lmin, lmax)
    return 1.0 / theta, pairs


def poly_reference(P, r, degree, lmin, lmax, dtype=None):
    """z = P_m r of r (already in the value type)"""
    W, S = P.prec(dtype)
    inv_theta, pairs = coeffs(degree, lmin, lmax)
    rs = r.astype(S)
    d = (S(inv_theta) * P.apply(rs, dtype)).astype(W)
    z = d.copy()
    for c1, c2 in pairs:
        t = P.mv(z, dtype)
        d = (S(c1) * d.astype(S) + S(c2) * P.apply(rs - t.astype(S), dtype)).astype(W)
        z = (z.astype(S) + d.astype(S)).astype(W)
    return z


def pcg_cheb_reference(P, b, degree, lmin, lmax, ks=(), dtype=None, tol=0.0, maxiter=None, x0=None):
    """{k: (u_k, iterations done)} from u = x0 (0) with the kernels' guards (alpha = 0 when p.q = 0, beta = 0 when r.z = 0,
    nothing more once r.r is not > tol^2 b.b); out["count"] = iterations until then"""
    W, S = P.prec(dtype)
    u = np.zeros(P.n, W) if x0 is None else x0.astype(W)
    r = (b.astype(S) - P.mv(u, dtype).astype(S)).astype(W)
    rr = np.dot(r.astype(S), r.astype(S))
    stop = S(tol) * S(tol) * np.dot(b.astype(S), b.astype(S))
    out, it, done = {}, 0, not (rr > stop)
    if not done:
        z = poly_reference(P, r, degree, lmin, lmax, dtype)
        p = z.copy()
        rz = np.dot(r.astype(S), z.astype(S))
    last = max(tuple(ks) + (maxiter or 0,))
    for k in range(0, last + 1):
        if k > 0 and not done:
            q = P.mv(p, dtype)
            pq = np.dot(p.astype(S), q.astype(S))
            alpha = rz / pq if pq != 0 else S(0)
            u = (u.astype(S) + alpha * p.astype(S)).astype(W)
            rs = r.astype(S) - alpha * q.astype(S)
            rrn = np.dot(rs, rs)
            r = rs.astype(W)
            z = poly_reference(P, r, degree, lmin, lmax, dtype)
            rzn = np.dot(r.astype(S), z.astype(S))
            beta = rzn / rz if rz != 0 else S(0)
            p = (z.astype(S) + beta * p.astype(S)).astype(W)
            rz, it, done = rzn, it + 1, not (rrn > stop)
        if k in ks:
            out[k] = (u.copy(), it)
        if done and maxiter is not None:
            break
    out["count"], out["u"] = it, u
    return out


def power_reference(P, v0, steps, dtype=None):
    W, S = P.prec(dtype)
    v = v0.astype(W)
    est = None
    for s in range(steps):
        t = P.mv(v, dtype)
        w = P.apply(t.astype(S), dtype).astype(W)
        est = np.dot(w.astype(S), t.astype(S)) / np.dot(v.astype(S), t.astype(S))
        ww = np.dot(w.astype(S), w.astype(S))
        v = (w.astype(S) / np.sqrt(ww)).astype(W)
    return est


# ---- the GPU side -------------------------------------------------------------------------------------
def _problem(name, dtype, base, A=None, block=3):
    """(Problem, handle): the scaled matrix of test_gpu_pcg_steps.py ("rotated<bs>": rotated_node_blocks(bs) as it
    is); the inverse blocks of `block` rows from the handle"""
    import torch
    import cfs_spmv_amd as cfs
    if name.startswith("rotated"):
        n, rp, ci, va, _ = rotated_node_blocks(int(name[7:]))
        va = va.astype(dtype)
    else:
        n, rp, ci, va = _matrix(name)
        va = scaled(n, rp, ci, va, dtype)
    if A is None:
        A = cfs.SymMatrix(n, rp, ci, va)
    minv = None
    if base == "block_jacobi":
        minv = A.block_inverse(block)
        torch.cuda.synchronize()
        minv = minv.cpu().numpy()
    return Problem(n, rp, ci, va, base, minv), A


def _apply_gpu(A, r, base, degree, lmin, lmax, block=3):
    import torch
    rd = torch.from_numpy(r).cuda()
    z = torch.full_like(rd, float("nan"))
    A.cheb_apply(z, rd, lmin, lmax, base=base, block=block, degree=degree)
    torch.cuda.synchronize()
    return z.cpu().numpy()


def _native(A, b, x0=None, **kw):
    import torch
    from cfs_spmv_amd.solver import pcg_cheb_native
    x0 = None if x0 is None else torch.from_numpy(x0).cuda()
    u, it, res, used = pcg_cheb_native(A, torch.from_numpy(b).cuda(), x0=x0, **kw)
    torch.cuda.synchronize()
    return u.cpu().numpy(), it, res, used


def _bases(name):
    return ("none", "jacobi", "block_jacobi") if name.startswith("rand") or name == "rotated3" else ("none", "jacobi")


# ---- 1. the polynomial alone ---------------------------------------------------------------------------
@DTYPES
@pytest.mark.parametrize("name", APPLY_MATRICES + ["rotated3"])
def test_cheb_apply_against_the_long_double_recurrence(name, dtype):
    """z = P_m r for m = 1, 2, 3, 5 and every base, and its symmetry: x . P y against y . P x, within the same
    bound times ||x|| ||P y||"""
    errors, A = [], None
    for base in _bases(name):
        P, A = _problem(name, dtype, base, A)
        n = P.n
        lmin, lmax = P.bounds()
        x, y = _rhs(n, dtype), np.random.default_rng(n + 77).uniform(-1, 1, n).astype(dtype)
        for m in DEGREES:
            ref = poly_reference(P, x, m, lmin, lmax)
            d = _deviation(poly_reference(P, x, m, lmin, lmax, dtype), ref)
            assert d <= D_LIMIT[dtype], f"{name} {base} m={m}: d = {d:.3e}: badly conditioned case"
            px, py = _apply_gpu(A, x, base, m, lmin, lmax), _apply_gpu(A, y, base, m, lmin, lmax)
            assert px.dtype == dtype and np.all(np.isfinite(px))
            g, allowed = _deviation(px, ref), 4 * d + 16 * UNIT[dtype]
            xl, yl, pxl, pyl = (v.astype(LD) for v in (x, y, px, py))
            asym = float(abs(np.dot(xl, pyl) - np.dot(yl, pxl)) / (np.sqrt(np.dot(xl, xl)) * np.sqrt(np.dot(pyl, pyl))))
            print(f"cheb-apply {np.dtype(dtype).name} {name} {base} n={n} m={m} bounds=({lmin:.4g}, {lmax:.4g}) d={d:.3e} "
                  f"gpu={g:.3e} allowed={allowed:.3e} asym={asym:.3e}")
            if not g <= allowed:
                errors.append(f"{base} m={m}: deviation {g:.3e}, allowed {allowed:.3e} (d = {d:.3e})")
            if not asym <= allowed:
                errors.append(f"{base} m={m}: |x.Py - y.Px| / (||x|| ||Py||) = {asym:.3e}, allowed {allowed:.3e}")
    A.close()
    assert not errors, f"{name} {np.dtype(dtype).name}: " + "; ".join(errors)


# ---- 2. the iterates ----------------------------------------------------------------------------------
def _check_iterates(name, P, b, dtype, degree, lmin, lmax, run, label="", ks=KS, x0=None):
    """run(k) -> (u_k, iterations) on the GPU from u = x0 (0); asserts every k of ks against the long-double iterate"""
    ref = pcg_cheb_reference(P, b, degree, lmin, lmax, ks, x0=x0)
    work = pcg_cheb_reference(P, b, degree, lmin, lmax, ks, dtype, x0=x0)
    errors = []
    for k in ks:
        u_ref, _ = ref[k]
        d = _deviation(work[k][0], u_ref)
        assert d <= D_LIMIT[dtype], f"{name} {P.base} m={degree}: d_{k} = {d:.3e}: badly conditioned case"
        u, it = run(k)
        g, allowed = _deviation(u, u_ref), 4 * d + 16 * UNIT[dtype]
        print(f"pcg-cheb-steps {np.dtype(dtype).name} {name}{label} {P.base} m={degree} n={P.n} k={k} d_k={d:.3e} gpu={g:.3e} "
              f"allowed={allowed:.3e} it={it}")
        # fewer than k iterations only where the recurrence's residual can vanish: the Krylov space is exhausted
        # (after n iterations -- or after the first when a single block makes M the matrix itself)
        if not (it == k if k < P.n and (P.base != "block_jacobi" or P.minv.shape[0] > 1) else 1 <= it <= k):
            errors.append(f"k={k}: {it} iterations")
        if not g <= allowed:
            errors.append(f"k={k}: deviation {g:.3e} from the long-double iterate, allowed {allowed:.3e} (d_k = {d:.3e})")
    return [f"{P.base} m={degree}{label}: " + e for e in errors]


@DTYPES
@pytest.mark.parametrize("name", APPLY_MATRICES)
def test_iterates_against_the_long_double_recurrence(name, dtype):
    errors, A = [], None
    b = None
    for base in _bases(name)[1:] + _bases(name)[:1]:
        P, A = _problem(name, dtype, base, A)
        b = _rhs(P.n, dtype)
        lmin, lmax = P.bounds()
        for m in (1, 3):
            errors += _check_iterates(name, P, b, dtype, m, lmin, lmax,
                                      lambda k: _native(A, b, base=base, block=3, degree=m, lmin=lmin, lmax=lmax, tol=0.0,
                                                        maxiter=k)[:2])
    A.close()
    assert not errors, f"{name} {np.dtype(dtype).name}: " + "; ".join(errors)


@DTYPES
def test_iterates_through_a_two_shard_handle(dtype):
    """an odd n through a multi-device handle (two shards, here on one device): the diagonal gathered and every
    product, the inner ones included, computed on the shards' streams, the vector kernels on the caller's"""
    import cfs_spmv_amd as cfs
    n, rp, ci, va = _matrix("band20001")
    va, b = scaled(n, rp, ci, va, dtype), _rhs(n, dtype)
    M = cfs.SymMatrix(n, rp, ci, va, ngpus=2)
    P = Problem(n, rp, ci, va, "jacobi")
    lmin, lmax = P.bounds()
    errors = []
    for m in (1, 3):
        errors += _check_iterates("band20001", P, b, dtype, m, lmin, lmax,
                                  lambda k: _native(M, b, degree=m, lmin=lmin, lmax=lmax, tol=0.0, maxiter=k)[:2],
                                  label=" (two shards)")
    # block Jacobi on a multi-device handle is out of scope
    from cfs_spmv_amd import _lib
    with pytest.raises(_lib.CfsHipError) as e:
        _native(M, b, base="block_jacobi", block=3, lmin=lmin, lmax=lmax, maxiter=2)
    assert e.value.code == _lib.ERR_UNSUPPORTED
    M.close()
    assert not errors, "; ".join(errors)


@DTYPES
def test_iterates_of_a_deterministic_handle(dtype):
    import cfs_spmv_amd as cfs
    n, rp, ci, va = _matrix("Flan_1565@0.01")
    va, b = scaled(n, rp, ci, va, dtype), _rhs(n, dtype)
    D = cfs.SymMatrix(n, rp, ci, va, options=cfs.make_options(flags=DET))
    assert D.kernel_variant()["det"] == 1
    P = Problem(n, rp, ci, va, "jacobi")
    lmin, lmax = P.bounds()
    errors = []
    for m in (1, 3):
        errors += _check_iterates("Flan_1565@0.01", P, b, dtype, m, lmin, lmax,
                                  lambda k: _native(D, b, degree=m, lmin=lmin, lmax=lmax, tol=0.0, maxiter=k)[:2],
                                  label=" (deterministic)")
    assert not errors, "; ".join(errors)
    # ... and the whole solve is bit-reproducible, the estimate of the default bounds included
    for kw in (dict(lmin=lmin, lmax=lmax), dict()):
        ua, ita, _, useda = _native(D, b, degree=3, tol=0.0, maxiter=12, **kw)
        ub, itb, _, usedb = _native(D, b, degree=3, tol=0.0, maxiter=12, check_every=5, **kw)
        assert ita == itb == 12 and useda == usedb and np.array_equal(ua.view(np.uint8), ub.view(np.uint8))
    D.close()


# ---- 3. the power method --------------------------------------------------------------------------------
@DTYPES
@pytest.mark.parametrize("name", APPLY_MATRICES)
def test_precond_lmax_against_the_long_double_power_method(name, dtype):
    """16 steps from an explicit v0 and from the default one; on the dense-sized cases the estimate is a LOWER one:
    est <= lambda_max(M^-1/2 A M^-1/2) (1 + 64 u), M^-1 as stored, lambda_max from numpy.linalg.eigvalsh"""
    import torch
    errors, A = [], None
    for base in _bases(name)[1:]:
        P, A = _problem(name, dtype, base, A)
        n = P.n
        lam = None
        if n <= 1026:
            Mi = P.minv_sparse().toarray()
            L = np.linalg.cholesky(Mi)  # M^-1 = L L^T: L^T A L has the spectrum of M^-1/2 A M^-1/2
            lam = float(np.linalg.eigvalsh(L.T @ P.A.astype(np.float64).toarray() @ L)[-1])
        for label, v0 in (("explicit v0", _rhs(n, dtype)), ("default v0", None)):
            start = default_v0(n).astype(dtype) if v0 is None else v0
            ref = power_reference(P, start, 16)
            d = float(abs(LD(power_reference(P, start, 16, dtype)) - ref) / abs(ref))
            assert d <= D_LIMIT[dtype], f"{name} {base}: d = {d:.3e}: badly conditioned case"
            est = A.precond_lmax(base=base, block=3, steps=16 if v0 is not None else 0,
                                 v0=None if v0 is None else torch.from_numpy(v0).cuda())
            g, allowed = float(abs(LD(est) - ref) / abs(ref)), 4 * d + 16 * UNIT[dtype]
            print(f"precond-lmax {np.dtype(dtype).name} {name} {base} {label} n={n} est={est:.17g} long double={float(ref):.17g} "
                  f"d={d:.3e} gpu={g:.3e} allowed={allowed:.3e} lambda_max={lam}")
            if not g <= allowed:
                errors.append(f"{base} {label}: estimate {est!r} against {float(ref)!r}: {g:.3e}, allowed {allowed:.3e}")
            if lam is not None and not est <= lam * (1 + 64 * UNIT[dtype]):
                errors.append(f"{base} {label}: estimate {est!r} above lambda_max {lam!r}")
    A.close()
    assert not errors, f"{name} {np.dtype(dtype).name}: " + "; ".join(errors)


# ---- 4. what it is for ----------------------------------------------------------------------------------
def _lap():
    n, rp, ci, va = lap2d(40, 33)
    va = scaled(n, rp, ci, va, np.float64)
    return n, rp, ci, va, _rhs(n, np.float64)


def test_what_the_preconditioner_is_for():
    """the scaled 2-D Laplacian, fp64, tol 1e-10, Jacobi base, degree 4, default bounds: at most half the outer
    iterations of Jacobi PCG on the same handle (numpy, before the kernels existed: 47 against 167; the factor 2
    leaves room for the different start vector of the estimate)"""
    import torch
    import cfs_spmv_amd as cfs
    from cfs_spmv_amd.solver import pcg_native
    n, rp, ci, va, b = _lap()
    tol = 1e-10
    A = cfs.SymMatrix(n, rp, ci, va)
    uj, itj, resj = pcg_native(A, torch.from_numpy(b).cuda(), precond="jacobi", tol=tol, maxiter=2000)
    u, it, res, (lmin, lmax) = _native(A, b, degree=4, tol=tol, maxiter=2000)
    true, slack = _true_relres(n, rp, ci, va, b, u, np.float64)
    est = A.precond_lmax()
    print(f"pcg-cheb-steps lap2d40x33: Jacobi {itj} iterations (relres {resj:.3e}), degree 4 {it} iterations, {4 * it + 3} products and 16 for the estimate "
          f"(relres {res:.3e}, long double {true:.3e}), bounds ({lmin:.6g}, {lmax:.6g}), Gershgorin {Problem(n, rp, ci, va, 'jacobi').gershgorin():.6g}")
    A.close()
    assert 0 < itj < 2000 and resj <= 10 * tol
    # the documented defaults (the estimate of a second call: equal up to the summation order inside the products)
    assert abs(lmax - 1.1 * est) <= 1e-10 * lmax and lmin == lmax / 30.0
    assert 0 < it and res <= 10 * tol and true <= 10 * tol + slack
    assert 2 * it <= itj, (it, itj)


def test_a_bad_lmax_is_reported_truthfully():
    """lmax = half the Gershgorin bound, and lmax = half the power-method estimate: whatever the bound is worth, the
    call returns without an error and what it reports is true.  (On this symmetrically scaled matrix the Gershgorin
    bound of D^-1 A is about 100 times lambda_max, so half of it is merely a loose bound; half the estimate is a LOW
    one -- eigenvalues of D^-1 A beyond lmin + lmax, the polynomial is indefinite and PCG promises nothing.)"""
    import cfs_spmv_amd as cfs
    n, rp, ci, va, b = _lap()
    A = cfs.SymMatrix(n, rp, ci, va)
    P = Problem(n, rp, ci, va, "jacobi")
    for what, lmax in (("Gershgorin", 0.5 * P.gershgorin()), ("estimate", 0.5 * A.precond_lmax())):
        u, it, res, used = _native(A, b, degree=4, lmax=lmax, tol=1e-10, maxiter=200)
        assert used == (lmax / 30.0, lmax) and 0 <= it <= 200
        if np.all(np.isfinite(u)):
            true, slack = _true_relres(n, rp, ci, va, b, u, np.float64)
            print(f"pcg-cheb-steps lap2d40x33 lmax = half the {what} = {lmax:.4g}: {it} iterations, reported {res:.6e}, "
                  f"long double {true:.6e}, slack {slack:.3e}")
            assert abs(res - true) <= slack, (what, res, true, slack)
        else:
            print(f"pcg-cheb-steps lap2d40x33 lmax = half the {what} = {lmax:.4g}: {it} iterations, reported {res}, u not finite")
            assert not np.isfinite(res)
    A.close()


# ---- 5. the remaining small checks --------------------------------------------------------------------------
@DTYPES
@pytest.mark.parametrize("base", ["jacobi", "block_jacobi"])
def test_a_base_that_is_not_positive_is_refused(base, dtype):
    """CFS_HIP_ERR_ARG, u untouched, *iterations = 0 -- as cfs_hip_sym_pcg / _pcg_block refuse it"""
    import torch
    import cfs_spmv_amd as cfs
    from cfs_spmv_amd import _lib
    n, rp, ci, va = _matrix("rand1023")
    va = scaled(n, rp, ci, va, dtype)
    rows = np.repeat(np.arange(n), np.diff(rp))
    va[int(np.flatnonzero((rows == ci) & (rows == 700))[0])] = -1.5
    A = cfs.SymMatrix(n, rp, ci, va)
    x0 = np.random.default_rng(5).uniform(-1, 1, n).astype(dtype)
    u, b = torch.from_numpy(x0).cuda(), torch.from_numpy(_rhs(n, dtype)).cuda()
    word = "positive diagonal" if base == "jacobi" else "positive definite"
    for kw in (dict(), dict(lmin=0.1, lmax=2.0), dict(degree=1, lmin=0.1, lmax=2.0)):
        with pytest.raises(_lib.CfsHipError, match=word) as e:
            A.pcg_cheb(u, b, base=base, block=3, tol=1e-8, maxiter=50, **kw)
        assert e.value.code == _lib.ERR_ARG
        torch.cuda.synchronize()
        assert np.array_equal(u.cpu().numpy().view(np.uint8), x0.view(np.uint8))
    it, res = C.c_int(9), C.c_double(9.0)
    rc = _lib.load().cfs_hip_sym_pcg_cheb(A._h, u.data_ptr(), b.data_ptr(), BASES[base], 4, 0.0, 0.0, 1e-8, 50, 8, C.byref(it),
                                          C.byref(res), None, torch.cuda.current_stream().cuda_stream)
    assert rc == _lib.ERR_ARG and it.value == 0
    with pytest.raises(_lib.CfsHipError, match=word):
        A.cheb_apply(torch.empty_like(b), b, 0.1, 2.0, base=base, block=3, degree=3)
    with pytest.raises(_lib.CfsHipError, match=word):
        A.precond_lmax(base=base, block=3)
    assert A.pcg_cheb(u, b, base="none", lmin=0.1, lmax=200.0, tol=0.0, maxiter=2)[0] == 2  # M = I still takes the matrix
    A.close()


@DTYPES
def test_argument_checks_on_the_device(dtype):
    import torch
    import cfs_spmv_amd as cfs
    from cfs_spmv_amd import _lib
    n, rp, ci, va = _matrix("rand1023")
    va = va.astype(dtype)
    A = cfs.SymMatrix(n, rp, ci, va)
    good = torch.zeros(n, dtype=torch.from_numpy(va).dtype, device="cuda")
    host = np.zeros(n, dtype)
    for call in (lambda: A.pcg_cheb(host, good, lmin=0.1, lmax=2.0, maxiter=5), lambda: A.cheb_apply(good, host, 0.1, 2.0),
                 lambda: A.precond_lmax(v0=host)):
        with pytest.raises(_lib.CfsHipError) as e:  # a host pointer
            call()
        assert e.value.code == _lib.ERR_ARG
    with pytest.raises(ValueError):
        A.pcg_cheb(good, good.clone(), base="ilu")
    A.close()
    S = cfs.SymMatrix(n, rp, ci, va, row_splits=np.array([0, n // 2, n], np.int32), rank=1)
    for call in (lambda: S.pcg_cheb(good, good.clone(), lmin=0.1, lmax=2.0, maxiter=5),
                 lambda: S.pcg_cheb(good, good.clone(), base="none", lmin=0.1, lmax=2.0, maxiter=5),
                 lambda: S.cheb_apply(good, good.clone(), 0.1, 2.0), lambda: S.precond_lmax()):
        with pytest.raises(_lib.CfsHipError) as e:  # a shard
            call()
        assert e.value.code == _lib.ERR_UNSUPPORTED
    S.close()


@DTYPES
def test_iteration_count_and_reported_residual(dtype):
    import cfs_spmv_amd as cfs
    n, rp, ci, va = _matrix("pwtk@0.05")
    va, b = scaled(n, rp, ci, va, dtype), _rhs(n, dtype)
    A = cfs.SymMatrix(n, rp, ci, va)
    lmin, lmax = Problem(n, rp, ci, va, "jacobi").bounds()
    # tol = 0: exactly maxiter iterations, whatever the window of enqueued iterations
    for m, check_every, k in ((1, 1, 7), (1, 16, 23), (3, 3, 11), (3, 1000, 11), (16, 8, 3)):
        u, it, res, _ = _native(A, b, degree=m, lmin=lmin, lmax=lmax, tol=0.0, maxiter=k, check_every=check_every)
        assert it == k, (m, check_every, k, it)
        true, slack = _true_relres(n, rp, ci, va, b, u, dtype)
        print(f"pcg-cheb-steps {np.dtype(dtype).name} relres m={m} k={k} reported={res:.6e} long double={true:.6e} slack={slack:.3e}")
        assert abs(res - true) <= slack, (m, k, res, true, slack)
    # b = 0 (and u = 0): nothing to do;  a NaN in b ends the solve at once
    u, it, res, _ = _native(A, np.zeros(n, dtype), degree=3, lmin=lmin, lmax=lmax, tol=1e-8, maxiter=50)
    assert it == 0 and not u.any() and np.isfinite(res)
    b[n // 2] = np.nan
    for check_every in (1, 16):
        u, it, res, _ = _native(A, b, degree=3, lmin=lmin, lmax=lmax, tol=1e-8, maxiter=300, check_every=check_every)
        assert it <= 1 and np.isnan(res), (it, res)
    A.close()


@DTYPES
def test_convergence_inside_a_window_of_enqueued_iterations(dtype):
    """the iterations enqueued behind the converged one change neither u nor the count (degree 3: at most
    80 // 11 = 7 iterations between two looks)"""
    import cfs_spmv_amd as cfs
    n, rp, ci, va = _matrix("pwtk@0.05")
    va, b = scaled(n, rp, ci, va, dtype), _rhs(n, dtype)
    tol = 1e-8 if dtype == np.float64 else 1e-4
    D = cfs.SymMatrix(n, rp, ci, va, options=cfs.make_options(flags=DET))
    lmin, lmax = Problem(n, rp, ci, va, "jacobi").bounds()
    kw = dict(degree=3, lmin=lmin, lmax=lmax, tol=tol, maxiter=500)
    u1, it1, res1, _ = _native(D, b, check_every=1, **kw)
    assert 2 < it1 < 500 and res1 <= 10 * tol
    windows = [c for c in (2, 3, 4, 5, 6, 7) if it1 % c]  # the converged iteration is not the last of its window
    assert len(windows) >= 2, it1
    for check_every in windows:
        u2, it2, _, _ = _native(D, b, check_every=check_every, **kw)
        assert it2 == it1 and np.array_equal(u2.view(np.uint8), u1.view(np.uint8)), (check_every, it1, it2)
    D.close()


@DTYPES
def test_host_driven_and_native_loops_agree(dtype):
    """solver.pcg_cheb (torch-driven, the rounding rules restated with torch operations) against
    solver.pcg_cheb_native with the same bounds.  Its iterates obey the rule of the native ones (rand1023, every
    base); on the pwtk stand-in the iteration counts of converged solves agree within 1 and both answers lie within
    the bound test_gpu_pcg_steps.py holds the Jacobi solvers to against a direct solve at these tolerances."""
    import scipy.sparse as sp
    import scipy.sparse.linalg as spl
    import torch
    import cfs_spmv_amd as cfs
    from cfs_spmv_amd import synth
    from cfs_spmv_amd.solver import pcg_cheb
    errors, A = [], None
    for base in _bases("rand1023"):
        P, A = _problem("rand1023", dtype, base, A)
        b = _rhs(P.n, dtype)
        lmin, lmax = P.bounds()

        def run(k):
            u, it, _, _ = pcg_cheb(A, torch.from_numpy(b).cuda(), base=base, block=3, degree=3, lmin=lmin, lmax=lmax, tol=0.0,
                                   maxiter=k)
            return u.cpu().numpy(), it
        errors += _check_iterates("rand1023", P, b, dtype, 3, lmin, lmax, run, label=" (host-driven)", ks=(1, 2, 5))
    A.close()
    assert not errors, "; ".join(errors)
    n, rp, ci, va = _matrix("pwtk@0.05")
    va = va.astype(dtype)
    A = cfs.SymMatrix(n, rp, ci, va)
    b = synth.make_x(n, 11, dtype)
    bd = torch.from_numpy(b).cuda()
    tol, lim = (1e-11, 1e-9) if dtype == np.float64 else (2e-5, 2e-3)
    u1, it1, res1, used = pcg_cheb(A, bd, degree=4, tol=tol, maxiter=500)
    torch.cuda.synchronize()
    u_ref = spl.spsolve(sp.csc_matrix(sp.csr_matrix((va.astype(np.float64), ci, rp), shape=(n, n))), b.astype(np.float64))
    assert 0 < it1 < 500 and res1 <= 10 * tol
    assert np.max(np.abs(u1.cpu().numpy() - u_ref)) <= lim * np.max(np.abs(u_ref))
    for check_every in (1, 8):
        u2, it2, res2, used2 = _native(A, b, degree=4, lmin=used[0], lmax=used[1], tol=tol, maxiter=500, check_every=check_every)
        print(f"pcg-cheb-steps {np.dtype(dtype).name} pwtk@0.05: host-driven {it1} iterations, native {it2} (check_every={check_every})")
        assert used2 == used and 0 < it2 < 500 and abs(it2 - it1) <= 1, (it1, it2, check_every)
        assert res2 <= 10 * tol, (res1, res2)
        assert np.max(np.abs(u2 - u_ref)) <= lim * np.max(np.abs(u_ref))
        assert np.max(np.abs(u2 - u1.cpu().numpy())) <= 2 * lim * np.max(np.abs(u_ref))
    A.close()
