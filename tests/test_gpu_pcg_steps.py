"""cfs_hip_sym_pcg step by step, by the method of test_gpu_cg_steps.py: the ITERATES u_k of the native
Jacobi-preconditioned conjugate gradients (cfs_diag_gather_kernel and cg_dinv_kernel once, then
cg_residual_kernel, cg_dot_kernel, cg_update_kernel, cg_direction_kernel<V, 1, ..., OneColumn> behind the
SpMV) against the same recurrence in np.longdouble on the CPU,

    r = b - A u;  z = D^-1 r;  p = z;  rz = r.z
    q = A p;  alpha = rz / p.q;  u += alpha p;  r -= alpha q;  z = D^-1 r;  rz' = r.z;  rr' = r.r
    beta = rz' / rz;  p = z + beta p

with the product as long-double row sums of the CSR (oracle.csr_spmv_ldx) and dinv = 1 / a_ii in long
double from the diagonal rounded to the value type.  pcg_native(..., tol=0, maxiter=k) returns u after
exactly k iterations.

Tolerance for ||u_k(GPU) - u_k(long double)||inf / ||u_k(long double)||inf, derived exactly as in the plain
test: the recurrence is run a second time on the CPU in the working precision with the kernels' rounding
rules -- vectors and the product in fp64 / fp32, dots accumulated in fp64, the updates computed in fp64
and rounded, dinv_i = (V)(1.0 / (double)a_ii) stored in the value type, z_i = (double)r_i * (double)dinv_i
of the ROUNDED r_i kept in fp64 and never rounded (it feeds r.z and the direction update directly), r.r
from the unrounded update as in the plain kernels; d_k is its deviation from the long-double run.  A
correct GPU run differs from that CPU run only in the order of the additions inside the product and the
dots, so it is allowed 4 d_k + 16 u (u = 2^-53 / 2^-24).  Neither the reference nor d_k involves the
library.  A case whose d_k exceeds D_LIMIT of the plain test (1e-6 / 1e-2) is badly chosen and fails.

Matrices: the MATRICES of the plain test, each scaled symmetrically, a_ij -> 2^e_i a_ij 2^e_j with e_i
integers in [-4, 4] (default_rng(7)): the scaling is exact in both value types, and it makes a wrong or
missing dinv move u_1 by orders of magnitude.

Measured on the MI355X (value type, matrix, then for k = 1, 2, 3, 5, 10: d_k / the GPU's deviation):

  f64 pwtk@0.05                     4.2e-16/1.5e-16  4.9e-16/3.0e-16  2.3e-16/2.9e-16  2.5e-16/3.4e-16  2.6e-16/3.9e-16
  f32 pwtk@0.05                     6.8e-08/6.8e-08  2.1e-07/7.5e-08  1.3e-07/6.9e-08  1.7e-07/1.2e-07  1.6e-07/1.1e-07
  f64 Flan_1565@0.01                2.8e-16/2.8e-16  5.3e-16/3.9e-16  2.9e-16/2.3e-16  3.4e-16/2.4e-16  3.9e-16/2.6e-16
  f32 Flan_1565@0.01                7.4e-08/7.4e-08  3.5e-07/1.7e-07  2.2e-07/9.8e-08  2.3e-07/1.2e-07  2.2e-07/1.6e-07
  f64 rand1                         0.0e+00/0.0e+00  0.0e+00/0.0e+00  0.0e+00/0.0e+00  0.0e+00/0.0e+00  0.0e+00/0.0e+00
  f32 rand1                         0.0e+00/0.0e+00  0.0e+00/0.0e+00  0.0e+00/0.0e+00  0.0e+00/0.0e+00  0.0e+00/0.0e+00
  f64 rand2                         5.4e-17/5.4e-17  1.1e-16/1.1e-16  1.1e-16/1.1e-16  1.1e-16/1.1e-16  1.1e-16/1.1e-16
  f32 rand2                         2.9e-09/2.9e-09  3.7e-08/3.7e-08  3.7e-08/3.7e-08  3.7e-08/3.7e-08  3.7e-08/3.7e-08
  f64 rand3                         9.6e-17/9.6e-17  2.0e-16/7.9e-17  1.6e-16/6.1e-17  1.6e-16/6.1e-17  1.6e-16/6.1e-17
  f32 rand3                         5.5e-08/5.5e-08  7.1e-08/7.1e-08  8.6e-08/8.6e-08  8.6e-08/8.6e-08  8.6e-08/8.6e-08
  f64 rand5                         9.5e-17/9.5e-17  1.4e-16/7.8e-17  9.9e-17/1.1e-16  1.5e-16/1.5e-16  1.5e-16/1.5e-16
  f32 rand5                         5.7e-08/5.7e-08  3.0e-08/1.1e-07  6.7e-08/1.4e-07  8.0e-08/1.3e-07  8.0e-08/1.3e-07
  f64 rand63                        8.2e-17/1.4e-16  1.4e-16/1.0e-16  1.0e-16/1.1e-16  1.4e-16/1.0e-16  1.9e-16/7.6e-17
  f32 rand63                        5.0e-08/5.0e-08  4.5e-08/4.4e-08  3.0e-08/3.8e-08  6.8e-08/6.8e-08  7.2e-08/7.2e-08
  f64 rand64                        9.5e-17/2.6e-16  6.7e-17/1.1e-16  9.2e-17/1.1e-16  6.5e-17/6.5e-17  1.1e-16/1.1e-16
  f32 rand64                        2.3e-08/2.3e-08  3.3e-08/3.3e-08  4.3e-08/4.3e-08  5.3e-08/5.3e-08  6.2e-08/6.2e-08
  f64 rand65                        1.6e-16/1.6e-16  2.7e-16/8.0e-17  3.2e-16/1.1e-16  4.1e-16/1.3e-16  5.0e-16/1.4e-16
  f32 rand65                        4.0e-08/2.2e-08  8.8e-08/8.0e-08  1.1e-07/1.1e-07  1.2e-07/1.2e-07  1.5e-07/1.3e-07
  f64 rand255                       4.3e-16/2.5e-16  2.2e-16/7.7e-17  2.0e-16/8.2e-17  1.3e-16/7.9e-17  1.8e-16/1.6e-16
  f32 rand255                       5.8e-08/5.8e-08  6.1e-08/6.1e-08  1.0e-07/1.0e-07  9.6e-08/9.6e-08  1.8e-07/1.8e-07
  f64 rand257                       1.5e-16/1.3e-16  1.5e-16/9.1e-17  2.1e-16/1.1e-16  1.8e-16/1.3e-16  3.2e-16/1.9e-16
  f32 rand257                       4.3e-08/4.9e-08  6.1e-08/7.9e-08  7.1e-08/7.1e-08  9.8e-08/9.8e-08  1.6e-07/1.6e-07
  f64 rand1023                      5.1e-16/1.0e-16  2.6e-16/1.7e-16  1.6e-16/1.7e-16  2.5e-16/1.4e-16  2.2e-16/1.6e-16
  f32 rand1023                      4.3e-08/4.3e-08  5.8e-08/5.8e-08  5.9e-08/5.9e-08  6.8e-08/6.8e-08  9.3e-08/9.3e-08
  f64 rand1026                      7.8e-17/1.2e-16  1.3e-16/1.8e-16  1.4e-16/2.5e-16  1.1e-16/2.0e-16  1.3e-16/1.7e-16
  f32 rand1026                      5.6e-08/5.6e-08  8.4e-08/8.4e-08  8.1e-08/8.9e-08  7.6e-08/7.6e-08  1.4e-07/1.4e-07
  f64 band600001                    4.4e-16/2.7e-16  3.7e-16/3.6e-16  3.6e-16/3.8e-16  3.9e-16/4.3e-16  4.3e-16/4.8e-16
  f32 band600001                    1.2e-07/1.2e-07  1.6e-07/1.2e-07  1.7e-07/1.2e-07  1.7e-07/1.6e-07  2.5e-07/2.2e-07
  f64 band20001 (two shards)        4.1e-16/2.2e-16  3.0e-16/2.6e-16  2.8e-16/3.1e-16  3.3e-16/2.9e-16  4.1e-16/3.6e-16
  f32 band20001 (two shards)        7.4e-08/7.4e-08  1.5e-07/8.1e-08  1.7e-07/1.1e-07  1.7e-07/1.4e-07  2.0e-07/2.0e-07
  f64 Flan_1565@0.01 (deterministic)  2.8e-16/1.5e-16  5.3e-16/2.8e-16  2.9e-16/1.8e-16  3.4e-16/2.1e-16  3.9e-16/2.6e-16
  f32 Flan_1565@0.01 (deterministic)  7.4e-08/7.4e-08  3.5e-07/1.7e-07  2.2e-07/9.8e-08  2.3e-07/1.2e-07  2.2e-07/1.6e-07

  f64 rand1023 (captured graph)  k = 4: 2.7e-16/1.5e-16  k = 5: 2.5e-16/1.4e-16
"""
import numpy as np
import pytest

from test_gpu_cg_steps import D_LIMIT, DET, DTYPES, KS, MATRICES, UNIT, _deviation, _matrix, _rhs, _true_relres
from test_gpu_kernel_variants import PLAN_KNOBS

pytestmark = pytest.mark.gpu

SCALE_SEED = 7


@pytest.fixture(autouse=True)
def _torch_first(monkeypatch):
    """torch brings a HIP runtime of its own: it has to initialise before libcfs_hip.so's"""
    import torch
    torch.cuda.init()
    torch.cuda.set_device(0)
    for k in PLAN_KNOBS + ("CFS_HIP_CG_GRAPH",):
        monkeypatch.delenv(k, raising=False)
    yield


def scaled(n, rp, ci, va, dtype, spread=4):
    """S A S with S = diag(2^e_i), e_i integers in [-spread, spread]: exact in `dtype`"""
    e = np.random.default_rng(SCALE_SEED).integers(-spread, spread + 1, n)
    s = np.ldexp(1.0, e).astype(dtype)
    rows = np.repeat(np.arange(n), np.diff(rp))
    out = va.astype(dtype) * s[rows] * s[ci]
    assert out.dtype == dtype and np.array_equal(np.ldexp(out.astype(np.float64), -(e[rows] + e[ci])).astype(dtype),
                                                 va.astype(dtype))
    return out


def _diag(n, rp, ci, va):
    import scipy.sparse as sp
    return sp.csr_matrix((va, ci, rp), shape=(n, n)).diagonal().astype(va.dtype)


def pcg_reference(n, rp, ci, va, b, ks=(), dtype=None, x0=None, tol=0.0, maxiter=None):
    """{k: (u_k, iterations done)} of the Jacobi recurrence above from u = x0 (0), with the kernels' guards
    (alpha = 0 when p.q = 0, beta = 0 when r.z = 0, nothing more once r.r is not > tol^2 b.b); with `maxiter`
    also out["count"] = iterations until then.  va is already in the value type.
    dtype None: np.longdouble throughout.  Otherwise the working precision of the kernels, see above."""
    import scipy.sparse as sp
    from oracle import oracle
    ld = dtype is None
    W, S = (np.longdouble, np.longdouble) if ld else (dtype, np.float64)
    d = _diag(n, rp, ci, va)
    if ld:
        dinv = 1 / d.astype(np.longdouble)

        def mv(x):
            return oracle.csr_spmv_ldx(n, rp, ci, va, x)
    else:
        dinv = (1.0 / d.astype(np.float64)).astype(dtype).astype(S)
        A = sp.csr_matrix((va.astype(dtype), ci, rp), shape=(n, n))

        def mv(x):
            return (A @ x).astype(dtype)
    u = np.zeros(n, W) if x0 is None else x0.astype(W)
    r = (b.astype(S) - mv(u).astype(S)).astype(W)
    z = r.astype(S) * dinv
    p = z.astype(W)
    rz, rr = np.dot(r.astype(S), z), np.dot(r.astype(S), r.astype(S))
    stop = S(tol) * S(tol) * np.dot(b.astype(S), b.astype(S))
    out, it, done = {}, 0, not (rr > stop)
    last = max(tuple(ks) + (maxiter or 0,))
    for k in range(0, last + 1):
        if k > 0 and not done:
            q = mv(p)
            pq = np.dot(p.astype(S), q.astype(S))
            alpha = rz / pq if pq != 0 else S(0)
            u = (u.astype(S) + alpha * p.astype(S)).astype(W)
            rs = r.astype(S) - alpha * q.astype(S)
            rrn = np.dot(rs, rs)
            r = rs.astype(W)
            z = r.astype(S) * dinv
            rzn = np.dot(r.astype(S), z)
            beta = rzn / rz if rz != 0 else S(0)
            p = (z + beta * p.astype(S)).astype(W)
            rz, it, done = rzn, it + 1, not (rrn > stop)
        if k in ks:
            out[k] = (u.copy(), it)
        if done and maxiter is not None:
            break
    out["count"], out["u"] = it, u
    return out


def plain_count(n, rp, ci, va, b, dtype, tol, maxiter):
    """iterations of the plain recurrence (test_gpu_cg_steps.cg_reference's, with its stopping rule at
    tol) in the working precision"""
    import scipy.sparse as sp
    S = np.float64
    A = sp.csr_matrix((va.astype(dtype), ci, rp), shape=(n, n))
    u = np.zeros(n, dtype)
    r = b.astype(dtype).copy()
    p = r.copy()
    rr = np.dot(r.astype(S), r.astype(S))
    stop = tol * tol * np.dot(b.astype(S), b.astype(S))
    it = 0
    while it < maxiter and rr > stop:
        q = (A @ p).astype(dtype)
        pq = np.dot(p.astype(S), q.astype(S))
        alpha = rr / pq if pq != 0 else S(0)
        u = (u.astype(S) + alpha * p.astype(S)).astype(dtype)
        rs = r.astype(S) - alpha * q.astype(S)
        rrn = np.dot(rs, rs)
        r = rs.astype(dtype)
        p = (r.astype(S) + (rrn / rr if rr != 0 else S(0)) * p.astype(S)).astype(dtype)
        rr, it = rrn, it + 1
    return it


def _native(A, b, torch, **kw):
    from cfs_spmv_amd.solver import pcg_native
    u, it, res = pcg_native(A, torch.from_numpy(b).cuda(), **kw)
    torch.cuda.synchronize()
    return u.cpu().numpy(), it, res


def _check_iterates(name, n, rp, ci, va, b, dtype, run, label="", ks=KS):
    """run(k) -> (u_k, iterations) on the GPU; asserts every k of ks against the long-double iterate"""
    ref = pcg_reference(n, rp, ci, va, b, ks)
    work = pcg_reference(n, rp, ci, va, b, ks, dtype)
    errors = []
    for k in ks:
        u_ref, it_ref = ref[k]
        d = _deviation(work[k][0], u_ref)
        assert d <= D_LIMIT[dtype], f"{name}: d_{k} = {d:.3e}: badly conditioned case"
        u, it = run(k)
        g = _deviation(u, u_ref)
        allowed = 4 * d + 16 * UNIT[dtype]
        print(f"pcg-steps {np.dtype(dtype).name} {name}{label} n={n} k={k} d_k={d:.3e} gpu={g:.3e} allowed={allowed:.3e} it={it}")
        # fewer than k iterations only where the recurrence's residual can vanish: the Krylov space is exhausted
        if not (it == k if k < n else 1 <= it <= k):
            errors.append(f"k={k}: {it} iterations")
        if not g <= allowed:
            errors.append(f"k={k}: deviation {g:.3e} from the long-double iterate, allowed {allowed:.3e} (d_k = {d:.3e})")
    assert not errors, f"{name}{label} {np.dtype(dtype).name}: " + "; ".join(errors)


@DTYPES
@pytest.mark.parametrize("name", MATRICES)
def test_iterates_against_the_long_double_recurrence(name, dtype):
    import torch
    import cfs_spmv_amd as cfs
    n, rp, ci, va = _matrix(name)
    va, b = scaled(n, rp, ci, va, dtype), _rhs(n, dtype)
    A = cfs.SymMatrix(n, rp, ci, va)
    assert A.stats()["n"] == n and A.row_end - A.row_begin == n
    _check_iterates(name, n, rp, ci, va, b, dtype, lambda k: _native(A, b, torch, tol=0.0, maxiter=k)[:2])
    A.close()


@DTYPES
def test_iterates_through_a_two_shard_handle(dtype):
    """an odd n through a multi-device handle (two shards, here on one device): the diagonal gathered and the
    products computed on the shards' streams, the vector kernels on the caller's"""
    import torch
    import cfs_spmv_amd as cfs
    n, rp, ci, va = _matrix("band20001")
    va, b = scaled(n, rp, ci, va, dtype), _rhs(n, dtype)
    M = cfs.SymMatrix(n, rp, ci, va, ngpus=2)
    _check_iterates("band20001", n, rp, ci, va, b, dtype, lambda k: _native(M, b, torch, tol=0.0, maxiter=k)[:2],
                    label=" (two shards)")
    M.close()


@DTYPES
def test_iterates_of_a_deterministic_handle(dtype):
    import torch
    import cfs_spmv_amd as cfs
    n, rp, ci, va = _matrix("Flan_1565@0.01")
    va, b = scaled(n, rp, ci, va, dtype), _rhs(n, dtype)
    D = cfs.SymMatrix(n, rp, ci, va, options=cfs.make_options(flags=DET))
    assert D.kernel_variant()["det"] == 1
    _check_iterates("Flan_1565@0.01", n, rp, ci, va, b, dtype, lambda k: _native(D, b, torch, tol=0.0, maxiter=k)[:2],
                    label=" (deterministic)")
    # ... and the whole solve is bit-reproducible
    ua, ita, _ = _native(D, b, torch, tol=0.0, maxiter=12)
    ub, itb, _ = _native(D, b, torch, tol=0.0, maxiter=12, check_every=5)
    assert ita == itb == 12 and np.array_equal(ua.view(np.uint8), ub.view(np.uint8))
    D.close()


def test_iterates_with_the_captured_graph(monkeypatch):
    """CFS_HIP_CG_GRAPH=1 on a non-null stream: two Jacobi iterations captured and replayed (a single chain of
    launches), plus one plain launch sequence when k is odd -- the same iterates"""
    import torch
    import cfs_spmv_amd as cfs
    dtype = np.float64
    n, rp, ci, va = _matrix("rand1023")
    va, b = scaled(n, rp, ci, va, dtype), _rhs(n, dtype)
    A = cfs.SymMatrix(n, rp, ci, va)
    monkeypatch.setenv("CFS_HIP_CG_GRAPH", "1")
    stream = torch.cuda.Stream()
    bd = torch.from_numpy(b).cuda()

    def run(k):
        u = torch.zeros_like(bd)
        torch.cuda.synchronize()
        it, _ = A.pcg(u, bd, tol=0.0, maxiter=k, stream=stream)
        torch.cuda.synchronize()
        return u.cpu().numpy(), it
    _check_iterates("rand1023", n, rp, ci, va, b, dtype, run, label=" (captured graph)", ks=(4, 5))
    A.close()


@DTYPES
def test_precond_none_is_the_plain_solver(dtype):
    """CFS_HIP_PRECOND_NONE takes cfs_hip_sym_cg's code path: on a deterministic handle the same bits"""
    import torch
    import cfs_spmv_amd as cfs
    from cfs_spmv_amd.solver import cg_native
    n, rp, ci, va = _matrix("pwtk@0.05")
    va, b = va.astype(dtype), _rhs(n, dtype)
    tol = 1e-8 if dtype == np.float64 else 1e-4
    D = cfs.SymMatrix(n, rp, ci, va, options=cfs.make_options(flags=DET))
    bd = torch.from_numpy(b).cuda()
    for kw in (dict(tol=0.0, maxiter=7), dict(tol=tol, maxiter=500), dict(tol=tol, maxiter=500, check_every=3)):
        u1, it1, res1 = cg_native(D, bd, **kw)
        u2, it2, res2 = _native(D, b, torch, precond="none", **kw)
        torch.cuda.synchronize()
        assert it1 == it2 > 0 and res1 == res2 and np.array_equal(u1.cpu().numpy().view(np.uint8), u2.view(np.uint8)), kw
    u3 = torch.zeros_like(bd)
    assert D.pcg(u3, bd, precond=0, tol=0.0, maxiter=7)[0] == 7  # the C constant as well as the name
    D.close()


@DTYPES
def test_what_the_preconditioner_is_for(dtype):
    """rows of very different scale: plain CG needs more than ten times the iterations of Jacobi.  Both
    counts are first established on the CPU with the working-precision recurrences (checked when the test was
    written: 3 644 against 24 in fp64, 1 939 against 14 in fp32; the MI355X then took 24 and 14); the GPU must then reproduce Jacobi's count
    J within +-2 (room for the last iterations' rounding at the threshold) while cfs_hip_sym_cg is still
    unconverged after 10 J iterations."""
    import torch
    import cfs_spmv_amd as cfs
    from cfs_spmv_amd.solver import cg_native
    n, rp, ci, va = _matrix("band20001")
    va = scaled(n, rp, ci, va, dtype)
    b = np.random.default_rng(SCALE_SEED + 1).uniform(-1, 1, n).astype(dtype)
    tol = 1e-8 if dtype == np.float64 else 1e-4
    J = pcg_reference(n, rp, ci, va, b, dtype=dtype, tol=tol, maxiter=2000)["count"]
    plain = plain_count(n, rp, ci, va, b, dtype, tol, 10 * J + 1)
    print(f"pcg-steps {np.dtype(dtype).name} band20001 scaled: Jacobi {J} iterations, plain CG more than {plain - 1} (CPU)")
    assert 5 <= J < 200 and plain > 10 * J, f"badly chosen case: plain CG {plain} iterations, Jacobi {J}"
    A = cfs.SymMatrix(n, rp, ci, va)
    u, it, res = _native(A, b, torch, tol=tol, maxiter=2000)
    true, slack = _true_relres(n, rp, ci, va, b, u, dtype)
    print(f"pcg-steps {np.dtype(dtype).name} band20001 scaled: GPU Jacobi {it} iterations, relres {res:.3e} (long double {true:.3e})")
    assert res <= 10 * tol and true <= 10 * tol + slack
    assert J - 2 <= it <= J + 2, (J, it)
    up, itp, resp = cg_native(A, torch.from_numpy(b).cuda(), tol=tol, maxiter=10 * J)
    torch.cuda.synchronize()
    print(f"pcg-steps {np.dtype(dtype).name} band20001 scaled: GPU plain CG relres {resp:.3e} after {itp} iterations")
    assert itp == 10 * J and resp > tol
    A.close()


@DTYPES
def test_iteration_count_and_reported_residual(dtype):
    import torch
    import cfs_spmv_amd as cfs
    n, rp, ci, va = _matrix("pwtk@0.05")
    va, b = scaled(n, rp, ci, va, dtype), _rhs(n, dtype)
    A = cfs.SymMatrix(n, rp, ci, va)
    # tol = 0: exactly maxiter iterations, whatever the window of enqueued iterations
    for check_every, k in ((1, 7), (3, 23), (16, 23), (1000, 23), (16, 40)):
        u, it, res = _native(A, b, torch, tol=0.0, maxiter=k, check_every=check_every)
        assert it == k, (check_every, k, it)
        true, slack = _true_relres(n, rp, ci, va, b, u, dtype)
        print(f"pcg-steps {np.dtype(dtype).name} relres k={k} reported={res:.6e} long double={true:.6e} slack={slack:.3e}")
        assert abs(res - true) <= slack, (k, res, true, slack)
    # maxiter = 0: u untouched, the residual of the first guess
    x0 = np.random.default_rng(4).uniform(-1, 1, n).astype(dtype)
    u, it, res = _native(A, b, torch, tol=0.0, maxiter=0, x0=torch.from_numpy(x0).cuda())
    true, slack = _true_relres(n, rp, ci, va, b, x0, dtype)
    assert it == 0 and np.array_equal(u.view(np.uint8), x0.view(np.uint8)) and abs(res - true) <= slack
    # b = 0 (and u = 0): nothing to do
    u, it, res = _native(A, np.zeros(n, dtype), torch, tol=1e-8, maxiter=50)
    assert it == 0 and not u.any() and np.isfinite(res)
    # a first guess that already solves the system: at most one iteration
    tol = 1e-10 if dtype == np.float64 else 1e-5
    us, its, ress = _native(A, b, torch, tol=tol, maxiter=500)
    assert 0 < its < 500 and ress <= 10 * tol
    u, it, res = _native(A, b, torch, tol=10 * tol, maxiter=500, x0=torch.from_numpy(us).cuda())
    assert it <= 1 and res <= 100 * tol
    A.close()


@DTYPES
def test_convergence_inside_a_window_of_enqueued_iterations(dtype):
    """the iterations enqueued behind the converged one change neither u nor the count"""
    import torch
    import cfs_spmv_amd as cfs
    n, rp, ci, va = _matrix("pwtk@0.05")
    va, b = scaled(n, rp, ci, va, dtype), _rhs(n, dtype)
    tol = 1e-8 if dtype == np.float64 else 1e-4
    D = cfs.SymMatrix(n, rp, ci, va, options=cfs.make_options(flags=DET))
    u1, it1, res1 = _native(D, b, torch, tol=tol, maxiter=500, check_every=1)
    assert 4 < it1 < 500 and res1 <= 10 * tol
    windows = [c for c in (3, 5, 7, 16) if it1 % c]  # the converged iteration is not the last of its window
    assert len(windows) >= 2, it1
    for check_every in windows:
        u2, it2, _ = _native(D, b, torch, tol=tol, maxiter=500, check_every=check_every)
        assert it2 == it1 and np.array_equal(u2.view(np.uint8), u1.view(np.uint8)), (check_every, it1, it2)
    D.close()


@DTYPES
def test_nan_in_b_ends_the_solve_at_once(dtype):
    import torch
    import cfs_spmv_amd as cfs
    n, rp, ci, va = _matrix("rand1023")
    va, b = scaled(n, rp, ci, va, dtype), _rhs(n, dtype)
    b[n // 2] = np.nan
    A = cfs.SymMatrix(n, rp, ci, va)
    for check_every in (1, 16):
        u, it, res = _native(A, b, torch, tol=1e-8, maxiter=300, check_every=check_every)
        assert it <= 1 and np.isnan(res), (it, res)
    A.close()


@DTYPES
@pytest.mark.parametrize("bad", [0.0, -1.5, np.nan, "missing"], ids=["zero", "negative", "nan", "not-stored"])
def test_a_diagonal_that_is_not_positive_is_refused(bad, dtype):
    """CFS_HIP_ERR_ARG, u untouched, no iteration -- and the plain solver still takes the matrix"""
    import torch
    import cfs_spmv_amd as cfs
    from cfs_spmv_amd import _lib
    n, rp, ci, va = _matrix("rand1023")
    va = scaled(n, rp, ci, va, dtype)
    rows = np.repeat(np.arange(n), np.diff(rp))
    k = int(np.flatnonzero((rows == ci) & (rows == 700))[0])
    if bad == "missing":
        keep = np.arange(va.size) != k
        rp = np.concatenate([[0], np.cumsum(np.bincount(rows[keep], minlength=n))]).astype(np.int32)
        ci, va = ci[keep], va[keep]
    else:
        va[k] = bad
    A = cfs.SymMatrix(n, rp, ci, va)
    x0 = np.random.default_rng(5).uniform(-1, 1, n).astype(dtype)
    u = torch.from_numpy(x0).cuda()
    b = torch.from_numpy(_rhs(n, dtype)).cuda()
    for check_every in (1, 8):
        with pytest.raises(_lib.CfsHipError, match="positive diagonal") as e:
            A.pcg(u, b, tol=1e-8, maxiter=50, check_every=check_every)
        assert e.value.code == _lib.ERR_ARG
        torch.cuda.synchronize()
        assert np.array_equal(u.cpu().numpy().view(np.uint8), x0.view(np.uint8))
    # through the raw ABI: *iterations = 0
    import ctypes as C
    it, res = C.c_int(9), C.c_double(9.0)
    rc = _lib.load().cfs_hip_sym_pcg(A._h, u.data_ptr(), b.data_ptr(), _lib.PRECOND_JACOBI, 1e-8, 50, 8, C.byref(it),
                                     C.byref(res), torch.cuda.current_stream().cuda_stream)
    assert rc == _lib.ERR_ARG and it.value == 0
    it2, _ = A.pcg(u, b, precond="none", tol=0.0, maxiter=2)
    assert it2 == (0 if isinstance(bad, float) and np.isnan(bad) else 2)  # (a NaN residual ends the plain solve at once)
    A.close()


@DTYPES
def test_argument_checks(dtype):
    import torch
    import cfs_spmv_amd as cfs
    from cfs_spmv_amd import _lib
    n, rp, ci, va = _matrix("rand1023")
    va = va.astype(dtype)
    A = cfs.SymMatrix(n, rp, ci, va)
    big = torch.zeros(n + 4, dtype=torch.from_numpy(va).dtype, device="cuda")
    good = torch.zeros(n, dtype=big.dtype, device="cuda")
    assert good.data_ptr() % 16 == 0 and big[1:n + 1].data_ptr() % 16 != 0
    for u, b in ((big[1:n + 1], good), (good, big[1:n + 1])):
        with pytest.raises(_lib.CfsHipError) as e:
            A.pcg(u, b, tol=1e-8, maxiter=5)
        assert e.value.code == _lib.ERR_ARG
    with pytest.raises(_lib.CfsHipError, match="unknown preconditioner") as e:
        A.pcg(good, good.clone(), precond=2, tol=1e-8, maxiter=5)
    assert e.value.code == _lib.ERR_ARG
    with pytest.raises(ValueError):
        A.pcg(good, good.clone(), precond="ilu")
    with pytest.raises(_lib.CfsHipError) as e:  # one vector for both
        A.pcg(good, good, tol=1e-8, maxiter=5)
    assert e.value.code == _lib.ERR_ARG
    host = np.zeros(n, dtype)
    with pytest.raises(_lib.CfsHipError) as e:  # a host pointer
        A.pcg(host, good, tol=1e-8, maxiter=5)
    assert e.value.code == _lib.ERR_ARG
    A.close()
    S = cfs.SymMatrix(n, rp, ci, va, row_splits=np.array([0, n // 2, n], np.int32), rank=1)
    for precond in ("jacobi", "none"):
        with pytest.raises(_lib.CfsHipError) as e:
            S.pcg(good, good.clone(), precond=precond, tol=1e-8, maxiter=5)
        assert e.value.code == _lib.ERR_UNSUPPORTED
    S.close()


@DTYPES
def test_host_driven_and_native_loops_agree(dtype):
    """solver.pcg (torch-driven, the diagonal from A.diagonal()) against solver.pcg_native on the pwtk stand-in:
    iteration counts within +-2, both answers within the bound test_gpu_parity.py holds the plain solvers to
    against a direct solve at these tolerances (the stand-in's conditioning: a factor 100 over the tolerance)"""
    import scipy.sparse as sp
    import scipy.sparse.linalg as spl
    import torch
    import cfs_spmv_amd as cfs
    from cfs_spmv_amd import synth
    from cfs_spmv_amd.solver import pcg, pcg_native
    n, rp, ci, va = _matrix("pwtk@0.05")
    va = va.astype(dtype)
    A = cfs.SymMatrix(n, rp, ci, va)
    b = synth.make_x(n, 11, dtype)
    bd = torch.from_numpy(b).cuda()
    tol, lim = (1e-11, 1e-9) if dtype == np.float64 else (2e-5, 2e-3)
    u1, it1, res1 = pcg(A, bd, tol=tol, maxiter=500)
    torch.cuda.synchronize()
    u_ref = spl.spsolve(sp.csc_matrix(sp.csr_matrix((va.astype(np.float64), ci, rp), shape=(n, n))), b.astype(np.float64))
    assert 0 < it1 < 500 and res1 <= 10 * tol
    assert np.max(np.abs(u1.cpu().numpy() - u_ref)) <= lim * np.max(np.abs(u_ref))
    for check_every in (1, 8, 1000):
        u2, it2, res2 = pcg_native(A, bd, tol=tol, maxiter=500, check_every=check_every)
        torch.cuda.synchronize()
        print(f"pcg-steps {np.dtype(dtype).name} pwtk@0.05: host-driven {it1} iterations, native {it2} (check_every={check_every})")
        assert 0 < it2 < 500 and abs(it2 - it1) <= 2, (it1, it2, check_every)
        assert res2 <= 10 * tol, (res1, res2)
        assert np.max(np.abs(u2.cpu().numpy() - u_ref)) <= lim * np.max(np.abs(u_ref))
        assert np.max(np.abs(u2.cpu().numpy() - u1.cpu().numpy())) <= 2 * lim * np.max(np.abs(u_ref))
    A.close()
