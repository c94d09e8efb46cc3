"""cfs_hip_sym_pcg_mixed: one CG recurrence in fp32 (the launches of cfs_hip_sym_pcg / _pcg_block on an fp32
handle, accumulating a correction xlo), the solution u and the true residuals in fp64 on an fp64 handle of
the same matrix; from time to time the true residual replaces the recurrence's, the search direction kept
(cfs_spmv_amd/csrc/cfs_solver_mixed.hpp).

The CPU side, mixed_reference(), restates the solver with its rounding rules and its host looks, and nothing
of the library: r, p, q, xlo in fp32, the product of the fp32-rounded matrix in fp32, dots and z = M^-1 r (from
the ROUNDED r and the fp32 preconditioner) in fp64, a look every min(check_every, 16) iterations, a
replacement when the recurrence's r.r is not > max(tol^2 b.b, delta^2 rr_ref) at any iteration of the window
(the device flag: the iterations behind it do nothing), rr_ref the largest r.r seen at a look since the last
replacement (the true r.r of that replacement included).

1. Iterates.  u_k after exactly k iterations (tol = 0, check_every = 1, delta = 1e-150: no replacement before
k, the closing fold applied) against the long-double Jacobi recurrence (test_gpu_pcg_steps.pcg_reference) on
the matrix ROUNDED TO fp32 (both handles hold it), b in fp64.  d_k = the deviation of mixed_reference from the
long-double run; the GPU is allowed 4 d_k + 16 * 2^-24; d_k > D_LIMIT[float32] = 1e-2 is a badly chosen case.

Measured on the MI355X (matrix, then for k = 1, 2, 3, 5, 10: d_k / the GPU's deviation):

  rand1       1.0e-08/1.0e-08  1.0e-08/1.0e-08  0.0e+00/0.0e+00  0.0e+00/0.0e+00  0.0e+00/0.0e+00
  rand2       3.3e-08/3.3e-08  7.2e-08/7.2e-08  7.2e-08/7.2e-08  7.2e-08/7.2e-08  7.2e-08/7.2e-08
  rand3       5.8e-08/5.8e-08  7.4e-08/7.4e-08  9.0e-08/9.0e-08  9.0e-08/9.0e-08  9.0e-08/9.0e-08
  rand63      3.7e-08/3.7e-08  5.3e-08/4.1e-08  2.8e-08/4.0e-08  7.7e-08/7.7e-08  7.0e-08/7.0e-08
  rand64      1.5e-08/1.5e-08  3.4e-08/3.4e-08  4.5e-08/4.5e-08  5.7e-08/5.7e-08  7.2e-08/7.2e-08
  rand65      2.9e-08/4.1e-08  1.0e-07/1.0e-07  1.4e-07/1.4e-07  1.5e-07/1.5e-07  1.6e-07/1.6e-07
  rand257     7.2e-08/7.2e-08  6.2e-08/9.4e-08  8.9e-08/9.4e-08  1.2e-07/1.2e-07  1.5e-07/1.5e-07
  rand1023    3.8e-08/4.4e-08  4.7e-08/4.7e-08  5.9e-08/5.9e-08  6.6e-08/6.6e-08  9.5e-08/9.5e-08
  rand1026    4.9e-08/4.9e-08  9.7e-08/9.7e-08  9.4e-08/9.4e-08  8.9e-08/8.9e-08  1.5e-07/1.5e-07
  band20001   9.6e-08/9.6e-08  1.5e-07/8.5e-08  1.6e-07/1.2e-07  1.8e-07/1.4e-07  2.3e-07/2.3e-07
  pwtk@0.05   8.2e-08/8.2e-08  2.0e-07/8.8e-08  1.4e-07/8.9e-08  1.8e-07/1.1e-07  1.7e-07/1.3e-07

2. What it is for: band20001 scaled, in fp64 (its fp32 handle holds the rounded values), tol = 1e-11,
delta = 0.1, check_every = 8.

  CPU: fp64 Jacobi 31 iterations; fp32 alone stalls at 2.812e-06 after 93; mixed 31 iterations, 10 replacements,
       relres 6.136e-12
  MI355X: mixed 31 iterations, 10 replacements, relres 6.136e-12 (long double 6.136e-12); cfs_hip_sym_pcg in fp32
       alone relres 2.647e-06 after 93 iterations (long double, against the fp64 matrix: 2.661e-06)

3. Block Jacobi on rotated 3 x 3 node blocks (test_gpu_block_pcg_steps.rotated_node_blocks, n = 20 001),
tol = 1e-10.  The residual falls 5 x per iteration here: with the replacement rule evaluated only at the host
looks (every 8 iterations) the CPU recurrence DIVERGES on this case (the fp32 recurrence runs 4e5 below the last
true residual before it is replaced), which is why the rule is evaluated on the device at every iteration.

  CPU: mixed 17 iterations, 8 replacements, relres 3.125e-11
  MI355X: mixed 17 iterations, 8 replacements, relres 3.125e-11 (long double 3.125e-11)

4. pwtk@0.05 scaled, deterministic handles, tol = 1e-10: 65 iterations, 10 replacements, relres 6.088e-11, twice;
host-driven (solver.pcg_mixed) and native: 65 / 10 both, block Jacobi 65 / 10 both, no preconditioner (unscaled)
62 / 10 both.
"""
import ctypes as C

import numpy as np
import pytest

from test_gpu_cg_steps import D_LIMIT, DET, KS, _deviation, _matrix, _rhs, _true_relres
from test_gpu_kernel_variants import PLAN_KNOBS
from test_gpu_pcg_steps import SCALE_SEED, pcg_reference, scaled
from test_gpu_block_pcg_steps import cholesky_inverse, node_blocks, rotated_node_blocks

pytestmark = pytest.mark.gpu

F32, F64 = np.float32, np.float64
UNIT32 = 2.0 ** -24
NO_REPLACEMENT = 1e-150  # delta: r.r would have to fall 300 decades below its reference
CASES = ["rand1", "rand2", "rand3", "rand63", "rand64", "rand65", "rand257", "rand1023", "rand1026", "band20001", "pwtk@0.05"]


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
def jacobi_apply(n, rp, ci, va32):
    """z = dinv r in fp64, dinv_i = (float)(1.0 / (double)a_ii) of the fp32 matrix"""
    import scipy.sparse as sp
    d = sp.csr_matrix((va32, ci, rp), shape=(n, n)).diagonal().astype(F32)
    dinv = (1.0 / d.astype(F64)).astype(F32).astype(F64)
    return lambda r: r * dinv


def block_apply(n, rp, ci, va32, bs, minv=None):
    """z = Minv r over the node blocks in fp64, Minv the fp64 Cholesky inverse of the fp32 blocks rounded to fp32
    (ascending j, as the kernels); minv: (nb, bs, bs) fp32 inverse blocks to use instead, converted exactly"""
    M = (cholesky_inverse(node_blocks(n, rp, ci, va32, bs), F64) if minv is None else minv).astype(F32).astype(F64)
    nb = M.shape[0]

    def apply(r):
        rp_ = np.zeros(nb * bs, F64)
        rp_[:n] = r
        rb, z = rp_.reshape(nb, bs), np.zeros((nb, bs), F64)
        for j in range(bs):
            z += M[:, :, j] * rb[:, j:j + 1]
        return z.reshape(-1)[:n]
    return apply


def mixed_reference(n, rp, ci, va64, b, apply, tol, delta, maxiter, check_every, x0=None, plain=False, margins=None):
    """(u, iterations, replacements, fp64 relative residual) of the solver's recurrence, see the module docstring.
    plain: no preconditioner, by the rule of the plain kernels -- p = r, and alpha and beta from r.r of the UNROUNDED
    residual (apply is not called).  margins: a list that receives |x - y| / max(|x|, |y|) of every comparison
    r.r > thr (one per iteration) and r.r >= delta^2 rr_ref (one per look) that steers the recurrence"""
    import scipy.sparse as sp
    A64 = sp.csr_matrix((va64, ci, rp), shape=(n, n))
    A32 = sp.csr_matrix((va64.astype(F32), ci, rp), shape=(n, n))
    check_every = min(check_every, 16)
    u = np.zeros(n, F64) if x0 is None else x0.astype(F64).copy()
    xlo = np.zeros(n, F32)

    def replace():
        d = b - A64 @ u
        r = d.astype(F32)
        z = r.astype(F64) if plain else apply(r.astype(F64))
        return r, z, np.dot(d, d) if plain else np.dot(r.astype(F64), z), np.dot(d, d)

    def apart(x, y):
        if margins is not None:
            margins.append(abs(x - y) / max(abs(x), abs(y)) if max(abs(x), abs(y)) > 0 else 0.0)
    r, z, rz, rr = replace()
    p = z.astype(F32)
    bb = np.dot(b, b)
    stop, drop = tol * tol * bb, delta * delta
    it, nrep, rr_ref, folded, done = 0, 0, rr, True, not (rr > stop)
    while not done and it < maxiter:
        until, flag, thr = min(maxiter, it + check_every), False, max(stop, drop * rr_ref)
        while it < until and not flag:
            q = (A32 @ p).astype(F32)
            pq = np.dot(p.astype(F64), q.astype(F64))
            alpha = rz / pq if pq != 0 else 0.0
            xlo = (xlo.astype(F64) + alpha * p.astype(F64)).astype(F32)
            rs = r.astype(F64) - alpha * q.astype(F64)
            rr = np.dot(rs, rs)
            r = rs.astype(F32)
            z = r.astype(F64) if plain else apply(r.astype(F64))
            rzn = rr if plain else np.dot(r.astype(F64), z)
            p = (z + (rzn / rz if rz != 0 else 0.0) * p.astype(F64)).astype(F32)
            rz, it, folded, flag = rzn, it + 1, False, not (rr > thr)
            apart(rr, thr)
        rr_ref = max(rr_ref, rr)
        apart(rr, drop * rr_ref)
        if flag or not (rr >= drop * rr_ref):
            u, xlo = u + xlo.astype(F64), np.zeros(n, F32)
            r, z, rz, rr = replace()
            nrep, folded, rr_ref, done = nrep + 1, True, rr, not (rr > stop)
    if not folded:
        u = u + xlo.astype(F64)
        rr = replace()[3]
    return u, it, nrep, float(np.sqrt(rr / bb)) if bb > 0 else float(np.sqrt(rr))


def fp32_stall(n, rp, ci, va64, b, iters):
    """the fp64 relative residual of what Jacobi PCG in fp32 alone returns after `iters` iterations (tol = 0)"""
    import scipy.sparse as sp
    u = pcg_reference(n, rp, ci, va64.astype(F32), b.astype(F32), dtype=F32, tol=0.0, maxiter=iters)["u"]
    d = b - sp.csr_matrix((va64, ci, rp), shape=(n, n)) @ u.astype(F64)
    return float(np.sqrt(np.dot(d, d) / np.dot(b, b)))


def _native(M, b, torch, x0=None, **kw):
    from cfs_spmv_amd.solver import pcg_mixed_native
    x0 = None if x0 is None else torch.from_numpy(x0).cuda()
    u, it, rep, res = pcg_mixed_native(M, torch.from_numpy(b).cuda(), x0=x0, **kw)
    torch.cuda.synchronize()
    return u.cpu().numpy(), it, rep, res


def _det_options():
    import cfs_spmv_amd as cfs
    return cfs.make_options(flags=DET)


# ---- 1. iterates ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", CASES)
def test_iterates_against_the_long_double_recurrence(name):
    import torch
    import cfs_spmv_amd as cfs
    n, rp, ci, va = _matrix(name)
    va32 = scaled(n, rp, ci, va, F32)
    va64, b = va32.astype(F64), _rhs(n, F64)
    ref = pcg_reference(n, rp, ci, va32, b, KS)
    apply = jacobi_apply(n, rp, ci, va32)
    M = cfs.MixedSym(n, rp, ci, va64)
    errors = []
    for k in KS:
        u_ref = ref[k][0]
        u_work = mixed_reference(n, rp, ci, va64, b, apply, 0.0, NO_REPLACEMENT, k, 1)[0]
        d = _deviation(u_work, u_ref)
        assert d <= D_LIMIT[F32], f"{name}: d_{k} = {d:.3e}: badly conditioned case"
        u, it, rep, _ = _native(M, b, torch, tol=0.0, delta=NO_REPLACEMENT, maxiter=k, check_every=1)
        g = _deviation(u, u_ref)
        allowed = 4 * d + 16 * UNIT32
        print(f"mixed-steps {name} n={n} k={k} d_k={d:.3e} gpu={g:.3e} allowed={allowed:.3e} it={it} rep={rep}")
        # fewer than k iterations only where the recurrence's residual can vanish: the Krylov space is exhausted
        if not (it == k if k < n else 1 <= it <= k):
            errors.append(f"k={k}: {it} iterations")
        if k < n and rep != 0:
            errors.append(f"k={k}: {rep} replacements before k")
        if not g <= allowed:
            errors.append(f"k={k}: deviation {g:.3e} from the long-double iterate, allowed {allowed:.3e} (d_k = {d:.3e})")
    M.close()
    assert not errors, f"{name}: " + "; ".join(errors)


# ---- 2. what it is for --------------------------------------------------------------------------------------
def test_what_the_mixed_solver_is_for():
    """an fp64 answer from fp32 products, in about the iterations of the fp64 solver, where fp32 alone stalls"""
    import torch
    import cfs_spmv_amd as cfs
    from cfs_spmv_amd.solver import pcg_native
    tol, delta, check_every = 1e-11, 0.1, 8
    n, rp, ci, va = _matrix("band20001")
    va = scaled(n, rp, ci, va, F64)
    b = np.random.default_rng(SCALE_SEED + 1).uniform(-1, 1, n)
    J64 = pcg_reference(n, rp, ci, va, b, dtype=F64, tol=tol, maxiter=2000)["count"]
    m32 = fp32_stall(n, rp, ci, va, b, 3 * J64)
    _, Jm, R, resm = mixed_reference(n, rp, ci, va, b, jacobi_apply(n, rp, ci, va.astype(F32)), tol, delta, 2000, check_every)
    print(f"mixed-steps band20001 scaled (CPU): fp64 Jacobi {J64} iterations; fp32 alone stalls at {m32:.3e} after {3 * J64}; "
          f"mixed {Jm} iterations, {R} replacements, relres {resm:.3e}")
    assert m32 > 1e-8 and resm <= tol and R >= 2 and Jm <= 1.5 * J64 + 16, \
        f"badly chosen case: J64 {J64}, m32 {m32:.3e}, mixed {Jm} iterations / {R} replacements / relres {resm:.3e}"
    M = cfs.MixedSym(n, rp, ci, va)
    u, it, rep, res = _native(M, b, torch, tol=tol, delta=delta, maxiter=2000, check_every=check_every)
    true, slack = _true_relres(n, rp, ci, va, b, u, F64)
    print(f"mixed-steps band20001 scaled (GPU): mixed {it} iterations, {rep} replacements, relres {res:.3e} (long double {true:.3e})")
    assert res <= 10 * tol and true <= 10 * tol + slack
    assert abs(it - Jm) <= check_every + 2, (Jm, it)
    assert abs(rep - R) <= 1, (R, rep)
    u32, it32, res32 = pcg_native(M.A32, torch.from_numpy(b.astype(F32)).cuda(), tol=0.0, maxiter=3 * J64)
    torch.cuda.synchronize()
    print(f"mixed-steps band20001 scaled (GPU): cfs_hip_sym_pcg in fp32 alone relres {res32:.3e} after {it32} iterations")
    true32 = _true_relres(n, rp, ci, va, b, u32.cpu().numpy().astype(F64), F64)[0]  # (not what that solver reports)
    print(f"mixed-steps band20001 scaled (GPU): ... its long-double residual against the fp64 matrix {true32:.3e}")
    assert it32 == 3 * J64 and res32 > 1e-8 and true32 > 1e-8
    M.close()


# ---- 3. block Jacobi ----------------------------------------------------------------------------------------
def test_block_jacobi_on_rotated_node_blocks():
    """block_rows = 3 reaches 1e-10 in the iterations and replacements of the CPU recurrence (the band of test 2);
    block_rows = 1 is the Jacobi path, bit for bit"""
    import torch
    import cfs_spmv_amd as cfs
    tol, delta, check_every = 1e-10, 0.1, 8
    n, rp, ci, va, b = rotated_node_blocks(3)
    _, Bm, R, resm = mixed_reference(n, rp, ci, va, b, block_apply(n, rp, ci, va.astype(F32), 3), tol, delta, 500, check_every)
    print(f"mixed-steps rotated blocks bs=3 (CPU): mixed {Bm} iterations, {R} replacements, relres {resm:.3e}")
    assert resm <= tol and 1 <= R and 5 <= Bm < 500, f"badly chosen case: {Bm} iterations, {R} replacements, relres {resm:.3e}"
    M = cfs.MixedSym(n, rp, ci, va, options=_det_options())
    u, it, rep, res = _native(M, b, torch, precond="block_jacobi", block=3, tol=tol, delta=delta, maxiter=500,
                              check_every=check_every)
    true, slack = _true_relres(n, rp, ci, va, b, u, F64)
    print(f"mixed-steps rotated blocks bs=3 (GPU): mixed {it} iterations, {rep} replacements, relres {res:.3e} (long double {true:.3e})")
    assert res <= 10 * tol and true <= 10 * tol + slack
    assert abs(it - Bm) <= check_every + 2 and abs(rep - R) <= 1, (Bm, it, R, rep)
    for kw in (dict(tol=0.0, maxiter=7), dict(tol=1e-9, maxiter=40, check_every=3)):
        u1, it1, rep1, res1 = _native(M, b, torch, precond="jacobi", **kw)
        u2, it2, rep2, res2 = _native(M, b, torch, precond="block_jacobi", block=1, **kw)
        assert it1 == it2 > 0 and rep1 == rep2 and res1 == res2 and np.array_equal(u1.view(np.uint8), u2.view(np.uint8)), kw
    M.close()


# ---- 4. determinism and windows -------------------------------------------------------------------------------
def test_deterministic_handles_and_windows():
    import torch
    import cfs_spmv_amd as cfs
    n, rp, ci, va = _matrix("pwtk@0.05")
    va, b = scaled(n, rp, ci, va, F64), _rhs(n, F64)
    A64 = cfs.SymMatrix(n, rp, ci, va, options=_det_options())
    A32 = cfs.SymMatrix(n, rp, ci, va.astype(F32), options=_det_options())
    assert A64.kernel_variant()["det"] == 1 and A32.kernel_variant()["det"] == 1
    M = cfs.MixedSym.from_handles(A64, A32)
    # two solves: identical bytes and counts
    ua, ita, repa, resa = _native(M, b, torch, tol=1e-10, maxiter=500)
    ub, itb, repb, resb = _native(M, b, torch, tol=1e-10, maxiter=500)
    print(f"mixed-steps pwtk@0.05 scaled (deterministic): {ita} iterations, {repa} replacements, relres {resa:.3e}")
    assert 0 < ita < 500 and repa >= 1 and resa <= 1e-9
    assert (ita, repa, resa) == (itb, repb, resb) and np.array_equal(ua.view(np.uint8), ub.view(np.uint8))
    # tol = 0: exactly maxiter iterations, whatever the window of enqueued iterations
    for check_every in (1, 3, 16, 1000):
        u, it, rep, res = _native(M, b, torch, tol=0.0, maxiter=23, check_every=check_every)
        true, slack = _true_relres(n, rp, ci, va, b, u, F64)
        print(f"mixed-steps relres check_every={check_every} it={it} rep={rep} reported={res:.6e} long double={true:.6e}")
        assert it == 23 and abs(res - true) <= slack, (check_every, it, res, true, slack)
    # the iterations enqueued behind a converged one change nothing.  Without replacements by the drop rule the
    # looks do not steer the recurrence: a replacement comes only from the device flag, at the iteration that
    # raised it, wherever the window ends -- the same u, the same counts for every window
    kw = dict(tol=1e-5, delta=NO_REPLACEMENT, maxiter=500)
    u1, it1, rep1, res1 = _native(M, b, torch, check_every=1, **kw)
    assert 4 < it1 < 500 and rep1 >= 1 and res1 <= 1e-4
    windows = [c for c in (3, 5, 7, 16) if it1 % c]
    assert len(windows) >= 2, it1
    for check_every in windows:
        u2, it2, rep2, res2 = _native(M, b, torch, check_every=check_every, **kw)
        assert (it2, rep2, res2) == (it1, rep1, res1) and np.array_equal(u2.view(np.uint8), u1.view(np.uint8)), check_every
    M.close()  # (wraps the caller's handles: they stay open)
    assert A64.stats()["n"] == n
    A64.close()
    A32.close()


# ---- 5. edges -------------------------------------------------------------------------------------------------
def test_edges_of_the_iteration():
    import torch
    import cfs_spmv_amd as cfs
    n, rp, ci, va = _matrix("rand1023")
    va, b = scaled(n, rp, ci, va, F64), _rhs(n, F64)
    M = cfs.MixedSym(n, rp, ci, va)
    # maxiter = 0: u untouched, the residual of the first guess
    x0 = np.random.default_rng(4).uniform(-1, 1, n)
    u, it, rep, res = _native(M, b, torch, x0=x0, tol=0.0, maxiter=0)
    true, slack = _true_relres(n, rp, ci, va, b, x0, F64)
    assert it == 0 and rep == 0 and np.array_equal(u.view(np.uint8), x0.view(np.uint8)) and abs(res - true) <= slack
    # b = 0 (and u = 0): nothing to do
    u, it, rep, res = _native(M, np.zeros(n), torch, tol=1e-8, maxiter=50)
    assert it == 0 and rep == 0 and not u.any() and res == 0.0
    # a first guess that already solves the system
    us, its, reps, ress = _native(M, b, torch, tol=1e-12, maxiter=500)
    assert 0 < its < 500 and ress <= 1e-11
    u, it, rep, res = _native(M, b, torch, x0=us, tol=1e-10, maxiter=500)
    assert it == 0 and rep in (0, 1) and res <= 1e-10 and np.array_equal(u.view(np.uint8), us.view(np.uint8))
    # NaN in b: ends at once
    bn = b.copy()
    bn[n // 2] = np.nan
    for check_every in (1, 16):
        u, it, rep, res = _native(M, bn, torch, tol=1e-8, maxiter=300, check_every=check_every)
        assert it <= 1 and rep <= 1 and np.isnan(res), (it, rep, res)
    M.close()


@pytest.mark.parametrize("bad", [0.0, -1.5], ids=["zero", "negative"])
def test_a_diagonal_that_is_not_positive_is_refused(bad):
    import torch
    import cfs_spmv_amd as cfs
    from cfs_spmv_amd import _lib
    n, rp, ci, va = _matrix("rand1023")
    va = scaled(n, rp, ci, va, F64)
    rows = np.repeat(np.arange(n), np.diff(rp))
    va[int(np.flatnonzero((rows == ci) & (rows == 700))[0])] = bad
    M = cfs.MixedSym(n, rp, ci, va)
    x0 = np.random.default_rng(5).uniform(-1, 1, n)
    u, b = torch.from_numpy(x0).cuda(), torch.from_numpy(_rhs(n, F64)).cuda()
    for kw, what in ((dict(precond="jacobi"), "positive diagonal"), (dict(precond="block_jacobi", block=3), "positive definite")):
        with pytest.raises(_lib.CfsHipError, match=what) as e:
            M.pcg(u, b, tol=1e-8, maxiter=50, **kw)
        assert e.value.code == _lib.ERR_ARG
        torch.cuda.synchronize()
        assert np.array_equal(u.cpu().numpy().view(np.uint8), x0.view(np.uint8))
    it, rep, res = C.c_int(9), C.c_int(9), C.c_double(9.0)  # through the raw ABI: the counts are zeroed
    rc = _lib.load().cfs_hip_sym_pcg_mixed(M.A64._h, M.A32._h, u.data_ptr(), b.data_ptr(), 1, 1e-8, 0.1, 50, 8, C.byref(it),
                                           C.byref(rep), C.byref(res), torch.cuda.current_stream().cuda_stream)
    assert rc == _lib.ERR_ARG and it.value == 0 and rep.value == 0
    assert M.pcg(u, b, precond="none", tol=0.0, maxiter=2)[0] == 2  # the plain recurrence still takes the matrix
    M.close()


def test_argument_checks():
    import torch
    import cfs_spmv_amd as cfs
    from cfs_spmv_amd import _lib
    lib = _lib.load()
    n, rp, ci, va = _matrix("rand1023")
    M = cfs.MixedSym(n, rp, ci, va.astype(F64))
    big = torch.zeros(n + 4, dtype=torch.float64, device="cuda")
    good, other = torch.zeros(n, dtype=torch.float64, device="cuda"), torch.zeros(n, dtype=torch.float64, device="cuda")
    bad = big[1:n + 1]
    assert good.data_ptr() % 16 == 0 and bad.data_ptr() % 16 != 0
    host = np.zeros(n)
    st = torch.cuda.current_stream().cuda_stream

    def raw(h64, h32, u, b, block_rows=1, tol=1e-8, delta=0.1, maxiter=5):
        it, rep, res = C.c_int(9), C.c_int(9), C.c_double(9.0)
        rc = lib.cfs_hip_sym_pcg_mixed(h64, h32, u, b, block_rows, tol, delta, maxiter, 8, C.byref(it), C.byref(rep),
                                       C.byref(res), st)
        return rc
    h64, h32, pu, pb = M.A64._h, M.A32._h, good.data_ptr(), other.data_ptr()
    assert raw(h64, h32, pu, pb) == 0
    for args in ((None, h32, pu, pb), (h64, None, pu, pb), (h64, h32, None, pb), (h64, h32, pu, None)):  # null pointers
        assert raw(*args) == _lib.ERR_ARG and b"null" in lib.cfs_hip_last_error(), args
    assert raw(h64, h32, pu, pu) == _lib.ERR_ARG  # one vector for both
    for u, b in ((bad.data_ptr(), pb), (pu, bad.data_ptr())):  # misaligned
        assert raw(h64, h32, u, b) == _lib.ERR_ARG
    for u, b in ((host.ctypes.data, pb), (pu, host.ctypes.data)):  # a host pointer
        assert raw(h64, h32, u, b) == _lib.ERR_ARG
    for a, c in ((h32, h64), (h64, h64), (h32, h32)):  # swapped value types
        assert raw(a, c, pu, pb) == _lib.ERR_ARG and b"fp64" in lib.cfs_hip_last_error()
    for delta in (-0.1, 1.0, 1.5, float("nan")):
        assert raw(h64, h32, pu, pb, delta=delta) == _lib.ERR_ARG and b"delta" in lib.cfs_hip_last_error(), delta
    assert raw(h64, h32, pu, pb, delta=0.0) == 0  # the default
    for block_rows in (5, 7, -1, 8):
        assert raw(h64, h32, pu, pb, block_rows=block_rows) == _lib.ERR_ARG and b"block_rows" in lib.cfs_hip_last_error()
    assert raw(h64, h32, pu, pb, tol=-1.0) == _lib.ERR_ARG and raw(h64, h32, pu, pb, maxiter=-1) == _lib.ERR_ARG
    n2, rp2, ci2, va2 = _matrix("rand257")
    small = cfs.SymMatrix(n2, rp2, ci2, va2.astype(F32))
    assert raw(h64, small._h, pu, pb) == _lib.ERR_ARG and b"rows" in lib.cfs_hip_last_error()  # n mismatch
    small.close()
    if torch.cuda.device_count() > 1:  # a pointer on another device
        far = torch.zeros(n, dtype=torch.float64, device="cuda:1")
        assert raw(h64, h32, far.data_ptr(), pb) == _lib.ERR_ARG
    # the Python mirror
    with pytest.raises(ValueError):
        M.pcg(good, other, precond="ilu")
    with pytest.raises(TypeError):
        cfs.MixedSym.from_handles(M.A32, M.A64)
    splits = np.array([0, n // 2, n], np.int32)
    for dt, pair in ((F64, lambda H: (H._h, h32)), (F32, lambda H: (h64, H._h))):
        S = cfs.SymMatrix(n, rp, ci, va.astype(dt), row_splits=splits, rank=1)
        G = cfs.SymMatrix(n, rp, ci, va.astype(dt), ngpus=2)
        for H in (S, G):
            for block_rows in (0, 1, 3):
                assert raw(*pair(H), pu, pb, block_rows=block_rows) == _lib.ERR_UNSUPPORTED, (dt, block_rows)
            H.close()
    torch.cuda.synchronize()
    M.close()


# ---- 6. the host-driven loop ------------------------------------------------------------------------------------
def test_host_driven_and_native_loops_agree():
    """solver.pcg_mixed (torch-driven) against solver.pcg_mixed_native: both reach the tolerance; the counts within
    the band of test 2 (the looks fall on the same iterations; the sums differ in their order)"""
    import torch
    import cfs_spmv_amd as cfs
    from cfs_spmv_amd.solver import pcg_mixed, pcg_mixed_native
    n, rp, ci, va = _matrix("pwtk@0.05")
    va, b = scaled(n, rp, ci, va, F64), _rhs(n, F64)
    M = cfs.MixedSym(n, rp, ci, va)
    bd = torch.from_numpy(b).cuda()
    tol, check_every = 1e-10, 8
    u1, it1, rep1, res1 = pcg_mixed(M, bd, tol=tol, maxiter=500, check_every=check_every)
    u2, it2, rep2, res2 = pcg_mixed_native(M, bd, tol=tol, maxiter=500, check_every=check_every)
    torch.cuda.synchronize()
    print(f"mixed-steps pwtk@0.05 scaled: host-driven {it1} iterations / {rep1} replacements / {res1:.3e}, "
          f"native {it2} / {rep2} / {res2:.3e}")
    assert 0 < it1 < 500 and 0 < it2 < 500 and res1 <= 10 * tol and res2 <= 10 * tol
    assert abs(it1 - it2) <= check_every + 2 and abs(rep1 - rep2) <= 1
    u3, it3, rep3, res3 = pcg_mixed(M, bd, tol=tol, maxiter=500, precond="block_jacobi", check_every=check_every)
    u4, it4, rep4, res4 = pcg_mixed_native(M, bd, tol=tol, maxiter=500, precond="block_jacobi", check_every=check_every)
    assert res3 <= 10 * tol and res4 <= 10 * tol and abs(it3 - it4) <= check_every + 2 and abs(rep3 - rep4) <= 1, (it3, it4)
    M.close()
    # without a preconditioner, on the matrix as it is (the scaling above is what Jacobi is for)
    M = cfs.MixedSym(n, rp, ci, _matrix("pwtk@0.05")[3].astype(F64))
    u5, it5, rep5, res5 = pcg_mixed(M, bd, tol=tol, maxiter=500, precond="none", check_every=check_every)
    u6, it6, rep6, res6 = pcg_mixed_native(M, bd, tol=tol, maxiter=500, precond="none", check_every=check_every)
    print(f"mixed-steps pwtk@0.05: block Jacobi host-driven {it3} / {rep3}, native {it4} / {rep4}; "
          f"no preconditioner host-driven {it5} / {rep5}, native {it6} / {rep6}")
    assert res5 <= 10 * tol and res6 <= 10 * tol and abs(it5 - it6) <= check_every + 2 and abs(rep5 - rep6) <= 1, (it5, it6)
    M.close()
