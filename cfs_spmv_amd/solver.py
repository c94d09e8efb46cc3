"""Solver-style caller of the SpMV path: (Jacobi-preconditioned) conjugate gradients, MINRES for
symmetric indefinite and shifted systems, thick-restart Lanczos for extreme eigenpairs and LOBPCG for the smallest
ones, on resident vectors.

SURVEY.md 8(f)-4 / 8(e): the reference's only caller is a benchmark loop with a
fixed x; a solver feeds every product back as the next input, which is what the
y -> x all-gather of the sharded path exists for.  This is host-side control
flow only: the matrix-vector product is the HIP path (SymMatrix / ShardedSym),
the vector updates and dot products are torch plumbing on the same device.
"""
import math


def cg(A, b, tol=1e-10, maxiter=1000, x0=None):
    """solve A u = b for a symmetric positive definite SymMatrix (one GPU).
    b, u: device tensors of A.nrows() values.  Returns (u, iterations, relative
    residual ||b - A u|| / ||b||), the residual recomputed at the end."""
    import torch
    u = torch.zeros_like(b) if x0 is None else x0.clone()
    q = torch.empty_like(b)
    A.dense_vector_multiply(q, u)
    r = b - q
    p = r.clone()
    rr = float(torch.dot(r, r))
    bnorm = math.sqrt(float(torch.dot(b, b))) or 1.0
    it = 0
    while it < maxiter and math.sqrt(rr) > tol * bnorm:
        A.dense_vector_multiply(q, p)          # the hot path
        alpha = rr / float(torch.dot(p, q))
        u.add_(p, alpha=alpha)
        r.add_(q, alpha=-alpha)
        rr_new = float(torch.dot(r, r))
        p.mul_(rr_new / rr).add_(r)
        rr = rr_new
        it += 1
    A.dense_vector_multiply(q, u)
    res = math.sqrt(float(torch.dot(b - q, b - q))) / bnorm
    return u, it, res


def cg_native(A, b, tol=1e-10, maxiter=1000, x0=None, check_every=8):
    """the same iteration inside the library (cfs_hip_sym_cg, cfs_spmv_amd/csrc/cfs_solver.hpp):
    five launches per iteration and no host round trip -- the loop above reads two dot products
    on the host per iteration, a stream synchronisation each.  Returns (u, iterations, relative
    residual), like cg()."""
    import torch
    u = torch.zeros_like(b) if x0 is None else x0.clone()
    it, res = A.cg(u, b, tol=tol, maxiter=maxiter, check_every=check_every)
    return u, it, res


def _block_apply(minv, r, z):
    """z = blockdiag(minv) r: a batched mat-vec over the (nb, bs, bs) inverse blocks, formed in fp64
    like the library's; the tail of a trailing partial block is padded with zeros"""
    import torch
    nb, bs, _ = minv.shape
    n = r.numel()
    rp = torch.zeros(nb * bs, dtype=torch.float64, device=r.device)
    rp[:n] = r
    zp = torch.bmm(minv.double(), rp.view(nb, bs, 1)).view(-1)
    z.copy_(zp[:n])
    return z


def pcg(A, b, tol=1e-10, maxiter=1000, x0=None, precond="jacobi", block=3):
    """Jacobi-preconditioned conjugate gradients, host-driven: the recurrence of cfs_hip_sym_pcg
    (z = D^-1 r, alpha = r.z / p.q, beta = r'.z' / r.z, stop on the unpreconditioned ||r|| <= tol ||b||)
    with the diagonal taken from the handle (A.diagonal()), so the caller's CSR is not needed.
    precond = "block_jacobi": z = M^-1 r with the inverse node blocks of the handle
    (A.block_inverse(block)), the recurrence of cfs_hip_sym_pcg_block.
    Returns (u, iterations, relative residual), like cg()."""
    import torch
    if precond == "block_jacobi":
        minv = A.block_inverse(block)
        if not bool(torch.all(torch.isfinite(minv))):
            raise ValueError("pcg: block Jacobi needs positive definite diagonal blocks")
        apply = lambda r, z: _block_apply(minv, r, z)
    elif precond == "jacobi":
        d = A.diagonal()
        if not bool(torch.all(torch.isfinite(d) & (d > 0))):
            raise ValueError("pcg: Jacobi needs a positive diagonal")
        dinv = (1.0 / d.double()).to(b.dtype)
        apply = lambda r, z: torch.mul(r, dinv, out=z)
    else:
        raise ValueError(f"unknown preconditioner {precond!r}: 'jacobi' or 'block_jacobi'")
    u = torch.zeros_like(b) if x0 is None else x0.clone()
    q = torch.empty_like(b)
    A.dense_vector_multiply(q, u)
    r = b - q
    z = apply(r, torch.empty_like(r))
    p = z.clone()
    rz = float(torch.dot(r, z))
    rr = float(torch.dot(r, r))
    bnorm = math.sqrt(float(torch.dot(b, b))) or 1.0
    it = 0
    while it < maxiter and math.sqrt(rr) > tol * bnorm:
        A.dense_vector_multiply(q, p)          # the hot path
        alpha = rz / float(torch.dot(p, q))
        u.add_(p, alpha=alpha)
        r.add_(q, alpha=-alpha)
        apply(r, z)
        rz_new = float(torch.dot(r, z))
        rr = float(torch.dot(r, r))
        p.mul_(rz_new / rz).add_(z)
        rz = rz_new
        it += 1
    A.dense_vector_multiply(q, u)
    res = math.sqrt(float(torch.dot(b - q, b - q))) / bnorm
    return u, it, res


def pcg_native(A, b, precond="jacobi", tol=1e-10, maxiter=1000, x0=None, check_every=8, block=3):
    """the same iteration inside the library (cfs_hip_sym_pcg): still five launches per iteration, the
    diagonal gathered from the handle, z = D^-1 r never stored.  precond = "block_jacobi":
    cfs_hip_sym_pcg_block on the block x block node blocks.  Returns (u, iterations, relative
    residual), like pcg()."""
    import torch
    u = torch.zeros_like(b) if x0 is None else x0.clone()
    it, res = A.pcg(u, b, precond=precond, tol=tol, maxiter=maxiter, check_every=check_every, block=block)
    return u, it, res


def cheb_coeffs(degree, lmin, lmax):
    """theta and the degree - 1 pairs (rho_j rho_{j-1}, 2 rho_j / delta) of the Chebyshev iteration on
    [lmin, lmax], in fp64 as cfs_hip_debug_cheb_coeffs computes them"""
    theta, delta = 0.5 * (lmax + lmin), 0.5 * (lmax - lmin)
    sigma1 = theta / delta
    rho, pairs = 1.0 / sigma1, []
    for _ in range(1, degree):
        rn = 1.0 / (2.0 * sigma1 - rho)
        pairs.append((rn * rho, 2.0 * rn / delta))
        rho = rn
    return theta, pairs


def pcg_cheb(A, b, base="jacobi", block=3, degree=4, lmin=None, lmax=None, tol=1e-10, maxiter=1000, x0=None):
    """PCG with the Chebyshev polynomial preconditioner, host-driven: the recurrence and the rounding rules
    of cfs_hip_sym_pcg_cheb with torch operations -- z, d and t stored in the value type, every update computed
    in fp64 from the stored operands and rounded once, M^-1 from A.diagonal() / A.block_inverse(block).  The
    default bounds are the library's (1.1 x A.precond_lmax(), lmax / 30).  The model of the native loop and its
    baseline.  Returns (u, iterations, relative residual, (lmin, lmax))."""
    import torch
    f64 = torch.float64
    if base == "block_jacobi":
        minv = A.block_inverse(block)
        if not bool(torch.all(torch.isfinite(minv))):
            raise ValueError("pcg_cheb: block Jacobi needs positive definite diagonal blocks")
        apply = lambda x: _block_apply(minv, x, torch.empty_like(x))
    elif base == "jacobi":
        dg = A.diagonal()
        if not bool(torch.all(torch.isfinite(dg) & (dg > 0))):
            raise ValueError("pcg_cheb: Jacobi needs a positive diagonal")
        dinv = (1.0 / dg.double()).to(b.dtype).double()
        apply = lambda x: x * dinv
    elif base == "none":
        apply = lambda x: x
    else:
        raise ValueError(f"unknown base preconditioner {base!r}: 'none', 'jacobi' or 'block_jacobi'")
    if not lmax or lmax <= 0:
        lmax = 1.1 * A.precond_lmax(base=base, block=block)
    if not lmin or lmin <= 0:
        lmin = lmax / 30.0
    theta, pairs = cheb_coeffs(degree, lmin, lmax)
    t = torch.empty_like(b)

    def poly(r):
        """z = P_m r of the stored r"""
        rd = r.double()
        d = ((1.0 / theta) * apply(rd)).to(b.dtype)
        z = d.clone()
        for c1, c2 in pairs:
            A.dense_vector_multiply(t, z)
            d = (c1 * d.double() + c2 * apply(rd - t.double())).to(b.dtype)
            z = (z.double() + d.double()).to(b.dtype)
        return z

    u = torch.zeros_like(b) if x0 is None else x0.clone()
    q = torch.empty_like(b)
    A.dense_vector_multiply(q, u)
    r = b - q
    rr = float(torch.dot(r.double(), r.double()))
    bb = float(torch.dot(b.double(), b.double()))
    bnorm = math.sqrt(bb) or 1.0
    it = 0
    if maxiter > 0 and rr > tol * tol * bb:
        z = poly(r)
        p = z.clone()
        rz = float(torch.dot(r.double(), z.double()))
    while it < maxiter and rr > tol * tol * bb:
        A.dense_vector_multiply(q, p)          # the hot path
        pq = float(torch.dot(p.double(), q.double()))
        alpha = rz / pq if pq != 0.0 else 0.0
        u = (u.double() + alpha * p.double()).to(b.dtype)
        rs = r.double() - alpha * q.double()
        rr = float(torch.dot(rs, rs))
        r = rs.to(b.dtype)
        z = poly(r)
        rz_new = float(torch.dot(r.double(), z.double()))
        p = (z.double() + (rz_new / rz if rz != 0.0 else 0.0) * p.double()).to(b.dtype)
        rz = rz_new
        it += 1
    A.dense_vector_multiply(q, u)
    res = math.sqrt(float(torch.dot((b - q).double(), (b - q).double()))) / bnorm
    return u, it, res, (lmin, lmax)


def pcg_cheb_native(A, b, base="jacobi", block=3, degree=4, lmin=None, lmax=None, tol=1e-10, maxiter=1000, x0=None,
                    check_every=8):
    """the same iteration inside the library (cfs_hip_sym_pcg_cheb): 5 + 3 (degree - 1) launches per outer
    iteration, no dot product and no device scalar inside the polynomial.  Returns (u, iterations, relative
    residual, (lmin, lmax)), like pcg_cheb()."""
    import torch
    u = torch.zeros_like(b) if x0 is None else x0.clone()
    it, res, used = A.pcg_cheb(u, b, base=base, block=block, degree=degree, lmin=lmin, lmax=lmax, tol=tol, maxiter=maxiter,
                               check_every=check_every)
    return u, it, res, used


def pcg_amg(A, b, amg, tol=1e-10, maxiter=1000, x0=None):
    """PCG with the multigrid V-cycle as the preconditioner, host-driven: the recurrence and the rounding rules of
    cfs_hip_sym_pcg_amg with torch operations and amg.apply() as M^-1 (amg = A.amg(...)) -- u, r, p stored in the
    value type, every update computed in fp64 from the stored operands and rounded once, the dots in fp64 over the
    stored values, r.r from the unrounded update.  The model of the native loop and its baseline.  Returns (u,
    iterations, relative residual)."""
    import torch
    u = torch.zeros_like(b) if x0 is None else x0.clone()
    q = torch.empty_like(b)
    z = torch.empty_like(b)
    A.dense_vector_multiply(q, u)
    r = b - q
    rr = float(torch.dot(r.double(), r.double()))
    bb = float(torch.dot(b.double(), b.double()))
    bnorm = math.sqrt(bb) or 1.0
    it = 0
    if maxiter > 0 and rr > tol * tol * bb:
        amg.apply(z, r)
        p = z.clone()
        rz = float(torch.dot(r.double(), z.double()))
    while it < maxiter and rr > tol * tol * bb:
        A.dense_vector_multiply(q, p)          # the hot path
        pq = float(torch.dot(p.double(), q.double()))
        alpha = rz / pq if pq != 0.0 else 0.0
        u = (u.double() + alpha * p.double()).to(b.dtype)
        rs = r.double() - alpha * q.double()
        rr = float(torch.dot(rs, rs))
        r = rs.to(b.dtype)
        amg.apply(z, r)
        rz_new = float(torch.dot(r.double(), z.double()))
        p = (z.double() + (rz_new / rz if rz != 0.0 else 0.0) * p.double()).to(b.dtype)
        rz = rz_new
        it += 1
    A.dense_vector_multiply(q, u)
    res = math.sqrt(float(torch.dot((b - q).double(), (b - q).double()))) / bnorm
    return u, it, res


def pcg_amg_native(A, b, amg, tol=1e-10, maxiter=1000, x0=None, check_every=1):
    """the same iteration inside the library (cfs_hip_sym_pcg_amg): the product, four vector kernels and one cycle
    per iteration, one host look per iteration.  Returns (u, iterations, relative residual), like pcg_amg()."""
    import torch
    u = torch.zeros_like(b) if x0 is None else x0.clone()
    it, res = A.pcg_amg(u, b, amg, tol=tol, maxiter=maxiter, check_every=check_every)
    return u, it, res


def _pcg_cols_amg_args(precond, amg):
    """the two ValueErrors of precond="amg" / amg=, before any device work"""
    if precond == "amg" and amg is None:
        raise ValueError('pcg_cols: precond="amg" needs amg=, the hierarchy (A.amg(...))')
    if amg is not None and precond != "amg":
        raise ValueError(f'pcg_cols: amg= goes with precond="amg", not with {precond!r}')


def column_block(n, ncols, dtype, device="cuda"):
    """a zeroed (n, ncols) device block in the layout the column entry points take: strides (1, ld), ld = n rounded up
    to 16 bytes"""
    import torch
    per = 16 // torch.empty(0, dtype=dtype).element_size()
    ld = -(-n // per) * per
    return torch.as_strided(torch.zeros(max(ncols, 1) * max(ld, 1), dtype=dtype, device=device), (n, ncols), (1, ld))


def pcg_cols(A, B, precond="jacobi", block=3, amg=None, tol=1e-10, maxiter=1000, X0=None):
    """PCG on the columns of the (n, ncols) device block B, host-driven: one pcg() (precond = "jacobi", "block_jacobi"),
    cg() ("none") or pcg_amg() (precond="amg", amg=G) per column -- the model of cfs_hip_sym_pcg_cols /
    cfs_hip_sym_pcg_amg_cols, in which every column is the one-column solve on (u_c, b_c) alone.  X0: the first guesses,
    (n, ncols).  Returns (U, iterations, relres): U (n, ncols) with strides (1, ld), numpy arrays of ncols entries."""
    import numpy as np
    import torch
    _pcg_cols_amg_args(precond, amg)
    n, ncols = int(B.shape[0]), int(B.shape[1])
    U = column_block(n, ncols, B.dtype, B.device)
    its, res = np.zeros(ncols, np.int32), np.zeros(ncols, np.float64)
    for c in range(ncols):
        b = B[:, c].contiguous()
        x0 = None if X0 is None else X0[:, c].contiguous()
        if precond == "amg":
            u, its[c], res[c] = pcg_amg(A, b, amg, tol=tol, maxiter=maxiter, x0=x0)
        elif precond == "none":
            u, its[c], res[c] = cg(A, b, tol=tol, maxiter=maxiter, x0=x0)
        else:
            u, its[c], res[c] = pcg(A, b, tol=tol, maxiter=maxiter, x0=x0, precond=precond, block=block)
        U[:, c] = u
    return U, its, res


def pcg_cols_native(A, B, precond="jacobi", block=3, amg=None, tol=1e-10, maxiter=1000, X0=None, check_every=8):
    """the same solves inside the library as ONE call (cfs_hip_sym_pcg_cols, or cfs_hip_sym_pcg_amg_cols with
    precond="amg", amg=G): the set-up once, one product per active column, every vector kernel once for the block.
    B (n, ncols), any strides: it is copied into the column layout.  Returns (U, iterations, relres), like pcg_cols()."""
    _pcg_cols_amg_args(precond, amg)
    n, ncols = int(B.shape[0]), int(B.shape[1])
    U, Bc = column_block(n, ncols, B.dtype, B.device), column_block(n, ncols, B.dtype, B.device)
    Bc.copy_(B)
    if X0 is not None:
        U.copy_(X0)
    its, res = A.pcg_cols(U, Bc, precond=amg if precond == "amg" else precond, block=block, tol=tol, maxiter=maxiter,
                          check_every=check_every)
    return U, its, res


def pcg_mixed(M, b, tol=1e-10, delta=0.1, maxiter=1000, x0=None, precond="jacobi", block=3, check_every=8):
    """mixed-precision PCG, host-driven: the recurrence of cfs_hip_sym_pcg_mixed on a MixedSym.  One CG
    recurrence in float32 (r, p, q and the correction xlo; the products on M.A32; dots and z = M^-1 r in
    float64); once the recurrence's r.r has fallen below delta^2 times the largest seen at a look (every
    `check_every` iterations) since the last replacement, or below tol^2 b.b, u += xlo, xlo = 0 and the
    true float64 residual b - A64 u replaces r -- the search direction is kept.  b, x0: float64
    device tensors.  Returns (u, iterations, replacements, relative residual in float64)."""
    import torch
    f32 = torch.float32
    A64, A32 = M.A64, M.A32
    if precond == "block_jacobi":
        minv = A32.block_inverse(block)
        if not bool(torch.all(torch.isfinite(minv))):
            raise ValueError("pcg_mixed: block Jacobi needs positive definite diagonal blocks")
        apply = lambda r, z: _block_apply(minv, r, z)
    elif precond == "jacobi":
        d = A32.diagonal()
        if not bool(torch.all(torch.isfinite(d) & (d > 0))):
            raise ValueError("pcg_mixed: Jacobi needs a positive diagonal")
        dinv = (1.0 / d.double()).to(f32).double()
        apply = lambda r, z: torch.mul(r.double(), dinv, out=z)
    elif precond == "none":
        apply = lambda r, z: z.copy_(r)
    else:
        raise ValueError(f"unknown preconditioner {precond!r}: 'none', 'jacobi' or 'block_jacobi'")
    u = torch.zeros_like(b) if x0 is None else x0.clone()
    q64 = torch.empty_like(b)
    z = torch.empty_like(b)
    q = torch.empty(b.numel(), dtype=f32, device=b.device)
    xlo = torch.zeros_like(q)

    def replace():
        A64.dense_vector_multiply(q64, u)
        d64 = b - q64
        r = d64.to(f32)
        apply(r, z)
        return r, float(torch.dot(r.double(), z)), float(torch.dot(d64, d64))
    r, rz, rr = replace()
    p = z.to(f32)
    bb = float(torch.dot(b, b))
    stop, check_every = tol * tol * bb, max(1, min(int(check_every) if check_every >= 1 else 8, 16))
    it, nrep, rr_ref, folded = 0, 0, rr, True
    done = not (rr > stop)
    while not done and it < maxiter:
        until, flag, thr = min(maxiter, it + check_every), False, max(stop, delta * delta * rr_ref)
        while it < until and not flag:
            A32.dense_vector_multiply(q, p)        # the hot path, in float32
            pq = float(torch.dot(p.double(), q.double()))
            alpha = rz / pq if pq != 0.0 else 0.0
            xlo = (xlo.double() + alpha * p.double()).to(f32)
            rs = r.double() - alpha * q.double()
            rr = float(torch.dot(rs, rs))
            r = rs.to(f32)
            apply(r, z)
            rz_new = float(torch.dot(r.double(), z))
            p = (z + (rz_new / rz if rz != 0.0 else 0.0) * p.double()).to(f32)
            rz, it, folded = rz_new, it + 1, False
            flag = not (rr > thr)           # (the device flag: the rest of the window does nothing)
        rr_ref = max(rr_ref, rr)
        if flag or not (rr >= delta * delta * rr_ref):
            u.add_(xlo.double())
            xlo.zero_()
            r, rz, rr = replace()
            nrep, folded, rr_ref = nrep + 1, True, rr
            done = not (rr > stop)
    if not folded:
        u.add_(xlo.double())
        rr = replace()[2]
    return u, it, nrep, math.sqrt(rr / bb) if bb > 0.0 else math.sqrt(rr)


def pcg_mixed_native(M, b, precond="jacobi", tol=1e-10, delta=0.1, maxiter=1000, x0=None, check_every=8, block=3):
    """the same iteration inside the library (cfs_hip_sym_pcg_mixed): the five float32 launches per iteration
    and one that raises the replacement flag, no host round trip between two looks.  Returns (u, iterations, replacements, relative residual)."""
    import torch
    u = torch.zeros_like(b) if x0 is None else x0.clone()
    it, rep, res = M.pcg(u, b, precond=precond, block=block, tol=tol, delta=delta, maxiter=maxiter, check_every=check_every)
    return u, it, rep, res


def minres(A, b, precond="none", shift=0.0, tol=1e-10, maxiter=1000, x0=None):
    """MINRES (Paige & Saunders) for (A - shift I) u = b, host-driven: the recurrence of cfs_hip_sym_minres for a
    symmetric, possibly indefinite SymMatrix, with the scalars read on the host.  precond = "jacobi":
    M = |diag(A) - shift| with the diagonal taken from the handle (A.diagonal()).  Stops when the recurrence's
    phibar is at most tol sqrt(b . M^-1 b).  Returns (u, iterations, relative residual
    ||b - (A - shift I) u|| / ||b||), the residual recomputed at the end."""
    import torch
    f64 = torch.float64
    if precond == "jacobi":
        d = (A.diagonal().double() - shift).abs()
        if not bool(torch.all(torch.isfinite(d) & (d > 0))):
            raise ValueError("minres: Jacobi needs a nonzero diagonal of A - shift I")
        dinv = (1.0 / d).to(b.dtype).double()
    elif precond == "none":
        dinv = None
    else:
        raise ValueError(f"unknown preconditioner {precond!r}: 'none' or 'jacobi'")
    apply = (lambda r: r.double() * dinv) if dinv is not None else (lambda r: r.double())
    u = torch.zeros_like(b) if x0 is None else x0.clone()
    q = torch.empty_like(b)

    def residual():
        A.dense_vector_multiply(q, u)
        return b.double() - (q.double() - shift * u.double())
    r2 = residual().to(b.dtype)
    r1 = r2.clone()
    z = apply(r2)
    beta1 = math.sqrt(float(torch.dot(r2.double(), z)))
    bb = float(torch.dot(b.double(), b.double()))
    stop = tol * math.sqrt(float(torch.dot(b.double(), apply(b))))
    it = 0
    if beta1 > stop and beta1 > 0.0 and maxiter > 0:
        v = (z / beta1).to(b.dtype)
        w, w2 = torch.zeros_like(b), torch.zeros_like(b)
        oldb, beta, dbar, epsln, phibar, cs, sn = 0.0, beta1, 0.0, 0.0, beta1, -1.0, 0.0
        eps = 2.0 ** -52
        while it < maxiter:
            A.dense_vector_multiply(q, v)          # the hot path
            t = q.double() - shift * v.double()
            if it >= 1:
                t -= (beta / oldb) * r1.double()
            t = t.to(b.dtype)
            alfa = float(torch.dot(v.double(), t.double()))
            y = (t.double() - (alfa / beta) * r2.double()).to(b.dtype)
            r1, r2 = r2, y
            z = apply(y)
            bn2 = float(torch.dot(y.double(), z))
            betan = math.sqrt(bn2) if bn2 >= 0.0 else float("nan")
            oldeps, delta, gbar = epsln, cs * dbar + sn * alfa, sn * dbar - cs * alfa
            epsln, dbar = sn * betan, -cs * betan
            gamma = max(math.sqrt(gbar * gbar + betan * betan), eps)
            cs, sn = gbar / gamma, betan / gamma
            phi, phibar = cs * phibar, sn * phibar
            wn = ((v.double() - oldeps * w2.double() - delta * w.double()) / gamma).to(b.dtype)
            w2, w = w, wn
            u = (u.double() + phi * wn.double()).to(b.dtype)
            v = (z / betan).to(b.dtype) if betan > 0.0 else torch.zeros_like(b)
            oldb, beta, it = beta, betan, it + 1
            if not (phibar > stop) or not (betan > 0.0):
                break
    d = residual()
    res2 = float(torch.dot(d, d))
    return u, it, math.sqrt(res2 / bb) if bb > 0.0 else math.sqrt(res2)


def minres_native(A, b, precond="none", shift=0.0, tol=1e-10, maxiter=1000, x0=None, check_every=8):
    """the same iteration inside the library (cfs_hip_sym_minres): five launches per iteration, every scalar in
    device memory.  Returns (u, iterations, relative residual), like minres()."""
    import torch
    u = torch.zeros_like(b) if x0 is None else x0.clone()
    it, res = A.minres(u, b, precond=precond, shift=shift, tol=tol, maxiter=maxiter, check_every=check_every)
    return u, it, res


def _order(w, which):
    """indices of the Ritz values w (ascending) in the order of `which`"""
    import numpy as np
    if which == "SA":
        return np.arange(len(w))
    if which == "LA":
        return np.arange(len(w))[::-1]
    if which == "LM":
        d = np.arange(len(w))[::-1]
        return d[np.argsort(-np.abs(w[d]), kind="stable")]
    raise ValueError(f"unknown which {which!r}: 'LA', 'SA' or 'LM'")


def eigs(A, k, which="LA", ncv=None, tol=1e-10, max_restarts=100, v0=None):
    """k extreme eigenpairs by thick-restart Lanczos, host-driven: the recurrence, restart rule and kept count of
    cfs_hip_sym_eigs (full re-orthogonalisation in two passes, alpha_j = c_j + c'_j, breakdown when beta_j is not above
    16 u sqrt(q.q), l = k + (ncv - k) / 2 Ritz vectors kept) with torch operations on A's product and every coefficient
    read on the host -- the model and the baseline of the native loop.  Returns (w, X, info) like SymMatrix.eigs; X is
    an (n, k) device tensor, info["residuals"] the norms ||A x - theta x|| / ||x|| recomputed at the end."""
    import numpy as np
    import torch
    n = A.nrows()
    tdt = torch.float64 if A.dtype == np.float64 else torch.float32
    unit = 2.0 ** -53 if A.dtype == np.float64 else 2.0 ** -24
    if ncv is None:
        ncv = min(n, max(2 * k + 1, 20))
    if not 1 <= k < ncv <= n:
        raise ValueError("eigs: 1 <= k < ncv <= n")
    if v0 is None:
        raise ValueError("eigs: the host-driven loop needs a start vector")
    f64 = torch.float64
    V = torch.zeros((ncv + 1, n), dtype=tdt, device=v0.device)  # row j = v_{j+1}
    q = torch.empty(n, dtype=tdt, device=v0.device)
    V[0] = (v0.double() / float(torch.linalg.vector_norm(v0.double()))).to(tdt)
    lkeep = k + (ncv - k) // 2
    alpha, beta, arrow = np.zeros(ncv), np.zeros(ncv), np.zeros(ncv)
    l, restarts, products, broke = 0, 0, 0, False
    while True:
        m = ncv
        for j in range(l, ncv):
            A.dense_vector_multiply(q, V[j])          # the hot path
            products += 1
            Vj = V[:j + 1].double()
            c = Vj @ q.double()
            qq = float(torch.dot(q.double(), q.double()))
            q1 = (q.double() - c @ Vj).to(tdt)
            c2 = Vj @ q1.double()
            q2 = (q1.double() - c2 @ Vj).to(tdt)
            alpha[j] = float(c[j]) + float(c2[j])
            beta[j] = math.sqrt(float(torch.dot(q2.double(), q2.double())))
            if not beta[j] > 16.0 * unit * math.sqrt(qq):
                V[j + 1].zero_()
                m, broke = j + 1, True
                break
            V[j + 1] = (q2.double() / beta[j]).to(tdt)
        T = np.diag(alpha[:m])
        T[:l, l] = T[l, :l] = arrow[:l]
        for i in range(l, m - 1):
            T[i, i + 1] = T[i + 1, i] = beta[i]
        w, S = np.linalg.eigh(T)
        order = _order(w, which)
        bm = 0.0 if broke else beta[m - 1]
        est = np.abs(bm * S[m - 1, order])
        kk = min(k, m)
        nconv = 0
        while nconv < kk and est[nconv] <= tol * np.max(np.abs(w)):
            nconv += 1
        if broke:
            nconv = kk
        if broke or nconv == k or restarts >= max_restarts:
            break
        Sk = torch.from_numpy(np.ascontiguousarray(S[:, order[:lkeep]])).to(V.device)
        V[:lkeep] = (Sk.T @ V[:m].double()).to(tdt)
        V[lkeep] = V[m]
        alpha[:lkeep], arrow[:lkeep] = w[order[:lkeep]], bm * S[m - 1, order[:lkeep]]
        l, restarts = lkeep, restarts + 1
    Sk = torch.from_numpy(np.ascontiguousarray(S[:, order[:kk]])).to(V.device)
    X = torch.zeros((k, n), dtype=tdt, device=V.device)
    X[:kk] = (Sk.T @ V[:m].double()).to(tdt)
    wk, res = np.zeros(k), np.zeros(k)
    wk[:kk] = w[order[:kk]]
    for i in range(kk):
        A.dense_vector_multiply(q, X[i])
        products += 1
        d = q.double() - wk[i] * X[i].double()
        res[i] = float(torch.linalg.vector_norm(d)) / float(torch.linalg.vector_norm(X[i].double()))
    return wk, X.T, {"nconv": nconv, "restarts": restarts, "products": products, "residuals": res}


def eigs_native(A, k, which="LA", ncv=None, tol=1e-10, max_restarts=100, v0=None, vectors=True):
    """the same iteration inside the library (cfs_hip_sym_eigs): nine launches per step, alpha, beta and the breakdown
    flag in device memory, the host looks only when the basis is full.  Returns (w, X, info), like eigs()."""
    return A.eigs(k=k, which=which, ncv=ncv, tol=tol, max_restarts=max_restarts, v0=v0, vectors=vectors)


def lobpcg_rr(G, H, k, drop):
    """step 2 of cfs_hip_sym_lobpcg in numpy (the upper triangles of G and H are read): d_j = G_jj^-1/2, columns whose
    G_jj is not finite and > 0 dropped; the eigenvectors of D G D with w > drop w_max kept, Q = D U w^-1/2; T = Q^T H Q
    symmetrised; C = Q Z[:, :k].  Returns (theta, C, rank), C (m, k) with zero rows for dropped columns."""
    import numpy as np
    m = G.shape[0]
    G = np.triu(G) + np.triu(G, 1).T
    H = np.triu(H) + np.triu(H, 1).T
    g = np.diag(G)
    with np.errstate(all="ignore"):
        keep = np.flatnonzero(np.isfinite(g) & (g > 0))
        d = 1.0 / np.sqrt(g[keep])
    theta, C = np.zeros(k, G.dtype), np.zeros((m, k), G.dtype)
    if keep.size == 0:
        return theta, C, 0
    w, U = np.linalg.eigh((d[:, None] * G[np.ix_(keep, keep)] * d[None, :]).astype(np.float64))
    sel = w > drop * w[-1]
    r = int(np.count_nonzero(sel))
    if r == 0:
        return theta, C, 0
    Q = (d[:, None] * U[:, sel].astype(G.dtype)) / np.sqrt(w[sel].astype(G.dtype))[None, :]
    T = Q.T @ H[np.ix_(keep, keep)] @ Q
    T = 0.5 * (T + T.T)
    tw, Z = np.linalg.eigh(T.astype(np.float64))
    kk = min(k, r)
    theta[:kk] = tw[:kk]
    C[keep, :kk] = Q @ Z[:, :kk].astype(G.dtype)
    return theta, C, r


def default_x0(n, k, dtype):
    """the start block of a NULL x0_dev (include/cfs_hip.h): x0[i, c] = v0(i + c n) of the splitmix64 sequence, as a
    numpy array (n, k) of `dtype`"""
    import numpy as np
    with np.errstate(over="ignore"):
        z = (np.arange(n * k, dtype=np.uint64) + np.uint64(1)) * np.uint64(0x9E3779B97F4A7C15)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        z ^= z >> np.uint64(31)
    v = (z >> np.uint64(11)).astype(np.float64) * 2.0 ** -53 - 0.5
    return np.ascontiguousarray(v.reshape(k, n).T.astype(dtype))


def _lobpcg_amg_args(precond, amg):
    """the two ValueErrors of precond="amg" / amg=, before any device work"""
    if precond == "amg" and amg is None:
        raise ValueError('lobpcg: precond="amg" needs amg=, the hierarchy (A.amg(...))')
    if amg is not None and precond != "amg":
        raise ValueError(f'lobpcg: amg= goes with precond="amg", not with {precond!r}')


def _lobpcg_minv(A, precond, block, amg=None):
    """apply(R) -> M^-1 R in fp64 for an (n, j) block, with the stored inverse diagonal / inverse blocks of the handle.
    precond="amg": apply(R, cols) -> an (n, j) block whose columns `cols` are one cycle of `amg` each, on the column
    rounded to the value type as the native loop stores it, by the ONE-COLUMN amg.apply (the model does not depend on the
    blocked kernels); the other columns are zero"""
    import numpy as np
    import torch
    if precond == "amg":
        tdt = torch.float64 if A.dtype == np.float64 else torch.float32

        def cycles(R, cols):
            n, j = R.shape
            out = torch.zeros((n, j), dtype=torch.float64, device=R.device)
            r, z = torch.empty(n, dtype=tdt, device=R.device), torch.empty(n, dtype=tdt, device=R.device)
            for c in cols:
                r.copy_(R[:, c])
                amg.apply(z, r)
                out[:, c] = z.double()
            return out
        return cycles
    if precond == "none":
        return lambda R: R
    if precond == "jacobi":
        d = A.diagonal()
        if not bool(torch.all(torch.isfinite(d) & (d > 0))):
            raise ValueError("lobpcg: Jacobi needs a positive diagonal")
        dinv = (1.0 / d.double()).to(d.dtype).double()
        return lambda R: R * dinv[:, None]
    if precond == "block_jacobi":
        minv = A.block_inverse(block)
        if not bool(torch.all(torch.isfinite(minv))):
            raise ValueError("lobpcg: block Jacobi needs positive definite diagonal blocks")
        nb, bs, _ = minv.shape
        m64 = minv.double()

        def apply(R):
            n, j = R.shape
            Rp = torch.zeros((nb * bs, j), dtype=torch.float64, device=R.device)
            Rp[:n] = R
            return torch.bmm(m64, Rp.view(nb, bs, j)).reshape(nb * bs, j)[:n]
        return apply
    raise ValueError(f"unknown preconditioner {precond!r}: 'none', 'jacobi' or 'block_jacobi'")


def _lobpcg_pencil_b(A, B):
    """the ValueError of a B that is not a SymMatrix of A's n and dtype, before any device work"""
    if B is not None:
        A._pencil_b(B)


def lobpcg(A, k, precond="jacobi", block=3, tol=1e-10, scale=None, maxiter=500, x0=None, iters=None, amg=None, B=None):
    """the k smallest eigenpairs by LOBPCG, host-driven: the recurrence of cfs_hip_sym_lobpcg (Gram matrices of
    S = [X | W | P_act] in fp64, the Rayleigh-Ritz step with its drop rule, X, P, AX, AP updated implicitly and rounded
    to the value type when stored, W = M^-1 R in fp64, soft locking, the confirm step) with torch operations on A's
    product and numpy on the host -- the model and the baseline of the native loop.  iters: like
    cfs_hip_sym_debug_lobpcg, iteration 0 and `iters` more with every pair active, no convergence test.  Returns
    (w, X, info) like SymMatrix.lobpcg; with iters, info["residuals"] are those of the implicit AX.
    precond="amg", amg=G: the model of cfs_hip_sym_lobpcg_amg -- W_i one cycle of G on the stored R_i, for the pairs the
    native loop forms it for (those active, as its wmask); info["cycles"] counts them.
    B = a SymMatrix of A's n and dtype: the model of cfs_hip_sym_lobpcg_gen(_amg), the pencil A x = lambda B x -- a third
    block BS = B S kept by products and updates as AS is, G = S^T BS, R = AX - theta BX, the confirm step recomputes AX and
    BX; X comes out B-orthonormal; info["b_products"] counts the products with B."""
    import numpy as np
    import torch
    _lobpcg_amg_args(precond, amg)
    _lobpcg_pencil_b(A, B)
    n = A.nrows()
    tdt = torch.float64 if A.dtype == np.float64 else torch.float32
    unit = 2.0 ** -53 if A.dtype == np.float64 else 2.0 ** -24
    if not (1 <= k <= 16 and 3 * k <= n):
        raise ValueError("lobpcg: 1 <= k <= 16 and 3 k <= n")
    debug = iters is not None
    if scale is None and not debug:
        scale = abs(float(A.eigs(k=1, which="LM", tol=1e-3, vectors=False)[0][0]))
    thr = 0.0 if debug else tol * scale
    apply = _lobpcg_minv(A, precond, block, amg)
    cycles = 0
    dev = "cuda" if x0 is None else x0.device
    S = torch.zeros((3 * k, n), dtype=tdt, device=dev)   # row c = physical column c: X | W | P
    AS = torch.zeros((3 * k, n), dtype=tdt, device=dev)
    BS = torch.zeros((3 * k, n), dtype=tdt, device=dev) if B is not None else None
    S[:k] = (torch.from_numpy(default_x0(n, k, A.dtype)).to(dev) if x0 is None else x0.to(tdt)).T
    products = b_products = 0

    def product(c):
        nonlocal products, b_products
        A.dense_vector_multiply(AS[c], S[c])          # the hot path
        products += 1
        if B is not None:
            B.dense_vector_multiply(BS[c], S[c])
            b_products += 1

    for c in range(k):
        product(c)
    theta = np.zeros(k)

    def rayleigh_ritz(cols):
        nonlocal theta
        idx = torch.tensor(cols, device=dev)
        Sa, ASa = S[idx].double(), AS[idx].double()
        BSa = BS[idx].double() if B is not None else Sa
        G, H = (Sa @ BSa.T).cpu().numpy(), (Sa @ ASa.T).cpu().numpy()
        theta, C, rank = lobpcg_rr(G, H, k, 64.0 * unit)
        Ct = torch.from_numpy(C).to(dev)
        Cp = Ct.clone()
        Cp[:k] = 0.0
        X, AX = (Ct.T @ Sa).to(tdt), (Ct.T @ ASa).to(tdt)
        if len(cols) > k:
            S[2 * k:], AS[2 * k:] = (Cp.T @ Sa).to(tdt), (Cp.T @ ASa).to(tdt)
        if B is not None:
            if len(cols) > k:
                BS[2 * k:] = (Cp.T @ BSa).to(tdt)
            BS[:k] = (Ct.T @ BSa).to(tdt)
        S[:k], AS[:k] = X, AX
        return rank

    res = np.zeros(k)

    def norms(wcols=None):
        nonlocal cycles
        X, AX = S[:k].double(), AS[:k].double()
        R = AX - torch.from_numpy(theta).to(dev)[:, None] * (BS[:k].double() if B is not None else X)
        if amg is None:
            S[k:2 * k] = apply(R.T).T.to(tdt)
        else:  # (the native loop's wmask: every pair, or those active)
            wcols = list(range(k)) if wcols is None else wcols
            cycles += len(wcols)
            S[k:2 * k] = apply(R.T, wcols).T.to(tdt)
        res[:] = (torch.linalg.vector_norm(R, dim=1) / torch.linalg.vector_norm(X, dim=1)).cpu().numpy()

    for attempt in range(3):
        rank = rayleigh_ritz(list(range(k)))
        if rank == k:
            break
        if attempt == 2:
            raise ValueError("lobpcg: the start block does not have rank k" +
                             (" in the B inner product: B may not be positive definite" if B is not None else ""))
        fill = default_x0(n, k * (attempt + 2), A.dtype)
        for c in range(rank, k):
            S[c] = torch.from_numpy(fill[:, k * (attempt + 1) + c]).to(dev)
            product(c)
    norms()
    it, fresh, have_p = 0, False, False
    wmask = list(range(k))
    while True:
        act = [i for i in range(k) if debug or not res[i] <= thr]
        if not debug and not act:
            if fresh:
                break
            for c in range(k):
                product(c)
            norms()
            wmask = list(range(k))
            fresh = True
            continue
        if it >= (iters if debug else maxiter):
            break
        if amg is not None and set(act) - set(wmask):  # a pair that had converged and no longer does: its W is formed now
            norms(act)
            wmask = act
        for i in act:
            product(k + i)
        cols = list(range(k)) + [k + i for i in act] + ([2 * k + i for i in act] if have_p else [])
        if rayleigh_ritz(cols) < k:
            raise RuntimeError("lobpcg: the basis lost rank")
        have_p, fresh = True, False
        wmask = act
        norms(act)
        it += 1
    if not debug and not fresh:
        for c in range(k):
            product(c)
        norms([])
    nconv = 0
    while nconv < k and res[nconv] <= thr:
        nconv += 1
    info = {"nconv": nconv, "iterations": it, "products": products, "residuals": res.copy()}
    if amg is not None:
        info["cycles"] = cycles
    if B is not None:
        info["b_products"] = b_products
    return theta.copy(), S[:k].T.clone(), info


def lobpcg_native(A, k, precond="jacobi", block=3, tol=1e-10, scale=None, maxiter=500, x0=None, amg=None, B=None):
    """the same iteration inside the library (cfs_hip_sym_lobpcg): the Gram matrices by one small-SYRK kernel, the
    update in place, residual and preconditioner in one kernel; two host looks per iteration.  Returns (w, X, info),
    like lobpcg().  precond="amg", amg=G: cfs_hip_sym_lobpcg_amg, W by one column-blocked cycle of G per iteration.
    B: the pencil A x = lambda B x (cfs_hip_sym_lobpcg_gen, _gen_amg)."""
    _lobpcg_amg_args(precond, amg)
    _lobpcg_pencil_b(A, B)
    kw = dict(k=k, precond=amg if amg is not None else precond, block=block, tol=tol, scale=scale, maxiter=maxiter, x0=x0)
    return A.lobpcg(**kw) if B is None else A.lobpcg_gen(B, **kw)


def cg_sharded(S, row_splits, b_block, tol=1e-10, maxiter=1000):
    """the same iteration over 1-D row blocks (cfs_spmv_amd.dist.ShardedSym): every
    rank keeps its block of u, r, q and a full replica of the search direction p,
    refreshed by one all-gather per iteration; dot products are all-reduced.
    Returns (u_block, iterations, relative residual)."""
    torch, dist = S.torch, S.dist
    S.setup_allgather(row_splits)
    rb, re = int(row_splits[S.rank]), int(row_splits[S.rank + 1])
    n = int(row_splits[-1])
    dev = b_block.device

    def gdot(a, c):
        t = torch.dot(a, c).reshape(1)
        if S.stage or t.device.type == "cpu":
            t = t.cpu()
            dist.all_reduce(t, group=S.pg)
        else:
            dist.all_reduce(t, group=S.pg)
        return float(t)

    u = torch.zeros_like(b_block)
    r = b_block.clone()                         # u = 0: r = b
    p_full = torch.zeros(n, dtype=b_block.dtype, device=dev)
    S.allgather_rows(r, p_full)
    q = torch.empty_like(b_block)
    rr = gdot(r, r)
    bnorm = math.sqrt(rr) or 1.0
    it = 0
    while it < maxiter and math.sqrt(rr) > tol * bnorm:
        S.spmv(q, p_full)                       # the hot path, exchange included
        p = p_full[rb:re]
        alpha = rr / gdot(p, q)
        u.add_(p, alpha=alpha)
        r.add_(q, alpha=-alpha)
        rr_new = gdot(r, r)
        p_new = r + p * (rr_new / rr)
        S.allgather_rows(p_new, p_full)         # y -> x: next input on every rank
        rr = rr_new
        it += 1
    u_full = torch.zeros(n, dtype=b_block.dtype, device=dev)
    S.allgather_rows(u, u_full)
    S.spmv(q, u_full)
    d = b_block - q
    res = math.sqrt(gdot(d, d)) / bnorm
    return u, it, res
