"""cfs_hip_sym_pcg_block step by step, by the method of test_gpu_pcg_steps.py: block Jacobi on the bs x bs
node blocks, M = blockdiag(A) -- cfs_block_gather_kernel and cg_binv_kernel once, then cg_residual_kernel,
cg_dot_kernel, cg_update_kernel, cg_direction_kernel<V, bs, ..., OneColumn> behind the SpMV.

1. The inverse.  Minv = A.block_inverse(bs) (the solver's two set-up kernels plus an unpack) against the
   inverse of the blocks in np.longdouble.  The yardstick e_ref is the distance from that of the same
   Cholesky-then-inverse run in numpy in fp64 on the blocks rounded to the value type, its result rounded to
   the value type (max-norm, relative per block, the largest over the blocks); the GPU is allowed
   4 e_ref + 16 u.  Neither side involves the library.

2. The iterates u_k against the recurrence of test_gpu_pcg_steps.py with z = Minv r in np.longdouble; the
   allowance 4 d_k + 16 u with d_k the deviation of the same recurrence in the working precision of the
   kernels (z kept in fp64 and formed from the rounded r).  The preconditioner in BOTH is the Minv read back
   from the library, converted exactly: the recurrence is then well defined whatever the last bits of the
   inversion (which 1. pins), and a correct GPU run differs from the working-precision run only in the order
   of the additions.

3. What it is for: a matrix of rotated node blocks, on which point Jacobi needs many times the iterations.

Measured on the MI355X (value type, matrix, bs, then for k = 1, 2, 3, 5, 10: d_k / the GPU's deviation):

  f64 pwtk@0.05                          bs=3  1.9e-16/1.1e-16  3.1e-16/2.0e-16  2.8e-16/2.0e-16  3.1e-16/2.5e-16  3.3e-16/2.2e-16
  f32 pwtk@0.05                          bs=3  6.1e-08/3.9e-08  1.7e-07/9.2e-08  1.4e-07/1.1e-07  1.4e-07/1.3e-07  1.5e-07/1.5e-07
  f64 Flan_1565@0.01                     bs=3  2.9e-16/1.6e-16  6.5e-16/3.7e-16  4.1e-16/3.5e-16  3.9e-16/4.4e-16  4.2e-16/7.3e-16
  f32 Flan_1565@0.01                     bs=3  6.2e-08/6.2e-08  3.2e-07/1.5e-07  2.3e-07/1.0e-07  2.4e-07/9.3e-08  2.1e-07/1.2e-07
  f64 rand1                              bs=3  0.0e+00/0.0e+00  0.0e+00/0.0e+00  0.0e+00/0.0e+00  0.0e+00/0.0e+00  0.0e+00/0.0e+00
  f32 rand1                              bs=3  0.0e+00/0.0e+00  0.0e+00/0.0e+00  0.0e+00/0.0e+00  0.0e+00/0.0e+00  0.0e+00/0.0e+00
  f64 rand2                              bs=3  7.1e-17/7.1e-17  7.1e-17/7.1e-17  7.1e-17/7.1e-17  7.1e-17/7.1e-17  7.1e-17/7.1e-17
  f32 rand2                              bs=3  6.1e-08/6.1e-08  6.1e-08/6.1e-08  6.1e-08/6.1e-08  6.1e-08/6.1e-08  6.1e-08/6.1e-08
  f64 rand3                              bs=3  7.7e-17/7.7e-17  7.7e-17/7.7e-17  7.7e-17/7.7e-17  7.7e-17/7.7e-17  7.7e-17/7.7e-17
  f32 rand3                              bs=3  3.2e-08/3.2e-08  4.3e-08/4.3e-08  4.3e-08/4.3e-08  4.3e-08/4.3e-08  4.3e-08/4.3e-08
  f64 rand5                              bs=3  1.6e-16/2.8e-17  3.9e-17/1.8e-16  7.4e-17/1.3e-16  1.5e-16/1.2e-16  1.5e-16/1.2e-16
  f32 rand5                              bs=3  9.4e-08/9.4e-08  6.7e-08/6.7e-08  8.9e-08/8.9e-08  8.0e-08/8.0e-08  8.0e-08/8.0e-08
  f64 rand63                             bs=3  1.9e-16/1.6e-16  1.0e-16/1.3e-16  7.9e-17/6.2e-17  1.2e-16/1.2e-16  1.9e-16/1.9e-16
  f32 rand63                             bs=3  3.3e-08/2.9e-08  6.9e-08/5.4e-08  1.1e-07/5.8e-08  1.6e-07/4.7e-08  7.6e-08/3.4e-08
  f64 rand64                             bs=3  1.8e-16/1.8e-16  1.2e-16/5.5e-17  1.3e-16/8.4e-17  1.1e-16/1.8e-16  1.5e-16/2.1e-16
  f32 rand64                             bs=3  4.8e-08/4.8e-08  4.3e-08/4.3e-08  5.3e-08/3.7e-08  4.1e-08/4.2e-08  9.6e-08/9.6e-08
  f64 rand65                             bs=3  4.7e-16/1.0e-16  2.4e-16/1.3e-16  1.8e-16/2.3e-16  1.5e-16/1.5e-16  2.4e-16/2.3e-16
  f32 rand65                             bs=3  2.2e-08/4.0e-08  5.3e-08/5.3e-08  1.2e-07/1.2e-07  9.1e-08/9.1e-08  1.3e-07/1.3e-07
  f64 rand255                            bs=3  3.9e-17/3.9e-17  7.7e-17/1.2e-16  9.8e-17/1.4e-16  1.3e-16/1.5e-16  1.9e-16/1.9e-16
  f32 rand255                            bs=3  2.7e-08/2.7e-08  5.4e-08/5.4e-08  4.5e-08/6.7e-08  1.1e-07/5.5e-08  9.5e-08/5.8e-08
  f64 rand257                            bs=3  1.1e-16/9.0e-17  1.4e-16/1.7e-16  1.3e-16/1.9e-16  2.2e-16/2.4e-16  2.2e-16/2.5e-16
  f32 rand257                            bs=3  3.3e-08/3.3e-08  7.5e-08/7.5e-08  1.0e-07/1.0e-07  1.1e-07/1.1e-07  1.8e-07/1.8e-07
  f64 rand1023                           bs=3  5.3e-16/1.3e-16  3.1e-16/1.5e-16  3.2e-16/1.5e-16  4.5e-16/2.8e-16  3.6e-16/2.1e-16
  f32 rand1023                           bs=3  5.5e-08/5.5e-08  5.1e-08/5.1e-08  6.8e-08/6.8e-08  1.1e-07/1.1e-07  2.4e-07/2.4e-07
  f64 rand1026                           bs=3  7.5e-17/3.1e-16  1.1e-16/2.0e-16  1.0e-16/2.1e-16  1.0e-16/2.5e-16  2.3e-16/3.9e-16
  f32 rand1026                           bs=3  5.4e-08/5.4e-08  6.3e-08/6.3e-08  5.6e-08/5.6e-08  7.0e-08/1.1e-07  8.2e-08/7.5e-08
  f64 band600001                         bs=3  2.8e-16/2.7e-16  3.5e-16/3.8e-16  3.2e-16/3.9e-16  3.7e-16/4.3e-16  4.8e-16/4.8e-16
  f32 band600001                         bs=3  8.9e-08/8.9e-08  1.6e-07/1.3e-07  1.9e-07/1.4e-07  2.1e-07/1.6e-07  2.5e-07/2.5e-07
  f64 rand65                             bs=2  1.5e-16/1.2e-16  2.4e-16/2.2e-16  2.6e-16/1.7e-16  1.9e-16/2.2e-16  2.6e-16/2.6e-16
  f32 rand65                             bs=2  6.4e-08/6.4e-08  1.1e-07/4.9e-08  1.7e-07/7.1e-08  1.8e-07/8.0e-08  1.1e-07/6.9e-08
  f64 rand65                             bs=4  3.8e-16/1.8e-16  2.0e-16/2.0e-16  2.6e-16/1.3e-16  1.6e-16/1.3e-16  2.5e-16/2.5e-16
  f32 rand65                             bs=4  5.6e-08/8.8e-08  9.4e-08/1.2e-07  1.6e-07/1.1e-07  1.8e-07/1.5e-07  2.5e-07/1.1e-07
  f64 rand65                             bs=6  3.4e-16/8.6e-17  1.1e-16/1.1e-16  1.2e-16/1.2e-16  2.1e-16/2.2e-16  2.8e-16/5.6e-16
  f32 rand65                             bs=6  8.5e-08/9.0e-08  7.5e-08/1.2e-07  1.6e-07/1.3e-07  1.1e-07/1.7e-07  1.8e-07/1.3e-07
  f64 rand1026                           bs=2  1.1e-16/1.1e-16  2.3e-16/1.1e-16  2.6e-16/1.2e-16  1.7e-16/1.4e-16  2.2e-16/2.2e-16
  f32 rand1026                           bs=2  5.7e-08/5.7e-08  5.1e-08/5.1e-08  5.5e-08/5.5e-08  4.7e-08/4.7e-08  7.5e-08/7.2e-08
  f64 rand1026                           bs=4  1.8e-16/5.5e-17  1.9e-16/8.4e-17  2.1e-16/9.3e-17  1.8e-16/1.3e-16  2.2e-16/2.2e-16
  f32 rand1026                           bs=4  4.4e-08/4.4e-08  3.5e-08/3.4e-08  5.0e-08/5.0e-08  5.5e-08/5.7e-08  8.2e-08/8.2e-08
  f64 rand1026                           bs=6  1.7e-16/2.3e-16  1.6e-16/1.6e-16  1.7e-16/1.7e-16  1.6e-16/1.5e-16  1.7e-16/2.1e-16
  f32 rand1026                           bs=6  2.8e-08/2.8e-08  4.8e-08/4.8e-08  5.7e-08/5.7e-08  8.2e-08/8.2e-08  8.6e-08/8.6e-08
  f64 Flan_1565@0.01 (deterministic)     bs=3  2.9e-16/1.6e-16  6.5e-16/2.0e-16  4.1e-16/1.8e-16  3.9e-16/2.0e-16  4.2e-16/2.3e-16
  f32 Flan_1565@0.01 (deterministic)     bs=3  6.2e-08/6.2e-08  3.2e-07/1.5e-07  2.3e-07/1.0e-07  2.4e-07/9.3e-08  2.1e-07/1.2e-07
  f64 rand1023 (captured graph)          bs=3  3.7e-16/2.0e-16  4.5e-16/2.8e-16
"""
import ctypes as C

import numpy as np
import pytest

from test_gpu_cg_steps import D_LIMIT, DET, DTYPES, KS, MATRICES, UNIT, _deviation, _matrix, _rhs, _true_relres
from test_gpu_kernel_variants import PLAN_KNOBS
from test_gpu_pcg_steps import pcg_reference, scaled

pytestmark = pytest.mark.gpu

LD = np.longdouble


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
def node_blocks(n, rp, ci, va, bs):
    """(nb, bs, bs) diagonal blocks of the CSR (va already in the value type), identity outside the matrix"""
    import scipy.sparse as sp
    A = sp.csr_matrix((va, ci.copy(), rp.copy()), shape=(n, n))
    A.sum_duplicates()
    coo = A.tocoo()
    m = coo.row // bs == coo.col // bs
    nb = -(-n // bs)
    out = np.zeros((nb, bs, bs), va.dtype)
    out[coo.row[m] // bs, coo.row[m] % bs, coo.col[m] % bs] = coo.data[m]
    for i in range(n, nb * bs):
        out[i // bs, i % bs, i % bs] = 1
    return out


def cholesky_inverse(blocks, S):
    """A = L L^T, L^-1, A^-1 = L^-T L^-1 of every block in precision S, vectorised over the blocks"""
    a = blocks.astype(S)
    nb, bs, _ = a.shape
    L = np.zeros_like(a)
    for j in range(bs):
        d = a[:, j, j] - np.sum(L[:, j, :j] * L[:, j, :j], axis=1)
        L[:, j, j] = np.sqrt(d)
        for i in range(j + 1, bs):
            L[:, i, j] = (a[:, i, j] - np.sum(L[:, i, :j] * L[:, j, :j], axis=1)) / L[:, j, j]
    Li = np.zeros_like(a)
    for j in range(bs):
        Li[:, j, j] = 1 / L[:, j, j]
        for i in range(j + 1, bs):
            Li[:, i, j] = -np.sum(L[:, i, j:i] * Li[:, j:i, j], axis=1) / L[:, i, i]
    return np.einsum("kci,kcj->kij", Li, Li)


def _block_distance(x, ref):
    """max-norm distance, relative per block; the largest over the blocks"""
    x, ref = x.astype(LD), ref.astype(LD)
    return float(np.max(np.max(np.abs(x - ref), axis=(1, 2)) / np.max(np.abs(ref), axis=(1, 2))))


def block_pcg_reference(n, rp, ci, va, b, minv, ks=(), dtype=None, tol=0.0, maxiter=None, x0=None):
    """test_gpu_pcg_steps.pcg_reference (from u = x0, or 0) with z = Minv r over the node blocks: minv (nb, bs, bs) is converted
    exactly to long double (dtype None) / to fp64 (the working precision: z formed in fp64 from the rounded r
    and never rounded)"""
    import scipy.sparse as sp
    from oracle import oracle
    ld = dtype is None
    W, S = (LD, LD) if ld else (dtype, np.float64)
    nb, bs, _ = minv.shape
    M = minv.astype(S)
    if ld:
        def mv(x):
            return oracle.csr_spmv_ldx(n, rp, ci, va, x)
    else:
        A = sp.csr_matrix((va.astype(dtype), ci, rp), shape=(n, n))

        def mv(x):
            return (A @ x).astype(dtype)

    def apply(r):  # r in S
        rp_ = np.zeros(nb * bs, S)
        rp_[:n] = r
        z = np.zeros((nb, bs), S)
        rb = rp_.reshape(nb, bs)
        for j in range(bs):  # (ascending j, as the kernels)
            z += M[:, :, j] * rb[:, j:j + 1]
        return z.reshape(-1)[:n]
    u = np.zeros(n, W) if x0 is None else x0.astype(W)
    r = (b.astype(S) - mv(u).astype(S)).astype(W)
    z = apply(r.astype(S))
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
            z = apply(r.astype(S))
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


def _native(A, b, torch, **kw):
    from cfs_spmv_amd.solver import pcg_native
    kw.setdefault("precond", "block_jacobi")
    u, it, res = pcg_native(A, torch.from_numpy(b).cuda(), **kw)
    torch.cuda.synchronize()
    return u.cpu().numpy(), it, res


def _minv(A, bs, torch):
    m = A.block_inverse(bs)
    torch.cuda.synchronize()
    return m.cpu().numpy()


# ---- 1. the inverse -----------------------------------------------------------------------------------
@DTYPES
@pytest.mark.parametrize("bs", [2, 3, 4, 6])
@pytest.mark.parametrize("name", ["rand65", "rand1026", "pwtk@0.05"])
def test_inverse_blocks_against_long_double(name, bs, dtype):
    import torch
    import cfs_spmv_amd as cfs
    n, rp, ci, va = _matrix(name)
    va = scaled(n, rp, ci, va, dtype)
    blocks = node_blocks(n, rp, ci, va, bs)
    exact = cholesky_inverse(blocks, LD)
    e_ref = _block_distance(cholesky_inverse(blocks, np.float64).astype(dtype), exact)
    A = cfs.SymMatrix(n, rp, ci, va)
    got = _minv(A, bs, torch)
    A.close()
    assert got.dtype == dtype and got.shape == exact.shape
    g = _block_distance(got, exact)
    allowed = 4 * e_ref + 16 * UNIT[dtype]
    print(f"block-inverse {np.dtype(dtype).name} {name} bs={bs} e_ref={e_ref:.3e} gpu={g:.3e} allowed={allowed:.3e}")
    assert g <= allowed
    assert np.array_equal(got, np.swapaxes(got, 1, 2)), "the two triangles differ"
    for i in range(n, exact.shape[0] * bs):  # identity outside the matrix
        assert np.array_equal(got[i // bs, i % bs], np.eye(bs, dtype=dtype)[i % bs])
        assert np.array_equal(got[i // bs, :, i % bs], np.eye(bs, dtype=dtype)[i % bs])


# ---- 2. the iterates ----------------------------------------------------------------------------------
def _check_iterates(name, n, rp, ci, va, b, dtype, bs, minv, run, label="", ks=KS):
    """run(k) -> (u_k, iterations) on the GPU; asserts every k of ks against the long-double iterate"""
    ref = block_pcg_reference(n, rp, ci, va, b, minv, ks)
    work = block_pcg_reference(n, rp, ci, va, b, minv, ks, dtype)
    errors, row = [], []
    for k in ks:
        u_ref, it_ref = ref[k]
        d = _deviation(work[k][0], u_ref)
        assert d <= D_LIMIT[dtype], f"{name}: d_{k} = {d:.3e}: badly conditioned case"
        u, it = run(k)
        g = _deviation(u, u_ref)
        allowed = 4 * d + 16 * UNIT[dtype]
        row.append(f"{d:.1e}/{g:.1e}")
        print(f"block-pcg-steps {np.dtype(dtype).name} {name}{label} bs={bs} n={n} k={k} d_k={d:.3e} gpu={g:.3e} allowed={allowed:.3e} it={it}")
        # fewer than k iterations only where the recurrence's residual can vanish: the Krylov space is exhausted
        # (after n iterations -- or after the first when a single block makes M the matrix itself)
        if not (it == k if k < n and minv.shape[0] > 1 else 1 <= it <= k):
            errors.append(f"k={k}: {it} iterations")
        if not g <= allowed:
            errors.append(f"k={k}: deviation {g:.3e} from the long-double iterate, allowed {allowed:.3e} (d_k = {d:.3e})")
    print(f"block-pcg-table   {'f64' if dtype == np.float64 else 'f32'} {name + label:<34} bs={bs}  " + "  ".join(row))
    assert not errors, f"{name}{label} bs={bs} {np.dtype(dtype).name}: " + "; ".join(errors)


CASES = [(name, 3) for name in MATRICES] + [(name, bs) for name in ("rand65", "rand1026") for bs in (2, 4, 6)]


@DTYPES
@pytest.mark.parametrize("name,bs", CASES, ids=[f"{name}-bs{bs}" for name, bs in CASES])
def test_iterates_against_the_long_double_recurrence(name, bs, dtype):
    import torch
    import cfs_spmv_amd as cfs
    n, rp, ci, va = _matrix(name)
    va, b = scaled(n, rp, ci, va, dtype), _rhs(n, dtype)
    A = cfs.SymMatrix(n, rp, ci, va)
    minv = _minv(A, bs, torch)
    _check_iterates(name, n, rp, ci, va, b, dtype, bs, minv, lambda k: _native(A, b, torch, block=bs, tol=0.0, maxiter=k)[:2])
    A.close()


@DTYPES
def test_iterates_of_a_deterministic_handle(dtype):
    import torch
    import cfs_spmv_amd as cfs
    n, rp, ci, va = _matrix("Flan_1565@0.01")
    va, b = scaled(n, rp, ci, va, dtype), _rhs(n, dtype)
    D = cfs.SymMatrix(n, rp, ci, va, options=cfs.make_options(flags=DET))
    assert D.kernel_variant()["det"] == 1
    _check_iterates("Flan_1565@0.01", n, rp, ci, va, b, dtype, 3, _minv(D, 3, torch),
                    lambda k: _native(D, b, torch, block=3, tol=0.0, maxiter=k)[:2], label=" (deterministic)")
    # ... and the whole solve is bit-reproducible
    ua, ita, _ = _native(D, b, torch, block=3, tol=0.0, maxiter=12)
    ub, itb, _ = _native(D, b, torch, block=3, tol=0.0, maxiter=12, check_every=5)
    assert ita == itb == 12 and np.array_equal(ua.view(np.uint8), ub.view(np.uint8))
    D.close()


def test_iterates_with_the_captured_graph(monkeypatch):
    """CFS_HIP_CG_GRAPH=1 on a non-null stream: two block-Jacobi iterations captured and replayed (a single
    chain of launches), plus one plain launch sequence when k is odd -- the same iterates"""
    import torch
    import cfs_spmv_amd as cfs
    dtype = np.float64
    n, rp, ci, va = _matrix("rand1023")
    va, b = scaled(n, rp, ci, va, dtype), _rhs(n, dtype)
    A = cfs.SymMatrix(n, rp, ci, va)
    minv = _minv(A, 3, torch)
    monkeypatch.setenv("CFS_HIP_CG_GRAPH", "1")
    stream = torch.cuda.Stream()
    bd = torch.from_numpy(b).cuda()

    def run(k):
        u = torch.zeros_like(bd)
        torch.cuda.synchronize()
        it, _ = A.pcg(u, bd, precond="block_jacobi", block=3, tol=0.0, maxiter=k, stream=stream)
        torch.cuda.synchronize()
        return u.cpu().numpy(), it
    _check_iterates("rand1023", n, rp, ci, va, b, dtype, 3, minv, run, label=" (captured graph)", ks=(4, 5))
    A.close()


# ---- 3. what it is for --------------------------------------------------------------------------------
def rotated_node_blocks(bs, n=20001):
    """A = H (I + 0.4 G) H: H = blockdiag(H_i), H_i^2 = Q_i diag(ev) Q_i^T a node block whose eigenvectors are
    rotated against the axes (Q_i: the Q of a standard-normal matrix), G couples dof a of node i with dof a of
    nodes i +- 1 and i +- 5, weight 0.25 each; n // bs full nodes and a trailing partial node of n % bs rows"""
    import scipy.sparse as sp
    ev = np.array((1, 30, 900, 2700, 5000, 8100), np.float64)
    rng = np.random.default_rng(11)
    m, tail = n // bs, n % bs

    def roots(count, size):  # H_i = Q_i diag(sqrt(ev)) Q_i^T
        Q = np.linalg.qr(rng.standard_normal((count, size, size)))[0]
        return np.einsum("kia,a,kja->kij", Q, np.sqrt(ev[:size]), Q)
    parts = [sp.bsr_matrix((roots(m, bs), np.arange(m), np.arange(m + 1)), shape=(m * bs, m * bs))]
    if tail:
        parts.append(roots(1, tail)[0])
    H = sp.block_diag(parts, format="csr")
    offs = [s * d for d in (bs, 5 * bs) for s in (1, -1)]
    G = sp.diags([np.full(n - abs(o), 0.25) for o in offs], offs, shape=(n, n), format="csr")
    A = (H @ (sp.identity(n) + 0.4 * G) @ H).tocsr()
    A = ((A + A.T) * 0.5).tocsr()
    A.sort_indices()
    b = np.random.default_rng(8).uniform(-1, 1, n)
    return n, A.indptr.astype(np.int32), A.indices.astype(np.int32), A.data, b


@pytest.mark.parametrize("bs,dtype", [(3, np.float64), (3, np.float32), (2, np.float64), (4, np.float64), (6, np.float64)],
                         ids=["bs3-f64", "bs3-f32", "bs2-f64", "bs4-f64", "bs6-f64"])
def test_what_the_preconditioner_is_for(bs, dtype):
    """couplings inside a node as strong as the diagonal: point Jacobi needs at least four times the iterations
    of block Jacobi.  Both counts are first established on the CPU with the working-precision recurrences (the
    block inverse there is numpy's: nothing of the library); the GPU must then reproduce the block count B
    within +-2 while cfs_hip_sym_pcg with Jacobi is still unconverged after 3 B iterations."""
    import torch
    import cfs_spmv_amd as cfs
    n, rp, ci, va, b = rotated_node_blocks(bs)
    va, b = va.astype(dtype), b.astype(dtype)
    tol = 1e-8 if dtype == np.float64 else 1e-4
    minv = cholesky_inverse(node_blocks(n, rp, ci, va, bs), np.float64).astype(dtype)
    B = block_pcg_reference(n, rp, ci, va, b, minv, dtype=dtype, tol=tol, maxiter=500)["count"]
    J = pcg_reference(n, rp, ci, va, b, dtype=dtype, tol=tol, maxiter=4 * B)["count"]
    print(f"block-pcg-steps {np.dtype(dtype).name} rotated blocks bs={bs}: block Jacobi {B} iterations, Jacobi at least {J} (CPU)")
    assert 5 <= B < 500 and J >= 4 * B, f"badly chosen case: Jacobi {J} iterations, block Jacobi {B}"
    A = cfs.SymMatrix(n, rp, ci, va)
    u, it, res = _native(A, b, torch, block=bs, tol=tol, maxiter=500)
    true, slack = _true_relres(n, rp, ci, va, b, u, dtype)
    print(f"block-pcg-steps {np.dtype(dtype).name} rotated blocks bs={bs}: GPU block Jacobi {it} iterations, relres {res:.3e} (long double {true:.3e})")
    assert res <= 10 * tol and true <= 10 * tol + slack
    assert B - 2 <= it <= B + 2, (B, it)
    uj, itj, resj = _native(A, b, torch, precond="jacobi", tol=tol, maxiter=3 * B)
    print(f"block-pcg-steps {np.dtype(dtype).name} rotated blocks bs={bs}: GPU Jacobi relres {resj:.3e} after {itj} iterations")
    assert itj == 3 * B and resj > tol
    A.close()


# ---- 4. the contract ----------------------------------------------------------------------------------
@DTYPES
def test_block_one_is_jacobi(dtype):
    """block = 1 takes cfs_hip_sym_pcg's Jacobi path: on a deterministic handle the same bits"""
    import torch
    import cfs_spmv_amd as cfs
    n, rp, ci, va = _matrix("pwtk@0.05")
    va, b = scaled(n, rp, ci, va, dtype), _rhs(n, dtype)
    tol = 1e-8 if dtype == np.float64 else 1e-4
    D = cfs.SymMatrix(n, rp, ci, va, options=cfs.make_options(flags=DET))
    for kw in (dict(tol=0.0, maxiter=7), dict(tol=tol, maxiter=500), dict(tol=tol, maxiter=500, check_every=3)):
        u1, it1, res1 = _native(D, b, torch, precond="jacobi", **kw)
        u2, it2, res2 = _native(D, b, torch, block=1, **kw)
        assert it1 == it2 > 0 and res1 == res2 and np.array_equal(u1.view(np.uint8), u2.view(np.uint8)), kw
    D.close()


@DTYPES
def test_iteration_count_and_reported_residual(dtype):
    import torch
    import cfs_spmv_amd as cfs
    n, rp, ci, va = _matrix("pwtk@0.05")
    va, b = scaled(n, rp, ci, va, dtype), _rhs(n, dtype)
    A = cfs.SymMatrix(n, rp, ci, va)
    # tol = 0: exactly maxiter iterations, whatever the window of enqueued iterations
    for check_every, k in ((1, 7), (3, 23), (16, 23), (1000, 23), (16, 40)):
        u, it, res = _native(A, b, torch, block=3, tol=0.0, maxiter=k, check_every=check_every)
        assert it == k, (check_every, k, it)
        true, slack = _true_relres(n, rp, ci, va, b, u, dtype)
        assert abs(res - true) <= slack, (k, res, true, slack)
    # maxiter = 0: u untouched, the residual of the first guess
    x0 = np.random.default_rng(4).uniform(-1, 1, n).astype(dtype)
    u, it, res = _native(A, b, torch, block=3, tol=0.0, maxiter=0, x0=torch.from_numpy(x0).cuda())
    true, slack = _true_relres(n, rp, ci, va, b, x0, dtype)
    assert it == 0 and np.array_equal(u.view(np.uint8), x0.view(np.uint8)) and abs(res - true) <= slack
    # b = 0 (and u = 0): nothing to do
    u, it, res = _native(A, np.zeros(n, dtype), torch, block=3, tol=1e-8, maxiter=50)
    assert it == 0 and not u.any() and np.isfinite(res)
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
    u1, it1, res1 = _native(D, b, torch, block=3, tol=tol, maxiter=500, check_every=1)
    assert 4 < it1 < 500 and res1 <= 10 * tol
    windows = [c for c in (3, 5, 7, 16) if it1 % c]  # the converged iteration is not the last of its window
    assert len(windows) >= 2, it1
    for check_every in windows:
        u2, it2, _ = _native(D, b, torch, block=3, tol=tol, maxiter=500, check_every=check_every)
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
        u, it, res = _native(A, b, torch, block=3, tol=1e-8, maxiter=300, check_every=check_every)
        assert it <= 1 and np.isnan(res), (it, res)
    A.close()


# ---- 5. refusals --------------------------------------------------------------------------------------
@DTYPES
@pytest.mark.parametrize("bad", ["indefinite", "nan", "no-diagonal"])
def test_a_block_that_is_not_positive_definite_is_refused(bad, dtype):
    """the block of rows 699 .. 701: CFS_HIP_ERR_ARG, u untouched, no iteration -- and the plain solver still
    takes the matrix"""
    import scipy.sparse as sp
    import torch
    import cfs_spmv_amd as cfs
    from cfs_spmv_amd import _lib
    n, rp, ci, va = _matrix("rand1023")
    L = sp.csr_matrix((va, ci, rp), shape=(n, n)).tolil()
    if bad == "indefinite":  # the sign of an in-block pair flipped, the pair enlarged beyond the diagonal
        L[700, 699] = L[699, 700] = -(abs(L[700, 699]) + 2.0 * max(L[699, 699], L[700, 700]))
    elif bad == "nan":
        L[701, 700] = L[700, 701] = 0.25  # (NaN once the matrix is scaled)
    else:
        L[700, 699] = L[699, 700] = 0.25  # (the block keeps an off-diagonal pair)
    L = L.tocsr()
    L.sort_indices()
    rp, ci, va = L.indptr.astype(np.int32), L.indices.astype(np.int32), L.data
    if bad == "no-diagonal":
        rows = np.repeat(np.arange(n), np.diff(rp))
        keep = ~((rows == 700) & (ci == 700))
        rp = np.concatenate([[0], np.cumsum(np.bincount(rows[keep], minlength=n))]).astype(np.int32)
        ci, va = ci[keep], va[keep]
    va = scaled(n, rp, ci, va, dtype)
    if bad == "nan":
        rows = np.repeat(np.arange(n), np.diff(rp))
        va[((rows == 701) & (ci == 700)) | ((rows == 700) & (ci == 701))] = np.nan
        assert np.count_nonzero(np.isnan(va)) == 2
    A = cfs.SymMatrix(n, rp, ci, va)
    x0 = np.random.default_rng(5).uniform(-1, 1, n).astype(dtype)
    u = torch.from_numpy(x0).cuda()
    b = torch.from_numpy(_rhs(n, dtype)).cuda()
    for check_every in (1, 8):
        with pytest.raises(_lib.CfsHipError, match="positive definite") as e:
            A.pcg(u, b, precond="block_jacobi", block=3, tol=1e-8, maxiter=50, check_every=check_every)
        assert e.value.code == _lib.ERR_ARG
        torch.cuda.synchronize()
        assert np.array_equal(u.cpu().numpy().view(np.uint8), x0.view(np.uint8))
    # through the raw ABI: *iterations = 0
    it, res = C.c_int(9), C.c_double(9.0)
    rc = _lib.load().cfs_hip_sym_pcg_block(A._h, u.data_ptr(), b.data_ptr(), 3, 1e-8, 50, 8, C.byref(it), C.byref(res),
                                           torch.cuda.current_stream().cuda_stream)
    assert rc == _lib.ERR_ARG and it.value == 0
    torch.cuda.synchronize()
    assert np.array_equal(u.cpu().numpy().view(np.uint8), x0.view(np.uint8))
    it2, _ = A.pcg(u, b, precond="none", tol=0.0, maxiter=2)
    assert it2 == (0 if bad == "nan" else 2)  # (a NaN residual ends the plain solve at once)
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
    kw = dict(precond="block_jacobi", block=3, tol=1e-8, maxiter=5)
    assert good.data_ptr() % 16 == 0 and big[1:n + 1].data_ptr() % 16 != 0
    for u, b in ((big[1:n + 1], good), (good, big[1:n + 1])):  # misaligned
        with pytest.raises(_lib.CfsHipError) as e:
            A.pcg(u, b, **kw)
        assert e.value.code == _lib.ERR_ARG
    with pytest.raises(_lib.CfsHipError) as e:  # one vector for both
        A.pcg(good, good, **kw)
    assert e.value.code == _lib.ERR_ARG
    host = np.zeros(n, dtype)
    for u, b in ((host, good), (good, host)):  # a host pointer
        with pytest.raises(_lib.CfsHipError) as e:
            A.pcg(u, b, **kw)
        assert e.value.code == _lib.ERR_ARG
    for block in (0, 5, 7, -1, 8):
        with pytest.raises(_lib.CfsHipError, match="block_rows") as e:
            A.pcg(good, good.clone(), precond="block_jacobi", block=block, tol=1e-8, maxiter=5)
        assert e.value.code == _lib.ERR_ARG
    # what was refused before still is
    with pytest.raises(_lib.CfsHipError, match="unknown preconditioner"):
        A.pcg(good, good.clone(), precond=2, tol=1e-8, maxiter=5)
    with pytest.raises(ValueError):
        A.pcg(good, good.clone(), precond="ilu")
    A.close()
    S = cfs.SymMatrix(n, rp, ci, va, row_splits=np.array([0, n // 2, n], np.int32), rank=1)
    M = cfs.SymMatrix(n, rp, ci, va, ngpus=2)
    for H in (S, M):
        with pytest.raises(_lib.CfsHipError) as e:
            H.pcg(good, good.clone(), **kw)
        assert e.value.code == _lib.ERR_UNSUPPORTED
        H.close()
    torch.cuda.synchronize()
    assert not good.cpu().numpy().any()


# ---- 6. the host-driven loop ----------------------------------------------------------------------------
@DTYPES
def test_host_driven_and_native_loops_agree(dtype):
    """solver.pcg(precond="block_jacobi") (torch-driven, on A.block_inverse()) against solver.pcg_native on the
    pwtk stand-in: iteration counts within +-2, both answers within the bound the Jacobi version of this test
    uses (test_gpu_pcg_steps.py)"""
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
    u1, it1, res1 = pcg(A, bd, tol=tol, maxiter=500, precond="block_jacobi", block=3)
    torch.cuda.synchronize()
    u_ref = spl.spsolve(sp.csc_matrix(sp.csr_matrix((va.astype(np.float64), ci, rp), shape=(n, n))), b.astype(np.float64))
    assert 0 < it1 < 500 and res1 <= 10 * tol
    assert np.max(np.abs(u1.cpu().numpy() - u_ref)) <= lim * np.max(np.abs(u_ref))
    for check_every in (1, 8, 1000):
        u2, it2, res2 = pcg_native(A, bd, precond="block_jacobi", block=3, tol=tol, maxiter=500, check_every=check_every)
        torch.cuda.synchronize()
        print(f"block-pcg-steps {np.dtype(dtype).name} pwtk@0.05: host-driven {it1} iterations, native {it2} (check_every={check_every})")
        assert 0 < it2 < 500 and abs(it2 - it1) <= 2, (it1, it2, check_every)
        assert res2 <= 10 * tol, (res1, res2)
        assert np.max(np.abs(u2.cpu().numpy() - u_ref)) <= lim * np.max(np.abs(u_ref))
        assert np.max(np.abs(u2.cpu().numpy() - u1.cpu().numpy())) <= 2 * lim * np.max(np.abs(u_ref))
    A.close()
