"""cfs_hip_sym_cg step by step: the ITERATES u_k of the native conjugate gradients (cg_residual_kernel,
cg_dot_kernel, cg_update_kernel, cg_direction_kernel behind the SpMV, in their BS = 0, OneColumn
instantiations) against the same recurrence in np.longdouble on the CPU,

    r = b - A u, p = r;   alpha = r.r / p.q;  u += alpha p;  r -= alpha q;  beta = r'.r' / r.r;  p = r + beta p

with the product as long-double row sums of the CSR (oracle.csr_spmv_ldx).  cg_native(..., tol=0, maxiter=k)
returns u after exactly k iterations; CG corrects itself, so the answer of a converged solve says little
about a single step, while a wrong beta, an alpha from the wrong parity slot or a stale element of p moves
u_2 by orders of magnitude more than rounding does.

Tolerance for ||u_k(GPU) - u_k(long double)||inf / ||u_k(long double)||inf: the recurrence is run a second
time on the CPU in the working precision (vectors and products in fp64 / fp32, dots accumulated in fp64, the
updates computed in fp64 and rounded, as the kernels do); d_k is its deviation from the long-double run.  A
correct GPU run differs from that CPU run only in the order of the additions inside the product and the
dots, so it is allowed 4 d_k + 16 u (u = 2^-53 / 2^-24).  Neither the reference nor d_k involves the library.
A case whose d_k exceeds 1e-6 (fp64) / 1e-2 (fp32) is badly chosen and fails.

Sizes: the vector kernels move 16 bytes per lane over n / W vectors (W = 2 / 4) and single values over the
rest, 512 x 256 threads, grid-stride: n = 1 .. 1026 cover every n mod 4, n below one vector and below one
vector per thread; n = 600 001 takes more than one grid-stride trip in both value types.

Measured on the MI355X (value type, matrix, then for k = 1, 2, 3, 5, 10: d_k / the GPU's deviation):

  f64 pwtk@0.05               1.3e-16/1.3e-16  5.9e-16/3.6e-16  3.6e-16/2.5e-16  3.6e-16/2.3e-16  3.1e-16/2.0e-16
  f32 pwtk@0.05               4.7e-08/4.7e-08  3.0e-07/1.4e-07  1.8e-07/1.0e-07  1.4e-07/1.1e-07  1.5e-07/1.3e-07
  f64 Flan_1565@0.01          2.0e-16/1.8e-16  9.1e-16/3.9e-16  3.9e-16/2.2e-16  3.6e-16/1.7e-16  3.6e-16/2.3e-16
  f32 Flan_1565@0.01          3.4e-08/3.4e-08  4.7e-07/1.7e-07  2.0e-07/9.6e-08  1.8e-07/7.7e-08  2.0e-07/1.6e-07
  f64 rand1                   0.0e+00/0.0e+00  0.0e+00/0.0e+00  0.0e+00/0.0e+00  0.0e+00/0.0e+00  0.0e+00/0.0e+00
  f32 rand1                   0.0e+00/0.0e+00  0.0e+00/0.0e+00  0.0e+00/0.0e+00  0.0e+00/0.0e+00  0.0e+00/0.0e+00
  f64 rand2                   1.9e-16/1.9e-16  1.2e-16/7.5e-17  1.7e-16/7.5e-17  1.7e-16/7.5e-17  1.7e-16/7.5e-17
  f32 rand2                   7.8e-08/7.8e-08  6.3e-08/6.3e-08  6.3e-08/6.3e-08  6.3e-08/6.3e-08  6.3e-08/6.3e-08
  f64 rand3                   7.9e-17/7.9e-17  1.9e-16/7.3e-17  2.1e-16/1.0e-16  2.1e-16/1.0e-16  2.1e-16/1.0e-16
  f32 rand3                   2.0e-08/2.0e-08  4.2e-08/4.2e-08  6.8e-08/6.8e-08  6.8e-08/6.8e-08  6.8e-08/6.8e-08
  f64 rand5                   5.9e-17/5.9e-17  1.3e-16/2.7e-16  1.2e-16/2.5e-16  1.7e-16/2.5e-16  1.7e-16/2.5e-16
  f32 rand5                   4.1e-08/4.2e-08  1.2e-07/6.9e-08  1.0e-07/6.1e-08  9.3e-08/8.9e-08  9.3e-08/8.9e-08
  f64 rand63                  7.8e-16/4.2e-16  5.6e-16/2.8e-16  4.7e-16/2.1e-16  3.2e-16/1.6e-16  3.3e-16/2.4e-16
  f32 rand63                  5.4e-08/5.4e-08  2.1e-07/8.1e-08  1.2e-07/1.2e-07  1.0e-07/8.7e-08  1.0e-07/1.6e-07
  f64 rand64                  1.6e-16/1.9e-16  1.3e-16/3.2e-16  1.4e-16/1.8e-16  1.3e-16/1.4e-16  1.5e-16/1.5e-16
  f32 rand64                  5.2e-08/5.8e-08  8.7e-08/6.6e-08  1.0e-07/6.8e-08  7.5e-08/6.8e-08  8.4e-08/8.4e-08
  f64 rand65                  2.2e-16/2.2e-16  2.5e-16/2.5e-16  2.2e-16/2.0e-16  1.6e-16/2.2e-16  3.0e-16/3.0e-16
  f32 rand65                  4.2e-08/4.2e-08  1.0e-07/7.5e-08  7.8e-08/8.1e-08  8.4e-08/6.8e-08  9.6e-08/1.0e-07
  f64 rand255                 3.7e-16/2.0e-16  2.3e-16/2.9e-16  2.8e-16/2.8e-16  1.9e-16/2.1e-16  2.6e-16/1.8e-16
  f32 rand255                 5.7e-08/5.7e-08  1.1e-07/9.3e-08  1.2e-07/1.1e-07  1.3e-07/1.0e-07  1.2e-07/1.1e-07
  f64 rand257                 8.6e-17/8.6e-17  3.6e-16/2.9e-16  3.3e-16/1.6e-16  2.6e-16/2.4e-16  2.5e-16/1.8e-16
  f32 rand257                 3.3e-08/3.2e-08  1.5e-07/1.2e-07  1.1e-07/1.0e-07  6.9e-08/6.6e-08  7.4e-08/7.0e-08
  f64 rand1023                2.8e-16/1.2e-16  4.5e-16/3.1e-16  5.9e-16/2.6e-16  5.0e-16/2.2e-16  4.1e-16/3.1e-16
  f32 rand1023                6.3e-08/5.6e-08  1.6e-07/1.4e-07  1.3e-07/1.0e-07  1.9e-07/8.5e-08  1.4e-07/1.1e-07
  f64 rand1026                7.0e-17/7.0e-17  3.2e-16/3.1e-16  3.7e-16/4.4e-16  3.2e-16/1.8e-16  2.6e-16/2.1e-16
  f32 rand1026                5.9e-08/5.9e-08  2.9e-07/2.8e-07  2.6e-07/1.2e-07  1.1e-07/9.6e-08  1.4e-07/1.2e-07
  f64 band600001              1.7e-16/2.3e-16  3.4e-16/4.2e-16  3.5e-16/3.8e-16  3.6e-16/3.8e-16  4.4e-16/4.4e-16
  f32 band600001              3.5e-08/3.5e-08  1.6e-07/1.1e-07  1.6e-07/1.2e-07  1.8e-07/1.5e-07  2.3e-07/2.3e-07
  f64 band20001 (two shards)  1.8e-16/1.8e-16  3.2e-16/3.1e-16  3.0e-16/3.3e-16  3.1e-16/3.5e-16  4.8e-16/4.2e-16
  f32 band20001 (two shards)  3.6e-08/3.6e-08  1.6e-07/1.0e-07  1.5e-07/1.3e-07  1.6e-07/1.4e-07  1.9e-07/1.8e-07

  f64 rand1023 (captured graph)  k = 4: 4.2e-16/2.5e-16  k = 5: 5.0e-16/2.2e-16
"""
import numpy as np
import pytest

from rand_matrices import banded_spd, dominant
from test_gpu_kernel_variants import PLAN_KNOBS
from test_gpu_parity import TOL

pytestmark = pytest.mark.gpu

UNIT = {np.float64: 2.0 ** -53, np.float32: 2.0 ** -24}
D_LIMIT = {np.float64: 1e-6, np.float32: 1e-2}
KS = (1, 2, 3, 5, 10)
DET = 1024
DTYPES = pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])


@pytest.fixture(autouse=True)
def _torch_first(monkeypatch):
    """torch brings a HIP runtime of its own: it has to initialise before libcfs_hip.so's"""
    import torch
    torch.cuda.init()
    torch.cuda.set_device(0)
    for k in PLAN_KNOBS + ("CFS_HIP_CG_GRAPH",):
        monkeypatch.delenv(k, raising=False)
    yield


def cg_reference(n, rp, ci, va, b, ks, dtype=None, x0=None):
    """{k: (u_k, iterations done)} of the recurrence above from u = x0 (0), with the kernels' guards
    (alpha = 0 when p.q = 0, beta = 0 when r.r = 0, nothing more once r.r is not > 0).
    dtype None: np.longdouble throughout.  Otherwise the working precision of the kernels: vectors and
    the product in `dtype`, dots accumulated in fp64, updates computed in fp64 and rounded to `dtype`."""
    import scipy.sparse as sp
    from oracle import oracle
    ld = dtype is None
    W, S = (np.longdouble, np.longdouble) if ld else (dtype, np.float64)
    if ld:
        def mv(x):
            return oracle.csr_spmv_ldx(n, rp, ci, va, x)
    else:
        A = sp.csr_matrix((va.astype(dtype), ci, rp), shape=(n, n))

        def mv(x):
            return (A @ x).astype(dtype)
    u = np.zeros(n, W) if x0 is None else x0.astype(W)
    r = (b.astype(S) - mv(u).astype(S)).astype(W)
    p = r.copy()
    rr = np.dot(r.astype(S), r.astype(S))
    out, it, done = {}, 0, not (rr > 0)
    for k in range(0, max(ks) + 1):
        if k > 0 and not done:
            q = mv(p)
            pq = np.dot(p.astype(S), q.astype(S))
            alpha = rr / pq if pq != 0 else S(0)
            u = (u.astype(S) + alpha * p.astype(S)).astype(W)
            rs = r.astype(S) - alpha * q.astype(S)
            rrn = np.dot(rs, rs)
            r = rs.astype(W)
            beta = rrn / rr if rr != 0 else S(0)
            p = (r.astype(S) + beta * p.astype(S)).astype(W)
            rr, it, done = rrn, it + 1, not (rrn > 0)
        if k in ks:
            out[k] = (u.copy(), it)
    return out


def _deviation(u, ref):
    ref = ref.astype(np.longdouble)
    return float(np.max(np.abs(u.astype(np.longdouble) - ref)) / np.max(np.abs(ref)))


def _rhs(n, dtype):
    return np.random.default_rng(n).uniform(-1, 1, n).astype(dtype)


def _matrix(name):
    from cfs_spmv_amd import synth
    if name.startswith("rand"):
        n = int(name[4:])
        return dominant(*synth.random_symmetric(n, 3, seed=100 + n))
    if name.startswith("band"):
        return banded_spd(int(name[4:]), 3, 1)
    stand_in, scale = name.split("@")
    return synth.generate(stand_in, float(scale))[:4]


def _native(A, b, torch, **kw):
    from cfs_spmv_amd.solver import cg_native
    u, it, res = cg_native(A, torch.from_numpy(b).cuda(), **kw)
    torch.cuda.synchronize()
    return u.cpu().numpy(), it, res


def _check_iterates(name, n, rp, ci, va, b, dtype, run, label=""):
    """run(k) -> (u_k, iterations) on the GPU; asserts every k of KS against the long-double iterate"""
    ref = cg_reference(n, rp, ci, va, b, KS)
    work = cg_reference(n, rp, ci, va, b, KS, dtype)
    errors = []
    for k in KS:
        u_ref, it_ref = ref[k]
        d = _deviation(work[k][0], u_ref)
        assert d <= D_LIMIT[dtype], f"{name}: d_{k} = {d:.3e}: badly conditioned case"
        u, it = run(k)
        g = _deviation(u, u_ref)
        allowed = 4 * d + 16 * UNIT[dtype]
        print(f"cg-steps {np.dtype(dtype).name} {name}{label} n={n} k={k} d_k={d:.3e} gpu={g:.3e} allowed={allowed:.3e} it={it}")
        # fewer than k iterations only where the recurrence's residual can vanish: the Krylov space is exhausted
        if not (it == k if k < n else 1 <= it <= k):
            errors.append(f"k={k}: {it} iterations")
        if not g <= allowed:
            errors.append(f"k={k}: deviation {g:.3e} from the long-double iterate, allowed {allowed:.3e} (d_k = {d:.3e})")
    assert not errors, f"{name}{label} {np.dtype(dtype).name}: " + "; ".join(errors)


MATRICES = ["pwtk@0.05", "Flan_1565@0.01"] + [f"rand{n}" for n in (1, 2, 3, 5, 63, 64, 65, 255, 257, 1023, 1026)] + \
           ["band600001"]


@DTYPES
@pytest.mark.parametrize("name", MATRICES)
def test_iterates_against_the_long_double_recurrence(name, dtype):
    import torch
    import cfs_spmv_amd as cfs
    n, rp, ci, va = _matrix(name)
    va, b = va.astype(dtype), _rhs(n, dtype)
    A = cfs.SymMatrix(n, rp, ci, va)
    assert A.stats()["n"] == n and A.row_end - A.row_begin == n
    _check_iterates(name, n, rp, ci, va, b, dtype, lambda k: _native(A, b, torch, tol=0.0, maxiter=k)[:2])
    A.close()


@DTYPES
def test_iterates_through_a_two_shard_handle(dtype):
    """an odd n through a multi-device handle (two shards, here on one device): the products on the shards'
    streams, the vector kernels on the caller's"""
    import torch
    import cfs_spmv_amd as cfs
    n, rp, ci, va = _matrix("band20001")
    va, b = va.astype(dtype), _rhs(n, dtype)
    M = cfs.SymMatrix(n, rp, ci, va, ngpus=2)
    _check_iterates("band20001", n, rp, ci, va, b, dtype, lambda k: _native(M, b, torch, tol=0.0, maxiter=k)[:2],
                    label=" (two shards)")
    M.close()


def test_iterates_with_the_captured_graph(monkeypatch):
    """CFS_HIP_CG_GRAPH=1 on a non-null stream: two iterations captured and replayed (a single chain of
    launches), plus one plain iteration when k is odd -- the same iterates"""
    import torch
    import cfs_spmv_amd as cfs
    dtype = np.float64
    n, rp, ci, va = _matrix("rand1023")
    b = _rhs(n, dtype)
    A = cfs.SymMatrix(n, rp, ci, va)
    monkeypatch.setenv("CFS_HIP_CG_GRAPH", "1")
    stream = torch.cuda.Stream()
    bd = torch.from_numpy(b).cuda()
    ref = cg_reference(n, rp, ci, va, b, (4, 5))
    work = cg_reference(n, rp, ci, va, b, (4, 5), dtype)
    for k in (4, 5):
        u = torch.zeros_like(bd)
        torch.cuda.synchronize()
        it, _ = A.cg(u, bd, tol=0.0, maxiter=k, stream=stream)
        torch.cuda.synchronize()
        d, g = _deviation(work[k][0], ref[k][0]), _deviation(u.cpu().numpy(), ref[k][0])
        print(f"cg-steps float64 rand1023 (graph) n={n} k={k} d_k={d:.3e} gpu={g:.3e}")
        assert it == k and g <= 4 * d + 16 * UNIT[dtype], (k, it, d, g)
    A.close()


def _true_relres(n, rp, ci, va, b, u, dtype):
    """(||b - A u|| / ||b|| in long double, the bound on what the library may report instead): the suite's
    product tolerance against the row scale, plus the rounding of the subtraction"""
    from oracle import oracle
    _, absrow = oracle.csr_spmv_ld(n, rp, ci, va, u)
    au = oracle.csr_spmv_ldx(n, rp, ci, va, u)
    bl = b.astype(np.longdouble)
    nb = np.sqrt(np.dot(bl, bl))
    res = bl - au
    slack = (TOL[dtype] * np.sqrt(np.dot(absrow, absrow)) + UNIT[dtype] * np.sqrt(np.sum((np.abs(bl) + np.abs(au)) ** 2))) / nb
    return float(np.sqrt(np.dot(res, res)) / nb), float(slack)


@DTYPES
def test_iteration_count_and_reported_residual(dtype):
    import torch
    import cfs_spmv_amd as cfs
    n, rp, ci, va = _matrix("pwtk@0.05")
    va, b = va.astype(dtype), _rhs(n, dtype)
    A = cfs.SymMatrix(n, rp, ci, va)
    # tol = 0: exactly maxiter iterations, whatever the window of enqueued iterations
    for check_every, k in ((1, 7), (3, 23), (16, 23), (1000, 23), (16, 40)):
        u, it, res = _native(A, b, torch, tol=0.0, maxiter=k, check_every=check_every)
        assert it == k, (check_every, k, it)
        true, slack = _true_relres(n, rp, ci, va, b, u, dtype)
        print(f"cg-steps {np.dtype(dtype).name} relres k={k} reported={res:.6e} long double={true:.6e} slack={slack:.3e}")
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
    va, b = va.astype(dtype), _rhs(n, dtype)
    tol = 1e-8 if dtype == np.float64 else 1e-4
    D = cfs.SymMatrix(n, rp, ci, va, options=cfs.make_options(flags=DET))
    u1, it1, res1 = _native(D, b, torch, tol=tol, maxiter=500, check_every=1)
    assert 16 < it1 < 500 and res1 <= 10 * tol
    windows = [c for c in (3, 5, 7, 16) if it1 % c]  # the converged iteration is not the last of its window
    assert len(windows) >= 2 and 16 in windows, it1
    for check_every in windows:
        u2, it2, _ = _native(D, b, torch, tol=tol, maxiter=500, check_every=check_every)
        assert it2 == it1 and np.array_equal(u2.view(np.uint8), u1.view(np.uint8)), (check_every, it1, it2)
    D.close()


@DTYPES
def test_breakdown_and_nan(dtype):
    import torch
    import cfs_spmv_amd as cfs
    # indefinite: p.q = 0 exactly in the first iteration and in every later one (alpha = 0, beta = 1)
    n = 6
    rp, ci = np.arange(n + 1, dtype=np.int32), np.arange(n, dtype=np.int32)
    va = np.array([1, -1, 1, 1, 1, 1], dtype)
    A = cfs.SymMatrix(n, rp, ci, va)
    b = np.array([1, 1, 0, 0, 0, 0], dtype)
    u, it, res = _native(A, b, torch, tol=1e-12, maxiter=20)
    assert it == 20 and np.all(np.isfinite(u)) and not u.any() and res == 1.0
    A.close()
    # a NaN in b ends the solve at once: it must not run on to maxiter
    n, rp, ci, va = _matrix("rand1023")
    va, b = va.astype(dtype), _rhs(n, dtype)
    b[n // 2] = np.nan
    A = cfs.SymMatrix(n, rp, ci, va)
    for check_every in (1, 16):
        u, it, res = _native(A, b, torch, tol=1e-8, maxiter=300, check_every=check_every)
        assert it <= 1 and np.isnan(res), (it, res)
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
            A.cg(u, b, tol=1e-8, maxiter=5)
        assert e.value.code == _lib.ERR_ARG
    A.close()
    S = cfs.SymMatrix(n, rp, ci, va, row_splits=np.array([0, n // 2, n], np.int32), rank=1)
    with pytest.raises(_lib.CfsHipError) as e:
        S.cg(good, good.clone(), tol=1e-8, maxiter=5)
    assert e.value.code == _lib.ERR_UNSUPPORTED
    S.close()
