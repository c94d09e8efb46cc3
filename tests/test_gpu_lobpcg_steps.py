"""The kernels of cfs_hip_sym_lobpcg one by one, on the GPU: the Gram kernel (cfs_hip_debug_gram) against long double, the
update kernel alone (cfs_hip_debug_lobpcg_update), and iteration 0 plus one and two more iterations of the solver's own
kernels (cfs_hip_sym_debug_lobpcg) against a long-double restatement of the same iterations.

Gram.  G = S^T S and H = S^T T of uniform(-1, 1) blocks in the value type, every n of GRAM_N (the vector tail, a
partial LDS row tile, one grid-stride sweep of 512 workgroups and beyond) with every m of GRAM_M (a single pair, a
partial 4 x 4 register block, the cap of 48 columns; n = 600001: m = 3 and 12 only), ld = n rounded up to 16 bytes and
that plus 16 bytes.  Every entry must lie within

    (n 2^-53 + 2^-53) sum_r |s_ri| |t_rj|        (the sum evaluated in long double)

of the long-double value: the a-priori bound of a sum of n products accumulated in fp64 in ANY order -- the inputs are
the stored values, whose conversion to fp64 is exact.  G must be symmetric bit for bit, two calls must give equal bits,
and integer-valued blocks (entries -8 .. 8, n <= 2^18, every partial sum below 2^53) must give the exact integers.

Update.  m = 3 k columns and a C with one nonzero, 1.0, per column: X and P must reproduce the chosen input columns bit
for bit, in place (0 + 1.0 a + 0 b ... is exact), whichever columns they overwrite, and W must stay as it was.

Iterations.  theta and the residual norms after iteration 0 and `iters` = 1, 2 more, k = 1 and 4, block_rows = 0, 1, 3,
on rand257, rand1023, band20001 and lap2d(16, 15), compared with a restatement in long double (Gram matrices, update,
residual and preconditioner in long double, what the library stores rounded to the value type, the Rayleigh-Ritz step by
solver.lobpcg_rr in numpy) -- not the vectors: Rayleigh-Ritz is free in sign and rotation.  The inverse diagonal and
inverse blocks are the handle's own (SymMatrix.diagonal / block_inverse, pinned by the PCG tests).  The deviation

    d = max(max_i |theta_i - theta_i^ref|, max_i |r_i - r_i^ref|) / max_i |theta_i^ref|

is what the fp64 / long-double difference of G and H (and of the products) moves them by.  It is measured for
solver.lobpcg, the host-driven torch model of the same recurrence, on the same case in both value types, by the test
itself; the native loop is allowed 4 x the larger of the two.  Measured on the MI355X (case: model f64, model f32, native
f64, native f32):

  rand257 k=1 block_rows=0 iters=1: 3.535e-16, 6.611e-09, 1.414e-15, 6.611e-09
  rand257 k=1 block_rows=0 iters=2: 5.746e-16, 1.472e-08, 4.596e-16, 1.472e-08
  rand257 k=1 block_rows=1 iters=1: 6.648e-16, 8.295e-09, 3.989e-16, 8.295e-09
  rand257 k=1 block_rows=1 iters=2: 6.493e-16, 7.031e-09, 2.783e-16, 7.031e-09
  rand257 k=1 block_rows=3 iters=1: 5.319e-16, 1.090e-08, 5.319e-16, 1.090e-08
  rand257 k=1 block_rows=3 iters=2: 9.281e-16, 7.740e-09, 3.713e-16, 7.740e-09
  rand257 k=4 block_rows=0 iters=1: 5.953e-15, 7.863e-08, 2.528e-15, 7.863e-08
  rand257 k=4 block_rows=0 iters=2: 1.628e-15, 3.035e-08, 1.085e-15, 3.035e-08
  rand257 k=4 block_rows=1 iters=1: 2.496e-15, 2.247e-08, 1.070e-15, 2.247e-08
  rand257 k=4 block_rows=1 iters=2: 2.072e-15, 7.959e-09, 1.813e-15, 7.959e-09
  rand257 k=4 block_rows=3 iters=1: 1.550e-15, 4.135e-08, 1.907e-15, 4.135e-08
  rand257 k=4 block_rows=3 iters=2: 1.900e-15, 2.068e-08, 1.425e-15, 2.068e-08
  rand1023 k=1 block_rows=0 iters=1: 1.929e-15, 1.668e-08, 3.216e-16, 1.668e-08
  rand1023 k=1 block_rows=0 iters=2: 1.250e-15, 8.552e-09, 2.083e-16, 8.552e-09
  rand1023 k=1 block_rows=1 iters=1: 1.185e-15, 1.745e-08, 2.370e-16, 1.745e-08
  rand1023 k=1 block_rows=1 iters=2: 1.685e-15, 7.269e-09, 2.527e-16, 7.269e-09
  rand1023 k=1 block_rows=3 iters=1: 9.495e-16, 2.212e-08, 7.121e-16, 2.212e-08
  rand1023 k=1 block_rows=3 iters=2: 5.905e-16, 5.160e-09, 3.374e-16, 5.160e-09
  rand1023 k=4 block_rows=0 iters=1: 2.553e-15, 3.316e-08, 7.179e-15, 3.316e-08
  rand1023 k=4 block_rows=0 iters=2: 3.013e-15, 3.243e-08, 2.286e-15, 3.243e-08
  rand1023 k=4 block_rows=1 iters=1: 2.330e-15, 1.686e-09, 9.985e-16, 1.686e-09
  rand1023 k=4 block_rows=1 iters=2: 1.869e-15, 1.382e-08, 1.168e-15, 1.382e-08
  rand1023 k=4 block_rows=3 iters=1: 2.331e-15, 9.493e-09, 8.882e-16, 9.493e-09
  rand1023 k=4 block_rows=3 iters=2: 1.714e-15, 1.725e-08, 7.790e-16, 1.725e-08
  band20001 k=1 block_rows=0 iters=1: 6.102e-15, 2.175e-09, 0.000e+00, 2.175e-09
  band20001 k=1 block_rows=0 iters=2: 3.144e-15, 3.313e-09, 2.515e-16, 3.313e-09
  band20001 k=1 block_rows=1 iters=1: 4.717e-15, 1.008e-09, 2.816e-16, 1.008e-09
  band20001 k=1 block_rows=1 iters=2: 6.824e-16, 1.599e-09, 3.412e-16, 1.599e-09
  band20001 k=1 block_rows=3 iters=1: 4.544e-15, 5.487e-10, 1.466e-16, 5.487e-10
  band20001 k=1 block_rows=3 iters=2: 5.023e-15, 2.080e-09, 5.382e-16, 2.079e-09
  band20001 k=4 block_rows=0 iters=1: 4.886e-15, 2.103e-09, 1.720e-15, 2.146e-09
  band20001 k=4 block_rows=0 iters=2: 5.856e-14, 6.341e-09, 1.065e-14, 7.991e-09
  band20001 k=4 block_rows=1 iters=1: 8.882e-15, 1.803e-09, 2.518e-15, 1.821e-09
  band20001 k=4 block_rows=1 iters=2: 7.281e-15, 1.914e-09, 1.355e-15, 1.533e-09
  band20001 k=4 block_rows=3 iters=1: 7.712e-15, 1.276e-09, 1.019e-15, 1.270e-09
  band20001 k=4 block_rows=3 iters=2: 6.841e-15, 2.971e-09, 2.132e-15, 2.974e-09
  lap2d16x15 k=1 block_rows=0 iters=1: 3.352e-16, 8.592e-09, 1.676e-16, 8.592e-09
  lap2d16x15 k=1 block_rows=0 iters=2: 6.428e-16, 1.322e-08, 3.857e-16, 1.322e-08
  lap2d16x15 k=1 block_rows=1 iters=1: 8.380e-16, 1.147e-09, 3.352e-16, 1.147e-09
  lap2d16x15 k=1 block_rows=1 iters=2: 1.543e-15, 1.006e-08, 6.428e-16, 1.006e-08
  lap2d16x15 k=1 block_rows=3 iters=1: 8.137e-16, 8.515e-09, 4.069e-16, 8.515e-09
  lap2d16x15 k=1 block_rows=3 iters=2: 1.070e-15, 1.061e-08, 5.352e-16, 1.061e-08
  lap2d16x15 k=4 block_rows=0 iters=1: 2.178e-15, 2.021e-08, 5.807e-16, 2.021e-08
  lap2d16x15 k=4 block_rows=0 iters=2: 1.749e-15, 5.214e-08, 1.312e-15, 5.214e-08
  lap2d16x15 k=4 block_rows=1 iters=1: 1.452e-15, 2.281e-08, 6.533e-16, 2.281e-08
  lap2d16x15 k=4 block_rows=1 iters=2: 1.530e-15, 3.651e-08, 1.312e-15, 3.651e-08
  lap2d16x15 k=4 block_rows=3 iters=1: 1.041e-15, 2.038e-08, 1.388e-15, 2.038e-08
  lap2d16x15 k=4 block_rows=3 iters=2: 2.561e-15, 4.282e-08, 1.440e-15, 4.282e-08

and the Gram kernel's worst error over its bound, per n:

  float64 n=1: worst error / bound 0.495
  float32 n=1: worst error / bound 0.000
  float64 n=2: worst error / bound 0.545
  float32 n=2: worst error / bound 0.300
  float64 n=63: worst error / bound 0.055
  float32 n=63: worst error / bound 0.048
  float64 n=65: worst error / bound 0.069
  float32 n=65: worst error / bound 0.072
  float64 n=257: worst error / bound 0.019
  float32 n=257: worst error / bound 0.026
  float64 n=1023: worst error / bound 0.002
  float32 n=1023: worst error / bound 0.002
  float64 n=20001: worst error / bound 0.000
  float32 n=20001: worst error / bound 0.000
  float64 n=600001: worst error / bound 0.000
  float32 n=600001: worst error / bound 0.000
"""
import ctypes as C
import functools

import numpy as np
import pytest

from test_gpu_cg_steps import DTYPES, UNIT, _matrix
from test_gpu_kernel_variants import PLAN_KNOBS

pytestmark = pytest.mark.gpu

GRAM_N = [1, 2, 63, 65, 257, 1023, 20001, 600001]
GRAM_M = [1, 2, 3, 8, 9, 12, 47, 48]
LD = np.longdouble


@pytest.fixture(autouse=True)
def _torch_first(monkeypatch):
    """torch brings a HIP runtime of its own: it has to initialise before libcfs_hip.so's"""
    import torch
    torch.cuda.init()
    torch.cuda.set_device(0)
    for k in PLAN_KNOBS:
        monkeypatch.delenv(k, raising=False)
    yield


def lap2d(nx, ny):
    """1 kron(I, T_nx) + 0.37 kron(T_ny, I), T = tridiag(-1, 2, -1)"""
    import scipy.sparse as sp
    T = lambda n: sp.diags([-np.ones(n - 1), 2 * np.ones(n), -np.ones(n - 1)], [-1, 0, 1])
    A = (sp.kron(sp.identity(ny), T(nx)) + 0.37 * sp.kron(T(ny), sp.identity(nx))).tocsr()
    A.sort_indices()
    return A.shape[0], A.indptr.astype(np.int32), A.indices.astype(np.int32), A.data


def matrix(name):
    if name.startswith("lap2d"):
        return lap2d(*(int(x) for x in name[5:].split("x")))
    return _matrix(name)


def _tdt(dtype):
    import torch
    return torch.float64 if dtype == np.float64 else torch.float32


def _block(host, ld):
    """a device block with strides (1, ld) holding the (n, m) numpy array"""
    import torch
    n, m = host.shape
    buf = torch.zeros(m * ld, dtype=_tdt(host.dtype.type), device="cuda")
    view = torch.as_strided(buf, (n, m), (1, ld))
    view.copy_(torch.from_numpy(np.array(host)))
    return buf, view


def gram_gpu(S, T, m, ld):
    import torch
    import cfs_spmv_amd as cfs
    from cfs_spmv_amd import _lib
    n = S.shape[0]
    sb, _ = _block(S[:, :m], ld)
    tb, _ = _block(T[:, :m], ld)
    g, hh = np.full((m, m), np.nan), np.full((m, m), np.nan)
    dp = C.POINTER(C.c_double)
    _lib.check(cfs.load().cfs_hip_debug_gram(sb.data_ptr(), tb.data_ptr(), ld, n, m, S.dtype.itemsize, g.ctypes.data_as(dp),
                                             hh.ctypes.data_as(dp), torch.cuda.current_stream().cuda_stream))
    return g, hh


@functools.lru_cache(maxsize=None)
def _gram_case(n, dtype):
    """(S, T, and in long double S^T S, S^T T, |S|^T |S|, |S|^T |T|) for the widest m of this n; the leading m x m blocks
    are the references of the narrower ones.  Computed once, shared, unchanged"""
    m = 12 if n > 100000 else 48
    rng = np.random.default_rng(1000 + n)
    S, T = rng.uniform(-1, 1, (n, m)).astype(dtype), rng.uniform(-1, 1, (n, m)).astype(dtype)
    Sl, Tl = S.astype(LD), T.astype(LD)
    out = S, T, Sl.T @ Sl, Sl.T @ Tl, np.abs(Sl).T @ np.abs(Sl), np.abs(Sl).T @ np.abs(Tl)
    for x in out:
        x.setflags(write=False)
    return out


@DTYPES
@pytest.mark.parametrize("n", GRAM_N)
def test_gram_against_long_double(n, dtype):
    S, T, G_ref, H_ref, G_abs, H_abs = _gram_case(n, dtype)
    per = 16 // np.dtype(dtype).itemsize
    ld0 = -(-n // per) * per
    errors, worst = [], 0.0
    for m in ([3, 12] if n > 100000 else GRAM_M):
        for ld in (ld0, ld0 + per):
            g, hh = gram_gpu(S, T, m, ld)
            if not np.array_equal(g.view(np.uint64), g.T.copy().view(np.uint64)):
                errors.append(f"m={m} ld={ld}: G is not symmetric bit for bit")
            g2, hh2 = gram_gpu(S, T, m, ld)
            if not (np.array_equal(g.view(np.uint64), g2.view(np.uint64)) and np.array_equal(hh.view(np.uint64), hh2.view(np.uint64))):
                errors.append(f"m={m} ld={ld}: two calls differ")
            for what, got, ref, ab in (("G", g, G_ref, G_abs), ("H", hh, H_ref, H_abs)):
                bound = (n * 2.0 ** -53 + 2.0 ** -53) * ab[:m, :m]
                err = np.abs(got.astype(LD) - ref[:m, :m])
                with np.errstate(invalid="ignore"):
                    worst = max(worst, float(np.max(err / bound)))
                if not np.all(err <= bound):
                    i, j = np.unravel_index(np.argmax(err - bound), err.shape)
                    errors.append(f"m={m} ld={ld}: {what}[{i},{j}] = {got[i, j]!r}, long double {float(ref[i, j])!r}, off by "
                                  f"{float(err[i, j]):.3e}, bound {float(bound[i, j]):.3e}")
    print(f"gram {np.dtype(dtype).name} n={n}: worst error / bound {worst:.3f}")
    assert not errors, f"n={n} {np.dtype(dtype).name}: " + "; ".join(errors[:8])


@DTYPES
@pytest.mark.parametrize("n,m", [(1, 1), (65, 9), (20001, 48), (1 << 18, 12)])
def test_gram_of_integers_is_exact(n, m, dtype):
    rng = np.random.default_rng(n + m)
    S, T = rng.integers(-8, 9, (n, m)).astype(dtype), rng.integers(-8, 9, (n, m)).astype(dtype)
    per = 16 // np.dtype(dtype).itemsize
    g, hh = gram_gpu(S, T, m, -(-n // per) * per)
    Si, Ti = S.astype(np.int64), T.astype(np.int64)
    assert np.array_equal(g, (Si.T @ Si).astype(np.float64)) and np.array_equal(hh, (Si.T @ Ti).astype(np.float64))


@DTYPES
@pytest.mark.parametrize("n,k", [(1, 1), (63, 1), (65, 4), (257, 16), (20001, 3), (600001, 2)])
def test_update_with_a_selection_reproduces_the_columns_in_place(n, k, dtype):
    import torch
    import cfs_spmv_amd as cfs
    from cfs_spmv_amd import _lib
    m = 3 * k
    rng = np.random.default_rng(n + k)
    S = rng.uniform(-1, 1, (n, m)).astype(dtype)
    per = 16 // np.dtype(dtype).itemsize
    ld = -(-n // per) * per + per
    buf, view = _block(S, ld)
    buf[n::ld] = 7  # (the word behind the rows of every column)
    # X_o <- column pick[o], P_o <- column pick[k + o]: a permutation that moves X, W and P columns into X and P
    pick = rng.permutation(m)[:2 * k]
    c = np.zeros((m, 2 * k))
    c[pick, np.arange(2 * k)] = 1.0
    _lib.check(cfs.load().cfs_hip_debug_lobpcg_update(buf.data_ptr(), ld, n, k, m, c.ctypes.data_as(C.POINTER(C.c_double)),
                                                      np.dtype(dtype).itemsize, torch.cuda.current_stream().cuda_stream))
    out = view.cpu().numpy()
    bits = np.uint64 if dtype == np.float64 else np.uint32
    expect = S.copy()
    expect[:, :k], expect[:, 2 * k:] = S[:, pick[:k]], S[:, pick[k:]]
    assert np.array_equal(np.ascontiguousarray(out).view(bits), np.ascontiguousarray(expect).view(bits))
    pad = buf.cpu().numpy()[n::ld]
    assert pad.shape == (m,) and np.all(pad == 7), "nothing outside rows [0, n) is written"


# ---- iterations against a long-double restatement ----------------------------------------------------------------
def _round(x, dtype):
    return x.astype(dtype).astype(LD)


def reference_iterations(n, rp, ci, va, dtype, k, block_rows, minv, x0, iters):
    """iteration 0 and `iters` more of the recurrence documented in cfs_hip.h, every pair active, in long double; the
    blocks hold values of `dtype`.  minv: None, the stored inverse diagonal (n,) or the stored inverse blocks (nb, bs, bs).
    Returns (theta, resnorms) after the last iteration."""
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
        if block_rows == 0:
            W = R
        elif block_rows == 1:
            W = R * minv.astype(LD)[None, :]
        else:
            nb, bs, _ = minv.shape
            Rp = np.zeros((k, nb * bs), LD)
            Rp[:, :n] = R
            W = np.einsum("bij,kbj->kbi", minv.astype(LD), Rp.reshape(k, nb, bs)).reshape(k, nb * bs)[:, :n]
        S[k:2 * k] = _round(W, dtype)
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


def _deviation(theta, res, ref):
    return float(max(np.max(np.abs(theta - ref[0])), np.max(np.abs(res - ref[1]))) / np.max(np.abs(ref[0])))


@functools.lru_cache(maxsize=None)
def _iteration_case(name, k, block_rows, iters):
    """per value type: (the native loop's deviation from the long-double iterations, the torch model's).  One handle per
    value type, one reference each; computed once for the case"""
    import torch
    import cfs_spmv_amd as cfs
    from cfs_spmv_amd import solver
    n, rp, ci, va = matrix(name)
    out = {}
    for dtype in (np.float64, np.float32):
        vd = np.asarray(va).astype(dtype)
        A = cfs.SymMatrix(n, rp, ci, vd)
        minv = None
        if block_rows == 1:
            d = A.diagonal().cpu().numpy()
            minv = (1.0 / d.astype(np.float64)).astype(dtype)
        elif block_rows > 1:
            minv = A.block_inverse(block_rows).cpu().numpy()
        x0 = solver.default_x0(n, k, dtype)
        ref = reference_iterations(n, rp, ci, vd, dtype, k, block_rows, minv, x0, iters)
        theta, X, res = A.debug_lobpcg(k, block_rows, iters)
        torch.cuda.synchronize()
        assert X.shape == (n, k) and bool(torch.all(torch.isfinite(X)))
        precond = {0: "none", 1: "jacobi"}.get(block_rows, "block_jacobi")
        wm, Xm, im = solver.lobpcg(A, k, precond=precond, block=block_rows, iters=iters)
        A.close()
        out[dtype] = (_deviation(theta, res, ref), _deviation(wm, im["residuals"], ref), ref)
    return out


@DTYPES
@pytest.mark.parametrize("iters", [1, 2])
@pytest.mark.parametrize("block_rows", [0, 1, 3])
@pytest.mark.parametrize("k", [1, 4])
@pytest.mark.parametrize("name", ["rand257", "rand1023", "band20001", "lap2d16x15"])
def test_iterations_against_the_long_double_recurrence(name, k, block_rows, iters, dtype):
    case = _iteration_case(name, k, block_rows, iters)
    native, model = case[dtype][0], max(case[np.float64][1], case[np.float32][1])
    print(f"lobpcg-steps {name} k={k} block_rows={block_rows} iters={iters}: model f64 {case[np.float64][1]:.3e}, model f32 "
          f"{case[np.float32][1]:.3e}, native f64 {case[np.float64][0]:.3e}, native f32 {case[np.float32][0]:.3e}")
    ref = case[dtype][2]
    assert np.all(np.isfinite(ref[0])) and np.all(np.diff(ref[0]) >= 0)
    assert native <= 4 * model, f"{name} {np.dtype(dtype).name}: deviation {native:.3e}, allowed 4 x {model:.3e}"
