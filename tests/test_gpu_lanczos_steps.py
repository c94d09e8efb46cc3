"""The Lanczos step of cfs_hip_sym_eigs through cfs_hip_sym_debug_lanczos (the solver's own kernels: eigs_start_kernel and
eigs_normalise_kernel once, then eigs_project_kernel, eigs_reduce_kernel, eigs_subtract_kernel twice each and
eigs_scale_kernel behind the SpMV), by the method of test_gpu_minres_steps.py: the recurrence

    v_1 = v0 / ||v0||
    q = A v_j;  c = V_j^T q;  qq = q.q;  q1 = q - sum_k c_k v_k (k ascending);  c' = V_j^T q1;  q2 = q1 - sum_k c'_k v_k
    alpha_j = c_j + c'_j;  beta_j = sqrt(q2.q2);  breakdown iff !(beta_j > 16 u sqrt(qq));  v_{j+1} = q2 / beta_j, or 0

is run twice on the CPU: in np.longdouble with the product as long-double row sums of the CSR (oracle.csr_spmv_ldx), and
in the working precision with the kernels' rounding rules -- the basis, q, q1, q2 stored in fp64 / fp32, every dot
product and scalar in fp64, q1, q2 and v_{j+1} computed in fp64 and rounded once when stored.  Neither involves the
library.  The start vector is default_rng(n).uniform(-1, 1, n) in the value type.

alpha_j, beta_j for j <= 3 (relative to ||A||inf) and v_2 (relative to its largest entry) are compared with the
long-double run: with d the working-precision model's own deviation of the same quantity, the GPU -- which differs from
that model only in the order of the additions inside the product and the dots -- is allowed 4 d + 16 u (u = 2^-53 /
2^-24).  Later Lanczos vectors are not compared as iterates: a Krylov basis is an ill-conditioned function of its data.
Two invariants are checked instead, computed here in long double from the returned basis, alpha and beta, at j in
{1, 2, 3, 5, 10, 20} (those not above the steps made):

    omega_j = max |V^T V - I| over v_1 .. v_{j+1}
    rho_j   = max_{i <= j} ||A v_i - (beta_{i-1} v_{i-1} + alpha_i v_i + beta_i v_{i+1})||inf / ||A||inf

The GPU is allowed 4 x the working-precision model's value + 16 u.

Deep bases: cfs_hip_sym_debug_lanczos admits 128 steps (CFS_HIP_EIGS_MAX_NCV), and the cases above stop at 20.  rand257,
rand1023 and band20001 are run for 128 steps as well -- the project kernel walks 16 chunks of 8 accumulators, the reduce
kernel launches 129 workgroups, the subtract kernel's coefficient array is full and the last flag word sits next to the
first coefficient word -- with the same rule and omega_j, rho_j at j in {20, 40, 64, 65, 100, 127, 128} in addition.  None
of the three breaks down in 128 steps in either precision on the CPU (the smallest beta is 1.06 to 2.1).

Measured on the MI355X (value type, matrix: the largest over the compared quantities of d / the GPU's deviation; then
the largest over j of the model's omega / the GPU's omega and of the model's rho / the GPU's rho):

  f64 rand2 n=2 steps=1: d=7.6e-17/gpu=9.7e-17  omega 1.3e-16/1.3e-16  rho 3.6e-17/3.5e-17
  f32 rand2 n=2 steps=1: d=5.3e-08/gpu=5.3e-08  omega 5.7e-08/5.7e-08  rho 5.9e-08/5.9e-08
  f64 rand3 n=3 steps=2: d=1.2e-15/gpu=6.0e-16  omega 1.2e-16/1.1e-16  rho 8.4e-17/6.8e-17
  f32 rand3 n=3 steps=2: d=9.9e-08/gpu=9.9e-08  omega 6.0e-08/6.0e-08  rho 2.7e-08/2.7e-08
  f64 rand5 n=5 steps=4: d=4.9e-16/gpu=3.9e-16  omega 2.9e-16/2.6e-16  rho 6.2e-17/7.7e-17
  f32 rand5 n=5 steps=4: d=2.6e-07/gpu=2.6e-07  omega 4.1e-08/5.2e-08  rho 2.5e-08/2.8e-08
  f64 rand63 n=63 steps=20: d=1.4e-16/gpu=2.8e-16  omega 4.1e-16/3.5e-16  rho 9.2e-17/8.3e-17
  f32 rand63 n=63 steps=20: d=1.1e-07/gpu=8.8e-08  omega 3.1e-08/2.0e-08  rho 3.3e-08/3.4e-08
  f64 rand64 n=64 steps=20: d=2.5e-16/gpu=2.4e-16  omega 3.0e-16/3.0e-16  rho 9.5e-17/5.7e-17
  f32 rand64 n=64 steps=20: d=1.1e-07/gpu=1.1e-07  omega 2.9e-08/3.2e-08  rho 2.5e-08/2.1e-08
  f64 rand65 n=65 steps=20: d=4.3e-16/gpu=3.3e-16  omega 2.1e-16/2.2e-16  rho 5.3e-17/4.3e-17
  f32 rand65 n=65 steps=20: d=1.4e-07/gpu=1.0e-07  omega 2.2e-08/2.0e-08  rho 2.3e-08/2.5e-08
  f64 rand255 n=255 steps=20: d=3.9e-16/gpu=2.7e-16  omega 4.5e-16/2.1e-16  rho 6.6e-17/7.1e-17
  f32 rand255 n=255 steps=20: d=1.6e-07/gpu=1.3e-07  omega 2.7e-08/1.8e-08  rho 3.9e-08/2.0e-08
  f64 rand257 n=257 steps=20: d=3.2e-16/gpu=2.9e-16  omega 3.4e-16/2.8e-16  rho 6.2e-17/7.1e-17
  f32 rand257 n=257 steps=20: d=2.8e-07/gpu=1.5e-07  omega 3.1e-08/1.7e-08  rho 3.2e-08/1.4e-08
  f64 rand1023 n=1023 steps=20: d=4.0e-16/gpu=3.3e-16  omega 4.5e-16/2.4e-16  rho 6.8e-17/5.7e-17
  f32 rand1023 n=1023 steps=20: d=2.1e-07/gpu=1.8e-07  omega 3.4e-08/2.1e-08  rho 4.2e-08/2.6e-08
  f64 rand1026 n=1026 steps=20: d=3.1e-16/gpu=3.4e-16  omega 2.6e-16/1.9e-16  rho 9.7e-17/5.8e-17
  f32 rand1026 n=1026 steps=20: d=2.5e-07/gpu=1.4e-07  omega 1.7e-08/1.4e-08  rho 4.2e-08/2.3e-08
  f64 band20001 n=20001 steps=20: d=6.1e-16/gpu=7.6e-16  omega 2.2e-16/1.4e-16  rho 4.4e-17/3.5e-17
  f32 band20001 n=20001 steps=20: d=3.4e-07/gpu=1.6e-07  omega 8.8e-09/9.5e-09  rho 1.5e-08/9.5e-09
  f64 band600001 n=600001 steps=3: d=5.2e-16/gpu=5.8e-16  omega 1.3e-16/9.8e-16  rho 1.3e-18/2.0e-18
  f32 band600001 n=600001 steps=3: d=2.8e-07/gpu=1.4e-07  omega 4.7e-10/3.6e-10  rho 8.3e-10/3.7e-10
  f64 pwtk@0.05 n=10895 steps=20: d=1.3e-15/gpu=7.6e-16  omega 3.8e-16/3.3e-16  rho 2.6e-17/1.1e-17
  f32 pwtk@0.05 n=10895 steps=20: d=6.4e-07/gpu=3.3e-07  omega 6.4e-09/7.9e-09  rho 1.4e-08/3.5e-09
  f64 band20001 (two shards) n=20001 steps=20: d=6.1e-16/gpu=7.6e-16  omega 2.2e-16/2.0e-16  rho 4.4e-17/2.9e-17
  f32 band20001 (two shards) n=20001 steps=20: d=3.4e-07/gpu=1.6e-07  omega 8.8e-09/7.5e-09  rho 1.5e-08/8.1e-09
  f64 Flan_1565@0.01 (deterministic) n=15647 steps=20: d=1.9e-15/gpu=7.6e-16  omega 2.9e-16/2.3e-16  rho 1.5e-17/6.6e-18
  f32 Flan_1565@0.01 (deterministic) n=15647 steps=20: d=1.0e-06/gpu=3.9e-07  omega 5.3e-09/4.5e-09  rho 1.2e-08/4.3e-09
  f64 rand257 (deep) n=257 steps=128: d=3.2e-16/gpu=2.9e-16  omega 3.4e-16/2.8e-16  rho 6.2e-17/7.1e-17
  f32 rand257 (deep) n=257 steps=128: d=2.8e-07/gpu=1.5e-07  omega 3.1e-08/1.7e-08  rho 3.2e-08/1.4e-08
  f64 rand1023 (deep) n=1023 steps=128: d=4.0e-16/gpu=3.3e-16  omega 6.8e-16/3.5e-16  rho 6.8e-17/5.7e-17
  f32 rand1023 (deep) n=1023 steps=128: d=2.1e-07/gpu=1.8e-07  omega 3.4e-08/2.1e-08  rho 4.2e-08/2.6e-08
  f64 band20001 (deep) n=20001 steps=128: d=6.1e-16/gpu=7.6e-16  omega 3.4e-16/2.7e-16  rho 5.0e-17/4.1e-17
  f32 band20001 (deep) n=20001 steps=128: d=3.4e-07/gpu=1.6e-07  omega 9.0e-09/9.5e-09  rho 1.5e-08/9.5e-09
"""
import ctypes as C
import functools

import numpy as np
import pytest

from test_gpu_cg_steps import DET, DTYPES, UNIT, _matrix
from test_gpu_kernel_variants import PLAN_KNOBS

pytestmark = pytest.mark.gpu

JS = (1, 2, 3, 5, 10, 20)
DEEP = 128  # = CFS_HIP_EIGS_MAX_NCV: the project kernel's 16 chunks, 129 reduce workgroups, cs[] full, the last flag word
DEEP_JS = JS + (40, 64, 65, 100, 127, 128)
DEEP_MATRICES = ["rand257", "rand1023", "band20001"]
STEP_MATRICES = [f"rand{n}" for n in (2, 3, 5, 63, 64, 65, 255, 257, 1023, 1026)] + ["band20001", "band600001", "pwtk@0.05"]


@pytest.fixture(autouse=True)
def _torch_first(monkeypatch):
    """torch brings a HIP runtime of its own: it has to initialise before libcfs_hip.so's"""
    import torch
    torch.cuda.init()
    torch.cuda.set_device(0)
    for k in PLAN_KNOBS:
        monkeypatch.delenv(k, raising=False)
    yield


def _steps(name, n):
    return 3 if name == "band600001" else min(n - 1, 20)


def _v0(n, dtype):
    return np.random.default_rng(n).uniform(-1, 1, n).astype(dtype)


def lanczos_reference(n, rp, ci, va, v0, steps, dtype=None, unit=None):
    """(V, alpha, beta, done) of the recurrence above: V holds v_1 .. v_{done+1} as rows.  va and v0 are already in the
    value type.  dtype None: np.longdouble throughout.  Otherwise the working precision of the kernels, see above."""
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

    def project_out(x, c, Vj):
        t = x.astype(S)
        for k in range(len(c)):
            t = t - c[k] * Vj[k]
        return t.astype(W)
    V = np.zeros((steps + 1, n), W)
    s0 = v0.astype(S)
    V[0] = (s0 / np.sqrt(np.dot(s0, s0))).astype(W)
    alpha, beta, done = np.zeros(steps, S), np.zeros(steps, S), steps
    for j in range(steps):
        q = mv(V[j])
        Vj = V[:j + 1].astype(S, copy=False)
        c = Vj @ q.astype(S)
        qq = np.dot(q.astype(S), q.astype(S))
        q1 = project_out(q, c, Vj)
        c2 = Vj @ q1.astype(S)
        q2 = project_out(q1, c2, Vj)
        alpha[j] = c[j] + c2[j]
        beta[j] = np.sqrt(np.dot(q2.astype(S), q2.astype(S)))
        if not beta[j] > 16 * S(unit) * np.sqrt(qq):
            done = j + 1
            break
        V[j + 1] = (q2.astype(S) / beta[j]).astype(W)
    return V, alpha, beta, done


def lanczos_gpu(A, v0, steps, dtype, ld=None, spare=0, fill=None):
    """(basis as rows (steps + 1 + spare, ld), alpha, beta, done) of cfs_hip_sym_debug_lanczos; v0 None: the library's"""
    import torch
    from cfs_spmv_amd import _lib
    n = A.nrows()
    per = 16 // np.dtype(dtype).itemsize
    ld = -(-n // per) * per if ld is None else ld
    host = np.zeros((steps + 1 + spare, ld), dtype) if fill is None else np.full((steps + 1 + spare, ld), fill, dtype)
    basis = torch.from_numpy(host.copy()).cuda()
    v0d = torch.from_numpy(np.array(v0)).cuda() if v0 is not None else None
    alpha, beta, done = np.full(steps, 7.0), np.full(steps, 7.0), C.c_int(-1)
    dp = C.POINTER(C.c_double)
    _lib.check(_lib.load().cfs_hip_sym_debug_lanczos(
        A._h, v0d.data_ptr() if v0d is not None else None, steps, basis.data_ptr(), ld, alpha.ctypes.data_as(dp),
        beta.ctypes.data_as(dp), C.byref(done), torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    return basis.cpu().numpy(), alpha, beta, done.value


def _norm_inf(n, rp, va):
    rows = np.repeat(np.arange(n), np.diff(rp))
    return float(np.max(np.bincount(rows, np.abs(va.astype(np.float64)), n)))


def invariants(n, rp, ci, va, V, alpha, beta, done, at=JS):
    """{j: (omega_j, rho_j)} in long double for the j of `at` not above `done`"""
    from oracle import oracle
    norm = np.longdouble(_norm_inf(n, rp, va))
    Vl = V[:done + 1, :n].astype(np.longdouble)
    a, b = alpha.astype(np.longdouble), beta.astype(np.longdouble)
    js = [j for j in at if j <= done]
    G = np.abs(Vl @ Vl.T - np.eye(done + 1, dtype=np.longdouble))
    out, rho = {}, 0.0
    for i in range(1, max(js, default=0) + 1):  # column i (1-based) of A V = V T
        r = oracle.csr_spmv_ldx(n, rp, ci, va, Vl[i - 1]) - a[i - 1] * Vl[i - 1] - b[i - 1] * Vl[i]
        if i >= 2:
            r = r - b[i - 2] * Vl[i - 2]
        rho = max(rho, float(np.max(np.abs(r)) / norm))
        if i in js:
            out[i] = (float(np.max(G[:i + 1, :i + 1])), rho)
    return out


@functools.lru_cache(maxsize=None)
def _case(name, dtype, steps=None):
    """the matrix in the value type, v0, and the two CPU runs with their invariants: computed once, shared, unchanged.
    steps None: _steps(name, n), the invariants at JS; DEEP: at DEEP_JS"""
    n, rp, ci, va = _matrix(name)
    va = va.astype(dtype)
    v0 = _v0(n, dtype)
    at = JS if steps is None else DEEP_JS
    steps = _steps(name, n) if steps is None else steps
    ref = lanczos_reference(n, rp, ci, va, v0, steps, unit=UNIT[dtype])
    work = lanczos_reference(n, rp, ci, va, v0, steps, dtype, unit=UNIT[dtype])
    assert ref[3] == work[3] == steps, f"{name}: a breakdown on the CPU: badly chosen case"
    inv = invariants(n, rp, ci, va, work[0], work[1], work[2], steps, at)
    for x in (rp, ci, va, v0) + ref[:3] + work[:3]:
        x.setflags(write=False)
    return n, rp, ci, va, v0, steps, ref, work, inv


def _check(name, dtype, A, label="", deep=None):
    n, rp, ci, va, v0, steps, ref, work, inv = _case(name, dtype, deep)
    u, norm = UNIT[dtype], _norm_inf(n, rp, va)
    V, alpha, beta, done = lanczos_gpu(A, v0, steps, dtype)
    errors = []
    if done != steps:
        errors.append(f"{done} steps made, not {steps}")
    worst = (0.0, 0.0)
    for j in range(min(3, steps)):
        for what, g, wk, rf in (("alpha", alpha, work[1], ref[1]), ("beta", beta, work[2], ref[2])):
            d = abs(float(np.longdouble(wk[j]) - rf[j])) / norm
            dev = abs(float(np.longdouble(g[j]) - rf[j])) / norm
            worst = max(worst, (dev, d))
            if not dev <= 4 * d + 16 * u:
                errors.append(f"{what}_{j + 1}: deviation {dev:.3e}, allowed {4 * d + 16 * u:.3e} (d = {d:.3e})")
    scale = float(np.max(np.abs(ref[0][1])))
    d = float(np.max(np.abs(work[0][1].astype(np.longdouble) - ref[0][1]))) / scale
    dev = float(np.max(np.abs(V[1, :n].astype(np.longdouble) - ref[0][1]))) / scale
    worst = max(worst, (dev, d))
    if not dev <= 4 * d + 16 * u:
        errors.append(f"v_2: deviation {dev:.3e}, allowed {4 * d + 16 * u:.3e} (d = {d:.3e})")
    got = invariants(n, rp, ci, va, V, alpha, beta, min(done, steps), tuple(inv))
    wo = max(((got[j][0], inv[j][0]) for j in got), default=(0.0, 0.0))
    wr = max(((got[j][1], inv[j][1]) for j in got), default=(0.0, 0.0))
    print(f"lanczos-steps {np.dtype(dtype).name} {name}{label} n={n} steps={steps}: d={worst[1]:.1e}/gpu={worst[0]:.1e}  "
          f"omega {wo[1]:.1e}/{wo[0]:.1e}  rho {wr[1]:.1e}/{wr[0]:.1e}")
    for j in got:
        for what, k in (("omega", 0), ("rho", 1)):
            if not got[j][k] <= 4 * inv[j][k] + 16 * u:
                errors.append(f"{what}_{j} = {got[j][k]:.3e}, allowed {4 * inv[j][k] + 16 * u:.3e} (the model's: {inv[j][k]:.3e})")
    assert not errors, f"{name}{label} {np.dtype(dtype).name}: " + "; ".join(errors)
    return V, alpha, beta


@DTYPES
@pytest.mark.parametrize("name", STEP_MATRICES)
def test_steps_against_the_long_double_recurrence(name, dtype):
    import cfs_spmv_amd as cfs
    n, rp, ci, va = _case(name, dtype)[:4]
    A = cfs.SymMatrix(n, rp, ci, va)
    assert A.stats()["n"] == n and A.row_end - A.row_begin == n
    _check(name, dtype, A)
    A.close()


@DTYPES
@pytest.mark.parametrize("name", DEEP_MATRICES)
def test_deep_bases_against_the_long_double_recurrence(name, dtype):
    """DEEP = 128 steps, a basis of 129 columns: alpha, beta and v_2 for j <= 3 as above, omega_j and rho_j at DEEP_JS"""
    import cfs_spmv_amd as cfs
    n, rp, ci, va, v0, steps, ref, work, inv = _case(name, dtype, DEEP)
    assert steps == DEEP and sorted(inv) == sorted(DEEP_JS)
    A = cfs.SymMatrix(n, rp, ci, va)
    _check(name, dtype, A, label=" (deep)", deep=DEEP)
    A.close()


@DTYPES
def test_steps_through_a_two_shard_handle(dtype):
    """an odd n through a multi-device handle (two shards, here on one device): the products on the shards' streams,
    the basis and the vector kernels on the home device and the caller's stream"""
    import cfs_spmv_amd as cfs
    n, rp, ci, va = _case("band20001", dtype)[:4]
    M = cfs.SymMatrix(n, rp, ci, va, ngpus=2)
    _check("band20001", dtype, M, label=" (two shards)")
    M.close()


@DTYPES
def test_a_deterministic_handle_is_bit_reproducible(dtype):
    import cfs_spmv_amd as cfs
    name = "Flan_1565@0.01"
    n, rp, ci, va = _case(name, dtype)[:4]
    D = cfs.SymMatrix(n, rp, ci, va, options=cfs.make_options(flags=DET))
    assert D.kernel_variant()["det"] == 1
    V1, a1, b1 = _check(name, dtype, D, label=" (deterministic)")
    V2, a2, b2, done = lanczos_gpu(D, _case(name, dtype)[4], _case(name, dtype)[5], dtype)
    assert np.array_equal(V1.view(np.uint8), V2.view(np.uint8))
    assert np.array_equal(a1.view(np.uint8), a2.view(np.uint8)) and np.array_equal(b1.view(np.uint8), b2.view(np.uint8))
    D.close()


@DTYPES
def test_padding_and_a_spare_column_stay_intact(dtype):
    """ld = n + 5 (a multiple of 16 bytes for n = 1023), the rows [n, ld) of every column and a spare column behind the
    last one patterned with NaNs of a recognisable payload: all of it bit-intact, the steps the same bits as with the
    tight layout"""
    import cfs_spmv_amd as cfs
    name = "rand1023"
    n, rp, ci, va, v0, steps = _case(name, dtype)[:6]
    ld = n + 5
    assert ld * np.dtype(dtype).itemsize % 16 == 0
    pattern = np.array([0x7ff8dead0000beef], np.uint64).view(np.float64)[0] if dtype == np.float64 else \
        np.array([0x7fc0beef], np.uint32).view(np.float32)[0]
    A = cfs.SymMatrix(n, rp, ci, va)
    V, alpha, beta, done = lanczos_gpu(A, v0, steps, dtype, ld=ld, spare=1, fill=pattern)
    Vt, at, bt, dt = lanczos_gpu(A, v0, steps, dtype)
    A.close()
    assert done == dt == steps
    bits = np.uint64 if dtype == np.float64 else np.uint32
    assert np.all(V[:, n:].view(bits) == np.array([pattern]).view(bits)[0])
    assert np.all(V[steps + 1].view(bits) == np.array([pattern]).view(bits)[0])
    assert not np.isnan(V[:steps + 1, :n]).any()
    # (the same steps as with the tight layout; the product of a plain handle adds in an order of its own in every
    # run, so alpha_1 -- a sum of n terms of size ||A|| / n -- agrees to rounding, not bitwise)
    assert abs(alpha[0] - at[0]) <= 16 * UNIT[dtype] * _norm_inf(n, rp, va)


@DTYPES
def test_padding_and_a_spare_column_stay_intact_at_a_deep_basis(dtype):
    """the same at DEEP = 128 steps -- 129 columns with ld = n + 5 and a spare one behind them -- on a deterministic handle,
    whose products add in a fixed order: the basis, alpha and beta are the same BITS as with the tight layout"""
    import cfs_spmv_amd as cfs
    name = "rand1023"
    n, rp, ci, va, v0 = _case(name, dtype, DEEP)[:5]
    ld = n + 5
    assert ld * np.dtype(dtype).itemsize % 16 == 0
    pattern = np.array([0x7ff8dead0000beef], np.uint64).view(np.float64)[0] if dtype == np.float64 else \
        np.array([0x7fc0beef], np.uint32).view(np.float32)[0]
    D = cfs.SymMatrix(n, rp, ci, va, options=cfs.make_options(flags=DET))
    assert D.kernel_variant()["det"] == 1
    V, alpha, beta, done = lanczos_gpu(D, v0, DEEP, dtype, ld=ld, spare=1, fill=pattern)
    Vt, at, bt, dt = lanczos_gpu(D, v0, DEEP, dtype)
    D.close()
    assert done == dt == DEEP
    bits = np.uint64 if dtype == np.float64 else np.uint32
    assert np.all(V[:, n:].view(bits) == np.array([pattern]).view(bits)[0])
    assert np.all(V[DEEP + 1].view(bits) == np.array([pattern]).view(bits)[0])
    assert not np.isnan(V[:DEEP + 1, :n]).any()
    assert np.array_equal(np.ascontiguousarray(V[:DEEP + 1, :n]).view(bits), np.ascontiguousarray(Vt[:, :n]).view(bits))
    assert np.array_equal(alpha.view(np.uint64), at.view(np.uint64)) and np.array_equal(beta.view(np.uint64), bt.view(np.uint64))


def default_v0(n):
    """the start vector cfs_hip.h documents for v0_dev = NULL"""
    z = (np.arange(n, dtype=np.uint64) + np.uint64(1)) * np.uint64(0x9E3779B97F4A7C15)
    z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
    z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    z = z ^ (z >> np.uint64(31))
    return (z >> np.uint64(11)).astype(np.float64) * 2.0 ** -53 - 0.5


@DTYPES
def test_the_null_start_vector(dtype):
    import cfs_spmv_amd as cfs
    name = "rand1023"
    n, rp, ci, va = _case(name, dtype)[:4]
    A = cfs.SymMatrix(n, rp, ci, va)
    V1, a1, b1, d1 = lanczos_gpu(A, None, 1, dtype)
    V2, a2, b2, d2 = lanczos_gpu(A, None, 1, dtype)
    A.close()
    assert d1 == d2 == 1
    assert np.array_equal(V1[0].view(np.uint8), V2[0].view(np.uint8))
    v = V1[0, :n].astype(np.longdouble)
    assert abs(float(np.sqrt(np.dot(v, v))) - 1.0) <= 16 * UNIT[dtype]
    assert np.ptp(V1[0, :n]) > 0.01, "not constant"
    # ... and it is the documented function of the row index
    with np.errstate(over="ignore"):
        w = default_v0(n).astype(dtype).astype(np.float64)
    w = w / np.sqrt(np.dot(w, w))
    assert np.max(np.abs(V1[0, :n] - w)) <= 4 * UNIT[dtype] * np.max(np.abs(w))


def decoupled(name, rows, block):
    """_matrix(name) with the rows and columns `rows` cut off from the rest and holding `block`"""
    import scipy.sparse as sp
    n, rp, ci, va = _matrix(name)
    A = sp.lil_matrix(sp.csr_matrix((va, ci, rp), shape=(n, n)))
    rows = list(rows)
    A[rows, :] = 0
    A[:, rows] = 0
    for i, r in enumerate(rows):
        for j, c in enumerate(rows):
            A[r, c] = block[i][j]
    A = A.tocsr()
    A.eliminate_zeros()
    A.sort_indices()
    assert abs(A - A.T).max() == 0
    return n, A.indptr.astype(np.int32), A.indices.astype(np.int32), A.data


BLOCK3 = [[2.0, 1.0, 0.0], [1.0, 2.0, 1.0], [0.0, 1.0, 2.0]]


@DTYPES
def test_breakdown(dtype):
    """both exact in floating point: a diagonal-only row i with v0 = e_i (alpha_1 = a_ii, beta_1 = 0, one step made); the
    integer block [[2, 1, 0], [1, 2, 1], [0, 1, 2]] cut off from the rest of rand257 with v0 = e_0 (v_2 = e_1, v_3 = e_2,
    three steps made, alpha = 2, 2, 2, beta = 1, 1, 0)"""
    import cfs_spmv_amd as cfs
    i = 100
    n, rp, ci, va = decoupled("rand257", [i], [[3.0]])
    A = cfs.SymMatrix(n, rp, ci, va.astype(dtype))
    e = np.zeros(n, dtype)
    e[i] = 1
    V, alpha, beta, done = lanczos_gpu(A, e, 5, dtype)
    A.close()
    assert done == 1 and alpha[0] == 3.0 and beta[0] == 0.0
    assert np.array_equal(V[0, :n], e) and not V[1:].any()
    assert not alpha[1:].any() and not beta[1:].any()
    n, rp, ci, va = decoupled("rand257", [0, 1, 2], BLOCK3)
    A = cfs.SymMatrix(n, rp, ci, va.astype(dtype))
    e = np.zeros(n, dtype)
    e[0] = 1
    V, alpha, beta, done = lanczos_gpu(A, e, 6, dtype)
    A.close()
    assert done == 3 and list(alpha[:3]) == [2.0, 2.0, 2.0] and list(beta[:3]) == [1.0, 1.0, 0.0]
    assert np.array_equal(V[:3, :3], np.eye(3, dtype=dtype)) and not V[:3, 3:].any() and not V[3:].any()


@DTYPES
def test_argument_checks(dtype):
    import torch
    import cfs_spmv_amd as cfs
    from cfs_spmv_amd import _lib
    n, rp, ci, va = _case("rand1023", dtype)[:4]
    A = cfs.SymMatrix(n, rp, ci, va)
    with pytest.raises(_lib.CfsHipError, match="bad ld") as e:
        lanczos_gpu(A, None, 2, dtype, ld=n - 1)  # below n
    assert e.value.code == _lib.ERR_ARG
    with pytest.raises(_lib.CfsHipError, match="bad ld") as e:
        lanczos_gpu(A, None, 2, dtype, ld=n + 2)  # odd: no multiple of 16 bytes
    assert e.value.code == _lib.ERR_ARG
    with pytest.raises(_lib.CfsHipError, match="start vector") as e:
        lanczos_gpu(A, np.zeros(n, dtype), 2, dtype)
    assert e.value.code == _lib.ERR_ARG
    a, b, d = (C.c_double * 4)(), (C.c_double * 4)(), C.c_int(7)
    host = np.zeros(4 * 1024, dtype)
    rc = _lib.load().cfs_hip_sym_debug_lanczos(A._h, None, 2, host.ctypes.data // 16 * 16 + 16, 1024, a, b, C.byref(d), None)
    assert rc == _lib.ERR_ARG and b"device pointer" in _lib.load().cfs_hip_last_error()
    A.close()
    S = cfs.SymMatrix(n, rp, ci, va, row_splits=np.array([0, n // 2, n], np.int32), rank=1)
    with pytest.raises(_lib.CfsHipError) as e:
        lanczos_gpu(S, None, 2, dtype)
    assert e.value.code == _lib.ERR_UNSUPPORTED
    S.close()
    torch.cuda.synchronize()
