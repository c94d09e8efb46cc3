"""cfs_hip_sym_minres step by step, by the method of test_gpu_cg_steps.py / test_gpu_pcg_steps.py: the ITERATES u_k of
the native MINRES (minres_residual_kernel and minres_start_kernel once, then minres_lanczos_kernel,
minres_residual2_kernel, minres_update_kernel behind the SpMV) for (A - shift I) u = b against the same recurrence
in np.longdouble on the CPU,

    q = A u;  r2 = b - (q - shift u);  z = dinv r2;  beta1 = sqrt(r2.z);  v = z / beta1;  r1 = r2;  w = w2 = 0
    oldb = 0, beta = beta1, dbar = 0, epsln = 0, phibar = beta1, cs = -1, sn = 0
    q = A v;  t = q - shift v - (beta / oldb) r1 [k >= 1];  alfa = v.t;  y = t - (alfa / beta) r2;  r1, r2 = r2, y
    betan = sqrt(y . dinv y);  oldeps = epsln;  delta = cs dbar + sn alfa;  gbar = sn dbar - cs alfa
    epsln = sn betan;  dbar = -cs betan;  gamma = max(sqrt(gbar^2 + betan^2), eps);  cs = gbar / gamma;  sn = betan / gamma
    phi = cs phibar;  phibar = sn phibar;  wn = (v - oldeps w2 - delta w) / gamma;  u += phi wn;  v = dinv y / betan

with the product as long-double row sums of the CSR (oracle.csr_spmv_ldx) and dinv = 1 / |a_ii - shift| in long
double from the diagonal rounded to the value type (dinv = 1 without a preconditioner).  minres_native(..., tol=0,
maxiter=k) returns u after exactly k iterations.

Tolerance for ||u_k(GPU) - u_k(long double)||inf / ||u_k(long double)||inf, derived exactly as in the sibling tests:
the recurrence is run a second time on the CPU in the working precision with the kernels' rounding rules -- vectors
and the product in fp64 / fp32, every dot product and scalar in fp64, r2, t, y, wn, u and v computed in fp64 and
rounded when stored, alfa and betan from the STORED t and y, u from the stored wn, dinv_i = (V)(1.0 / fabs((double)a_ii
- shift)) stored in the value type, z = dinv r formed in fp64 and never rounded; d_k is its deviation from the
long-double run.  A correct GPU run differs from that CPU run only in the order of the additions inside the product
and the dots, so it is allowed 4 d_k + 16 u (u = 2^-53 / 2^-24).  Neither the reference nor d_k involves the library.
A case whose d_k exceeds D_LIMIT of the plain test (1e-6 / 1e-2) is badly chosen and fails.

Matrices: signed(name) is _matrix(name) of the plain test with the sign of the diagonal flipped on the rows drawn by
default_rng(3).choice([-1, 1], n) (rows 0 and 1 pinned to +, -): the rand / band matrices keep |a_ii| = 1 + the
row's absolute off-diagonal sum, so by Gershgorin every |lambda| >= 1 -- indefinite and well conditioned.  For the
Jacobi cases the matrix is additionally scaled(...) as in test_gpu_pcg_steps.py, so a wrong dinv moves u_1 by orders
of magnitude.

Measured on the MI355X (value type, matrix, preconditioner, then for k = 1, 2, 3, 5, 10: d_k / the GPU's deviation):

  f64 rand1 none                             0.0e+00/0.0e+00  0.0e+00/0.0e+00  0.0e+00/0.0e+00  0.0e+00/0.0e+00  0.0e+00/0.0e+00
  f32 rand1 none                             0.0e+00/0.0e+00  7.2e-20/7.2e-20  7.2e-20/7.2e-20  7.2e-20/7.2e-20  7.2e-20/7.2e-20
  f64 rand1 jacobi                           0.0e+00/0.0e+00  0.0e+00/0.0e+00  0.0e+00/0.0e+00  0.0e+00/0.0e+00  0.0e+00/0.0e+00
  f32 rand1 jacobi                           0.0e+00/0.0e+00  7.2e-20/7.2e-20  7.2e-20/7.2e-20  7.2e-20/7.2e-20  7.2e-20/7.2e-20
  f64 rand2 none                             1.0e-16/3.0e-16  6.1e-17/4.1e-16  1.5e-16/4.1e-16  1.5e-16/2.7e-16  1.5e-16/2.7e-16
  f32 rand2 none                             6.0e-08/1.0e-07  4.2e-08/1.2e-07  4.2e-08/1.2e-07  4.2e-08/1.2e-07  4.2e-08/1.2e-07
  f64 rand2 jacobi                           2.0e-16/2.0e-16  2.7e-16/4.8e-16  2.7e-16/5.5e-17  2.7e-16/5.5e-17  2.7e-16/5.5e-17
  f32 rand2 jacobi                           4.5e-08/4.5e-08  5.5e-08/5.5e-08  5.5e-08/5.5e-08  5.5e-08/5.5e-08  5.5e-08/5.5e-08
  f64 rand3 none                             2.6e-15/3.7e-16  1.4e-16/1.4e-16  1.7e-16/1.7e-16  3.3e-16/3.3e-16  3.3e-16/3.3e-16
  f32 rand3 none                             1.4e-06/1.4e-06  6.0e-08/6.0e-08  7.5e-08/7.5e-08  7.4e-08/7.4e-08  7.4e-08/7.4e-08
  f64 rand3 jacobi                           6.3e-17/6.0e-17  1.6e-17/2.5e-16  4.1e-17/3.1e-17  4.1e-17/2.4e-17  4.1e-17/2.4e-17
  f32 rand3 jacobi                           2.6e-08/2.6e-08  1.6e-08/1.6e-08  3.0e-08/3.0e-08  3.0e-08/3.0e-08  3.0e-08/3.0e-08
  f64 rand5 none                             8.1e-17/8.1e-17  1.8e-16/2.8e-16  2.4e-16/3.1e-16  1.4e-16/6.8e-16  1.9e-16/3.4e-16
  f32 rand5 none                             7.1e-08/7.1e-08  8.6e-08/8.6e-08  9.0e-08/9.0e-08  7.8e-08/7.8e-08  7.8e-08/7.8e-08
  f64 rand5 jacobi                           2.5e-16/1.2e-16  1.6e-16/4.9e-17  2.1e-16/3.5e-17  1.4e-16/1.1e-16  1.4e-16/1.1e-16
  f32 rand5 jacobi                           3.7e-08/3.7e-08  4.6e-08/4.6e-08  3.3e-08/3.3e-08  4.1e-09/6.0e-08  4.1e-09/6.0e-08
  f64 rand63 none                            2.5e-16/4.9e-16  4.6e-16/2.1e-16  3.7e-16/3.8e-16  3.9e-16/3.1e-16  5.3e-16/3.1e-16
  f32 rand63 none                            7.3e-08/1.1e-07  1.4e-07/1.1e-07  2.8e-07/1.6e-07  2.1e-07/1.4e-07  2.0e-07/1.5e-07
  f64 rand63 jacobi                          2.6e-16/4.1e-16  4.3e-16/4.2e-16  2.8e-16/4.7e-16  4.6e-16/4.6e-16  3.3e-16/4.7e-16
  f32 rand63 jacobi                          3.0e-08/1.0e-07  5.2e-08/5.7e-08  5.3e-08/7.7e-08  4.7e-08/7.6e-08  1.2e-07/1.2e-07
  f64 rand64 none                            2.2e-16/2.9e-16  4.5e-16/3.7e-16  6.9e-16/6.1e-16  6.9e-16/5.8e-16  4.8e-16/5.2e-16
  f32 rand64 none                            1.0e-07/1.5e-07  1.5e-07/1.5e-07  3.2e-07/2.3e-07  1.4e-07/1.6e-07  1.9e-07/1.6e-07
  f64 rand64 jacobi                          3.4e-16/1.8e-16  4.0e-16/1.9e-16  2.2e-16/2.5e-16  8.5e-17/3.4e-17  9.4e-17/9.4e-17
  f32 rand64 jacobi                          3.7e-08/3.7e-08  5.7e-08/5.7e-08  9.4e-08/7.8e-08  1.4e-07/5.3e-08  2.5e-07/1.4e-07
  f64 rand65 none                            1.4e-15/1.5e-15  2.3e-16/2.3e-16  3.5e-16/3.5e-16  3.2e-16/4.3e-16  4.2e-16/3.5e-16
  f32 rand65 none                            2.9e-07/4.8e-07  1.4e-07/1.2e-07  1.2e-07/1.1e-07  1.8e-07/1.7e-07  1.5e-07/1.6e-07
  f64 rand65 jacobi                          3.7e-16/1.4e-16  3.1e-16/1.7e-16  3.7e-16/2.8e-16  1.4e-16/2.3e-16  1.2e-16/2.6e-16
  f32 rand65 jacobi                          1.5e-07/2.4e-07  1.2e-07/6.2e-08  9.1e-08/6.1e-08  8.0e-08/4.7e-08  6.4e-08/3.8e-08
  f64 rand255 none                           3.5e-16/1.8e-16  3.0e-16/3.8e-16  3.8e-16/2.9e-16  6.1e-16/4.5e-16  5.3e-16/3.6e-16
  f32 rand255 none                           1.1e-07/8.7e-08  1.9e-07/1.2e-07  2.2e-07/1.4e-07  1.8e-07/2.4e-07  2.9e-07/1.3e-07
  f64 rand255 jacobi                         5.2e-16/2.3e-16  6.0e-16/4.9e-16  7.2e-16/6.0e-16  1.4e-16/3.7e-16  3.1e-16/2.4e-16
  f32 rand255 jacobi                         4.0e-08/4.0e-08  9.4e-08/9.4e-08  8.0e-08/7.5e-08  6.5e-08/9.7e-08  8.4e-08/9.9e-08
  f64 rand257 none                           3.5e-16/2.2e-16  4.3e-16/2.8e-16  3.6e-16/4.0e-16  8.1e-16/7.5e-16  6.6e-16/1.3e-15
  f32 rand257 none                           1.5e-07/1.1e-07  1.4e-07/1.5e-07  2.5e-07/1.0e-07  1.8e-07/2.2e-07  3.3e-07/2.1e-07
  f64 rand257 jacobi                         1.5e-16/3.8e-16  5.3e-16/2.4e-16  5.0e-16/2.3e-16  4.3e-16/2.1e-16  4.6e-16/2.3e-16
  f32 rand257 jacobi                         1.3e-07/1.1e-07  1.6e-07/1.6e-07  1.4e-07/1.4e-07  1.4e-07/1.4e-07  1.2e-07/8.1e-08
  f64 rand1023 none                          2.1e-15/5.2e-16  4.3e-16/3.5e-16  5.3e-16/4.0e-16  4.2e-16/6.2e-16  1.5e-15/1.9e-15
  f32 rand1023 none                          7.7e-07/4.9e-07  1.8e-07/2.3e-07  1.6e-07/2.6e-07  3.9e-07/1.9e-07  6.1e-07/4.4e-07
  f64 rand1023 jacobi                        2.4e-15/1.1e-15  5.3e-16/3.3e-16  5.1e-16/3.3e-16  3.8e-16/1.3e-16  4.3e-16/2.2e-16
  f32 rand1023 jacobi                        4.0e-07/3.7e-07  9.8e-08/9.8e-08  1.1e-07/1.1e-07  8.4e-08/8.4e-08  1.1e-07/1.1e-07
  f64 rand1026 none                          6.6e-16/4.1e-16  4.0e-16/4.0e-16  3.7e-16/3.7e-16  5.7e-16/8.8e-16  6.6e-16/9.7e-16
  f32 rand1026 none                          1.9e-07/2.3e-07  1.7e-07/9.7e-08  2.2e-07/8.9e-08  5.2e-07/5.2e-07  4.6e-07/4.3e-07
  f64 rand1026 jacobi                        1.2e-16/2.6e-16  1.9e-16/2.3e-16  2.3e-16/2.8e-16  1.4e-16/1.8e-16  2.3e-16/2.3e-16
  f32 rand1026 jacobi                        9.0e-08/9.0e-08  1.1e-07/1.1e-07  7.8e-08/7.8e-08  7.6e-08/7.6e-08  8.3e-08/8.3e-08
  f64 band600001 none                        3.8e-15/1.4e-15  4.3e-16/4.3e-16  5.0e-16/4.8e-16  6.4e-16/7.9e-16  1.0e-15/1.3e-15
  f32 band600001 none                        2.3e-07/1.4e-07  2.2e-07/1.8e-07  2.2e-07/2.0e-07  3.1e-07/2.2e-07  5.2e-07/2.7e-07
  f64 band600001 jacobi                      3.4e-15/3.1e-16  6.1e-16/6.6e-16  6.0e-16/6.9e-16  5.5e-16/3.8e-16  7.7e-16/5.9e-16
  f32 band600001 jacobi                      1.4e-07/1.4e-07  2.5e-07/2.0e-07  2.3e-07/2.3e-07  1.7e-07/1.5e-07  2.3e-07/2.1e-07
  f64 pwtk@0.05 none                         1.7e-15/1.1e-15  8.0e-16/5.5e-16  7.3e-16/5.7e-16  1.2e-15/8.5e-16  6.2e-16/6.6e-16
  f32 pwtk@0.05 none                         5.5e-07/4.2e-07  3.2e-07/1.7e-07  3.6e-07/1.7e-07  8.3e-07/3.2e-07  3.2e-07/2.1e-07
  f64 pwtk@0.05 jacobi                       7.9e-16/5.8e-16  6.6e-16/2.8e-16  9.3e-16/4.4e-16  4.1e-16/2.4e-16  5.4e-16/2.7e-16
  f32 pwtk@0.05 jacobi                       1.6e-07/9.8e-08  2.6e-07/1.2e-07  2.8e-07/1.2e-07  2.3e-07/1.8e-07  2.8e-07/1.3e-07
  f64 rand1023 none shift=3.0                4.0e-16/4.0e-16  6.5e-16/5.8e-16  9.6e-16/5.8e-16  6.9e-16/6.2e-16  1.1e-15/1.1e-15
  f32 rand1023 none shift=3.0                1.3e-07/1.3e-07  1.6e-07/1.5e-07  3.7e-07/3.1e-07  6.1e-07/3.2e-07  5.1e-07/3.8e-07
  f64 rand1023 jacobi shift=3.0              4.3e-14/4.4e-14  2.4e-15/2.7e-15  2.2e-15/2.4e-15  1.6e-14/3.2e-14  2.3e-12/1.8e-12
  f32 rand1023 jacobi shift=3.0              3.3e-05/3.3e-05  3.3e-06/3.3e-06  6.1e-06/6.0e-06  3.0e-05/2.1e-05  2.7e-03/3.0e-03
  f64 band20001 none shift=3.0               6.3e-16/5.2e-16  5.8e-16/6.8e-16  7.8e-16/6.8e-16  9.7e-16/1.5e-15  2.1e-15/3.3e-15
  f32 band20001 none shift=3.0               2.2e-07/1.5e-07  3.1e-07/2.0e-07  3.0e-07/2.1e-07  5.1e-07/5.0e-07  1.0e-06/6.2e-07
  f64 band20001 jacobi shift=3.0             1.3e-16/1.3e-16  1.5e-15/1.5e-15  1.2e-14/2.8e-14  2.7e-15/1.8e-15  7.7e-15/1.7e-14
  f32 band20001 jacobi shift=3.0             8.0e-08/1.5e-08  1.1e-06/1.1e-07  6.3e-06/5.2e-06  7.9e-07/2.2e-06  7.5e-06/5.2e-06
  f64 band20001 none (two shards)            4.2e-16/4.6e-16  5.0e-16/5.9e-16  5.3e-16/6.2e-16  6.2e-16/5.2e-16  7.0e-16/9.0e-16
  f32 band20001 none (two shards)            5.2e-07/2.9e-07  2.2e-07/1.6e-07  2.2e-07/1.9e-07  2.1e-07/1.8e-07  2.2e-07/2.0e-07
  f64 band20001 jacobi (two shards)          4.2e-16/2.3e-16  7.2e-16/5.5e-16  7.8e-16/5.3e-16  4.4e-16/4.5e-16  4.7e-16/6.4e-16
  f32 band20001 jacobi (two shards)          3.3e-07/2.0e-07  2.1e-07/1.6e-07  2.0e-07/1.7e-07  1.4e-07/1.3e-07  1.9e-07/2.1e-07
  f64 Flan_1565@0.01 none (deterministic)    3.8e-16/1.2e-15  1.1e-15/5.5e-16  1.1e-15/5.7e-16  1.6e-15/9.4e-16  7.3e-16/5.3e-16
  f32 Flan_1565@0.01 none (deterministic)    5.1e-07/2.5e-07  4.9e-07/2.4e-07  4.7e-07/2.5e-07  7.4e-07/3.4e-07  4.4e-07/1.8e-07
  f64 Flan_1565@0.01 jacobi (deterministic)  3.6e-16/2.6e-16  1.0e-15/7.4e-16  1.2e-15/9.7e-16  5.1e-16/4.1e-16  5.6e-16/4.2e-16
  f32 Flan_1565@0.01 jacobi (deterministic)  3.0e-07/2.4e-07  2.5e-07/1.9e-07  3.2e-07/2.1e-07  2.5e-07/1.2e-07  3.3e-07/1.7e-07

The shifted Jacobi cases are the sensitive ones: some |a_ii - 3| is small (0.025 on band20001, 0.011 on rand1023), so
M is badly conditioned and d_k itself jumps between iterations.  On the CPU, the working-precision recurrence of
band20001 (fp64) with nothing changed but the order of the additions inside its dot products deviates from the
long-double run at k = 10 by 5.7e-15 ... 3.2e-14 (seven orders tried).  The vector kernels are compiled without
fused multiply-adds so that the order of additions is indeed all that separates the GPU from the working-precision
run: with contraction on, this case measured 3.5e-14 at k = 10 against the 3.3e-14 allowed; without, 1.7e-14, and
u_2 of that case agrees with the CPU run to every digit printed.

Converged solves on the MI355X:

  f64 Flan_1565@0.01 none (deterministic): 106 iterations, relres 9.402e-09
  f32 Flan_1565@0.01 none (deterministic): 52 iterations, relres 7.699e-05
  f64 Flan_1565@0.01 jacobi (deterministic): 36 iterations, relres 1.534e-07
  f32 Flan_1565@0.01 jacobi (deterministic): 17 iterations, relres 3.008e-03
  f64 saddle: GPU 98 iterations, relres 9.799e-09 (long double 9.799e-09, slack 2.002e-12)
  f32 saddle: GPU 48 iterations, relres 9.465e-05 (long double 9.465e-05, slack 2.014e-05)
  f64 band20001 signed, scaled: GPU Jacobi 66 iterations, relres 2.844e-07
  f64 band20001 signed, scaled: GPU none relres 7.036e-01 after 330 iterations
  f32 band20001 signed, scaled: GPU Jacobi 32 iterations, relres 2.362e-03
  f32 band20001 signed, scaled: GPU none relres 7.368e-01 after 160 iterations
"""
import ctypes as C

import numpy as np
import pytest

from rand_matrices import banded_spd
from test_gpu_cg_steps import D_LIMIT, DET, DTYPES, KS, MATRICES, UNIT, _deviation, _matrix, _rhs, _true_relres
from test_gpu_kernel_variants import PLAN_KNOBS
from test_gpu_pcg_steps import _diag, scaled

pytestmark = pytest.mark.gpu

PRECONDS = pytest.mark.parametrize("precond", ["none", "jacobi"])
SIGN_SEED = 3
STEP_MATRICES = [m for m in MATRICES if m.startswith(("rand", "band"))] + ["pwtk@0.05"]
assert STEP_MATRICES == [f"rand{n}" for n in (1, 2, 3, 5, 63, 64, 65, 255, 257, 1023, 1026)] + ["band600001", "pwtk@0.05"]


@pytest.fixture(autouse=True)
def _torch_first(monkeypatch):
    """torch brings a HIP runtime of its own: it has to initialise before libcfs_hip.so's"""
    import torch
    torch.cuda.init()
    torch.cuda.set_device(0)
    for k in PLAN_KNOBS + ("CFS_HIP_CG_GRAPH",):
        monkeypatch.delenv(k, raising=False)
    yield


def signed(name):
    """_matrix(name) with the sign of the diagonal flipped on random rows; rows 0 and 1 are +, -"""
    n, rp, ci, va = _matrix(name)
    sign = np.random.default_rng(SIGN_SEED).choice([-1, 1], n)
    sign[:2] = (1, -1)[:min(n, 2)]
    rows = np.repeat(np.arange(n), np.diff(rp))
    va = np.array(va, np.float64)
    on = rows == ci
    va[on] *= sign[rows[on]]
    return n, rp, ci, va


def _case(name, dtype, precond, sign=True):
    """(n, rp, ci, va in the value type): signed (or not), and scaled for Jacobi"""
    n, rp, ci, va = signed(name) if sign else _matrix(name)
    return n, rp, ci, (scaled(n, rp, ci, va, dtype) if precond == "jacobi" else va.astype(dtype))


def _shifted(n, rp, ci, va, shift):
    """A - shift I as a CSR with float64 values (a_ii - shift is exact there for the cases used)"""
    if shift == 0.0:
        return rp, ci, va
    import scipy.sparse as sp
    A = (sp.csr_matrix((va.astype(np.float64), ci, rp), shape=(n, n)) - shift * sp.identity(n)).tocsr()
    A.sort_indices()
    return A.indptr.astype(np.int32), A.indices.astype(np.int32), A.data


def _relres(n, rp, ci, va, b, u, dtype, shift=0.0):
    """_true_relres of the plain test for the shifted operator"""
    rps, cis, vas = _shifted(n, rp, ci, va, shift)
    return _true_relres(n, rps, cis, vas, b.astype(vas.dtype), u.astype(vas.dtype), dtype)


def minres_reference(n, rp, ci, va, b, ks=(), dtype=None, x0=None, precond="none", shift=0.0, tol=0.0, maxiter=None):
    """{k: (u_k, iterations done)} of the recurrence above from u = x0 (0), with the kernels' ends (nothing more once
    phibar is not > tol sqrt(b . dinv b) or betan is not > 0; v = 0 when betan = 0); with `maxiter` also
    out["count"] = iterations until then.  va is already in the value type.
    dtype None: np.longdouble throughout.  Otherwise the working precision of the kernels, see above."""
    import scipy.sparse as sp
    from oracle import oracle
    ld = dtype is None
    W, S = (np.longdouble, np.longdouble) if ld else (dtype, np.float64)
    sig, eps = S(shift), S(2.0 ** -52)
    if precond == "jacobi":
        d = _diag(n, rp, ci, va)
        dinv = 1 / np.abs(d.astype(S) - sig) if ld else (1.0 / np.abs(d.astype(S) - sig)).astype(dtype).astype(S)
    else:
        assert precond == "none"
        dinv = np.ones(n, S)
    if ld:
        def mv(x):
            return oracle.csr_spmv_ldx(n, rp, ci, va, x)
    else:
        A = sp.csr_matrix((va.astype(dtype), ci, rp), shape=(n, n))

        def mv(x):
            return (A @ x).astype(dtype)
    u = np.zeros(n, W) if x0 is None else x0.astype(W)
    r2 = (b.astype(S) - (mv(u).astype(S) - sig * u.astype(S))).astype(W)
    r1 = r2.copy()
    z = r2.astype(S) * dinv
    beta1 = np.sqrt(np.dot(r2.astype(S), z))
    stop = S(tol) * np.sqrt(np.dot(b.astype(S), b.astype(S) * dinv))
    done = not (beta1 > stop) or not (beta1 > 0)
    v = (z / beta1).astype(W) if not done else np.zeros(n, W)
    w, w2 = np.zeros(n, W), np.zeros(n, W)
    oldb, beta, dbar, epsln, phibar, cs, sn = S(0), beta1, S(0), S(0), beta1, S(-1), S(0)
    out, it = {}, 0
    last = max(tuple(ks) + (maxiter or 0,))
    for k in range(0, last + 1):
        if k > 0 and not done:
            t = mv(v).astype(S) - sig * v.astype(S)
            if it >= 1:
                t = t - (beta / oldb) * r1.astype(S)
            t = t.astype(W)
            alfa = np.dot(v.astype(S), t.astype(S))
            y = (t.astype(S) - (alfa / beta) * r2.astype(S)).astype(W)
            r1, r2 = r2, y
            z = y.astype(S) * dinv
            betan = np.sqrt(np.dot(y.astype(S), z))
            oldeps, delta, gbar = epsln, cs * dbar + sn * alfa, sn * dbar - cs * alfa
            epsln, dbar = sn * betan, -cs * betan
            gamma = max(np.sqrt(gbar * gbar + betan * betan), eps)
            cs, sn = gbar / gamma, betan / gamma
            phi, phibar = cs * phibar, sn * phibar
            wn = ((v.astype(S) - oldeps * w2.astype(S) - delta * w.astype(S)) / gamma).astype(W)
            w2, w = w, wn
            u = (u.astype(S) + phi * wn.astype(S)).astype(W)
            v = (z / betan).astype(W) if betan > 0 else np.zeros(n, W)
            oldb, beta, it = beta, betan, it + 1
            done = not (phibar > stop) or not (betan > 0)
        if k in ks:
            out[k] = (u.copy(), it)
        if done and maxiter is not None:
            break
    out["count"], out["u"] = it, u
    return out


def _native(A, b, torch, **kw):
    from cfs_spmv_amd.solver import minres_native
    u, it, res = minres_native(A, torch.from_numpy(b).cuda(), **kw)
    torch.cuda.synchronize()
    return u.cpu().numpy(), it, res


def _check_iterates(name, n, rp, ci, va, b, dtype, run, label="", ks=KS, **kw):
    """run(k) -> (u_k, iterations) on the GPU; asserts every k of ks against the long-double iterate"""
    ref = minres_reference(n, rp, ci, va, b, ks, **kw)
    work = minres_reference(n, rp, ci, va, b, ks, dtype, **kw)
    errors = []
    for k in ks:
        u_ref, it_ref = ref[k]
        d = _deviation(work[k][0], u_ref)
        assert d <= D_LIMIT[dtype], f"{name}: d_{k} = {d:.3e}: badly conditioned case"
        u, it = run(k)
        g = _deviation(u, u_ref)
        allowed = 4 * d + 16 * UNIT[dtype]
        print(f"minres-steps {np.dtype(dtype).name} {name}{label} n={n} k={k} d_k={d:.3e} gpu={g:.3e} allowed={allowed:.3e} it={it}")
        # fewer than k iterations only where the Lanczos beta can vanish: the Krylov space is exhausted
        if not (it == k if k < n else 1 <= it <= k):
            errors.append(f"k={k}: {it} iterations")
        if not g <= allowed:
            errors.append(f"k={k}: deviation {g:.3e} from the long-double iterate, allowed {allowed:.3e} (d_k = {d:.3e})")
    assert not errors, f"{name}{label} {np.dtype(dtype).name}: " + "; ".join(errors)


@DTYPES
@PRECONDS
@pytest.mark.parametrize("name", STEP_MATRICES)
def test_iterates_against_the_long_double_recurrence(name, precond, dtype):
    import torch
    import cfs_spmv_amd as cfs
    n, rp, ci, va = _case(name, dtype, precond)
    b = _rhs(n, dtype)
    A = cfs.SymMatrix(n, rp, ci, va)
    assert A.stats()["n"] == n and A.row_end - A.row_begin == n
    _check_iterates(name, n, rp, ci, va, b, dtype, lambda k: _native(A, b, torch, precond=precond, tol=0.0, maxiter=k)[:2],
                    label=f" {precond}", precond=precond)
    A.close()


@DTYPES
@PRECONDS
@pytest.mark.parametrize("name", ["rand1023", "band20001"])
def test_iterates_with_a_shift_inside_the_spectrum(name, precond, dtype):
    """the SPD matrices of the plain test minus 3 I: indefinite; band20001 from a nonzero first guess"""
    import torch
    import cfs_spmv_amd as cfs
    shift = 3.0
    n, rp, ci, va = _case(name, dtype, precond, sign=False)
    b = _rhs(n, dtype)
    x0 = np.random.default_rng(4).uniform(-1, 1, n).astype(dtype) if name == "band20001" else None
    A = cfs.SymMatrix(n, rp, ci, va)

    def run(k):
        kw = {} if x0 is None else dict(x0=torch.from_numpy(x0).cuda())
        return _native(A, b, torch, precond=precond, shift=shift, tol=0.0, maxiter=k, **kw)[:2]
    _check_iterates(name, n, rp, ci, va, b, dtype, run, label=f" {precond} shift={shift}", precond=precond, shift=shift, x0=x0)
    A.close()


@DTYPES
@PRECONDS
def test_iterates_through_a_two_shard_handle(precond, dtype):
    """an odd n through a multi-device handle (two shards, here on one device): the diagonal gathered and the
    products computed on the shards' streams, the vector kernels on the caller's"""
    import torch
    import cfs_spmv_amd as cfs
    n, rp, ci, va = _case("band20001", dtype, precond)
    b = _rhs(n, dtype)
    M = cfs.SymMatrix(n, rp, ci, va, ngpus=2)
    _check_iterates("band20001", n, rp, ci, va, b, dtype, lambda k: _native(M, b, torch, precond=precond, tol=0.0, maxiter=k)[:2],
                    label=f" {precond} (two shards)", precond=precond)
    M.close()


@DTYPES
@PRECONDS
def test_a_deterministic_handle_is_bit_reproducible(precond, dtype):
    import torch
    import cfs_spmv_amd as cfs
    n, rp, ci, va = _case("Flan_1565@0.01", dtype, precond)
    b = _rhs(n, dtype)
    D = cfs.SymMatrix(n, rp, ci, va, options=cfs.make_options(flags=DET))
    assert D.kernel_variant()["det"] == 1
    _check_iterates("Flan_1565@0.01", n, rp, ci, va, b, dtype,
                    lambda k: _native(D, b, torch, precond=precond, tol=0.0, maxiter=k)[:2],
                    label=f" {precond} (deterministic)", precond=precond)
    # the whole solve is bit-reproducible, whatever the window of enqueued iterations
    ua, ita, _ = _native(D, b, torch, precond=precond, tol=0.0, maxiter=12)
    ub, itb, _ = _native(D, b, torch, precond=precond, tol=0.0, maxiter=12, check_every=5)
    assert ita == itb == 12 and np.array_equal(ua.view(np.uint8), ub.view(np.uint8))
    # ... and the iterations enqueued behind the converged one change neither u nor the count
    tol = 1e-8 if dtype == np.float64 else 1e-4
    u1, it1, res1 = _native(D, b, torch, precond=precond, tol=tol, maxiter=3000, check_every=1)
    print(f"minres-steps {np.dtype(dtype).name} Flan_1565@0.01 {precond} (deterministic): {it1} iterations, relres {res1:.3e}")
    assert 4 < it1 < 3000
    windows = [c for c in (3, 5, 7, 16) if it1 % c]  # the converged iteration is not the last of its window
    assert len(windows) >= 2, it1
    for check_every in windows[:2]:
        u2, it2, res2 = _native(D, b, torch, precond=precond, tol=tol, maxiter=3000, check_every=check_every)
        assert it2 == it1 and res2 == res1 and np.array_equal(u2.view(np.uint8), u1.view(np.uint8)), (check_every, it1, it2)
    D.close()


def _saddle(dtype):
    """A = [[0, K], [K, 0]], K = banded_spd(10000, 3, 1): n = 20 000, no diagonal stored;  b = [f; 0]"""
    import scipy.sparse as sp
    m, rp, ci, va = banded_spd(10000, 3, 1)
    K = sp.csr_matrix((va, ci, rp), shape=(m, m))
    A = sp.bmat([[None, K], [K, None]]).tocsr()
    A.sort_indices()
    assert not A.diagonal().any() and abs(A - A.T).max() == 0
    b = np.concatenate([np.random.default_rng(8).uniform(-1, 1, m), np.zeros(m)]).astype(dtype)
    return 2 * m, A.indptr.astype(np.int32), A.indices.astype(np.int32), A.data.astype(dtype), b


@DTYPES
def test_what_it_is_for(dtype):
    """a saddle-point matrix with a zero diagonal: MINRES converges in the count J the working-precision recurrence
    takes on the CPU (when written: 98 in fp64 at tol 1e-8, 48 in fp32 at tol 1e-4), cfs_hip_sym_cg does nothing at
    all -- its first p.q is an exact floating-point zero, alpha = 0, u stays 0 -- and Jacobi is refused."""
    import torch
    import cfs_spmv_amd as cfs
    from cfs_spmv_amd import _lib
    from cfs_spmv_amd.solver import cg_native
    n, rp, ci, va, b = _saddle(dtype)
    tol = 1e-8 if dtype == np.float64 else 1e-4
    J = minres_reference(n, rp, ci, va, b, dtype=dtype, tol=tol, maxiter=400)["count"]
    print(f"minres-steps {np.dtype(dtype).name} saddle n={n}: {J} iterations (CPU)")
    assert 20 <= J < 400, f"badly chosen case: {J} iterations"
    A = cfs.SymMatrix(n, rp, ci, va)
    u, it, res = _native(A, b, torch, tol=tol, maxiter=400)
    true, slack = _relres(n, rp, ci, va, b, u, dtype)
    print(f"minres-steps {np.dtype(dtype).name} saddle: GPU {it} iterations, relres {res:.3e} (long double {true:.3e}, slack {slack:.3e})")
    assert J - 2 <= it <= J + 2, (J, it)
    assert res <= 10 * tol and abs(res - true) <= slack
    bd = torch.from_numpy(b).cuda()
    uc, itc, resc = cg_native(A, bd, tol=tol, maxiter=50)
    torch.cuda.synchronize()
    assert not uc.cpu().numpy().any() and resc == 1.0, (itc, resc)
    # Jacobi: there is no diagonal
    x0 = np.random.default_rng(5).uniform(-1, 1, n).astype(dtype)
    ud = torch.from_numpy(x0).cuda()
    with pytest.raises(_lib.CfsHipError, match="nonzero diagonal") as e:
        A.minres(ud, bd, precond="jacobi", tol=tol, maxiter=50)
    assert e.value.code == _lib.ERR_ARG
    itr, rr = C.c_int(9), C.c_double(9.0)
    rc = _lib.load().cfs_hip_sym_minres(A._h, ud.data_ptr(), bd.data_ptr(), _lib.PRECOND_JACOBI, 0.0, tol, 50, 8, C.byref(itr),
                                        C.byref(rr), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert rc == _lib.ERR_ARG and itr.value == 0 and b"nonzero diagonal" in _lib.load().cfs_hip_last_error()
    assert np.array_equal(ud.cpu().numpy().view(np.uint8), x0.view(np.uint8))
    A.close()


@DTYPES
def test_jacobi_pays_for_itself(dtype):
    """rows of very different scale and a diagonal of both signs: the CPU recurrences in the working precision take
    J iterations with M = |diag(A)| and more than 5 J without (when written: 66 against 661 in fp64 at tol 1e-8, 32
    against 321 in fp32 at tol 1e-4); the GPU must reproduce J within +-2 and still be unconverged without the
    preconditioner after 5 J iterations."""
    import torch
    import cfs_spmv_amd as cfs
    n, rp, ci, va = _case("band20001", dtype, "jacobi")
    b = np.random.default_rng(8).uniform(-1, 1, n).astype(dtype)
    tol = 1e-8 if dtype == np.float64 else 1e-4
    J = minres_reference(n, rp, ci, va, b, dtype=dtype, precond="jacobi", tol=tol, maxiter=2000)["count"]
    plain = minres_reference(n, rp, ci, va, b, dtype=dtype, tol=tol, maxiter=5 * J + 1)["count"]
    print(f"minres-steps {np.dtype(dtype).name} band20001 signed, scaled: Jacobi {J} iterations, none more than {plain - 1} (CPU)")
    assert 5 <= J < 400 and plain > 5 * J, f"badly chosen case: {plain} iterations without, {J} with Jacobi"
    A = cfs.SymMatrix(n, rp, ci, va)
    u, it, res = _native(A, b, torch, precond="jacobi", tol=tol, maxiter=2000)
    print(f"minres-steps {np.dtype(dtype).name} band20001 signed, scaled: GPU Jacobi {it} iterations, relres {res:.3e}")
    assert J - 2 <= it <= J + 2, (J, it)
    up, itp, resp = _native(A, b, torch, tol=tol, maxiter=5 * J)
    print(f"minres-steps {np.dtype(dtype).name} band20001 signed, scaled: GPU none relres {resp:.3e} after {itp} iterations")
    assert itp == 5 * J and resp > tol
    A.close()


def test_the_residual_never_increases():
    """||b - A u_k|| of the returned u_k for k = 0 .. 12, within what the recomputed residual may be off by"""
    import torch
    import cfs_spmv_amd as cfs
    dtype = np.float64
    n, rp, ci, va = _case("pwtk@0.05", dtype, "none")
    b = _rhs(n, dtype)
    A = cfs.SymMatrix(n, rp, ci, va)
    res, slack = [], []
    for k in range(13):
        u, it, r = _native(A, b, torch, tol=0.0, maxiter=k)
        assert it == k
        res.append(r)
        slack.append(_relres(n, rp, ci, va, b, u, dtype)[1])
    print("minres-steps float64 pwtk@0.05 signed: relres " + " ".join(f"{r:.6e}" for r in res))
    assert res[12] < res[0]
    for k in range(12):
        assert res[k + 1] <= res[k] + slack[k] + slack[k + 1], (k, res[k], res[k + 1])
    A.close()


@DTYPES
def test_iteration_count_and_reported_residual(dtype):
    import torch
    import cfs_spmv_amd as cfs
    shift = 0.5
    n, rp, ci, va = _case("pwtk@0.05", dtype, "jacobi")
    b = _rhs(n, dtype)
    A = cfs.SymMatrix(n, rp, ci, va)
    kw = dict(precond="jacobi", shift=shift)
    # tol = 0: exactly maxiter iterations, whatever the window of enqueued iterations
    for check_every, k in ((1, 7), (3, 23), (16, 23), (1000, 23), (16, 40)):
        u, it, res = _native(A, b, torch, tol=0.0, maxiter=k, check_every=check_every, **kw)
        assert it == k, (check_every, k, it)
        true, slack = _relres(n, rp, ci, va, b, u, dtype, shift)
        print(f"minres-steps {np.dtype(dtype).name} relres k={k} reported={res:.6e} long double={true:.6e} slack={slack:.3e}")
        assert abs(res - true) <= slack, (k, res, true, slack)
    # maxiter = 0: u untouched, the residual of the first guess
    x0 = np.random.default_rng(4).uniform(-1, 1, n).astype(dtype)
    u, it, res = _native(A, b, torch, tol=0.0, maxiter=0, x0=torch.from_numpy(x0).cuda(), **kw)
    true, slack = _relres(n, rp, ci, va, b, x0, dtype, shift)
    assert it == 0 and np.array_equal(u.view(np.uint8), x0.view(np.uint8)) and abs(res - true) <= slack
    # b = 0 (and u = 0): nothing to do
    u, it, res = _native(A, np.zeros(n, dtype), torch, tol=1e-8, maxiter=50, **kw)
    assert it == 0 and not u.any() and np.isfinite(res)
    # a first guess that already solves the system: at most one iteration
    tol = 1e-10 if dtype == np.float64 else 1e-5
    us, its, ress = _native(A, b, torch, tol=tol, maxiter=3000, **kw)
    print(f"minres-steps {np.dtype(dtype).name} pwtk@0.05 signed, scaled, shift={shift}: {its} iterations, relres {ress:.3e}")
    assert 0 < its < 3000
    u, it, res = _native(A, b, torch, tol=10 * tol, maxiter=3000, x0=torch.from_numpy(us).cuda(), **kw)
    assert it <= 1, it
    A.close()


@DTYPES
@PRECONDS
def test_nan_in_b_ends_the_solve_at_once(precond, dtype):
    import torch
    import cfs_spmv_amd as cfs
    n, rp, ci, va = _case("rand1023", dtype, precond)
    b = _rhs(n, dtype)
    b[n // 2] = np.nan
    A = cfs.SymMatrix(n, rp, ci, va)
    for check_every in (1, 16):
        u, it, res = _native(A, b, torch, precond=precond, tol=1e-8, maxiter=300, check_every=check_every)
        assert it <= 1 and np.isnan(res), (it, res)
    A.close()


@DTYPES
def test_argument_checks(dtype):
    import torch
    import cfs_spmv_amd as cfs
    from cfs_spmv_amd import _lib
    n, rp, ci, va = _matrix("rand1023")
    va = va.astype(dtype)
    rows = np.repeat(np.arange(n), np.diff(rp))
    va[int(np.flatnonzero((rows == ci) & (rows == 700))[0])] = 3.0  # |a_ii - shift| = 0 at shift = 3
    A = cfs.SymMatrix(n, rp, ci, va)
    big = torch.zeros(n + 4, dtype=torch.from_numpy(va).dtype, device="cuda")
    good = torch.zeros(n, dtype=big.dtype, device="cuda")
    assert good.data_ptr() % 16 == 0 and big[1:n + 1].data_ptr() % 16 != 0

    def refused(code, *args, **kw):
        with pytest.raises(_lib.CfsHipError) as e:
            A.minres(*args, **dict(dict(tol=1e-8, maxiter=5), **kw))
        assert e.value.code == code, (args, kw, e.value)
        return str(e.value)
    refused(_lib.ERR_ARG, big[1:n + 1], good)
    refused(_lib.ERR_ARG, good, big[1:n + 1])
    refused(_lib.ERR_ARG, good, good)  # one vector for both
    refused(_lib.ERR_ARG, np.zeros(n, dtype), good)  # a host pointer
    refused(_lib.ERR_ARG, good, np.zeros(n, dtype))
    assert "unknown preconditioner" in refused(_lib.ERR_ARG, good, good.clone(), precond=2)
    with pytest.raises(ValueError):
        A.minres(good, good.clone(), precond="ilu")
    assert "shift" in refused(_lib.ERR_ARG, good, good.clone(), shift=float("nan"))
    # a zero of diag(A) - shift I: refused with Jacobi, u untouched; solved without
    b = torch.from_numpy(_rhs(n, dtype)).cuda()
    x0 = np.random.default_rng(5).uniform(-1, 1, n).astype(dtype)
    u = torch.from_numpy(x0).cuda()
    assert "nonzero diagonal" in refused(_lib.ERR_ARG, u, b, precond="jacobi", shift=3.0, maxiter=50)
    torch.cuda.synchronize()
    assert np.array_equal(u.cpu().numpy().view(np.uint8), x0.view(np.uint8))
    it, res = A.minres(u, b, precond="jacobi", shift=0.0, tol=0.0, maxiter=3)  # (the same diagonal, another shift)
    assert it == 3
    tol = 1e-8 if dtype == np.float64 else 1e-4
    u = torch.zeros_like(b)
    it, res = A.minres(u, b, precond="none", shift=3.0, tol=tol, maxiter=10000)  # (2 328 / 2 668 on the CPU)
    torch.cuda.synchronize()
    true, slack = _relres(n, rp, ci, va, b.cpu().numpy(), u.cpu().numpy(), dtype, 3.0)
    print(f"minres-steps {np.dtype(dtype).name} rand1023 - 3 I: {it} iterations, relres {res:.3e} (long double {true:.3e})")
    assert 0 < it < 10000 and res <= 10 * tol and abs(res - true) <= slack
    A.close()
    S = cfs.SymMatrix(n, rp, ci, va, row_splits=np.array([0, n // 2, n], np.int32), rank=1)
    for precond in ("jacobi", "none"):
        with pytest.raises(_lib.CfsHipError) as e:
            S.minres(good, good.clone(), precond=precond, tol=1e-8, maxiter=5)
        assert e.value.code == _lib.ERR_UNSUPPORTED
    S.close()


@DTYPES
def test_host_driven_and_native_loops_agree(dtype):
    """solver.minres (torch-driven) against solver.minres_native on the signed pwtk stand-in: iteration counts within
    +-2, both answers within the bound test_gpu_pcg_steps.py holds the PCG pair to against a direct solve"""
    import scipy.sparse as sp
    import scipy.sparse.linalg as spl
    import torch
    import cfs_spmv_amd as cfs
    from cfs_spmv_amd import synth
    from cfs_spmv_amd.solver import minres, minres_native
    n, rp, ci, va = _case("pwtk@0.05", dtype, "none")
    A = cfs.SymMatrix(n, rp, ci, va)
    b = synth.make_x(n, 11, dtype)
    bd = torch.from_numpy(b).cuda()
    tol, lim = (1e-11, 1e-9) if dtype == np.float64 else (2e-5, 2e-3)
    u_ref = spl.spsolve(sp.csc_matrix(sp.csr_matrix((va.astype(np.float64), ci, rp), shape=(n, n))), b.astype(np.float64))
    for precond in ("none", "jacobi"):
        u1, it1, res1 = minres(A, bd, precond=precond, tol=tol, maxiter=3000)
        torch.cuda.synchronize()
        assert 0 < it1 < 3000 and res1 <= 10 * tol, (precond, it1, res1)
        assert np.max(np.abs(u1.cpu().numpy() - u_ref)) <= lim * np.max(np.abs(u_ref))
        for check_every in (1, 8, 1000):
            u2, it2, res2 = minres_native(A, bd, precond=precond, tol=tol, maxiter=3000, check_every=check_every)
            torch.cuda.synchronize()
            print(f"minres-steps {np.dtype(dtype).name} pwtk@0.05 signed {precond}: host-driven {it1} iterations, native {it2} "
                  f"(check_every={check_every})")
            assert 0 < it2 < 3000 and abs(it2 - it1) <= 2, (it1, it2, check_every)
            assert res2 <= 10 * tol, (res1, res2)
            assert np.max(np.abs(u2.cpu().numpy() - u_ref)) <= lim * np.max(np.abs(u_ref))
            assert np.max(np.abs(u2.cpu().numpy() - u1.cpu().numpy())) <= 2 * lim * np.max(np.abs(u_ref))
    A.close()
