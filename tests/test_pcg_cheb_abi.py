"""cfs_hip_sym_pcg_cheb, cfs_hip_sym_cheb_apply, cfs_hip_sym_precond_lmax and cfs_hip_debug_cheb_coeffs without a
GPU, by the method of test_pcg_abi.py: the library exports them, the ctypes binding declares them, their argument
checks answer before anything touches a device -- and the coefficients the solver passes to its inner steps are
those of the Chebyshev iteration:

  against the formula (theta = (lmax + lmin) / 2, delta = (lmax - lmin) / 2, sigma1 = theta / delta, rho_0 = 1 /
  sigma1, rho_j = 1 / (2 sigma1 - rho_{j-1}), c1 = rho_j rho_{j-1}, c2 = 2 rho_j / delta) in np.longdouble.  The
  library works in fp64 (u = 2^-53): theta, delta and their quotient give sigma1 to 3 u; the denominator 2 sigma1 -
  rho_{j-1} is above 1 and rho_j below 1, so the absolute error e_j of rho_j obeys e_j <= rho_j^2 (6 sigma1 u +
  e_{j-1}) + 2 u rho_j <= e_{j-1} + (6 sigma1 + 2) u with e_0 <= 4 u -- no contraction is assumed (near sigma1 = 1
  there is none): e_j <= (j (6 sigma1 + 2) + 4) u.  A product or quotient adds the relative errors and one rounding:
  c1_j and c2_j are allowed ((2 j (6 sigma1 + 2) + 8) / rho_j + 4) u relative, at most 5e-14 over these cases.

  by running the scalar recurrence z_1 = d_1 = 1 / theta, d_{j+1} = c1 d_j + c2 (1 - lambda z_j), z_{j+1} = z_j +
  d_{j+1} (M = 1, A = lambda, r = 1) with the LIBRARY's coefficients in long double on lambda across (0, lmin +
  lmax): 1 - lambda z_m = T_m((theta - lambda) / delta) / T_m(sigma1) to 1e-12 (the worst deviation when this was
  written: 1.2e-14), and lambda z_m > 0 on the whole open interval -- the margin inside which the polynomial is
  positive definite."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import cfs_spmv_amd as cfs
from cfs_spmv_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("cfs_hip_sym_pcg_cheb", "cfs_hip_sym_cheb_apply", "cfs_hip_sym_precond_lmax", "cfs_hip_debug_cheb_coeffs")
DEGREES = (1, 2, 3, 5, 8, 16)
BOUNDS = ((0.1, 2.0), (2.0 / 30.0, 2.0), (1e-3, 7.5))
LD = np.longdouble


def test_the_four_symbols_are_declared_exported_and_bound():
    text = open(os.path.join(ROOT, "include", "cfs_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    lib = cfs.load()
    raw = C.CDLL(cfs.lib_path())
    for name in NEW:
        assert re.search(r"\bint\s+" + name + r"\s*\(", code), f"{name} is not declared in cfs_hip.h"
        assert name in _lib.SYMBOLS
        getattr(raw, name)  # dlsym
    assert re.search(r"#define\s+CFS_HIP_ABI_VERSION\s+4\b", code) and lib.cfs_hip_abi_version() == 4
    vp, ip, dp, i, d = C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_double), C.c_int, C.c_double
    assert lib.cfs_hip_sym_pcg_cheb.argtypes == [vp, vp, vp, i, i, d, d, d, i, i, ip, dp, dp, vp]
    assert lib.cfs_hip_sym_cheb_apply.argtypes == [vp, i, i, d, d, vp, vp, vp]
    assert lib.cfs_hip_sym_precond_lmax.argtypes == [vp, i, i, vp, dp, vp]
    assert lib.cfs_hip_debug_cheb_coeffs.argtypes == [i, d, d, dp, dp, dp]
    # the Python mirror
    for name in ("pcg_cheb", "cheb_apply", "precond_lmax"):
        assert callable(getattr(cfs.SymMatrix, name))
    from cfs_spmv_amd import solver
    assert callable(solver.pcg_cheb) and callable(solver.pcg_cheb_native)


def test_argument_checks_answer_before_any_device_work():
    lib = cfs.load()
    bound = lib.cfs_hip_runtime_bound()
    it, res = C.c_int(7), C.c_double(7.0)
    used = (C.c_double * 2)(7.0, 7.0)
    est = C.c_double(7.0)
    # (a non-null handle that is never dereferenced: every check below comes before the handle is looked at)
    fake, vec, vec2 = C.c_void_p(0x1000), C.c_void_p(0x2000), C.c_void_p(0x3000)

    def solve(h=fake, u=vec, b=vec2, block_rows=1, degree=4, lmin=0.0, lmax=0.0, tol=1e-8, maxiter=10):
        return lib.cfs_hip_sym_pcg_cheb(h, u, b, block_rows, degree, lmin, lmax, tol, maxiter, 8, C.byref(it), C.byref(res),
                                        used, None)

    def apply(h=fake, z=vec, r=vec2, block_rows=1, degree=4, lmin=0.1, lmax=2.0):
        return lib.cfs_hip_sym_cheb_apply(h, block_rows, degree, lmin, lmax, z, r, None)

    for h, u, b in ((None, vec, vec2), (fake, None, vec2), (fake, vec, None), (None, None, None)):
        # (null comes first: the other arguments are bad as well)
        assert solve(h, u, b, block_rows=5, degree=0, lmin=np.nan) == _lib.ERR_ARG and b"null" in lib.cfs_hip_last_error()
        assert apply(h, u, b, block_rows=5, degree=0) == _lib.ERR_ARG and b"null" in lib.cfs_hip_last_error()
    for h, e in ((None, C.byref(est)), (fake, None)):
        assert lib.cfs_hip_sym_precond_lmax(h, 1, 16, None, e, None) == _lib.ERR_ARG and b"null" in lib.cfs_hip_last_error()
    assert lib.cfs_hip_sym_precond_lmax(fake, 5, 16, None, C.byref(est), None) == _lib.ERR_ARG
    assert b"block_rows" in lib.cfs_hip_last_error() and est.value == 0.0
    bad = [(dict(b=vec), b"different"), (dict(u=C.c_void_p(0x2008)), b"aligned"), (dict(b=C.c_void_p(0x3004)), b"aligned"),
           (dict(tol=-1e-8), b"tolerance"), (dict(tol=np.nan), b"tolerance"), (dict(maxiter=-1), b"iteration limit"),
           (dict(degree=0), b"degree"), (dict(degree=17), b"degree"), (dict(degree=-3), b"degree"),
           (dict(block_rows=5), b"block_rows"), (dict(block_rows=-1), b"block_rows"), (dict(block_rows=8), b"block_rows"),
           (dict(lmax=np.inf), b"finite"), (dict(lmin=np.nan), b"finite"), (dict(lmax=np.nan, lmin=0.1), b"finite"),
           (dict(lmin=2.0, lmax=2.0), b"not below"), (dict(lmin=3.0, lmax=2.0), b"not below")]
    for kw, word in bad:
        it.value = 7
        assert solve(**kw) == _lib.ERR_ARG, kw
        assert word in lib.cfs_hip_last_error(), (kw, lib.cfs_hip_last_error())
        assert it.value == 0 and used[0] == 7.0 and used[1] == 7.0
    for kw, word in ((dict(r=vec), b"different"), (dict(z=C.c_void_p(0x2008)), b"aligned"), (dict(degree=0), b"degree"),
                     (dict(degree=17), b"degree"), (dict(block_rows=7), b"block_rows"), (dict(lmin=0.0), b"both bounds"),
                     (dict(lmax=0.0), b"both bounds"), (dict(lmax=-2.0), b"both bounds"), (dict(lmax=np.inf), b"finite"),
                     (dict(lmin=2.0), b"not below"), (dict(lmin=2.5), b"not below")):
        assert apply(**kw) == _lib.ERR_ARG, kw
        assert word in lib.cfs_hip_last_error(), (kw, lib.cfs_hip_last_error())
    th = C.c_double()
    c = (C.c_double * 16)()
    for args in ((0, 0.1, 2.0), (17, 0.1, 2.0), (4, 0.0, 2.0), (4, 0.1, 0.0), (4, 2.0, 2.0), (4, 0.1, np.inf), (4, np.nan, 2.0)):
        assert lib.cfs_hip_debug_cheb_coeffs(*args, C.byref(th), c, c) == _lib.ERR_ARG, args
    assert lib.cfs_hip_debug_cheb_coeffs(4, 0.1, 2.0, None, c, c) == _lib.ERR_ARG
    assert lib.cfs_hip_debug_cheb_coeffs(4, 0.1, 2.0, C.byref(th), None, c) == _lib.ERR_ARG
    assert lib.cfs_hip_debug_cheb_coeffs(1, 0.1, 2.0, C.byref(th), None, None) == 0 and th.value == 1.05
    assert lib.cfs_hip_runtime_bound() == bound  # nothing above initialised the runtime


def _coeffs(m, lmin, lmax):
    lib = cfs.load()
    th = C.c_double()
    c1, c2 = np.full(16, np.nan), np.full(16, np.nan)
    dp = C.POINTER(C.c_double)
    assert lib.cfs_hip_debug_cheb_coeffs(m, lmin, lmax, C.byref(th), c1.ctypes.data_as(dp), c2.ctypes.data_as(dp)) == 0
    assert np.all(np.isnan(c1[m - 1:])) and np.all(np.isnan(c2[m - 1:]))  # degree - 1 pairs and nothing behind them
    return th.value, c1[:m - 1], c2[:m - 1]


def _cheb_t(m, x):
    """T_m(x) in long double by the three-term recurrence (any real x)"""
    a, b = np.ones_like(x), x
    if m == 0:
        return a
    for _ in range(m - 1):
        a, b = b, 2 * x * b - a
    return b


@pytest.mark.parametrize("lmin,lmax", BOUNDS)
@pytest.mark.parametrize("m", DEGREES)
def test_coefficients_against_the_formula_in_long_double(m, lmin, lmax):
    theta, c1, c2 = _coeffs(m, lmin, lmax)
    lo, hi = LD(lmin), LD(lmax)
    th, de = (hi + lo) / 2, (hi - lo) / 2
    s1 = th / de
    rho = 1 / s1
    u = LD(2.0) ** -53
    assert abs(LD(theta) - th) <= 2 * u * th
    for j in range(1, m):
        rn = 1 / (2 * s1 - rho)
        tol = ((2 * j * (6 * s1 + 2) + 8) / rn + 4) * u
        assert tol <= 5e-14
        assert abs(LD(c1[j - 1]) - rn * rho) <= tol * rn * rho, (j, c1[j - 1], rn * rho)
        assert abs(LD(c2[j - 1]) - 2 * rn / de) <= tol * 2 * rn / de, (j, c2[j - 1], 2 * rn / de)
        rho = rn
    # ... and the Python mirror of the host-driven solver computes the same bits
    from cfs_spmv_amd.solver import cheb_coeffs
    th2, pairs = cheb_coeffs(m, lmin, lmax)
    assert th2 == theta and [p[0] for p in pairs] == list(c1) and [p[1] for p in pairs] == list(c2)


@pytest.mark.parametrize("lmin,lmax", BOUNDS)
@pytest.mark.parametrize("m", DEGREES)
def test_the_scalar_recurrence_is_the_chebyshev_residual_polynomial(m, lmin, lmax):
    theta, c1, c2 = _coeffs(m, lmin, lmax)
    th, de = (LD(lmax) + LD(lmin)) / 2, (LD(lmax) - LD(lmin)) / 2
    top = LD(lmin) + LD(lmax)
    # the open interval (0, lmin + lmax): a fine grid, and points hard against both ends
    edge = np.array([1e-12, 1e-9, 1e-6, 1e-3], LD)
    lam = np.concatenate([top * edge, top * np.linspace(LD(0), LD(1), 4003)[1:-1], top * (1 - edge)]).astype(LD)
    assert lam.min() > 0 and lam.max() < top
    d = np.full_like(lam, 1 / LD(theta))
    z = d.copy()
    for a, b in zip(c1, c2):
        d = LD(a) * d + LD(b) * (1 - lam * z)
        z = z + d
    want = _cheb_t(m, (th - lam) / de) / _cheb_t(m, np.array([th / de], LD))[0]
    err = float(np.max(np.abs((1 - lam * z) - want)))
    print(f"cheb-coeffs m={m} [{lmin}, {lmax}]: worst deviation from T_m((theta-l)/delta)/T_m(sigma1) {err:.2e}")
    assert err <= 1e-12, err
    assert np.all(np.abs(want) < 1)  # the margin: |residual polynomial| < 1 on the whole open interval ...
    assert np.all(lam * z > 0), float(np.min(lam * z))  # ... so lambda p(lambda) > 0 there
