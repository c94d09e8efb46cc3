"""The three dense kernels of cfs_hip_sym_lobpcg in the forms the SOLVER launches them in, on the GPU: the Gram kernel with
a column list and the triangle-only task table (cfs_hip_debug_gram_cols), the update kernel with a dense C, lists with
holes, with_p = 0 and the second block (cfs_hip_debug_lobpcg_update_cols), the fused residual / preconditioner kernel alone
at every block size (cfs_hip_sym_debug_lobpcg_residual) -- and whole solves at the block sizes 2, 4 and 6.  Inputs are
uniform(-1, 1) in the value type; references are evaluated in np.longdouble from the stored values.

Lists.  solver_lists(): [0 .. k) + the active W_i (+ the active P_i) for k = 1, 2, 8, 16 and the masks all / one pair /
alternating / all but the first, without P (iteration 1) and with it: m in {1, 2, 3, 4, 6, 9, 10, 12, 15, 16, 17, 18, 22,
24, 31, 32, 46, 48}.  Equal W and P sets cannot give an odd m - k, so the widths 5, 7, 23, 33, 41, 47 -- and 40, the
third of the widths at which the triangle-only table has another number of row slices (m = 24: 4 against 6, m = 32: 2
against 3, m = 40: 1 against 2) -- come from width_lists(): X whole, then a seeded choice among the W and P columns,
ascending.  One list is a non-ascending permutation.

Gram.  On an n x 48 block whose unlisted columns are NaN, the call with a list and full_h = 1 must give the bits of
cfs_hip_debug_gram on a contiguous copy of the listed columns (the order of summation depends on (n, m, full_h) alone; a
NaN proves that an unlisted column was read).  With full_h = 0 every upper-triangle entry of G and H must lie within

    (n + 1) 2^-53 sum_r |s_ri| |t_rj|        (the a-priori bound of test_gpu_lobpcg_steps.py)

of the long-double value, the lower triangles must carry the bits of the upper ones, and two calls must give equal bits.
Integer blocks (-8 .. 8) with full_h = 0 and a holed list must be exact.  n = 600001 (beyond one sweep of 512 workgroups)
on a block of 6 columns, k = 2.

Update.  Dense uniform(-1, 1) fp64 C.  Every written value must have the bits of the documented order restated in numpy
fp64 -- acc = 0; for j ascending: acc = acc + a_j c_jo, a separate multiply and add; one cast to V -- and lie within

    gamma_m A + u_V (|ref| + gamma_m A) + (m + 1) 2^-64 A,    A = sum_j |a_j| |c_jo|,  gamma_m = m u / (1 - m u),  u = 2^-53

of the long-double value ref: m products and m adds in fp64 (the textbook bound of a dot product of m terms in any
order), one rounding to V (u_V = 2^-24 for fp32, and 0 for fp64, whose cast is the identity), and the reference's own
rounding.  W, the P columns with with_p = 0, and the words of the rows [n, ld) must keep their bits (they hold NaNs with
distinct payloads where they are not inputs); with_p = 1 writes ALL k columns of P.  The second block holds other data,
gets the same C and is checked the same way; one form per case passes as_dev = NULL.

Residual.  d_r = ax_r - theta x_r in fp64 (two roundings), rho_r = |ax_r| + |theta| |x_r|:  |d_r - exact| <= (2 u + u^2)
rho_r.  z_i = sum_j m_ij d_j over the B = block_rows entries of a node block, B products and B adds in fp64, contracted
or not: |z_i - sum_j m_ij d_j| <= gamma_B sum_j |m_ij| |d_j| and |d_j| <= (1 + 2 u + u^2) rho_j, so with
q = (|M^-1| rho)_i

    |z_i - exact_i| <= E_i = ((2 u + u^2) + gamma_B (1 + 2 u + u^2)) q        (gamma_0 = 0: no product)

and W_i = (V) z_i lies within E_i + u_V (|exact_i| + E_i) + (B + 2) 2^-64 q of the long-double value (the last term: the
reference's own rounding).  Inactive W_i and the rows [n, ld) keep their NaN payloads.  The sums: the terms d_r^2 and
x_r^2 of the fp64 d_r above, added in long double; the kernel's fp64 sum of n products in any order lies within
(n + 1) 2^-53 sum |term| of that, for all k pairs whatever the mask.  Integer X, AX and theta with block_rows = 0 give
exact W bits and exact sums.

Measured on the MI355X (worst error / bound):

  gram-triangles float64 n=1: worst error / bound 0.495
  gram-triangles float32 n=1: worst error / bound 0.000
  gram-triangles float64 n=2: worst error / bound 0.543
  gram-triangles float32 n=2: worst error / bound 0.245
  gram-triangles float64 n=63: worst error / bound 0.087
  gram-triangles float32 n=63: worst error / bound 0.048
  gram-triangles float64 n=65: worst error / bound 0.076
  gram-triangles float32 n=65: worst error / bound 0.076
  gram-triangles float64 n=257: worst error / bound 0.019
  gram-triangles float32 n=257: worst error / bound 0.026
  gram-triangles float64 n=1023: worst error / bound 0.002
  gram-triangles float32 n=1023: worst error / bound 0.003
  gram-triangles float64 n=20001: worst error / bound 0.000
  gram-triangles float32 n=20001: worst error / bound 0.000
  gram-triangles float64 n=600001: worst error / bound 0.000
  gram-triangles float32 n=600001: worst error / bound 0.000
  update float64 n=1 k=1: worst error / bound 0.596
  update float32 n=1 k=1: worst error / bound 0.772
  update float64 n=1 k=4: worst error / bound 0.235
  update float32 n=1 k=4: worst error / bound 0.882
  update float64 n=1 k=16: worst error / bound 0.106
  update float32 n=1 k=16: worst error / bound 0.935
  update float64 n=31 k=1: worst error / bound 0.883
  update float32 n=31 k=1: worst error / bound 0.980
  update float64 n=31 k=4: worst error / bound 0.414
  update float32 n=31 k=4: worst error / bound 0.977
  update float64 n=31 k=16: worst error / bound 0.154
  update float32 n=31 k=16: worst error / bound 0.989
  update float64 n=33 k=1: worst error / bound 0.965
  update float32 n=33 k=1: worst error / bound 0.969
  update float64 n=33 k=4: worst error / bound 0.392
  update float32 n=33 k=4: worst error / bound 0.966
  update float64 n=33 k=16: worst error / bound 0.139
  update float32 n=33 k=16: worst error / bound 0.992
  update float64 n=63 k=1: worst error / bound 0.980
  update float32 n=63 k=1: worst error / bound 0.976
  update float64 n=63 k=4: worst error / bound 0.434
  update float32 n=63 k=4: worst error / bound 0.991
  update float64 n=63 k=16: worst error / bound 0.162
  update float32 n=63 k=16: worst error / bound 0.990
  update float64 n=65 k=1: worst error / bound 0.896
  update float32 n=65 k=1: worst error / bound 0.950
  update float64 n=65 k=4: worst error / bound 0.454
  update float32 n=65 k=4: worst error / bound 0.988
  update float64 n=65 k=16: worst error / bound 0.167
  update float32 n=65 k=16: worst error / bound 0.984
  update float64 n=257 k=1: worst error / bound 0.949
  update float32 n=257 k=1: worst error / bound 0.987
  update float64 n=257 k=4: worst error / bound 0.495
  update float32 n=257 k=4: worst error / bound 0.989
  update float64 n=257 k=16: worst error / bound 0.182
  update float32 n=257 k=16: worst error / bound 0.996
  update float64 n=20001 k=1: worst error / bound 0.998
  update float32 n=20001 k=1: worst error / bound 0.999
  update float64 n=20001 k=4: worst error / bound 0.752
  update float32 n=20001 k=4: worst error / bound 0.999
  update float64 n=20001 k=16: worst error / bound 0.242
  update float32 n=20001 k=16: worst error / bound 1.000
  update float64 n=70001 k=2: worst error / bound 0.917
  update float32 n=70001 k=2: worst error / bound 0.999
  residual float64 rand257 block_rows=0: W worst error / bound 0.730, sums 0.008
  residual float32 rand257 block_rows=0: W worst error / bound 0.982, sums 0.008
  residual float64 rand257 block_rows=1: W worst error / bound 0.801, sums 0.009
  residual float32 rand257 block_rows=1: W worst error / bound 0.997, sums 0.011
  residual float64 rand257 block_rows=2: W worst error / bound 0.512, sums 0.010
  residual float32 rand257 block_rows=2: W worst error / bound 0.994, sums 0.008
  residual float64 rand257 block_rows=3: W worst error / bound 0.509, sums 0.007
  residual float32 rand257 block_rows=3: W worst error / bound 0.981, sums 0.006
  residual float64 rand257 block_rows=4: W worst error / bound 0.353, sums 0.008
  residual float32 rand257 block_rows=4: W worst error / bound 0.989, sums 0.007
  residual float64 rand257 block_rows=6: W worst error / bound 0.260, sums 0.006
  residual float32 rand257 block_rows=6: W worst error / bound 0.978, sums 0.007
  residual float64 band20001 block_rows=0: W worst error / bound 0.749, sums 0.000
  residual float32 band20001 block_rows=0: W worst error / bound 0.999, sums 0.000
  residual float64 band20001 block_rows=1: W worst error / bound 0.761, sums 0.000
  residual float32 band20001 block_rows=1: W worst error / bound 0.999, sums 0.000
  residual float64 band20001 block_rows=3: W worst error / bound 0.614, sums 0.000
  residual float32 band20001 block_rows=3: W worst error / bound 0.999, sums 0.000
  residual float64 band140001 block_rows=0: W worst error / bound 0.748, sums 0.000
  residual float32 band140001 block_rows=0: W worst error / bound 0.995, sums 0.000
  residual float64 band140001 block_rows=1: W worst error / bound 0.749, sums 0.000
  residual float32 band140001 block_rows=1: W worst error / bound 0.999, sums 0.000
  lobpcg float64 lap2d16x15 block 2 n=240 k=4 block_jacobi: iterations 96, products 301, nconv 4, max r/(tol lmax) 0.823, max |theta - lambda|/lmax 1.35e-15, library residuals off by 1.82e-18 lmax
  lobpcg float32 lap2d16x15 block 2 n=240 k=4 block_jacobi: iterations 33, products 117, nconv 4, max r/(tol lmax) 0.887, max |theta - lambda|/lmax 7.90e-08, library residuals off by 8.27e-10 lmax
  lobpcg float64 lap2d16x15 block 4 n=240 k=4 block_jacobi: iterations 64, products 229, nconv 4, max r/(tol lmax) 0.739, max |theta - lambda|/lmax 1.35e-15, library residuals off by 2.01e-18 lmax
  lobpcg float32 lap2d16x15 block 4 n=240 k=4 block_jacobi: iterations 28, products 105, nconv 4, max r/(tol lmax) 0.888, max |theta - lambda|/lmax 4.46e-08, library residuals off by 1.33e-09 lmax
  lobpcg float64 lap2d16x15 block 6 n=240 k=4 block_jacobi: iterations 67, products 217, nconv 4, max r/(tol lmax) 0.999, max |theta - lambda|/lmax 1.34e-15, library residuals off by 2.23e-18 lmax
  lobpcg float32 lap2d16x15 block 6 n=240 k=4 block_jacobi: iterations 25, products 88, nconv 4, max r/(tol lmax) 0.976, max |theta - lambda|/lmax 1.01e-07, library residuals off by 1.99e-09 lmax
  lobpcg float64 rand257 block 2 n=257 k=4 block_jacobi: iterations 44, products 175, nconv 4, max r/(tol lmax) 0.810, max |theta - lambda|/lmax 1.35e-16, library residuals off by 2.60e-24 lmax
  lobpcg float32 rand257 block 2 n=257 k=4 block_jacobi: iterations 16, products 64, nconv 4, max r/(tol lmax) 0.849, max |theta - lambda|/lmax 6.90e-08, library residuals off by 1.30e-12 lmax
  lobpcg float64 rand257 block 4 n=257 k=4 block_jacobi: iterations 43, products 172, nconv 4, max r/(tol lmax) 0.986, max |theta - lambda|/lmax 1.18e-16, library residuals off by 8.81e-25 lmax
  lobpcg float32 rand257 block 4 n=257 k=4 block_jacobi: iterations 16, products 64, nconv 4, max r/(tol lmax) 0.819, max |theta - lambda|/lmax 6.28e-08, library residuals off by 1.84e-12 lmax
  lobpcg float64 rand257 block 6 n=257 k=4 block_jacobi: iterations 44, products 174, nconv 4, max r/(tol lmax) 0.674, max |theta - lambda|/lmax 1.27e-16, library residuals off by 1.46e-24 lmax
  lobpcg float32 rand257 block 6 n=257 k=4 block_jacobi: iterations 16, products 64, nconv 4, max r/(tol lmax) 0.793, max |theta - lambda|/lmax 6.53e-08, library residuals off by 1.27e-12 lmax
"""
import ctypes as C

import numpy as np
import pytest

from test_gpu_cg_steps import DTYPES, UNIT, _matrix
from test_gpu_kernel_variants import PLAN_KNOBS
from test_gpu_lobpcg_steps import LD, _block, _gram_case, gram_gpu

pytestmark = pytest.mark.gpu

U = 2.0 ** -53
MASKS = {"all": lambda k: (1 << k) - 1, "one": lambda k: 1 << (k // 2), "alternating": lambda k: sum(1 << i for i in range(0, k, 2)),
         "allbutfirst": lambda k: ((1 << k) - 1) & ~1}
WIDTHS = [2, 3, 5, 7, 23, 24, 32, 33, 40, 41, 47, 48]
DP = C.POINTER(C.c_double)


@pytest.fixture(autouse=True)
def _torch_first(monkeypatch):
    """torch brings a HIP runtime of its own: it has to initialise before libcfs_hip.so's"""
    import torch
    torch.cuda.init()
    torch.cuda.set_device(0)
    for k in PLAN_KNOBS:
        monkeypatch.delenv(k, raising=False)
    yield


def solver_list(k, mask, with_p):
    act = [i for i in range(k) if (mask >> i) & 1]
    return list(range(k)) + [k + i for i in act] + ([2 * k + i for i in act] if with_p else [])


def solver_lists(ks=(1, 2, 8, 16)):
    """the lists of the iteration, without repeats: {name: list}"""
    out = {}
    for k in ks:
        for name, f in MASKS.items():
            for with_p in (0, 1):
                lst = solver_list(k, f(k), with_p)
                if lst not in out.values():
                    out[f"k{k}-{name}-{'wp' if with_p else 'w'}"] = lst
    return out


def width_lists():
    """m of WIDTHS with k = ceil(m / 3): X whole, then m - k of the 2 k columns of W and P, ascending"""
    out = {}
    for m in WIDTHS:
        k = -(-m // 3)
        rest = np.sort(np.random.default_rng(m).permutation(2 * k)[:m - k]) + k
        out[f"m{m}"] = list(range(k)) + [int(c) for c in rest]
    return out


def all_lists():
    out = dict(solver_lists(), **width_lists())
    out["permuted"] = [int(c) for c in np.random.default_rng(7).permutation(48)[:21]]
    assert sorted({len(v) for v in solver_lists().values()}) == [1, 2, 3, 4, 6, 9, 10, 12, 15, 16, 17, 18, 22, 24, 31, 32, 46, 48]
    assert out["permuted"] != sorted(out["permuted"]) and all(0 <= c < 48 for v in out.values() for c in v)
    return out


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64 if a.dtype.itemsize == 8 else np.uint32)


def _lds(n, dtype):
    per = 16 // np.dtype(dtype).itemsize
    ld0 = -(-n // per) * per
    return ld0, ld0 + per


def _nans(count, dtype, salt=0):
    """`count` quiet NaNs of `dtype` with distinct payloads"""
    i = np.arange(1, count + 1, dtype=np.uint64) + np.uint64(salt)
    if dtype == np.float64:
        return (np.uint64(0x7ff8000000000000) | i).view(np.float64)
    assert count + salt < (1 << 22)
    return (np.uint32(0x7fc00000) | i.astype(np.uint32)).view(np.float32)


def _stream():
    import torch
    return torch.cuda.current_stream().cuda_stream


# ---- Gram ---------------------------------------------------------------------------------------------------------
def gram_cols(sbuf, tbuf, ld, n, idx, full_h, itemsize):
    import cfs_spmv_amd as cfs
    from cfs_spmv_amd import _lib
    m = len(idx)
    g, hh = np.full((m, m), np.nan), np.full((m, m), np.nan)
    _lib.check(cfs.load().cfs_hip_debug_gram_cols(sbuf.data_ptr(), tbuf.data_ptr(), ld, n, m, (C.c_int * m)(*idx), full_h, itemsize,
                                                  g.ctypes.data_as(DP), hh.ctypes.data_as(DP), _stream()))
    return g, hh


def _holed(clean, view_of, idx, ncols):
    """a copy of the device block `clean` whose unlisted columns are NaN"""
    buf = clean.clone()
    unlisted = [c for c in range(ncols) if c not in idx]
    if unlisted:
        view_of(buf)[:, unlisted] = float("nan")
    return buf


def _gram_lists(n):
    if n > 100000:  # a block of 6 columns, k = 2: one pair active, and every column
        return 6, {"k2-second-wp": [0, 1, 3, 5], "k2-all-wp": [0, 1, 2, 3, 4, 5]}
    return 48, all_lists()


GRAM_N = [1, 2, 63, 65, 257, 1023, 20001, 600001]


@DTYPES
@pytest.mark.parametrize("n", GRAM_N)
def test_gram_with_a_list_has_the_bits_of_the_contiguous_call(n, dtype):
    import torch
    S, T = _gram_case(n, dtype)[:2]
    ncols, lists = _gram_lists(n)
    errors = []
    for ld in _lds(n, dtype):
        sclean, _ = _block(S[:, :ncols], ld)
        tclean, _ = _block(T[:, :ncols], ld)
        view_of = lambda b: torch.as_strided(b, (n, ncols), (1, ld))
        for name, idx in lists.items():
            g, hh = gram_cols(_holed(sclean, view_of, idx, ncols), _holed(tclean, view_of, idx, ncols), ld, n, idx, 1, S.itemsize)
            g0, hh0 = gram_gpu(S[:, idx], T[:, idx], len(idx), ld)
            if np.isnan(g).any() or np.isnan(hh).any():
                errors.append(f"{name} ld={ld}: NaN, an unlisted column was read")
            elif not (np.array_equal(_bits(g), _bits(g0)) and np.array_equal(_bits(hh), _bits(hh0))):
                errors.append(f"{name} ld={ld}: the bits differ from the contiguous call's in {int(np.sum(_bits(g) != _bits(g0)))} entries "
                              f"of G and {int(np.sum(_bits(hh) != _bits(hh0)))} of H")
    assert not errors, f"n={n} {np.dtype(dtype).name}: " + "; ".join(errors[:8])


@DTYPES
@pytest.mark.parametrize("n", GRAM_N)
def test_gram_triangles_against_long_double(n, dtype):
    import torch
    S, T, G_ref, H_ref, G_abs, H_abs = _gram_case(n, dtype)
    ncols, lists = _gram_lists(n)
    errors, worst = [], 0.0
    for ld in _lds(n, dtype):
        sclean, _ = _block(S[:, :ncols], ld)
        tclean, _ = _block(T[:, :ncols], ld)
        view_of = lambda b: torch.as_strided(b, (n, ncols), (1, ld))
        for name, idx in lists.items():
            m = len(idx)
            sb, tb = _holed(sclean, view_of, idx, ncols), _holed(tclean, view_of, idx, ncols)
            g, hh = gram_cols(sb, tb, ld, n, idx, 0, S.itemsize)
            g2, hh2 = gram_cols(sb, tb, ld, n, idx, 0, S.itemsize)
            if not (np.array_equal(_bits(g), _bits(g2)) and np.array_equal(_bits(hh), _bits(hh2))):
                errors.append(f"{name} ld={ld}: two calls differ")
            up = np.triu(np.ones((m, m), bool))
            for what, got, ref, ab in (("G", g, G_ref, G_abs), ("H", hh, H_ref, H_abs)):
                if not np.array_equal(_bits(got), _bits(got.T.copy())):
                    errors.append(f"{name} ld={ld}: the lower triangle of {what} does not mirror the upper bit for bit")
                ix = np.ix_(idx, idx)
                bound = (n + 1) * 2.0 ** -53 * ab[ix]
                err = np.abs(got.astype(LD) - ref[ix])
                ok = (err <= bound) | ~up
                with np.errstate(invalid="ignore", divide="ignore"):
                    ratio = np.where(up & (bound > 0), err / bound, 0)
                worst = max(worst, float(np.max(ratio))) if np.all(np.isfinite(ratio.astype(np.float64))) else np.inf
                if not np.all(ok):
                    i, j = np.argwhere(~ok)[0]
                    errors.append(f"{name} ld={ld}: {what}[{i},{j}] = {got[i, j]!r}, long double {float(ref[ix][i, j])!r}, off by "
                                  f"{float(err[i, j]):.3e}, bound {float(bound[i, j]):.3e}")
    print(f"gram-triangles {np.dtype(dtype).name} n={n}: worst error / bound {worst:.3f}")
    assert not errors, f"n={n} {np.dtype(dtype).name}: " + "; ".join(errors[:8])


@DTYPES
@pytest.mark.parametrize("n,name", [(1, "k1-allbutfirst-w"), (65, "k2-one-wp"), (65, "m7"), (20001, "k16-alternating-wp"),
                                    (20001, "m41"), (20001, "permuted"), (1 << 18, "k2-one-wp")])
def test_gram_triangles_of_integers_with_a_holed_list_are_exact(n, name, dtype):
    import torch
    idx = all_lists()[name]
    ncols = 48 if n < 100000 else 6
    rng = np.random.default_rng(n + len(idx))
    S, T = rng.integers(-8, 9, (n, ncols)).astype(dtype), rng.integers(-8, 9, (n, ncols)).astype(dtype)
    ld = _lds(n, dtype)[0]
    view_of = lambda b: torch.as_strided(b, (n, ncols), (1, ld))
    g, hh = gram_cols(_holed(_block(S, ld)[0], view_of, idx, ncols), _holed(_block(T, ld)[0], view_of, idx, ncols), ld, n, idx, 0, S.itemsize)
    Si, Ti = S[:, idx].astype(np.int64), T[:, idx].astype(np.int64)
    H = Si.T @ Ti
    H = np.triu(H) + np.triu(H, 1).T  # (the lower triangle mirrors the upper: H is S^T T, not symmetric in itself)
    assert np.array_equal(g, (Si.T @ Si).astype(np.float64)) and np.array_equal(hh, H.astype(np.float64))


# ---- update -------------------------------------------------------------------------------------------------------
def _update_forms(n, k):
    """(name, list, with_p, second block): the forms of a case.  Every case has with_p = 0 and 1, a holed list and a call
    without the second block; the wide cases leave out what the narrow ones cover"""
    alt = MASKS["alternating"](k)
    forms = [("x", list(range(k)), 0, True), ("holed", solver_list(k, alt, 1), 1, True), ("w-only", solver_list(k, MASKS["all"](k), 0), 1, False)]
    if n * k <= 20001 * 4:
        forms += [("xw-keeps-p", solver_list(k, MASKS["allbutfirst"](k), 0) if k > 1 else [0, 1], 0, True),
                  ("identity", list(range(3 * k)), 1, True), ("one", solver_list(k, MASKS["one"](k), 1), 1, True),
                  ("allbutfirst", solver_list(k, MASKS["allbutfirst"](k), 1), 1, True),
                  ("permuted", [int(c) for c in np.random.default_rng(k).permutation(3 * k)[:2 * k + 1]], 1, True)]
    return forms


def _update_expect(A, idx, c, dtype):
    """(the kernel's order in numpy fp64 rounded once to V, the long-double value, A = sum |a_j| |c_jo|): (n, nout) each"""
    a64 = A[:, idx].astype(np.float64)
    acc = np.zeros((A.shape[0], c.shape[1]))
    for j in range(len(idx)):
        prod = a64[:, j, None] * c[j][None, :]  # (a multiply of its own ...
        acc = acc + prod                          # ... and an add of its own)
    al, cl = A[:, idx].astype(LD), c.astype(LD)
    return acc.astype(dtype), al @ cl, np.abs(al) @ np.abs(cl)


UPDATE_CASES = [(n, k) for n in (1, 31, 33, 63, 65, 257, 20001) for k in (1, 4, 16)] + [(70001, 2)]


@DTYPES
@pytest.mark.parametrize("n,k", UPDATE_CASES)
def test_update_with_a_dense_c_lists_and_both_blocks(n, k, dtype):
    import torch
    import cfs_spmv_amd as cfs
    from cfs_spmv_amd import _lib
    ld = _lds(n, dtype)[1]  # (one 16-byte word of rows [n, ld) behind every column)
    uv = 0.0 if dtype == np.float64 else UNIT[dtype]
    rng = np.random.default_rng(31 * n + k)
    errors, worst = [], 0.0
    for name, idx, with_p, second in _update_forms(n, k):
        m, nout = len(idx), (2 * k if with_p else k)
        c = rng.uniform(-1, 1, (m, nout))
        gamma = m * U / (1 - m * U)
        hosts, bufs = [], []
        for b in range(2 if second else 1):
            # the whole buffer NaNs with distinct payloads, then the listed columns' rows [0, n) the data
            host = _nans(3 * k * ld, dtype, salt=b * 3 * k * ld).reshape(3 * k, ld).copy()
            host[idx, :n] = rng.uniform(-1, 1, (m, n)).astype(dtype)
            hosts.append(host)
            bufs.append(torch.from_numpy(host.reshape(-1)).cuda())
        _lib.check(cfs.load().cfs_hip_debug_lobpcg_update_cols(bufs[0].data_ptr(), bufs[1].data_ptr() if second else None, ld, n, k, m,
                                                               (C.c_int * m)(*idx), with_p, c.ctypes.data_as(DP), np.dtype(dtype).itemsize,
                                                               _stream()))
        for b, (host, buf) in enumerate(zip(hosts, bufs)):
            out = buf.cpu().numpy().reshape(3 * k, ld)
            written = list(range(k)) + (list(range(2 * k, 3 * k)) if with_p else [])
            expect, ref, A = _update_expect(host[:, :n].T, idx, c, dtype)
            want = host.copy()
            want[written, :n] = expect.T
            tag = f"{name} block {b}"
            for what, cols in (("W", range(k, 2 * k)), ("P", [] if with_p else range(2 * k, 3 * k))):
                if not np.array_equal(_bits(out[list(cols)]), _bits(host[list(cols)])):
                    errors.append(f"{tag}: {what} was written")
            if not np.array_equal(_bits(out[:, n:]), _bits(host[:, n:])):
                errors.append(f"{tag}: the rows [n, ld) were written")
            got = out[written, :n].T
            if not np.array_equal(_bits(got), _bits(expect)):
                o, r = np.argwhere(_bits(got.T) != _bits(expect.T))[0]
                errors.append(f"{tag}: {int(np.sum(_bits(got) != _bits(expect)))} values differ from the documented order, first at output "
                              f"{o} row {r}: {got[r, o]!r} against {expect[r, o]!r}")
            bound = gamma * A + uv * (np.abs(ref) + gamma * A) + (m + 1) * 2.0 ** -64 * A
            err = np.abs(got.astype(LD) - ref)
            if not np.all(err <= bound):
                r, o = np.argwhere(~(err <= bound))[0]
                errors.append(f"{tag}: output {o} row {r} = {got[r, o]!r}, long double {float(ref[r, o])!r}, off by {float(err[r, o]):.3e}, "
                              f"bound {float(bound[r, o]):.3e}")
            else:
                worst = max(worst, float(np.max(err / bound)))
    print(f"update {np.dtype(dtype).name} n={n} k={k}: worst error / bound {worst:.3f}")
    assert not errors, f"n={n} k={k} {np.dtype(dtype).name}: " + "; ".join(errors[:8])


# ---- residual -----------------------------------------------------------------------------------------------------
def _handle(name, dtype):
    import cfs_spmv_amd as cfs
    n, rp, ci, va = _matrix(name)
    return cfs.SymMatrix(n, rp, ci, np.asarray(va).astype(dtype))


def _minv(A, block_rows, dtype):
    """M^-1 as the library stores it, as _iteration_case of test_gpu_lobpcg_steps.py takes it (pinned by the PCG tests)"""
    if block_rows == 0:
        return None
    if block_rows == 1:
        return (1.0 / A.diagonal().cpu().numpy().astype(np.float64)).astype(dtype)
    return A.block_inverse(block_rows).cpu().numpy()


def residual_gpu(A, block_rows, X, AX, theta, active, ld, wfill, refused=False):
    """X, AX: (k, n) host arrays; wfill: the (k, ld) host array W holds before.  Returns (W as (k, ld), sums); with
    `refused`, (W, sums, the error the call has to raise)"""
    import torch
    from cfs_spmv_amd import _lib
    import cfs_spmv_amd as cfs
    k, n = X.shape

    def dev(a):
        full = np.zeros((k, ld), a.dtype)
        full[:, :n] = a
        return torch.from_numpy(full.reshape(-1)).cuda()
    xb, axb, wb = dev(X), dev(AX), torch.from_numpy(wfill.reshape(-1).copy()).cuda()
    sums = np.full(2 * k, np.nan)
    th = np.ascontiguousarray(theta, np.float64)
    rc = cfs.load().cfs_hip_sym_debug_lobpcg_residual(A._h, block_rows, xb.data_ptr(), axb.data_ptr(), wb.data_ptr(), ld, k,
                                                      th.ctypes.data_as(DP), active, sums.ctypes.data_as(DP), _stream())
    if refused:
        with pytest.raises(_lib.CfsHipError) as e:
            _lib.check(rc)
        torch.cuda.synchronize()
        return wb.cpu().numpy().reshape(k, ld), sums, e.value
    _lib.check(rc)
    return wb.cpu().numpy().reshape(k, ld), sums


def _residual_reference(X, AX, theta, minv, block_rows):
    """(exact W, q = |M^-1| rho) in long double, (k, n) each"""
    k, n = X.shape
    Xl, AXl, tl = X.astype(LD), AX.astype(LD), theta.astype(LD)[:, None]
    R, rho = AXl - tl * Xl, np.abs(AXl) + np.abs(tl) * np.abs(Xl)
    if block_rows == 0:
        return R, rho
    if block_rows == 1:
        ml = minv.astype(LD)[None, :]
        return R * ml, rho * np.abs(ml)
    nb, bs, _ = minv.shape
    pad = lambda a: np.concatenate([a, np.zeros((k, nb * bs - n), LD)], axis=1).reshape(k, nb, bs)
    ml = minv.astype(LD)
    ap = lambda mm, a: np.einsum("bij,kbj->kbi", mm, pad(a)).reshape(k, nb * bs)[:, :n]
    return ap(ml, R), ap(np.abs(ml), rho)


def _residual_masks(k):
    return sorted({0, (1 << k) - 1, MASKS["alternating"](k), ((1 << k) - 1) & ~0xff})


def _check_residual(name, block_rows, dtype, ks):
    A = _handle(name, dtype)
    n = A.nrows()
    minv = _minv(A, block_rows, dtype)
    ld = _lds(n, dtype)[1]
    uv = 0.0 if dtype == np.float64 else UNIT[dtype]
    B = block_rows
    gamma = B * U / (1 - B * U)
    rng = np.random.default_rng(1000 * n + block_rows)
    errors, worst_w, worst_s = [], 0.0, 0.0
    for k in ks:
        X, AX = rng.uniform(-1, 1, (k, n)).astype(dtype), rng.uniform(-1, 1, (k, n)).astype(dtype)
        theta = rng.uniform(-1, 1, k)
        exact, q = _residual_reference(X, AX, theta, minv, block_rows)
        E = ((2 * U + U * U) + gamma * (1 + 2 * U + U * U)) * q
        bound = E + uv * (np.abs(exact) + E) + (B + 2) * 2.0 ** -64 * q
        d = AX.astype(np.float64) - theta[:, None] * X.astype(np.float64)  # (fp64: a multiply, then a subtraction)
        terms = np.stack([d.astype(LD) ** 2, X.astype(LD) ** 2], axis=1).reshape(2 * k, n)
        sref = np.sum(terms, axis=1)
        sbound = (n + 1) * 2.0 ** -53 * sref
        wfill = _nans(k * ld, dtype).reshape(k, ld)
        for active in _residual_masks(k):
            tag = f"k={k} active={active:#x}"
            W, sums = residual_gpu(A, block_rows, X, AX, theta, active, ld, wfill)
            W2, sums2 = residual_gpu(A, block_rows, X, AX, theta, active, ld, wfill)
            if not (np.array_equal(_bits(W), _bits(W2)) and np.array_equal(_bits(sums), _bits(sums2))):
                errors.append(f"{tag}: two calls differ")
            on = [i for i in range(k) if (active >> i) & 1]
            off = [i for i in range(k) if not (active >> i) & 1]
            if not np.array_equal(_bits(W[off]), _bits(wfill[off])):
                errors.append(f"{tag}: an inactive W_i was written")
            if not np.array_equal(_bits(W[:, n:]), _bits(wfill[:, n:])):
                errors.append(f"{tag}: the rows [n, ld) were written")
            err = np.abs(W[on, :n].astype(LD) - exact[on])
            if not np.all(err <= bound[on]):
                i, r = np.argwhere(~(err <= bound[on]))[0]
                errors.append(f"{tag}: W_{on[i]}[{r}] = {W[on[i], r]!r}, long double {float(exact[on[i], r])!r}, off by {float(err[i, r]):.3e}, "
                              f"bound {float(bound[on[i], r]):.3e}")
            elif on:
                worst_w = max(worst_w, float(np.max(err / bound[on])))
            serr = np.abs(sums.astype(LD) - sref)
            if not np.all(serr <= sbound):
                i = int(np.argwhere(~(serr <= sbound))[0][0])
                errors.append(f"{tag}: sums[{i}] = {sums[i]!r}, long double {float(sref[i])!r}, off by {float(serr[i]):.3e}, bound "
                              f"{float(sbound[i]):.3e}")
            else:
                worst_s = max(worst_s, float(np.max(serr / sbound)))
    A.close()
    print(f"residual {np.dtype(dtype).name} {name} block_rows={block_rows}: W worst error / bound {worst_w:.3f}, sums {worst_s:.3f}")
    assert not errors, f"{name} block_rows={block_rows} {np.dtype(dtype).name}: " + "; ".join(errors[:8])


@DTYPES
@pytest.mark.parametrize("block_rows", [0, 1, 2, 3, 4, 6])
def test_residual_kernel_with_a_trailing_partial_block(block_rows, dtype):
    """rand257: 257 mod 2, 3, 4, 6 = 1, 2, 1, 5"""
    _check_residual("rand257", block_rows, dtype, (1, 8, 9, 16))


@DTYPES
@pytest.mark.parametrize("block_rows", [0, 1, 3])
def test_residual_kernel_on_more_than_one_workgroup(block_rows, dtype):
    _check_residual("band20001", block_rows, dtype, (1, 8, 9, 16))


@DTYPES
@pytest.mark.parametrize("block_rows", [0, 1])
def test_residual_kernel_beyond_one_grid_stride_sweep(block_rows, dtype):
    """band140001: more than 512 x 256 = 131072 node blocks"""
    _check_residual("band140001", block_rows, dtype, (2,))


@DTYPES
@pytest.mark.parametrize("name,k", [("rand257", 9), ("band20001", 16)])
def test_residual_of_integers_is_exact(name, k, dtype):
    A = _handle(name, dtype)
    n = A.nrows()
    ld = _lds(n, dtype)[1]
    rng = np.random.default_rng(n + k)
    X, AX, theta = rng.integers(-8, 9, (k, n)), rng.integers(-8, 9, (k, n)), rng.integers(-8, 9, k)
    wfill = _nans(k * ld, dtype).reshape(k, ld)
    active = MASKS["alternating"](k) | (1 << (k - 1))
    W, sums = residual_gpu(A, 0, X.astype(dtype), AX.astype(dtype), theta.astype(np.float64), active, ld, wfill)
    A.close()
    R = AX - theta[:, None] * X
    want = wfill.copy()
    on = [i for i in range(k) if (active >> i) & 1]
    want[on, :n] = R[on].astype(dtype)
    assert np.array_equal(_bits(W), _bits(want))
    assert np.array_equal(sums, np.stack([np.sum(R * R, axis=1), np.sum(X * X, axis=1)], axis=1).reshape(-1).astype(np.float64))


@DTYPES
def test_residual_refuses_a_matrix_the_preconditioner_cannot_take(dtype):
    """the refusals of cfs_hip_sym_lobpcg, with its words, and nothing written"""
    import scipy.sparse as sp
    import cfs_spmv_amd as cfs
    from cfs_spmv_amd import _lib
    n, rp, ci, va = _matrix("rand257")
    M = sp.lil_matrix(sp.csr_matrix((np.asarray(va, np.float64), ci, rp), shape=(n, n)))
    k, ld = 4, _lds(n, dtype)[1]
    X = np.random.default_rng(1).uniform(-1, 1, (k, n)).astype(dtype)
    wfill = _nans(k * ld, dtype).reshape(k, ld)
    for bad, block_rows, word in ((0.0, 1, "lobpcg: Jacobi needs a positive diagonal, 1 of 257 entries are zero, negative or not finite"),
                                  (None, 3, "lobpcg: block Jacobi needs positive definite diagonal blocks, 1 of 86 blocks of 3 rows have a "
                                            "pivot that is zero, negative or not finite")):
        Mb = M.copy()
        if bad is None:
            Mb[30, 31] = Mb[31, 30] = 4.0 * max(Mb[30, 30], Mb[31, 31])  # a 2 x 2 minor with a negative determinant
        else:
            Mb[100, 100] = bad
        Mb = Mb.tocsr()
        Mb.sort_indices()
        Z = cfs.SymMatrix(n, Mb.indptr.astype(np.int32), Mb.indices.astype(np.int32), Mb.data.astype(dtype))
        W, sums, e = residual_gpu(Z, block_rows, X, X, np.ones(k), 0xf, ld, wfill, refused=True)
        assert e.code == _lib.ERR_ARG and word in str(e)
        assert np.array_equal(_bits(W), _bits(wfill)) and np.all(np.isnan(sums)), "nothing written"
        with pytest.raises(_lib.CfsHipError) as e2:  # the solver says the same
            Z.lobpcg(k=k, scale=1.0, maxiter=2, **(dict(precond="jacobi") if block_rows == 1 else dict(precond="block_jacobi", block=3)))
        assert str(e2.value) == str(e)
        W, sums = residual_gpu(Z, 0, X, X, np.ones(k), 0, ld, wfill)  # (block_rows = 0: the matrix is as good as any)
        assert np.array_equal(_bits(W), _bits(wfill)) and np.all(sums[0::2] == 0)
        Z.close()


@DTYPES
def test_the_refusals_that_need_a_device(dtype):
    """after the checks test_lobpcg_abi.py pins: a bad ld against the handle's n, overlapping columns, a shard, block Jacobi
    on a multi-device handle, host memory -- CFS_HIP_ERR_ARG / _UNSUPPORTED, and nothing written"""
    import torch
    import cfs_spmv_amd as cfs
    from cfs_spmv_amd import _lib
    lib = cfs.load()
    n, rp, ci, va = _matrix("rand257")
    va = np.asarray(va).astype(dtype)
    item = np.dtype(dtype).itemsize
    ld, k = _lds(n, dtype)[1], 2
    host = np.zeros(3 * k * ld + 8, dtype)
    host = host[(-host.ctypes.data % 16) // item:][:3 * k * ld]
    dev = torch.zeros(3 * k * ld, dtype=torch.float64 if dtype == np.float64 else torch.float32, device="cuda")
    hp, dp_ = host.ctypes.data, dev.data_ptr()
    out, idx = np.full(2 * 9, 7.0), (C.c_int * 3)(0, 1, 3)
    o = out.ctypes.data_as(DP)

    def refused(rc, code, word):
        assert rc == code and word in lib.cfs_hip_last_error(), (rc, lib.cfs_hip_last_error())
    dev2 = torch.zeros_like(dev)
    for s, t in ((hp, dev2.data_ptr()), (dp_, hp)):
        refused(lib.cfs_hip_debug_gram_cols(s, t, ld, n, 3, idx, 0, item, o, o, None), _lib.ERR_ARG, b"device pointers")
        refused(lib.cfs_hip_debug_lobpcg_update_cols(s, t, ld, n, k, 3, idx, 1, o, item, None), _lib.ERR_ARG, b"device pointers")
    refused(lib.cfs_hip_debug_lobpcg_update_cols(hp, None, ld, n, k, 3, idx, 1, o, item, None), _lib.ERR_ARG, b"device pointers")
    A = cfs.SymMatrix(n, rp, ci, va)
    th = (C.c_double * 2)(0.5, 0.5)
    col = lambda c: dp_ + c * ld * item
    res = lambda h, bs, x, ax, w, ld_: lib.cfs_hip_sym_debug_lobpcg_residual(h, bs, x, ax, w, ld_, k, th, 3, o, None)
    refused(res(A._h, 1, col(0), col(2), col(4), n - 1), _lib.ERR_ARG, b"bad ld")
    refused(res(A._h, 1, col(0), col(2), col(4), ld - 1), _lib.ERR_ARG, b"bad ld")  # (not a multiple of 16 bytes)
    refused(res(A._h, 1, col(0), col(2), col(1), ld), _lib.ERR_ARG, b"overlaps")  # W_0 is X_1
    refused(res(A._h, 1, col(0), col(2), col(3), ld), _lib.ERR_ARG, b"overlaps")  # W_0 is AX_1
    for x, ax, w in ((hp, col(2), col(4)), (col(0), hp, col(4)), (col(0), col(2), hp)):
        refused(res(A._h, 1, x, ax, w, ld), _lib.ERR_ARG, b"must be a device pointer")
    A.close()
    S = cfs.SymMatrix(n, rp, ci, va, row_splits=np.array([0, n // 2, n], np.int32), rank=1)
    refused(res(S._h, 1, col(0), col(2), col(4), ld), _lib.ERR_UNSUPPORTED, b"shard")
    S.close()
    M = cfs.SymMatrix(n, rp, ci, va, ngpus=2)
    refused(res(M._h, 3, col(0), col(2), col(4), ld), _lib.ERR_UNSUPPORTED, b"one device")
    assert res(M._h, 1, col(0), col(2), col(4), ld) == 0  # (Jacobi: the diagonal of a multi-device handle is whole)
    M.close()
    torch.cuda.synchronize()
    assert not host.any() and not bool(dev2.any()) and np.all(out[4:] == 7.0)


# ---- whole solves at the block sizes 2, 4 and 6 -------------------------------------------------------------------
class _WithBlock:
    """a handle whose lobpcg() runs block Jacobi with blocks of `block` rows (test_gpu_lobpcg._check names no block)"""

    def __init__(self, A, block):
        self.A, self.block = A, block

    def lobpcg(self, **kw):
        return self.A.lobpcg(**dict(kw, block=self.block))


@DTYPES
@pytest.mark.parametrize("block", [2, 4, 6])
@pytest.mark.parametrize("name", ["lap2d16x15", "rand257"])
def test_whole_solves_at_the_other_block_sizes(name, block, dtype):
    import cfs_spmv_amd as cfs
    from test_gpu_lobpcg import TOL, _case, _check
    case = _case(name, dtype)
    A = cfs.SymMatrix(*case[:4])
    _check(f"{name} block {block}", case, dtype, _WithBlock(A, block), TOL[dtype], precond="block_jacobi")
    A.close()
