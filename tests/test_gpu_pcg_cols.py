"""cfs_hip_sym_pcg_cols and cfs_hip_sym_pcg_amg_cols, PCG on a block of right-hand sides, on the GPU.

C1 (the main check).  On a CFS_HIP_FLAG_DETERMINISTIC handle, in both value types, every column of U and its
iterations[c] and relres[c] must equal the one-column entry point on (u_c, b_c) alone BYTE FOR BYTE: cfs_hip_sym_cg (none),
cfs_hip_sym_pcg (Jacobi), cfs_hip_sym_pcg_block (2, 3, 4, 6) and cfs_hip_sym_pcg_amg (scalar hierarchies at degrees 1 and
3, node-block hierarchies, a device-built one), for the column counts 1, 2, 8, 9, 16, which straddle the chunk widths of
the kernels (2 and 4).  The blocks have ld > n, SENTINEL in the padding rows n .. ld - 1 of every
column and guard words before and behind both blocks: B, the padding and the guards must be unchanged.  The columns are
chosen to stop at different iterations (COLUMNS below; some stop at MAXITER): two ordinary ones, a zero column, one whose first guess already
solves it, one that holds a NaN, and the rest started from first guesses at different distances from the solution.  The
test asserts that the counts do differ, that the zero, solved and NaN columns never iterate in their one-column solves
(so the block may not either), and the equality covers the columns beside them.  Both sides run the same four kernel
sources of csrc/cfs_solver.hpp, the one-column solves their OneColumn instantiation and the block its ColumnMask one: C1
and C2 are the judge that the two are compiled to the same arithmetic.

C2.  The same solve with check_every = 1, with the largest window, and with maxiter cutting some columns short gives
the bytes of the one-column solves: a column is frozen by the device inside a window of enqueued iterations.

C3.  On a default handle the iterates after maxiter in KS iterations of a 9-column Jacobi and block-Jacobi solve lie
within the allowance _check_iterates of test_gpu_pcg_steps.py / test_gpu_block_pcg_steps.py uses against the long-double
recurrence (4 d_k + 16 u); no new tolerance.

C4.  The refusals of cfs_hip.h, U untouched; a diagonal that is not positive refuses the whole call.

C5.  Amg.column_cycles() grows by exactly the sum of iterations[c] + 1 over the columns that were ever active.

Matrices (name: coarse_max of the hierarchy):  rand63: 512, fewer rows than a wave;  rand3: 1;  rand257: 40, n no multiple
of the vector width;  rand1026: 8, seven levels;  band300: 40, a scaled() band matrix;  rotated_node_laplacian(3, 12, 11)
and (6, 8, 7) for the block forms.
"""
import functools

import numpy as np
import pytest

from test_amg_block_abi import rotated_node_laplacian
from test_gpu_amg_steps import LEAD, SENTINEL, TRAIL, _case, _torch_first  # noqa: F401
from test_gpu_block_pcg_steps import _check_iterates as _check_block_iterates
from test_gpu_block_pcg_steps import _minv
from test_gpu_cg_steps import DET, DTYPES, KS
from test_gpu_cg_steps import _matrix as _unscaled
from test_gpu_pcg_steps import D_LIMIT, UNIT, _check_iterates, _deviation, pcg_reference  # noqa: F401

pytestmark = pytest.mark.gpu

MAXC = 16
NCOLS = (1, 2, 8, 9, 16)
TOL = {np.float64: 1e-10, np.float32: 1e-5}
TOL_PLAIN = {np.float64: 1e-5, np.float32: 3e-3}  # without a preconditioner, on the scaled matrices: TOL ** 0.5
MAXITER = 1000
# what column c of the block is: "zero" (b = 0, u = 0), "solved" (b = A u in the value type), "nan" (one NaN in b), or the
# exponent f of the first guess u = (1 - eps) x, x the solution and eps = TOL ** f: its residual is eps b, so the
# tolerance still to go differs from column to column (f = 0: the zero guess) and eps > TOL in both value types
COLUMNS = [0.0, 0.3, "zero", "solved", "nan", 0.1, 0.5, 0.0, 0.15, 0.4, 0.2, 0.0, 0.35, 0.6, 0.05, 0.3]
SPECIAL = {c: k for c, k in enumerate(COLUMNS) if isinstance(k, str)}
# (label, matrix, block_rows of the stored preconditioners)
STORED = [("rand63", (0, 1, 2, 3, 4, 6)), ("rand3", (0, 1, 2, 3, 4, 6)), ("rand257", (0, 1, 2, 3, 4, 6)), ("rand1026", (0, 1, 2, 3, 4, 6)),
          ("band300", (0, 1, 3)), ("node3", (1, 3)), ("node6", (2, 3, 6))]
# (label, matrix, coarse_max, degree, keywords of SymMatrix.amg)
HIERARCHIES = [("rand63-m1", "rand63", 512, 1, {}), ("rand3-m3", "rand3", 1, 3, {}), ("rand257-m1", "rand257", 40, 1, {}),
               ("rand257-m3", "rand257", 40, 3, {}), ("rand1026-m1", "rand1026", 8, 1, {}), ("rand1026-m3", "rand1026", 8, 3, {}),
               ("band300-m1", "band300", 40, 1, {}), ("node3-m1", "node3", 32, 1, dict(block=3)), ("node3-m3", "node3", 32, 3, dict(block=3)),
               ("node6-m1", "node6", 32, 1, dict(block=6)), ("rand1026-device-m1", "rand1026", 8, 1, dict(setup="device", matching="dominant"))]


@functools.lru_cache(maxsize=None)
def _matrix(name, dtype):
    """(n, rp, ci, va in the value type); computed once, shared, unchanged"""
    if name.startswith("node"):
        n, rp, ci, va = rotated_node_laplacian(3, 12, 11) if name == "node3" else rotated_node_laplacian(6, 8, 7)
        return n, rp, ci, np.asarray(va).astype(dtype)
    return _case(name, dtype)


@functools.lru_cache(maxsize=None)
def _problem(name, dtype):
    """(B, X0): (n, MAXC) right-hand sides and first guesses of COLUMNS in the value type; computed once, shared, unchanged"""
    import scipy.sparse as sp
    import scipy.sparse.linalg as spl
    n, rp, ci, va = _matrix(name, dtype)
    A = sp.csr_matrix((va.astype(np.float64), ci.copy(), rp.copy()), shape=(n, n))
    rng = np.random.default_rng(4000 + n)
    B, X0 = np.zeros((n, MAXC), dtype, order="F"), np.zeros((n, MAXC), dtype, order="F")
    for c, kind in enumerate(COLUMNS):
        b = rng.uniform(-1, 1, n).astype(dtype)
        if kind == "zero":
            continue
        if kind == "solved":
            X0[:, c] = b
            B[:, c] = (A @ X0[:, c].astype(np.float64)).astype(dtype)
            continue
        B[:, c] = b
        if kind == "nan":
            B[n // 2, c] = np.nan
            continue
        x = spl.spsolve(A.tocsc(), b.astype(np.float64))
        X0[:, c] = ((1.0 - TOL[dtype] ** kind) * x).astype(dtype) if kind > 0 else 0
    B.setflags(write=False)
    X0.setflags(write=False)
    return B, X0


def _ld(n, dtype):
    per = 16 // np.dtype(dtype).itemsize
    return -(-n // per) * per + per  # (rounded up to 16 bytes, and one vector more: ld > n)


def _tdt(dtype):
    import torch
    return torch.float64 if dtype == np.float64 else torch.float32


class Blocks:
    """U and B on the device: guard words, ncols columns of ld values, guard words; the padding rows SENTINEL"""

    def __init__(self, B, X0, ncols, ld=None):
        import torch
        n, dtype = B.shape[0], B.dtype.type
        self.n, self.ncols, self.ld = n, ncols, _ld(n, dtype) if ld is None else ld
        size = LEAD + (ncols - 1) * self.ld + max(self.ld, n) + TRAIL
        u, b = np.full(size, SENTINEL, dtype), np.full(size, SENTINEL, dtype)
        for c in range(ncols):
            u[LEAD + c * self.ld:LEAD + c * self.ld + n] = X0[:, c]
            b[LEAD + c * self.ld:LEAD + c * self.ld + n] = B[:, c]
        self.u0, self.b0 = u, b
        self.ubuf, self.bbuf = torch.from_numpy(u).cuda(), torch.from_numpy(b).cuda()
        assert self.ubuf.data_ptr() % 16 == 0 and self.bbuf.data_ptr() % 16 == 0

    def views(self):
        import torch
        shape, strides = (self.n, self.ncols), (1, self.ld)
        return torch.as_strided(self.ubuf[LEAD:], shape, strides), torch.as_strided(self.bbuf[LEAD:], shape, strides)

    def check(self, want):
        """the errors of a solve: want[:, c] the expected bytes of column c of U (None: U as it was)"""
        import torch
        torch.cuda.synchronize()
        u, b = self.ubuf.cpu().numpy(), self.bbuf.cpu().numpy()
        errors = []
        if not np.array_equal(b.view(np.uint8), self.b0.view(np.uint8)):
            errors.append("B or its guards changed")
        expect = self.u0.copy()
        if want is not None:
            for c in range(self.ncols):
                expect[LEAD + c * self.ld:LEAD + c * self.ld + self.n] = want[:, c]
        vb = u.dtype.itemsize
        if not np.array_equal(u.view(np.uint8), expect.view(np.uint8)):
            diff = np.flatnonzero((u.view(np.uint8).reshape(len(u), vb) != expect.view(np.uint8).reshape(len(u), vb)).any(axis=1))
            where = sorted({("guard" if i < LEAD or i >= LEAD + (self.ncols - 1) * self.ld + self.n else
                             f"column {(i - LEAD) // self.ld} {'row' if (i - LEAD) % self.ld < self.n else 'padding'}") for i in diff[:2000]})
            errors.append(f"U differs in {len(diff)} words ({', '.join(where[:6])})")
        return errors


def _same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def _one_column(A, B, X0, precond, block=3, **kw):
    """the one-column entry point on every column alone: (U (n, MAXC), iterations, relres)"""
    import torch
    import cfs_spmv_amd as cfs
    n, ncols = B.shape
    U, its, res = np.zeros(B.shape, B.dtype, order="F"), np.zeros(ncols, np.int32), np.zeros(ncols, np.float64)
    for c in range(ncols):
        u, b = torch.from_numpy(np.array(X0[:, c])).cuda(), torch.from_numpy(np.array(B[:, c])).cuda()
        if isinstance(precond, cfs.Amg):
            its[c], res[c] = A.pcg_amg(u, b, precond, **kw)
        else:
            its[c], res[c] = A.pcg(u, b, precond=precond, block=block, **kw)
        torch.cuda.synchronize()
        U[:, c] = u.cpu().numpy()
    return U, its, res


def _blocked(A, B, X0, ncols, precond, want, block=3, **kw):
    """the errors of one blocked solve of the first ncols columns against `want` = (U, iterations, relres) of _one_column"""
    blocks = Blocks(B, X0, ncols)
    U, Bv = blocks.views()
    its, res = A.pcg_cols(U, Bv, precond=precond, block=block, **kw)
    errors = blocks.check(want[0])
    assert its.dtype == np.int32 and res.dtype == np.float64 and its.shape == res.shape == (ncols,)
    if not np.array_equal(its, want[1][:ncols]):
        errors.append(f"iterations {its.tolist()}, one column at a time {want[1][:ncols].tolist()}")
    if not _same_bits(res, want[2][:ncols]):
        errors.append(f"relres {res.tolist()}, one column at a time {want[2][:ncols].tolist()}")
    return errors


def _check_the_columns_differ(label, want, same=False):
    """the properties of the one-column solves the block is compared with: C1 would show little without them.  same: a
    case whose columns all stop together (three rows, or a hierarchy that is one dense level: the cycle is a direct solve)"""
    U, its, res = want
    for c, kind in SPECIAL.items():
        assert its[c] == 0, f"{label}: the {kind} column iterates {its[c]} times in its one-column solve"
    assert np.isnan(res[4]) and res[2] == 0.0 and np.all(np.isfinite(np.delete(res, 4))), f"{label}: relres {res.tolist()}"
    ordinary = [int(its[c]) for c in range(MAXC) if c not in SPECIAL]
    # (a column may also stop at MAXITER: the plain iteration on the scaled matrices does)
    assert its[0] >= 1 and (same or len(set(ordinary)) >= 2), f"{label}: iterations {its.tolist()}"


def _precond_of(bs):
    return ("none", 3) if bs == 0 else ("jacobi", 3) if bs == 1 else ("block_jacobi", bs)


# ---- C1 ---------------------------------------------------------------------------------------------------------
@DTYPES
@pytest.mark.parametrize("name,sizes", STORED, ids=[s[0] for s in STORED])
def test_every_column_has_the_bits_of_its_one_column_solve(name, sizes, dtype):
    import cfs_spmv_amd as cfs
    n, rp, ci, va = _matrix(name, dtype)
    B, X0 = _problem(name, dtype)
    A = cfs.SymMatrix(n, rp, ci, va, options=cfs.make_options(flags=DET))
    assert A.kernel_variant()["det"] == 1
    errors = []
    for bs in sizes:
        precond, block = _precond_of(bs)
        kw = dict(tol=(TOL_PLAIN if bs == 0 else TOL)[dtype], maxiter=MAXITER)
        want = _one_column(A, B, X0, precond, block, **kw)
        print(f"pcg-cols {np.dtype(dtype).name} {name} block_rows={bs}: iterations {want[1].tolist()}")
        _check_the_columns_differ(f"{name} block_rows={bs}", want, same=n <= 3)
        for ncols in NCOLS:
            errors += [f"block_rows={bs} ncols={ncols}: {e}" for e in _blocked(A, B, X0, ncols, precond, want, block, **kw)]
    A.close()
    assert not errors, f"{name} {np.dtype(dtype).name}: " + "; ".join(errors[:8])


@DTYPES
@pytest.mark.parametrize("label,name,cm,degree,kw", HIERARCHIES, ids=[h[0] for h in HIERARCHIES])
def test_every_column_has_the_bits_of_its_one_column_multigrid_solve(label, name, cm, degree, kw, dtype):
    import cfs_spmv_amd as cfs
    n, rp, ci, va = _matrix(name, dtype)
    B, X0 = _problem(name, dtype)
    A = cfs.SymMatrix(n, rp, ci, va, options=cfs.make_options(flags=DET))
    assert A.kernel_variant()["det"] == 1
    G = A.amg(rp, ci, va, degree=degree, coarse_max=cm, **kw)
    skw = dict(tol=TOL[dtype], maxiter=MAXITER)
    want = _one_column(A, B, X0, G, **skw)
    print(f"pcg-cols {np.dtype(dtype).name} {label}: iterations {want[1].tolist()}")
    _check_the_columns_differ(label, want, same=name in ("rand3", "rand63"))
    errors = []
    for ncols in NCOLS:
        before = G.column_cycles()
        errors += [f"ncols={ncols}: {e}" for e in _blocked(A, B, X0, ncols, G, want, **skw)]
        # C5: one cycle before the first iteration and one per iteration, for the columns that were ever active
        grown, expect = G.column_cycles() - before, sum(int(want[1][c]) + 1 for c in range(ncols) if c not in SPECIAL)
        if grown != expect:
            errors.append(f"ncols={ncols}: column_cycles grew by {grown}, the columns' iterations + 1 add up to {expect}")
    G.close()
    A.close()
    assert not errors, f"{label} {np.dtype(dtype).name}: " + "; ".join(errors[:8])


# ---- C2 ---------------------------------------------------------------------------------------------------------
@DTYPES
@pytest.mark.parametrize("name,bs", [("rand1026", 0), ("rand1026", 1), ("rand257", 3), ("node6", 6), ("rand1026", "amg")],
                         ids=["rand1026-none", "rand1026-jacobi", "rand257-block3", "node6-block6", "rand1026-amg"])
def test_the_window_and_maxiter_do_not_change_the_bits(name, bs, dtype):
    import cfs_spmv_amd as cfs
    n, rp, ci, va = _matrix(name, dtype)
    B, X0 = _problem(name, dtype)
    A = cfs.SymMatrix(n, rp, ci, va, options=cfs.make_options(flags=DET))
    G = A.amg(rp, ci, va, degree=1, coarse_max=8) if bs == "amg" else None
    precond, block = (G, 3) if G is not None else _precond_of(bs)
    tol = (TOL_PLAIN if bs == 0 else TOL)[dtype]
    full = _one_column(A, B, X0, precond, block, tol=tol, maxiter=MAXITER)[1]
    ordinary = sorted(int(full[c]) for c in range(MAXC) if c not in SPECIAL)
    cut = ordinary[len(ordinary) // 2] - 1  # some columns converge before it, the others are cut short by it
    assert ordinary[0] < cut < ordinary[-1], full.tolist()
    errors = []
    for maxiter in (MAXITER, cut, 0):
        kw = dict(tol=tol, maxiter=maxiter)
        want = _one_column(A, B, X0, precond, block, **kw)
        assert np.all(want[1] <= maxiter) and (maxiter != cut or (np.any(want[1] == cut) and np.any((want[1] > 0) & (want[1] < cut))))
        for ncols in (2, 3, 9, 16):  # (the window is at most 11, 8, 3 and 2 iterations wide)
            for check_every in (1, 1000, 0):
                errors += [f"maxiter={maxiter} ncols={ncols} check_every={check_every}: {e}"
                           for e in _blocked(A, B, X0, ncols, precond, want, block, check_every=check_every, **kw)]
    if G is not None:
        G.close()
    A.close()
    assert not errors, f"{name} {bs} {np.dtype(dtype).name}: " + "; ".join(errors[:8])


# ---- C3 ---------------------------------------------------------------------------------------------------------
@DTYPES
@pytest.mark.parametrize("bs", (1, 3), ids=("jacobi", "block3"))
def test_iterates_of_nine_columns_against_the_long_double_recurrence(bs, dtype):
    import torch
    import cfs_spmv_amd as cfs
    name, ncols = "rand257", 9
    n, rp, ci, va = _matrix(name, dtype)
    R = np.asfortranarray(np.random.default_rng(5000 + n).uniform(-1, 1, (n, ncols)).astype(dtype))
    Z = np.zeros((n, ncols), dtype, order="F")
    A = cfs.SymMatrix(n, rp, ci, va)
    precond, block = _precond_of(bs)
    minv = _minv(A, bs, torch) if bs >= 2 else None
    got = {}
    for k in KS:  # one blocked solve per k, shared by the columns
        blocks = Blocks(R, Z, ncols)
        U, Bv = blocks.views()
        its, _ = A.pcg_cols(U, Bv, precond=precond, block=block, tol=0.0, maxiter=k)
        assert not [e for e in blocks.check(None) if e.startswith("B or")]
        got[k] = (U.cpu().numpy().copy(), its)
    for c in range(ncols):
        b = np.ascontiguousarray(R[:, c])
        run = lambda k: (np.ascontiguousarray(got[k][0][:, c]), int(got[k][1][c]))
        if bs >= 2:
            _check_block_iterates(name, n, rp, ci, va, b, dtype, bs, minv, run, label=f" column {c} of {ncols}")
        else:
            _check_iterates(name, n, rp, ci, va, b, dtype, run, label=f" column {c} of {ncols}")
    A.close()


# ---- C4 ---------------------------------------------------------------------------------------------------------
@DTYPES
def test_refusals_leave_u_untouched(dtype):
    import ctypes as C
    import cfs_spmv_amd as cfs
    from cfs_spmv_amd import _lib
    lib = cfs.load()
    name = "rand257"
    n, rp, ci, va = _matrix(name, dtype)
    B, X0 = _problem(name, dtype)
    A = cfs.SymMatrix(n, rp, ci, va)
    G = A.amg(rp, ci, va, coarse_max=40, refreshable=True)
    A2 = cfs.SymMatrix(n, rp, ci, va)
    ld, vb = _ld(n, dtype), np.dtype(dtype).itemsize
    blocks = Blocks(B, X0, 4)
    up, bp = blocks.ubuf.data_ptr() + LEAD * vb, blocks.bbuf.data_ptr() + LEAD * vb

    def refused(word, code=_lib.ERR_ARG, amg=None, h=None, u=up, b=bp, ld=ld, ncols=4, block_rows=1, tol=1e-8, maxiter=10):
        it, res = (C.c_int * 16)(*([7] * 16)), (C.c_double * 16)(*([7.0] * 16))
        h = A._h if h is None else h
        if amg is not None:
            rc = lib.cfs_hip_sym_pcg_amg_cols(h, amg, u, b, ld, ncols, tol, maxiter, 8, it, res, None)
        else:
            rc = lib.cfs_hip_sym_pcg_cols(h, u, b, ld, ncols, block_rows, tol, maxiter, 8, it, res, None)
        assert rc == code and word in lib.cfs_hip_last_error(), (word, rc, lib.cfs_hip_last_error())
        zeroed = ncols if 1 <= ncols <= 16 else 1
        assert list(it) == [0] * zeroed + [7] * (16 - zeroed) and list(res) == [0.0] * zeroed + [7.0] * (16 - zeroed), word
        assert not blocks.check(None), word
    for amg in (None, G._a):
        # in the documented order: what comes later is bad as well
        for ncols in (0, -1, 17):
            refused(b"ncols", amg=amg, ncols=ncols, u=up + vb, ld=n - 1, tol=-1.0, block_rows=5)
        refused(b"16-byte aligned", amg=amg, u=up + vb, ld=n - 1, tol=-1.0, block_rows=5)
        refused(b"16-byte aligned", amg=amg, b=bp + vb, ld=n - 1, tol=-1.0, block_rows=5)
        refused(b"bad ld", amg=amg, ld=n - 1, b=up, tol=-1.0, block_rows=5)
        refused(b"bad ld", amg=amg, ld=n, ncols=2, b=up, tol=-1.0)        # n = 257: n sizeof(V) is no multiple of 16
        refused(b"bad ld", amg=amg, ld=ld + 1, ncols=2, b=up, tol=-1.0)
        last = ((3 * ld + n) * vb - 1) // 16 * 16  # the last 16-byte aligned address inside the span of a block
        for off in (0, 16, last, -last):  # B inside the span of U, before and behind
            refused(b"overlap", amg=amg, b=up + off, tol=-1.0, block_rows=5)
        for kw in (dict(tol=-1e-3), dict(tol=float("nan")), dict(maxiter=-1)):
            refused(b"tolerance", amg=amg, **kw)
    for block_rows in (-1, 5, 7, 8):
        refused(b"block_rows", block_rows=block_rows)
    host = np.zeros(4 * ld + 8, dtype)
    host = host[(-host.ctypes.data % 16) // vb:]
    refused(b"device pointer", u=host.ctypes.data)
    refused(b"device pointer", amg=G._a, u=host.ctypes.data)
    assert not host.any()
    # the hierarchy of another handle, then a hierarchy whose last refresh failed, before the placement of the blocks
    refused(b"another handle", amg=G._a, h=A2._h, u=host.ctypes.data)
    rows = np.repeat(np.arange(n), np.diff(rp))
    zero = np.array(va)
    zero[int(np.flatnonzero((rows == ci) & (rows == 40))[0])] = 0.0
    with pytest.raises(_lib.CfsHipError):
        G.update_values(zero)
    refused(b"the last refresh failed", amg=G._a, u=host.ctypes.data)
    G.update_values(np.array(va))
    # a shard is CFS_HIP_ERR_UNSUPPORTED, before the placement of the blocks
    S = cfs.SymMatrix(n, rp, ci, va, row_splits=np.array([0, n // 2, n], np.int32), rank=1)
    refused(b"shard", code=_lib.ERR_UNSUPPORTED, h=S._h, u=host.ctypes.data)
    refused(b"shard", code=_lib.ERR_UNSUPPORTED, h=S._h, amg=G._a, u=host.ctypes.data)
    S.close()
    # a diagonal entry that is not positive refuses the whole call: no column is solved
    bad = np.array(va)
    bad[int(np.flatnonzero((rows == ci) & (rows == 40))[0])] = -1.5
    N = cfs.SymMatrix(n, rp, ci, bad)
    refused(b"positive diagonal", h=N._h)
    refused(b"positive definite", h=N._h, block_rows=3)
    N.close()
    # ld = n is fine for one column
    one = Blocks(B, X0, 1, ld=n)
    U, Bv = one.views()
    its, res = A.pcg_cols(U, Bv, tol=TOL[dtype])
    assert its[0] >= 1 and res[0] <= 10 * TOL[dtype] and not [e for e in one.check(None) if "B or" in e]
    G.close()
    A2.close()
    A.close()


def test_the_host_driven_model_agrees():
    """solver.pcg_cols (one host-driven solve per column) and solver.pcg_cols_native solve the same systems"""
    import torch
    import cfs_spmv_amd as cfs
    from cfs_spmv_amd import solver
    n, rp, ci, va = _unscaled("rand257")  # (diagonally dominant and not scaled: the plain iteration converges too)
    va = np.asarray(va, np.float64)
    B = torch.from_numpy(np.random.default_rng(7).uniform(-1, 1, (n, 3))).cuda()
    A = cfs.SymMatrix(n, rp, ci, va)
    G = A.amg(rp, ci, va, coarse_max=40)
    for kw in (dict(precond="jacobi"), dict(precond="block_jacobi", block=3), dict(precond="none"), dict(precond="amg", amg=G)):
        U0, it0, res0 = solver.pcg_cols(A, B, tol=1e-10, **kw)
        U1, it1, res1 = solver.pcg_cols_native(A, B, tol=1e-10, **kw)
        assert np.all(np.abs(it0 - it1) <= 2) and np.all(res0 <= 1e-9) and np.all(res1 <= 1e-9), (kw, it0, it1, res0, res1)
        assert U1.stride() == (1, 258) and U0.stride() == (1, 258)
    G.close()
    A.close()
