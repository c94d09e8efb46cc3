"""The three dense kernels of the pencil solver cfs_hip_sym_lobpcg_gen in the forms it launches them in, on the GPU: the
Gram kernel on three blocks (cfs_hip_debug_gram3_cols: G = S^T BS, H = S^T AS), the update kernel on three blocks in one
launch (cfs_hip_debug_lobpcg_update3_cols) and the residual kernel with R_i = AX_i - theta_i BX_i
(cfs_hip_sym_debug_lobpcg_residual_gen).  Inputs are uniform(-1, 1) in the value type, the three blocks hold different
data; references are evaluated in np.longdouble from the stored values.  Lists, bounds and helpers are those of
test_gpu_lobpcg_kernels.py.

Gram3.  On n x 48 blocks whose unlisted columns are NaN in all three, with the lists of solver_lists() and width_lists()
(n = 600001: 6 columns): every upper-triangle entry of G within (n + 1) 2^-53 sum_r |s_ri| |bs_rj| of the long-double
value, H the same with as; the lower triangles carry the bits of the upper ones; no NaN; the bits of the call on a
contiguous copy of the listed columns; two calls give equal bits; and G differs from the S^T S of cfs_hip_debug_gram_cols
(a kernel that still reads S twice gives exactly that).  Integer blocks (-8 .. 8) are exact.

Update3.  Every written value of each of the three blocks has the bits of the documented order restated in numpy fp64
(acc = 0; for j ascending acc = acc + a_j c_jo, a separate multiply and add; one cast); W, P with with_p = 0 and the rows
[n, ld) keep their NaN payloads in all three blocks.

Residual.  The bounds of the residual test of test_gpu_lobpcg_kernels.py with rho_r = |ax_r| + |theta| |bx_r|;
sums[2 i + 1] is still X_i . X_i; integers with block_rows = 0 give exact W and sums; with BX other than X the result
differs from cfs_hip_sym_debug_lobpcg_residual's.

Measured on the MI355X (worst error / bound): gram3 0.48 / 0.54 at n = 1 / 2 in fp64 (fp32 0.00 / 0.32), 0.04 at n = 63, 65,
below 0.005 from n = 257 on; residual_gen W 0.28-0.75 in fp64 and 0.98-1.00 in fp32 over the block sizes (the rounding to
fp32 is most of that bound), the sums below 0.01."""
import ctypes as C
import functools

import numpy as np
import pytest

from test_gpu_cg_steps import DTYPES, UNIT
from test_gpu_kernel_variants import PLAN_KNOBS
from test_gpu_lobpcg_kernels import (DP, MASKS, U, _bits, _handle, _holed, _lds, _minv, _nans, _residual_masks, _residual_reference,
                                     _stream, _update_expect, _update_forms, gram_cols, residual_gpu, solver_lists, width_lists)
from test_gpu_lobpcg_steps import LD, _block

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def _torch_first(monkeypatch):
    """torch brings a HIP runtime of its own: it has to initialise before libcfs_hip.so's"""
    import torch
    torch.cuda.init()
    torch.cuda.set_device(0)
    for k in PLAN_KNOBS:
        monkeypatch.delenv(k, raising=False)
    yield


# ---- Gram3 --------------------------------------------------------------------------------------------------------
def gram3_cols(sbuf, abuf, bbuf, ld, n, idx, itemsize):
    import cfs_spmv_amd as cfs
    from cfs_spmv_amd import _lib
    m = len(idx)
    g, hh = np.full((m, m), np.nan), np.full((m, m), np.nan)
    _lib.check(cfs.load().cfs_hip_debug_gram3_cols(sbuf.data_ptr(), abuf.data_ptr(), bbuf.data_ptr(), ld, n, m, (C.c_int * m)(*idx), itemsize,
                                                   g.ctypes.data_as(DP), hh.ctypes.data_as(DP), _stream()))
    return g, hh


@functools.lru_cache(maxsize=None)
def _gram3_case(n, dtype):
    """(S, AS, BS, and in long double S^T BS, S^T AS, |S|^T |BS|, |S|^T |AS|).  Computed once, shared, unchanged"""
    m = 6 if n > 100000 else 48
    rng = np.random.default_rng(3000 + n)
    S, AS, BS = (rng.uniform(-1, 1, (n, m)).astype(dtype) for _ in range(3))
    Sl, Al, Bl = S.astype(LD), AS.astype(LD), BS.astype(LD)
    out = S, AS, BS, Sl.T @ Bl, Sl.T @ Al, np.abs(Sl).T @ np.abs(Bl), np.abs(Sl).T @ np.abs(Al)
    for x in out:
        x.setflags(write=False)
    return out


def _gram3_lists(n):
    if n > 100000:  # a block of 6 columns, k = 2: one pair active, and every column
        return 6, {"k2-second-wp": [0, 1, 3, 5], "k2-all-wp": [0, 1, 2, 3, 4, 5]}
    return 48, dict(solver_lists(), **width_lists())


@DTYPES
@pytest.mark.parametrize("n", [1, 2, 63, 65, 257, 1023, 20001, 600001])
def test_gram3_against_long_double(n, dtype):
    import torch
    S, AS, BS, G_ref, H_ref, G_abs, H_abs = _gram3_case(n, dtype)
    ncols, lists = _gram3_lists(n)
    errors, worst = [], 0.0
    for ld in _lds(n, dtype):
        clean = [_block(X[:, :ncols], ld)[0] for X in (S, AS, BS)]
        view_of = lambda b: torch.as_strided(b, (n, ncols), (1, ld))
        for name, idx in lists.items():
            m = len(idx)
            sb, ab, bb = (_holed(c, view_of, idx, ncols) for c in clean)
            g, hh = gram3_cols(sb, ab, bb, ld, n, idx, S.itemsize)
            g2, hh2 = gram3_cols(sb, ab, bb, ld, n, idx, S.itemsize)
            tag = f"{name} ld={ld}"
            if np.isnan(g).any() or np.isnan(hh).any():
                errors.append(f"{tag}: NaN, an unlisted column was read")
                continue
            if not (np.array_equal(_bits(g), _bits(g2)) and np.array_equal(_bits(hh), _bits(hh2))):
                errors.append(f"{tag}: two calls differ")
            if ld == _lds(n, dtype)[0]:  # the contiguous copy of the listed columns, idx = 0 .. m - 1
                gc, hc = gram3_cols(*(_block(X[:, idx], ld)[0] for X in (S, AS, BS)), ld, n, list(range(m)), S.itemsize)
                if not (np.array_equal(_bits(g), _bits(gc)) and np.array_equal(_bits(hh), _bits(hc))):
                    errors.append(f"{tag}: the bits differ from the contiguous call's")
                # BS is not S: a kernel that reads S twice would give the S^T S of the two-block form
                gs = gram_cols(sb, ab, ld, n, idx, 0, S.itemsize)[0]
                if np.array_equal(_bits(np.triu(g)), _bits(np.triu(gs))):
                    errors.append(f"{tag}: G is S^T S, BS was not read")
            up = np.triu(np.ones((m, m), bool))
            for what, got, ref, ab_ in (("G", g, G_ref, G_abs), ("H", hh, H_ref, H_abs)):
                if not np.array_equal(_bits(got), _bits(got.T.copy())):
                    errors.append(f"{tag}: the lower triangle of {what} does not mirror the upper bit for bit")
                ix = np.ix_(idx, idx)
                bound = (n + 1) * 2.0 ** -53 * ab_[ix]
                err = np.abs(got.astype(LD) - ref[ix])
                ok = (err <= bound) | ~up
                with np.errstate(invalid="ignore", divide="ignore"):
                    ratio = np.where(up & (bound > 0), err / bound, 0)
                worst = max(worst, float(np.max(ratio)))
                if not np.all(ok):
                    i, j = np.argwhere(~ok)[0]
                    errors.append(f"{tag}: {what}[{i},{j}] = {got[i, j]!r}, long double {float(ref[ix][i, j])!r}, off by "
                                  f"{float(err[i, j]):.3e}, bound {float(bound[i, j]):.3e}")
    print(f"gram3 {np.dtype(dtype).name} n={n}: worst error / bound {worst:.3f}")
    assert not errors, f"n={n} {np.dtype(dtype).name}: " + "; ".join(errors[:8])


@DTYPES
@pytest.mark.parametrize("n,name", [(1, "k1-allbutfirst-w"), (65, "k2-one-wp"), (65, "m7"), (20001, "k16-alternating-wp"), (20001, "m41"),
                                    (20001, "k16-all-wp"), (1 << 18, "k2-one-wp")])
def test_gram3_of_integers_with_a_holed_list_is_exact(n, name, dtype):
    import torch
    idx = dict(solver_lists(), **width_lists())[name]
    ncols = 48 if n < 100000 else 6
    rng = np.random.default_rng(n + len(idx))
    S, AS, BS = (rng.integers(-8, 9, (n, ncols)).astype(dtype) for _ in range(3))
    ld = _lds(n, dtype)[0]
    view_of = lambda b: torch.as_strided(b, (n, ncols), (1, ld))
    g, hh = gram3_cols(*(_holed(_block(X, ld)[0], view_of, idx, ncols) for X in (S, AS, BS)), ld, n, idx, S.itemsize)
    Si, Ai, Bi = (X[:, idx].astype(np.int64) for X in (S, AS, BS))
    sym = lambda M: np.triu(M) + np.triu(M, 1).T  # (the lower triangle mirrors the upper: S^T T is not symmetric in itself)
    assert np.array_equal(g, sym(Si.T @ Bi).astype(np.float64)) and np.array_equal(hh, sym(Si.T @ Ai).astype(np.float64))
    if n >= 65:  # (on one row of small integers s_i b_j may equal s_i s_j by chance)
        assert not np.array_equal(np.triu(g), np.triu(Si.T @ Si).astype(np.float64))


# ---- update3 ------------------------------------------------------------------------------------------------------
@DTYPES
@pytest.mark.parametrize("n,k", [(n, k) for n in (1, 31, 33, 63, 65, 257, 20001) for k in (1, 4, 16)])
def test_update3_on_three_blocks_in_one_launch(n, k, dtype):
    import torch
    import cfs_spmv_amd as cfs
    from cfs_spmv_amd import _lib
    ld = _lds(n, dtype)[1]  # (one 16-byte word of rows [n, ld) behind every column)
    rng = np.random.default_rng(37 * n + k)
    errors = []
    for name, idx, with_p, _ in _update_forms(n, k):
        m, nout = len(idx), (2 * k if with_p else k)
        c = rng.uniform(-1, 1, (m, nout))
        hosts, bufs = [], []
        for b in range(3):
            # the whole buffer NaNs with distinct payloads, then the listed columns' rows [0, n) the data
            host = _nans(3 * k * ld, dtype, salt=b * 3 * k * ld).reshape(3 * k, ld).copy()
            host[idx, :n] = rng.uniform(-1, 1, (m, n)).astype(dtype)
            hosts.append(host)
            bufs.append(torch.from_numpy(host.reshape(-1)).cuda())
        _lib.check(cfs.load().cfs_hip_debug_lobpcg_update3_cols(bufs[0].data_ptr(), bufs[1].data_ptr(), bufs[2].data_ptr(), ld, n, k, m,
                                                                (C.c_int * m)(*idx), with_p, c.ctypes.data_as(DP), np.dtype(dtype).itemsize,
                                                                _stream()))
        written = list(range(k)) + (list(range(2 * k, 3 * k)) if with_p else [])
        for b, (host, buf) in enumerate(zip(hosts, bufs)):
            out = buf.cpu().numpy().reshape(3 * k, ld)
            expect = _update_expect(host[:, :n].T, idx, c, dtype)[0]
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
    assert not errors, f"n={n} k={k} {np.dtype(dtype).name}: " + "; ".join(errors[:8])


# ---- residual -----------------------------------------------------------------------------------------------------
def residual_gen_gpu(A, block_rows, X, AX, BX, theta, active, ld, wfill):
    """X, AX, BX: (k, n) host arrays; wfill: the (k, ld) host array W holds before.  Returns (W as (k, ld), sums)"""
    import torch
    from cfs_spmv_amd import _lib
    import cfs_spmv_amd as cfs
    k, n = X.shape

    def dev(a):
        full = np.zeros((k, ld), a.dtype)
        full[:, :n] = a
        return torch.from_numpy(full.reshape(-1)).cuda()
    xb, axb, bxb, wb = dev(X), dev(AX), dev(BX), torch.from_numpy(wfill.reshape(-1).copy()).cuda()
    sums = np.full(2 * k, np.nan)
    th = np.ascontiguousarray(theta, np.float64)
    _lib.check(cfs.load().cfs_hip_sym_debug_lobpcg_residual_gen(A._h, block_rows, xb.data_ptr(), axb.data_ptr(), bxb.data_ptr(), wb.data_ptr(),
                                                                ld, k, th.ctypes.data_as(DP), active, sums.ctypes.data_as(DP), _stream()))
    return wb.cpu().numpy().reshape(k, ld), sums


@DTYPES
@pytest.mark.parametrize("block_rows", [0, 1, 2, 3, 4, 6])
@pytest.mark.parametrize("name", ["rand257", "band20001"])
def test_residual_gen_kernel(name, block_rows, dtype):
    """rand257: 257 mod 2, 3, 4, 6 = 1, 2, 1, 5, a trailing partial block; band20001: more than one workgroup"""
    A = _handle(name, dtype)
    n = A.nrows()
    minv = _minv(A, block_rows, dtype)
    ld = _lds(n, dtype)[1]
    uv = 0.0 if dtype == np.float64 else UNIT[dtype]
    B = block_rows
    gamma = B * U / (1 - B * U)
    rng = np.random.default_rng(2000 * n + block_rows)
    errors, worst_w, worst_s = [], 0.0, 0.0
    for k in ((1, 8, 9, 16) if n < 1000 else (9, 16)):
        X, AX, BX = (rng.uniform(-1, 1, (k, n)).astype(dtype) for _ in range(3))
        theta = rng.uniform(-1, 1, k)
        exact, q = _residual_reference(BX, AX, theta, minv, block_rows)  # (R = AX - theta BX, rho = |ax| + |theta| |bx|)
        E = ((2 * U + U * U) + gamma * (1 + 2 * U + U * U)) * q
        bound = E + uv * (np.abs(exact) + E) + (B + 2) * 2.0 ** -64 * q
        d = AX.astype(np.float64) - theta[:, None] * BX.astype(np.float64)  # (fp64: a multiply, then a subtraction)
        terms = np.stack([d.astype(LD) ** 2, X.astype(LD) ** 2], axis=1).reshape(2 * k, n)
        sref = np.sum(terms, axis=1)
        sbound = (n + 1) * 2.0 ** -53 * sref
        wfill = _nans(k * ld, dtype).reshape(k, ld)
        for active in _residual_masks(k):
            tag = f"k={k} active={active:#x}"
            W, sums = residual_gen_gpu(A, block_rows, X, AX, BX, theta, active, ld, wfill)
            W2, sums2 = residual_gen_gpu(A, block_rows, X, AX, BX, theta, active, ld, wfill)
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
            if active == (1 << k) - 1:  # BX is not X: the standard kernel on the same X and AX gives something else
                W0, sums0 = residual_gpu(A, block_rows, X, AX, theta, active, ld, wfill)
                if np.array_equal(_bits(W), _bits(W0)) or np.array_equal(_bits(sums[0::2]), _bits(sums0[0::2])):
                    errors.append(f"{tag}: the result of the standard residual kernel, BX was not read")
                if not np.array_equal(_bits(sums[1::2]), _bits(sums0[1::2])):
                    errors.append(f"{tag}: X_i . X_i differs from the standard kernel's")
    A.close()
    print(f"residual_gen {np.dtype(dtype).name} {name} block_rows={block_rows}: W worst error / bound {worst_w:.3f}, sums {worst_s:.3f}")
    assert not errors, f"{name} block_rows={block_rows} {np.dtype(dtype).name}: " + "; ".join(errors[:8])


@DTYPES
@pytest.mark.parametrize("name,k", [("rand257", 9), ("band20001", 16)])
def test_residual_gen_of_integers_is_exact(name, k, dtype):
    A = _handle(name, dtype)
    n = A.nrows()
    ld = _lds(n, dtype)[1]
    rng = np.random.default_rng(n + k + 1)
    X, AX, BX, theta = rng.integers(-8, 9, (k, n)), rng.integers(-8, 9, (k, n)), rng.integers(-8, 9, (k, n)), rng.integers(-8, 9, k)
    wfill = _nans(k * ld, dtype).reshape(k, ld)
    active = MASKS["alternating"](k) | (1 << (k - 1))
    W, sums = residual_gen_gpu(A, 0, X.astype(dtype), AX.astype(dtype), BX.astype(dtype), theta.astype(np.float64), active, ld, wfill)
    A.close()
    R = AX - theta[:, None] * BX
    want = wfill.copy()
    on = [i for i in range(k) if (active >> i) & 1]
    want[on, :n] = R[on].astype(dtype)
    assert np.array_equal(_bits(W), _bits(want))
    assert np.array_equal(sums, np.stack([np.sum(R * R, axis=1), np.sum(X * X, axis=1)], axis=1).reshape(-1).astype(np.float64))
