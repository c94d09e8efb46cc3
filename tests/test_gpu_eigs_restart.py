"""eigs_combine_kernel, the restart's V <- V_m S of cfs_hip_sym_eigs, alone on the GPU through cfs_hip_debug_eigs_combine
(the solver's own launch: the same grid rule, dynamic LDS size and upload of s), against plain references.  Inside a
whole solve a wrong kept vector is corrected by the restarts that follow; here every column is looked at.

The kernel: a workgroup stages all m columns of its R = 256 / sizeof(V) rows (32 fp64, 64 fp32) in LDS, then thread (r, g)
of R x G (G = 256 / R: 8 fp64, 4 fp32) owns row r and the columns g, g + G, ... in chunks of 8 accumulators -- a second
chunk from nout > 8 G on -- and the workgroups walk the tiles grid-stride, min(ntiles, 2048) of them.

Exact.  Basis entries and s are integers in [-8, 8]: with m <= 128 every partial sum stays below 2^13, exact in fp64 and,
rounded when stored, in fp32, in any order, so the result has to equal the integer product bit for bit.  n of SMALL_N
(one row, one short of / exactly / one beyond a tile, a few tiles with a partial last one) with every (m, nout) of
shapes(G) (one column; one chunk part full; the solver's ncv = 20 restart; 33 of 65; few of many; the first chunk full,
8 G, and one column into the second, 8 G + 1; all but one; all), and n = 2048 R + 1 (the first grid-stride trip of one
workgroup) and 600001 (ten trips in fp64, five in fp32) with (20, 12) and (128, 8 G + 1).  Every case in place (out ==
basis, ldo == ld, ld one aligned step above the tight value) and out of place (ldo != ld).  Rows [n, ld) of every basis
column, rows [n, ldo) of out, a spare column behind the last one and, out of place, columns [nout, m) of out hold a NaN of
a recognisable payload before the call: all of that is bit-intact after it, and so are columns [nout, m) of the basis in
place and the whole basis out of place.

Selection, in place.  s = the first nout columns of a random permutation matrix over uniform(-1, 1) data: 0 + 1.0 a + 0 b
... is exact, so output column c is input column perm[c] bit for bit -- whichever columns the call overwrites.  This is
the row-safety check: a workgroup that stores before it has staged its whole tile corrupts a column it has yet to read.
(n, m, nout) = (R + 1, 128, 127), (1023, 67, 53), (2048 R + 1, 20, 12), and (257, 9, 8), (1023, 9, 8), where the waves of a
workgroup stage unequal shares (m R is no multiple of 256): see the end.

Rounded.  uniform(-1, 1) data, s = the first nout columns of the Q factor of a seeded random m x m matrix, against the
long-double product.  Per entry the error may be

    (m + 1) 2^-53 sum_k |v_k| |s_kc|  +  u_V |ref|        (u_V = 2^-53 / 2^-24)

the a-priori bound of m products accumulated in fp64 (the stored values convert to fp64 exactly), and one rounding when
stored.  Two calls return the same bits.

Host memory for out or the basis is refused (the checks that need no device are in test_eigs_abi.py).

Measured on the MI355X (value type, shape: the worst error over its bound):

  f64 n=1023 m=128 nout=66: 0.028
  f32 n=1023 m=128 nout=66: 0.996
  f64 n=20001 m=65 nout=33: 0.076
  f32 n=20001 m=65 nout=33: 0.999

(in fp32 the rounding when stored is all of the error, and the bound's second term is sharp).

Tried by hand on scratch copies of the kernel, one run each:
  - the first two columns of a thread's SECOND chunk swapped when stored: every exact case fails (at nout = 127 and 128), the
    selection at nout = 127 (and at 53 in fp32) and the rounded case at nout = 66 in fp32;
  - no barrier between staging and the stores: a race, which no test can force.  In the first of two runs it was lost in the
    exact cases of n = 257 and 1023 in fp64 at (m, nout) = (9, 8) -- m R is no multiple of the 256 threads there, so some
    waves stage one value more than the others, and those run ahead -- and in no selection case; in the second run, with the
    selections at (257, 9, 8) and (1023, 9, 8) added for that reason, in no case at all.  A kernel that lacks the barrier
    is NOT reliably caught here; one that reads what it has overwritten in program order is, as the next one shows;
  - the accumulation reading the basis from memory instead of the staged tile: the selections at nout = 127 (and 53 in fp32)
    fail, the exact cases of n = 1023 and the rounded case at nout = 66.
"""
import ctypes as C
import functools

import numpy as np
import pytest

from test_gpu_cg_steps import DTYPES, UNIT
from test_gpu_kernel_variants import PLAN_KNOBS

pytestmark = pytest.mark.gpu

LD = np.longdouble
MMAX = 128


@pytest.fixture(autouse=True)
def _torch_first(monkeypatch):
    """torch brings a HIP runtime of its own: it has to initialise before libcfs_hip.so's"""
    import torch
    torch.cuda.init()
    torch.cuda.set_device(0)
    for k in PLAN_KNOBS:
        monkeypatch.delenv(k, raising=False)
    yield


def _rg(dtype):
    r = 256 // np.dtype(dtype).itemsize
    return r, 256 // r


def shapes(g):
    return [(1, 1), (2, 1), (9, 8), (20, 12), (65, 33), (128, 4), (128, 8 * g), (128, 8 * g + 1), (128, 127), (128, 128)]


def _bits(dtype):
    return np.uint64 if dtype == np.float64 else np.uint32


def _pattern(dtype):
    """a quiet NaN of a recognisable payload"""
    return np.array([0x7ff8dead0000beef], np.uint64).view(np.float64)[0] if dtype == np.float64 else \
        np.array([0x7fc0beef], np.uint32).view(np.float32)[0]


def _lds(n, dtype, steps):
    """n rounded up to 16 bytes, plus `steps` more aligned steps"""
    per = 16 // np.dtype(dtype).itemsize
    return -(-n // per) * per + steps * per


def _block(Vt, ld, dtype):
    """a device block of m + 1 columns with stride ld, as a host array (m + 1, ld) of the NaN pattern with the columns of
    Vt (m, n; column k of the basis is row k) in rows [0, n), and its device copy"""
    import torch
    m, n = Vt.shape
    host = np.full((m + 1, ld), _pattern(dtype), dtype)
    host[:m, :n] = Vt
    return host, torch.from_numpy(host).cuda()


def combine_gpu(Vt, s, nout, dtype, in_place):
    """cfs_hip_debug_eigs_combine on the columns Vt (m, n) with the first nout columns of s (m, >= nout).  Returns (out, basis
    before, basis after) as host arrays (m + 1, ldo / ld): in place out IS the basis after.  Everything outside rows
    [0, n) of the m columns is the NaN pattern before the call"""
    import torch
    import cfs_spmv_amd as cfs
    from cfs_spmv_amd import _lib
    m, n = Vt.shape
    ld, ldo = _lds(n, dtype, 1), _lds(n, dtype, 1 if in_place else 2)
    before, basis = _block(Vt, ld, dtype)
    out = basis if in_place else torch.from_numpy(np.full((m + 1, ldo), _pattern(dtype), dtype)).cuda()
    sc = np.ascontiguousarray(s[:m, :nout], np.float64)
    _lib.check(cfs.load().cfs_hip_debug_eigs_combine(out.data_ptr(), ldo, basis.data_ptr(), ld, n, m, nout,
                                                     sc.ctypes.data_as(C.POINTER(C.c_double)), np.dtype(dtype).itemsize,
                                                     torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    return out.cpu().numpy(), before, basis.cpu().numpy()


def untouched(out, before, after, n, nout, dtype, in_place):
    """the list of what was written although it is not rows [0, n) of columns [0, nout) of out"""
    bits = _bits(dtype)
    pat = np.array([_pattern(dtype)]).view(bits)[0]
    m = before.shape[0] - 1
    errors = []
    if not np.all(out[:, n:].view(bits) == pat):
        errors.append("rows [n, ldo) of out")
    if not np.all(out[m].view(bits) == pat):
        errors.append("the spare column of out")
    if in_place:
        if not np.array_equal(out[nout:m].view(bits), before[nout:m].view(bits)):
            errors.append("columns [nout, m) of the basis")
    else:
        if not np.all(out[nout:m].view(bits) == pat):
            errors.append("columns [nout, m) of out")
        if not np.array_equal(after.view(bits), before.view(bits)):
            errors.append("the basis")
    return errors


# ---- exact ----------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _integers(n, m, dtype):
    """(the columns as rows (m, n) in the value type, s (m, m) as doubles), integers in [-8, 8]: computed once, shared,
    unchanged.  The narrower shapes of this n use the leading rows / columns"""
    rng = np.random.default_rng(7000 + n)
    Vt = rng.integers(-8, 9, (m, n), dtype=np.int8).astype(dtype)
    s = rng.integers(-8, 9, (m, m)).astype(np.float64)
    Vt.setflags(write=False)
    s.setflags(write=False)
    return Vt, s


def _exact(n, cases, dtype, mmax):
    Vt, s = _integers(n, mmax, dtype)
    errors = []
    for m, nout in cases:
        if n > 4096:
            # by BLAS in fp64, where the integer product is exact as well (every sum below 2^13): int64 matmul is slow
            ref = np.rint(s[:m, :nout].T @ Vt[:m].astype(np.float64)).astype(np.int64)
        else:
            ref = s[:m, :nout].T.astype(np.int64) @ Vt[:m].astype(np.int64)
        assert np.max(np.abs(ref)) < 2 ** 13
        for in_place in (True, False):
            out, before, after = combine_gpu(Vt[:m], s, nout, dtype, in_place)
            where = f"m={m} nout={nout} {'in place' if in_place else 'out of place'}"
            got = out[:nout, :n]
            if not np.array_equal(got, ref):  # (a NaN equals nothing)
                bad = np.argwhere(got != ref)
                c, r = bad[0]
                errors.append(f"{where}: {len(bad)} wrong entries in columns {sorted(set(bad[:, 0].tolist()))[:8]}, the first "
                              f"out[{r}, {c}] = {got[c, r]!r}, not {ref[c, r]}")
            errors += [f"{where}: written: {e}" for e in untouched(out, before, after, n, nout, dtype, in_place)]
    assert not errors, f"n={n} {np.dtype(dtype).name}: " + "; ".join(errors[:8])


SMALL_N = ["1", "R-1", "R", "R+1", "257", "1023"]


def _n(text, dtype):
    return eval(text, {"R": _rg(dtype)[0]})


@DTYPES
@pytest.mark.parametrize("n", SMALL_N)
def test_integers_are_combined_exactly(n, dtype):
    _exact(_n(n, dtype), shapes(_rg(dtype)[1]), dtype, MMAX)


@DTYPES
@pytest.mark.parametrize("shape", ["20,12", "128,8*G+1"])
@pytest.mark.parametrize("n", ["2048*R+1", "600001"])
def test_integers_are_combined_exactly_beyond_one_sweep_of_the_grid(n, shape, dtype):
    r, g = _rg(dtype)
    m, nout = eval(shape, {"G": g})
    n = _n(n, dtype)
    assert (n + r - 1) // r > 2048, "the first workgroup makes a second trip"
    _exact(n, [(m, nout)], dtype, m)


# ---- selection ------------------------------------------------------------------------------------------------------
@DTYPES
@pytest.mark.parametrize("shape", ["R+1,128,127", "1023,67,53", "2048*R+1,20,12", "257,9,8", "1023,9,8"])
def test_a_selection_reproduces_the_columns_in_place(shape, dtype):
    n, m, nout = eval(shape, {"R": _rg(dtype)[0]})
    rng = np.random.default_rng(n + m)
    Vt = rng.uniform(-1, 1, (m, n)).astype(dtype)
    perm = rng.permutation(m)
    s = np.zeros((m, m))
    s[perm, np.arange(m)] = 1.0
    assert np.any(perm[:nout] > np.arange(nout)) and np.any(perm[:nout] < np.arange(nout)), "columns move both ways"
    out, before, after = combine_gpu(Vt, s, nout, dtype, True)
    bits = _bits(dtype)
    wrong = [c for c in range(nout) if not np.array_equal(out[c, :n].view(bits), Vt[perm[c]].view(bits))]
    assert not wrong, f"{len(wrong)} output columns are not the chosen input columns, the first {wrong[:8]} (chosen: {perm[wrong[:8]]})"
    assert not untouched(out, before, after, n, nout, dtype, True)


# ---- rounded --------------------------------------------------------------------------------------------------------
@DTYPES
@pytest.mark.parametrize("n,m,nout", [(1023, 128, 66), (20001, 65, 33)])
def test_against_the_long_double_product(n, m, nout, dtype):
    rng = np.random.default_rng(n + m + nout)
    Vt = rng.uniform(-1, 1, (m, n)).astype(dtype)
    s = np.ascontiguousarray(np.linalg.qr(rng.standard_normal((m, m)))[0])
    sl, vl = s[:, :nout].T.astype(LD), Vt.astype(LD)
    ref, mag = sl @ vl, np.abs(sl) @ np.abs(vl)
    bound = (m + 1) * LD(2.0) ** -53 * mag + LD(UNIT[dtype]) * np.abs(ref)
    errors, worst = [], 0.0
    for in_place in (True, False):
        out, before, after = combine_gpu(Vt, s, nout, dtype, in_place)
        out2 = combine_gpu(Vt, s, nout, dtype, in_place)[0]
        where = "in place" if in_place else "out of place"
        if not np.array_equal(out.view(_bits(dtype)), out2.view(_bits(dtype))):
            errors.append(f"{where}: two calls differ")
        err = np.abs(out[:nout, :n].astype(LD) - ref)
        worst = max(worst, float(np.max(err / bound)))
        if not np.all(err <= bound):  # (a NaN fails)
            c, r = np.unravel_index(np.argmax(np.where(np.isnan(err), np.inf, err - bound)), err.shape)
            errors.append(f"{where}: out[{r}, {c}] = {out[c, r]!r}, long double {float(ref[c, r])!r}, off by {float(err[c, r]):.3e}, "
                          f"bound {float(bound[c, r]):.3e}")
        errors += [f"{where}: written: {e}" for e in untouched(out, before, after, n, nout, dtype, in_place)]
    print(f"eigs-combine {np.dtype(dtype).name} n={n} m={m} nout={nout}: worst error / bound {worst:.3f}")
    assert not errors, f"n={n} m={m} nout={nout} {np.dtype(dtype).name}: " + "; ".join(errors)


@DTYPES
def test_memory_that_is_not_the_devices_is_refused(dtype):
    import torch
    import cfs_spmv_amd as cfs
    from cfs_spmv_amd import _lib
    lib = cfs.load()
    n, m, nout = 64, 4, 2
    dev = torch.zeros(m * n, dtype=torch.float64 if dtype == np.float64 else torch.float32, device="cuda")
    host = np.zeros(m * n + 4, dtype)
    hp = host.ctypes.data // 16 * 16 + 16  # a host pointer, 16-byte aligned
    s = np.zeros((m, nout))
    sp, vb, st = s.ctypes.data_as(C.POINTER(C.c_double)), np.dtype(dtype).itemsize, torch.cuda.current_stream().cuda_stream
    for out, basis in ((hp, dev.data_ptr()), (dev.data_ptr(), hp)):
        assert lib.cfs_hip_debug_eigs_combine(out, n, basis, n, n, m, nout, sp, vb, st) == _lib.ERR_ARG
        assert b"device memory of the current device" in lib.cfs_hip_last_error()
    torch.cuda.synchronize()
    assert not dev.any() and not host.any()
