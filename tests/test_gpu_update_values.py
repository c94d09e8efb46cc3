"""cfs_hip_sym_update_values_*: a refreshed handle IS the handle a fresh tune() of the new values gives.

A pour has no rounding in it, so nothing here has a tolerance (the one exception: the solver iterates of part 7,
which keep the rule of the harnesses they borrow, 4 d_k + 16 u).

Inputs (rand_matrices.exact_values / exact_x / exact_product): the caller's array holds, at every position with
col <= row, a small integer that depends on the POSITION, not on the pair (min, max), and NaN at every position with
col > row.  A value read from the upper triangle is a NaN in y; a value read from a wrong lower position is a wrong
integer.  The reference product is computed in int64 from the lower triangle alone, and the helper asserts -- from
the reference alone -- that max_i sum_j |a_ij| |x_j| < 2^24, so every partial sum is exact in fp32 and fp64 in any
order; y is compared with np.array_equal.

1. digest identity: create(v1) -> update_values(v2) against an independent host build of v2, every digest word
   but device_built (vals, cvals, fvals, diag, their maps, every schedule array), for the device builder, the host
   builder and a handle loaded from a plan file; whole matrices (natural, clustered, HYB, HYB + clustered) and
   every rank of 3-way mirrored (natural and clustered order), mirrored + HYB and exchange-form splits
2. round trip v1 -> v2 -> v1, host and device pointers
3. the exact product after every update of 1. (shards: spmv_phases; exchange form: assembled over the ranks)
4. multi-device handles (3 shards on one device): mirrored, reduce-scatter, sparse
5. rows without a stored diagonal, n = 1, 2, 17, and the matrix without any entry
6. more values than one grid of cfs_value_scatter_kernel covers (256 x 4 096)
7. PCG (Jacobi), block-Jacobi PCG and MINRES (Jacobi, shifted) follow the update: the existing step harnesses
8. refusals leave the handle alone
9. the values are in place when the call returns: an SpMV on a second, non-blocking stream sees them
"""
import numpy as np
import pytest

import cfs_spmv_amd as cfs
from cfs_spmv_amd import _lib, synth
from rand_matrices import (banded_mesh, banded_spd, exact_matrix, exact_product, exact_values, exact_x, random_matrix,
                           sym_int_product, sym_int_values, without_diagonal)
from test_gpu_kernel_variants import PLAN_KNOBS, _group_features
from test_gpu_parity import exchange_spmv

pytestmark = pytest.mark.gpu

NO_REORDER, CLUSTER, NO_CALIBRATE, EXCHANGE, HYB, DET = 8, 16, 32, 64, 128, 1024
KEEP, HOST_PLAN = cfs.FLAG_KEEP_VALUE_MAP, cfs.FLAG_HOST_PLAN
DTYPES = pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
ONE_GRID = 256 * 4096  # threads of one grid of cfs_value_scatter_kernel
F_STREAM, F_COO = 5, 7  # cfs_hip_sym_debug_group_features: packet-stream entries, COO leftovers

# form -> (stand-in, scale, flags, max_slots, ranks)
FORMS = {
    "natural": ("Flan_1565", 0.05, NO_REORDER, 0, 1),
    "clustered": ("Flan_1565", 0.05, CLUSTER, 0, 1),
    "hyb": ("ldoor", 0.1, HYB, 0, 1),
    "hyb+clustered": ("ldoor", 0.1, HYB | CLUSTER, 1024, 1),
    "mirrored": ("Flan_1565", 0.05, NO_REORDER, 0, 3),
    "mirrored+clustered": ("Flan_1565", 0.05, CLUSTER, 0, 3),  # (the other way to the lower entry (c, i): both orders)
    "mirrored+hyb": ("ldoor", 0.1, HYB, 0, 3),
    "exchange": ("Flan_1565", 0.05, EXCHANGE, 0, 3),
}
SEED1, SEED2, SEEDX = 1, 2, 3


@pytest.fixture(autouse=True)
def _torch_first(monkeypatch):
    """torch brings a HIP runtime of its own: it has to initialise before libcfs_hip.so's"""
    import torch
    torch.cuda.init()
    torch.cuda.set_device(0)
    for k in PLAN_KNOBS + ("CFS_HIP_NT", "CFS_HIP_COMBINE", "CFS_HIP_TAKE_HYB", "CFS_HIP_SHAPE", "CFS_HIP_KEEP_ALT",
                           "CFS_HIP_DEVICE_PLAN", "CFS_MULTI_EXCHANGE", "CFS_MULTI_TRANSPORT", "CFS_MULTI_X",
                           "CFS_HIP_CG_GRAPH"):
        monkeypatch.delenv(k, raising=False)
    yield


# ---- inputs and references, computed once ------------------------------------------------------------------
_CASES, _FRESH = {}, {}


def _case(name, scale):
    """pattern, row splits, x and the two int64 reference products of a stand-in (shared, never changed)"""
    if (name, scale) not in _CASES:
        n, rp, ci = synth.generate(name, scale)[:3]
        x = exact_x(n, SEEDX)
        ref = {s: exact_product(n, rp, ci, exact_values(n, rp, ci, s), x) for s in (SEED1, SEED2)}
        for r in ref.values():
            r.setflags(write=False)
        _CASES[name, scale] = dict(n=n, rp=rp, ci=ci, x=x, ref=ref, rs=cfs.balanced_splits(n, rp, ci, 3))
    return _CASES[name, scale]


def _values(c, seed, dtype):
    return exact_values(c["n"], c["rp"], c["ci"], seed, dtype)


def _create(c, va, flags, slots=0, ranks=1, rank=0):
    kw = dict(row_splits=c["rs"], rank=rank) if ranks > 1 else {}
    return cfs.SymMatrix(c["n"], c["rp"], c["ci"], va, options=cfs.make_options(slots, 0, 0, flags | KEEP | NO_CALIBRATE), **kw)


def _fresh_digest(form, dtype, rank):
    """digest of an independent host build of the SEED2 values"""
    key = (form, dtype, rank)
    if key not in _FRESH:
        name, scale, flags, slots, ranks = FORMS[form]
        c = _case(name, scale)
        B = _create(c, _values(c, SEED2, dtype), flags | HOST_PLAN, slots, ranks, rank)
        _FRESH[key] = B.digest()
        assert _FRESH[key]["device_built"] == 0
        B.close()
    return _FRESH[key]


def _same_but_builder(got, want, what):
    diff = [k for k in want if k != "device_built" and got[k] != want[k]]
    assert not diff, f"{what}: digest words {diff} differ"


def _exact(y, ref, what):
    assert np.all(np.isfinite(y)), f"{what}: {int((~np.isfinite(y)).sum())} non-finite rows, first {int(np.flatnonzero(~np.isfinite(y))[0])}"
    bad = np.flatnonzero(y.astype(np.int64) != ref)
    assert bad.size == 0 and np.array_equal(y, ref.astype(y.dtype)), f"{what}: {bad.size} wrong rows, first {bad[:5]}"


def _tdt(dtype):
    import torch
    return torch.float64 if dtype == np.float64 else torch.float32


def _whole_product(A, x, dtype, stream=None):
    import torch
    xd = torch.from_numpy(x.astype(dtype)).cuda()
    yd = torch.full((x.size,), float("nan"), dtype=_tdt(dtype), device="cuda")
    torch.cuda.synchronize()
    A.dense_vector_multiply(yd, xd, stream=stream)
    torch.cuda.synchronize()
    return yd.cpu().numpy()


def _shard_product(shards, c, dtype):
    """y over the ranks: a mirrored shard's block is complete after the tile kernel and the halo fold; the
    exchange form is assembled over the ranks (test_gpu_parity.exchange_spmv: pack, routing, owner-side fold)"""
    import torch
    xd = torch.from_numpy(c["x"].astype(dtype)).cuda()
    if any(s.send_rows().size for s in shards):
        return exchange_spmv(shards, c["rs"], xd, torch, prefill=float("nan"))
    y = np.zeros(c["n"], dtype)
    for r, s in enumerate(shards):
        yb = torch.full((s.row_end - s.row_begin,), float("nan"), dtype=_tdt(dtype), device="cuda")
        s.spmv_phases(yb, xd, None, 3)
        torch.cuda.synchronize()
        y[c["rs"][r]:c["rs"][r + 1]] = yb.cpu().numpy()
    return y


def _product(handles, c, dtype):
    return _whole_product(handles[0], c["x"], dtype) if len(handles) == 1 and handles[0].nranks == 1 else _shard_product(handles, c, dtype)


def _covers(A, form, rank, ranks):
    """the arrays the case claims to cover are not empty"""
    f, st, d = _group_features(A), A.stats(), A.digest()
    assert f[:, F_STREAM].sum() > 0 and d["vals"] != 0 and d["val_map"] != 0, "no packets"
    assert f[:, F_COO].sum() > 0 and d["cvals"] != 0 and d["cval_map"] != 0, "no COO leftovers"
    assert d["diag"] != 0 and d["diag_map"] != 0
    if "hyb" in form:
        assert st["far_entries"] > 0 and d["fvals"] != 0 and d["fval_map"] != 0, "no far entries"
    if form.startswith("mirrored") and rank < ranks - 1:
        assert st["mirror_entries"] > 0, "no one-sided entries"
    if form == "exchange" and rank > 0:
        assert st["remote_vals"] > 0 and d["send_idx"] != 0


# ---- 1. + 3. a refreshed handle is the fresh handle, and multiplies exactly --------------------------------
# every form from the device builder and from the host builder; a handle loaded from a plan file once per kind
BUILDS = [(form, source) for form in FORMS for source in ("device", "host")] + [("hyb+clustered", "loaded"),
                                                                              ("mirrored+hyb", "loaded")]


@DTYPES
@pytest.mark.parametrize("form,source", BUILDS, ids=[f"{f}-{s}" for f, s in BUILDS])
def test_refreshed_handle_is_the_fresh_handle_of_the_new_values(form, source, dtype, tmp_path):
    name, scale, flags, slots, ranks = FORMS[form]
    c = _case(name, scale)
    v1, v2 = _values(c, SEED1, dtype), _values(c, SEED2, dtype)
    handles = []
    for rank in range(ranks):
        A = _create(c, v1, flags | (HOST_PLAN if source == "host" else 0), slots, ranks, rank)
        assert A.digest()["device_built"] == (0 if source == "host" else 1), A.plan_note()
        if source == "loaded":
            path = str(tmp_path / f"rank{rank}.plan")
            A.save(path)
            A.close()
            A = cfs.SymMatrix.load(path)
            assert A.digest()["device_built"] == 1
        _covers(A, form, rank, ranks)
        handles.append(A)
    _exact(_product(handles, c, dtype), c["ref"][SEED1], f"{form} {source}: create")
    for rank, A in enumerate(handles):
        A.update_values(v2)
        _same_but_builder(A.digest(), _fresh_digest(form, dtype, rank), f"{form} {source} rank {rank}")
    _exact(_product(handles, c, dtype), c["ref"][SEED2], f"{form} {source}: after update_values")
    for A in handles:
        A.close()


# ---- 2. round trip -----------------------------------------------------------------------------------------
@DTYPES
@pytest.mark.parametrize("pointers", ["host", "device"])
@pytest.mark.parametrize("form", ["hyb+clustered", "mirrored+hyb", "exchange"])
def test_round_trip_returns_every_array(form, pointers, dtype):
    import torch
    name, scale, flags, slots, ranks = FORMS[form]
    c = _case(name, scale)
    v1, v2 = _values(c, SEED1, dtype), _values(c, SEED2, dtype)
    if pointers == "device":
        p1, p2 = torch.from_numpy(v1).cuda(), torch.from_numpy(v2).cuda()
    else:
        p1, p2 = v1, v2
    for rank in range(ranks):
        A = _create(c, v1, flags, slots, ranks, rank)
        first = A.digest()
        A.update_values(p2)
        second = A.digest()
        assert second["vals"] != first["vals"] and second["diag"] != first["diag"] and second["cvals"] != first["cvals"]
        _same_but_builder(second, _fresh_digest(form, dtype, rank), f"{form} rank {rank} ({pointers} pointer)")
        A.update_values(p1)
        assert A.digest() == first, f"{form} rank {rank}: v1 -> v2 -> v1 did not come back"
        A.close()


# ---- 4. multi-device handles -------------------------------------------------------------------------------
@DTYPES
@pytest.mark.parametrize("kind", ["mirrored", "reduce_scatter", "sparse"])
def test_multi_device_handle(kind, dtype):
    """three shards on one device; no digest, so the products: after create, after an update from a host pointer,
    after one from a device pointer -- and, in exchange form, under the other exchange form as well"""
    import torch
    c = _case("Flan_1565", 0.05)
    v1, v2 = _values(c, SEED1, dtype), _values(c, SEED2, dtype)
    flags = KEEP | NO_CALIBRATE | (0 if kind == "mirrored" else EXCHANGE)
    A = cfs.SymMatrix(c["n"], c["rp"], c["ci"], v1, options=cfs.make_options(flags=flags), ngpus=3, devices=[0, 0, 0])
    if kind != "mirrored":
        A.set_exchange(kind)
        form = {"reduce_scatter": cfs.EXCHANGE_REDUCE_SCATTER, "sparse": cfs.EXCHANGE_SPARSE}[kind]
        assert A.exchange_info()["form"] == form and A.exchange_info()["values_moved"] > 0
    _exact(_whole_product(A, c["x"], dtype), c["ref"][SEED1], f"{kind}: create")
    A.update_values(v2)
    _exact(_whole_product(A, c["x"], dtype), c["ref"][SEED2], f"{kind}: host pointer")
    A.update_values(torch.from_numpy(v1).cuda())
    _exact(_whole_product(A, c["x"], dtype), c["ref"][SEED1], f"{kind}: device pointer")
    if kind != "mirrored":
        A.set_exchange("sparse" if kind == "reduce_scatter" else "reduce_scatter")
        A.update_values(v2)
        _exact(_whole_product(A, c["x"], dtype), c["ref"][SEED2], f"{kind}: the other form")
    A.close()


# ---- 5. rows without a stored diagonal, tiny matrices ------------------------------------------------------
def _no_diag_pattern(n):
    """every third row (1, 4, 7, ...) stores no diagonal entry (random_matrix leaves out a few more, and has empty rows)"""
    if n > 100:
        n, M = random_matrix(np.random.default_rng(n), n, "nodes")
        rp, ci = M.indptr.astype(np.int32), M.indices.astype(np.int32)
    else:
        n, rp, ci, _ = banded_spd(n, 3, 1)
    rp, ci = without_diagonal(n, rp, ci, np.arange(n) % 3 == 1)
    return n, rp, ci


def _expected_diag_and_blocks(n, rp, ci, va, bs, dtype):
    M = exact_matrix(n, rp, ci, va).tocoo()
    d = np.zeros(n, dtype)
    on = M.row == M.col
    d[M.row[on]] = M.data[on]
    nb = -(-n // bs)
    blocks = np.zeros((nb, bs, bs), dtype)
    m = M.row // bs == M.col // bs
    blocks[M.row[m] // bs, M.row[m] % bs, M.col[m] % bs] = M.data[m]
    return d, blocks


@DTYPES
@pytest.mark.parametrize("flags", [NO_REORDER, CLUSTER], ids=["natural", "clustered"])
@pytest.mark.parametrize("n", [1, 2, 17, 1500])
def test_rows_without_a_stored_diagonal(n, flags, dtype):
    import torch
    n, rp, ci = _no_diag_pattern(n)
    rows = np.repeat(np.arange(n), np.diff(rp))
    has = np.zeros(n, bool)
    has[rows[rows == ci]] = True
    assert not has[1::3].any() and (n == 1 or has[1::3].size > 0) and has[0::3].sum() + has[2::3].sum() >= n // 2
    v1, v2 = exact_values(n, rp, ci, SEED1, dtype), exact_values(n, rp, ci, SEED2, dtype)
    x = exact_x(n, SEEDX)
    A = cfs.SymMatrix(n, rp, ci, v1, options=cfs.make_options(flags=flags | KEEP | NO_CALIBRATE))
    for va, what in ((v1, "create"), (v2, "after update_values")):
        if va is v2:
            A.update_values(v2)
        want_d, want_b = _expected_diag_and_blocks(n, rp, ci, va, 3, dtype)
        d = A.diagonal()
        b = A.block_diagonal(3)
        torch.cuda.synchronize()
        d, b = d.cpu().numpy(), b.cpu().numpy()
        # (bytes: +0 where no diagonal is stored, not -0)
        assert np.array_equal(d.view(np.uint8), want_d.view(np.uint8)), what
        assert np.all(np.isfinite(b)) and b.shape == want_b.shape and np.array_equal(b, want_b), what
        _exact(_whole_product(A, x, dtype), exact_product(n, rp, ci, va, x), f"n={n} {what}")
    B = cfs.SymMatrix(n, rp, ci, v2, options=cfs.make_options(flags=flags | KEEP | NO_CALIBRATE | HOST_PLAN))
    _same_but_builder(A.digest(), B.digest(), f"n={n}")
    A.close(), B.close()


@DTYPES
def test_a_matrix_without_entries(dtype):
    """n = 1, nnz = 0: there is nothing to pour.  The call succeeds as a no-op (include/cfs_hip.h), the handle is
    unchanged and still multiplies to +0; a count other than 0 is refused like any wrong count"""
    import torch
    rp, ci, va = np.zeros(2, np.int32), np.zeros(0, np.int32), np.zeros(0, dtype)
    A = cfs.SymMatrix(1, rp, ci, va, options=cfs.make_options(flags=KEEP | NO_CALIBRATE))
    first = A.digest()
    suf = "f64" if dtype == np.float64 else "f32"
    fn = getattr(_lib.load(), "cfs_hip_sym_update_values_" + suf)
    one = np.ones(1, dtype)
    assert fn(A._h, one.ctypes.data, 0) == 0, _lib.load().cfs_hip_last_error()
    assert fn(A._h, one.ctypes.data, 1) == _lib.ERR_ARG
    assert A.digest() == first
    y = _whole_product(A, np.full(1, 5.0), dtype)
    assert np.array_equal(y.view(np.uint8), np.zeros(1, dtype).view(np.uint8))
    d = A.diagonal()
    torch.cuda.synchronize()
    assert np.array_equal(d.cpu().numpy().view(np.uint8), np.zeros(1, dtype).view(np.uint8))
    A.close()


# ---- 6. more than one grid of the scatter kernel -----------------------------------------------------------
_BIG = {}


def _big():
    """banded_mesh: rows of 9 .. 11 lower entries, two packets and 1 .. 3 COO leftovers each, so 24 of a node's 30
    lower entries are in the packet stream -- 43 750 nodes put just over 256 x 4 096 values there"""
    if not _BIG:
        n, rp, ci, _ = banded_mesh(43750)
        x = exact_x(n, SEEDX)
        _BIG.update(n=n, rp=rp, ci=ci, x=x, rs=None,
                    ref={s: exact_product(n, rp, ci, exact_values(n, rp, ci, s), x) for s in (SEED1, SEED2)})
    return _BIG


@DTYPES
def test_more_values_than_one_grid_of_the_scatter_kernel(dtype):
    c = _big()
    v1, v2 = _values(c, SEED1, dtype), _values(c, SEED2, dtype)
    A = _create(c, v1, NO_REORDER)
    assert A.digest()["device_built"] == 1, A.plan_note()
    assert A.stats()["nnz_low"] > ONE_GRID
    assert _group_features(A)[:, F_STREAM].sum() > ONE_GRID  # (the packet stream alone: the loop runs twice)
    A.update_values(v2)
    B = _create(c, v2, NO_REORDER | HOST_PLAN)
    _same_but_builder(A.digest(), B.digest(), "big banded mesh")
    B.close()
    _exact(_whole_product(A, c["x"], dtype), c["ref"][SEED2], "big banded mesh: after update_values")
    A.close()


# ---- 7. the consumers that promise to follow the update ----------------------------------------------------
KS3 = (1, 2, 3)


def _updated_handle(name, dtype):
    """a handle created from the matrix of the plain solver tests and updated to its symmetric scaling S A S (the
    values of the preconditioned tests: a stale dinv or inverse block moves u_1 by orders of magnitude); the
    handle sees NaN above the diagonal at create and at update.  Returns (A, n, rp, ci, the new symmetric values)"""
    from test_gpu_cg_steps import _matrix
    from test_gpu_pcg_steps import scaled
    n, rp, ci, va = _matrix(name)
    v1, v2 = va.astype(dtype), scaled(n, rp, ci, va, dtype)
    upper = ci > np.repeat(np.arange(n), np.diff(rp))
    p1, p2 = v1.copy(), v2.copy()
    p1[upper] = np.nan
    p2[upper] = np.nan
    A = cfs.SymMatrix(n, rp, ci, p1, options=cfs.make_options(flags=KEEP | NO_CALIBRATE))
    A.update_values(p2)
    return A, n, rp, ci, v2


@DTYPES
@pytest.mark.parametrize("name", ["rand257", "band20001"])
def test_jacobi_pcg_follows_the_update(name, dtype):
    import torch
    from test_gpu_cg_steps import _rhs
    from test_gpu_pcg_steps import _check_iterates, _native
    A, n, rp, ci, v2 = _updated_handle(name, dtype)
    b = _rhs(n, dtype)
    _check_iterates(name, n, rp, ci, v2, b, dtype, lambda k: _native(A, b, torch, tol=0.0, maxiter=k)[:2],
                    label=" (after update_values)", ks=KS3)
    A.close()


@DTYPES
@pytest.mark.parametrize("name", ["rand257", "band20001"])
def test_block_jacobi_pcg_follows_the_update(name, dtype):
    """the inverse blocks come from the handle (the harness takes them as input), so they are first held against
    the long-double inverse of the NEW blocks with the rule of test_inverse_blocks_against_long_double"""
    import torch
    from test_gpu_cg_steps import UNIT, _rhs
    from test_gpu_block_pcg_steps import LD, _block_distance, _check_iterates, _minv, _native, cholesky_inverse, node_blocks
    A, n, rp, ci, v2 = _updated_handle(name, dtype)
    b = _rhs(n, dtype)
    minv = _minv(A, 3, torch)
    blocks = node_blocks(n, rp, ci, v2, 3)
    exact = cholesky_inverse(blocks, LD)
    e_ref = _block_distance(cholesky_inverse(blocks, np.float64).astype(dtype), exact)
    assert _block_distance(minv, exact) <= 4 * e_ref + 16 * UNIT[dtype]
    _check_iterates(name, n, rp, ci, v2, b, dtype, 3, minv,
                    lambda k: _native(A, b, torch, block=3, tol=0.0, maxiter=k)[:2], label=" (after update_values)", ks=KS3)
    A.close()


def _shift_between_diagonal_entries(n, rp, ci, va):
    """a shift inside the range of the diagonal (a_ii - shift takes both signs, so the |.| of M = |diag(A) - shift|
    matters) and as far from every a_ii as such a shift can be: the midpoint of the widest gap between consecutive
    entries of the sorted diagonal, among its middle half, rounded to a multiple of 1/8.  A function of the new
    values alone.  It matters: 1 / |a_ii - shift| multiplies the rounding of row i's product, and the harness's
    d_k is ONE sample of that rounding.  The shift 3.0 of test_gpu_minres_steps.py comes within 0.0099 of a
    diagonal entry of the scaled rand257; in fp32 the MI355X then deviated 5.72e-06 at k = 1 where d_1 = 8.97e-07
    allows 4.54e-06 -- on the updated handle and on a fresh handle of the same values alike, bit for bit (the
    other eleven figures of rand257 / band20001, fp64 / fp32, k = 1, 2, 3 were inside): a property of that
    shift, not of the update, so not one to test the update with."""
    from test_gpu_pcg_steps import _diag
    d = np.sort(_diag(n, rp, ci, va).astype(np.float64))
    mid = d[n // 4:n - n // 4]
    j = int(np.argmax(np.diff(mid)))
    shift = round(4 * (mid[j] + mid[j + 1])) / 8
    assert d[0] < shift < d[-1] and mid[j] < shift < mid[j + 1]
    return shift


@DTYPES
@pytest.mark.parametrize("name", ["rand257", "band20001"])
def test_shifted_jacobi_minres_follows_the_update(name, dtype):
    import torch
    from test_gpu_cg_steps import _rhs
    from test_gpu_minres_steps import _check_iterates, _native
    A, n, rp, ci, v2 = _updated_handle(name, dtype)
    b = _rhs(n, dtype)
    shift = _shift_between_diagonal_entries(n, rp, ci, v2)
    _check_iterates(name, n, rp, ci, v2, b, dtype,
                    lambda k: _native(A, b, torch, precond="jacobi", shift=shift, tol=0.0, maxiter=k)[:2],
                    label=f" jacobi shift={shift} (after update_values)", ks=KS3, precond="jacobi", shift=shift)
    A.close()


# ---- 8. refusals leave the handle alone --------------------------------------------------------------------
def _raw_update(A, ptr, cnt, suf):
    rc = getattr(_lib.load(), "cfs_hip_sym_update_values_" + suf)(A._h, ptr, cnt)
    return rc, _lib.load().cfs_hip_last_error().decode(errors="replace")


@DTYPES
def test_refusals_leave_the_handle_alone(dtype):
    c = _case("Flan_1565", 0.05)
    n, rp, ci, x = c["n"], c["rp"], c["ci"], c["x"]
    nnz = int(rp[-1])
    v1 = _values(c, SEED1, dtype)
    mine, other = ("f64", "f32") if dtype == np.float64 else ("f32", "f64")
    other_dtype = np.float32 if dtype == np.float64 else np.float64
    longer = np.concatenate([_values(c, SEED2, dtype), np.ones(1, dtype)])  # nnz + 1 readable values
    wrong_type = _values(c, SEED2, other_dtype)
    A = _create(c, v1, NO_REORDER)
    first = A.digest()

    def untouched(what):
        assert A.digest() == first, f"{what}: the handle changed"
        _exact(_whole_product(A, x, dtype), c["ref"][SEED1], what)
    for cnt in (nnz - 1, nnz + 1):
        rc, msg = _raw_update(A, longer.ctypes.data, cnt, mine)
        assert rc == _lib.ERR_ARG, (cnt, rc, msg)
        untouched(f"count {cnt - nnz:+d}")
    rc, msg = _raw_update(A, wrong_type.ctypes.data, nnz, other)
    assert rc == _lib.ERR_ARG, (rc, msg)
    untouched("the other value type's entry")
    rc, msg = _raw_update(A, None, nnz, mine)
    assert rc == _lib.ERR_ARG, (rc, msg)
    untouched("NULL values")
    A.close()
    # a handle without the map
    M = cfs.SymMatrix(n, rp, ci, v1, options=cfs.make_options(flags=NO_REORDER | NO_CALIBRATE))
    first = M.digest()
    rc, msg = _raw_update(M, longer.ctypes.data, nnz, mine)
    assert rc == _lib.ERR_ARG and "KEEP_VALUE_MAP" in msg, (rc, msg)
    assert M.digest() == first
    _exact(_whole_product(M, x, dtype), c["ref"][SEED1], "without the map")
    M.close()
    # a deterministic handle (its scale is taken from both triangles of the caller's array: symmetric integers)
    s1, xs = sym_int_values(np.random.default_rng(5), n, rp, ci, dtype)
    s2, _ = sym_int_values(np.random.default_rng(6), n, rp, ci, dtype)
    D = cfs.SymMatrix(n, rp, ci, s1, options=cfs.make_options(flags=DET | KEEP | NO_CALIBRATE))
    assert D.kernel_variant()["det"] == 1
    first = D.digest()
    rc, msg = _raw_update(D, s2.ctypes.data, nnz, mine)
    assert rc == _lib.ERR_UNSUPPORTED, (rc, msg)
    assert D.digest() == first
    _exact(_whole_product(D, xs, dtype), sym_int_product(n, rp, ci, s1, xs), "deterministic handle")
    D.close()


# ---- 9. visibility after return ----------------------------------------------------------------------------
@DTYPES
@pytest.mark.parametrize("pointers", ["host", "device"])
def test_the_values_are_in_place_when_the_call_returns(pointers, dtype):
    """an SpMV enqueued right after the call on a second, non-blocking stream multiplies with the new values"""
    import torch
    c = _case("Flan_1565", 0.05)
    v1, v2 = _values(c, SEED1, dtype), _values(c, SEED2, dtype)
    A = _create(c, v1, NO_REORDER)
    s = torch.cuda.Stream()
    xd = torch.from_numpy(c["x"].astype(dtype)).cuda()
    yd = torch.full((c["n"],), float("nan"), dtype=_tdt(dtype), device="cuda")
    p2 = torch.from_numpy(v2).cuda() if pointers == "device" else v2
    torch.cuda.synchronize()  # x, y and a device `values` array are ready: that much is the caller's to order
    A.update_values(p2)
    A.dense_vector_multiply(yd, xd, stream=s)
    s.synchronize()
    _exact(yd.cpu().numpy(), c["ref"][SEED2], f"second stream, {pointers} pointer")
    A.close()
