"""A one-process multi-device handle (MultiSym) under a BUSY caller stream, and with row blocks that are
tiny or empty.

A handle orders its shard streams against the caller's stream through two events only (start_ recorded
on the caller's stream, done_ of every shard awaited by it), and an exchange-form handle runs the event
protocol of cfs_hip_comm_* inside.  So: chains x1 = A x0, x2 = A x1, x3 = A x2 ping-pong between two
buffers on a non-null stream that is held back by a timed torch.cuda._sleep, nothing synchronised before
the end -- a shard that reads x early, a peer copy that comes late or an exchange that reuses a buffer too
soon sees overwritten data.  Integer data (rand_matrices.sym_int_product in int64 is the reference), every
sum of magnitudes below 2^24: fp32 and fp64 are exact in any order, the comparison is equality.

Row blocks: cfs_hip_sym_balanced_splits cuts at multiples of 16, so n <= 16 * (ngpus - 1) leaves shards
without rows.  The host-side checks (no GPU) come first; on the GPU every handle kind and x mode must still write
every row of y, exactly."""
import numpy as np
import pytest
import scipy.sparse as sp

import cfs_spmv_amd as cfs
from cfs_spmv_amd import _lib
from rand_matrices import banded_mesh, scattered_mesh, sym_int_product, sym_int_values
from test_gpu_kernel_variants import PLAN_KNOBS

NO_CALIBRATE = 32
XMODE_PEER, XMODE_REPLICATE_ALL = 0, 2
KINDS = ["mirrored", "reduce_scatter", "sparse"]
DTYPES = pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
LIMIT = 1 << 24


@pytest.fixture(autouse=True)
def _torch_first(request, monkeypatch):
    """(GPU tests only) torch brings a HIP runtime of its own: it has to initialise before libcfs_hip.so's"""
    if request.node.get_closest_marker("gpu") is None:
        yield
        return
    import torch
    assert torch.cuda.is_available()
    torch.cuda.init()
    torch.cuda.set_device(0)
    for k in PLAN_KNOBS + ("CFS_HIP_CG_GRAPH", "CFS_MULTI_EXCHANGE", "CFS_MULTI_TRANSPORT", "CFS_MULTI_X"):
        monkeypatch.delenv(k, raising=False)
    yield


def _tdt(dtype):
    import torch
    return torch.float64 if dtype == np.float64 else torch.float32


def make_handle(kind, n, rp, ci, va, ngpus, xmode):
    flags = NO_CALIBRATE | (0 if kind == "mirrored" else cfs.FLAG_SHARD_EXCHANGE)
    A = cfs.SymMatrix(n, rp, ci, va, ngpus=ngpus, options=cfs.make_options(flags=flags))
    if kind == "sparse":
        A.set_exchange("sparse")
    _lib.check(_lib.load().cfs_hip_sym_multi_set_xmode(A._h, xmode))
    return A


def host_counts(n, rp, ci, va, nranks):
    """(counts[g, r], row_splits) of the exchange-form shards, host only"""
    rs = cfs.balanced_splits(n, rp, ci, nranks)
    cnt = np.zeros((nranks, nranks), np.int64)
    for g in range(nranks):
        c, rows = cfs.plan_send_info(n, rp, ci, va.astype(np.float64), nranks, g, rs, cfs.make_options(flags=NO_CALIBRATE))
        assert c.sum() == rows.size
        cnt[g] = c
    return cnt, rs


# ---------------------------------------------------------------------------------------------------
# 1. chains on a held stream
# ---------------------------------------------------------------------------------------------------
_MESH = {}


def chain_case(mesh):
    """(n, rowptr, colind, values, x0, [x1, x2, x3] in int64, diagonal): off-diagonals +-1, diagonal 1 or 2,
    x0 in -2..2 without zeros, so that three products stay far below 2^24 -- which is asserted here, on the
    sums of magnitudes, so that it holds for every partial sum in every order"""
    if mesh not in _MESH:
        n, rp, ci, _ = banded_mesh(1100, links=3, dof=3) if mesh == "banded" else scattered_mesh(1300, 3, seed=5)
        va, x = sym_int_values(np.random.default_rng(11), n, rp, ci)
        row = np.repeat(np.arange(n), np.diff(rp))
        va = np.where(row == ci, (np.abs(va) - 1) % 2 + 1, np.sign(va))
        x0 = np.sign(x) * ((np.abs(x) - 1) % 2 + 1)
        chain, absx = [], np.abs(x0).astype(np.int64)
        xk = x0.astype(np.int64)
        for _ in range(3):
            assert sym_int_product(n, rp, ci, np.abs(va), absx).max() < LIMIT
            xk = sym_int_product(n, rp, ci, va, xk)
            absx = np.abs(xk)
            chain.append(xk)
        assert np.abs(chain[-1]).max() > 1000  # (and not a chain of zeros)
        diag = np.zeros(n)
        diag[row[row == ci]] = va[row == ci]
        cnt, rs = host_counts(n, rp, ci, va, 8)
        assert (np.diff(rs) > 0).all() and (cnt[1:].sum(axis=1) > 0).all(), cnt  # every block sends to a lower one
        _MESH[mesh] = (n, rp, ci, va, x0, chain, diag)
    return _MESH[mesh]


def test_chain_cases_are_exact_in_fp32():
    """(no GPU) the magnitudes: asserted inside chain_case"""
    for mesh in ("banded", "scattered"):
        n, rp, ci, va, x0, chain, diag = chain_case(mesh)
        assert n > 3000 and len(chain) == 3 and (diag >= 1).all()
        assert np.array_equal(chain[0], sym_int_product(n, rp, ci, va, x0))


def run_chain(A, x0, dtype, forms=(None, None, None), with_diagonal=False):
    """x1 = A x0 -> b, x2 = A x1 -> a (over x0), x3 = A x2 -> b (over x1) on a held non-null stream; returns
    (x3, diagonal or None) read after ONE synchronise.  forms[k]: exchange form set before step k."""
    import torch
    from test_gpu_comm_edges import hold_cycles
    n = x0.size
    s = torch.cuda.Stream()
    a = torch.from_numpy(x0.astype(dtype)).cuda()
    b = torch.full((n,), float("nan"), dtype=_tdt(dtype), device="cuda")
    d = torch.full((n,), float("nan"), dtype=_tdt(dtype), device="cuda") if with_diagonal else None
    cycles = hold_cycles()
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        torch.cuda._sleep(cycles)
        for k, (y, x) in enumerate(((b, a), (a, b), (b, a))):
            if forms[k] is not None:
                A.set_exchange(forms[k])
            A.dense_vector_multiply(y, x, stream=s)
            if with_diagonal and k == 0:
                A.diagonal(out=d, stream=s)
        held = not s.query()
        last = b.clone()
    torch.cuda.synchronize()
    print(f"multi-ordering: caller's stream still held when the chain was enqueued: {held}")
    return last.cpu().numpy(), (d.cpu().numpy() if with_diagonal else None)


@pytest.mark.gpu
@pytest.mark.parametrize("mesh", ["banded", "scattered"])
@pytest.mark.parametrize("ngpus", [2, 3, 8])
@pytest.mark.parametrize("xmode", [XMODE_PEER, XMODE_REPLICATE_ALL], ids=["peer", "replicate_all"])
@pytest.mark.parametrize("kind", KINDS)
@DTYPES
def test_chained_spmv_on_a_held_stream(kind, xmode, ngpus, mesh, dtype):
    n, rp, ci, va, x0, chain, _ = chain_case(mesh)
    A = make_handle(kind, n, rp, ci, va.astype(dtype), ngpus, xmode)
    got, _ = run_chain(A, x0, dtype)
    A.close()
    assert np.isfinite(got).all()
    bad = np.flatnonzero(got.astype(np.int64) != chain[2])
    assert bad.size == 0 and np.array_equal(got, chain[2].astype(dtype)), (bad[:8], got[bad[:8]], chain[2][bad[:8]])


@pytest.mark.gpu
@pytest.mark.parametrize("ngpus", [3, 8])
@pytest.mark.parametrize("xmode", [XMODE_PEER, XMODE_REPLICATE_ALL], ids=["peer", "replicate_all"])
@DTYPES
def test_exchange_form_switched_inside_a_chain(xmode, ngpus, dtype):
    """dense, sparse, dense between the steps of one chain, nothing synchronised by the caller; the sparse
    form's buffers are built at that first switch, in the middle of the chain"""
    n, rp, ci, va, x0, chain, _ = chain_case("scattered")
    A = make_handle("reduce_scatter", n, rp, ci, va.astype(dtype), ngpus, xmode)
    got, _ = run_chain(A, x0, dtype, forms=("reduce_scatter", "sparse", "reduce_scatter"))
    assert A.exchange_info()["form"] == cfs.EXCHANGE_REDUCE_SCATTER
    assert np.array_equal(got, chain[2].astype(dtype))
    got, _ = run_chain(A, x0, dtype, forms=("sparse", "reduce_scatter", "sparse"))  # (both forms built by now)
    A.close()
    assert np.array_equal(got, chain[2].astype(dtype))


@pytest.mark.gpu
@pytest.mark.parametrize("xmode", [XMODE_PEER, XMODE_REPLICATE_ALL], ids=["peer", "replicate_all"])
@pytest.mark.parametrize("kind", KINDS)
@DTYPES
def test_diagonal_inside_a_chain(kind, xmode, dtype):
    """cfs_hip_sym_diagonal_async between two SpMVs of the chain (in the replicate modes it stages through
    the shards' local y blocks, which the SpMVs use too): the diagonal exactly, and the chain"""
    n, rp, ci, va, x0, chain, diag = chain_case("banded")
    A = make_handle(kind, n, rp, ci, va.astype(dtype), 3, xmode)
    got, d = run_chain(A, x0, dtype, with_diagonal=True)
    A.close()
    assert np.array_equal(d, diag.astype(dtype))
    assert np.array_equal(got, chain[2].astype(dtype))


# ---------------------------------------------------------------------------------------------------
# 2. small and empty row blocks
# ---------------------------------------------------------------------------------------------------
SMALL_N = [1, 16, 17, 33, 100]


def small_matrix(n, pattern):
    """band: row i coupled to the 3 rows before it; arrow: row i coupled to row 0 and to row i - 1, so
    every row block has entries in block 0's columns.  Integer values (sym_int_values)."""
    if pattern == "band":
        _, rp, ci, _ = banded_mesh(n, links=3, dof=1)
    else:
        i = np.arange(1, n)
        L = sp.coo_matrix((np.ones(2 * (n - 1)), (np.concatenate([i, i]), np.concatenate([np.zeros(n - 1, np.int64), i - 1]))),
                          shape=(n, n)).tocsr()
        L = sp.tril(L, k=-1)
        A = (L + L.T + sp.identity(n)).tocsr()
        A.sum_duplicates()
        A.sort_indices()
        rp, ci = A.indptr.astype(np.int32), A.indices.astype(np.int32)
    va, x = sym_int_values(np.random.default_rng(n), n, rp, ci)
    return rp, ci, va, x


@pytest.mark.parametrize("pattern", ["band", "arrow"])
@pytest.mark.parametrize("ngpus", [2, 8])
@pytest.mark.parametrize("n", SMALL_N)
def test_small_row_blocks_on_the_host(n, ngpus, pattern):
    """(no GPU) the cut, the schedule of every shard -- the empty ones included -- in both shard forms, and
    what the shards would send"""
    rp, ci, va, _ = small_matrix(n, pattern)
    rs = cfs.balanced_splits(n, rp, ci, ngpus)
    assert rs.size == ngpus + 1 and rs[0] == 0 and rs[-1] == n and (np.diff(rs) >= 0).all()
    assert (rs[:-1] % 16 == 0).all()
    if n <= 16 * (ngpus - 1):  # (cuts at multiples of 16: fewer 16-row pieces than blocks)
        assert (np.diff(rs) == 0).any()  # this is the case the test is about
    low = int(np.sum(np.repeat(np.arange(n), np.diff(rp)) > ci))
    row = np.repeat(np.arange(n), np.diff(rp))
    tot = sent = 0
    for g in range(ngpus):
        rep = cfs.plan_check(n, rp, ci, va, ngpus, g, rs, options=cfs.make_options(flags=NO_CALIBRATE))
        assert rep["mismatches"] == 0 and rep["remote_vals"] == 0, (g, rep)
        rep = cfs.plan_check(n, rp, ci, va, ngpus, g, rs, options=cfs.make_options(flags=NO_CALIBRATE | cfs.FLAG_SHARD_EXCHANGE))
        assert rep["mismatches"] == 0 and rep["mirror_entries"] == 0, (g, rep)
        tot += rep["nnz_low"]
        counts, rows = cfs.plan_send_info(n, rp, ci, va, ngpus, g, rs, cfs.make_options(flags=NO_CALIBRATE))
        assert counts.sum() == rows.size == rep["remote_vals"]
        assert not counts[g:].any()  # contributions only go to lower ranks
        # one packed value per distinct column below the block that the block's rows touch
        mine = (row >= rs[g]) & (row < rs[g + 1]) & (ci < rs[g])
        assert np.array_equal(np.sort(rows), np.unique(ci[mine]))
        if rs[g + 1] == rs[g]:
            assert rows.size == 0 and rep["nnz_low"] == 0
        sent += rows.size
    assert tot == low
    assert sent > 0 or (np.diff(rs) > 0).sum() <= 1


@pytest.mark.gpu
@pytest.mark.parametrize("ngpus", [2, 8])
@pytest.mark.parametrize("n", SMALL_N)
@DTYPES
def test_small_and_empty_row_blocks(n, ngpus, dtype):
    """every handle kind in both x modes, y pre-filled with NaN (a row nobody writes is seen), exact integer
    data; exchange_info of the two forms against the host-side send counts"""
    import torch
    for pattern in ("band", "arrow"):
        rp, ci, va, x = small_matrix(n, pattern)
        want = sym_int_product(n, rp, ci, va, x)
        assert sym_int_product(n, rp, ci, np.abs(va), np.abs(x)).max() < LIMIT
        cnt, rs = host_counts(n, rp, ci, va, ngpus)
        xd = torch.from_numpy(x.astype(dtype)).cuda()
        for kind in KINDS:
            for xmode in (XMODE_PEER, XMODE_REPLICATE_ALL):
                what = f"n={n} N={ngpus} {pattern} {kind} xmode={xmode}"
                A = make_handle(kind, n, rp, ci, va.astype(dtype), ngpus, xmode)
                if kind != "mirrored":
                    vb = np.dtype(dtype).itemsize
                    moved = int(cnt.sum()) if kind == "sparse" else ngpus * ngpus * int(np.max(np.diff(rs)))
                    form = cfs.EXCHANGE_SPARSE if kind == "sparse" else cfs.EXCHANGE_REDUCE_SCATTER
                    assert A.exchange_info() == {"form": form, "values_moved": moved, "bytes_moved": moved * vb}, what
                for _ in range(2):  # (twice: the second call reuses the exchange's buffers)
                    yd = torch.full((n,), float("nan"), dtype=_tdt(dtype), device="cuda")
                    A.dense_vector_multiply(yd, xd)
                    torch.cuda.synchronize()
                    got = yd.cpu().numpy()
                    assert np.isfinite(got).all(), (what, np.flatnonzero(~np.isfinite(got))[:8])
                    assert np.array_equal(got, want.astype(dtype)), what
                A.close()
