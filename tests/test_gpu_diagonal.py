"""SymMatrix.diagonal() / cfs_hip_sym_diagonal_async: the diagonal of the rows a handle owns, gathered by
cfs_diag_gather_kernel from the handle's DEVICE arrays (tiles, rowinfo, diag in virtual-row order, the
own-row slots of slot_col).  It is a copy, so every case asks for EXACT equality, bit for bit, with

    scipy.sparse.csr_matrix((values.astype(dtype), colind, rowptr)).diagonal().astype(dtype)

(0 where the matrix stores no diagonal entry).  Every call writes into a buffer that is larger than the
block on both sides and filled with a sentinel: the guard regions must come back untouched, and -- the
launch zeroes nothing first and uses no atomics -- every entry of the block must have been written.
"""
import numpy as np
import pytest

from test_gpu_cg_steps import _matrix
from test_gpu_kernel_variants import PLAN_KNOBS

pytestmark = pytest.mark.gpu

NO_REORDER, CLUSTER, NO_CALIBRATE, EXCHANGE, HYB, DET = 8, 16, 32, 64, 128, 1024
DTYPES = pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
SENTINEL = -777.25
LEAD, TRAIL = 256, 1024  # guard entries before / behind the block (LEAD keeps the block 16-byte aligned)


@pytest.fixture(autouse=True)
def _torch_first(monkeypatch):
    """torch brings a HIP runtime of its own: it has to initialise before libcfs_hip.so's"""
    import torch
    torch.cuda.init()
    torch.cuda.set_device(0)
    for k in PLAN_KNOBS:
        monkeypatch.delenv(k, raising=False)
    yield


def _expected(n, rp, ci, va, dtype, lo=0, hi=None):
    import scipy.sparse as sp
    d = sp.csr_matrix((va.astype(dtype), ci, rp), shape=(n, n)).diagonal().astype(dtype)
    return d[lo:n if hi is None else hi]


def _same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def _diagonal(A, dtype, stream=None):
    """A.diagonal() into the middle of a guarded buffer; returns the block after checking the guards"""
    import torch
    rows = A.row_end - A.row_begin
    buf = torch.full((LEAD + rows + TRAIL,), SENTINEL, dtype=torch.from_numpy(np.zeros(1, dtype)).dtype, device="cuda")
    torch.cuda.synchronize()
    out = A.diagonal(out=buf[LEAD:LEAD + rows], stream=stream)
    torch.cuda.synchronize()
    assert out.data_ptr() == buf.data_ptr() + LEAD * np.dtype(dtype).itemsize
    h = buf.cpu().numpy()
    guard = np.full(1, SENTINEL, dtype)
    assert _same_bits(h[:LEAD], np.repeat(guard, LEAD)), "the launch wrote in front of the block"
    assert _same_bits(h[LEAD + rows:], np.repeat(guard, TRAIL)), "the launch wrote behind the block"
    return h[LEAD:LEAD + rows].copy()


def _check(n, rp, ci, va, dtype, options=None, what=""):
    import cfs_spmv_amd as cfs
    va = va.astype(dtype)
    A = cfs.SymMatrix(n, rp, ci, va, options=options)
    got, want = _diagonal(A, dtype), _expected(n, rp, ci, va, dtype)
    assert _same_bits(got, want), f"{what}: {int(np.sum(got != want))} of {n} entries differ"
    # a fresh tensor of the right type and length when none is given
    d = A.diagonal()
    import torch
    torch.cuda.synchronize()
    assert d.is_cuda and d.numel() == n and _same_bits(d.cpu().numpy(), want)
    A.close()


STAND_INS = ["pwtk@0.05", "Flan_1565@0.01"]
SIZES = [f"rand{n}" for n in (1, 2, 63, 64, 65, 1023, 1026)] + ["band600001"]


@DTYPES
@pytest.mark.parametrize("name", STAND_INS + SIZES)
def test_diagonal_is_an_exact_copy(name, dtype):
    import cfs_spmv_amd as cfs
    n, rp, ci, va = _matrix(name)
    _check(n, rp, ci, va, dtype, what=name)
    if name in STAND_INS:  # signed and tiny entries keep their bits too
        va = np.array(va, np.float64)
        rows = np.repeat(np.arange(n), np.diff(rp))
        on = np.flatnonzero(rows == ci)
        va[on[::5]] *= -1.0
        va[on[2::11]] = 1e-300 if dtype == np.float64 else 1e-42  # (fp32: a denormal)
        _check(n, rp, ci, va, dtype, options=cfs.make_options(flags=NO_CALIBRATE), what=name + " signed")


@DTYPES
@pytest.mark.parametrize("flags", [NO_REORDER, CLUSTER], ids=["natural", "clustered"])
@pytest.mark.parametrize("name", ["Flan_1565@0.02", "rand1026"])
def test_forced_row_orders(name, flags, dtype):
    import cfs_spmv_amd as cfs
    n, rp, ci, va = _matrix(name)
    _check(n, rp, ci, va, dtype, options=cfs.make_options(flags=flags | NO_CALIBRATE), what=f"{name} flags={flags}")


@DTYPES
@pytest.mark.parametrize("block", [256, 512, 1024])
@pytest.mark.parametrize("flags", [0, NO_REORDER], ids=["default", "natural"])
def test_all_three_window_shapes(block, flags, dtype):
    import cfs_spmv_amd as cfs
    n, rp, ci, va = _matrix("Flan_1565@0.03")
    _check(n, rp, ci, va, dtype, options=cfs.make_options(block_threads=block, flags=flags | NO_CALIBRATE),
           what=f"block_threads={block}")


@DTYPES
@pytest.mark.parametrize("flags", [HYB, HYB | NO_REORDER, DET, DET | NO_REORDER, "host", "host-natural"])
def test_hyb_deterministic_and_host_built_schedules(flags, dtype):
    import cfs_spmv_amd as cfs
    if isinstance(flags, str):
        flags = cfs.FLAG_HOST_PLAN | (NO_REORDER if flags.endswith("natural") else 0)
    n, rp, ci, va = _matrix("ldoor@0.05")
    _check(n, rp, ci, va, dtype, options=cfs.make_options(flags=flags | NO_CALIBRATE), what=f"ldoor flags={flags}")


@DTYPES
@pytest.mark.parametrize("flags", [0, NO_REORDER], ids=["default", "natural"])
def test_rows_split_into_several_virtual_rows(flags, dtype):
    """a few rows 50 times longer than the rest: each is cut into chunks with a lane of their own, and only
    the first chunk carries the diagonal -- the row must still be written once, with that value"""
    import scipy.sparse as sp
    import cfs_spmv_amd as cfs
    n = 6000
    rng = np.random.default_rng(11)
    rows, cols = [], []
    for i in range(1, n):
        c = np.unique(rng.integers(max(0, i - 1500), i, size=min(600 if i % 997 == 0 else 12, i)))
        rows.append(np.full(c.size, i))
        cols.append(c)
    r, c = np.concatenate(rows), np.concatenate(cols)
    L = sp.coo_matrix((rng.uniform(-1, 1, r.size), (r, c)), shape=(n, n)).tocsr()
    d = rng.uniform(1, 2, n)
    d[997::1994] = 0.0  # ... and some of the long rows store no diagonal at all
    A = (L + L.T + sp.diags(d)).tocsr()
    A.eliminate_zeros()
    A.sort_indices()
    _check(n, A.indptr.astype(np.int32), A.indices.astype(np.int32), A.data, dtype,
           options=cfs.make_options(max_slots=2496, flags=flags | NO_CALIBRATE), what="split rows")


@DTYPES
@pytest.mark.parametrize("flags", [0, NO_REORDER, HYB, DET], ids=["default", "natural", "hyb", "det"])
def test_a_third_of_the_diagonal_is_not_stored(flags, dtype):
    import cfs_spmv_amd as cfs
    n, rp, ci, va = _matrix("Flan_1565@0.02")
    rows = np.repeat(np.arange(n), np.diff(rp))
    keep = ~((rows == ci) & (rows % 3 == 1))
    rp2 = np.concatenate([[0], np.cumsum(np.bincount(rows[keep], minlength=n))]).astype(np.int32)
    ci2, va2 = ci[keep], va[keep]
    want = _expected(n, rp2, ci2, va2, dtype)
    assert np.count_nonzero(want == 0) == len(range(1, n, 3)) and np.count_nonzero(want) == n - len(range(1, n, 3))
    _check(n, rp2, ci2, va2, dtype, options=cfs.make_options(flags=flags | NO_CALIBRATE), what="missing diagonal")


@DTYPES
def test_shards_return_their_block(dtype):
    import cfs_spmv_amd as cfs
    n, rp, ci, va = _matrix("Flan_1565@0.03")
    va = va.astype(dtype)
    for nranks, flags in ((3, 0), (3, NO_REORDER), (2, EXCHANGE), (2, EXCHANGE | NO_REORDER)):
        rs = cfs.balanced_splits(n, rp, ci, nranks)
        for rank in range(nranks):
            S = cfs.SymMatrix(n, rp, ci, va, options=cfs.make_options(flags=flags | NO_CALIBRATE), row_splits=rs, rank=rank)
            assert (S.row_begin, S.row_end) == (int(rs[rank]), int(rs[rank + 1]))
            assert (S.stats()["remote_vals"] > 0) == bool(flags & EXCHANGE and rank > 0)
            got = _diagonal(S, dtype)
            assert _same_bits(got, _expected(n, rp, ci, va, dtype, S.row_begin, S.row_end)), (nranks, flags, rank)
            S.close()


@DTYPES
@pytest.mark.parametrize("flags", [0, EXCHANGE], ids=["mirrored", "exchange"])
def test_two_shard_handle_returns_the_whole_diagonal(flags, dtype):
    """cfs_hip_sym_create_multi_*, both shards on this device: every shard gathers its block on its own stream;
    REPLICATE_ALL (2) brings the blocks home through the copy path, PEER (0) / REPLICATE (1) write in place"""
    import torch
    import cfs_spmv_amd as cfs
    from cfs_spmv_amd import _lib
    n, rp, ci, va = _matrix("band20001")
    va = va.astype(dtype)
    M = cfs.SymMatrix(n, rp, ci, va, options=cfs.make_options(flags=flags), ngpus=2)
    want = _expected(n, rp, ci, va, dtype)
    side = torch.cuda.Stream()
    for mode in (2, 0, 1):
        _lib.check(_lib.load().cfs_hip_sym_multi_set_xmode(M._h, mode))
        for stream in (None, side):
            assert _same_bits(_diagonal(M, dtype, stream=stream), want), (mode, stream)
    M.close()


@DTYPES
@pytest.mark.parametrize("flags", [0, NO_REORDER, HYB], ids=["default", "natural", "hyb"])
def test_diagonal_follows_update_values(flags, dtype):
    import cfs_spmv_amd as cfs
    n, rp, ci, va = _matrix("ldoor@0.05")
    va = va.astype(dtype)
    A = cfs.SymMatrix(n, rp, ci, va, options=cfs.make_options(flags=flags | NO_CALIBRATE | cfs.FLAG_KEEP_VALUE_MAP))
    assert _same_bits(_diagonal(A, dtype), _expected(n, rp, ci, va, dtype))
    rows = np.repeat(np.arange(n), np.diff(rp))
    va2 = (va.astype(np.float64) * (0.5 + ((rows * 31 + ci * 17) % 13) / 13.0) + 0.125 * ((rows + ci) % 3)).astype(dtype)
    A.update_values(va2)
    want = _expected(n, rp, ci, va2, dtype)
    assert not _same_bits(want, _expected(n, rp, ci, va, dtype))
    assert _same_bits(_diagonal(A, dtype), want)
    A.close()
    M = cfs.SymMatrix(n, rp, ci, va, options=cfs.make_options(flags=flags | cfs.FLAG_KEEP_VALUE_MAP), ngpus=2)
    M.update_values(va2)
    assert _same_bits(_diagonal(M, dtype), want)
    M.close()


@DTYPES
def test_argument_checks(dtype):
    import torch
    import cfs_spmv_amd as cfs
    from cfs_spmv_amd import _lib
    lib = _lib.load()
    n, rp, ci, va = _matrix("rand1023")
    A = cfs.SymMatrix(n, rp, ci, va.astype(dtype))
    host = np.zeros(n, dtype)
    good = torch.zeros(n, dtype=torch.from_numpy(host).dtype, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream
    assert lib.cfs_hip_sym_diagonal_async(A._h, host.ctypes.data, stream) == _lib.ERR_ARG  # a host pointer
    assert b"device pointer" in lib.cfs_hip_last_error()
    assert not host.any()
    assert lib.cfs_hip_sym_diagonal_async(A._h, None, stream) == _lib.ERR_ARG
    assert lib.cfs_hip_sym_diagonal_async(None, good.data_ptr(), stream) == _lib.ERR_ARG
    assert lib.cfs_hip_sym_diagonal_async(A._h, good.data_ptr(), stream) == 0
    # the Python mirror refuses a tensor it could not fill
    with pytest.raises(ValueError):
        A.diagonal(out=torch.zeros(n - 1, dtype=good.dtype, device="cuda"))
    with pytest.raises(ValueError):
        A.diagonal(out=torch.zeros(n, dtype=torch.float16, device="cuda"))
    torch.cuda.synchronize()
    A.close()
