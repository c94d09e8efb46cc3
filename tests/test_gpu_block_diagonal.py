"""SymMatrix.block_diagonal() / cfs_hip_sym_block_diagonal_async: the bs x bs diagonal blocks of the matrix,
gathered by cfs_block_gather_kernel from the handle's DEVICE arrays -- the diagonal as
cfs_diag_gather_kernel takes it, the off-diagonal positions by the walk of cfs_plan::decode_plan (slices,
packets, leaders, the COO and the lower far section).  It is a copy, so every case asks for EXACT equality
(np.array_equal) with the blocks scattered in numpy from

    A = scipy.sparse.csr_matrix((values.astype(dtype), colind, rowptr));  A.sum_duplicates()

(0 where nothing is stored and outside the matrix in a trailing partial block), and for the BITS of
A.diagonal() in the diagonal positions.  Every call writes into a buffer that is larger than the blocks
on both sides and filled with a sentinel: the guard regions must come back untouched and every word of
the blocks must have been written.
"""
import numpy as np
import pytest

from test_gpu_cg_steps import _matrix
from test_gpu_diagonal import CLUSTER, DET, DTYPES, HYB, LEAD, NO_CALIBRATE, NO_REORDER, SENTINEL, TRAIL, _same_bits
from test_gpu_kernel_variants import PLAN_KNOBS

pytestmark = pytest.mark.gpu

BLOCKS = (1, 2, 3, 4, 6)


@pytest.fixture(autouse=True)
def _torch_first(monkeypatch):
    """torch brings a HIP runtime of its own: it has to initialise before libcfs_hip.so's"""
    import torch
    torch.cuda.init()
    torch.cuda.set_device(0)
    for k in PLAN_KNOBS:
        monkeypatch.delenv(k, raising=False)
    yield


def _expected(n, rp, ci, va, dtype, bs):
    """(blocks (nb, bs, bs), diagonal) restated in numpy"""
    import scipy.sparse as sp
    A = sp.csr_matrix((va.astype(dtype), ci.copy(), rp.copy()), shape=(n, n))  # (sum_duplicates works in place)
    A.sum_duplicates()
    coo = A.tocoo()
    m = coo.row // bs == coo.col // bs
    out = np.zeros((-(-n // bs), bs, bs), dtype)
    out[coo.row[m] // bs, coo.row[m] % bs, coo.col[m] % bs] = coo.data[m]
    return out, A.diagonal().astype(dtype)


def _blocks(A, dtype, bs, stream=None):
    """A.block_diagonal(bs) into the middle of a guarded buffer; returns the blocks after checking the guards"""
    import torch
    nb = -(-A.nrows() // bs)
    words = nb * bs * bs
    buf = torch.full((LEAD + words + TRAIL,), SENTINEL, dtype=torch.from_numpy(np.zeros(1, dtype)).dtype, device="cuda")
    torch.cuda.synchronize()
    out = A.block_diagonal(bs, out=buf[LEAD:LEAD + words], stream=stream)
    torch.cuda.synchronize()
    assert out.data_ptr() == buf.data_ptr() + LEAD * np.dtype(dtype).itemsize
    h = buf.cpu().numpy()
    guard = np.full(1, SENTINEL, dtype)
    assert _same_bits(h[:LEAD], np.repeat(guard, LEAD)), "the call wrote in front of the blocks"
    assert _same_bits(h[LEAD + words:], np.repeat(guard, TRAIL)), "the call wrote behind the blocks"
    return h[LEAD:LEAD + words].reshape(nb, bs, bs).copy()


def _compare(A, n, rp, ci, va, dtype, blocks=BLOCKS, what=""):
    for bs in blocks:
        got = _blocks(A, dtype, bs)
        want, diag = _expected(n, rp, ci, va, dtype, bs)
        assert got.dtype == want.dtype and np.array_equal(got, want), \
            f"{what} bs={bs}: {int(np.sum(got != want))} of {want.size} words differ"
        k = np.arange(n)
        assert _same_bits(got[k // bs, k % bs, k % bs], diag), f"{what} bs={bs}: the diagonal positions are not the diagonal's bits"
    if 1 in blocks:  # bs = 1 IS the diagonal
        import torch
        d = A.diagonal()
        torch.cuda.synchronize()
        assert _same_bits(_blocks(A, dtype, 1).reshape(-1), d.cpu().numpy())


def _check(n, rp, ci, va, dtype, options=None, blocks=BLOCKS, what=""):
    import cfs_spmv_amd as cfs
    va = va.astype(dtype)
    A = cfs.SymMatrix(n, rp, ci, va, options=options)
    _compare(A, n, rp, ci, va, dtype, blocks, what)
    return A


@DTYPES
@pytest.mark.parametrize("name", [f"rand{n}" for n in (1, 2, 63, 64, 65, 1023, 1026)])
def test_blocks_are_an_exact_copy(name, dtype):
    import torch
    n, rp, ci, va = _matrix(name)
    A = _check(n, rp, ci, va, dtype, what=name)
    # a fresh tensor of the right type and shape when none is given
    b = A.block_diagonal(3)
    torch.cuda.synchronize()
    assert b.is_cuda and tuple(b.shape) == (-(-n // 3), 3, 3)
    assert np.array_equal(b.cpu().numpy(), _expected(n, rp, ci, va, dtype, 3)[0])
    A.close()


@DTYPES
@pytest.mark.parametrize("name", ["pwtk@0.05", "Flan_1565@0.01", "band600001"])
def test_stand_ins(name, dtype):
    n, rp, ci, va = _matrix(name)
    _check(n, rp, ci, va, dtype, blocks=(3, 6), what=name).close()


def _options(cfs, kind):
    if kind.startswith("window"):  # a small window: node blocks are cut by tile boundaries and arrive as halo slots
        return cfs.make_options(max_slots=256, block_threads=int(kind[6:]), flags=NO_CALIBRATE)
    flags = {"natural": NO_REORDER, "clustered": CLUSTER, "hyb": HYB, "det": DET, "host": cfs.FLAG_HOST_PLAN}[kind]
    return cfs.make_options(flags=flags | NO_CALIBRATE)


@DTYPES
@pytest.mark.parametrize("kind", ["natural", "clustered", "window256", "window512", "window1024", "hyb", "det", "host"])
@pytest.mark.parametrize("name", ["Flan_1565@0.01", "rand1026"])
def test_every_build_option(name, kind, dtype):
    import cfs_spmv_amd as cfs
    n, rp, ci, va = _matrix(name)
    A = _check(n, rp, ci, va, dtype, options=_options(cfs, kind), what=f"{name} {kind}")
    if kind == "hyb":
        assert A.stats()["far_entries"] > 0
    if kind == "det":
        assert A.kernel_variant()["det"] == 1
    A.close()


@DTYPES
def test_far_entries_inside_a_node_block(dtype):
    """a tridiagonal matrix in natural order under Format::hyb with a small window: the only coupling across
    a tile boundary is the sub-diagonal entry of the tile's first row, a column the tile uses once -- a far
    entry, and inside a node block wherever the boundary is no multiple of bs"""
    import cfs_spmv_amd as cfs
    from rand_matrices import banded_spd
    n, rp, ci, va = banded_spd(3001, 1, 1)
    A = _check(n, rp, ci, va, dtype, options=cfs.make_options(max_slots=256, flags=HYB | NO_REORDER | NO_CALIBRATE),
               what="tridiagonal hyb")
    st = A.stats()
    assert st["far_entries"] > 0 and st["ntiles"] > 4
    A.close()


@DTYPES
@pytest.mark.parametrize("flags", [0, NO_REORDER], ids=["default", "natural"])
def test_rows_split_into_several_virtual_rows(flags, dtype):
    """a few rows 50 times longer than the rest (test_gpu_diagonal.py's): each is cut into chunks with a lane
    of their own; here the rows before them are made their neighbours, so the long rows have in-block entries"""
    import scipy.sparse as sp
    import cfs_spmv_amd as cfs
    n = 6000
    rng = np.random.default_rng(11)
    rows, cols = [], []
    for i in range(1, n):
        c = rng.integers(max(0, i - 1500), i, size=min(600 if i % 997 == 0 else 12, i))
        c = np.unique(np.concatenate([c, np.arange(max(0, i - 5), i)]))
        rows.append(np.full(c.size, i))
        cols.append(c)
    r, c = np.concatenate(rows), np.concatenate(cols)
    L = sp.coo_matrix((rng.uniform(-1, 1, r.size), (r, c)), shape=(n, n)).tocsr()
    d = rng.uniform(1, 2, n)
    d[997::1994] = 0.0  # ... and some of the long rows store no diagonal at all
    A = (L + L.T + sp.diags(d)).tocsr()
    A.eliminate_zeros()
    A.sort_indices()
    H = _check(n, A.indptr.astype(np.int32), A.indices.astype(np.int32), A.data, dtype,
               options=cfs.make_options(max_slots=2496, flags=flags | NO_CALIBRATE), what="split rows")
    H.close()


@DTYPES
def test_blocks_without_off_diagonal_entries_and_missing_diagonal_entries(dtype):
    n, rp, ci, va = _matrix("rand1026")
    rows = np.repeat(np.arange(n), np.diff(rp))
    # no off-diagonal entry inside the blocks of 6 that cover rows 120 .. 131 and 600 .. 605; no diagonal entry in every 7th row
    inblock = (rows // 6 == ci // 6) & (rows != ci) & np.isin(rows // 6, (20, 21, 100))
    keep = ~(inblock | ((rows == ci) & (rows % 7 == 3)))
    rp2 = np.concatenate([[0], np.cumsum(np.bincount(rows[keep], minlength=n))]).astype(np.int32)
    ci2, va2 = ci[keep], va[keep]
    want, diag = _expected(n, rp2, ci2, va2, dtype, 6)
    assert np.count_nonzero(diag == 0) == len(range(3, n, 7)) and not want[20][~np.eye(6, dtype=bool)].any()
    _check(n, rp2, ci2, va2, dtype, what="missing entries").close()
    # ... and a matrix that stores nothing but its diagonal
    import scipy.sparse as sp
    D = sp.diags(np.arange(1.0, 41.0)).tocsr()
    _check(40, D.indptr.astype(np.int32), D.indices.astype(np.int32), D.data, dtype, what="diagonal matrix").close()


@DTYPES
def test_a_position_stored_twice_holds_the_sum(dtype):
    """n = 50; (13, 12) and (40, 38) -- inside their blocks for every bs but (40, 38) at 2 and 3 -- are stored twice, in both
    triangles: two copies only, so the sum does not depend on the order"""
    import scipy.sparse as sp
    n, rp, ci, va = _matrix("rand50")
    A = sp.csr_matrix((va, ci, rp), shape=(n, n)).tolil()
    A[13, 12] = A[12, 13] = 0.375
    A[40, 38] = A[38, 40] = -0.625
    A = A.tocsr()
    A.sort_indices()
    rows = np.repeat(np.arange(n), np.diff(A.indptr))
    extra = [(13, 12, 0.3), (12, 13, 0.3), (40, 38, 0.7), (38, 40, 0.7)]
    r = np.concatenate([rows, [e[0] for e in extra]])
    c = np.concatenate([A.indices, [e[1] for e in extra]])
    v = np.concatenate([A.data, [e[2] for e in extra]])
    order = np.lexsort((c, r))  # (stable: the second copy follows the first)
    r, c, v = r[order], c[order], v[order]
    rp2 = np.concatenate([[0], np.cumsum(np.bincount(r, minlength=n))]).astype(np.int32)
    ci2 = c.astype(np.int32)
    assert rp2[-1] == A.nnz + 4
    want = _expected(n, rp2, ci2, v, dtype, 6)[0]
    assert want[2, 1, 0] == dtype(dtype(0.375) + dtype(0.3)) and want[6, 4, 2] == dtype(dtype(-0.625) + dtype(0.7))
    _check(n, rp2, ci2, v, dtype, what="duplicates").close()


@DTYPES
@pytest.mark.parametrize("flags", [0, HYB], ids=["default", "hyb"])
def test_blocks_follow_update_values(flags, dtype):
    import cfs_spmv_amd as cfs
    n, rp, ci, va = _matrix("Flan_1565@0.01")
    va = va.astype(dtype)
    A = cfs.SymMatrix(n, rp, ci, va, options=cfs.make_options(flags=flags | NO_CALIBRATE | cfs.FLAG_KEEP_VALUE_MAP))
    _compare(A, n, rp, ci, va, dtype, (3,), "before")
    rows = np.repeat(np.arange(n), np.diff(rp))
    lo, hi = np.minimum(rows, ci), np.maximum(rows, ci)  # (symmetric: a function of the unordered pair)
    va2 = (va.astype(np.float64) * (0.5 + ((hi * 31 + lo * 17) % 13) / 13.0) + 0.125 * (1 + (hi + lo) % 3)).astype(dtype)
    assert np.all(va2 != va)
    A.update_values(va2)
    _compare(A, n, rp, ci, va2, dtype, (2, 3, 6), "after update_values")
    A.close()


@DTYPES
def test_a_saved_and_loaded_handle(dtype, tmp_path):
    import cfs_spmv_amd as cfs
    n, rp, ci, va = _matrix("Flan_1565@0.01")
    va = va.astype(dtype)
    A = cfs.SymMatrix(n, rp, ci, va, options=cfs.make_options(flags=NO_CALIBRATE))
    path = str(tmp_path / "flan.plan")
    A.save(path)
    A.close()
    B = cfs.SymMatrix.load(path)
    _compare(B, n, rp, ci, va, dtype, (1, 3, 4), "loaded")
    B.close()


@DTYPES
def test_refusals(dtype):
    import torch
    import cfs_spmv_amd as cfs
    from cfs_spmv_amd import _lib
    lib = _lib.load()
    n, rp, ci, va = _matrix("rand1023")
    va = va.astype(dtype)
    stream = torch.cuda.current_stream().cuda_stream
    words = -(-n // 3) * 9
    good = torch.full((words,), SENTINEL, dtype=torch.from_numpy(va).dtype, device="cuda")
    A = cfs.SymMatrix(n, rp, ci, va)
    host = np.zeros(words, dtype)
    for f in (lib.cfs_hip_sym_block_diagonal_async, lib.cfs_hip_sym_block_inverse_async):
        assert f(A._h, 3, host.ctypes.data, stream) == _lib.ERR_ARG  # a host pointer
        assert b"device pointer" in lib.cfs_hip_last_error()
        assert not host.any()
        assert f(A._h, 3, None, stream) == _lib.ERR_ARG
        assert f(None, 3, good.data_ptr(), stream) == _lib.ERR_ARG
        for bs in (0, 5, 7, -1, 8):
            assert f(A._h, bs, good.data_ptr(), stream) == _lib.ERR_ARG and b"block_rows" in lib.cfs_hip_last_error()
    torch.cuda.synchronize()
    assert _same_bits(good.cpu().numpy(), np.full(words, SENTINEL, dtype))
    # the Python mirror refuses a tensor it could not fill
    with pytest.raises(ValueError):
        A.block_diagonal(3, out=torch.zeros(words - 1, dtype=good.dtype, device="cuda"))
    with pytest.raises(ValueError):
        A.block_diagonal(3, out=torch.zeros(words, dtype=torch.float16, device="cuda"))
    A.close()
    # a shard and a multi-device handle: blocks straddle the row splits
    S = cfs.SymMatrix(n, rp, ci, va, row_splits=np.array([0, n // 2 // 16 * 16, n], np.int32), rank=1)
    M = cfs.SymMatrix(n, rp, ci, va, ngpus=2)
    for H in (S, M):
        for bs in (1, 3):
            for call in (H.block_diagonal, H.block_inverse):
                with pytest.raises(_lib.CfsHipError) as e:
                    call(bs, out=good)
                assert e.value.code == _lib.ERR_UNSUPPORTED
        H.close()
    torch.cuda.synchronize()
    assert _same_bits(good.cpu().numpy(), np.full(words, SENTINEL, dtype))
