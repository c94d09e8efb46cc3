"""cfs_fold_kernel (the halo fold and the receive fold) against long-double sums, list length by list length.

The kernel has four paths, chosen by the length L of a destination's list: L = 1, 2, 3 inlined in the
16-byte record; L = 4 .. 18 two entries in the record and up to 16 more summed by the lane, four
clamped loads at a time; L >= 19 the rest summed by the whole wave, strided, one long-list lane after
the other out of a ballot.  Every test here KNOWS the lengths it reached: SymMatrix.fold_lists()
(cfs_hip_sym_debug_fold_lists) decodes the lists from the device arrays the launch reads.

Part 1 drives the kernel alone: SymMatrix.set_recv(rows) + recv_fold(y, recv) launch it on a receive
list and a buffer the test constructs, on a whole-matrix handle and on an exchange-form shard
(row_begin != 0).  Reference: y0[dst] + sum recv[k] in np.longdouble.  The contract asserted is
  * the summation bound |err| <= gamma_L (|y0| + sum |recv[k]|), gamma_L = L u / (1 - L u), which holds
    for ANY order of the L additions -- the order itself is the implementation's to change;
  * rows that are no destination keep their bytes (NaN and +-Inf among them);
  * two launches on identical inputs give identical bytes;
  * a +Inf and a NaN entry reach exactly their own destination.

Part 2 runs the local halo fold behind the tile kernel on rand_matrices.hub_columns: hub column k
collects exactly FOLD_LENGTHS[k] strip entries, one per tile, under NO_REORDER | NO_CALIBRATE | NO_HYB
and a window smaller than the spacing of the referencing rows; y against oracle.csr_spmv_ld at the
parity suite's tolerances."""
import numpy as np
import pytest

from conftest import scaled_err
from rand_matrices import FOLD_LENGTHS, hub_columns
from test_gpu_kernel_variants import PLAN_KNOBS
from test_gpu_parity import TOL, exchange_spmv

pytestmark = pytest.mark.gpu

NO_REORDER, NO_CALIBRATE, HYB, NO_HYB, DET = 8, 32, 128, 256, 1024
UNIT = {np.float64: 2.0 ** -53, np.float32: 2.0 ** -24}
LONG = 19  # shortest list with a wave-strided part (2 in the record + 16 of the lane + 1)
VERY_LONG = 5000
N_HARNESS = 3000  # rows of the matrix the part-1 handles are built from


@pytest.fixture(autouse=True)
def _torch_first(monkeypatch):
    """torch brings a HIP runtime of its own: it has to initialise before libcfs_hip.so's"""
    import torch
    torch.cuda.init()
    torch.cuda.set_device(0)
    for k in PLAN_KNOBS:
        monkeypatch.delenv(k, raising=False)
    yield


def _tdt(dtype):
    import torch
    return torch.float64 if dtype == np.float64 else torch.float32


# ---------------------------------------------------------------------------------------------
# part 1: the kernel in isolation
# ---------------------------------------------------------------------------------------------
def _harness(dtype, shard):
    """a small handle whose receive fold the tests drive: the whole matrix, or rank 1 of 2 in the
    exchange form (row_begin != 0)"""
    import cfs_spmv_amd as cfs
    from cfs_spmv_amd import synth
    n, rp, ci, va = synth.random_symmetric(N_HARNESS, 4, seed=1, band=30)
    va = va.astype(dtype)
    if not shard:
        return cfs.SymMatrix(n, rp, ci, va, options=cfs.make_options(flags=NO_CALIBRATE))
    rs = np.array([0, 1100, n], np.int32)
    A = cfs.SymMatrix(n, rp, ci, va, options=cfs.make_options(flags=NO_CALIBRATE | cfs.FLAG_SHARD_EXCHANGE),
                      row_splits=rs, rank=1)
    assert A.row_begin == 1100 and A.row_end == n
    return A


def _cases():
    """(name, lens): list lengths of the destinations, in record (= ascending row) order"""
    rng = np.random.default_rng(2024)
    bnd = np.array(FOLD_LENGTHS)
    out = [(f"one destination, L={L}", [L]) for L in FOLD_LENGTHS + (VERY_LONG,)]
    out.append(("every boundary length once", list(rng.permutation(bnd)) + [VERY_LONG]))
    for m in (1, 63, 64, 65, 255, 256, 257):  # partial last wave / last workgroup
        out.append((f"{m} destinations, boundary lengths", list(rng.choice(bnd, m))))
    for m, at in ((130, 0), (130, 63), (130, 129), (257, 256), (64, 63)):
        lens = list(rng.integers(1, 4, m))
        lens[at] = 211
        out.append((f"{m} destinations, the one long list at record {at}", lens))
    out.append(("a wave of 64 long lists of different lengths", list(rng.permutation(LONG + 3 * np.arange(64)))))
    lens = list(rng.permutation(LONG + 5 * np.arange(64))) + list(rng.integers(1, 19, 36))
    out.append(("64 long lists, then a partial wave of short ones", lens))
    lens = list(rng.integers(1, 19, 64))
    lens[5], lens[40] = 83, 147
    out.append(("a wave with exactly two long lists", lens))
    lens = list(rng.integers(1, 19, 192))
    lens[64 + 17], lens[64 + 18] = LONG, 20
    out.append(("two long lists on neighbouring lanes of the second wave", lens))
    return out


CASES = _cases()


def _build(rng, rows, row_begin, lens, dtype):
    """destinations = a random subset of the handle's rows; the entries of a destination scattered through
    the receive buffer; signed values of mixed magnitude (sums cancel); every row of y0 distinct, rows
    that are no destination partly NaN / +-Inf"""
    lens = np.asarray(lens, np.int64)
    dst = np.sort(rng.choice(rows, lens.size, replace=False))
    recv_local = rng.permutation(np.repeat(dst, lens))
    recv = (rng.standard_normal(recv_local.size) * 10.0 ** rng.integers(-2, 3, recv_local.size)).astype(dtype)
    y0 = (rng.standard_normal(rows) + np.arange(rows)).astype(dtype)
    other = np.setdiff1d(np.arange(rows), dst)
    special = rng.choice(other, min(other.size, 30), replace=False)
    y0[special] = np.resize(np.array([np.nan, np.inf, -np.inf], dtype), special.size)
    return dst, lens, (recv_local + row_begin).astype(np.int32), recv, y0


def _reference(dst, recv_local, recv, y0):
    """(sum, sum of absolute values) per destination, in long double"""
    pos = np.searchsorted(dst, recv_local)
    s = y0[dst].astype(np.longdouble)
    a = np.abs(s)
    np.add.at(s, pos, recv.astype(np.longdouble))
    np.add.at(a, pos, np.abs(recv.astype(np.longdouble)))
    return s, a


def _fold(A, y0, recv, torch):
    y = torch.from_numpy(y0).cuda()
    A.recv_fold(y, torch.from_numpy(recv).cuda())
    torch.cuda.synchronize()
    return y.cpu().numpy()


def _bound(lens, dtype):
    Lu = lens.astype(np.longdouble) * np.longdouble(UNIT[dtype])
    return Lu / (1 - Lu)


@pytest.mark.parametrize("shard", [False, True], ids=["whole", "shard"])
@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
def test_fold_kernel_on_constructed_receive_lists(dtype, shard):
    import torch
    A = _harness(dtype, shard)
    rows, rb = A.row_end - A.row_begin, A.row_begin
    rng = np.random.default_rng(7 + shard)
    errors, seen = [], set()
    for name, lens in CASES:
        dst, lens, recv_rows, recv, y0 = _build(rng, rows, rb, lens, dtype)
        A.set_recv(recv_rows)
        gd, gl = A.fold_lists(1)
        assert np.array_equal(gd, dst) and np.array_equal(gl, lens), f"{name}: the kernel got other lists than asked for"
        seen.update(int(v) for v in lens)
        y = _fold(A, y0, recv, torch)
        ref, scale = _reference(dst, recv_rows - rb, recv, y0)
        err = np.abs(y[dst].astype(np.longdouble) - ref)
        lim = _bound(lens, dtype) * scale
        bad = np.flatnonzero(~(err <= lim))
        if bad.size:
            errors.append(f"{name}: {bad.size} destinations outside the summation bound, first: record {bad[0]} "
                          f"(lane {bad[0] % 64}) L={lens[bad[0]]} err={float(err[bad[0]]):.3e} bound={float(lim[bad[0]]):.3e}")
        keep = np.ones(rows, bool)
        keep[dst] = False
        if not np.array_equal(y[keep].view(np.uint8), y0[keep].view(np.uint8)):
            errors.append(f"{name}: a row that is no destination changed")
        if not np.array_equal(_fold(A, y0, recv, torch).view(np.uint8), y.view(np.uint8)):
            errors.append(f"{name}: two launches on identical inputs differ")
    assert not errors, "\n".join(errors)
    assert seen >= set(FOLD_LENGTHS) | {VERY_LONG}
    A.close()


@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
def test_fold_kernel_keeps_inf_and_nan_to_their_own_destination(dtype):
    """one +Inf and one NaN entry, each tried in the record, among the lane's own entries and in the
    wave-strided part (list order = ascending position in the receive buffer), in a partial wave of
    lists of every kind: only the destination of the entry changes class"""
    import torch
    A = _harness(dtype, True)
    rows, rb = A.row_end - A.row_begin, A.row_begin
    rng = np.random.default_rng(11)
    lens = list(rng.choice(np.array(FOLD_LENGTHS), 100))
    lens[3], lens[4], lens[70], lens[99] = 147, 146, 83, 3
    for (d_inf, k_inf), (d_nan, k_nan) in (((3, 100), (99, 2)), ((70, 1), (4, 19)), ((4, 10), (3, 146)), ((99, 0), (70, 17))):
        dst, ln, recv_rows, recv, y0 = _build(rng, rows, rb, lens, dtype)
        for d, k, v in ((d_inf, k_inf, np.inf), (d_nan, k_nan, np.nan)):
            recv[np.flatnonzero(recv_rows - rb == dst[d])[k]] = v
        A.set_recv(recv_rows)
        assert np.array_equal(A.fold_lists(1)[1], ln)
        y = _fold(A, y0, recv, torch)
        assert y[dst[d_inf]] == np.inf and np.isnan(y[dst[d_nan]]), (d_inf, k_inf, d_nan, k_nan)
        rest = np.setdiff1d(np.arange(len(lens)), [d_inf, d_nan])
        fin = np.where(np.isfinite(recv), recv, 0).astype(dtype)
        ref, scale = _reference(dst, recv_rows - rb, fin, y0)
        err = np.abs(y[dst].astype(np.longdouble) - ref)
        assert np.all(err[rest] <= (_bound(ln, dtype) * scale)[rest]), (d_inf, k_inf, d_nan, k_nan)
    A.close()


@pytest.mark.parametrize("shard", [False, True], ids=["whole", "shard"])
def test_set_recv_rejects_rows_outside_the_block_and_an_empty_list_folds_nothing(shard):
    import torch
    from cfs_spmv_amd import _lib
    A = _harness(np.float64, shard)
    rows, rb = A.row_end - A.row_begin, A.row_begin
    for bad in ([A.row_end], [rb, rb - 1], [rb + 5, A.row_end + 7]):
        with pytest.raises(_lib.CfsHipError) as e:
            A.set_recv(np.array(bad, np.int32))
        assert e.value.code == _lib.ERR_ARG
    y0 = np.random.default_rng(3).standard_normal(rows)
    y0[::7] = np.nan
    recv = np.ones(4)
    A.set_recv(np.array([rb, rb, A.row_end - 1], np.int32))
    assert [list(v) for v in A.fold_lists(1)] == [[0, rows - 1], [2, 1]]
    A.set_recv(np.zeros(0, np.int32))
    assert A.fold_lists(1)[0].size == 0
    assert np.array_equal(_fold(A, y0, recv, torch).view(np.uint8), y0.view(np.uint8))
    A.close()


def test_fold_lists_of_a_multi_device_handle_is_an_argument_error():
    import cfs_spmv_amd as cfs
    from cfs_spmv_amd import _lib, synth
    n, rp, ci, va = synth.random_symmetric(N_HARNESS, 4, seed=1, band=30)
    M = cfs.SymMatrix(n, rp, ci, va, ngpus=2)
    for which in (0, 1):
        with pytest.raises(_lib.CfsHipError) as e:
            M.fold_lists(which)
        assert e.value.code == _lib.ERR_ARG
    M.close()


# ---------------------------------------------------------------------------------------------
# part 2: the local halo fold behind the tile kernel, on designed list lengths
# ---------------------------------------------------------------------------------------------
SLOTS, SPACING = 512, 1100  # a tile has at most SLOTS rows: rows SPACING apart lie in different tiles
CLASSES = {"1": (1, 1), "2": (2, 2), "3": (3, 3), "4": (4, 4), "5-17": (5, 17), "18": (18, 18), "19": (19, 19),
           "20-82": (20, 82), ">=83": (83, 1 << 30)}
_HUB = {}


def _hub(dtype):
    """(n, rp, ci, va, x, y_ld, absrow, hubs, targets), the oracle computed once per value type"""
    if dtype not in _HUB:
        from oracle import oracle
        n, rp, ci, va, hubs, targets = hub_columns(spacing=SPACING)
        va = va.astype(dtype)
        x = np.random.default_rng(5).uniform(-1, 1, n).astype(dtype)
        y_ld, absrow = oracle.csr_spmv_ld(n, rp, ci, va, x)
        _HUB.clear()
        _HUB[dtype] = (n, rp, ci, va, x, y_ld, absrow, hubs, targets)
    return _HUB[dtype]


def _spmv(A, xd, dtype, phases=None):
    """y poisoned with NaN first; phases: a sequence of spmv_phases calls instead of the one SpMV"""
    import torch
    y = torch.full((A.row_end - A.row_begin,), float("nan"), dtype=_tdt(dtype), device="cuda")
    if phases is None and A.nranks == 1:
        A.dense_vector_multiply(y, xd)
    else:
        for ph in phases or (7,):
            A.spmv_phases(y, xd, None, ph)
    torch.cuda.synchronize()
    return y.cpu().numpy()


def _assert_designed_lists(A, hubs, targets):
    """the lists of the launch: hub k's has targets[k] entries, every class occurs, two long lists
    share a wave of records; returns (dst, len)"""
    st = A.stats()
    assert st["max_slots_used"] < SPACING and st["far_entries"] == 0
    dst, ln = A.fold_lists(0)
    assert dst.size == st["fold_rows"] and np.unique(dst).size == dst.size
    at = {int(d): i for i, d in enumerate(dst)}
    got = np.array([ln[at[int(h)]] if int(h) in at else 0 for h in hubs])
    assert np.array_equal(got, targets), (got, targets)
    for name, (lo, hi) in CLASSES.items():
        assert np.any((ln >= lo) & (ln <= hi)), f"no fold list of length class {name}"
    waves = np.flatnonzero(ln >= LONG) // 64
    assert np.unique(waves).size < waves.size, "no two long lists in one wave of records"
    return dst, ln


@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("block", [256, 512, 1024])
def test_halo_fold_on_designed_list_lengths(block, dtype):
    """natural order: every length class occurs in the lists the launch reads; the device-built and
    the host-built schedule hold the same lists and both are right"""
    import torch
    import cfs_spmv_amd as cfs
    n, rp, ci, va, x, y_ld, absrow, hubs, targets = _hub(dtype)
    xd = torch.from_numpy(x).cuda()
    flags = NO_REORDER | NO_CALIBRATE | NO_HYB
    D = cfs.SymMatrix(n, rp, ci, va, options=cfs.make_options(SLOTS, 0, block, flags))
    H = cfs.SymMatrix(n, rp, ci, va, options=cfs.make_options(SLOTS, 0, block, flags | cfs.FLAG_HOST_PLAN))
    d, h = D.digest(), H.digest()
    assert d["device_built"] == 1 and h["device_built"] == 0, D.plan_note()
    assert [k for k in d if k != "device_built" and d[k] != h[k]] == []
    ld, lh = _assert_designed_lists(D, hubs, targets), _assert_designed_lists(H, hubs, targets)
    assert np.array_equal(ld[0], lh[0]) and np.array_equal(ld[1], lh[1])
    for A in (D, H):
        assert A.stats()["block_threads"] == block
        assert scaled_err(_spmv(A, xd, dtype), y_ld, absrow) <= TOL[dtype]
        # the tile kernel and the fold as two calls: the same sums, the tile kernel's atomics in another order
        two = _spmv(A, xd, dtype, phases=(1, 2))
        assert scaled_err(two, y_ld, absrow) <= TOL[dtype]
        assert scaled_err(two, _spmv(A, xd, dtype, phases=(7,)).astype(np.float64), absrow) <= (1e-13 if dtype == np.float64 else 1e-6)
        A.close()


@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
def test_halo_fold_deterministic_build_is_bit_identical_on_long_lists(dtype):
    """the fixed order of the fold's additions, on lists of every class: two runs of a deterministic
    handle agree bit for bit, and TILES then FOLD as two calls equals ALL bit for bit"""
    import torch
    import cfs_spmv_amd as cfs
    n, rp, ci, va, x, y_ld, absrow, hubs, targets = _hub(dtype)
    xd = torch.from_numpy(x).cuda()
    A = cfs.SymMatrix(n, rp, ci, va, options=cfs.make_options(SLOTS, 0, 512, NO_REORDER | NO_CALIBRATE | NO_HYB | DET))
    assert A.kernel_variant()["det"] == 1
    _assert_designed_lists(A, hubs, targets)
    y1, y2 = _spmv(A, xd, dtype), _spmv(A, xd, dtype)
    assert scaled_err(y1, y_ld, absrow) <= TOL[dtype]
    assert np.array_equal(y1.view(np.uint8), y2.view(np.uint8))
    assert np.array_equal(_spmv(A, xd, dtype, phases=(1, 2)).view(np.uint8), _spmv(A, xd, dtype, phases=(7,)).view(np.uint8))
    assert np.array_equal(_spmv(A, xd, dtype, phases=(7,)).view(np.uint8), y1.view(np.uint8))
    A.close()


@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("flags", [0, HYB], ids=["clustered", "hyb"])
def test_halo_fold_parity_in_the_default_order_and_with_far_entries(flags, dtype):
    import torch
    import cfs_spmv_amd as cfs
    n, rp, ci, va, x, y_ld, absrow, _, _ = _hub(dtype)
    xd = torch.from_numpy(x).cuda()
    A = cfs.SymMatrix(n, rp, ci, va, options=cfs.make_options(SLOTS, 0, 0, NO_CALIBRATE | flags))
    if flags & HYB:
        assert A.stats()["far_entries"] > 0
    assert scaled_err(_spmv(A, xd, dtype), y_ld, absrow) <= TOL[dtype]
    A.close()


@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("nranks", [2, 4])
def test_halo_fold_over_shards_of_the_hub_matrix(nranks, dtype):
    """exchange form: the hubs belong to rank 0, the rows that reference them to the higher ranks, so
    cfs_pack_kernel sums many strip entries per remote row and rank 0's receive fold gets one entry per
    hub and source rank; and mirrored shards (no exchange) of the same matrix"""
    import torch
    import cfs_spmv_amd as cfs
    n, rp, ci, va, x, y_ld, absrow, hubs, targets = _hub(dtype)
    xd = torch.from_numpy(x).cuda()
    first = 2000  # hub_columns: the first referencing row
    rs = np.concatenate([[0], np.linspace(first - 500, n, nranks).astype(np.int64)]).astype(np.int32)
    assert hubs.max() < rs[1] <= first
    flags = NO_REORDER | NO_CALIBRATE | NO_HYB
    xopt = cfs.make_options(SLOTS, 0, 0, flags | cfs.FLAG_SHARD_EXCHANGE)
    shards = [cfs.SymMatrix(n, rp, ci, va, options=xopt, row_splits=rs, rank=r) for r in range(nranks)]
    y = exchange_spmv(shards, rs, xd, torch, prefill=float("nan"))
    assert scaled_err(y, y_ld, absrow) <= TOL[dtype]
    # what rank 0 folds in: hub k from every higher rank that holds one of its targets[k] rows
    ref_rows = [first + SPACING * np.arange(t) for t in targets]
    want = np.array([np.unique(np.searchsorted(rs, r, side="right") - 1).size for r in ref_rows])
    dst, ln = shards[0].fold_lists(1)
    at = {int(d): i for i, d in enumerate(dst)}
    assert np.array_equal(np.array([ln[at[int(h)]] for h in hubs]), want)
    assert want.max() == nranks - 1
    assert sum(int(s.stats()["remote_vals"]) for s in shards[1:]) >= int(want.sum())
    for s in shards:
        s.close()
    ym = np.zeros(n, dtype=dtype)
    for r in range(nranks):
        A = cfs.SymMatrix(n, rp, ci, va, options=cfs.make_options(SLOTS, 0, 0, flags), row_splits=rs, rank=r)
        assert A.stats()["remote_vals"] == 0
        ym[rs[r]:rs[r + 1]] = _spmv(A, xd, dtype)
        A.close()
    assert scaled_err(ym, y_ld, absrow) <= TOL[dtype]
