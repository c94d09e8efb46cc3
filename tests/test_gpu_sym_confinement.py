"""Where a NaN / Inf goes in the symmetric tile path, exactly.

The contract (include/cfs_hip.h at cfs_hip_sym_spmv; rand_matrices.sym_reference states it in numpy):
y_i = d_i x_i + sum over the stored off-diagonal (i, j) of a_ij x_j, d_i = 0 where no diagonal is
stored.  Row i is non-finite iff x_i is, or a stored (i, j) / (j, i) has a non-finite x_j or a_ij.

The matrix (rand_matrices.sym_confinement_case) has one designated column in every structure whose
load the kernel clamps, pads or shares: packets, COO leftovers, split rows, sibling chains, the last
slot of a window, halo columns, far entries, off-block slots, column 0, row n - 1.  Everything else is
integer-valued (|a| <= 8, |x| <= 8, no zeros), so every finite row must EQUAL the int64 product -- in
any order of the LDS atomics -- and a contribution lost, doubled or multiplied in from a clamped lane
shows, however small.

Default mode: the non-finite rows are the reference's; every other row is exact; the class (NaN, +Inf,
-Inf) is the reference's where x_i is finite, and the reference's or NaN where x_i itself is not (a
row split into virtual rows adds 0 * x_i in every chunk after the first).  Deterministic mode: per
tile, see test_deterministic_*."""
import ctypes as C
import itertools

import numpy as np
import pytest

import rand_matrices as rm
from test_gpu_kernel_variants import GROUP_FEATURES, PLAN_KNOBS
from test_gpu_parity import exchange_spmv

pytestmark = pytest.mark.gpu

NO_REORDER, CLUSTER, NO_CALIBRATE, EXCHANGE, HYB, DET, KEEP_MAP, HOST_PLAN = 8, 16, 32, 64, 128, 1024, 2048, 4096
POISONS = (np.nan, np.inf, -np.inf)
DTYPES = [np.float64, np.float32]
_CASE = {}


def _case(dtype):
    """(n, rp, ci, special, expect, sites, va, x, exact) -- integer data in the value type"""
    if "pattern" not in _CASE:
        _CASE["pattern"] = rm.sym_confinement_case(np.random.default_rng(0))
        _CASE["pattern"] += (_CASE["pattern"][4].sites,)
        n, rp, ci = _CASE["pattern"][:3]
        va, x = rm.sym_int_values(np.random.default_rng(1), n, rp, ci)
        _CASE["data"] = (va, x, rm.sym_int_product(n, rp, ci, va, x))
    va, x, exact = _CASE["data"]
    return _CASE["pattern"] + (va.astype(dtype), x.astype(dtype), exact)


@pytest.fixture(autouse=True)
def _torch_first(monkeypatch):
    """torch brings a HIP runtime of its own: it has to initialise before libcfs_hip.so's"""
    import torch
    torch.cuda.init()
    torch.cuda.set_device(0)
    for k in PLAN_KNOBS + ("CFS_HIP_NT", "CFS_HIP_COMBINE"):
        monkeypatch.delenv(k, raising=False)
    yield


def _run(A, x):
    """y of the handle's rows, pre-filled with NaN and one element longer: that element stays NaN"""
    import torch
    rows = A.row_end - A.row_begin
    tdt = torch.float64 if A.dtype == np.float64 else torch.float32
    y = torch.full((rows + 1,), float("nan"), dtype=tdt, device="cuda")
    xd = torch.from_numpy(np.ascontiguousarray(x, A.dtype)).cuda()
    if A.nranks > 1:
        A.spmv_phases(y, xd, None, 7)
    else:
        A.dense_vector_multiply(y, xd)
    torch.cuda.synchronize()
    y = y.cpu().numpy()
    assert np.isnan(y[rows]), "the element behind the last row was written"
    return y[:rows]


def _classes(v):
    return np.where(np.isnan(v), 0, np.sign(v)).astype(np.int8)  # of non-finite rows: 0 NaN, +1 / -1 Inf


def _check(y, ref, exact, xp, r0, r1, tag, det=False):
    """the default-mode rules (det: non-finite rows of the reference read NaN, others may too) on rows
    [r0, r1); returns the rows whose own x_i is non-finite and that read NaN where the reference has Inf"""
    ref, exact, own = ref[r0:r1], exact[r0:r1], ~np.isfinite(np.asarray(xp, np.float64)[r0:r1])
    bad, want = ~np.isfinite(y), ~np.isfinite(ref)
    if det:
        assert np.all(np.isnan(y[want])), f"{tag}: rows {r0 + np.flatnonzero(want & ~np.isnan(y))[:5]} are not NaN"
        assert not np.any(np.isinf(y)), tag
    else:
        assert np.array_equal(np.flatnonzero(bad), np.flatnonzero(want)), \
            f"{tag}: non-finite without a reference to the poison: rows {r0 + np.flatnonzero(bad & ~want)[:8]}; " \
            f"finite but poisoned: rows {r0 + np.flatnonzero(want & ~bad)[:8]}"
    fin = ~bad
    wrong = np.flatnonzero(y[fin].astype(np.float64) != exact[fin])
    assert wrong.size == 0, f"{tag}: {wrong.size} finite rows differ from the integer product, first rows " \
                            f"{r0 + np.flatnonzero(fin)[wrong[:8]]}"
    if det:
        return np.zeros(0, np.int64)
    cy, cr = _classes(y[bad]), _classes(ref[bad])
    ok = (cy == cr) | (own[bad] & (cy == 0))
    assert np.all(ok), f"{tag}: class differs in rows {r0 + np.flatnonzero(bad)[~ok][:8]}"
    return r0 + np.flatnonzero(bad)[(cy != cr)]


def _group_features(A):
    from cfs_spmv_amd import _lib
    lib, ng = _lib.load(), C.c_int()
    buf = (C.c_longlong * (A.stats()["ngroups"] * GROUP_FEATURES))()
    _lib.check(lib.cfs_hip_sym_debug_group_features(A._h, buf, len(buf), C.byref(ng)))
    return np.frombuffer(buf, dtype=np.int64).reshape(ng.value, GROUP_FEATURES)


def _features(A, hyb=False):
    """what a natural-order handle holds of the things the case was built for, from its stats, its
    kernel variant and its group features ([0] tiles, [1] rows, [2] virtual rows, [7] COO leftovers,
    [8] halo slots).  "run_tile": a group of one tile with exactly 16 halo slots, no COO leftovers and
    no split row, of at least 37 rows, lies inside the hub run (every other row of the matrix has
    leftovers or other halo columns): the 16 columns up to the hub are its halo, ascending, so the hub is
    the LAST slot of its window, and -- a lonely row every 37 rows, zero-packet rows sorted last -- its
    last virtual row is a poisoned lonely row; "ragged_run_tile": such a tile whose virtual rows are no
    multiple of 64; "wide_fill": the fill loop's U x BLOCK exceeds the window, so the clamped gathers of
    the threads past the window's end carry the last slot's x"""
    f, st, kv = _group_features(A), A.stats(), A.kernel_variant()
    assert (st["far_entries"] > 0) == bool(hyb)
    run = (f[:, 0] == 1) & (f[:, 8] == 16) & (f[:, 7] == 0) & (f[:, 2] == f[:, 1]) & (f[:, 1] >= 37)
    return {"split": bool(np.any(f[:, 2] > f[:, 1])), "coo": bool(f[:, 7].sum() > 0), "halo": st["halo_slots"] > 0,
            "fold": st["fold_rows"] > 0, "run_tile": bool(run.any()), "ragged_run_tile": bool(np.any(f[run, 2] % 64 != 0)),
            "wide_fill": kv["u"] * kv["block"] > st["max_slots_used"]}


ALL_FEATURES = ("split", "coo", "halo", "fold", "run_tile", "ragged_run_tile", "wide_fill")


def _assert_features(A, tag, hyb=False, need=ALL_FEATURES):
    """before poisoning: the handle has the features the case was built for"""
    got = _features(A, hyb)
    assert all(got[k] for k in need), f"{tag}: {got}"


def _poison_rounds(A, case, tag, det=False):
    """NaN, +Inf, -Inf in every special column at once, then the clean x: nothing sticks in the handle.
    Returns the special rows that read NaN where the reference has Inf: rows the schedule split (which
    rows those are depends on the order of the rows: clustered, or with mirrored entries, the hub row
    holds its whole run as stored entries)"""
    n, rp, ci, special, expect, site, va, x, exact = case
    r0, r1 = A.row_begin, A.row_end
    deviations = set()
    for poison in POISONS + (None,):
        xp = x.copy()
        if poison is not None:
            xp[special] = poison
        if ("ref", poison) not in _CASE:  # (the same integers in both value types)
            _CASE["ref", poison] = rm.sym_reference(n, rp, ci, va, xp)
        ref = _CASE["ref", poison]
        y = _run(A, xp)
        deviations.update(int(v) for v in _check(y, ref, exact, xp, r0, r1, f"{tag} x={poison}", det))
        if poison is None:
            assert np.array_equal(y.astype(np.float64), exact[r0:r1]), f"{tag}: the clean x after the poisons is not exact"
    return deviations


@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
@pytest.mark.parametrize("block", [256, 512, 1024])
def test_natural_order_every_combine_and_nt_setting(monkeypatch, block, dtype):
    """BLOCK x value type x CFS_HIP_COMBINE = 2 | 3 x CFS_HIP_NT = 0 | 1 in natural order, windows of
    3 x BLOCK slots: the sites are where sym_confinement_case put them"""
    import cfs_spmv_amd as cfs
    case = _case(dtype)
    n, rp, ci, special, expect, site, va, x, exact = case
    seen = set()
    for comb, nt in itertools.product((1, 0), (0, 1)):
        monkeypatch.setenv("CFS_HIP_NT", str(nt))
        monkeypatch.setenv("CFS_HIP_COMBINE", "2" if comb else "3")
        A = cfs.SymMatrix(n, rp, ci, va, options=cfs.make_options(3 * block, 0, block, NO_REORDER | NO_CALIBRATE))
        kv = A.kernel_variant()
        tag = f"block {block} comb {comb} nt {nt}"
        assert (kv["block"], kv["comb"], kv["nt"], kv["det"], kv["offb"], kv["mode"]) == (block, comb, nt, 0, 0, 0), (tag, kv)
        assert kv["value_bytes"] == np.dtype(dtype).itemsize
        _assert_features(A, tag)
        seen |= _poison_rounds(A, case, tag)
        A.close()
    # natural order: the one row of 160 more entries whose own x is poisoned is the only split one
    assert seen <= {site["long_row"]}, f"NaN for Inf in rows {sorted(seen)}"
    print(f"split-row deviation (NaN for Inf at x_i of a split row) seen in rows {sorted(seen)}")


@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
@pytest.mark.parametrize("flags", [CLUSTER, NO_REORDER | HYB, CLUSTER | HYB, 0], ids=["cluster", "hyb", "cluster-hyb", "default"])
def test_clustered_order_and_far_entries(flags, dtype):
    """FORCE_CLUSTER: tiles are clusters of the graph, the own rows go through the slot table; HYB: the
    far_once column is a far entry of the row that holds it (and every far section is padded with
    column 0, itself poisoned)"""
    import cfs_spmv_amd as cfs
    case = _case(dtype)
    n, rp, ci, va = case[0], case[1], case[2], case[6]
    A = cfs.SymMatrix(n, rp, ci, va, options=cfs.make_options(flags=flags | NO_CALIBRATE))
    if flags & HYB:
        assert A.stats()["far_entries"] > 0
    if flags & NO_REORDER:
        _assert_features(A, "hyb", hyb=True)
    _poison_rounds(A, case, f"flags {flags}")
    A.close()


@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
def test_host_built_and_device_built_schedule_agree(dtype):
    """same non-finite rows, same bytes in the finite ones"""
    import cfs_spmv_amd as cfs
    case = _case(dtype)
    n, rp, ci, special, expect, site, va, x, exact = case
    for flags in (NO_REORDER, NO_REORDER | HYB):
        D = cfs.SymMatrix(n, rp, ci, va, options=cfs.make_options(1536, 0, 512, flags | NO_CALIBRATE))
        H = cfs.SymMatrix(n, rp, ci, va, options=cfs.make_options(1536, 0, 512, flags | NO_CALIBRATE | HOST_PLAN))
        d, h = D.digest(), H.digest()
        assert d["device_built"] == 1 and h["device_built"] == 0, D.plan_note()
        assert [k for k in d if k != "device_built" and d[k] != h[k]] == []
        for M in (D, H):
            _assert_features(M, f"host / device plan flags {flags}", hyb=flags & HYB)
        _poison_rounds(H, case, f"host plan flags {flags}")
        for poison in POISONS:
            xp = x.copy()
            xp[special] = poison
            yd, yh = _run(D, xp), _run(H, xp)
            fin = np.isfinite(yd)
            assert np.array_equal(fin, np.isfinite(yh))
            assert np.array_equal(yd[fin].view(np.uint8), yh[fin].view(np.uint8))
        D.close()
        H.close()


@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
@pytest.mark.parametrize("nranks", [2, 3])
def test_mirrored_shards(nranks, dtype):
    """the first-quarter columns that rows of the last quarter hold are one-sided slots of the last
    rank (x only), and the first rank computes their transposed side from its own copy of the entry"""
    import cfs_spmv_amd as cfs
    case = _case(dtype)
    n, rp, ci, va = case[0], case[1], case[2], case[6]
    rs = np.array([n * r // nranks for r in range(nranks + 1)], np.int32)
    mirror, got = 0, {k: False for k in ALL_FEATURES}
    for rank in range(nranks):
        A = cfs.SymMatrix(n, rp, ci, va, options=cfs.make_options(1536, 0, 512, NO_REORDER | NO_CALIBRATE),
                          row_splits=rs, rank=rank)
        st = A.stats()
        assert st["remote_vals"] == 0
        mirror += st["mirror_entries"]
        if rank == nranks - 1:
            assert A.kernel_variant()["offb"] == 1
        got = {k: got[k] or v for k, v in _features(A).items()}  # (a rank holds its part of the sites)
        _poison_rounds(A, case, f"mirrored rank {rank} of {nranks}")
        A.close()
    assert mirror > 0 and all(got.values()), got


@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
@pytest.mark.parametrize("nranks", [2, 3])
def test_exchange_form_shards(nranks, dtype):
    """pack, routing by the static row lists, receive fold: the `sender` row's packed contribution
    carries its poison to the first rank, and nowhere else"""
    import torch
    import cfs_spmv_amd as cfs
    n, rp, ci, special, expect, site, va, x, exact = _case(dtype)
    rs = np.array([n * r // nranks for r in range(nranks + 1)], np.int32)
    opts = cfs.make_options(1536, 0, 512, NO_REORDER | NO_CALIBRATE | EXCHANGE)
    shards = [cfs.SymMatrix(n, rp, ci, va, options=opts, row_splits=rs, rank=r) for r in range(nranks)]
    assert shards[-1].stats()["remote_vals"] > 0 and all(s.stats()["mirror_entries"] == 0 for s in shards)
    got = {k: any(_features(s)[k] for s in shards) for k in ALL_FEATURES}  # (a rank holds its part of the sites)
    assert all(got.values()), got
    for poison in POISONS + (None,):
        xp = x.copy()
        if poison is not None:
            xp[special] = poison
        y = exchange_spmv(shards, rs, torch.from_numpy(xp).cuda(), torch, prefill=float("nan"))
        _check(y, rm.sym_reference(n, rp, ci, va, xp), exact, xp, 0, n, f"exchange {nranks} x={poison}")
    for s in shards:
        s.close()


@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
def test_multi_device_handle_on_one_device(dtype):
    import cfs_spmv_amd as cfs
    from cfs_spmv_amd import _lib
    case = _case(dtype)
    n, rp, ci, va = case[0], case[1], case[2], case[6]
    A = cfs.SymMatrix(n, rp, ci, va, ngpus=2, options=cfs.make_options(flags=NO_CALIBRATE))
    for mode in (2, 0, 1):
        _lib.check(_lib.load().cfs_hip_sym_multi_set_xmode(A._h, mode))
        _poison_rounds(A, case, f"multi-device xmode {mode}")
    A.close()


def _poisoned_values(rp, ci, va, i, j, bad):
    """va with the stored (i, j) and its image (j, i) replaced (i == j: the diagonal)"""
    out = va.copy()
    for r, c in ((i, j), (j, i)):
        q = rp[r] + np.flatnonzero(ci[rp[r]:rp[r + 1]] == c)
        assert q.size == 1
        out[q[0]] = bad
    return out


def _value_sites(case):
    """(i, j) of the stored entries a test poisons: a follower of the sibling chain against the chain's
    first column; a COO leftover (the last lower entry of a row of 4 k + 1 .. 3); a diagonal"""
    n, rp, ci, special, expect, site = case[:6]
    low = lambda i: (lambda c: c[c < i])(ci[rp[i]:rp[i + 1]])
    top = next(int(r) for r in expect[site["sibling"]]  # the chain's long row: 12 lower entries, its siblings 9 and 8
               if r > 2 and (low(r).size, low(r - 1).size, low(r - 2).size) == (12, 9, 8))
    i = next(i for i in range(n // 2 + 3000, n) if low(i).size % 4 and low(i).size > 4)
    return [(top - 1, int(low(top - 1)[0])), (i, int(low(i)[-1])), (n // 2 + 5000, n // 2 + 5000)]


@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
@pytest.mark.parametrize("flags", [NO_REORDER, NO_REORDER | HYB], ids=["natural", "hyb"])
def test_non_finite_matrix_value_through_update_values(flags, dtype):
    """exactly rows i and j of a poisoned a_ij = a_ji are non-finite; the clean values sent back make
    every row exact again; diagonal() shows the poison only at a poisoned diagonal"""
    import torch
    import cfs_spmv_amd as cfs
    case = _case(dtype)
    n, rp, ci, special, expect, site, va, x, exact = case
    A = cfs.SymMatrix(n, rp, ci, va, options=cfs.make_options(1536, 0, 512, flags | NO_CALIBRATE | KEEP_MAP))
    _assert_features(A, f"value map flags {flags}", hyb=flags & HYB)
    dg = np.zeros(n, dtype)
    on = np.repeat(np.arange(n), np.diff(rp)) == ci
    dg[ci[on]] = va[on]
    for (i, j), bad in itertools.product(_value_sites(case), POISONS):
        vb = _poisoned_values(rp, ci, va, i, j, bad)
        A.update_values(vb)
        ref = rm.sym_reference(n, rp, ci, vb, x)
        assert set(np.flatnonzero(~np.isfinite(ref))) == {i, j}
        dev = _check(_run(A, x), ref, exact, x, 0, n, f"a[{i},{j}]={bad}")
        assert dev.size == 0
        d = A.diagonal()
        torch.cuda.synchronize()
        d = d.cpu().numpy()
        want = dg.copy()
        if i == j:
            want[i] = bad
        assert np.array_equal(d.view(np.uint8), want.view(np.uint8)) or \
            (i == j and np.isnan(bad) and np.isnan(d[i]) and np.array_equal(np.delete(d, i), np.delete(dg, i)))
        A.update_values(va)
        assert np.array_equal(_run(A, x).astype(np.float64), exact), f"a[{i},{j}]={bad}: the clean values do not restore y"
    A.close()


@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
@pytest.mark.parametrize("hyb", [0, HYB], ids=["sss", "hyb"])
@pytest.mark.parametrize("block", [512, 1024])
def test_deterministic_mode_turns_whole_tiles_nan_and_no_more(block, hyb, dtype):
    """per tile: a window that holds a non-finite x turns the tile's slots NaN.  One poisoned column j
    sits in the window of at most 1 + deg(j) tiles (its own and one per row that holds it) and a tile
    spreads to at most max_slots_used slots, so at most (1 + deg(j)) max_slots_used rows are
    non-finite -- far below n / 4 here.  Every row the reference calls non-finite is NaN, every finite
    row is the integer product, two runs and a second handle give the same bytes."""
    import cfs_spmv_amd as cfs
    case = _case(dtype)
    n, rp, ci, special, expect, site, va, x, exact = case
    opts = cfs.make_options(3 * block, 0, block, NO_REORDER | NO_CALIBRATE | DET | hyb)
    A, B = (cfs.SymMatrix(n, rp, ci, va, options=opts) for _ in range(2))
    kv, st = A.kernel_variant(), A.stats()
    assert (kv["det"], kv["block"]) == (1, block)
    _assert_features(A, f"det block {block}", hyb=hyb)
    for key, poison in itertools.product(("band", "sibling", "far_once", "far_node", "col0", "last"), POISONS):
        j = int(site[key])
        cap = (1 + (expect[j].size - 1)) * st["max_slots_used"]
        assert cap < n / 4
        xp = x.copy()
        xp[j] = poison
        ref = rm.sym_reference(n, rp, ci, va, xp)
        y = _run(A, xp)
        _check(y, ref, exact, xp, 0, n, f"det {key} x={poison}", det=True)
        assert np.count_nonzero(~np.isfinite(y)) <= cap, (key, poison)
        assert np.array_equal(y.view(np.uint8), _run(A, xp).view(np.uint8))
        assert np.array_equal(y.view(np.uint8), _run(B, xp).view(np.uint8))
    assert np.array_equal(_run(A, x).astype(np.float64), exact)
    A.close()
    B.close()
    # a non-finite matrix value: its rows i, j are NaN, and at most their two tiles with them
    for (i, j), bad in itertools.product(_value_sites(case), POISONS):
        vb = _poisoned_values(rp, ci, va, i, j, bad)
        M, M2 = (cfs.SymMatrix(n, rp, ci, vb, options=opts) for _ in range(2))
        y = _run(M, x)
        ref = rm.sym_reference(n, rp, ci, vb, x)
        _check(y, ref, exact, x, 0, n, f"det a[{i},{j}]={bad}", det=True)
        assert np.all(np.isnan(y[[i, j]]))
        assert np.count_nonzero(~np.isfinite(y)) <= 2 * M.stats()["max_slots_used"] < n / 4
        assert np.array_equal(y.view(np.uint8), _run(M, x).view(np.uint8))
        assert np.array_equal(y.view(np.uint8), _run(M2, x).view(np.uint8))
        M.close()
        M2.close()
