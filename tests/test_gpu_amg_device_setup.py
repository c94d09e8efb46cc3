"""cfs_hip_amg_create_device_*: the multigrid hierarchy built by kernels on the device, held to the host builder with
the same (locally dominant) matching, cfs_hip_amg_create_dominant_*, in EVERY BIT -- through the readers
(level_aggregates, level_matrix, coarse_inverse) and info() (n, nnz, kind, lmin, lmax), on CFS_HIP_FLAG_DETERMINISTIC
handles, whose level handles are deterministic too, so that the power method behind lmax has no run-to-run spread.
The host builder itself is held to the text of include/cfs_hip.h by tests/test_amg_dominant_abi.py.

  small matrices at passes 1, 2, 3 and coarse_max 8 and 512 (n <= coarse_max: one dense level, no matching at all);
  pairs2300 (a smoother-only last level); the chain of 200 rows on which the cap of 64 rounds is reached, on the device
  as well; rand1026 with isolated rows and stored zeros (s = 0 is no candidate);
  band600001, 2 passes: every per-row and per-entry kernel, the sorts and the run detection beyond one trip of the
  512 x 256 grid, asserted from info();
  both ways to level 0's lower triangle (a clean CSR on the device, a disturbed one through the host), told apart by
  setup_info(); apply and pcg_amg bit for bit on both hierarchies, the solve reaching its tolerance; a greedy hierarchy
  untouched by a device create on the same handle; the refusals; a create while a side stream has work in flight,
  followed at once by a solve on that stream."""
import ctypes as C
import time

import numpy as np
import pytest

from test_amg_abi import _disturbed, _iso2d, matrix
from test_amg_dominant_abi import CAP, chain
from test_gpu_amg_steps import _apply_gpu, _case, _native, _torch_first  # noqa: F401
from test_gpu_cg_steps import DET, DTYPES, _true_relres
from test_gpu_pcg_steps import _rhs

pytestmark = pytest.mark.gpu

GRID = 512 * 256
TOL = {np.float64: 1e-8, np.float32: 1e-4}


def _f(dtype):
    return "f64" if dtype == np.float64 else "f32"


def _csr(name, dtype):
    if name == "chain200":
        n, rp, ci, va = chain(200)
    elif name.startswith("iso2d"):
        n, rp, ci, va = _iso2d(13, 11)
    elif name.startswith("lap2d"):
        n, rp, ci, va = matrix(name)
    else:
        return _case(name, dtype)
    return n, rp, ci, va.astype(dtype)


def _handle(n, rp, ci, va):
    import cfs_spmv_amd as cfs
    D = cfs.SymMatrix(n, rp, ci, va, options=cfs.make_options(flags=DET))
    assert D.kernel_variant()["det"] == 1
    return D


def _bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def _assert_same_hierarchy(G1, G2, tag):
    a, b = G1.info(), G2.info()
    for k in ("levels", "passes", "degree", "coarse_max", "ratio", "n", "nnz", "kind", "lmin", "lmax"):
        assert a[k] == b[k], (tag, k, a[k], b[k])
    for l in range(a["levels"]):
        if l + 1 < a["levels"]:
            (agg1, w1), (agg2, w2) = G1.aggregates(l), G2.aggregates(l)
            assert np.array_equal(agg1, agg2), (tag, "agg", l)
            assert _bits(w1, w2), (tag, "w", l)
        if l >= 1:
            (n1, rp1, ci1, va1), (n2, rp2, ci2, va2) = G1.level_matrix(l), G2.level_matrix(l)
            assert n1 == n2 and np.array_equal(rp1, rp2) and np.array_equal(ci1, ci2), (tag, "pattern", l)
            assert _bits(va1, va2), (tag, "values", l)
    if a["kind"][-1] == 2:
        assert _bits(G1.coarse_inverse(), G2.coarse_inverse()), (tag, "inverse")
    return a


def _pair(D, rp, ci, va, **kw):
    """(the device-built hierarchy, the host-built one with the same matching)"""
    Gd = D.amg(rp, ci, va, matching="dominant", setup="device", **kw)
    Gh = D.amg(rp, ci, va, matching="dominant", setup="host", **kw)
    sd, sh = Gd.setup_info(), Gh.setup_info()
    assert (sd["matching"], sd["setup"], sh["matching"], sh["setup"]) == ("dominant", "device", "dominant", "host")
    assert sd["rounds"] == sh["rounds"], (sd["rounds"], sh["rounds"])
    assert sh["scratch_bytes"] == 0 and not any(sh["split_seconds"].values()) and not sh["lower_on_host"]
    return Gd, Gh


@DTYPES
@pytest.mark.parametrize("name", ("lap2d40x33", "lap2d40x33-scaled", "iso2d13x11", "rand63", "rand1026", "rand1", "rand2"))
def test_the_device_builds_the_hierarchy_of_the_host_bit_for_bit(name, dtype):
    n, rp, ci, va = _csr(name, dtype)
    D = _handle(n, rp, ci, va)
    for coarse_max in (8, 512):
        for passes in (1, 2, 3):
            Gd, Gh = _pair(D, rp, ci, va, passes=passes, coarse_max=coarse_max)
            inf = _assert_same_hierarchy(Gd, Gh, (name, coarse_max, passes))
            sd = Gd.setup_info()
            if n > coarse_max:  # the kernels ran: rounds were counted, scratch was held
                assert inf["levels"] >= 2 and all(1 <= r <= CAP for r in sd["rounds"][0]) and sd["scratch_bytes"] > 0, sd
                assert not sd["lower_on_host"]
            else:  # a single dense level, no matching at all
                assert inf["levels"] == 1 and inf["kind"] == [2] and sd["rounds"] == [] and sd["scratch_bytes"] == 0
            print(f"amg-device {_f(dtype)} {name} cm={coarse_max} passes={passes}: n={inf['n']} rounds={sd['rounds']}")
            Gd.close(), Gh.close()
    D.close()


@DTYPES
def test_a_smoother_only_last_level_the_cap_and_rows_without_candidates(dtype):
    # pairs2300: every pair matches in the first pass, nothing is left to match: 2300 / 1150, the coarsening stalls
    n, rp, ci, va = _csr("pairs2300", dtype)
    D = _handle(n, rp, ci, va)
    Gd, Gh = _pair(D, rp, ci, va, coarse_max=8)
    inf = _assert_same_hierarchy(Gd, Gh, "pairs2300")
    assert inf["kind"][-1] == 1 and inf["n"][:2] == [2300, 1150], inf
    Gd.close(), Gh.close(), D.close()
    # the chain whose strength grows strictly: one pair per round, the cap of 64 on the device too
    n, rp, ci, va = _csr("chain200", dtype)
    D = _handle(n, rp, ci, va)
    Gd, Gh = _pair(D, rp, ci, va, coarse_max=8, passes=1)
    inf = _assert_same_hierarchy(Gd, Gh, "chain200")
    assert Gd.setup_info()["rounds"][0] == [CAP] and inf["n"][1] == 200 - CAP, (Gd.setup_info()["rounds"], inf["n"])
    Gd.close(), Gh.close(), D.close()
    # rand1026 with 40 rows cut off from every neighbour and 150 off-diagonal entries stored as explicit zeros
    n, rp, ci, va = _csr("rand1026", dtype)
    rows = np.repeat(np.arange(n), np.diff(rp))
    rng = np.random.default_rng(11)
    alone = rng.choice(n, 40, replace=False)
    keep = (rows == ci) | ~(np.isin(rows, alone) | np.isin(ci, alone))
    rp2 = np.concatenate([[0], np.cumsum(np.bincount(rows[keep], minlength=n))]).astype(np.int32)
    ci2, va2, rows2 = ci[keep], va[keep].copy(), rows[keep]
    off = np.flatnonzero(ci2 < rows2)
    for k in rng.choice(off, 150, replace=False):  # both mirrors
        va2[k] = 0
        va2[np.flatnonzero((rows2 == ci2[k]) & (ci2 == rows2[k]))] = 0
    assert int((va2 == 0).sum()) == 300
    D = _handle(n, rp2, ci2, va2)
    Gd, Gh = _pair(D, rp2, ci2, va2, coarse_max=8)
    _assert_same_hierarchy(Gd, Gh, "rand1026 with holes")
    agg = Gd.aggregates(0)[0]
    assert np.all(np.bincount(agg)[agg[alone]] == 1)  # an isolated row is a singleton
    Gd.close(), Gh.close(), D.close()


def _solve_both(D, Gd, Gh, n, dtype, tag, csr):
    """apply and pcg_amg on the two hierarchies: identical bits, and the tolerance reached"""
    r = _rhs(n, dtype)
    (zd, okd), (zh, okh) = _apply_gpu(Gd, r), _apply_gpu(Gh, r)
    assert okd and okh and np.all(np.isfinite(zd)) and zd.any() and _bits(zd, zh), (tag, "apply")
    (ud, itd, resd), (uh, ith, resh) = (_native(D, G, r, tol=TOL[dtype], maxiter=500) for G in (Gd, Gh))
    true, slack = _true_relres(*csr, r, ud, dtype)
    print(f"amg-device {_f(dtype)} {tag}: pcg_amg {itd} iterations, relres {resd:.3e} (recomputed in long double {true:.3e})")
    assert itd == ith and resd == resh and _bits(ud, uh), (tag, "pcg_amg")
    # (as test_gpu_amg_steps.py: the recurrence stopped below tol; the recomputed residual may stand a little above it)
    assert 0 < itd < 500 and resd <= 10 * TOL[dtype] and abs(resd - true) <= slack, (tag, itd, resd, true, slack)


@DTYPES
def test_beyond_one_grid_trip_and_the_solves(dtype):
    """band600001, 2 passes: levels 0 and 1 have more than 131 072 rows, and three levels more entries than that"""
    n, rp, ci, va = _csr("band600001", dtype)
    D = _handle(n, rp, ci, va)
    t0 = time.perf_counter()
    Gd, Gh = _pair(D, rp, ci, va, passes=2, coarse_max=512)
    inf = _assert_same_hierarchy(Gd, Gh, "band600001")
    big = [l for l in range(inf["levels"] - 1) if inf["n"][l] > GRID or inf["nnz"][l] > GRID]
    assert len(big) >= 2 and inf["n"][1] > GRID, inf
    sd, ih = Gd.setup_info(), Gh.info()
    print(f"amg-device {_f(dtype)} band600001: n={inf['n']} rounds={sd['rounds']} set-up device {inf['setup_seconds']:.3f} s "
          f"(handles {inf['handles_seconds']:.3f} s; split {sd['split_seconds']}; scratch {sd['scratch_bytes']} bytes), host "
          f"{ih['setup_seconds']:.3f} s (handles {ih['handles_seconds']:.3f} s); both and the readers {time.perf_counter() - t0:.2f} s")
    assert not sd["lower_on_host"] and sd["scratch_bytes"] > 0
    _solve_both(D, Gd, Gh, n, dtype, "band600001", (n, rp, ci, va))
    Gd.close(), Gh.close(), D.close()


@DTYPES
def test_both_ways_to_the_lower_triangle_of_level_0(dtype):
    """a clean CSR is read on the device; one with entries above the diagonal changed, duplicates and shuffled rows goes
    through amg_lower on the host; setup_info() tells which; the hierarchies equal each other and the host's"""
    n, rp, ci, va = _csr("lap2d40x33-scaled", dtype)
    va64 = va.astype(np.float64)
    rp2, ci2, va2 = _disturbed(n, rp, ci, va64, seed=3)
    va2 = va2.astype(dtype)
    if dtype == np.float32:  # (v / 2 is exact in fp32 as well: the halves still sum to the entry)
        assert np.array_equal(va2.astype(np.float64) * 2, (va2 * dtype(2)).astype(np.float64))
    D = _handle(n, rp, ci, va)
    Gc, Gh = _pair(D, rp, ci, va, coarse_max=8)
    Gx = D.amg(rp2, ci2, va2, matching="dominant", setup="device", coarse_max=8)
    assert Gc.setup_info()["lower_on_host"] is False and Gx.setup_info()["lower_on_host"] is True
    assert Gx.setup_info()["setup"] == "device"
    _assert_same_hierarchy(Gc, Gh, "clean")
    _assert_same_hierarchy(Gx, Gh, "disturbed")
    _solve_both(D, Gx, Gh, n, dtype, "lap2d40x33-scaled (disturbed CSR)", (n, rp, ci, va))
    _solve_both(D, Gc, Gh, n, dtype, "lap2d40x33-scaled", (n, rp, ci, va))
    for G in (Gc, Gx, Gh):
        G.close()
    D.close()


@DTYPES
def test_a_greedy_hierarchy_is_untouched_by_a_device_create(dtype):
    n, rp, ci, va = _csr("rand1026", dtype)
    D = _handle(n, rp, ci, va)
    r = _rhs(n, dtype)
    G1 = D.amg(rp, ci, va, coarse_max=8)
    assert G1.setup_info() == dict(matching="greedy", setup="host", lower_on_host=False, rounds=[[0, 0]] * (G1.info()["levels"] - 1),
                                   split_seconds=dict(lower=0.0, matching=0.0, galerkin=0.0, download=0.0), scratch_bytes=0)
    u1, it1, res1 = _native(D, G1, r, tol=TOL[dtype], maxiter=500)
    Gd = D.amg(rp, ci, va, matching="dominant", setup="device", coarse_max=8)
    G2 = D.amg(rp, ci, va, coarse_max=8)
    _assert_same_hierarchy(G1, G2, "greedy before and after")
    assert not np.array_equal(G1.aggregates(0)[0], Gd.aggregates(0)[0])
    ud, itd, resd = _native(D, Gd, r, tol=TOL[dtype], maxiter=500)
    for G in (G1, G2):
        u, it, res = _native(D, G, r, tol=TOL[dtype], maxiter=500)
        assert it == it1 and res == res1 and _bits(u, u1)
    print(f"amg-device {_f(dtype)} rand1026 cm=8: pcg_amg greedy {it1} iterations, dominant {itd}")
    assert 0 < it1 < 500 and 0 < itd < 500 and resd <= 10 * TOL[dtype]
    for G in (G1, G2, Gd):
        G.close()
    D.close()


@DTYPES
def test_refusals(dtype):
    import cfs_spmv_amd as cfs
    from cfs_spmv_amd import _lib
    lib = _lib.load()
    n, rp, ci, va = _csr("rand1026", dtype)
    D = _handle(n, rp, ci, va)
    suf = _f(dtype)
    create = getattr(lib, "cfs_hip_amg_create_device_" + suf)
    opt = _lib.AmgOptions(0, 0, 8, 0, 0.0)

    def good():
        G = D.amg(rp, ci, va, matching="dominant", setup="device", coarse_max=8)
        assert G.info()["levels"] >= 3
        G.close()

    def raw(h, nn, values):
        out = C.c_void_p(0x7)
        rc = create(h, nn, rp.ctypes.data, ci.ctypes.data, values.ctypes.data, C.byref(opt), C.byref(out))
        assert rc != 0 and out.value is None  # *out = NULL
        return rc, lib.cfs_hip_last_error()

    rows = np.repeat(np.arange(n), np.diff(rp))
    k = int(np.flatnonzero((rows == ci) & (rows == 700))[0])
    for value in (0.0, -1.5, np.nan):
        bad = va.copy()
        bad[k] = value
        rc, msg = raw(D._h, n, bad)
        assert rc == _lib.ERR_ARG and b"positive diagonal, 1 of 1026" in msg and b"(level 0)" in msg, msg
        with pytest.raises(_lib.CfsHipError) as e:  # the words of the host's create
            D.amg(rp, ci, bad, matching="dominant", coarse_max=8)
        assert e.value.code == rc and str(e.value).endswith(msg.decode())
        good()
    S = cfs.SymMatrix(n, rp, ci, va, row_splits=np.array([0, n // 2, n], np.int32), rank=1)
    M = cfs.SymMatrix(n, rp, ci, va, ngpus=2)
    for H in (S, M):
        rc, msg = raw(H._h, n, va)
        assert rc == _lib.ERR_UNSUPPORTED, msg
        good()
    other = np.float32 if dtype == np.float64 else np.float64
    O = _handle(n, rp, ci, va.astype(other))
    rc, msg = raw(O._h, n, va)
    assert rc == _lib.ERR_ARG and b"bytes" in msg, msg
    good()
    rc, msg = raw(D._h, n - 1, va)
    assert rc == _lib.ERR_ARG and b"rows" in msg, msg
    good()
    for H in (S, M, O, D):
        H.close()


@DTYPES
def test_a_create_beside_a_side_stream_and_a_solve_on_it_at_once(dtype):
    """the right-hand side reaches its buffer on a side stream, by a copy queued behind a large matmul; the hierarchy is
    created while that is in flight and the solve follows on the side stream at once.  The bits are those of the
    host-built hierarchy solved on the default stream."""
    import torch
    n, rp, ci, va = _csr("rand1026", dtype)
    D = _handle(n, rp, ci, va)
    r = _rhs(n, dtype)
    Gh = D.amg(rp, ci, va, matching="dominant", coarse_max=8, degree=2)
    u0, it0, res0 = _native(D, Gh, r, tol=0.0, maxiter=3)
    src = torch.from_numpy(r).cuda()
    m1 = torch.ones((4096, 4096), dtype=torch.float32, device="cuda")
    side = torch.cuda.Stream()
    late, out = torch.zeros_like(src), torch.zeros_like(src)
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        m2 = m1 @ m1
        late.copy_(src, non_blocking=True)
        Gd = D.amg(rp, ci, va, matching="dominant", setup="device", coarse_max=8, degree=2)
        it, res = D.pcg_amg(out, late, Gd, tol=0.0, maxiter=3, stream=side)
    side.synchronize()
    torch.cuda.synchronize()
    assert float(m2[0, 0]) == 4096.0
    assert it == it0 == 3 and res == res0 and _bits(out.cpu().numpy(), u0)
    _assert_same_hierarchy(Gd, Gh, "side stream")
    Gd.close(), Gh.close(), D.close()
