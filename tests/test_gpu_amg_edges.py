"""cfs_hip_amg_apply and cfs_hip_sym_pcg_amg where test_gpu_amg_steps.py stops, by its method and with its CPU side
(Hierarchy: the V-cycle rebuilt from what the readers return): the long-double cycle is the reference, d the deviation
of the same cycle in the working precision with the kernels' rounding rules, the GPU is allowed 4 d + 16 u, a case with
d > D_LIMIT is badly chosen and fails.  Where bits are compared they are those of a clean run of the same object on a
CFS_HIP_FLAG_DETERMINISTIC handle (and, for pairs2300 alone, on a default-mode one: the docstring of that test says why
that is sound).  No number here comes from the library under test.

1. Beyond one trip of the grid (512 x 256 = 131 072 threads): band600001, 2 passes, coarse_max 512, degree 2.  The
levels are 600001 / 150823 / 40295 / 11271 / 3292 / 1017 / 333: amg_restrict_kernel at level 0 (150 823 aggregates)
and amg_prolong_kernel at levels 0 and 1 take a second trip; the 16-byte loop of amg_restart_kernel runs over 300 000
(fp64) / 150 000 (fp32) vectors, a second trip in both, and its scalar tail has the one row 600 000 to do.  The tests
assert these shapes from info().  One hierarchy per value type, built once: the cycle, its symmetry and confinement,
and the iterates k = 1, 2 from a first guess that is not zero.

2. Every option on the device: degree 4; ratio 2 and 30; passes 1 and 3 -- with 3 passes rand1026 has aggregates of
every size 1 .. 8 at level 0, with 1 pass singletons and pairs, asserted from aggregates(0) -- the cycle applied on each.

3. Iterates k = 1, 2, 5 under a smoother-only last level (pairs2300), from u = 0 and from x0 uniform in (-1, 1); from
x0 on rand1026 and rand257 at degree 2; and a first guess that already solves the system: no iteration, u untouched.

4. Where a NaN goes and that it does not stay.  pairs2300 is block diagonal: on a default-mode handle a NaN or +Inf in
r_i reaches exactly the two rows of i's pair; on a deterministic handle, whose product turns whole tiles NaN
(include/cfs_hip.h at CFS_HIP_FLAG_DETERMINISTIC), it reaches the pair and the rest of the tiles the cycle's products
pass it through, as NaN, reproducibly.  In both every finite entry of z keeps the bits of the clean run.  With a dense
last level (rand63, rand1026; deterministic handles) the set of non-finite entries is the one the working-precision
CPU cycle predicts for the same r -- all of z: the dense level spreads it.  The work vectors and the done flag belong
to the object: the next clean apply and the next clean solve give the bits of before.

5. Two hierarchies on one handle used alternately (they share the handle's product workspace), and apply / pcg_amg on
a stream other than the default one, r and b written on that stream immediately before.

Measured on the MI355X.  z = M^-1 r: d / the GPU's deviation, then |x.My - y.Mx| / (||x|| ||My||), fp64 and fp32; the
levels as _shape gives them (m multigrid, s smoother-only, d dense):

    band600001 cm=512 m=2                   3.3e-16/4.2e-16  2.5e-19    1.6e-07/1.1e-07  5.1e-11    600001m/150823m/40295m/11271m/3292m/1017m/333d
    rand257    cm=40  m=4                   1.6e-16/1.3e-16  1.5e-18    5.7e-08/5.7e-08  3.5e-09    257m/89m/35d
    rand1026   cm=8   m=4                   1.1e-16/9.1e-17  7.3e-18    8.1e-08/6.8e-08  1.1e-09    1026m/344m/116m/42m/22m/16m/13d
    rand1026   cm=8   m=2 ratio=2           8.1e-17/9.8e-17  2.7e-18    5.8e-08/5.8e-08  1.8e-09    the same
    rand1026   cm=8   m=2 ratio=30          2.3e-16/2.7e-16  4.5e-18    1.4e-07/1.0e-07  8.5e-10    the same
    rand1026   cm=8   m=1 passes=1          9.7e-17/1.1e-16  1.8e-18    5.1e-08/5.1e-08  5.3e-09    1026m/593m/344m/197m/114m/70m/45m/31m/23m/19m/17m/15d
    rand1026   cm=8   m=3 passes=1          7.1e-17/1.7e-16  5.4e-18    8.9e-08/8.9e-08  1.5e-09    the same
    rand1026   cm=8   m=1 passes=3          6.1e-17/7.7e-17  7.1e-19    4.1e-08/5.3e-08  1.9e-09    1026m/200m/44m/19m/14d
    rand1026   cm=8   m=3 passes=3          1.3e-16/1.3e-16  1.8e-19    7.4e-08/3.9e-08  1.1e-09    the same
  aggregates of 1 .. 2^passes rows at level 0 of rand1026: 160/433 (1 pass), 63/32/97/152 (2), 35/5/13/14/26/29/42/36 (3)

  band600001: amg_create takes 0.21 s (fp64) / 0.16 s (fp32) by info()'s setup_seconds, of which the level handles
  0.08 / 0.09 s; the fixture (handle, hierarchy, readers, the CPU side's matrices) 2.3 s for the first value type,
  0.4 s for the second; the test of the cycle 0.4 s, the test of the iterates 1.1 s, in either value type.

  iterates, d_k / the GPU's deviation for k = 1, 2 (band600001) or k = 1, 2, 5:
    f64 band600001 m=2 from x0  6.5e-16/6.4e-16  7.1e-16/7.5e-16
    f32 band600001 m=2 from x0  3.0e-07/2.3e-07  3.1e-07/2.4e-07
    f64 pairs2300  m=1          1.4e-16/3.0e-16  9.6e-16/1.1e-15  4.4e-16/4.9e-16      (2300m/1150s)
    f32 pairs2300  m=1          8.4e-08/9.6e-08  9.4e-07/8.8e-07  3.1e-07/2.8e-07
    f64 pairs2300  m=1 from x0  4.4e-16/3.0e-16  1.1e-15/1.5e-15  4.1e-16/3.8e-16
    f32 pairs2300  m=1 from x0  2.9e-07/1.4e-07  6.5e-07/3.3e-07  2.6e-07/5.6e-07
    f64 pairs2300  m=2          3.5e-16/2.0e-16  5.2e-16/5.7e-16  2.6e-16/3.1e-16
    f32 pairs2300  m=2          1.2e-07/4.8e-08  3.3e-07/1.5e-07  1.9e-07/1.4e-07
    f64 pairs2300  m=2 from x0  2.4e-16/2.3e-16  6.4e-16/6.4e-16  6.0e-16/4.2e-16
    f32 pairs2300  m=2 from x0  1.9e-07/1.6e-07  2.3e-07/2.7e-07  2.6e-07/1.6e-07
    f64 rand1026   m=2 from x0  2.1e-16/1.9e-16  2.3e-16/9.1e-17  2.0e-16/1.3e-16
    f32 rand1026   m=2 from x0  1.0e-07/1.0e-07  1.0e-07/7.7e-08  1.1e-07/8.9e-08
    f64 rand257    m=2 from x0  3.2e-16/2.4e-16  3.2e-16/5.8e-16  2.3e-16/4.7e-16
    f32 rand257    m=2 from x0  2.5e-07/1.2e-07  1.1e-07/1.1e-07  1.4e-07/1.4e-07
  the first guess that solves rand1026: relres 6.0e-15 (fp64) / 4.5e-07 (fp32) in long double

  a NaN or +Inf in r[1151] of pairs2300: 2 entries of z not finite on the default-mode handle (rows 1150, 1151); on the
  deterministic handle 58 at degree 1 (rows 1150 .. 1207) and 116 at degree 2 (1150 .. 1265), all NaN, in both value
  types.  rand63 and rand1026 with a dense last level: all of z, on the GPU and in the CPU cycle.
"""
import time

import numpy as np
import pytest

from test_gpu_amg_steps import LD, _apply_gpu, _case, _check_iterates, _native, _setup, _shape, _torch_first  # noqa: F401
from test_gpu_cg_steps import DET, DTYPES, _true_relres
from test_gpu_kernel_variants import PLAN_KNOBS
from test_gpu_pcg_steps import D_LIMIT, UNIT, _deviation, _rhs

pytestmark = pytest.mark.gpu

GRID = 512 * 256  # the threads of every vector kernel of the cycle


def _f(dtype):
    return "f64" if dtype == np.float64 else "f32"


def _x0(n, dtype):
    return np.random.default_rng(n + 5).uniform(-1, 1, n).astype(dtype)


def _det(name, dtype):
    """a CFS_HIP_FLAG_DETERMINISTIC handle of the scaled matrix"""
    import cfs_spmv_amd as cfs
    n, rp, ci, va = _case(name, dtype)
    D = cfs.SymMatrix(n, rp, ci, va, options=cfs.make_options(flags=DET))
    assert D.kernel_variant()["det"] == 1
    return D


def _same(a, b):
    return a.dtype == b.dtype and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def _check_apply(name, G, H, dtype, tag):
    """z = M^-1 r against the long-double cycle, the symmetry quantity and the confinement of the apply test of
    test_gpu_amg_steps.py; returns the errors"""
    n, errors = H.levels[0].n, []
    x, y = _rhs(n, dtype), np.random.default_rng(n + 77).uniform(-1, 1, n).astype(dtype)
    ref = H.cycle(x)
    d = _deviation(H.cycle(x, dtype), ref)
    assert d <= D_LIMIT[dtype], f"{name} {tag}: d = {d:.3e}: badly conditioned case"
    (px, cx), (py, cy) = _apply_gpu(G, x), _apply_gpu(G, y)
    assert px.dtype == dtype and np.all(np.isfinite(px)) and np.all(np.isfinite(py))
    g, allowed = _deviation(px, ref), 4 * d + 16 * UNIT[dtype]
    xl, yl, pxl, pyl = (v.astype(LD) for v in (x, y, px, py))
    asym = float(abs(np.dot(xl, pyl) - np.dot(yl, pxl)) / (np.sqrt(np.dot(xl, xl)) * np.sqrt(np.dot(pyl, pyl))))
    print(f"amg-edges apply {_f(dtype)} {name} {tag} levels={_shape(H)} d={d:.3e} gpu={g:.3e} allowed={allowed:.3e} asym={asym:.3e}")
    if not (cx and cy):
        errors.append(f"{tag}: a guard word was overwritten or r changed")
    if not g <= allowed:
        errors.append(f"{tag}: deviation {g:.3e}, allowed {allowed:.3e} (d = {d:.3e})")
    if not asym <= allowed:
        errors.append(f"{tag}: |x.My - y.Mx| / (||x|| ||My||) = {asym:.3e}, allowed {allowed:.3e}")
    return errors


def _check_options(H, passes, degree, coarse_max, ratio):
    inf = H.info
    assert (inf["passes"], inf["degree"], inf["coarse_max"], inf["ratio"]) == (passes, degree, coarse_max, float(ratio)), inf
    for l in range(inf["levels"]):
        if inf["kind"][l] != 2:
            assert inf["lmax"][l] > 0 and inf["lmin"][l] == inf["lmax"][l] / float(ratio), (l, inf["lmin"][l], inf["lmax"][l])
        else:
            assert inf["lmax"][l] == 0


# ---- 1. beyond one trip of the grid ---------------------------------------------------------------------------------
@pytest.fixture(scope="module", params=[np.float64, np.float32], ids=["f64", "f32"])
def big(request):
    """(A, G, H, dtype) of band600001, one per value type for all the tests of this section: the set-up is the expensive
    part.  (A module fixture is made before the function fixtures: torch first, and no plan knobs, here as well.)"""
    import torch
    torch.cuda.init()
    torch.cuda.set_device(0)
    dtype = request.param
    with pytest.MonkeyPatch.context() as mp:
        for k in PLAN_KNOBS + ("CFS_HIP_CG_GRAPH",):
            mp.delenv(k, raising=False)
        t0 = time.perf_counter()
        A, G, H = _setup("band600001", dtype, 512, 2)
        wall = time.perf_counter() - t0
    print(f"amg-edges band600001 {_f(dtype)}: levels={_shape(H)} set-up {H.info['setup_seconds']:.3f} s by info(), of which the level "
          f"handles {H.info['handles_seconds']:.3f} s; handle, hierarchy and readers {wall:.3f} s")
    yield A, G, H, dtype
    G.close()
    A.close()


def _assert_second_trips(H, dtype):
    """the shape that makes the tests of this section mean something"""
    inf, W = H.info, 16 // np.dtype(dtype).itemsize
    _check_options(H, 2, 2, 512, 4.0)
    assert inf["n"][0] == 600001 and tuple(inf["kind"][:2]) == (0, 0) and inf["kind"][-1] == 2
    assert inf["n"][1] > GRID  # the restriction at level 0, the prolongation at levels 0 and 1
    assert inf["n"][0] // W > GRID  # the 16-byte loop of the restart kernel
    assert inf["n"][0] % W == 1  # ... and its scalar tail exists


def test_beyond_one_grid_trip_the_cycle(big):
    A, G, H, dtype = big
    _assert_second_trips(H, dtype)
    t0 = time.perf_counter()
    errors = _check_apply("band600001", G, H, dtype, "cm=512 m=2")
    print(f"amg-edges band600001 {_f(dtype)} the cycle: {time.perf_counter() - t0:.2f} s")
    assert not errors, f"band600001 {_f(dtype)}: " + "; ".join(errors)


def test_beyond_one_grid_trip_iterates_from_a_first_guess(big):
    """u_1, u_2 (tol = 0) from x0 uniform in (-1, 1) against the long-double recurrence from the same x0"""
    A, G, H, dtype = big
    _assert_second_trips(H, dtype)
    t0 = time.perf_counter()
    n = H.levels[0].n
    b, x0 = _rhs(n, dtype), _x0(n, dtype)
    errors = _check_iterates("band600001", H, b, dtype, lambda k: _native(A, G, b, x0=x0, tol=0.0, maxiter=k)[:2], label=" (x0)",
                             ks=(1, 2), x0=x0)
    print(f"amg-edges band600001 {_f(dtype)} the iterates: {time.perf_counter() - t0:.2f} s")
    assert not errors, f"band600001 {_f(dtype)}: " + "; ".join(errors)


# ---- 2. every option on the device -----------------------------------------------------------------------------------
OPTION_CASES = [("rand257", 40, dict(degree=4)), ("rand1026", 8, dict(degree=4)),
                ("rand1026", 8, dict(degree=2, ratio=2.0)), ("rand1026", 8, dict(degree=2, ratio=30.0)),
                ("rand1026", 8, dict(degree=1, passes=1)), ("rand1026", 8, dict(degree=3, passes=1)),
                ("rand1026", 8, dict(degree=1, passes=3)), ("rand1026", 8, dict(degree=3, passes=3))]


@DTYPES
@pytest.mark.parametrize("name,coarse_max,kw", OPTION_CASES,
                         ids=[f"{n}-cm{c}-" + "-".join(f"{k}{v:g}" for k, v in kw.items()) for n, c, kw in OPTION_CASES])
def test_every_option_on_the_device(name, coarse_max, kw, dtype):
    """degree 4, ratio 2 and 30, passes 1 and 3: the options as info() reports them, lmin = lmax / ratio on every level
    that smooths, the aggregate sizes the case is there for, and the cycle against the long-double one"""
    kw = dict(kw)
    degree, passes, ratio = kw.pop("degree"), kw.get("passes", 2), kw.get("ratio", 4.0)
    A, G, H = _setup(name, dtype, coarse_max, degree, **kw)
    _check_options(H, passes, degree, coarse_max, ratio)
    assert H.info["levels"] >= 3 and H.info["kind"][-1] == 2
    sizes = np.bincount(np.bincount(G.aggregates(0)[0]), minlength=2 ** passes + 1)[1:]
    print(f"amg-edges {name} passes={passes}: aggregates of 1 .. {2 ** passes} rows at level 0: " + "/".join(str(int(s)) for s in sizes))
    assert len(sizes) == 2 ** passes and int(sizes.sum()) == H.info["n"][1]
    if "passes" in kw:  # the member loop of the restriction at both ends: one member, and as many as there can be
        assert sizes[0] > 0 and sizes[-1] > 0, sizes
    errors = _check_apply(name, G, H, dtype, f"cm={coarse_max} m={degree} passes={passes} ratio={ratio:g}")
    G.close()
    A.close()
    assert not errors, f"{name} {_f(dtype)}: " + "; ".join(errors)


# ---- 3. iterates where they have not been -----------------------------------------------------------------------------
ITERATE_CASES = [("pairs2300", 8, 1, False), ("pairs2300", 8, 1, True), ("pairs2300", 8, 2, False), ("pairs2300", 8, 2, True),
                 ("rand1026", 8, 2, True), ("rand257", 40, 2, True)]


@DTYPES
@pytest.mark.parametrize("name,coarse_max,degree,guess", ITERATE_CASES,
                         ids=[f"{n}-cm{c}-m{m}-{'x0' if g else 'zero'}" for n, c, m, g in ITERATE_CASES])
def test_iterates_under_a_smoother_only_level_and_from_a_first_guess(name, coarse_max, degree, guess, dtype):
    """u_k, k = 1, 2, 5 (tol = 0, maxiter = k) against the long-double recurrence from the same first guess"""
    A, G, H = _setup(name, dtype, coarse_max, degree)
    assert tuple(H.info["kind"]) == (0, 1) if name == "pairs2300" else H.info["kind"][-1] == 2, H.info["kind"]
    n = H.levels[0].n
    b, x0 = _rhs(n, dtype), _x0(n, dtype) if guess else None
    errors = _check_iterates(name, H, b, dtype, lambda k: _native(A, G, b, x0=x0, tol=0.0, maxiter=k)[:2],
                             label=" (x0)" if guess else "", ks=(1, 2, 5), x0=x0)
    G.close()
    A.close()
    assert not errors, f"{name} {_f(dtype)}: " + "; ".join(errors)


@DTYPES
def test_a_first_guess_that_solves_the_system(dtype):
    """x0 = scipy's fp64 solution rounded to the value type, tol 1e-6 (fp64) / 1e-2 (fp32): its residual in long double
    is below tol, so the solve does no iteration and leaves every byte of u as it was"""
    import scipy.sparse as sp
    import torch
    from scipy.sparse.linalg import spsolve
    n, rp, ci, va = _case("rand1026", dtype)
    b = _rhs(n, dtype)
    tol = 1e-6 if dtype == np.float64 else 1e-2
    x0 = spsolve(sp.csc_matrix(sp.csr_matrix((va.astype(np.float64), ci, rp), shape=(n, n))), b.astype(np.float64)).astype(dtype)
    true, slack = _true_relres(n, rp, ci, va, b, x0, dtype)
    print(f"amg-edges solved first guess {_f(dtype)}: relres {true:.3e} in long double, tol {tol:g}")
    assert true + slack < tol, f"relres {true:.3e} (+ {slack:.3e}) of the first guess is not below {tol}: badly chosen case"
    A, G, H = _setup("rand1026", dtype, 8, 2)
    u = torch.from_numpy(x0).cuda()
    it, res = A.pcg_amg(u, torch.from_numpy(b).cuda(), G, tol=tol, maxiter=50)
    torch.cuda.synchronize()
    got = u.cpu().numpy()
    G.close()
    A.close()
    assert it == 0 and _same(got, x0), it
    assert abs(res - true) <= slack, (res, true, slack)


# ---- 4. where a NaN goes, and that it does not stay -------------------------------------------------------------------
def _clean_runs(D, G, r):
    """(z, (u, it, relres) of five iterations) of a clean right-hand side"""
    z, ok = _apply_gpu(G, r)
    assert ok and np.all(np.isfinite(z))
    u, it, res = _native(D, G, r, tol=0.0, maxiter=5)
    assert it == 5 and np.all(np.isfinite(u)) and np.isfinite(res)
    return z, (u, it, res)


def _check_nothing_stays(D, G, r, z, solve, tag):
    """after a poisoned apply: the clean apply gives the bits of before;  then a solve whose b holds a NaN ends at once
    with relres NaN, and the clean solve gives the bits and the relres of before"""
    z2, ok = _apply_gpu(G, r)
    assert ok and _same(z2, z), f"{tag}: the clean apply after a poisoned one differs from the one before"
    bad = r.copy()
    bad[len(r) // 2] = np.nan
    _, it, res = _native(D, G, bad, tol=1e-8, maxiter=300)
    assert it <= 1 and np.isnan(res), (tag, it, res)
    u, it, res = _native(D, G, r, tol=0.0, maxiter=5)
    assert it == solve[1] and res == solve[2] and _same(u, solve[0]), f"{tag}: the clean solve after a poisoned one differs"
    z3, ok = _apply_gpu(G, r)
    assert ok and _same(z3, z), f"{tag}: the clean apply after a poisoned solve differs"


@DTYPES
@pytest.mark.parametrize("degree", (1, 2))
@pytest.mark.parametrize("mode", ("default", "det"))
def test_a_nan_stays_inside_its_pair(mode, degree, dtype):
    """pairs2300, coarse_max 8 (a diagonal smoother-only level of 1150 rows): NaN, then +Inf, in r_i.
    On a handle of the default mode, whose product makes a row non-finite if and only if the contract at
    cfs_hip_sym_spmv says so, the entries of z that are not finite are EXACTLY the two rows of i's pair.  (Bits can be
    compared on this handle as well: every row of this matrix, and of its diagonal coarse level, is a sum of at most
    two terms, which has the same bits in either order; everything else in the cycle and the solve has a fixed order.)
    On a CFS_HIP_FLAG_DETERMINISTIC handle the product turns whole TILES NaN (include/cfs_hip.h at the flag: every
    slot of a tile whose window holds a non-finite x), so the cycle's NaN reach beyond the pair by design -- measured:
    58 rows at degree 1, 116 at degree 2, in both value types -- and what holds is: the pair is NaN, nothing is +-Inf,
    the pattern repeats bit for bit, it stays below n / 4 (the bound test_gpu_sym_confinement.py uses).
    In both modes every finite entry has the bits of the clean run on the same hierarchy."""
    import cfs_spmv_amd as cfs
    n, rp, ci, va = _case("pairs2300", dtype)
    D = _det("pairs2300", dtype) if mode == "det" else cfs.SymMatrix(n, rp, ci, va)
    assert D.kernel_variant()["det"] == (1 if mode == "det" else 0)
    _, G, H = _setup("pairs2300", dtype, 8, degree, D)
    assert tuple(H.info["kind"]) == (0, 1) and tuple(H.info["n"]) == (2300, 1150)
    agg = G.aggregates(0)[0]
    assert np.array_equal(agg, np.arange(2300) // 2)  # (the aggregates are the pairs)
    r = _rhs(2300, dtype)
    z, solve = _clean_runs(D, G, r)
    i = 2300 // 2 + 1
    for poison in (np.nan, np.inf):
        bad = r.copy()
        bad[i] = poison
        zb, ok = _apply_gpu(G, bad)
        assert ok
        where = np.flatnonzero(~np.isfinite(zb))
        print(f"amg-edges nan {_f(dtype)} pairs2300 {mode} m={degree} r[{i}]={poison}: {len(where)} entries of z are not finite, "
              f"rows {where.min()} .. {where.max()}")
        if mode == "default":
            assert where.tolist() == [i - 1, i], (poison, where[:10], len(where))
        else:
            assert {i - 1, i} <= set(where.tolist()) and len(where) < 2300 // 4 and np.all(np.isnan(zb[where])), (poison, where[:10])
            assert _same(_apply_gpu(G, bad)[0], zb), "the NaN pattern of a deterministic handle does not repeat"
        keep = np.ones(2300, bool)
        keep[where] = False
        assert _same(zb[keep], z[keep]), f"{poison} in r[{i}] changed the bits of finite entries"
        _check_nothing_stays(D, G, r, z, solve, f"pairs2300 {mode} m={degree} {poison}")
    G.close()
    D.close()


@DTYPES
@pytest.mark.parametrize("name,coarse_max", [("rand63", 1), ("rand1026", 8)])
def test_a_nan_goes_where_the_cpu_cycle_says(name, coarse_max, dtype):
    """a dense last level: the set of entries of z that are not finite is the one the working-precision CPU cycle gives
    for the same r (the sets, not the kinds); what is finite obeys the usual bound"""
    D = _det(name, dtype)
    _, G, H = _setup(name, dtype, coarse_max, 2, D)
    assert H.info["kind"][-1] == 2 and H.info["levels"] >= 3
    n = H.levels[0].n
    r = _rhs(n, dtype)
    z, solve = _clean_runs(D, G, r)
    bad = r.copy()
    bad[n // 2] = np.nan
    with np.errstate(all="ignore"):
        work, ref = H.cycle(bad, dtype), H.cycle(bad)
    zb, ok = _apply_gpu(G, bad)
    assert ok
    want, got = ~np.isfinite(work), ~np.isfinite(zb)
    print(f"amg-edges nan {_f(dtype)} {name} levels={_shape(H)}: {int(got.sum())} of {n} entries of z are not finite, the CPU cycle "
          f"says {int(want.sum())}")
    assert want.any() and np.array_equal(got, want), (np.flatnonzero(got != want)[:10], int(got.sum()), int(want.sum()))
    if not got.all():
        fin = ~got
        assert np.all(np.isfinite(ref[fin]))
        d = _deviation(work[fin], ref[fin])
        assert d <= D_LIMIT[dtype]
        g, allowed = _deviation(zb[fin], ref[fin]), 4 * d + 16 * UNIT[dtype]
        assert g <= allowed, (g, allowed, d)
    _check_nothing_stays(D, G, r, z, solve, name)
    G.close()
    D.close()


# ---- 5. a shared handle, another stream --------------------------------------------------------------------------------
def _spmv(D, x):
    import torch
    y = torch.full_like(x, float("nan"))
    D.dense_vector_multiply(y, x)
    torch.cuda.synchronize()
    return y.cpu().numpy()


@DTYPES
def test_two_hierarchies_on_one_handle_used_alternately(dtype):
    """degree 1 with coarse_max 8 and degree 3 with coarse_max 512 on one deterministic handle of rand1026, which lends
    both the workspace of its products: apply of each, a 3-iteration solve with each, the handle's own SpMV, and once
    more in the other order -- every result has the bits it had when its hierarchy was the only one"""
    import torch
    D = _det("rand1026", dtype)
    n, rp, ci, va = _case("rand1026", dtype)
    r = _rhs(n, dtype)
    x = torch.from_numpy(r).cuda()
    configs = (dict(degree=1, coarse_max=8), dict(degree=3, coarse_max=512))

    def use(G):
        z, ok = _apply_gpu(G, r)
        assert ok and np.all(np.isfinite(z))
        return z

    def solve(G):
        u, it, res = _native(D, G, r, tol=0.0, maxiter=3)
        assert it == 3 and np.all(np.isfinite(u))
        return u, res
    y0 = _spmv(D, x)
    alone = []
    for kw in configs:
        G = D.amg(rp, ci, va, **kw)
        alone.append((use(G), solve(G)))
        G.close()
    assert not _same(alone[0][0], alone[1][0])  # (two different preconditioners)
    G = [D.amg(rp, ci, va, **kw) for kw in configs]
    assert G[0].info()["levels"] > G[1].info()["levels"] >= 2
    for order in ((0, 1), (1, 0)):
        zs = {k: use(G[k]) for k in order}
        us = {k: solve(G[k]) for k in order}
        y = _spmv(D, x)
        for k in order:
            assert _same(zs[k], alone[k][0]), f"hierarchy {k}: z differs from the run alone"
            assert _same(us[k][0], alone[k][1][0]) and us[k][1] == alone[k][1][1], f"hierarchy {k}: u differs from the run alone"
        assert _same(y, y0)
    for g in G:
        g.close()
    D.close()


@DTYPES
def test_apply_and_solve_on_a_side_stream(dtype):
    """apply and pcg_amg on a torch side stream; r and b reach their buffers on that same stream immediately before, by
    a copy queued behind a large matmul, and hold zeros until then.  The bits are those of the default-stream run.  A
    launch on the wrong stream is not ordered behind that copy and would read the zeros -- it is caught only with high
    probability, not with certainty: nothing forbids the device to finish the matmul and the copy first."""
    import torch
    D = _det("rand1026", dtype)
    n, rp, ci, va = _case("rand1026", dtype)
    G = D.amg(rp, ci, va, degree=2, coarse_max=8)
    r = _rhs(n, dtype)
    z0, ok = _apply_gpu(G, r)
    u0, it0, res0 = _native(D, G, r, tol=0.0, maxiter=3)
    assert ok and it0 == 3 and np.all(np.isfinite(z0)) and np.all(np.isfinite(u0)) and z0.any() and u0.any()
    src = torch.from_numpy(r).cuda()
    m1 = torch.ones((4096, 4096), dtype=torch.float32, device="cuda")
    side = torch.cuda.Stream()
    for what in ("apply", "solve"):
        late = torch.zeros_like(src)
        out = torch.full_like(src, float("nan")) if what == "apply" else torch.zeros_like(src)
        torch.cuda.synchronize()
        with torch.cuda.stream(side):
            m2 = m1 @ m1
            late.copy_(src, non_blocking=True)
            if what == "apply":
                G.apply(out, late, stream=side)
            else:
                it, res = D.pcg_amg(out, late, G, tol=0.0, maxiter=3, stream=side)
        side.synchronize()
        torch.cuda.synchronize()
        assert float(m2[0, 0]) == 4096.0
        got = out.cpu().numpy()
        if what == "apply":
            assert _same(got, z0), "apply on a side stream differs from the default-stream run"
        else:
            assert it == 3 and res == res0 and _same(got, u0), "pcg_amg on a side stream differs from the default-stream run"
    G.close()
    D.close()
