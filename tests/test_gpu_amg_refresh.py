"""cfs_hip_amg_create_refreshable_* and cfs_hip_amg_update_values_* on the device: the numeric re-set-up of a multigrid
hierarchy with its aggregates kept, against references that do not involve the kernels under test.

1. Unchanged values: after update_values(values) the readers return, in every bit, what they returned before and what
   a plain cfs_hip_amg_create_* object returns; lmax agrees within the run-to-run spread of the product's LDS atomics
   (the largest relative difference of lmax over three plain creates, code this change does not touch; 8 x that with a
   floor of 64 units in the last place of the value type is allowed); apply passes _check_apply of
   test_gpu_amg_edges.py against the long-double Hierarchy rebuilt from the readers.
2. lap2d40x33 -> its scaled form against a fresh create on the scaled values: the aggregates coincide (asserted), then
   every w, level matrix and the inverse are equal in every bit; pcg_amg needs the same number of iterations give or take
   one (rounding in lmax may move the crossing of tol), and a hierarchy that was NOT refreshed needs strictly more.
   tol is 1e-8 in fp64 and, as everywhere in this suite, 1e-4 in fp32, whose unit roundoff is 6e-8.
3. Frozen aggregates: rand63 and rand1026 at 1, 2, 3 passes, every diagonal entry times 1 + uniform(0, 1): every level's
   w and matrix equal, in every bit, the chain of the frozen model of test_amg_refresh_abi.py with rounding to the value
   type between the levels; the aggregates are unchanged, those of a fresh create differ (asserted); pcg_amg converges.
4. The same through _disturbed (the hierarchy is given the disturbed CSR and array, the handle the clean ones), and in
   fp64 through disturbed3, whose three unequal parts per split entry make the order of the sum visible.
5. band600001, more than one trip of the 512 x 256 grid in every kernel of a refresh at level 0, against
   cfs.recoarsen chained level by level.
6. Refusals and the stale state;  7. A -> B -> A, two hierarchies on one handle, the handle poured after the refresh,
   a solve on a side stream.

A coarse diagonal that goes non-positive while level 0's stays positive is constructed in section 6: one coupling
inside a first-round pair is set to -10 sqrt(a_ii a_jj), the pair's coarse diagonal is then 1 + 1 - 20 < 0.

Measured on the MI355X (one run):
  lmax spread of three plain creates: 1.6e-16 on pwtk@0.05 in fp64 (10895m/2731m/690m/175m/46d) and 0 in every other case
  and in fp32 -- these products meet few atomics' reorderings -- so the floor, 64 eps = 1.4e-14 / 7.6e-06, is what is
  allowed; the refreshed lmax differed from the created one by 1.6e-16 on that case and by 0 elsewhere.
  w on the device: no bit differed from the host's 1 / sqrt(a_ii) in any case of this file.
  lap2d40x33 -> scaled, iterations refreshed / fresh create / NOT refreshed: fp64 30 / 30 / 300 (maxiter, relres 0.91),
  fp32 18 / 18 / 300 (relres 0.89).  Frozen aggregates: 6 - 8 iterations in fp64, 3 - 4 in fp32, the long-double
  residual equal to the reported one to three digits; a fresh create ends with other level sizes (rand1026, 2 passes:
  1026/344/111/44/... for the frozen 1026/344/116/42/...).
  The handle poured after the refresh (lap2d40x33 -> scaled): 30 / 30 iterations in fp64 and 18 / 18 in fp32 for handle
  first / handle last; info() shows lmax of level 0 as 2.1371 (from the handle's old values) before the solve and
  2.1154, the other order's in every digit printed, after it.
  band600001: a refresh takes 4.6 - 5.2 ms (fp64) / 4.5 - 5.1 ms (fp32) over two runs for a create of 0.25 s / 0.17 - 0.24 s;
  Galerkin kernels 0.2 - 0.3 ms, pours 0.1, dinv + power methods 1.7 - 2.0, the dense inverse of 333 rows 2.6 - 2.7; 127 MB of
  177 MB held are the capability's (fp64).
"""
import numpy as np
import pytest

from test_amg_abi import _disturbed, matrix
from test_amg_refresh_abi import bits, disturbed3, model_frozen, new_values
from test_gpu_amg_edges import GRID, _check_apply
from test_gpu_amg_steps import Hierarchy, _case, _native, _shape, _torch_first  # noqa: F401
from test_gpu_cg_steps import DET, DTYPES, _true_relres
from test_gpu_pcg_steps import _matrix, _rhs

pytestmark = pytest.mark.gpu

TOL = {np.float64: 1e-8, np.float32: 1e-4}


def _f(dtype):
    return "f64" if dtype == np.float64 else "f32"


def _handle(n, rp, ci, va, flags=0):
    import cfs_spmv_amd as cfs
    return cfs.SymMatrix(n, rp, ci, va, options=cfs.make_options(flags=cfs.FLAG_KEEP_VALUE_MAP | flags))


def _snap(G):
    """everything the readers return"""
    inf = G.info()
    s = dict(n=tuple(inf["n"]), nnz=tuple(inf["nnz"]), kind=tuple(inf["kind"]), lmax=tuple(inf["lmax"]), agg=[], w=[], mat=[], inv=None)
    for l in range(inf["levels"] - 1):
        agg, w = G.aggregates(l)
        s["agg"].append(agg), s["w"].append(w)
    for l in range(1, inf["levels"]):
        s["mat"].append(G.level_matrix(l))
    if inf["kind"][-1] == 2:
        s["inv"] = G.coarse_inverse()
    return s


def _differences(a, b):
    """where two snapshots differ in a bit (lmax apart)"""
    out = []
    if (a["n"], a["nnz"], a["kind"]) != (b["n"], b["nnz"], b["kind"]):
        return ["the shape of the hierarchy"]
    for l, (x, y) in enumerate(zip(a["agg"], b["agg"])):
        if not np.array_equal(x, y):
            out.append(f"agg of level {l}")
    for l, (x, y) in enumerate(zip(a["w"], b["w"])):
        if not bits(x, y):
            out.append(f"w of level {l}")
    for l, (x, y) in enumerate(zip(a["mat"], b["mat"])):
        if not (x[0] == y[0] and np.array_equal(x[1], y[1]) and np.array_equal(x[2], y[2])):
            out.append(f"the pattern of level {l + 1}")
        elif not bits(x[3], y[3]):
            out.append(f"the values of level {l + 1}")
    if (a["inv"] is None) != (b["inv"] is None) or (a["inv"] is not None and not bits(a["inv"], b["inv"])):
        out.append("the dense inverse")
    return out


def _rel(a, b):
    return max([abs(x - y) / max(abs(x), abs(y)) for x, y in zip(a, b) if x != 0 or y != 0] + [0.0])


def _solve(A, G, b, dtype, maxiter=300):
    return _native(A, G, b, tol=TOL[dtype], maxiter=maxiter)


# ---- 1. unchanged values ---------------------------------------------------------------------------------------
@DTYPES
@pytest.mark.parametrize("name,coarse_max,passes", [("rand1", 512, 2), ("rand2", 1, 1), ("rand2", 1, 3), ("rand63", 1, 1), ("rand63", 1, 3),
                                                    ("rand1026", 8, 2), ("pairs2300", 8, 2), ("pwtk@0.05", 64, 2)])
def test_a_refresh_with_unchanged_values_changes_no_bit(name, coarse_max, passes, dtype):
    n, rp, ci, va = _case(name, dtype)
    A = _handle(n, rp, ci, va)
    kw = dict(coarse_max=coarse_max, passes=passes)
    plain = [A.amg(rp, ci, va, **kw) for _ in range(3)]
    lmaxes = [P.info()["lmax"] for P in plain]
    spread = max(_rel(lmaxes[0], lmaxes[1]), _rel(lmaxes[0], lmaxes[2]), _rel(lmaxes[1], lmaxes[2]))
    allowed = max(8 * spread, 64 * float(np.finfo(dtype).eps))
    G = A.amg(rp, ci, va, refreshable=True, **kw)
    before, ref = _snap(G), _snap(plain[0])
    assert not _differences(before, ref), "create_refreshable differs from create: " + ", ".join(_differences(before, ref))
    assert G.refresh_info()["refreshes"] == 0 and plain[0].refresh_info()["map_bytes"] == 0
    G.update_values(va)
    after, ri = _snap(G), G.refresh_info()
    got = max(_rel(after["lmax"], ref["lmax"]), _rel(after["lmax"], before["lmax"]))
    print(f"amg-refresh same {_f(dtype)} {name} cm={coarse_max} passes={passes} levels={_shape(Hierarchy(G, n, rp, ci, va, 1))}: "
          f"lmax spread of three creates {spread:.3e}, refreshed against created {got:.3e}, allowed {allowed:.3e}; "
          f"map_bytes {ri['map_bytes']} of {G.info()['device_bytes']}, {ri['last_seconds'] * 1e3:.2f} ms")
    assert not _differences(after, before), "the refresh changed " + ", ".join(_differences(after, before))
    assert got <= allowed, (got, allowed)
    assert ri["refreshes"] == 1 and ri["last_seconds"] > 0 and 0 < ri["map_bytes"] <= G.info()["device_bytes"]
    assert G.info()["device_bytes"] > plain[0].info()["device_bytes"]
    errors = _check_apply(name, G, Hierarchy(G, n, rp, ci, va, 1), dtype, f"cm={coarse_max} passes={passes} refreshed")
    for P in plain + [G]:
        P.close()
    A.close()
    assert not errors, "; ".join(errors)


# ---- 2. scaled values against a fresh create ---------------------------------------------------------------------
@DTYPES
def test_scaled_values_against_a_fresh_create(dtype):
    """iterations refreshed / fresh create / not refreshed, measured: fp64 30 / 30 / 300 (maxiter; relres 0.91), fp32 18 / 18 /
    300 (relres 0.89)"""
    n, rp, ci, va = matrix("lap2d40x33")
    vs = matrix("lap2d40x33-scaled")[3].astype(dtype)
    va = va.astype(dtype)
    kw = dict(coarse_max=8, passes=2)
    A = _handle(n, rp, ci, va)
    G, S = A.amg(rp, ci, va, refreshable=True, **kw), A.amg(rp, ci, va, **kw)
    A.update_values(vs)
    G.update_values(vs)
    A2 = _handle(n, rp, ci, vs)
    F = A2.amg(rp, ci, vs, **kw)
    got, want = _snap(G), _snap(F)
    assert got["n"] == want["n"] and all(np.array_equal(x, y) for x, y in zip(got["agg"], want["agg"])), "badly chosen: the aggregates differ"
    assert not _differences(got, want), "the refreshed hierarchy differs from a fresh create in " + ", ".join(_differences(got, want))
    b = _rhs(n, dtype)
    (u_g, it_g, res_g), (_, it_f, res_f), (_, it_s, res_s) = _solve(A, G, b, dtype), _solve(A2, F, b, dtype), _solve(A, S, b, dtype)
    true, slack = _true_relres(n, rp, ci, vs, b, u_g, dtype)
    print(f"amg-refresh scaled {_f(dtype)} lap2d40x33 levels={got['n']}: iterations refreshed {it_g} (relres {res_g:.2e}), fresh {it_f} "
          f"({res_f:.2e}), not refreshed {it_s} ({res_s:.2e})")
    for P in (G, S, F):
        P.close()
    A.close(), A2.close()
    # (it < maxiter: the stopping rule, r.r <= tol^2 b.b on the recurrence's residual, was met; the reported residual is
    # the recomputed one, held to the long-double one.  The issue sets the iteration counts here, no residual.)
    assert 0 < it_g < 300 and 0 < it_f < 300 and abs(it_g - it_f) <= 1 and abs(res_g - true) <= slack, (it_g, it_f, res_g, true, slack)
    assert it_s > max(it_g, it_f) or not res_s <= TOL[dtype], "the case shows nothing: the old hierarchy does as well"


# ---- 3. / 4. frozen aggregates ---------------------------------------------------------------------------------
def _frozen_chain(G, n, rp, ci, va, vb, passes, dtype):
    """[(w, values of the next level) in the value type] per level with a coarser one: the frozen model chained, the
    matchings those of the model on the OLD level matrices (which must be the hierarchy's aggregates), rounding to the
    value type between the levels.  G: the hierarchy as created on va."""
    inf, out = G.info(), []
    old, new = (n, rp, ci, va), vb
    for l in range(inf["levels"] - 1):
        (agg, _, (nc, crp, cci, cva)), qs = model_frozen(old[0], old[1], old[2], old[3].astype(np.float64), passes)
        assert np.array_equal(agg, G.aggregates(l)[0]), f"level {l}: the model's matching is not the hierarchy's"
        nxt = G.level_matrix(l + 1)
        assert nxt[0] == nc and np.array_equal(nxt[1], crp) and np.array_equal(nxt[2], cci) and bits(nxt[3], cva.astype(dtype))
        (_, w, (_, _, _, cvb)), _ = model_frozen(old[0], old[1], old[2], new.astype(np.float64), passes, qs)
        out.append((w.astype(dtype), cvb.astype(dtype)))
        old, new = nxt, cvb.astype(dtype)
    return out


def _check_frozen(name, passes, dtype, disturbed):
    n, rp, ci, va = matrix(name)
    vb = new_values(n, rp, ci, va).astype(dtype)
    va = va.astype(dtype)
    if disturbed == 3:  # three unequal parts per split entry: the order of their sum shows (fp64 only: sums of fp32 are exact)
        grp, gci, (gva, gvb), (va, vb), reordered = disturbed3(n, rp, ci, [va, vb], seed=n + passes)
        assert dtype == np.float64 and reordered > n // 8 and len(gci) > len(ci)
    A = _handle(n, rp, ci, va)
    if disturbed == 3:
        pass
    elif disturbed:  # the hierarchy reads another CSR of the same matrix (and the model the clean one)
        grp, gci, gva = _disturbed(n, rp, ci, va.astype(np.float64), seed=n + passes)
        grp2, gci2, gvb = _disturbed(n, rp, ci, vb.astype(np.float64), seed=n + passes)
        assert np.array_equal(grp, grp2) and np.array_equal(gci, gci2) and len(gci) > len(ci)
        gva, gvb = gva.astype(dtype), gvb.astype(dtype)
    else:
        grp, gci, gva, gvb = rp, ci, va, vb
    G = A.amg(grp, gci, gva, refreshable=True, coarse_max=8, passes=passes)
    created = _snap(G)
    want = _frozen_chain(G, n, rp, ci, va, vb, passes, dtype)
    A.update_values(vb)
    G.update_values(gvb)
    got = _snap(G)
    assert got["n"] == created["n"] and all(np.array_equal(x, y) for x, y in zip(got["agg"], created["agg"])), "the aggregates moved"
    wrong = []
    for l, (w, cv) in enumerate(want):
        if not bits(got["w"][l], w):
            wrong.append(f"w of level {l}")
        if not bits(got["mat"][l][3], cv):
            wrong.append(f"the values of level {l + 1}")
    assert any(not bits(x[3], y[3]) for x, y in zip(got["mat"], created["mat"]))  # (the values did change)
    A2 = _handle(n, rp, ci, vb)
    F = A2.amg(rp, ci, vb, coarse_max=8, passes=passes)
    fresh = _snap(F)
    moved = fresh["n"] != got["n"] or any(not np.array_equal(x, y) for x, y in zip(fresh["agg"], got["agg"]))
    b = _rhs(n, dtype)
    u, it, res = _solve(A, G, b, dtype)
    true, slack = _true_relres(n, rp, ci, vb, b, u, dtype)
    print(f"amg-refresh frozen {_f(dtype)} {name} passes={passes}{' disturbed' if disturbed else ''} levels={got['n']} (fresh: {fresh['n']}): "
          f"{it} iterations, relres {res:.2e}, long double {true:.2e}")
    for P in (G, F):
        P.close()
    A.close(), A2.close()
    assert not wrong, "differs from the frozen model in " + ", ".join(wrong)
    assert moved, "a fresh create chooses the same aggregates: the case does not tell a refresh from a re-match"
    assert 0 < it < 300 and res <= TOL[dtype] and true <= TOL[dtype] + slack, (it, res, true, slack)


@DTYPES
@pytest.mark.parametrize("passes", (1, 2, 3))
@pytest.mark.parametrize("name", ("rand63", "rand1026"))
def test_the_refresh_is_the_frozen_model_on_every_level(name, passes, dtype):
    _check_frozen(name, passes, dtype, False)


@DTYPES
@pytest.mark.parametrize("name", ("rand63", "rand1026"))
def test_the_callers_csr_is_read_as_amg_lower_reads_it(name, dtype):
    _check_frozen(name, 2, dtype, True)


@pytest.mark.parametrize("name", ("rand63", "rand1026"))
def test_duplicates_are_summed_on_the_device_in_the_order_amg_lower_reads_them(name):
    """disturbed3 of test_amg_refresh_abi.py: the gather-sum over the caller's array adds three unequal parts in the order
    they stand in the row"""
    _check_frozen(name, 2, np.float64, 3)


# ---- 5. past one trip of the grid --------------------------------------------------------------------------------
@DTYPES
def test_past_one_trip_of_the_grid(dtype):
    import cfs_spmv_amd as cfs
    n, rp, ci, vs = _case("band600001", dtype)
    va = np.asarray(_matrix("band600001")[3]).astype(dtype)
    assert not np.array_equal(va, vs)
    A = _handle(n, rp, ci, va)
    G = A.amg(rp, ci, va, refreshable=True, coarse_max=512, passes=2)
    inf = G.info()
    # the weights (n_0), the scaling (nnz_0) and the gather-sums (nnz_0 at level 0, then those of every round: the
    # last writes nnz_1) each make more than one trip
    assert inf["n"][0] == 600001 and min(inf["n"][0], inf["nnz"][0], inf["nnz"][1]) > GRID, inf
    old = [(n, rp, ci, va)] + [G.level_matrix(l) for l in range(1, inf["levels"])]
    aggs = [G.aggregates(l)[0] for l in range(inf["levels"] - 1)]
    A.update_values(vs)
    G.update_values(vs)
    ri, new, wrong = G.refresh_info(), vs, []
    for l in range(inf["levels"] - 1):
        w, cva = cfs.recoarsen(old[l][0], old[l][1], old[l][2], old[l][3].astype(np.float64), new.astype(np.float64), 2)
        agg, gw = G.aggregates(l)
        gm = G.level_matrix(l + 1)
        if not (np.array_equal(agg, aggs[l]) and np.array_equal(gm[1], old[l + 1][1]) and np.array_equal(gm[2], old[l + 1][2])):
            wrong.append(f"the aggregates or the pattern of level {l}")
        if not bits(gw, w.astype(dtype)):
            wrong.append(f"w of level {l}")
        if not bits(gm[3], cva.astype(dtype)):
            wrong.append(f"the values of level {l + 1}")
        new = cva.astype(dtype)
    print(f"amg-refresh band600001 {_f(dtype)} levels={inf['n']}: refresh {ri['last_seconds'] * 1e3:.2f} ms ({ri['split_seconds']}), create "
          f"{inf['setup_seconds']:.3f} s, map_bytes {ri['map_bytes']} of {G.info()['device_bytes']}")
    G.close()
    A.close()
    assert not wrong, ", ".join(wrong)


# ---- 6. refusals and the stale state -----------------------------------------------------------------------------
def _raises(code, word, fn):
    from cfs_spmv_amd import _lib
    with pytest.raises(_lib.CfsHipError) as e:
        fn()
    assert e.value.code == code and word in str(e.value), (e.value.code, str(e.value))


@DTYPES
def test_refusals_and_the_stale_state(dtype):
    import torch

    import cfs_spmv_amd as cfs
    from cfs_spmv_amd import _lib
    n, rp, ci, va = matrix("rand63")
    vb = new_values(n, rp, ci, va).astype(dtype)
    va = va.astype(dtype)
    A = _handle(n, rp, ci, va)
    kw = dict(coarse_max=8, passes=1)
    P, G, G2 = A.amg(rp, ci, va, **kw), A.amg(rp, ci, va, refreshable=True, **kw), A.amg(rp, ci, va, refreshable=True, **kw)
    created = _snap(G)
    _raises(_lib.ERR_ARG, "create_refreshable", lambda: P.update_values(va))
    assert not _differences(_snap(P), created)
    _raises(_lib.ERR_ARG, "values", lambda: G.update_values(vb[:-1]))
    other = vb.astype(np.float32 if dtype == np.float64 else np.float64)
    rc = getattr(_lib.load(), "cfs_hip_amg_update_values_" + ("f32" if dtype == np.float64 else "f64"))(G._a, other.ctypes.data, other.size)
    assert rc == _lib.ERR_ARG and b"value type" in _lib.load().cfs_hip_last_error()
    assert not _differences(_snap(G), created) and G.refresh_info()["refreshes"] == 0
    D = cfs.SymMatrix(n, rp, ci, va, options=cfs.make_options(flags=DET))
    _raises(_lib.ERR_UNSUPPORTED, "deterministic", lambda: D.amg(rp, ci, va, refreshable=True, **kw))
    D.close()
    # failures inside a refresh: a zero on the diagonal of level 0; a coarse diagonal that goes negative
    rows = np.repeat(np.arange(n), np.diff(rp))
    zero = vb.copy()
    zero[int(np.flatnonzero((rows == ci) & (rows == 40))[0])] = 0.0
    agg = created["agg"][0]
    diag = {int(i): float(vb[k]) for k, (i, j) in enumerate(zip(rows, ci)) if i == j}
    k = int(np.flatnonzero((rows != ci) & (agg[rows] == agg[ci]))[0])
    i, j = int(rows[k]), int(ci[k])
    neg = vb.copy()
    neg[(rows == i) & (ci == j)] = neg[(rows == j) & (ci == i)] = -10.0 * np.sqrt(diag[i] * diag[j])
    z, r = torch.zeros(n, dtype=torch.from_numpy(va).dtype, device="cuda"), torch.from_numpy(_rhs(n, dtype)).cuda()
    for bad, word in ((zero, "positive diagonal, 1 of 63 entries are zero, negative or not finite (level 0)"), (neg, "level 1")):
        _raises(_lib.ERR_ARG, word, lambda: G.update_values(bad))
        _raises(_lib.ERR_ARG, "the last refresh failed", lambda: G.apply(z, r))
        _raises(_lib.ERR_ARG, "the last refresh failed", lambda: A.pcg_amg(z, r, G, tol=1e-4, maxiter=5))
        assert G.refresh_info()["refreshes"] == 0
    A.update_values(vb)
    G.update_values(vb)
    G2.update_values(vb)
    assert G.refresh_info()["refreshes"] == 1
    assert not _differences(_snap(G), _snap(G2)), "after a failed refresh a good one does not give the bits of a clean one"
    u, it, res = _solve(A, G, _rhs(n, dtype), dtype)
    assert 0 < it < 300 and res <= TOL[dtype], (it, res)
    for X in (P, G, G2):
        X.close()
    A.close()


# ---- 7. state -------------------------------------------------------------------------------------------------
@DTYPES
def test_there_and_back_and_two_hierarchies_on_one_handle(dtype):
    n, rp, ci, va = matrix("rand1026")
    vb = new_values(n, rp, ci, va).astype(dtype)
    va = va.astype(dtype)
    A = _handle(n, rp, ci, va)
    configs = (dict(coarse_max=8, passes=2), dict(coarse_max=512, passes=1))
    alone = []
    for kw in configs:  # each hierarchy alone: created, to B, back to A
        G = A.amg(rp, ci, va, refreshable=True, **kw)
        created = _snap(G)
        A.update_values(vb), G.update_values(vb)
        at_b = _snap(G)
        A.update_values(va), G.update_values(va)
        back = _snap(G)
        assert _differences(at_b, created) and not _differences(back, created), _differences(back, created)
        alone.append((created, at_b))
        G.close()
    G = [A.amg(rp, ci, va, refreshable=True, **kw) for kw in configs]
    A.update_values(vb)
    G[0].update_values(vb)
    assert not _differences(_snap(G[0]), alone[0][1]) and not _differences(_snap(G[1]), alone[1][0])
    G[1].update_values(vb)
    A.update_values(va)
    G[0].update_values(va)
    assert not _differences(_snap(G[0]), alone[0][0]) and not _differences(_snap(G[1]), alone[1][1])
    G[1].update_values(va)
    for k in (0, 1):
        assert not _differences(_snap(G[k]), alone[k][0]) and G[k].refresh_info()["refreshes"] == 2
        G[k].close()
    A.close()


@DTYPES
def test_the_handle_poured_after_the_refresh(dtype):
    """cfs_hip_sym_update_values_* AFTER cfs_hip_amg_update_values_*: level 0's dinv and bound, made during the refresh
    from the handle's old values, are made again by the next solve -- the iteration count is that of the other order,
    give or take one, and afterwards info() shows that order's lmax of level 0 within the floor of section 1.  info()
    itself only reports: before the solve it still shows the bound made from the old values."""
    n, rp, ci, va = matrix("lap2d40x33")
    vs = matrix("lap2d40x33-scaled")[3].astype(dtype)
    va = va.astype(dtype)
    b, counts, lmax0 = _rhs(n, dtype), [], []
    for handle_first in (True, False):
        A = _handle(n, rp, ci, va)
        G = A.amg(rp, ci, va, refreshable=True, coarse_max=8)
        if handle_first:
            A.update_values(vs)
        G.update_values(vs)
        if not handle_first:
            A.update_values(vs)
        early = G.info()["lmax"][0]
        _, it, res = _solve(A, G, b, dtype)
        counts.append(it), lmax0.append((early, G.info()["lmax"][0]))
        G.close(), A.close()
    print(f"amg-refresh order {_f(dtype)}: iterations handle first {counts[0]}, handle last {counts[1]}; lmax of level 0 "
          f"before / after the solve {lmax0}")
    assert 0 < counts[0] < 300 and 0 < counts[1] < 300 and abs(counts[0] - counts[1]) <= 1
    assert lmax0[0][0] == lmax0[0][1]  # (handle first: nothing to redo)
    assert abs(lmax0[1][1] - lmax0[0][1]) <= 64 * float(np.finfo(dtype).eps) * lmax0[0][1]


@DTYPES
def test_a_solve_on_a_side_stream_right_after_a_refresh(dtype):
    """the refresh returns when the hierarchy is complete: a solve enqueued at once on a non-blocking stream uses it --
    the iteration count of the refreshed hierarchy (that of the default-stream run, give or take one), not the larger
    one of the hierarchy as created"""
    import torch
    n, rp, ci, va = matrix("lap2d40x33")
    vs = matrix("lap2d40x33-scaled")[3].astype(dtype)
    va = va.astype(dtype)
    A = _handle(n, rp, ci, va)
    G, S = A.amg(rp, ci, va, refreshable=True, coarse_max=8), A.amg(rp, ci, va, coarse_max=8)
    b = torch.from_numpy(_rhs(n, dtype)).cuda()
    u = torch.zeros_like(b)
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    A.update_values(vs)
    G.update_values(vs)
    it, res = A.pcg_amg(u, b, G, tol=TOL[dtype], maxiter=300, stream=side)
    side.synchronize()
    _, it0, res0 = _solve(A, G, b.cpu().numpy(), dtype)
    _, it_s, res_s = _solve(A, S, b.cpu().numpy(), dtype)
    print(f"amg-refresh side stream {_f(dtype)}: {it} iterations, on the default stream {it0}, the hierarchy as created {it_s}")
    G.close(), S.close()
    A.close()
    assert 0 < it < 300 and 0 < it0 < 300 and abs(it - it0) <= 1
    assert it_s > max(it, it0) or not res_s <= TOL[dtype]
