"""per-iteration time of conjugate gradients on resident vectors: the torch-driven loop of
cfs_spmv_amd/solver.py (two host-read dot products per iteration) against cfs_hip_sym_cg (the whole
iteration behind the C ABI, no host round trip), and the same pair with the Jacobi preconditioner
(solver.pcg against cfs_hip_sym_pcg: dinv read in two kernels, 2 n s bytes more per iteration).
Fixed number of iterations (tol = 0).  The Jacobi columns are left out when the library loaded
through CFS_HIP_LIB has no cfs_hip_sym_pcg (an A/B run against an older build).  Block Jacobi on
3 x 3 node blocks (cfs_hip_sym_pcg_block) sits beside Jacobi: the native loop's time per iteration,
taken in the same run with the two interleaved, and for both the iterations down to TOL.
The mixed-precision solver (cfs_hip_sym_pcg_mixed: fp32 products, fp64 solution) sits beside the fp64 native
Jacobi PCG, on fp64 stand-ins only: time per fp32 iteration over K iterations (replacements included), and
for both the iterations, the replacements and the wall time down to MIXED_TOL.
MINRES (cfs_hip_sym_minres) sits beside the Jacobi PCG on the same SPD stand-ins, with M = |diag(A)|: the native loop's
time per iteration over K iterations against the host-driven loop (solver.minres) and against cfs_hip_sym_pcg, taken in
the same run with the two native loops interleaved.
The Chebyshev-preconditioned PCG (cfs_hip_sym_pcg_cheb) sits beside the native Jacobi PCG (and, with 3 x 3 node blocks as
the base, beside the block-Jacobi PCG): solves down to TOL at degrees 2 and 4, interleaved with the plain solver, CHEB_ROUNDS
rounds, the best wall time of each; outer iterations, products (the estimate's 16 and the two residuals included) and the
time per outer iteration.  The default bounds are estimated inside the timed call; "_bounds_given" passes the bounds of
an earlier call, as a caller with many right-hand sides would.
The multigrid-preconditioned PCG (cfs_hip_sym_pcg_amg, --only-amg) sits beside the native Jacobi PCG and the Chebyshev degree-4
PCG of the same build: solves down to TOL at smoother degrees 1 and 2 with the default hierarchy, interleaved, AMG_ROUNDS rounds,
the best wall time of each; iterations, ms per solve, and per hierarchy the levels, the device bytes and the set-up seconds (the
whole create, and of it the create path of the level handles).  The hierarchy is built once, outside the timed solves.
With --only-amg also the REFRESH of a hierarchy (cfs_hip_amg_update_values_*): a refreshable hierarchy of the default options,
its set-up seconds (the number to beat: the create path is unchanged code) and device bytes beside map_bytes, then one warm-up
refresh and REFRESH_TIMED timed ones alternating between two value arrays on the device (the second: every diagonal entry times
1 + uniform(0, 1)), the host clock around the call, which ends in a synchronise; the handle is poured first, outside the timed
call, and its pour timed by itself.  Minimum and median, the split of the fastest one (Galerkin kernels, pours, dinv + power
methods, dense inverse) and, with handle and hierarchy refreshed to the SECOND array, the iterations of a solve beside those
of a fresh create on that array.  --only-amg-refresh: that part alone, without the solves above.
--only-amg-setup: what the SET-UP of a hierarchy costs and what its matching costs in iterations -- greedy / host,
dominant / host and dominant / device (cfs_hip_amg_create_device_*), SETUP_CREATES creates each, interleaved: minimum and
median of setup_seconds, of handles_seconds and of their difference (the level handles' create path is the same code in
all three); the split and the scratch of the device set-up (cfs_hip_amg_setup_info); the levels and device_bytes; then
pcg_amg to TOL on the greedy and the dominant hierarchy, interleaved as above.
--only-amg-block: the NODE-BLOCK hierarchy (SymMatrix.amg(block=3)) beside the block-Jacobi PCG, the scalar hierarchy and the
Chebyshev degree-4 PCG on block Jacobi of the same build: solves down to TOL, interleaved, AMG_ROUNDS rounds, the best wall time
of each, both hierarchies built outside the timed solves; iterations, ms, ms per iteration of the two hierarchies (the block
kernels move bs^2 weights per node where the scalar ones move bs), their levels, device bytes and set-up seconds.  A matrix
whose n is not a multiple of 3 has no node-block hierarchy (a trailing partial node): the refusal is recorded.  Default
matrices: pwtk, ldoor, Flan_1565 and rotnode3x400x330 -- rotnodeBSxNXxNY is the rotated node Laplacian of
tests/test_amg_block_abi.py, A = H (L' (x) I) H with node frames rotated against the axes.
--only-cols: PCG on a BLOCK OF RIGHT-HAND SIDES (cfs_hip_sym_pcg_cols, cfs_hip_sym_pcg_amg_cols) beside k one-column solves of
the same build in the same process: for k = 1, 4, 16 one blocked solve down to TOL against cfs_hip_sym_pcg / _pcg_block /
_pcg_amg called once per column, with Jacobi, block Jacobi on 3 x 3 node blocks and the multigrid hierarchy at degree 1 (built
once, outside the timed part), interleaved, COLS_ROUNDS rounds, the best wall time of each; the iterations of every column, and
the launches per iteration of both forms while all k columns are active.  Default matrices: lap2d400x330, pwtk, ldoor,
Flan_1565.
usage: python tools/cg_bench.py [--only-cheb | --only-amg | --only-amg-refresh | --only-amg-setup | --only-amg-block | --only-cols]
       [matrix[:scale] | lap2dNXxNY | rotnodeBSxNXxNY ...]"""
import json, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
import cfs_spmv_amd as cfs
from cfs_spmv_amd import synth
from cfs_spmv_amd.solver import cg, cg_native, minres, minres_native, pcg, pcg_native, pcg_mixed_native
from cfs_spmv_amd.solver import pcg_cheb_native
from cfs_spmv_amd.solver import pcg_amg_native

HAVE_PCG = hasattr(cfs.load(), "cfs_hip_sym_pcg")
HAVE_BLOCK = hasattr(cfs.load(), "cfs_hip_sym_pcg_block")
HAVE_MIXED = hasattr(cfs.load(), "cfs_hip_sym_pcg_mixed")
HAVE_MINRES = hasattr(cfs.load(), "cfs_hip_sym_minres")
HAVE_CHEB = hasattr(cfs.load(), "cfs_hip_sym_pcg_cheb")
ONLY_CHEB = "--only-cheb" in sys.argv
HAVE_AMG = hasattr(cfs.load(), "cfs_hip_sym_pcg_amg")
ONLY_REFRESH = "--only-amg-refresh" in sys.argv
ONLY_AMG = "--only-amg" in sys.argv or ONLY_REFRESH
HAVE_REFRESH = hasattr(cfs.load(), "cfs_hip_amg_update_values_f64")
ONLY_SETUP = "--only-amg-setup" in sys.argv
ONLY_BLOCK = "--only-amg-block" in sys.argv
ONLY_COLS = "--only-cols" in sys.argv
COLS_K, COLS_ROUNDS = (1, 4, 16), 3
SETUP_CREATES = 3
REFRESH_TIMED = 5
AMG_DEGREES, AMG_ROUNDS = (1, 2), 3
CHEB_DEGREES, CHEB_ROUNDS = (2, 4), 3
BLOCK, TOL, MAXITER = 3, 1e-8, 5000
MIXED_TOL, MIXED_MAXITER = 1e-10, 20000


def cheb_section(A, b, res):
    """solves down to TOL: Jacobi PCG and the Chebyshev polynomial on it at CHEB_DEGREES, the same on 3 x 3 node blocks"""
    bases = [("jacobi", "jacobi")] + ([(f"block{BLOCK}", "block_jacobi")] if HAVE_BLOCK else [])
    loops = {}
    for tag, base in bases:
        loops[f"pcg_{tag}"] = (lambda base=base: pcg_native(A, b, precond=base, block=BLOCK, tol=TOL, maxiter=MAXITER, check_every=16)[1:3],
                               lambda it: it + 2)
        for m in CHEB_DEGREES:
            used = pcg_cheb_native(A, b, base=base, block=BLOCK, degree=m, tol=TOL, maxiter=1)[3]
            res[f"cheb_{tag}_bounds"] = list(used)
            loops[f"cheb{m}_{tag}"] = (lambda base=base, m=m: pcg_cheb_native(A, b, base=base, block=BLOCK, degree=m, tol=TOL,
                                                                              maxiter=MAXITER, check_every=16)[1:3],
                                       lambda it, m=m: 16 + 2 + (m - 1) + it * m)
            loops[f"cheb{m}_{tag}_bounds_given"] = (lambda base=base, m=m, used=used: pcg_cheb_native(
                A, b, base=base, block=BLOCK, degree=m, lmin=used[0], lmax=used[1], tol=TOL, maxiter=MAXITER, check_every=16)[1:3],
                lambda it, m=m: 2 + (m - 1) + it * m)
    best = {}
    for _ in range(CHEB_ROUNDS):
        for label, (fn, _) in loops.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            it, rel = fn()
            torch.cuda.synchronize()
            t = time.perf_counter() - t0
            if t < best.get(label, (float("inf"),))[0]:
                best[label] = (t, it, rel)
    res["cheb_tolerance"], res["cheb_rounds"] = TOL, CHEB_ROUNDS
    for label, (t, it, rel) in best.items():
        res[label + "_ms_to_tolerance"] = round(t * 1e3, 3)
        res[label + "_iterations"] = it
        res[label + "_products"] = loops[label][1](it)
        res[label + "_relres"] = rel
        res[label + "_us_per_outer_iteration"] = round(t / max(it, 1) * 1e6, 2)
    for tag, _ in bases:
        for m in CHEB_DEGREES:
            for suffix in ("", "_bounds_given"):
                res[f"cheb{m}_{tag}{suffix}_over_pcg_{tag}_time"] = round(best[f"cheb{m}_{tag}{suffix}"][0] / best[f"pcg_{tag}"][0], 4)


def refresh_section(A, b, res, rp, ci, va):
    """a refreshable hierarchy followed through REFRESH_TIMED + 1 value updates; A was made with FLAG_KEEP_VALUE_MAP"""
    n = A.n
    rows = np.repeat(np.arange(n), np.diff(rp))
    vb = va.copy()
    d = rows == ci
    vb[d] *= 1.0 + np.random.default_rng(7).uniform(0.0, 1.0, n)[rows[d]]
    dev = [torch.from_numpy(va).cuda(), torch.from_numpy(vb).cuda()]
    G = A.amg(rp, ci, va, refreshable=True)
    inf = G.info()
    res["refresh_levels"], res["refresh_kinds"] = inf["n"], inf["kind"]
    res["refresh_create_setup_seconds"] = round(inf["setup_seconds"], 4)
    res["refresh_create_setup_seconds_level_handles"] = round(inf["handles_seconds"], 4)
    res["refresh_device_bytes"], res["refresh_map_bytes"] = inf["device_bytes"], G.refresh_info()["map_bytes"]
    times, pours, splits = [], [], []
    for k in range(REFRESH_TIMED + 1):  # (the first one is the warm-up)
        v = dev[(k + 1) % 2]
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        A.update_values(v)
        t1 = time.perf_counter()
        G.update_values(v)
        t2 = time.perf_counter()
        if k > 0:
            pours.append(t1 - t0), times.append(t2 - t1), splits.append(G.refresh_info()["split_seconds"])
    res["refresh_ms_min"], res["refresh_ms_median"] = round(min(times) * 1e3, 3), round(float(np.median(times)) * 1e3, 3)
    res["refresh_handle_pour_ms_min"] = round(min(pours) * 1e3, 3)
    res["refresh_split_ms"] = {k: round(v * 1e3, 3) for k, v in splits[int(np.argmin(times))].items()}
    res["refresh_over_create"] = round(min(times) / inf["setup_seconds"], 5)
    # what frozen aggregates cost: handle and hierarchy on the PERTURBED array vb, against a fresh create on vb
    A.update_values(dev[1])
    G.update_values(dev[1])
    it, rel = pcg_amg_native(A, b, G, tol=TOL, maxiter=MAXITER)[1:3]
    F = A.amg(rp, ci, vb)
    res["refresh_solve_values"] = "perturbed: every diagonal entry times 1 + uniform(0, 1), default_rng(7)"
    itf, relf = pcg_amg_native(A, b, F, tol=TOL, maxiter=MAXITER)[1:3]
    res.update(refresh_solve_iterations=it, refresh_solve_relres=rel, fresh_create_solve_iterations=itf, fresh_create_solve_relres=relf,
               fresh_create_setup_seconds=round(F.info()["setup_seconds"], 4))
    F.close()
    G.close()
    A.update_values(dev[0])


def setup_section(A, b, res, rp, ci, va):
    """the three ways to a hierarchy, SETUP_CREATES creates each, interleaved; then the solves on greedy and dominant"""
    ways = {"greedy_host": dict(), "dominant_host": dict(matching="dominant"), "dominant_device": dict(matching="dominant", setup="device")}
    seen = {w: [] for w in ways}
    kept = {}
    for k in range(SETUP_CREATES):
        for w, kw in ways.items():
            G = A.amg(rp, ci, va, **kw)
            inf = G.info()
            seen[w].append((inf["setup_seconds"], inf["handles_seconds"], G.setup_info()))
            if k + 1 == SETUP_CREATES:
                kept[w] = G
                res[f"{w}_levels"], res[f"{w}_kinds"], res[f"{w}_device_bytes"] = inf["n"], inf["kind"], inf["device_bytes"]
            else:
                G.close()
    for w, runs in seen.items():
        total, handles = np.array([r[0] for r in runs]), np.array([r[1] for r in runs])
        for label, v in (("setup_seconds", total), ("handles_seconds", handles), ("setup_minus_handles_seconds", total - handles)):
            res[f"{w}_{label}_min"], res[f"{w}_{label}_median"] = round(float(v.min()), 5), round(float(np.median(v)), 5)
    best = seen["dominant_device"][int(np.argmin([r[0] for r in seen["dominant_device"]]))][2]
    res["dominant_device_split_ms"] = {k: round(v * 1e3, 3) for k, v in best["split_seconds"].items()}
    res["dominant_device_scratch_bytes"], res["dominant_device_lower_on_host"] = best["scratch_bytes"], best["lower_on_host"]
    res["dominant_rounds"] = best["rounds"]
    res["device_over_greedy_host_setup"] = round(res["dominant_device_setup_seconds_min"] / res["greedy_host_setup_seconds_min"], 4)
    res["device_over_greedy_host_setup_minus_handles"] = round(res["dominant_device_setup_minus_handles_seconds_min"] /
                                                               res["greedy_host_setup_minus_handles_seconds_min"], 4)
    loops = {w: (lambda G=kept[w]: pcg_amg_native(A, b, G, tol=TOL, maxiter=MAXITER)[1:3]) for w in ("greedy_host", "dominant_device")}
    solved = {}
    for _ in range(AMG_ROUNDS):
        for label, fn in loops.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            it, rel = fn()
            torch.cuda.synchronize()
            t = time.perf_counter() - t0
            if t < solved.get(label, (float("inf"),))[0]:
                solved[label] = (t, it, rel)
    res["amg_tolerance"], res["amg_rounds"], res["setup_creates"] = TOL, AMG_ROUNDS, SETUP_CREATES
    for label, (t, it, rel) in solved.items():
        tag = label.split("_")[0]
        res[f"{tag}_ms_to_tolerance"], res[f"{tag}_iterations"], res[f"{tag}_relres"] = round(t * 1e3, 3), it, rel
    res["dominant_over_greedy_iterations"] = round(res["dominant_iterations"] / max(res["greedy_iterations"], 1), 3)
    res["dominant_over_greedy_time"] = round(res["dominant_ms_to_tolerance"] / res["greedy_ms_to_tolerance"], 4)
    for G in kept.values():
        G.close()


def rotated_node_laplacian(bs, nx, ny, seed=11):
    """A = H (L' (x) I_bs) H, symmetrised: H_i = Q_i diag(sqrt(ev)) Q_i^T with seeded rotations Q_i, L' the anisotropic
    Laplacian below with the two mirrors of every off-diagonal entry multiplied by 1 + 0.3 u and the row sums kept"""
    import scipy.sparse as sp
    T = lambda k: sp.diags([-np.ones(k - 1), 2 * np.ones(k), -np.ones(k - 1)], [-1, 0, 1])
    L = (sp.kron(sp.identity(ny), T(nx)) + 0.37 * sp.kron(T(ny), sp.identity(nx))).tocoo()
    m = L.shape[0]
    low = L.row > L.col
    i, j, v = L.row[low], L.col[low], L.data[low]
    extra = 0.3 * np.random.default_rng(seed + 1).uniform(0, 1, len(v)) * v
    diag = L.diagonal()
    np.subtract.at(diag, i, extra)
    np.subtract.at(diag, j, extra)
    Lp = sp.csr_matrix((np.concatenate([v + extra, v + extra, diag]), (np.concatenate([i, j, np.arange(m)]), np.concatenate([j, i, np.arange(m)]))),
                       shape=(m, m))
    ev = np.array((1, 30, 900, 2700, 5000, 8100), np.float64)[:bs]
    Q = np.linalg.qr(np.random.default_rng(seed).standard_normal((m, bs, bs)))[0]
    H = sp.bsr_matrix((np.einsum("kia,a,kja->kij", Q, np.sqrt(ev), Q), np.arange(m), np.arange(m + 1)), shape=(m * bs, m * bs)).tocsr()
    A = (H @ sp.kron(Lp, sp.identity(bs), format="csr") @ H).tocsr()
    A = ((A + A.T) * 0.5).tocsr()
    A.sort_indices()
    return m * bs, A.indptr.astype(np.int32), A.indices.astype(np.int32), A.data.astype(np.float64)


def block_section(A, b, res, rp, ci, va):
    """solves down to TOL: block-Jacobi PCG, Chebyshev degree 4 on block Jacobi, the scalar and the node-block hierarchy"""
    loops = {f"pcg_block{BLOCK}": lambda: pcg_native(A, b, precond="block_jacobi", block=BLOCK, tol=TOL, maxiter=MAXITER, check_every=16)[1:3],
             f"cheb4_block{BLOCK}": lambda: pcg_cheb_native(A, b, base="block_jacobi", block=BLOCK, degree=4, tol=TOL, maxiter=MAXITER,
                                                            check_every=16)[1:3]}
    hierarchies = {}
    for tag, kw in (("amg_scalar", dict()), (f"amg_block{BLOCK}", dict(block=BLOCK))):
        try:
            hierarchies[tag] = G = A.amg(rp, ci, va, **kw)
        except cfs.CfsHipError as e:
            res[tag + "_refused"] = str(e)
            continue
        inf = G.info()
        res[tag + "_levels"], res[tag + "_kinds"], res[tag + "_device_bytes"] = inf["n"], inf["kind"], inf["device_bytes"]
        res[tag + "_setup_seconds"] = round(inf["setup_seconds"], 4)
        res[tag + "_setup_seconds_level_handles"] = round(inf["handles_seconds"], 4)
        loops[tag] = (lambda G=G: pcg_amg_native(A, b, G, tol=TOL, maxiter=MAXITER)[1:3])
    res["matrix_device_bytes"] = A.stats()["device_bytes"]
    best = {}
    for _ in range(AMG_ROUNDS):
        for label, fn in loops.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            it, rel = fn()
            torch.cuda.synchronize()
            t = time.perf_counter() - t0
            if t < best.get(label, (float("inf"),))[0]:
                best[label] = (t, it, rel)
    res["amg_tolerance"], res["amg_rounds"], res["maxiter"] = TOL, AMG_ROUNDS, MAXITER
    for label, (t, it, rel) in best.items():
        res[label + "_ms_to_tolerance"] = round(t * 1e3, 3)
        res[label + "_iterations"] = it
        res[label + "_relres"] = rel
        res[label + "_ms_per_iteration"] = round(t * 1e3 / max(it, 1), 4)
    blk = f"amg_block{BLOCK}"
    if blk in best:
        res[blk + "_over_amg_scalar_ms_per_iteration"] = round(res[blk + "_ms_per_iteration"] / res["amg_scalar_ms_per_iteration"], 4)
        for other in ("amg_scalar", f"pcg_block{BLOCK}", f"cheb4_block{BLOCK}"):
            res[f"{blk}_over_{other}_time"] = round(best[blk][0] / best[other][0], 4)
    for G in hierarchies.values():
        G.close()


def cols_section(A, res, rp, ci, va):
    """one blocked solve of k right-hand sides down to TOL against k one-column solves, for Jacobi, block Jacobi and multigrid"""
    from cfs_spmv_amd.solver import column_block
    n = A.n
    G = A.amg(rp, ci, va, degree=1)  # (outside the timed part: both forms use it)
    levels = G.info()["levels"]
    forms = {"jacobi": dict(precond="jacobi"), f"block{BLOCK}": dict(precond="block_jacobi", block=BLOCK), "amg1": dict(precond=G)}
    res["cols_tolerance"], res["cols_rounds"], res["maxiter"], res["amg1_levels"] = TOL, COLS_ROUNDS, MAXITER, G.info()["n"]
    tdt = torch.float64 if A.dtype == np.float64 else torch.float32
    for k in COLS_K:
        B, U = column_block(n, k, tdt), column_block(n, k, tdt)
        for c in range(k):
            B[:, c] = torch.from_numpy(synth.make_x(n, 11 + c).astype(A.dtype)).cuda()
        u = torch.zeros(n, dtype=tdt, device="cuda")

        def blocked(kw):
            U.zero_()
            return A.pcg_cols(U, B, tol=TOL, maxiter=MAXITER, check_every=16, **kw)

        def one_by_one(kw):
            its, rel = [], []
            for c in range(k):
                u.zero_()
                if kw["precond"] is G:
                    it, r = A.pcg_amg(u, B[:, c], G, tol=TOL, maxiter=MAXITER)
                else:
                    it, r = A.pcg(u, B[:, c], tol=TOL, maxiter=MAXITER, check_every=16, **kw)
                its.append(it), rel.append(r)
            return np.array(its), np.array(rel)
        loops = {}
        for tag, kw in forms.items():
            loops[f"{tag}_k{k}_blocked"] = lambda kw=kw: blocked(kw)
            loops[f"{tag}_k{k}_one_by_one"] = lambda kw=kw: one_by_one(kw)
        best = {}
        for _ in range(COLS_ROUNDS):
            for label, fn in loops.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                it, rel = fn()
                torch.cuda.synchronize()
                t = time.perf_counter() - t0
                if t < best.get(label, (float("inf"),))[0]:
                    best[label] = (t, it, rel)
        for label, (t, it, rel) in best.items():
            res[label + "_ms"] = round(t * 1e3, 3)
            res[label + "_iterations"] = [int(v) for v in it]
            res[label + "_max_relres"] = float(np.max(rel))
        for tag in forms:
            res[f"{tag}_k{k}_blocked_over_one_by_one_time"] = round(best[f"{tag}_k{k}_blocked"][0] / best[f"{tag}_k{k}_one_by_one"][0], 4)
            # launches per iteration while all k columns are active (a product is two launches; a level that has a coarser one
            # costs 4 vector kernels and 2 products at degree 1, the last level one kernel)
            if tag == "amg1":
                one, blk = k * (8 * levels - 1), 2 * k + 4 + 4 * (levels - 1) + 1 + 4 * k * (levels - 1)
            else:
                one, blk = 5 * k, 2 * k + 3
            res[f"{tag}_k{k}_launches_per_iteration_one_by_one"], res[f"{tag}_k{k}_launches_per_iteration_blocked"] = one, blk
            print(f"# {tag} k={k}: launches per iteration {one} one by one, {blk} blocked; "
                  f"{res[f'{tag}_k{k}_one_by_one_ms']} ms one by one, {res[f'{tag}_k{k}_blocked_ms']} ms blocked", file=sys.stderr, flush=True)
    G.close()


def amg_section(A, b, res, rp, ci, va):
    """solves down to TOL: Jacobi PCG, Chebyshev degree 4 on Jacobi, and the V-cycle at AMG_DEGREES, interleaved"""
    if ONLY_REFRESH:
        return refresh_section(A, b, res, rp, ci, va)
    loops = {"pcg_jacobi": lambda: pcg_native(A, b, precond="jacobi", tol=TOL, maxiter=MAXITER, check_every=16)[1:3],
             "cheb4_jacobi": lambda: pcg_cheb_native(A, b, degree=4, tol=TOL, maxiter=MAXITER, check_every=16)[1:3]}
    hierarchies = {}
    for m in AMG_DEGREES:
        hierarchies[m] = G = A.amg(rp, ci, va, degree=m)
        inf = G.info()
        res[f"amg{m}_levels"] = inf["n"]
        res[f"amg{m}_kinds"] = inf["kind"]
        res[f"amg{m}_device_bytes"] = inf["device_bytes"]
        res[f"amg{m}_setup_seconds"] = round(inf["setup_seconds"], 4)
        res[f"amg{m}_setup_seconds_level_handles"] = round(inf["handles_seconds"], 4)
        loops[f"amg{m}"] = (lambda G=G: pcg_amg_native(A, b, G, tol=TOL, maxiter=MAXITER)[1:3])
    res["matrix_device_bytes"] = A.stats()["device_bytes"]
    best = {}
    for _ in range(AMG_ROUNDS):
        for label, fn in loops.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            it, rel = fn()
            torch.cuda.synchronize()
            t = time.perf_counter() - t0
            if t < best.get(label, (float("inf"),))[0]:
                best[label] = (t, it, rel)
    res["amg_tolerance"], res["amg_rounds"] = TOL, AMG_ROUNDS
    for label, (t, it, rel) in best.items():
        res[label + "_ms_to_tolerance"] = round(t * 1e3, 3)
        res[label + "_iterations"] = it
        res[label + "_relres"] = rel
    for m in AMG_DEGREES:
        res[f"amg{m}_over_pcg_jacobi_time"] = round(best[f"amg{m}"][0] / best["pcg_jacobi"][0], 4)
        res[f"amg{m}_over_cheb4_jacobi_time"] = round(best[f"amg{m}"][0] / best["cheb4_jacobi"][0], 4)
        hierarchies[m].close()
    if ONLY_AMG and HAVE_REFRESH:
        refresh_section(A, b, res, rp, ci, va)


out = {}
for spec in ([a for a in sys.argv[1:] if not a.startswith("--")] or (["lap2d400x330"] if ONLY_COLS else []) + ["pwtk", "ldoor", "Flan_1565"] + (["rotnode3x400x330"] if ONLY_BLOCK else [])):
    name, _, sc = spec.partition(":")
    if name.startswith("lap2d"):  # lap2dNXxNY: the anisotropic 5-point Laplacian of the tests, a matrix that needs many iterations
        import scipy.sparse as sp
        nx, ny = (int(v) for v in name[5:].split("x"))
        T = lambda k: sp.diags([-np.ones(k - 1), 2 * np.ones(k), -np.ones(k - 1)], [-1, 0, 1])
        L = (sp.kron(sp.identity(ny), T(nx)) + 0.37 * sp.kron(T(ny), sp.identity(nx))).tocsr()
        L.sort_indices()
        n, rp, ci, va = L.shape[0], L.indptr.astype(np.int32), L.indices.astype(np.int32), L.data
    elif name.startswith("rotnode"):  # rotnodeBSxNXxNY: node frames rotated against the axes, what the node-block hierarchy is for
        n, rp, ci, va = rotated_node_laplacian(*(int(v) for v in name[7:].split("x")))
    else:
        n, rp, ci, va, _ = synth.generate(name, float(sc or 1.0))
    # (--only-amg: the refresh part pours new values into the handle)
    A = cfs.SymMatrix(n, rp, ci, va, options=cfs.make_options(flags=cfs.FLAG_KEEP_VALUE_MAP) if ONLY_AMG and HAVE_REFRESH else None)
    b = torch.from_numpy(synth.make_x(n, 11)).cuda()
    y = torch.empty_like(b)
    for _ in range(50):
        A.dense_vector_multiply(y, b)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(200):
        A.dense_vector_multiply(y, b)
    torch.cuda.synchronize()
    spmv_us = (time.perf_counter() - t0) / 200 * 1e6
    K = 200
    res = {"n": n, "spmv_us": round(spmv_us, 2)}
    if ONLY_CHEB or ONLY_AMG or ONLY_SETUP or ONLY_BLOCK or ONLY_COLS:
        if ONLY_COLS:
            cols_section(A, res, rp, ci, va)
        if ONLY_BLOCK:
            block_section(A, b, res, rp, ci, va)
        if ONLY_SETUP:
            setup_section(A, b, res, rp, ci, va)
        if ONLY_CHEB:
            cheb_section(A, b, res)
        if ONLY_AMG:
            amg_section(A, b, res, rp, ci, va)
        out[spec] = res
        A.close()
        continue
    side = torch.cuda.Stream()  # (a stream capture needs a stream of its own: CFS_HIP_CG_GRAPH=1)

    def on_side(f):
        def run():
            side.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(side):
                out = f()
            torch.cuda.current_stream().wait_stream(side)
            return out
        return run
    runs = [("torch_loop", lambda: cg(A, b, tol=0.0, maxiter=K)),
            ("native_side_stream", on_side(lambda: cg_native(A, b, tol=0.0, maxiter=K, check_every=16))),
            ("native_check8", lambda: cg_native(A, b, tol=0.0, maxiter=K, check_every=8)),
            ("native_check16", lambda: cg_native(A, b, tol=0.0, maxiter=K, check_every=16))]
    if HAVE_PCG:
        runs += [("jacobi_torch_loop", lambda: pcg(A, b, tol=0.0, maxiter=K)),
                 ("jacobi_native_check8", lambda: pcg_native(A, b, tol=0.0, maxiter=K, check_every=8)),
                 ("jacobi_native_check16", lambda: pcg_native(A, b, tol=0.0, maxiter=K, check_every=16))]
        if HAVE_BLOCK:  # interleaved with the Jacobi runs
            blk = lambda ce: (lambda: pcg_native(A, b, precond="block_jacobi", block=BLOCK, tol=0.0, maxiter=K, check_every=ce))
            runs = runs[:-2] + [runs[-2], (f"block{BLOCK}_native_check8", blk(8)), runs[-1], (f"block{BLOCK}_native_check16", blk(16))]
        # bytes of the plain iteration (B_alg + 11 n s) against the 2 n s more that dinv costs
        st, s_ = A.stats(), A.dtype.itemsize
        res["jacobi_extra_bytes_ratio"] = round(2 * n * s_ / (st["bytes_algorithmic"] + 11 * n * s_), 4)
    for label, fn in runs:
        fn()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        u, it, r = fn()
        torch.cuda.synchronize()
        res[label + "_us_per_iteration"] = round((time.perf_counter() - t0) / max(it, 1) * 1e6, 2)
        res[label + "_iterations"] = it
    if HAVE_BLOCK:  # what the preconditioners buy: iterations until ||r|| <= TOL ||b||
        res["tolerance"] = TOL
        res["jacobi_iterations_to_tolerance"] = pcg_native(A, b, tol=TOL, maxiter=MAXITER, check_every=16)[1]
        res[f"block{BLOCK}_iterations_to_tolerance"] = pcg_native(A, b, precond="block_jacobi", block=BLOCK, tol=TOL,
                                                                  maxiter=MAXITER, check_every=16)[1]
        j16, b16 = res["jacobi_native_check16_us_per_iteration"], res[f"block{BLOCK}_native_check16_us_per_iteration"]
        res[f"block{BLOCK}_over_jacobi_check16"] = round(b16 / j16 - 1.0, 4)
    if HAVE_MIXED and A.dtype == np.float64:
        A32 = cfs.SymMatrix(n, rp, ci, va.astype(np.float32))
        M = cfs.MixedSym.from_handles(A, A32)

        def timed(fn):
            fn()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            r = fn()
            torch.cuda.synchronize()
            return r, time.perf_counter() - t0
        b32 = b.float()  # the floor: the fp32 solver alone, which cannot reach MIXED_TOL
        (_, it, _), t = timed(lambda: pcg_native(A32, b32, tol=0.0, maxiter=K, check_every=16))
        res["fp32_jacobi_native_check16_us_per_iteration"] = round(t / max(it, 1) * 1e6, 2)
        (_, it, nrep, _), t = timed(lambda: pcg_mixed_native(M, b, tol=0.0, maxiter=K, check_every=16))
        res["mixed_check16_us_per_fp32_iteration"] = round(t / max(it, 1) * 1e6, 2)
        res["mixed_check16_replacements"] = nrep
        res["mixed_over_fp64_jacobi_check16"] = round(res["mixed_check16_us_per_fp32_iteration"] /
                                                      res["jacobi_native_check16_us_per_iteration"], 4)
        res["mixed_tolerance"] = MIXED_TOL
        (_, it, nrep, rel), t = timed(lambda: pcg_mixed_native(M, b, tol=MIXED_TOL, maxiter=MIXED_MAXITER, check_every=16))
        res.update(mixed_iterations_to_tolerance=it, mixed_replacements_to_tolerance=nrep, mixed_relres=rel,
                   mixed_ms_to_tolerance=round(t * 1e3, 3))
        (_, it, rel), t = timed(lambda: pcg_native(A, b, tol=MIXED_TOL, maxiter=MIXED_MAXITER, check_every=16))
        res.update(fp64_jacobi_iterations_to_tolerance=it, fp64_jacobi_relres=rel, fp64_jacobi_ms_to_tolerance=round(t * 1e3, 3))
        res["mixed_over_fp64_jacobi_time_to_tolerance"] = round(res["mixed_ms_to_tolerance"] / res["fp64_jacobi_ms_to_tolerance"], 4)
        A32.close()
    if HAVE_MINRES and HAVE_PCG:  # the two native loops interleaved, three rounds, the best of each
        def timed_iteration(fn):
            fn()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            it = fn()[1]
            torch.cuda.synchronize()
            return (time.perf_counter() - t0) / max(it, 1) * 1e6
        loops = {"minres_jacobi_native_check16": lambda: minres_native(A, b, precond="jacobi", tol=0.0, maxiter=K, check_every=16),
                 "minres_none_native_check16": lambda: minres_native(A, b, tol=0.0, maxiter=K, check_every=16),
                 "pcg_jacobi_native_check16_beside_minres": lambda: pcg_native(A, b, tol=0.0, maxiter=K, check_every=16)}
        best = {}
        for _ in range(3):
            for label, fn in loops.items():
                best[label] = min(best.get(label, float("inf")), timed_iteration(fn))
        for label, us in best.items():
            res[label + "_us_per_iteration"] = round(us, 2)
        res["minres_jacobi_torch_loop_us_per_iteration"] = round(timed_iteration(
            lambda: minres(A, b, precond="jacobi", tol=0.0, maxiter=K)), 2)
        res["minres_over_pcg_jacobi_check16"] = round(best["minres_jacobi_native_check16"] /
                                                      best["pcg_jacobi_native_check16_beside_minres"], 4)
        res["minres_native_over_torch_loop"] = round(best["minres_jacobi_native_check16"] /
                                                     res["minres_jacobi_torch_loop_us_per_iteration"], 4)
        res["minres_jacobi_iterations_to_tolerance"] = minres_native(A, b, precond="jacobi", tol=TOL, maxiter=MAXITER,
                                                                     check_every=16)[1]
    if HAVE_CHEB:
        cheb_section(A, b, res)
    if HAVE_AMG:
        amg_section(A, b, res, rp, ci, va)
    out[spec] = res
    A.close()
print(json.dumps(out))
