"""The node-block form of the multigrid set-up without a GPU (cfs_hip_amg_create_block_*, cfs_hip_amg_block,
cfs_hip_amg_level_node_weights, cfs_hip_debug_amg_coarsen_block), by the method of test_amg_abi.py and
test_amg_dominant_abi.py: the symbols are declared, exported and bound; the argument checks answer before a device is
touched; and one level, cfs.coarsen(..., block=bs), against model_coarsen_block below -- a plain numpy restatement of
the text of include/cfs_hip.h:

  W_i = D_i^-1/2 from numpy.linalg.eigh;  B = W A W;  per pass the node graph with n_ij = ||B_ij||_F and
  s_ij = n_ij / sqrt(n_ii n_jj), matched by the greedy rule (test_amg_abi._model_coarsen) or the locally dominant one
  (test_amg_dominant_abi._model), then B <- Q^T B Q with Q = Q_node (x) I.

The model's W comes from another eigen-solver, so nothing of it equals the library's in every bit: the AGGREGATES and the
coarse PATTERN must be equal exactly, and for that every choice of the matching must have a gap far above rounding.  That
is a condition on the case, asserted by the model at every round: the best and the second-best candidate strength of a
node differ by more than GAP relative, else "badly chosen case".  rotated_node_laplacian has such gaps by construction.

  W: ||W_i D_i W_i - I||_F of the library's W_i at most 4 x the largest such residual of numpy's own W_i on the same
  blocks (two correct fp64 eigen-solvers of different kinds), with a floor of 64 bs eps.
  Coarse values: against P^T A P formed in np.longdouble FROM THE LIBRARY'S OWN W and aggregates, by the rule of
  test_amg_abi.py -- an entry of k terms W_i[c, a] a_ab W_j[b, d] with S = the sum of their moduli may differ by
  (k + 4) 2^-53 S.  (The library forms (W_i A_ij) W_j: 2 bs - 2 additions and 2 roundings of a product per term of a
  fine block, then the additions of the Galerkin sums -- fewer roundings per entry than its k >= bs^2 terms.)

rotated_node_laplacian(bs, nx, ny, seed) is A = H (L' (x) I_bs) H, symmetrised: H_i = Q_i diag(sqrt(ev)) Q_i^T as in
test_gpu_block_pcg_steps.rotated_node_blocks, L' = lap2d(nx, ny) with the two mirrors of every off-diagonal entry
multiplied by 1 + 0.3 u (u seeded, uniform) and the diagonal raised by the same amounts: the row sums stay, and no two
neighbours of a node tie."""
import ctypes as C
import functools
import os
import re

import numpy as np
import pytest

import cfs_spmv_amd as cfs
from cfs_spmv_amd import _lib
from test_amg_abi import LD, U, _same_level, matrix
from test_amg_dominant_abi import CAP, _order
from test_gpu_lobpcg_steps import lap2d

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("cfs_hip_amg_create_block_f64", "cfs_hip_amg_create_block_f32", "cfs_hip_amg_block", "cfs_hip_amg_level_node_weights",
       "cfs_hip_debug_amg_coarsen_block")
BLOCKS = (2, 3, 4, 6)
GAP = 1e-6
EV = np.array((1, 30, 900, 2700, 5000, 8100), np.float64)


# ---- the test matrix ------------------------------------------------------------------------------------------
def node_roots(bs, m, seed):
    """H_i = Q_i diag(sqrt(ev)) Q_i^T, m of them: node blocks whose frames are rotated against the axes"""
    rng = np.random.default_rng(seed)
    Q = np.linalg.qr(rng.standard_normal((m, bs, bs)))[0]
    return np.einsum("kia,a,kja->kij", Q, np.sqrt(EV[:bs]), Q)


def perturbed(n, rp, ci, va, seed):
    """the symmetric matrix with the two mirrors of every off-diagonal entry multiplied by 1 + 0.3 u and the diagonal
    changed by the same amounts: the row sums stay (scipy CSR)"""
    import scipy.sparse as sp
    L = sp.csr_matrix((va, ci.copy(), rp.copy()), shape=(n, n)).tocoo()
    low = L.row > L.col
    i, j, v = L.row[low], L.col[low], L.data[low]
    extra = 0.3 * np.random.default_rng(seed).uniform(0, 1, len(v)) * v
    diag = L.diagonal()
    np.subtract.at(diag, i, extra)
    np.subtract.at(diag, j, extra)
    r = np.concatenate([i, j, np.arange(n)])
    c = np.concatenate([j, i, np.arange(n)])
    P = sp.csr_matrix((np.concatenate([v + extra, v + extra, diag]), (r, c)), shape=(n, n))
    P.sort_indices()
    return P


def node_matrix(bs, Lp, seed):
    """A = H (Lp (x) I_bs) H, symmetrised, as (n, rowptr, colind, values): both triangles, columns ascending"""
    import scipy.sparse as sp
    m = Lp.shape[0]
    H = sp.bsr_matrix((node_roots(bs, m, seed), np.arange(m), np.arange(m + 1)), shape=(m * bs, m * bs)).tocsr()
    A = (H @ sp.kron(Lp, sp.identity(bs), format="csr") @ H).tocsr()
    A = ((A + A.T) * 0.5).tocsr()
    A.sort_indices()
    return m * bs, A.indptr.astype(np.int32), A.indices.astype(np.int32), A.data.astype(np.float64)


@functools.lru_cache(maxsize=None)
def rotated_node_laplacian(bs, nx, ny, seed=11):
    """computed once, shared, unchanged"""
    return node_matrix(bs, perturbed(*lap2d(nx, ny), seed=seed + 1), seed)


# ---- one level, restated ----------------------------------------------------------------------------------------
def node_blocks_of(n, rp, ci, va, bs):
    """the bs x bs diagonal blocks, (m, bs, bs)"""
    import scipy.sparse as sp
    A = sp.csr_matrix((va, ci.copy(), rp.copy()), shape=(n, n))
    m = n // bs
    D = np.zeros((m, bs, bs))
    rows = np.repeat(np.arange(n), np.diff(rp))
    inside = rows // bs == ci // bs
    np.add.at(D, (rows[inside] // bs, rows[inside] % bs, ci[inside] % bs), va[inside])
    assert A.shape == (n, n)
    return D


def inverse_roots(D):
    """W_i = Q diag(1 / sqrt(ev)) Q^T by numpy.linalg.eigh"""
    ev, Q = np.linalg.eigh(D)
    assert np.all(ev > 0)
    return np.einsum("kia,ka,kja->kij", Q, 1 / np.sqrt(ev), Q)


def root_residual(W, D):
    """the largest ||W_i D_i W_i - I||_F"""
    R = np.einsum("kia,kab,kbj->kij", W, D, W) - np.eye(D.shape[1])
    return float(np.max(np.sqrt(np.sum(R * R, axis=(1, 2)))))


def _match_greedy(S, check):
    """S: {i: {j: strength}} of the node graph; the rule of test_amg_abi._model_coarsen"""
    q, made = {}, 0
    for i in sorted(S):
        if i in q:
            continue
        cand = sorted(((s, j) for j, s in S[i].items() if j != i and j not in q and s > 0), reverse=True)
        check(cand)
        q[i] = made
        if cand:
            q[cand[0][1]] = made
        made += 1
    return q, made


def _match_dominant(S, check):
    """the rule of test_amg_dominant_abi._model: synchronous rounds over the total order of the edges"""
    mate, r = {}, 0
    while r < CAP:
        r += 1
        to = {}
        for i in S:
            if i in mate:
                continue
            cand = sorted(_order(s, i, j) + (j,) for j, s in S[i].items() if j != i and j not in mate and s > 0)
            check([(-c[0], c[-1]) for c in cand])
            if cand:
                to[i] = cand[0][-1]
        pairs = [(i, j) for i, j in to.items() if i < j and to.get(j) == i]
        for i, j in pairs:
            mate[i], mate[j] = j, i
        if not pairs:
            break
    q, made = {}, 0
    for i in sorted(S):
        if i not in q:
            q[i] = made
            if i in mate:
                q[mate[i]] = made
            made += 1
    return q, made


def model_coarsen_block(n, rp, ci, va, bs, passes, matching, need_gap=True):
    """(agg per unknown, W of numpy, (nc, rowptr, colind) of the coarse lower triangle + diagonal, the smallest relative
    gap met between the best and the second-best candidate of a node, the coarse matrix as a scipy CSR).  Fails with
    "badly chosen case" when a gap is not above GAP.  bs = 1 is the scalar form: W_i = 1 / sqrt(a_ii), s_ij =
    |b_ij| / sqrt(b_ii b_jj); need_gap=False for a caller that compares no aggregates."""
    import scipy.sparse as sp
    A = sp.csr_matrix((va, ci.copy(), rp.copy()), shape=(n, n))
    A = (sp.tril(A) + sp.tril(A, -1).T).tocsr()  # (only the entries with col <= row are read)
    m = n // bs
    W = inverse_roots(node_blocks_of(n, A.indptr, A.indices, A.data, bs))
    Wd = sp.bsr_matrix((W, np.arange(m), np.arange(m + 1)), shape=(n, n)).tocsr()
    B = (Wd @ A @ Wd).tocsr()
    nagg = np.arange(m)
    gaps = [np.inf]

    def check(cand):  # cand: (strength, node) with the best first
        if len(cand) > 1:
            gap = (cand[0][0] - cand[1][0]) / cand[0][0]
            gaps.append(gap)
            assert gap > GAP or not need_gap, f"badly chosen case: the two best candidates of a node differ by {gap:.3e} relative"

    for _ in range(passes):
        mm = B.shape[0] // bs
        Bb = B.tobsr((bs, bs))
        Bb.sort_indices()
        norm = np.sqrt(np.sum(Bb.data * Bb.data, axis=(1, 2)))
        brow = np.repeat(np.arange(mm), np.diff(Bb.indptr))
        N = {i: {} for i in range(mm)}
        for i, j, v in zip(brow.tolist(), Bb.indices.tolist(), norm.tolist()):
            if j <= i:
                N[i][j] = N[j][i] = v
        S = {i: {j: v / np.sqrt(N[i][i] * N[j][j]) for j, v in N[i].items() if j != i} for i in N}
        q, made = (_match_dominant if matching == "dominant" else _match_greedy)(S, check)
        qn = np.array([q[i] for i in range(mm)])
        Q = sp.kron(sp.csr_matrix((np.ones(mm), (np.arange(mm), qn)), shape=(mm, made)), sp.identity(bs), format="csr")
        B = (Q.T @ B @ Q).tocsr()
        nagg = qn[nagg]
    # the pattern: a coupled pair of nodes is a full block
    Bb = B.tobsr((bs, bs))
    Bb.sort_indices()
    nc = B.shape[0]
    rows = []
    for I in range(nc // bs):
        cols = [int(J) for J in Bb.indices[Bb.indptr[I]:Bb.indptr[I + 1]] if J <= I]
        for c in range(bs):
            rows.append([J * bs + d for J in cols for d in range(bs) if J * bs + d <= I * bs + c])
    crp = np.cumsum([0] + [len(r) for r in rows]).astype(np.int32)
    agg = (nagg[:, None] * bs + np.arange(bs)[None, :]).reshape(-1).astype(np.int32)
    return agg, W, (nc, crp, np.array([j for r in rows for j in r], np.int32)), float(min(gaps)), B


def galerkin_reference(n, rp, ci, va, bs, agg, W, nc):
    """{entry (I c, J d) with col <= row: (the sum of W_i[c, a] a_ab W_j[b, d], the sum of their moduli, their number)}
    in long double, from the given W and aggregates: keys ascending, then the three arrays"""
    import scipy.sparse as sp
    A = sp.csr_matrix((va, ci.copy(), rp.copy()), shape=(n, n))
    A = (sp.tril(A) + sp.tril(A, -1).T).tobsr((bs, bs))
    A.sort_indices()
    bi, bj = np.repeat(np.arange(n // bs), np.diff(A.indptr)), A.indices
    Wl, Al = W.astype(LD), A.data.astype(LD)
    val = np.einsum("kca,kab,kbd->kcd", Wl[bi], Al, Wl[bj])
    mod = np.einsum("kca,kab,kbd->kcd", np.abs(Wl[bi]), np.abs(Al), np.abs(Wl[bj]))
    I, J = agg[bi * bs] // bs, agg[bj * bs] // bs
    c, d = np.meshgrid(np.arange(bs), np.arange(bs), indexing="ij")
    row = (I[:, None, None] * bs + c[None]).reshape(-1)
    col = (J[:, None, None] * bs + d[None]).reshape(-1)
    keep = col <= row
    key = row[keep].astype(np.int64) * nc + col[keep]
    uniq, inv = np.unique(key, return_inverse=True)
    s, sa, k = np.zeros(len(uniq), LD), np.zeros(len(uniq), LD), np.zeros(len(uniq), np.int64)
    np.add.at(s, inv, val.reshape(-1)[keep])
    np.add.at(sa, inv, mod.reshape(-1)[keep])
    np.add.at(k, inv, bs * bs)
    return uniq, s, sa, k


# ---- the tests ------------------------------------------------------------------------------------------------
def test_the_symbols_are_declared_exported_and_bound():
    text = open(os.path.join(ROOT, "include", "cfs_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    lib = cfs.load()
    raw = C.CDLL(cfs.lib_path())
    for name in NEW:
        assert re.search(r"\bint\s+" + name + r"\s*\(", code), f"{name} is not declared in cfs_hip.h"
        assert name in _lib.SYMBOLS
        getattr(raw, name)  # dlsym
    assert lib.cfs_hip_abi_version() == 4 and C.sizeof(_lib.AmgOptions) == 24  # (no new field: the size is ABI)
    vp, ip, i, ll = C.c_void_p, C.POINTER(C.c_int), C.c_int, C.c_longlong
    for suf in ("f64", "f32"):
        assert getattr(lib, "cfs_hip_amg_create_block_" + suf).argtypes == [vp, i, vp, vp, vp, i, i, C.POINTER(_lib.AmgOptions),
                                                                            C.POINTER(vp)]
    assert lib.cfs_hip_amg_block.argtypes == [vp, ip] and lib.cfs_hip_amg_level_node_weights.argtypes == [vp, i, vp]
    assert lib.cfs_hip_debug_amg_coarsen_block.argtypes == [i, vp, vp, vp, i, i, i, vp, vp, ip, vp, vp, vp, ll, C.POINTER(ll), ip]
    assert callable(cfs.Amg.node_weights)
    import inspect
    for f in (cfs.SymMatrix.amg, cfs.Amg.__init__, cfs.coarsen):
        assert inspect.signature(f).parameters["block"].default == 1


@pytest.mark.parametrize("passes", (1, 2))
@pytest.mark.parametrize("matching", ("greedy", "dominant"))
@pytest.mark.parametrize("size", ((12, 10), (24, 20)), ids=("12x10", "24x20"))
@pytest.mark.parametrize("bs", BLOCKS)
def test_one_level_against_the_model(bs, size, matching, passes):
    n, rp, ci, va = rotated_node_laplacian(bs, *size)
    agg, W, (nc, crp, cci, cva) = cfs.coarsen(n, rp, ci, va, passes, matching=matching, block=bs)
    magg, mW, (mnc, mcrp, mcci), gap, _ = model_coarsen_block(n, rp, ci, va, bs, passes, matching)
    # the aggregates: exactly the model's, node by node
    assert W.shape == (n // bs, bs, bs) and agg.dtype == np.int32
    assert nc == mnc and nc % bs == 0 and np.array_equal(agg, magg), "the aggregates differ from the documented matching"
    assert np.array_equal(agg % bs, np.arange(n) % bs) and np.all(agg.reshape(-1, bs) // bs == (agg[::bs] // bs)[:, None])
    sizes = np.bincount(agg[::bs] // bs, minlength=nc // bs)
    assert sizes.min() >= 1 and sizes.max() <= 2 ** passes and nc <= 0.62 * n
    # W: symmetric in every bit, and as good an inverse square root as numpy's
    D = node_blocks_of(n, rp, ci, va, bs)
    res, mres = root_residual(W, D), root_residual(mW, D)
    allowed = max(4 * mres, 64 * bs * np.finfo(np.float64).eps)
    assert np.array_equal(W, W.transpose(0, 2, 1)) and res <= allowed, (res, allowed)
    # the coarse matrix: the pattern exactly, the values against long double from the library's own W and aggregates
    assert np.array_equal(crp, mcrp) and np.array_equal(cci, mcci)
    crow = np.repeat(np.arange(nc), np.diff(crp))
    key = crow.astype(np.int64) * nc + cci
    uniq, s, sa, k = galerkin_reference(n, rp, ci, va, bs, agg, W, nc)
    assert np.array_equal(key, uniq)
    err = np.abs(cva.astype(LD) - s)
    bound = (k + 4) * LD(U) * sa
    worst = float(np.max(err / np.maximum(bound, LD(1e-300))))
    print(f"amg-block-coarsen bs={bs} {size[0]}x{size[1]} {matching} passes={passes}: n={n} nc={nc} nnz={len(cva)} aggregates of "
          f"1..{2 ** passes} nodes {np.bincount(sizes)[1:].tolist()} smallest gap {gap:.2e} W residual {res:.2e} (numpy {mres:.2e}) "
          f"worst error / allowed {worst:.3f}")
    assert np.all(err <= bound), worst


@pytest.mark.parametrize("passes", (1, 2, 3))
@pytest.mark.parametrize("matching", ("greedy", "dominant"))
@pytest.mark.parametrize("name", ("lap2d40x33", "rand1026"))
def test_block_1_is_the_scalar_coarsening_in_every_bit(name, matching, passes):
    n, rp, ci, va = matrix(name)
    r1, r2 = [], []
    got, want = cfs.coarsen(n, rp, ci, va, passes, matching=matching, rounds=r1, block=1), cfs.coarsen(n, rp, ci, va, passes, matching=matching, rounds=r2)
    assert _same_level(got, want) and r1 == r2
    # ... and through the new entry point itself, which block = 1 hands to the old ones
    lib = cfs.load()
    agg, w = np.zeros(n, np.int32), np.zeros(n)
    cap = len(ci)
    crp, cci, cva = np.zeros(n + 1, np.int32), np.zeros(cap, np.int32), np.zeros(cap)
    nc, nnz, rnd = C.c_int(), C.c_longlong(), (C.c_int * 3)()
    rc = lib.cfs_hip_debug_amg_coarsen_block(n, rp.ctypes.data, ci.ctypes.data, va.ctypes.data, 1, passes, 1 if matching == "dominant" else 0,
                                             agg.ctypes.data, w.ctypes.data, C.byref(nc), crp.ctypes.data, cci.ctypes.data, cva.ctypes.data,
                                             cap, C.byref(nnz), rnd)
    assert rc == 0, lib.cfs_hip_last_error()
    mine = (agg, w, (nc.value, crp[:nc.value + 1], cci[:nnz.value], cva[:nnz.value]))
    assert _same_level(mine, want) and (matching == "greedy" or list(rnd)[:passes] == r2)


def test_the_errors_of_the_host_level():
    n, rp, ci, va = rotated_node_laplacian(3, 12, 10)
    lib = cfs.load()
    bound = lib.cfs_hip_runtime_bound()
    for block in (0, -1, 5, 7, 8):
        with pytest.raises(_lib.CfsHipError, match=f"block must be 1, 2, 3, 4 or 6, got {block}") as e:
            cfs.coarsen(n, rp, ci, va, 2, block=block)
        assert e.value.code == _lib.ERR_ARG
    for block in (2, 4):  # 360 rows: a multiple of 2 and 4 -- take one row away
        n1, rp1 = n - 1, rp[:n]
        with pytest.raises(_lib.CfsHipError, match=f"n = {n1} is not a multiple of block = {block} .a trailing partial node.") as e:
            cfs.coarsen(n1, rp1, ci[:rp1[-1]], va[:rp1[-1]], 2, block=block)
        assert e.value.code == _lib.ERR_ARG
    for passes in (0, 4):
        with pytest.raises(_lib.CfsHipError, match="passes must lie in") as e:
            cfs.coarsen(n, rp, ci, va, passes, block=3)
        assert e.value.code == _lib.ERR_ARG
    # the raw entry: block, matching, null arguments, too little room
    agg, W = np.zeros(n, np.int32), np.zeros(3 * n)
    cap = len(ci)
    crp, cci, cva = np.zeros(n + 1, np.int32), np.zeros(cap, np.int32), np.zeros(cap)
    nc, nnz = C.c_int(), C.c_longlong()
    args = [n, rp.ctypes.data, ci.ctypes.data, va.ctypes.data, 3, 2, 0, agg.ctypes.data, W.ctypes.data, C.byref(nc), crp.ctypes.data,
            cci.ctypes.data, cva.ctypes.data, cap, C.byref(nnz), None]
    for k in (1, 7, 8, 9, 10, 14):
        bad = list(args)
        bad[k] = None
        assert lib.cfs_hip_debug_amg_coarsen_block(*bad) == _lib.ERR_ARG and b"null" in lib.cfs_hip_last_error(), k
    for m in (-1, 2):
        bad = list(args)
        bad[6] = m
        assert lib.cfs_hip_debug_amg_coarsen_block(*bad) == _lib.ERR_ARG and b"matching must be" in lib.cfs_hip_last_error()
    bad = list(args)
    bad[13] = 3
    assert lib.cfs_hip_debug_amg_coarsen_block(*bad) == _lib.ERR_ARG and b"room for 3" in lib.cfs_hip_last_error() and 3 < nnz.value <= cap
    assert lib.cfs_hip_debug_amg_coarsen_block(*args) == 0
    assert lib.cfs_hip_runtime_bound() == bound


@pytest.mark.parametrize("bs", BLOCKS)
def test_a_node_block_that_is_not_positive_definite_is_refused(bs):
    """one negative eigenvalue, every diagonal entry positive: a_01 = a_10 = 2 sqrt(a_00 a_11) in two node blocks"""
    n, rp, ci, va = rotated_node_laplacian(bs, 12, 10)
    va = va.copy()
    rows = np.repeat(np.arange(n), np.diff(rp))
    for node in (5, 77):
        r0, r1 = node * bs, node * bs + 1
        d0, d1 = (float(va[(rows == r) & (ci == r)][0]) for r in (r0, r1))
        va[((rows == r0) & (ci == r1)) | ((rows == r1) & (ci == r0))] = 2 * np.sqrt(d0 * d1)
    D = node_blocks_of(n, rp, ci, va, bs)
    assert np.all(np.einsum("kii->ki", D) > 0) and int((np.linalg.eigvalsh(D).min(axis=1) <= 0).sum()) == 2
    for matching in ("greedy", "dominant"):
        with pytest.raises(_lib.CfsHipError, match=f"positive definite node blocks, 2 of {n // bs} blocks of {bs} rows .*level 0") as e:
            cfs.coarsen(n, rp, ci, va, 2, matching=matching, block=bs)
        assert e.value.code == _lib.ERR_ARG
    va[int(np.flatnonzero((rows == 9 * bs) & (ci == 9 * bs))[0])] = np.nan  # a third one, not finite
    with pytest.raises(_lib.CfsHipError, match=f"3 of {n // bs} blocks") as e:
        cfs.coarsen(n, rp, ci, va, 2, block=bs)
    assert e.value.code == _lib.ERR_ARG


def test_the_argument_checks_of_create_answer_before_any_device_work():
    """block, matching and the partial node first; then every check of cfs_hip_amg_create_* in its words"""
    lib = cfs.load()
    bound = lib.cfs_hip_runtime_bound()
    n, rp, ci, va = rotated_node_laplacian(3, 12, 10)
    fake = C.c_void_p(0x1000)  # (never dereferenced: every check below comes before the handle is looked at)

    def create(h=fake, nn=n, rowptr=rp, out=True, suf="f64", block=3, matching=0, **kw):
        a = C.c_void_p(0x7)
        o = dict(passes=0, degree=0, coarse_max=0, ratio=0.0)
        o.update(kw)
        opt = _lib.AmgOptions(o["passes"], o["degree"], o["coarse_max"], 0, o["ratio"])
        v = va.astype(np.float64 if suf == "f64" else np.float32)
        rc = getattr(lib, "cfs_hip_amg_create_block_" + suf)(h, nn, None if rowptr is None else rowptr.ctypes.data, ci.ctypes.data,
                                                             v.ctypes.data, block, matching, C.byref(opt), C.byref(a) if out else None)
        assert not out or a.value is None  # *out = NULL on every error
        return rc, lib.cfs_hip_last_error()

    bad_options = dict(passes=9, degree=9, ratio=np.nan, coarse_max=5000)
    for suf in ("f64", "f32"):
        for block in (0, -3, 5, 7, 12):  # (first: everything else is bad as well)
            rc, msg = create(suf=suf, block=block, matching=9, nn=n + 1, h=None, **bad_options)
            assert rc == _lib.ERR_ARG and b"block must be 1, 2, 3, 4 or 6" in msg, msg
        for matching in (-1, 2):
            rc, msg = create(suf=suf, matching=matching, nn=n + 1, h=None, **bad_options)
            assert rc == _lib.ERR_ARG and b"matching must be" in msg, msg
        for block, nn in ((2, n + 1), (3, n + 1), (4, n + 2), (6, n + 3)):
            rc, msg = create(suf=suf, block=block, nn=nn, h=None, **bad_options)
            assert rc == _lib.ERR_ARG and b"is not a multiple of block" in msg and b"trailing partial node" in msg, msg
        for block in (1,) + BLOCKS:  # then the scalar create's checks, in its words and order
            nn = n - n % block if block != 1 else n
            for kw in (dict(h=None), dict(rowptr=None), dict(out=False)):
                rc, msg = create(suf=suf, block=block, nn=nn, **kw, **bad_options)
                assert rc == _lib.ERR_ARG and msg == b"amg_create: null argument", (kw, msg)
            order = [("passes", 4, b"amg_create: passes must lie in [1, 3], got 4"), ("degree", 5, b"amg_create: the degree must lie in [1, 4], got 5"),
                     ("ratio", 1.0, b"amg_create: the ratio lmax / lmin must be finite and > 1"), ("coarse_max", 1025, b"amg_create: coarse_max must lie in")]
            for k, (field, v, words) in enumerate(order):
                later = {f: bad_options[f] for f, _, _ in order[k + 1:]}
                rc, msg = create(suf=suf, block=block, nn=nn, **{field: v}, **later)
                assert rc == _lib.ERR_ARG and msg.startswith(words), (field, msg)
    blk = C.c_int(9)
    assert lib.cfs_hip_amg_block(None, C.byref(blk)) == _lib.ERR_ARG and b"null" in lib.cfs_hip_last_error()
    assert lib.cfs_hip_amg_level_node_weights(None, 0, None) == _lib.ERR_ARG and b"null" in lib.cfs_hip_last_error()
    assert lib.cfs_hip_runtime_bound() == bound  # nothing above initialised the runtime


def test_the_python_arguments_are_checked_before_the_library_is_asked():
    """a node-block hierarchy is host-built and not refreshable"""
    n, rp, ci, va = rotated_node_laplacian(3, 12, 10)

    class NoHandle:  # (the ValueError comes before the matrix is looked at)
        pass

    for kw in (dict(refreshable=True), dict(setup="device", matching="dominant"), dict(refreshable=True, matching="dominant")):
        for block in BLOCKS:
            with pytest.raises(ValueError):
                cfs.Amg(NoHandle(), rp, ci, va, block=block, **kw)
