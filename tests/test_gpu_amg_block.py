"""The node-block multigrid on the device (SymMatrix.amg(..., block=bs), csrc/cfs_solver_amg.hpp at THE NODE-BLOCK FORM),
by the method of test_gpu_amg_steps.py and with its bound.

NodeHierarchy is the V-cycle rebuilt ONLY from what the readers return -- the level matrices, W (Amg.node_weights) and
the aggregates of every level, lmin / lmax, the stored dense inverse; the inverse node blocks of the smoother are made
from the level matrices by the arithmetic of cg_binv_kernel (test_gpu_block_pcg_steps.cholesky_inverse):

    smoother:  z_1 = d_1 = (1/theta) Minv r;  t = A z_j;  d_{j+1} = c1_j d_j + c2_j Minv (r - t);  z_{j+1} = z_j + d_{j+1}
    restrict:  rc_I = sum_{i in I, ascending} W_i (r_i - t_i)        prolong:  z_i += W_i ec_I
    restart:   t = A z;  d = (1/theta) Minv (r - t);  z += d;  then the same m - 1 steps

once in np.longdouble and once in the working precision with the kernels' rounding rules (every vector stored in the
value type, every update computed in fp64 from the stored operands and rounded once, W_i x and Minv x summed over
ascending columns).  d is the deviation between the two runs; the GPU is allowed 4 d + 16 u, a case with d > D_LIMIT is
badly chosen and fails -- the rule of test_gpu_amg_steps.py, unchanged.

Cases of the cycle: rotated_node_laplacian(bs, 24, 20) with coarse_max 128 (ends dense) and node_pairs(bs): 600 pairs of
coupled nodes, the block form of pairs2300 -- the level of 600 nodes is block diagonal, stalls and, with more than 1024
rows, is smoother-only.

The loop edges.  Every transfer kernel gives one thread a node in its BS >= 2 form: amg_restrict_kernel a COARSE node of
the level, amg_prolong_kernel and amg_restart_kernel a fine one; one trip of the grid is 512 x 256 = 131 072 nodes.
node_band(bs, 524 292): a chain of nodes, 2 passes pair it perfectly twice, so level 0 has 524 292 = 4 x 131 072 + 4 fine
nodes -- prolong and restart take four full trips and a fifth of 4 threads -- and 131 073 = 131 072 + 1 coarse ones:
restrict takes a second trip of one thread.  524 289 nodes is the least number with more than 131 072 coarse nodes; 524 292
keeps n a multiple of every block size.  The host set-up of level 0 at that size takes 0.8 s (bs = 2) / 1.7 s (bs = 3)
on one CPU core, so passes stays 2.

What it is for: rotated_node_laplacian, where the scalar hierarchy is worse than none.  N (node-block AMG), BJ (block
Jacobi) and S (scalar AMG) are established on the CPU with the working-precision recurrences, every hierarchy built by
model_hierarchy below in numpy -- nothing of the library.

Measured on the MI355X.  z = M^-1 r: d / the GPU's deviation, then |x.My - y.Mx| / (||x|| ||My||); the worse of the
degrees 1 and 3; fp64, then fp32; the levels as _shape gives them (m multigrid, s smoother-only, d dense):

    lap   bs=2   9.8e-16/1.2e-15  2.0e-17    5.3e-07/3.4e-07  1.4e-09    960m/240m/60d
    lap   bs=3   2.0e-14/3.2e-14  1.2e-15    1.4e-05/5.5e-06  1.0e-07    1440m/360m/90d
    lap   bs=4   4.4e-14/7.6e-14  5.6e-16    2.4e-05/1.6e-05  3.8e-07    1920m/480m/120d
    lap   bs=6   1.6e-13/2.1e-13  4.2e-16    1.3e-04/4.9e-05  1.6e-06    2880m/720m/180m/48d
    pairs bs=2   1.2e-15/9.3e-16  1.5e-17    9.8e-07/7.5e-07  2.5e-09    2400m/1200s
    pairs bs=3   1.2e-14/2.9e-14  7.2e-17    7.2e-06/1.1e-05  1.9e-08    3600m/1800s
    pairs bs=4   7.8e-14/1.1e-13  1.2e-15    3.9e-05/3.3e-05  6.3e-08    4800m/2400s
    pairs bs=6   4.0e-13/4.1e-13  2.2e-15    8.4e-05/8.6e-05  6.9e-08    7200m/3600s
    band  bs=2   1.5e-15/1.7e-15  1.6e-18    7.0e-07/3.7e-07  2.0e-10    1048584m/262146m/65538m/16386m/4098m/1026m/258d
    band  bs=3   3.6e-14/3.0e-14  4.3e-18    1.7e-05/9.3e-06  4.8e-09    1572876m/393219m/98307m/24579m/6147m/1539m/387d
  (the node blocks have condition numbers of 30 to 8100: d grows with bs, and the bound with it)
  band: amg_create takes 0.58 / 0.48 s (bs = 2, fp64 / fp32) and 1.06 / 1.01 s (bs = 3), of which the level handles
  0.05 - 0.16 s; the four tests take 1.4 - 3.5 s each.
  what it is for, N / BJ / S on the CPU and the GPU's count: bs=3 24x20 19 / >= 57 / >= 57, 19;  bs=2 40x33 24 / >= 72 / >= 72,
  24;  bs=4 40x33 26 / >= 78 / >= 78, 26;  bs=6 30x25 25 / >= 75 / >= 75, 25;  fp32 bs=3 24x20 11 / >= 33 / >= 33, 11.  After
  2 N iterations the scalar hierarchy is at relres 0.06 - 1.7, block Jacobi at 0.03 - 0.36.
"""
import functools

import numpy as np
import pytest

from test_amg_block_abi import BLOCKS, inverse_roots, model_coarsen_block, node_blocks_of, node_matrix, rotated_node_laplacian
from test_gpu_amg_steps import LD, Hierarchy, Level, _apply_gpu, _full, _native, _shape, _torch_first, pairs  # noqa: F401
from test_gpu_block_pcg_steps import block_pcg_reference, cholesky_inverse, node_blocks
from test_gpu_cg_steps import DET, DTYPES, _true_relres
from test_gpu_lanczos_steps import default_v0
from test_gpu_pcg_steps import D_LIMIT, UNIT, _deviation, _rhs

pytestmark = pytest.mark.gpu

GRID = 512 * 256
EDGE_NODES = 4 * GRID + 4


def _f(dtype):
    return "f64" if dtype == np.float64 else "f32"


# ---- the matrices ---------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def node_pairs(bs, npairs=600):
    """nodes coupled in pairs only: H (P (x) I) H with P = blockdiag of npairs positive definite 2 x 2 blocks"""
    import scipy.sparse as sp
    n, rp, ci, va = pairs(npairs)
    return node_matrix(bs, sp.csr_matrix((va, ci, rp), shape=(n, n)), seed=17)


@functools.lru_cache(maxsize=None)
def node_band(bs, m=EDGE_NODES):
    """a chain of m nodes, node i coupled with i - 1 and i + 1, positive definite by diagonal dominance of the chain"""
    import scipy.sparse as sp
    off = -np.random.default_rng(3).uniform(0.5, 1.0, m - 1)
    d = np.full(m, 0.05)
    d[:-1] -= off
    d[1:] -= off
    L = sp.diags([off, d, off], [-1, 0, 1]).tocsr()
    L.sort_indices()
    return node_matrix(bs, L, seed=5)


def _matrix(name, bs, dtype):
    n, rp, ci, va = {"lap": lambda: rotated_node_laplacian(bs, 24, 20), "pairs": lambda: node_pairs(bs), "band": lambda: node_band(bs)}[name]()
    return n, rp, ci, va.astype(dtype)


# ---- the CPU side ---------------------------------------------------------------------------------------------
def bapply(M, x):
    """M_i x_i over the node blocks, the columns ascending as block_apply adds them; M (m, bs, bs), x (m bs,)"""
    m, bs, _ = M.shape
    xb = x.reshape(m, bs)
    z = np.zeros((m, bs), x.dtype)
    for j in range(bs):
        z += M[:, :, j] * xb[:, j:j + 1]
    return z.reshape(-1)


class NodeLevel(Level):
    def __init__(self, A, bs, kind, lmin, lmax, degree):
        super().__init__(A, kind, lmin, lmax, degree)
        self.bs = bs
        self.blocks = node_blocks(self.n, self.rp, self.ci, self.va, bs) if kind != 2 else None
        self.W = self.nagg = None

    def minv(self, dtype):
        """the inverse node blocks: exact in long double, else as cg_binv_kernel stores them"""
        if self.bs == 1:
            return self.dinv(dtype).reshape(-1, 1, 1)
        if dtype is None:
            return cholesky_inverse(self.blocks, LD)
        return cholesky_inverse(self.blocks, np.float64).astype(dtype).astype(np.float64)


class NodeHierarchy(Hierarchy):
    """the cycle of a node-block hierarchy; pcg() is Hierarchy's"""

    def __init__(self, levels, dtype, degree, info=None):
        self.levels, self.dtype, self.degree, self.info = levels, dtype, degree, info

    @classmethod
    def of(cls, G, n, rp, ci, va, degree):
        """from what the readers of an Amg return"""
        import scipy.sparse as sp
        inf = G.info()
        bs, levels = inf["block"], []
        for l in range(inf["levels"]):
            if l == 0:
                A = sp.csr_matrix((va, ci.copy(), rp.copy()), shape=(n, n))
                A.sort_indices()
            else:
                ln, lrp, lci, lva = G.level_matrix(l)
                assert ln == inf["n"][l] and lva.dtype == va.dtype and len(lva) == inf["nnz"][l]
                A = _full(ln, lrp, lci, lva)
            L = NodeLevel(A, bs, inf["kind"][l], inf["lmin"][l], inf["lmax"][l], degree)
            if l + 1 < inf["levels"]:
                agg, w = G.aggregates(l)
                L.W = G.node_weights(l)
                assert w is None and L.W.dtype == va.dtype and L.W.shape == (L.n // bs, bs, bs)
                assert np.array_equal(agg % bs, np.arange(L.n) % bs) and agg.min() == 0 and agg.max() == inf["n"][l + 1] - 1
                L.nagg = agg[::bs] // bs
                assert np.array_equal(agg, (L.nagg[:, None] * bs + np.arange(bs)).reshape(-1))
            levels.append(L)
        if inf["kind"][-1] == 2:
            levels[-1].inv = G.coarse_inverse()
        return cls(levels, va.dtype.type, degree, inf)

    def cycle(self, r, dtype=None, l=0):
        W, S = (LD, LD) if dtype is None else (dtype, np.float64)
        L = self.levels[l]
        rs = r.astype(S)
        if L.kind == 2:
            return (L.inv.astype(S) @ rs).astype(W)
        minv = L.minv(dtype).astype(S)
        d = (S(L.inv_theta) * bapply(minv, rs)).astype(W)
        z = d.copy()

        def chain(z, d):
            for c1, c2 in L.pairs:
                t = L.mv(z, dtype)
                d = (S(c1) * d.astype(S) + S(c2) * bapply(minv, rs - t.astype(S))).astype(W)
                z = (z.astype(S) + d.astype(S)).astype(W)
            return z, d
        z, d = chain(z, d)
        if L.kind == 1:
            return z
        C, bs, Wl = self.levels[l + 1], L.bs, L.W.astype(S)
        t = L.mv(z, dtype)
        rc = np.zeros((C.n // bs, bs), S)
        np.add.at(rc, L.nagg, bapply(Wl, rs - t.astype(S)).reshape(-1, bs))  # (in ascending i: the member nodes in order)
        ec = self.cycle(rc.reshape(-1).astype(W), dtype, l + 1)
        z = (z.astype(S) + bapply(Wl, ec.astype(S).reshape(-1, bs)[L.nagg].reshape(-1))).astype(W)
        t = L.mv(z, dtype)
        d = (S(L.inv_theta) * bapply(minv, rs - t.astype(S))).astype(W)
        z = (z.astype(S) + d.astype(S)).astype(W)
        return chain(z, d)[0]


def model_hierarchy(n, rp, ci, va, bs, dtype, degree=1, passes=2, ratio=4.0, coarse_max=512):
    """the hierarchy the header describes, built in numpy: W from eigh, the greedy matching of model_coarsen_block, every
    level rounded to the value type, lmax = 1.1 x 16 power steps from the documented start vector, the dense inverse
    numpy's.  bs = 1: the scalar hierarchy.  Nothing of the library."""
    import scipy.sparse as sp
    from test_gpu_pcg_cheb_steps import Problem, power_reference
    levels = []
    A = sp.csr_matrix((va.astype(dtype), ci.copy(), rp.copy()), shape=(n, n))
    A.sort_indices()
    while True:
        ln = A.shape[0]
        last, kind = ln <= coarse_max, 2 if ln <= coarse_max else 0
        if not last:
            a64 = A.astype(np.float64)
            agg, W, (nc, _, _), _, B = model_coarsen_block(ln, a64.indptr, a64.indices, a64.data, bs, passes, "greedy", need_gap=bs > 1)
            if nc > 0.9 * ln or len(levels) + 1 == 16:
                last, kind = True, 2 if ln <= 1024 else 1
        lmin = lmax = 0.0
        if kind != 2:
            blocks = node_blocks(ln, A.indptr, A.indices, A.data, bs)
            minv = cholesky_inverse(blocks, np.float64).astype(dtype) if bs > 1 else (1.0 / blocks.astype(np.float64)).astype(dtype)
            P = Problem(ln, A.indptr.astype(np.int32), A.indices.astype(np.int32), A.data, "block_jacobi", minv)
            lmax = 1.1 * float(power_reference(P, default_v0(ln), 16, dtype))
            lmin = lmax / ratio
        L = NodeLevel(A, bs, kind, lmin, lmax, degree)
        levels.append(L)
        if kind == 2:
            inv = np.linalg.inv(A.astype(np.float64).toarray())
            L.inv = (0.5 * (inv + inv.T)).astype(dtype)
        if last:
            break
        L.W, L.nagg = W.astype(dtype), agg[::bs] // bs
        B = B.astype(dtype).tocsr()
        B.sort_indices()
        A = B
    return NodeHierarchy(levels, dtype, degree)


# ---- the GPU side ---------------------------------------------------------------------------------------------
def _setup(name, bs, dtype, degree, A=None, coarse_max=128, **kw):
    import cfs_spmv_amd as cfs
    n, rp, ci, va = _matrix(name, bs, dtype)
    if A is None:
        A = cfs.SymMatrix(n, rp, ci, va)
    G = A.amg(rp, ci, va, degree=degree, coarse_max=coarse_max, block=bs, **kw)
    return A, G, NodeHierarchy.of(G, n, rp, ci, va, degree)


def _check_apply(name, G, H, dtype, tag):
    """z = M^-1 r against the long-double cycle, its symmetry and its confinement; returns the errors"""
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
    print(f"amg-block apply {_f(dtype)} {name} {tag} levels={_shape(H)} d={d:.3e} gpu={g:.3e} allowed={allowed:.3e} asym={asym:.3e}")
    if not (cx and cy):
        errors.append(f"{tag}: a guard word was overwritten or r changed")
    if not g <= allowed:
        errors.append(f"{tag}: deviation {g:.3e}, allowed {allowed:.3e} (d = {d:.3e})")
    if not asym <= allowed:
        errors.append(f"{tag}: |x.My - y.Mx| / (||x|| ||My||) = {asym:.3e}, allowed {allowed:.3e}")
    return errors


# ---- 4. the hierarchy -----------------------------------------------------------------------------------------
@DTYPES
@pytest.mark.parametrize("matching", ("greedy", "dominant"))
@pytest.mark.parametrize("bs", BLOCKS)
def test_the_hierarchy_is_the_host_coarsening_level_by_level(bs, matching, dtype):
    """cfs.coarsen(..., block=bs) applied to the matrix of level l (as returned, in the value type) gives the aggregates
    of level l, W rounded to the value type and the matrix of level l + 1 rounded to the value type: bit for bit"""
    import cfs_spmv_amd as cfs
    from cfs_spmv_amd import _lib
    n, rp, ci, va = _matrix("lap", bs, dtype)
    A = cfs.SymMatrix(n, rp, ci, va)
    G = A.amg(rp, ci, va, coarse_max=40, matching=matching, block=bs)
    inf = G.info()
    assert inf["block"] == bs and inf["levels"] >= 3 and inf["n"][0] == n and all(k % bs == 0 for k in inf["n"])
    assert tuple(inf["kind"]) == (0,) * (inf["levels"] - 1) + (2,) and inf["n"][-1] <= 40 and inf["device_bytes"] > 0
    assert G.setup_info()["matching"] == matching and G.setup_info()["setup"] == "host"
    for l in range(inf["levels"]):
        k = inf["kind"][l]
        assert (inf["lmin"][l] == inf["lmax"][l] / 4.0 and inf["lmax"][l] > 0) if k != 2 else inf["lmax"][l] == 0
    cur = (n, rp, ci, va)
    for l in range(inf["levels"] - 1):
        agg, W, (nc, crp, cci, cva) = cfs.coarsen(cur[0], cur[1], cur[2], cur[3].astype(np.float64), 2, matching=matching, block=bs)
        gagg, gw = G.aggregates(l)
        gW = G.node_weights(l)
        assert gw is None and np.array_equal(agg, gagg), l
        assert gW.dtype == dtype and np.array_equal(W.astype(dtype).view(np.uint8), gW.view(np.uint8)), l
        assert np.array_equal(gW, gW.transpose(0, 2, 1))
        ln, lrp, lci, lva = G.level_matrix(l + 1)
        assert ln == nc == inf["n"][l + 1] and np.array_equal(lrp, crp) and np.array_equal(lci, cci)
        assert np.array_equal(lva.view(np.uint8), cva.astype(dtype).view(np.uint8)), l
        cur = (ln, lrp, lci, lva)
    # the readers' refusals, and what a node-block hierarchy is not
    lib = _lib.load()
    w = np.zeros(n, dtype)
    assert lib.cfs_hip_amg_level_aggregates(G._a, 0, None, w.ctypes.data) == _lib.ERR_ARG and b"w must be NULL" in lib.cfs_hip_last_error()
    for call in (lambda: G.node_weights(inf["levels"] - 1), lambda: G.node_weights(-1), lambda: G.aggregates(inf["levels"] - 1),
                 lambda: G.update_values(va)):
        with pytest.raises(_lib.CfsHipError) as e:
            call()
        assert e.value.code == _lib.ERR_ARG
    S = A.amg(rp, ci, va, coarse_max=40)  # every other kind of hierarchy answers 1 and has no W
    assert S.info()["block"] == 1
    with pytest.raises(_lib.CfsHipError, match="block > 1") as e:
        S.node_weights(0)
    assert e.value.code == _lib.ERR_ARG
    for h in (S, G, A):
        h.close()


@DTYPES
@pytest.mark.parametrize("matching", ("greedy", "dominant"))
def test_block_1_is_the_scalar_create(matching, dtype):
    """cfs_hip_amg_create_block_* with block = 1 against cfs_hip_amg_create_* / _dominant_* on a deterministic handle: the
    same levels, aggregates, weights, matrices and inverse, and the same bits in z"""
    import ctypes as C
    import cfs_spmv_amd as cfs
    from cfs_spmv_amd import _lib
    n, rp, ci, va = _matrix("lap", 3, dtype)
    D = cfs.SymMatrix(n, rp, ci, va, options=cfs.make_options(flags=DET))
    want = D.amg(rp, ci, va, coarse_max=128, matching=matching)
    got = cfs.Amg.__new__(cfs.Amg)
    got.A, got.dtype, got.refreshable, got._a = D, D.dtype, False, C.c_void_p()
    opt = _lib.AmgOptions(2, 1, 128, 0, 4.0)
    create = getattr(_lib.load(), "cfs_hip_amg_create_block_" + _f(dtype))
    _lib.check(create(D._h, n, rp.ctypes.data, ci.ctypes.data, va.ctypes.data, 1, 1 if matching == "dominant" else 0, C.byref(opt),
                      C.byref(got._a)))
    a, b = got.info(), want.info()
    assert a["block"] == b["block"] == 1 and got.setup_info()["matching"] == matching
    for k in ("levels", "n", "nnz", "kind", "lmin", "lmax", "device_bytes", "passes", "degree", "coarse_max", "ratio"):
        assert a[k] == b[k], k
    same = lambda x, y: x.dtype == y.dtype and np.array_equal(x.view(np.uint8), y.view(np.uint8))
    for l in range(a["levels"] - 1):
        assert all(same(x, y) for x, y in zip(got.aggregates(l), want.aggregates(l)))
        (gn, *garrays), (wn, *warrays) = got.level_matrix(l + 1), want.level_matrix(l + 1)
        assert gn == wn and all(same(x, y) for x, y in zip(garrays, warrays))
    r = _rhs(n, dtype)
    assert same(got.coarse_inverse(), want.coarse_inverse()) and same(_apply_gpu(got, r)[0], _apply_gpu(want, r)[0])
    for h in (got, want, D):
        h.close()


# ---- 5. one cycle, 6. its symmetry ----------------------------------------------------------------------------
@DTYPES
@pytest.mark.parametrize("name", ("lap", "pairs"))
@pytest.mark.parametrize("bs", BLOCKS)
def test_apply_against_the_long_double_cycle(bs, name, dtype):
    """z = M^-1 r at degrees 1 and 3, a hierarchy that ends dense (lap) and one that ends smoother-only (pairs); the
    symmetry x . M y = y . M x within the same bound; nothing outside z[0:n] is written, r is unchanged"""
    errors, A = [], None
    for m in (1, 3):
        A, G, H = _setup(name, bs, dtype, m, A)
        inf = H.info
        assert inf["block"] == bs and inf["degree"] == m and all(k % bs == 0 for k in inf["n"])
        assert tuple(inf["kind"]) == ((0, 1) if name == "pairs" else (0,) * (inf["levels"] - 1) + (2,)), inf["kind"]
        if name == "pairs":
            assert inf["n"][1] == 600 * bs > 1024
        errors += _check_apply(f"{name} bs={bs}", G, H, dtype, f"m={m}")
        G.close()
    A.close()
    assert not errors, f"{name} bs={bs} {_f(dtype)}: " + "; ".join(errors)


@DTYPES
def test_a_deterministic_handle_repeats_its_bits(dtype):
    """two hierarchies on a CFS_HIP_FLAG_DETERMINISTIC handle, two runs each: identical bits in z and in u"""
    import cfs_spmv_amd as cfs
    n, rp, ci, va = _matrix("lap", 3, dtype)
    b = _rhs(n, dtype)
    D = cfs.SymMatrix(n, rp, ci, va, options=cfs.make_options(flags=DET))
    assert D.kernel_variant()["det"] == 1
    zs, us = [], []
    for _ in range(2):
        G = D.amg(rp, ci, va, degree=2, coarse_max=128, block=3)
        for _ in range(2):
            zs.append(_apply_gpu(G, b)[0])
            us.append(_native(D, G, b, tol=0.0, maxiter=9))
        G.close()
    D.close()
    assert all(it == 9 for _, it, _ in us) and np.all(np.isfinite(zs[0]))
    for z in zs[1:]:
        assert np.array_equal(z.view(np.uint8), zs[0].view(np.uint8))
    for u, _, res in us[1:]:
        assert np.array_equal(u.view(np.uint8), us[0][0].view(np.uint8)) and res == us[0][2]


# ---- 7. the loop edges ----------------------------------------------------------------------------------------
@DTYPES
@pytest.mark.parametrize("bs", (2, 3))
def test_beyond_one_trip_of_the_grid(bs, dtype):
    """node_band(bs): 524 292 = 4 x 131 072 + 4 fine nodes and 131 073 = 131 072 + 1 coarse nodes at level 0 (the module
    docstring has the arithmetic): amg_prolong_kernel and amg_restart_kernel run five trips, the last of 4
    threads, amg_restrict_kernel a second trip of one thread.  The cycle against the long-double model."""
    A, G, H = _setup("band", bs, dtype, 1, coarse_max=512)
    inf = H.info
    print(f"amg-block edges {_f(dtype)} bs={bs}: levels {_shape(H)}, set-up {inf['setup_seconds']:.2f} s of which the level handles "
          f"{inf['handles_seconds']:.2f} s, {inf['device_bytes']} bytes")
    assert inf["passes"] == 2 and inf["n"][0] == bs * EDGE_NODES and inf["n"][0] // bs == 4 * GRID + 4
    assert inf["n"][1] // bs == GRID + 1 and inf["kind"][0] == inf["kind"][1] == 0
    errors = _check_apply(f"band bs={bs}", G, H, dtype, "m=1")
    G.close()
    A.close()
    assert not errors, "; ".join(errors)


# ---- 8. what it is for ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("bs,size,dtype", [(3, (24, 20), np.float64), (2, (40, 33), np.float64), (4, (40, 33), np.float64),
                                           (6, (30, 25), np.float64), (3, (24, 20), np.float32)],
                         ids=["bs3-24x20-f64", "bs2-40x33-f64", "bs4-40x33-f64", "bs6-30x25-f64", "bs3-24x20-f32"])
def test_what_the_preconditioner_is_for(bs, size, dtype):
    """couplings inside a node as strong as the diagonal, node frames rotated against the axes: block Jacobi and the
    scalar hierarchy both need at least three times the iterations of the node-block hierarchy.  The three counts are
    first established on the CPU (model_hierarchy, the working-precision recurrences); the GPU must then reproduce N
    within +-2, while block-Jacobi PCG and PCG with the scalar hierarchy are still unconverged after 2 N iterations."""
    import torch
    import cfs_spmv_amd as cfs
    from cfs_spmv_amd.solver import pcg_native
    n, rp, ci, va = rotated_node_laplacian(bs, *size)
    va = va.astype(dtype)
    b = np.random.default_rng(8).uniform(-1, 1, n).astype(dtype)
    tol = 1e-8 if dtype == np.float64 else 1e-4
    N = model_hierarchy(n, rp, ci, va, bs, dtype).pcg(b, (), dtype, tol=tol, maxiter=500)["count"]
    minv = cholesky_inverse(node_blocks(n, rp, ci, va, bs), np.float64).astype(dtype)
    BJ = block_pcg_reference(n, rp, ci, va, b, minv, dtype=dtype, tol=tol, maxiter=3 * N)["count"]
    S = model_hierarchy(n, rp, ci, va, 1, dtype).pcg(b, (), dtype, tol=tol, maxiter=3 * N)["count"]
    print(f"amg-block what-for {_f(dtype)} bs={bs} {size[0]}x{size[1]} n={n}: node-block AMG {N} iterations, block Jacobi at least {BJ}, "
          f"scalar AMG at least {S} (CPU)")
    assert 0 < N < 500 and BJ >= 3 * N and S >= 3 * N, f"badly chosen case: N = {N}, BJ >= {BJ}, S >= {S}"
    A = cfs.SymMatrix(n, rp, ci, va)
    G = A.amg(rp, ci, va, block=bs)
    u, it, res = _native(A, G, b, tol=tol, maxiter=500)
    true, slack = _true_relres(n, rp, ci, va, b, u, dtype)
    Gs = A.amg(rp, ci, va)
    us, its, ress = _native(A, Gs, b, tol=tol, maxiter=2 * N)
    ub, itb, resb = pcg_native(A, torch.from_numpy(b).cuda(), precond="block_jacobi", block=bs, tol=tol, maxiter=2 * N)
    inf = G.info()
    print(f"amg-block what-for {_f(dtype)} bs={bs}: GPU {it} iterations (relres {res:.3e}, long double {true:.3e}); after {2 * N}: scalar AMG "
          f"relres {ress:.3e}, block Jacobi {resb:.3e}; levels {inf['n']} kinds {inf['kind']}, {inf['device_bytes']} bytes")
    for h in (Gs, G, A):
        h.close()
    assert inf["block"] == bs and (inf["passes"], inf["degree"], inf["coarse_max"], inf["ratio"]) == (2, 1, 512, 4.0)
    assert res <= 10 * tol and abs(res - true) <= slack, (res, true, slack)
    assert N - 2 <= it <= N + 2, (it, N)
    assert its == 2 * N and ress > tol and itb == 2 * N and resb > tol, (its, ress, itb, resb)
