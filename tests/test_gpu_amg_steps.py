"""cfs_hip_amg_apply and cfs_hip_sym_pcg_amg step by step, by the method of test_gpu_pcg_cheb_steps.py: what the
kernels of csrc/cfs_solver_amg.hpp compute against the same V-cycle in np.longdouble on the CPU, the products as
long-double row sums of the CSR (oracle.csr_spmv_ldx).

The reference is built ONLY from what the readers return -- the aggregates and the stored w of every level
(Amg.aggregates), the level matrices (Amg.level_matrix; level 0 is the caller's CSR in the value type), the bounds
(Amg.info: theta and the coefficient pairs follow from them by solver.cheb_coeffs, bit for bit the library's) and
the stored inverse of the dense level (Amg.coarse_inverse), all converted exactly:

    dense level:          z = inv r
    smoother-only level:  z = S r:   z_1 = d_1 = (1/theta) dinv r;  t = A z_j;  d_{j+1} = c1_j d_j + c2_j dinv (r - t);  z_{j+1} = z_j + d_{j+1}
    otherwise:            z = S r;  t = A z;  rc_I = sum_{i in I} w_i (r_i - t_i);  ec = cycle(l + 1, rc);  z_i += w_i ec_agg(i)
                          t = A z;  d = (1/theta) dinv (r - t);  z += d;  then the same m - 1 steps
    PCG:                  the recurrence of test_gpu_pcg_cheb_steps.py with z = cycle(0, r)

It is run once in np.longdouble and once in the working precision with the kernels' rounding rules -- every vector of
every level stored in the value type, every update computed in fp64 from the stored operands and rounded once, the
restriction summed in fp64 over the members in ascending order, dinv_i = (V)(1.0 / (double)a_ii), dots in fp64 over the
stored values, r.r from the unrounded update.  d is the deviation between the two runs; the GPU, which differs from the
second only in the order of the additions inside the products, the dense rows and the dots, is allowed 4 d + 16 u
(u = 2^-53 / 2^-24).  A case whose d exceeds D_LIMIT (1e-6 / 1e-2) is badly chosen and fails.  Neither the reference
nor d involves the library's arithmetic.

Cases (matrix: coarse_max -> the levels the hierarchy then has; 2 passes, ratio 4; every one at degrees 1, 2, 3 and in
both value types; the matrices scaled as in test_gpu_pcg_steps.py):
    dense only             rand1 (a dense level of size 1), rand2, rand63: 512
    two levels             rand2: 1 (a coarse level of size 1), rand3: 1, rand63: 30, rand1023: 512, rand1026: 512
    three and more         rand5: 1, rand63: 1, rand64: 8, rand255: 16, rand257: 40, pwtk@0.05: 512
    stalled                rand65: 2 and rand1026: 8 -- the coarsening stalls at 3 and at 13 rows, above coarse_max, and
                           the level is dense all the same (n <= 1024)
    smoother-only last     pairs2300: 8 -- 1150 coupled pairs: the level of 1150 rows is diagonal, stalls, and is too
                           large for a dense one

Measured on the MI355X (d / the GPU's deviation; every line is the worst over the degrees 1, 2, 3):

  apply     f64 rand1 (1d)  0/0          rand2 (2m/1d)  1.4e-16/1.2e-16    rand63 (63m/21m/7m/2m/1d)  1.9e-16/1.8e-16
  apply     f64 rand65 (65m/24m/9m/4m/3d)  1.9e-16/1.3e-16     rand1023 (1023m/343d)  1.7e-16/1.8e-16
  apply     f64 rand1026 (1026m/344m/116m/42m/22m/16m/13d)  1.4e-16/1.0e-16     pairs2300 (2300m/1150s)  2.1e-16/2.1e-16
  apply     f64 pwtk@0.05 (10895m/2731m/690m/175d)  4.6e-16/2.8e-16    symmetry 2.0e-18
  apply     f32 rand63  1.3e-07/6.1e-08    rand1026  7.6e-08/7.6e-08    pairs2300  9.8e-08/9.1e-08
  apply     f32 pwtk@0.05  2.6e-07/1.0e-07    symmetry 1.5e-09
  iterates  f64 pwtk@0.05 m=1 k=10  3.2e-16/3.1e-16      f32 k=10  1.9e-07/1.4e-07
  iterates  f64 rand1023 (host-driven, 8 levels) m=2 k=5  3.9e-16/2.3e-16      f32  8.9e-08/8.8e-08
  inverse   f64 rand63 (63)  numpy 7.1e-14, stored 3.3e-14     rand255 (86)  3.5e-16, 7.6e-16     pwtk@0.05 (175)  3.7e-16, 6.2e-16
  inverse   f32 rand63  stored 3.6e-06 of 5.4e-06 allowed      pwtk@0.05  5.1e-08 of 6.7e-08
  pwtk@0.05 to tol 1e-8 (f64) / 1e-4 (f32): 12 / 7 iterations, the working-precision reference 12 / 7, the host-driven loop 12 / 7
  lap2d(120, 99): Jacobi PCG 409 iterations, AMG 33 (relres 8.98e-09 in long double); scaled: 438 and 37 (6.98e-09);
  levels 11880 / 2970 / 743 / 186, 1.38 MB held.
"""
import ctypes as C
import functools

import numpy as np
import pytest

from test_gpu_cg_steps import DET, DTYPES, _true_relres
from test_gpu_kernel_variants import PLAN_KNOBS
from test_gpu_lobpcg import scaled as scaled_lobpcg
from test_gpu_lobpcg_steps import lap2d
from test_gpu_pcg_steps import D_LIMIT, KS, UNIT, _deviation, _matrix, _rhs, scaled

pytestmark = pytest.mark.gpu

LD = np.longdouble
DEGREES = (1, 2, 3)
# matrix -> the coarse_max values it is run with (the module docstring says what each gives)
CONFIGS = {"rand1": (512,), "rand2": (512, 1), "rand3": (1,), "rand5": (1,), "rand63": (512, 30, 1), "rand64": (8,),
           "rand65": (2,), "rand255": (16,), "rand257": (40,), "rand1023": (512,), "rand1026": (512, 8),
           "pwtk@0.05": (512,), "pairs2300": (8,)}
APPLY_MATRICES = [f"rand{n}" for n in (1, 2, 3, 5, 63, 64, 65, 255, 257, 1023, 1026)] + ["pwtk@0.05"]
KINDS = {("rand1", 512): (2,), ("rand2", 512): (2,), ("rand63", 512): (2,), ("rand2", 1): (0, 2), ("rand3", 1): (0, 2),
         ("rand63", 30): (0, 2), ("rand1023", 512): (0, 2), ("rand1026", 512): (0, 2), ("pairs2300", 8): (0, 1)}
SENTINEL = -777.25
LEAD, TRAIL = 256, 1024  # guard entries before / behind a vector (LEAD keeps it 16-byte aligned)


@pytest.fixture(autouse=True)
def _torch_first(monkeypatch):
    """torch brings a HIP runtime of its own: it has to initialise before libcfs_hip.so's"""
    import torch
    torch.cuda.init()
    torch.cuda.set_device(0)
    for k in PLAN_KNOBS + ("CFS_HIP_CG_GRAPH",):
        monkeypatch.delenv(k, raising=False)
    yield


# ---- the matrices ---------------------------------------------------------------------------------------
def pairs(npairs):
    """blockdiag of npairs symmetric positive definite 2 x 2 blocks, as a full CSR"""
    rng = np.random.default_rng(npairs)
    a, c = rng.uniform(1.0, 2.0, npairs), rng.uniform(1.0, 2.0, npairs)
    b = rng.uniform(0.2, 0.9, npairs) * np.sqrt(a * c) * rng.choice([-1.0, 1.0], npairs)
    n = 2 * npairs
    rp = 2 * np.arange(n + 1, dtype=np.int32)
    ci = np.repeat(2 * np.arange(npairs, dtype=np.int32), 4) + np.tile(np.array([0, 1, 0, 1], np.int32), npairs)
    va = np.stack([a, b, b, c], axis=1).reshape(-1)
    return n, rp, ci.astype(np.int32), va


@functools.lru_cache(maxsize=None)
def _case(name, dtype):
    """(n, rp, ci, va in the value type): the scaled matrix of test_gpu_pcg_steps.py; computed once, shared, unchanged"""
    n, rp, ci, va = pairs(int(name[5:]) // 2) if name.startswith("pairs") else _matrix(name)
    return n, rp, ci, scaled(n, rp, ci, va, dtype)


def _full(n, rp, ci, va):
    """both triangles, as a scipy CSR with sorted columns, from a lower triangle + diagonal"""
    import scipy.sparse as sp
    L = sp.csr_matrix((va, ci.copy(), rp.copy()), shape=(n, n))
    A = (L + sp.tril(L, -1).T).tocsr()
    A.sort_indices()
    return A


# ---- the CPU side -----------------------------------------------------------------------------------------
class Level:
    def __init__(self, A, kind, lmin, lmax, degree):
        from cfs_spmv_amd.solver import cheb_coeffs
        self.A, self.n, self.kind = A, A.shape[0], kind
        self.rp, self.ci, self.va = A.indptr.astype(np.int32), A.indices.astype(np.int32), A.data
        self.diag = A.diagonal().astype(A.dtype)
        if kind != 2:
            theta, self.pairs = cheb_coeffs(degree, lmin, lmax)
            self.inv_theta = 1.0 / theta
        self.agg = self.w = self.inv = None

    def mv(self, x, dtype):
        from oracle import oracle
        if dtype is None:
            return oracle.csr_spmv_ldx(self.n, self.rp, self.ci, self.va, x)
        return (self.A @ x).astype(dtype)

    def dinv(self, dtype):
        if dtype is None:
            return 1 / self.diag.astype(LD)
        return (1.0 / self.diag.astype(np.float64)).astype(dtype).astype(np.float64)


class Hierarchy:
    """what the readers of an Amg return, and the V-cycle they define: in long double (dtype None) or in the working
    precision"""

    def __init__(self, G, n, rp, ci, va, degree):
        import scipy.sparse as sp
        inf = G.info()
        self.info, self.dtype, self.degree, self.levels = inf, va.dtype.type, degree, []
        for l in range(inf["levels"]):
            if l == 0:
                A = sp.csr_matrix((va, ci.copy(), rp.copy()), shape=(n, n))
                A.sort_indices()
            else:
                ln, lrp, lci, lva = G.level_matrix(l)
                assert ln == inf["n"][l] and lva.dtype == va.dtype and len(lva) == inf["nnz"][l]
                A = _full(ln, lrp, lci, lva)
            L = Level(A, inf["kind"][l], inf["lmin"][l], inf["lmax"][l], degree)
            if l + 1 < inf["levels"]:
                L.agg, L.w = G.aggregates(l)
                assert L.w.dtype == va.dtype and L.agg.min() == 0 and L.agg.max() == inf["n"][l + 1] - 1
            self.levels.append(L)
        if inf["kind"][-1] == 2:
            self.levels[-1].inv = G.coarse_inverse()
            assert self.levels[-1].inv.dtype == va.dtype

    def cycle(self, r, dtype=None, l=0):
        W, S = (LD, LD) if dtype is None else (dtype, np.float64)
        L = self.levels[l]
        rs = r.astype(S)
        if L.kind == 2:
            return (L.inv.astype(S) @ rs).astype(W)
        dinv = L.dinv(dtype)
        d = (S(L.inv_theta) * (rs * dinv)).astype(W)
        z = d.copy()

        def chain(z, d):
            for c1, c2 in L.pairs:
                t = L.mv(z, dtype)
                d = (S(c1) * d.astype(S) + S(c2) * ((rs - t.astype(S)) * dinv)).astype(W)
                z = (z.astype(S) + d.astype(S)).astype(W)
            return z, d
        z, d = chain(z, d)
        if L.kind == 1:
            return z
        t = L.mv(z, dtype)
        rc = np.zeros(self.levels[l + 1].n, S)
        np.add.at(rc, L.agg, L.w.astype(S) * (rs - t.astype(S)))  # (in ascending i: the members of an aggregate in order)
        ec = self.cycle(rc.astype(W), dtype, l + 1)
        z = (z.astype(S) + L.w.astype(S) * ec.astype(S)[L.agg]).astype(W)
        t = L.mv(z, dtype)
        d = (S(L.inv_theta) * ((rs - t.astype(S)) * dinv)).astype(W)
        z = (z.astype(S) + d.astype(S)).astype(W)
        return chain(z, d)[0]

    def pcg(self, b, ks=(), dtype=None, tol=0.0, maxiter=None, x0=None):
        """{k: (u_k, iterations done)} from u = x0 (0) with the kernels' guards; out["count"] = iterations until r.r is
        not > tol^2 b.b"""
        W, S = (LD, LD) if dtype is None else (dtype, np.float64)
        A = self.levels[0]
        u = np.zeros(A.n, W) if x0 is None else x0.astype(W)
        r = (b.astype(S) - A.mv(u, dtype).astype(S)).astype(W)
        rr = np.dot(r.astype(S), r.astype(S))
        stop = S(tol) * S(tol) * np.dot(b.astype(S), b.astype(S))
        out, it, done = {}, 0, not (rr > stop)
        if not done:
            z = self.cycle(r, dtype)
            p = z.copy()
            rz = np.dot(r.astype(S), z.astype(S))
        last = max(tuple(ks) + (maxiter or 0,))
        for k in range(0, last + 1):
            if k > 0 and not done:
                q = A.mv(p, dtype)
                pq = np.dot(p.astype(S), q.astype(S))
                alpha = rz / pq if pq != 0 else S(0)
                u = (u.astype(S) + alpha * p.astype(S)).astype(W)
                rs = r.astype(S) - alpha * q.astype(S)
                rrn = np.dot(rs, rs)
                r = rs.astype(W)
                z = self.cycle(r, dtype)
                rzn = np.dot(r.astype(S), z.astype(S))
                beta = rzn / rz if rz != 0 else S(0)
                p = (z.astype(S) + beta * p.astype(S)).astype(W)
                rz, it, done = rzn, it + 1, not (rrn > stop)
            if k in ks:
                out[k] = (u.copy(), it)
            if done and maxiter is not None:
                break
        out["count"], out["u"] = it, u
        return out


# ---- the GPU side -----------------------------------------------------------------------------------------
def _setup(name, dtype, coarse_max, degree, A=None, **kw):
    import cfs_spmv_amd as cfs
    n, rp, ci, va = _case(name, dtype)
    if A is None:
        A = cfs.SymMatrix(n, rp, ci, va)
    G = A.amg(rp, ci, va, degree=degree, coarse_max=coarse_max, **kw)
    return A, G, Hierarchy(G, n, rp, ci, va, degree)


def _apply_gpu(G, r):
    """(z, the guard words are intact and r is unchanged)"""
    import torch
    n = len(r)
    zbuf = torch.full((LEAD + n + TRAIL,), SENTINEL, dtype=torch.from_numpy(r).dtype, device="cuda")
    rbuf = torch.full((LEAD + n + TRAIL,), SENTINEL, dtype=zbuf.dtype, device="cuda")
    rbuf[LEAD:LEAD + n] = torch.from_numpy(r).cuda()
    zbuf[LEAD:LEAD + n] = float("nan")
    G.apply(zbuf[LEAD:LEAD + n], rbuf[LEAD:LEAD + n])
    torch.cuda.synchronize()
    zh, rh = zbuf.cpu().numpy(), rbuf.cpu().numpy()
    clean = (np.all(zh[:LEAD] == SENTINEL) and np.all(zh[LEAD + n:] == SENTINEL) and np.all(rh[:LEAD] == SENTINEL) and
             np.all(rh[LEAD + n:] == SENTINEL) and np.array_equal(rh[LEAD:LEAD + n].view(np.uint8), r.view(np.uint8)))
    return zh[LEAD:LEAD + n].copy(), bool(clean)


def _native(A, G, b, x0=None, **kw):
    import torch
    from cfs_spmv_amd.solver import pcg_amg_native
    x0 = None if x0 is None else torch.from_numpy(x0).cuda()
    u, it, res = pcg_amg_native(A, torch.from_numpy(b).cuda(), G, x0=x0, **kw)
    torch.cuda.synchronize()
    return u.cpu().numpy(), it, res


def _shape(H):
    return "/".join(f"{n}{'msd'[k]}" for n, k in zip(H.info["n"], H.info["kind"]))


# ---- 1. the cycle alone ------------------------------------------------------------------------------------
@DTYPES
@pytest.mark.parametrize("name", APPLY_MATRICES + ["pairs2300"])
def test_apply_against_the_long_double_cycle(name, dtype):
    """z = M^-1 r at degrees 1, 2, 3 for every hierarchy of CONFIGS, its symmetry -- x . M y against y . M x within
    the same bound times ||x|| ||M y|| -- and its confinement: nothing outside z[0:n] is written, r is unchanged"""
    errors, A = [], None
    n = _case(name, dtype)[0]
    x, y = _rhs(n, dtype), np.random.default_rng(n + 77).uniform(-1, 1, n).astype(dtype)
    for coarse_max in CONFIGS[name]:
        for m in DEGREES:
            A, G, H = _setup(name, dtype, coarse_max, m, A)
            inf = H.info
            tag = f"cm={coarse_max} m={m}"
            assert (inf["passes"], inf["degree"], inf["coarse_max"], inf["ratio"]) == (2, m, coarse_max, 4.0)
            assert inf["n"][0] == n and inf["device_bytes"] > 0 and inf["setup_seconds"] >= inf["handles_seconds"] >= 0
            if (name, coarse_max) in KINDS:
                assert tuple(inf["kind"]) == KINDS[name, coarse_max], (tag, inf["kind"])
            for l in range(inf["levels"]):  # the documented rule of the last level, and the bounds
                k, last = inf["kind"][l], l + 1 == inf["levels"]
                assert (k == 0) == (not last) and (k != 2 or inf["n"][l] <= max(coarse_max, 1024)), (tag, inf)
                assert (inf["lmin"][l] == inf["lmax"][l] / 4.0 and inf["lmax"][l] > 0) if k != 2 else inf["lmax"][l] == 0
            ref = H.cycle(x)
            d = _deviation(H.cycle(x, dtype), ref)
            assert d <= D_LIMIT[dtype], f"{name} {tag}: d = {d:.3e}: badly conditioned case"
            (px, cx), (py, cy) = _apply_gpu(G, x), _apply_gpu(G, y)
            G.close()
            assert px.dtype == dtype and np.all(np.isfinite(px))
            g, allowed = _deviation(px, ref), 4 * d + 16 * UNIT[dtype]
            xl, yl, pxl, pyl = (v.astype(LD) for v in (x, y, px, py))
            asym = float(abs(np.dot(xl, pyl) - np.dot(yl, pxl)) / (np.sqrt(np.dot(xl, xl)) * np.sqrt(np.dot(pyl, pyl))))
            print(f"amg-apply {np.dtype(dtype).name} {name} {tag} levels={_shape(H)} d={d:.3e} gpu={g:.3e} allowed={allowed:.3e} "
                  f"asym={asym:.3e}")
            if not (cx and cy):
                errors.append(f"{tag}: a guard word was overwritten or r changed")
            if not g <= allowed:
                errors.append(f"{tag}: deviation {g:.3e}, allowed {allowed:.3e} (d = {d:.3e})")
            if not asym <= allowed:
                errors.append(f"{tag}: |x.My - y.Mx| / (||x|| ||My||) = {asym:.3e}, allowed {allowed:.3e}")
    A.close()
    assert not errors, f"{name} {np.dtype(dtype).name}: " + "; ".join(errors)


# ---- 2. the hierarchy ---------------------------------------------------------------------------------------
@DTYPES
@pytest.mark.parametrize("name,coarse_max,passes", [("rand63", 1, 1), ("rand63", 1, 3), ("rand1026", 8, 2), ("pwtk@0.05", 64, 2),
                                                    ("pairs2300", 8, 2)])
def test_the_hierarchy_is_the_host_coarsening_level_by_level(name, coarse_max, passes, dtype):
    """cfs_hip_debug_amg_coarsen applied to the matrix of level l (as returned, in the value type) gives the aggregates
    of level l, w rounded to the value type, and the matrix of level l + 1 rounded to the value type: bit for bit"""
    import cfs_spmv_amd as cfs
    n, rp, ci, va = _case(name, dtype)
    A, G, H = _setup(name, dtype, coarse_max, 1, passes=passes)
    inf = H.info
    assert inf["passes"] == passes and inf["levels"] >= 2
    cur = (n, rp, ci, va)
    for l in range(inf["levels"] - 1):
        agg, w, (nc, crp, cci, cva) = cfs.coarsen(cur[0], cur[1], cur[2], cur[3].astype(np.float64), passes)
        gagg, gw = G.aggregates(l)
        assert np.array_equal(agg, gagg) and np.array_equal(w.astype(dtype).view(np.uint8), gw.view(np.uint8)), l
        assert nc <= 0.9 * cur[0], (l, nc, cur[0])  # (the hierarchy went on: the coarsening had not stalled)
        ln, lrp, lci, lva = G.level_matrix(l + 1)
        assert ln == nc and np.array_equal(lrp, crp) and np.array_equal(lci, cci)
        assert np.array_equal(lva.view(np.uint8), cva.astype(dtype).view(np.uint8)), l
        cur = (ln, lrp, lci, lva)
    # why it ended here
    last = cur[0]
    if last > coarse_max:
        nc = cfs.coarsen(cur[0], cur[1], cur[2], cur[3].astype(np.float64), passes)[2][0]
        assert nc > 0.9 * last or inf["levels"] == 16
        assert inf["kind"][-1] == (2 if last <= 1024 else 1)
    else:
        assert inf["kind"][-1] == 2
    from cfs_spmv_amd import _lib
    for call in (lambda: G.aggregates(inf["levels"] - 1), lambda: G.aggregates(-1), lambda: G.level_matrix(0),
                 lambda: G.level_matrix(inf["levels"])):
        with pytest.raises(_lib.CfsHipError) as e:
            call()
        assert e.value.code == _lib.ERR_ARG
    if inf["kind"][-1] != 2:
        with pytest.raises(_lib.CfsHipError, match="smoother-only") as e:
            G.coarse_inverse()
        assert e.value.code == _lib.ERR_ARG
    G.close()
    A.close()


def _inverse_ld(A64):
    """the inverse in long double: Newton's iteration X <- X + X (I - A X) from the fp64 inverse"""
    A = A64.astype(LD)
    X = np.linalg.inv(A64).astype(LD)
    eye = np.eye(A.shape[0], dtype=LD)
    for _ in range(3):
        X = X + X @ (eye - A @ X)
    assert float(np.max(np.abs(eye - A @ X))) <= 1e-13  # (far below what fp64 reaches)
    return X


@DTYPES
@pytest.mark.parametrize("name,coarse_max", [("rand1", 512), ("rand63", 512), ("rand65", 2), ("rand255", 128), ("pwtk@0.05", 256)])
def test_the_stored_inverse_against_a_long_double_inverse(name, coarse_max, dtype):
    """||inv - inv_ref||max of the dense level; allowed: 4 x the deviation of numpy.linalg.inv (fp64) from the same
    long-double inverse, plus u_V ||inv||max for the rounding to the value type"""
    A, G, H = _setup(name, dtype, coarse_max, 1)
    L = H.levels[-1]
    assert L.kind == 2
    A64 = L.A.astype(np.float64).toarray()
    ref = _inverse_ld(A64)
    d = float(np.max(np.abs(np.linalg.inv(A64).astype(LD) - ref)))
    g = float(np.max(np.abs(L.inv.astype(LD) - ref)))
    allowed = 4 * d + UNIT[dtype] * float(np.max(np.abs(ref)))
    print(f"amg-inverse {np.dtype(dtype).name} {name} cm={coarse_max} levels={_shape(H)} numpy={d:.3e} stored={g:.3e} allowed={allowed:.3e}")
    G.close()
    A.close()
    assert np.array_equal(L.inv, L.inv.T) and g <= allowed, (g, allowed)


# ---- 3. the iterates ----------------------------------------------------------------------------------------
def _check_iterates(name, H, b, dtype, run, label="", ks=KS, x0=None):
    """run(k) -> (u_k, iterations) on the GPU from u = x0 (0); asserts every k of ks against the long-double iterate"""
    ref, work = H.pcg(b, ks, x0=x0), H.pcg(b, ks, dtype, x0=x0)
    errors = []
    for k in ks:
        u_ref, _ = ref[k]
        d = _deviation(work[k][0], u_ref)
        assert d <= D_LIMIT[dtype], f"{name} m={H.degree}: d_{k} = {d:.3e}: badly conditioned case"
        u, it = run(k)
        g, allowed = _deviation(u, u_ref), 4 * d + 16 * UNIT[dtype]
        print(f"amg-pcg-steps {np.dtype(dtype).name} {name}{label} m={H.degree} levels={_shape(H)} k={k} d_k={d:.3e} gpu={g:.3e} "
              f"allowed={allowed:.3e} it={it}")
        # fewer than k iterations only where the recurrence's residual can vanish exactly: tiny systems
        if not (it == k if H.levels[0].n > 5 else 1 <= it <= k):
            errors.append(f"k={k}: {it} iterations")
        if not g <= allowed:
            errors.append(f"k={k}: deviation {g:.3e} from the long-double iterate, allowed {allowed:.3e} (d_k = {d:.3e})")
    return [f"m={H.degree}{label}: " + e for e in errors]


@DTYPES
@pytest.mark.parametrize("name", APPLY_MATRICES)
def test_iterates_against_the_long_double_recurrence(name, dtype):
    """u_k, k in KS (tol = 0, maxiter = k), at degree 1 with the deepest hierarchy of CONFIGS; rand257 also at degree 2"""
    errors, A = [], None
    n = _case(name, dtype)[0]
    b = _rhs(n, dtype)
    for m in (1, 2) if name == "rand257" else (1,):
        A, G, H = _setup(name, dtype, min(CONFIGS[name]), m, A)
        errors += _check_iterates(name, H, b, dtype, lambda k: _native(A, G, b, tol=0.0, maxiter=k)[:2])
        G.close()
    A.close()
    assert not errors, f"{name} {np.dtype(dtype).name}: " + "; ".join(errors)


@DTYPES
def test_iteration_count_and_reported_residual(dtype):
    n, rp, ci, va = _case("pwtk@0.05", dtype)
    b = _rhs(n, dtype)
    A, G, H = _setup("pwtk@0.05", dtype, 512, 1)
    # tol = 0: exactly maxiter iterations, whatever check_every says
    for check_every, k in ((1, 7), (16, 12), (1000, 3)):
        u, it, res = _native(A, G, b, tol=0.0, maxiter=k, check_every=check_every)
        assert it == k, (check_every, k, it)
        true, slack = _true_relres(n, rp, ci, va, b, u, dtype)
        print(f"amg-pcg-steps {np.dtype(dtype).name} relres k={k} reported={res:.6e} long double={true:.6e} slack={slack:.3e}")
        assert abs(res - true) <= slack, (k, res, true, slack)
    # a converged solve: the count of the reference run in the working precision, give or take the one iteration a
    # residual hard against the threshold may move
    tol = 1e-8 if dtype == np.float64 else 1e-4
    count = H.pcg(b, (), dtype, tol=tol, maxiter=200)["count"]
    u, it, res = _native(A, G, b, tol=tol, maxiter=200)
    true, slack = _true_relres(n, rp, ci, va, b, u, dtype)
    print(f"amg-pcg-steps {np.dtype(dtype).name} pwtk@0.05 tol={tol}: {it} iterations, the reference {count}; reported {res:.3e}, "
          f"long double {true:.3e}")
    assert 0 < count < 200 and abs(it - count) <= 1 and res <= 10 * tol and abs(res - true) <= slack
    # b = 0 (and u = 0): nothing to do;  a NaN in b ends the solve at once
    u, it, res = _native(A, G, np.zeros(n, dtype), tol=1e-8, maxiter=50)
    assert it == 0 and not u.any() and np.isfinite(res)
    b = b.copy()
    b[n // 2] = np.nan
    u, it, res = _native(A, G, b, tol=1e-8, maxiter=300)
    assert it <= 1 and np.isnan(res), (it, res)
    G.close()
    A.close()


@DTYPES
def test_host_driven_and_native_loops_agree(dtype):
    """solver.pcg_amg (torch-driven, amg.apply as M^-1) obeys the rule of the native iterates, and on the pwtk stand-in
    the iteration counts of converged solves agree within 1"""
    import torch
    from cfs_spmv_amd.solver import pcg_amg
    A, G, H = _setup("rand1023", dtype, 8, 2)
    b = _rhs(H.levels[0].n, dtype)

    def run(k):
        u, it, _ = pcg_amg(A, torch.from_numpy(b).cuda(), G, tol=0.0, maxiter=k)
        return u.cpu().numpy(), it
    errors = _check_iterates("rand1023", H, b, dtype, run, label=" (host-driven)", ks=(1, 2, 5))
    G.close()
    A.close()
    assert not errors, "; ".join(errors)
    A, G, H = _setup("pwtk@0.05", dtype, 512, 1)
    b = _rhs(H.levels[0].n, dtype)
    tol = 1e-8 if dtype == np.float64 else 1e-4
    u1, it1, res1 = pcg_amg(A, torch.from_numpy(b).cuda(), G, tol=tol, maxiter=200)
    u2, it2, res2 = _native(A, G, b, tol=tol, maxiter=200)
    print(f"amg-pcg-steps {np.dtype(dtype).name} pwtk@0.05: host-driven {it1} iterations, native {it2}")
    assert 0 < it1 < 200 and abs(it1 - it2) <= 1 and res1 <= 10 * tol and res2 <= 10 * tol
    G.close()
    A.close()


@DTYPES
def test_a_deterministic_handle_repeats_its_bits(dtype):
    """two hierarchies on a CFS_HIP_FLAG_DETERMINISTIC handle, two runs each: identical bits in z and in u"""
    import cfs_spmv_amd as cfs
    n, rp, ci, va = _case("pwtk@0.05", dtype)
    b = _rhs(n, dtype)
    D = cfs.SymMatrix(n, rp, ci, va, options=cfs.make_options(flags=DET))
    assert D.kernel_variant()["det"] == 1
    zs, us = [], []
    for _ in range(2):
        G = D.amg(rp, ci, va, degree=2, coarse_max=64)
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


# ---- 4. refusals on the device --------------------------------------------------------------------------------
@DTYPES
def test_refusals_on_the_device(dtype):
    import torch
    import cfs_spmv_amd as cfs
    from cfs_spmv_amd import _lib
    lib = _lib.load()
    n, rp, ci, va = _case("rand1023", dtype)
    A = cfs.SymMatrix(n, rp, ci, va)
    B = cfs.SymMatrix(n, rp, ci, va)
    G = A.amg(rp, ci, va, coarse_max=64)
    S = cfs.SymMatrix(n, rp, ci, va, row_splits=np.array([0, n // 2, n], np.int32), rank=1)
    M = cfs.SymMatrix(n, rp, ci, va, ngpus=2)
    x0 = np.random.default_rng(5).uniform(-1, 1, n + 4).astype(dtype)
    buf, b = torch.from_numpy(x0).cuda(), torch.from_numpy(_rhs(n, dtype)).cuda()
    u = buf[:n]
    for H in (S, M):  # a shard, a two-shard multi-device handle: no hierarchy, no solve
        with pytest.raises(_lib.CfsHipError) as e:
            H.amg(rp, ci, va)
        assert e.value.code == _lib.ERR_UNSUPPORTED

    def solve(h, uu, bb):
        it, res = C.c_int(9), C.c_double(9.0)
        rc = lib.cfs_hip_sym_pcg_amg(h._h, G._a, uu, bb, 1e-8, 50, 1, C.byref(it), C.byref(res),
                                     torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        assert it.value == 0 and np.array_equal(buf.cpu().numpy().view(np.uint8), x0.view(np.uint8)), rc  # u untouched
        return rc
    host = np.zeros(n, dtype)
    step = x0.itemsize
    assert solve(S, u.data_ptr(), b.data_ptr()) == _lib.ERR_UNSUPPORTED
    assert solve(M, u.data_ptr(), b.data_ptr()) == _lib.ERR_UNSUPPORTED
    assert solve(B, u.data_ptr(), b.data_ptr()) == _lib.ERR_ARG and b"another handle" in lib.cfs_hip_last_error()
    assert solve(A, u.data_ptr(), u.data_ptr()) == _lib.ERR_ARG and b"different" in lib.cfs_hip_last_error()
    assert solve(A, u.data_ptr() + step, b.data_ptr()) == _lib.ERR_ARG and b"aligned" in lib.cfs_hip_last_error()
    assert solve(A, u.data_ptr(), b.data_ptr() + step) == _lib.ERR_ARG and b"aligned" in lib.cfs_hip_last_error()
    assert solve(A, host.ctypes.data & ~15, b.data_ptr()) == _lib.ERR_ARG
    assert solve(A, u.data_ptr(), host.ctypes.data & ~15) == _lib.ERR_ARG
    # the cycle alone
    z = torch.empty_like(b)
    for zz, rr in ((b.data_ptr(), b.data_ptr()), (z.data_ptr() + step, b.data_ptr()), (host.ctypes.data & ~15, b.data_ptr()),
                   (z.data_ptr(), host.ctypes.data & ~15), (None, b.data_ptr()), (z.data_ptr(), None)):
        assert lib.cfs_hip_amg_apply(G._a, zz, rr, torch.cuda.current_stream().cuda_stream) == _lib.ERR_ARG
    # a CSR of another size, another value type
    other = np.float32 if dtype == np.float64 else np.float64
    a = C.c_void_p()
    suf = "f32" if other == np.float32 else "f64"
    vo = va.astype(other)
    assert getattr(lib, "cfs_hip_amg_create_" + suf)(A._h, n, rp.ctypes.data, ci.ctypes.data, vo.ctypes.data, None,
                                                     C.byref(a)) == _lib.ERR_ARG and a.value is None
    n2, rp2, ci2, va2 = _case("rand255", dtype)
    suf = "f64" if dtype == np.float64 else "f32"
    assert getattr(lib, "cfs_hip_amg_create_" + suf)(A._h, n2, rp2.ctypes.data, ci2.ctypes.data, va2.ctypes.data, None,
                                                     C.byref(a)) == _lib.ERR_ARG and a.value is None
    # a diagonal that is not positive; a matrix that is not positive definite (one 2 x 2 minor made indefinite, the
    # diagonal still positive) on its dense level
    rows = np.repeat(np.arange(n), np.diff(rp))
    vb = va.copy()
    vb[int(np.flatnonzero((rows == ci) & (rows == 700))[0])] = -1.5
    with pytest.raises(_lib.CfsHipError, match="positive diagonal") as e:
        A.amg(rp, ci, vb)
    assert e.value.code == _lib.ERR_ARG
    n3, rp3, ci3, va3 = _case("rand63", dtype)
    r3 = np.repeat(np.arange(n3), np.diff(rp3))
    first = int(np.flatnonzero(r3 != ci3)[0])
    i, j = int(r3[first]), int(ci3[first])
    dii, djj = (float(va3[(r3 == k) & (ci3 == k)][0]) for k in (i, j))
    vc = va3.copy()
    vc[((r3 == i) & (ci3 == j)) | ((r3 == j) & (ci3 == i))] = 2 * np.sqrt(dii * djj)
    C3 = cfs.SymMatrix(n3, rp3, ci3, vc)
    with pytest.raises(_lib.CfsHipError, match="not positive definite") as e:
        C3.amg(rp3, ci3, vc)
    assert e.value.code == _lib.ERR_ARG
    # ... and everything still works
    assert A.pcg_amg(u, b, G, tol=0.0, maxiter=2)[0] == 2
    for h in (G, C3, M, S, B, A):
        h.close()


# ---- 5. what it is for ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", ["plain", "scaled"])
def test_what_the_preconditioner_is_for(form):
    """lap2d(120, 99) and its scaled form (test_gpu_lobpcg.scaled), fp64, tol 1e-8, the defaults: the native AMG-PCG
    converges, relres <= 1e-8 in long double, in at most one fifth of the iterations of the native Jacobi PCG on the
    same handle (a numpy model of the algorithm: 34 against 409, scaled 37 against 438)"""
    import torch
    import cfs_spmv_amd as cfs
    from cfs_spmv_amd.solver import pcg_native
    n, rp, ci, va = lap2d(120, 99)
    if form == "scaled":
        n, rp, ci, va = scaled_lobpcg(n, rp, ci, va)
    b = np.random.default_rng(8).uniform(-1, 1, n)
    tol = 1e-8
    A = cfs.SymMatrix(n, rp, ci, va)
    uj, itj, resj = pcg_native(A, torch.from_numpy(b).cuda(), precond="jacobi", tol=tol, maxiter=5000)
    G = A.amg(rp, ci, va)
    inf = G.info()
    u, it, res = _native(A, G, b, tol=tol, maxiter=5000)
    true, slack = _true_relres(n, rp, ci, va, b, u, np.float64)
    print(f"amg-pcg-steps lap2d120x99 {form}: Jacobi {itj} iterations (relres {resj:.3e}), AMG {it} iterations (relres {res:.3e}, "
          f"long double {true:.3e}), levels {inf['n']} kinds {inf['kind']}, {inf['device_bytes']} bytes, set-up {inf['setup_seconds']:.3f} s")
    G.close()
    A.close()
    assert (inf["passes"], inf["degree"], inf["coarse_max"], inf["ratio"]) == (2, 1, 512, 4.0)
    assert 0 < itj < 5000 and resj <= 10 * tol
    assert 0 < it and true <= tol, (it, res, true)
    assert 5 * it <= itj, (it, itj)
