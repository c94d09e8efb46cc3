"""cfs_hip_amg_apply_cols, the V-cycle on a block of columns, on the GPU.

B1 (the main check).  On a CFS_HIP_FLAG_DETERMINISTIC handle column c of a blocked call must equal cfs_hip_amg_apply on
R_c alone BYTE FOR BYTE, for every hierarchy of CASES at degrees 1 and 3 in both value types, every column count of
CALLS (1, 2, 8, 9, 16: they straddle the chunk widths of the kernels, 2, 4 and 8) and every mask (all set, 0b10100101 of
8, only the top bit of 16, and 0).  The blocks have ld > n, NaN in the Z columns before the call, SENTINEL in the padding
rows n .. ld - 1 of every column and guard words before and behind both blocks: an inactive column, the padding and the
guards must be untouched and R unchanged.  At ncols = 1 the result is that of cfs_hip_amg_apply.

B2.  On a default handle every column of a 9-column call lies within 4 d + 16 u of Hierarchy.cycle in long double, d the
deviation of the same cycle in the working precision: the allowance and the D_LIMIT rule of test_gpu_amg_steps.py.

B3 / B4.  A blocked call, a one-column apply, a narrower blocked call: the work vectors are kept (info()["device_bytes"]
grows at the first blocked call by what the documented layout needs at least, and not again), nothing leaks into the
one-column path, and the bits match on the deterministic handle.

B5.  The refusals of cfs_hip.h, Z untouched.

Hierarchies (name: coarse_max):  rand63: 512 dense only, 63 < 64 lanes;  rand3: 1 a dense level of size 1;  rand1023: 512
two levels, dense 343;  rand1026: 8 seven levels, dense 13;  rand257: 40 n no multiple of the vector width;  pairs2300: 8
smoother-only last level;  pwtk@0.05: 512 a mesh matrix;  rotated_node_laplacian(3, 12, 11) and (6, 8, 7) with block=;
rand1026: 8 once more with setup="device", matching="dominant".
"""
import functools

import numpy as np
import pytest

from test_amg_block_abi import rotated_node_laplacian
from test_gpu_amg_block import NodeHierarchy
from test_gpu_amg_steps import LEAD, SENTINEL, TRAIL, Hierarchy, _case, _torch_first  # noqa: F401
from test_gpu_cg_steps import DET, DTYPES
from test_gpu_pcg_steps import D_LIMIT, UNIT, _deviation

pytestmark = pytest.mark.gpu

DEGREES = (1, 3)
# (label, matrix, coarse_max, keywords of SymMatrix.amg)
CASES = [("rand63", "rand63", 512, {}), ("rand3", "rand3", 1, {}), ("rand1023", "rand1023", 512, {}), ("rand1026", "rand1026", 8, {}),
         ("rand257", "rand257", 40, {}), ("pairs2300", "pairs2300", 8, {}), ("pwtk@0.05", "pwtk@0.05", 512, {}),
         ("node3", "node3", 32, dict(block=3)), ("node6", "node6", 32, dict(block=6)),
         ("rand1026-device", "rand1026", 8, dict(setup="device", matching="dominant"))]
IDS = [c[0] for c in CASES]
# (ncols, mask): every call of B1
CALLS = [(1, 0b1), (2, 0b11), (8, 0xff), (8, 0b10100101), (9, 0x1ff), (16, 0xffff), (16, 1 << 15), (16, 0), (8, 0)]
MAXC = 16


@functools.lru_cache(maxsize=None)
def _matrix(name, dtype):
    """(n, rp, ci, va in the value type); computed once, shared, unchanged"""
    if name.startswith("node"):
        n, rp, ci, va = rotated_node_laplacian(3, 12, 11) if name == "node3" else rotated_node_laplacian(6, 8, 7)
        return n, rp, ci, np.asarray(va).astype(dtype)
    return _case(name, dtype)


@functools.lru_cache(maxsize=None)
def _columns(n, dtype):
    """R: (n, MAXC) uniform(-1, 1) in the value type, column-major; computed once, shared, unchanged"""
    R = np.asfortranarray(np.random.default_rng(1000 + n).uniform(-1, 1, (n, MAXC)).astype(dtype))
    R.setflags(write=False)
    return R


def _ld(n, dtype):
    per = 16 // np.dtype(dtype).itemsize
    return -(-n // per) * per + per  # (rounded up as lobpcg() rounds its ld, and one vector more: ld > n)


def _tdt(dtype):
    import torch
    return torch.float64 if dtype == np.float64 else torch.float32


class Blocks:
    """Z and R on the device: guard words, ncols columns of ld values, guard words; Z rows NaN, the padding rows SENTINEL"""

    def __init__(self, R, ncols, ld=None):
        import torch
        n, dtype = R.shape[0], R.dtype.type
        self.n, self.ncols, self.ld = n, ncols, _ld(n, dtype) if ld is None else ld
        size = LEAD + (ncols - 1) * self.ld + max(self.ld, n) + TRAIL
        z = np.full(size, SENTINEL, dtype)
        r = np.full(size, SENTINEL, dtype)
        for c in range(ncols):
            z[LEAD + c * self.ld:LEAD + c * self.ld + n] = np.nan
            r[LEAD + c * self.ld:LEAD + c * self.ld + n] = R[:, c]
        self.z0, self.r0 = z, r
        self.zbuf, self.rbuf = torch.from_numpy(z).cuda(), torch.from_numpy(r).cuda()
        assert self.zbuf.data_ptr() % 16 == 0 and self.rbuf.data_ptr() % 16 == 0

    def views(self):
        import torch
        shape, strides = (self.n, self.ncols), (1, self.ld)
        return torch.as_strided(self.zbuf[LEAD:], shape, strides), torch.as_strided(self.rbuf[LEAD:], shape, strides)

    def check(self, mask, want):
        """the errors of a call with `mask`: want[:, c] the expected bytes of the active columns"""
        import torch
        torch.cuda.synchronize()
        z, r = self.zbuf.cpu().numpy(), self.rbuf.cpu().numpy()
        errors = []
        if not np.array_equal(r.view(np.uint8), self.r0.view(np.uint8)):
            errors.append("R or its guards changed")
        expect = self.z0.copy()
        for c in range(self.ncols):
            if (mask >> c) & 1:
                expect[LEAD + c * self.ld:LEAD + c * self.ld + self.n] = want[:, c]
        if not np.array_equal(z.view(np.uint8), expect.view(np.uint8)):
            diff = np.flatnonzero((z.view(np.uint8).reshape(len(z), -1) != expect.view(np.uint8).reshape(len(z), -1)).any(axis=1))
            where = sorted({("guard" if i < LEAD or i >= LEAD + (self.ncols - 1) * self.ld + self.n else
                             f"column {(i - LEAD) // self.ld} {'row' if (i - LEAD) % self.ld < self.n else 'padding'}") for i in diff[:2000]})
            errors.append(f"Z differs in {len(diff)} words ({', '.join(where[:6])})")
        return errors

    def columns(self):
        z = self.zbuf.cpu().numpy()
        return np.stack([z[LEAD + c * self.ld:LEAD + c * self.ld + self.n] for c in range(self.ncols)], axis=1)


def _one_column(G, R):
    """cfs_hip_amg_apply on every column of R alone: (n, MAXC)"""
    import torch
    n = R.shape[0]
    out = np.zeros(R.shape, R.dtype, order="F")
    z, r = torch.zeros(n, dtype=_tdt(R.dtype.type), device="cuda"), torch.zeros(n, dtype=_tdt(R.dtype.type), device="cuda")
    for c in range(R.shape[1]):
        r.copy_(torch.from_numpy(np.ascontiguousarray(R[:, c])))
        z.fill_(float("nan"))
        G.apply(z, r)
        out[:, c] = z.cpu().numpy()
    return out


def _hierarchy(A, name, cm, degree, dtype, kw):
    n, rp, ci, va = _matrix(name, dtype)
    return A.amg(rp, ci, va, degree=degree, coarse_max=cm, **kw)


# ---- B1 ---------------------------------------------------------------------------------------------------------
@DTYPES
@pytest.mark.parametrize("label,name,cm,kw", CASES, ids=IDS)
def test_every_column_has_the_bits_of_the_one_column_cycle(label, name, cm, kw, dtype):
    import cfs_spmv_amd as cfs
    n, rp, ci, va = _matrix(name, dtype)
    R = _columns(n, dtype)
    A = cfs.SymMatrix(n, rp, ci, va, options=cfs.make_options(flags=DET))
    assert A.kernel_variant()["det"] == 1
    errors = []
    for degree in DEGREES:
        G = _hierarchy(A, name, cm, degree, dtype, kw)
        want = _one_column(G, R)
        assert np.all(np.isfinite(want))
        before = G.column_cycles()
        for ncols, mask in CALLS:
            B = Blocks(R, ncols)
            z, r = B.views()
            assert G.apply(z, r, active=mask) is z
            errors += [f"m={degree} ncols={ncols} mask={mask:#x}: {e}" for e in B.check(mask, want)]
        assert G.column_cycles() - before == sum(bin(m).count("1") for _, m in CALLS)
        G.close()
    A.close()
    assert not errors, f"{label} {np.dtype(dtype).name}: " + "; ".join(errors[:8])


# ---- B2 ---------------------------------------------------------------------------------------------------------
@DTYPES
@pytest.mark.parametrize("label,name,cm,kw", CASES, ids=IDS)
def test_every_column_against_the_long_double_cycle(label, name, cm, kw, dtype):
    import cfs_spmv_amd as cfs
    n, rp, ci, va = _matrix(name, dtype)
    R = _columns(n, dtype)
    ncols = 9
    A = cfs.SymMatrix(n, rp, ci, va)
    errors = []
    for degree in DEGREES:
        G = _hierarchy(A, name, cm, degree, dtype, kw)
        H = (NodeHierarchy.of if "block" in kw else Hierarchy)(G, n, rp, ci, va, degree)
        B = Blocks(R, ncols)
        z, r = B.views()
        G.apply(z, r)
        errors += [f"m={degree}: {e}" for e in B.check(0, None)[:1] if "R or" in e]
        Z = B.columns()
        G.close()
        assert np.all(np.isfinite(Z))
        for c in range(ncols):
            x = np.ascontiguousarray(R[:, c])
            ref = H.cycle(x)
            d = _deviation(H.cycle(x, dtype), ref)
            assert d <= D_LIMIT[dtype], f"{label} m={degree} column {c}: d = {d:.3e}: badly conditioned case"
            g, allowed = _deviation(Z[:, c], ref), 4 * d + 16 * UNIT[dtype]
            if c in (0, ncols - 1):
                print(f"amg-apply-cols {np.dtype(dtype).name} {label} m={degree} column {c}: d={d:.3e} gpu={g:.3e} allowed={allowed:.3e}")
            if not g <= allowed:
                errors.append(f"m={degree} column {c}: deviation {g:.3e}, allowed {allowed:.3e} (d = {d:.3e})")
    A.close()
    assert not errors, f"{label} {np.dtype(dtype).name}: " + "; ".join(errors[:8])


# ---- B3, B4 -----------------------------------------------------------------------------------------------------
@DTYPES
@pytest.mark.parametrize("label,name,cm,kw", [CASES[3], CASES[5], CASES[7]], ids=[IDS[3], IDS[5], IDS[7]])
def test_the_work_vectors_are_kept_and_nothing_leaks(label, name, cm, kw, dtype):
    import torch
    import cfs_spmv_amd as cfs
    n, rp, ci, va = _matrix(name, dtype)
    R = _columns(n, dtype)
    A = cfs.SymMatrix(n, rp, ci, va, options=cfs.make_options(flags=DET))
    G = _hierarchy(A, name, cm, 3, dtype, kw)
    want = _one_column(G, R)
    inf = G.info()
    b0 = inf["device_bytes"]
    per = 16 // np.dtype(dtype).itemsize
    # d and t on every level that smooths, r and z below level 0, columns of n rounded up to 16 bytes
    need = lambda w: sum(w * (-(-nl // per) * per) * np.dtype(dtype).itemsize * ((2 if kind != 2 else 0) + (2 if l > 0 else 0))
                         for l, (nl, kind) in enumerate(zip(inf["n"], inf["kind"])))

    def blocked(ncols, mask):
        B = Blocks(R, ncols)
        z, r = B.views()
        G.apply(z, r, active=mask)
        return B.check(mask, want)
    errors = blocked(8, 0xff)
    b1 = G.info()["device_bytes"]
    assert need(8) <= b1 - b0 <= need(8) + 64 * 4 * inf["levels"], (b0, b1, need(8))
    errors += blocked(8, 0b10100101)
    assert G.info()["device_bytes"] == b1, "a second call of the same width allocates nothing"
    z1, r1 = torch.full((n,), float("nan"), dtype=_tdt(dtype), device="cuda"), torch.from_numpy(np.ascontiguousarray(R[:, 5])).cuda()
    G.apply(z1, r1)
    if not np.array_equal(z1.cpu().numpy().view(np.uint8), np.ascontiguousarray(want[:, 5]).view(np.uint8)):
        errors.append("the one-column apply behind a blocked call changed its bits")
    errors += blocked(2, 0b10)
    assert G.info()["device_bytes"] == b1, "a narrower call keeps the buffers"
    errors += blocked(16, 0xffff)
    b2 = G.info()["device_bytes"]
    assert need(16) <= b2 - b0 <= need(16) + 64 * 4 * inf["levels"], "a wider call makes them again, once"
    errors += blocked(9, 0x1ff)
    assert G.info()["device_bytes"] == b2
    G.close()
    A.close()
    assert not errors, f"{label} {np.dtype(dtype).name}: " + "; ".join(errors[:8])


# ---- B5 ---------------------------------------------------------------------------------------------------------
@DTYPES
def test_refusals_leave_z_untouched(dtype):
    import torch
    import cfs_spmv_amd as cfs
    from cfs_spmv_amd import _lib
    lib = cfs.load()
    n, rp, ci, va = _matrix("rand257", dtype)
    R = _columns(n, dtype)
    A = cfs.SymMatrix(n, rp, ci, va)
    G = A.amg(rp, ci, va, coarse_max=40, refreshable=True)
    ld, vb = _ld(n, dtype), np.dtype(dtype).itemsize
    B = Blocks(R, 4)
    zp, rp_ = B.zbuf.data_ptr() + LEAD * vb, B.rbuf.data_ptr() + LEAD * vb

    def refused(word, code=_lib.ERR_ARG, a=None, z=zp, r=rp_, ld=ld, ncols=4, active=0xf):
        rc = lib.cfs_hip_amg_apply_cols(G._a if a is None else a, z, r, ld, ncols, active, None)
        assert rc == code and word in lib.cfs_hip_last_error(), (word, rc, lib.cfs_hip_last_error())
        assert not B.check(0, None), word
    for ncols in (0, -1, 17):
        refused(b"ncols", ncols=ncols)
    for ncols, active in ((4, 0x10), (4, 0xffffffff), (1, 2), (16, 1 << 16)):
        refused(b"active", ncols=ncols, active=active)
    refused(b"16-byte aligned", z=zp + vb)
    refused(b"16-byte aligned", r=rp_ + vb)
    refused(b"bad ld", ld=n - 1)
    refused(b"bad ld", ld=n, ncols=2, active=3)       # n = 257: n sizeof(V) is no multiple of 16
    refused(b"bad ld", ld=ld + 1, ncols=2, active=3)
    last = ((3 * ld + n) * vb - 1) // 16 * 16  # the last 16-byte aligned address inside the span of a block
    for off in (0, 16, last, -last):  # R inside the span of Z, before and behind
        refused(b"overlap", r=zp + off)
    host = np.zeros(4 * ld + 8, dtype)
    host = host[(-host.ctypes.data % 16) // vb:]
    refused(b"device pointer", z=host.ctypes.data)
    assert not host.any()
    # ld = n is fine for one column, and a mask of 0 enqueues nothing and returns 0 behind the checks
    before = G.column_cycles()
    assert lib.cfs_hip_amg_apply_cols(G._a, zp, rp_, ld, 4, 0, None) == 0
    assert not B.check(0, None) and G.column_cycles() == before
    one = Blocks(R, 1, ld=n)
    z, r = one.views()
    G.apply(z, r)
    got = one.columns()
    assert np.all(np.isfinite(got)) and not one.check(1, got)  # (B1 holds its bits; here: accepted, and confined)
    # a shard's hierarchy cannot exist; a hierarchy whose last refresh failed is refused
    rows = np.repeat(np.arange(n), np.diff(rp))
    zero = np.array(va)
    zero[int(np.flatnonzero((rows == ci) & (rows == 40))[0])] = 0.0
    with pytest.raises(_lib.CfsHipError):
        G.update_values(zero)
    refused(b"the last refresh failed")
    G.update_values(np.array(va))
    z, r = B.views()
    G.apply(z, r)
    torch.cuda.synchronize()
    assert bool(torch.all(torch.isfinite(z)))
    # the Python side: shapes and layouts that are not a block
    with pytest.raises(ValueError):
        G.apply(z, r[:, :2])
    with pytest.raises(ValueError):
        G.apply(z[:, 0], r[:, 0], active=1)
    with pytest.raises(ValueError):
        G.apply(torch.zeros((n, 4), dtype=_tdt(dtype), device="cuda"), r)  # row-major: not stored by columns
    G.close()
    A.close()
