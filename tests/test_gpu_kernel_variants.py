"""Every product instantiation of the tile kernel against the long-double oracle.

cfs_sym_tile_kernel<V, BLOCK, MODE, NT, OFFB, U, DET, COMB> is compiled 96 times per value type
(72 non-deterministic: BLOCK x COMB x NT x OFFB x U; 24 deterministic: BLOCK 512 / 1024 x NT x OFFB
x U, always COMB).  Each test below reaches the instantiations of one BLOCK x DET, asserts through
SymMatrix.kernel_variant() that the intended one is what the handle launches, and compares y
(poisoned with NaN first) with oracle.csr_spmv_ld.  How each is reached:

  * U: max_slots = U x BLOCK, on a matrix whose tiles fill more than the next smaller bucket;
  * NT: CFS_HIP_NT=0|1 (the 240 MiB rule is never met at test scale);
  * COMB: CFS_HIP_COMBINE=2 (combining) / 3 (chained plan, plain kernel); a COMB = 1 report means
    the plan has sibling chains, since the knob takes effect only when there are enough;
  * OFFB: a mirrored shard (rows n/32 .. n of two ranks) whose tiles hold one-sided slots.

The matrices (rand_matrices.scattered_mesh) are mesh nodes of 1-4 unknowns coupled to random
earlier nodes: sibling rows of 2-4 lanes, rows of none to many packets with len % 4 leftovers,
and -- under CFS_HIP_FLAG_NO_REORDER -- no locality, so the tiles are cut full.  The U = 3 cases
run Format::hyb (far entries) and x is signed, so rows cancel.

Without locality a full window holds few rows: fewer slices than 2 x waves and fewer COO
leftovers than 256 x waves per tile.  So every BLOCK x DET also runs its U = 3 instantiations
(NT x COMB x OFFB) on a banded mesh (rand_matrices.banded_mesh: nodes of 3 unknowns, rows of
9-11 lower entries) whose tiles hold a whole chunk, and asserts from the group features that
some tile has more than 2 x waves slices (slices handed out by ticket) and more than 256 x waves
COO entries (the prefetched COO section)."""
import itertools

import numpy as np
import pytest

from conftest import scaled_err
from rand_matrices import banded_mesh, scattered_mesh

pytestmark = pytest.mark.gpu

NO_REORDER, NO_CALIBRATE, HYB, DET = 8, 32, 128, 1024
GROUP_FEATURES = 10  # CFS_HIP_GROUP_FEATURES: [0] tiles, [3] slices, [7] COO leftovers
# knobs that to_opts reads and that would change which instantiation or which tiles a case gets
# (the parity suites are run once with some of them forced)
PLAN_KNOBS = ("CFS_HIP_DETERMINISTIC", "CFS_HIP_HYB", "CFS_HIP_FAR_USES", "CFS_HIP_MAX_SLOTS",
              "CFS_HIP_COST_MODEL", "CFS_HIP_GROUP_SHARE_FILE")
TOL = {np.float64: 1e-12, np.float32: 1e-5}
# name order of SymMatrix.kernel_variant() (CFS_HIP_KERNEL_WORDS)
KEYS = ("value_bytes", "block", "mode", "nt", "offb", "u", "det", "comb")


def instantiations(vb, block, det):
    """the product instantiations of one value size, BLOCK and DET (pick_kernel's tables)"""
    if det:
        return {(vb, block, 0, nt, offb, u, 1, 1) for nt, offb, u in itertools.product((0, 1), (0, 1), (3, 6, 10))}
    return {(vb, block, 0, nt, offb, u, 0, comb)
            for comb, nt, offb, u in itertools.product((1, 0), (0, 1), (0, 1), (3, 6, 10))}


# instantiations no matrix can reach, each with the capacity arithmetic that rules it out.
# None: every window of 10 slots a thread fits the LDS in whole 64-slot steps (the smallest,
# deterministic fp64 at 1 024 threads, allows 6 272 > 6 x 1 024 slots).
UNREACHABLE = {}

_MATS = {}


def _matrix(kind, dtype):
    """(n, rp, ci, va, x, y_ld, absrow) of the medium, large and banded matrix, oracle computed
    once per value type"""
    key = (kind, dtype)
    if key not in _MATS:
        from oracle import oracle
        n, rp, ci, va = {"medium": lambda: scattered_mesh(50000, 10, 1),
                         "big": lambda: scattered_mesh(100000, 16, 1),
                         "banded": lambda: banded_mesh(250000)}[kind]()
        va = va.astype(dtype)
        x = np.random.default_rng(5).uniform(-1, 1, n).astype(dtype)
        y_ld, absrow = oracle.csr_spmv_ld(n, rp, ci, va, x)
        for k in [k for k in _MATS if k[1] != dtype]:  # (one value type at a time)
            del _MATS[k]
        _MATS[key] = (n, rp, ci, va, x, y_ld, absrow)
    return _MATS[key]


def _group_features(A):
    import ctypes as C
    from cfs_spmv_amd import _lib
    lib, ng = _lib.load(), C.c_int()
    buf = (C.c_longlong * (A.stats()["ngroups"] * GROUP_FEATURES))()
    _lib.check(lib.cfs_hip_sym_debug_group_features(A._h, buf, len(buf), C.byref(ng)))
    return np.frombuffer(buf, dtype=np.int64).reshape(ng.value, GROUP_FEATURES)


@pytest.fixture(autouse=True)
def _torch_first():
    """torch brings a HIP runtime of its own: it has to initialise before libcfs_hip.so's"""
    import torch
    torch.cuda.init()
    torch.cuda.set_device(0)
    yield


def _run(A, xd, rows, tdt):
    import torch
    y = torch.full((rows,), float("nan"), dtype=tdt, device="cuda")
    if A.nranks > 1:
        A.spmv_phases(y, xd, None, 7)  # mirrored shard: tiles + fold, the whole row block
    else:
        A.dense_vector_multiply(y, xd)
    torch.cuda.synchronize()
    return y.cpu().numpy()


@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("block,det", [(256, 0), (512, 0), (1024, 0), (512, 1), (1024, 1)],
                         ids=["256", "512", "1024", "512det", "1024det"])
def test_every_instantiation_against_the_oracle(monkeypatch, dtype, block, det):
    import torch
    import cfs_spmv_amd as cfs
    vb = np.dtype(dtype).itemsize
    want = instantiations(vb, block, det)
    reached, errors = set(), []
    far_seen = False
    tdt = torch.float64 if dtype == np.float64 else torch.float32
    for k in PLAN_KNOBS:
        monkeypatch.delenv(k, raising=False)
    nw = block // 64
    edges = 0
    for u, kind in ((3, "medium"), (6, "big" if block == 1024 else "medium"),
                    (10, "big" if block >= 512 else "medium"), (3, "banded")):
        n, rp, ci, va, x, y_ld, absrow = _matrix(kind, dtype)
        xd = torch.from_numpy(x).cuda()
        hyb = u == 3 and kind == "medium"
        flags = NO_REORDER | NO_CALIBRATE | (DET if det else 0) | (HYB if hyb else 0)
        opts = cfs.make_options(u * block, 0, block, flags)
        rs = np.array([0, n // 32, n], np.int32)
        for offb, nt, comb in itertools.product((0, 1), (0, 1), (1,) if det else (1, 0)):
            target = (vb, block, 0, nt, offb, u, det, comb)
            monkeypatch.setenv("CFS_HIP_NT", str(nt))
            monkeypatch.setenv("CFS_HIP_COMBINE", "2" if comb else "3")
            kw = dict(row_splits=rs, rank=1) if offb else {}
            A = cfs.SymMatrix(n, rp, ci, va, options=opts, **kw)
            got = tuple(A.kernel_variant()[k] for k in KEYS)
            st = A.stats()
            if got != target:
                errors.append(f"{kind}: wanted {dict(zip(KEYS, target))}, launches {dict(zip(KEYS, got))} "
                              f"(window {st['max_slots_used']} slots)")
                A.close()
                continue
            far_seen |= st["far_entries"] > 0
            if kind == "banded":
                f = _group_features(A)
                one = f[f[:, 0] == 1]  # groups of one tile: the features are the tile's
                if not np.any((one[:, 3] > 2 * nw) & (one[:, 7] > 256 * nw)):
                    errors.append(f"banded {dict(zip(KEYS, got))}: no tile with more than {2 * nw} slices and "
                                  f"{256 * nw} COO entries (max {one[:, 3].max(initial=0)}, "
                                  f"{one[:, 7].max(initial=0)})")
                edges += 1
            r0, r1 = A.row_begin, A.row_end
            y = _run(A, xd, r1 - r0, tdt)
            err = scaled_err(y, y_ld[r0:r1], absrow[r0:r1])
            if not err <= TOL[dtype]:
                errors.append(f"{kind} {dict(zip(KEYS, got))}: error {err:.3e} against the oracle")
            elif det and not np.array_equal(y.view(np.uint8), _run(A, xd, r1 - r0, tdt).view(np.uint8)):
                errors.append(f"{kind} {dict(zip(KEYS, got))}: two deterministic runs differ")
            else:
                reached.add(got)
            A.close()
    assert not errors, "\n".join(errors)
    assert reached | set(UNREACHABLE) == want, sorted(want - reached)
    assert far_seen, "no case of this BLOCK x DET had Format::hyb far entries"
    assert edges == (4 if det else 8)
