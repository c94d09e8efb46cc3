"""The failure paths of cfs_hip_sym_create_multi_* (cfs_multi.hpp), and what is left behind them.

A multi-device create that fails after its first shards exist has to take apart a half-built handle --
shards with their device arrays, streams and events -- and still report the code and the message of
what failed, not of the teardown.  So: a device list whose second entry is out of range, and a matrix
that a later shard refuses (an upper off-block entry without its mirror), each followed by a good handle
whose products are exact; the two failures twenty times over and an exchange-form handle behind them;
and the one-shard multi handle, which matrix.py never builds.

The matrix: banded_mesh(100, links=3, dof=1) with sym_int_values -- integer data, every sum far below
2^24, compared by equality with the int64 product."""
import ctypes as C

import numpy as np
import pytest

import cfs_spmv_amd as cfs
from cfs_spmv_amd import _lib
from cfs_spmv_amd.matrix import _ptr, _stream_ptr
from rand_matrices import banded_mesh, sym_int_product, sym_int_values
from test_gpu_kernel_variants import PLAN_KNOBS

NO_CALIBRATE = 32
XMODES = (0, 1, 2)  # CFS_HIP_XMODE_PEER, _REPLICATE, _REPLICATE_ALL
_CASE = {}


@pytest.fixture(autouse=True)
def _torch_first(monkeypatch):
    """torch brings a HIP runtime of its own: it has to initialise before libcfs_hip.so's"""
    import torch
    assert torch.cuda.is_available()
    torch.cuda.init()
    torch.cuda.set_device(0)
    for k in PLAN_KNOBS + ("CFS_MULTI_EXCHANGE", "CFS_MULTI_TRANSPORT", "CFS_MULTI_X"):
        monkeypatch.delenv(k, raising=False)
    yield


def case():
    """(n, rowptr, colind, values, x, A x in int64) of the good matrix, and (rowptr, colind, values) of the
    refused one: the same without the upper entry (last row of block 1, first row of block 2) of the
    three-block cut -- block 1 then stores one entry above itself less than block 2 stores below it"""
    if not _CASE:
        n, rp, ci, _ = banded_mesh(100, links=3, dof=1)
        va, x = sym_int_values(np.random.default_rng(100), n, rp, ci)
        want = sym_int_product(n, rp, ci, va, x)
        rs = cfs.balanced_splits(n, rp, ci, 3)
        assert (np.diff(rs) > 0).all(), rs
        i, j = int(rs[2]) - 1, int(rs[2])
        k = np.flatnonzero(ci[rp[i]:rp[i + 1]] == j)
        assert k.size == 1, (rs, i, j)  # the band couples neighbouring rows
        k = int(rp[i] + k[0])
        rp2 = rp.copy()
        rp2[i + 1:] -= 1
        ci2, va2 = np.delete(ci, k), np.delete(va, k)
        assert np.array_equal(cfs.balanced_splits(n, rp2, ci2, 3), rs)  # (the cut did not move)
        _CASE["good"] = (n, rp, ci, va, x, want)
        _CASE["refused"] = (rp2, ci2, va2)
    return _CASE["good"], _CASE["refused"]


def opts(flags=0):
    return cfs.make_options(flags=NO_CALIBRATE | flags)


def last_error():
    return _lib.load().cfs_hip_last_error().decode(errors="replace")


def create_multi(n, rp, ci, va, ngpus, devices, options):
    """cfs_hip_sym_create_multi_f64 as the ABI has it: (code, message, handle)"""
    h = C.c_void_p()
    dv = np.ascontiguousarray(devices, dtype=np.int32) if devices is not None else None
    va = np.ascontiguousarray(va, dtype=np.float64)
    rc = _lib.load().cfs_hip_sym_create_multi_f64(n, rp.ctypes.data, ci.ctypes.data, va.ctypes.data, ngpus,
                                                  dv.ctypes.data if dv is not None else None, C.byref(options), C.byref(h))
    return rc, (last_error() if rc else ""), h


def bad_device_list():
    """[0, number of visible devices]: shard 0 is built, then the second entry is refused"""
    import torch
    (n, rp, ci, va, _, _), _ = case()
    rc, msg, h = create_multi(n, rp, ci, va, 2, [0, torch.cuda.device_count()], opts())
    assert (rc, msg, h.value) == (_lib.ERR_ARG, "bad device index", None)


def shard_refusal():
    """(code, message) of the first rank whose own create refuses the unsymmetric matrix; rank 0 builds"""
    if "refusal" not in _CASE:
        lib = _lib.load()
        (n, _, _, _, _, _), (rp, ci, va) = case()
        rs = cfs.balanced_splits(n, rp, ci, 3)
        own = []
        for rank in range(3):
            h, o = C.c_void_p(), opts()
            rc = lib.cfs_hip_sym_create_shard_f64(n, rp.ctypes.data, ci.ctypes.data, va.ctypes.data, 3, rank,
                                                  rs.ctypes.data, C.byref(o), C.byref(h))
            own.append((rc, last_error() if rc else ""))
            if rc == 0:
                _lib.check(lib.cfs_hip_sym_destroy(h))
        refusing = [r for r in range(3) if own[r][0] != 0]
        assert own[0][0] == 0 and refusing and refusing[0] >= 1, own  # (what the input has to be)
        _CASE["refusal"] = own[refusing[0]]
    return _CASE["refusal"]


def refused_shard():
    """the unsymmetric matrix on three shards of device 0: shard 0 is built, and the first shard that
    refuses speaks for the whole handle, in its own words"""
    (n, _, _, _, _, _), (rp, ci, va) = case()
    own = shard_refusal()
    rc, msg, h = create_multi(n, rp, ci, va, 3, [0, 0, 0], opts())
    assert (rc, msg) == own and h.value is None, (rc, msg, own)


def exact_product(A, xmodes=(None,)):
    import torch
    (n, _, _, _, x, want), _ = case()
    xd = torch.from_numpy(x).cuda()
    for xmode in xmodes:
        if xmode is not None:
            _lib.check(_lib.load().cfs_hip_sym_multi_set_xmode(A._h, xmode))
        yd = torch.full((n,), float("nan"), dtype=torch.float64, device="cuda")
        A.dense_vector_multiply(yd, xd)
        torch.cuda.synchronize()
        assert np.array_equal(yd.cpu().numpy(), want.astype(np.float64)), xmode


def good_handle(flags=0, ngpus=2):
    (n, rp, ci, va, _, _), _ = case()
    return cfs.SymMatrix(n, rp, ci, va, ngpus=ngpus, options=opts(flags))


@pytest.mark.gpu
def test_device_list_with_an_entry_out_of_range():
    bad_device_list()
    A = good_handle()
    exact_product(A, XMODES)
    A.close()


@pytest.mark.gpu
def test_matrix_that_a_later_shard_refuses():
    refused_shard()
    A = good_handle(ngpus=3)
    exact_product(A, XMODES)
    A.close()


@pytest.mark.gpu
def test_twenty_failed_creates_then_an_exchange_form_handle():
    """a teardown that frees something twice or leaves a stream behind shows in the handle built after
    it: an error return, or a wrong product"""
    for _ in range(20):
        bad_device_list()
        refused_shard()
    A = good_handle(cfs.FLAG_SHARD_EXCHANGE, ngpus=3)
    A.set_exchange("sparse")
    assert A.exchange_info()["form"] == cfs.EXCHANGE_SPARSE
    exact_product(A)
    A.close()


@pytest.mark.gpu
def test_multi_handle_of_one_shard():
    """ngpus = 1 through the ABI: a multi-device handle of one mirrored shard, never an exchange form"""
    import torch
    lib = _lib.load()
    (n, rp, ci, va, x, want), _ = case()
    rc, msg, h = create_multi(n, rp, ci, va, 1, None, opts(cfs.FLAG_SHARD_EXCHANGE))
    assert rc == 0 and h.value, (rc, msg)
    k = C.c_int(-1)
    _lib.check(lib.cfs_hip_sym_num_gpus(h, C.byref(k)))
    assert k.value == 1
    xd = torch.from_numpy(x).cuda()
    yd = torch.full((n,), float("nan"), dtype=torch.float64, device="cuda")
    _lib.check(lib.cfs_hip_sym_spmv_async(h, _ptr(yd), _ptr(xd), _stream_ptr()))
    torch.cuda.synchronize()
    assert np.array_equal(yd.cpu().numpy(), want.astype(np.float64))
    for form in (cfs.EXCHANGE_REDUCE_SCATTER, cfs.EXCHANGE_SPARSE):
        assert lib.cfs_hip_sym_multi_set_exchange(h, form) == _lib.ERR_ARG
    _lib.check(lib.cfs_hip_sym_destroy(h))
