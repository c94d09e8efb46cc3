"""The SPARSE form of the native exchange: the packed all-to-all cfs_hip_comm_alltoallv (a pull kernel on
the peer transport, grouped ncclSend / ncclRecv on RCCL) and the multi-device handle that uses it
(cfs_hip_sym_multi_set_exchange, CFS_MULTI_EXCHANGE=sparse): tiles, pack, ONE collective that moves one
value per remote boundary row, local fold, fold of what arrived -- no zeroed dense vector, no scatter,
no add.

On a one-GPU box, as tests/test_gpu_comm.py: the ranks share cuda:0 (peer transport), and the RCCL
transport runs with ONE rank, where the only block is the self block.

Bounds: the product of a sparse-form handle is held to what tests/test_gpu_comm.py holds the dense form
to for the same matrices, 1e-12 (fp64) / 1e-5 (fp32) of conftest.scaled_err against the long-double
oracle; the primitive only moves values, so what arrives is compared bit for bit."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import cfs_spmv_amd as cfs
from cfs_spmv_amd import _lib, synth
from conftest import scaled_err
from test_gpu_kernel_variants import PLAN_KNOBS

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL = {np.float64: 1e-12, np.float32: 1e-5}
AUTO, RCCL, PEER = 0, 1, 2
NO_CALIBRATE = 32
DTYPES = pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])


@pytest.fixture(autouse=True)
def _torch_first(monkeypatch):
    """torch brings a HIP runtime of its own: it has to initialise before libcfs_hip.so's"""
    import torch
    assert torch.cuda.is_available()
    torch.cuda.init()
    torch.cuda.set_device(0)
    for k in PLAN_KNOBS + ("CFS_HIP_CG_GRAPH", "CFS_MULTI_EXCHANGE", "CFS_MULTI_TRANSPORT", "CFS_MULTI_X"):
        monkeypatch.delenv(k, raising=False)
    yield


# ---------------------------------------------------------------------------------------------------
# 1. the primitive
# ---------------------------------------------------------------------------------------------------
def counts_matrix(nranks, rng, rnd):
    """counts[g, r] = values rank g hands to rank r, with: zeros, a rank that sends nothing (a zero row),
    a rank that receives nothing (a zero column) and a non-zero self block.
    N >= 3 has room for all four in every matrix.  N = 2 has not: a zero row and a zero column leave ONE
    entry, so the three rounds take the three placements in turn (round 0: the self block [0, 0]; rounds
    1 and 2: the two cross blocks) and every matrix still has its zeros, its silent sender and its silent
    receiver.  N = 1: the self block is the only block."""
    if nranks == 1:
        return np.array([[int(rng.integers(100, 3000))]], dtype=np.int64)
    c = rng.integers(1, 3000, (nranks, nranks)).astype(np.int64)
    c[rng.uniform(size=c.shape) < 0.3] = 0
    if nranks == 2:
        silent, deaf = ((1, 1), (0, 1), (1, 0))[rnd % 3]
        keep = None
    else:
        silent, deaf = (int(v) for v in rng.choice(nranks, 2, replace=False))
        keep = next(q for q in range(nranks) if q not in (silent, deaf))
        c[keep, keep] = int(rng.integers(1, 3000))  # the self block
        other = next((q for q in range(nranks) if q not in (silent, deaf, keep)), None)
        if other is not None:
            c[keep, other] = 0  # a zero that is neither in the silent row nor in the deaf column
    c[silent, :] = 0
    c[:, deaf] = 0
    if nranks == 2:
        g, r = 1 - silent, 1 - deaf
        c[g, r] = max(1, c[g, r])
    assert (c == 0).any() and not c[silent].any() and not c[:, deaf].any()
    assert c.sum() > 0 and (nranks == 2 or c[keep, keep] > 0)
    return c


@pytest.mark.parametrize("transport,nranks", [(PEER, 2), (PEER, 4), (AUTO, 3), (RCCL, 1)])
@DTYPES
def test_alltoallv_delivers_every_block_bit_for_bit(transport, nranks, dtype):
    import torch
    lib = _lib.load()
    comm = C.c_void_p()
    devs = (C.c_int * nranks)(*([0] * nranks))
    _lib.check(lib.cfs_hip_comm_create(nranks, devs, transport, C.byref(comm)))
    nd, tr = C.c_int(), C.c_int()
    _lib.check(lib.cfs_hip_comm_info(comm, C.byref(nd), C.byref(tr)))
    assert nd.value == nranks
    assert tr.value == (RCCL if nranks == 1 else PEER)
    tdt = torch.float64 if dtype == np.float64 else torch.float32
    vb = np.dtype(dtype).itemsize
    rng = np.random.default_rng(1000 * nranks + vb)
    streams = [torch.cuda.Stream() for _ in range(nranks)]
    sp = (C.c_void_p * nranks)(*[s.cuda_stream for s in streams])
    GUARD = 64  # values behind the received total that must stay NaN
    cap = 3000 * nranks + GUARD
    # one send / receive buffer per rank for all rounds: the buffers are REUSED (wait_consumed)
    send = [torch.zeros(cap, dtype=tdt, device="cuda") for _ in range(nranks)]
    recv = [torch.zeros(cap, dtype=tdt, device="cuda") for _ in range(nranks)]
    seen_self = seen_cross = False
    torch.cuda.synchronize()
    for rnd in range(3):
        cnt = counts_matrix(nranks, rng, rnd)
        seen_self |= bool(np.diag(cnt).any())
        seen_cross |= bool((cnt - np.diag(np.diag(cnt))).any())
        out_tot, in_tot = cnt.sum(axis=1), cnt.sum(axis=0)
        send_h = [rng.uniform(-1, 1, int(out_tot[g])).astype(dtype) for g in range(nranks)]
        for g in range(nranks):
            _lib.check(lib.cfs_hip_comm_wait_consumed(comm, g, sp[g]))
            with torch.cuda.stream(streams[g]):
                send[g][:int(out_tot[g])].copy_(torch.from_numpy(send_h[g]), non_blocking=False)
                recv[g].fill_(float("nan"))
        # (a rank that moves nothing hands NULL over)
        sptr = (C.c_void_p * nranks)(*[send[g].data_ptr() if out_tot[g] else None for g in range(nranks)])
        rptr = (C.c_void_p * nranks)(*[recv[g].data_ptr() if in_tot[g] else None for g in range(nranks)])
        cc = np.ascontiguousarray(cnt.reshape(-1))
        _lib.check(lib.cfs_hip_comm_alltoallv(comm, sptr, rptr, cc.ctypes.data, vb, sp))
        torch.cuda.synchronize()
        off = np.concatenate([np.zeros((nranks, 1), np.int64), np.cumsum(cnt, axis=1)], axis=1)
        for r in range(nranks):
            want = np.concatenate([send_h[g][off[g, r]:off[g, r + 1]] for g in range(nranks)] + [np.zeros(0, dtype)])
            got = recv[r].cpu().numpy()
            assert want.size == in_tot[r]
            assert np.array_equal(got[:want.size].view(np.uint8), want.view(np.uint8)), (rnd, r, cnt)
            assert np.isnan(got[want.size:]).all(), (rnd, r)  # nothing written behind the total
    assert seen_self and (seen_cross or nranks == 1)
    _lib.check(lib.cfs_hip_comm_destroy(comm))


def test_alltoallv_argument_checks_on_a_live_communicator():
    import torch
    lib = _lib.load()
    comm = C.c_void_p()
    _lib.check(lib.cfs_hip_comm_create(2, (C.c_int * 2)(0, 0), PEER, C.byref(comm)))
    buf = [torch.zeros(8, dtype=torch.float64, device="cuda") for _ in range(2)]
    ptr = (C.c_void_p * 2)(*[b.data_ptr() for b in buf])
    st = (C.c_void_p * 2)(*([torch.cuda.current_stream().cuda_stream] * 2))
    ok = np.array([0, 1, 2, 0], np.int64)
    for cnt, send, recv, vb in ((ok, ptr, ptr, 2), (np.array([0, -1, 0, 0], np.int64), ptr, ptr, 8),
                                (ok, (C.c_void_p * 2)(None, buf[1].data_ptr()), ptr, 8),
                                (ok, ptr, (C.c_void_p * 2)(None, buf[1].data_ptr()), 8)):
        assert lib.cfs_hip_comm_alltoallv(comm, send, recv, cnt.ctypes.data, vb, st) == _lib.ERR_ARG
    _lib.check(lib.cfs_hip_comm_destroy(comm))


def test_rccl_transport_still_refuses_two_ranks_on_one_device():
    comm = C.c_void_p()
    rc = _lib.load().cfs_hip_comm_create(2, (C.c_int * 2)(0, 0), RCCL, C.byref(comm))
    assert rc == _lib.ERR_UNSUPPORTED
    assert b"one rank per device" in _lib.load().cfs_hip_last_error()


# ---------------------------------------------------------------------------------------------------
# 2.-4. the handle
# ---------------------------------------------------------------------------------------------------
def host_counts(n, rp, ci, va, nranks, flags=NO_CALIBRATE):
    """(counts[g, r], row_splits) of the exchange-form shards, host only"""
    rs = cfs.balanced_splits(n, rp, ci, nranks)
    cnt = np.zeros((nranks, nranks), np.int64)
    for g in range(nranks):
        c, rows = cfs.plan_send_info(n, rp, ci, va.astype(np.float64), nranks, g, rs, cfs.make_options(flags=flags))
        assert c.sum() == rows.size
        cnt[g] = c
    return cnt, rs


def _spmv_ok(A, xd, n, y_ld, absrow, dtype, garbage, what):
    import torch
    yd = torch.full((n,), garbage, dtype=xd.dtype, device="cuda")
    A.dense_vector_multiply(yd, xd)
    torch.cuda.synchronize()
    e = scaled_err(yd.cpu().numpy(), y_ld, absrow)
    print(f"sparse-exchange {np.dtype(dtype).name} {what} y0={garbage} err={e:.3e} bound={TOL[dtype]:.0e}")
    assert e <= TOL[dtype], (what, garbage, e)


@pytest.mark.parametrize("ngpus", [2, 3, 8])
@DTYPES
def test_multi_device_handle_sparse_form(ngpus, dtype):
    from oracle import oracle
    import torch
    n, rp, ci, va, _ = synth.generate("Flan_1565", 0.03)
    va = va.astype(dtype)
    x = synth.make_x(n, 42, dtype)
    A = cfs.SymMatrix(n, rp, ci, va, ngpus=ngpus, options=cfs.make_options(flags=cfs.FLAG_SHARD_EXCHANGE | NO_CALIBRATE))
    y_ld, absrow = oracle.csr_spmv_ld(n, rp, ci, va, x)
    xd = torch.from_numpy(x).cuda()
    vb = np.dtype(dtype).itemsize
    cnt, rs = host_counts(n, rp, ci, va, ngpus)
    dense_values = ngpus * ngpus * int(np.max(np.diff(rs)))
    # the flag alone still means the reduce-scatter form
    assert A.exchange_info() == {"form": cfs.EXCHANGE_REDUCE_SCATTER, "values_moved": dense_values,
                                 "bytes_moved": dense_values * vb}
    A.set_exchange("sparse")
    info = A.exchange_info()
    print(f"sparse-exchange {np.dtype(dtype).name} N={ngpus}: sparse moves {info['values_moved']} values, dense {dense_values}")
    assert info == {"form": cfs.EXCHANGE_SPARSE, "values_moved": int(cnt.sum()), "bytes_moved": int(cnt.sum()) * vb}
    assert cnt.sum() > 0
    for garbage in (7.0, -1.0, float("nan")):
        _spmv_ok(A, xd, n, y_ld, absrow, dtype, garbage, f"N={ngpus} sparse")
    # with replicated x and local y blocks on top (the copy path of a multi-GPU node)
    _lib.check(_lib.load().cfs_hip_sym_multi_set_xmode(A._h, 2))
    for garbage in (7.0, -1.0, float("nan")):
        _spmv_ok(A, xd, n, y_ld, absrow, dtype, garbage, f"N={ngpus} sparse, xmode 2")
    # and back: the dense form of the same handle, the same bound
    A.set_exchange("reduce_scatter")
    assert A.exchange_info()["form"] == cfs.EXCHANGE_REDUCE_SCATTER and A.exchange_info()["values_moved"] == dense_values
    for garbage in (7.0, -1.0, float("nan")):
        _spmv_ok(A, xd, n, y_ld, absrow, dtype, garbage, f"N={ngpus} back to reduce-scatter, xmode 2")
    A.set_exchange(cfs.EXCHANGE_SPARSE)  # a second switch builds nothing anew
    _spmv_ok(A, xd, n, y_ld, absrow, dtype, float("nan"), f"N={ngpus} sparse again")
    A.close()


def test_non_neighbour_traffic_on_a_matrix_without_a_band():
    """the power-law stand-in in 8 row blocks: every block sends to EVERY lower block (hub columns), so
    the all-to-all is not a neighbour exchange"""
    from oracle import oracle
    import torch
    dtype, N = np.float64, 8
    n, rp, ci, va, _ = synth.generate("powerlaw", 0.02)
    cnt, rs = host_counts(n, rp, ci, va, N)
    far = [(g, r, int(cnt[g, r])) for g in range(N) for r in range(N) if g - r >= 2 and cnt[g, r] > 0]
    assert far, cnt
    assert not np.triu(cnt).any()  # contributions only go to lower ranks
    x = synth.make_x(n, 42, dtype)
    y_ld, absrow = oracle.csr_spmv_ld(n, rp, ci, va, x)
    A = cfs.SymMatrix(n, rp, ci, va, ngpus=N, options=cfs.make_options(flags=cfs.FLAG_SHARD_EXCHANGE | NO_CALIBRATE))
    A.set_exchange("sparse")
    assert A.exchange_info()["values_moved"] == int(cnt.sum())
    xd = torch.from_numpy(x).cuda()
    for garbage in (7.0, -1.0, float("nan")):
        _spmv_ok(A, xd, n, y_ld, absrow, dtype, garbage, f"powerlaw N={N} sparse ({len(far)} non-neighbour blocks)")
    A.close()


@DTYPES
def test_environment_selects_the_sparse_form(dtype, monkeypatch):
    from oracle import oracle
    import torch
    monkeypatch.setenv("CFS_MULTI_EXCHANGE", "sparse")  # read at create
    n, rp, ci, va, _ = synth.generate("Flan_1565", 0.03)
    va = va.astype(dtype)
    x = synth.make_x(n, 42, dtype)
    A = cfs.SymMatrix(n, rp, ci, va, ngpus=4, options=cfs.make_options(flags=NO_CALIBRATE))  # no exchange flag
    monkeypatch.delenv("CFS_MULTI_EXCHANGE")
    cnt, _ = host_counts(n, rp, ci, va, 4)
    info = A.exchange_info()
    assert info["form"] == cfs.EXCHANGE_SPARSE and info["values_moved"] == int(cnt.sum())
    y_ld, absrow = oracle.csr_spmv_ld(n, rp, ci, va, x)
    _spmv_ok(A, torch.from_numpy(x).cuda(), n, y_ld, absrow, dtype, float("nan"), "CFS_MULTI_EXCHANGE=sparse N=4")
    A.close()


def test_cxx_drivers_with_the_sparse_exchange(tmp_path):
    """the reference's self-check and bench drivers, unmodified command line, CFS_NUM_GPUS=4
    CFS_MULTI_EXCHANGE=sparse (four shards on the one visible device): the variable is read in the library"""
    n, rp, ci, va, _ = synth.generate("ldoor", 0.05)
    p = str(tmp_path / "ldoor_like.mtx")
    synth.write_mtx(p, n, rp, ci, va)
    env = dict(os.environ, CFS_SEED="11", CFS_NUM_GPUS="4", CFS_MULTI_EXCHANGE="sparse")
    r = subprocess.run([os.path.join(ROOT, "build", "test_spmv_mmf"), p, "1"], capture_output=True, text=True, env=env,
                       timeout=300)
    assert r.returncode == 0 and "PASSED!" in r.stdout, r.stdout + r.stderr
    r = subprocess.run([os.path.join(ROOT, "build", "bench_spmv_mmf"), p, "1", "32"], capture_output=True, text=True,
                       env=env, timeout=300)
    assert r.returncode == 0 and "gpus: 4" in r.stdout, r.stdout + r.stderr


def test_set_exchange_refuses_what_has_no_exchange():
    n, rp, ci, va, _ = synth.generate("pwtk", 0.02)
    lib = _lib.load()
    rs = cfs.balanced_splits(n, rp, ci, 2)
    handles = {"mirrored multi": cfs.SymMatrix(n, rp, ci, va, ngpus=2, options=cfs.make_options(flags=NO_CALIBRATE)),
               "plain": cfs.SymMatrix(n, rp, ci, va, options=cfs.make_options(flags=NO_CALIBRATE)),
               "shard": cfs.SymMatrix(n, rp, ci, va, row_splits=rs, rank=1,
                                      options=cfs.make_options(flags=NO_CALIBRATE | cfs.FLAG_SHARD_EXCHANGE))}
    for what, A in handles.items():
        for form in (cfs.EXCHANGE_SPARSE, cfs.EXCHANGE_REDUCE_SCATTER):
            assert lib.cfs_hip_sym_multi_set_exchange(A._h, form) == _lib.ERR_ARG, what
            assert b"not an exchange-form multi-device handle" in lib.cfs_hip_last_error()
        with pytest.raises(_lib.CfsHipError):
            A.exchange_info()
        A.close()
    E = cfs.SymMatrix(n, rp, ci, va, ngpus=2, options=cfs.make_options(flags=NO_CALIBRATE | cfs.FLAG_SHARD_EXCHANGE))
    assert lib.cfs_hip_sym_multi_set_exchange(E._h, 2) == _lib.ERR_ARG
    assert b"unknown exchange form" in lib.cfs_hip_last_error()
    with pytest.raises(ValueError):
        E.set_exchange("dense")
    assert E.exchange_info()["form"] == cfs.EXCHANGE_REDUCE_SCATTER
    E.close()


# ---------------------------------------------------------------------------------------------------
# 5. native CG and Jacobi PCG through a sparse-form handle
# ---------------------------------------------------------------------------------------------------
@DTYPES
@pytest.mark.parametrize("solver", ["cg", "pcg"])
def test_native_solvers_on_an_eight_shard_sparse_handle(solver, dtype):
    """what tests/test_gpu_cg_steps.py and tests/test_gpu_pcg_steps.py assert of a one-device handle of the
    pwtk stand-in: the iterates against the long-double recurrence (4 d_k + 16 u), the reported residual
    against the long-double one (their slack), convergence to 10 tol"""
    import torch
    import test_gpu_cg_steps as tc
    import test_gpu_pcg_steps as tp
    n, rp, ci, va = tc._matrix("pwtk@0.05")
    b = tc._rhs(n, dtype)
    if solver == "cg":
        va, native, check = va.astype(dtype), tc._native, tc._check_iterates
    else:
        va, native, check = tp.scaled(n, rp, ci, va, dtype), tp._native, tp._check_iterates
    A = cfs.SymMatrix(n, rp, ci, va, ngpus=8, options=cfs.make_options(flags=cfs.FLAG_SHARD_EXCHANGE | NO_CALIBRATE))
    A.set_exchange("sparse")
    assert A.exchange_info()["form"] == cfs.EXCHANGE_SPARSE and A.exchange_info()["values_moved"] > 0
    check("pwtk@0.05", n, rp, ci, va, b, dtype, lambda k: native(A, b, torch, tol=0.0, maxiter=k)[:2],
          label=" (8 shards, sparse exchange)")
    for check_every, k in ((1, 7), (16, 23)):
        u, it, res = native(A, b, torch, tol=0.0, maxiter=k, check_every=check_every)
        assert it == k, (check_every, k, it)
        true, slack = tc._true_relres(n, rp, ci, va, b, u, dtype)
        print(f"sparse-exchange {solver} {np.dtype(dtype).name} relres k={k} reported={res:.6e} long double={true:.6e} slack={slack:.3e}")
        assert abs(res - true) <= slack, (k, res, true, slack)
    tol = 1e-10 if dtype == np.float64 else 1e-5
    us, its, ress = native(A, b, torch, tol=tol, maxiter=500)
    true, slack = tc._true_relres(n, rp, ci, va, b, us, dtype)
    print(f"sparse-exchange {solver} {np.dtype(dtype).name} tol={tol}: {its} iterations, relres {ress:.3e} (long double {true:.3e})")
    assert 0 < its < 500 and ress <= 10 * tol and abs(ress - true) <= slack
    assert A.exchange_info()["form"] == cfs.EXCHANGE_SPARSE
    A.close()


# ---------------------------------------------------------------------------------------------------
# 6. a box without RCCL
# ---------------------------------------------------------------------------------------------------
CHILD = r"""
import ctypes as C, sys
import numpy as np
import torch
torch.cuda.init(); torch.cuda.set_device(0)
from cfs_spmv_amd import _lib
lib = _lib.load()
AUTO, RCCL, PEER = 0, 1, 2
comm = C.c_void_p()
rc = lib.cfs_hip_comm_create(1, (C.c_int * 1)(0), RCCL, C.byref(comm))
msg = lib.cfs_hip_last_error()
assert rc == _lib.ERR_UNSUPPORTED and b"not loadable" in msg, (rc, msg)
_lib.check(lib.cfs_hip_comm_create(1, (C.c_int * 1)(0), AUTO, C.byref(comm)))  # distinct devices: RCCL if it loaded
nd, tr = C.c_int(), C.c_int()
_lib.check(lib.cfs_hip_comm_info(comm, C.byref(nd), C.byref(tr)))
assert (nd.value, tr.value) == (1, PEER), (nd.value, tr.value)
_lib.check(lib.cfs_hip_comm_destroy(comm))
_lib.check(lib.cfs_hip_comm_create(2, (C.c_int * 2)(0, 0), AUTO, C.byref(comm)))
_lib.check(lib.cfs_hip_comm_info(comm, C.byref(nd), C.byref(tr)))
assert (nd.value, tr.value) == (2, PEER)
cnt = np.array([3, 5, 7, 0], np.int64)
send_h = [np.arange(8, dtype=np.float64) + 1, np.arange(7, dtype=np.float64) + 101]
send = [torch.from_numpy(s).cuda() for s in send_h]
recv = [torch.full((16,), float("nan"), dtype=torch.float64, device="cuda") for _ in range(2)]
streams = [torch.cuda.Stream() for _ in range(2)]
sp = (C.c_void_p * 2)(*[s.cuda_stream for s in streams])
torch.cuda.synchronize()
_lib.check(lib.cfs_hip_comm_alltoallv(comm, (C.c_void_p * 2)(*[t.data_ptr() for t in send]),
                                      (C.c_void_p * 2)(*[t.data_ptr() for t in recv]), cnt.ctypes.data, 8, sp))
torch.cuda.synchronize()
want = [np.concatenate([send_h[0][:3], send_h[1][:7]]), send_h[0][3:8]]
for r in range(2):
    got = recv[r].cpu().numpy()
    assert np.array_equal(got[:want[r].size], want[r]) and np.isnan(got[want[r].size:]).all(), (r, got)
_lib.check(lib.cfs_hip_comm_destroy(comm))
print("CHILD-OK")
"""


def test_loader_falls_back_to_the_peer_transport_without_rccl(tmp_path):
    """CFS_HIP_RCCL_LIB names a file that does not exist: AUTO yields the peer transport instead of ending
    the process, RCCL is CFS_HIP_ERR_UNSUPPORTED with the loader's message, the all-to-all works.  In a
    fresh process: the loader runs once per process."""
    env = dict(os.environ)
    env["CFS_HIP_RCCL_LIB"] = str(tmp_path / "no_such_librccl.so")
    env["PYTHONPATH"] = ROOT + os.pathsep + env.get("PYTHONPATH", "")
    p = subprocess.run([sys.executable, "-c", CHILD], env=env, cwd=ROOT, timeout=300, capture_output=True, text=True)
    print(p.stdout[-2000:], p.stderr[-2000:])
    assert p.returncode == 0, (p.returncode, p.stderr[-2000:])
    assert "CHILD-OK" in p.stdout
