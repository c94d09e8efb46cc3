"""The three collectives of the native exchange (cfs_hip_comm_reduce_scatter / _allgather / _alltoallv) at
their edges, and the event protocol of the peer transport under streams that are NOT idle.

Shapes: counts around one block of 256 and at the first second grid stride (the kernels cap their grid
at 2048 blocks of 256), every receive buffer inside a larger allocation whose 64 guard values on each
side must keep their bits, every case once more with all pointers advanced by one value.  The sum of the
peer reduce-scatter is the sequential sum in rank order from V(0) in the value type, so it is compared
bit for bit with that sum in numpy; the other two move bits and are compared as bytes.

Protocol (PEER, ranks sharing cuda:0): a stream is held back by a timed torch.cuda._sleep, so a call is
made while its predecessors have not run.  What the tests pin, as include/cfs_hip.h states it:
  * the host tables (send, recv, counts) are read before a call returns, and a call returns at once;
  * a send buffer may be overwritten on its rank's stream behind cfs_hip_comm_wait_consumed;
  * what a rank enqueued on its own stream before a call is ordered before that call's writes to the
    rank's buffers (the all-gather pushes into OTHER ranks' receive buffers);
  * the ready / done events are shared by the three collectives: mixed sequences, no synchronisation.
tests/test_gpu_comm.py and tests/test_gpu_sparse_exchange.py hold the same calls at ordinary sizes."""
import ctypes as C
import itertools
import time

import numpy as np
import pytest

from cfs_spmv_amd import _lib
from test_gpu_kernel_variants import PLAN_KNOBS

pytestmark = pytest.mark.gpu
AUTO, RCCL, PEER = 0, 1, 2
GUARD = 64
BIG = 2048 * 256  # one full grid: element BIG is the first a thread reaches in its second stride
SMALL_COUNTS = (0, 1, 255, 256, 257)
UINT = {np.float64: np.uint64, np.float32: np.uint32}
SENTINEL = {np.float64: 0xA5C3A5C3A5C3A5C3, np.float32: 0xA5C3A5C3}  # (finite, negative, in no payload)
DTYPES = pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
CONFIGS = [(PEER, 2), (PEER, 3), (PEER, 8), (RCCL, 1)]


def _cases():
    """(transport, nranks, count): the small counts everywhere, the two large ones with 2 ranks only"""
    out = [(t, n, c) for (t, n) in CONFIGS for c in SMALL_COUNTS]
    out += [(PEER, 2, BIG), (PEER, 2, BIG + 1)]
    return out


CASES = pytest.mark.parametrize("transport,nranks,count", _cases(),
                                ids=[f"{'peer' if t == PEER else 'rccl'}{n}-{c}" for (t, n, c) in _cases()])


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
# communicators (one per transport and size for the whole module: the events of a communicator live
# through every case, which is how a handle uses them), guarded buffers, payloads
# ---------------------------------------------------------------------------------------------------
class Comm:
    def __init__(self, transport, nranks):
        import torch
        self.lib = _lib.load()
        self.n = nranks
        self.h = C.c_void_p()
        _lib.check(self.lib.cfs_hip_comm_create(nranks, (C.c_int * nranks)(*([0] * nranks)), transport, C.byref(self.h)))
        nd, tr = C.c_int(), C.c_int()
        _lib.check(self.lib.cfs_hip_comm_info(self.h, C.byref(nd), C.byref(tr)))
        assert (nd.value, tr.value) == (nranks, transport)
        self.streams = [torch.cuda.Stream() for _ in range(nranks)]
        self.sp = (C.c_void_p * nranks)(*[s.cuda_stream for s in self.streams])

    def wait_consumed(self, g):
        _lib.check(self.lib.cfs_hip_comm_wait_consumed(self.h, g, self.sp[g]))

    def wait_consumed_all(self):
        for g in range(self.n):
            self.wait_consumed(g)

    def close(self):
        _lib.check(self.lib.cfs_hip_comm_destroy(self.h))


_COMMS = {}


@pytest.fixture(scope="module", autouse=True)
def _close_comms():
    yield
    import torch
    torch.cuda.synchronize()
    for c in _COMMS.values():
        c.close()
    _COMMS.clear()


def comm_of(transport, nranks):
    if (transport, nranks) not in _COMMS:
        _COMMS[(transport, nranks)] = Comm(transport, nranks)
    return _COMMS[(transport, nranks)]


def _tdt(dtype):
    import torch
    return torch.float64 if dtype == np.float64 else torch.float32


class Guarded:
    """`n` values inside a larger allocation: GUARD sentinel values, `shift` more, the payload, GUARD
    sentinel values.  ptr names the payload; with shift = 1 it is aligned to the value size only."""

    def __init__(self, n, dtype, shift, payload=None):
        import torch
        self.n, self.dtype, self.lo = int(n), dtype, GUARD + shift
        host = np.full(self.lo + self.n + GUARD, SENTINEL[dtype], UINT[dtype])
        if payload is not None:
            assert payload.dtype == dtype and payload.size == self.n
            host[self.lo:self.lo + self.n] = payload.view(UINT[dtype])
        self.before = host.copy()
        self.t = torch.from_numpy(host.view(dtype)).cuda()
        self.ptr = self.t.data_ptr() + self.lo * np.dtype(dtype).itemsize

    def bits(self):
        return self.t.cpu().numpy().view(UINT[self.dtype])

    def payload_bits(self):
        return self.bits()[self.lo:self.lo + self.n]

    def assert_guards(self, what):
        b = self.bits()
        assert np.array_equal(b[:self.lo], self.before[:self.lo]), f"{what}: values in front of the block changed"
        assert np.array_equal(b[self.lo + self.n:], self.before[self.lo + self.n:]), f"{what}: values behind the block changed"

    def assert_unchanged(self, what):
        assert np.array_equal(self.bits(), self.before), f"{what}: buffer changed"


def _voidp(values):
    return (C.c_void_p * len(values))(*[v if v else None for v in values])


def tiny(dtype):
    return np.finfo(dtype).tiny


def sum_payload(rng, dtype, nranks, count):
    """send[g] (nranks blocks of count values) for the reduce-scatter.  Random values in (-1, 1) and, at
    the first positions of every block: -0.0 in every rank (the sum is +0.0), a cancelling pair, +Inf,
    -Inf, one NaN, +Inf and -Inf together (NaN)."""
    send = [rng.uniform(-1, 1, nranks * count).astype(dtype) for _ in range(nranks)]
    for r in range(nranks):
        def put(k, g, v):
            if k < count:
                send[g][r * count + k] = v
        for g in range(nranks):
            put(0, g, -0.0)
        big = dtype(12345.678)
        put(1, 0, big)
        put(1, nranks - 1, -big if nranks > 1 else big)
        put(2, r % nranks, np.inf)
        put(3, (r + 1) % nranks, -np.inf)
        put(4, nranks - 1, np.nan)
        if nranks > 1:
            put(5, 0, np.inf)
            put(5, 1, -np.inf)
    return send


def sequential_sum(send, dtype, nranks, count, r):
    """what cfs_peer_sum_kernel computes for rank r: s = V(0); for g in rank order: s = s + in[g]"""
    s = np.zeros(count, dtype)
    with np.errstate(invalid="ignore"):
        for g in range(nranks):
            s = s + send[g][r * count:(r + 1) * count]
    assert s.dtype == dtype
    return s


def no_subnormals(a, dtype):
    a = np.abs(a[np.isfinite(a)])
    return not ((a > 0) & (a < tiny(dtype))).any()


def bit_payload(rng, dtype, n):
    """n values that only a bit-exact move keeps: random values, NaNs with distinct payload bits (quiet
    and signalling), -0.0, +-Inf, subnormals (the smallest, the largest, a random one)"""
    u = UINT[dtype]
    v = rng.uniform(-1, 1, n).astype(dtype)
    b = v.view(u)
    mant = 52 if dtype == np.float64 else 23
    expo = u((1 << (63 - mant if dtype == np.float64 else 31 - mant)) - 1) << u(mant)  # all exponent bits
    quiet = u(1) << u(mant - 1)
    special = [expo | quiet | u(k + 1) for k in range(3)]              # quiet NaNs, payloads 1..3
    special += [expo | u(0x155 + k) for k in range(2)]                 # signalling NaNs
    special += [(u(1) << u(8 * np.dtype(dtype).itemsize - 1)) | expo | quiet | u(7)]  # a negative NaN
    special += [u(1) << u(8 * np.dtype(dtype).itemsize - 1)]           # -0.0
    special += [expo, u(1), (u(1) << u(mant)) - u(1), u(int(rng.integers(2, 1 << 20)))]  # +Inf, subnormals
    for k, s in enumerate(special):
        if n:
            b[(k * 37) % n if n > len(special) else k % n] = s
    return v


def test_payload_generators_hold_what_they_promise():
    """(numpy only) the special values are really in the payloads, and no f32 subnormal is in a sum"""
    rng = np.random.default_rng(0)
    for dtype in (np.float64, np.float32):
        v = bit_payload(rng, dtype, 300)
        a = np.abs(v[np.isfinite(v)])
        assert np.isnan(v).sum() == 6 and np.isinf(v).sum() == 1 and ((a > 0) & (a < tiny(dtype))).sum() == 3
        assert np.signbit(v[v == 0]).all() and (v == 0).sum() == 1
        assert np.unique(v[np.isnan(v)].view(UINT[dtype])).size == 6
        for nranks, count in ((2, 257), (8, 255), (3, 1)):
            send = sum_payload(rng, dtype, nranks, count)
            for r in range(nranks):
                s = sequential_sum(send, dtype, nranks, count, r)
                assert no_subnormals(s, dtype) and all(no_subnormals(x, dtype) for x in send)
                assert s[0] == 0 and not np.signbit(s[0])
                if count > 5:
                    assert s[1] != 0 or nranks == 2
                    assert s[2] == np.inf and s[3] == -np.inf and np.isnan(s[4]) and np.isnan(s[5])


# ---------------------------------------------------------------------------------------------------
# 1. shapes
# ---------------------------------------------------------------------------------------------------
def run_reduce_scatter(c, dtype, count, shift, send_h, what):
    import torch
    vb = np.dtype(dtype).itemsize
    send = [Guarded(c.n * count, dtype, shift, send_h[g]) for g in range(c.n)]
    recv = [Guarded(count, dtype, shift) for _ in range(c.n)]
    torch.cuda.synchronize()
    c.wait_consumed_all()
    rc = c.lib.cfs_hip_comm_reduce_scatter(c.h, _voidp([s.ptr for s in send]), _voidp([r.ptr for r in recv]), count, vb, c.sp)
    assert rc == 0, (what, rc, c.lib.cfs_hip_last_error())
    torch.cuda.synchronize()
    for g in range(c.n):
        send[g].assert_unchanged(f"{what}: send[{g}]")
        recv[g].assert_guards(f"{what}: recv[{g}]")
    return [r.payload_bits().view(dtype) for r in recv]


@CASES
@DTYPES
def test_reduce_scatter_shapes(transport, nranks, count, dtype):
    c = comm_of(transport, nranks)
    for shift in (0, 1):
        rng = np.random.default_rng(count * 8 + nranks)
        send_h = sum_payload(rng, dtype, nranks, count)
        what = f"reduce_scatter N={nranks} count={count} shift={shift}"
        got = run_reduce_scatter(c, dtype, count, shift, send_h, what)
        for r in range(nranks):
            if transport == RCCL:  # one rank: a copy
                assert np.array_equal(got[r].view(UINT[dtype]), send_h[r].view(UINT[dtype])), what
                continue
            ref = sequential_sum(send_h, dtype, nranks, count, r)
            assert no_subnormals(ref, dtype)
            nan = np.isnan(ref)
            assert np.array_equal(np.isnan(got[r]), nan), (what, r)
            bad = np.flatnonzero((got[r].view(UINT[dtype]) != ref.view(UINT[dtype])) & ~nan)
            assert bad.size == 0, (what, r, bad[:8], got[r][bad[:8]], ref[bad[:8]])
            if count:
                assert got[r].view(UINT[dtype])[0] == 0, (what, r)  # -0.0 in every rank sums to +0.0
        if count == 0:  # an empty call leaves the communicator usable
            got = run_reduce_scatter(c, dtype, 5, shift, sum_payload(rng, dtype, nranks, 5), what + " then count=5")
            assert all(g.size == 5 and not np.isnan(g[1]) for g in got)


@pytest.mark.parametrize("nranks", [2, 3, 8])
@DTYPES
def test_reduce_scatter_of_integers_is_the_int64_sum(nranks, dtype):
    c = comm_of(PEER, nranks)
    count = 257
    rng = np.random.default_rng(nranks)
    ints = [rng.integers(-(1 << 10), (1 << 10) + 1, nranks * count) for _ in range(nranks)]
    total = np.sum(np.stack(ints), axis=0, dtype=np.int64)
    got = run_reduce_scatter(c, dtype, count, 0, [a.astype(dtype) for a in ints], f"integers N={nranks}")
    for r in range(nranks):
        assert np.array_equal(got[r].astype(np.int64), total[r * count:(r + 1) * count]) and np.isfinite(got[r]).all()


@CASES
@DTYPES
def test_allgather_shapes(transport, nranks, count, dtype):
    import torch
    c = comm_of(transport, nranks)
    vb = np.dtype(dtype).itemsize
    for shift in (0, 1):
        rng = np.random.default_rng(count * 8 + nranks + 1)
        for n in ((0, 5) if count == 0 else (count,)):  # (an empty call, then a call that moves values)
            what = f"allgather N={nranks} count={n} shift={shift}"
            blk_h = [bit_payload(rng, dtype, n) for _ in range(nranks)]
            blk = [Guarded(n, dtype, shift, blk_h[g]) for g in range(nranks)]
            full = [Guarded(nranks * n, dtype, shift) for _ in range(nranks)]
            torch.cuda.synchronize()
            c.wait_consumed_all()
            rc = c.lib.cfs_hip_comm_allgather(c.h, _voidp([b.ptr for b in blk]), _voidp([f.ptr for f in full]), n, vb, c.sp)
            assert rc == 0, (what, rc, c.lib.cfs_hip_last_error())
            torch.cuda.synchronize()
            want = np.concatenate(blk_h + [np.zeros(0, dtype)]).view(np.uint8)
            for r in range(nranks):
                blk[r].assert_unchanged(f"{what}: send[{r}]")
                full[r].assert_guards(f"{what}: recv[{r}]")
                assert np.array_equal(full[r].payload_bits().view(np.uint8), want), (what, r)


def run_alltoallv(c, dtype, cnt, shift, rng, what, null_where_empty=False):
    """one all-to-all with the count matrix cnt[g, r] into guarded buffers; every received byte, every
    guard and every send buffer is checked"""
    import torch
    N, vb = c.n, np.dtype(dtype).itemsize
    cnt = np.ascontiguousarray(cnt, np.int64)
    assert cnt.shape == (N, N)
    out_tot, in_tot = cnt.sum(axis=1), cnt.sum(axis=0)
    send_h = [bit_payload(rng, dtype, int(out_tot[g])) for g in range(N)]
    send = [Guarded(out_tot[g], dtype, shift, send_h[g]) for g in range(N)]
    recv = [Guarded(in_tot[r], dtype, shift) for r in range(N)]
    sptr = [0 if (null_where_empty and not out_tot[g]) else send[g].ptr for g in range(N)]
    rptr = [0 if (null_where_empty and not in_tot[r]) else recv[r].ptr for r in range(N)]
    torch.cuda.synchronize()
    c.wait_consumed_all()
    rc = c.lib.cfs_hip_comm_alltoallv(c.h, _voidp(sptr), _voidp(rptr), cnt.ctypes.data, vb, c.sp)
    assert rc == 0, (what, rc, c.lib.cfs_hip_last_error())
    torch.cuda.synchronize()
    off = np.concatenate([np.zeros((N, 1), np.int64), np.cumsum(cnt, axis=1)], axis=1)
    for r in range(N):
        want = np.concatenate([send_h[g][off[g, r]:off[g, r + 1]] for g in range(N)] + [np.zeros(0, dtype)])
        assert want.size == in_tot[r]
        send[r].assert_unchanged(f"{what}: send[{r}]")
        recv[r].assert_guards(f"{what}: recv[{r}]")
        got = recv[r].payload_bits()
        bad = np.flatnonzero(got != want.view(UINT[dtype]))
        assert bad.size == 0, (what, r, bad[:8], cnt[:, r])


@CASES
@DTYPES
def test_alltoallv_shapes(transport, nranks, count, dtype):
    """every block `count` long: a receiver's total is nranks * count"""
    c = comm_of(transport, nranks)
    for shift in (0, 1):
        rng = np.random.default_rng(count * 8 + nranks + 2)
        what = f"alltoallv N={nranks} every block {count} shift={shift}"
        run_alltoallv(c, dtype, np.full((nranks, nranks), count), shift, rng, what)
        if count == 0:
            run_alltoallv(c, dtype, np.full((nranks, nranks), 5), shift, rng, what + " then 5")


def _a2a_matrices():
    """count matrices of 8 ranks at the edges of the pull kernel's search over `prefix`"""
    N = 8
    z = lambda: np.zeros((N, N), np.int64)
    out = [("all-zero", z(), True)]
    m = z()
    np.fill_diagonal(m, [3, 1, 256, 257, 0, 255, 2, 5])
    out.append(("self-blocks", m, True))
    for g, r in ((0, 0), (0, 7), (7, 0), (7, 7), (3, 5)):  # exactly one value in the whole matrix
        m = z()
        m[g, r] = 1
        out.append((f"one-value-{g}-{r}", m, True))
    for g in range(N):  # receiver 2: one non-empty source among empty ones
        m = z()
        m[g, 2] = 3 + g
        out.append((f"single-source-{g}", m, True))
    for g, h in itertools.combinations(range(N), 2):  # ... and every pair of non-empty sources
        m = z()
        m[g, 2], m[h, 2] = 1 + g, 2 + h
        out.append((f"pair-{g}-{h}", m, True))
    m = z()  # receiver 5: block boundaries exactly on element 256 and on element BIG of its buffer
    m[1, 5], m[2, 5], m[4, 5], m[7, 5] = 256, BIG - 256, 1, 3
    m[1, 0], m[6, 5] = 2, 0  # (source 1's block for 5 does not start its send buffer)
    out.append(("boundary-256-and-grid", m, False))
    m = z()  # receiver 0: a total of BIG + 1 from three sources, empty ones between
    m[0, 0], m[3, 0], m[7, 0] = 1, BIG - 1, 1
    out.append(("total-grid-plus-1", m, False))
    return out


A2A = _a2a_matrices()


def test_alltoallv_matrices_are_what_they_claim():
    """(numpy only)"""
    names = [n for n, _, _ in A2A]
    assert len(set(names)) == len(names) and sum(n.startswith("pair-") for n in names) == 28
    m = dict((n, m) for n, m, _ in A2A)
    assert not m["all-zero"].any() and m["total-grid-plus-1"][:, 0].sum() == BIG + 1
    p = np.cumsum(m["boundary-256-and-grid"][:, 5])
    assert 256 in p and BIG in p and p[-1] > BIG


@pytest.mark.parametrize("name,cnt,nulls", A2A, ids=[n for n, _, _ in A2A])
def test_alltoallv_count_matrices(name, cnt, nulls):
    c = comm_of(PEER, 8)
    big = cnt.sum() > 100000
    for dtype, shift in ((np.float64, 0), (np.float32, 1)) if big else itertools.product((np.float64, np.float32), (0, 1)):
        rng = np.random.default_rng(int(cnt.sum()) + shift)
        run_alltoallv(c, dtype, cnt, shift, rng, f"alltoallv {name} {np.dtype(dtype).name} shift={shift}", null_where_empty=nulls)


# ---------------------------------------------------------------------------------------------------
# 2. the protocol, with streams held back
# ---------------------------------------------------------------------------------------------------
_SLEEP = {}


def hold_cycles():
    """torch.cuda._sleep cycles for a delay of about 40 ms (never above 200 ms): 10^7 cycles are timed with
    events once per module (after a first call that pays for loading the kernel)"""
    import torch
    if not _SLEEP:
        s = torch.cuda.Stream()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        with torch.cuda.stream(s):
            torch.cuda._sleep(1000)
            e0.record()
            torch.cuda._sleep(10 ** 7)
            e1.record()
        e1.synchronize()
        ms = e0.elapsed_time(e1)
        assert ms > 0
        cycles = int(10 ** 7 * 40.0 / ms)
        _SLEEP.update(ms_per_1e7=ms, cycles=cycles, ms=cycles * ms / 10 ** 7)
        print(f"comm-edges: 10^7 sleep cycles = {ms:.2f} ms; holding with {cycles} cycles = {_SLEEP['ms']:.1f} ms")
        assert 30.0 <= _SLEEP["ms"] <= 50.0
    return _SLEEP["cycles"]


def hold(stream):
    import torch
    with torch.cuda.stream(stream):
        torch.cuda._sleep(hold_cycles())


def _dev(a, dtype):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).astype(dtype)).cuda()


def _ints(rng, n, dtype):
    return rng.integers(-1000, 1001, n).astype(dtype)


def _a2a_ref(cnt, send_h, r, dtype):
    N = cnt.shape[0]
    off = np.concatenate([np.zeros((N, 1), np.int64), np.cumsum(cnt, axis=1)], axis=1)
    return np.concatenate([send_h[g][off[g, r]:off[g, r + 1]] for g in range(N)] + [np.zeros(0, dtype)])


def _protocol_counts(N, rng, count):
    cnt = rng.integers(1, count + 1, (N, N)).astype(np.int64)
    cnt[0, N - 1] = count  # the held receiver reads a full block of rank 0
    cnt[1, 0] = 0
    return cnt


@pytest.mark.parametrize("collective", ["reduce_scatter", "allgather", "alltoallv"])
@DTYPES
def test_tables_are_read_before_the_call_returns(collective, dtype):
    """every stream is held, the call is made, the host arrays it was given are overwritten at once with
    decoys (live buffers of the same sizes holding other numbers; another count matrix): the results come
    from the original buffers, the decoys are untouched, and the call came back at once, while the streams
    were still held (host timers against the measured hold)"""
    import torch
    N, count, vb = 3, 300, np.dtype(dtype).itemsize
    c = comm_of(PEER, N)
    rng = np.random.default_rng(5)
    cnt = _protocol_counts(N, rng, count)
    cnt2 = np.ascontiguousarray(cnt.T[::-1, ::-1])  # (another valid matrix: no total exceeds N * count)
    cap = N * count
    send_h = [_ints(rng, cap, dtype) for _ in range(N)]
    send = [_dev(s, dtype) for s in send_h]
    recv = [torch.full((cap,), float("nan"), dtype=_tdt(dtype), device="cuda") for _ in range(N)]
    decoy_send = [_dev(_ints(rng, cap, dtype) + 5000, dtype) for _ in range(N)]
    decoy_recv = [torch.full((cap,), -7.0, dtype=_tdt(dtype), device="cuda") for _ in range(N)]
    sptr, rptr = _voidp([t.data_ptr() for t in send]), _voidp([t.data_ptr() for t in recv])
    cc = cnt.reshape(-1).copy()
    hold_cycles()
    torch.cuda.synchronize()
    c.wait_consumed_all()
    for s in c.streams:
        hold(s)
    t0 = time.perf_counter()
    if collective == "reduce_scatter":
        rc = c.lib.cfs_hip_comm_reduce_scatter(c.h, sptr, rptr, count, vb, c.sp)
    elif collective == "allgather":
        rc = c.lib.cfs_hip_comm_allgather(c.h, sptr, rptr, count, vb, c.sp)
    else:
        rc = c.lib.cfs_hip_comm_alltoallv(c.h, sptr, rptr, cc.ctypes.data, vb, c.sp)
    t1 = time.perf_counter()
    held = [not s.query() for s in c.streams]
    for g in range(N):  # the decoys, at once
        sptr[g], rptr[g] = decoy_send[g].data_ptr(), decoy_recv[g].data_ptr()
    cc[:] = cnt2.reshape(-1)
    torch.cuda.synchronize()
    print(f"comm-edges tables {collective} {np.dtype(dtype).name}: call took {(t1 - t0) * 1e3:.3f} ms with the streams "
          f"held for {_SLEEP['ms']:.1f} ms; still held when it returned: {held}")
    assert rc == 0
    for r in range(N):
        got = recv[r].cpu().numpy()
        if collective == "reduce_scatter":
            want = np.sum(np.stack([s[r * count:(r + 1) * count].astype(np.int64) for s in send_h]), axis=0)
        elif collective == "allgather":
            want = np.concatenate([s[:count] for s in send_h])
        else:
            want = _a2a_ref(cnt, send_h, r, dtype)
        assert np.array_equal(got[:want.size], want.astype(dtype)), (collective, r)
        assert np.isnan(got[want.size:]).all(), (collective, r)
        assert (decoy_recv[r].cpu().numpy() == -7.0).all(), (collective, r)
    assert all(held), f"{collective} blocked the host until the streams had drained ({(t1 - t0) * 1e3:.1f} ms)"
    # "returns at once": the host spent less than half the measured hold inside the call (a copy of a table
    # from pageable memory behind the event waits kept it there for 38 of 40 ms)
    assert (t1 - t0) * 1e3 < 0.5 * _SLEEP["ms"], f"{collective} kept the host for {(t1 - t0) * 1e3:.1f} ms of a {_SLEEP['ms']:.0f} ms hold"


@pytest.mark.parametrize("collective", ["reduce_scatter", "alltoallv"])
@DTYPES
def test_send_buffer_reuse_behind_wait_consumed(collective, dtype):
    """round 1 with the last rank's stream held, so its kernel has not read the others' send buffers yet;
    then every rank, on its own stream: wait_consumed, overwrite its send buffer, round 2 into other
    receive buffers.  Both rounds must be exact."""
    import torch
    N, count, vb = 3, 300, np.dtype(dtype).itemsize
    c = comm_of(PEER, N)
    rng = np.random.default_rng(6)
    cap = N * count
    cnts = [_protocol_counts(N, rng, count) for _ in range(2)]
    data_h = [[_ints(rng, cap, dtype) for _ in range(N)] for _ in range(2)]
    send = [_dev(data_h[0][g], dtype) for g in range(N)]
    fresh = [_dev(data_h[1][g], dtype) for g in range(N)]
    recv = [[torch.full((cap,), float("nan"), dtype=_tdt(dtype), device="cuda") for _ in range(N)] for _ in range(2)]
    sptr = _voidp([t.data_ptr() for t in send])

    def call(rnd):
        rptr = _voidp([t.data_ptr() for t in recv[rnd]])
        if collective == "reduce_scatter":
            return c.lib.cfs_hip_comm_reduce_scatter(c.h, sptr, rptr, count, vb, c.sp)
        return c.lib.cfs_hip_comm_alltoallv(c.h, sptr, rptr, cnts[rnd].reshape(-1).ctypes.data, vb, c.sp)

    hold_cycles()
    torch.cuda.synchronize()
    c.wait_consumed_all()
    hold(c.streams[N - 1])
    assert call(0) == 0
    held = None
    for g in range(N):
        c.wait_consumed(g)
        with torch.cuda.stream(c.streams[g]):
            send[g].copy_(fresh[g], non_blocking=True)
        if g == 0:
            held = not c.streams[0].query()
    assert call(1) == 0
    torch.cuda.synchronize()
    print(f"comm-edges reuse {collective} {np.dtype(dtype).name}: rank 0's overwrite still pending when enqueued: {held}")
    for rnd in range(2):
        for r in range(N):
            got = recv[rnd][r].cpu().numpy()
            if collective == "reduce_scatter":
                want = np.sum(np.stack([s[r * count:(r + 1) * count].astype(np.int64) for s in data_h[rnd]]), axis=0).astype(dtype)
            else:
                want = _a2a_ref(cnts[rnd], data_h[rnd], r, dtype)
            assert np.array_equal(got[:want.size], want), (collective, "round", rnd + 1, "rank", r)


@pytest.mark.parametrize("reader", [0, 2])
@DTYPES
def test_allgather_orders_its_pushes_behind_the_receivers_own_stream(reader, dtype):
    """round 1; then rank `reader`'s stream is held and a copy of its receive buffer is enqueued behind the
    hold; round 2 pushes new blocks into the same receive buffers while the other ranks' streams are
    free.  The copy must hold round 1: what a rank enqueued on its own stream before a call is ordered
    before that call's writes to the rank's buffers."""
    import torch
    N, count, vb = 3, 300, np.dtype(dtype).itemsize
    c = comm_of(PEER, N)
    rng = np.random.default_rng(7)
    blk_h = [[_ints(rng, count, dtype) for _ in range(N)] for _ in range(2)]
    blk = [[_dev(b, dtype) for b in blk_h[rnd]] for rnd in range(2)]
    full = [torch.full((N * count,), float("nan"), dtype=_tdt(dtype), device="cuda") for _ in range(N)]
    snap = torch.full((N * count,), float("nan"), dtype=_tdt(dtype), device="cuda")
    rptr = _voidp([t.data_ptr() for t in full])
    hold_cycles()
    torch.cuda.synchronize()
    c.wait_consumed_all()
    assert c.lib.cfs_hip_comm_allgather(c.h, _voidp([t.data_ptr() for t in blk[0]]), rptr, count, vb, c.sp) == 0
    hold(c.streams[reader])
    with torch.cuda.stream(c.streams[reader]):
        snap.copy_(full[reader], non_blocking=True)
    assert c.lib.cfs_hip_comm_allgather(c.h, _voidp([t.data_ptr() for t in blk[1]]), rptr, count, vb, c.sp) == 0
    held = not c.streams[reader].query()
    torch.cuda.synchronize()
    print(f"comm-edges allgather reader {reader} {np.dtype(dtype).name}: reader still held after round 2 was enqueued: {held}")
    assert np.array_equal(snap.cpu().numpy(), np.concatenate(blk_h[0])), f"rank {reader}: round 2 overtook the reader of round 1"
    for r in range(N):
        assert np.array_equal(full[r].cpu().numpy(), np.concatenate(blk_h[1])), r


@pytest.mark.parametrize("nranks", [3, 8])
@DTYPES
def test_mixed_sequences_on_one_communicator(nranks, dtype):
    """three rounds of reduce_scatter, alltoallv, allgather, reduce_scatter with ONE set of send buffers,
    overwritten behind wait_consumed before every step, one stream held at the start of every round, no
    synchronisation until the end: the ready / done events are shared by the collectives"""
    import torch
    N, count, vb = nranks, 300, np.dtype(dtype).itemsize
    c = comm_of(PEER, N)
    rng = np.random.default_rng(8 + N)
    cap = N * count
    steps = ["reduce_scatter", "alltoallv", "allgather", "reduce_scatter"] * 3
    data_h = [[_ints(rng, cap, dtype) for _ in range(N)] for _ in steps]
    data = [[_dev(a, dtype) for a in row] for row in data_h]
    cnts = [_protocol_counts(N, rng, count // 2) if s == "alltoallv" else None for s in steps]
    send = [torch.zeros(cap, dtype=_tdt(dtype), device="cuda") for _ in range(N)]
    recv = [[torch.full((cap,), float("nan"), dtype=_tdt(dtype), device="cuda") for _ in range(N)] for _ in steps]
    sptr = _voidp([t.data_ptr() for t in send])
    hold_cycles()
    torch.cuda.synchronize()
    for k, step in enumerate(steps):
        if k % 4 == 0:
            hold(c.streams[(k // 4) % N])
        for g in range(N):
            c.wait_consumed(g)
            with torch.cuda.stream(c.streams[g]):
                send[g].copy_(data[k][g], non_blocking=True)
        rptr = _voidp([t.data_ptr() for t in recv[k]])
        if step == "reduce_scatter":
            rc = c.lib.cfs_hip_comm_reduce_scatter(c.h, sptr, rptr, count, vb, c.sp)
        elif step == "allgather":
            rc = c.lib.cfs_hip_comm_allgather(c.h, sptr, rptr, count, vb, c.sp)
        else:
            rc = c.lib.cfs_hip_comm_alltoallv(c.h, sptr, rptr, cnts[k].reshape(-1).ctypes.data, vb, c.sp)
        assert rc == 0, (k, step)
    torch.cuda.synchronize()
    for k, step in enumerate(steps):
        for r in range(N):
            got = recv[k][r].cpu().numpy()
            if step == "reduce_scatter":
                want = np.sum(np.stack([s[r * count:(r + 1) * count].astype(np.int64) for s in data_h[k]]), axis=0).astype(dtype)
            elif step == "allgather":
                want = np.concatenate([s[:count] for s in data_h[k]])
            else:
                want = _a2a_ref(cnts[k], data_h[k], r, dtype)
            assert np.array_equal(got[:want.size], want), (k, step, "rank", r)
            assert np.isnan(got[want.size:]).all(), (k, step, "rank", r)
