"""cfs_hip_sym_save / cfs_hip_sym_load: a tuned handle written to a plan file and loaded back without tune().

No tolerance anywhere.  The loaded handle must BE the saved one: the same 28 digest words over the device
arrays, the same tile-kernel instantiation, stats, fold lists and plan note; saving it again gives the
first file byte for byte.  Products are compared exactly: integer-valued matrices (every sum is an exact
integer in fp32 and fp64, rand_matrices.sym_int_values) against sym_int_product, and deterministic
handles (bit-reproducible by contract) on the stand-ins' real values bit for bit.  Every y is written
into a guarded buffer.  A damaged file, a wrong tag and a wrong kind of handle are refused with the
documented code and leave nothing behind; the checksums the device kernel computed at save are the
host function of the same bytes.
"""
import ctypes as C
import os
import struct

import numpy as np
import pytest

from rand_matrices import banded_spd, sym_int_product, sym_int_values
from test_gpu_cg_steps import _matrix
from test_gpu_kernel_variants import PLAN_KNOBS
from test_planfile_host import SECTIONS, _layout

pytestmark = pytest.mark.gpu

NO_REORDER, NO_CALIBRATE, EXCHANGE, HYB, DET, KEEP_MAP, HOST_PLAN = 8, 32, 64, 128, 1024, 2048, 4096
DTYPES = pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
SENTINEL = -777.25
LEAD, TRAIL = 256, 1024
MATRICES = ["rand1", "rand2", "rand63", "rand64", "rand65", "rand1023", "rand1026", "band600001", "pwtk@0.05",
            "Flan_1565@0.01"]
OPTIONS = {"default": 0, "natural": NO_REORDER, "hyb": HYB, "det": DET, "map": KEEP_MAP, "host": HOST_PLAN,
           "nocal": NO_CALIBRATE}


@pytest.fixture(autouse=True)
def _torch_first(monkeypatch):
    """torch brings a HIP runtime of its own: it has to initialise before libcfs_hip.so's"""
    import torch
    torch.cuda.init()
    torch.cuda.set_device(0)
    for k in PLAN_KNOBS + ("CFS_HIP_NT", "CFS_HIP_COMBINE", "CFS_HIP_TAKE_HYB", "CFS_HIP_SHAPE", "CFS_HIP_KEEP_ALT"):
        monkeypatch.delenv(k, raising=False)
    yield


def _bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def _guarded(rows, dtype, launch):
    """run launch(y) with y in the middle of a sentinel-filled buffer; the guards must come back untouched"""
    import torch
    buf = torch.full((LEAD + rows + TRAIL,), SENTINEL, dtype=torch.from_numpy(np.zeros(1, dtype)).dtype, device="cuda")
    torch.cuda.synchronize()
    launch(buf[LEAD:LEAD + rows])
    torch.cuda.synchronize()
    h = buf.cpu().numpy()
    guard = np.full(1, SENTINEL, dtype)
    assert _bits(h[:LEAD], np.repeat(guard, LEAD)), "the launch wrote in front of y"
    assert _bits(h[LEAD + rows:], np.repeat(guard, TRAIL)), "the launch wrote behind y"
    return h[LEAD:LEAD + rows].copy()


def _product(A, x, dtype):
    import torch
    xd = torch.from_numpy(np.ascontiguousarray(x, dtype)).cuda()
    return _guarded(A.row_end - A.row_begin, dtype, lambda y: A.dense_vector_multiply(y, xd))


def _same_handle(A, B):
    da, db = A.digest(), B.digest()
    assert len(da) == 28
    for k in da:
        assert da[k] == db[k], f"digest word {k} differs"
    assert A.kernel_variant() == B.kernel_variant()
    assert A.stats() == B.stats()
    for which in (0, 1):
        (d0, l0), (d1, l1) = A.fold_lists(which), B.fold_lists(which)
        assert np.array_equal(d0, d1) and np.array_equal(l0, l1)
    assert A.plan_note() == B.plan_note()
    assert (A.n, A.row_begin, A.row_end, A.nranks, A.rank, A.dtype) == (B.n, B.row_begin, B.row_end, B.nranks, B.rank, B.dtype)


def _cycle(tmp_path, A, tag=None):
    """save -> load -> save again: the handle is the same, the two files are identical"""
    import cfs_spmv_amd as cfs
    p1, p2 = str(tmp_path / "one.plan"), str(tmp_path / "two.plan")
    A.save(p1, tag)
    assert not os.path.exists(p1 + ".tmp")
    B = cfs.SymMatrix.load(p1, expected_tag=tag)
    _same_handle(A, B)
    B.save(p2, tag)
    assert open(p1, "rb").read() == open(p2, "rb").read(), "saving the loaded handle gave another file"
    info = cfs.plan_file_info(p1)  # (the host validator: the device-computed checksums are the host function)
    assert info["tag"] == (tag or "") and info["ntiles"] == A.stats()["ntiles"] and info["nnz_low"] == A.stats()["nnz_low"]
    assert info["device_built"] == A.digest()["device_built"]
    return B


@DTYPES
@pytest.mark.parametrize("name", MATRICES)
def test_identity_and_exact_product(tmp_path, name, dtype):
    import cfs_spmv_amd as cfs
    n, rp, ci, _ = _matrix(name)
    va, x = sym_int_values(np.random.default_rng(n), n, rp, ci, dtype)
    A = cfs.SymMatrix(n, rp, ci, va)
    B = _cycle(tmp_path, A, tag=name)
    want = sym_int_product(n, rp, ci, va, x).astype(dtype)
    ya, yb = _product(A, x, dtype), _product(B, x, dtype)
    assert _bits(yb, want) and _bits(ya, yb)
    import torch
    da, db = A.diagonal(), B.diagonal()
    torch.cuda.synchronize()
    assert _bits(da.cpu().numpy(), db.cpu().numpy())
    A.close()
    assert _bits(_product(B, x, dtype), want), "the loaded handle depends on the one it was saved from"
    B.close()


@DTYPES
@pytest.mark.parametrize("opt", sorted(OPTIONS))
@pytest.mark.parametrize("name", ["rand1026", "pwtk@0.05"])
def test_identity_under_every_option(tmp_path, name, opt, dtype):
    import cfs_spmv_amd as cfs
    n, rp, ci, _ = _matrix(name)
    va, x = sym_int_values(np.random.default_rng(7), n, rp, ci, dtype)
    A = cfs.SymMatrix(n, rp, ci, va, options=cfs.make_options(flags=OPTIONS[opt]))
    B = _cycle(tmp_path, A)
    want = sym_int_product(n, rp, ci, va, x).astype(dtype)
    assert _bits(_product(B, x, dtype), want) and _bits(_product(A, x, dtype), want)
    assert cfs.plan_file_info(str(tmp_path / "one.plan"))["flags"] == OPTIONS[opt]
    A.close(), B.close()


def test_a_schedule_kept_by_measurement_is_the_one_loaded(tmp_path, monkeypatch):
    """Tuning::Aggressive with the alternatives pinned (the clock decides otherwise): the HYB schedule
    tune() kept is what the file holds, although the option flags do not ask for it"""
    import cfs_spmv_amd as cfs
    from cfs_spmv_amd import synth
    monkeypatch.setenv("CFS_HIP_SHAPE", "512")
    monkeypatch.setenv("CFS_HIP_TAKE_HYB", "1")
    n, rp, ci, va, _ = synth.generate("ldoor", 0.3)
    A = cfs.SymMatrix(n, rp, ci, va)
    assert A.stats()["far_entries"] > 0
    monkeypatch.delenv("CFS_HIP_SHAPE")
    monkeypatch.delenv("CFS_HIP_TAKE_HYB")
    B = _cycle(tmp_path, A)
    assert B.stats()["far_entries"] == A.stats()["far_entries"]
    A.close(), B.close()


def test_empty_matrix(tmp_path):
    import cfs_spmv_amd as cfs
    A = cfs.SymMatrix(0, np.zeros(1, np.int32), np.zeros(0, np.int32), np.zeros(0))
    B = _cycle(tmp_path, A)
    assert B.n == 0 and B.stats()["ntiles"] == 0
    A.close(), B.close()


@DTYPES
@pytest.mark.parametrize("name", ["pwtk@0.05", "Flan_1565@0.01"])
def test_deterministic_handles_keep_their_bits(tmp_path, name, dtype):
    import cfs_spmv_amd as cfs
    n, rp, ci, va = _matrix(name)
    va = va.astype(dtype)
    x = np.random.default_rng(3).uniform(-1, 1, n).astype(dtype)
    A = cfs.SymMatrix(n, rp, ci, va, options=cfs.make_options(flags=DET))
    before = _product(A, x, dtype)
    B = _cycle(tmp_path, A)
    assert _bits(_product(B, x, dtype), before) and _bits(_product(A, x, dtype), before)
    A.close(), B.close()


@DTYPES
def test_cg_and_pcg_take_the_same_steps(tmp_path, dtype):
    import torch
    import cfs_spmv_amd as cfs
    n, rp, ci, va = banded_spd(3001, 3, 1)
    va = va.astype(dtype)
    b = torch.from_numpy(np.random.default_rng(5).uniform(-1, 1, n).astype(dtype)).cuda()
    A = cfs.SymMatrix(n, rp, ci, va, options=cfs.make_options(flags=DET))
    B = _cycle(tmp_path, A)
    tol = 1e-10 if dtype == np.float64 else 1e-5
    for solve in ("cg", "pcg"):
        res = []
        for M in (A, B):
            u = torch.zeros_like(b)
            it, _ = getattr(M, solve)(u, b, tol=tol, maxiter=200)
            torch.cuda.synchronize()
            res.append((it, u.cpu().numpy()))
        assert res[0][0] == res[1][0] and res[0][0] > 0 and _bits(res[0][1], res[1][1]), solve
    A.close(), B.close()


@DTYPES
def test_update_values_after_load(tmp_path, dtype):
    import cfs_spmv_amd as cfs
    from cfs_spmv_amd import _lib
    n, rp, ci, _ = _matrix("rand1026")
    v1, x = sym_int_values(np.random.default_rng(1), n, rp, ci, dtype)
    v2, _ = sym_int_values(np.random.default_rng(2), n, rp, ci, dtype)
    A = cfs.SymMatrix(n, rp, ci, v1, options=cfs.make_options(flags=KEEP_MAP))
    B = _cycle(tmp_path, A)
    B.update_values(v2)
    assert _bits(_product(B, x, dtype), sym_int_product(n, rp, ci, v2, x).astype(dtype))
    assert _bits(_product(A, x, dtype), sym_int_product(n, rp, ci, v1, x).astype(dtype)), "the original handle changed"
    A.close(), B.close()
    # without the map a loaded handle refuses, as a fresh one does
    A = cfs.SymMatrix(n, rp, ci, v1)
    B = _cycle(tmp_path, A)
    for M in (A, B):
        with pytest.raises(_lib.CfsHipError, match="KEEP_VALUE_MAP") as e:
            M.update_values(v2)
        assert e.value.code == _lib.ERR_ARG
    A.close(), B.close()


@DTYPES
@pytest.mark.parametrize("nranks", [2, 3])
@pytest.mark.parametrize("form", [0, EXCHANGE], ids=["mirrored", "exchange"])
def test_shards(tmp_path, form, nranks, dtype):
    import torch
    import cfs_spmv_amd as cfs
    n, rp, ci, _ = _matrix("rand1026")
    va, x = sym_int_values(np.random.default_rng(11), n, rp, ci, dtype)
    want = sym_int_product(n, rp, ci, va, x).astype(dtype)
    rs = cfs.balanced_splits(n, rp, ci, nranks)
    loaded = []
    for r in range(nranks):
        A = cfs.SymMatrix(n, rp, ci, va, options=cfs.make_options(flags=form), row_splits=rs, rank=r)
        d = tmp_path / f"rank{r}"
        d.mkdir()
        B = _cycle(d, A, tag=f"rank {r} of {nranks}")
        assert np.array_equal(A.send_counts(), B.send_counts()) and np.array_equal(A.send_rows(), B.send_rows())
        if form == 0:
            assert B.send_rows().size == 0
        A.close()
        loaded.append(B)
    xd = torch.from_numpy(x).cuda()
    tdt = xd.dtype
    sends, blocks = [], []
    for B in loaded:
        rows = B.row_end - B.row_begin
        send = torch.zeros(max(1, B.send_rows().size), dtype=tdt, device="cuda")
        yb = torch.full((LEAD + rows + TRAIL,), SENTINEL, dtype=tdt, device="cuda")
        B.spmv_local(yb[LEAD:LEAD + rows], xd, send)
        sends.append(send), blocks.append(yb)
    torch.cuda.synchronize()
    if form == EXCHANGE:  # the exchange as a plain tensor copy: what rank q receives, sender after sender
        owner = [np.searchsorted(rs, B.send_rows(), side="right") - 1 for B in loaded]
        for q, B in enumerate(loaded):
            idx = [np.flatnonzero(owner[r] == q) for r in range(nranks)]
            recv_rows = np.concatenate([loaded[r].send_rows()[idx[r]] for r in range(nranks)])
            B.set_recv(recv_rows)
            if recv_rows.size:
                recv = torch.cat([sends[r][torch.from_numpy(idx[r]).cuda()] for r in range(nranks)])
                rows = B.row_end - B.row_begin
                B.recv_fold(blocks[q][LEAD:LEAD + rows], recv)
        torch.cuda.synchronize()
    got = []
    for B, yb in zip(loaded, blocks):
        h = yb.cpu().numpy()
        rows = B.row_end - B.row_begin
        assert np.all(h[:LEAD] == SENTINEL) and np.all(h[LEAD + rows:] == SENTINEL)
        got.append(h[LEAD:LEAD + rows])
        B.close()
    assert _bits(np.concatenate(got), want)


@DTYPES
@pytest.mark.parametrize("name", ["rand1026", "pwtk@0.05"])
def test_a_file_written_on_the_host_loads(tmp_path, name, dtype):
    import cfs_spmv_amd as cfs
    n, rp, ci, _ = _matrix(name)
    va, x = sym_int_values(np.random.default_rng(13), n, rp, ci, dtype)
    path = str(tmp_path / "host.plan")
    cfs.plan_save(path, n, rp, ci, va, tag="host")
    B = cfs.SymMatrix.load(path, expected_tag="host")
    assert B.digest()["device_built"] == 0 and B.stats()["value_bytes"] == np.dtype(dtype).itemsize
    assert _bits(_product(B, x, dtype), sym_int_product(n, rp, ci, va, x).astype(dtype))
    B.close()


def _load_rc(path, tag=None):
    import cfs_spmv_amd as cfs
    out = C.c_void_p(1)
    rc = cfs.load().cfs_hip_sym_load(os.fsencode(str(path)), tag, C.byref(out))
    assert (rc == 0) == bool(out.value), "a refused load must leave *out = NULL"
    return rc, out, cfs.load().cfs_hip_last_error().decode()


def test_refusals(tmp_path):
    import torch
    import cfs_spmv_amd as cfs
    from cfs_spmv_amd import _lib
    lib = cfs.load()
    n, rp, ci, _ = _matrix("rand1026")
    va, x = sym_int_values(np.random.default_rng(17), n, rp, ci, np.float32)
    want = sym_int_product(n, rp, ci, va, x).astype(np.float32)
    A = cfs.SymMatrix(n, rp, ci, va)
    good, bad = str(tmp_path / "good.plan"), tmp_path / "bad.plan"
    A.save(good, "right")
    data = open(good, "rb").read()
    header_bytes, rows = _layout(data)

    def good_load_still_works():
        B = cfs.SymMatrix.load(good, expected_tag="right")
        assert _bits(_product(B, x, np.float32), want)
        B.close()

    good_load_still_works()  # (streams, page-locked blocks and torch's cache exist from here on)
    torch.cuda.synchronize()
    free0 = torch.cuda.mem_get_info()[0]

    # a payload byte flipped and the host-visible part left consistent: the DEVICE checksum catches it
    for name in ("vals", "slots", "tiles"):
        _, off, nbytes = rows[SECTIONS.index(name)]
        assert nbytes > 0
        b = bytearray(data)
        b[off + nbytes // 2] ^= 0x01
        bad.write_bytes(bytes(b))
        rc, _, msg = _load_rc(bad)
        assert rc == _lib.ERR_FILE and "checksum mismatch in section " + name in msg, msg
        good_load_still_works()
    rc, _, msg = _load_rc(good, b"wrong")
    assert rc == _lib.ERR_FILE and "right" in msg and "wrong" in msg, msg
    good_load_still_works()
    b = bytearray(data)  # an f32 file that claims 8-byte values
    assert struct.unpack_from("<I", b, 16)[0] == 4
    struct.pack_into("<I", b, 16, 8)
    bad.write_bytes(bytes(b))
    rc, _, msg = _load_rc(bad)
    assert rc == _lib.ERR_FILE, msg
    good_load_still_works()
    bad.write_bytes(data[:len(data) // 2])
    assert _load_rc(bad)[0] == _lib.ERR_FILE
    assert _load_rc(tmp_path / "missing.plan")[0] == _lib.ERR_FILE
    # what the refused loads allocated is gone: a handle of this matrix holds ~100 KB, five were refused
    # after their upload; the allowance is one 2 MiB segment of torch's caching allocator
    torch.cuda.synchronize()
    assert torch.cuda.mem_get_info()[0] >= free0 - (2 << 20), "a refused load left device memory behind"
    # NULL arguments
    out = C.c_void_p()
    assert lib.cfs_hip_sym_save(None, good.encode(), None) == _lib.ERR_ARG
    assert lib.cfs_hip_sym_save(A._h, None, None) == _lib.ERR_ARG
    assert lib.cfs_hip_sym_load(None, None, C.byref(out)) == _lib.ERR_ARG
    assert lib.cfs_hip_sym_load(good.encode(), None, None) == _lib.ERR_ARG
    # a multi-device handle (two shards on this device) is not a file
    M = cfs.SymMatrix(n, rp, ci, va, ngpus=2, devices=[0, 0])
    assert lib.cfs_hip_sym_save(M._h, str(tmp_path / "multi.plan").encode(), None) == _lib.ERR_UNSUPPORTED
    assert not os.path.exists(tmp_path / "multi.plan") and not os.path.exists(str(tmp_path / "multi.plan") + ".tmp")
    M.close()
    good_load_still_works()
    assert _bits(_product(A, x, np.float32), want), "save changed the handle"
    A.close()


def _checksum_by_definition(data):
    """cfs_planfile.hpp's header comment, in numpy: sum over the 64-bit little-endian words (tail
    zero-padded) of mix64(w_i + (i + 1) * 0x9E3779B97F4A7C15), mod 2^64"""
    b = np.frombuffer(bytes(data) + b"\0" * (-len(data) % 8), dtype="<u8").copy()
    with np.errstate(over="ignore"):
        z = b + (np.arange(b.size, dtype=np.uint64) + np.uint64(1)) * np.uint64(0x9E3779B97F4A7C15)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        z = z ^ (z >> np.uint64(31))
        return int(np.sum(z, dtype=np.uint64))


def _checksum(ptr, nbytes, on_device):
    import cfs_spmv_amd as cfs
    from cfs_spmv_amd import _lib
    out = C.c_ulonglong()
    _lib.check(cfs.load().cfs_hip_debug_checksum(ptr, nbytes, on_device, C.byref(out)))
    return out.value


@pytest.mark.parametrize("nbytes", [1, 7, 15, 16, 17, 4097, (1 << 22) + 9])
def test_device_checksum_equals_host_checksum(nbytes):
    """the kernel reads [p, p + bytes) and nothing else: the bytes behind the range are 0xFF here and
    would change the sum; (1 << 22) + 9 bytes takes the full grid, several strides per thread and a tail"""
    import torch
    data = np.random.default_rng(nbytes).integers(0, 256, nbytes + 64, dtype=np.uint8)
    data[nbytes:] = 0xFF
    d = torch.from_numpy(data).cuda()
    torch.cuda.synchronize()
    assert d.data_ptr() % 16 == 0
    want = _checksum_by_definition(data[:nbytes])
    assert _checksum(data.ctypes.data, nbytes, 0) == want
    assert _checksum(d.data_ptr(), nbytes, 1) == want
    if nbytes >= 17:  # position-sensitive: two different words swapped
        sw = data.copy()
        sw[0:8], sw[8:16] = data[8:16].copy(), data[0:8].copy()
        assert _checksum_by_definition(sw[:nbytes]) != want
        assert _checksum(torch.from_numpy(sw).cuda().data_ptr(), nbytes, 1) == _checksum_by_definition(sw[:nbytes])


def test_every_section_checksum_of_a_saved_file_is_the_host_function(tmp_path):
    """the table save() writes holds what the DEVICE kernel computed; plan_file_info recomputes every
    section on the host from the file's bytes, and so does this test from the definition"""
    import cfs_spmv_amd as cfs
    n, rp, ci, va = _matrix("rand1026")
    A = cfs.SymMatrix(n, rp, ci, va, options=cfs.make_options(flags=KEEP_MAP | HYB))
    p = str(tmp_path / "c.plan")
    A.save(p)
    A.close()
    cfs.plan_file_info(p)
    data = open(p, "rb").read()
    header_bytes, rows = _layout(data)
    odd = 0
    for i, (name, off, nb) in enumerate(rows):
        stored, = struct.unpack_from("<Q", data, header_bytes + 32 * i + 24)
        assert stored == _checksum_by_definition(data[off:off + nb]), name
        odd += nb % 16 != 0
    assert odd >= 3, "no section length that exercises the tail path"
