"""Plan files on the host (no GPU): cfs_hip_sym_plan_save_* writes the schedule the host builder makes,
cfs_hip_plan_file_check -- the validator of cfs_spmv_amd/csrc/cfs_planfile.hpp -- reads it back.

Round trip: every field the file's header shares with plan_check's report agrees with it, and writing
twice gives identical bytes.  Corruption: one flipped byte anywhere, a truncation at or next to any
section boundary, an empty file, a directory and a missing path are each CFS_HIP_ERR_FILE with a
message that says what failed; a flipped payload byte fails on the checksum of ITS section.
"""
import ctypes as C
import os
import struct

import numpy as np
import pytest

import cfs_spmv_amd as cfs
from cfs_spmv_amd import _lib
from test_gpu_cg_steps import _matrix

NO_REORDER, EXCHANGE, HYB, DET, KEEP_MAP = 8, 64, 128, 1024, 2048
DTYPES = pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
MATRICES = ["rand1", "rand2", "rand65", "rand1026", "pwtk@0.05"]
SHARED = ("ntiles", "ngroups", "lds_slots", "nslices", "halo_slots", "stream_len", "nnz_low", "fold_rows",
          "remote_vals", "mirror_entries", "far_entries")
# cfs_planfile.hpp: 64 fixed bytes, the 64-bit scalars, tag and plan_note of 256 bytes each; 31 rows of
# {id u32, elem u32, offset u64, bytes u64, checksum u64}
SECTIONS = ["tiles", "slot_col", "rowinfo", "diag", "slice_meta", "leadlane", "vals", "slots", "cvals", "crows", "ccols",
            "fvals", "frows", "fcols", "val_map", "cval_map", "fval_map", "diag_map", "fold_rec", "fold_idx", "send_ptr",
            "send_idx", "slot_exp", "group_first", "group_ptr", "launch_order", "fold_dst", "send_row", "send_counts",
            "tile_rounds", "row_splits"]


def _layout(data):
    """(header bytes, [(name, offset, bytes)]) read from the file itself"""
    header_bytes, = struct.unpack_from("<I", data, 12)
    nsec, row_bytes = struct.unpack_from("<2I", data, 32)
    assert nsec == len(SECTIONS) and row_bytes == 32
    rows = []
    for i in range(nsec):
        sid, _, off, nbytes, _ = struct.unpack_from("<2I3Q", data, header_bytes + 32 * i)
        assert sid == i
        rows.append((SECTIONS[i], off, nbytes))
    return header_bytes, rows


def _refused(path):
    info = _lib.PlanFileInfo()
    rc = cfs.load().cfs_hip_plan_file_check(os.fsencode(str(path)), C.byref(info))
    assert rc == _lib.ERR_FILE, f"expected CFS_HIP_ERR_FILE, got {rc}"
    msg = cfs.load().cfs_hip_last_error().decode()
    assert len(msg) > 10
    return msg


def _roundtrip(tmp_path, n, rp, ci, va, flags, nranks=1, rank=0, rs=None):
    opt = cfs.make_options(flags=flags)
    a, b = str(tmp_path / "a.plan"), str(tmp_path / "b.plan")
    cfs.plan_save(a, n, rp, ci, va, nranks, rank, rs, opt, tag="first")
    cfs.plan_save(b, n, rp, ci, va, nranks, rank, rs, opt, tag="first")
    assert open(a, "rb").read() == open(b, "rb").read(), "writing twice gave different bytes"
    assert not os.path.exists(a + ".tmp")
    info = cfs.plan_file_info(a)
    rep = cfs.plan_check(n, rp, ci, va, nranks, rank, rs, opt)
    assert rep["mismatches"] == 0
    for k in SHARED:
        assert info[k] == rep[k], (k, info[k], rep[k])
    lo, hi = (0, n) if rs is None else (int(rs[rank]), int(rs[rank + 1]))
    assert (info["n"], info["row_begin"], info["row_end"], info["nranks"], info["rank"]) == (n, lo, hi, nranks, rank)
    assert info["format_version"] == 1 and info["value_bytes"] == va.dtype.itemsize and info["flags"] == flags
    assert info["has_value_map"] == int(bool(flags & KEEP_MAP)) and info["deterministic"] == int(bool(flags & DET))
    assert info["device_built"] == 0 and info["nsections"] == len(SECTIONS) and info["tag"] == "first"
    assert info["block_threads"] in (256, 512, 1024) and info["file_bytes"] == os.path.getsize(a)
    assert sum(nb for _, _, nb in _layout(open(a, "rb").read())[1]) == info["payload_bytes"]
    return a


@DTYPES
@pytest.mark.parametrize("flags", [0, NO_REORDER, HYB, DET, KEEP_MAP], ids=["default", "natural", "hyb", "det", "map"])
@pytest.mark.parametrize("name", MATRICES)
def test_round_trip(tmp_path, name, flags, dtype):
    n, rp, ci, va = _matrix(name)
    _roundtrip(tmp_path, n, rp, ci, va.astype(dtype), flags)


@DTYPES
@pytest.mark.parametrize("flags", [0, EXCHANGE], ids=["mirrored", "exchange"])
def test_round_trip_of_two_shards(tmp_path, flags, dtype):
    n, rp, ci, va = _matrix("rand1026")
    rs = cfs.balanced_splits(n, rp, ci, 2)
    for rank in range(2):
        _roundtrip(tmp_path, n, rp, ci, va.astype(dtype), flags, 2, rank, rs)


@pytest.fixture(scope="module")
def good_file(tmp_path_factory):
    """one file with every kind of section present: HYB far entries, the value map, a halo fold"""
    n, rp, ci, va = _matrix("rand1026")
    path = str(tmp_path_factory.mktemp("plan") / "good.plan")
    cfs.plan_save(path, n, rp, ci, va, options=cfs.make_options(flags=HYB | KEEP_MAP), tag="t")
    cfs.plan_file_info(path)
    return open(path, "rb").read()


def test_a_flipped_byte_is_refused_wherever_it_is(tmp_path, good_file):
    header_bytes, rows = _layout(good_file)
    p = tmp_path / "bad.plan"

    def flipped(pos):
        b = bytearray(good_file)
        b[pos] ^= 0x40
        p.write_bytes(bytes(b))
        return _refused(p)

    # header: magic, version, a struct size, the file size, a count, a kept choice, the tag
    for pos in (0, 8, 20, 40, 64 + 8 * 14, header_bytes - 512 - 8, header_bytes - 512):
        flipped(pos)
    # section table: a checksum, a length and an offset of a row in the middle
    mid = header_bytes + 32 * SECTIONS.index("vals")
    for pos in (mid + 24, mid + 16, mid + 8, mid):
        flipped(pos)
    some = 0
    for name, off, nbytes in rows:
        if nbytes == 0:
            continue
        some += 1
        msg = flipped(off + nbytes // 2)
        assert "checksum mismatch in section " + name in msg, (name, msg)
        others = [s for s in SECTIONS if s != name and ("section " + s + " ") in msg + " "]
        assert not others, msg
    assert some >= 20, "the fixture was meant to have most sections present"


def test_truncations_are_refused(tmp_path, good_file):
    _, rows = _layout(good_file)
    p = tmp_path / "cut.plan"
    cuts = {0, 1, 63, 64, len(good_file) - 1}
    for _, off, nbytes in rows:
        cuts.update((off - 1, off, off + nbytes - 1, off + nbytes))
    for cut in sorted(c for c in cuts if 0 <= c < len(good_file)):
        p.write_bytes(good_file[:cut])
        msg = _refused(p)
        assert "truncated" in msg, (cut, msg)
    p.write_bytes(good_file + b"\0" * 64)  # longer than the header says
    assert "extended" in _refused(p)


def test_what_is_not_a_plan_file(tmp_path):
    p = tmp_path / "empty.plan"
    p.write_bytes(b"")
    assert "truncated" in _refused(p)
    assert "not a regular file" in _refused(tmp_path)
    assert "cannot open" in _refused(tmp_path / "missing.plan")
    p.write_bytes(b"%%MatrixMarket matrix coordinate real symmetric\n" + b"1 1 1\n" * 400)
    assert "not a plan file" in _refused(p)


def test_abi(tmp_path):
    lib = cfs.load()
    assert lib.cfs_hip_abi_version() == 4
    for name in ("cfs_hip_sym_save", "cfs_hip_sym_load", "cfs_hip_plan_file_check", "cfs_hip_sym_plan_save_f64",
                 "cfs_hip_sym_plan_save_f32"):
        assert hasattr(lib, name) and name in _lib.SYMBOLS
    assert _lib.ERR_FILE == -7
    info = _lib.PlanFileInfo()
    assert lib.cfs_hip_plan_file_check(None, C.byref(info)) == _lib.ERR_ARG
    assert lib.cfs_hip_plan_file_check(b"x", None) == _lib.ERR_ARG
    n, rp, ci, va = _matrix("rand65")
    rp, ci = rp.astype(np.int32), ci.astype(np.int32)
    args = (n, rp.ctypes.data, ci.ctypes.data, va.ctypes.data, 1, 0, None, None)
    assert lib.cfs_hip_sym_plan_save_f64(*args, None, None) == _lib.ERR_ARG
    assert lib.cfs_hip_sym_plan_save_f64(*args, os.fsencode(str(tmp_path / "x.plan")), b"t" * 256) == _lib.ERR_ARG
    assert lib.cfs_hip_sym_plan_save_f64(*args, os.fsencode(str(tmp_path / "x.plan")), b"t" * 255) == 0
    assert cfs.plan_file_info(str(tmp_path / "x.plan"))["tag"] == "t" * 255
    # a directory that does not exist: the writer says so, nothing is left behind
    assert lib.cfs_hip_sym_plan_save_f64(*args, os.fsencode(str(tmp_path / "no" / "x.plan")), None) == _lib.ERR_FILE
    assert "cannot create" in lib.cfs_hip_last_error().decode()
    # load and save refuse NULL arguments before they touch a device
    out = C.c_void_p(1)
    assert lib.cfs_hip_sym_load(None, None, C.byref(out)) == _lib.ERR_ARG and not out.value
    assert lib.cfs_hip_sym_load(b"x", None, None) == _lib.ERR_ARG
    assert lib.cfs_hip_sym_save(None, b"x", None) == _lib.ERR_ARG
