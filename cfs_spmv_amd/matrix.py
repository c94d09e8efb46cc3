"""Host-side mirror of the reference's operator surface for the hot path, over
the C ABI (include/cfs_hip.h).  Names and argument meaning follow

    SparseMatrix<I,V>::create / nrows / ncols / nnz / symmetric / size / tune /
    dense_vector_multiply     include/matrix/sparse_matrix.hpp:23-41
    SpDMV<I,V>(A, Tuning), operator()(y, M, x, N)
                              include/kernel/sparse_kernel.hpp:17-27

so the parity tests read like test/test_spmv_mmf.cpp.  torch is used only for
device memory and streams; nothing here computes an SpMV on the host."""
import ctypes as C
import enum
import os
import struct

import numpy as np

from . import _lib


class Format(enum.IntEnum):  # include/utils/platform.hpp:23
    none = 0
    csr = 1
    sss = 2
    hyb = 3


class Tuning(enum.IntEnum):  # include/utils/platform.hpp:22
    NONE = 0
    Aggressive = 1


class Kernel(enum.IntEnum):  # include/utils/platform.hpp:21
    SpDMV = 0


def _np_i32(a):
    return np.ascontiguousarray(a, dtype=np.int32)


def _ptr(t):
    """raw pointer of a torch tensor / numpy array / int"""
    if isinstance(t, int):
        return t
    if isinstance(t, np.ndarray):
        return t.ctypes.data
    return t.data_ptr()


def _stream_ptr(stream=None):
    import torch
    s = stream if stream is not None else torch.cuda.current_stream()
    return s.cuda_stream


FLAG_SHARD_EXCHANGE = 64  # include/cfs_hip.h: CFS_HIP_FLAG_SHARD_EXCHANGE
FLAG_KEEP_VALUE_MAP = 2048  # CFS_HIP_FLAG_KEEP_VALUE_MAP
FLAG_HOST_PLAN = 4096  # CFS_HIP_FLAG_HOST_PLAN: build the schedule with the host builder
# CFS_HIP_KERNEL_WORDS: cfs_sym_tile_kernel<V, BLOCK, MODE, NT, OFFB, U, DET, COMB> ("value_bytes" = sizeof(V))
EXCHANGE_REDUCE_SCATTER, EXCHANGE_SPARSE = _lib.EXCHANGE_REDUCE_SCATTER, _lib.EXCHANGE_SPARSE  # CFS_HIP_EXCHANGE_*
EXCHANGE = {"reduce_scatter": EXCHANGE_REDUCE_SCATTER, "sparse": EXCHANGE_SPARSE}
PRECOND = {"none": _lib.PRECOND_NONE, "jacobi": _lib.PRECOND_JACOBI}  # CFS_HIP_PRECOND_*
LOBPCG_PRECOND = {"none": 0, "jacobi": 1, "block_jacobi": 3}  # block_rows of cfs_hip_sym_lobpcg (block_jacobi: `block`)
EIGS_WHICH = {"LA": _lib.EIGS_LARGEST, "SA": _lib.EIGS_SMALLEST, "LM": _lib.EIGS_MAGNITUDE}  # CFS_HIP_EIGS_*
KERNEL_NAMES = ["value_bytes", "block", "mode", "nt", "offb", "u", "det", "comb"]
DIGEST_WORDS = 28  # CFS_HIP_DIGEST_WORDS
DIGEST_NAMES = ["tiles", "gfirst", "group_range", "slot_col", "rowinfo", "diag", "slice_meta", "leadlane",
                "vals", "slots", "cvals", "crows", "ccols", "fold_rec", "fold_idx", "val_map", "cval_map",
                "diag_map", "window", "slot_exp", "send_ptr", "send_idx", "fvals", "frows", "fcols", "fval_map",
                "far_entries", "device_built"]


def make_options(max_slots=0, max_tile_nnz=0, block_threads=0, flags=0):
    return _lib.Options(max_slots, max_tile_nnz, block_threads, flags)


def balanced_splits(n, rowptr, colind, nranks):
    rowptr, colind = _np_i32(rowptr), _np_i32(colind)
    out = np.zeros(nranks + 1, dtype=np.int32)
    _lib.check(_lib.load().cfs_hip_sym_balanced_splits(
        n, rowptr.ctypes.data, colind.ctypes.data, nranks, out.ctypes.data))
    return out


def plan_check(n, rowptr, colind, values, nranks=1, rank=0, row_splits=None, options=None):
    """host-only structural self-check of the tile schedule (no GPU needed)"""
    lib = _lib.load()
    rowptr, colind = _np_i32(rowptr), _np_i32(colind)
    values = np.ascontiguousarray(values)
    suf = "f64" if values.dtype == np.float64 else "f32"
    rs = _np_i32(row_splits) if row_splits is not None else None
    rep = _lib.PlanReport()
    _lib.check(getattr(lib, "cfs_hip_sym_plan_check_" + suf)(
        n, rowptr.ctypes.data, colind.ctypes.data, values.ctypes.data, nranks, rank,
        rs.ctypes.data if rs is not None else None,
        C.byref(options) if options is not None else None, C.byref(rep)))
    return rep.asdict()


def _cstr(s):
    return None if s is None else os.fsencode(s)


def plan_file_info(path):
    """host-only: validate a plan file (header, section table, lengths, checksums) and return what
    its header says (cfs_hip_plan_file_check); raises CfsHipError (code ERR_FILE) with the reason"""
    info = _lib.PlanFileInfo()
    _lib.check(_lib.load().cfs_hip_plan_file_check(_cstr(path), C.byref(info)))
    return info.asdict()


def plan_save(path, n, rowptr, colind, values, nranks=1, rank=0, row_splits=None, options=None, tag=None):
    """host-only: build the schedule with the host builder, as plan_check does, and write it as a
    plan file that SymMatrix.load reads on a machine with a GPU (cfs_hip_sym_plan_save_*)"""
    lib = _lib.load()
    rowptr, colind = _np_i32(rowptr), _np_i32(colind)
    values = np.ascontiguousarray(values)
    suf = "f64" if values.dtype == np.float64 else "f32"
    rs = _np_i32(row_splits) if row_splits is not None else None
    _lib.check(getattr(lib, "cfs_hip_sym_plan_save_" + suf)(
        n, rowptr.ctypes.data, colind.ctypes.data, values.ctypes.data, nranks, rank,
        rs.ctypes.data if rs is not None else None,
        C.byref(options) if options is not None else None, _cstr(path), _cstr(tag)))


def plan_send_info(n, rowptr, colind, values, nranks, rank, row_splits, options=None):
    """host-only (send_counts, send_rows) of one shard in the EXCHANGE form
    (CFS_HIP_FLAG_SHARD_EXCHANGE) -- for the CPU exchange tests"""
    lib = _lib.load()
    if options is None:
        options = make_options(flags=FLAG_SHARD_EXCHANGE)
    else:
        options = _lib.Options(options.max_slots, options.max_tile_nnz, options.block_threads,
                               options.flags | FLAG_SHARD_EXCHANGE)
    rowptr, colind = _np_i32(rowptr), _np_i32(colind)
    values = np.ascontiguousarray(values, dtype=np.float64)
    rs = _np_i32(row_splits)
    counts = np.zeros(nranks, dtype=np.int32)
    nr = C.c_int()
    optp = C.byref(options) if options is not None else None
    _lib.check(lib.cfs_hip_sym_plan_send_info_f64(
        n, rowptr.ctypes.data, colind.ctypes.data, values.ctypes.data, nranks, rank,
        rs.ctypes.data, optp, counts.ctypes.data, None, 0, C.byref(nr)))
    rows = np.zeros(nr.value, dtype=np.int32)
    if nr.value:
        _lib.check(lib.cfs_hip_sym_plan_send_info_f64(
            n, rowptr.ctypes.data, colind.ctypes.data, values.ctypes.data, nranks, rank,
            rs.ctypes.data, optp, counts.ctypes.data, rows.ctypes.data, nr.value,
            C.byref(nr)))
    return counts, rows


class SymMatrix:
    """A symmetric matrix tuned for the MI355X tile kernel (Format::sss).

    Built from the FULL CSR exactly as CSRMatrix holds it before tune()
    (csr_matrix.tpp:74-107).  `row_splits`/`rank` build one 1-D row block of a
    sharded matrix."""

    def __init__(self, n, rowptr, colind, values, options=None, row_splits=None, rank=0,
                 ngpus=1, devices=None):
        lib = _lib.load()
        rowptr, colind = _np_i32(rowptr), _np_i32(colind)
        values = np.ascontiguousarray(values)
        if values.dtype not in (np.float64, np.float32):
            raise TypeError("values must be float64 or float32 (src/csr.cpp:10-11)")
        self.dtype = values.dtype
        self.n = int(n)
        suf = "f64" if self.dtype == np.float64 else "f32"
        self._h = C.c_void_p()
        optp = C.byref(options) if options is not None else None
        if ngpus > 1:
            # one host thread, ngpus shards (cfs_hip_sym_create_multi_*: what the C++
            # surface builds for CFS_NUM_GPUS); shards may share devices
            dv = _np_i32(devices) if devices is not None else None
            _lib.check(getattr(lib, "cfs_hip_sym_create_multi_" + suf)(
                n, rowptr.ctypes.data, colind.ctypes.data, values.ctypes.data, int(ngpus),
                dv.ctypes.data if dv is not None else None, optp, C.byref(self._h)))
            self.nranks, self.rank = 1, 0
        elif row_splits is None:
            _lib.check(getattr(lib, "cfs_hip_sym_create_" + suf)(
                n, rowptr.ctypes.data, colind.ctypes.data, values.ctypes.data, optp,
                C.byref(self._h)))
            self.nranks, self.rank = 1, 0
        else:
            rs = _np_i32(row_splits)
            self.nranks, self.rank = len(rs) - 1, int(rank)
            _lib.check(getattr(lib, "cfs_hip_sym_create_shard_" + suf)(
                n, rowptr.ctypes.data, colind.ctypes.data, values.ctypes.data, self.nranks,
                self.rank, rs.ctypes.data, optp, C.byref(self._h)))
        self._tuned = True
        st = self.stats()
        self.row_begin, self.row_end = st["row_begin"], st["row_end"]

    # -- plan files: the tuned handle on disk (cfs_hip_sym_save / cfs_hip_sym_load) --
    def save(self, path, tag=None):
        """write the handle -- the schedule and the kernel choices tune() kept -- to `path`; `tag` (at
        most 255 bytes) is stored verbatim for load(expected_tag=...)"""
        _lib.check(_lib.load().cfs_hip_sym_save(self._h, _cstr(path), _cstr(tag)))

    @classmethod
    def load(cls, path, expected_tag=None):
        """a handle from a plan file, on the current device, without tune(); raises CfsHipError (code
        ERR_FILE) when the file is damaged, of another format version or saved with another tag"""
        lib = _lib.load()
        self = cls.__new__(cls)
        self._h = C.c_void_p()
        _lib.check(lib.cfs_hip_sym_load(_cstr(path), _cstr(expected_tag), C.byref(self._h)))
        self._tuned = True
        st = self.stats()
        self.dtype = np.dtype(np.float64 if st["value_bytes"] == 8 else np.float32)
        self.n = st["n"]
        self.row_begin, self.row_end = st["row_begin"], st["row_end"]
        # (nranks / rank: the 4th and 5th 64-bit scalar behind the 64 fixed bytes of the header,
        # cfs_planfile.hpp -- read directly, plan_file_info would checksum the whole file again)
        with open(path, "rb") as f:
            self.nranks, self.rank = struct.unpack_from("<2q", f.read(104), 88)
        return self

    # -- SparseMatrix surface (sparse_matrix.hpp:25-33) --
    def nrows(self):
        return self.n

    def ncols(self):
        return self.n

    def nnz(self):
        return self.stats()["nnz_full"]

    def symmetric(self):
        return True

    def size(self):
        return self.stats()["device_bytes"]

    def tune(self, kernel=Kernel.SpDMV, tuning=Tuning.Aggressive):
        return True  # the schedule is built at construction

    def digest(self):
        """developer / test: digests of the schedule's device arrays (cfs_hip_sym_debug_digest)"""
        w = (C.c_ulonglong * DIGEST_WORDS)()
        _lib.check(_lib.load().cfs_hip_sym_debug_digest(self._h, w, DIGEST_WORDS))
        return dict(zip(DIGEST_NAMES, [int(v) for v in w]))

    def kernel_variant(self):
        """developer / test: template arguments of the tile-kernel instantiation this handle
        launches (cfs_hip_sym_debug_kernel)"""
        w = (C.c_int * len(KERNEL_NAMES))()
        _lib.check(_lib.load().cfs_hip_sym_debug_kernel(self._h, w, len(KERNEL_NAMES)))
        return dict(zip(KERNEL_NAMES, [int(v) for v in w]))

    def fold_lists(self, which=0):
        """developer / test: (dst, len) of the lists cfs_fold_kernel walks, in record order, decoded from
        the device arrays (cfs_hip_sym_debug_fold_lists): which = 0 the local halo fold, 1 the receive
        fold; dst = local rows"""
        cap = max(1, self.row_end - self.row_begin)  # at most one list per owned row
        dst, ln, cnt = np.zeros(cap, np.int32), np.zeros(cap, np.int32), C.c_int()
        _lib.check(_lib.load().cfs_hip_sym_debug_fold_lists(self._h, int(which), dst.ctypes.data, ln.ctypes.data,
                                                            cap, C.byref(cnt)))
        return dst[:cnt.value].copy(), ln[:cnt.value].copy()

    def plan_note(self):
        """why the device builder handed the schedule to the host builder ('' = it built it)"""
        buf = C.create_string_buffer(256)
        _lib.check(_lib.load().cfs_hip_sym_debug_plan_note(self._h, buf, 256))
        return buf.value.decode(errors="replace")

    def stats(self):
        st = _lib.SymStats()
        _lib.check(_lib.load().cfs_hip_sym_get_stats(self._h, C.byref(st)))
        return st.asdict()

    def dense_vector_multiply(self, y, x, stream=None):
        """y <- A x on device tensors (fully overwrites y), enqueued on torch's
        current stream (or `stream`)."""
        _lib.check(_lib.load().cfs_hip_sym_spmv_async(
            self._h, _ptr(y), _ptr(x), _stream_ptr(stream)))

    def dense_vector_multiply_host(self, y, x):
        """host numpy arrays: the slow staged drop-in path of cfs_hip_sym_spmv"""
        _lib.check(_lib.load().cfs_hip_sym_spmv(self._h, _ptr(y), _ptr(x)))

    def cg(self, u, b, tol=1e-10, maxiter=1000, check_every=8, stream=None):
        """conjugate gradients inside the library (cfs_hip_sym_cg): u (device tensor) holds the
        first guess and receives the solution of A u = b; no host round trip inside the loop.
        Returns (iterations, ||b - A u|| / ||b||)."""
        it, res = C.c_int(), C.c_double()
        _lib.check(_lib.load().cfs_hip_sym_cg(self._h, _ptr(u), _ptr(b), float(tol), int(maxiter), int(check_every),
                                              C.byref(it), C.byref(res), _stream_ptr(stream)))
        return it.value, res.value

    def diagonal(self, out=None, stream=None):
        """the diagonal of the rows this handle owns (cfs_hip_sym_diagonal_async): a device tensor of
        row_end - row_begin values of the matrix's value type, 0 where the matrix stores no diagonal
        entry, gathered from the handle's device arrays (so it follows update_values).  `out`: a
        device tensor to fill instead of a new one."""
        import torch
        rows = self.row_end - self.row_begin
        tdt = torch.float64 if self.dtype == np.float64 else torch.float32
        if out is None:
            out = torch.empty(rows, dtype=tdt, device="cuda")
        elif out.dtype != tdt or out.numel() < rows or not out.is_contiguous():
            raise ValueError(f"out must be a contiguous {tdt} tensor of at least {rows} values")
        _lib.check(_lib.load().cfs_hip_sym_diagonal_async(self._h, _ptr(out), _stream_ptr(stream)))
        return out

    def _blocks(self, fn, block, out, stream):
        import torch
        block = int(block)
        nb = -(-self.nrows() // block) if block > 0 else 0
        tdt = torch.float64 if self.dtype == np.float64 else torch.float32
        if out is None:
            out = torch.empty((nb, max(block, 0), max(block, 0)), dtype=tdt, device="cuda")
        elif out.dtype != tdt or out.numel() < nb * block * block or not out.is_contiguous():
            raise ValueError(f"out must be a contiguous {tdt} tensor of at least {nb * block * block} values")
        _lib.check(fn(self._h, block, _ptr(out), _stream_ptr(stream)))
        return out

    def block_diagonal(self, block, out=None, stream=None):
        """the block x block diagonal blocks of the matrix (cfs_hip_sym_block_diagonal_async): a device
        tensor (ceil(n / block), block, block) of the value type, both triangles, 0 where the matrix
        stores nothing and outside the matrix in a trailing partial block; block one of 1, 2, 3, 4, 6.
        Gathered from the handle's device arrays (so it follows update_values).  A whole-matrix handle
        on one device.  `out`: a device tensor to fill instead of a new one."""
        return self._blocks(_lib.load().cfs_hip_sym_block_diagonal_async, block, out, stream)

    def block_inverse(self, block, out=None, stream=None):
        """the inverse blocks pcg(precond="block_jacobi", block=block) would use now
        (cfs_hip_sym_block_inverse_async), same shape as block_diagonal(); identity outside the
        matrix in a trailing partial block.  For developers and tests."""
        return self._blocks(_lib.load().cfs_hip_sym_block_inverse_async, block, out, stream)

    def pcg(self, u, b, precond="jacobi", tol=1e-10, maxiter=1000, check_every=8, stream=None, block=3):
        """preconditioned conjugate gradients inside the library (cfs_hip_sym_pcg): like cg(), with
        precond = "jacobi" (the diagonal of the handle; it must be positive), "none" (exactly
        cg()) or "block_jacobi" (cfs_hip_sym_pcg_block: the block x block diagonal blocks, block one
        of 1, 2, 3, 4, 6; they must be positive definite; block = 1 is "jacobi").  Stops on the
        unpreconditioned residual ||r|| <= tol ||b||.  Returns (iterations, ||b - A u|| / ||b||)."""
        if precond == "block_jacobi":
            it, res = C.c_int(), C.c_double()
            _lib.check(_lib.load().cfs_hip_sym_pcg_block(self._h, _ptr(u), _ptr(b), int(block), float(tol), int(maxiter),
                                                         int(check_every), C.byref(it), C.byref(res), _stream_ptr(stream)))
            return it.value, res.value
        if isinstance(precond, str):
            if precond not in PRECOND:
                raise ValueError(f"unknown preconditioner {precond!r}: one of {sorted(PRECOND)}")
            precond = PRECOND[precond]
        it, res = C.c_int(), C.c_double()
        _lib.check(_lib.load().cfs_hip_sym_pcg(self._h, _ptr(u), _ptr(b), int(precond), float(tol), int(maxiter),
                                               int(check_every), C.byref(it), C.byref(res), _stream_ptr(stream)))
        return it.value, res.value

    @staticmethod
    def _cheb_base(base, block):
        """block_rows of the Chebyshev entry points: 0 none, 1 Jacobi, `block` block Jacobi"""
        if isinstance(base, str):
            if base not in LOBPCG_PRECOND:
                raise ValueError(f"unknown base preconditioner {base!r}: one of {sorted(LOBPCG_PRECOND)}")
            return int(block) if base == "block_jacobi" else LOBPCG_PRECOND[base]
        return int(base)

    def pcg_cheb(self, u, b, base="jacobi", block=3, degree=4, lmin=None, lmax=None, tol=1e-10, maxiter=1000,
                 check_every=8, stream=None):
        """PCG with a Chebyshev polynomial of `degree` (1 .. 16) in M^-1 A as the preconditioner
        (cfs_hip_sym_pcg_cheb): M from base = "none", "jacobi" or "block_jacobi" (block one of 1, 2, 3, 4, 6).
        degree - 1 products per application and no dot product inside it; 5 + 3 (degree - 1) launches per outer
        iteration.  lmax None: 1.1 x the power-method estimate of lambda_max(M^-1 A) (precond_lmax()); lmin None:
        lmax / 30.  The polynomial is positive definite as long as the spectrum of M^-1 A lies in (0, lmin + lmax).
        Stops on the unpreconditioned residual ||r|| <= tol ||b||.  Returns (iterations, ||b - A u|| / ||b||,
        (lmin, lmax) actually used -- pass them to the next solve with the same matrix)."""
        it, res, used = C.c_int(), C.c_double(), (C.c_double * 2)()
        _lib.check(_lib.load().cfs_hip_sym_pcg_cheb(
            self._h, _ptr(u), _ptr(b), self._cheb_base(base, block), int(degree), float(lmin or 0.0), float(lmax or 0.0),
            float(tol), int(maxiter), int(check_every), C.byref(it), C.byref(res), used, _stream_ptr(stream)))
        return it.value, res.value, (used[0], used[1])

    def cheb_apply(self, z, r, lmin, lmax, base="jacobi", block=3, degree=4, stream=None):
        """z <- P_m r, the polynomial of pcg_cheb() alone (cfs_hip_sym_cheb_apply): device tensors of nrows()
        values, both bounds required.  Returns z."""
        _lib.check(_lib.load().cfs_hip_sym_cheb_apply(self._h, self._cheb_base(base, block), int(degree), float(lmin),
                                                      float(lmax), _ptr(z), _ptr(r), _stream_ptr(stream)))
        return z

    def precond_lmax(self, base="jacobi", block=3, steps=16, v0=None, stream=None):
        """a lower estimate of lambda_max(M^-1 A) by `steps` power steps (cfs_hip_sym_precond_lmax), M as for
        pcg_cheb(); v0: a device tensor of nrows() values (None: the library's fixed start vector)."""
        est = C.c_double()
        _lib.check(_lib.load().cfs_hip_sym_precond_lmax(self._h, self._cheb_base(base, block), int(steps),
                                                        _ptr(v0) if v0 is not None else None, C.byref(est),
                                                        _stream_ptr(stream)))
        return est.value

    def amg(self, rowptr, colind, values, passes=2, degree=1, ratio=4.0, coarse_max=512, refreshable=False, matching="greedy",
            setup="host", block=1):
        """the aggregation multigrid hierarchy of this matrix (cfs_hip_amg_create_*), an Amg: rowptr, colind, values
        are the CSR the handle was created from (only entries with col <= row are read; the caller vouches that it is
        this handle's matrix).  passes 1 .. 3 rounds of pairwise matching per level, degree 1 .. 4 of the Chebyshev
        smoother, ratio = lmax / lmin of its interval, coarse_max <= 1024 the largest dense last level.  A whole-matrix
        handle on one device.  The hierarchy holds the values of now: to follow update_values() make it with
        refreshable=True (cfs_hip_amg_create_refreshable_*; the matrix needs FLAG_KEEP_VALUE_MAP) and call
        Amg.update_values() with the same array.
        matching: "greedy" (the rows in ascending order, each takes its strongest free neighbour) or "dominant" (the
        locally dominant matching of cfs_hip.h, parallel by definition: usually more iterations, and the only one with
        setup="device", where the hierarchy is built by kernels on the device -- the hierarchy of matching="dominant",
        setup="host" in every bit, in a fraction of the time).  setup="device" with matching="greedy" and a refreshable
        hierarchy with matching="dominant" do not exist: ValueError.
        block = 2, 3, 4 or 6: the node-block form (cfs_hip_amg_create_block_*) for a multi-dof mesh matrix whose
        `block` consecutive rows are one node -- the nodes are aggregated, the transfers carry W_i = D_i^-1/2 of the node
        blocks and the smoother is block Jacobi; n must be a multiple of block.  Host-built and not refreshable:
        refreshable=True or setup="device" with block > 1 is a ValueError.  pcg_amg() and Amg.apply() take it unchanged."""
        return Amg(self, rowptr, colind, values, passes=passes, degree=degree, ratio=ratio, coarse_max=coarse_max,
                   refreshable=refreshable, matching=matching, setup=setup, block=block)

    def pcg_amg(self, u, b, amg, tol=1e-10, maxiter=1000, check_every=1, stream=None):
        """PCG with one V-cycle of `amg` (self.amg(...)) as the preconditioner (cfs_hip_sym_pcg_amg): like
        pcg_cheb(), the polynomial replaced by the cycle; the host looks at the convergence flag after every
        iteration whatever check_every says.  Returns (iterations, ||b - A u|| / ||b||)."""
        it, res = C.c_int(), C.c_double()
        _lib.check(_lib.load().cfs_hip_sym_pcg_amg(self._h, amg._a, _ptr(u), _ptr(b), float(tol), int(maxiter),
                                                   int(check_every), C.byref(it), C.byref(res), _stream_ptr(stream)))
        return it.value, res.value

    @staticmethod
    def _block_layout(U, B):
        """(ld, ncols) of two 2-D blocks stored by columns, strides (1, ld), as Amg.apply takes them; ValueError otherwise"""
        if U.dim() != 2 or B.dim() != 2 or U.shape != B.shape or U.dtype != B.dtype:
            raise ValueError("U and B are both 2-D blocks of the same shape and type")
        ncols = int(U.shape[1])
        ld = int(U.stride(1)) if ncols > 1 else max(int(U.shape[0]), 1)
        for t in (U, B):
            if (U.shape[0] > 1 and t.stride(0) != 1) or (ncols > 1 and t.stride(1) != ld):
                raise ValueError("a block is stored by columns: strides (1, ld), the same ld for U and B")
        return ld, ncols

    def pcg_cols(self, U, B, precond="jacobi", block=3, tol=1e-10, maxiter=1000, check_every=8, stream=None):
        """preconditioned CG on a block of right-hand sides inside the library (cfs_hip_sym_pcg_cols): A U_c = B_c for
        the columns of the 2-D device blocks U (in: the first guesses, out: the solutions) and B, shape (n, ncols),
        strides (1, ld) as Amg.apply() takes them, ncols <= 16.  precond = "none", "jacobi" or "block_jacobi" (block one
        of 1, 2, 3, 4, 6), or G, an Amg of this matrix (cfs_hip_sym_pcg_amg_cols: one column-blocked cycle per
        iteration).  Every column runs the recurrence of pcg() / pcg_amg() and stops by its rule on its own; the set-up
        runs once, the products stay one per active column and every vector kernel runs once for the block.  Returns
        (iterations, relres): numpy arrays of ncols entries, what pcg() returns per column.  ValueError, before any
        device work, for blocks that are not 2-D, differ in shape or type, or are not stored by columns with one ld."""
        ld, ncols = SymMatrix._block_layout(U, B)
        amg = precond if isinstance(precond, Amg) else None
        if amg is not None:
            if amg.A is not self:
                raise ValueError("the hierarchy was made for another matrix")
        elif isinstance(precond, str):
            if precond == "amg":
                raise ValueError('precond="amg" needs the hierarchy: pass it as precond (precond=A.amg(...)), or call '
                                 'solver.pcg_cols_native(A, B, precond="amg", amg=G)')
            if precond not in LOBPCG_PRECOND:
                raise ValueError(f"unknown preconditioner {precond!r}: one of {sorted(LOBPCG_PRECOND)}")
            block_rows = int(block) if precond == "block_jacobi" else LOBPCG_PRECOND[precond]
        else:
            block_rows = int(precond)
        it, res = np.zeros(max(ncols, 1), np.int32), np.zeros(max(ncols, 1), np.float64)
        ip, dp = C.POINTER(C.c_int), C.POINTER(C.c_double)
        if amg is not None:
            _lib.check(_lib.load().cfs_hip_sym_pcg_amg_cols(
                self._h, amg._a, _ptr(U), _ptr(B), ld, ncols, float(tol), int(maxiter), int(check_every), it.ctypes.data_as(ip),
                res.ctypes.data_as(dp), _stream_ptr(stream)))
        else:
            _lib.check(_lib.load().cfs_hip_sym_pcg_cols(
                self._h, _ptr(U), _ptr(B), ld, ncols, block_rows, float(tol), int(maxiter), int(check_every),
                it.ctypes.data_as(ip), res.ctypes.data_as(dp), _stream_ptr(stream)))
        return it[:ncols], res[:ncols]

    def minres(self, u, b, precond="none", shift=0.0, tol=1e-10, maxiter=1000, check_every=8, stream=None):
        """MINRES inside the library (cfs_hip_sym_minres): u (device tensor) holds the first guess and
        receives the solution of (A - shift I) u = b, A symmetric and possibly indefinite; five launches per
        iteration, no host round trip inside the loop.  precond = "none", or "jacobi": M = |diag(A) - shift|
        (every entry must be nonzero).  Stops when the recurrence's residual, in the M^-1 norm, is at most
        tol times that norm of b -- with "none", ||r|| <= tol ||b||.  Returns (iterations,
        ||b - (A - shift I) u|| / ||b||)."""
        if isinstance(precond, str):
            if precond not in PRECOND:
                raise ValueError(f"unknown preconditioner {precond!r}: one of {sorted(PRECOND)}")
            precond = PRECOND[precond]
        it, res = C.c_int(), C.c_double()
        _lib.check(_lib.load().cfs_hip_sym_minres(self._h, _ptr(u), _ptr(b), int(precond), float(shift), float(tol),
                                                  int(maxiter), int(check_every), C.byref(it), C.byref(res),
                                                  _stream_ptr(stream)))
        return it.value, res.value

    def eigs(self, k=6, which="LA", ncv=None, tol=1e-10, max_restarts=100, v0=None, vectors=True, stream=None):
        """k extreme eigenpairs inside the library (cfs_hip_sym_eigs): thick-restart Lanczos with full
        re-orthogonalisation on a basis of ncv device vectors (None: min(n, max(2 k + 1, 20))), no host round trip
        inside a step.  which = "LA" (largest algebraic), "SA" (smallest algebraic) or "LM" (largest magnitude); v0: a
        device tensor of n values (None: the library's fixed start vector).  Returns (w, X, info): w a numpy float64
        array (k,) ordered by `which`; X a device tensor (n, k) with strides (1, ld) whose columns are the vectors, or
        None with vectors=False; info = dict(nconv, restarts, products, residuals) -- residuals recomputed from the
        returned vectors, the Lanczos estimates without them."""
        import torch
        if isinstance(which, str):
            if which not in EIGS_WHICH:
                raise ValueError(f"unknown which {which!r}: one of {sorted(EIGS_WHICH)}")
            which = EIGS_WHICH[which]
        k = int(k)
        tdt = torch.float64 if self.dtype == np.float64 else torch.float32
        w, res = np.zeros(max(k, 0), np.float64), np.zeros(max(k, 0), np.float64)
        X, ld = None, 0
        if vectors:
            per = 16 // self.dtype.itemsize
            ld = -(-self.nrows() // per) * per
            X = torch.zeros(max(k, 1) * ld, dtype=tdt, device="cuda")
        dp = C.POINTER(C.c_double)
        nconv, restarts, products = C.c_int(), C.c_int(), C.c_int()
        _lib.check(_lib.load().cfs_hip_sym_eigs(
            self._h, k, int(which), int(ncv or 0), float(tol), int(max_restarts), _ptr(v0) if v0 is not None else None,
            w.ctypes.data_as(dp), _ptr(X) if X is not None else None, ld, res.ctypes.data_as(dp), C.byref(nconv),
            C.byref(restarts), C.byref(products), _stream_ptr(stream)))
        if X is not None:
            X = torch.as_strided(X, (self.nrows(), k), (1, ld))
        return w, X, {"nconv": nconv.value, "restarts": restarts.value, "products": products.value, "residuals": res}

    def _pencil_b(self, B):
        """the B of a pencil (A, B): a SymMatrix of this matrix's n and dtype, else ValueError -- before any device work"""
        if not isinstance(B, SymMatrix):
            raise ValueError(f"B must be a SymMatrix (a diagonal B is a handle like any other), not {type(B).__name__}")
        if B.nrows() != self.nrows() or B.dtype != self.dtype:
            raise ValueError(f"B must have the n and the dtype of A: B is {B.nrows()} x {B.nrows()} {np.dtype(B.dtype).name}, "
                             f"A {self.nrows()} x {self.nrows()} {np.dtype(self.dtype).name}")
        return B

    def lobpcg(self, k=6, precond="jacobi", block=3, tol=1e-10, scale=None, maxiter=500, x0=None, stream=None):
        """the k smallest (algebraic) eigenpairs inside the library (cfs_hip_sym_lobpcg): LOBPCG on blocks of 3 k
        device columns with the preconditioners of pcg() -- precond = "none", "jacobi" or "block_jacobi" (block one
        of 1, 2, 3, 4, 6) -- k products per iteration, two host looks per iteration.  Pair i has converged when
        ||A x_i - theta_i x_i|| / ||x_i|| <= tol scale; scale: an estimate of ||A||_2 (None: |theta| of
        self.eigs(k=1, which="LM", tol=1e-3), whose products are not counted).  x0: a device tensor (n, k) whose
        columns are the start block (any strides; None: the library's fixed start block).  Returns (w, X, info): w a
        numpy float64 array (k,), ascending; X a device tensor (n, k) with strides (1, ld); info = dict(nconv,
        iterations, products, residuals) -- residuals recomputed from the returned vectors.
        precond = G, an Amg of this matrix (self.amg(...)): one column-blocked multigrid cycle per iteration forms W on the
        pairs still active (cfs_hip_sym_lobpcg_amg); info then also has "cycles", the cycles applied, one per column.
        The name "amg" alone is a ValueError here -- this method has no argument for the hierarchy -- and
        solver.lobpcg_native(A, k, precond="amg", amg=G) is the spelling by name.
        The pencil A x = lambda B x: lobpcg_gen(B, ...) below -- this method keeps its argument list."""
        return SymMatrix._lobpcg(self, None, k, precond, block, tol, scale, maxiter, x0, stream)

    def lobpcg_gen(self, B, k=6, precond="jacobi", block=3, tol=1e-10, scale=None, maxiter=500, x0=None, stream=None):
        """the k smallest eigenpairs of the PENCIL A x = lambda B x (cfs_hip_sym_lobpcg_gen; with precond = G, an Amg of
        this matrix, cfs_hip_sym_lobpcg_gen_amg) -- K x = lambda M x with a mass matrix.  B: a SymMatrix of the same n and
        dtype (else ValueError, before any device work), symmetric positive definite; B = self is allowed, and a lumped
        (diagonal) B is a handle like any other.  Every other argument and the return value as for lobpcg().  Pair i has
        converged when ||A x_i - theta_i B x_i|| / ||x_i|| <= tol scale (scale still an estimate of ||A||_2); the columns
        of X are B-orthonormal; the preconditioner is still built from A; info also has "b_products", the products with B
        ("products" counts those with A).  solver.lobpcg_native(A, k, ..., B=B) is the same call."""
        return SymMatrix._lobpcg(self, SymMatrix._pencil_b(self, B), k, precond, block, tol, scale, maxiter, x0, stream)

    def _lobpcg(self, B, k, precond, block, tol, scale, maxiter, x0, stream):
        """lobpcg() (B = None) and lobpcg_gen() behind their argument lists"""
        import torch
        amg = precond if isinstance(precond, Amg) else None
        if amg is not None:
            if amg.A is not self:
                raise ValueError("the hierarchy was made for another matrix")
            block_rows = 0
        elif isinstance(precond, str):
            if precond == "amg":
                raise ValueError('precond="amg" needs the hierarchy: pass it as precond (precond=A.amg(...)), or call '
                                 'solver.lobpcg_native(A, k, precond="amg", amg=G)')
            if precond not in LOBPCG_PRECOND:
                raise ValueError(f"unknown preconditioner {precond!r}: one of {sorted(LOBPCG_PRECOND)}")
            block_rows = int(block) if precond == "block_jacobi" else LOBPCG_PRECOND[precond]
        else:
            block_rows = int(precond)
        k = int(k)
        if scale is None:
            scale = abs(float(self.eigs(k=1, which="LM", tol=1e-3, vectors=False, stream=stream)[0][0]))
        tdt = torch.float64 if self.dtype == np.float64 else torch.float32
        n = self.nrows()
        per = 16 // self.dtype.itemsize
        ld = -(-n // per) * per
        w, res = np.zeros(max(k, 0), np.float64), np.zeros(max(k, 0), np.float64)
        X = torch.zeros(max(k, 1) * ld, dtype=tdt, device="cuda")
        x0buf = None
        if x0 is not None:
            if x0.dtype != tdt or tuple(x0.shape) != (n, k):
                raise ValueError(f"x0 must be a {tdt} tensor of shape ({n}, {k})")
            x0buf = torch.zeros(k * ld, dtype=tdt, device="cuda")
            torch.as_strided(x0buf, (n, k), (1, ld)).copy_(x0)
        dp = C.POINTER(C.c_double)
        nconv, iterations, products, b_products = C.c_int(), C.c_int(), C.c_int(), C.c_int()
        if B is not None:
            before = amg.column_cycles() if amg is not None else 0
            tail = (float(tol), float(scale), int(maxiter), _ptr(x0buf) if x0buf is not None else None, ld, w.ctypes.data_as(dp),
                    _ptr(X), ld, res.ctypes.data_as(dp), C.byref(nconv), C.byref(iterations), C.byref(products), C.byref(b_products),
                    _stream_ptr(stream))
            if amg is not None:
                _lib.check(_lib.load().cfs_hip_sym_lobpcg_gen_amg(self._h, B._h, amg._a, k, *tail))
            else:
                _lib.check(_lib.load().cfs_hip_sym_lobpcg_gen(self._h, B._h, k, block_rows, *tail))
            info = {"nconv": nconv.value, "iterations": iterations.value, "products": products.value, "residuals": res,
                    "b_products": b_products.value}
            if amg is not None:
                info["cycles"] = amg.column_cycles() - before
            return w, torch.as_strided(X, (n, k), (1, ld)), info
        if amg is not None:
            before = amg.column_cycles()
            _lib.check(_lib.load().cfs_hip_sym_lobpcg_amg(
                self._h, amg._a, k, float(tol), float(scale), int(maxiter), _ptr(x0buf) if x0buf is not None else None, ld,
                w.ctypes.data_as(dp), _ptr(X), ld, res.ctypes.data_as(dp), C.byref(nconv), C.byref(iterations),
                C.byref(products), _stream_ptr(stream)))
            X = torch.as_strided(X, (n, k), (1, ld))
            return w, X, {"nconv": nconv.value, "iterations": iterations.value, "products": products.value, "residuals": res,
                          "cycles": amg.column_cycles() - before}
        _lib.check(_lib.load().cfs_hip_sym_lobpcg(
            self._h, k, block_rows, float(tol), float(scale), int(maxiter), _ptr(x0buf) if x0buf is not None else None, ld,
            w.ctypes.data_as(dp), _ptr(X), ld, res.ctypes.data_as(dp), C.byref(nconv), C.byref(iterations),
            C.byref(products), _stream_ptr(stream)))
        X = torch.as_strided(X, (n, k), (1, ld))
        return w, X, {"nconv": nconv.value, "iterations": iterations.value, "products": products.value, "residuals": res}

    def debug_lobpcg(self, k, block_rows, iters, x0=None, stream=None, B=None):
        """developer / test: iteration 0 and `iters` more of the solver's own kernels, every pair active
        (cfs_hip_sym_debug_lobpcg; with B, the pencil form cfs_hip_sym_debug_lobpcg_gen).  Returns (theta, X, resnorms)."""
        import torch
        if B is not None:
            self._pencil_b(B)
        tdt = torch.float64 if self.dtype == np.float64 else torch.float32
        n = self.nrows()
        per = 16 // self.dtype.itemsize
        ld = -(-n // per) * per
        theta, res = np.zeros(k), np.zeros(k)
        X = torch.zeros(k * ld, dtype=tdt, device="cuda")
        x0buf = None
        if x0 is not None:
            x0buf = torch.zeros(k * ld, dtype=tdt, device="cuda")
            torch.as_strided(x0buf, (n, k), (1, ld)).copy_(x0)
        dp = C.POINTER(C.c_double)
        tail = (int(k), int(block_rows), _ptr(x0buf) if x0buf is not None else None, ld, int(iters), theta.ctypes.data_as(dp), _ptr(X),
                ld, res.ctypes.data_as(dp), _stream_ptr(stream))
        if B is not None:
            _lib.check(_lib.load().cfs_hip_sym_debug_lobpcg_gen(self._h, B._h, *tail))
        else:
            _lib.check(_lib.load().cfs_hip_sym_debug_lobpcg(self._h, *tail))
        return theta, torch.as_strided(X, (n, k), (1, ld)), res

    def debug_lobpcg_amg(self, amg, k, iters, x0=None, stream=None):
        """developer / test: debug_lobpcg() with W formed by the blocked cycle of `amg` (cfs_hip_sym_debug_lobpcg_amg).
        Returns (theta, X, resnorms)."""
        import torch
        tdt = torch.float64 if self.dtype == np.float64 else torch.float32
        n = self.nrows()
        per = 16 // self.dtype.itemsize
        ld = -(-n // per) * per
        theta, res = np.zeros(k), np.zeros(k)
        X = torch.zeros(k * ld, dtype=tdt, device="cuda")
        x0buf = None
        if x0 is not None:
            x0buf = torch.zeros(k * ld, dtype=tdt, device="cuda")
            torch.as_strided(x0buf, (n, k), (1, ld)).copy_(x0)
        dp = C.POINTER(C.c_double)
        _lib.check(_lib.load().cfs_hip_sym_debug_lobpcg_amg(
            self._h, amg._a, int(k), _ptr(x0buf) if x0buf is not None else None, ld, int(iters),
            theta.ctypes.data_as(dp), _ptr(X), ld, res.ctypes.data_as(dp), _stream_ptr(stream)))
        return theta, torch.as_strided(X, (n, k), (1, ld)), res

    # -- the exchange of a one-process multi-device handle (ngpus > 1, FLAG_SHARD_EXCHANGE) --
    def set_exchange(self, form):
        """"sparse": one packed all-to-all per SpMV (cfs_hip_comm_alltoallv); "reduce_scatter": the
        dense reduce-scatter.  Switchable at any time (cfs_hip_sym_multi_set_exchange)."""
        if isinstance(form, str):
            if form not in EXCHANGE:
                raise ValueError(f"unknown exchange form {form!r}: one of {sorted(EXCHANGE)}")
            form = EXCHANGE[form]
        _lib.check(_lib.load().cfs_hip_sym_multi_set_exchange(self._h, int(form)))

    def exchange_info(self):
        """dict(form, values_moved, bytes_moved): the current form and what the ranks hand to the
        collective per SpMV under it (cfs_hip_sym_multi_exchange_info)"""
        form, vals, nbytes = C.c_int(), C.c_int64(), C.c_int64()
        _lib.check(_lib.load().cfs_hip_sym_multi_exchange_info(self._h, C.byref(form), C.byref(vals), C.byref(nbytes)))
        return {"form": form.value, "values_moved": vals.value, "bytes_moved": nbytes.value}

    # -- sharded operation --
    def send_counts(self):
        out = np.zeros(self.nranks, dtype=np.int32)
        _lib.check(_lib.load().cfs_hip_sym_shard_send_counts(self._h, out.ctypes.data))
        return out

    def send_rows(self):
        out = np.zeros(int(self.stats()["remote_vals"]), dtype=np.int32)
        if out.size:
            _lib.check(_lib.load().cfs_hip_sym_shard_send_rows(self._h, out.ctypes.data))
        return out

    def set_recv(self, recv_rows):
        recv_rows = _np_i32(recv_rows)
        _lib.check(_lib.load().cfs_hip_sym_shard_set_recv(
            self._h, recv_rows.size, recv_rows.ctypes.data if recv_rows.size else None))

    def spmv_local(self, y_block, x, send_buf, stream=None):
        _lib.check(_lib.load().cfs_hip_sym_spmv_local_async(
            self._h, _ptr(y_block), _ptr(x), _ptr(send_buf) if send_buf is not None else None,
            _stream_ptr(stream)))

    def spmv_phases(self, y_block, x, send_buf, phases, stream=None):
        """enqueue only the selected launches (1 = tile kernel, 2 = halo fold, 4 = pack)"""
        _lib.check(_lib.load().cfs_hip_sym_spmv_phases_async(
            self._h, _ptr(y_block), _ptr(x), _ptr(send_buf) if send_buf is not None else None,
            int(phases), _stream_ptr(stream)))

    def recv_fold(self, y_block, recv_buf, stream=None):
        _lib.check(_lib.load().cfs_hip_sym_recv_fold_async(
            self._h, _ptr(y_block), _ptr(recv_buf) if recv_buf is not None else None,
            _stream_ptr(stream)))

    def update_values(self, values):
        """new values, same sparsity pattern (numpy array or device tensor in the order of the
        CSR the matrix was created from); needs FLAG_KEEP_VALUE_MAP at construction"""
        suf = "f64" if self.dtype == np.float64 else "f32"
        if isinstance(values, np.ndarray):
            values = np.ascontiguousarray(values, dtype=self.dtype)
            ptr, cnt = values.ctypes.data, values.size
        else:
            ptr, cnt = values.data_ptr(), values.numel()
        _lib.check(getattr(_lib.load(), "cfs_hip_sym_update_values_" + suf)(self._h, ptr, cnt))

    def close(self):
        if getattr(self, "_h", None) and self._h.value:
            _lib.load().cfs_hip_sym_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Amg:
    """The aggregation multigrid hierarchy of a SymMatrix (cfs_hip_amg_create_*) and its V-cycle.  Keeps a reference
    to its matrix, which must stay open for as long as the hierarchy is used."""

    def __init__(self, A, rowptr, colind, values, passes=2, degree=1, ratio=4.0, coarse_max=512, refreshable=False,
                 matching="greedy", setup="host", block=1):
        if matching not in ("greedy", "dominant") or setup not in ("host", "device"):
            raise ValueError(f'matching is "greedy" or "dominant" and setup "host" or "device", got {matching!r}, {setup!r}')
        if block != 1 and (refreshable or setup == "device"):
            raise ValueError(f"a node-block hierarchy (block={block}) is built on the host and is not refreshable")
        if setup == "device" and matching == "greedy":
            raise ValueError('setup="device" needs matching="dominant": the greedy matching has no parallel form')
        if refreshable and matching != "greedy":
            raise ValueError("a refreshable hierarchy is made with the greedy matching on the host")
        lib = _lib.load()
        rowptr, colind = _np_i32(rowptr), _np_i32(colind)
        values = np.ascontiguousarray(values, dtype=A.dtype)
        self.A, self.dtype = A, A.dtype
        self._a = C.c_void_p()
        opt = _lib.AmgOptions(int(passes), int(degree), int(coarse_max), 0, float(ratio))
        suf = "f64" if self.dtype == np.float64 else "f32"
        self.refreshable = bool(refreshable)
        kind = "refreshable_" if refreshable else "device_" if setup == "device" else "dominant_" if matching == "dominant" else ""
        if block != 1:  # (block = 1 through this entry point is the scalar create itself; the scalar names stay in use)
            create = getattr(lib, "cfs_hip_amg_create_block_" + suf)
            _lib.check(create(A._h, A.n, rowptr.ctypes.data, colind.ctypes.data, values.ctypes.data, int(block),
                              1 if matching == "dominant" else 0, C.byref(opt), C.byref(self._a)))
            return
        create = getattr(lib, "cfs_hip_amg_create_" + kind + suf)
        _lib.check(create(A._h, A.n, rowptr.ctypes.data, colind.ctypes.data, values.ctypes.data, C.byref(opt), C.byref(self._a)))

    def info(self):
        """dict: levels, the options used, device_bytes, setup_seconds (of which handles_seconds for the create path
        of the level handles), per level n, nnz (stored), lmin, lmax, kind (0 multigrid, 1 smoother-only,
        2 dense), and block, the rows per node (1: the scalar form)"""
        out, blk = _lib.AmgInfo(), C.c_int()
        lib = _lib.load()
        _lib.check(lib.cfs_hip_amg_info(self._a, C.byref(out)))
        _lib.check(lib.cfs_hip_amg_block(self._a, C.byref(blk)))
        return dict(out.asdict(), block=blk.value)

    def setup_info(self):
        """dict (cfs_hip_amg_setup_info): matching ("greedy" / "dominant"), setup ("host" / "device"), lower_on_host (a
        device set-up whose level 0 was read on the host: unsorted rows or duplicates), rounds (per level that has a
        coarser one, the rounds of every pass), split_seconds of a device set-up (lower, matching, galerkin, download)
        and scratch_bytes, the device scratch it held"""
        inf = self.info()
        mt, dev, sb = C.c_int(), C.c_int(), C.c_longlong()
        rounds, sec = (C.c_int * (3 * _lib.AMG_MAX_LEVELS))(), (C.c_double * 4)()
        _lib.check(_lib.load().cfs_hip_amg_setup_info(self._a, C.byref(mt), C.byref(dev), rounds, sec, C.byref(sb)))
        return dict(matching=("greedy", "dominant")[mt.value], setup="device" if dev.value else "host", lower_on_host=dev.value == 2,
                    rounds=[list(rounds[3 * l:3 * l + inf["passes"]]) for l in range(inf["levels"] - 1)],
                    split_seconds=dict(zip(("lower", "matching", "galerkin", "download"), list(sec))), scratch_bytes=sb.value)

    def update_values(self, values):
        """new values, same sparsity pattern, for a refreshable hierarchy (cfs_hip_amg_update_values_*): a numpy array or
        a contiguous device tensor of the hierarchy's value type, in the order of the CSR given at construction.  The
        aggregates stay; every level's weights, matrix, bounds and the dense inverse are made again on the device."""
        suf = "f64" if self.dtype == np.float64 else "f32"
        if isinstance(values, np.ndarray):
            values = np.ascontiguousarray(values, dtype=self.dtype)
            ptr, cnt = values.ctypes.data, values.size
        else:
            if values.element_size() != np.dtype(self.dtype).itemsize or not values.is_floating_point():
                raise TypeError(f"the hierarchy holds {np.dtype(self.dtype).name} values, the tensor is {values.dtype}")
            if not values.is_contiguous():
                raise ValueError("a device tensor of values must be contiguous")
            ptr, cnt = values.data_ptr(), values.numel()
        _lib.check(getattr(_lib.load(), "cfs_hip_amg_update_values_" + suf)(self._a, ptr, cnt))

    def refresh_info(self):
        """dict: map_bytes (the device bytes being refreshable adds), refreshes (successful ones), last_seconds, and
        split_seconds of the last one: galerkin, pour, power, dense"""
        mb, cnt, sec, split = C.c_longlong(), C.c_int(), C.c_double(), (C.c_double * 4)()
        lib = _lib.load()
        _lib.check(lib.cfs_hip_amg_refresh_info(self._a, C.byref(mb), C.byref(cnt), C.byref(sec)))
        _lib.check(lib.cfs_hip_debug_amg_refresh_split(self._a, split))
        return dict(map_bytes=mb.value, refreshes=cnt.value, last_seconds=sec.value,
                    split_seconds=dict(zip(("galerkin", "pour", "power", "dense"), list(split))))

    def aggregates(self, level):
        """(agg, w) of a level that has a coarser one, as the device holds them: the aggregate of every row and the
        weights in the value type"""
        inf = self.info()
        n = inf["n"][level] if 0 <= level < inf["levels"] else 0
        agg, w = np.zeros(n, np.int32), np.zeros(n, self.dtype)
        if inf["block"] != 1:  # (agg is the map of the unknowns; the weights are node_weights())
            _lib.check(_lib.load().cfs_hip_amg_level_aggregates(self._a, int(level), agg.ctypes.data, None))
            return agg, None
        _lib.check(_lib.load().cfs_hip_amg_level_aggregates(self._a, int(level), agg.ctypes.data, w.ctypes.data))
        return agg, w

    def node_weights(self, level):
        """W of a level of a node-block hierarchy that has a coarser one (cfs_hip_amg_level_node_weights): an
        (n_l / block, block, block) array of the symmetric W_i = D_i^-1/2 in the value type, as the device holds them"""
        inf = self.info()
        bs = inf["block"]
        n = inf["n"][level] if 0 <= level < inf["levels"] else 0
        W = np.zeros((n // bs, bs, bs), self.dtype)
        _lib.check(_lib.load().cfs_hip_amg_level_node_weights(self._a, int(level), W.ctypes.data))
        return W

    def level_matrix(self, level):
        """(n, rowptr, colind, values) of level >= 1: the lower triangle + diagonal its handle was created from"""
        inf = self.info()
        ok = 1 <= level < inf["levels"]
        n, nnz = (inf["n"][level], inf["nnz"][level]) if ok else (0, 0)
        rp, ci, va = np.zeros(n + 1, np.int32), np.zeros(nnz, np.int32), np.zeros(nnz, self.dtype)
        _lib.check(_lib.load().cfs_hip_amg_level_matrix(self._a, int(level), rp.ctypes.data, ci.ctypes.data, va.ctypes.data))
        return n, rp, ci, va

    def coarse_inverse(self):
        """the (n_L, n_L) inverse of the dense last level as the device holds it"""
        inf = self.info()
        n = inf["n"][-1]
        inv = np.zeros((n, n), self.dtype)
        _lib.check(_lib.load().cfs_hip_amg_coarse_inverse(self._a, inv.ctypes.data))
        return inv

    def apply(self, z, r, *, active=None, stream=None):
        """z <- M^-1 r, one cycle.  1-D device tensors of n values: cfs_hip_amg_apply.  2-D blocks (n, ncols) in the
        column layout SymMatrix.lobpcg uses -- strides (1, ld), ld >= n and, for more than one column, ld a multiple
        of 16 bytes: the column-blocked cycle (cfs_hip_amg_apply_cols), every vector kernel once for the block.
        active: a bit mask of the columns to work on (None: all); the others are neither read nor written.
        Returns z."""
        if z.dim() == 1 and r.dim() == 1:
            if active is not None:
                raise ValueError("active names columns of a 2-D block")
            _lib.check(_lib.load().cfs_hip_amg_apply(self._a, _ptr(z), _ptr(r), _stream_ptr(stream)))
            return z
        if z.dim() != 2 or r.dim() != 2 or z.shape != r.shape or z.dtype != r.dtype:
            raise ValueError("z and r are both 1-D vectors, or both 2-D blocks of the same shape and type")
        ncols = int(z.shape[1])
        ld = int(z.stride(1)) if ncols > 1 else max(int(z.shape[0]), 1)
        for t in (z, r):
            if (z.shape[0] > 1 and t.stride(0) != 1) or (ncols > 1 and t.stride(1) != ld):
                raise ValueError("a block is stored by columns: strides (1, ld), the same ld for z and r")
        mask = (1 << ncols) - 1 if active is None else int(active)
        if mask < 0 or mask >> 32:
            raise ValueError("active is a mask of at most 32 bits")
        _lib.check(_lib.load().cfs_hip_amg_apply_cols(self._a, _ptr(z), _ptr(r), ld, ncols, mask, _stream_ptr(stream)))
        return z

    def column_cycles(self):
        """the cycles applied to columns of blocks since the hierarchy was made (cfs_hip_amg_column_cycles)"""
        out = C.c_longlong()
        _lib.check(_lib.load().cfs_hip_amg_column_cycles(self._a, C.byref(out)))
        return out.value

    def close(self):
        if getattr(self, "_a", None) and self._a.value:
            _lib.load().cfs_hip_amg_destroy(self._a)
            self._a = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def coarsen(n, rowptr, colind, values, passes=2, matching="greedy", rounds=None, block=1):
    """host only: one level of the multigrid set-up (cfs_hip_debug_amg_coarsen, or cfs_hip_debug_amg_coarsen_dominant
    with matching="dominant").  Returns (agg, w, (nc, rowptr, colind, values)): the aggregate of every row, the weights
    1 / sqrt(a_ii) and the lower triangle + diagonal of the coarse matrix, all in fp64.  rounds (a list, dominant only):
    receives the rounds every pass ran.  block != 1: one level of the node-block form (cfs_hip_debug_amg_coarsen_block);
    w is then W, an (n / block, block, block) array of the symmetric W_i = D_i^-1/2, and agg the map of the unknowns"""
    if matching not in ("greedy", "dominant"):
        raise ValueError(f'matching is "greedy" or "dominant", got {matching!r}')
    rowptr, colind = _np_i32(rowptr), _np_i32(colind)
    values = np.ascontiguousarray(values, dtype=np.float64)
    if block != 1:
        bs = int(block)
        cap = 0
        if bs > 1 and n > 0 and int(rowptr[n]) > 0:  # a coupled pair of nodes is a full block of the coarse matrix
            rows = np.repeat(np.arange(n, dtype=np.int64), np.diff(rowptr[:n + 1]))
            cols = colind[:int(rowptr[n])].astype(np.int64)
            low = (cols >= 0) & (cols <= rows)
            cap = bs * bs * int(np.unique((rows[low] // bs) * (n // bs + 1) + cols[low] // bs).size)
        agg, W = np.zeros(max(n, 0), np.int32), np.zeros((max(n, 0) // max(bs, 1), max(bs, 1), max(bs, 1)), np.float64)
        crp, cci, cva = np.zeros(max(n, 0) + 1, np.int32), np.zeros(max(cap, 1), np.int32), np.zeros(max(cap, 1), np.float64)
        nc, nnz, rnd = C.c_int(), C.c_longlong(), (C.c_int * 3)()
        _lib.check(_lib.load().cfs_hip_debug_amg_coarsen_block(
            n, rowptr.ctypes.data, colind.ctypes.data, values.ctypes.data, bs, int(passes), 1 if matching == "dominant" else 0,
            agg.ctypes.data, W.ctypes.data, C.byref(nc), crp.ctypes.data, cci.ctypes.data, cva.ctypes.data, cap, C.byref(nnz), rnd))
        if rounds is not None and matching == "dominant":
            rounds[:] = list(rnd)[:int(passes)]
        return agg, W, (nc.value, crp[:nc.value + 1].copy(), cci[:nnz.value].copy(), cva[:nnz.value].copy())
    cap = int(rowptr[n]) if n > 0 else 0
    agg, w = np.zeros(n, np.int32), np.zeros(n, np.float64)
    crp, cci, cva = np.zeros(n + 1, np.int32), np.zeros(max(cap, 1), np.int32), np.zeros(max(cap, 1), np.float64)
    nc, nnz = C.c_int(), C.c_longlong()
    args = (n, rowptr.ctypes.data, colind.ctypes.data, values.ctypes.data, int(passes), agg.ctypes.data, w.ctypes.data, C.byref(nc),
            crp.ctypes.data, cci.ctypes.data, cva.ctypes.data, cap, C.byref(nnz))
    if matching == "dominant":
        rnd = (C.c_int * 3)()
        _lib.check(_lib.load().cfs_hip_debug_amg_coarsen_dominant(*args, rnd))
        if rounds is not None:
            rounds[:] = list(rnd)[:int(passes)]
    else:
        _lib.check(_lib.load().cfs_hip_debug_amg_coarsen(*args))
    return agg, w, (nc.value, crp[:nc.value + 1].copy(), cci[:nnz.value].copy(), cva[:nnz.value].copy())


def recoarsen(n, rowptr, colind, values_at_create, values_new, passes=2):
    """host only: one level of a refresh (cfs_hip_debug_amg_recoarsen) -- the matchings of values_at_create, frozen, the
    sums evaluated for values_new in the order the kernels add.  Returns (w, coarse values) in fp64, the values in the
    pattern coarsen() returns for values_at_create"""
    rowptr, colind = _np_i32(rowptr), _np_i32(colind)
    old, new = (np.ascontiguousarray(v, dtype=np.float64) for v in (values_at_create, values_new))
    cap = int(rowptr[n]) if n > 0 else 0
    assert old.size == new.size == cap
    w, cva = np.zeros(n, np.float64), np.zeros(max(cap, 1), np.float64)
    nnz = C.c_longlong()
    _lib.check(_lib.load().cfs_hip_debug_amg_recoarsen(n, rowptr.ctypes.data, colind.ctypes.data, old.ctypes.data, new.ctypes.data,
                                                       int(passes), w.ctypes.data, cva.ctypes.data, cap, C.byref(nnz)))
    return w, cva[:nnz.value].copy()


class MixedSym:
    """One symmetric matrix as two handles, fp64 and fp32, for the mixed-precision solver
    (cfs_hip_sym_pcg_mixed): the iteration's products run on the fp32 handle, the solution and the
    true residuals are fp64.  Both matrices stay resident: about 5/3 of the fp64 handle's memory.

    Built from one CSR with float64 values; the fp32 handle gets values.astype(float32).
    `options` go to both handles.  MixedSym.from_handles(A64, A32) wraps two existing SymMatrix
    objects instead (they stay the caller's: close() leaves them open)."""

    def __init__(self, n, rowptr, colind, values, options=None):
        values = np.ascontiguousarray(values)
        if values.dtype != np.float64:
            raise TypeError("MixedSym takes float64 values (the fp32 handle is built from values.astype(float32))")
        self.n = int(n)
        self.A64 = SymMatrix(n, rowptr, colind, values, options=options)
        try:
            self.A32 = SymMatrix(n, rowptr, colind, values.astype(np.float32), options=options)
        except Exception:
            self.A64.close()
            raise
        self._owned = True

    @classmethod
    def from_handles(cls, A64, A32):
        if A64.dtype != np.float64 or A32.dtype != np.float32:
            raise TypeError("from_handles(A64, A32): a float64 and a float32 SymMatrix, in this order")
        if A64.nrows() != A32.nrows():
            raise ValueError(f"the two matrices have {A64.nrows()} and {A32.nrows()} rows")
        self = cls.__new__(cls)
        self.n, self.A64, self.A32, self._owned = A64.nrows(), A64, A32, False
        return self

    def nrows(self):
        return self.n

    def size(self):
        return self.A64.size() + self.A32.size()

    def pcg(self, u, b, precond="jacobi", block=3, tol=1e-10, delta=0.1, maxiter=1000, check_every=8, stream=None):
        """mixed-precision PCG inside the library (cfs_hip_sym_pcg_mixed): u (float64 device tensor) holds
        the first guess and receives the solution of A u = b (float64).  precond "none", "jacobi" or
        "block_jacobi" (block one of 1, 2, 3, 4, 6), built from the fp32 handle.  delta: the drop of the
        recurrence's residual that triggers a replacement by the true fp64 residual.  Returns (fp32
        iterations, replacements, fp64 ||b - A u|| / ||b||)."""
        if precond == "block_jacobi":
            block_rows = int(block)
            if block_rows == 0:
                raise ValueError("block_jacobi needs block one of 1, 2, 3, 4, 6")
        elif precond in PRECOND:
            block_rows = PRECOND[precond]
        else:
            raise ValueError(f"unknown preconditioner {precond!r}: one of {sorted(PRECOND) + ['block_jacobi']}")
        it, rep, res = C.c_int(), C.c_int(), C.c_double()
        _lib.check(_lib.load().cfs_hip_sym_pcg_mixed(self.A64._h, self.A32._h, _ptr(u), _ptr(b), block_rows, float(tol),
                                                     float(delta), int(maxiter), int(check_every), C.byref(it), C.byref(rep),
                                                     C.byref(res), _stream_ptr(stream)))
        return it.value, rep.value, res.value

    def close(self):
        if getattr(self, "_owned", False):
            self.A64.close()
            self.A32.close()
        self._owned = False


class CsrMatrix:
    """General CSR on the GPU (Format::csr; cpu_mv's role, csr_matrix.tpp:2683-2704)."""

    def __init__(self, nrows, ncols, rowptr, colind, values):
        lib = _lib.load()
        rowptr, colind = _np_i32(rowptr), _np_i32(colind)
        values = np.ascontiguousarray(values)
        self.dtype = values.dtype
        self._nrows, self._ncols, self._nnz = int(nrows), int(ncols), int(rowptr[-1])
        suf = "f64" if self.dtype == np.float64 else "f32"
        self._h = C.c_void_p()
        _lib.check(getattr(lib, "cfs_hip_csr_create_" + suf)(
            nrows, ncols, rowptr.ctypes.data, colind.ctypes.data, values.ctypes.data,
            C.byref(self._h)))

    def nrows(self):
        return self._nrows

    def ncols(self):
        return self._ncols

    def nnz(self):
        return self._nnz

    def symmetric(self):
        return False

    def tune(self, kernel=Kernel.SpDMV, tuning=Tuning.Aggressive):
        return True

    def dense_vector_multiply(self, y, x, stream=None):
        _lib.check(_lib.load().cfs_hip_csr_spmv_async(
            self._h, _ptr(y), _ptr(x), _stream_ptr(stream)))

    def dense_vector_multiply_host(self, y, x):
        _lib.check(_lib.load().cfs_hip_csr_spmv(self._h, _ptr(y), _ptr(x)))

    # name order of cfs_hip_csr_debug_layout (CFS_HIP_CSR_LAYOUT_WORDS)
    LAYOUT_KEYS = ("blocks", "blocks_col16", "blocks_lane32", "blocks_natural", "blocks_long_row",
                   "blocks_empty", "descriptors", "chunks", "long_rows", "block_grid", "wave_grid",
                   "lw", "xcd_map")

    def layout(self):
        """developer / test: how the handle was cut (cfs_hip_csr_debug_layout), as a dict"""
        buf = (C.c_longlong * len(self.LAYOUT_KEYS))()
        _lib.check(_lib.load().cfs_hip_csr_debug_layout(self._h, buf, len(buf)))
        return dict(zip(self.LAYOUT_KEYS, (int(v) for v in buf)))

    def kernel_form(self):
        """(form, measured): 0 = block, 1 = wave; measured = the choice has been made"""
        form, measured = C.c_int(), C.c_int()
        _lib.check(_lib.load().cfs_hip_csr_kernel_form(self._h, C.byref(form), C.byref(measured)))
        return form.value, measured.value

    def narrow_nnz(self):
        """nonzeros the kept form reads through 16-bit column codes (cfs_hip_csr_stats)"""
        streamed, nar = C.c_int64(), C.c_int64()
        _lib.check(_lib.load().cfs_hip_csr_stats(self._h, C.byref(streamed), C.byref(nar)))
        return nar.value

    def close(self):
        if getattr(self, "_h", None) and self._h.value:
            _lib.load().cfs_hip_csr_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class SpDMV:
    """include/kernel/sparse_kernel.hpp:17-27: ctor tunes, call multiplies."""

    def __init__(self, A, tuning=Tuning.Aggressive):
        self.A = A
        A.tune(Kernel.SpDMV, tuning)

    def __call__(self, y, M, x, N):
        assert self.A.nrows() == M  # sparse_kernel.tpp:23-24
        assert self.A.ncols() == N
        if isinstance(y, np.ndarray):
            self.A.dense_vector_multiply_host(y, x)
        else:
            self.A.dense_vector_multiply(y, x)
