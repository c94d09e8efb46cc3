"""ctypes binding of the C ABI (include/cfs_hip.h).  No torch types cross the
boundary: tensors are handed over as raw device pointers (data_ptr())."""
import ctypes as C
import os

HERE = os.path.dirname(os.path.abspath(__file__))
_LIB = None


class CfsHipError(RuntimeError):
    code = 0


PRECOND_NONE, PRECOND_JACOBI = 0, 1  # include/cfs_hip.h: CFS_HIP_PRECOND_*
EIGS_LARGEST, EIGS_SMALLEST, EIGS_MAGNITUDE, EIGS_MAX_NCV = 0, 1, 2, 128  # CFS_HIP_EIGS_*
LOBPCG_MAX_K = 16  # CFS_HIP_LOBPCG_MAX_K
EXCHANGE_REDUCE_SCATTER, EXCHANGE_SPARSE = 0, 1  # CFS_HIP_EXCHANGE_*
ERR_ARG, ERR_DEVICE, ERR_UNSUPPORTED, ERR_NOMEM, ERR_INTERNAL, ERR_MIRROR, ERR_FILE = -1, -2, -3, -4, -5, -6, -7


class Options(C.Structure):
    _fields_ = [("max_slots", C.c_int), ("max_tile_nnz", C.c_int),
                ("block_threads", C.c_int), ("flags", C.c_int)]


class SymStats(C.Structure):
    _fields_ = [("n", C.c_int), ("row_begin", C.c_int), ("row_end", C.c_int),
                ("value_bytes", C.c_int), ("nnz_low", C.c_int64), ("nnz_diag", C.c_int64),
                ("nnz_full", C.c_int64), ("ntiles", C.c_int), ("nslices", C.c_int),
                ("max_slots_used", C.c_int), ("block_threads", C.c_int),
                ("halo_slots", C.c_int64), ("fold_rows", C.c_int64),
                ("remote_vals", C.c_int64), ("lds_bytes", C.c_int64),
                ("bytes_algorithmic", C.c_int64), ("bytes_streamed", C.c_int64),
                ("device_bytes", C.c_int64), ("mirror_entries", C.c_int64),
                ("far_entries", C.c_int64), ("ngroups", C.c_int), ("reserved_", C.c_int)]

    def asdict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


class PlanReport(C.Structure):
    _fields_ = [("ntiles", C.c_int), ("ngroups", C.c_int), ("lds_slots", C.c_int),
                ("nslices", C.c_int64), ("halo_slots", C.c_int64), ("stream_len", C.c_int64),
                ("nnz_low", C.c_int64), ("fold_rows", C.c_int64), ("remote_vals", C.c_int64),
                ("decoded", C.c_int64), ("mismatches", C.c_int64),
                ("mirror_entries", C.c_int64), ("far_entries", C.c_int64)]

    def asdict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


class PlanFileInfo(C.Structure):
    _fields_ = [("format_version", C.c_int), ("value_bytes", C.c_int), ("n", C.c_int), ("row_begin", C.c_int),
                ("row_end", C.c_int), ("nranks", C.c_int), ("rank", C.c_int), ("flags", C.c_int),
                ("ntiles", C.c_int), ("ngroups", C.c_int), ("block_threads", C.c_int), ("lds_slots", C.c_int),
                ("has_value_map", C.c_int), ("deterministic", C.c_int), ("device_built", C.c_int),
                ("nsections", C.c_int), ("nnz_low", C.c_int64), ("nslices", C.c_int64), ("halo_slots", C.c_int64),
                ("stream_len", C.c_int64), ("fold_rows", C.c_int64), ("remote_vals", C.c_int64),
                ("mirror_entries", C.c_int64), ("far_entries", C.c_int64), ("payload_bytes", C.c_int64),
                ("file_bytes", C.c_int64), ("tag", C.c_char * 256)]

    def asdict(self):
        d = {k: getattr(self, k) for k, _ in self._fields_}
        d["tag"] = d["tag"].decode(errors="replace")
        return d


AMG_MAX_LEVELS, AMG_MAX_COARSE = 16, 1024  # CFS_HIP_AMG_MAX_LEVELS, CFS_HIP_AMG_MAX_COARSE
AMG_MATCHING_GREEDY, AMG_MATCHING_DOMINANT, AMG_MATCH_ROUNDS = 0, 1, 64  # CFS_HIP_AMG_MATCHING_*, CFS_HIP_AMG_MATCH_ROUNDS


class AmgOptions(C.Structure):
    _fields_ = [("passes", C.c_int), ("degree", C.c_int), ("coarse_max", C.c_int), ("reserved_", C.c_int),
                ("ratio", C.c_double)]


class AmgInfo(C.Structure):
    _fields_ = [("levels", C.c_int), ("passes", C.c_int), ("degree", C.c_int), ("coarse_max", C.c_int),
                ("ratio", C.c_double), ("device_bytes", C.c_longlong), ("setup_seconds", C.c_double),
                ("handles_seconds", C.c_double), ("n", C.c_int * AMG_MAX_LEVELS), ("nnz", C.c_longlong * AMG_MAX_LEVELS),
                ("lmin", C.c_double * AMG_MAX_LEVELS), ("lmax", C.c_double * AMG_MAX_LEVELS),
                ("kind", C.c_int * AMG_MAX_LEVELS)]

    def asdict(self):
        d = {k: getattr(self, k) for k, _ in self._fields_[:8]}
        for k in ("n", "nnz", "lmin", "lmax", "kind"):
            d[k] = list(getattr(self, k))[:self.levels]
        return d


# every symbol include/cfs_hip.h declares (tests check the .so exports them all)
SYMBOLS = [
    "cfs_hip_abi_version", "cfs_hip_last_error", "cfs_hip_device_count", "cfs_hip_init",
    "cfs_hip_current_device", "cfs_hip_runtime_bound", "cfs_hip_pinned_owns", "cfs_hip_pinned_pool_stats", "cfs_hip_default_stream", "cfs_hip_synchronize", "cfs_hip_alloc", "cfs_hip_free",
    "cfs_hip_memcpy", "cfs_hip_memset", "cfs_hip_sym_create_f64", "cfs_hip_sym_create_f32",
    "cfs_hip_sym_create_shard_f64", "cfs_hip_sym_create_shard_f32",
    "cfs_hip_sym_create_multi_f64", "cfs_hip_sym_create_multi_f32", "cfs_hip_comm_create", "cfs_hip_comm_info", "cfs_hip_comm_destroy", "cfs_hip_comm_reduce_scatter",
    "cfs_hip_comm_allgather", "cfs_hip_comm_alltoallv", "cfs_hip_comm_wait_consumed", "cfs_hip_sym_num_gpus", "cfs_hip_sym_multi_set_xmode", "cfs_hip_sym_multi_set_exchange", "cfs_hip_sym_multi_exchange_info", "cfs_hip_sym_multi_devices", "cfs_hip_sym_balanced_splits", "cfs_hip_sym_destroy", "cfs_hip_sym_update_values_f64", "cfs_hip_sym_update_values_f32", "cfs_hip_sym_spmv",
    "cfs_hip_sym_spmv_async", "cfs_hip_sym_cg", "cfs_hip_sym_pcg", "cfs_hip_sym_diagonal_async", "cfs_hip_sym_block_diagonal_async",
    "cfs_hip_sym_pcg_block", "cfs_hip_sym_block_inverse_async", "cfs_hip_sym_pcg_mixed", "cfs_hip_sym_minres", "cfs_hip_sym_pcg_cheb", "cfs_hip_sym_cheb_apply", "cfs_hip_sym_precond_lmax", "cfs_hip_debug_cheb_coeffs",
    "cfs_hip_amg_create_f64", "cfs_hip_amg_create_f32", "cfs_hip_amg_destroy", "cfs_hip_amg_info", "cfs_hip_amg_level_aggregates", "cfs_hip_amg_level_matrix", "cfs_hip_amg_coarse_inverse", "cfs_hip_amg_apply", "cfs_hip_sym_pcg_amg", "cfs_hip_debug_amg_coarsen", "cfs_hip_amg_create_refreshable_f64", "cfs_hip_amg_create_refreshable_f32", "cfs_hip_amg_update_values_f64", "cfs_hip_amg_update_values_f32", "cfs_hip_amg_refresh_info", "cfs_hip_debug_amg_refresh_split", "cfs_hip_debug_amg_recoarsen",
    "cfs_hip_amg_create_dominant_f64", "cfs_hip_amg_create_dominant_f32", "cfs_hip_amg_create_device_f64", "cfs_hip_amg_create_device_f32",
    "cfs_hip_amg_setup_info", "cfs_hip_debug_amg_coarsen_dominant",
    "cfs_hip_amg_create_block_f64", "cfs_hip_amg_create_block_f32", "cfs_hip_amg_block", "cfs_hip_amg_level_node_weights", "cfs_hip_debug_amg_coarsen_block",
    "cfs_hip_sym_eigs", "cfs_hip_sym_debug_lanczos", "cfs_hip_debug_symeig", "cfs_hip_debug_eigs_combine", "cfs_hip_sym_lobpcg", "cfs_hip_debug_lobpcg_rr", "cfs_hip_debug_gram", "cfs_hip_sym_debug_lobpcg", "cfs_hip_debug_lobpcg_update", "cfs_hip_debug_gram_cols", "cfs_hip_debug_lobpcg_update_cols", "cfs_hip_sym_debug_lobpcg_residual",
    "cfs_hip_amg_apply_cols", "cfs_hip_amg_column_cycles", "cfs_hip_sym_lobpcg_amg", "cfs_hip_sym_debug_lobpcg_amg", "cfs_hip_sym_pcg_cols", "cfs_hip_sym_pcg_amg_cols",
    "cfs_hip_sym_lobpcg_gen", "cfs_hip_sym_lobpcg_gen_amg", "cfs_hip_sym_debug_lobpcg_gen", "cfs_hip_debug_gram3_cols", "cfs_hip_debug_lobpcg_update3_cols", "cfs_hip_sym_debug_lobpcg_residual_gen",
    "cfs_hip_sym_shard_send_counts", "cfs_hip_sym_shard_send_rows",
    "cfs_hip_sym_shard_set_recv", "cfs_hip_sym_spmv_local_async",
    "cfs_hip_sym_recv_fold_async", "cfs_hip_sym_spmv_phases_async", "cfs_hip_sym_get_stats", "cfs_hip_sym_debug_digest", "cfs_hip_sym_debug_kernel", "cfs_hip_sym_debug_fold_lists", "cfs_hip_sym_debug_plan_note", "cfs_hip_sym_debug_timeline", "cfs_hip_sym_debug_group_features", "cfs_hip_sym_plan_check_f64",
    "cfs_hip_sym_plan_check_f32", "cfs_hip_sym_plan_send_info_f64",
    "cfs_hip_sym_save", "cfs_hip_sym_load", "cfs_hip_plan_file_check", "cfs_hip_debug_checksum", "cfs_hip_sym_plan_save_f64", "cfs_hip_sym_plan_save_f32", "cfs_hip_csr_create_f64", "cfs_hip_csr_create_f32",
    "cfs_hip_csr_spmv", "cfs_hip_csr_spmv_async", "cfs_hip_csr_destroy", "cfs_hip_csr_kernel_form", "cfs_hip_csr_stats",
    "cfs_hip_csr_debug_layout",
    "cfs_hip_event_create", "cfs_hip_event_record", "cfs_hip_event_elapsed_ms",
    "cfs_hip_event_destroy",
]


def lib_path():
    # CFS_HIP_LIB: developer override to A/B an experimental build of the library
    return os.environ.get("CFS_HIP_LIB") or os.path.join(HERE, "libcfs_hip.so")


def load():
    """Load libcfs_hip.so.  There is NO fallback: if the HIP extension is
    missing the product path fails here, loudly."""
    global _LIB
    if _LIB is not None:
        return _LIB
    path = lib_path()
    if not os.path.exists(path):
        raise CfsHipError(
            f"{path} is missing: the HIP extension is not built "
            "(run `python -c 'import __graft_entry__ as g; g.build()'`). "
            "There is no CPU fallback for the product path.")
    lib = C.CDLL(path)
    vp, ip, i64 = C.c_void_p, C.POINTER(C.c_int), C.c_int64
    lib.cfs_hip_last_error.restype = C.c_char_p
    lib.cfs_hip_alloc.argtypes = [C.c_size_t, C.c_int, C.POINTER(vp)]
    lib.cfs_hip_free.argtypes = [vp, C.c_int]
    lib.cfs_hip_current_device.argtypes = [ip]
    lib.cfs_hip_pinned_owns.argtypes = [vp]
    lib.cfs_hip_pinned_pool_stats.argtypes = [C.POINTER(C.c_size_t)] * 3
    lib.cfs_hip_memcpy.argtypes = [vp, vp, C.c_size_t, C.c_int]
    lib.cfs_hip_memset.argtypes = [vp, C.c_int, C.c_size_t]
    lib.cfs_hip_default_stream.argtypes = [C.POINTER(vp)]
    lib.cfs_hip_synchronize.argtypes = [vp]
    for suf in ("f64", "f32"):
        getattr(lib, "cfs_hip_sym_create_" + suf).argtypes = [
            C.c_int, vp, vp, vp, C.POINTER(Options), C.POINTER(vp)]
        getattr(lib, "cfs_hip_sym_create_shard_" + suf).argtypes = [
            C.c_int, vp, vp, vp, C.c_int, C.c_int, vp, C.POINTER(Options), C.POINTER(vp)]
        getattr(lib, "cfs_hip_sym_create_multi_" + suf).argtypes = [
            C.c_int, vp, vp, vp, C.c_int, vp, C.POINTER(Options), C.POINTER(vp)]
        getattr(lib, "cfs_hip_sym_plan_check_" + suf).argtypes = [
            C.c_int, vp, vp, vp, C.c_int, C.c_int, vp, C.POINTER(Options),
            C.POINTER(PlanReport)]
        getattr(lib, "cfs_hip_csr_create_" + suf).argtypes = [
            C.c_int, C.c_int, vp, vp, vp, C.POINTER(vp)]
    lib.cfs_hip_sym_plan_send_info_f64.argtypes = [
        C.c_int, vp, vp, vp, C.c_int, C.c_int, vp, C.POINTER(Options), vp, vp, C.c_int, ip]
    lib.cfs_hip_sym_balanced_splits.argtypes = [C.c_int, vp, vp, C.c_int, vp]
    lib.cfs_hip_sym_num_gpus.argtypes = [vp, ip]
    if hasattr(lib, "cfs_hip_comm_create"):
        lib.cfs_hip_comm_create.argtypes = [C.c_int, vp, C.c_int, C.POINTER(vp)]
        lib.cfs_hip_comm_info.argtypes = [vp, ip, ip]
        lib.cfs_hip_comm_destroy.argtypes = [vp]
        lib.cfs_hip_comm_reduce_scatter.argtypes = [vp, vp, vp, C.c_size_t, C.c_int, vp]
        lib.cfs_hip_comm_allgather.argtypes = [vp, vp, vp, C.c_size_t, C.c_int, vp]
        lib.cfs_hip_comm_wait_consumed.argtypes = [vp, C.c_int, vp]
    if hasattr(lib, "cfs_hip_sym_multi_set_xmode"):
        lib.cfs_hip_sym_multi_set_xmode.argtypes = [vp, C.c_int]
        lib.cfs_hip_sym_multi_devices.argtypes = [vp, vp, C.c_int, ip]
    if hasattr(lib, "cfs_hip_comm_alltoallv"):  # (absent from older builds loaded through CFS_HIP_LIB)
        lib.cfs_hip_comm_alltoallv.argtypes = [vp, vp, vp, vp, C.c_int, vp]
        lib.cfs_hip_sym_multi_set_exchange.argtypes = [vp, C.c_int]
        lib.cfs_hip_sym_multi_exchange_info.argtypes = [vp, ip, C.POINTER(i64), C.POINTER(i64)]
    if hasattr(lib, "cfs_hip_sym_save"):  # (absent from older builds loaded through CFS_HIP_LIB)
        lib.cfs_hip_sym_save.argtypes = [vp, C.c_char_p, C.c_char_p]
        lib.cfs_hip_sym_load.argtypes = [C.c_char_p, C.c_char_p, C.POINTER(vp)]
        lib.cfs_hip_plan_file_check.argtypes = [C.c_char_p, C.POINTER(PlanFileInfo)]
        lib.cfs_hip_debug_checksum.argtypes = [vp, C.c_size_t, C.c_int, C.POINTER(C.c_ulonglong)]
        for suf in ("f64", "f32"):
            getattr(lib, "cfs_hip_sym_plan_save_" + suf).argtypes = [
                C.c_int, vp, vp, vp, C.c_int, C.c_int, vp, C.POINTER(Options), C.c_char_p, C.c_char_p]
    lib.cfs_hip_sym_destroy.argtypes = [vp]
    lib.cfs_hip_sym_update_values_f64.argtypes = [vp, vp, C.c_longlong]
    lib.cfs_hip_sym_update_values_f32.argtypes = [vp, vp, C.c_longlong]
    lib.cfs_hip_sym_spmv.argtypes = [vp, vp, vp]
    lib.cfs_hip_sym_spmv_async.argtypes = [vp, vp, vp, vp]
    lib.cfs_hip_sym_shard_send_counts.argtypes = [vp, vp]
    lib.cfs_hip_sym_shard_send_rows.argtypes = [vp, vp]
    lib.cfs_hip_sym_shard_set_recv.argtypes = [vp, C.c_int, vp]
    lib.cfs_hip_sym_spmv_local_async.argtypes = [vp, vp, vp, vp, vp]
    lib.cfs_hip_sym_recv_fold_async.argtypes = [vp, vp, vp, vp]
    lib.cfs_hip_sym_spmv_phases_async.argtypes = [vp, vp, vp, vp, C.c_int, vp]
    lib.cfs_hip_sym_get_stats.argtypes = [vp, C.POINTER(SymStats)]
    lib.cfs_hip_sym_debug_timeline.argtypes = [vp, vp, vp, vp, C.c_int, ip]
    if hasattr(lib, "cfs_hip_sym_debug_digest"):  # (absent from older builds loaded through CFS_HIP_LIB)
        lib.cfs_hip_sym_debug_digest.argtypes = [vp, vp, C.c_int]
        lib.cfs_hip_sym_debug_plan_note.argtypes = [vp, C.c_char_p, C.c_int]
    if hasattr(lib, "cfs_hip_sym_debug_kernel"):
        lib.cfs_hip_sym_debug_kernel.argtypes = [vp, ip, C.c_int]
    if hasattr(lib, "cfs_hip_sym_debug_fold_lists"):
        lib.cfs_hip_sym_debug_fold_lists.argtypes = [vp, C.c_int, vp, vp, C.c_int, ip]
    lib.cfs_hip_sym_debug_group_features.argtypes = [vp, vp, C.c_int, ip]
    lib.cfs_hip_csr_spmv.argtypes = [vp, vp, vp]
    lib.cfs_hip_csr_spmv_async.argtypes = [vp, vp, vp, vp]
    lib.cfs_hip_csr_destroy.argtypes = [vp]
    if hasattr(lib, "cfs_hip_csr_kernel_form"):
        lib.cfs_hip_csr_kernel_form.argtypes = [vp, ip, ip]
    if hasattr(lib, "cfs_hip_sym_cg"):
        lib.cfs_hip_sym_cg.argtypes = [vp, vp, vp, C.c_double, C.c_int, C.c_int, ip, C.POINTER(C.c_double), vp]
    if hasattr(lib, "cfs_hip_sym_pcg"):  # (absent from older builds loaded through CFS_HIP_LIB)
        lib.cfs_hip_sym_diagonal_async.argtypes = [vp, vp, vp]
        lib.cfs_hip_sym_pcg.argtypes = [vp, vp, vp, C.c_int, C.c_double, C.c_int, C.c_int, ip, C.POINTER(C.c_double), vp]
    if hasattr(lib, "cfs_hip_sym_pcg_block"):  # (absent from older builds loaded through CFS_HIP_LIB)
        lib.cfs_hip_sym_block_diagonal_async.argtypes = [vp, C.c_int, vp, vp]
        lib.cfs_hip_sym_block_inverse_async.argtypes = [vp, C.c_int, vp, vp]
        lib.cfs_hip_sym_pcg_block.argtypes = [vp, vp, vp, C.c_int, C.c_double, C.c_int, C.c_int, ip, C.POINTER(C.c_double), vp]
    if hasattr(lib, "cfs_hip_sym_pcg_mixed"):  # (absent from older builds loaded through CFS_HIP_LIB)
        lib.cfs_hip_sym_pcg_mixed.argtypes = [vp, vp, vp, vp, C.c_int, C.c_double, C.c_double, C.c_int, C.c_int, ip, ip,
                                              C.POINTER(C.c_double), vp]
    if hasattr(lib, "cfs_hip_sym_minres"):  # (absent from older builds loaded through CFS_HIP_LIB)
        lib.cfs_hip_sym_minres.argtypes = [vp, vp, vp, C.c_int, C.c_double, C.c_double, C.c_int, C.c_int, ip,
                                           C.POINTER(C.c_double), vp]
    if hasattr(lib, "cfs_hip_sym_pcg_cheb"):  # (absent from older builds loaded through CFS_HIP_LIB)
        dp = C.POINTER(C.c_double)
        lib.cfs_hip_sym_pcg_cheb.argtypes = [vp, vp, vp, C.c_int, C.c_int, C.c_double, C.c_double, C.c_double, C.c_int, C.c_int,
                                             ip, dp, dp, vp]
        lib.cfs_hip_sym_cheb_apply.argtypes = [vp, C.c_int, C.c_int, C.c_double, C.c_double, vp, vp, vp]
        lib.cfs_hip_sym_precond_lmax.argtypes = [vp, C.c_int, C.c_int, vp, dp, vp]
        lib.cfs_hip_debug_cheb_coeffs.argtypes = [C.c_int, C.c_double, C.c_double, dp, dp, dp]
    if hasattr(lib, "cfs_hip_amg_create_f64"):  # (absent from older builds loaded through CFS_HIP_LIB)
        dp = C.POINTER(C.c_double)
        for suf in ("f64", "f32"):
            getattr(lib, "cfs_hip_amg_create_" + suf).argtypes = [vp, C.c_int, vp, vp, vp, C.POINTER(AmgOptions), C.POINTER(vp)]
        lib.cfs_hip_amg_destroy.argtypes = [vp]
        lib.cfs_hip_amg_info.argtypes = [vp, C.POINTER(AmgInfo)]
        lib.cfs_hip_amg_level_aggregates.argtypes = [vp, C.c_int, vp, vp]
        lib.cfs_hip_amg_level_matrix.argtypes = [vp, C.c_int, vp, vp, vp]
        lib.cfs_hip_amg_coarse_inverse.argtypes = [vp, vp]
        lib.cfs_hip_amg_apply.argtypes = [vp, vp, vp, vp]
        lib.cfs_hip_sym_pcg_amg.argtypes = [vp, vp, vp, vp, C.c_double, C.c_int, C.c_int, ip, dp, vp]
        lib.cfs_hip_debug_amg_coarsen.argtypes = [C.c_int, vp, vp, vp, C.c_int, vp, vp, ip, vp, vp, vp, C.c_longlong,
                                                  C.POINTER(C.c_longlong)]
    if hasattr(lib, "cfs_hip_amg_create_device_f64"):  # (absent from older builds loaded through CFS_HIP_LIB)
        dp = C.POINTER(C.c_double)
        for suf in ("f64", "f32"):
            for kind in ("dominant_", "device_"):
                getattr(lib, "cfs_hip_amg_create_" + kind + suf).argtypes = [vp, C.c_int, vp, vp, vp, C.POINTER(AmgOptions), C.POINTER(vp)]
        lib.cfs_hip_amg_setup_info.argtypes = [vp, ip, ip, ip, dp, C.POINTER(C.c_longlong)]
        lib.cfs_hip_debug_amg_coarsen_dominant.argtypes = [C.c_int, vp, vp, vp, C.c_int, vp, vp, ip, vp, vp, vp, C.c_longlong,
                                                           C.POINTER(C.c_longlong), ip]
    if hasattr(lib, "cfs_hip_amg_update_values_f64"):  # (absent from older builds loaded through CFS_HIP_LIB)
        for suf in ("f64", "f32"):
            getattr(lib, "cfs_hip_amg_create_refreshable_" + suf).argtypes = [vp, C.c_int, vp, vp, vp, C.POINTER(AmgOptions),
                                                                              C.POINTER(vp)]
            getattr(lib, "cfs_hip_amg_update_values_" + suf).argtypes = [vp, vp, C.c_longlong]
        lib.cfs_hip_amg_refresh_info.argtypes = [vp, C.POINTER(C.c_longlong), ip, C.POINTER(C.c_double)]
        lib.cfs_hip_debug_amg_refresh_split.argtypes = [vp, C.POINTER(C.c_double)]
        lib.cfs_hip_debug_amg_recoarsen.argtypes = [C.c_int, vp, vp, vp, vp, C.c_int, vp, vp, C.c_longlong, C.POINTER(C.c_longlong)]
    if hasattr(lib, "cfs_hip_amg_create_block_f64"):  # (absent from older builds loaded through CFS_HIP_LIB)
        for suf in ("f64", "f32"):
            getattr(lib, "cfs_hip_amg_create_block_" + suf).argtypes = [vp, C.c_int, vp, vp, vp, C.c_int, C.c_int, C.POINTER(AmgOptions),
                                                                        C.POINTER(vp)]
        lib.cfs_hip_amg_block.argtypes = [vp, ip]
        lib.cfs_hip_amg_level_node_weights.argtypes = [vp, C.c_int, vp]
        lib.cfs_hip_debug_amg_coarsen_block.argtypes = [C.c_int, vp, vp, vp, C.c_int, C.c_int, C.c_int, vp, vp, ip, vp, vp, vp,
                                                        C.c_longlong, C.POINTER(C.c_longlong), ip]
    if hasattr(lib, "cfs_hip_sym_eigs"):  # (absent from older builds loaded through CFS_HIP_LIB)
        dp = C.POINTER(C.c_double)
        lib.cfs_hip_sym_eigs.argtypes = [vp, C.c_int, C.c_int, C.c_int, C.c_double, C.c_int, vp, dp, vp, C.c_longlong, dp,
                                         ip, ip, ip, vp]
        lib.cfs_hip_sym_debug_lanczos.argtypes = [vp, vp, C.c_int, vp, C.c_longlong, dp, dp, ip, vp]
        lib.cfs_hip_debug_symeig.argtypes = [C.c_int, dp, dp, dp]
    if hasattr(lib, "cfs_hip_debug_eigs_combine"):  # (absent from older builds loaded through CFS_HIP_LIB)
        lib.cfs_hip_debug_eigs_combine.argtypes = [vp, C.c_longlong, vp, C.c_longlong, C.c_longlong, C.c_int, C.c_int,
                                                   C.POINTER(C.c_double), C.c_int, vp]
    if hasattr(lib, "cfs_hip_sym_lobpcg"):  # (absent from older builds loaded through CFS_HIP_LIB)
        dp = C.POINTER(C.c_double)
        lib.cfs_hip_sym_lobpcg.argtypes = [vp, C.c_int, C.c_int, C.c_double, C.c_double, C.c_int, vp, C.c_longlong, dp, vp,
                                           C.c_longlong, dp, ip, ip, ip, vp]
        lib.cfs_hip_debug_lobpcg_rr.argtypes = [C.c_int, dp, dp, C.c_int, C.c_double, dp, dp, ip]
        lib.cfs_hip_debug_gram.argtypes = [vp, vp, C.c_longlong, C.c_longlong, C.c_int, C.c_int, dp, dp, vp]
        lib.cfs_hip_sym_debug_lobpcg.argtypes = [vp, C.c_int, C.c_int, vp, C.c_longlong, C.c_int, dp, vp, C.c_longlong, dp, vp]
        lib.cfs_hip_debug_lobpcg_update.argtypes = [vp, C.c_longlong, C.c_longlong, C.c_int, C.c_int, dp, C.c_int, vp]
    if hasattr(lib, "cfs_hip_debug_gram_cols"):  # (absent from older builds loaded through CFS_HIP_LIB)
        dp = C.POINTER(C.c_double)
        lib.cfs_hip_debug_gram_cols.argtypes = [vp, vp, C.c_longlong, C.c_longlong, C.c_int, ip, C.c_int, C.c_int, dp, dp, vp]
        lib.cfs_hip_debug_lobpcg_update_cols.argtypes = [vp, vp, C.c_longlong, C.c_longlong, C.c_int, C.c_int, ip, C.c_int, dp,
                                                         C.c_int, vp]
        lib.cfs_hip_sym_debug_lobpcg_residual.argtypes = [vp, C.c_int, vp, vp, vp, C.c_longlong, C.c_int, dp, C.c_uint, dp, vp]
    if hasattr(lib, "cfs_hip_amg_apply_cols"):  # (absent from older builds loaded through CFS_HIP_LIB)
        dp = C.POINTER(C.c_double)
        lib.cfs_hip_amg_apply_cols.argtypes = [vp, vp, vp, C.c_longlong, C.c_int, C.c_uint, vp]
        lib.cfs_hip_amg_column_cycles.argtypes = [vp, C.POINTER(C.c_longlong)]
        lib.cfs_hip_sym_lobpcg_amg.argtypes = [vp, vp, C.c_int, C.c_double, C.c_double, C.c_int, vp, C.c_longlong, dp, vp,
                                               C.c_longlong, dp, ip, ip, ip, vp]
        lib.cfs_hip_sym_debug_lobpcg_amg.argtypes = [vp, vp, C.c_int, vp, C.c_longlong, C.c_int, dp, vp, C.c_longlong, dp, vp]
    if hasattr(lib, "cfs_hip_sym_lobpcg_gen"):  # (absent from older builds loaded through CFS_HIP_LIB)
        dp = C.POINTER(C.c_double)
        lib.cfs_hip_sym_lobpcg_gen.argtypes = [vp, vp, C.c_int, C.c_int, C.c_double, C.c_double, C.c_int, vp, C.c_longlong, dp, vp,
                                               C.c_longlong, dp, ip, ip, ip, ip, vp]
        lib.cfs_hip_sym_lobpcg_gen_amg.argtypes = [vp, vp, vp, C.c_int, C.c_double, C.c_double, C.c_int, vp, C.c_longlong, dp, vp,
                                                   C.c_longlong, dp, ip, ip, ip, ip, vp]
        lib.cfs_hip_sym_debug_lobpcg_gen.argtypes = [vp, vp, C.c_int, C.c_int, vp, C.c_longlong, C.c_int, dp, vp, C.c_longlong, dp, vp]
        lib.cfs_hip_debug_gram3_cols.argtypes = [vp, vp, vp, C.c_longlong, C.c_longlong, C.c_int, ip, C.c_int, dp, dp, vp]
        lib.cfs_hip_debug_lobpcg_update3_cols.argtypes = [vp, vp, vp, C.c_longlong, C.c_longlong, C.c_int, C.c_int, ip, C.c_int, dp,
                                                          C.c_int, vp]
        lib.cfs_hip_sym_debug_lobpcg_residual_gen.argtypes = [vp, C.c_int, vp, vp, vp, vp, C.c_longlong, C.c_int, dp, C.c_uint, dp, vp]
    if hasattr(lib, "cfs_hip_sym_pcg_cols"):  # (absent from older builds loaded through CFS_HIP_LIB)
        dp = C.POINTER(C.c_double)
        lib.cfs_hip_sym_pcg_cols.argtypes = [vp, vp, vp, C.c_longlong, C.c_int, C.c_int, C.c_double, C.c_int, C.c_int, ip, dp, vp]
        lib.cfs_hip_sym_pcg_amg_cols.argtypes = [vp, vp, vp, vp, C.c_longlong, C.c_int, C.c_double, C.c_int, C.c_int, ip, dp, vp]
    if hasattr(lib, "cfs_hip_csr_stats"):
        lib.cfs_hip_csr_stats.argtypes = [vp, C.POINTER(C.c_int64), C.POINTER(C.c_int64)]
    if hasattr(lib, "cfs_hip_csr_debug_layout"):
        lib.cfs_hip_csr_debug_layout.argtypes = [vp, C.POINTER(C.c_longlong), C.c_int]
    lib.cfs_hip_event_create.argtypes = [C.POINTER(vp)]
    lib.cfs_hip_event_record.argtypes = [vp, vp]
    lib.cfs_hip_event_elapsed_ms.argtypes = [vp, vp, C.POINTER(C.c_float)]
    lib.cfs_hip_event_destroy.argtypes = [vp]
    _LIB = lib
    return lib


def check(rc):
    if rc != 0:
        msg = load().cfs_hip_last_error().decode(errors="replace")
        e = CfsHipError(f"cfs_hip error {rc}: {msg}")
        e.code = rc
        raise e
