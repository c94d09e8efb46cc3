/*
 * cfs_hip.h -- C ABI of libcfs_hip.so: the MI355X (gfx950) symmetric-SpMV hot
 * path of cfs-spmv behind plain pointers and sizes.
 *
 * This is the drop-in boundary.  The reference (athelaf/cfs-spmv) has no FFI of
 * its own -- it is a C++ library whose hot path hides behind two seams:
 *     tune()                   include/matrix/csr_matrix.tpp:230-310
 *     dense_vector_multiply()  include/matrix/csr_matrix.hpp:67-70  (spmv_fn)
 * and the allocation seam internal_alloc/internal_free
 *     include/utils/allocator.hpp:11-12, src/allocator.cpp:8-43.
 * Each entry point below names the reference interface it replaces.  The C++
 * surface (include/cfs.hpp: SparseMatrix / CSRMatrix / SpDMV) and the Python
 * mirror (cfs_spmv_amd/) are thin callers of this ABI; INTEGRATION.md shows
 * the binding a maintainer of the reference would add.
 *
 * Conventions: every function returns 0 on success or a negative error code;
 * cfs_hip_last_error() returns the message of the calling thread's last
 * failure.  No C++ objects or exceptions cross this line.  Indices are int32
 * (only <int,float> and <int,double> are instantiated in the reference:
 * src/csr.cpp:10-11, src/cfs.cpp:11-21).
 */
#ifndef CFS_HIP_H
#define CFS_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define CFS_HIP_ABI_VERSION 4

/* error codes */
#define CFS_HIP_OK 0
#define CFS_HIP_ERR_ARG (-1)      /* bad argument                            */
#define CFS_HIP_ERR_DEVICE (-2)   /* HIP runtime failure (message has detail) */
/* the tile schedule does not cover this matrix (a row denser than an LDS window,
 * offsets exhausted): the caller may fall back to the general CSR kernel.      */
#define CFS_HIP_ERR_UNSUPPORTED (-3)
#define CFS_HIP_ERR_NOMEM (-4)
#define CFS_HIP_ERR_INTERNAL (-5) /* a consistency check of the schedule builder failed */
/* a shard cannot be built in the mirrored form (off-block structure unsymmetric
 * or duplicated): rebuild it with CFS_HIP_FLAG_SHARD_EXCHANGE                   */
#define CFS_HIP_ERR_MIRROR (-6)
/* a plan file (cfs_hip_sym_save / _load): cannot open / truncated / not a plan file / version
 * or layout mismatch / checksum / tag mismatch; the message says which                        */
#define CFS_HIP_ERR_FILE (-7)

typedef struct cfs_hip_sym_s *cfs_hip_sym_t; /* symmetric (SSS) matrix handle */
typedef struct cfs_hip_csr_s *cfs_hip_csr_t; /* general CSR matrix handle     */

/* ---- runtime (replaces src/runtime.cpp:10-34: CFS_NUM_THREADS / affinity) -- */
int cfs_hip_abi_version(void);
const char *cfs_hip_last_error(void);
int cfs_hip_device_count(int *count);
/* Make `device` the calling thread's current device and the HOME of the
 * synchronous entry points (cfs_hip_alloc, host-pointer SpMV).  Idempotent, and it
 * leaves the contexts of other devices alone: handles remember the device they
 * were created on and keep working.  A process that never calls it adopts the
 * device that is current in the calling thread at the first use (never a
 * hard-wired device 0).                                                        */
int cfs_hip_init(int device);
int cfs_hip_current_device(int *device); /* the home device */
/* 1 once a home device is bound; never initialises the runtime itself (the allocator seam asks
 * before it hands out page-locked host memory: a plain host allocation must not start HIP) */
int cfs_hip_runtime_bound(void);
/* stream used internally by the synchronous (host-pointer capable) entry
 * points; created by cfs_hip_init.  The *_async entry points take the caller's
 * hipStream_t verbatim: NULL there means HIP's null stream (which is what
 * torch.cuda.current_stream() is by default), never this one.               */
int cfs_hip_default_stream(void **stream);
int cfs_hip_synchronize(void *stream); /* NULL = the library stream */

/* ---- allocator (replaces internal_alloc / internal_free,
 *      src/allocator.cpp:8-43; Platform::gpu memory)                      ---- */
#define CFS_HIP_MEM_DEVICE 0 /* hipMalloc: HBM, the residency the timed loop needs */
#define CFS_HIP_MEM_PINNED 1 /* hipHostMalloc: page-locked host staging buffer      */
int cfs_hip_alloc(size_t bytes, int kind, void **out);
int cfs_hip_free(void *p, int kind);
/* The page-locked blocks come from a pool (power-of-two classes >= 64 KiB; a
 * released block is kept for the next request).  owns: 1 if p is a live block of
 * the pool (the allocator seam frees those through cfs_hip_free).              */
int cfs_hip_pinned_owns(const void *p);
int cfs_hip_pinned_pool_stats(size_t *live_blocks, size_t *spare_blocks, size_t *spare_bytes);
#define CFS_HIP_H2D 0
#define CFS_HIP_D2H 1
#define CFS_HIP_D2D 2
int cfs_hip_memcpy(void *dst, const void *src, size_t bytes, int dir);
int cfs_hip_memset(void *dst, int value, size_t bytes);

/* ---- tuning knobs of the tile schedule (all 0 = library default) ---------- */
typedef struct {
  int max_slots;     /* LDS slots (x and y windows) per tile               */
  int max_tile_nnz;  /* cap on stored nonzeros per tile                    */
  int block_threads; /* workgroup size of the tile kernel: 256, 512, 1024  */
  int flags;         /* CFS_HIP_FLAG_*                                      */
} cfs_hip_options;
/* timing-only ablations of the tile kernel (WRONG results by construction;
 * used by tools/ to price LDS atomics and LDS gathers against the pure matrix
 * stream; never set by the product callers): 1 = no transposed LDS atomics,
 * 2 = no LDS traffic at all, 3 = LDS windows only (no matrix stream),
 * 4 = matrix stream only (no x gather / y flush)                             */
#define CFS_HIP_FLAG_ABLATE_MASK 7
/* keep rows in their given order (tiles = runs of consecutive rows) instead of
 * clustering the matrix graph first (the default, fewer halo columns)        */
#define CFS_HIP_FLAG_NO_REORDER 8
/* always keep the clustered order (skip the halo-count comparison)            */
#define CFS_HIP_FLAG_FORCE_CLUSTER 16
/* tune() of a matrix with >= 2M stored nonzeros measures alternatives and keeps the
 * fastest: when no block / slot count is given and the rows are scheduled in
 * clustered order, the default window shape (512 threads x 2 workgroups per CU)
 * against 1024 threads x 1 with a window twice the size; when a noticeable share of
 * the halo columns is used only once, the HYB form against the plain one.  This
 * flag skips the measurements (one schedule build; Tuning::None).              */
#define CFS_HIP_FLAG_NO_CALIBRATE 32
/* Shards only.  Default: off-block entries are MIRRORED -- stored by both ranks
 * they touch and processed one-sided, so that no contribution to y ever leaves
 * the rank and a sharded SpMV needs no exchange (x is replicated anyway; the
 * duplicated boundary entries are a few per cent of a shard).  With this flag a
 * shard keeps its off-block entries two-sided and packs its contributions to
 * rows of lower ranks for an all-to-all / reduce-scatter (the exchange form). */
#define CFS_HIP_FLAG_SHARD_EXCHANGE 64
/* Format::hyb (the reference's split_by_bandwidth, csr_matrix.tpp:312-401, as a
 * working feature): an entry whose column lies outside its tile and is used by that
 * tile only once leaves the symmetric tile format.  It is stored by BOTH tiles it
 * touches as (value, own row slot, global column) and processed one-sided with x
 * gathered from global memory -- no LDS slot, no strip entry, no fold entry.  With
 * the flag the split is always made; without it tune() may still choose it by
 * measurement (see CFS_HIP_FLAG_NO_CALIBRATE); CFS_HIP_FLAG_NO_HYB forbids it.     */
#define CFS_HIP_FLAG_HYB 128
#define CFS_HIP_FLAG_NO_HYB 256
/* Bit-reproducible results.  By default the transposed updates y_j += a_ij x_i of a
 * tile meet in LDS through floating-point atomics, whose order varies from run to
 * run: results agree to ~1e-13 of the row scale, not bitwise (the reference adds in a
 * fixed order, csr_matrix.tpp:3005-3013).  With this flag every contribution is
 * converted to a fixed-point number (2 x 40 bits below a PER-SLOT scale: the 1-norm of
 * the slot's matrix row times the largest |x| of the tile's window, a bound of every
 * partial sum) and accumulated with INTEGER LDS atomics -- associative, hence the same
 * bits whatever the order; the halo fold already adds in a fixed order.  The precision
 * does not depend on how the matrix is scaled.  Costs LDS (26 instead of 16 bytes per
 * slot: smaller tiles) and ALU; 512- or 1 024-thread workgroups.  Far entries (HYB) are
 * covered: the x values they gather from outside the window enter the tile's scale.  A
 * contribution keeps 2^-80 of (row 1-norm) x (largest |x| the TILE reads).
 * NaN / Inf (they have no fixed-point image) are handled per TILE: every row that the contract at
 * cfs_hip_sym_spmv calls non-finite reads NaN (never +-Inf, never a finite number), and so does every
 * other slot of a tile whose window -- or whose far entries -- hold a non-finite x, and of a tile that
 * holds a non-finite matrix value.  One bad x_j therefore costs at most (1 + rows that hold j) x
 * max_slots_used rows, one bad a_ij = a_ji at most 2 x max_slots_used; every other row is the same
 * number as without it, and the NaN pattern is as reproducible as the rest.
 * Same tolerance against the oracle as the default.                                   */
#define CFS_HIP_FLAG_DETERMINISTIC 1024
/* keep, for every stored value of the device format, its position in the caller's CSR
 * value array (4 bytes per stored nonzero of device memory): cfs_hip_sym_update_values_*
 * can then refresh the numbers of the matrix without repeating tune()             */
#define CFS_HIP_FLAG_KEEP_VALUE_MAP 2048
/* tune() builds the tile schedule ON THE GPU from one upload of the caller's CSR (split,
 * tile cut, slot tables, virtual rows, leaders, packing: HIP kernels) whenever
 * the input is covered by the device builder -- everything but rows that are unsorted, hold
 * duplicates or exceed 4096 stored entries (noticed on the GPU, cfs_hip_sym_debug_plan_note
 * says which).  With this flag the host builder
 * (cfs_plan.hpp, OpenMP) is used instead; the two produce the same schedule bit for bit
 * (cfs_hip_sym_debug_digest).                                                          */
#define CFS_HIP_FLAG_HOST_PLAN 4096

/* ---- tune() for a symmetric matrix
 *      (replaces CSRMatrix::tune -> compress_symmetry ->
 *       conflict_free_aposteriori, csr_matrix.tpp:230-310, :1204-1639).
 * Input is the FULL CSR exactly as CSRMatrix holds it before tune()
 * (csr_matrix.tpp:74-107: 0-based, rows ascending, columns ascending), in host
 * memory; the handle copies what it needs (the caller may free the arrays
 * afterwards, as compress_symmetry does at :1700-1706).  Only entries with
 * col <= row are read; a missing diagonal entry counts as 0.
 *
 * The *_shard_* forms build rank `rank`'s 1-D row block of a matrix sharded
 * over `nranks` GPUs at row boundaries row_splits[0..nranks].  By
 * default the shard is MIRRORED (see CFS_HIP_FLAG_SHARD_EXCHANGE): it also reads
 * the entries of its rows right of the block and the lower entries (c, i) they
 * mirror, its SpMV needs no exchange, and a matrix whose off-block structure is
 * not symmetric (or has duplicate entries there) is refused with an error whose
 * message starts with "mirror:" -- build it with CFS_HIP_FLAG_SHARD_EXCHANGE.   */
int cfs_hip_sym_create_f64(int n, const int *rowptr, const int *colind,
                           const double *values, const cfs_hip_options *opt,
                           cfs_hip_sym_t *out);
int cfs_hip_sym_create_f32(int n, const int *rowptr, const int *colind,
                           const float *values, const cfs_hip_options *opt,
                           cfs_hip_sym_t *out);
int cfs_hip_sym_create_shard_f64(int n, const int *rowptr, const int *colind,
                                 const double *values, int nranks, int rank,
                                 const int *row_splits,
                                 const cfs_hip_options *opt, cfs_hip_sym_t *out);
int cfs_hip_sym_create_shard_f32(int n, const int *rowptr, const int *colind,
                                 const float *values, int nranks, int rank,
                                 const int *row_splits,
                                 const cfs_hip_options *opt, cfs_hip_sym_t *out);
/* One host thread, `ngpus` GPUs (the C++ surface with CFS_NUM_GPUS; the reference's
 * knob of this kind is CFS_NUM_THREADS, src/runtime.cpp:10-21): ngpus mirrored row
 * blocks, shard g on devices[g] (NULL: the visible devices round-robin from the
 * current one; several shards may share a device), each on a stream of its own.
 * The handle behaves like a whole-matrix one: cfs_hip_sym_spmv[_async] take x / y
 * of n entries on the device that was current at create (or host pointers);
 * shards on other devices get a replica of x per SpMV and copy their y block back
 * (cfs_hip_sym_multi_set_xmode; or reach both through peer access).            */
int cfs_hip_sym_create_multi_f64(int n, const int *rowptr, const int *colind,
                                 const double *values, int ngpus, const int *devices,
                                 const cfs_hip_options *opt, cfs_hip_sym_t *out);
int cfs_hip_sym_create_multi_f32(int n, const int *rowptr, const int *colind,
                                 const float *values, int ngpus, const int *devices,
                                 const cfs_hip_options *opt, cfs_hip_sym_t *out);
int cfs_hip_sym_num_gpus(cfs_hip_sym_t h, int *ngpus); /* shards of the handle (1: plain) */
/* How the shards of a multi-device handle that live on ANOTHER device than its home reach x / y.
 * REPLICATE (default; env CFS_MULTI_X=replicate): x is replicated -- one peer copy home ->
 * device per shard and SpMV, kernels gather x and write their y block in local HBM, one peer
 * copy brings the block home (north_star: "x replicated").  PEER (CFS_MULTI_X=peer): kernels
 * read x / write y in the home device's memory through peer access over xGMI, no copies.
 * REPLICATE_ALL copies for shards on the home device too (tests on a one-GPU box).
 * NOTE: with more than one physical device neither form has run on hardware yet (the build
 * and test boxes have one GPU); treat cross-device operation as unverified.           */
#define CFS_HIP_XMODE_PEER 0
#define CFS_HIP_XMODE_REPLICATE 1
#define CFS_HIP_XMODE_REPLICATE_ALL 2
int cfs_hip_sym_multi_set_xmode(cfs_hip_sym_t h, int xmode);
/* The exchange of a multi-device handle whose shards are in the exchange form
 * (CFS_HIP_FLAG_SHARD_EXCHANGE at create, or env CFS_MULTI_EXCHANGE=reduce_scatter | sparse), switched
 * at run time; the buffers of a form are allocated at its first use.
 * REDUCE_SCATTER (what the flag alone selects): the packed contributions are scattered into a zeroed
 * vector of ngpus equal blocks and ONE cfs_hip_comm_reduce_scatter hands every owner its sums --
 * seven launches per shard and SpMV (memset, tiles, pack, scatter, sum, local fold, add).
 * SPARSE (CFS_MULTI_EXCHANGE=sparse at create): ONE cfs_hip_comm_alltoallv moves the packed values
 * alone, one per remote boundary row, and the owner folds them in with the receive fold of a shard
 * (cfs_hip_sym_shard_set_recv, built here at the first switch) -- five launches (tiles, pack, pull,
 * local fold, receive fold).  A mirrored multi-device handle, a plain handle, a shard, NULL or an
 * unknown form: CFS_HIP_ERR_ARG.                                                            */
#define CFS_HIP_EXCHANGE_REDUCE_SCATTER 0
#define CFS_HIP_EXCHANGE_SPARSE 1
int cfs_hip_sym_multi_set_exchange(cfs_hip_sym_t h, int form);
/* *form = the current form; *values_moved = values the ranks hand to the collective per SpMV under
 * it (SPARSE: the sum of the shards' packed values; REDUCE_SCATTER: ngpus * ngpus * longest block);
 * *bytes_moved = that times the value size.  Any of the three may be NULL.  Handles: as above. */
int cfs_hip_sym_multi_exchange_info(cfs_hip_sym_t h, int *form, int64_t *values_moved, int64_t *bytes_moved);
/* devices[g] = device of shard g (may be NULL); *distinct = number of distinct devices */
int cfs_hip_sym_multi_devices(cfs_hip_sym_t h, int *devices, int capacity, int *distinct);
/* nnz_low-balanced row boundaries (multiples of 16, csr_matrix.tpp:418) for
 * sharding; row_splits has nranks+1 entries.                                 */
int cfs_hip_sym_balanced_splits(int n, const int *rowptr, const int *colind,
                                int nranks, int *row_splits);
int cfs_hip_sym_destroy(cfs_hip_sym_t h);
/* New values, SAME sparsity pattern (a stiffness matrix reassembled in every Newton step;
 * the reference would run tune() -- split, conflict graph, colouring,
 * csr_matrix.tpp:1204-1639 -- again): `values` is the full CSR value array in the order
 * of the rowptr / colind the handle was created from, nnz entries, host or device
 * pointer.  A device kernel pours it into the existing schedule (the value half of
 * tune()'s packing, on the GPU); tiles, slots, fold index stay.  The handle must have
 * been created with CFS_HIP_FLAG_KEEP_VALUE_MAP; returns after the new values are in
 * place.  Not for CFS_HIP_FLAG_DETERMINISTIC handles (their scale depends on the values).
 * Ordering: the pour runs on the library's own stream of the handle's device (on the home device
 * the one cfs_hip_default_stream returns), a BLOCKING stream -- it orders behind work on the null
 * stream -- and the call waits for it (a multi-device handle: then for every shard's pour), so an
 * SpMV enqueued afterwards on any stream multiplies with the new values.  What the library cannot
 * see is the caller's to order BEFORE the call: SpMVs of this handle still in flight on a
 * non-blocking stream of the caller's, and a device `values` array still being produced on such a
 * stream.  A matrix without stored entries (nnz = 0) has nothing to pour: the call with nnz = 0 and
 * a non-null `values` succeeds and changes nothing.  A refused call (CFS_HIP_ERR_ARG: a null
 * argument, the other value type's entry, another nnz, a handle without the map;
 * CFS_HIP_ERR_UNSUPPORTED: a deterministic handle) leaves the handle as it was.                    */
int cfs_hip_sym_update_values_f64(cfs_hip_sym_t h, const double *values, long long nnz);
int cfs_hip_sym_update_values_f32(cfs_hip_sym_t h, const float *values, long long nnz);

/* ---- dense_vector_multiply (replaces spmv_fn = cpu_mv_sym_conflict_free_v2,
 *      csr_matrix.tpp:2965-3028).  y is fully overwritten (the reference test
 *      never zeroes it: test/test_spmv_mmf.cpp:71,82-83); x and y must not
 *      alias.  x has n entries, y has n entries (block rows for a shard).
 *
 * cfs_hip_sym_spmv      : x / y may be host or device pointers (detected).
 *                         With a host pointer the call stages through PCIe and
 *                         returns after the result is complete.  With both
 *                         vectors device-resident it is enqueued on the
 *                         library stream and returns at once; cfs_hip_memcpy
 *                         and cfs_hip_synchronize(NULL) wait for that stream,
 *                         so a caller that reads y back always sees it done.
 * cfs_hip_sym_spmv_async: device pointers only, enqueued on `stream`
 *                         (a hipStream_t; NULL = HIP's null stream), returns
 *                         immediately.
 *
 * NaN and Inf.  The product is y_i = d_i x_i + sum over the stored off-diagonal (i, j) of
 * a_ij x_j, with d_i = 0 where no diagonal is stored (the reference's SSS kernels with their
 * dense diagonal, csr_matrix.tpp:2989): row i is non-finite if and only if x_i is, or a stored
 * (i, j) / (j, i) has a non-finite x_j or a_ij -- a missing diagonal does not shield a row from
 * its own x_i -- and every other row is the number it would be without the NaN / Inf (no clamped
 * or padded load is ever multiplied in).  Where x_i is finite the class of a non-finite y_i (NaN,
 * +Inf, -Inf) is that of the plain IEEE evaluation.  Where x_i itself is non-finite, y_i has
 * that class or is NaN: a row the schedule splits over several lanes carries its diagonal in
 * the first lane only and adds 0 * x_i in the others, so x_i = +-Inf may give NaN there where the
 * reference has +-Inf (which rows are split depends on the tile's other rows and on the order
 * of the rows).  CFS_HIP_FLAG_DETERMINISTIC handles: per tile, see the flag.
 * (tests/test_gpu_sym_confinement.py)                                                    */
int cfs_hip_sym_spmv(cfs_hip_sym_t h, void *y, const void *x);
/* A solver-style caller of the path, native (no counterpart in the reference: its only callers
 * are a benchmark loop and a self-check with a fixed x, bench/bench_spmv_mmf.cpp:139-173):
 * conjugate gradients for A u = b on RESIDENT vectors of a symmetric positive definite matrix.
 * u_dev: in = first guess, out = solution; b_dev: right-hand side; both device pointers of the
 * handle's device and value type, 16-byte aligned.  An iteration is five launches on `stream` -- the SpMV (two),
 * p.q, the fused update of u and r with r.r, the new direction -- with every scalar in device
 * memory: no host round trip inside the loop; the host reads the convergence flag every
 * `check_every` iterations (<= 0: 8; at most 16).  Stops when ||r|| <= tol ||b|| (the recurrence's r) or after
 * maxiter iterations; *iterations = iterations done, *relres = ||b - A u|| / ||b|| RECOMPUTED from
 * the returned u.  Dot products are accumulated in fp64.  Returns after the result is complete.
 * A handle of the whole matrix: one device, or a multi-device handle (cfs_hip_sym_create_multi_*:
 * the vector kernels run on its home device, the products on all of them); not a shard.       */
int cfs_hip_sym_cg(cfs_hip_sym_t h, void *u_dev, const void *b_dev, double tol, int maxiter, int check_every,
                   int *iterations, double *relres, void *stream);
/* The same iteration with a preconditioner.  CFS_HIP_PRECOND_NONE is cfs_hip_sym_cg: the same code
 * path, the same bits.  CFS_HIP_PRECOND_JACOBI runs
 *     r = b - A u;  z = D^-1 r;  p = z;  rz = r.z
 *     q = A p;  alpha = rz / p.q;  u += alpha p;  r -= alpha q;  z = D^-1 r;  rz' = r.z;  rr' = r.r
 *     beta = rz' / rz;  p = z + beta p
 * with D the diagonal of the handle (gathered from its device arrays, as cfs_hip_sym_diagonal_async
 * does, so it follows cfs_hip_sym_update_values_*).  STILL five launches per iteration and no host
 * round trip: dinv_i = (V)(1.0 / (double)a_ii) is stored once in the value type; z_i = (double)r_i *
 * (double)dinv_i (r_i as stored) is formed in fp64 inside the fused update (for r.z) and the direction
 * kernel and never written to memory.  Stops on the UNPRECONDITIONED residual, r.r <= tol^2 b.b --
 * the rule of cfs_hip_sym_cg, so iteration counts and tolerances of the two compare directly.
 * Alignment, placement, check_every, *iterations, *relres, CFS_HIP_CG_GRAPH and the handles
 * accepted are those of cfs_hip_sym_cg (a shard: CFS_HIP_ERR_UNSUPPORTED).  A diagonal entry that is
 * zero (or not stored), negative or not finite: CFS_HIP_ERR_ARG, u untouched, *iterations = 0.  An
 * unknown `precond`: CFS_HIP_ERR_ARG.                                                         */
#define CFS_HIP_PRECOND_NONE 0
#define CFS_HIP_PRECOND_JACOBI 1
int cfs_hip_sym_pcg(cfs_hip_sym_t h, void *u_dev, const void *b_dev, int precond, double tol, int maxiter,
                    int check_every, int *iterations, double *relres, void *stream);
int cfs_hip_sym_spmv_async(cfs_hip_sym_t h, void *y_dev, const void *x_dev,
                           void *stream);
/* d_dev[i - row_begin] = a_ii for the rows the handle owns (n for a whole matrix, the block for a
 * shard), 0 where the matrix stores none; device pointer of the handle's device and value type;
 * enqueued on `stream`.  Read from the handle's DEVICE arrays, so it follows
 * cfs_hip_sym_update_values_* and needs nothing of the caller's CSR (which may have been freed
 * after tune()).  One launch, every entry written exactly once (no atomics, nothing zeroed first).
 * A multi-device handle gathers every block on its shard's device and stream and brings it home
 * the way the y block of an SpMV comes home (cfs_hip_sym_multi_set_xmode).  A null argument, a
 * host pointer or a pointer on another device: CFS_HIP_ERR_ARG.                              */
int cfs_hip_sym_diagonal_async(cfs_hip_sym_t h, void *d_dev, void *stream);
/* The block_rows x block_rows diagonal blocks of the matrix (the node blocks of a multi-dof mesh
 * matrix), the sibling of cfs_hip_sym_diagonal_async: block k holds rows and columns [k bs, min((k + 1)
 * bs, n)) of the caller's numbering, nb = ceil(n / bs) blocks, bs = block_rows one of 1, 2, 3, 4, 6
 * (anything else: CFS_HIP_ERR_ARG).  blocks_dev receives nb bs^2 values of the handle's value type,
 * row-major per block: blocks_dev[k bs^2 + (i mod bs) bs + (j mod bs)] = a_ij, both triangles, 0 where
 * the matrix stores no entry and in the positions of a trailing partial block that lie outside the
 * matrix.  Every word is defined after the call (the zeroing is enqueued on `stream` in front of the
 * gather) and nothing outside the nb bs^2 words is written.  Read from the handle's DEVICE arrays,
 * like the diagonal: it follows cfs_hip_sym_update_values_*, needs nothing of the caller's CSR and
 * works on a handle from cfs_hip_sym_load.  The diagonal positions are bit for bit what
 * cfs_hip_sym_diagonal_async returns (bs = 1: the output IS that diagonal); an off-diagonal position
 * holds the stored value, the sum where the matrix stores the position more than once, as the SpMV
 * gives (+-0 need not keep its sign).  A whole-matrix handle on one device only: blocks straddle the
 * row splits (multiples of 16, not of bs), so a shard or a multi-device handle gets
 * CFS_HIP_ERR_UNSUPPORTED -- merging two owners' halves of a block is left for a later change.  A
 * null argument, a host pointer or a pointer on another device: CFS_HIP_ERR_ARG.             */
int cfs_hip_sym_block_diagonal_async(cfs_hip_sym_t h, int block_rows, void *blocks_dev, void *stream);
/* cfs_hip_sym_pcg with M = blockdiag(A) at block size block_rows: z = M^-1 r.  block_rows = 1 is
 * CFS_HIP_PRECOND_JACOBI, the same code path, the same bits.  For 2, 3, 4, 6: once per call the blocks
 * are gathered (as cfs_hip_sym_block_diagonal_async does) and inverted, one thread per block in fp64
 * (the block read as stored; Cholesky, then the inverse; the positions of a trailing partial block
 * outside the matrix count as identity); the inverse is kept rounded to the value type.  STILL five
 * launches per iteration and no host round trip: z_i = sum_j (double)Minv_ij (double)r_j over the
 * block (r_j as stored) is formed in fp64 inside the fused update and the direction kernel and never
 * written to memory; the same fixed-order partial sums, so a solve on a deterministic handle is
 * bit-reproducible.  Stopping rule, check_every, *iterations, *relres, alignment, placement and
 * CFS_HIP_CG_GRAPH are those of cfs_hip_sym_pcg.  A block whose Cholesky pivot is not finite and > 0
 * ("not positive definite": an indefinite block, a NaN, a missing diagonal entry): CFS_HIP_ERR_ARG, u
 * untouched, *iterations = 0.  Another block_rows: CFS_HIP_ERR_ARG.  A shard or a multi-device
 * handle: CFS_HIP_ERR_UNSUPPORTED.                                                            */
int cfs_hip_sym_pcg_block(cfs_hip_sym_t h, void *u_dev, const void *b_dev, int block_rows, double tol, int maxiter,
                          int check_every, int *iterations, double *relres, void *stream);
/* For developers and tests: the inverse blocks cfs_hip_sym_pcg_block would use at this moment, as
 * nb bs^2 values, full row-major blocks of the value type (both triangles, identity in the positions
 * of a trailing partial block outside the matrix) -- the solver's two set-up kernels plus an unpack,
 * so that a test can run the SAME preconditioner in higher precision.  A block that is not positive
 * definite leaves non-finite or meaningless words; no error is raised for it here.  Arguments and
 * handles as for cfs_hip_sym_block_diagonal_async; temporary device memory is released before the
 * call returns, which waits for the kernels.                                                  */
int cfs_hip_sym_block_inverse_async(cfs_hip_sym_t h, int block_rows, void *minv_dev, void *stream);
/* Mixed-precision PCG: an fp64 solution from fp32 products.  h64 and h32 are whole-matrix handles of the
 * SAME matrix on one device, h64 with fp64 values and h32 with fp32 values (the caller builds both; the
 * memory cost is both matrices resident); u_dev (first guess in, solution out) and b_dev are fp64.
 * One CG recurrence runs in fp32 on h32 with the launches of cfs_hip_sym_cg / _pcg / _pcg_block,
 * unchanged and in the same order -- five per iteration, no host round trip -- and accumulates a
 * correction xlo (fp32) to u.  A REPLACEMENT is made once the recurrence's r.r is no longer above
 * max(tol^2 b.b, delta^2 rr_ref), rr_ref the largest r.r seen at a host look since the last replacement
 * (delta in (0, 1); 0 means the default 0.1).  The device evaluates that at every iteration -- a
 * sixth, single-workgroup launch behind the direction kernel raises the flag that makes the launches
 * enqueued behind it return at once -- and the host acts on the flag at its next look, every
 * check_every (at most 16) iterations:
 *     u += (double)xlo;  xlo = 0;  q64 = A64 u;  r = (float)(b - q64);  r.r from the unrounded fp64
 *     residual;  r.z from the rounded r and the fp32 preconditioner
 * The search direction p is kept across a replacement ("CG with residual replacement"), so the Krylov
 * space is not thrown away as a restart of the iteration would.  The preconditioner is built from h32:
 * block_rows 0 none, 1 Jacobi, 2 / 3 / 4 / 6 block Jacobi (anything else: CFS_HIP_ERR_ARG); a diagonal
 * or a block that is not positive is refused as by cfs_hip_sym_pcg / _pcg_block, u untouched.  The solve
 * ends when a replacement's true residual has r.r <= tol^2 b.b (or is NaN), or after maxiter fp32
 * iterations, then with a closing fold and true residual.  *iterations: fp32 iterations done;
 * *replacements: replacements made inside the loop (neither the first residual nor the closing one
 * counts); *relres: ||b - A64 u|| / ||b|| of the returned u, in fp64 (||b - A64 u|| when b = 0).  The
 * scalars are fixed-order partial sums: on two CFS_HIP_FLAG_DETERMINISTIC handles the solve is
 * bit-reproducible.  CFS_HIP_CG_GRAPH is not consulted.
 * CFS_HIP_ERR_ARG: a null pointer, u == b, u or b not 16-byte aligned, a host pointer or a pointer on
 * another device, handles on two devices, h64 not fp64 or h32 not fp32, different n, delta outside
 * (0, 1), tol < 0, maxiter < 0.  A shard or a multi-device handle: CFS_HIP_ERR_UNSUPPORTED.       */
int cfs_hip_sym_pcg_mixed(cfs_hip_sym_t h64, cfs_hip_sym_t h32, void *u_dev, const void *b_dev, int block_rows, double tol,
                          double delta, int maxiter, int check_every, int *iterations, int *replacements, double *relres,
                          void *stream);
/* cfs_hip_sym_pcg with a Chebyshev polynomial in M^-1 A as the preconditioner, z = P_m r.  M is the base:
 * block_rows 0 means M = I, 1 the diagonal of cfs_hip_sym_pcg, 2 / 3 / 4 / 6 the node blocks of
 * cfs_hip_sym_pcg_block (anything else: CFS_HIP_ERR_ARG); dinv and the inverse blocks are built and stored exactly
 * as there.  With theta = (lmax + lmin) / 2, delta = (lmax - lmin) / 2, sigma1 = theta / delta, rho_0 = 1 / sigma1,
 *     z_1 = d_1 = (1 / theta) M^-1 r
 *     j = 1 .. m - 1:  t = A z_j;  rho_j = 1 / (2 sigma1 - rho_{j-1})
 *                      d_{j+1} = rho_j rho_{j-1} d_j + (2 rho_j / delta) M^-1 (r - t);  z_{j+1} = z_j + d_{j+1}
 * the Chebyshev iteration for A z = r from z = 0: degree m = `degree` (1 .. 16) costs m - 1 products; degree 1
 * is the base preconditioner scaled by 1 / theta and makes none.  For fixed bounds P_m is a fixed symmetric linear
 * operator, so plain PCG is valid with it.  THE MARGIN: 1 - lambda p(lambda) = T_m((theta - lambda) / delta) /
 * T_m(sigma1) has modulus below 1 exactly for lambda in (0, lmin + lmax), so P_m is positive definite as long as
 * every eigenvalue of M^-1 A lies in that open interval.  An lmax that is a little low is therefore survivable
 * (lmin covers it); one that is badly low makes P_m indefinite, PCG then promises nothing, and *relres says so.
 * BOUNDS: lmax <= 0 means 1.1 x the estimate of cfs_hip_sym_precond_lmax (16 steps from its default start vector,
 * made inside this call); lmin <= 0 means lmax / 30.  The 1.1 and the 30 are the conventions of PETSc's and
 * Ifpack2's Chebyshev smoothers, not numbers measured here.  bounds_used (2 doubles, or NULL) receives the pair
 * actually used, lmin then lmax, so a caller who solves many systems pays for the estimate once.
 * LAUNCHES: 5 + 3 (m - 1) per outer iteration -- the product and p.q, a fused update (u, r, r.r and z_1 in one
 * pass), per inner step the product and one fused kernel (r, t, d, z and M^-1 read, d and z written: 7 n words
 * against the 13 n of a CG iteration), the direction kernel.  The coefficient pairs are computed on the host in
 * fp64 and passed as kernel arguments: an inner step has no dot product and reads no device scalar.  The host looks
 * at the convergence flag every min(check_every, 16, max(1, 80 / (5 + 3 (m - 1)))) iterations (check_every <= 0:
 * 8).  Memory held during the call: five vectors (r, p, q, z, d; t lives in q) and the stored M^-1.
 * ROUNDING: z, d and t are stored in the value type; every update is computed in fp64 from the stored operands and
 * rounded once; M^-1 (r - t) is formed in fp64 from (double)r_i - (double)t_i; r.z sums (double)r_i (double)z_i of
 * the stored r and the stored final z; r.r as in cfs_hip_sym_pcg; all in the same fixed-order partial sums, so a
 * solve on a CFS_HIP_FLAG_DETERMINISTIC handle is bit-reproducible.  Stops on the UNPRECONDITIONED residual,
 * r.r <= tol^2 b.b, the rule of cfs_hip_sym_pcg; a NaN ends the solve; *iterations = outer iterations done,
 * *relres = ||b - A u|| / ||b|| RECOMPUTED from the returned u.  CFS_HIP_CG_GRAPH is not consulted.
 * Handles: block_rows 0 or 1, those of cfs_hip_sym_pcg (a multi-device handle is accepted, a shard gets
 * CFS_HIP_ERR_UNSUPPORTED); block_rows >= 2, those of cfs_hip_sym_pcg_block.  A diagonal entry or a block that is
 * not positive is refused exactly as there: CFS_HIP_ERR_ARG, u untouched, *iterations = 0.
 * CFS_HIP_ERR_ARG, before any device work: a null pointer (checked first), u == b, u or b not 16-byte aligned,
 * tol < 0, maxiter < 0, another block_rows, a degree outside 1 .. 16, a bound that is not finite, lmin >= lmax when
 * both are given; then a host pointer or a pointer on another device.  Also CFS_HIP_ERR_ARG, u untouched: no
 * positive estimate (A or M indefinite, or A = 0), or a given lmin that is not below the estimated lmax.     */
int cfs_hip_sym_pcg_cheb(cfs_hip_sym_t h, void *u_dev, const void *b_dev, int block_rows, int degree, double lmin,
                         double lmax, double tol, int maxiter, int check_every, int *iterations, double *relres,
                         double *bounds_used, void *stream);
/* z = P_m r alone: the polynomial of cfs_hip_sym_pcg_cheb, by the same kernels and with the same rounding, for a
 * caller who wants it as a smoother and for tests that pin the chain by itself.  Both bounds are required
 * (0 < lmin < lmax, finite).  z_dev (fully overwritten) and r_dev: different device vectors of n values of the
 * handle's value type on its device, 16-byte aligned.  block_rows, degree and the handles accepted as for
 * cfs_hip_sym_pcg_cheb.  m - 1 products and 1 + 3 (m - 1) launches; two vectors of temporary device memory and the
 * stored M^-1, released before the call returns, which waits for the kernels.  A diagonal entry or a block that
 * is not positive: CFS_HIP_ERR_ARG once the kernels have run, z then holds nothing meaningful.              */
int cfs_hip_sym_cheb_apply(cfs_hip_sym_t h, int block_rows, int degree, double lmin, double lmax, void *z_dev,
                           const void *r_dev, void *stream);
/* An estimate of lambda_max(M^-1 A) by `steps` power steps (<= 0: 16), M as for cfs_hip_sym_pcg_cheb:
 *     t = A v;  w = M^-1 t;  est = (w.t) / (v.t);  v = w / sqrt(w.w)
 * from v = v0_dev (n device values of the value type; NULL: the start vector of cfs_hip_sym_eigs).  w and v are
 * stored in the value type, all dots are fixed-order fp64 partial sums of the stored values, and the normalising
 * scalar is read on the device: there is no host look until the last step.  *estimate is the last est.  For
 * positive definite A and M, est = y^T B^2 y / y^T B y with B = M^-1/2 A M^-1/2 and y = M^1/2 v, so it never
 * exceeds lambda_max(M^-1 A) (up to rounding): it is a LOWER estimate, which is why cfs_hip_sym_pcg_cheb multiplies
 * it by 1.1 and keeps the margin described there.  Per step: the product and two launches (the last step: one).
 * A diagonal entry or a block that is not positive: CFS_HIP_ERR_ARG.  Handles as for cfs_hip_sym_pcg_cheb.     */
int cfs_hip_sym_precond_lmax(cfs_hip_sym_t h, int block_rows, int steps, const void *v0_dev, double *estimate,
                             void *stream);
/* Host only, no device work: *theta and the degree - 1 coefficient pairs cfs_hip_sym_pcg_cheb would pass to its
 * inner steps for these bounds, c1[j-1] = rho_j rho_{j-1} and c2[j-1] = 2 rho_j / delta for j = 1 .. degree - 1
 * (c1, c2: degree - 1 doubles each; may be NULL at degree 1).  Both bounds required, 0 < lmin < lmax.          */
int cfs_hip_debug_cheb_coeffs(int degree, double lmin, double lmax, double *theta, double *c1, double *c2);
/* ---- aggregation multigrid: a V-cycle as the preconditioner of the native PCG ------------------------------------
 * For scalar problems whose condition number, not their size, is the cost: the iteration count of every solver above
 * grows with its square root, a multilevel cycle removes the low end of the spectrum.  (On a multi-dof matrix whose
 * couplings inside a node are as strong as the diagonal use the node-block form, cfs_hip_amg_create_block_* below: this
 * one does worse than block Jacobi there.)  CFS_HIP_ABI_VERSION is unchanged; callers detect the symbols.
 * THE HIERARCHY, built on the host in fp64 from the caller's CSR (as for cfs_hip_sym_create_*: only entries with
 * col <= row are read).  Per level l, A_0 = A:  w_i = 1 / sqrt(a_ii), B = W A_l W;  `passes` rounds of pairwise
 * matching on B -- the rows in ascending order, an unmatched row i takes the unmatched neighbour j != i with the largest
 * s_ij = |b_ij| / sqrt(b_ii b_jj) > 0, ties to the smallest j; the pair is the next aggregate, a row without a candidate
 * a singleton -- each followed by B <- Q^T B Q, every coarse entry the fp64 sum of its contributions in ascending
 * (row, column) order.  agg_l is the composition of the rounds (at most 2^passes members per aggregate),
 * P_l = W Q_1 .. Q_p and A_{l+1} = P_l^T A_l P_l, rounded to the value type before it is coarsened further.  The weights
 * make the hierarchy invariant under a symmetric scaling of A.  Level l is the last one, DENSE, when n_l <= coarse_max;
 * otherwise, when the coarsening stalls (n_{l+1} > 0.9 n_l) or l + 1 == CFS_HIP_AMG_MAX_LEVELS, it is the last one,
 * dense when n_l <= CFS_HIP_AMG_MAX_COARSE and SMOOTHER-ONLY otherwise: a stalled hierarchy degrades to the Chebyshev
 * preconditioner, never to an error.  The dense level keeps the inverse (Cholesky in fp64, solves, symmetrised, rounded
 * to the value type) as an n_L x n_L device array.  Levels 1 .. L are handles of the library's own create path
 * (CFS_HIP_FLAG_NO_CALIBRATE, plus CFS_HIP_FLAG_DETERMINISTIC when h has it); level 0 is h itself, not copied.
 * Every other level smooths with the Chebyshev polynomial of `degree` in D^-1 A_l on [lmax / ratio, lmax],
 * lmax = 1.1 x the power-method estimate (Jacobi, 16 steps, the fixed start vector), made at create.
 * THE CYCLE z = M^-1 r:  dense level: z = A_L^-1 r, one kernel; smoother-only level: z = S_l r; otherwise z = S_l r,
 * t = A_l z, rc_I = sum_{i in I} w_i (r_i - t_i), ec = cycle(l + 1, rc), z_i += w_i ec_agg(i), then the Chebyshev
 * iteration again from that z.  8 + 6 (degree - 1) launches per multigrid level, 1 + 3 (degree - 1) on a
 * smoother-only level, 1 on the dense one.  Vectors are stored in the value type, every update is computed in fp64
 * from the stored operands and rounded once, all sums have a fixed order.  M^-1 is symmetric; it is positive definite
 * while every level's spectrum of D^-1 A_l lies in (0, lmin + lmax), the margin of cfs_hip_sym_pcg_cheb:
 * 1.375 x the estimate at ratio 4.
 * MEMORY: per level dinv, w, the aggregate lists, the work vectors r, z, d, t and the level's handle
 * (cfs_hip_amg_info reports the bytes).                                                                          */
#define CFS_HIP_AMG_MAX_LEVELS 16
#define CFS_HIP_AMG_MAX_COARSE 1024
typedef struct cfs_hip_amg_s *cfs_hip_amg_t;
typedef struct {
  int passes;     /* rounds of pairwise matching per level, 1 .. 3 (0: 2)          */
  int degree;     /* of the smoother, 1 .. 4 (0: 1)                                */
  int coarse_max; /* largest dense last level, 1 .. CFS_HIP_AMG_MAX_COARSE (0: 512) */
  int reserved_;
  double ratio;   /* lmax / lmin of the smoother, finite and > 1 (0: 4)            */
} cfs_hip_amg_options; /* 0 = default */
#define CFS_HIP_AMG_KIND_MULTIGRID 0
#define CFS_HIP_AMG_KIND_SMOOTHER 1
#define CFS_HIP_AMG_KIND_DENSE 2
typedef struct {
  int levels, passes, degree, coarse_max; /* the options as used */
  double ratio;
  long long device_bytes;  /* held by the object: the level handles, the transfer lists, the vectors, the inverse  */
  double setup_seconds;    /* the whole create ...                                                                  */
  double handles_seconds;  /* ... of which the create path of the level handles                                     */
  int n[CFS_HIP_AMG_MAX_LEVELS];
  long long nnz[CFS_HIP_AMG_MAX_LEVELS]; /* stored: lower triangle + diagonal */
  double lmin[CFS_HIP_AMG_MAX_LEVELS], lmax[CFS_HIP_AMG_MAX_LEVELS]; /* 0 on a dense level */
  int kind[CFS_HIP_AMG_MAX_LEVELS]; /* CFS_HIP_AMG_KIND_* */
} cfs_hip_amg_info_t;
/* The hierarchy of the matrix behind h.  h: a whole-matrix handle on one device of the matching value type and n (a
 * shard or a multi-device handle: CFS_HIP_ERR_UNSUPPORTED); it must outlive the object, and the caller vouches that the
 * CSR is h's matrix.  THE HIERARCHY HOLDS THE VALUES AT CREATE: to follow cfs_hip_sym_update_values_* make it with
 * cfs_hip_amg_create_refreshable_* and call cfs_hip_amg_update_values_* (below).
 * CFS_HIP_ERR_ARG, before any device work and in this order: a null pointer (h, rowptr, out;
 * colind / values when there are entries), passes outside 1 .. 3, degree outside 1 .. 4, a ratio that is not finite and
 * > 1, coarse_max outside 1 .. CFS_HIP_AMG_MAX_COARSE (0 is the default in each).  Then, from the handle: a shard or a
 * multi-device handle (CFS_HIP_ERR_UNSUPPORTED), a value type or an n different from h's (CFS_HIP_ERR_ARG).  A diagonal entry of any level that is zero, missing, negative or not finite: CFS_HIP_ERR_ARG in
 * the words of cfs_hip_sym_pcg; a dense level whose Cholesky factorisation meets a pivot that is not finite and > 0:
 * CFS_HIP_ERR_ARG ("not positive definite").  On any error *out = NULL and nothing stays allocated.             */
int cfs_hip_amg_create_f64(cfs_hip_sym_t h, int n, const int *rowptr, const int *colind, const double *values,
                           const cfs_hip_amg_options *opt, cfs_hip_amg_t *out);
int cfs_hip_amg_create_f32(cfs_hip_sym_t h, int n, const int *rowptr, const int *colind, const float *values,
                           const cfs_hip_amg_options *opt, cfs_hip_amg_t *out);
int cfs_hip_amg_destroy(cfs_hip_amg_t a); /* NULL is allowed */
/* ---- the LOCALLY DOMINANT matching, and the set-up on the device --------------------------------------------------
 * The matching above is sequential by definition (row i's choice depends on row i - 2's on a chain).  The second
 * matching is parallel by definition and deterministic; everything else of a level -- w, B = W A W, B <- Q^T B Q with
 * the sums in the same order, the rounding to the value type, the rules that end a hierarchy, the smoother, the dense
 * inverse and the cycle -- is unchanged.  One round of pairwise matching on B:
 *   CANDIDATE EDGES: every off-diagonal entry with s_ij = |b_ij| / sqrt(b_ii b_jj) > 0, the fp64 expression above (the
 *   product b_ii b_jj and the stored b_ij = b_ji give both endpoints the same bits).
 *   TOTAL ORDER of the edges: (1) the larger s first; (2) at equal s (compared as doubles) the edge whose smaller
 *   endpoint lo = min(i, j) is even; (3) then the smaller h(lo, hi); (4) then the smaller (lo, hi).  h is this 32-bit
 *   mix, all arithmetic mod 2^32:
 *     x = (lo * 0x9E3779B1u) ^ (hi * 0x85EBCA77u);  x ^= x >> 15;  x *= 0x2C1B3C6Du;  x ^= x >> 12;  x *= 0x297A2D39u;
 *     x ^= x >> 15
 *   SYNCHRONOUS ROUNDS: every free row that has a free neighbour over a candidate edge points to the first such edge in
 *   the total order; all pointers are computed from the state at the start of the round; rows that point at each
 *   other become a pair.  The rounds end with a round that forms no pair (it is counted), or after
 *   CFS_HIP_AMG_MATCH_ROUNDS rounds; the rows still free are singletons.
 *   NUMBERING: the aggregates by their smallest member, ascending.
 * Below the cap the result is the matching of a sequential pass over the edges in the total order (take an edge when
 * both ends are free), whatever the schedule of the rounds.  The hash keeps the number of rounds logarithmic on chains of
 * equal weights (ties to the smallest index would need n / 2); the parity key lets naturally ordered grids match
 * perfectly in one round.  Heaviest-edge-first leaves more singletons on structured grids than the sweep in index
 * order: expect more iterations than with the greedy hierarchy (README), against a set-up that runs on the device.
 * cfs_hip_amg_create_dominant_*: the arguments, checks, messages and their order of cfs_hip_amg_create_*; the set-up on
 * the host with this matching; not refreshable.
 * cfs_hip_amg_create_device_*: the same arguments and checks, and THE SAME HIERARCHY IN EVERY BIT -- aggregates, w, every
 * level's pattern and values, the inverse -- built by HIP kernels, hipcub sorts and scans on the handle's device: level
 * 0's lower triangle from one upload of the caller's CSR (rows whose kept columns do not ascend strictly: read on the host,
 * as above, and uploaded), per level the weights, the scaling, both triangles by a stable sort of (row, col) records,
 * the rounds (one host look per round), Q^T B Q as lists over the stably sorted (I, J) records summed one thread per
 * coarse entry, the transfer; the coarse CSR comes to the host once per level for the level's handle and the dense
 * inverse.  In addition: a CSR with 2 nnz beyond 32-bit positions is CFS_HIP_ERR_UNSUPPORTED, before any device work;
 * a failed allocation returns the device error.  The scratch (cfs_hip_amg_setup_info) is freed before the call returns.
 * cfs_hip_amg_setup_info, for every hierarchy: *matching = CFS_HIP_AMG_MATCHING_*; *on_device = 0 (host), 1 (device) or
 * 2 (device, level 0's lower triangle read on the host); rounds[3 * level + pass] = the rounds of every pass (levels x 3
 * ints, 0 where none ran); seconds[4] of a device set-up: level 0's lower triangle with the upload, the matching, the
 * mirror + Galerkin product + transfer, the downloads; *scratch_bytes = the device scratch a device set-up held.  Greedy,
 * 0 and zeros for the entry points above.  Any of the five may be NULL.                                            */
#define CFS_HIP_AMG_MATCHING_GREEDY 0
#define CFS_HIP_AMG_MATCHING_DOMINANT 1
#define CFS_HIP_AMG_MATCH_ROUNDS 64
int cfs_hip_amg_create_dominant_f64(cfs_hip_sym_t h, int n, const int *rowptr, const int *colind, const double *values,
                                    const cfs_hip_amg_options *opt, cfs_hip_amg_t *out);
int cfs_hip_amg_create_dominant_f32(cfs_hip_sym_t h, int n, const int *rowptr, const int *colind, const float *values,
                                    const cfs_hip_amg_options *opt, cfs_hip_amg_t *out);
int cfs_hip_amg_create_device_f64(cfs_hip_sym_t h, int n, const int *rowptr, const int *colind, const double *values,
                                  const cfs_hip_amg_options *opt, cfs_hip_amg_t *out);
int cfs_hip_amg_create_device_f32(cfs_hip_sym_t h, int n, const int *rowptr, const int *colind, const float *values,
                                  const cfs_hip_amg_options *opt, cfs_hip_amg_t *out);
int cfs_hip_amg_setup_info(cfs_hip_amg_t a, int *matching, int *on_device, int *rounds, double *seconds,
                           long long *scratch_bytes);
/* ---- a hierarchy that follows cfs_hip_sym_update_values_*: the numeric re-set-up with the aggregates kept ---------
 * cfs_hip_amg_create_refreshable_*: the arguments and rules of cfs_hip_amg_create_*, and the same hierarchy bit for
 * bit; the level handles are created with CFS_HIP_FLAG_KEEP_VALUE_MAP and the object keeps, on the device, what a refresh
 * evaluates (below).  In addition: a CFS_HIP_FLAG_DETERMINISTIC handle is CFS_HIP_ERR_UNSUPPORTED (its levels would
 * be deterministic, and those refuse update_values), a level whose contributions per round exceed 32-bit indices
 * CFS_HIP_ERR_UNSUPPORTED.
 * cfs_hip_amg_create_* itself is unchanged, in behaviour and in the bytes it holds.
 * cfs_hip_amg_update_values_*: `values` is the caller's full CSR value array in the order of the rowptr / colind given
 * at create, nnz entries, host or device pointer, as for cfs_hip_sym_update_values_*.  The call runs on the library's
 * stream of the handle's device and returns when the hierarchy is complete: a cfs_hip_sym_pcg_amg or cfs_hip_amg_apply
 * enqueued afterwards, on any stream, sees the new one.  THE REFRESH is the arithmetic of create with the matchings of
 * every round FROZEN, in the same order of operations, in HIP kernels over lists built at create:
 *   level 0: the lower triangle of `values`, duplicates summed in the order amg_lower reads them (gather-sum lists);
 *   per level: w_i = 1 / sqrt(a_ii) in fp64 ON THE DEVICE (division and sqrt are correctly rounded: the same bits as
 *   the host's at create), b_k = (w_row a_k) w_col per stored entry, then per round every entry of Q^T B Q as the fp64
 *   sum of its contributions in the order create adds them -- the members of the aggregate ascending, each member's
 *   row of the full B by ascending column, an entry above the diagonal read from its mirror (amg_gather_sum_kernel,
 *   one thread per output entry); the last round rounds to the value type;  the values are poured into the next
 *   level's handle through its update_values;  dinv, the power method (16 steps, the fixed start vector),
 *   lmax = 1.1 x the estimate, lmin and the coefficient pairs are made again per level;  the dense last level is
 *   brought to the host, inverted by the code of create and uploaded.
 * If a fresh create on the new values would choose the same aggregates, the refreshed hierarchy equals it in every
 * bit of w, of every level matrix and of the dense inverse (lmax: within the run-to-run spread of the product's
 * atomics).  agg, every pattern, the schedules of the level handles and the options stay.  Level 0 is h, not a
 * copy: the caller pours h's own array into h with cfs_hip_sym_update_values_*, before or after this call and before
 * the next cycle, and vouches, as at create, that the two arrays are one matrix.  Level 0's dinv and bound are taken
 * from h: they are made during the refresh from what h holds then and, when h has been poured since, once more by the
 * next cfs_hip_amg_apply or cfs_hip_sym_pcg_amg, on its stream (pouring h first saves that second power method;
 * cfs_hip_amg_info only reports, and until that cycle shows level 0's bound as the refresh made it).
 * cfs_hip_amg_level_matrix reads a refreshed level's values back from the device at its first call after a refresh.
 * CFS_HIP_ERR_ARG, the hierarchy untouched: a null argument, an object of cfs_hip_amg_create_*, the other value
 * type's entry point, another nnz -- these before any device work -- or `values` on another device.
 * FAILURE INSIDE A REFRESH -- a diagonal entry of a level that is zero, negative or not finite (counted on the device,
 * read at the level's host look), a power method without a positive estimate, a dense level that is not positive
 * definite: CFS_HIP_ERR_ARG in the words of create.  The object is then STALE: cfs_hip_amg_apply and
 * cfs_hip_sym_pcg_amg return CFS_HIP_ERR_ARG ("the last refresh failed") until a refresh succeeds; nothing is leaked
 * and the object can be destroyed.
 * cfs_hip_amg_refresh_info: *map_bytes = the device bytes the capability adds (the lists, two fp64 arrays of the
 * longest level and the fp64 weights, kept between calls, the levels' values on the device, and for each level
 * handle's value map 4 bytes per stored entry of the level -- that last part an ESTIMATE: the handle's own count,
 * which covers the padding of its format, is inside its device bytes), also counted in
 * cfs_hip_amg_info().device_bytes (there with the handles' own count of their maps); 0 for an object of
 * cfs_hip_amg_create_*.  *refreshes = successful refreshes, *last_seconds = the wall time of the last one.  Any of the
 * three may be NULL.  cfs_hip_debug_amg_refresh_split: seconds[4] of the last successful refresh -- the Galerkin
 * kernels (gather, weights, scaling, rounds), the pours, dinv + power method with its host look (all three between
 * events on the stream), the dense inverse with its two copies (host clock).                                        */
int cfs_hip_amg_create_refreshable_f64(cfs_hip_sym_t h, int n, const int *rowptr, const int *colind, const double *values,
                                       const cfs_hip_amg_options *opt, cfs_hip_amg_t *out);
int cfs_hip_amg_create_refreshable_f32(cfs_hip_sym_t h, int n, const int *rowptr, const int *colind, const float *values,
                                       const cfs_hip_amg_options *opt, cfs_hip_amg_t *out);
int cfs_hip_amg_update_values_f64(cfs_hip_amg_t a, const double *values, long long nnz);
int cfs_hip_amg_update_values_f32(cfs_hip_amg_t a, const float *values, long long nnz);
int cfs_hip_amg_refresh_info(cfs_hip_amg_t a, long long *map_bytes, int *refreshes, double *last_seconds);
int cfs_hip_debug_amg_refresh_split(cfs_hip_amg_t a, double *seconds);
/* The readers: what the launches read.  info: the level count and per level n, the stored nonzeros, the bounds and
 * the kind, the options used, the device bytes held and the set-up seconds.  level_aggregates (level < levels - 1):
 * agg[n_l], the aggregate of every row, and w[n_l] in the value type, both copied back from the device (either may be
 * NULL).  level_matrix (1 <= level < levels): the lower triangle + diagonal CSR the level's handle was created from,
 * rowptr[n_l + 1], colind[nnz_l], values[nnz_l] in the value type (any may be NULL).  coarse_inverse: the n_L x n_L
 * values of the dense level, copied back from the device; a hierarchy that ends smoother-only: CFS_HIP_ERR_ARG.   */
int cfs_hip_amg_info(cfs_hip_amg_t a, cfs_hip_amg_info_t *out);
int cfs_hip_amg_level_aggregates(cfs_hip_amg_t a, int level, int *agg, void *w);
int cfs_hip_amg_level_matrix(cfs_hip_amg_t a, int level, int *rowptr, int *colind, void *values);
int cfs_hip_amg_coarse_inverse(cfs_hip_amg_t a, void *inv);
/* One cycle, z = M^-1 r, enqueued on `stream`.  z_dev (fully overwritten) and r_dev: different device vectors of n
 * values of the value type on the handle's device, 16-byte aligned; nothing else of the caller's is written.  The work
 * vectors belong to the object: one cycle of an object at a time.  CFS_HIP_ERR_ARG: a null pointer, z == r, a pointer
 * that is not 16-byte aligned, a host pointer or one on another device.                                          */
int cfs_hip_amg_apply(cfs_hip_amg_t a, void *z_dev, const void *r_dev, void *stream);
/* One cycle on a BLOCK OF COLUMNS, enqueued on `stream`: Z_c = M^-1 R_c for every column c < ncols whose bit is set in
 * `active`; a column whose bit is clear is neither read nor written.  Column c of Z at z_dev + c ld values, of R at
 * r_dev + c ld values; rows [0, n) of the active columns of Z are fully overwritten, nothing else of the caller's is
 * written, R is not modified.  Every vector kernel of the cycle runs ONCE for the block -- a level costs the launches
 * of the one-column cycle, 4 at degree 1 and 2 more per further degree, whatever ncols -- and reads the level's data
 * (the inverse diagonal or blocks, W, the aggregates, the dense inverse) once per chunk of columns; the products stay
 * one per active column.  Per column the arithmetic is that of cfs_hip_amg_apply: on a CFS_HIP_FLAG_DETERMINISTIC
 * handle column c has the bits of cfs_hip_amg_apply on R_c alone.  Serves every hierarchy cfs_hip_amg_apply serves
 * (scalar, node-block, device-built, refreshable: the values poured into the fine handle since are followed).  The
 * levels' work vectors for ncols columns are allocated at the first call of that width and kept (counted in
 * cfs_hip_amg_info().device_bytes); only a wider call makes them again.  One cycle of an object at a time.
 * CFS_HIP_ERR_ARG, before any device work, in this order: a null pointer; ncols outside 1 .. CFS_HIP_LOBPCG_MAX_K; a
 * bit of `active` from ncols on; z_dev or r_dev not 16-byte aligned; ld < n, or ncols > 1 and ld sizeof(V) not a
 * multiple of 16; the two blocks overlap; a hierarchy whose last refresh failed; then as cfs_hip_amg_apply for a host
 * pointer or one on another device.  active == 0: returns 0 behind those checks and enqueues nothing.            */
int cfs_hip_amg_apply_cols(cfs_hip_amg_t a, void *z_dev, const void *r_dev, long long ld, int ncols, unsigned active,
                           void *stream);
/* *cycles: the cycles the object has applied to columns of blocks since it was created -- one per active column of
 * every cfs_hip_amg_apply_cols and of every W block formed by cfs_hip_sym_lobpcg_amg / _debug_lobpcg_amg (the
 * difference across a solve is the number of cycles it cost).  cfs_hip_amg_apply and cfs_hip_sym_pcg_amg do not count. */
int cfs_hip_amg_column_cycles(cfs_hip_amg_t a, long long *cycles);
/* cfs_hip_sym_pcg_cheb with the polynomial replaced by the cycle of `a`, which must have been created on h (otherwise
 * CFS_HIP_ERR_ARG): the same residual kernel, the same stopping rule on the UNPRECONDITIONED residual, r.r <= tol^2 b.b;
 * a NaN ends the solve; *relres is RECOMPUTED from the returned u; r.z sums the stored r and the stored final z; all
 * scalars are fixed-order partial sums, so a solve on a CFS_HIP_FLAG_DETERMINISTIC handle is bit-reproducible.  Per
 * iteration: the product, four vector kernels and the cycle.  A cycle is more than may be enqueued between two host
 * looks, so the host looks at the convergence flag after EVERY iteration; check_every is accepted and not used.
 * Argument checks as for cfs_hip_sym_pcg_cheb: CFS_HIP_ERR_ARG for a null pointer (first), u == b, u or b not 16-byte
 * aligned, tol < 0, maxiter < 0; CFS_HIP_ERR_UNSUPPORTED for a shard or a multi-device handle; then CFS_HIP_ERR_ARG
 * for a hierarchy of another handle, a host pointer or a pointer on another device.  In each case u is untouched and
 * *iterations = 0.                                                                                                */
int cfs_hip_sym_pcg_amg(cfs_hip_sym_t h, cfs_hip_amg_t a, void *u_dev, const void *b_dev, double tol, int maxiter,
                        int check_every, int *iterations, double *relres, void *stream);
/* PRECONDITIONED CG ON A BLOCK OF RIGHT-HAND SIDES: A U_c = B_c for the columns c < ncols <= CFS_HIP_LOBPCG_MAX_K, column c
 * of U at u_dev + c ld values and of B at b_dev + c ld values.  On entry U holds the first guesses, on return the
 * solutions; B, the rows from n on of every column and everything else of the caller's are not written.  block_rows: the
 * stored M^-1, as in the Chebyshev entry points -- 0 none (cfs_hip_sym_cg), 1 Jacobi (cfs_hip_sym_pcg), 2, 3, 4 or 6
 * block Jacobi (cfs_hip_sym_pcg_block).  Every column runs the recurrence of its one-column entry point and stops by
 * its rule, r_c.r_c <= tol^2 b_c.b_c, on its own: the set-up of M^-1 runs once per call, the products stay one per
 * column that is still active, and the dot, update and direction kernels run ONCE for the block, 2 k + 3 launches per
 * iteration with k active columns where k one-column solves enqueue 5 k.  The scalars, the iteration counter and the
 * convergence flag are per column and live on the device; a column whose flag is up is frozen by the kernels
 * themselves, so the host's looks (every check_every iterations, < 1 means 8, and never more iterations than keep
 * about 80 launches ahead of the GPU) decide nothing but when the loop ends.  A column with b_c = 0, one whose first
 * guess already solves it and one that holds a NaN never become active.  iterations[ncols], relres[ncols] (either may
 * be NULL): per column what the one-column entry point returns, relres RECOMPUTED from the returned U.  Returns 0 also
 * when some column reaches maxiter.  MEMORY: 3 blocks of (ncols - 1) ld + n values (R, P, Q) besides M^-1.  On a
 * CFS_HIP_FLAG_DETERMINISTIC handle column c of U, iterations[c] and relres[c] have the bits of the one-column entry
 * point on (u_c, b_c) alone.  CFS_HIP_CG_GRAPH has no effect here.  Refusals, all before U is touched and with every
 * iterations[c] = 0, in this order: CFS_HIP_ERR_ARG for a null pointer; ncols outside 1 .. CFS_HIP_LOBPCG_MAX_K; u_dev or
 * b_dev not 16-byte aligned; ld < n, or ncols > 1 and ld sizeof(V) not a multiple of 16; the two blocks overlap;
 * tol < 0, maxiter < 0 or a block_rows that is not one of 0, 1, 2, 3, 4, 6; CFS_HIP_ERR_UNSUPPORTED for a shard or a
 * multi-device handle; then CFS_HIP_ERR_ARG for a host pointer or one on another device, and for a diagonal entry or
 * block that is not positive (definite), which refuses the whole call.  Out of scope: Chebyshev, mixed-precision and
 * MINRES block forms, and a product that serves several columns in one pass over the matrix.                      */
int cfs_hip_sym_pcg_cols(cfs_hip_sym_t h, void *u_dev, const void *b_dev, long long ld, int ncols, int block_rows,
                         double tol, int maxiter, int check_every, int *iterations, double *relres, void *stream);
/* cfs_hip_sym_pcg_amg on a block of right-hand sides, the blocks, outputs and guarantee as for cfs_hip_sym_pcg_cols:
 * the cycle of `a` runs column-blocked on the columns still active (cfs_hip_amg_apply_cols: every vector kernel once
 * for the block) and so do the four kernels of the recurrence; every hierarchy cfs_hip_sym_pcg_amg serves is served.
 * The host looks after every iteration, check_every is accepted and not used.  cfs_hip_amg_column_cycles grows by
 * iterations[c] + 1 for every column that was ever active.  MEMORY: 4 blocks of (ncols - 1) ld + n values (R, P, Q,
 * Z) and the hierarchy's work vectors for ncols columns (kept, as by cfs_hip_amg_apply_cols).  Refusals as for
 * cfs_hip_sym_pcg_cols (no block_rows), with, behind CFS_HIP_ERR_UNSUPPORTED and in this order, CFS_HIP_ERR_ARG for a
 * hierarchy created on another handle, one whose last refresh failed, a host pointer or one on another device.    */
int cfs_hip_sym_pcg_amg_cols(cfs_hip_sym_t h, cfs_hip_amg_t a, void *u_dev, const void *b_dev, long long ld, int ncols,
                             double tol, int maxiter, int check_every, int *iterations, double *relres, void *stream);
/* Host only, no device work: one level of the set-up above.  In: the CSR of A_l (entries with col <= row are read),
 * passes (1 .. 3).  Out: agg[n], w[n] (fp64), *nc, and the lower triangle + diagonal CSR of A_{l+1} in fp64,
 * c_rowptr[*nc + 1] (at least n + 1 ints: *nc is not known before), c_colind / c_values with room for `capacity`
 * entries, *c_nnz the number written.  The coarse matrix never has more stored entries than the lower triangle +
 * diagonal of the input, so capacity = nnz always suffices; too little room: CFS_HIP_ERR_ARG with *c_nnz set to what
 * is needed.  A diagonal entry that is zero, missing, negative or not finite: CFS_HIP_ERR_ARG as above.           */
int cfs_hip_debug_amg_coarsen(int n, const int *rowptr, const int *colind, const double *values, int passes,
                              int *agg, double *w, int *nc, int *c_rowptr, int *c_colind, double *c_values,
                              long long capacity, long long *c_nnz);
/* The same with the locally dominant matching; rounds[passes]: the rounds every pass ran.                         */
int cfs_hip_debug_amg_coarsen_dominant(int n, const int *rowptr, const int *colind, const double *values, int passes,
                                       int *agg, double *w, int *nc, int *c_rowptr, int *c_colind, double *c_values,
                                       long long capacity, long long *c_nnz, int *rounds);
/* ---- the NODE-BLOCK form: aggregate mesh nodes, smooth with block Jacobi ------------------------------------------
 * For multi-dof mesh matrices (`block` consecutive rows are one node, as for cfs_hip_sym_pcg_block) whose couplings
 * inside a node are as strong as the diagonal and whose node frames are not the coordinate axes: there the scalar
 * hierarchy above -- scaled by 1 / sqrt(a_ii), matched row by row, smoothed by point Jacobi -- can be worse than none.
 * n must be a multiple of block; m = n / block nodes.  Per level, D_i the block x block diagonal block of A_l:
 *   W_i = D_i^-1/2, the SYMMETRIC inverse square root, from a cyclic Jacobi eigen-solve in fp64 (Q diag(1 / sqrt(ev)) Q^T,
 *   exactly symmetric).  The symmetric root keeps the node's frame; a Cholesky factor would not.
 *   B = W A_l W with W = blockdiag(W_i), a coupled pair of nodes stored as a full block.
 *   `passes` rounds of pairwise matching on the NODE graph with s_ij = ||B_ij||_F / sqrt(||B_ii||_F ||B_jj||_F) > 0, by
 *   the rule of `matching` (CFS_HIP_AMG_MATCHING_GREEDY or _DOMINANT) exactly as above, each followed by B <- Q^T B Q
 *   with Q = Q_node (x) I, the sums in the order of the scalar form.
 *   Coarse unknown I * block + c is component c of coarse node I: agg[i * block + c] = agg_node[i] * block + c,
 *   P_l = W Q_1 .. Q_p, A_{l+1} = the last B rounded to the value type -- again a node-block matrix.
 * The rules that end a hierarchy (coarse_max counts rows), the dense level and the level handles are those above.
 * THE CYCLE is the one above with M = blockdiag(A_l) on the node blocks in the smoother (the inverse blocks and the
 * power method of cfs_hip_sym_pcg_cheb with CFS_HIP_CHEB_BLOCK), rc_I = sum_{i in I} W_i (r_i - t_i) over the member
 * nodes ascending, z_i += W_i ec_I and d_i = (1 / theta) M_i^-1 (r_i - t_i): one thread per node, the same launch counts,
 * the same rounding rule, no atomics; M^-1 is symmetric because W_i is and restriction is the transpose of prolongation.
 * cfs_hip_sym_pcg_amg and cfs_hip_amg_apply take the object unchanged.  MEMORY: per level block (block + 1) / 2 words of
 * W and as many of M^-1 per node where the scalar form holds w and dinv; the aggregate lists hold nodes.
 * cfs_hip_amg_create_block_*: block = 1 IS cfs_hip_amg_create_* (greedy) or cfs_hip_amg_create_dominant_* (dominant),
 * bit for bit.  CFS_HIP_ERR_ARG, in this order and before anything else: a block outside 1, 2, 3, 4, 6; a matching that
 * is neither constant; an n that is not a multiple of block (a trailing partial node is not supported); then every
 * check of cfs_hip_amg_create_* in its words and order.  A node block of any level with an eigenvalue that is not
 * finite and > 0: CFS_HIP_ERR_ARG, "... needs positive definite node blocks, <count> of <nodes> blocks of <block> rows
 * ... (level <l>)".  The hierarchy is built on the host and is NOT refreshable: cfs_hip_amg_update_values_* returns
 * CFS_HIP_ERR_ARG as for any object of cfs_hip_amg_create_*.  There is no device set-up of this form.
 * cfs_hip_amg_block: *block = the rows per node of the hierarchy, 1 for every object of the entry points above.
 * cfs_hip_amg_level_node_weights (level < levels - 1, block > 1; otherwise CFS_HIP_ERR_ARG): W[m_l * block * block] in
 * the value type, node i's W_i row-major at W + i * block * block, as the device holds them (it keeps the lower
 * triangles, packed like the block-Jacobi inverse).  On a node-block hierarchy cfs_hip_amg_level_aggregates returns the
 * map of the unknowns in agg[n_l] and its w must be NULL (CFS_HIP_ERR_ARG otherwise).                              */
int cfs_hip_amg_create_block_f64(cfs_hip_sym_t h, int n, const int *rowptr, const int *colind, const double *values,
                                 int block, int matching, const cfs_hip_amg_options *opt, cfs_hip_amg_t *out);
int cfs_hip_amg_create_block_f32(cfs_hip_sym_t h, int n, const int *rowptr, const int *colind, const float *values,
                                 int block, int matching, const cfs_hip_amg_options *opt, cfs_hip_amg_t *out);
int cfs_hip_amg_block(cfs_hip_amg_t a, int *block);
int cfs_hip_amg_level_node_weights(cfs_hip_amg_t a, int level, void *W);
/* Host only, no device work: one level of the node-block set-up in fp64, the counterpart of cfs_hip_debug_amg_coarsen.
 * block = 1: that function (or cfs_hip_debug_amg_coarsen_dominant) itself, W = w[n].  Otherwise agg[n] is the map of the
 * unknowns, W[(n / block) * block * block] the full row-major W_i, and the coarse CSR is returned as there; a coupled
 * pair of nodes is a full block, so size `capacity` for block * block entries per pair of coupled nodes (too little
 * room: CFS_HIP_ERR_ARG with *c_nnz set).  rounds[passes] (may be NULL): the rounds of the dominant matching.
 * CFS_HIP_ERR_ARG: block, matching, a null argument, passes, n not a multiple of block, a node block that is not
 * positive definite (the message of create, level 0).                                                              */
int cfs_hip_debug_amg_coarsen_block(int n, const int *rowptr, const int *colind, const double *values, int block,
                                    int passes, int matching, int *agg, double *W, int *nc, int *c_rowptr, int *c_colind,
                                    double *c_values, long long capacity, long long *c_nnz, int *rounds);
/* Host only, no device work: one level of a REFRESH.  The lists are built from values_at_create by the code
 * cfs_hip_amg_create_refreshable_* uses (the matchings of that array, frozen), then evaluated for values_new -- the
 * same CSR pattern -- in a host loop that adds in the order the kernels add.  Out: w[n] (fp64) and the coarse values in
 * the pattern cfs_hip_debug_amg_coarsen returns for values_at_create, room for `capacity`, *c_nnz written (too little
 * room: CFS_HIP_ERR_ARG with *c_nnz set).  A diagonal of either array that is not positive: CFS_HIP_ERR_ARG.      */
int cfs_hip_debug_amg_recoarsen(int n, const int *rowptr, const int *colind, const double *values_at_create,
                                const double *values_new, int passes, double *w, double *c_values, long long capacity,
                                long long *c_nnz);
/* MINRES (Paige & Saunders) for (A - shift I) u = b: A symmetric, possibly INDEFINITE, or singular with a
 * consistent b -- saddle-point matrices (a zero diagonal block), shifted operators, mixed-sign diagonals, on
 * which the conjugate gradients above promise nothing (on [[0, K], [K, 0]] with b = [f; 0] their first p.q is
 * exactly 0 and u stays 0).  One Lanczos recurrence, no breakdown on a nonsingular matrix, and the norm of the
 * recurrence's residual never increases.  The launch layout is cfs_hip_sym_cg's: five launches per iteration
 * on `stream` -- the SpMV (two) and three fused vector kernels -- every scalar in device memory as fixed-order
 * partial sums in fp64, no host round trip inside the loop, so on a CFS_HIP_FLAG_DETERMINISTIC handle the solve
 * is bit-reproducible whatever check_every.  u_dev, b_dev, alignment, placement, check_every (<= 0: 8; at most
 * 16), *iterations and the handles accepted are those of cfs_hip_sym_cg (a shard: CFS_HIP_ERR_UNSUPPORTED).
 * precond: CFS_HIP_PRECOND_NONE, or CFS_HIP_PRECOND_JACOBI, which HERE means M = |diag(A) - shift| (MINRES
 * needs a positive definite M): dinv_i = (V)(1.0 / fabs((double)a_ii - shift)) is stored once in the value
 * type, gathered from the handle as for cfs_hip_sym_pcg (it follows cfs_hip_sym_update_values_* and works on a
 * handle from cfs_hip_sym_load); z = M^-1 r is formed in fp64 where it is needed and never stored.  An entry
 * whose |a_ii - shift| is zero or not finite (a diagonal that is not stored counts as a_ii = 0):
 * CFS_HIP_ERR_ARG ("nonzero diagonal"), u untouched, *iterations = 0.  Another `precond`: CFS_HIP_ERR_ARG.
 * STOPPING RULE: the recurrence's phibar, the M^-1-norm of its residual, against tol sqrt(b . M^-1 b); a NaN
 * ends the solve.  With CFS_HIP_PRECOND_NONE that is cfs_hip_sym_cg's rule, ||r|| <= tol ||b||.  With Jacobi it
 * is NOT: MINRES carries no unpreconditioned residual, so the solve stops on sqrt(r . M^-1 r) <= tol sqrt(b .
 * M^-1 b), and on a badly scaled matrix the two rules differ -- look at *relres.  A vanishing Lanczos beta (the
 * Krylov space is exhausted, u is exact) is a normal end.  *relres = ||b - (A - shift I) u|| / ||b||, RECOMPUTED
 * in fp64 from the returned u (the norm alone when b = 0).  CFS_HIP_CG_GRAPH is not consulted.
 * CFS_HIP_ERR_ARG, before any device work: a null pointer (checked first), an unknown precond, u == b, u or b
 * not 16-byte aligned, tol < 0, maxiter < 0, a shift that is not finite, a host pointer or a pointer on another
 * device.                                                                                       */
int cfs_hip_sym_minres(cfs_hip_sym_t h, void *u_dev, const void *b_dev, int precond, double shift,
                       double tol, int maxiter, int check_every,
                       int *iterations, double *relres, void *stream);
/* k eigenpairs of A at one end of the spectrum -- which = CFS_HIP_EIGS_LARGEST (largest algebraic), _SMALLEST
 * (smallest algebraic) or _MAGNITUDE (largest |lambda|) -- by thick-restart Lanczos (Wu & Simon) with full
 * re-orthogonalisation on a basis of ncv vectors resident on the device: lambda_max and lambda_min for condition
 * numbers, smoother step sizes and the shift of cfs_hip_sym_minres, without a host synchronisation per dot product.
 * Handles accepted are those of cfs_hip_sym_cg, one device or multi-device (the basis lives on the home device; a
 * shard: CFS_HIP_ERR_UNSUPPORTED); both value types; the basis is stored in the value type V, EVERY dot product
 * and scalar is fp64.  Step j of the recurrence, no contracted multiply-adds:
 *     v_1 = (V)(v0 / ||v0||)
 *     q = A v_j;  c = V_j^T q;  qq = q.q;  q1 = (V)(q - sum_k c_k v_k)  (fp64, k ascending, rounded once when stored)
 *     c' = V_j^T q1;  q2 = (V)(q1 - sum_k c'_k v_k);  alpha_j = c_j + c'_j;  beta_j = sqrt(q2.q2)
 *     breakdown iff !(beta_j > 16 u_V sqrt(qq))  (u_V = 2^-53 / 2^-24);  v_{j+1} = (V)(q2 / beta_j), or 0
 * Nine launches per step on `stream` (the SpMV's two and seven vector kernels), alpha, beta and the breakdown flag in
 * device memory, no host round trip inside a step or between steps: the host looks when the basis is full.  It then
 * solves the projected matrix (cyclic Jacobi in fp64, no LAPACK), and unless the k wanted pairs have converged --
 * estimate |beta_m s_{m,i}| <= tol max|theta| over the Ritz values of the current projected matrix -- keeps
 * l = k + (ncv - k) / 2 Ritz vectors, V[:, 0..l) <- V_m S on the device, and continues at step l + 1.  All sums are
 * fixed-order partial sums: on a CFS_HIP_FLAG_DETERMINISTIC handle the solve is bit-reproducible.  Device memory
 * held during the call: (ncv + 2) n values.
 * ncv = 0 means min(n, max(2 k + 1, 20)); otherwise 1 <= k < ncv <= min(n, CFS_HIP_EIGS_MAX_NCV).
 * v0_dev: the start vector, n values of the value type, 16-byte aligned, not modified.  NULL selects the fixed
 * vector v0_i = (double)(z_i >> 11) 2^-53 - 0.5 with z_i the splitmix64 finaliser of (i + 1) 0x9E3779B97F4A7C15
 * (z ^= z >> 30, z *= 0xBF58476D1CE4E5B9, z ^= z >> 27, z *= 0x94D049BB133111EB, z ^= z >> 31; 64-bit wrap-around),
 * a pure function of the row index i: the same bits in every call.
 * eigenvalues: host array of k doubles, ordered by `which` (descending, ascending, descending magnitude).
 * vectors_dev: column i at vectors_dev + i ld values; ld >= n, the pointer and ld sizeof(V) multiples of 16; nothing
 * outside rows [0, n) of the k columns is written; NULL for values only.  The columns have unit norm up to rounding.
 * residuals: nullable host array of k doubles, ||A x_i - theta_i x_i||_2 / ||x_i||_2 RECOMPUTED in fp64 from the
 * returned, stored x_i with k extra products (as *relres is elsewhere); with vectors_dev == NULL the Lanczos
 * estimates |beta_m s_{m,i}|.  *nconv: the number of leading pairs whose estimate met the tolerance; the call
 * returns 0 also when nconv < k after max_restarts restarts, all k pairs written, the unconverged ones as the
 * best available.  *restarts, *products: restarts made and SpMVs issued; any of the three counters may be NULL.
 * A breakdown at step j means "v0 lies in an invariant subspace of dimension j": the Ritz pairs of T_j are exact
 * there, the solve ends and returns min(k, j) pairs as converged (in *nconv), return code 0, the remaining
 * eigenvalues, residuals and columns zero-filled.
 * SCOPE: plain Lanczos finds the well-separated end of a spectrum quickly and the clustered low end of a stiffness
 * matrix slowly; shift-invert (an inner cfs_hip_sym_minres or _pcg solve per step) is left for a later change.
 * cfs_hip_sym_lobpcg below, which uses the preconditioners directly, is the route to the low end.
 * CFS_HIP_ERR_ARG, before any device work, in this order: a null h or eigenvalues ("null"); an unknown which; bad
 * k / ncv (the part against n once the handle is read); tol < 0 or NaN, max_restarts < 0; v0_dev or vectors_dev
 * not 16-byte aligned, or a bad ld; a host pointer or a pointer on another device.  A start vector whose norm is
 * zero or not finite: CFS_HIP_ERR_ARG ("start vector"), nothing written.                          */
#define CFS_HIP_EIGS_LARGEST   0  /* largest algebraic  */
#define CFS_HIP_EIGS_SMALLEST  1  /* smallest algebraic */
#define CFS_HIP_EIGS_MAGNITUDE 2  /* largest |lambda|   */
#define CFS_HIP_EIGS_MAX_NCV 128
int cfs_hip_sym_eigs(cfs_hip_sym_t h, int k, int which, int ncv, double tol, int max_restarts,
                     const void *v0_dev, double *eigenvalues, void *vectors_dev, long long ld,
                     double *residuals, int *nconv, int *restarts, int *products, void *stream);
/* For developers and tests: `steps` plain steps (no restart) of the recurrence above with the solver's own kernels.
 * basis_dev receives v_1 .. v_{done+1} (column i at basis_dev + i ld values; ld, alignment and placement as for
 * vectors_dev; steps + 1 columns of room), alpha[steps] and beta[steps] on the host (0 behind a breakdown),
 * *done = steps made up to and with a breakdown (column `done` is then 0).  1 <= steps <= CFS_HIP_EIGS_MAX_NCV.
 * v0_dev as above.  The call waits for the kernels.                                                */
int cfs_hip_sym_debug_lanczos(cfs_hip_sym_t h, const void *v0_dev, int steps, void *basis_dev, long long ld,
                              double *alpha, double *beta, int *done, void *stream);
/* host-only, no GPU: the small dense symmetric eigensolver the restart uses (cyclic Jacobi, fp64).  a: m x m
 * symmetric, row-major (the upper triangle is read), 1 <= m <= CFS_HIP_EIGS_MAX_NCV (else CFS_HIP_ERR_ARG);
 * w: the m eigenvalues ascending; s: m x m row-major, eigenvector i in column i.                   */
int cfs_hip_debug_symeig(int m, const double *a, double *w, double *s);
/* For developers and tests: the restart's V S alone, with the solver's own launch.  out[:, c] = (V)(sum_{k < m} basis[:, k]
 * s[k nout + c]) for c < nout, rows [0, n); fp64 accumulation, k ascending, rounded once when stored.  basis_dev: n x m
 * values of value_bytes 4 / 8, column k at basis_dev + k ld values; out_dev: column c at out_dev + c ldo values; s:
 * m x nout row-major on the host.  1 <= nout <= m <= CFS_HIP_EIGS_MAX_NCV, n >= 1, ld, ldo >= n; the pointers,
 * ld value_bytes and ldo value_bytes multiples of 16; device memory of the current device.  out_dev == basis_dev with
 * ldo == ld is the in-place restart; any other overlap of the two blocks (first byte to row n - 1 of the last column)
 * is refused.  WRITTEN: rows [0, n) of columns [0, nout) of out and nothing else -- not the rows [n, ldo), not a column
 * from nout on; in place, columns [nout, m) of the basis are read and left as they were.  The call waits for the
 * kernel.  CFS_HIP_ERR_ARG, before any device work, in this order: a null pointer ("null"); bad m / nout; value_bytes;
 * a pointer not 16-byte aligned; a bad n / ld / ldo; an overlap; memory that is not the current device's.           */
int cfs_hip_debug_eigs_combine(void *out_dev, long long ldo, const void *basis_dev, long long ld, long long n,
                               int m, int nout, const double *s, int value_bytes, void *stream);
/* The k SMALLEST (algebraic) eigenpairs of A by LOBPCG (Knyazev's locally optimal block preconditioned CG) with the
 * preconditioners of the PCG solvers: the first vibration or buckling modes of a stiffness matrix, the clustered low
 * end that cfs_hip_sym_eigs finds slowly.  k products per iteration, no factorisation.  Handles accepted are those
 * of cfs_hip_sym_cg, one device or multi-device (the blocks live on the home device; a shard:
 * CFS_HIP_ERR_UNSUPPORTED); both value types; the blocks are stored in the value type V, EVERY dot product and
 * scalar is fp64, no contracted multiply-adds.  1 <= k <= CFS_HIP_LOBPCG_MAX_K and 3 k <= n.
 * block_rows: 0 no preconditioner, 1 Jacobi, 2, 3, 4, 6 block Jacobi on the node blocks; M is built exactly as
 * cfs_hip_sym_pcg / cfs_hip_sym_pcg_block build theirs, and a diagonal entry or block that is not positive
 * (definite) is refused the same way (CFS_HIP_ERR_ARG, nothing written).  Block sizes above 1 on a multi-device
 * handle: CFS_HIP_ERR_UNSUPPORTED.
 * An iteration works on S = [X | W | P_act], m <= 3 k columns, and AS, the same columns of A S:
 *   1. G = S^T S and H = S^T AS, upper triangles, in ONE pass over S and AS: fixed-order partial sums per workgroup,
 *      added up by a second kernel; the host reads both matrices (first look).
 *   2. Rayleigh-Ritz on the host, fp64: d_j = G_jj^-1/2, a column whose G_jj is not finite and > 0 is dropped; the
 *      eigenvectors of D G D with w > 64 u_V w_max are kept (u_V = 2^-53 / 2^-24), Q = D U w^-1/2; T = Q^T H Q,
 *      symmetrised; C = Q Z[:, :k], theta = the k smallest eigenvalues of T.  (The drop makes a W or P column that
 *      is nearly dependent on the others harmless.)
 *   3. X <- (V)(S C), AX <- (V)(AS C), P <- (V)(S C'), AP <- (V)(AS C'), C' = C with its first k rows zeroed: in
 *      place, fp64 accumulation with the columns ascending, rounded once when stored.
 *   4. R_i = AX_i - theta_i X_i; the norms ||R_i||, ||X_i||; W_i = (V)(M^-1 R_i) in fp64 from the stored inverse
 *      diagonal or inverse blocks.  The host reads the norms (second look).  Soft locking: only the pairs with
 *      r_i = ||R_i|| / ||X_i|| > tol scale contribute their W and P columns to the next S; X always stays whole.
 *   5. When all k residuals pass, AX = A X is recomputed with k products and step 4 repeated; the solve ends only if
 *      they still pass, else it goes on with the fresh AX (the drift of the implicitly updated AX does not reach
 *      the caller).
 *   6. AW_i = A W_i, one product per active pair.
 * Iteration 0 is steps 1 - 4 on S = X0, AS by k products.  TWO host looks per iteration are inherent in this
 * design: C depends on G and H, the active set on the norms.  All sums are fixed-order partial sums: on a
 * CFS_HIP_FLAG_DETERMINISTIC handle the solve is bit-reproducible.  Device memory held during the call: (6 k + 1) n
 * values (S, AS and the inverse diagonal; the packed inverse blocks take (block_rows + 1) / 2 n instead of n) plus
 * the scalars (the partial sums of G and H: 2 (3 k)^2 x 512 doubles).
 * scale: finite and > 0, the caller's estimate of ||A||_2: pair i has converged when ||A x_i - theta_i x_i||_2 /
 * ||x_i||_2 <= tol scale -- the criterion of cfs_hip_sym_eigs with lambda_max made explicit, because LOBPCG never
 * sees the top of the spectrum.
 * x0_dev: k start columns, column c at x0_dev + c ld0 values, not modified; NULL selects x0[i, c] = v0_{i + c n} of
 * the fixed sequence documented at cfs_hip_sym_eigs: the same bits in every call.  A start block short of rank k has
 * its dependent columns replaced from that sequence.
 * vectors_dev (required): column i at vectors_dev + i ld values; ld, ld0 >= n, the pointers, ld sizeof(V) and
 * ld0 sizeof(V) multiples of 16; device memory on the handle's device; nothing outside rows [0, n) of the k columns is
 * written.  The columns have unit norm up to rounding.
 * eigenvalues: host array of k doubles, ascending.  residuals: nullable host array of k doubles, ||A x_i - theta_i
 * x_i||_2 / ||x_i||_2 in fp64 from the returned, stored x_i and a fresh product A x_i.  *nconv: the number of
 * leading pairs whose residual meets the tolerance; the call returns 0 also when nconv < k after maxiter
 * iterations, the best pairs written.  *iterations (iteration 0 not counted), *products (every SpMV issued): any of
 * the three counters may be NULL.
 * CFS_HIP_ERR_ARG, before any device work, in this order: a null h, eigenvalues or vectors_dev ("null"); bad k (the
 * part against n once the handle is read); an unknown block_rows; tol < 0 or NaN, scale not finite and > 0,
 * maxiter < 0 ("tolerance"); x0_dev or vectors_dev not 16-byte aligned, or a bad ld / ld0; a host pointer or a
 * pointer on another device.  On a refusal the counters are zeroed and nothing else is written.            */
#define CFS_HIP_LOBPCG_MAX_K 16
int cfs_hip_sym_lobpcg(cfs_hip_sym_t h, int k, int block_rows, double tol, double scale, int maxiter,
                       const void *x0_dev, long long ld0, double *eigenvalues, void *vectors_dev, long long ld,
                       double *residuals, int *nconv, int *iterations, int *products, void *stream);
/* For developers and tests.  host-only: step 2.  g, hh: m x m row-major, upper triangles read
 * (1 <= m <= 3 CFS_HIP_LOBPCG_MAX_K, 1 <= k <= min(m, CFS_HIP_LOBPCG_MAX_K)); drop: the threshold on w / w_max,
 * in [0, 1); out: theta[k], c[m x k] row-major, *rank = columns kept (with rank < k the trailing theta and columns
 * of c are 0).                                                                                            */
int cfs_hip_debug_lobpcg_rr(int m, const double *g, const double *hh, int k, double drop, double *theta, double *c, int *rank);
/* G = S^T S, H = S^T T of two n x m device blocks (value_bytes 4 / 8; column c at + c ld values; pointers and
 * ld value_bytes multiples of 16), full m x m row-major on the host, with the solver's Gram and reduce kernels
 * (every entry of H is summed; the lower triangle of G mirrors the upper).  The call waits for the kernels.   */
int cfs_hip_debug_gram(const void *s_dev, const void *t_dev, long long ld, long long n, int m, int value_bytes,
                       double *g, double *hh, void *stream);
/* iteration 0 and `iters` more iterations with the solver's own kernels, every pair active, no convergence test,
 * no confirm step: X, theta and the residual norms ||AX_i - theta_i X_i|| / ||X_i|| of the implicitly updated AX
 * after the last one (the sibling of cfs_hip_sym_debug_lanczos).  Arguments as for cfs_hip_sym_lobpcg.       */
int cfs_hip_sym_debug_lobpcg(cfs_hip_sym_t h, int k, int block_rows, const void *x0_dev, long long ld0, int iters,
                             double *theta, void *vectors_dev, long long ld, double *resnorms, void *stream);
/* cfs_hip_sym_lobpcg with W_i = M^-1 R_i formed by ONE column-blocked multigrid cycle of `a` per iteration
 * (cfs_hip_amg_apply_cols on the pairs still active) instead of a stored inverse diagonal.  Everything else of the
 * iteration is the same code: the Gram kernel, the Rayleigh-Ritz step, the update kernel, the stopping rule on
 * tol scale, soft locking, the confirm step, the rank rule for x0; all arguments as there.  Step 4 writes the raw
 * (V)R_i into the W-columns of AS, which are free until the products of step 6 rewrite them, and the cycle reads them
 * from there: device memory held is that of cfs_hip_sym_lobpcg without the inverse diagonal, 6 k n values, plus the
 * hierarchy's work vectors for k columns (cfs_hip_amg_apply_cols).  *products counts only the solver's own products,
 * as cfs_hip_sym_lobpcg does.  A cycle costs 2 + 2 (degree - 1) smoothing products per multigrid level and column
 * (one for the restriction and one for the restart, and degree - 1 in each Chebyshev chain), and degree - 1 on a
 * smoother-only level; the number of cycles is the difference of cfs_hip_amg_column_cycles across the call.  On a
 * CFS_HIP_FLAG_DETERMINISTIC handle the solve is bit-reproducible.
 * Refusals, nothing written but the counters zeroed: CFS_HIP_ERR_ARG for a null h, a, eigenvalues or vectors_dev
 * ("null"); then those of cfs_hip_sym_lobpcg from "bad k" on, in its order, with CFS_HIP_ERR_ARG for a value type of
 * `a` other than h's where the handle is first read (before a shard: CFS_HIP_ERR_UNSUPPORTED); then
 * CFS_HIP_ERR_UNSUPPORTED for a multi-device handle; then CFS_HIP_ERR_ARG for a hierarchy created on another handle,
 * and for one whose last refresh failed.                                                                       */
int cfs_hip_sym_lobpcg_amg(cfs_hip_sym_t h, cfs_hip_amg_t a, int k, double tol, double scale, int maxiter,
                           const void *x0_dev, long long ld0, double *eigenvalues, void *vectors_dev, long long ld,
                           double *residuals, int *nconv, int *iterations, int *products, void *stream);
/* the counterpart of cfs_hip_sym_debug_lobpcg: iteration 0 and `iters` more with the kernels of
 * cfs_hip_sym_lobpcg_amg, every pair active, no convergence test, no confirm step.  Arguments and refusals as there. */
int cfs_hip_sym_debug_lobpcg_amg(cfs_hip_sym_t h, cfs_hip_amg_t a, int k, const void *x0_dev, long long ld0, int iters,
                                 double *theta, void *vectors_dev, long long ld, double *resnorms, void *stream);
/* step 3 alone, on one n x 3 k device block (X | W | P): with S its first m columns (1 <= m <= 3 k) and c m x 2 k
 * row-major on the host, X <- (V)(S c[:, :k]) and P <- (V)(S c[:, k:]), in place.  The call waits for the kernel. */
int cfs_hip_debug_lobpcg_update(void *s_dev, long long ld, long long n, int k, int m, const double *c, int value_bytes,
                                void *stream);
/* The three kernels in the forms the solver launches them in, through the solver's own launch functions.  The blocks
 * are device memory of one device, column c at + c ld values; the pointers and ld value_bytes are multiples of 16.
 * Each call waits for its kernels.  CFS_HIP_ERR_ARG, before any device work, in this order: a null pointer ("null");
 * the sizes (k, m, then an idx[j] out of range, then full_h / with_p / block_rows / active); value_bytes; a pointer
 * not 16-byte aligned or a bad n / ld; an overlap; memory that is not device memory of one device.
 *
 * cfs_hip_debug_gram_cols: step 1 on the m listed columns (1 <= m <= 48): column j of S and of T is the physical
 * column idx[j], 0 <= idx[j] < 48, in any order; the columns that are not listed are not read.  g, hh: m x m row-major
 * on the host.  full_h = 0 is the solver's form: only the upper triangles of G and H are summed and the lower ones are
 * their mirror images, bit for bit; full_h = 1 sums every entry of H.  The order of summation depends on (n, m,
 * full_h) alone, not on idx.  cfs_hip_debug_gram is this call with idx[j] = j and full_h = 1.
 *
 * cfs_hip_debug_lobpcg_update_cols: step 3 on blocks of 3 k columns (X | W | P).  S = the m listed columns
 * (1 <= m <= 3 k, 0 <= idx[j] < 3 k) of s_dev; c: m x nout row-major on the host, nout = 2 k with with_p = 1 and k
 * with with_p = 0.  Column o < k <- (V)(S c[:, o]) and, with_p = 1, column 2 k + o <- (V)(S c[:, k + o]): for every
 * row acc = 0, then acc = acc + s_j c_jo for j = 0 .. m - 1 in fp64 with a separate multiply and add, rounded once.
 * In place: a listed column may be an output.  WRITTEN: rows [0, n) of the k columns of X and, with_p = 1, of ALL k
 * columns of P, listed or not; nothing else -- not W, not P with with_p = 0, not the rows [n, ld).  as_dev: NULL, or a
 * second block of the same shape that does not overlap the first; it gets the same c and idx in the same launch.
 * cfs_hip_debug_lobpcg_update is this call with idx[j] = j, with_p = 1 and as_dev = NULL.
 *
 * cfs_hip_sym_debug_lobpcg_residual: step 4 alone, after the solver's own preconditioner set-up for block_rows (0, 1,
 * 2, 3, 4, 6; a diagonal entry or a block that is not positive (definite) is refused with the words of
 * cfs_hip_sym_lobpcg, nothing written).  x_dev, ax_dev, w_dev: k columns each (1 <= k <= CFS_HIP_LOBPCG_MAX_K) of the
 * handle's value type on the handle's device, ld >= n; the columns of W overlap neither X nor AX.  theta: k host
 * doubles.  active: bit i set: W_i <- (V)(M^-1 (AX_i - theta_i X_i)), rows [0, n); a W_i whose bit is clear is not
 * touched; a bit from k on is refused.  sums: 2 k host doubles, sums[2 i] = R_i . R_i and sums[2 i + 1] = X_i . X_i
 * for EVERY pair, whatever the mask.  A shard, or block_rows >= 2 on a multi-device handle: CFS_HIP_ERR_UNSUPPORTED. */
int cfs_hip_debug_gram_cols(const void *s_dev, const void *t_dev, long long ld, long long n, int m, const int *idx,
                            int full_h, int value_bytes, double *g, double *hh, void *stream);
int cfs_hip_debug_lobpcg_update_cols(void *s_dev, void *as_dev, long long ld, long long n, int k, int m, const int *idx,
                                     int with_p, const double *c, int value_bytes, void *stream);
int cfs_hip_sym_debug_lobpcg_residual(cfs_hip_sym_t h, int block_rows, const void *x_dev, const void *ax_dev, void *w_dev,
                                      long long ld, int k, const double *theta, unsigned active, double *sums,
                                      void *stream);
/* LOBPCG for the GENERALIZED problem A x = lambda B x: the k <= CFS_HIP_LOBPCG_MAX_K SMALLEST eigenpairs of the pencil
 * (A, B) -- K x = lambda M x with a mass matrix (vibration), K x = lambda K_g x with a definite geometric stiffness
 * (buckling).  A (the handle h) is symmetric; B is symmetric POSITIVE DEFINITE and held by a handle of its own, hb, with
 * h's n, value type and device.  hb == h is allowed (every theta is 1); a diagonal (lumped) B is a handle like any other.
 * No factorisation of B: B enters by products only, which keeps its sparsity.
 * This is the iteration of cfs_hip_sym_lobpcg -- the same templates, a compile-time switch and a third block -- on THREE
 * resident blocks of 3 k columns, S = [X | W | P], AS = A S and BS = B S, all in the value type V, every dot product and
 * scalar fp64, no contracted multiply-adds:
 *   1. G = S^T (BS) and H = S^T (AS), upper triangles, in ONE pass over the three blocks: the Gram kernel stages rows
 *      of all 3 m columns and a G task takes its second operand from the BS part of the row; the same 4 x 4 register
 *      blocks, task table, fixed-order slice and workgroup sums as cfs_hip_sym_lobpcg.  First host look.
 *   2. Rayleigh-Ritz on the host, unchanged: it already solves the pencil (H, G).  A column whose G_jj = s_j^T B s_j is
 *      not finite and > 0 is dropped.
 *   3. X <- (V)(S C), P <- (V)(S C'), AX, AP and BX <- (V)(BS C), BP <- (V)(BS C') in ONE launch, with the order and
 *      the rounding of step 3 of cfs_hip_sym_lobpcg for each of the three blocks: BX is carried along implicitly like AX.
 *   4. R_i = AX_i - theta_i BX_i in fp64 from the stored values; the sums R_i . R_i and X_i . X_i; W_i = (V)(M^-1 R_i)
 *      with M built from A exactly as cfs_hip_sym_lobpcg builds it (block_rows 0, 1, 2, 3, 4, 6), or by one column-
 *      blocked multigrid cycle of `a`, a hierarchy of A, on the raw R_i (cfs_hip_sym_lobpcg_gen_amg).  Second host look.
 *      Pair i has converged when ||A x_i - theta_i B x_i||_2 / ||x_i||_2 <= tol scale; scale: the caller's estimate of
 *      ||A||_2, as there.  Soft locking as there.
 *   5. When all k residuals pass, AX = A X and BX = B X are both recomputed (2 k products) and step 4 repeated.
 *   6. AW_i = A W_i and BW_i = B W_i for the active pairs.
 * Iteration 0 is steps 1 - 4 on S = X0 with k products of each matrix.  *products counts the products with A,
 * *b_products those with B (both nullable, as are nconv and iterations).  Device memory held during the call:
 * (9 k + 1) n values (without the inverse diagonal for block_rows 0 and the multigrid form) plus the scalars.
 * The returned columns are B-ORTHONORMAL, X^T B X = I up to rounding (not of unit 2-norm).  eigenvalues ascending.
 * residuals: ||A x_i - theta_i B x_i||_2 / ||x_i||_2 in fp64 from the returned, stored x_i and FRESH products with both
 * matrices.  All other arguments as for cfs_hip_sym_lobpcg.  The solve is bit-reproducible when both handles are
 * CFS_HIP_FLAG_DETERMINISTIC.
 * Refusals, nothing written and the counters zeroed, in this order: those of cfs_hip_sym_lobpcg (of _lobpcg_amg for the
 * multigrid form) with hb among the null checks; where the handles are first read, CFS_HIP_ERR_ARG for an hb whose n or
 * value type differs from h's or which lives on another device; CFS_HIP_ERR_UNSUPPORTED for a shard or a multi-device
 * handle on either side; then the remaining checks of cfs_hip_sym_lobpcg.  A start block that still has rank < k in
 * the B inner product after the two refills: CFS_HIP_ERR_ARG, "B may not be positive definite" (with B = -I every G_jj
 * is negative and this is what fires).  An indefinite B is out of scope.
 * cfs_hip_sym_debug_lobpcg_gen: the counterpart of cfs_hip_sym_debug_lobpcg, resnorms = ||AX_i - theta_i BX_i|| /
 * ||X_i|| of the implicitly updated blocks.                                                                      */
int cfs_hip_sym_lobpcg_gen(cfs_hip_sym_t h, cfs_hip_sym_t hb, int k, int block_rows, double tol, double scale,
                           int maxiter, const void *x0_dev, long long ld0, double *eigenvalues, void *vectors_dev,
                           long long ld, double *residuals, int *nconv, int *iterations, int *products,
                           int *b_products, void *stream);
int cfs_hip_sym_lobpcg_gen_amg(cfs_hip_sym_t h, cfs_hip_sym_t hb, cfs_hip_amg_t a, int k, double tol, double scale,
                               int maxiter, const void *x0_dev, long long ld0, double *eigenvalues, void *vectors_dev,
                               long long ld, double *residuals, int *nconv, int *iterations, int *products,
                               int *b_products, void *stream);
int cfs_hip_sym_debug_lobpcg_gen(cfs_hip_sym_t h, cfs_hip_sym_t hb, int k, int block_rows, const void *x0_dev,
                                 long long ld0, int iters, double *theta, void *vectors_dev, long long ld,
                                 double *resnorms, void *stream);
/* The three kernels in the forms the pencil solver launches them in; arguments, checks and their order as for the
 * two-block forms above, with the third block among the null, geometry, overlap and device checks.
 * cfs_hip_debug_gram3_cols: G = S^T BS and H = S^T AS on the m listed columns of three n x 48 blocks, the solver's
 * form (upper triangles summed, the lower ones their mirror images).
 * cfs_hip_debug_lobpcg_update3_cols: step 3 on three blocks of 3 k columns in one launch, the same c and idx for each.
 * cfs_hip_sym_debug_lobpcg_residual_gen: step 4 with R_i = AX_i - theta_i BX_i; sums[2 i + 1] is still X_i . X_i;
 * the columns of W overlap none of X, AX, BX.                                                                    */
int cfs_hip_debug_gram3_cols(const void *s_dev, const void *as_dev, const void *bs_dev, long long ld, long long n, int m,
                             const int *idx, int value_bytes, double *g, double *hh, void *stream);
int cfs_hip_debug_lobpcg_update3_cols(void *s_dev, void *as_dev, void *bs_dev, long long ld, long long n, int k, int m,
                                      const int *idx, int with_p, const double *c, int value_bytes, void *stream);
int cfs_hip_sym_debug_lobpcg_residual_gen(cfs_hip_sym_t h, int block_rows, const void *x_dev, const void *ax_dev,
                                          const void *bx_dev, void *w_dev, long long ld, int k, const double *theta,
                                          unsigned active, double *sums, void *stream);

/* ---- sharded operation: y_block = local rows; contributions to rows owned
 *      by lower ranks are packed into send_buf (device), exchanged by the
 *      caller (RCCL all-to-all / reduce-scatter), and folded in by
 *      cfs_hip_sym_recv_fold.                                                */
/* send_counts[r] = number of packed values destined to rank r (0 for r>=rank) */
int cfs_hip_sym_shard_send_counts(cfs_hip_sym_t h, int *send_counts);
/* global row index of every packed value, in send order (host array)        */
int cfs_hip_sym_shard_send_rows(cfs_hip_sym_t h, int *rows);
/* describe what this rank will receive: recv_rows are global row indices in
 * receive-buffer order (concatenated by source rank), host array            */
int cfs_hip_sym_shard_set_recv(cfs_hip_sym_t h, int nrecv, const int *recv_rows);
int cfs_hip_sym_spmv_local_async(cfs_hip_sym_t h, void *y_block_dev,
                                 const void *x_dev, void *send_buf_dev,
                                 void *stream);
int cfs_hip_sym_recv_fold_async(cfs_hip_sym_t h, void *y_block_dev,
                                const void *recv_buf_dev, void *stream);
/* The SpMV of a handle is two launches -- the tile kernel (streams the matrix;
 * the roofline kernel) and the halo fold -- plus, for a shard, the pack of the
 * contributions to lower ranks.  This entry point enqueues only the selected
 * ones (in the order tiles, pack, fold) so that bench.py can bracket the tile
 * kernel with HIP events and a shard can start its exchange before the local
 * fold; CFS_HIP_PHASE_ALL is a full local SpMV.                               */
#define CFS_HIP_PHASE_TILES 1
#define CFS_HIP_PHASE_FOLD 2
#define CFS_HIP_PHASE_PACK 4
#define CFS_HIP_PHASE_ALL 7
int cfs_hip_sym_spmv_phases_async(cfs_hip_sym_t h, void *y_block_dev,
                                  const void *x_dev, void *send_buf_dev,
                                  int phases, void *stream);

/* ---- native exchange between the row blocks of one process's devices: the north-star's
 *      reduce-scatter over xGMI, and the y -> x all-gather of a solver loop, without Python.
 *      (The reference has no exchange beyond its barrier between colours,
 *      csr_matrix.tpp:3018; what crosses a block boundary here are its direct conflicts,
 *      :1443-1451.)  Transports: RCCL (one communicator per device, ncclCommInitAll;
 *      librccl.so is loaded at the first use, the library does not link against it) and PEER
 *      (plain kernels / copies over peer access: what several ranks on ONE device -- the
 *      test boxes -- use, RCCL refusing two ranks per device; also the fall-back when RCCL
 *      cannot be loaded).  AUTO = RCCL when the devices are distinct and it loads.
 *      NOTE: what has run on hardware is the PEER transport with 2 / 3 / 4 / 8 ranks sharing one
 *      device and the RCCL transport with ONE rank (tests/test_gpu_comm.py, test_gpu_comm_edges.py,
 *      test_gpu_sparse_exchange.py).  With more than one rank the RCCL transport has not run on
 *      hardware yet, nor has the PEER transport between two physical devices.
 *
 *      Buffers and streams, all three collectives (pinned by tests/test_gpu_comm_edges.py):
 *      - a call is enqueued on streams[0..ndev-1] and returns at once; the host arrays it is given
 *        (send, recv, streams, counts) are read before it returns and may be reused or freed then;
 *      - rank g's part runs behind what is on streams[g] at the call: what g enqueued there before --
 *        writing its send buffer, reading its receive buffer of an earlier round -- is ordered before
 *        this call's reads of send[g] AND before its writes to recv[g], whichever rank's stream does
 *        them; work enqueued on streams[g] after the call sees recv[g] complete;
 *      - a send buffer is read by OTHER ranks' streams (PEER reduce-scatter and all-to-all): before
 *        rank g overwrites send[g], cfs_hip_comm_wait_consumed(c, g, streams[g]).  The all-gather
 *        reads send[g] on streams[g] itself and needs no such call.                            */
typedef struct cfs_hip_comm_s *cfs_hip_comm_t;
#define CFS_HIP_TRANSPORT_AUTO 0
#define CFS_HIP_TRANSPORT_RCCL 1
#define CFS_HIP_TRANSPORT_PEER 2
/* ranks 0..ndev-1 on devices[] (NULL: the visible devices round-robin from the current one) */
int cfs_hip_comm_create(int ndev, const int *devices, int transport, cfs_hip_comm_t *out);
int cfs_hip_comm_info(cfs_hip_comm_t c, int *ndev, int *transport);
int cfs_hip_comm_destroy(cfs_hip_comm_t c);
/* sum-reduce-scatter: rank g contributes send[g] (ndev * count values, on its device) and
 * receives the g-th block of the sum in recv[g] (count values); enqueued on streams[g], returns at
 * once; the tables are read before it returns (PEER: they go to the sum kernels by value).  PEER
 * adds in rank order from 0: the sum is the same bits in every call.  count = 0 moves nothing.  */
int cfs_hip_comm_reduce_scatter(cfs_hip_comm_t c, void *const *send, void *const *recv, size_t count,
                                int value_bytes, void *const *streams);
/* all-gather: recv[g] (ndev * count values) = the blocks send[0..ndev-1] (count values each);
 * enqueued on streams[g], returns at once.  PEER: rank g pushes its block into every recv[r] on
 * streams[g], behind an event recorded on streams[r] at entry -- so a rank that is still reading
 * recv[r] of the round before, on its own stream, is not overtaken.                          */
int cfs_hip_comm_allgather(cfs_hip_comm_t c, void *const *send, void *const *recv, size_t count,
                           int value_bytes, void *const *streams);
/* packed all-to-all (the sparse form of the reduce-scatter): counts is a HOST array of ndev * ndev
 * entries, counts[g * ndev + r] = values rank g hands to rank r.  send[g] holds rank g's blocks for
 * r = 0..ndev-1 back to back (the order of cfs_hip_sym_shard_send_counts / the pack), recv[r] the
 * blocks from g = 0..ndev-1 back to back (the "concatenated by source rank" order of
 * cfs_hip_sym_shard_set_recv).  Zero counts and self blocks (g = r) are legal; a rank that sends
 * (receives) nothing may pass NULL for its send (receive) buffer.  Enqueued on streams[g], returns
 * at once; counts is read before the call returns.  PEER: one pull kernel per receiving rank; RCCL:
 * ncclSend / ncclRecv in one group (a librccl.so without them: CFS_HIP_ERR_UNSUPPORTED).  value_bytes
 * other than 4 or 8, a null argument or a negative count: CFS_HIP_ERR_ARG.                  */
int cfs_hip_comm_alltoallv(cfs_hip_comm_t c, void *const *send, void *const *recv, const int64_t *counts,
                           int value_bytes, void *const *streams);
/* before rank `rank` overwrites its send buffer on `stream`: wait until the previous
 * collective has consumed it (PEER transport: other ranks' kernels read it)                */
int cfs_hip_comm_wait_consumed(cfs_hip_comm_t c, int rank, void *stream);

/* ---- introspection (A->nnz(), A->size(), and what bench.py needs) --------- */
typedef struct {
  int n;               /* matrix order                                    */
  int row_begin, row_end; /* rows owned by this handle                    */
  int value_bytes;     /* 8 or 4                                          */
  int64_t nnz_low;     /* stored strict-lower nonzeros of the owned rows  */
  int64_t nnz_diag;    /* stored diagonal entries                         */
  int64_t nnz_full;    /* expanded count = what A->nnz() reports          */
  int ntiles, nslices, max_slots_used, block_threads;
  int64_t halo_slots;  /* sum over tiles of halo (non-own) slots          */
  int64_t fold_rows;   /* destination rows touched by the halo fold       */
  int64_t remote_vals; /* packed values sent to lower ranks (shards)      */
  int64_t lds_bytes;   /* dynamic LDS per workgroup                       */
  /* algorithmic bytes of one SpMV over the owned rows, SURVEY.md 8(d):
   * nnz_low*(4+s) + rows*(4+3s)                                          */
  int64_t bytes_algorithmic;
  /* bytes the device format actually streams per SpMV (values + 16-bit
   * slots + per-row metadata + x/y + halo strips + fold index)           */
  int64_t bytes_streamed;
  int64_t device_bytes; /* device memory held by the handle               */
  int64_t mirror_entries; /* one-sided entries a mirrored shard stores for rows of
                             higher ranks (0 for a whole matrix / exchange form)  */
  int64_t far_entries; /* HYB: nonzeros kept outside the tile format (each stored twice) */
  int ngroups;         /* persistent workgroups of a launch                          */
  int reserved_;
} cfs_hip_sym_stats;
int cfs_hip_sym_get_stats(cfs_hip_sym_t h, cfs_hip_sym_stats *out);
/* developer diagnostic: one extra launch of the tile kernel that records, per
 * persistent workgroup (in blockIdx order), 8 words of 100 MHz wall-clock
 * stamps: [0] start, [1] first x window ready (after the barrier), [2] slices
 * of the last tile done, [3] end, [4] first tile descriptor loaded, [5] slot
 * table of the first tile arrived (thread 0), [6] its x values arrived
 * (thread 0), [7] wave 0 finished its last slice.  Not used by any product
 * path; tools/timeline.py reads it.                                          */
int cfs_hip_sym_debug_timeline(cfs_hip_sym_t h, void *y_dev, const void *x_dev,
                               unsigned long long *stamps, int capacity_words,
                               int *ngroups);

/* developer diagnostic: what the group in every launch slot (block b runs slot
 * (b % 8) * (ngroups / 8) + b / 8) has to do, CFS_HIP_GROUP_FEATURES words
 * each: [0] tiles, [1] rows, [2] virtual rows, [3] slices, [4] packet rounds (sum
 * over slices of the longest lane's packets), [5] value-stream entries, [6] slot-
 * stream entries, [7] COO leftovers, [8] halo slots, [9] slots.  tools/ fit the
 * cost model of the row cut against the timeline with it.                      */
#define CFS_HIP_GROUP_FEATURES 10
int cfs_hip_sym_debug_group_features(cfs_hip_sym_t h, long long *out, int capacity_words,
                                     int *ngroups);

/* developer / test: 64-bit FNV-1a digests of the device arrays of a handle's schedule, over
 * their logical lengths, in this order: tiles (aexp masked), launch-slot first tiles, launch-
 * slot tile ranges, slot_col, rowinfo, diag, slice_meta, leadlane, vals, slots, cvals, crows,
 * ccols, fold records, fold remainder lists, val_map, cval_map, diag_map, window / launch shape,
 * slot exponents (deterministic build), send_ptr, send_idx (exchange-form shard), the far sections
 * (fvals, frows, fcols, fval_map, count) -- 0 when absent.  A
 * schedule built on the GPU and one built by the host builder for the same matrix and options
 * have equal digests.  words[CFS_HIP_DIGEST_WORDS - 1] = 1 if the handle's schedule was built
 * on the GPU.                                                                           */
#define CFS_HIP_DIGEST_WORDS 28
int cfs_hip_sym_debug_digest(cfs_hip_sym_t h, unsigned long long *words, int capacity_words);
/* developer / test: the instantiation of the tile kernel this handle launches,
 * cfs_sym_tile_kernel<V, BLOCK, MODE, NT, OFFB, U, DET, COMB>, as CFS_HIP_KERNEL_WORDS ints:
 * [0] value bytes (8 / 4), [1] BLOCK (256, 512, 1024), [2] MODE (0 = product, 1-4 = the
 * timing-only ablations), [3] NT (non-temporal stream loads), [4] OFFB (mirrored shard:
 * one-sided slots), [5] U (3, 6 or 10 slots a thread), [6] DET (fixed-point sums), [7] COMB
 * (sibling-combined atomics; 1 for every deterministic handle).  The launch reads the same
 * choice.  A multi-device handle returns CFS_HIP_ERR_ARG.                                  */
#define CFS_HIP_KERNEL_WORDS 8
int cfs_hip_sym_debug_kernel(cfs_hip_sym_t h, int *words, int capacity_words);
/* developer / test: the lists cfs_fold_kernel walks, decoded from the DEVICE arrays (records and remainder
 * lists are copied back, so a device-built and a host-built schedule both report what the launch reads):
 * which = 0 the local halo fold, 1 the receive fold; dst[i] = local row, len[i] = entries of its list,
 * in record order (record i is read by thread i of the launch).  *count = number of lists; more than
 * `capacity` of them, or a multi-device handle, returns CFS_HIP_ERR_ARG (*count is set first).        */
int cfs_hip_sym_debug_fold_lists(cfs_hip_sym_t h, int which, int *dst, int *len, int capacity, int *count);
/* why the device builder handed this handle's schedule to the host builder ("" = it built it) */
int cfs_hip_sym_debug_plan_note(cfs_hip_sym_t h, char *buf, int capacity);

/* ---- host-only self-check of the tile schedule (needs no GPU): builds the
 *      schedule tune() would upload, decodes it back to (row, col, value)
 *      triples and compares them with the strict lower triangle of the input;
 *      also checks that the halo-fold index covers every strip entry once.
 *      Structure only -- no SpMV arithmetic is performed on the host.      ---- */
typedef struct {
  int ntiles, ngroups, lds_slots;
  int64_t nslices, halo_slots, stream_len, nnz_low, fold_rows, remote_vals;
  int64_t decoded;    /* triples recovered from the device format           */
  int64_t mismatches; /* 0 = the schedule encodes exactly the input         */
  int64_t mirror_entries; /* mirrored off-block entries (shards, default form)  */
  int64_t far_entries;    /* HYB: nonzeros outside the tile format (mirror images checked) */
} cfs_hip_plan_report;
int cfs_hip_sym_plan_check_f64(int n, const int *rowptr, const int *colind,
                               const double *values, int nranks, int rank,
                               const int *row_splits, const cfs_hip_options *opt,
                               cfs_hip_plan_report *report);
int cfs_hip_sym_plan_check_f32(int n, const int *rowptr, const int *colind,
                               const float *values, int nranks, int rank,
                               const int *row_splits, const cfs_hip_options *opt,
                               cfs_hip_plan_report *report);

/* ---- plan files: a tuned symmetric handle saved to a file and loaded back without tune()
 *      (cfs_spmv_amd/csrc/cfs_planfile.hpp is the format: little-endian, self-describing, one
 *      64-bit checksum per section).  One file holds one handle: a plain one or one shard of
 *      either form; the value type, the struct layouts of this library version and the LDS
 *      window must fit where it is loaded.  A file whose checksums pass is trusted input:
 *      the cache is not a security boundary.
 *
 * save: waits for the handle's device, has a device kernel compute every section's checksum
 * from the DEVICE arrays, copies them back through page-locked blocks and writes
 * path + ".tmp", renamed to `path` once complete.  The handle is unchanged.  `tag`: an opaque
 * string of at most 255 bytes, stored verbatim (NULL = ""); a caller's key for "is this file
 * still the schedule of my matrix".  A multi-device handle: CFS_HIP_ERR_UNSUPPORTED.
 *
 * load: validates the header and the section table on the host (before anything is allocated
 * from a size of the file), uploads the arrays to the CURRENT device through two page-locked
 * blocks, has the checksum kernel verify every uploaded array, and only then sets the handle up.
 * A non-NULL expected_tag must equal the stored tag.  CFS_HIP_ERR_FILE for anything wrong with
 * the file, CFS_HIP_ERR_UNSUPPORTED when the stored LDS window does not fit this device; on any
 * failure *out = NULL and nothing stays allocated.  The loaded handle is a full handle: it
 * launches the schedule and the kernel choices (window shape, HYB, sibling-combined or plain
 * kernel, stream-load policy) that the saved one had kept -- the developer knobs CFS_HIP_NT and
 * CFS_HIP_COMBINE still override, as at create -- and has the same stats, digests and
 * update_values behaviour; the owner of a shard calls cfs_hip_sym_shard_set_recv again.  The
 * timing-only ablation mode is not stored.                                                    */
int cfs_hip_sym_save(cfs_hip_sym_t h, const char *path, const char *tag);
int cfs_hip_sym_load(const char *path, const char *expected_tag, cfs_hip_sym_t *out);

/* host-only (no GPU): the validator -- magic, version and struct sizes; the file size against
 * the section table; every section length against the header's counts; the checksums -- and
 * what the header says.                                                                       */
typedef struct {
  int format_version, value_bytes;
  int n, row_begin, row_end, nranks, rank;
  int flags; /* cfs_hip_options.flags the schedule was built with (ablation bits cleared) */
  int ntiles, ngroups, block_threads, lds_slots;
  int has_value_map, deterministic, device_built;
  int nsections;
  int64_t nnz_low, nslices, halo_slots, stream_len, fold_rows, remote_vals, mirror_entries, far_entries;
  int64_t payload_bytes, file_bytes;
  char tag[256];
} cfs_hip_plan_file_info;
int cfs_hip_plan_file_check(const char *path, cfs_hip_plan_file_info *info);
/* developer / test: the checksum of cfs_planfile.hpp over [p, p + bytes): on_device = 1, p is a
 * 16-byte aligned device pointer and the kernel that save and load use computes it (enqueued on
 * the null stream, complete on return); on_device = 0, p is a host pointer and the host function
 * does.  The two agree bit for bit for every length.                                           */
int cfs_hip_debug_checksum(const void *p, size_t bytes, int on_device, unsigned long long *out);
/* host-only: build the schedule with the host builder exactly as cfs_hip_sym_plan_check_* does
 * and write it as a plan file (checksums in their host form): a file can be produced and
 * inspected on a machine without a GPU and loaded on one.  The launch shape is sized for the
 * default device (256 CUs, estimated residency), so the file need not equal a GPU-made one
 * byte for byte.                                                                              */
int cfs_hip_sym_plan_save_f64(int n, const int *rowptr, const int *colind,
                              const double *values, int nranks, int rank,
                              const int *row_splits, const cfs_hip_options *opt,
                              const char *path, const char *tag);
int cfs_hip_sym_plan_save_f32(int n, const int *rowptr, const int *colind,
                              const float *values, int nranks, int rank,
                              const int *row_splits, const cfs_hip_options *opt,
                              const char *path, const char *tag);

/* host-only: the send side of rank `rank`'s shard (what cfs_hip_sym_shard_send_
 * counts / _rows would return) without touching a device; used by the CPU
 * (gloo) tests of the exchange.  rows may be NULL to query *nrows_out.        */
int cfs_hip_sym_plan_send_info_f64(int n, const int *rowptr, const int *colind,
                                   const double *values, int nranks, int rank,
                                   const int *row_splits, const cfs_hip_options *opt,
                                   int *send_counts, int *rows, int rows_cap,
                                   int *nrows_out);

/* ---- general CSR (replaces cpu_mv / cpu_mv_serial, csr_matrix.tpp:2664-2704:
 *      Format::csr and the silent fall-back for non-symmetric files,
 *      csr_matrix.tpp:13-19)                                              ---- */
int cfs_hip_csr_create_f64(int nrows, int ncols, const int *rowptr,
                           const int *colind, const double *values,
                           cfs_hip_csr_t *out);
int cfs_hip_csr_create_f32(int nrows, int ncols, const int *rowptr,
                           const int *colind, const float *values,
                           cfs_hip_csr_t *out);
int cfs_hip_csr_spmv(cfs_hip_csr_t h, void *y, const void *x);
int cfs_hip_csr_spmv_async(cfs_hip_csr_t h, void *y_dev, const void *x_dev,
                           void *stream);
int cfs_hip_csr_destroy(cfs_hip_csr_t h);
/* The general CSR kernel exists in two forms -- a workgroup per block of rows (products staged
 * in LDS between two barriers) and a wave per chunk of rows (no workgroup barrier, the next
 * chunk's loads in flight) -- within a few per cent of each other, the order depending on the
 * matrix and the box: the FIRST SpMV of a handle with >= 1M nonzeros times five SpMVs of each
 * (y is fully overwritten by either) and keeps the faster.  CFS_HIP_CSR_KERNEL=block|wave
 * pins the form.                                                                        */
#define CFS_HIP_CSR_FORM_BLOCK 0
#define CFS_HIP_CSR_FORM_WAVE 1
int cfs_hip_csr_kernel_form(cfs_hip_csr_t h, int *form, int *measured);
/* The block form reads 16-bit column codes (2 bytes per nonzero instead of 4) in every row
 * block whose columns fit into four windows of 16 384 columns (window << 14 | offset; banded
 * matrices, 3-D stencils; written once, on the device, when the handle is created;
 * CFS_HIP_CSR_COL16=0: never); the codes -- or, for a block that needs more windows, its 32-bit
 * columns -- and a copy of the block's values are stored in the order the lanes consume them; and
 * both forms hand the k-th eighth of the matrix to XCD k (CFS_HIP_CSR_XCD=0: round robin).
 * bytes_streamed = bytes one SpMV of the kept form reads from the handle's arrays;
 * narrow_nnz = nonzeros stored with 16-bit columns.                                          */
int cfs_hip_csr_stats(cfs_hip_csr_t h, int64_t *bytes_streamed, int64_t *narrow_nnz);
/* developer / test: how this handle was cut, as CFS_HIP_CSR_LAYOUT_WORDS words: [0] row blocks (at
 * most 4 096 nonzeros and 1 024 rows each, a longer row alone); of these [1] stored with 16-bit
 * column codes, [2] in lane order with 32-bit columns, [3] read in natural order through the
 * product branch, [4] one long row (more than 4 096 nonzeros), [5] empty rows only -- [1]..[5]
 * partition [0], decoded from the DEVICE array of window starts copied back, so they report what
 * the launch reads (no such array, or single-entry loads: every block that is neither a long row
 * nor empty counts under [3]); [6] chunk descriptors of the wave form, padding included, [7]
 * descriptors with at least one row, [8] long rows of the wave form (more than 1 024 nonzeros);
 * [9] / [10] workgroups of a block-form / wave-form launch (0: nothing to launch); [11] entries a
 * lane loads at once (1 or 2, CFS_HIP_CSR_WIDE); [12] 1 if the XCD map is on.  Fewer than
 * CFS_HIP_CSR_LAYOUT_WORDS words of capacity is CFS_HIP_ERR_ARG.                              */
#define CFS_HIP_CSR_LAYOUT_WORDS 13
int cfs_hip_csr_debug_layout(cfs_hip_csr_t h, long long *words, int capacity_words);

/* ---- HIP-event timing on the stream the kernels run on (bench.py) --------- */
int cfs_hip_event_create(void **ev);
int cfs_hip_event_record(void *ev, void *stream);
int cfs_hip_event_elapsed_ms(void *start, void *stop, float *ms); /* syncs stop */
int cfs_hip_event_destroy(void *ev);

#ifdef __cplusplus
}
#endif
#endif /* CFS_HIP_H */
