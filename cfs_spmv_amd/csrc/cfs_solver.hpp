// cfs_solver.hpp -- a solver-style caller of the SpMV path behind the C ABI: conjugate
// gradients on resident vectors.
//
// The reference has no counterpart: its only callers are a benchmark loop and a
// self-check with a fixed x (bench/bench_spmv_mmf.cpp:139-173, test/test_spmv_mmf.cpp:71-109).
// A solver feeds every product back as the next input; on a GPU the loop must not come
// back to the host between products -- a dot product read on the host costs a stream
// synchronisation (20-30 us), more than a whole SpMV of a small matrix.  Here an iteration
// is five launches on one stream and no host round trip:
//   tile kernel + fold            q = A p                        (cfs_hip.hip)
//   cg_dot_kernel                 pq = p . q
//   cg_update_kernel              u += (rr/pq) p;  r -= (rr/pq) q;  rr' = r . r   (one pass)
//   cg_direction_kernel           p = r + (rr'/rr) p;  converged?
// The scalars live in device memory as 512 partial sums each (one per workgroup of the kernel
// that produced them, fp64 whatever the value type); every workgroup of the consuming kernel adds
// them up for itself in a fixed order -- no atomics, bit-reproducible scalars (with a
// deterministic handle the whole solve is).  r . r has two slots, alternating with the parity of
// the iteration (the host passes the iteration number as a kernel argument).  The host looks at
// the convergence flag every `check_every` iterations (one 8-byte copy + synchronisation);
// kernels enqueued behind a converged iteration return at once.  cfs_hip_sym_cg recomputes the
// true residual ||b - A u|| / ||b|| at the end.
//
// Jacobi (cfs_hip_sym_pcg; BS = 1): the same five launches.  dinv_i = (V)(1 / a_ii) is
// built once from the handle's own diagonal (cfs_diag_gather_kernel, then cg_dinv_kernel);
// z = D^-1 r is never stored: z_i = (double)r_i * (double)dinv_i, with r_i the rounded value in
// memory, is formed in fp64 where it is needed --
//   cg_update_kernel<V, 1>        u += (rz/pq) p;  r -= (rz/pq) q;  rz' = r . z;  rr' = r . r
//   cg_direction_kernel<V, 1>     p = dinv r + (rz'/rz) p;  converged?  (rr' <= stop: the
//                                 unpreconditioned residual, the same rule as without)
// r . z has two slots alternating with the parity of the iteration, like r . r.  The BS = 0
// instantiations are the kernels of the plain iteration, operation for operation.
//
// Block Jacobi (cfs_hip_sym_pcg_block, BS = 2, 3, 4, 6): M = blockdiag(A) on the BS x BS node blocks
// of a multi-dof mesh matrix, whose couplings inside a node are as strong as the diagonal.  Set-up, once
// per call: the blocks are gathered from the handle (cfs_block_gather_kernel) and cg_binv_kernel inverts
// them, one thread per block, in fp64 registers (Cholesky, then the inverse); the inverse is stored rounded
// to the value type as its packed lower triangle, structure of arrays (word t of block k at minv[t nb + k]:
// consecutive lanes read consecutive words).  The same five launches per iteration: z_i = sum_j
// (double)Minv_ij (double)r_j over the block, r_j the rounded value in memory, is formed in fp64 inside
// cg_update_kernel<V, BS> (for r . z) and again in cg_direction_kernel<V, BS>, and never stored.  These
// instantiations walk the vectors one node block per thread, grid-stride; the scalars are the same
// partial-sum slots, so a solve on a deterministic handle stays bit-reproducible.
//
// Each of the four kernels is ONE source, templated on BS and on the set of columns it works on: OneColumn for
// the solvers above, ColumnMask for the same recurrence on a block of right-hand sides (cfs_hip_sym_pcg_cols),
// launched once for the block.  See "the recurrence" below.
#pragma once

namespace cfs_solver {

// partial sums: one double per workgroup and quantity (no atomics: thousands of device-scope atomics
// on one address cost tens of microseconds -- they are resolved one after the other -- and their
// order would vary; a fixed grid and a fixed summation order make the scalars bit-reproducible)
constexpr int kThreads = 256;
constexpr int kGrid = 512;                                  // workgroups of every vector kernel
// part[slot][kGrid]; P_RZ0 / P_RZ1 (r . z) and P_BAD (diagonal entries that are not finite and > 0) only with Jacobi
enum Slot { P_RR0 = 0, P_RR1, P_PQ, P_BB, P_RES, P_RZ0, P_RZ1, P_BAD, P_COUNT };
enum Counter { I_ITER = 0, I_DONE, I_COUNT };

// sum of v over the workgroup, returned to every thread (fixed order)
__device__ __forceinline__ double block_sum(double v) {
  __shared__ double part[kThreads / 64];
  __shared__ double total;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  __syncthreads(); // (a second call may not overwrite `total` before everybody has read it)
  if (lane == 0) part[wave] = v;
  __syncthreads();
  if (threadIdx.x == 0) {
    double s = 0.0;
#pragma unroll
    for (int w = 0; w < kThreads / 64; ++w) s += part[w];
    total = s;
  }
  __syncthreads();
  return total;
}
// the scalar a slot holds: the sum of its kGrid partial sums, by every workgroup for itself
__device__ __forceinline__ double slot_sum(const double *part, int slot) {
  double v = 0.0;
  for (int g = threadIdx.x; g < kGrid; g += kThreads) v += part[slot * kGrid + g];
  return block_sum(v);
}

// The vector kernels move 16 bytes per lane and load (two doubles / four floats) over the part of
// the vectors that is a multiple of that -- every vector here is 16-byte aligned: library memory, or
// checked by the entry point -- and single values over the rest; grid-stride.
template <typename V> struct Vec16 {
  static constexpr int W = 16 / (int)sizeof(V);
  typedef V type __attribute__((ext_vector_type(16 / sizeof(V))));
};

// The columns a kernel of the multigrid cycle works on (cfs_solver_cheb.hpp, cfs_solver_amg.hpp), as a type.  Column c of
// a vector lives at base + c ld.  each(f) calls f(c) for every column of the set, ascending; where a kernel's accumulators
// are per column it takes the columns in chunks of chunk(cw): chunks<CW>(f) calls f(c0, bits) per chunk that has a
// column, bit e of bits saying whether column c0 + e is one.
// OneColumn: column 0, known at compile time: no loop, no mask test, and the c ld offsets fold away.
struct OneColumn {
  static constexpr bool one = true;
  static constexpr int chunk(int) { return 1; }
  template <class F> __host__ __device__ __forceinline__ void each(F &&f) const { f(0); }
  template <int CW, class F> __device__ __forceinline__ void chunks(F &&f) const { f(0, 1u); }
};
// ColumnMask: the columns c < ncols <= 16 whose bit is set in `active` (no bit from ncols on is set), known at run time
// and uniform over the grid; a column whose bit is clear is neither read nor written
struct ColumnMask {
  static constexpr bool one = false;
  static constexpr int chunk(int cw) { return cw; }
  int ncols;
  unsigned active;
  template <class F> __host__ __device__ __forceinline__ void each(F &&f) const {
    for (int c = 0; c < ncols; ++c)
      if ((active >> c) & 1u) f(c);
  }
  template <int CW, class F> __device__ __forceinline__ void chunks(F &&f) const {
    for (int c0 = 0; c0 < ncols; c0 += CW)
      if (const unsigned bits = (active >> c0) & ((1u << CW) - 1u)) f(c0, bits);
  }
};

// dinv = (V)(1 / d) in place over the gathered diagonal;  part[P_BAD] <- entries that are not finite and > 0
template <typename V>
__global__ void __launch_bounds__(kThreads) cg_dinv_kernel(V *__restrict__ d, long long n, double *__restrict__ part) {
  double bad = 0.0;
  for (long long i = (long long)blockIdx.x * kThreads + threadIdx.x; i < n; i += (long long)gridDim.x * kThreads) {
    const double a = (double)d[i];
    // (!(a > 0): a NaN counts too)
    if (!(a > 0.0) || a * 0.0 != 0.0) bad += 1.0;
    d[i] = (V)(1.0 / a);
  }
  bad = block_sum(bad);
  if (threadIdx.x == 0) part[P_BAD * kGrid + blockIdx.x] = bad;
}

// ---- block Jacobi --------------------------------------------------------------------------------
constexpr int tri_words(int bs) { return bs * (bs + 1) / 2; } // packed lower triangle of a block

// minv <- the inverse of every BS x BS block of `blocks` (row-major, as cfs_block_gather_kernel leaves
// them), rounded to V, packed lower triangle, word t = i (i + 1) / 2 + j of block k at minv[t nb + k].
// fp64 registers: A = L L^T, then L^-1, then A^-1 = L^-T L^-1.  The positions of a trailing partial block
// that lie outside the matrix count as identity.  part[P_BAD] <- blocks with a pivot that is not finite
// and > 0.  BS = 1: (V)(1 / a), the word cg_dinv_kernel stores.
template <typename V, int BS>
__global__ void __launch_bounds__(kThreads)
    cg_binv_kernel(const V *__restrict__ blocks, V *__restrict__ minv, long long nb, long long n, double *__restrict__ part) {
  double bad = 0.0;
  for (long long k = (long long)blockIdx.x * kThreads + threadIdx.x; k < nb; k += (long long)gridDim.x * kThreads) {
    double a[BS][BS], li[BS][BS];
#pragma unroll
    for (int i = 0; i < BS; ++i)
#pragma unroll
      for (int j = 0; j <= i; ++j)
        a[i][j] = k * BS + i < n ? (double)blocks[k * (BS * BS) + i * BS + j] : (i == j ? 1.0 : 0.0);
    if (BS == 1) {
      if (!(a[0][0] > 0.0) || a[0][0] * 0.0 != 0.0) bad += 1.0;
      minv[k] = (V)(1.0 / a[0][0]);
      continue;
    }
    bool ok = true;
#pragma unroll
    for (int j = 0; j < BS; ++j) { // Cholesky, column by column: a <- L
      double dj = a[j][j];
#pragma unroll
      for (int c = 0; c < j; ++c) dj -= a[j][c] * a[j][c];
      // (!(dj > 0): a NaN counts too)
      if (!(dj > 0.0) || dj * 0.0 != 0.0) ok = false;
      const double l = sqrt(dj);
      a[j][j] = l;
#pragma unroll
      for (int i = j + 1; i < BS; ++i) {
        double v = a[i][j];
#pragma unroll
        for (int c = 0; c < j; ++c) v -= a[i][c] * a[j][c];
        a[i][j] = v / l;
      }
    }
    if (!ok) bad += 1.0;
#pragma unroll
    for (int j = 0; j < BS; ++j) { // li <- L^-1, column by column
      li[j][j] = 1.0 / a[j][j];
#pragma unroll
      for (int i = j + 1; i < BS; ++i) {
        double v = 0.0;
#pragma unroll
        for (int c = j; c < i; ++c) v += a[i][c] * li[c][j];
        li[i][j] = -v / a[i][i];
      }
    }
#pragma unroll
    for (int i = 0; i < BS; ++i)
#pragma unroll
      for (int j = 0; j <= i; ++j) {
        double v = 0.0;
#pragma unroll
        for (int c = i; c < BS; ++c) v += li[c][i] * li[c][j];
        minv[(long long)(i * (i + 1) / 2 + j) * nb + k] = (V)v;
      }
  }
  bad = block_sum(bad);
  if (threadIdx.x == 0) part[P_BAD * kGrid + blockIdx.x] = bad;
}

// full <- the packed inverse as nb full row-major blocks, both triangles (cfs_hip_sym_block_inverse_async)
template <typename V, int BS>
__global__ void __launch_bounds__(kThreads)
    cg_bunpack_kernel(V *__restrict__ full, const V *__restrict__ minv, long long nb) {
  for (long long k = (long long)blockIdx.x * kThreads + threadIdx.x; k < nb; k += (long long)gridDim.x * kThreads)
#pragma unroll
    for (int i = 0; i < BS; ++i)
#pragma unroll
      for (int j = 0; j <= i; ++j) {
        const V v = minv[(long long)(i * (i + 1) / 2 + j) * nb + k];
        full[k * (BS * BS) + i * BS + j] = v;
        full[k * (BS * BS) + j * BS + i] = v;
      }
}

// z = Minv_k r over node block k, in fp64 (r: the block's rounded residual, 0 outside the matrix), in two halves: the
// packed inverse block of node k into registers (the one place that reads the packed layout), and its product with
// one vector's values -- a kernel that works on several columns loads once and multiplies per column
template <typename V, int BS>
__device__ __forceinline__ void block_load(const V *__restrict__ minv, long long nb, long long k, double (&m)[BS][BS]) {
#pragma unroll
  for (int i = 0; i < BS; ++i)
#pragma unroll
    for (int j = 0; j <= i; ++j) m[i][j] = m[j][i] = (double)minv[(long long)(i * (i + 1) / 2 + j) * nb + k];
}
template <int BS> __device__ __forceinline__ void block_mul(const double (&m)[BS][BS], const double (&r)[BS], double (&z)[BS]) {
#pragma unroll
  for (int i = 0; i < BS; ++i) {
    double v = 0.0;
#pragma unroll
    for (int j = 0; j < BS; ++j) v += m[i][j] * r[j];
    z[i] = v;
  }
}
template <typename V, int BS>
__device__ __forceinline__ void block_apply(const V *__restrict__ minv, long long nb, long long k, const double (&r)[BS],
                                            double (&z)[BS]) {
  double m[BS][BS];
  block_load<V, BS>(minv, nb, k, m);
  block_mul<BS>(m, r, z);
}

// ---- the recurrence: four kernels, each written once over the columns of a set CS ------------------
// OneColumn: the one-column solvers (cg, cg_cheb, cg_mixed, Amg::pcg).  ColumnMask: the solvers on a block of
// right-hand sides (cg_cols, Amg::pcg_cols), ONE launch for the block.  Column c of every vector at base + c ld; its
// scalars in slots of its own, part[c][slot][kGrid], its counters at ic[c][I_ITER], ic[c][I_DONE], its stop in
// stop.v[c] -- for one column that is part[slot][kGrid], ic[I_ITER], ic[I_DONE] and stop.v[0], and c ld folds away.
// BS = 0: no stored M^-1, 1: dinv (PRE below), 2, 3, 4, 6: the packed inverse blocks.  BS <= 1 walks 16-byte vectors
// and single values over the rest, BS >= 2 one node block per thread; both grid-stride.  Per column the arithmetic does
// not depend on CS: the same walk, casts, parentheses and order of sums from the same text -- block_sum_cols and
// slot_sums add in the order of block_sum and slot_sum, for the columns of a chunk at once, so a chunk costs the
// barriers of one column.  The columns are taken in chunks of CW (chunks<CW>; one column is one chunk of one, no loop
// and no mask test): the accumulators and the scalars are per column of a chunk, and dinv or the inverse block is
// read once per chunk.  The dot, update and direction kernels do nothing behind a raised ic[I_DONE]: one column
// returns at once; of a block every column whose flag is up is skipped (live_columns) -- nothing of it is read or
// written, not its vectors, its slots or its counters, so a column stops at the iteration at which its one-column
// solve stops while the host's mask may be a window old.  A column whose bit is clear in the mask is neither read nor
// written.
constexpr int kColSlots = P_COUNT * kGrid; // doubles between the slots of two columns
// the first of the two slots the numerator of alpha and beta alternates between: r . z with a stored M^-1, else r . r
constexpr int num_slot(int bs) { return bs >= 1 ? P_RZ0 : P_RR0; }
struct ColumnStops {
  double v[16];
};
// the columns per chunk for a stored M^-1 of BS: the widest that keeps every instantiation free of spills, scalar
// registers included.  four: the residual and update kernels, which hold four vectors' addresses per column
constexpr int cols_chunk(int bs, bool four = false) { return bs >= 6 || (four && bs <= 1) ? 2 : 4; }

// block_sum for N values at once, each summed in block_sum's order
template <int N> __device__ __forceinline__ void block_sum_cols(double (&v)[N]) {
  if constexpr (N == 1) { // (one column: block_sum itself -- the same sum; cg_update_kernel keeps its registers with it)
    v[0] = block_sum(v[0]);
    return;
  }
  __shared__ double part[N][kThreads / 64];
  __shared__ double total[N];
#pragma unroll
  for (int e = 0; e < N; ++e)
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v[e] += __shfl_down(v[e], o);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  __syncthreads();
  if (lane == 0)
#pragma unroll
    for (int e = 0; e < N; ++e) part[e][wave] = v[e];
  __syncthreads();
  if (threadIdx.x < N) {
    double s = 0.0;
#pragma unroll
    for (int w = 0; w < kThreads / 64; ++w) s += part[threadIdx.x][w];
    total[threadIdx.x] = s;
  }
  __syncthreads();
#pragma unroll
  for (int e = 0; e < N; ++e) v[e] = total[e];
}
// out[e] = slot_sum of column c0 + e for the columns of `bits` (0 for the others, whose slots are not read)
template <int CW> __device__ __forceinline__ void slot_sums(const double *part, int slot, int c0, unsigned bits, double (&out)[CW]) {
#pragma unroll
  for (int e = 0; e < CW; ++e) {
    double v = 0.0;
    if ((bits >> e) & 1u)
      for (int g = threadIdx.x; g < kGrid; g += kThreads) v += part[(size_t)(c0 + e) * kColSlots + slot * kGrid + g];
    out[e] = v;
  }
  block_sum_cols<CW>(out);
}
// the columns of cs whose flag is down, the same answer in every thread of the workgroup (one thread reads the flags:
// workgroup 0 of a direction kernel raises them while other workgroups may still be starting)
__device__ __forceinline__ ColumnMask live_columns(const int *ic, ColumnMask cs) {
  __shared__ unsigned live;
  if (threadIdx.x == 0) {
    unsigned m = 0;
    cs.each([&](int c) {
      if (!ic[c * I_COUNT + I_DONE]) m |= 1u << c;
    });
    live = m;
  }
  __syncthreads();
  return ColumnMask{cs.ncols, live};
}
// (one column: the kernel has returned if its flag is up)
__device__ __forceinline__ OneColumn live_columns(const int *, OneColumn cs) { return cs; }

// r = b - q;  p = r (when given);  part[slot_rr] <- r . r;  part[P_BB] <- b . b (when with_bb)
// BS >= 1: p = z = M^-1 r instead, and part[P_RZ0] <- r . z.  r, p may be null for BS = 0
// (BS >= 2, here and in the direction kernel: one column reads the inverse block BEHIND its vector loads, by block_apply,
// so that the block's words are consumed row by row as they arrive, between the loads and stores of p; a block of columns
// reads it once, ahead of its column loop)
template <typename V, int BS, class CS>
__global__ void __launch_bounds__(kThreads)
    cg_residual_kernel(V *__restrict__ r, V *__restrict__ p, const V *__restrict__ b, const V *__restrict__ q, long long ld,
                       long long n, double *__restrict__ part, int slot_rr, int with_bb, const V *__restrict__ minv, long long nb,
                       CS cs) {
  constexpr int CW = CS::chunk(cols_chunk(BS, true));
  constexpr bool PRE = BS == 1;
  cs.template chunks<CW>([&](int c0, unsigned bits) {
    double rr[CW], bb[CW], rz[CW];
#pragma unroll
    for (int e = 0; e < CW; ++e) rr[e] = bb[e] = rz[e] = 0.0;
    if constexpr (BS >= 2) {
      for (long long k = (long long)blockIdx.x * kThreads + threadIdx.x; k < nb; k += (long long)gridDim.x * kThreads) {
        double m[BS][BS];
        if constexpr (!CS::one) block_load<V, BS>(minv, nb, k, m);
#pragma unroll
        for (int e = 0; e < CW; ++e) {
          if (!((bits >> e) & 1u)) continue;
          const long long off = (long long)(c0 + e) * ld;
          double rd[BS], z[BS];
#pragma unroll
          for (int i = 0; i < BS; ++i) {
            const long long g = k * BS + i;
            rd[i] = 0.0;
            if (g < n) {
              const V bi = b[off + g], ri = bi - q[off + g];
              r[off + g] = ri;
              rd[i] = (double)ri;
              rr[e] += (double)ri * (double)ri;
              bb[e] += (double)bi * (double)bi;
            }
          }
          if constexpr (CS::one) block_apply<V, BS>(minv, nb, k, rd, z);
          else block_mul<BS>(m, rd, z);
#pragma unroll
          for (int i = 0; i < BS; ++i) {
            const long long g = k * BS + i;
            if (g < n) {
              rz[e] += rd[i] * z[i];
              p[off + g] = (V)z[i];
            }
          }
        }
      }
    } else {
      constexpr int W = Vec16<V>::W;
      typedef typename Vec16<V>::type VT;
      const long long nv = n / W, t0 = (long long)blockIdx.x * kThreads + threadIdx.x, stride = (long long)gridDim.x * kThreads;
      for (long long i = t0; i < nv; i += stride) {
        VT dv;
        if (PRE) dv = reinterpret_cast<const VT *>(minv)[i];
#pragma unroll
        for (int e = 0; e < CW; ++e) {
          if (!((bits >> e) & 1u)) continue;
          const long long off = (long long)(c0 + e) * ld;
          const VT bv = reinterpret_cast<const VT *>(b + off)[i], qv = reinterpret_cast<const VT *>(q + off)[i];
          VT rv, zv;
#pragma unroll
          for (int k = 0; k < W; ++k) {
            rv[k] = bv[k] - qv[k];
            rr[e] += (double)rv[k] * (double)rv[k];
            bb[e] += (double)bv[k] * (double)bv[k];
            if (PRE) {
              const double z = (double)rv[k] * (double)dv[k];
              rz[e] += (double)rv[k] * z;
              zv[k] = (V)z;
            }
          }
          if (r) reinterpret_cast<VT *>(r + off)[i] = rv;
          if (p) reinterpret_cast<VT *>(p + off)[i] = PRE ? zv : rv;
        }
      }
      for (long long i = nv * W + t0; i < n; i += stride) {
        const V di = PRE ? minv[i] : (V)0;
#pragma unroll
        for (int e = 0; e < CW; ++e) {
          if (!((bits >> e) & 1u)) continue;
          const long long off = (long long)(c0 + e) * ld;
          const V bi = b[off + i], ri = bi - q[off + i];
          if (r) r[off + i] = ri;
          if (PRE) {
            const double z = (double)ri * (double)di;
            rz[e] += (double)ri * z;
            if (p) p[off + i] = (V)z;
          } else if (p) {
            p[off + i] = ri;
          }
          rr[e] += (double)ri * (double)ri;
          bb[e] += (double)bi * (double)bi;
        }
      }
    }
    block_sum_cols<CW>(rr);
    block_sum_cols<CW>(bb);
    if (BS >= 1) block_sum_cols<CW>(rz);
    if (threadIdx.x == 0)
#pragma unroll
      for (int e = 0; e < CW; ++e)
        if ((bits >> e) & 1u) {
          double *pc = part + (size_t)(c0 + e) * kColSlots;
          pc[slot_rr * kGrid + blockIdx.x] = rr[e];
          if (with_bb) pc[P_BB * kGrid + blockIdx.x] = bb[e];
          if (BS >= 1) pc[P_RZ0 * kGrid + blockIdx.x] = rz[e];
        }
  });
}

// part[slot] <- a . b of the stored values (p . q into P_PQ; r . z where z is stored: cfs_solver_amg.hpp)
template <typename V, class CS>
__global__ void __launch_bounds__(kThreads)
    cg_dot_kernel(const V *__restrict__ a, const V *__restrict__ b, long long ld, long long n, double *__restrict__ part, int slot,
                  const int *__restrict__ ic, CS cs) {
  constexpr int CW = CS::chunk(cols_chunk(0));
  if constexpr (CS::one)
    if (ic[I_DONE]) return;
  live_columns(ic, cs).template chunks<CW>([&](int c0, unsigned bits) {
    constexpr int W = Vec16<V>::W;
    typedef typename Vec16<V>::type VT;
    const long long nv = n / W, t0 = (long long)blockIdx.x * kThreads + threadIdx.x, stride = (long long)gridDim.x * kThreads;
    double s[CW];
#pragma unroll
    for (int e = 0; e < CW; ++e) s[e] = 0.0;
    for (long long i = t0; i < nv; i += stride)
#pragma unroll
      for (int e = 0; e < CW; ++e) {
        if (!((bits >> e) & 1u)) continue;
        const long long off = (long long)(c0 + e) * ld;
        const VT av = reinterpret_cast<const VT *>(a + off)[i], bv = reinterpret_cast<const VT *>(b + off)[i];
#pragma unroll
        for (int k = 0; k < W; ++k) s[e] += (double)av[k] * (double)bv[k];
      }
    for (long long i = nv * W + t0; i < n; i += stride)
#pragma unroll
      for (int e = 0; e < CW; ++e) {
        if (!((bits >> e) & 1u)) continue;
        const long long off = (long long)(c0 + e) * ld;
        s[e] += (double)a[off + i] * (double)b[off + i];
      }
    block_sum_cols<CW>(s);
    if (threadIdx.x == 0)
#pragma unroll
      for (int e = 0; e < CW; ++e)
        if ((bits >> e) & 1u) part[(size_t)(c0 + e) * kColSlots + slot * kGrid + blockIdx.x] = s[e];
  });
}

// alpha = rr / pq;  u += alpha p;  r -= alpha q;  part[rr of the next iteration] <- r . r
// BS >= 1: alpha = rz / pq, and part[rz of the next iteration] <- r . z with z = M^-1 r of the ROUNDED r
// ALPHA: the first of the two slots alpha's numerator alternates between (BS = 0 with P_RZ0: z is stored elsewhere and
// r . z comes from cg_dot_kernel, cfs_solver_amg.hpp).  Registers: a block reads M^-1 ahead of its columns, one column
// behind its vectors (block_apply) -- read ahead, it holds dinv or the inverse block across the loads; and the body is
// inlined before it is optimised (always_inline), or the 21 words of a 6 x 6 fp64 block are all loaded before the first
// product: 76 VGPRs and 6 waves per SIMD where these lines keep the 62 and 8 of a kernel without a lambda.  They steer
// THIS compiler's scheduler and nothing committed guards them: after a compiler change, re-check the one-column side of
// the resource table in DESIGN.md ("PCG on a block of right-hand sides")
template <typename V, int BS, int ALPHA, class CS>
__global__ void __launch_bounds__(kThreads)
    cg_update_kernel(V *__restrict__ u, V *__restrict__ r, const V *__restrict__ p, const V *__restrict__ q, long long ld,
                     long long n, double *__restrict__ part, const int *__restrict__ ic, int it, const V *__restrict__ minv,
                     long long nb, CS cs) {
  constexpr int CW = CS::chunk(cols_chunk(BS, true));
  constexpr bool PRE = BS == 1;
  if constexpr (CS::one)
    if (ic[I_DONE]) return;
  live_columns(ic, cs).template chunks<CW>([&](int c0, unsigned bits) __attribute__((always_inline)) {
    double alpha[CW], s[CW], sz[CW];
    {
      double pq[CW], rr_old[CW];
      slot_sums<CW>(part, P_PQ, c0, bits, pq);
      slot_sums<CW>(part, ALPHA + (it & 1), c0, bits, rr_old);
#pragma unroll
      for (int e = 0; e < CW; ++e) {
        alpha[e] = pq[e] != 0.0 ? rr_old[e] / pq[e] : 0.0;
        s[e] = sz[e] = 0.0;
      }
    }
    if constexpr (BS >= 2) {
      for (long long k = (long long)blockIdx.x * kThreads + threadIdx.x; k < nb; k += (long long)gridDim.x * kThreads) {
        double m[BS][BS];
        if constexpr (!CS::one) block_load<V, BS>(minv, nb, k, m);
#pragma unroll
        for (int e = 0; e < CW; ++e) {
          if (!((bits >> e) & 1u)) continue;
          const long long off = (long long)(c0 + e) * ld;
          double rd[BS], z[BS];
#pragma unroll
          for (int i = 0; i < BS; ++i) {
            const long long g = k * BS + i;
            rd[i] = 0.0;
            if (g < n) {
              u[off + g] = (V)((double)u[off + g] + alpha[e] * (double)p[off + g]);
              const double ri = (double)r[off + g] - alpha[e] * (double)q[off + g];
              const V rn = (V)ri;
              r[off + g] = rn;
              s[e] += ri * ri;
              rd[i] = (double)rn;
            }
          }
          if constexpr (CS::one) block_apply<V, BS>(minv, nb, k, rd, z);
          else block_mul<BS>(m, rd, z);
#pragma unroll
          for (int i = 0; i < BS; ++i) sz[e] += rd[i] * z[i]; // (rd = 0 outside the matrix)
        }
      }
    } else {
      constexpr int W = Vec16<V>::W;
      typedef typename Vec16<V>::type VT;
      const long long nv = n / W, t0 = (long long)blockIdx.x * kThreads + threadIdx.x, stride = (long long)gridDim.x * kThreads;
      for (long long i = t0; i < nv; i += stride) {
        VT dv;
        if (PRE && !CS::one) dv = reinterpret_cast<const VT *>(minv)[i];
#pragma unroll
        for (int e = 0; e < CW; ++e) {
          if (!((bits >> e) & 1u)) continue;
          const long long off = (long long)(c0 + e) * ld;
          VT uv = reinterpret_cast<VT *>(u + off)[i], rv = reinterpret_cast<VT *>(r + off)[i];
          const VT pv = reinterpret_cast<const VT *>(p + off)[i], qv = reinterpret_cast<const VT *>(q + off)[i];
          if (PRE && CS::one) dv = reinterpret_cast<const VT *>(minv)[i];
#pragma unroll
          for (int k = 0; k < W; ++k) {
            uv[k] = (V)((double)uv[k] + alpha[e] * (double)pv[k]);
            const double ri = (double)rv[k] - alpha[e] * (double)qv[k];
            rv[k] = (V)ri;
            s[e] += ri * ri;
            if (PRE) sz[e] += (double)rv[k] * ((double)rv[k] * (double)dv[k]);
          }
          reinterpret_cast<VT *>(u + off)[i] = uv;
          reinterpret_cast<VT *>(r + off)[i] = rv;
        }
      }
      for (long long i = nv * W + t0; i < n; i += stride) {
        const V di = PRE ? minv[i] : (V)0;
#pragma unroll
        for (int e = 0; e < CW; ++e) {
          if (!((bits >> e) & 1u)) continue;
          const long long off = (long long)(c0 + e) * ld;
          u[off + i] = (V)((double)u[off + i] + alpha[e] * (double)p[off + i]);
          const double ri = (double)r[off + i] - alpha[e] * (double)q[off + i];
          const V rn = (V)ri;
          r[off + i] = rn;
          s[e] += ri * ri;
          if (PRE) sz[e] += (double)rn * ((double)rn * (double)di);
        }
      }
    }
    block_sum_cols<CW>(s);
    if (BS >= 1) block_sum_cols<CW>(sz);
    if (threadIdx.x == 0)
#pragma unroll
      for (int e = 0; e < CW; ++e)
        if ((bits >> e) & 1u) {
          double *pc = part + (size_t)(c0 + e) * kColSlots;
          pc[(P_RR0 + ((it + 1) & 1)) * kGrid + blockIdx.x] = s[e];
          if (BS >= 1) pc[(P_RZ0 + ((it + 1) & 1)) * kGrid + blockIdx.x] = sz[e];
        }
  });
}

// r d + beta p (PRE) or r + beta p of cg_direction_kernel.  With PRE the sum of two products can be contracted two
// ways, and which one the compiler takes depends on the code around it: written as r * d + beta * p, the one-column
// form was compiled to fma(r, d, beta p) in both value types, in its vector loop and in its tail, while the same
// expression inside a column loop became fma(beta, p, r d), whose iterates differ in the last bit.  So the contraction
// is spelled out here, for both instantiations; test C1 of tests/test_gpu_pcg_cols.py fails if the two ever part.
template <bool PRE> __device__ __forceinline__ double direction_sum(double r, double d, double beta, double p) {
  if constexpr (PRE) {
    const double bp = beta * p;
    return __builtin_fma(r, d, bp);
  } else {
    return r + beta * p;
  }
}

// beta = rr' / rr;  p = r + beta p;  one thread: iteration count, convergence flag (rr' <= stop), per column
// BS >= 1: beta = rz' / rz;  p = M^-1 r + beta p;  the flag still from rr', the unpreconditioned residual
// S0: the first of the two slots beta alternates between (BS = 0 with P_RZ0 and the stored z for r: p = z + beta p,
// cfs_solver_cheb.hpp, cfs_solver_amg.hpp)
template <typename V, int BS, int S0, class CS>
__global__ void __launch_bounds__(kThreads)
    cg_direction_kernel(V *__restrict__ p, const V *__restrict__ r, long long ld, long long n, const double *__restrict__ part,
                        int *__restrict__ ic, int it, ColumnStops stop, const V *__restrict__ minv, long long nb, CS cs) {
  constexpr int CW = CS::chunk(cols_chunk(BS));
  constexpr bool PRE = BS == 1;
  if constexpr (CS::one)
    if (ic[I_DONE]) return;
  live_columns(ic, cs).template chunks<CW>([&](int c0, unsigned bits) {
    double beta[CW], res[CW];
    {
      double rr[CW];
      slot_sums<CW>(part, S0 + (it & 1), c0, bits, rr);
      slot_sums<CW>(part, S0 + ((it + 1) & 1), c0, bits, res);
#pragma unroll
      for (int e = 0; e < CW; ++e) beta[e] = rr[e] != 0.0 ? res[e] / rr[e] : 0.0;
      // what the stopping rule looks at: r . r (only workgroup 0 adds it up)
      if (S0 != P_RR0 && blockIdx.x == 0) slot_sums<CW>(part, P_RR0 + ((it + 1) & 1), c0, bits, res);
    }
    if constexpr (BS >= 2) {
      for (long long k = (long long)blockIdx.x * kThreads + threadIdx.x; k < nb; k += (long long)gridDim.x * kThreads) {
        double m[BS][BS];
        if constexpr (!CS::one) block_load<V, BS>(minv, nb, k, m);
#pragma unroll
        for (int e = 0; e < CW; ++e) {
          if (!((bits >> e) & 1u)) continue;
          const long long off = (long long)(c0 + e) * ld;
          double rd[BS], z[BS];
#pragma unroll
          for (int i = 0; i < BS; ++i) {
            const long long g = k * BS + i;
            rd[i] = g < n ? (double)r[off + g] : 0.0;
          }
          if constexpr (CS::one) block_apply<V, BS>(minv, nb, k, rd, z);
          else block_mul<BS>(m, rd, z);
#pragma unroll
          for (int i = 0; i < BS; ++i) {
            const long long g = k * BS + i;
            if (g < n) p[off + g] = (V)(z[i] + beta[e] * (double)p[off + g]);
          }
        }
      }
    } else {
      constexpr int W = Vec16<V>::W;
      typedef typename Vec16<V>::type VT;
      const long long nv = n / W, t0 = (long long)blockIdx.x * kThreads + threadIdx.x, stride = (long long)gridDim.x * kThreads;
      for (long long i = t0; i < nv; i += stride) {
        VT dv;
        if (PRE) dv = reinterpret_cast<const VT *>(minv)[i];
#pragma unroll
        for (int e = 0; e < CW; ++e) {
          if (!((bits >> e) & 1u)) continue;
          const long long off = (long long)(c0 + e) * ld;
          VT pv = reinterpret_cast<VT *>(p + off)[i];
          const VT rv = reinterpret_cast<const VT *>(r + off)[i];
#pragma unroll
          for (int k = 0; k < W; ++k)
            pv[k] = (V)direction_sum<PRE>((double)rv[k], PRE ? (double)dv[k] : 0.0, beta[e], (double)pv[k]);
          reinterpret_cast<VT *>(p + off)[i] = pv;
        }
      }
      for (long long i = nv * W + t0; i < n; i += stride) {
        const V di = PRE ? minv[i] : (V)0;
#pragma unroll
        for (int e = 0; e < CW; ++e) {
          if (!((bits >> e) & 1u)) continue;
          const long long off = (long long)(c0 + e) * ld;
          p[off + i] = (V)direction_sum<PRE>((double)r[off + i], (double)di, beta[e], (double)p[off + i]);
        }
      }
    }
    if (blockIdx.x == 0 && threadIdx.x == 0)
#pragma unroll
      for (int e = 0; e < CW; ++e)
        if ((bits >> e) & 1u) {
          int *icc = ic + (c0 + e) * I_COUNT;
          icc[I_ITER] += 1; // (counted on the device: a replayed graph passes the same `it` again, only its parity matters)
          // (!(x > y): a NaN residual also ends the iteration)
          if (!(res[e] > stop.v[c0 + e])) icc[I_DONE] = 1;
        }
  });
}

// ---- host: what every solver behind the C ABI shares ---------------------------------------------
// n values of V (+ 64 bytes) in each of the buffers
template <typename V> inline int alloc_vectors(long long n, std::initializer_list<cfs_rt::DevBuf *> bufs) {
  for (cfs_rt::DevBuf *b : bufs)
    if (int rc = b->alloc((size_t)n * sizeof(V) + 64)) return rc;
  return 0;
}

// the host side of partial-sum slots, part[nslots][kGrid] (P_*, M_* of MINRES, L_* of the power method): the device
// array, its mirror and the stream it is read on
struct Slots {
  cfs_rt::DevBuf buf;
  std::vector<double> host;
  hipStream_t st = nullptr;
  double *dev() const { return (double *)buf.p; }
  int alloc(int nslots, hipStream_t stream) {
    st = stream;
    host.assign((size_t)nslots * kGrid, 0.0);
    return buf.alloc(host.size() * sizeof(double));
  }
  int zero() {
    HIPCHK(hipMemsetAsync(buf.p, 0, host.size() * sizeof(double), st));
    return 0;
  }
  // a host look: every slot in one copy, one synchronisation of the stream
  int fetch() {
    HIPCHK(hipMemcpyAsync(host.data(), buf.p, host.size() * sizeof(double), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    return 0;
  }
  // the scalar a slot held at the last fetch(): its partial sums added in the order g = 0 .. kGrid - 1 (the order
  // fixes bb, stop and relres: it is not free to change)
  double sum(int slot) const {
    double s = 0.0;
    for (int g = 0; g < kGrid; g++) s += host[(size_t)slot * kGrid + g];
    return s;
  }
};

// the stored M^-1 of one call, from the handle's own entries: nothing (BS = 0), dinv = (V)(1 / a_ii) (BS = 1) or the
// packed inverse node blocks (BS = 2, 3, 4, 6).  The kernels' PRE is BS == 1.
template <typename V, int BS> struct Precond {
  static_assert(BS == 0 || BS == 1 || BS == 2 || BS == 3 || BS == 4 || BS == 6, "the block sizes of cfs_hip.h");
  cfs_rt::DevBuf dbuf, blkbuf; // the inverse; the gathered full blocks (BS >= 2)
  long long nb = 0;            // node blocks (BS >= 2)
  const V *minv() const { return (const V *)dbuf.p; }
  // enqueues gather and inversion; entries / blocks that are not positive (definite) are counted into part[P_BAD],
  // which the caller has zeroed.  gathered: room for the full blocks of the caller's own (cfs_hip_sym_block_inverse_async,
  // BS = 1 included: block_diagonal and cg_binv_kernel then)
  template <class Handle> int setup(Handle *h, double *part, hipStream_t st, void *gathered = nullptr) {
    if constexpr (BS >= 1) {
      const long long n = h->n(), nblk = (n + BS - 1) / BS;
      int rc;
      if (BS >= 2 || gathered) {
        if (BS >= 2) nb = nblk;
        if ((rc = dbuf.alloc((size_t)nblk * tri_words(BS) * sizeof(V) + 64)) ||
            (!gathered && (rc = blkbuf.alloc((size_t)nblk * BS * BS * sizeof(V) + 64))))
          return rc;
        void *blocks = gathered ? gathered : blkbuf.p;
        if ((rc = h->block_diagonal(blocks, BS, st))) return rc;
        hipLaunchKernelGGL((cg_binv_kernel<V, BS>), dim3(kGrid), dim3(kThreads), 0, st, (const V *)blocks, (V *)dbuf.p, nblk, n, part);
      } else {
        if ((rc = dbuf.alloc((size_t)n * sizeof(V) + 64)) || (rc = h->diagonal(dbuf.p, st))) return rc;
        hipLaunchKernelGGL((cg_dinv_kernel<V>), dim3(kGrid), dim3(kThreads), 0, st, (V *)dbuf.p, n, part);
      }
      HIPCHK(hipGetLastError());
    }
    return 0;
  }
  static int refuse(const char *who, double bad, long long n, long long nb) {
    if (BS >= 2)
      return cfs_rt::set_err(CFS_HIP_ERR_ARG, std::string(who) + ": block Jacobi needs positive definite diagonal blocks, " +
                                                  std::to_string((long long)bad) + " of " + std::to_string(nb) + " blocks of " +
                                                  std::to_string(BS) + " rows have a pivot that is zero, negative or not finite");
    return cfs_rt::set_err(CFS_HIP_ERR_ARG, std::string(who) + ": Jacobi needs a positive diagonal, " + std::to_string((long long)bad) +
                                                " of " + std::to_string(n) + " entries are zero, negative or not finite");
  }
  // after a fetch() of the slots set-up counted into: 0, or the refusal
  int check(const char *who, const Slots &part, long long n) const {
    const double bad = BS >= 1 ? part.sum(P_BAD) : 0.0;
    return bad != 0.0 ? refuse(who, bad, n, nb) : 0;
  }
};

// the inverse blocks cfs_hip_sym_pcg_block would use now, as nb full row-major blocks
// (cfs_hip_sym_block_inverse_async): the solver's set-up, gathering into the caller's memory, then the unpack
template <typename V, int BS, class Handle> int block_inverse(Handle *h, void *minv_dev, hipStream_t st) {
  Precond<V, BS> pre; // (freed on return: hipFree waits for the kernels that use them)
  cfs_rt::DevBuf part;
  int rc;
  if ((rc = part.alloc((size_t)P_COUNT * kGrid * sizeof(double))) || (rc = pre.setup(h, (double *)part.p, st, minv_dev))) return rc;
  hipLaunchKernelGGL((cg_bunpack_kernel<V, BS>), dim3(kGrid), dim3(kThreads), 0, st, (V *)minv_dev, pre.minv(),
                     (h->n() + BS - 1) / BS);
  HIPCHK(hipGetLastError());
  return 0;
}

// check_every as the windowed solvers use it: < 1 means 8, and never more than `cap` iterations between two looks
// (more than ~100 launches enqueued ahead of the GPU make the runtime stall: pwtk stand-in, 64 iterations = 320
// launches between two looks, 187 us per iteration instead of 32)
inline int look_window(int check_every, int cap = 16) { return std::min(check_every < 1 ? 8 : check_every, cap); }

// The host side of preconditioned CG, the part cg(), cg_cheb() and Amg::pcg() share: r, p, q, the slots and the
// counters; the first residual and the first look; the looks at the counters between windows of iterations; the true
// residual of what is returned.  A solver calls these in order and enqueues its own recurrence between them:
//   begin;  [its set-up of M^-1];  first_residual (or product_u, a residual kernel of its own, first_look);
//   [its refusals: u has not been written];  if (live()) [its start];
//   while (live()) { until = window_end(w);  [iterations it .. until - 1, ++it each];  look(); }   finish
template <typename V, class Handle> struct Pcg {
  Handle *h = nullptr;
  V *u = nullptr;
  const V *b = nullptr;
  long long n = 0;
  hipStream_t st = nullptr;
  int maxiter = 0;
  double tol = 0.0, bb = 0.0, stop = 0.0;
  cfs_rt::DevBuf rbuf, pbuf, qbuf, cnt;
  Slots part;
  V *r = nullptr, *p = nullptr, *q = nullptr;
  int *ic = nullptr;
  int host_ic[I_COUNT] = {0, 0};
  int it = 0;        // iterations enqueued
  bool done = false; // the device has raised ic[I_DONE], or the first guess already solves it (or b = 0)

  int begin(const char *who, Handle *handle, void *u_dev, const void *b_dev, double tolerance, int max_iterations, hipStream_t stream) {
    h = handle, u = (V *)u_dev, b = (const V *)b_dev, n = h->n(), st = stream, tol = tolerance, maxiter = max_iterations;
    if (h->rows() != h->n())
      return cfs_rt::set_err(CFS_HIP_ERR_UNSUPPORTED, std::string(who) + ": the handle holds a row block, not the whole matrix");
    int rc;
    if ((rc = alloc_vectors<V>(n, {&rbuf, &pbuf, &qbuf})) || (rc = part.alloc(P_COUNT, st)) || (rc = cnt.alloc(I_COUNT * sizeof(int))))
      return rc;
    r = (V *)rbuf.p, p = (V *)pbuf.p, q = (V *)qbuf.p, ic = (int *)cnt.p;
    if ((rc = part.zero())) return rc;
    HIPCHK(hipMemsetAsync(ic, 0, I_COUNT * sizeof(int), st));
    return 0;
  }
  int product_u() { return h->spmv_local(q, u, nullptr, st); } // q = A u
  // behind a residual kernel that left r . r in P_RR0 and b . b in P_BB
  int first_look() {
    HIPCHK(hipGetLastError());
    if (int rc = part.fetch()) return rc;
    bb = part.sum(P_BB);
    stop = tol * tol * bb;
    done = !(part.sum(P_RR0) > stop);
    return 0;
  }
  // r = b - A u, rr[0] = r . r, bb = b . b by the residual kernel of the plain iteration (the same bits), and the look
  int first_residual() {
    if (int rc = product_u()) return rc;
    hipLaunchKernelGGL((cg_residual_kernel<V, 0, OneColumn>), dim3(kGrid), dim3(kThreads), 0, st, r, (V *)nullptr, b, (const V *)q, n, n,
                       part.dev(), (int)P_RR0, 1, (const V *)nullptr, 0LL, OneColumn{});
    return first_look();
  }
  bool live() const { return !done && it < maxiter; } // (maxiter = 0 behaves like done)
  int window_end(int window) const { return std::min(maxiter, it + window); }
  int look() { // one 8-byte copy + synchronisation
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(host_ic, ic, sizeof host_ic, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    done = host_ic[I_DONE] != 0;
    return 0;
  }
  // the true residual of what is returned; *iterations from the device's counter; relres absolute when bb = 0
  int finish(int *iterations, double *relres) {
    int rc;
    if ((rc = product_u())) return rc;
    hipLaunchKernelGGL((cg_residual_kernel<V, 0, OneColumn>), dim3(kGrid), dim3(kThreads), 0, st, (V *)nullptr, (V *)nullptr, b,
                       (const V *)q, n, n, part.dev(), (int)P_RES, 0, (const V *)nullptr, 0LL, OneColumn{});
    HIPCHK(hipGetLastError());
    if ((rc = part.fetch())) return rc;
    const double res2 = part.sum(P_RES);
    HIPCHK(hipMemcpy(host_ic, ic, sizeof host_ic, hipMemcpyDeviceToHost));
    if (iterations) *iterations = host_ic[I_ITER];
    if (relres) *relres = bb > 0.0 ? std::sqrt(res2 / bb) : std::sqrt(res2);
    return 0;
  }
};

// cfs_hip_sym_cg (BS = 0), cfs_hip_sym_pcg (1), cfs_hip_sym_pcg_block (2, 3, 4, 6).  u: in = first guess, out = solution.
// Returns 0 / an error code; *iterations, *relres as documented in cfs_hip.h
template <typename V, int BS = 0, class Handle>
int cg(Handle *h, void *u_dev, const void *b_dev, double tol, int maxiter, int check_every, int *iterations,
       double *relres, hipStream_t st) {
  check_every = look_window(check_every);
  const char *eg = getenv("CFS_HIP_CG_GRAPH");
  const bool use_graph = eg && atoi(eg) != 0;
  Pcg<V, Handle> s;
  Precond<V, BS> pre;
  int rc;
  if ((rc = s.begin("cg", h, u_dev, b_dev, tol, maxiter, st)) || (rc = pre.setup(h, s.part.dev(), st))) return rc;
  V *u = s.u, *r = s.r, *p = s.p, *q = s.q;
  const long long n = s.n, nb = pre.nb;
  double *part = s.part.dev();
  int *ic = s.ic;
  const V *minv = pre.minv();
  constexpr OneColumn one{};
  // r = b - A u, p = r, rr[0] = r . r, bb = b . b  (BS >= 1: p = M^-1 r, rz[0] = r . p), in one pass
  if ((rc = s.product_u())) return rc;
  hipLaunchKernelGGL((cg_residual_kernel<V, BS, OneColumn>), dim3(kGrid), dim3(kThreads), 0, st, r, p, s.b, (const V *)q, n, n, part,
                     (int)P_RR0, 1, minv, nb, one);
  if ((rc = s.first_look()) || (rc = pre.check("pcg", s.part, n))) return rc; // (u has not been touched yet)
  const ColumnStops stop{{s.stop}};
  auto iteration = [&](int k) -> int {
    int r2 = h->spmv_local(q, p, nullptr, st);
    if (r2) return r2;
    hipLaunchKernelGGL((cg_dot_kernel<V, OneColumn>), dim3(kGrid), dim3(kThreads), 0, st, (const V *)p, (const V *)q, n, n, part,
                       (int)P_PQ, (const int *)ic, one);
    hipLaunchKernelGGL((cg_update_kernel<V, BS, num_slot(BS), OneColumn>), dim3(kGrid), dim3(kThreads), 0, st, u, r, (const V *)p,
                       (const V *)q, n, n, part, (const int *)ic, k, minv, nb, one);
    hipLaunchKernelGGL((cg_direction_kernel<V, BS, num_slot(BS), OneColumn>), dim3(kGrid), dim3(kThreads), 0, st, p, (const V *)r, n,
                       n, (const double *)part, ic, k, stop, minv, nb, one);
    return 0;
  };
  // CFS_HIP_CG_GRAPH=1: two iterations (both parities) captured once and replayed as one graph launch.
  // Measured and NOT the default: the replay is 3-10 % slower than ten plain launches (pwtk stand-in
  // 34.2 against 31.1 us per iteration, ldoor 91 / 87, Flan 145 / 142) -- as for the SpMV's two launches
  // alone; the host enqueues plain launches faster than the GPU retires them anyway.
  hipGraph_t graph = nullptr;
  hipGraphExec_t gexec = nullptr;
  struct GraphGuard {
    hipGraph_t &g;
    hipGraphExec_t &e;
    ~GraphGuard() {
      if (e) (void)hipGraphExecDestroy(e);
      if (g) (void)hipGraphDestroy(g);
    }
  } graph_guard{graph, gexec};
  if (use_graph && !s.done && maxiter >= 2 && st != nullptr) {
    bool ok = hipStreamBeginCapture(st, hipStreamCaptureModeThreadLocal) == hipSuccess;
    if (ok) {
      const int r0 = iteration(0), r1 = r0 ? r0 : iteration(1);
      ok = hipStreamEndCapture(st, &graph) == hipSuccess && !r1 && graph &&
           hipGraphInstantiate(&gexec, graph, nullptr, nullptr, 0) == hipSuccess;
    }
    if (!ok) {
      (void)hipGetLastError();
      gexec = nullptr;
    }
  }
  while (s.live()) {
    const int until = s.window_end(check_every);
    while (s.it < until) {
      if (gexec && (s.it & 1) == 0 && s.it + 2 <= until) {
        HIPCHK(hipGraphLaunch(gexec, st));
        s.it += 2;
      } else {
        if ((rc = iteration(s.it))) return rc;
        ++s.it;
      }
    }
    if ((rc = s.look())) return rc;
  }
  return s.finish(iterations, relres);
}

// ---- preconditioned CG on a block of right-hand sides ---------------------------------------------
// The iterations a block solve may enqueue between two host looks.  The limit of look_window() is on LAUNCHES: its cap
// of 16 iterations of 5 launches keeps at most 80 of them ahead of the GPU, under the ~100 beyond which the runtime
// stalls.  An iteration of a block with k columns the host believes active is 2 k + 3 launches -- a product is two,
// the tile kernel and the fold, and there is one per column; then the dot, update and direction kernels, once for
// the block -- so the window is the largest w with w (2 k + 3) <= 80, at least 1 (k = 16: 35 launches, w = 2; k = 1:
// 5 launches, w = 16), and never more than check_every asks for.  The window only decides when the host looks: a
// column is frozen by the device at its own iteration, so the bits do not depend on it.
inline int look_window_cols(int check_every, int active_cols) {
  return look_window(check_every, std::max(1, 80 / (2 * active_cols + 3)));
}

// Pcg<V, Handle> for the columns c < ncols of blocks U and B with leading dimension ld: R, P, Q are blocks with the
// caller's ld, there is one slot array part[c][slot][kGrid] and one counter array ic[c][I_COUNT].  `active`: the columns
// the host believes are not done; after first_look() those with r_c . r_c > stop_c (a column with b_c = 0, one whose
// first guess solves it or one with a NaN never is), after look() those whose flag the device has not raised.
//   begin;  [set-up of M^-1];  product_u(all());  a residual kernel;  first_look;  [refusals: U has not been written];
//   while (live()) { until = window_end();  [iterations it .. until - 1 on the columns of active, ++it each];  look(); }
//   finish
template <typename V, class Handle> struct PcgCols {
  Handle *h = nullptr;
  V *u = nullptr;
  const V *b = nullptr;
  long long n = 0, ld = 0;
  int ncols = 0;
  hipStream_t st = nullptr;
  int maxiter = 0, check_every = 0;
  double tol = 0.0;
  std::vector<double> bb;
  ColumnStops stop;
  cfs_rt::DevBuf rbuf, pbuf, qbuf, cnt;
  Slots part;
  V *r = nullptr, *p = nullptr, *q = nullptr;
  int *ic = nullptr;
  std::vector<int> host_ic;
  int it = 0;          // iterations enqueued
  unsigned active = 0; // the columns the host believes are not done
  unsigned ever = 0;   // the columns that were active after the first look

  unsigned all() const { return ncols >= 32 ? ~0u : (1u << ncols) - 1u; }
  ColumnMask mask(unsigned bits) const { return ColumnMask{ncols, bits}; }
  size_t block_values() const { return (size_t)(ncols - 1) * (size_t)ld + (size_t)n; }

  int begin(const char *who, Handle *handle, void *u_dev, const void *b_dev, long long lead, int columns, double tolerance,
            int max_iterations, int look_every, hipStream_t stream) {
    h = handle, u = (V *)u_dev, b = (const V *)b_dev, n = h->n(), ld = lead, ncols = columns, st = stream, tol = tolerance;
    maxiter = max_iterations, check_every = look_every;
    if (h->rows() != h->n())
      return cfs_rt::set_err(CFS_HIP_ERR_UNSUPPORTED, std::string(who) + ": the handle holds a row block, not the whole matrix");
    int rc;
    if ((rc = alloc_vectors<V>((long long)block_values(), {&rbuf, &pbuf, &qbuf})) || (rc = part.alloc(ncols * P_COUNT, st)) ||
        (rc = cnt.alloc((size_t)ncols * I_COUNT * sizeof(int))))
      return rc;
    r = (V *)rbuf.p, p = (V *)pbuf.p, q = (V *)qbuf.p, ic = (int *)cnt.p;
    bb.assign(ncols, 0.0);
    host_ic.assign((size_t)ncols * I_COUNT, 0);
    for (double &s : stop.v) s = 0.0;
    if ((rc = part.zero())) return rc;
    HIPCHK(hipMemsetAsync(ic, 0, (size_t)ncols * I_COUNT * sizeof(int), st));
    return 0;
  }
  // dst_c = A src_c for the columns of bits: one product per column
  int products(V *dst, const V *src, unsigned bits) {
    int rc = 0;
    mask(bits).each([&](int c) {
      if (!rc) rc = h->spmv_local(dst + (long long)c * ld, src + (long long)c * ld, nullptr, st);
    });
    return rc;
  }
  int product_u(unsigned bits) { return products(q, u, bits); } // Q_c = A U_c
  // behind a residual kernel that left r_c . r_c in P_RR0 and b_c . b_c in P_BB of every column
  int first_look() {
    HIPCHK(hipGetLastError());
    if (int rc = part.fetch()) return rc;
    active = 0;
    for (int c = 0; c < ncols; ++c) {
      bb[c] = part.sum(c * P_COUNT + P_BB);
      stop.v[c] = tol * tol * bb[c];
      if (part.sum(c * P_COUNT + P_RR0) > stop.v[c]) active |= 1u << c;
    }
    if (maxiter <= 0) active = 0; // (maxiter = 0 behaves like done)
    ever = active;
    return 0;
  }
  // R = B - A U, rr[0], bb per column by the residual kernel of the plain iteration, and the look
  int first_residual() {
    if (int rc = product_u(all())) return rc;
    hipLaunchKernelGGL((cg_residual_kernel<V, 0, ColumnMask>), dim3(kGrid), dim3(kThreads), 0, st, r, (V *)nullptr, b, (const V *)q, ld, n,
                       part.dev(), (int)P_RR0, 1, (const V *)nullptr, 0LL, mask(all()));
    return first_look();
  }
  bool live() const { return active != 0 && it < maxiter; }
  int window_end() const { return std::min(maxiter, it + look_window_cols(check_every, __builtin_popcount(active))); }
  int look() { // one copy of the counters + synchronisation
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(host_ic.data(), ic, host_ic.size() * sizeof(int), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    for (int c = 0; c < ncols; ++c)
      if (host_ic[(size_t)c * I_COUNT + I_DONE]) active &= ~(1u << c);
    return 0;
  }
  // the true residual of every column of what is returned: one product per column and one residual kernel
  int finish(int *iterations, double *relres) {
    int rc;
    if ((rc = product_u(all()))) return rc;
    hipLaunchKernelGGL((cg_residual_kernel<V, 0, ColumnMask>), dim3(kGrid), dim3(kThreads), 0, st, (V *)nullptr, (V *)nullptr, b, (const V *)q,
                       ld, n, part.dev(), (int)P_RES, 0, (const V *)nullptr, 0LL, mask(all()));
    HIPCHK(hipGetLastError());
    if ((rc = part.fetch())) return rc;
    HIPCHK(hipMemcpy(host_ic.data(), ic, host_ic.size() * sizeof(int), hipMemcpyDeviceToHost));
    for (int c = 0; c < ncols; ++c) {
      const double res2 = part.sum(c * P_COUNT + P_RES);
      if (iterations) iterations[c] = host_ic[(size_t)c * I_COUNT + I_ITER];
      if (relres) relres[c] = bb[c] > 0.0 ? std::sqrt(res2 / bb[c]) : std::sqrt(res2);
    }
    return 0;
  }
};

// cfs_hip_sym_pcg_cols: cg<V, BS> on the columns of U and B.  Set-up of M^-1 once; per iteration one product per
// column the host believes active, then the dot, update and direction kernels once for the block.  iterations, relres:
// ncols entries each (or null).  CFS_HIP_CG_GRAPH is not looked at.
template <typename V, int BS = 0, class Handle>
int cg_cols(Handle *h, void *u_dev, const void *b_dev, long long ld, int ncols, double tol, int maxiter, int check_every,
            int *iterations, double *relres, hipStream_t st) {
  PcgCols<V, Handle> s;
  Precond<V, BS> pre;
  int rc;
  if ((rc = s.begin("pcg_cols", h, u_dev, b_dev, ld, ncols, tol, maxiter, check_every, st)) || (rc = pre.setup(h, s.part.dev(), st)))
    return rc;
  V *u = s.u, *r = s.r, *p = s.p, *q = s.q;
  const long long n = s.n, nb = pre.nb;
  double *part = s.part.dev();
  int *ic = s.ic;
  const V *minv = pre.minv();
  if ((rc = s.product_u(s.all()))) return rc;
  hipLaunchKernelGGL((cg_residual_kernel<V, BS, ColumnMask>), dim3(kGrid), dim3(kThreads), 0, st, r, p, s.b, (const V *)q, ld, n, part,
                     (int)P_RR0, 1, minv, nb, s.mask(s.all()));
  if ((rc = s.first_look()) || (rc = pre.check("pcg_cols", s.part, n))) return rc; // (U has not been touched yet)
  while (s.live()) {
    const int until = s.window_end();
    const ColumnMask cs = s.mask(s.active);
    for (; s.it < until; ++s.it) {
      if ((rc = s.products(q, p, s.active))) return rc;
      hipLaunchKernelGGL((cg_dot_kernel<V, ColumnMask>), dim3(kGrid), dim3(kThreads), 0, st, (const V *)p, (const V *)q, ld, n, part, (int)P_PQ,
                         (const int *)ic, cs);
      hipLaunchKernelGGL((cg_update_kernel<V, BS, num_slot(BS), ColumnMask>), dim3(kGrid), dim3(kThreads), 0, st, u, r, (const V *)p, (const V *)q, ld, n, part,
                         (const int *)ic, s.it, minv, nb, cs);
      hipLaunchKernelGGL((cg_direction_kernel<V, BS, num_slot(BS), ColumnMask>), dim3(kGrid), dim3(kThreads), 0, st, p, (const V *)r, ld, n,
                         (const double *)part, ic, s.it, s.stop, minv, nb, cs);
    }
    if ((rc = s.look())) return rc;
  }
  return s.finish(iterations, relres);
}

} // namespace cfs_solver
