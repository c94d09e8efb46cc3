// cfs_solver_amg.hpp -- an aggregation multigrid V-cycle as the preconditioner of the native PCG
// (cfs_hip_sym_pcg_amg), the cycle alone (cfs_hip_amg_apply) and the set-up of its hierarchy
// (cfs_hip_amg_create_*, cfs_hip_debug_amg_coarsen).
//
// SET-UP (host, fp64).  Per level l with matrix A_l (A_0 = the caller's CSR, entries with col <= row):
//   w_i = 1 / sqrt(a_ii);  B = W A_l W                      (unit diagonal up to rounding)
//   `passes` rounds of pairwise matching on B: the rows in ascending order, an unmatched row i takes the unmatched
//   neighbour j != i with the largest s_ij = |b_ij| / sqrt(b_ii b_jj) > 0 (ties: the smallest j) -- the pair is the next
//   aggregate, a row without a candidate a singleton -- then B <- Q^T B Q, every coarse entry the fp64 sum of its
//   contributions in ascending (row, column) order (the lower triangle is summed, the upper one is its mirror)
//   agg_l = the composition of the rounds;  P_l = W Q_1 .. Q_p;  A_{l+1} = the last B = P_l^T A_l P_l
// The weights make the hierarchy invariant under a symmetric scaling of A: B does not see it.  A_{l+1} is rounded to the
// value type V before it is coarsened further, so every level is the Galerkin product of the matrix its handle holds.
// The hierarchy ends with a DENSE level (n_l <= coarse_max; or the coarsening stalled, n_{l+1} > 0.9 n_l, or level 16
// is reached, at n_l <= 1024), whose inverse -- Cholesky in fp64, solves, symmetrised, rounded to V -- is kept as an
// n_L x n_L array, or else with a SMOOTHER-ONLY level: a stalled hierarchy degrades to the Chebyshev preconditioner.
// Levels 1 .. L are handles of the library's own create path (no measured alternatives; deterministic when the fine
// handle is); level 0 is the caller's handle.  Per non-dense level: dinv as cg_dinv_kernel stores it, the bound
// lmax = 1.1 x cheb_power (Jacobi, 16 steps, the fixed start vector), lmin = lmax / ratio, the coefficient pairs.
//
// ONE CYCLE z = M^-1 r, S_l the level's Chebyshev polynomial of degree m in D^-1 A_l (cfs_solver_cheb.hpp).  Amg::cycle
// and every vector kernel of it are templates over the set of columns they work on (OneColumn or ColumnMask,
// cfs_solver.hpp): written once, for one column here and for a block of columns under THE COLUMNS OF A CYCLE below.
//   dense level:          z = (V)(A_L^-1 r)                                   amg_dense_kernel               1 launch
//   smoother-only level:  z = S_l r                                           cheb_start_kernel + cheb_chain 1 + 3 (m - 1)
//   otherwise:            z = S_l r                                                                          1 + 3 (m - 1)
//                         t = A_l z;  rc_I = (V)(sum_{i in I} w_i (r_i - t_i))  product + amg_restrict_kernel  3
//                         ec = cycle(l + 1, rc)
//                         z_i = (V)(z_i + w_i ec_agg(i))                        amg_prolong_kernel             1
//                         t = A_l z;  d = (V)((1/theta) D^-1 (r - t));  z = (V)(z + d)
//                                                                             product + amg_restart_kernel   3
//                         the m - 1 steps of cheb_chain, unchanged                                           3 (m - 1)
// 8 + 6 (m - 1) launches per multigrid level.  cheb_chain forms r - A z_j from the full iterate, so the Chebyshev
// iteration from a nonzero start is the same recurrence and post-smoothing needs only the start kernel that takes t.
// Pre- and post-smoother are the same symmetric polynomial and restriction is the transpose of prolongation with the
// same stored w: M^-1 is symmetric, and positive definite while every level's spectrum of D^-1 A_l lies in
// (0, lmin + lmax) -- the margin of cfs_hip_sym_pcg_cheb, here (1 + 1 / ratio) x 1.1 = 1.375 x the estimate at ratio 4.
//
// The outer PCG (cg_amg) is cg_cheb with the chain replaced by the cycle:
//   tile kernel + fold   q = A p
//   cg_dot_kernel        pq = p . q
//   cg_update_kernel<V, 0, P_RZ0>      u += (rz/pq) p;  r -= (rz/pq) q;  rr' = r . r
//   the cycle            z = M^-1 r
//   cg_dot_kernel        rz' = r . z of the stored r and the stored final z
//   cg_direction_kernel<V, 0, P_RZ0>   p = z + (rz'/rz) p, z in the place of r;  iteration count;  converged?
//                                      (rr' <= tol^2 b.b)
// (the kernels of cfs_solver.hpp in their OneColumn instantiations; pcg_cols launches the ColumnMask ones)
// 6 launches and the cycle; a cycle exceeds what may be enqueued between two host looks, so the host looks at the
// convergence flag after every iteration.
//
// Rounding: vectors are stored in V; every update is computed in fp64 from the stored operands and rounded once; the
// restriction sums its members in ascending order, the dense rows in a fixed lane order; all scalars are the
// fixed-order partial sums of cfs_solver.hpp.  No atomics: on a deterministic handle the solve is bit-reproducible.
//
// REFRESH (cfs_hip_amg_create_refreshable_*, cfs_hip_amg_update_values_*): the arithmetic of the set-up with the matching
// q of every round FROZEN, in the same order of operations, on the device over lists recorded at create --
//   level 0:   a_k = the caller's values summed as amg_lower sums them         amg_gather_sum_kernel over amg_lower_lists
//   per level: w_i = 1 / sqrt(a_ii) in fp64 on the device (correctly rounded division and sqrt: the bits of the host's;
//              the test with unchanged values is the judge, and it found no differing bit), (V)w_i for the transfers,
//              the entries that are not finite and > 0 counted                 amg_weight_kernel
//              b_k = (w_row(k) a_k) w_col(k), the operand order of amg_mirror  amg_scale_kernel
//              per round, every entry of Q^T B Q with J <= I as the sum of its contributions in the order amg_galerkin
//              adds them; the last round writes (V)s and (double)(V)s           amg_gather_sum_kernel
//              the pour into the next level's handle (update_values), then dinv, cheb_power and the pairs again
//   dense level: its values to the host, amg_dense_inverse, the inverse back.
// If a fresh set-up would choose the same aggregates the result equals it in every bit of w, the level matrices and the
// inverse.  Kept between calls (map_bytes): the lists, row / column / diagonal position per stored entry of a level, every
// level's values in V on the device (level_matrix() reads them back at its first call after a refresh), two fp64 arrays
// of the longest level (the scaling is in place, the rounds go to and fro) and the fp64 weights.  Level 0 is the caller's
// handle, poured by the caller: follow_fine().
//
// THE LOCALLY DOMINANT MATCHING (cfs_hip_amg_create_dominant_*, amg_match_dominant) replaces the sweep in row order by
// synchronous rounds over a total order of the edges (strength, parity of the smaller endpoint, a hash, the indices):
// parallel by definition and deterministic, everything else of a level unchanged.  With it the whole set-up runs ON THE
// DEVICE (cfs_hip_amg_create_device_*, cfs_solver_amg_setup.hpp) and gives the host's hierarchy in every bit; build()
// below is one loop over the levels for both, the host keeping what it kept: the level handles' create path, the dense
// inverse and the power method's look.
//
// THE NODE-BLOCK FORM (cfs_hip_amg_create_block_*, Amg<V, BS> with BS = 2, 3, 4 or 6; amg_coarsen_block) treats the
// m = n / BS mesh nodes as the units of a level, for multi-dof matrices whose couplings inside a node are as strong as
// the diagonal.  Per level, with D_i the BS x BS diagonal block of A_l (both triangles):
//   W_i = D_i^-1/2, the SYMMETRIC root: D_i = Q diag(ev) Q^T by symeig (cyclic Jacobi, fp64), W_i = Q diag(1/sqrt(ev)) Q^T,
//         its lower triangle computed (the sum over the eigenpairs ascending) and mirrored; an eigenvalue that is not
//         finite and > 0 refuses the block.  The symmetric root keeps the node's frame -- on H (L x I) H it returns L x I --
//         where a Cholesky factor would leave a rotation in every off-diagonal block
//   B = W A_l W, node block by node block: B_ij = (W_i A_ij) W_j for j <= i, every sum over the inner index ascending,
//         a coupled pair of nodes stored as a full block (zeros included); the upper triangle is the mirror
//   `passes` rounds of pairwise matching on the NODE graph with n_ij = ||B_ij||_F (the squares added row-major, j <= i,
//         the other triangle mirrored): amg_match / amg_match_dominant unchanged, so s_ij = n_ij / sqrt(n_ii n_jj);
//         then B <- Q^T B Q by amg_galerkin with q[i BS + c] = q_node[i] BS + c
//   agg_l[i BS + c] = agg_node[i] BS + c;  P_l = W Q_1 .. Q_p;  A_{l+1} = the last B, again a node-block matrix
// Everything else of a level is the scalar form's.  The hierarchy is host-built and not refreshable.  On the device W is
// kept the way the block-Jacobi inverse is -- packed lower triangle, word t = i (i + 1) / 2 + j of node k at
// w[t m + k], read by block_load -- and the aggregate lists and agg hold NODES.  The cycle is the one above, the BS >= 2
// branch of the same kernels, with
//   the smoother in M^-1 A_l, M = blockdiag(A_l):  Precond<V, BS>, cheb_power<V, BS>, cheb_start_kernel<V, BS>, cheb_chain<V, BS>
//   rc_I = (V)(sum_{i in I, ascending} W_i (r_i - t_i))                          amg_restrict_kernel<V, BS>
//   z_i = (V)(z_i + W_i ec_I)                                                    amg_prolong_kernel<V, BS>
//   d_i = (V)((1/theta) M_i^-1 (r_i - t_i));  z_i = (V)(z_i + d_i)               amg_restart_kernel<V, BS>
// one thread per node, the same 8 + 6 (m - 1) launches; W_i is symmetric and restriction the transpose of prolongation,
// so M^-1 stays symmetric, and nothing is atomic.
//
// THE COLUMNS OF A CYCLE.  cfs_hip_amg_apply_cols and cfs_hip_sym_lobpcg_amg run the cycle above on the columns
// c < ncols <= 16 of a block whose bit is set in a mask, Z_c = M^-1 R_c, for the W block of LOBPCG: cycle() with a
// ColumnMask where cfs_hip_amg_apply and cfs_hip_sym_pcg_amg pass OneColumn.  Every vector kernel is launched ONCE for
// the columns, so a level costs 4 + 2 (m - 1) vector-kernel launches for any ncols, where ncols one-column cycles cost
// ncols times that; the products stay one spmv_local per column at each place.  What a row, node or aggregate reads of
// the level -- dinv or the packed inverse block, the packed W, agg, the aggregate list, a row of the dense inverse -- is
// loaded once and used for all columns of a chunk: the whole block in the element-wise kernels (the columns are the
// inner loop, the level's words stay in registers), chunks of 8 / 4 / 2 columns (BS = 1 / 2, 3, 4 / 6) in the
// restriction, whose fp64 accumulators are per column, and of 8 in the dense kernel.  A column whose bit is clear is
// neither read nor written.  For OneColumn the loops, the mask tests and the c ld offsets fold away at compile time.
// There is one body per kernel, but its OneColumn and ColumnMask instantiations are compiled separately, and neither
// switches contraction off: that column c of a block has the bits of the one-column cycle on R_c alone (on a
// deterministic handle) still rests on the compiler contracting both alike -- now from literally the same source text,
// the same casts, parentheses and order of sums -- and test B1 of tests/test_gpu_amg_apply_cols.py remains the judge.
// The work vectors differ (Amg::work): one column uses the level's d, t, r, z that build() allocates; a block uses cd, ct
// on a level that smooths and cr, cz below level 0, columns of n_l rounded up to 16 bytes, allocated at the first blocked
// call of a width, kept, and made again only for a wider call (reserve_cols).  Nothing is allocated for blocks before.
#pragma once

#include <algorithm>
#include <chrono>
#include <climits>
#include <memory>
#include <utility>

// what cfs_hip_amg_t points to
struct cfs_hip_amg_s {
  int value_bytes = 8;
  cfs_hip_sym_s *fine = nullptr; // the handle the hierarchy was created on (level 0; not owned)
  virtual ~cfs_hip_amg_s() {}
  virtual int info(cfs_hip_amg_info_t *out) = 0;
  virtual int level_aggregates(int level, int *agg, void *w) = 0;
  virtual int level_matrix(int level, int *rowptr, int *colind, void *values) = 0;
  virtual int coarse_inverse(void *inv) = 0;
  virtual int apply(void *z_dev, const void *r_dev, hipStream_t st) = 0;
  virtual int apply_cols(void *z_dev, const void *r_dev, long long ld, int ncols, unsigned active, hipStream_t st) = 0;
  // (hb: the B of the pencil form cfs_hip_sym_lobpcg_gen_amg, with its counter b_products; nullptr: A x = lambda x)
  virtual int lobpcg(cfs_hip_sym_s *hb, int k, double tol, double scale, int maxiter, int debug_iters, const void *x0_dev, long long ld0,
                     double *eigenvalues, void *vectors_dev, long long ld, double *residuals, int *nconv, int *iterations, int *products,
                     int *b_products, hipStream_t st) = 0;
  virtual bool is_stale() const = 0;              // the last refresh failed
  virtual long long column_cycles() const = 0;    // cycles applied to columns of blocks, since create
  virtual int pcg(void *u_dev, const void *b_dev, double tol, int maxiter, int *iterations, double *relres, hipStream_t st) = 0;
  virtual int pcg_cols(void *u_dev, const void *b_dev, long long ld, int ncols, double tol, int maxiter, int *iterations, double *relres,
                       hipStream_t st) = 0;
  virtual int update_check(long long nnz) = 0;
  virtual int update_values(const void *values_dev, long long nnz, hipStream_t st) = 0;
  virtual int refresh_info(long long *map_bytes, int *refreshes, double *last_seconds, double *split) = 0;
  virtual int setup_info(int *matching, int *on_device, int *rounds, double *seconds, long long *scratch_bytes) = 0;
  virtual int block() const = 0; // rows per node: 1, or the BS of a node-block hierarchy
  virtual int level_node_weights(int level, void *W) = 0;
};

namespace cfs_solver {

// ---- set-up on the host ----------------------------------------------------------------------------
// a CSR in fp64 with 64-bit row pointers: the lower triangle + diagonal of a level, or both triangles of B
struct AmgCsr {
  int n = 0;
  std::vector<long long> rp;
  std::vector<int> ci;
  std::vector<double> va;
  long long nnz() const { return rp.empty() ? 0 : rp.back(); }
};

// the entries with col <= row of the caller's CSR, columns ascending, duplicates summed in the order given
template <typename T> inline void amg_lower(int n, const int *rowptr, const int *colind, const T *values, AmgCsr &out) {
  out.n = n;
  out.rp.assign((size_t)n + 1, 0);
  out.ci.clear();
  out.va.clear();
  std::vector<std::pair<int, double>> row;
  for (int i = 0; i < n; ++i) {
    row.clear();
    bool sorted = true;
    for (int k = rowptr[i]; k < rowptr[i + 1]; ++k) {
      const int j = colind[k];
      if (j < 0 || j > i) continue;
      if (!row.empty() && row.back().first >= j) sorted = false;
      row.emplace_back(j, (double)values[k]);
    }
    if (!sorted) std::stable_sort(row.begin(), row.end(), [](const auto &a, const auto &b) { return a.first < b.first; });
    for (size_t k = 0; k < row.size(); ++k) {
      if (k > 0 && row[k].first == row[k - 1].first) {
        out.va.back() += row[k].second;
      } else {
        out.ci.push_back(row[k].first);
        out.va.push_back(row[k].second);
      }
    }
    out.rp[(size_t)i + 1] = (long long)out.ci.size();
  }
}

// both triangles of a symmetric matrix from its lower triangle + diagonal, columns ascending; scale: the entry
// (i, j) becomes (scale_i a_ij) scale_j, computed once and mirrored (nullptr: the entries as they are).  from (when
// given): the position in `low` every entry of `full` was taken from
inline void amg_mirror(const AmgCsr &low, const double *scale, AmgCsr &full, std::vector<int> *from = nullptr) {
  const int n = low.n;
  full.n = n;
  full.rp.assign((size_t)n + 1, 0);
  for (int i = 0; i < n; ++i)
    for (long long k = low.rp[i]; k < low.rp[i + 1]; ++k) {
      full.rp[(size_t)i + 1] += 1;
      if (low.ci[k] != i) full.rp[(size_t)low.ci[k] + 1] += 1;
    }
  for (int i = 0; i < n; ++i) full.rp[(size_t)i + 1] += full.rp[i];
  full.ci.assign((size_t)full.rp[n], 0);
  full.va.assign((size_t)full.rp[n], 0.0);
  if (from) from->assign((size_t)full.rp[n], 0);
  std::vector<long long> pos(full.rp.begin(), full.rp.end() - 1);
  auto value = [&](int i, long long k) { return scale ? (scale[i] * low.va[k]) * scale[low.ci[k]] : low.va[k]; };
  for (int i = 0; i < n; ++i) // the columns up to the diagonal ...
    for (long long k = low.rp[i]; k < low.rp[i + 1]; ++k) {
      full.ci[pos[i]] = low.ci[k];
      if (from) (*from)[pos[i]] = (int)k;
      full.va[pos[i]++] = value(i, k);
    }
  for (int i = 0; i < n; ++i) // ... then those behind it, rows ascending
    for (long long k = low.rp[i]; k < low.rp[i + 1]; ++k) {
      const int j = low.ci[k];
      if (j == i) continue;
      full.ci[pos[j]] = i;
      if (from) (*from)[pos[j]] = (int)k;
      full.va[pos[j]++] = value(i, k);
    }
}

// the diagonal of a lower triangle + diagonal; returns the number of entries that are missing, zero, negative or not finite
inline long long amg_diagonal(const AmgCsr &low, std::vector<double> &diag) {
  long long bad = 0;
  diag.assign((size_t)low.n, 0.0);
  for (int i = 0; i < low.n; ++i) {
    const long long e = low.rp[(size_t)i + 1];
    const double a = (e > low.rp[i] && low.ci[e - 1] == i) ? low.va[e - 1] : 0.0;
    diag[i] = a;
    // (!(a > 0): a NaN counts too)
    if (!(a > 0.0) || a * 0.0 != 0.0) bad += 1;
  }
  return bad;
}

// one round of pairwise matching on B (both triangles): q[i] = the aggregate of row i, numbered in order of creation
inline int amg_match(const AmgCsr &B, std::vector<int> &q) {
  const int n = B.n;
  std::vector<double> diag((size_t)n, 0.0);
  for (int i = 0; i < n; ++i)
    for (long long k = B.rp[i]; k < B.rp[i + 1]; ++k)
      if (B.ci[k] == i) diag[i] = B.va[k];
  q.assign((size_t)n, -1);
  int nc = 0;
  for (int i = 0; i < n; ++i) {
    if (q[i] >= 0) continue;
    int best = -1;
    double sbest = 0.0;
    for (long long k = B.rp[i]; k < B.rp[i + 1]; ++k) {
      const int j = B.ci[k];
      if (j == i || q[j] >= 0) continue;
      const double s = std::fabs(B.va[k]) / std::sqrt(diag[i] * diag[j]);
      if (s > sbest) best = j, sbest = s; // (columns ascending and a strict comparison: a tie keeps the smallest j)
    }
    q[i] = nc;
    if (best >= 0) q[best] = nc;
    ++nc;
  }
  return nc;
}

// ---- the locally dominant matching (CFS_HIP_AMG_MATCHING_DOMINANT): parallel by definition, host and device ----
// the 32-bit mix of an edge's endpoints, lo < hi: it decides between edges of equal strength and equal parity
__host__ __device__ inline unsigned amg_edge_hash(unsigned lo, unsigned hi) {
  unsigned x = (lo * 0x9E3779B1u) ^ (hi * 0x85EBCA77u);
  x ^= x >> 15;
  x *= 0x2C1B3C6Du;
  x ^= x >> 12;
  x *= 0x297A2D39u;
  x ^= x >> 15;
  return x;
}

// the total order of the candidate edges: does (i, j1) of strength s1 come before (i, j2) of strength s2?  Larger s,
// then an even smaller endpoint, then the smaller hash, then the smaller (lo, hi)
__host__ __device__ inline bool amg_edge_before(double s1, int i, int j1, double s2, int j2) {
  if (s1 != s2) return s1 > s2;
  const int lo1 = i < j1 ? i : j1, hi1 = i < j1 ? j1 : i, lo2 = i < j2 ? i : j2, hi2 = i < j2 ? j2 : i;
  if ((lo1 & 1) != (lo2 & 1)) return !(lo1 & 1);
  const unsigned h1 = amg_edge_hash((unsigned)lo1, (unsigned)hi1), h2 = amg_edge_hash((unsigned)lo2, (unsigned)hi2);
  if (h1 != h2) return h1 < h2;
  return lo1 != lo2 ? lo1 < lo2 : hi1 < hi2;
}

// one round of pairwise matching on B (both triangles) by synchronous rounds: every free row points to its first free
// neighbour in the total order, computed from the state at the start of the round; rows that point at each other pair.
// The rounds end with one that forms no pair, or after CFS_HIP_AMG_MATCH_ROUNDS; *rounds = the rounds run.  q[i] = the
// aggregate of row i, numbered by smallest member
inline int amg_match_dominant(const AmgCsr &B, std::vector<int> &q, int *rounds) {
  const int n = B.n;
  std::vector<double> diag((size_t)n, 0.0);
  for (int i = 0; i < n; ++i)
    for (long long k = B.rp[i]; k < B.rp[i + 1]; ++k)
      if (B.ci[k] == i) diag[i] = B.va[k];
  std::vector<int> mate((size_t)n, -1), to((size_t)n, -1);
  int r = 0;
  while (r < CFS_HIP_AMG_MATCH_ROUNDS) {
    ++r;
    for (int i = 0; i < n; ++i) {
      int best = -1;
      double sbest = 0.0;
      if (mate[i] < 0)
        for (long long k = B.rp[i]; k < B.rp[i + 1]; ++k) {
          const int j = B.ci[k];
          if (j == i || mate[j] >= 0) continue;
          const double s = std::fabs(B.va[k]) / std::sqrt(diag[i] * diag[j]);
          if (!(s > 0.0)) continue;
          if (best < 0 || amg_edge_before(s, i, j, sbest, best)) best = j, sbest = s;
        }
      to[i] = best;
    }
    int made = 0;
    for (int i = 0; i < n; ++i) {
      const int j = to[i];
      if (j >= 0 && to[j] == i) mate[i] = j, made += i < j;
    }
    if (!made) break;
  }
  if (rounds) *rounds = r;
  q.assign((size_t)n, -1);
  int nc = 0;
  for (int i = 0; i < n; ++i) {
    if (q[i] >= 0) continue;
    q[i] = nc;
    if (mate[i] >= 0) q[mate[i]] = nc;
    ++nc;
  }
  return nc;
}

// what a refresh evaluates (cfs_hip_amg_update_values_*): output entry e is the sum of src[idx[k]], k = ptr[e] ..
// ptr[e + 1] - 1, added in that order.  32-bit: a list that would not fit sets `overflow`
struct AmgList {
  std::vector<int> ptr, idx;
  bool overflow = false;
  long long entries() const { return ptr.empty() ? 0 : (long long)ptr.size() - 1; }
};

// the lists of amg_lower: per entry it writes, the positions in the caller's values[] it sums, in its order
inline void amg_lower_lists(int n, const int *rowptr, const int *colind, AmgList &out) {
  out.ptr.assign(1, 0);
  out.idx.clear();
  std::vector<std::pair<int, int>> row;
  for (int i = 0; i < n; ++i) {
    row.clear();
    bool sorted = true;
    for (int k = rowptr[i]; k < rowptr[i + 1]; ++k) {
      const int j = colind[k];
      if (j < 0 || j > i) continue;
      if (!row.empty() && row.back().first >= j) sorted = false;
      row.emplace_back(j, k);
    }
    if (!sorted) std::stable_sort(row.begin(), row.end(), [](const auto &a, const auto &b) { return a.first < b.first; });
    for (size_t k = 0; k < row.size(); ++k) {
      out.idx.push_back(row[k].second);
      if (k > 0 && row[k].first == row[k - 1].first)
        out.ptr.back() = (int)out.idx.size();
      else
        out.ptr.push_back((int)out.idx.size());
    }
  }
}

// out[e] = the sum of list e over src, on the host in the order amg_gather_sum_kernel adds
template <typename S> inline void amg_eval_list(const AmgList &li, const S *src, double *out) {
  for (long long e = 0; e < li.entries(); ++e) {
    double s = (double)src[li.idx[li.ptr[e]]];
    for (int k = li.ptr[e] + 1; k < li.ptr[e + 1]; ++k) s += (double)src[li.idx[k]];
    out[e] = s;
  }
}

// the lower triangle + diagonal of Q^T B Q: every entry the sum of its contributions in ascending (row, column) order.
// from + rec (when given): from[k] = where entry k of B sits in the lower-triangle array B was mirrored from; rec <- per
// entry of `out`, as it stands after the sort of its row, those positions in the order the sum below adds them
inline void amg_galerkin(const AmgCsr &B, const std::vector<int> &q, int nc, AmgCsr &out, const std::vector<int> *from = nullptr,
                         AmgList *rec = nullptr) {
  const int n = B.n;
  std::vector<int> first((size_t)nc, -1), second((size_t)nc, -1);
  for (int i = 0; i < n; ++i) (first[q[i]] < 0 ? first[q[i]] : second[q[i]]) = i;
  out.n = nc;
  out.rp.assign((size_t)nc + 1, 0);
  out.ci.clear();
  out.va.clear();
  std::vector<long long> where((size_t)nc, -1);
  std::vector<std::pair<int, double>> row;
  std::vector<std::pair<int, int>> added; // rec: (entry of the row before the sort, position in the source array)
  std::vector<int> cnt;
  if (rec) rec->ptr.assign(1, 0), rec->idx.clear(), rec->overflow = false;
  for (int I = 0; I < nc; ++I) {
    const long long start = (long long)out.ci.size();
    added.clear();
    for (int m : {first[I], second[I]}) {
      if (m < 0) continue;
      for (long long k = B.rp[m]; k < B.rp[m + 1]; ++k) {
        const int J = q[B.ci[k]];
        if (J > I) continue;
        if (where[J] < start) {
          where[J] = (long long)out.ci.size();
          out.ci.push_back(J);
          out.va.push_back(B.va[k]);
        } else {
          out.va[where[J]] += B.va[k];
        }
        if (rec) added.emplace_back((int)(where[J] - start), (*from)[k]);
      }
    }
    const long long end = (long long)out.ci.size();
    row.clear();
    for (long long k = start; k < end; ++k) row.emplace_back(out.ci[k], out.va[k]);
    std::sort(row.begin(), row.end(), [](const auto &a, const auto &b) { return a.first < b.first; });
    if (rec) { // the lists follow their entries through the sort; inside a list the order of the sum stays
      const size_t len = (size_t)(end - start), base = rec->idx.size();
      if (base + added.size() > (size_t)INT_MAX) {
        rec->overflow = true;
        rec = nullptr;
      } else {
        cnt.assign(len + 1, 0);
        for (const auto &c : added) cnt[(size_t)c.first + 1] += 1;
        for (size_t k = 0; k < len; ++k) cnt[k + 1] += cnt[k];
        std::vector<int> at(len); // where the list of the entry that was at `old` before the sort begins
        for (size_t k = 0; k < len; ++k) {
          const size_t old = (size_t)(where[row[k].first] - start);
          at[old] = (int)rec->idx.size();
          rec->idx.resize(rec->idx.size() + (size_t)(cnt[old + 1] - cnt[old]));
          rec->ptr.push_back((int)rec->idx.size());
        }
        for (const auto &c : added) rec->idx[(size_t)at[c.first]++] = c.second;
      }
    }
    for (long long k = start; k < end; ++k) out.ci[k] = row[k - start].first, out.va[k] = row[k - start].second, where[out.ci[k]] = -1;
    out.rp[(size_t)I + 1] = end;
  }
}

// one level with its matchings frozen, as a refresh evaluates it: w_i = 1 / sqrt(a[diag[i]]), b_k = (w_row[k] a_k) w_col[k]
// over the lower-triangle array a (col: the pattern's colind), then rounds[p] over the array of the round before
struct AmgFrozen {
  std::vector<int> diag, row;
  std::vector<AmgList> rounds;
  bool overflow() const {
    for (const AmgList &r : rounds)
      if (r.overflow) return true;
    return false;
  }
};

// the frozen level for other values of the same pattern, on the host: a (the lower-triangle array) -> w and the values
// of the last round, every operation in the order of the kernels (which is that of amg_coarsen)
inline void amg_eval_frozen(const AmgFrozen &f, const std::vector<int> &col, const double *a, std::vector<double> &w, std::vector<double> &out) {
  const size_t n = f.diag.size(), m = f.row.size();
  w.resize(n);
  for (size_t i = 0; i < n; ++i) w[i] = 1.0 / std::sqrt(a[f.diag[i]]);
  std::vector<double> src(m), dst;
  for (size_t k = 0; k < m; ++k) src[k] = (w[f.row[k]] * a[k]) * w[col[k]];
  for (const AmgList &r : f.rounds) {
    dst.resize((size_t)r.entries());
    amg_eval_list(r, src.data(), dst.data());
    src.swap(dst);
  }
  out = std::move(src);
}

// one level: agg, w and the lower triangle + diagonal of A_{l+1} from that of A_l.  *bad: diagonal entries that are not positive.
// rec (when given): the level's lists, for a refresh.  matching: CFS_HIP_AMG_MATCHING_*; rounds (when given, dominant
// only): the rounds every pass ran
inline int amg_coarsen(const AmgCsr &low, int passes, std::vector<int> &agg, std::vector<double> &w, AmgCsr &coarse, long long *bad,
                       AmgFrozen *rec = nullptr, int matching = CFS_HIP_AMG_MATCHING_GREEDY, int *rounds = nullptr) {
  const int n = low.n;
  std::vector<double> diag;
  *bad = amg_diagonal(low, diag);
  if (*bad) return -1;
  w.resize((size_t)n);
  for (int i = 0; i < n; ++i) w[i] = 1.0 / std::sqrt(diag[i]);
  AmgCsr B, next;
  std::vector<int> from;
  if (rec) {
    rec->diag.resize((size_t)n);
    rec->row.resize((size_t)low.nnz());
    for (int i = 0; i < n; ++i) {
      rec->diag[i] = (int)low.rp[(size_t)i + 1] - 1; // (amg_diagonal found it there)
      for (long long k = low.rp[i]; k < low.rp[(size_t)i + 1]; ++k) rec->row[k] = i;
    }
    rec->rounds.assign((size_t)passes, AmgList());
  }
  amg_mirror(low, w.data(), B, rec ? &from : nullptr);
  agg.resize((size_t)n);
  for (int i = 0; i < n; ++i) agg[i] = i;
  std::vector<int> q;
  for (int p = 0; p < passes; ++p) {
    const int nc = matching == CFS_HIP_AMG_MATCHING_DOMINANT ? amg_match_dominant(B, q, rounds ? rounds + p : nullptr) : amg_match(B, q);
    amg_galerkin(B, q, nc, next, rec ? &from : nullptr, rec ? &rec->rounds[p] : nullptr);
    for (int i = 0; i < n; ++i) agg[i] = q[agg[i]];
    if (p + 1 < passes) amg_mirror(next, nullptr, B, rec ? &from : nullptr);
  }
  coarse = std::move(next);
  return 0;
}

// ---- the node-block form of a level (see THE NODE-BLOCK FORM in the header comment) ------------------
// the node blocks of row i of a lower triangle + diagonal whose n is a multiple of bs: cols <- the node columns j <= i,
// ascending; blk <- per column the bs x bs block, row-major, zeros where nothing is stored, the diagonal block mirrored
// into both triangles.  slot: m entries of -1, restored on return
inline void amg_node_row(const AmgCsr &low, int bs, int i, std::vector<int> &slot, std::vector<int> &cols, std::vector<double> &blk) {
  const size_t bb = (size_t)bs * bs;
  std::vector<int> seen;
  std::vector<double> raw;
  for (int c = 0; c < bs; ++c) {
    const int row = i * bs + c;
    for (long long k = low.rp[row]; k < low.rp[(size_t)row + 1]; ++k) {
      const int j = low.ci[k] / bs, d = low.ci[k] % bs;
      if (slot[j] < 0) {
        slot[j] = (int)seen.size();
        seen.push_back(j);
        raw.resize(raw.size() + bb, 0.0);
      }
      raw[(size_t)slot[j] * bb + (size_t)c * bs + d] = low.va[k];
    }
  }
  cols = seen;
  std::sort(cols.begin(), cols.end());
  blk.resize(raw.size());
  for (size_t s = 0; s < cols.size(); ++s) std::copy_n(&raw[(size_t)slot[cols[s]] * bb], bb, &blk[s * bb]);
  if (!cols.empty() && cols.back() == i) {
    double *dg = &blk[(cols.size() - 1) * bb];
    for (int c = 0; c < bs; ++c)
      for (int d = 0; d < c; ++d) dg[(size_t)d * bs + c] = dg[(size_t)c * bs + d];
  }
  for (int j : seen) slot[j] = -1;
}

// W_i = D_i^-1/2 of every node block, m x bs x bs row-major, exactly symmetric; returns the blocks with an eigenvalue
// that is not finite and > 0 (their W_i is left zero)
inline long long amg_node_weights(const AmgCsr &low, int bs, std::vector<double> &W) {
  const int m = low.n / bs;
  const size_t bb = (size_t)bs * bs;
  W.assign((size_t)m * bb, 0.0);
  std::vector<int> slot((size_t)m, -1), cols;
  std::vector<double> blk, ev((size_t)bs), Q(bb), dz(bb, 0.0);
  long long bad = 0;
  for (int i = 0; i < m; ++i) {
    amg_node_row(low, bs, i, slot, cols, blk);
    const double *D = !cols.empty() && cols.back() == i ? &blk[(cols.size() - 1) * bb] : dz.data();
    bool ok = true;
    for (size_t k = 0; k < bb; ++k) ok = ok && D[k] * 0.0 == 0.0; // (symeig is given finite numbers only)
    if (ok) ok = symeig(bs, D, ev.data(), Q.data()) >= 0;
    for (int k = 0; ok && k < bs; ++k) ok = ev[k] > 0.0 && ev[k] * 0.0 == 0.0;
    if (!ok) {
      bad += 1;
      continue;
    }
    double *Wi = &W[(size_t)i * bb];
    for (int k = 0; k < bs; ++k) ev[k] = 1.0 / std::sqrt(ev[k]);
    for (int c = 0; c < bs; ++c)
      for (int d = 0; d <= c; ++d) {
        double s = 0.0;
        for (int k = 0; k < bs; ++k) s += (Q[(size_t)c * bs + k] * ev[k]) * Q[(size_t)d * bs + k];
        Wi[(size_t)c * bs + d] = Wi[(size_t)d * bs + c] = s;
      }
  }
  return bad;
}

// the lower triangle + diagonal of B = W A W: B_ij = (W_i A_ij) W_j for the node pairs j <= i of `low`, full blocks
inline void amg_scale_block(const AmgCsr &low, int bs, const std::vector<double> &W, AmgCsr &out) {
  const int m = low.n / bs;
  const size_t bb = (size_t)bs * bs;
  std::vector<int> slot((size_t)m, -1), cols;
  std::vector<double> blk, T(bb), B;
  out.n = low.n;
  out.rp.assign((size_t)low.n + 1, 0);
  out.ci.clear();
  out.va.clear();
  for (int i = 0; i < m; ++i) {
    amg_node_row(low, bs, i, slot, cols, blk);
    B.resize(blk.size());
    const double *Wi = &W[(size_t)i * bb];
    for (size_t s = 0; s < cols.size(); ++s) {
      const double *A = &blk[s * bb], *Wj = &W[(size_t)cols[s] * bb];
      for (int c = 0; c < bs; ++c)
        for (int d = 0; d < bs; ++d) {
          double v = 0.0;
          for (int k = 0; k < bs; ++k) v += Wi[(size_t)c * bs + k] * A[(size_t)k * bs + d];
          T[(size_t)c * bs + d] = v;
        }
      for (int c = 0; c < bs; ++c)
        for (int d = 0; d < bs; ++d) {
          double v = 0.0;
          for (int k = 0; k < bs; ++k) v += T[(size_t)c * bs + k] * Wj[(size_t)k * bs + d];
          B[s * bb + (size_t)c * bs + d] = v;
        }
    }
    for (int c = 0; c < bs; ++c) {
      for (size_t s = 0; s < cols.size(); ++s)
        for (int d = 0; d < bs && cols[s] * bs + d <= i * bs + c; ++d) {
          out.ci.push_back(cols[s] * bs + d);
          out.va.push_back(B[s * bb + (size_t)c * bs + d]);
        }
      out.rp[(size_t)i * bs + c + 1] = (long long)out.ci.size();
    }
  }
}

// the node graph of a lower triangle + diagonal, both triangles: entry (i, j) = ||B_ij||_F, computed for j <= i (the
// squares added row-major over the full block) and mirrored -- what amg_match and amg_match_dominant are given
inline void amg_node_graph(const AmgCsr &low, int bs, AmgCsr &graph) {
  const int m = low.n / bs;
  const size_t bb = (size_t)bs * bs;
  std::vector<int> slot((size_t)m, -1), cols;
  std::vector<double> blk;
  AmgCsr g;
  g.n = m;
  g.rp.assign((size_t)m + 1, 0);
  for (int i = 0; i < m; ++i) {
    amg_node_row(low, bs, i, slot, cols, blk);
    for (size_t s = 0; s < cols.size(); ++s) {
      double f = 0.0;
      for (size_t k = 0; k < bb; ++k) f += blk[s * bb + k] * blk[s * bb + k];
      g.ci.push_back(cols[s]);
      g.va.push_back(std::sqrt(f));
    }
    g.rp[(size_t)i + 1] = (long long)g.ci.size();
  }
  amg_mirror(g, nullptr, graph);
}

// one level of the node-block form: agg (per unknown), W (m x bs x bs) and the lower triangle + diagonal of A_{l+1} from
// that of A_l, low.n a multiple of bs.  *bad: node blocks that are not positive definite (then -1 is returned)
inline int amg_coarsen_block(const AmgCsr &low, int bs, int passes, std::vector<int> &agg, std::vector<double> &W, AmgCsr &coarse,
                             long long *bad, int matching = CFS_HIP_AMG_MATCHING_GREEDY, int *rounds = nullptr) {
  const int n = low.n, m = n / bs;
  *bad = amg_node_weights(low, bs, W);
  if (*bad) return -1;
  AmgCsr cur, B, graph, next;
  amg_scale_block(low, bs, W, cur);
  std::vector<int> nagg((size_t)m), qn, q;
  for (int i = 0; i < m; ++i) nagg[i] = i;
  for (int p = 0; p < passes; ++p) {
    amg_node_graph(cur, bs, graph);
    const int nc = matching == CFS_HIP_AMG_MATCHING_DOMINANT ? amg_match_dominant(graph, qn, rounds ? rounds + p : nullptr) : amg_match(graph, qn);
    q.resize((size_t)cur.n);
    for (int i = 0; i < cur.n / bs; ++i)
      for (int c = 0; c < bs; ++c) q[(size_t)i * bs + c] = qn[i] * bs + c;
    amg_mirror(cur, nullptr, B);
    amg_galerkin(B, q, nc * bs, next);
    for (int i = 0; i < m; ++i) nagg[i] = qn[nagg[i]];
    cur = std::move(next);
  }
  agg.resize((size_t)n);
  for (int i = 0; i < m; ++i)
    for (int c = 0; c < bs; ++c) agg[(size_t)i * bs + c] = nagg[i] * bs + c;
  coarse = std::move(cur);
  return 0;
}

// the inverse of a dense level from its lower triangle + diagonal: A = L L^T in fp64, the columns by two triangular
// solves each, then (X + X^T) / 2.  Returns the first pivot that is not finite and > 0, or -1
inline int amg_dense_inverse(const AmgCsr &low, std::vector<double> &inv) {
  const int n = low.n;
  std::vector<double> a((size_t)n * n, 0.0);
  for (int i = 0; i < n; ++i)
    for (long long k = low.rp[i]; k < low.rp[i + 1]; ++k) a[(size_t)i * n + low.ci[k]] = low.va[k];
  for (int j = 0; j < n; ++j) { // a <- L, column by column (the order of cg_binv_kernel)
    double dj = a[(size_t)j * n + j];
    for (int c = 0; c < j; ++c) dj -= a[(size_t)j * n + c] * a[(size_t)j * n + c];
    if (!(dj > 0.0) || dj * 0.0 != 0.0) return j;
    const double l = std::sqrt(dj);
    a[(size_t)j * n + j] = l;
#pragma omp parallel for schedule(static) if (n - j > 256)
    for (int i = j + 1; i < n; ++i) {
      double v = a[(size_t)i * n + j];
      for (int c = 0; c < j; ++c) v -= a[(size_t)i * n + c] * a[(size_t)j * n + c];
      a[(size_t)i * n + j] = v / l;
    }
  }
  std::vector<double> x((size_t)n * n, 0.0); // x[j * n + i] = column j of the inverse
#pragma omp parallel for schedule(dynamic, 8) if (n > 128)
  for (int j = 0; j < n; ++j) {
    double *y = &x[(size_t)j * n];
    for (int i = j; i < n; ++i) { // L y = e_j (y_i = 0 above j)
      double v = i == j ? 1.0 : 0.0;
      for (int c = j; c < i; ++c) v -= a[(size_t)i * n + c] * y[c];
      y[i] = v / a[(size_t)i * n + i];
    }
    for (int i = n - 1; i >= 0; --i) { // L^T x = y, in place
      const double xi = y[i] / a[(size_t)i * n + i];
      y[i] = xi;
      for (int c = 0; c < i; ++c) y[c] -= a[(size_t)i * n + c] * xi;
    }
  }
  inv.resize((size_t)n * n);
  for (int i = 0; i < n; ++i)
    for (int j = 0; j < n; ++j) inv[(size_t)i * n + j] = 0.5 * (x[(size_t)j * n + i] + x[(size_t)i * n + j]);
  return -1;
}

// ---- the kernels of the cycle, on a set of columns CS (see ONE CYCLE and THE COLUMNS OF A CYCLE in the header comment) ----
// Column c of a vector at base + c ld; the columns of cs are worked on in one launch, the others neither read nor
// written.  BS = 1: the scalar form, BS >= 2: the node-block form (one thread per node, w the packed W or M^-1 read by
// block_load, m the nodes of the level).  Where the accumulators are per column the columns go in chunks of CW: what a
// row, node or aggregate reads of the level -- w_i or W_i, agg, the aggregate list, a row of the dense inverse -- is
// loaded once per chunk.  One column is one chunk of one.
template <int BS> constexpr int amg_restrict_chunk() { return BS == 1 ? 8 : BS == 6 ? 2 : 4; } // (CW BS fp64 accumulators)
constexpr int kAmgDenseChunk = 8;

// rc_{I,c} = (V)(sum over the members i of aggregate I, ascending, of W_i (r_{i,c} - t_{i,c})): one thread per aggregate
// (BS >= 2: per coarse node, the members fine nodes)
template <typename V, int BS, class CS>
__global__ void __launch_bounds__(kThreads)
    amg_restrict_kernel(V *__restrict__ rc, long long ldc, const V *__restrict__ r, long long ldr, const V *__restrict__ t, long long ldt,
                        const V *__restrict__ w, long long m, const int *__restrict__ aggptr, const int *__restrict__ aggidx,
                        long long nc, const int *__restrict__ ic, CS cs) {
  if (ic[I_DONE]) return;
  constexpr int CW = CS::chunk(amg_restrict_chunk<BS>());
  cs.template chunks<CW>([&](int c0, unsigned bits) { // (uniform over the grid)
    for (long long I = (long long)blockIdx.x * kThreads + threadIdx.x; I < nc; I += (long long)gridDim.x * kThreads) {
      if constexpr (BS >= 2) {
        double s[CW][BS];
#pragma unroll
        for (int e = 0; e < CW; ++e)
#pragma unroll
          for (int c = 0; c < BS; ++c) s[e][c] = 0.0;
        for (int k = aggptr[I]; k < aggptr[I + 1]; ++k) {
          const long long i = aggidx[k];
          double mm[BS][BS];
          block_load<V, BS>(w, m, i, mm);
#pragma unroll
          for (int e = 0; e < CW; ++e) {
            if (!((bits >> e) & 1u)) continue;
            const V *re = r + (c0 + e) * ldr, *te = t + (c0 + e) * ldt;
            double x[BS], y[BS];
#pragma unroll
            for (int c = 0; c < BS; ++c) x[c] = (double)re[i * BS + c] - (double)te[i * BS + c];
            block_mul<BS>(mm, x, y);
#pragma unroll
            for (int c = 0; c < BS; ++c) s[e][c] += y[c];
          }
        }
#pragma unroll
        for (int e = 0; e < CW; ++e) {
          if (!((bits >> e) & 1u)) continue;
#pragma unroll
          for (int c = 0; c < BS; ++c) rc[(c0 + e) * ldc + I * BS + c] = (V)s[e][c];
        }
      } else {
        double s[CW];
#pragma unroll
        for (int e = 0; e < CW; ++e) s[e] = 0.0;
        for (int k = aggptr[I]; k < aggptr[I + 1]; ++k) {
          const int i = aggidx[k];
          const V wi = w[i];
#pragma unroll
          for (int e = 0; e < CW; ++e)
            if ((bits >> e) & 1u) s[e] += (double)wi * ((double)r[(c0 + e) * ldr + i] - (double)t[(c0 + e) * ldt + i]);
        }
#pragma unroll
        for (int e = 0; e < CW; ++e)
          if ((bits >> e) & 1u) rc[(c0 + e) * ldc + I] = (V)s[e];
      }
    }
  });
}

// z_{i,c} = (V)(z_{i,c} + W_i ec_{agg(i),c}): one thread per row (BS = 1, m = n) or per fine node
template <typename V, int BS, class CS>
__global__ void __launch_bounds__(kThreads)
    amg_prolong_kernel(V *__restrict__ z, long long ldz, const V *__restrict__ ec, long long lde, const V *__restrict__ w,
                       const int *__restrict__ agg, long long m, const int *__restrict__ ic, CS cs) {
  if (ic[I_DONE]) return;
  for (long long i = (long long)blockIdx.x * kThreads + threadIdx.x; i < m; i += (long long)gridDim.x * kThreads) {
    const long long I = agg[i];
    if constexpr (BS >= 2) {
      double mm[BS][BS];
      block_load<V, BS>(w, m, i, mm);
      cs.each([&](int c) {
        const V *ecc = ec + c * lde;
        V *zc = z + c * ldz;
        double e[BS], y[BS];
#pragma unroll
        for (int q = 0; q < BS; ++q) e[q] = (double)ecc[I * BS + q];
        block_mul<BS>(mm, e, y);
#pragma unroll
        for (int q = 0; q < BS; ++q) zc[i * BS + q] = (V)((double)zc[i * BS + q] + y[q]);
      });
    } else {
      const V wi = w[i];
      cs.each([&](int c) { z[c * ldz + i] = (V)((double)z[c * ldz + i] + (double)wi * (double)ec[c * lde + I]); });
    }
  }
}

// cheb_start_kernel from a nonzero z, t = A z given:  d_c = (V)((1 / theta) M^-1 (r_c - t_c));  z_c = (V)(z_c + d_c), M^-1
// applied as cheb_start_kernel<V, BS> applies it
template <typename V, int BS, class CS>
__global__ void __launch_bounds__(kThreads)
    amg_restart_kernel(V *__restrict__ z, long long ldz, V *__restrict__ d, long long ldd, const V *__restrict__ r, long long ldr,
                       const V *__restrict__ t, long long ldt, long long n, double inv_theta, const V *__restrict__ minv, long long nb,
                       const int *__restrict__ ic, CS cs) {
  if (ic[I_DONE]) return;
  if constexpr (BS >= 2) {
    for (long long k = (long long)blockIdx.x * kThreads + threadIdx.x; k < nb; k += (long long)gridDim.x * kThreads) {
      double mm[BS][BS];
      block_load<V, BS>(minv, nb, k, mm);
      cs.each([&](int c) {
        const V *rc = r + c * ldr, *tc = t + c * ldt;
        V *zc = z + c * ldz, *dc = d + c * ldd;
        double x[BS], zz[BS];
#pragma unroll
        for (int i = 0; i < BS; ++i) {
          const long long g = k * BS + i;
          x[i] = g < n ? (double)rc[g] - (double)tc[g] : 0.0;
        }
        block_mul<BS>(mm, x, zz);
#pragma unroll
        for (int i = 0; i < BS; ++i) {
          const long long g = k * BS + i;
          if (g < n) {
            const V di = (V)(inv_theta * zz[i]);
            dc[g] = di;
            zc[g] = (V)((double)zc[g] + (double)di);
          }
        }
      });
    }
  } else {
    constexpr int W = Vec16<V>::W;
    typedef typename Vec16<V>::type VT;
    const long long nv = n / W, t0 = (long long)blockIdx.x * kThreads + threadIdx.x, stride = (long long)gridDim.x * kThreads;
    for (long long i = t0; i < nv; i += stride) {
      const VT mv = reinterpret_cast<const VT *>(minv)[i];
      cs.each([&](int c) {
        const VT rv = reinterpret_cast<const VT *>(r + c * ldr)[i], tv = reinterpret_cast<const VT *>(t + c * ldt)[i];
        VT zv = reinterpret_cast<VT *>(z + c * ldz)[i], dv;
#pragma unroll
        for (int k = 0; k < W; ++k) {
          dv[k] = (V)(inv_theta * (((double)rv[k] - (double)tv[k]) * (double)mv[k]));
          zv[k] = (V)((double)zv[k] + (double)dv[k]);
        }
        reinterpret_cast<VT *>(d + c * ldd)[i] = dv;
        reinterpret_cast<VT *>(z + c * ldz)[i] = zv;
      });
    }
    for (long long i = nv * W + t0; i < n; i += stride) {
      const V mi = minv[i];
      cs.each([&](int c) {
        const V di = (V)(inv_theta * (((double)r[c * ldr + i] - (double)t[c * ldt + i]) * (double)mi));
        d[c * ldd + i] = di;
        z[c * ldz + i] = (V)((double)z[c * ldz + i] + (double)di);
      });
    }
  }
}

// z_c = (V)(inv r_c) on the dense level: one wave per row, which it reads ONCE per chunk of columns; per column the lanes
// stride over the row, a fixed-order sum
template <typename V, class CS>
__global__ void __launch_bounds__(kThreads)
    amg_dense_kernel(V *__restrict__ z, long long ldz, const V *__restrict__ inv, const V *__restrict__ r, long long ldr, int n,
                     const int *__restrict__ ic, CS cs) {
  if (ic[I_DONE]) return;
  constexpr int CW = CS::chunk(kAmgDenseChunk);
  const int lane = threadIdx.x & 63, nwaves = gridDim.x * (kThreads / 64);
  cs.template chunks<CW>([&](int c0, unsigned bits) { // (uniform over the grid)
    for (int i = blockIdx.x * (kThreads / 64) + (threadIdx.x >> 6); i < n; i += nwaves) { // (uniform over the wave)
      const V *row = inv + (size_t)i * n;
      double s[CW];
#pragma unroll
      for (int e = 0; e < CW; ++e) s[e] = 0.0;
      for (int j = lane; j < n; j += 64) {
        const V a = row[j];
#pragma unroll
        for (int e = 0; e < CW; ++e)
          if ((bits >> e) & 1u) s[e] += (double)a * (double)r[(c0 + e) * ldr + j];
      }
#pragma unroll
      for (int e = 0; e < CW; ++e) {
        if (!((bits >> e) & 1u)) continue;
        double v = s[e];
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o);
        if (lane == 0) z[(c0 + e) * ldz + i] = (V)v;
      }
    }
  });
}

// ---- the kernels of a refresh (see REFRESH at the end of the header comment) ------------------------
// out[e] = src[idx[ptr[e]]] + src[idx[ptr[e] + 1]] + ... in fp64, in the order of the list: one thread per output entry.
// LAST (the last round of a level): vout[e] = (V)s, what the next level's handle is poured, and out[e] = (double)(V)s,
// what the next level is coarsened from.  Adds only: nothing for the compiler to contract
template <typename S, typename V, bool LAST>
__global__ void __launch_bounds__(kThreads)
    amg_gather_sum_kernel(double *__restrict__ out, V *__restrict__ vout, const S *__restrict__ src, const int *__restrict__ ptr,
                          const int *__restrict__ idx, long long m) {
  for (long long e = (long long)blockIdx.x * kThreads + threadIdx.x; e < m; e += (long long)gridDim.x * kThreads) {
    int k = ptr[e];
    const int end = ptr[e + 1];
    double s = (double)src[idx[k]];
    for (++k; k < end; ++k) s += (double)src[idx[k]];
    if (LAST) {
      const V v = (V)s;
      vout[e] = v;
      out[e] = (double)v;
    } else {
      out[e] = s;
    }
  }
}

// w64_i = 1 / sqrt(a[diag[i]]) in fp64, w_i = (V)w64_i;  bad[workgroup] <- diagonal entries that are not finite and > 0
template <typename V>
__global__ void __launch_bounds__(kThreads)
    amg_weight_kernel(double *__restrict__ w64, V *__restrict__ w, const double *__restrict__ a, const int *__restrict__ diag, long long n,
                      double *__restrict__ bad_out) {
  double bad = 0.0;
  for (long long i = (long long)blockIdx.x * kThreads + threadIdx.x; i < n; i += (long long)gridDim.x * kThreads) {
    const double d = a[diag[i]];
    if (!(d > 0.0) || d * 0.0 != 0.0) bad += 1.0;
    const double wi = 1.0 / sqrt(d);
    w64[i] = wi;
    w[i] = (V)wi;
  }
  bad = block_sum(bad);
  if (threadIdx.x == 0) bad_out[blockIdx.x] = bad;
}

// a_k <- b_k = (w_row(k) a_k) w_col(k), in place: the operand order of amg_mirror, the row the larger index
__global__ void __launch_bounds__(kThreads)
    amg_scale_kernel(double *__restrict__ a, const double *__restrict__ w64, const int *__restrict__ row, const int *__restrict__ col,
                     long long m) {
  for (long long k = (long long)blockIdx.x * kThreads + threadIdx.x; k < m; k += (long long)gridDim.x * kThreads)
    a[k] = (w64[row[k]] * a[k]) * w64[col[k]];
}

// ---- the hierarchy on the device -------------------------------------------------------------------
enum AmgKind { AMG_MULTIGRID = 0, AMG_SMOOTHER = 1, AMG_DENSE = 2 };
enum AmgPhase { AMG_T_GALERKIN = 0, AMG_T_POUR, AMG_T_POWER, AMG_T_DENSE, AMG_T_COUNT }; // the split of a refresh's time

template <typename V, int BS = 1> struct AmgLevel {
  int n = 0, nc = 0, kind = AMG_MULTIGRID;
  long long nnz = 0;
  double lmin = 0.0, lmax = 0.0, theta = 1.0, c1[kChebMaxDegree], c2[kChebMaxDegree];
  cfs_hip_sym_s *h = nullptr;
  bool owned = false;
  Precond<V, BS> pre; // dinv (BS >= 2: the packed inverse node blocks) of a level that smooths
  // (BS >= 2: aggptr, aggidx and agg hold NODES, w the packed W_i)
  cfs_rt::DevBuf aggptr, aggidx, agg, w, r, z, d, t, inv;
  // the work vectors of the column-blocked cycle, column c at + c cld values (cld: n rounded up to 16 bytes): cd and ct
  // on a level that smooths, cr and cz below level 0; made by Amg::reserve_cols at the first blocked call of a width
  cfs_rt::DevBuf cr, cz, cd, ct;
  long long cld = 0;
  // the CSR the level's handle was created from (levels >= 1): lower triangle + diagonal, values in V
  std::vector<int> rp, ci;
  std::vector<V> va;
  // a refreshable hierarchy only: the lists of amg_lower (level 0), the frozen level (a level with a coarser one) and
  // vdev, the device image of va in V (levels >= 1): written by the level above, poured into h, read back into va on demand
  cfs_rt::DevBuf lptr, lidx, fdiag, frow, fcol, rptr[3], ridx[3], vdev;
  long long rout[3] = {0, 0, 0}; // entries round p writes
  bool va_stale = false;
  AmgCsr dense;                  // the pattern of a dense level, for amg_dense_inverse
  ~AmgLevel() {
    if (owned) delete h;
  }
  size_t bytes() const {
    return pre.dbuf.bytes + aggptr.bytes + aggidx.bytes + agg.bytes + w.bytes + r.bytes + z.bytes + d.bytes + t.bytes + inv.bytes +
           cr.bytes + cz.bytes + cd.bytes + ct.bytes;
  }
  size_t map_bytes() const {
    size_t b = lptr.bytes + lidx.bytes + fdiag.bytes + frow.bytes + fcol.bytes + vdev.bytes;
    for (int p = 0; p < 3; ++p) b += rptr[p].bytes + ridx[p].bytes;
    return b;
  }
};

} // namespace cfs_solver
#include "cfs_solver_amg_setup.hpp" // a level coarsened on the device: AmgDeviceSetup
namespace cfs_solver {

template <typename V, int BS = 1> struct Amg : cfs_hip_amg_s {
  using Level = AmgLevel<V, BS>;
  std::vector<std::unique_ptr<Level>> lv;
  Slots part;         // the partial-sum slots the smoother's kernels are handed
  cfs_rt::DevBuf cnt; // a done flag that is never set
  int passes = 2, degree = 1, coarse_max = 512, device = 0;
  double ratio = 4.0, setup_seconds = 0.0, handles_seconds = 0.0;
  // a refreshable hierarchy (cfs_hip_amg_create_refreshable_*)
  bool refreshable = false, stale = false;
  int refreshes = 0;
  long long nnz_caller = 0, value_map_bytes = 0; // ... of the level handles' value maps: 4 per stored entry, an ESTIMATE
  unsigned long long fine_epoch = 0;             // fine->values_epoch when level 0's dinv and bound were last made
  double last_seconds = 0.0, split[AMG_T_COUNT] = {0.0, 0.0, 0.0, 0.0};
  cfs_rt::DevBuf rbuf[2], w64, pw; // kept: two fp64 arrays of the longest level, the fp64 weights, the power method's vector
  Slots rpart, rlpart;             // P_COUNT slots of a level's smoother + one for amg_weight_kernel; the power method's, kept
  std::vector<hipEvent_t> ev;
  // how the hierarchy was made (cfs_hip_amg_setup_info): the matching, where (0 host, 1 device, 2 device after amg_lower
  // on the host), the rounds every pass of every level ran, the split of a device set-up and its scratch
  int matching = CFS_HIP_AMG_MATCHING_GREEDY, on_device = 0, rounds[CFS_HIP_AMG_MAX_LEVELS][3] = {};
  double setup_split[4] = {0.0, 0.0, 0.0, 0.0};
  long long scratch_bytes = 0;
  int col_cap = 0;           // the columns the levels' blocked work vectors hold (0: no blocked call yet)
  long long col_cycles = 0;  // cycles applied to the columns of a ColumnMask, one per active column (cfs_hip_amg_column_cycles)

  ~Amg() override {
    cfs_rt::DeviceGuard g(device);
    for (hipEvent_t e : ev) (void)hipEventDestroy(e);
    lv.clear();
  }

  // mk(n, rowptr, colind, values, flags, &handle): the library's own create path
  template <class Make>
  int build(cfs_hip_sym_s *h, int n, const int *rowptr, const int *colind, const V *values, int flags, Make &&mk) {
    using clock = std::chrono::steady_clock;
    const auto t_begin = clock::now();
    fine = h;
    fine_epoch = h->values_epoch;
    value_bytes = (int)sizeof(V);
    hipStream_t st = nullptr;
    int rc;
    if ((rc = part.alloc(P_COUNT, st)) || (rc = cnt.alloc(I_COUNT * sizeof(int))) || (rc = part.zero())) return rc;
    HIPCHK(hipMemset(cnt.p, 0, I_COUNT * sizeof(int)));
    AmgCsr cur, next;
    // a device set-up holds the level on the device; `cur` is then the coarse CSR it brought down (levels >= 1), or
    // amg_lower's when level 0 is the last one
    std::unique_ptr<AmgDeviceSetup<V>> dev;
    if (BS == 1 && on_device && n > coarse_max) {
      dev.reset(new AmgDeviceSetup<V>());
      if ((rc = dev->begin(n, rowptr, colind, values, st))) return rc;
      if (dev->host_lower) on_device = 2;
      scratch_bytes = dev->scratch_bytes;
    } else {
      amg_lower(n, rowptr, colind, values, cur);
    }
    auto bad_diagonal = [](long long bad, int rows, int l) {
      return cfs_rt::set_err(CFS_HIP_ERR_ARG, "amg_create: Jacobi needs a positive diagonal, " + std::to_string(bad) + " of " +
                                                  std::to_string(rows) + " entries are zero, negative or not finite (level " +
                                                  std::to_string(l) + ")");
    };
    auto bad_blocks = [](long long bad, int rows, int l) {
      return cfs_rt::set_err(CFS_HIP_ERR_ARG, "amg_create: node-block multigrid needs positive definite node blocks, " + std::to_string(bad) +
                                                  " of " + std::to_string(rows / BS) + " blocks of " + std::to_string(BS) +
                                                  " rows have an eigenvalue that is zero, negative or not finite (level " +
                                                  std::to_string(l) + ")");
    };
    std::vector<int> agg;
    std::vector<double> w, inv;
    AmgFrozen frozen;
    size_t longest = 0;
    for (int l = 0;; ++l) {
      lv.emplace_back(new Level());
      Level &L = *lv.back();
      const bool resident0 = dev && l == 0; // level 0 of a device set-up: only the device holds its lower triangle
      L.n = resident0 ? dev->n : cur.n;
      L.nnz = resident0 ? dev->m : cur.nnz();
      longest = std::max(longest, (size_t)L.nnz);
      if (refreshable && l == 0) {
        AmgList li;
        amg_lower_lists(n, rowptr, colind, li);
        nnz_caller = n > 0 ? rowptr[n] : 0;
        if ((rc = L.lptr.upload(li.ptr.data(), li.ptr.size() * sizeof(int))) || (rc = L.lidx.upload(li.idx.data(), li.idx.size() * sizeof(int))))
          return rc;
      }
      long long bad = 0;
      std::vector<double> diag;
      if (!resident0 && (bad = amg_diagonal(cur, diag))) return bad_diagonal(bad, cur.n, l);
      if (l == 0) {
        L.h = h;
      } else { // the level as a handle of its own, from the values rounded to V (which `cur` already holds)
        L.rp.resize((size_t)cur.n + 1);
        for (int i = 0; i <= cur.n; ++i) L.rp[i] = (int)cur.rp[i];
        L.ci = cur.ci;
        L.va.resize(cur.va.size());
        for (size_t k = 0; k < cur.va.size(); ++k) L.va[k] = (V)cur.va[k];
        const auto t0 = clock::now();
        if ((rc = mk(cur.n, L.rp.data(), L.ci.data(), L.va.data(), flags, &L.h))) return rc;
        L.owned = true;
        if (refreshable && (rc = L.vdev.upload(L.va.data(), L.va.size() * sizeof(V)))) return rc;
        handles_seconds += std::chrono::duration<double>(clock::now() - t0).count();
      }
      // how the hierarchy goes on
      bool last = L.n <= coarse_max;
      L.kind = last ? AMG_DENSE : AMG_MULTIGRID;
      if (!last) {
        if constexpr (BS >= 2) {
          if (amg_coarsen_block(cur, BS, passes, agg, w, next, &bad, matching, rounds[l])) return bad_blocks(bad, L.n, l);
        } else if (dev) {
          if ((rc = dev->coarsen(L, passes, &bad, next, rounds[l]))) return rc == 1 ? bad_diagonal(bad, L.n, l) : rc;
        } else if (amg_coarsen(cur, passes, agg, w, next, &bad, refreshable ? &frozen : nullptr, matching, rounds[l])) {
          return cfs_rt::set_err(CFS_HIP_ERR_INTERNAL, "amg_create: the diagonal changed");
        }
        if ((double)next.n > 0.9 * (double)L.n || l + 1 == CFS_HIP_AMG_MAX_LEVELS) {
          last = true;
          L.kind = L.n <= CFS_HIP_AMG_MAX_COARSE ? AMG_DENSE : AMG_SMOOTHER;
          if (resident0 && L.kind == AMG_DENSE) amg_lower(n, rowptr, colind, values, cur); // (at most 1024 rows)
          if (dev) L.agg = cfs_rt::DevBuf(), L.w = cfs_rt::DevBuf(), L.aggptr = cfs_rt::DevBuf(), L.aggidx = cfs_rt::DevBuf();
        }
      }
      if (L.kind == AMG_DENSE) {
        const int piv = amg_dense_inverse(cur, inv);
        if (piv >= 0)
          return cfs_rt::set_err(CFS_HIP_ERR_ARG, "amg_create: the matrix of level " + std::to_string(l) + " (" + std::to_string(cur.n) +
                                                      " rows) is not positive definite: pivot " + std::to_string(piv) +
                                                      " of its Cholesky factorisation is zero, negative or not finite");
        std::vector<V> iv(inv.size());
        for (size_t k = 0; k < inv.size(); ++k) iv[k] = (V)inv[k];
        if ((rc = L.inv.upload(iv.data(), iv.size() * sizeof(V)))) return rc;
        if (refreshable) L.dense.n = cur.n, L.dense.rp = cur.rp, L.dense.ci = cur.ci;
      } else {
        if ((rc = setup_smoother(L, st))) return rc;
      }
      if (l > 0 && ((rc = L.r.alloc((size_t)L.n * sizeof(V) + 64)) || (rc = L.z.alloc((size_t)L.n * sizeof(V) + 64)))) return rc;
      if (last) break;
      if (refreshable) { // the lists a refresh evaluates at this level
        if (frozen.overflow())
          return cfs_rt::set_err(CFS_HIP_ERR_UNSUPPORTED, "amg_create_refreshable: the contributions of a round of level " +
                                                              std::to_string(l) + " exceed the 32-bit indices of the lists");
        if ((rc = L.fdiag.upload(frozen.diag.data(), frozen.diag.size() * sizeof(int))) ||
            (rc = L.frow.upload(frozen.row.data(), frozen.row.size() * sizeof(int))) ||
            (rc = L.fcol.upload(cur.ci.data(), cur.ci.size() * sizeof(int))))
          return rc;
        for (int p = 0; p < passes; ++p) {
          const AmgList &r = frozen.rounds[p];
          L.rout[p] = r.entries();
          if ((rc = L.rptr[p].upload(r.ptr.data(), r.ptr.size() * sizeof(int))) || (rc = L.ridx[p].upload(r.idx.data(), r.idx.size() * sizeof(int))))
            return rc;
        }
      }
      // the transfer to the next level
      L.nc = next.n;
      if (dev) { // (agg, the lists and w are on the device already)
        cur = std::move(next);
        continue;
      }
      std::vector<V> wv;
      if constexpr (BS >= 2) { // the lists and agg over the nodes; W packed as cg_binv_kernel packs the inverse
        const int m = cur.n / BS;
        for (int i = 0; i < m; ++i) agg[i] = agg[(size_t)i * BS] / BS;
        agg.resize((size_t)m);
        wv.resize((size_t)m * tri_words(BS));
        for (int i = 0; i < m; ++i)
          for (int c = 0; c < BS; ++c)
            for (int e = 0; e <= c; ++e) wv[(size_t)(c * (c + 1) / 2 + e) * m + i] = (V)w[((size_t)i * BS + c) * BS + e];
      } else {
        wv.resize((size_t)cur.n);
        for (int i = 0; i < cur.n; ++i) wv[i] = (V)w[i];
      }
      const int units = cur.n / BS, cunits = next.n / BS; // rows, or nodes
      std::vector<int> ptr((size_t)cunits + 1, 0), idx((size_t)units);
      for (int i = 0; i < units; ++i) ptr[(size_t)agg[i] + 1] += 1;
      for (int I = 0; I < cunits; ++I) ptr[(size_t)I + 1] += ptr[I];
      {
        std::vector<int> pos(ptr.begin(), ptr.end() - 1);
        for (int i = 0; i < units; ++i) idx[pos[agg[i]]++] = i; // (rows ascending: members ascending)
      }
      if ((rc = L.aggptr.upload(ptr.data(), ptr.size() * sizeof(int))) || (rc = L.aggidx.upload(idx.data(), idx.size() * sizeof(int))) ||
          (rc = L.agg.upload(agg.data(), agg.size() * sizeof(int))) || (rc = L.w.upload(wv.data(), wv.size() * sizeof(V))))
        return rc;
      for (double &v : next.va) v = (double)(V)v; // the next level is what its handle will hold
      cur = std::move(next);
    }
    if (refreshable) {
      for (int k = 0; k < 2; ++k)
        if ((rc = rbuf[k].alloc(longest * sizeof(double) + 64))) return rc;
      if ((rc = w64.alloc((size_t)n * sizeof(double) + 64)) || (rc = alloc_vectors<V>(n, {&pw})) || (rc = rpart.alloc(P_COUNT + 1, st)) ||
          (rc = rlpart.alloc(L_COUNT, st)))
        return rc;
      for (size_t l = 1; l < lv.size(); ++l) value_map_bytes += 4 * lv[l]->nnz;
    }
    HIPCHK(hipDeviceSynchronize());
    if (dev)
      for (int k = 0; k < 4; ++k) setup_split[k] = dev->seconds[k];
    dev.reset(); // (the scratch goes before the call returns)
    setup_seconds = std::chrono::duration<double>(clock::now() - t_begin).count();
    return 0;
  }

  int setup_info(int *mt, int *where, int *rnd, double *seconds, long long *scratch) override {
    if (mt) *mt = matching;
    if (where) *where = on_device;
    if (rnd)
      for (size_t l = 0; l < lv.size(); ++l)
        for (int p = 0; p < 3; ++p) rnd[3 * l + p] = rounds[l][p];
    if (seconds)
      for (int k = 0; k < 4; ++k) seconds[k] = setup_split[k];
    if (scratch) *scratch = scratch_bytes;
    return 0;
  }

  long long map_bytes() const {
    long long b = (long long)(rbuf[0].bytes + rbuf[1].bytes + w64.bytes + pw.bytes + rpart.buf.bytes + rlpart.buf.bytes) + value_map_bytes;
    for (const auto &L : lv) b += (long long)L->map_bytes();
    return b;
  }

  // cfs_hip_amg_update_values_*: the arithmetic of build() with the matchings frozen, on `st`.  vals: the caller's
  // values[] on the device.  Returns when the hierarchy is complete; on an error the object is stale
  int refresh(const V *vals, hipStream_t st) {
    using clock = std::chrono::steady_clock;
    const auto t_begin = clock::now();
    const int nl = (int)lv.size();
    stale = true;
    rpart.st = st;
    if (ev.empty()) {
      ev.resize((size_t)4 * nl);
      for (hipEvent_t &e : ev) HIPCHK(hipEventCreate(&e));
    }
    // X: what the next kernel reads -- the level's lower-triangle array in fp64, B (scaled in place), a round's output;
    // Y: what a round writes.  They change places after every round
    double *X = (double *)rbuf[0].p, *Y = (double *)rbuf[1].p, *bad_dev = rpart.dev() + (size_t)P_COUNT * kGrid;
    double dense_seconds = 0.0;
    int rc, done = 0;
    for (int l = 0; l < nl; ++l) {
      Level &L = *lv[l];
      HIPCHK(hipEventRecord(ev[4 * l + 0], st));
      if (l == 0 && L.nnz > 0)
        hipLaunchKernelGGL((amg_gather_sum_kernel<V, V, false>), dim3(kGrid), dim3(kThreads), 0, st, X, (V *)nullptr, vals,
                           (const int *)L.lptr.p, (const int *)L.lidx.p, L.nnz);
      if ((rc = rpart.zero())) return rc;
      if (L.kind == AMG_MULTIGRID) {
        Level &C = *lv[l + 1];
        hipLaunchKernelGGL((amg_weight_kernel<V>), dim3(kGrid), dim3(kThreads), 0, st, (double *)w64.p, (V *)L.w.p, (const double *)X,
                           (const int *)L.fdiag.p, (long long)L.n, bad_dev);
        hipLaunchKernelGGL(amg_scale_kernel, dim3(kGrid), dim3(kThreads), 0, st, X, (const double *)w64.p, (const int *)L.frow.p,
                           (const int *)L.fcol.p, L.nnz);
        for (int p = 0; p < passes; ++p) {
          const int *ptr = (const int *)L.rptr[p].p, *idx = (const int *)L.ridx[p].p;
          if (p + 1 < passes)
            hipLaunchKernelGGL((amg_gather_sum_kernel<double, V, false>), dim3(kGrid), dim3(kThreads), 0, st, Y, (V *)nullptr,
                               (const double *)X, ptr, idx, L.rout[p]);
          else
            hipLaunchKernelGGL((amg_gather_sum_kernel<double, V, true>), dim3(kGrid), dim3(kThreads), 0, st, Y, (V *)C.vdev.p,
                               (const double *)X, ptr, idx, L.rout[p]);
          std::swap(X, Y); // (what was written is the next round's source, and after the last round the next level's array)
        }
        HIPCHK(hipGetLastError());
        HIPCHK(hipEventRecord(ev[4 * l + 1], st));
        C.va_stale = true;
        if ((rc = C.h->update_values(C.vdev.p, C.nnz, st))) return rc;
      } else {
        HIPCHK(hipEventRecord(ev[4 * l + 1], st));
      }
      HIPCHK(hipEventRecord(ev[4 * l + 2], st));
      if (L.kind == AMG_DENSE) {
        HIPCHK(hipEventRecord(ev[4 * l + 3], st));
        const auto t0 = clock::now();
        L.dense.va.resize((size_t)L.nnz);
        HIPCHK(hipMemcpyAsync(L.dense.va.data(), X, (size_t)L.nnz * sizeof(double), hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));
        std::vector<double> inv;
        const int piv = amg_dense_inverse(L.dense, inv);
        if (piv >= 0)
          return cfs_rt::set_err(CFS_HIP_ERR_ARG, "amg_update_values: the matrix of level " + std::to_string(l) + " (" + std::to_string(L.n) +
                                                      " rows) is not positive definite: pivot " + std::to_string(piv) +
                                                      " of its Cholesky factorisation is zero, negative or not finite");
        std::vector<V> iv(inv.size());
        for (size_t k = 0; k < inv.size(); ++k) iv[k] = (V)inv[k];
        HIPCHK(hipMemcpyAsync(L.inv.p, iv.data(), iv.size() * sizeof(V), hipMemcpyHostToDevice, st));
        HIPCHK(hipStreamSynchronize(st));
        dense_seconds = std::chrono::duration<double>(clock::now() - t0).count();
      } else {
        rc = refresh_smoother(L, l, st); // (the level's host look)
        HIPCHK(hipEventRecord(ev[4 * l + 3], st));
        if (rc) return rc;
      }
      done = l + 1;
    }
    HIPCHK(hipStreamSynchronize(st));
    for (int k = 0; k < AMG_T_COUNT; ++k) split[k] = 0.0;
    for (int l = 0; l < done; ++l)
      for (int k = 0; k < 3; ++k) {
        float ms = 0.0f;
        HIPCHK(hipEventElapsedTime(&ms, ev[4 * l + k], ev[4 * l + k + 1]));
        split[k] += 1e-3 * (double)ms;
      }
    split[AMG_T_DENSE] = dense_seconds;
    stale = false;
    refreshes += 1;
    last_seconds = std::chrono::duration<double>(clock::now() - t_begin).count();
    return 0;
  }

  // Level 0 is the caller's handle, and the caller pours its values: dinv and the bound of level 0 are made from what h
  // holds during the refresh and, when h has been poured since (cfs_hip_sym_update_values_* AFTER the refresh), once
  // more by the next apply or pcg, on its stream (info() only reports: until then it shows the bound of the refresh)
  int follow_fine(hipStream_t st) {
    if (!refreshable || lv.empty() || lv[0]->kind == AMG_DENSE || fine_epoch == fine->values_epoch) return 0;
    rpart.st = st;
    int rc = rpart.zero();
    if (!rc) rc = refresh_smoother(*lv[0], 0, st);
    if (rc) {
      stale = true;
      return rc;
    }
    return 0;
  }

  // the numbers of setup_smoother again, into the buffers it allocated: dinv from the level's handle, the bound, the pairs
  int refresh_smoother(Level &L, int l, hipStream_t st) {
    const long long n = L.n;
    double est = 0.0;
    int rc;
    if (l == 0) fine_epoch = fine->values_epoch;
    if ((rc = L.h->diagonal(L.pre.dbuf.p, st))) return rc;
    hipLaunchKernelGGL((cg_dinv_kernel<V>), dim3(kGrid), dim3(kThreads), 0, st, (V *)L.pre.dbuf.p, n, rpart.dev());
    if ((rc = cheb_power<V, 1>(L.h, (V *)L.d.p, (V *)L.t.p, (V *)pw.p, (const V *)nullptr, n, 16, rlpart, L.pre.minv(), 0LL, &est, st)) ||
        (rc = rpart.fetch()))
      return rc;
    const double bad = std::max(rpart.sum(P_BAD), L.kind == AMG_MULTIGRID ? rpart.sum(P_COUNT) : 0.0);
    if (bad != 0.0)
      return cfs_rt::set_err(CFS_HIP_ERR_ARG, "amg_update_values: Jacobi needs a positive diagonal, " + std::to_string((long long)bad) +
                                                  " of " + std::to_string(n) + " entries are zero, negative or not finite (level " +
                                                  std::to_string(l) + ")");
    if (!(est > 0.0) || est * 0.0 != 0.0)
      return cfs_rt::set_err(CFS_HIP_ERR_ARG, "amg_update_values: the power method gave no positive estimate of lambda_max(D^-1 A) on a level of " +
                                                  std::to_string(n) + " rows (" + std::to_string(est) + ")");
    L.lmax = 1.1 * est;
    L.lmin = L.lmax / ratio;
    cheb_coeffs(degree, L.lmin, L.lmax, &L.theta, L.c1, L.c2);
    return 0;
  }

  // dinv, the work vectors and the bounds of a level that smooths
  int setup_smoother(Level &L, hipStream_t st) {
    const long long n = L.n;
    cfs_rt::DevBuf vbuf;
    Slots lpart;
    double est = 0.0;
    int rc;
    if ((rc = alloc_vectors<V>(n, {&L.d, &L.t})) || (rc = L.pre.setup(L.h, part.dev(), st)) || (rc = alloc_vectors<V>(n, {&vbuf})) ||
        (rc = cheb_power<V, BS>(L.h, (V *)L.d.p, (V *)L.t.p, (V *)vbuf.p, (const V *)nullptr, n, 16, lpart, L.pre.minv(), L.pre.nb, &est, st)) ||
        (rc = part.fetch()) || (rc = L.pre.check("amg_create", part, n)))
      return rc;
    L.pre.blkbuf = cfs_rt::DevBuf(); // (the gathered blocks of BS >= 2 have been inverted: the stream is idle after the fetch)
    if (!(est > 0.0) || est * 0.0 != 0.0)
      return cfs_rt::set_err(CFS_HIP_ERR_ARG, "amg_create: the power method gave no positive estimate of lambda_max(D^-1 A) on a level of " +
                                                  std::to_string(n) + " rows (" + std::to_string(est) + ")");
    L.lmax = 1.1 * est;
    L.lmin = L.lmax / ratio;
    cheb_coeffs(degree, L.lmin, L.lmax, &L.theta, L.c1, L.c2);
    return 0;
  }

  // the work vectors of a level for a column set and their leading dimension: those build() allocates for one column,
  // those of reserve_cols for a block
  struct Work {
    V *d, *t, *r, *z;
    long long ld;
  };
  static Work work(Level &L, OneColumn) { return {(V *)L.d.p, (V *)L.t.p, (V *)L.r.p, (V *)L.z.p, L.n}; }
  static Work work(Level &L, ColumnMask) { return {(V *)L.cd.p, (V *)L.ct.p, (V *)L.cr.p, (V *)L.cz.p, L.cld}; }

  // Z_c = M^-1 R_c for the columns c of cs, from level l down, on `st`; ic: the done flag the kernels look at.  Every
  // vector kernel is launched ONCE for the columns, the products are one per column.  Column c of Z at Z + c ld_z, of R
  // at R + c ld_r; for a ColumnMask reserve_cols(cs.ncols) has been called
  template <class CS> int cycle(int l, CS cs, V *Z, long long ld_z, const V *R, long long ld_r, const int *ic, hipStream_t st) {
    Level &L = *lv[l];
    const long long n = L.n;
    double *pp = part.dev();
    if (L.kind == AMG_DENSE) {
      hipLaunchKernelGGL((amg_dense_kernel<V, CS>), dim3(kGrid), dim3(kThreads), 0, st, Z, ld_z, (const V *)L.inv.p, R, ld_r, L.n, ic, cs);
      return 0;
    }
    const Work wk = work(L, cs);
    V *d = wk.d, *t = wk.t;
    const long long ldw = wk.ld;
    const V *dinv = L.pre.minv();
    const long long nb = L.pre.nb; // the nodes of the level (BS >= 2), else 0
    int rc;
    auto products = [&]() -> int { // t_c = A_l z_c
      int r2 = 0;
      cs.each([&](int c) {
        if (!r2) r2 = L.h->spmv_local(t + c * ldw, Z + c * ld_z, nullptr, st);
      });
      return r2;
    };
    hipLaunchKernelGGL((cheb_start_kernel<V, BS, CS>), dim3(kGrid), dim3(kThreads), 0, st, Z, ld_z, d, ldw, R, ld_r, n, 1.0 / L.theta, -1,
                       pp, dinv, nb, cs);
    if ((rc = cheb_chain<V, BS>(L.h, cs, Z, ld_z, d, t, ldw, R, ld_r, n, degree, L.c1, L.c2, -1, pp, ic, dinv, nb, st))) return rc;
    if (L.kind == AMG_SMOOTHER) return 0;
    const Work cw = work(*lv[l + 1], cs);
    const long long units = BS >= 2 ? nb : n; // nodes, or rows
    if ((rc = products())) return rc;
    hipLaunchKernelGGL((amg_restrict_kernel<V, BS, CS>), dim3(kGrid), dim3(kThreads), 0, st, cw.r, cw.ld, R, ld_r, (const V *)t, ldw,
                       (const V *)L.w.p, units, (const int *)L.aggptr.p, (const int *)L.aggidx.p, (long long)(L.nc / BS), ic, cs);
    if ((rc = cycle(l + 1, cs, cw.z, cw.ld, (const V *)cw.r, cw.ld, ic, st))) return rc;
    hipLaunchKernelGGL((amg_prolong_kernel<V, BS, CS>), dim3(kGrid), dim3(kThreads), 0, st, Z, ld_z, (const V *)cw.z, cw.ld,
                       (const V *)L.w.p, (const int *)L.agg.p, units, ic, cs);
    if ((rc = products())) return rc;
    hipLaunchKernelGGL((amg_restart_kernel<V, BS, CS>), dim3(kGrid), dim3(kThreads), 0, st, Z, ld_z, d, ldw, R, ld_r, (const V *)t, ldw, n,
                       1.0 / L.theta, dinv, nb, ic, cs);
    return cheb_chain<V, BS>(L.h, cs, Z, ld_z, d, t, ldw, R, ld_r, n, degree, L.c1, L.c2, -1, pp, ic, dinv, nb, st);
  }

  // the levels' work vectors for a block of `ncols` columns: allocated at the first blocked call, kept, and made again
  // only for a wider one (hipFree waits for the device: nothing enqueued still uses the old ones)
  int reserve_cols(int ncols) {
    if (ncols <= col_cap) return 0;
    col_cap = 0; // (an allocation that fails half-way leaves no width behind: the next call reserves again)
    for (size_t l = 0; l < lv.size(); ++l) {
      Level &L = *lv[l];
      L.cld = ((long long)L.n + Vec16<V>::W - 1) / Vec16<V>::W * Vec16<V>::W;
      const size_t bytes = (size_t)ncols * (size_t)L.cld * sizeof(V) + 64;
      int rc;
      if (L.kind != AMG_DENSE && ((rc = L.cd.alloc(bytes)) || (rc = L.ct.alloc(bytes)))) return rc;
      if (l > 0 && ((rc = L.cr.alloc(bytes)) || (rc = L.cz.alloc(bytes)))) return rc;
    }
    col_cap = ncols;
    return 0;
  }

  // cfs_hip_amg_apply_cols (arguments checked by the caller; active != 0)
  int apply_cols(void *z_dev, const void *r_dev, long long ld, int ncols, unsigned active, hipStream_t st) override {
    if (stale) return cfs_rt::set_err(CFS_HIP_ERR_ARG, "amg_apply_cols: the last refresh failed");
    int rc = follow_fine(st);
    if (rc || (rc = reserve_cols(ncols))) return rc;
    rc = cycle(0, ColumnMask{ncols, active}, (V *)z_dev, ld, (const V *)r_dev, ld, (const int *)cnt.p, st);
    if (rc) return rc;
    col_cycles += __builtin_popcount(active);
    HIPCHK(hipGetLastError());
    return 0;
  }
  // cfs_hip_sym_lobpcg_amg / cfs_hip_sym_debug_lobpcg_amg: the iteration of cfs_solver_lobpcg.hpp with W formed by the
  // blocked cycle on the columns still active (arguments checked by the caller)
  int lobpcg(cfs_hip_sym_s *hb, int k, double tol, double scale, int maxiter, int debug_iters, const void *x0_dev, long long ld0,
             double *eigenvalues, void *vectors_dev, long long ld, double *residuals, int *nconv, int *iterations, int *products,
             int *b_products, hipStream_t st) override {
    if (stale) return cfs_rt::set_err(CFS_HIP_ERR_ARG, "lobpcg_amg: the last refresh failed");
    int rc = follow_fine(st);
    if (rc || (rc = reserve_cols(k))) return rc;
    auto form_w = [&](V *W, const V *R, long long ldw, int kk, unsigned mask) -> int {
      if (int r2 = cycle(0, ColumnMask{kk, mask}, W, ldw, R, ldw, (const int *)cnt.p, st)) return r2;
      col_cycles += __builtin_popcount(mask);
      return 0;
    };
    if (hb)
      return cfs_solver::lobpcg<V, 0, true>(fine, hb, k, tol, scale, maxiter, debug_iters, x0_dev, ld0, eigenvalues, vectors_dev, ld,
                                            residuals, nconv, iterations, products, b_products, st, form_w);
    return cfs_solver::lobpcg<V, 0, false>(fine, hb, k, tol, scale, maxiter, debug_iters, x0_dev, ld0, eigenvalues, vectors_dev, ld, residuals,
                                           nconv, iterations, products, nullptr, st, form_w);
  }
  bool is_stale() const override { return stale; }
  long long column_cycles() const override { return col_cycles; }

  int apply(void *z_dev, const void *r_dev, hipStream_t st) override {
    if (stale) return cfs_rt::set_err(CFS_HIP_ERR_ARG, "amg_apply: the last refresh failed");
    int rc = follow_fine(st);
    if (rc) return rc;
    rc = cycle(0, OneColumn{}, (V *)z_dev, lv[0]->n, (const V *)r_dev, lv[0]->n, (const int *)cnt.p, st);
    if (rc) return rc;
    HIPCHK(hipGetLastError());
    return 0;
  }

  int info(cfs_hip_amg_info_t *o) override {
    memset(o, 0, sizeof *o);
    o->levels = (int)lv.size();
    o->passes = passes;
    o->degree = degree;
    o->coarse_max = coarse_max;
    o->ratio = ratio;
    o->setup_seconds = setup_seconds;
    o->handles_seconds = handles_seconds;
    long long bytes = (long long)(part.buf.bytes + cnt.bytes);
    for (size_t l = 0; l < lv.size(); ++l) {
      const Level &L = *lv[l];
      o->n[l] = L.n;
      o->nnz[l] = L.nnz;
      o->lmin[l] = L.lmin;
      o->lmax[l] = L.lmax;
      o->kind[l] = L.kind;
      bytes += (long long)L.bytes();
      if (L.owned) {
        cfs_hip_sym_stats s;
        memset(&s, 0, sizeof s);
        L.h->stats(&s);
        bytes += s.device_bytes;
      }
    }
    o->device_bytes = bytes + (refreshable ? map_bytes() - value_map_bytes : 0); // (the handles' stats count their maps)
    return 0;
  }

  int level_aggregates(int level, int *agg, void *w) override {
    if (level < 0 || level + 1 >= (int)lv.size())
      return cfs_rt::set_err(CFS_HIP_ERR_ARG, "amg_level_aggregates: level " + std::to_string(level) + " has no coarser level (" +
                                                  std::to_string(lv.size()) + " levels)");
    const Level &L = *lv[level];
    cfs_rt::DeviceGuard g(device);
    if constexpr (BS >= 2) { // the device holds the map of the nodes: agg[i BS + c] = agg_node[i] BS + c
      if (w)
        return cfs_rt::set_err(CFS_HIP_ERR_ARG, "amg_level_aggregates: a node-block hierarchy has no scalar weights, w must be NULL "
                                                "(cfs_hip_amg_level_node_weights returns its W)");
      if (agg) {
        const size_t m = (size_t)L.n / BS;
        std::vector<int> nagg(m);
        HIPCHK(hipMemcpy(nagg.data(), L.agg.p, m * sizeof(int), hipMemcpyDeviceToHost));
        for (size_t i = 0; i < m; ++i)
          for (int c = 0; c < BS; ++c) agg[i * BS + c] = nagg[i] * BS + c;
      }
      return 0;
    }
    if (agg) HIPCHK(hipMemcpy(agg, L.agg.p, (size_t)L.n * sizeof(int), hipMemcpyDeviceToHost));
    if (w) HIPCHK(hipMemcpy(w, L.w.p, (size_t)L.n * sizeof(V), hipMemcpyDeviceToHost));
    return 0;
  }

  int block() const override { return BS; }

  // W of a level that has a coarser one as m full row-major blocks, unpacked from what the kernels read
  int level_node_weights(int level, void *W) override {
    if (BS == 1)
      return cfs_rt::set_err(CFS_HIP_ERR_ARG, "amg_level_node_weights: the hierarchy was not made by cfs_hip_amg_create_block_* with "
                                              "block > 1 (cfs_hip_amg_level_aggregates returns its w)");
    if (level < 0 || level + 1 >= (int)lv.size())
      return cfs_rt::set_err(CFS_HIP_ERR_ARG, "amg_level_node_weights: level " + std::to_string(level) + " has no coarser level (" +
                                                  std::to_string(lv.size()) + " levels)");
    const Level &L = *lv[level];
    const size_t m = (size_t)L.n / BS;
    std::vector<V> packed(m * tri_words(BS));
    cfs_rt::DeviceGuard g(device);
    HIPCHK(hipMemcpy(packed.data(), L.w.p, packed.size() * sizeof(V), hipMemcpyDeviceToHost));
    V *out = (V *)W;
    for (size_t i = 0; i < m; ++i)
      for (int c = 0; c < BS; ++c)
        for (int e = 0; e <= c; ++e) out[(i * BS + c) * BS + e] = out[(i * BS + e) * BS + c] = packed[(size_t)(c * (c + 1) / 2 + e) * m + i];
    return 0;
  }

  int level_matrix(int level, int *rowptr, int *colind, void *values) override {
    if (level < 1 || level >= (int)lv.size())
      return cfs_rt::set_err(CFS_HIP_ERR_ARG, "amg_level_matrix: level " + std::to_string(level) + " is not one of 1 .. " +
                                                  std::to_string((int)lv.size() - 1) + " (level 0 is the caller's matrix)");
    Level &L = *lv[level];
    if (values && L.va_stale) { // a refresh wrote the values on the device: read them back at the first look
      cfs_rt::DeviceGuard g(device);
      HIPCHK(hipMemcpy(L.va.data(), L.vdev.p, L.va.size() * sizeof(V), hipMemcpyDeviceToHost));
      L.va_stale = false;
    }
    if (rowptr) memcpy(rowptr, L.rp.data(), L.rp.size() * sizeof(int));
    if (colind) memcpy(colind, L.ci.data(), L.ci.size() * sizeof(int));
    if (values) memcpy(values, L.va.data(), L.va.size() * sizeof(V));
    return 0;
  }

  int coarse_inverse(void *inv) override {
    const Level &L = *lv.back();
    if (L.kind != AMG_DENSE) return cfs_rt::set_err(CFS_HIP_ERR_ARG, "amg_coarse_inverse: the hierarchy ends with a smoother-only level");
    cfs_rt::DeviceGuard g(device);
    HIPCHK(hipMemcpy(inv, L.inv.p, (size_t)L.n * L.n * sizeof(V), hipMemcpyDeviceToHost));
    return 0;
  }

  int update_check(long long nnz) override {
    if (!refreshable)
      return cfs_rt::set_err(CFS_HIP_ERR_ARG, "amg_update_values: the hierarchy was made by cfs_hip_amg_create_*, not by "
                                              "cfs_hip_amg_create_refreshable_*");
    if (nnz != nnz_caller)
      return cfs_rt::set_err(CFS_HIP_ERR_ARG, "amg_update_values: " + std::to_string(nnz) + " values, the CSR at create had " +
                                                  std::to_string(nnz_caller));
    return 0;
  }
  int update_values(const void *values_dev, long long nnz, hipStream_t st) override {
    if (int rc = update_check(nnz)) return rc;
    return refresh((const V *)values_dev, st);
  }

  int refresh_info(long long *mb, int *count, double *seconds, double *parts) override {
    if (mb) *mb = refreshable ? map_bytes() : 0;
    if (count) *count = refreshes;
    if (seconds) *seconds = last_seconds;
    if (parts)
      for (int k = 0; k < AMG_T_COUNT; ++k) parts[k] = split[k];
    return 0;
  }

  // cfs_hip_sym_pcg_amg.  u: in = first guess, out = solution
  int pcg(void *u_dev, const void *b_dev, double tol, int maxiter, int *iterations, double *relres, hipStream_t st) override {
    if (stale) return cfs_rt::set_err(CFS_HIP_ERR_ARG, "pcg_amg: the last refresh failed");
    Pcg<V, cfs_hip_sym_s> s;
    cfs_rt::DevBuf zbuf;
    int rc;
    if ((rc = follow_fine(st))) return rc;
    if ((rc = s.begin("pcg_amg", fine, u_dev, b_dev, tol, maxiter, st)) || (rc = alloc_vectors<V>(s.n, {&zbuf})) || (rc = s.first_residual()))
      return rc;
    V *u = s.u, *r = s.r, *p = s.p, *q = s.q, *z = (V *)zbuf.p;
    const long long n = s.n;
    double *pp = s.part.dev();
    int *ic = s.ic;
    // z = M^-1 r;  part[slot] <- r . z of the stored r and the stored final z
    auto cycle_and_dot = [&](int slot) -> int {
      if (int r2 = cycle(0, OneColumn{}, z, n, (const V *)r, n, (const int *)ic, st)) return r2;
      hipLaunchKernelGGL((cg_dot_kernel<V, OneColumn>), dim3(kGrid), dim3(kThreads), 0, st, (const V *)r, (const V *)z, n, n, pp, slot,
                         (const int *)ic, OneColumn{});
      return 0;
    };
    if (s.live()) { // z = M^-1 r, rz[0] = r . z, p = z
      if ((rc = cycle_and_dot((int)P_RZ0))) return rc;
      HIPCHK(hipMemcpyAsync(p, z, (size_t)n * sizeof(V), hipMemcpyDeviceToDevice, st));
    }
    while (s.live()) { // (a window of one: a cycle is more than may be enqueued ahead of the GPU)
      const int it = s.it;
      if ((rc = fine->spmv_local(q, p, nullptr, st))) return rc;
      hipLaunchKernelGGL((cg_dot_kernel<V, OneColumn>), dim3(kGrid), dim3(kThreads), 0, st, (const V *)p, (const V *)q, n, n, pp, (int)P_PQ,
                         (const int *)ic, OneColumn{});
      hipLaunchKernelGGL((cg_update_kernel<V, 0, P_RZ0, OneColumn>), dim3(kGrid), dim3(kThreads), 0, st, u, r, (const V *)p, (const V *)q, n,
                         n, pp, (const int *)ic, it, (const V *)nullptr, 0LL, OneColumn{});
      if ((rc = cycle_and_dot((int)P_RZ0 + ((it + 1) & 1)))) return rc;
      hipLaunchKernelGGL((cg_direction_kernel<V, 0, P_RZ0, OneColumn>), dim3(kGrid), dim3(kThreads), 0, st, p, (const V *)z, n, n,
                         (const double *)pp, ic, it, ColumnStops{{s.stop}}, (const V *)nullptr, 0LL, OneColumn{});
      ++s.it;
      if ((rc = s.look())) return rc;
    }
    return s.finish(iterations, relres);
  }

  // cfs_hip_sym_pcg_amg_cols: pcg() on the columns of blocks U and B (arguments checked by the caller).  One Z block;
  // the cycle runs on the columns still active, every vector kernel of it once for the block, and so do the four
  // kernels of the recurrence; the products stay one per active column.  The host looks after every iteration, as
  // pcg() does, so its mask is exact: the cycle's kernels, which know one flag only, are given the object's own counters
  // (never raised) and the mask alone says which columns they work on.
  int pcg_cols(void *u_dev, const void *b_dev, long long ld, int ncols, double tol, int maxiter, int *iterations, double *relres,
               hipStream_t st) override {
    if (stale) return cfs_rt::set_err(CFS_HIP_ERR_ARG, "pcg_amg_cols: the last refresh failed");
    PcgCols<V, cfs_hip_sym_s> s;
    cfs_rt::DevBuf zbuf;
    int rc;
    if ((rc = follow_fine(st)) || (rc = reserve_cols(ncols))) return rc;
    if ((rc = s.begin("pcg_amg_cols", fine, u_dev, b_dev, ld, ncols, tol, maxiter, 1, st)) ||
        (rc = alloc_vectors<V>((long long)s.block_values(), {&zbuf})) || (rc = s.first_residual()))
      return rc;
    V *u = s.u, *r = s.r, *p = s.p, *q = s.q, *z = (V *)zbuf.p;
    const long long n = s.n;
    double *pp = s.part.dev();
    int *ic = s.ic;
    // Z_c = M^-1 R_c;  part[c][slot] <- r_c . z_c of the stored r and the stored final z, for the active columns
    auto cycle_and_dot = [&](int slot) -> int {
      const ColumnMask cs = s.mask(s.active);
      if (int r2 = cycle(0, cs, z, ld, (const V *)r, ld, (const int *)cnt.p, st)) return r2;
      col_cycles += __builtin_popcount(s.active);
      hipLaunchKernelGGL((cg_dot_kernel<V, ColumnMask>), dim3(kGrid), dim3(kThreads), 0, st, (const V *)r, (const V *)z, ld, n, pp, slot,
                         (const int *)ic, cs);
      return 0;
    };
    if (s.live()) { // Z = M^-1 R, rz[0] = r . z, P = Z
      if ((rc = cycle_and_dot((int)P_RZ0))) return rc;
      int r2 = 0;
      s.mask(s.active).each([&](int c) {
        if (!r2 && hipMemcpyAsync(p + (long long)c * ld, z + (long long)c * ld, (size_t)n * sizeof(V), hipMemcpyDeviceToDevice, st) != hipSuccess)
          r2 = cfs_rt::set_err(CFS_HIP_ERR_DEVICE, "pcg_amg_cols: copying Z to P failed");
      });
      if (r2) return r2;
    }
    while (s.live()) { // (a window of one: a cycle is more than may be enqueued ahead of the GPU)
      const int it = s.it;
      const ColumnMask cs = s.mask(s.active);
      if ((rc = s.products(q, p, s.active))) return rc;
      hipLaunchKernelGGL((cg_dot_kernel<V, ColumnMask>), dim3(kGrid), dim3(kThreads), 0, st, (const V *)p, (const V *)q, ld, n, pp, (int)P_PQ,
                         (const int *)ic, cs);
      hipLaunchKernelGGL((cg_update_kernel<V, 0, P_RZ0, ColumnMask>), dim3(kGrid), dim3(kThreads), 0, st, u, r, (const V *)p, (const V *)q, ld, n,
                         pp, (const int *)ic, it, (const V *)nullptr, 0LL, cs);
      if ((rc = cycle_and_dot((int)P_RZ0 + ((it + 1) & 1)))) return rc;
      hipLaunchKernelGGL((cg_direction_kernel<V, 0, P_RZ0, ColumnMask>), dim3(kGrid), dim3(kThreads), 0, st, p, (const V *)z, ld, n,
                         (const double *)pp, ic, it, s.stop, (const V *)nullptr, 0LL, cs);
      ++s.it;
      if ((rc = s.look())) return rc;
    }
    return s.finish(iterations, relres);
  }
};

} // namespace cfs_solver
