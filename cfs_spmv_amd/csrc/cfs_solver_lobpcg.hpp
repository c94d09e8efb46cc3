// cfs_solver_lobpcg.hpp -- LOBPCG (Knyazev's locally optimal block preconditioned CG) for the k SMALLEST eigenpairs
// of A (cfs_hip_sym_lobpcg), with the preconditioners of the PCG solvers: none, Jacobi, block Jacobi.  The products
// are the tile kernel + fold of the handle; everything else here is tall-skinny dense algebra on two resident blocks
// of 3 k columns, S = [X | W | P] and AS = A S (physical columns X: 0 .. k - 1, W: k .. 2 k - 1, P: 2 k .. 3 k - 1,
// column c at base + c ld, stored in the value type V).  An iteration works on the m <= 3 k ACTIVE columns of them,
// named by an index list that travels as a kernel argument (soft locking: X always whole, W_i and P_i only while pair
// i has not converged).  Every dot product and scalar is fp64, no contracted multiply-adds.
//
//   lobpcg_gram_kernel          part <- the upper triangles of G = S^T S and H = S^T AS, ONE pass over S and AS
//   lobpcg_gram_reduce_kernel   the m (m + 1) sums, once, as doubles                    -> host look 1 (2 m^2 doubles)
//   host                        Rayleigh-Ritz: lobpcg_rr() below (two symeig() of at most 48 x 48), C and theta
//   lobpcg_update_kernel        X <- (V)(S C), P <- (V)(S C'), AX <- (V)(AS C), AP <- (V)(AS C'), in place, row-safe
//   lobpcg_residual_kernel      R_i = AX_i - theta_i X_i;  part <- R_i . R_i, X_i . X_i;  W_i = (V)(M^-1 R_i)
//   lobpcg_reduce_kernel        the 2 k sums                                            -> host look 2 (2 k doubles)
//   tile kernel + fold          AW_i = A W_i for the active i
// Two host looks per iteration are inherent: C depends on G and H, the active set on the norms.
// cfs_hip_sym_lobpcg_amg is the same lobpcg() with W formed outside the residual kernel: that kernel runs in its BS = 0
// form and writes the raw (V)R_i into the W-columns of AS, and the column-blocked multigrid cycle of cfs_solver_amg.hpp
// (Amg::cycle on a ColumnMask) reads them there and writes W_i = M^-1 R_i for the pairs still active.  Memory: no extra k n block.
//
// The Gram kernel is a small SYRK: m (m + 1) sums of n terms each, m <= 48.  One walk per chunk of 8 accumulators
// (eigs_project_kernel) would read its rows 290 times at m = 48; instead a workgroup stages R rows of all 2 m columns
// in LDS, as doubles and ROW-major (one row = [s_0 .. s_mp-1 | t_0 .. t_mp-1 | 2 pad], mp = m rounded up to 4, so a
// row is 2 mp + 2 doubles: 16-byte aligned for 128-bit reads, and 784 bytes at m = 48, NOT a multiple of the 256
// bytes the 64 banks span, so the rows that different lanes of a wave read start in different banks).  A thread owns a
// 4 x 4 register block of pairs -- block (bi, bj), bi <= bj, of G or of H: at most 2 x 78 = 156 tasks at m = 48 -- and,
// where there are fewer tasks than threads, one of nsl = 256 / tasks row slices (rows slice, slice + nsl, ...).  Per
// row it reads 2 x 32 bytes of LDS (lanes with the same block row read the same address: a broadcast) and makes 16
// multiplies and 16 adds: the kernel is bound by the fp64 pipe at m = 48 (32 four-cycle instructions against four
// 128-bit LDS reads per wave and row) and by the stream of S and AS at small m.  16 accumulators + 8 operands in
// registers: 82 VGPRs as compiled (room for five to six waves per SIMD), so the 32 KiB of LDS -- five workgroups of
// four waves per CU, five waves per SIMD -- set the occupancy, not the registers.
// The accumulators live across all row tiles of the workgroup; at the end the slices are added in ascending order
// through LDS and the workgroup writes ONE partial sum per entry.  Fixed grid, fixed order: bit-reproducible.
//
// THE PENCIL A x = lambda B x (cfs_hip_sym_lobpcg_gen, _gen_amg; B a second handle, SPD) is the same templates with a
// compile-time switch GEN and a nullable third block BS = B S, carried along like AS:
//   lobpcg_gram_kernel<V, true>      G = S^T BS and H = S^T AS in ONE pass over the three blocks: a row of the tile is
//                                    [s | t | u | 2 pad], 3 mp + 2 doubles (1168 bytes at m = 48, 96 j + 16 bytes in general:
//                                    never a multiple of 256), and a G task takes its b operand from the u part
//   lobpcg_update_kernel             gridDim.y = 3: BX <- (V)(BS C), BP <- (V)(BS C'), order and rounding of the other two
//   lobpcg_residual_kernel<.., true> R_i = AX_i - theta_i BX_i; the sums stay R_i . R_i and X_i . X_i
//   tile kernel + fold               AW_i = A W_i and BW_i = B W_i; the confirm step recomputes AX and BX
// With the rows per tile of the standard form (lobpcg_gram_rows) the three-block tile takes up to 39936 bytes (mp = 8; 37376
// at mp = 48): kLobTileBytes3 = 40 KiB, FOUR workgroups per CU instead of five.  Fewer rows (24 at m = 48) would have kept
// 32 KiB, at the price of 96-byte runs per fp32 column in the staging loads; the fp64 pipe bounds the kernel at m = 48 and
// four waves per SIMD feed it.  The GEN = false instantiations are the kernels as they were: same stride, same task table,
// same order of summation.  Memory held: (9 k + 1) n values.
#pragma once

#include <algorithm>
#include <cmath>
#include <string>
#include <type_traits>
#include <vector>

namespace cfs_solver {

#define CFS_LOBPCG_ROUNDING _Pragma("clang fp contract(off)")

constexpr int kLobK = CFS_HIP_LOBPCG_MAX_K;
constexpr int kLobM = 3 * kLobK;                 // the widest S
constexpr int kLobTileBytes = 32768;             // LDS of the Gram kernel: a row tile, later the slices' accumulators
static_assert(kLobM % 4 == 0 && (kLobM / 4) * (kLobM / 4 + 1) / 2 + (kLobM / 4) * (kLobM / 4) <= kThreads,
              "one 4 x 4 register block of G or H per thread");
static_assert(kThreads * 16 * sizeof(double) <= kLobTileBytes, "the slices' accumulators fit the tile");
// the pencil form stages three blocks: a row is 3 mp + 2 doubles, and with the SAME rows per tile (lobpcg_gram_rows) the
// tile is at most 39936 bytes (mp = 8: 192 rows of 208 bytes; 37376 at mp = 48): 40 KiB, four workgroups per CU
constexpr int kLobTileBytes3 = 40960;
constexpr int lobpcg_tile3_bytes(int mp) { return 32 * (8 < kLobM / mp ? 8 : kLobM / mp) * (3 * mp + 2) * (int)sizeof(double); }
static_assert(lobpcg_tile3_bytes(4) <= kLobTileBytes3 && lobpcg_tile3_bytes(8) <= kLobTileBytes3 && lobpcg_tile3_bytes(12) <= kLobTileBytes3 &&
                  lobpcg_tile3_bytes(16) <= kLobTileBytes3 && lobpcg_tile3_bytes(20) <= kLobTileBytes3 && lobpcg_tile3_bytes(24) <= kLobTileBytes3 &&
                  lobpcg_tile3_bytes(28) <= kLobTileBytes3 && lobpcg_tile3_bytes(32) <= kLobTileBytes3 && lobpcg_tile3_bytes(36) <= kLobTileBytes3 &&
                  lobpcg_tile3_bytes(40) <= kLobTileBytes3 && lobpcg_tile3_bytes(44) <= kLobTileBytes3 && lobpcg_tile3_bytes(48) <= kLobTileBytes3,
              "the three-block row tile fits at every width");

struct LobpcgCols { // the active columns of S (and of AS): physical column idx[j] is column j of this iteration
  int m;
  int idx[kLobM];
};
struct LobpcgTheta {
  double theta[kLobK];
  unsigned active; // bit i: W_i is wanted
};

// rows of a Gram tile for m columns: 32 .. 256, the tile within kLobTileBytes
inline int lobpcg_gram_rows(int m) {
  const int mp = (m + 3) & ~3;
  return 32 * std::max(1, std::min(8, kLobM / mp));
}
// block task `task` of the Gram kernel -> (which: 0 = G, 1 = H; block row; block column)
__host__ __device__ inline void lobpcg_task(int task, int nb, int full_h, int &which, int &bi, int &bj) {
  const int ntri = nb * (nb + 1) / 2;
  which = task >= ntri;
  if (which) task -= ntri;
  if (which && full_h) {
    bi = task / nb;
    bj = task % nb;
    return;
  }
  bi = 0;
  while (task >= nb - bi) {
    task -= nb - bi;
    ++bi;
  }
  bj = bi + task;
}

// column c <- the default start block: x0[i, c] = eigs_default_v0(i + offset), offset = c n
template <typename V>
__global__ void __launch_bounds__(kThreads) lobpcg_fill_kernel(V *__restrict__ x, long long n, long long offset) {
  for (long long i = (long long)blockIdx.x * kThreads + threadIdx.x; i < n; i += (long long)gridDim.x * kThreads)
    x[i] = (V)eigs_default_v0(i + offset);
}

// part[(w m m + i m + j) kGrid + workgroup] <- this workgroup's share of column i of s . column j of s (w = 0) or of
// t (w = 1), for i <= j (full_h: every (i, j) of w = 1).  Launched with kGrid workgroups and kLobTileBytes of LDS.
// GEN, the pencil form (kLobTileBytes3 of LDS): a third block u = B S is staged behind t, a row is [s | t | u | 2 pad],
// and a task of w = 0 takes its b operand from u: part of w = 0 is column i of s . column j of u, G = S^T (B S).
template <typename V, bool GEN>
__global__ void __launch_bounds__(kThreads)
    lobpcg_gram_kernel(const V *__restrict__ s, const V *__restrict__ t, const V *__restrict__ u, long long ld, long long n,
                       LobpcgCols cols, int R, int full_h, double *__restrict__ part) {
  CFS_LOBPCG_ROUNDING
  extern __shared__ __align__(16) unsigned char lobpcg_lds[];
  __shared__ int sidx[kLobM];
  double *tile = reinterpret_cast<double *>(lobpcg_lds); // tile[r stride + c], c < mp: s, mp <= c < 2 mp: t, then u
  constexpr int NBLK = GEN ? 3 : 2;
  const int m = cols.m, mp = (m + 3) & ~3, nb = mp / 4, stride = NBLK * mp + 2;
  const int ntri = nb * (nb + 1) / 2, nt = ntri + (full_h ? nb * nb : ntri);
  const int nsl = min(kThreads / nt, R);
  const int task = threadIdx.x % nt, slice = threadIdx.x / nt;
  for (int j = threadIdx.x; j < m; j += kThreads) sidx[j] = cols.idx[j];
  int which, bi, bj;
  lobpcg_task(task, nb, full_h, which, bi, bj);
  const int ao = 4 * bi, bo = (which ? mp : GEN ? 2 * mp : 0) + 4 * bj;
  double acc[4][4];
#pragma unroll
  for (int e = 0; e < 4; ++e)
#pragma unroll
    for (int f = 0; f < 4; ++f) acc[e][f] = 0.0;
  __syncthreads();
  const long long ntiles = (n + R - 1) / R;
  for (long long tl = blockIdx.x; tl < ntiles; tl += gridDim.x) {
    const long long row0 = tl * R;
    // (consecutive threads read consecutive rows of one column: coalesced; rows and columns outside count as 0)
    for (int e = threadIdx.x; e < NBLK * mp * R; e += kThreads) {
      const int c = e / R, r = e - c * R, cc = c < mp ? c : c < 2 * mp ? c - mp : c - 2 * mp;
      double v = 0.0;
      if (cc < m && row0 + r < n) v = (double)(c < mp ? s : (!GEN || c < 2 * mp) ? t : u)[(long long)sidx[cc] * ld + row0 + r];
      tile[r * stride + c] = v;
    }
    __syncthreads();
    if (slice < nsl)
      for (int r = slice; r < R; r += nsl) {
        const double *row = tile + r * stride;
        double a[4], b[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          a[e] = row[ao + e];
          b[e] = row[bo + e];
        }
#pragma unroll
        for (int e = 0; e < 4; ++e)
#pragma unroll
          for (int f = 0; f < 4; ++f) acc[e][f] = acc[e][f] + a[e] * b[f];
      }
    __syncthreads(); // (the next tile is staged over this one)
  }
  // the slices of a task, added in ascending order; one partial sum per entry and workgroup
  double *red = tile; // red[(slice nt + task) 16 + 4 e + f]
  if (slice < nsl)
#pragma unroll
    for (int e = 0; e < 4; ++e)
#pragma unroll
      for (int f = 0; f < 4; ++f) red[(slice * nt + task) * 16 + 4 * e + f] = acc[e][f];
  __syncthreads();
  for (int c = threadIdx.x; c < nt * 16; c += kThreads) {
    double sum = red[c];
    for (int sl = 1; sl < nsl; ++sl) sum = sum + red[sl * nt * 16 + c];
    lobpcg_task(c / 16, nb, full_h, which, bi, bj);
    const int i = 4 * bi + (c % 16) / 4, j = 4 * bj + c % 4;
    if (i < m && j < m && (j >= i || (which && full_h)))
      part[(long long)(which * m * m + i * m + j) * kGrid + blockIdx.x] = sum;
  }
}

// out[slot] <- the sum of the kGrid partial sums of entry slot = w m m + i m + j, one workgroup each, in the order of
// slot_sum; the entries the Gram kernel does not produce (j < i) are skipped.  Launched with 2 m m workgroups.
__global__ void __launch_bounds__(kThreads)
    lobpcg_gram_reduce_kernel(const double *__restrict__ part, double *__restrict__ out, int m, int full_h) {
  const int slot = blockIdx.x, which = slot / (m * m), i = (slot - which * m * m) / m, j = slot % m;
  if (j < i && !(which && full_h)) return;
  const double s = slot_sum(part, slot);
  if (threadIdx.x == 0) out[slot] = s;
}
// out[slot] <- the sum of part[slot], one workgroup per slot
__global__ void __launch_bounds__(kThreads) lobpcg_reduce_kernel(const double *__restrict__ part, double *__restrict__ out) {
  const double s = slot_sum(part, blockIdx.x);
  if (threadIdx.x == 0) out[blockIdx.x] = s;
}

// Step 3.  buf = sbuf (blockIdx.y = 0), asbuf (1) or bsbuf (2: the pencil form's B S), 3 k physical columns each.  With the m active columns S of buf:
// column o <- (V)(S c[:, o]) for o < k (X / AX) and, with_p, column 2 k + o <- (V)(S c[:, k + o]) (P / AP); c is m x nout
// row-major, nout = k or 2 k.  fp64, columns ascending, rounded once when stored.  Row-safe IN PLACE: a workgroup
// stages all m columns of its R = 256 / sizeof(V) rows in LDS before it writes any of them -- X and P both come from
// the same staged rows -- and no other workgroup touches those rows.  Thread (r, g) of R x (kThreads / R) owns row r
// and the outputs g, g + G, ... in chunks of 8.  LDS: m nout doubles, then m R values.
template <typename V>
__global__ void __launch_bounds__(kThreads)
    lobpcg_update_kernel(V *sbuf, V *asbuf, V *bsbuf, long long ld, long long n, LobpcgCols cols, int k, int with_p,
                         const double *__restrict__ c) {
  CFS_LOBPCG_ROUNDING
  extern __shared__ __align__(16) unsigned char lobpcg_lds[];
  __shared__ int sidx[kLobM];
  const int m = cols.m, nout = with_p ? 2 * k : k;
  double *cs = reinterpret_cast<double *>(lobpcg_lds);
  V *tile = reinterpret_cast<V *>(cs + m * nout); // tile[j R + r]
  V *buf = blockIdx.y == 0 ? sbuf : blockIdx.y == 1 ? asbuf : bsbuf;
  constexpr int R = 256 / (int)sizeof(V), G = kThreads / R;
  const int r = threadIdx.x % R, g = threadIdx.x / R;
  for (int j = threadIdx.x; j < m; j += kThreads) sidx[j] = cols.idx[j];
  for (int e = threadIdx.x; e < m * nout; e += kThreads) cs[e] = c[e];
  __syncthreads();
  const long long ntiles = (n + R - 1) / R;
  for (long long tl = blockIdx.x; tl < ntiles; tl += gridDim.x) {
    const long long row0 = tl * R;
    for (int e = threadIdx.x; e < m * R; e += kThreads) {
      const int j = e / R, rr = e % R;
      tile[e] = row0 + rr < n ? buf[(long long)sidx[j] * ld + row0 + rr] : (V)0;
    }
    __syncthreads();
    if (row0 + r < n)
      for (int o0 = g; o0 < nout; o0 += G * 8) {
        double acc[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) acc[e] = 0.0;
        for (int j = 0; j < m; ++j) {
          const double a = (double)tile[j * R + r];
          const double *cj = cs + j * nout;
#pragma unroll
          for (int e = 0; e < 8; ++e) {
            const int o = o0 + e * G;
            if (o < nout) acc[e] = acc[e] + a * cj[o];
          }
        }
#pragma unroll
        for (int e = 0; e < 8; ++e) {
          const int o = o0 + e * G;
          if (o < nout) buf[(long long)(o < k ? o : k + o) * ld + row0 + r] = (V)acc[e];
        }
      }
    __syncthreads(); // (the next tile is staged over this one)
  }
}

// Step 4, one kernel.  For every pair i < k: R_i = AX_i - theta_i X_i in fp64 from the stored values;
// part[2 i] <- R_i . R_i, part[2 i + 1] <- X_i . X_i;  for the active i: W_i = (V)(M^-1 R_i), formed in fp64 from the
// stored inverse diagonal (BS = 1, the words of cg_dinv_kernel) or inverse node blocks (BS >= 2, the packed words of
// cg_binv_kernel through block_apply(), as the PCG kernels form z; the rows of a trailing partial block that lie
// outside the matrix count as 0 and are not written);  BS = 0: W_i = (V)R_i.  x, ax, w: column 0 of X, AX and W.
// One node block per thread, grid-stride; the pairs in chunks of 8 (16 accumulators).
// GEN, the pencil form: R_i = AX_i - theta_i BX_i with bx column 0 of BX; part[2 i + 1] stays X_i . X_i.
template <typename V, int BS, bool GEN>
__global__ void __launch_bounds__(kThreads)
    lobpcg_residual_kernel(const V *__restrict__ x, const V *__restrict__ ax, const V *__restrict__ bx, V *__restrict__ w, long long ld,
                           long long n, int k, LobpcgTheta th, const V *__restrict__ minv, long long nb, double *__restrict__ part) {
  CFS_LOBPCG_ROUNDING
  constexpr int B = BS < 1 ? 1 : BS;
  __shared__ double stheta[kLobK];
  if (threadIdx.x < kLobK) stheta[threadIdx.x] = th.theta[threadIdx.x];
  __syncthreads();
  for (int c0 = 0; c0 < k; c0 += 8) {
    double acc[16];
#pragma unroll
    for (int e = 0; e < 16; ++e) acc[e] = 0.0;
    for (long long kb = (long long)blockIdx.x * kThreads + threadIdx.x; kb < nb; kb += (long long)gridDim.x * kThreads) {
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const int col = c0 + e;
        if (col >= k) continue;
        const double theta = stheta[col];
        const long long base = (long long)col * ld;
        double rd[B], z[B];
#pragma unroll
        for (int i = 0; i < B; ++i) {
          const long long gi = kb * B + i;
          rd[i] = 0.0;
          if (gi < n) {
            const double xk = (double)x[base + gi];
            double d;
            if constexpr (GEN)
              d = (double)ax[base + gi] - theta * (double)bx[base + gi];
            else
              d = (double)ax[base + gi] - theta * xk;
            rd[i] = d;
            acc[2 * e] = acc[2 * e] + d * d;
            acc[2 * e + 1] = acc[2 * e + 1] + xk * xk;
          }
        }
        if (!((th.active >> col) & 1u)) continue;
        if constexpr (BS == 0) {
          z[0] = rd[0];
        } else if constexpr (BS == 1) {
          z[0] = rd[0] * (double)minv[kb];
        } else {
          block_apply<V, BS>(minv, nb, kb, rd, z);
        }
#pragma unroll
        for (int i = 0; i < B; ++i) {
          const long long gi = kb * B + i;
          if (gi < n) w[base + gi] = (V)z[i];
        }
      }
    }
    double total;
    block_sum_n<16>(acc, total);
    if (threadIdx.x < 16 && c0 + (int)threadIdx.x / 2 < k)
      part[(long long)(2 * c0 + threadIdx.x) * kGrid + blockIdx.x] = total;
  }
}

// ---- step 2, on the host, fp64 (cfs_hip_debug_lobpcg_rr) ----
// g, hh: m x m row-major, the upper triangles are read.  d_j = G_jj^-1/2, a column whose G_jj is not finite and > 0
// is dropped;  symeig(D G D), the eigenvectors with w > drop w_max are kept;  Q = D U w^-1/2;  T = Q^T H Q,
// symmetrised;  symeig(T);  c = Q Z[:, :k] (m x k row-major, zero rows for dropped columns), theta = the k smallest.
// *rank = columns of Q; with rank < k the trailing theta and columns of c are 0.  Returns 0, -1: an entry that is not
// finite, or no convergence of symeig.
inline int lobpcg_rr(int m, const double *g, const double *hh, int k, double drop, double *theta, double *c, int *rank) {
  auto G = [&](int i, int j) { return i <= j ? g[(size_t)i * m + j] : g[(size_t)j * m + i]; };
  auto H = [&](int i, int j) { return i <= j ? hh[(size_t)i * m + j] : hh[(size_t)j * m + i]; };
  std::fill(theta, theta + k, 0.0);
  std::fill(c, c + (size_t)m * k, 0.0);
  *rank = 0;
  std::vector<int> keep;
  std::vector<double> d(m, 0.0);
  for (int j = 0; j < m; ++j) {
    const double gjj = G(j, j);
    if (gjj > 0.0 && std::isfinite(gjj) && std::isfinite(1.0 / std::sqrt(gjj))) {
      d[j] = 1.0 / std::sqrt(gjj);
      keep.push_back(j);
    }
  }
  const int mk = (int)keep.size();
  if (mk == 0) return 0;
  std::vector<double> B((size_t)mk * mk), w(mk), U((size_t)mk * mk);
  for (int a = 0; a < mk; ++a)
    for (int b = 0; b < mk; ++b) {
      const double v = d[keep[a]] * G(keep[a], keep[b]) * d[keep[b]];
      if (!std::isfinite(v) || !std::isfinite(H(keep[a], keep[b]))) return -1;
      B[(size_t)a * mk + b] = v;
    }
  if (symeig(mk, B.data(), w.data(), U.data()) < 0) return -1;
  const double wmax = w[mk - 1];
  int first = 0; // (w ascending: the kept eigenvectors are first .. mk - 1)
  while (first < mk && !(w[first] > drop * wmax)) ++first;
  const int r = mk - first;
  *rank = r;
  if (r == 0) return 0;
  std::vector<double> Q((size_t)m * r, 0.0), HQ((size_t)m * r, 0.0), T((size_t)r * r), tw(r), Z((size_t)r * r);
  for (int a = 0; a < mk; ++a)
    for (int q = 0; q < r; ++q) Q[(size_t)keep[a] * r + q] = d[keep[a]] * U[(size_t)a * mk + first + q] / std::sqrt(w[first + q]);
  for (int a = 0; a < mk; ++a)
    for (int q = 0; q < r; ++q) {
      double s = 0.0;
      for (int b = 0; b < mk; ++b) s += H(keep[a], keep[b]) * Q[(size_t)keep[b] * r + q];
      HQ[(size_t)keep[a] * r + q] = s;
    }
  for (int p = 0; p < r; ++p)
    for (int q = 0; q < r; ++q) {
      double s = 0.0;
      for (int a = 0; a < mk; ++a) s += Q[(size_t)keep[a] * r + p] * HQ[(size_t)keep[a] * r + q];
      T[(size_t)p * r + q] = s;
    }
  for (int p = 0; p < r; ++p)
    for (int q = p + 1; q < r; ++q) T[(size_t)p * r + q] = T[(size_t)q * r + p] = 0.5 * (T[(size_t)p * r + q] + T[(size_t)q * r + p]);
  if (symeig(r, T.data(), tw.data(), Z.data()) < 0) return -1;
  const int kk = std::min(k, r);
  for (int i = 0; i < kk; ++i) {
    theta[i] = tw[i];
    for (int a = 0; a < mk; ++a) {
      double s = 0.0;
      for (int q = 0; q < r; ++q) s += Q[(size_t)keep[a] * r + q] * Z[(size_t)q * r + i];
      c[(size_t)keep[a] * k + i] = s;
    }
  }
  return 0;
}

// ---- launches shared by the solver and the developer entry points ----
// (u: the third block B S of the pencil form, G = S^T u; nullptr: the standard form, G = S^T S)
template <typename V>
int lobpcg_gram(const V *s, const V *t, const V *u, long long ld, long long n, const LobpcgCols &cols, int full_h, double *part,
                double *out, double *g, double *hh, hipStream_t st) {
  const int m = cols.m;
  if (u)
    hipLaunchKernelGGL((lobpcg_gram_kernel<V, true>), dim3(kGrid), dim3(kThreads), kLobTileBytes3, st, s, t, u, ld, n, cols,
                       lobpcg_gram_rows(m), full_h, part);
  else
    hipLaunchKernelGGL((lobpcg_gram_kernel<V, false>), dim3(kGrid), dim3(kThreads), kLobTileBytes, st, s, t, u, ld, n, cols,
                       lobpcg_gram_rows(m), full_h, part);
  hipLaunchKernelGGL(lobpcg_gram_reduce_kernel, dim3(2 * m * m), dim3(kThreads), 0, st, (const double *)part, out, m, full_h);
  HIPCHK(hipGetLastError());
  std::vector<double> host((size_t)2 * m * m);
  HIPCHK(hipMemcpyAsync(host.data(), out, host.size() * sizeof(double), hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  for (int i = 0; i < m; ++i)
    for (int j = 0; j < m; ++j) {
      g[(size_t)i * m + j] = host[(size_t)(i <= j ? i * m + j : j * m + i)];
      hh[(size_t)i * m + j] = host[(size_t)m * m + (i <= j || full_h ? i * m + j : j * m + i)];
    }
  return 0;
}
inline size_t lobpcg_gram_part_bytes(int m) { return (size_t)2 * m * m * kGrid * sizeof(double); }

template <typename V>
int lobpcg_update(V *sbuf, V *asbuf, V *bsbuf, long long ld, long long n, const LobpcgCols &cols, int k, int with_p,
                  const double *c_host, double *c_dev, hipStream_t st) {
  const int nout = with_p ? 2 * k : k;
  // (c_host stays as it is until the stream has been synchronised again: the callers see to that)
  HIPCHK(hipMemcpyAsync(c_dev, c_host, (size_t)cols.m * nout * sizeof(double), hipMemcpyHostToDevice, st));
  constexpr int R = 256 / (int)sizeof(V);
  const long long ntiles = (n + R - 1) / R;
  // (bsbuf goes with asbuf: the callers see to that)
  hipLaunchKernelGGL((lobpcg_update_kernel<V>), dim3((unsigned)std::min<long long>(ntiles, 2 * kGrid), bsbuf ? 3 : asbuf ? 2 : 1),
                     dim3(kThreads), (size_t)cols.m * nout * sizeof(double) + (size_t)cols.m * R * sizeof(V), st, sbuf, asbuf, bsbuf, ld, n,
                     cols, k, with_p, (const double *)c_dev);
  HIPCHK(hipGetLastError());
  return 0;
}

// The preconditioner of the iteration, exactly as cfs_hip_sym_pcg / _pcg_block build theirs (Precond, cfs_solver.hpp); a
// diagonal entry or a block that is not positive (definite) is refused after a look of its own, and the gathered blocks
// are freed with it.  BS = 0: nothing, and no look.  part: kLobSlots slots, zeroed.
constexpr int kLobSlots = P_COUNT > 2 * kLobK ? (int)P_COUNT : 2 * kLobK;
template <typename V, int BS, class Handle> int lobpcg_precond(Handle *h, Precond<V, BS> &pre, Slots &part) {
  if constexpr (BS >= 1) {
    int rc;
    if ((rc = pre.setup(h, part.dev(), part.st)) || (rc = part.fetch()) || (rc = pre.check("lobpcg", part, h->n()))) return rc;
    pre.blkbuf = cfs_rt::DevBuf();
  }
  return 0;
}

// step 4 and the host's look: sums[2 i] = R_i . R_i, sums[2 i + 1] = X_i . X_i (host, 2 k doubles); W_i written for the
// bits set in `active`.  x, ax, w: column 0 of X, AX and W;  out_dev: 2 k doubles.  Waits for the stream.
// GEN: R_i = AX_i - theta_i BX_i, bx column 0 of BX (otherwise bx is not read).
template <typename V, int BS, bool GEN = false>
int lobpcg_residual(const V *x, const V *ax, const V *bx, V *w, long long ld, long long n, int k, const double *theta, unsigned active,
                    const V *minv, double *part, double *out_dev, double *sums, hipStream_t st) {
  constexpr int B = BS < 1 ? 1 : BS;
  const long long nb = (n + B - 1) / B;
  LobpcgTheta th;
  for (int i = 0; i < kLobK; ++i) th.theta[i] = i < k ? theta[i] : 0.0;
  th.active = active;
  hipLaunchKernelGGL((lobpcg_residual_kernel<V, BS, GEN>), dim3(kGrid), dim3(kThreads), 0, st, x, ax, bx, w, ld, n, k, th, minv, nb, part);
  hipLaunchKernelGGL(lobpcg_reduce_kernel, dim3(2 * k), dim3(kThreads), 0, st, (const double *)part, out_dev);
  HIPCHK(hipGetLastError());
  HIPCHK(hipMemcpyAsync(sums, out_dev, (size_t)2 * k * sizeof(double), hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  return 0;
}


// cfs_hip_debug_gram_cols (cfs_hip_debug_gram: the identity list and full_h = 1); cfs_hip_debug_gram3_cols: u_dev, the
// third block, and full_h = 0
template <typename V>
int debug_gram(const void *s_dev, const void *t_dev, const void *u_dev, long long ld, long long n, int m, const int *idx, int full_h,
               double *g, double *hh, hipStream_t st) {
  cfs_rt::DevBuf pbuf, obuf;
  int rc;
  if ((rc = pbuf.alloc(lobpcg_gram_part_bytes(m))) || (rc = obuf.alloc((size_t)2 * m * m * sizeof(double)))) return rc;
  LobpcgCols cols;
  cols.m = m;
  for (int j = 0; j < kLobM; ++j) cols.idx[j] = j < m ? idx[j] : 0;
  return lobpcg_gram<V>((const V *)s_dev, (const V *)t_dev, (const V *)u_dev, ld, n, cols, full_h, (double *)pbuf.p, (double *)obuf.p, g,
                        hh, st);
}

// cfs_hip_debug_lobpcg_update_cols (cfs_hip_debug_lobpcg_update: the identity list, with_p = 1, no second block);
// cfs_hip_debug_lobpcg_update3_cols: bs_dev, the third block
template <typename V>
int debug_update(void *s_dev, void *as_dev, void *bs_dev, long long ld, long long n, int k, int m, const int *idx, int with_p,
                 const double *c, hipStream_t st) {
  cfs_rt::DevBuf cbuf;
  int rc;
  if ((rc = cbuf.alloc((size_t)m * 2 * k * sizeof(double)))) return rc;
  LobpcgCols cols;
  cols.m = m;
  for (int j = 0; j < kLobM; ++j) cols.idx[j] = j < m ? idx[j] : 0;
  if ((rc = lobpcg_update<V>((V *)s_dev, (V *)as_dev, (V *)bs_dev, ld, n, cols, k, with_p, c, (double *)cbuf.p, st))) return rc;
  HIPCHK(hipStreamSynchronize(st));
  return 0;
}

// cfs_hip_sym_debug_lobpcg_residual: the solver's preconditioner set-up, then step 4 alone (bx_dev: _residual_gen)
template <typename V, int BS, class Handle>
int debug_residual(Handle *h, const void *x_dev, const void *ax_dev, const void *bx_dev, void *w_dev, long long ld, int k,
                   const double *theta, unsigned active, double *sums, hipStream_t st) {
  cfs_rt::DevBuf nout;
  Slots part;
  Precond<V, BS> pre;
  int rc;
  if ((rc = part.alloc(kLobSlots, st)) || (rc = nout.alloc((size_t)2 * kLobK * sizeof(double))) || (rc = part.zero()) ||
      (rc = lobpcg_precond<V, BS>(h, pre, part)))
    return rc;
  std::vector<double> hn(2 * kLobK);
  if (bx_dev)
    rc = lobpcg_residual<V, BS, true>((const V *)x_dev, (const V *)ax_dev, (const V *)bx_dev, (V *)w_dev, ld, h->n(), k, theta, active,
                                      pre.minv(), part.dev(), (double *)nout.p, hn.data(), st);
  else
    rc = lobpcg_residual<V, BS, false>((const V *)x_dev, (const V *)ax_dev, nullptr, (V *)w_dev, ld, h->n(), k, theta, active, pre.minv(),
                                       part.dev(), (double *)nout.p, hn.data(), st);
  if (rc) return rc;
  std::copy(hn.begin(), hn.begin() + 2 * k, sums);
  return 0;
}

// cfs_hip_sym_lobpcg, and with debug_iters >= 0 cfs_hip_sym_debug_lobpcg: iteration 0 and debug_iters more, every
// pair active, no convergence test, no confirm step (arguments checked by the caller).
// HOW W IS FORMED is the one thing the iteration leaves open.  form_w = nullptr: by the residual kernel itself from the
// stored M^-1 of BS.  Otherwise (cfs_hip_sym_lobpcg_amg, BS = 0): the residual kernel writes the raw (V)R_i into the
// W-columns of AS -- free at that moment: the products of step 6 rewrite them before anything reads them, so no extra
// block is held -- and form_w(W, R, ld, k, mask) enqueues W_i = M^-1 R_i for the bits of mask (column i at + i ld).
// GEN (cfs_hip_sym_lobpcg_gen, _gen_amg, _debug_lobpcg_gen): the pencil A x = lambda B x, B the handle hb (hb == h is
// allowed).  A third resident block BS = B S is carried along like AS -- by products where AS is (the start block, the
// W columns of step 6, the confirm step) and by the update kernel where AS is -- G = S^T BS, R_i = AX_i - theta_i BX_i;
// the W-columns of BS are as free after step 4 as those of AS.  Without GEN hb and b_products_out are not looked at.
template <typename V, int BS, bool GEN, class Handle, class FormW = std::nullptr_t>
int lobpcg(Handle *h, Handle *hb, int k, double tol, double scale, int maxiter, int debug_iters, const void *x0_dev, long long ld0,
           double *eigenvalues, void *vectors_dev, long long ldx, double *residuals, int *nconv_out, int *iterations_out,
           int *products_out, int *b_products_out, hipStream_t st, FormW form_w = nullptr) {
  using cfs_rt::DevBuf;
  constexpr bool external_w = !std::is_same<FormW, std::nullptr_t>::value;
  static_assert(!external_w || BS == 0, "an external M^-1 reads the raw residuals");
  const bool debug = debug_iters >= 0;
  const long long n = h->n();
  const long long ld = (n + Vec16<V>::W - 1) / Vec16<V>::W * Vec16<V>::W; // columns 16-byte aligned
  const int mmax = 3 * k;
  const double unit = sizeof(V) == 8 ? 0x1p-53 : 0x1p-24, drop = 64.0 * unit;
  DevBuf sb, asb, bsb, gpart, gout, cdev, nout;
  Slots slots;
  Precond<V, BS> pre;
  int rc;
  if ((rc = sb.alloc((size_t)mmax * ld * sizeof(V) + 64)) || (rc = asb.alloc((size_t)mmax * ld * sizeof(V) + 64)) ||
      (GEN && (rc = bsb.alloc((size_t)mmax * ld * sizeof(V) + 64))) || (rc = slots.alloc(kLobSlots, st)) ||
      (rc = gpart.alloc(lobpcg_gram_part_bytes(mmax))) || (rc = gout.alloc((size_t)2 * mmax * mmax * sizeof(double))) ||
      (rc = cdev.alloc((size_t)mmax * 2 * k * sizeof(double))) || (rc = nout.alloc((size_t)2 * kLobK * sizeof(double))))
    return rc;
  V *S = (V *)sb.p, *AS = (V *)asb.p, *BSb = GEN ? (V *)bsb.p : nullptr;
  double *part = slots.dev();
  auto col = [&](V *base, int c) { return base + (long long)c * ld; };
  if ((rc = slots.zero())) return rc;
  // the preconditioner; refused before anything else happens
  if ((rc = lobpcg_precond<V, BS>(h, pre, slots))) return rc;
  const V *minv = pre.minv();
  int products = 0, b_products = 0, it = 0;
  auto product = [&](int c) -> int { // AS[:, c] = A S[:, c]; GEN: and BS[:, c] = B S[:, c]
    ++products;
    if (int r2 = h->spmv_local(col(AS, c), col(S, c), nullptr, st)) return r2;
    if constexpr (GEN) {
      ++b_products;
      return hb->spmv_local(col(BSb, c), col(S, c), nullptr, st);
    }
    return 0;
  };
  // X0
  for (int c = 0; c < k; ++c) {
    if (x0_dev)
      HIPCHK(hipMemcpyAsync(col(S, c), (const V *)x0_dev + (long long)c * ld0, (size_t)n * sizeof(V), hipMemcpyDeviceToDevice, st));
    else
      hipLaunchKernelGGL((lobpcg_fill_kernel<V>), dim3(kGrid), dim3(kThreads), 0, st, col(S, c), n, (long long)c * n);
    if ((rc = product(c))) return rc;
  }
  HIPCHK(hipGetLastError());
  std::vector<double> G((size_t)mmax * mmax), H((size_t)mmax * mmax), theta(k, 0.0), C((size_t)mmax * k), pack((size_t)mmax * 2 * k),
      res(k, 0.0), hn(2 * kLobK);
  LobpcgCols cols;
  for (int j = 0; j < kLobM; ++j) cols.idx[j] = 0;
  const unsigned all = (1u << k) - 1u;
  // steps 1 - 3 on the columns in `cols`
  auto rayleigh_ritz = [&](int *rank) -> int {
    const int m = cols.m;
    int r2 = lobpcg_gram<V>(S, AS, BSb, ld, n, cols, 0, (double *)gpart.p, (double *)gout.p, G.data(), H.data(), st);
    if (r2) return r2;
    if (lobpcg_rr(m, G.data(), H.data(), k, drop, theta.data(), C.data(), rank) < 0)
      return cfs_rt::set_err(CFS_HIP_ERR_INTERNAL, "lobpcg: the projected eigenproblem has entries that are not finite, or did not converge");
    const int with_p = m > k;
    const int no = with_p ? 2 * k : k;
    for (int j = 0; j < m; ++j)
      for (int o = 0; o < no; ++o) pack[(size_t)j * no + o] = o < k ? C[(size_t)j * k + o] : (j < k ? 0.0 : C[(size_t)j * k + o - k]);
    return lobpcg_update<V>(S, AS, BSb, ld, n, cols, k, with_p, pack.data(), (double *)cdev.p, st);
  };
  // step 4 and the host's look at the norms: res[i] = ||R_i|| / ||X_i||
  auto norms = [&](unsigned wmask) -> int {
    int r2 = lobpcg_residual<V, BS, GEN>((const V *)S, (const V *)AS, (const V *)BSb, col(external_w ? AS : S, k), ld, n, k, theta.data(),
                                         wmask, minv, part, (double *)nout.p, hn.data(), st);
    if (r2) return r2;
    if constexpr (external_w)
      if (wmask && (r2 = form_w(col(S, k), (const V *)col(AS, k), ld, k, wmask))) return r2;
    for (int i = 0; i < k; ++i) res[i] = std::sqrt(hn[2 * i]) / std::sqrt(hn[2 * i + 1]);
    return 0;
  };
  const double thr = tol * scale;
  auto unconverged = [&]() {
    unsigned a = 0;
    for (int i = 0; i < k; ++i)
      if (debug || !(res[i] <= thr)) a |= 1u << i; // (a NaN counts as not converged)
    return a;
  };
  // iteration 0: S = X0.  A start block that is short of rank k (dependent or zero columns) leaves zero columns
  // behind; they are filled from the default sequence, further along, and iteration 0 is made again
  for (int attempt = 0;; ++attempt) {
    cols.m = k;
    for (int j = 0; j < k; ++j) cols.idx[j] = j;
    int rank = 0;
    if ((rc = rayleigh_ritz(&rank))) return rc;
    if (rank == k) break;
    if (attempt == 2)
      return cfs_rt::set_err(CFS_HIP_ERR_ARG, GEN ? "lobpcg_gen: the start block does not have rank k in the B inner product: B may not be "
                                                    "positive definite"
                                                  : "lobpcg: the start block does not have rank k");
    for (int c = rank; c < k; ++c) {
      hipLaunchKernelGGL((lobpcg_fill_kernel<V>), dim3(kGrid), dim3(kThreads), 0, st, col(S, c), n, (long long)(k * (attempt + 1) + c) * n);
      if ((rc = product(c))) return rc;
    }
  }
  if ((rc = norms(all))) return rc;
  bool fresh = false, have_p = false;
  unsigned wmask = all;
  for (;;) {
    unsigned act = unconverged();
    if (!debug && act == 0) {
      if (fresh) break;
      // step 5: the implicit residuals pass; AX = A X afresh, and they must pass again
      for (int c = 0; c < k; ++c)
        if ((rc = product(c))) return rc;
      if ((rc = norms(all))) return rc;
      wmask = all;
      fresh = true;
      continue;
    }
    if (it >= (debug ? debug_iters : maxiter)) break;
    if (act & ~wmask) { // a pair that had converged and no longer does: its W has not been formed
      if ((rc = norms(act))) return rc;
      wmask = act;
    }
    int m = k;
    for (int i = 0; i < k; ++i)
      if ((act >> i) & 1u) {
        if ((rc = product(k + i))) return rc; // step 6
        cols.idx[m++] = k + i;
      }
    if (have_p)
      for (int i = 0; i < k; ++i)
        if ((act >> i) & 1u) cols.idx[m++] = 2 * k + i;
    cols.m = m;
    int rank = 0;
    if ((rc = rayleigh_ritz(&rank))) return rc;
    if (rank < k) return cfs_rt::set_err(CFS_HIP_ERR_INTERNAL, "lobpcg: the basis lost rank");
    have_p = true;
    fresh = false;
    wmask = act;
    if ((rc = norms(wmask))) return rc;
    ++it;
  }
  if (!debug && !fresh) { // the residuals of what is returned, from the stored vectors: k more products
    for (int c = 0; c < k; ++c)
      if ((rc = product(c))) return rc;
    if ((rc = norms(0u))) return rc;
  }
  int nconv = 0;
  while (nconv < k && res[nconv] <= thr) ++nconv;
  V *X = (V *)vectors_dev;
  for (int c = 0; c < k; ++c)
    HIPCHK(hipMemcpyAsync(X + (long long)c * ldx, col(S, c), (size_t)n * sizeof(V), hipMemcpyDeviceToDevice, st));
  HIPCHK(hipStreamSynchronize(st));
  for (int i = 0; i < k; ++i) {
    eigenvalues[i] = theta[i];
    if (residuals) residuals[i] = res[i];
  }
  if (nconv_out) *nconv_out = nconv;
  if (iterations_out) *iterations_out = it;
  if (products_out) *products_out = products;
  if (GEN && b_products_out) *b_products_out = b_products;
  return 0;
}

#undef CFS_LOBPCG_ROUNDING

} // namespace cfs_solver
