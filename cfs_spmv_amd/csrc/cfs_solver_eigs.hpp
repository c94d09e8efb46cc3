// cfs_solver_eigs.hpp -- thick-restart Lanczos (Wu & Simon) for k extreme eigenpairs of A (cfs_hip_sym_eigs), with
// full re-orthogonalisation against a basis of ncv + 1 vectors resident on the device.  The products are the tile
// kernel + fold of the handle; everything else here is tall-skinny dense algebra against the basis V (n x j, column
// i at basis + i ld, stored in the value type V): V^T q, q - V c, V S.  Pure bandwidth work.
//
// Step j (1-based; v_j is column j - 1), every dot product and scalar in fp64, no contracted multiply-adds:
//   tile kernel + fold          q = A v_j                                         (2 launches, stored in V)
//   eigs_project_kernel         part[k] <- v_k . q  (k = 1 .. j),  part[QQ] <- q . q      reads (j + j/8 + 1) n
//   eigs_reduce_kernel          c = the j + 1 sums, once, as doubles                      reads (j + 1) 512 doubles
//   eigs_subtract_kernel        q1 = (V)(q - sum_k c_k v_k), k ascending -> column j       reads (j + 1) n, writes n
//   eigs_project_kernel         part[k] <- v_k . q1                                       reads (j + j/8) n
//   eigs_reduce_kernel          c' = the j sums
//   eigs_subtract_kernel        q2 = (V)(q1 - sum_k c'_k v_k) in place;  part[QQ] <- q2 . q2   reads (j + 1) n, writes n
//   eigs_scale_kernel           alpha_j = c_j + c'_j;  beta_j = sqrt(q2 . q2);  breakdown iff !(beta_j > 16 u_V sqrt(q . q));
//                               v_{j+1} = (V)(q2 / beta_j) in place, or 0                   reads n, writes n
// NINE launches per step and (4 + 1/4) j n + 8 n words moved (a word = one value of V), the product aside.  The
// second projection does not share a pass with the first subtraction: a row of q1 is final only after all j
// columns of that row have been walked, so a fused kernel reads its rows of V twice as well -- it would save one
// launch, no traffic -- and the two kernels stay the two plain ones.
//
// A step produces up to ncv dot products at once.  The projection kernel leaves them as kGrid partial sums each
// (one thread cannot hold ncv fp64 accumulators: it walks the columns in chunks of kEigsChunk = 8 accumulators and
// re-reads its slice of q once per chunk -- the j/8 above; a slice of q is n / kGrid values, too many for LDS at the
// sizes this library serves, and comes from the L2 / Infinity Cache on the second to last walk); eigs_reduce_kernel,
// one workgroup per coefficient, adds them up ONCE in the fixed order of slot_sum and stores c[] as doubles, so the
// consumer reads j doubles, not j x kGrid partial sums per workgroup (128 MB of L2 reads per kernel at ncv = 64).
//
// No host round trip inside a step or between steps: alpha[], beta[] and the breakdown flags live in device
// memory and the host looks only when the basis is full.  flag[j] is read by the kernels of step j (0-based) and
// flag[j + 1] is written by one thread of that step's eigs_scale_kernel (the flag of step j copied forward, or
// raised by a breakdown): no workgroup reads a word that its own launch writes, and every kernel enqueued behind a
// breakdown returns at once.  All sums are fixed-order partial sums (no atomics), so on a deterministic handle
// the whole solve is bit-reproducible.
//
// Restart (host + eigs_combine_kernel): with the basis full (m = ncv) the host copies alpha and beta, builds the
// projected matrix T (tridiagonal at first; after a restart the kept Ritz values on the diagonal, the arrow
// beta_m s_{m,i} in row / column l, a tridiagonal tail), solves it with symeig() below (cyclic Jacobi, fp64, no
// LAPACK), and -- unless the k wanted pairs have |beta_m s_{m,i}| <= tol max|theta| -- keeps l = k + (ncv - k) / 2
// Ritz vectors: V[:, 0..l) <- V_m S_keep by eigs_combine_kernel, IN PLACE and row-safe (a workgroup stages all m
// columns of its 256 / sizeof(V) rows in LDS before it writes any of them; fp64 accumulation in chunks of 8
// columns, rounded when stored), v_{m+1} moves to column l and the iteration continues at step l + 1.  The
// returned X = V_m S is the same kernel writing into the caller's array.  Memory held: (ncv + 1 + 1) n values.
#pragma once

#include <algorithm>
#include <cfloat>
#include <cmath>
#include <vector>

namespace cfs_solver {

#define CFS_EIGS_ROUNDING _Pragma("clang fp contract(off)")

constexpr int kEigsMax = CFS_HIP_EIGS_MAX_NCV;
constexpr int kEigsChunk = 8;           // fp64 accumulators a thread carries through one walk
constexpr int kEigsQQ = kEigsMax;       // the slot (and the word of c[]) of q . q / q2 . q2
constexpr int kEigsSlots = 2 * kEigsMax + 2; // part[slot][kGrid]: kEigsMax coefficients + QQ; the closing residuals use 2 i, 2 i + 1
// the device scalars, one array of doubles
enum EigsWords { EW_ALPHA = 0, EW_BETA = kEigsMax, EW_FLAG = 2 * kEigsMax, EW_C1 = 3 * kEigsMax + 8,
                 EW_C2 = 4 * kEigsMax + 16, EW_COUNT = 5 * kEigsMax + 24 };

// The start vector of a NULL v0_dev (documented in cfs_hip.h): a pure function of the row index
__host__ __device__ inline double eigs_default_v0(long long i) {
  unsigned long long z = ((unsigned long long)i + 1ull) * 0x9E3779B97F4A7C15ull;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  z ^= z >> 31;
  return (double)(z >> 11) * (1.0 / 9007199254740992.0) - 0.5;
}

// N sums over the workgroup at once (fixed order): thread e < N of the workgroup returns the e-th total in `out`
template <int N> __device__ __forceinline__ void block_sum_n(double (&v)[N], double &out) {
  __shared__ double wpart[kThreads / 64][N];
#pragma unroll
  for (int e = 0; e < N; ++e)
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v[e] += __shfl_down(v[e], o);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  __syncthreads(); // (a second call may not overwrite wpart before everybody has read it)
  if (lane == 0)
#pragma unroll
    for (int e = 0; e < N; ++e) wpart[wave][e] = v[e];
  __syncthreads();
  out = 0.0;
  if (threadIdx.x < N) {
    double s = 0.0;
#pragma unroll
    for (int w = 0; w < kThreads / 64; ++w) s += wpart[w][threadIdx.x];
    out = s;
  }
}

// v1 <- v0 (the caller's, or the default one), as values of V;  part[0] <- v0 . v0 of the stored values
template <typename V>
__global__ void __launch_bounds__(kThreads)
    eigs_start_kernel(V *__restrict__ v1, const V *__restrict__ v0, long long n, double *__restrict__ part) {
  double s = 0.0;
  for (long long i = (long long)blockIdx.x * kThreads + threadIdx.x; i < n; i += (long long)gridDim.x * kThreads) {
    const V a = v0 ? v0[i] : (V)eigs_default_v0(i);
    v1[i] = a;
    s += (double)a * (double)a;
  }
  s = block_sum(s);
  if (threadIdx.x == 0) part[blockIdx.x] = s;
}

// x = (V)(x / nrm) in place
template <typename V> __global__ void __launch_bounds__(kThreads) eigs_normalise_kernel(V *__restrict__ x, long long n, double nrm) {
  CFS_EIGS_ROUNDING
  for (long long i = (long long)blockIdx.x * kThreads + threadIdx.x; i < n; i += (long long)gridDim.x * kThreads)
    x[i] = (V)((double)x[i] / nrm);
}

// part[k] <- column k of the basis . q for k < nc (as stored, fp64 sums);  with_qq: part[QQ] <- q . q
template <typename V>
__global__ void __launch_bounds__(kThreads)
    eigs_project_kernel(const V *__restrict__ basis, long long ld, int nc, const V *__restrict__ q, long long n,
                        double *__restrict__ part, const double *__restrict__ flag, int with_qq) {
  CFS_EIGS_ROUNDING
  if (*flag != 0.0) return;
  constexpr int W = Vec16<V>::W;
  typedef typename Vec16<V>::type VT;
  const long long nv = n / W, t0 = (long long)blockIdx.x * kThreads + threadIdx.x, stride = (long long)gridDim.x * kThreads;
  for (int c0 = 0; c0 < nc; c0 += kEigsChunk) {
    const int cn = min(kEigsChunk, nc - c0);
    const bool qq_here = with_qq && c0 == 0;
    double acc[kEigsChunk + 1];
#pragma unroll
    for (int e = 0; e <= kEigsChunk; ++e) acc[e] = 0.0;
    const V *col = basis + (long long)c0 * ld;
    for (long long i = t0; i < nv; i += stride) {
      const VT qv = reinterpret_cast<const VT *>(q)[i];
#pragma unroll
      for (int e = 0; e < kEigsChunk; ++e)
        if (e < cn) {
          const VT vv = reinterpret_cast<const VT *>(col + (long long)e * ld)[i];
#pragma unroll
          for (int k = 0; k < W; ++k) acc[e] += (double)vv[k] * (double)qv[k];
        }
      if (qq_here)
#pragma unroll
        for (int k = 0; k < W; ++k) acc[kEigsChunk] += (double)qv[k] * (double)qv[k];
    }
    for (long long i = nv * W + t0; i < n; i += stride) {
      const double qi = (double)q[i];
#pragma unroll
      for (int e = 0; e < kEigsChunk; ++e)
        if (e < cn) acc[e] += (double)col[(long long)e * ld + i] * qi;
      if (qq_here) acc[kEigsChunk] += qi * qi;
    }
    double total;
    block_sum_n<kEigsChunk + 1>(acc, total);
    if ((int)threadIdx.x < cn) part[(long long)(c0 + threadIdx.x) * kGrid + blockIdx.x] = total;
    if (qq_here && threadIdx.x == kEigsChunk) part[(long long)kEigsQQ * kGrid + blockIdx.x] = total;
  }
}

// c[k] <- the sum of part[k] for k < nc, one workgroup each, in the order of slot_sum;  with_qq: workgroup nc does c[QQ]
__global__ void __launch_bounds__(kThreads)
    eigs_reduce_kernel(const double *__restrict__ part, double *__restrict__ c, int nc, const double *__restrict__ flag) {
  if (*flag != 0.0) return;
  const int slot = (int)blockIdx.x < nc ? (int)blockIdx.x : kEigsQQ;
  const double s = slot_sum(part, slot);
  if (threadIdx.x == 0) c[slot] = s;
}

// out = (V)(in - sum_{k < nc} c_k column k), fp64, k ascending, rounded once when stored (out may be in);
// with_norm: part[QQ] <- out . out of the stored values
template <typename V>
__global__ void __launch_bounds__(kThreads)
    eigs_subtract_kernel(V *out, const V *in, const V *__restrict__ basis, long long ld, int nc, long long n,
                         const double *__restrict__ c, double *__restrict__ part, const double *__restrict__ flag, int with_norm) {
  CFS_EIGS_ROUNDING
  if (*flag != 0.0) return;
  __shared__ double cs[kEigsMax];
  for (int k = threadIdx.x; k < nc; k += kThreads) cs[k] = c[k];
  __syncthreads();
  constexpr int W = Vec16<V>::W;
  typedef typename Vec16<V>::type VT;
  const long long nv = n / W, t0 = (long long)blockIdx.x * kThreads + threadIdx.x, stride = (long long)gridDim.x * kThreads;
  double nrm = 0.0;
  for (long long i = t0; i < nv; i += stride) {
    const VT iv = reinterpret_cast<const VT *>(in)[i];
    double t[W];
#pragma unroll
    for (int k = 0; k < W; ++k) t[k] = (double)iv[k];
#pragma unroll 4
    for (int j = 0; j < nc; ++j) {
      const VT vv = reinterpret_cast<const VT *>(basis + (long long)j * ld)[i];
      const double cj = cs[j];
#pragma unroll
      for (int k = 0; k < W; ++k) t[k] = t[k] - cj * (double)vv[k];
    }
    VT ov;
#pragma unroll
    for (int k = 0; k < W; ++k) {
      ov[k] = (V)t[k];
      nrm += (double)ov[k] * (double)ov[k];
    }
    reinterpret_cast<VT *>(out)[i] = ov;
  }
  for (long long i = nv * W + t0; i < n; i += stride) {
    double t = (double)in[i];
    for (int j = 0; j < nc; ++j) t = t - cs[j] * (double)basis[(long long)j * ld + i];
    const V o = (V)t;
    out[i] = o;
    nrm += (double)o * (double)o;
  }
  if (with_norm) {
    nrm = block_sum(nrm);
    if (threadIdx.x == 0) part[(long long)kEigsQQ * kGrid + blockIdx.x] = nrm;
  }
}

// beta = sqrt(part[QQ]) (q2 . q2), by every workgroup for itself;  x = (V)(x / beta) in place, or 0 on a breakdown:
// !(beta > 16 u_V sqrt(q . q)), q . q = c1[QQ] (a NaN counts).  One thread: alpha[j] = c1[j] + c2[j], beta[j],
// flag[j + 1]; behind a breakdown only flag[j + 1] = 1.
template <typename V>
__global__ void __launch_bounds__(kThreads)
    eigs_scale_kernel(V *__restrict__ x, long long n, const double *__restrict__ part, double *__restrict__ words, int j) {
  CFS_EIGS_ROUNDING
  if (words[EW_FLAG + j] != 0.0) {
    if (blockIdx.x == 0 && threadIdx.x == 0) words[EW_FLAG + j + 1] = 1.0;
    return;
  }
  const double beta = sqrt(slot_sum(part, kEigsQQ));
  const double unit = sizeof(V) == 8 ? 0x1p-53 : 0x1p-24;
  const bool live = beta > 16.0 * unit * sqrt(words[EW_C1 + kEigsQQ]);
  constexpr int W = Vec16<V>::W;
  typedef typename Vec16<V>::type VT;
  const long long nv = n / W, t0 = (long long)blockIdx.x * kThreads + threadIdx.x, stride = (long long)gridDim.x * kThreads;
  for (long long i = t0; i < nv; i += stride) {
    VT xv = reinterpret_cast<VT *>(x)[i];
#pragma unroll
    for (int k = 0; k < W; ++k) xv[k] = live ? (V)((double)xv[k] / beta) : (V)0;
    reinterpret_cast<VT *>(x)[i] = xv;
  }
  for (long long i = nv * W + t0; i < n; i += stride) x[i] = live ? (V)((double)x[i] / beta) : (V)0;
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    words[EW_ALPHA + j] = words[EW_C1 + j] + words[EW_C2 + j];
    words[EW_BETA + j] = beta;
    words[EW_FLAG + j + 1] = live ? 0.0 : 1.0;
  }
}

// out[:, c] = (V)(sum_{k < m} column k of the basis * s[k nout + c]) for c < nout, rows [0, n): fp64, k ascending,
// rounded when stored.  Row-safe IN PLACE (out == basis, ldo == ld): a workgroup stages all m columns of its R =
// 256 / sizeof(V) rows in LDS (m R values, at most 32 KiB) before it writes any of them, and no other workgroup
// touches those rows.  Thread (r, g) of R x (kThreads / R) owns row r and the columns g, g + G, ... in chunks of 8.
template <typename V>
__global__ void __launch_bounds__(kThreads)
    eigs_combine_kernel(V *out, long long ldo, const V *basis, long long ld, int m, const double *__restrict__ s, int nout,
                        long long n) {
  CFS_EIGS_ROUNDING
  extern __shared__ __align__(16) unsigned char eigs_lds[];
  V *tile = reinterpret_cast<V *>(eigs_lds); // tile[k R + r]
  constexpr int R = 256 / (int)sizeof(V), G = kThreads / R;
  const int r = threadIdx.x % R, g = threadIdx.x / R;
  const long long ntiles = (n + R - 1) / R;
  for (long long t = blockIdx.x; t < ntiles; t += gridDim.x) {
    const long long row0 = t * R;
    for (int e = threadIdx.x; e < m * R; e += kThreads) {
      const int k = e / R, rr = e % R;
      tile[e] = row0 + rr < n ? basis[(long long)k * ld + row0 + rr] : (V)0;
    }
    __syncthreads();
    if (row0 + r < n)
      for (int c0 = g; c0 < nout; c0 += G * kEigsChunk) {
        double acc[kEigsChunk];
#pragma unroll
        for (int e = 0; e < kEigsChunk; ++e) acc[e] = 0.0;
        for (int k = 0; k < m; ++k) {
          const double a = (double)tile[k * R + r];
          const double *sk = s + (long long)k * nout;
#pragma unroll
          for (int e = 0; e < kEigsChunk; ++e) {
            const int c = c0 + e * G;
            if (c < nout) acc[e] = acc[e] + a * sk[c];
          }
        }
#pragma unroll
        for (int e = 0; e < kEigsChunk; ++e) {
          const int c = c0 + e * G;
          if (c < nout) out[(long long)c * ldo + row0 + r] = (V)acc[e];
        }
      }
    __syncthreads(); // (the next tile is staged over this one)
  }
}

// part[2 i] <- sum (q - theta x)^2,  part[2 i + 1] <- x . x, in fp64 from the stored values
template <typename V>
__global__ void __launch_bounds__(kThreads)
    eigs_residual_kernel(const V *__restrict__ q, const V *__restrict__ x, double theta, long long n, double *__restrict__ part, int i) {
  CFS_EIGS_ROUNDING
  double rr = 0.0, xx = 0.0;
  for (long long k = (long long)blockIdx.x * kThreads + threadIdx.x; k < n; k += (long long)gridDim.x * kThreads) {
    const double xk = (double)x[k], d = (double)q[k] - theta * xk;
    rr += d * d;
    xx += xk * xk;
  }
  rr = block_sum(rr);
  xx = block_sum(xx);
  if (threadIdx.x == 0) {
    part[(long long)(2 * i) * kGrid + blockIdx.x] = rr;
    part[(long long)(2 * i + 1) * kGrid + blockIdx.x] = xx;
  }
}

// ---- the small dense symmetric eigensolver of the restart (host, fp64): cyclic Jacobi (Rutishauser's form) ----
// a: m x m symmetric row-major (the upper triangle is read);  w: eigenvalues ascending;  s: row-major, eigenvector i
// in column i.  Returns the sweeps made, -1 without convergence (50 sweeps).
inline int symeig(int m, const double *a_in, double *w, double *s) {
  std::vector<double> a(a_in, a_in + (size_t)m * m), b(m), z(m, 0.0), v((size_t)m * m, 0.0);
  auto A = [&](int i, int j) -> double & { return a[(size_t)i * m + j]; };
  auto Vv = [&](int i, int j) -> double & { return v[(size_t)i * m + j]; };
  std::vector<double> d(m);
  for (int i = 0; i < m; ++i) {
    Vv(i, i) = 1.0;
    d[i] = b[i] = A(i, i);
  }
  int sweep = 0;
  for (; sweep < 50; ++sweep) {
    double sm = 0.0;
    for (int p = 0; p < m - 1; ++p)
      for (int q = p + 1; q < m; ++q) sm += std::fabs(A(p, q));
    if (sm == 0.0) break;
    const double tresh = sweep < 3 ? 0.2 * sm / ((double)m * m) : 0.0;
    for (int p = 0; p < m - 1; ++p)
      for (int q = p + 1; q < m; ++q) {
        const double apq = A(p, q), g = 100.0 * std::fabs(apq);
        if (apq == 0.0) continue;
        if (sweep > 3 && std::fabs(d[p]) + g == std::fabs(d[p]) && std::fabs(d[q]) + g == std::fabs(d[q])) {
          A(p, q) = 0.0;
          continue;
        }
        if (!(std::fabs(apq) > tresh)) continue;
        const double h = d[q] - d[p];
        double t;
        if (std::fabs(h) + g == std::fabs(h)) {
          t = apq / h;
        } else {
          const double theta = 0.5 * h / apq;
          t = 1.0 / (std::fabs(theta) + std::sqrt(1.0 + theta * theta));
          if (theta < 0.0) t = -t;
        }
        const double c = 1.0 / std::sqrt(1.0 + t * t), sn = t * c, tau = sn / (1.0 + c), hh = t * apq;
        z[p] -= hh;
        z[q] += hh;
        d[p] -= hh;
        d[q] += hh;
        A(p, q) = 0.0;
        auto rot = [&](double &x, double &y) {
          const double gx = x, hy = y;
          x = gx - sn * (hy + gx * tau);
          y = hy + sn * (gx - hy * tau);
        };
        for (int j = 0; j < p; ++j) rot(A(j, p), A(j, q));
        for (int j = p + 1; j < q; ++j) rot(A(p, j), A(j, q));
        for (int j = q + 1; j < m; ++j) rot(A(p, j), A(q, j));
        for (int j = 0; j < m; ++j) rot(Vv(j, p), Vv(j, q));
      }
    for (int i = 0; i < m; ++i) {
      b[i] += z[i];
      d[i] = b[i];
      z[i] = 0.0;
    }
  }
  std::vector<int> idx(m);
  for (int i = 0; i < m; ++i) idx[i] = i;
  std::stable_sort(idx.begin(), idx.end(), [&](int x, int y) { return d[x] < d[y]; });
  for (int i = 0; i < m; ++i) {
    w[i] = d[idx[i]];
    for (int j = 0; j < m; ++j) s[(size_t)j * m + i] = Vv(j, idx[i]);
  }
  return sweep < 50 ? sweep : -1;
}

// ---- the recurrence on a handle: the basis (caller's or the solver's), one scratch vector, the scalars ----
template <typename V, class Handle> struct Lanczos {
  Handle *h;
  V *basis;
  long long ld, n;
  hipStream_t st;
  cfs_rt::DevBuf qbuf, pbuf, wbuf;
  V *q = nullptr;
  double *part = nullptr, *words = nullptr;
  std::vector<double> hp;

  int init() {
    int rc;
    if ((rc = qbuf.alloc((size_t)n * sizeof(V) + 64)) || (rc = pbuf.alloc((size_t)kEigsSlots * kGrid * sizeof(double))) ||
        (rc = wbuf.alloc(EW_COUNT * sizeof(double))))
      return rc;
    q = (V *)qbuf.p;
    part = (double *)pbuf.p;
    words = (double *)wbuf.p;
    HIPCHK(hipMemsetAsync(part, 0, (size_t)kEigsSlots * kGrid * sizeof(double), st));
    HIPCHK(hipMemsetAsync(words, 0, EW_COUNT * sizeof(double), st));
    return 0;
  }
  V *col(int j) const { return basis + (long long)j * ld; }
  // column 0 <- (V)(v0 / ||v0||); one host look.  *nrm = ||v0|| (the caller refuses 0 and non-finite norms BEFORE
  // anything of its own is written: only column 0 of the basis has been touched)
  int start(const V *v0, double *nrm) {
    hipLaunchKernelGGL((eigs_start_kernel<V>), dim3(kGrid), dim3(kThreads), 0, st, col(0), v0, n, part);
    HIPCHK(hipGetLastError());
    hp.resize(kGrid);
    HIPCHK(hipMemcpyAsync(hp.data(), part, kGrid * sizeof(double), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    double s = 0.0;
    for (int g = 0; g < kGrid; g++) s += hp[g];
    *nrm = std::sqrt(s);
    if (!(*nrm > 0.0) || !std::isfinite(*nrm)) return 0;
    hipLaunchKernelGGL((eigs_normalise_kernel<V>), dim3(kGrid), dim3(kThreads), 0, st, col(0), n, *nrm);
    HIPCHK(hipGetLastError());
    return 0;
  }
  // step j (0-based): reads columns 0 .. j, writes column j + 1, alpha[j], beta[j], flag[j + 1]
  int step(int j) {
    int rc = h->spmv_local(q, col(j), nullptr, st);
    if (rc) return rc;
    const int nc = j + 1;
    const double *flag = words + EW_FLAG + j;
    V *next = col(j + 1);
    const dim3 grid(kGrid), block(kThreads);
    hipLaunchKernelGGL((eigs_project_kernel<V>), grid, block, 0, st, (const V *)basis, ld, nc, (const V *)q, n, part, flag, 1);
    hipLaunchKernelGGL(eigs_reduce_kernel, dim3(nc + 1), block, 0, st, (const double *)part, words + EW_C1, nc, flag);
    hipLaunchKernelGGL((eigs_subtract_kernel<V>), grid, block, 0, st, next, (const V *)q, (const V *)basis, ld, nc, n,
                       (const double *)(words + EW_C1), part, flag, 0);
    hipLaunchKernelGGL((eigs_project_kernel<V>), grid, block, 0, st, (const V *)basis, ld, nc, (const V *)next, n, part, flag, 0);
    hipLaunchKernelGGL(eigs_reduce_kernel, dim3(nc), block, 0, st, (const double *)part, words + EW_C2, nc, flag);
    hipLaunchKernelGGL((eigs_subtract_kernel<V>), grid, block, 0, st, next, (const V *)next, (const V *)basis, ld, nc, n,
                       (const double *)(words + EW_C2), part, flag, 1);
    hipLaunchKernelGGL((eigs_scale_kernel<V>), grid, block, 0, st, next, n, (const double *)part, words, j);
    HIPCHK(hipGetLastError());
    return 0;
  }
  // the host's look: alpha[from .. to), beta[from .. to) and *made = steps made up to and with a breakdown (to - from
  // without one).  Synchronises the stream.
  int look(int from, int to, double *alpha, double *beta, int *made, bool *broke) {
    std::vector<double> w(EW_COUNT);
    HIPCHK(hipMemcpyAsync(w.data(), words, EW_COUNT * sizeof(double), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    *made = to - from;
    *broke = false;
    for (int j = from; j < to; ++j)
      if (w[EW_FLAG + j + 1] != 0.0) {
        *made = j + 1 - from;
        *broke = true;
        break;
      }
    for (int j = from; j < from + *made; ++j) {
      alpha[j] = w[EW_ALPHA + j];
      beta[j] = w[EW_BETA + j];
    }
    return 0;
  }
};

// out[:, 0 .. nout) = V_m S on rows [0, n) (s: m x nout row-major on the host, uploaded to s_dev, m nout doubles of room);
// out == basis with ldo == ld is the in-place restart.  THE launch of eigs_combine_kernel: the solver's restart, its
// returned X and cfs_hip_debug_eigs_combine all come through here.  Synchronises the stream.
template <typename V>
int eigs_combine(V *out, long long ldo, const V *basis, long long ld, long long n, int m, const double *s, int nout, double *s_dev,
                 hipStream_t st) {
  HIPCHK(hipMemcpyAsync(s_dev, s, (size_t)m * nout * sizeof(double), hipMemcpyHostToDevice, st));
  constexpr int R = 256 / (int)sizeof(V);
  const long long ntiles = (n + R - 1) / R;
  hipLaunchKernelGGL((eigs_combine_kernel<V>), dim3((unsigned)std::min<long long>(ntiles, 4 * kGrid)), dim3(kThreads),
                     (size_t)m * R * sizeof(V), st, out, ldo, basis, ld, m, (const double *)s_dev, nout, n);
  HIPCHK(hipGetLastError());
  HIPCHK(hipStreamSynchronize(st)); // (s is the host's to change again)
  return 0;
}

// cfs_hip_debug_eigs_combine (arguments checked by the caller)
template <typename V>
int debug_eigs_combine(void *out_dev, long long ldo, const void *basis_dev, long long ld, long long n, int m, int nout, const double *s,
                       hipStream_t st) {
  cfs_rt::DevBuf sdev;
  int rc;
  if ((rc = sdev.alloc((size_t)m * nout * sizeof(double)))) return rc;
  return eigs_combine<V>((V *)out_dev, ldo, (const V *)basis_dev, ld, n, m, s, nout, (double *)sdev.p, st);
}

// cfs_hip_sym_debug_lanczos
template <typename V, class Handle>
int debug_lanczos(Handle *h, const void *v0_dev, int steps, void *basis_dev, long long ld, double *alpha, double *beta, int *done,
                  hipStream_t st) {
  Lanczos<V, Handle> L{h, (V *)basis_dev, ld, h->n(), st};
  int rc;
  if ((rc = L.init())) return rc;
  double nrm = 0.0;
  if ((rc = L.start((const V *)v0_dev, &nrm))) return rc;
  if (!(nrm > 0.0) || !std::isfinite(nrm))
    return cfs_rt::set_err(CFS_HIP_ERR_ARG, "lanczos: the start vector has a norm that is zero or not finite");
  for (int j = 0; j < steps; ++j)
    if ((rc = L.step(j))) return rc;
  std::vector<double> a(kEigsMax, 0.0), b(kEigsMax, 0.0);
  int made = 0;
  bool broke = false;
  if ((rc = L.look(0, steps, a.data(), b.data(), &made, &broke))) return rc;
  for (int j = 0; j < steps; ++j) {
    alpha[j] = j < made ? a[j] : 0.0;
    beta[j] = j < made ? b[j] : 0.0;
  }
  *done = made;
  return 0;
}

// cfs_hip_sym_eigs (arguments checked by the caller; ncv resolved)
template <typename V, class Handle>
int eigs(Handle *h, int k, int which, int ncv, double tol, int max_restarts, const void *v0_dev, double *eigenvalues,
         void *vectors_dev, long long ldx, double *residuals, int *nconv_out, int *restarts_out, int *products_out, hipStream_t st) {
  using cfs_rt::DevBuf;
  const long long n = h->n();
  const long long ld = (n + Vec16<V>::W - 1) / Vec16<V>::W * Vec16<V>::W; // columns 16-byte aligned
  DevBuf vbuf, sdev;
  int rc;
  if ((rc = vbuf.alloc((size_t)(ncv + 1) * ld * sizeof(V) + 64)) || (rc = sdev.alloc((size_t)kEigsMax * kEigsMax * sizeof(double))))
    return rc;
  Lanczos<V, Handle> L{h, (V *)vbuf.p, ld, n, st};
  if ((rc = L.init())) return rc;
  double nrm = 0.0;
  if ((rc = L.start((const V *)v0_dev, &nrm))) return rc;
  if (!(nrm > 0.0) || !std::isfinite(nrm))
    return cfs_rt::set_err(CFS_HIP_ERR_ARG, "eigs: the start vector has a norm that is zero or not finite");
  const int lkeep = k + (ncv - k) / 2;
  std::vector<double> alpha(kEigsMax, 0.0), beta(kEigsMax, 0.0), arrow(kEigsMax, 0.0);
  std::vector<double> T, w, S, pack, est;
  std::vector<int> order;
  int l = 0, m = ncv, restarts = 0, products = 0, nconv = 0;
  bool broke = false;
  for (;;) {
    for (int j = l; j < ncv; ++j)
      if ((rc = L.step(j))) return rc;
    int made = 0;
    if ((rc = L.look(l, ncv, alpha.data(), beta.data(), &made, &broke))) return rc;
    products += made;
    m = l + made;
    // T: the kept Ritz values and their arrow in row / column l, then the tridiagonal tail
    T.assign((size_t)m * m, 0.0);
    for (int i = 0; i < m; ++i) T[(size_t)i * m + i] = alpha[i];
    for (int i = 0; i < l; ++i) T[(size_t)i * m + l] = T[(size_t)l * m + i] = arrow[i];
    for (int i = l; i + 1 < m; ++i) T[(size_t)i * m + i + 1] = T[(size_t)(i + 1) * m + i] = beta[i];
    w.resize(m);
    S.resize((size_t)m * m);
    if (symeig(m, T.data(), w.data(), S.data()) < 0) return cfs_rt::set_err(CFS_HIP_ERR_INTERNAL, "eigs: the projected eigenproblem did not converge");
    order.resize(m);
    for (int i = 0; i < m; ++i) order[i] = which == CFS_HIP_EIGS_SMALLEST ? i : m - 1 - i;
    if (which == CFS_HIP_EIGS_MAGNITUDE)
      std::stable_sort(order.begin(), order.end(), [&](int x, int y) { return std::fabs(w[x]) > std::fabs(w[y]); });
    const double bm = broke ? 0.0 : beta[m - 1];
    double tmax = 0.0;
    for (int i = 0; i < m; ++i) tmax = std::max(tmax, std::fabs(w[i]));
    est.assign(m, 0.0);
    for (int i = 0; i < m; ++i) est[i] = std::fabs(bm * S[(size_t)(m - 1) * m + order[i]]);
    const int kk = std::min(k, m);
    for (nconv = 0; nconv < kk && est[nconv] <= tol * tmax; ++nconv) {}
    if (broke) nconv = kk; // the Ritz pairs of T_m are exact in the Krylov space of v0
    if (broke || nconv == k || restarts >= max_restarts) break;
    // keep lkeep Ritz vectors, in place;  v_{m+1} -> column lkeep
    pack.resize((size_t)m * lkeep);
    for (int r = 0; r < m; ++r)
      for (int c = 0; c < lkeep; ++c) pack[(size_t)r * lkeep + c] = S[(size_t)r * m + order[c]];
    if ((rc = eigs_combine<V>(L.basis, ld, L.basis, ld, n, m, pack.data(), lkeep, (double *)sdev.p, st))) return rc;
    HIPCHK(hipMemcpyAsync(L.col(lkeep), L.col(m), (size_t)n * sizeof(V), hipMemcpyDeviceToDevice, st));
    for (int c = 0; c < lkeep; ++c) {
      alpha[c] = w[order[c]];
      arrow[c] = bm * S[(size_t)(m - 1) * m + order[c]];
    }
    l = lkeep;
    ++restarts;
  }
  const int kk = std::min(k, m);
  for (int i = 0; i < k; ++i) {
    eigenvalues[i] = i < kk ? w[order[i]] : 0.0;
    if (residuals) residuals[i] = i < kk ? est[i] : 0.0;
  }
  if (vectors_dev) {
    V *X = (V *)vectors_dev;
    pack.resize((size_t)m * kk);
    for (int r = 0; r < m; ++r)
      for (int c = 0; c < kk; ++c) pack[(size_t)r * kk + c] = S[(size_t)r * m + order[c]];
    if ((rc = eigs_combine<V>(X, ldx, L.basis, ld, n, m, pack.data(), kk, (double *)sdev.p, st))) return rc;
    for (int i = kk; i < k; ++i) HIPCHK(hipMemsetAsync(X + (long long)i * ldx, 0, (size_t)n * sizeof(V), st));
    // the residuals of what is returned, from the stored vectors: kk more products, one look
    for (int i = 0; i < kk; ++i) {
      if ((rc = h->spmv_local(L.q, X + (long long)i * ldx, nullptr, st))) return rc;
      hipLaunchKernelGGL((eigs_residual_kernel<V>), dim3(kGrid), dim3(kThreads), 0, st, (const V *)L.q, (const V *)(X + (long long)i * ldx),
                         eigenvalues[i], n, L.part, i);
    }
    HIPCHK(hipGetLastError());
    products += kk;
    std::vector<double> hp((size_t)2 * kk * kGrid);
    HIPCHK(hipMemcpyAsync(hp.data(), L.part, hp.size() * sizeof(double), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    for (int i = 0; i < kk && residuals; ++i) {
      double rr = 0.0, xx = 0.0;
      for (int g = 0; g < kGrid; g++) {
        rr += hp[(size_t)(2 * i) * kGrid + g];
        xx += hp[(size_t)(2 * i + 1) * kGrid + g];
      }
      residuals[i] = std::sqrt(rr) / std::sqrt(xx);
    }
  }
  if (nconv_out) *nconv_out = nconv;
  if (restarts_out) *restarts_out = restarts;
  if (products_out) *products_out = products;
  return 0;
}

#undef CFS_EIGS_ROUNDING

} // namespace cfs_solver
