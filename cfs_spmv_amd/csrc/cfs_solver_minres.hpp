// cfs_solver_minres.hpp -- MINRES (Paige & Saunders) for (A - shift I) u = b on resident vectors, A symmetric and
// possibly indefinite (cfs_hip_sym_minres): the solver for what conjugate gradients cannot promise anything on --
// saddle-point matrices, shifted operators, mixed-sign diagonals.  One Lanczos recurrence, no breakdown on a
// nonsingular matrix, a residual norm that never increases.
//
// The layout is that of cfs_solver.hpp: one product and three fused vector kernels per iteration, five launches,
// every scalar in device memory, no host round trip between two looks.  With V the value type, every dot product
// and scalar in fp64, M = I or M = |diag(A) - shift| (dinv_i = (V)(1 / |a_ii - shift|), z = dinv r formed in fp64
// where it is needed and never stored):
//   set-up   q = A u;  r2 = (V)(b - (q - shift u));  beta1 = sqrt(r2 . z);  v = (V)(z / beta1);  r1 = r2;  w = w2 = 0
//   tile kernel + fold            q = A v
//   minres_lanczos_kernel         t = (V)(q - shift v - (beta / oldb) r1)  [k >= 1];  alfa = v . t;  t overwrites r1
//   minres_residual2_kernel       y = (V)(t - (alfa / beta) r2), in place;  bn2 = y . (dinv y)
//                                 (y is the next r2, the old r2 the next r1: the two buffers swap with the parity of k)
//   minres_update_kernel          the plane rotation, by every workgroup for itself;  wn = (V)((v - oldeps w2 - delta w)
//                                 / gamma) over w2;  u += phi wn;  v = (V)(dinv y / betan)
// alfa and bn2 are kGrid partial sums that every consumer adds up in a fixed order (cfs_solver::slot_sum), so on a
// deterministic handle the whole solve is bit-reproducible.
//
// The recurrence's scalars -- oldb, beta, dbar, epsln, phibar, cs, sn -- the iteration count and the DONE FLAG are
// one small STATE in device memory, double-buffered by the parity of the iteration: the kernels of iteration k read
// state[k & 1]; thread 0 of workgroup 0 of minres_update_kernel writes state[(k + 1) & 1].  So no workgroup ever
// reads a word that a thread of the same launch writes.  That matters for the flag: minres_update_kernel both
// updates u and decides convergence, and a workgroup that started late and saw a flag raised by its OWN launch
// would skip its slice of the last update of u.  Kernels of an iteration whose state says done return at once; the
// update kernel's one thread then copies the state forward, unchanged, so every iteration enqueued behind a
// converged one does nothing, whatever the window of enqueued iterations.
//
// wn overwrites w2 element by element, so the w buffers swap with the parity of k as the r buffers do: two
// iterations make a period.
#pragma once

#include <cfloat>

namespace cfs_solver {

// No fused multiply-adds in the vector kernels: every product and every sum of an update is rounded to fp64 by
// itself, so the kernels round exactly as the recurrence in cfs_hip.h is written and a run differs from the same
// recurrence on the CPU (numpy, the host-driven loop in torch) only in the order of the additions inside the
// products and the dot products.  In fp64 a contracted update would differ from the written one by as much as
// the written one's own rounding.  The kernels are bound by memory; the extra instructions cost nothing.
#define CFS_MINRES_ROUNDING _Pragma("clang fp contract(off)")

// part[slot][kGrid] of this solver (a buffer of its own: the slots of cfs_solver.hpp are not touched)
enum MinresSlot { M_ALFA = 0, M_BN2, M_R0, M_BM, M_BB, M_RES, M_BAD, M_COUNT };
// state[parity][word]
enum MinresState { S_OLDB = 0, S_BETA, S_DBAR, S_EPSLN, S_PHIBAR, S_CS, S_SN, S_ITER, S_DONE, S_COUNT };

// dinv = (V)(1 / |d - shift|) in place over the gathered diagonal;  part[M_BAD] <- entries whose |d - shift| is zero or not finite
template <typename V>
__global__ void __launch_bounds__(kThreads)
    minres_dinv_kernel(V *__restrict__ d, long long n, double shift, double *__restrict__ part) {
  double bad = 0.0;
  for (long long i = (long long)blockIdx.x * kThreads + threadIdx.x; i < n; i += (long long)gridDim.x * kThreads) {
    const double a = fabs((double)d[i] - shift);
    // (!(a > 0): a NaN counts too)
    if (!(a > 0.0) || a * 0.0 != 0.0) bad += 1.0;
    d[i] = (V)(1.0 / a);
  }
  bad = block_sum(bad);
  if (threadIdx.x == 0) part[M_BAD * kGrid + blockIdx.x] = bad;
}

// d = b - (q - shift u) in fp64, q = A u.
// first: r1 = r2 = (V)d;  part[M_R0] <- r2 . z (z = dinv r2 of the ROUNDED r2),  part[M_BM] <- b . (dinv b),  part[M_BB] <- b . b
// else (the closing residual): nothing stored;  part[M_RES] <- d . d of the unrounded d
template <typename V, bool PRE>
__global__ void __launch_bounds__(kThreads)
    minres_residual_kernel(V *__restrict__ r1, V *__restrict__ r2, const V *__restrict__ b, const V *__restrict__ q,
                           const V *__restrict__ u, double shift, long long n, double *__restrict__ part, int first,
                           const V *__restrict__ dinv) {
  CFS_MINRES_ROUNDING
  constexpr int W = Vec16<V>::W;
  typedef typename Vec16<V>::type VT;
  const long long nv = n / W, t0 = (long long)blockIdx.x * kThreads + threadIdx.x, stride = (long long)gridDim.x * kThreads;
  double rz = 0.0, bm = 0.0, bb = 0.0, dd = 0.0;
  for (long long i = t0; i < nv; i += stride) {
    const VT bv = reinterpret_cast<const VT *>(b)[i], qv = reinterpret_cast<const VT *>(q)[i],
             uv = reinterpret_cast<const VT *>(u)[i];
    VT rv, dv;
    if (PRE) dv = reinterpret_cast<const VT *>(dinv)[i];
#pragma unroll
    for (int k = 0; k < W; ++k) {
      const double d = (double)bv[k] - ((double)qv[k] - shift * (double)uv[k]);
      rv[k] = (V)d;
      dd += d * d;
      const double m = PRE ? (double)dv[k] : 1.0;
      rz += (double)rv[k] * ((double)rv[k] * m);
      bm += (double)bv[k] * ((double)bv[k] * m);
      bb += (double)bv[k] * (double)bv[k];
    }
    if (first) {
      reinterpret_cast<VT *>(r1)[i] = rv;
      reinterpret_cast<VT *>(r2)[i] = rv;
    }
  }
  for (long long i = nv * W + t0; i < n; i += stride) {
    const double bi = (double)b[i], d = bi - ((double)q[i] - shift * (double)u[i]);
    const V ri = (V)d;
    dd += d * d;
    const double m = PRE ? (double)dinv[i] : 1.0;
    rz += (double)ri * ((double)ri * m);
    bm += bi * (bi * m);
    bb += bi * bi;
    if (first) {
      r1[i] = ri;
      r2[i] = ri;
    }
  }
  if (first) {
    rz = block_sum(rz);
    bm = block_sum(bm);
    bb = block_sum(bb);
    if (threadIdx.x == 0) {
      part[M_R0 * kGrid + blockIdx.x] = rz;
      part[M_BM * kGrid + blockIdx.x] = bm;
      part[M_BB * kGrid + blockIdx.x] = bb;
    }
  } else {
    dd = block_sum(dd);
    if (threadIdx.x == 0) part[M_RES * kGrid + blockIdx.x] = dd;
  }
}

// beta1 = sqrt(r2 . z);  v = (V)(z / beta1) with z = dinv r2;  one thread: state[0], the state of iteration 0
template <typename V, bool PRE>
__global__ void __launch_bounds__(kThreads)
    minres_start_kernel(V *__restrict__ v, const V *__restrict__ r2, long long n, const double *__restrict__ part,
                        double *__restrict__ state, const V *__restrict__ dinv) {
  CFS_MINRES_ROUNDING
  const double beta1 = sqrt(slot_sum(part, M_R0));
  constexpr int W = Vec16<V>::W;
  typedef typename Vec16<V>::type VT;
  const long long nv = n / W, t0 = (long long)blockIdx.x * kThreads + threadIdx.x, stride = (long long)gridDim.x * kThreads;
  for (long long i = t0; i < nv; i += stride) {
    const VT rv = reinterpret_cast<const VT *>(r2)[i];
    VT vv, dv;
    if (PRE) dv = reinterpret_cast<const VT *>(dinv)[i];
#pragma unroll
    for (int k = 0; k < W; ++k) vv[k] = (V)((PRE ? (double)rv[k] * (double)dv[k] : (double)rv[k]) / beta1);
    reinterpret_cast<VT *>(v)[i] = vv;
  }
  for (long long i = nv * W + t0; i < n; i += stride)
    v[i] = (V)((PRE ? (double)r2[i] * (double)dinv[i] : (double)r2[i]) / beta1);
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    double *s = state;
    s[S_OLDB] = 0.0;
    s[S_BETA] = beta1;
    s[S_DBAR] = 0.0;
    s[S_EPSLN] = 0.0;
    s[S_PHIBAR] = beta1;
    s[S_CS] = -1.0;
    s[S_SN] = 0.0;
    s[S_ITER] = 0.0;
    s[S_DONE] = 0.0;
  }
}

// K1:  t = (V)(q - shift v - (beta / oldb) r1)  (the last term from iteration 1 on), over r1;  part[M_ALFA] <- v . t, t as stored
template <typename V>
__global__ void __launch_bounds__(kThreads)
    minres_lanczos_kernel(V *__restrict__ r1, const V *__restrict__ q, const V *__restrict__ v, double shift, long long n,
                          double *__restrict__ part, const double *__restrict__ state, int it) {
  CFS_MINRES_ROUNDING
  const double *s = state + (it & 1) * S_COUNT;
  if (s[S_DONE] != 0.0) return;
  const double c = it >= 1 ? s[S_BETA] / s[S_OLDB] : 0.0;
  constexpr int W = Vec16<V>::W;
  typedef typename Vec16<V>::type VT;
  const long long nv = n / W, t0 = (long long)blockIdx.x * kThreads + threadIdx.x, stride = (long long)gridDim.x * kThreads;
  double a = 0.0;
  for (long long i = t0; i < nv; i += stride) {
    const VT qv = reinterpret_cast<const VT *>(q)[i], vv = reinterpret_cast<const VT *>(v)[i];
    VT rv = reinterpret_cast<VT *>(r1)[i];
#pragma unroll
    for (int k = 0; k < W; ++k) {
      double t = (double)qv[k] - shift * (double)vv[k];
      if (it >= 1) t -= c * (double)rv[k];
      rv[k] = (V)t;
      a += (double)vv[k] * (double)rv[k];
    }
    reinterpret_cast<VT *>(r1)[i] = rv;
  }
  for (long long i = nv * W + t0; i < n; i += stride) {
    double t = (double)q[i] - shift * (double)v[i];
    if (it >= 1) t -= c * (double)r1[i];
    const V ts = (V)t;
    r1[i] = ts;
    a += (double)v[i] * (double)ts;
  }
  a = block_sum(a);
  if (threadIdx.x == 0) part[M_ALFA * kGrid + blockIdx.x] = a;
}

// K2:  y = (V)(t - (alfa / beta) r2), over t;  part[M_BN2] <- y . (dinv y), y as stored
template <typename V, bool PRE>
__global__ void __launch_bounds__(kThreads)
    minres_residual2_kernel(V *__restrict__ t, const V *__restrict__ r2, long long n, double *__restrict__ part,
                            const double *__restrict__ state, int it, const V *__restrict__ dinv) {
  CFS_MINRES_ROUNDING
  const double *s = state + (it & 1) * S_COUNT;
  if (s[S_DONE] != 0.0) return;
  const double c = slot_sum(part, M_ALFA) / s[S_BETA];
  constexpr int W = Vec16<V>::W;
  typedef typename Vec16<V>::type VT;
  const long long nv = n / W, t0 = (long long)blockIdx.x * kThreads + threadIdx.x, stride = (long long)gridDim.x * kThreads;
  double bn = 0.0;
  for (long long i = t0; i < nv; i += stride) {
    VT tv = reinterpret_cast<VT *>(t)[i];
    const VT rv = reinterpret_cast<const VT *>(r2)[i];
    VT dv;
    if (PRE) dv = reinterpret_cast<const VT *>(dinv)[i];
#pragma unroll
    for (int k = 0; k < W; ++k) {
      tv[k] = (V)((double)tv[k] - c * (double)rv[k]);
      bn += (double)tv[k] * (PRE ? (double)tv[k] * (double)dv[k] : (double)tv[k]);
    }
    reinterpret_cast<VT *>(t)[i] = tv;
  }
  for (long long i = nv * W + t0; i < n; i += stride) {
    const V y = (V)((double)t[i] - c * (double)r2[i]);
    t[i] = y;
    bn += (double)y * (PRE ? (double)y * (double)dinv[i] : (double)y);
  }
  bn = block_sum(bn);
  if (threadIdx.x == 0) part[M_BN2 * kGrid + blockIdx.x] = bn;
}

// K3:  the plane rotation from state[it & 1], alfa and bn2, by every workgroup for itself;
//      wn = (V)((v - oldeps w2 - delta w) / gamma), over w2;  u = (V)(u + phi wn), wn as stored;
//      v = (V)(dinv y / betan)  (0 when betan = 0: the Krylov space is exhausted, u is exact)
// one thread: state[(it + 1) & 1] -- the iteration counted, the flag raised when !(phibar > stop) or !(betan > 0)
// (a NaN raises it too); for an iteration that found the flag up, the state copied forward unchanged
template <typename V, bool PRE>
__global__ void __launch_bounds__(kThreads)
    minres_update_kernel(V *__restrict__ u, V *__restrict__ v, V *__restrict__ w2, const V *__restrict__ w,
                         const V *__restrict__ y, long long n, const double *__restrict__ part, double *__restrict__ state,
                         int it, double stop, const V *__restrict__ dinv) {
  CFS_MINRES_ROUNDING
  const double *s = state + (it & 1) * S_COUNT;
  double *sn_ = state + ((it + 1) & 1) * S_COUNT;
  if (s[S_DONE] != 0.0) {
    if (blockIdx.x == 0 && threadIdx.x == 0)
      for (int k = 0; k < S_COUNT; ++k) sn_[k] = s[k];
    return;
  }
  const double alfa = slot_sum(part, M_ALFA), bn2 = slot_sum(part, M_BN2);
  const double betan = sqrt(bn2), oldeps = s[S_EPSLN], dbar0 = s[S_DBAR], cs0 = s[S_CS], sn0 = s[S_SN];
  const double delta = cs0 * dbar0 + sn0 * alfa, gbar = sn0 * dbar0 - cs0 * alfa;
  const double epsln = sn0 * betan, dbar = -cs0 * betan;
  const double gamma = fmax(sqrt(gbar * gbar + betan * betan), DBL_EPSILON);
  const double cs = gbar / gamma, sn = betan / gamma;
  const double phi = cs * s[S_PHIBAR], phibar = sn * s[S_PHIBAR];
  const bool live = betan > 0.0;
  constexpr int W = Vec16<V>::W;
  typedef typename Vec16<V>::type VT;
  const long long nv = n / W, t0 = (long long)blockIdx.x * kThreads + threadIdx.x, stride = (long long)gridDim.x * kThreads;
  for (long long i = t0; i < nv; i += stride) {
    VT uv = reinterpret_cast<VT *>(u)[i], vv = reinterpret_cast<VT *>(v)[i], w2v = reinterpret_cast<VT *>(w2)[i];
    const VT wv = reinterpret_cast<const VT *>(w)[i], yv = reinterpret_cast<const VT *>(y)[i];
    VT dv;
    if (PRE) dv = reinterpret_cast<const VT *>(dinv)[i];
#pragma unroll
    for (int k = 0; k < W; ++k) {
      w2v[k] = (V)(((double)vv[k] - oldeps * (double)w2v[k] - delta * (double)wv[k]) / gamma);
      uv[k] = (V)((double)uv[k] + phi * (double)w2v[k]);
      vv[k] = live ? (V)((PRE ? (double)yv[k] * (double)dv[k] : (double)yv[k]) / betan) : (V)0;
    }
    reinterpret_cast<VT *>(w2)[i] = w2v;
    reinterpret_cast<VT *>(u)[i] = uv;
    reinterpret_cast<VT *>(v)[i] = vv;
  }
  for (long long i = nv * W + t0; i < n; i += stride) {
    const V wn = (V)(((double)v[i] - oldeps * (double)w2[i] - delta * (double)w[i]) / gamma);
    w2[i] = wn;
    u[i] = (V)((double)u[i] + phi * (double)wn);
    v[i] = live ? (V)((PRE ? (double)y[i] * (double)dinv[i] : (double)y[i]) / betan) : (V)0;
  }
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    sn_[S_OLDB] = s[S_BETA];
    sn_[S_BETA] = betan;
    sn_[S_DBAR] = dbar;
    sn_[S_EPSLN] = epsln;
    sn_[S_PHIBAR] = phibar;
    sn_[S_CS] = cs;
    sn_[S_SN] = sn;
    sn_[S_ITER] = s[S_ITER] + 1.0;
    // (!(x > y): a NaN also ends the iteration)
    sn_[S_DONE] = (!(phibar > stop) || !live) ? 1.0 : 0.0;
  }
}

// u: in = first guess, out = solution of (A - shift I) u = b.  Returns 0 / an error code; *iterations, *relres as
// documented in cfs_hip.h.  PRE: M = |diag(A) - shift|
template <typename V, bool PRE, class Handle>
int minres(Handle *h, void *u_dev, const void *b_dev, double shift, double tol, int maxiter, int check_every, int *iterations,
           double *relres, hipStream_t st) {
  using cfs_rt::DevBuf;
  const long long n = h->n();
  if (h->rows() != h->n())
    return cfs_rt::set_err(CFS_HIP_ERR_UNSUPPORTED, "minres: the handle holds a row block, not the whole matrix");
  check_every = look_window(check_every);
  V *u = (V *)u_dev;
  const V *b = (const V *)b_dev;
  DevBuf vbuf, qbuf, rbuf[2], wbuf[2], sbuf, dbuf;
  Slots slots;
  int rc;
  if (PRE && (rc = alloc_vectors<V>(n, {&dbuf}))) return rc;
  const V *dinv = (const V *)dbuf.p;
  if ((rc = alloc_vectors<V>(n, {&vbuf, &qbuf, &rbuf[0], &rbuf[1], &wbuf[0], &wbuf[1]})) || (rc = slots.alloc(M_COUNT, st)) ||
      (rc = sbuf.alloc(2 * S_COUNT * sizeof(double))) || (rc = slots.zero()))
    return rc;
  V *v = (V *)vbuf.p, *q = (V *)qbuf.p;
  V *r[2] = {(V *)rbuf[0].p, (V *)rbuf[1].p}, *w[2] = {(V *)wbuf[0].p, (V *)wbuf[1].p};
  double *part = slots.dev(), *state = (double *)sbuf.p;
  HIPCHK(hipMemsetAsync(state, 0, 2 * S_COUNT * sizeof(double), st));
  if (PRE) { // dinv from the handle's own diagonal; entries whose |a_ii - shift| is zero or not finite are counted
    if ((rc = h->diagonal(dbuf.p, st))) return rc;
    hipLaunchKernelGGL((minres_dinv_kernel<V>), dim3(kGrid), dim3(kThreads), 0, st, (V *)dbuf.p, n, shift, part);
  }
  // r1 = r2 = b - (A - shift I) u and the three sums of the set-up (r1: r[0], r2: r[1])
  if ((rc = h->spmv_local(q, u, nullptr, st))) return rc;
  hipLaunchKernelGGL((minres_residual_kernel<V, PRE>), dim3(kGrid), dim3(kThreads), 0, st, r[0], r[1], b, (const V *)q,
                     (const V *)u, shift, n, part, 1, dinv);
  HIPCHK(hipGetLastError());
  if ((rc = slots.fetch())) return rc;
  if (PRE) { // (read with the first host look: u has not been touched yet)
    const double bad = slots.sum(M_BAD);
    if (bad != 0.0)
      return cfs_rt::set_err(CFS_HIP_ERR_ARG, "minres: Jacobi needs a nonzero diagonal of A - shift I, " +
                                                  std::to_string((long long)bad) + " of " + std::to_string(n) +
                                                  " entries are zero (or not stored) or not finite");
  }
  const double bb = slots.sum(M_BB), beta1 = std::sqrt(slots.sum(M_R0)), stop = tol * std::sqrt(slots.sum(M_BM));
  // the first guess already solves it (or b = 0, or a NaN)
  bool done = !(beta1 > stop) || !(beta1 > 0.0);
  int it = 0, counted = 0;
  if (!done && maxiter > 0) {
    HIPCHK(hipMemsetAsync(w[0], 0, (size_t)n * sizeof(V), st));
    HIPCHK(hipMemsetAsync(w[1], 0, (size_t)n * sizeof(V), st));
    hipLaunchKernelGGL((minres_start_kernel<V, PRE>), dim3(kGrid), dim3(kThreads), 0, st, v, (const V *)r[1], n,
                       (const double *)part, state, dinv);
  }
  // iteration k: r1 = r[k & 1], r2 = r[(k + 1) & 1];  w2 = w[k & 1], w = w[(k + 1) & 1]
  auto iteration = [&](int k) -> int {
    int r2 = h->spmv_local(q, v, nullptr, st);
    if (r2) return r2;
    V *r1k = r[k & 1], *r2k = r[(k + 1) & 1];
    hipLaunchKernelGGL((minres_lanczos_kernel<V>), dim3(kGrid), dim3(kThreads), 0, st, r1k, (const V *)q, (const V *)v, shift, n,
                       part, (const double *)state, k);
    hipLaunchKernelGGL((minres_residual2_kernel<V, PRE>), dim3(kGrid), dim3(kThreads), 0, st, r1k, (const V *)r2k, n, part,
                       (const double *)state, k, dinv);
    hipLaunchKernelGGL((minres_update_kernel<V, PRE>), dim3(kGrid), dim3(kThreads), 0, st, u, v, w[k & 1],
                       (const V *)w[(k + 1) & 1], (const V *)r1k, n, (const double *)part, state, k, stop, dinv);
    return 0;
  };
  double hs[S_COUNT];
  while (!done && it < maxiter) {
    const int until = std::min(maxiter, it + check_every);
    for (; it < until; ++it)
      if ((rc = iteration(it))) return rc;
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(hs, state + (it & 1) * S_COUNT, sizeof hs, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    counted = (int)hs[S_ITER];
    done = hs[S_DONE] != 0.0;
  }
  // the true residual of what is returned, shift included
  if ((rc = h->spmv_local(q, u, nullptr, st))) return rc;
  hipLaunchKernelGGL((minres_residual_kernel<V, false>), dim3(kGrid), dim3(kThreads), 0, st, (V *)nullptr, (V *)nullptr, b,
                     (const V *)q, (const V *)u, shift, n, part, 0, (const V *)nullptr);
  HIPCHK(hipGetLastError());
  if ((rc = slots.fetch())) return rc;
  const double res2 = slots.sum(M_RES);
  if (iterations) *iterations = counted;
  if (relres) *relres = bb > 0.0 ? std::sqrt(res2 / bb) : std::sqrt(res2);
  return 0;
}

#undef CFS_MINRES_ROUNDING

} // namespace cfs_solver
