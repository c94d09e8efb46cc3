// cfs_solver_mixed.hpp -- mixed-precision PCG: the fp32 products of one handle, the fp64 solution of another
// (cfs_hip_sym_pcg_mixed).
//
// The fp32 symmetric SpMV streams 8 bytes per stored nonzero where the fp64 one streams 12, and its vectors
// are half as wide; a solve in fp32 alone stalls near 1e-6 - 1e-7 relative residual.  Here ONE conjugate
// gradient recurrence runs in fp32 with the kernels of cfs_solver.hpp, launch for launch, on an fp32 handle
// of the matrix; what it accumulates is not the solution but a correction xlo to the fp64 solution u.  From
// time to time the TRUE residual b - A u, formed in fp64 with the fp64 handle, replaces the recurrence's
// fp32 residual ("CG with residual replacement", "reliable updates"):
//   cg_fold_kernel                u += (double)xlo;  xlo = 0
//   fp64 tile kernel + fold       q64 = A u
//   cg_replace_kernel             r = (float)(b - q64);  r . r (from the unrounded fp64 residual), r . z
// The search direction p is KEPT across a replacement: the Krylov space built so far is not thrown away, as
// it is by iterative refinement, which restarts CG with p = z at every correction equation.  A replacement
// costs one fp64 product and two vector passes; it happens when the recurrence's r . r has dropped by
// delta^2 against the largest r . r seen at a host look since the last one (or below the stopping rule),
// so about once per decade of the residual.  The device decides that at every iteration, see `thr` below;
// the host acts on the flag at its next look.  Between replacements an iteration is the five fp32 launches of
// cfs_solver::cg<float, BS>, one single-workgroup launch that raises the flag, and no host round trip.
//
// The scalars are the partial-sum slots of cfs_solver.hpp (no atomics, fixed order): on two deterministic
// handles the whole solve is bit-reproducible.  z = M^-1 r is formed in fp64 from the ROUNDED r and the fp32
// preconditioner, exactly as cg_update_kernel<float, BS, P_RZ0, OneColumn> forms it.
#pragma once

namespace cfs_solver {

// u += (double)xlo;  xlo = 0   (16-byte accesses: four floats, two pairs of doubles)
__global__ void __launch_bounds__(kThreads) cg_fold_kernel(double *__restrict__ u, float *__restrict__ xlo, long long n) {
  typedef Vec16<float>::type FT;
  typedef Vec16<double>::type DT;
  const long long nv = n / 4, t0 = (long long)blockIdx.x * kThreads + threadIdx.x, stride = (long long)gridDim.x * kThreads;
  for (long long i = t0; i < nv; i += stride) {
    const FT xv = reinterpret_cast<const FT *>(xlo)[i];
    DT a = reinterpret_cast<DT *>(u)[2 * i], c = reinterpret_cast<DT *>(u)[2 * i + 1];
    a[0] += (double)xv[0];
    a[1] += (double)xv[1];
    c[0] += (double)xv[2];
    c[1] += (double)xv[3];
    reinterpret_cast<DT *>(u)[2 * i] = a;
    reinterpret_cast<DT *>(u)[2 * i + 1] = c;
    reinterpret_cast<FT *>(xlo)[i] = FT{0.f, 0.f, 0.f, 0.f};
  }
  for (long long i = nv * 4 + t0; i < n; i += stride) {
    u[i] += (double)xlo[i];
    xlo[i] = 0.f;
  }
}

// d = b - q64 in fp64, never stored;  r = (float)d;  p = (float)z (when given);  part[slot_rr] <- d . d;
// part[P_BB] <- b . b (when with_bb);  BS >= 1: part[slot_rz] <- r . z with z = M^-1 r of the ROUNDED r (BS = 1: dinv;
// BS >= 2: the inverse node blocks, one node block per thread, as cg_residual_kernel<float, BS> walks).
// BS = 0: p = r (when given), no r . z (the plain iteration takes alpha from the r . r slot).
template <int BS>
__global__ void __launch_bounds__(kThreads)
    cg_replace_kernel(float *__restrict__ r, float *__restrict__ p, const double *__restrict__ b, const double *__restrict__ q64,
                      long long n, double *__restrict__ part, int slot_rr, int slot_rz, int with_bb,
                      const float *__restrict__ minv, long long nb) {
  constexpr bool PRE = BS == 1;
  double rr = 0.0, bb = 0.0, rz = 0.0;
  if constexpr (BS >= 2) {
    for (long long k = (long long)blockIdx.x * kThreads + threadIdx.x; k < nb; k += (long long)gridDim.x * kThreads) {
      double rd[BS], z[BS];
#pragma unroll
      for (int i = 0; i < BS; ++i) {
        const long long g = k * BS + i;
        rd[i] = 0.0;
        if (g < n) {
          const double bi = b[g], d = bi - q64[g];
          const float ri = (float)d;
          r[g] = ri;
          rd[i] = (double)ri;
          rr += d * d;
          bb += bi * bi;
        }
      }
      block_apply<float, BS>(minv, nb, k, rd, z);
#pragma unroll
      for (int i = 0; i < BS; ++i) {
        const long long g = k * BS + i;
        if (g < n) {
          rz += rd[i] * z[i];
          if (p) p[g] = (float)z[i];
        }
      }
    }
  } else {
    typedef Vec16<float>::type FT;
    typedef Vec16<double>::type DT;
    const long long nv = n / 4, t0 = (long long)blockIdx.x * kThreads + threadIdx.x, stride = (long long)gridDim.x * kThreads;
    for (long long i = t0; i < nv; i += stride) {
      const DT b0 = reinterpret_cast<const DT *>(b)[2 * i], b1 = reinterpret_cast<const DT *>(b)[2 * i + 1];
      const DT q0 = reinterpret_cast<const DT *>(q64)[2 * i], q1 = reinterpret_cast<const DT *>(q64)[2 * i + 1];
      const double bv[4] = {b0[0], b0[1], b1[0], b1[1]}, qv[4] = {q0[0], q0[1], q1[0], q1[1]};
      FT rv, zv;
      if (PRE) zv = reinterpret_cast<const FT *>(minv)[i];
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const double d = bv[k] - qv[k];
        rv[k] = (float)d;
        rr += d * d;
        bb += bv[k] * bv[k];
        if (PRE) {
          const double z = (double)rv[k] * (double)zv[k];
          rz += (double)rv[k] * z;
          zv[k] = (float)z;
        }
      }
      reinterpret_cast<FT *>(r)[i] = rv;
      if (p) reinterpret_cast<FT *>(p)[i] = PRE ? zv : rv;
    }
    for (long long i = nv * 4 + t0; i < n; i += stride) {
      const double bi = b[i], d = bi - q64[i];
      const float ri = (float)d;
      r[i] = ri;
      if (PRE) {
        const double z = (double)ri * (double)minv[i];
        rz += (double)ri * z;
        if (p) p[i] = (float)z;
      } else if (p) {
        p[i] = ri;
      }
      rr += d * d;
      bb += bi * bi;
    }
  }
  rr = block_sum(rr);
  bb = block_sum(bb);
  if (BS >= 1) rz = block_sum(rz);
  if (threadIdx.x == 0) {
    part[slot_rr * kGrid + blockIdx.x] = rr;
    if (with_bb) part[P_BB * kGrid + blockIdx.x] = bb;
    if (BS >= 1) part[slot_rz * kGrid + blockIdx.x] = rz;
  }
}

// one workgroup, behind the direction kernel of iteration `it`:  r . r of that iteration not above thr (or NaN)
// raises the flag that makes the launches enqueued behind it return at once
__global__ void __launch_bounds__(kThreads) cg_pause_kernel(const double *__restrict__ part, int *__restrict__ ic, int it, double thr) {
  if (ic[I_DONE]) return;
  const double rr = slot_sum(part, P_RR0 + ((it + 1) & 1));
  // (!(x > y): a NaN also raises it)
  if (threadIdx.x == 0 && !(rr > thr)) ic[I_DONE] = 1;
}

// u (fp64): in = first guess, out = solution.  h64 / h32: the same matrix in fp64 / fp32, whole-matrix handles on
// one device.  BS as in cg().  *iterations: fp32 iterations done;  *replacements: replacements made inside
// the loop (neither the first residual nor the closing one after maxiter counts);  *relres: the fp64 true
// residual of the returned u.
template <int BS, class Handle>
int cg_mixed(Handle *h64, Handle *h32, void *u_dev, const void *b_dev, double tol, double delta, int maxiter, int check_every,
             int *iterations, int *replacements, double *relres, hipStream_t st) {
  using cfs_rt::DevBuf;
  typedef float V;
  const long long n = h64->n();
  if (h64->rows() != h64->n() || h32->rows() != h32->n())
    return cfs_rt::set_err(CFS_HIP_ERR_UNSUPPORTED, "pcg_mixed: the handles hold a row block, not the whole matrix");
  check_every = look_window(check_every);
  double *u = (double *)u_dev;
  const double *b = (const double *)b_dev;
  DevBuf q64buf, rbuf, pbuf, qbuf, xbuf, cnt;
  Slots slots;
  Precond<V, BS> pre; // from the fp32 handle's own blocks / diagonal, by the fp32 path of cg()
  int rc;
  if ((rc = alloc_vectors<double>(n, {&q64buf})) || (rc = alloc_vectors<V>(n, {&rbuf, &pbuf, &qbuf, &xbuf})) ||
      (rc = slots.alloc(P_COUNT, st)) || (rc = cnt.alloc(I_COUNT * sizeof(int))) || (rc = slots.zero()))
    return rc;
  double *q64 = (double *)q64buf.p;
  V *r = (V *)rbuf.p, *p = (V *)pbuf.p, *q = (V *)qbuf.p, *xlo = (V *)xbuf.p;
  double *part = slots.dev();
  int *ic = (int *)cnt.p;
  HIPCHK(hipMemsetAsync(ic, 0, I_COUNT * sizeof(int), st));
  HIPCHK(hipMemsetAsync(xlo, 0, (size_t)n * sizeof(V), st));
  if ((rc = pre.setup(h32, part, st))) return rc;
  const V *dinv = pre.minv();
  const long long nb = pre.nb;
  // q64 = A u, then r = (float)(b - q64) and the scalars for the fp32 iteration number `k` that comes next;
  // `first`: p = z (or r) and b . b as well.  Synchronises; returns the true r . r in *rr_true.
  auto true_residual = [&](int k, bool first, double *rr_true) -> int {
    int r2 = h64->spmv_local(q64, u, nullptr, st);
    if (r2) return r2;
    const int slot_rr = P_RR0 + (k & 1), slot_rz = P_RZ0 + (k & 1);
    hipLaunchKernelGGL((cg_replace_kernel<BS>), dim3(kGrid), dim3(kThreads), 0, st, r, first ? p : (V *)nullptr, b,
                       (const double *)q64, n, part, slot_rr, slot_rz, first ? 1 : 0, dinv, nb);
    HIPCHK(hipGetLastError());
    if ((r2 = slots.fetch())) return r2;
    *rr_true = slots.sum(slot_rr);
    return 0;
  };
  double rr_true = 0.0;
  if ((rc = true_residual(0, true, &rr_true))) return rc;
  const double bb = slots.sum(P_BB);
  if ((rc = pre.check("pcg", slots, n))) return rc; // (read with the first host look: u has not been touched yet)
  const double stop = tol * tol * bb, drop = delta * delta;
  bool done = !(rr_true > stop); // the first guess already solves it (or b = 0, or a NaN)
  bool folded = true;            // u holds everything: xlo = 0
  double rr_ref = rr_true;
  int it = 0, nrep = 0;
  // the launches of cg<float, BS>, with xlo in the place of u, and cg_pause_kernel behind them.  The
  // direction kernels get a stop that only a NaN trips (r . r >= 0 > -1): their flag is written by workgroup 0
  // while other workgroups of the same launch may not have started, which is harmless where p is dead once the
  // flag is up, but here p is KEPT across a replacement -- a workgroup that saw the flag and returned would
  // leave its slice of p one iteration behind.  So the pause is raised by a launch of its own, after every
  // workgroup of the direction kernel has finished.  `thr`: the stopping rule, or -- when that is larger --
  // delta^2 times the reference r . r, so the DEVICE halts the recurrence at the very iteration that asks for a
  // replacement, wherever the window of enqueued iterations ends (an fp32 recurrence that ran on past that
  // point has drifted from the true residual by more than a replacement can mend: with p kept, it diverges)
  auto iteration = [&](int k, double thr) -> int {
    int r2 = h32->spmv_local(q, p, nullptr, st);
    if (r2) return r2;
    hipLaunchKernelGGL((cg_dot_kernel<V, OneColumn>), dim3(kGrid), dim3(kThreads), 0, st, (const V *)p, (const V *)q, n, n, part,
                       (int)P_PQ, (const int *)ic, OneColumn{});
    hipLaunchKernelGGL((cg_update_kernel<V, BS, num_slot(BS), OneColumn>), dim3(kGrid), dim3(kThreads), 0, st, xlo, r, (const V *)p,
                       (const V *)q, n, n, part, (const int *)ic, k, dinv, nb, OneColumn{});
    hipLaunchKernelGGL((cg_direction_kernel<V, BS, num_slot(BS), OneColumn>), dim3(kGrid), dim3(kThreads), 0, st, p, (const V *)r, n,
                       n, (const double *)part, ic, k, ColumnStops{{-1.0}}, dinv, nb, OneColumn{});
    hipLaunchKernelGGL(cg_pause_kernel, dim3(1), dim3(kThreads), 0, st, (const double *)part, ic, k, thr);
    return 0;
  };
  int host_ic[I_COUNT] = {0, 0};
  while (!done && it < maxiter) {
    const int until = std::min(maxiter, it + check_every);
    const double thr = std::max(stop, drop * rr_ref);
    for (int k = it; k < until; ++k)
      if ((rc = iteration(k, thr))) return rc;
    folded = false;
    HIPCHK(hipGetLastError());
    // host look: the counters and the slots in one synchronisation
    HIPCHK(hipMemcpyAsync(host_ic, ic, sizeof host_ic, hipMemcpyDeviceToHost, st));
    if ((rc = slots.fetch())) return rc;
    // (iterations enqueued behind a converged one did nothing: the device's count is the one that holds, and
    // its parity names the slots the next iteration reads)
    it = host_ic[I_ITER];
    const double rr = slots.sum(P_RR0 + (it & 1));
    if (rr > rr_ref) rr_ref = rr;
    // (!(x >= y): a NaN also asks for the true residual, which then ends the solve)
    if (host_ic[I_DONE] || !(rr >= drop * rr_ref)) {
      hipLaunchKernelGGL(cg_fold_kernel, dim3(kGrid), dim3(kThreads), 0, st, u, xlo, n);
      if ((rc = true_residual(it, false, &rr_true))) return rc;
      folded = true;
      ++nrep;
      // (!(x > y): a NaN residual also ends the iteration)
      if (!(rr_true > stop)) {
        done = true;
        break;
      }
      HIPCHK(hipMemsetAsync(ic + I_DONE, 0, sizeof(int), st));
      rr_ref = rr_true;
    }
  }
  if (!folded) { // maxiter reached between two replacements: the true residual of what is returned
    hipLaunchKernelGGL(cg_fold_kernel, dim3(kGrid), dim3(kThreads), 0, st, u, xlo, n);
    if ((rc = true_residual(it, false, &rr_true))) return rc;
  }
  if (iterations) *iterations = it;
  if (replacements) *replacements = nrep;
  if (relres) *relres = bb > 0.0 ? std::sqrt(rr_true / bb) : std::sqrt(rr_true);
  return 0;
}

} // namespace cfs_solver
