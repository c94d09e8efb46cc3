// cfs_solver_cheb.hpp -- a Chebyshev polynomial in M^-1 A as the preconditioner of the native PCG
// (cfs_hip_sym_pcg_cheb), the polynomial alone (cfs_hip_sym_cheb_apply) and the power method that bounds
// its interval (cfs_hip_sym_precond_lmax).  M is what the library already builds: nothing (BS = 0), the
// diagonal (BS = 1, cg_dinv_kernel) or the node blocks (BS = 2, 3, 4, 6: cg_binv_kernel, block_apply).
//
// With theta = (lmax + lmin) / 2, delta = (lmax - lmin) / 2, sigma1 = theta / delta, rho_0 = 1 / sigma1,
// z = P_m r is the Chebyshev iteration for A z = r from z = 0 in the residual-free form,
//     z_1 = d_1 = (1 / theta) M^-1 r
//     j = 1 .. m - 1:  t = A z_j;  rho_j = 1 / (2 sigma1 - rho_{j-1})
//                      d_{j+1} = rho_j rho_{j-1} d_j + (2 rho_j / delta) M^-1 (r - t);  z_{j+1} = z_j + d_{j+1}
// m - 1 products for degree m, no vector for the inner residual.  For fixed bounds P_m is a fixed linear
// operator, a polynomial in M^-1 A times M^-1, hence symmetric, and plain PCG is valid with it.  Its residual
// polynomial is 1 - lambda p(lambda) = T_m((theta - lambda) / delta) / T_m(sigma1), of modulus below 1 exactly
// for lambda in (0, lmin + lmax): P_m is positive definite as long as every eigenvalue of M^-1 A lies in that
// open interval.  That margin -- lmin above the largest eigenvalue the bound missed -- is why an lmax that is a
// little low only costs iterations, while bounds with lmin + lmax below the true lambda_max (with the default
// lmin = lmax / 30: lmax below lambda_max / 1.033; whatever lmin: lmax below lambda_max / 2) make P_m
// indefinite and PCG meaningless; the solver then still reports the true residual of what it returns.
//
// The pairs (rho_j rho_{j-1}, 2 rho_j / delta) are computed on the host in fp64 (cheb_coeffs) and passed as
// kernel arguments: an inner step has no dot product and reads no device scalar.  An outer iteration:
//   tile kernel + fold            q = A p
//   cg_dot_kernel                 pq = p . q                                      (cfs_solver.hpp)
//   cheb_update_kernel            u += (rz/pq) p;  r -= (rz/pq) q;  rr' = r . r;  z = d = (1/theta) M^-1 r
//                                 (degree 1: also rz' = r . z)
//   m - 1 times:  tile kernel + fold   t = A z        (t lives in the q buffer: q = A p has been consumed)
//                 cheb_step_kernel     one pass over r, t, d, z and M^-1: d, z written; the last one: rz' = r . z
//   cg_direction_kernel<V, 0, P_RZ0>  p = z + (rz'/rz) p: the direction kernel of cfs_solver.hpp with no stored M^-1,
//                                 beta from the r . z slots and the stored z in the place of r;  iteration count;
//                                 converged?  (rr' <= tol^2 b.b: the unpreconditioned residual, the rule of
//                                 cfs_hip_sym_pcg)
// 5 + 3 (m - 1) launches; an inner step moves 7 n words (r, t, d, z read, d, z written, M^-1 read) against
// the 13 n of a CG iteration's vector kernels.  Memory held during a solve: r, p, q, z, d and the stored M^-1.
//
// Rounding: z, d and t are stored in the value type; each update is computed in fp64 from the stored operands
// and rounded once; M^-1 (r - t) is formed in fp64 from (double)r_i - (double)t_i; r . z sums (double)r_i
// (double)z_i of the stored r and the stored final z in the fixed-order partial-sum slots of cfs_solver.hpp;
// r . r comes from the unrounded update as in cg_update_kernel.  Every kernel returns at once when
// ic[I_DONE] is set.
#pragma once

namespace cfs_solver {

constexpr int kChebMaxDegree = 16;
enum ChebLmaxSlot { L_WT = 0, L_VT, L_WW, L_COUNT }; // part[slot][kGrid] of the power method

// theta and the degree - 1 pairs c1[j-1] = rho_j rho_{j-1}, c2[j-1] = 2 rho_j / delta (host, fp64)
inline void cheb_coeffs(int degree, double lmin, double lmax, double *theta, double *c1, double *c2) {
  const double th = 0.5 * (lmax + lmin), de = 0.5 * (lmax - lmin), s1 = th / de;
  double rho = 1.0 / s1;
  *theta = th;
  for (int j = 1; j < degree; ++j) {
    const double rn = 1.0 / (2.0 * s1 - rho);
    c1[j - 1] = rn * rho;
    c2[j - 1] = 2.0 * rn / de;
    rho = rn;
  }
}

// One element of the diagonal forms (BS = 0: M = I, BS = 1: the stored dinv), in fp64
template <typename V, int BS> __device__ __forceinline__ double cheb_minv1(double x, V dinv) {
  return BS == 1 ? x * (double)dinv : x;
}

// ---- the two smoother kernels, on a set of columns CS (OneColumn or ColumnMask, cfs_solver.hpp) ----
// Column c of a vector lives at base + c ld; the columns of cs are worked on in ONE launch, the others neither read nor
// written.  The stored M^-1 of a row (its dinv word, or the packed inverse block of its node: block_load) is loaded once
// and used for every column.  There is one body: PCG and the one-column V-cycle run its OneColumn instantiation, where
// the column loop and the offsets fold away, the column-blocked V-cycle of cfs_solver_amg.hpp its ColumnMask one.  The
// two are compiled separately, so that column c of a block has the bits of the one-column kernel still rests on the
// compiler contracting both alike -- now from literally the same source text (contraction is left at the compiler's
// default) -- and test B1 of tests/test_gpu_amg_apply_cols.py remains the judge.  The r . z partial sum exists in the
// OneColumn instantiation only; a blocked launch has no dot product (the cycle asks for none).  BS = 0 (M = I) is
// instantiated for one column only.

// z_c = d_c = (V)((1 / theta) M^-1 r_c);  one column and rz_slot >= 0: part[rz_slot] <- r . z of the stored values
template <typename V, int BS, class CS>
__global__ void __launch_bounds__(kThreads)
    cheb_start_kernel(V *__restrict__ z, long long ldz, V *__restrict__ d, long long ldd, const V *__restrict__ r, long long ldr,
                      long long n, double inv_theta, int rz_slot, double *__restrict__ part, const V *__restrict__ minv, long long nb,
                      CS cs) {
  double sz = 0.0;
  if constexpr (BS >= 2) {
    for (long long k = (long long)blockIdx.x * kThreads + threadIdx.x; k < nb; k += (long long)gridDim.x * kThreads) {
      double m[BS][BS];
      block_load<V, BS>(minv, nb, k, m);
      cs.each([&](int c) {
        const V *rc = r + c * ldr;
        V *zc = z + c * ldz, *dc = d + c * ldd;
        double rd[BS], zz[BS];
#pragma unroll
        for (int i = 0; i < BS; ++i) {
          const long long g = k * BS + i;
          rd[i] = g < n ? (double)rc[g] : 0.0;
        }
        block_mul<BS>(m, rd, zz);
#pragma unroll
        for (int i = 0; i < BS; ++i) {
          const long long g = k * BS + i;
          if (g < n) {
            const V zi = (V)(inv_theta * zz[i]);
            zc[g] = zi;
            dc[g] = zi;
            if constexpr (CS::one) sz += rd[i] * (double)zi;
          }
        }
      });
    }
  } else {
    constexpr int W = Vec16<V>::W;
    typedef typename Vec16<V>::type VT;
    const long long nv = n / W, t0 = (long long)blockIdx.x * kThreads + threadIdx.x, stride = (long long)gridDim.x * kThreads;
    for (long long i = t0; i < nv; i += stride) {
      VT mv;
      if (BS == 1) mv = reinterpret_cast<const VT *>(minv)[i];
      cs.each([&](int c) {
        const VT rv = reinterpret_cast<const VT *>(r + c * ldr)[i];
        VT zv;
#pragma unroll
        for (int k = 0; k < W; ++k) {
          zv[k] = (V)(inv_theta * cheb_minv1<V, BS>((double)rv[k], BS == 1 ? mv[k] : (V)1));
          if constexpr (CS::one) sz += (double)rv[k] * (double)zv[k];
        }
        reinterpret_cast<VT *>(z + c * ldz)[i] = zv;
        reinterpret_cast<VT *>(d + c * ldd)[i] = zv;
      });
    }
    for (long long i = nv * W + t0; i < n; i += stride) {
      const V mi = BS == 1 ? minv[i] : (V)1;
      cs.each([&](int c) {
        const V ri = r[c * ldr + i];
        const V zi = (V)(inv_theta * cheb_minv1<V, BS>((double)ri, mi));
        z[c * ldz + i] = zi;
        d[c * ldd + i] = zi;
        if constexpr (CS::one) sz += (double)ri * (double)zi;
      });
    }
  }
  if constexpr (CS::one)
    if (rz_slot >= 0) { // (uniform over the grid)
      sz = block_sum(sz);
      if (threadIdx.x == 0) part[rz_slot * kGrid + blockIdx.x] = sz;
    }
}

// cg_update_kernel<V, 1> with z stored:  alpha = rz / pq;  u += alpha p;  r -= alpha q;  part[rr'] <- r . r;
// z = d = (V)((1 / theta) M^-1 r) of the ROUNDED r;  with_rz (degree 1): part[rz'] <- r . z
template <typename V, int BS>
__global__ void __launch_bounds__(kThreads)
    cheb_update_kernel(V *__restrict__ u, V *__restrict__ r, const V *__restrict__ p, const V *__restrict__ q, V *__restrict__ z,
                       V *__restrict__ d, long long n, double *__restrict__ part, const int *__restrict__ ic, int it,
                       double inv_theta, int with_rz, const V *__restrict__ minv, long long nb) {
  if (ic[I_DONE]) return;
  const double pq = slot_sum(part, P_PQ), rz_old = slot_sum(part, P_RZ0 + (it & 1));
  const double alpha = pq != 0.0 ? rz_old / pq : 0.0;
  double s = 0.0, sz = 0.0;
  if constexpr (BS >= 2) {
    for (long long k = (long long)blockIdx.x * kThreads + threadIdx.x; k < nb; k += (long long)gridDim.x * kThreads) {
      double rd[BS], zz[BS];
#pragma unroll
      for (int i = 0; i < BS; ++i) {
        const long long g = k * BS + i;
        rd[i] = 0.0;
        if (g < n) {
          u[g] = (V)((double)u[g] + alpha * (double)p[g]);
          const double ri = (double)r[g] - alpha * (double)q[g];
          const V rn = (V)ri;
          r[g] = rn;
          s += ri * ri;
          rd[i] = (double)rn;
        }
      }
      block_apply<V, BS>(minv, nb, k, rd, zz);
#pragma unroll
      for (int i = 0; i < BS; ++i) {
        const long long g = k * BS + i;
        if (g < n) {
          const V zi = (V)(inv_theta * zz[i]);
          z[g] = zi;
          d[g] = zi;
          sz += rd[i] * (double)zi;
        }
      }
    }
  } else {
    constexpr int W = Vec16<V>::W;
    typedef typename Vec16<V>::type VT;
    const long long nv = n / W, t0 = (long long)blockIdx.x * kThreads + threadIdx.x, stride = (long long)gridDim.x * kThreads;
    for (long long i = t0; i < nv; i += stride) {
      VT uv = reinterpret_cast<VT *>(u)[i], rv = reinterpret_cast<VT *>(r)[i];
      const VT pv = reinterpret_cast<const VT *>(p)[i], qv = reinterpret_cast<const VT *>(q)[i];
      VT mv, zv;
      if (BS == 1) mv = reinterpret_cast<const VT *>(minv)[i];
#pragma unroll
      for (int k = 0; k < W; ++k) {
        uv[k] = (V)((double)uv[k] + alpha * (double)pv[k]);
        const double ri = (double)rv[k] - alpha * (double)qv[k];
        rv[k] = (V)ri;
        s += ri * ri;
        zv[k] = (V)(inv_theta * cheb_minv1<V, BS>((double)rv[k], BS == 1 ? mv[k] : (V)1));
        sz += (double)rv[k] * (double)zv[k];
      }
      reinterpret_cast<VT *>(u)[i] = uv;
      reinterpret_cast<VT *>(r)[i] = rv;
      reinterpret_cast<VT *>(z)[i] = zv;
      reinterpret_cast<VT *>(d)[i] = zv;
    }
    for (long long i = nv * W + t0; i < n; i += stride) {
      u[i] = (V)((double)u[i] + alpha * (double)p[i]);
      const double ri = (double)r[i] - alpha * (double)q[i];
      const V rn = (V)ri;
      r[i] = rn;
      s += ri * ri;
      const V zi = (V)(inv_theta * cheb_minv1<V, BS>((double)rn, BS == 1 ? minv[i] : (V)1));
      z[i] = zi;
      d[i] = zi;
      sz += (double)rn * (double)zi;
    }
  }
  s = block_sum(s);
  if (with_rz) sz = block_sum(sz);
  if (threadIdx.x == 0) {
    part[(P_RR0 + ((it + 1) & 1)) * kGrid + blockIdx.x] = s;
    if (with_rz) part[(P_RZ0 + ((it + 1) & 1)) * kGrid + blockIdx.x] = sz;
  }
}

// One inner step:  d_c = (V)(c1 d_c + c2 M^-1 (r_c - t_c));  z_c = (V)(z_c + d_c);  one column and rz_slot >= 0 (the last
// step): part[rz_slot] <- r . z
template <typename V, int BS, class CS>
__global__ void __launch_bounds__(kThreads)
    cheb_step_kernel(const V *__restrict__ r, long long ldr, const V *__restrict__ t, long long ldt, V *__restrict__ d, long long ldd,
                     V *__restrict__ z, long long ldz, long long n, double c1, double c2, int rz_slot, double *__restrict__ part,
                     const int *__restrict__ ic, const V *__restrict__ minv, long long nb, CS cs) {
  if (ic[I_DONE]) return;
  double sz = 0.0;
  if constexpr (BS >= 2) {
    for (long long k = (long long)blockIdx.x * kThreads + threadIdx.x; k < nb; k += (long long)gridDim.x * kThreads) {
      double m[BS][BS];
      block_load<V, BS>(minv, nb, k, m);
      cs.each([&](int c) {
        const V *rc = r + c * ldr, *tc = t + c * ldt;
        V *zc = z + c * ldz, *dc = d + c * ldd;
        double rd[BS], w[BS], zz[BS];
#pragma unroll
        for (int i = 0; i < BS; ++i) {
          const long long g = k * BS + i;
          rd[i] = g < n ? (double)rc[g] : 0.0;
          w[i] = g < n ? rd[i] - (double)tc[g] : 0.0;
        }
        block_mul<BS>(m, w, zz);
#pragma unroll
        for (int i = 0; i < BS; ++i) {
          const long long g = k * BS + i;
          if (g < n) {
            const V di = (V)(c1 * (double)dc[g] + c2 * zz[i]);
            const V zi = (V)((double)zc[g] + (double)di);
            dc[g] = di;
            zc[g] = zi;
            if constexpr (CS::one) sz += rd[i] * (double)zi;
          }
        }
      });
    }
  } else {
    constexpr int W = Vec16<V>::W;
    typedef typename Vec16<V>::type VT;
    const long long nv = n / W, t0 = (long long)blockIdx.x * kThreads + threadIdx.x, stride = (long long)gridDim.x * kThreads;
    for (long long i = t0; i < nv; i += stride) {
      VT mv;
      if (BS == 1) mv = reinterpret_cast<const VT *>(minv)[i];
      cs.each([&](int c) {
        const VT rv = reinterpret_cast<const VT *>(r + c * ldr)[i], tv = reinterpret_cast<const VT *>(t + c * ldt)[i];
        VT dv = reinterpret_cast<VT *>(d + c * ldd)[i], zv = reinterpret_cast<VT *>(z + c * ldz)[i];
#pragma unroll
        for (int k = 0; k < W; ++k) {
          dv[k] = (V)(c1 * (double)dv[k] + c2 * cheb_minv1<V, BS>((double)rv[k] - (double)tv[k], BS == 1 ? mv[k] : (V)1));
          zv[k] = (V)((double)zv[k] + (double)dv[k]);
          if constexpr (CS::one) sz += (double)rv[k] * (double)zv[k];
        }
        reinterpret_cast<VT *>(d + c * ldd)[i] = dv;
        reinterpret_cast<VT *>(z + c * ldz)[i] = zv;
      });
    }
    for (long long i = nv * W + t0; i < n; i += stride) {
      const V mi = BS == 1 ? minv[i] : (V)1;
      cs.each([&](int c) {
        const V ri = r[c * ldr + i];
        const V di = (V)(c1 * (double)d[c * ldd + i] + c2 * cheb_minv1<V, BS>((double)ri - (double)t[c * ldt + i], mi));
        const V zi = (V)((double)z[c * ldz + i] + (double)di);
        d[c * ldd + i] = di;
        z[c * ldz + i] = zi;
        if constexpr (CS::one) sz += (double)ri * (double)zi;
      });
    }
  }
  if constexpr (CS::one)
    if (rz_slot >= 0) { // (uniform over the grid)
      sz = block_sum(sz);
      if (threadIdx.x == 0) part[rz_slot * kGrid + blockIdx.x] = sz;
    }
}

// ---- the power method on M^-1 A ------------------------------------------------------------------
// v <- v0 (the caller's, or the start vector of cfs_hip_sym_eigs), as values of V
template <typename V>
__global__ void __launch_bounds__(kThreads) cheb_lmax_start_kernel(V *__restrict__ v, const V *__restrict__ v0, long long n) {
  for (long long i = (long long)blockIdx.x * kThreads + threadIdx.x; i < n; i += (long long)gridDim.x * kThreads)
    v[i] = v0 ? v0[i] : (V)eigs_default_v0(i);
}

// w = (V)(M^-1 t);  part <- w . t, v . t, w . w of the stored values
template <typename V, int BS>
__global__ void __launch_bounds__(kThreads)
    cheb_lmax_apply_kernel(V *__restrict__ w, const V *__restrict__ t, const V *__restrict__ v, long long n,
                           double *__restrict__ part, const V *__restrict__ minv, long long nb) {
  double wt = 0.0, vt = 0.0, ww = 0.0;
  if constexpr (BS >= 2) {
    for (long long k = (long long)blockIdx.x * kThreads + threadIdx.x; k < nb; k += (long long)gridDim.x * kThreads) {
      double td[BS], zz[BS];
#pragma unroll
      for (int i = 0; i < BS; ++i) {
        const long long g = k * BS + i;
        td[i] = g < n ? (double)t[g] : 0.0;
      }
      block_apply<V, BS>(minv, nb, k, td, zz);
#pragma unroll
      for (int i = 0; i < BS; ++i) {
        const long long g = k * BS + i;
        if (g < n) {
          const V wi = (V)zz[i];
          w[g] = wi;
          wt += (double)wi * td[i];
          vt += (double)v[g] * td[i];
          ww += (double)wi * (double)wi;
        }
      }
    }
  } else {
    for (long long i = (long long)blockIdx.x * kThreads + threadIdx.x; i < n; i += (long long)gridDim.x * kThreads) {
      const double ti = (double)t[i];
      const V wi = (V)cheb_minv1<V, BS>(ti, BS == 1 ? minv[i] : (V)1);
      w[i] = wi;
      wt += (double)wi * ti;
      vt += (double)v[i] * ti;
      ww += (double)wi * (double)wi;
    }
  }
  wt = block_sum(wt);
  vt = block_sum(vt);
  ww = block_sum(ww);
  if (threadIdx.x == 0) {
    part[L_WT * kGrid + blockIdx.x] = wt;
    part[L_VT * kGrid + blockIdx.x] = vt;
    part[L_WW * kGrid + blockIdx.x] = ww;
  }
}

// v = (V)(w / sqrt(w . w)), the scalar read on the device (w . w not finite and > 0: v = w)
template <typename V>
__global__ void __launch_bounds__(kThreads)
    cheb_lmax_normalise_kernel(V *__restrict__ v, const V *__restrict__ w, long long n, const double *__restrict__ part) {
  const double ww = slot_sum(part, L_WW);
  const double nrm = (ww > 0.0 && ww * 0.0 == 0.0) ? sqrt(ww) : 1.0;
  for (long long i = (long long)blockIdx.x * kThreads + threadIdx.x; i < n; i += (long long)gridDim.x * kThreads)
    v[i] = (V)((double)w[i] / nrm);
}

// ---- host ----------------------------------------------------------------------------------------
// (the stored M^-1 of a call is Precond<V, BS> of cfs_solver.hpp)

// the m - 1 inner steps behind a z = d = z_1 that is already enqueued, on the columns of cs: per step one product per
// column, then ONE step kernel.  Column c of z at z + c ldz, of r at r + c ldr, of d and of t (n values of scratch per
// column) at + c ldw
template <typename V, int BS, class CS, class Handle>
int cheb_chain(Handle *h, CS cs, V *z, long long ldz, V *d, V *t, long long ldw, const V *r, long long ldr, long long n, int degree,
               const double *c1, const double *c2, int rz_slot, double *part, const int *ic, const V *minv, long long nb, hipStream_t st) {
  for (int j = 1; j < degree; ++j) {
    int rc = 0;
    cs.each([&](int c) {
      if (!rc) rc = h->spmv_local(t + c * ldw, z + c * ldz, nullptr, st);
    });
    if (rc) return rc;
    hipLaunchKernelGGL((cheb_step_kernel<V, BS, CS>), dim3(kGrid), dim3(kThreads), 0, st, r, ldr, (const V *)t, ldw, d, ldw, z, ldz, n,
                       c1[j - 1], c2[j - 1], j == degree - 1 ? rz_slot : -1, part, ic, minv, nb, cs);
  }
  return 0;
}

// `steps` power steps on M^-1 A from the start vector v0 (nullptr: that of cfs_hip_sym_eigs); v, t, w: n values each.
// One host look, after the last step.  lpart: the caller's (it lives as long as the caller's buffers), allocated here
// unless an earlier call has done so
template <typename V, int BS, class Handle>
int cheb_power(Handle *h, V *v, V *t, V *w, const V *v0, long long n, int steps, Slots &lpart, const V *minv, long long nb,
               double *estimate, hipStream_t st) {
  int rc;
  if (lpart.buf.p && lpart.host.size() == (size_t)L_COUNT * kGrid)
    lpart.st = st;
  else if ((rc = lpart.alloc(L_COUNT, st)))
    return rc;
  if ((rc = lpart.zero())) return rc;
  hipLaunchKernelGGL((cheb_lmax_start_kernel<V>), dim3(kGrid), dim3(kThreads), 0, st, v, v0, n);
  for (int s = 0; s < steps; ++s) {
    if ((rc = h->spmv_local(t, v, nullptr, st))) return rc;
    hipLaunchKernelGGL((cheb_lmax_apply_kernel<V, BS>), dim3(kGrid), dim3(kThreads), 0, st, w, (const V *)t, (const V *)v, n,
                       lpart.dev(), minv, nb);
    if (s + 1 < steps)
      hipLaunchKernelGGL((cheb_lmax_normalise_kernel<V>), dim3(kGrid), dim3(kThreads), 0, st, v, (const V *)w, n,
                         (const double *)lpart.dev());
  }
  HIPCHK(hipGetLastError());
  if ((rc = lpart.fetch())) return rc;
  *estimate = lpart.sum(L_WT) / lpart.sum(L_VT);
  return 0;
}

// cfs_hip_sym_precond_lmax
template <typename V, int BS, class Handle>
int cheb_lmax(Handle *h, int steps, const void *v0_dev, double *estimate, hipStream_t st) {
  using cfs_rt::DevBuf;
  const long long n = h->n();
  if (h->rows() != h->n()) return cfs_rt::set_err(CFS_HIP_ERR_UNSUPPORTED, "precond_lmax: the handle holds a row block, not the whole matrix");
  if (steps <= 0) steps = 16;
  DevBuf vbuf, tbuf, wbuf;
  Slots part, lpart;
  Precond<V, BS> pre;
  int rc;
  if ((rc = alloc_vectors<V>(n, {&vbuf, &tbuf, &wbuf})) || (rc = part.alloc(P_COUNT, st)) || (rc = part.zero()) ||
      (rc = pre.setup(h, part.dev(), st)) ||
      (rc = cheb_power<V, BS>(h, (V *)vbuf.p, (V *)tbuf.p, (V *)wbuf.p, (const V *)v0_dev, n, steps, lpart, pre.minv(), pre.nb, estimate, st)) ||
      (rc = part.fetch()))
    return rc;
  return pre.check("precond_lmax", part, n);
}

// cfs_hip_sym_cheb_apply: z = P_m r
template <typename V, int BS, class Handle>
int cheb_apply(Handle *h, int degree, double lmin, double lmax, void *z_dev, const void *r_dev, hipStream_t st) {
  using cfs_rt::DevBuf;
  const long long n = h->n();
  if (h->rows() != h->n()) return cfs_rt::set_err(CFS_HIP_ERR_UNSUPPORTED, "cheb_apply: the handle holds a row block, not the whole matrix");
  DevBuf dvec, tvec, cnt;
  Slots part;
  Precond<V, BS> pre;
  int rc;
  if ((rc = alloc_vectors<V>(n, {&dvec, &tvec})) || (rc = part.alloc(P_COUNT, st)) || (rc = cnt.alloc(I_COUNT * sizeof(int))) ||
      (rc = part.zero()))
    return rc;
  HIPCHK(hipMemsetAsync(cnt.p, 0, I_COUNT * sizeof(int), st));
  if ((rc = pre.setup(h, part.dev(), st))) return rc;
  double theta, c1[kChebMaxDegree], c2[kChebMaxDegree];
  cheb_coeffs(degree, lmin, lmax, &theta, c1, c2);
  hipLaunchKernelGGL((cheb_start_kernel<V, BS, OneColumn>), dim3(kGrid), dim3(kThreads), 0, st, (V *)z_dev, n, (V *)dvec.p, n,
                     (const V *)r_dev, n, n, 1.0 / theta, -1, part.dev(), pre.minv(), pre.nb, OneColumn{});
  if ((rc = cheb_chain<V, BS>(h, OneColumn{}, (V *)z_dev, n, (V *)dvec.p, (V *)tvec.p, n, (const V *)r_dev, n, n, degree, c1, c2, -1,
                              part.dev(), (const int *)cnt.p, pre.minv(), pre.nb, st)))
    return rc;
  HIPCHK(hipGetLastError());
  if ((rc = part.fetch())) return rc;
  return pre.check("cheb_apply", part, n);
}

// cfs_hip_sym_pcg_cheb.  u: in = first guess, out = solution; lmin / lmax <= 0: the defaults (cfs_hip.h)
template <typename V, int BS, class Handle>
int cg_cheb(Handle *h, void *u_dev, const void *b_dev, int degree, double lmin, double lmax, double tol, int maxiter, int check_every,
            int *iterations, double *relres, double *bounds_used, hipStream_t st) {
  // (the cap of cg(); an iteration here is 5 + 3 (m - 1) launches)
  check_every = look_window(check_every, std::min(16, std::max(1, 80 / (5 + 3 * (degree - 1)))));
  Pcg<V, Handle> s;
  Precond<V, BS> pre;
  cfs_rt::DevBuf zbuf, dvec;
  Slots lpart;
  int rc;
  if ((rc = s.begin("pcg_cheb", h, u_dev, b_dev, tol, maxiter, st)) || (rc = alloc_vectors<V>(s.n, {&zbuf, &dvec})) ||
      (rc = pre.setup(h, s.part.dev(), st)) || (rc = s.first_residual()) || (rc = pre.check("pcg_cheb", s.part, s.n)))
    return rc; // (u has not been touched yet)
  V *u = s.u, *r = s.r, *p = s.p, *q = s.q, *z = (V *)zbuf.p, *d = (V *)dvec.p;
  const long long n = s.n, nb = pre.nb;
  double *part = s.part.dev();
  int *ic = s.ic;
  const V *minv = pre.minv();
  if (!(lmax > 0.0)) { // the power method, in the buffers the iteration does not use yet
    double est = 0.0;
    if ((rc = cheb_power<V, BS>(h, p, q, z, (const V *)nullptr, n, 16, lpart, minv, nb, &est, st))) return rc;
    if (!(est > 0.0) || est * 0.0 != 0.0)
      return cfs_rt::set_err(CFS_HIP_ERR_ARG, "pcg_cheb: the power method gave no positive estimate of lambda_max(M^-1 A) (" +
                                                  std::to_string(est) + "): pass lmax");
    lmax = 1.1 * est;
  }
  if (!(lmin > 0.0)) lmin = lmax / 30.0;
  if (!(lmin < lmax))
    return cfs_rt::set_err(CFS_HIP_ERR_ARG, "pcg_cheb: lmin " + std::to_string(lmin) + " is not below the estimated lmax " +
                                                std::to_string(lmax));
  if (bounds_used) bounds_used[0] = lmin, bounds_used[1] = lmax;
  double theta, c1[kChebMaxDegree], c2[kChebMaxDegree];
  cheb_coeffs(degree, lmin, lmax, &theta, c1, c2);
  const double inv_theta = 1.0 / theta;
  const ColumnStops stop{{s.stop}};
  if (s.live()) { // z = P_m r, rz[0] = r . z, p = z
    hipLaunchKernelGGL((cheb_start_kernel<V, BS, OneColumn>), dim3(kGrid), dim3(kThreads), 0, st, z, n, d, n, (const V *)r, n, n,
                       inv_theta, degree == 1 ? (int)P_RZ0 : -1, part, minv, nb, OneColumn{});
    if ((rc = cheb_chain<V, BS>(h, OneColumn{}, z, n, d, q, n, (const V *)r, n, n, degree, c1, c2, (int)P_RZ0, part, (const int *)ic, minv,
                                nb, st)))
      return rc;
    HIPCHK(hipMemcpyAsync(p, z, (size_t)n * sizeof(V), hipMemcpyDeviceToDevice, st));
  }
  auto iteration = [&](int k) -> int {
    int r2 = h->spmv_local(q, p, nullptr, st);
    if (r2) return r2;
    hipLaunchKernelGGL((cg_dot_kernel<V, OneColumn>), dim3(kGrid), dim3(kThreads), 0, st, (const V *)p, (const V *)q, n, n, part,
                       (int)P_PQ, (const int *)ic, OneColumn{});
    hipLaunchKernelGGL((cheb_update_kernel<V, BS>), dim3(kGrid), dim3(kThreads), 0, st, u, r, (const V *)p, (const V *)q, z, d, n, part,
                       (const int *)ic, k, inv_theta, degree == 1 ? 1 : 0, minv, nb);
    if ((r2 = cheb_chain<V, BS>(h, OneColumn{}, z, n, d, q, n, (const V *)r, n, n, degree, c1, c2, (int)P_RZ0 + ((k + 1) & 1), part,
                                (const int *)ic, minv, nb, st)))
      return r2;
    hipLaunchKernelGGL((cg_direction_kernel<V, 0, P_RZ0, OneColumn>), dim3(kGrid), dim3(kThreads), 0, st, p, (const V *)z, n, n,
                       (const double *)part, ic, k, stop, (const V *)nullptr, 0LL, OneColumn{});
    return 0;
  };
  while (s.live()) {
    for (const int until = s.window_end(check_every); s.it < until; ++s.it)
      if ((rc = iteration(s.it))) return rc;
    if ((rc = s.look())) return rc;
  }
  return s.finish(iterations, relres);
}

} // namespace cfs_solver
