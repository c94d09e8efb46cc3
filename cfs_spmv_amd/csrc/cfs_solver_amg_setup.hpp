// cfs_solver_amg_setup.hpp -- the set-up of a multigrid hierarchy ON THE DEVICE (cfs_hip_amg_create_device_*), with the
// locally dominant matching of cfs_solver_amg.hpp: the hierarchy of cfs_hip_amg_create_dominant_* in every bit, the host
// builder kept as the yardstick.  Everything runs on one stream; no atomic reaches a result (the one atomicAdd counts the
// pairs of a round, an integer the host only compares with zero).
//
// LEVEL 0, from one upload of the caller's CSR:
//   amg_lower_count_kernel   per row the entries with 0 <= col <= row, and whether every row's kept columns ascend strictly
//   hipcub ExclusiveSum      the row pointers of the lower triangle
//   amg_lower_fill_kernel    columns, values in fp64, the row of every entry
// (unsorted rows or duplicates: amg_lower on the host, uploaded -- the same bits, no sum is formed on the fast path)
// PER LEVEL, the lower triangle + diagonal (rp, ci, va in fp64, row) resident:
//   amg_diagpos_kernel + amg_weight_kernel   w = 1 / sqrt(a_ii) in fp64 and in V, the bad diagonal entries counted
//   amg_scale_kernel                         b_k = (w_row a_k) w_col in place
//   per pass:
//     amg_mirror_keys_kernel + radix sort    both triangles as (row, col) keys, columns ascending, every entry with the
//                                            position in the lower array it came from;  amg_bounds_kernel: its row pointers
//     amg_strength_kernel                    s = |b_ij| / sqrt(b_ii b_jj) per entry, once per pass
//     amg_point_kernel, amg_shake_kernel     one round: every free row's first free neighbour in the total order, then the
//                                            handshake -- a kernel boundary between them, one host look per round
//     amg_head_kernel + scan + amg_number_kernel   aggregates numbered by smallest member
//     amg_galerkin_keys_kernel + radix sort  every entry of B with q[col] <= q[row] keyed (I, J); generated in the order of
//                                            the full B and sorted STABLY they stand as amg_galerkin adds them
//     amg_run_heads_kernel + scan + amg_run_fill_kernel   the lists (ptr over the sorted records) and the coarse pattern
//     amg_gather_sum_kernel                  the sums, one thread per coarse entry (LAST: rounded to V)
//     amg_compose_kernel                     agg <- q o agg
//   radix sort of (agg, row) + amg_bounds_kernel           the members of every aggregate, ascending
//   the coarse CSR to the host, once: the level's handle is made from it by the create path
#pragma once

#include <hipcub/hipcub.hpp>

namespace cfs_solver {

typedef unsigned long long amg_key_t;

template <typename V>
__global__ void __launch_bounds__(kThreads)
    amg_lower_count_kernel(const int *__restrict__ rowptr, const int *__restrict__ colind, long long n, int *__restrict__ cnt,
                           int *__restrict__ unsorted) {
  for (long long i = (long long)blockIdx.x * kThreads + threadIdx.x; i <= n; i += (long long)gridDim.x * kThreads) {
    int c = 0, prev = -1;
    bool bad = false;
    if (i < n)
      for (int k = rowptr[i]; k < rowptr[i + 1]; ++k) {
        const int j = colind[k];
        if (j < 0 || j > i) continue;
        if (j <= prev) bad = true;
        prev = j;
        ++c;
      }
    cnt[i] = c;
    if (bad) *unsorted = 1; // (every writer stores the same value)
  }
}

template <typename V>
__global__ void __launch_bounds__(kThreads)
    amg_lower_fill_kernel(const int *__restrict__ rowptr, const int *__restrict__ colind, const V *__restrict__ values, long long n,
                          const int *__restrict__ rp, int *__restrict__ ci, double *__restrict__ va, int *__restrict__ row) {
  for (long long i = (long long)blockIdx.x * kThreads + threadIdx.x; i < n; i += (long long)gridDim.x * kThreads) {
    int o = rp[i];
    for (int k = rowptr[i]; k < rowptr[i + 1]; ++k) {
      const int j = colind[k];
      if (j < 0 || j > i) continue;
      ci[o] = j;
      va[o] = (double)values[k];
      row[o] = (int)i;
      ++o;
    }
  }
}

// diag[i] = where a_ii sits: the last entry of its row, or m (an entry that holds 0: amg_weight_kernel counts it) when missing
__global__ void __launch_bounds__(kThreads)
    amg_diagpos_kernel(const int *__restrict__ rp, const int *__restrict__ ci, long long n, int m, int *__restrict__ diag) {
  for (long long i = (long long)blockIdx.x * kThreads + threadIdx.x; i < n; i += (long long)gridDim.x * kThreads) {
    const int e = rp[i + 1];
    diag[i] = (e > rp[i] && ci[e - 1] == i) ? e - 1 : m;
  }
}

// both triangles as records: entry k = (row, col) of the lower array, and its mirror (col, row) at m + k -- the mirror of
// a diagonal entry gets the row n, behind every real one.  val = k
__global__ void __launch_bounds__(kThreads)
    amg_mirror_keys_kernel(const int *__restrict__ row, const int *__restrict__ col, long long m, int n, amg_key_t *__restrict__ key,
                           int *__restrict__ val) {
  for (long long k = (long long)blockIdx.x * kThreads + threadIdx.x; k < m; k += (long long)gridDim.x * kThreads) {
    const amg_key_t i = (amg_key_t)(unsigned)row[k], j = (amg_key_t)(unsigned)col[k];
    key[k] = (i << 32) | j;
    key[m + k] = i == j ? ((amg_key_t)(unsigned)n << 32) : ((j << 32) | i);
    val[k] = (int)k;
    val[m + k] = (int)k;
  }
}

// rp[r] = the first position p < cnt with (key[p] >> shift) >= r, for r = 0 .. nrows: the row pointers of sorted keys
template <typename K>
__global__ void __launch_bounds__(kThreads)
    amg_bounds_kernel(const K *__restrict__ key, long long cnt, int shift, long long nrows, int *__restrict__ rp) {
  for (long long r = (long long)blockIdx.x * kThreads + threadIdx.x; r <= nrows; r += (long long)gridDim.x * kThreads) {
    long long lo = 0, hi = cnt;
    while (lo < hi) {
      const long long mid = (lo + hi) >> 1;
      if ((long long)(key[mid] >> shift) < r)
        lo = mid + 1;
      else
        hi = mid;
    }
    rp[r] = (int)lo;
  }
}

// s = |b_ij| / sqrt(b_ii b_jj) of every entry of the full B (0 on the diagonal: no candidate), the expression of amg_match
__global__ void __launch_bounds__(kThreads)
    amg_strength_kernel(const amg_key_t *__restrict__ fkey, const int *__restrict__ from, const double *__restrict__ va,
                        const int *__restrict__ rp, long long f, double *__restrict__ s) {
  for (long long p = (long long)blockIdx.x * kThreads + threadIdx.x; p < f; p += (long long)gridDim.x * kThreads) {
    const int i = (int)(fkey[p] >> 32), j = (int)(fkey[p] & 0xffffffffu);
    s[p] = i == j ? 0.0 : fabs(va[from[p]]) / sqrt(va[rp[i + 1] - 1] * va[rp[j + 1] - 1]);
  }
}

// to[i] = the free neighbour of the free row i over its first candidate edge in the total order, or -1: one thread per row
__global__ void __launch_bounds__(kThreads)
    amg_point_kernel(const int *__restrict__ frp, const amg_key_t *__restrict__ fkey, const double *__restrict__ s,
                     const int *__restrict__ mate, int *__restrict__ to, long long n) {
  for (long long i = (long long)blockIdx.x * kThreads + threadIdx.x; i < n; i += (long long)gridDim.x * kThreads) {
    int best = -1;
    double sbest = 0.0;
    if (mate[i] < 0)
      for (int k = frp[i]; k < frp[i + 1]; ++k) {
        const double sk = s[k];
        if (!(sk > 0.0)) continue;
        const int j = (int)(fkey[k] & 0xffffffffu);
        if (mate[j] >= 0) continue;
        if (best < 0 || amg_edge_before(sk, (int)i, j, sbest, best)) best = j, sbest = sk;
      }
    to[i] = best;
  }
}

// rows that point at each other become a pair; *made += the pairs (an integer count: its order of addition shows nowhere)
__global__ void __launch_bounds__(kThreads) amg_shake_kernel(const int *__restrict__ to, int *__restrict__ mate, long long n, int *__restrict__ made) {
  for (long long i = (long long)blockIdx.x * kThreads + threadIdx.x; i < n; i += (long long)gridDim.x * kThreads) {
    const int j = to[i];
    if (j >= 0 && to[j] == i) {
      mate[i] = j;
      if (i < j) atomicAdd(made, 1);
    }
  }
}

// head[i] = row i is the smallest member of its aggregate;  head[n] = 0
__global__ void __launch_bounds__(kThreads) amg_head_kernel(const int *__restrict__ mate, long long n, int *__restrict__ head) {
  for (long long i = (long long)blockIdx.x * kThreads + threadIdx.x; i <= n; i += (long long)gridDim.x * kThreads)
    head[i] = i < n && (mate[i] < 0 || mate[i] > i) ? 1 : 0;
}

// q[i] = the number of row i's aggregate: num = the exclusive scan of head
__global__ void __launch_bounds__(kThreads)
    amg_number_kernel(const int *__restrict__ mate, const int *__restrict__ num, long long n, int *__restrict__ q) {
  for (long long i = (long long)blockIdx.x * kThreads + threadIdx.x; i < n; i += (long long)gridDim.x * kThreads) {
    const int j = mate[i];
    q[i] = (j < 0 || j > i) ? num[i] : num[j];
  }
}

// the contributions to the lower triangle of Q^T B Q: entry p of the full B with J = q[col] <= I = q[row] keyed (I, J),
// every other one (nc, 0), behind them;  val = its position in the lower array
__global__ void __launch_bounds__(kThreads)
    amg_galerkin_keys_kernel(const amg_key_t *__restrict__ fkey, const int *__restrict__ from, const int *__restrict__ q, long long f, int nc,
                             amg_key_t *__restrict__ key, int *__restrict__ val) {
  for (long long p = (long long)blockIdx.x * kThreads + threadIdx.x; p < f; p += (long long)gridDim.x * kThreads) {
    const amg_key_t I = (amg_key_t)(unsigned)q[(int)(fkey[p] >> 32)], J = (amg_key_t)(unsigned)q[(int)(fkey[p] & 0xffffffffu)];
    key[p] = J <= I ? ((I << 32) | J) : ((amg_key_t)(unsigned)nc << 32);
    val[p] = from[p];
  }
}

// head[p] = the sorted record p is a real one (key < end) and the first of its (I, J);  head[f] = 0
__global__ void __launch_bounds__(kThreads)
    amg_run_heads_kernel(const amg_key_t *__restrict__ key, long long f, amg_key_t end, int *__restrict__ head) {
  for (long long p = (long long)blockIdx.x * kThreads + threadIdx.x; p <= f; p += (long long)gridDim.x * kThreads)
    head[p] = p < f && key[p] < end && (p == 0 || key[p] != key[p - 1]) ? 1 : 0;
}

// pos = the exclusive scan of head: coarse entry e = pos[p] of a head p begins its list at p and is (I, J); the position
// behind the last real record closes the last list
__global__ void __launch_bounds__(kThreads)
    amg_run_fill_kernel(const amg_key_t *__restrict__ key, long long f, amg_key_t end, const int *__restrict__ head, const int *__restrict__ pos,
                        int *__restrict__ ptr, int *__restrict__ row, int *__restrict__ col) {
  for (long long p = (long long)blockIdx.x * kThreads + threadIdx.x; p <= f; p += (long long)gridDim.x * kThreads) {
    if (head[p]) {
      const int e = pos[p];
      ptr[e] = (int)p;
      row[e] = (int)(key[p] >> 32);
      col[e] = (int)(key[p] & 0xffffffffu);
    }
    if ((p == f || key[p] >= end) && (p == 0 || key[p - 1] < end)) ptr[pos[p]] = (int)p;
  }
}

// agg <- q (the first pass) or q o agg
__global__ void __launch_bounds__(kThreads) amg_compose_kernel(int *__restrict__ agg, const int *__restrict__ q, long long n, int first) {
  for (long long i = (long long)blockIdx.x * kThreads + threadIdx.x; i < n; i += (long long)gridDim.x * kThreads)
    agg[i] = q[first ? (int)i : agg[i]];
}

// key = agg, val = the row: sorted stably by key, the members of every aggregate ascending
__global__ void __launch_bounds__(kThreads)
    amg_member_keys_kernel(const int *__restrict__ agg, long long n, unsigned *__restrict__ key, int *__restrict__ val) {
  for (long long i = (long long)blockIdx.x * kThreads + threadIdx.x; i < n; i += (long long)gridDim.x * kThreads)
    key[i] = (unsigned)agg[i], val[i] = (int)i;
}

inline int amg_bits(unsigned long long v) {
  int b = 1;
  while (b < 64 && (v >> b) != 0) ++b;
  return b;
}

// a device array of `bytes` with the 64 zero bytes behind it that DevBuf::upload leaves
inline int amg_alloc_padded(cfs_rt::DevBuf &b, size_t bytes, hipStream_t st) {
  int rc = b.alloc(bytes + 64);
  if (rc) return rc;
  b.bytes = bytes;
  HIPCHK(hipMemsetAsync((char *)b.p + bytes, 0, 64, st));
  return 0;
}

// the level the device holds, and the scratch of the longest one (level 0): allocated in begin(), freed with the object
template <typename V> struct AmgDeviceSetup {
  using clock = std::chrono::steady_clock;
  hipStream_t st = nullptr;
  int n = 0, cur = 0;
  long long m = 0;
  bool host_lower = false;
  cfs_rt::DevBuf rp[2], ci[2], va[2], row[2], vout, key[3], val[3], str, frp, gptr, mate, to, head, num, q, diag, w64, bad, cnt, tmp;
  size_t tmp_bytes = 0;
  double seconds[4] = {0.0, 0.0, 0.0, 0.0}; // lower + upload, matching, Galerkin + mirror, downloads
  long long scratch_bytes = 0;
  clock::time_point mark;

  int lap(int phase) { // the stream's work so far belongs to `phase`
    HIPCHK(hipStreamSynchronize(st));
    const auto now = clock::now();
    seconds[phase] += std::chrono::duration<double>(now - mark).count();
    mark = now;
    return 0;
  }
  int scan(const int *in, int *out, long long count) {
    size_t tb = tmp_bytes;
    HIPCHK(hipcub::DeviceScan::ExclusiveSum(tmp.p, tb, in, out, (int)count, st));
    return 0;
  }
  template <typename K> int sort(const K *kin, K *kout, const int *vin, int *vout_, long long count, int end_bit) {
    size_t tb = tmp_bytes;
    HIPCHK(hipcub::DeviceRadixSort::SortPairs(tmp.p, tb, kin, kout, vin, vout_, (int)count, 0, end_bit, st));
    return 0;
  }

  // level 0 from the caller's CSR, and every allocation
  int begin(int n0, const int *rowptr, const int *colind, const V *values, hipStream_t stream) {
    st = stream;
    n = n0;
    mark = clock::now();
    const long long nnz = n0 > 0 ? rowptr[n0] : 0;
    const size_t N = (size_t)n0 + 1;
    cfs_rt::DevBuf crp, cci, cva, flag, stmp;
    int rc, unsorted = 0;
    if ((rc = crp.upload(rowptr, N * sizeof(int))) || (rc = cci.upload(colind, (size_t)nnz * sizeof(int))) ||
        (rc = cva.upload(values, (size_t)nnz * sizeof(V))) || (rc = flag.alloc(sizeof(int))) || (rc = rp[0].alloc(N * sizeof(int))) ||
        (rc = rp[1].alloc(N * sizeof(int))) || (rc = head.alloc(N * sizeof(int))))
      return rc;
    HIPCHK(hipMemsetAsync(flag.p, 0, sizeof(int), st));
    hipLaunchKernelGGL((amg_lower_count_kernel<V>), dim3(kGrid), dim3(kThreads), 0, st, (const int *)crp.p, (const int *)cci.p, (long long)n0,
                       (int *)head.p, (int *)flag.p);
    size_t sb = 0;
    HIPCHK(hipcub::DeviceScan::ExclusiveSum(nullptr, sb, (const int *)head.p, (int *)rp[0].p, (int)N, st));
    if ((rc = stmp.alloc(sb))) return rc;
    HIPCHK(hipcub::DeviceScan::ExclusiveSum(stmp.p, sb, (const int *)head.p, (int *)rp[0].p, (int)N, st));
    int m0 = 0;
    HIPCHK(hipMemcpyAsync(&unsorted, flag.p, sizeof(int), hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(&m0, (const int *)rp[0].p + n0, sizeof(int), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    host_lower = unsorted != 0;
    AmgCsr low;
    if (host_lower) {
      amg_lower(n0, rowptr, colind, values, low);
      m0 = (int)low.nnz();
    }
    m = m0;
    const size_t M = (size_t)m0 + 1, F = 2 * (size_t)m0 + 1;
    // hipcub's temporary storage for the longest sort and scan
    size_t t1 = 0, t2 = 0, t3 = 0;
    HIPCHK(hipcub::DeviceRadixSort::SortPairs(nullptr, t1, (const amg_key_t *)nullptr, (amg_key_t *)nullptr, (const int *)nullptr,
                                              (int *)nullptr, (int)(F - 1), 0, 64, st));
    HIPCHK(hipcub::DeviceRadixSort::SortPairs(nullptr, t2, (const unsigned *)nullptr, (unsigned *)nullptr, (const int *)nullptr, (int *)nullptr,
                                              (int)N, 0, 32, st));
    HIPCHK(hipcub::DeviceScan::ExclusiveSum(nullptr, t3, (const int *)nullptr, (int *)nullptr, (int)F, st));
    tmp_bytes = std::max(t1, std::max(t2, t3)) + 256;
    for (int k = 0; k < 2; ++k)
      if ((rc = ci[k].alloc(M * sizeof(int))) || (rc = va[k].alloc(M * sizeof(double))) || (rc = row[k].alloc(M * sizeof(int)))) return rc;
    for (int k = 0; k < 3; ++k)
      if ((rc = key[k].alloc(F * sizeof(amg_key_t))) || (rc = val[k].alloc(F * sizeof(int)))) return rc;
    // (head and num also serve the run detection over the records)
    if ((rc = vout.alloc(M * sizeof(V))) || (rc = str.alloc(F * sizeof(double))) || (rc = frp.alloc(N * sizeof(int))) ||
        (rc = gptr.alloc(M * sizeof(int))) || (rc = mate.alloc(N * sizeof(int))) || (rc = to.alloc(N * sizeof(int))) ||
        (rc = head.alloc(std::max(N, F) * sizeof(int))) || (rc = num.alloc(std::max(N, F) * sizeof(int))) || (rc = q.alloc(N * sizeof(int))) ||
        (rc = diag.alloc(N * sizeof(int))) || (rc = w64.alloc(N * sizeof(double))) || (rc = bad.alloc(kGrid * sizeof(double))) ||
        (rc = cnt.alloc(CFS_HIP_AMG_MATCH_ROUNDS * sizeof(int))) || (rc = tmp.alloc(tmp_bytes)))
      return rc;
    if (host_lower) {
      std::vector<int> hrp(N), hrow((size_t)m0);
      for (size_t i = 0; i < N; ++i) hrp[i] = (int)low.rp[i];
      for (int i = 0; i < n0; ++i)
        for (long long k = low.rp[i]; k < low.rp[(size_t)i + 1]; ++k) hrow[(size_t)k] = i;
      HIPCHK(hipMemcpyAsync(rp[0].p, hrp.data(), N * sizeof(int), hipMemcpyHostToDevice, st));
      HIPCHK(hipMemcpyAsync(ci[0].p, low.ci.data(), (size_t)m0 * sizeof(int), hipMemcpyHostToDevice, st));
      HIPCHK(hipMemcpyAsync(va[0].p, low.va.data(), (size_t)m0 * sizeof(double), hipMemcpyHostToDevice, st));
      HIPCHK(hipMemcpyAsync(row[0].p, hrow.data(), (size_t)m0 * sizeof(int), hipMemcpyHostToDevice, st));
      HIPCHK(hipStreamSynchronize(st)); // (the host arrays go away)
    } else {
      hipLaunchKernelGGL((amg_lower_fill_kernel<V>), dim3(kGrid), dim3(kThreads), 0, st, (const int *)crp.p, (const int *)cci.p,
                         (const V *)cva.p, (long long)n0, (const int *)rp[0].p, (int *)ci[0].p, (double *)va[0].p, (int *)row[0].p);
    }
    HIPCHK(hipGetLastError());
    scratch_bytes = (long long)(crp.bytes + cci.bytes + cva.bytes + vout.bytes + str.bytes + frp.bytes + gptr.bytes + mate.bytes + to.bytes +
                                head.bytes + num.bytes + q.bytes + diag.bytes + w64.bytes + bad.bytes + cnt.bytes + tmp.bytes);
    for (int k = 0; k < 2; ++k) scratch_bytes += (long long)(rp[k].bytes + ci[k].bytes + va[k].bytes + row[k].bytes);
    for (int k = 0; k < 3; ++k) scratch_bytes += (long long)(key[k].bytes + val[k].bytes);
    cur = 0;
    return lap(0); // (the caller's arrays on the device go away here, after the stream has drained)
  }

  // one level: L.agg, L.w, L.aggptr, L.aggidx on the device, the coarse matrix to `next` (values rounded to V) and
  // resident as the next level.  *nbad != 0 (returns 1): the diagonal is not positive, nothing else was done
  int coarsen(AmgLevel<V> &L, int passes, long long *nbad, AmgCsr &next, int *rounds) {
    const dim3 G(kGrid), T(kThreads);
    int rc;
    mark = clock::now();
    if ((rc = amg_alloc_padded(L.w, (size_t)n * sizeof(V), st)) || (rc = amg_alloc_padded(L.agg, (size_t)n * sizeof(int), st))) return rc;
    HIPCHK(hipMemsetAsync((double *)va[cur].p + m, 0, sizeof(double), st));
    hipLaunchKernelGGL(amg_diagpos_kernel, G, T, 0, st, (const int *)rp[cur].p, (const int *)ci[cur].p, (long long)n, (int)m, (int *)diag.p);
    hipLaunchKernelGGL((amg_weight_kernel<V>), G, T, 0, st, (double *)w64.p, (V *)L.w.p, (const double *)va[cur].p, (const int *)diag.p,
                       (long long)n, (double *)bad.p);
    std::vector<double> hbad(kGrid);
    HIPCHK(hipMemcpyAsync(hbad.data(), bad.p, kGrid * sizeof(double), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    double b = 0.0;
    for (double v : hbad) b += v;
    *nbad = (long long)b;
    if (*nbad) return 1;
    hipLaunchKernelGGL(amg_scale_kernel, G, T, 0, st, (double *)va[cur].p, (const double *)w64.p, (const int *)row[cur].p,
                       (const int *)ci[cur].p, m);
    int in = cur, nB = n;
    long long mB = m;
    for (int p = 0; p < passes; ++p) {
      const int out = 1 - in;
      const long long f = 2 * mB - nB;
      // both triangles of B
      hipLaunchKernelGGL(amg_mirror_keys_kernel, G, T, 0, st, (const int *)row[in].p, (const int *)ci[in].p, mB, nB, (amg_key_t *)key[0].p,
                         (int *)val[0].p);
      if ((rc = sort((const amg_key_t *)key[0].p, (amg_key_t *)key[1].p, (const int *)val[0].p, (int *)val[1].p, 2 * mB,
                     32 + amg_bits((unsigned long long)nB))))
        return rc;
      const amg_key_t *fkey = (const amg_key_t *)key[1].p;
      const int *from = (const int *)val[1].p;
      hipLaunchKernelGGL((amg_bounds_kernel<amg_key_t>), G, T, 0, st, fkey, f, 32, (long long)nB, (int *)frp.p);
      HIPCHK(hipGetLastError());
      if ((rc = lap(2))) return rc;
      // the matching
      hipLaunchKernelGGL(amg_strength_kernel, G, T, 0, st, fkey, from, (const double *)va[in].p, (const int *)rp[in].p, f, (double *)str.p);
      HIPCHK(hipMemsetAsync(mate.p, 0xff, (size_t)nB * sizeof(int), st));
      HIPCHK(hipMemsetAsync(cnt.p, 0, CFS_HIP_AMG_MATCH_ROUNDS * sizeof(int), st));
      int r = 0;
      while (r < CFS_HIP_AMG_MATCH_ROUNDS) {
        int made = 0;
        hipLaunchKernelGGL(amg_point_kernel, G, T, 0, st, (const int *)frp.p, fkey, (const double *)str.p, (const int *)mate.p, (int *)to.p,
                           (long long)nB);
        hipLaunchKernelGGL(amg_shake_kernel, G, T, 0, st, (const int *)to.p, (int *)mate.p, (long long)nB, (int *)cnt.p + r);
        HIPCHK(hipMemcpyAsync(&made, (const int *)cnt.p + r, sizeof(int), hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));
        ++r;
        if (!made) break;
      }
      rounds[p] = r;
      int nc = 0;
      hipLaunchKernelGGL(amg_head_kernel, G, T, 0, st, (const int *)mate.p, (long long)nB, (int *)head.p);
      if ((rc = scan((const int *)head.p, (int *)num.p, (long long)nB + 1))) return rc;
      hipLaunchKernelGGL(amg_number_kernel, G, T, 0, st, (const int *)mate.p, (const int *)num.p, (long long)nB, (int *)q.p);
      HIPCHK(hipMemcpyAsync(&nc, (const int *)num.p + nB, sizeof(int), hipMemcpyDeviceToHost, st));
      HIPCHK(hipGetLastError());
      if ((rc = lap(1))) return rc;
      // Q^T B Q
      const amg_key_t end = (amg_key_t)(unsigned)nc << 32;
      hipLaunchKernelGGL(amg_galerkin_keys_kernel, G, T, 0, st, fkey, from, (const int *)q.p, f, nc, (amg_key_t *)key[0].p, (int *)val[0].p);
      if ((rc = sort((const amg_key_t *)key[0].p, (amg_key_t *)key[2].p, (const int *)val[0].p, (int *)val[2].p, f,
                     32 + amg_bits((unsigned long long)nc))))
        return rc;
      const amg_key_t *gkey = (const amg_key_t *)key[2].p;
      hipLaunchKernelGGL(amg_run_heads_kernel, G, T, 0, st, gkey, f, end, (int *)head.p);
      if ((rc = scan((const int *)head.p, (int *)num.p, f + 1))) return rc;
      int mc = 0;
      HIPCHK(hipMemcpyAsync(&mc, (const int *)num.p + f, sizeof(int), hipMemcpyDeviceToHost, st));
      hipLaunchKernelGGL(amg_run_fill_kernel, G, T, 0, st, gkey, f, end, (const int *)head.p, (const int *)num.p, (int *)gptr.p,
                         (int *)row[out].p, (int *)ci[out].p);
      HIPCHK(hipStreamSynchronize(st)); // (mc)
      hipLaunchKernelGGL((amg_bounds_kernel<int>), G, T, 0, st, (const int *)row[out].p, (long long)mc, 0, (long long)nc, (int *)rp[out].p);
      if (p + 1 < passes)
        hipLaunchKernelGGL((amg_gather_sum_kernel<double, V, false>), G, T, 0, st, (double *)va[out].p, (V *)nullptr, (const double *)va[in].p,
                           (const int *)gptr.p, (const int *)val[2].p, (long long)mc);
      else
        hipLaunchKernelGGL((amg_gather_sum_kernel<double, V, true>), G, T, 0, st, (double *)va[out].p, (V *)vout.p, (const double *)va[in].p,
                           (const int *)gptr.p, (const int *)val[2].p, (long long)mc);
      hipLaunchKernelGGL(amg_compose_kernel, G, T, 0, st, (int *)L.agg.p, (const int *)q.p, (long long)n, p == 0 ? 1 : 0);
      HIPCHK(hipGetLastError());
      in = out, nB = nc, mB = mc;
      if ((rc = lap(2))) return rc;
    }
    // the members of every aggregate, ascending
    if ((rc = amg_alloc_padded(L.aggptr, ((size_t)nB + 1) * sizeof(int), st)) || (rc = amg_alloc_padded(L.aggidx, (size_t)n * sizeof(int), st)))
      return rc;
    hipLaunchKernelGGL(amg_member_keys_kernel, G, T, 0, st, (const int *)L.agg.p, (long long)n, (unsigned *)val[0].p, (int *)val[1].p);
    if ((rc = sort((const unsigned *)val[0].p, (unsigned *)val[2].p, (const int *)val[1].p, (int *)L.aggidx.p, (long long)n,
                   amg_bits((unsigned long long)nB))))
      return rc;
    hipLaunchKernelGGL((amg_bounds_kernel<unsigned>), G, T, 0, st, (const unsigned *)val[2].p, (long long)n, 0, (long long)nB, (int *)L.aggptr.p);
    HIPCHK(hipGetLastError());
    if ((rc = lap(2))) return rc;
    // the coarse matrix to the host
    std::vector<int> hrp((size_t)nB + 1);
    std::vector<V> hva((size_t)mB);
    next.n = nB;
    next.ci.resize((size_t)mB);
    HIPCHK(hipMemcpyAsync(hrp.data(), rp[in].p, hrp.size() * sizeof(int), hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(next.ci.data(), ci[in].p, (size_t)mB * sizeof(int), hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(hva.data(), vout.p, (size_t)mB * sizeof(V), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    next.rp.assign(hrp.begin(), hrp.end());
    next.va.resize((size_t)mB);
    for (size_t k = 0; k < (size_t)mB; ++k) next.va[k] = (double)hva[k];
    cur = in, n = nB, m = mB;
    return lap(3);
  }
};

} // namespace cfs_solver
