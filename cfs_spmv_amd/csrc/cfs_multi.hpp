// cfs_multi.hpp -- one host thread, N GPUs (the C++ surface with CFS_NUM_GPUS=N; reference knob:
// CFS_NUM_THREADS, src/runtime.cpp:10-21): N 1-D row-block shards, one per device, each on a
// stream of its own.  x and y stay where the caller put them (the handle's HOME device); a shard
// on another device reads x and writes its rows of y through peer access over xGMI, or works on
// copies (x modes below).  An SpMV is ordered like any other work of the caller's stream: the
// shard streams wait for an event recorded on it (fork), it waits for theirs (join).  (The
// performance path for several GPUs is one process per GPU, bench.py; this is the drop-in path
// of an unmodified single-process caller.)
//
// Included by cfs_hip.hip, behind cfs_hip_sym_s and cfs_comm.hpp.
#pragma once

// one shard (cfs_hip.hip, below the include of this file)
template <typename V>
static int sym_create(int n, const int *rowptr, const int *colind, const V *values, int nranks, int rank,
                      const int *row_splits, const cfs_hip_options *opt, cfs_hip_sym_t *out);

// the dense form of the exchange (north-star: reduce-scatter of the off-block contributions):
// a shard's packed contributions go to their slot of a zeroed vector of nranks equal blocks ...
template <typename V>
__global__ void __launch_bounds__(256)
    cfs_scatter_pos_kernel(V *__restrict__ dense, const int32_t *__restrict__ pos, const V *__restrict__ packed, int m) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i < m) dense[pos[i]] = packed[i];
}
// ... and the block a rank receives is added to its rows
template <typename V>
__global__ void __launch_bounds__(256) cfs_add_rows_kernel(V *__restrict__ y, const V *__restrict__ add, int m) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i < m) y[i] += add[i];
}

// one row block: where it lives, what orders it, and its buffers (on `dev`, allocated at first use)
struct Shard {
  int dev = 0;
  hipStream_t st = nullptr;
  hipEvent_t done = nullptr;
  std::unique_ptr<cfs_hip_sym_s> h;
  DevBuf xrep, yloc;                     // the x modes that copy: x replicated, the local y block
  DevBuf sbuf, pos, dense, rsout, rbuf;  // the exchange forms
  int nsend = 0;
};

struct MultiSym : cfs_hip_sym_s {
  std::vector<Shard> shards;
  std::vector<int> splits;
  hipEvent_t start_ = nullptr;
  int n_ = 0;
  std::vector<int32_t> none_;
  // How a shard on another device than the handle's home reaches x and y:
  //   CFS_HIP_XMODE_REPLICATE (default)  x is REPLICATED (north-star / SURVEY 8e): one
  //       hipMemcpyPeerAsync home -> device per shard and SpMV into the shard's own copy,
  //       the kernels gather x and write their y block in LOCAL HBM, one peer copy brings
  //       the block home;
  //   CFS_HIP_XMODE_PEER  the kernels read x and write y in the home device's memory
  //       through peer access over xGMI (no copies, every gather crosses the fabric).
  // Shards on the home device itself never copy.  CFS_HIP_XMODE_REPLICATE_ALL copies for
  // every shard, home or not: the way a one-GPU box exercises the copy path.
  int xmode = CFS_HIP_XMODE_REPLICATE;
  int rows_of(size_t g) const { return splits[g + 1] - splits[g]; }
  bool copies(size_t g) const {
    return xmode == CFS_HIP_XMODE_REPLICATE_ALL || (xmode == CFS_HIP_XMODE_REPLICATE && shards[g].dev != device);
  }
  int ensure_copies(size_t g) {
    Shard &s = shards[g];
    if (s.xrep.p) return 0;
    DeviceGuard dg(s.dev);
    int rc;
    if ((rc = s.xrep.alloc((size_t)n_ * value_bytes))) return rc;
    return s.yloc.alloc((size_t)rows_of(g) * value_bytes);
  }

  // ---- the skeleton of everything a handle enqueues: fork, per shard { local_xy, work,
  // bring_home }, join.  The per-shard steps run under the shard's DeviceGuard. ----
  // the shard streams run behind what the caller's stream holds now
  int fork(hipStream_t st) {
    HIPCHK(hipEventRecord(start_, st));
    for (Shard &s : shards) {
      DeviceGuard dg(s.dev);
      HIPCHK(hipStreamWaitEvent(s.st, start_, 0));
    }
    return 0;
  }
  // the (x, y) shard g works on: the caller's x and the shard's rows of the caller's y in place, or --
  // copies(g) -- the shard's own copy of x, brought over here (x = NULL: nothing to bring), and its
  // local y block
  struct XY {
    const void *x;
    void *y;
  };
  int local_xy(size_t g, const void *x, void *y, XY *w) {
    Shard &s = shards[g];
    *w = {x, (char *)y + (size_t)splits[g] * value_bytes};
    if (!copies(g)) return 0;
    int rc = ensure_copies(g);
    if (rc) return rc;
    if (x) HIPCHK(hipMemcpyPeerAsync(s.xrep.p, s.dev, x, device, (size_t)n_ * value_bytes, s.st));
    *w = {s.xrep.p, s.yloc.p};
    return 0;
  }
  // the local y block of shard g to its rows of the caller's y
  int bring_home(size_t g, void *y) {
    Shard &s = shards[g];
    const size_t bytes = (size_t)rows_of(g) * value_bytes;
    if (copies(g) && bytes)
      HIPCHK(hipMemcpyPeerAsync((char *)y + (size_t)splits[g] * value_bytes, device, s.yloc.p, s.dev, bytes, s.st));
    return 0;
  }
  // the caller's stream runs behind what the shard streams hold now
  int join(hipStream_t st) {
    for (Shard &s : shards) {
      DeviceGuard dg(s.dev);
      HIPCHK(hipEventRecord(s.done, s.st));
    }
    for (Shard &s : shards) HIPCHK(hipStreamWaitEvent(st, s.done, 0));
    return 0;
  }
  // every shard stream drained (a shard whose create failed may have none)
  int sync_shards() {
    for (Shard &s : shards) {
      DeviceGuard dg(s.dev);
      if (s.st) HIPCHK(hipStreamSynchronize(s.st));
    }
    return 0;
  }

  // Exchange form (CFS_HIP_FLAG_SHARD_EXCHANGE at create, or CFS_MULTI_EXCHANGE=reduce_scatter):
  // the shards keep their off-block entries two-sided, pack the contributions to rows of lower
  // ranks, scatter them into a dense vector of N equal blocks and ONE native reduce-scatter
  // (cfs_hip_comm_*: RCCL over xGMI, or the peer transport) hands every owner its sums --
  // the north-star's form, without Python.  The local fold runs beside the collective.
  //
  // Two forms of that exchange on one handle (cfs_hip_sym_multi_set_exchange; the buffers of a
  // form are allocated at its first use):
  //   CFS_HIP_EXCHANGE_REDUCE_SCATTER  the dense one above: memset, tiles, pack, scatter, the sum
  //       kernel (or ncclReduceScatter), local fold, add -- N * rs_rows values per rank;
  //   CFS_HIP_EXCHANGE_SPARSE  the packed all-to-all (cfs_hip_comm_alltoallv): tiles, pack, the
  //       pull kernel (or grouped ncclSend / ncclRecv), local fold, fold of what arrived -- one
  //       value per remote boundary row, no memset, no scatter, no add.
  std::unique_ptr<cfs_hip_comm_s> comm;
  int form = CFS_HIP_EXCHANGE_REDUCE_SCATTER;
  int rs_rows = 0; // block length of the reduce-scatter (longest row block)
  std::vector<int64_t> a2a_counts_; // N x N, [g * N + r] = values shard g packs for shard r
  bool dense_ready_ = false, sparse_ready_ = false;
  template <typename V> int setup_exchange(int transport, int first_form) {
    const int N = (int)shards.size();
    int devs[cfs_rt::kMaxDevices];
    for (int g = 0; g < N; g++) devs[g] = shards[g].dev;
    cfs_hip_comm_t c = nullptr;
    int rc = cfs_hip_comm_create(N, devs, transport, &c);
    if (rc) return rc;
    comm.reset(c);
    rs_rows = 0;
    for (int g = 0; g < N; g++) rs_rows = std::max(rs_rows, rows_of(g));
    for (Shard &s : shards) {
      DeviceGuard dg(s.dev);
      s.nsend = (int)s.h->send_rows().size();
      if ((rc = s.sbuf.alloc(std::max<size_t>(1, (size_t)s.nsend) * sizeof(V)))) return rc;
    }
    if ((rc = ensure_form<V>(first_form))) return rc;
    form = first_form;
    return 0;
  }
  template <typename V> int ensure_form(int f) {
    const int N = (int)shards.size();
    int rc;
    if (f == CFS_HIP_EXCHANGE_REDUCE_SCATTER && !dense_ready_) {
      for (Shard &s : shards) {
        DeviceGuard dg(s.dev);
        const std::vector<int32_t> &rows = s.h->send_rows();
        std::vector<int32_t> p(rows.size());
        for (size_t k = 0; k < rows.size(); k++) {
          const int owner = (int)(std::upper_bound(splits.begin(), splits.end(), rows[k]) - splits.begin()) - 1;
          p[k] = owner * rs_rows + (rows[k] - splits[owner]);
        }
        if ((rc = s.pos.upload(p.data(), p.size() * 4)) || (rc = s.dense.alloc((size_t)N * rs_rows * sizeof(V))) ||
            (rc = s.rsout.alloc((size_t)rs_rows * sizeof(V))))
          return rc;
        // this shard receives nothing through the sparse route: recv side stays empty
      }
      dense_ready_ = true;
    }
    if (f == CFS_HIP_EXCHANGE_SPARSE && !sparse_ready_) {
      // the receive side: for every owner r the rows of each (higher) rank's send_rows() that are
      // destined for r, concatenated by source rank -- the order cfs_hip_comm_alltoallv delivers
      a2a_counts_.assign((size_t)N * N, 0);
      std::vector<size_t> first((size_t)N * N, 0); // [g * N + r]: where g's block for r starts
      for (int g = 0; g < N; g++) {
        const std::vector<int32_t> &sc = shards[g].h->send_counts();
        size_t off = 0;
        for (int r = 0; r < N && r < (int)sc.size(); r++) {
          a2a_counts_[(size_t)g * N + r] = sc[r];
          first[(size_t)g * N + r] = off;
          off += (size_t)sc[r];
        }
        if (off != shards[g].h->send_rows().size()) return set_err(CFS_HIP_ERR_INTERNAL, "send counts and send rows disagree");
      }
      for (int r = 0; r < N; r++) {
        DeviceGuard dg(shards[r].dev);
        std::vector<int> rows;
        for (int g = 0; g < N; g++) {
          const std::vector<int32_t> &sr = shards[g].h->send_rows();
          const size_t b = first[(size_t)g * N + r];
          rows.insert(rows.end(), sr.begin() + b, sr.begin() + b + (size_t)a2a_counts_[(size_t)g * N + r]);
        }
        if ((rc = shards[r].h->set_recv((int)rows.size(), rows.data())) ||
            (rc = shards[r].rbuf.alloc(std::max<size_t>(1, rows.size()) * sizeof(V))))
          return rc;
      }
      sparse_ready_ = true;
    }
    return 0;
  }
  // Both exchange forms, per shard stream: [x over], wait_consumed, {dense: memset of the dense
  // vector}, tiles + pack into sbuf, {dense: scatter into the dense vector}, the collective (dense:
  // reduce-scatter into rsout; sparse: all-to-all into rbuf), local fold, {dense: rsout added to the
  // rows; sparse: fold of rbuf}, [y block home].  `phases` of the caller is not looked at.
  // (Stream order: the local fold is enqueued behind this rank's part of the collective; on the
  // RCCL transport the two run on the same stream, on the peer transport the sum / pull kernel is
  // short -- overlapping them needs a second stream per shard and has not been measured.)
  template <typename V> int spmv_exchange(void *y, const void *x, hipStream_t st) {
    const int N = (int)shards.size();
    const bool dense = form != CFS_HIP_EXCHANGE_SPARSE;
    // (the collectives read these tables before they return)
    void *sp[cfs_rt::kMaxDevices], *rp[cfs_rt::kMaxDevices], *streams[cfs_rt::kMaxDevices];
    XY w[cfs_rt::kMaxDevices];
    int rc;
    if ((rc = fork(st))) return rc;
    for (int g = 0; g < N; g++) {
      Shard &s = shards[g];
      DeviceGuard dg(s.dev);
      if ((rc = local_xy(g, x, y, &w[g])) || (rc = cfs_hip_comm_wait_consumed(comm.get(), g, s.st))) return rc;
      if (dense) HIPCHK(hipMemsetAsync(s.dense.p, 0, (size_t)N * rs_rows * sizeof(V), s.st));
      if ((rc = s.h->spmv_local(w[g].y, w[g].x, s.sbuf.p, s.st, CFS_HIP_PHASE_TILES | CFS_HIP_PHASE_PACK))) return rc;
      if (dense && s.nsend > 0)
        hipLaunchKernelGGL((cfs_scatter_pos_kernel<V>), dim3((s.nsend + 255) / 256), dim3(256), 0, s.st,
                           (V *)s.dense.p, (const int32_t *)s.pos.p, (const V *)s.sbuf.p, s.nsend);
      sp[g] = dense ? s.dense.p : s.sbuf.p;
      rp[g] = dense ? s.rsout.p : s.rbuf.p;
      streams[g] = (void *)s.st;
    }
    rc = dense ? cfs_hip_comm_reduce_scatter(comm.get(), sp, rp, (size_t)rs_rows, value_bytes, streams)
               : cfs_hip_comm_alltoallv(comm.get(), sp, rp, a2a_counts_.data(), value_bytes, streams);
    if (rc) return rc;
    for (int g = 0; g < N; g++) {
      Shard &s = shards[g];
      DeviceGuard dg(s.dev);
      const int rows_g = rows_of(g);
      if ((rc = s.h->spmv_local(w[g].y, w[g].x, s.sbuf.p, s.st, CFS_HIP_PHASE_FOLD))) return rc;
      if (!dense) {
        if ((rc = s.h->recv_fold(w[g].y, s.rbuf.p, s.st))) return rc;
      } else if (rows_g > 0) {
        hipLaunchKernelGGL((cfs_add_rows_kernel<V>), dim3((rows_g + 255) / 256), dim3(256), 0, s.st, (V *)w[g].y,
                           (const V *)s.rsout.p, rows_g);
      }
      if ((rc = bring_home(g, y))) return rc;
    }
    if ((rc = join(st))) return rc;
    HIPCHK(hipGetLastError());
    return 0;
  }
  // per shard, under its device: stream drained, handle, event, stream; then start_, the communicator,
  // and (members) the buffers
  ~MultiSym() override {
    (void)sync_shards();
    for (Shard &s : shards) {
      DeviceGuard dg(s.dev);
      s.h.reset();
      if (s.done) (void)hipEventDestroy(s.done);
      if (s.st) (void)hipStreamDestroy(s.st);
    }
    if (start_) {
      DeviceGuard dg(device);
      (void)hipEventDestroy(start_);
    }
    comm.reset();
  }
  // mirrored shards: nothing to exchange, every shard writes its rows (tiles and fold of `phases`)
  int spmv_local(void *y, const void *x, void *, hipStream_t st, int phases) override {
    if (comm) return cfs_rt::with_value_type(value_bytes, [&](auto v) { return spmv_exchange<decltype(v)>(y, x, st); });
    int rc;
    if ((rc = fork(st))) return rc;
    for (size_t g = 0; g < shards.size(); g++) {
      Shard &s = shards[g];
      DeviceGuard dg(s.dev);
      XY w;
      if ((rc = local_xy(g, x, y, &w)) ||
          (rc = s.h->spmv_local(w.y, w.x, nullptr, s.st, phases & (CFS_HIP_PHASE_TILES | CFS_HIP_PHASE_FOLD))) ||
          (rc = bring_home(g, y)))
        return rc;
    }
    return join(st);
  }
  int recv_fold(void *, const void *, hipStream_t) override { return 0; }
  int set_recv(int, const int *) override { return set_err(CFS_HIP_ERR_ARG, "not a shard"); }
  void stats(cfs_hip_sym_stats *o) override {
    memset(o, 0, sizeof *o);
    for (Shard &s : shards) {
      cfs_hip_sym_stats t;
      s.h->stats(&t);
      o->nnz_low += t.nnz_low;
      o->nnz_diag += t.nnz_diag;
      o->nnz_full += t.nnz_full;
      o->ntiles += t.ntiles;
      o->nslices += t.nslices;
      o->halo_slots += t.halo_slots;
      o->fold_rows += t.fold_rows;
      o->bytes_algorithmic += t.bytes_algorithmic;
      o->bytes_streamed += t.bytes_streamed;
      o->device_bytes += t.device_bytes;
      o->mirror_entries += t.mirror_entries;
      o->far_entries += t.far_entries;
      o->ngroups += t.ngroups;
      o->max_slots_used = std::max(o->max_slots_used, t.max_slots_used);
      o->lds_bytes = std::max(o->lds_bytes, t.lds_bytes);
      o->block_threads = t.block_threads;
      o->value_bytes = t.value_bytes;
    }
    o->n = n_;
    o->row_begin = 0;
    o->row_end = n_;
  }
  const std::vector<int32_t> &send_counts() override { return none_; }
  const std::vector<int32_t> &send_rows() override { return none_; }
  int n() override { return n_; }
  int rows() override { return n_; }
  int timeline(void *, const void *, unsigned long long *, int, int *) override {
    return set_err(CFS_HIP_ERR_ARG, "no timeline for a multi-device handle");
  }
  int group_features(long long *, int, int *) override {
    return set_err(CFS_HIP_ERR_ARG, "no group features for a multi-device handle");
  }
  int update_values(const void *values_dev, long long nnz, hipStream_t st) override {
    // (values_dev lives on the home device; shards on other devices read it over peer access)
    HIPCHK(hipStreamSynchronize(st));
    for (Shard &s : shards) {
      DeviceGuard dg(s.dev);
      int rc = s.h->update_values(values_dev, nnz, s.st);
      if (rc) return rc;
      HIPCHK(hipStreamSynchronize(s.st));
    }
    return 0;
  }
  // every shard gathers its block on its own device and stream; the block comes home the way its
  // y block does (a peer copy in the replicate modes, written in place otherwise)
  int diagonal(void *d, hipStream_t st) override {
    int rc;
    if ((rc = fork(st))) return rc;
    for (size_t g = 0; g < shards.size(); g++) {
      Shard &s = shards[g];
      DeviceGuard dg(s.dev);
      XY w;
      if ((rc = local_xy(g, nullptr, d, &w)) || (rc = s.h->diagonal(w.y, s.st)) || (rc = bring_home(g, d))) return rc;
    }
    return join(st);
  }
  int ngpus() const { return (int)shards.size(); }
};

template <typename V>
static int sym_create_multi(int n, const int *rowptr, const int *colind, const V *values, int ngpus,
                            const int *devices, const cfs_hip_options *opt, cfs_hip_sym_t *out) {
  if (!out) return set_err(CFS_HIP_ERR_ARG, "out is NULL");
  *out = nullptr;
  if (ngpus < 1 || ngpus > cfs_rt::kMaxDevices) return set_err(CFS_HIP_ERR_ARG, "bad ngpus");
  if (n < 0 || !rowptr) return set_err(CFS_HIP_ERR_ARG, "null CSR array");
  int rc = ensure_init();
  if (rc) return rc;
  int home = 0, ndev = 0;
  HIPCHK(hipGetDevice(&home));
  HIPCHK(hipGetDeviceCount(&ndev));
  std::unique_ptr<MultiSym> m(new MultiSym());
  m->value_bytes = (int)sizeof(V);
  m->device = home;
  m->n_ = n;
  m->splits.assign(ngpus + 1, 0);
  cfs_plan::balanced_splits(n, rowptr, colind, ngpus, m->splits.data());
  if (const char *e = getenv("CFS_MULTI_X")) // peer | replicate | replicate_all
    m->xmode = !strcmp(e, "peer") ? CFS_HIP_XMODE_PEER
               : !strcmp(e, "replicate_all") ? CFS_HIP_XMODE_REPLICATE_ALL : CFS_HIP_XMODE_REPLICATE;
  {
    DeviceGuard dg(home);
    if (hipEventCreateWithFlags(&m->start_, hipEventDisableTiming) != hipSuccess)
      return set_err(CFS_HIP_ERR_DEVICE, "hipEventCreate failed");
  }
  // a part of the handle refused: its own code and message, read before the teardown (which must
  // not speak over it) and set again behind it
  auto fail = [&m](int code) {
    const std::string e = cfs_rt::last_error();
    m.reset();
    return set_err(code, e);
  };
  cfs_hip_options o2;
  memset(&o2, 0, sizeof o2);
  if (opt) o2 = *opt;
  // default: mirrored shards, nothing to exchange.  With CFS_HIP_FLAG_SHARD_EXCHANGE (or
  // CFS_MULTI_EXCHANGE=reduce_scatter) the shards take the exchange form and one native
  // reduce-scatter per SpMV; CFS_MULTI_EXCHANGE=sparse: the same shards and the packed
  // all-to-all (MultiSym::spmv_exchange, both)
  bool exchange = (o2.flags & CFS_HIP_FLAG_SHARD_EXCHANGE) != 0;
  int first_form = CFS_HIP_EXCHANGE_REDUCE_SCATTER;
  if (const char *e = getenv("CFS_MULTI_EXCHANGE")) {
    exchange = !strcmp(e, "reduce_scatter") || !strcmp(e, "sparse");
    if (!strcmp(e, "sparse")) first_form = CFS_HIP_EXCHANGE_SPARSE;
  }
  if (ngpus < 2) exchange = false;
  if (exchange) o2.flags = (o2.flags | CFS_HIP_FLAG_SHARD_EXCHANGE) & ~(CFS_HIP_FLAG_HYB);
  else o2.flags &= ~CFS_HIP_FLAG_SHARD_EXCHANGE;
  m->shards.reserve(ngpus);
  for (int g = 0; g < ngpus; g++) {
    // devices[g] when given, else the visible devices round-robin (several shards may
    // share a device: that is how a one-GPU box rehearses the path)
    const int d = devices ? devices[g] : (home + g) % std::max(1, ndev);
    if (d < 0 || d >= ndev) return set_err(CFS_HIP_ERR_ARG, "bad device index");
    DeviceGuard dg(d);
    if (d != home && !cfs_rt::enable_peer_access(d, home)) // the shard reads x / writes y on the home device
      return set_err(CFS_HIP_ERR_DEVICE, "device " + std::to_string(d) + " cannot access device " +
                                             std::to_string(home) + " (peer access)");
    // (in the handle before anything of it exists: whatever does is released with the handle)
    m->shards.emplace_back();
    Shard &s = m->shards.back();
    s.dev = d;
    if (hipStreamCreateWithFlags(&s.st, hipStreamNonBlocking) != hipSuccess ||
        hipEventCreateWithFlags(&s.done, hipEventDisableTiming) != hipSuccess)
      return set_err(CFS_HIP_ERR_DEVICE, "stream / event creation failed");
    cfs_hip_sym_t h = nullptr;
    if ((rc = sym_create<V>(n, rowptr, colind, values, ngpus, g, m->splits.data(), &o2, &h))) return fail(rc);
    s.h.reset(h);
  }
  if (exchange) {
    int transport = CFS_HIP_TRANSPORT_AUTO;
    if (const char *e = getenv("CFS_MULTI_TRANSPORT"))
      transport = !strcmp(e, "rccl") ? CFS_HIP_TRANSPORT_RCCL : (!strcmp(e, "peer") ? CFS_HIP_TRANSPORT_PEER : CFS_HIP_TRANSPORT_AUTO);
    if ((rc = m->template setup_exchange<V>(transport, first_form))) return fail(rc);
  }
  *out = m.release();
  return 0;
}
int cfs_hip_sym_create_multi_f64(int n, const int *rowptr, const int *colind, const double *values,
                                 int ngpus, const int *devices, const cfs_hip_options *opt,
                                 cfs_hip_sym_t *out) {
  return sym_create_multi<double>(n, rowptr, colind, values, ngpus, devices, opt, out);
}
int cfs_hip_sym_create_multi_f32(int n, const int *rowptr, const int *colind, const float *values,
                                 int ngpus, const int *devices, const cfs_hip_options *opt,
                                 cfs_hip_sym_t *out) {
  return sym_create_multi<float>(n, rowptr, colind, values, ngpus, devices, opt, out);
}
int cfs_hip_sym_multi_set_xmode(cfs_hip_sym_t h, int xmode) {
  auto *m = dynamic_cast<MultiSym *>(h);
  if (!m) return set_err(CFS_HIP_ERR_ARG, "not a multi-device handle");
  if (xmode != CFS_HIP_XMODE_PEER && xmode != CFS_HIP_XMODE_REPLICATE && xmode != CFS_HIP_XMODE_REPLICATE_ALL)
    return set_err(CFS_HIP_ERR_ARG, "unknown x mode");
  int rc = m->sync_shards(); // pending SpMVs of the other mode finish first
  if (rc) return rc;
  m->xmode = xmode;
  return 0;
}
int cfs_hip_sym_multi_set_exchange(cfs_hip_sym_t h, int form) {
  if (!h) return set_err(CFS_HIP_ERR_ARG, "null handle");
  auto *m = dynamic_cast<MultiSym *>(h);
  if (!m || !m->comm) return set_err(CFS_HIP_ERR_ARG, "not an exchange-form multi-device handle");
  if (form != CFS_HIP_EXCHANGE_REDUCE_SCATTER && form != CFS_HIP_EXCHANGE_SPARSE)
    return set_err(CFS_HIP_ERR_ARG, "unknown exchange form");
  int rc = m->sync_shards(); // pending SpMVs of the other form finish first (the receive side is uploaded below)
  if (!rc) rc = cfs_rt::with_value_type(m->value_bytes, [&](auto v) { return m->ensure_form<decltype(v)>(form); });
  if (rc) return rc;
  m->form = form;
  return 0;
}
int cfs_hip_sym_multi_exchange_info(cfs_hip_sym_t h, int *form, int64_t *values_moved, int64_t *bytes_moved) {
  if (!h) return set_err(CFS_HIP_ERR_ARG, "null handle");
  auto *m = dynamic_cast<MultiSym *>(h);
  if (!m || !m->comm) return set_err(CFS_HIP_ERR_ARG, "not an exchange-form multi-device handle");
  const int64_t N = (int64_t)m->shards.size();
  int64_t v = 0;
  if (m->form == CFS_HIP_EXCHANGE_SPARSE)
    for (const Shard &s : m->shards) v += s.nsend;
  else
    v = N * N * m->rs_rows;
  if (form) *form = m->form;
  if (values_moved) *values_moved = v;
  if (bytes_moved) *bytes_moved = v * m->value_bytes;
  return 0;
}
int cfs_hip_sym_multi_devices(cfs_hip_sym_t h, int *devices, int capacity, int *distinct) {
  auto *m = dynamic_cast<MultiSym *>(h);
  if (!m || !distinct) return set_err(CFS_HIP_ERR_ARG, "not a multi-device handle");
  std::vector<int> seen;
  for (size_t g = 0; g < m->shards.size(); g++) {
    const int d = m->shards[g].dev;
    if (devices && (int)g < capacity) devices[g] = d;
    if (std::find(seen.begin(), seen.end(), d) == seen.end()) seen.push_back(d);
  }
  *distinct = (int)seen.size();
  return 0;
}
int cfs_hip_sym_num_gpus(cfs_hip_sym_t h, int *ngpus) {
  if (!h || !ngpus) return set_err(CFS_HIP_ERR_ARG, "null argument");
  auto *m = dynamic_cast<MultiSym *>(h);
  *ngpus = m ? m->ngpus() : 1;
  return 0;
}
