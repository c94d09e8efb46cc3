// cfs_comm.hpp -- the exchange of the off-block y contributions, native (no Python, no
// torch.distributed): the north-star's reduce-scatter over xGMI behind the C ABI.
//
// The reference has no counterpart (it is a single-process OpenMP code whose only
// exchange is the barrier between colours, csr_matrix.tpp:3018); what is exchanged
// here are its DIRECT CONFLICTS (csr_matrix.tpp:1443-1451): transposed updates
// y_j += a_ij x_i whose row j belongs to another row block.
//
// One process drives N devices (CFS_NUM_GPUS behind the C++ surface):
//   * transport "rccl": one communicator per device (ncclCommInitAll), collectives
//     issued for all ranks between ncclGroupStart / ncclGroupEnd, each on its
//     device's stream.  librccl.so is dlopen'ed at the first use: the library has
//     no link-time dependency on it, and a box without RCCL keeps everything else.
//     RCCL refuses two ranks on one device, so
//   * transport "peer": the same reduce-scatter / all-gather as plain kernels and
//     copies over peer access -- what N shards on ONE device (the test boxes) use,
//     and the fall-back when RCCL cannot be loaded.
// Either way: sum-reduce-scatter of N x count values per rank (rank r receives the
// r-th block), and all-gather of count values per rank.
//
// The SPARSE form of the same exchange is the packed all-to-all (cfs_hip_comm_alltoallv):
// only the one value per remote boundary row that cfs_pack_kernel produces crosses a cut.
// RCCL: grouped ncclSend / ncclRecv (optional entry points, Rccl::p2p_ok); peer: one pull
// kernel per receiving rank (cfs_peer_alltoallv_kernel).
#pragma once

#include <dlfcn.h>

#include <memory>

namespace cfs_comm {

using cfs_rt::DeviceGuard;
using cfs_rt::set_err;

// the few RCCL entry points, resolved at run time (signatures: rccl/rccl.h)
struct Rccl {
  void *lib = nullptr;
  int (*CommInitAll)(void **comms, int ndev, const int *devlist) = nullptr;
  int (*CommDestroy)(void *comm) = nullptr;
  const char *(*GetErrorString)(int) = nullptr;
  int (*GroupStart)() = nullptr;
  int (*GroupEnd)() = nullptr;
  int (*ReduceScatter)(const void *send, void *recv, size_t recvcount, int dtype, int op, void *comm,
                       hipStream_t st) = nullptr;
  int (*AllGather)(const void *send, void *recv, size_t sendcount, int dtype, void *comm, hipStream_t st) = nullptr;
  // optional (the packed all-to-all only): a librccl without them still serves the collectives above
  int (*Send)(const void *send, size_t count, int dtype, int peer, void *comm, hipStream_t st) = nullptr;
  int (*Recv)(void *recv, size_t count, int dtype, int peer, void *comm, hipStream_t st) = nullptr;
  bool ok = false;
  bool p2p_ok = false;
  std::string why;
};
inline Rccl &rccl() {
  static Rccl r;
  static std::once_flag once;
  std::call_once(once, [] {
    // CFS_HIP_RCCL_LIB=<path>: read once, here; replaces the list of library names
    std::vector<std::string> names = {"librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so.1"};
    if (const char *e = getenv("CFS_HIP_RCCL_LIB"))
      if (*e) names.assign(1, e);
    for (const std::string &nm : names)
      if ((r.lib = dlopen(nm.c_str(), RTLD_NOW | RTLD_LOCAL))) break;
    if (!r.lib) {
      const char *why = dlerror(); // (a second call returns NULL: the message is consumed)
      r.why = std::string("librccl.so not loadable: ") + (why ? why : "?");
      return;
    }
    auto sym = [&](const char *n) { return dlsym(r.lib, n); };
    r.CommInitAll = (decltype(r.CommInitAll))sym("ncclCommInitAll");
    r.CommDestroy = (decltype(r.CommDestroy))sym("ncclCommDestroy");
    r.GetErrorString = (decltype(r.GetErrorString))sym("ncclGetErrorString");
    r.GroupStart = (decltype(r.GroupStart))sym("ncclGroupStart");
    r.GroupEnd = (decltype(r.GroupEnd))sym("ncclGroupEnd");
    r.ReduceScatter = (decltype(r.ReduceScatter))sym("ncclReduceScatter");
    r.AllGather = (decltype(r.AllGather))sym("ncclAllGather");
    r.ok = r.CommInitAll && r.CommDestroy && r.GroupStart && r.GroupEnd && r.ReduceScatter && r.AllGather;
    if (!r.ok) r.why = "librccl.so lacks an entry point";
    r.Send = (decltype(r.Send))sym("ncclSend");
    r.Recv = (decltype(r.Recv))sym("ncclRecv");
    r.p2p_ok = r.ok && r.Send && r.Recv;
  });
  return r;
}
constexpr int kNcclSum = 0, kNcclFloat32 = 7, kNcclFloat64 = 8; // rccl.h enumerators

// out[i] = sum over ranks g of in[g][off + i]  (the peer transport's reduce-scatter)
// The table of the ranks' send buffers travels BY VALUE in the kernel-argument segment, like the
// all-to-all's below: it is read from the caller's array before the call returns, and nothing is
// copied from host memory behind the event waits of a stream.
struct SumTable {
  const void *src[cfs_rt::kMaxDevices];
  int nranks;
};
template <typename V>
__global__ void __launch_bounds__(256) cfs_peer_sum_kernel(V *__restrict__ out, const SumTable t, size_t off, size_t count) {
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < count; i += (size_t)gridDim.x * 256) {
    V s = V(0);
    for (int g = 0; g < t.nranks; ++g) s += ((const V *)t.src[g])[off + i]; // fixed order: bit-reproducible
    out[i] = s;
  }
}

// The packed all-to-all of the peer transport, a PULL: rank r gathers the block every source
// rank g holds for it into its own receive buffer, blocks concatenated by source rank.
//   src[g]    = rank g's send buffer advanced to its block for r (NULL where that block is empty)
//   prefix[g] = offset of that block in out; prefix[nranks] = everything r receives
// The table travels BY VALUE in the kernel-argument segment: no per-call copy of a pointer
// table from host memory, nothing that depends on the lifetime of a host vector.
// Ordering (the protocol of the reduce-scatter): r's stream waits for the `ready` event of every
// source it reads, recorded behind that rank's pack, and records `done` behind this kernel;
// cfs_hip_comm_wait_consumed makes a rank wait for every `done` before it overwrites its send
// buffer.  The receive buffer needs no event: only this kernel writes it and only r's own
// recv_fold reads it, both on r's stream, so a call runs behind the previous round's fold.
struct A2aTable {
  const void *src[cfs_rt::kMaxDevices];
  long long prefix[cfs_rt::kMaxDevices + 1];
  int nranks;
};
template <typename V>
__global__ void __launch_bounds__(256) cfs_peer_alltoallv_kernel(V *__restrict__ out, const A2aTable t) {
  const long long total = t.prefix[t.nranks];
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
    int lo = 0, hi = t.nranks; // the last g with prefix[g] <= i: its block is not empty
    while (hi - lo > 1) {
      const int mid = (lo + hi) >> 1;
      if (t.prefix[mid] <= i) lo = mid;
      else hi = mid;
    }
    out[i] = ((const V *)t.src[lo])[i - t.prefix[lo]];
  }
}

} // namespace cfs_comm

struct cfs_hip_comm_s {
  std::vector<int> dev;
  std::vector<void *> comm;      // RCCL communicators (transport rccl)
  bool use_rccl = false;
  std::string note;              // why the peer transport is in use
  std::vector<hipEvent_t> ready, done; // peer transport: send buffer written / block summed
  std::vector<hipEvent_t> entered;     // peer all-gather: what rank r enqueued before the call is behind it
  bool done_valid = false;
  ~cfs_hip_comm_s() {
    for (size_t g = 0; g < dev.size(); g++) {
      cfs_rt::DeviceGuard dg(dev[g]);
      if (use_rccl && g < comm.size() && comm[g]) (void)cfs_comm::rccl().CommDestroy(comm[g]);
      if (g < ready.size() && ready[g]) (void)hipEventDestroy(ready[g]);
      if (g < done.size() && done[g]) (void)hipEventDestroy(done[g]);
      if (g < entered.size() && entered[g]) (void)hipEventDestroy(entered[g]);
    }
  }
};

// ---------------------------------------------------------------------------
// cfs_hip_comm_* (declared extern "C" in cfs_hip.h): RCCL over xGMI, or kernels / copies over
// peer access
// ---------------------------------------------------------------------------
using cfs_rt::DeviceGuard;
using cfs_rt::set_err;

int cfs_hip_comm_create(int ndev, const int *devices, int transport, cfs_hip_comm_t *out) {
  if (!out || ndev < 1 || ndev > cfs_rt::kMaxDevices) return set_err(CFS_HIP_ERR_ARG, "bad argument");
  *out = nullptr;
  int rc = cfs_rt::ensure_home();
  if (rc) return rc;
  int visible = 0, cur = 0;
  HIPCHK(hipGetDeviceCount(&visible));
  HIPCHK(hipGetDevice(&cur));
  std::unique_ptr<cfs_hip_comm_s> c(new cfs_hip_comm_s());
  bool distinct = true;
  for (int g = 0; g < ndev; g++) {
    const int d = devices ? devices[g] : (cur + g) % std::max(1, visible);
    if (d < 0 || d >= visible) return set_err(CFS_HIP_ERR_ARG, "bad device index");
    for (int q : c->dev) distinct = distinct && q != d;
    c->dev.push_back(d);
  }
  cfs_comm::Rccl &R = cfs_comm::rccl();
  if (transport == CFS_HIP_TRANSPORT_RCCL && (!distinct || !R.ok))
    return set_err(CFS_HIP_ERR_UNSUPPORTED, "rccl transport: " + (!distinct ? "RCCL needs one rank per device" : R.why));
  c->use_rccl = transport != CFS_HIP_TRANSPORT_PEER && distinct && R.ok;
  if (!c->use_rccl) c->note = transport == CFS_HIP_TRANSPORT_PEER ? "asked for" : (!distinct ? "ranks share a device" : R.why);
  if (c->use_rccl) {
    c->comm.assign(ndev, nullptr);
    const int r2 = R.CommInitAll(c->comm.data(), ndev, c->dev.data());
    if (r2 != 0) {
      c->use_rccl = false; // (nothing to destroy)
      return set_err(CFS_HIP_ERR_DEVICE, std::string("ncclCommInitAll: ") + (R.GetErrorString ? R.GetErrorString(r2) : "?"));
    }
  } else {
    c->ready.assign(ndev, nullptr);
    c->done.assign(ndev, nullptr);
    c->entered.assign(ndev, nullptr);
    for (int g = 0; g < ndev; g++) {
      DeviceGuard dg(c->dev[g]);
      for (int q = 0; q < ndev; q++) // every rank reads every other rank's buffers
        if (c->dev[q] != c->dev[g] && !cfs_rt::enable_peer_access(c->dev[g], c->dev[q]))
          return set_err(CFS_HIP_ERR_DEVICE, "peer access between the devices of the communicator is not available");
      if (hipEventCreateWithFlags(&c->ready[g], hipEventDisableTiming) != hipSuccess ||
          hipEventCreateWithFlags(&c->done[g], hipEventDisableTiming) != hipSuccess ||
          hipEventCreateWithFlags(&c->entered[g], hipEventDisableTiming) != hipSuccess)
        return set_err(CFS_HIP_ERR_DEVICE, "event creation failed");
    }
  }
  *out = c.release();
  return 0;
}
int cfs_hip_comm_info(cfs_hip_comm_t c, int *ndev, int *transport) {
  if (!c) return set_err(CFS_HIP_ERR_ARG, "null communicator");
  if (ndev) *ndev = (int)c->dev.size();
  if (transport) *transport = c->use_rccl ? CFS_HIP_TRANSPORT_RCCL : CFS_HIP_TRANSPORT_PEER;
  return 0;
}
int cfs_hip_comm_destroy(cfs_hip_comm_t comm) {
  delete comm;
  return 0;
}
// make `stream` (of rank `rank`) wait until the previous collective has consumed that rank's
// send buffer (peer transport: other ranks' kernels read it; RCCL orders on the stream itself)
int cfs_hip_comm_wait_consumed(cfs_hip_comm_t c, int rank, void *stream) {
  if (!c || rank < 0 || rank >= (int)c->dev.size()) return set_err(CFS_HIP_ERR_ARG, "bad argument");
  if (c->use_rccl || !c->done_valid) return 0;
  DeviceGuard dg(c->dev[rank]);
  for (size_t r = 0; r < c->dev.size(); r++) HIPCHK(hipStreamWaitEvent((hipStream_t)stream, c->done[r], 0));
  return 0;
}
int cfs_hip_comm_reduce_scatter(cfs_hip_comm_t c, void *const *send, void *const *recv, size_t count,
                                int value_bytes, void *const *streams) {
  if (!c || !send || !recv || !streams || (value_bytes != 4 && value_bytes != 8))
    return set_err(CFS_HIP_ERR_ARG, "bad argument");
  const int N = (int)c->dev.size();
  if (c->use_rccl) {
    cfs_comm::Rccl &R = cfs_comm::rccl();
    int r2 = R.GroupStart();
    for (int g = 0; g < N && r2 == 0; g++) {
      DeviceGuard dg(c->dev[g]);
      r2 = R.ReduceScatter(send[g], recv[g], count, value_bytes == 8 ? cfs_comm::kNcclFloat64 : cfs_comm::kNcclFloat32,
                           cfs_comm::kNcclSum, c->comm[g], (hipStream_t)streams[g]);
    }
    const int r3 = R.GroupEnd();
    if (r2 == 0) r2 = r3;
    if (r2 != 0) return set_err(CFS_HIP_ERR_DEVICE, std::string("ncclReduceScatter: ") + (R.GetErrorString ? R.GetErrorString(r2) : "?"));
    return 0;
  }
  // peer transport: rank r sums the r-th block of every rank's send buffer
  for (int g = 0; g < N; g++) {
    DeviceGuard dg(c->dev[g]);
    HIPCHK(hipEventRecord(c->ready[g], (hipStream_t)streams[g]));
  }
  // (the table of send buffers goes to the kernels by value: read here, before the call returns)
  cfs_comm::SumTable t;
  memset(&t, 0, sizeof t);
  t.nranks = N;
  for (int g = 0; g < N; g++) t.src[g] = send[g];
  for (int r = 0; r < N; r++) {
    DeviceGuard dg(c->dev[r]);
    hipStream_t st = (hipStream_t)streams[r];
    for (int g = 0; g < N; g++) HIPCHK(hipStreamWaitEvent(st, c->ready[g], 0));
    const int grid = (int)std::min<size_t>((count + 255) / 256, 2048);
    if (count) {
      if (value_bytes == 8)
        hipLaunchKernelGGL((cfs_comm::cfs_peer_sum_kernel<double>), dim3(grid), dim3(256), 0, st, (double *)recv[r], t,
                           (size_t)r * count, count);
      else
        hipLaunchKernelGGL((cfs_comm::cfs_peer_sum_kernel<float>), dim3(grid), dim3(256), 0, st, (float *)recv[r], t,
                           (size_t)r * count, count);
    }
    HIPCHK(hipEventRecord(c->done[r], st));
  }
  c->done_valid = true;
  HIPCHK(hipGetLastError());
  return 0;
}
int cfs_hip_comm_allgather(cfs_hip_comm_t c, void *const *send, void *const *recv, size_t count,
                           int value_bytes, void *const *streams) {
  if (!c || !send || !recv || !streams || (value_bytes != 4 && value_bytes != 8))
    return set_err(CFS_HIP_ERR_ARG, "bad argument");
  const int N = (int)c->dev.size();
  if (c->use_rccl) {
    cfs_comm::Rccl &R = cfs_comm::rccl();
    int r2 = R.GroupStart();
    for (int g = 0; g < N && r2 == 0; g++) {
      DeviceGuard dg(c->dev[g]);
      r2 = R.AllGather(send[g], recv[g], count, value_bytes == 8 ? cfs_comm::kNcclFloat64 : cfs_comm::kNcclFloat32,
                       c->comm[g], (hipStream_t)streams[g]);
    }
    const int r3 = R.GroupEnd();
    if (r2 == 0) r2 = r3;
    if (r2 != 0) return set_err(CFS_HIP_ERR_DEVICE, std::string("ncclAllGather: ") + (R.GetErrorString ? R.GetErrorString(r2) : "?"));
    return 0;
  }
  // peer transport: rank g pushes its block into every rank's receive buffer -- behind what rank r
  // had enqueued on its own stream when the call was made (`entered[r]`): r may still be reading
  // recv[r] of the round before
  const size_t bytes = count * (size_t)value_bytes;
  for (int r = 0; r < N; r++) {
    DeviceGuard dg(c->dev[r]);
    HIPCHK(hipEventRecord(c->entered[r], (hipStream_t)streams[r]));
  }
  for (int g = 0; g < N; g++) {
    DeviceGuard dg(c->dev[g]);
    hipStream_t st = (hipStream_t)streams[g];
    for (int r = 0; r < N && bytes; r++)
      if (r != g) HIPCHK(hipStreamWaitEvent(st, c->entered[r], 0));
    for (int r = 0; r < N && bytes; r++)
      HIPCHK(hipMemcpyPeerAsync((char *)recv[r] + (size_t)g * bytes, c->dev[r], send[g], c->dev[g], bytes, st));
    HIPCHK(hipEventRecord(c->ready[g], st));
  }
  for (int r = 0; r < N; r++) {
    DeviceGuard dg(c->dev[r]);
    for (int g = 0; g < N; g++) HIPCHK(hipStreamWaitEvent((hipStream_t)streams[r], c->ready[g], 0));
  }
  return 0;
}
// the packed all-to-all: counts[g * N + r] values go from rank g (its blocks for r = 0..N-1 back
// to back in send[g]) to rank r (the blocks from g = 0..N-1 back to back in recv[r])
int cfs_hip_comm_alltoallv(cfs_hip_comm_t c, void *const *send, void *const *recv, const int64_t *counts,
                           int value_bytes, void *const *streams) {
  if (!c || !send || !recv || !counts || !streams || (value_bytes != 4 && value_bytes != 8))
    return set_err(CFS_HIP_ERR_ARG, "bad argument");
  const int N = (int)c->dev.size();
  for (int g = 0; g < N; g++) {
    int64_t out = 0, in = 0;
    for (int r = 0; r < N; r++) {
      if (counts[(size_t)g * N + r] < 0) return set_err(CFS_HIP_ERR_ARG, "alltoallv: negative count");
      out += counts[(size_t)g * N + r];
      in += counts[(size_t)r * N + g];
    }
    if ((out && !send[g]) || (in && !recv[g])) return set_err(CFS_HIP_ERR_ARG, "alltoallv: null buffer of a rank that moves values");
  }
  if (c->use_rccl) {
    cfs_comm::Rccl &R = cfs_comm::rccl();
    if (!R.p2p_ok)
      return set_err(CFS_HIP_ERR_UNSUPPORTED, "alltoallv: librccl.so lacks ncclSend / ncclRecv (use the peer transport)");
    const int dt = value_bytes == 8 ? cfs_comm::kNcclFloat64 : cfs_comm::kNcclFloat32;
    int r2 = R.GroupStart();
    for (int g = 0; g < N && r2 == 0; g++) {
      DeviceGuard dg(c->dev[g]);
      hipStream_t st = (hipStream_t)streams[g];
      size_t soff = 0, roff = 0;
      for (int r = 0; r < N && r2 == 0; r++) {
        const size_t k = (size_t)counts[(size_t)g * N + r];
        if (k) r2 = R.Send((const char *)send[g] + soff * value_bytes, k, dt, r, c->comm[g], st);
        soff += k;
      }
      for (int s = 0; s < N && r2 == 0; s++) {
        const size_t k = (size_t)counts[(size_t)s * N + g];
        if (k) r2 = R.Recv((char *)recv[g] + roff * value_bytes, k, dt, s, c->comm[g], st);
        roff += k;
      }
    }
    const int r3 = R.GroupEnd();
    if (r2 == 0) r2 = r3;
    if (r2 != 0) return set_err(CFS_HIP_ERR_DEVICE, std::string("ncclSend / ncclRecv: ") + (R.GetErrorString ? R.GetErrorString(r2) : "?"));
    return 0;
  }
  // peer transport: rank r pulls its blocks with one launch (cfs_peer_alltoallv_kernel)
  for (int g = 0; g < N; g++) {
    DeviceGuard dg(c->dev[g]);
    HIPCHK(hipEventRecord(c->ready[g], (hipStream_t)streams[g]));
  }
  for (int r = 0; r < N; r++) {
    DeviceGuard dg(c->dev[r]);
    hipStream_t st = (hipStream_t)streams[r];
    cfs_comm::A2aTable t;
    memset(&t, 0, sizeof t);
    t.nranks = N;
    for (int g = 0; g < N; g++) {
      size_t soff = 0; // where rank g's block for r starts in send[g]
      for (int q = 0; q < r; q++) soff += (size_t)counts[(size_t)g * N + q];
      const int64_t k = counts[(size_t)g * N + r];
      t.src[g] = k ? (const char *)send[g] + soff * value_bytes : nullptr;
      t.prefix[g + 1] = t.prefix[g] + k;
      if (k) HIPCHK(hipStreamWaitEvent(st, c->ready[g], 0)); // (only the sources this rank reads)
    }
    const int64_t total = t.prefix[N];
    if (total) {
      const int grid = (int)std::min<int64_t>((total + 255) / 256, 2048);
      if (value_bytes == 8)
        hipLaunchKernelGGL((cfs_comm::cfs_peer_alltoallv_kernel<double>), dim3(grid), dim3(256), 0, st, (double *)recv[r], t);
      else
        hipLaunchKernelGGL((cfs_comm::cfs_peer_alltoallv_kernel<float>), dim3(grid), dim3(256), 0, st, (float *)recv[r], t);
    }
    HIPCHK(hipEventRecord(c->done[r], st));
  }
  c->done_valid = true;
  HIPCHK(hipGetLastError());
  return 0;
}
