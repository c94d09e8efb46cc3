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
